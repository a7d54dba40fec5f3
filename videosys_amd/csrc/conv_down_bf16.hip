// Stride-2 implicit-GEMM convolution on bf16 MFMA for the VAE ENCODERS: the two downsampling layers of the Open-Sora-Plan v1.2
// CausalVAE (autoencoder_kl_open_sora_plan_v120.py: Downsample :430-464, Spatial2xTime2x3DDownsample :418-427 over CausalConv3d
// :40-113).  Channels-last activations, fp32 accumulation on v_mfma_f32_16x16x32_bf16, bias + bf16 output.
//
//   spatial mode (kt = 1)          out[n, t, ho, wo] = b + sum_{kh, kw, c} x[n, t, 2 ho + kh, 2 wo + kw, c] w[., (kh 3 + kw) cin + c]
//   spatio-temporal mode (kt = 3)  out[n, t', ho, wo] = b + sum_{a, kh, kw, c} x[n, max(2 t' + a - 2, 0), 2 ho + kh, 2 wo + kw, c] w[...]
//
// with x = 0 for row index H and column index W: ONE implicit zero row below and ONE zero column to the right, none above or to the
// left (F.pad (0, 1, 0, 1)); Ho = H / 2, Wo = W / 2 rounded down, so with an odd H (W) the zero row (column) is never reached and the last
// source row (column) is read by the last output row (column) as its third tap — what F.pad + Conv2d(stride 2) gives.  In time the
// two frames in front are COPIES OF THE FIRST FRAME (CausalConv3d.forward :94-97), not zeros: output frame 0 reads frame 0 three
// times, output frame t' >= 1 reads frames 2 t' - 2 .. 2 t'; To = (T - 1) / 2 + 1 (T = 1 and T = 2 give one frame, an even T leaves
// its last frame unread).
//
// The tile engine — split, geometry, staging pipeline, padding by clamped address + zeroed fragment, epilogue — is conv_tile16.h.
// Particular to this kernel:
//   * reference tap (0, 0, 0); the map rises with the voxel index except at one place: in the causal mode output frames 0 and 1 both
//     start at source frame 0, so a tile that begins inside output frame 0 and reaches output frame 1 has its lowest row at the first
//     voxel of the sample, not at its own first voxel.  A tap is the row shift a plane_pitch + kh row_pitch + kw rows;
//   * bottom row / right column (2 ho + 2 >= H with kh = 2, 2 wo + 2 >= W with kw = 2): the address is clamped to the neighbouring tap
//     (kh = 1 / kw = 1, always inside the voxels of the grid) and the fragment zeroed;
//   * first output frame (kt = 3, t' = 0): the temporal shift is dropped, every a reads frame 0.
//
// Refused before any launch (launch_conv_down2): VSYS_ERR_SHAPE for kt not 1 or 3, cout % 128, cin % 32, what ct16::refuse_grid
// refuses, and a tile whose source span — 256 consecutive output voxels with their
// taps: 2 * 255 + ceil(255 / Wo) * 2 row_pitch + ceil(255 / (Ho Wo)) * (2 or 1) plane_pitch + the last tap's shift, in rows of ldx
// elements (a tile that wraps from output frame 0 to 1 spans less than one plane_pitch plus that shift, which the bound covers) — or
// whose weight panel reaches 2 GiB (tile-relative offsets are 32-bit); VSYS_ERR_ALIGN as ct16::refuse_align.
#include "conv_tile16.h"

namespace vsys {
namespace {

using namespace ct16;

__global__ __launch_bounds__(256, 2) void conv_down2_kernel(ConvDownParams p) {
#if __HIP_DEVICE_COMPILE__  // buffer-resource types exist in the device pass only
  __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];   // static: the code object carries the figure
  const Tile tl = make_tile(p.N, p.ldw);
  const int row0 = tl.row0;

  // output voxel r of the sample -> source row of its tap (0, 0, 0) inside the sample; flags: 1 first output frame of the causal mode,
  // 2 bottom output row whose kh = 2 tap is the zero row, 4 right output column whose kw = 2 tap is the zero column
  const int HoWo = p.Ho * p.Wo;
  auto src_of = [&](int r, int& flags) -> int {
    const int t = r / HoWo, rem = r - t * HoWo;
    const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
    const int tb = p.kt == 3 ? (t > 0 ? 2 * t - 2 : 0) : t;
    flags = (p.kt == 3 && t == 0 ? 1 : 0) | (2 * ho + 2 >= p.H ? 2 : 0) | (2 * wo + 2 >= p.Wd ? 4 : 0);
    return p.row00 + tb * p.plane + 2 * ho * p.Wp + 2 * wo;
  };
  // the tile's lowest source row: its first voxel's (row0 < M: the grid has ceil(M / BM) row tiles), or the sample's first voxel when
  // the tile runs from output frame 0 into output frame 1 of the causal mode, which starts at source frame 0 again
  int f_unused;
  const bool wraps = p.kt == 3 && row0 < HoWo && HoWo < (row0 + BM < p.M ? row0 + BM : p.M);
  const int base_row = __builtin_amdgcn_readfirstlane(wraps ? p.row00 : src_of(row0, f_unused));

  const int ldx2 = (int)p.ldx * 2;
  const int hstep = p.Wp * ldx2, tstep = p.plane * ldx2;
  int a_off[4], a_flags[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) a_off[i] = (src_of(tl.dma_voxel(i, p.M), a_flags[i]) - base_row) * ldx2 + tl.dchunk;
  // edges: bottom (kh = 2), right (kw = 2)
  const auto mask = frag_masks<2>(tl, p.M, [&](int r) { int f; (void)src_of(r, f); return f; });

  const auto rsrc_a = rows_rsrc(p.X, tl.zb * p.sample_rows + base_row, p.rows_total, p.ldx, p.cin);
  const auto rsrc_b = rows_rsrc(p.W, tl.col0, p.N, p.ldw, p.K);
  // byte offset of this lane's source row for tap (a, b, c) of DMA group i: the tile-wide row shift, clamped where the tap leaves the grid
  auto a_voff = [&](int i, int a, int b, int c) -> int {
    const int f = a_flags[i];
    const int hb = (b == 2 && (f & 2)) ? 1 : b;
    const int wc = (c == 2 && (f & 4)) ? 1 : c;
    return a_off[i] + ((f & 1) ? 0 : a * tstep) + hb * hstep + wc * ldx2;
  };

  f32x4 acc16[8][4];
  zero_acc(acc16);
  k_loop(smem, tl, rsrc_a, rsrc_b, p.K / BK, p.nkc, a_voff, [&](int b, int c) { return (b == 2 ? mask.m[0] : 0) | (c == 2 ? mask.m[1] : 0); },
         acc16);
  store_tile_bf16(smem, tl, acc16, p.bias, p.out, p.ldo, p.M, NoHook());
#endif
}

}  // namespace

int launch_conv_down2(const bf16_t* x, int64_t ldx, const VaeGrid& g, int64_t nsamples, const bf16_t* w, int64_t ldw, const bf16_t* bias,
                      bf16_t* out, int64_t ldo, int64_t cin, int64_t cout, int kt, hipStream_t stream) {
  if (kt != 1 && kt != 3) return VSYS_ERR_SHAPE;
  SrcGrid s;
  if (int e = refuse_grid(g, nsamples, s)) return e;
  if (cout <= 0 || cout % BN != 0 || cin <= 0 || cin % BK != 0 || cin > (1 << 20) || cout > (1 << 20)) return VSYS_ERR_SHAPE;
  if (nsamples == 0) return 0;
  const int64_t To = kt == 3 ? (g.T - 1) / 2 + 1 : g.T, Ho = g.H / 2, Wo = g.W / 2;
  const int64_t K = 9 * kt * cin;
  if (ldx < cin || ldo < cout || ldw < K) return VSYS_ERR_SHAPE;
  if (int e = refuse_align(x, ldx, w, ldw, bias, out, ldo)) return e;
  // tile-relative operand offsets are 32-bit (buffer addressing): the widest source span of BM consecutive output voxels and their taps
  const int64_t q = BM - 1;
  const int64_t span = 2 * q + (q + Wo - 1) / Wo * 2 * s.Wp + (q + Ho * Wo - 1) / (Ho * Wo) * (kt == 3 ? 2 : 1) * s.plane +
                       (kt - 1) * s.plane + 2 * s.Wp + 2;
  if ((span + 1) * ldx * 2 >= 0x7fffffff || ldw * 256 + K * 2 >= 0x7fffffff) return VSYS_ERR_SHAPE;
  const int64_t M = To * Ho * Wo;
  const int64_t nbm = (M + BM - 1) / BM, nbn = cout / BN;
  if (M > 0x7fffffff || nbm * nbn > 0x7fffffff) return VSYS_ERR_SHAPE;
  ConvDownParams p;
  p.X = x; p.ldx = ldx; p.sample_rows = g.sample_rows; p.rows_total = nsamples * g.sample_rows;
  p.W = w; p.ldw = ldw; p.bias = bias; p.out = out; p.ldo = ldo;
  p.M = (int)M; p.N = (int)cout; p.K = (int)K; p.cin = (int)cin; p.nkc = (int)(cin / BK); p.kt = kt;
  p.H = g.H; p.Wd = g.W; p.Ho = (int)Ho; p.Wo = (int)Wo; p.Wp = (int)s.Wp; p.plane = (int)s.plane;
  p.row00 = (int)s.row00;
  hipLaunchKernelGGL(conv_down2_kernel, dim3((unsigned)(nbm * nbn), (unsigned)nsamples), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

}  // namespace vsys
