// Time-stride-2 causal implicit-GEMM convolution on bf16 MFMA for the Open-Sora v1.2 VAE ENCODER: the two stride-(2, 1, 1) CausalConv3d
// layers of VAE_Temporal's Encoder (autoencoder_kl_open_sora.py:107-125 CausalConv3d, :229-236 the conv_blocks of the encoder) in ONE
// launch each.  CausalConv3d pads kt - 1 = 2 ZERO frames in front; with a time stride of 2 over an even T only ONE of them is ever
// reached.  Channels-last activations, cin channels in, cout out, To = T / 2 frames (rounded down: an odd T leaves its last frame
// unread) of the same H x W:
//
//   f(t', a)             = 2 t' + a - 1                                                    source frame of temporal tap a
//   out[n, t', h, w, o]  = bf16(bias[o] + sum_{a, kh, kw, c} x[n, f(t', a), h + kh - 1, w + kw - 1, c] w[o, ((a 3 + kh) 3 + kw) cin + c])
//
// with x = 0 for frame -1 and outside 0..H-1 / 0..W-1; fp32 accumulation, one rounding.  This is NOT conv_time_down2_kernel's
// convention (two COPIES of the first frame, f = max(2 t' + a - 2, 0), To = (T - 1) / 2 + 1): here the front of the clip is padding.
//
// The tile engine — split, geometry, staging pipeline, padding by clamped address + zeroed fragment, epilogue — is conv_tile16.h.
// Particular to this kernel:
//   * reference tap: the CENTRE tap of time tap 1, (2 t', h, w), which is a voxel for every output.  The map output voxel -> reference
//     row RISES STRICTLY with the voxel index (an output row adds a row pitch, an output frame two plane pitches), so a tile of 256
//     consecutive output voxels that straddles output frames — and with them source frame pairs — needs no special case: its lowest
//     source row is its first voxel's tap (0, 0, 0), one plane pitch, one row pitch and one row below that voxel's reference row, and
//     never below the sample's first voxel (where a tile that starts in output frame 0 has it: its frame -1 taps read frame 0).  A tap
//     is the tile-wide row shift (a - 1) plane_pitch + (kh - 1) row_pitch + (kw - 1) rows;
//   * THE ZERO FRONT FRAME is a padding case of its own, in time: tap a = 0 of output frame 0 is frame -1.  Its address drops the
//     temporal shift (frame 0 at the same (h, w), itself clamped in space as below) and its fragment is zeroed under a time bit of the
//     pad mask, which holds for the first 9 cin / 32 k-tiles (a = 0) and on the token blocks whose voxel lies in output frame 0.  No
//     zero frame is stored or multiplied;
//   * all four spatial edges pad from the addressing (kh = 0 at h = 0, kh = 2 at h = H - 1, kw = 0 at w = 0, kw = 2 at w = W - 1): the
//     address is clamped to the centre tap (kh = 1 / kw = 1) and the fragment zeroed.
// k_loop hands its pad-mask hook the (kh, kw) of the k-tile it multiplies and calls it once a k-tile, in k order; the time tap is
// counted here, in the hook's own state (k-tiles of a = 0 left).
// 65536 bytes of static LDS, at most 256 VGPRs, no scratch: pinned by tests/test_build_resources_conv_causal_tdown.py.
//
// Refused before any launch (launch_conv_causal_tdown2): VSYS_ERR_SHAPE for what ct16::refuse_grid refuses, T < 2, cout % 128, cin % 32,
// rows narrower than their channels, a tile whose source span or a weight panel that reaches 2 GiB (tile-relative offsets are 32-bit);
// VSYS_ERR_ALIGN as ct16::refuse_align.  nsamples == 0 passes every check and launches nothing.
#include "conv_tile16.h"

namespace vsys {
namespace {

using namespace ct16;

// bit 0 is frag_masks' spare; bits 1..5 become its m[0..4]
enum : int { F_TOP = 2, F_BOTTOM = 4, F_LEFT = 8, F_RIGHT = 16, F_FRONT = 32 };

// output voxel r of the sample -> source row of (2 t', h, w) inside the sample; flags: the four edges, and output frame 0 (whose time tap 0
// is the zero front frame)
__device__ __forceinline__ int src_of(const ConvDownParams& p, int r, int& flags) {
  const int HW = p.H * p.Wd;
  const int t = r / HW, rem = r - t * HW;
  const int h = rem / p.Wd, w = rem - h * p.Wd;
  flags = (h == 0 ? F_TOP : 0) | (h == p.H - 1 ? F_BOTTOM : 0) | (w == 0 ? F_LEFT : 0) | (w == p.Wd - 1 ? F_RIGHT : 0) | (t == 0 ? F_FRONT : 0);
  return p.row00 + 2 * t * p.plane + h * p.Wp + w;
}

__global__ __launch_bounds__(256, 2) void conv_causal_tdown2_kernel(ConvDownParams p) {
#if __HIP_DEVICE_COMPILE__  // buffer-resource types exist in the device pass only
  __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];   // static: the code object carries the figure
  const Tile tl = make_tile(p.N, p.ldw);

  // the tile's lowest source row: tap (0, 0, 0) of its first voxel (row0 < M: the grid has ceil(M / BM) row tiles), not below the sample's
  // first voxel.  Every later voxel of the tile has a higher reference row, whichever output frame it lies in.
  int f_unused;
  const int low = src_of(p, tl.row0, f_unused) - p.plane - p.Wp - 1;
  const int base_row = __builtin_amdgcn_readfirstlane(low < p.row00 ? p.row00 : low);

  const int ldx2 = (int)p.ldx * 2;
  const int hstep = p.Wp * ldx2, tstep = p.plane * ldx2;
  // per DMA group: the reference row's offset and the five shifts a tap may add, each already 0 where the tap is clamped (the edges, the
  // front frame) — plain integers a lane, so no lane mask is carried through the loop.  Time tap 2 (frame 2 t' + 1 <= T - 1) always exists.
  int a_off[4], d_bk[4], d_up[4], d_dn[4], d_lf[4], d_rt[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int f;
    a_off[i] = (src_of(p, tl.dma_voxel(i, p.M), f) - base_row) * ldx2 + tl.dchunk;
    d_bk[i] = (f & F_FRONT) ? 0 : -tstep;
    d_up[i] = (f & F_TOP) ? 0 : -hstep;
    d_dn[i] = (f & F_BOTTOM) ? 0 : hstep;
    d_lf[i] = (f & F_LEFT) ? 0 : -ldx2;
    d_rt[i] = (f & F_RIGHT) ? 0 : ldx2;
  }
  // m[0..3]: top (kh = 0), bottom (kh = 2), left (kw = 0), right (kw = 2); m[4]: output frame 0 (time tap 0)
  const auto mask = frag_masks<5>(tl, p.M, [&](int r) { int f; (void)src_of(p, r, f); return f; });

  const auto rsrc_a = rows_rsrc(p.X, tl.zb * p.sample_rows + base_row, p.rows_total, p.ldx, p.cin);
  const auto rsrc_b = rows_rsrc(p.W, tl.col0, p.N, p.ldw, p.K);
  // byte offset of this lane's source row for tap (a, b, c) of DMA group i: the tile-wide row shift, clamped where the tap leaves the grid
  // (the sum is >= 0: the clamped row is a voxel, and no voxel the tile reads lies below base_row)
  auto a_voff = [&](int i, int a, int b, int c) -> int {
    return a_off[i] + (a == 0 ? d_bk[i] : a == 2 ? tstep : 0) + (b == 0 ? d_up[i] : b == 2 ? d_dn[i] : 0) + (c == 0 ? d_lf[i] : c == 2 ? d_rt[i] : 0);
  };
  int front_left = 9 * p.nkc;   // k-tiles of time tap 0 not multiplied yet: k runs (a, kh, kw, chunk), a outermost
  auto pad_mask = [&](int b, int c) -> int {
    const int zt = front_left > 0 ? mask.m[4] : 0;
    --front_left;
    return zt | (b == 0 ? mask.m[0] : 0) | (b == 2 ? mask.m[1] : 0) | (c == 0 ? mask.m[2] : 0) | (c == 2 ? mask.m[3] : 0);
  };

  f32x4 acc16[8][4];
  zero_acc(acc16);
  k_loop(smem, tl, rsrc_a, rsrc_b, p.K / BK, p.nkc, a_voff, pad_mask, acc16);   // 27 cin / 32 >= 27 k-tiles
  store_tile_bf16(smem, tl, acc16, p.bias, p.out, p.ldo, p.M, NoHook());
#endif
}

}  // namespace

int launch_conv_causal_tdown2(const bf16_t* x, int64_t ldx, const VaeGrid& g, int64_t nsamples, const bf16_t* w, int64_t ldw, const bf16_t* bias,
                              bf16_t* out, int64_t ldo, int64_t cin, int64_t cout, hipStream_t stream) {
  SrcGrid s;
  if (int e = refuse_grid(g, nsamples, s)) return e;
  if (g.T < 2) return VSYS_ERR_SHAPE;
  if (cout <= 0 || cout % BN != 0 || cin <= 0 || cin % BK != 0 || cin > (1 << 20) || cout > (1 << 20)) return VSYS_ERR_SHAPE;
  const int64_t To = g.T / 2, HW = (int64_t)g.H * g.W, K = 27 * cin;
  if (ldx < cin || ldo < cout || ldw < K) return VSYS_ERR_SHAPE;
  // tile-relative operand offsets are 32-bit (buffer addressing): the widest source span of BM consecutive output voxels and their taps.
  // Reference rows: one row a voxel, at most a row pitch more per wrapped output row and two plane pitches more per wrapped output frame;
  // taps: a plane pitch, a row pitch and a row below the first reference row (the tile's lowest row) and above the last.
  const int64_t q = BM - 1;
  const int64_t span = q + (q + g.W - 1) / g.W * s.Wp + (q + HW - 1) / HW * 2 * s.plane + 2 * (s.plane + s.Wp + 1);
  if ((span + 1) * ldx * 2 >= 0x7fffffff || ldw * 256 + K * 2 >= 0x7fffffff) return VSYS_ERR_SHAPE;
  const int64_t M = To * HW;
  const int64_t nbm = (M + BM - 1) / BM, nbn = cout / BN;
  if (M > 0x7fffffff || nbm * nbn > 0x7fffffff) return VSYS_ERR_SHAPE;
  if (int e = refuse_align(x, ldx, w, ldw, bias, out, ldo)) return e;
  if (nsamples == 0) return 0;
  ConvDownParams p;
  p.X = x; p.ldx = ldx; p.sample_rows = g.sample_rows; p.rows_total = nsamples * g.sample_rows;
  p.W = w; p.ldw = ldw; p.bias = bias; p.out = out; p.ldo = ldo;
  p.M = (int)M; p.N = (int)cout; p.K = (int)K; p.cin = (int)cin; p.nkc = (int)(cin / BK); p.kt = 3;
  p.H = g.H; p.Wd = g.W; p.Ho = g.H; p.Wo = g.W; p.Wp = (int)s.Wp; p.plane = (int)s.plane;
  p.row00 = (int)s.row00;
  hipLaunchKernelGGL(conv_causal_tdown2_kernel, dim3((unsigned)(nbm * nbn), (unsigned)nsamples), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

}  // namespace vsys
