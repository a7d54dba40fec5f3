// Time-stride-2 implicit-GEMM convolution with a fused pooled residual on bf16 MFMA for the Open-Sora-Plan v1.1 CausalVAE ENCODER:
// TimeDownsampleRes2x (autoencoder_kl_open_sora_plan_v110.py:1557-1575) in ONE launch, and TimeDownsample2x (:1533-1542) as its
// weightless mode.  With x' = x behind two copies of its first frame and alpha = sigmoid(mix_factor) the layer is
//   alpha AvgPool3d((3, 1, 1), stride (2, 1, 1))(x') + (1 - alpha) Conv3d(3 x 3 x 3, stride (2, 1, 1), padding (0, 1, 1))(x')
// Channels-last activations, C channels in and out, To = (T - 1) / 2 + 1 frames of the same H x W (T = 1 and T = 2 give one frame, an
// even T leaves its last frame unread):
//
//   f(t', a)             = max(2 t' + a - 2, 0)                                            source frame of temporal tap a
//   acc[n, t', h, w, o]  = sum_{a, kh, kw, c} x[n, f(t', a), h + kh - 1, w + kw - 1, c] w_s[o, ((a 3 + kh) 3 + kw) C + c]      fp32
//   out[n, t', h, w, o]  = bf16(fma(a3, (x0 + x1) + x2, acc + bias_s[o])),   x_a = x[n, f(t', a), h, w, o]     fp32, ONE rounding
//
// with x = 0 outside 0..H-1 / 0..W-1 (one zero row and column on EVERY side).  The caller folds (1 - alpha) into w_s and bias_s (scaled in
// fp32, then their one rounding to bf16, as the decoder's TimeUpsampleRes2x does) and passes a3 = fp32(alpha / 3).
//   w == NULL: TimeDownsample2x, out = bf16(((x0 + x1) + x2) * fp32(1 / 3)): no matrix work, the bandwidth kernel at the end of the file.
//
// The tile engine — split, geometry, staging pipeline, padding by clamped address + zeroed fragment, epilogue — is conv_tile16.h.
// Particular to this kernel:
//   * reference tap: the CENTRE tap in time tap 0, (f(t', 0), h, w).  A tap is the tile-wide row shift a plane_pitch + (kh - 1) row_pitch +
//     (kw - 1) rows.  The map rises with the voxel index — a tile crosses output frames, each of which jumps TWO source planes — except
//     at one place: output frames 0 and 1 both start at source frame 0, so a tile that begins in output frame 0 and reaches frame 1 has
//     its lowest row at the sample's first voxel.  Every other tile's lowest row is one row pitch and one row below its first voxel's
//     centre (its tap (., 0, 0)), but never below the sample's first voxel;
//   * ALL FOUR spatial edges pad from the addressing (kh = 0 at h = 0, kh = 2 at h = H - 1, kw = 0 at w = 0, kw = 2 at w = W - 1): the
//     address is clamped to the centre tap (kh = 1 / kw = 1, always a voxel) and the fragment zeroed.  On output frame 0 the temporal
//     shift is dropped: every a reads frame 0;
//   * the pooled residual is no separate pass: in the epilogue (its hook) the lane that owns (voxel, column quad) of the accumulator tile
//     FETCHES the three source values itself — three 8-byte loads of rows whose 128-column segment is the centre-tap k-tiles the main
//     loop of this very tile pulled through L2.  Keeping them from the staged A image was the alternative and is not taken: the image
//     of a k-tile holds 32 channels of ONE tap for 256 voxels, the residual columns of a tile are 128 channels of THREE taps, which pass
//     through the three A slots at 12 different k-tiles; holding them would take 3 x 256 x 128 x 2 = 192 KiB of LDS, more than a CU has,
//     or 48 more registers a lane beside 128 accumulators.  The fetch costs 96 8-byte L2 hits per lane after 27 C / 32 k-tiles of 32
//     MFMAs.  The adds stay single fp32 operations (no packed fp32: conv_tile16.h) and the a3 multiply-add is an explicit fma.
// 65536 bytes of static LDS, at most 222 VGPRs, no scratch: pinned by tests/test_build_resources_conv_time_down.py.
//
// Refused before any launch (launch_conv_time_down2): VSYS_ERR_SHAPE for C % 128 with weights or C % 8 without, what ct16::refuse_grid
// refuses, a tile whose source span or a weight panel that reaches 2 GiB (tile-relative offsets are 32-bit); VSYS_ERR_ALIGN as
// ct16::refuse_align; VSYS_ERR_ARG for a3 outside [0, fp32(1 / 3)].
#include "conv_tile16.h"

namespace vsys {
namespace {

using namespace ct16;

struct TimeDownParams {
  const bf16_t* X = nullptr; int64_t ldx = 0;   // source rows over the grid, [*, >= C]
  int64_t sample_rows = 0, rows_total = 0;      // rows per sample / of the whole operand
  const bf16_t* W = nullptr; int64_t ldw = 0;   // [C, 27 C], k = tap * C + channel
  const bf16_t* bias = nullptr;                 // [C] or null
  bf16_t* out = nullptr; int64_t ldo = 0;       // dense rows [samples * M, C]
  int M = 0, C = 0, K = 0, nkc = 0;             // M = To * H * W output voxels per sample; nkc = C / 32
  int To = 0, H = 0, Wd = 0;
  int Wp = 0, plane = 0, row00 = 0;             // source row pitch, plane pitch, row of voxel (0, 0, 0) inside a sample
  float a3 = 0.f;                               // alpha / 3
};

enum : int { F_FIRST = 1, F_TOP = 2, F_BOTTOM = 4, F_LEFT = 8, F_RIGHT = 16 };

// output voxel r of the sample -> source row of (f(t', 0), h, w) inside the sample; flags: first output frame, and the four edges
__device__ __forceinline__ int src_of(const TimeDownParams& p, int r, int& flags) {
  const int HW = p.H * p.Wd;
  const int t = r / HW, rem = r - t * HW;
  const int h = rem / p.Wd, w = rem - h * p.Wd;
  flags = (t == 0 ? F_FIRST : 0) | (h == 0 ? F_TOP : 0) | (h == p.H - 1 ? F_BOTTOM : 0) | (w == 0 ? F_LEFT : 0) | (w == p.Wd - 1 ? F_RIGHT : 0);
  return p.row00 + (t > 0 ? 2 * t - 2 : 0) * p.plane + h * p.Wp + w;
}

__global__ __launch_bounds__(256, 2) void conv_time_down2_kernel(TimeDownParams p) {
#if __HIP_DEVICE_COMPILE__  // buffer-resource types exist in the device pass only
  __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
  const Tile tl = make_tile(p.C, p.ldw);
  const int row0 = tl.row0;

  // the tile's lowest source row: tap (., 0, 0) of its first voxel (row0 < M: the grid has ceil(M / BM) row tiles), not below the sample's
  // first voxel; the sample's first voxel when the tile runs from output frame 0 into output frame 1, which starts at source frame 0 again
  const int HW = p.H * p.Wd;
  int f_unused;
  const bool wraps = row0 < HW && HW < (row0 + BM < p.M ? row0 + BM : p.M);
  const int low = src_of(p, row0, f_unused) - p.Wp - 1;
  const int base_row = __builtin_amdgcn_readfirstlane(wraps || low < p.row00 ? p.row00 : low);

  const int ldx2 = (int)p.ldx * 2;
  const int hstep = p.Wp * ldx2, tstep = p.plane * ldx2;
  // per DMA group: the centre row's offset and the five shifts a tap may add, each already 0 where the tap is clamped (edges) or the
  // temporal shift dropped (output frame 0) — plain integers a lane, so no lane mask is carried through the loop
  int a_off[4], d_t[4], d_up[4], d_dn[4], d_lf[4], d_rt[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int f;
    a_off[i] = (src_of(p, tl.dma_voxel(i, p.M), f) - base_row) * ldx2 + tl.dchunk;
    d_t[i] = (f & F_FIRST) ? 0 : tstep;
    d_up[i] = (f & F_TOP) ? 0 : -hstep;
    d_dn[i] = (f & F_BOTTOM) ? 0 : hstep;
    d_lf[i] = (f & F_LEFT) ? 0 : -ldx2;
    d_rt[i] = (f & F_RIGHT) ? 0 : ldx2;
  }
  // edges: top (kh = 0), bottom (kh = 2), left (kw = 0), right (kw = 2)
  const auto mask = frag_masks<4>(tl, p.M, [&](int r) { int f; (void)src_of(p, r, f); return f; });

  const auto rsrc_a = rows_rsrc(p.X, tl.zb * p.sample_rows + base_row, p.rows_total, p.ldx, p.C);
  const auto rsrc_b = rows_rsrc(p.W, tl.col0, p.C, p.ldw, p.K);
  // byte offset of this lane's source row for tap (a, b, c) of DMA group i: the tile-wide row shift, clamped to the centre tap where
  // the tap leaves the grid (the sum is >= 0: the clamped row is a voxel, and no voxel the tile reads lies below base_row)
  auto a_voff = [&](int i, int a, int b, int c) -> int {
    return a_off[i] + a * d_t[i] + (b == 0 ? d_up[i] : b == 2 ? d_dn[i] : 0) + (c == 0 ? d_lf[i] : c == 2 ? d_rt[i] : 0);
  };
  auto pad_mask = [&](int b, int c) -> int {
    return (b == 0 ? mask.m[0] : 0) | (b == 2 ? mask.m[1] : 0) | (c == 0 ? mask.m[2] : 0) | (c == 2 ? mask.m[3] : 0);
  };

  f32x4 acc16[8][4];
  zero_acc(acc16);
  k_loop(smem, tl, rsrc_a, rsrc_b, p.K / BK, p.nkc, a_voff, pad_mask, acc16);   // 27 C / 32 >= 108 k-tiles

  // the pooled residual, between the bias add and the rounding: the lane that owns (voxel, column quad) fetches the three source values
  // of that voxel and channel quad itself (8 bytes each; the frame step is dropped on output frame 0)
  const int ncol0 = tl.col0 + tl.wn * 64;
  const float a3 = p.a3;
  const bf16_t* xr = nullptr;   // the hook's voxel, set at its first column quad (the epilogue walks j = 0..3 of a token block in order)
  int64_t fstep = 0;
  auto residual = [&](int, int j, int rr, float (&v)[4]) {
    if (j == 0) {
      int f;
      const int centre = src_of(p, rr < p.M ? rr : p.M - 1, f);
      xr = p.X + (tl.zb * p.sample_rows + centre) * p.ldx + ncol0 + 4 * tl.lq;
      fstep = (f & F_FIRST) ? 0 : (int64_t)p.plane * p.ldx;
    }
    const uint2 q0 = *reinterpret_cast<const uint2*>(xr + j * 16);
    const uint2 q1 = *reinterpret_cast<const uint2*>(xr + fstep + j * 16);
    const uint2 q2 = *reinterpret_cast<const uint2*>(xr + 2 * fstep + j * 16);
    float s[4];
    s[0] = (bflo(q0.x) + bflo(q1.x)) + bflo(q2.x); s[1] = (bfhi(q0.x) + bfhi(q1.x)) + bfhi(q2.x);
    s[2] = (bflo(q0.y) + bflo(q1.y)) + bflo(q2.y); s[3] = (bfhi(q0.y) + bfhi(q1.y)) + bfhi(q2.y);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = __builtin_fmaf(a3, s[r], v[r]);
  };
  store_tile_bf16(smem, tl, acc16, p.bias, p.out, p.ldo, p.M, residual);
#endif
}

// TimeDownsample2x: a thread owns one (pixel, 8-channel chunk) of a sample and walks the output frames, carrying frame 2 t' as the first
// operand of output frame t' + 1 — every source row is read ONCE, 16 bytes a lane, and every output row written once.
__global__ __launch_bounds__(256) void time_pool_down2_kernel(TimeDownParams p) {
  const int cpr = p.C / 8, HW = p.H * p.Wd;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)HW * cpr) return;
  const int pix = (int)(idx / cpr), ch = (int)(idx - (int64_t)pix * cpr);
  const int h = pix / p.Wd, w = pix - h * p.Wd;
  const int64_t zb = blockIdx.y;
  const bf16_t* src = p.X + (zb * p.sample_rows + p.row00 + (int64_t)h * p.Wp + w) * p.ldx + ch * 8;
  bf16_t* dst = p.out + (zb * p.M + pix) * p.ldo + ch * 8;
  const int64_t fstep = (int64_t)p.plane * p.ldx, ostep = (int64_t)HW * p.ldo;
  const float third = 1.0f / 3.0f;
  auto pool = [&](const uint4& a, const uint4& b, const uint4& c) -> uint4 {
    float fa[8], fb[8], fc[8], o[8];
    unpack8(a, fa); unpack8(b, fb); unpack8(c, fc);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = ((fa[e] + fb[e]) + fc[e]) * third;
    return pack8(o);
  };
  uint4 prev = *reinterpret_cast<const uint4*>(src);
  *reinterpret_cast<uint4*>(dst) = pool(prev, prev, prev);
  for (int t = 1; t < p.To; ++t) {
    const uint4 b = *reinterpret_cast<const uint4*>(src + (2 * t - 1) * fstep);
    const uint4 c = *reinterpret_cast<const uint4*>(src + (2 * t) * fstep);
    *reinterpret_cast<uint4*>(dst + t * ostep) = pool(prev, b, c);
    prev = c;
  }
}

}  // namespace

int launch_conv_time_down2(const bf16_t* x, int64_t ldx, const VaeGrid& g, int64_t nsamples, const bf16_t* w, int64_t ldw, const bf16_t* bias,
                           bf16_t* out, int64_t ldo, int64_t C, float a3, hipStream_t stream) {
  SrcGrid s;
  if (int e = refuse_grid(g, nsamples, s)) return e;
  if (C <= 0 || C > (1 << 20) || C % (w != nullptr ? BN : 8) != 0) return VSYS_ERR_SHAPE;
  const int64_t Wp = s.Wp, plane = s.plane;
  const int64_t To = (g.T - 1) / 2 + 1, HW = (int64_t)g.H * g.W, K = 27 * C;
  if (ldx < C || ldo < C || (w != nullptr && ldw < K)) return VSYS_ERR_SHAPE;
  // tile-relative operand offsets are 32-bit (buffer addressing): the widest source span of BM consecutive output voxels and their taps —
  // a row pitch per wrapped output row, two planes per wrapped output frame, the last time tap's two planes, a row pitch and a row on
  // either side of the centre
  const int64_t q = BM - 1;
  const int64_t span = q + (q + g.W - 1) / g.W * Wp + (q + HW - 1) / HW * 2 * plane + 2 * plane + 2 * Wp + 2;
  if (w != nullptr && ((span + 1) * ldx * 2 >= 0x7fffffff || ldw * 256 + K * 2 >= 0x7fffffff)) return VSYS_ERR_SHAPE;
  const int64_t M = To * HW;
  const int64_t nbm = (M + BM - 1) / BM, nbn = C / BN, npool = (HW * (C / 8) + 255) / 256;
  if (M > 0x7fffffff || nbm * nbn > 0x7fffffff || npool > 0x7fffffff) return VSYS_ERR_SHAPE;
  if (int e = refuse_align(x, ldx, w, w != nullptr ? ldw : 0, bias, out, ldo)) return e;
  if (!(a3 >= 0.f && a3 <= 1.0f / 3.0f)) return VSYS_ERR_ARG;
  if (nsamples == 0) return 0;
  TimeDownParams p;
  p.X = x; p.ldx = ldx; p.sample_rows = g.sample_rows; p.rows_total = nsamples * g.sample_rows;
  p.W = w; p.ldw = ldw; p.bias = bias; p.out = out; p.ldo = ldo;
  p.M = (int)M; p.C = (int)C; p.K = (int)K; p.nkc = (int)(C / BK);
  p.To = (int)To; p.H = g.H; p.Wd = g.W; p.Wp = (int)Wp; p.plane = (int)plane;
  p.row00 = (int)s.row00;
  p.a3 = a3;
  if (w == nullptr)
    hipLaunchKernelGGL(time_pool_down2_kernel, dim3((unsigned)npool, (unsigned)nsamples), dim3(256), 0, stream, p);
  else
    hipLaunchKernelGGL(conv_time_down2_kernel, dim3((unsigned)(nbm * nbn), (unsigned)nsamples), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

}  // namespace vsys
