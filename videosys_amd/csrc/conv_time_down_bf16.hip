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
// Split: per-lane DMA addresses from an output-voxel -> source-row map, as conv_down_bf16.hip.  A tile is 256 consecutive output voxels
// (t', h, w) of ONE sample x 128 output channels.  Every DMA lane owns one output voxel per 16-row group and computes ONCE the byte offset
// of the source row of its CENTRE tap in time tap 0, (f(t', 0), h, w), relative to the tile's lowest source row, where the buffer
// resource starts.  A tap is then the tile-wide row shift a plane_pitch + (kh - 1) row_pitch + (kw - 1) rows.  The map rises with the
// voxel index — a tile crosses output frames, each of which jumps TWO source planes — except at one place: output frames 0 and 1 both
// start at source frame 0, so a tile that begins in output frame 0 and reaches frame 1 has its lowest row at the sample's first voxel.
// Every other tile's lowest row is one row pitch and one row below its first voxel's centre (its tap (., 0, 0)), but never below the
// sample's first voxel.
//
// Edges: ALL FOUR spatial edges pad from the addressing.  On the voxels whose tap leaves the grid (kh = 0 at h = 0, kh = 2 at h = H - 1,
// kw = 0 at w = 0, kw = 2 at w = W - 1) the ADDRESS is clamped to the centre tap (kh = 1 / kw = 1, always a voxel) and the FRAGMENT is
// replaced by zeros in registers before its MFMAs (a select: whatever the clamped row holds never reaches a result).  On output frame 0
// the temporal shift is dropped: every a reads frame 0.  The source is read where it lies (any VaeGrid: the padded output grid of the
// spatial downsampler, a dense one), no padded copy is made and nothing but voxels of the grid is ever read.
//
// The pooled residual is no separate pass: in the epilogue the lane that owns (voxel, column quad) of the accumulator tile FETCHES the
// three source values itself — three 8-byte loads of rows whose 128-column segment is the centre-tap k-tiles the main loop of this
// very tile pulled through L2.  Keeping them from the staged A image was the alternative and is not taken: the image of a k-tile holds
// 32 channels of ONE tap for 256 voxels, the residual columns of a tile are 128 channels of THREE taps, which pass through the three A
// slots at 12 different k-tiles; holding them would take 3 x 256 x 128 x 2 = 192 KiB of LDS, more than a CU has, or 48 more registers a
// lane beside 128 accumulators.  The fetch costs 96 8-byte L2 hits per lane after 27 C / 32 k-tiles of 32 MFMAs.
//
// Geometry: that of conv_down_bf16.hip.  4 waves (2 x 2), wave tile 128 voxels x 64 channels = 8 x 4 accumulators of 16 x 16,
// v_mfma_f32_16x16x32_bf16, BK = 32, A by LDS-DMA with the 16-byte chunk swizzle on the source side, three A slots + two W slots =
// 65536 bytes of STATIC LDS (the code object carries the figure), 256 threads, two workgroups per CU, no scratch (pinned by
// tests/test_build_resources_conv_time_down.py).  k runs tap-major, (a, kh, kw) outermost to innermost, then the C / 32 channel chunks.
// The file is compiled without packed fp32 instructions (__graft_entry__.py SOURCE_FLAGS): the epilogue's adds stay single fp32
// operations, so the output bits do not depend on how the compiler would pair them; the a3 multiply-add is an explicit fma.
//
// Refused before any launch (launch_conv_time_down2): VSYS_ERR_SHAPE for C % 128 with weights or C % 8 without, T < 1, H or W < 2, a grid
// whose sample_rows is below its frames, more than 65535 samples, a tile whose source span or a weight panel that reaches 2 GiB
// (tile-relative offsets are 32-bit); VSYS_ERR_ALIGN for strides that are no multiple of 8 elements or pointers off the 16-byte grid;
// VSYS_ERR_ARG for a3 outside [0, fp32(1 / 3)].
#include "common.h"
#include "vsys_internal.h"

namespace vsys {
namespace {

constexpr int BM = 256, BN = 128, BK = 32;
constexpr int A_SLOT = BM * BK * 2;   // 16384
constexpr int W_SLOT = BN * BK * 2;   // 8192
constexpr int W_BASE = 3 * A_SLOT;    // 49152
constexpr int LDS_BYTES = W_BASE + 2 * W_SLOT;  // 65536
constexpr int OUT_ROW_BYTES = 64 * 2 + 16;
constexpr int OUT_WAVE_BYTES = 64 * OUT_ROW_BYTES;  // 9216 per wave and pass
static_assert(4 * OUT_WAVE_BYTES <= LDS_BYTES, "epilogue image must fit in the staging buffers");
static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");

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

__device__ __forceinline__ bf16x8 zero_if(bf16x8 v, bool z) {
  uint4 u = __builtin_bit_cast(uint4, v);
  u.x = z ? 0u : u.x; u.y = z ? 0u : u.y; u.z = z ? 0u : u.z; u.w = z ? 0u : u.w;
  return __builtin_bit_cast(bf16x8, u);
}

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
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l15 = lane & 15, lq = lane >> 4;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);

  const int nbn = p.C / BN;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int bm = tile / nbn, bn = tile - bm * nbn;
  const int row0 = bm * BM, col0 = bn * BN;
  const int64_t zb = blockIdx.y;

  // the tile's lowest source row: tap (., 0, 0) of its first voxel (row0 < M: the grid has ceil(M / BM) row tiles), not below the sample's
  // first voxel; the sample's first voxel when the tile runs from output frame 0 into output frame 1, which starts at source frame 0 again
  const int HW = p.H * p.Wd;
  int f_unused;
  const bool wraps = row0 < HW && HW < (row0 + BM < p.M ? row0 + BM : p.M);
  const int low = src_of(p, row0, f_unused) - p.Wp - 1;
  const int base_row = __builtin_amdgcn_readfirstlane(wraps || low < p.row00 ? p.row00 : low);

  const int ldx2 = (int)p.ldx * 2;
  const int hstep = p.Wp * ldx2, tstep = p.plane * ldx2;
  const int dchunk = ((lane & 3) ^ ((0x78 >> (2 * ((lane >> 4) & 3))) & 3)) * 16;
  // per DMA group: the centre row's offset and the five shifts a tap may add, each already 0 where the tap is clamped (edges) or the
  // temporal shift dropped (output frame 0) — plain integers a lane, so no lane mask is carried through the loop
  int a_off[4], d_t[4], d_up[4], d_dn[4], d_lf[4], d_rt[4], b_off[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = row0 + wave_u * 64 + i * 16 + (lane >> 2);
    const int rl = r < p.M ? r : p.M - 1;  // rows past M re-read the last voxel (never stored)
    int f;
    a_off[i] = (src_of(p, rl, f) - base_row) * ldx2 + dchunk;
    d_t[i] = (f & F_FIRST) ? 0 : tstep;
    d_up[i] = (f & F_TOP) ? 0 : -hstep;
    d_dn[i] = (f & F_BOTTOM) ? 0 : hstep;
    d_lf[i] = (f & F_LEFT) ? 0 : -ldx2;
    d_rt[i] = (f & F_RIGHT) ? 0 : ldx2;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) b_off[i] = (wave_u * 32 + i * 16 + (lane >> 2)) * (int)p.ldw * 2 + dchunk;
  // which of this lane's eight fragment voxels (16 i + l15 of the wave's 128) lose their kh = 0 / kh = 2 / kw = 0 / kw = 2 tap to the padding
  int mask_top = 0, mask_bot = 0, mask_left = 0, mask_right = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = row0 + wm * 128 + i * 16 + l15;
    int f;
    (void)src_of(p, r < p.M ? r : p.M - 1, f);
    mask_top |= ((f >> 1) & 1) << i;
    mask_bot |= ((f >> 2) & 1) << i;
    mask_left |= ((f >> 3) & 1) << i;
    mask_right |= ((f >> 4) & 1) << i;
  }

  const int64_t abs_row = zb * p.sample_rows + base_row;
  const int64_t a_bytes = ((p.rows_total - 1 - abs_row) * p.ldx + p.C) * 2;   // to the end of the operand's last row
  const int64_t b_bytes = ((int64_t)(p.C - 1 - col0) * p.ldw + p.K) * 2;
  const auto rsrc_a = __builtin_amdgcn_make_buffer_rsrc((void*)(p.X + abs_row * p.ldx), 0,
                                                        (int)(a_bytes < 0x7fffffff ? a_bytes : 0x7fffffff), 0x00020000);
  const auto rsrc_b = __builtin_amdgcn_make_buffer_rsrc((void*)(p.W + (int64_t)col0 * p.ldw), 0,
                                                        (int)(b_bytes < 0x7fffffff ? b_bytes : 0x7fffffff), 0x00020000);
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  // byte offset of this lane's source row for tap (a, b, c) of DMA group i: the tile-wide row shift, clamped to the centre tap where
  // the tap leaves the grid (the sum is >= 0: the clamped row is a voxel, and no voxel the tile reads lies below base_row)
  auto a_voff = [&](int i, int a, int b, int c) -> int {
    return a_off[i] + a * d_t[i] + (b == 0 ? d_up[i] : b == 2 ? d_dn[i] : 0) + (c == 0 ? d_lf[i] : c == 2 ? d_rt[i] : 0);
  };
  auto dma_a = [&](int i, int voff, int kc, int slot) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, (lds_ptr_t)(smem + slot * A_SLOT + (wave_u * 64 + i * 16) * 64), 16, voff,
                                             kc * (BK * 2), 0, 0);
  };
  auto dma_w = [&](int i, int t, int slot) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_b, (lds_ptr_t)(smem + W_BASE + slot * W_SLOT + (wave_u * 32 + i * 16) * 64), 16,
                                             b_off[i], t * (BK * 2), 0, 0);
  };
  // k-tile counters (temporal tap, kh, kw, channel chunk), carried
  auto advance = [&](int& a, int& b, int& c, int& kc) {
    if (++kc == p.nkc) {
      kc = 0;
      if (++c == 3) {
        c = 0;
        if (++b == 3) { b = 0; ++a; }
      }
    }
  };

  const int fsw = (lq ^ ((0x78 >> (2 * ((l15 >> 2) & 3))) & 3)) << 4;
  const int xo = (wm * 128 + l15) * 64 + fsw;           // + i*1024 for token block i
  const int wo_ = W_BASE + (wn * 64 + l15) * 64 + fsw;  // + j*1024 for column block j

  f32x4 acc16[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc16[i][j][r] = 0.f;

  const int nt = p.K / BK;              // 27 C / 32 >= 108
  int pa = 0, pb = 0, pc = 0, pk = 0;   // the k-tile being fetched
  int mb = 0, mc = 0, mk = 0, ma = 0;   // the k-tile being multiplied
#pragma unroll
  for (int i = 0; i < 4; ++i) dma_a(i, a_voff(i, pa, pb, pc), pk, 0);
#pragma unroll
  for (int i = 0; i < 2; ++i) dma_w(i, 0, 0);
  advance(pa, pb, pc, pk);
#pragma unroll
  for (int i = 0; i < 4; ++i) dma_a(i, a_voff(i, pa, pb, pc), pk, 1);
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  advance(pa, pb, pc, pk);
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  int sa = 0, sw = 0;
  for (int t = 0; t < nt; ++t) {
    const int sa1 = sa == 2 ? 0 : sa + 1, sa2 = sa1 == 2 ? 0 : sa1 + 1, sw1 = sw ^ 1;
    const bool n1 = t + 1 < nt, n2 = t + 2 < nt;
    int v2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v2[i] = a_voff(i, pa, pb, pc);
    const int k2 = pk;
    // fragment voxels whose tap is padding
    const int mz = (mb == 0 ? mask_top : 0) | (mb == 2 ? mask_bot : 0) | (mc == 0 ? mask_left : 0) | (mc == 2 ? mask_right : 0);
    const char* ab = smem + sa * A_SLOT;
    const char* wb = smem + sw * W_SLOT;
    bf16x8 x0, x1, x2, x3, w0, w1, v0, v1;
    // (w0, w1, v0, v1) = the four column blocks, x0..x3 = token blocks 0..3, reloaded with blocks 4..7 behind their MFMAs
    x0 = *reinterpret_cast<const bf16x8*>(ab + xo);
    w0 = *reinterpret_cast<const bf16x8*>(wb + wo_);
    w1 = *reinterpret_cast<const bf16x8*>(wb + wo_ + 1024);
    v0 = *reinterpret_cast<const bf16x8*>(wb + wo_ + 2048);
    v1 = *reinterpret_cast<const bf16x8*>(wb + wo_ + 3072);
    x1 = *reinterpret_cast<const bf16x8*>(ab + xo + 1024);
    x2 = *reinterpret_cast<const bf16x8*>(ab + xo + 2048);
    x3 = *reinterpret_cast<const bf16x8*>(ab + xo + 3072);
    __builtin_amdgcn_sched_barrier(0);
#define CT16_ROW(i_, X_)                                                                              \
  X_ = zero_if(X_, (mz >> (i_)) & 1);                                                                 \
  acc16[i_][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, X_, acc16[i_][0], 0, 0, 0);              \
  acc16[i_][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, X_, acc16[i_][1], 0, 0, 0);              \
  acc16[i_][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v0, X_, acc16[i_][2], 0, 0, 0);              \
  acc16[i_][3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v1, X_, acc16[i_][3], 0, 0, 0)
    CT16_ROW(0, x0);
    __builtin_amdgcn_sched_barrier(0);
    x0 = *reinterpret_cast<const bf16x8*>(ab + xo + 4096);
    if (n1) { dma_w(0, t + 1, sw1); dma_w(1, t + 1, sw1); }
    __builtin_amdgcn_sched_barrier(0);
    CT16_ROW(1, x1);
    __builtin_amdgcn_sched_barrier(0);
    x1 = *reinterpret_cast<const bf16x8*>(ab + xo + 5120);
    if (n2) { dma_a(0, v2[0], k2, sa2); dma_a(1, v2[1], k2, sa2); }
    __builtin_amdgcn_sched_barrier(0);
    CT16_ROW(2, x2);
    __builtin_amdgcn_sched_barrier(0);
    x2 = *reinterpret_cast<const bf16x8*>(ab + xo + 6144);
    if (n2) dma_a(2, v2[2], k2, sa2);
    __builtin_amdgcn_sched_barrier(0);
    CT16_ROW(3, x3);
    __builtin_amdgcn_sched_barrier(0);
    x3 = *reinterpret_cast<const bf16x8*>(ab + xo + 7168);
    if (n2) dma_a(3, v2[3], k2, sa2);
    __builtin_amdgcn_sched_barrier(0);
    CT16_ROW(4, x0);
    CT16_ROW(5, x1);
    CT16_ROW(6, x2);
    CT16_ROW(7, x3);
#undef CT16_ROW
    __builtin_amdgcn_sched_barrier(0);
    if (n2) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();  // stage t+1 has landed everywhere; nobody reads the slots of stage t any more
    __builtin_amdgcn_sched_barrier(0);
    sa = sa1;
    sw = sw1;
    advance(pa, pb, pc, pk);
    advance(ma, mb, mc, mk);
  }

  // bias + pooled residual + bf16 output through a per-wave LDS image (two passes of 64 rows), so the global stores are whole 128-byte
  // row segments; element (voxel 16 i + l15, channel 16 j + 4 lq + r) sits in acc16[i][j][r], and its lane fetches the three source
  // values of that voxel and channel quad itself (8 bytes each; the frame step is dropped on output frame 0)
  const int ncol0 = col0 + wn * 64;
  bf16_t* ob = p.out + zb * (int64_t)p.M * p.ldo;
  char* st = smem + wave * OUT_WAVE_BYTES;
  const float a3 = p.a3;
  uint2 bb16[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    bb16[j] = p.bias != nullptr ? *reinterpret_cast<const uint2*>(p.bias + ncol0 + j * 16 + 4 * lq) : make_uint2(0, 0);
#pragma unroll
  for (int ih = 0; ih < 2; ++ih) {
    const int wrow0 = row0 + wm * 128 + ih * 64;
#pragma unroll
    for (int i2 = 0; i2 < 4; ++i2) {
      const int i = ih * 4 + i2;
      const int rr = wrow0 + i2 * 16 + l15;
      int f;
      const int centre = src_of(p, rr < p.M ? rr : p.M - 1, f);
      const bf16_t* xr = p.X + (zb * p.sample_rows + centre) * p.ldx + ncol0 + 4 * lq;
      const int64_t fstep = (f & F_FIRST) ? 0 : (int64_t)p.plane * p.ldx;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint2 q0 = *reinterpret_cast<const uint2*>(xr + j * 16);
        const uint2 q1 = *reinterpret_cast<const uint2*>(xr + fstep + j * 16);
        const uint2 q2 = *reinterpret_cast<const uint2*>(xr + 2 * fstep + j * 16);
        float v[4], s[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc16[i][j][r];
        v[0] += bflo(bb16[j].x); v[1] += bfhi(bb16[j].x); v[2] += bflo(bb16[j].y); v[3] += bfhi(bb16[j].y);
        s[0] = (bflo(q0.x) + bflo(q1.x)) + bflo(q2.x); s[1] = (bfhi(q0.x) + bfhi(q1.x)) + bfhi(q2.x);
        s[2] = (bflo(q0.y) + bflo(q1.y)) + bflo(q2.y); s[3] = (bfhi(q0.y) + bfhi(q1.y)) + bfhi(q2.y);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = __builtin_fmaf(a3, s[r], v[r]);
        uint2 o;
        o.x = pack2bf(v[0], v[1]);
        o.y = pack2bf(v[2], v[3]);
        *reinterpret_cast<uint2*>(st + (i2 * 16 + l15) * OUT_ROW_BYTES + (j * 16 + 4 * lq) * 2) = o;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    uint4 val[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int q = lane + 64 * it;
      val[it] = *reinterpret_cast<const uint4*>(st + (q >> 3) * OUT_ROW_BYTES + (q & 7) * 16);
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int q = lane + 64 * it;
      const int64_t grow = wrow0 + (q >> 3);
      if (grow < p.M) *reinterpret_cast<uint4*>(ob + grow * p.ldo + ncol0 + (q & 7) * 8) = val[it];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // image reads done before the next pass overwrites it
    __builtin_amdgcn_wave_barrier();
  }
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

inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

}  // namespace

int launch_conv_time_down2(const bf16_t* x, int64_t ldx, const VaeGrid& g, int64_t nsamples, const bf16_t* w, int64_t ldw, const bf16_t* bias,
                           bf16_t* out, int64_t ldo, int64_t C, float a3, hipStream_t stream) {
  if (g.T < 1 || g.H < 2 || g.W < 2 || g.pad < 0 || g.tf < 0 || nsamples < 0 || nsamples > 65535) return VSYS_ERR_SHAPE;
  if (C <= 0 || C > (1 << 20) || C % (w != nullptr ? BN : 8) != 0) return VSYS_ERR_SHAPE;
  const int64_t Hp = g.H + 2 * g.pad, Wp = g.W + 2 * g.pad, plane = Hp * Wp;
  if ((g.T + g.tf) * plane > g.sample_rows || g.sample_rows > 0x7fffffff) return VSYS_ERR_SHAPE;
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
  if ((ldx % 8) || (ldo % 8) || (w != nullptr && (ldw % 8))) return VSYS_ERR_ALIGN;
  if (!aligned16(x) || !aligned16(w) || !aligned16(out) || (reinterpret_cast<uintptr_t>(bias) & 7)) return VSYS_ERR_ALIGN;
  if (!(a3 >= 0.f && a3 <= 1.0f / 3.0f)) return VSYS_ERR_ARG;
  if (nsamples == 0) return 0;
  TimeDownParams p;
  p.X = x; p.ldx = ldx; p.sample_rows = g.sample_rows; p.rows_total = nsamples * g.sample_rows;
  p.W = w; p.ldw = ldw; p.bias = bias; p.out = out; p.ldo = ldo;
  p.M = (int)M; p.C = (int)C; p.K = (int)K; p.nkc = (int)(C / BK);
  p.To = (int)To; p.H = g.H; p.Wd = g.W; p.Wp = (int)Wp; p.plane = (int)plane;
  p.row00 = (int)((g.tf * Hp + g.pad) * Wp + g.pad);
  p.a3 = a3;
  if (w == nullptr)
    hipLaunchKernelGGL(time_pool_down2_kernel, dim3((unsigned)npool, (unsigned)nsamples), dim3(256), 0, stream, p);
  else
    hipLaunchKernelGGL(conv_time_down2_kernel, dim3((unsigned)(nbm * nbn), (unsigned)nsamples), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

}  // namespace vsys
