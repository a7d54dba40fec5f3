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
// Split (the choice the stride forces): PER-ROW DMA ADDRESSES FROM AN OUTPUT-PIXEL -> SOURCE-ROW MAP, not whole source rows in LDS.
// A tile is 256 consecutive output voxels (t', ho, wo) of ONE sample x 128 output channels.  Every DMA lane owns one output voxel per
// 16-row group and computes ONCE the byte offset of the source row its tap (0, 0, 0) reads, relative to the tile's LOWEST source row,
// where the buffer resource starts, so offsets are >= 0.  The map rises with the voxel index except at one place: in the causal mode
// output frames 0 and 1 both start at source frame 0, so a tile that begins inside output frame 0 and reaches output frame 1 has its
// lowest row at the first voxel of the sample, not at its own first voxel.  A tap is then the same row shift for the whole
// tile, as in conv_bf16.hip: a plane_pitch + kh row_pitch + kw rows — except on the voxels whose tap leaves the grid:
//   * bottom row / right column (2 ho + 2 >= H with kh = 2, 2 wo + 2 >= W with kw = 2): the ADDRESS is clamped to the neighbouring tap
//     (kh = 1 / kw = 1, always inside the voxels of the grid) and the FRAGMENT is replaced by zeros in registers before its MFMAs (a
//     select, not a multiply: whatever the clamped row holds never reaches a result);
//   * first output frame (kt = 3, t' = 0): the temporal shift is dropped, every a reads frame 0.
// So the padding comes from the addressing; the source is read where it lies (any VaeGrid: a conv-output grid with junk borders, a
// dense one), no padded copy of the activation is made, and nothing but voxels of the grid is ever read.  LDS holds the staged k-tiles
// exactly as in conv_bf16.hip (16-byte chunk swizzle on the source side, fragments straight from the image), so fragment reads are
// not strided.  Whole source rows in LDS would move 4x the bytes the MFMAs use through the DMA path (two of three rows, both column
// parities) and tie the tile shape to W.
//
// Geometry: that of conv_kernel<0, 1>.  4 waves (2 x 2), wave tile 128 voxels x 64 channels = 8 x 4 accumulators of 16 x 16, BK = 32,
// three A slots + two W slots = 64 KiB of LDS, 256 threads, two workgroups per CU (<= 256 VGPRs, no scratch: pinned by
// tests/test_build_resources_conv_down.py).  k runs tap-major: (a, kh, kw) outermost to innermost, then the channel chunks of 32, the
// order of conv_bf16.hip; cin is any multiple of 32 (the tap / chunk counters are carried, not divided out).  The file is compiled
// without packed fp32 instructions (__graft_entry__.py SOURCE_FLAGS): the epilogue's bias adds are four independent fp32 adds per
// lane, which the compiler may otherwise pair into v_pk_add_f32; single adds keep the output bits independent of that choice.
//
// Refused before any launch (launch_conv_down2): VSYS_ERR_SHAPE for kt not 1 or 3, H or W < 2, cout % 128, cin % 32, a grid whose
// sample_rows is below its frames, more than 65535 samples, and a tile whose source span — 256 consecutive output voxels with their
// taps: 2 * 255 + ceil(255 / Wo) * 2 row_pitch + ceil(255 / (Ho Wo)) * (2 or 1) plane_pitch + the last tap's shift, in rows of ldx
// elements (a tile that wraps from output frame 0 to 1 spans less than one plane_pitch plus that shift, which the bound covers) — or
// whose weight panel reaches 2 GiB (tile-relative offsets are 32-bit); VSYS_ERR_ALIGN for strides that are no multiple of 8 elements
// or pointers off the 16-byte grid.
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

__device__ __forceinline__ bf16x8 zero_if(bf16x8 v, bool z) {
  uint4 u = __builtin_bit_cast(uint4, v);
  u.x = z ? 0u : u.x; u.y = z ? 0u : u.y; u.z = z ? 0u : u.z; u.w = z ? 0u : u.w;
  return __builtin_bit_cast(bf16x8, u);
}

__global__ __launch_bounds__(256, 2) void conv_down2_kernel(ConvDownParams p) {
#if __HIP_DEVICE_COMPILE__  // buffer-resource types exist in the device pass only
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l15 = lane & 15, lq = lane >> 4;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);

  const int nbn = p.N / BN;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int bm = tile / nbn, bn = tile - bm * nbn;
  const int row0 = bm * BM, col0 = bn * BN;
  const int64_t zb = blockIdx.y;

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
  const int dchunk = ((lane & 3) ^ ((0x78 >> (2 * ((lane >> 4) & 3))) & 3)) * 16;
  int a_off[4], a_flags[4], b_off[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = row0 + wave_u * 64 + i * 16 + (lane >> 2);
    const int rl = r < p.M ? r : p.M - 1;  // rows past M re-read the last voxel (never stored)
    a_off[i] = (src_of(rl, a_flags[i]) - base_row) * ldx2 + dchunk;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) b_off[i] = (wave_u * 32 + i * 16 + (lane >> 2)) * (int)p.ldw * 2 + dchunk;
  // which of this lane's eight fragment voxels (16 i + l15 of the wave's 128) lose their kh = 2 / kw = 2 tap to the zero row / column
  int mask_bot = 0, mask_right = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = row0 + wm * 128 + i * 16 + l15;
    int f;
    (void)src_of(r < p.M ? r : p.M - 1, f);
    mask_bot |= ((f >> 1) & 1) << i;
    mask_right |= ((f >> 2) & 1) << i;
  }

  const int64_t abs_row = zb * p.sample_rows + base_row;
  const int64_t a_bytes = ((p.rows_total - 1 - abs_row) * p.ldx + p.cin) * 2;   // to the end of the operand's last row
  const int64_t b_bytes = ((int64_t)(p.N - 1 - col0) * p.ldw + p.K) * 2;
  const auto rsrc_a = __builtin_amdgcn_make_buffer_rsrc((void*)(p.X + abs_row * p.ldx), 0,
                                                        (int)(a_bytes < 0x7fffffff ? a_bytes : 0x7fffffff), 0x00020000);
  const auto rsrc_b = __builtin_amdgcn_make_buffer_rsrc((void*)(p.W + (int64_t)col0 * p.ldw), 0,
                                                        (int)(b_bytes < 0x7fffffff ? b_bytes : 0x7fffffff), 0x00020000);
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  // byte offset of this lane's source row for tap (a, b, c) of DMA group i: the tile-wide row shift, clamped where the tap leaves the grid
  auto a_voff = [&](int i, int a, int b, int c) -> int {
    const int f = a_flags[i];
    const int hb = (b == 2 && (f & 2)) ? 1 : b;
    const int wc = (c == 2 && (f & 4)) ? 1 : c;
    return a_off[i] + ((f & 1) ? 0 : a * tstep) + hb * hstep + wc * ldx2;
  };
  auto dma_a = [&](int i, int voff, int kc, int slot) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, (lds_ptr_t)(smem + slot * A_SLOT + (wave_u * 64 + i * 16) * 64), 16, voff,
                                             kc * (BK * 2), 0, 0);
  };
  auto dma_w = [&](int i, int t, int slot) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_b, (lds_ptr_t)(smem + W_BASE + slot * W_SLOT + (wave_u * 32 + i * 16) * 64), 16,
                                             b_off[i], t * (BK * 2), 0, 0);
  };
  // k-tile counters (temporal tap, kh, kw, channel chunk), carried: cin / 32 need not be a power of two
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

  const int nt = p.K / BK;
  int pa = 0, pb = 0, pc = 0, pk = 0;   // the k-tile being fetched
  int mb = 0, mc = 0, mk = 0, ma = 0;   // the k-tile being multiplied
#pragma unroll
  for (int i = 0; i < 4; ++i) dma_a(i, a_voff(i, pa, pb, pc), pk, 0);
#pragma unroll
  for (int i = 0; i < 2; ++i) dma_w(i, 0, 0);
  advance(pa, pb, pc, pk);
  if (nt > 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) dma_a(i, a_voff(i, pa, pb, pc), pk, 1);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
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
    const int mz = (mb == 2 ? mask_bot : 0) | (mc == 2 ? mask_right : 0);   // fragment voxels whose tap is padding
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
#define CD16_ROW(i_, X_)                                                                              \
  X_ = zero_if(X_, (mz >> (i_)) & 1);                                                                 \
  acc16[i_][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, X_, acc16[i_][0], 0, 0, 0);              \
  acc16[i_][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, X_, acc16[i_][1], 0, 0, 0);              \
  acc16[i_][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v0, X_, acc16[i_][2], 0, 0, 0);              \
  acc16[i_][3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v1, X_, acc16[i_][3], 0, 0, 0)
    CD16_ROW(0, x0);
    __builtin_amdgcn_sched_barrier(0);
    x0 = *reinterpret_cast<const bf16x8*>(ab + xo + 4096);
    if (n1) { dma_w(0, t + 1, sw1); dma_w(1, t + 1, sw1); }
    __builtin_amdgcn_sched_barrier(0);
    CD16_ROW(1, x1);
    __builtin_amdgcn_sched_barrier(0);
    x1 = *reinterpret_cast<const bf16x8*>(ab + xo + 5120);
    if (n2) { dma_a(0, v2[0], k2, sa2); dma_a(1, v2[1], k2, sa2); }
    __builtin_amdgcn_sched_barrier(0);
    CD16_ROW(2, x2);
    __builtin_amdgcn_sched_barrier(0);
    x2 = *reinterpret_cast<const bf16x8*>(ab + xo + 6144);
    if (n2) dma_a(2, v2[2], k2, sa2);
    __builtin_amdgcn_sched_barrier(0);
    CD16_ROW(3, x3);
    __builtin_amdgcn_sched_barrier(0);
    x3 = *reinterpret_cast<const bf16x8*>(ab + xo + 7168);
    if (n2) dma_a(3, v2[3], k2, sa2);
    __builtin_amdgcn_sched_barrier(0);
    CD16_ROW(4, x0);
    CD16_ROW(5, x1);
    CD16_ROW(6, x2);
    CD16_ROW(7, x3);
#undef CD16_ROW
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

  // bf16 output through a per-wave LDS image (two passes of 64 rows), so the global stores are whole 128-byte row segments; element
  // (voxel 16 i + l15, channel 16 j + 4 lq + r) sits in acc16[i][j][r]
  const int ncol0 = col0 + wn * 64;
  bf16_t* ob = p.out + zb * (int64_t)p.M * p.ldo;
  char* st = smem + wave * OUT_WAVE_BYTES;
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
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc16[i][j][r];
        v[0] += bflo(bb16[j].x); v[1] += bfhi(bb16[j].x); v[2] += bflo(bb16[j].y); v[3] += bfhi(bb16[j].y);
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

inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

}  // namespace

int launch_conv_down2(const bf16_t* x, int64_t ldx, const VaeGrid& g, int64_t nsamples, const bf16_t* w, int64_t ldw, const bf16_t* bias,
                      bf16_t* out, int64_t ldo, int64_t cin, int64_t cout, int kt, hipStream_t stream) {
  if (kt != 1 && kt != 3) return VSYS_ERR_SHAPE;
  if (g.T < 1 || g.H < 2 || g.W < 2 || nsamples < 0 || nsamples > 65535) return VSYS_ERR_SHAPE;
  if (cout <= 0 || cout % BN != 0 || cin <= 0 || cin % BK != 0 || cin > (1 << 20) || cout > (1 << 20)) return VSYS_ERR_SHAPE;
  const int64_t Hp = g.H + 2 * g.pad, Wp = g.W + 2 * g.pad, plane = Hp * Wp;
  if ((g.T + g.tf) * plane > g.sample_rows || g.sample_rows > 0x7fffffff) return VSYS_ERR_SHAPE;
  if (nsamples == 0) return 0;
  const int64_t To = kt == 3 ? (g.T - 1) / 2 + 1 : g.T, Ho = g.H / 2, Wo = g.W / 2;
  const int64_t K = 9 * kt * cin;
  if (ldx < cin || ldo < cout || ldw < K) return VSYS_ERR_SHAPE;
  if ((ldx % 8) || (ldw % 8) || (ldo % 8)) return VSYS_ERR_ALIGN;
  if (!aligned16(x) || !aligned16(w) || !aligned16(out) || (reinterpret_cast<uintptr_t>(bias) & 7)) return VSYS_ERR_ALIGN;
  // tile-relative operand offsets are 32-bit (buffer addressing): the widest source span of BM consecutive output voxels and their taps
  const int64_t q = BM - 1;
  const int64_t span = 2 * q + (q + Wo - 1) / Wo * 2 * Wp + (q + Ho * Wo - 1) / (Ho * Wo) * (kt == 3 ? 2 : 1) * plane +
                       (kt - 1) * plane + 2 * Wp + 2;
  if ((span + 1) * ldx * 2 >= 0x7fffffff || ldw * 256 + K * 2 >= 0x7fffffff) return VSYS_ERR_SHAPE;
  const int64_t M = To * Ho * Wo;
  const int64_t nbm = (M + BM - 1) / BM, nbn = cout / BN;
  if (M > 0x7fffffff || nbm * nbn > 0x7fffffff) return VSYS_ERR_SHAPE;
  ConvDownParams p;
  p.X = x; p.ldx = ldx; p.sample_rows = g.sample_rows; p.rows_total = nsamples * g.sample_rows;
  p.W = w; p.ldw = ldw; p.bias = bias; p.out = out; p.ldo = ldo;
  p.M = (int)M; p.N = (int)cout; p.K = (int)K; p.cin = (int)cin; p.nkc = (int)(cin / BK); p.kt = kt;
  p.H = g.H; p.Wd = g.W; p.Ho = (int)Ho; p.Wo = (int)Wo; p.Wp = (int)Wp; p.plane = (int)plane;
  p.row00 = (int)((g.tf * Hp + g.pad) * Wp + g.pad);
  static std::atomic<unsigned long long> attr_seen{0};   // per device
  for (DeviceOnce once(attr_seen); once.todo(); once.done())
    (void)hipFuncSetAttribute((const void*)conv_down2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
  hipLaunchKernelGGL(conv_down2_kernel, dim3((unsigned)(nbm * nbn), (unsigned)nsamples), dim3(256), LDS_BYTES, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

}  // namespace vsys
