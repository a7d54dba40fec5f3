// Time-pooling stride-2 implicit-GEMM convolution on bf16 MFMA for the CogVideoX VAE ENCODER: CogVideoXDownsample3D with
// compress_time=True (videosys/models/modules/downsampling.py:40-71, down blocks 0 and 1 of CogVideoXEncoder3D,
// autoencoder_kl_cogvideox.py:597-728) — a pairwise mean over time, then F.pad (0, 1, 0, 1) + Conv2d(3, stride 2) per pooled frame — in
// ONE launch that reads the source where it lies: no pooled copy of the activation is made.
//
//   To = T / 2 + (T odd)
//   frames(t') = (2 t', 2 t' + 1)        T even
//              = (0, 0)                  T odd, t' = 0   (the lone first frame: F.avg_pool1d is applied to frames 1 .. T - 1 only)
//              = (2 t' - 1, 2 t')        T odd, t' >= 1
//   m[n, t', h, w, c]  = bf16((x[n, f0, h, w, c] + x[n, f1, h, w, c]) / 2)        sum in fp32, ONE rounding (what avg_pool1d on bf16 does)
//   out[n, t', ho, wo] = b + sum_{kh, kw, c} m[n, t', 2 ho + kh, 2 wo + kw, c] w[., (3 kh + kw) cin + c]
//
// with m = 0 at row H and column W (one zero row below, one zero column to the right, none above or to the left), Ho = H / 2 and
// Wo = W / 2 rounded down.  T = 1 is the spatial mode of conv_down_bf16.hip on the one frame, bit for bit.
//
// THE 1/2 IS NOT IN THE KERNEL: the caller passes w / 2 (exact in bf16 for every normal weight; folded once when the weights are loaded,
// vae_blocks.conv_pool_down2), so the loop forms s = bf16(x0 + x1) and bf16(s) / 2 = bf16(s / 2) = m exactly (a power-of-two scale
// commutes with the rounding).  The lone frame gives s = bf16(a + a) = 2 a exactly, so (2 a)(w / 2) = a w: no branch.
//
// Split: that of conv_down_bf16.hip — a tile is 256 consecutive output voxels (t', ho, wo) of one sample x 128 output channels; every
// DMA lane owns one output voxel per 16-row group and computes ONCE the byte offset of the source row its tap (0, 0) reads in the FIRST
// frame of its pair, relative to the tile's lowest source row (its first voxel's: the map rises with the voxel index for even and odd
// T alike), where the buffer resource starts.  A tap is a tile-wide row shift kh row_pitch + kw, the second frame of the pair one
// plane_pitch further — PER LANE, since a tile may hold voxels of output frame 0 (lone: shift dropped, both images hold frame 0) and of
// output frame 1 (a pair).  Bottom row / right column taps that leave the grid clamp the ADDRESS to the neighbouring tap and zero the
// FRAGMENT in registers by a select, so nothing but voxels of the grid is ever read.
//
// Data movement: each k-tile (spatial tap, 32-channel chunk) is fetched by LDS-DMA as TWO images of 256 rows x 64 bytes, one per frame
// of the pair, with the 16-byte chunk swizzle of conv_down_bf16.hip on the source side; the weight panel is one image of 128 x 64
// bytes.  Two stages of (2 A images + 1 W image) = 2 x 40 KiB = 80 KiB of LDS: stage t + 1 is in flight while stage t is multiplied
// (three A stages of two images would not fit twice in 160 KiB).  A wave reads the two fragments of a 16-voxel block from the two
// images, unpacks them to fp32, adds, rounds to bf16 once (v_cvt_pk_bf16_f32), applies the padding select and feeds four
// v_mfma_f32_16x16x32_bf16 (the wave's 64 output channels); fp32 accumulators, bias added in the epilogue, bf16 stores of whole
// 128-byte row segments through a per-wave LDS image, as conv_down_bf16.hip.
//
// Geometry and resources (gfx950, pinned by tests/test_build_resources_conv_pool_down.py): 4 waves (2 x 2), wave tile 128 voxels x 64
// channels = 8 x 4 accumulators of 16 x 16, BK = 32; 256 threads, 180 VGPRs (128 of them accumulators), 81920 bytes of static LDS,
// NO scratch, two workgroups per CU.  Per k-tile and wave: 32 MFMAs against 8 x (16 unpack + 8 add + 4 convert + 4 select) vector
// instructions — the vector work is of the order of the matrix time, so the kernel is bound by the sum of the two pipes where
// conv_down2 is bound by the matrix pipe alone.  The file is compiled without packed fp32 instructions (__graft_entry__.py
// SOURCE_FLAGS), as conv_down_bf16.hip is: the pair sums and the bias adds stay single fp32 adds whatever the compiler would pair.
//
// Refused before any launch (launch_conv_pool_down2): VSYS_ERR_SHAPE for T < 1, H or W < 2, cout % 128, cin % 32, a grid whose
// sample_rows is below its frames, more than 65535 samples, and a tile whose source span — 256 consecutive output voxels with their
// taps in both frames — or whose weight panel reaches 2 GiB (tile-relative offsets are 32-bit); VSYS_ERR_ALIGN for strides that are no
// multiple of 8 elements or pointers off the 16-byte grid.
#include "common.h"
#include "vsys_internal.h"

namespace vsys {
namespace {

constexpr int BM = 256, BN = 128, BK = 32;
constexpr int A_IMG = BM * BK * 2;            // 16384: one frame image of a k-tile
constexpr int W_IMG = BN * BK * 2;            // 8192
constexpr int STAGE = 2 * A_IMG + W_IMG;      // 40960: frame 0 image | frame 1 image | weight image
constexpr int LDS_BYTES = 2 * STAGE;          // 81920
constexpr int OUT_ROW_BYTES = 64 * 2 + 16;
constexpr int OUT_WAVE_BYTES = 64 * OUT_ROW_BYTES;  // 9216 per wave and pass
static_assert(4 * OUT_WAVE_BYTES <= LDS_BYTES, "epilogue image must fit in the staging buffers");
static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");

// bf16(a + b) element-wise, the sum in fp32; zeros instead where the tap is padding
__device__ __forceinline__ bf16x8 pair_sum(bf16x8 a, bf16x8 b, bool z) {
  const uint4 ua = __builtin_bit_cast(uint4, a), ub = __builtin_bit_cast(uint4, b);
  uint4 u;
  u.x = pack2bf(f32x2{bflo(ua.x) + bflo(ub.x), bfhi(ua.x) + bfhi(ub.x)});
  u.y = pack2bf(f32x2{bflo(ua.y) + bflo(ub.y), bfhi(ua.y) + bfhi(ub.y)});
  u.z = pack2bf(f32x2{bflo(ua.z) + bflo(ub.z), bfhi(ua.z) + bfhi(ub.z)});
  u.w = pack2bf(f32x2{bflo(ua.w) + bflo(ub.w), bfhi(ua.w) + bfhi(ub.w)});
  u.x = z ? 0u : u.x; u.y = z ? 0u : u.y; u.z = z ? 0u : u.z; u.w = z ? 0u : u.w;
  return __builtin_bit_cast(bf16x8, u);
}

__global__ __launch_bounds__(256, 2) void conv_pool_down2_kernel(ConvDownParams p) {
#if __HIP_DEVICE_COMPILE__  // buffer-resource types exist in the device pass only
  __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];   // static: the code object carries the figure
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l15 = lane & 15, lq = lane >> 4;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);

  const int nbn = p.N / BN;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int bm = tile / nbn, bn = tile - bm * nbn;
  const int row0 = bm * BM, col0 = bn * BN;
  const int64_t zb = blockIdx.y;

  // output voxel r of the sample -> source row, inside the sample, that tap (0, 0) reads in the FIRST frame of its pair; flags:
  // 1 the lone first frame (odd T, t' = 0: the second image reads the same frame), 2 bottom output row whose kh = 2 tap is the zero
  // row, 4 right output column whose kw = 2 tap is the zero column.  p.kt holds T & 1.
  const int HoWo = p.Ho * p.Wo;
  auto src_of = [&](int r, int& flags) -> int {
    const int t = r / HoWo, rem = r - t * HoWo;
    const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
    const bool lone = p.kt && t == 0;
    const int f0 = p.kt ? (lone ? 0 : 2 * t - 1) : 2 * t;
    flags = (lone ? 1 : 0) | (2 * ho + 2 >= p.H ? 2 : 0) | (2 * wo + 2 >= p.Wd ? 4 : 0);
    return p.row00 + f0 * p.plane + 2 * ho * p.Wp + 2 * wo;
  };
  int f_unused;
  const int base_row = __builtin_amdgcn_readfirstlane(src_of(row0, f_unused));   // row0 < M; the map rises with the voxel index

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
  // byte offset of this lane's source row, first frame of the pair, for tap (b, c) of DMA group i: the tile-wide row shift, clamped where
  // the tap leaves the grid; the second frame lies one plane further unless the voxel belongs to the lone first frame
  auto a_voff = [&](int i, int b, int c) -> int {
    const int f = a_flags[i];
    const int hb = (b == 2 && (f & 2)) ? 1 : b;
    const int wc = (c == 2 && (f & 4)) ? 1 : c;
    return a_off[i] + hb * hstep + wc * ldx2;
  };
  auto dma_a = [&](int i, int voff, int kc, int stage) {
    char* dst = smem + stage * STAGE + (wave_u * 64 + i * 16) * 64;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, (lds_ptr_t)dst, 16, voff, kc * (BK * 2), 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, (lds_ptr_t)(dst + A_IMG), 16, voff + ((a_flags[i] & 1) ? 0 : tstep), kc * (BK * 2), 0, 0);
  };
  auto dma_w = [&](int i, int t, int stage) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_b, (lds_ptr_t)(smem + stage * STAGE + 2 * A_IMG + (wave_u * 32 + i * 16) * 64), 16,
                                             b_off[i], t * (BK * 2), 0, 0);
  };
  auto fetch = [&](int b, int c, int kc, int t, int stage) {
#pragma unroll
    for (int i = 0; i < 4; ++i) dma_a(i, a_voff(i, b, c), kc, stage);
#pragma unroll
    for (int i = 0; i < 2; ++i) dma_w(i, t, stage);
  };
  // k-tile counters (kh, kw, channel chunk), carried: cin / 32 need not be a power of two
  auto advance = [&](int& b, int& c, int& kc) {
    if (++kc == p.nkc) {
      kc = 0;
      if (++c == 3) { c = 0; ++b; }
    }
  };

  const int fsw = (lq ^ ((0x78 >> (2 * ((l15 >> 2) & 3))) & 3)) << 4;
  const int xo = (wm * 128 + l15) * 64 + fsw;               // + i*1024 for token block i, + A_IMG for the second frame
  const int wo_ = 2 * A_IMG + (wn * 64 + l15) * 64 + fsw;   // + j*1024 for column block j

  f32x4 acc16[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc16[i][j][r] = 0.f;

  const int nt = p.K / BK;
  int pb = 0, pc = 0, pk = 0;   // the k-tile being fetched
  int mb = 0, mc = 0, mk = 0;   // the k-tile being multiplied
  fetch(pb, pc, pk, 0, 0);
  advance(pb, pc, pk);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  int st = 0;
  for (int t = 0; t < nt; ++t) {
    // stage st ^ 1 was last read in iteration t - 1, which every wave left through the barrier below
    if (t + 1 < nt) fetch(pb, pc, pk, t + 1, st ^ 1);
    __builtin_amdgcn_sched_barrier(0);
    const int mz = (mb == 2 ? mask_bot : 0) | (mc == 2 ? mask_right : 0);   // fragment voxels whose tap is padding
    const char* ab = smem + st * STAGE;
    const bf16x8 w0 = *reinterpret_cast<const bf16x8*>(ab + wo_);
    const bf16x8 w1 = *reinterpret_cast<const bf16x8*>(ab + wo_ + 1024);
    const bf16x8 v0 = *reinterpret_cast<const bf16x8*>(ab + wo_ + 2048);
    const bf16x8 v1 = *reinterpret_cast<const bf16x8*>(ab + wo_ + 3072);
    // two token blocks in flight: the fragments of block i + 1 are read while block i is summed and multiplied
    bf16x8 fa = *reinterpret_cast<const bf16x8*>(ab + xo);
    bf16x8 fb = *reinterpret_cast<const bf16x8*>(ab + xo + A_IMG);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      bf16x8 na = fa, nb = fb;
      if (i < 7) {
        na = *reinterpret_cast<const bf16x8*>(ab + xo + (i + 1) * 1024);
        nb = *reinterpret_cast<const bf16x8*>(ab + xo + (i + 1) * 1024 + A_IMG);
      }
      const bf16x8 x = pair_sum(fa, fb, (mz >> i) & 1);
      acc16[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, x, acc16[i][0], 0, 0, 0);
      acc16[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, x, acc16[i][1], 0, 0, 0);
      acc16[i][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v0, x, acc16[i][2], 0, 0, 0);
      acc16[i][3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v1, x, acc16[i][3], 0, 0, 0);
      fa = na; fb = nb;
      __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();  // stage t + 1 has landed everywhere; nobody reads stage t any more
    __builtin_amdgcn_sched_barrier(0);
    st ^= 1;
    advance(pb, pc, pk);
    advance(mb, mc, mk);
  }

  // bf16 output through a per-wave LDS image (two passes of 64 rows), so the global stores are whole 128-byte row segments; element
  // (voxel 16 i + l15, channel 16 j + 4 lq + r) sits in acc16[i][j][r]
  const int ncol0 = col0 + wn * 64;
  bf16_t* ob = p.out + zb * (int64_t)p.M * p.ldo;
  char* img = smem + wave * OUT_WAVE_BYTES;
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
        *reinterpret_cast<uint2*>(img + (i2 * 16 + l15) * OUT_ROW_BYTES + (j * 16 + 4 * lq) * 2) = o;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    uint4 val[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int q = lane + 64 * it;
      val[it] = *reinterpret_cast<const uint4*>(img + (q >> 3) * OUT_ROW_BYTES + (q & 7) * 16);
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

int launch_conv_pool_down2(const bf16_t* x, int64_t ldx, const VaeGrid& g, int64_t nsamples, const bf16_t* w_half, int64_t ldw,
                           const bf16_t* bias, bf16_t* out, int64_t ldo, int64_t cin, int64_t cout, hipStream_t stream) {
  if (g.T < 1 || g.H < 2 || g.W < 2 || g.pad < 0 || g.tf < 0 || nsamples < 0 || nsamples > 65535) return VSYS_ERR_SHAPE;
  if (cout <= 0 || cout % BN != 0 || cin <= 0 || cin % BK != 0 || cin > (1 << 20) || cout > (1 << 20)) return VSYS_ERR_SHAPE;
  const int64_t Hp = g.H + 2 * g.pad, Wp = g.W + 2 * g.pad, plane = Hp * Wp;
  if ((g.T + g.tf) * plane > g.sample_rows || g.sample_rows > 0x7fffffff) return VSYS_ERR_SHAPE;
  if (nsamples == 0) return 0;
  const int64_t To = g.T / 2 + (g.T & 1), Ho = g.H / 2, Wo = g.W / 2;
  const int64_t K = 9 * cin;
  if (ldx < cin || ldo < cout || ldw < K) return VSYS_ERR_SHAPE;
  if ((ldx % 8) || (ldw % 8) || (ldo % 8)) return VSYS_ERR_ALIGN;
  if (!aligned16(x) || !aligned16(w_half) || !aligned16(out) || (reinterpret_cast<uintptr_t>(bias) & 7)) return VSYS_ERR_ALIGN;
  // tile-relative operand offsets are 32-bit (buffer addressing): the widest source span of BM consecutive output voxels — two columns a
  // voxel, two rows a wrapped output row, two planes a wrapped output frame — with the last tap's shift and the second frame's plane
  const int64_t q = BM - 1;
  const int64_t span = 2 * q + (q + Wo - 1) / Wo * 2 * Wp + (q + Ho * Wo - 1) / (Ho * Wo) * 2 * plane + plane + 2 * Wp + 2;
  if ((span + 1) * ldx * 2 >= 0x7fffffff || ldw * 256 + K * 2 >= 0x7fffffff) return VSYS_ERR_SHAPE;
  const int64_t M = To * Ho * Wo;
  const int64_t nbm = (M + BM - 1) / BM, nbn = cout / BN;
  if (M > 0x7fffffff || nbm * nbn > 0x7fffffff) return VSYS_ERR_SHAPE;
  ConvDownParams p;
  p.X = x; p.ldx = ldx; p.sample_rows = g.sample_rows; p.rows_total = nsamples * g.sample_rows;
  p.W = w_half; p.ldw = ldw; p.bias = bias; p.out = out; p.ldo = ldo;
  p.M = (int)M; p.N = (int)cout; p.K = (int)K; p.cin = (int)cin; p.nkc = (int)(cin / BK); p.kt = g.T & 1;   // kt: T is odd
  p.H = g.H; p.Wd = g.W; p.Ho = (int)Ho; p.Wo = (int)Wo; p.Wp = (int)Wp; p.plane = (int)plane;
  p.row00 = (int)((g.tf * Hp + g.pad) * Wp + g.pad);
  hipLaunchKernelGGL(conv_pool_down2_kernel, dim3((unsigned)(nbm * nbn), (unsigned)nsamples), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

}  // namespace vsys
