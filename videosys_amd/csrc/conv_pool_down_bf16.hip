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
// The tile engine — split, geometry, padding by clamped address + zeroed fragment, epilogue — is conv_tile16.h.  Particular to this
// kernel:
//   * reference tap (0, 0) in the FIRST frame of the voxel's pair; the tile's lowest source row is its first voxel's (the map rises with
//     the voxel index for even and odd T alike).  A tap is the row shift kh row_pitch + kw, the second frame of the pair one plane_pitch
//     further — PER LANE, since a tile may hold voxels of output frame 0 (lone: shift dropped, both images hold frame 0) and of output
//     frame 1 (a pair).  Bottom row / right column taps clamp and zero as in conv_down_bf16.hip;
//   * its own pipeline: each k-tile (spatial tap, 32-channel chunk) is fetched as TWO A images, one per frame of the pair, and one W
//     image.  Two stages of (2 A images + 1 W image) = 2 x 40 KiB = 80 KiB of LDS: stage t + 1 is in flight while stage t is multiplied
//     (three A stages of two images would not fit twice in 160 KiB).  A wave reads the two fragments of a 16-voxel block from the two
//     images, unpacks them to fp32, adds, rounds to bf16 once (v_cvt_pk_bf16_f32), applies the padding select and feeds four MFMAs.
//
// Resources (gfx950, pinned by tests/test_build_resources_conv_pool_down.py): 180 VGPRs (128 of them accumulators), 81920 bytes of static
// LDS, NO scratch, two workgroups per CU.  Per k-tile and wave: 32 MFMAs against 8 x (16 unpack + 8 add + 4 convert + 4 select) vector
// instructions — the vector work is of the order of the matrix time, so the kernel is bound by the sum of the two pipes where
// conv_down2 is bound by the matrix pipe alone.  Compiled without packed fp32 instructions, as conv_down_bf16.hip is: the pair sums
// and the bias adds stay single fp32 adds whatever the compiler would pair.
//
// Refused before any launch (launch_conv_pool_down2): VSYS_ERR_SHAPE for cout % 128, cin % 32, what ct16::refuse_grid refuses, and a
// tile whose source span — 256 consecutive output voxels with their taps in both frames — or whose weight panel reaches 2 GiB
// (tile-relative offsets are 32-bit); VSYS_ERR_ALIGN as ct16::refuse_align.
#include "conv_tile16.h"

namespace vsys {
namespace {

using namespace ct16;

constexpr int STAGE = 2 * A_SLOT + W_SLOT;    // 40960: frame 0 image | frame 1 image | weight image
constexpr int POOL_LDS_BYTES = 2 * STAGE;     // 81920
static_assert(4 * OUT_WAVE_BYTES <= POOL_LDS_BYTES, "epilogue image must fit in the staging buffers");
static_assert(2 * POOL_LDS_BYTES <= 160 * 1024, "two workgroups per CU");

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
  __shared__ __attribute__((aligned(16))) char smem[POOL_LDS_BYTES];   // static: the code object carries the figure
  const Tile tl = make_tile(p.N, p.ldw);

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
  const int base_row = __builtin_amdgcn_readfirstlane(src_of(tl.row0, f_unused));   // row0 < M; the map rises with the voxel index

  const int ldx2 = (int)p.ldx * 2;
  const int hstep = p.Wp * ldx2, tstep = p.plane * ldx2;
  int a_off[4], a_flags[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) a_off[i] = (src_of(tl.dma_voxel(i, p.M), a_flags[i]) - base_row) * ldx2 + tl.dchunk;
  // edges: bottom (kh = 2), right (kw = 2)
  const auto mask = frag_masks<2>(tl, p.M, [&](int r) { int f; (void)src_of(r, f); return f; });

  const auto rsrc_a = rows_rsrc(p.X, tl.zb * p.sample_rows + base_row, p.rows_total, p.ldx, p.cin);
  const auto rsrc_b = rows_rsrc(p.W, tl.col0, p.N, p.ldw, p.K);
  // byte offset of this lane's source row, first frame of the pair, for tap (b, c) of DMA group i: the tile-wide row shift, clamped where
  // the tap leaves the grid; the second frame lies one plane further unless the voxel belongs to the lone first frame
  auto a_voff = [&](int i, int b, int c) -> int {
    const int f = a_flags[i];
    const int hb = (b == 2 && (f & 2)) ? 1 : b;
    const int wc = (c == 2 && (f & 4)) ? 1 : c;
    return a_off[i] + hb * hstep + wc * ldx2;
  };
  auto fetch = [&](const KTile& k, int t, int stage) {
    char* img = smem + stage * STAGE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int voff = a_voff(i, k.b, k.c);
      dma_a(rsrc_a, img, tl, i, voff, k.kc);
      dma_a(rsrc_a, img + A_SLOT, tl, i, voff + ((a_flags[i] & 1) ? 0 : tstep), k.kc);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) dma_w(rsrc_b, img + 2 * A_SLOT, tl, i, t);
  };

  const int xo = tl.frag_x();                  // + i*1024 for token block i, + A_SLOT for the second frame
  const int wo_ = 2 * A_SLOT + tl.frag_w();    // + j*1024 for column block j

  f32x4 acc16[8][4];
  zero_acc(acc16);

  const int nt = p.K / BK;
  KTile pf, mul;   // the k-tile being fetched / being multiplied; no time tap: a stays 0 while k-tiles remain
  fetch(pf, 0, 0);
  pf.advance(p.nkc);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  int st = 0;
  for (int t = 0; t < nt; ++t) {
    // stage st ^ 1 was last read in iteration t - 1, which every wave left through the barrier below
    if (t + 1 < nt) fetch(pf, t + 1, st ^ 1);
    __builtin_amdgcn_sched_barrier(0);
    const int mz = (mul.b == 2 ? mask.m[0] : 0) | (mul.c == 2 ? mask.m[1] : 0);   // fragment voxels whose tap is padding
    const char* ab = smem + st * STAGE;
    const bf16x8 w0 = *reinterpret_cast<const bf16x8*>(ab + wo_);
    const bf16x8 w1 = *reinterpret_cast<const bf16x8*>(ab + wo_ + 1024);
    const bf16x8 v0 = *reinterpret_cast<const bf16x8*>(ab + wo_ + 2048);
    const bf16x8 v1 = *reinterpret_cast<const bf16x8*>(ab + wo_ + 3072);
    // two token blocks in flight: the fragments of block i + 1 are read while block i is summed and multiplied
    bf16x8 fa = *reinterpret_cast<const bf16x8*>(ab + xo);
    bf16x8 fb = *reinterpret_cast<const bf16x8*>(ab + xo + A_SLOT);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      bf16x8 na = fa, nb = fb;
      if (i < 7) {
        na = *reinterpret_cast<const bf16x8*>(ab + xo + (i + 1) * 1024);
        nb = *reinterpret_cast<const bf16x8*>(ab + xo + (i + 1) * 1024 + A_SLOT);
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
    pf.advance(p.nkc);
    mul.advance(p.nkc);
  }

  store_tile_bf16(smem, tl, acc16, p.bias, p.out, p.ldo, p.M, NoHook());
#endif
}

}  // namespace

int launch_conv_pool_down2(const bf16_t* x, int64_t ldx, const VaeGrid& g, int64_t nsamples, const bf16_t* w_half, int64_t ldw,
                           const bf16_t* bias, bf16_t* out, int64_t ldo, int64_t cin, int64_t cout, hipStream_t stream) {
  SrcGrid s;
  if (int e = refuse_grid(g, nsamples, s)) return e;
  if (cout <= 0 || cout % BN != 0 || cin <= 0 || cin % BK != 0 || cin > (1 << 20) || cout > (1 << 20)) return VSYS_ERR_SHAPE;
  if (nsamples == 0) return 0;
  const int64_t To = g.T / 2 + (g.T & 1), Ho = g.H / 2, Wo = g.W / 2;
  const int64_t K = 9 * cin;
  if (ldx < cin || ldo < cout || ldw < K) return VSYS_ERR_SHAPE;
  if (int e = refuse_align(x, ldx, w_half, ldw, bias, out, ldo)) return e;
  // tile-relative operand offsets are 32-bit (buffer addressing): the widest source span of BM consecutive output voxels — two columns a
  // voxel, two rows a wrapped output row, two planes a wrapped output frame — with the last tap's shift and the second frame's plane
  const int64_t q = BM - 1;
  const int64_t span = 2 * q + (q + Wo - 1) / Wo * 2 * s.Wp + (q + Ho * Wo - 1) / (Ho * Wo) * 2 * s.plane + s.plane + 2 * s.Wp + 2;
  if ((span + 1) * ldx * 2 >= 0x7fffffff || ldw * 256 + K * 2 >= 0x7fffffff) return VSYS_ERR_SHAPE;
  const int64_t M = To * Ho * Wo;
  const int64_t nbm = (M + BM - 1) / BM, nbn = cout / BN;
  if (M > 0x7fffffff || nbm * nbn > 0x7fffffff) return VSYS_ERR_SHAPE;
  ConvDownParams p;
  p.X = x; p.ldx = ldx; p.sample_rows = g.sample_rows; p.rows_total = nsamples * g.sample_rows;
  p.W = w_half; p.ldw = ldw; p.bias = bias; p.out = out; p.ldo = ldo;
  p.M = (int)M; p.N = (int)cout; p.K = (int)K; p.cin = (int)cin; p.nkc = (int)(cin / BK); p.kt = g.T & 1;   // kt: T is odd
  p.H = g.H; p.Wd = g.W; p.Ho = (int)Ho; p.Wo = (int)Wo; p.Wp = (int)s.Wp; p.plane = (int)s.plane;
  p.row00 = (int)s.row00;
  hipLaunchKernelGGL(conv_pool_down2_kernel, dim3((unsigned)(nbm * nbn), (unsigned)nsamples), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

}  // namespace vsys
