// The tile engine that the three stride-2 convolutions of the VAE ENCODERS share: conv_down2_kernel (conv_down_bf16.hip),
// conv_pool_down2_kernel (conv_pool_down_bf16.hip) and conv_time_down2_kernel (conv_time_down_bf16.hip).  Implicit GEMM over
// channels-last activations, fp32 accumulation on v_mfma_f32_16x16x32_bf16, bias (+ a per-kernel hook) and bf16 output.  Each kernel
// keeps what is particular to its layer — the output-voxel -> source-row map with its edge flags, the tile's lowest source row, the
// byte offset of a tap — and plugs it into the pieces below; ONE copy of the tile prologue, the padding masks, the k-tile counter, the
// pipelined k-loop, the epilogue and the host refusals lives here.
//
// Split (the choice a stride forces): PER-ROW DMA ADDRESSES FROM AN OUTPUT-VOXEL -> SOURCE-ROW MAP, not whole source rows in LDS.  A tile
// is 256 consecutive output voxels of ONE sample x 128 output channels.  Every DMA lane owns one output voxel per 16-row group
// (Tile::dma_voxel) and computes ONCE the byte offset of the source row its reference tap reads, relative to the tile's LOWEST source
// row, where the buffer resource starts (rows_rsrc), so offsets are >= 0.  A tap is then the same row shift for the whole tile, as in
// conv_bf16.hip — except on the voxels whose tap leaves the grid: there the ADDRESS is clamped to a neighbouring tap that is always a
// voxel of the grid (the kernel's a_voff) and the FRAGMENT is replaced by zeros in registers before its MFMAs (zero_if under the
// kernel's pad_mask over frag_masks: a select, not a multiply, so whatever the clamped row holds never reaches a result).  So the
// padding comes from the addressing: the source is read where it lies (any VaeGrid: a conv-output grid with junk borders, a dense
// one), no padded copy of the activation is made, and nothing but voxels of the grid is ever read.  LDS holds the staged k-tiles
// exactly as in conv_bf16.hip (16-byte chunk swizzle on the source side, Tile::dchunk; fragments straight from the image, Tile::fsw),
// so fragment reads are not strided.  Whole source rows in LDS would move 4x the bytes the MFMAs use through the DMA path (two of
// three rows, both column parities) and tie the tile shape to W.
//
// Geometry: that of conv_kernel<0, 1>.  4 waves (2 x 2), wave tile 128 voxels x 64 channels = 8 x 4 accumulators of 16 x 16, BK = 32,
// 256 threads, two workgroups per CU (<= 256 VGPRs, no scratch: pinned by tests/test_build_resources_conv_*down.py).  k runs
// tap-major: (time tap, kh, kw) outermost to innermost, then the channel chunks of 32, the order of conv_bf16.hip; cin is any multiple of
// 32 (KTile carries the tap / chunk counters, nothing is divided out).  k_loop is the pipeline of three A slots + two W slots = 64 KiB
// of LDS: while k-tile t is multiplied, the W image of t + 1 and the A image of t + 2 are fetched, their DMA pieces slotted between
// the token blocks' MFMAs; one barrier a k-tile.  conv_pool_down2_kernel has two A images a stage and a sum in front of its MFMAs, a
// different pipeline: it keeps its own loop and takes everything else from here.
//
// Epilogue (store_tile_bf16): bias quads, bf16 through a per-wave LDS image in two passes of 64 rows, global stores of whole 128-byte
// row segments.  Between the bias add and the rounding a kernel may change the four fp32 values of an accumulator quad (the hook).
// The three sources are compiled without packed fp32 instructions (__graft_entry__.py SOURCE_FLAGS): the epilogue's adds are four
// independent fp32 adds per lane, which the compiler may otherwise pair into v_pk_add_f32; single operations keep the output bits
// independent of that choice.
//
// Host side: refuse_grid / refuse_align are the refusals the three launchers have in common; each launcher keeps the order of its
// checks (the error code of an input that fails two of them depends on it) and its own source-span formula.
#pragma once
#include "common.h"
#include "vsys_internal.h"

namespace vsys {
namespace ct16 {

constexpr int BM = 256, BN = 128, BK = 32;
constexpr int A_SLOT = BM * BK * 2;   // 16384: the image of one k-tile of the activation
constexpr int W_SLOT = BN * BK * 2;   // 8192: of the weight panel
constexpr int W_BASE = 3 * A_SLOT;    // 49152
constexpr int LDS_BYTES = W_BASE + 2 * W_SLOT;  // 65536: k_loop's three A slots + two W slots
constexpr int OUT_ROW_BYTES = 64 * 2 + 16;
constexpr int OUT_WAVE_BYTES = 64 * OUT_ROW_BYTES;  // 9216 per wave and pass
static_assert(4 * OUT_WAVE_BYTES <= LDS_BYTES, "epilogue image must fit in the staging buffers");
static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");

#if __HIP_DEVICE_COMPILE__  // buffer-resource types exist in the device pass only

__device__ __forceinline__ bf16x8 zero_if(bf16x8 v, bool z) {
  uint4 u = __builtin_bit_cast(uint4, v);
  u.x = z ? 0u : u.x; u.y = z ? 0u : u.y; u.z = z ? 0u : u.z; u.w = z ? 0u : u.w;
  return __builtin_bit_cast(bf16x8, u);
}

// who this lane is and which tile its workgroup owns: N output channels in column tiles of BN (gridDim.x = row tiles x column tiles, XCD
// remapped), the sample in blockIdx.y
struct Tile {
  int lane, wave, wave_u;   // wave_u: the wave index in a scalar register
  int wm, wn, l15, lq;      // the wave's place in the 2 x 2 grid; the lane's place in a 16 x 16 fragment
  int row0, col0;           // first output voxel (of the sample) and first output channel of the tile
  int64_t zb;               // sample
  int dchunk, fsw;          // 16-byte chunk swizzle of a DMA lane (source side) and of a fragment read
  int b_off[2];             // byte offset of this lane's two weight rows inside the tile's panel

  // output voxel of DMA group i (0..3) / of token block i (0..7) of this lane; rows past M re-read the last voxel (never stored)
  __device__ __forceinline__ int dma_voxel(int i, int M) const {
    const int r = row0 + wave_u * 64 + i * 16 + (lane >> 2);
    return r < M ? r : M - 1;
  }
  __device__ __forceinline__ int frag_voxel(int i, int M) const {
    const int r = row0 + wm * 128 + i * 16 + l15;
    return r < M ? r : M - 1;
  }
  // where the lane reads its fragments inside an A image (+ i*1024 for token block i) / a W image (+ j*1024 for column block j)
  __device__ __forceinline__ int frag_x() const { return (wm * 128 + l15) * 64 + fsw; }
  __device__ __forceinline__ int frag_w() const { return (wn * 64 + l15) * 64 + fsw; }
};

__device__ __forceinline__ Tile make_tile(int N, int64_t ldw) {
  Tile t;
  const int tid = threadIdx.x;
  t.lane = tid & 63; t.wave = tid >> 6;
  t.wm = t.wave >> 1; t.wn = t.wave & 1;
  t.l15 = t.lane & 15; t.lq = t.lane >> 4;
  t.wave_u = __builtin_amdgcn_readfirstlane(t.wave);
  const int nbn = N / BN;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int bm = tile / nbn, bn = tile - bm * nbn;
  t.row0 = bm * BM; t.col0 = bn * BN;
  t.zb = blockIdx.y;
  t.dchunk = ((t.lane & 3) ^ ((0x78 >> (2 * ((t.lane >> 4) & 3))) & 3)) * 16;
#pragma unroll
  for (int i = 0; i < 2; ++i) t.b_off[i] = (t.wave_u * 32 + i * 16 + (t.lane >> 2)) * (int)ldw * 2 + t.dchunk;
  t.fsw = (t.lq ^ ((0x78 >> (2 * ((t.l15 >> 2) & 3))) & 3)) << 4;
  return t;
}

// buffer resource over rows [row, rows) of a matrix of ld elements a row whose last row has `width` elements: from the row where the
// tile's offsets start to the end of the operand's last row (2 GiB at the most: tile-relative offsets are 32-bit)
__device__ __forceinline__ auto rows_rsrc(const bf16_t* base, int64_t row, int64_t rows, int64_t ld, int width) {
  const int64_t bytes = ((rows - 1 - row) * ld + width) * 2;
  return __builtin_amdgcn_make_buffer_rsrc((void*)(base + row * ld), 0, (int)(bytes < 0x7fffffff ? bytes : 0x7fffffff), 0x00020000);
}

typedef __attribute__((address_space(3))) void* lds_ptr_t;
// LDS-DMA of 16 bytes a lane: DMA group i (16 voxels, 0..3) of a k-tile's A image from this lane's row offset voff and channel chunk kc,
// group i (16 channels, 0..1) of the W image of k-tile t
template <class Rsrc>
__device__ __forceinline__ void dma_a(Rsrc rsrc_a, char* img, const Tile& tl, int i, int voff, int kc) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, (lds_ptr_t)(img + (tl.wave_u * 64 + i * 16) * 64), 16, voff, kc * (BK * 2), 0, 0);
}
template <class Rsrc>
__device__ __forceinline__ void dma_w(Rsrc rsrc_b, char* img, const Tile& tl, int i, int t) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_b, (lds_ptr_t)(img + (tl.wave_u * 32 + i * 16) * 64), 16, tl.b_off[i], t * (BK * 2), 0, 0);
}

// which of this lane's eight fragment voxels (16 i + l15 of the wave's 128) lose a tap to the padding: flags_of(voxel) gives the voxel's
// edge flags, bit 0 the kernel's own (first frame) and bits 1 .. NB one edge each; m[e] has bit i set when token block i's voxel has edge e
template <int NB>
struct FragMasks {
  int m[NB];
};
template <int NB, class FlagsOf>
__device__ __forceinline__ FragMasks<NB> frag_masks(const Tile& tl, int M, FlagsOf flags_of) {
  FragMasks<NB> r;
#pragma unroll
  for (int e = 0; e < NB; ++e) r.m[e] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int f = flags_of(tl.frag_voxel(i, M));
#pragma unroll
    for (int e = 0; e < NB; ++e) r.m[e] |= ((f >> (e + 1)) & 1) << i;
  }
  return r;
}

// k-tile counters (time tap, kh, kw, channel chunk), carried: cin / 32 need not be a power of two.  A kernel without time taps runs out
// of k-tiles before a leaves 0.
struct KTile {
  int a = 0, b = 0, c = 0, kc = 0;
  __device__ __forceinline__ void advance(int nkc) {
    if (++kc == nkc) {
      kc = 0;
      if (++c == 3) {
        c = 0;
        if (++b == 3) { b = 0; ++a; }
      }
    }
  }
};

__device__ __forceinline__ void zero_acc(f32x4 (&acc16)[8][4]) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc16[i][j][r] = 0.f;
}

// acc16 += the tile's nt k-tiles, three A slots and two W slots in smem[LDS_BYTES].  a_voff(i, a, b, c): byte offset of this lane's source
// row for tap (a, b, c) of DMA group i; pad_mask(b, c): the token blocks (bits 0..7) whose tap (., b, c) is padding.
template <class Rsrc, class AVoff, class PadMask>
__device__ __forceinline__ void k_loop(char* smem, const Tile& tl, Rsrc rsrc_a, Rsrc rsrc_b, int nt, int nkc, AVoff a_voff, PadMask pad_mask,
                                       f32x4 (&acc16)[8][4]) {
  auto fetch_a = [&](int i, int voff, int kc, int slot) { dma_a(rsrc_a, smem + slot * A_SLOT, tl, i, voff, kc); };
  auto fetch_w = [&](int i, int t, int slot) { dma_w(rsrc_b, smem + W_BASE + slot * W_SLOT, tl, i, t); };
  const int xo = tl.frag_x(), wo_ = W_BASE + tl.frag_w();

  KTile pf, mul;   // the k-tile being fetched / being multiplied (of which only kh and kw are read)
#pragma unroll
  for (int i = 0; i < 4; ++i) fetch_a(i, a_voff(i, pf.a, pf.b, pf.c), pf.kc, 0);
#pragma unroll
  for (int i = 0; i < 2; ++i) fetch_w(i, 0, 0);
  pf.advance(nkc);
  if (nt > 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) fetch_a(i, a_voff(i, pf.a, pf.b, pf.c), pf.kc, 1);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  pf.advance(nkc);
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  int sa = 0, sw = 0;
  for (int t = 0; t < nt; ++t) {
    const int sa1 = sa == 2 ? 0 : sa + 1, sa2 = sa1 == 2 ? 0 : sa1 + 1, sw1 = sw ^ 1;
    const bool n1 = t + 1 < nt, n2 = t + 2 < nt;
    int v2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v2[i] = a_voff(i, pf.a, pf.b, pf.c);
    const int k2 = pf.kc;
    const int mz = pad_mask(mul.b, mul.c);   // fragment voxels whose tap is padding
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
    if (n1) { fetch_w(0, t + 1, sw1); fetch_w(1, t + 1, sw1); }
    __builtin_amdgcn_sched_barrier(0);
    CT16_ROW(1, x1);
    __builtin_amdgcn_sched_barrier(0);
    x1 = *reinterpret_cast<const bf16x8*>(ab + xo + 5120);
    if (n2) { fetch_a(0, v2[0], k2, sa2); fetch_a(1, v2[1], k2, sa2); }
    __builtin_amdgcn_sched_barrier(0);
    CT16_ROW(2, x2);
    __builtin_amdgcn_sched_barrier(0);
    x2 = *reinterpret_cast<const bf16x8*>(ab + xo + 6144);
    if (n2) fetch_a(2, v2[2], k2, sa2);
    __builtin_amdgcn_sched_barrier(0);
    CT16_ROW(3, x3);
    __builtin_amdgcn_sched_barrier(0);
    x3 = *reinterpret_cast<const bf16x8*>(ab + xo + 7168);
    if (n2) fetch_a(3, v2[3], k2, sa2);
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
    pf.advance(nkc);
    mul.advance(nkc);
  }
}

struct NoHook {
  __device__ __forceinline__ void operator()(int, int, int, float (&)[4]) const {}
};

// out[zb M + voxel, col0 ..] = bf16(hook(acc16 + bias)) through a per-wave LDS image at the start of smem (two passes of 64 rows), so the
// global stores are whole 128-byte row segments; element (voxel 16 i + l15, channel 16 j + 4 lq + r) of the wave's tile sits in
// acc16[i][j][r].  hook(i, j, row, v): v = the quad's four fp32 values with the bias added, row = its voxel's index in the sample (which
// may lie past M in a ragged tile: such rows are not stored); what it leaves in v is rounded once.  Every wave must be past its last
// read of the staging buffers (the k-loop's closing barrier).
template <class Hook>
__device__ __forceinline__ void store_tile_bf16(char* smem, const Tile& tl, const f32x4 (&acc16)[8][4], const bf16_t* bias, bf16_t* out,
                                                int64_t ldo, int M, Hook hook) {
  // the lane's fields are derived again from an opaque copy of the thread index: what the epilogue computes from them is then
  // computed here, behind the k-loop, and only the index itself is carried through the loop beside the 128 accumulators (as a plain
  // reuse of tl's fields the compiler hoists the epilogue's address arithmetic in front of the loop: three more VGPRs at its peak)
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63, l15 = lane & 15, lq = lane >> 4, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int ncol0 = tl.col0 + wn * 64;
  bf16_t* ob = out + tl.zb * (int64_t)M * ldo;
  char* st = smem + wave * OUT_WAVE_BYTES;
  uint2 bb16[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    bb16[j] = bias != nullptr ? *reinterpret_cast<const uint2*>(bias + ncol0 + j * 16 + 4 * lq) : make_uint2(0, 0);
#pragma unroll
  for (int ih = 0; ih < 2; ++ih) {
    const int wrow0 = tl.row0 + wm * 128 + ih * 64;
#pragma unroll
    for (int i2 = 0; i2 < 4; ++i2) {
      const int i = ih * 4 + i2;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc16[i][j][r];
        v[0] += bflo(bb16[j].x); v[1] += bfhi(bb16[j].x); v[2] += bflo(bb16[j].y); v[3] += bfhi(bb16[j].y);
        hook(i, j, wrow0 + i2 * 16 + l15, v);
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
      if (grow < M) *reinterpret_cast<uint4*>(ob + grow * ldo + ncol0 + (q & 7) * 8) = val[it];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // image reads done before the next pass overwrites it
    __builtin_amdgcn_wave_barrier();
  }
}

#endif  // __HIP_DEVICE_COMPILE__

// Host side.  The source grid as the kernels address it: padded row and plane pitch in rows, row of voxel (0, 0, 0) inside a sample.
struct SrcGrid {
  int64_t Wp = 0, plane = 0, row00 = 0;
};

// VSYS_ERR_SHAPE for a grid the kernels cannot walk (T < 1, H or W < 2, negative borders, a sample_rows below the grid's frames or past
// 32 bits, more than 65535 samples: the sample is gridDim.y); 0 and the pitches otherwise
inline int refuse_grid(const VaeGrid& g, int64_t nsamples, SrcGrid& s) {
  if (g.T < 1 || g.H < 2 || g.W < 2 || g.pad < 0 || g.tf < 0 || nsamples < 0 || nsamples > 65535) return VSYS_ERR_SHAPE;
  const int64_t Hp = g.H + 2 * g.pad;
  s.Wp = g.W + 2 * g.pad;
  s.plane = Hp * s.Wp;
  s.row00 = (g.tf * Hp + g.pad) * s.Wp + g.pad;
  if ((g.T + g.tf) * s.plane > g.sample_rows || g.sample_rows > 0x7fffffff) return VSYS_ERR_SHAPE;
  return 0;
}

inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// VSYS_ERR_ALIGN for strides that are no multiple of 8 elements (16-byte DMA chunks and row stores) or pointers off the 16-byte grid (the
// bias: 8 bytes, a quad); a launcher without weights passes w = nullptr, ldw = 0
inline int refuse_align(const bf16_t* x, int64_t ldx, const bf16_t* w, int64_t ldw, const bf16_t* bias, const bf16_t* out, int64_t ldo) {
  if ((ldx % 8) || (ldw % 8) || (ldo % 8)) return VSYS_ERR_ALIGN;
  if (!aligned16(x) || !aligned16(w) || !aligned16(out) || (reinterpret_cast<uintptr_t>(bias) & 7)) return VSYS_ERR_ALIGN;
  return 0;
}

}  // namespace ct16
}  // namespace vsys
