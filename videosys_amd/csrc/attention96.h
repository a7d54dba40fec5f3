// Attention kernels for head_dim 96 (Open-Sora-Plan v1.2: 24 x 96 = 2304) on gfx950.
//
// Reference call sites replaced (videosys/models/transformers/open_sora_plan_v120_transformer_3d.py): AttnProcessor2_0.__call__
//   :886-1128 — full 3-D self-attention with RoPE3D on q and k (:63-118: the 96 head columns are three chunks of 32 for the frame,
//   row and column position; inside a chunk out = x cos + rotate_half(x) sin, rotate_half = (-x[16:32], x[0:16])), and the masked
//   cross-attention over the text keys, both F.scaled_dot_product_attention at scale 96^-0.5.
//
// Geometry: v_mfma_f32_16x16x32_bf16 in the swapped form S^T = K Q^T, O^T = V^T P^T, so a query is one MFMA COLUMN: its logits
// live in the four lanes {n, n+16, n+32, n+48} and the row maximum / sum are two cross-lane steps.  96 = 3 x 32 is the exact K
// depth of Q K^T (3 MFMAs per 16 keys) and 6 x 16 output rows of P V (6 MFMAs per 32 keys): no padding MFMAs.  A wave owns 32
// query rows (two column groups of 16) which share every K and V^T fragment read from LDS; a workgroup is 4 waves = 128 rows.
// K rows are permuted when they are read (MFMA row 4g + r of the 16-key tile tau of a 32-key group is key 8g + 4 tau + r), so that
// the 8 probabilities a lane holds after two tiles are 8 CONSECUTIVE keys = its B-operand slice of the P V MFMA, with no shuffle.
// K / V^T tiles of 64 keys go global -> registers (under the previous tile's MFMAs) -> LDS; one LDS stage of 26.5 KiB.
//
// Rounding contract (tests/test_gpu_osp_attention.py):
//   q^ = bf16(fp32(q cos) + fp32(rot(q) sin))                      two fp32 products, one fp32 sum, one rounding (no fma)
//   k^ = bf16((fp32(k cos) + fp32(rot(k) sin)) * 96^-0.5 log2(e))  the same, the softmax scale rides on K before the one rounding
//   s = q^ . k^ in fp32 (MFMA), p = exp2(s - m) with the running maximum m, P rounded to bf16 for P V, the row sum taken from the
//   fp32 p, O accumulated in fp32, one division, one rounding of the output.
//
// This header holds the ONE body of each kernel, templated on how the row of token s is found (row96 below).  attention96.hip
// instantiates the plain addressing (vsys_attn_prep_kv96, vsys_flash_attn_d96), attention96_img.hip the two-level addressing of a
// sequence-parallel receive / send image (vsys_attn_prep_kv96_img, vsys_flash_attn_d96_img): same arithmetic, tile walk, LDS use and
// rounding, hence the same bits.
#pragma once
#include "common.h"
#include "vsys_internal.h"

namespace vsys {
namespace {

// Where token s of sample b lies.  IMG = false: row b * len + s.  IMG = true: the tokens lie in slabs of seg_len (slab = the rank the
// tokens came from, or go to), row (s / seg_len) * slab_rows + b * seg_len + s % seg_len.  One integer division per ROW (the Q prologue
// and the output epilogue of the flash kernel, the token row of the prep kernel), never inside the key loop.
template <bool IMG>
__device__ __forceinline__ int64_t row96(int b, int s, int len, int seg_len, int64_t slab_rows) {
  if constexpr (IMG) {
    const int slab = s / seg_len;
    return (int64_t)slab * slab_rows + (int64_t)b * seg_len + (s - slab * seg_len);
  } else {
    return (int64_t)b * len + s;
  }
}

constexpr int HD = 96;
constexpr int KPITCH = 208;                    // bytes per K row in LDS (192 + 16 pad)
constexpr int VPITCH = 144;                    // bytes per V^T row in LDS (64 keys = 128 + 16 pad)
constexpr int K_LDS = 64 * KPITCH;             // 13312
constexpr int V_LDS = HD * VPITCH;             // 13824
constexpr float NEG_BIG = -1.0e30f;
constexpr float KSCALE = 0.10206207261596575f * 1.4426950408889634f;   // 96^-0.5 * log2(e)

// one 8-column slice of the RoPE3D rotation: x = the slice, xp = the partner slice (16 columns up for the lower half of a 32-chunk,
// 16 down for the upper half), sgn = -1 / +1 accordingly.  Two products, one sum, each rounded to fp32 (no contraction).
__device__ __forceinline__ void rope8(float* x, const float* xp, const float* cs, const float* sn, float sgn) {
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = __fadd_rn(__fmul_rn(x[e], cs[e]), __fmul_rn(sgn * xp[e], sn[e]));
}
__device__ __forceinline__ void load8f(const float* p, float* f) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

// ---------------------------------------------------------------------------------------------------------
// attn_prep_kv96: k, v rows (strided, heads interleaved) ->
//   Kp[batch][H][kv_pad][96]  RoPE3D (optional) + softmax scale, plain rows; keys >= kv_len are zero
//   Vt[batch][H][96][kv_pad]  transposed; keys >= kv_len are zero
// grid: (kv_pad/64, batch*H); block 256 = 64 token rows x 4 lanes; lane ``part`` owns columns 32c + 8 part .. + 8, c = 0..2.
// ---------------------------------------------------------------------------------------------------------
template <bool IMG>
__device__ __forceinline__ void attn_prep_kv96_body(const bf16_t* __restrict__ k, int64_t k_stride, const bf16_t* __restrict__ v,
                                                    int64_t v_stride, const float* __restrict__ rope_cos,
                                                    const float* __restrict__ rope_sin, bf16_t* __restrict__ kp, bf16_t* __restrict__ vt,
                                                    int heads, int kv_len, int kv_pad, int seg_len, int64_t slab_rows) {
  __shared__ __attribute__((aligned(16))) bf16_t vs[64][HD + 8];  // [token][d], 208-byte rows
  const int tid = threadIdx.x;
  const int s0 = blockIdx.x * 64;
  const int bh = blockIdx.y;
  const int b = bh / heads, h = bh - b * heads;
  const int r = tid >> 2, part = tid & 3;
  const int s = s0 + r;
  const bool live = s < kv_len;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int col = 32 * c + 8 * part;
    uint4 vv = make_uint4(0, 0, 0, 0), kk = vv;
    if (live) {
      const int64_t row = row96<IMG>(b, s, kv_len, seg_len, slab_rows);
      vv = *reinterpret_cast<const uint4*>(v + row * v_stride + h * HD + col);
      const bf16_t* krow = k + row * k_stride + h * HD;
      float x[8];
      unpack8(*reinterpret_cast<const uint4*>(krow + col), x);
      if (rope_cos != nullptr) {
        float xp[8], cs[8], sn[8];
        unpack8(*reinterpret_cast<const uint4*>(krow + (col ^ 16)), xp);
        load8f(rope_cos + (int64_t)s * HD + col, cs);
        load8f(rope_sin + (int64_t)s * HD + col, sn);
        rope8(x, xp, cs, sn, part < 2 ? -1.0f : 1.0f);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = __fmul_rn(x[e], KSCALE);
      kk = pack8(x);
    }
    *reinterpret_cast<uint4*>(&vs[r][col]) = vv;
    *reinterpret_cast<uint4*>(kp + ((int64_t)bh * kv_pad + s) * HD + col) = kk;
  }
  __syncthreads();
  // ---- Vt rows: thread -> (d, 8-token chunk), 768 chunks
  for (int q = tid; q < HD * 8; q += 256) {
    const int d = q >> 3, c = q & 7;
    uint32_t w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = (uint32_t)vs[c * 8 + 2 * e][d] | ((uint32_t)vs[c * 8 + 2 * e + 1][d] << 16);
    uint4 o;
    o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
    *reinterpret_cast<uint4*>(vt + ((int64_t)bh * HD + d) * kv_pad + s0 + c * 8) = o;
  }
}

struct Flash96Params {
  const bf16_t* q; int64_t q_stride;      // q(b, s, h) at q + (b*q_len + s)*q_stride + h*96
  const float* rope_cos; const float* rope_sin;   // [q_len, 96] or null
  const bf16_t* kp;                        // [batch][H][kv_pad][96]
  const bf16_t* vt;                        // [batch][H][96][kv_pad]
  const int* kv_lens;                      // [batch] or null
  bf16_t* out; int64_t out_stride;
  int heads, q_len, kv_len, kv_pad, nqb;
};
// the image form: q and out are images with slabs of seg_len query tokens, each with its own slab stride (row96<true>)
struct Flash96ImgParams : Flash96Params {
  int seg_len;
  int64_t q_slab_rows, out_slab_rows;
};

// grid: ceil(q_len/128) * batch * heads workgroups of 4 waves x 32 query rows (1-D, XCD-remapped so the q-blocks of one
// (batch, head) share an L2).
// (the KERNEL is the template, not a device function it calls: handing the by-value parameter block to an inlined body changed the
// register allocation of the plain instantiation, and that one must stay the code it was, instruction for instruction)
template <bool IMG, class Params>
__global__ __launch_bounds__(256, 2) void flash_attn_d96_kernel(Params p) {
  __shared__ __attribute__((aligned(16))) char smem[K_LDS + V_LDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int tile_id = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = tile_id / p.nqb;
  const int qb = tile_id - bh * p.nqb;
  const int b = bh / p.heads, h = bh - b * p.heads;
  const int q0 = qb * 128 + wave * 32;
  // keys this sample attends to: the count in device memory (a replayed launch carries no count), never past kv_len
  int eff = p.kv_len;
  if (p.kv_lens != nullptr) {
    const int c = p.kv_lens[b];
    eff = c < eff ? c : eff;
  }

  // ---- Q fragments (B operand, 32 dims x 16 queries): lane holds Q[q0 + 16 qg + n][32c + 8g .. + 8]; RoPE3D applied here
  bf16x8 qf[2][3];
#pragma unroll
  for (int qg = 0; qg < 2; ++qg) {
    int qs = q0 + 16 * qg + n;
    qs = qs < p.q_len ? qs : p.q_len - 1;
    int64_t row;
    if constexpr (IMG) row = row96<true>(b, qs, p.q_len, p.seg_len, p.q_slab_rows);
    else row = (int64_t)b * p.q_len + qs;
    const bf16_t* qrow = p.q + row * p.q_stride + h * HD;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int col = 32 * c + 8 * g;
      float x[8];
      unpack8(*reinterpret_cast<const uint4*>(qrow + col), x);
      if (p.rope_cos != nullptr) {
        float xp[8], cs[8], sn[8];
        unpack8(*reinterpret_cast<const uint4*>(qrow + (col ^ 16)), xp);
        load8f(p.rope_cos + (int64_t)qs * HD + col, cs);
        load8f(p.rope_sin + (int64_t)qs * HD + col, sn);
        rope8(x, xp, cs, sn, g < 2 ? -1.0f : 1.0f);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) qf[qg][c][e] = (__bf16)x[e];
    }
  }

  // ---- K / V^T tile staging: 768 + 768 16-byte pieces per 64-key tile, three of each per thread
  const bf16_t* kbase = p.kp + (int64_t)bh * p.kv_pad * HD;
  const bf16_t* vbase = p.vt + (int64_t)bh * HD * p.kv_pad;
  // (named registers and macros, not arrays behind lambdas: the compiler kept the arrays in scratch)
  uint4 kreg0, kreg1, kreg2, vreg0, vreg1, vreg2;
#define FLASH96_FETCH1(i_, t_)                                                                                                 \
  {                                                                                                                            \
    const int piece = tid + 256 * (i_); /* K: row piece / 12, 16-byte chunk piece % 12 (the rows of a tile are contiguous) */  \
    kreg##i_ = *reinterpret_cast<const uint4*>(kbase + (int64_t)(t_) * 64 * HD + piece * 8);                                   \
    const int d = piece >> 3, ch = piece & 7; /* V^T: row d, keys t*64 + 8 ch .. + 8 */                                        \
    vreg##i_ = *reinterpret_cast<const uint4*>(vbase + (int64_t)d * p.kv_pad + (t_) * 64 + ch * 8);                            \
  }
#define FLASH96_COMMIT1(i_)                                                                \
  {                                                                                        \
    const int piece = tid + 256 * (i_);                                                    \
    const int kr = piece / 12, kc = piece - kr * 12;                                       \
    *reinterpret_cast<uint4*>(smem + kr * KPITCH + kc * 16) = kreg##i_;                    \
    const int d = piece >> 3, ch = piece & 7;                                              \
    *reinterpret_cast<uint4*>(smem + K_LDS + d * VPITCH + ch * 16) = vreg##i_;             \
  }
// (ONE statement each: as the body of an unbraced `if` all three pieces stay behind the condition — a tile past the last one is
// never fetched, so no load leaves the (batch, head) image)
#define FLASH96_FETCH(t_) do { FLASH96_FETCH1(0, t_) FLASH96_FETCH1(1, t_) FLASH96_FETCH1(2, t_) } while (0)
#define FLASH96_COMMIT() do { FLASH96_COMMIT1(0) FLASH96_COMMIT1(1) FLASH96_COMMIT1(2) } while (0)
  // K fragment (A operand, 16 keys x 32 dims) of tile tau of 32-key group kk: row 32 kk + 8 (n >> 2) + 4 tau + (n & 3), dims 32c + 8g
  const int k_roff = (8 * (n >> 2) + (n & 3)) * KPITCH + 16 * g;
  // V^T fragment (A operand, 16 dims x 32 keys) of output tile dt, group kk: row 16 dt + n, keys 32 kk + 8g .. + 8
  const int v_roff = K_LDS + n * VPITCH + 16 * g;

  f32x4 o[2][6];
#pragma unroll
  for (int qg = 0; qg < 2; ++qg)
#pragma unroll
    for (int dt = 0; dt < 6; ++dt) o[qg][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[2] = {NEG_BIG, NEG_BIG}, l_run[2] = {0.f, 0.f};

  const int ntiles = (eff + 63) / 64;
  if (ntiles > 0) {
    FLASH96_FETCH(0);
  }
  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();          // every wave is done reading tile t - 1
    FLASH96_COMMIT();
    __syncthreads();
    if (t + 1 < ntiles) {
      FLASH96_FETCH(t + 1);
    }
    // ---- S^T = K Q^T: s[qg][kk][tau] holds keys t*64 + 32 kk + 8 g + 4 tau + r of query column n
    f32x4 s[2][2][2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int tau = 0; tau < 2; ++tau) {
        s[0][kk][tau] = f32x4{0.f, 0.f, 0.f, 0.f};
        s[1][kk][tau] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(smem + k_roff + (32 * kk + 4 * tau) * KPITCH + 64 * c);
          s[0][kk][tau] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[0][c], s[0][kk][tau], 0, 0, 0);
          s[1][kk][tau] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[1][c], s[1][kk][tau], 0, 0, 0);
        }
      }
    if (t == ntiles - 1 && (eff & 63)) {
      const int lim = eff - t * 64 - 8 * g;      // lane-local key index 32 kk + 4 tau + r is live below this
#pragma unroll
      for (int qg = 0; qg < 2; ++qg)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int tau = 0; tau < 2; ++tau)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (32 * kk + 4 * tau + r >= lim) s[qg][kk][tau][r] = NEG_BIG;
    }
    // ---- online softmax per query column
    bf16x8 pf[2][2];
#pragma unroll
    for (int qg = 0; qg < 2; ++qg) {
      float mx = s[qg][0][0][0];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int tau = 0; tau < 2; ++tau)
#pragma unroll
          for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[qg][kk][tau][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run[qg], mx);
      // the maximum moved for some query of the wave (always in the first tile, rarely later): rescale.  Otherwise alpha is exactly
      // 1 in every lane and the 25 multiplies below would change no bit — the branch is wave-uniform
      const bool moved = __builtin_amdgcn_ballot_w64(m_new > m_run[qg]) != 0;
      const float alpha = __builtin_amdgcn_exp2f(m_run[qg] - m_new);   // first tile: exp2(-1e30) = 0 on zero accumulators
      m_run[qg] = m_new;
      float lsum = 0.f;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int tau = 0; tau < 2; ++tau)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float pv = __builtin_amdgcn_exp2f(s[qg][kk][tau][r] - m_new);
            lsum += pv;
            pf[qg][kk][4 * tau + r] = (__bf16)pv;
          }
      if (moved) {
        l_run[qg] *= alpha;
#pragma unroll
        for (int dt = 0; dt < 6; ++dt)
#pragma unroll
          for (int r = 0; r < 4; ++r) o[qg][dt][r] *= alpha;
      }
      l_run[qg] += lsum;
    }
    // ---- O^T += V^T P^T
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int dt = 0; dt < 6; ++dt) {
        const bf16x8 vf = *reinterpret_cast<const bf16x8*>(smem + v_roff + 16 * dt * VPITCH + 64 * kk);
        o[0][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[0][kk], o[0][dt], 0, 0, 0);
        o[1][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[1][kk], o[1][dt], 0, 0, 0);
      }
  }

#undef FLASH96_FETCH
#undef FLASH96_COMMIT
#undef FLASH96_FETCH1
#undef FLASH96_COMMIT1
  // ---- epilogue: O[q][d] = O^T[d][q] / l ; lane holds d = 16 dt + 4 g + r of query column n
#pragma unroll
  for (int qg = 0; qg < 2; ++qg) {
    float l_tot = l_run[qg];
    l_tot += __shfl_xor(l_tot, 16, 64);
    l_tot += __shfl_xor(l_tot, 32, 64);
    const float inv = 1.0f / l_tot;
    const int qs = q0 + 16 * qg + n;
    if (qs < p.q_len) {
      int64_t row;
      if constexpr (IMG) row = row96<true>(b, qs, p.q_len, p.seg_len, p.out_slab_rows);
      else row = (int64_t)b * p.q_len + qs;
      bf16_t* orow = p.out + row * p.out_stride + h * HD;
#pragma unroll
      for (int dt = 0; dt < 6; ++dt) {
        uint2 w;
        w.x = pack2bf(o[qg][dt][0] * inv, o[qg][dt][1] * inv);
        w.y = pack2bf(o[qg][dt][2] * inv, o[qg][dt][3] * inv);
        *reinterpret_cast<uint2*>(orow + 16 * dt + 4 * g) = w;
      }
    }
  }
}

template <class... T> inline bool aligned16(const T*... ptrs) { return ((((uintptr_t)ptrs & 15) == 0) && ...); }   // (null passes)

// ---- the host checks both translation units share (0 = launch)
inline int check_prep_kv96(const bf16_t* k, int64_t k_stride, const bf16_t* v, int64_t v_stride, const float* rope_cos,
                           const float* rope_sin, const bf16_t* kp, const bf16_t* vt, int batch, int heads, int kv_len, int kv_pad) {
  if (kv_pad % 64 != 0 || kv_pad < kv_len || (k_stride % 8) || (v_stride % 8) || k_stride < (int64_t)heads * HD ||
      v_stride < (int64_t)heads * HD || (int64_t)batch * heads > 65535)
    return VSYS_ERR_SHAPE;
  if ((rope_cos == nullptr) != (rope_sin == nullptr)) return VSYS_ERR_ARG;
  if (!aligned16(k, v, kp, vt, rope_cos, rope_sin)) return VSYS_ERR_ALIGN;   // 16-byte loads and stores of all of them
  return 0;
}

// fills ``p`` (the base part) and the grid size
inline int check_flash_d96(Flash96Params& p, int64_t& nblk, const bf16_t* q, int64_t q_stride, const float* rope_cos,
                           const float* rope_sin, const bf16_t* kp, const bf16_t* vt, const int* kv_lens, bf16_t* out,
                           int64_t out_stride, int batch, int heads, int q_len, int kv_len, int kv_pad) {
  if (kv_len <= 0 || kv_pad % 64 != 0 || kv_pad < kv_len || (q_stride % 8) || (out_stride % 4) || q_stride < (int64_t)heads * HD ||
      out_stride < (int64_t)heads * HD)
    return VSYS_ERR_SHAPE;
  if ((rope_cos == nullptr) != (rope_sin == nullptr)) return VSYS_ERR_ARG;
  // 16-byte loads of q, the tables and the K / V^T images; 8-byte stores to out; 4-byte loads of the counts
  if (!aligned16(q, kp, vt, rope_cos, rope_sin) || ((uintptr_t)out & 7) || ((uintptr_t)kv_lens & 3)) return VSYS_ERR_ALIGN;
  p.q = q; p.q_stride = q_stride; p.rope_cos = rope_cos; p.rope_sin = rope_sin; p.kp = kp; p.vt = vt; p.kv_lens = kv_lens;
  p.out = out; p.out_stride = out_stride; p.heads = heads; p.q_len = q_len; p.kv_len = kv_len; p.kv_pad = kv_pad;
  p.nqb = (q_len + 127) / 128;
  nblk = (int64_t)p.nqb * batch * heads;
  return nblk > 0x7fffffff ? VSYS_ERR_SHAPE : 0;
}

// the slab rule of the image entry points: with more than one slab, a slab holds at least batch * seg_len rows
inline bool slabs_ok(int batch, int len, int64_t seg_len, int64_t slab_rows) {
  return seg_len >= 1 && (seg_len >= len || slab_rows >= (int64_t)batch * seg_len);
}

}  // namespace
}  // namespace vsys
