// attn_temporal_d64: temporal self-attention of Vchitect-2.0 (sequence = the T frames of one token, head dim 64), the text tokens
// riding along as extra "pixels".
//
// Replaces (reference videosys): models/modules/attentions.py:705-764 without the projections — the concatenation of the
// video and the text rows (:723-725), the `(B T) S H C -> (B S) T H C` rearranges (:737,755), apply_rotary_emb (:654-665: interleaved
// pairs times cos / sin in fp32, cast back to bf16) and F.scaled_dot_product_attention (:750-752, scale 1/8, no qk-norm, no mask).
//
// Layout.  q, k, v and the output are rows ordered (b, t, s): the video rows (S per frame) and the text rows (L per frame) live in
// different tensors (they leave different GEMMs and enter different ones), each with its own row stride; head h at column 64 h.
// The frames of one token are S (or L) rows apart, so a problem never reads more than 128 contiguous bytes per frame and operand: what
// can be contiguous is the HEADS of a token.  One workgroup = one token (b, s') and four neighbouring heads (one per wave): the four
// waves read the same 512-byte piece of each row at the same time, 8 lanes x 16 bytes per head and frame (row-contiguous cooperative
// loads; the per-lane row loads of the first d72 kernels were what bound them).
//
// A wave keeps one query per lane (64 per pass): q as the 32 dwords of its rotated bf16 row, the output row as 64 fp32.  K and V pass
// through LDS 32 frames at a time (rotated K as bf16, exactly the reference's operand); every lane reads the SAME key row, so the LDS
// reads are broadcasts.  Scores, softmax and P V are fp32 on the VALU with a running maximum that is adopted once per 4 keys (online
// softmax: any T), P is never rounded.  Whether HBM or the VALU binds at 24 heads and T = 40 is unmeasured.
// Queries and outputs are staged through the same LDS (144-byte pitch: conflict-free 16-byte reads of one row per lane).
#include "common.h"
#include "vsys_internal.h"

namespace vsys {
namespace {

constexpr int T64_KC = 32;                       // frames of K / V per LDS chunk
constexpr int T64_QPITCH = 144;                  // bytes per staged q / output row (128 + 16)
constexpr int T64_WAVE_LDS = 64 * T64_QPITCH;    // 9216 >= 2 x 32 x 128 (the K and the V chunk)
constexpr int T64_V_OFF = T64_KC * 128;
constexpr float T64_NEG = -1e30f;

struct T64Params {
  const bf16_t *q_vid, *k_vid, *v_vid, *q_txt, *k_txt, *v_txt;
  int64_t q_vid_ld, k_vid_ld, v_vid_ld, q_txt_ld, k_txt_ld, v_txt_ld;
  const float *cos, *sin;
  bf16_t *o_vid, *o_txt;
  int64_t o_vid_ld, o_txt_ld;
  int B, T, S, L, heads, hgroups;
  // the exchange image (attn_temporal_d64_img_kernel only): frame t lies in slab t / Tl, at frame t % Tl of the slab's [B][Tl][n] rows
  int Tl;
  int64_t slab_vid, slab_txt;
};

// one rotary pair: (x0 + i x1)(c + i s) in fp32, back to bf16
__device__ __forceinline__ uint32_t t64_rot(uint32_t u, float c, float s) {
  const float x0 = bflo(u), x1 = bfhi(u);
  return pack2bf(x0 * c - x1 * s, x0 * s + x1 * c);
}
__device__ __forceinline__ uint4 t64_rope(uint4 u, const float* __restrict__ cos, const float* __restrict__ sin) {
  const float4 c = *reinterpret_cast<const float4*>(cos), s = *reinterpret_cast<const float4*>(sin);
  return make_uint4(t64_rot(u.x, c.x, s.x), t64_rot(u.y, c.y, s.y), t64_rot(u.z, c.z, s.z), t64_rot(u.w, c.w, s.w));
}

// IMG = false: rows (b, t, s).  IMG = true: the receive image of the frame -> token switch of a sequence-parallel step,
// [slab = source rank][b][t % Tl][s] with a slab stride in rows; T counts the real frames, so the tail of the last slab is never touched.
// Everything after the row address is the same code: same tile walk, same LDS use, same rounding, same bits.
template <bool IMG>
__device__ __forceinline__ void attn_temporal_d64_body(const T64Params& p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * T64_WAVE_LDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int piece = lane & 7, rsub = lane >> 3;      // cooperative loads: 8 lanes x 16 bytes = one head of one frame
  char* wl = smem + wave * T64_WAVE_LDS;
  const int64_t item = blockIdx.x;
  const int hg = (int)(item % p.hgroups);
  const int64_t tok = item / p.hgroups;
  const int SL = p.S + p.L, T = p.T;
  const int sp = (int)(tok % SL), b = (int)(tok / SL);
  const int head = hg * 4 + wave;
  const bool active = head < p.heads;               // (a wave without a head stages zeros and stores nothing; it keeps the barriers)
  const bool txt = sp >= p.S, rope = p.cos != nullptr;
  const int64_t n = txt ? p.L : p.S;                // rows per frame of this token's tensor
  const int64_t r0 = (int64_t)b * (IMG ? p.Tl : T) * n + (txt ? sp - p.S : sp);
  const int64_t slab = txt ? p.slab_txt : p.slab_vid;
  // row of frame t of this token (one division per 16-byte load in the image: 12 per lane and 32-key chunk, beside 2048 FMAs)
  auto frow = [&](int t) -> int64_t {
    if constexpr (IMG) {
      const int sl = t / p.Tl;
      return r0 + (int64_t)sl * slab + (int64_t)(t - sl * p.Tl) * n;
    } else {
      return r0 + (int64_t)t * n;
    }
  };
  const int64_t col = (int64_t)head * 64 + piece * 8;
  const int64_t qld = txt ? p.q_txt_ld : p.q_vid_ld, kld = txt ? p.k_txt_ld : p.k_vid_ld, vld = txt ? p.v_txt_ld : p.v_vid_ld,
                old = txt ? p.o_txt_ld : p.o_vid_ld;
  const bf16_t* qb = (txt ? p.q_txt : p.q_vid) + col;
  const bf16_t* kb = (txt ? p.k_txt : p.k_vid) + col;
  const bf16_t* vb = (txt ? p.v_txt : p.v_vid) + col;
  bf16_t* ob = (txt ? p.o_txt : p.o_vid) + col;

  for (int q0 = 0; q0 < T; q0 += 64) {
    // ---- the pass's 64 queries: rows -> rotation -> LDS -> one row per lane
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = i * 8 + rsub, t = q0 + r;
      uint4 u = make_uint4(0, 0, 0, 0);
      if (active && t < T) {
        u = *reinterpret_cast<const uint4*>(qb + frow(t) * qld);
        if (rope) u = t64_rope(u, p.cos + t * 32 + piece * 4, p.sin + t * 32 + piece * 4);
      }
      *reinterpret_cast<uint4*>(wl + r * T64_QPITCH + piece * 16) = u;
    }
    __syncthreads();
    uint32_t qr[32];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const uint4 x = *reinterpret_cast<const uint4*>(wl + lane * T64_QPITCH + c * 16);
      qr[4 * c] = x.x; qr[4 * c + 1] = x.y; qr[4 * c + 2] = x.z; qr[4 * c + 3] = x.w;
    }
    __syncthreads();
    float o[64];
#pragma unroll
    for (int d = 0; d < 64; ++d) o[d] = 0.f;
    float m = T64_NEG, l = 0.f;
    for (int k0 = 0; k0 < T; k0 += T64_KC) {
      // ---- 32 frames of K (rotated) and V; frames past T are zero rows (their scores are masked, their P is 0)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = i * 8 + rsub, t = k0 + r;
        uint4 ku = make_uint4(0, 0, 0, 0), vu = make_uint4(0, 0, 0, 0);
        if (active && t < T) {
          ku = *reinterpret_cast<const uint4*>(kb + frow(t) * kld);
          vu = *reinterpret_cast<const uint4*>(vb + frow(t) * vld);
          if (rope) ku = t64_rope(ku, p.cos + t * 32 + piece * 4, p.sin + t * 32 + piece * 4);
        }
        *reinterpret_cast<uint4*>(wl + r * 128 + piece * 16) = ku;
        *reinterpret_cast<uint4*>(wl + T64_V_OFF + r * 128 + piece * 16) = vu;
      }
      __syncthreads();
      const int kn = T - k0 < T64_KC ? T - k0 : T64_KC;
      const int ngroups = (kn + 3) >> 2;             // every group holds at least one real key
      for (int g = 0; g < ngroups; ++g) {
        float s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const char* kr = wl + (g * 4 + j) * 128;
          float a0 = 0.f, a1 = 0.f;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const uint4 kk = *reinterpret_cast<const uint4*>(kr + c * 16);
            a0 = fmaf(bflo(qr[4 * c]), bflo(kk.x), a0);     a1 = fmaf(bfhi(qr[4 * c]), bfhi(kk.x), a1);
            a0 = fmaf(bflo(qr[4 * c + 1]), bflo(kk.y), a0); a1 = fmaf(bfhi(qr[4 * c + 1]), bfhi(kk.y), a1);
            a0 = fmaf(bflo(qr[4 * c + 2]), bflo(kk.z), a0); a1 = fmaf(bfhi(qr[4 * c + 2]), bfhi(kk.z), a1);
            a0 = fmaf(bflo(qr[4 * c + 3]), bflo(kk.w), a0); a1 = fmaf(bfhi(qr[4 * c + 3]), bfhi(kk.w), a1);
          }
          s[j] = g * 4 + j < kn ? (a0 + a1) * 0.125f : T64_NEG;
        }
        const float mn = fmaxf(fmaxf(m, fmaxf(s[0], s[1])), fmaxf(s[2], s[3]));
        const float alpha = __expf(m - mn);            // 0 on the first group (m = -1e30)
        m = mn;
        float pj[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) pj[j] = __expf(s[j] - mn);   // 0 for a masked key
        l = l * alpha + ((pj[0] + pj[1]) + (pj[2] + pj[3]));
#pragma unroll
        for (int d = 0; d < 64; ++d) o[d] *= alpha;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const char* vr = wl + T64_V_OFF + (g * 4 + j) * 128;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const uint4 vv = *reinterpret_cast<const uint4*>(vr + c * 16);
            o[8 * c] = fmaf(pj[j], bflo(vv.x), o[8 * c]);         o[8 * c + 1] = fmaf(pj[j], bfhi(vv.x), o[8 * c + 1]);
            o[8 * c + 2] = fmaf(pj[j], bflo(vv.y), o[8 * c + 2]); o[8 * c + 3] = fmaf(pj[j], bfhi(vv.y), o[8 * c + 3]);
            o[8 * c + 4] = fmaf(pj[j], bflo(vv.z), o[8 * c + 4]); o[8 * c + 5] = fmaf(pj[j], bfhi(vv.z), o[8 * c + 5]);
            o[8 * c + 6] = fmaf(pj[j], bflo(vv.w), o[8 * c + 6]); o[8 * c + 7] = fmaf(pj[j], bfhi(vv.w), o[8 * c + 7]);
          }
        }
      }
      __syncthreads();   // (every lane is done with the chunk: the next one, or the output rows, may land)
    }
    // ---- o / l -> bf16 -> LDS (one row per lane) -> cooperative row stores
    const float inv = 1.0f / l;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = o[8 * c + e] * inv;
      *reinterpret_cast<uint4*>(wl + lane * T64_QPITCH + c * 16) = pack8(f);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = i * 8 + rsub, t = q0 + r;
      if (active && t < T)
        *reinterpret_cast<uint4*>(ob + frow(t) * old) = *reinterpret_cast<const uint4*>(wl + r * T64_QPITCH + piece * 16);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256, 2) void attn_temporal_d64_kernel(const T64Params p) { attn_temporal_d64_body<false>(p); }
__global__ __launch_bounds__(256, 2) void attn_temporal_d64_img_kernel(const T64Params p) { attn_temporal_d64_body<true>(p); }

// the checks both entry points share; 0 or a VSYS_ERR code (a refused call launches nothing)
int t64_check(const void* const* ptrs, const int64_t* lds_v, const int64_t* lds_t, int B, int T, int S, int L, int heads) {
  if (B < 1 || T < 1 || S < 0 || L < 0 || (int64_t)S + L < 1 || heads < 1 || (int64_t)heads * 64 > 0x7fffffff) return VSYS_ERR_SHAPE;
  if ((ptrs[8] == nullptr) != (ptrs[9] == nullptr)) return VSYS_ERR_ARG;
  if (S > 0 && (!ptrs[0] || !ptrs[1] || !ptrs[2] || !ptrs[3])) return VSYS_ERR_ARG;
  if (L > 0 && (!ptrs[4] || !ptrs[5] || !ptrs[6] || !ptrs[7])) return VSYS_ERR_ARG;
  const int64_t width = (int64_t)heads * 64;
  for (int i = 0; i < 4; ++i) {
    if (S > 0 && lds_v[i] < width) return VSYS_ERR_SHAPE;
    if (L > 0 && lds_t[i] < width) return VSYS_ERR_SHAPE;
    if ((S > 0 && (lds_v[i] % 8)) || (L > 0 && (lds_t[i] % 8))) return VSYS_ERR_ALIGN;
  }
  for (int i = 0; i < 10; ++i)
    if (reinterpret_cast<uintptr_t>(ptrs[i]) % 16) return VSYS_ERR_ALIGN;
  const int64_t grid = (int64_t)B * ((int64_t)S + L) * ((heads + 3) / 4);
  if (grid > 0x7fffffff || (int64_t)T * 32 > 0x7fffffff) return VSYS_ERR_SHAPE;
  return 0;
}

}  // namespace

int launch_attn_temporal_d64(const bf16_t* q_vid, int64_t q_vid_ld, const bf16_t* k_vid, int64_t k_vid_ld, const bf16_t* v_vid,
                             int64_t v_vid_ld, const bf16_t* q_txt, int64_t q_txt_ld, const bf16_t* k_txt, int64_t k_txt_ld,
                             const bf16_t* v_txt, int64_t v_txt_ld, const float* rope_cos, const float* rope_sin, bf16_t* out_vid,
                             int64_t out_vid_ld, bf16_t* out_txt, int64_t out_txt_ld, int B, int T, int S, int L, int heads,
                             hipStream_t stream) {
  const int64_t lds_v[4] = {q_vid_ld, k_vid_ld, v_vid_ld, out_vid_ld}, lds_t[4] = {q_txt_ld, k_txt_ld, v_txt_ld, out_txt_ld};
  const void* ptrs[10] = {q_vid, k_vid, v_vid, out_vid, q_txt, k_txt, v_txt, out_txt, rope_cos, rope_sin};
  if (const int rc = t64_check(ptrs, lds_v, lds_t, B, T, S, L, heads)) return rc;
  const int hgroups = (heads + 3) / 4;
  const int64_t grid = (int64_t)B * ((int64_t)S + L) * hgroups;
  T64Params p;
  p.q_vid = q_vid; p.k_vid = k_vid; p.v_vid = v_vid; p.q_txt = q_txt; p.k_txt = k_txt; p.v_txt = v_txt;
  p.q_vid_ld = q_vid_ld; p.k_vid_ld = k_vid_ld; p.v_vid_ld = v_vid_ld; p.q_txt_ld = q_txt_ld; p.k_txt_ld = k_txt_ld; p.v_txt_ld = v_txt_ld;
  p.cos = rope_cos; p.sin = rope_sin;
  p.o_vid = out_vid; p.o_txt = out_txt; p.o_vid_ld = out_vid_ld; p.o_txt_ld = out_txt_ld;
  p.B = B; p.T = T; p.S = S; p.L = L; p.heads = heads; p.hgroups = hgroups;
  p.Tl = T; p.slab_vid = p.slab_txt = 0;
  hipLaunchKernelGGL(attn_temporal_d64_kernel, dim3((unsigned)grid), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

int launch_attn_temporal_d64_img(const bf16_t* q_vid, int64_t q_vid_ld, const bf16_t* k_vid, int64_t k_vid_ld, const bf16_t* v_vid,
                                 int64_t v_vid_ld, const bf16_t* q_txt, int64_t q_txt_ld, const bf16_t* k_txt, int64_t k_txt_ld,
                                 const bf16_t* v_txt, int64_t v_txt_ld, const float* rope_cos, const float* rope_sin, bf16_t* out_vid,
                                 int64_t out_vid_ld, bf16_t* out_txt, int64_t out_txt_ld, int B, int T, int Tl, int64_t slab_vid,
                                 int64_t slab_txt, int S, int L, int heads, hipStream_t stream) {
  const int64_t lds_v[4] = {q_vid_ld, k_vid_ld, v_vid_ld, out_vid_ld}, lds_t[4] = {q_txt_ld, k_txt_ld, v_txt_ld, out_txt_ld};
  const void* ptrs[10] = {q_vid, k_vid, v_vid, out_vid, q_txt, k_txt, v_txt, out_txt, rope_cos, rope_sin};
  if (const int rc = t64_check(ptrs, lds_v, lds_t, B, T, S, L, heads)) return rc;
  if (Tl < 1) return VSYS_ERR_SHAPE;
  if (T > Tl) {   // more than one slab: a slab holds its B x Tl frames, so slabs never overlap
    if (S > 0 && slab_vid < (int64_t)B * Tl * S) return VSYS_ERR_SHAPE;
    if (L > 0 && slab_txt < (int64_t)B * Tl * L) return VSYS_ERR_SHAPE;
  }
  const int hgroups = (heads + 3) / 4;
  const int64_t grid = (int64_t)B * ((int64_t)S + L) * hgroups;
  T64Params p;
  p.q_vid = q_vid; p.k_vid = k_vid; p.v_vid = v_vid; p.q_txt = q_txt; p.k_txt = k_txt; p.v_txt = v_txt;
  p.q_vid_ld = q_vid_ld; p.k_vid_ld = k_vid_ld; p.v_vid_ld = v_vid_ld; p.q_txt_ld = q_txt_ld; p.k_txt_ld = k_txt_ld; p.v_txt_ld = v_txt_ld;
  p.cos = rope_cos; p.sin = rope_sin;
  p.o_vid = out_vid; p.o_txt = out_txt; p.o_vid_ld = out_vid_ld; p.o_txt_ld = out_txt_ld;
  p.B = B; p.T = T; p.S = S; p.L = L; p.heads = heads; p.hgroups = hgroups;
  p.Tl = Tl; p.slab_vid = slab_vid; p.slab_txt = slab_txt;
  hipLaunchKernelGGL(attn_temporal_d64_img_kernel, dim3((unsigned)grid), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

}  // namespace vsys
