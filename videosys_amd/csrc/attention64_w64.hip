// flash_attn_d64_w64: joint [text | video] self-attention of CogVideoX (head_dim 64) with 64 query rows per wave and ONE wave per SIMD.
//
// Replaces (/root/reference/videosys): CogVideoXAttnProcessor2_0.__call__, models/transformers/cogvideox_transformer_3d.py:93-175 —
// LayerNorm qk-norm, rotary embedding on the video slice, F.scaled_dot_product_attention — the same contract and layouts (Kp / Vt of
// attn_prep_kv64) as flash_attn_d64_kernel (attention64.hip), for long key sequences without a bias table.
//
// The tile loop is the hand-allocated instruction stream of attention_w64.hip generated for this head size
// (csrc/gen/flash72_gen.py generate(d64=True) -> FLASH64_W64_ASM): 4 QK^T chunks instead of 5, K rows of 128 bytes with their
// chunks XOR-swizzled (four fragment address registers), 8 + 8 LDS-DMA pieces per tile (four per wave), and the THIRD 32-row block of
// the Vt image — in the d72 kernel the padding that carries the ones rows — kept constant in LDS (rows 72 / 76 = 1.0, the rest 0):
// the row sum of P rides on the matrix pipe, which has the slack here (40 MFMAs against ~190 VALU issues per tile), where
// flash_attn_d64_kernel adds it on the VALU.  At CogVideoX's 17 776 keys an item walks 278 tiles, so the one-item-per-workgroup
// form's seams (attention_w64.hip) do not matter.
//
// The register map (Q into / O out of the accumulator file, the statements' operand names) comes from the generator with the
// stream (FLASH64_W64_WRITE_Q_*, _READ_O_*, _OPERANDS in flash72_w64_map.inc); the variables the statement reads carry its
// operand names (the operand list binds by name).  Descriptors, fragment addressing, the row bound and the launch are flash_w64.h,
// shared with attention_w64.hip.
#include "flash_w64.h"

namespace vsys {
namespace {

using w64::VROW;
constexpr int HD = 64, KROW = 128;
constexpr int K_TILE_BYTES = 64 * KROW;              // 8192
constexpr int KV_STAGE = K_TILE_BYTES + 96 * VROW;   // 20480: K tile + Vt image of 96 rows (64 fetched + 32 constant)
constexpr int W64_STAGES = w64::STAGES;

struct Flash64W64Params {
  const bf16_t* q; int64_t q_stride;
  const bf16_t* ln_w; const bf16_t* ln_b;
  const float* rope_cos; const float* rope_sin; int rope_start, rope_len;
  const bf16_t* kp;
  const bf16_t* vt;
  bf16_t* out; int64_t out_stride;
  int heads, q_len, kv_len, kv_pad, nqb;
  float eps;
  float k_bound;   // VAR 5: upper bound on the norm of every Kp row (FlashW64Params::k_bound, attention_w64.hip)
};

// VAR: placement variant of the generated stream (flash72_gen.py body(): 1 = as the d72 kernel, 4 = one more P unit in the PV phase)
template <int VAR>
__global__ __launch_bounds__(256, 1) void flash_attn_d64_w64_kernel(Flash64W64Params p) {
#if __HIP_DEVICE_COMPILE__
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int tile_id = xcd_remap(blockIdx.x, gridDim.x);   // the q-blocks of one (batch, head) are consecutive on one XCD
  const int bh = tile_id / p.nqb, qb = tile_id - bh * p.nqb;
  const int b = bh / p.heads, h = bh - b * p.heads;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int q0 = qb * 256 + wave_u * 64;

  // ---- LDS-DMA assignment (as flash_attn_d64_kernel): 8 K pieces + 8 Vt pieces of 1 KiB per tile; wave w issues K pieces w, w + 4 and
  // Vt pieces w, w + 4 (rows 8 j + (lane >> 3), slot (lane & 7) holding logical slot (lane & 7) ^ ((row >> 1) & 7))
  const bf16_t* kbase = p.kp + (int64_t)bh * p.kv_pad * HD;
  const bf16_t* vbase = p.vt + (int64_t)bh * HD * p.kv_pad;
  const w64::u32x4 rk = w64::make_rsrc(kbase, (unsigned)(p.kv_pad * HD * 2)), rv = w64::make_rsrc(vbase, (unsigned)(HD * p.kv_pad * 2));
  const int kvo = lane * 16;
  const int vvo = ((lane >> 3) * p.kv_pad * 2 + (((lane & 7) ^ (lane >> 4)) << 4)) ^ ((wave_u & 1) << 6);
  const int wl = wave_u * 1024;
  const int sv0 = wave_u * 8 * p.kv_pad * 2, sv1 = (wave_u + 4) * 8 * p.kv_pad * 2;
  const int lb = w64::lds_base(smem);
  const int nt = (p.kv_len + 63) >> 6;
  const int lim = p.kv_len - (nt - 1) * 64 - 16 * hi;

  // rows 64..95 of every stage's Vt image: constant — row 72 (read by the hi = 0 half) and 76 (hi = 1) are ones, so accumulator 4 of
  // the third PV block is sum_k P[k][q]; the rest is MFMA padding
  for (int u = tid; u < W64_STAGES * 256; u += 256) {
    const int row = 64 + ((u & 255) >> 3);
    const unsigned w1 = (row == 72 || row == 76) ? 0x3f803f80u : 0u;
    *reinterpret_cast<uint4*>(smem + (u >> 8) * KV_STAGE + K_TILE_BYTES + row * VROW + (u & 7) * 16) = make_uint4(w1, w1, w1, w1);
  }

  // ---- fragment read offsets inside a stage
  const int krow = w64::frag_krow(l31);
  const int k_roff = krow * KROW + ((hi ^ ((krow >> 1) & 7)) << 4);   // logical chunk 2 cc + hi at physical chunk ^ ((row >> 1) & 7)
  const int kfa0 = k_roff, kfa1 = k_roff ^ (1 << 5), kfa2 = k_roff ^ (2 << 5), kfa3 = k_roff ^ (3 << 5);
  const w64::VtFrag vf = w64::vt_frag<K_TILE_BYTES>(l31, hi);
  const int vfa0 = vf.vfa0, vfa1 = vf.vfa1, vfa2 = vf.vfa2, vfa3 = vf.vfa3;

  // ---- Q fragments of the two 32-row blocks (B operand: lane holds Q[row][16c + 8hi .. +8], c = 0..3): LayerNorm + RoPE as
  // flash_attn_d64_kernel's prologue
  uint4 qw[2][4];
  float nmv[2] = {0.f, 0.f};   // VAR 5: -(row bound) of this lane's query row in block A / B
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    int qs = q0 + 32 * blk + l31;
    qs = qs < p.q_len ? qs : p.q_len - 1;
    const bf16_t* qrow = p.q + ((int64_t)b * p.q_len + qs) * p.q_stride + h * HD;
    float x[4][8];
#pragma unroll
    for (int c = 0; c < 4; ++c) unpack8(*reinterpret_cast<const uint4*>(qrow + 16 * c + 8 * hi), x[c]);
    if (p.ln_w != nullptr) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) s += x[c][e];
      s += __shfl_xor(s, 32, 64);
      const float mean = s * (1.0f / 64.0f);
      float v = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) v += (x[c][e] - mean) * (x[c][e] - mean);
      v += __shfl_xor(v, 32, 64);
      const float rstd = rsqrtf(v * (1.0f / 64.0f) + p.eps);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float w[8], bb[8];
        unpack8(*reinterpret_cast<const uint4*>(p.ln_w + 16 * c + 8 * hi), w);
        if (p.ln_b != nullptr) {
          unpack8(*reinterpret_cast<const uint4*>(p.ln_b + 16 * c + 8 * hi), bb);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) bb[e] = 0.f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) x[c][e] = bf2f(f2bf((x[c][e] - mean) * rstd * w[e] + bb[e]));
      }
    }
    const int rp = qs - p.rope_start;
    if (p.rope_cos != nullptr && rp >= 0 && rp < p.rope_len) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float4* cs = reinterpret_cast<const float4*>(p.rope_cos + (int64_t)rp * HD + 16 * c + 8 * hi);
        const float4* sn = reinterpret_cast<const float4*>(p.rope_sin + (int64_t)rp * HD + 16 * c + 8 * hi);
        const float4 c0 = cs[0], c1 = cs[1], s0 = sn[0], s1 = sn[1];
        const float cv[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
        const float sv[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
          const float a = x[c][e], bb = x[c][e + 1];
          x[c][e] = a * cv[e] - bb * sv[e];
          x[c][e + 1] = bb * cv[e + 1] + a * sv[e + 1];
        }
      }
    }
    if constexpr (VAR == 5) nmv[blk] = w64::neg_row_bound<4>(x, p.k_bound);
#pragma unroll
    for (int c = 0; c < 4; ++c) qw[blk][c] = pack8(x[c]);
  }
  FLASH64_W64_WRITE_Q_A(qw[0]);
  FLASH64_W64_WRITE_Q_B(qw[1]);

  // ---- the tile loop
  if constexpr (VAR == 5) {   // no running max: the row bounds ride in as the -m splat
    const float nma = nmv[0], nmb = nmv[1];
    asm volatile(FLASH64_W64_ASM_V5 : : FLASH64_W64_OPERANDS_S : FLASH64_W64_CLOBBERS);
  }
  else if constexpr (VAR == 4) asm volatile(FLASH64_W64_ASM_V4 : : FLASH64_W64_OPERANDS : FLASH64_W64_CLOBBERS);
  else asm volatile(FLASH64_W64_ASM_V1 : : FLASH64_W64_OPERANDS : FLASH64_W64_CLOBBERS);

  // ---- epilogue: O / l of the two blocks; l = row 72 (hi = 0) / 76 (hi = 1) of the Vt image: sum_k P[k][q]
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    float o[2][16], lsum;
    if (blk == 0) FLASH64_W64_READ_O_A(o, lsum);
    else FLASH64_W64_READ_O_B(o, lsum);
    const float inv = 1.0f / lsum;
    const int qs = q0 + 32 * blk + l31;
    bf16_t* orow = p.out + ((int64_t)b * p.q_len + (qs < p.q_len ? qs : p.q_len - 1)) * p.out_stride + h * HD + 8 * hi;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      uint2 w[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        w[g].x = pack2bf(o[dt][4 * g + 0] * inv, o[dt][4 * g + 1] * inv);
        w[g].y = pack2bf(o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv);
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const auto sx = __builtin_amdgcn_permlane32_swap(w[2 * k].x, w[2 * k + 1].x, false, false);
        const auto sy = __builtin_amdgcn_permlane32_swap(w[2 * k].y, w[2 * k + 1].y, false, false);
        if (qs < p.q_len) *reinterpret_cast<uint4*>(orow + dt * 32 + 16 * k) = make_uint4(sx[0], sy[0], sx[1], sy[1]);
      }
    }
  }
#endif
}

}  // namespace

// true when the w64 kernel takes the problem (launch_flash_attn_d64 falls back to flash_attn_d64_kernel otherwise)
bool flash64_w64_supports(int q_len, int kv_len) { return kv_len >= 256 && q_len >= 256; }

int launch_flash_attn_d64_w64(const bf16_t* q, int64_t q_stride, const bf16_t* ln_w, const bf16_t* ln_b, const float* rope_cos,
                              const float* rope_sin, int rope_start, int rope_len, const bf16_t* kp, const bf16_t* vt, bf16_t* out,
                              int64_t out_stride, int batch, int heads, int q_len, int kv_len, int kv_pad, float eps, int var,
                              float k_bound, hipStream_t stream) {
  Flash64W64Params p;
  p.k_bound = k_bound;
  p.q = q; p.q_stride = q_stride; p.ln_w = ln_w; p.ln_b = ln_b; p.rope_cos = rope_cos; p.rope_sin = rope_sin;
  p.rope_start = rope_start; p.rope_len = rope_len; p.kp = kp; p.vt = vt; p.out = out; p.out_stride = out_stride;
  p.heads = heads; p.q_len = q_len; p.kv_len = kv_len; p.kv_pad = kv_pad; p.eps = eps;
  p.nqb = (q_len + 255) / 256;
  const int64_t nblk = (int64_t)p.nqb * batch * heads;
  if (nblk > 0x7fffffff || (int64_t)kv_pad * HD * 2 >= 0x7fffffff) return VSYS_ERR_SHAPE;
  const size_t lds = (size_t)W64_STAGES * KV_STAGE;   // 81920
  switch (var) {   // (named in the order 1, 4, 5 they have always been instantiated in: the statements' labels count the functions)
    default: return w64::launch<flash_attn_d64_w64_kernel<1>>((unsigned)nblk, lds, stream, p);
    case 4: return w64::launch<flash_attn_d64_w64_kernel<4>>((unsigned)nblk, lds, stream, p);
    case 5: return k_bound > 0.f ? w64::launch<flash_attn_d64_w64_kernel<5>>((unsigned)nblk, lds, stream, p) : VSYS_ERR_ARG;
  }
}

}  // namespace vsys
