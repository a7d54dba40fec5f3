// CLIP text encoder pieces that are not GEMMs — the two `CLIPTextModelWithProjection` objects of Vchitect-2.0 (transformers
// modeling_clip.py, third-party; call site pipeline_vchitect.py:368): the causal self-attention of CLIPAttention at head dim 64, and
// the finish of the weight-streaming linears (gemm2_bf16.hip launch_gemm2_slices) for layers with a bias and an activation.  Token
// and position embedding, LayerNorm and the pooled-row gather run on the kernels T5 and the transformers already have.
#include "common.h"
#include "vsys_internal.h"

namespace vsys {
namespace {

// ---- causal self-attention, head dim 64, L <= 128 --------------------------------------------------------------------------------
// Workgroup = one (head, sample), 4 waves; K [L][64] and V^T [64][L] of the head sit in LDS, staged once.  A wave owns 16 query rows
// at a time (tiles wave, wave + 4).  Both products run on v_mfma_f32_16x16x32_bf16 with the QUERY on the lane (column) index:
//   S^T[key][query]  = K[key][d] Q^T[d][query]      A = K rows from LDS, B = q rows from HBM, both 16-byte row reads;
//                      lane (l15 = lane & 15, g = lane >> 4) then holds, per 16-key block, the logits of query l15 against keys
//                      4 g + r (r = 0..3): a whole row of <= 128 logits lives in the 32 registers of the four lanes that share l15;
//   O^T[d][query]    = V^T[d][key] P^T[key][query]  B = the weights straight from those registers: k-step t covers key blocks 2t and
//                      2t + 1, element j of lane group g is key 32 t + 16 (j >> 2) + 4 g + (j & 3); A = V^T read in that same key order
//                      (two 8-byte LDS reads); the lane ends up with 4 consecutive channels of its query: one 8-byte store each.
// One softmax pass: true row max, p = exp(s - m), l = sum p (fp32), w = bf16(p / l).  Key blocks above the diagonal are not touched
// (no K read, no V read, no MFMA); inside the diagonal block masked weights are exact zeros.
constexpr int CLIP_LMAX = 128;
constexpr int CLIP_KS = 72;    // K row pitch in LDS, elements (64 + 8: rows 144 B apart)
constexpr int CLIP_VS = 136;   // V^T row pitch, elements (128 keys + 8)

__global__ __launch_bounds__(256) void clip_attention_d64_kernel(const bf16_t* __restrict__ qkv, int64_t row_stride, int inner,
                                                                 bf16_t* __restrict__ out, int64_t out_stride, int L) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[CLIP_LMAX * CLIP_KS];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[64 * CLIP_VS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int h = blockIdx.x, b = blockIdx.y;
  const int nqt = (L + 15) >> 4;   // 16-row tiles (queries and keys alike)
  const bf16_t* base = qkv + (int64_t)b * L * row_stride + h * 64;
  // stage: item = (key row, 16-byte chunk); rows L .. 16 nqt - 1 are zeros (never a row of another sample, never past B L)
  for (int i = tid; i < nqt * 16 * 8; i += 256) {
    const int r = i >> 3, c = i & 7;
    uint4 kk = make_uint4(0u, 0u, 0u, 0u), vv = make_uint4(0u, 0u, 0u, 0u);
    if (r < L) {
      kk = *reinterpret_cast<const uint4*>(base + (int64_t)r * row_stride + inner + 8 * c);
      vv = *reinterpret_cast<const uint4*>(base + (int64_t)r * row_stride + 2 * inner + 8 * c);
    }
    *reinterpret_cast<uint4*>(Ks + r * CLIP_KS + 8 * c) = kk;
    const uint32_t w[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) Vt[(8 * c + e) * CLIP_VS + r] = (bf16_t)(w[e >> 1] >> (16 * (e & 1)));
  }
  __syncthreads();
  for (int qt = wave; qt < nqt; qt += 4) {   // wave-uniform
    const int qi = qt * 16 + l15;            // this lane's query row
    uint4 q0 = make_uint4(0u, 0u, 0u, 0u), q1 = q0;
    if (qi < L) {
      const bf16_t* qr = base + (int64_t)qi * row_stride + 8 * g;
      q0 = *reinterpret_cast<const uint4*>(qr);
      q1 = *reinterpret_cast<const uint4*>(qr + 32);
    }
    const bf16x8 qf0 = __builtin_bit_cast(bf16x8, q0), qf1 = __builtin_bit_cast(bf16x8, q1);
    f32x4 s[8];
#pragma unroll
    for (int kb = 0; kb < 8; ++kb) {
      s[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (kb <= qt) {
        const bf16_t* kr = Ks + (16 * kb + l15) * CLIP_KS + 8 * g;
        const bf16x8 k0 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(kr));
        const bf16x8 k1 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(kr + 32));
        s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf0, s[kb], 0, 0, 0);
        s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf1, s[kb], 0, 0, 0);
      }
    }
    // scale, causal mask (key <= query; only the diagonal block has any masked key), row max
    const float NEG = -__builtin_inff();
    float m = NEG;
#pragma unroll
    for (int kb = 0; kb < 8; ++kb) {
      if (kb <= qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = 16 * kb + 4 * g + r <= qi ? s[kb][r] * 0.125f : NEG;
          s[kb][r] = v;
          m = fmaxf(m, v);
        }
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));   // finite: key 0 is valid for every query
    float l = 0.f;
#pragma unroll
    for (int kb = 0; kb < 8; ++kb) {
      if (kb <= qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f((s[kb][r] - m) * 1.4426950408889634f);
          s[kb][r] = p;
          l += p;
        }
      }
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    f32x4 o[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (2 * t <= qt) {
        const bool two = 2 * t + 1 <= qt;   // the step's second key block is at or below the diagonal
        uint4 pw;
        pw.x = pack2bf(s[2 * t][0] / l, s[2 * t][1] / l);
        pw.y = pack2bf(s[2 * t][2] / l, s[2 * t][3] / l);
        pw.z = two ? pack2bf(s[2 * t + 1][0] / l, s[2 * t + 1][1] / l) : 0u;
        pw.w = two ? pack2bf(s[2 * t + 1][2] / l, s[2 * t + 1][3] / l) : 0u;
        const bf16x8 pf = __builtin_bit_cast(bf16x8, pw);
#pragma unroll
        for (int db = 0; db < 4; ++db) {
          const bf16_t* vr = Vt + (16 * db + l15) * CLIP_VS + 32 * t + 4 * g;
          const uint2 lo = *reinterpret_cast<const uint2*>(vr);
          uint2 hi = make_uint2(0u, 0u);
          if (two) hi = *reinterpret_cast<const uint2*>(vr + 16);
          const bf16x8 vf = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
          o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[db], 0, 0, 0);
        }
      }
    }
    if (qi < L) {
      bf16_t* orow = out + ((int64_t)b * L + qi) * out_stride + h * 64 + 4 * g;
#pragma unroll
      for (int db = 0; db < 4; ++db)
        *reinterpret_cast<uint2*>(orow + 16 * db) = make_uint2(pack2bf(o[db][0], o[db][1]), pack2bf(o[db][2], o[db][3]));
    }
  }
}

// ---- finish of a weight-streaming linear with bias and activation ----------------------------------------------------------------
// part[s][m][n] fp32 (launch_gemm2_slices) -> out[m][n] = bf16(act(bf16(((p_0 + p_1) + ...) + bias[n])) + res[m][n]); thread = 8
// consecutive n.  The sum starts from 0.f and runs over ascending s exactly as splitk_reduce_kernel (t5_ops.hip) does, so without
// bias and activation the two kernels give the same bits.
//   ACT 1  quick_gelu: bf16(y * bf16(sigmoid(bf16(1.702 y)))) — the three roundings of `input * torch.sigmoid(1.702 * input)` on a
//          bf16 tensor (transformers activations.py QuickGELUActivation);
//   ACT 2  gelu: bf16(0.5 y (1 + erf(y / sqrt 2))) in fp32, one rounding (nn.functional.gelu on a bf16 tensor).
template <int ACT>
__device__ __forceinline__ float clip_act(float y) {
  if (ACT == 1) {
    const float a = bf2f(f2bf(1.702f * y));
    const float sg = bf2f(f2bf(1.0f / (1.0f + __expf(-a))));
    return bf2f(f2bf(y * sg));
  }
  if (ACT == 2) return bf2f(f2bf(0.5f * y * (1.0f + erff(y * 0.70710678118654752f))));
  return y;
}

template <int ACT>
__global__ __launch_bounds__(256) void splitk_reduce_bias_act_kernel(const float* __restrict__ part, int S, int64_t slab, int64_t ldp,
                                                                     const bf16_t* __restrict__ bias, const bf16_t* res, int64_t ldr,
                                                                     bf16_t* out, int64_t ldo, int M, int N) {
  const int nch = N >> 3;
  const int64_t total = (int64_t)M * nch;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t m = i / nch;
    const int n = (int)(i - m * nch) * 8;
    const float* src = part + m * ldp + n;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) {
      const float4 a = *reinterpret_cast<const float4*>(src + s * slab), b = *reinterpret_cast<const float4*>(src + s * slab + 4);
      v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w; v[4] += b.x; v[5] += b.y; v[6] += b.z; v[7] += b.w;
    }
    if (bias != nullptr) {
      float bb[8];
      unpack8(*reinterpret_cast<const uint4*>(bias + n), bb);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += bb[e];
    }
    if (ACT != 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = clip_act<ACT>(bf2f(f2bf(v[e])));
    }
    if (res != nullptr) {
      float r[8];
      unpack8(*reinterpret_cast<const uint4*>(res + m * ldr + n), r);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = bf2f(f2bf(v[e])) + r[e];
    }
    *reinterpret_cast<uint4*>(out + m * ldo + n) = pack8(v);
  }
}

}  // namespace

int launch_clip_attention_d64(const bf16_t* qkv, int64_t row_stride, int inner, bf16_t* out, int64_t out_stride, int B, int L,
                              hipStream_t stream) {
  if (B < 1 || L < 1 || L > CLIP_LMAX || inner < 64 || inner % 64 != 0 || row_stride < 3 * (int64_t)inner || out_stride < inner)
    return VSYS_ERR_SHAPE;
  const int heads = inner / 64;
  if (B > 65535) return VSYS_ERR_SHAPE;
  if ((row_stride % 8) || (out_stride % 8) || ((uintptr_t)qkv & 15) || ((uintptr_t)out & 15)) return VSYS_ERR_ALIGN;
  hipLaunchKernelGGL(clip_attention_d64_kernel, dim3(heads, B), dim3(256), 0, stream, qkv, row_stride, inner, out, out_stride, L);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

int launch_splitk_reduce_bias_act(const float* part, int S, int64_t slab, int64_t ldp, const bf16_t* res, int64_t ldr, bf16_t* out,
                                  int64_t ldo, int M, int N, const bf16_t* bias, int act, hipStream_t stream) {
  if (act < 0 || act > 2) return VSYS_ERR_ARG;
  if (M <= 0 || N <= 0) return 0;
  if (S < 1 || S > 64 || N % 8 != 0 || ldp % 4 != 0 || ldp < N || slab < (int64_t)M * ldp || (ldo % 8) || ldo < N ||
      (res && ((ldr % 8) || ldr < N)))
    return VSYS_ERR_SHAPE;
  if (((uintptr_t)part & 15) || ((uintptr_t)out & 15) || ((uintptr_t)res & 15) || ((uintptr_t)bias & 15)) return VSYS_ERR_ALIGN;
  int64_t blocks = ((int64_t)M * (N >> 3) + 255) / 256;
  const dim3 grid((unsigned)(blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks)));
  if (act == 0)
    hipLaunchKernelGGL(splitk_reduce_bias_act_kernel<0>, grid, dim3(256), 0, stream, part, S, slab, ldp, bias, res, ldr, out, ldo, M, N);
  else if (act == 1)
    hipLaunchKernelGGL(splitk_reduce_bias_act_kernel<1>, grid, dim3(256), 0, stream, part, S, slab, ldp, bias, res, ldr, out, ldo, M, N);
  else
    hipLaunchKernelGGL(splitk_reduce_bias_act_kernel<2>, grid, dim3(256), 0, stream, part, S, slab, ldp, bias, res, ldr, out, ldo, M, N);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

}  // namespace vsys
