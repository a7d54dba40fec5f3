// Head-dim-96 attention, the plain addressing: token s of sample b is row b * len + s (vsys_attn_prep_kv96, vsys_flash_attn_d96).
// The kernel bodies, their geometry and the rounding contract are attention96.h; the image addressing is attention96_img.hip.
#include "attention96.h"

namespace vsys {
namespace {

__global__ __launch_bounds__(256) void attn_prep_kv96_kernel(const bf16_t* __restrict__ k, int64_t k_stride,
                                                             const bf16_t* __restrict__ v, int64_t v_stride,
                                                             const float* __restrict__ rope_cos, const float* __restrict__ rope_sin,
                                                             bf16_t* __restrict__ kp, bf16_t* __restrict__ vt, int heads, int kv_len,
                                                             int kv_pad) {
  attn_prep_kv96_body<false>(k, k_stride, v, v_stride, rope_cos, rope_sin, kp, vt, heads, kv_len, kv_pad, 0, 0);
}

}  // namespace

int launch_attn_prep_kv96(const bf16_t* k, int64_t k_stride, const bf16_t* v, int64_t v_stride, const float* rope_cos,
                          const float* rope_sin, bf16_t* kp, bf16_t* vt, int batch, int heads, int kv_len, int kv_pad,
                          hipStream_t stream) {
  if (batch <= 0 || heads <= 0 || kv_len <= 0) return 0;
  if (const int rc = check_prep_kv96(k, k_stride, v, v_stride, rope_cos, rope_sin, kp, vt, batch, heads, kv_len, kv_pad)) return rc;
  dim3 grid(kv_pad / 64, batch * heads);
  hipLaunchKernelGGL(attn_prep_kv96_kernel, grid, dim3(256), 0, stream, k, k_stride, v, v_stride, rope_cos, rope_sin, kp, vt, heads,
                     kv_len, kv_pad);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

int launch_flash_attn_d96(const bf16_t* q, int64_t q_stride, const float* rope_cos, const float* rope_sin, const bf16_t* kp,
                          const bf16_t* vt, const int* kv_lens, bf16_t* out, int64_t out_stride, int batch, int heads, int q_len,
                          int kv_len, int kv_pad, hipStream_t stream) {
  if (batch <= 0 || heads <= 0 || q_len <= 0) return 0;
  Flash96Params p;
  int64_t nblk;
  if (const int rc = check_flash_d96(p, nblk, q, q_stride, rope_cos, rope_sin, kp, vt, kv_lens, out, out_stride, batch, heads, q_len,
                                     kv_len, kv_pad))
    return rc;
  hipLaunchKernelGGL((flash_attn_d96_kernel<false, Flash96Params>), dim3((unsigned)nblk), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

}  // namespace vsys
