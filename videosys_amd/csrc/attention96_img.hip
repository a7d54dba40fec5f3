// Head-dim-96 attention on a sequence-parallel exchange image (vsys_attn_prep_kv96_img, vsys_flash_attn_d96_img): the bodies of
// attention96.h with the two-level row addressing.  Token s of sample b is row (s / seg_len) * slab_rows + b * seg_len + s % seg_len
// of k / v (prep) and of q and out (flash): the receive image [P (source)][B][Nl][...] of the Ulysses all-to-all as it lies, and the
// send image of the way back.  Everything else is the base kernels', hence the same bits as theirs on the gathered rows
// (tests/test_gpu_osp_attention_img.py).  Tokens past len in the last slab and the rows between batch * seg_len and slab_rows are
// neither read nor written (tests/test_gpu_isolation_osp_img.py).
#include "attention96.h"

namespace vsys {
namespace {

__global__ __launch_bounds__(256) void attn_prep_kv96_img_kernel(const bf16_t* __restrict__ k, int64_t k_stride,
                                                                 const bf16_t* __restrict__ v, int64_t v_stride,
                                                                 const float* __restrict__ rope_cos, const float* __restrict__ rope_sin,
                                                                 bf16_t* __restrict__ kp, bf16_t* __restrict__ vt, int heads, int kv_len,
                                                                 int kv_pad, int seg_len, int64_t slab_rows) {
  attn_prep_kv96_body<true>(k, k_stride, v, v_stride, rope_cos, rope_sin, kp, vt, heads, kv_len, kv_pad, seg_len, slab_rows);
}

}  // namespace

int launch_attn_prep_kv96_img(const bf16_t* k, int64_t k_stride, const bf16_t* v, int64_t v_stride, const float* rope_cos,
                              const float* rope_sin, bf16_t* kp, bf16_t* vt, int batch, int heads, int kv_len, int kv_pad, int seg_len,
                              int64_t slab_rows, hipStream_t stream) {
  if (batch <= 0 || heads <= 0 || kv_len <= 0) return 0;
  if (!slabs_ok(batch, kv_len, seg_len, slab_rows)) return VSYS_ERR_SHAPE;
  if (const int rc = check_prep_kv96(k, k_stride, v, v_stride, rope_cos, rope_sin, kp, vt, batch, heads, kv_len, kv_pad)) return rc;
  dim3 grid(kv_pad / 64, batch * heads);
  hipLaunchKernelGGL(attn_prep_kv96_img_kernel, grid, dim3(256), 0, stream, k, k_stride, v, v_stride, rope_cos, rope_sin, kp, vt, heads,
                     kv_len, kv_pad, seg_len, slab_rows);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

int launch_flash_attn_d96_img(const bf16_t* q, int64_t q_stride, const float* rope_cos, const float* rope_sin, const bf16_t* kp,
                              const bf16_t* vt, const int* kv_lens, bf16_t* out, int64_t out_stride, int batch, int heads, int q_len,
                              int kv_len, int kv_pad, int seg_len, int64_t q_slab_rows, int64_t out_slab_rows, hipStream_t stream) {
  if (batch <= 0 || heads <= 0 || q_len <= 0) return 0;
  if (!slabs_ok(batch, q_len, seg_len, q_slab_rows) || !slabs_ok(batch, q_len, seg_len, out_slab_rows)) return VSYS_ERR_SHAPE;
  Flash96ImgParams p;
  int64_t nblk;
  if (const int rc = check_flash_d96(p, nblk, q, q_stride, rope_cos, rope_sin, kp, vt, kv_lens, out, out_stride, batch, heads, q_len,
                                     kv_len, kv_pad))
    return rc;
  p.seg_len = seg_len; p.q_slab_rows = q_slab_rows; p.out_slab_rows = out_slab_rows;
  hipLaunchKernelGGL((flash_attn_d96_kernel<true, Flash96ImgParams>), dim3((unsigned)nblk), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

}  // namespace vsys
