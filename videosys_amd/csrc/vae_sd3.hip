// The two ends of the SD3 VAE decode of the Vchitect-2.0 pipeline (pipeline_vchitect.py:980-985) that the 4-channel first layer and
// the planar last layer of vae_ops.hip cannot do; everything between them is the 2-D decoder of vae_open_sora.py, unchanged.
//
//   vsys_vae_first_im2col_nc   fp32 latents [F][Cz][H][W] (Cz <= 32, no post_quant_conv) -> `latents / scaling_factor + shift_factor`
//                              with the reference's bf16 roundings -> im2col rows of the 3 x 3 conv_in
//   vsys_pixels_to_u8          conv_out rows -> uint8 [F][H][W][3], VaeImageProcessor.postprocess(..., "pil") with its roundings
//
// Grid convention (VaeGrid, grid_row) as in vae_ops.hip: kernels read INTERIOR rows only.
#include "common.h"
#include "vsys_internal.h"

namespace vsys {
namespace {

__device__ __forceinline__ int64_t grid_row(const VaeGrid& g, int n, int t, int h, int w) {
  return (int64_t)n * g.sample_rows + ((int64_t)(t + g.tf) * (g.H + 2 * g.pad) + h + g.pad) * (g.W + 2 * g.pad) + w + g.pad;
}

// One thread = 8 consecutive columns of one output row (one 16-byte store).  Column tap * Cz + c holds the latent of channel c at
// the 3 x 3 tap (dy, dx) = (tap / 3, tap % 3) around the row's pixel; outside the image and from column 9 Cz on: zero.
// Value: bf16(bf16(bf16(z) / scaling) + shift) — the pipeline holds bf16 latents at :980 and each of its two tensor ops rounds once;
// the division is a correctly rounded fp32 division, not a multiplication by the reciprocal.
__global__ __launch_bounds__(256) void first_im2col_nc_kernel(const float* __restrict__ z, int F, int Cz, int H, int W, int kcols,
                                                              float scaling, float shift, bf16_t* __restrict__ out) {
  const int chunks = kcols >> 3;
  const int live = 9 * Cz;
  const int64_t plane = (int64_t)H * W;
  const int64_t total = (int64_t)F * plane * chunks;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int chunk = (int)(i % chunks);
    const int64_t row = i / chunks;
    int64_t pos = row;
    const int w = (int)(pos % W); pos /= W;
    const int h = (int)(pos % H);
    const int f = (int)(pos / H);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = chunk * 8 + e;
      v[e] = 0.f;
      if (col < live) {
        const int tap = col / Cz, c = col - tap * Cz;
        const int dy = tap / 3, dx = tap - dy * 3;
        const int hh = h + dy - 1, ww = w + dx - 1;
        if (hh >= 0 && hh < H && ww >= 0 && ww < W) {
          const float zb = bf2f(f2bf(z[((int64_t)f * Cz + c) * plane + (int64_t)hh * W + ww]));
          v[e] = bf2f(f2bf(__fdiv_rn(zb, scaling))) + shift;
        }
      }
    }
    *reinterpret_cast<uint4*>(out + row * kcols + chunk * 8) = pack8(v);
  }
}

// bf16 pixel value x in [-1, 1] -> the byte of VaeImageProcessor.postprocess: d = clamp(bf16(bf16(x / 2) + 0.5), 0, 1) (denormalize
// on the bf16 tensor), then round-half-even(float(d) * 255) (numpy_to_pil on the float32 copy; d has 8 significant bits, so the
// product is exact in fp32 and rintf rounds the exact value).
__device__ __forceinline__ uint32_t pixel_byte(uint32_t bits16) {
  const float x = __uint_as_float(bits16 << 16);
  const float d = bf2f(f2bf(bf2f(f2bf(x * 0.5f)) + 0.5f));
  return (uint32_t)rintf(fminf(fmaxf(d, 0.f), 1.f) * 255.f);
}

// One thread = 4 consecutive pixels of the (frame, h, w) order = 12 consecutive destination bytes.  Source: one 8-byte load per pixel
// (4 channels of its row, 3 used).  Destination: three dwords per lane, consecutive lanes 12 bytes apart, when the first byte of the
// run is dword aligned (it is whenever H * W % 4 == 0: every decoder output); byte stores otherwise and for the last, partial group.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void pixels_to_u8_kernel(const bf16_t* __restrict__ x, VaeGrid g, int64_t ldx, uint8_t* __restrict__ dst,
                                                           int64_t npix) {
  const int64_t groups = (npix + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < groups; q += (int64_t)gridDim.x * 256) {
    uint32_t b[12];
    const int64_t p0 = q * 4;
    const int cnt = (int)(npix - p0 < 4 ? npix - p0 : 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      b[3 * k] = b[3 * k + 1] = b[3 * k + 2] = 0;
      if (k < cnt) {
        int64_t pos = p0 + k;
        const int w = (int)(pos % g.W); pos /= g.W;
        const int h = (int)(pos % g.H); pos /= g.H;
        const int t = (int)(pos % g.T);
        const int n = (int)(pos / g.T);
        const uint2 v = *reinterpret_cast<const uint2*>(x + grid_row(g, n, t, h, w) * ldx);
        b[3 * k] = pixel_byte(v.x & 0xffffu);
        b[3 * k + 1] = pixel_byte(v.x >> 16);
        b[3 * k + 2] = pixel_byte(v.y & 0xffffu);
      }
    }
    uint8_t* o = dst + p0 * 3;
    if (ALIGNED && cnt == 4) {
      uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
      o32[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
      o32[1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
      o32[2] = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
    } else {
#pragma unroll
      for (int e = 0; e < 12; ++e)
        if (e < 3 * cnt) o[e] = (uint8_t)b[e];
    }
  }
}

inline unsigned grid_for(int64_t work_items) {
  int64_t b = (work_items + 255) / 256;
  const int64_t cap = 256 * 32;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

int launch_vae_first_im2col_nc(const float* z, int F, int Cz, int H, int W, int kcols, float scaling, float shift, bf16_t* out,
                               hipStream_t stream) {
  if (!z || !out) return VSYS_ERR_ARG;
  if (F < 0 || H <= 0 || W <= 0 || Cz < 1 || Cz > 32 || kcols <= 0 || kcols % 32 != 0 || kcols < 9 * Cz) return VSYS_ERR_SHAPE;
  if (!(scaling != 0.f)) return VSYS_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(z) % 4 || reinterpret_cast<uintptr_t>(out) % 16) return VSYS_ERR_ALIGN;
  if (F == 0) return 0;
  hipLaunchKernelGGL(first_im2col_nc_kernel, dim3(grid_for((int64_t)F * H * W * (kcols >> 3))), dim3(256), 0, stream, z, F, Cz, H, W,
                     kcols, scaling, shift, out);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

int launch_pixels_to_u8(const bf16_t* x, const VaeGrid& g, int N, int64_t ldx, uint8_t* out, int64_t Ftot, int64_t f0,
                        hipStream_t stream) {
  if (!x || !out) return VSYS_ERR_ARG;
  if (N < 0 || g.T <= 0 || g.H <= 0 || g.W <= 0 || g.pad < 0 || g.pad > 1 || g.tf < 0 || ldx < 4 || Ftot <= 0 || f0 < 0 ||
      f0 + (int64_t)N * g.T > Ftot)
    return VSYS_ERR_SHAPE;
  if (g.sample_rows < (int64_t)(g.T + g.tf) * (g.H + 2 * g.pad) * (g.W + 2 * g.pad)) return VSYS_ERR_SHAPE;
  if (ldx % 4 || reinterpret_cast<uintptr_t>(x) % 8) return VSYS_ERR_ALIGN;
  if (N == 0) return 0;
  const int64_t plane = (int64_t)g.H * g.W;
  const int64_t npix = (int64_t)N * g.T * plane;
  uint8_t* dst = out + f0 * plane * 3;
  const unsigned grid = grid_for((npix + 3) >> 2);
  if (reinterpret_cast<uintptr_t>(dst) % 4 == 0)
    hipLaunchKernelGGL(pixels_to_u8_kernel<true>, dim3(grid), dim3(256), 0, stream, x, g, ldx, dst, npix);
  else
    hipLaunchKernelGGL(pixels_to_u8_kernel<false>, dim3(grid), dim3(256), 0, stream, x, g, ldx, dst, npix);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

}  // namespace vsys
