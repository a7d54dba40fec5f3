// The kernels the Open-Sora-Plan pipelines need beside the ones they share with the other families.  v1.2
// (autoencoder_kl_open_sora_plan_v120.py, pipeline_open_sora_plan.py):
//
//   vsys_upsample_trilinear2x   Spatial2xTime2x3DUpsample.forward (:349-357) up to its conv: F.interpolate(mode="trilinear") of frame 0
//                               by (1, 2, 2) and of frames 1.. by (2, 2, 2), written into the interior of the conv's padded input grid
//   vsys_cfg_ancestral_step     CFG combine + EulerAncestralDiscreteScheduler.step + the next step's scale_model_input, one launch
//   vsys_pixels_to_u8_trunc     conv_out rows -> uint8 [F][H][W][3] with the reference's own post-process (:1186-1188: bf16 tensor
//                               arithmetic, then a truncating cast)
//
// v1.1 (autoencoder_kl_open_sora_plan_v110.py, pipeline_open_sora_plan.py with PNDMScheduler):
//
//   vsys_upsample_time2x        TimeUpsample2x.forward (:1545-1554) / TimeUpsampleRes2x.forward (:1590-1596) up to its conv: frame 0 copied,
//                               frames 1.. interpolated by (2, 1, 1) among themselves, written into the interior of the conv's padded
//                               input grid; optionally alpha * the same value into a second grid (the conv's residual operand)
//   vsys_cfg_pndm_step          CFG combine + one PNDMScheduler.step (a Runge-Kutta warm-up call or the linear multistep) + the next
//                               call's model input, one launch
//
// Grid convention (VaeGrid, grid_row) as in vae_ops.hip: kernels read and write INTERIOR rows only.
#include "common.h"
#include "vsys_internal.h"

namespace vsys {
namespace {

__device__ __forceinline__ int64_t grid_row(const VaeGrid& g, int n, int t, int h, int w) {
  return (int64_t)n * g.sample_rows + ((int64_t)(t + g.tf) * (g.H + 2 * g.pad) + h + g.pad) * (g.W + 2 * g.pad) + w + g.pad;
}

// One axis of F.interpolate(scale_factor=2, mode="(tri)linear", align_corners=False) over source indices lo .. hi: destination
// index o (counted from the start of the range) sits at source coordinate o / 2 - 1 / 4, clamped below at 0 — even o = 2k reads
// (k - 1, k) with weights (1/4, 3/4), odd o = 2k + 1 reads (k, k + 1) with (3/4, 1/4), and a tap outside the range folds onto the
// edge sample (the weights still add up to 1).
struct Taps {
  int i0, i1;
  float w0, w1;
};
__device__ __forceinline__ Taps taps2x(int o, int lo, int hi) {
  const int k = o >> 1;
  Taps t;
  if (o & 1) { t.i0 = lo + k; t.i1 = lo + k + 1; t.w0 = 0.75f; t.w1 = 0.25f; }
  else { t.i0 = lo + k - 1; t.i1 = lo + k; t.w0 = 0.25f; t.w1 = 0.75f; }
  t.i0 = t.i0 < lo ? lo : t.i0;
  t.i1 = t.i1 > hi ? hi : t.i1;
  return t;
}

// Block = one destination image row (n, t, h): its frame and row taps are block-uniform.  Thread = (pixel lane, 8-channel chunk),
// both fixed for the whole kernel (no division in the loops); an item is eight 16-byte loads (the 2 x 2 x 2 source neighbourhood),
// 64 fp32 multiply-adds and one 16-byte store.  The eight taps are accumulated in fp32 and rounded to bf16 once.
__global__ __launch_bounds__(256) void upsample_trilinear2x_kernel(const bf16_t* __restrict__ x, VaeGrid gs, bf16_t* __restrict__ y,
                                                                   VaeGrid gd, int C, int N) {
  const int nch = C >> 3;
  const int lanes = 256 / nch;
  const int ch = threadIdx.x % nch, pl = threadIdx.x / nch;
  if (pl >= lanes) return;
  const int64_t nrows = (int64_t)N * gd.T * gd.H;
  for (int64_t br = blockIdx.x; br < nrows; br += gridDim.x) {
    const int h = (int)(br % gd.H);
    const int64_t r1 = br / gd.H;
    const int t = (int)(r1 % gd.T), n = (int)(r1 / gd.T);
    Taps tt;
    if (t == 0) { tt.i0 = tt.i1 = 0; tt.w0 = 1.f; tt.w1 = 0.f; }   // frame 0 is upsampled on its own, (1, 2, 2)
    else tt = taps2x(t - 1, 1, gs.T - 1);                          // frames 1.. among themselves
    const Taps th = taps2x(h, 0, gs.H - 1);
    const bf16_t* s00 = x + grid_row(gs, n, tt.i0, th.i0, 0) * C + ch * 8;
    const bf16_t* s01 = x + grid_row(gs, n, tt.i0, th.i1, 0) * C + ch * 8;
    const bf16_t* s10 = x + grid_row(gs, n, tt.i1, th.i0, 0) * C + ch * 8;
    const bf16_t* s11 = x + grid_row(gs, n, tt.i1, th.i1, 0) * C + ch * 8;
    const float c00 = tt.w0 * th.w0, c01 = tt.w0 * th.w1, c10 = tt.w1 * th.w0, c11 = tt.w1 * th.w1;   // exact: products of k / 4
    bf16_t* yr = y + grid_row(gd, n, t, h, 0) * C + ch * 8;
    for (int w = pl; w < gd.W; w += lanes) {
      const Taps tw = taps2x(w, 0, gs.W - 1);
      const int64_t o0 = (int64_t)tw.i0 * C, o1 = (int64_t)tw.i1 * C;
      float a[8], b[8], acc[8];
      unpack8(*reinterpret_cast<const uint4*>(s00 + o0), a);
      unpack8(*reinterpret_cast<const uint4*>(s00 + o1), b);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = c00 * (tw.w0 * a[e] + tw.w1 * b[e]);
      unpack8(*reinterpret_cast<const uint4*>(s01 + o0), a);
      unpack8(*reinterpret_cast<const uint4*>(s01 + o1), b);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += c01 * (tw.w0 * a[e] + tw.w1 * b[e]);
      unpack8(*reinterpret_cast<const uint4*>(s10 + o0), a);
      unpack8(*reinterpret_cast<const uint4*>(s10 + o1), b);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += c10 * (tw.w0 * a[e] + tw.w1 * b[e]);
      unpack8(*reinterpret_cast<const uint4*>(s11 + o0), a);
      unpack8(*reinterpret_cast<const uint4*>(s11 + o1), b);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += c11 * (tw.w0 * a[e] + tw.w1 * b[e]);
      *reinterpret_cast<uint4*>(yr + (int64_t)w * C) = pack8(acc);
    }
  }
}

// eps = uncond + g (cond - uncond) on the first Cin of Cout channels (negative prompt first: uncond = model_out[b], cond =
// model_out[b + Bz]); z' = z + dt eps + sigma_up noise; model_in[b] = model_in[b + Bz] = bf16(z' * in_scale).  The update is
// evaluated in fp64 and rounded to fp32 once (a few hundred thousand elements per step: the kernel is a launch and a memory pass,
// the arithmetic is free), so z' is the correctly rounded value of the formula on the fp32 operands.
__global__ __launch_bounds__(256) void cfg_ancestral_kernel(float* __restrict__ z, const float* __restrict__ model_out,
                                                            const float* __restrict__ noise, bf16_t* __restrict__ model_in, int Bz,
                                                            int Cin, int Cout, int64_t thw, float guidance, float dt, float sigma_up,
                                                            float in_scale) {
  const int64_t per = (int64_t)Cin * thw;
  const int64_t total = (int64_t)Bz * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / per, r = i - b * per;   // r = c * thw + position, c < Cin: the same offset inside a model_out sample
    const double unc = model_out[b * Cout * thw + r];
    const double cond = model_out[(b + Bz) * Cout * thw + r];
    double v = (double)z[i] + (double)dt * (unc + (double)guidance * (cond - unc));
    if (noise) v += (double)sigma_up * (double)noise[i];
    const float zn = (float)v;
    z[i] = zn;
    const bf16_t m = f2bf(zn * in_scale);
    model_in[i] = m;
    model_in[total + i] = m;
  }
}

// Block = one destination image row (n, t, h), thread = (pixel lane, 8-channel chunk) as upsample_trilinear2x_kernel; the frame taps
// are block-uniform.  A destination frame whose two taps are the same source frame (frame 0; both frames of a one-frame range) is that
// frame's bits.  Otherwise v = w0 a + w1 b in fp32 (exact: a bf16 value times k / 4 has ten significant bits, the sum one rounding)
// and y = bf16(v).  RES: y2 = bf16(alpha * v) from the same fp32 v, over its own grid.
template <bool RES>
__global__ __launch_bounds__(256) void upsample_time2x_kernel(const bf16_t* __restrict__ x, VaeGrid gs, bf16_t* __restrict__ y, VaeGrid gd,
                                                              bf16_t* __restrict__ y2, VaeGrid g2, float alpha, int C, int N) {
  const int nch = C >> 3;
  const int lanes = 256 / nch;
  const int ch = threadIdx.x % nch, pl = threadIdx.x / nch;
  if (pl >= lanes) return;
  const int64_t nrows = (int64_t)N * gd.T * gd.H;
  for (int64_t br = blockIdx.x; br < nrows; br += gridDim.x) {
    const int h = (int)(br % gd.H);
    const int64_t r1 = br / gd.H;
    const int t = (int)(r1 % gd.T), n = (int)(r1 / gd.T);
    Taps tt;
    if (t == 0) { tt.i0 = tt.i1 = 0; tt.w0 = 1.f; tt.w1 = 0.f; }   // frame 0 is copied
    else tt = taps2x(t - 1, 1, gs.T - 1);                          // frames 1.. among themselves
    const bool same = tt.i0 == tt.i1;
    const bf16_t* s0 = x + grid_row(gs, n, tt.i0, h, 0) * C + ch * 8;
    const bf16_t* s1 = x + grid_row(gs, n, tt.i1, h, 0) * C + ch * 8;
    bf16_t* yr = y + grid_row(gd, n, t, h, 0) * C + ch * 8;
    bf16_t* y2r = RES ? y2 + grid_row(g2, n, t, h, 0) * C + ch * 8 : nullptr;
    for (int w = pl; w < gd.W; w += lanes) {
      const int64_t o = (int64_t)w * C;
      const uint4 va = *reinterpret_cast<const uint4*>(s0 + o);
      float a[8], b[8], acc[8];
      unpack8(va, a);
      if (same) {
        *reinterpret_cast<uint4*>(yr + o) = va;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = a[e];
      } else {
        unpack8(*reinterpret_cast<const uint4*>(s1 + o), b);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = tt.w0 * a[e] + tt.w1 * b[e];
        *reinterpret_cast<uint4*>(yr + o) = pack8(acc);
      }
      if (RES) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] *= alpha;
        *reinterpret_cast<uint4*>(y2r + o) = pack8(acc);
      }
    }
  }
}

// e = uncond + g (cond - uncond) on the first Cin of Cout channels (negative prompt first), then two linear forms over S = {e, src[0..3]}:
// z_out = c_base base + sum cz[i] S[i] and aux_out = sum ca[i] S[i].  Everything is evaluated in fp64 on the fp32 operands and every
// stored value is rounded once, as cfg_ancestral_kernel does.  A source is read only where one of its weights is non-zero, and enters
// only the sums whose weight is non-zero.  Element i of every output depends on element i of the inputs alone and a thread reads all
// of them before it writes, so an output may share its buffer with an input (base == z_out: the multistep runs in place; aux_out ==
// src[k]: the Runge-Kutta accumulator) — hence no __restrict__ on them.
struct PndmArgs {
  const float* src[4];
  double g, cb, cz[5], ca[5];
};
__global__ __launch_bounds__(256) void cfg_pndm_kernel(const float* model_out, float* e_out, PndmArgs a, const float* base, float* z_out,
                                                       float* aux_out, bf16_t* __restrict__ model_in, int Bz, int Cin, int Cout,
                                                       int64_t thw) {
  const int64_t per = (int64_t)Cin * thw;
  const int64_t total = (int64_t)Bz * per;
  const int64_t b = blockIdx.y;                   // one sample per grid row: no division in the loop
  const float* mu = model_out + b * Cout * thw;
  const float* mc = model_out + (b + Bz) * Cout * thw;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < per; r += (int64_t)gridDim.x * 256) {
    const int64_t i = b * per + r;                // r = c * thw + position, c < Cin: the same offset inside a model_out sample
    const double unc = mu[r];
    const double cond = mc[r];
    const double e = unc + a.g * (cond - unc);
    double z = a.cb != 0.0 ? a.cb * (double)base[i] : 0.0;
    double aux = 0.0;
    if (a.cz[0] != 0.0) z += a.cz[0] * e;
    if (a.ca[0] != 0.0) aux += a.ca[0] * e;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (a.cz[k + 1] != 0.0 || a.ca[k + 1] != 0.0) {
        const double s = a.src[k][i];
        if (a.cz[k + 1] != 0.0) z += a.cz[k + 1] * s;
        if (a.ca[k + 1] != 0.0) aux += a.ca[k + 1] * s;
      }
    }
    const float zn = (float)z;
    if (e_out) e_out[i] = (float)e;
    if (aux_out) aux_out[i] = (float)aux;
    z_out[i] = zn;
    // one rounding of the fp64 value, like every other store — NOT bf16(zn): the compiler folds (bf16)(float)z into this conversion
    // anyway (round-to-odd to fp32, then to bf16), so it is spelled out; the two differ in about one element in 2^16
    const bf16_t m = __builtin_bit_cast(bf16_t, (__bf16)z);
    model_in[i] = m;
    model_in[total + i] = m;
  }
}

// bf16 pixel value -> the byte of OpenSoraPlanPipeline.decode_latents (:1186-1188), every tensor op of the reference rounding to bf16:
// d = clamp(bf16(bf16(x / 2) + 0.5), 0, 1), m = bf16(d * 255), byte = trunc(m) (m is a non-negative integer-or-fraction <= 255).
__device__ __forceinline__ uint32_t pixel_byte_trunc(uint32_t bits16) {
  const float x = __uint_as_float(bits16 << 16);
  const float d = bf2f(f2bf(bf2f(f2bf(x * 0.5f)) + 0.5f));
  const float m = bf2f(f2bf(fminf(fmaxf(d, 0.f), 1.f) * 255.f));
  return (uint32_t)m;
}

// Thread = 4 consecutive pixels = 12 destination bytes, as pixels_to_u8_kernel of vae_sd3.hip: three dword stores when the run's
// first byte is dword aligned, byte stores otherwise and for the last, partial group.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void pixels_to_u8_trunc_kernel(const bf16_t* __restrict__ x, VaeGrid g, int64_t ldx,
                                                                 uint8_t* __restrict__ dst, int64_t npix) {
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
        b[3 * k] = pixel_byte_trunc(v.x & 0xffffu);
        b[3 * k + 1] = pixel_byte_trunc(v.x >> 16);
        b[3 * k + 2] = pixel_byte_trunc(v.y & 0xffffu);
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

bool grid_ok(const VaeGrid& g) {
  return g.T > 0 && g.H > 0 && g.W > 0 && g.pad >= 0 && g.pad <= 1 && g.tf >= 0 &&
         g.sample_rows >= (int64_t)(g.T + g.tf) * (g.H + 2 * g.pad) * (g.W + 2 * g.pad);
}

}  // namespace

int launch_upsample_trilinear2x(const bf16_t* x, const VaeGrid& gs, bf16_t* y, const VaeGrid& gd, int N, int C, hipStream_t stream) {
  if (!x || !y) return VSYS_ERR_ARG;
  if (N < 0 || N > 65535 || !grid_ok(gs) || !grid_ok(gd) || gd.T != (gs.T == 1 ? 1 : 2 * gs.T - 1) || gd.H != 2 * gs.H ||
      gd.W != 2 * gs.W || C <= 0 || C % 8 != 0 || C > 2048)
    return VSYS_ERR_SHAPE;
  if (reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(y) % 16) return VSYS_ERR_ALIGN;
  if (N == 0) return 0;
  const int64_t nrows = (int64_t)N * gd.T * gd.H;
  hipLaunchKernelGGL(upsample_trilinear2x_kernel, dim3((unsigned)(nrows < 65536 ? nrows : 65536)), dim3(256), 0, stream, x, gs, y, gd,
                     C, N);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

int launch_cfg_ancestral_step(float* z, const float* model_out, const float* noise, bf16_t* model_in, int Bz, int Cin, int Cout,
                              int64_t thw, float guidance, float dt, float sigma_up, float in_scale, hipStream_t stream) {
  if (!z || !model_out || !model_in) return VSYS_ERR_ARG;
  if (!noise && sigma_up != 0.f) return VSYS_ERR_ARG;
  if (Bz < 0 || Cin <= 0 || Cout != 2 * Cin || thw < 0) return VSYS_ERR_SHAPE;
  const int64_t total = (int64_t)Bz * Cin * thw;
  if (total == 0) return 0;
  hipLaunchKernelGGL(cfg_ancestral_kernel, dim3(grid_for(total)), dim3(256), 0, stream, z, model_out, noise, model_in, Bz, Cin, Cout,
                     thw, guidance, dt, sigma_up, in_scale);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

int launch_upsample_time2x(const bf16_t* x, const VaeGrid& gs, bf16_t* y, const VaeGrid& gd, bf16_t* y_res, const VaeGrid* g_res,
                           float alpha, int N, int C, hipStream_t stream) {
  if (!x || !y || (y_res && !g_res)) return VSYS_ERR_ARG;
  if (N < 0 || N > 65535 || !grid_ok(gs) || !grid_ok(gd) || gd.T != (gs.T == 1 ? 1 : 2 * gs.T - 1) || gd.H != gs.H || gd.W != gs.W ||
      C <= 0 || C % 8 != 0 || C > 2048)
    return VSYS_ERR_SHAPE;
  if (y_res && (!grid_ok(*g_res) || g_res->T != gd.T || g_res->H != gd.H || g_res->W != gd.W)) return VSYS_ERR_SHAPE;
  if (reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(y) % 16 || reinterpret_cast<uintptr_t>(y_res) % 16)
    return VSYS_ERR_ALIGN;
  if (N == 0) return 0;
  const int64_t nrows = (int64_t)N * gd.T * gd.H;
  const dim3 grid((unsigned)(nrows < 65536 ? nrows : 65536));
  if (y_res)
    hipLaunchKernelGGL(upsample_time2x_kernel<true>, grid, dim3(256), 0, stream, x, gs, y, gd, y_res, *g_res, alpha, C, N);
  else
    hipLaunchKernelGGL(upsample_time2x_kernel<false>, grid, dim3(256), 0, stream, x, gs, y, gd, (bf16_t*)nullptr, gd, 0.f, C, N);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

int launch_cfg_pndm_step(const float* model_out, float* e_out, const float* const* src, const float* base, float* z_out, float* aux_out,
                         bf16_t* model_in, int Bz, int Cin, int Cout, int64_t thw, const double* coef, hipStream_t stream) {
  if (!model_out || !z_out || !model_in || !coef) return VSYS_ERR_ARG;
  PndmArgs a;
  a.g = coef[0];
  a.cb = coef[1];
  for (int k = 0; k < 5; ++k) { a.cz[k] = coef[2 + k]; a.ca[k] = aux_out ? coef[7 + k] : 0.0; }   // no aux_out: nothing to store
  for (int k = 0; k < 4; ++k) {
    a.src[k] = src[k];
    if (!src[k] && (a.cz[k + 1] != 0.0 || a.ca[k + 1] != 0.0)) return VSYS_ERR_ARG;   // a weight on a source that is not there
  }
  if (!base && a.cb != 0.0) return VSYS_ERR_ARG;
  if (Bz < 0 || Bz > 65535 || Cin <= 0 || Cout != 2 * Cin || thw < 0) return VSYS_ERR_SHAPE;
  const int64_t total = (int64_t)Bz * Cin * thw;
  if (total == 0) return 0;
  hipLaunchKernelGGL(cfg_pndm_kernel, dim3(grid_for((int64_t)Cin * thw), (unsigned)Bz), dim3(256), 0, stream, model_out, e_out, a, base, z_out, aux_out, model_in, Bz,
                     Cin, Cout, thw);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

int launch_pixels_to_u8_trunc(const bf16_t* x, const VaeGrid& g, int N, int64_t ldx, uint8_t* out, int64_t Ftot, int64_t f0,
                              hipStream_t stream) {
  if (!x || !out) return VSYS_ERR_ARG;
  if (N < 0 || !grid_ok(g) || ldx < 4 || Ftot <= 0 || f0 < 0 || f0 + (int64_t)N * g.T > Ftot) return VSYS_ERR_SHAPE;
  if (ldx % 4 || reinterpret_cast<uintptr_t>(x) % 8) return VSYS_ERR_ALIGN;
  if (N == 0) return 0;
  const int64_t plane = (int64_t)g.H * g.W;
  const int64_t npix = (int64_t)N * g.T * plane;
  uint8_t* dst = out + f0 * plane * 3;
  const unsigned grid = grid_for((npix + 3) >> 2);
  if (reinterpret_cast<uintptr_t>(dst) % 4 == 0)
    hipLaunchKernelGGL(pixels_to_u8_trunc_kernel<true>, dim3(grid), dim3(256), 0, stream, x, g, ldx, dst, npix);
  else
    hipLaunchKernelGGL(pixels_to_u8_trunc_kernel<false>, dim3(grid), dim3(256), 0, stream, x, g, ldx, dst, npix);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

}  // namespace vsys
