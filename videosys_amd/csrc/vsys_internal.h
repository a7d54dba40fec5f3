// Internal launch declarations shared by the .hip translation units and the C-ABI layer (capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <vector>

#include "../../include/videosys_amd.h"

namespace vsys {

typedef uint16_t bf16_t;

// One-time per-DEVICE work of a launcher (hipFuncSetAttribute for > 64 KiB of dynamic LDS is a per-device property of the
// function).  Use:  for (DeviceOnce once(seen); once.todo(); once.done()) { ...attribute calls... }
// The device's bit in ``seen`` is set AFTER the body ran: a second host thread that arrives while the first is still inside the body
// runs the (idempotent) body itself instead of launching before the limit is raised — the bit used to be set before the body.
// Not a stream operation, so it is legal while a stream is being captured into a hipGraph.
class DeviceOnce {
 public:
  explicit DeviceOnce(std::atomic<unsigned long long>& seen) : seen_(seen) {
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev <= 63) bit_ = 1ull << dev;
    todo_ = bit_ == 0 || (seen_.load(std::memory_order_acquire) & bit_) == 0;
  }
  bool todo() const { return todo_; }
  void done() {
    if (bit_ != 0) seen_.fetch_or(bit_, std::memory_order_release);
    todo_ = false;
  }

 private:
  std::atomic<unsigned long long>& seen_;
  unsigned long long bit_ = 0;
  bool todo_ = false;
};
// multiprocessor count of the current device (cached per device)
inline int cu_count_this_device() {
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return 256;
  int n = cache[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    hipDeviceProp_t prop;
    n = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    cache[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

enum { EPI_BIAS = VSYS_EPI_BIAS, EPI_BIAS_GELU = VSYS_EPI_BIAS_GELU, EPI_GATE_RES = VSYS_EPI_GATE_RES,
       // AdaLN folded into the GEMM (vsys_gemm_bf16_ln): W is the pre-scaled weight, the epilogue applies the row statistics
       EPI_LN_BIAS = 3, EPI_LN_GELU = 4,
       // EPI_GATE_RES that also emits the LayerNorm partials of the rows it stores (vsys_gemm_bf16_stats); no aux
       EPI_GATE_RES_STATS = 5,
       // EPI_LN_BIAS of the spatial qkv site in the K/V column order (vsys_gemm_bf16_ln_qkv_kv, gemm2_bf16.hip): Q windows are stored
       // as rows, K windows leave as Kp (RMS norm + softmax scale), V columns as Vt — the attn_prep_kv pass without its launch
       EPI_LN_QKV_KV = 6,
       EPI_F32_SLICES = 100 /* internal (gemm2_bf16.hip): fp32 K-slice partials, see launch_gemm2_slices */ };
constexpr int LN_BLOCK = 96;   // columns per LayerNorm partial (= the column width of a GEMM wave tile)
enum { ACT_NONE = VSYS_ACT_NONE, ACT_SILU = VSYS_ACT_SILU, ACT_GELU_TANH = VSYS_ACT_GELU_TANH };

struct GemmParams {
  // (every member has a default: `GemmParams p;` is fully defined, an entry point sets only what it uses)
  const bf16_t* A = nullptr; int64_t lda = 0;   // activations [M, K]
  const bf16_t* W = nullptr; int64_t ldw = 0;   // nn.Linear weight [N, K]
  const bf16_t* bias = nullptr;                 // [N] or null
  bf16_t* out = nullptr; int64_t ldo = 0;       // [M, N]
  int M = 0, N = 0, K = 0;
  const bf16_t* gate = nullptr; int64_t gate_stride = 0;  // per-sample gate row [N] at gate + sample*gate_stride, or null (gate = 1)
  const bf16_t* res = nullptr; int64_t ldr = 0;           // residual [M, N] or null
  bf16_t* aux = nullptr; int64_t ldaux = 0;               // optional copy of gate*(acc+bias) (PAB cache slab) or null
  int rows_per_sample = 0;
  // CogVideoX joint [text | video] rows: rows whose position inside the sample is < seg_split take their gate vector
  // gate_alt elements further on (enc_gate vs gate of CogVideoXLayerNormZero); 0 = one gate per sample
  int seg_split = 0; int64_t gate_alt = 0;
  // EPI_F32_SLICES only (launch_gemm2_slices): K slice length, fp32 output [slices][N][M] (element (m, n) of slice s at
  // out32[s * slab + n * ldo32 + m]: "A" is the weight here, so this is activation-row-major)
  int ks = 0; float* out32 = nullptr; int64_t slab = 0, ldo32 = 0;
  // AdaLN fold.  Row statistics travel as per-96-column partials (mean_b, M2_b) at stats[b * ld + row], b = column / 96:
  //   EPI_GATE_RES_STATS writes them for x_new = res + gate (acc + bias) (what it stores to out);
  //   EPI_LN_BIAS / EPI_LN_GELU combine the ln_nb partials of a row into (mu, rstd) and compute
  //   out = rstd (acc - mu cs[n]) + cv[n]  with W = bf16(W0 (1 + scale)), cs[n] = sum_k W[n][k], cv[n] = shift . W0[n] + bias[n].
  const float* cs = nullptr; const float* cv = nullptr;
  const float2* ln_stats = nullptr; int64_t ln_ld = 0; int ln_nb = 0; float ln_eps = 0.f;
  float2* stats_out = nullptr; int64_t stats_ld = 0;
  // EPI_GATE_RES only: up to two more rows-of-x operands (leading dimension ldr) added AFTER the residual, each with its own bf16
  // rounding — out = bf16(bf16(bf16(res + u) + add1) + add2): the `x += slab` passes of PAB broadcasts that follow this GEMM in
  // program order, folded into its store phase.  With stats_out set the same epilogue also emits the LayerNorm partials of what it
  // stored (same bits as EPI_GATE_RES_STATS / ln_row_stats give for those rows).
  const bf16_t* add1 = nullptr; const bf16_t* add2 = nullptr;
  // tile raster (common.h gemm_raster), filled in by launch_gemm: column-group width / panel-chunk height; 6 / 0 = the default
  int raster_gw = 6, raster_ph = 0;
  // two-way split K of the 128-row geometry (gemm_bf16.hip KS): fp32 partial sums [tile][wave][24][64 lanes] float4 and one flag per
  // (tile, wave), both owned by the library (one workspace per stream); filled in by launch_gemm
  float* sk_ws = nullptr; int* sk_flags = nullptr;
  // EPI_LN_QKV_KV only.  N = 216 kv_heads output columns in 96-column windows (qkv_kv_column below): out / ldo take the Q windows;
  // row m is key m % kv_S of sample m / kv_S in kp [M / kv_S][kv_heads][kv_S][72] and vt [M / kv_S][kv_heads][96][kv_S] (the
  // attn_prep_kv layouts at kv_len = kv_pad = kv_S; vt rows 72-95 are the caller's constants).  kv_S % 64 == 0, M % kv_S == 0.
  bf16_t* kp = nullptr; bf16_t* vt = nullptr; const bf16_t* k_norm_w = nullptr;
  int kv_S = 0, kv_heads = 0; float k_eps = 0.f, kscale = 0.f;
};

// Column order of the spatial qkv site under EPI_LN_QKV_KV: where output feature n (0 .. 216 heads - 1: q | k | v as the checkpoint
// has them, a head = 72 features) sits among the GEMM's columns.  Windows of 96 columns = one wave's column window: 3 heads / 4
// windows of Q in place, then one window per head h = its 72 K features + V features 24 h .. 24 h + 23, then the remaining V features
// 96 to a window.  adaln_prescale_kernel writes W', cs, cv through it; the epilogue reads window kinds back from the column offset.
__host__ __device__ inline int qkv_kv_column(int n, int heads) {
  const int C = 72 * heads, nq = C / 96;
  if (n < C) return n;
  if (n < 2 * C) return (nq + (n - C) / 72) * 96 + (n - C) % 72;
  const int f = n - 2 * C;
  return f < 24 * heads ? (nq + f / 24) * 96 + 72 + f % 24 : (nq + heads) * 96 + (f - 24 * heads);
}

// implicit-GEMM convolution / 128-column GEMM (conv_bf16.hip).  A points at the row that tap (0,0,0) reads for output row 0.
struct ConvParams {
  const bf16_t* A = nullptr; int64_t lda = 0;   // activation rows [*, cin]
  const bf16_t* W = nullptr; int64_t ldw = 0;   // [N, taps*cin], k = tap*cin + channel
  const bf16_t* bias = nullptr;                 // [N] or null
  const bf16_t* res = nullptr; int64_t ldr = 0; // residual rows [M, N] added after rounding, or null
  bf16_t* out = nullptr; float* out32 = nullptr; int64_t ldo = 0;  // exactly one of out / out32
  int M = 0, N = 0, K = 0;
  int cin = 0, taps = 0, cshift = 0, taps_hw = 0, kw = 0, row_pitch = 0, plane_pitch = 0, max_tap_rows = 0;
  int batch = 0; int64_t batch_a = 0, batch_w = 0, batch_o = 0;  // gridDim.y operand strides in elements
  float out_scale = 0.f;                        // fp32 output only
};
int launch_conv(const ConvParams& p, hipStream_t stream);

// activation grid of the VAE kernels (vae_ops.hip): row(n,t,h,w) = n*sample_rows + ((t+tf)*(H+2pad) + h+pad)*(W+2pad) + w+pad
struct VaeGrid {
  int T, H, W, pad, tf;
  int64_t sample_rows;
};
int launch_gn_stats(const bf16_t* x, const VaeGrid& g, int N, int C, int groups, float eps, float* partial, int nblk, float* stats,
                    hipStream_t stream);
int launch_gn_apply(const bf16_t* x, const VaeGrid& gs, bf16_t* y, const VaeGrid& gd, int N, int C, int groups, const float* stats,
                    const bf16_t* gamma, const bf16_t* beta, int act, hipStream_t stream);
int launch_regrid(const bf16_t* x, const VaeGrid& gs, bf16_t* y, const VaeGrid& gd, int N, int C, int up, int tmode, hipStream_t stream);
int launch_subsample(const bf16_t* x, const VaeGrid& gs, bf16_t* y, const VaeGrid& gd, int N, int C, int st, int ss, int t0, int s0,
                     hipStream_t stream);
int launch_spatial_norm_apply(const bf16_t* x, const VaeGrid& gs, bf16_t* y, const VaeGrid& gd, int N, int C, int groups,
                              const float* stats, const bf16_t* gamma, const bf16_t* beta, const bf16_t* yb, int zT, int zH, int zW,
                              hipStream_t stream);
int launch_blend_edge(const bf16_t* a, bf16_t* b, int64_t outer, int Ha, int Wa, int Hb, int Wb, int ext, int axis, hipStream_t stream);
int launch_d2s_time(const bf16_t* x, const VaeGrid& gs, bf16_t* y, const VaeGrid& gd, int N, int Cout, hipStream_t stream);
int launch_vae_first_im2col(const bf16_t* z, int F, int H, int W, int kt, int kcols, const float* scale, const float* shift,
                            const float* pq_w, const float* pq_b, bf16_t* out, hipStream_t stream);
int launch_extract_planar(const bf16_t* x, const VaeGrid& g, int N, int ldx, int nc, int tskip, bf16_t* out, int64_t Ftot, int f0,
                          hipStream_t stream);
int launch_softmax_rows(const float* s, bf16_t* p, int64_t rows, int n, int ld, hipStream_t stream);

// SD3 VAE ends of the Vchitect-2.0 decode (vae_sd3.hip)
int launch_vae_first_im2col_nc(const float* z, int F, int Cz, int H, int W, int kcols, float scaling, float shift, bf16_t* out,
                               hipStream_t stream);
int launch_pixels_to_u8(const bf16_t* x, const VaeGrid& g, int N, int64_t ldx, uint8_t* out, int64_t Ftot, int64_t f0,
                        hipStream_t stream);
// Open-Sora-Plan v1.2 CausalVAE decode and sampler (vae_osp.hip)
int launch_upsample_trilinear2x(const bf16_t* x, const VaeGrid& gs, bf16_t* y, const VaeGrid& gd, int N, int C, hipStream_t stream);
int launch_cfg_ancestral_step(float* z, const float* model_out, const float* noise, bf16_t* model_in, int Bz, int Cin, int Cout,
                              int64_t thw, float guidance, float dt, float sigma_up, float in_scale, hipStream_t stream);
int launch_pixels_to_u8_trunc(const bf16_t* x, const VaeGrid& g, int N, int64_t ldx, uint8_t* out, int64_t Ftot, int64_t f0,
                              hipStream_t stream);
// Open-Sora-Plan v1.1 CausalVAE decode and sampler (vae_osp.hip); g_res belongs to y_res (both null: no second destination),
// src: four pointers, coef: {guidance, c_base, cz[5], ca[5]} on the host
int launch_upsample_time2x(const bf16_t* x, const VaeGrid& gs, bf16_t* y, const VaeGrid& gd, bf16_t* y_res, const VaeGrid* g_res,
                           float alpha, int N, int C, hipStream_t stream);
int launch_cfg_pndm_step(const float* model_out, float* e_out, const float* const* src, const float* base, float* z_out, float* aux_out,
                         bf16_t* model_in, int Bz, int Cin, int Cout, int64_t thw, const double* coef, hipStream_t stream);

// T5 encoder pieces (t5_ops.hip)
int launch_gather_rows(const bf16_t* table, const int64_t* ids, bf16_t* out, int64_t n, int C, int64_t vocab, hipStream_t stream);
int launch_rms_norm_rows(const bf16_t* x, const bf16_t* w, bf16_t* y, int64_t rows, int C, float eps, hipStream_t stream);
int launch_geglu(const bf16_t* h, bf16_t* out, int64_t rows, int F, hipStream_t stream);
int launch_t5_attention(const bf16_t* qkv, int64_t row_stride, int inner, const float* relbias, const int* klen, bf16_t* out,
                        int64_t out_stride, int B, int L, int heads, hipStream_t stream);
int launch_splitk_reduce_t(const float* part, int S, int64_t slab, int ldp, const bf16_t* res, int64_t ldr, bf16_t* out, int64_t ldo,
                           int M, int N, hipStream_t stream);
int launch_splitk_reduce(const float* part, int S, int64_t slab, int64_t ldp, const bf16_t* res, int64_t ldr, bf16_t* out, int64_t ldo,
                         int M, int N, hipStream_t stream);
int launch_t5_attention_mfma(const bf16_t* qkv, int64_t row_stride, int inner, const float* bias, int bias_ld, int bias_center,
                             int kv_len, bf16_t* kp, bf16_t* vt, bf16_t* out, int64_t out_stride, int L, int heads,
                             hipStream_t stream);

// CLIP text encoder pieces (clip_ops.hip)
int launch_clip_attention_d64(const bf16_t* qkv, int64_t row_stride, int inner, bf16_t* out, int64_t out_stride, int B, int L,
                              hipStream_t stream);
int launch_splitk_reduce_bias_act(const float* part, int S, int64_t slab, int64_t ldp, const bf16_t* res, int64_t ldr, bf16_t* out,
                                  int64_t ldo, int M, int N, const bf16_t* bias, int act, hipStream_t stream);

int launch_gemm(const GemmParams& p, int epi, hipStream_t stream);
int launch_gemm2(const GemmParams& p, int epi, int wide, hipStream_t stream);
int launch_gemm2_qkv_kv(const GemmParams& p, hipStream_t stream);   // EPI_LN_QKV_KV (gemm2_bf16.hip); raster fields as given
int launch_gemm_qkv_kv(const GemmParams& p, hipStream_t stream);    // ... with the library's tile raster (gemm_bf16.hip)
bool gemm_ln_qkv_kv_dispatched(int64_t M, int64_t N, int64_t K);    // launch_gemm would run EPI_LN_BIAS at this shape on that kernel
int launch_gemm2_slices(const GemmParams& p, int slices, hipStream_t stream);
int launch_gemm3(const GemmParams& p, int epi, hipStream_t stream);
// ping-pong wave groups (gemm4_bf16.hip); persistent = 1: one workgroup per CU walks the tiles, 2: + stream-K tail
int launch_gemm4(const GemmParams& p, int epi, int persistent, hipStream_t stream);
bool gemm4_supports(const GemmParams& p, int epi);
bool sk_plan(int ntiles, int nt, int grid, std::vector<int4>& segs, int& nseg_max);  // stream-K segment lists (host)
int launch_gemm4_lab(const GemmParams& p, int abl, int persistent, hipStream_t stream);
int launch_gemm2_stamp(const GemmParams& p, hipStream_t stream);  // lab: per-stage cycle stamps into p.aux (int64)
int set_gemm_variant(int v);   // VSYS_ERR_ARG for ids this build does not contain
int set_flash_variant(int v);
int get_flash_variant();
void set_flash_debug_buffer(void* p);
void* get_lab_debug_buffer();
int launch_linear_small(const bf16_t* x, int64_t ldx, const bf16_t* w, int64_t ldw, const bf16_t* bias, bf16_t* out,
                        int64_t ldo, int M, int N, int K, int act_in, int act_out, hipStream_t stream);
int launch_adaln_modulate(const bf16_t* x, const bf16_t* shift, const bf16_t* scale, bf16_t* y, int64_t rows, int C,
                          int64_t rows_per_sample, int64_t mod_stride, float eps, hipStream_t stream);
// AdaLN fold (adaln_fold.hip): pre-scaled weights + column sums of every site of a step; row statistics of a tensor
int launch_adaln_prescale(const int64_t* sites, int nsites, int64_t nblocks, const bf16_t* mod, hipStream_t stream);
int launch_ln_row_stats(const bf16_t* x, int64_t rows, int C, float2* stats, int64_t ld, hipStream_t stream);
int launch_mod_table(const bf16_t* table, const bf16_t* t_mlp, bf16_t* out, int nblk, int B, int C6, hipStream_t stream);
int launch_timestep_embedding(const float* t, bf16_t* out, int B, int dim, hipStream_t stream);
int launch_patch_embed(const float* x, int Bz, const bf16_t* w, const bf16_t* bias, const bf16_t* pos, bf16_t* out, int B,
                       int Cin, int T, int H, int W, int ph, int pw, int C, int s0, int Sl, hipStream_t stream);  // Sl < 0: whole frame
int launch_unpatchify_tokens(const float* tok, float* out, int P, int B, int T, int Sl, int Hp, int Wp, int H, int W, int ph,
                             int pw, int Cout, hipStream_t stream);
int launch_final_layer(const bf16_t* x, const bf16_t* table, const bf16_t* tvec, const bf16_t* w, const bf16_t* bias,
                       float* out, int B, int T, int Hp, int Wp, int H, int W, int ph, int pw, int Cout, int C, float eps,
                       int Sl, float* tokens, hipStream_t stream);   // Sl < 0, tokens = null: whole frames -> pixels
int launch_cfg_euler(float* z, const float* model_out, int Bz, int Cin, int Cout, int64_t thw, float guidance, float dt,
                     hipStream_t stream);
int launch_cfg_axpby(float* z, const float* model_out, int Bz, int Cin, int Cout, int64_t thw, float guidance, float c_z,
                     float c_eps, int cond_first, hipStream_t stream);
int launch_add_bcast_rows(bf16_t* x, const bf16_t* e, int64_t rows, int C, int64_t group, int64_t period, hipStream_t stream);
int launch_add_rows(bf16_t* x, const bf16_t* y, int64_t n, hipStream_t stream);
int launch_copy_4d(const bf16_t* src, bf16_t* dst, int n0, int n1, int n2, int C, int64_t ss0, int64_t ss1, int64_t ss2,
                   int64_t ds0, int64_t ds1, int64_t ds2, int n1_valid, int n2_valid, hipStream_t stream);
constexpr int VSYS_COPY_BATCH_MAX = 16;
struct CopyDesc {  // one copy_4d problem relative to a common (src, dst) pair; offsets and strides in elements
  int64_t src_off, dst_off;
  int n0, n1, n2, C;
  int64_t ss0, ss1, ss2, ds0, ds1, ds2;
  int n1_valid, n2_valid;
};
int launch_copy_4d_batch(const bf16_t* src, bf16_t* dst, const CopyDesc* ops, int nops, hipStream_t stream);
// one-kernel peer-to-peer DSP exchange (p2p.hip): problem i copies into dsts[i] (+ ops[i].dst_off) and signals peer_flags[i]
int launch_p2p_exchange(const bf16_t* src, const CopyDesc* ops, bf16_t* const* dsts, unsigned* const* peer_flags, const int* remote, int nops,
                        const unsigned* my_flags, int n_flags, int self_index, unsigned* state, long long timeout_ticks,
                        hipStream_t stream);
int launch_attn_prep_kv(const bf16_t* k, int64_t k_stride, const bf16_t* v, int64_t v_stride, const bf16_t* k_norm_w,
                        bf16_t* kp, bf16_t* vt, int batch, int heads, int kv_len, int kv_pad, float eps,
                        hipStream_t stream);
int launch_flash_attn_d72(const bf16_t* q, int64_t q_stride, const bf16_t* q_norm_w, const bf16_t* kp, const bf16_t* vt,
                          bf16_t* out, int64_t out_stride, int batch, int heads, int q_len, int kv_len, int kv_pad,
                          float eps, float k_bound, hipStream_t stream,    // k_bound: see FlashW64Params::k_bound (0 = none)
                          bool keys_exact = false);   // the caller's promise of vsys_flash_attn_d72_exact (attention.hip, EXACT)
// per-sample key counts in one launch (packed text, vsys_attn_prep_kv_varlen / vsys_flash_attn_d72_varlen): the device arrays are what
// the kernels read, the host copies of the same numbers are what the launchers validate (and fall back) with
int launch_attn_prep_kv_varlen(const bf16_t* k, int64_t k_stride, const bf16_t* v, int64_t v_stride, const bf16_t* k_norm_w,
                               const int* cu_seqlens, const int* cu_seqlens_host, bf16_t* kp, bf16_t* vt, int batch, int heads,
                               int kv_pad, float eps, hipStream_t stream);
int launch_flash_attn_d72_varlen(const bf16_t* q, int64_t q_stride, const bf16_t* q_norm_w, const bf16_t* kp, const bf16_t* vt,
                                 const int* kv_lens, const int* kv_lens_host, bf16_t* out, int64_t out_stride, int batch, int heads,
                                 int q_len, int kv_pad, float eps, hipStream_t stream);
// 64 query rows per wave, one wave per SIMD, hand-allocated tile loop (attention_w64.hip); same contract as launch_flash_attn_d72
bool flash_w64_supports(int q_len, int kv_len, int kv_pad);
int launch_flash_attn_d72_w64(const bf16_t* q, int64_t q_stride, const bf16_t* q_norm_w, const bf16_t* kp, const bf16_t* vt, bf16_t* out,
                              int64_t out_stride, int batch, int heads, int q_len, int kv_len, int kv_pad, float eps, int var,
                              float k_bound, hipStream_t stream);   // var: LDS-DMA placement variant 0 / 1 / 3, 5 = no running max (k_bound)
bool flash64_w64_supports(int q_len, int kv_len);
int launch_flash_attn_d64_w64(const bf16_t* q, int64_t q_stride, const bf16_t* ln_w, const bf16_t* ln_b, const float* rope_cos,
                              const float* rope_sin, int rope_start, int rope_len, const bf16_t* kp, const bf16_t* vt, bf16_t* out,
                              int64_t out_stride, int batch, int heads, int q_len, int kv_len, int kv_pad, float eps, int var,
                              float k_bound, hipStream_t stream);
bool flash_w64p_supports(int q_len, int kv_len, int kv_pad, int64_t q_stride);   // persistent form of the w64 kernel
int launch_flash_attn_d72_w64p(const bf16_t* q, int64_t q_stride, const bf16_t* q_norm_w, const bf16_t* kp, const bf16_t* vt, bf16_t* out,
                               int64_t out_stride, int batch, int heads, int q_len, int kv_len, int kv_pad, float eps, bool stamp,
                               float k_bound, hipStream_t stream);   // stamp: lab builds only (cycle accounting into the lab debug buffer)
int launch_attn_prep_kv64(const bf16_t* k, int64_t k_stride, const bf16_t* v, int64_t v_stride, const bf16_t* ln_w,
                          const bf16_t* ln_b, const float* rope_cos, const float* rope_sin, int rope_start, int rope_len,
                          bf16_t* kp, bf16_t* vt, int batch, int heads, int kv_len, int kv_pad, float eps, hipStream_t stream);
int launch_flash_attn_d64(const bf16_t* q, int64_t q_stride, const bf16_t* ln_w, const bf16_t* ln_b, const float* rope_cos,
                          const float* rope_sin, int rope_start, int rope_len, const bf16_t* kp, const bf16_t* vt, bf16_t* out,
                          int64_t out_stride, int batch, int heads, int q_len, int kv_len, int kv_pad, float eps, float k_bound,
                          hipStream_t stream);
// Open-Sora-Plan v1.1: head dim 72 with interleaved-pair RoPE tables [len][36] per token (attention.hip)
int launch_attn_prep_kv_rope(const bf16_t* k, int64_t k_stride, const bf16_t* v, int64_t v_stride, const float* rope_cos,
                             const float* rope_sin, bf16_t* kp, bf16_t* vt, int batch, int heads, int kv_len, int kv_pad,
                             hipStream_t stream);
int launch_flash_attn_d72_rope(const bf16_t* q, int64_t q_stride, const float* rope_cos, const float* rope_sin, const bf16_t* kp,
                               const bf16_t* vt, bf16_t* out, int64_t out_stride, int batch, int heads, int q_len, int kv_len,
                               int kv_pad, hipStream_t stream);
// Open-Sora-Plan v1.2: head dim 96 with RoPE3D tables per token (attention96.hip)
int launch_attn_prep_kv96(const bf16_t* k, int64_t k_stride, const bf16_t* v, int64_t v_stride, const float* rope_cos,
                          const float* rope_sin, bf16_t* kp, bf16_t* vt, int batch, int heads, int kv_len, int kv_pad,
                          hipStream_t stream);
int launch_flash_attn_d96(const bf16_t* q, int64_t q_stride, const float* rope_cos, const float* rope_sin, const bf16_t* kp,
                          const bf16_t* vt, const int* kv_lens, bf16_t* out, int64_t out_stride, int batch, int heads, int q_len,
                          int kv_len, int kv_pad, hipStream_t stream);
int launch_attn_prep_kv96_img(const bf16_t* k, int64_t k_stride, const bf16_t* v, int64_t v_stride, const float* rope_cos,
                              const float* rope_sin, bf16_t* kp, bf16_t* vt, int batch, int heads, int kv_len, int kv_pad, int seg_len,
                              int64_t slab_rows, hipStream_t stream);
int launch_flash_attn_d96_img(const bf16_t* q, int64_t q_stride, const float* rope_cos, const float* rope_sin, const bf16_t* kp,
                              const bf16_t* vt, const int* kv_lens, bf16_t* out, int64_t out_stride, int batch, int heads, int q_len,
                              int kv_len, int kv_pad, int seg_len, int64_t q_slab_rows, int64_t out_slab_rows, hipStream_t stream);
int launch_ln_modulate(const bf16_t* x, const bf16_t* ln_w, const bf16_t* ln_b, const bf16_t* shift, const bf16_t* scale,
                       bf16_t* y, int64_t rows, int C, int64_t rows_per_sample, int64_t mod_stride, int64_t seg_split,
                       int64_t mod_alt, float eps, hipStream_t stream);
int launch_gate_add_rows(bf16_t* x, const bf16_t* y, const bf16_t* gate, int64_t rows, int C, int64_t rows_per_sample,
                         int64_t gate_stride, int64_t seg_split, int64_t gate_alt, hipStream_t stream);
int launch_unpatchify_cvx(const bf16_t* x, int64_t ldx, float* out, int B, int F, int Hp, int Wp, int Cout, int p,
                          hipStream_t stream);
int launch_im2col_patch(const float* z, int Bz, bf16_t* out, int B, int F, int Cin, int H, int W, int p, hipStream_t stream);
// T <= 32 on the matrix pipe, operands loaded in fragment layout (attention_t3.hip)
int launch_attn_temporal_d72_v3(const bf16_t* qkv, int64_t row_stride, int C, const bf16_t* q_norm_w, const bf16_t* k_norm_w,
                                const float* rope_cos, const float* rope_sin, bf16_t* out, int64_t out_stride, int B, int T, int S,
                                int heads, float eps, float scale, hipStream_t stream, bool ref_rounding = false,
                                bool no_v5 = false);   // no_v5: keep the per-lane-load kernel (A/B id 22)
int launch_attn_temporal_d72(const bf16_t* qkv, int64_t row_stride, int C, const bf16_t* q_norm_w, const bf16_t* k_norm_w,
                             const float* rope_cos, const float* rope_sin, bf16_t* out, int64_t out_stride, int B, int T,
                             int S, int heads, float eps, hipStream_t stream);

// Vchitect-2.0: temporal attention at head dim 64 over separate video / text row tensors (attention_t64.hip)
int launch_attn_temporal_d64(const bf16_t* q_vid, int64_t q_vid_ld, const bf16_t* k_vid, int64_t k_vid_ld, const bf16_t* v_vid,
                             int64_t v_vid_ld, const bf16_t* q_txt, int64_t q_txt_ld, const bf16_t* k_txt, int64_t k_txt_ld,
                             const bf16_t* v_txt, int64_t v_txt_ld, const float* rope_cos, const float* rope_sin, bf16_t* out_vid,
                             int64_t out_vid_ld, bf16_t* out_txt, int64_t out_txt_ld, int B, int T, int S, int L, int heads,
                             hipStream_t stream);
// the same kernel body on the exchange image of a sequence-parallel step: frame t at slab t / Tl, frame t % Tl of the slab
int launch_attn_temporal_d64_img(const bf16_t* q_vid, int64_t q_vid_ld, const bf16_t* k_vid, int64_t k_vid_ld, const bf16_t* v_vid,
                                 int64_t v_vid_ld, const bf16_t* q_txt, int64_t q_txt_ld, const bf16_t* k_txt, int64_t k_txt_ld,
                                 const bf16_t* v_txt, int64_t v_txt_ld, const float* rope_cos, const float* rope_sin, bf16_t* out_vid,
                                 int64_t out_vid_ld, bf16_t* out_txt, int64_t out_txt_ld, int B, int T, int Tl, int64_t slab_vid,
                                 int64_t slab_txt, int S, int L, int heads, hipStream_t stream);
int launch_scale_add_rows(const bf16_t* a, int64_t lda, const bf16_t* b, int64_t ldb, bf16_t* out, int64_t ldo, int64_t rows, int C,
                          float scale, hipStream_t stream);

}  // namespace vsys
