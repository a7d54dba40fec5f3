/* videosys_amd — C ABI of the MI355X (gfx950) STDiT3 denoise-step kernels.
 *
 * The reference (NUS-HPC-AI-Lab/VideoSys @ 2024-12-20) has NO FFI: its hot path is torch ops inside
 * videosys/models/transformers/open_sora_transformer_3d.py and videosys/models/modules/.  This header is the
 * drop-in boundary for that path: every entry point below replaces the torch op sequence at the cited reference
 * lines and is what a reference-side ctypes binding calls (INTEGRATION.md shows the stub).  Plain C: device pointers
 * and sizes only, no torch types.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HBM) unless named host_*; bf16 tensors are raw uint16 bit patterns;
 *  - all tensors row-major, inner (channel) dimension contiguous; "stride"/"ld*" arguments are in ELEMENTS;
 *  - `stream` is a hipStream_t (NULL = the null stream); every call only enqueues work on it — no host sync,
 *    no allocation; the caller owns all buffers;
 *  - return 0 on success, a negative VSYS_ERR_* code otherwise (nothing is enqueued on error);
 *    vsys_strerror() names the code.  There is NO CPU fallback anywhere in the library.
 */
#ifndef VIDEOSYS_AMD_H
#define VIDEOSYS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSYS_ABI_VERSION 1

#define VSYS_ERR_SHAPE  (-1)  /* unsupported size / divisibility */
#define VSYS_ERR_ALIGN  (-2)  /* stride or pointer not 16-byte friendly */
#define VSYS_ERR_ARG    (-3)  /* bad enum / null pointer */
#define VSYS_ERR_LAUNCH (-4)  /* HIP launch error */

/* GEMM epilogues */
#define VSYS_EPI_BIAS      0  /* out = x W^T + b */
#define VSYS_EPI_BIAS_GELU 1  /* out = gelu_tanh(x W^T + b) */
#define VSYS_EPI_GATE_RES  2  /* u = gate[sample] * (x W^T + b); aux = u (optional); out = res + u */

#define VSYS_ACT_NONE      0
#define VSYS_ACT_SILU      1
#define VSYS_ACT_GELU_TANH 2

/* Library identity and error text — no reference counterpart (the reference is pure Python and has no FFI). */
int vsys_abi_version(void);
const char* vsys_strerror(int code);
/* number of HIP devices visible to the library (fails loudly instead of falling back when 0); no reference counterpart */
int vsys_device_count(void);

/* Kernel selection for A/B measurement and for the schedule-equivalence tests — NOT part of the per-call data path: the
 * selection is one process-wide atomic word read once per launch (safe to set from any thread, but it applies to every thread's
 * launches; the product never calls it).  EVERY id this library accepts selects a kernel with VALID output — the GEMM ids differ
 * in schedule / geometry only and are bit-identical to each other; an id the build does not contain returns VSYS_ERR_ARG and
 * leaves the selection unchanged.  (Ablation / cycle-stamp variants whose output is NOT valid, and the measured-but-not-shipped
 * ping-pong / persistent / stream-K GEMMs 60 / 70 / 80, exist only in -DVSYS_LAB builds together with
 * include/videosys_amd_lab.h; the shipped library contains no such code, and no launch path of it allocates or synchronises.)
 * gemm:  2GGPP = tile raster only (see vsys_gemm_raster_probe); 0 = shape dispatch (default); 8 = schedule 8 for every shape (three A slots + two W slots, counted waits); 3 / 6 =
 *        two-stage LDS-DMA schedules; 9 = schedule 8, plain row-major tile order; 20 = 4-wave workgroups, two per CU; 28 =
 *        schedule 8 + producer waves; 30 = 256 x 384 tile; 103 = 128-row tiles.
 * flash: 14 / 15 = the 64-query-rows-per-wave kernel with the hand-allocated tile loop wherever it applies (>= 256 keys and rows) /
 *        never (default: for >= 512 keys);  0 = default (two workgroups per CU; resident K/V for few keys; temporal attention on the matrix pipe for T <= 32); 3 = three workgroups per CU;
 *        4 = VALU temporal kernel (v2) for T <= 40; 8 / 10 = the resident-K/V kernel (all KV tiles of a
 *        (batch, head) staged once per workgroup; default for <= 320 keys and many query rows) whenever the keys fit / never;
 *        9 = online-softmax temporal kernel for every T; 12 = the head-dim-64 kernel on a two-stage K/V ring (shipped: three).
 * No reference counterpart (measurement tooling). */
int vsys_tune_gemm_variant(int variant);
int vsys_tune_flash_variant(int variant);
/* Host-only: where the GEMM kernels' tile raster (column groups of gw tiles inside panel chunks of ph panels inside the 8 per-XCD
 * panel groups; vsys_tune_gemm_variant(20000 + 100 gw + ph) selects it for measurements, 20600 = the default) sends logical tile
 * ``tile`` of an nbm x nbn grid: *bm, *bn.  Lets a CPU test check that every raster is a bijection.  No reference counterpart
 * (measurement tooling). */
int vsys_gemm_raster_probe(int64_t tile, int64_t nbm, int64_t nbn, int64_t gw, int64_t ph, int64_t* bm, int64_t* bn);

/* nn.Linear on token rows with fused epilogue (bf16 in/out, fp32 MFMA accumulate).
 * Replaces: attentions.py:59 (qkv), :107 (proj) + open_sora_transformer_3d.py:219,228 (gate, residual);
 * attentions.py:156,183 + open_sora_transformer_3d.py:237-240 (cross q / proj + residual);
 * timm Mlp fc1+GELU(tanh)/fc2 (open_sora_transformer_3d.py:130-132,267,270,284).
 * Requires N % 192 == 0, K % 64 == 0, strides % 8 == 0; any M.  gate may be NULL (= 1), res/aux may be NULL. */
int vsys_gemm_bf16(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* out, int64_t ldo,
                   int64_t M, int64_t N, int64_t K, int epilogue, const void* gate, int64_t gate_sample_stride,
                   int64_t rows_per_sample, const void* res, int64_t ldr, void* aux, int64_t ldaux, void* stream);

/* AdaLN folded into the qkv / fc1 GEMMs: x_m = t2i_modulate(norm(x), shift, scale) followed by the Linear
 * (open_sora_transformer_3d.py:196-197 + attentions.py:59; :260-261 + timm Mlp fc1 :130-132,267) without ever writing x_m:
 *   out[m][n] = rstd_m (sum_k x[m][k] W'[n][k] - mu_m cs[n]) + cv[n]   (+ GELU-tanh for VSYS_EPI_BIAS_GELU)
 * with W' = bf16(W (1 + scale)), cs[n] = sum_k W'[n][k], cv[n] = shift . W[n] + bias[n] (fp32 [N] each, from
 * vsys_adaln_prescale) and the LayerNorm statistics of row m (eps as nn.LayerNorm, :116-117) combined from K / 96 partial
 * (mean, M2) pairs over 96-column blocks: float2 stats[b * stats_ld + m] (written by vsys_gemm_bf16_stats or vsys_ln_row_stats).
 * x is the RAW residual stream [M, K]; K % 96 == 0, K <= 1152; epilogue = VSYS_EPI_BIAS or VSYS_EPI_BIAS_GELU; otherwise as
 * vsys_gemm_bf16. */
int vsys_gemm_bf16_ln(const void* x, int64_t ldx, const void* wp, int64_t ldw, const void* cs, const void* cv, void* out, int64_t ldo,
                      int64_t M, int64_t N, int64_t K, int epilogue, const void* stats, int64_t stats_ld, float eps, void* stream);

/* vsys_gemm_bf16_ln (VSYS_EPI_BIAS) of the SPATIAL qkv site followed by vsys_attn_prep_kv, in one launch: the K and V thirds of the
 * qkv rows never reach memory as rows, the GEMM's epilogue writes the Kp / Vt layouts itself (the k half of the qk-norm and the
 * softmax scale as vsys_attn_prep_kv applies them, attentions.py:59,75 + normalization.py:28-33; same bits).  N = 216 heads output
 * columns (a head = 72) in the K/V COLUMN ORDER: windows of 96 columns, 3 heads / 4 windows of Q in the checkpoint's order, then one
 * window per head h with its 72 K features followed by V features 24 h .. 24 h + 23 (V features counted h_v * 72 + d), then the
 * remaining V features 96 to a window.  wp, cs, cv must be in that order: vsys_adaln_prescale writes them so for a site whose N word
 * carries ``heads`` in its upper half.  Row m is key m % S of sample m / S.  Outputs: q[m][0 .. 72 heads) with leading dimension ldq
 * (what vsys_gemm_bf16_ln stores in its first third), kp [M / S][heads][S][72], vt [M / S][heads][96][S] rows 0-71.  vt rows 72-95 are
 * NOT written: with every key valid they are constants (rows 72 and 76 = 1.0, the rest 0) that the caller sets once.  heads % 8 == 0,
 * S % 64 == 0, M % S == 0, K % 96 == 0, K <= 1152, k_norm_w [72] required and 16-byte aligned; eps: LayerNorm, k_eps: the RMS norm;
 * anything else VSYS_ERR_SHAPE / _ARG / _ALIGN.  Always the two-workgroup 16x16x32 tile kernel. */
int vsys_gemm_bf16_ln_qkv_kv(const void* x, int64_t ldx, const void* wp, int64_t ldw, const void* cs, const void* cv, const void* stats,
                             int64_t stats_ld, const void* k_norm_w, void* q, int64_t ldq, void* kp, void* vt, int64_t M, int64_t K,
                             int64_t S, int64_t heads, float eps, float k_eps, void* stream);
/* 1 when vsys_gemm_bf16_ln at [M, K] x [N, K] runs on that same kernel (so that the fused form replaces a launch of it and not of
 * another tile shape the dispatch prefers there), else 0.  Host-side, no launch; no reference counterpart. */
int vsys_gemm_bf16_ln_qkv_kv_dispatched(int64_t M, int64_t N, int64_t K);

/* vsys_gemm_bf16 with VSYS_EPI_GATE_RES (out = res + gate (x W^T + b): attentions.py:107 / :183 / timm Mlp fc2 + the residual adds
 * of open_sora_transformer_3d.py:228,240,284) that ALSO emits the LayerNorm partials of the rows it stores — what the next block's
 * norm1 / norm2 (open_sora_transformer_3d.py:116-117,196,260) would compute from them: float2 stats[b * stats_ld + m] = (mean, M2)
 * of out[m][96 b .. 96 b + 95].  No aux output; N % 192 == 0. */
int vsys_gemm_bf16_stats(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* out, int64_t ldo, int64_t M,
                         int64_t N, int64_t K, const void* gate, int64_t gate_sample_stride, int64_t rows_per_sample, const void* res,
                         int64_t ldr, void* stats, int64_t stats_ld, void* stream);

/* vsys_gemm_bf16 with VSYS_EPI_GATE_RES whose store phase also takes the `x = x + cached_output` passes that FOLLOW it in program
 * order when the next sub-blocks of the residual stream are PAB broadcasts (open_sora_transformer_3d.py:186-190,219-225,
 * /root/reference/videosys/core/pab/pab_mgr.py:54-91):  out = bf16(bf16(bf16(res + u) + add1) + add2),  u = bf16(gate (x W^T + b)) —
 * the roundings of the separate torch adds.  res is required; add1 / add2 ([M, N], leading dimension ldr) and aux (the PAB slab
 * copy of u, leading dimension ldr) may be NULL; stats (format of vsys_gemm_bf16_stats, may be NULL) receives the LayerNorm
 * partials of the rows stored. */
int vsys_gemm_bf16_gate_res_add(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* out, int64_t ldo,
                                int64_t M, int64_t N, int64_t K, const void* gate, int64_t gate_sample_stride, int64_t rows_per_sample,
                                const void* res, int64_t ldr, void* aux, const void* add1, const void* add2, void* stats,
                                int64_t stats_ld, void* stream);

/* The step-level half of the AdaLN fold: for every site of a step (one qkv or fc1 Linear of one block) W' = bf16(W (1 + scale)),
 * cs, cv as defined at vsys_gemm_bf16_ln, all sites in ONE launch.  shift / scale are the sample-0 rows of the step's modulation
 * table (t2i_modulate operands, open_sora_transformer_3d.py:177-179; valid when every sample of the batch shares the timestep, as
 * the CFG pair of scheduling_rflow_open_sora.py:239-244 does).  ``sites``: DEVICE array of nsites x 10 int64: W, bias, W', cs, cv
 * (addresses), shift_off, scale_off (element offsets into ``mod``), N, K, first block of the site; 4 weight rows per block,
 * nblocks = sum ceil(N / 4).  N word: bits 0-31 = N; bits 32 and up = 0, or ``heads`` of a spatial qkv site (N = 216 heads) whose
 * W', cs, cv are to be written in the K/V column order of vsys_gemm_bf16_ln_qkv_kv (row n at its column; same values). */
int vsys_adaln_prescale(const void* sites, int64_t nsites, int64_t nblocks, const void* mod, void* stream);

/* LayerNorm partials (format of vsys_gemm_bf16_ln) of a [rows, C] bf16 tensor no GEMM epilogue produced: the patch embedding
 * in front of block 0 and the x += cached-output steps of PAB (open_sora_transformer_3d.py:116-117,192-193).  Same accumulation
 * order as the epilogue of vsys_gemm_bf16_stats: the same rows give the same partial bits from either.  C % 96 == 0, C <= 1536. */
int vsys_ln_row_stats(const void* x, int64_t rows, int64_t C, void* stats, int64_t stats_ld, void* stream);

/* Small / odd-shaped nn.Linear (any M, N; K % 8 == 0): act_in is applied to x (SiLU of t_block,
 * open_sora_transformer_3d.py:396-399), act_out to the result (TimestepEmbedder/SizeEmbedder mlp, embeddings.py:114-118;
 * OpenSoraCaptionEmbedder y_proj, embeddings.py:197-203). */
int vsys_linear_small(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* out, int64_t ldo,
                      int64_t M, int64_t N, int64_t K, int act_in, int act_out, void* stream);

/* y = LayerNorm(x, eps, no affine) * (1 + scale[b]) + shift[b], b = row / rows_per_sample.
 * Replaces nn.LayerNorm + t2i_modulate (open_sora_transformer_3d.py:47-48,117,129,196-197,260-261). C % 8 == 0, C <= 2048. */
int vsys_adaln_modulate(const void* x, const void* shift, const void* scale, void* y, int64_t rows, int64_t C,
                        int64_t rows_per_sample, int64_t mod_sample_stride, float eps, void* stream);

/* out[blk][b][6*C] = bf16(table[blk][6*C] + t_mlp[b][6*C])  (open_sora_transformer_3d.py:177-179 for all blocks). */
int vsys_mod_table(const void* table, const void* t_mlp, void* out, int64_t nblk, int64_t B, int64_t C6, void* stream);

/* TimestepEmbedder.timestep_embedding (embeddings.py:123-141): t fp32 [B] -> out bf16 [B, dim] = [cos | sin]. */
int vsys_timestep_embedding(const void* t_f32, void* out, int64_t B, int64_t dim, void* stream);

/* OpenSoraPatchEmbed3D + "x + pos_emb" (embeddings.py:85-104; open_sora_transformer_3d.py:593-595).
 * z fp32 [Bz, Cin, T, H, W]; sample b reads z[b % Bz] (CFG duplicate, scheduling_rflow_open_sora.py:239);
 * w bf16 [C, Cin*ph*pw]; pos bf16 [Hp*Wp, C]; out bf16 [B, T, Hp*Wp, C]. */
int vsys_patch_embed(const void* z_f32, int64_t Bz, const void* w, const void* bias, const void* pos, void* out, int64_t B,
                     int64_t Cin, int64_t T, int64_t H, int64_t W, int64_t ph, int64_t pw, int64_t C, void* stream);

/* T2IFinalLayer + unpatchify + .to(float32) (open_sora_transformer_3d.py:75-87,622-630,634-658).
 * x bf16 [B, T*Hp*Wp, C]; table bf16 [2, C]; tvec bf16 [B, C]; w bf16 [ph*pw*Cout, C]; out fp32 [B, Cout, T, H, W]. */
int vsys_final_layer(const void* x, const void* table, const void* tvec, const void* w, const void* bias, void* out_f32,
                     int64_t B, int64_t T, int64_t Hp, int64_t Wp, int64_t H, int64_t W, int64_t ph, int64_t pw,
                     int64_t Cout, int64_t C, float eps, void* stream);

/* The same two layers on the S-shard of a sequence-parallel rank (DSP at rest: rank r holds tokens r*Sl .. r*Sl+Sl-1 of every
 * (b, t), open_sora_transformer_3d.py:598-603,615-619): the patch embedding is computed for the local tokens only (tokens past
 * Hp*Wp are the zero rows split_sequence pads with), the final layer runs on the local rows and leaves its ph*pw*Cout values per
 * token in tokens_f32 [B, T, Sl, n_out]; after an all-gather of those (0.6 MB per rank at config 2 instead of the 11 MB of hidden
 * state) vsys_unpatchify_tokens scatters [P, B, T, Sl, n_out] into out_f32 [B, Cout, T, H, W].  Same arithmetic per token as the
 * whole-frame entry points. */
int vsys_patch_embed_shard(const void* z_f32, int64_t Bz, const void* w, const void* bias, const void* pos, void* out, int64_t B,
                           int64_t Cin, int64_t T, int64_t H, int64_t W, int64_t ph, int64_t pw, int64_t C, int64_t s0, int64_t Sl,
                           void* stream);
int vsys_final_layer_tokens(const void* x, const void* table, const void* tvec, const void* w, const void* bias, void* tokens_f32,
                            int64_t B, int64_t T, int64_t Sl, int64_t n_out, int64_t C, float eps, void* stream);
int vsys_unpatchify_tokens(const void* tokens_f32, void* out_f32, int64_t P, int64_t B, int64_t T, int64_t Sl, int64_t Hp,
                           int64_t Wp, int64_t H, int64_t W, int64_t ph, int64_t pw, int64_t Cout, void* stream);

/* RFLOW CFG combine + Euler update (scheduling_rflow_open_sora.py:245-252): z fp32 [Bz, Cin, thw] +=
 * (uncond + g (cond - uncond)) * dt with cond = model_out[b, :Cin], uncond = model_out[b + Bz, :Cin]. */
int vsys_cfg_euler_step(void* z_f32, const void* model_out_f32, int64_t Bz, int64_t Cin, int64_t Cout, int64_t thw,
                        float guidance, float dt, void* stream);

/* CFG combine + one linear scheduler update, z fp32 [Bz, Cin, thw] = c_z z + c_eps (uncond + g (cond - uncond)) on the
 * first Cin of Cout predicted channels (learned-sigma half dropped).  DDIM eta = 0
 * (diffusers DDIMScheduler.step as called from pipelines/latte/pipeline_latte.py:864-876 and
 * schedulers/scheduling_ddim_cogvideox.py:299-393 with v-prediction folded on the host):
 * c_z = sqrt(a_prev / a_t), c_eps = sqrt(1 - a_prev) - sqrt(a_prev (1 - a_t) / a_t).
 * cond_first != 0: model_out[b] is the conditional half (RFLOW order); 0: model_out[b + Bz] is (negative prompt first). */
int vsys_cfg_linear_step(void* z_f32, const void* model_out_f32, int64_t Bz, int64_t Cin, int64_t Cout, int64_t thw,
                         float guidance, float c_z, float c_eps, int cond_first, void* stream);

/* x[r, :] += e[(r / group) % period, :] over rows of C bf16 — Latte's temporal position embedding added to the
 * (b, f, s)-ordered hidden states before the first temporal block (latte_transformer_3d.py:1410-1411; group = S,
 * period = F). */
int vsys_add_bcast_rows(void* x, const void* e, int64_t rows, int64_t C, int64_t group, int64_t period, void* stream);

/* x += y over n bf16 elements (PAB broadcast step: x + last_attn / last_cross, open_sora_transformer_3d.py:192-193,228,234-235). */
int vsys_add_rows(void* x, const void* y, int64_t n, void* stream);

/* 4-D strided row copy with zero fill outside (n1_valid, n2_valid): DSP all-to-all pack/unpack
 * (core/distributed/comm.py:104-108,282-304; open_sora_transformer_3d.py:288-315). */
int vsys_copy_4d(const void* src, void* dst, int64_t n0, int64_t n1, int64_t n2, int64_t C, int64_t ss0, int64_t ss1,
                 int64_t ss2, int64_t ds0, int64_t ds1, int64_t ds2, int64_t n1_valid, int64_t n2_valid, void* stream);

/* K RMS-norm (normalization.py:28-33; k_norm_w NULL = none) + head-major K and transposed V for vsys_flash_attn_d72.
 * k(b,s,h) at k + (b*kv_len + s)*k_stride + h*72, same for v.  kp [batch, H, kv_pad, 72]; vt [batch, H, 96, kv_pad]
 * (rows 72..95 must be zero-initialised by the caller once).  kv_pad % 64 == 0.
 * The pair (kp, vt) is an opaque operand of vsys_flash_attn_d72: kp carries the softmax scale 72^-1/2 * log2(e)
 * (folded in before its single bf16 rounding) and vt rows 72 and 76 are written as ones over the valid keys, so the
 * flash kernel gets exp2-ready logits and the softmax denominator from the matrix pipe. */
int vsys_attn_prep_kv(const void* k, int64_t k_stride, const void* v, int64_t v_stride, const void* k_norm_w, void* kp,
                      void* vt, int64_t batch, int64_t heads, int64_t kv_len, int64_t kv_pad, float eps, void* stream);

/* softmax(q k^T / sqrt(72)) v for head_dim 72, non-causal, keys >= kv_len masked; optional q RMS-norm.
 * Spatial self-attention (attentions.py:75,100) and cross-attention (attentions.py:259-270).
 * q(b,s,h) at q + (b*q_len + s)*q_stride + h*72; out likewise with out_stride.
 * Padding: the kernels read the Kp rows and Vt columns of keys kv_len .. 64 ceil(kv_len / 64) - 1 and give them the weight 0 by
 * masking, not by skipping: both MUST BE FINITE there (0 x NaN is NaN: with NaN in the Kp pad rows alone, or in the Vt pad columns
 * alone, every output element is NaN; any finite value gives the bits of zeros).  vsys_attn_prep_kv writes zeros there; a kv_len
 * shorter than the one the buffers were prepared for (Latte's per-sample text lengths) leaves real K / V values, which is fine.
 * The same holds for vsys_flash_attn_d72_kb. */
int vsys_flash_attn_d72(const void* q, int64_t q_stride, const void* q_norm_w, const void* kp, const void* vt, void* out,
                        int64_t out_stride, int64_t batch, int64_t heads, int64_t q_len, int64_t kv_len, int64_t kv_pad,
                        float eps, void* stream);

/* vsys_flash_attn_d72 for the cross attention against hoisted text K / V (attentions.py:259-270; kv_linear of the packed prompt
 * :157, :240-258) with a promise about the PADDING: (kp, vt) were written by vsys_attn_prep_kv for exactly this kv_len into
 * zero-initialised buffers, so every Kp row and Vt column behind kv_len is zero — including the ones rows of Vt.  A padding key then
 * has logit 0 and weight 0 in numerator and denominator, and the kernels that take the promise (the resident-K/V cross-attention
 * kernel) drop the mask of the ragged last tile.  Same results as vsys_flash_attn_d72 to the last bit of the tolerance (P of the last
 * tile may be rounded at another scale when a padding key raises the running max); a row whose real logits all lie ~100 (exp2
 * domain) below zero is detected and recomputed with the mask.  NOT valid when kv_len is SHORTER than what the buffers were
 * prepared for (Latte's per-sample text lengths inside one buffer: call vsys_flash_attn_d72).  kv_len % 64 == 0: identical to
 * vsys_flash_attn_d72. */
int vsys_flash_attn_d72_exact(const void* q, int64_t q_stride, const void* q_norm_w, const void* kp, const void* vt, void* out,
                              int64_t out_stride, int64_t batch, int64_t heads, int64_t q_len, int64_t kv_len, int64_t kv_pad,
                              float eps, void* stream);

/* vsys_attn_prep_kv for a batch whose samples have DIFFERENT key counts: the reference's varlen cross-attention path
 * (attentions.py:240-258; the packed text of open_sora_transformer_3d.py:526-537).  k / v are rows of the PACKED text
 * (sum(lens) rows, sample after sample), cu_seqlens is a device int32[batch + 1] of row offsets (cu[0] = first row of sample 0,
 * lens[b] = cu[b + 1] - cu[b]).  kp[b] / vt[b] get exactly what vsys_attn_prep_kv writes for kv_len = lens[b]: scale folded into Kp,
 * ones rows 72 and 76 of Vt over the valid keys, zeros behind lens[b] up to kv_pad (Vt rows 73..75, 77..95 are not written: zero
 * them once, as for vsys_attn_prep_kv).  One launch for the batch.  cu_seqlens_host is a HOST copy of the same batch + 1 numbers:
 * the entry point validates with it (no device read-back) — any lens[b] < 1 or > kv_pad, or cu[0] < 0, is VSYS_ERR_SHAPE and
 * nothing is launched.  The caller guarantees that k and v hold cu[batch] rows. */
int vsys_attn_prep_kv_varlen(const void* k, int64_t k_stride, const void* v, int64_t v_stride, const void* k_norm_w,
                             const int* cu_seqlens, const int* cu_seqlens_host, void* kp, void* vt, int64_t batch, int64_t heads,
                             int64_t kv_pad, float eps, void* stream);

/* vsys_flash_attn_d72_exact for a batch whose samples have DIFFERENT key counts, in one launch: sample b attends to its own
 * kv_lens[b] keys (attentions.py:240-258, flash_attn_varlen_func over the packed text; open_sora_transformer_3d.py:526-537).
 * kv_lens is a device int32[batch]: the workgroup of (b, h) reads its count there (one scalar load), so a recorded launch program
 * replays the call with no key count baked in.  Carries the padding promise of vsys_flash_attn_d72_exact PER SAMPLE: (kp, vt) were
 * written by vsys_attn_prep_kv_varlen for exactly these counts into zero-initialised buffers; the underflow guard of that entry
 * point applies per query block.  kv_lens_host is a HOST copy of the same numbers, read at every call (also at every replay of a
 * recorded call: keep it alive and unchanged).  With it the entry point validates — any count < 1 or > kv_pad is VSYS_ERR_SHAPE,
 * nothing is launched — and picks the kernel: max(kv_lens) <= 320 keys runs the resident-K/V kernel once for the whole batch; what
 * that kernel does not take (longer text, q_len * q_stride past its 32-bit staging offsets, VSYS_FLASH_VARIANT or VSYS_FLASH_EXACT
 * selecting another kernel) is answered by one vsys_flash_attn_d72_exact launch per sample with kv_len = kv_lens_host[b] — same
 * results, batch launches. */
int vsys_flash_attn_d72_varlen(const void* q, int64_t q_stride, const void* q_norm_w, const void* kp, const void* vt,
                               const int* kv_lens, const int* kv_lens_host, void* out, int64_t out_stride, int64_t batch,
                               int64_t heads, int64_t q_len, int64_t kv_pad, float eps, void* stream);

/* vsys_flash_attn_d72 (attentions.py:75,100) with a promise about the keys: k_norm_bound >= the Euclidean norm of every Kp row (as stored: normed, scaled
 * by log2(e) / sqrt(72)).  For an RMS-normed key that is sqrt(72) max|k_norm.weight| log2(e) / sqrt(72) (1 + rounding), a property
 * of the WEIGHTS (normalization.py:28-33): the caller computes it once per block.  By Cauchy-Schwarz m_i = |q_i| k_norm_bound bounds
 * every logit of query row i, and softmax is invariant under the choice of the subtracted m: the kernels that take the promise
 * (64 rows per wave, attention_w64.hip) use exp2(s - m_i) with no running maximum and no rescale of the accumulator.  The caller
 * must also guarantee |q_i| k_norm_bound <= 60 for every query row (RMS-normed q: sqrt(72) max|q_norm.weight| k_norm_bound):
 * 2 m < 126 keeps every row sum representable.  k_norm_bound = 0: exactly vsys_flash_attn_d72.  q_norm_w == NULL: the bound is
 * ignored.  The BITS of vsys_flash_attn_d72 are not promised (P is rounded to bf16 at another scale): the same tolerance is. */
int vsys_flash_attn_d72_kb(const void* q, int64_t q_stride, const void* q_norm_w, const void* kp, const void* vt, void* out,
                           int64_t out_stride, int64_t batch, int64_t heads, int64_t q_len, int64_t kv_len, int64_t kv_pad,
                           float eps, float k_norm_bound, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * CogVideoX: joint [text | video] blocks, head_dim 64.
 * ------------------------------------------------------------------------------------------------------------------ */

/* vsys_gemm_bf16 with VSYS_EPI_GATE_RES and TWO gate vectors per sample: rows whose position inside the sample is
 * < seg_split (the text tokens) read the gate gate_alt elements after the sample's gate pointer
 * (CogVideoXBlock.forward: hidden + gate_msa * attn / encoder_hidden + enc_gate_msa * attn,
 * cogvideox_transformer_3d.py:288-289,300-301; gates from CogVideoXLayerNormZero, modules/normalization.py:52-59). */
int vsys_gemm_bf16_gate2(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* out, int64_t ldo,
                         int64_t M, int64_t N, int64_t K, const void* gate, int64_t gate_sample_stride,
                         int64_t rows_per_sample, int64_t seg_split, int64_t gate_alt, const void* res, int64_t ldr,
                         void* aux, int64_t ldaux, void* stream);

/* y = (LayerNorm(x) * ln_w + ln_b) * (1 + scale) + shift over rows of C bf16 (C <= 3072).  ln_w/ln_b NULL: no affine;
 * shift/scale NULL: no modulation (nn.LayerNorm norm_final, cogvideox_transformer_3d.py:566-572).  shift/scale point at
 * sample 0's vectors (sample stride mod_sample_stride); rows at position < seg_split inside their sample read them
 * mod_alt elements further on (CogVideoXLayerNormZero, modules/normalization.py:36-60; AdaLayerNorm chunk_dim=1 :62-114). */
int vsys_ln_modulate(const void* x, const void* ln_w, const void* ln_b, const void* shift, const void* scale, void* y,
                     int64_t rows, int64_t C, int64_t rows_per_sample, int64_t mod_sample_stride, int64_t seg_split,
                     int64_t mod_alt, float eps, void* stream);

/* x[r] += gate[sample(r)] * y[r] with the two-segment gate addressing above: the PAB broadcast step of CogVideoXBlock
 * re-gates the cached, un-gated attention output (cogvideox_transformer_3d.py:276-289). */
int vsys_gate_add_rows(void* x, const void* y, const void* gate, int64_t rows, int64_t C, int64_t rows_per_sample,
                       int64_t gate_sample_stride, int64_t seg_split, int64_t gate_alt, void* stream);

/* CogVideoXPatchEmbed's Conv2d(k = s = p) operand (modules/embeddings.py:14-51): z fp32 [Bz, F, Cin, H, W] (sample b reads
 * z[b % Bz]) -> out bf16 [B*F*(H/p)*(W/p), Cin*p*p] with columns ordered (c, dy, dx) like the flattened conv weight. */
int vsys_im2col_patch(const void* z_f32, int64_t Bz, void* out, int64_t B, int64_t F, int64_t Cin, int64_t H, int64_t W,
                      int64_t p, void* stream);

/* CogVideoX unpatchify (cogvideox_transformer_3d.py:581-583): x bf16 [(b, f, hp, wp)] rows of ldx >= Cout*p*p elements,
 * columns ordered (c, dy, dx) -> out fp32 [B, F, Cout, Hp*p, Wp*p]. */
int vsys_unpatchify_cvx(const void* x, int64_t ldx, void* out_f32, int64_t B, int64_t F, int64_t Hp, int64_t Wp, int64_t Cout,
                        int64_t p, void* stream);

/* K side of CogVideoXAttnProcessor2_0 (cogvideox_transformer_3d.py:108,127-149): LayerNorm qk-norm (ln_w/ln_b [64] or NULL),
 * rotary embedding on tokens rope_start <= s < rope_start + rope_len (cos/sin fp32 [rope_len, 64], NULL = none), softmax
 * scale folded in; head-major K (16-byte chunks of a row stored at chunk ^ ((row>>1)&7): an operand private to
 * vsys_flash_attn_d64) and transposed V.  kp [batch, H, kv_pad, 64], vt [batch, H, 64, kv_pad], kv_pad % 64 == 0. */
int vsys_attn_prep_kv64(const void* k, int64_t k_stride, const void* v, int64_t v_stride, const void* ln_w, const void* ln_b,
                        const void* rope_cos_f32, const void* rope_sin_f32, int64_t rope_start, int64_t rope_len, void* kp,
                        void* vt, int64_t batch, int64_t heads, int64_t kv_len, int64_t kv_pad, float eps, void* stream);

/* softmax(q k^T / 8) v for head_dim 64, non-causal (F.scaled_dot_product_attention in CogVideoXAttnProcessor2_0,
 * cogvideox_transformer_3d.py:151-158), with the q side of the processor above (LayerNorm + RoPE, :108-149) applied on
 * the fly.  q(b,s,h) at q + (b*q_len + s)*q_stride + h*64; out likewise. */
int vsys_flash_attn_d64(const void* q, int64_t q_stride, const void* ln_w, const void* ln_b, const void* rope_cos_f32,
                        const void* rope_sin_f32, int64_t rope_start, int64_t rope_len, const void* kp, const void* vt, void* out,
                        int64_t out_stride, int64_t batch, int64_t heads, int64_t q_len, int64_t kv_len, int64_t kv_pad, float eps,
                        void* stream);

/* vsys_flash_attn_d64 (cogvideox_transformer_3d.py:108-158) with the promise of vsys_flash_attn_d72_kb about the Kp rows (LayerNorm qk-norm with affine weights, rotary
 * embedding, scale log2(e) / 8: |k| <= (8 max|w| + |b|_2) log2(e) / 8, a property of the block's norm_k weights): no running
 * maximum in the kernels that take it (attention64_w64.hip).  |q_i| k_norm_bound <= 60 for every query row is the caller's to
 * guarantee (|q_i| <= 8 max|norm_q.weight| + |norm_q.bias|_2).  0 = exactly vsys_flash_attn_d64. */
int vsys_flash_attn_d64_kb(const void* q, int64_t q_stride, const void* ln_w, const void* ln_b, const void* rope_cos_f32,
                        const void* rope_sin_f32, int64_t rope_start, int64_t rope_len, const void* kp, const void* vt, void* out,
                        int64_t out_stride, int64_t batch, int64_t heads, int64_t q_len, int64_t kv_len, int64_t kv_pad, float eps, float k_norm_bound,
                        void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Open-Sora-Plan v1.2 (OpenSoraT2V): full 3-D self-attention and masked cross-attention at head_dim 96.
 * Neither entry point has a VSYS_OP code (the op table keeps its size): a launch program replays them from a host closure.
 * ------------------------------------------------------------------------------------------------------------------ */

/* K side of AttnProcessor2_0 (open_sora_plan_v120_transformer_3d.py:886-1128) with RoPE3D (:63-118): the 96 columns of a head are
 * three chunks of 32 (frame, row, column position); inside a chunk out = x cos + rotate_half(x) sin, rotate_half = (-x[16:32],
 * x[0:16]).  rope_cos / rope_sin: fp32 [kv_len, 96], one row per KEY TOKEN (the same tables for every sample and head), applied
 * column by column; NULL = no rotation (cross-attention).  Rounding: k^ = bf16((fp32(k cos) + fp32(rot(k) sin)) * 96^-0.5 log2(e)):
 * two fp32 products and one fp32 sum (no fused multiply-add), the softmax scale in fp32, ONE rounding to bf16.
 * kp [batch, H, kv_pad, 96] plain rows, vt [batch, H, 96, kv_pad] transposed V, kv_pad % 64 == 0; keys kv_len <= s < kv_pad are
 * written as zeros in both.  k(b, s, h) at k + (b*kv_len + s)*k_stride + h*96, v likewise; strides % 8 == 0.  k, v, kp, vt and the
 * tables are read / written 16 bytes at a time: a base pointer that is not 16-byte aligned is VSYS_ERR_ALIGN. */
int vsys_attn_prep_kv96(const void* k, int64_t k_stride, const void* v, int64_t v_stride, const void* rope_cos_f32,
                        const void* rope_sin_f32, void* kp, void* vt, int64_t batch, int64_t heads, int64_t kv_len, int64_t kv_pad,
                        void* stream);

/* softmax(q k^T / sqrt(96)) v for head_dim 96, non-causal (F.scaled_dot_product_attention in AttnProcessor2_0,
 * open_sora_plan_v120_transformer_3d.py:1090-1110), q rotated on the fly: q^ = bf16(fp32(q cos) + fp32(rot(q) sin)) with
 * rope_cos / rope_sin fp32 [q_len, 96] (NULL = none).  (kp, vt) are the layouts of vsys_attn_prep_kv96.  Keys >= kv_len are masked;
 * with kv_lens (device int32 [batch], NULL = none) sample b attends to its first min(kv_lens[b], kv_len) keys — the count is read
 * on the device, so a replayed launch carries no count; kv_lens[b] < 1 is the caller's error (that sample's rows are not finite).
 * The logits of masked keys are overwritten, so Kp may hold anything there; their Vt entries must be FINITE (they are multiplied by
 * a zero probability): the zeros vsys_attn_prep_kv96 writes behind kv_len, or the ordinary values of padded text tokens.
 * Logits and the running maximum in fp32, P rounded to bf16 for P V, the row sum from the fp32 p, one division, one rounding.
 * q(b, s, h) at q + (b*q_len + s)*q_stride + h*96, out likewise; q_stride % 8 == 0, out_stride % 4 == 0.  Writes only the q_len
 * rows x heads*96 columns of out.  Base pointers: q, kp, vt and the tables 16-byte aligned, out 8-byte, kv_lens 4-byte, else
 * VSYS_ERR_ALIGN. */
int vsys_flash_attn_d96(const void* q, int64_t q_stride, const void* rope_cos_f32, const void* rope_sin_f32, const void* kp,
                        const void* vt, const void* kv_lens_i32, void* out, int64_t out_stride, int64_t batch, int64_t heads,
                        int64_t q_len, int64_t kv_len, int64_t kv_pad, void* stream);

/* vsys_attn_prep_kv96 on a sequence-parallel exchange image (the receive image [P (source)][B][Nl][...] of the Ulysses all-to-all,
 * open_sora_plan_v120_transformer_3d.py:916-941 all_to_all_comm): the same arithmetic, tile walk, LDS use and rounding, RoPE tables
 * indexed by the global token s, the same Kp / Vt layouts, hence the same bits; only the row of token s differs.  The kv_len tokens of
 * a sample lie in slabs of seg_len tokens (slab = the rank the tokens came from): token s of sample b is row
 *     (s / seg_len) * slab_rows + b * seg_len + s % seg_len
 * of k and of v, each with its own row stride.  Tokens past kv_len in the last slab are neither read nor written, nor are the rows
 * between batch * seg_len and slab_rows of a slab.  seg_len >= 1.  seg_len >= kv_len is one slab (slab_rows is then unused) whose
 * samples lie seg_len rows apart: seg_len == kv_len is exactly vsys_attn_prep_kv96's call.  With more than one slab, slab_rows below
 * batch * seg_len is VSYS_ERR_SHAPE.  Alignment and stride checks as vsys_attn_prep_kv96.  Not in the op table: a recorded step
 * issues it from a host closure (program.host_call). */
int vsys_attn_prep_kv96_img(const void* k, int64_t k_stride, const void* v, int64_t v_stride, const void* rope_cos_f32,
                            const void* rope_sin_f32, void* kp, void* vt, int64_t batch, int64_t heads, int64_t kv_len, int64_t kv_pad,
                            int64_t seg_len, int64_t slab_rows, void* stream);

/* vsys_flash_attn_d96 with q and out as exchange images (the attention between the two all_to_all_comm calls of
 * open_sora_plan_v120_transformer_3d.py:916-941): token s of sample b is row
 *     (s / seg_len) * q_slab_rows + b * seg_len + s % seg_len            of q    (the receive image of the way there)
 *     (s / seg_len) * out_slab_rows + b * seg_len + s % seg_len          of out  (the send image of the way back)
 * each with its own row stride; the RoPE tables are indexed by the global token s and (kp, vt, kv_lens) are vsys_flash_attn_d96's.
 * Same arithmetic, tile walk and rounding, hence the same bits as vsys_flash_attn_d96 on the gathered rows.  Query tokens past q_len
 * in the last slab are neither read nor written, nor are the rows between batch * seg_len and the slab stride.  seg_len >= 1;
 * seg_len >= q_len is one slab (the slab strides are then unused), seg_len == q_len exactly vsys_flash_attn_d96's call; with more
 * than one slab a slab stride below batch * seg_len is VSYS_ERR_SHAPE.  Alignment and stride checks as vsys_flash_attn_d96.  Not in
 * the op table: a recorded step issues it from the host closure of the collective it feeds (program.host_call). */
int vsys_flash_attn_d96_img(const void* q, int64_t q_stride, const void* rope_cos_f32, const void* rope_sin_f32, const void* kp,
                            const void* vt, const void* kv_lens_i32, void* out, int64_t out_stride, int64_t batch, int64_t heads,
                            int64_t q_len, int64_t kv_len, int64_t kv_pad, int64_t seg_len, int64_t q_slab_rows, int64_t out_slab_rows,
                            void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Open-Sora-Plan v1.1 (LatteT2V with use_rope): spatial self-attention at head_dim 72 with RoPE2D.
 * The reference rotates rotate-half inside the row half and the column half of a head (RoPE2D,
 * open_sora_plan_v110_transformer_3d.py:136-196, called from AttnProcessor2_0 :1142-1154, :1228-1238).  Attention logits do not change
 * when the same column permutation is applied inside every head to q and to k, so the caller permutes the to_q / to_k output rows
 * once at load time such that every rotate-half pair (j, j + 18) of a half becomes the neighbours (2p, 2p + 1), and these two entry
 * points rotate INTERLEAVED pairs.  Neither has a VSYS_OP code (the op table keeps its size): a launch program replays them from a
 * host closure.
 * ------------------------------------------------------------------------------------------------------------------ */

/* K side of AttnProcessor2_0 with use_rope (open_sora_plan_v110_transformer_3d.py:1220-1244, RoPE2D.forward :167-184): vsys_attn_prep_kv
 * without the K norm, with a per-key rotation before the scale.  rope_cos_f32 / rope_sin_f32: fp32 [kv_len, 36],
 * entry p of row s belongs to the column pair (2p, 2p + 1) of every head of key s; ONE table serves every batch item (the batch is
 * the (sample, frame) pairs, every frame has the same token grid) and every head.  NULL tables are VSYS_ERR_SHAPE: that case is
 * vsys_attn_prep_kv.  Rounding: k^[2p] = bf16((fp32(k[2p] c) - fp32(k[2p+1] s)) * KSCALE), k^[2p+1] = bf16((fp32(k[2p+1] c) +
 * fp32(k[2p] s)) * KSCALE): two fp32 products and one fp32 sum (no fused multiply-add), KSCALE = 72^-1/2 * log2(e) the fp32 constant
 * vsys_attn_prep_kv folds in, ONE rounding.  Writes exactly the opaque (kp, vt) pair of vsys_attn_prep_kv — same layouts, the ones
 * rows 72 and 76 of vt over the valid keys, zeros behind kv_len up to kv_pad — so every vsys_flash_attn_d72* entry point consumes
 * it.  Strides % 8 == 0, kv_pad % 64 == 0; k, v, kp, vt and the tables 16-byte aligned, else VSYS_ERR_ALIGN. */
int vsys_attn_prep_kv_rope(const void* k, int64_t k_stride, const void* v, int64_t v_stride, const void* rope_cos_f32,
                           const void* rope_sin_f32, void* kp, void* vt, int64_t batch, int64_t heads, int64_t kv_len, int64_t kv_pad,
                           void* stream);

/* Q side and the attention of AttnProcessor2_0 with use_rope (open_sora_plan_v110_transformer_3d.py:1213-1252): vsys_flash_attn_d72
 * without the q norm, with Q rotated in the prologue: q^[2p] = bf16(fp32(q[2p] c) - fp32(q[2p+1] s)),
 * q^[2p+1] = bf16(fp32(q[2p+1] c) + fp32(q[2p] s)) with rope_cos_f32 / rope_sin_f32 fp32 [q_len, 36] (one table for every batch
 * item and head; NULL is VSYS_ERR_SHAPE); two fp32 products, one fp32 sum, no fused multiply-add, ONE rounding.  Everything after the
 * prologue is the 32-rows-per-wave streaming kernel of vsys_flash_attn_d72: same tile walk, same masking of keys >= kv_len, same
 * padding rules for Kp / Vt.  It ALWAYS runs that kernel: it never dispatches to the generated 64-row instruction streams or to the
 * resident-K/V kernel (neither carries a rotation).  v1.1's spatial attention is 1 024 keys per frame at 512 x 512, where the 32-row
 * kernel is vsys_flash_attn_d72's default as well.  q_stride % 8 == 0, out_stride % 4 == 0; q, kp, vt and the tables 16-byte
 * aligned, out 8-byte, else VSYS_ERR_ALIGN. */
int vsys_flash_attn_d72_rope(const void* q, int64_t q_stride, const void* rope_cos_f32, const void* rope_sin_f32, const void* kp,
                             const void* vt, void* out, int64_t out_stride, int64_t batch, int64_t heads, int64_t q_len,
                             int64_t kv_len, int64_t kv_pad, void* stream);

/* Temporal self-attention over the T frames of every (b, s) token: RMS qk-norm, RoPE (cos/sin fp32 [T, 72], NULL =
 * none), fp32 softmax (attentions.py:75-78,95-97,111-120; open_sora_transformer_3d.py:203-206).
 * q_norm_w == k_norm_w == NULL: no qk-norm (Latte temporal blocks, latte_transformer_3d.py:680-760).
 * qkv bf16 rows ordered (b, t, s), row_stride elements per row, q|k|v at column offsets 0|C|2C, head h at h*72. */
int vsys_attn_temporal_d72(const void* qkv, int64_t row_stride, int64_t C, const void* q_norm_w, const void* k_norm_w,
                           const void* rope_cos_f32, const void* rope_sin_f32, void* out, int64_t out_stride, int64_t B,
                           int64_t T, int64_t S, int64_t heads, float eps, void* stream);

/* Temporal self-attention of Vchitect-2.0 at head dim 64 (VchitectAttnProcessor.temporal_attention, attentions.py:705-764, without
 * the projections): every token (b, s'), s' in [0, S + L), attends over its own T frames; the L text tokens of a frame follow its S
 * video tokens.  Video rows ordered (b, t, s) in q_vid / k_vid / v_vid / out_vid, text rows ordered (b, t, l) in q_txt / k_txt /
 * v_txt / out_txt, every tensor with its own row stride (elements, % 8 == 0, >= heads * 64; pointers 16-byte aligned), head h at
 * column 64 h.  No qk-norm.  RoPE as apply_rotary_emb (:654-665): the interleaved pair (2i, 2i + 1) of frame t times
 * (cos, sin)[t][i] in fp32, cast back to bf16 (cos / sin fp32 [T, 32]; both NULL = none).  fp32 softmax, scale 1/8.  Any T >= 1,
 * heads >= 1, S + L >= 1 (S == 0 or L == 0: that side's pointers are not read). */
int vsys_attn_temporal_d64(const void* q_vid, int64_t q_vid_stride, const void* k_vid, int64_t k_vid_stride, const void* v_vid,
                           int64_t v_vid_stride, const void* q_txt, int64_t q_txt_stride, const void* k_txt, int64_t k_txt_stride,
                           const void* v_txt, int64_t v_txt_stride, const void* rope_cos_f32, const void* rope_sin_f32, void* out_vid,
                           int64_t out_vid_stride, void* out_txt, int64_t out_txt_stride, int64_t B, int64_t T, int64_t S, int64_t L,
                           int64_t heads, void* stream);

/* vsys_attn_temporal_d64 on the receive image of a sequence-parallel frame -> token switch (attentions.py:733-757 dynamic_switch):
 * the same arithmetic, tile walk and rounding, hence the same bits; only the row of frame t differs.  The T real frames lie in slabs of
 * Tl frames (slab = the rank the frames came from): frame t of token (b, s) is row
 *     (t / Tl) * slab_rows + (b * Tl + t % Tl) * n + s          n = S (video tensors, slab_vid_rows) or L (text, slab_txt_rows)
 * of q / k / v AND of the output, which is therefore the image the return collective sends.  Frames past T in the last slab are
 * neither read nor written.  Tl >= 1.  Tl >= T is one slab (the slab strides are then unused) whose samples lie Tl frames apart:
 * Tl == T is exactly vsys_attn_temporal_d64's call, Tl > T the same with Tl - T unused frames behind every sample.  With more than one
 * slab a slab stride below B * Tl * n is refused.  All other checks as vsys_attn_temporal_d64.  Not in the op table:
 * a recorded step issues it from the host closure of the collective it feeds (program.host_call). */
int vsys_attn_temporal_d64_img(const void* q_vid, int64_t q_vid_stride, const void* k_vid, int64_t k_vid_stride, const void* v_vid,
                               int64_t v_vid_stride, const void* q_txt, int64_t q_txt_stride, const void* k_txt, int64_t k_txt_stride,
                               const void* v_txt, int64_t v_txt_stride, const void* rope_cos_f32, const void* rope_sin_f32, void* out_vid,
                               int64_t out_vid_stride, void* out_txt, int64_t out_txt_stride, int64_t B, int64_t T, int64_t Tl,
                               int64_t slab_vid_rows, int64_t slab_txt_rows, int64_t S, int64_t L, int64_t heads, void* stream);

/* out[r] = bf16(bf16(a[r] * scale) + b[r]) over rows of C bf16 (C % 8 == 0; strides in elements, % 8 == 0), out may be a or b:
 * `hidden_states * 1.1 + cross_output` of VchitectAttnProcessor (attentions.py:899) with the reference's two roundings. */
int vsys_scale_add_rows(const void* a, int64_t a_stride, const void* b, int64_t b_stride, void* out, int64_t out_stride, int64_t rows,
                        int64_t C, float scale, void* stream);

/* Up to 16 vsys_copy_4d problems over one (src, dst) pair in a single launch: the per-peer pack (or unpack) pieces of a DSP /
 * Ulysses all-to-all (comm.py:104-108,282-304; cogvideox_transformer_3d.py:45-86).  desc (HOST) holds nops x 14 int64:
 * src_off, dst_off, n0, n1, n2, run, ss0, ss1, ss2, ds0, ds1, ds2, n1_valid, n2_valid (elements; run % 8 == 0). */
int vsys_copy_4d_batch(const void* src, void* dst, int64_t nops, const int64_t* desc, void* stream);

/* The whole layout switch of Dynamic Sequence Parallelism in ONE launch per rank, peer to peer over xGMI (comm.py:104-141 _all_to_all_func
 * and :282-304 all_to_all_with_pad around open_sora_transformer_3d.py:288-315 dynamic_switch; replaces pack + all_to_all_single + unpack).
 * Problem i of the batch copies rows of ``src`` straight into the DESTINATION tensor of peer i in its final layout: desc (HOST) holds
 * nops x 17 int64 — the 14 of vsys_copy_4d_batch (dst_off relative to the problem's own destination), then the destination base
 * address (this process's mapping of the peer's tensor: vsys_p2p_ipc_open, or a plain device pointer inside one process), the
 * address of flag[self_index] in that peer's flag array (0 for the rank's own problem) and 1 when ANOTHER process or device reads
 * that destination (its rows then leave as system-scope write-through stores; 0: a reader ordered by launches on this device).  After the write-through stores of EVERY problem of the
 * launch have been acknowledged (drained per wave, counted per workgroup) the launch's last workgroup stores the exchange's sequence number into each
 * peer's flag (a relaxed system-scope store: the ordering comes from the drained write-through payload, there is no release fence); the launch ends when every flag q != self_index of
 * ``my_flags`` (n_flags x uint32, fine-grained memory: vsys_p2p_alloc) has reached that number, i.e. when this rank's own destination
 * is complete: the consumer is simply the next launch on ``stream``.  ``state``: 19 x 32 uint32 (one 128-byte line per word) of zeroed
 * device memory private to this exchange site — word 0 the sequence number (advanced by the kernel itself, so a recorded launch
 * program replays unchanged), word 18 (uint32 index 576) an error word (0; 1 + q when peer q's flag did not arrive within ``timeout_ticks`` of the 100 MHz wall clock; sticky: a site that timed
 * out once no longer waits; timeout_ticks 0 = wait for ever, < 0 = do not wait at all: the caller orders the peers' launches itself).
 * Every rank of the group must issue the same sequence of exchanges per site. */
int vsys_p2p_exchange(const void* src, int64_t nops, const int64_t* desc, const void* my_flags, int64_t n_flags, int64_t self_index,
                      void* state, int64_t timeout_ticks, void* stream);
/* Set-up of vsys_p2p_exchange (host side, synchronous, never inside a step; no reference counterpart: the reference's exchange is
 * torch.distributed over NCCL, comm.py:104-141).  Zeroed device memory — fine-grained (flags: polled inside a running kernel while a
 * peer stores to them) or ordinary. */
int vsys_p2p_alloc(int64_t bytes, int64_t fine_grained, void** ptr);
/* Release of vsys_p2p_alloc memory (no reference counterpart). */
int vsys_p2p_free(void* ptr);
/* The 64-byte HIP IPC handle of a vsys_p2p_alloc allocation, for the other rank processes (no reference counterpart). */
int vsys_p2p_ipc_export(const void* ptr, void* handle64);
/* Mapping of a peer process's handle into this process: a device pointer valid here (no reference counterpart). */
int vsys_p2p_ipc_open(const void* handle64, void** ptr);
/* Unmapping of vsys_p2p_ipc_open (no reference counterpart). */
int vsys_p2p_ipc_close(void* ptr);

/* ---- T5 text encoder (T5EncoderModel of transformers, third-party; called once per prompt at pipeline_open_sora.py:269-287,
 * pipeline_cogvideox.py:211-247, pipeline_latte.py) — the linears are vsys_conv_bf16 with one tap. */
/* out[i, :] = table[ids[i], :] (nn.Embedding = T5Stack.embed_tokens, transformers, third-party; ids int64 on the device, clamped
 * to [0, vocab)). */
int vsys_gather_rows(const void* table, const void* ids_i64, void* out, int64_t n, int64_t C, int64_t vocab, void* stream);
/* T5LayerNorm (transformers modeling_t5.py, third-party): y = w * bf16(x * rsqrt(mean(x^2) + eps)), fp32 statistics, C <= 8192. */
int vsys_rms_norm_rows(const void* x, const void* w, void* y, int64_t rows, int64_t C, float eps, void* stream);
/* T5DenseGatedActDense (transformers modeling_t5.py, third-party): out[r, f] = bf16(gelu_new(h[r, f])) * h[r, F + f],
 * h = [wi_0 x | wi_1 x] of 2F columns. */
int vsys_geglu(const void* h, void* out, int64_t rows, int64_t F, void* stream);
/* Finish of a split-K, transposed skinny linear (few activation rows against a large weight — T5 at 300 tokens: every weight byte
 * is used for 300 MACs, so the layer is a weight stream): the GEMM ran as vsys_conv_bf16 with the WEIGHT as the row operand, the
 * activations as the 128-column operand and S slices of K in the batch dimension, leaving part_f32[s][n][m] (row pitch ldp >= M,
 * slice pitch slab elements); out[m][n] = bf16(sum_s part[s][n][m]) (+ res[m][n], added after the rounding).
 * Replaces the tail of nn.Linear inside transformers' T5Attention / T5DenseGatedActDense (third-party; call sites
 * pipeline_open_sora.py:269-287). */
int vsys_splitk_reduce_t(const void* part_f32, int64_t nsplit, int64_t slab, int64_t ldp, const void* res, int64_t ldr, void* out, int64_t ldo,
                         int64_t M, int64_t N, void* stream);
/* T5Attention (transformers modeling_t5.py, third-party; encoder self-attention, d_kv = 64, no score scaling):
 * softmax_j(q_i k_j + relbias[h][j - i + L - 1]) v over the
 * first klen[b] keys.  qkv rows (b, l) of row_stride elements, q | k | v at column 0 | inner | 2 inner, head h at h*64;
 * relbias fp32 [heads, 2L-1]; klen int32 [B] on the device; L <= 512. */
int vsys_t5_attention(const void* qkv, int64_t row_stride, int64_t inner, const void* relbias_f32, const void* klen_i32, void* out,
                      int64_t out_stride, int64_t B, int64_t L, int64_t heads, void* stream);
/* The weight-streaming linear on the 256 x 384 tile (one 8-wave workgroup per CU): part_f32[s][m][n] = sum over K slice s of
 * x[m][k] w[n][k] for m < rows (x holds rows_padded rows, a multiple of 384; the rows past the real ones are multiplied but not
 * stored), n < N, nsplit slices of ceil(K / 32 / nsplit) * 32 columns (the last one takes what is left; K % 32 == 0).  Every 256-row weight panel is read by exactly one workgroup.  vsys_splitk_reduce then
 * gives out[m][n] = bf16(sum_s part[s][m][n]) (+ res[m][n] after the rounding), slab = rows_padded * N, ldp = N.
 * Replaces nn.Linear inside transformers' T5 stack at a few hundred rows (third-party; call sites pipeline_open_sora.py:269-287). */
int vsys_gemm_skinny_slices(const void* w, int64_t ldw, const void* x, int64_t ldx, void* part_f32, int64_t rows, int64_t rows_padded,
                            int64_t N, int64_t K, int64_t nsplit, void* stream);
int vsys_splitk_reduce(const void* part_f32, int64_t nsplit, int64_t slab, int64_t ldp, const void* res, int64_t ldr, void* out, int64_t ldo,
                       int64_t M, int64_t N, void* stream);
/* The same attention (T5Attention, transformers modeling_t5.py, third-party; call sites pipeline_open_sora.py:269-287) on the matrix
 * pipe, ONE sample per call (its own key length kv_len <= L): the head_dim-64 flash kernel with
 * an additive (head, key - query) logit bias.  qkv bf16 rows [L, 3*inner] (q | k | v, head h at h*64); bias_f32 [heads, bias_ld]
 * holds log2(e) * T5Attention.compute_bias, entry of (h, key - query) at bias_center + key - query, padded by the caller so that
 * every key < 64*ceil(L/64) and query < 128*ceil(L/128) stays inside (bias_center >= 128*ceil(L/128) - 1, bias_ld >= bias_center +
 * 64*ceil(L/64)); kp / vt: workspaces of heads * 64*ceil(L/64) * 64 bf16 each (the K / V^T layouts of vsys_attn_prep_kv64). */
int vsys_t5_attention_mfma(const void* qkv, int64_t row_stride, int64_t inner, const void* bias_f32, int64_t bias_ld, int64_t bias_center,
                           int64_t kv_len, void* kp, void* vt, void* out, int64_t out_stride, int64_t L, int64_t heads, void* stream);

/* ---- CLIP text encoders (the two CLIPTextModelWithProjection of Vchitect-2.0: transformers modeling_clip.py, third-party; call
 * site pipeline_vchitect.py:368).  Embedding, LayerNorm and the pooled-row gather are vsys_gather_rows / vsys_add_bcast_rows /
 * vsys_ln_modulate, the linears vsys_gemm_skinny_slices; neither entry point below has a VSYS_OP code (they run once per prompt). */
/* CLIPAttention (transformers modeling_clip.py, third-party; call site pipeline_vchitect.py:368), head dim 64, causal:
 * out_i = bf16(sum_{j <= i} w_j v_j), w_j = bf16(p_j / l) with p_j = exp(s_j - max_j s_j), s_j = (q_i . k_j) / 8 and l = sum_j p_j
 * all in fp32 (the division from the unrounded p_j: `softmax(..., dtype=float32).to(bf16)`).  qkv rows (b, l) of row_stride
 * elements, q | k | v at column 0 | inner | 2 inner, head h at h*64 (the layout of vsys_t5_attention); out bf16 [B*L, inner] with
 * out_stride.  One launch covers all B samples and inner / 64 heads; 1 <= L <= 128.  Strides % 8 == 0, pointers 16-byte aligned.
 * Rows at or past B*L and columns outside [0, 3 inner) are never read. */
int vsys_clip_attention_d64(const void* qkv, int64_t row_stride, int64_t inner, void* out, int64_t out_stride, int64_t B, int64_t L,
                            void* stream);
/* vsys_splitk_reduce for layers with a bias and an activation (nn.Linear + CLIPMLP.activation_fn inside transformers' CLIPEncoderLayer,
 * modeling_clip.py, third-party; call site pipeline_vchitect.py:368): y = bf16(((p_0 + p_1) + ...) + bias[n]) in fp32, slices in
 * ascending order, bias (bf16 [N], may be NULL) last; act 0: none, 1: quick_gelu = bf16(y * bf16(sigmoid(bf16(1.702 y)))),
 * 2: gelu = bf16(0.5 y (1 + erf(y / sqrt 2))) evaluated in fp32; then + res[m][n], added after the rounding and rounded again.
 * bias == NULL and act == 0 give the bits of vsys_splitk_reduce.  out may alias res. */
int vsys_splitk_reduce_bias_act(const void* part_f32, int64_t nsplit, int64_t slab, int64_t ldp, const void* res, int64_t ldr, void* out,
                                int64_t ldo, int64_t M, int64_t N, const void* bias, int64_t act, void* stream);

/* ---- VAE decode (VideoAutoencoderPipeline.decode, autoencoder_kl_open_sora.py:672-695) --------------
 * Activations are channels-last bf16 row matrices over a grid; a grid is described by int64 g[6] = {T, H, W, pad, tf,
 * sample_rows}: sample n, frame t, pixel (h, w) is row n*sample_rows + ((t + tf)*(H + 2 pad) + h + pad)*(W + 2 pad) + w + pad.
 * Borders (pad = 1) and front frames (tf) of conv INPUT buffers are zero and never written by these entry points. */

/* Implicit-GEMM convolution (replaces nn.Conv3d inside CausalConv3d, autoencoder_kl_open_sora.py:89-124, and the Conv2d /
 * Linear layers of the diffusers 0.30.0 AutoencoderKL decoder): out[r, n] = bias[n] + sum_{tap, c} a[r + delta(tap), c] *
 * w[n, tap*cin + c] (+ res[r, n] after rounding to bf16), tap = (a, b, c) in kt x kh x kw, delta = a*plane_pitch +
 * b*row_pitch + c rows.  `a` points at the row tap (0,0,0) reads for output row 0; rows up to M - 1 + delta(last tap) must
 * be readable.  kt*kh*kw == 1 is a plain GEMM with any K = cin (multiple of 32); otherwise cin/32 must be a power of two.
 * N % 128 == 0.  Exactly one of out (bf16) / out_f32 (fp32, scaled by out_scale, no bias/res) is non-NULL.  batch > 1
 * repeats the product with operand strides batch_a / batch_w / batch_o (elements). */
int vsys_conv_bf16(const void* a, int64_t lda, const void* w, int64_t ldw, const void* bias, const void* res, int64_t ldr,
                   void* out, void* out_f32, int64_t ldo, int64_t M, int64_t N, int64_t cin, int64_t kt, int64_t kh, int64_t kw,
                   int64_t row_pitch, int64_t plane_pitch, int64_t batch, int64_t batch_a, int64_t batch_w, int64_t batch_o,
                   float out_scale, void* stream);

/* nn.GroupNorm statistics over the interior of every sample (autoencoder_kl_open_sora.py:145,147,343; diffusers ResnetBlock2D
 * norm1/norm2): stats_f32[n][group] = (mean, 1/sqrt(var + eps)).  partial_f32 is scratch of N*nblk*(C/4)*2 floats. */
int vsys_gn_stats(const void* x, const int64_t* grid, int64_t N, int64_t C, int64_t groups, float eps, void* partial_f32,
                  int64_t nblk, void* stats_f32, void* stream);
/* y = act(bf16((x - mean) * rstd * gamma + beta)), act = VSYS_ACT_NONE | VSYS_ACT_SILU, interior rows of grid_dst only: the
 * GroupNorm (+ SiLU) of ResBlock.forward (autoencoder_kl_open_sora.py:152-164) / diffusers ResnetBlock2D with vsys_gn_stats. */
int vsys_gn_apply(const void* x, const int64_t* grid_src, void* y, const int64_t* grid_dst, int64_t N, int64_t C, int64_t groups,
                  const void* stats_f32, const void* gamma, const void* beta, int act, void* stream);
/* grid-to-grid copy of the interior; up = 1: nearest-neighbour 2x upsampling in H and W (diffusers Upsample2D before its conv).
 * tmode 0: same frame count; 1: destination frame t reads source frame t/2; 2: CogVideoXUpsample3D with an odd frame count
 * (modules/upsampling.py:42-49): 2T-1 frames, frame 0 stays single. */
int vsys_regrid(const void* x, const int64_t* grid_src, void* y, const int64_t* grid_dst, int64_t N, int64_t C, int64_t up,
                int64_t tmode, void* stream);
/* Strided pick, destination (t, h, w) = source (t * t_stride + t_first, h * s_stride + s_first, w * s_stride + s_first): the
 * strided convolutions of the VAE ENCODERS are their stride-1 convolution (vsys_conv_bf16) sampled — diffusers Downsample2D
 * (pad (0, 1, 0, 1) + 3 x 3 stride 2; third-party, called from autoencoder_kl_open_sora.py:503-520) at (2i + 1, 2j + 1) of the
 * pad-1 conv, the stride-(2, 1, 1) CausalConv3d of the temporal encoder (autoencoder_kl_open_sora.py:107-125,229-236) at frame
 * 2t + 1 of the two-front-frames conv. */
int vsys_subsample(const void* x, const int64_t* grid_src, void* y, const int64_t* grid_dst, int64_t N, int64_t C, int64_t t_stride,
                   int64_t s_stride, int64_t t_first, int64_t s_first, void* stream);
/* CogVideoXSpatialNorm3D + SiLU (autoencoder_kl_cogvideox.py:165-178,275-276): y = silu(GN(x) * Y + B); yb = [conv_y(zq) |
 * conv_b(zq)] computed at LATENT resolution, rows (n, zt, zh, zw) of 2C columns; the latent voxel of (t, h, w) follows
 * F.interpolate(zq, size=f.shape) including the first-frame split for odd frame counts.  stats from vsys_gn_stats. */
int vsys_spatial_norm_apply(const void* x, const int64_t* grid_src, void* y, const int64_t* grid_dst, int64_t N, int64_t C,
                            int64_t groups, const void* stats_f32, const void* gamma, const void* beta, const void* yb, int64_t zT,
                            int64_t zH, int64_t zW, void* stream);
/* tiled_decode's blend_v (axis 0) / blend_h (axis 1) (autoencoder_kl_cogvideox.py:1145-1159) on planar bf16 tiles
 * a [outer, Ha, Wa], b [outer, Hb, Wb], in place on b: the first ext rows (columns) of b fade in from the last ext of a. */
int vsys_blend_edge(const void* a, void* b, int64_t outer, int64_t Ha, int64_t Wa, int64_t Hb, int64_t Wb, int64_t ext, int64_t axis,
                    void* stream);
/* temporal depth-to-space "B (C ts) T H W -> B C (T ts) H W", ts = 2 (autoencoder_kl_open_sora.py:362-368): x has 2*Cout channels. */
int vsys_d2s_time(const void* x, const int64_t* grid_src, void* y, const int64_t* grid_dst, int64_t N, int64_t Cout, void* stream);
/* First decoder layer (VideoAutoencoderPipeline.decode z * scale + shift, autoencoder_kl_open_sora.py:676-677; post_quant_conv
 * + Decoder.conv1 :459,355-357; also the encoders' first convolutions with identity parameters): planar bf16 latent
 * z[4][F][H][W] -> z*scale + shift -> 1x1 post_quant_conv -> im2col rows
 * [F*H*W, kcols] (column = tap*4 + channel, zero padding; kt = 3: causal, two virtual zero frames in front).
 * params (HOST floats): scale[4], shift[4], pq_w[4][4], pq_b[4]. */
int vsys_vae_first_im2col(const void* z, int64_t F, int64_t H, int64_t W, int64_t kt, int64_t kcols, const float* params,
                          void* out, void* stream);
/* Last decoder layer: the first nc (<= 4) channels of rows [*, ldx] -> planar bf16 out[c][f0 + frame - tskip][h][w], frames
 * below tskip dropped (VAE_Temporal.decode's x[:, :, time_padding:], autoencoder_kl_open_sora.py:461). */
int vsys_extract_planar(const void* x, const int64_t* grid, int64_t N, int64_t ldx, int64_t nc, int64_t tskip, void* out,
                        int64_t Ftot, int64_t f0, void* stream);
/* First layer of the SD3 VAE decode of the Vchitect-2.0 pipeline (pipeline_vchitect.py:980-983: `latents / scaling_factor +
 * shift_factor` on the bf16 latents, then AutoencoderKL.decode -> Decoder.conv_in; the SD3 VAE has 16 latent channels and no
 * post_quant_conv): fp32 latents z[F][Cz][H][W] (1 <= Cz <= 32; `latents[0]` of the pipeline's [1, F, Cz, h, w] tensor as it is) ->
 * bf16 im2col rows [F*H*W, kcols] of the 3 x 3 conv (kcols % 32 == 0, kcols >= 9 Cz; column = tap * Cz + channel, tap = 3 dy + dx;
 * zero outside the image and from column 9 Cz on).  Value: bf16(bf16(bf16(z) / scaling_factor) + shift_factor), the division a
 * correctly rounded fp32 division.  No VSYS_OP code (the decode is not part of a recorded step). */
int vsys_vae_first_im2col_nc(const void* z_f32, int64_t F, int64_t Cz, int64_t H, int64_t W, int64_t kcols, float scaling_factor,
                             float shift_factor, void* out, void* stream);
/* Last layer of the same decode (pipeline_vchitect.py:984, VaeImageProcessor.postprocess(image, "pil") of diffusers): the first 3
 * channels of the interior rows [*, ldx] of a conv-output grid (grid descriptor and ldx as vsys_extract_planar; ldx % 4 == 0, x 8-byte
 * aligned) -> uint8 out[Ftot][H][W][3], frames f0 .. f0 + N*T - 1 (f0 + N*T <= Ftot).  Value: d = clamp(bf16(bf16(x / 2) + 0.5), 0, 1),
 * byte = round-half-even(float(d) * 255).  No VSYS_OP code. */
int vsys_pixels_to_u8(const void* x, const int64_t* grid, int64_t N, int64_t ldx, void* out_u8, int64_t Ftot, int64_t f0,
                      void* stream);
/* row softmax over the first n of ld columns, fp32 [rows, ld] -> bf16 [rows, ld] with zeros in columns n..ld-1 (mid-block
 * attention of the 2-D VAE — diffusers Attention under VideoAutoencoderKL.decode / .encode, autoencoder_kl_open_sora.py:503-538 —
 * keys padded to the 128-column tile; n % 4 == 0, ld % 4 == 0, ld <= 8192). */
int vsys_softmax_rows(const void* s_f32, void* p, int64_t rows, int64_t n, int64_t ld, void* stream);

/* Open-Sora-Plan v1.2 CausalVAE decode and sampler (csrc/vae_osp.hip).  None of the three has a VSYS_OP code: the decode is not part
 * of a recorded step, and the step kernel is launched by the host after each replay. */
/* Spatial2xTime2x3DUpsample.forward up to its conv (autoencoder_kl_open_sora_plan_v120.py:349-357): F.interpolate(mode="trilinear",
 * align_corners=False) of frame 0 by (1, 2, 2) and of frames 1..T-1 by (2, 2, 2) among themselves (source indices clamp at the ends
 * of THAT range), concatenated: grid_dst has T == 1 ? 1 : 2T - 1 frames of (2H, 2W).  x: bf16 channels-last rows over grid_src; y:
 * rows over grid_dst, interior rows written only (the causal conv that follows reads the padded grid as it is).  Per axis the weights
 * are 1/4 and 3/4 with edge clamping; the eight taps are accumulated in fp32 and rounded to bf16 once.  C % 8 == 0, C <= 2048,
 * x and y 16-byte aligned. */
int vsys_upsample_trilinear2x(const void* x, const int64_t* grid_src, void* y, const int64_t* grid_dst, int64_t N, int64_t C,
                              void* stream);
/* One sampler step of OpenSoraPlanPipeline (pipeline_open_sora_plan.py): the CFG combine and the drop of the learned-sigma half
 * (:1149-1156), EulerAncestralDiscreteScheduler.step (:1161) and the scale_model_input of the NEXT step (:1109-1110).  z fp32
 * [Bz, Cin, thw] in place; model_out fp32 [2 Bz, Cout, thw], Cout == 2 Cin, negative prompt first (uncond = model_out[b], cond =
 * model_out[b + Bz]); noise fp32 [Bz, Cin, thw], may be NULL when sigma_up == 0; model_in bf16 [2 Bz, Cin, thw].
 * z' = z + dt (u + guidance (c - u)) + sigma_up noise, evaluated in fp64 on the fp32 operands and rounded once;
 * model_in[b] = model_in[b + Bz] = bf16(z' * in_scale), in_scale = 1 / sqrt(sigma_next^2 + 1). */
int vsys_cfg_ancestral_step(void* z_f32, const void* model_out_f32, const void* noise_f32, void* model_in, int64_t Bz, int64_t Cin,
                            int64_t Cout, int64_t thw, float guidance, float dt, float sigma_up, float in_scale, void* stream);
/* OpenSoraPlanPipeline.decode_latents' post-process (pipeline_open_sora_plan.py:1186-1188) on the bf16 video: grid descriptor, ldx and
 * the uint8 layout out[Ftot][H][W][3] as vsys_pixels_to_u8.  Value, every tensor op of the reference rounding to bf16:
 * d = clamp(bf16(bf16(x / 2) + 0.5), 0, 1), m = bf16(d * 255), byte = trunc(m) (vsys_pixels_to_u8 rounds float(d) * 255 half-even). */
int vsys_pixels_to_u8_trunc(const void* x, const int64_t* grid, int64_t N, int64_t ldx, void* out_u8, int64_t Ftot, int64_t f0,
                            void* stream);

/* Open-Sora-Plan v1.1 CausalVAE decode and sampler (csrc/vae_osp.hip).  Neither has a VSYS_OP code, for the reasons above. */
/* TimeUpsample2x.forward (autoencoder_kl_open_sora_plan_v110.py:1549-1554) and TimeUpsampleRes2x.forward up to its conv (:1590-1596):
 * frame 0 is copied; frames 1..T-1 are F.interpolate(scale_factor=(2, 1, 1), mode="trilinear", align_corners=False) of source frames
 * 1..T-1 taken as a range of their own (weights 1/4 and 3/4, source indices clamped at both ends of THAT range), concatenated:
 * grid_dst has T == 1 ? 1 : 2T - 1 frames of the same (H, W).  x: bf16 channels-last rows over grid_src; y: rows over grid_dst,
 * interior rows written only (the destination is the padded input grid of the causal conv that follows).  v = w0 a + w1 b in fp32,
 * y = bf16(v): one rounding (a frame whose two taps coincide is a copy).  y_res (may be NULL, then grid_res and alpha are unused):
 * a second destination over its own descriptor grid_res with the frame count, H and W of grid_dst, interior rows only, receives
 * bf16(alpha * v) from the same fp32 v — the `alpha * x` term of TimeUpsampleRes2x, to be handed to vsys_conv_bf16 as `res` with the
 * conv's weights and bias scaled by (1 - alpha); alpha = sigmoid(mix_factor) is the host's.  C % 8 == 0, C <= 2048; x, y and y_res
 * 16-byte aligned and distinct buffers. */
int vsys_upsample_time2x(const void* x, const int64_t* grid_src, void* y, const int64_t* grid_dst, void* y_res, const int64_t* grid_res,
                         float alpha, int64_t N, int64_t C, void* stream);
/* One PNDMScheduler.step of the Open-Sora-Plan v1.1 pipeline (pipeline_open_sora_plan.py with `PNDMScheduler()`, :302-304; diffusers,
 * third-party) in ONE launch: the CFG combine and the drop of the learned-sigma half, the scheduler update as a linear form, and the
 * next call's model input.  e = u + guidance (c - u) on the first Cin of the Cout == 2 Cin channels of model_out fp32 [2 Bz, Cout, thw],
 * negative prompt first (u = model_out[b], c = model_out[b + Bz]).  With S = {e, src0, src1, src2, src3} (src: fp32 [Bz, Cin, thw]):
 *   e_out   (fp32 [Bz, Cin, thw], may be NULL) = e                                    the history slot
 *   z_out   (fp32 [Bz, Cin, thw])              = c_base base + sum_i cz[i] S[i]        the previous sample
 *   aux_out (fp32 [Bz, Cin, thw], may be NULL) = sum_i ca[i] S[i]                      the Runge-Kutta accumulator
 *   model_in[b] = model_in[b + Bz] (bf16 [2 Bz, Cin, thw]) = the same form in bf16      scale_model_input is the identity
 * coef: 12 doubles ON THE HOST, read during the call: {guidance, c_base, cz[0..4], ca[0..4]}.  Every form is evaluated in fp64 on the
 * fp32 operands and each stored value is rounded once from the fp64 value (e enters the sums unrounded; model_in is the fp64 value
 * rounded to bf16, not the fp32 z_out rounded again — the two differ in about one element in 2^16). A source or base whose weights are all zero is
 * never read and may be NULL (NaN there is harmless); a non-zero weight on a NULL operand is VSYS_ERR_ARG; ca is ignored when aux_out
 * is NULL.  Element i of an output depends on element i of the inputs only, so an output may be an input's buffer (base == z_out,
 * aux_out == a source); the outputs are distinct from each other and from model_out. */
int vsys_cfg_pndm_step(const void* model_out_f32, void* e_out_f32, const void* src0_f32, const void* src1_f32, const void* src2_f32,
                       const void* src3_f32, const void* base_f32, void* z_out_f32, void* aux_out_f32, void* model_in, int64_t Bz,
                       int64_t Cin, int64_t Cout, int64_t thw, const double* coef, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Launch programs.  A denoise step is ~450 launches of the entry points above with arguments that do not change from step to
 * step (workspaces, weights and PAB slabs are resident; per-step values live in device buffers).  The host mirror records the
 * sequence once per (geometry, PAB decision pattern, parallel layout) and replays it with ONE call: the loop below runs in C,
 * so the per-launch host cost is hipLaunchKernel alone — what matters when P-way sequence parallelism shrinks a rank's device
 * time per step P-fold while the launch count stays (the reference issues every op from Python every step,
 * open_sora_transformer_3d.py:608-613).  A command = an entry point (VSYS_OP_*), its integer / pointer arguments in declaration
 * order in a[], its float arguments in declaration order in f[], and the index of its stream in the table handed to
 * vsys_program_run.  Commands run in order; the first failing command stops the run, its index goes to *failed_at and its error
 * code is returned (nothing after it is enqueued).  No allocation, no synchronisation.  Host-side actions between launches
 * (collectives, event record / wait across streams) stay with the caller, which replays the program in segments. */
/* >>> VSYS_OP codes (generated: csrc/gen/program_gen.py) */
#define VSYS_OP_GEMM_BF16                    1
#define VSYS_OP_LINEAR_SMALL                 2
#define VSYS_OP_ADALN_MODULATE               3
#define VSYS_OP_MOD_TABLE                    4
#define VSYS_OP_TIMESTEP_EMBEDDING           5
#define VSYS_OP_PATCH_EMBED                  6
#define VSYS_OP_FINAL_LAYER                  7
#define VSYS_OP_CFG_EULER_STEP               8
#define VSYS_OP_ADD_ROWS                     9
#define VSYS_OP_COPY_4D_BATCH                10
#define VSYS_OP_ATTN_PREP_KV                 11
#define VSYS_OP_FLASH_ATTN_D72               12
#define VSYS_OP_ATTN_TEMPORAL_D72            13
#define VSYS_OP_ADD_BCAST_ROWS               14
#define VSYS_OP_GEMM_BF16_GATE2              15
#define VSYS_OP_LN_MODULATE                  16
#define VSYS_OP_GATE_ADD_ROWS                17
#define VSYS_OP_ATTN_PREP_KV64               18
#define VSYS_OP_FLASH_ATTN_D64               19
#define VSYS_OP_PATCH_EMBED_SHARD            20
#define VSYS_OP_FINAL_LAYER_TOKENS           21
#define VSYS_OP_UNPATCHIFY_TOKENS            22
#define VSYS_OP_GEMM_BF16_LN                 23
#define VSYS_OP_GEMM_BF16_STATS              24
#define VSYS_OP_ADALN_PRESCALE               25
#define VSYS_OP_LN_ROW_STATS                 26
#define VSYS_OP_GEMM_BF16_GATE_RES_ADD       27
#define VSYS_OP_FLASH_ATTN_D72_KB            28
#define VSYS_OP_FLASH_ATTN_D64_KB            29
#define VSYS_OP_FLASH_ATTN_D72_EXACT         30
#define VSYS_OP_P2P_EXCHANGE                 31
#define VSYS_OP_CFG_LINEAR_STEP              32
#define VSYS_OP_COPY_4D                      33
#define VSYS_OP_IM2COL_PATCH                 34
#define VSYS_OP_UNPATCHIFY_CVX               35
#define VSYS_OP_GATHER_ROWS                  36
#define VSYS_OP_RMS_NORM_ROWS                37
#define VSYS_OP_GEGLU                        38
#define VSYS_OP_SPLITK_REDUCE_T              39
#define VSYS_OP_T5_ATTENTION                 40
#define VSYS_OP_GEMM_SKINNY_SLICES           41
#define VSYS_OP_SPLITK_REDUCE                42
#define VSYS_OP_T5_ATTENTION_MFMA            43
#define VSYS_OP_CONV_BF16                    44
#define VSYS_OP_GN_STATS                     45
#define VSYS_OP_GN_APPLY                     46
#define VSYS_OP_REGRID                       47
#define VSYS_OP_SUBSAMPLE                    48
#define VSYS_OP_SPATIAL_NORM_APPLY           49
#define VSYS_OP_BLEND_EDGE                   50
#define VSYS_OP_D2S_TIME                     51
#define VSYS_OP_VAE_FIRST_IM2COL             52
#define VSYS_OP_EXTRACT_PLANAR               53
#define VSYS_OP_SOFTMAX_ROWS                 54
#define VSYS_OP_ATTN_PREP_KV_VARLEN          55
#define VSYS_OP_FLASH_ATTN_D72_VARLEN        56
#define VSYS_OP_GEMM_BF16_LN_QKV_KV          57
#define VSYS_OP_ATTN_TEMPORAL_D64            58
#define VSYS_OP_SCALE_ADD_ROWS               59
#define VSYS_OP_ATTN_PREP_KV96               60
#define VSYS_OP_FLASH_ATTN_D96               61
#define VSYS_OP_ATTN_PREP_KV96_IMG           62
#define VSYS_OP_FLASH_ATTN_D96_IMG           63
#define VSYS_OP_ATTN_PREP_KV_ROPE            64
#define VSYS_OP_FLASH_ATTN_D72_ROPE          65
#define VSYS_OP_CLIP_ATTENTION_D64           66
#define VSYS_OP_SPLITK_REDUCE_BIAS_ACT       67
#define VSYS_OP_VAE_FIRST_IM2COL_NC          68
#define VSYS_OP_PIXELS_TO_U8                 69
#define VSYS_OP_UPSAMPLE_TRILINEAR2X         70
#define VSYS_OP_CFG_ANCESTRAL_STEP           71
#define VSYS_OP_PIXELS_TO_U8_TRUNC           72
#define VSYS_OP_UPSAMPLE_TIME2X              73
#define VSYS_OP_CFG_PNDM_STEP                74
#define VSYS_OP_COUNT 75
/* <<< VSYS_OP codes */

#define VSYS_CMD_MAX_INT 24
#define VSYS_CMD_MAX_FLOAT 4
typedef struct vsys_cmd {
  int32_t op;      /* VSYS_OP_* */
  int32_t stream;  /* index into the streams[] table of vsys_program_run */
  int64_t a[VSYS_CMD_MAX_INT];   /* integer and pointer arguments, declaration order, the trailing stream excluded */
  float f[VSYS_CMD_MAX_FLOAT];      /* float arguments, declaration order */
} vsys_cmd;

/* arity of an op (what the recorder must fill): 0, or VSYS_ERR_ARG for an unknown op.  (vsys_program_*: no reference counterpart —
 * the reference issues every op from Python every step, open_sora_transformer_3d.py:608-613.) */
int vsys_program_op_info(int op, int* n_int, int* n_float);
int vsys_program_run(const vsys_cmd* cmds, int64_t n, void* const* streams, int64_t n_streams, int64_t* failed_at);

#ifdef __cplusplus
}
#endif
#endif /* VIDEOSYS_AMD_H */
