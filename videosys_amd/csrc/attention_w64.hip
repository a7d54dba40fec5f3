// flash_attn_d72_w64: spatial self-attention of STDiT3 (head_dim 72) with 64 query rows per wave and ONE wave per SIMD.
//
// Replaces (/root/reference/videosys): OpenSoraAttention.forward q/k LlamaRMSNorm + SDPA (modules/attentions.py:75,80-120;
// normalization.py:28-33) — the same contract, layouts (attn_prep_kv's Kp / Vt) and arithmetic as flash_attn_d72_kernel
// (attention.hip), for long unmasked-or-ragged key sequences (>= 4 tiles of 64 keys).
//
// Why a second kernel: at 32 query rows per wave the tile loop is bound by per-wave issue and dependent latency (DESIGN.md
// §3.2); 64 rows per wave halve the K / Vt fragment reads and the staged bytes per MFMA, but need ~400 live registers, which
// hipcc answers with accumulator-file shuffling.  Here the whole tile loop is ONE asm statement with a hand-made register
// allocation and instruction placement (csrc/gen/flash72_gen.py -> flash72_w64_asm.inc): O, Q and the K / Vt fragments live in
// a[0:223], S / P / the running max in v[0:209]; the C++ around it only computes addresses and the Q fragments (prologue) and
// normalises / stores O (epilogue).  The statement lists every register it owns as a clobber; nothing else in this kernel uses
// the accumulator file (tests/test_build_resources.py: no accumulator-file move outside the asm statements, no scratch).
//
// The register map (Q into / O out of the accumulator file, the statements' operand names) comes from the generator with the
// streams: FLASH72_W64_WRITE_Q_*, _READ_O_* and FLASH72_W64[P]_OPERANDS[_S] in flash72_w64_map.inc.  The variables a statement
// reads carry its operand names (the operand lists bind by name).  Descriptors, fragment addressing, the row bound and the launch
// are flash_w64.h, shared with attention64_w64.hip.  The LDS-DMA lane addressing, the RMS-norm Q fragments and the O store stand
// in each kernel: as shared inline functions they did not compile to the instruction stream they have here (flash_w64.h).
#include "flash_w64.h"

namespace vsys {
namespace {

using w64::VROW;
using w64::make_rsrc;
using w64::u32x4;
constexpr int HD = 72, HD_ROWS = 96, KROW = 144;
constexpr int K_TILE_BYTES = 64 * KROW;                   // 9216
constexpr int KV_STAGE = K_TILE_BYTES + HD_ROWS * VROW;   // 21504
constexpr int W64_STAGES = w64::STAGES;

struct FlashW64Params {
  const bf16_t* q; int64_t q_stride;
  const bf16_t* q_norm_w;
  const bf16_t* kp;
  const bf16_t* vt;
  bf16_t* out; int64_t out_stride;
  int heads, q_len, kv_len, kv_pad, nqb;
  float eps;
  // VAR 5 / the _S persistent statement: an upper bound on the Euclidean norm of every Kp row of this launch (as stored: normed and
  // scaled into the exp2 domain).  -|q_i| k_bound (1 + 2^-6) replaces the running max of query row i; the caller guarantees
  // |q_i| k_bound <= 60 for every row (2 m < 126: no term of a row can underflow to zero while its sum is still representable).
  float k_bound;
  unsigned long long* dbg;   // lab variant 7: per wave 8 s_memtime stamps
};

// VAR: placement variant of the LDS-DMA pieces inside the tile loop (flash72_gen.py body()); same arithmetic, same bits
template <int VAR>
__global__ __launch_bounds__(256, 1) void flash_attn_d72_w64_kernel(FlashW64Params p) {
#if __HIP_DEVICE_COMPILE__
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  unsigned long long stamp[6] = {0, 0, 0, 0, 0, 0};
  if constexpr (VAR == 7) stamp[0] = __builtin_amdgcn_s_memtime();
  const int tile_id = xcd_remap(blockIdx.x, gridDim.x);   // the q-blocks of one (batch, head) are consecutive on one XCD
  const int bh = tile_id / p.nqb, qb = tile_id - bh * p.nqb;
  const int b = bh / p.heads, h = bh - b * p.heads;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int q0 = qb * 256 + wave_u * 64;

  // ---- LDS-DMA assignment (as flash_attn_d72_kernel): 9 K pieces + 10 Vt pieces per tile; wave w issues K pieces w, w + 4, Vt
  // pieces w, w + 4, and one of {K piece 8, Vt piece 8, Vt piece 9, Vt piece 9 again}
  const bf16_t* kbase = p.kp + (int64_t)bh * p.kv_pad * HD;
  const bf16_t* vbase = p.vt + (int64_t)bh * HD_ROWS * p.kv_pad;
  const unsigned kbytes = (unsigned)(p.kv_pad * HD * 2), vbytes = (unsigned)(HD_ROWS * p.kv_pad * 2);
  const u32x4 rk = make_rsrc(kbase, kbytes), rv = make_rsrc(vbase, vbytes);
  const bool s4k = wave_u == 0;
  const int s4j = wave_u == 1 ? 8 : 9;
  const u32x4 r4 = make_rsrc(s4k ? (const void*)kbase : (const void*)vbase, s4k ? kbytes : vbytes);
  const int kvo = lane * 16;
  const int v_voff0 = (lane >> 3) * p.kv_pad * 2 + (((lane & 7) ^ (lane >> 4)) << 4);
  const int vvo = v_voff0 ^ ((wave_u & 1) << 6);
  const int v4o = s4k ? kvo : (v_voff0 ^ ((s4j & 1) << 6));
  const int wl = wave_u * 1024;
  const int sv0 = wave_u * 8 * p.kv_pad * 2, sv1 = (wave_u + 4) * 8 * p.kv_pad * 2;
  const int s4 = s4k ? 8 * 1024 : s4j * 8 * p.kv_pad * 2, st4 = s4k ? K_TILE_BYTES : 128;
  const int l4 = s4k ? 8 * 1024 : K_TILE_BYTES + s4j * 1024;
  const int lb = w64::lds_base(smem);   // LDS address of the ring
  const int nt = (p.kv_len + 63) >> 6;
  const int lim = p.kv_len - (nt - 1) * 64 - 16 * hi;

  // rows 80..95 of every stage's Vt image: MFMA padding the DMA never writes
  for (int u = tid; u < W64_STAGES * 128; u += 256)
    *reinterpret_cast<uint4*>(smem + (u >> 7) * KV_STAGE + K_TILE_BYTES + 80 * VROW + (u & 127) * 16) = make_uint4(0, 0, 0, 0);

  // ---- fragment read offsets inside a stage
  const int kfa = w64::frag_krow(l31) * KROW + 16 * hi;
  const w64::VtFrag vf = w64::vt_frag<K_TILE_BYTES>(l31, hi);
  const int vfa0 = vf.vfa0, vfa1 = vf.vfa1, vfa2 = vf.vfa2, vfa3 = vf.vfa3;

  // ---- Q fragments of the two 32-row blocks (B operand: lane holds Q[row][16c + 8hi .. +8], c = 0..4, d >= 72 -> 0), RMS-normed
  uint4 qw[2][5];
  float nmv[2] = {0.f, 0.f};   // VAR 5: -(row bound) of this lane's query row in block A / B
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    int qs = q0 + 32 * blk + l31;
    qs = qs < p.q_len ? qs : p.q_len - 1;
    const bf16_t* qrow = p.q + ((int64_t)b * p.q_len + qs) * p.q_stride + h * HD;
    uint4 qraw[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const int d0 = 16 * c + 8 * hi;
      qraw[c] = d0 < HD ? *reinterpret_cast<const uint4*>(qrow + d0) : make_uint4(0, 0, 0, 0);
    }
    float x[5][8];
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      unpack8(qraw[c], x[c]);
#pragma unroll
      for (int e = 0; e < 8; ++e) ss += x[c][e] * x[c][e];
    }
    if (p.q_norm_w != nullptr) {
      ss += __shfl_xor(ss, 32, 64);
      const float rstd = rsqrtf(ss / (float)HD + p.eps);
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        const int d0 = 16 * c + 8 * hi;
        if (d0 < HD) {
          float w[8];
          unpack8(*reinterpret_cast<const uint4*>(p.q_norm_w + d0), w);
#pragma unroll
          for (int e = 0; e < 8; ++e) x[c][e] = bf2f(f2bf(x[c][e] * rstd)) * w[e];
        }
      }
    }
    if constexpr (VAR == 5) nmv[blk] = w64::neg_row_bound<5>(x, p.k_bound);
#pragma unroll
    for (int c = 0; c < 5; ++c) qw[blk][c] = pack8(x[c]);
  }
  FLASH72_W64_WRITE_Q_A(qw[0]);
  FLASH72_W64_WRITE_Q_B(qw[1]);
  const float nma = nmv[0], nmb = nmv[1];

  // ---- the tile loop
#define W64_LOOP(TEXT_) asm volatile(TEXT_ : : FLASH72_W64_OPERANDS : FLASH72_W64_CLOBBERS)
#define W64_STAMPS [t0] "=s"(stamp[1]), [t1] "=s"(stamp[2]), [t2] "=s"(stamp[3])
  if constexpr (VAR == 0) W64_LOOP(FLASH72_W64_ASM_V0);
  else if constexpr (VAR == 5)   // no running max: the row bounds ride in as the -m splat
    asm volatile(FLASH72_W64_ASM_V5 : : FLASH72_W64_OPERANDS_S : FLASH72_W64_CLOBBERS);
  else if constexpr (VAR == 1) W64_LOOP(FLASH72_W64_ASM_V1);
  else if constexpr (VAR == 3) W64_LOOP(FLASH72_W64_ASM_V3);
#ifdef VSYS_LAB
  else if constexpr (VAR == 7) {
    asm volatile(FLASH72_W64_ASM_V7 : W64_STAMPS : FLASH72_W64_OPERANDS : FLASH72_W64_CLOBBERS);
    stamp[4] = __builtin_amdgcn_s_memtime();
  }
  else if constexpr (VAR == 10)   // per-phase cycle sums of the loop tiles: X, wait + barrier, Y
    asm volatile(FLASH72_W64_ASM_V10 : W64_STAMPS : FLASH72_W64_OPERANDS : FLASH72_W64_CLOBBERS_PHASE);
  else if constexpr (VAR == 8) W64_LOOP(FLASH72_W64_ASM_V8);
  else if constexpr (VAR == 9) W64_LOOP(FLASH72_W64_ASM_V9);
#endif
#undef W64_STAMPS
#undef W64_LOOP

  // ---- epilogue: O[q][d] = O^T[d][q] / l ; lane holds d = 32dt + (r&3) + 8(r>>2) + 4hi; 16-byte stores through
  // v_permlane32_swap (as flash_attn_d72_kernel::store_o)
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    float o[3][16];
    if (blk == 0) FLASH72_W64_READ_O_A(o);
    else FLASH72_W64_READ_O_B(o);
    const float inv = 1.0f / o[2][4];   // d = 72 (hi = 0) / 76 (hi = 1): the ones rows of Vt, i.e. sum_k P[k][q]
    const int qs = q0 + 32 * blk + l31;
    bf16_t* orow = p.out + ((int64_t)b * p.q_len + (qs < p.q_len ? qs : p.q_len - 1)) * p.out_stride + h * HD + 8 * hi;
#pragma unroll
    for (int dt = 0; dt < 3; ++dt) {
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
        const int d0 = dt * 32 + 16 * k;
        if (qs < p.q_len && d0 + 8 * hi + 8 <= HD) *reinterpret_cast<uint4*>(orow + d0) = make_uint4(sx[0], sy[0], sx[1], sy[1]);
      }
    }
  }
  if constexpr (VAR == 7 || VAR == 10) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the stores have left
    stamp[5] = __builtin_amdgcn_s_memtime();
    if (lane == 0 && p.dbg != nullptr) {
      unsigned long long* d = p.dbg + ((size_t)blockIdx.x * 4 + wave) * 8;
#pragma unroll
      for (int i = 0; i < 6; ++i) d[i] = stamp[i];
    }
  }
#endif
}

// ---------------------------------------------------------------------------------------------------------------------------
// Persistent form: gridDim.x workgroups (one per CU) walk the (batch, head, 256-row query block) items with stride gridDim.x.
// What an item pays at its seams in the one-item-per-workgroup kernel above (stamps, profiles/r04_flash_w64_stamps_nonpersistent.json:
// 11k cycles of Q fetch + norm, 4.3k of LDS-DMA issue + landing + pipeline fill, 3.5k of output stores against 27k in the tile loop,
// none of it covered at one workgroup per CU) is taken out of the seam where it can be: the tail of an item's tile loop already
// fetches the NEXT item's first four K / Vt tiles and its Q rows (LDS-DMA into a wave-private [chunk][row] image), so an item
// starts with everything on chip.  Any tile count >= 4: the ring continues from item to item (tile 0 of the k-th item of a workgroup
// sits in stage (k ntiles) mod 4); whole tiles of real keys only (kv_len % 64 == 0: nothing is masked).
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int W64P_QIMG = 64 * KROW;   // 9216 bytes per wave: 9 chunks x 64 rows x 16 B

__device__ __forceinline__ unsigned long long uniform_addr(const void* ptr) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(ptr);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi_ = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32) & 0xffffu);
  return ((unsigned long long)hi_ << 32) | lo;
}

// STAMP (lab): per wave the s_memtime cycles of an item's phases, summed over the items it walked, into p.dbg[wave][8]
// SM: the statement without the running max (FlashW64Params::k_bound)
template <bool STAMP, bool SM = false>
__global__ __launch_bounds__(256, 1) void flash_attn_d72_w64p_kernel(FlashW64Params p, int total_items) {
#if __HIP_DEVICE_COMPILE__
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  // Round j of the walk is items j G .. j G + G - 1, workgroup wgp takes item j G + wgp: the workgroups of one XCD (consecutive wgp) are
  // then on consecutive query blocks of the same one or two (batch, head) at any moment and share their K / Vt in that XCD's L2.
  // (Contiguous item RANGES per workgroup put every workgroup on its own head: 180 MB of K / Vt in flight, every tile from the
  // fabric, tile loop 34.0k cycles per item instead of 27.1k — profiles/r04_flash_w64p_stamps_ranges.json.)
  const int wgp = xcd_remap(blockIdx.x, gridDim.x), istep = (int)gridDim.x;
  const int i0 = wgp, i1 = total_items;
  if (i0 >= i1) return;

  const unsigned kbytes = (unsigned)(p.kv_pad * HD * 2), vbytes = (unsigned)(HD_ROWS * p.kv_pad * 2);
  const bool s4k = wave_u == 0;
  const int s4j = wave_u == 1 ? 8 : 9;
  const int kvo = lane * 16;
  const int v_voff0 = (lane >> 3) * p.kv_pad * 2 + (((lane & 7) ^ (lane >> 4)) << 4);
  const int vvo = v_voff0 ^ ((wave_u & 1) << 6);
  const int v4o = s4k ? kvo : (v_voff0 ^ ((s4j & 1) << 6));
  const int wl = wave_u * 1024, kvp2 = p.kv_pad * 2;
  const int s4 = s4k ? 8 * 1024 : s4j * 8 * p.kv_pad * 2, st4 = s4k ? K_TILE_BYTES : 128;
  const int l4 = s4k ? 8 * 1024 : K_TILE_BYTES + s4j * 1024;
  const int lb = w64::lds_base(smem);
  const int qlds = lb + W64_STAGES * KV_STAGE + wave_u * W64P_QIMG;
  const int nt = p.kv_len >> 6;   // whole tiles (flash_w64p_supports)
  for (int u = tid; u < W64_STAGES * 128; u += 256)
    *reinterpret_cast<uint4*>(smem + (u >> 7) * KV_STAGE + K_TILE_BYTES + 80 * VROW + (u & 127) * 16) = make_uint4(0, 0, 0, 0);
  const int kfa = w64::frag_krow(l31) * KROW + 16 * hi;
  const w64::VtFrag vf = w64::vt_frag<K_TILE_BYTES>(l31, hi);
  const int vfa0 = vf.vfa0, vfa1 = vf.vfa1, vfa2 = vf.vfa2, vfa3 = vf.vfa3;

  // what an item needs from the outside: K / Vt of its (batch, head), its Q rows (descriptor over the batch's rows of head h + the
  // lane's row offset), its output rows
  auto item_bh = [&](int it) { return it / p.nqb; };
  auto q_rsrc = [&](int it) {
    const int bh = item_bh(it), b = bh / p.heads, h = bh - b * p.heads;
    return make_rsrc(p.q + (int64_t)b * p.q_len * p.q_stride + h * HD, (unsigned)((int64_t)p.q_len * p.q_stride * 2));
  };
  auto q_row_voff = [&](int it) {   // this lane's row of the wave's 64 (clamped at the end of the sequence)
    const int qb = it - item_bh(it) * p.nqb;
    int r = qb * 256 + wave * 64 + lane;
    r = r < p.q_len ? r : p.q_len - 1;
    return r * (int)p.q_stride * 2;
  };
  typedef __attribute__((address_space(3))) void* lds_ptr_t;

  // ---- entry: Q rows and the first four tiles of the first item
  {
    const int bh = item_bh(i0);
    const bf16_t* kbase = p.kp + (int64_t)bh * p.kv_pad * HD;
    const bf16_t* vbase = p.vt + (int64_t)bh * HD_ROWS * p.kv_pad;
    const auto rk = __builtin_amdgcn_make_buffer_rsrc((void*)kbase, 0, (int)kbytes, 0x00020000);
    const auto rv = __builtin_amdgcn_make_buffer_rsrc((void*)vbase, 0, (int)vbytes, 0x00020000);
    const int bq = bh / p.heads, hq = bh - bq * p.heads;
    const auto rq = __builtin_amdgcn_make_buffer_rsrc((void*)(p.q + (int64_t)bq * p.q_len * p.q_stride + hq * HD), 0,
                                                      (int)((int64_t)p.q_len * p.q_stride * 2), 0x00020000);
    const int qv = q_row_voff(i0);
#pragma unroll
    for (int pc = 0; pc < 9; ++pc)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rq, (lds_ptr_t)(smem + W64_STAGES * KV_STAGE + wave_u * W64P_QIMG + pc * 1024), 16, qv, pc * 16, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      char* st = smem + t * KV_STAGE;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (lds_ptr_t)(st + wl), 16, kvo, t * K_TILE_BYTES + wl, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (lds_ptr_t)(st + wl + 4096), 16, kvo, t * K_TILE_BYTES + wl + 4096, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (lds_ptr_t)(st + K_TILE_BYTES + wl), 16, vvo, wave_u * 8 * kvp2 + t * 128, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (lds_ptr_t)(st + K_TILE_BYTES + wl + 4096), 16, vvo, (wave_u + 4) * 8 * kvp2 + t * 128, 0, 0);
      if (s4k) __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (lds_ptr_t)(st + l4), 16, v4o, s4 + t * st4, 0, 0);
      else __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (lds_ptr_t)(st + l4), 16, v4o, s4 + t * st4, 0, 0);
    }
  }

  // the RMS-norm weights of this lane's five column chunks, held packed across the items (registers above the statement's clobbers):
  // read per item they were five global round trips behind the item's opening vmcnt(0)
  uint4 qnw[5];
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    const int d0 = 16 * c + 8 * hi;
    qnw[c] = (p.q_norm_w != nullptr && d0 < HD) ? *reinterpret_cast<const uint4*>(p.q_norm_w + d0) : make_uint4(0, 0, 0, 0);
  }
  unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ta = 0, tb = 0;
  int ring = 0;   // stage of this item's tile 0: the ring continues from item to item, (items walked x ntiles) mod 4
  for (int it = i0; it < i1; it += istep) {
    const int bh = item_bh(it), qb = it - bh * p.nqb;
    const int b = bh / p.heads, h = bh - b * p.heads;
    const int q0 = qb * 256 + wave_u * 64;
    unsigned long long t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
    if constexpr (STAMP) t0 = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's Q image has landed (nobody else touches it)
    if constexpr (STAMP) t1 = __builtin_amdgcn_s_memtime();
    // ---- Q fragments from the image [chunk][row]: lane holds Q[row][16c + 8hi .. +8] = chunk 2c + hi of row 32 blk + l31
    uint4 qw[2][5];
    float nmv[2] = {0.f, 0.f};
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const char* qimg = smem + W64_STAGES * KV_STAGE + wave_u * W64P_QIMG + (32 * blk + l31) * 16;
      uint4 qraw[5];
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        const int ch = 2 * c + hi;
        qraw[c] = ch < 9 ? *reinterpret_cast<const uint4*>(qimg + ch * 1024) : make_uint4(0, 0, 0, 0);
      }
      float x[5][8];
      float ss = 0.f;
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        unpack8(qraw[c], x[c]);
#pragma unroll
        for (int e = 0; e < 8; ++e) ss += x[c][e] * x[c][e];
      }
      if (p.q_norm_w != nullptr) {
        ss += __shfl_xor(ss, 32, 64);
        const float rstd = rsqrtf(ss / (float)HD + p.eps);
#pragma unroll
        for (int c = 0; c < 5; ++c) {
          const int d0 = 16 * c + 8 * hi;
          if (d0 < HD) {
            float w[8];
            unpack8(qnw[c], w);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[c][e] = bf2f(f2bf(x[c][e] * rstd)) * w[e];
          }
        }
      }
      if constexpr (SM) nmv[blk] = w64::neg_row_bound<5>(x, p.k_bound);
#pragma unroll
      for (int c = 0; c < 5; ++c) qw[blk][c] = pack8(x[c]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the image reads are done before the tile loop overwrites it with the next item's rows
    FLASH72_W64_WRITE_Q_A(qw[0]);
    FLASH72_W64_WRITE_Q_B(qw[1]);
    const float nma = nmv[0], nmb = nmv[1];

    // ---- this item's K / Vt, and what the tail of the loop prefetches for the next one
    const bool has_next = it + istep < i1;
    const int nit = has_next ? it + istep : it;
    const int nbh = item_bh(nit);
    const unsigned long long kb = uniform_addr(p.kp + (int64_t)bh * p.kv_pad * HD), vb = uniform_addr(p.vt + (int64_t)bh * HD_ROWS * p.kv_pad);
    const unsigned long long kbn = uniform_addr(p.kp + (int64_t)nbh * p.kv_pad * HD), vbn = uniform_addr(p.vt + (int64_t)nbh * HD_ROWS * p.kv_pad);
    const u32x4 rqn = q_rsrc(nit);
    const int qvo = q_row_voff(nit);
    const int hn = __builtin_amdgcn_readfirstlane(has_next ? 1 : 0);
    const int st0 = lb + ring * KV_STAGE, st1 = lb + ((ring + 1) & 3) * KV_STAGE, st2 = lb + ((ring + 2) & 3) * KV_STAGE;
    ring = (ring + nt) & 3;
    if constexpr (STAMP) {
      t2 = __builtin_amdgcn_s_memtime();
#ifdef VSYS_LAB
      asm volatile(FLASH72_W64P_ASM_STAMP : [t0] "=s"(ta), [t1] "=s"(tb) : FLASH72_W64P_OPERANDS : FLASH72_W64_CLOBBERS);
#endif
      t3 = __builtin_amdgcn_s_memtime();
    } else if constexpr (SM)
      asm volatile(FLASH72_W64P_ASM_S : : FLASH72_W64P_OPERANDS_S : FLASH72_W64_CLOBBERS);
    else
      asm volatile(FLASH72_W64P_ASM : : FLASH72_W64P_OPERANDS : FLASH72_W64_CLOBBERS);

    // ---- epilogue (as the one-item kernel)
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      float o[3][16];
      if (blk == 0) FLASH72_W64_READ_O_A(o);
      else FLASH72_W64_READ_O_B(o);
      const float inv = 1.0f / o[2][4];   // d = 72 (hi = 0) / 76 (hi = 1): the ones rows of Vt, i.e. sum_k P[k][q]
      const int qs = q0 + 32 * blk + l31;
      bf16_t* orow = p.out + ((int64_t)b * p.q_len + (qs < p.q_len ? qs : p.q_len - 1)) * p.out_stride + h * HD + 8 * hi;
#pragma unroll
      for (int dt = 0; dt < 3; ++dt) {
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
          const int d0 = dt * 32 + 16 * k;
          if (qs < p.q_len && d0 + 8 * hi + 8 <= HD) *reinterpret_cast<uint4*>(orow + d0) = make_uint4(sx[0], sy[0], sx[1], sy[1]);
        }
      }
    }
    if constexpr (STAMP) {
      t4 = __builtin_amdgcn_s_memtime();
      acc[0] += t1 - t0;   // wait for the Q image (and whatever else is in flight)
      acc[1] += t2 - t1;   // Q fragments: LDS reads, RMS norm, accumulator-file writes, next item's descriptors
      acc[2] += ta - t2;   // the statement's opening wait + barrier (output stores of the previous item, tiles 0..3)
      acc[3] += tb - ta;   // O / -m init, descriptors, K(0), S(0), adopt
      acc[4] += t3 - tb;   // tile loop
      acc[5] += t4 - t3;   // O read-out, normalise, stores issued
      acc[6] += 1;
    }
  }
  if constexpr (STAMP) {
    if (lane == 0 && p.dbg != nullptr) {
      unsigned long long* d = p.dbg + ((size_t)blockIdx.x * 4 + wave) * 8;
#pragma unroll
      for (int i = 0; i < 7; ++i) d[i] = acc[i];
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (zero-length pieces of the last item's tail: nothing may be in flight when the LDS is released)
#endif
}

}  // namespace

// true when the w64 kernel takes the problem (launch_flash_attn_d72 falls back to flash_attn_d72_kernel otherwise)
bool flash_w64_supports(int q_len, int kv_len, int kv_pad) {
  (void)kv_pad;
  return kv_len >= 256 && q_len >= 256;   // >= 4 tiles of 64 keys, at least one full 256-row workgroup
}

// what both launchers hand to their kernels (dbg: the lab stamp buffer, or null)
static FlashW64Params w64_params(const bf16_t* q, int64_t q_stride, const bf16_t* q_norm_w, const bf16_t* kp, const bf16_t* vt, bf16_t* out,
                                 int64_t out_stride, int heads, int q_len, int kv_len, int kv_pad, float eps, float k_bound,
                                 unsigned long long* dbg) {
  FlashW64Params p;
  p.q = q; p.q_stride = q_stride; p.q_norm_w = q_norm_w; p.kp = kp; p.vt = vt; p.out = out; p.out_stride = out_stride;
  p.heads = heads; p.q_len = q_len; p.kv_len = kv_len; p.kv_pad = kv_pad; p.eps = eps; p.k_bound = k_bound;
  p.dbg = dbg;
  p.nqb = (q_len + 255) / 256;
  return p;
}

// persistent form: >= 4 tiles of tile-padded keys, 32-bit Q row offsets
bool flash_w64p_supports(int q_len, int kv_len, int kv_pad, int64_t q_stride) {
  // Any tile count >= 4, but WHOLE tiles of real keys only: the walk does not mask, and the keys behind kv_len inside a buffer are not
  // necessarily zero (a caller may pass a key count shorter than what the buffers were prepared for: Latte's per-sample text lengths).
  return kv_len >= 256 && kv_len % 64 == 0 && q_len >= 256 && (int64_t)q_len * q_stride * 2 < 0x7fffffff;
}

int launch_flash_attn_d72_w64p(const bf16_t* q, int64_t q_stride, const bf16_t* q_norm_w, const bf16_t* kp, const bf16_t* vt, bf16_t* out,
                               int64_t out_stride, int batch, int heads, int q_len, int kv_len, int kv_pad, float eps, bool stamp,
                               float k_bound, hipStream_t stream) {
  FlashW64Params p = w64_params(q, q_stride, q_norm_w, kp, vt, out, out_stride, heads, q_len, kv_len, kv_pad, eps, k_bound, nullptr);
  const int64_t total = (int64_t)p.nqb * batch * heads;
  if (total > 0x7fffffff) return VSYS_ERR_SHAPE;
  const int ncu = cu_count_this_device();
  const unsigned grid = (unsigned)(total < ncu ? total : ncu);
  const size_t lds = (size_t)W64_STAGES * KV_STAGE + 4 * W64P_QIMG;
  // (the three forms are named in the order they have always been instantiated in — plain, SM, STAMP: the labels inside the
  // statements carry the number of the function they are expanded in)
  (void)stamp;
#ifdef VSYS_LAB
  if (!stamp)
#endif
    return !(k_bound > 0.f && q_norm_w != nullptr) ? w64::launch<flash_attn_d72_w64p_kernel<false>>(grid, lds, stream, p, (int)total)
                                                    : w64::launch<flash_attn_d72_w64p_kernel<false, true>>(grid, lds, stream, p, (int)total);
#ifdef VSYS_LAB
  p.dbg = reinterpret_cast<unsigned long long*>(get_lab_debug_buffer());
  return w64::launch<flash_attn_d72_w64p_kernel<true>>(grid, lds, stream, p, (int)total);
#endif
}

int launch_flash_attn_d72_w64(const bf16_t* q, int64_t q_stride, const bf16_t* q_norm_w, const bf16_t* kp, const bf16_t* vt, bf16_t* out,
                              int64_t out_stride, int batch, int heads, int q_len, int kv_len, int kv_pad, float eps, int var,
                              float k_bound, hipStream_t stream) {
  const FlashW64Params p = w64_params(q, q_stride, q_norm_w, kp, vt, out, out_stride, heads, q_len, kv_len, kv_pad, eps, k_bound,
                                      reinterpret_cast<unsigned long long*>(get_lab_debug_buffer()));
  const int64_t nblk = (int64_t)p.nqb * batch * heads;
  if (nblk > 0x7fffffff) return VSYS_ERR_SHAPE;
  const size_t lds = (size_t)W64_STAGES * KV_STAGE;
#define W64_CASE(VAR_) w64::launch<flash_attn_d72_w64_kernel<VAR_>>((unsigned)nblk, lds, stream, p)
  switch (var) {
    case 0: return W64_CASE(0);
    case 1: return W64_CASE(1);
    case 3: return W64_CASE(3);
    case 5: return k_bound > 0.f && q_norm_w != nullptr ? W64_CASE(5) : VSYS_ERR_ARG;
#ifdef VSYS_LAB
    case 7: return W64_CASE(7);
    case 10: return W64_CASE(10);
    case 8: return W64_CASE(8);
    case 9: return W64_CASE(9);
#endif
    default: return VSYS_ERR_ARG;
  }
#undef W64_CASE
}

}  // namespace vsys
