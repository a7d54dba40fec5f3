// attn_temporal_d72_long: temporal self-attention at head dim 72 for EVERY T >= 65 frames (Open-Sora's 16 s preset is T = 120; the
// round-1 VALU kernel that served T > 64 keeps K and V of a head in LDS as fp32, 2 T 72 4 bytes per wave, and refuses T >= 285).
// Same contract as vsys_attn_temporal_d72 (attention.hip / attention_t3.hip) up to the softmax: a block loop with a running maximum.
//
// Work split.  One workgroup = 4 waves = one UNIT (b, s, group of four heads, block of 32 query frames); wave w owns head 4 hg + w
// (a last partial group keeps its spare waves for the data movement and the barriers only).  The unit walks the ceil(T / 32) key
// blocks; per (query block, key block) pair and head
//   S^T = K Q^T     5 x v_mfma_f32_32x32x16_bf16  (d = 72 -> 80; A = K rows in the permuted key order of attention_t3.hip: the 16
//                                                  accumulators of a lane are keys 8hi..8hi+7 and 16+8hi..16+8hi+7 of ITS query)
//   online softmax  exp2 domain, fp32 running max m and sum l per query row; P rounded to bf16 (unnormalised, <= 1), l summed from
//                   the unrounded P; the rescale of O by 2^(m - m') is skipped when no row of the wave moved its maximum
//   O^T += V^T P^T  6 x v_mfma_f32_32x32x16_bf16  (96 output dims x 2 chunks of 16 keys; P never leaves its lane)
// and O / l is rounded ONCE at the end of the unit.  (The <= 64 kernels round the normalised weights of all keys at once; that
// contract cannot hold for unbounded T.  ops.attn_temporal states both.)
//
// Data movement: row-contiguous, as attn_temporal_d72_v5.  Per frame the q, k and v bytes of four heads are 576 contiguous bytes; a
// block's 32 rows of one operand come in by LDS-DMA (buffer_load_dwordx4 ... lds) as a lane-linear image with a 592-byte row pitch
// (36 pieces + 1 pad: conflict-free 16-byte fragment reads), 20 wave instructions = 5 per wave.  The compact [32][36] cos / sin rows
// of the block come the same way with dword LDS-DMA (lane e fetches table element 2 e of its row: the reference's table holds every
// value twice), 9 per wave: nothing of a block passes through registers.  V(kb), K(kb + 1) and the next table rows are issued as
// soon as every wave holds its K fragments and travel under QK^T and the softmax of the pair.  (Issuing V(kb) one phase earlier and
// waiting with s_waitcnt vmcnt(14) for it alone was built first: hipcc puts its own s_waitcnt vmcnt(0) in front of the first LDS
// read behind any LDS-DMA, so the transfer was waited for where it was issued.  With the issue point behind the last LDS read of
// the K preparation the compiler's wait falls where the V rows are needed anyway.)
// Three s_barrier per pair: [K(kb) landed, V(kb-1) consumed]; [K(kb) in registers] -> issue V(kb), K(kb+1); [V(kb) landed].
// The V^T fragments are gathered with 16-bit LDS reads from the row-major V rows (v5), outputs go back through the dead Q rows so
// that the workgroup stores 144-byte-per-head row segments with 16-byte stores; rows >= T are never stored.
// Rows of a tail block behind T are the last frame's again (row index clamped in the DMA offsets): finite, and masked to -1e30.
//
// LDS does not grow with T: Q / K / V images 3 x 20 480, cos | sin rows of the query and of the key block 2 x 9 216, norm weights
// 640 = 80 512 bytes -> TWO workgroups per CU (2 waves per SIMD, 256 VGPRs each; the build-resource test pins no scratch, <= 256
// VGPRs, <= 81 920 bytes).  Compiled for gfx950: 204 (Latte) to 239 (Open-Sora) VGPRs, no scratch.
//
// K rows are prepared (RMS-norm, weight, rotation) PER PAIR, not once per (item, key block): a unit owns one query block, the raw K
// block is re-fetched (L2: the units of an item are neighbours in the grid) and re-prepared by each of the T / 32 units of the item.
// Per lane and pair that is ~150 VALU instructions (18 dwords x ~7 + the sum of squares) beside ~140 of softmax and ~100 of V^T
// gather / P packing; preparing once would need the prepared K of the whole item resident (grows with T) or a second kernel and a
// round trip through HBM for 1/3 of the operand bytes.  At T = 120 the redo is 3 extra preparations of 4 per head and query block.
//
// Addressing: the buffer descriptor is re-based with a 64-bit address per (unit, frame block), so only a 32-frame block's span
// (31 S row_stride 2 bytes + a row) must fit 31 bits — 796 MB at 720p x 16 s, where T S row_stride 2 is 2.98 GB.
// Modes (flags at compile time): 1 = norm + RoPE (Open-Sora), 2 = neither (Latte), 4 = RoPE only (Open-Sora-Plan v1.1).  Norm without
// RoPE is not built: the launcher returns VSYS_ERR_SHAPE and launch_attn_temporal_d72 keeps the VALU kernel for it up to T = 284.
// The rotation is written as plain fp32 FMAs and this file is compiled without packed-fp32 instructions (__graft_entry__.py).
#include "common.h"
#include "vsys_internal.h"

namespace vsys {
namespace {

constexpr int HD = 72;
constexpr int HPG = 4;                        // heads (= waves) per workgroup
constexpr int PIECES = 37;                    // 16-byte pieces per image row (36 + 1 pad)
constexpr int PITCH = PIECES * 16;            // 592
constexpr int NIW = 5;                        // LDS-DMA instructions per wave and operand block: 4 x 5 x 64 pieces >= 32 x 37
constexpr int IMG_BYTES = HPG * NIW * 1024;   // 20480 (rows 32 .. 34 are the spare tail)
constexpr int TAB_ROW = 36;                   // floats per position in the compact cos / sin rows
constexpr int TAB_BYTES = 2 * 32 * TAB_ROW * 4;   // cos rows, then sin rows: 9216
constexpr int NTW = 9;                        // dword LDS-DMA instructions per wave and table block: 4 x 9 x 64 = 2 x 32 x 36
constexpr int WF_BYTES = 320;                 // one norm-weight vector as fp32 (72 floats, padded)
constexpr int OFF_Q = 0, OFF_K = IMG_BYTES, OFF_V = 2 * IMG_BYTES, OFF_QTAB = 3 * IMG_BYTES, OFF_KTAB = OFF_QTAB + TAB_BYTES,
              OFF_W = OFF_KTAB + TAB_BYTES, LDS_BYTES = OFF_W + 2 * WF_BYTES;   // 80512
constexpr float NEG_BIG = -1e30f;
constexpr float LOG2E = 1.4426950408889634f;

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// One 16-byte piece (8 dims = 4 rotary pairs) of a q / k row -> the fragment dwords, ONE rounding: x * rs [* w], rotated.
template <int MODE>
__device__ __forceinline__ void tl_piece(uint32_t (&u)[4], const float* wf, const float* cosrow, const float* sinrow, int c, int hi,
                                         float rs, bool scaled) {
  constexpr bool NORM = MODE == 1, ROPE = MODE == 1 || MODE == 4;
  if (!NORM && !ROPE && !scaled) return;     // (Latte keys: the raw bf16 pairs are the fragment)
  float wv[8], cv[4], sv[4];
  if constexpr (NORM) {
    const float4 wa = *reinterpret_cast<const float4*>(wf + 16 * c + 8 * hi), wb = *reinterpret_cast<const float4*>(wf + 16 * c + 8 * hi + 4);
    wv[0] = wa.x; wv[1] = wa.y; wv[2] = wa.z; wv[3] = wa.w; wv[4] = wb.x; wv[5] = wb.y; wv[6] = wb.z; wv[7] = wb.w;
  }
  if constexpr (ROPE) {
    const float4 cs = *reinterpret_cast<const float4*>(cosrow + 8 * c + 4 * hi);
    const float4 sn = *reinterpret_cast<const float4*>(sinrow + 8 * c + 4 * hi);
    cv[0] = cs.x; cv[1] = cs.y; cv[2] = cs.z; cv[3] = cs.w; sv[0] = sn.x; sv[1] = sn.y; sv[2] = sn.z; sv[3] = sn.w;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float x0 = bflo(u[e]) * rs, x1 = bfhi(u[e]) * rs;
    if constexpr (NORM) { x0 *= wv[2 * e]; x1 *= wv[2 * e + 1]; }
    if constexpr (ROPE) {   // (x0, x1) c + (-x1, x0) s
      const float r0 = __builtin_fmaf(-x1, sv[e], x0 * cv[e]), r1 = __builtin_fmaf(x0, sv[e], x1 * cv[e]);
      x0 = r0; x1 = r1;
    }
    u[e] = pack2bf(f32x2{x0, x1});
  }
}

// every LDS access so far has completed and (N >= 0) at most N of this wave's memory transfers are still in flight, then the
// workgroup meets.  Written out: a compiler-generated s_barrier is preceded by s_waitcnt vmcnt(0) on this target.
#define TL_BARRIER_VM(N_) asm volatile("s_waitcnt vmcnt(" #N_ ") lgkmcnt(0)\n\ts_barrier" ::: "memory")
#define TL_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

template <int MODE>
__global__ __launch_bounds__(256, 2) void attn_temporal_d72_long_kernel(
    const bf16_t* __restrict__ qkv, int64_t row_stride, int C, const bf16_t* __restrict__ q_norm_w, const bf16_t* __restrict__ k_norm_w,
    const float* __restrict__ rope_cos, const float* __restrict__ rope_sin, bf16_t* __restrict__ out, int64_t out_stride, int T, int S,
    int heads, float eps, float scale) {
#if __HIP_DEVICE_COMPILE__
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool NORM = MODE == 1, ROPE = MODE == 1 || MODE == 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  float* qwf = reinterpret_cast<float*>(smem + OFF_W);
  float* kwf = reinterpret_cast<float*>(smem + OFF_W + WF_BYTES);

  // ---- the unit: query block fastest, then the head group, the pixel token, the sample (neighbours share an XCD's L2)
  const int nblk = (T + 31) >> 5, HG = (heads + HPG - 1) / HPG;
  int u = xcd_remap(blockIdx.x, gridDim.x);
  const int qb = u % nblk; u /= nblk;
  const int hg = u % HG; u /= HG;
  const int s = u % S, b = u / S;
  const int nh = heads - HPG * hg < HPG ? heads - HPG * hg : HPG;   // heads of this group (a last partial group: 1 .. 3)
  const bool active = wave_u < nh;

  // ---- unit-independent addressing of the LDS-DMA.  Image: instruction ii = wave + 4 i of the workgroup fills pieces 64 ii .. + 63;
  // LDS piece L = piece (L % 37) of row (L / 37).  The pad slot and the pieces of absent heads receive a copy of the last real piece.
  const int frame_bytes = S * (int)row_stride * 2;        // consecutive frames of one pixel token (launcher: 32 of them fit 31 bits)
  int rowi[NIW], pofi[NIW];
#pragma unroll
  for (int i = 0; i < NIW; ++i) {
    const int L = lane + 64 * (wave_u + HPG * i);
    int row = L / PIECES, piece = L - row * PIECES;
    piece = piece < nh * 9 ? piece : nh * 9 - 1;
    rowi[i] = row < 32 ? row : 31;
    pofi[i] = piece * 16;
  }
  // table rows: instruction ii = wave + 4 j fills floats 64 ii .. + 63 of [cos: 32 x 36 | sin: 32 x 36]; ii < 18 is cos (wave-uniform)
  int trel[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int ii = wave_u + HPG * j;
    const int e = lane + 64 * (ii < 18 ? ii : ii - 18);
    const int row = e / TAB_ROW, col = e - row * TAB_ROW;
    trel[j] = (row << 16) | (col * 8);                    // element 2 col of the [T][72] fp32 table
  }
  const auto rs_cos = __builtin_amdgcn_make_buffer_rsrc((void*)rope_cos, 0, ROPE ? T * HD * 4 : 0, 0x00020000);
  const auto rs_sin = __builtin_amdgcn_make_buffer_rsrc((void*)rope_sin, 0, ROPE ? T * HD * 4 : 0, 0x00020000);

  // rows of frame block ``blk`` of operand column ``col`` (0 = q, C = k, 2 C = v) -> image ``dst``: descriptor re-based per block
  auto dma_rows = [&](char* dst, int blk, int col) {
    const int rows = T - 32 * blk < 32 ? T - 32 * blk : 32;
    const bf16_t* base = qkv + (((int64_t)b * T + 32 * blk) * S + s) * row_stride + hg * (HPG * HD);
    const int nbytes = (rows - 1) * frame_bytes + (col + nh * HD) * 2;
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, nbytes, 0x00020000);
#pragma unroll
    for (int i = 0; i < NIW; ++i) {
      const int r = rowi[i] < rows ? rowi[i] : rows - 1;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr_t)(dst + (wave_u + HPG * i) * 1024), 16, r * frame_bytes + pofi[i] + col * 2, 0, 0, 0);
    }
  };
  auto dma_tab = [&](char* dst, int blk) {
    if constexpr (ROPE) {
#pragma unroll
      for (int j = 0; j < NTW; ++j) {
        const int ii = wave_u + HPG * j;
        int t = 32 * blk + (trel[j] >> 16);
        t = t < T ? t : T - 1;
        const int vo = t * (HD * 4) + (trel[j] & 0xffff);
        if (ii < 18) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_cos, (lds_ptr_t)(dst + ii * 256), 4, vo, 0, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_sin, (lds_ptr_t)(dst + ii * 256), 4, vo, 0, 0, 0);
      }
    }
  };

  dma_rows(smem + OFF_Q, qb, 0);
  dma_tab(smem + OFF_QTAB, qb);
  dma_rows(smem + OFF_K, 0, C);
  dma_tab(smem + OFF_KTAB, 0);
  if (NORM && tid < HD) {
    qwf[tid] = bf2f(q_norm_w[tid]);
    kwf[tid] = bf2f(k_norm_w[tid]);
  }

  // A-operand row m = l31 of the first product holds this key of a block (attention_t3.hip); query / value rows are natural
  const int r_of_m = (l31 & 3) + 4 * (l31 >> 3);
  const int krow = 8 * ((l31 >> 2) & 1) + r_of_m + (r_of_m >= 8 ? 8 : 0);
  const int hoff = wave * (HD * 2);                       // this wave's head inside the 576-byte segments
  const char* kpiece = smem + OFF_K + krow * PITCH + hoff + 16 * hi;
  char* qpiece = smem + OFF_Q + l31 * PITCH + hoff + 16 * hi;          // Q in, O out
  const char* vbase = smem + OFF_V + hoff + l31 * 2 + hi * 8 * PITCH;  // + 64 d + (16 ch + j) * 592: V^T element (dim 32 d + l31, key 16 ch + 8 hi + j)
  const bool q_ok = 32 * qb + l31 < T;

  // the pieces of one row held by this lane: RMS-norm, weight, rotation (q: 72^-1/2 rides on rstd) -> MFMA fragments
  auto make_frags = [&](const char* rowp, bf16x8 (&frag)[5], const float* wf, const float* tab, int pos, bool scaled) {
    uint4 raw[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      raw[c] = make_uint4(0, 0, 0, 0);
      if (c < 4 || hi == 0) raw[c] = *reinterpret_cast<const uint4*>(rowp + 32 * c);
    }
    float rstd = 1.f;
    if constexpr (NORM) {
      float ss = 0.f;
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        const uint32_t w[4] = {raw[c].x, raw[c].y, raw[c].z, raw[c].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bf16x2 pr = __builtin_bit_cast(bf16x2, w[e]);
          ss = __builtin_amdgcn_fdot2_f32_bf16(pr, pr, ss, false);
        }
      }
      ss += __shfl_xor(ss, 32, 64);
      rstd = rsqrtf(ss * (1.0f / (float)HD) + eps);
    }
    const float rs = scaled ? rstd * scale : rstd;
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      uint32_t w[4] = {raw[c].x, raw[c].y, raw[c].z, raw[c].w};
      if (c < 4 || hi == 0) tl_piece<MODE>(w, wf, tab + pos * TAB_ROW, tab + (32 + pos) * TAB_ROW, c, hi, rs, scaled);
      frag[c] = __builtin_bit_cast(bf16x8, make_uint4(w[0], w[1], w[2], w[3]));
    }
  };

  bf16x8 qf[5];
  f32x16 oacc[3];
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;
  float m = NEG_BIG, l = 0.f;     // running maximum of the row (both lanes of a query agree) and THIS lane's part of the sum

  for (int kb = 0; kb < nblk; ++kb) {
    TL_BARRIER_VM(0);             // K(kb) and its table rows (kb = 0: Q, its rows, the weights) are in LDS; V(kb - 1) is consumed
    bf16x8 kf[5];
    if (active) {
      if (kb == 0) make_frags(qpiece, qf, qwf, reinterpret_cast<const float*>(smem + OFF_QTAB), l31, true);
      make_frags(kpiece, kf, kwf, reinterpret_cast<const float*>(smem + OFF_KTAB), krow, false);
    }
    TL_BARRIER();                 // every wave holds its K fragments: the K image and the key rows of the tables are free
    dma_rows(smem + OFF_V, kb, 2 * C);
    if (kb + 1 < nblk) {
      dma_rows(smem + OFF_K, kb + 1, C);
      dma_tab(smem + OFF_KTAB, kb + 1);
    }
    bf16x8 p0, p1;
    if (active) {
      f32x16 sacc;
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
      for (int c = 0; c < 5; ++c) sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[c], qf[c], sacc, 0, 0, 0);
      // accumulator r <-> key 32 kb + 8 hi + r + 8 (r >= 8) of this lane's query
      if (32 * kb + 32 > T) {     // (the tail block: wave-uniform)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (32 * kb + 8 * hi + r + (r >= 8 ? 8 : 0) >= T) sacc[r] = NEG_BIG;
      }
      float bm = sacc[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) bm = fmaxf(bm, sacc[r]);
      bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
      const float m_new = fmaxf(m, bm);
      if (__any(m_new > m)) {     // some row of the wave moved its maximum: O and l follow it
        const float alpha = __builtin_amdgcn_exp2f((m - m_new) * LOG2E);
        l *= alpha;
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
          for (int r = 0; r < 16; ++r) oacc[d][r] *= alpha;
      }
      m = m_new;
      const float ml = m * LOG2E;
      float p[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[r], LOG2E, -ml));
        l += p[r];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        p0[e] = (__bf16)p[e];
        p1[e] = (__bf16)p[8 + e];
      }
    }
    TL_BARRIER_VM(0);             // V(kb) has landed (and K(kb + 1) with it: see the header on the compiler's own waits)
    if (active) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        // V^T fragments gathered from the row-major V rows: element j <-> key 16 ch + 8 hi + j of dim 32 d + l31 (dims >= 72 of the
        // last head run on into the pad and the next row: those output rows are discarded)
        bf16x8 v0, v1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          v0[j] = *reinterpret_cast<const __bf16*>(vbase + 64 * d + j * PITCH);
          v1[j] = *reinterpret_cast<const __bf16*>(vbase + 64 * d + (16 + j) * PITCH);
        }
        oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v0, p0, oacc[d], 0, 0, 0);
        oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v1, p1, oacc[d], 0, 0, 0);
      }
    }
  }

  // ---- O / l, one rounding, into this wave's own bytes of the Q rows (its Q pieces are in registers; no other wave touches them)
  if (active) {
    l += __shfl_xor(l, 32, 64);
    const float inv = __builtin_amdgcn_rcpf(l);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      uint2 o[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        o[g].x = pack2bf(f32x2{oacc[d][4 * g] * inv, oacc[d][4 * g + 1] * inv});
        o[g].y = pack2bf(f32x2{oacc[d][4 * g + 2] * inv, oacc[d][4 * g + 3] * inv});
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {   // accumulator 4 g + r' of block d <-> dim 32 d + 8 g + 4 hi + r': swap pairs of groups -> 16 contiguous bytes
        auto sx = __builtin_amdgcn_permlane32_swap(o[2 * k].x, o[2 * k + 1].x, false, false);
        auto sy = __builtin_amdgcn_permlane32_swap(o[2 * k].y, o[2 * k + 1].y, false, false);
        const int dim0 = 32 * d + 16 * k;   // + 8 hi: the 16 hi bytes inside qpiece
        if (q_ok && dim0 + 8 * hi + 8 <= HD)
          *reinterpret_cast<uint4*>(qpiece + dim0 * 2) = make_uint4(sx[0], sy[0], sx[1], sy[1]);
      }
    }
  }
  TL_BARRIER();
  // ---- the workgroup stores the real rows of the block, the real heads of the group: nh x 9 pieces of 16 bytes per row
  const int rows = T - 32 * qb < 32 ? T - 32 * qb : 32, npo = nh * 9;
  bf16_t* obase = out + (((int64_t)b * T + 32 * qb) * S + s) * out_stride + hg * (HPG * HD);
  for (int Lp = tid; Lp < rows * npo; Lp += 256) {
    const int row = Lp / npo, piece = Lp - row * npo;
    const uint4 v = *reinterpret_cast<const uint4*>(smem + OFF_Q + row * PITCH + piece * 16);
    *reinterpret_cast<uint4*>(obase + (int64_t)row * S * out_stride + piece * 8) = v;
  }
#endif
}

}  // namespace

// VSYS_ERR_SHAPE / VSYS_ERR_ALIGN = this kernel does not take the problem (launch_attn_temporal_d72 then keeps the VALU kernel where
// that one still fits, T <= 284); nothing has been launched in that case.
int launch_attn_temporal_d72_long(const bf16_t* qkv, int64_t row_stride, int C, const bf16_t* q_norm_w, const bf16_t* k_norm_w,
                                  const float* rope_cos, const float* rope_sin, bf16_t* out, int64_t out_stride, int B, int T, int S,
                                  int heads, float eps, float scale, hipStream_t stream) {
  if (T <= 64 || (row_stride % 8) || (out_stride % 8) || (C % 8)) return VSYS_ERR_SHAPE;
  const bool norm = q_norm_w != nullptr, rope = rope_cos != nullptr;
  if (norm != (k_norm_w != nullptr) || rope != (rope_sin != nullptr)) return VSYS_ERR_SHAPE;
  if (norm && !rope) return VSYS_ERR_SHAPE;                    // norm without RoPE: no model runs it; not built here
  // one 32-frame block of one pixel token, to the end of its last v segment, in 31 bits (the descriptor is re-based per block)
  if (31 * (int64_t)S * row_stride * 2 + ((int64_t)2 * C + HPG * HD) * 2 > 0x7fffffff) return VSYS_ERR_SHAPE;
  if ((int64_t)T * HD * 4 > 0x7fffffff) return VSYS_ERR_SHAPE;  // the RoPE tables behind one descriptor
  const int64_t units = (int64_t)B * S * ((heads + HPG - 1) / HPG) * ((T + 31) / 32);
  if (units > 0x7fffffff) return VSYS_ERR_SHAPE;
  // 16-byte LDS-DMA pieces and 16-byte stores; the tables are read dword by dword
  if (((uintptr_t)qkv & 15) || ((uintptr_t)out & 15) || ((uintptr_t)rope_cos & 3) || ((uintptr_t)rope_sin & 3)) return VSYS_ERR_ALIGN;
  static std::atomic<unsigned long long> attr_seen{0};
  for (DeviceOnce once(attr_seen); once.todo(); once.done()) {
    (void)hipFuncSetAttribute((const void*)attn_temporal_d72_long_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    (void)hipFuncSetAttribute((const void*)attn_temporal_d72_long_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    (void)hipFuncSetAttribute((const void*)attn_temporal_d72_long_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
  }
#define TL_LAUNCH(M_)                                                                                                                  \
  hipLaunchKernelGGL(attn_temporal_d72_long_kernel<M_>, dim3((unsigned)units), dim3(256), LDS_BYTES, stream, qkv, row_stride, C, q_norm_w, \
                     k_norm_w, rope_cos, rope_sin, out, out_stride, T, S, heads, eps, scale)
  if (norm) TL_LAUNCH(1);
  else if (rope) TL_LAUNCH(4);
  else TL_LAUNCH(2);
#undef TL_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

}  // namespace vsys
