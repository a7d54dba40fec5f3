// vae_flash_attn: the single-head mid-block attention of the VAEs (AttnBlock3DFix, autoencoder_kl_open_sora_plan_v120.py:360-415;
// diffusers Attention under the 2-D decoders) as a flash kernel at head dim C = 128 NB, NB = 1, 2, 4 (hidden sizes 32, 64 and the
// 512 channels of every real checkpoint).  Per frame  o = softmax(scale q k^T) v  over the first L of Lp rows; no score matrix
// exists, so the 8192-key limit of vsys_softmax_rows and the L^2 x 12 bytes of score traffic of the three-GEMM form are gone.
// The d72 / d64 / d96 flash kernels keep O of a query row in a few registers per lane; here O of ONE row is 512 fp32, and the whole
// design follows from where those live.
//
// Work split.  One workgroup = 8 waves = one UNIT (frame, block of 128 query rows); wave w owns query rows 16 w .. 16 w + 15 and the
// FULL width C of their output.  The unit walks the ceil(L / 32) key blocks; per (query block, key block) pair and wave
//   S^T = K Q^T     2 x C / 32 x v_mfma_f32_16x16x32_bf16  (two tiles of 16 keys; A = K rows in a permuted key order: row m of tile h
//                                                           is key 8 (m / 4) + 4 h + m % 4, so the 2 x 4 accumulators of lane (query,
//                                                           quad) are keys 8 quad .. 8 quad + 7 of ITS query)
//   online softmax  exp2 domain (scale log2 e is applied to the fp32 logits, q is the stored operand bit for bit), fp32 running max m
//                   and sum l per query row; P rounded to bf16 (unnormalised, <= 1), l summed from the unrounded P; the rescale of O
//                   by 2^(m - m') is skipped when no row of the wave moved its maximum
//   O^T += V^T P^T  C / 16 x v_mfma_f32_16x16x32_bf16  (blocks of 16 output dims x all 32 keys; those eight keys per lane ARE the B
//                                                       operand: P never leaves its lane)
// and O / l is rounded ONCE at the end of the unit: the block-loop contract of attention_tlong.hip.
//
// Registers (NB = 4): O^T 16 query columns x 512 dims = 128 accumulators per lane, Q fragments 64 (read from HBM once per unit, the B
// operand of every S product), S 8, P 4, two pairs of K / V fragments 16, addresses: 249 of the 256 that two waves per SIMD
// (__launch_bounds__(512, 1)) leave a wave, no scratch; NB = 2 / 1: 151 / 96.  32 query rows per wave on v_mfma_f32_32x32x16_bf16
// (O 256 + Q 128 at one wave per SIMD) was built first: S and O must both live in the accumulation half there, 272 of its 256
// registers, and the compiler spilled 237.  What 16 rows cost is in "what bounds it".  The fragment reads are issued in pairs, one
// pair ahead of its MFMAs, between scheduling fences: left alone the scheduler hoists all 64 reads of a block and spills.
//
// Data movement.  V arrives as V^T [n, C, ldv] (what attention_core's batched GEMM already writes): lane (dim, quad) of the PV product
// needs 8 consecutive KEYS of one dim, which is ONE 16-byte LDS read from V^T rows and would be eight 16-bit gathers from plain V
// rows (attention_tlong.hip pays those at d = 72; at d = 512 they would outnumber the MFMAs 8 : 1).  A key block is 32 K rows
// (32 x 2 C bytes) and C V^T rows of 32 keys (C x 64 bytes): 64 KB at NB = 4, fetched by LDS-DMA (buffer_load_dwordx4 ... lds),
// NB wave instructions per wave and operand, nothing through registers, into one of TWO buffers: block kb + 1 is issued right
// behind the barrier that opens block kb and travels under its 64 MFMAs (the compiler puts no wait of its own into the loop).
// ONE s_barrier per key block: [K / V(kb) landed in every wave's view, buffer of kb - 1 consumed].  16-byte pieces are XOR-swizzled
// on the way in (K: piece ^ swz(row); V^T: piece ^ (row / 4 & 3)) so that the 16 lanes of a ds_read_b128 phase hit 16 different
// bank groups although K rows are 1 KB and V^T rows 64 B apart.  LDS = 32 KB x NB x 2 buffers = 128 KB of the CU's 160 KB at NB = 4
// (a static_assert; tests/test_build_resources_vae_flash.py pins no scratch and <= 256 registers); the O rows leave through the
// same bytes (128 rows x 2 C) so that the workgroup stores whole rows with 16-byte stores.
//
// What bounds it.  Per key block a wave reads 32 KB of K and 32 KB of V^T fragments from LDS for 2 x 16 x 32 x 512 x 2 = 1.05 MFLOP:
// 16 flop per LDS byte.  The CU's LDS port (128 bytes per clock) then allows 8 waves x 64 KB / 128 = 4096 clocks per block against
// 8 x 64 MFMAs x 16 clocks / 4 SIMDs = 2048 on the matrix pipe: LDS binds at about half the MFMA rate, which is where the measurement
// sits (profiles/vae_flash_attn_timing.json: 788 TFLOP/s at 720p with the projections in the time).  32 rows per wave would double
// the flop per LDS byte and balance the two; so would splitting C over the waves (a cross-wave S reduction, two more barriers per
// block, another split at NB = 1).  HBM / L2 traffic is not the limit: the 128 rows of a unit share each DMA'd byte, and no score
// matrix exists.
//
// Edges.  Keys >= L are masked to -1e30 before the maximum (L need not be a multiple of 4; block 0 always holds a real key).  DMA
// row indices of a tail block are clamped to the last real K row, V^T pieces behind Lp to the last piece inside the row: nothing
// outside the operands is read, and the buffer descriptors — re-based with a 64-bit address per (frame, key block), so only a
// block's span must fit 31 bits — end at the last byte the block owns.  V^T columns L .. Lp - 1 meet P = 0 and must be FINITE
// (attention_core leaves zeros there).  Query rows >= L read row L - 1 again and are never stored; rows L .. Lp - 1 of o are not
// written.  The softmax scale and the rescale are plain fp32 multiplies / FMAs and this file is compiled without packed-fp32
// instructions (__graft_entry__.py), so the bits do not depend on what the compiler would pair.
#include "common.h"
#include "vsys_internal.h"

namespace vsys {
namespace {

constexpr float NEG_BIG = -1e30f;
constexpr float LOG2E = 1.4426950408889634f;

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// every LDS access of this wave has completed and none of its memory transfers is in flight, then the workgroup meets
#define VF_BARRIER() asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory")

constexpr int NW = 8;          // waves per workgroup
constexpr int QR = 16 * NW;    // query rows per unit
// K rows 8 a + 4 h + b (a, b = 0 .. 3) are what the 16 lanes of one ds_read_b128 phase read for S tile h: 4 a + b tells them apart
__device__ __forceinline__ int swz(int row) { return ((row >> 3) << 2) | (row & 3); }

template <int NB>
__global__ __launch_bounds__(64 * NW, 1) void vae_flash_attn_kernel(const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k,
                                                                    int64_t ldk, const bf16_t* __restrict__ vt, int64_t ldv,
                                                                    bf16_t* __restrict__ o, int64_t ldo, int L, int Lp, float sl2) {
#if __HIP_DEVICE_COMPILE__
  constexpr int C = 128 * NB;
  constexpr int PPR = C / 8;                 // 16-byte pieces per K (and O) row
  constexpr int PPR_SHIFT = NB == 1 ? 4 : NB == 2 ? 5 : 6;
  constexpr int NI = 8 * NB / NW;            // LDS-DMA instructions per wave and operand block: NW x NI x 64 pieces = 32 x PPR = C x 4
  constexpr int K_BYTES = 32 * C * 2;        // K image of a block; the V^T image (C rows x 64 bytes) is as large
  constexpr int BUF = 2 * K_BYTES;
  static_assert(2 * BUF <= 160 * 1024 && 2 * BUF == QR * C * 2, "two buffers inside the CU's LDS; the O image of the unit fills exactly them");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, quad = lane >> 4;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);

  // ---- the unit: query block fastest, then the frame (neighbours in the grid walk the same K / V^T in an XCD's L2)
  const int nqb = (L + QR - 1) / QR, nkb = (L + 31) >> 5;
  const int u = xcd_remap(blockIdx.x, gridDim.x);
  const int qb = u % nqb, f = u / nqb;
  const int q0 = QR * qb;
  const bf16_t* kfr = k + (int64_t)f * Lp * ldk;
  const bf16_t* vfr = vt + (int64_t)f * C * ldv;
  const int ldk2 = (int)ldk * 2, ldv2 = (int)ldv * 2;   // row pitches in bytes (launcher: a block's span fits 31 bits)

  // key block kb -> buffer buf.  K image: instruction ii = wave + NW i fills LDS pieces 64 ii .. + 63; LDS piece P = (row P / PPR,
  // slot P % PPR) receives piece slot ^ swz(row) of that row.  V^T image: LDS piece P = (dim P / 4, slot P % 4) receives the keys
  // 8 g .. 8 g + 7 of the block with g = slot ^ (dim / 4 & 3) — a lane constant, since dim / 4 & 3 = lane bits 4, 5.
  const int gv = (lane & 3) ^ ((lane >> 4) & 3);
  auto dma_block = [&](int kb, int buf) {
    char* dst = smem + buf * BUF;
    const int rows = L - 32 * kb < 32 ? L - 32 * kb : 32;
    const auto rs_k = __builtin_amdgcn_make_buffer_rsrc((void*)(kfr + (int64_t)32 * kb * ldk), 0, (rows - 1) * ldk2 + C * 2, 0x00020000);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int ii = wave_u + NW * i;
      const int P = lane + 64 * ii;
      const int row = P >> PPR_SHIFT, slot = P & (PPR - 1);
      const int r = row < rows ? row : rows - 1;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_k, (lds_ptr_t)(dst + ii * 1024), 16, r * ldk2 + ((slot ^ swz(row)) << 4), 0, 0, 0);
    }
    const int pieces = Lp - 32 * kb < 32 ? (Lp - 32 * kb) >> 3 : 4;   // 16-byte pieces of the block inside a V^T row (>= 1)
    const auto rs_v = __builtin_amdgcn_make_buffer_rsrc((void*)(vfr + 32 * kb), 0, (C - 1) * ldv2 + pieces * 16, 0x00020000);
    const int g = gv < pieces ? gv : pieces - 1;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int ii = wave_u + NW * i;
      const int dim = (lane >> 2) + 16 * ii;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_v, (lds_ptr_t)(dst + K_BYTES + ii * 1024), 16, dim * ldv2 + (g << 4), 0, 0, 0);
    }
  };
  dma_block(0, 0);

  // ---- Q fragments of this lane's query (B operand: lane (query l15, quad) holds dims 32 c + 8 quad .. + 7), straight from HBM
  const bool active = q0 + 16 * wave_u < L;    // a wave whose 16 rows are all behind L only moves data and meets the barriers
  bf16x8 qf[C / 32];
  {
    int qrow = q0 + 16 * wave + l15;
    qrow = qrow < L ? qrow : L - 1;
    const bf16_t* qp = q + ((int64_t)f * Lp + qrow) * ldq + 8 * quad;
#pragma unroll
    for (int c = 0; c < C / 32; ++c) qf[c] = *reinterpret_cast<const bf16x8*>(qp + 32 * c);
  }

  // A-operand row m = l15 of S tile h holds key 8 (m / 4) + 4 h + m % 4 of the block, so that accumulator r of tile h in lane
  // (query, quad) is key 8 quad + 4 h + r: the eight keys 8 quad .. + 7 the lane feeds to the PV product as its B operand
  const int krow0 = 8 * (l15 >> 2) + (l15 & 3);   // tile 1: + 4 (swz ignores that bit)
  const int kx = quad ^ swz(krow0);               // piece 4 c + quad of the row sits in slot (4 c) ^ kx (bits 0, 1 of 4 c are clear)
  const int koff = krow0 * (C * 2);
  const int voff = K_BYTES + l15 * 64 + ((quad ^ ((l15 >> 2) & 3)) << 4);   // keys 8 quad .. + 7 of dim 16 d + l15: + d x 1024

  f32x4 oacc[C / 16];
#pragma unroll
  for (int d = 0; d < C / 16; ++d) oacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = NEG_BIG, l = 0.f;     // running maximum of the row (the four lanes of a query agree) and THIS lane's part of the sum

  for (int kb = 0; kb < nkb; ++kb) {
    VF_BARRIER();                 // K / V^T(kb) are in LDS for every wave; the other buffer (block kb - 1) is consumed
    if (kb + 1 < nkb) dma_block(kb + 1, (kb + 1) & 1);
    if (active) {
      const char* img = smem + (kb & 1) * BUF;
      f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = s0;
      // fragments in pairs (one 32-dim slice x the two key tiles), the next pair's LDS reads issued in front of this pair's MFMAs and
      // fenced there: left to itself the scheduler hoists every read of the block to its top, and the registers for that do not
      // exist beside Q and O
      bf16x8 kf[2][2];
#pragma unroll
      for (int j = 0; j < 2; ++j) kf[0][j] = *reinterpret_cast<const bf16x8*>(img + koff + j * (4 * C * 2) + (kx << 4));
#pragma unroll
      for (int c = 0; c < C / 32; ++c) {
        if (c + 1 < C / 32) {
#pragma unroll
          for (int j = 0; j < 2; ++j)
            kf[(c + 1) & 1][j] = *reinterpret_cast<const bf16x8*>(img + koff + j * (4 * C * 2) + (((4 * (c + 1)) ^ kx) << 4));
        }
        __builtin_amdgcn_sched_barrier(0);
        s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[c & 1][0], qf[c], s0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[c & 1][1], qf[c], s1, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      float sv[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};   // sv[j] <-> key 32 kb + 8 quad + j of this lane's query
      if (32 * kb + 32 > L) {     // (the tail block: wave-uniform)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (32 * kb + 8 * quad + j >= L) sv[j] = NEG_BIG;
      }
      float bm = sv[0];
#pragma unroll
      for (int j = 1; j < 8; ++j) bm = fmaxf(bm, sv[j]);
      bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
      bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
      const float m_new = fmaxf(m, bm);
      if (__any(m_new > m)) {     // some row of the wave moved its maximum: O and l follow it
        const float alpha = __builtin_amdgcn_exp2f((m - m_new) * sl2);
        l *= alpha;
#pragma unroll
        for (int d = 0; d < C / 16; ++d)
#pragma unroll
          for (int r = 0; r < 4; ++r) oacc[d][r] *= alpha;
      }
      m = m_new;
      const float ml = m * sl2;
      bf16x8 pf;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sv[j], sl2, -ml));
        l += p;
        pf[j] = (__bf16)p;
      }
      bf16x8 vf[2][2];           // two output blocks of 16 dims per step, pipelined and fenced like the K fragments
#pragma unroll
      for (int j = 0; j < 2; ++j) vf[0][j] = *reinterpret_cast<const bf16x8*>(img + voff + j * 1024);
#pragma unroll
      for (int g = 0; g < C / 32; ++g) {
        if (g + 1 < C / 32) {
#pragma unroll
          for (int j = 0; j < 2; ++j) vf[(g + 1) & 1][j] = *reinterpret_cast<const bf16x8*>(img + voff + (2 * g + 2 + j) * 1024);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 2; ++j) oacc[2 * g + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[g & 1][j], pf, oacc[2 * g + j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // ---- O / l, one rounding, through LDS (both buffers are dead once every wave has left the loop): row R = 16 wave + l15 of the
  // unit at R x 2 C bytes, piece g of it in slot g ^ (R & 15); accumulator r of block d <-> dim 16 d + 4 quad + r
  VF_BARRIER();
  if (active) {
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = __builtin_amdgcn_rcpf(l);
    const int R = 16 * wave + l15;
    char* orow = smem + R * (C * 2) + (quad & 1) * 8;
#pragma unroll
    for (int d = 0; d < C / 16; ++d) {
      const uint2 v = make_uint2(pack2bf(f32x2{oacc[d][0] * inv, oacc[d][1] * inv}), pack2bf(f32x2{oacc[d][2] * inv, oacc[d][3] * inv}));
      *reinterpret_cast<uint2*>(orow + (((2 * d + (quad >> 1)) ^ l15) << 4)) = v;
    }
  }
  VF_BARRIER();
  // ---- the workgroup stores the rows of the block in front of L
  const int rows = L - q0 < QR ? L - q0 : QR;
  bf16_t* ob = o + ((int64_t)f * Lp + q0) * ldo;
  for (int idx = tid; idx < rows * PPR; idx += 64 * NW) {
    const int row = idx >> PPR_SHIFT, piece = idx & (PPR - 1);
    const uint4 v = *reinterpret_cast<const uint4*>(smem + row * (C * 2) + ((piece ^ (row & 15)) << 4));
    *reinterpret_cast<uint4*>(ob + (int64_t)row * ldo + piece * 8) = v;
  }
#endif
}

template <int NB>
int vf_launch(const bf16_t* q, int64_t ldq, const bf16_t* k, int64_t ldk, const bf16_t* vt, int64_t ldv, bf16_t* o, int64_t ldo,
              int64_t units, int L, int Lp, float sl2, hipStream_t stream) {
  constexpr int LDS_BYTES = 4 * 32 * 128 * NB * 2;   // two buffers of (K + V^T) images: 32 KB x NB
  static std::atomic<unsigned long long> attr_seen{0};
  for (DeviceOnce once(attr_seen); once.todo(); once.done())
    (void)hipFuncSetAttribute((const void*)vae_flash_attn_kernel<NB>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
  hipLaunchKernelGGL(vae_flash_attn_kernel<NB>, dim3((unsigned)units), dim3(64 * NW), LDS_BYTES, stream, q, ldq, k, ldk, vt, ldv, o, ldo, L, Lp,
                     sl2);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

}  // namespace

// VSYS_ERR_SHAPE / VSYS_ERR_ALIGN / VSYS_ERR_ARG: nothing has been launched.
int launch_vae_flash_attn(const bf16_t* q, int64_t ldq, const bf16_t* k, int64_t ldk, const bf16_t* vt, int64_t ldv, bf16_t* o,
                          int64_t ldo, int64_t n, int64_t L, int64_t Lp, int64_t C, float scale, hipStream_t stream) {
  if (C != 128 && C != 256 && C != 512) return VSYS_ERR_SHAPE;
  if (n < 1 || L < 1 || Lp < L || Lp > 0x7fffffff || ldq < C || ldk < C || ldo < C || ldv < Lp) return VSYS_ERR_SHAPE;
  if (!(scale > 0.f) || !(scale < 1e30f)) return VSYS_ERR_ARG;   // the running maximum is taken on the unscaled logits
  if ((ldq % 8) || (ldk % 8) || (ldv % 8) || (ldo % 8) || (Lp % 8)) return VSYS_ERR_ALIGN;
  if (((uintptr_t)q & 15) || ((uintptr_t)k & 15) || ((uintptr_t)vt & 15) || ((uintptr_t)o & 15)) return VSYS_ERR_ALIGN;
  // one key block behind one descriptor: 32 K rows, C V^T rows (the descriptor is re-based per frame and block)
  if (31 * ldk * 2 + C * 2 > 0x7fffffff || (C - 1) * ldv * 2 + 64 > 0x7fffffff) return VSYS_ERR_SHAPE;
  const int64_t units = n * ((L + QR - 1) / QR);
  if (units > 0x7fffffff) return VSYS_ERR_SHAPE;
  const float sl2 = scale * LOG2E;
  if (C == 128) return vf_launch<1>(q, ldq, k, ldk, vt, ldv, o, ldo, units, (int)L, (int)Lp, sl2, stream);
  if (C == 256) return vf_launch<2>(q, ldq, k, ldk, vt, ldv, o, ldo, units, (int)L, (int)Lp, sl2, stream);
  return vf_launch<4>(q, ldq, k, ldk, vt, ldv, o, ldo, units, (int)L, (int)Lp, sl2, stream);
}

}  // namespace vsys
