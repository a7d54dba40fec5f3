// The C++ around the generated 64-rows-per-wave flash statements that flash_attn_d72_w64_kernel, flash_attn_d72_w64p_kernel
// (attention_w64.hip) and flash_attn_d64_w64_kernel (attention64_w64.hip) share: buffer descriptors, the fragment addressing inside a
// stage, the row bound of the statements without a running max, the launch.  The register map (where Q goes, where O comes from,
// the operand names of the statements) is the generator's: csrc/gen/flash72_gen.py writes it into flash72_w64_map.inc as
// <F>_WRITE_Q_<blk>, <F>_READ_O_<blk> and <F>_OPERANDS; nothing here or in the kernels names an accumulation register.
//
// What is NOT here, and why: the LDS-DMA lane addressing, the d72 RMS-norm Q fragments, the zero fill of the Vt padding and the O
// store stand in each kernel.  hipcc simplifies an inline function before it inlines it, so a piece that shares subexpressions or
// branch conditions with its surroundings (lane bit fields, qs < q_len) reaches the scheduler in another order as a function than
// as part of the kernel body, and the kernels' instruction streams were to stay as they are.  Each helper below was kept because
// the streams of all its callers did not change (tools/isa_same.py, profiles/w64_share_isa.json); compare again after touching one.
#pragma once
#include "common.h"
#include "vsys_internal.h"

#include "flash72_w64_asm.inc"
#include "flash72_w64_map.inc"

namespace vsys {
namespace w64 {

constexpr int VROW = 128, STAGES = 4;   // bytes of a row of a stage's Vt image (64 keys); stages of the K / Vt ring

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// wave-uniform buffer descriptor over [base, base + bytes)
__device__ __forceinline__ u32x4 make_rsrc(const void* base, unsigned bytes) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(base);
  u32x4 r;
  r.x = __builtin_amdgcn_readfirstlane((unsigned)a);
  r.y = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32) & 0xffffu);
  r.z = __builtin_amdgcn_readfirstlane(bytes);
  r.w = 0x00020000u;
  return r;
}

// Where a lane reads its fragments inside a stage (K tile of K_TILE_BYTES, then the Vt image).
// K: MFMA row i <-> key such that a lane's 16 accumulators are 16 consecutive keys
__device__ __forceinline__ int frag_krow(int l31) { return 16 * ((l31 >> 2) & 1) + 4 * (l31 >> 3) + (l31 & 3); }

struct VtFrag {
  int vfa0, vfa1, vfa2, vfa3;   // (operand names)
};

template <int K_TILE_BYTES>
__device__ __forceinline__ VtFrag vt_frag(int l31, int hi) {
  const int v_roff = K_TILE_BYTES + l31 * VROW + (((2 * hi) ^ ((l31 >> 1) & 7)) << 4);
  return {v_roff ^ (0 << 4), v_roff ^ (1 << 4), v_roff ^ (4 << 4), v_roff ^ (5 << 4)};
}

// LDS address of the dynamic shared memory
__device__ __forceinline__ int lds_base(char* smem) { return (int)(unsigned)(unsigned long long)(__attribute__((address_space(3))) char*)smem; }

// the statements without the running max: -(row bound) of this lane's query row, |q| k_bound (1 + 2^-6); the row is split over the
// lane pair (l, l + 32)
template <int NCC>
__device__ __forceinline__ float neg_row_bound(const float (&x)[NCC][8], float k_bound) {
  float qn2 = 0.f;
#pragma unroll
  for (int c = 0; c < NCC; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e) qn2 += x[c][e] * x[c][e];
  qn2 += __shfl_xor(qn2, 32, 64);
  return -(sqrtf(qn2) * k_bound * 1.015625f);
}

// raise KERNEL's dynamic LDS limit once per device, launch nblk workgroups of 256
template <auto KERNEL, class... Args>
int launch(unsigned nblk, size_t lds, hipStream_t stream, Args... args) {
  static std::atomic<unsigned long long> attr_seen{0};
  for (DeviceOnce once(attr_seen); once.todo(); once.done())
    (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(KERNEL, dim3(nblk), dim3(256), lds, stream, args...);
  return hipGetLastError() == hipSuccess ? 0 : VSYS_ERR_LAUNCH;
}

}  // namespace w64
}  // namespace vsys
