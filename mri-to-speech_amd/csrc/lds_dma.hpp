// Device primitives of the kernels that fill LDS by DMA (global_load_lds_dwordx4) and wait for it with counted
// `s_waitcnt vmcnt`s: the two DMA forms, the waits, the zero page, LDS addresses, LDS reads that wait only for
// themselves, the block-scaled-MFMA operand types and the 128-byte-row swizzles.  Device-only: included by .hip
// files, every definition has internal linkage (one copy per translation unit, as when each kernel had its own).
#pragma once

#include "m2s_common.hpp"

namespace m2s {
namespace {

// ---- LDS-DMA: 16 bytes per lane, lane i of the wave lands at lds_wave_base + 16 i ------------------------------
// Two forms, not overloads, because the compiler treats them differently:
//  * dma16, the builtin.  hipcc counts it in its own vmcnt bookkeeping and, since it cannot tell which LDS bytes
//    it writes, puts a conservative s_waitcnt vmcnt(0) before the next ordinary LDS read of the wave.  Right where
//    the wave's next LDS read wants that DMA anyway, or is made through lds_u2 / lds_f4 below.
//  * dma16_asm, the same instruction in inline asm (m0 saved, set to the LDS address, restored).  hipcc neither
//    sees nor counts it, so it drains nothing before the wave's own LDS reads (with the builtin a producer wave
//    waited for its newest DMA at every slice); completion is entirely the caller's wait_vm.  The LDS address
//    must be wave-uniform (an SGPR): lds_off_u / lds_lo32_u.
__device__ __forceinline__ void dma16(const void* src, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(src, lds_wave_base, 16, 0, 0);
}
__device__ __forceinline__ void dma16_asm(const void* src, uint32_t lds_wave_base) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(src), "s"(lds_wave_base)
               : "memory");
}

template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// vmcnt(n) for a wave-uniform n the immediate cannot take: the nearest count <= n (waiting for more is safe)
__device__ __forceinline__ void wait_vm_le(int n) {
  if (n >= 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if (n == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
  else if (n == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if (n == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
  else if (n == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else if (n == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- the zero page: 64 zero bytes, the DMA source of padding lanes -------------------------------------------
__device__ __attribute__((aligned(16))) uint4 g_zero_page[4];
// Its address, pinned in SGPRs; call once at the top of a kernel and use the result in the DMA loops.  Named
// directly in those loops, the address was re-fetched from the GOT (s_getpc + s_load + s_waitcnt lgkmcnt(0), which
// also drains the wave's LDS reads) at every piece.
__device__ __forceinline__ const char* zero_page() {
  const char* zp = reinterpret_cast<const char*>(g_zero_page);
  asm volatile("" : "+s"(zp));
  return zp;
}

// ---- LDS byte address of a pointer into LDS: per lane, and wave-uniform (_u: an SGPR, for dma16_asm's m0) -----
// Two spellings of the same number.  lds_off casts the generic pointer to the LDS address space, which the compiler
// lowers to `p ? low 32 bits : -1` (a compare and a select on the null pointer) unless it has folded the pointer to
// smem + constant; lds_lo32 just truncates.  Each kernel keeps the spelling it was tuned and measured with: the
// other one changes its scalar code and, in the ring kernels, its SGPR spill count, and which is
// faster where has not been measured.
__device__ __forceinline__ uint32_t lds_off(const void* p) {
  return (uint32_t)(size_t)(const __attribute__((address_space(3))) char*)p;
}
__device__ __forceinline__ uint32_t lds_lo32(const void* p) { return (uint32_t)(uintptr_t)p; }
__device__ __forceinline__ uint32_t lds_off_u(const void* p) { return __builtin_amdgcn_readfirstlane(lds_off(p)); }
__device__ __forceinline__ uint32_t lds_lo32_u(const void* p) { return __builtin_amdgcn_readfirstlane(lds_lo32(p)); }

// LDS reads the compiler does not see: an ordinary ds_read after a dma16 gets the conservative vmcnt(0) above, which
// would also wait for the ring's prefetch and the tile's stores.  These wait only for themselves.
__device__ __forceinline__ uint2 lds_u2(const void* p) {
  uint2 r;
  asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(r) : "v"(lds_off(p)));
  return r;
}
__device__ __forceinline__ float4 lds_f4(const void* p) {
  float4 r;
  asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(r) : "v"(lds_off(p)));
  return r;
}

// ---- v_mfma_scale_f32_16x16x128_f8f6f4 operands: 32 e4m3 bytes per lane, unit E8M0 block scales ---------------
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int E8M0_ONE = 0x7f7f7f7f;  // 2^0 block scale in every byte
__device__ __forceinline__ i32x8 cat8(u32x4 a, u32x4 b) {
  return i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
}
// 4 e4m3 (one dword) x 4 gates -> 4 e4m3 (the gate is in (0, 1): no new saturation)
__device__ __forceinline__ int gate4(int d, const float* s) {
  const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8(d, false);
  const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8(d, true);
  const int r = __builtin_amdgcn_cvt_pk_fp8_f32(lo[0] * s[0], lo[1] * s[1], 0, false);
  return __builtin_amdgcn_cvt_pk_fp8_f32(hi[0] * s[2], hi[1] * s[3], r, true);
}

// ---- 128-byte LDS rows ----------------------------------------------------------------------------------------
// Physical 16-byte chunk of logical chunk c in row r: c ^ f(r), f(r) = ((r >> 1) & 1) | (r & 4).  A
// fragment is two ds_read_b128 (lane (g = lane >> 4, r = lane & 15) reads chunks 2g and 2g + 1 of row r);
// with 128-byte rows a row pair spans the 64 banks, and this f puts the 16 lanes of each of ds_read_b128's
// lane groups ({0-3,12-15,20-27}, {4-11,16-19,28-31}, ...; MI355X_MICROARCH.md LDS table) on 16 distinct
// 16-byte bank quads for both reads (exhaustive check over the XOR swizzles of the row's low 4 bits).
__device__ __forceinline__ int f8_swz(int r) { return ((r >> 1) & 1) | (r & 4); }
// SP (split rows, 32 channels [hi 32 | lo 32] bf16): a fragment reads chunks g (hi) and g + 4 (lo); f(r) = r & 6 is
// conflict-free for that pair (same check)
template <bool SP>
__device__ __forceinline__ int swz128(int r) { return SP ? (r & 6) : f8_swz(r); }
// 64-byte rows (32 bf16, four chunks).  Physical chunk of logical chunk c in row r: c ^ f((r >> 2) & 3) with
// f = [0, 2, 3, 1].  A fragment read (lane = (g = lane >> 4, r16 = lane & 15): row r16, chunk g) is then
// conflict-free for ds_read_b128's lane groups on gfx950 (the groups above): within each group the four lanes that
// share (r16 & 3) land in four different 16-byte bank slots.  (The plain c ^ ((r >> 2) & 3) put lanes 0-3 and 20-23
// on the same slots: 2-way conflicts, SQ LDS_BANK_CONFLICT ~3x the LDS-active cycles.)
__device__ __forceinline__ int swz_f(int x) { return (0x1320 >> (4 * x)) & 3; }

}  // namespace
}  // namespace m2s
