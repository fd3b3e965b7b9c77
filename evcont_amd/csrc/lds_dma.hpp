// LDS-DMA (global_load_lds_dwordx4: global memory straight into LDS, no VGPRs in between) and its waits.  The only place
// that spells the instruction: K5 (gemv_lds.hip), K8 (gemv_cols_lds.hip) and the pair steps of pair_dma.hip (through pair_dma.hpp) include it.
#pragma once
#include "common.hpp"

namespace evc {

// 16 bytes per lane: LDS address = M0 + 16 * lane (M0 is written right in front of the load; the s_nop covers the
// hazard between a scalar write of M0 and the LDS-DMA that reads it).  The compiler neither counts these loads in its
// own s_waitcnt placement nor knows that they write LDS: every wait for one is explicit (below), and the "memory"
// clobbers keep the compiler's own LDS reads on their side of the load and of the wait.
// glds_s: scalar base + 32-bit lane offset; glds_v: a 64-bit address per lane.
__device__ __forceinline__ void glds_s(unsigned voff, const void *sbase, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
                 :
                 : "v"(voff), "s"(sbase), "s"(lds_addr)
                 : "memory");
}
__device__ __forceinline__ void glds_v(const void *vaddr, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(vaddr), "s"(lds_addr) : "memory");
}
// wave-uniform values the compiler's divergence analysis may not recognise as such (an "s" constraint alone does not
// move a VGPR value into an SGPR)
__device__ __forceinline__ unsigned uniform_u32(unsigned x) { return (unsigned)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ const void *uniform_ptr(const void *p) {
    const unsigned long long b = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = uniform_u32((unsigned)b), hi = uniform_u32((unsigned)(b >> 32));
    return reinterpret_cast<const void *>(((unsigned long long)hi << 32) | lo);
}

// Counted waits, two families that generate different code:
//   wait_vm<N> / wait_vm_n(n): the count is a compile-time constant, or becomes one when the loop around the call is
//     unrolled (the switch folds to one instruction) -- the K5 / K8 streams;
//   wait_vm_dyn(k) / wait_vm_dyn8(k): the count is a wave-uniform RUNTIME value (it depends on how many stores and
//     DMA pieces the wave has behind the row it waits for): a chain of scalar compares and one wait -- the pair steps.
template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" : : "n"(N) : "memory");
}
__device__ __forceinline__ void wait_vm_n(int n) {
#define EVC_VM_CASE(k) case k: wait_vm<k>(); break;
    switch (n) {
        EVC_VM_CASE(0) EVC_VM_CASE(2) EVC_VM_CASE(4) EVC_VM_CASE(6) EVC_VM_CASE(8) EVC_VM_CASE(10) EVC_VM_CASE(12)
        EVC_VM_CASE(14) EVC_VM_CASE(16) EVC_VM_CASE(18) EVC_VM_CASE(20) EVC_VM_CASE(22) EVC_VM_CASE(24)
        EVC_VM_CASE(26) EVC_VM_CASE(28) EVC_VM_CASE(30) EVC_VM_CASE(32) EVC_VM_CASE(34) EVC_VM_CASE(36)
        EVC_VM_CASE(38) EVC_VM_CASE(40) EVC_VM_CASE(42) EVC_VM_CASE(44) EVC_VM_CASE(46) EVC_VM_CASE(48)
        EVC_VM_CASE(50) EVC_VM_CASE(52) EVC_VM_CASE(54) EVC_VM_CASE(56) EVC_VM_CASE(58) EVC_VM_CASE(60)
        default: wait_vm<0>(); break;
    }
#undef EVC_VM_CASE
}
// k (0..3) wave-uniform
__device__ __forceinline__ void wait_vm_dyn(int k) {
    if (k <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (k == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else if (k == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
}
// the same for 0..8 (the pair step with Y2 has the DMA of a second row among the younger instructions)
__device__ __forceinline__ void wait_vm_dyn8(int k) {
    if (k <= 3) wait_vm_dyn(k);
    else if (k == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if (k == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if (k == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if (k == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
}
// the wave's own LDS reads have left LDS (the slot they read may be refilled)
__device__ __forceinline__ void wait_lds() { asm volatile("s_waitcnt lgkmcnt(0)" : : : "memory"); }

}  // namespace evc
