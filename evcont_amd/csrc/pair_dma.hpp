// The device pieces of the LDS-DMA pair steps (ptd_body, y2d_kernel<0> of pair_dma.hip): stores and LDS accesses at
// addresses the compiler shall leave alone and the request of one operand row.  All inlined.  What else the two
// prologues have in common stays INLINE in both -- the fa table, the X fragments, the zero slots, the (p, q) walker, the
// [4][32][33] reduction (y2_fused_kernel's third copy too): each hoist changed the machine code of at least one of its
// users (tools/isa_diff.py; the figures are in DESIGN.md 4.5).
#pragma once
#include "common.hpp"
#include "lds_dma.hpp"
#include "pair_plan.hpp"
#include "pair_rows.hpp"

namespace evc {

// 16-byte store, scalar base + 32-bit lane offset (the compiler forms a 64-bit vector address for the same C++)
__device__ __forceinline__ void gstore16(unsigned voff, d2 v, const void *sbase) {
    asm volatile("global_store_dwordx4 %0, %1, %2" : : "v"(voff), "v"(v), "s"(sbase) : "memory");
}
// an address the compiler shall not take apart (it folds constants out of it and leaves `v_add_u32 v, 0, v` behind)
__device__ __forceinline__ unsigned opaque(unsigned x) {
    asm volatile("" : "+v"(x));
    return x;
}
// LDS accesses at integer byte addresses (through the `lds` array the compiler adds the array's base -- the literal 0 --
// with a vector instruction per access in some of the unrolled phases)
typedef __attribute__((address_space(3))) double lds_f64;
typedef __attribute__((address_space(3))) float lds_f32;
typedef float f2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) f2 lds_f2;
typedef __attribute__((address_space(3))) d2 lds_d2;
__device__ __forceinline__ double lds_ld(unsigned addr) { return *(lds_f64 *)(uintptr_t)addr; }
__device__ __forceinline__ void lds_st(unsigned addr, double v) { *(lds_f64 *)(uintptr_t)addr = v; }
__device__ __forceinline__ d2 lds_ld2(unsigned addr) { return *(lds_d2 *)(uintptr_t)addr; }

// One operand row by LDS-DMA: `wbytes` bytes (a multiple of 16) from a 16-byte aligned `src` to the LDS address `dst`, in
// npieces (wave-uniform) pieces of 1 KiB, lanes past the end re-read the first granule.  A counted wait for an older
// row leaves `npieces` instructions per younger row in flight.
struct RowDma {
    unsigned vo[kPdRaw];
    int npieces;
    __device__ __forceinline__ RowDma(unsigned wbytes, int lane) {
#pragma unroll
        for (unsigned u = 0; u < kPdRaw; ++u) {
            const unsigned o = 1024u * u + 16u * (unsigned)lane;
            vo[u] = o < wbytes ? o : 0u;
        }
        npieces = __builtin_amdgcn_readfirstlane((int)((wbytes + 1023u) >> 10));
    }
    __device__ __forceinline__ void request(const void *src, unsigned dst) const {
#pragma unroll
        for (unsigned u = 0; u < kPdRaw; ++u)
            if ((int)u < npieces) glds_s(vo[u], src, dst + 1024u * u);
    }
};

}  // namespace evc
