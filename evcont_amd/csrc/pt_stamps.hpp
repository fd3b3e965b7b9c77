// Timing experiments (tools/micro/pt_stamps.py; build with EVC_DEBUG_STAMPS=1): the four waves of one workgroup in the
// middle of the grid stamp their phases with the 100 MHz wall clock.  Compiled out of the product library.
// Device code is not relocatable, so every unit that includes this header (pair_transform.hip, pair_pipe.hip) has its own
// copy of the two symbols and its own reader: evc_debug_read_pt_phase[_wg] and evc_debug_read_pt[_wg].
#pragma once
#include "common.hpp"

#ifdef EVC_DEBUG_STAMPS
namespace evc {
static __device__ long long g_pt_stamp[4 * 64];
static __device__ long long g_pt_wg[4096 * 3];   // per workgroup: entry, exit, (XCC_ID << 8 | CU/SE id register)
}  // namespace evc
#define EVC_PT_WG(i_)                                                                                          \
    do {                                                                                                       \
        const int L_ = blockIdx.y * gridDim.x + blockIdx.x;                                                    \
        if (threadIdx.x == 0 && L_ < 4096) {                                                                   \
            g_pt_wg[3 * L_ + (i_)] = wall_clock64();                                                           \
            if ((i_) == 0) {                                                                                   \
                unsigned hw_, xcc_;                                                                            \
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_));                              \
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));                            \
                g_pt_wg[3 * L_ + 2] = ((long long)(xcc_ & 0xF) << 32) | hw_;                                   \
            }                                                                                                  \
        }                                                                                                      \
    } while (0)
#define EVC_PT_STAMP(i_)                                                                                       \
    do {                                                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        long long t_;                                                                                          \
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                         \
        if (blockIdx.x == gridDim.x / 2 && blockIdx.y == gridDim.y / 2 && (threadIdx.x & 63) == 0 && (i_) < 64) \
            g_pt_stamp[(threadIdx.x >> 6) * 64 + (i_)] = t_;                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
    } while (0)
// the including unit's readers of its copies: 4 waves x 64 stamps of the last launch, and the workgroup records
#define EVC_PT_STAMP_READERS(read_, read_wg_)                                                                  \
    extern "C" int read_(long long *stamps) {                                                                  \
        return (int)hipMemcpyFromSymbol(stamps, HIP_SYMBOL(evc::g_pt_stamp), sizeof(long long) * 4 * 64);      \
    }                                                                                                          \
    extern "C" int read_wg_(long long *stamps) {                                                               \
        return (int)hipMemcpyFromSymbol(stamps, HIP_SYMBOL(evc::g_pt_wg), sizeof(long long) * 4096 * 3);       \
    }
#else
#define EVC_PT_STAMP(i_) do { } while (0)
#define EVC_PT_WG(i_) do { } while (0)
#define EVC_PT_STAMP_READERS(read_, read_wg_)
#endif
