// The small device pieces the pair kernels share (pair_transform.hip, pair_pipe.hip, y2.hip, pair_dma.hip, pair64.hip):
// the operand-row window of the dense (pair, pair) forms, the diagonal test of a pair index and the padding of the packed
// result.  All are inlined: hoisting them here left every kernel of those units instruction for instruction as it was.
// What stays INLINE in the kernels: the fragment-offset table foff[rt][kk] = tri(max(r,s), min(r,s)), the stage
// addresses fa / sa and the X-fragment load xf[kk][t].  Through an array-reference helper all 8 pt_pipe* instantiations
// came out different (pt_pipe_kernel<32,0> 188 -> 202 VGPRs, <32,1> 206 -> 214), through a scalar-returning helper inside
// the existing loops still all 8 (offsets) or 4 (X fragments): hand-scheduled code nobody has measured in that form.
// Likewise in pair_dma.hip (fa, X fragments, zero slots, walker) and for the Y2 kernels' cross-wave sum: DESIGN.md 4.5.
#pragma once
#include "common.hpp"

namespace evc {

// One packed symmetric row (npairs doubles at `row`, 8-byte aligned) through a 16-byte aligned window: lane i holds the
// doubles 128 u + 2 i, + 1 of the window that starts `shift` (0 / 1, returned) doubles before the row.
// Every lane loads an aligned 16-byte granule that holds at least one double of the row (lanes past the end re-read the
// first granule): no predicates, and such a load cannot leave the pages of the operand.
template <int RAWN>
__device__ __forceinline__ int fetch_packed_row(const double *row, int npairs, int lane, d2 (&raw)[RAWN]) {
    const int d_ = (int)((reinterpret_cast<uintptr_t>(row) >> 3) & 1);
    const double *w0 = row - d_;          // 16-byte aligned window
    const int lim = npairs + d_;          // valid doubles of the window
#pragma unroll
    for (int u = 0; u < RAWN; ++u) {
        const int j = 128 * u + 2 * lane;
        raw[u] = *reinterpret_cast<const d2 *>(w0 + (j < lim ? j : 0));
    }
    return d_;
}
// ... and into the wave's LDS row: element k of the row sits at lds_row[k + shift]
template <int RAWN>
__device__ __forceinline__ void park_packed_row(double *lds_row, int lane, const d2 (&raw)[RAWN]) {
#pragma unroll
    for (int u = 0; u < RAWN; ++u) *reinterpret_cast<d2 *>(lds_row + 128 * u + 2 * lane) = raw[u];
}

// pair x = tri(r, s) is on the diagonal r == s (x < 2^20)
__device__ __forceinline__ bool tri_is_diag(int x) {
    const int r = tri_row_small(x);
    return x == r * (r + 3) / 2;
}

// zero the padding [M, packed_len) of a packed result (a workgroup of 256 threads)
__device__ __forceinline__ void zero_packed_tail(double *pk, int64_t M, int64_t packed_len) {
    for (int64_t m = M + threadIdx.x; m < packed_len; m += 256) pk[m] = 0.0;
}

}  // namespace evc
