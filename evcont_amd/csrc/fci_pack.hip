// Packed epilogue of the full-CI row call (evc_fci_trdm_rows_packed, fci.hip): the dense two-body t-RDM of one ket,
// dm2[p,q,r,s] (N^4 doubles, written into a slot of the workspace by fci_trdm_reduce2_kernel), goes into one row of the
// (pairs, ld) matrix the evaluator streams, in the layout it reads:
//   EVC_LAYOUT_PACK2   column R(R+1)/2 + C, R = pN+q >= C = rN+s:                     dm2[p,q,r,s]
//   EVC_LAYOUT_SYM8    column u(u+1)/2 + v, u = i(i+1)/2+j (i >= j), v = k(k+1)/2+l (k >= l), u >= v:
//                      0.125 * (((((((d0+d1)+d2)+d3)+d4)+d5)+d6)+d7), d_m = dm2 at the images
//                      (i,j,k,l) (j,i,k,l) (i,j,l,k) (j,i,l,k) (k,l,i,j) (l,k,i,j) (k,l,j,i) (l,k,j,i)
//                      -- the order of evaluator.sym8_column_images and the arithmetic of DeviceTRDMs.compress_sym8_ on a
//                      six-index source, so a row written here has the bits of a row compressed there.
// Columns cols ... ld - 1 of the row are written as zeros.
// One thread per output column; blockIdx.y is the leading index (R or u) and the threads run over the trailing one, so
// a block's stores are consecutive and (i, j) is block-uniform; (k, l) comes from fifteen compares at most, no square
// root.  The gathers read the slot (0.5 MB at sixteen orbitals, resident in L2), never the per-block partials.  A VALU /
// memory kernel in a launch of its own (FP64 MFMA blocks its SIMD's vector issue).
#include "common.hpp"
#include "kernels.hpp"

namespace evc {

// Launch through the runtime call (not the chevrons): tests/test_fci_pack_closure.py keeps the list of the kernels this
// file launches against the record of EVC_PROF_FCI_PACK.
template <typename T>
struct pack_same_type {
    using type = T;
};
template <typename... P>
static void pack_launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t st,
                        typename pack_same_type<P>::type... a) {
    void *args[] = {(void *)&a...};
    // the result is read by the EVC_LAUNCH_CHECK (hipGetLastError) that follows the call
    (void)hipLaunchKernel(reinterpret_cast<const void *>(kernel), grid, block, args, 0, st);
}

// IMAGES 1: nu = N^2 leading indices (pack2); IMAGES 8: nu = N(N+1)/2 (sym8).  blockIdx.y < nu: columns
// tri(u, v), v <= u; blockIdx.y == nu: the pad columns cols ... ld - 1.
template <int IMAGES>
__global__ __launch_bounds__(256) void fci_row_pack_kernel(const double *__restrict__ dm2, int norb, int nu,
                                                           int64_t cols, int64_t ld, double *__restrict__ row) {
    const int u = blockIdx.y, v = blockIdx.x * 256 + threadIdx.x;
    if (u == nu) {
        if (cols + v < ld) row[cols + v] = 0.0;
        return;
    }
    if (v > u) return;
    const int n2 = norb * norb;
    double out;
    if (IMAGES == 1) {
        out = dm2[u * n2 + v];
    } else {
        int i = 0, k = 0;
        for (int t = 1; t < norb; ++t) {
            const int first = t * (t + 1) / 2;   // the first pair index of leading orbital t
            i += u >= first;
            k += v >= first;
        }
        const int j = u - i * (i + 1) / 2, l = v - k * (k + 1) / 2;
        const int ij = i * norb + j, ji = j * norb + i, kl = k * norb + l, lk = l * norb + k;
        double acc = dm2[ij * n2 + kl];
        acc += dm2[ji * n2 + kl];
        acc += dm2[ij * n2 + lk];
        acc += dm2[ji * n2 + lk];
        acc += dm2[kl * n2 + ij];
        acc += dm2[lk * n2 + ij];
        acc += dm2[kl * n2 + ji];
        acc += dm2[lk * n2 + ji];
        out = acc * 0.125;
    }
    row[(int64_t)u * (u + 1) / 2 + v] = out;
}

int64_t fci_row_pack_cols(int layout, int norb) {
    const int64_t n2 = (int64_t)norb * norb, ms = (int64_t)norb * (norb + 1) / 2;
    return layout == EVC_LAYOUT_SYM8 ? ms * (ms + 1) / 2 : n2 * (n2 + 1) / 2;
}

int launch_fci_row_pack(int layout, int norb, const double *dm2, double *row, int64_t ld, hipStream_t st) {
    const int64_t cols = fci_row_pack_cols(layout, norb);
    const int nu = layout == EVC_LAYOUT_SYM8 ? norb * (norb + 1) / 2 : norb * norb;
    const int64_t widest = ld - cols > nu ? ld - cols : nu;
    const dim3 grid((unsigned)ceil_div(widest, 256), (unsigned)nu + 1), block(256);
    if (layout == EVC_LAYOUT_SYM8)
        pack_launch(fci_row_pack_kernel<8>, grid, block, st, dm2, norb, nu, cols, ld, row);
    else
        pack_launch(fci_row_pack_kernel<1>, grid, block, st, dm2, norb, nu, cols, ld, row);
    EVC_LAUNCH_CHECK("fci_row_pack_kernel");
    return 0;
}

void note_fci_row_pack(int layout, int norb, int nrows, int64_t ld) {
    note_kernel(EVC_PROF_FCI_PACK, "fci_row_pack_kernel<%d> rows=%d cols=%lld ld=%lld", layout == EVC_LAYOUT_SYM8 ? 8 : 1,
                nrows, (long long)fci_row_pack_cols(layout, norb), (long long)ld);
}

}  // namespace evc
