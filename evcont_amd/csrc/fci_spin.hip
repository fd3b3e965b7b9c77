// S^2 on CI vectors that stay on the device, for a spin penalty shift (S^2 - S(S+1)) on the operator an eigensolver sees
// (fci_device.py: DeviceFCI(spin_penalty=...)) and for <S^2> of a state.  With c[Ia][Ib], Sz = (n_alpha - n_beta) / 2 and
// the string tables tab[I][p N + q] = +-(J + 1) for <I| a_p^+ a_q |J> = +-1:
//   (S^2 c)[Ia, Ib] = k c[Ia, Ib] - sum_pq sgn_a sgn_b c[Ja, Jb],   k = Sz (Sz + 1) + n_beta,
//                     Ja, sgn_a from tab_a[Ia][p N + q], Jb, sgn_b from tab_b[Ib][q N + p]
//   <I|S^2|I>       = k - popcount(occ(Ia) & occ(Ib))
//   apply   out = beta out + alpha (S^2 c - ss c): a workgroup owns 64 beta strings, whose table rows it stages once in
//           LDS, string-minor (the [Ib][pq] rows of the global table become [pq][Ib]: the lanes of a wave, one beta string
//           each, read consecutive entries), and walks a run of alpha strings, one per wave at a time.  The alpha row is
//           wave-uniform: it is read through scalar loads and its zeros (N^2 - n_alpha (N - n_alpha + 1) of N^2) are
//           skipped by a uniform branch; the beta entry of the transposed pair is one LDS read at a uniform row.
//   diag    hdiag[I] += alpha (<I|S^2|I> - ss), one thread per determinant
// One pass, FP64 vector code, no atomics, no workspace.  Every element is one sum in a fixed order: (k - ss) c first, the
// pairs pq ascending, then alpha times the sum, then + beta out, each step rounded on its own (no contraction): the same
// bits from run to run and for every launch shape; fci_tables.spin_square_through_tables states it in numpy.
#include "common.hpp"
#include "kernels.hpp"

namespace evc {

constexpr int kSpinTile = 64;                 // beta strings per workgroup: one per lane
constexpr int kSpinPitch = kSpinTile + 2;     // int16 entries per staged pair: 33 dwords, an odd pitch, so that the staging
                                              // stores of 64 consecutive pairs of one string fall into 32 different banks
constexpr int kSpinMaxRun = 64;               // alpha strings per workgroup, at most (a multiple of the 4 waves)

// Launch through the runtime call (not the chevrons), as solve_launch does: tests/test_fci_spin_closure.py keeps the list
// of the kernels this file launches against the records of EVC_PROF_FCI_SOLVE.
template <typename T>
struct spin_same_type {
    using type = T;
};
template <typename... P>
static void spin_launch(void (*kernel)(P...), dim3 grid, size_t lds, hipStream_t st, typename spin_same_type<P>::type... a) {
    void *args[] = {(void *)&a...};
    (void)hipLaunchKernel(reinterpret_cast<const void *>(kernel), grid, dim3(256), args, lds, st);
}

// k - ss, k = Sz (Sz + 1) + n_beta: the electron numbers are the occupied orbitals of the first string of each table
// (orbital p is occupied iff E_pp keeps the string, as fci_hdiag_string_kernel reads it); the same loads in every thread.
__device__ __forceinline__ double spin_kms(int norb, const int32_t *__restrict__ tab_a, const int32_t *__restrict__ tab_b,
                                           double ss) {
    int nal = 0, nbe = 0;
    for (int p = 0; p < norb; ++p) {
        nal += tab_a[p * norb + p] != 0;
        nbe += tab_b[p * norb + p] != 0;
    }
    const double sz = 0.5 * (double)(nal - nbe);
    return (sz * (sz + 1.0) + (double)nbe) - ss;
}

// blockIdx = (tile of 64 beta strings, run of `run` alpha strings).  |J + 1| <= 12870 fits the int16 of the staged rows.
__global__ __launch_bounds__(256) void fci_spin_apply_kernel(int norb, int npad, int64_t na, int64_t nb, int run,
                                                             const int32_t *__restrict__ tab_a,
                                                             const int32_t *__restrict__ tab_b,
                                                             const double *__restrict__ c, double alpha, double ss,
                                                             double beta, double *__restrict__ out) {
#pragma clang fp contract(off)
    extern __shared__ int16_t spin_rows[];    // [pq][kSpinPitch]
    const double kms = spin_kms(norb, tab_a, tab_b, ss);
    const int n2 = norb * norb;
    const int64_t ib0 = (int64_t)blockIdx.x * kSpinTile;
    // stage: consecutive threads read consecutive pairs of one string (coalesced) and store them kSpinPitch apart
    for (int e = threadIdx.x; e < n2 * kSpinTile; e += 256) {
        const int r = e / n2, pq = e - r * n2;
        const int64_t ib = ib0 + r;
        spin_rows[pq * kSpinPitch + r] = ib < nb ? (int16_t)tab_b[ib * npad + pq] : (int16_t)0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t ib = ib0 + lane;
    const int64_t ia0 = (int64_t)blockIdx.y * run;
    const int64_t ia1 = ia0 + run < na ? ia0 + run : na;
    if (ib >= nb) return;
    for (int64_t ia = ia0 + wave; ia < ia1; ia += 4) {
        const int32_t *__restrict__ row = tab_a + ia * npad;
        double t = kms * c[ia * nb + ib];
        for (int p = 0; p < norb; ++p)
            for (int q = 0; q < norb; ++q) {
                const int32_t a = row[p * norb + q];
                if (a == 0) continue;                                   // wave-uniform
                const int b = spin_rows[(q * norb + p) * kSpinPitch + lane];
                if (b == 0) continue;
                const double v = c[(int64_t)((a < 0 ? -a : a) - 1) * nb + ((b < 0 ? -b : b) - 1)];
                t = ((a ^ b) < 0) ? t + v : t - v;
            }
        double r = alpha * t;
        if (beta != 0.0) r = beta * out[ia * nb + ib] + r;
        out[ia * nb + ib] = r;
    }
}

// One thread per determinant; orbital p is occupied in a string iff E_pp keeps it (as fci_hdiag_string_kernel reads it).
__global__ __launch_bounds__(256) void fci_spin_diag_kernel(int norb, int npad, int64_t na, int64_t nb,
                                                            const int32_t *__restrict__ tab_a,
                                                            const int32_t *__restrict__ tab_b, double alpha, double ss,
                                                            double *__restrict__ hdiag) {
#pragma clang fp contract(off)
    const double kms = spin_kms(norb, tab_a, tab_b, ss);
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= na * nb) return;
    const int32_t *__restrict__ ra = tab_a + (k / nb) * npad, *__restrict__ rb = tab_b + (k % nb) * npad;
    int both = 0;
    for (int p = 0; p < norb; ++p)
        if (ra[p * norb + p] != 0 && rb[p * norb + p] != 0) ++both;
    hdiag[k] = hdiag[k] + alpha * (kms - (double)both);
}

static int spin_shape(const char *who, int norb, int64_t na, int64_t nb) {
    EVC_REQUIRE(norb >= 1 && norb <= kFciMaxOrb, "%s: norb=%d, supported 1 ... %d", who, norb, kFciMaxOrb);
    EVC_REQUIRE(na >= 1 && nb >= 1 && na <= 12870 && nb <= 12870, "%s: na=%lld nb=%lld strings (1 ... 12870 each)", who,
                (long long)na, (long long)nb);
    return 0;
}

}  // namespace evc

using namespace evc;

extern "C" int evc_fci_spin_apply(int norb, int64_t na, int64_t nb, const int32_t *tab_a, const int32_t *tab_b,
                                  const double *c, double alpha, double ss, double beta, double *out, void *stream) {
    if (int rc = spin_shape("evc_fci_spin_apply", norb, na, nb)) return rc;
    EVC_REQUIRE(tab_a && tab_b && c && out, "evc_fci_spin_apply: null pointer");
    const int64_t dim = na * nb;
    EVC_REQUIRE(!(c < out + dim && out < c + dim), "evc_fci_spin_apply: out must not alias c");
    hipStream_t st = as_stream(stream);
    note_kernel(EVC_PROF_FCI_SOLVE, "%s", "");
    const int npad = (norb * norb + 15) / 16 * 16;
    const int64_t tiles_b = ceil_div(nb, kSpinTile);
    // alpha strings per workgroup: enough workgroups for the device at small shapes, the staging amortised at large ones
    int64_t run = 4 * ceil_div(na * tiles_b, 4 * 1024);
    run = run > kSpinMaxRun ? kSpinMaxRun : run;
    const int64_t runs = ceil_div(na, run);
    const size_t lds = (size_t)norb * norb * kSpinPitch * sizeof(int16_t);
    spin_launch(fci_spin_apply_kernel, dim3((unsigned)tiles_b, (unsigned)runs), lds, st, norb, npad, na, nb, (int)run, tab_a,
                tab_b, c, alpha, ss, beta, out);
    EVC_LAUNCH_CHECK("fci_spin_apply_kernel");
    note_kernel(EVC_PROF_FCI_SOLVE, "fci_spin_apply_kernel beta=%d tiles=%lld", beta != 0.0 ? 1 : 0,
                (long long)(tiles_b * runs));
    return 0;
}

extern "C" int evc_fci_spin_diag(int norb, int64_t na, int64_t nb, const int32_t *tab_a, const int32_t *tab_b, double alpha,
                                 double ss, double *hdiag, void *stream) {
    if (int rc = spin_shape("evc_fci_spin_diag", norb, na, nb)) return rc;
    EVC_REQUIRE(tab_a && tab_b && hdiag, "evc_fci_spin_diag: null pointer");
    hipStream_t st = as_stream(stream);
    note_kernel(EVC_PROF_FCI_SOLVE, "%s", "");
    const int npad = (norb * norb + 15) / 16 * 16;
    spin_launch(fci_spin_diag_kernel, dim3((unsigned)ceil_div(na * nb, 256)), (size_t)0, st, norb, npad, na, nb, tab_a, tab_b,
                alpha, ss, hdiag);
    EVC_LAUNCH_CHECK("fci_spin_diag_kernel");
    note_kernel(EVC_PROF_FCI_SOLVE, "fci_spin_diag_kernel");
    return 0;
}
