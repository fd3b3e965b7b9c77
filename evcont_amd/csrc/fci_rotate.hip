// Rotation of a CI vector under an orbital transformation u (PySCF's fci.addons.transform_ci, square u; the host
// statement is fci_small.transform_ci):
//   T[I, J] = det( u[occ(I)][:, occ(J)] )     per spin, strings ordered by integer value, k = electrons of the spin
//   out     = T_a^T . c . T_b                 c (na, nb)
//   minors    fci_minor_kernel<K>: one thread per element of a panel of T, a K x K determinant by LU with partial
//             pivoting, the matrix in registers, rows moved by select.  K = 1 ... 8; for k >= 9 Jacobi's identity
//             det(u[I, J]) = det(u) (-1)^(sum I + sum J) det((u^-1)[J^c, I^c]) turns the minor into one of order
//             norb - k <= 7 of w = (u^-1)^T, which the entry point forms on the host.
//   products  fci_rotate_gemm_kernel: C = op(A) . B on the FP64 matrix cores, any m, n, k, tails predicated; used for
//             M = c . T_b and out = T_a^T . M.
// Minors (VALU) and products (MFMA) are separate launches (FP64 MFMA blocks its SIMD's vector issue).
// u is a HOST argument and reaches the minor kernel by value, as a kernel argument: a wave works on one row I, so the
// rows of u it needs and every element it reads are wave-uniform.
// T is formed in panels of its columns (the new strings J', I'), whose width depends on the shape alone; a panel cuts
// the output index of a product, never a sum, so every workspace gives the same bits.
// evc_fci_rotate_block rotates several vectors under one u: each panel of T is formed once and the product launches
// take the vectors in their grid's z, every vector through the arithmetic of the single call.
#include <math.h>

#include "common.hpp"
#include "kernels.hpp"

namespace evc {

constexpr int kRotMaxMinor = 8;             // largest instantiated determinant
constexpr int64_t kRotPanelDoubles = 1 << 19;   // a panel of T holds about this many doubles (4 MiB)
constexpr int kRotVecs = 16;                // vectors one product launch takes (its grid's z)

struct RotU {
    double v[kFciMaxOrb * kFciMaxOrb];      // row-major (norb, norb)
};

// Launch through the runtime call (not the chevrons): tests/test_fci_rotate_closure.py keeps the list of the kernels
// this file launches against the record of EVC_PROF_FCI_ROTATE.
template <typename T>
struct rot_same_type {
    using type = T;
};
template <typename... P>
static void rotate_launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t st,
                          typename rot_same_type<P>::type... a) {
    void *args[] = {(void *)&a...};
    // the result is read by the EVC_LAUNCH_CHECK (hipGetLastError) that follows every call, as after solve_launch
    (void)hipLaunchKernel(reinterpret_cast<const void *>(kernel), grid, block, args, 0, st);
}

// ---- minors ----------------------------------------------------------------------
// T[i * ld + (j - j0)] = scale * sgn * det( w[rows(i)][:, cols(j)] ), j0 <= j < j0 + width, i = blockIdx.y:
// rows(i) = the set bits of strs_r[i] ^ flip, cols(j) those of strs_c[j] ^ flip (flip = 0: the strings themselves,
// flip = all orbitals: their complements), sgn = (-1)^(sum of the orbitals of both strings) when `parity` is set.
// The matrix is gathered orbital by orbital: w[p_r][q] is wave-uniform, and the lane whose string holds q as its c-th
// orbital keeps it in column c.
template <int K>
__global__ __launch_bounds__(64) void fci_minor_kernel(RotU w, const int32_t *__restrict__ strs_r,
                                                       const int32_t *__restrict__ strs_c, int norb, uint32_t flip,
                                                       int parity, double scale, int64_t j0, int64_t width,
                                                       double *__restrict__ T, int64_t ld) {
    const int64_t i = blockIdx.y, jj = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = jj < width;
    const uint32_t sr = (uint32_t)strs_r[i], sc = live ? (uint32_t)strs_c[j0 + jj] : (uint32_t)strs_c[j0];
    const uint32_t full = (1u << norb) - 1u;
    const uint32_t mr = (sr ^ flip) & full, mc = (sc ^ flip) & full;
    int p[K];
    {
        uint32_t m = mr;
#pragma unroll
        for (int r = 0; r < K; ++r) {
            p[r] = m ? __builtin_ctz(m) : 0;
            m &= m - 1;
        }
    }
    double a[K][K];
#pragma unroll
    for (int r = 0; r < K; ++r)
#pragma unroll
        for (int c = 0; c < K; ++c) a[r][c] = 0.0;
    for (int q = 0; q < norb; ++q) {
        const bool has = mc >> q & 1u;
        const int rank = __builtin_popcount(mc & ((1u << q) - 1u));
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const bool take = has && rank == c;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const double x = w.v[p[r] * norb + q];
                a[r][c] = take ? x : a[r][c];
            }
        }
    }
    // LU with partial pivoting; the pivot row reaches position s by select
    double det = 1.0;
#pragma unroll
    for (int s = 0; s < K; ++s) {
        int piv = s;
        double best = fabs(a[s][s]);
#pragma unroll
        for (int r = s + 1; r < K; ++r) {
            const double v = fabs(a[r][s]);
            const bool up = v > best;
            piv = up ? r : piv;
            best = up ? v : best;
        }
#pragma unroll
        for (int r = s + 1; r < K; ++r) {
            const bool sw = piv == r;
#pragma unroll
            for (int c = s; c < K; ++c) {
                const double top = a[s][c], low = a[r][c];
                a[s][c] = sw ? low : top;
                a[r][c] = sw ? top : low;
            }
        }
        const double d = a[s][s];
        det = piv != s ? -det * d : det * d;
        const double inv = d != 0.0 ? 1.0 / d : 0.0;
#pragma unroll
        for (int r = s + 1; r < K; ++r) {
            const double f = a[r][s] * inv;
#pragma unroll
            for (int c = s + 1; c < K; ++c) a[r][c] = fma(-f, a[s][c], a[r][c]);
        }
    }
    double v = scale * det;
    if (parity && (__builtin_popcount((sr ^ sc) & 0xAAAAu) & 1)) v = -v;
    if (live) T[i * ld + jj] = v;
}

// ---- products ---------------------------------------------------------------------
// C[i * ldc + j] = sum_l A(i, l) B[l * ldb + j], A(i, l) = A[i * sam + l * sak], i < m, j < n, l < k.  A workgroup of
// 2 x 2 waves makes a 64 x 64 tile of C, a wave 2 x 2 MFMA tiles.  The sum runs over l in steps of 16 = four MFMAs; in
// MFMA s of a step, lane group g = lane / 16 carries l = l0 + 4 g + s, so that the four operands a lane holds are
// adjacent in l (a row of an A stored l-contiguous is read in whole 128-byte lines) and a fragment of an operand
// stored [l][.] is one line.  Elements beyond m, n, k are neither read nor written; they enter as 0.
// blockIdx.z picks one of up to kRotVecs products of the same shape and strides (evc_fci_rotate_block: the vectors that
// share a panel of T); the operands reach the kernel by value, and an element of C is the same sum in the same order
// whichever z computes it.
struct RotOps {
    const double *A[kRotVecs];
    const double *B[kRotVecs];
    double *C[kRotVecs];
};
__global__ __launch_bounds__(256) void fci_rotate_gemm_kernel(RotOps ops, int64_t sam, int64_t sak, int64_t ldb,
                                                              int64_t ldc, int64_t m, int64_t n, int64_t k) {
    const double *__restrict__ A = ops.A[blockIdx.z];
    const double *__restrict__ B = ops.B[blockIdx.z];
    double *__restrict__ C = ops.C[blockIdx.z];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int64_t i0 = (int64_t)blockIdx.y * 64 + (wave >> 1) * 32, j0 = (int64_t)blockIdx.x * 64 + (wave & 1) * 32;
    bool iok[2], jok[2];
    const double *ap[2], *bp[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        iok[t] = i0 + t * 16 + l15 < m;
        jok[t] = j0 + t * 16 + l15 < n;
        ap[t] = A + (iok[t] ? (i0 + t * 16 + l15) * sam : 0);
        bp[t] = B + (jok[t] ? j0 + t * 16 + l15 : 0);
    }
    d4 acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[r][c] = (d4){0.0, 0.0, 0.0, 0.0};
    for (int64_t l0 = 0; l0 < k; l0 += 16) {
        double af[2][4], bf[2][4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int64_t l = l0 + 4 * l4 + s;
            const bool lok = l < k;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                af[t][s] = (lok && iok[t]) ? ap[t][l * sak] : 0.0;
                bf[t][s] = (lok && jok[t]) ? bp[t][l * ldb] : 0.0;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c) acc[r][c] = mfma_f64(af[r][s], bf[c][s], acc[r][c]);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t i = i0 + r * 16 + l4 + 4 * v, j = j0 + c * 16 + l15;
                if (i < m && j < n) C[i * ldc + j] = acc[r][c][v];
            }
}

// ---- host side ----------------------------------------------------------------------
static int64_t rot_binomial(int n, int k) {
    int64_t b = 1;
    for (int i = 1; i <= k; ++i) b = b * (n - k + i) / i;
    return b;
}

// det(u) by LU with partial pivoting on a copy of u; `singular`: the smallest pivot is below 1e-12 of the largest (or
// exactly 0, det = 0).
static double rot_det(int n, const double *u, bool &singular) {
    double lu[kFciMaxOrb][kFciMaxOrb];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) lu[i][j] = u[i * n + j];
    double det = 1.0, pmin = INFINITY, pmax = 0.0;
    for (int s = 0; s < n; ++s) {
        int piv = s;
        for (int r = s + 1; r < n; ++r)
            if (fabs(lu[r][s]) > fabs(lu[piv][s])) piv = r;
        if (piv != s) {
            for (int c = 0; c < n; ++c) {
                const double t = lu[s][c];
                lu[s][c] = lu[piv][c];
                lu[piv][c] = t;
            }
            det = -det;
        }
        const double d = lu[s][s];
        det *= d;
        pmin = fmin(pmin, fabs(d));
        pmax = fmax(pmax, fabs(d));
        if (d == 0.0) {
            singular = true;
            return 0.0;
        }
        for (int r = s + 1; r < n; ++r) {
            const double f = lu[r][s] / d;
            for (int c = s + 1; c < n; ++c) lu[r][c] -= f * lu[s][c];
        }
    }
    singular = !(pmin >= 1e-12 * pmax);
    return det;
}

// inv = u^-1 by Gauss-Jordan with partial pivoting; only for a u that rot_det did not find singular
static void rot_invert(int n, const double *u, double *inv) {
    double a[kFciMaxOrb][2 * kFciMaxOrb];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            a[i][j] = u[i * n + j];
            a[i][n + j] = i == j ? 1.0 : 0.0;
        }
    for (int s = 0; s < n; ++s) {
        int piv = s;
        for (int r = s + 1; r < n; ++r)
            if (fabs(a[r][s]) > fabs(a[piv][s])) piv = r;
        if (piv != s)
            for (int c = 0; c < 2 * n; ++c) {
                const double t = a[s][c];
                a[s][c] = a[piv][c];
                a[piv][c] = t;
            }
        const double d = a[s][s];
        for (int c = 0; c < 2 * n; ++c) a[s][c] /= d;
        for (int r = 0; r < n; ++r) {
            if (r == s) continue;
            const double f = a[r][s];
            if (f == 0.0) continue;
            for (int c = 0; c < 2 * n; ++c) a[r][c] -= f * a[s][c];
        }
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) inv[i * n + j] = a[i][n + j];
}

// How the minors of one spin are made
struct RotSpin {
    RotU w;          // the matrix the kernel reads
    int norb;        // its order
    int K;           // instantiation
    int comp;        // 1: complementary minors of (u^-1)^T
    uint32_t flip;
    int parity;
    double scale;
    int64_t ns, pw, npanels;   // strings, panel width, panels
};

static int64_t rot_panel_width(int64_t ns) {
    int64_t w = kRotPanelDoubles / ns / 64 * 64;
    if (w < 64) w = 64;
    return w < ns ? w : ns;
}

static int rot_plan_spin(const char *who, int norb, int nocc, int64_t ns, const double *u, RotSpin &s) {
    const uint32_t full = norb >= 32 ? 0xFFFFFFFFu : (1u << norb) - 1u;
    s.ns = ns;
    s.pw = rot_panel_width(ns);
    s.npanels = ceil_div(ns, s.pw);
    s.norb = norb;
    s.comp = 0;
    s.flip = 0;
    s.parity = 0;
    s.scale = 1.0;
    for (int i = 0; i < kFciMaxOrb * kFciMaxOrb; ++i) s.w.v[i] = 0.0;
    if (nocc >= 1 && nocc <= kRotMaxMinor && nocc < norb) {
        s.K = nocc;
        for (int i = 0; i < norb * norb; ++i) s.w.v[i] = u[i];
        return 0;
    }
    if (nocc == 0 || nocc == norb) {
        // one string: T = [1] or [det u], as the 1 x 1 minor of the 1 x 1 matrix that holds it
        bool singular = false;
        s.K = 1;
        s.norb = 1;
        s.w.v[0] = nocc == 0 ? 1.0 : rot_det(norb, u, singular);
        s.flip = nocc == 0 ? 1u : (full ^ 1u);
        return 0;
    }
    bool singular = false;
    const double det = rot_det(norb, u, singular);
    EVC_REQUIRE(!singular, "%s: u is numerically singular (smallest pivot below 1e-12 of the largest) and "
                "%d electrons in %d orbitals need its inverse (complementary minors)", who, nocc, norb);
    double inv[kFciMaxOrb * kFciMaxOrb];
    rot_invert(norb, u, inv);
    s.K = norb - nocc;
    s.comp = 1;
    s.flip = full;
    s.parity = 1;
    s.scale = det;
    for (int i = 0; i < norb; ++i)
        for (int j = 0; j < norb; ++j) s.w.v[i * norb + j] = inv[j * norb + i];
    return 0;
}

static void rot_launch_minor(const RotSpin &s, const int32_t *strs, int64_t j0, int64_t width, double *T, int64_t ld,
                             hipStream_t st) {
    const dim3 grid((unsigned)ceil_div(width, 64), (unsigned)s.ns), block(64);
    switch (s.K) {
        case 1: rotate_launch(fci_minor_kernel<1>, grid, block, st, s.w, strs, strs, s.norb, s.flip, s.parity, s.scale, j0, width, T, ld); break;
        case 2: rotate_launch(fci_minor_kernel<2>, grid, block, st, s.w, strs, strs, s.norb, s.flip, s.parity, s.scale, j0, width, T, ld); break;
        case 3: rotate_launch(fci_minor_kernel<3>, grid, block, st, s.w, strs, strs, s.norb, s.flip, s.parity, s.scale, j0, width, T, ld); break;
        case 4: rotate_launch(fci_minor_kernel<4>, grid, block, st, s.w, strs, strs, s.norb, s.flip, s.parity, s.scale, j0, width, T, ld); break;
        case 5: rotate_launch(fci_minor_kernel<5>, grid, block, st, s.w, strs, strs, s.norb, s.flip, s.parity, s.scale, j0, width, T, ld); break;
        case 6: rotate_launch(fci_minor_kernel<6>, grid, block, st, s.w, strs, strs, s.norb, s.flip, s.parity, s.scale, j0, width, T, ld); break;
        case 7: rotate_launch(fci_minor_kernel<7>, grid, block, st, s.w, strs, strs, s.norb, s.flip, s.parity, s.scale, j0, width, T, ld); break;
        default: rotate_launch(fci_minor_kernel<8>, grid, block, st, s.w, strs, strs, s.norb, s.flip, s.parity, s.scale, j0, width, T, ld); break;
    }
}

// nz products of one shape, operands z of `ops`
static void rot_launch_gemm(const RotOps &ops, int nz, int64_t sam, int64_t sak, int64_t ldb, int64_t ldc, int64_t m,
                            int64_t n, int64_t k, hipStream_t st) {
    rotate_launch(fci_rotate_gemm_kernel, dim3((unsigned)ceil_div(n, 64), (unsigned)ceil_div(m, 64), (unsigned)nz),
                  dim3(256), st, ops, sam, sak, ldb, ldc, m, n, k);
}

// Workspace: M (nvec of (na, nb)) | T_a | T_b.  Resident: T_a (na, na) and T_b (nb, nb) whole; when both spins have the
// same strings and the same u, T_b is formed once and serves as T_a.  Panelled: one panel (ns, pw) of each.
struct RotLayout {
    size_t m_bytes, ta_full, tb_full, ta_panel, tb_panel;   // m_bytes: the M of one vector
};
static RotLayout rot_layout(int64_t na, int64_t nb) {
    RotLayout l;
    l.m_bytes = align_up((size_t)na * nb * 8, 256);
    l.ta_full = align_up((size_t)na * na * 8, 256);
    l.tb_full = align_up((size_t)nb * nb * 8, 256);
    l.ta_panel = align_up((size_t)na * rot_panel_width(na) * 8, 256);
    l.tb_panel = align_up((size_t)nb * rot_panel_width(nb) * 8, 256);
    return l;
}
// the resident grant, and the least one: the panelled form where it is the smaller
static size_t rot_resident_bytes(const RotLayout &l, int nvec) { return nvec * l.m_bytes + l.ta_full + l.tb_full; }
static size_t rot_least_bytes(const RotLayout &l, int nvec) {
    const size_t part = nvec * l.m_bytes + l.ta_panel + l.tb_panel, full = rot_resident_bytes(l, nvec);
    return part < full ? part : full;
}
static void clear_rotate_record() { note_kernel(EVC_PROF_FCI_ROTATE, "%s", ""); }

static int rot_shape(const char *who, int norb, int nocc_a, int nocc_b, int64_t na, int64_t nb) {
    EVC_REQUIRE(norb >= 1 && norb <= kFciMaxOrb, "%s: norb=%d, supported 1 ... %d", who, norb, kFciMaxOrb);
    EVC_REQUIRE(nocc_a >= 0 && nocc_a <= norb && nocc_b >= 0 && nocc_b <= norb, "%s: %d alpha and %d beta electrons in %d "
                "orbitals", who, nocc_a, nocc_b, norb);
    EVC_REQUIRE(na == rot_binomial(norb, nocc_a) && nb == rot_binomial(norb, nocc_b), "%s: na=%lld nb=%lld, but %d orbitals "
                "with (%d, %d) electrons have %lld and %lld strings", who, (long long)na, (long long)nb, norb, nocc_a, nocc_b,
                (long long)rot_binomial(norb, nocc_a), (long long)rot_binomial(norb, nocc_b));
    return 0;
}

// Both entry points: every refusal, then the launches for c[v] -> out[v], v < nvec, under one (u_a, u_b).  A panel of
// T is formed once and applied to all vectors, kRotVecs of them per product launch; vector v goes through the launches
// of a single call on it with the same arguments but its own M, so it has that call's bits.  The record is the caller's.
static int rot_run(const char *who, int norb, int nocc_a, int nocc_b, int64_t na, int64_t nb, const int32_t *strs_a,
                   const int32_t *strs_b, const double *u_a, const double *u_b, int nvec, const double *const *c,
                   double *const *out, void *ws, size_t ws_bytes, void *stream, RotSpin &sa, RotSpin &sb) {
    if (int rc = rot_shape(who, norb, nocc_a, nocc_b, na, nb)) return rc;
    EVC_REQUIRE(nvec >= 1, "%s: nvec=%d, at least 1", who, nvec);
    EVC_REQUIRE(strs_a && strs_b && u_a && u_b && c && out && ws, "%s: null pointer", who);
    for (int v = 0; v < nvec; ++v) EVC_REQUIRE(c[v] && out[v], "%s: null pointer (vector %d)", who, v);
    for (int v = 0; v < nvec; ++v)
        for (int w = 0; w < nvec; ++w) {
            EVC_REQUIRE(out[v] != c[w], "%s: out must not alias c (output %d, input %d)", who, v, w);
            EVC_REQUIRE(v == w || out[v] != out[w], "%s: outputs %d and %d are the same", who, v, w);
        }
    EVC_REQUIRE(aligned16(ws), "%s: workspace not 16-byte aligned", who);
    const RotLayout l = rot_layout(na, nb);
    bool shared = nocc_a == nocc_b;   // one T serves both spins
    for (int i = 0; shared && i < norb * norb; ++i) shared = u_a[i] == u_b[i];
    const size_t full = rot_resident_bytes(l, nvec), need = rot_least_bytes(l, nvec);
    EVC_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, at least %zu needed for %d vector(s) of %lld x %lld strings",
                who, ws_bytes, need, nvec, (long long)na, (long long)nb);
    if (int rc = rot_plan_spin(who, norb, nocc_a, na, u_a, sa)) return rc;
    if (int rc = rot_plan_spin(who, norb, nocc_b, nb, u_b, sb)) return rc;
    hipStream_t st = as_stream(stream);
    clear_rotate_record();
    const bool resident = ws_bytes >= full;
    char *base = static_cast<char *>(ws);
    char *tbase = base + nvec * l.m_bytes;
    double *Ta = reinterpret_cast<double *>(tbase);
    double *Tb = resident ? (shared ? Ta : reinterpret_cast<double *>(tbase + l.ta_full))
                          : reinterpret_cast<double *>(tbase + l.ta_panel);
    auto M = [&](int v) { return reinterpret_cast<double *>(base + v * l.m_bytes); };
    // M[:, J'] = sum_J c[:, J] T_b[J, J'], panel of J' by panel
    for (int64_t p = 0; p < sb.npanels; ++p) {
        const int64_t j0 = p * sb.pw, w = nb - j0 < sb.pw ? nb - j0 : sb.pw;
        double *T = resident ? Tb + j0 : Tb;
        const int64_t ld = resident ? nb : sb.pw;
        rot_launch_minor(sb, strs_b, j0, w, T, ld, st);
        EVC_LAUNCH_CHECK("fci_minor_kernel");
        for (int v0 = 0; v0 < nvec; v0 += kRotVecs) {
            const int nz = nvec - v0 < kRotVecs ? nvec - v0 : kRotVecs;
            RotOps ops = {};
            for (int z = 0; z < nz; ++z) {
                ops.A[z] = c[v0 + z];
                ops.B[z] = T;
                ops.C[z] = M(v0 + z) + j0;
            }
            rot_launch_gemm(ops, nz, nb, 1, ld, nb, na, w, nb, st);
            EVC_LAUNCH_CHECK("fci_rotate_gemm_kernel");
        }
    }
    // out[I', :] = sum_I T_a[I, I'] M[I, :], panel of I' by panel
    for (int64_t p = 0; p < sa.npanels; ++p) {
        const int64_t i0 = p * sa.pw, w = na - i0 < sa.pw ? na - i0 : sa.pw;
        double *T = resident ? Ta + i0 : Ta;
        const int64_t ld = resident ? na : sa.pw;
        if (!(resident && shared)) {
            rot_launch_minor(sa, strs_a, i0, w, T, ld, st);
            EVC_LAUNCH_CHECK("fci_minor_kernel");
        }
        for (int v0 = 0; v0 < nvec; v0 += kRotVecs) {
            const int nz = nvec - v0 < kRotVecs ? nvec - v0 : kRotVecs;
            RotOps ops = {};
            for (int z = 0; z < nz; ++z) {
                ops.A[z] = T;
                ops.B[z] = M(v0 + z);
                ops.C[z] = out[v0 + z] + i0 * nb;
            }
            rot_launch_gemm(ops, nz, 1, ld, nb, nb, w, nb, na, st);
            EVC_LAUNCH_CHECK("fci_rotate_gemm_kernel");
        }
    }
    return 0;
}

}  // namespace evc

using namespace evc;

extern "C" size_t evc_fci_rotate_workspace_bytes(int norb, int nocc_a, int nocc_b, int64_t na, int64_t nb, int minimal) {
    if (rot_shape("evc_fci_rotate_workspace_bytes", norb, nocc_a, nocc_b, na, nb)) return 0;
    const RotLayout l = rot_layout(na, nb);
    return minimal ? rot_least_bytes(l, 1) : rot_resident_bytes(l, 1);
}

extern "C" size_t evc_fci_rotate_block_workspace_bytes(int norb, int nocc_a, int nocc_b, int64_t na, int64_t nb, int nvec,
                                                       int minimal) {
    if (rot_shape("evc_fci_rotate_block_workspace_bytes", norb, nocc_a, nocc_b, na, nb)) return 0;
    if (nvec < 1) {
        set_error("evc_fci_rotate_block_workspace_bytes: nvec=%d, at least 1", nvec);
        return 0;
    }
    const RotLayout l = rot_layout(na, nb);
    return minimal ? rot_least_bytes(l, nvec) : rot_resident_bytes(l, nvec);
}

extern "C" int evc_fci_rotate_block(int norb, int nocc_a, int nocc_b, int64_t na, int64_t nb, const int32_t *strs_a,
                                    const int32_t *strs_b, const double *u_a, const double *u_b, int nvec,
                                    const double *const *c, double *const *out, void *ws, size_t ws_bytes, void *stream) {
    RotSpin sa, sb;
    if (int rc = rot_run("evc_fci_rotate_block", norb, nocc_a, nocc_b, na, nb, strs_a, strs_b, u_a, u_b, nvec, c, out, ws,
                         ws_bytes, stream, sa, sb))
        return rc;
    note_kernel(EVC_PROF_FCI_ROTATE, "fci_minor_kernel<%d> + fci_minor_kernel<%d> comp=%d,%d panels=%lld,%lld + "
                "fci_rotate_gemm_kernel vecs=%d", sa.K, sb.K, sa.comp, sb.comp, (long long)sa.npanels, (long long)sb.npanels,
                nvec);
    return 0;
}

extern "C" int evc_fci_rotate(int norb, int nocc_a, int nocc_b, int64_t na, int64_t nb, const int32_t *strs_a,
                              const int32_t *strs_b, const double *u_a, const double *u_b, const double *c, double *out,
                              void *ws, size_t ws_bytes, void *stream) {
    RotSpin sa, sb;
    if (int rc = rot_run("evc_fci_rotate", norb, nocc_a, nocc_b, na, nb, strs_a, strs_b, u_a, u_b, 1, &c, &out, ws, ws_bytes,
                         stream, sa, sb))
        return rc;
    note_kernel(EVC_PROF_FCI_ROTATE, "fci_minor_kernel<%d> + fci_minor_kernel<%d> comp=%d,%d panels=%lld,%lld + "
                "fci_rotate_gemm_kernel", sa.K, sb.K, sa.comp, sb.comp, (long long)sa.npanels, (long long)sb.npanels);
    return 0;
}
