// Expansion of active-space transition RDMs into the OAO basis (evc_cas_expand_rows; evcont_amd/cas_small.py states the
// algebra): for each ket, with the biorthogonal active orbitals A (n, ncas; the bra's, made orthogonal to
// that ket's core) and B (n, ncas; the ket's), the core matrix Qc (n, n) and the overlap S,
//   Qa  = A d1^T B^T                                    dm1 = (2 S Qc + Qa)^T
//   dm2[p,q,r,s] = sum_tuvw d2[t,u,v,w] A[p,t] B[q,u] A[r,v] B[s,w]
//                + S (4 Qc[p,q] Qc[r,s] - 2 Qc[p,s] Qc[r,q]) + 2 Qc[p,q] Qa[r,s] + 2 Qa[p,q] Qc[r,s]
//                - Qc[p,s] Qa[r,q] - Qa[p,s] Qc[r,q]
// Kernels:
//   cas_qa_kernel        one thread per (p, q), blockIdx.y the ket: Qa into the workspace and dm1.
//   cas_step_kernel<KS>  one quarter step of the rectangular four-index rotation ncas^4 -> n^4 in the form of quarter.hip
//                        (rotate the last index, move it to the front): out[j, row] = sum_k in[row, k] M[j, k], K = ncas
//                        <= 4 KS.  Four steps with M = B, A, B, A restore the index order.  A wave owns 16 rows, keeps
//                        their K values as the B operand (KS registers) and walks the <= 4 column tiles of M: KS
//                        v_mfma_f64_16x16x4_f64 per 16 x 16 tile, operand maps and the zero-masking of ragged K / ragged
//                        tiles as in small_mm.hpp.  A store instruction writes four runs of 16 consecutive doubles; the
//                        last step writes n^4 doubles for n^3 ncas read and its grid is sized for that.
//   cas_core_kernel      the core terms added to the dense block, one thread per element, (p, q) block-uniform.  A
//                        memory kernel in a launch of its own, as fci_row_pack_kernel.
// Packed layouts expand into a dense slot of the workspace and go through launch_fci_row_pack (fci_pack.hip), so a packed
// row has the bits of the host codecs on the dense block.  No atomics and no split sums: the same bits from run to run,
// and the kets are independent of one another.
#include "common.hpp"
#include "kernels.hpp"

namespace evc {

constexpr int kCasMaxOrb = 64;
constexpr int kCasMaxKets = 512;
constexpr int kCasStepBlocks = 4096;   // grid cap of a quarter step (grid-stride beyond)

// Launch through the runtime call (not the chevrons): tests/test_cas_closure.py keeps the list of the kernels this file
// launches against evc_cas_expand_describe.
template <typename T>
struct cas_same_type {
    using type = T;
};
template <typename... P>
static void cas_launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t st,
                       typename cas_same_type<P>::type... a) {
    void *args[] = {(void *)&a...};
    // the result is read by the EVC_LAUNCH_CHECK (hipGetLastError) that follows the call
    (void)hipLaunchKernel(reinterpret_cast<const void *>(kernel), grid, block, args, 0, st);
}

// Qa[ket][p,q] = sum_t A[p,t] (sum_u d1[u,t] B[q,u]);  dm1[ket][q,p] = 2 S Qc[p,q] + Qa[p,q]
__global__ __launch_bounds__(256) void cas_qa_kernel(int n, int ncas, const double *__restrict__ A,
                                                     const double *__restrict__ B, const double *__restrict__ Qc,
                                                     const double *__restrict__ ovlp, const double *__restrict__ d1,
                                                     double *__restrict__ Qa, int64_t qa_stride,
                                                     double *__restrict__ dm1) {
    const int ket = blockIdx.y, pq = blockIdx.x * 256 + threadIdx.x, n2 = n * n;
    if (pq >= n2) return;
    const int p = pq / n, q = pq - p * n;
    const double *a = A + ((int64_t)ket * n + p) * ncas, *b = B + ((int64_t)ket * n + q) * ncas, *d = d1 + (int64_t)ket * ncas * ncas;
    double acc = 0.0;
    for (int t = 0; t < ncas; ++t) {
        double inner = 0.0;
        for (int u = 0; u < ncas; ++u) inner = fma(d[u * ncas + t], b[u], inner);
        acc = fma(a[t], inner, acc);
    }
    Qa[ket * qa_stride + pq] = acc;
    const double core = Qc ? 2.0 * ovlp[ket] * Qc[(int64_t)ket * n2 + pq] : 0.0;
    dm1[(int64_t)ket * n2 + q * n + p] = core + acc;
}

// out[j * rows + row] = sum_k in[row * K + k] M[j * K + k],  row < rows, j < nout, k < K <= 4 KSTEPS
template <int KSTEPS>
__global__ __launch_bounds__(256) void cas_step_kernel(const double *__restrict__ in, const double *__restrict__ M, int K,
                                                       int nout, int64_t rows, double *__restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int64_t ntiles = (rows + 15) >> 4;
    const int nt = (nout + 15) >> 4;
    for (int64_t rt = (int64_t)blockIdx.x * 4 + wave; rt < ntiles; rt += (int64_t)gridDim.x * 4) {   // wave-uniform
        const int64_t row = rt * 16 + l15;
        const bool rv = row < rows;
        const double *src = in + (rv ? row : 0) * K;   // (rows beyond the end: read on row 0, masked, never stored)
        double b[KSTEPS];
#pragma unroll
        for (int kk = 0; kk < KSTEPS; ++kk) {
            const int k = 4 * kk + l4;
            const double v = src[k < K ? k : 0];
            b[kk] = rv && k < K ? v : 0.0;
        }
        for (int jt = 0; jt < nt; ++jt) {
            const int j = 16 * jt + l15;
            const bool jv = j < nout;
            const double *m = M + (jv ? j : 0) * K;
            d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < KSTEPS; ++kk) {
                const int k = 4 * kk + l4;
                const double v = m[k < K ? k : 0];
                acc = mfma_f64(jv && k < K ? v : 0.0, b[kk], acc);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jo = 16 * jt + l4 + 4 * r;
                if (jo < nout && rv) out[jo * rows + row] = acc[r];
            }
        }
    }
}

// dm2[p,q,r,s] += S (4 Qc[p,q] Qc[r,s] - 2 Qc[p,s] Qc[r,q]) + 2 Qc[p,q] Qa[r,s] + 2 Qa[p,q] Qc[r,s]
//               - Qc[p,s] Qa[r,q] - Qa[p,s] Qc[r,q];   blockIdx.y = p n + q, the threads run over r n + s
__global__ __launch_bounds__(256) void cas_core_kernel(int n, const double *__restrict__ Qc, const double *__restrict__ Qa,
                                                       const double *__restrict__ ovlp, double *__restrict__ dm2) {
    const int n2 = n * n, pq = blockIdx.y, rs = blockIdx.x * 256 + threadIdx.x;
    if (rs >= n2) return;
    const int p = pq / n, q = pq - p * n, r = rs / n, s = rs - r * n;
    const int ps = p * n + s, rq = r * n + q;
    const double S = ovlp[0];
    double v = dm2[(int64_t)pq * n2 + rs];
    v += S * (4.0 * Qc[pq] * Qc[rs] - 2.0 * Qc[ps] * Qc[rq]);
    v += 2.0 * Qc[pq] * Qa[rs] + 2.0 * Qa[pq] * Qc[rs];
    v -= Qc[ps] * Qa[rq] + Qa[ps] * Qc[rq];
    dm2[(int64_t)pq * n2 + rs] = v;
}

// ---- the plan of a call: what the launcher launches and what evc_cas_expand_describe prints ---------------------
struct CasPlan {
    int n, ncas, ksteps;
    int64_t n2, n4, qa_stride;          // doubles
    int64_t rows[4];                    // rows of the four quarter steps
    unsigned step_grid[4], qa_grid, core_grid;
    size_t off_qa, off_p, off_q, off_slot, bytes;   // workspace: Qa of every ket, the two step buffers, the dense slot
};

static CasPlan cas_plan(int n, int ncas, int nkets) {
    CasPlan p;
    p.n = n;
    p.ncas = ncas;
    p.ksteps = (ncas + 3) / 4;
    p.n2 = (int64_t)n * n;
    p.n4 = p.n2 * p.n2;
    p.qa_stride = (p.n2 + 1) & ~(int64_t)1;
    const int64_t c = ncas;
    p.rows[0] = c * c * c;
    p.rows[1] = n * c * c;
    p.rows[2] = p.n2 * c;
    p.rows[3] = p.n2 * n;
    for (int s = 0; s < 4; ++s) {
        const int64_t blocks = ceil_div(ceil_div(p.rows[s], 16), 4);
        p.step_grid[s] = (unsigned)(blocks < kCasStepBlocks ? blocks : kCasStepBlocks);
    }
    p.qa_grid = p.core_grid = (unsigned)ceil_div(p.n2, 256);
    p.off_qa = 0;
    p.off_p = align_up((size_t)nkets * p.qa_stride * 8, 256);
    p.off_q = p.off_p + align_up((size_t)(p.n2 * n * c) * 8, 256);     // P holds steps 1 and 3: n c^3 <= n^3 c
    p.off_slot = p.off_q + align_up((size_t)(p.n2 * c * c) * 8, 256);
    p.bytes = p.off_slot + align_up((size_t)p.n4 * 8, 256);
    return p;
}

static int cas_shape(const char *who, int n, int ncas, int nkets) {
    EVC_REQUIRE(ncas >= 1 && ncas <= kFciMaxOrb, "%s: ncas=%d (1 ... %d)", who, ncas, kFciMaxOrb);
    EVC_REQUIRE(n >= ncas && n <= kCasMaxOrb, "%s: n=%d (ncas=%d ... %d)", who, n, ncas, kCasMaxOrb);
    EVC_REQUIRE(nkets >= 1 && nkets <= kCasMaxKets, "%s: nkets=%d (1 ... %d)", who, nkets, kCasMaxKets);
    return 0;
}

static bool cas_layout_ok(int layout) {
    return layout == EVC_LAYOUT_FULL6 || layout == EVC_LAYOUT_PACK2 || layout == EVC_LAYOUT_SYM8;
}

template <int KSTEPS>
static int cas_step(const CasPlan &p, int s, const double *in, const double *M, double *out, hipStream_t st) {
    cas_launch(cas_step_kernel<KSTEPS>, dim3(p.step_grid[s]), dim3(256), st, in, M, p.ncas, p.n, p.rows[s], out);
    EVC_LAUNCH_CHECK("cas_step_kernel");
    return 0;
}

static int cas_steps(const CasPlan &p, const double *d2, const double *A, const double *B, double *P, double *Q,
                     double *dst, hipStream_t st) {
    const double *in[4] = {d2, P, Q, P}, *M[4] = {B, A, B, A};
    double *out[4] = {P, Q, P, dst};
    for (int s = 0; s < 4; ++s) {
        switch (p.ksteps) {
            case 1: EVC_TRY(cas_step<1>(p, s, in[s], M[s], out[s], st)); break;
            case 2: EVC_TRY(cas_step<2>(p, s, in[s], M[s], out[s], st)); break;
            case 3: EVC_TRY(cas_step<3>(p, s, in[s], M[s], out[s], st)); break;
            default: EVC_TRY(cas_step<4>(p, s, in[s], M[s], out[s], st)); break;
        }
    }
    return 0;
}

}  // namespace evc

using namespace evc;

extern "C" size_t evc_cas_expand_workspace_bytes(int n, int ncas, int nkets) {
    if (cas_shape("evc_cas_expand_workspace_bytes", n, ncas, nkets)) return 0;
    return cas_plan(n, ncas, nkets).bytes;
}

extern "C" int evc_cas_expand_rows(int n, int ncas, int nkets, const double *A_act, const double *B_act, const double *Qc,
                                   const double *ovlp, const double *d1, const double *d2, double *dm1, int layout,
                                   double *rows, int64_t ld, void *ws, size_t ws_bytes, void *stream) {
    if (int rc = cas_shape("evc_cas_expand_rows", n, ncas, nkets)) return rc;
    EVC_REQUIRE(A_act && B_act && ovlp && d1 && d2 && dm1 && rows && ws, "evc_cas_expand_rows: null pointer");
    EVC_REQUIRE(cas_layout_ok(layout),
                "evc_cas_expand_rows: layout=%d (EVC_LAYOUT_FULL6, EVC_LAYOUT_PACK2 or EVC_LAYOUT_SYM8)", layout);
    const CasPlan p = cas_plan(n, ncas, nkets);
    const bool packed = layout != EVC_LAYOUT_FULL6;
    if (packed) {
        const int64_t cols = fci_row_pack_cols(layout, n);
        EVC_REQUIRE(ld % 16 == 0 && ld >= cols && ld < ((int64_t)1 << 31),
                    "evc_cas_expand_rows: ld=%lld (a multiple of 16, at least %lld columns rounded up to 16, below 2^31)",
                    (long long)ld, (long long)cols);
    } else {
        EVC_REQUIRE(ld >= p.n4 && ld < ((int64_t)1 << 31), "evc_cas_expand_rows: ld=%lld (at least n^4 = %lld, below 2^31)",
                    (long long)ld, (long long)p.n4);
    }
    EVC_REQUIRE(aligned16(A_act) && aligned16(B_act) && aligned16(Qc) && aligned16(ovlp) && aligned16(d1) && aligned16(d2) &&
                    aligned16(dm1) && aligned16(rows) && aligned16(ws),
                "evc_cas_expand_rows: every pointer must be 16-byte aligned");
    EVC_REQUIRE(ws_bytes >= p.bytes, "evc_cas_expand_rows: workspace of %zu bytes, %zu needed for n=%d ncas=%d nkets=%d",
                ws_bytes, p.bytes, n, ncas, nkets);
    hipStream_t st = as_stream(stream);
    char *base = static_cast<char *>(ws);
    double *Qa = reinterpret_cast<double *>(base + p.off_qa), *P = reinterpret_cast<double *>(base + p.off_p);
    double *Q = reinterpret_cast<double *>(base + p.off_q), *slot = reinterpret_cast<double *>(base + p.off_slot);
    const int64_t c2 = (int64_t)ncas * ncas;

    cas_launch(cas_qa_kernel, dim3(p.qa_grid, (unsigned)nkets), dim3(256), st, n, ncas, A_act, B_act, Qc, ovlp, d1, Qa,
               p.qa_stride, dm1);
    EVC_LAUNCH_CHECK("cas_qa_kernel");
    for (int i = 0; i < nkets; ++i) {
        double *dst = packed ? slot : rows + (int64_t)i * ld;
        EVC_TRY(cas_steps(p, d2 + i * c2 * c2, A_act + (int64_t)i * n * ncas, B_act + (int64_t)i * n * ncas, P, Q, dst, st));
        if (Qc) {
            cas_launch(cas_core_kernel, dim3(p.core_grid, (unsigned)p.n2), dim3(256), st, n, Qc + i * p.n2,
                       (const double *)(Qa + i * p.qa_stride), ovlp + i, dst);
            EVC_LAUNCH_CHECK("cas_core_kernel");
        }
        if (packed) EVC_TRY(launch_fci_row_pack(layout, n, slot, rows + (int64_t)i * ld, ld, st));
    }
    return 0;
}

extern "C" int evc_cas_expand_describe(int n, int ncas, int layout, char *buf, size_t buf_len) {
    EVC_REQUIRE(buf && buf_len > 0, "evc_cas_expand_describe: buf is NULL");
    if (int rc = cas_shape("evc_cas_expand_describe", n, ncas, 1)) return rc;
    EVC_REQUIRE(cas_layout_ok(layout),
                "evc_cas_expand_describe: layout=%d (EVC_LAYOUT_FULL6, EVC_LAYOUT_PACK2 or EVC_LAYOUT_SYM8)", layout);
    const CasPlan p = cas_plan(n, ncas, 1);
    size_t len = 0;
    auto line = [&](const char *fmt, auto... a) {
        const int k = snprintf(len < buf_len ? buf + len : nullptr, len < buf_len ? buf_len - len : 0, fmt, a...);
        if (k > 0) len += (size_t)k;
    };
    buf[0] = '\0';
    line("cas_qa_kernel grid=(%u,nkets)\n", p.qa_grid);
    for (int s = 0; s < 4; ++s)
        line("cas_step_kernel<%d> step=%d M=%c rows=%lld grid=%u\n", p.ksteps, s + 1, s & 1 ? 'A' : 'B',
             (long long)p.rows[s], p.step_grid[s]);
    line("cas_core_kernel grid=(%u,%lld) if Qc\n", p.core_grid, (long long)p.n2);
    if (layout != EVC_LAYOUT_FULL6)
        line("fci_row_pack_kernel<%d> cols=%lld\n", layout == EVC_LAYOUT_SYM8 ? 8 : 1, (long long)fci_row_pack_cols(layout, n));
    return (int)len;
}
