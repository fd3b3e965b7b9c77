#include "pipeline.hpp"

namespace evc {

// ---- several roots: evc_phase_gradient_roots (one geometry), evc_phase_gradient_roots_batch (several) -------------
// Root-pair-major slots s = p * count + g: pair p = (k, l) of geometry g, whose row weights are those of the symmetric
// weighting of rows k, l of geometry g's coefficient block.  Block p = 0 is the workspace the energy-only call left
// (geometries 0 .. count-1); the state phases A+B left there (X, U, s, lflag, h1, K3) is copied into the blocks p >= 1,
// so that the batched gradient chain runs unchanged for count * npairs slots: K8 reads the t-RDM once per kMaxBatchG
// slots.  Behind the slots: the per-slot nuclear term (grad_nuc on the diagonal pairs, zero on the couplings).
// gradient_roots does all of that for both entry points; they differ in their geometry alone:
//   evc_phase_gradient_roots        count = 1, every stride 0 and geo_period = 0: to the chain every slot is a geometry
//                                   of its own, so the IP1 contraction keeps its one-slot form;
//                                   gnuc is optional (NULL: no nuclear term);
//   evc_phase_gradient_roots_batch  geo_period = count: slot s reads the caller's inputs of geometry s % count
//                                   (kernels.hpp geo_of); gnuc is required.
// The nuclear term: with a coupling pair in the list the buffer is cleared and grad_nuc copied to each diagonal pair;
// with the diagonal alone it is copied once and fanned out like the slot state.
constexpr int kMaxRootPairs = 4096;
// count * npairs slots of `slot_bytes` each, then the per-slot nuclear term
static size_t roots_bytes(size_t slot_bytes, int natm, int nslots) {
    return slot_bytes * (size_t)nslots + align_up((size_t)nslots * (natm > 0 ? natm : 1) * 3 * sizeof(double), 256);
}

static size_t workspace_bytes_roots(const char *who, const evc_trdm_set *t, int natm, int count, int npairs) {
    if (check_set(t)) return 0;
    if (count < 1 || npairs < 1 || (int64_t)count * npairs > kMaxRootPairs) {
        set_error("%s: count=%d, npairs=%d (need count >= 1, npairs >= 1, count * npairs <= %d)", who, count, npairs,
                  kMaxRootPairs);
        return 0;
    }
    return roots_bytes(carve(t, natm, nullptr).bytes, natm, count * npairs);
}

// Block b of `rows` rows (row r at base + (b * rows + r) * pitch, `bytes` bytes each) := block 0, for b = 1 .. blocks-1:
// log2(blocks) 2-D copies, each doubling the filled prefix.
static int fan_out_blocks(char *base, size_t bytes, size_t pitch, int rows, int blocks, hipStream_t st) {
    if (pitch > (size_t)INT32_MAX) {   // (beyond the pitch a 2-D copy takes: one copy per row)
        for (int s = rows; s < rows * blocks; ++s)
            EVC_HIP(hipMemcpyAsync(base + (size_t)s * pitch, base + (size_t)(s % rows) * pitch, bytes,
                                   hipMemcpyDeviceToDevice, st));
        return 0;
    }
    for (int have = 1; have < blocks;) {
        const int m = blocks - have < have ? blocks - have : have;
        EVC_HIP(hipMemcpy2DAsync(base + (size_t)have * rows * pitch, pitch, base, pitch, bytes, (size_t)m * rows,
                                 hipMemcpyDeviceToDevice, st));
        have += m;
    }
    return 0;
}

// g: the caller's count = g.count geometries; a batch brings one (T, T) coefficient block per geometry, one geometry
// one block for every slot (stride 0).
static int gradient_roots(const char *who, const evc_trdm_set *t, Geo g, const double *coeffs, int nvec,
                          const int32_t *pairs, int npairs, const evc_outputs_roots *out, int flags, void *ws,
                          size_t ws_bytes, void *stream) {
    if (check_set(t) || check_geometry(who, g, true)) return -1;
    EVC_REQUIRE(coeffs && pairs, "%s: coeffs / pairs is NULL", who);
    EVC_REQUIRE(out && out->grad, "%s: outputs.grad is required", who);
    EVC_REQUIRE(!(flags & EVC_FLAG_PARTIAL_RANK), "%s: EVC_FLAG_PARTIAL_RANK is not supported", who);
    EVC_REQUIRE(!(flags & ~EVC_FLAG_IP1_S2KL), "%s: flags=%d (only EVC_FLAG_IP1_S2KL is accepted)", who, flags);
    EVC_REQUIRE(npairs >= 1 && npairs <= kMaxRootPairs, "%s: npairs=%d out of range 1..%d", who, npairs, kMaxRootPairs);
    const int count = g.count;
    EVC_REQUIRE((int64_t)count * npairs <= kMaxRootPairs, "%s: count * npairs = %d * %d exceeds %d slots", who, count,
                npairs, kMaxRootPairs);
    EVC_REQUIRE(nvec >= 1 && nvec <= t->ntrain, "%s: nvec=%d out of range 1..%d (T)", who, nvec, t->ntrain);
    bool any_coupling = false;
    for (int p = 0; p < npairs; ++p) {
        const int k = pairs[2 * p], l = pairs[2 * p + 1];
        EVC_REQUIRE(0 <= k && k <= l && l < nvec, "%s: pair %d = (%d, %d) outside 0 <= k <= l < nvec=%d", who, p, k, l,
                    nvec);
        any_coupling = any_coupling || k != l;
    }
    const int nslots = count * npairs;
    Call c;
    if (setup(who, t, g, flags, ws, ws_bytes, nslots, c)) return -1;   // (flags: EVC_FLAG_IP1_S2KL alone, checked above)
    const Ws &w = c.w;
    const size_t need = roots_bytes(w.bytes, g.natm, nslots);
    EVC_REQUIRE(ws_bytes >= need, "%s: workspace too small: %zu < %zu", who, ws_bytes, need);
    hipStream_t st = as_stream(stream);
    const int n = t->n;
    const int64_t n2 = (int64_t)n * n, A3 = (int64_t)g.natm * 3;
    // (1) row weights of every slot: pair p of coefficient block g (+ the transposed group copies of the batched K8)
    const int64_t sc = g.batch ? (int64_t)t->ntrain * t->ntrain : 0;
    EVC_TRY(launch_pair_weights_geo(coeffs, sc, g.geo_period, t->ntrain, t->layout, pairs, npairs, w.w1, w.w2,
                                      nslots > 1 ? w.w1t : nullptr, nslots > 1 ? w.w2t : nullptr, w.stride,
                                      t->row_offset, t->rows2, st));
    // (2) block 0 into the blocks p >= 1; U and s may still come from the side stream (phase A of an energy-only call)
    EVC_TRY(side_join(w.base, st));
    char *b0 = static_cast<char *>(ws);
    if (npairs > 1) {
        // X, U, s, lflag, h1 (consecutive at the head of a slot) and what phase A left in the K3 buffer for Y2 (route.hpp)
        EVC_TRY(fan_out_blocks(b0, (size_t)((char *)(w.h1 + n2) - (char *)w.X), w.bytes, count, npairs, st));
        EVC_TRY(fan_out_blocks((char *)w.K3, sizeof(double) * (size_t)c.ip1.k3_doubles, w.bytes, count, npairs, st));
    }
    // (3) nuclear term: the geometry's grad_nuc on the diagonal pairs, zero on the couplings
    if (g.gnuc) {
        char *gnuc = b0 + w.bytes * (size_t)nslots;
        const size_t blk = sizeof(double) * A3 * count;   // one pair's (count, A, 3)
        if (any_coupling) {
            EVC_HIP(hipMemsetAsync(gnuc, 0, blk * npairs, st));
            for (int p = 0; p < npairs; ++p)
                if (pairs[2 * p] == pairs[2 * p + 1])
                    EVC_HIP(hipMemcpyAsync(gnuc + blk * p, g.gnuc, blk, hipMemcpyDeviceToDevice, st));
        } else {
            EVC_HIP(hipMemcpyAsync(gnuc, g.gnuc, blk, hipMemcpyDeviceToDevice, st));
            EVC_TRY(fan_out_blocks(gnuc, blk, blk, 1, npairs, st));
        }
        g.gnuc = reinterpret_cast<const double *>(gnuc);
    }
    // (4) the gradient chain for count * npairs slots
    g.count = nslots;
    g.sgn = A3;
    Out o;
    memset(&o, 0, sizeof(o));
    o.grad = out->grad;
    o.sg = A3;
    o.d_pred = out->d_pred;
    o.sd = n2;
    o.g_pred = out->g_pred;
    o.sG = n2 * n2;
    return phase_gradient(t, g, o, flags, c, st);
}

}  // namespace evc

using namespace evc;

extern "C" size_t evc_workspace_bytes_roots(const evc_trdm_set *t, int natm, int npairs) {
    return workspace_bytes_roots("evc_workspace_bytes_roots", t, natm, 1, npairs);
}

extern "C" size_t evc_workspace_bytes_roots_batch(const evc_trdm_set *t, int natm, int count, int npairs) {
    return workspace_bytes_roots("evc_workspace_bytes_roots_batch", t, natm, count, npairs);
}

extern "C" int evc_phase_gradient_roots(const evc_trdm_set *t, const evc_geometry *g, const double *coeffs, int nvec,
                                        const int32_t *pairs, int npairs, const evc_outputs_roots *out, int flags,
                                        void *ws, size_t ws_bytes, void *stream) {
    clear_kernels(kStagesGradient);
    return gradient_roots("evc_phase_gradient_roots", t, geo_single(g), coeffs, nvec, pairs, npairs, out, flags, ws,
                          ws_bytes, stream);
}

extern "C" int evc_phase_gradient_roots_batch(const evc_trdm_set *t, const evc_geometry_batch *gb, const double *coeffs,
                                              int nvec, const int32_t *pairs, int npairs, const evc_outputs_roots *out,
                                              int flags, void *ws, size_t ws_bytes, void *stream) {
    clear_kernels(kStagesGradient);
    Geo g = geo_batch(t, gb);
    g.geo_period = g.count;
    return gradient_roots("evc_phase_gradient_roots_batch", t, g, coeffs, nvec, pairs, npairs, out, flags, ws, ws_bytes,
                          stream);
}
