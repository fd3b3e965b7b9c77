// The transform route of a call: which form the four-index rotations take and what the energy phase leaves in the K3
// buffer for the gradient phase.  Pure host functions of (layout, n, flags): decided here and nowhere else.
#pragma once
#include "common.hpp"

namespace evc {

constexpr int kPairTransformMaxN = 32;
// Row pitch of the pipeline's dense (pair, pair) intermediates: n(n+1)/2 rounded up to 16 doubles.
__host__ __device__ inline int pair_ld(int n) { return (n * (n + 1) / 2 + 15) & ~15; }

inline bool is_sym8(int layout) { return layout == EVC_LAYOUT_SYM8; }
// the two-body columns are the packed lower triangle of the (pair, pair) matrix (or its 8-fold compressed form)
inline bool is_packed(int layout) { return layout == EVC_LAYOUT_ELEC3 || layout == EVC_LAYOUT_PACK2 || is_sym8(layout); }

enum class Steps {
    Quarter,   // four quarter steps
    Pair,      // n <= 32: two fused pair steps (pair_transform.hip / pair_pipe.hip / pair_dma.hip)
    Pair64,    // 32 < n <= 64 on the compressed layout with the large array handed over packed (EVC_FLAG_ERI_S4 with the
               // energy phase, EVC_FLAG_IP1_S2KL with the gradient phase): pair steps on 64 x 64 operand matrices
               // (pair64.hip).  (Full arrays take the quarter-step route.)
};
struct Route {
    Steps steps;
    bool symmetric;   // the symmetric pipeline: compressed layout on pair steps, every operand a dense (pair, pair) matrix
    // What the K3 buffer holds after the energy phase, the contract between the two phases: K3, the three-quarter-
    // transformed integrals, or (symmetric pipeline) the dense (pair, pair) intermediate of the first pair step, pair_ld(n)
    // rows at the pitch pair_ld(n), from which Y2 recomputes the half-transformed integrals (y2.hip y2_fused_kernel)
    bool k3_is_dense_mid() const { return symmetric; }
    int64_t k3_doubles;   // ... and its extent
    bool pairs() const { return steps != Steps::Quarter; }
};

// The integral-side route; packed_input: int2e (energy phase) / int2e_ip1 (gradient phase) comes packed.
inline Route transform_route(int layout, int n, bool packed_input) {
    Route r;
    const bool pair64 = is_sym8(layout) && n <= 64 && packed_input;
    r.steps = n <= kPairTransformMaxN ? Steps::Pair : pair64 ? Steps::Pair64 : Steps::Quarter;
    r.symmetric = is_sym8(layout) && r.pairs();
    r.k3_doubles = r.symmetric ? (int64_t)pair_ld(n) * pair_ld(n) : (int64_t)n * n * n * n;
    return r;
}

// The two phases of one evaluation must agree on the route (the gradient phase finds in the K3 buffer what the energy
// phase left there).  Up to 32 orbitals the packed flags do not select it; beyond, both large arrays come packed or
// neither: the fused entry points check it, callers of the phase entry points pass both flags or neither.
inline bool phases_agree(int n, bool eri_packed, bool ip1_packed) {
    return n <= kPairTransformMaxN || eri_packed == ip1_packed;
}

}  // namespace evc
