// The side stream of the split Loewdin step: one per device, two events per workspace.
#include <stdlib.h>

#include <mutex>
#include <unordered_map>

#include "pipeline.hpp"

namespace evc {

// ---- the Loewdin step in two halves (n <= 64) -------------------------------------------------------------
// The energy phase needs X = S^-1/2 and h1 only; the eigenvectors and eigenvalues of S enter at the very end of the
// gradient (the response term, launch_grad_final).  A full call therefore computes X and h1 by Newton-Schulz on the
// matrix cores (loewdin.hpp loewdin_ns / loewdin.hip loewdin_ns64_kernel) and keeps the eigensolver off the critical path
// (loewdin_split_mode below): either in the launch of the subspace solve (Call::split = 3) or on a side stream, forked at
// the start of the call and joined by whichever call reads U and s next (Call::split = 1):
// one side stream per device and two events per workspace, created at the workspace's first such call; the events live
// until evc_release_workspace, the stream until the last workspace that used it is released.
struct Side {
    hipStream_t s;           // the device's side stream (shared by all workspaces on it: one more hardware queue in use,
                             // not one per workspace -- the runtime multiplexes all streams onto four of them, and a
                             // process whose streams outnumber them sees unrelated streams serialised)
    hipEvent_t fork, join;   // of this workspace
    int dev;
    bool pending;            // an eigensolver launch into this workspace has not been joined yet
};
struct SideStream {
    hipStream_t s;
    int users;               // workspaces holding events on it; destroyed with the last one
};
static std::mutex g_side_mu;
static std::unordered_map<void *, Side> g_side;
static std::unordered_map<int, SideStream> g_side_stream;   // by device

static Side *side_of(void *ws) {
    std::lock_guard<std::mutex> lk(g_side_mu);
    auto it = g_side.find(ws);
    if (it != g_side.end()) return &it->second;
    int dev = 0;
    Side sd{};
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    auto ds = g_side_stream.find(dev);
    if (ds == g_side_stream.end()) {
        hipStream_t ns;
        if (hipStreamCreateWithFlags(&ns, hipStreamNonBlocking) != hipSuccess) {
            set_error("side stream: %s", hipGetErrorString(hipGetLastError()));
            return nullptr;
        }
        ds = g_side_stream.emplace(dev, SideStream{ns, 0}).first;
    }
    sd.s = ds->second.s;
    sd.dev = dev;
    if (hipEventCreateWithFlags(&sd.fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&sd.join, hipEventDisableTiming) != hipSuccess) {
        set_error("side stream events: %s", hipGetErrorString(hipGetLastError()));
        return nullptr;
    }
    ++ds->second.users;
    return &g_side.emplace(ws, sd).first->second;
}

int side_launch_loewdin(void *ws, const LoewdinArgs &la, int count, hipStream_t st) {
    Side *sd = side_of(ws);
    if (!sd) return -1;
    EVC_HIP(hipEventRecord(sd->fork, st));
    EVC_HIP(hipStreamWaitEvent(sd->s, sd->fork, 0));
    EVC_TRY(launch_loewdin(la, count, sd->s));
    EVC_HIP(hipEventRecord(sd->join, sd->s));
    std::lock_guard<std::mutex> lk(g_side_mu);
    auto it = g_side.find(ws);
    if (it != g_side.end()) it->second.pending = true;
    return 0;
}

int side_join(void *ws, hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_side_mu);
    auto it = g_side.find(ws);
    if (it == g_side.end() || !it->second.pending) return 0;
    EVC_HIP(hipStreamWaitEvent(st, it->second.join, 0));
    it->second.pending = false;
    return 0;
}

// which form the Loewdin step of a FULL call (evc_energy_with_grad[_batch]) takes
int loewdin_split_mode(int n, int ntrain, int count, bool loewdin_done, bool warm, hipStream_t st) {
    // EVC_LOEWDIN_SPLIT=0: the one-kernel Loewdin step always.
    static const int knob = getenv("EVC_LOEWDIN_SPLIT") ? atoi(getenv("EVC_LOEWDIN_SPLIT")) : 12;
    if (knob == 0 || loewdin_done || !loewdin_split_available(n)) return 0;
    // Small kernels on both sides (n <= 32 orbitals, T <= 32 states), any number of geometries, cold or warm: the
    // eigensolver half rides in the launch of the subspace solve, one workgroup per geometry beside one workgroup per
    // geometry (subspace_small.hip subspace_loewdin_kernel) -- no second stream.  One geometry per call it performs like the
    // side stream below (H30: 4 480 against 4 500 steps/s, H10: 11 170 against 11 210) without costing the process a
    // hardware queue; 32 geometries per call on one stream: 60 700 -> 64 500 geometries/s, three streams unchanged.
    if (n <= kPairTransformMaxN && ntrain <= kSubspaceSmallT) return 3;
    // Otherwise (33 ... 64 orbitals: the 1024-thread eigensolver, 550 us at n = 58, has no launch to ride in; or a large
    // training set) the side stream, for calls of fewer than `knob` geometries (default 12: the latency regime).  Not the
    // large batches: with several of them in flight on different streams the chip is full anyway and a fifth stream
    // shares a hardware queue with one of them (measured at H30, 32 geometries per call, three streams: 87 000 -> 73 700).
    if (count >= knob) return 0;
    if (warm && n <= kPairTransformMaxN) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return 0;
    // (energy-only calls as well: a later evc_phase_gradient on the same workspace reads U and s -- hosted.py uploads the
    //  gradient's inputs in between)
    return 1;
}

}  // namespace evc

using namespace evc;

extern "C" int evc_release_workspace(void *ws) {
    std::lock_guard<std::mutex> lk(g_side_mu);
    auto it = g_side.find(ws);
    if (it == g_side.end()) return 0;
    (void)hipEventSynchronize(it->second.join);   // (the last eigensolver launch that writes into this workspace)
    (void)hipEventDestroy(it->second.fork);
    (void)hipEventDestroy(it->second.join);
    auto ds = g_side_stream.find(it->second.dev);
    if (ds != g_side_stream.end() && --ds->second.users == 0) {
        (void)hipStreamDestroy(ds->second.s);   // (idle: every launch on it was followed by a join event, all waited for)
        g_side_stream.erase(ds);
    }
    g_side.erase(it);
    return 0;
}
