#!/usr/bin/env python3
"""Throughput benchmark of the continuation energy+force hot path (BASELINE.json metric:
continuation geometries/sec, energy+force, H30 STO-3G, 20 training states).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch G] [--streams S]
                    [--layout sym8|pack2|full6|pair5|elec3] [--workload H30|H10|H2O|Zundel]

One "step" = one pass of the hot path over one batch of G synthetic geometries (N=30 orbitals,
A=30 atoms) against T=20 training states whose t-RDMs are resident in HBM: G energy+force
evaluations.  Every launch of the pipeline covers the whole batch and the two streaming kernels
read the t-RDM once per 32 geometries (evc_energy_with_grad_batch).  S streams keep S batches in
flight so the single-workgroup (latency-bound) kernels of one batch overlap the streaming kernels
of another.  64 distinct geometry bundles are resident on the device and cycled.

`--layout sym8` (default) keeps the training data in the 8-fold compressed device layout built from
the reference's pack2 rows (include/evcont_hip.h EVC_LAYOUT_SYM8: same energies and forces for AO
integrals with the index symmetries of real two-electron integrals, which the synthetic geometries
have); the same run also measures the reference's own pack2 layout ("reference_layout").  The
roofline block describes kernel K5 (the 2-RDM x ERI contraction) in the single-stream leg, where it has
the device to itself; its figure inside the multi-stream headline region is given as "contended".

`--batch 1 --streams 1` is the strictly sequential regime of an MD run (one geometry at a time);
it is measured as well and reported under "md_regime".

With --gpus N > 1 (launched by torch.distributed.run, one rank per GPU) two ways of using the
node are measured in the same run:
  --shard geometries (default, `value`): every rank holds a replica of the t-RDMs (0.68 GB) and
      evaluates its own batches of geometries; no data-path collective; per-GPU work is fixed, so
      scaling is "weak" and `value` = geometries of ALL ranks / max-over-ranks time.
  --shard pairs (reported under "pair_sharded"; `value` when selected): the training PAIRS are
      sharded over the ranks, every rank sees the same batch, two KB-sized RCCL collectives per
      step (evcont_amd/distributed.py); total work is fixed: "strong".

Rank 0 prints ONE JSON line (see DESIGN.md §5 for every field).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np
import torch
import torch.distributed as dist

WORKLOADS = {
    # name: (N, A, T, ao_sizes)
    "H30": (30, 30, 20, None),            # BASELINE configs[2], the metric's configuration
    "H10": (10, 10, 5, None),             # configs[1]
    "H2O": (13, 3, 10, (9, 2, 2)),        # configs[3] (T assumed 10)
    "Zundel": (28, 7, 30, (9, 2, 2, 2, 9, 2, 2)),  # configs[4]
    # the same molecule with the 100 training states of the reference's learning curve
    # (scripts/MD/Zundel_thermodynamics/continuation/05_Zundel_test_potential_energy.py:182-210): 5050 pair rows
    "Zundel100": (28, 7, 100, (9, 2, 2, 2, 9, 2, 2)),
    # cc-pVTZ water, the reference's largest orbital space (scripts/MD/H2O/md_H2O_vtz_CAS_continuation.py:31)
    "H2Ovtz": (58, 3, 8, (30, 14, 14)),
}
LAYOUT_ND = {"full6": 6, "pair5": 5, "elec3": 3, "pack2": 2,
             "sym8": 8}   # sym8: 8-fold compressed device layout, built from the pack2 rows (include/evcont_hip.h)
HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: 8 TB/s spec (~6 TB/s achievable by a plain streaming read)
MFMA_F64_PEAK_TFLOPS = 78.6   # MI355X_MICROARCH.md: dense FP64 matrix peak (v_mfma_f64_16x16x4_f64)
MAX_G_PER_LAUNCH = 32   # geometries that share one pass over the t-RDM (csrc/gemv_mfma.hip; K8 always)


def k5_launch_info(lib, G: int):
    """(kernel symbol, geometries per launch) of the K5 launch the library made LAST (``evc_profile_kernel``: the
    launchers record what they enqueue) -- asked of the library instead of mirroring its dispatch rules here."""
    name = lib.evc_profile_kernel(0).decode()
    gl = min(G, MAX_G_PER_LAUNCH)
    if " G=" in name:
        name, g = name.rsplit(" G=", 1)
        gl = int(g)
    return name, gl


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--workload", default="H30", choices=list(WORKLOADS))
    p.add_argument("--layout", default="sym8", choices=list(LAYOUT_ND))
    p.add_argument("--geoms", type=int, default=64, help="distinct synthetic geometries resident on the device")
    p.add_argument("--batch", type=int, default=32, help="geometries per step (1 = one geometry per step, MD regime)")
    p.add_argument("--streams", type=int, default=3, help="batches in flight (one HIP stream + workspace each)")
    p.add_argument("--repeats", type=int, default=5,
                   help="the timed region of EXACTLY --steps steps is run this many times back to back (each bracketed "
                        "by barrier + synchronize, max over ranks); `value` is the median, every repeat is listed")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-md-regime", action="store_true", help="skip the extra sequential (batch 1, 1 stream) leg")
    p.add_argument("--cpu-samples", type=int, default=0, help="geometries timed on the host (0 = auto)")
    p.add_argument("--energy-only", action="store_true")
    p.add_argument("--shard", default="geometries", choices=["geometries", "pairs"],
                   help="what is distributed over the ranks when --gpus N > 1")
    p.add_argument("--no-second-mode", action="store_true", help="N > 1: skip the leg for the other --shard mode")
    p.add_argument("--integrals", default="packed", choices=["packed", "full"],
                   help="two-electron AO integrals of the sym8 legs: packed as PySCF delivers them with aosym='s4' "
                        "(int2e, EVC_FLAG_ERI_S4) and aosym='s2kl' (int2e_ip1, EVC_FLAG_IP1_S2KL), or the full "
                        "(N,N,N,N) / (3,N,N,N,N) arrays; other layouts always take the full arrays")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the LAST timed step of the headline leg computed on rank 0 "
                        "as DIR/<name>.npy (float64): `energy` (G,) ground-state energies and, unless --energy-only, "
                        "`grad` (G,A,3) nuclear gradients; the inputs depend only on the arguments")
    return p.parse_args()


def cpu_baseline(workload, layout_nd, trd, aos, samples):
    """Time the numpy oracle (a restatement of the reference's CPU algorithm, kind="port") on the
    host cores for a bounded sample of the same workload."""
    from oracle import evcont_oracle as orc
    n, A, T, _ = WORKLOADS[workload]
    if layout_nd == 8:
        # the CPU path works on the reference's own layout: the pack2 rows the compressed set was built from
        two, layout_nd = trd.source_rows().cpu().numpy(), 2
    else:
        two = trd.two[: trd.rows_local, : trd.cols].cpu().numpy()
    if layout_nd == 6:
        two = two.reshape(T, T, n, n, n, n)
    elif layout_nd == 5:
        two = two.reshape(-1, n, n, n, n)
    elif layout_nd == 3:
        two = two.reshape(T, T, -1)
    one = trd.one[:, : n * n].cpu().numpy().reshape(T, T, n, n)
    S = trd.S.cpu().numpy()
    times = []
    for k in range(samples + 1):
        ao = aos[k % len(aos)]
        b = orc.AOBundle(S=ao.S.cpu().numpy(), hcore=ao.hcore.cpu().numpy(), eri=ao.eri.cpu().numpy(),
                         ipovlp=ao.ipovlp.cpu().numpy(), dhcore=ao.dhcore.cpu().numpy(),
                         eri_ip1=ao.eri_ip1.cpu().numpy(), aoslices=ao.aoslices.cpu().numpy(),
                         enuc=ao.enuc, gnuc=ao.gnuc.cpu().numpy())
        t0 = time.perf_counter()
        orc.energy_with_grad(b, one, two, S)
        dt = time.perf_counter() - t0
        if k > 0:           # first call = warm-up (BLAS thread pool, page faults)
            times.append(dt)
    med = float(np.median(times))
    try:
        from threadpoolctl import threadpool_info
        cores = max([d.get("num_threads", 1) for d in threadpool_info()] or [os.cpu_count() or 1])
    except Exception:
        cores = os.cpu_count() or 1
    return {"value": 1.0 / med, "unit": "geometries/s", "cores": int(cores), "kind": "port",
            "sample": f"{samples} energy+force evaluations of the same {workload} workload "
                      f"(layout ndim {layout_nd}) by oracle/evcont_oracle.py (numpy/OpenBLAS), median, after 1 warm-up"}


def self_launch(ngpus):
    """`python bench.py --gpus N` (N > 1) without a launcher: start the N ranks as fresh child processes through
    torch.distributed.run -- nothing in THIS process has touched the GPU yet (torch is imported, no device call) --
    stream their output through and return the launcher's exit code.  Never exec: a child per rank."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // ngpus)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ngpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def main():
    a = parse()
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        sys.exit(self_launch(a.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world:
        a.gpus = world
    # The contract is ONE JSON line on stdout.  Native libraries write there too (RCCL prints a five-line version
    # banner when its first communicator comes up): file descriptor 1 is pointed at stderr for the whole run and the
    # JSON line goes to the saved descriptor of the real stdout.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    assert torch.cuda.is_available(), "bench.py needs a HIP device"
    # EVC_BENCH_BACKEND=gloo lets several ranks share one card (rehearsal on a one-GPU box); RCCL needs a card per rank
    backend = os.environ.get("EVC_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    assert backend != "nccl" or world <= ndev, f"{world} ranks but {ndev} visible devices"
    dev = torch.device("cuda", local_rank % ndev)
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from evcont_amd import _lib
    from evcont_amd.evaluator import (DeviceTRDMs, ContinuationEvaluator, BatchedEvaluator, DeviceAOBatch,
                                      layout_shape)
    from evcont_amd.distributed import PairShardedContinuation, shard_rows
    from evcont_amd.synthetic import make_device_ao, make_device_trdm_rows

    n, A, T, sizes = WORKLOADS[a.workload]
    nd = LAYOUT_ND[a.layout]
    rows, cols = layout_shape(nd, T, n)
    seed = 1234 + list(WORKLOADS).index(a.workload)
    lib = _lib.load()

    def trdms(row_range, nd=nd):
        src_nd = 2 if nd == 8 else nd
        S_train, one, two_rows = make_device_trdm_rows(n, T, src_nd, seed, dev, row_range)
        t = DeviceTRDMs.from_device_rows(one, two_rows, S_train, src_nd, row_range[0], rows)
        if nd == 8:
            del two_rows
            t.compress_sym8_()
            t.source_rows = lambda: make_device_trdm_rows(n, T, 2, seed, dev, row_range)[2]
        return t

    def geometries(first_seed):
        # eri 8-fold symmetric and eri_ip1 symmetric in its last two indices, as real int2e / int2e_ip1 are
        return [make_device_ao(n, A, first_seed + k, dev, sizes, ip1_rs_symmetric=True) for k in range(a.geoms)]

    solo_mode = [False]   # rank 0 measuring alone (the other ranks wait at a barrier behind it): no cross-rank fences

    def fence():
        torch.cuda.synchronize(dev)
        if world > 1 and not solo_mode[0]:
            dist.barrier()
            torch.cuda.synchronize(dev)

    def ensure_group():
        """Pair sharding needs a process group even with one rank (RCCL with world size 1)."""
        if not dist.is_initialized():
            import socket
            with socket.socket() as so:
                so.bind(("127.0.0.1", 0))
                port = so.getsockname()[1]
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            kw = {"device_id": dev} if backend == "nccl" else {}
            dist.init_process_group(backend, init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, **kw)

    def measure(trd, aos, G, nslots, steps, warmup, sharded_pairs, all_stages=False, pipelined=False, repeats=1,
                keep_outputs=False):
        """Time `steps` passes over batches of G geometries with `nslots` batches in flight on this rank, `repeats` times.
        all_stages: time every instrumented stage (two event records per launch), not only K5 and K8.
        keep_outputs: return, under "outputs", host copies of what the last timed step computed."""
        mk_stream = lambda: (torch.cuda.Stream(dev) if nslots > 1 else None)
        if G > 1:
            nb = max(1, len(aos) // G)
            inputs = [DeviceAOBatch.stack([aos[(i * G + j) % len(aos)] for j in range(G)]) for i in range(nb)]
            evs = [BatchedEvaluator(trd, A, G, stream=mk_stream()) for _ in range(nslots)]
        else:
            inputs = aos
            evs = [ContinuationEvaluator(trd, A, stream=mk_stream(), want_two_rdm=False) for _ in range(nslots)]
        if sharded_pairs:
            ensure_group()
            runners = [PairShardedContinuation(ev, rows) for ev in evs]
        else:
            runners = evs
        step = lambda k: runners[k % nslots].enqueue(inputs[k % len(inputs)], 1, a.energy_only)
        if pipelined:
            # ONE caller stream; the library keeps three batches in flight on its own streams
            from evcont_amd.evaluator import PipelinedBatchedEvaluator
            pe = PipelinedBatchedEvaluator(trd, A, G, depth=3)
            evs = pe.evs
            runners = [pe]
            tickets = []

            def step(k):
                if len(tickets) >= pe.depth:
                    pe.results(tickets.pop(0))       # the caller's stream joins the batch whose slot is reused
                tickets.append(pe.enqueue(inputs[k % len(inputs)], energy_only=a.energy_only))
        # set-up, not a step: every slot's evaluator is touched once (first-use kernel attributes, first touch of its
        # workspace), so that a small --warmup does not leave that inside the timed region of the other streams
        for k in range(nslots):
            step(k)
        fence()
        for k in range(warmup):
            step(k)
        fence()
        _lib.check(lib.evc_profile_select(0xFF if all_stages else 0x3), "evc_profile_select")
        _lib.check(lib.evc_profile_begin(steps * repeats), "evc_profile_begin")
        dts = []
        for rep in range(repeats):
            t0 = time.perf_counter()
            for k in range(steps):
                step(warmup + rep * steps + k)
            fence()
            dts.append(time.perf_counter() - t0)
        outputs = None
        if keep_outputs:
            # the slot of the last timed step, read before anything else is enqueued on it
            assert not pipelined and steps >= 1
            ev_ = evs[(warmup + repeats * steps - 1) % nslots]
            outputs = {"energy": ev_.energy.reshape(-1, T)[:, 0].cpu().numpy().astype(np.float64)}
            if not a.energy_only:
                outputs["grad"] = ev_.grad.reshape(-1, max(A, 1), 3)[:, :A].cpu().numpy().astype(np.float64)
        if world > 1 and not solo_mode[0]:
            # max over ranks, repeat by repeat
            tt = torch.tensor(dts, dtype=torch.float64, device=dev)
            every = [torch.zeros_like(tt) for _ in range(world)]
            dist.all_gather(every, tt)
            dts_rank = [[float(x) for x in e.tolist()] for e in every]
            dts = [max(col) for col in zip(*dts_rank)]
        else:
            dts_rank = [list(dts)]
        dt = float(np.median(dts))
        rows_ms, cols_ms = C.c_double(), C.c_double()
        rows_n, cols_n = C.c_int(), C.c_int()
        _lib.check(lib.evc_profile_end(C.byref(rows_ms), C.byref(rows_n), C.byref(cols_ms), C.byref(cols_n)),
                   "evc_profile_end")
        stages = {}   # mean duration per launch of every instrumented stage (HIP events on the launch stream)
        for name, sid in _lib.PROF_STAGES.items():
            ms_, n_ = C.c_double(), C.c_int()
            _lib.check(lib.evc_profile_stage(sid, C.byref(ms_), C.byref(n_)), "evc_profile_stage")
            if n_.value:
                stages[name + "_ms"] = ms_.value / n_.value
        e_last = float(evs[0].energy.reshape(-1)[0].item())
        assert np.isfinite(e_last), "non-finite energy in the timed region"
        # one more, untimed evaluation of the FIRST input: a number that can be compared between legs
        if pipelined:
            slot_ = runners[0].enqueue(inputs[0], energy_only=a.energy_only)
            fence()
            e_check = float(runners[0].results(slot_).energy.reshape(-1)[0].item())
        else:
            runners[0].enqueue(inputs[0], 1, a.energy_only)
            fence()
            e_check = float(evs[0].energy.reshape(-1)[0].item())
        # every rank's own rate (its G geometries per step over the median of ITS wall times)
        per_rank = [steps * G / float(np.median(r)) for r in dts_rank]
        k5_name, gl = k5_launch_info(lib, G)                       # the kernel that ran, geometries per K5 launch (K8: <= 32)
        k8_name = lib.evc_profile_kernel(1).decode()
        pt_name = lib.evc_profile_kernel(2).decode()
        lps = -(-G // gl)                                          # K5 launches per step
        gl8, lps8 = min(G, MAX_G_PER_LAUNCH), -(-G // MAX_G_PER_LAUNCH)
        # ALGORITHMIC bytes of one K5 / K8 launch: the local two-body rows + the one-body t-RDM once,
        # plus one h2 (K5) / predicted-RDM (K8) vector per geometry of the launch
        nbytes = trd.rows_local * trd.cols * 8 + T * T * n * n * 8 + gl * (trd.cols * 8 + n * n * 8)
        nbytes8 = trd.rows_local * trd.cols * 8 + T * T * n * n * 8 + gl8 * (trd.cols * 8 + n * n * 8)
        k5 = rows_ms.value / max(rows_n.value, 1) / lps
        k8 = cols_ms.value / max(cols_n.value, 1) / lps8 if cols_n.value else None
        # geometries evaluated by the whole job per step: G on every rank (distinct ones unless pair-sharded)
        job_g = G if (sharded_pairs or world == 1 or solo_mode[0]) else G * world
        return {"value": steps * job_g / dt, "ms_per_step": 1e3 * dt / steps, "batch": G, "streams": nslots,
                "repeat_values": [steps * job_g / x for x in dts],
                "k5_ms": k5, "k8_ms": k8, "bytes_per_launch": nbytes, "launches": rows_n.value * lps,
                "geometries_per_launch": gl, "k5_GBs": nbytes / (k5 * 1e-3) / 1e9,
                "k5_kernel": k5_name, "k8_kernel": k8_name, "pt_kernel": pt_name,
                "k8_GBs": (nbytes8 / (k8 * 1e-3) / 1e9) if k8 else None, "last_energy": e_last, "check_energy": e_check,
                "k5_flops_per_launch": 2.0 * trd.rows_local * trd.cols * gl,
                "stages": stages, "per_rank": per_rank,
                "geometries_per_step": job_g, "outputs": outputs}

    def step_roofline(ms_per_step, geoms, k5_per_launch):
        """Whole step against the two rooflines at once: ALGORITHMIC bytes (the resident t-RDMs twice, the AO inputs
        of every geometry once, the results) at the HBM peak PLUS the FP64 matrix work of the four-index rotations and
        the two batched contractions at the MFMA peak, over the measured time of a step on ONE GPU."""
        packed_in = a.layout == "sym8" and a.integrals == "packed" and n <= 64
        npr = n * (n + 1) // 2
        ao = (npr * npr + 3 * n * n * npr if packed_in else 4 * n ** 4) + (2 + 3 + 3 * A) * n * n + 3 * A
        passes = 1 if a.energy_only else 2
        # passes over the resident t-RDMs: K5 (up to 64 geometries each) and, with forces, K8 (up to 32 each)
        l5 = -(-geoms // max(1, k5_per_launch))   # (geometries per K5 launch: what the library launched)
        l8 = 0 if a.energy_only else -(-geoms // MAX_G_PER_LAUNCH)
        nbytes = 8.0 * ((l5 + l8) * (rows * cols + T * T * n * n) + geoms * ao + geoms * (3 * A + T))
        lead = npr if a.layout == "sym8" else n * n
        flops_rot = geoms * (2 if a.energy_only else 4) * lead * 4.0 * n ** 3
        flops_con = passes * 2.0 * rows * cols * geoms
        flops = flops_rot + flops_con
        # the two contractions stream the t-RDMs AND multiply them on the matrix cores in the same kernels: each is
        # bounded by the larger of its two rooflines, not by their sum; everything else: bytes at the HBM peak plus the
        # rotations' flops at the MFMA peak
        bytes_con = 8.0 * (l5 + l8) * (rows * cols + T * T * n * n)
        t_con = max(bytes_con / (HBM_PEAK_GBS * 1e9), flops_con / (MFMA_F64_PEAK_TFLOPS * 1e12))
        t_min = t_con + (nbytes - bytes_con) / (HBM_PEAK_GBS * 1e9) + flops_rot / (MFMA_F64_PEAK_TFLOPS * 1e12)
        return {"frac": t_min / (ms_per_step * 1e-3), "bytes_per_step": nbytes, "flops_per_step": flops,
                "ms_at_peaks": t_min * 1e3, "ms_per_step": ms_per_step,
                "note": "max(t-RDM bytes / 8 TB/s, contraction flops / 78.6 TFLOP/s) for the two batched contractions "
                        "+ all other bytes / 8 TB/s + rotation flops / 78.6 TFLOP/s, over the measured step (per GPU); "
                        "FP64 MFMA reaches 77 TFLOP/s with ArchVGPR accumulators (profiles/mfma_f64_regclass.txt)"}

    G, S = max(1, a.batch), max(1, a.streams)
    pairs_first = world > 1 and a.shard == "pairs"
    full_range, my_range = (0, rows), shard_rows(rows, world, rank)
    # geometry sharding: every rank draws its own geometries; pair sharding: all ranks see the same ones
    trd = trdms(my_range if pairs_first else full_range)
    aos = geometries(seed * 1000 + (0 if pairs_first else rank * a.geoms))
    # what the sym8 legs are fed: the same integrals with int2e_ip1 packed in (r,s), gathered on the device here,
    # outside every timed region -- the form PySCF delivers with aosym="s2kl"
    packed_ip1 = a.layout == "sym8" and a.integrals == "packed" and n <= 64
    # (the phase entry points of the pair-sharded mode take the same packed arrays: flags since ABI 7)
    run_view = ((lambda lst, phases=False: [x.packed_ip1(eri=True) for x in lst]) if packed_ip1
                else (lambda lst, phases=False: lst))
    aos_run = run_view(aos, pairs_first)
    m = measure(trd, aos_run, G, 1 if pairs_first else S, a.steps, a.warmup, pairs_first, repeats=max(1, a.repeats),
                keep_outputs=a.dump_outputs is not None)
    if a.dump_outputs is not None and rank == 0:
        os.makedirs(a.dump_outputs, exist_ok=True)
        for name, arr in m["outputs"].items():
            np.save(os.path.join(a.dump_outputs, f"{name}.npy"), arr)

    # The headline is quoted on the LDS-ring K5 kernel, which needs >= 250 CUs (csrc/gemv_lds.hip: lds_device_fits); on a
    # smaller or partitioned device the library falls back to the fragment-shaped kernel.  That is a different measurement:
    # refuse to print a headline for it unless the fallback was asked for by name.
    if (a.workload == "H30" and a.layout == "sym8" and G >= 12 and not pairs_first and not os.environ.get("EVC_ROWS_LDS")
            and not os.environ.get("EVC_BENCH_ALLOW_FALLBACK") and not m["k5_kernel"].startswith("gemv_rows_lds_kernel")):
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        raise SystemExit(f"bench.py: K5 ran as `{m['k5_kernel']}` instead of gemv_rows_lds_kernel on rank {rank} "
                         f"({cus} CUs visible; the LDS-ring kernel needs >= 250): this is not the configuration the "
                         f"headline is defined on.  Set EVC_BENCH_ALLOW_FALLBACK=1 to measure the fallback anyway.")

    out = None
    if rank == 0:
        # HBM traffic of one K5 launch: PMC counters cannot be read from inside this process, so the figure comes from
        # the committed rocprofv3 --pmc passes of the same command (profiles/pmc_traffic.json) -- and only while the
        # streaming-kernel sources are byte-identical to the profiled ones; otherwise null
        traffic, traffic_note = None, "no PMC record for this configuration"
        tj = os.path.join(REPO, "profiles", "pmc_traffic.json")
        if os.path.exists(tj):
            try:
                import hashlib
                rec = json.load(open(tj))
                hh = hashlib.sha256()
                for f_ in ("gemv_mfma.hip", "gemv_stream.hip", "gemv_lds.hip"):
                    hh.update(open(os.path.join(REPO, "evcont_amd", "csrc", f_), "rb").read())
                key = f"{a.workload}/{a.layout}/batch{G}/k5"
                if key in rec and not pairs_first:
                    if rec.get("_source_sha256") == hh.hexdigest():
                        traffic = rec[key]["hbm_bytes_per_launch"]
                        traffic_note = f"profiles/pmc_traffic.json, kernel {rec[key]['kernel']}, same kernel sources"
                    else:
                        traffic_note = "profiles/pmc_traffic.json was collected with other kernel sources: not quoted"
            except Exception:
                traffic = None
        what = "energy" if a.energy_only else "energy+force"
        if world == 1:
            par = "single"
        elif pairs_first:
            par = f"pairs{world}: training pairs sharded, all-gather of H rows + all-reduce of the gradient per step"
        else:
            par = f"geometries{world}: replicated t-RDMs, independent batches per GPU, no data-path collective"
        out = {
            "metric": ("continuation geometries/sec (energy+force), H30 STO-3G, 20 training states"
                       if a.workload == "H30" and not a.energy_only else
                       f"continuation geometries/sec ({what}), {a.workload}"),
            "value": m["value"],
            "unit": "geometries/s",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": m["ms_per_step"],
            "repeats": max(1, a.repeats),
            "repeat_values": m["repeat_values"],
            "higher_is_better": True,
            # geometry sharding: the work per GPU is fixed (its own batches) whatever N is -> weak, also at N = 1;
            # pair sharding: one batch for the whole job -> strong
            "scaling": "strong" if pairs_first else "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": f"{a.workload}: N={n} orbitals, A={A} atoms, T={T} training states, "
                                   f"two-body t-RDM layout {a.layout} ({rows}x{cols} f64, "
                                   f"{rows * cols * 8 / 1e9:.3f} GB resident in HBM), int2e_ip1 "
                                   f"{'and int2e packed as PySCF aosym s2kl / s4' if packed_ip1 else 'and int2e full'}, "
                                   f"{a.geoms} resident geometries "
                                   f"per GPU; step = {m['geometries_per_step']} {what} evaluations",
                       "parallelism": par,
                       "geometries_per_step": m["geometries_per_step"], "batch_per_gpu": G, "streams": m["streams"]},
            "roofline": {"bound": "hbm",
                         "kernel": "K5: H_ab = Gamma . h2 (gemv_rows_*_kernel, the 2-RDM x ERI contraction), rank 0",
                         "achieved": m["k5_GBs"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": m["k5_GBs"] / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_note,
                         "region": f"the timed region `value` is measured in ({m['streams']} stream(s); other batches' "
                                   f"kernels share the chip when > 1)",
                         "bytes_per_launch": m["bytes_per_launch"], "ms_per_launch": m["k5_ms"],
                         "launches": m["launches"], "geometries_per_launch": m["geometries_per_launch"],
                         # the symbol the library launched for K5 in this region (evc_profile_kernel), not the profile's
                         "kernel_ran": m["k5_kernel"]},
            "kernels": {"k5_rows_ms": m["k5_ms"], "k8_cols_ms": m["k8_ms"], "k8_cols_GBs": m["k8_GBs"],
                        "k5_kernel_ran": m["k5_kernel"], "k8_kernel_ran": m["k8_kernel"],
                        "pair_transform_kernel_ran": m["pt_kernel"]},
            "last_energy": m["last_energy"],
            "roofline_step": step_roofline(m["ms_per_step"], m["geometries_per_step"] if world == 1 else G,
                                           m["geometries_per_launch"]),
            # what the collectives library itself reports, and what each rank delivered on its own clock: in the
            # geometry-sharded job a rank's figure is directly comparable with the N=1 run of the same command
            "ranks_seen": dist.get_world_size() if world > 1 else 1,
            "backend": (dist.get_backend() if world > 1 else None),
            "visible_devices": ndev,
            "per_rank_value": m["per_rank"],
        }
    if world > 1 and not a.no_second_mode:
        # the other way of using the node, same batch size, reported next to the headline
        del trd
        torch.cuda.empty_cache()
        second_pairs = not pairs_first
        trd2 = trdms(my_range if second_pairs else full_range)
        del aos
        # pair sharding needs identical geometries on all ranks, geometry sharding distinct ones
        aos2 = geometries(seed * 1000 + (0 if second_pairs else rank * a.geoms))
        aos_run = run_view(aos2, second_pairs)
        m2 = measure(trd2, aos_run, G, 1 if second_pairs else S, a.steps, a.warmup, second_pairs,
                     repeats=max(1, a.repeats))
        if rank == 0:
            out["pair_sharded" if second_pairs else "geometry_sharded"] = {
                "value": m2["value"], "unit": "geometries/s", "ms_per_step": m2["ms_per_step"],
                "repeat_values": m2["repeat_values"],
                "scaling": "strong" if second_pairs else "weak", "geometries_per_step": m2["geometries_per_step"],
                "batch_per_gpu": G, "streams": m2["streams"], "k5_rows_ms": m2["k5_ms"], "k5_GBs": m2["k5_GBs"],
                "k5_frac": m2["k5_GBs"] / HBM_PEAK_GBS, "k8_cols_ms": m2["k8_ms"],
                "rows_per_rank": (my_range[1] - my_range[0]) if second_pairs else rows,
                "last_energy": m2["last_energy"]}
        # the same two jobs on ONE GPU of this node, measured by rank 0 alone while the other ranks wait: the N = 1
        # reference each mode's efficiency is taken against (the driver computes its own from separate runs)
        del trd2
        torch.cuda.empty_cache()
        solo = None
        if rank == 0:
            solo_mode[0] = True
            trd1 = trdms(full_range)
            v1 = run_view(geometries(seed * 1000), False)
            g1 = measure(trd1, v1, G, S, a.steps, a.warmup, False, repeats=max(1, a.repeats))
            solo = {"geometries": g1["value"]}
            solo_mode[0] = False
            geo_v = out["value"] if not pairs_first else out["geometry_sharded"]["value"]
            pair_v = out["value"] if pairs_first else out["pair_sharded"]["value"]
            out["n1_same_run"] = {
                "value": g1["value"], "unit": "geometries/s", "repeat_values": g1["repeat_values"],
                "note": "rank 0 alone (other ranks idle at a barrier): same batch size and streams on one GPU"}
            out["efficiency_vs_n1"] = {"geometry_sharded": geo_v / (world * g1["value"]),
                                       "pair_sharded": pair_v / (world * g1["value"]),
                                       "note": "job rate / (N x the one-GPU rate of this run); pair sharding only "
                                               "divides the two streaming kernels, the rest of a step is replicated "
                                               "(DESIGN.md section 6)"}
            del trd1, v1
        dist.barrier()
        torch.cuda.synchronize(dev)
        trd = None
    if world == 1 and not a.no_md_regime and S > 1:
        # the same batches on ONE stream: the streaming kernels without another batch's kernels beside them
        # twice: `one` with only K5 / K8 bracketed by events (as the headline region; its rate is the leg's `value`),
        # `stg` with every instrumented stage bracketed (two event records per launch cost the stream ~8 % of its rate)
        one = measure(trd, aos_run, G, 1, max(10, a.steps // 2), 3, False)
        stg = measure(trd, aos_run, G, 1, max(10, a.steps // 2), 3, False, all_stages=True)
        pipe = measure(trd, aos_run, G, 1, max(10, a.steps // 2), 3, False, pipelined=True) if G > 1 else None
        if rank == 0:
            if pipe is not None:
                out["single_stream_pipelined"] = {
                    "value": pipe["value"], "unit": "geometries/s", "ms_per_step": pipe["ms_per_step"],
                    "note": "ONE caller stream; the library keeps three batches in flight on its internal streams and the "
                            "caller's stream joins a batch when its results are asked for "
                            "(evaluator.PipelinedBatchedEvaluator, depth 3)"}
            out["single_stream"] = {"value": one["value"], "unit": "geometries/s", "ms_per_step": one["ms_per_step"],
                                    "value_all_stages_timed": stg["value"],
                                    "note": "same batch size, one stream: kernels of one batch at a time; "
                                            "`value_all_stages_timed`: the same with every stage bracketed by events "
                                            "(the pass `stages_ms_per_launch` comes from)",
                                    "k5_rows_ms": one["k5_ms"], "k5_GBs": one["k5_GBs"],
                                    "k5_frac": one["k5_GBs"] / HBM_PEAK_GBS, "k8_cols_ms": one["k8_ms"],
                                    "k8_GBs": one["k8_GBs"], "k8_frac": one["k8_GBs"] / HBM_PEAK_GBS}
            # `roofline` describes K5 inside the headline region; the same kernel with the device to itself:
            out["roofline"]["uncontended"] = {
                "achieved": one["k5_GBs"], "frac": one["k5_GBs"] / HBM_PEAK_GBS, "ms_per_launch": one["k5_ms"],
                "launches": one["launches"], "kernel_ran": one["k5_kernel"],
                "region": "single_stream leg (HIP events on the launch stream, same batches, one stream)"}
            # the other multi-workgroup stages of the same leg, against their own rooflines
            st = stg["stages"]
            out["single_stream"]["stages_ms_per_launch"] = st
            others = []
            if "pair_transform_ms" in st and n <= 32:
                pairs = n * (n + 1) // 2 if a.layout == "sym8" else n * n
                flops = G * pairs * 4.0 * n ** 3          # two N x N x N products per leading pair, unpadded
                tf = flops / (st["pair_transform_ms"] * 1e-3) / 1e12
                others.append({"kernel": f"{stg['pt_kernel']}: one fused pair step of a four-index rotation (4 launches "
                                         "per evaluation, the largest share of the step)", "bound": "mfma",
                               "achieved": tf, "peak": MFMA_F64_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": tf / MFMA_F64_PEAK_TFLOPS, "flops_per_launch": flops,
                               "ms_per_launch": st["pair_transform_ms"]})
            if "ip1_ms" in st and not a.energy_only:
                # bytes the kernel has to read: int2e_ip1 and the AO-basis 2-RDM, lower triangles only with sym8
                tri = (n + 1) / (2.0 * n) if a.layout == "sym8" else 1.0
                nb = G * (3 * n ** 4 * tri + n ** 4 * tri * (tri if a.layout == "sym8" else 1.0)) * 8.0
                gbs = nb / (st["ip1_ms"] * 1e-3) / 1e9
                others.append({"kernel": "ip1_dh_kernel: int2e_ip1 : 2-RDM(AO) contraction", "bound": "hbm",
                               "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                               "bytes_per_launch": nb, "ms_per_launch": st["ip1_ms"]})
            out["roofline_other_kernels"] = others
    if world == 1 and not a.no_md_regime and G > 1:
        # the pair-sharded mode (phases + all-gather of the H rows + all-reduce of the gradient)
        # with ONE rank: the same phases, the same two collectives through the same backend (RCCL), on this GPU
        try:
            ps1 = measure(trd, aos_run, G, 1, max(10, a.steps // 2), 3, True)
            psS = measure(trd, aos_run, G, S, max(10, a.steps // 2), 3, True) if S > 1 else None
            if rank == 0:
                out["pair_sharded"] = {
                    "value": ps1["value"], "unit": "geometries/s", "ms_per_step": ps1["ms_per_step"], "scaling": "strong",
                    "world": 1, "backend": dist.get_backend(), "streams": 1, "k5_rows_ms": ps1["k5_ms"],
                    "k8_cols_ms": ps1["k8_ms"], "check_energy": ps1["check_energy"],
                    "energy_difference_vs_fused": abs(ps1["check_energy"] - m["check_energy"]),
                    "value_streams": (psS["value"] if psS else None), "streams_in_flight": S,
                    "note": "pair-sharded phases + both collectives with one rank, one stream: to be compared with "
                            "`single_stream.value` (the fused entry point on one stream); `value_streams`: the same "
                            "with several batches in flight, to be compared with `value`"}
        except Exception as exc:   # a collectives backend that cannot start must not take the headline down
            if rank == 0:
                out["pair_sharded"] = {"value": None, "error": repr(exc)}
    if world == 1 and not a.no_md_regime and G == 32 and len(aos_run) >= 64:
        # twice the geometries per step: K5 then contracts 64 per pass over the t-RDM (four geometry sets,
        # csrc/gemv_lds.hip) and is bound by its MFMAs instead of the HBM stream; K8 and everything else as before
        try:   # (a supplementary leg must not take the headline down)
            b64 = measure(trd, aos_run, 64, S, max(10, a.steps // 2), max(2, a.warmup // 2), False, repeats=3)
            if rank == 0:
                out["batch64"] = {"value": b64["value"], "unit": "geometries/s", "ms_per_step": b64["ms_per_step"],
                                  "repeat_values": b64["repeat_values"], "streams": S,
                                  "k5_geometries_per_launch": b64["geometries_per_launch"],
                                  "k5_rows_ms_contended": b64["k5_ms"], "k5_bytes_per_launch": b64["bytes_per_launch"],
                                  "k5_flops_per_launch": b64["k5_flops_per_launch"],
                                  "note": "the default configuration with 64 geometries per step (never `value`)"}
        except Exception as exc:
            if rank == 0:
                out["batch64"] = {"value": None, "error": repr(exc)}
    if world == 1 and not a.no_md_regime and (G, S) != (1, 1):
        md = measure(trd, aos_run, 1, 1, max(20, min(a.steps * 2, 200)), 10, False)
        if rank == 0:
            out["md_regime"] = {"value": md["value"], "unit": "geometries/s", "ms_per_step": md["ms_per_step"],
                                "note": "one geometry per step on one stream (no batching, no overlap)",
                                "k5_rows_ms": md["k5_ms"], "k5_GBs": md["k5_GBs"], "k5_frac": md["k5_GBs"] / HBM_PEAK_GBS,
                                "k8_cols_ms": md["k8_ms"], "k8_GBs": md["k8_GBs"]}
    if world == 1 and not a.no_md_regime and not a.energy_only:
        # the same one-geometry-per-step regime with the integrals arriving from the HOST every step, as in an MD run
        # driven by PySCF (MD_utils.py:40-55): pinned staging buffers -> H2D inside the timed region -> one HIP graph
        # per step (evcont_amd/hosted.py).  Four evaluators with four different staged geometries are cycled, cold
        # start (comparable with md_regime); the host-side production of the integrals is not part of the path.
        from evcont_amd.hosted import HostedEvaluator
        hevs = []
        for k in range(4):
            src = aos[k]
            hv = HostedEvaluator(trd, A, src.aoslices.cpu().numpy(), warm_start=False)
            run = src.packed_ip1(eri=True) if hv.packed else src
            st_ = hv.staging()
            for name in ("S", "hcore", "ipovlp", "dhcore", "gnuc", "eri", "eri_ip1"):
                np.copyto(st_[name], getattr(run, name).cpu().numpy().reshape(st_[name].shape))
            st_["enuc"][0] = src.enuc
            for _ in range(3):
                hv.run()               # two eager calls, then the capture
            hevs.append(hv)
        fence()
        nst = max(20, min(a.steps * 2, 200))
        reps_h = []
        for _ in range(5):      # (single runs of this host-paced leg scatter from box to box: median and best of five)
            t0 = time.perf_counter()
            for k in range(nst):
                e_h, _ = hevs[k % 4].run()
            fence()
            reps_h.append(nst / (time.perf_counter() - t0))
        val_h = sorted(reps_h)[len(reps_h) // 2]
        up_bytes = sum(v.numel() * 8 for v in hevs[0].host.values())
        if rank == 0:
            out["md_hosted"] = {"value": val_h, "unit": "geometries/s", "ms_per_step": 1e3 / val_h,
                                "repeat_values": reps_h, "best": max(reps_h), "zero_copy_inputs": hevs[0].zero_copy,
                                "h2d_bytes_per_step": up_bytes, "graph": hevs[0].graph is not None,
                                "note": "one geometry per step, AO integrals in pinned HOST memory, uploaded inside the "
                                        "timed region (two uploads, the late one on a forked stream; one download; "
                                        "small systems (`zero_copy_inputs`): no copies at all, the kernels read the "
                                        "pinned staging buffers and write the results into pinned memory; "
                                        "`graph`: whether the step is replayed as a HIP graph, "
                                        "EVCONT_AMD_HOSTED_GRAPH); cold start; PCIe-inclusive, never `value`"}
        del hevs
    if world == 1 and not a.no_md_regime and not a.energy_only and a.layout == "sym8" and n <= 64 \
            and not os.environ.get("EVCONT_AMD_COMPRESS"):
        # The reference's call pattern, unchanged: `scanner = MD_utils.get_scanner(mol, one_rdm, two_rdm, overlap)`
        # with the container's 6-index arrays (FCI_EVCont.py:106-131; 2.6 GB on the HOST at H30 / T = 20) and then
        # `scanner(mol)` once per step (MD_utils.py:40-57) -- no extra arguments, no environment.  `mol` is an
        # array-level molecule (evcont_amd.synthetic.AOArrays, product code) that holds its two large integral arrays
        # packed in pinned memory, as an integral producer writing into caller-supplied buffers leaves them.
        try:
            from evcont_amd.MD_utils import get_scanner
            from evcont_amd.synthetic import AOArrays
            from evcont_amd import ops, cache
            import evcont_amd.ab_initio_eigenvector_continuation as aec
            S_d, one_d, rows2 = make_device_trdm_rows(n, T, 2, seed, dev, full_range)
            two6 = torch.empty((T, T, n, n, n, n), dtype=torch.float64, device=dev)
            r_ = 0
            for ia in range(T):
                for ib in range(ia + 1):
                    g4 = ops.unpack_pair_sym(rows2[r_], n)
                    two6[ia, ib] = g4
                    if ib != ia:
                        two6[ib, ia] = g4.permute(1, 0, 3, 2)
                    r_ += 1
            del rows2
            one_h, S_h, two_h = one_d.cpu().numpy(), S_d.cpu().numpy(), two6.cpu().numpy()
            del two6
            torch.cuda.empty_cache()
            host = lambda x: x.cpu().numpy()
            mols = [AOArrays(host(g_.S), host(g_.hcore), host(g_.eri), host(g_.ipovlp), host(g_.dhcore),
                             host(g_.eri_ip1), host(g_.aoslices), float(g_.enuc), host(g_.gnuc),
                             integral_symmetry=True).pinned_packed() for g_ in aos[:4]]
            fence()
            t0 = time.perf_counter()
            sc = get_scanner(mols[0], one_h, two_h, S_h)
            e_first, _ = sc(mols[0])
            first_s = time.perf_counter() - t0
            for k in range(8):
                sc(mols[k % 4])
            nst = max(20, min(a.steps * 2, 200))
            reps_a = []
            for _ in range(5):
                t0 = time.perf_counter()
                for k in range(nst):
                    e_a, _ = sc(mols[k % 4])
                reps_a.append(nst / (time.perf_counter() - t0))
            val_a = sorted(reps_a)[len(reps_a) // 2]
            e0_again, g_api = sc(mols[0])
            # the forces of the same geometry from a device-resident evaluator (one fused call, no staging)
            from evcont_amd.evaluator import BatchedEvaluator as _BE, DeviceAOBatch as _DB
            _, g_res = _BE(trd, A, 1).energies_with_grads(_DB.stack([aos_run[0]]))
            if rank == 0:
                out["api_default"] = {
                    "value": val_a, "unit": "geometries/s", "ms_per_step": 1e3 / val_a, "repeat_values": reps_a,
                    "best": max(reps_a), "first_call_s": first_s,
                    "compressed_evaluator_used": bool(sc._hev is not None and sc._hev.packed),
                    "compression_mode": aec.get_trdm_compression(),
                    "uploads_from_producer_buffers": bool(sc._hev._direct_slabs is not None
                                                          or all(v is not None for v in sc._hev._direct.values())),
                    "host_two_rdm_bytes": int(two_h.nbytes),
                    "energy_difference_vs_headline": abs(e0_again - m["check_energy"]),
                    "force_difference_vs_resident": float(np.abs(np.asarray(g_api) - g_res[0]).max()),
                    "vs_md_hosted": (val_a / out["md_hosted"]["value"]) if "md_hosted" in out else None,
                    "note": "evcont_amd.MD_utils.get_scanner(mol, one_rdm, two_rdm, overlap)(mol) exactly as the "
                            "reference is called (6-index host arrays, default arguments, no environment): first call "
                            "(upload of the 6-index t-RDMs, 8-fold compression on the device, evaluator set-up) "
                            "reported as `first_call_s`, then one call per step, eigensolvers warm-started as the "
                            "scanner does; host-paced, PCIe-inclusive, never `value`"}
            del sc, two_h, mols
            cache.clear()
        except Exception as exc:   # a supplementary leg must not take the headline down
            if rank == 0:
                out["api_default"] = {"value": None, "error": repr(exc)}
    if world == 1 and not a.no_md_regime and not a.energy_only:
        # an MD-like sequence: geometries that change slowly from step to step (linear blend of two of the
        # synthetic geometries in 0.1 % steps), one per step on one stream, the eigensolvers warm-started
        # from the previous step (EVC_FLAG_WARM_START) as evcont_amd.MD_utils.get_scanner does
        from evcont_amd.evaluator import DeviceAO
        a0, a1 = aos_run[0], aos_run[1]
        assert not a0.eri_s4 or a0.eri.dim() == 2
        nsteps = 40
        lerp = lambda x, y, t: torch.lerp(x, y, t)
        traj = [DeviceAO(S=lerp(a0.S, a1.S, t), hcore=lerp(a0.hcore, a1.hcore, t), eri=lerp(a0.eri, a1.eri, t),
                         enuc=(1 - t) * a0.enuc + t * a1.enuc, natm=a0.natm, ipovlp=lerp(a0.ipovlp, a1.ipovlp, t),
                         dhcore=lerp(a0.dhcore, a1.dhcore, t), eri_ip1=lerp(a0.eri_ip1, a1.eri_ip1, t),
                         gnuc=lerp(a0.gnuc, a1.gnuc, t), aoslices=a0.aoslices, ip1_s2kl=a0.ip1_s2kl, eri_s4=a0.eri_s4)
                for t in (1e-3 * k for k in range(nsteps))]
        res = {}
        for name, warm in (("cold", False), ("warm", True)):
            ev = ContinuationEvaluator(trd, A, warm_start=warm, want_two_rdm=False)
            for k in range(8):
                ev.enqueue(traj[k])
            fence()
            t0 = time.perf_counter()
            for k in range(8, nsteps):
                ev.enqueue(traj[k])
            fence()
            res[name] = (nsteps - 8) / (time.perf_counter() - t0)
            res[name + "_E"] = float(ev.energy[0].item())
        del traj
        if rank == 0:
            out["md_trajectory"] = {"value": res["warm"], "unit": "geometries/s", "cold_start_value": res["cold"],
                                    "note": "one slowly varying geometry per step, one stream, eigensolvers "
                                            "warm-started from the previous step; cold_start_value = same sequence "
                                            "without warm start", "energy_difference": abs(res["warm_E"] - res["cold_E"])}
    if world == 1 and not a.no_md_regime and a.layout == "sym8":
        # the reference's own storage layout (pack2, the rows the compressed set was built from): same
        # geometries, batch size and streams
        del trd
        torch.cuda.empty_cache()
        trd = trdms(full_range, nd=2)
        ref = measure(trd, aos, G, S, max(20, a.steps // 2), 5, False)
        if rank == 0:
            out["reference_layout"] = {"layout": "pack2", "value": ref["value"], "unit": "geometries/s",
                                       "ms_per_step": ref["ms_per_step"], "k5_rows_ms": ref["k5_ms"],
                                       "k5_GBs": ref["k5_GBs"], "k5_frac": ref["k5_GBs"] / HBM_PEAK_GBS,
                                       "k8_cols_ms": ref["k8_ms"], "k8_GBs": ref["k8_GBs"],
                                       "bytes_per_launch": ref["bytes_per_launch"],
                                       "energy_difference_vs_sym8": abs(ref["check_energy"] - m["check_energy"]),
                                       "note": "t-RDMs resident in the reference's packed layout "
                                               "(pairs x packed electron pairs), no symmetry compression"}
        nd_cpu = 2
    else:
        nd_cpu = nd
    if rank == 0:
        if not a.no_cpu_baseline and world == 1 and not a.energy_only:
            samples = a.cpu_samples or (2 if a.workload == "Zundel100" else 8 if a.workload in ("H30", "Zundel") else 50)
            out["cpu_baseline"] = cpu_baseline(a.workload, nd_cpu, trd, aos, samples)
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    if world > 1:
        dist.barrier()
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
