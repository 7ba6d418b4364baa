"""Headline benchmark: keyframes/s of the DPVO update loop (altcorr + update
operator + fastba + point cloud) at 512x384 on a 2048-keyframe buffer.

One step = one steady-state DPVO.update() (dpvo/dpvo.py:711-749) over the
C3 workload (dpvo_2k.yaml: M=192, buffer 2048, n=2040 keyframes,
E=95,424 active edges, 2 BA iterations), inputs resident in HBM.
Multi-GPU: one independent sequence per rank (seed = rank), no collective in
the timed region (weak scaling); poses/points are gathered over RCCL after.

  python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the result line.
--dump-outputs DIR also writes what the last timed update() left for its
caller (dump_arrays) as DIR/<name>.npy.  --full adds everything measured
around the headline figure: altcorr events inside the timed loop, the host
calibration, the per-phase breakdown and roofline objects, the CPU baseline
and the end-to-end frames/s.
"""
import argparse
import hashlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(REPO, "wild-video-3d-reconstruction_amd")
for _p in (REPO, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

METRIC = "keyframes/s (altcorr+BA update loop), 512×384, 2048-KF buffer, 1/2/4/8 GPU"
HBM_PEAK_GBS = 8000.0     # MI355X HBM3E spec (MI355X_MICROARCH.md)
MFMA_PEAK_TFLOPS = 2500.0  # dense fp16 MFMA peak (MI355X_MICROARCH.md; no sparsity)
C, P, LEVELS = 128, 3, 2
# algorithmic bytes per edge of the fused 2-level altcorr launch:
# gmap patch + 10x10 level-1 window + 9x9 level-2 window (fp16) + fp16 output + coords + ii/jj
CORR_BYTES_PER_EDGE = 2 * C * (P * P + 10 * 10 + 9 * 9) + 2 * 2 * 49 * P * P + 4 * 2 * P * P + 8 * 2
# the update operator per edge (net.py:75-93): multiply-adds of
# its Linear layers (corr 882 -> 384, then 16 Linear(384, 384): corr x2, c1 x2, c2 x2,
# SoftAgg f, g x2, GatedResidual gate + res x2 twice; d / w heads), and the bytes the
# fused launches move per edge row (inputs read + outputs written, fp16 / fp32 as stored)
UPD_MACS_PER_EDGE = 882 * 384 + 16 * 384 * 384 + 384 * 4
UPD_MACS_PER_GROUP = 384 * 384   # SoftAgg's h Linear runs on the G groups only
UPD_BYTES_PER_EDGE = (
    (1792 + 768)                      # corr chain: corr rows in (896 fp16), h out (fp16)
    + (768 + 1536 + 768 + 1536 + 768)  # corr Linear 3 + RES|LN: h, net32, ctx row in; net32, net16 out
    + 2 * (768 + 1536 + 1536 + 768)    # c1, c2 chains: gathered row, net32 in; net32, net16 out
    + 2 * (768 + 1536)                 # SoftAgg f|g pair GEMMs: net16 in, f16 | g16 out
    + 2 * 1536                         # SoftAgg reduce: f, g rows in
    + (1536 + 768)                     # rowadd (agg_kk): net32 in; net16 out (the fp32 sum is recomputed)
    + (1536 + 1536 + 768)              # rowadd + LN (agg_ij): net32 in; net32, net16 out
    + (768 + 1536 + 1536 + 768)        # gated chain 1: net16, net32 in; net32, net16 out
    + (768 + 1536 + 1536 + 8))         # gated chain 2: net16, net32 in; net32, heads out
COUNTERS_JSON = os.path.join(REPO, "profiles", "counters_c3.json")


def source_sha(*names):
    """hash of the HIP sources a counter record was taken with (the record is
    used only for the same kernel version)"""
    h = hashlib.sha256()
    for n in names:
        with open(os.path.join(PKG, "csrc", n), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


CORR_SOURCES = ("corrmfma.hip", "corrmfma.hpp", "altcorr.hip")
UPD_SOURCES = ("rowgemm.hip", "updateop.hip")


# BASELINE.json configs that fit one GPU: preset, overrides, buffer, BA iterations
CONFIGS = {
    "C3": dict(preset="dpvo_2k", overrides={}, buffer=2048, iterations=2,
               name="C3 dpvo_2k.yaml"),
    "C2": dict(preset="default", overrides={"PATCHES_PER_FRAME": 96}, buffer=512, iterations=8,
               name="C2 default.yaml with M=96 (BASELINE.json)"),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="C3", choices=sorted(CONFIGS),
                    help="C3 (the metric's workload, default) or C2 (512-KF buffer, M=96, 8 BA iterations)")
    ap.add_argument("--buffer", type=int, default=None)
    ap.add_argument("--iterations", type=int, default=None)
    ap.add_argument("--e2e-frames", type=int, default=32, help="--full: end-to-end frames timed after the bench (0: skip)")
    ap.add_argument("--exact-corr", action="store_true", help="the bit-exact fp16-chain altcorr instead of the MFMA one")
    ap.add_argument("--graph", action="store_true",
                    help="replay update() from a HIP graph (captured in the warmup) instead of launching it eagerly")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--cpu-sample-edges", type=int, default=1500)
    ap.add_argument("--counters-json", default=COUNTERS_JSON,
                    help="rocprofv3 counter record of the same kernel versions (scripts/counters_json.py)")
    ap.add_argument("--no-affinity", action="store_true", help="do not pin this rank's host threads")
    ap.add_argument("--full", action="store_true",
                    help="also measure what surrounds the headline figure: altcorr events in the timed loop, host "
                         "calibration, per-phase breakdown, roofline objects, CPU baseline (--no-cpu-baseline, "
                         "--cpu-sample-edges) and end-to-end frames/s (--e2e-frames)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the state the last timed update() produced (rank 0's "
                         "sequence) as DIR/<name>.npy in float32; see dump_arrays")
    return ap.parse_args()


def pin_host_cores(local, local_world):
    """One process per GPU with its own host cores: the CPUs this
    process may use are split into local_world contiguous blocks and rank
    `local` keeps block `local` -- before any GPU call, so the HIP runtime's
    threads inherit it.  Returns the core list (None if not pinned)."""
    try:
        cpus = sorted(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        return None
    if local_world <= 1 or len(cpus) < local_world:
        return cpus
    per = len(cpus) // local_world
    mine = cpus[local * per:(local + 1) * per]
    os.sched_setaffinity(0, mine)
    torch.set_num_threads(max(1, min(len(mine), torch.get_num_threads())))
    return mine


def dist_setup(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    args.cores = None if args.no_affinity else pin_host_cores(local, local_world)
    # one process per GPU; DPVO_BENCH_BACKEND=gloo (collectives through host
    # copies) lets the multi-rank path run with several ranks on one GPU (tests)
    local = local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if _backend() == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(_backend(), rank=rank, world_size=world)
    return world, rank, local


def _backend():
    return os.environ.get("DPVO_BENCH_BACKEND", "nccl")


def barrier(world):
    if world > 1:
        import torch.distributed as dist
        dist.barrier()


def max_over_ranks(value, device):
    """The timed region's wall time: MAX over ranks (the slowest sequence)."""
    import torch.distributed as dist
    if dist.get_backend() == "gloo":
        device = "cpu"
    t = torch.tensor([float(value)], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def gather_to_rank0(tensors, rank, world):
    """gather every rank's result tensors (same shapes on all ranks: one
    sequence per rank) to rank 0; returns [tensor][rank] there."""
    import torch.distributed as dist
    out = []
    for t in tensors:
        t = t.contiguous()
        if dist.get_backend() == "gloo":
            t = t.cpu()
        bufs = [torch.empty_like(t) for _ in range(world)] if rank == 0 else None
        dist.gather(t, bufs, dst=0)
        out.append(bufs)
    return out if rank == 0 else None


DUMP_ARRAY_BYTES = 10 << 20   # per array; six arrays stay under 64 MB in all


def sample_rows(rows, itemsize_row, seed, max_bytes=DUMP_ARRAY_BYTES):
    """all row indices if they fit max_bytes, else a seeded, sorted sample of
    them (the same rows on every run and every build); None means all rows"""
    keep = max_bytes // itemsize_row
    if rows <= keep:
        return None
    return np.sort(np.random.default_rng(seed).choice(rows, size=keep, replace=False))


def dump_arrays(slam):
    """What update() leaves for its caller (it returns nothing: the tracker
    reads its state), as float32 host arrays, rows along the first axis:
      poses   [n, 7]       keyframe poses after BA
      patches [n M, 27]    patches of the n keyframes (BA updates their inverse depths)
      points  [m, 3]       point cloud of the m stored patches
      net     [E, 384]     the update operator's edge state
      target  [E, 2], weight [E, 2]   the BA targets and confidences of the edges
    An array above DUMP_ARRAY_BYTES keeps a fixed seeded sample of its rows
    (sample_rows, seed = position in this list)."""
    n, m = slam.n, slam.pg.m
    full = (("poses", slam.pg.poses_[:n]), ("patches", slam.pg.patches_[:n].reshape(n * slam.M, -1)),
            ("points", slam.pg.points_[:m]), ("net", slam.pg.net[0]), ("target", slam.pg.target[0]),
            ("weight", slam.pg.weight[0]))
    out = {}
    for seed, (name, t) in enumerate(full):
        t = t.reshape(t.shape[0], -1)
        idx = sample_rows(t.shape[0], 4 * t.shape[1], seed)
        if idx is not None:
            t = t[torch.from_numpy(idx).to(t.device)]
        out[name] = t.float().cpu().numpy()
    return out


def write_arrays(path, arrays):
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, f"{name}.npy"), np.ascontiguousarray(a, dtype=np.float32))


class CorrProbe:
    """HIP events around every altcorr call on the stream it runs on: the
    per-edge kernels (corr_pyramid / corr_pyramid_mfma) and the latter's edge
    ordering (cuda_corr.edge_order) when the caller did not supply one."""

    def __init__(self):
        self.pairs = {"corr": [], "order": []}

    def wrap(self, slam):
        import cuda_corr
        from dpvo import altcorr

        def timed(inner, kind):
            def f(*a, **k):
                # (ROCm torch refuses event-record nodes in a graph capture:
                # a captured update() is timed per step only)
                if torch.cuda.is_current_stream_capturing():
                    return inner(*a, **k)
                s = torch.cuda.Event(enable_timing=True)
                e = torch.cuda.Event(enable_timing=True)
                s.record()
                out = inner(*a, **k)
                e.record()
                self.pairs[kind].append((s, e))
                return out
            return f
        altcorr.corr_pyramid = timed(altcorr.corr_pyramid, "corr")
        altcorr.corr_pyramid_mfma = timed(altcorr.corr_pyramid_mfma, "corr")
        cuda_corr.edge_order = timed(cuda_corr.edge_order, "order")

    def clear(self):
        for v in self.pairs.values():
            v.clear()

    def mean_ms(self, kind="corr"):
        ts = [s.elapsed_time(e) for s, e in self.pairs[kind]]
        return float(np.mean(ts)) if ts else 0.0


def _gpu_head_start(ms=2.0):
    """Keep the device busy for ~ms so the host enqueues the launches that
    follow ahead of it: event gaps then measure back-to-back device time, not
    the host's launch pace (small phases otherwise read as Python + ctypes
    enqueue time whenever the GPU has drained)."""
    try:
        torch.cuda._sleep(int(ms * 2.0e6))   # ~2 GHz shader clock
    except (AttributeError, RuntimeError):
        pass


def phase_breakdown(slam, reps=5):
    """Per-phase device time of one update, measured with events outside the
    timed loop.  The phases follow DPVO.update() (dpvo/dpvo.py) step by step,
    with the same arguments: reproject; the window keys and both group-bys
    (dpvo_window_group_by, with altcorr's visiting order); altcorr (the
    per-edge matrix-core kernel in that order); the update operator; the BA
    targets + fastba; the point cloud.  Each rep starts behind a device-side
    delay, so the phases run back to back as in the timed loop."""
    import update_ops
    from dpvo import fastba
    from dpvo import projective_ops as pops
    from dpvo.lietorch import SE3
    ev = lambda: torch.cuda.Event(enable_timing=True)
    names = ("reproject", "group_by", "altcorr", "update_op", "fastba", "point_cloud")
    acc = {k: [] for k in names}
    assert slam._window_keys(), "phase_breakdown follows the window-key path of DPVO.update"
    for _ in range(reps):
        slam._ba_status.zero_()
        e = [ev() for _ in range(len(names) + 1)]
        _gpu_head_start()
        e[0].record()
        coords = slam.reproject()
        e[1].record()
        ctx_idx, jslot, kk_groups, ij_groups, order = update_ops.window_group_by(
            slam.pg.ii, slam.pg.jj, slam.pg.kk, slam.M, slam.n - 64, slam.M * slam.pmem, slam.pmem,
            flag=slam._ba_status, jj_order=True)
        e[2].record()
        with torch.autocast("cuda", enabled=True):
            corr = slam.corr(coords, slots=(ctx_idx, jslot), order=order)
            e[3].record()
            net, (delta, weight, _) = slam.network.update(slam.pg.net, slam.imap, corr, None, slam.pg.ii, slam.pg.jj,
                                                          slam.pg.kk, inp_idx=ctx_idx,
                                                          index_bounds=(slam.N * slam.M, slam.N),
                                                          kk_groups=kk_groups, ij_groups=ij_groups)
        e[4].record()
        target, weight = update_ops.edge_targets(coords[..., P // 2, P // 2], delta, weight)
        fastba.BA(slam.poses, slam.patches, slam.intrinsics, target, weight, slam._lmbda, slam.pg.ii,
                  slam.pg.jj, slam.pg.kk, max(slam.n - slam.cfg.OPTIMIZATION_WINDOW, 1), slam.n,
                  slam.cfg.BA_ITERATIONS, csr=kk_groups[1:], status=slam._ba_status, keep_status=True)
        e[5].record()
        m = slam.pg.m
        pops.point_cloud_centre(SE3(slam.poses), slam.patches[:, :m], slam.intrinsics, slam.ix[:m],
                                out=slam.pg.points_[:m])
        e[6].record()
        torch.cuda.synchronize()
        for k, (a, b) in zip(acc, zip(e[:-1], e[1:])):
            acc[k].append(a.elapsed_time(b))
    slam.check_ba(int(slam._ba_status.item()))
    out = {k: round(float(np.median(v)), 4) for k, v in acc.items()}
    return out


def gmap_pack_ms(slam, reps=5):
    """The matrix-core altcorr's gmap table (dpvo_corr_pack_mfma): packed once
    per NEW keyframe by DPVO.corr (the ring's version changed), so it belongs
    to the frame ingest, not to update(); timed here for the end-to-end
    account."""
    import cuda_corr
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        _gpu_head_start(0.5)
        a.record()
        cuda_corr.pack_mfma(slam.gmap, out=slam._gtab)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return round(float(np.median(ts)), 4)


def host_cost(slam, cores, reps=6):
    """Host CPU per eager update(): the Python thread's CPU time (launches,
    ctypes, torch dispatch) against the GPU time of the same update, from
    updates run back to back behind a device-side delay (so the host never
    waits for the device inside the measured span).  Every rank launches from
    its own thread on its own pinned block of cores (pin_host_cores), so the
    figure that decides whether a rank is launch-bound is its own launching
    thread's share of a step, thread_ms / gpu_ms (1.0 = launch-bound)."""
    slam.update()
    torch.cuda.synchronize()
    _gpu_head_start(20.0)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    c0 = time.thread_time()
    a.record()
    for _ in range(reps):
        slam.update()
    b.record()
    c1 = time.thread_time()
    torch.cuda.synchronize()
    thread_ms = (c1 - c0) / reps * 1e3
    gpu_ms = a.elapsed_time(b) / reps
    return {"thread_ms": round(thread_ms, 4), "gpu_ms": round(gpu_ms, 4),
            "launch_thread_share": round(thread_ms / max(gpu_ms, 1e-6), 3),
            "pinned_cores_per_rank": len(cores) if cores else None}


def load_counters(path, edges):
    """the rocprofv3 counter record (scripts/counters_json.py) if it was
    taken on this workload with the current kernel sources, else None"""
    if not path or not os.path.exists(path):
        return None
    with open(path) as f:
        rec = json.load(f)
    if rec.get("edges") != edges:
        return None
    ok = {"corr": rec.get("sha", {}).get("corr") == source_sha(*CORR_SOURCES),
          "update_op": rec.get("sha", {}).get("update_op") == source_sha(*UPD_SOURCES)}
    return rec, ok


def roofline_lines(slam, corr_ms, order_ms, breakdown, counters, path):
    """The two roofline objects of the bench line.

    altcorr (the matrix-core kernel + its edge ordering): HBM bytes measured
    by rocprofv3 (FETCH_SIZE x 2 + WRITE_SIZE, MI355X_MICROARCH.md's gfx950
    correction) for the same kernel sources, divided by the phase time
    measured here; the PMC shows the kernel bound by its vector-memory address
    path (TA), so `bound` says so and `ta` reports that unit's busy fraction
    from the same record.  The algorithmic bytes (no cross-edge
    reuse) are reported beside it: the edge-grouped kernel reads each target
    frame's window pixels once per XCD L2, so HBM sees ~30 % of them.

    update operator: its fused launches' bytes (counter record when current,
    else the per-launch model UPD_BYTES_PER_EDGE) over the phase time vs HBM
    peak, and its Linear layers' flops vs the dense fp16 MFMA peak."""
    E = slam.pg.ii.numel()
    rec, ok = counters if counters else (None, {"corr": False, "update_op": False})
    phase_ms = corr_ms + order_ms
    alg = CORR_BYTES_PER_EDGE * E
    corr = {"kernel": ("corr_sfast_kernel<2,16> (bit-exact fp16-chain altcorr)" if slam.cfg.EXACT_CORR
                       else "corr_mfma_kernel (2-level altcorr on the matrix cores, edges in the window "
                            "group-by's target-frame order)"),
            "unit": "GB/s", "peak": HBM_PEAK_GBS, "avg_launch_ms": round(phase_ms, 5),
            "kernel_ms": round(corr_ms, 5), "edge_order_ms": round(order_ms, 5),
            "algorithmic_bytes": alg, "algorithmic_GBs": round(alg / (phase_ms * 1e-3) / 1e9, 1),
            "bytes_per_edge": CORR_BYTES_PER_EDGE}
    if ok["corr"] and not slam.cfg.EXACT_CORR:
        c = rec["corr"]
        traffic = c["hbm_bytes_per_launch"]
        achieved = traffic / (phase_ms * 1e-3) / 1e9
        corr.update({"bound": "ta", "achieved": round(achieved, 1), "frac": round(achieved / HBM_PEAK_GBS, 4),
                     "traffic": traffic, "basis": "HBM counter bytes (same kernel sources) / phase time",
                     "ta": {"busy_frac": c.get("ta_busy_frac"),
                            "note": "TA_BUSY_avr / kernel cycles per XCD: the address path is the binding unit"},
                     "counters": os.path.relpath(path, REPO)})
    else:
        achieved = alg / (phase_ms * 1e-3) / 1e9
        corr.update({"bound": "ta", "achieved": round(achieved, 1), "frac": None, "traffic": None,
                     "basis": "no counter record for these kernel sources: algorithmic bytes only (no reuse "
                              "model; not a utilisation)"})
    upd_ms = breakdown["update_op"]
    G = E // 22 + E // slam.M   # SoftAgg groups: ~E / 21.6 patches (497 M edges, 23 M patches) + ~E / M frame pairs
    flops = 2.0 * (UPD_MACS_PER_EDGE * E + UPD_MACS_PER_GROUP * G)
    upd_bytes = UPD_BYTES_PER_EDGE * E
    upd = {"kernel": "update operator (rowchain5 / rowgemm5 / rowadd_ln / sa_reduce_csr launches)",
           "bound": "latency (k-loop + row epilogue; see DESIGN.md)", "unit": "GB/s", "peak": HBM_PEAK_GBS,
           "phase_ms": upd_ms, "algorithmic_bytes": upd_bytes, "flops": flops,
           "tflops": round(flops / (upd_ms * 1e-3) / 1e12, 1), "mfma_peak_tflops": MFMA_PEAK_TFLOPS,
           "mfma_frac": round(flops / (upd_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4)}
    if ok["update_op"]:
        traffic = rec["update_op"]["hbm_bytes_per_update"]
        upd.update({"traffic": traffic, "basis": "HBM counter bytes of the operator's launches / phase time"})
    else:
        traffic = upd_bytes
        upd.update({"traffic": None, "basis": "per-launch byte model (no counter record for these sources)"})
    a = traffic / (upd_ms * 1e-3) / 1e9
    upd.update({"achieved": round(a, 1), "frac": round(a / HBM_PEAK_GBS, 4)})
    return corr, upd


def _core_str(cores):
    """compact core list: '0-15' / '0-3,8-11'"""
    if not cores:
        return None
    runs, start, prev = [], cores[0], cores[0]
    for c in cores[1:] + [None]:
        if c is not None and c == prev + 1:
            prev = c
            continue
        runs.append(f"{start}-{prev}" if prev != start else f"{start}")
        if c is not None:
            start = prev = c
    return ",".join(runs)


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _update_op_cpu_seconds(slam, rows, threads):
    """The learned update operator (net.py:75-93) on the host: the module's
    own layers in fp32 on torch's CPU backend with `threads` intra-op
    threads, over a bounded sample of edge rows (the cost is linear in rows:
    every layer is row-wise except the two SoftAggs, done here with
    scatter_reduce over the sample's own groups); scaled to all edges by the
    caller."""
    import copy
    upd = copy.deepcopy(slam.network.update).float().cpu().eval()
    E = slam.pg.ii.numel()
    idx = torch.linspace(0, E - 1, rows).long()
    dev = slam.device
    net = slam.pg.net[0, idx.to(dev)].float().cpu()
    ctx = slam.imap[0, (slam.pg.kk[idx.to(dev)] % (slam.M * slam.pmem))].float().cpu()
    corr = torch.randn(rows, 882)
    kk = slam.pg.kk[idx.to(dev)].cpu()
    ii, jj = slam.pg.ii[idx.to(dev)].cpu(), slam.pg.jj[idx.to(dev)].cpu()

    def softagg(agg, x, key):
        _, gid = torch.unique(key, return_inverse=True)
        G = int(gid.max()) + 1
        f, g = agg.f(x), agg.g(x)
        gmax = torch.full((G, x.shape[1]), -float("inf")).scatter_reduce(0, gid[:, None].expand_as(g), g, "amax")
        w = torch.exp(g - gmax[gid])
        den = torch.zeros(G, x.shape[1]).index_add_(0, gid, w)
        y = torch.zeros(G, x.shape[1]).index_add_(0, gid, f * w) / den
        return agg.h(y)[gid]

    prev = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        with torch.no_grad():
            t = time.perf_counter()
            x = upd.norm(net + ctx + upd.corr(corr))
            # neighbour rows (net[:, ix], net.py:82-85): a fixed permutation of the sample
            x = x + upd.c1(x[torch.roll(torch.arange(rows), 1)])
            x = x + upd.c2(x[torch.roll(torch.arange(rows), -1)])
            x = x + softagg(upd.agg_kk, x, kk)
            x = x + softagg(upd.agg_ij, x, ii * 12345 + jj)
            x = upd.gru(x)
            upd.d(x), upd.w(x)
            return time.perf_counter() - t
    finally:
        torch.set_num_threads(prev)


def cpu_baseline(slam, sample_edges, iterations):
    """A whole keyframe of the hot path on this host's CPU, timed phase by
    phase on bounded samples and scaled to the full workload:
      * altcorr: the C oracle (a restatement of correlation_kernel.cu) on a
        sample of edges, with T = min(16, cpu_count) OpenMP threads (the box's
        CPU share per GPU) and with 1 thread;
      * update operator: the module's own layers in fp32 torch-CPU (T threads),
        on a sample of edge rows;
      * fastba (the C oracle, 1 thread) and the point cloud (1 thread) on the
        full patch graph.
    Per-phase seconds and threads are reported; cores = the largest thread
    count any phase used."""
    from oracle import oracle
    E = slam.pg.ii.numel()
    threads = max(1, min(16, os.cpu_count() or 1))

    def corr_seconds(n_edges, nthreads):
        idx = torch.linspace(0, E - 1, n_edges).long().to(slam.device)
        coords = slam.reproject()[:, idx].cpu().numpy()
        ii1 = (slam.pg.kk[idx] % (slam.M * slam.pmem)).cpu().numpy()
        jj1 = (slam.pg.jj[idx] % slam.pmem).cpu().numpy()
        oracle.set_threads(nthreads)
        t = time.perf_counter()
        oracle.corr_pyramid(gmap, [f1, f2], coords, ii1, jj1)
        return (time.perf_counter() - t) * E / n_edges

    gmap = slam.gmap.cpu().numpy()
    f1 = slam.fmap1_.contiguous().cpu().numpy()
    f2 = slam.fmap2_.contiguous().cpu().numpy()
    t_corr1 = corr_seconds(sample_edges, 1)
    sample_t = min(E, sample_edges * threads)
    t_corr = corr_seconds(sample_t, threads)
    oracle.set_threads(1)
    rows = min(E, 8192)
    t_net = _update_op_cpu_seconds(slam, rows, threads) * E / rows
    t_net1 = _update_op_cpu_seconds(slam, min(E, 2048), 1) * E / min(E, 2048)
    n = slam.n
    target = (slam.reproject()[..., 1, 1] + torch.randn(1, E, 2, device=slam.device)).cpu().numpy()
    weight = torch.rand(1, E, 2).numpy()
    poses = slam.pg.poses_[:slam.N].cpu().numpy()
    patches = slam.pg.patches_.view(-1, 3, P, P).cpu().numpy()
    intr = slam.pg.intrinsics_.cpu().numpy()
    ii, jj, kk = (x.cpu().numpy() for x in (slam.pg.ii, slam.pg.jj, slam.pg.kk))
    t = time.perf_counter()
    oracle.ba_forward(poses, patches, intr, target, weight, 1e-4, ii, jj, kk, max(n - 10, 1), n, iterations)
    t_ba = time.perf_counter() - t
    m = slam.pg.m
    t = time.perf_counter()
    oracle.point_cloud_centre(poses, patches[:m], intr, slam.ix[:m].cpu().numpy())
    t_pc = time.perf_counter() - t
    total = t_corr + t_net + t_ba + t_pc
    total1 = t_corr1 + t_net1 + t_ba + t_pc
    r = lambda x: round(x, 4)
    return {"value": round(1.0 / total, 6), "unit": "keyframes/s", "cores": threads, "kind": "port",
            "cpu_model": _cpu_model(), "whole_keyframe": True,
            "phases": {"altcorr": {"seconds": r(t_corr), "threads": threads,
                                   "sample": f"C oracle on {sample_t} of {E} edges, scaled x{E / sample_t:.1f}"},
                       "update_op": {"seconds": r(t_net), "threads": threads,
                                     "sample": f"torch-CPU fp32 module layers on {rows} of {E} rows, scaled"},
                       "fastba": {"seconds": r(t_ba), "threads": 1, "sample": f"C oracle, full graph, {iterations} it"},
                       "point_cloud": {"seconds": r(t_pc), "threads": 1, "sample": f"C oracle, {m} patches"}},
            "sample": f"altcorr and update operator on edge samples with {threads} threads (scaled to E={E}); "
                      f"fastba ({iterations} it) and point cloud single-threaded on the full graph",
            "seconds_per_keyframe": round(total, 3),
            "single_thread": {"value": round(1.0 / total1, 6), "cores": 1, "seconds_per_keyframe": round(total1, 3),
                              "sample": f"altcorr on {sample_edges} edges, update operator on 2048 rows, 1 thread"}}


def end_to_end(cfgd, buffer, iterations, frames, warmup=8, device="cuda", defer=True, mark_gap=0.0):
    """North-star end-to-end frames/s: DPVO.__call__ per synthetic 512x384
    frame (ingest CNNs + patchify + edges + update + keyframe) from the
    injected steady state.  Random weights give the motion magnitude no
    natural scale, so keyframe()'s decision alternates keep / drop frame by
    frame (KEYFRAME_THRESH set to -1 / +inf before each call; the motion
    magnitude is still computed and read): both paths are timed in equal
    shares, and the counts are reported.  defer: cfg.DEFER_KEYFRAME (each
    decision applied by the next __call__, after its encoders are enqueued;
    the last one inside the timed region, by flush_keyframe())."""
    from dpvo.synthetic import image_stream, steady_state_tracker
    total = frames + warmup
    slam = steady_state_tracker(cfgd["preset"], buffer=buffer, n=buffer - 8 - total, seed=0, iterations=iterations,
                                device=device, DEFER_KEYFRAME=defer, **cfgd["overrides"])
    intr = torch.tensor([320.0, 320.0, 320.0, 240.0], device=slam.device)
    imgs = [img for _, img in image_stream(total, device=slam.device)]
    calls = [0]
    inner = slam.keyframe

    def keyframe():
        slam.cfg.KEYFRAME_THRESH = float("inf") if calls[0] % 2 == 0 else -1.0
        calls[0] += 1
        inner()
    slam.keyframe = keyframe
    t_first = slam.n
    with torch.no_grad():
        for k, img in enumerate(imgs):
            if k == warmup:
                slam.flush_keyframe()
                calls[0], drops0 = 0, getattr(slam, "keyframes_dropped", 0)
                torch.cuda.synchronize()
                if mark_gap:   # an idle gap that marks the timed frames in a kernel trace
                    time.sleep(mark_gap)
                t0 = time.perf_counter()
            slam(t_first + k, img, None, None, intr)
        slam.flush_keyframe()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    dropped = getattr(slam, "keyframes_dropped", 0) - drops0
    return {"metric": "end-to-end frames/s (DPVO.__call__: ingest CNNs + patchify + update + keyframe)",
            "value": round(frames / dt, 2), "unit": "frames/s", "ms_per_frame": round(dt / frames * 1e3, 3),
            "frames": frames, "warmup": warmup, "keyframes_kept": calls[0] - dropped, "keyframes_dropped": dropped,
            "keyframe_policy": "alternating keep / drop", "deferred_keyframe": bool(defer)}


def main():
    args = parse()
    world, rank, local = dist_setup(args)
    assert world == args.gpus or world == 1, "launch N>1 with torch.distributed.run"
    from dpvo.synthetic import steady_state_tracker

    cfgd = CONFIGS[args.config]
    args.buffer = args.buffer or cfgd["buffer"]
    args.iterations = args.iterations or cfgd["iterations"]
    slam = steady_state_tracker(cfgd["preset"], buffer=args.buffer, seed=rank, iterations=args.iterations,
                                device=f"cuda:{local}", EXACT_CORR=args.exact_corr, **cfgd["overrides"])
    E = slam.pg.ii.numel()
    probe = CorrProbe()
    if args.full:
        probe.wrap(slam)

    # update() makes no host read (BA's status is checked after the loop,
    # slam.check_ba).  --graph captures it once into a HIP graph during the
    # warmup and replays it (the patch graph does not change between steps);
    # within box spread of eager on one GPU (profiles/r4/bench_c3_graph_r4.json),
    # so eager is the default and (--full) the corr events below time every launch live
    host = None
    if args.full or world > 1:
        with torch.no_grad():
            host = host_cost(slam, args.cores)
    # each rank launches from its own pinned cores: replay update() from a HIP
    # graph (one launch per step) when a rank's launching thread is busy for
    # more than half of its step -- host jitter could then starve its GPU
    graph = args.graph or (world > 1 and host["launch_thread_share"] > 0.5)
    upd = slam.update_graphed if graph else slam.update
    with torch.no_grad():
        for _ in range(max(args.warmup, 2 if graph else 0)):
            upd()
        probe.clear()
        barrier(world)
        torch.cuda.synchronize()
        c0, p0 = time.thread_time(), time.process_time()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            upd()
        torch.cuda.synchronize()
        barrier(world)
        elapsed = time.perf_counter() - t0
        c1, p1 = time.thread_time(), time.process_time()
        slam.check_ba()
        # the state as the last timed step left it, before anything below runs more updates
        if args.dump_outputs and rank == 0:
            write_arrays(args.dump_outputs, dump_arrays(slam))
        if args.full:
            # every timed launch (eager); with --graph the captured launches are
            # not evented (ROCm torch has no event-record nodes), so the probe
            # falls back to a short eager pass after the loop
            corr_ms, order_ms = probe.mean_ms("corr"), probe.mean_ms("order")
            if graph:
                for _ in range(3):
                    slam.update()
                torch.cuda.synchronize()
                corr_ms, order_ms = probe.mean_ms("corr"), probe.mean_ms("order")
                slam.check_ba()
            breakdown = phase_breakdown(slam)
            if not slam.cfg.EXACT_CORR:
                breakdown["ingest_gmap_pack"] = gmap_pack_ms(slam)

    gather_ms = None
    if world > 1:
        elapsed = max_over_ranks(elapsed, slam.device)
        # result gather (C5): poses and point cloud of every sequence to rank 0, over RCCL
        torch.cuda.synchronize()
        tg = time.perf_counter()
        gather_to_rank0([slam.pg.points_[:slam.pg.m], slam.pg.poses_[:slam.n]], rank, world)
        torch.cuda.synchronize()
        gather_ms = round((time.perf_counter() - tg) * 1e3, 3)

    if rank == 0:
        value = world * args.steps / elapsed
        metric = METRIC if args.buffer == 2048 else METRIC.replace("2048-KF buffer", f"{args.buffer}-KF buffer")
        line = {
            "metric": metric, "value": round(value, 3), "unit": "keyframes/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f16+f32",
            "launch": "hip-graph replay of update()" if graph else "eager",
            "data": "synthetic (seeded steady-state patch graph, random-init VONet weights)",
            "config": {"workload": f"{cfgd['name']}: M={slam.M}, {args.buffer}-KF buffer, n={slam.n} keyframes, "
                                   f"E={E} edges, 512x384, {slam.cfg.BA_ITERATIONS} BA iterations",
                       "patches_per_frame": slam.M, "buffer": args.buffer, "n_keyframes": slam.n, "edges": E,
                       "ba_iterations": slam.cfg.BA_ITERATIONS, "image": "512x384",
                       "parallelism": f"replicas{world}"},
            "host_cores": {"rank0": _core_str(args.cores), "cpu_model": _cpu_model()},
            "host_ms_per_step": round((c1 - c0) / args.steps * 1e3, 4),
            "host_process_ms_per_step": round((p1 - p0) / args.steps * 1e3, 4),
        }
        if host is not None:
            line["host_calibration"] = host
        if args.dump_outputs:
            line["outputs"] = args.dump_outputs
        if args.full:
            counters = load_counters(args.counters_json, E)
            roof, roof_upd = roofline_lines(slam, corr_ms, order_ms, breakdown, counters, args.counters_json)
            line.update({
                "roofline": roof,
                "roofline_update_op": roof_upd,
                "breakdown_ms": breakdown,
                "fastba_us_per_iteration": round(breakdown["fastba"] * 1e3 / slam.cfg.BA_ITERATIONS, 2),
            })
        if gather_ms is not None:
            line["gather_ms"] = gather_ms
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(slam, args.cpu_sample_edges, slam.cfg.BA_ITERATIONS)
        if args.full and world == 1 and args.e2e_frames > 0:
            del slam
            torch.cuda.empty_cache()
            e2e = end_to_end(cfgd, args.buffer, args.iterations, args.e2e_frames, device=f"cuda:{local}")
            torch.cuda.empty_cache()
            imm = end_to_end(cfgd, args.buffer, args.iterations, args.e2e_frames, device=f"cuda:{local}", defer=False)
            e2e["immediate_keyframe"] = {"value": imm["value"], "ms_per_frame": imm["ms_per_frame"]}
            line["end_to_end"] = e2e
        print(json.dumps(line), flush=True)

    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
