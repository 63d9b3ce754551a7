#!/usr/bin/env python3
"""Headline benchmark: Graphalytics PageRank edges/s on MI355X.

Workload (the north-star target "datagen-8_5-fb PageRank at 1 GPU"):
PageRank, d = 0.85, 10 iterations, fp64, on SYN-8_5 -- the seeded stand-in for datagen-8_5-fb
(no network for the real dataset): undirected R-MAT (a,b,c,d) = (0.57,0.19,0.19,0.05), scale 23,
edgefactor 40, seed 85, duplicates and self-loops removed, vertex ids randomly permuted
(8.4 M vertices, 628 M stored entries).  One "step" = one complete PageRank run (init + 10 pull
iterations) with the graph resident in HBM.  A plain run sets up, warms up, times the K steps
and prints the line; --full adds every leg that takes runs of its own (roofline.traffic and
stream_copy_gbs, processing_ms, cpu_baseline, the parity fields and, at N = 1, `secondary`: the
same measurement on SYN-7_5, configs[1]'s datagen-7_5-fb stand-in, scale 20, ef 32, seed 75);
their fields are null without it.  --dump-outputs DIR writes what the last timed step returned
as DIR/<name>.npy (dump_outputs); the inputs are seeded, so two builds can be compared.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--graph SYN-7_5] [--full] [--dump-outputs DIR]

N > 1 is launched by torch.distributed.run (one rank per GPU, RCCL): the pull matrix is
row-partitioned and the rank vector is all-gathered every iteration (strong scaling on the
same graph).  Rank 0 prints ONE JSON line.

value    = (stored entries * iterations * K) / max-over-ranks wall time of the K steps
roofline = k_pr_pull_units: algorithmic bytes per launch (4 nnz + 8 (n+1) + 8 n + 8 n, SURVEY.md
           8d) / mean launch duration from hipEvents on the launch stream during the timed
           steps; peak 8.0 TB/s (MI355X HBM3E); traffic from the committed rocprofv3 PMC pass.
processing_ms = the Graphalytics processing time of the executable path (bin/exe/pr brackets
           gx_graph_create's upload + one gx_pagerank call, whose first call builds the plan:
           pr.cpp:77-79 brackets LAGraph_New .. LAGr_PageRankGX the same way).
cpu_baseline = the oracle's OpenMP PageRank (oracle/gx_oracle.c, "port" -- SuiteSparse is not
           installed) on every host core this process may use (the cgroup CPU quota, e.g. 16 on
           the GPU box), on the same graph, rank 0 at N = 1 only.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec (MI355X_MICROARCH.md, chip-level parameters)
METRIC = "edges/sec (GTEPS) per algorithm at 1/2/4/8 GPUs; % HBM roofline"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # ~9.5 s of PageRank on SYN-8_5: a timed region the driver's GPU-busy sampling can see (300
    # steps, 1.9 s, was seen 0 % busy in all 10 samples of a 47 s run)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--damping", type=float, default=0.85)
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="budget of the CPU baseline leg")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="PR: skip the SYN-7_5 secondary measurement")
    ap.add_argument("--algorithm", default="pr", choices=["pr", "bfs", "wcc", "sssp", "cdlp", "lcc"],
                    help="pr = the headline (SYN-8_5, BASELINE configs[3]'s graph); the others measure configs 3-5 "
                         "on 1 GPU")
    ap.add_argument("--graph", default=None, choices=sorted(PRESETS), help="synthetic stand-in (SURVEY.md 8d)")
    ap.add_argument("--pmc-traffic", choices=["run", "committed"], default="run",
                    help="PR roofline.traffic: measured in this run by two rocprofv3 --pmc child passes "
                         "(FETCH_SIZE, WRITE_SIZE) of a one-step bench, or read from profiles/pmc_pr_pull.json")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--partitioned", action="store_true",
                    help="run --algorithm through the multi-GPU (vertex-range) path even at N=1")
    ap.add_argument("--full", action="store_true",
                    help="PR: beside the headline, everything that takes runs of its own -- the rocprofv3 traffic "
                         "passes, the stream-copy bandwidth, the executables' processing time, the CPU baseline, "
                         "parity against the oracle and the SYN-7_5 secondary (their fields are null without it); "
                         "an --algorithm line is complete either way")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned as DIR/<name>.npy (float64; a "
                         "fixed seeded sample of an output larger than the cap, see dump_outputs)")
    return ap.parse_args()


DUMP_CAP_BYTES = 32 << 20   # all files of one --dump-outputs together
DUMP_SEED = 0


def dump_outputs(dirpath: str, arrays: dict) -> None:
    """--dump-outputs: each array the timed path returned in its last step, as DIR/<name>.npy in
    float64 (integer labels and levels are exact below 2^53; BFS's unreached marker rounds to
    2^63).  An array over its share of DUMP_CAP_BYTES is cut to a sample at sorted positions drawn
    by default_rng(DUMP_SEED) from its size alone, so two runs with the same arguments write the
    same positions."""
    os.makedirs(dirpath, exist_ok=True)
    share = DUMP_CAP_BYTES // max(1, len(arrays))
    for name, a in arrays.items():
        a = np.ascontiguousarray(a).ravel()
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        if a.nbytes > share:
            a = a[np.sort(np.random.default_rng(DUMP_SEED).choice(a.size, share // a.itemsize, replace=False))]
        np.save(os.path.join(dirpath, f"{name}.npy"), a)


# SURVEY.md 8d synthetic stand-ins (no network for the Graphalytics datasets)
PRESETS = {
    "SYN-7_5": dict(scale=20, ef=32, seed=75, undirected=True, weighted=False, stands_for="datagen-7_5-fb"),
    "SYN-g500-22": dict(scale=22, ef=16, seed=22, undirected=True, weighted=False, stands_for="graph500-22"),
    "SYN-8_5": dict(scale=23, ef=40, seed=85, undirected=True, weighted=True, stands_for="datagen-8_5-fb"),
    "SYN-cit": dict(scale=22, ef=4, seed=3, undirected=False, weighted=False, stands_for="cit-Patents"),
}
DEFAULT_GRAPH = {"pr": "SYN-8_5", "cdlp": "SYN-7_5", "bfs": "SYN-g500-22", "wcc": "SYN-g500-22",
                 "sssp": "SYN-8_5", "lcc": "SYN-cit"}
# the dominant kernel of each algorithm: the KTimer names summed (CDLP's light tier runs as
# two launches, the 256-slot instance "cdlp_light_s" and the 1024-slot "cdlp_light")
DOMINANT = {"bfs": ["bfs_expand"], "wcc": ["wcc_hook"], "sssp": ["sssp_relax"],
            "cdlp": ["cdlp_light", "cdlp_light_s"], "lcc": ["lcc_triangles"]}
# BFS: a level's frontier phase (bitmap / queue rebuild) and expansion (bottom-up / top-down);
# GX_BFS_FUSED=0 brackets them as "bfs_bottomup" (bitmap + bottom-up) and "bfs_topdown"
KERNELS = {"bfs": ["bfs_frontier", "bfs_expand", "bfs_topdown", "bfs_bottomup"],
           "wcc": ["wcc_sample", "wcc_hook", "wcc_compress"],
           "sssp": ["sssp_relax", "sssp_advance"],
           "cdlp": ["cdlp_tiny", "cdlp_small", "cdlp_light_s", "cdlp_light", "cdlp_mid2", "cdlp_mid4", "cdlp_mid",
                    "cdlp_heavy", "cdlp_first", "cdlp_mark", "cdlp_keep", "cdlp_sparse"],
           "lcc": ["lcc_orient", "lcc_triangles", "lcc_core"]}


def usable_cores() -> int:
    """Host cores this process may use: the CPU affinity mask, capped by the cgroup CPU quota
    (cgroup v2 cpu.max; the GPU box grants 16 of its 256 CPUs this way, and `nproc` reports
    the same 16 there through OMP_NUM_THREADS)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def host_cpu() -> dict:
    """Core counts and the CPU model name, recorded with every CPU baseline."""
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    import shutil
    import subprocess
    nproc = None
    if shutil.which("nproc"):
        try:
            nproc = int(subprocess.run(["nproc"], capture_output=True, text=True).stdout.strip())
        except ValueError:
            pass
    return {"nproc": nproc, "cpu_count": os.cpu_count(), "usable_cores": usable_cores(), "cpu_model": model}


def stream_copy_gbs(device, nbytes: int = 1 << 30, reps: int = 10) -> float:
    """Measured device-to-device copy bandwidth (read + write bytes / time), the STREAM-copy
    denominator SURVEY.md 8d asks for beside the 8 TB/s spec."""
    import torch
    a = torch.empty(nbytes // 8, dtype=torch.float64, device=device).fill_(1.0)
    b = torch.empty_like(a)
    b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        b.copy_(a)
    e1.record()
    e1.synchronize()
    gbs = 2.0 * nbytes * reps / (e0.elapsed_time(e1) / 1e3) / 1e9
    del a, b
    torch.cuda.empty_cache()
    return gbs


def run_algorithm(args):
    """One GPU, one algorithm on its BASELINE config (3-5); prints one JSON line.
    value = work units / device time of a warm call (graph resident in HBM; the transpose /
    closure built by the first call is cached and reported separately as first_call_ms)."""
    import torch  # noqa: F401  (device init like the PR path)
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat
    alg = args.algorithm
    gname = args.graph or DEFAULT_GRAPH[alg]
    P = PRESETS[gname]
    t_gen = time.time()
    csr = rmat(P["scale"], P["ef"], P["seed"], undirected=P["undirected"], weighted=(alg == "sssp"))
    t_gen = time.time() - t_gen
    directed = not P["undirected"]
    n, nnz = csr.n, csr.nnz
    deg = np.diff(csr.rowptr.astype(np.int64))
    src = int(np.argmax(deg))
    ctx = A.Context(0)
    dev_name, cus = ctx.info()
    t_up = time.perf_counter()
    G = A.Graph(ctx, csr, directed)   # H2D upload (inside Graphalytics processing time)
    t_up = time.perf_counter() - t_up
    iters = args.iters

    def call():
        if alg == "bfs":
            return A.LA_BFS(G, src)
        if alg == "wcc":
            return A.WeaklyConnectedComponents(G)
        if alg == "sssp":
            return A.LA_SSSP(G, src)
        if alg == "cdlp":
            return A.LA_CDLP(G, iters)
        return A.LA_LCC(G)

    t1 = time.perf_counter()
    out = call()
    first_ms = (time.perf_counter() - t1) * 1e3
    for _ in range(max(0, args.warmup - 1)):
        call()
    # timed steps without per-kernel events (they add a gap around every launch)
    dev_ms = []
    t1 = time.perf_counter()
    for _ in range(args.steps):
        out = call()
        dev_ms.append(ctx.last_device_ms())
    wall = time.perf_counter() - t1
    # per-kernel breakdown from a separate instrumented pass
    stat_runs = max(1, min(args.steps, 3))
    ctx.reset_kernel_stats()
    ctx.set_kernel_timing(True)
    for _ in range(stat_runs):
        call()
    ctx.set_kernel_timing(False)
    kl, kms = 0, 0.0
    for name in DOMINANT[alg]:
        l_, ms_ = ctx.kernel_stats(name)
        kl, kms = kl + l_, kms + ms_
    kms = kms * args.steps / stat_runs   # scaled to the timed steps (dominant_kernel_ms_per_run divides)
    per_kernel = {k: dict(zip(("launches", "ms_per_run"), (lambda t: (t[0], t[1] / stat_runs))(
        ctx.kernel_stats(k)))) for k in KERNELS[alg]}
    t_dev = float(np.median(dev_ms)) / 1e3
    # work units and algorithmic bytes (SURVEY.md 8d / BASELINE.md)
    nnz_eff = nnz * (2 if (alg == "cdlp" and directed) else 1)
    if alg == "bfs":
        reached = out != np.iinfo(np.int64).max
        work = int(deg[reached].sum()) // (1 if directed else 2)   # Graph500 TEPS: input edges reached
        nbytes = 4 * nnz + 16 * n + 8
        unit = "TEPS"
    elif alg == "wcc":
        work, nbytes, unit = nnz, 4 * nnz + 16 * n + 8, "edges/s"
    elif alg == "sssp":
        work, nbytes, unit = nnz, 12 * nnz + 16 * n + 8, "edges/s"
    elif alg == "cdlp":
        work = nnz_eff * iters
        nbytes = (4 * nnz_eff + 8 * (n + 1) * (2 if directed else 1) + 16 * n) * iters
        unit = "edges/s"
    else:
        from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
        rows = np.repeat(np.arange(n, dtype=np.int64), deg)
        cl = csr_from_edges(n, rows, csr.colidx.astype(np.int64), None, symmetric=True)
        sdeg = np.diff(cl.rowptr.astype(np.int64))
        work = cl.nnz
        # bytes of the algorithm that runs (gx_lcc.hip): orientation reads every closure entry
        # (5 B) and the degree of its column (16 B) and writes the kept ones packed (4 B); the
        # transpose writes, radix-sorts (3 passes of 8-B keys) and unpacks the m oriented
        # entries (~68 B each); the triangle pass probes every entry of O(v) for each oriented
        # edge (v, u) (4 B each, sum of |O(v)|^2) and builds a table from O(u) per work item.
        srows = np.repeat(np.arange(n, dtype=np.int64), sdeg)
        scols = cl.colidx.astype(np.int64)
        keep = (sdeg[scols] > sdeg[srows]) | ((sdeg[scols] == sdeg[srows]) & (scols > srows))
        odeg = np.bincount(srows[keep], minlength=n).astype(np.int64)
        m_or = int(keep.sum())
        probes = int((odeg.astype(np.float64) ** 2).sum())
        nbytes = 25 * cl.nnz + 68 * m_or + 4 * probes + 8 * (n + 1)
        ref_model_bytes = 4 * int((sdeg.astype(np.float64) ** 2).sum()) + 4 * cl.nnz + 8 * (n + 1)
        unit = "edges/s"
    if alg != "lcc":
        ref_model_bytes = None
    split = None
    if alg == "sssp":
        # config 4's multi-GPU SSSP path (1-D split, gx_sssp_split) at N = 1: the same rounds,
        # no exchange -- its device time against gx_sssp's
        sp = A.SsspSplit(G)
        try:
            sp.run(src)
            sms = []
            for _ in range(max(1, min(args.steps, 5))):
                d_split = sp.run(src)
                sms.append(ctx.last_device_ms())
            split = {"path": "gx_sssp_split_run (1 rank owning every vertex)", "ms": float(np.median(sms)),
                     "ratio_vs_gx_sssp": float(np.median(sms)) / (t_dev * 1e3),
                     "equal_to_gx_sssp": bool(np.array_equal(d_split, out))}
        finally:
            sp.close()
    # Graphalytics processing time: upload + the first call (transpose /
    # closure / layout built inside it), as the executables' markers bracket it
    proc_ms = t_up * 1e3 + first_ms
    import torch
    copy_gbs = stream_copy_gbs(torch.device("cuda", 0))
    cpu = None
    parity = None
    if not args.no_cpu_baseline:
        from oracle import oracle as O
        threads = usable_cores()
        # the multithreaded baselines (direction-optimising BFS, lock-free union-find WCC,
        # delta-stepping SSSP; CDLP and LCC are OpenMP over vertices) on every usable core
        t1 = time.perf_counter()
        if alg == "bfs":
            base = O.bfs_par(csr, src, not directed, nthreads=threads)
        elif alg == "wcc":
            base = O.wcc_par(csr, nthreads=threads)
        elif alg == "sssp":
            base = O.sssp_par(csr, src, 0.0, nthreads=threads)
        elif alg == "cdlp":
            base = O.cdlp(csr, directed, iters, nthreads=threads)
        else:
            base = O.lcc(csr, directed, nthreads=threads)
        t_cpu = time.perf_counter() - t1
        cpu = {"value": work / t_cpu, "unit": unit, "cores": threads, "kind": "port",
               "sample": f"one full {alg} run on the same {gname} graph (oracle/gx_oracle.c, {threads} threads), "
                         f"{t_cpu:.2f} s", **host_cpu()}
        # parity against the serial checker (the *_par baselines equal it bitwise, tests)
        ref = {"bfs": lambda: O.bfs(csr, src), "wcc": lambda: O.wcc(csr), "sssp": lambda: O.sssp(csr, src)}.get(
            alg, lambda: base)()
        parity = "bit-exact" if np.array_equal(out, ref) else f"MISMATCH ({int((out != ref).sum())} vertices)"
    traffic, traffic_src = pmc_alg_traffic(alg, f"{alg.upper()} {gname}")
    rocprof_kernels = pmc_alg_kernels(alg, f"{alg.upper()} {gname}")
    # the dominant kernel as measured now (largest per-run time of the instrumented pass), not a
    # fixed name; and whether the committed PMC figure still describes these
    # kernels: its profiled per-run kernel time against this run's device time
    measured_dom = max(per_kernel.items(), key=lambda kv: kv[1]["ms_per_run"])[0] if per_kernel else None
    traffic_note = None
    if rocprof_kernels:
        prof_ms = sum(v for k, v in rocprof_kernels.items() if k != "source") / 1e3
        rel = abs(prof_ms - t_dev * 1e3) / max(t_dev * 1e3, 1e-9)
        traffic_note = (f"{traffic_src}: its profiled kernels took {prof_ms:.3f} ms per run, this run's device time "
                        f"{t_dev * 1e3:.3f} ms" + (" -- from an older tree than these kernels (differs by "
                                                    f"{rel:.0%})" if rel > 0.15 else " (same kernels within 15 %)"))
    line = {
        "metric": METRIC, "value": work / t_dev, "unit": unit, "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": t_dev * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": {"sssp": "f64", "lcc": "int64+f64"}.get(alg, "int32"),
        "data": f"synthetic (seeded R-MAT stand-in for {P['stands_for']}; no network for the real dataset)",
        "config": {"workload": f"{alg.upper()} {gname}", "algorithm": alg, "graph": gname, "n": n, "nnz": nnz,
                   "directed": directed, "iterations": iters if alg == "cdlp" else None, "source": src,
                   "parallelism": "single", "device": dev_name, "cus": cus},
        "roofline": {"kernel": f"{alg} (whole device time)", "dominant_kernel": measured_dom,
                     "dominant_kernel_fixed": " + ".join(DOMINANT[alg]), "bound": "hbm",
                     "achieved": nbytes / t_dev / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": nbytes / t_dev / 1e9 / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                     "traffic_note": traffic_note,
                     "bytes_per_run": nbytes,
                     "dominant_kernel_ms_per_run": per_kernel[measured_dom]["ms_per_run"] if measured_dom else None,
                     "dominant_launches": per_kernel[measured_dom]["launches"] if measured_dom else None,
                     "dominant_fixed_ms_per_run": kms / max(1, args.steps), "dominant_fixed_launches": kl,
                     # event brackets of an instrumented pass (they include launch gaps and host waits);
                     # the committed rocprofv3 durations of the same workload are the attribution to trust
                     "kernels": per_kernel, "kernels_source": "KTimer event brackets, instrumented pass",
                     "kernels_rocprof_us_per_run": rocprof_kernels,
                     "survey_8d_bytes_per_run": ref_model_bytes,
                     "stream_copy_gbs": copy_gbs, "frac_of_stream": nbytes / t_dev / 1e9 / copy_gbs},
        "processing_ms": proc_ms,
        "evps": (n + (nnz if directed else nnz // 2)) / (proc_ms / 1e3),
        "cpu_baseline": cpu, "parity_vs_oracle": parity, "first_call_ms": first_ms, "split_n1": split,
        "wall_ms_per_call_incl_d2h": wall * 1e3 / args.steps, "graph_gen_s": t_gen,
    }
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {alg: out})
    print(json.dumps(line), flush=True)
    G.close()
    ctx.close()


def _pmc_alg_entry(alg: str, workload: str):
    """The newest committed rocprofv3 PMC summary (tools/alg_pmc.sh + tools/alg_pmc_json.py:
    profiles/rNN_pmc_*.json with an "algorithms" table) that covers this workload: (entry, file)."""
    for p in sorted((ROOT / "profiles").glob("r*_pmc_*.json"), reverse=True):
        try:
            a = json.loads(p.read_text()).get("algorithms", {}).get(alg)
        except Exception:
            continue
        if a and a.get("workload") == workload:
            return a, p.name
    return None, None


def pmc_alg_traffic(alg: str, workload: str):
    """Per-run HBM bytes of an algorithm's per-run kernels from the newest PMC summary covering
    the workload, if any."""
    a, name = _pmc_alg_entry(alg, workload)
    return (a.get("hbm_bytes_per_run"), name) if a else (None, None)


def pmc_alg_kernels(alg: str, workload: str):
    """rocprofv3 kernel durations (us per run) of an algorithm's per-run kernels from the newest
    PMC summary (the event brackets cover more than the kernels)."""
    a, name = _pmc_alg_entry(alg, workload)
    if not a:
        return None
    return {"source": name, **{k: round(v.get("us_per_run", 0.0), 2) for k, v in a.get("per_run_kernels", {}).items()}}


def measure_pr_traffic(gname: str, timeout_s: int = 180):
    """HBM bytes per k_pr_pull_units launch measured now: two child runs of a
    one-step bench on the same graph under rocprofv3, one counter set each (MI355X_MICROARCH.md:
    separate --pmc passes, FETCH_SIZE doubled on gfx950, WRITE_SIZE as is; KB per dispatch, the
    mean over the pass's dispatches).  A child is a new process started by this one (never an
    exec), in its own session, killed with its group at the time limit.  Returns (bytes or
    None, note)."""
    import csv
    import glob
    import shutil
    import signal
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    kb = {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="gx_pmc_", dir="/tmp")
        cmd = [exe, "--pmc", ctr, "--kernel-include-regex", "k_pr_pull_units", "--output-format", "csv", "-d", d,
               "-o", "pmc", "--", sys.executable, str(ROOT / "bench.py"), "--graph", gname, "--steps", "1",
               "--warmup", "0", "--no-cpu-baseline", "--no-secondary", "--pmc-child"]
        env = dict(os.environ, TMPDIR="/tmp")
        try:
            p = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, env=env, cwd=str(ROOT),
                                 start_new_session=True)
            try:
                rc = p.wait(timeout=timeout_s)
            except subprocess.TimeoutExpired:
                os.killpg(p.pid, signal.SIGKILL)
                p.wait()
                return None, f"the {ctr} pass exceeded {timeout_s} s"
            if rc != 0:
                return None, f"the {ctr} pass failed (exit {rc})"
            v = [float(r["Counter_Value"]) for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
                 for r in csv.DictReader(open(f)) if r.get("Counter_Name") == ctr]
            if not v:
                return None, f"the {ctr} pass recorded no dispatch"
            kb[ctr] = (sum(v) / len(v), len(v))
        finally:
            shutil.rmtree(d, ignore_errors=True)
    fetch, write = kb["FETCH_SIZE"][0], kb["WRITE_SIZE"][0]
    return (2 * fetch + write) * 1024, (f"measured in this run: rocprofv3 --pmc FETCH_SIZE ({kb['FETCH_SIZE'][1]} "
                                        f"dispatches, x2 for gfx950) and WRITE_SIZE ({kb['WRITE_SIZE'][1]}) child passes "
                                        f"of a one-step bench on {gname}")


def pmc_traffic(workload: str):
    """Per-launch HBM bytes of k_pr_pull from the committed rocprofv3 PMC pass, if present."""
    p = ROOT / "profiles" / "pmc_pr_pull.json"
    if not p.exists():
        return None
    try:
        d = json.loads(p.read_text())
        for e in d.get("entries", [d]):
            if e.get("workload") == workload:
                return e.get("hbm_bytes_per_launch")
    except Exception:
        return None
    return None


def run_algorithm_distributed(args):
    """--algorithm X on N GPUs (one process per GPU, torch.distributed.run): the graph is
    replicated, ranks own vertex ranges and exchange state once per round over RCCL
    (distributed.py).  `value` = work units of the whole job / max-over-ranks
    time per call; scaling is strong (every N runs the same graph)."""
    import torch
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    from ldbc_graphalytics_platforms_graphblas_amd import distributed as D
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and not (world == 1 and args.gpus == 1):
        raise SystemExit("--gpus N > 1 must be launched with torch.distributed.run (one rank per GPU)")
    dist = None
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1 or "MASTER_ADDR" in os.environ:   # under torch.distributed.run: RCCL, even at N=1
        import torch.distributed as dist
        dist.init_process_group("nccl")
    alg = args.algorithm
    gname = args.graph or DEFAULT_GRAPH[alg]
    P = PRESETS[gname]
    csr = rmat(P["scale"], P["ef"], P["seed"], undirected=P["undirected"], weighted=(alg == "sssp"))
    directed = not P["undirected"]
    n, nnz = csr.n, csr.nnz
    deg = np.diff(csr.rowptr.astype(np.int64))
    src = int(np.argmax(deg))
    ctx = A.Context(local_rank)
    dev_name, cus = ctx.info()
    G = A.Graph(ctx, csr, directed)
    # GX_SIM_RANKS=k at N = 1: k ranks on this GPU (LocalComm), for the exchange volumes of a
    # k-GPU run (the times are one GPU's)
    sim = int(os.environ.get("GX_SIM_RANKS", "0")) if world == 1 and not dist else 0
    rng = D.vertex_ranges(csr.rowptr, sim or world)
    if sim:
        ranks = [D.LocalRank(D.GpuBackend(G), int(rng[k]), int(rng[k + 1]), device, k) for k in range(sim)]
    else:
        ranks = [D.LocalRank(D.GpuBackend(G), int(rng[rank]), int(rng[rank + 1]), device, rank)]
    comm = D.TorchComm() if dist else D.LocalComm()

    def call():
        if alg == "bfs":
            return D.bfs(ranks, comm, n, src)
        if alg == "wcc":
            return D.wcc(ranks, comm, n)
        if alg == "sssp":
            return D.sssp(ranks, comm, n, src)
        if alg == "cdlp":
            return D.cdlp(ranks, comm, n, args.iters, rng)
        return D.lcc(ranks, comm, n)

    def barrier():
        torch.cuda.synchronize(device)
        if dist:
            dist.barrier()
        torch.cuda.synchronize(device)

    for _ in range(max(1, args.warmup)):
        out = call()
    barrier()
    D.reset_stats()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = call()
    barrier()
    elapsed = time.perf_counter() - t0
    xstats = {k: v / args.steps for k, v in D.STATS.items()}   # per call
    if dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    res = out.cpu().numpy()
    t_call = elapsed / args.steps
    if alg == "bfs":
        reached = res != np.iinfo(np.int64).max
        work, unit = int(deg[reached].sum()) // (1 if directed else 2), "TEPS"
    elif alg == "cdlp":
        work, unit = nnz * (2 if directed else 1) * args.iters, "edges/s"
    else:
        work, unit = nnz, "edges/s"
    parity = None
    if rank == 0 and not args.no_cpu_baseline:
        from oracle import oracle as O
        threads = usable_cores()
        ref = {"bfs": lambda: O.bfs(csr, src), "wcc": lambda: O.wcc(csr), "sssp": lambda: O.sssp(csr, src),
               "cdlp": lambda: O.cdlp(csr, directed, args.iters, nthreads=threads),
               "lcc": lambda: O.lcc(csr, directed, nthreads=threads)}[alg]()
        got = res.astype(ref.dtype) if alg in ("wcc", "cdlp") else res
        parity = "bit-exact" if np.array_equal(got, ref) else f"MISMATCH ({int((got != ref).sum())} vertices)"
    if rank == 0:
        line = {
            "metric": METRIC, "value": work / t_call, "unit": unit, "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": t_call * 1e3, "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": {"sssp": "f64", "lcc": "int64+f64"}.get(alg, "int32"),
            "data": f"synthetic (seeded R-MAT stand-in for {P['stands_for']}; no network for the real dataset)",
            "config": {"workload": f"{alg.upper()} {gname} (partitioned)", "algorithm": alg, "graph": gname,
                       "n": n, "nnz": nnz, "directed": directed, "source": src,
                       "parallelism": (f"replicated graph, {sim} vertex ranges simulated on one GPU" if sim else
                                       f"replicated graph, {world} vertex ranges, RCCL exchange per round"),
                       "device": dev_name, "cus": cus},
            # per call and rank: frontier-sized words vs the dense collectives (distributed._exchange)
            "exchange": {"mode": D.EXCHANGE, **xstats},
            "roofline": None, "cpu_baseline": None, "parity_vs_oracle": parity,
            "note": "wall time per call incl. per-round host syncs; the single-GPU path is bench.py --algorithm X",
        }
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, {alg: res})
        print(json.dumps(line), flush=True)
    G.close()
    ctx.close()
    if dist:
        dist.destroy_process_group()


def pr_workload(gname: str) -> str:
    P = PRESETS[gname]
    return f"PageRank {gname} (R-MAT scale {P['scale']}, ef {P['ef']}, seed {P['seed']}, undirected)"


def measure_pr(csr, args, ctx, device, stream, world, rank, dist, collect=True):
    """K timed PageRank runs of the partitioned path (gx_pr_part_* + gx_pr_dist_*, which is
    gx_pagerank's kernel at N = 1) on this rank's share of `csr`; returns the timings, the
    k_pr_pull_units launch statistics and (rank 0, collect) the scores in csr's vertex order."""
    import torch
    from ldbc_graphalytics_platforms_graphblas_amd.pr_partition import Comm, DevicePageRank, GpuStep, \
        PartitionedPageRank, hub_relabel, interleaved_relabel, partition_rows, slice_rows
    n, nnz = csr.n, csr.nnz
    # GX_PR_PIECES = P > 1: each rank owns P virtual ranks p * N + rank whose all-gathers overlap
    # the next piece's SpMV.  Default 2 at N > 1 (round 6: the scheme bin/exe/pr's
    # gx_pagerank_multi runs, so a scaling line measures the executables' path; only the last
    # piece's exchange is exposed), 1 at N = 1, where there is nothing to hide (a 1/16 piece ran
    # its SpMV at 0.48x the rate of a 1/8 one -- tools/pr_dist_n1.sh).  Layout: the hub-first
    # order (what gx_pagerank does internally) dealt round-robin over the N * pieces virtual
    # ranks, so each owns n / (N * pieces) rows AND ~nnz / (N * pieces) entries and the
    # exchanged vector is ~n long (interleaved_relabel); GX_PR_PARTITION=ranges keeps the
    # round-1 contiguous hub-first ranges balanced by entries.
    # (at N = 1, GX_PR_PIECES = 8 runs the 8 rank shares of config 4 on one GPU back to back:
    # the per-piece launch against 1/8 of the whole-graph launch is the per-rank efficiency)
    pieces = max(1, int(os.environ.get("GX_PR_PIECES", "2" if world > 1 else "1")))
    vranks = world * pieces
    # default: a huge graph (more than 2 Mi entries per CU: config 4's SYN-8_5) is dealt by
    # the single-GPU plan's blocks (block_relabel; 1/8 pieces 139-150 us per SpMV against 208
    # interleaved), a smaller one interleaved
    huge = nnz / max(1, torch.cuda.get_device_properties(device).multi_processor_count) > (2 << 20)
    partition = os.environ.get("GX_PR_PARTITION", "blocks" if huge and vranks > 1 else "interleave")
    if partition == "ranges":
        perm, hub = hub_relabel(csr)
        bounds = partition_rows(hub.rowptr, vranks)
    elif partition == "blocks":
        # GX_PR_PARTITION=blocks: the whole-graph plan's blocks dealt whole (block_relabel); each
        # rank's plan then cuts its rows as the whole graph's (GX_PR_HUGE=1 semantics)
        from ldbc_graphalytics_platforms_graphblas_amd.pr_partition import block_relabel
        perm, hub, bounds = block_relabel(csr, vranks)
        if vranks > 1:
            os.environ.setdefault("GX_PR_HUGE", "1")
    else:
        perm, hub, bounds = interleaved_relabel(csr, vranks)
    lrs = [slice_rows(hub, bounds, p * world + rank) for p in range(pieces)]
    del hub
    t_setup = time.perf_counter()
    steppers = [GpuStep(ctx, n, world * pieces, lr, args.damping) for lr in lrs]   # H2D upload + plans
    torch.cuda.synchronize(device)
    t_setup = time.perf_counter() - t_setup
    # driver "device" (default): libgx enqueues the whole run -- SpMVs and ncclAllGathers on its
    # own RCCL communicator -- and replays it as one hipGraph; "host": one ctypes call and one
    # torch.distributed all-gather per piece and iteration (pr_partition.PartitionedPageRank)
    driver = os.environ.get("GX_PR_DRIVER", "device")
    use_graph = os.environ.get("GX_PR_GRAPH", "1") != "0"
    # GX_PR_EXCHANGE=p2p: the one-shot peer-to-peer exchange (IPC-mapped peer vectors, one
    # write per peer) instead of RCCL's all-gather; off by default (not yet measured on a node
    # with more than one GPU)
    exchange = os.environ.get("GX_PR_EXCHANGE", "rccl")
    comm = dpr = None
    if driver == "device":
        ok = 1
        try:
            if exchange == "p2p":
                def share_all(h: bytes):
                    if not dist:
                        return [h]
                    box = [None] * world
                    dist.all_gather_object(box, h)
                    return box
                dpr = DevicePageRank(steppers, None, use_graph=use_graph, p2p=(world, rank, share_all))
            else:
                if dist:
                    def share_id(uid: bytes) -> bytes:
                        box = [uid]
                        dist.broadcast_object_list(box, src=0)
                        return box[0]
                    comm = Comm(ctx, world, rank, share_id)
                dpr = DevicePageRank(steppers, comm, use_graph=use_graph)
            dpr.run(args.iters, stream.cuda_stream)
            torch.cuda.synchronize(device)
        except Exception as e:   # noqa: BLE001 -- reported, then every rank takes the host driver
            print(f"[bench] device-driven PageRank unavailable ({e}); using the host driver", file=sys.stderr)
            ok = 0
        if dist:   # all ranks agree, so nobody waits in a collective the others skip
            t = torch.tensor([ok], dtype=torch.int32, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            ok = int(t.item())
        if not ok:
            if dpr is not None:
                dpr.close()
            if comm is not None:
                comm.close()
            comm = dpr = None
            driver = "host"
    if driver == "device":
        class _Run:
            def run(self, iters):
                dpr.run(iters, stream.cuda_stream)
        pr = _Run()
    else:
        gather = (lambda out, inp: dist.all_gather_into_tensor(out, inp, async_op=True)) if dist else None
        pr = PartitionedPageRank(steppers, world, [lr.rows for lr in lrs], device, all_gather=gather,
                                 stream_handle=lambda: stream.cuda_stream)
    # hipEvents around every k_pr_pull launch during the timed steps (roofline.achieved).  At
    # N > 1 the timed steps replay the captured graph (events would force direct launches), so
    # the launch durations come from an instrumented pass right after them instead.
    events_in_timed = world == 1 or driver != "device" or not use_graph

    def barrier():
        torch.cuda.synchronize(device)
        if dist:
            dist.barrier()
        torch.cuda.synchronize(device)

    t_first = time.perf_counter()
    pr.run(args.iters)
    torch.cuda.synchronize(device)
    t_first = time.perf_counter() - t_first
    for _ in range(max(0, args.warmup - 1)):
        pr.run(args.iters)
    barrier()
    ctx.reset_kernel_stats()
    ctx.set_kernel_timing(events_in_timed)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pr.run(args.iters)
    barrier()
    elapsed = time.perf_counter() - t0
    if not events_in_timed:
        ctx.set_kernel_timing(True)
        for _ in range(max(1, min(args.steps, 5))):
            pr.run(args.iters)
        barrier()
    ctx.set_kernel_timing(False)
    launches, pull_ms = ctx.kernel_stats("pr_pull")
    if dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    result = None
    if collect:
        # result of the last step (parity check on rank 0), assembled by virtual rank
        if driver == "device":
            mine = list(zip([lr.rank for lr in lrs], dpr.scores([lr.rows for lr in lrs])))
        else:
            mine = [(lr.rank, o[:lr.rows].detach().cpu().numpy()) for lr, o in zip(lrs, pr.rank_outs)]
        if dist:
            parts = [None] * world
            dist.all_gather_object(parts, mine)
            mine = [t for part in parts for t in part]
        result = np.concatenate([a for _, a in sorted(mine, key=lambda t: t[0])])[perm]   # generator's order
    # roofline of k_pr_pull_units on this rank (per launch, averaged over the pieces)
    bytes_per_launch = sum(4 * lr.nnz + 8 * (lr.rows + 1) + 8 * lr.rows + 8 * lr.rows for lr in lrs) / len(lrs)
    mean_launch_s = (pull_ms / launches) / 1e3 if launches else float("nan")
    out = dict(elapsed=elapsed, t_setup=t_setup, t_first=t_first, launches=launches, mean_launch_s=mean_launch_s,
               bytes_per_launch=bytes_per_launch, achieved=bytes_per_launch / mean_launch_s / 1e9,
               driver=driver, use_graph=use_graph, pieces=pieces, vranks=vranks, partition=partition,
               exchange=("p2p" if exchange == "p2p" else "rccl" if comm is not None else "device copies")
               if driver == "device" else "torch.distributed",
               events_in_timed=events_in_timed, exchanged=steppers[0].chunk * vranks / n, result=result)
    if dpr is not None:
        dpr.close()
    if comm is not None:
        comm.close()
    for st in steppers:
        st.close()
    torch.cuda.synchronize(device)
    torch.cuda.empty_cache()
    return out


def exe_path_pr(csr, args, ctx):
    """The Graphalytics processing time of bin/exe/pr (exe/common.cpp): its markers bracket one
    gx_pagerank_csr call -- the H2D upload of the columns overlapped with the plan, which builds
    the hub-first order from the row pointers and takes each column chunk as it lands, then the
    iterations (pr.cpp:77-79 brackets LAGraph_New .. LAGr_PageRankGX, with
    LAGraph_Cached_OutDegree / _AT inside).  Beside it, the two-call path it replaced
    (gx_graph_create, whose upload rate is reported, then the first gx_pagerank, which plans) and
    a warm call of the API."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    t0 = time.perf_counter()
    r, g = A.LA_PR_csr(ctx, csr, False, args.damping, args.iters, keep=True)
    t_fused = time.perf_counter() - t0
    N.lib().gx_graph_free(g)   # after the end marker, as bin/exe/pr does
    t0 = time.perf_counter()
    G = A.Graph(ctx, csr, False)
    t_up = time.perf_counter() - t0
    t0 = time.perf_counter()
    A.LA_PR(G, args.damping, args.iters)
    t_call = time.perf_counter() - t0
    t0 = time.perf_counter()
    A.LA_PR(G, args.damping, args.iters)
    t_warm = time.perf_counter() - t0
    G.close()
    up_bytes = 4 * csr.nnz + 8 * (csr.n + 1)
    return dict(processing_ms=t_fused * 1e3, path="gx_pagerank_csr (upload overlapped with the plan)",
                two_call_processing_ms=(t_up + t_call) * 1e3, upload_ms=t_up * 1e3,
                upload_gbs=up_bytes / t_up / 1e9, first_call_ms=t_call * 1e3, warm_call_ms=t_warm * 1e3), r


def main():
    args = parse()
    import torch

    if args.algorithm != "pr":
        if int(os.environ.get("WORLD_SIZE", "1")) > 1 or args.gpus > 1 or args.partitioned:
            return run_algorithm_distributed(args)
        return run_algorithm(args)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus N > 1 must be launched with torch.distributed.run (one rank per GPU)")
    dist = None
    if world > 1 or "MASTER_ADDR" in os.environ:   # under torch.distributed.run: RCCL, even at N=1
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl")
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)

    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat

    gname = args.graph or DEFAULT_GRAPH["pr"]
    P = PRESETS[gname]
    workload = pr_workload(gname)
    t_gen = time.time()
    csr = rmat(P["scale"], P["ef"], P["seed"], undirected=True)
    t_gen = time.time() - t_gen
    n, nnz = csr.n, csr.nnz

    ctx = Context(local_rank)
    dev_name, cus = ctx.info()
    # a real (non-null) stream: libgx launches on it and RCCL orders against it
    stream = torch.cuda.Stream(device)
    torch.cuda.set_stream(stream)
    # a plain run: set up, warm up, time the steps, dump, print; every other leg needs --full
    full = args.full and not args.pmc_child
    collect = bool(args.dump_outputs) or (full and not args.no_cpu_baseline)
    m = measure_pr(csr, args, ctx, device, stream, world, rank, dist, collect=collect)
    elapsed = m["elapsed"]
    edges_total = nnz * args.iters * args.steps
    value = edges_total / elapsed
    ms_per_step = elapsed * 1e3 / args.steps
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"pagerank": m["result"]})
    traffic, traffic_src = None, None
    if world == 1 and full:
        if args.pmc_traffic == "run":
            traffic, traffic_src = measure_pr_traffic(gname)
            if traffic is None:   # e.g. no profiler access: the committed pass, labelled as such
                why = traffic_src
                traffic = pmc_traffic(workload)
                traffic_src = f"profiles/pmc_pr_pull.json (committed; the in-run passes: {why})"
        else:
            traffic, traffic_src = pmc_traffic(workload), "profiles/pmc_pr_pull.json (committed)"
    copy_gbs = stream_copy_gbs(device) if rank == 0 and full else None

    exe = None
    secondary = None
    cpu = None
    parity = None
    ref = None
    if rank == 0 and world == 1 and full:
        exe, exe_r = exe_path_pr(csr, args, ctx)
        if not args.no_cpu_baseline:
            from oracle import oracle as O
            threads = usable_cores()
            # bounded sample: whole PageRank runs on the same graph until the budget is spent
            runs, t_cpu, ref = 0, 0.0, None
            while runs == 0 or (t_cpu < args.cpu_seconds and runs < 200):
                t1 = time.perf_counter()
                ref = O.pagerank(csr, False, args.damping, args.iters, nthreads=threads)
                t_cpu += time.perf_counter() - t1
                runs += 1
            cpu = {"value": nnz * args.iters * runs / t_cpu, "unit": "edges/s", "cores": threads, "kind": "port",
                   "sample": f"{runs} full PageRank run(s) ({args.iters} iterations) on the same {gname} graph, "
                             f"OpenMP pull restatement (oracle/gx_oracle.c) on {threads} threads, {t_cpu:.2f} s",
                   **host_cpu()}
            exe["parity_max_rel_err_vs_oracle"] = float(np.max(np.abs(exe_r - ref) / np.abs(ref)))
        if not args.no_secondary and gname != "SYN-7_5":
            # configs[1]'s graph (datagen-7_5-fb stand-in), same measurement, no CPU leg
            S = PRESETS["SYN-7_5"]
            csr2 = rmat(S["scale"], S["ef"], S["seed"], undirected=True)
            m2 = measure_pr(csr2, args, ctx, device, stream, 1, 0, None, collect=True)
            err2 = None
            if not args.no_cpu_baseline:
                ref2 = O.pagerank(csr2, False, args.damping, args.iters, nthreads=usable_cores())
                err2 = float(np.max(np.abs(m2["result"] - ref2) / np.abs(ref2)))
            secondary = {"workload": pr_workload("SYN-7_5"), "n": csr2.n, "nnz": csr2.nnz,
                         "value": csr2.nnz * args.iters * args.steps / m2["elapsed"],
                         "ms_per_step": m2["elapsed"] * 1e3 / args.steps,
                         "mean_launch_us": m2["mean_launch_s"] * 1e6, "bytes_per_launch": m2["bytes_per_launch"],
                         "roofline_frac": m2["achieved"] / HBM_PEAK_GBS,
                         "traffic": pmc_traffic(pr_workload("SYN-7_5")),
                         # the timed steps' result against the fp64 oracle
                         "parity_max_rel_err_vs_oracle": err2,
                         # bin/exe/pr's processing time on this graph too
                         "processing": exe_path_pr(csr2, args, ctx)[0]}

    if rank == 0 and not args.no_cpu_baseline and full:
        # the last timed step's scores (gathered from every rank at N > 1) against the fp64 oracle
        from oracle import oracle as O
        if ref is None:
            ref = O.pagerank(csr, False, args.damping, args.iters, nthreads=usable_cores())
        parity = float(np.max(np.abs(m["result"] - ref) / np.abs(ref)))
    if rank == 0:
        achieved = m["achieved"]
        line = {
            "metric": METRIC,
            "value": value,
            "unit": "edges/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": f"synthetic (seeded R-MAT stand-in for {P['stands_for']}; no network for the real dataset)",
            "config": {
                "workload": workload,
                "algorithm": "pagerank",
                "graph": gname,
                "n": n,
                "nnz": nnz,
                "iterations": args.iters,
                "damping": args.damping,
                "parallelism": f"row{world}" + (f", {m['pieces']} pipelined pieces" if m["pieces"] > 1 else ""),
                "partition": (m["partition"] + " over " + str(m["vranks"]) + " virtual ranks") if m["vranks"] > 1
                else "one rank",
                "exchanged_doubles_per_n": m["exchanged"],
                "driver": m["driver"] + (", hipGraph" if m["driver"] == "device" and m["use_graph"] else ""),
                "exchange": m["exchange"],
                "roofline_events": "timed steps" if m["events_in_timed"] else "instrumented pass after the timed steps",
                "device": dev_name,
                "cus": cus,
            },
            "roofline": {
                "kernel": "k_pr_pull_units",
                "bound": "hbm",
                "achieved": achieved,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS,
                "traffic": traffic,
                "traffic_source": traffic_src,
                "traffic_over_algorithmic": traffic / m["bytes_per_launch"] if traffic else None,
                "bytes_per_launch": m["bytes_per_launch"],
                "mean_launch_us": m["mean_launch_s"] * 1e6,
                "launches": m["launches"],
                "stream_copy_gbs": copy_gbs,
                "frac_of_stream": achieved / copy_gbs if copy_gbs else None,
            },
            "processing_ms": exe["processing_ms"] if exe else None,
            "processing": exe,
            "evps": (n + nnz // 2) / (exe["processing_ms"] / 1e3) if exe else None,
            "bench_setup_ms": (m["t_setup"] + m["t_first"]) * 1e3,
            "cpu_baseline": cpu,
            "speedup_vs_cpu": value / cpu["value"] if cpu else None,
            "parity_max_rel_err_vs_oracle": parity,
            "secondary": secondary,
            "graph_gen_s": t_gen,
        }
        print(json.dumps(line), flush=True)
    ctx.close()
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
