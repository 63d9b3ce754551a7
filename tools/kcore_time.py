#!/usr/bin/env python3
"""Device time of gx_core_all and gx_kcore (k = 2, a middle k and kmax) beside one gx_wcc on the same graph.

    python tools/kcore_time.py [--scale 22] [--edgefactor 16] [--seed 22] [--reps 7]
                               [--solo 0,16,64,256,1024] [--batch 4,8,16,32,64]
                               [--tiers 8:512,16:1024,32:2048,64:4096] [--chain 4096]

The graph is gx_rmat_csr(scale, edgefactor, seed) undirected; the defaults are the stand-in the bench
uses for SYN-g500-22.  After warm-up calls (the first builds the graph's k-core cache) every figure is
gx_last_device_ms of a call that returns only its statistics: the median of `reps` calls, with the
smallest and the largest beside it:
  - gx_wcc, the yardstick: one existing full pass over the same graph's edges from the same process;
    the peel's time is also given as a number of such passes, which says how far the latency of a
    round, not the bytes, sets it;
  - gx_core_all: kmax, the rounds that removed a vertex and the steps (from GX_CORE_VERBOSE's last
    line), the kernel launches (gx_kernel_stats of a call with kernel timing on) and the time per round;
  - gx_kcore at k = 2, kmax // 2 and kmax, with the statistics;
  - with --solo / --batch / --tiers, gx_core_all and the middle gx_kcore under each value of
    GX_CORE_SOLO / GX_CORE_BATCH / GX_CORE_SHORT:GX_CORE_LONG, alternated in the same process; the
    results must not change;
  - with --chain N, gx_kcore at k = 2 on an N-vertex path (two vertices per round) under each
    GX_CORE_SOLO of --solo (default 0 and the library's default).
Ends with one JSON line.  Needs a gfx950 device; there is no CPU path.
"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from ldbc_graphalytics_platforms_graphblas_amd import _native as N   # noqa: E402
from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A   # noqa: E402
from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges, rmat   # noqa: E402

LINE = re.compile(r"k (\d+) rounds (\d+) alive (\d+) steps (\d+) done (\d+)")
KERNELS = ("core_prep", "core_init", "core_plan", "core_seed", "core_expand", "core_finish")


def traced(fn):
    """fn() with GX_CORE_VERBOSE set and the library's stderr lines parsed: [(k, rounds, alive, steps, done)]."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["GX_CORE_VERBOSE"] = "1"
        try:
            fn()
        finally:
            os.environ.pop("GX_CORE_VERBOSE")
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    return [tuple(int(x) for x in m.groups()) for m in LINE.finditer(text)]


def spread(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=22)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--solo", type=str, default="")
    ap.add_argument("--batch", type=str, default="")
    ap.add_argument("--tiers", type=str, default="")
    ap.add_argument("--chain", type=int, default=0)
    a = ap.parse_args()
    csr = rmat(a.scale, a.edgefactor, a.seed)
    name = f"rmat({a.scale},{a.edgefactor},{a.seed}) undirected"
    print(f"{name}  n {csr.n}  nnz {csr.nnz}", flush=True)
    ctx = A.Context(0)
    G = A.Graph(ctx, csr, directed=False)
    kmax_c = C.c_uint64(0)

    def timed(fn, reps=a.reps):
        ms, res = [], None
        for _ in range(reps):
            res = fn()
            ms.append(ctx.last_device_ms())
        return spread(ms), res

    def core_all(g=G):   # kmax alone: no n values cross the host link
        N.check(N.lib().gx_core_all(g.handle, None, C.byref(kmax_c)), "gx_core_all")
        return int(kmax_c.value)

    def kcore(k, g=G):
        return [int(x) for x in A.LA_KCore(g, k, degree=False, stats=True)]

    out = {"graph": name, "n": int(csr.n), "nnz": int(csr.nnz), "reps": a.reps,
           "knob_defaults": {"GX_CORE_SHORT": A.CORE_SHORT, "GX_CORE_LONG": A.CORE_LONG, "GX_CORE_SOLO": A.CORE_SOLO,
                             "GX_CORE_BATCH": A.CORE_BATCH}}
    for _ in range(2):   # the second gx_wcc on a graph moves to its hub-first copy: steady state from then on
        A.WeaklyConnectedComponents(G)
    out["wcc"], _ = timed(lambda: A.WeaklyConnectedComponents(G))
    print(f"gx_wcc {out['wcc']}", flush=True)
    kmax = core_all()   # warm-up: builds the cache
    print(f"first gx_core_all (cache built) {ctx.last_device_ms():.3f} ms  kmax {kmax}", flush=True)
    t, _ = timed(core_all)
    trace = traced(core_all)
    ctx.set_kernel_timing(True)
    ctx.reset_kernel_stats()
    core_all()
    split = {kn: [ctx.kernel_stats(kn)[0], round(ctx.kernel_stats(kn)[1], 3)] for kn in KERNELS}
    ctx.set_kernel_timing(False)
    rounds, steps = trace[-1][1], trace[-1][3]
    launches = sum(v[0] for v in split.values())
    out["core_all"] = dict(t, kmax=kmax, rounds=rounds, steps=steps, host_reads=len(trace), kernel_launches=launches,
                           us_per_round=round(1000.0 * t["median_ms"] / max(rounds, 1), 3),
                           wcc_passes=round(t["median_ms"] / out["wcc"]["median_ms"], 1),
                           timed_split_launches_ms=split)
    print(f"gx_core_all {t}  kmax {kmax} rounds {rounds} steps {steps} launches {launches} "
          f"{out['core_all']['us_per_round']} us/round = {out['core_all']['wcc_passes']} gx_wcc passes", flush=True)
    print(f"      split {split}", flush=True)
    mid = max(kmax // 2, 1)
    base = {}
    out["kcore"] = {}
    for k in sorted({2, mid, kmax}):
        t, st = timed(lambda: kcore(k))
        base[k] = st
        out["kcore"][str(k)] = dict(t, vertices=st[0], edges=st[1], rounds=st[2],
                                    us_per_round=round(1000.0 * t["median_ms"] / max(st[2], 1), 3))
        print(f"gx_kcore k {k}: {t}  vertices {st[0]} edges {st[1]} rounds {st[2]}", flush=True)
    same = True

    def sweep(title, forms, calls):
        """Every form's calls alternated `reps` times; medians per form and call."""
        nonlocal same
        times = {key: {w: [] for w, _, _ in calls} for key, _ in forms}
        for _ in range(a.reps):
            for key, env in forms:
                os.environ.update(env)
                for what, call, want in calls:
                    same = (call() == want) and same
                    times[key][what].append(ctx.last_device_ms())
                for k in env:
                    os.environ.pop(k)
        res = {key: {w: spread(v) for w, v in t.items()} for key, t in times.items()}
        for key, t in res.items():
            print(f"{title} {key:>10}: " + "  ".join(f"{w} {v['median_ms']:.3f} [{v['min_ms']:.3f}, {v['max_ms']:.3f}]"
                                                     for w, v in t.items()) + " ms", flush=True)
        return res

    calls = [("core_all", core_all, kmax), (f"kcore_{mid}", lambda: kcore(mid), base[mid])]
    if a.solo:
        out["solo"] = sweep("GX_CORE_SOLO", [("default", {})] + [(x, {"GX_CORE_SOLO": x}) for x in a.solo.split(",")], calls)
    if a.batch:
        out["batch"] = sweep("GX_CORE_BATCH", [("default", {})] + [(x, {"GX_CORE_BATCH": x}) for x in a.batch.split(",")],
                             calls)
    if a.tiers:
        forms = [("default", {})]
        for pair in a.tiers.split(","):
            sh, lg = pair.split(":")
            forms.append((pair, {"GX_CORE_SHORT": sh, "GX_CORE_LONG": lg}))
        out["tiers"] = sweep("GX_CORE_SHORT:LONG", forms, calls)
    G.close()
    if a.chain:
        v = np.arange(a.chain - 1)
        P = A.Graph(ctx, csr_from_edges(a.chain, v, v + 1, None, symmetric=True), directed=False)
        want = [0, 0, a.chain // 2]
        assert kcore(2, P) == want
        solos = a.solo.split(",") if a.solo else ["0"]
        out["chain"] = {"vertices": a.chain, "rounds": want[2],
                        "solo": sweep(f"path({a.chain}) GX_CORE_SOLO",
                                      [("default", {})] + [(x, {"GX_CORE_SOLO": x}) for x in solos],
                                      [("kcore_2", lambda: kcore(2, P), want)])}
        P.close()
    out["results_equal_under_every_knob"] = bool(same)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
