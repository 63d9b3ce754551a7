#!/usr/bin/env python3
"""Device time of a statistics-only gx_scc beside one gx_wcc and two gx_bfs from the pivot on the same graph.

    python tools/scc_time.py [--graphs cit,rmat] [--scale 22] [--edgefactor 16] [--seed 22] [--reps 7]
                             [--solo 0,256,4096] [--batch 2,8,32] [--tiers 8:512,32:2048] [--grid 512,2048]
                             [--chain 4096]

The graphs are directed: `cit` is gx_rmat_csr(22, 4, 3), the stand-in the bench uses for SYN-cit, `rmat`
gx_rmat_csr(scale, edgefactor, seed).  After a warm-up call (the first builds the transpose and the
graph's buffers) every figure is gx_last_device_ms of a call: the median of `reps` calls, with the
smallest and the largest beside it:
  - gx_scc returning only its statistics, which are printed;
  - the rounds per phase (from GX_SCC_VERBOSE's last line: outer iterations, trim rounds, the pivot's
    levels, colour rounds, backward levels, steps), the microseconds every stage took (its `us` line:
    the device's wall clock between two plans, launch gaps included) and the kernel launches (gx_kernel_stats of a call
    with kernel timing on);
  - the yardsticks: gx_wcc, one existing pass over the same entries, and two gx_bfs calls from the pivot
    (the traversal the pivot phase does forward; gx_scc does it backward too);
  - the same call under GX_SCC_PIVOT=0 and under GX_SCC_TRIM=0, with their rounds; the statistics must
    not change;
  - with --solo / --batch / --grid / --tiers, the call under each value of GX_SCC_SOLO / GX_SCC_BATCH /
    GX_SCC_GRID / GX_SCC_SHORT:GX_SCC_LONG, alternated in the same process;
  - with --chain N, the N-ring and the N-path under each GX_SCC_SOLO of --solo (default 0 and the
    library's default).
Ends with one JSON line.  Needs a gfx950 device; there is no CPU path.
"""
import argparse
import json
import os
import re
import sys
import tempfile
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A   # noqa: E402
from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges, rmat   # noqa: E402

LINE = re.compile(r"outer (\d+) trim (\d+) levels (\d+) colour (\d+) back (\d+) pivot (-?\d+) alive (\d+) steps (\d+) done (\d+)")
FIELDS = ("outer", "trim_rounds", "pivot_levels", "colour_rounds", "back_levels", "pivot", "alive", "steps", "done")
STAGE_US = re.compile(r"gx_scc: us((?: \w+ [\d.]+)+)")
KERNELS = ("scc_prep", "scc_init", "scc_plan", "scc_step", "scc_finish")


def traced(fn):
    """fn() with GX_SCC_VERBOSE set and the library's stderr lines parsed: (host reads, the last line's fields)."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["GX_SCC_VERBOSE"] = "1"
        try:
            fn()
        finally:
            os.environ.pop("GX_SCC_VERBOSE")
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    lines = [dict(zip(FIELDS, (int(x) for x in m.groups()))) for m in LINE.finditer(text)]
    us = STAGE_US.search(text)
    if us:   # the stages' device time, launch gaps included; the stages that never ran are left out
        words = us.group(1).split()
        lines[-1]["stage_us"] = {k: float(v) for k, v in zip(words[::2], words[1::2]) if float(v) > 0}
    return len(lines), lines[-1]


def spread(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


class Bench:
    def __init__(self, ctx, reps):
        self.ctx, self.reps, self.same = ctx, reps, True

    def timed(self, fn, reps=None):
        ms, res = [], None
        for _ in range(reps or self.reps):
            res = fn()
            ms.append(self.ctx.last_device_ms())
        return spread(ms), res

    def sweep(self, title, forms, call, want):
        """Every form's call alternated `reps` times; medians per form."""
        times = {key: [] for key, _ in forms}
        for _ in range(self.reps):
            for key, env in forms:
                os.environ.update(env)
                self.same = (call() == want) and self.same
                times[key].append(self.ctx.last_device_ms())
                for k in env:
                    os.environ.pop(k)
        res = {key: spread(v) for key, v in times.items()}
        for key, v in res.items():
            print(f"{title} {key:>10}: {v['median_ms']:.3f} [{v['min_ms']:.3f}, {v['max_ms']:.3f}] ms", flush=True)
        return res


def stats_of(G):
    return [int(x) for x in A.LA_SCC(G, comp=False, stats=True)]


def one_graph(B, name, csr, a):
    ctx = B.ctx
    print(f"{name}  n {csr.n}  nnz {csr.nnz}", flush=True)
    G = A.Graph(ctx, csr, directed=True)
    out = {"graph": name, "n": int(csr.n), "nnz": int(csr.nnz)}
    want = stats_of(G)   # warm-up: builds the transpose and the buffers
    print(f"first gx_scc (buffers built) {ctx.last_device_ms():.3f} ms  stats {want}", flush=True)
    t, _ = B.timed(lambda: stats_of(G))
    reads, last = traced(lambda: stats_of(G))
    ctx.set_kernel_timing(True)
    ctx.reset_kernel_stats()
    stats_of(G)
    split = {kn: [ctx.kernel_stats(kn)[0], round(ctx.kernel_stats(kn)[1], 3)] for kn in KERNELS}
    ctx.set_kernel_timing(False)
    out["scc"] = dict(t, components=want[0], largest=want[1], singletons=want[2], host_reads=reads, rounds=last,
                      kernel_launches=sum(v[0] for v in split.values()), timed_split_launches_ms=split)
    print(f"gx_scc {t}  rounds {last}  host reads {reads}", flush=True)
    print(f"      split {split}", flush=True)
    A.WeaklyConnectedComponents(G)
    out["wcc"], _ = B.timed(lambda: A.WeaklyConnectedComponents(G))
    pivot = last["pivot"]
    A.LA_BFS(G, pivot)
    out["bfs_from_pivot"], lev = B.timed(lambda: A.LA_BFS(G, pivot))
    out["bfs_from_pivot"]["reached"] = int((lev != np.iinfo(np.int64).max).sum())
    out["bfs_from_pivot"]["levels"] = int(lev[lev != np.iinfo(np.int64).max].max())
    out["two_bfs_ms"] = round(2 * out["bfs_from_pivot"]["median_ms"], 3)
    print(f"gx_wcc {out['wcc']}  gx_bfs from the pivot {pivot} {out['bfs_from_pivot']}", flush=True)
    for key in ("GX_SCC_PIVOT", "GX_SCC_TRIM"):
        os.environ[key] = "0"
        t, got = B.timed(lambda: stats_of(G), reps=max(3, B.reps // 2))
        reads, last = traced(lambda: stats_of(G))
        os.environ.pop(key)
        B.same = (got == want) and B.same
        out[key + "=0"] = dict(t, rounds=last, host_reads=reads)
        print(f"{key}=0 {t}  rounds {last}", flush=True)
    call = lambda: stats_of(G)   # noqa: E731
    if a.solo:
        out["solo"] = B.sweep("GX_SCC_SOLO", [("default", {})] + [(x, {"GX_SCC_SOLO": x}) for x in a.solo.split(",")],
                              call, want)
    if a.batch:
        out["batch"] = B.sweep("GX_SCC_BATCH", [("default", {})] + [(x, {"GX_SCC_BATCH": x}) for x in a.batch.split(",")],
                               call, want)
    if a.grid:
        out["grid"] = B.sweep("GX_SCC_GRID", [("default", {})] + [(x, {"GX_SCC_GRID": x}) for x in a.grid.split(",")],
                              call, want)
    if a.tiers:
        forms = [("default", {})]
        for pair in a.tiers.split(","):
            sh, lg = pair.split(":")
            forms.append((pair, {"GX_SCC_SHORT": sh, "GX_SCC_LONG": lg}))
        out["tiers"] = B.sweep("GX_SCC_SHORT:LONG", forms, call, want)
    G.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=str, default="cit,rmat")
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=22)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--solo", type=str, default="")
    ap.add_argument("--batch", type=str, default="")
    ap.add_argument("--tiers", type=str, default="")
    ap.add_argument("--grid", type=str, default="")
    ap.add_argument("--chain", type=int, default=0)
    a = ap.parse_args()
    ctx = A.Context(0)
    B = Bench(ctx, a.reps)
    out = {"reps": a.reps, "knob_defaults": {"GX_SCC_SHORT": A.SCC_SHORT, "GX_SCC_LONG": A.SCC_LONG,
                                            "GX_SCC_SOLO": A.SCC_SOLO, "GX_SCC_BATCH": A.SCC_BATCH}, "graphs": []}
    for which in [x for x in a.graphs.split(",") if x]:
        if which == "cit":
            out["graphs"].append(one_graph(B, "rmat(22,4,3) directed (SYN-cit stand-in)", rmat(22, 4, 3, undirected=False), a))
        else:
            out["graphs"].append(one_graph(B, f"rmat({a.scale},{a.edgefactor},{a.seed}) directed",
                                           rmat(a.scale, a.edgefactor, a.seed, undirected=False), a))
    if a.chain:
        v = np.arange(a.chain)
        solos = a.solo.split(",") if a.solo else ["0"]
        forms = [("default", {})] + [(x, {"GX_SCC_SOLO": x}) for x in solos]
        out["chain"] = {"vertices": a.chain}
        for name, csr, want in (("ring", csr_from_edges(a.chain, v, (v + 1) % a.chain, None, symmetric=False), [1, a.chain, 0]),
                                ("path", csr_from_edges(a.chain, v[1:], v[:-1], None, symmetric=False), [a.chain, 1, a.chain])):
            P = A.Graph(ctx, csr, directed=True)
            assert stats_of(P) == want
            _, last = traced(lambda: stats_of(P))
            out["chain"][name] = {"rounds": last, "solo": B.sweep(f"{name}({a.chain}) GX_SCC_SOLO", forms,
                                                                   lambda: stats_of(P), want)}
            P.close()
    out["results_equal_under_every_knob"] = bool(B.same)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
