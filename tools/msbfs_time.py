#!/usr/bin/env python3
"""Device time of one 64-source gx_msbfs call beside the same 64 sources' gx_bfs calls.

    python tools/msbfs_time.py [--scale 22] [--edgefactor 16] [--seed 22] [--rounds 5]
                               [--grid W H] [--alphas 8,64,512]

The graph is gx_rmat_csr(scale, edgefactor, seed) undirected (the defaults are SYN-g500-22), or with
--grid W H the W x H four-neighbour grid (a deep, thin graph: W + H - 2 levels from a corner).  The
sources are the largest hub plus the first 63 ids from 1 up that have an edge.  After one warm-up of
each side (code objects, the hub-first copy gx_bfs runs on from its second call), `rounds` rounds
alternate one LA_MSBFS(levels=False, stats=True) and the same 64 LA_BFS calls, each timed by
gx_last_device_ms (device events around the call's device work).  Prints the per-round times, the
medians, whether every call's statistics were bit-equal to the first and equal to those of the
gx_bfs rows; with --alphas the same call under each GX_MSBFS_ALPHA and both forced forms,
alternated in the same process; and -- from one more batch with kernel timing on, outside the
timed rounds -- the split over msbfs_pull / msbfs_push / msbfs_commit / msbfs_out.  Ends with one
JSON line.  Needs a gfx950 device; there is no CPU path.
"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A   # noqa: E402
from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges, rmat   # noqa: E402

MAX = np.iinfo(np.int64).max


def grid_graph(w, h):
    ids = np.arange(w * h, dtype=np.int64).reshape(h, w)
    src = np.concatenate([ids[:, :-1].ravel(), ids[:-1, :].ravel()])
    dst = np.concatenate([ids[:, 1:].ravel(), ids[1:, :].ravel()])
    return csr_from_edges(w * h, src, dst, None, symmetric=True)


def stats_of(level):
    reached = level != MAX
    return [int(reached.sum()), int(level[reached].sum()), int(level[reached].max())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--grid", type=int, nargs=2, metavar=("W", "H"))
    ap.add_argument("--alphas", type=str, default="")
    a = ap.parse_args()
    if a.grid:
        csr, name = grid_graph(*a.grid), f"grid({a.grid[0]},{a.grid[1]}) undirected"
    else:
        csr, name = rmat(a.scale, a.edgefactor, a.seed), f"rmat({a.scale},{a.edgefactor},{a.seed}) undirected"
    deg = np.diff(csr.rowptr.astype(np.int64))
    hub = int(np.argmax(deg))
    rest = [int(v) for v in np.flatnonzero(deg[1:] > 0)[:A.MSBFS_BATCH] + 1 if int(v) != hub][:A.MSBFS_BATCH - 1]
    sources = [hub] + rest
    print(f"{name}  n {csr.n}  nnz {csr.nnz}  sources {len(sources)}: {sources[:4]} ...", flush=True)
    ctx = A.Context(0)
    G = A.Graph(ctx, csr, directed=False)
    first = A.LA_MSBFS(G, sources, levels=False, stats=True)   # warm-up; also what the rounds must repeat
    print(f"reached {int(first[:, 0].min())}..{int(first[:, 0].max())}  largest level {int(first[:, 2].max())}",
          flush=True)
    same = True
    for s in sources:   # the second call on a graph builds the hub-first copy gx_bfs then runs on
        same = same and stats_of(A.LA_BFS(G, s)) == [int(x) for x in first[sources.index(s)]]
    A.LA_BFS(G, hub)
    ms_ms, bfs_ms = [], []
    for r in range(a.rounds):
        got = A.LA_MSBFS(G, sources, levels=False, stats=True)
        ms_ms.append(ctx.last_device_ms())
        same = same and np.array_equal(got, first)
        t = 0.0
        for s in sources:
            A.LA_BFS(G, s)
            t += ctx.last_device_ms()
        bfs_ms.append(t)
        print(f"round {r}: gx_msbfs {ms_ms[-1]:.3f} ms   {len(sources)} x gx_bfs {bfs_ms[-1]:.3f} ms", flush=True)
    ab = {}
    if a.alphas:
        forms = [("default", {})] + [(f"alpha={x}", {"GX_MSBFS_ALPHA": x}) for x in a.alphas.split(",")] + \
                [("push", {"GX_MSBFS_DIR": "push"}), ("pull", {"GX_MSBFS_DIR": "pull"})]
        times = {k: [] for k, _ in forms}
        for r in range(a.rounds):
            for key, env in forms:
                os.environ.update(env)
                got = A.LA_MSBFS(G, sources, levels=False, stats=True)
                for k in env:
                    os.environ.pop(k)
                times[key].append(ctx.last_device_ms())
                same = same and np.array_equal(got, first)
        ab = {k: round(float(np.median(v)), 3) for k, v in times.items()}
        print("forms, median ms: " + "  ".join(f"{k}: {v:.3f}" for k, v in ab.items()), flush=True)
    ctx.set_kernel_timing(True)
    ctx.reset_kernel_stats()
    A.LA_MSBFS(G, sources, levels=False, stats=True)
    timed_ms = ctx.last_device_ms()
    split = {k: [ctx.kernel_stats(k)[0], round(ctx.kernel_stats(k)[1], 3)] for k in
             ("msbfs_pull", "msbfs_push", "msbfs_commit", "msbfs_out")}
    ctx.set_kernel_timing(False)
    ms_med, bfs_med = float(np.median(ms_ms)), float(np.median(bfs_ms))
    out = {"graph": name, "n": int(csr.n), "nnz": int(csr.nnz), "sources": len(sources), "rounds": a.rounds,
           "msbfs_device_ms_median": round(ms_med, 3), "msbfs_device_ms_min": round(min(ms_ms), 3),
           "msbfs_device_ms_max": round(max(ms_ms), 3),
           "bfs64_device_ms_median": round(bfs_med, 3), "bfs64_device_ms_min": round(min(bfs_ms), 3),
           "bfs64_device_ms_max": round(max(bfs_ms), 3),
           "bfs64_over_msbfs": round(bfs_med / ms_med, 2), "msbfs_below_bfs64": bool(ms_med < bfs_med),
           "largest_level": int(first[:, 2].max()), "forms_ms_median": ab,
           "stats_equal_every_call_and_to_gx_bfs": bool(same), "timed_batch_ms": round(timed_ms, 3),
           "timed_split_launches_ms": split}
    G.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
