#!/usr/bin/env python3
"""Device time of one gx_betweenness batch beside the same sources' gx_bfs calls.

    python tools/bc_time.py [--scale 22] [--edgefactor 16] [--seed 22] [--rounds 5]

The graph is gx_rmat_csr(scale, edgefactor, seed) undirected (the defaults are SYN-g500-22); the
batch is GAP's four sources: the largest hub and the first three ids from 1 up that have an edge.
After one warm-up of each (code objects, the hub-first copy gx_bfs runs on from its second call),
`rounds` rounds alternate one LA_BC batch and four LA_BFS calls, each timed by gx_last_device_ms
(device events around the call's device work).  Prints the per-round times, the medians, whether
every batch was bit-equal to the first, the same batch with GX_BC_BITS=-1 (level probes instead of
the bitmap) alternated against the default, and -- from one more batch with kernel timing on,
outside the timed rounds -- the split over bc_bucket / bc_sigma / bc_delta.  Ends with one JSON line.
Needs a gfx950 device; there is no CPU path.
"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A   # noqa: E402
from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    csr = rmat(a.scale, a.edgefactor, a.seed)
    deg = np.diff(csr.rowptr.astype(np.int64))
    hub = int(np.argmax(deg))
    rest = [int(v) for v in np.flatnonzero(deg[1:] > 0)[:4] + 1 if int(v) != hub][:3]
    sources = [hub] + rest
    print(f"n {csr.n}  nnz {csr.nnz}  sources {sources}  degrees {[int(deg[s]) for s in sources]}", flush=True)
    ctx = A.Context(0)
    G = A.Graph(ctx, csr, directed=False)
    first, paths = A.LA_BC(G, sources, return_paths=True)   # warm-up; also the result the rounds must repeat
    print(f"reached {[int((p > 0).sum()) for p in paths]}  max sigma {paths.max():.6g}  "
          f"max centrality {first.max():.6g}", flush=True)
    for s in sources:   # the second call on a graph builds the hub-first copy gx_bfs then runs on
        A.LA_BFS(G, s)
        A.LA_BFS(G, s)
    bc_ms, bfs_ms, same = [], [], True
    for r in range(a.rounds):
        got = A.LA_BC(G, sources)
        bc_ms.append(ctx.last_device_ms())
        same = same and np.array_equal(got, first)
        t = 0.0
        for s in sources:
            A.LA_BFS(G, s)
            t += ctx.last_device_ms()
        bfs_ms.append(t)
        print(f"round {r}: gx_betweenness {bc_ms[-1]:.3f} ms   4 x gx_bfs {bfs_ms[-1]:.3f} ms", flush=True)
    # the probe knob, alternated in the same process: GX_BC_BITS = -1 reads level[x] everywhere
    ab = {"default": [], "-1": []}
    for r in range(a.rounds):
        for key in ab:
            if key != "default":
                os.environ["GX_BC_BITS"] = key
            got = A.LA_BC(G, sources)
            os.environ.pop("GX_BC_BITS", None)
            ab[key].append(ctx.last_device_ms())
            same = same and np.array_equal(got, first)
    print("GX_BC_BITS A/B, median ms: " + "  ".join(f"{k}: {np.median(v):.3f}" for k, v in ab.items()), flush=True)
    ctx.set_kernel_timing(True)
    ctx.reset_kernel_stats()
    A.LA_BC(G, sources)
    timed_ms = ctx.last_device_ms()
    split = {k: round(ctx.kernel_stats(k)[1], 3) for k in
             ("bc_bucket", "bc_sigma", "bc_delta", "bfs_frontier", "bfs_expand")}
    ctx.set_kernel_timing(False)
    out = {"graph": f"rmat({a.scale},{a.edgefactor},{a.seed}) undirected", "n": int(csr.n), "nnz": int(csr.nnz),
           "sources": sources, "rounds": a.rounds,
           "bc_device_ms_median": round(float(np.median(bc_ms)), 3), "bc_device_ms_min": round(min(bc_ms), 3),
           "bc_device_ms_max": round(max(bc_ms), 3),
           "bfs4_device_ms_median": round(float(np.median(bfs_ms)), 3), "bfs4_device_ms_min": round(min(bfs_ms), 3),
           "bfs4_device_ms_max": round(max(bfs_ms), 3),
           "level_probe_ms_median": round(float(np.median(ab["-1"])), 3),
           "bit_equal_every_round": bool(same), "timed_batch_ms": round(timed_ms, 3), "timed_split_ms": split}
    G.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
