#!/usr/bin/env python3
"""Device time of gx_ktruss (k = 3, 4 and kmax) and gx_truss_all beside gx_mxm_masked on the same graph.

    python tools/ktruss_time.py [--scale 22] [--edgefactor 16] [--seed 22] [--rounds 3]
                                [--shares 0,5,10,25,50,100] [--tiers 8:512,16:1024,32:2048]
                                [--mxm-only] [--kmax K]

The graph is gx_rmat_csr(scale, edgefactor, seed) undirected; the defaults are the stand-in the bench
uses for SYN-g500-22.  After one warm-up call (it builds the graph's k-truss cache) every figure is
gx_last_device_ms of a call that returns only its statistics, the median of `rounds` calls:
  - gx_mxm_masked, the yardstick: one thread-per-entry support count of the whole graph (its device
    time includes the sort of its row-sorted copy; --mxm-only runs nothing else, so that a
    kernel-trace profiler sees k_op_mxm_pair alone);
  - gx_ktruss at k = 2 with kernel timing on: the first round's truss_support (every edge counted);
  - gx_ktruss at k = 3, 4 and kmax, with the statistics and, from one call under GX_TRUSS_VERBOSE,
    the edges recounted and removed in every round;
  - gx_truss_all, once (--kmax K skips it, here and in the sweeps, and takes K as kmax);
  - with --shares, k = 4, kmax and gx_truss_all under each GX_TRUSS_SHARE and both forced forms
    (GX_TRUSS_RECOUNT=all|marked), alternated in the same process; the statistics must not change;
  - with --tiers, k = 2's truss_support and the k = 4 call under each GX_TRUSS_SHORT:GX_TRUSS_LONG.
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
from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat   # noqa: E402

LINE = re.compile(r"k (\d+) round (\d+) alive (\d+) recounted (\d+) removed (\d+) next (\S+)")


def traced(fn):
    """fn() with GX_TRUSS_VERBOSE set and the library's stderr lines parsed: [(round, alive,
    recounted, removed, next form)]."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["GX_TRUSS_VERBOSE"] = "1"
        try:
            fn()
        finally:
            os.environ.pop("GX_TRUSS_VERBOSE")
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    return [(int(m[2]), int(m[3]), int(m[4]), int(m[5]), m[6]) for m in LINE.finditer(text)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shares", type=str, default="")
    ap.add_argument("--tiers", type=str, default="")
    ap.add_argument("--mxm-only", action="store_true")
    ap.add_argument("--kmax", type=int, default=0, help="skip gx_truss_all (also in the sweeps) and take this as kmax")
    a = ap.parse_args()
    csr = rmat(a.scale, a.edgefactor, a.seed)
    name = f"rmat({a.scale},{a.edgefactor},{a.seed}) undirected"
    print(f"{name}  n {csr.n}  nnz {csr.nnz}", flush=True)
    ctx = A.Context(0)
    G = A.Graph(ctx, csr, directed=False)

    def timed(fn, rounds=a.rounds):
        ms, res = [], None
        for _ in range(rounds):
            res = fn()
            ms.append(ctx.last_device_ms())
        return round(float(np.median(ms)), 3), res

    mxm_ms, c = timed(lambda: A.mxm_masked(G))
    mxm_sum = int(c.sum())
    del c
    print(f"gx_mxm_masked {mxm_ms:.3f} ms (device, the sort included)", flush=True)
    out = {"graph": name, "n": int(csr.n), "nnz": int(csr.nnz), "rounds": a.rounds, "mxm_masked_device_ms": mxm_ms}
    if a.mxm_only:
        G.close()
        ctx.close()
        print(json.dumps(out))
        return

    def ktruss(k):
        return [int(x) for x in A.LA_KTruss(G, k, support=False, stats=True)]

    first = ktruss(2)   # warm-up: builds the cache
    assert first == [csr.nnz // 2, mxm_sum // 6, 0], (first, mxm_sum)
    print(f"first call (cache built) {ctx.last_device_ms():.3f} ms: edges {first[0]} triangles {first[1]}", flush=True)

    def support_k2():
        ctx.set_kernel_timing(True)
        ms = []
        for _ in range(a.rounds):
            ctx.reset_kernel_stats()
            ktruss(2)
            ms.append(ctx.kernel_stats("truss_support")[1])
        ctx.set_kernel_timing(False)
        return round(float(np.median(ms)), 3)

    out["k2_truss_support_ms"] = support_k2()
    out["k2_device_ms"], _ = timed(lambda: ktruss(2))
    print(f"k 2: truss_support (every edge, lists included) {out['k2_truss_support_ms']:.3f} ms, "
          f"call {out['k2_device_ms']:.3f} ms", flush=True)
    kmax_c = C.c_uint64(0)

    def truss_all():   # kmax alone: no nnz values cross the host link
        N.check(N.lib().gx_truss_all(G.handle, None, C.byref(kmax_c)), "gx_truss_all")
        return int(kmax_c.value)

    if a.kmax:
        kmax = a.kmax
    else:
        out["truss_all_device_ms"], kmax = timed(truss_all, rounds=1)   # minutes at this size: once
        print(f"gx_truss_all {out['truss_all_device_ms']:.3f} ms  kmax {kmax}", flush=True)
    out["kmax"] = kmax
    ks = sorted({3, 4, kmax})
    base = {}
    out["ktruss"] = {}
    for k in ks:
        ms, st = timed(lambda: ktruss(k))
        base[k] = st
        rounds = traced(lambda: ktruss(k))
        ctx.set_kernel_timing(True)
        ctx.reset_kernel_stats()
        ktruss(k)
        split = {kn: [ctx.kernel_stats(kn)[0], round(ctx.kernel_stats(kn)[1], 3)] for kn in
                 ("truss_support", "truss_prune", "truss_mark", "truss_commit")}
        ctx.set_kernel_timing(False)
        out["ktruss"][str(k)] = {"device_ms": ms, "edges": st[0], "triangles": st[1], "rounds": st[2],
                                 "per_round_alive_recounted_removed_next": [r[1:] for r in rounds],
                                 "timed_split_launches_ms": split}
        shown = ", ".join(f"{r[2]}/{r[3]}{'*' if r[4] == 'all' else ''}" for r in rounds[:12])
        print(f"k {k}: {ms:.3f} ms  edges {st[0]} triangles {st[1]} rounds {st[2]}; recounted/removed per round "
              f"(* = the next round recounts all): {shown}{' ...' if len(rounds) > 12 else ''}", flush=True)
        print(f"      split {split}", flush=True)
    same = True
    if a.shares:
        forms = [("default", {})] + [(f"share={x}", {"GX_TRUSS_SHARE": x}) for x in a.shares.split(",")] + \
                [("all", {"GX_TRUSS_RECOUNT": "all"}), ("marked", {"GX_TRUSS_RECOUNT": "marked"})]
        times = {key: {"k4": [], "kmax": [], "all_k": []} for key, _ in forms}
        for _ in range(a.rounds):
            for key, env in forms:
                os.environ.update(env)
                for what, call, want in (("k4", lambda: ktruss(4), base[4]), ("kmax", lambda: ktruss(kmax), base[kmax]),
                                         ("all_k", truss_all, kmax))[:2 if a.kmax else 3]:
                    same = (call() == want) and same
                    times[key][what].append(ctx.last_device_ms())
                for k in env:
                    os.environ.pop(k)
        out["shares_ms_median"] = {key: {w: round(float(np.median(v)), 3) for w, v in t.items() if v}
                                   for key, t in times.items()}
        for key, t in out["shares_ms_median"].items():
            print(f"{key:>10}: k 4 {t['k4']:.3f}  k {kmax} {t['kmax']:.3f}" +
                  (f"  gx_truss_all {t['all_k']:.3f}" if "all_k" in t else "") + " ms", flush=True)
    if a.tiers:
        out["tiers"] = {}
        for pair in a.tiers.split(","):
            sh, lg = pair.split(":")
            os.environ.update({"GX_TRUSS_SHORT": sh, "GX_TRUSS_LONG": lg})
            same = (ktruss(2) == first) and same   # rebuilds the tier bytes
            sup = support_k2()
            ms, st = timed(lambda: ktruss(4))
            same = (st == base[4]) and same
            for k in ("GX_TRUSS_SHORT", "GX_TRUSS_LONG"):
                os.environ.pop(k)
            out["tiers"][pair] = {"k2_truss_support_ms": sup, "k4_device_ms": ms}
            print(f"tiers {pair}: k 2 truss_support {sup:.3f} ms  k 4 {ms:.3f} ms", flush=True)
        ktruss(2)   # back to the defaults' tier bytes
    out["stats_equal_under_every_knob"] = bool(same)
    out["k2_support_below_mxm_masked"] = bool(out["k2_truss_support_ms"] <= mxm_ms)
    G.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
