#!/usr/bin/env python3
"""Offline model of PageRank's run groups (GX_PR_RUNS, gather_runs): what a run
region ahead of the pair prefix of every sorted block does to the index bytes, the vector memory
wave-instructions and the LDS-array cycles of one k_pr_pull_units launch.

A run group is 64 two-byte codes (sel << 14 | row) of one column pair; a pair's run inside the
region is padded at its end to whole groups, and a run supergroup of 8 groups (512 codes, one
16-byte load per lane) carries a header of 8 pair indices (32 bytes).  The run prefix R of a block
is the prefix of its 256-entry supergroups that maximises entries - w x padding codes
(k_run_cost, k_narrow_split), the padding of a run counted in the supergroup holding the run's
last entry; the pair and narrow prefixes are then chosen from R on as before.

Per block class and weight w (GX_PR_RUN_FILL_COST, quarters of an entry per padding code) it
prints R, the entries covered, the padding codes, the index bytes (headers and bases included),
the vector memory wave-instructions (run 3 per 512 codes, pair 6 per 256 slots = 512 entries,
narrow 10 per 512 codes, wide 11 per 512 entries) and the LDS-array cycles with the bank order
applied to every region (tools/pr_bank_model.py), all per launch and before -> after.  The same
counts for groups of 32 codes (16 groups and a 64-byte header per supergroup) are printed as a
note.

python tools/pr_run_model.py [scale edgefactor seed] [--rows R] [--block B] [--every K] [--w W ...]
(default 23 40 85, every 8th block: SYN-8_5 as tools/pr_bank_model.py models it)"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from pr_bank_model import (JUNK, bank_order, block_cycles, block_entries, group_cycles, prefix_split,  # noqa: E402
                           run_starts, splits)

RUN_FILL_COST = 32   # GX_PR_RUN_FILL_COST: quarters of an entry per padding code


def run_lengths(col, n):
    """Lengths of the column-pair runs of the first n sorted entries (the last one cut at n)."""
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    first = np.flatnonzero(run_starts(col[:n] >> 1))
    return np.diff(np.append(first, n))


def run_prefix(col, w4=RUN_FILL_COST, group=64):
    """R: the block's run prefix in 256-entry supergroups (k_run_cost + k_narrow_split)."""
    N = len(col)
    if N == 0:
        return 0
    ng = (N + 255) >> 8
    cnt = np.minimum(256, N - 256 * np.arange(ng))
    first = np.flatnonzero(run_starts(col >> 1))
    length = np.diff(np.append(first, N))
    last = first + length - 1
    pad = (-length) % group
    fill = np.bincount(last >> 8, weights=pad, minlength=ng).astype(np.int64)
    return prefix_split(4 * cnt - w4 * fill)


def run_codes(col, row, R, group=64, order=True):
    """The rows of the run region's codes in code order (padding: the lane's junk row), padded to
    whole 512-code supergroups, and (entries, padding codes, supergroups)."""
    Nr = min(len(col), R << 8)
    if Nr == 0:
        return np.zeros(0, dtype=np.int64), (0, 0, 0)
    c, r = col[:Nr], row[:Nr]
    if order:   # k_bank_order on the region: runs keyed by column pair, plain positions
        _, r = bank_order(c >> 1, r, 0, R)
    length = run_lengths(c, Nr)
    codes = (length + group - 1) // group * group
    start = np.cumsum(codes) - codes
    at = np.repeat(start, length) + (np.arange(Nr) - np.repeat(np.cumsum(length) - length, length))
    total = int(codes.sum())
    nsg = (total + 511) // 512
    out = JUNK + (np.arange(nsg * 512) & 63)
    out[at] = r
    return out, (Nr, total - Nr, nsg)


def block_counts(col, row, w4, group=64, runs=True):
    """One block's launch: dict of entries / codes / bytes / vmem instructions / LDS cycles."""
    N = len(col)
    R = run_prefix(col, w4, group) if runs else 0
    rows_r, (Nr, pad, rsg) = run_codes(col, row, R, group)
    c2, r2 = col[Nr:], row[Nr:]
    Q, P = splits(c2) if len(c2) else (0, 0)
    c2, r2 = bank_order(c2, r2, Q, P) if len(c2) else (c2, r2)
    cyc = block_cycles(c2, r2, Q, P) if len(c2) else {"pair": (0, 0), "narrow": (0, 0), "wide": (0, 0)}
    psg = cyc["pair"][0] * 16 // 2 // 256          # 256-slot supergroups
    nsg = cyc["narrow"][0] * 16 // 512             # 512-code supergroups
    wide = len(c2) - min(len(c2), P << 8)
    wsg = (wide + 255) // 256
    hdr = 4 * (512 // group)
    return dict(R=R, run_entries=Nr, run_pad=pad, run_sg=rsg, entries=N,
                bytes=rsg * (1024 + hdr) + psg * (1024 + 4) + nsg * (1024 + 4) + 4 * wide + 4 * wsg,
                vmem=3 * rsg + 6 * psg + 10 * nsg + (11 * wsg + 1) // 2,
                lds=group_cycles(rows_r.reshape(-1, 16)) + cyc["pair"][1] + cyc["narrow"][1] + cyc["wide"][1],
                run_lds=group_cycles(rows_r.reshape(-1, 16)))


KEYS = ("R", "run_entries", "run_pad", "run_sg", "entries", "bytes", "vmem", "lds", "run_lds")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("graph", nargs="*", type=int, default=[23, 40, 85])
    ap.add_argument("--rows", type=int, default=16320)
    ap.add_argument("--block", type=int, default=32 << 20)
    ap.add_argument("--every", type=int, default=8)
    ap.add_argument("--w", type=int, nargs="*", default=[2, 4, 8, 16, 32])
    a = ap.parse_args()
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat
    scale, ef, seed = a.graph[:3]
    t0 = time.time()
    csr = rmat(scale, ef, seed)
    print(f"R-MAT {scale}/{ef}/{seed}: n {csr.n} nnz {csr.nnz}; blocks of <= {a.rows} rows, <= {a.block} entries; "
          f"every {a.every}. block with entries modelled, counts scaled by {a.every} to a launch ({time.time() - t0:.0f} s)",
          flush=True)
    classes = ("entry-limited", "row-limited")
    cases = [("before", 0, 64, False)] + [(f"w4={w}", w, 64, True) for w in a.w] + [(f"w4={w} g32", w, 32, True) for w in a.w]
    tot = {(name, c): np.zeros(len(KEYS) + 1, dtype=np.int64) for name, _, _, _ in cases for c in classes}
    for b, (nrows, col, row) in enumerate(block_entries(csr, a.rows, a.block)):
        if b % a.every:
            continue
        cls = "row-limited" if nrows == a.rows else "entry-limited"
        for name, w, group, runs in cases:
            d = block_counts(col, row, w, group, runs)
            tot[(name, cls)] += np.array([d[k] for k in KEYS] + [1])
    print(f"modelled ({time.time() - t0:.0f} s).  Per launch; R is the mean over the class's blocks, in 256-entry supergroups.")
    print(f"{'case':12s} {'block class':14s} {'blocks':>6s} {'R':>8s} {'run entries':>12s} {'share':>6s} {'padding':>10s} "
          f"{'index bytes':>13s} {'x before':>8s} {'vmem insts':>10s} {'x before':>8s} {'LDS cycles':>11s} {'x before':>8s}")
    for name, _, _, _ in cases:
        allv = np.zeros(len(KEYS) + 1, dtype=np.int64)
        allb = np.zeros(len(KEYS) + 1, dtype=np.int64)
        for c in classes + ("all",):
            if c == "all":
                v, b0 = allv, allb
            else:
                v, b0 = tot[(name, c)], tot[("before", c)]
                allv += v
                allb += b0
            if v[-1] == 0:
                continue
            d = dict(zip(KEYS, v))
            d0 = dict(zip(KEYS, b0))
            s = a.every
            print(f"{name:12s} {c:14s} {v[-1]:6d} {d['R'] / v[-1]:8.1f} {s * d['run_entries']:12d} "
                  f"{d['run_entries'] / max(d['entries'], 1):6.3f} {s * d['run_pad']:10d} {s * d['bytes']:13d} "
                  f"{d['bytes'] / max(d0['bytes'], 1):8.4f} {s * d['vmem']:10d} {d['vmem'] / max(d0['vmem'], 1):8.4f} "
                  f"{s * d['lds']:11d} {d['lds'] / max(d0['lds'], 1):8.4f}")


if __name__ == "__main__":
    main()
