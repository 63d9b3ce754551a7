#!/usr/bin/env python3
"""Offline model of PageRank's pair slots (gather_pairs, gx_pr_sorted.hip).

A pair slot holds two entries of a block whose columns lie in one 16-byte aligned pair of x
(columns 2p and 2p + 1), so one 16-byte load per lane serves both.  This cuts the hub-first rows
as the plan does (tools/pr_tail_order_model.py: 16 320 rows / 32 Mi entries per block on a huge
graph; --rows 4096 --block 1048576 for SYN-7_5), sorts every block's entries by column and, for
each rule choosing the entries to put in slots, counts

- covered entries;
- fillers: half fillers (a column pair holding an odd number of the block's covered entries ends
  in a half-empty slot) and, for the prefix rules, step fillers (a pair more than 3 pairs past the
  previous one is preceded by ceil(step / 3) - 1 slots with two empty halves);
- slots: (covered + fillers) / 2;
- gather wave-instructions removed: (covered - slots) / 64, against one 8-byte gather per entry
  (entries / 64 per launch in all).

Rules: the prefix of each block's columns below 64 Ki / 256 Ki / 1 Mi, and (not a prefix, so
without step fillers: an upper bound for a layout that could skip freely) every column pair with
at least 4 of the block's entries.  --quads also prints the four-entry slots of one column pair
for the prefix rules (a follow-up, not built).

These are counts, not times: what a removed gather instruction is worth is measured on the GPU
(timing probe 19, since removed, and the A/B runs of GX_PR_PAIRS, both in DESIGN.md 4).

python tools/pr_pair_model.py [scale edgefactor seed] [--rows R] [--block B] [--quads]
(default 23 40 85: SYN-8_5, about 40 GB of host memory; 20 32 75 --rows 4096 --block 1048576: SYN-7_5)"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat  # noqa: E402

from pr_tail_order_model import cut  # noqa: E402  (the plan's block cut)


def sorted_blocks(csr, R=16320, B=32 << 20):
    """(block, column) of every entry in the plan's order: hub-first rows cut into blocks of at
    most R rows and B entries, each block's entries sorted by hub-first column."""
    rp = csr.rowptr.astype(np.int64)
    ci = csr.colidx.astype(np.int64)
    deg = np.diff(rp)
    n = len(deg)
    order = np.argsort(-deg, kind="stable")
    perm = np.empty(n, dtype=np.int64)
    perm[order] = np.arange(n)
    st = cut(deg[order], R, B)
    bpos = np.searchsorted(st, np.arange(n), side="right") - 1   # block of each position
    bvert = bpos[perm].astype(np.uint64)                         # block of each vertex's row
    erow = np.repeat(np.arange(n, dtype=np.int64), deg)
    key = (bvert[erow] << np.uint64(32)) | perm[ci].astype(np.uint64)
    del erow
    key.sort()
    return (key >> np.uint64(32)).astype(np.int64), (key & np.uint64(0xFFFFFFFF)).astype(np.int64)


def pair_slots(blk, col, covered, step_fillers=True, width=2):
    """The slots of the covered entries (a boolean mask over the sorted entries).  Returns a dict:
    covered, half (empty halves of the runs' last slots), step (filler slots), fillers (empty
    halves in all), slots, and lead / partner: the sorted-entry indices of each real slot's first
    entry and of its second (-1: a half filler; width 2 only)."""
    idx = np.flatnonzero(covered)
    b, p = blk[idx], col[idx] >> 1
    m = len(idx)
    if m == 0:
        z = np.zeros(0, dtype=np.int64)
        return dict(covered=0, half=0, step=0, fillers=0, slots=0, lead=z, partner=z)
    new = np.ones(m, dtype=bool)            # first entry of a (block, pair) run
    new[1:] = (b[1:] != b[:-1]) | (p[1:] != p[:-1])
    pos = np.arange(m, dtype=np.int64)
    start = np.maximum.accumulate(np.where(new, pos, 0))
    k = pos - start                         # rank inside the run
    leads = (k % width) == 0
    runs = np.flatnonzero(new)
    length = np.diff(np.append(runs, m))
    real = int(leads.sum())
    half = int(real * width - m)            # empty places of the runs' last slots
    nstep = 0
    if step_fillers:
        s = p[runs][1:] - p[runs][:-1]
        same = b[runs][1:] == b[runs][:-1]
        s = s[same & (s > 3)]
        nstep = int(((s + 2) // 3 - 1).sum())
    out = dict(covered=m, half=half, step=nstep, fillers=half + width * nstep, slots=real + nstep, runs=len(length))
    if width == 2:
        li = pos[leads]
        has = (li + 1 < m)
        nxt = np.minimum(li + 1, m - 1)
        has &= ~new[nxt]
        out["lead"] = idx[li]
        out["partner"] = np.where(has, idx[nxt], -1)
    return out


def rules(blk, col):
    """(name, covered mask, is a prefix) for each rule."""
    out = [(f"columns below {c >> 10} Ki", col < c, True) for c in (64 << 10, 256 << 10, 1 << 20)]
    m = len(col)
    p = col >> 1
    new = np.ones(m, dtype=bool)
    new[1:] = (blk[1:] != blk[:-1]) | (p[1:] != p[:-1])
    runs = np.flatnonzero(new)
    length = np.diff(np.append(runs, m))
    out.append(("column pairs with >= 4 entries (not a prefix)", np.repeat(length >= 4, length), False))
    return out


def report(name, total, st):
    removed = st["covered"] - st["slots"]
    print(f"{name}: covered {st['covered']} ({st['covered'] / total:.3f}); fillers {st['fillers']} "
          f"({st['fillers'] / total:.3f}: {st['half']} half ({st['half'] / total:.3f}), {st['step']} step slots); "
          f"slots {st['slots']}; gather wave-instructions removed {removed // 64} of {total // 64} ({removed / total:.3f}; "
          f"{(removed + st['step']) / total:.3f} without the step slots)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("graph", nargs="*", type=int, default=[23, 40, 85])
    ap.add_argument("--rows", type=int, default=16320)
    ap.add_argument("--block", type=int, default=32 << 20)
    ap.add_argument("--quads", action="store_true")
    a = ap.parse_args()
    scale, ef, seed = a.graph[:3]
    t = time.time()
    csr = rmat(scale, ef, seed)
    blk, col = sorted_blocks(csr, a.rows, a.block)
    total = len(col)
    print(f"R-MAT {scale}/{ef}/{seed}: n {csr.n} nnz {total}; {int(blk[-1]) + 1} blocks of <= {a.rows} rows, "
          f"<= {a.block} entries ({time.time() - t:.0f} s)", flush=True)
    for name, covered, prefix in rules(blk, col):
        report(name, total, pair_slots(blk, col, covered, step_fillers=prefix))
        if a.quads and prefix:
            report(name + " [four-entry slots]", total, pair_slots(blk, col, covered, step_fillers=True, width=4))


if __name__ == "__main__":
    main()
