#!/usr/bin/env python3
"""Offline model of the LDS bank conflicts of PageRank's row adds (k_pr_pull_units)
and of the bank-aware order inside column runs (GX_PR_BANK_ORDER, k_bank_order).

A no-return LDS add of a double is served in groups of 16 consecutive lanes; two different rows
of a group collide when they are equal mod 16 (tools/lds_add_banks.hip measures this), and a
group takes as many LDS-array cycles as its fullest slot holds rows.  The model cuts the graph as
the plan does (tools/pr_pair_model.py), chooses each block's pair prefix Q and narrow prefix P as
k_narrow_split does, lays the entries out as k_pair_emit, k_narrow_emit and the wide X4 rounds
do (step fillers, half fillers, junk rows and padding included), and counts the LDS-array cycles
of a launch for

- the present order (ascending rows inside a run; the wide part after k_sorted_laneperm),
- the bank-aware order (each piece of a run inside a 2 Ki-entry tile dealt round-robin over its
  rows' classes, gx_pr_bank.h; the wide part unchanged; --tile for other tile sizes),
- the conflict-free bound (one cycle per group).

It also prints the share of entries in runs of at least 16 and 64 entries, by region and by block
class (entry-limited: the block ends at its entry limit; row-limited: at its row limit).

These are cycle counts of the LDS array alone, not times.

python tools/pr_bank_model.py [scale edgefactor seed] [--rows R] [--block B] [--every K] [--tile T]
(default 23 40 85: SYN-8_5; --every K models every K-th block only)"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat  # noqa: E402

from pr_tail_order_model import cut  # noqa: E402  (the plan's block cut)

JUNK = 16320          # kJunkRow: fillers and padding add into accumulators JUNK + lane
PAIR_FILL_COST = 48   # GX_PR_PAIR_FILL_COST: quarters of an entry per filler half


def block_entries(csr, R=16320, B=32 << 20):
    """Yields (rows of the block, col, row) per block with entries, in the plan's order: hub-first
    rows cut into blocks of at most R rows and B entries; each block's entries sorted by hub-first
    column, equal columns by ascending row of the block (the plan's stable sort)."""
    rp = csr.rowptr.astype(np.int64)
    ci = csr.colidx.astype(np.int64)
    deg = np.diff(rp)
    n = len(deg)
    order = np.argsort(-deg, kind="stable")
    perm = np.empty(n, dtype=np.int64)
    perm[order] = np.arange(n)
    st = cut(deg[order], R, B)
    for b in range(len(st) - 1):
        r0, r1 = int(st[b]), int(st[b + 1])
        verts = order[r0:r1]
        d = deg[verts]
        if d.sum() == 0:
            continue
        idx = np.repeat(rp[verts] - (np.cumsum(d) - d), d) + np.arange(int(d.sum()))   # the rows' entries, row by row
        row = np.repeat(np.arange(r1 - r0, dtype=np.int64), d)
        key = (perm[ci[idx]] << 14) | row
        key.sort()
        yield r1 - r0, key >> 14, key & 16383


def prefix_split(benefit):
    """The prefix of supergroups with the largest benefit sum (the shortest on ties, 0 if none)."""
    if len(benefit) == 0:
        return 0
    c = np.cumsum(benefit)
    k = int(np.argmax(c))
    return k + 1 if c[k] > 0 else 0


def run_starts(key):
    new = np.ones(len(key), dtype=bool)
    new[1:] = key[1:] != key[:-1]
    return new


def splits(col, pairs=True, narrow=True):
    """(Q, P): the block's pair and narrow prefixes in 256-entry supergroups (k_pair_cost,
    k_narrow_cost, k_narrow_split with their default weights)."""
    N = len(col)
    ng = (N + 255) >> 8
    cnt = np.minimum(256, N - 256 * np.arange(ng))
    Q = 0
    if pairs:
        p = col >> 1
        new = run_starts(p)
        pos = np.arange(N)
        start = np.maximum.accumulate(np.where(new, pos, 0))
        lead = ((pos - start) & 1) == 0
        nxt_same = np.zeros(N, dtype=bool)
        nxt_same[:-1] = ~new[1:]
        half = lead & ~nxt_same
        step = np.zeros(N, dtype=np.int64)
        step[1:] = np.where(new[1:], p[1:] - p[:-1], 0)
        sf = np.where(step > 3, (step + 2) // 3 - 1, 0)
        nf = np.bincount(pos >> 8, weights=half + 2 * sf, minlength=ng).astype(np.int64)
        Q = prefix_split(4 * cnt - PAIR_FILL_COST * nf)
    P = Q
    if narrow:
        zq = Q << 8
        step = np.zeros(N, dtype=np.int64)
        step[zq + 1:] = col[zq + 1:] - col[zq:-1]
        fl = np.where(step > 3, (step + 2) // 3 - 1, 0)
        D = np.bincount(np.arange(N) >> 8, weights=fl, minlength=ng).astype(np.int64)
        P = Q + prefix_split((4 * cnt - 4 * D)[Q:])
    return Q, P


def deal_piece(rows):
    """gx_pr_bank.h bank_deal_pos on one piece: the indices of its entries in dealt order."""
    rows = np.asarray(rows, dtype=np.int64)
    cls = rows & 15
    t = np.zeros(len(rows), dtype=np.int64)
    for b in range(16):
        m = cls == b
        t[m] = np.arange(int(m.sum()))
    return np.lexsort((cls, t))


def bank_order(col, row, Q, P, tile=2048):
    """The block's (col, row) after k_bank_order: in the pair prefix [0, 256 Q) pieces of one column
    pair, in the narrow prefix [256 Q, 256 P) pieces of one column, each inside a tile of `tile`
    entries (kBankTile; 0 = whole runs, the limit of larger tiles)."""
    N = len(col)
    Nq, Np = min(N, Q << 8), min(N, P << 8)
    col, row = col.copy(), row.copy()
    if Np == 0:
        return col, row
    i = np.arange(Np)
    key = np.where(i < Nq, col[:Np] >> 1, col[:Np])
    head = run_starts(key) | ((i % tile == 0) if tile else (i == Nq))
    piece = np.cumsum(head) - 1
    first = np.flatnonzero(head)
    length = np.diff(np.append(first, Np))
    cls = row[:Np] & 15
    g = piece * 16 + cls
    o = np.argsort(g, kind="stable")
    gs = g[o]
    gstart = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]])
    glen = np.diff(np.append(gstart, Np))
    t = np.empty(Np, dtype=np.int64)
    t[o] = np.arange(Np) - np.repeat(gstart, glen)
    # position in the deal: entries ordered by (t, class) inside the piece
    o2 = np.lexsort((cls, t, piece))
    k = np.empty(Np, dtype=np.int64)
    k[o2] = np.arange(Np) - np.repeat(first, length)
    n = np.repeat(length, length)
    h = (n + 1) // 2
    off = np.where(i < Nq, np.where(k < h, 2 * k, 2 * (k - h) + 1), k)
    dst = np.repeat(first, length) + off
    col[dst], row[dst] = col[:Np].copy(), row[:Np].copy()
    return col, row


def pair_slots(col, row, Q):
    """(rowA, rowB) of the slots of the pair prefix in slot order (gather_pairs decode: slot e of a
    256-slot supergroup sits in lane e mod 64 of instruction e / 64), padded to whole supergroups."""
    Nq = min(len(col), Q << 8)
    if Nq == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z
    p = col[:Nq] >> 1
    new = run_starts(p)
    pos = np.arange(Nq)
    start = np.maximum.accumulate(np.where(new, pos, 0))
    lead = ((pos - start) & 1) == 0
    step = np.zeros(Nq, dtype=np.int64)
    step[1:] = np.where(new[1:], p[1:] - p[:-1], 0)
    sf = np.where(step > 3, (step + 2) // 3 - 1, 0)
    nslot = lead.astype(np.int64) + sf
    at = np.cumsum(nslot) - 1            # a lead entry's slot (its fillers come before it)
    total = int(nslot.sum())
    padded = (total + 255) // 256 * 256
    junk = JUNK + (np.arange(padded) & 63)
    ra, rb = junk.copy(), junk.copy()
    li = np.flatnonzero(lead)
    ra[at[li]] = row[li]
    has = np.zeros(len(li), dtype=bool)
    ok = li + 1 < Nq
    has[ok] = ~new[li[ok] + 1]
    rb[at[li[has]]] = row[li[has] + 1]
    return ra, rb


def narrow_codes(col, row, Q, P):
    """The rows of the narrow codes in code order (gather_narrow decode: code e of a 512-code
    supergroup sits in lane e mod 64 of instruction e / 64), padded to whole supergroups."""
    N = len(col)
    zq, zp = min(N, Q << 8), min(N, P << 8)
    if zp <= zq:
        return np.zeros(0, dtype=np.int64)
    c = col[zq:zp]
    step = np.zeros(len(c), dtype=np.int64)
    step[1:] = c[1:] - c[:-1]
    fl = np.where(step > 3, (step + 2) // 3 - 1, 0)
    at = np.cumsum(fl + 1) - 1
    total = int(at[-1]) + 1
    padded = (total + 511) // 512 * 512
    out = JUNK + (np.arange(padded) & 63)
    out[at] = row[zq:zp]
    return out


def laneperm(row):
    """k_sorted_laneperm on the wide part: every full 64-entry group ranked by (row mod 16, bit 4 of
    the row, position), entry k of that order to position 4 (k / 4) + k mod 4 -- the order itself."""
    row = row.copy()
    nfull = len(row) // 64 * 64
    if nfull:
        g = row[:nfull].reshape(-1, 64)
        key = ((g & 15) << 1) | ((g >> 4) & 1)
        o = np.argsort(key, axis=1, kind="stable")
        row[:nfull] = np.take_along_axis(g, o, axis=1).reshape(-1)
    return row


def wide_groups(row):
    """The 16-lane groups of the wide X4 rounds: lane l of a 256-entry supergroup holds entries
    4 l .. 4 l + 3, instruction j adds entry 4 l + j, so a group is positions 4 s + j (s < 16) of
    one 64-entry group.  The tail is padded with junk rows."""
    n = len(row)
    if n == 0:
        return np.zeros((0, 16), dtype=np.int64)
    padded = (n + 63) // 64 * 64
    r = np.concatenate([row, JUNK + (np.arange(padded - n) & 63)])
    return r.reshape(-1, 16, 4).transpose(0, 2, 1).reshape(-1, 16)


def group_cycles(groups, combine=False):
    """LDS-array cycles of 16-lane groups (one row of `groups` each): the fullest slot's rows,
    equal rows counted once when `combine`."""
    if len(groups) == 0:
        return 0
    g = np.sort(groups, axis=1)
    keep = np.ones(g.shape, dtype=bool)
    if combine:
        keep[:, 1:] = g[:, 1:] != g[:, :-1]
    cls = np.where(keep, g & 15, -1).astype(np.int8)
    worst = np.zeros(len(g), dtype=np.int64)
    for c in range(16):
        worst = np.maximum(worst, (cls == c).sum(axis=1))
    return int(worst.sum())


def block_cycles(col, row, Q, P, combine=False):
    """{region: (groups, cycles)} of one block's launch in the given order."""
    ra, rb = pair_slots(col, row, Q)
    nc = narrow_codes(col, row, Q, P)
    wide = wide_groups(laneperm(row[min(len(row), P << 8):]))
    out = {}
    out["pair"] = (2 * (len(ra) // 16), group_cycles(ra.reshape(-1, 16), combine) + group_cycles(rb.reshape(-1, 16), combine))
    out["narrow"] = (len(nc) // 16, group_cycles(nc.reshape(-1, 16), combine))
    out["wide"] = (len(wide), group_cycles(wide, combine))
    return out


def run_shares(col, Q, P):
    """{region: (entries, in runs >= 16, in runs >= 64)}: runs of one column pair in the pair
    prefix, of one column elsewhere."""
    N = len(col)
    zq, zp = min(N, Q << 8), min(N, P << 8)
    out = {}
    for name, key in (("pair", col[:zq] >> 1), ("narrow", col[zq:zp]), ("wide", col[zp:])):
        if len(key) == 0:
            out[name] = (0, 0, 0)
            continue
        first = np.flatnonzero(run_starts(key))
        length = np.diff(np.append(first, len(key)))
        out[name] = (len(key), int(length[length >= 16].sum()), int(length[length >= 64].sum()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("graph", nargs="*", type=int, default=[23, 40, 85])
    ap.add_argument("--rows", type=int, default=16320)
    ap.add_argument("--block", type=int, default=32 << 20)
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--combine", action="store_true", help="equal rows of a group take one cycle")
    ap.add_argument("--tile", type=int, default=2048, help="entries dealt together (kBankTile; 0: whole runs)")
    a = ap.parse_args()
    scale, ef, seed = a.graph[:3]
    t0 = time.time()
    csr = rmat(scale, ef, seed)
    print(f"R-MAT {scale}/{ef}/{seed}: n {csr.n} nnz {csr.nnz}; blocks of <= {a.rows} rows, <= {a.block} entries; "
          f"every {a.every}. block with entries modelled, tiles of {a.tile} entries ({time.time() - t0:.0f} s)", flush=True)
    regions = ("pair", "narrow", "wide")
    classes = ("entry-limited", "row-limited")
    tot = {(c, r): np.zeros(6, dtype=np.int64) for c in classes for r in regions}   # groups, now, new, entries, >=16, >=64
    nb = 0
    for b, (nrows, col, row) in enumerate(block_entries(csr, a.rows, a.block)):
        if b % a.every:
            continue
        nb += 1
        cls = "row-limited" if nrows == a.rows else "entry-limited"
        Q, P = splits(col)
        now = block_cycles(col, row, Q, P, a.combine)
        c2, r2 = bank_order(col, row, Q, P, a.tile)
        new = block_cycles(c2, r2, Q, P, a.combine)
        sh = run_shares(col, Q, P)
        for r in regions:
            tot[(cls, r)] += np.array([now[r][0], now[r][1], new[r][1], *sh[r]])
    print(f"{nb} blocks ({time.time() - t0:.0f} s).  LDS-array cycles per launch (all CUs), one per conflict-free 16-lane group:")
    print(f"{'block class':14s} {'region':7s} {'entries':>12s} {'runs>=16':>9s} {'runs>=64':>9s} {'groups':>12s} {'present':>12s} "
          f"{'bank order':>12s} {'conflict cycles':>24s}")
    allr = np.zeros(6, dtype=np.int64)
    for c in classes:
        for r in regions:
            g, now, new, e, e16, e64 = tot[(c, r)]
            allr += tot[(c, r)]
            if g == 0:
                continue
            print(f"{c:14s} {r:7s} {e:12d} {e16 / max(e, 1):9.3f} {e64 / max(e, 1):9.3f} {g:12d} {now:12d} {new:12d} "
                  f"{now - g:11d} -> {new - g:9d}")
    g, now, new, e, e16, e64 = allr
    print(f"{'all':14s} {'':7s} {e:12d} {e16 / max(e, 1):9.3f} {e64 / max(e, 1):9.3f} {g:12d} {now:12d} {new:12d} "
          f"{now - g:11d} -> {new - g:9d}")
    print(f"conflict cycles x {(new - g) / max(now - g, 1):.3f}; LDS-array cycles x {new / max(now, 1):.3f}; "
          f"conflict-free bound x {g / max(now, 1):.3f}")


if __name__ == "__main__":
    main()
