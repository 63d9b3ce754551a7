"""Op-level GraphBLAS ABI (gx_mxv / gx_vxm / gx_mxm_masked) at the shapes where csrc/gx_ops.hip branches.

The device pulls over the rows of M (A or A'): a thread per row up to 64 entries, longer rows cut into
2048-entry segments, one wave each, joined by the monoid's atomic.  tests/test_ops.py never has a row
above 2048 entries on that path, so there every atomic meets the identity.  This module does.

Reference.  `Product` / `finish` restate the op-level section of include/gx.h in vectorised numpy on
the CSR arrays (reduceat per row); they share no code with oracle/gx_oracle.c or test_ops.numpy_mxv.
The CPU tests pin the C oracle (orc_mxv, orc_mxm_masked) to that restatement on the same cases first;
the GPU tests then compare the device with the numpy reference.

Covered
  row lengths   star centres with out-rows AND in-rows of exactly 0, 1, 63, 64, 65, 2047, 2048, 2049, 4096,
                4097 and 5000 entries (asserted on the CPU) over a sparse background, n = 7001; directed and
                weighted (U(0,1] plus exact 0.0 and 1e300), and undirected unweighted (A' = A, where mxv
                with T0 runs the PageRank kernel); an edgeless graph; n = 1 with a self-loop; for
                MIN_SECONDI a copy whose rows run in descending column order (the smallest index sits in
                the last, partial segment while every segment has terms).
  descriptors   mxv and vxm, with and without T0; mask None x {0, ACCUM}; a random mask x all eight
                combinations of MASK_COMP, REPLACE, ACCUM; each once with a random w_present and once with
                w_present = None (every old entry present, nothing written back).
  u presence    None / random 60 % (the one-entry last segments kept) / nothing present / only the last
                segment of every multi-segment row / one long row without a present entry / segment 0 of the
                longest row absent; cycled over the cases.  u = None (or an array of nothing but poison)
                where the header allows it.
  poison        absent u entries and absent old w entries hold NaN (fp64), 0 (MIN over uint64), INT64_MIN
                (MIN over int64), 2^64-1 / -1 / 1 otherwise: the result must not depend on them.
  value edges   MIN_SECOND mxv: u over the whole uint64 range with 2^63-1, 2^63 and 2^64-2; MIN_SECOND vxm:
                the crafted weights, test_ops.odd_weights (negative, NaN, >= 2^64, fractional) and weights
                spread over 2^50 (so that segments have different minima); MIN_PLUS: present +inf in u (a
                present +inf result where it is the only term) and DBL_MAX + 1e300 overflowing to +inf;
                PLUS_PAIR / MIN_SECONDI ACCUM into negative w and w near +-2^62; PLUS_SECOND with u in [0,1)
                and in (-1,1).
  combine       asserted on the reference before any device call: with u_present None or random every
                multi-segment row has terms in at least two segments, and for each MIN semiring some such
                row has its minimum outside segment 0 and some has it only in the last, partial segment.
  comparison    presence bit-exact; values over the WHOLE array (kept entries, identity at absent ones)
                bit-exact for every semiring but PLUS_SECOND.
  PLUS_SECOND   reference = math.fsum per row (correctly rounded).  Any order of m correctly rounded adds is
                within (m-1) 2^-53 sum|term| of the exact sum (first order), so |got - fsum| <=
                len_i 2^-53 sum_j |term_ij| with len_i the row length of M, rtol 0; one more than m-1 for the
                PageRank epilogue's add on the T0 path.  With ACCUM the old w(i) is one more term of the same
                sum: reference fsum(terms + [w]), bound (len_i + 1) 2^-53 (sum|term| + |w|).
  mxm_masked    self-loops, empty rows, shuffled rows, one row above 1000 entries, directed and undirected,
                n = 1 with a self-loop, n = 2, nnz = 0, against the dense S @ S.T read at A's entries.
  errors/state  unknown semiring, NULL u, unsupported mxm arguments, each followed by a good call; PageRank
                and mxv(PLUS_SECOND, T0) alternating on one graph (the op borrows the cached plan): repeated
                results bit-identical on the deterministic CSR-Adaptive kernel, within their bounds on both.

Not covered (on purpose)
  NaN inputs to the MIN semirings (min with NaN depends on the order of the terms); MASK_COMP with a NULL
  mask (the header does not define it); gx_part_* and the multi-device drivers; sizes beyond these graphs
  (test_ops.test_gpu_pr_mxv_on_large_graph is the workload-sized case); any check of generated code.
"""
import functools
import math

import numpy as np
import pytest

from oracle import oracle as O
from test_ops import odd_weights, sat_u64
from ldbc_graphalytics_platforms_graphblas_amd.graphio import CSR, csr_from_edges

PS, MS, AP, MP, PP, SI = range(6)   # include/gx.h GX_PLUS_SECOND_FP64 .. GX_MIN_SECONDI_INT64
NAMES = {PS: "PLUS_SECOND_FP64", MS: "MIN_SECOND_UINT64", AP: "ANY_PAIR_BOOL", MP: "MIN_PLUS_FP64",
         PP: "PLUS_PAIR_INT64", SI: "MIN_SECONDI_INT64"}
T0, COMP, REPLACE, ACCUM = 1, 2, 4, 8
GX_NULL_POINTER, GX_INVALID_VALUE, GX_NOT_IMPLEMENTED = -2, -3, -101
SEG = 2048                          # gx_ops.hip kSegNnz (kShortDeg = 64: LENGTHS straddles both)
LENGTHS = (0, 1, 63, 64, 65, 2047, 2048, 2049, 4096, 4097, 5000)
EPS = 2.0 ** -53
U64MAX = np.uint64(2 ** 64 - 1)
I64 = np.iinfo(np.int64)
DTYPE = {PS: np.float64, MS: np.uint64, AP: np.uint8, MP: np.float64, PP: np.int64, SI: np.int64}
IDENT = {PS: 0.0, MS: U64MAX, AP: 0, MP: np.inf, PP: 0, SI: I64.max}
MIN_SR = (MS, MP, SI)
# what an absent entry holds in the inputs: the value that would do most damage if it were read
POISON = {PS: np.nan, MS: np.uint64(0), AP: 1, MP: np.nan, PP: -1, SI: I64.min}
READS_U = {(PS, False), (MS, False), (MP, False), (MP, True)}   # (semiring, vxm); the others allow u = NULL


# ------------------------------------------------------------------------------------ graphs

def _star(rng, length, lo, split, hi):
    """`length` distinct leaves in [lo, hi).  A multi-segment star takes exactly its last segment's leaves
    from [split, hi) and the others below, so that in the sorted row the last segment is those leaves."""
    if length <= SEG:
        return rng.choice(np.arange(lo, hi), length, replace=False)
    tail = length - (-(-length // SEG) - 1) * SEG
    return np.concatenate([rng.choice(np.arange(lo, split), length - tail, replace=False),
                           rng.choice(np.arange(split, hi), tail, replace=False)])


def _crafted(directed):
    """Star centres (they take no other edge) with the LENGTHS as out-rows (vertices 0..10) and, when
    directed, as in-rows (11..21), over a sparse random background."""
    rng = np.random.default_rng(2049)
    n, k = 7001, len(LENGTHS)
    first = 2 * k if directed else k
    split = n - SEG
    src, dst = [], []
    for c, length in enumerate(LENGTHS):
        src.append(np.full(length, c, np.int64))
        dst.append(_star(rng, length, first, split, n))
        if directed:
            src.append(_star(rng, length, first, split, n))
            dst.append(np.full(length, k + c, np.int64))
    m = 8000 if directed else 4000
    bs, bd = rng.integers(first, n, m), rng.integers(first, n, m)
    src.append(bs[bs != bd])
    dst.append(bd[bs != bd])
    s, d = np.concatenate(src), np.concatenate(dst)
    w = None
    if directed:
        w = 1.0 - rng.random(len(s))                       # U(0, 1]
        w[rng.choice(len(s), 40, replace=False)] = 0.0
        w[rng.choice(len(s), 40, replace=False)] = 1e300
    return csr_from_edges(n, s, d, w, symmetric=not directed)


def _with_vals(csr, vals):
    return CSR(csr.n, csr.rowptr, csr.colidx, vals)


def _wide(name):
    """Integer weights spread over 2^50, the smallest (1) planted in the last segment of the longest row
    of A and of A', so that MIN_SECOND vxm has a minimum that only one segment holds."""
    csr = graph(name)
    with np.errstate(over="ignore"):
        vals = np.floor(csr.vals * 2.0 ** 50) + 2.0          # 1e300 goes to +inf, which saturates
    for use_t in (False, True):
        rp, _, _, _, perm = pull(name, use_t)
        i = int(np.argmax(np.diff(rp)))
        vals[perm[max(rp[i], rp[i + 1] - 7)]] = 1.0
    return _with_vals(csr, vals)


def _reversed_rows(csr):
    rp = csr.rowptr.astype(np.int64)
    rows = np.repeat(np.arange(csr.n), np.diff(rp))
    back = rp[rows] + rp[rows + 1] - 1 - np.arange(csr.nnz)
    return CSR(csr.n, csr.rowptr, csr.colidx[back].copy(), None if csr.vals is None else csr.vals[back].copy())


def _shuffled_rows(csr, seed):
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(csr.n), np.diff(csr.rowptr.astype(np.int64)))
    order = np.lexsort((rng.random(csr.nnz), rows))
    return CSR(csr.n, csr.rowptr, csr.colidx[order].copy(), None if csr.vals is None else csr.vals[order].copy())


def _mxm_graph(directed):
    """Self-loops, empty rows, one row above 1000 entries against many short ones, shuffled rows."""
    rng = np.random.default_rng(1100 + directed)
    n = 1201 if directed else 1500
    s = np.concatenate([np.zeros(1100, np.int64), rng.integers(1, n - 20, 3000), np.arange(0, n - 20, 23)])
    d = np.concatenate([rng.choice(np.arange(1, n - 20), 1100, replace=False), rng.integers(1, n - 20, 3000),
                        np.arange(0, n - 20, 23)])
    return _shuffled_rows(csr_from_edges(n, s, d, None, symmetric=not directed), 5)


def _edges(n, pairs, w=None, symmetric=False):
    e = np.array(pairs, np.int64).reshape(-1, 2)
    return csr_from_edges(n, e[:, 0], e[:, 1], w, symmetric=symmetric)


BUILDERS = {
    "dw": lambda: _crafted(True),
    "uu": lambda: _crafted(False),
    "dw-odd": lambda: odd_weights(graph("dw")),
    "dw-wide": lambda: _wide("dw"),
    "dw-rev": lambda: _reversed_rows(graph("dw")),
    "empty": lambda: _edges(37, []),
    "one": lambda: _edges(1, [(0, 0)], np.array([0.5])),
    "mxm-directed": lambda: _mxm_graph(True),
    "mxm-undirected": lambda: _mxm_graph(False),
    "mxm-one": lambda: _edges(1, [(0, 0)]),
    "mxm-two": lambda: _edges(2, [(0, 1), (1, 1), (1, 0)]),
    "mxm-empty": lambda: _edges(5, []),
}
DIRECTED = {"dw": True, "uu": False, "dw-odd": True, "dw-wide": True, "dw-rev": True, "empty": False, "one": True,
            "mxm-directed": True, "mxm-undirected": False, "mxm-one": True, "mxm-two": True, "mxm-empty": False}
MXM_GRAPHS = [k for k in BUILDERS if k.startswith("mxm-")]


@functools.lru_cache(maxsize=None)
def graph(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def pull(name, use_t):
    """The rows the op pulls over: (rowptr, row, column, value, position in A) per entry of M = A, or of
    A' with its rows in ascending source order (the device builds A' by a full key sort)."""
    csr = graph(name)
    rp = csr.rowptr.astype(np.int64)
    ci = csr.colidx.astype(np.int64)
    rows = np.repeat(np.arange(csr.n), np.diff(rp))
    perm = np.arange(len(ci))
    if use_t:
        perm = np.lexsort((rows, ci))
        rp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=csr.n))]).astype(np.int64)
        rows, ci = ci[perm], rows[perm]
    vals = None if csr.vals is None else csr.vals[perm]
    return rp, rows, ci, vals, perm


# ------------------------------------------------------------------------------------ reference

def cast_u64(a):
    """GraphBLAS's fp64 -> uint64 typecast, the rule of test_ops.sat_u64, on an array."""
    a = np.asarray(a, np.float64)
    out = np.zeros(a.shape, np.uint64)
    big = a >= 2.0 ** 64
    high = (a >= 2.0 ** 63) & ~big
    low = (a > 0.0) & (a < 2.0 ** 63)
    out[low] = a[low].astype(np.int64).astype(np.uint64)
    out[high] = (a[high] - 2.0 ** 63).astype(np.int64).astype(np.uint64) + np.uint64(2 ** 63)
    out[big] = U64MAX
    return out


class Product:
    """t = M (+).(x) u without mask or accumulator: values (identity where absent), presence, and for
    PLUS_SECOND the kept terms per row (for fsum with one more term, and for the bound)."""

    def __init__(self, name, sr, u, up, vxm, t0):
        rp, rows, cols, vals, _ = pull(name, bool(vxm) != bool(t0))
        n = len(rp) - 1
        keep = np.ones(len(cols), bool) if up is None else up[cols] != 0
        r, c = rows[keep], cols[keep]
        a = np.ones(len(c)) if vals is None else vals[keep]
        if sr == PS:
            term = a if vxm else u[c]
        elif sr == MS:
            term = cast_u64(a) if vxm else u[c]
        elif sr == MP:
            with np.errstate(over="ignore"):
                term = u[c] + a
            self.overflow = bool((np.isinf(term) & np.isfinite(u[c])).any())
        elif sr == SI:
            term = c
        else:
            term = np.ones(len(c), np.int64)
        cnt = np.bincount(r, minlength=n)
        self.hit = cnt > 0
        self.start = (np.cumsum(cnt) - cnt)[self.hit]
        self.cnt = cnt[self.hit]
        self.term, self.row_len = term, np.diff(rp)
        self.seg = ((np.arange(len(cols)) - rp[rows]) // SEG)[keep]   # the device's segment of each kept entry
        self.rows = r
        self.t = np.full(n, IDENT[sr], DTYPE[sr])
        self.abs_sum = np.zeros(n)
        if not len(c):
            return
        if sr in MIN_SR:
            self.t[self.hit] = np.minimum.reduceat(term, self.start)
        elif sr == PP:
            self.t[self.hit] = np.add.reduceat(term, self.start)
        elif sr == AP:
            self.t[self.hit] = 1
        else:
            self.abs_sum[self.hit] = np.add.reduceat(np.abs(term), self.start)
            self.t[self.hit] = self.fsum_rows(np.nonzero(self.hit)[0])

    def fsum_rows(self, rows, extra=None):
        """math.fsum of each given (present) row's terms, plus extra[i] as one more term."""
        where = np.cumsum(self.hit) - 1
        out = np.empty(len(rows))
        for o, i in enumerate(rows):
            s = self.start[where[i]]
            terms = self.term[s:s + self.cnt[where[i]]].tolist()
            if extra is not None:
                terms.append(float(extra[i]))
            out[o] = math.fsum(terms)
        return out

    def multi_rows(self):
        """Per row of M above SEG entries: (row, length, segments with a kept term, segments holding the
        row's minimum term)."""
        out = []
        for i in np.nonzero(self.row_len > SEG)[0]:
            sel = self.rows == i
            seg, term = self.seg[sel], self.term[sel]
            at_min = set(seg[term == term.min()].tolist()) if len(term) else set()
            out.append((int(i), int(self.row_len[i]), set(seg.tolist()), at_min))
        return out


def combine(sr, a, b):
    if sr in (PS, PP):
        return a + b
    if sr == AP:
        return ((a != 0) | (b != 0)).astype(np.uint8)
    return np.minimum(a, b)


def finish(sr, t, hit, mask, desc, w, w_present):
    """w<mask> = t, or w (+)= t with ACCUM, as include/gx.h states it.  w_present None: every old entry is
    present and no presence is returned.  Entries that end absent hold the monoid identity; masked-out
    entries are kept as they are (cleared with REPLACE)."""
    n = len(t)
    allowed = np.ones(n, bool) if mask is None else (mask != 0) != bool(desc & COMP)
    old = np.ones(n, bool) if w_present is None else w_present != 0
    out, present = np.array(w, copy=True), old.copy()
    acc = allowed & old if desc & ACCUM else np.zeros(n, bool)
    put = allowed & ~acc
    out[put] = t[put]                        # the identity where t is absent
    present[put] = hit[put]
    both = acc & hit                         # old entries without a new term are kept, and present
    out[both] = combine(sr, w[both], t[both])
    if desc & REPLACE:
        out[~allowed] = IDENT[sr]
        present[~allowed] = False
    return out, (None if w_present is None else present.astype(np.uint8)), put, both


# ------------------------------------------------------------------------------------ cases

def u_patterns(name, use_t, rng):
    """(label, u_present) over the rows the case pulls: see the module docstring."""
    rp, rows, cols, _, _ = pull(name, use_t)
    n = len(rp) - 1
    rnd = lambda: (rng.random(n) < 0.6).astype(np.uint8)
    pats = [("all", None), ("random", rnd()), ("none", np.zeros(n, np.uint8))]
    length = np.diff(rp)
    multi = np.nonzero(length > SEG)[0]
    if not len(multi):
        return pats
    nseg = -(-length // SEG)
    in_last = (np.arange(len(cols)) - rp[rows]) // SEG == nseg[rows] - 1
    big = length[rows] > SEG
    pats[1][1][cols[rp[multi + 1] - 1]] = 1     # 2049 and 4097: the last segment is one entry; keep it
    last = np.zeros(n, np.uint8)
    last[cols[big & in_last]] = 1
    last[cols[big & ~in_last]] = 0
    pats.append(("last-segment", last))
    hole = rnd()
    hole[cols[rp[multi[0]]:rp[multi[0] + 1]]] = 0
    pats.append(("empty-long-row", hole))
    i = int(np.argmax(length))
    tail = rnd()
    tail[cols[rp[i] + SEG:rp[i + 1]]] = 1
    tail[cols[rp[i]:rp[i] + SEG]] = 0
    pats.append(("no-segment-0", tail))
    return pats


def planted(name):
    """A vertex in the last segment of the longest row of A, and one of A'."""
    out = []
    for use_t in (False, True):
        rp, _, cols, _, _ = pull(name, use_t)
        if len(cols):
            i = int(np.argmax(np.diff(rp)))
            out.append(int(cols[max(rp[i], rp[i + 1] - 7)]))
    return out


def draw_u(name, sr, vxm, rng, signed):
    csr = graph(name)
    n = csr.n
    if (sr, vxm) not in READS_U:
        return None
    if sr == PS:
        return rng.uniform(-1.0, 1.0, n) if signed else rng.random(n)
    if sr == MS:
        u = rng.integers(2, 2 ** 64 - 1, n, dtype=np.uint64)
        edges = np.array([2 ** 63 - 1, 2 ** 63, 2 ** 64 - 2], np.uint64)[:n]
        u[rng.choice(n, len(edges), replace=False)] = edges
        u[planted(name)] = 1
        return u
    u = rng.random(n) * 10.0                                  # MIN_PLUS
    u[rng.random(n) < 0.02] = np.inf
    rp, rows, cols, vals, _ = pull(name, False)
    for i in np.nonzero(np.diff(rp) == 1)[0][:4]:              # a present +inf as a row's only term
        u[cols[rp[i]]] = np.inf
    rpt, _, colst, _, _ = pull(name, True)
    for i in np.nonzero(np.diff(rpt) == 1)[0][:4]:
        u[colst[rpt[i]]] = np.inf
    if vals is not None:                                       # DBL_MAX + 1e300 overflows
        huge = np.nonzero(vals == 1e300)[0][:6]
        u[cols[huge[:3]]] = np.finfo(np.float64).max
        u[rows[huge[3:]]] = np.finfo(np.float64).max
    u[planted(name)] = -5.0
    return u


def draw_w(sr, n, rng):
    if sr == PS:
        return rng.uniform(-1.0, 1.0, n)
    if sr == MS:
        return rng.integers(0, 2 ** 64 - 1, n, dtype=np.uint64, endpoint=True)
    if sr == AP:
        return rng.integers(0, 2, n).astype(np.uint8)
    if sr == MP:
        w = rng.random(n) * 10.0 - 3.0
        w[rng.random(n) < 0.05] = np.inf
        return w
    w = rng.integers(-100, n + 100, n)
    far = rng.random(n) < 0.2
    w[far] = rng.choice(np.array([-2 ** 62, -2 ** 62 + 3, 2 ** 62, 2 ** 62 - 5, -7, I64.min + 9000]), int(far.sum()))
    return w.astype(np.int64)


MASK_DESCS = [(False, 0), (False, ACCUM)] + [(True, b) for b in (0, COMP, REPLACE, ACCUM, COMP | REPLACE,
                                                                 COMP | ACCUM, REPLACE | ACCUM, COMP | REPLACE | ACCUM)]


def op_cases(name, sr, orientations=((False, False), (False, True), (True, False), (True, True)), seed=0,
             signed=False, patterns=None):
    """Every case of one semiring on one graph, with the numpy reference's answer."""
    n = graph(name).n
    rng = np.random.default_rng(1000 * sr + seed)
    k = 0
    for vxm, t0 in orientations:
        use_t = vxm != t0
        pats = u_patterns(name, use_t, rng)
        if patterns:
            pats = [p for p in pats if p[0] in patterns]
        u0 = draw_u(name, sr, vxm, rng, signed)
        products = {}
        for with_mask, bits in MASK_DESCS:
            for wp_given in (True, False):
                label, up = pats[k % len(pats)]
                if u0 is None:    # the header allows NULL; an array of poison must do as well
                    u = None if k % 2 else np.full(n, POISON[sr], np.uint64 if sr == AP else DTYPE[sr])
                else:
                    u = u0.copy()
                    if up is not None:
                        u[up == 0] = POISON[sr]
                if label not in products:
                    products[label] = Product(name, sr, u0, up, vxm, t0)
                prod = products[label]
                desc = bits | (T0 if t0 else 0)
                mask = (rng.random(n) < 0.5).astype(np.uint8) if with_mask else None
                w = draw_w(sr, n, rng)
                wp = (rng.random(n) < 0.5).astype(np.uint8) if wp_given else None
                if wp is not None:
                    w[wp == 0] = POISON[sr]
                want, wantp, put, both = finish(sr, prod.t, prod.hit, mask, bits, w, wp)
                atol = None
                if sr == PS:
                    idx = np.nonzero(both)[0]
                    want[idx] = prod.fsum_rows(idx, extra=w)
                    atol = np.zeros(n)
                    atol[put] = (prod.row_len * EPS * prod.abs_sum)[put]
                    atol[both] = ((prod.row_len + 1) * EPS * (prod.abs_sum + np.abs(w)))[both]
                yield dict(name=name, sr=sr, vxm=vxm, desc=desc, mask=mask, u=u, up=up, w=w, wp=wp, want=want,
                           wantp=wantp, atol=atol, prod=prod, pattern=label,
                           what=f"{name} {NAMES[sr]} {'vxm' if vxm else 'mxv'} desc={desc} mask={with_mask} "
                                f"u_present={label} u={'NULL' if u is None else 'given'} "
                                f"w_present={'given' if wp_given else 'NULL'}")
                k += 1


M_IS_A = ((False, False), (True, True))   # mxv, and vxm with T0, pull over A itself


def family_cases(sr, family):
    """The cases of one semiring: on the directed weighted crafted graph with its value-edge variants, or on
    the undirected unweighted one."""
    if family == "undirected":
        return list(op_cases("uu", sr))
    cases = list(op_cases("dw", sr))
    if sr == PS:
        cases += list(op_cases("dw", sr, orientations=((False, False), (False, True)), seed=1, signed=True))
    if sr == MS:
        cases += list(op_cases("dw-odd", sr, orientations=((True, False), (True, True)), seed=2))
        cases += list(op_cases("dw-wide", sr, orientations=((True, False), (True, True)), seed=3))
    if sr == SI:
        cases += list(op_cases("dw-rev", sr, orientations=M_IS_A, seed=4, patterns=("all", "random")))
    return cases


def assert_combine_observable(sr, cases, minima):
    """Every multi-segment row has terms in two segments or more when u_present is None or random; and, for
    a MIN semiring on the directed family, for mxv and for vxm: some such row has its minimum outside
    segment 0, and some has it only in its last, partial segment."""
    seen = {(v, k): False for v in (False, True) for k in ("outside-0", "last-partial")}
    n_multi = 0
    for c in cases:
        for row, length, segs, at_min in c["prod"].multi_rows():
            if c["pattern"] in ("all", "random"):
                n_multi += 1
                assert len(segs) >= 2, f"row {row} of {c['what']} has terms in segments {segs} only"
            if sr in MIN_SR and len(segs) >= 2:
                last = -(-length // SEG) - 1
                seen[c["vxm"], "outside-0"] |= 0 not in at_min
                seen[c["vxm"], "last-partial"] |= at_min == {last} and length % SEG != 0
    assert n_multi > 0
    if sr in MIN_SR and minima:
        assert all(seen.values()), f"{NAMES[sr]}: minimum placement not covered: {seen}"


def compare(c, got, gotp, worst=None):
    assert got.dtype == DTYPE[c["sr"]]
    if c["wantp"] is None:
        assert gotp is None
    else:
        np.testing.assert_array_equal(gotp, c["wantp"], err_msg="presence: " + c["what"])
    want = c["want"]
    if c["sr"] != PS:
        np.testing.assert_array_equal(got, want, err_msg=c["what"])   # NaN (kept poison) equals NaN
        return
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=c["what"])
    err = np.abs(got[~nan] - want[~nan])
    atol = c["atol"][~nan]
    if worst is not None and (atol > 0).any():
        worst.append(float(np.max(err[atol > 0] / atol[atol > 0])))
    bad = np.nonzero(err > atol)[0]
    assert not len(bad), (f"{c['what']}: {len(bad)} entries beyond len * 2^-53 * sum|term|; worst error/bound "
                          f"{np.max(err[bad] / np.maximum(atol[bad], 1e-300)):.3g}")


def dense_mxm(csr):
    """C<A> = A A' with PLUS_PAIR: the dense 0/1 product (exact in fp64 at these sizes) at A's entries."""
    rows = np.repeat(np.arange(csr.n), np.diff(csr.rowptr.astype(np.int64)))
    cols = csr.colidx.astype(np.int64)
    S = np.zeros((csr.n, csr.n))
    S[rows, cols] = 1.0
    return (S @ S.T)[rows, cols].astype(np.int64)


# ------------------------------------------------------------------------------------ CPU

def test_crafted_graphs_have_the_row_lengths():
    for name in ("dw", "uu"):
        csr = graph(name)
        out_len = np.diff(pull(name, False)[0])
        in_len = np.diff(pull(name, True)[0])
        assert csr.n == 7001 and csr.n & (csr.n - 1) and csr.nnz < 60000
        assert set(LENGTHS) <= set(out_len.tolist()) and set(LENGTHS) <= set(in_len.tolist())
        k = len(LENGTHS)
        np.testing.assert_array_equal(out_len[:k], LENGTHS)        # the out-star centres...
        if name == "dw":
            assert not in_len[:k].any()                            # ...take no other edge
            np.testing.assert_array_equal(in_len[k:2 * k], LENGTHS)
            assert not out_len[k:2 * k].any()
            assert (csr.vals == 0.0).sum() >= 3 and (csr.vals == 1e300).sum() >= 3
            assert ((csr.vals > 0) & (csr.vals <= 1.0)).sum() > csr.nnz - 100
            rows = np.repeat(np.arange(csr.n), out_len)
            assert not np.array_equal(np.sort(rows * csr.n + csr.colidx.astype(np.int64)),
                                      np.sort(csr.colidx.astype(np.int64) * csr.n + rows))   # A' != A
        else:
            assert csr.vals is None
            np.testing.assert_array_equal(out_len, in_len)
            t = pull(name, True)
            np.testing.assert_array_equal(t[2], csr.colidx.astype(np.int64))               # A' = A
    assert graph("empty").nnz == 0 and graph("empty").n > 1
    assert graph("one").n == 1 and graph("one").nnz == 1
    rev = graph("dw-rev")
    rp = rev.rowptr.astype(np.int64)
    assert (np.diff(rev.colidx[rp[10]:rp[11]].astype(np.int64)) < 0).all() and rp[11] - rp[10] == 5000


def test_cast_matches_sat_u64():
    pool = np.array([-3.5, np.nan, 2.0 ** 70, 0.75, 7.9, 1e19, 0.0, 42.0, 2.0 ** 63, 2.0 ** 64, np.inf, -np.inf,
                     1e300, 1.0, np.nextafter(2.0 ** 64, 0), np.nextafter(2.0 ** 63, 0), 2.0 ** 53 + 2])
    np.testing.assert_array_equal(cast_u64(pool), np.array([sat_u64(x) for x in pool], np.uint64))


def test_finish_by_hand():
    """finish() against the header's sentences, entry by entry, on a hand-made vector."""
    t = np.array([5, 7, I64.max, I64.max, 2, I64.max, 4, 1], np.int64)
    hit = t != I64.max
    w = np.array([3, 9, 6, I64.min, -8, 8, 0, I64.min], np.int64)
    wp = np.array([1, 1, 1, 0, 1, 1, 1, 0], np.uint8)
    mask = np.array([1, 1, 1, 1, 0, 0, 0, 0], np.uint8)
    f = lambda desc, p=wp, m=mask: finish(SI, t, hit, m, desc, w, p)[:2]
    out, p = f(0)
    assert out.tolist() == [5, 7, I64.max, I64.max, -8, 8, 0, I64.min] and p.tolist() == [1, 1, 0, 0, 1, 1, 1, 0]
    out, p = f(ACCUM)
    assert out.tolist() == [3, 7, 6, I64.max, -8, 8, 0, I64.min] and p.tolist() == [1, 1, 1, 0, 1, 1, 1, 0]
    out, p = f(REPLACE | ACCUM)
    assert out.tolist() == [3, 7, 6, I64.max] + [I64.max] * 4 and p.tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    out, p = f(COMP | REPLACE)
    assert out.tolist() == [I64.max] * 4 + [2, I64.max, 4, 1] and p.tolist() == [0, 0, 0, 0, 1, 0, 1, 1]
    out, p = f(ACCUM, None, None)            # every old entry present: min(w, t), w kept where t is absent
    assert p is None and out.tolist() == [3, 7, 6, I64.min, -8, 8, 0, I64.min]
    out, p = f(0, None, None)
    assert p is None and out.tolist() == t.tolist()


@pytest.mark.parametrize("family", ["directed", "undirected"])
@pytest.mark.parametrize("sr", list(NAMES), ids=list(NAMES.values()))
def test_oracle_matches_numpy_reference(sr, family):
    """orc_mxv against the numpy restatement over the whole case set (MIN_SECONDI is not in the oracle:
    for it this only checks that the cases make the segment combine observable)."""
    cases = family_cases(sr, family)
    assert_combine_observable(sr, cases, minima=family == "directed")
    if sr == MP and family == "directed":
        assert any((c["prod"].hit & np.isinf(c["prod"].t)).any() for c in cases)   # a present +inf result
        assert any(c["prod"].overflow for c in cases)                              # finite u + 1e300 = +inf
    if sr == SI:
        return
    for c in cases:
        got, gotp = O.mxv(graph(c["name"]), sr, c["u"], c["up"], c["mask"], c["desc"], c["w"], c["wp"], vxm=c["vxm"])
        compare(c, got, gotp)


def test_oracle_matches_numpy_reference_tiny_graphs():
    for name in ("empty", "one"):
        for sr in (PS, MS, AP, MP, PP):
            for c in op_cases(name, sr):
                got, gotp = O.mxv(graph(name), sr, c["u"], c["up"], c["mask"], c["desc"], c["w"], c["wp"], vxm=c["vxm"])
                compare(c, got, gotp)


@pytest.mark.parametrize("name", MXM_GRAPHS)
def test_oracle_mxm_matches_dense_product(name):
    csr = graph(name)
    rp = csr.rowptr.astype(np.int64)
    rows = np.repeat(np.arange(csr.n), np.diff(rp))
    cols = csr.colidx.astype(np.int64)
    if name in ("mxm-directed", "mxm-undirected"):
        assert csr.n <= 1500 and np.diff(rp).max() > 1000 and (np.diff(rp) == 0).sum() >= 20
        assert (rows == cols).sum() >= 20                                                  # self-loops
        assert (np.diff(cols)[np.diff(rows) == 0] < 0).any()                               # unsorted rows
        sym = np.array_equal(np.sort(rows * csr.n + cols), np.sort(cols * csr.n + rows))
        assert sym == (name == "mxm-undirected")
    np.testing.assert_array_equal(O.mxm_masked(csr), dense_mxm(csr))


# ------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def gpu_ctx():
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    c = Context(0)
    yield c
    c.close()


class Graphs:
    """Device graphs by name, made on first use and freed together."""

    def __init__(self, ctx):
        self.ctx, self.made = ctx, {}

    def __getitem__(self, name):
        from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
        if name not in self.made:
            self.made[name] = A.Graph(self.ctx, graph(name), directed=DIRECTED[name])
        return self.made[name]

    def close(self):
        for g in self.made.values():
            g.close()


def run_cases(gpu_ctx, cases, worst=None):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    gs = Graphs(gpu_ctx)
    try:
        for c in cases:
            fn = A.vxm if c["vxm"] else A.mxv
            got, gotp = fn(gs[c["name"]], c["sr"], c["u"], c["up"], c["mask"], c["desc"], c["w"], c["wp"])
            compare(c, got, gotp, worst)
    finally:
        gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["directed", "undirected"])
@pytest.mark.parametrize("sr", list(NAMES), ids=list(NAMES.values()))
def test_gpu_ops_match_numpy_reference(gpu_ctx, sr, family):
    cases = family_cases(sr, family)
    assert_combine_observable(sr, cases, minima=family == "directed")   # before any device call
    worst = []
    run_cases(gpu_ctx, cases, worst)
    if worst:
        print(f"{NAMES[sr]} {family}: worst error / bound = {max(worst):.3g} over {len(cases)} cases")


@pytest.mark.gpu
def test_gpu_ops_tiny_graphs(gpu_ctx):
    """nnz = 0 and n = 1 (a weighted self-loop), every semiring and descriptor."""
    run_cases(gpu_ctx, [c for name in ("empty", "one") for sr in NAMES for c in op_cases(name, sr)])


@pytest.mark.gpu
def test_gpu_mxm_masked_matches_dense_product(gpu_ctx):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    from ldbc_graphalytics_platforms_graphblas_amd._native import GxError
    gs = Graphs(gpu_ctx)
    try:
        for name in MXM_GRAPHS:
            got = A.mxm_masked(gs[name])
            assert got.dtype == np.int64
            np.testing.assert_array_equal(got, dense_mxm(graph(name)), err_msg=name)
        G = gs["mxm-directed"]
        for sr, desc in [(PS, 0), (MS, 0), (AP, 0), (MP, 0), (SI, 0), (PP, T0), (PP, ACCUM), (PP, COMP | REPLACE)]:
            with pytest.raises(GxError) as e:
                A.mxm_masked(G, sr, desc)
            assert e.value.code == GX_NOT_IMPLEMENTED
            np.testing.assert_array_equal(A.mxm_masked(G), dense_mxm(graph("mxm-directed")))
    finally:
        gs.close()


@pytest.mark.gpu
def test_gpu_argument_errors_leave_the_context_usable(gpu_ctx):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    from ldbc_graphalytics_platforms_graphblas_amd._native import GxError
    gs = Graphs(gpu_ctx)
    try:
        G = gs["mxm-directed"]
        n = G.n
        good = next(iter(op_cases("mxm-directed", MP, orientations=((True, False),))))

        def still_works():
            compare(good, *A.vxm(G, MP, good["u"], good["up"], good["mask"], good["desc"], good["w"], good["wp"]))

        still_works()
        u, w = np.zeros(n), np.zeros(n)
        for fn in (N.lib().gx_mxv, N.lib().gx_vxm):      # the Python wrappers know no such semiring
            for sr in (6, -1, 99):
                assert fn(G.handle, sr, 0, None, A._vp(u), None, A._vp(w), None) == GX_INVALID_VALUE
                still_works()
        for sr, vxm in sorted(READS_U):
            with pytest.raises(GxError) as e:
                (A.vxm if vxm else A.mxv)(G, sr, None, None, None, 0, None, None)
            assert e.value.code == GX_NULL_POINTER
            still_works()
    finally:
        gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dw", "uu"])
@pytest.mark.parametrize("kernel", ["adaptive", "default"])
def test_gpu_pagerank_and_mxv_share_one_plan(gpu_ctx, monkeypatch, kernel, name):
    """mxv(PLUS_SECOND, T0) borrows the graph's cached PageRank plan and swaps its damping for the call:
    alternating the two on one graph changes neither.

    Bit-identity of the repeated results is asserted on the CSR-Adaptive kernel (GX_PR_KERNEL=adaptive),
    whose row-order sums are bitwise deterministic; the plan, its buffers, the damping swap and pr_step's
    call are the same code for both kernels.  The default column-sorted kernel adds into LDS in wave-arrival
    order and is documented as not bit-reproducible run to run (gx_pr_sorted.hip, DESIGN.md "Numerics"):
    measured on an MI355X, two LA_PR(0.85, 5) calls straight after each other on the directed crafted graph
    differed in 6998 of 7001 entries (at most 1.1e-15 relative; 5492 entries on the undirected one), and two
    mxv calls in 135 (43).  So there every result is held to its reference instead (1e-12 of the oracle, the
    fsum bound), which a leaked damping of 1 or a stale x would miss by many orders of magnitude."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    if kernel != "default":
        monkeypatch.setenv("GX_PR_KERNEL", kernel)
    csr = graph(name)
    u = np.random.default_rng(12).random(csr.n)
    prod = Product(name, PS, u, None, False, True)
    G = A.Graph(gpu_ctx, csr, directed=DIRECTED[name])
    try:
        pr1 = A.LA_PR(G, 0.85, 5)
        m1, _ = A.mxv(G, PS, u, None, None, T0)
        pr2 = A.LA_PR(G, 0.85, 5)
        m2, _ = A.mxv(G, PS, u, None, None, T0)
    finally:
        G.close()
    want = O.pagerank(csr, DIRECTED[name], 0.85, 5)
    atol = prod.row_len * EPS * prod.abs_sum
    for pr, m in ((pr1, m1), (pr2, m2)):
        np.testing.assert_allclose(pr, want, rtol=1e-12, atol=0)
        err = np.abs(m - prod.t)
        assert (err <= atol).all(), f"worst error/bound {np.max(err[atol > 0] / atol[atol > 0]):.3g}"
    if kernel == "adaptive":
        np.testing.assert_array_equal(pr1, pr2)
        np.testing.assert_array_equal(m1, m2)
