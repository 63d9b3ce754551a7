"""LCC on every triangle tier, the large workgroup tables, the merge fallback and the inputs the
closure build has to clean up, against a dense restatement of the formula.

The reference (`_dense_lcc`) is plain numpy and never calls the oracle: with A the 0/1 matrix of
the stored entries (diagonal cleared) and S = max(A, A^T),
    num(v) = sum_{u, w} S[v, u] A[u, w] S[w, v],   k(v) = sum_u S[v, u],
    LCC(v) = num / (k (k - 1)),   0 when k < 2.
Every matrix entry and every product entry is an integer below 2^24, so fp32 and fp64 products
are exact, and the quotient is the one fp64 division k_lcc_final performs: comparisons are
bit-exact.  The CPU tests hold the oracle to the same reference.

Tier membership is decided by the oriented out-degree |O(u)| (neighbours ranking above u by
(closure degree, id)); `_oriented` restates it and every GPU test first asserts, on the CPU,
that its graph populates the paths it is there for.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (sys.path)
from oracle import oracle as O

KNOBS = {"GX_LCC_WAVE_MAX": "8", "GX_LCC_WAVE2_MAX": "24", "GX_LCC_BLOCK_MAX": "48"}
KNOB_LIMITS = (8, 24, 48)
DEFAULT_LIMITS = (256, 512, 8192)   # kWaveMax, kWave2Max, kBlockMax of gx_lcc.h
TIMERS = ("lcc_wave", "lcc_wave2", "lcc_block", "lcc_merge")
KNOB_SEED = 51   # chosen so that the 128th and 129th largest closure degrees differ (_knob_case)
FP64_MAX_N = 1500


# ----------------------------------------------------------------------------- reference
def _entries(csr):
    rp = csr.rowptr.astype(np.int64)
    rows = np.repeat(np.arange(csr.n, dtype=np.int64), np.diff(rp))
    return rows, csr.colidx.astype(np.int64)


def _matrices(csr, verts=None):
    """A (stored entries, diagonal cleared) and S = max(A, A^T), dense, over `verts` (sorted
    vertex ids holding every entry's endpoints) or all vertices."""
    rows, cols = _entries(csr)
    m = csr.n
    if verts is not None:
        verts = np.asarray(verts, dtype=np.int64)
        assert np.all(np.diff(verts) > 0) and np.isin(rows, verts).all() and np.isin(cols, verts).all()
        rows, cols = np.searchsorted(verts, rows), np.searchsorted(verts, cols)
        m = len(verts)
    A = np.zeros((m, m), dtype=np.float64 if m <= FP64_MAX_N else np.float32)
    A[rows, cols] = 1
    np.fill_diagonal(A, 0)
    return A, np.maximum(A, A.T)


def _lcc_of(A, S):
    assert A.shape[0] < 2 ** 24   # product entries stay exact in fp32
    num = ((S @ A) * S).sum(1, dtype=np.float64).astype(np.int64)
    k = S.sum(1, dtype=np.float64)
    lcc = np.zeros(len(k))
    np.divide(num.astype(np.float64), k * (k - 1), out=lcc, where=k >= 2)
    return lcc, num


def _scatter(csr, verts, lcc, num):
    if verts is None:
        return lcc, num
    full_l, full_n = np.zeros(csr.n), np.zeros(csr.n, dtype=np.int64)
    full_l[verts], full_n[verts] = lcc, num
    return full_l, full_n


def _dense_lcc(csr, verts=None):
    """(LCC, numerators) of every vertex of `csr`; `verts` restricts the dense matrices to the
    vertices that carry entries (all others are isolated: 0)."""
    return _scatter(csr, verts, *_lcc_of(*_matrices(csr, verts)))


def _oriented(S):
    """(|O(u)|, |I(u)|, rank key): neighbours ranking above / below u by (degree, id), the
    orientation of ranks_above in gx_lcc_orient.hip."""
    n = S.shape[0]
    deg = S.sum(1, dtype=np.float64).astype(np.int64)
    key = deg * n + np.arange(n)
    nb = S > 0
    d = (nb & (key[None, :] > key[:, None])).sum(1)
    return d, deg - d, key


def _tiers(d, e, limits):
    """Tier of every vertex that makes work items (non-empty O and I lists), -1 for the others:
    0 wave, 1 wave (1024 slots), 2 workgroup, 3 merge fallback (k_lcc_items)."""
    return np.where((d > 0) & (e > 0), np.digitize(d, limits, right=True), -1)


# -------------------------------------------------------------------------------- graphs
def _clique_edges(n, K, p, seed, background):
    """clique(K, p) in n vertices: each pair of 0..K-1 kept with probability p, stored in one
    random direction and 30 % also in the other; `background` random edges over all vertices."""
    rng = np.random.default_rng(seed)
    a, b = np.triu_indices(K, 1)
    if p < 1.0:
        keep = rng.random(len(a)) < p
        a, b = a[keep], b[keep]
    flip = rng.random(len(a)) < 0.5
    s, d = np.where(flip, a, b), np.where(flip, b, a)
    both = rng.random(len(a)) < 0.3
    bs, bd = rng.integers(0, n, background), rng.integers(0, n, background)
    ok = bs != bd
    return np.concatenate([s, d[both], bs[ok]]), np.concatenate([d, s[both], bd[ok]])


def _clique_csr(n, K, p, seed, background, directed):
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
    src, dst = _clique_edges(n, K, p, seed, background)
    return csr_from_edges(n, src, dst, None, symmetric=not directed)


@functools.lru_cache(maxsize=None)
def _knob_case(directed):
    """clique(400, 1.0) in 1500 vertices.  With the limits lowered to 8 / 24 / 48 it holds
    vertices of all four tiers, workgroup-tier vertices with more than one 256-entry chunk of
    I(u) and wave-tier ones with more than one 64-entry chunk; its 128 highest degrees are
    strictly above the 129th (a dense core of exactly 128 at GX_LCC_CORE=128), and block- and
    merge-tier vertices have in-neighbours in that core."""
    n, K = 1500, 400
    csr = _clique_csr(n, K, 1.0, KNOB_SEED, 4000, directed)
    A, S = _matrices(csr)
    lcc, num = _lcc_of(A, S)
    d, e, key = _oriented(S)
    t = _tiers(d, e, KNOB_LIMITS)
    pop = [int((t == i).sum()) for i in range(4)]
    assert min(pop) >= 16, pop
    assert pop[3] >= 300 and d.max() >= K - 1, pop
    assert (e[t == 2] > 256).all(), "every workgroup-tier vertex has several chunks of I(u)"
    assert ((t <= 1) & (t >= 0) & (e > 64)).sum() >= 16, "wave-tier vertices with several chunks"
    # without the knobs: the wave tiers only
    t0 = _tiers(d, e, DEFAULT_LIMITS)
    assert (t0 == 0).any() and (t0 == 1).any() and not (t0 >= 2).any()
    # the dense core at GX_LCC_CORE=128 (lcc_dense_build): degrees above the 129th largest
    deg = S.sum(1).astype(np.int64)
    top = np.sort(deg)[::-1]
    assert top[127] > top[128], "the degree cut must leave a core of exactly 128"
    core = deg > top[128]
    assert core.sum() == 128
    core_in = ((S > 0) & (key[None, :] < key[:, None]) & core[None, :]).any(1)
    assert (core_in & (t == 2)).any() and (core_in & (t == 3)).any()
    return csr, lcc, num


@functools.lru_cache(maxsize=None)
def _big_case(K, p, n, seed, lo, hi, at_least):
    """Directed clique(K, p) in n vertices with at least `at_least` work-item vertices of
    |O(u)| in (lo, hi] and none above hi."""
    csr = _clique_csr(n, K, p, seed, 3000, True)
    A, S = _matrices(csr)
    lcc, num = _lcc_of(A, S)
    d, e, _ = _oriented(S)
    live = (d > 0) & (e > 0)
    assert d.max() <= hi and int((live & (d > lo)).sum()) >= at_least, (int(d.max()), int((live & (d > lo)).sum()))
    return csr, lcc, num, d


def _table_case():
    """clique(2300, 0.98) in 2400 vertices: |O(u)| in (2048, 4096] -- 8192-slot tables, 64 KiB
    of dynamic LDS next to the kernel's static arrays -- and in (1024, 2048] (4096 slots)."""
    csr, lcc, num, d = _big_case(2300, 0.98, 2400, 2, 2048, 4096, 100)
    assert int(((d > 1024) & (d <= 2048)).sum()) >= 500
    return csr, lcc, num


def _shuffled_csr(n, src, dst, seed):
    """CSR of distinct (src, dst) pairs with every row's columns in a random order."""
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import CSR
    pairs = np.unique(np.stack([src, dst], axis=1), axis=0)
    rng = np.random.default_rng(seed)
    order = np.lexsort((rng.random(len(pairs)), pairs[:, 0]))
    pairs = pairs[order]
    rp = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.bincount(pairs[:, 0], minlength=n), out=rp[1:])
    return CSR(n, rp, pairs[:, 1].astype(np.uint64))


@functools.lru_cache(maxsize=None)
def _raw_case(symmetric):
    """3000 vertices, 40 000 random entries of which 500 are self-loops, rows in random column
    order, no column twice in a row; `symmetric` adds every entry's reverse."""
    n = 3000
    rng = np.random.default_rng(4)
    loops = rng.choice(n, 500, replace=False)
    src = np.concatenate([rng.integers(0, n, 39500), loops])
    dst = np.concatenate([rng.integers(0, n, 39500), loops])
    if symmetric:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    csr = _shuffled_csr(n, src, dst, 5)
    rows, cols = _entries(csr)
    assert (rows == cols).sum() >= 500
    same_row = rows[1:] == rows[:-1]
    assert (cols[1:][same_row] < cols[:-1][same_row]).sum() > 1000, "rows are not sorted"
    assert len(np.unique(rows * n + cols)) == len(rows), "a column repeats in a row"
    lcc, num = _dense_lcc(csr)
    assert np.count_nonzero(lcc) > 100
    return csr, lcc, num


def _loop_cases():
    """(csr, expected LCC): a graph whose only entries are self-loops, and a triangle 3-4-5 whose
    last vertex's row -- the end of the column array -- ends in a self-loop."""
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import CSR
    u64 = np.uint64
    only = CSR(5, np.array([0, 1, 1, 2, 2, 3], dtype=u64), np.array([0, 2, 4], dtype=u64))
    last = CSR(6, np.array([0, 0, 0, 0, 2, 3, 6], dtype=u64), np.array([5, 4, 5, 4, 3, 5], dtype=u64))
    # row 3 = {5, 4}, row 4 = {5}, row 5 = {4, 3, 5}: every vertex of the triangle has k = 2;
    # 3: 4->5 and 5->4 (2 / 2); 4: 3->5 and 5->3 (2 / 2); 5: 3->4 only (1 / 2)
    return [(only, np.zeros(5)), (last, np.array([0, 0, 0, 1.0, 1.0, 0.5]))]


@functools.lru_cache(maxsize=None)
def _sparse_case():
    """n = 2^24 + 5 with ~380 vertices carrying edges (the 40 lowest ids, the 40 highest, 300
    random ones) and 6000 random directed entries among them: ids past 2^24 (4-byte column
    upload, 25 key bits in the orientation's sort) and long runs of empty rows."""
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
    n = 2 ** 24 + 5
    rng = np.random.default_rng(6)
    verts = np.unique(np.concatenate([np.arange(40), np.arange(n - 40, n), rng.integers(40, n - 40, 300)]))
    src, dst = verts[rng.integers(0, len(verts), 6000)], verts[rng.integers(0, len(verts), 6000)]
    csr = csr_from_edges(n, src, dst, None, symmetric=False)
    lcc, num = _dense_lcc(csr, verts)
    assert 370 <= len(verts) <= 380 and np.count_nonzero(lcc) >= 370
    assert lcc[n - 1] > 0 and lcc[0] > 0 and lcc[2 ** 24:].all()
    return csr, lcc, num


# ----------------------------------------------------------------------------- CPU tests
def test_dense_reference_by_hand():
    """A triangle 0-1-2 with the pendant vertex 3 on 2 and one reciprocal edge (0 <-> 1)."""
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
    src, dst = np.array([0, 1, 1, 2, 2]), np.array([1, 0, 2, 0, 3])
    lcc, num = _dense_lcc(csr_from_edges(4, src, dst, None, symmetric=False))
    # 0: N = {1, 2}, 1->2; 1: N = {0, 2}, 2->0; 2: N = {0, 1, 3}, 0->1 and 1->0; 3: k = 1
    np.testing.assert_array_equal(num, [1, 1, 2, 0])
    np.testing.assert_array_equal(lcc, [1 / 2, 1 / 2, 2 / 6, 0.0])
    lcc, num = _dense_lcc(csr_from_edges(4, src, dst, None, symmetric=True))
    np.testing.assert_array_equal(num, [2, 2, 2, 0])
    np.testing.assert_array_equal(lcc, [1.0, 1.0, 2 / 6, 0.0])
    for csr, want in _loop_cases():
        np.testing.assert_array_equal(_dense_lcc(csr)[0], want)


@pytest.mark.parametrize("name", ["example-directed", "example-undirected", "test-lcc-directed",
                                  "test-lcc-undirected"])
def test_oracle_matches_dense_on_fixtures(name, fixture_graphs):
    g = fixture_graphs(name)
    np.testing.assert_array_equal(O.lcc(g.csr, g.directed), _dense_lcc(g.csr)[0])


@pytest.mark.parametrize("case", ["knob-directed", "knob-undirected", "raw-directed", "raw-undirected", "sparse",
                                  "loops"])
def test_oracle_matches_dense(case):
    """The oracle equals the dense formula bit for bit on the graphs of the GPU tests below
    (all but the two large cliques, which take it tens of seconds)."""
    if case == "loops":
        for csr, want in _loop_cases():
            np.testing.assert_array_equal(O.lcc(csr, True), want)
        return
    kind, _, direction = case.partition("-")
    directed = direction != "undirected"
    csr, lcc, _ = {"knob": lambda: _knob_case(directed), "raw": lambda: _raw_case(not directed),
                   "sparse": _sparse_case}[kind]()
    np.testing.assert_array_equal(O.lcc(csr, directed), lcc)


# ----------------------------------------------------------------------------- GPU tests
@pytest.fixture(scope="module")
def ctx():
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    c = Context(0)
    yield c
    c.close()


def _gpu_lcc(ctx, csr, directed, calls=1):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    G = A.Graph(ctx, csr, directed)
    try:
        return [A.LA_LCC(G) for _ in range(calls)]
    finally:
        G.close()


@pytest.mark.gpu
@pytest.mark.parametrize("knobs,core", [(True, None), (True, "128"), (False, None)])
def test_all_tiers_and_fallback(ctx, monkeypatch, knobs, core):
    """clique(400, 1.0) in 1500 vertices with the tier limits lowered to 8 / 24 / 48: both wave
    kernels, the workgroup kernel over several 256-entry chunks of I(u) and the merge fallback
    all run (one nested timer each per call), twice on one graph (the second call on the cached
    items).  With GX_LCC_CORE=128 the block and merge kernels also skip core-bit entries and the
    core's triangles come from the MFMA pass.  Without the knobs the same graph takes the two
    wave kernels only."""
    monkeypatch.delenv("GX_LCC_CORE", raising=False)
    for k, v in KNOBS.items():
        monkeypatch.setenv(k, v) if knobs else monkeypatch.delenv(k, raising=False)
    if core:
        monkeypatch.setenv("GX_LCC_CORE", core)
    calls = 2
    for directed in (True, False):
        csr, want, _ = _knob_case(directed)
        ctx.reset_kernel_stats()
        ctx.set_kernel_timing(True)
        try:
            got = _gpu_lcc(ctx, csr, directed, calls)
        finally:
            ctx.set_kernel_timing(False)
        launches = {name: ctx.kernel_stats(name)[0] for name in TIMERS + ("lcc_triangles", "lcc_core")}
        for g in got:
            np.testing.assert_array_equal(g, want)
        expect = dict.fromkeys(TIMERS, calls if knobs else 0)
        expect.update(lcc_wave=calls, lcc_wave2=calls, lcc_triangles=calls, lcc_core=calls if core else 0)
        assert launches == expect


@pytest.mark.gpu
def test_block_tables_64k(ctx):
    """|O(u)| in (2048, 4096]: the workgroup kernel with 8192-slot tables, exactly 64 KiB of
    dynamic LDS on top of its static arrays."""
    csr, want, _ = _table_case()
    np.testing.assert_array_equal(_gpu_lcc(ctx, csr, True)[0], want)


@pytest.mark.gpu
def test_block_tables_128k(ctx):
    """|O(u)| above 4096 (at most 8192, so still the workgroup tier): 16 384-slot tables, 128 KiB
    of dynamic LDS.  clique(4400, 0.985) in 4500 vertices, directed."""
    csr, want, _, _ = _big_case(4400, 0.985, 4500, 3, 4096, 8192, 32)
    np.testing.assert_array_equal(_gpu_lcc(ctx, csr, True)[0], want)


@pytest.mark.gpu
@pytest.mark.parametrize("symmetric", [False, True])
def test_raw_csr(ctx, symmetric):
    """Rows in random column order and self-loops, given as a raw CSR (directed, and symmetrised
    as an undirected graph); a graph of self-loops only; a last row ending in a self-loop."""
    csr, want, _ = _raw_case(symmetric)
    np.testing.assert_array_equal(_gpu_lcc(ctx, csr, not symmetric)[0], want)
    if not symmetric:
        for small, expect in _loop_cases():
            np.testing.assert_array_equal(_gpu_lcc(ctx, small, True)[0], expect)


@pytest.mark.gpu
def test_sparse_high_ids(ctx):
    """Vertex ids above 2^24 among 16.7 M mostly isolated vertices."""
    csr, want, _ = _sparse_case()
    np.testing.assert_array_equal(_gpu_lcc(ctx, csr, True)[0], want)


PART_RANGES = [(0, 37), (37, 37), (37, 250), (250, 1499), (1499, 1500)]


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [True, False])
def test_partition_ranges(ctx, monkeypatch, knobs):
    """gx_lcc_part_counts on arbitrary vertex ranges (an empty one, a single vertex) adds up to
    the dense numerators exactly -- the n counters themselves, not only the quotient -- as do
    one range over everything and the balanced ranges of gx_lcc_part_ranges."""
    import torch
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    from ldbc_graphalytics_platforms_graphblas_amd.distributed import GpuBackend
    monkeypatch.delenv("GX_LCC_CORE", raising=False)
    for k, v in KNOBS.items():
        monkeypatch.setenv(k, v) if knobs else monkeypatch.delenv(k, raising=False)
    for directed in (True, False):
        csr, want, num = _knob_case(directed)
        n = csr.n
        G = A.Graph(ctx, csr, directed)
        part = None
        try:
            part = GpuBackend(G).lcc_part()

            def counted(ranges):
                tc = torch.zeros(n, dtype=torch.int64, device="cuda:0")
                for v0, v1 in ranges:
                    part.counts(int(v0), int(v1), tc)
                return tc

            tc = counted(PART_RANGES)
            np.testing.assert_array_equal(tc.cpu().numpy(), num)
            np.testing.assert_array_equal(counted([(0, n)]).cpu().numpy(), num)
            out = torch.zeros(n, dtype=torch.float64, device="cuda:0")
            part.finish(tc, out)
            np.testing.assert_array_equal(out.cpu().numpy(), want)
            for k in (1, 2, 3, 7):
                r = part.ranges(k).astype(np.int64)
                assert len(r) == k + 1 and r[0] == 0 and r[-1] == n and (np.diff(r) >= 0).all(), r
                np.testing.assert_array_equal(counted(zip(r[:-1], r[1:])).cpu().numpy(), num)
        finally:
            if part is not None:
                part.close()
            G.close()


def _multi_lcc(ctxs, csr, directed):
    """gx_lcc_multi over the contexts `ctxs` (virtual devices when they share a GPU)."""
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    out = np.zeros(csr.n)
    arr = (C.c_void_p * len(ctxs))(*[c.handle.value for c in ctxs])
    s = csr.as_c()
    N.check(N.lib().gx_lcc_multi(arr, len(ctxs), C.byref(s), int(directed), N.as_dp(out)), "gx_lcc_multi")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["knobs", "tables"])
def test_multi_three_virtual_devices(monkeypatch, case):
    """gx_lcc_multi on three virtual devices: the knob graph with the limits lowered (every
    device's range holds several tiers), and the 64 KiB-table graph."""
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    monkeypatch.delenv("GX_LCC_CORE", raising=False)
    for k, v in KNOBS.items():
        monkeypatch.setenv(k, v) if case == "knobs" else monkeypatch.delenv(k, raising=False)
    graphs = [(_knob_case(d)[:2], d) for d in (True, False)] if case == "knobs" else [(_table_case()[:2], True)]
    ctxs = [Context(0) for _ in range(3)]
    try:
        for (csr, want), directed in graphs:
            np.testing.assert_array_equal(_multi_lcc(ctxs, csr, directed), want)
    finally:
        for c in ctxs:
            c.close()
