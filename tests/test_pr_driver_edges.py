"""Edges of the PageRank driver (gx_pr.hip, gx_pr_order.hip, gx_pr_part.hip) that the other files
do not reach: the adaptive kernel's LONG rows in several segments, a partition whose dangling rows
are a list, a range that is no suffix, or absent, a cached plan called under another GX_PR_KERNEL,
and GX_PLAN_TIMES on both entry points.  Every GPU case against the oracle at the parity bar of
tests/test_pr_first.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (sys.path)
from oracle import oracle as O

PR_RTOL = 1e-12

_CACHE = {}


def _want(key, csr, directed, d, iters):
    """The oracle's scores, computed once per (graph key, damping, iterations)."""
    k = ("r", key, d, iters)
    if k not in _CACHE:
        _CACHE[k] = O.pagerank(csr, directed, d, iters)
    return _CACHE[k]


def _small():
    if "small" not in _CACHE:
        from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat
        _CACHE["small"] = rmat(12, 16, 11)
    return _CACHE["small"]


STAR_N = 24000


def _star(directed):
    """A star on STAR_N vertices over an R-MAT graph of scale 11 among the first 2048.
    Undirected: the centre (vertex 0) is joined to everyone, a row of STAR_N - 1 entries.
    Directed: every vertex v with v % 7 != 3 points at the centre, which has no out-edge (a
    sink of in-degree about 20 570); the others past the R-MAT part have none either, so the
    dangling vertices lie scattered over the whole id range."""
    key = ("star", directed)
    if key not in _CACHE:
        from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges, rmat
        base = rmat(11, 8, 5, undirected=not directed)
        rp = base.rowptr.astype(np.int64)
        bs = np.repeat(np.arange(base.n, dtype=np.int64), np.diff(rp))
        bd = base.colidx.astype(np.int64)
        v = np.arange(1, STAR_N, dtype=np.int64)
        if directed:
            keep = bs != 0
            bs, bd = bs[keep], bd[keep]
            v = v[v % 7 != 3]
        src = np.concatenate([bs, v])
        dst = np.concatenate([bd, np.zeros(len(v), np.int64)])
        _CACHE[key] = csr_from_edges(STAR_N, src, dst, None, symmetric=not directed)
    return _CACHE[key]


def test_star_rows_span_three_segments():
    """The inputs are what the GPU cases say: the centre's pull row has more than two and at
    most three segments of 8192 entries, and the directed star's dangling vertices are neither
    one range nor few."""
    seg = 8192   # kSegNnz, gx_pr.h
    und = _star(False)
    assert 2 * seg < int(np.diff(und.rowptr.astype(np.int64))[0]) <= 3 * seg
    dcsr = _star(True)
    deg = np.diff(dcsr.rowptr.astype(np.int64))
    assert deg[0] == 0
    assert 2 * seg < int(np.count_nonzero(dcsr.colidx == 0)) <= 3 * seg
    dang = np.flatnonzero(deg == 0)
    assert len(dang) > 1000 and dang[-1] - dang[0] + 1 > len(dang)


@pytest.fixture(scope="module")
def ctx():
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("directed", [False, True], ids=["undirected", "directed"])
def test_adaptive_long_row_in_segments(ctx, monkeypatch, directed):
    """GX_PR_KERNEL=adaptive: the centre's row is three LONG segments joined by the ticket, beside
    STREAM blocks; 1 and 4 iterations on one resident graph."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    monkeypatch.setenv("GX_PR_KERNEL", "adaptive")
    csr = _star(directed)
    G = A.Graph(ctx, csr, directed)
    try:
        for iters in (1, 4):
            np.testing.assert_allclose(A.LA_PR(G, 0.85, iters), _want(("star", directed), csr, directed, 0.85, iters),
                                       rtol=PR_RTOL, atol=0, err_msg=f"iters {iters}")
    finally:
        G.close()


PART_N = 2000


def _dangling_graph(shape):
    """A directed graph on PART_N vertices in its own order: 12 000 random edges and a ring
    v -> v + 1, with the out-edges of some vertices removed: 300 scattered ones ("list"), the
    range [700, 900) ("range"), or none ("none")."""
    key = ("dang", shape)
    if key not in _CACHE:
        from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
        rng = np.random.default_rng(31)
        n = PART_N
        ring = np.arange(n, dtype=np.int64)
        src = np.concatenate([rng.integers(0, n, 12000), ring])
        dst = np.concatenate([rng.integers(0, n, 12000), (ring + 1) % n])
        sink = np.zeros(n, dtype=bool)
        if shape == "list":
            sink[rng.choice(n, 300, replace=False)] = True
        elif shape == "range":
            sink[700:900] = True
        keep = ~sink[src]
        _CACHE[key] = csr_from_edges(n, src[keep], dst[keep], None, symmetric=False)
    return _CACHE[key]


@pytest.mark.parametrize("shape,count", [("list", 300), ("range", 200), ("none", 0)])
def test_dangling_graph_shapes(shape, count):
    """The partition cases' inputs: the dangling vertices are scattered, one range that is no
    suffix, or absent, and (where there are any) they have in-edges."""
    csr = _dangling_graph(shape)
    deg = np.diff(csr.rowptr.astype(np.int64))
    dang = np.flatnonzero(deg == 0)
    assert len(dang) == count
    if shape == "list":
        assert dang[-1] - dang[0] + 1 > len(dang)
    if shape == "range":
        assert dang[0] == 700 and dang[-1] == 899 < csr.n - 1
    if count:
        assert np.isin(csr.colidx.astype(np.int64), dang).any()


def _part_step(ctx, n_global, nranks, lr, damping):
    """A pr_partition.GpuStep whose part comes from gx_pr_part_create itself (every row
    exchanged), not from the _live variant GpuStep calls."""
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    from ldbc_graphalytics_platforms_graphblas_amd.pr_partition import GpuStep
    st = GpuStep.__new__(GpuStep)
    st.N, st.lib, st.part, st._live = N, N.lib(), C.c_void_p(), None
    N.check(st.lib.gx_pr_part_create(ctx.handle, n_global, nranks, lr.rank, N.as_u64p(lr.row_ranges),
                                     N.as_u64p(lr.rowptr), N.as_u64p(lr.colidx) if lr.nnz else None,
                                     N.as_u64p(lr.outdeg), damping, C.byref(st.part)), "gx_pr_part_create")
    ch = C.c_uint64(0)
    N.check(st.lib.gx_pr_part_chunk(st.part, C.byref(ch)), "gx_pr_part_chunk")
    st.chunk = ch.value
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["sorted", "adaptive"])
@pytest.mark.parametrize("nranks", [1, 2])
@pytest.mark.parametrize("shape", ["list", "range", "none"])
def test_partition_dangling_rows(monkeypatch, shape, nranks, kernel):
    """gx_pr_part_create on a directed graph in its original vertex order, stepped as
    pr_partition.GpuStep steps a part, the exchange a device concat: the dangling rows of a rank
    are a list, a range inside its rows, or none, where every other partition test relabels
    hub-first and has them as a suffix."""
    import torch
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    from ldbc_graphalytics_platforms_graphblas_amd.pr_partition import local_rows
    monkeypatch.setenv("GX_PR_KERNEL", kernel)
    csr = _dangling_graph(shape)
    pull = csr.transpose()
    c = Context(0)
    dev = torch.device("cuda", 0)
    steps, lrs = [], []
    try:
        for r in range(nranks):
            lr = local_rows(csr, True, nranks, r, pull=pull)
            lrs.append(lr)
            steps.append(_part_step(c, csr.n, nranks, lr, 0.85))
        chunk = steps[0].chunk
        xl = [torch.zeros(chunk, dtype=torch.float64, device=dev) for _ in range(nranks)]
        xf = torch.zeros(chunk * nranks, dtype=torch.float64, device=dev)
        ro = [torch.zeros(max(lr.rows, 1), dtype=torch.float64, device=dev) for lr in lrs]
        iters = 5
        for r in range(nranks):
            steps[r].init(xl[r], 0)
        torch.cuda.synchronize()
        xf.copy_(torch.cat(xl))
        for it in range(iters):
            for r in range(nranks):
                steps[r].step(xf, xl[r], ro[r] if it == iters - 1 else None, 0)
            torch.cuda.synchronize()
            xf.copy_(torch.cat(xl))
        got = np.concatenate([ro[r][:lrs[r].rows].cpu().numpy() for r in range(nranks)])
    finally:
        for s in steps:
            s.close()
        c.close()
    np.testing.assert_allclose(got, _want(("dang", shape), csr, True, 0.85, iters), rtol=PR_RTOL, atol=0)


@pytest.mark.gpu
def test_cached_plan_keeps_its_kernel(ctx, monkeypatch):
    """The plan records its kernel: built under GX_PR_KERNEL=adaptive (its own relabelled CSR, no
    sorted tables), it is run by the adaptive kernel again when the next call on the same Graph
    finds the variable unset."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    csr = _small()
    G = A.Graph(ctx, csr, False)
    try:
        monkeypatch.setenv("GX_PR_KERNEL", "adaptive")
        np.testing.assert_allclose(A.LA_PR(G, 0.85, 6), _want("small", csr, False, 0.85, 6), rtol=PR_RTOL, atol=0)
        monkeypatch.delenv("GX_PR_KERNEL")
        np.testing.assert_allclose(A.LA_PR(G, 0.85, 6), _want("small", csr, False, 0.85, 6), rtol=PR_RTOL, atol=0)
        np.testing.assert_allclose(A.LA_PR(G, 0.85, 3), _want("small", csr, False, 0.85, 3), rtol=PR_RTOL, atol=0)
    finally:
        G.close()


@pytest.mark.gpu
@pytest.mark.parametrize("level", ["1", "2"])
def test_plan_times_levels(ctx, monkeypatch, level):
    """GX_PLAN_TIMES=1 (a stream synchronisation at every mark) and 2 (host clock only) change no
    score: gx_pagerank_csr, and gx_pagerank_multi on one device with the block partition (two
    pieces, so that the call is partitioned and not routed to gx_pagerank_csr)."""
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    monkeypatch.setenv("GX_PLAN_TIMES", level)
    csr = _small()
    want = _want("small", csr, False, 0.85, 6)
    np.testing.assert_allclose(A.LA_PR_csr(ctx, csr, False, 0.85, 6), want, rtol=PR_RTOL, atol=0)
    monkeypatch.setenv("GX_PR_MULTI_PARTITION", "blocks")
    monkeypatch.setenv("GX_PR_MULTI_PIECES", "2")
    out = np.zeros(csr.n)
    arr = (C.c_void_p * 1)(ctx.handle.value)
    s = csr.as_c()
    N.check(N.lib().gx_pagerank_multi(arr, 1, C.byref(s), 0, 0.85, 6, N.as_dp(out)), "gx_pagerank_multi")
    np.testing.assert_allclose(out, want, rtol=PR_RTOL, atol=0)


@pytest.mark.gpu
def test_adaptive_plan_without_columns_is_refused(ctx, monkeypatch):
    """A plan laid out for the sorted kernel (pr_multi_plan: a directed graph uploaded whole, its
    entries read through order / perm) holds no columns of its own, so under GX_PR_KERNEL=adaptive
    pr_plan refuses it with GX_NOT_IMPLEMENTED before anything is launched; the context then runs
    the same call without the variable."""
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat
    csr = rmat(10, 8, 3, undirected=False)
    arr = (C.c_void_p * 1)(ctx.handle.value)
    s = csr.as_c()
    out = np.zeros(csr.n)
    monkeypatch.setenv("GX_PR_MULTI_PIECES", "2")
    monkeypatch.setenv("GX_PR_KERNEL", "adaptive")
    assert N.lib().gx_pagerank_multi(arr, 1, C.byref(s), 1, 0.85, 6, N.as_dp(out)) == -101   # GX_NOT_IMPLEMENTED
    assert b"adaptive" in N.lib().gx_last_error()
    monkeypatch.delenv("GX_PR_KERNEL")
    N.check(N.lib().gx_pagerank_multi(arr, 1, C.byref(s), 1, 0.85, 6, N.as_dp(out)), "gx_pagerank_multi")
    np.testing.assert_allclose(out, O.pagerank(csr, True, 0.85, 6), rtol=PR_RTOL, atol=0)
