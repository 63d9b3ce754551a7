"""PageRank's first iteration in closed form (GX_PR_FIRST; PrPart::S, k_pr_first, gx_pr.hip):
S = A (1/outdeg) is built by a plan's first run and every run starts from r1 = t1 + d/n S.  Every
GPU case against the oracle at the parity bar of tests/test_pr_pairs.py."""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (sys.path)
from oracle import oracle as O

PR_RTOL = 1e-12

_CACHE = {}


def _rmat(spec):
    """(csr, directed) of an R-MAT graph (scale, ef, seed, undirected), generated once."""
    if ("g", spec) not in _CACHE:
        from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat
        scale, ef, seed, undirected = spec
        _CACHE[("g", spec)] = (rmat(scale, ef, seed, undirected=undirected), not undirected)
    return _CACHE[("g", spec)]


def _want(key, csr, directed, d, iters):
    """The oracle's scores, computed once per (graph key, damping, iterations)."""
    k = ("r", key, d, iters)
    if k not in _CACHE:
        _CACHE[k] = O.pagerank(csr, directed, d, iters)
    return _CACHE[k]


UNDIR = (12, 16, 11, True)
DIR = (12, 4, 3, False)


@pytest.fixture(scope="module")
def ctx():
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    c = Context(0)
    yield c
    c.close()


def _calls(ctx, key, csr, directed, calls):
    """One resident Graph through (damping, iters) calls in order, each against the oracle."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    G = A.Graph(ctx, csr, directed)
    try:
        for d, iters in calls:
            np.testing.assert_allclose(A.LA_PR(G, d, iters), _want(key, csr, directed, d, iters), rtol=PR_RTOL, atol=0,
                                       err_msg=f"d {d} iters {iters}")
    finally:
        G.close()


def _isolated_graph():
    """40 000 vertices, random edges among the first 20 000 only: half the rows are edgeless, so
    several whole blocks lie past the live prefix (the closed-form isolated blocks)."""
    if "iso" not in _CACHE:
        from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
        rng = np.random.default_rng(7)
        a, b = rng.integers(0, 20000, 120000), rng.integers(0, 20000, 120000)
        keep = a != b
        _CACHE["iso"] = csr_from_edges(40000, a[keep], b[keep], None, symmetric=True)
    return _CACHE["iso"]


def _star_graph():
    """A star (vertex 0 to everyone: one LONG row) on top of an R-MAT graph."""
    if "star" not in _CACHE:
        from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
        csr, _ = _rmat((13, 8, 5, True))
        n = csr.n
        rp = csr.rowptr.astype(np.int64)
        src = np.concatenate([np.repeat(np.arange(n, dtype=np.int64), np.diff(rp)), np.zeros(n - 1, np.int64)])
        dst = np.concatenate([csr.colidx.astype(np.int64), np.arange(1, n, dtype=np.int64)])
        _CACHE["star"] = csr_from_edges(n, src, dst, None, symmetric=True)
    return _CACHE["star"]


def test_directed_input_has_gathered_dangling_rows():
    """The directed graph of the cases below has dangling vertices with in-edges: the sum of
    S = sum over in-neighbours of 1 / outdeg over them (the cached dangling slot) is positive."""
    csr, directed = _rmat(DIR)
    assert directed
    rp = csr.rowptr.astype(np.int64)
    ci = csr.colidx.astype(np.int64)
    deg = np.diff(rp)
    dangling = deg == 0
    assert dangling.any() and (~dangling).any()
    S = np.zeros(csr.n)
    np.add.at(S, ci, np.repeat(1.0 / np.maximum(deg, 1), deg))   # u -> v adds 1 / outdeg(u) to S(v)
    assert S[dangling].sum() > 0.0


def test_closed_form_is_the_first_iteration():
    """r1 = t1 + d/n S and its dangling sum against the plain first iteration, in numpy."""
    csr, _ = _rmat(DIR)
    n = csr.n
    rp = csr.rowptr.astype(np.int64)
    ci = csr.colidx.astype(np.int64)
    deg = np.diff(rp)
    dangling = deg == 0
    S = np.zeros(n)
    np.add.at(S, ci, np.repeat(1.0 / np.maximum(deg, 1), deg))
    for d in (0.85, 0.5):
        nd = int(dangling.sum())
        t1 = (1.0 - d) / n + d / n * (nd / n)
        r1 = t1 + d / n * S
        np.testing.assert_allclose(r1, O.pagerank(csr, True, d, 1), rtol=PR_RTOL, atol=0)
        np.testing.assert_allclose(nd * t1 + d / n * S[dangling].sum(), r1[dangling].sum(), rtol=1e-13)


@pytest.mark.gpu
def test_resident_graph_mixed_calls(ctx):
    """Undirected: S built by the first call, reused under other dampings and iteration counts."""
    csr, directed = _rmat(UNDIR)
    _calls(ctx, UNDIR, csr, directed, [(0.85, 10), (0.85, 1), (0.5, 2), (0.85, 0), (0.6, 10)])


@pytest.mark.gpu
def test_directed_dangling_with_in_edges(ctx):
    """Directed, dangling rows that are gathered: the cached dangling slot is not zero."""
    csr, directed = _rmat(DIR)
    _calls(ctx, DIR, csr, directed, [(0.85, 1), (0.85, 2), (0.85, 3), (0.85, 10)])


@pytest.mark.gpu
@pytest.mark.parametrize("iso", ["1", "0"])
def test_isolated_rows(ctx, monkeypatch, iso):
    """Edgeless rows past the live prefix, with and without their closed form: S mode runs every
    item (S = 0 there), k_pr_first writes their x, the next launch leaves their blocks out."""
    monkeypatch.setenv("GX_PR_ISO_CLOSED", iso)
    csr = _isolated_graph()
    _calls(ctx, "iso", csr, False, [(0.85, 1), (0.85, 4)])


@pytest.mark.gpu
@pytest.mark.parametrize("combine", ["0", "1"])
def test_long_rows_and_multi_unit_blocks(ctx, monkeypatch, combine):
    """A LONG row (the star's centre) beside blocks cut into several units, their slabs added by
    the last arriver or by the combine kernel: S mode goes through each of these paths."""
    monkeypatch.setenv("GX_PR_LONG_NNZ", "1024")
    monkeypatch.setenv("GX_PR_UNIT_NNZ", "8192")
    monkeypatch.setenv("GX_PR_BLOCK_NNZ", "65536")
    monkeypatch.setenv("GX_PR_COMBINE", combine)
    csr = _star_graph()
    _calls(ctx, "star", csr, False, [(0.85, 3), (0.85, 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [UNDIR, DIR], ids=["undirected", "directed"])
def test_adaptive_kernel(ctx, monkeypatch, spec):
    """GX_PR_KERNEL=adaptive: S mode through k_pr_pull and the separate dangling sum."""
    monkeypatch.setenv("GX_PR_KERNEL", "adaptive")
    csr, directed = _rmat(spec)
    _calls(ctx, spec, csr, directed, [(0.85, 1), (0.85, 5)])


@pytest.mark.gpu
@pytest.mark.parametrize("first", ["0", "1"])
@pytest.mark.parametrize("spec", [UNDIR, DIR], ids=["undirected", "directed"])
def test_knob_off_and_on(ctx, monkeypatch, spec, first):
    """GX_PR_FIRST=0 (k_pr_init and a full first iteration) and 1, both within the bar."""
    monkeypatch.setenv("GX_PR_FIRST", first)
    csr, directed = _rmat(spec)
    _calls(ctx, spec, csr, directed, [(0.85, 10), (0.85, 1), (0.85, 10)])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["one", "pair", "edgeless"])
def test_degenerate_graphs(ctx, shape):
    """One vertex; two vertices and one edge; five vertices and no edge."""
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
    e = np.zeros(0, np.int64)
    csr = {"one": lambda: csr_from_edges(1, e, e, None, symmetric=True),
           "pair": lambda: csr_from_edges(2, np.array([0]), np.array([1]), None, symmetric=True),
           "edgeless": lambda: csr_from_edges(5, e, e, None, symmetric=True)}[shape]()
    _calls(ctx, shape, csr, False, [(0.85, 1), (0.85, 3)])


def _device_runs(csr, perm, lrs, use_graph):
    """DevicePageRank without a communicator over the pieces lrs: run(10) twice, run(3) (a
    re-capture), run(1), the scores checked after each."""
    import torch
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    from ldbc_graphalytics_platforms_graphblas_amd.pr_partition import DevicePageRank, GpuStep
    c = Context(0)
    steps = [GpuStep(c, csr.n, len(lrs), lr, 0.85) for lr in lrs]
    dpr = DevicePageRank(steps, None, use_graph=use_graph)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    try:
        for iters in (10, 10, 3, 1):
            dpr.run(iters, stream.cuda_stream)
            got = np.concatenate(dpr.scores([lr.rows for lr in lrs]))[perm]
            np.testing.assert_allclose(got, _want(UNDIR, csr, False, 0.85, iters), rtol=PR_RTOL, atol=0,
                                       err_msg=f"iters {iters}")
    finally:
        dpr.close()
        for s in steps:
            s.close()
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [1, 2, 3])
@pytest.mark.parametrize("use_graph", [True, False])
def test_device_runner_without_comm(pieces, use_graph):
    """gx_pr_dist_run with device copies: S built before the capture, the replayed graph holds
    k_pr_first and iters - 1 iterations; with P pieces S mode goes through their exchange."""
    from ldbc_graphalytics_platforms_graphblas_amd.pr_partition import interleaved_relabel, slice_rows
    csr, _ = _rmat(UNDIR)
    perm, hub, bounds = interleaved_relabel(csr, pieces)
    _device_runs(csr, perm, [slice_rows(hub, bounds, p) for p in range(pieces)], use_graph)


@pytest.mark.gpu
def test_device_runner_block_partition(monkeypatch):
    """The block partition's pieces, each planned as a huge graph (GX_PR_HUGE=1: the combine
    kernel, live prefixes)."""
    from ldbc_graphalytics_platforms_graphblas_amd.pr_partition import block_relabel, slice_rows
    monkeypatch.setenv("GX_PR_HUGE", "1")
    csr, _ = _rmat(UNDIR)
    perm, hub, bounds = block_relabel(csr, 2, rows_per_block=1024, block_nnz=65536)
    _device_runs(csr, perm, [slice_rows(hub, bounds, p) for p in range(2)], True)


@pytest.mark.gpu
def test_kernel_timing_counts(ctx):
    """With kernel timing on, a call on a plan that has its S reports iters - 1 pr_pull launches
    and one pr_first: the second and third calls of test_resident_graph_mixed_calls."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    csr, directed = _rmat(UNDIR)
    G = A.Graph(ctx, csr, directed)
    try:
        A.LA_PR(G, 0.85, 10)
        for d, iters in ((0.85, 1), (0.5, 2)):
            ctx.reset_kernel_stats()
            ctx.set_kernel_timing(True)
            try:
                got = A.LA_PR(G, d, iters)
            finally:
                ctx.set_kernel_timing(False)
            assert ctx.kernel_stats("pr_pull")[0] == iters - 1
            assert ctx.kernel_stats("pr_first")[0] == 1
            np.testing.assert_allclose(got, _want(UNDIR, csr, directed, d, iters), rtol=PR_RTOL, atol=0)
    finally:
        G.close()
