"""SSSP on the 1-D split (gx_sssp_split.hip, config 4's partition) against the oracle.

GPU: one rank owning every vertex (gx_sssp_split_run, rounds on the device) and 2-5 ranks
simulated on one device through the lock-step driver (distributed.sssp with LocalComm: the
pairs all-gather is a concatenation) -- bit-exact distances, whatever the bucket width.
The gloo world-2 run of the same driver is in test_distributed_algs.py.
"""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (sys.path)
from ldbc_graphalytics_platforms_graphblas_amd import distributed as D
from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges, rmat
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    c = Context(0)
    yield c
    c.close()


def _src(csr):
    return int(np.argmax(np.diff(csr.rowptr.astype(np.int64))))


GRAPHS = [(10, 8, 1, True), (13, 16, 2, True), (12, 8, 3, False), (14, 6, 4, False)]


ENVS = [{}, {"GX_SSSP_DSCALE": "0.25"}, {"GX_SSSP_DSCALE": "40"}, {"GX_SSSP_PULL": "2"}, {"GX_SSSP_PULL": "0"},
        {"GX_SSSP_FUSE": "1"}, {"GX_SSSP_FUSE": "1", "GX_SSSP_DSCALE": "0.05"},
        {"GX_SSSP_FUSE": "0"}]   # the split clamps 0 to 1 (gx_sssp.h SsspKnobs::fuse)


@pytest.mark.parametrize("scale,ef,seed,und", GRAPHS)
@pytest.mark.parametrize("env", ENVS)
def test_split_run_one_rank(ctx, monkeypatch, scale, ef, seed, und, env):
    """Every schedule: bucket widths (0.05 x the default puts most vertices past the 32-bucket
    ring window, through the overflow), pulled / pushed heavy phases, no bucket fusion."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    csr = rmat(scale, ef, seed, undirected=und, weighted=True)
    G = A.Graph(ctx, csr, not und)
    sp = A.SsspSplit(G)
    try:
        for src in (_src(csr), 0):
            assert np.array_equal(sp.run(src), O.sssp(csr, src))
    finally:
        sp.close()
        G.close()


def test_split_run_verbose(ctx, monkeypatch, capfd):
    """GX_SPLIT_VERBOSE=1: the run reports its rounds per mode and the mode log on stderr."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    monkeypatch.setenv("GX_SPLIT_VERBOSE", "1")
    csr = rmat(10, 8, 1, undirected=True, weighted=True)
    G = A.Graph(ctx, csr, False)
    sp = A.SsspSplit(G)
    try:
        capfd.readouterr()
        assert np.array_equal(sp.run(_src(csr)), O.sssp(csr, _src(csr)))
        assert "[gx_sssp_split] modes:" in capfd.readouterr().err
    finally:
        sp.close()
        G.close()


def _split_delta(sp):
    import ctypes as C
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    d = C.c_double(0.0)
    N.check(N.lib().gx_sssp_split_delta(sp.h, C.byref(d)), "gx_sssp_split_delta")
    return np.float64(d.value).view(np.uint64)


@pytest.mark.parametrize("split_first", [False, True])
@pytest.mark.parametrize("spec,und", [((10, 8, 1), True), ((10, 6, 3), False)])
def test_split_and_gx_sssp_share_graph_stats(ctx, spec, und, split_first):
    """gx_sssp and the split on one resident graph, in both orders: whichever runs first fills the
    graph's cached mean weight and non-isolated count, and both give the oracle's distances.  Two
    splits made on one graph get the same bucket width bit for bit."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    csr = rmat(*spec, undirected=und, weighted=True)
    src = _src(csr)
    want = O.sssp(csr, src)
    G = A.Graph(ctx, csr, not und)
    sps = []
    try:
        if not split_first:
            assert np.array_equal(A.LA_SSSP(G, src), want)
        sps += [A.SsspSplit(G), A.SsspSplit(G)]
        assert _split_delta(sps[0]) == _split_delta(sps[1])
        assert np.array_equal(sps[0].run(src), want)
        for _ in range(2):   # on the graph itself, then (undirected) on its hub-first copy
            assert np.array_equal(A.LA_SSSP(G, src), want)
        assert np.array_equal(sps[1].run(src), want)
        assert _split_delta(sps[0]) == _split_delta(sps[1])   # both rebuilt on the same copy
    finally:
        for sp in sps:
            sp.close()
        G.close()


def test_split_run_unreachable_and_isolated(ctx):
    """Two components, isolated vertices and a source without edges."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    rng = np.random.default_rng(5)
    n = 3000
    a, b = rng.integers(0, 1000, 6000), rng.integers(0, 1000, 6000)
    c, d = rng.integers(1500, 2500, 4000), rng.integers(1500, 2500, 4000)
    src = np.concatenate([a, c])
    dst = np.concatenate([b, d])
    keep = src != dst
    w = rng.random(int(keep.sum())) * 3.0
    csr = csr_from_edges(n, src[keep], dst[keep], w, symmetric=True)
    G = A.Graph(ctx, csr, False)
    sp = A.SsspSplit(G)
    try:
        for s in (int(src[0]), 1200, int(c[0])):
            assert np.array_equal(sp.run(s), O.sssp(csr, s))
    finally:
        sp.close()
        G.close()


@pytest.mark.parametrize("nranks,env", [(2, {}), (4, {}), (5, {}), (3, {"GX_SSSP_PULL": "2"}),
                                        (3, {"GX_SSSP_FUSE": "1", "GX_SSSP_DSCALE": "0.05"})])
def test_split_simulated_ranks(ctx, monkeypatch, nranks, env):
    """The per-round protocol with 2, 4 and 5 ranks on one device (rank ranges balanced by
    entries), also with an always-pulled heavy phase and through the overflow."""
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Graph
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dev = torch.device("cuda", 0)
    for csr, directed in [(rmat(13, 8, 31, undirected=True, weighted=True), False),
                          (rmat(12, 6, 32, undirected=False, weighted=True), True)]:
        g = Graph(ctx, csr, directed)
        try:
            be = D.GpuBackend(g)
            rng = D.vertex_ranges(csr.rowptr, nranks)
            ranks = [D.LocalRank(be, int(rng[k]), int(rng[k + 1]), dev, k) for k in range(nranks)]
            src = _src(csr)
            got = D.sssp(ranks, D.LocalComm(), csr.n, src).cpu().numpy()
            assert np.array_equal(got, O.sssp(csr, src))
        finally:
            g.close()


def test_split_empty_rank(ctx):
    """A rank owning no vertex still takes part in every round."""
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Graph
    dev = torch.device("cuda", 0)
    csr = rmat(11, 8, 33, undirected=True, weighted=True)
    g = Graph(ctx, csr, False)
    try:
        be = D.GpuBackend(g)
        n = csr.n
        bounds = [0, n // 3, n // 3, n]
        ranks = [D.LocalRank(be, bounds[k], bounds[k + 1], dev, k) for k in range(3)]
        src = _src(csr)
        assert np.array_equal(D.sssp(ranks, D.LocalComm(), n, src).cpu().numpy(), O.sssp(csr, src))
    finally:
        g.close()
