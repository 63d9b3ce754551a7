"""Betweenness centrality (gx_betweenness / LA_BC): batched Brandes over a handful of sources.

The reference is ref_bc below, numpy over the edge arrays: levels, then path counts level by
level, then dependencies back up.  On the CPU it is pinned by hand-written values and by networkx.

Comparison rule.  `paths` (sigma) holds integers below 2^53 and is compared bit for bit.
`centrality` is compared with atol = 0 and rtol = 2 * ((Dmax + 3) * (L + 1) + ns) * 2^-53, Dmax the
largest row length (in- or out-) and L the deepest level reached: every term is positive, one
level adds at most k + 2 roundings to a k-term row, the batch sum ns - 1, and the reference and the
device each get that bound.  Entries the reference gives as 0 must be 0.  Two calls on one graph
must be bit-equal: no floating-point atomics, every sum in a fixed order.
"""
import ctypes as C
import functools
import re
import subprocess

import numpy as np
import pytest

from conftest import FIXTURES, ROOT
from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges, load_graphalytics, rmat

MAX = np.iinfo(np.int64).max
FIXTURE_NAMES = ["example-directed", "example-undirected", "test-bfs-directed", "test-bfs-undirected"]


def edges_of(csr):
    rows = np.repeat(np.arange(csr.n, dtype=np.int64), np.diff(csr.rowptr.astype(np.int64)))
    return rows, csr.colidx.astype(np.int64)


def ref_levels(csr, s):
    """Hop levels over out-edges, -1 = unreached."""
    rows, cols = edges_of(csr)
    lev = np.full(csr.n, -1, np.int64)
    lev[s] = 0
    d = 0
    while True:
        hit = cols[(lev[rows] == d) & (lev[cols] < 0)]
        if len(hit) == 0:
            return lev
        lev[hit] = d + 1
        d += 1


def ref_bc(csr, sources):
    """(centrality[n], paths[ns, n]) as include/gx.h defines gx_betweenness."""
    n = csr.n
    rows, cols = edges_of(csr)
    cent = np.zeros(n)
    paths = np.zeros((len(sources), n))
    for k, s in enumerate(sources):
        lev = ref_levels(csr, s)
        down = lev[cols] == lev[rows] + 1
        down &= lev[rows] >= 0
        r, c = rows[down], cols[down]
        order = np.argsort(lev[r], kind="stable")
        r, c = r[order], c[order]
        cut = np.searchsorted(lev[r], np.arange(lev.max() + 2))   # edges leaving level d: cut[d]:cut[d+1]
        sigma = np.zeros(n)
        sigma[s] = 1.0
        for d in range(lev.max()):
            e = slice(cut[d], cut[d + 1])
            np.add.at(sigma, c[e], sigma[r[e]])
        delta = np.zeros(n)
        for d in range(lev.max() - 1, -1, -1):
            e = slice(cut[d], cut[d + 1])
            np.add.at(delta, r[e], sigma[r[e]] / sigma[c[e]] * (1.0 + delta[c[e]]))
        delta[s] = 0.0
        cent += delta
        paths[k] = sigma
    return cent, paths


def rtol_for(csr, sources):
    rows, cols = edges_of(csr)
    dmax = int(max(np.bincount(rows, minlength=csr.n).max(), np.bincount(cols, minlength=csr.n).max())) \
        if len(rows) else 0
    depth = max([int(ref_levels(csr, s).max()) for s in sources], default=0)
    return 2.0 * ((dmax + 3) * (depth + 1) + len(sources)) * 2.0 ** -53


def compare(csr, sources, got, want, what=""):
    cent, paths = got
    want_cent, want_paths = want
    assert cent.dtype == np.float64 and paths.dtype == np.float64
    assert paths.shape == (len(sources), csr.n)
    if paths.size:
        assert want_paths.max() < 2 ** 53 and paths.max() < 2 ** 53
    np.testing.assert_array_equal(paths, want_paths, err_msg="paths " + what)
    np.testing.assert_allclose(cent, want_cent, rtol=rtol_for(csr, sources), atol=0, err_msg="centrality " + what)


# ------------------------------------------------------------------------------------- CPU

def test_abi_declares_exports_and_binds_gx_betweenness():
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gx.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+gx_betweenness\s*\(\s*gx_graph\s*\*\s*g\s*,\s*const\s+uint64_t\s*\*\s*sources\s*,"
                     r"\s*uint64_t\s+ns\s*,\s*double\s*\*\s*centrality\s*,\s*double\s*\*\s*paths\s*\)", header)
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True).stdout
    assert "gx_betweenness" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    sig = {name: (res, args) for name, res, args in N.SIGNATURES}
    assert sig["gx_betweenness"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64,
                                               C.POINTER(C.c_double), C.POINTER(C.c_double)])
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    assert callable(A.LA_BC)
    assert 0 < A.BC_SHORT < A.BC_LONG


def test_null_graph_is_refused_before_any_device_call():
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    src = np.zeros(1, np.uint64)
    cent = np.zeros(1)
    assert N.lib().gx_betweenness(None, N.as_u64p(src), 1, N.as_dp(cent), None) == -2   # GX_NULL_POINTER
    assert b"gx_betweenness" in N.lib().gx_last_error()


def test_reference_matches_hand_written_values():
    path = csr_from_edges(3, [0, 1], [1, 2], None, symmetric=True)
    cent, paths = ref_bc(path, [0, 1, 2])
    np.testing.assert_array_equal(cent, [0, 2, 0])
    np.testing.assert_array_equal(paths, np.ones((3, 3)))
    diamond = csr_from_edges(4, [0, 0, 1, 2], [1, 2, 3, 3], None, symmetric=False)
    cent, paths = ref_bc(diamond, [0])
    np.testing.assert_array_equal(paths, [[1, 1, 1, 2]])
    np.testing.assert_array_equal(cent, [0, .5, .5, 0])
    cent, paths = ref_bc(diamond, [3])   # nothing reachable
    np.testing.assert_array_equal(paths, [[0, 0, 0, 1]])
    np.testing.assert_array_equal(cent, np.zeros(4))


@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_reference_matches_networkx(name):
    nx = pytest.importorskip("networkx")
    g = load_graphalytics(FIXTURES, name)
    csr, n = g.csr, g.csr.n
    rows, cols = edges_of(csr)
    H = nx.DiGraph() if g.directed else nx.Graph()
    H.add_nodes_from(range(n))
    H.add_edges_from(zip(rows.tolist(), cols.tolist()))
    scale = 1.0 if g.directed else 2.0
    want = nx.betweenness_centrality(H, normalized=False)
    cent, _ = ref_bc(csr, list(range(n)))
    np.testing.assert_allclose(cent, scale * np.array([want[v] for v in range(n)]), rtol=1e-12, atol=0)
    sub = [0, n - 1]
    want = nx.betweenness_centrality_subset(H, sub, list(range(n)), normalized=False)
    cent, _ = ref_bc(csr, sub)
    np.testing.assert_allclose(cent, scale * np.array([want[v] for v in range(n)]), rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    c = Context(0)
    yield c
    c.close()


def run_and_check(ctx, csr, directed, sources, ref=None, G=None):
    """Two LA_BC calls on one graph: each equal to the reference by the rule above, and the two
    bit-equal to each other.  Returns the first result."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    want = ref if ref is not None else ref_bc(csr, sources)
    own = G is None
    if own:
        G = A.Graph(ctx, csr, directed)
    try:
        first = A.LA_BC(G, sources, return_paths=True)
        second = A.LA_BC(G, sources, return_paths=True)
        compare(csr, sources, first, want, "call 1")
        compare(csr, sources, second, want, "call 2")
        np.testing.assert_array_equal(first[0], second[0], err_msg="centrality differs between two calls")
        np.testing.assert_array_equal(first[1], second[1], err_msg="paths differ between two calls")
        np.testing.assert_array_equal(A.LA_BC(G, sources), first[0], err_msg="without paths")
    finally:
        if own:
            G.close()
    return first


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_gpu_fixtures_every_vertex_a_source(ctx, fixture_graphs, name):
    g = fixture_graphs(name)
    assert g.csr.n <= 10
    run_and_check(ctx, g.csr, g.directed, list(range(g.csr.n)))


@functools.lru_cache(maxsize=None)
def rmat_case(directed):
    """The sizes tests/test_bfs_parent.py runs on; sources with a repeat; the reference."""
    csr = rmat(12, 8, 3, undirected=False) if directed else rmat(14, 16, 4)
    hub = int(np.argmax(np.diff(csr.rowptr.astype(np.int64))))
    srcs = (hub, 1, hub, csr.n - 1)
    return csr, srcs, ref_bc(csr, srcs)


@pytest.mark.gpu
@pytest.mark.parametrize("directed", [False, True])
def test_gpu_rmat_batch_with_a_repeat(ctx, directed):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    csr, srcs, ref = rmat_case(directed)
    G = A.Graph(ctx, csr, directed)
    try:
        run_and_check(ctx, csr, directed, srcs, ref=ref, G=G)
        a, b = srcs[0], srcs[1]
        both, one, other = A.LA_BC(G, [a, b]), A.LA_BC(G, [a]), A.LA_BC(G, [b])
        np.testing.assert_allclose(both, one + other, rtol=rtol_for(csr, [a, b]), atol=0)
        twice = A.LA_BC(G, [a, a])
        np.testing.assert_array_equal(twice, one + one)
    finally:
        G.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"GX_BFS_ALPHA": "1", "GX_BFS_BETA": "1000"},
                                 {"GX_BFS_ALPHA": "1000", "GX_BFS_BETA": "1"},
                                 {"GX_BFS_DEVICE": "0"}, {"GX_BFS_TRANSPOSE": "0"}])
def test_gpu_result_does_not_depend_on_the_traversal(ctx, monkeypatch, env):
    """Levels are unique, so top-down or bottom-up, host- or device-driven, the sums are the same
    bit for bit as the default run's."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    for directed in (False, True):
        csr, srcs, ref = rmat_case(directed)
        G = A.Graph(ctx, csr, directed)
        try:
            default = A.LA_BC(G, srcs, return_paths=True)
        finally:
            G.close()
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            got = run_and_check(ctx, csr, directed, srcs, ref=ref)
        np.testing.assert_array_equal(got[0], default[0])
        np.testing.assert_array_equal(got[1], default[1])


def layered(width, layers, directed, seed):
    """`layers` layers of `width` vertices under a random id permutation, consecutive layers
    completely connected, and a source joined to layer 0 (as in test_bfs_parent.py): sigma at
    layer k is width^k."""
    n = width * layers + 1
    perm = np.random.default_rng(seed).permutation(n)
    lay = perm[:-1].reshape(layers, width)
    src = [np.full(width, perm[-1])] + [np.repeat(lay[k], width) for k in range(layers - 1)]
    dst = [lay[0]] + [np.tile(lay[k + 1], width) for k in range(layers - 1)]
    return csr_from_edges(n, np.concatenate(src), np.concatenate(dst), None, symmetric=not directed), \
        int(perm[-1]), lay


@pytest.mark.gpu
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("width,layers", [(70, 6), (40, 4), (300, 3)])
def test_gpu_layered_path_counts_are_powers(ctx, width, layers, directed):
    csr, s, lay = layered(width, layers, directed, seed=width)
    ref = ref_bc(csr, [s])
    for k in range(layers):
        np.testing.assert_array_equal(ref[1][0][lay[k]], float(width) ** k)
    assert np.any(ref[0] != np.floor(ref[0]))   # fractional dependencies
    run_and_check(ctx, csr, directed, [s], ref=ref)


def tier_graph(lens, mirror, seed):
    """Directed.  mirror = False: source -> a_k, a_k -> the first lens[k] of a second layer, so a_k's
    out-row (the delta pull) has exactly lens[k] entries.  mirror = True: source -> every b_j,
    the first lens[k] b_j -> a_k, a_k -> a sink, so a_k's in-row (the sigma pull) has lens[k]."""
    m, width = len(lens), max(lens)
    n = 1 + m + width + 1
    perm = np.random.default_rng(seed).permutation(n)
    s, sink = perm[0], perm[-1]
    a, b = perm[1:1 + m], perm[1 + m:1 + m + width]
    fan_a = np.concatenate([np.full(l, a[k]) for k, l in enumerate(lens)])
    fan_b = np.concatenate([b[:l] for l in lens])
    if mirror:
        src = np.concatenate([np.full(width, s), fan_b, a])
        dst = np.concatenate([b, fan_a, np.full(m, sink)])
    else:
        src = np.concatenate([np.full(m, s), fan_a, b[:1]])
        dst = np.concatenate([a, fan_b, [sink]])
    return csr_from_edges(n, src, dst, None, symmetric=False), int(s), a


@pytest.mark.gpu
@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("env", [{}, {"GX_BC_SHORT": "0"}])
def test_gpu_rows_around_the_tier_thresholds(ctx, monkeypatch, mirror, env):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    lens = sorted({1, 2, 63, 64, 65} | {t + d for t in (A.BC_SHORT, A.BC_LONG) for d in (-1, 0, 1)})
    csr, s, a = tier_graph(lens, mirror, seed=11)
    row = np.bincount(edges_of(csr)[1 if mirror else 0], minlength=csr.n)
    np.testing.assert_array_equal(row[a], lens)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cent, paths = run_and_check(ctx, csr, True, [s])
    if mirror:
        np.testing.assert_array_equal(paths[0][a], lens)   # one path through each b_j that points at a_k
    else:
        assert (cent[a] > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("bits", ["0", "-1"])
def test_gpu_bitmap_and_level_probes_agree(ctx, monkeypatch, bits):
    """GX_BC_BITS = 0: every bucket probes a level bitmap; -1: none does (the default: buckets of
    1 024 rows and more).  The same edges in the same order, so the same bits as the default run."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    cases = [(rmat_case(d)[0], d, list(rmat_case(d)[1]), rmat_case(d)[2]) for d in (False, True)]
    for directed in (False, True):
        csr, s, _ = layered(70, 6, directed, seed=70)
        cases.append((csr, directed, [s], None))
    for mirror in (False, True):
        lens = sorted({1, 65} | {t + d for t in (A.BC_SHORT, A.BC_LONG) for d in (0, 1)})
        csr, s, _ = tier_graph(lens, mirror, seed=12)
        cases.append((csr, True, [s], None))
    for csr, directed, srcs, ref in cases:
        G = A.Graph(ctx, csr, directed)
        try:
            default = A.LA_BC(G, srcs, return_paths=True)
        finally:
            G.close()
        with monkeypatch.context() as m:
            m.setenv("GX_BC_BITS", bits)
            got = run_and_check(ctx, csr, directed, srcs, ref=ref)
        np.testing.assert_array_equal(got[0], default[0])
        np.testing.assert_array_equal(got[1], default[1])


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["undirected", "in", "out"])
def test_gpu_star(ctx, form):
    """test_bfs_parent's star: a hub with 1 000 leaves and an isolated vertex, n = 1 002."""
    n, hub = 1002, 500
    leaves = np.array([v for v in range(n - 1) if v != hub])
    hubs = np.full(len(leaves), hub)
    src, dst = (leaves, hubs) if form == "in" else (hubs, leaves)
    csr = csr_from_edges(n, src, dst, None, symmetric=form == "undirected")
    for s in (hub, 7, n - 1):
        cent, paths = run_and_check(ctx, csr, form != "undirected", [s])
        if s == n - 1:
            np.testing.assert_array_equal(cent, np.zeros(n))
            np.testing.assert_array_equal(paths[0], np.eye(n)[s])
        if s == 7 and form == "undirected":
            assert cent[hub] == 999.0
    run_and_check(ctx, csr, form != "undirected", [hub, 7, n - 1])


@pytest.mark.gpu
def test_gpu_grid_many_equal_paths(ctx):
    side = 20
    idx = np.arange(side * side).reshape(side, side)
    src = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    dst = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    csr = csr_from_edges(side * side, src, dst, None, symmetric=True)
    corner, centre = 0, int(idx[side // 2, side // 2])
    ref = ref_bc(csr, [corner, centre])
    assert ref[1][0].max() == 35345263800.0   # C(38, 19)
    run_and_check(ctx, csr, False, [corner, centre], ref=ref)


@pytest.mark.gpu
def test_gpu_deep_path(ctx):
    """test_bfs_parent's 3 000-vertex path under a permutation plus an isolated vertex: 3 000 level
    buckets from an end, and the launch loop over them."""
    n = 3000
    perm = np.random.default_rng(2).permutation(n)
    csr = csr_from_edges(n + 1, perm[:-1], perm[1:], None, symmetric=True)
    end, mid = int(perm[0]), int(perm[n // 2])
    cent, paths = run_and_check(ctx, csr, False, [end, mid])
    assert paths[0].max() == 1.0 and paths[0][n] == 0.0 and cent[n] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("directed", [False, True])
def test_gpu_edge_cases(ctx, directed):
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    one = csr_from_edges(1, [], [], None, symmetric=not directed)
    cent, paths = run_and_check(ctx, one, directed, [0])
    assert cent[0] == 0.0 and paths[0][0] == 1.0
    g = load_graphalytics(FIXTURES, "example-directed" if directed else "example-undirected")
    csr, n = g.csr, g.csr.n
    G = A.Graph(ctx, csr, directed)
    try:
        cent, paths = A.LA_BC(G, [], return_paths=True)
        np.testing.assert_array_equal(cent, np.zeros(n))
        assert paths.shape == (0, n)
        with pytest.raises(N.GxError) as err:
            A.LA_BC(G, [0, n])
        assert err.value.code == -4   # GX_INVALID_INDEX
        src = np.array([0, n], np.uint64)
        cent, paths = np.full(n, 7.5), np.full((2, n), -3.25)
        assert N.lib().gx_betweenness(G.handle, N.as_u64p(src), 2, N.as_dp(cent), N.as_dp(paths)) == -4
        assert (cent == 7.5).all() and (paths == -3.25).all()
        run_and_check(ctx, csr, directed, [0, n - 1], G=G)
    finally:
        G.close()


@pytest.mark.gpu
@pytest.mark.parametrize("directed", [True, False])
def test_gpu_interleaved_with_bfs_on_one_graph(ctx, directed):
    """Directed: the BFS calls build and use the transpose.  Undirected: from its second BFS call the
    graph has a hub-first copy, which gx_bfs runs on and gx_betweenness must not."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    csr, srcs, ref = rmat_case(directed)
    s = srcs[0]
    lev = ref_levels(csr, s)
    rows, cols = edges_of(csr)
    ok = (lev[rows] >= 0) & (lev[cols] == lev[rows] + 1)
    par = np.full(csr.n, MAX)
    np.minimum.at(par, cols[ok], rows[ok])
    par[lev < 0] = -1
    par[s] = s
    want_level = np.where(lev < 0, MAX, lev)
    G = A.Graph(ctx, csr, directed)
    try:
        np.testing.assert_array_equal(A.LA_BFS(G, s), want_level)
        bc1 = A.LA_BC(G, srcs, return_paths=True)
        level, parent = A.LA_BFS_parent(G, s)
        np.testing.assert_array_equal(level, want_level)
        np.testing.assert_array_equal(parent, par)
        bc2 = A.LA_BC(G, srcs, return_paths=True)
        np.testing.assert_array_equal(A.LA_BFS(G, s), want_level)
        compare(csr, srcs, bc1, ref, "first")
        compare(csr, srcs, bc2, ref, "second")
        np.testing.assert_array_equal(bc1[0], bc2[0])
        np.testing.assert_array_equal(bc1[1], bc2[1])
    finally:
        G.close()


@pytest.mark.gpu
def test_gpu_kernel_stats_name_the_passes(ctx):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    csr, srcs, _ = rmat_case(True)
    G = A.Graph(ctx, csr, True)
    try:
        ctx.set_kernel_timing(True)
        ctx.reset_kernel_stats()
        A.LA_BC(G, srcs[:1])
        for name in ("bc_bucket", "bc_sigma", "bc_delta"):
            launches, _ = ctx.kernel_stats(name)
            assert launches > 0, name
    finally:
        ctx.set_kernel_timing(False)
        G.close()
