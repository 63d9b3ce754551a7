"""Multi-source BFS (gx_msbfs / LA_MSBFS): 64 traversals per pass, one bit per source.

Row k of the result is what gx_bfs gives from sources[k]; the statistics are (vertices reached, sum
of their levels, largest level) per source.  Everything is an integer and unique, so every
comparison is bit for bit (assert_array_equal); there is no tolerance in this file.

The reference is ref_msbfs below: numpy over the edge arrays, one uint64 word per vertex and batch
of 64 sources, np.bitwise_or.at per level.  On the CPU it is pinned by the oracle's BFS, by scipy's
shortest_path and by a hand-written row.  GPU: fixtures, R-MAT over three calls on one graph with
gx_bfs calls in between, both forms forced, rows in each pull tier (thread / wave / workgroup),
bits that reach one vertex from different neighbours and at different levels, depth past 255, and
the edges of the contract.
"""
import ctypes as C
import functools
import re
import subprocess

import numpy as np
import pytest

from conftest import FIXTURES, ROOT
from oracle import oracle as O
from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges, load_graphalytics, rmat
from test_bfs_parent import edges_of, layered

MAX = np.iinfo(np.int64).max
FIXTURE_NAMES = ["example-directed", "example-undirected", "test-bfs-directed", "test-bfs-undirected"]
ONE = np.uint64(1)


def ref_msbfs(csr, sources):
    """level[ns, n] int64, INT64_MAX = unreached: 64 sources per word, taken in the order given."""
    n = csr.n
    rows, cols = edges_of(csr)
    out = np.full((len(sources), n), MAX, np.int64)
    for off in range(0, len(sources), 64):
        batch = [int(s) for s in sources[off:off + 64]]
        seen = np.zeros(n, np.uint64)
        for k, s in enumerate(batch):
            seen[s] |= ONE << np.uint64(k)
            out[off + k, s] = 0
        front = seen.copy()
        d = 0
        while front.any():
            act = front[rows] != 0
            nxt = np.zeros(n, np.uint64)
            np.bitwise_or.at(nxt, cols[act], front[rows[act]])
            new = nxt & ~seen
            seen |= new
            d += 1
            for k in range(len(batch)):
                out[off + k, ((new >> np.uint64(k)) & ONE) != 0] = d
            front = new
    return out


def ref_stats(level):
    """stats[ns, 3] uint64 from the rows: reached (the source included), sum of levels, largest."""
    reached = level != MAX
    lv = np.where(reached, level, 0)
    return np.stack([reached.sum(axis=1), lv.sum(axis=1), lv.max(axis=1, initial=0)], axis=1).astype(np.uint64)


def random_graph(directed, seed):
    """1 002 vertices, the last one isolated."""
    rng = np.random.default_rng(seed)
    n = 1002
    src, dst = rng.integers(0, n - 1, 2500), rng.integers(0, n - 1, 2500)
    return csr_from_edges(n, src, dst, None, symmetric=not directed)


# ------------------------------------------------------------------------------------- CPU

def test_abi_declares_exports_and_binds_gx_msbfs():
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gx.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+gx_msbfs\s*\(\s*gx_graph\s*\*\s*g\s*,\s*const\s+uint64_t\s*\*\s*sources\s*,"
                     r"\s*uint64_t\s+ns\s*,\s*int64_t\s*\*\s*level\s*,\s*uint64_t\s*\*\s*stats\s*\)", header)
    assert re.search(r"#define\s+GX_MSBFS_BATCH\s+64\b", header)
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True).stdout
    assert "gx_msbfs" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    sig = {name: (res, args) for name, res, args in N.SIGNATURES}
    assert sig["gx_msbfs"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_int64),
                                         C.POINTER(C.c_uint64)])
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    assert callable(A.LA_MSBFS)
    assert A.MSBFS_BATCH == 64


def test_null_graph_is_refused_before_any_device_call():
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    src = np.zeros(1, np.uint64)
    level = np.zeros(1, np.int64)
    stats = np.zeros(3, np.uint64)
    assert N.lib().gx_msbfs(None, N.as_u64p(src), 1, N.as_i64p(level), N.as_u64p(stats)) == -2   # GX_NULL_POINTER
    assert b"gx_msbfs" in N.lib().gx_last_error()


@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_reference_matches_oracle_rows(name):
    csr = load_graphalytics(FIXTURES, name).csr
    got = ref_msbfs(csr, list(range(csr.n)))
    for s in range(csr.n):
        np.testing.assert_array_equal(got[s], O.bfs(csr, s), err_msg=f"source {s}")


@pytest.mark.parametrize("directed", [False, True])
def test_reference_matches_scipy(directed):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse import csgraph
    csr = random_graph(directed, seed=7 + directed)
    n = csr.n
    rng = np.random.default_rng(11)
    sources = [n - 1, 5] + [int(v) for v in rng.integers(0, n, 64)] + [5]   # 67: isolated, a duplicate, two words
    rows, cols = edges_of(csr)
    M = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    dist = csgraph.shortest_path(M, directed=True, unweighted=True, indices=sources)
    got = ref_msbfs(csr, sources)
    assert (got[0] == MAX).sum() == n - 1
    np.testing.assert_array_equal(got[1], got[-1])
    np.testing.assert_array_equal(got == MAX, np.isinf(dist))
    np.testing.assert_array_equal(np.where(got == MAX, -1, got), np.where(np.isinf(dist), -1, dist).astype(np.int64))


def test_reference_matches_hand_written_row():
    """example-directed from vertex 1 (internal index 0): the row tests/test_bfs_parent.py pins."""
    csr = load_graphalytics(FIXTURES, "example-directed").csr
    lev = ref_msbfs(csr, [0])
    np.testing.assert_array_equal(lev, [[0, MAX, 1, 2, 1, MAX, MAX, 2, MAX, 2]])
    np.testing.assert_array_equal(ref_stats(lev), [[6, 8, 2]])


# ------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    c = Context(0)
    yield c
    c.close()


def run_and_check(ctx, csr, directed, sources, want=None, calls=1, bfs_between=False):
    """`calls` LA_MSBFS calls on one graph, each equal to the reference in levels and statistics;
    with bfs_between, gx_bfs calls on the same graph after each (from the second on they run on the
    hub-first copy of an undirected graph) must equal rows of the result."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    if want is None:
        want = ref_msbfs(csr, sources)
    want_stats = ref_stats(want)
    G = A.Graph(ctx, csr, directed)
    try:
        for call in range(calls):
            level, stats = A.LA_MSBFS(G, sources, levels=True, stats=True)
            assert level.dtype == np.int64 and level.shape == (len(sources), csr.n)
            assert stats.dtype == np.uint64 and stats.shape == (len(sources), 3)
            np.testing.assert_array_equal(level, want, err_msg=f"level, call {call + 1}")
            np.testing.assert_array_equal(stats, want_stats, err_msg=f"stats, call {call + 1}")
            if bfs_between:
                for k in (0, min(1, len(sources) - 1)):
                    np.testing.assert_array_equal(A.LA_BFS(G, int(sources[k])), level[k],
                                                  err_msg=f"gx_bfs after call {call + 1}, row {k}")
    finally:
        G.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_gpu_fixtures_every_vertex_a_source(ctx, fixture_graphs, name):
    g = fixture_graphs(name)
    assert 0 < g.csr.n < 64   # ns = n: one partial batch
    run_and_check(ctx, g.csr, g.directed, list(range(g.csr.n)), calls=2, bfs_between=True)


NS = [1, 3, 64, 65, 130]


@functools.lru_cache(maxsize=None)
def rmat_case(directed):
    """The sizes tests/test_bfs_parent.py uses.  130 sources: the hub, vertex 1, a vertex without any
    edge, seeded-random ones, and the hub again; their rows, computed once and read-only."""
    csr = rmat(12, 8, 3, undirected=False) if directed else rmat(14, 16, 4)
    rows, cols = edges_of(csr)
    deg = np.bincount(rows, minlength=csr.n) + np.bincount(cols, minlength=csr.n)
    assert (deg == 0).any()
    hub = int(np.argmax(np.diff(csr.rowptr.astype(np.int64))))
    rng = np.random.default_rng(130)
    full = [hub, 1, int(np.flatnonzero(deg == 0)[0])] + [int(v) for v in rng.integers(0, csr.n, 126)] + [hub]
    want = ref_msbfs(csr, full)
    want.setflags(write=False)
    return csr, full, want


def rmat_sources(directed, ns):
    """The first ns - 1 of the 130 and the duplicate (ns >= 4), else the first ns; and their rows."""
    csr, full, want = rmat_case(directed)
    idx = list(range(ns)) if ns < 4 else list(range(ns - 1)) + [len(full) - 1]
    return csr, [full[i] for i in idx], want[idx]


@pytest.mark.gpu
@pytest.mark.parametrize("ns", NS)
@pytest.mark.parametrize("directed", [False, True])
def test_gpu_rmat_three_calls_with_bfs_between(ctx, directed, ns):
    """On the directed graph the first call builds the transpose; on the undirected one the gx_bfs
    calls in between build the hub-first copy and run on it, which gx_msbfs must not."""
    csr, sources, want = rmat_sources(directed, ns)
    if ns >= 4:
        np.testing.assert_array_equal(want[0], want[-1])   # the duplicate's row
    run_and_check(ctx, csr, directed, sources, want, calls=3, bfs_between=True)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"GX_MSBFS_DIR": "push"}, {"GX_MSBFS_DIR": "pull"}, {"GX_MSBFS_ALPHA": "1"},
                                 {"GX_MSBFS_ALPHA": "1000000"}], ids=["push", "pull", "alpha1", "alpha1e6"])
@pytest.mark.parametrize("directed", [False, True])
def test_gpu_rmat_forced_forms(ctx, monkeypatch, directed, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for ns in NS:
        csr, sources, want = rmat_sources(directed, ns)
        run_and_check(ctx, csr, directed, sources, want, calls=3, bfs_between=True)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "pull"])
@pytest.mark.parametrize("m", [70, 300, 3000])
def test_gpu_fan_in_every_bit_from_its_own_neighbour(ctx, monkeypatch, m, form):
    """u_i -> t for i < m: t's in-row sits in the thread, wave and workgroup tier.  The 64 sources are
    the LAST 64 entries of that row, each the only neighbour that holds its bit: a pull that stops on
    "some bit found", or an OR-reduction that loses a lane, leaves t unreached for some of them."""
    if form == "pull":
        monkeypatch.setenv("GX_MSBFS_DIR", "pull")
    n = m + 2
    perm = np.random.default_rng(m).permutation(n)
    t, us = int(perm[0]), perm[1:m + 1]   # perm[m + 1] stays isolated
    csr = csr_from_edges(n, us, np.full(m, t), None, symmetric=False)
    sources = [int(u) for u in np.sort(us)[-64:]]   # the in-row is sorted by id
    want = ref_msbfs(csr, sources)
    np.testing.assert_array_equal(want[:, t], np.ones(64, np.int64))
    np.testing.assert_array_equal((want != MAX).sum(axis=1), np.full(64, 2))
    run_and_check(ctx, csr, True, sources, want, calls=2)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["undirected", "in", "out"])
def test_gpu_star_rows_in_the_wave_tier(ctx, form):
    """A hub with 1 000 leaves and an isolated vertex (n = 1 002), as tests/test_bfs_parent.py builds it."""
    n, hub = 1002, 500
    leaves = np.array([v for v in range(n - 1) if v != hub])
    hubs = np.full(len(leaves), hub)
    src, dst = (leaves, hubs) if form == "in" else (hubs, leaves)
    csr = csr_from_edges(n, src, dst, None, symmetric=form == "undirected")
    sources = [hub, n - 1] + [int(v) for v in leaves[::16][:62]]
    assert len(sources) == 64
    run_and_check(ctx, csr, form != "undirected", sources, calls=2, bfs_between=True)


@pytest.mark.gpu
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("width,layers", [(70, 6), (40, 4), (300, 3)])
def test_gpu_layers_bits_arrive_at_different_levels(ctx, width, layers, directed):
    """The root and one vertex of each layer as sources: a vertex's bits are set level after level."""
    csr, root = layered(width, layers, directed, seed=width)
    lay = np.random.default_rng(width).permutation(width * layers + 1)[:-1].reshape(layers, width)
    sources = [root] + [int(lay[k][k % width]) for k in range(layers)]
    want = ref_msbfs(csr, sources)
    assert want[0].max() == layers
    run_and_check(ctx, csr, directed, sources, want, calls=2, bfs_between=True)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "pull"])
def test_gpu_deep_path_levels_past_255(ctx, monkeypatch, form):
    """A 3 000-vertex path plus an isolated vertex; levels are int32 on the device, so depth is
    bounded by n alone."""
    if form == "pull":
        monkeypatch.setenv("GX_MSBFS_DIR", "pull")
    n = 3000
    perm = np.random.default_rng(2).permutation(n)
    csr = csr_from_edges(n + 1, perm[:-1], perm[1:], None, symmetric=True)   # vertex n isolated
    sources = [int(perm[0]), int(perm[-1]), int(perm[n // 2]), n]
    want = ref_msbfs(csr, sources)
    assert want[0][:n].max() == n - 1 and want[0][n] == MAX and (want[3] != MAX).sum() == 1
    run_and_check(ctx, csr, False, sources, want)


@pytest.mark.gpu
@pytest.mark.parametrize("directed", [False, True])
def test_gpu_single_vertex(ctx, directed):
    csr = csr_from_edges(1, [], [], None, symmetric=not directed)
    run_and_check(ctx, csr, directed, [0, 0], want=np.zeros((2, 1), np.int64), calls=2, bfs_between=True)


@pytest.mark.gpu
def test_gpu_contract_edges(ctx, fixture_graphs):
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    g = fixture_graphs("example-undirected")
    n = g.csr.n
    G = A.Graph(ctx, g.csr, g.directed)
    try:
        level = np.full((2, n), -7, np.int64)
        stats = np.full((2, 3), 77, np.uint64)
        src = np.array([0, 1], np.uint64)
        # ns == 0: success, nothing written (with and without a sources pointer)
        assert N.lib().gx_msbfs(G.handle, N.as_u64p(src), 0, N.as_i64p(level), N.as_u64p(stats)) == 0
        assert N.lib().gx_msbfs(G.handle, None, 0, N.as_i64p(level), N.as_u64p(stats)) == 0
        assert (level == -7).all() and (stats == 77).all()
        assert A.LA_MSBFS(G, [], levels=True, stats=True)[0].shape == (0, n)
        # a source >= n: GX_INVALID_INDEX, nothing written
        bad = np.array([0, n], np.uint64)
        assert N.lib().gx_msbfs(G.handle, N.as_u64p(bad), 2, N.as_i64p(level), N.as_u64p(stats)) == -4
        assert b"gx_msbfs" in N.lib().gx_last_error()
        assert (level == -7).all() and (stats == 77).all()
        # nothing to write to, or no sources to read: GX_NULL_POINTER
        assert N.lib().gx_msbfs(G.handle, N.as_u64p(src), 2, None, None) == -2
        assert b"gx_msbfs" in N.lib().gx_last_error()
        assert N.lib().gx_msbfs(G.handle, None, 2, N.as_i64p(level), N.as_u64p(stats)) == -2
        assert (level == -7).all() and (stats == 77).all()
        with pytest.raises(N.GxError) as err:
            A.LA_MSBFS(G, [0, 1], levels=False, stats=False)
        assert err.value.code == -2
        # each output alone equals its half of the full call
        sources = list(range(n))
        full_level, full_stats = A.LA_MSBFS(G, sources, levels=True, stats=True)
        np.testing.assert_array_equal(A.LA_MSBFS(G, sources, levels=False, stats=True), full_stats)
        np.testing.assert_array_equal(A.LA_MSBFS(G, sources), full_level)
        np.testing.assert_array_equal(full_stats, ref_stats(ref_msbfs(g.csr, sources)))
    finally:
        G.close()
