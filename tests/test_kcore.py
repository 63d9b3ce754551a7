"""k-core and core numbers (gx_kcore / LA_KCore, gx_core_all / LA_CoreAll).

An edge is an unordered pair {i, j}, i != j, of an undirected graph stored in both directions; the
k-core is the largest subgraph whose every vertex has at least k neighbours inside it.  degree is one
int64 per vertex (its neighbours inside the k-core, -1 when it is not in it), stats = (vertices, edges,
rounds of synchronous pruning that removed a vertex), core = the largest k whose k-core holds the
vertex (0 without an edge).  Everything is an integer and unique, so every comparison is bit for bit
(assert_array_equal); there is no tolerance in this file.

The reference is ref_kcore below: a numpy synchronous peel, diagonal entries dropped first, every
round removing all alive vertices with deg < k and subtracting a bincount of the dead-to-alive
entries.  On the CPU it is pinned by networkx.core_number / k_core and by hand-checked graphs (K6, a
triangulated torus, the same torus with one edge cut, whose 6-core unravels in 16 rounds, and a
4 096-vertex path that loses two vertices per round).  GPU: the Graphalytics fixtures, R-MAT with
other algorithms' calls in between, the long cascades under every way of scheduling the rounds, 3 000
leaves decrementing the same two hubs in one round, every row tier on a dying hub, diagonal entries,
unsorted rows and the edges of the contract.
"""
import ctypes as C
import functools
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from ldbc_graphalytics_platforms_graphblas_amd.graphio import CSR, csr_from_edges, rmat

UNDIRECTED_FIXTURES = ["example-undirected", "test-bfs-undirected", "test-cdlp-undirected", "test-lcc-undirected",
                       "test-pr-undirected", "test-sssp-undirected", "test-wcc-undirected"]


def edges_of(csr):
    rows = np.repeat(np.arange(csr.n, dtype=np.int64), np.diff(csr.rowptr.astype(np.int64)))
    return rows, csr.colidx.astype(np.int64)


def peel_to(k, rows, cols, deg, alive, core=None):
    """Synchronous rounds toward k on (deg, alive), in place; the rounds that removed a vertex."""
    rounds = 0
    while True:
        die = alive & (deg < k)
        if not die.any():
            return rounds
        alive &= ~die
        if core is not None:
            core[die] = k - 1
        hit = die[rows] & alive[cols]   # the dead-to-alive entries
        deg -= np.bincount(cols[hit], minlength=len(deg))
        rounds += 1


def start_of(csr):
    rows, cols = edges_of(csr)
    off = rows != cols
    rows, cols = rows[off], cols[off]
    return rows, cols, np.bincount(rows, minlength=csr.n).astype(np.int64), np.ones(csr.n, bool)


def ref_kcore(csr, k):
    """(degree[n] int64, stats[3] uint64) of the k-core."""
    rows, cols, deg, alive = start_of(csr)
    rounds = peel_to(k, rows, cols, deg, alive)
    assert deg[alive].sum() % 2 == 0
    stats = np.array([alive.sum(), deg[alive].sum() // 2, rounds], np.uint64)
    return np.where(alive, deg, -1), stats


def ref_core_all(csr):
    """(core[n] int64, kmax)."""
    rows, cols, deg, alive = start_of(csr)
    core = np.zeros(csr.n, np.int64)
    k = 1
    while alive.any():
        peel_to(k, rows, cols, deg, alive, core)
        k += 1
    return core, int(core.max(initial=0))


def ref_every_k(csr):
    """(core, kmax, {k: (degree, stats)} for k = 0 .. kmax + 1), computed once and read-only."""
    core, kmax = ref_core_all(csr)
    per_k = {k: ref_kcore(csr, k) for k in range(kmax + 2)}
    for k, (deg, st) in per_k.items():
        np.testing.assert_array_equal(deg >= 0, core >= k)   # the reference's two halves agree
        deg.setflags(write=False)
        st.setflags(write=False)
    core.setflags(write=False)
    return core, kmax, per_k


def clique(m, first=0):
    ids = np.arange(first, first + m)
    i, j = np.meshgrid(ids, ids, indexing="ij")
    keep = i < j
    return i[keep], j[keep]


def torus(a, b, cut=False):
    """Triangulated a x b torus: (x, y) joined to (x+1, y), (x, y+1), (x+1, y+1) mod a, b; vertex
    x * b + y.  cut: without the edge (0,0)-(1,0)."""
    x, y = np.meshgrid(np.arange(a), np.arange(b), indexing="ij")
    x, y = x.ravel(), y.ravel()
    v = x * b + y
    src = np.concatenate([v, v, v])
    dst = np.concatenate([((x + 1) % a) * b + y, x * b + (y + 1) % b, ((x + 1) % a) * b + (y + 1) % b])
    if cut:
        keep = ~((src == 0) & (dst == b))
        assert keep.sum() == len(src) - 1
        src, dst = src[keep], dst[keep]
    return csr_from_edges(a * b, src, dst, None, symmetric=True)


def path(n):
    v = np.arange(n - 1)
    return csr_from_edges(n, v, v + 1, None, symmetric=True)


def two_hubs(m):
    """K(2, m): two hubs with m common leaves and no edge between them, ids permuted, one isolated vertex."""
    n = m + 3
    perm = np.random.default_rng(m).permutation(n)
    h0, h1, leaves, lone = int(perm[0]), int(perm[1]), perm[2:m + 2], int(perm[m + 2])
    src = np.concatenate([np.full(m, h0), np.full(m, h1)])
    dst = np.concatenate([leaves, leaves])
    return csr_from_edges(n, src, dst, None, symmetric=True), h0, h1, lone


def dying_hub(m, t=3):
    """K8 on 0..7, the hub 8 joined to the members 0..t-1 and to the leaves 9..8+m."""
    s8, d8 = clique(8)
    src = np.concatenate([s8, np.full(t, 8), np.full(m, 8)])
    dst = np.concatenate([d8, np.arange(t), np.arange(9, 9 + m)])
    return csr_from_edges(9 + m, src, dst, None, symmetric=True)


def shuffled_rows(csr, seed):
    """The same graph with every row's entries in a random order."""
    rng = np.random.default_rng(seed)
    rows, _ = edges_of(csr)
    order = np.lexsort((rng.random(csr.nnz), rows))
    return CSR(csr.n, csr.rowptr.copy(), np.ascontiguousarray(csr.colidx[order]))


@functools.lru_cache(maxsize=None)
def rmat_case():
    """R-MAT scale 11, edge factor 8, and its reference for every k (computed once, read-only)."""
    csr = rmat(11, 8, 5)
    return (csr,) + ref_every_k(csr)


@functools.lru_cache(maxsize=None)
def cascade_case(name):
    csr = path(4096) if name == "path" else torus(24, 24, cut=True)
    k = 2 if name == "path" else 6
    return (csr, k, ref_kcore(csr, k)) + ref_core_all(csr)


# ------------------------------------------------------------------------------------- CPU

def test_abi_declares_exports_and_binds_kcore():
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gx.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+gx_kcore\s*\(\s*gx_graph\s*\*\s*g\s*,\s*uint32_t\s+k\s*,\s*int64_t\s*\*\s*degree\s*,"
                     r"\s*uint64_t\s*\*\s*stats\s*\)", header)
    assert re.search(r"\bint\s+gx_core_all\s*\(\s*gx_graph\s*\*\s*g\s*,\s*int64_t\s*\*\s*core\s*,"
                     r"\s*uint64_t\s*\*\s*kmax\s*\)", header)
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"gx_kcore", "gx_core_all"} <= exported
    sig = {name: (res, args) for name, res, args in N.SIGNATURES}
    assert sig["gx_kcore"] == (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_uint64)])
    assert sig["gx_core_all"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint64)])
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    assert callable(A.LA_KCore) and callable(A.LA_CoreAll)
    assert all(isinstance(x, int) and x > 0 for x in (A.CORE_SHORT, A.CORE_LONG, A.CORE_BATCH))
    assert A.CORE_SHORT <= A.CORE_LONG and isinstance(A.CORE_SOLO, int) and A.CORE_SOLO >= 0


def test_null_graph_is_refused_before_any_device_call():
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    deg = np.zeros(1, np.int64)
    stats = np.zeros(3, np.uint64)
    kmax = C.c_uint64(0)
    assert N.lib().gx_kcore(None, 3, N.as_i64p(deg), N.as_u64p(stats)) == -2   # GX_NULL_POINTER
    assert b"gx_kcore" in N.lib().gx_last_error()
    assert N.lib().gx_core_all(None, N.as_i64p(deg), C.byref(kmax)) == -2
    assert b"gx_core_all" in N.lib().gx_last_error()


def test_reference_matches_networkx():
    """300 vertices, 4 000 drawn pairs (seed 3): networkx.core_number, and the vertex sets of
    networkx.k_core for k = 0 .. kmax + 1."""
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(3)
    src, dst = rng.integers(0, 300, 4000), rng.integers(0, 300, 4000)
    keep = src != dst
    csr = csr_from_edges(300, src[keep], dst[keep], None, symmetric=True)
    rows, cols = edges_of(csr)
    G = nx.Graph()
    G.add_nodes_from(range(300))
    G.add_edges_from(zip(rows.tolist(), cols.tolist()))
    core, kmax, per_k = ref_every_k(csr)
    theirs = nx.core_number(G)
    np.testing.assert_array_equal(core, [theirs[v] for v in range(300)])
    assert kmax == max(theirs.values()) and kmax >= 10
    for k in range(kmax + 2):
        deg, stats = per_k[k]
        H = nx.k_core(G, k)
        assert set(np.flatnonzero(deg >= 0).tolist()) == set(H.nodes()), k
        assert (int(stats[0]), int(stats[1])) == (H.number_of_nodes(), H.number_of_edges())
        np.testing.assert_array_equal(deg[deg >= 0], [H.degree(v) for v in np.flatnonzero(deg >= 0).tolist()])


def test_reference_on_k6():
    csr = csr_from_edges(6, *clique(6), None, symmetric=True)
    core, kmax, per_k = ref_every_k(csr)
    np.testing.assert_array_equal(core, np.full(6, 5))
    assert kmax == 5
    np.testing.assert_array_equal(per_k[5][0], np.full(6, 5))
    np.testing.assert_array_equal(per_k[5][1], [6, 15, 0])
    np.testing.assert_array_equal(per_k[6][0], np.full(6, -1))
    np.testing.assert_array_equal(per_k[6][1], [0, 0, 1])


def test_reference_on_the_torus_and_the_cut_torus():
    csr = torus(24, 24)
    assert csr.nnz == 2 * 1728
    np.testing.assert_array_equal(ref_kcore(csr, 6)[0], np.full(576, 6))
    np.testing.assert_array_equal(ref_kcore(csr, 6)[1], [576, 1728, 0])
    np.testing.assert_array_equal(ref_kcore(csr, 7)[1], [0, 0, 1])
    csr, k, (deg, stats), core, kmax = cascade_case("torus")
    assert csr.nnz == 2 * 1727 and k == 6
    np.testing.assert_array_equal(ref_kcore(csr, 5)[1], [576, 1727, 0])
    np.testing.assert_array_equal(deg, np.full(576, -1))
    np.testing.assert_array_equal(stats, [0, 0, 16])
    np.testing.assert_array_equal(core, np.full(576, 5))
    assert kmax == 5


def test_reference_on_the_path():
    csr, k, (deg, stats), core, kmax = cascade_case("path")
    np.testing.assert_array_equal(ref_kcore(csr, 1)[1], [4096, 4095, 0])
    np.testing.assert_array_equal(deg, np.full(4096, -1))
    np.testing.assert_array_equal(stats, [0, 0, 2048])
    np.testing.assert_array_equal(core, np.full(4096, 1))
    assert kmax == 1


# ------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    c = Context(0)
    yield c
    c.close()


def check_every_k(G, ref, ks=None, calls=2, tag=""):
    """Every call twice on the one Graph: LA_CoreAll, then LA_KCore for the ks (default 0 .. kmax + 1),
    degree and statistics together and the statistics alone."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    core, kmax, per_k = ref
    for call in range(calls):
        got, gmax = A.LA_CoreAll(G)
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, core, err_msg=f"{tag} core, call {call + 1}")
        assert gmax == kmax
        for k in (ks if ks is not None else sorted(per_k)):
            deg, stats = A.LA_KCore(G, k, degree=True, stats=True)
            assert deg.dtype == np.int64 and stats.dtype == np.uint64
            np.testing.assert_array_equal(deg, per_k[k][0], err_msg=f"{tag} degree, k {k}, call {call + 1}")
            np.testing.assert_array_equal(stats, per_k[k][1], err_msg=f"{tag} stats, k {k}, call {call + 1}")
            np.testing.assert_array_equal(A.LA_KCore(G, k, degree=False, stats=True), per_k[k][1])
            np.testing.assert_array_equal(got >= k, deg >= 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", UNDIRECTED_FIXTURES)
def test_gpu_fixtures_every_k(ctx, fixture_graphs, name):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    g = fixture_graphs(name)
    assert not g.directed
    G = A.Graph(ctx, g.csr, False)
    try:
        check_every_k(G, ref_every_k(g.csr), tag=name)
    finally:
        G.close()


@pytest.mark.gpu
def test_gpu_rmat_every_k_with_other_calls_between(ctx):
    """gx_bfs, gx_wcc and gx_ktruss between the k-core calls return what they return, call for call, on
    a fresh graph that never saw a k-core call; every edge of the k-truss joins vertices of the
    (k-1)-core."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    csr, core, kmax, per_k = rmat_case()
    assert kmax >= 8 and max(int(st[2]) for _, st in per_k.values()) >= 4
    rows, cols = edges_of(csr)
    hub = int(np.argmax(np.diff(csr.rowptr.astype(np.int64))))
    truss_ks = (3, 4, 6)

    def others(X, i):
        return [A.LA_BFS(X, hub), A.WeaklyConnectedComponents(X), A.LA_KTruss(X, truss_ks[i])]

    F = A.Graph(ctx, csr, False)
    try:
        fresh = [others(F, i) for i in range(3)]
    finally:
        F.close()
    G = A.Graph(ctx, csr, False)
    try:
        for call in range(3):
            check_every_k(G, (core, kmax, per_k), calls=1, tag=f"call {call + 1}")
            got = others(G, call)
            for a, b in zip(got, fresh[call]):
                np.testing.assert_array_equal(a, b)
            again, amax = A.LA_CoreAll(G)
            np.testing.assert_array_equal(again, core)
            assert amax == kmax
            in_truss = got[2] >= 0
            assert in_truss.any()
            assert (again[rows[in_truss]] >= truss_ks[call] - 1).all()
            assert (again[cols[in_truss]] >= truss_ks[call] - 1).all()
    finally:
        G.close()


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{"GX_CORE_SOLO": "0"}, {}, {"GX_CORE_SOLO": "1"}, {"GX_CORE_BATCH": "1"},
                                   {"GX_CORE_BATCH": "512"}, {"GX_CORE_SOLO": "0", "GX_CORE_BATCH": "1"}],
                         ids=["solo0", "default", "solo1", "batch1", "batch512", "solo0-batch1"])
@pytest.mark.parametrize("name", ["path", "torus"])
def test_gpu_long_cascade_under_every_schedule(ctx, monkeypatch, name, knobs):
    """The 4 096-vertex path at k = 2 (two vertices per round, 2 048 rounds) and the cut torus at k = 6
    (16 rounds of a few vertices): outputs and the round count are those of the synchronous peel
    whether one workgroup runs the rounds, the grid does, or they alternate."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    for key, v in knobs.items():
        monkeypatch.setenv(key, v)
    csr, k, (deg, stats), core, kmax = cascade_case(name)
    G = A.Graph(ctx, csr, False)
    try:
        for _ in range(2):
            got_deg, got_stats = A.LA_KCore(G, k, degree=True, stats=True)
            np.testing.assert_array_equal(got_deg, deg)
            np.testing.assert_array_equal(got_stats, stats)
            got, gmax = A.LA_CoreAll(G)
            np.testing.assert_array_equal(got, core)
            assert gmax == kmax
    finally:
        G.close()


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{}, {"GX_CORE_SOLO": "0"}], ids=["default", "solo0"])
def test_gpu_two_hubs_appended_exactly_once(ctx, monkeypatch, knobs):
    """K(2, 3000): at k = 3 round 1 removes the 3 000 leaves, which decrement the two hubs 3 000 times
    each in the one round; each hub joins the next frontier once (twice would remove it twice and the
    vertex count would wrap)."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    for key, v in knobs.items():
        monkeypatch.setenv(key, v)
    m = 3000
    csr, h0, h1, lone = two_hubs(m)
    want2 = np.full(csr.n, 2)
    want2[[h0, h1]] = m
    want2[lone] = -1
    np.testing.assert_array_equal(ref_kcore(csr, 2)[0], want2)
    np.testing.assert_array_equal(ref_kcore(csr, 3)[1], [0, 0, 2])
    want_core = np.full(csr.n, 2)
    want_core[lone] = 0
    G = A.Graph(ctx, csr, False)
    try:
        for _ in range(2):
            deg, stats = A.LA_KCore(G, 2, degree=True, stats=True)
            np.testing.assert_array_equal(deg, want2)
            np.testing.assert_array_equal(stats, [m + 2, 2 * m, 1])   # the isolated vertex leaves
            deg, stats = A.LA_KCore(G, 3, degree=True, stats=True)
            np.testing.assert_array_equal(deg, np.full(csr.n, -1))
            np.testing.assert_array_equal(stats, [0, 0, 2])
            core, kmax = A.LA_CoreAll(G)
            np.testing.assert_array_equal(core, want_core)
            assert kmax == 2
    finally:
        G.close()


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{}, {"GX_CORE_SHORT": "4", "GX_CORE_LONG": "16"},
                                   {"GX_CORE_SHORT": "1", "GX_CORE_LONG": "4096"},
                                   {"GX_CORE_SHORT": "4096", "GX_CORE_LONG": "4096"}],
                         ids=["default", "short4-long16", "all-wave", "all-thread"])
@pytest.mark.parametrize("m", [8, 40, 3000])
def test_gpu_row_tiers_dying_hub(ctx, monkeypatch, m, knobs):
    """K8 plus a hub joined to three members and m leaves, k = 4: round 1 removes the leaves, round 2
    the hub, whose row has m + 3 entries of which three are alive.  The thresholds (the defaults and
    three forced pairs) put that row, and the leaves' and members' rows, through the thread, the wave
    and the workgroup form; with GX_CORE_SOLO = 0 the grid's expand kernel walks the hub's row, else
    the solo workgroup does."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    for key, v in knobs.items():
        monkeypatch.setenv(key, v)
    csr = dying_hub(m)
    assert int(csr.rowptr[9] - csr.rowptr[8]) == m + 3
    core, kmax, per_k = ref_every_k(csr)
    want = np.full(csr.n, -1)
    want[:8] = 7
    np.testing.assert_array_equal(per_k[4][0], want)
    np.testing.assert_array_equal(per_k[4][1], [8, 28, 2])
    for solo in (None, "0"):
        if solo is not None:
            monkeypatch.setenv("GX_CORE_SOLO", solo)
        G = A.Graph(ctx, csr, False)
        try:
            check_every_k(G, (core, kmax, per_k), ks=[0, 1, 2, 3, 4, 7, 8], tag=f"m {m} solo {solo}")
        finally:
            G.close()


@pytest.mark.gpu
def test_gpu_diagonal_entries_count_toward_no_degree(ctx, fixture_graphs):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    plain = fixture_graphs("test-lcc-undirected").csr
    rows, cols = edges_of(plain)
    assert (rows != cols).all()
    loops_at = np.arange(0, plain.n, 3)
    loops = csr_from_edges(plain.n, np.concatenate([rows, loops_at]), np.concatenate([cols, loops_at]), None,
                           symmetric=False)
    assert loops.nnz == plain.nnz + len(loops_at)
    ref = ref_every_k(plain)
    core, kmax, per_k = ref_every_k(loops)   # the reference itself treats the loops that way
    np.testing.assert_array_equal(core, ref[0])
    for k in per_k:
        np.testing.assert_array_equal(per_k[k][0], ref[2][k][0])
        np.testing.assert_array_equal(per_k[k][1], ref[2][k][1])
    G = A.Graph(ctx, loops, False)
    try:
        check_every_k(G, ref, tag="loops")
    finally:
        G.close()


@pytest.mark.gpu
def test_gpu_unsorted_rows_give_the_same_arrays(ctx):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    csr, core, kmax, per_k = rmat_case()
    mixed = shuffled_rows(csr, 9)
    assert (mixed.colidx != csr.colidx).any()
    G = A.Graph(ctx, mixed, False)
    try:
        check_every_k(G, (core, kmax, per_k), ks=[0, 1, 2, kmax // 2, kmax, kmax + 1], calls=1, tag="unsorted")
    finally:
        G.close()


@pytest.mark.gpu
def test_gpu_contract_edges(ctx, fixture_graphs):
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    L = N.lib()
    g = fixture_graphs("example-undirected")
    n = g.csr.n
    deg = np.full(n, -7, np.int64)
    stats = np.full(3, 77, np.uint64)
    kmax = C.c_uint64(77)

    def untouched():
        return (deg == -7).all() and (stats == 77).all() and kmax.value == 77

    rows, cols = edges_of(g.csr)
    plain_deg = np.bincount(rows[rows != cols], minlength=n)
    G = A.Graph(ctx, g.csr, False)
    try:
        assert L.gx_kcore(G.handle, 3, None, None) == -2   # nothing to write to: GX_NULL_POINTER
        assert b"gx_kcore" in L.gx_last_error()
        assert L.gx_core_all(G.handle, None, None) == -2
        assert b"gx_core_all" in L.gx_last_error()
        with pytest.raises(N.GxError) as err:
            A.LA_KCore(G, 3, degree=False, stats=False)
        assert err.value.code == -2
        for k in (-1, 2 ** 32):
            with pytest.raises(ValueError):
                A.LA_KCore(G, k)
        assert untouched()
        # k = 0 keeps every vertex: the plain off-diagonal degree, no round
        d0, s0 = A.LA_KCore(G, 0, degree=True, stats=True)
        np.testing.assert_array_equal(d0, plain_deg)
        np.testing.assert_array_equal(s0, [n, plain_deg.sum() // 2, 0])
        # k = 2^32 - 1: everybody leaves in the one round
        dm, sm = A.LA_KCore(G, 2 ** 32 - 1, degree=True, stats=True)
        np.testing.assert_array_equal(dm, np.full(n, -1))
        np.testing.assert_array_equal(sm, [0, 0, 1])
        # each output alone equals its half of the full call
        full_deg, full_stats = A.LA_KCore(G, 2, degree=True, stats=True)
        np.testing.assert_array_equal(full_deg, ref_kcore(g.csr, 2)[0])
        np.testing.assert_array_equal(A.LA_KCore(G, 2), full_deg)
        np.testing.assert_array_equal(A.LA_KCore(G, 2, degree=False, stats=True), full_stats)
        core, top = A.LA_CoreAll(G)
        only = np.full(n, -7, np.int64)
        assert L.gx_core_all(G.handle, N.as_i64p(only), None) == 0
        np.testing.assert_array_equal(only, core)
        assert L.gx_core_all(G.handle, None, C.byref(kmax)) == 0 and kmax.value == top
        kmax.value = 77
    finally:
        G.close()
    D = A.Graph(ctx, fixture_graphs("example-directed").csr, True)   # a directed graph: GX_INVALID_VALUE
    try:
        for _ in range(2):
            assert L.gx_kcore(D.handle, 3, N.as_i64p(deg), N.as_u64p(stats)) == -3
            assert b"gx_kcore" in L.gx_last_error() and untouched()
            assert L.gx_core_all(D.handle, N.as_i64p(deg), C.byref(kmax)) == -3
            assert b"gx_core_all" in L.gx_last_error() and untouched()
    finally:
        D.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5])
def test_gpu_no_entries_and_a_single_vertex(ctx, n):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    csr = csr_from_edges(n, [], [], None, symmetric=True)
    loop = csr_from_edges(n, [0], [0], None, symmetric=True)   # one diagonal entry and no edge
    for case in (csr, loop):
        G = A.Graph(ctx, case, False)
        try:
            for _ in range(2):
                deg, stats = A.LA_KCore(G, 0, degree=True, stats=True)
                np.testing.assert_array_equal(deg, np.zeros(n))
                np.testing.assert_array_equal(stats, [n, 0, 0])
                deg, stats = A.LA_KCore(G, 1, degree=True, stats=True)
                np.testing.assert_array_equal(deg, np.full(n, -1))
                np.testing.assert_array_equal(stats, [0, 0, 1])
                core, kmax = A.LA_CoreAll(G)
                np.testing.assert_array_equal(core, np.zeros(n))
                assert kmax == 0
        finally:
            G.close()
