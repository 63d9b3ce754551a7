"""k-truss and truss numbers (gx_ktruss / LA_KTruss, gx_truss_all / LA_AllKTruss).

An edge is an unordered pair {i, j}, i != j, of an undirected graph stored in both directions; the
k-truss is the largest subgraph whose every edge lies in at least k - 2 of its triangles.  support is
one int64 per stored entry (the triangles of the k-truss through the entry's edge, -1 when the edge
is not in it or the entry is diagonal), stats = (edges, triangles, rounds of synchronous pruning that
removed an edge), truss = the largest k whose k-truss holds the entry's edge (0 on the diagonal).
Everything is an integer and unique, so every comparison is bit for bit (assert_array_equal); there
is no tolerance in this file.

The reference is ref_ktruss below: scipy sparse, S = (A @ A).multiply(A) on the surviving 0/1 matrix,
entries below k - 2 dropped, repeated; the supports are read by explicit indexing, so zero supports
are not lost.  On the CPU it is pinned by networkx.k_truss and by hand-checked graphs (cliques, a
triangulated torus and the same torus with one edge cut, whose 4-truss unravels in 32 rounds).  GPU:
the Graphalytics fixtures, gx_mxm_masked at k = 2, R-MAT with other algorithms' calls in between,
both recount forms forced, the cascade, every row tier, diagonal entries, unsorted rows and the
edges of the contract.
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


def ref_ktruss(csr, k):
    """(support[nnz] int64, stats[3] uint64) of the k-truss: LAGraph's loop, one round per pass."""
    sp = pytest.importorskip("scipy.sparse")
    n = csr.n
    rows, cols = edges_of(csr)
    alive = rows != cols
    rounds = 0
    while True:
        A = sp.csr_matrix((np.ones(int(alive.sum()), np.int64), (rows[alive], cols[alive])), shape=(n, n))
        S = sp.csr_matrix((A @ A).multiply(A))
        sup = np.asarray(S[rows, cols]).ravel().astype(np.int64) if len(rows) else np.zeros(0, np.int64)
        die = alive & (sup < k - 2)
        if not die.any():
            break
        alive &= ~die
        rounds += 1
    assert alive.sum() % 2 == 0 and sup[alive].sum() % 6 == 0
    stats = np.array([alive.sum() // 2, sup[alive].sum() // 6, rounds], np.uint64)
    return np.where(alive, sup, -1), stats


def ref_truss_all(csr):
    """(truss[nnz] int64, kmax, {k: (support, stats)} for k = 2 .. kmax + 1)."""
    rows, cols = edges_of(csr)
    truss = np.where(rows != cols, 2, 0).astype(np.int64)
    per_k = {}
    k = 2
    while True:
        sup, stats = ref_ktruss(csr, k)
        per_k[k] = (sup, stats)
        truss[sup >= 0] = k
        if stats[0] == 0:
            break
        k += 1
    kmax = int(truss.max(initial=0))
    for v in per_k.values():
        v[0].setflags(write=False)
    truss.setflags(write=False)
    assert sorted(per_k) == list(range(2, max(kmax, 1) + 2))   # no edge at all: k = 2 alone
    return truss, kmax, per_k


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


def hubs_graph(m):
    """Two hubs joined by an edge with m common leaves, ids permuted, one isolated vertex."""
    n = m + 3
    perm = np.random.default_rng(m).permutation(n)
    h0, h1, leaves = int(perm[0]), int(perm[1]), perm[2:m + 2]   # perm[m + 2] stays isolated
    src = np.concatenate([[h0], np.full(m, h0), np.full(m, h1)])
    dst = np.concatenate([[h1], leaves, leaves])
    return csr_from_edges(n, src, dst, None, symmetric=True), h0, h1


def shuffled_rows(csr, seed):
    """The same graph with every row's entries in a random order, and the map new entry -> old."""
    rng = np.random.default_rng(seed)
    rows, _ = edges_of(csr)
    order = np.lexsort((rng.random(csr.nnz), rows))
    return CSR(csr.n, csr.rowptr.copy(), np.ascontiguousarray(csr.colidx[order])), order


@functools.lru_cache(maxsize=None)
def rmat_case():
    """R-MAT scale 11, edge factor 8, and its reference for every k (computed once, read-only)."""
    csr = rmat(11, 8, 5)
    return (csr,) + ref_truss_all(csr)


@functools.lru_cache(maxsize=None)
def torus_case():
    csr = torus(24, 24, cut=True)
    return (csr,) + ref_truss_all(csr)


# ------------------------------------------------------------------------------------- CPU

def test_abi_declares_exports_and_binds_ktruss():
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gx.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+gx_ktruss\s*\(\s*gx_graph\s*\*\s*g\s*,\s*uint32_t\s+k\s*,\s*int64_t\s*\*\s*support\s*,"
                     r"\s*uint64_t\s*\*\s*stats\s*\)", header)
    assert re.search(r"\bint\s+gx_truss_all\s*\(\s*gx_graph\s*\*\s*g\s*,\s*int64_t\s*\*\s*truss\s*,"
                     r"\s*uint64_t\s*\*\s*kmax\s*\)", header)
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"gx_ktruss", "gx_truss_all"} <= exported
    sig = {name: (res, args) for name, res, args in N.SIGNATURES}
    assert sig["gx_ktruss"] == (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_uint64)])
    assert sig["gx_truss_all"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint64)])
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    assert callable(A.LA_KTruss) and callable(A.LA_AllKTruss)
    assert (A.TRUSS_SHORT, A.TRUSS_LONG) == (16, 1024)


def test_null_graph_is_refused_before_any_device_call():
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    sup = np.zeros(1, np.int64)
    stats = np.zeros(3, np.uint64)
    kmax = C.c_uint64(0)
    assert N.lib().gx_ktruss(None, 3, N.as_i64p(sup), N.as_u64p(stats)) == -2   # GX_NULL_POINTER
    assert b"gx_ktruss" in N.lib().gx_last_error()
    assert N.lib().gx_truss_all(None, N.as_i64p(sup), C.byref(kmax)) == -2
    assert b"gx_truss_all" in N.lib().gx_last_error()


def test_reference_matches_networkx():
    """300 vertices, 4 000 drawn pairs (seed 3): the edge sets of networkx.k_truss for k = 2 .. 8."""
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(3)
    src, dst = rng.integers(0, 300, 4000), rng.integers(0, 300, 4000)
    keep = src != dst
    csr = csr_from_edges(300, src[keep], dst[keep], None, symmetric=True)
    rows, cols = edges_of(csr)
    G = nx.Graph()
    G.add_nodes_from(range(300))
    G.add_edges_from(zip(rows.tolist(), cols.tolist()))
    seen = {}
    for k in range(2, 9):
        sup, stats = ref_ktruss(csr, k)
        ours = {(int(i), int(j)) for i, j, s in zip(rows, cols, sup) if s >= 0 and i < j}
        theirs = {(min(u, v), max(u, v)) for u, v in nx.k_truss(G, k).edges()}
        assert ours == theirs, k
        assert int(stats[0]) == len(theirs)
        seen[k] = (int(stats[0]), int(stats[2]))
    # (edges, rounds); support-0 edges take no triangle with them, so k = 3 is one round
    assert [seen[k] for k in (2, 3, 4, 5)] == [(3800, 0), (3353, 1), (721, 20), (0, 5)]


def test_reference_on_cliques():
    csr = csr_from_edges(6, *clique(6), None, symmetric=True)
    truss, kmax, per_k = ref_truss_all(csr)
    np.testing.assert_array_equal(per_k[2][0], np.full(30, 4))
    np.testing.assert_array_equal(per_k[6][0], np.full(30, 4))
    np.testing.assert_array_equal(per_k[6][1], [15, 20, 0])
    np.testing.assert_array_equal(per_k[7][1], [0, 0, 1])
    np.testing.assert_array_equal(truss, np.full(30, 6))
    assert kmax == 6
    # K5 on 0..4, the pendant edge 4-5, a triangle on 6..8
    s5, d5 = clique(5)
    s3, d3 = clique(3, first=6)
    csr = csr_from_edges(9, np.concatenate([s5, [4], s3]), np.concatenate([d5, [5], d3]), None, symmetric=True)
    rows, cols = edges_of(csr)
    truss, kmax, per_k = ref_truss_all(csr)
    want = np.where((rows <= 4) & (cols <= 4), 5, np.where((rows >= 6) & (cols >= 6), 3, 2))
    np.testing.assert_array_equal(truss, want)
    assert kmax == 5
    np.testing.assert_array_equal(per_k[3][1], [13, 11, 1])
    np.testing.assert_array_equal(per_k[4][1], [10, 10, 1])


def test_reference_on_the_torus():
    csr = torus(24, 24)
    assert csr.nnz == 2 * 1728
    sup, stats = ref_ktruss(csr, 4)
    np.testing.assert_array_equal(sup, np.full(csr.nnz, 2))
    np.testing.assert_array_equal(stats, [1728, 1152, 0])
    sup, stats = ref_ktruss(csr, 5)
    np.testing.assert_array_equal(sup, np.full(csr.nnz, -1))
    np.testing.assert_array_equal(stats, [0, 0, 1])


def test_reference_on_the_cut_torus_unravels_in_32_rounds():
    csr, truss, kmax, per_k = torus_case()
    assert csr.nnz == 2 * 1727 and kmax == 3
    np.testing.assert_array_equal(per_k[4][0], np.full(csr.nnz, -1))
    np.testing.assert_array_equal(per_k[4][1], [0, 0, 32])
    np.testing.assert_array_equal(truss, np.full(csr.nnz, 3))
    assert ref_ktruss(torus(16, 40, cut=True), 4)[1].tolist() == [0, 0, 40]


# ------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    c = Context(0)
    yield c
    c.close()


def check_every_k(G, ref, ks=None, calls=2, tag=""):
    """Every call twice on the one Graph: LA_KTruss for the ks (default 2 .. kmax + 1), support and
    statistics together and each alone, then LA_AllKTruss."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    truss, kmax, per_k = ref
    for call in range(calls):
        for k in (ks if ks is not None else sorted(per_k)):
            sup, stats = A.LA_KTruss(G, k, support=True, stats=True)
            assert sup.dtype == np.int64 and stats.dtype == np.uint64
            np.testing.assert_array_equal(sup, per_k[k][0], err_msg=f"{tag} support, k {k}, call {call + 1}")
            np.testing.assert_array_equal(stats, per_k[k][1], err_msg=f"{tag} stats, k {k}, call {call + 1}")
            np.testing.assert_array_equal(A.LA_KTruss(G, k, support=False, stats=True), per_k[k][1])
        got, gmax = A.LA_AllKTruss(G)
        np.testing.assert_array_equal(got, truss, err_msg=f"{tag} truss, call {call + 1}")
        assert gmax == kmax


@pytest.mark.gpu
@pytest.mark.parametrize("name", UNDIRECTED_FIXTURES)
def test_gpu_fixtures_every_k(ctx, fixture_graphs, name):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    g = fixture_graphs(name)
    assert not g.directed
    G = A.Graph(ctx, g.csr, False)
    try:
        check_every_k(G, ref_truss_all(g.csr), tag=name)
    finally:
        G.close()


@pytest.mark.gpu
def test_gpu_k2_equals_mxm_masked(ctx):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    csr = rmat(10, 8, 3)
    rows, cols = edges_of(csr)
    assert (rows != cols).all()
    G = A.Graph(ctx, csr, False)
    try:
        want = A.mxm_masked(G)
        for _ in range(2):
            sup, stats = A.LA_KTruss(G, 2, support=True, stats=True)
            np.testing.assert_array_equal(sup, want)
            np.testing.assert_array_equal(stats, [csr.nnz // 2, want.sum() // 6, 0])
    finally:
        G.close()


@pytest.mark.gpu
def test_gpu_rmat_every_k_with_other_calls_between(ctx):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    csr, truss, kmax, per_k = rmat_case()
    assert kmax >= 6 and max(int(st[2]) for _, st in per_k.values()) >= 5
    hub = int(np.argmax(np.diff(csr.rowptr.astype(np.int64))))
    F = A.Graph(ctx, csr, False)
    try:
        fresh = [A.LA_LCC(F), A.LA_BFS(F, hub), A.WeaklyConnectedComponents(F)]
    finally:
        F.close()
    G = A.Graph(ctx, csr, False)
    try:
        for call in range(3):
            check_every_k(G, (truss, kmax, per_k), calls=1, tag=f"call {call + 1}")
            np.testing.assert_array_equal(A.LA_LCC(G), fresh[0])
            np.testing.assert_array_equal(A.LA_BFS(G, hub), fresh[1])
            np.testing.assert_array_equal(A.WeaklyConnectedComponents(G), fresh[2])
    finally:
        G.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["all", "marked"])
def test_gpu_forced_recount_form(ctx, monkeypatch, form):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    monkeypatch.setenv("GX_TRUSS_RECOUNT", form)
    for case in (rmat_case, torus_case):
        csr, truss, kmax, per_k = case()
        G = A.Graph(ctx, csr, False)
        try:
            check_every_k(G, (truss, kmax, per_k), tag=f"{case.__name__} {form}")
        finally:
            G.close()


@pytest.mark.gpu
def test_gpu_cascade_on_the_cut_torus(ctx):
    """Every round but the first removes a handful of edges next to the last round's: a recount that
    misses a lost triangle, or reads alive flags that are being written, ends early or late."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    csr, truss, kmax, per_k = torus_case()
    G = A.Graph(ctx, csr, False)
    try:
        for _ in range(2):
            sup, stats = A.LA_KTruss(G, 4, support=True, stats=True)
            np.testing.assert_array_equal(sup, np.full(csr.nnz, -1))
            np.testing.assert_array_equal(stats, [0, 0, 32])
            got, gmax = A.LA_AllKTruss(G)
            np.testing.assert_array_equal(got, np.full(csr.nnz, 3))
            assert gmax == 3
    finally:
        G.close()


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{}, {"GX_TRUSS_SHORT": "4", "GX_TRUSS_LONG": "16"}], ids=["default", "short4-long16"])
@pytest.mark.parametrize("m", [70, 300, 3000])
def test_gpu_row_tiers_two_hubs(ctx, monkeypatch, m, knobs):
    """The hub edge's shorter row has m + 1 entries: the wave tier at 70 and 300, the workgroup tier
    at 3 000 (and at all three under the small thresholds); a leaf edge's has 2: the thread tier."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    for key, v in knobs.items():
        monkeypatch.setenv(key, v)
    csr, h0, h1 = hubs_graph(m)
    rows, cols = edges_of(csr)
    hub_edge = ((rows == h0) & (cols == h1)) | ((rows == h1) & (cols == h0))
    assert hub_edge.sum() == 2 and csr.nnz == 4 * m + 2
    want = np.where(hub_edge, m, 1)
    G = A.Graph(ctx, csr, False)
    try:
        for _ in range(2):
            for k in (2, 3):
                sup, stats = A.LA_KTruss(G, k, support=True, stats=True)
                np.testing.assert_array_equal(sup, want)
                np.testing.assert_array_equal(stats, [2 * m + 1, m, 0])
            sup, stats = A.LA_KTruss(G, 4, support=True, stats=True)
            np.testing.assert_array_equal(sup, np.full(csr.nnz, -1))
            np.testing.assert_array_equal(stats, [0, 0, 2])
            got, gmax = A.LA_AllKTruss(G)
            np.testing.assert_array_equal(got, np.full(csr.nnz, 3))
            assert gmax == 3
    finally:
        G.close()


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{}, {"GX_TRUSS_SHORT": "4", "GX_TRUSS_LONG": "16"}], ids=["default", "short4-long16"])
def test_gpu_row_tiers_k300(ctx, monkeypatch, knobs):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    for key, v in knobs.items():
        monkeypatch.setenv(key, v)
    csr = csr_from_edges(300, *clique(300), None, symmetric=True)
    G = A.Graph(ctx, csr, False)
    try:
        for _ in range(2):
            for k in (2, 300):
                sup, stats = A.LA_KTruss(G, k, support=True, stats=True)
                np.testing.assert_array_equal(sup, np.full(csr.nnz, 298))
                np.testing.assert_array_equal(stats, [300 * 299 // 2, 300 * 299 * 298 // 6, 0])
            np.testing.assert_array_equal(A.LA_KTruss(G, 301, support=False, stats=True), [0, 0, 1])
            got, gmax = A.LA_AllKTruss(G)
            np.testing.assert_array_equal(got, np.full(csr.nnz, 300))
            assert gmax == 300
    finally:
        G.close()


@pytest.mark.gpu
def test_gpu_diagonal_entries_belong_to_no_truss(ctx):
    """K5 + pendant + triangle, with self-loops on a clique vertex, the pendant vertex and an
    otherwise isolated vertex: -1 / 0 there, the other values as without the loops."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    s5, d5 = clique(5)
    s3, d3 = clique(3, first=6)
    src, dst = np.concatenate([s5, [4], s3]), np.concatenate([d5, [5], d3])
    plain = csr_from_edges(10, src, dst, None, symmetric=True)
    loops = csr_from_edges(10, np.concatenate([src, [0, 5, 9]]), np.concatenate([dst, [0, 5, 9]]), None, symmetric=True)
    assert loops.nnz == plain.nnz + 3
    rows, cols = edges_of(loops)
    off = rows != cols
    ref_plain, ref_loops = ref_truss_all(plain), ref_truss_all(loops)
    for k, (sup, stats) in ref_loops[2].items():   # the reference itself treats the loops that way
        np.testing.assert_array_equal(sup[off], ref_plain[2][k][0])
        np.testing.assert_array_equal(sup[~off], [-1, -1, -1])
        np.testing.assert_array_equal(stats, ref_plain[2][k][1])
    np.testing.assert_array_equal(ref_loops[0][~off], [0, 0, 0])
    G = A.Graph(ctx, loops, False)
    try:
        check_every_k(G, ref_loops, tag="loops")
    finally:
        G.close()


@pytest.mark.gpu
def test_gpu_unsorted_rows_give_the_entry_order_back(ctx):
    """Rows in a random order take the sorted copy; the output is in the caller's entry order."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    csr, truss, kmax, per_k = rmat_case()
    mixed, order = shuffled_rows(csr, 9)
    assert (mixed.colidx != csr.colidx).any()
    ref = (truss[order], kmax, {k: (sup[order], st) for k, (sup, st) in per_k.items()})
    G = A.Graph(ctx, mixed, False)
    try:
        check_every_k(G, ref, ks=[2, 4, kmax, kmax + 1], tag="unsorted")
    finally:
        G.close()


@pytest.mark.gpu
def test_gpu_contract_edges(ctx, fixture_graphs):
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    L = N.lib()
    g = fixture_graphs("example-undirected")
    nnz = g.csr.nnz
    sup = np.full(nnz, -7, np.int64)
    stats = np.full(3, 77, np.uint64)
    kmax = C.c_uint64(77)

    def untouched():
        return (sup == -7).all() and (stats == 77).all() and kmax.value == 77

    G = A.Graph(ctx, g.csr, False)
    try:
        for k in (0, 1):   # k < 2: GX_INVALID_VALUE
            assert L.gx_ktruss(G.handle, k, N.as_i64p(sup), N.as_u64p(stats)) == -3
            assert b"gx_ktruss" in L.gx_last_error() and untouched()
        assert L.gx_ktruss(G.handle, 3, None, None) == -2   # nothing to write to: GX_NULL_POINTER
        assert b"gx_ktruss" in L.gx_last_error()
        assert L.gx_truss_all(G.handle, None, None) == -2
        assert b"gx_truss_all" in L.gx_last_error()
        with pytest.raises(N.GxError) as err:
            A.LA_KTruss(G, 3, support=False, stats=False)
        assert err.value.code == -2
        # each output alone equals its half of the full call
        full_sup, full_stats = A.LA_KTruss(G, 3, support=True, stats=True)
        np.testing.assert_array_equal(A.LA_KTruss(G, 3), full_sup)
        np.testing.assert_array_equal(A.LA_KTruss(G, 3, support=False, stats=True), full_stats)
        truss, top = A.LA_AllKTruss(G)
        only = np.full(nnz, -7, np.int64)
        assert L.gx_truss_all(G.handle, N.as_i64p(only), None) == 0
        np.testing.assert_array_equal(only, truss)
        assert L.gx_truss_all(G.handle, None, C.byref(kmax)) == 0 and kmax.value == top
        kmax.value = 77
    finally:
        G.close()
    D = A.Graph(ctx, fixture_graphs("example-directed").csr, True)   # a directed graph: GX_INVALID_VALUE
    try:
        assert L.gx_ktruss(D.handle, 3, N.as_i64p(sup), N.as_u64p(stats)) == -3
        assert b"gx_ktruss" in L.gx_last_error() and untouched()
        assert L.gx_truss_all(D.handle, N.as_i64p(sup), C.byref(kmax)) == -3
        assert b"gx_truss_all" in L.gx_last_error() and untouched()
    finally:
        D.close()
    # an "undirected" graph whose CSR lacks one reverse entry: found on the device, nothing written
    rows, cols = edges_of(g.csr)
    drop = int(np.flatnonzero(rows != cols)[-1])
    keep = np.arange(nnz) != drop
    lame = csr_from_edges(g.csr.n, rows[keep], cols[keep], None, symmetric=False)
    assert lame.nnz == nnz - 1
    B = A.Graph(ctx, lame, False)
    try:
        for _ in range(2):
            assert L.gx_ktruss(B.handle, 3, N.as_i64p(sup), N.as_u64p(stats)) == -3
            assert b"gx_ktruss" in L.gx_last_error() and untouched()
            assert L.gx_truss_all(B.handle, N.as_i64p(sup), C.byref(kmax)) == -3
            assert b"gx_truss_all" in L.gx_last_error() and untouched()
    finally:
        B.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5])
def test_gpu_no_entries_and_a_single_vertex(ctx, n):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    csr = csr_from_edges(n, [], [], None, symmetric=True)
    G = A.Graph(ctx, csr, False)
    try:
        for _ in range(2):
            sup, stats = A.LA_KTruss(G, 3, support=True, stats=True)
            assert sup.shape == (0,)
            np.testing.assert_array_equal(stats, [0, 0, 0])
            truss, kmax = A.LA_AllKTruss(G)
            assert truss.shape == (0,) and kmax == 0
    finally:
        G.close()
    loop = csr_from_edges(n, [0], [0], None, symmetric=True)   # one diagonal entry and no edge
    G = A.Graph(ctx, loop, False)
    try:
        sup, stats = A.LA_KTruss(G, 2, support=True, stats=True)
        np.testing.assert_array_equal(sup, [-1])
        np.testing.assert_array_equal(stats, [0, 0, 0])
        truss, kmax = A.LA_AllKTruss(G)
        np.testing.assert_array_equal(truss, [0])
        assert kmax == 0
    finally:
        G.close()
