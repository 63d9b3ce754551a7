"""Strongly connected components (gx_scc / LA_SCC).

u and v share a component exactly when each reaches the other over stored entries; comp[v] is the
smallest id of v's component (gx_wcc's labelling rule) and stats = (components, vertices of the largest,
single-vertex components).  Everything is an integer and unique, so every comparison is bit for bit
(assert_array_equal); there is no tolerance in this file.

The reference is ref_scc below: an iterative Tarjan with an explicit stack, each component's members
set to their smallest id; ref_stats is np.unique with counts.  On the CPU it is pinned by scipy and
networkx on a drawn graph, by a ring, a path and the seven directed Graphalytics fixtures.  GPU: the
fixtures (the undirected ones against gx_wcc), planted components under every phase setting, the long
chains under every way of scheduling the rounds, the colour phase in its worst and best order, a hub
whose two degree words reach zero in the same round, diagonal entries, unsorted rows, other algorithms'
calls in between and the edges of the contract.  Every GPU call is made twice on the one Graph: comp
and stats together, and stats alone.
"""
import ctypes as C
import functools
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from ldbc_graphalytics_platforms_graphblas_amd.graphio import CSR, csr_from_edges, rmat

DIRECTED_FIXTURES = {"example-directed": (7, 4, 6), "test-bfs-directed": (4, 7, 3), "test-cdlp-directed": (2, 5, 0),
                     "test-lcc-directed": (7, 4, 6), "test-pr-directed": (3, 48, 2), "test-sssp-directed": (4, 7, 3),
                     "test-wcc-directed": (5, 3, 3)}
UNDIRECTED_FIXTURES = ["example-undirected", "test-bfs-undirected", "test-cdlp-undirected", "test-lcc-undirected",
                       "test-pr-undirected", "test-sssp-undirected", "test-wcc-undirected"]
RMAT_SEED = 5


def edges_of(csr):
    rows = np.repeat(np.arange(csr.n, dtype=np.int64), np.diff(csr.rowptr.astype(np.int64)))
    return rows, csr.colidx.astype(np.int64)


def ref_scc(csr):
    """comp[n] uint64 by Tarjan's algorithm, iterative: an explicit stack of (vertex, next entry)."""
    n = csr.n
    rp = csr.rowptr.astype(np.int64).tolist()
    ci = csr.colidx.astype(np.int64).tolist()
    index = [-1] * n
    low = [0] * n
    on_stack = [False] * n
    comp = [0] * n
    stack, count = [], 0
    for root in range(n):
        if index[root] >= 0:
            continue
        index[root] = low[root] = count
        count += 1
        stack.append(root)
        on_stack[root] = True
        work = [(root, rp[root])]
        while work:
            v, p = work[-1]
            if p < rp[v + 1]:
                work[-1] = (v, p + 1)
                w = ci[p]
                if index[w] < 0:
                    index[w] = low[w] = count
                    count += 1
                    stack.append(w)
                    on_stack[w] = True
                    work.append((w, rp[w]))
                elif on_stack[w]:
                    low[v] = min(low[v], index[w])
                continue
            work.pop()
            if work:
                u = work[-1][0]
                low[u] = min(low[u], low[v])
            if low[v] == index[v]:
                members = []
                while True:
                    w = stack.pop()
                    on_stack[w] = False
                    members.append(w)
                    if w == v:
                        break
                label = min(members)
                for w in members:
                    comp[w] = label
    out = np.array(comp, dtype=np.uint64).reshape(n)
    out.setflags(write=False)
    return out


def ref_stats(comp):
    _, counts = np.unique(comp, return_counts=True)
    return np.array([len(counts), counts.max(initial=0), int((counts == 1).sum())], np.uint64)


def ring(n):
    v = np.arange(n)
    return csr_from_edges(n, v, (v + 1) % n, None, symmetric=False)


def path(n):
    """n - 1 -> n - 2 -> ... -> 0: no vertex is reached by a smaller id, so without the trim every vertex
    keeps its own colour (n one-vertex colour classes)."""
    v = np.arange(n - 1)
    return csr_from_edges(n, v + 1, v, None, symmetric=False)


def shuffled_rows(csr, seed):
    """The same graph with every row's entries in a random order."""
    rng = np.random.default_rng(seed)
    rows, _ = edges_of(csr)
    order = np.lexsort((rng.random(csr.nnz), rows))
    return CSR(csr.n, csr.rowptr.copy(), np.ascontiguousarray(csr.colidx[order]))


@functools.lru_cache(maxsize=None)
def planted_case():
    """(csr, comp by construction).  Blocks in shuffled order: one of 1 500 vertices, 60 of sizes drawn
    from 1 .. 64, 600 single vertices; a block of more than one vertex is a ring plus size / 2 chords
    inside it; of 12 000 drawn pairs those from a lower block to a higher one are kept; 50 diagonal
    entries; the ids permuted."""
    rng = np.random.default_rng(11)
    sizes = np.concatenate([[1500], rng.integers(1, 65, 60), np.ones(600, np.int64)])
    sizes = sizes[rng.permutation(len(sizes))]
    n = int(sizes.sum())
    start = np.concatenate([[0], np.cumsum(sizes)])
    block = np.repeat(np.arange(len(sizes)), sizes)
    src, dst = [], []
    for b, sz in enumerate(sizes.tolist()):
        if sz == 1:
            continue
        v = np.arange(sz)
        src += [start[b] + v, start[b] + rng.integers(0, sz, sz // 2)]
        dst += [start[b] + (v + 1) % sz, start[b] + rng.integers(0, sz, sz // 2)]
    a, b = rng.integers(0, n, 12000), rng.integers(0, n, 12000)
    keep = block[a] < block[b]
    loops = rng.integers(0, n, 50)
    src = np.concatenate(src + [a[keep], loops])
    dst = np.concatenate(dst + [b[keep], loops])
    perm = rng.permutation(n)
    csr = csr_from_edges(n, perm[src], perm[dst], None, symmetric=False)
    low = np.full(len(sizes), n, np.int64)
    np.minimum.at(low, block, perm)
    comp = np.empty(n, np.uint64)
    comp[perm] = low[block]
    comp.setflags(write=False)
    return csr, comp


@functools.lru_cache(maxsize=None)
def chain_case(name):
    csr = ring(4096) if name == "ring" else path(4096)
    comp = ref_scc(csr)
    return csr, comp, ref_stats(comp)


def ring_chain(rings, size, reverse):
    """`rings` rings of `size` vertices, ring b joined to ring b + 1 by one entry; reverse: the ids
    fall along the chain."""
    n = rings * size
    v = np.arange(n)
    src = np.concatenate([v, (np.arange(rings - 1) + 1) * size - 1])
    dst = np.concatenate([v - v % size + (v + 1) % size, (np.arange(rings - 1) + 1) * size])
    if reverse:
        src, dst = n - 1 - src, n - 1 - dst
    return csr_from_edges(n, src, dst, None, symmetric=False)


def hub_case(m, bridge):
    """A hub with m in-leaves (leaf -> hub) and m out-leaves (hub -> leaf), ids permuted, one isolated
    vertex; bridge: one entry out-leaf -> in-leaf, which closes a cycle of three through the hub."""
    n = 2 * m + 2
    perm = np.random.default_rng(m).permutation(n)
    hub, ins, outs = int(perm[0]), perm[1:m + 1], perm[m + 1:2 * m + 1]
    src = np.concatenate([ins, np.full(m, hub)])
    dst = np.concatenate([np.full(m, hub), outs])
    if bridge:
        src, dst = np.append(src, outs[7]), np.append(dst, ins[5])
    return csr_from_edges(n, src, dst, None, symmetric=False), hub, int(ins[5]), int(outs[7])


@functools.lru_cache(maxsize=None)
def rmat_case():
    csr = rmat(11, 8, RMAT_SEED, undirected=False)
    comp = ref_scc(csr)
    return csr, comp, ref_stats(comp)


# ------------------------------------------------------------------------------------- CPU

def test_abi_declares_exports_and_binds_scc():
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gx.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+gx_scc\s*\(\s*gx_graph\s*\*\s*g\s*,\s*uint64_t\s*\*\s*comp\s*,"
                     r"\s*uint64_t\s*\*\s*stats\s*\)", header)
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "gx_scc" in exported
    sig = {name: (res, args) for name, res, args in N.SIGNATURES}
    assert sig["gx_scc"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    assert callable(A.LA_SCC)
    assert all(isinstance(x, int) and x > 0 for x in (A.SCC_SHORT, A.SCC_LONG)) and A.SCC_SHORT <= A.SCC_LONG


def test_null_graph_is_refused_before_any_device_call():
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    comp = np.zeros(1, np.uint64)
    stats = np.zeros(3, np.uint64)
    assert N.lib().gx_scc(None, N.as_u64p(comp), N.as_u64p(stats)) == -2   # GX_NULL_POINTER
    assert b"gx_scc" in N.lib().gx_last_error()


def test_reference_matches_scipy_and_networkx():
    """2 048 vertices, 4 096 drawn pairs (seed 3, the source array first)."""
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(3)
    src = rng.integers(0, 2048, 4096)
    dst = rng.integers(0, 2048, 4096)
    csr = csr_from_edges(2048, src, dst, None, symmetric=False)
    comp = ref_scc(csr)
    np.testing.assert_array_equal(ref_stats(comp), [815, 1233, 813])
    rows, cols = edges_of(csr)
    M = sp.csr_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(2048, 2048))
    ncomp, theirs = csgraph.connected_components(M, directed=True, connection="strong")
    assert ncomp == 815
    low = np.full(ncomp, 2048, np.int64)
    np.minimum.at(low, theirs, np.arange(2048))
    np.testing.assert_array_equal(comp, low[theirs])
    G = nx.DiGraph()
    G.add_nodes_from(range(2048))
    G.add_edges_from(zip(rows.tolist(), cols.tolist()))
    want = np.empty(2048, np.uint64)
    for members in nx.strongly_connected_components(G):
        want[list(members)] = min(members)
    np.testing.assert_array_equal(comp, want)


def test_reference_on_the_ring_and_the_path():
    csr, comp, stats = chain_case("ring")
    np.testing.assert_array_equal(comp, np.zeros(4096))
    np.testing.assert_array_equal(stats, [1, 4096, 0])
    csr, comp, stats = chain_case("path")
    assert csr.nnz == 4095
    np.testing.assert_array_equal(comp, np.arange(4096))
    np.testing.assert_array_equal(stats, [4096, 1, 4096])


@pytest.mark.parametrize("name", sorted(DIRECTED_FIXTURES))
def test_reference_on_the_directed_fixtures(fixture_graphs, name):
    g = fixture_graphs(name)
    assert g.directed
    assert tuple(int(x) for x in ref_stats(ref_scc(g.csr))) == DIRECTED_FIXTURES[name]


def test_planted_components_are_what_the_reference_finds():
    csr, comp = planted_case()
    _, counts = np.unique(comp, return_counts=True)
    assert counts.max() >= 1000 and ((counts >= 2) & (counts <= 64)).sum() >= 40 and (counts == 1).sum() >= 500
    rows, cols = edges_of(csr)
    assert (rows == cols).sum() >= 40
    np.testing.assert_array_equal(ref_scc(csr), comp)


def test_rmat_case_has_a_giant_and_singletons():
    csr, comp, stats = rmat_case()
    assert int(stats[1]) >= csr.n // 8 and int(stats[2]) >= 100


# ------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    c = Context(0)
    yield c
    c.close()


def check_scc(G, comp, tag="", calls=2):
    """comp and stats together, then stats alone; `calls` times on the one Graph."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    stats = ref_stats(comp)
    for call in range(calls):
        got, st = A.LA_SCC(G, comp=True, stats=True)
        assert got.dtype == np.uint64 and st.dtype == np.uint64
        np.testing.assert_array_equal(got, comp, err_msg=f"{tag} comp, call {call + 1}")
        np.testing.assert_array_equal(st, stats, err_msg=f"{tag} stats, call {call + 1}")
        np.testing.assert_array_equal(A.LA_SCC(G, comp=False, stats=True), stats, err_msg=f"{tag} stats alone")


def run_scc(ctx, csr, comp, directed=True, tag=""):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    G = A.Graph(ctx, csr, directed)
    try:
        check_scc(G, comp, tag)
    finally:
        G.close()


PHASES = [{}, {"GX_SCC_PIVOT": "0"}, {"GX_SCC_TRIM": "0"}, {"GX_SCC_PIVOT": "0", "GX_SCC_TRIM": "0"}]
PHASE_IDS = ["default", "pivot0", "trim0", "pivot0-trim0"]
TIERS = [{}, {"GX_SCC_SHORT": "4", "GX_SCC_LONG": "16"}, {"GX_SCC_SHORT": "1", "GX_SCC_LONG": "4096"},
         {"GX_SCC_SHORT": "4096", "GX_SCC_LONG": "4096"}]
TIER_IDS = ["default", "short4-long16", "all-wave", "all-thread"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DIRECTED_FIXTURES))
def test_gpu_directed_fixtures(ctx, fixture_graphs, name):
    g = fixture_graphs(name)
    comp = ref_scc(g.csr)
    assert tuple(int(x) for x in ref_stats(comp)) == DIRECTED_FIXTURES[name]
    run_scc(ctx, g.csr, comp, True, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", UNDIRECTED_FIXTURES)
def test_gpu_undirected_fixtures_equal_wcc(ctx, fixture_graphs, name):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    g = fixture_graphs(name)
    assert not g.directed
    F = A.Graph(ctx, g.csr, False)
    try:
        wcc = A.WeaklyConnectedComponents(F)
    finally:
        F.close()
    run_scc(ctx, g.csr, wcc, False, name)


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", PHASES + [{"GX_SCC_BATCH": "1"}, TIERS[3], TIERS[2], {"GX_SCC_SOLO": "0"}],
                         ids=PHASE_IDS + ["batch1", "all-thread", "all-wave", "solo0"])
def test_gpu_planted_components_under_every_phase_setting(ctx, monkeypatch, knobs):
    for key, v in knobs.items():
        monkeypatch.setenv(key, v)
    csr, comp = planted_case()
    run_scc(ctx, csr, comp, True, str(knobs))


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{"GX_SCC_SOLO": "0"}, {}, {"GX_SCC_SOLO": "1"}, {"GX_SCC_BATCH": "1"},
                                   {"GX_SCC_BATCH": "512"}, {"GX_SCC_SOLO": "0", "GX_SCC_BATCH": "1"},
                                   {"GX_SCC_SOLO": "100000"}],
                         ids=["solo0", "default", "solo1", "batch1", "batch512", "solo0-batch1", "solo-all"])
@pytest.mark.parametrize("name,phase", [("ring", {}), ("ring", {"GX_SCC_PIVOT": "0"}), ("path", {}),
                                        ("path", {"GX_SCC_TRIM": "0"})],
                         ids=["ring", "ring-pivot0", "path", "path-trim0"])
def test_gpu_long_chains_under_every_schedule(ctx, monkeypatch, name, phase, knobs):
    """The 4 096-ring: the pivot's 4 095 levels each way, or without the pivot one colour going all the
    way round.  The 4 096-path: 2 048 trim rounds, or without the trim 4 096 one-vertex colour classes.
    The same outputs whether one workgroup runs the rounds, the grid does, or they alternate."""
    for key, v in {**phase, **knobs}.items():
        monkeypatch.setenv(key, v)
    csr, comp, _ = chain_case(name)
    run_scc(ctx, csr, comp, True, f"{name} {phase} {knobs}")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{}, {"GX_SCC_PIVOT": "0"}, {"GX_SCC_PIVOT": "0", "GX_SCC_SOLO": "0"}],
                         ids=["default", "pivot0", "pivot0-solo0"])
@pytest.mark.parametrize("reverse", [False, True], ids=["rising", "falling"])
def test_gpu_colour_phase_worst_and_best_order(ctx, monkeypatch, reverse, knobs):
    """16 rings of 32 in a chain.  Ids rising along it: one colour floods everything and 16 outer
    iterations each take one ring; falling: every ring keeps its own colour and one iteration suffices."""
    for key, v in knobs.items():
        monkeypatch.setenv(key, v)
    csr = ring_chain(16, 32, reverse)
    comp = ref_scc(csr)
    np.testing.assert_array_equal(ref_stats(comp), [16, 32, 0])
    run_scc(ctx, csr, comp, True, f"reverse {reverse}")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", TIERS, ids=TIER_IDS)
@pytest.mark.parametrize("bridge", [False, True], ids=["plain", "bridge"])
def test_gpu_hub_is_appended_exactly_once(ctx, monkeypatch, bridge, knobs):
    """Round 1 removes the 6 000 leaves, which take the hub's two words to zero in the same round: the
    hub leaves once (twice would take it out of the alive count twice and the count would wrap).  With
    one entry out-leaf -> in-leaf the hub and those two stay and form a component of three."""
    for key, v in knobs.items():
        monkeypatch.setenv(key, v)
    m = 3000
    csr, hub, leaf_in, leaf_out = hub_case(m, bridge)
    want = np.arange(csr.n, dtype=np.uint64)
    if bridge:
        want[[hub, leaf_in, leaf_out]] = min(hub, leaf_in, leaf_out)
    np.testing.assert_array_equal(ref_scc(csr), want)
    np.testing.assert_array_equal(ref_stats(want), [6000, 3, 5999] if bridge else [6002, 1, 6002])
    for solo in (None, "0"):
        if solo is not None:
            monkeypatch.setenv("GX_SCC_SOLO", solo)
        run_scc(ctx, csr, want, True, f"bridge {bridge} solo {solo}")


@pytest.mark.gpu
def test_gpu_diagonal_entries_change_nothing(ctx, fixture_graphs, monkeypatch):
    plain = fixture_graphs("test-pr-directed").csr
    rows, cols = edges_of(plain)
    assert (rows != cols).all()
    loops_at = np.arange(0, plain.n, 3)
    loops = csr_from_edges(plain.n, np.concatenate([rows, loops_at]), np.concatenate([cols, loops_at]), None,
                           symmetric=False)
    assert loops.nnz == plain.nnz + len(loops_at)
    comp = ref_scc(plain)
    np.testing.assert_array_equal(ref_scc(loops), comp)
    run_scc(ctx, loops, comp, True, "loops")
    # a vertex with a diagonal entry and nothing else, beside a cycle of three
    lone = csr_from_edges(5, [0, 1, 2, 3], [1, 2, 0, 3], None, symmetric=False)
    want = np.array([0, 0, 0, 3, 4], np.uint64)
    np.testing.assert_array_equal(ref_scc(lone), want)
    for trim in ("1", "0"):
        monkeypatch.setenv("GX_SCC_TRIM", trim)
        run_scc(ctx, lone, want, True, f"lone trim {trim}")


@pytest.mark.gpu
def test_gpu_unsorted_rows_give_the_same_arrays(ctx):
    csr, comp = planted_case()
    mixed = shuffled_rows(csr, 9)
    assert (mixed.colidx != csr.colidx).any()
    run_scc(ctx, mixed, comp, True, "unsorted")


@pytest.mark.gpu
def test_gpu_rmat_with_other_calls_between(ctx):
    """gx_bfs, gx_wcc, gx_cdlp and gx_msbfs between the gx_scc calls return what they return, call for
    call, on a fresh graph that never saw gx_scc; every component lies inside one weakly connected one."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    csr, comp, stats = rmat_case()
    assert int(stats[1]) >= csr.n // 8 and int(stats[2]) >= 100
    hub = int(np.argmax(np.diff(csr.rowptr.astype(np.int64))))
    sources = [hub, 0, csr.n - 1]

    def others(X, i):
        return [A.LA_BFS(X, sources[i]), A.WeaklyConnectedComponents(X), A.LA_CDLP(X, 3 + i), A.LA_MSBFS(X, sources)]

    F = A.Graph(ctx, csr, True)
    try:
        fresh = [others(F, i) for i in range(3)]
    finally:
        F.close()
    G = A.Graph(ctx, csr, True)
    try:
        for call in range(3):
            check_scc(G, comp, f"call {call + 1}", calls=1)
            got = others(G, call)
            for a, b in zip(got, fresh[call]):
                np.testing.assert_array_equal(a, b)
            again = A.LA_SCC(G)
            np.testing.assert_array_equal(again, comp)
            wcc = got[1]
            assert (again >= wcc).all()
            np.testing.assert_array_equal(wcc, wcc[again.astype(np.int64)])   # one label of gx_wcc per component
    finally:
        G.close()


@pytest.mark.gpu
def test_gpu_contract_edges(ctx, fixture_graphs):
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    L = N.lib()
    g = fixture_graphs("example-directed")
    n = g.csr.n
    comp = np.full(n, 7777, np.uint64)
    stats = np.full(3, 77, np.uint64)
    want = ref_scc(g.csr)
    G = A.Graph(ctx, g.csr, True)
    try:
        assert L.gx_scc(G.handle, None, None) == -2   # nothing to write to: GX_NULL_POINTER
        assert b"gx_scc" in L.gx_last_error()
        assert (comp == 7777).all() and (stats == 77).all()
        with pytest.raises(N.GxError) as err:
            A.LA_SCC(G, comp=False, stats=False)
        assert err.value.code == -2
        # each output alone equals its half of the full call
        full_comp, full_stats = A.LA_SCC(G, comp=True, stats=True)
        np.testing.assert_array_equal(full_comp, want)
        np.testing.assert_array_equal(full_stats, ref_stats(want))
        assert L.gx_scc(G.handle, N.as_u64p(comp), None) == 0
        np.testing.assert_array_equal(comp, full_comp)
        assert (stats == 77).all()
        assert L.gx_scc(G.handle, None, N.as_u64p(stats)) == 0
        np.testing.assert_array_equal(stats, full_stats)
        np.testing.assert_array_equal(A.LA_SCC(G), full_comp)
    finally:
        G.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5])
def test_gpu_no_entries_and_a_single_diagonal_entry(ctx, n):
    csr = csr_from_edges(n, [], [], None, symmetric=False)
    loop = csr_from_edges(n, [0], [0], None, symmetric=False)
    for case in (csr, loop):
        for directed in (True, False):
            run_scc(ctx, case, np.arange(n, dtype=np.uint64), directed, f"n {n} nnz {case.nnz} directed {directed}")
