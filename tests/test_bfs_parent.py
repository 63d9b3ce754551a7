"""BFS parent tree (gx_bfs_parent / LA_BFS_parent) and the MIN_SECONDI_INT64 semiring.

parent[src] = src, -1 = unreachable, else the SMALLEST u with A(u, v) stored one level up: the
result is unique, so every comparison is bit for bit.  The reference is numpy on the oracle's
levels (ref_parents); a hand-written tree pins it on the CPU, and check_tree validates every
GPU result without it.  CPU: the ABI, the null-pointer error, the references.  GPU: fixtures,
R-MAT over three calls on one graph (push, then the transpose / the hub-first copy), the
direction and copy knobs, ties (only the minimum of many valid parents passes), rows around
the thread / wave / chunk thresholds, depth, the semiring against numpy and LAGraph's loop
written op by op.
"""
import ctypes as C
import functools
import re
import subprocess

import numpy as np
import pytest

from conftest import FIXTURES, ROOT, internal_index
from oracle import oracle as O
from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges, load_graphalytics, rmat

MAX = np.iinfo(np.int64).max


def edges_of(csr):
    rows = np.repeat(np.arange(csr.n, dtype=np.int64), np.diff(csr.rowptr.astype(np.int64)))
    return rows, csr.colidx.astype(np.int64)


def ref_parents(csr, s):
    """(level, parent) from the oracle's levels: the minimum over the edges one level down."""
    n = csr.n
    lev = O.bfs(csr, s)
    rows, cols = edges_of(csr)
    ok = (lev[rows] != MAX) & (lev[cols] != MAX)
    ok[ok] = lev[cols[ok]] == lev[rows[ok]] + 1
    par = np.full(n, MAX)
    np.minimum.at(par, cols[ok], rows[ok])
    par[lev == MAX] = -1
    par[s] = s
    return lev, par


def check_tree(csr, s, level, parent):
    """Independent of ref_parents: every reached v != s hangs on a stored edge from one level up."""
    n = csr.n
    assert parent[s] == s and level[s] == 0
    reached = level != MAX
    np.testing.assert_array_equal(parent[~reached], -1)
    v = np.nonzero(reached)[0]
    v = v[v != s]
    p = parent[v]
    assert ((p >= 0) & (p < n)).all()
    np.testing.assert_array_equal(level[p], level[v] - 1)
    rows, cols = edges_of(csr)
    assert np.isin(p * n + v, rows * n + cols).all()


def numpy_secondi(csr, up, vxm, t0):
    """t = M min.secondi u without mask or accumulator: (values, presence).  vxm contracts A's
    row index, mxv its column index; T0 swaps them."""
    rows, cols = edges_of(csr)
    out, k = (cols, rows) if vxm != t0 else (rows, cols)
    keep = np.ones(len(k), bool) if up is None else up[k] != 0
    t = np.full(csr.n, MAX)
    np.minimum.at(t, out[keep], k[keep])
    return t, t != MAX


def numpy_finish(t, hit, mask, desc, w, wp):
    """w<mask> (+)= t as include/gx.h states it, the monoid being min with identity INT64_MAX."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    n = len(t)
    allowed = np.ones(n, bool) if mask is None else (mask != 0) != bool(desc & A.DESC_MASK_COMP)
    old = np.ones(n, bool) if wp is None else wp != 0
    val = np.where(hit, t, MAX)
    pres = hit.copy()
    if desc & A.DESC_ACCUM:
        val = np.where(old, np.where(hit, np.minimum(w, t), w), val)
        pres = pres | old
    if desc & A.DESC_REPLACE:
        val, pres = np.where(allowed, val, MAX), pres & allowed
    else:
        val, pres = np.where(allowed, val, w), np.where(allowed, pres, old)
    return val, pres.astype(np.uint8)


# ------------------------------------------------------------------------------------- CPU

def test_abi_declares_exports_and_binds_gx_bfs_parent():
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gx.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+gx_bfs_parent\s*\(\s*gx_graph\s*\*\s*g\s*,\s*uint64_t\s+src\s*,\s*int64_t\s*\*\s*level"
                     r"\s*,\s*int64_t\s*\*\s*parent\s*\)", header)
    assert re.search(r"#define\s+GX_MIN_SECONDI_INT64\s+5\b", header)
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True).stdout
    assert "gx_bfs_parent" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    sig = {name: (res, args) for name, res, args in N.SIGNATURES}
    assert sig["gx_bfs_parent"] == (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)])
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    assert A.MIN_SECONDI_INT64 == 5 and A._OUT_DTYPE[A.MIN_SECONDI_INT64] is np.int64


def test_null_graph_is_refused_before_any_device_call():
    from ldbc_graphalytics_platforms_graphblas_amd import _native as N
    level = np.zeros(1, np.int64)
    parent = np.zeros(1, np.int64)
    assert N.lib().gx_bfs_parent(None, 0, N.as_i64p(level), N.as_i64p(parent)) == -2   # GX_NULL_POINTER
    assert b"gx_bfs_parent" in N.lib().gx_last_error()


def test_reference_matches_hand_written_tree():
    """example-directed from vertex 1 (internal ids = id - 1): 1 -> {3, 5}; 4 hangs on 5 alone (2, 6,
    7 and 9 also point at it but are unreached); 8 has two parents one level up, 3 and 5, and
    takes 3; 10 hangs on 3 (2 is unreached)."""
    g = load_graphalytics(FIXTURES, "example-directed")
    s = internal_index(g.mapping, int(g.param("bfs", "source-vertex")))
    assert s == 0
    lev, par = ref_parents(g.csr, s)
    np.testing.assert_array_equal(lev, [0, MAX, 1, 2, 1, MAX, MAX, 2, MAX, 2])
    np.testing.assert_array_equal(par, [0, -1, 0, 4, 0, -1, -1, 2, -1, 2])
    check_tree(g.csr, s, lev, par)
    bad = par.copy()
    bad[7] = 4   # a valid parent that is not the smallest: the tree check passes, the comparison must not
    check_tree(g.csr, s, lev, bad)
    assert not np.array_equal(bad, par)


@pytest.mark.parametrize("name", ["example-directed", "example-undirected"])
def test_secondi_reference_matches_dense_restatement(name):
    csr = load_graphalytics(FIXTURES, name).csr
    n = csr.n
    S = np.zeros((n, n), bool)
    S[edges_of(csr)] = True
    up = (np.arange(n) % 3 != 1).astype(np.uint8)
    for vxm in (False, True):
        for t0 in (False, True):
            M = S.T if vxm != t0 else S
            for u in (None, up):
                t, hit = numpy_secondi(csr, u, vxm, t0)
                for i in range(n):
                    js = np.nonzero(M[i] & (True if u is None else u != 0))[0]
                    assert hit[i] == (len(js) > 0) and t[i] == (js.min() if len(js) else MAX)


# ------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    c = Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def rmat_case(directed):
    """The sizes tests/test_gpu_parity.py runs BFS on; (csr, sources, their references)."""
    csr = rmat(12, 8, 3, undirected=False) if directed else rmat(14, 16, 4)
    srcs = (int(np.argmax(np.diff(csr.rowptr.astype(np.int64)))), 1)
    return csr, srcs, {s: ref_parents(csr, s) for s in srcs}


def run_and_check(ctx, csr, directed, s, calls=3, ref=None):
    """`calls` gx_bfs_parent calls on one graph (the first on its own rows, push when directed;
    the later ones over the transpose or on the hub-first copy), each equal to the reference and
    a valid tree; then gx_bfs on the same graph gives the same levels."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    want_level, want_parent = ref if ref is not None else ref_parents(csr, s)
    G = A.Graph(ctx, csr, directed)
    try:
        for call in range(calls):
            level, parent = A.LA_BFS_parent(G, s)
            assert level.dtype == np.int64 and parent.dtype == np.int64
            np.testing.assert_array_equal(level, want_level, err_msg=f"level, call {call + 1}")
            np.testing.assert_array_equal(parent, want_parent, err_msg=f"parent, call {call + 1}")
            check_tree(csr, s, level, parent)
        np.testing.assert_array_equal(A.LA_BFS(G, s), level)
    finally:
        G.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["example-directed", "example-undirected", "test-bfs-directed",
                                  "test-bfs-undirected"])
def test_gpu_fixtures(ctx, fixture_graphs, name):
    g = fixture_graphs(name)
    s = internal_index(g.mapping, int(g.param("bfs", "source-vertex")))
    run_and_check(ctx, g.csr, g.directed, s)


@pytest.mark.gpu
@pytest.mark.parametrize("directed", [False, True])
def test_gpu_rmat_three_calls(ctx, directed):
    csr, srcs, refs = rmat_case(directed)
    for s in srcs:
        run_and_check(ctx, csr, directed, s, calls=3, ref=refs[s])


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"GX_BFS_ALPHA": "1", "GX_BFS_BETA": "1000"},
                                 {"GX_BFS_ALPHA": "1000", "GX_BFS_BETA": "1"},
                                 {"GX_HUB": "2"}, {"GX_HUB": "2", "GX_HUB_SORT": "0"},
                                 {"GX_BFS_DEVICE": "0"},
                                 {"GX_BFS_PARENT_PUSH": "1"}, {"GX_BFS_PARENT_PUSH": "1", "GX_HUB": "2"}],
                         # env4 was the scatter remap, since removed: the others keep their ids
                         ids=["env0", "env1", "env2", "env3", "env5", "env6", "env7"])
def test_gpu_parents_do_not_depend_on_direction_or_copy(ctx, monkeypatch, env):
    """Top-down or bottom-up levels, the hub-first copy (sorted rows or not), host-driven levels,
    and the push form of the parent pass where pull is the default."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for directed in (False, True):
        csr, srcs, refs = rmat_case(directed)
        run_and_check(ctx, csr, directed, srcs[0], calls=2, ref=refs[srcs[0]])


def layered(width, layers, directed, seed):
    """`layers` layers of `width` vertices under a random id permutation, consecutive layers
    completely connected, and a source joined to layer 0: every vertex past layer 0 has `width`
    valid parents and only the smallest is right."""
    n = width * layers + 1
    perm = np.random.default_rng(seed).permutation(n)
    lay = perm[:-1].reshape(layers, width)
    src = [np.full(width, perm[-1])] + [np.repeat(lay[k], width) for k in range(layers - 1)]
    dst = [lay[0]] + [np.tile(lay[k + 1], width) for k in range(layers - 1)]
    return csr_from_edges(n, np.concatenate(src), np.concatenate(dst), None, symmetric=not directed), int(perm[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("width,layers", [(70, 6),     # across a wave boundary, past the thread-per-row limit
                                          (40, 4),     # rows one thread scans
                                          (300, 3)])   # rows of two chunks, combined by atomicMin
def test_gpu_ties_take_the_smallest_parent(ctx, width, layers, directed):
    csr, s = layered(width, layers, directed, seed=width)
    lev, par = ref_parents(csr, s)
    assert lev.max() == layers and len(np.unique(par)) <= layers + 1
    run_and_check(ctx, csr, directed, s, ref=(lev, par))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["undirected", "in", "out"])
def test_gpu_star_rows_span_chunks(ctx, form):
    """A hub with 1 000 leaves (four chunks of 256) and an isolated vertex: n = 1 002."""
    n, hub = 1002, 500
    leaves = np.array([v for v in range(n - 1) if v != hub])
    hubs = np.full(len(leaves), hub)
    src, dst = (leaves, hubs) if form == "in" else (hubs, leaves)
    csr = csr_from_edges(n, src, dst, None, symmetric=form == "undirected")
    for s in (hub, 7, n - 1):
        lev, par = ref_parents(csr, s)
        if s == n - 1:
            assert par[s] == s and (np.delete(par, s) == -1).all()
        run_and_check(ctx, csr, form != "undirected", s, ref=(lev, par))


@pytest.mark.gpu
@pytest.mark.parametrize("directed", [False, True])
def test_gpu_single_vertex(ctx, directed):
    csr = csr_from_edges(1, [], [], None, symmetric=not directed)
    run_and_check(ctx, csr, directed, 0, ref=(np.zeros(1, np.int64), np.zeros(1, np.int64)))


@pytest.mark.gpu
def test_gpu_deep_path(ctx):
    """More levels than the device-driven loop's first batch: a 3 000-vertex path, one vertex apart."""
    n = 3000
    perm = np.random.default_rng(2).permutation(n)
    csr = csr_from_edges(n + 1, perm[:-1], perm[1:], None, symmetric=True)   # vertex n isolated
    for s, calls in ((int(perm[0]), 2), (int(perm[n // 2]), 1), (n, 1)):
        run_and_check(ctx, csr, False, s, calls=calls)


def op_cases(n, rng):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    sparse = (rng.random(n) < 0.3).astype(np.uint8)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    w0 = rng.integers(-5, n, n).astype(np.int64)
    wp0 = (rng.random(n) < 0.5).astype(np.uint8)
    for up in (sparse, None):
        for t0 in (0, A.DESC_T0):
            yield up, None, t0, None, None
            yield up, None, t0, None, np.zeros(n, np.uint8)
            for md in (0, A.DESC_MASK_COMP, A.DESC_REPLACE, A.DESC_MASK_COMP | A.DESC_REPLACE):
                yield up, mask, t0 | md, w0, wp0
            yield up, None, t0 | A.DESC_ACCUM, w0, wp0
            yield up, mask, t0 | A.DESC_ACCUM | A.DESC_MASK_COMP | A.DESC_REPLACE, w0, wp0
            yield up, None, t0 | A.DESC_ACCUM, w0, None


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["rmat-directed", "example-undirected"])
def test_gpu_min_secondi_ops_match_numpy(ctx, fixture_graphs, which):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    if which == "rmat-directed":
        csr, directed = rmat_case(True)[0], True
    else:
        csr, directed = fixture_graphs(which).csr, False
    n = csr.n
    G = A.Graph(ctx, csr, directed)
    try:
        for vxm in (True, False):
            for up, mask, desc, w0, wp0 in op_cases(n, np.random.default_rng(n)):
                t, hit = numpy_secondi(csr, up, vxm, bool(desc & A.DESC_T0))
                want, wantp = numpy_finish(t, hit, mask, desc, np.zeros(n, np.int64) if w0 is None else w0, wp0)
                got, gotp = (A.vxm if vxm else A.mxv)(G, A.MIN_SECONDI_INT64, None, up, mask, desc, w0, wp0)
                what = f"vxm={vxm} desc={desc} u_present={'sparse' if up is not None else None}"
                assert got.dtype == np.int64
                if wp0 is None:
                    assert gotp is None
                    np.testing.assert_array_equal(got, want, err_msg=what)
                else:
                    np.testing.assert_array_equal(gotp, wantp, err_msg="presence " + what)
                    np.testing.assert_array_equal(got[gotp != 0], want[wantp != 0], err_msg=what)
    finally:
        G.close()


@pytest.mark.gpu
@pytest.mark.parametrize("directed", [True, False])
def test_gpu_lagraph_loop_op_by_op(ctx, directed):
    """LAGraph's parent BFS, one GraphBLAS call at a time: q<!pi, replace> = q min.secondi A, then
    pi<q> = q, until q is empty -- a second implementation of the definition gx_bfs_parent
    states.  From the largest hub an R-MAT graph is a handful of levels deep."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    csr, srcs, refs = rmat_case(directed)
    s = srcs[0]
    assert refs[s][0][refs[s][0] != MAX].max() <= 10
    G = A.Graph(ctx, csr, directed)
    try:
        level, parent = A.LA_BFS_parent(G, s)
        n = csr.n
        pi = np.full(n, -1, np.int64)
        pi_present = np.zeros(n, np.uint8)
        pi[s], pi_present[s] = s, 1
        q_present = pi_present.copy()
        steps = 0
        while q_present.any():
            q, q_present = A.vxm(G, A.MIN_SECONDI_INT64, None, q_present, pi_present,
                                 A.DESC_MASK_COMP | A.DESC_REPLACE, None, np.zeros(n, np.uint8))
            pi[q_present != 0] = q[q_present != 0]
            pi_present |= q_present
            steps += 1
            assert steps <= 12
        np.testing.assert_array_equal(pi, parent)
        np.testing.assert_array_equal(parent, refs[s][1])
        np.testing.assert_array_equal(level, refs[s][0])
    finally:
        G.close()
