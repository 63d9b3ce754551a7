"""Call histories: one resident graph through mixed sequences of calls.

libgx keeps state on a gx_graph between calls (DESIGN.md 2 lists it): the transpose and the BFS
call count, the level-step hint, the hub-first copy and its remap scratch, the SSSP layout with
its captured step graph and replay hint, the CDLP cache, the PageRank plan -- and per device the
grow-only scratch, the rocPRIM temporary and the staging buffers.  tests/test_gpu_parity.py's
gpu_run opens a fresh Graph per call, so it reaches first-call paths only; here every sequence
runs on ONE Graph and every result is checked as it arrives.

run_sequence(ctx, csr, directed, steps): a step is (name, params) with name one of bfs,
bfs_parent, bc, sssp, pr, wcc, cdlp, lcc, mxv, vxm, or a control step: ("timing", on) calls
ctx.set_kernel_timing, ("env", {VAR: value or None}) sets / deletes variables through monkeypatch.
Expected values are the oracle's (oracle/oracle.py), for bfs_parent and bc the references of
tests/test_bfs_parent.py (ref_parents, check_tree) and tests/test_betweenness.py (ref_bc, compare,
whose tolerance is rtol_for), memoised per (graph, name, params).  Bars: BFS, BFS-parent, SSSP,
WCC, CDLP, LCC and the min / any / pair semirings bit for bit; PageRank and PLUS_SECOND within
1e-12 relative; BC by test_betweenness.compare.

A wrong value fails with the step index, the steps made so far and the verdict of that ONE call
on a fresh Graph ("fresh graph agrees with the oracle: yes" = the history is at fault, "no" = the
kernel is).  The fresh call is made once, after a wrong value; an error of the library (GxError)
propagates as it is and nothing more runs.

Inputs (built here, their properties asserted on the CPU by test_inputs_have_the_properties):
  U  undirected R-MAT scale 12, edge factor 8, weighted, renamed to random ids below 4099
  D  directed R-MAT scale 11, edge factor 8, weighted, renamed to random ids below 2053
  T  a star of 10 000 leaves (CDLP's huge tier) plus 400 random edges among the leaves and an
     isolated vertex; undirected, and directed (Td: half the spokes point in, half out)
  P  a weighted path of 3 000 vertices in random id order plus an isolated vertex, undirected
  DP D plus a directed path of 3 000 new vertices whose last vertex points at D's hub
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import oracle as O
from test_betweenness import compare as bc_compare, ref_bc
from test_bfs_parent import check_tree, ref_parents

PR_RTOL = 1e-12
ALGS = ("bfs", "bfs_parent", "bc", "sssp", "pr", "wcc", "cdlp", "lcc", "mxv", "vxm")
SEMIRINGS = ("PLUS_SECOND_FP64", "MIN_SECOND_UINT64", "ANY_PAIR_BOOL", "MIN_PLUS_FP64", "PLUS_PAIR_INT64")
CDLP_ITERS = (0, 1, 2, 3, 17, 5, 40, 2, 10, 40)                                    # sequence (c)
PR_PARAMS = ((0.85, 10), (0.5, 3), (0.85, 1), (0.99, 7), (0.85, 10), (0.85, 2))    # sequence (d)


# ------------------------------------------------------------------------------------ inputs

def _edges(csr):
    rows = np.repeat(np.arange(csr.n, dtype=np.int64), np.diff(csr.rowptr.astype(np.int64)))
    return rows, csr.colidx.astype(np.int64), csr.vals


def _degree(csr):
    """Out- plus in-degree (an undirected graph stores both directions: twice its degree)."""
    rows, cols, _ = _edges(csr)
    return np.bincount(rows, minlength=csr.n) + np.bincount(cols, minlength=csr.n)


def _case(name, csr, directed, **vertices):
    deg = _degree(csr)
    iso = np.nonzero(deg == 0)[0]
    c = SimpleNamespace(name=name, csr=csr, directed=directed, n=csr.n,
                        hub=int(np.argmax(np.diff(csr.rowptr.astype(np.int64)))),
                        isolated=int(iso[0]) if len(iso) else None)
    c.__dict__.update(vertices)
    if "far" not in vertices:   # the deepest vertex the hub reaches
        lev = O.bfs(csr, c.hub)
        c.far = int(np.argmax(np.where(lev == np.iinfo(np.int64).max, -1, lev)))
    c.random = int(np.random.default_rng(csr.n).integers(0, csr.n))
    return c


def _renamed_rmat(scale, ef, seed, n, undirected):
    """tests/test_gpu_parity.py's _odd_rmat with weights (and its directed form): the R-MAT
    graph's 2^scale vertices renamed to random ids below n, n no multiple of 64; the ids no
    vertex got stay isolated."""
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges, rmat
    csr = rmat(scale, ef, seed, undirected=undirected, weighted=True)
    u, v, w = _edges(csr)
    ids = np.random.default_rng(11).permutation(n)[:csr.n]
    keep = u < v if undirected else np.ones(len(u), bool)
    return csr_from_edges(n, ids[u[keep]], ids[v[keep]], w[keep], symmetric=undirected)


def _path_ids(count, seed):
    return np.random.default_rng(seed).permutation(count)


@functools.lru_cache(maxsize=None)
def case(name):
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
    if name == "U":   # seed 61: label propagation settles after 7 iterations (most seeds oscillate)
        return _case("U", _renamed_rmat(12, 8, 61, 4099, True), False)
    if name == "D":
        return _case("D", _renamed_rmat(11, 8, 3, 2053, False), True)
    if name in ("T", "Td"):
        directed = name == "Td"
        rng = np.random.default_rng(5)
        leaves = np.arange(1, 10001)
        a, b = rng.integers(1, 10001, 400), rng.integers(1, 10001, 400)
        out = leaves % 2 == 0 if directed else np.ones(10000, bool)
        src = np.concatenate([np.where(out, 0, leaves), a[a != b]])
        dst = np.concatenate([np.where(out, leaves, 0), b[a != b]])
        csr = csr_from_edges(10002, src, dst, rng.random(len(src)) + 0.25, symmetric=not directed)
        return _case(name, csr, directed)   # vertex 10001 is isolated
    if name == "P":
        perm = _path_ids(3000, 2)
        w = np.random.default_rng(3).random(2999) + 0.25
        csr = csr_from_edges(3001, perm[:-1], perm[1:], w, symmetric=True)
        return _case("P", csr, False, hub=int(perm[0]), end=int(perm[0]), middle=int(perm[1500]), far=int(perm[-1]))
    if name == "DP":
        d = case("D")
        u, v, w = _edges(d.csr)
        path = d.n + _path_ids(3000, 4)
        src = np.concatenate([u, path])
        dst = np.concatenate([v, path[1:], [d.hub]])
        wts = np.concatenate([w, np.random.default_rng(6).random(3000) + 0.25])
        csr = csr_from_edges(d.n + 3000, src, dst, wts, symmetric=False)
        return _case("DP", csr, True, hub=d.hub, end=int(path[0]), middle=int(path[1500]), far=int(path[-1]))
    raise KeyError(name)


# ------------------------------------------------------------------------- expected values

def _key(params):
    return tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple, np.ndarray)) else v) for k, v in params.items()))


def _op_inputs(csr, semiring):
    """The u and u_present of an mxv / vxm step: fixed by the graph's size and the semiring."""
    sr = getattr(O, semiring)
    rng = np.random.default_rng(csr.n + sr)
    present = (rng.random(csr.n) < 0.6).astype(np.uint8)
    if sr == O.MIN_SECOND_UINT64:
        return rng.integers(0, 1 << 40, csr.n).astype(np.uint64), present
    if sr in (O.PLUS_SECOND_FP64, O.MIN_PLUS_FP64):
        return rng.random(csr.n), present
    return None, present


_memo = {}


def expected(c, name, params):
    """The oracle's value of one step, computed once per (graph, name, params)."""
    key = (c.name, name, _key(params))
    if key not in _memo:
        csr, p = c.csr, params
        if name == "bfs":
            want = O.bfs(csr, p["source"])
        elif name == "bfs_parent":
            want = ref_parents(csr, p["source"])
        elif name == "bc":
            want = ref_bc(csr, list(p["sources"]))
        elif name == "sssp":
            want = O.sssp(csr, p["source"])
        elif name == "pr":
            want = O.pagerank(csr, c.directed, p["damping"], p["iters"])
        elif name == "wcc":
            want = O.wcc(csr)
        elif name == "cdlp":
            want = O.cdlp(csr, c.directed, p["iters"])
        elif name == "lcc":
            want = O.lcc(csr, c.directed)
        elif name in ("mxv", "vxm"):
            u, up = _op_inputs(csr, p["semiring"])
            want = O.mxv(csr, getattr(O, p["semiring"]), u, up, None, 0, None, np.zeros(csr.n, np.uint8),
                         vxm=name == "vxm")
        else:
            raise AssertionError(name)
        for a in want if isinstance(want, tuple) else (want,):
            a.setflags(write=False)   # shared among the tests: nobody changes it
        _memo[key] = want
    return _memo[key]


def check(c, name, params, got, want):
    """The project's bar for one step's result; AssertionError on a mismatch."""
    if name == "bfs_parent":
        np.testing.assert_array_equal(got[0], want[0], err_msg="level")
        np.testing.assert_array_equal(got[1], want[1], err_msg="parent")
        check_tree(c.csr, params["source"], got[0], got[1])
    elif name == "bc":
        bc_compare(c.csr, list(params["sources"]), got, want)
    elif name == "pr":
        np.testing.assert_allclose(got, want, rtol=PR_RTOL, atol=0)
    elif name in ("mxv", "vxm"):
        np.testing.assert_array_equal(got[1], want[1], err_msg="presence")
        if params["semiring"] == "PLUS_SECOND_FP64":
            np.testing.assert_allclose(got[0], want[0], rtol=PR_RTOL, atol=0)
        else:
            np.testing.assert_array_equal(got[0], want[0])
    else:
        assert got.dtype == want.dtype
        np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------- the runner

class GpuBackend:
    """Graphs on the device through the package's entry points."""

    def __init__(self, ctx):
        self.ctx = ctx

    def open(self, c):
        from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
        return A.Graph(self.ctx, c.csr, c.directed)

    def close(self, G):
        G.close()

    def timing(self, on):
        self.ctx.set_kernel_timing(on)

    def call(self, c, G, name, p):
        from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
        if name == "bfs":
            return A.LA_BFS(G, p["source"])
        if name == "bfs_parent":
            return A.LA_BFS_parent(G, p["source"])
        if name == "bc":
            return A.LA_BC(G, list(p["sources"]), return_paths=True)
        if name == "sssp":
            return A.LA_SSSP(G, p["source"])
        if name == "pr":
            return A.LA_PR(G, p["damping"], p["iters"])
        if name == "wcc":
            return A.WeaklyConnectedComponents(G)
        if name == "cdlp":
            return A.LA_CDLP(G, p["iters"])
        if name == "lcc":
            return A.LA_LCC(G)
        if name in ("mxv", "vxm"):
            u, up = _op_inputs(c.csr, p["semiring"])
            return getattr(A, name)(G, getattr(A, p["semiring"]), u, up, None, 0, None, np.zeros(c.n, np.uint8))
        raise AssertionError(name)


class Session:
    """One open graph and the steps made on it.  `history` may be shared among the sessions of
    one context (sequence g): then it holds every graph's steps in the order they were made."""

    def __init__(self, backend, c, monkeypatch=None, history=None, want=expected):
        self.backend, self.c, self.monkeypatch, self.want = backend, c, monkeypatch, want
        self.history = [] if history is None else history
        self.G = backend.open(c)

    def close(self):
        if self.G is not None:
            self.backend.close(self.G)
            self.G = None

    def step(self, step):
        name, params = step
        index = len(self.history)
        self.history.append((self.c.name, name, params))
        if name == "timing":
            self.backend.timing(bool(params))
        elif name == "env":
            for k, v in params.items():
                if v is None:
                    self.monkeypatch.delenv(k, raising=False)
                else:
                    self.monkeypatch.setenv(k, v)
        else:
            assert name in ALGS, name
            got = self.backend.call(self.c, self.G, name, params)   # a GxError leaves from here
            want = self.want(self.c, name, params)
            try:
                check(self.c, name, params, got, want)
            except AssertionError as e:
                raise AssertionError(failure_message(index, self.history, self._fresh_agrees(name, params), e)) from e

    def _fresh_agrees(self, name, params):
        """The same call, under the same environment, as the first call on a new graph."""
        G = self.backend.open(self.c)
        try:
            got = self.backend.call(self.c, G, name, params)
        finally:
            self.backend.close(G)
        try:
            check(self.c, name, params, got, self.want(self.c, name, params))
        except AssertionError:
            return False
        return True


def failure_message(index, history, fresh_agrees, error):
    lines = [f"wrong result at step {index}: {history[index]}", "steps so far (graph, name, params):"]
    lines += [f"  {i:3d}  {h}" for i, h in enumerate(history)]
    lines.append(f"fresh graph agrees with the oracle: {'yes' if fresh_agrees else 'no'}")
    lines.append(str(error).strip())
    return "\n".join(lines)


def run_sequence(ctx, csr, directed, steps, monkeypatch=None, backend=None, want=expected):
    """One Graph, the steps in order, each result checked as it arrives; the graph is closed and
    kernel timing switched off whatever happens.  csr / directed name one of the inputs above."""
    c = next(k for k in map(case, ("U", "D", "T", "Td", "P", "DP")) if k.csr is csr and k.directed == directed)
    backend = backend or GpuBackend(ctx)
    s = None
    try:
        s = Session(backend, c, monkeypatch, want=want)
        for step in steps:
            s.step(step)
    finally:
        try:
            if s is not None:
                s.close()
        finally:
            backend.timing(False)


def run_on(ctx, name, steps, monkeypatch=None):
    c = case(name)
    run_sequence(ctx, c.csr, c.directed, steps, monkeypatch)


# -------------------------------------------------------------------------------- sequences

def traversal_steps(c, third):
    """(a): depth 1, ~3 000, `third`, 1, ..., three entry points taking turns, WCC between two BFS."""
    return [("bfs", {"source": c.isolated}), ("bfs", {"source": c.end}), ("bfs_parent", {"source": third}),
            ("bfs", {"source": c.isolated}), ("bc", {"sources": (c.end, c.isolated, c.middle)}),
            ("bfs_parent", {"source": c.end}), ("bfs", {"source": c.middle}), ("wcc", {}), ("bfs", {"source": c.end})]


def cdlp_steps(flip_relabel):
    steps = [("cdlp", {"iters": k}) for k in CDLP_ITERS]
    if flip_relabel:   # the cache dropped before call 4 and again before call 7
        steps.insert(6, ("env", {"GX_CDLP_RELABEL": None}))
        steps.insert(3, ("env", {"GX_CDLP_RELABEL": "0"}))
    return steps


def pr_steps():
    """(d), then iters = 0 (gx_pagerank accepts it: 1 / n everywhere) and one more call after it."""
    steps = [("pr", {"damping": d, "iters": k}) for d, k in PR_PARAMS]
    return steps + [("pr", {"damping": 0.5, "iters": 0}), ("pr", {"damping": 0.85, "iters": 10})]


def sssp_steps(c):
    hub, iso = ("sssp", {"source": c.hub}), ("sssp", {"source": c.isolated})
    return [hub, iso, ("sssp", {"source": c.far}), ("timing", True), hub, ("timing", False), hub,
            ("env", {"GX_SSSP_DSCALE": "0.25"}), hub, ("env", {"GX_SSSP_DSCALE": None}), hub, iso]


def everything_steps(c):
    """(f)'s forward pass."""
    return [("pr", {"damping": 0.85, "iters": 10}), ("bfs", {"source": c.hub}), ("cdlp", {"iters": 5}),
            ("sssp", {"source": c.hub}), ("wcc", {}), ("lcc", {}), ("vxm", {"semiring": "MIN_PLUS_FP64"}),
            ("bc", {"sources": (c.hub, c.isolated, c.random)}), ("bfs_parent", {"source": c.hub})]


def random_steps(c, seed):
    """24 steps drawn from the whole vocabulary, one timing toggle at a random place."""
    rng = np.random.default_rng([seed, c.n])
    sources = (c.hub, c.isolated, 0, c.n - 1, c.random)
    src = lambda: int(sources[rng.integers(len(sources))])
    steps = []
    for _ in range(24):
        name = ALGS[rng.integers(len(ALGS))]
        if name in ("bfs", "bfs_parent", "sssp"):
            p = {"source": src()}
        elif name == "bc":
            p = {"sources": tuple(src() for _ in range(int(rng.integers(1, 4))))}
        elif name == "pr":
            d, k = PR_PARAMS[rng.integers(len(PR_PARAMS))]
            p = {"damping": d, "iters": k}
        elif name == "cdlp":
            p = {"iters": int((1, 2, 3, 6, 17)[rng.integers(5)])}
        elif name in ("mxv", "vxm"):
            p = {"semiring": SEMIRINGS[rng.integers(len(SEMIRINGS))]}
        else:
            p = {}
        steps.append((name, p))
    steps.insert(int(rng.integers(0, 25)), ("timing", True))
    return steps


# -------------------------------------------------------------------------------------- CPU

def test_inputs_have_the_properties():
    """Every property of the inputs that the sequences rely on, by the oracle alone.  These are
    conditions on the graphs: one that fails calls for another graph, not another assertion."""
    MAX = np.iinfo(np.int64).max
    U, D, T, Td, P, DP = (case(k) for k in ("U", "D", "T", "Td", "P", "DP"))
    for c in (U, D, T, Td, P, DP):
        assert c.isolated is not None and _degree(c.csr)[c.isolated] == 0, c.name
        assert c.csr.vals is not None and len(c.csr.vals) == c.csr.nnz       # weighted: every algorithm runs
        assert c.n <= 10002 and c.csr.nnz <= 70000
    assert (U.n, D.n) == (4099, 2053) and U.n % 64 != 0 and D.n % 64 != 0
    assert _degree(T.csr).max() // 2 > 8192 and _degree(Td.csr).max() > 8192   # CDLP's huge tier
    for c in (P, DP):
        assert len(np.unique(O.bfs(c.csr, c.end))) >= 27                       # past the hint cap of 24
        assert len(np.unique(O.bfs(c.csr, c.middle))) >= 27
        lev = O.bfs(c.csr, c.isolated)
        assert len(np.unique(lev)) == 2 and (lev == 0).sum() == 1              # one level: 0, the rest unreached
    assert O.bfs(P.csr, P.end)[P.far] == 2999 and len(np.unique(O.bfs(P.csr, P.end))) == 3001
    assert O.bfs(DP.csr, DP.end)[DP.hub] == 3000                               # the path runs into D's hub
    for c in (U, D):
        lev = O.bfs(c.csr, c.hub)
        assert len(np.unique(lev[lev != MAX])) < 24
    # SSSP from P's end: a bucket per vertex or so, far more than 12 replays of 8 steps
    assert np.isfinite(O.sssp(P.csr, P.end)).sum() == 3000
    assert np.isfinite(O.sssp(U.csr, U.far)).sum() > 1 and U.far != U.hub
    cdlp = lambda c, k: expected(c, "cdlp", {"iters": k})
    for c in (U, T, Td):   # active-set iterations have work
        assert any(not np.array_equal(cdlp(c, k), cdlp(c, k + 1)) for k in (3, 4, 5)), c.name
    # a 40-iteration call on U takes the lagged early exit; T never settles, so every iteration
    # asked for runs on its huge tier
    assert np.array_equal(cdlp(U, 16), cdlp(U, 17))
    assert not np.array_equal(cdlp(T, 39), cdlp(T, 40)) and not np.array_equal(cdlp(Td, 39), cdlp(Td, 40))
    assert sum(CDLP_ITERS) > 63 and max(CDLP_ITERS[:4]) <= 16 < CDLP_ITERS[4] < CDLP_ITERS[6]   # regrown twice
    kinds = [name for name, _ in cdlp_steps(True)]
    assert kinds.index("env") == 3 and kinds[7] == "env" and kinds.count("cdlp") == len(CDLP_ITERS)
    assert {k % 2 for _, k in PR_PARAMS} == {0, 1}                             # both ping-pong parities
    for seed in (1, 2, 3):
        for c in (U, D):
            steps = random_steps(c, seed)
            assert len(steps) == 25 and [n for n, _ in steps].count("timing") == 1
            assert steps == random_steps(c, seed)


class _StandIn:
    """A CPU stand-in for the device: every call returns the oracle's value, except that with
    `leak` the second and later bfs calls on one open graph are off by one level."""

    def __init__(self, leak):
        self.leak, self.timed = leak, []

    def open(self, c):
        return {"bfs_calls": 0}

    def close(self, G):
        G["closed"] = True

    def timing(self, on):
        self.timed.append(on)

    def call(self, c, G, name, p):
        want = expected(c, name, p)
        if name == "bfs":
            G["bfs_calls"] += 1
            if self.leak and G["bfs_calls"] >= 2:
                return want + 1
        return want


def test_failure_message_names_step_history_and_fresh_verdict(monkeypatch):
    """The runner's report, without a device.  A stand-in whose second bfs on one graph is wrong:
    the fresh graph agrees.  A wrong expected value: it does not."""
    c = case("D")
    steps = [("bfs", {"source": c.hub}), ("wcc", {}), ("env", {"GX_TEST_CALL_HISTORY": "1"}), ("timing", True),
             ("bfs", {"source": c.isolated}), ("lcc", {})]
    ok = _StandIn(leak=False)
    run_sequence(None, c.csr, c.directed, steps, monkeypatch, backend=ok)
    assert ok.timed == [True, False]
    leaky = _StandIn(leak=True)
    with pytest.raises(AssertionError) as err:
        run_sequence(None, c.csr, c.directed, steps, monkeypatch, backend=leaky)
    text = str(err.value)
    print(text)
    assert text.startswith(f"wrong result at step 4: ('D', 'bfs', {{'source': {c.isolated}}})")
    assert f"    0  ('D', 'bfs', {{'source': {c.hub}}})" in text and "    3  ('D', 'timing', True)" in text
    assert "'lcc'" not in text                                   # nothing ran after the wrong value
    assert "fresh graph agrees with the oracle: yes" in text
    assert "Mismatched elements" in text                         # numpy's own report follows
    assert leaky.timed[-1] is False

    def wrong(k, name, params):
        want = expected(k, name, params)
        return want + 1 if name == "wcc" else want

    with pytest.raises(AssertionError) as err:
        run_sequence(None, c.csr, c.directed, steps, monkeypatch, backend=_StandIn(leak=False), want=wrong)
    assert "wrong result at step 1: ('D', 'wcc', {})" in str(err.value)
    assert "fresh graph agrees with the oracle: no" in str(err.value)


# -------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["P", "DP"])
def test_a_traversal_hint_and_shared_remap(ctx, name):
    """bfs, bfs_parent and bc share one level-step hint and, on the hub-first copy, one remap
    scratch, which WCC uses as 2n int32 between two BFS calls."""
    c = case(name)
    run_on(ctx, name, traversal_steps(c, c.middle if name == "P" else c.hub))


@pytest.mark.gpu
@pytest.mark.parametrize("before", ["cdlp", "bfs_bfs_pr", "lcc"])
def test_b_first_directed_bfs_and_the_transpose(ctx, before):
    """CDLP, PageRank and LCC build A' on a directed graph, so their place in the history decides
    which BFS call first goes bottom-up: the same levels every time."""
    c = case("D")
    bfs = ("bfs", {"source": c.hub})
    steps = {"cdlp": [("cdlp", {"iters": 3}), bfs],
             "bfs_bfs_pr": [bfs, bfs, ("pr", {"damping": 0.85, "iters": 10}), bfs],
             "lcc": [("lcc", {}), bfs]}[before]
    run_on(ctx, "D", steps)


@pytest.mark.gpu
@pytest.mark.parametrize("flip_relabel", [False, True], ids=["default", "relabel_flipped"])
@pytest.mark.parametrize("name", ["U", "T", "Td"])
def test_c_cdlp_iteration_counts(ctx, monkeypatch, name, flip_relabel):
    """Caller order then the relabelled copy, cap_iters regrown twice, the active set off between
    calls where it is on, an early fixed point (U) followed by short calls, the huge tier's 63
    epochs used up between calls (T); and the cache dropped and rebuilt in mid-history.  The
    recount bound's arrays outlive every one of these calls (gx_cdlp)."""
    monkeypatch.delenv("GX_CDLP_RELABEL", raising=False)
    run_on(ctx, name, cdlp_steps(flip_relabel), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["U", "D"])
def test_d_pagerank_parameters_on_a_cached_plan(ctx, name):
    run_on(ctx, name, pr_steps())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["U", "P"])
def test_e_sssp_sources_layout_and_timing(ctx, monkeypatch, name):
    """Sources near and far on one layout (the replay hint), kernel timing moving the run off the
    captured step graph and back, another bucket width (new layout, new work) and back."""
    monkeypatch.delenv("GX_SSSP_DSCALE", raising=False)
    run_on(ctx, name, sssp_steps(case(name)), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["U", "D"])
def test_f_everything_on_one_graph(ctx, name):
    """Forward, reversed, forward: every algorithm on its first, second and third call with all the
    others' caches present."""
    fwd = everything_steps(case(name))
    run_on(ctx, name, fwd + fwd[::-1] + fwd)


@pytest.mark.gpu
def test_g_several_graphs_on_one_context(ctx):
    """T, U and D open together, (f)'s forward pass one step on each in turn; U closed, P opened
    (freed addresses reused), and again on T, P and D.  The device's grow-only scratch and
    rocPRIM temporary are sized by one graph and used by the others."""
    backend, history, sessions = GpuBackend(ctx), [], {}

    def round_robin(names):
        plans = [everything_steps(case(k)) for k in names]
        for i in range(len(plans[0])):
            for k, plan in zip(names, plans):
                sessions[k].step(plan[i])

    try:
        for k in ("T", "U", "D"):
            sessions[k] = Session(backend, case(k), history=history)
        round_robin(("T", "U", "D"))
        sessions.pop("U").close()
        sessions["P"] = Session(backend, case("P"), history=history)
        round_robin(("T", "P", "D"))
    finally:
        for s in sessions.values():
            s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("name", ["U", "D"])
def test_random_sequences(ctx, name, seed):
    run_on(ctx, name, random_steps(case(name), seed))
