"""Edges of the LCC and WCC drivers (gx_lcc.hip, gx_lcc_part.hip, gx_wcc.hip) that the other files do
not reach: when each knob is read (gx_lcc latches its knobs with the cache, gx_lcc_part_counts and
gx_wcc read theirs at every call), how the tier limits are parsed (clamped, never a fallback to the
default), tiers without items, degenerate sizes, and the launch counts of every WCC knob setting.

LCC results are compared bit for bit with the dense formula of tests/test_lcc_tiers.py, WCC labels
with scipy's components relabelled to their smallest vertex id.  Launch counts are those of the
KTimer names (one count per timed region); the WCC literals were read from the driver before it was
split into stages."""
import functools

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (sys.path)
from test_lcc_tiers import (DEFAULT_LIMITS, KNOB_LIMITS, KNOBS, TIMERS, _dense_lcc, _knob_case, _loop_cases,
                            _matrices, _oriented, _tiers)

LCC_TIMERS = TIMERS + ("lcc_triangles", "lcc_core")
WCC_TIMERS = ("wcc_sample", "wcc_compress", "wcc_hook")
ALL_KNOBS = tuple(KNOBS) + ("GX_LCC_CORE", "GX_WCC_ROUNDS", "GX_WCC_MINHOOK", "GX_WCC_HOOK0", "GX_HUB", "GX_HUB_SORT")


def _set_env(monkeypatch, env):
    """Exactly `env` among the knobs these drivers (and the hub-first copy) read."""
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------- tier limits
def _limits(env):
    """lcc_knobs restated: each limit clamped to [1, compiled value] (unset or empty: the compiled
    value), then forced to wave <= wave2 <= block."""
    out = []
    for name, compiled in zip(KNOBS, DEFAULT_LIMITS):
        e = env.get(name, "")
        out.append(compiled if e == "" else min(max(int(e), 1), compiled))
    out[1] = max(out[0], out[1])
    out[2] = max(out[1], out[2])
    return tuple(out)


def _tier_launches(csr, limits):
    """The launches of one gx_lcc call under `limits`: one per tier holding a vertex, one
    lcc_triangles around them; and the population of the four tiers."""
    d, e, _ = _oriented(_matrices(csr)[1])
    t = _tiers(d, e, limits)
    pop = [int((t == i).sum()) for i in range(4)]
    launches = {name: int(p > 0) for name, p in zip(TIMERS, pop)}
    launches.update(lcc_triangles=1, lcc_core=0)
    return launches, pop


# wave_max, wave2_max, block_max after parsing; the tiers of _knob_case(True) that hold vertices
CLAMP_CASES = {
    "unset": ({}, (256, 512, 8192), (1, 1, 0, 0)),
    "above": ({"GX_LCC_WAVE_MAX": "100000"}, (256, 512, 8192), (1, 1, 0, 0)),
    "zero": ({"GX_LCC_WAVE_MAX": "0"}, (1, 512, 8192), (1, 1, 0, 0)),
    "empty": ({"GX_LCC_WAVE_MAX": ""}, (256, 512, 8192), (1, 1, 0, 0)),
    # block is raised to wave2, which is unset (512): every vertex stays in the wave tiers
    "block-below-wave": ({"GX_LCC_BLOCK_MAX": "4", "GX_LCC_WAVE_MAX": "8"}, (8, 512, 512), (1, 1, 0, 0)),
    # wave2 and block both raised to wave (8): everything above 8 is the merge fallback's
    "block-raised-to-8": ({"GX_LCC_BLOCK_MAX": "4", "GX_LCC_WAVE_MAX": "8", "GX_LCC_WAVE2_MAX": "2"}, (8, 8, 8),
                          (1, 0, 0, 1)),
}


@pytest.mark.parametrize("case", sorted(CLAMP_CASES))
def test_clamp_cases_on_the_cpu(case):
    """The parsed limits of every clamp case and the tiers they populate on the knob graph."""
    env, limits, tiers = CLAMP_CASES[case]
    assert _limits(env) == limits
    launches, pop = _tier_launches(_knob_case(True)[0], limits)
    assert tuple(int(p > 0) for p in pop) == tiers, pop
    assert tuple(launches[t] for t in TIMERS) == tiers
    if case == "zero":
        d, e, _ = _oriented(_matrices(_knob_case(True)[0])[1])
        assert ((d == 1) & (e > 0)).any() and ((d > 1) & (e > 0)).any()


def test_knob_limits_restated():
    assert _limits(KNOBS) == KNOB_LIMITS and _limits({}) == DEFAULT_LIMITS


# -------------------------------------------------------------------------------- graphs
@functools.lru_cache(maxsize=None)
def _wave_only_case():
    """300 vertices, 2 400 random directed entries: every work-item vertex has |O(u)| <= 256."""
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
    rng = np.random.default_rng(77)
    csr = csr_from_edges(300, rng.integers(0, 300, 2400), rng.integers(0, 300, 2400), None, symmetric=False)
    launches, pop = _tier_launches(csr, DEFAULT_LIMITS)
    assert pop[0] >= 100 and pop[1:] == [0, 0, 0], pop
    lcc, _ = _dense_lcc(csr)
    assert np.count_nonzero(lcc) > 100
    return csr, lcc, launches


@functools.lru_cache(maxsize=None)
def _star_case():
    """Vertex 0 joined to 1..199: the leaves point at the centre in the orientation, so every
    vertex has an empty O or an empty I list and no work item is made, though O has entries."""
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
    leaves = np.arange(1, 200)
    csr = csr_from_edges(200, np.zeros(199, np.int64), leaves, None, symmetric=True)
    d, e, _ = _oriented(_matrices(csr)[1])
    assert d.sum() == 199 and ((d == 0) | (e == 0)).all()
    return csr


def _empty_csr(n):
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import CSR
    return CSR(n, np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64))


WCC_N, WCC_GIANT, WCC_SMALL, WCC_SMALL_SIZE = 2000, 1790, 50, 4


@functools.lru_cache(maxsize=None)
def _wcc_case():
    """(undirected CSR, the same edges stored one way, min-id labels): 2 000 vertices in a random
    order; a giant component of 1 790 (a random tree plus 3 000 edges), 50 paths of 4 vertices and
    10 isolated vertices."""
    import scipy.sparse as sp
    from scipy.sparse import csgraph
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
    rng = np.random.default_rng(91)
    ids = rng.permutation(WCC_N)
    g = np.arange(1, WCC_GIANT)
    src = [g, rng.integers(0, WCC_GIANT, 3000)]
    dst = [(rng.random(WCC_GIANT - 1) * g).astype(np.int64), rng.integers(0, WCC_GIANT, 3000)]
    path = WCC_GIANT + np.arange(WCC_SMALL * WCC_SMALL_SIZE).reshape(WCC_SMALL, WCC_SMALL_SIZE)
    src.append(path[:, :-1].ravel())
    dst.append(path[:, 1:].ravel())
    src, dst = ids[np.concatenate(src)], ids[np.concatenate(dst)]
    keep = src != dst
    src, dst = src[keep], dst[keep]
    und = csr_from_edges(WCC_N, src, dst, None, symmetric=True)
    one = csr_from_edges(WCC_N, np.minimum(src, dst), np.maximum(src, dst), None, symmetric=False)
    assert one.nnz * 2 == und.nnz
    m = sp.csr_matrix((np.ones(one.nnz), one.colidx.astype(np.int64), one.rowptr.astype(np.int64)), shape=(WCC_N, WCC_N))
    ncomp, lab = csgraph.connected_components(m, directed=True, connection="weak")
    sizes = np.sort(np.bincount(lab))[::-1]
    assert ncomp == 1 + WCC_SMALL + (WCC_N - WCC_GIANT - WCC_SMALL * WCC_SMALL_SIZE)
    assert sizes[0] == WCC_GIANT and (sizes[1:1 + WCC_SMALL] == WCC_SMALL_SIZE).all() and (sizes[1 + WCC_SMALL:] == 1).all()
    mins = np.full(ncomp, WCC_N, dtype=np.int64)
    np.minimum.at(mins, lab, np.arange(WCC_N))
    return und, one, mins[lab]


def test_wcc_case_shape():
    und, one, want = _wcc_case()
    assert len(np.unique(want)) == 61 and (want <= np.arange(WCC_N)).all()
    # no vertex is a giant-component vertex by its id alone
    giant = want == np.bincount(want).argmax()
    assert giant[:100].any() and not giant[:100].all()


# ----------------------------------------------------------------------------- GPU tests
@pytest.fixture(scope="module")
def ctx():
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    c = Context(0)
    yield c
    c.close()


def _timed(ctx, names, fn):
    """fn()'s result and the launches of the timers `names` during it."""
    ctx.reset_kernel_stats()
    ctx.set_kernel_timing(True)
    try:
        got = fn()
    finally:
        ctx.set_kernel_timing(False)
    return got, {name: ctx.kernel_stats(name)[0] for name in names}


def _expect(wave=0, wave2=0, block=0, merge=0, triangles=1, core=0):
    return dict(lcc_wave=wave, lcc_wave2=wave2, lcc_block=block, lcc_merge=merge, lcc_triangles=triangles,
                lcc_core=core)


@pytest.mark.gpu
@pytest.mark.parametrize("knob", ["tiers", "core"])
def test_lcc_knobs_latched_with_the_cache(ctx, monkeypatch, knob):
    """gx_lcc reads its knobs when it builds the cache: a graph first called with the tier limits
    lowered (or with GX_LCC_CORE=128) keeps its four tiers (its dense core) when the variables are
    gone, and a fresh graph without them takes the two wave kernels only."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    csr, want, _ = _knob_case(True)
    all_tiers = _expect(1, 1, 1, 1) if knob == "tiers" else _expect(1, 1, core=1)
    _set_env(monkeypatch, KNOBS if knob == "tiers" else {"GX_LCC_CORE": "128"})
    G = A.Graph(ctx, csr, True)
    try:
        got, launches = _timed(ctx, LCC_TIMERS, lambda: A.LA_LCC(G))
        np.testing.assert_array_equal(got, want)
        assert launches == all_tiers
        _set_env(monkeypatch, {})
        again, launches = _timed(ctx, LCC_TIMERS, lambda: A.LA_LCC(G))
        np.testing.assert_array_equal(again, got)
        assert launches == all_tiers
    finally:
        G.close()
    F = A.Graph(ctx, csr, True)
    try:
        got, launches = _timed(ctx, LCC_TIMERS, lambda: A.LA_LCC(F))
        np.testing.assert_array_equal(got, want)
        assert launches == _expect(1, 1)
    finally:
        F.close()


@pytest.mark.gpu
def test_lcc_part_reads_the_knobs_per_call(ctx, monkeypatch):
    """gx_lcc_part_counts cuts its items at every call: one handle counts with all four tiers
    under the lowered limits and with the two wave kernels once the variables are gone, the
    counters equal to the dense numerators both times."""
    import torch
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    from ldbc_graphalytics_platforms_graphblas_amd.distributed import GpuBackend
    csr, _, num = _knob_case(True)
    n = csr.n
    _set_env(monkeypatch, KNOBS)
    G = A.Graph(ctx, csr, True)
    part = None
    try:
        part = GpuBackend(G).lcc_part()

        def counted():
            tc = torch.zeros(n, dtype=torch.int64, device="cuda:0")
            part.counts(0, n, tc)
            torch.cuda.synchronize()
            return tc.cpu().numpy()

        got, launches = _timed(ctx, LCC_TIMERS, counted)
        np.testing.assert_array_equal(got, num)
        assert launches == _expect(1, 1, 1, 1)
        _set_env(monkeypatch, {})
        got, launches = _timed(ctx, LCC_TIMERS, counted)
        np.testing.assert_array_equal(got, num)
        assert launches == _expect(1, 1)
    finally:
        if part is not None:
            part.close()
        G.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CLAMP_CASES))
def test_lcc_limits_are_clamped(ctx, monkeypatch, case):
    """A tier limit out of range is clamped to [1, compiled value], never replaced by the default,
    and the three are forced into order; the launches are those the parsed limits give on the
    knob graph's |O(u)| histogram (test_clamp_cases_on_the_cpu), the result exact."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    env, limits, _ = CLAMP_CASES[case]
    csr, want, _ = _knob_case(True)
    expect, _ = _tier_launches(csr, limits)
    _set_env(monkeypatch, env)
    G = A.Graph(ctx, csr, True)
    try:
        got, launches = _timed(ctx, LCC_TIMERS, lambda: A.LA_LCC(G))
    finally:
        G.close()
    np.testing.assert_array_equal(got, want)
    assert launches == expect


@pytest.mark.gpu
def test_lcc_skipped_tiers(ctx, monkeypatch):
    """Tiers without items launch nothing: a graph in the first wave tier alone runs lcc_wave
    inside one lcc_triangles; a star, whose orientation has entries but no work item, opens
    lcc_triangles around no launch and returns zeros."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    _set_env(monkeypatch, {})
    csr, want, expect = _wave_only_case()
    assert expect == _expect(1)
    G = A.Graph(ctx, csr, True)
    try:
        got, launches = _timed(ctx, LCC_TIMERS, lambda: A.LA_LCC(G))
    finally:
        G.close()
    np.testing.assert_array_equal(got, want)
    assert launches == expect
    star = _star_case()
    G = A.Graph(ctx, star, False)
    try:
        got, launches = _timed(ctx, LCC_TIMERS, lambda: A.LA_LCC(G))
    finally:
        G.close()
    np.testing.assert_array_equal(got, np.zeros(star.n))
    assert launches == _expect(triangles=1)


def _degenerate():
    return [("n1", _empty_csr(1)), ("n5-empty", _empty_csr(5)), ("loops", _loop_cases()[0][0])]


@pytest.mark.gpu
@pytest.mark.parametrize("directed", [True, False], ids=["directed", "undirected"])
def test_degenerate_sizes(ctx, monkeypatch, directed):
    """One vertex, five vertices without entries, and self-loops only: LCC is zero everywhere,
    through gx_lcc and through the partitioned entry points (create, ranges, counts, finish), and
    every vertex is its own component, on the first call and on the second."""
    import torch
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    from ldbc_graphalytics_platforms_graphblas_amd.distributed import GpuBackend
    _set_env(monkeypatch, {})
    for name, csr in _degenerate():
        n = csr.n
        G = A.Graph(ctx, csr, directed)
        part = None
        try:
            for call in range(2):
                np.testing.assert_array_equal(A.LA_LCC(G), np.zeros(n), err_msg=f"{name} lcc {call}")
                np.testing.assert_array_equal(A.WeaklyConnectedComponents(G), np.arange(n), err_msg=f"{name} wcc {call}")
            part = GpuBackend(G).lcc_part()
            r = part.ranges(3).astype(np.int64)
            assert len(r) == 4 and r[0] == 0 and r[-1] == n and (np.diff(r) >= 0).all(), (name, r)
            tc = torch.zeros(n, dtype=torch.int64, device="cuda:0")
            for v0, v1 in zip(r[:-1], r[1:]):
                part.counts(int(v0), int(v1), tc)
            out = torch.ones(n, dtype=torch.float64, device="cuda:0")
            part.finish(tc, out)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(tc.cpu().numpy(), np.zeros(n, dtype=np.int64), err_msg=name)
            np.testing.assert_array_equal(out.cpu().numpy(), np.zeros(n), err_msg=name)
        finally:
            if part is not None:
                part.close()
            G.close()


# (wcc_sample, wcc_compress, wcc_hook) launches of the first call and of the second (on the
# hub-first copy, rows sorted: one sampling round unless GX_WCC_ROUNDS says otherwise).  A round is
# one wcc_sample and one wcc_compress; round 1 has GX_WCC_MINHOOK more wcc_sample (whose compress is
# untimed); the finish is one wcc_hook and one wcc_compress.
WCC_UNDIRECTED = {
    "default": ({}, (3, 3, 1), (1, 2, 1)),
    "rounds-0": ({"GX_WCC_ROUNDS": "0"}, (1, 2, 1), (1, 2, 1)),
    "rounds-9": ({"GX_WCC_ROUNDS": "9"}, (3, 3, 1), (3, 3, 1)),
    "minhook-0": ({"GX_WCC_MINHOOK": "0"}, (2, 3, 1), (1, 2, 1)),
    "hook0-0": ({"GX_WCC_HOOK0": "0"}, (3, 3, 1), (1, 2, 1)),
}
WCC_DIRECTED = (2, 3, 1)   # two rounds without min-hook passes, whatever GX_WCC_ROUNDS


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(WCC_UNDIRECTED))
def test_wcc_knobs_undirected(ctx, monkeypatch, case):
    """Every knob setting labels the 61 components by their smallest vertex, on the first call and
    on the second (the hub-first copy), with the launch counts the setting stands for."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    env, first, second = WCC_UNDIRECTED[case]
    und, _, want = _wcc_case()
    _set_env(monkeypatch, env)
    G = A.Graph(ctx, und, False)
    try:
        for call, expect in enumerate((first, second)):
            got, launches = _timed(ctx, WCC_TIMERS, lambda: A.WeaklyConnectedComponents(G))
            print(case, "call", call, launches)
            np.testing.assert_array_equal(got.astype(np.int64), want, err_msg=f"call {call}")
            assert tuple(launches[t] for t in WCC_TIMERS) == expect, f"call {call}"
    finally:
        G.close()


@pytest.mark.gpu
def test_wcc_directed_ignores_rounds(ctx, monkeypatch):
    """The same edges stored one way, as a directed graph: the same labels, two sampling rounds
    and a skip of 2 whatever GX_WCC_ROUNDS says."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    _, one, want = _wcc_case()
    for env in ({}, {"GX_WCC_ROUNDS": "1"}, {"GX_WCC_ROUNDS": "0"}):
        _set_env(monkeypatch, env)
        G = A.Graph(ctx, one, True)
        try:
            for call in range(2):
                got, launches = _timed(ctx, WCC_TIMERS, lambda: A.WeaklyConnectedComponents(G))
                print(env, "call", call, launches)
                np.testing.assert_array_equal(got.astype(np.int64), want, err_msg=f"{env} call {call}")
                assert tuple(launches[t] for t in WCC_TIMERS) == WCC_DIRECTED, f"{env} call {call}"
        finally:
            G.close()
