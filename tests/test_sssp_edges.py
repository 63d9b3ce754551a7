"""SSSP at the boundaries its kernels are built around (gx_sssp.hip, gx_sssp_split.hip, gx_sssp.h):
the 256-edge relax chunk, the 512-entry push stage, the 32-slot bucket ring and its overflow, the
light/heavy split at w == delta, the dense opening, and the 31-bit stamps that 64-bit bucket
numbers are kept in.

Every graph is crafted here with csr_from_edges.  The bar is bit-for-bit equality with the oracle;
trees (chains, stars, two-hop stars) are also held against distances written down in the test from
dyadic weights, whose left-to-right sums are exact, so a mistake shared with the oracle cannot
hide.  Each GPU case runs on three paths: gx_sssp twice on one resident graph (the second call of
an undirected graph takes the hub-first copy), the one-rank split, and two simulated ranks in lock
step.  The unmarked tests check the constructions themselves and need no GPU.
"""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (sys.path)
from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
from oracle import oracle as O

gpu = pytest.mark.gpu

INF = np.inf
D32 = 2.0 ** -32            # GX_SSSP_DELTA of case 1: exact, and 1 / D32 == 2 ** 32
KNOBS = ("GX_SSSP_DELTA", "GX_SSSP_DSCALE", "GX_SSSP_PULL", "GX_SSSP_PULL_FRAC", "GX_SSSP_FUSE",
         "GX_SSSP_FUSE_MAX", "GX_SSSP_DENSE", "GX_SSSP_GRAPH", "GX_SSSP_VERBOSE", "GX_SPLIT_VERBOSE")
K_MAX_BUCKET = 4000000000000000000   # gx_sssp.h kMaxBucket


# ------------------------------------------------------------------ helpers

class Case:
    """A crafted graph: directed edge list, source, and (trees only) the expected distances."""

    def __init__(self, n, src, dst, w, source=0, closed=None):
        self.n = int(n)
        self.src = np.asarray(src, dtype=np.int64)
        self.dst = np.asarray(dst, dtype=np.int64)
        self.w = np.asarray(w, dtype=np.float64)
        self.source = int(source)
        self.closed = closed    # float64[n], a function (csr, source) -> float64[n], or None

    def csr(self, symmetric):
        return csr_from_edges(self.n, self.src, self.dst, self.w.copy(), symmetric=symmetric)


def path_sums(csr, source):
    """Distances in a graph where every vertex is reached from `source` by one simple path (a tree
    or forest, directed or stored symmetrically): the weights added left to right along that path.
    No minimum is taken anywhere, so this is the closed form, not a shortest-path algorithm."""
    rp = csr.rowptr.astype(np.int64)
    ci = csr.colidx.astype(np.int64)
    d = np.full(csr.n, INF)
    d[source] = 0.0
    parent = np.full(csr.n, -1, dtype=np.int64)
    stack = [source]
    while stack:
        u = stack.pop()
        for e in range(rp[u], rp[u + 1]):
            v = int(ci[e])
            if v == parent[u] or v == u:
                continue
            assert d[v] == INF, "path_sums: not a tree"
            d[v] = d[u] + csr.vals[e]
            parent[v] = u
            stack.append(v)
    return d


def buckets(d, delta):
    """bucket_of (gx_sssp.h): floor(d * (1 / delta)) clamped to kMaxBucket, as Python ints; unreached: None."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        inv = np.float64(1.0) / np.float64(delta)
        q = np.asarray(d, dtype=np.float64) * inv
    return [None if x == INF and dd == INF else (int(x) if x < 4.0e18 else K_MAX_BUCKET) for x, dd in zip(q, d)]


def set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def knob_str(x):
    """A knob value that atof reads back bit for bit."""
    return "%.17g" % x


@pytest.fixture(scope="module")
def ctx():
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    c = Context(0)
    yield c
    c.close()


def run_paths(ctx, csr, directed, source):
    """The three paths' distances: gx_sssp twice on one resident graph, the split on one rank, two
    simulated ranks."""
    import torch
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    from ldbc_graphalytics_platforms_graphblas_amd import distributed as D
    out = {}
    G = A.Graph(ctx, csr, directed)
    try:
        out["gx_sssp call 1"] = A.LA_SSSP(G, source)
        out["gx_sssp call 2"] = A.LA_SSSP(G, source)
        sp = A.SsspSplit(G)
        try:
            out["split, one rank"] = sp.run(source)
        finally:
            sp.close()
        dev = torch.device("cuda", 0)
        be = D.GpuBackend(G)
        rng = D.vertex_ranges(csr.rowptr, 2)
        ranks = [D.LocalRank(be, int(rng[k]), int(rng[k + 1]), dev, k) for k in range(2)]
        out["split, two ranks"] = D.sssp(ranks, D.LocalComm(), csr.n, source).cpu().numpy()
    finally:
        G.close()
    return out


def mismatches(got, want, label):
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if len(bad) == 0 and got.shape == want.shape:
        return []
    head = ", ".join(f"d[{v}] = {got[v]!r} want {want[v]!r}" for v in bad[:4])
    return [f"{label}: {len(bad)} of {len(want)} differ: {head}"]


def check(ctx, monkeypatch, case, symmetric, envs=({},), sources=None):
    """Every knob setting in `envs` x every source x the three paths, against the oracle and, where
    the case has one, the closed form.  All mismatches are reported together."""
    csr = case.csr(symmetric)
    errs = []
    for source in (sources if sources is not None else (case.source,)):
        want = O.sssp(csr, source)
        closed = None
        if case.closed is not None:
            closed = case.closed(csr, source) if callable(case.closed) else case.closed
            assert np.array_equal(want, closed), "the oracle and the closed form disagree"
        for env in envs:
            set_knobs(monkeypatch, env)
            for name, got in run_paths(ctx, csr, not symmetric, source).items():
                errs += mismatches(got, want, f"{'undirected' if symmetric else 'directed'} src {source} {env} {name}")
    assert not errs, "\n".join(errs[:24])


# ------------------------------------------------------------------ case 1: buckets around 2^31 and 2^32

CRITICAL = [2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 33 - 1]


def chain4(kind, crit, fillers):
    """0 -> 1 -> 2 -> 3 under delta = 2^-32.
    kind "settle": weights ((crit - 31) d, d / 2, 0.5).  Vertex 1 is alone on the overflow, the
    split puts the window at its bucket crit - 31 and unbounded fusion opens it whole, cur = crit;
    vertex 2 is reached by a light edge, joins near and must join the settled list of `crit`.
    kind "ring": weights ((crit - 5) d, 5 d, 0.5).  With buckets opened one at a time vertex 2's
    first ring push is into bucket crit.
    fillers: 40 vertices hanging off vertex 1 at buckets spread over its window, and 8 off vertex 0
    in the same window, so other ring slots are non-empty when the critical one opens."""
    w1 = (crit - 31) * D32 if kind == "settle" else (crit - 5) * D32
    w2 = D32 / 2 if kind == "settle" else 5 * D32
    b1 = crit - 31 if kind == "settle" else crit - 5
    src, dst, w = [0, 1, 2], [1, 2, 3], [w1, w2, 0.5]
    n = 4
    if fillers:
        for i in range(40):
            src.append(1), dst.append(n), w.append((1 + (i * 7) % 30) * D32)
            n += 1
        for i in range(8):
            src.append(0), dst.append(n), w.append((b1 + 3 * i + 1) * D32)
            n += 1
    return Case(n, src, dst, w, 0, closed=path_sums)


def case1_envs(symmetric):
    envs = []
    for fuse in ({}, {"GX_SSSP_FUSE": 0}, {"GX_SSSP_FUSE": 1}, {"GX_SSSP_FUSE_MAX": 1}):
        for pull in (({"GX_SSSP_PULL": 0}, {"GX_SSSP_PULL": 2}) if symmetric else ({},)):
            for dense in ({"GX_SSSP_DENSE": 0}, {"GX_SSSP_DENSE": 1000000}):
                envs.append({"GX_SSSP_DELTA": knob_str(D32), **fuse, **pull, **dense})
    return envs


def test_delta_2_pow_minus_32_is_exact():
    assert float(knob_str(D32)) == D32 and 1.0 / D32 == 2.0 ** 32


@pytest.mark.parametrize("crit", CRITICAL)
@pytest.mark.parametrize("kind", ["settle", "ring"])
@pytest.mark.parametrize("fillers", [False, True])
def test_chain4_construction(kind, crit, fillers):
    """Oracle == closed form, and the chain's buckets are the ones the case is named for."""
    case = chain4(kind, crit, fillers)
    for symmetric in (False, True):
        csr = case.csr(symmetric)
        d = O.sssp(csr, 0)
        assert np.array_equal(d, path_sums(csr, 0))
        b = buckets(d, D32)
        if kind == "settle":
            # window base = vertex 1's bucket (the smallest on the overflow), whole window: cur = crit
            assert b[1] == crit - 31 == min(x for x in b[1:]) and b[1] + 31 == crit
            assert b[2] == b[1] and csr.vals[csr.rowptr[1]:csr.rowptr[2]].min() < D32   # a light edge, same bucket
            assert d[3] == d[2] + 0.5 and 0.5 >= D32
        else:
            assert (b[1], b[2]) == (crit - 5, crit) and b[2] < b[1] + 32    # a ring push inside 1's window
        assert all(x is not None for x in b)
        if fillers:
            slots = {x % 32 for x in b[4:]}
            assert len(slots) >= 20 and all(b[1] < x < b[1] + 32 for x in b[4:])
    if crit == 2 ** 32 - 1 and not fillers:
        want = [0.0, 1 - 2.0 ** -27, 1 - 2.0 ** -27 + 2.0 ** -33, 1.5 - 2.0 ** -27 + 2.0 ** -33] if kind == "settle" \
            else [0.0, 1 - 6 * D32, 1 - D32, 1.5 - D32]
        assert O.sssp(case.csr(False), 0).tolist() == want
        assert np.int32(np.uint32(crit & 0xFFFFFFFF)) == -1    # the 32-bit form of the bucket: the old "never" word


@gpu
@pytest.mark.parametrize("crit", CRITICAL)
@pytest.mark.parametrize("kind", ["settle", "ring"])
@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("fillers", [False, True])
def test_bucket_numbers_around_2_31_and_2_32(ctx, monkeypatch, kind, crit, symmetric, fillers):
    """Bucket numbers around 2^31 and 2^32 with GX_SSSP_DELTA = 2^-32: the settled-list claim
    against `cur` ("settle": a vertex first reached by a light edge while cur's stamp equals the
    initial one never gets its heavy edges relaxed) and the first ring push against the initial
    stamp ("ring": dropped when the bucket's stamp equals the initial one), on the push path, in
    sssp_pull (GX_SSSP_PULL=2) and in the dense opening (GX_SSSP_DENSE), with buckets opened whole,
    one at a time (GX_SSSP_FUSE=0 / 1, GX_SSSP_FUSE_MAX=1) and with other ring slots filled."""
    check(ctx, monkeypatch, chain4(kind, crit, fillers), symmetric, case1_envs(symmetric))


# ------------------------------------------------------------------ case 2: the same magnitudes, no knob

def big_default_graph():
    """No knob: the bucket-width rule itself must give max d / delta > 4 * 2^33.  The rule is
    delta = dscale * mean w / mean degree, and d <= sum w, so d / delta <= nnz^2 / (dscale * n): no
    graph of test size gets there through a finite mean.  Two dead-end edges of weight 2^1023 make
    the mean infinite, and the rule then falls back to delta = 1 (sssp_delta).  Source cluster
    (2^-40 edges) -> a: 2^32 - 32 -> b: 0.5 (light: the "settle" shape at cur = 2^32 - 1) ->
    c: 31.5 -> a dozen edges of 2^32 -> tail cluster (2^-40 edges) -> the two 2^1023 edges."""
    rng = np.random.default_rng(7)
    src, dst, w = [], [], []
    na, nt = 50, 30
    for i in range(na):                                   # cluster A: ring + chords
        src.append(i), dst.append((i + 1) % na), w.append(2.0 ** -40)
    for _ in range(250):
        a, b = rng.integers(0, na, 2)
        if a != b:
            src.append(int(a)), dst.append(int(b)), w.append(2.0 ** -40)
    a_, b_, c_ = na, na + 1, na + 2
    src += [na // 2, a_, b_]
    dst += [a_, b_, c_]
    w += [2.0 ** 32 - 32, 0.5, 31.5]
    v = c_
    for _ in range(12):
        src.append(v), dst.append(v + 1), w.append(2.0 ** 32)
        v += 1
    t0 = v
    for i in range(nt):                                   # tail cluster behind the chain
        src.append(t0 + i), dst.append(t0 + (i + 1) % nt), w.append(2.0 ** -40)
    for _ in range(120):
        a, b = rng.integers(0, nt, 2)
        if a != b:
            src.append(t0 + int(a)), dst.append(t0 + int(b)), w.append(2.0 ** -40)
    e0 = t0 + nt
    src += [t0 + 3, t0 + 5]
    dst += [e0, e0 + 1]
    w += [2.0 ** 1023, 2.0 ** 1023]
    return Case(e0 + 2, src, dst, w, 0), (a_, b_, c_, t0)


def default_delta(csr, dscale):
    """sssp_delta (gx_sssp.hip) in numpy."""
    with np.errstate(over="ignore"):
        mean = np.sum(csr.vals) / csr.nnz if csr.nnz else 1.0
    delta = dscale * mean / max(1.0, csr.nnz / max(1.0, csr.n))
    return delta if delta > 0.0 and np.isfinite(delta) else 1.0


def test_big_default_graph_construction():
    case, (a_, b_, c_, t0) = big_default_graph()
    for symmetric, scales in ((False, (0.5,)), (True, (2.0, 3.0))):
        csr = case.csr(symmetric)
        d = O.sssp(csr, 0)
        assert np.isfinite(d).all()
        for dscale in scales:
            delta = default_delta(csr, dscale)
            assert delta == 1.0      # whatever the summation order: every partial sum past both 2^1023 is inf
            b = buckets(d, delta)
            assert max(x for x in b if x < K_MAX_BUCKET) > 4 * 2 ** 33
            assert b[a_] == 2 ** 32 - 32 and b[b_] == b[a_] and b[c_] == 2 ** 32
            assert b[-1] == K_MAX_BUCKET and b[-2] == K_MAX_BUCKET
            assert b[t0] > 12 * 2 ** 32
    # the bound of the docstring, for the graph without the two huge edges
    keep = case.w < 2.0 ** 1000
    small = csr_from_edges(case.n, case.src[keep], case.dst[keep], case.w[keep], symmetric=False)
    dd = O.sssp(small, 0)
    assert dd[np.isfinite(dd)].max() / default_delta(small, 0.5) <= small.nnz ** 2 / (0.5 * small.n)


@gpu
@pytest.mark.parametrize("symmetric", [False, True])
def test_bucket_numbers_past_2_33_without_knobs(ctx, monkeypatch, symmetric):
    """The magnitudes of case 1 with no knob set: the default rule's delta (1, through its
    non-finite fallback) puts vertices at buckets 2^32 - 32 (the "settle" shape at cur = 2^32 - 1),
    2^32, up to 13 * 2^32 and, behind the 2^1023 edges, at the kMaxBucket clamp."""
    case, _ = big_default_graph()
    check(ctx, monkeypatch, case, symmetric, ({}, {"GX_SSSP_FUSE": 0}))


# ------------------------------------------------------------------ case 3: kMaxBucket clamp, non-finite 1 / delta

CHAIN8_W = [1.0, 0.5, 2.0, 1.5, 0.75, 1.25, 1.0]


def chain(weights):
    k = len(weights)
    return Case(k + 1, np.arange(k), np.arange(1, k + 1), weights, 0, closed=path_sums)


@pytest.mark.parametrize("delta", [1e-300, 1e-310])
def test_chain8_construction(delta):
    case = chain(CHAIN8_W)
    want = np.concatenate([[0.0], np.cumsum(CHAIN8_W)])
    for symmetric in (False, True):
        csr = case.csr(symmetric)
        assert np.array_equal(O.sssp(csr, 0), want) and np.array_equal(path_sums(csr, 0), want)
    assert float(knob_str(delta)) == delta and delta > 0.0
    b = buckets(want, delta)
    assert all(x == K_MAX_BUCKET for x in b[1:])            # every positive distance clamps
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        inv = np.float64(1.0) / np.float64(delta)
        assert np.isinf(inv) == (delta == 1e-310)
        assert np.isnan(np.float64(0.0) * inv) == (delta == 1e-310)   # the source's own quotient


@gpu
@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("delta", [1e-300, 1e-310])
def test_max_bucket_clamp_and_infinite_inv_delta(ctx, monkeypatch, delta, symmetric):
    """The kMaxBucket clamp and a non-finite inv_delta: with GX_SSSP_DELTA=1e-300 every positive
    distance clamps to kMaxBucket and the window advances by overflow splits only; with 1e-310,
    1 / delta is inf and the source's 0 * inf is NaN.  8 vertices: a correct run is a few dozen
    steps, a run that does not converge ends at the step bound with an error, not a hang."""
    env = {"GX_SSSP_DELTA": knob_str(delta)}
    check(ctx, monkeypatch, chain(CHAIN8_W), symmetric, (env, {**env, "GX_SSSP_FUSE": 0}))


# ------------------------------------------------------------------ case 4: row chunks

CHUNK_LENS = [0, 1, 255, 256, 257, 512, 513]


def star(n_light, n_heavy):
    """Hub 0 under delta = 1 with n_light leaves at w < 1 and n_heavy at w >= 1 (the first exactly
    1 = delta); every leaf has one edge to a private tail, alternately light and heavy.  Vertices
    p (2.5 -> hub: a ring push) and q (0.25 -> hub: a near push) lead into the hub; they are only
    added to directed graphs, where they leave the hub's row alone."""
    src, dst, w = [], [], []
    n = 1
    for i in range(n_light + n_heavy):
        leaf, tail = n, n + 1
        n += 2
        wl = (1 + i % 127) / 256.0 if i < n_light else 1.0 + ((i - n_light) % 64) / 4.0
        src += [0, leaf]
        dst += [leaf, tail]
        w += [wl, 0.375 if i % 2 == 0 else 1.5]
    return Case(n, src, dst, w, 0, closed=path_sums)


def with_feeders(case):
    p, q = case.n, case.n + 1
    return Case(case.n + 2, np.append(case.src, [p, q]), np.append(case.dst, [0, 0]), np.append(case.w, [2.5, 0.25]),
                0, closed=path_sums), p, q


@pytest.mark.parametrize("n_light", CHUNK_LENS)
@pytest.mark.parametrize("n_heavy", CHUNK_LENS)
def test_star_construction(n_light, n_heavy):
    """The hub's light and heavy parts (what lend cuts the row into) have the lengths asked for."""
    case = star(n_light, n_heavy)
    for symmetric in (False, True):
        csr = case.csr(symmetric)
        hub = csr.vals[csr.rowptr[0]:csr.rowptr[1]]
        assert (int((hub < 1.0).sum()), int((hub >= 1.0).sum())) == (n_light, n_heavy)
        if n_heavy:
            assert hub[hub >= 1.0].min() == 1.0
        d = O.sssp(csr, 0)
        assert np.array_equal(d, path_sums(csr, 0)) and np.isfinite(d).all()
    if n_light + n_heavy:
        dcase, p, q = with_feeders(case)
        csr = dcase.csr(False)
        assert csr.rowptr[1] - csr.rowptr[0] == n_light + n_heavy
        for s in (p, q):
            assert np.array_equal(O.sssp(csr, s), path_sums(csr, s))


@gpu
@pytest.mark.parametrize("n_light", CHUNK_LENS)
@pytest.mark.parametrize("symmetric", [False, True])
def test_row_chunks(ctx, monkeypatch, n_light, symmetric):
    """Row chunks (kChunk = 256, chunks_of / chunks_min1): the hub's light part and heavy part each
    0, 1, 255, 256, 257, 512 and 513 edges long under GX_SSSP_DELTA=1; a private tail behind every
    leaf turns a chunk that is skipped, or read past its end, into a wrong distance.  Sources: the
    hub, and vertices that queue the hub by a near push and by a ring push (directed: the feeders
    q and p; undirected: a light and a heavy leaf)."""
    env = ({"GX_SSSP_DELTA": 1},)
    for n_heavy in CHUNK_LENS:
        case = star(n_light, n_heavy)
        sources = [0]
        if not symmetric and n_light + n_heavy:
            case, p, q = with_feeders(case)
            sources += [p, q]
        elif symmetric:
            sources += [1] if n_light + n_heavy else []                       # the first leaf
            sources += [2 * (n_light + n_heavy) - 1] if n_heavy and n_light else []   # the last (heavy) leaf
        check(ctx, monkeypatch, case, symmetric, env, sources)


# ------------------------------------------------------------------ case 5: the push stage

def push_star(n_leaves=3000):
    """Hub 0 with n_leaves leaves whose weights cycle, under delta = 1, through near (0.5), each of
    the 31 ring buckets (k + 0.5, k = 1..31) and the overflow (32.5 .. 71.5: the next window's ring
    and its overflow again); tails behind every leaf.  A second hub hangs off the first overflow
    leaf, with the same leaves and tails, so its pushes happen in a later window and the split
    of the overflow (mode 2) stages ring and overflow pushes of many categories as well."""
    src, dst, w = [], [], []
    n = 1
    first_ovf = None

    def hub(h):
        nonlocal n, first_ovf
        for i in range(n_leaves):
            c = i % 33
            wl = 0.5 if c == 0 else c + 0.5 if c < 32 else 32.5 + (i // 33) % 40
            leaf, tail = n, n + 1
            n += 2
            if c == 32 and first_ovf is None:
                first_ovf = leaf
            src.extend([h, leaf]), dst.extend([leaf, tail]), w.extend([wl, 0.25 if i % 2 else 1.75])

    hub(0)
    h2 = n
    n += 1
    src.append(first_ovf), dst.append(h2), w.append(0.5)
    hub(h2)
    return Case(n, src, dst, w, 0, closed=path_sums), h2


def test_push_star_construction():
    case, h2 = push_star()
    for symmetric in (False, True):
        csr = case.csr(symmetric)
        d = O.sssp(csr, 0)
        assert np.array_equal(d, path_sums(csr, 0)) and np.isfinite(d).all()
        for h, base in ((0, 0), (h2, int(d[h2]))):
            row = csr.colidx[csr.rowptr[h]:csr.rowptr[h + 1]].astype(np.int64)
            leaves = row[d[row] > d[h]]
            rel = np.array(buckets(d[leaves], 1.0)) - base
            near, ring, ovf = (rel == 0).sum(), [(rel == k).sum() for k in range(1, 32)], (rel >= 32).sum()
            assert near >= 90 and min(ring) >= 90 and ovf >= 90 and near + sum(ring) + ovf == 3000
            assert near + sum(ring) + ovf > 6 * 448        # the hub's pushes fill several 512-entry stages
            assert len(set(rel[rel >= 32])) == 40 and (rel >= 64).sum() > 0   # next window's ring, and past it
        assert buckets(d[[h2]], 1.0)[0] == 33                # reached in the second window


@gpu
@pytest.mark.parametrize("symmetric", [False, True])
def test_push_stage_every_category(ctx, monkeypatch, symmetric):
    """The push stage (kStage = 512, flush at > kStage - kWave): one launch stages the 3 000 pushes
    of a hub into every category at once -- near, each of the 31 ring slots, the overflow -- and
    the overflow split restages them for the next window; tails behind every leaf.  (A single
    wave's share stays below the mid-kernel flush: items are spread one per wave until the queue
    holds more items than the grid has waves, which needs millions of edges.)"""
    case, _ = push_star()
    check(ctx, monkeypatch, case, symmetric, ({"GX_SSSP_DELTA": 1}, {"GX_SSSP_DELTA": 1, "GX_SSSP_FUSE": 0}))


# ------------------------------------------------------------------ case 6: ring and overflow bookkeeping

FUSES = ({}, {"GX_SSSP_FUSE": 0}, {"GX_SSSP_FUSE": 3})


def stale_graph():
    """delta = 1.  Vertex 3 sits in ring slot 20 (edge 0 -> 3: 20.5) when the path 0-1-2-3 lowers
    it to slot 4 of the same window; vertex 5 sits on the overflow (50.5) when 3-4-5 lowers it into
    the ring (10.5); vertex 7 sits on the overflow (70.25) and is lowered there (52.5), to be found
    in the next window's ring.  The older entries are stale and must be skipped."""
    src = [0, 1, 2, 0, 3, 0, 4, 5, 0, 6, 7]
    dst = [1, 2, 3, 3, 4, 5, 5, 6, 7, 7, 8]
    w = [1.5, 1.5, 1.5, 20.5, 1.0, 50.5, 5.0, 40.0, 70.25, 2.0, 0.25]
    want = np.array([0, 1.5, 3.0, 4.5, 5.5, 10.5, 50.5, 52.5, 52.75])
    return Case(9, src, dst, w, 0, closed=want)


def test_ring_cases_construction():
    case = stale_graph()
    for symmetric in (False, True):
        assert np.array_equal(O.sssp(case.csr(symmetric), 0), case.closed)
    b = buckets(case.closed, 1.0)
    assert (b[3], b[5], b[7]) == (4, 10, 52)
    assert buckets([20.5, 50.5, 70.25], 1.0) == [20, 50, 70]     # where the stale entries were put
    d = np.arange(400.0)
    assert np.array_equal(O.sssp(chain(np.ones(399)).csr(True), 0), d)
    assert buckets(d, 1.0) == list(range(400))                     # 400 buckets: a split every 32
    assert np.diff(buckets(d, 1 / 64)).min() == 64 >= 32           # every hop overflows
    assert max(buckets(d, 64.0)) == 6


@gpu
@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("delta", [1.0, 1 / 64, 64.0])
def test_ring_wraps_and_overflow_splits(ctx, monkeypatch, delta, symmetric):
    """Ring and overflow bookkeeping: a 400-vertex chain of weight-1 edges is 400 buckets with a
    split every 32 at delta = 1, an overflow push per hop at delta = 1/64 and 7 buckets at
    delta = 64; with GX_SSSP_FUSE unset, 0 and 3."""
    envs = [{"GX_SSSP_DELTA": knob_str(delta), **f} for f in FUSES]
    check(ctx, monkeypatch, chain(np.ones(399)), symmetric, envs)


@gpu
@pytest.mark.parametrize("symmetric", [False, True])
def test_stale_ring_and_overflow_entries(ctx, monkeypatch, symmetric):
    """Ring and overflow bookkeeping: a later, shorter path lowers a vertex that already sits in a
    ring slot to a lower slot of the same window, one that sits on the overflow into the ring, and
    one within the overflow; the stale entries are skipped by dist == relaxed or by the stamp."""
    envs = [{"GX_SSSP_DELTA": 1, **f} for f in FUSES]
    check(ctx, monkeypatch, stale_graph(), symmetric, envs)


# ------------------------------------------------------------------ case 7: weight values

def zero_chain():
    return chain(np.append(np.zeros(300), 1.5))


def zero_cycle():
    """0 -> 1 (0.5), the zero-weight cycle 1 -> 2 -> 3 -> 1, 3 -> 4 (1.0)."""
    return Case(5, [0, 1, 2, 3, 3], [1, 2, 3, 1, 4], [0.5, 0.0, 0.0, 0.0, 1.0], 0,
                closed=np.array([0, 0.5, 0.5, 0.5, 1.5]))


def random_graph(n, m, weights, seed):
    rng = np.random.default_rng(seed)
    s, t = rng.integers(0, n, m), rng.integers(0, n, m)
    # one edge per unordered pair: stored symmetrically, (a, b) and (b, a) must carry one weight
    pairs = np.unique(np.stack([np.minimum(s, t), np.maximum(s, t)], axis=1)[s != t], axis=0)
    flip = rng.random(len(pairs)) < 0.5
    s, t = np.where(flip, pairs[:, 1], pairs[:, 0]), np.where(flip, pairs[:, 0], pairs[:, 1])
    return Case(n, s, t, weights(rng, len(pairs)), 0)


def extreme_chains(which):
    """Ten edges of 2^-1074 (denormal), ten of 2^1000, or both: one chain after the other from the
    source on two branches, and the huge chain continued by the denormal one."""
    tiny, huge = [2.0 ** -1074] * 10, [2.0 ** 1000] * 10
    if which == "tiny":
        return chain(tiny)
    if which == "huge":
        return chain(huge)
    src = [0] + list(range(1, 10)) + [0] + list(range(11, 30))
    dst = list(range(1, 11)) + list(range(11, 31))
    return Case(31, src, dst, tiny + huge + tiny, 0, closed=path_sums)


def grid(k=30):
    """k x k grid, right edges 0.75 and down edges 1.25: every monotone path to (i, j) has the same
    exact length, so every vertex off the border is a tie between at least two paths."""
    src, dst, w = [], [], []
    for i in range(k):
        for j in range(k):
            if j + 1 < k:
                src.append(i * k + j), dst.append(i * k + j + 1), w.append(0.75)
            if i + 1 < k:
                src.append(i * k + j), dst.append((i + 1) * k + j), w.append(1.25)
    ii, jj = np.divmod(np.arange(k * k), k)
    return Case(k * k, src, dst, w, 0, closed=jj * 0.75 + ii * 1.25)


def test_weight_cases_construction():
    for case in (zero_chain(), zero_cycle(), extreme_chains("tiny"), extreme_chains("huge"), extreme_chains("both"),
                 grid()):
        for symmetric in (False, True):
            csr = case.csr(symmetric)
            closed = case.closed(csr, 0) if callable(case.closed) else case.closed
            assert np.array_equal(O.sssp(csr, 0), closed)
    assert set(buckets(zero_chain().closed(zero_chain().csr(False), 0)[:-1], 1.0)) == {0}   # 300 rounds in bucket 0
    d = extreme_chains("both").closed(extreme_chains("both").csr(False), 0)
    assert d[10] == 10 * 2.0 ** -1074 and d[20] == 10 * 2.0 ** 1000 == d[30]    # the denormals are absorbed
    # the default rule on the denormal chain: delta underflows (directed: fallback 1) or 1 / delta is inf
    tiny = extreme_chains("tiny")
    assert default_delta(tiny.csr(False), 0.5) == 1.0
    with np.errstate(over="ignore", divide="ignore"):
        assert np.isinf(np.float64(1.0) / np.float64(default_delta(tiny.csr(True), 2.0)))
    # the random graphs: stored symmetrically they are symmetric in the weights too, all weights
    # equal delta or are integers, and most vertices are reached
    for case, delta in ((random_graph(300, 1200, lambda r, m: np.full(m, 0.75), 1), 0.75),
                        (random_graph(500, 2500, lambda r, m: r.integers(1, 10, m).astype(np.float64), 2), 1.0)):
        csr = case.csr(True)
        t = csr.transpose()
        assert np.array_equal(t.colidx, csr.colidx) and np.array_equal(t.vals, csr.vals)
        d = O.sssp(csr, 0)
        assert np.isfinite(d).sum() > 0.9 * case.n and not (case.w < delta).any()
        if delta == 1.0:
            assert np.array_equal(d[np.isfinite(d)], np.array(buckets(d[np.isfinite(d)], delta)))   # on boundaries
    g = grid()
    b = np.array(buckets(g.closed, 1.0))
    assert (g.closed == b).sum() > 100 and (g.closed != b).sum() > 100   # on and off bucket boundaries


@gpu
@pytest.mark.parametrize("symmetric", [False, True])
def test_zero_weights(ctx, monkeypatch, symmetric):
    """Weight values: a chain of 300 zero-weight edges is 300 near rounds inside bucket 0 (then one
    heavy edge), and a zero-weight cycle hanging off the source must not keep re-queuing; with the
    default width (mean weight ~0) and GX_SSSP_DELTA=1."""
    for case in (zero_chain(), zero_cycle()):
        check(ctx, monkeypatch, case, symmetric, ({}, {"GX_SSSP_DELTA": 1}))


@gpu
@pytest.mark.parametrize("symmetric", [False, True])
def test_weights_on_bucket_boundaries(ctx, monkeypatch, symmetric):
    """Weight values: all weights equal to delta (heavy: the test is w < delta), and integer
    weights with delta = 1, so every distance sits on a bucket boundary; a chain with a closed
    form and a random graph for each."""
    env34, env1 = {"GX_SSSP_DELTA": 0.75}, {"GX_SSSP_DELTA": 1}
    check(ctx, monkeypatch, chain(np.full(70, 0.75)), symmetric, (env34, {**env34, "GX_SSSP_FUSE": 0}))
    check(ctx, monkeypatch, random_graph(300, 1200, lambda r, m: np.full(m, 0.75), 1), symmetric, (env34,))
    check(ctx, monkeypatch, chain(1.0 + np.arange(70) % 5), symmetric, (env1, {**env1, "GX_SSSP_FUSE": 0}))
    check(ctx, monkeypatch, random_graph(500, 2500, lambda r, m: r.integers(1, 10, m).astype(np.float64), 2),
          symmetric, (env1, {**env1, "GX_SSSP_PULL": 2}))


@gpu
@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("which", ["tiny", "huge", "both"])
def test_denormal_and_huge_weights(ctx, monkeypatch, which, symmetric):
    """Weight values: 2^-1074 (denormal: the default width underflows or has an infinite inverse)
    and 2^1000, each on its own chain and then together in one graph, no knob set."""
    check(ctx, monkeypatch, extreme_chains(which), symmetric)


@gpu
@pytest.mark.parametrize("symmetric", [False, True])
def test_grid_ties(ctx, monkeypatch, symmetric):
    """Weight values: two or more equal-length paths to every inner vertex of a 30 x 30 grid
    (right 0.75, down 1.25), under the default width and GX_SSSP_DELTA=1 (light and heavy mixed)."""
    check(ctx, monkeypatch, grid(), symmetric, ({}, {"GX_SSSP_DELTA": 1}, {"GX_SSSP_DELTA": 1, "GX_SSSP_PULL": 2}))


# ------------------------------------------------------------------ case 8: degenerate graphs

def degenerate_cases():
    """name -> (case, directed-only, want)."""
    e = np.zeros(0)
    return {
        "n = 1": (Case(1, e, e, e, 0), False, [0.0]),
        "source with no edges": (Case(4, [1, 2], [2, 3], [1.0, 0.5], 0), False, [0.0, INF, INF, INF]),
        "source with only a self-loop": (Case(4, [0, 1, 2], [0, 2, 3], [0.25, 1.0, 0.5], 0), False,
                                         [0.0, INF, INF, INF]),
        "two components": (Case(6, [0, 1, 3, 4], [1, 2, 4, 5], [0.5, 1.5, 1.0, 1.0], 3), False,
                           [INF, INF, INF, 0.0, 1.0, 2.0]),
        "all edges into the source": (Case(5, [1, 2, 3, 4, 2], [0, 0, 0, 0, 1], [0.5, 1.0, 2.0, 0.25, 1.0], 0), True,
                                      [0.0, INF, INF, INF, INF]),
    }


DEGENERATE = sorted(degenerate_cases())


@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_construction(name):
    case, directed_only, want = degenerate_cases()[name]
    for symmetric in ((False,) if directed_only else (False, True)):
        assert O.sssp(case.csr(symmetric), case.source).tolist() == want


@gpu
@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_graphs(ctx, monkeypatch, name):
    """Degenerate graphs: n = 1; a source with no edges; a source with only a self-loop; two
    components; all edges leading into the source of a directed graph.  Unreached vertices read
    +inf."""
    case, directed_only, want = degenerate_cases()[name]
    case.closed = np.array(want)
    for symmetric in ((False,) if directed_only else (False, True)):
        check(ctx, monkeypatch, case, symmetric, ({}, {"GX_SSSP_DELTA": 1}))
