"""PageRank's bank-aware order inside column runs (GX_PR_BANK_ORDER; k_bank_order,
gx_pr_plan.hip) and the isolated rows in closed form (GX_PR_ISO_CLOSED).  Every GPU case runs
with the knob on and off, each against the fp64 oracle at the parity bar of
tests/test_gpu_parity.py, and the two against each other; the deal itself and the model's counts
are checked on the CPU."""
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as O

PR_RTOL = 1e-12


@pytest.fixture(scope="module")
def ctx():
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    c = Context(0)
    yield c
    c.close()


def _pr(ctx, csr, directed, iters, calls=1):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    G = A.Graph(ctx, csr, directed)
    try:
        for _ in range(calls):
            got = A.LA_PR(G, 0.85, iters)
        return got
    finally:
        G.close()


def _on_off(ctx, monkeypatch, knob, csr, directed, iters, want=None, calls=1):
    """Scores with `knob` on, checked against the oracle and against the scores with it off."""
    if want is None:
        want = O.pagerank(csr, directed, 0.85, iters)
    got = {}
    for v in ("1", "0"):
        monkeypatch.setenv(knob, v)
        got[v] = _pr(ctx, csr, directed, iters, calls)
        np.testing.assert_allclose(got[v], want, rtol=PR_RTOL, atol=0)
    np.testing.assert_allclose(got["1"], got["0"], rtol=PR_RTOL, atol=0)
    return got["1"]


def _edges(n, src, dst, symmetric):
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
    return csr_from_edges(n, np.concatenate(src), np.concatenate(dst), None, symmetric=symmetric)


# ---- bank order ---------------------------------------------------------------------------

@pytest.fixture
def bank_env(monkeypatch):
    monkeypatch.setenv("GX_PR_PAIRS", "1")
    monkeypatch.setenv("GX_PR_PAIR_MIN", "256")
    monkeypatch.setenv("GX_PR_ISO_CLOSED", "1")


def _hub_graph(n, hubs, extra, seed):
    """Directed: `hubs` vertices that every other vertex is reached from (the densest columns of
    every block), plus `extra` random edges among the others."""
    rng = np.random.default_rng(seed)
    rest = np.arange(hubs, n, dtype=np.int64)
    src = [np.full(len(rest), h, dtype=np.int64) for h in range(hubs)]
    dst = [rest] * hubs
    a, b = rng.integers(hubs, n, extra), rng.integers(hubs, n, extra)
    keep = a != b
    return _edges(n, src + [a[keep]], dst + [b[keep]], False)


HUB_MODES = [{"GX_PR_QUEUE": "1"}, {"GX_PR_QUEUE": "0"}, {"GX_PR_COMBINE": "1"}]
_HUB = {}


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["16320", "64"])
@pytest.mark.parametrize("mode", HUB_MODES, ids=lambda e: ",".join(f"{k[6:]}={v}" for k, v in e.items()))
def test_bank_hub_runs(ctx, monkeypatch, bank_env, rows, mode):
    """Three hub columns that every row reaches, beside sparse columns.  A run holds at most one
    entry per row of its block, so with 16 320-row blocks the hubs' pair run (about 32 Ki entries)
    and column runs are longer than a 256-entry supergroup and than an 8 Ki-entry round, and with
    8 Ki-entry units they cross supergroup, round, unit and (2 Ki-entry) tile boundaries; with 64-row
    blocks a tile holds the short runs of several blocks' worth of columns.  Under the work queue, without it, and with the combine kernel."""
    monkeypatch.setenv("GX_PR_SORTED_ROWS", rows)
    monkeypatch.setenv("GX_PR_BLOCK_NNZ", "131072")
    monkeypatch.setenv("GX_PR_UNIT_NNZ", "8192")
    for k, v in mode.items():
        monkeypatch.setenv(k, v)
    if "g" not in _HUB:
        csr = _hub_graph(20000, 3, 60000, 5)
        _HUB["g"] = (csr, O.pagerank(csr, True, 0.85, 5))
    csr, want = _HUB["g"]
    _on_off(ctx, monkeypatch, "GX_PR_BANK_ORDER", csr, True, 5, want)


def _column_graph(nsrc, nblk, rows_of):
    """Directed: source c of 0 .. nsrc-1 points at rows rows_of(c) (numbers below 64) of each of nblk
    64-row blocks of sinks.  The hub-first order renames the sources by out-degree and keeps the
    sinks where they are (nsrc is rounded up to whole blocks)."""
    base = (nsrc + 63) // 64 * 64
    src, dst = [], []
    for c in range(nsrc):
        r = np.asarray(rows_of(c), dtype=np.int64)
        rows = (base + 64 * np.arange(nblk, dtype=np.int64)[:, None] + r[None, :]).ravel()
        src.append(np.full(len(rows), c, dtype=np.int64))
        dst.append(rows)
    return _edges(base + 64 * nblk + 3, src, dst, False)


@pytest.mark.gpu
def test_bank_short_runs(ctx, monkeypatch, bank_env):
    """Runs of 1 .. 15 entries only: column c holds 1 + c mod 15 entries of every 64-row block,
    at rows spread by a stride, so pieces of several runs share every tile."""
    monkeypatch.setenv("GX_PR_SORTED_ROWS", "64")
    monkeypatch.setenv("GX_PR_PAIR_FILL_COST", "0")
    csr = _column_graph(480, 6, lambda c: (7 * np.arange(1 + c % 15) + 3 * c) % 64)
    _on_off(ctx, monkeypatch, "GX_PR_BANK_ORDER", csr, True, 6)


@pytest.mark.gpu
def test_bank_few_rows(ctx, monkeypatch, bank_env):
    """Blocks of 8 rows (512 entries per row, 4 Ki entries per block): every 16-lane group holds
    rows that collide whatever the order."""
    monkeypatch.setenv("GX_PR_SORTED_ROWS", "64")
    monkeypatch.setenv("GX_PR_BLOCK_NNZ", "4096")
    csr = _column_graph(512, 2, lambda c: np.arange(64))
    _on_off(ctx, monkeypatch, "GX_PR_BANK_ORDER", csr, True, 5)


@pytest.mark.gpu
def test_bank_one_class(ctx, monkeypatch, bank_env):
    """Every run's rows are 0 mod 16 (64 of them per 1 Ki-row block): one class, nothing to spread,
    beside columns whose rows are all 5 mod 16."""
    monkeypatch.setenv("GX_PR_SORTED_ROWS", "1024")
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
    nsrc, base = 256, 256
    rows = base + 16 * np.arange(2 * 64, dtype=np.int64)
    src = np.repeat(np.arange(nsrc, dtype=np.int64), len(rows))
    dst = np.tile(rows, nsrc) + np.repeat(np.where(np.arange(nsrc) % 3 == 0, 5, 0), len(rows))
    csr = csr_from_edges(base + 2048 + 7, src, dst, None, symmetric=False)
    _on_off(ctx, monkeypatch, "GX_PR_BANK_ORDER", csr, True, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("per", [1, 5, 63])
def test_bank_odd_pair_runs(ctx, monkeypatch, bank_env, per):
    """tests/test_pr_pairs.py's two-set graph: blocks with entries in every second column only, so
    one column of each pair is empty, every pair run is odd (1, 5 or 63 entries) and ends in a half
    filler, which the permutation must leave in the run's last slot."""
    monkeypatch.setenv("GX_PR_SORTED_ROWS", "64")
    monkeypatch.setenv("GX_PR_PAIR_FILL_COST", "0")
    m, nblk = 512, 8
    base = 2 * m
    rows_a = np.array([base + 64 * b + (11 * i) % 64 for b in range(nblk) for i in range(per)], dtype=np.int64)
    src, dst = [], []
    for c in range(2 * m):
        rows = rows_a if c % 2 == 0 else rows_a + 64 * nblk
        src.append(np.full(len(rows), c, dtype=np.int64))
        dst.append(rows)
    csr = _edges(base + 2 * 64 * nblk + 5, src, dst, False)
    _on_off(ctx, monkeypatch, "GX_PR_BANK_ORDER", csr, True, 6)


@pytest.mark.gpu
def test_bank_step_fillers(ctx, monkeypatch, bank_env):
    """The 6-regular multiplicative graph of test_pairs_step_fillers: column gaps of all sizes
    inside both prefixes, so filler slots and filler codes sit between the runs."""
    monkeypatch.setenv("GX_PR_PAIR_FILL_COST", "0")
    monkeypatch.setenv("GX_PR_UNIT_NNZ", "8192")
    n = 200003
    v = np.arange(1, n, dtype=np.int64)
    src = np.concatenate([v, v, v])
    dst = np.concatenate([(5 * v) % n, (7 * v) % n, (11 * v) % n])
    keep = src != dst
    csr = _edges(n, [src[keep]], [dst[keep]], True)
    _on_off(ctx, monkeypatch, "GX_PR_BANK_ORDER", csr, False, 8)


@pytest.mark.gpu
def test_bank_escape_supergroups(ctx, monkeypatch, bank_env):
    """The perfect matching on 2^21 + 64 vertices in 64-row blocks of test_gpu_parity.py, the
    smallest shape with escape supergroups (a supergroup's columns span 2^18 ids): they stay in
    the wide part, which the order does not touch."""
    monkeypatch.setenv("GX_PR_SORTED_ROWS", "64")
    n = (1 << 21) + 64
    perm = np.random.default_rng(9).permutation(n)
    csr = _edges(n, [perm[0::2]], [perm[1::2]], True)
    _on_off(ctx, monkeypatch, "GX_PR_BANK_ORDER", csr, False, 4)


_RMAT = {}


def _rmat_ref(spec, iters=10):
    if spec not in _RMAT:
        from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat
        scale, ef, seed, undirected = spec
        csr = rmat(scale, ef, seed, undirected=undirected)
        _RMAT[spec] = (csr, not undirected, O.pagerank(csr, not undirected, 0.85, iters))
    return _RMAT[spec]


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"GX_PR_PAIRS": "0"}, {"GX_PR_NARROW": "0"}, {"GX_PR_PAIRS": "0", "GX_PR_NARROW": "0"},
                                 {"GX_PR_LONG_NNZ": "1024"}],
                         ids=lambda e: ",".join(f"{k[6:]}={v}" for k, v in e.items()) or "default")
def test_bank_regions(ctx, monkeypatch, bank_env, env):
    """R-MAT graphs with the pair prefix, the narrow prefix or both switched off (the order then
    has nothing to do in that region, or anywhere), and beside LONG rows."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for spec in ((14, 16, 4, True), (11, 8, 3, False)):
        csr, directed, want = _rmat_ref(spec)
        _on_off(ctx, monkeypatch, "GX_PR_BANK_ORDER", csr, directed, 10, want)


def _partitioned(csr, nranks, live, iters, runs=1):
    """gx_pr_part_* with `nranks` ranks simulated on one device, as tests/test_pr_pairs.py runs
    them; `runs` runs in a row on the same plans (the scores of the last)."""
    import torch
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    from ldbc_graphalytics_platforms_graphblas_amd.pr_partition import GpuStep, hub_relabel, local_rows
    perm, hub = hub_relabel(csr)
    c = Context(0)
    dev = torch.device("cuda", 0)
    steps, lrs = [], []
    for r in range(nranks):
        lr = local_rows(hub, directed=False, nranks=nranks, rank=r)
        if not live:
            lr.live = None
        lrs.append(lr)
        steps.append(GpuStep(c, csr.n, nranks, lr, 0.85))
    chunk = steps[0].chunk
    xl = [torch.zeros(chunk, dtype=torch.float64, device=dev) for _ in range(nranks)]
    xf = torch.zeros(chunk * nranks, dtype=torch.float64, device=dev)
    ro = [torch.zeros(max(lr.rows, 1), dtype=torch.float64, device=dev) for lr in lrs]
    for _ in range(runs):
        for r in range(nranks):
            steps[r].init(xl[r], 0)
        torch.cuda.synchronize()
        xf.copy_(torch.cat(xl))
        for it in range(iters):
            for r in range(nranks):
                steps[r].step(xf, xl[r], ro[r] if it == iters - 1 else None, 0)
            torch.cuda.synchronize()
            xf.copy_(torch.cat(xl))
    got = np.concatenate([ro[r][:lrs[r].rows].cpu().numpy() for r in range(nranks)])[perm]
    for s in steps:
        s.close()
    c.close()
    return got


def _partitioned_on_off(monkeypatch, knob, csr, nranks, live, iters, want, runs=1):
    got = {}
    for v in ("1", "0"):
        monkeypatch.setenv(knob, v)
        got[v] = _partitioned(csr, nranks, live, iters, runs)
        np.testing.assert_allclose(got[v], want, rtol=PR_RTOL, atol=0)
    np.testing.assert_allclose(got["1"], got["0"], rtol=PR_RTOL, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("nranks,live", [(2, True), (3, False)])
def test_bank_partitioned(monkeypatch, bank_env, nranks, live):
    """Two and three ranks on one device, 64-row blocks: every rank's plan orders its own runs."""
    monkeypatch.setenv("GX_PR_SORTED_ROWS", "64")
    csr, _, want = _rmat_ref((12, 16, 11, True), 6)
    _partitioned_on_off(monkeypatch, "GX_PR_BANK_ORDER", csr, nranks, live, 6, want)


def test_bank_deal_native(tmp_path):
    """csrc/gx_pr_bank.h on hand-made runs (tests/native/bank_order_check.cpp): a bijection, rounds
    of distinct classes, full windows distinct while the counts allow, the uneven tail, the pair
    form."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "bank_order_check"
    inc = ROOT / "ldbc_graphalytics_platforms_graphblas_amd" / "csrc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{inc}", str(ROOT / "tests" / "native" / "bank_order_check.cpp"),
                    "-o", str(exe)], check=True, timeout=120)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "bank order ok" in out.stdout, out.stdout + out.stderr


def _model():
    sys.path.insert(0, str(ROOT / "tools"))
    try:
        import pr_bank_model as M
    finally:
        sys.path.pop(0)
    return M


def test_bank_model_maps():
    """The model's lane <-> entry maps on a tiny hand-made block, against the decode of
    gather_pairs and gather_narrow: slot (code) e of a supergroup is lane e mod 64 of instruction
    e / 64, so a 16-lane group is 16 consecutive slots (codes); a run's entries pair up from its
    start, an odd run ends in a junk half, a pair step above 3 puts filler slots (junk rows
    16320 + lane) before the run, a column step above 3 filler codes."""
    M = _model()
    # pair prefix: pair 0 holds columns 0, 0, 1 (rows 5, 9, 2); pair 4 holds column 9 (rows 7, 1)
    col = np.array([0, 0, 1, 9, 9], dtype=np.int64)
    row = np.array([5, 9, 2, 7, 1], dtype=np.int64)
    ra, rb = M.pair_slots(col, row, 1)
    assert len(ra) == 256 and len(rb) == 256
    # slots: (5, 9), (2, junk), one filler slot for the step of 4 pairs, (7, 1), then padding
    assert ra[:4].tolist() == [5, 2, 16320 + 2, 7]
    assert rb[:4].tolist() == [9, 16320 + 1, 16320 + 2, 1]
    assert (ra[4:] == 16320 + (np.arange(4, 256) & 63)).all() and (rb[4:] == ra[4:]).all()
    # narrow codes of the same entries (Q = 0, P = 1): the step 1 -> 9 takes ceil(8 / 3) - 1 = 2 fillers
    nc = M.narrow_codes(col, row, 0, 1)
    assert len(nc) == 512
    assert nc[:7].tolist() == [5, 9, 2, 16320 + 3, 16320 + 4, 7, 1]
    # the wide part: group j of a 64-entry group is its positions 4 s + j
    g = M.wide_groups(np.arange(64, dtype=np.int64))
    assert g.shape == (4, 16) and g[1].tolist() == list(range(1, 64, 4))
    # the deal of one piece: gx_pr_bank.h's order (the native check's uneven example)
    rows = [3, 19, 35, 5, 51, 9, 67, 83, 21, 99, 115, 131]
    assert M.deal_piece(rows).tolist() == [0, 3, 5, 1, 8, 2, 4, 6, 7, 9, 10, 11]


def test_bank_model_cycles_by_hand():
    """The model's cycle count of a tiny block by hand.  One column holding rows 0, 16, 32, 48, 1,
    17, 33, 49, ..., 15, 31, 47, 63 in ascending order is rows 0 .. 63: every group of 16
    consecutive codes holds 16 distinct classes.  The same rows times 16 are all of class 0: 16
    cycles a group.  Rows 0, 16, 32, ... in runs of four classes' worth collide four ways before
    the deal and not after it."""
    M = _model()
    col = np.zeros(64, dtype=np.int64)
    row = np.arange(64, dtype=np.int64)
    # narrow only (no pairs): 512 codes = 32 groups, 4 of them real, 28 of junk rows 16320 + lane
    assert M.block_cycles(col, row, 0, 1)["narrow"] == (32, 32)
    assert M.block_cycles(col, 16 * row, 0, 1)["narrow"] == (32, 28 + 4 * 16)
    # rows 0, 16, 32, 48 | 1, 17, 33, 49 | ...: ascending order would not be this, but a block may
    # hold them in two columns' runs; as one run: four classes per group, four rows each
    r4 = (np.arange(64) // 4 + 16 * (np.arange(64) % 4)).astype(np.int64)
    assert M.block_cycles(col, r4, 0, 1)["narrow"] == (32, 28 + 4 * 4)
    c2, r2 = M.bank_order(col, r4, 0, 1)
    assert sorted(r2.tolist()) == sorted(r4.tolist()) and (c2 == col).all()
    assert M.block_cycles(c2, r2, 0, 1)["narrow"] == (32, 32)
    # as a pair run (Q = 1): 32 slots, first halves the first 32 dealt entries, second halves the rest
    ra, rb = M.pair_slots(*M.bank_order(col, r4, 1, 1), 1)
    assert sorted(ra[:32].tolist() + rb[:32].tolist()) == sorted(r4.tolist())
    assert M.block_cycles(*M.bank_order(col, r4, 1, 1), 1, 1)["pair"] == (32, 32)
    assert M.block_cycles(col, r4, 1, 1)["pair"] == (32, 28 + 4 * 2)   # rows 0, 32 | 1, 33 | ... per half
    # equal rows of a group: one cycle when they combine, else serialised
    same = np.zeros((1, 16), dtype=np.int64)
    assert M.group_cycles(same) == 16 and M.group_cycles(same, combine=True) == 1


# ---- isolated rows in closed form ---------------------------------------------------------

def _iso_stats(err):
    m = re.findall(r"closed-form isolated rows: (\d+) of (\d+) units, (\d+) rows, (\d+) of (\d+) dangling slots", err)
    assert m, err
    return tuple(int(v) for v in m[-1])


def _ring(nlive, niso, chords=()):
    """Undirected: a ring over vertices 0 .. nlive-1 plus the chords v -- v + k, and niso vertices
    without any edge."""
    v = np.arange(nlive, dtype=np.int64)
    src, dst = [v], [(v + 1) % nlive]
    for k in chords:
        src.append(v)
        dst.append((v + k) % nlive)
    return _edges(nlive + niso, src, dst, True)


@pytest.fixture
def iso_env(monkeypatch):
    monkeypatch.setenv("GX_PR_SORTED_ROWS", "64")
    monkeypatch.setenv("GX_PR_VERBOSE", "1")


@pytest.mark.gpu
@pytest.mark.parametrize("queue", ["1", "0"])
@pytest.mark.parametrize("iters", [1, 2, 10])
def test_iso_undirected(ctx, monkeypatch, capfd, iso_env, iters, queue):
    """A ring with chords over 1000 vertices and 170 isolated vertices in 64-row blocks: the block holding rows 960 .. 1023 mixes live and isolated
    rows and keeps its path, two whole blocks of isolated rows and the 18-row tail are left out of
    every launch but the last.  With one iteration the only launch is the last."""
    monkeypatch.setenv("GX_PR_QUEUE", queue)
    csr = _ring(1000, 170, chords=(7, 31))
    capfd.readouterr()
    _on_off(ctx, monkeypatch, "GX_PR_ISO_CLOSED", csr, False, iters)
    err = capfd.readouterr().err
    on = re.findall(r"closed-form isolated rows: (\d+) of \d+ units, (\d+) rows", err)
    assert ("3", "146") in on and ("0", "0") in on, err   # knob on: 3 blocks, 64 + 64 + 18 rows; off: none


@pytest.mark.gpu
@pytest.mark.parametrize("queue", ["1", "0"])
def test_iso_only_dangling(ctx, monkeypatch, capfd, iso_env, queue):
    """1024 ring vertices (16 whole blocks, none dangling) and 128 isolated ones (2 whole blocks):
    the isolated blocks hold every dangling slot, so no block publishes a partial and item 0
    writes the sum.  Two calls on one plan."""
    monkeypatch.setenv("GX_PR_QUEUE", queue)
    monkeypatch.setenv("GX_PR_ISO_CLOSED", "1")
    csr = _ring(1024, 128, chords=(5,))
    capfd.readouterr()
    got = _pr(ctx, csr, False, 4, calls=2)
    assert _iso_stats(capfd.readouterr().err) == (2, 18, 128, 2, 2)
    np.testing.assert_allclose(got, O.pagerank(csr, False, 0.85, 4), rtol=PR_RTOL, atol=0)
    _on_off(ctx, monkeypatch, "GX_PR_ISO_CLOSED", csr, False, 4, calls=2)


@pytest.mark.gpu
@pytest.mark.parametrize("queue", ["1", "0"])
@pytest.mark.parametrize("iters", [1, 2, 10])
def test_iso_directed_sources(ctx, monkeypatch, capfd, iso_env, iters, queue):
    """Directed: 128 source-only vertices (no in-edge, 40 out-edges each: two whole blocks without
    entries whose rows still need x' = r / (outdeg / d)), 1000 ring vertices with one or two
    out-edges, 60 sinks (in-edges only: dangling rows with entries) and 150 vertices without any edge
    (the last two blocks, closed-form, after a block that mixes sinks and isolated rows)."""
    monkeypatch.setenv("GX_PR_QUEUE", queue)
    ns, nr, nk, ni = 128, 1000, 60, 150
    s = np.arange(ns, dtype=np.int64)
    ring = ns + np.arange(nr, dtype=np.int64)
    src = [np.repeat(s, 40), ring, ring[::3], ring[:nk]]
    dst = [ns + (np.repeat(s, 40) * 7 + np.tile(np.arange(40), ns) * 13) % nr, ns + (ring - ns + 1) % nr,
           ns + (ring[::3] - ns + 17) % nr, ns + nr + np.arange(nk, dtype=np.int64)]
    csr = _edges(ns + nr + nk + ni, src, dst, False)
    capfd.readouterr()
    _on_off(ctx, monkeypatch, "GX_PR_ISO_CLOSED", csr, True, iters, calls=2)
    on = re.findall(r"closed-form isolated rows: (\d+) of \d+ units, (\d+) rows", capfd.readouterr().err)
    assert any(int(u) >= 2 and int(r) >= 100 for u, r in on) and ("0", "0") in on, on


@pytest.mark.gpu
@pytest.mark.parametrize("nranks,live", [(2, True), (2, False), (3, True), (3, False)])
def test_iso_partitioned(monkeypatch, iso_env, nranks, live):
    """Two and three ranks on one device over R-MAT scale 12 (a quarter of its vertices isolated),
    with the live prefix (the isolated rows' x in xd) and without it (every row in the chunk), two
    runs in a row on the same plans: the ticket's count changes between a run's last launch and
    the next run's first."""
    csr, _, want = _rmat_ref((12, 16, 11, True), 6)
    _partitioned_on_off(monkeypatch, "GX_PR_ISO_CLOSED", csr, nranks, live, 6, want, runs=2)
