"""PageRank's pair slots (GX_PR_PAIRS=1; gather_pairs, gx_pr_sorted.hip): two entries of one
16-byte aligned pair of x per 4-byte slot in each block's hub prefix.  Every case against the
oracle at the parity bar of tests/test_gpu_parity.py; the model tool's counts on the CPU."""
import re
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


@pytest.fixture(autouse=True)
def pairs_on(monkeypatch):
    monkeypatch.setenv("GX_PR_PAIRS", "1")
    monkeypatch.setenv("GX_PR_PAIR_MIN", "256")


def _pr(ctx, csr, directed, iters):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    G = A.Graph(ctx, csr, directed)
    try:
        return A.LA_PR(G, 0.85, iters)
    finally:
        G.close()


def _check(ctx, csr, directed, iters):
    np.testing.assert_allclose(_pr(ctx, csr, directed, iters), O.pagerank(csr, directed, 0.85, iters),
                               rtol=PR_RTOL, atol=0)


_REF = {}


def _rmat_ref(spec, iters=10):
    """(csr, directed, oracle scores) of an R-MAT graph, computed once."""
    if spec not in _REF:
        from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat
        scale, ef, seed, undirected = spec
        csr = rmat(scale, ef, seed, undirected=undirected)
        _REF[spec] = (csr, not undirected, O.pagerank(csr, not undirected, 0.85, iters))
    return _REF[spec]


def _pair_stats(err):
    """(entries, filler halves) of the plan's pair slots from its GX_PR_VERBOSE=1 line."""
    m = re.search(r"pairs: (\d+) entries and (\d+) filler halves", err)
    assert m, err
    return int(m.group(1)), int(m.group(2))


@pytest.mark.gpu
def test_pairs_exact_supergroups(ctx, monkeypatch, capfd):
    """K(512, 1024) in 64-row blocks: every column pair of a block holds an even number of
    entries (128), so there is no filler and the blocks' 32 768 and 16 384 slots fill whole
    256-slot supergroups: the base after a block's last slot belongs to the next block and must
    not be written.  Every entry is in a slot."""
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
    monkeypatch.setenv("GX_PR_SORTED_ROWS", "64")
    monkeypatch.setenv("GX_PR_BLOCK_NNZ", "131072")
    monkeypatch.setenv("GX_PR_VERBOSE", "1")
    a = np.repeat(np.arange(512, dtype=np.int64), 1024)
    b = np.tile(np.arange(512, 1536, dtype=np.int64), 512)
    csr = csr_from_edges(1536, a, b, None, symmetric=True)
    capfd.readouterr()
    got = _pr(ctx, csr, False, 5)
    assert _pair_stats(capfd.readouterr().err) == (2 * 512 * 1024, 0)
    np.testing.assert_allclose(got, O.pagerank(csr, False, 0.85, 5), rtol=PR_RTOL, atol=0)


def _two_set_graph(in_a, per, m=512, nblk=8):
    """Directed: sources 0 .. 2m-1, all of out-degree nblk * per, so the hub-first order is the
    identity.  Source c points at `per` rows of each of nblk 64-row blocks: the blocks of set A
    when in_a(c), else those of set B.  A block of set A then holds `per` entries in each column c
    with in_a(c) and none elsewhere."""
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
    base = 2 * m   # a multiple of 64
    rows_a = np.array([base + 64 * b + i for b in range(nblk) for i in range(per)], dtype=np.int64)
    rows_b = rows_a + 64 * nblk
    src, dst = [], []
    for c in range(2 * m):
        rows = rows_a if in_a(c) else rows_b
        src.append(np.full(len(rows), c, dtype=np.int64))
        dst.append(rows)
    n = base + 2 * 64 * nblk + 5
    return csr_from_edges(n, np.concatenate(src), np.concatenate(dst), None, symmetric=False)


@pytest.mark.gpu
@pytest.mark.parametrize("per", [1, 63])
def test_pairs_odd_runs(ctx, monkeypatch, capfd, per):
    """Blocks with entries in every second column only (one entry per column, or 63): every
    column pair of a block holds an odd number of entries, so every run ends in a half filler."""
    monkeypatch.setenv("GX_PR_SORTED_ROWS", "64")
    monkeypatch.setenv("GX_PR_PAIR_FILL_COST", "0")
    monkeypatch.setenv("GX_PR_VERBOSE", "1")
    csr = _two_set_graph(lambda c: c % 2 == 0, per)
    capfd.readouterr()
    got = _pr(ctx, csr, True, 6)
    # 16 blocks x 512 pairs, one half filler each
    assert _pair_stats(capfd.readouterr().err) == (16 * 512 * per, 16 * 512)
    np.testing.assert_allclose(got, O.pagerank(csr, True, 0.85, 6), rtol=PR_RTOL, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("per", [1, 63])
def test_pairs_straddle(ctx, monkeypatch, per):
    """Blocks with entries only in columns 4q + 1 and 4q + 2 (the others: 4q and 4q + 3): sorted
    neighbours 4q + 1, 4q + 2 lie in different pairs of x and must not share a slot, although
    the first ends an odd run."""
    monkeypatch.setenv("GX_PR_SORTED_ROWS", "64")
    monkeypatch.setenv("GX_PR_PAIR_FILL_COST", "0")
    csr = _two_set_graph(lambda c: c % 4 in (1, 2), per)
    _check(ctx, csr, True, 6)


@pytest.mark.gpu
@pytest.mark.parametrize("unit", [None, "8192"])
def test_pairs_step_fillers(ctx, monkeypatch, capfd, unit):
    """The 6-regular multiplicative graph of test_pagerank_narrow_fillers: column steps of all
    sizes; with fillers free every block is pair-coded whole, steps above 3 split by filler
    slots.  Also with blocks cut into units."""
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
    monkeypatch.setenv("GX_PR_PAIR_FILL_COST", "0")
    monkeypatch.setenv("GX_PR_VERBOSE", "1")
    if unit:
        monkeypatch.setenv("GX_PR_UNIT_NNZ", unit)
    n = 200003   # prime: v -> m v is a permutation
    v = np.arange(1, n, dtype=np.int64)
    src = np.concatenate([v, v, v])
    dst = np.concatenate([(5 * v) % n, (7 * v) % n, (11 * v) % n])
    keep = src != dst
    csr = csr_from_edges(n, src[keep], dst[keep], None, symmetric=True)
    capfd.readouterr()
    got = _pr(ctx, csr, False, 8)
    entries, fillers = _pair_stats(capfd.readouterr().err)
    assert entries == int(csr.rowptr[-1]) and fillers > entries   # sparse columns: mostly step fillers
    np.testing.assert_allclose(got, O.pagerank(csr, False, 0.85, 8), rtol=PR_RTOL, atol=0)


VARIANTS = [{}, {"GX_PR_PAIRS": "0"},
            {"GX_PR_UNIT_NNZ": "8192", "GX_PR_BLOCK_NNZ": "65536", "GX_PR_QUEUE": "1"},
            {"GX_PR_UNIT_NNZ": "8192", "GX_PR_BLOCK_NNZ": "65536", "GX_PR_COMBINE": "1"},
            {"GX_PR_CP": "5", "GX_PR_NT_COL": "1000"},
            {"GX_PR_NARROW": "0"},
            {"GX_PR_LONG_NNZ": "1024"},
            {"GX_PR_PAIR_FILL_COST": "0", "GX_PR_UNIT_NNZ": "8192", "GX_PR_BLOCK_NNZ": "65536"}]


@pytest.mark.gpu
@pytest.mark.parametrize("env", VARIANTS, ids=lambda e: ",".join(f"{k[6:]}={v}" for k, v in e.items()) or "default")
def test_pairs_plan_variants(ctx, monkeypatch, env):
    """Pair prefix, narrow codes and wide entries together under the plan's modes: off, blocks
    cut into interleaved units under the work queue and under the combine kernel, non-temporal
    gathers past column 1000, no narrow codes (pairs then wide), LONG rows, fillers free."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for spec in ((14, 16, 4, True), (11, 8, 3, False)):
        csr, directed, want = _rmat_ref(spec)
        np.testing.assert_allclose(_pr(ctx, csr, directed, 10), want, rtol=PR_RTOL, atol=0)


@pytest.mark.gpu
def test_pairs_long_row_segments(ctx):
    """The 150 001-vertex hub-row graph of test_pagerank_long_row_segments: a LONG row beside
    sorted blocks whose first column (the hub) holds most of their entries."""
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
    n = 150001
    rng = np.random.default_rng(3)
    a, b = rng.integers(1, n, 200000), rng.integers(1, n, 200000)
    keep = a != b
    src = np.concatenate([np.zeros(n - 1, np.int64), a[keep]])
    dst = np.concatenate([np.arange(1, n, dtype=np.int64), b[keep]])
    csr = csr_from_edges(n, src, dst, None, symmetric=True)
    _check(ctx, csr, False, 6)


@pytest.mark.gpu
@pytest.mark.parametrize("nranks,live", [(2, True), (2, False), (3, False)])
def test_pairs_partitioned(nranks, live):
    """gx_pr_part_* with two and three ranks simulated on one device (as
    tests/test_distributed.py builds them): a pair of the exchanged vector never straddles two
    ranks' chunks, because every chunk is padded to an even length (a multiple of 32) -- also
    where the largest rank's rows + 2 padding slots are odd ((2, False): 3879, (3, False): 3661)."""
    import torch
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat
    from ldbc_graphalytics_platforms_graphblas_amd.pr_partition import GpuStep, hub_relabel, local_rows
    csr = rmat(12, 16, 11)
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
    need = int(max(np.diff(lrs[0].row_ranges.astype(np.int64))) if not live else max(lrs[0].live)) + 2
    assert (need % 2 == 1) == (not live) and chunk >= need and chunk % 2 == 0
    xl = [torch.zeros(chunk, dtype=torch.float64, device=dev) for _ in range(nranks)]
    xf = torch.zeros(chunk * nranks, dtype=torch.float64, device=dev)
    ro = [torch.zeros(max(lr.rows, 1), dtype=torch.float64, device=dev) for lr in lrs]
    iters = 6
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
    np.testing.assert_allclose(got, O.pagerank(csr, False, 0.85, iters), rtol=PR_RTOL)


def test_pair_model_counts():
    """tools/pr_pair_model.py on rmat(12, 8, 1): slots x 2 - fillers = covered entries for every
    rule, and the two entries of a slot lie in one column pair of one block."""
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat
    sys.path.insert(0, str(ROOT / "tools"))
    try:
        import pr_pair_model as M
    finally:
        sys.path.pop(0)
    blk, col = M.sorted_blocks(rmat(12, 8, 1), R=256, B=8192)
    assert blk[-1] > 0 and (np.diff(blk) >= 0).all()
    prefix = col < 1024
    named = M.rules(blk, col) + [("columns below 1024", prefix, True), ("columns below 1023 (odd cut)", col < 1023, True)]
    for name, covered, is_prefix in named:
        st = M.pair_slots(blk, col, covered, step_fillers=is_prefix)
        assert st["slots"] * 2 - st["fillers"] == st["covered"] == int(covered.sum()), name
        lead, partner = st["lead"], st["partner"]
        both = partner >= 0
        assert covered[lead].all() and covered[partner[both]].all(), name
        assert (col[lead[both]] >> 1 == col[partner[both]] >> 1).all() and (blk[lead[both]] == blk[partner[both]]).all(), name
        # every covered entry is in exactly one slot
        seen = np.concatenate([lead, partner[both]])
        assert len(seen) == st["covered"] and len(np.unique(seen)) == len(seen), name
    # a prefix by columns covers a prefix of every block's sorted entries
    st = M.pair_slots(blk, col, prefix)
    assert st["covered"] > 0 and st["half"] > 0
    first = np.flatnonzero(np.diff(blk, prepend=-1))
    for z0, z1 in zip(first, np.append(first[1:], len(blk))):
        k = int(prefix[z0:z1].sum())
        assert prefix[z0:z0 + k].all()
