"""PageRank's run groups (GX_PR_RUNS=1; gather_runs, gx_pr_sorted.hip, gx_pr_runs.h): 64 two-byte
codes of one column pair per group in each block's run region, ahead of its pair prefix.  Every
GPU case against the oracle at the parity bar of tests/test_gpu_parity.py; the layout arithmetic
and the model tool's counts on the CPU."""
import re
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as O

PR_RTOL = 1e-12
CSRC = ROOT / "ldbc_graphalytics_platforms_graphblas_amd" / "csrc"


@pytest.fixture(scope="module")
def ctx():
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def runs_on(monkeypatch):
    monkeypatch.setenv("GX_PR_RUNS", "1")
    monkeypatch.setenv("GX_PR_PAIRS", "1")
    monkeypatch.setenv("GX_PR_RUN_MIN", "256")
    monkeypatch.setenv("GX_PR_PAIR_MIN", "256")


def _model():
    sys.path.insert(0, str(ROOT / "tools"))
    try:
        import pr_bank_model as B
        import pr_run_model as M
    finally:
        sys.path.pop(0)
    return B, M


def _pr(ctx, csr, directed, iters):
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    G = A.Graph(ctx, csr, directed)
    try:
        return A.LA_PR(G, 0.85, iters)
    finally:
        G.close()


def _run_stats(err):
    """(entries, padding codes, blocks with a run prefix) of the last plan's GX_PR_VERBOSE=1 line."""
    m = re.findall(r"runs: (\d+) entries and (\d+) padding codes in \d+ codes[^;]*; (\d+) of \d+ blocks", err)
    assert m, err
    return tuple(int(v) for v in m[-1])


def _pair_stats(err):
    m = re.findall(r"pairs: (\d+) entries and (\d+) filler halves", err)
    assert m, err
    return tuple(int(v) for v in m[-1])


def _narrow_entries(err):
    m = re.findall(r"narrow (\d+) entries in", err)
    assert m, err
    return int(m[-1])


def _plan_stats(err):
    """(sorted blocks, units, multi-unit blocks) of the last plan's GX_PR_VERBOSE=1 line."""
    m = re.findall(r"(\d+) sorted blocks, .*? (\d+) units, (\d+) multi-unit blocks", err)
    assert m, err
    return tuple(int(v) for v in m[-1])


def _k512_1024():
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
    a = np.repeat(np.arange(512, dtype=np.int64), 1024)
    b = np.tile(np.arange(512, 1536, dtype=np.int64), 512)
    return csr_from_edges(1536, a, b, None, symmetric=True)


@pytest.mark.gpu
def test_runs_exact_groups(ctx, monkeypatch, capfd):
    """K(512, 1024) in 64-row blocks: every column pair of a block holds 128 entries, two whole
    groups, so there is no padding, every entry is a run code, and the blocks' 65 536 and 32 768
    codes fill whole 512-code supergroups: the header after a block's last group belongs to the
    next block and must not be written."""
    monkeypatch.setenv("GX_PR_SORTED_ROWS", "64")
    monkeypatch.setenv("GX_PR_BLOCK_NNZ", "131072")
    monkeypatch.setenv("GX_PR_VERBOSE", "1")
    csr = _k512_1024()
    # the property: every vertex of one side is joined to every vertex of the other
    deg = np.diff(csr.rowptr.astype(np.int64))
    assert (deg[:512] == 1024).all() and (deg[512:] == 512).all()
    capfd.readouterr()
    got = _pr(ctx, csr, False, 5)
    err = capfd.readouterr().err
    assert _run_stats(err) == (2 * 512 * 1024, 0, 24)
    assert _pair_stats(err) == (0, 0) and _narrow_entries(err) == 0
    np.testing.assert_allclose(got, O.pagerank(csr, False, 0.85, 5), rtol=PR_RTOL, atol=0)


@pytest.mark.gpu
def test_runs_off(ctx, monkeypatch, capfd):
    """GX_PR_RUNS=0: R = 0 everywhere, no run entries, and the pair slots hold what
    tests/test_pr_pairs.py asserts of the same graph."""
    monkeypatch.setenv("GX_PR_RUNS", "0")
    monkeypatch.setenv("GX_PR_SORTED_ROWS", "64")
    monkeypatch.setenv("GX_PR_BLOCK_NNZ", "131072")
    monkeypatch.setenv("GX_PR_VERBOSE", "1")
    csr = _k512_1024()
    capfd.readouterr()
    got = _pr(ctx, csr, False, 5)
    err = capfd.readouterr().err
    assert _run_stats(err) == (0, 0, 0)
    assert _pair_stats(err) == (2 * 512 * 1024, 0)
    np.testing.assert_allclose(got, O.pagerank(csr, False, 0.85, 5), rtol=PR_RTOL, atol=0)


def _pair_count_graph(counts_a, rows=128, nblk=2):
    """Directed: sources 0 .. C-1 (C = len(counts_a), a multiple of `rows`), all of out-degree
    nblk * rows, so the hub-first order is the identity.  Source c points at the first
    counts_a[c] rows of each of nblk `rows`-row blocks of set A and at the first
    rows - counts_a[c] rows of each block of set B.  Returns the graph and, per set, the entries
    each column pair holds in one block."""
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
    counts_a = np.asarray(counts_a, dtype=np.int64)
    C = len(counts_a)
    assert C % rows == 0 and C % 2 == 0 and (counts_a >= 0).all() and (counts_a <= rows).all()
    src, dst = [], []
    for c in range(C):
        for s, cnt in ((0, int(counts_a[c])), (1, rows - int(counts_a[c]))):
            for b in range(nblk):
                r = C + rows * (s * nblk + b) + np.arange(cnt, dtype=np.int64)
                src.append(np.full(cnt, c, dtype=np.int64))
                dst.append(r)
    n = C + 2 * rows * nblk + 6
    src, dst = np.concatenate(src), np.concatenate(dst)
    csr = csr_from_edges(n, src, dst, None, symmetric=False)
    # the property, from the edges: entries per (destination block, source pair)
    blk = (dst - C) // rows
    per = np.zeros((2 * nblk, C // 2), dtype=np.int64)
    np.add.at(per, (blk, src >> 1), 1)
    assert (per[:nblk] == per[0]).all() and (per[nblk:] == per[nblk]).all()
    return csr, per[0], per[nblk]


def _split(L, rows):
    """A pair's L entries as (even column, odd column) counts."""
    return min(L, rows), L - min(L, rows)


@pytest.mark.gpu
def test_runs_lengths_around_group(ctx, monkeypatch, capfd):
    """Column pairs holding 63, 64, 65, 127, 128 and 129 entries per block of set A (and
    256 - that in set B), 32 pairs of each: with padding free every entry is a run code, and
    the padding is each run's round-up to 64."""
    rows, nblk = 128, 2
    monkeypatch.setenv("GX_PR_SORTED_ROWS", str(rows))
    monkeypatch.setenv("GX_PR_RUN_FILL_COST", "0")
    monkeypatch.setenv("GX_PR_VERBOSE", "1")
    lens = [63, 64, 65, 127, 128, 129]
    counts = []
    for p in range(192):
        counts += _split(lens[p % 6], rows)
    csr, la, lb = _pair_count_graph(counts, rows, nblk)
    assert sorted(set(la.tolist())) == lens and sorted(set(lb.tolist())) == sorted(256 - v for v in lens)
    entries = nblk * int(la.sum() + lb.sum())
    padding = nblk * int(((-la) % 64).sum() + ((-lb) % 64).sum())
    assert entries == int(csr.rowptr[-1]) and padding == nblk * 32 * 256
    capfd.readouterr()
    got = _pr(ctx, csr, True, 6)
    assert _run_stats(capfd.readouterr().err) == (entries, padding, 2 * nblk)
    np.testing.assert_allclose(got, O.pagerank(csr, True, 0.85, 6), rtol=PR_RTOL, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["even_odd", "same_row"])
def test_runs_sel_bit(ctx, monkeypatch, capfd, case):
    """even_odd: set A's blocks hold 64 entries in every even column only (every sel 0), set B's
    in every odd column only (every sel 1).  same_row: a pair's two columns each hold rows 0..31
    of the block, so its one group names every one of its 32 LDS addresses twice."""
    rows, nblk = 64, 4
    monkeypatch.setenv("GX_PR_SORTED_ROWS", str(rows))
    monkeypatch.setenv("GX_PR_RUN_FILL_COST", "0")
    monkeypatch.setenv("GX_PR_VERBOSE", "1")
    if case == "even_odd":
        counts = [rows if c % 2 == 0 else 0 for c in range(512)]
        csr, la, lb = _pair_count_graph(counts, rows, nblk)
        assert (la == 64).all() and (lb == 64).all()
    else:
        counts = [32] * 512
        csr, la, lb = _pair_count_graph(counts, rows, nblk)
        assert (la == 64).all() and (lb == 64).all()
    capfd.readouterr()
    got = _pr(ctx, csr, True, 6)
    assert _run_stats(capfd.readouterr().err) == (2 * nblk * 256 * 64, 0, 2 * nblk)
    np.testing.assert_allclose(got, O.pagerank(csr, True, 0.85, 6), rtol=PR_RTOL, atol=0)


@pytest.mark.gpu
def test_runs_last_columns(ctx, monkeypatch, capfd):
    """Every vertex has out-degree 128, so the hub-first order is the identity; vertices 128 ..
    1023 all point at rows 0 .. 127: the first block's last run is the pair of columns 1022 and
    1023, the chunk's last real pair."""
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import csr_from_edges
    n = 1024
    monkeypatch.setenv("GX_PR_SORTED_ROWS", "128")
    monkeypatch.setenv("GX_PR_BLOCK_NNZ", "131072")
    monkeypatch.setenv("GX_PR_VERBOSE", "1")
    src = np.repeat(np.arange(n, dtype=np.int64), 128)
    dst = np.where(src >= 128, np.tile(np.arange(128, dtype=np.int64), n), np.tile(np.arange(128, 256, dtype=np.int64), n))
    csr = csr_from_edges(n, src, dst, None, symmetric=False)
    assert n % 2 == 0 and int(src[dst < 128].max()) == n - 1 and int((src[dst < 128] >> 1 == (n - 2) >> 1).sum()) == 256
    capfd.readouterr()
    got = _pr(ctx, csr, True, 6)
    assert _run_stats(capfd.readouterr().err) == (n * 128, 0, 2)
    np.testing.assert_allclose(got, O.pagerank(csr, True, 0.85, 6), rtol=PR_RTOL, atol=0)


# ---- an R-MAT graph with a block that has all four regions

RMAT_SPEC = (14, 16, 4)
RMAT_ROWS, RMAT_BLOCK, RMAT_W4 = 1024, 1 << 20, 8
RUN_MIN = 256   # the fixture's GX_PR_RUN_MIN
UNIT = 8192     # GX_PR_UNIT_NNZ of the unit cases: one round of the kernel
_RMAT = {}


def _rmat_case():
    """(csr, {iters: oracle scores}, per block (entries, R, Q, P, run codes)) from the model's functions."""
    if not _RMAT:
        from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat
        B, M = _model()
        csr = rmat(*RMAT_SPEC)
        blocks = []
        for _, col, row in B.block_entries(csr, RMAT_ROWS, RMAT_BLOCK):
            R = M.run_prefix(col, RMAT_W4) if len(col) >= RUN_MIN else 0
            Nr = min(len(col), R << 8)
            Q, P = B.splits(col[Nr:]) if Nr < len(col) else (0, 0)
            _, (_, pad, _) = M.run_codes(col, row, R, order=False)
            blocks.append((len(col), R, R + Q, R + P, Nr + pad))
        four = [b for b in blocks if 0 < b[1] < b[2] < b[3] < (b[0] + 255) >> 8]
        _RMAT.update(csr=csr, ref={}, blocks=blocks, four=four)
        # the plan's totals by the model: run entries, padding codes, blocks with a run prefix
        _RMAT["runs"] = (sum(min(b[0], 256 * b[1]) for b in blocks), sum(b[4] - min(b[0], 256 * b[1]) for b in blocks),
                         sum(b[1] > 0 for b in blocks))
        # cut into units of one round: a unit per round of the blocks with entries, one per empty block
        nblocks = -(-csr.n // RMAT_ROWS)
        per = [(b[0] + UNIT - 1) // UNIT for b in blocks]
        _RMAT["units"] = (nblocks, sum(per) + nblocks - len(blocks), sum(k > 1 for k in per))
    return _RMAT


def _rmat_ref(iters):
    c = _rmat_case()
    if iters not in c["ref"]:
        c["ref"][iters] = O.pagerank(c["csr"], False, 0.85, iters)
    return c["ref"][iters]


def _rmat_env(monkeypatch):
    monkeypatch.setenv("GX_PR_SORTED_ROWS", str(RMAT_ROWS))
    monkeypatch.setenv("GX_PR_BLOCK_NNZ", str(RMAT_BLOCK))
    monkeypatch.setenv("GX_PR_RUN_FILL_COST", str(RMAT_W4))


@pytest.mark.gpu
@pytest.mark.parametrize("bank", ["0", "1"])
def test_runs_four_regions(ctx, monkeypatch, capfd, bank):
    """Blocks with a run region, a pair prefix, narrow codes and wide entries, R < Q < P < their
    supergroups (found with the model's functions), with and without the bank order.  The plan's
    run entries, padding codes and blocks with a run prefix are the model's, so it chose the
    model's R in every block."""
    c = _rmat_case()
    assert c["four"], c["blocks"]
    E, R, Q, P, _ = c["four"][0]
    assert 0 < R < Q < P < (E + 255) >> 8
    _rmat_env(monkeypatch)
    monkeypatch.setenv("GX_PR_BANK_ORDER", bank)
    monkeypatch.setenv("GX_PR_VERBOSE", "1")
    capfd.readouterr()
    got = _pr(ctx, c["csr"], False, 10)
    err = capfd.readouterr().err
    assert _run_stats(err) == c["runs"]
    runs = c["runs"][0]
    pairs, _ = _pair_stats(err)
    narrow = _narrow_entries(err)
    assert pairs > 0 and narrow > 0 and runs + pairs + narrow < int(c["csr"].rowptr[-1])
    np.testing.assert_allclose(got, _rmat_ref(10), rtol=PR_RTOL, atol=0)


UNIT_MODES = [{"GX_PR_QUEUE": "0"}, {"GX_PR_QUEUE": "1"}, {"GX_PR_COMBINE": "1"}]


@pytest.mark.gpu
@pytest.mark.parametrize("env", UNIT_MODES, ids=lambda e: ",".join(f"{k[6:]}={v}" for k, v in e.items()))
def test_runs_units_every_unit_a_round(ctx, monkeypatch, capfd, env):
    """K(512, 1024) in 64-row blocks cut into units of one round: each of the 8 blocks of the
    larger side is 8 rounds of run codes dealt to 8 interleaved units, each of the 16 of the
    smaller side 4 rounds to 4 units: 128 units in 24 multi-unit blocks, every entry a run code."""
    monkeypatch.setenv("GX_PR_SORTED_ROWS", "64")
    monkeypatch.setenv("GX_PR_BLOCK_NNZ", "131072")
    monkeypatch.setenv("GX_PR_UNIT_NNZ", str(UNIT))
    monkeypatch.setenv("GX_PR_VERBOSE", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    csr = _k512_1024()
    capfd.readouterr()
    got = _pr(ctx, csr, False, 5)
    err = capfd.readouterr().err
    assert _plan_stats(err) == (24, 8 * (64 * 1024 // UNIT) + 16 * (64 * 512 // UNIT), 24)
    assert _run_stats(err) == (2 * 512 * 1024, 0, 24)   # 65 536 / 32 768 codes a block: 8 / 4 run rounds
    np.testing.assert_allclose(got, O.pagerank(csr, False, 0.85, 5), rtol=PR_RTOL, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("env", UNIT_MODES, ids=lambda e: ",".join(f"{k[6:]}={v}" for k, v in e.items()))
def test_runs_units_some_without_a_round(ctx, monkeypatch, capfd, env):
    """The R-MAT graph's four-region block cut into units of one round: it has more units than run
    rounds, so the later units start with the pair slots.  The plan's units, multi-unit blocks,
    run entries and padding codes are the model's, which pins both counts."""
    c = _rmat_case()
    E, R, _, _, codes = c["four"][0]
    units = (E + UNIT - 1) // UNIT   # one per round
    run_rounds = ((codes + 511) // 512 + 15) // 16
    assert 1 <= run_rounds < units and units >= 3, (run_rounds, units)
    _rmat_env(monkeypatch)
    monkeypatch.setenv("GX_PR_UNIT_NNZ", str(UNIT))
    monkeypatch.setenv("GX_PR_VERBOSE", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    got = _pr(ctx, c["csr"], False, 10)
    err = capfd.readouterr().err
    assert _plan_stats(err) == c["units"]
    assert _run_stats(err) == c["runs"]
    np.testing.assert_allclose(got, _rmat_ref(10), rtol=PR_RTOL, atol=0)


@pytest.mark.gpu
def test_runs_call_history(ctx, monkeypatch):
    """Iterations 0, 1 and 10, and two calls on one Graph."""
    from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A
    c = _rmat_case()
    _rmat_env(monkeypatch)
    G = A.Graph(ctx, c["csr"], False)
    try:
        for iters in (10, 0, 1, 10):
            np.testing.assert_allclose(A.LA_PR(G, 0.85, iters), _rmat_ref(iters), rtol=PR_RTOL, atol=0)
    finally:
        G.close()


@pytest.mark.gpu
def test_runs_partitioned(monkeypatch, capfd):
    """gx_pr_part_* with two ranks simulated on one device (as tests/test_pr_pairs.py builds
    them), run groups forced on: each piece's plan has a run region."""
    import torch
    from ldbc_graphalytics_platforms_graphblas_amd.algorithms import Context
    from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat
    from ldbc_graphalytics_platforms_graphblas_amd.pr_partition import GpuStep, hub_relabel, local_rows
    monkeypatch.setenv("GX_PR_VERBOSE", "1")
    nranks = 2
    csr = rmat(12, 16, 11)
    perm, hub = hub_relabel(csr)
    c = Context(0)
    dev = torch.device("cuda", 0)
    steps, lrs = [], []
    capfd.readouterr()
    for r in range(nranks):
        lr = local_rows(hub, directed=False, nranks=nranks, rank=r)
        lrs.append(lr)
        steps.append(GpuStep(c, csr.n, nranks, lr, 0.85))
    chunk = steps[0].chunk
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
    lines = re.findall(r"runs: (\d+) entries", capfd.readouterr().err)
    assert len(lines) == nranks and all(int(v) > 0 for v in lines), lines
    np.testing.assert_allclose(got, O.pagerank(csr, False, 0.85, iters), rtol=PR_RTOL)


# ---- CPU

def test_run_layout_check(tmp_path):
    """tests/native/run_layout_check.cpp under the address and undefined-behaviour sanitizers:
    gx_pr_runs.h on random run-length lists."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (the build needs one too)"
    exe = tmp_path / "run_layout_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
           str(ROOT / "tests" / "native" / "run_layout_check.cpp"), "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
    assert "ok" in res.stdout


def test_run_model_counts():
    """tools/pr_run_model.py on a hand-made graph: 300 rows of in-degree 4 from the same four
    sources.  Hub-first, the rows come first and the sources are columns 300 .. 303: one block of
    1200 entries in five supergroups, two runs of 600 (pairs 150 and 151), each padded by 40."""
    B, M = _model()
    rp = np.concatenate([np.zeros(5, dtype=np.int64), 4 * np.arange(1, 301, dtype=np.int64)])
    csr = SimpleNamespace(rowptr=rp, colidx=np.tile(np.arange(4), 300), n=304, nnz=1200)
    (nrows, col, row), = list(B.block_entries(csr))
    assert nrows == 304 and (np.bincount(col >> 1)[150:] == [600, 600]).all()
    # w = 2 entries per padding code: every supergroup pays; 1280 codes in 3 supergroups of
    # 1024 + 32 bytes, 3 instructions each; the pair slots before: 600 slots in 3 supergroups of
    # 1024 + 4 bytes, 6 instructions each
    d = M.block_counts(col, row, 8)
    assert (d["R"], d["run_entries"], d["run_pad"], d["run_sg"], d["bytes"], d["vmem"]) == (5, 1200, 80, 3, 3168, 9)
    d0 = M.block_counts(col, row, 8, runs=False)
    assert (d0["R"], d0["run_entries"], d0["bytes"], d0["vmem"]) == (0, 0, 3084, 18)
    # w = 25: the third supergroup (the first run's 40 padding codes) costs 1000 entries against
    # its 256 and the prefix stops before it: 512 codes of the cut run, no padding, then 344 slots
    d = M.block_counts(col, row, 100)
    assert (d["R"], d["run_entries"], d["run_pad"], d["run_sg"], d["bytes"], d["vmem"]) == (2, 512, 0, 1, 1056 + 2 * 1028, 15)
    # groups of 32: 600 = 18 groups + 24, 8 padding codes per run
    d = M.block_counts(col, row, 8, group=32)
    assert (d["R"], d["run_pad"], d["run_sg"], d["bytes"]) == (5, 16, 3, 3 * (1024 + 64))
