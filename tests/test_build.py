"""Build-level guards (CPU, no GPU): the PageRank hot kernel must not spill registers.

k_pr_pull_units runs 16 waves per CU (launch bounds 1024 threads, 4 waves per SIMD), so it has
128 VGPRs; an edit that pushed it past them (round 3: 34 VGPRs spilled to scratch) made the
launch 2x slower without failing any parity test.  This compiles gx_pr_sorted.hip with the
compiler's resource report and checks the product instantiation."""
import re
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"


def resource_report(src):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT}/include",
           f"-I{ROOT}/ldbc_graphalytics_platforms_graphblas_amd/csrc", "-c", str(src), "-o", "/dev/null",
           "-Rpass-analysis=kernel-resource-usage"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    kernels, cur = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", line)
        if m and cur:
            kernels[cur][m.group(1).strip()] = int(m.group(2))
    return kernels


def test_pagerank_kernel_does_not_spill():
    import shutil
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    ks = resource_report(ROOT / "ldbc_graphalytics_platforms_graphblas_amd" / "csrc" / "gx_pr_sorted.hip")
    prod = [k for k in ks if "k_pr_pull_unitsILb0ELi" in k]   # every TIMES = false instantiation
    assert prod, sorted(ks)
    for k in prod:
        assert ks[k].get("VGPRs Spill", 0) == 0 and ks[k].get("ScratchSize", 0) == 0, (k, ks[k])
        assert ks[k].get("VGPRs", 0) <= 128, (k, ks[k])


def device_asm(src):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT}/include",
           f"-I{ROOT}/ldbc_graphalytics_platforms_graphblas_amd/csrc", "--offload-device-only", "-S", str(src),
           "-o", "-"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    return res.stdout


def test_queue_fetch_exit_is_uniform():
    """the work-queue kernel's loop exit after queue_fetch must be a scalar
    branch on SCC, set by a scalar compare of the readfirstlane'd item, and neither barrier that
    publishes the item may sit inside an exec-masked region.  The two hangs of rounds 4-5
    (gpurun_out/m1/variants.log) were exactly a divergent exit here, so this guards the emitted
    ISA on the CPU instead of on a GPU box."""
    import shutil
    import sys
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    sys.path.insert(0, str(ROOT / "tools"))
    import isa_exec_check as X
    asm = device_asm(ROOT / "ldbc_graphalytics_platforms_graphblas_amd" / "csrc" / "gx_pr_sorted.hip")
    syms = sorted(set(re.findall(r"^(_Z\w+k_pr_pull_unitsILb0ELi\d+ELb1E\w*):", asm, re.M)))
    assert syms, "no QUEUE=true instantiation of k_pr_pull_units in the device assembly"
    for sym in syms:
        ins, labels = X.parse(X.kernel_body(asm, sym))
        r = X.queue_fetch_region(ins, labels)
        assert r is not None, sym
        exit_op = ins[r["exit"]].split()[0]
        assert exit_op in ("s_cbranch_scc0", "s_cbranch_scc1"), (sym, ins[r["exit"]])
        assert r["cond"] is not None and ins[r["cond"]].startswith("s_cmp"), (sym, r["cond"] and ins[r["cond"]])
        # the compared item is a scalar read back from LDS through readfirstlane
        between = ins[r["barriers"][-1]:r["cond"]]
        assert any(t.startswith("v_readfirstlane_b32") for t in between), (sym, between)
        depth = X.exec_depth(ins, r["header"], r["exit"] + 1)
        for b in r["barriers"][:2]:
            assert depth[b - r["header"]] == 0, (sym, b, ins[r["header"]:b + 1])
        assert depth[r["exit"] - r["header"]] == 0, (sym, "exit branch inside a masked region")
