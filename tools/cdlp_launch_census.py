#!/usr/bin/env python3
"""Launch census of gx_cdlp: for four small graphs and 1, 3, 7 and 12 iterations, two
consecutive calls on a fresh graph (the relabelled copy arrives with the second), and per call
the launch count of every cdlp_* timer bench.py lists.  The sparse-only decision reads only
flags the host has already waited for, so the output is deterministic: two trees that launch
the same kernels print the same text.  Usage: python tools/cdlp_launch_census.py > census.txt
"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

from bench import KERNELS  # noqa: E402
from ldbc_graphalytics_platforms_graphblas_amd import algorithms as A  # noqa: E402
from ldbc_graphalytics_platforms_graphblas_amd.graphio import rmat  # noqa: E402
from test_gpu_parity import _tier_graph  # noqa: E402


def main():
    graphs = [("tier undirected", _tier_graph(False), False),
              ("tier directed", _tier_graph(True), True),
              ("rmat 12x4 undirected", rmat(12, 4, 7), False),
              ("rmat 11 directed", rmat(11, 6, 3, undirected=False), True)]
    ctx = A.Context(0)
    ctx.set_kernel_timing(True)
    try:
        for name, csr, directed in graphs:
            for iters in (1, 3, 7, 12):
                G = A.Graph(ctx, csr, directed=directed)
                try:
                    for call in (1, 2):
                        ctx.reset_kernel_stats()
                        A.LA_CDLP(G, iters)
                        counts = " ".join(f"{k[5:]}={ctx.kernel_stats(k)[0]}" for k in KERNELS["cdlp"])
                        print(f"{name}, {iters} iterations, call {call}: {counts}")
                finally:
                    G.close()
    finally:
        ctx.set_kernel_timing(False)
        ctx.close()


if __name__ == "__main__":
    main()
