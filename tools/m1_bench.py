#!/usr/bin/env python3
"""M1 (similarity + arg-max) on the shapes of the three BASELINE workloads (612 pairs of 500 x 500 x 128, ...): time and
TFLOP/s of both matcher forms (test-only knob SSLAM_M1_VARIANT).  python tools/m1_bench.py"""
import os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-slam-master_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from sslam_amd import lib
if os.environ.get("SSLAM_BENCH_SO"):            # a variant build of the library (experiments)
    lib.LIBRARIES["lib"].so_path = os.path.abspath(os.environ["SSLAM_BENCH_SO"])

for K, pairs in ((500, 612), (1024, 511), (2048, 127)):
    d = torch.nn.functional.normalize(torch.randn(pairs + 1, K, 128, device="cuda"), dim=-1)
    ws = torch.empty(lib.workspace_bytes(1, 28, K, pairs), dtype=torch.uint8, device="cuda")
    row = []
    for tiles in (2, 1):
        with lib.knobs(SSLAM_M1_VARIANT=tiles):
            for _ in range(3):
                lib.sim_argmax(d[:-1], K * 128, K, d[1:], K * 128, K, pairs, workspace=ws)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                lib.sim_argmax(d[:-1], K * 128, K, d[1:], K * 128, K, pairs, workspace=ws)
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / 20
        row.append(f"variant {tiles} ({'S once + key reduction' if tiles == 2 else 'S per direction'}): {ms:6.3f} ms ({pairs * K * K * 128 * 2 / ms / 1e9:5.1f} TF)")
    print(f"K {K:4d}, {pairs} pairs: " + "   ".join(row), flush=True)
