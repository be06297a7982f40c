#!/usr/bin/env python3
"""K1 with conv1 from the table (cnn_conv1_table = 1) against the gather (0), interleaved in one process: back-to-back kernel time
(fx_debug_time_score, what bench.py --full reports as kernel_ms_b2b), bits compared.  -> profiles/conv1_table_ab.log"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flexs_amd import _native, synth  # noqa: E402
from tools.bench_common import build_members, time_launches  # noqa: E402

eng = _native.Engine.get(0)
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
CASES = [("3xCNN L=8 N=1e5 (headline)", 3, 100_000), ("1xCNN L=8 N=1e5", 1, 100_000), ("3xCNN L=8 N=1e6", 3, 1_000_000), ("8xCNN L=8 N=1e5", 8, 100_000)]
for name, M, n in CASES:
    L, alpha = 8, "TGCA"
    mods = build_members("cnn", L, alpha, M, 0)
    d_in = torch.from_numpy(synth.random_sequence_bytes(n, L, alpha, 0)).cuda()
    stride = (n + 63) // 64 * 64
    planes = {q: torch.zeros((M, stride), dtype=torch.float32, device="cuda") for q in (0, 1)}
    res = {0: [], 1: []}
    for rep in range(REPS):
        for q in ((0, 1) if rep % 2 == 0 else (1, 0)):
            eng.set_option("cnn_conv1_table", q)
            ms, _ = time_launches(eng, mods, d_in.data_ptr(), n, L, mods[0]._lut, planes[q], stride, min_ms=40.0)
            res[q].append(ms * 1e3)
    torch.cuda.synchronize()
    same = bool(torch.equal(planes[0][:, :n].view(torch.int32), planes[1][:, :n].view(torch.int32)))
    a, b = float(np.median(res[0])), float(np.median(res[1]))
    print(f"{name:30s} gather {a:8.2f} us (spread {max(res[0]) - min(res[0]):.2f})  table {b:8.2f} us (spread {max(res[1]) - min(res[1]):.2f})  "
          f"({(b / a - 1) * 100:+.2f} %)  same bits {same}   runs {[round(x, 2) for x in res[0]]} / {[round(x, 2) for x in res[1]]}", flush=True)
eng.set_option("cnn_conv1_table", 1)
print("table launches counted:", eng.get_option("conv1_table_launches"))
