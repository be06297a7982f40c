#!/usr/bin/env python3
"""K1 with conv2's first taps read from the member's prefix tables (cnn_conv2_prefix = 1, 2) against all taps (0), interleaved in one
process: back-to-back kernel time (fx_debug_time_score, what bench.py --full reports as kernel_ms_b2b), bits compared against depth 0;
then what the tables cost where weights change (fx_model_set_weights per member, Ensemble.train; `--weights-only` runs just this part, which
also runs on a library without the option: the parent's arm).  -> profiles/conv2_prefix_ab.log"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import flexs_amd  # noqa: E402
from flexs_amd import _native, synth  # noqa: E402
from flexs_amd.baselines.models import CNN  # noqa: E402
from tools.bench_common import build_members, time_launches  # noqa: E402

eng = _native.Engine.get(0)
WEIGHTS_ONLY = "--weights-only" in sys.argv
REPS = 6
DEPTHS = (0, 1, 2)
shipped = 0 if WEIGHTS_ONLY else eng.get_option("cnn_conv2_prefix")
CASES = [("3xCNN L=8 N=1e5 (headline)", 3, 100_000), ("1xCNN L=8 N=1e5", 1, 100_000), ("3xCNN L=8 N=1e6", 3, 1_000_000), ("8xCNN L=8 N=1e5", 8, 100_000),
         ("3xCNN L=8 N=98304 (no remainder)", 3, 98_304)]
for name, M, n in ([] if WEIGHTS_ONLY else CASES):
    L, alpha = 8, "TGCA"
    mods = build_members("cnn", L, alpha, M, 0)
    d_in = torch.from_numpy(synth.random_sequence_bytes(n, L, alpha, 0)).cuda()
    stride = (n + 63) // 64 * 64
    planes = {q: torch.zeros((M, stride), dtype=torch.float32, device="cuda") for q in DEPTHS}
    res = {q: [] for q in DEPTHS}
    for rep in range(REPS):
        for k in range(len(DEPTHS)):
            q = DEPTHS[(k + rep) % len(DEPTHS)]
            eng.set_option("cnn_conv2_prefix", q)
            ms, _ = time_launches(eng, mods, d_in.data_ptr(), n, L, mods[0]._lut, planes[q], stride, min_ms=40.0)
            res[q].append(ms * 1e3)
    torch.cuda.synchronize()
    same = [bool(torch.equal(planes[0][:, :n].view(torch.int32), planes[q][:, :n].view(torch.int32))) for q in DEPTHS[1:]]
    med = {q: float(np.median(res[q])) for q in DEPTHS}
    print(f"{name:34s} " + "  ".join(f"depth {q} {med[q]:8.2f} us (spread {max(res[q]) - min(res[q]):.2f})" for q in DEPTHS) +
          f"  depth 1 {(med[1] / med[0] - 1) * 100:+.2f} %  depth 2 {(med[2] / med[0] - 1) * 100:+.2f} %  same bits {same}", flush=True)
    print("   runs " + " / ".join(str([round(x, 2) for x in res[q]]) for q in DEPTHS), flush=True)
if not WEIGHTS_ONLY:
    eng.set_option("cnn_conv2_prefix", shipped)
    print("prefix launches counted:", eng.get_option("conv2_prefix_launches"), " shipped depth:", shipped)

# ---- where weights change: fx_model_set_weights (the host packer, two copies, the conv1 table kernel and the prefix kernel) per member ...
mods = build_members("cnn", 8, "TGCA", 1, 0)
nat = mods[0].native()
w = mods[0].model.get_weights()
for _ in range(20):
    nat.set_weights(w)
eng.sync()
runs = []
for _ in range(7):
    t0 = time.perf_counter()
    for _ in range(200):
        nat.set_weights(w)
    eng.sync()
    runs.append((time.perf_counter() - t0) / 200 * 1e6)
print(f"fx_model_set_weights, CNN L=8 member, tables built and awaited: median {np.median(runs):.1f} us per call (spread {max(runs) - min(runs):.1f})   runs {[round(x, 1) for x in runs]}")
# ... and Ensemble.train of the headline ensemble on 1000 labelled rows
rng = np.random.default_rng(0)
seqs = ["".join("TGCA"[i] for i in row) for row in rng.integers(0, 4, (1000, 8))]
labels = rng.normal(size=1000).astype(np.float32)
runs = []
for rep in range(6):
    ens = flexs_amd.Ensemble([CNN(8, 32, 100, "TGCA", seed=10 + m) for m in range(3)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ens.train(seqs, labels)
    torch.cuda.synchronize()
    eng.sync()
    runs.append((time.perf_counter() - t0) * 1e3)
print(f"Ensemble.train, 3 x CNN L=8, n=1000: median {np.median(runs[1:]):.1f} ms (spread {max(runs[1:]) - min(runs[1:]):.1f}, first call {runs[0]:.1f})   runs {[round(x, 1) for x in runs]}")
