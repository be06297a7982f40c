#!/usr/bin/env python3
"""K1 answered from the members' pooled-feature tables (cnn_pool_table = 1) against the conv2-prefix form (0), interleaved in one process:
back-to-back kernel time (fx_debug_time_score, what bench.py --full reports as kernel_ms_b2b), bits compared against option 0; then what the
table costs where weights change (fx_model_set_weights per member, the builder, the first large call after new weights, Ensemble.train, an
explorer-size loop).  `--weights-only` runs just that part and also runs on a library without the option: the parent's arm.
-> profiles/pool_table_ab.log"""
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
try:
    shipped = eng.get_option("cnn_pool_table")
    ARMS = (0, 1)
except Exception:  # noqa: BLE001  (the parent's library: one arm, no option)
    shipped, ARMS = None, (None,)
REPS = 6
L, ALPHA = 8, "TGCA"


def set_pool(q):
    if q is not None:
        eng.set_option("cnn_pool_table", q)


CASES = [("3xCNN L=8 N=1e5 (headline)", 3, 100_000), ("1xCNN L=8 N=1e5", 1, 100_000), ("3xCNN L=8 N=1e6", 3, 1_000_000), ("8xCNN L=8 N=1e5", 8, 100_000),
         ("3xCNN L=8 N=98304 (no remainder)", 3, 98_304)]
for name, M, n in ([] if WEIGHTS_ONLY or shipped is None else CASES):
    mods = build_members("cnn", L, ALPHA, M, 0)
    d_in = torch.from_numpy(synth.random_sequence_bytes(n, L, ALPHA, 0)).cuda()
    stride = (n + 63) // 64 * 64
    planes = {q: torch.zeros((M, stride), dtype=torch.float32, device="cuda") for q in ARMS}
    res = {q: [] for q in ARMS}
    for rep in range(REPS):
        for k in range(len(ARMS)):
            q = ARMS[(k + rep) % len(ARMS)]
            set_pool(q)
            ms, _ = time_launches(eng, mods, d_in.data_ptr(), n, L, mods[0]._lut, planes[q], stride, min_ms=40.0)
            res[q].append(ms * 1e3)
    torch.cuda.synchronize()
    same = bool(torch.equal(planes[0][:, :n].view(torch.int32), planes[1][:, :n].view(torch.int32)))
    med = {q: float(np.median(res[q])) for q in ARMS}
    print(f"{name:34s} " + "  ".join(f"pool {q} {med[q]:8.2f} us (spread {max(res[q]) - min(res[q]):.2f})" for q in ARMS) +
          f"  pool 1 {(med[1] / med[0] - 1) * 100:+.2f} %  same bits {same}", flush=True)
    print("   runs " + " / ".join(str([round(x, 2) for x in res[q]]) for q in ARMS), flush=True)
if shipped is not None and not WEIGHTS_ONLY:
    set_pool(shipped)
    print("table launches counted:", eng.get_option("pool_table_launches"), " tables built:", eng.get_option("pool_table_builds"), " shipped option:", shipped)


def timed(fn, loops, runs=7, warm=3):
    for _ in range(warm):
        fn()
    eng.sync()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        for _ in range(loops):
            fn()
        eng.sync()
        out.append((time.perf_counter() - t0) / loops * 1e6)
    return out


def report(what, runs, unit="us"):
    print(f"{what}: median {np.median(runs):.1f} {unit} (spread {max(runs) - min(runs):.1f})   runs {[round(x, 1) for x in runs]}", flush=True)


# ---- where weights change.  fx_model_set_weights per member: nothing of the table is built there
mods = build_members("cnn", L, ALPHA, 3, 0)
nats = [m.native() for m in mods]
ws = [m.model.get_weights() for m in mods]
report("fx_model_set_weights, CNN L=8 member, conv tables built and awaited", timed(lambda: nats[0].set_weights(ws[0]), 200))

# ... the builder's own duration: a 16-row launch behind set_weights with the table built for it (option 2) against the same call without (0)
d16 = torch.from_numpy(synth.random_sequence_bytes(16, L, ALPHA, 1)).cuda()
o16 = torch.zeros((16, 1), dtype=torch.float32, device="cuda")


def small_after_weights(q):
    def fn():
        nats[0].set_weights(ws[0])
        set_pool(q)
        eng.score_dev([nats[0]], d16.data_ptr(), 16, L, mods[0]._lut, o16.data_ptr(), None)
        eng.sync()
    return fn


if shipped is not None:
    eng.set_option("cnn_big_units", 0)
    eng.set_option("cnn_quad", 0)
    a = timed(small_after_weights(0), 50)
    b = timed(small_after_weights(2), 50)
    eng.set_option("cnn_big_units", 12)
    eng.set_option("cnn_quad", 1)
    report("set_weights + 16-row launch, conv form (16-wave form forced)", a)
    report("set_weights + 16-row launch, table built first (option 2)", b)
    print(f"   builder: {np.median(b) - np.median(a):.1f} us per member by difference (kernel + the first call's allocation amortised away)")

# ... the first 1e5-row call after new weights for all three members
n = 100_000
d_in = torch.from_numpy(synth.random_sequence_bytes(n, L, ALPHA, 0)).cuda()
stride = (n + 63) // 64 * 64
planes = torch.zeros((3, stride), dtype=torch.float32, device="cuda")


def first_big_call(q):
    def fn():
        for nat, w in zip(nats, ws):
            nat.set_weights(w)
        set_pool(q)
        eng.score_planes_dev(nats, d_in.data_ptr(), n, L, mods[0]._lut, planes.data_ptr(), stride)
        eng.sync()
    return fn


for q in ARMS:
    report(f"3 x set_weights + first 3 x 1e5 call, pool {q}", timed(first_big_call(q), 20))
set_pool(shipped)

# ... Ensemble.train of the headline ensemble on 1000 labelled rows
rng = np.random.default_rng(0)
seqs = ["".join(ALPHA[i] for i in row) for row in rng.integers(0, 4, (1000, 8))]
labels = rng.normal(size=1000).astype(np.float32)
runs = []
for rep in range(6):
    ens = flexs_amd.Ensemble([CNN(8, 32, 100, ALPHA, seed=10 + m) for m in range(3)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ens.train(seqs, labels)
    torch.cuda.synchronize()
    eng.sync()
    runs.append((time.perf_counter() - t0) * 1e3)
print(f"Ensemble.train, 3 x CNN L=8, n=1000: median {np.median(runs[1:]):.1f} ms (spread {max(runs[1:]) - min(runs[1:]):.1f}, first call {runs[0]:.1f})   runs {[round(x, 1) for x in runs]}")

# ... an explorer-size loop: get_fitness of 20 sequences after every set_weights (the small forms never build)
ens = flexs_amd.Ensemble(mods)
few = seqs[:20]
before = eng.get_option("pool_table_builds") if shipped is not None else 0


def explorer_step():
    mods[0].model.set_weights(ws[0])
    ens.get_fitness(few)


report("set_weights of one member + get_fitness(20 sequences)", timed(explorer_step, 100))
if shipped is not None:
    print("   tables built by that loop:", eng.get_option("pool_table_builds") - before)
