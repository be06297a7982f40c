#!/usr/bin/env python3
"""K1 answered from the members' score tables (cnn_score_table = 1: one table read per row and member, the mean in the same kernel) against
the head-only kernel on the pooled-feature tables (0 = the parent's behaviour).

    score_table_ab.py                      back-to-back kernel time (fx_debug_time_score, what bench.py --full reports as kernel_ms_b2b), the two
                                           values of the option interleaved in one process, bits compared; then what the table costs where weights change
    score_table_ab.py --weights-only       just that second part; also runs on a library without the option: the parent's arm
    score_table_ab.py --bench PARENT LIB0  `python bench.py --gpus 1 --steps 1000 --warmup 100`, three arms alternated five times: PARENT = a checkout of
                                           the parent commit with its library built, LIB0 = this library built with -DFX_SCORE_TABLE_DEFAULT=0, and this
                                           library as it ships; then bench.py --dump-outputs for parent and child, np.array_equal on mean.npy
-> profiles/score_table_ab.log"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench_arms(parent_root, lib0, reps=5):
    arms = [("parent", parent_root, None), ("score 0", ROOT, lib0), ("score 1", ROOT, None)]
    runs = {name: [] for name, _, _ in arms}

    def bench(root, lib, extra=()):
        env = dict(os.environ)
        env.pop("FLEXS_AMD_LIB", None)
        if lib:
            env["FLEXS_AMD_LIB"] = os.path.abspath(lib)
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "1000", "--warmup", "100", *extra], cwd=root, env=env,
                           capture_output=True, text=True, timeout=240)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            raise SystemExit(f"bench.py failed in {root} (exit {r.returncode})")
        out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        full = [ln for ln in r.stderr.splitlines() if ln.startswith("{")]      # (the full record: host_issue_ms_per_step lives there)
        if full:
            out.setdefault("host_issue_ms_per_step", json.loads(full[-1]).get("host_issue_ms_per_step"))
        return out

    for rep in range(reps):
        for k in range(len(arms)):
            name, root, lib = arms[(k + rep) % len(arms)]
            runs[name].append(bench(root, lib))
            last = runs[name][-1]
            print(f"   rep {rep} {name}: value {last['value']:.4e}  ms_per_step {last['ms_per_step']:.6g}  host_issue_ms_per_step {last['host_issue_ms_per_step']:.6g}", flush=True)
    med, spread = {}, {}
    for name, _, _ in arms:
        v = [r["value"] for r in runs[name]]
        med[name], spread[name] = float(np.median(v)), max(v) - min(v)
        ms = [r["ms_per_step"] for r in runs[name]]
        issue = [r["host_issue_ms_per_step"] for r in runs[name]]
        print(f"{name:8s} value median {med[name]:.4e} seq/s  spread (max - min) {spread[name]:.3e} ({spread[name] / med[name] * 100:.2f} %)  "
              f"ms_per_step median {np.median(ms):.6g}  host_issue_ms_per_step median {np.median(issue):.6g}")
        print(f"         value runs {[f'{x:.4e}' for x in v]}")
        print(f"         ms_per_step runs {[round(x, 5) for x in ms]}  host_issue_ms_per_step runs {[round(x, 5) for x in issue]}", flush=True)
    for name in ("score 0", "score 1"):
        d = med[name] - med["parent"]
        verdict = "inside the parent's spread" if abs(d) <= spread["parent"] else (
            "a gain by the issue's rule" if d > 3 * spread["parent"] else "outside the parent's spread, not a gain by the issue's rule")
        print(f"{name} vs parent: {d:+.4e} seq/s = {d / med['parent'] * 100:+.2f} %; the parent's spread {spread['parent']:.3e}, three times that "
              f"{3 * spread['parent']:.3e}: {verdict}")
    one = runs["score 1"]
    step, issue = float(np.median([r["ms_per_step"] for r in one])), float(np.median([r["host_issue_ms_per_step"] for r in one]))
    print(f"score 1: step {step * 1e3:.2f} us, host issue {issue * 1e3:.2f} us = {issue / step * 100:.1f} % of the step"
          + ("  -> the step is HOST-BOUND: bounded by how fast launch / finish are issued, not by the GPU" if issue >= 0.9 * step else ""), flush=True)
    # identical outputs
    with tempfile.TemporaryDirectory() as tmp:
        dirs = {}
        for name, root, lib in arms:
            dirs[name] = os.path.join(tmp, name.replace(" ", "_"))
            bench(root, lib, ("--dump-outputs", dirs[name]))
        want = np.load(os.path.join(dirs["parent"], "mean.npy"))
        for name in ("score 0", "score 1"):
            got = np.load(os.path.join(dirs[name], "mean.npy"))
            print(f"bench.py --dump-outputs: np.array_equal(mean.npy of {name}, the parent's) = {np.array_equal(got, want)}  "
                  f"(uint32 views: {np.array_equal(got.view(np.uint32), want.view(np.uint32))}; {got.shape[0]} floats)", flush=True)


if "--bench" in sys.argv:
    at = sys.argv.index("--bench")
    bench_arms(os.path.abspath(sys.argv[at + 1]), sys.argv[at + 2], int(sys.argv[at + 3]) if len(sys.argv) > at + 3 else 5)
    raise SystemExit(0)

sys.path.insert(0, ROOT)
import torch  # noqa: E402

import flexs_amd  # noqa: E402
from flexs_amd import _native, synth  # noqa: E402
from flexs_amd.baselines.models import CNN  # noqa: E402
from tools.bench_common import build_members, time_launches  # noqa: E402

eng = _native.Engine.get(0)
WEIGHTS_ONLY = "--weights-only" in sys.argv
try:
    shipped = eng.get_option("cnn_score_table")
    ARMS = (0, 1)
except Exception:  # noqa: BLE001  (the parent's library: one arm, no option)
    shipped, ARMS = None, (None,)
REPS = 6
L, ALPHA = 8, "TGCA"


def set_score(q):
    if q is not None:
        eng.set_option("cnn_score_table", q)


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
            set_score(q)
            ms, _ = time_launches(eng, mods, d_in.data_ptr(), n, L, mods[0]._lut, planes[q], stride, min_ms=40.0)
            res[q].append(ms * 1e3)
    torch.cuda.synchronize()
    same = bool(torch.equal(planes[0][:, :n].view(torch.int32), planes[1][:, :n].view(torch.int32)))
    med = {q: float(np.median(res[q])) for q in ARMS}
    print(f"{name:34s} " + "  ".join(f"score {q} {med[q]:8.2f} us (spread {max(res[q]) - min(res[q]):.2f})" for q in ARMS) +
          f"  score 1 {(med[1] / med[0] - 1) * 100:+.2f} %  same bits {same}", flush=True)
    print("   runs " + " / ".join(str([round(x, 2) for x in res[q]]) for q in ARMS), flush=True)
if shipped is not None and not WEIGHTS_ONLY:
    set_score(shipped)
    print("table launches counted:", eng.get_option("pool_table_launches"), " of them lookups:", eng.get_option("score_table_launches"),
          " pooled tables built:", eng.get_option("pool_table_builds"), " score tables built:", eng.get_option("score_table_builds"), " shipped option:", shipped)


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


# ---- where weights change.  fx_model_set_weights per member: nothing of either table is built there
mods = build_members("cnn", L, ALPHA, 3, 0)
nats = [m.native() for m in mods]
ws = [m.model.get_weights() for m in mods]
report("fx_model_set_weights, CNN L=8 member, conv tables built and awaited", timed(lambda: nats[0].set_weights(ws[0]), 200))

# ... the builders' own duration: a 16-row launch behind set_weights with the tables built for it (cnn_pool_table = 2) against the same call without
d16 = torch.from_numpy(synth.random_sequence_bytes(16, L, ALPHA, 1)).cuda()
o16 = torch.zeros((16, 1), dtype=torch.float32, device="cuda")


def small_after_weights(pool, q):
    def fn():
        nats[0].set_weights(ws[0])
        eng.set_option("cnn_pool_table", pool)
        set_score(q)
        eng.score_dev([nats[0]], d16.data_ptr(), 16, L, mods[0]._lut, o16.data_ptr(), None)
        eng.sync()
    return fn


pool_shipped = eng.get_option("cnn_pool_table")
eng.set_option("cnn_big_units", 0)
eng.set_option("cnn_quad", 0)
a = timed(small_after_weights(0, None), 50)
b = {q: timed(small_after_weights(2, q), 50) for q in ARMS}
eng.set_option("cnn_big_units", 12)
eng.set_option("cnn_quad", 1)
eng.set_option("cnn_pool_table", pool_shipped)
set_score(shipped)
report("set_weights + 16-row launch, conv form (16-wave form forced)", a)
for q in ARMS:
    report(f"set_weights + 16-row launch, tables built first (cnn_pool_table 2), score {q}", b[q])
if shipped is not None:
    print(f"   score-table builder: {np.median(b[1]) - np.median(b[0]):.1f} us per member by difference (builder kernel + lookup instead of the head-only launch)")

# ... the first 1e5-row call after new weights for all three members, and the second one
n = 100_000
d_in = torch.from_numpy(synth.random_sequence_bytes(n, L, ALPHA, 0)).cuda()
stride = (n + 63) // 64 * 64
planes = torch.zeros((3, stride), dtype=torch.float32, device="cuda")


def big_call():
    eng.score_planes_dev(nats, d_in.data_ptr(), n, L, mods[0]._lut, planes.data_ptr(), stride)
    eng.sync()


def first_big_call(q):
    def fn():
        for nat, w in zip(nats, ws):
            nat.set_weights(w)
        set_score(q)
        big_call()
    return fn


for q in ARMS:
    report(f"3 x set_weights + first 3 x 1e5 call, score {q}", timed(first_big_call(q), 20))
    report(f"   the second 3 x 1e5 call (tables fresh), one call + sync, score {q}", timed(big_call, 20))
set_score(shipped)

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
before = (eng.get_option("pool_table_builds"), eng.get_option("score_table_builds") if shipped is not None else 0)


def explorer_step():
    mods[0].model.set_weights(ws[0])
    ens.get_fitness(few)


report("set_weights of one member + get_fitness(20 sequences)", timed(explorer_step, 100))
print("   tables built by that loop: pooled", eng.get_option("pool_table_builds") - before[0],
      " score", (eng.get_option("score_table_builds") if shipped is not None else 0) - before[1])
