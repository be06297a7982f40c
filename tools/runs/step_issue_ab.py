#!/usr/bin/env python3
"""The headline step issued through a prepared step (engine option step_call = 1: `fx_step_launch`, one short native call per resident step)
against the direct calls (0 = the parent's issue path), and against the parent commit itself.

    step_issue_ab.py PARENT LIB0 [REPS] [--full | --full-only]

`python bench.py --gpus 1 --steps 1000 --warmup 100`, a fresh process per run, three arms in rotated order, REPS (default 8, at least 8) runs
per arm: PARENT = a checkout of the parent commit with its library built, LIB0 = this library built with -DFX_STEP_CALL_DEFAULT=0 on
fx_engine.hip (FLEXS_AMD_LIB selects it), and this library as it ships.  Per arm the median, min and max of `value`, `ms_per_step` and
`host_issue_ms_per_step`; a gain is a median `value` more than three of the parent's own max - min spreads above the parent's median.  Then
bench.py --dump-outputs for every arm, np.array_equal on mean.npy.  --full: one `bench.py --full --no-cpu-baseline --no-live-pmc` per arm, the
figures that pass through DistributedEnsemble / get_fitness side by side (kernel_ms, kernel_ms_b2b, e2e_value, small_call_n*_us, the
member-parallel block); --full-only: just that part.
-> profiles/step_issue_ab.log (stdout)"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if len(args) < 2:
    raise SystemExit(__doc__)
PARENT, LIB0 = os.path.abspath(args[0]), os.path.abspath(args[1])
REPS = max(int(args[2]) if len(args) > 2 else 8, 8)
ARMS = [("parent", PARENT, None), ("step 0", ROOT, LIB0), ("step 1", ROOT, None)]
FIGURES = ("value", "ms_per_step", "host_issue_ms_per_step")


def bench(root, lib, extra=(), timeout=300):
    env = dict(os.environ)
    env.pop("FLEXS_AMD_LIB", None)
    if lib:
        env["FLEXS_AMD_LIB"] = lib
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "1000", "--warmup", "100", *extra], cwd=root, env=env,
                       capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        raise SystemExit(f"bench.py failed in {root} (exit {r.returncode})")
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    full = [ln for ln in r.stderr.splitlines() if ln.startswith("{")]      # (the full record: host_issue_ms_per_step lives there)
    record = json.loads(full[-1]) if full else {}
    out.setdefault("host_issue_ms_per_step", record.get("host_issue_ms_per_step"))
    return out, record


def headline_arms():
    print(f"== (1) bench.py --gpus 1 --steps 1000 --warmup 100, a fresh process per run, {REPS} runs per arm in rotated order (tools/runs/step_issue_ab.py)")
    runs = {name: [] for name, _, _ in ARMS}
    for rep in range(REPS):
        for k in range(len(ARMS)):
            name, root, lib = ARMS[(k + rep) % len(ARMS)]
            last, _ = bench(root, lib)
            runs[name].append(last)
            print(f"   rep {rep} {name:7s} value {last['value']:.4e}  ms_per_step {last['ms_per_step']:.6g}  host_issue_ms_per_step {last['host_issue_ms_per_step']:.6g}", flush=True)
    stat = {}
    for name, _, _ in ARMS:
        for fig in FIGURES:
            v = [r[fig] for r in runs[name]]
            stat[name, fig] = (float(np.median(v)), min(v), max(v))
        med, lo, hi = stat[name, "value"]
        print(f"{name:7s} value median {med:.4e} min {lo:.4e} max {hi:.4e} seq/s (spread {hi - lo:.3e} = {(hi - lo) / med * 100:.2f} %)")
        for fig in FIGURES[1:]:
            med, lo, hi = stat[name, fig]
            print(f"        {fig} median {med * 1e3:.3f} us  min {lo * 1e3:.3f}  max {hi * 1e3:.3f}")
        print("        value runs " + " ".join(f"{r['value']:.4e}" for r in runs[name]), flush=True)
    p_med, p_lo, p_hi = stat["parent", "value"]
    for name in ("step 0", "step 1"):
        d = stat[name, "value"][0] - p_med
        verdict = "inside the parent's spread" if abs(d) <= p_hi - p_lo else (
            "a gain by the issue's rule" if d > 3 * (p_hi - p_lo) else "outside the parent's spread, not a gain by the issue's rule")
        print(f"{name} vs parent: {d:+.4e} seq/s = {d / p_med * 100:+.2f} %; the parent's spread {p_hi - p_lo:.3e}, three times that {3 * (p_hi - p_lo):.3e}: {verdict}")
    saved = (stat["parent", "host_issue_ms_per_step"][0] - stat["step 1", "host_issue_ms_per_step"][0]) * 1e3
    print(f"host issue per step, medians: parent {stat['parent', 'host_issue_ms_per_step'][0] * 1e3:.2f} us -> step 1 {stat['step 1', 'host_issue_ms_per_step'][0] * 1e3:.2f} us "
          f"({saved:.2f} us less)", flush=True)

    print("== (2) identical outputs: bench.py --dump-outputs per arm")
    with tempfile.TemporaryDirectory() as tmp:
        dirs = {}
        for name, root, lib in ARMS:
            dirs[name] = os.path.join(tmp, name.replace(" ", "_"))
            bench(root, lib, ("--dump-outputs", dirs[name]))
        want = np.load(os.path.join(dirs["parent"], "mean.npy"))
        for name in ("step 0", "step 1"):
            got = np.load(os.path.join(dirs[name], "mean.npy"))
            print(f"   np.array_equal(mean.npy of {name}, the parent's) = {np.array_equal(got, want)}  (uint32 views: "
                  f"{np.array_equal(got.view(np.uint32), want.view(np.uint32))}; {got.shape[0]} floats)", flush=True)


if "--full-only" not in sys.argv:
    headline_arms()

if "--full" in sys.argv or "--full-only" in sys.argv:
    print("== (3) bench.py --full --no-cpu-baseline --no-live-pmc, once per arm: what else passes through DistributedEnsemble / get_fitness")

    def flat(d, prefix=""):
        for k, v in d.items():
            if isinstance(v, dict):
                yield from flat(v, prefix + k + ".")
            elif isinstance(v, (int, float)) and not isinstance(v, bool):
                yield prefix + k, v

    keep = ("kernel_ms", "e2e_value", "e2e_ms", "small_call", "member", "host_issue", "ms_per_step", "value")
    rows = {}
    for name, root, lib in ARMS:
        _, record = bench(root, lib, ("--full", "--no-cpu-baseline", "--no-live-pmc"), timeout=900)
        # (of the roofline block only the back-to-back launch time: the rest restates kernel_ms)
        rows[name] = {k: v for k, v in flat(record)
                      if k.endswith("kernel_ms_b2b") or (any(s in k for s in keep) and "roofline" not in k and "config" not in k)}
        print(f"   {name}: {len(rows[name])} figures", flush=True)
    for k in sorted(rows["parent"]):
        vals = [rows[name].get(k) for name, _, _ in ARMS]
        if all(v is not None for v in vals):
            print(f"   {k:60s} parent {vals[0]:.6g}   step 0 {vals[1]:.6g}   step 1 {vals[2]:.6g}   step 1 / parent {vals[2] / vals[0] if vals[0] else float('nan'):.3f}")
