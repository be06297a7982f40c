#!/usr/bin/env python3
"""Mutant-neighbourhood screening on the device (`model.screen_mutants`, fx_screen_mutants), measured.  Log: profiles/screen_mutants.log.

  python tools/runs/screen_mutants.py [--log PATH] [--cases aav,gfp1,gfp2] [--no-trace] [--append]

runs the steps below one after the other, each as a child process of its own under `timeout`, and stops at the first one that
fails (a step that faulted or hung is not followed by another on the same GPU).  Cases: aav (L = 90, radius 2, one parent:
1 447 516 rows), gfp1 / gfp2 (L = 237, radius 1 / 2, one parent: 4 504 / 10 100 230 rows); models: 3 x CNN and MLP(L, 200); k = 100.

  <case>          (a) model.screen_mutants(parents, k, radius), wall time, against (b) what a user had before: a host loop that
                  builds every string (timed once: it does not depend on the model), then model.screen(strings, k).  Warm runs
                  first, the two arms alternated, every timed run listed.  Then the device time of one warm call between two
                  events on the engine's stream.
  trace:<case>:<model>   one call under `rocprofv3 --kernel-trace --stats` (a run of its own): the enumeration kernel's share
                  of the call's kernel time beside the scoring kernels', and its rate in bytes of rows written per second.
"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PROTEIN = "ACDEFGHIKLMNPQRSTVWY"
CASES = {"aav": (90, 2), "gfp1": (237, 1), "gfp2": (237, 2)}
LIMITS = {"aav": 420, "gfp1": 180, "gfp2": 900}
K = 100
HBM_WRITE_GBS = 6.0e3                                       # what a plain store stream achieves on an MI355X (8 TB/s HBM3E spec)


def build_model(name, L):
    import flexs_amd
    from flexs_amd import synth
    from flexs_amd.baselines.models import CNN, MLP

    if name == "mlp":
        m = MLP(L, 200, PROTEIN)
        m.model.set_weights(synth.synthetic_weights(m.model.shapes(), 2000))
        return m
    out = []
    for i in range(3):
        cnn = CNN(L, 32, 100, PROTEIN)
        cnn.model.set_weights(synth.synthetic_weights(cnn.model.shapes(), 1000 + i))
        out.append(cnn)
    return flexs_amd.Ensemble(out)


def parent_of(L):
    from flexs_amd import synth

    return synth.bytes_to_strings(synth.random_sequence_bytes(1, L, PROTEIN, 7))[0]


def step_case(case):
    import numpy as np
    from flexs_amd.utils.screen import mutant_ball, mutant_ball_size

    L, radius = CASES[case]
    parent = parent_of(L)
    rows = mutant_ball_size(L, 20, radius)
    t0 = time.perf_counter()
    strings = list(mutant_ball(parent, PROTEIN, radius))
    t_build = time.perf_counter() - t0
    assert len(strings) == rows
    print(f"{case}: L = {L}, radius {radius}, one parent: {rows:,} rows = {rows * L / 1e6:.1f} MB of row bytes; "
          f"host loop building the strings: {t_build:.3f} s", flush=True)
    budget = 25.0                                           # seconds of timed runs per arm and model
    for name in ("cnn3", "mlp"):
        model = build_model(name, L)
        eng = (model.models[0] if name == "cnn3" else model)._engine()

        def dev():
            return model.screen_mutants([parent], K, radius)

        def host():
            return model.screen(strings, K)

        warm = {}
        for fn in (dev, host, dev, host):                   # warm runs (tables, scratch, the clocks)
            t0 = time.perf_counter(); warm[fn.__name__] = fn(); w = time.perf_counter() - t0
        seqs, val, _ = warm["dev"]
        idx, hval = warm["host"]
        same = seqs == [strings[i] for i in idx] and np.array_equal(val.view(np.uint32), hval.view(np.uint32))
        reps = int(max(3, min(15, budget / max(w, 1e-3))))
        res = {"dev": [], "host": []}
        for rnd in range(reps):
            for fn in ((dev, host) if rnd % 2 == 0 else (host, dev)):
                t0 = time.perf_counter(); fn(); res[fn.__name__].append(time.perf_counter() - t0)
        a, b_screen = float(np.median(res["dev"])), float(np.median(res["host"]))
        b = t_build + b_screen
        eng.sync(); eng.timer_start(); dev(); t_dev = eng.timer_stop()
        fmt = lambda xs: "[" + " ".join(f"{x * 1e3:.2f}" for x in xs) + "]"
        print(f"  {name}: (a) screen_mutants median {a * 1e3:.2f} ms of {reps} {fmt(res['dev'])} ms\n"
              f"        (b) host loop {t_build * 1e3:.1f} ms + model.screen(strings) median {b_screen * 1e3:.2f} ms {fmt(res['host'])} ms = {b * 1e3:.1f} ms\n"
              f"        (b) / (a) = {b / a:.1f} (model.screen alone / (a) = {b_screen / a:.2f}); winners and score bits equal: {same}; "
              f"device time of one call between stream events: {t_dev:.2f} ms = {rows / (t_dev * 1e-3):.3e} rows/s", flush=True)


def step_trace_child(case, name):
    L, radius = CASES[case]
    model = build_model(name, L)
    parent = parent_of(L)
    model.screen_mutants([parent], K, radius)


def step_trace(case, name, python):
    from flexs_amd.utils.screen import mutant_ball_size

    L, radius = CASES[case]
    rows = mutant_ball_size(L, 20, radius)
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix="screen_mutants_trace_")
    try:
        r = subprocess.run([prof, "--kernel-trace", "--stats", "-d", out, "--output-format", "csv", "--", python, os.path.abspath(__file__),
                            "--trace-child", f"{case}:{name}"], capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            return r.returncode
        files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            print(f"trace {case} {name}: no kernel_stats.csv written")
            return 1
        table = list(csv.DictReader(open(files[0])))
        dur = next(c for c in table[0] if "TotalDuration" in c)
        for x in table:
            x["TotalDurationNs"] = x[dur]
        total = sum(float(x["TotalDurationNs"]) for x in table)
        print(f"trace {case} {name}: one call (cold: tables and scratch included), {total / 1e6:.3f} ms of kernel time", flush=True)
        for x in sorted(table, key=lambda x: -float(x["TotalDurationNs"]))[:6]:
            print(f"    {float(x['TotalDurationNs']) / total * 100:5.1f} %  {float(x['TotalDurationNs']) / 1e3:10.1f} us  {x['Calls']:>4} calls  {x['Name'][:90]}")
        for x in table:
            if "k_enumerate_mutants" in x["Name"]:
                ns = float(x["TotalDurationNs"])
                print(f"    k_enumerate_mutants: {ns / total * 100:.2f} % of the call's kernel time; {rows * L} bytes of rows in {ns / 1e3:.1f} us = "
                      f"{rows * L / ns:.1f} GB/s written = {rows * L / ns / HBM_WRITE_GBS * 100:.1f} % of the {HBM_WRITE_GBS / 1e3:.1f} TB/s plain stores reach on this chip "
                      f"({rows / ns * 1e3:.1f} rows/us); the step is bound by {'the enumerator' if ns > total / 2 else 'the scoring kernels'}", flush=True)
        return 0
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--trace-child")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--cases", default="aav,gfp1,gfp2")
    ap.add_argument("--append", action="store_true", help="add to the log instead of starting it")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "screen_mutants.log"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.trace_child:
        step_trace_child(*args.trace_child.split(":"))
        return 0
    if args.step:
        if args.step.startswith("trace:"):
            _, case, name = args.step.split(":")
            return step_trace(case, name, sys.executable)
        step_case(args.step)
        return 0
    cases = args.cases.split(",")
    steps = [(c, LIMITS[c]) for c in cases]
    if not args.no_trace:
        steps += [(f"trace:{c}:{m}", 300) for c in cases for m in ("cnn3", "mlp")]
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "a" if args.append else "w") as log:
        for name, limit in steps:                           # chained: a step runs only if every step before it ended well
            log.write(f"== {name}\n")
            with tempfile.TemporaryFile("w+") as err:
                child = subprocess.Popen(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                                         stdout=subprocess.PIPE, stderr=err, text=True)
                for line in child.stdout:                   # (as it comes: a long step is seen to be alive)
                    log.write(line); log.flush()
                    sys.stdout.write(line); sys.stdout.flush()
                rc = child.wait()
                if rc != 0:
                    err.seek(0)
                    tail = err.read()[-4000:]
                    log.write(f"step {name} ended with status {rc}; stopping\n{tail}\n")
                    sys.stderr.write(tail)
                    return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
