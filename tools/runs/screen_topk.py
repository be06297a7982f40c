#!/usr/bin/env python3
"""Device-side screening (K8: score + top-k select, full-space enumeration), measured.  Log: profiles/screen_topk.log.

  python tools/runs/screen_topk.py [--log PATH]

runs the steps below one after the other, each as a child process of its own under `timeout`, and stops at the first one that
fails (a step that faulted or hung is not followed by another on the same GPU):

  kernels   3 x CNN L=8, rows resident, N = 1e5 / 1e6 / 1e7: fx_score_dev alone, fx_score_topk_dev at k = 100, the select alone
            (both forms where the size allows), beside one read of 4 N bytes at the 6.8 TB/s DESIGN.md quotes for K3
  e2e       list[str] -> winners at N = 1e5: model.screen(seqs, 100) against today's spelling, get_fitness +
            np.argsort(...)[:-101:-1], same process, arms alternated
  all8      screen_all(100), 3 x CNN L=8: 4^8 rows
  all12     screen_all(100), 3 x CNN L=12: 4^12 = 1.7e7 rows
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEPS = (("kernels", 240), ("e2e", 240), ("all8", 120), ("all12", 240))
HBM_RATE = 6.8e12


def members(L, n=3):
    import flexs_amd
    from flexs_amd.baselines.models import CNN
    from flexs_amd import synth

    out = []
    for m in range(n):
        cnn = CNN(L, 32, 100, "TGCA")
        cnn.model.set_weights(synth.synthetic_weights(cnn.model.shapes(), 1000 + m))
        out.append(cnn)
    return flexs_amd.Ensemble(out)


def timed(eng, reps, fn):
    fn(); eng.sync()
    eng.timer_start()
    for _ in range(reps):
        fn()
    return eng.timer_stop() * 1e3 / reps                    # us per call, back to back on the engine's stream


def step_kernels():
    import numpy as np
    import torch
    from flexs_amd import synth

    ens = members(8)
    eng = ens.models[0]._engine()
    natives = [m.native() for m in ens.models]
    lut = ens.models[0]._lut
    for N in (100_000, 1_000_000, 10_000_000):
        d_rows = torch.from_numpy(synth.random_sequence_bytes(N, 8, "TGCA", 1)).cuda()
        d_mean = torch.empty(N, device="cuda")
        d_idx = torch.empty(100, dtype=torch.int64, device="cuda")
        d_val = torch.empty(100, device="cuda")
        torch.cuda.synchronize()
        reps = 200 if N <= 1_000_000 else 30
        t_score = timed(eng, reps, lambda: eng.score_dev(natives, d_rows.data_ptr(), N, 8, lut, None, d_mean.data_ptr()))
        t_fused = timed(eng, reps, lambda: eng.score_topk_dev(natives, d_rows.data_ptr(), N, 8, lut, 100, d_idx.data_ptr(), d_val.data_ptr()))
        t_sel = timed(eng, reps, lambda: eng.topk_dev(d_mean.data_ptr(), N, 100, d_idx.data_ptr(), d_val.data_ptr()))
        mean = d_mean.cpu().numpy()                         # (random 8-mers repeat: equal scores, so the VALUES are compared with argsort's)
        agree = bool((mean[np.argsort(mean)[:-101:-1]] == d_val.cpu().numpy()).all() and (mean[d_idx.cpu().numpy()] == d_val.cpu().numpy()).all())
        print(f"N = {N:>10,}: fx_score_dev {t_score:8.1f} us ({N / t_score:.3e} seq/us)   fx_score_topk_dev(k=100) {t_fused:8.1f} us   "
              f"select alone {t_sel:7.1f} us = {t_sel / (4 * N / HBM_RATE * 1e6):5.1f} x one read of 4N bytes at 6.8 TB/s ({4 * N / HBM_RATE * 1e6:.1f} us)   "
              f"winners' scores = argsort's: {agree}", flush=True)
    # the two forms on one size both take
    shipped = eng.get_option("topk_small_rows")
    d_x = torch.randn(8192, device="cuda")
    torch.cuda.synchronize()
    for n in (1024, 2048, 4096, 8192):
        for k in (100, min(n, 4096)):
            d_idx = torch.empty(k, dtype=torch.int64, device="cuda")
            d_val = torch.empty(k, device="cuda")
            torch.cuda.synchronize()
            eng.set_option("topk_small_rows", 8192)
            t_small = timed(eng, 200, lambda: eng.topk_dev(d_x.data_ptr(), n, k, d_idx.data_ptr(), d_val.data_ptr()))
            eng.set_option("topk_small_rows", 0)
            t_large = timed(eng, 200, lambda: eng.topk_dev(d_x.data_ptr(), n, k, d_idx.data_ptr(), d_val.data_ptr()))
            print(f"N = {n}, k = {k}: one-workgroup form {t_small:.1f} us, radix select {t_large:.1f} us (topk_small_rows as shipped: {shipped})", flush=True)
    eng.set_option("topk_small_rows", shipped)


def step_e2e():
    import numpy as np
    from flexs_amd import synth

    ens = members(8)
    seqs = synth.bytes_to_strings(synth.random_sequence_bytes(100_000, 8, "TGCA", 1))

    def today():
        return np.argsort(ens.get_fitness(seqs))[:-101:-1]

    def screen():
        return ens.screen(seqs, 100)[0]

    res = {"today": [], "screen": []}
    for rnd in range(3):
        for name, fn in (("today", today), ("screen", screen)):
            for _ in range(3):
                fn()
            ts = []
            for _ in range(15):
                t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
            res[name].append(float(np.median(ts)) * 1e6)
    print(f"list[str] -> 100 winners, 3 x CNN L=8, N = 1e5, median of 15, three alternated rounds: get_fitness + argsort "
          f"{[round(x, 1) for x in res['today']]} us   model.screen {[round(x, 1) for x in res['screen']]} us", flush=True)
    # where the time of screen goes: packing the strings, then the call on packed rows
    from flexs_amd import _native

    eng = ens.models[0]._engine()
    natives = [m.native() for m in ens.models]
    ts_pack, ts_call = [], []
    for _ in range(15):
        t0 = time.perf_counter()
        b = _native.sequences_to_bytes(seqs, L=8, staging=eng)
        t1 = time.perf_counter()
        eng.score_topk(natives, b, ens.models[0]._lut, 100)
        ts_pack.append(t1 - t0); ts_call.append(time.perf_counter() - t1)
    print(f"  of which: packing the strings {np.median(ts_pack) * 1e6:.1f} us, fx_score_topk on the packed rows {np.median(ts_call) * 1e6:.1f} us", flush=True)


def step_all(L):
    import numpy as np

    ens = members(L)
    total = 4 ** L
    ens.screen_all(100)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); seqs, val = ens.screen_all(100); ts.append(time.perf_counter() - t0)
    t = float(np.median(ts))
    print(f"screen_all(100), 3 x CNN L={L}: {total:,} rows in {t * 1e3:.3f} ms = {total / t:.3e} rows/s (headline rate of bench.py: 1.3e9 seq/s at L=8); "
          f"best {seqs[0]} {val[0]:.6f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "screen_topk.log"))
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, ROOT)
        {"kernels": step_kernels, "e2e": step_e2e, "all8": lambda: step_all(8), "all12": lambda: step_all(12)}[args.step]()
        return 0
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as log:
        for name, limit in STEPS:                           # chained: a step runs only if every step before it ended well
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                               capture_output=True, text=True)
            log.write(f"== {name}\n{r.stdout}")
            log.flush()
            sys.stdout.write(r.stdout)
            if r.returncode != 0:
                log.write(f"step {name} ended with status {r.returncode}; stopping\n{r.stderr[-4000:]}\n")
                sys.stderr.write(r.stderr[-4000:])
                return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
