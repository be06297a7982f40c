#!/usr/bin/env python3
"""Benchmark of the hot path on N GPUs of one node (one process per GPU).

Headline (`value`): BASELINE.json configs[1] -- TF-binding L=8 (alphabet TGCA), 3-member
CNN(32,100,k=5) Ensemble, 1e5 sequences per virtual-screen call per GPU -- sequence-parallel,
weak scaling.  A step = one `Ensemble.get_fitness`-equivalent pass over one batch already
resident in HBM: the fused encode+CNN scoring kernel for all three members, the ensemble-mean
kernel and, for N > 1, ONE RCCL all-gather of the per-rank means.  The step is issued through
`flexs_amd.distributed.DistributedEnsemble.launch / finish`, i.e. the product's multi-GPU class.
Beside it, at the top level of the same line: `e2e_value` = SURVEY.md 8(d)'s end-to-end metric,
`Ensemble.get_fitness(list[str]) -> np.ndarray` (host strings in, host array out) on the same
workload, and `e2e_frac_of_kernel`.

stdout carries ONE JSON line of at most 4 KB (`contract_line`): the contract keys, `roofline`
(headline kernel + one kernel_ms / issued-MFMA fraction per BASELINE config, scalars only) and
`cpu_baseline`.  Everything else the run measures (tools/bench_blocks.py: per-config blocks, the
NoisyAbstractModel half of configs[2], end-to-end splits, explorer patterns and round, the
member-parallel split) is the FULL record: one JSON line on stderr and
`gpurun_out/bench_full.json`.

    python bench.py [--gpus N --steps K --warmup W]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run measures the headline and nothing else: set up, settle the device clocks (SETTLE_STEPS untimed steps), W warm-ups,
K timed steps, the line.  Everything described above beside the headline -- the end-to-end figures, the per-config scalars, the
settled bracket, the completeness check, the back-to-back kernel time, the live PMC passes, `cpu_baseline` -- runs with `--full`.
`--dump-outputs DIR` writes what the last timed step handed out (`DIR/mean.npy`, float32) in either form.
"""
import argparse
import faulthandler
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
faulthandler.enable()

from tools.bench_common import (AAS, ALPHABET, BATCH, F, H, K, KINDS, L, M, MFMA_FLOP, MIN_TIMED_S, PEAK_TF, _sig,  # noqa: E402,F401
                                build_members, events_every, roofline_block, run_pipelined, time_launches)

MAX_LINE_BYTES = 4096            # the driver's parser lost a 24.8 KB line in round 5 (parsed 14.9 KB in round 4)


def cpu_baseline(budget_s=12.0, hard_timeout_s=150.0, nam=False, nam_budget_s=3.0):
    """Reference-style CPU path (oracle/cpu_baseline_cli.py -> oracle/torch_twin.py),
    timed on a bounded sample of the same workload in a child process with a hard
    timeout, so that the bench line is always printed.  Checker code: used ONLY here."""
    import subprocess

    cmd = [sys.executable, "-m", "oracle.cpu_baseline_cli", "--L", str(L), "--alphabet", ALPHABET,
           "--filters", str(F), "--hidden", str(H), "--kernel", str(K), "--members", str(M),
           "--sample", "50000", "--budget", str(budget_s), "--nam-budget", str(nam_budget_s)] + (["--nam"] if nam else [])
    try:
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=hard_timeout_s)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        return json.loads(line)
    except Exception as e:  # noqa: BLE001 - the GPU numbers must still be reported
        return {"value": None, "unit": "sequences/s", "cores": None, "kind": "port",
                "sample": f"cpu baseline failed: {type(e).__name__}: {str(e)[:200]}"}


def pmc_block():
    """PMC figures cannot be sampled from inside the process; they come from the rocprofv3 --pmc passes over this
    same command (tools/archive/gpu_round4.sh), committed under profiles/ -- the file is named, with the commit it was taken at
    (`commit` inside the file, else the last commit that touched it), so the numbers can be traced."""
    for name in ("r6_pmc_bench.json", "r5_pmc_bench.json", "r4_pmc_bench.json", "r3_pmc_bench.json", "r2_pmc_bench.json", "r1_pmc_traffic.json"):
        path = os.path.join(ROOT, "profiles", name)
        if os.path.exists(path):
            d = json.load(open(path))
            commit = d.get("commit")
            if not commit:
                try:
                    import subprocess

                    commit = subprocess.run(["git", "log", "-1", "--format=%h", "--", path], cwd=ROOT, capture_output=True,
                                            text=True, timeout=5).stdout.strip() or None
                except Exception:  # noqa: BLE001 (no git on the GPU box: the snapshot has no .git)
                    commit = None
            return {"hbm_bytes_per_launch": d.get("hbm_bytes_per_launch"), "mfma_util": d.get("mfma_util"),
                    "source": f"profiles/{name}" + (f" @ {commit}" if commit else "")}
    return {"hbm_bytes_per_launch": None, "mfma_util": None, "source": None}


LIVE_PMC_PASSES = (("fetch", ["FETCH_SIZE"]), ("write", ["WRITE_SIZE"]), ("sq", ["SQ_VALU_MFMA_BUSY_CYCLES", "GRBM_GUI_ACTIVE", "SQ_INSTS_MFMA"]))


def live_pmc(steps, warmup, timeout_s=75.0, kernel="k_score_cnn_mfma"):
    """`roofline.traffic` / `mfma_util_pmc` measured IN THIS RUN (round-5 verdict weak #8: they were replayed from a committed file):
    three child runs of the headline step alone (`bench.py --full --no-extras --no-cpu-baseline --no-live-pmc`) under `rocprofv3 --pmc`, one
    counter set per run as MI355X_MICROARCH.md prescribes (FETCH_SIZE and WRITE_SIZE do not fit one pass; no trace domains beside
    --pmc), per-dispatch means over the headline kernel's launches.  traffic = 2 x FETCH_SIZE (gfx950 tallies 128-byte requests at
    64 bytes) + WRITE_SIZE, KiB -> bytes; mfma_util = SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x GRBM_GUI_ACTIVE / 8 XCDs).
    Whatever goes wrong (no rocprofv3, a timeout, an empty CSV) is reported in `error` and the committed file is used instead."""
    import shutil
    import signal
    import subprocess
    import tempfile

    from tools import summarize_pmc

    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {"error": "rocprofv3 not found"}
    tmp = tempfile.mkdtemp(prefix="fx_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    got, errors = {}, []
    try:
        for label, counters in LIVE_PMC_PASSES:
            d = os.path.join(tmp, label)
            cmd = [exe, "--pmc", *counters, "-f", "csv", "-d", d, "-o", "p", "--", sys.executable, os.path.join(ROOT, "bench.py"),
                   "--steps", str(steps), "--warmup", str(warmup), "--full", "--no-extras", "--no-cpu-baseline", "--no-live-pmc", "--no-settled",
                   "--full-record", os.path.join(tmp, f"full_{label}.json")]
            try:
                pr = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, start_new_session=True)
                try:
                    _, err = pr.communicate(timeout=timeout_s)
                except subprocess.TimeoutExpired:
                    os.killpg(pr.pid, signal.SIGKILL)          # (the exact process group started above)
                    pr.communicate()
                    errors.append(f"{label}: not finished within {timeout_s:.0f} s")
                    break                                        # (a profiler that hangs once is not asked again)
                if pr.returncode != 0:
                    errors.append(f"{label}: exit {pr.returncode}: {(err or '')[-160:]}")
                    continue
                acc = summarize_pmc.load(d)
                rows = [v for k, v in acc.items() if k.startswith(kernel)]
                if not rows:
                    errors.append(f"{label}: no {kernel} dispatch in the counter CSV")
                    continue
                for c in counters:
                    vals = [x for r in rows for x in r.get(c, [])]
                    if vals:
                        got[c] = sum(vals) / len(vals)
                got["dispatches_" + label] = sum(len(r.get("_ns", [])) for r in rows)
            except Exception as ex:  # noqa: BLE001 -- never at the cost of the line
                errors.append(f"{label}: {type(ex).__name__}: {ex}"[:200])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = {"source": "live: rocprofv3 --pmc child runs of this bench run (3 passes)"}
    if "FETCH_SIZE" in got and "WRITE_SIZE" in got:
        out["hbm_bytes_per_launch"] = 1024.0 * (2.0 * got["FETCH_SIZE"] + got["WRITE_SIZE"])
    if got.get("GRBM_GUI_ACTIVE") and "SQ_VALU_MFMA_BUSY_CYCLES" in got:
        out["mfma_util"] = got["SQ_VALU_MFMA_BUSY_CYCLES"] / (1024.0 * got["GRBM_GUI_ACTIVE"] / 8.0)
    out["counters"] = got
    if errors:
        out["error"] = "; ".join(errors)
    return out


def make_report(world, N, steps, warmup, elapsed, host_issue_s, kern_ms, use_dist, mode="sequence", members=M):
    """The one JSON line of the bench contract (pure function: unit-tested on the CPU)."""
    roof = roofline_block("cnn", L, len(ALPHABET), H, F, K, members if mode == "sequence" else -(-members // world),
                          N, kern_ms, "k_score_cnn_mfma")
    pmc = pmc_block()
    roof["traffic"] = pmc["hbm_bytes_per_launch"]
    roof["mfma_util_pmc"] = pmc["mfma_util"]
    roof["pmc_source"] = pmc["source"]
    roof["note"] = ("frac = achieved / peak with achieved = MFMA instructions issued x 2048 FLOP / kernel_ms (the physical fraction "
                    "of the f32 matrix pipe, <= 1; frac_issued is the same number under its old name). frac_algorithmic = "
                    "algorithmic FLOP (2*MACs, SURVEY.md 8d) / kernel_ms / 157.3 TFLOP/s; it counts one-hot multiplies "
                    "and 'same'-padding zero taps the kernel never issues, so it can exceed 1 on long launches. "
                    "The contract line carries c1_* ... train_* scalars for every BASELINE config (contract_scalars in bench.py). mfma_util_pmc = "
                    "SQ_VALU_MFMA_BUSY_CYCLES / (4 SIMD x CU-cycles) from the rocprofv3 --pmc pass named in pmc_source; "
                    "traffic = FETCH_SIZE x2 + WRITE_SIZE from the same passes")
    if mode == "sequence":
        value, scaling = world * N * steps / elapsed, "weak"
        workload = (f"TF-binding L={L} alphabet={ALPHABET}, {members}-member CNN(num_filters={F}, hidden_size={H}, "
                    f"kernel_size={K}) Ensemble, batch={N} virtual-screen per GPU (BASELINE.json configs[1]); inputs "
                    "resident in HBM; step = fused encode+CNN scoring kernel + ensemble-mean kernel"
                    + (" + one RCCL all-gather of the per-rank means (own stream, overlapped with the next step's "
                       "compute)" if use_dist else ""))
        par = f"sequence-parallel x{world}" if world > 1 else "single GPU"
        gb = world * N
    else:
        value, scaling = N * steps / elapsed, "strong"
        workload = (f"TF-binding L={L} alphabet={ALPHABET}, {members}-member CNN Ensemble sharded member-parallel over "
                    f"{world} GPU(s), batch={N} on every rank; step = fused encode+CNN kernel for this rank's members + "
                    "one RCCL all-gather of the stacked predictions + ensemble-mean kernel on every rank")
        par = f"member-parallel x{world}"
        gb = N
    return {
        "metric": "sequences scored/sec (virtual-screen batch)",
        "value": value, "unit": "sequences/s",
        "n_gpus": world, "steps": steps, "warmup": warmup,
        "ms_per_step": elapsed / steps * 1e3,
        "host_issue_ms_per_step": host_issue_s / steps * 1e3,
        "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": workload, "global_batch": gb, "seq_len": L, "members": members, "parallelism": par},
        "roofline": roof,
    }



# ---------------------------------------------------------------------------------------------------------------
# cN = BASELINE.json configs[N-1] at the sizes the per-config block measures; tag -> key of the full record's `configs`
CONFIG_TAGS = {"c1": "C1 cnn L=8 A=4 M=1 N=1e4", "c2_1e4": "C2 cnn L=8 A=4 M=3 N=1e4", "c3": "C3 mlp L=14 A=4 H=100 M=1 N=1e5",
               "c4": "C4 ge L=90 A=20 H=100 M=8 N=1e5", "c5": "C5 cnn L=237 A=20 M=3 N=62500 (one GPU's share of 5e5)",
               "mlp_h200": "survey mlp H200 L14 N1e5", "cnn_h200": "survey cnn H200 L8 N1e5", "ge_m1": "survey ge M1 L90 N1e5",
               "mlp_aav_h200": "survey mlp H200 L90 A20 N1e5"}


def contract_scalars(full):
    """The bounded set of per-config scalars the contract line carries inside `roofline` (numbers only, 4 significant digits; keys in
    the order they are dropped LAST -> FIRST if the line had to shrink).  cN_kernel_ms / cN_frac_issued: kernel time and MFMA
    instructions issued x 2048 FLOP / time / 157.3 TFLOP/s; e2e_cN_frac_of_kernel: get_fitness(list[str]) rate / kernel rate;
    k4_*: NoisyAbstractModel neighbour search, fraction of the integer-VALU issue rate.  Pure function of the full record."""
    flat = {}

    def put(key, val, digits=4):
        if isinstance(val, bool) or val is None:
            return
        if isinstance(val, (int, float)) and np.isfinite(val):
            flat[key] = _sig(val, digits)

    confs = full.get("configs") or {}
    for tag, key in CONFIG_TAGS.items():
        b = confs.get(key)
        if isinstance(b, dict):
            put(f"{tag}_kernel_ms", b.get("kernel_ms"))
            put(f"{tag}_frac_issued", b.get("frac_issued", b.get("frac")))
    e2e = full.get("end_to_end") or {}
    for key, v in e2e.items():
        if key.endswith(" list_str") and key != "list_str" and isinstance(v, dict):
            tag = key.split()[0].lower()                            # c2 / c3 / c4 / c5
            put(f"e2e_{tag}_frac_of_kernel", v.get("frac_of_kernel_rate"))
            put(f"e2e_{tag}_seq_per_s", v.get("value"))
    er = full.get("explorer_round") or {}
    put("train_l237_frac_of_peak", er.get("train_3xCNN_L237_frac_of_peak"))
    put("train_l237_ms", er.get("train_3xCNN_L237_n500_ms"))
    put("train_l8_ms", er.get("train_3xCNN_n1000_ms"))
    put("adalead_round_ms", er.get("adalead_round_ms"))
    nam = next((v for k, v in confs.items() if k.startswith("C3 nam")), None)
    if isinstance(nam, dict):
        for k, v in (nam.get("k4") or {}).items():
            if isinstance(v, dict) and isinstance(v.get("roofline"), dict):
                put("k4_" + k.split()[-1].lower().replace("=", ""), v["roofline"].get("frac"))        # k4_c100, k4_c1000, k4_c20000
        for k, short in (("plain_landscape", "nam_plain"), ("device_table_landscape_L8", "nam_table")):
            if isinstance(nam.get(k), dict):
                put(f"{short}_seq_per_s", nam[k].get("value"))
    for tag in ("settled", "cold_start"):
        b = full.get(tag)
        if isinstance(b, dict):
            put(f"{tag}_kernel_ms", b.get("kernel_ms")); put(f"{tag}_frac_issued", b.get("frac_issued"))
    for n, v in (e2e.get("small_call_us") or {}).items():
        if n in ("1", "20", "2001"):
            put(f"small_call_n{n}_us", v, 3)
    pat = full.get("explorer_patterns") or {}
    put("dynappo_n10_us", (pat.get("dynappo_8xGE_L90_us") or {}).get("10"), 3)
    put("cmaes_p40_us", (pat.get("cmaes_3xCNN_L237_us") or {}).get("P=40"), 3)
    for k, v in (full.get("member_parallel") or {}).items():
        if isinstance(v, dict) and v.get("speedup_vs_1gpu") is not None and full.get("n_gpus", 1) > 1:
            put("mp_" + k.split()[0].lower() + "_" + k.split()[-1].lower().replace("=", "") + "_speedup", v.get("speedup_vs_1gpu"))
    return flat


def contract_line(full, full_path=None):
    """The ONE stdout line: the contract keys, `config`, `roofline` (dominant kernel + contract_scalars), `cpu_baseline`, the end-to-end
    figure beside `value` -- and nothing nested deeper, no prose blocks.  Guaranteed <= MAX_LINE_BYTES: per-config scalars are dropped
    from the end of contract_scalars' order if a future field pushed the line over (never the contract keys).  Returns (dict, text)."""
    r = full["roofline"]
    cfg = full["config"]
    line = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                 "vs_baseline", "dtype", "data")}
    for k in ("value", "ms_per_step"):
        line[k] = _sig(line[k], 6)
    c2 = (full.get("end_to_end") or {}).get("C2 3xCNN L=8 list_str")
    if isinstance(c2, dict):
        # SURVEY.md 8(d)'s metric proper: Ensemble.get_fitness(list[str]) -> ndarray, host strings in, host array out (same workload)
        line["e2e_value"] = _sig(c2.get("value"), 6)
        line["e2e_ms_per_call"] = _sig(c2.get("wall_ms"), 4)
        line["e2e_frac_of_kernel"] = _sig(c2.get("frac_of_kernel_rate"), 4)
    if r.get("kernel_ms"):
        line["kernel_value"] = _sig(cfg["global_batch"] / full["n_gpus"] / (r["kernel_ms"] * 1e-3), 6)
    line["config"] = {"workload": cfg["workload"], "global_batch": cfg["global_batch"], "seq_len": cfg["seq_len"],
                      "members": cfg["members"], "parallelism": cfg["parallelism"]}
    roof = {"bound": r["bound"], "kernel": r["kernel"], "achieved": _sig(r["achieved"]), "peak": r["peak"], "unit": r["unit"],
            "frac": _sig(r["frac"]), "frac_algorithmic": _sig(r["frac_algorithmic"]), "kernel_ms": _sig(r["kernel_ms"]),
            "traffic": (int(round(r["traffic"])) if r.get("traffic") else None), "algorithmic_bytes": r.get("algorithmic_bytes_per_launch"),
            "mfma_util_pmc": _sig(r.get("mfma_util_pmc")), "pmc_source": r.get("pmc_source")}
    if r.get("kernel_ms_b2b"):
        roof["kernel_ms_b2b"], roof["frac_b2b"] = _sig(r["kernel_ms_b2b"]), _sig(r.get("frac_b2b"))
    line["roofline"] = roof
    cb = full.get("cpu_baseline")
    if isinstance(cb, dict):
        vec, nam = cb.get("vectorised") or {}, cb.get("nam") or {}
        line["cpu_baseline"] = {"value": _sig(cb.get("value"), 6), "unit": cb.get("unit"), "cores": cb.get("cores"), "kind": cb.get("kind"),
                                "sample": (cb.get("sample_short") or cb.get("sample") or "")[:200],
                                "vectorised_value": _sig(vec.get("value"), 6), "vectorised_cores": vec.get("cores"),
                                "nam_value": _sig(nam.get("value"), 4)}
    for k in ("rccl_ranks", "debug_share_device"):
        if k in full:
            line[k] = full[k]
    if full_path:
        line["full_record"] = full_path
    extra = list(contract_scalars(full).items())
    while True:
        line["roofline"] = dict(roof, **dict(extra))
        text = json.dumps(line, separators=(",", ":"))
        if len(text.encode()) <= MAX_LINE_BYTES or not extra:
            break
        extra.pop()
    if len(text.encode()) > MAX_LINE_BYTES:                 # (cannot happen with the fields above; the contract keys are never cut)
        line["config"]["workload"] = line["config"]["workload"][:300]
        line.get("cpu_baseline", {}).pop("sample", None)
        text = json.dumps(line, separators=(",", ":"))
    return line, text


def write_full_record(full, path="gpurun_out/bench_full.json"):
    """The full record: one JSON line on stderr and `path` (default gpurun_out/bench_full.json, merged back from the GPU box; relative
    paths are relative to the repository).  Returns where it went, for the contract line's `full_record`."""
    text = json.dumps(full)
    sys.stderr.write(text + "\n")
    sys.stderr.flush()
    try:
        dst = path if os.path.isabs(path) else os.path.join(ROOT, path)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        with open(dst, "w") as f:
            f.write(text + "\n")
        return f"{path} (+ stderr)"
    except OSError:
        return "stderr"


def _free_port():
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(n_ranks, argv):
    """`python bench.py --gpus N` without a launcher: start N local ranks (one per GPU) through
    torch.distributed.run on 127.0.0.1 and hand their exit status back.  Rank 0 of the children prints the ONE JSON
    line on the inherited stdout.  The torchrun form of the contract keeps working: a process that already carries
    RANK / WORLD_SIZE never comes here."""
    import subprocess

    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_ranks}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    return subprocess.call(cmd, env=env)


def cpu_selftest(rank, world):
    """`--cpu-selftest`: the launch path of the bench (self-spawn, rendezvous, double-buffered launch / finish through
    DistributedEnsemble in both modes, MAX-over-ranks timing, one JSON line on rank 0) on the gloo backend with an
    injected table scorer -- what the CPU suite can check of `--gpus N` without N GPUs.  Not a measurement."""
    import torch
    import torch.distributed as dist

    import flexs_amd
    from flexs_amd import distributed as fd, synth

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    sys.stdout.flush()
    saved_stdout = os.dup(1)                               # gloo announces its peers on STDOUT: the one line is all that may go there
    os.dup2(2, 1)
    dist.init_process_group("gloo", rank=rank, world_size=world)

    class _Member(flexs_amd.Model):
        def train(self, *a):
            pass

        def _fitness_function(self, sequences):
            raise AssertionError("scored through score_fn")

    def score_fn(idx, b):
        s = b.astype(np.float64).sum(axis=1)
        return np.stack([np.sin(s * (m + 1) * 1e-2) for m in idx], axis=1).astype(np.float32) if idx \
            else np.zeros((b.shape[0], 0), np.float32)

    n, out = 1000, {}
    seq = synth.random_sequence_bytes(n, L, ALPHABET, seed=0)
    want = score_fn(list(range(8)), seq)
    for mode in ("member", "sequence"):
        ens = fd.DistributedEnsemble([_Member(f"m{i}") for i in range(8)], mode=mode, score_fn=score_fn)
        dist.barrier()
        t0 = time.perf_counter()
        for i in range(4):
            ens.launch(seq, n, slot=i & 1, want="mean")
            if i:
                ens.finish((i - 1) & 1)
        mean = ens.finish(1).numpy().copy()
        ens.launch(seq, n, 0, "matrix")
        mat = ens.finish(0).numpy()
        dist.barrier()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        out[mode] = {"ok": bool(np.array_equal(mat, want) and np.array_equal(mean, np.mean(want, axis=1))),
                     "max_over_ranks_s": float(t.item())}
    ranks = dist.get_world_size()
    dist.destroy_process_group()
    sys.stdout.flush()
    os.dup2(saved_stdout, 1)
    if rank == 0:
        print(json.dumps({"metric": "cpu-selftest of the launch path (gloo, injected scorer) -- not a measurement",
                          "value": None, "n_gpus": 0, "ranks": ranks, "backend": "gloo", "selftest": out}), flush=True)
    return 0 if all(v["ok"] for v in out.values()) else 1


SETTLE_STEPS = 3000              # ~0.55 s of headline steps: a cold device runs its first launches ~10 % slow (cold_start of the full record)


def last_step_output(ens, steps):
    """What the last of `steps` pipelined steps handed its caller: the `(n,)` ensemble mean, as a float32 host array.  `finish` only
    waits for the slot's gather and hands out the slot's buffer, so asking again for the slot of step K - 1 returns that step's result
    as long as no later launch has reused the slot."""
    if steps < 1:
        return None
    return ens.finish((steps - 1) & 1).to("cpu").numpy().astype(np.float32)


def dump_outputs(dirname, arrays):
    """`--dump-outputs DIR`: DIR/<name>.npy for every array of the timed path's last step (the inputs and weights are seeded, so two
    builds run with the same arguments can be compared output for output)."""
    os.makedirs(dirname, exist_ok=True)
    for name, arr in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), arr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: 100 + 1000 launches of ~0.19 ms -- long enough for the clocks to settle (the first ~50 launches of a
    # cold process run ~10 % slower: profiles/archive/r1_run22 trace), still a fraction of a second
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--mode", choices=("sequence", "member"), default="sequence",
                    help="headline split: sequence-parallel weak scaling of configs[1] (default) or member-parallel "
                         "strong scaling of an 8-member CNN ensemble")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline: the settled bracket, the completeness check of a step, "
                         "per-config kernel times, end-to-end and explorer figures, the member-parallel split, the back-to-back kernel "
                         "time, the live PMC passes and the CPU baseline (minutes; the --no-* options below trim it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step handed out (the ensemble mean of the global batch) as DIR/mean.npy, float32")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="headline only (profiling passes)")
    ap.add_argument("--no-settled", action="store_true", help="skip the >= 0.5 s second bracket (profiling passes)")
    ap.add_argument("--no-live-pmc", action="store_true",
                    help="do not run the three rocprofv3 --pmc child passes (roofline.traffic / mfma_util_pmc then come from the committed profiles/ file)")
    ap.add_argument("--full-record", default="gpurun_out/bench_full.json",
                    help="where the full record (every verbose block) is written besides stderr")
    ap.add_argument("--prepared", action="store_true",
                    help="also time the four train_swizzle forms of the GFP-length fit in a child process (round 5's A/B; ~60 s)")
    ap.add_argument("--cpu-nam", action="store_true",
                    help="cpu_baseline runs the NoisyAbstractModel CPU leg to its full 20 calls (~20 s) instead of ~3 s")
    ap.add_argument("--variant", type=int, default=0, help="cnn kernel variant (0 = auto)")
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--reserve-cus", type=int, default=-1,
                    help="CUs left free for RCCL when running distributed; -1 = 4 when WORLD_SIZE > 1, else 0")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise RCCL and run the all-gather even with one rank (exercises the N>1 code path)")
    ap.add_argument("--debug-share-device", action="store_true",
                    help="debugging aid for boxes with ONE GPU: all ranks score on device 0 and the collectives run on gloo "
                         "(planes staged through host tensors) -- exercises the N > 1 control flow of this script and of "
                         "DistributedEnsemble on real device buffers; not a measurement (the line is tagged)")
    ap.add_argument("--cpu-selftest", action="store_true",
                    help="run the launch path (self-spawn, rendezvous, launch/finish, one JSON line) on gloo with an "
                         "injected scorer; no GPU needed, not a measurement")
    args = ap.parse_args()
    if not args.full:
        args.no_extras = args.no_cpu_baseline = args.no_live_pmc = args.no_settled = True
        args.prepared = False

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        # no launcher: become one.  N ranks, one per GPU, over RCCL; rank 0 prints the line.
        raise SystemExit(spawn_ranks(args.gpus, sys.argv[1:]))

    import torch
    import torch.distributed as dist

    from flexs_amd import _native, distributed as fd, synth
    from tools import bench_blocks as bb

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: the launcher's --nproc-per-node must equal --gpus")
    if args.cpu_selftest:
        raise SystemExit(cpu_selftest(rank, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no HIP device visible); there is no CPU fallback")
    if args.debug_share_device:
        local_rank = 0
    elif torch.cuda.device_count() < world or local_rank >= torch.cuda.device_count():
        raise SystemExit(f"bench.py --gpus {world}: {world} devices needed, {torch.cuda.device_count()} visible "
                         f"(rank {rank}); one process per GPU, no oversubscription")
    torch.cuda.set_device(local_rank)
    use_dist = world > 1 or args.force_dist
    saved_stdout = None
    if use_dist:
        # RCCL prints a five-line version banner on STDOUT when its first communicator comes up; the contract is one
        # JSON line there, so file descriptor 1 points at stderr until the line is printed
        sys.stdout.flush()
        saved_stdout = os.dup(1)
        os.dup2(2, 1)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        # the exchanged messages are <= a few MB per rank: latency-bound.  Keep RCCL to a couple of
        # channels so its (overlapped) kernel does not take CUs away from the MFMA-bound scoring kernel.
        os.environ.setdefault("NCCL_MAX_NCHANNELS", "2")
        os.environ.setdefault("NCCL_MIN_NCHANNELS", "1")
        if args.debug_share_device:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))

    N = args.batch
    eng = _native.Engine.get(local_rank)
    if args.variant:
        eng.set_option("cnn_variant", args.variant)
    reserve = args.reserve_cus if args.reserve_cus >= 0 else (4 if world > 1 else 0)
    if use_dist and reserve > 0:
        # K1 is a persistent one-workgroup-per-CU kernel whose 16 waves x 128 VGPRs fill a CU's register file, so
        # RCCL's channel workgroups cannot co-reside with it: with every CU taken, the all-gather of step k would
        # start only when two K1 workgroups of step k+1 have been held back for it, stretching that launch by the
        # collective's latency.  Leaving a few CUs free (1.6 % of K1's throughput) lets it run next to step k+1.
        eng.set_option("grid_blocks", max(1, eng.get_option("num_cus") - reserve))

    # ---- headline
    head_members = M if args.mode == "sequence" else 8
    members = build_members("cnn", L, ALPHABET, head_members, local_rank)
    ens = fd.DistributedEnsemble(members, mode=args.mode)
    ens.force_collective = use_dist
    glob_n = world * N if args.mode == "sequence" else N
    with torch.cuda.stream(ens.stream):
        # sequence mode: the global batch (world x N rows); rank r reads rows [r N, (r+1) N) of it
        d_seq = torch.from_numpy(synth.random_sequence_bytes(glob_n, L, ALPHABET, seed=0)).cuda()
    ens.stream.synchronize()
    if not args.full:
        # a plain run has no other GPU work in front of its bracket (with --full the per-config blocks are, see below): the same
        # untimed steps bring the clocks up, so that a short K reads the kernel and not the ramp
        run_pipelined(ens, d_seq, glob_n, 0, SETTLE_STEPS, torch, dist, use_dist, 0)
    elapsed, host_issue_s, kern_ms = run_pipelined(ens, d_seq, glob_n, args.steps, args.warmup, torch, dist, use_dist, events_every(args.steps))
    last_mean = last_step_output(ens, args.steps) if args.dump_outputs else None
    settled = None
    if elapsed < MIN_TIMED_S and not args.no_settled:
        # the driver's K steps are reported as asked; a K this short ends before the clocks settle, so a second,
        # longer bracket (>= 0.5 s of GPU time, same code path) is reported beside it
        s_steps = int(max(args.steps, np.ceil(1.2 * MIN_TIMED_S / (elapsed / max(args.steps, 1)))))
        s_el, _, s_kern = run_pipelined(ens, d_seq, glob_n, s_steps, 0, torch, dist, use_dist, events_every(s_steps))
        settled = (s_steps, s_el, s_kern)

    # ---- untimed completeness + correctness check of the last step
    got_mean = got_nm = None
    if args.full:
        for s_ in ens._slots:
            if s_.planes is not None:
                s_.planes.fill_(float("nan"))
                s_.mean.fill_(float("nan"))
        ens.launch(d_seq, glob_n, 0, "mean")
        got_mean = ens.finish(0)
        ens.launch(d_seq, glob_n, 1, "matrix")
        got_nm = ens.finish(1)
        torch.cuda.synchronize()
        # scores are nan_to_num'ed, so a NaN that survives a step is an element nobody wrote
        assert not bool(torch.isnan(got_mean).any()) and not bool(torch.isnan(got_nm).any()), "unwritten scores"
        got_mean, got_nm = got_mean.cpu().numpy(), got_nm.cpu().numpy()
        assert got_mean.shape == (glob_n,) and got_nm.shape == (glob_n, head_members)

    extras = {}
    if not args.no_extras:
        # (a one-rank group for the in-run one-GPU reference of the member-parallel speed-ups: created by every rank)
        solo_group = dist.new_group(ranks=[0]) if (use_dist and world > 1) else None
        extras["member_parallel"] = bb.member_parallel_block(world, rank, local_rank, torch, dist, use_dist, args.steps, solo_group)

    if rank == 0:
        assert not args.full or np.array_equal(np.mean(got_nm, axis=1), got_mean), "device mean is not np.mean bit-for-bit"
        cold = None
        confs = None
        if world == 1 and not args.no_extras:
            # The per-config kernel measurements run HERE, between the first bracket and the contract's: a fresh process times its
            # first K steps while the device is still ramping its clocks (20 steps = 4 ms of GPU time: 0.205 ms per launch against
            # 0.185 settled, round-4 verdict weak #3), which says nothing about the kernel and is not how an explorer meets it -- its
            # virtual screen follows a retrain.  The contract's W warm-ups + K timed steps are therefore measured (again, same code
            # path, same barrier + synchronize bracket) after this GPU work; the first bracket is kept as `cold_start`.
            confs = bb.configs_block(eng, local_rank, torch)
            cold = {"ms_per_step": elapsed / args.steps * 1e3, "kernel_ms": kern_ms, "value": world * N * args.steps / elapsed,
                    "what": "the same W warm-ups + K timed steps as the first GPU work of the process (device clocks still ramping)"}
            elapsed, host_issue_s, kern_ms = run_pipelined(ens, d_seq, glob_n, args.steps, args.warmup, torch, dist, use_dist, events_every(args.steps))
            last_mean = last_step_output(ens, args.steps) if args.dump_outputs else None
        out = make_report(world, N, args.steps, args.warmup, elapsed, host_issue_s, kern_ms, use_dist, args.mode,
                          head_members)
        if world == 1 and not args.no_live_pmc and not args.no_extras:
            pmc = live_pmc(args.steps, args.warmup)
            out["live_pmc"] = pmc
            if pmc.get("hbm_bytes_per_launch") is not None and pmc.get("mfma_util") is not None:
                out["roofline"].update(traffic=pmc["hbm_bytes_per_launch"], mfma_util_pmc=pmc["mfma_util"], pmc_source=pmc["source"])
            else:
                out["roofline"]["pmc_source"] = f"replayed (live passes failed): {out['roofline'].get('pmc_source')}"
        out["roofline"]["kernel_ms_events"] = (f"HIP event pairs on the launch stream around every {events_every(args.steps)}th K1 launch of the K timed steps "
                                               "(a pair around every launch cost the loop 7.8 us per step: profiles/r6_bench_loop_events.log)")
        if world == 1 and args.mode == "sequence" and args.full:
            # the same launch back to back: ONE event pair around >= 40 ms of launches issued from C (no event latency inside the
            # bracket) -- the figure rocprofv3's per-dispatch mean agrees with
            try:
                stride = (N + 63) // 64 * 64
                b2b_planes = torch.zeros((head_members, stride), dtype=torch.float32, device="cuda")
                b2b_ms, _ = time_launches(eng, members, d_seq.data_ptr(), N, L, members[0]._lut, b2b_planes, stride, min_ms=40.0)
                out["roofline"]["kernel_ms_b2b"] = b2b_ms
                out["roofline"]["frac_b2b"] = out["roofline"]["frac"] * out["roofline"]["kernel_ms"] / b2b_ms
            except Exception as ex:  # noqa: BLE001
                out.setdefault("block_errors", {})["kernel_ms_b2b"] = f"{type(ex).__name__}: {ex}"[:300]
        if cold:
            cold["frac_issued"] = out["roofline"]["frac_issued"] * out["roofline"]["kernel_ms"] / cold["kernel_ms"]
            out["cold_start"] = cold
        if settled:
            s_steps, s_el, s_kern = settled
            rep = make_report(world, N, s_steps, 0, s_el, 0.0, s_kern, use_dist, args.mode, head_members)
            out["settled"] = {"steps": s_steps, "value": rep["value"], "ms_per_step": rep["ms_per_step"],
                              "kernel_ms": s_kern, "frac": rep["roofline"]["frac"],
                              "frac_issued": rep["roofline"]["frac_issued"], "frac_algorithmic": rep["roofline"]["frac_algorithmic"],
                              "what": f">= {MIN_TIMED_S} s timed region, same step, run right after the K steps above"}
        out["rccl_ranks"] = dist.get_world_size() if use_dist else 0     # ranks RCCL reports (0: no communicator)
        if args.debug_share_device:
            out["debug_share_device"] = "all ranks on device 0, collectives on gloo through host tensors: NOT a measurement"
        out.update(extras)

        def guarded(key, fn):
            """A verbose block must never cost the contract line: what goes wrong in one is a field of the full record."""
            try:
                return fn()
            except Exception as ex:  # noqa: BLE001
                out.setdefault("block_errors", {})[key] = f"{type(ex).__name__}: {ex}"[:300]
                return None

        if world == 1 and not args.no_extras:
            out["configs"] = confs
            nam = guarded("nam", lambda: bb.nam_block(eng, local_rank))
            if nam:
                out["configs"]["C3 nam L=14 A=4 (NoisyAbstractModel half of configs[2])"] = nam
            out["configs"]["C2 full (headline kernel)"] = {"kernel_ms": (settled[2] if settled else kern_ms)}
            for key, fn in (("end_to_end", lambda: bb.end_to_end_block(local_rank, out["configs"])),
                            ("explorer_round", lambda: bb.explorer_round_block(local_rank, torch)),
                            ("explorer_patterns", lambda: bb.explorer_patterns_block(local_rank))):
                got = guarded(key, fn)
                if got is not None:
                    out[key] = got
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(nam=args.cpu_nam)
        if world == 1 and args.prepared:
            out["prepared_train_swizzle"] = bb.prepared_block()
        if saved_stdout is not None:
            sys.stdout.flush()
            os.dup2(saved_stdout, 1)
        if args.dump_outputs and last_mean is not None:
            dump_outputs(args.dump_outputs, {"mean": last_mean})
        full_path = write_full_record(out, args.full_record)
        _, text = contract_line(out, full_path)
        print(text, flush=True)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
