#!/usr/bin/env python3
"""Where the host time of one resident `DistributedEnsemble.launch` / `finish` step goes (headline shape: 3 x CNN, seq_len 8, N = 1e5, one rank,
sequence mode, want = "mean").  The step is host-bound (profiles/score_table_ab.log), so the sections are HOST time: `perf_counter_ns` around a
loop of STEPS (>= 1e4) repetitions of each section, after the usual settle, the GPU drained between sections.

    step_issue_breakdown.py [--label TEXT] [--out FILE] [--steps K] [--no-bench]

Sections: the pieces of the direct issue path (what `launch` / `finish` do with engine option step_call = 0, and all they did before the
prepared step existed), the native calls alone (the direct 10-argument call; the prepared step's two-argument call where the library has it),
the whole step as bench.py drives it, and the C-loop figure of `time_score_planes` (launches issued back to back from C).  `ms_per_step` of a
plain `bench.py --steps 1000` run in a fresh process is printed beside them.  The result is APPENDED to --out (default
profiles/step_issue_breakdown.log): run it before and after a change of the issue path."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_issue_breakdown.log"))
ap.add_argument("--steps", type=int, default=20000)
ap.add_argument("--no-bench", action="store_true")
args = ap.parse_args()
STEPS = max(args.steps, 10000)

import torch  # noqa: E402

from flexs_amd import _native, distributed as fd, synth  # noqa: E402
from tools.bench_common import ALPHABET, BATCH, L, M, build_members, run_pipelined  # noqa: E402

lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


eng = _native.Engine.get(0)
members = build_members("cnn", L, ALPHABET, M, 0)
ens = fd.DistributedEnsemble(members, mode="sequence")
n = BATCH
with torch.cuda.stream(ens.stream):
    d_seq = torch.from_numpy(synth.random_sequence_bytes(n, L, ALPHABET, seed=0)).cuda()
ens.stream.synchronize()
try:
    step_call = eng.get_option("step_call")
except Exception:  # noqa: BLE001  (a library from before the prepared step)
    step_call = None


def drain():
    ens.stream.synchronize()
    torch.cuda.synchronize()


def timed(fn, reps=STEPS, rounds=3):
    """Median over `rounds` of (ns for `reps` calls of fn) / reps, in microseconds."""
    out = []
    for _ in range(rounds):
        drain()
        t0 = time.perf_counter_ns()
        for _ in range(reps):
            fn()
        out.append((time.perf_counter_ns() - t0) / reps * 1e-3)
        drain()
    out.sort()
    return out[len(out) // 2]


def empty_loop():
    pass


def whole_steps(count):
    for i in range(count):
        ens.launch(d_seq, n, slot=i & 1, want="mean")
        if i:
            ens.finish((i - 1) & 1)
    ens.finish((count - 1) & 1)


def whole_step_us(rounds=3):
    out = []
    for _ in range(rounds):
        drain()
        t0 = time.perf_counter_ns()
        whole_steps(STEPS)
        issue = time.perf_counter_ns() - t0
        drain()
        out.append((issue / STEPS * 1e-3, (time.perf_counter_ns() - t0) / STEPS * 1e-3))
    out.sort()
    return out[len(out) // 2]


run_pipelined(ens, d_seq, n, 0, 3000, torch, None, False, 0)            # settle the clocks, build the tables, size the slots
say(f"== step issue breakdown {('[' + args.label + '] ') if args.label else ''}(tools/runs/step_issue_breakdown.py): {M} x CNN seq_len {L}, N = {n}, one rank, "
    f"sequence mode, want = mean; {STEPS} repetitions per section, median of 3 rounds; engine option step_call = {step_call}")
loop = timed(empty_loop)
say(f"   (an empty Python call in the same loop: {loop:.3f} us -- included in every section below)")

s = ens._slots[0]
m0 = members[0]
group = ens.group
stride = s.key[2]
natives = [m.native() for m in members]
seq_ptr = d_seq.data_ptr()
planes_ptr, local_ptr = s.planes.data_ptr(), s.local.data_ptr()
st = ens.stream
lib = eng._lib

sections = []


def section(name, fn, per_step=1):
    us = timed(fn) * per_step
    sections.append((name, us))
    say(f"   {name:86s} {us:7.3f} us")


say("-- the direct issue path, piece by piece (host time per step)")
section("_world(group), two torch.distributed queries        [launch and finish: x 2]", lambda: fd._world(group), 2)


def shape_key_device():
    key = (n, 1, stride, 1, "mean")
    ens._shape(n, "mean")
    s.key != key
    torch.device("cuda", torch.cuda.current_device())


section("_shape + slot key compare + torch.device(...)        [launch]", shape_key_device)
section("self.stream: _engine(), Engine.get, torch_stream     [launch and finish: x 2]", lambda: ens.stream, 2)


def stream_ctx():
    with torch.cuda.stream(st):
        pass


section("with torch.cuda.stream(st): (nothing enqueued inside) [launch and finish: x 2]", stream_ctx, 2)
section("[m.native() for m in members]                        [launch]", lambda: [m.native() for m in members])


def marshal():
    (C.c_void_p * M)(*[x.handle for x in natives])
    _native._lut_ptr(m0._lut)
    C.c_void_p(seq_ptr), C.c_void_p(planes_ptr), C.c_void_p(local_ptr)


section("(c_void_p * M)(...) + _lut_ptr(lut) + three c_void_p  [launch]", marshal)
arr = (C.c_void_p * M)(*[x.handle for x in natives])
lutp = _native._lut_ptr(m0._lut)
a_seq, a_planes, a_local = C.c_void_p(seq_ptr), C.c_void_p(planes_ptr), C.c_void_p(local_ptr)
section("fx_score_mean_planes_dev alone, arguments prepared     [launch; enqueues the kernel]",
        lambda: lib.fx_score_mean_planes_dev(eng.handle, arr, M, a_seq, n, L, lutp, a_planes, stride, a_local))
section("s.recv.view(-1)[:n]                                  [finish]", lambda: s.recv.view(-1)[:n])
total = sum(us for _, us in sections)
say(f"   {'sum of the sections':86s} {total:7.3f} us")

say("-- the native calls alone, through ctypes (host time per call; each enqueues the step's kernel)")
direct = timed(lambda: eng.score_mean_planes_dev(natives, seq_ptr, n, L, m0._lut, planes_ptr, stride, local_ptr))
say(f"   {'Engine.score_mean_planes_dev (array build + LUT look-up + 10-argument call)':86s} {direct:7.3f} us")
if hasattr(_native, "NativeStep"):
    step = _native.NativeStep(eng, natives, L, m0._lut, planes_ptr, stride, local_ptr, None)
    say(f"   {'NativeStep.launch(d_ascii, N) (the prepared step: one 3-argument call)':86s} {timed(lambda: step.launch(seq_ptr, n)):7.3f} us")
    del step
else:
    say("   (this library has no prepared step)")

say("-- the whole step as bench.py drives it: launch(k), finish(k - 1), two slots")
issue_us, wall_us = whole_step_us()
say(f"   {'host issue per step':86s} {issue_us:7.3f} us")
say(f"   {'wall per step, queue drained at the end':86s} {wall_us:7.3f} us")
say(f"   {'not accounted for by the sections (calls, attribute reads, slot bookkeeping)':86s} {issue_us - total:7.3f} us")

say("-- launches issued back to back from C (time_score_planes -> fx_debug_time_score: fx_score_planes_dev in a loop, one event pair)")
reps = 20000
eng.time_score_planes(natives, seq_ptr, n, L, m0._lut, planes_ptr, stride, 200)
drain()
t0 = time.perf_counter_ns()
ms = eng.time_score_planes(natives, seq_ptr, n, L, m0._lut, planes_ptr, stride, reps)
host = (time.perf_counter_ns() - t0) / reps * 1e-3
say(f"   {'GPU time per launch (event pair)':86s} {ms / reps * 1e3:7.3f} us")
say(f"   {'host wall per launch, the final event wait included: bounds the native issue cost':86s} {host:7.3f} us")
drain()
eng.sync()

if not args.no_bench:
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "1000", "--warmup", "100"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    if r.returncode == 0:
        out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        full = [ln for ln in r.stderr.splitlines() if ln.startswith("{")]
        issue = json.loads(full[-1]).get("host_issue_ms_per_step") if full else None
        say(f"-- plain bench.py --steps 1000, fresh process: ms_per_step {out['ms_per_step']:.6g} ({out['ms_per_step'] * 1e3:.2f} us)  value {out['value']:.4e}"
            + (f"  host_issue_ms_per_step {issue:.6g}" if issue is not None else ""))
    else:
        say(f"-- plain bench.py failed (exit {r.returncode}): {r.stderr[-400:]}")
say()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    f.write("\n".join(lines) + "\n")
