"""Host-only checks of the prepared step (csrc/fx_step.hip): its per-call validity decision as a stand-alone program under the sanitizers, and
that the option, the ABI and the documents name it.  No GPU."""
import os
import subprocess

import pytest

from flexs_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_verdict_under_sanitizers(tmp_path):
    """csrc/fx_step_valid.h as a stand-alone host program under ASAN + UBSAN: every member stale in every way at every position for
    M = 1 .. 17 in exactly-sized heap arrays, the bounds of N against the stride, the LUT generations, a dead step with no members to read."""
    exe = tmp_path / "step_valid_check"
    r = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "native", "step_valid_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and "unsupported" in r.stderr:
        pytest.skip("sanitizers not available to this g++")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "step_valid_check: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_step_is_declared_bound_and_documented():
    for name in ("fx_step_create", "fx_step_launch", "fx_step_destroy"):
        assert name in _native.SIGNATURES
        assert hasattr(_native.lib(), name)
    assert callable(_native.NativeStep.launch)
    text = open(os.path.join(ROOT, "flexs_amd", "csrc", "OPTIONS.md")).read()
    assert "step_call" in text
    assert "fx_step_launch" in open(os.path.join(ROOT, "include", "flexs_amd.h")).read()
