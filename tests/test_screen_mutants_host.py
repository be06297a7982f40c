"""Mutant-neighbourhood screening on the host (flexs_amd/utils/screen.py `screen_mutants`, `mutant_ball`): the enumeration order
against the definition (written out here, not imported), the fallback path for a model that is not a device surrogate, argument
checks, the binding's entry points, and the stand-alone sanitizer run of csrc/mutant_rank.h (ranking, sizes, and the enumeration
kernel's per-thread body over whole chunks).  No GPU."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import flexs_amd
from flexs_amd import _abi, _native
from flexs_amd.utils import screen as scr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTEIN = "ACDEFGHIKLMNPQRSTVWY"


def ball(s, alphabet, r):
    yield s
    for d in range(1, r + 1):
        for pos in itertools.combinations(range(len(s)), d):
            for letters in itertools.product(*[[c for c in alphabet if c != s[p]] for p in pos]):
                t = list(s)
                for p, c in zip(pos, letters):
                    t[p] = c
                yield "".join(t)


def ball_size(L, A, r):
    return 1 + L * (A - 1) + (L * (L - 1) // 2 * (A - 1) ** 2 if r == 2 else 0)


@pytest.mark.parametrize("L,A,r", [(1, 4, 2), (2, 4, 2), (5, 4, 2), (8, 4, 1), (4, 20, 2)])
def test_mutant_ball_is_the_definition(L, A, r):
    alphabet = "TGCA" if A == 4 else PROTEIN
    rng = np.random.default_rng(L * 100 + A)
    for _ in range(3):
        parent = "".join(alphabet[i] for i in rng.integers(0, A, L))
        got = list(scr.mutant_ball(parent, alphabet, r))
        assert got == list(ball(parent, alphabet, r))
        assert len(got) == ball_size(L, A, r) == scr.mutant_ball_size(L, A, r)
        assert len(set(got)) == len(got) and got[0] == parent
        assert all(sum(a != b for a, b in zip(parent, s)) <= r for s in got)
    assert scr.mutant_ball_size(90, 20, 2) == 1447516 and scr.mutant_ball_size(237, 20, 2) == 10100230
    for bad in (0, 3):
        with pytest.raises(ValueError):
            list(scr.mutant_ball("ACGT", "ACGT", bad))


class Foreign(flexs_amd.Model):
    """A model this package knows nothing about: a few distinct scores, many ties."""

    alphabet, seq_len = "ACG", 5

    def __init__(self):
        super().__init__("foreign")
        self.calls = []

    def train(self, sequences, labels):
        return None

    def _fitness_function(self, sequences):
        self.calls.append(len(sequences))
        return np.array([s.count("A") - 0.5 * s.count("G") for s in sequences], np.float64)


@pytest.mark.parametrize("radius", [1, 2])
def test_fallback_screen_mutants(radius):
    m = Foreign()
    parents = ["CCCCC", "ACGAC", "CCCCC", "GGGGA"]
    B = ball_size(5, 3, radius)
    seqs = [s for p in parents for s in ball(p, "ACG", radius)]
    assert len(seqs) == len(parents) * B
    want = Foreign()._fitness_function(seqs)
    for k in (1, 7, 100, 4096):
        before = m.cost
        got_seqs, val, parent_index = scr.screen_mutants(m, parents, k, radius)
        assert m.cost == before + len(seqs)                      # charged P * B
        idx, w_val = scr.host_top_k(want, k)
        assert got_seqs == [seqs[i] for i in idx] and np.array_equal(val, w_val)
        assert parent_index.dtype == np.int64 and np.array_equal(parent_index, idx // B)
        for s, p in zip(got_seqs, parent_index):
            assert sum(a != b for a, b in zip(parents[p], s)) <= radius
    # the parent listed twice: its copies tie, and the one of the earlier listing comes first
    got_seqs, val, parent_index = scr.screen_mutants(m, parents, 4096, radius)
    first = {}
    for s, p in zip(got_seqs, parent_index):
        if p in (0, 2):
            first.setdefault(s, []).append(p)
    assert first and all(v == [0, 2] for v in first.values())


def test_fallback_ensemble_and_defaults():
    members = [Foreign(), Foreign()]
    ens = flexs_amd.Ensemble(members, combine_with=lambda x: np.max(x, axis=1))
    seqs = list(ball("ACGAC", "ACG", 1))
    got_seqs, val, parent_index = ens.screen_mutants(["ACGAC"], 5)                 # radius defaults to 1
    idx, w_val = scr.host_top_k(Foreign()._fitness_function(seqs), 5)
    assert got_seqs == [seqs[i] for i in idx] and np.array_equal(val, w_val) and not parent_index.any()
    assert ens.cost == len(seqs) and all(m.cost == len(seqs) for m in members)
    m = Foreign()
    assert scr.screen_mutants(m, "ACGAC", 5)[0] == got_seqs                        # one parent as a plain string

    class Bare(flexs_amd.Model):                                                   # no alphabet, no seq_len: the caller's, the parents'
        def train(self, sequences, labels):
            return None

        def _fitness_function(self, sequences):
            return np.zeros(len(sequences))

    assert scr.screen_mutants(Bare("bare"), ["XY"], 9, 2, alphabet="XYZ")[0] == list(ball("XY", "XYZ", 2))   # all tied: ball order
    with pytest.raises(ValueError, match="alphabet"):
        scr.screen_mutants(Bare("bare"), ["XY"], 9, 2)


def test_fallback_limits():
    class Wide(Foreign):
        alphabet, seq_len = PROTEIN, 237

    m = Wide()
    parent = "A" * 237
    assert ball_size(237, 20, 1) * 3724 <= 2 ** 24 < ball_size(237, 20, 1) * 3725
    with pytest.raises(ValueError, match="too many"):
        scr.screen_mutants(m, [parent] * 3725, 10, 1)          # 16 777 400 rows > 2^24 = 16 777 216
    with pytest.raises(ValueError, match="too many"):
        scr.screen_mutants(m, [parent] * 2, 10, 2)             # 2 x 10 100 230
    assert m.cost == 0 and m.calls == []
    f = Foreign()
    for bad in (0, 3, -1, 2.0, True):
        with pytest.raises(ValueError):
            scr.screen_mutants(f, ["ACGAC"], 10, bad)
    for bad in (0, 4097):
        with pytest.raises(ValueError):
            scr.screen_mutants(f, ["ACGAC"], bad)
    with pytest.raises(ValueError):
        scr.screen_mutants(f, [], 10)
    assert f.cost == 0 and f.calls == []
    for bad_parent in ("ACGA", "ACGAT"):                        # wrong length, foreign letter: charged, then refused
        f = Foreign()
        with pytest.raises(ValueError):
            scr.screen_mutants(f, ["ACGAC", bad_parent], 10, 1)
        assert f.cost == 2 * ball_size(5, 3, 1) and f.calls == []


def test_entry_points_exist():
    assert "fx_screen_mutants" in _abi.SIGNATURES and hasattr(_native.lib(), "fx_screen_mutants")
    assert callable(_native.Engine.screen_mutants)
    from flexs_amd.baselines.models import CNN

    for cls in (CNN, flexs_amd.Ensemble):
        assert callable(cls.screen_mutants)
    text = open(os.path.join(ROOT, "flexs_amd", "csrc", "OPTIONS.md")).read()
    assert "mutant_rows_enumerated" in text
    assert "fx_screen_mutants" in open(os.path.join(ROOT, "include", "flexs_amd.h")).read()


def test_mutant_rank_under_sanitizers(tmp_path):
    """csrc/mutant_rank.h as a stand-alone host program under ASAN + UBSAN: exhaustive rank / unrank round trip for every L <= 40
    with A in {2, 4, 20} at radius 2, the first and last row of every first position at L = 237, 1024, 4096, the overflow guard
    at P * B = 2^31 - 1 and 2^31, and the enumeration kernel's per-thread body over whole chunks in exactly-sized heap buffers."""
    exe = tmp_path / "mutant_rank_check"
    r = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "native", "mutant_rank_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and "unsupported" in r.stderr:
        pytest.skip("sanitizers not available to this g++")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "mutant_rank_check: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
