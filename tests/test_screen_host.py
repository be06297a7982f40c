"""Screening on the host (flexs_amd/utils/screen.py): `host_top_k` against the ordering rule's oracle, the fallback path of
`screen` / `screen_all` (any model that is not a device surrogate goes through `get_fitness`), argument checks, the binding's
entry points, and the stand-alone sanitizer run of the select kernels' key / bin arithmetic (csrc/topk_keys.h).  No GPU."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import flexs_amd
from flexs_amd import _abi, _native
from flexs_amd.utils import screen as scr
from oracle import ref_np

from screen_common import bits, fills, ge_clipped_weights, ks_for, oracle_order, two_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_is_the_issue_s():
    x = np.array([0, -0.0, np.nan, np.inf, 1, np.nan, -np.inf, 1, 1e-45, -3.4e38, 0], np.float32)
    assert oracle_order(x, 4096).tolist() == [2, 5, 3, 4, 7, 8, 0, 1, 10, 9, 6]
    y = np.random.default_rng(0).standard_normal(1000)
    assert np.array_equal(oracle_order(y, 99), np.argsort(y)[:-100:-1])


@pytest.mark.parametrize("n", [1, 2, 63, 257, 4097, 100003])
def test_host_top_k_equals_the_oracle(n):
    for name, x in fills(n, 7).items():
        full = oracle_order(x, 4096)
        for k in ks_for(n):
            idx, val = scr.host_top_k(x, k)
            assert idx.dtype == np.int64 and val.dtype == np.float32
            assert np.array_equal(idx, full[:k]), (name, n, k)
            assert np.array_equal(bits(val), bits(x[full[:k]])), (name, n, k)
    for k in ks_for(n):
        x = two_values(n, k, 11)
        idx, _ = scr.host_top_k(x, k)
        assert np.array_equal(idx, oracle_order(x, k)), ("b_two_values", n, k)
    x64 = np.random.default_rng(3).standard_normal(n).round(1)            # float64 with ties, as a foreign model returns
    assert np.array_equal(scr.host_top_k(x64, 100)[0], oracle_order(x64, 100))
    assert np.array_equal(scr.host_top_k(np.arange(n) % 5, 100)[0], oracle_order(np.arange(n) % 5, 100))


def test_empty_input_and_k_range():
    idx, val = scr.host_top_k(np.zeros(0, np.float32), 5)
    assert idx.shape == (0,) and idx.dtype == np.int64 and val.shape == (0,)
    for bad in (0, -1, 4097, 10 ** 9):
        with pytest.raises(ValueError):
            scr.host_top_k(np.ones(10), bad)
    with pytest.raises(TypeError):
        scr.host_top_k(np.ones(10), 2.5)
    assert scr.host_top_k(np.ones(10), 4096)[0].tolist() == list(range(10))
    assert scr.MAX_K == _native.SMALL_CALL_ROWS == 4096


class Foreign(flexs_amd.Model):
    """A model this package knows nothing about: a few distinct scores, many ties, one NaN."""

    alphabet, seq_len = "ACG", 5

    def __init__(self):
        super().__init__("foreign")
        self.calls = []

    def train(self, sequences, labels):
        return None

    def _fitness_function(self, sequences):
        self.calls.append(len(sequences))
        out = np.array([s.count("A") - 0.5 * s.count("G") for s in sequences], np.float64)
        out[[i for i, s in enumerate(sequences) if s == "CCCCC"]] = np.nan
        return out


def all_seqs(alphabet, L):
    return ["".join(p) for p in itertools.product(alphabet, repeat=L)]


def test_fallback_screen():
    m = Foreign()
    seqs = all_seqs("ACG", 5)[::-1] * 2
    want = m._fitness_function(seqs)
    for k in (1, 7, 100, 4096):
        before = m.cost
        idx, val = m_screen = scr.screen(m, seqs, k)
        assert m.cost == before + len(seqs)                       # as get_fitness charges
        o = oracle_order(want, k)
        assert np.array_equal(idx, o) and np.array_equal(val, want[o], equal_nan=True), k
        assert len(m_screen) == 2
    assert np.isnan(scr.screen(m, seqs, 1)[1][0])                # NaN ranks above everything
    idx, val = scr.screen(m, [], 3)
    assert idx.shape == (0,) and val.shape == (0,)
    for bad in (0, 4097):
        cost = m.cost
        with pytest.raises(ValueError):
            scr.screen(m, seqs, bad)
        assert m.cost == cost                                     # refused before anything is scored


def test_fallback_ensemble_custom_combine_charges_members():
    members = [Foreign(), Foreign()]
    ens = flexs_amd.Ensemble(members, combine_with=lambda x: np.max(x, axis=1))
    seqs = all_seqs("ACG", 5)
    want = Foreign()._fitness_function(seqs)                      # (both members score alike: their maximum is either's)
    idx, val = ens.screen(seqs, 10)
    assert ens.cost == len(seqs) and all(m.cost == len(seqs) for m in members)
    assert np.array_equal(idx, oracle_order(want, 10)) and np.array_equal(val, want[idx], equal_nan=True)
    got_seqs, got_val = ens.screen_all(10)
    assert got_seqs == [seqs[i] for i in idx] and np.array_equal(got_val, val, equal_nan=True)
    assert ens.cost == 2 * len(seqs) and all(m.cost == 2 * len(seqs) for m in members)


def test_fallback_screen_all_is_in_product_order():
    m = Foreign()
    seqs = all_seqs(m.alphabet, m.seq_len)
    want = m._fitness_function(seqs)
    for k in (1, 50, 243, 300):
        before = m.cost
        got, val = scr.screen_all(m, k)
        assert m.cost == before + 3 ** 5
        o = oracle_order(want, k)
        assert got == [seqs[i] for i in o] and np.array_equal(val, want[o], equal_nan=True)

    class Flat(Foreign):
        def _fitness_function(self, sequences):
            return np.zeros(len(sequences), np.float32)

    got, _ = scr.screen_all(Flat(), 20)
    assert got == seqs[:20]                                       # all tied: itertools.product order
    got, _ = scr.screen_all(Flat(), 4, alphabet="XY", seq_len=2)
    assert got == ["XX", "XY", "YX", "YY"]


def test_fallback_screen_all_limits():
    class Wide(Foreign):
        alphabet, seq_len = "ACDEFGHIKLMNPQRSTVWY", 6          # 6.4e7 > 2^24

    m = Wide()
    with pytest.raises(ValueError, match="too large"):
        scr.screen_all(m, 10)
    assert m.cost == 0 and m.calls == []
    with pytest.raises(ValueError):
        scr.screen_all(Foreign(), 0)

    class Bare(flexs_amd.Model):
        def train(self, sequences, labels):
            return None

        def _fitness_function(self, sequences):
            return np.zeros(len(sequences))

    with pytest.raises(ValueError, match="alphabet"):
        scr.screen_all(Bare("bare"), 3)


def test_entry_points_exist():
    for name in ("fx_topk_dev", "fx_topk", "fx_score_topk", "fx_score_topk_dev", "fx_screen_all"):
        assert name in _abi.SIGNATURES and hasattr(_native.lib(), name)
    for name in ("topk_dev", "topk", "score_topk", "score_topk_dev", "screen_all"):
        assert callable(getattr(_native.Engine, name))
    from flexs_amd.baselines.models import CNN

    for cls in (CNN, flexs_amd.Ensemble):
        assert callable(cls.screen) and callable(cls.screen_all)
    text = open(os.path.join(ROOT, "flexs_amd", "csrc", "OPTIONS.md")).read()
    for key in ("topk_small_rows", "topk_large_launches", "screen_chunk_rows"):
        assert key in text


def test_ge_test_weights_tie_at_the_cut():
    """The GPU tests of the fused select rely on GlobalEpistasis members that clip almost every row (test_gpu_screen.py): with these
    seeds and this bias the float64 restatement gives, among the 20 000 rows, a run of equal ensemble scores that every k of those
    tests cuts through -- fewer than 100 rows lie outside it, and some do."""
    from flexs_amd import synth

    alphabet, L, n = "ACDEFGHIKLMNPQRSTVWY", 90, 20000
    seqs = synth.bytes_to_strings(synth.random_sequence_bytes(n, L, alphabet, 4242))
    x = ref_np.encode_batch(seqs, alphabet).reshape(n, -1)
    clipped_by_all = np.ones(n, bool)
    for m in range(8):
        w = ge_clipped_weights(L, 20, 100, 3000 + m, -1.2)
        clipped_by_all &= (x @ w[0].astype(x.dtype)[:, 0] + w[1][0]) <= 0
    outside = n - int(clipped_by_all.sum())
    assert 0 < outside < 100, outside


def test_topk_keys_under_sanitizers(tmp_path):
    """csrc/topk_keys.h -- key map, prefix / digit / bin arithmetic of the select kernels -- as a stand-alone host program under
    ASAN + UBSAN: monotone in the rule over the edge values and millions of random bit patterns, and a radix select built from
    it alone agrees with a sort."""
    exe = tmp_path / "topk_keys_check"
    r = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "native", "topk_keys_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and "unsupported" in r.stderr:
        pytest.skip("sanitizers not available to this g++")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "topk_keys_check: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
