"""Screening on the device: score + select in one call (`model.screen`, fx_score_topk*) and the enumeration of the whole sequence
space (`model.screen_all`, fx_screen_all), against `get_fitness` of THE SAME model followed by the host rule
(flexs_amd.utils.screen.host_top_k, itself held to the oracle in test_screen_host.py).  Exact: indices with array_equal, scores
by their bits.  The GlobalEpistasis members clip almost every row (screen_common.ge_clipped_weights), so the cut runs through
long runs of bit-equal REAL model outputs and the index tie rule decides."""
import itertools

import numpy as np
import pytest

import flexs_amd
from flexs_amd import _native, synth
from flexs_amd.baselines import models as bm
from flexs_amd.utils.screen import host_top_k
from oracle import ref_np

from gpu_common import eng  # noqa: F401  (the module's engine fixture)
from screen_common import bits, ge_clipped_weights

pytestmark = pytest.mark.gpu

PROTEIN = "ACDEFGHIKLMNPQRSTVWY"
KS = (1, 100, 1999)


@pytest.fixture()
def shipped(eng):
    keys = ("topk_small_rows", "screen_chunk_rows", "cnn_pool_table")
    keep = {k: eng.get_option(k) for k in keys}
    try:
        yield eng
    finally:
        for k, v in keep.items():
            eng.set_option(k, v)


def cnn_ensemble(L=8, alphabet="TGCA", members=3, seed=1000):
    out = []
    for m in range(members):
        cnn = bm.CNN(L, 32, 100, alphabet)
        cnn.model.set_weights(ref_np.synth_weights(ref_np.cnn_shapes(L, len(alphabet), 32, 100, 5), seed + m))
        out.append(cnn)
    return flexs_amd.Ensemble(out)


def mlp(L, alphabet, seed=2000):
    m = bm.MLP(L, 100, alphabet)
    m.model.set_weights(ref_np.synth_weights(ref_np.mlp_shapes(L, len(alphabet), 100), seed))
    return m


def ge(L, alphabet, seed, bias):
    m = bm.GlobalEpistasisModel(L, 100, alphabet)
    m.model.set_weights(ge_clipped_weights(L, len(alphabet), 100, seed, bias))
    return m


def ge_ensemble():
    return flexs_amd.Ensemble([ge(90, PROTEIN, 3000 + m, -1.2) for m in range(8)])       # (seeds and bias: test_screen_host.py checks the ties)


def members_of(model):
    return list(getattr(model, "models", [])) or [model]


def reset_costs(model):
    for m in [model] + members_of(model):
        m.cost = 0


def check_screen(model, seqs, ks, large_expected=None):
    want_scores = model.get_fitness(seqs)
    n = len(seqs)
    eng_ = members_of(model)[0]._engine()
    for k in ks:
        reset_costs(model)
        before = eng_.get_option("topk_large_launches")
        idx, val = model.screen(seqs, k)
        if large_expected is not None:
            assert eng_.get_option("topk_large_launches") - before == large_expected
        assert model.cost == n and all(m.cost == n for m in members_of(model))
        w_idx, w_val = host_top_k(want_scores, k)
        assert idx.dtype == np.int64 and val.dtype == np.float32
        assert np.array_equal(idx, w_idx), (k, n)
        assert np.array_equal(bits(val), bits(w_val)), (k, n)
    return want_scores


@pytest.mark.parametrize("n", [5000, 70001])
def test_cnn_ensemble_screen(shipped, n):
    ens = cnn_ensemble()
    seqs = synth.bytes_to_strings(synth.random_sequence_bytes(n, 8, "TGCA", 77))
    check_screen(ens, seqs, KS, large_expected=1)           # (more rows than the shipped topk_small_rows)
    if n == 5000:                                           # the same rows through the one-workgroup form
        shipped.set_option("topk_small_rows", 8192)
        check_screen(ens, seqs, KS, large_expected=0)


def test_mlp_screen(shipped):
    m = mlp(14, "UGCA")
    seqs = synth.bytes_to_strings(synth.random_sequence_bytes(20000, 14, "UGCA", 78))
    check_screen(m, seqs, KS, large_expected=1)
    assert shipped.get_option("topk_small_rows") == 4096
    check_screen(m, np.array(seqs[:4096]), (100,), large_expected=0)          # a NumPy string array, the one-workgroup form
    check_screen(m, seqs[:4097], (100,), large_expected=1)


def test_ge_ensemble_screen_ties_at_the_cut(shipped):
    ens = ge_ensemble()
    seqs = synth.bytes_to_strings(synth.random_sequence_bytes(20000, 90, PROTEIN, 4242))
    scores = check_screen(ens, seqs, KS, large_expected=1)
    ranked = scores[host_top_k(scores, 4096)[0]]
    for k in (100, 1999):                                   # the cut lies inside a run of equal scores longer than k
        assert bits(ranked[k - 1 : k + 1]).tolist() == [bits(ranked[k - 1 : k])[0]] * 2
    values, counts = np.unique(scores, return_counts=True)
    assert counts.max() > 1999 and values.size > 1


def test_device_rows_and_host_rows_agree(shipped):
    import torch

    eng = shipped
    for model, L, alphabet in ((cnn_ensemble(), 8, "TGCA"), (mlp(14, "UGCA"), 14, "UGCA")):
        natives = [m.native() for m in members_of(model)]
        lut = members_of(model)[0]._lut
        b = synth.random_sequence_bytes(20000, L, alphabet, 79)
        want = host_top_k(model.get_fitness(synth.bytes_to_strings(b)), 100)
        idx, val = eng.score_topk(natives, b, lut, 100)
        d_b = torch.from_numpy(b).cuda()
        d_idx = torch.full((100,), -1, dtype=torch.int64, device="cuda")
        d_val = torch.full((100,), float("nan"), device="cuda")
        torch.cuda.synchronize()
        assert eng.score_topk_dev(natives, d_b.data_ptr(), 20000, L, lut, 100, d_idx.data_ptr(), d_val.data_ptr()) == 100
        eng.sync()
        for got_idx, got_val in ((idx, val), (d_idx.cpu().numpy(), d_val.cpu().numpy())):
            assert np.array_equal(got_idx, want[0]) and np.array_equal(bits(got_val), bits(want[1]))


def test_bad_character_raises_after_charging(shipped):
    ens = cnn_ensemble()
    seqs = synth.bytes_to_strings(synth.random_sequence_bytes(20000, 8, "TGCA", 80))
    seqs[12345] = "TGCATGCN"
    for model in (ens, ens.models[0]):
        reset_costs(ens)
        with pytest.raises(ValueError):
            model.screen(seqs, 100)
        assert model.cost == len(seqs)
        if model is ens:
            assert all(m.cost == len(seqs) for m in ens.models)
    natives = [m.native() for m in ens.models]
    b = _native.sequences_to_bytes(seqs)
    idx = np.full(100, -1, np.int64)
    val = np.full(100, np.nan, np.float32)
    import ctypes as C

    arr = (C.c_void_p * 3)(*[m.handle for m in natives])
    n = C.c_int(0)
    rc = shipped._lib.fx_score_topk(shipped.handle, arr, 3, _native._ptr(b), len(seqs), 8, _native._lut_ptr(ens.models[0]._lut), 100,
                                    _native._ptr(idx), _native._ptr(val), C.byref(n))
    assert rc == _native.FX_EBADCHAR and (idx == -1).all() and np.isnan(val).all()       # nothing written
    with pytest.raises(ValueError):
        ens.screen(seqs[:100], 0)
    idx, val = ens.screen([], 5)
    assert idx.shape == (0,) and val.shape == (0,)
    seqs[12345] = "TGCATGCA"
    check_screen(ens, seqs, (100,))                         # the engine is fine afterwards


def all_strings(alphabet, L):
    return ["".join(p) for p in itertools.product(alphabet, repeat=L)]


def check_screen_all(model, alphabet, L, ks):
    seqs = all_strings(alphabet, L)
    scores = model.get_fitness(seqs)
    natives = [m.native() for m in members_of(model)]
    eng_ = members_of(model)[0]._engine()
    for k in ks:
        reset_costs(model)
        got_seqs, got_val = model.screen_all(k)
        assert model.cost == len(seqs) and all(m.cost == len(seqs) for m in members_of(model))
        w_idx, w_val = host_top_k(scores, k)
        assert got_seqs == [seqs[i] for i in w_idx], k
        assert np.array_equal(bits(got_val), bits(w_val)), k
        idx, rows, val = eng_.screen_all(natives, L, alphabet, members_of(model)[0]._lut, k)
        assert np.array_equal(idx, w_idx) and np.array_equal(bits(val), bits(w_val))
        assert synth.bytes_to_strings(rows) == got_seqs
    return scores


def test_screen_all_cnn_default_and_small_chunks(shipped):
    ens = cnn_ensemble()
    assert shipped.get_option("screen_chunk_rows") == 1 << 22
    results = {}
    for pool in (1, 0):
        shipped.set_option("cnn_pool_table", pool)
        shipped.set_option("screen_chunk_rows", 1 << 22)
        check_screen_all(ens, "TGCA", 8, KS)
        results[pool] = ens.screen_all(1999)
        shipped.set_option("screen_chunk_rows", 4096)       # 16 chunks: the running winners are merged 15 times
        check_screen_all(ens, "TGCA", 8, KS)
    assert results[0][0] == results[1][0] and np.array_equal(bits(results[0][1]), bits(results[1][1]))


def test_screen_all_ties_cross_chunks(shipped):
    m = ge(6, "TGCA", 3100, -1.0)
    shipped.set_option("screen_chunk_rows", 1024)
    scores = check_screen_all(m, "TGCA", 6, KS + (4096,))
    ranked = scores[host_top_k(scores, 4096)[0]]
    assert ranked[1998] == ranked[1999]                     # the cut of k = 1999 lies inside a run of equal scores ...
    tied = np.flatnonzero(scores == ranked[1998])
    assert tied.size > 1999 and len(set(tied // 1024)) == 4  # ... that has rows in every chunk: global row numbers decide
    shipped.set_option("topk_small_rows", 0)                # chunks through the radix select
    check_screen_all(m, "TGCA", 6, (1999,))


@pytest.mark.parametrize("alphabet,chunk", [(PROTEIN, 1 << 22), (PROTEIN, 3008), ("ACDEFGHIKL", 304)])
def test_screen_all_other_alphabets(shipped, alphabet, chunk):
    """20 letters (8 000 rows) and 10 letters (1 000 rows, whose last chunk of 88 rows is no multiple of 16)."""
    m = mlp(3, alphabet, seed=2100)
    shipped.set_option("screen_chunk_rows", chunk)
    check_screen_all(m, alphabet, 3, (1, 100, 1999))


def test_screen_all_limits(shipped):
    m = mlp(14, PROTEIN)                                    # 20^14 rows
    with pytest.raises(ValueError):
        m.screen_all(10)
    assert m.cost == 0
    with pytest.raises(ValueError):
        cnn_ensemble().screen_all(4097)
    for bad in (0, 8, 100, (1 << 26) + 16):
        with pytest.raises(_native.FxError):
            shipped.set_option("screen_chunk_rows", bad)
