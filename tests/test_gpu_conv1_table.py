"""The conv1-table form of the unrolled seq_len = 8 CNN kernel (`cnn_conv1_table`, csrc/score_cnn_kernel.h C1T): a tile reads conv1's four
outputs from the member's table of all 4^5 windows instead of gathering and summing kernel rows in LDS.  The table is built on the device
with the gather's own adds and ReLU, so the scores are the gather's BIT FOR BIT -- for ordinary weights, after every way of replacing them,
and for conv1 weights that hold -0.0, denormals, infinities and NaNs.

The 16-wave form is put on small launches with `cnn_big_units` = 0 (and `cnn_quad` = 0: small launches would take the quad kernel) and two
or three workgroups (`grid_blocks`), rows in device memory (fx_score_dev: host calls of this size read pinned host memory and take the
staged form).  Batch sizes: 27 tiles over two workgroups = 13 + 14 (quad round of 1 and 2 tiles behind the main loop), 31 tiles = 15 + 16
(3 and 0), a ragged last tile, three members whose unit ranges straddle a member boundary, and 1 / 16 / 17 sequences."""
import numpy as np
import pytest

from flexs_amd import _native
from flexs_amd.baselines import models as bm
from oracle import ref_np

from gpu_common import assert_scores, eng, make_native, rand_seqs  # noqa: F401  (eng: the session fixture)

pytestmark = pytest.mark.gpu

L, ALPHA, F, H, K = 8, "TGCA", 32, 100, 5
LUT = _native.make_lut(ALPHA)


@pytest.fixture()
def small_16wave(eng):
    eng.set_option("cnn_big_units", 0)
    eng.set_option("cnn_quad", 0)
    try:
        yield eng
    finally:
        eng.set_option("cnn_big_units", 12)
        eng.set_option("cnn_quad", 1)
        eng.set_option("grid_blocks", 0)
        eng.set_option("cnn_conv1_table", 1)
        eng.set_option("cnn_quad_tail", 1)


def score_dev(eng, natives, b, table):
    """(N, M) scores of rows resident in device memory, and how many launches took the table form."""
    import torch

    n, M = b.shape[0], len(natives)
    d_in = torch.from_numpy(np.ascontiguousarray(b)).cuda()
    out = torch.full((n, M), float("nan"), device="cuda")
    eng.set_option("cnn_conv1_table", table)
    before = eng.get_option("conv1_table_launches")
    eng.score_dev(list(natives), d_in.data_ptr(), n, L, LUT, out.data_ptr(), None)
    eng.sync()
    return out.cpu().numpy(), eng.get_option("conv1_table_launches") - before


@pytest.mark.parametrize("M,blocks,n", [(1, 2, 427), (1, 2, 485), (1, 2, 496), (3, 2, 427), (3, 3, 411), (1, 2, 1), (1, 2, 16), (3, 3, 17),
                                        (3, 2, 1)])
@pytest.mark.parametrize("quad_tail", [1, 0])
def test_table_form_gives_the_gathers_bits(small_16wave, M, blocks, n, quad_tail):
    eng = small_16wave
    natives, ws = zip(*[make_native(eng, "cnn", L, 4, H, F, K, seed=900 + m) for m in range(M)])
    b, seqs = rand_seqs(n, L, ALPHA, seed=7 * n + M)
    eng.set_option("grid_blocks", blocks)
    eng.set_option("cnn_quad_tail", quad_tail)
    gather, took0 = score_dev(eng, natives, b, 0)
    table, took1 = score_dev(eng, natives, b, 1)
    assert took0 == 0 and took1 == 1, (took0, took1)
    assert np.array_equal(table.view(np.uint32), gather.view(np.uint32))
    for m in range(M):
        assert_scores(table[:, m], ref_np.keras_fitness(seqs, ALPHA, "cnn", ws[m], exact=True), f"cnn L=8 conv1 table member {m}")


def test_bad_character_in_any_row_and_position(small_16wave):
    eng = small_16wave
    n = 427                                               # 13 + 14 tiles: main loop and quad round
    (nat, _), = [make_native(eng, "cnn", L, 4, H, F, K, seed=910)]
    b, _ = rand_seqs(n, L, ALPHA, seed=11)
    eng.set_option("grid_blocks", 2)
    want, _ = score_dev(eng, [nat], b, 1)
    for table in (1, 0):
        for i, row in enumerate((0, 15, 16, 200, 207, 208 + 13 * 16 - 1, n - 12, n - 1)):
            bad = b.copy()
            bad[row, i % L] = ord("N")
            with pytest.raises(ValueError):
                score_dev(eng, [nat], bad, table)
        for pos in range(L):
            bad = b.copy()
            bad[101, pos] = 0xFF
            with pytest.raises(ValueError):
                score_dev(eng, [nat], bad, table)
    again, took = score_dev(eng, [nat], b, 1)
    assert took == 1 and np.array_equal(again.view(np.uint32), want.view(np.uint32))


def test_table_follows_set_weights_and_train(small_16wave):
    """The table is rebuilt wherever weights change: the scores of a model whose weights were replaced (set_weights; a short fit) are those
    of a fresh model that only ever saw the new weights."""
    eng = small_16wave
    n = 427
    b, seqs = rand_seqs(n, L, ALPHA, seed=23)
    eng.set_option("grid_blocks", 2)
    shapes = ref_np.cnn_shapes(L, 4, F, H, K)
    nat, w_old = make_native(eng, "cnn", L, 4, H, F, K, seed=920)
    old, _ = score_dev(eng, [nat], b, 1)
    w_new = ref_np.synth_weights(shapes, 921)
    nat.set_weights(w_new)
    replaced, took = score_dev(eng, [nat], b, 1)
    fresh_nat, _ = make_native(eng, "cnn", L, 4, H, F, K, seed=921)
    fresh, _ = score_dev(eng, [fresh_nat], b, 1)
    assert took == 1 and not np.array_equal(replaced, old)
    assert np.array_equal(replaced.view(np.uint32), fresh.view(np.uint32))
    assert_scores(replaced[:, 0], ref_np.keras_fitness(seqs, ALPHA, "cnn", w_new, exact=True), "cnn L=8 conv1 table after set_weights")

    cnn = bm.CNN(L, F, H, ALPHA, seed=3)
    cnn.epochs = 2
    before, _ = score_dev(eng, [cnn.native()], b, 1)
    labels = np.random.default_rng(5).normal(size=64).astype(np.float32)
    cnn.train(seqs[:64], labels, seed=9)
    trained_w = cnn.model.get_weights()
    assert any(not np.array_equal(a, c) for a, c in zip(trained_w, bm.CNN(L, F, H, ALPHA, seed=3).model.get_weights()))
    trained, took = score_dev(eng, [cnn.native()], b, 1)
    fresh_nat = _native.NativeModel(eng, 0, L, 4, F, H, K)
    fresh_nat.set_weights(trained_w)
    fresh, _ = score_dev(eng, [fresh_nat], b, 1)
    gather, _ = score_dev(eng, [cnn.native()], b, 0)
    assert took == 1 and not np.array_equal(trained, before)
    assert np.array_equal(trained.view(np.uint32), fresh.view(np.uint32))
    assert np.array_equal(trained.view(np.uint32), gather.view(np.uint32))


def table_ref(w1, b1):
    """conv1 for all 4^5 windows as the gather computes it: float32 adds in the order bias, tap 0 ... tap 4, then max(bits, 0) on the float bits."""
    win = np.arange(1024)
    acc = np.broadcast_to(np.asarray(b1, np.float32), (1024, F)).copy()
    with np.errstate(all="ignore"):
        for j in range(K):
            acc = acc + w1[j, (win >> (2 * j)) & 3, :]
    assert acc.dtype == np.float32
    return np.maximum(acc.view(np.int32), 0).view(np.float32)


NEG_NAN = np.array([0xFFC00001], np.uint32).view(np.float32)[0]
POS_NAN = np.array([0x7FC00001], np.uint32).view(np.float32)[0]


def finite_specials(w1, b1):
    w1[0, 0, 0] = -0.0
    w1[:, :, 1] = -0.0; b1[1] = -0.0                      # a sum of negative zeros (-0.0: the integer ReLU makes it +0.0)
    w1[1, 2, 2] = 1e-40; w1[2, 0, 2] = -3e-41             # denormal kernel entries
    b1[3] = -1e-41; w1[:, :, 3] *= 1e-38                  # denormal bias, sums that end denormal
    w1[:, :, 11] = 0.0; b1[11] = 3e-42; w1[3, 2, 11] = 5e-42; w1[0, 1, 11] = -2e-42   # denormal + denormal
    w1[2, 1, 4] = np.inf
    w1[3, 3, 5] = -np.inf
    b1[10] = np.inf
    b1[12] = -np.inf


@pytest.mark.parametrize("what", ["ordinary", "specials"])
def test_table_holds_the_gathers_sums_for_all_windows(eng, what):
    """The table as the device built it (fx_debug_conv1_table) against np.float32 sequential sums and the integer-max ReLU, all 1024 windows x
    32 channels bit for bit: ordinary weights, and -0.0, denormals and +-inf in kernel rows and biases (no NaN arises in this case: the sign of
    a NaN is the hardware's, the cases below hold it to the gather)."""
    w = ref_np.synth_weights(ref_np.cnn_shapes(L, 4, F, H, K), 940)
    if what == "specials":
        finite_specials(w[0], w[1])
    nat = _native.NativeModel(eng, 0, L, 4, F, H, K)
    nat.set_weights(w)
    want = table_ref(w[0], w[1])
    got = nat.debug_conv1_table()
    assert not np.isnan(want).any()
    if what == "specials":
        tiny = (want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)
        assert tiny.sum() >= 1024 and np.isinf(want).sum() >= 1024 and (want[:, 1].view(np.uint32) == 0).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # ... and 14-mers of the same alphabet, which never take the table form, carry no table
    with pytest.raises(_native.FxError):
        make_native(eng, "cnn", 14, 4, H, F, K, seed=1)[0].debug_conv1_table()


# (name, [(array: 0 = conv1 kernel, 1 = conv1 bias; index; value)], tap, letter, channel): the windows whose letter at `tap` is `letter` hold a NaN
# in `channel` before the ReLU; every other window, and every other channel, is finite.  tap None: every window.
NAN_CASES = [
    ("stored +NaN in a kernel row", [(0, (4, 0, 7), POS_NAN)], 4, 0, 7),
    ("stored -NaN in a kernel row", [(0, (1, 3, 9), NEG_NAN)], 1, 3, 9),
    ("-inf + inf", [(1, (6,), -np.inf), (0, (0, 1, 6), np.inf)], 0, 1, 6),
    ("inf - inf", [(0, (2, 2, 13), np.inf), (0, (3, 2, 13), -np.inf), (0, (2, 0, 13), -np.inf), (0, (2, 1, 13), -np.inf), (0, (2, 3, 13), -np.inf)], None, None, 13),
    ("stored -NaN in the bias", [(1, (8,), NEG_NAN)], None, None, 8),
    ("stored +NaN in the bias", [(1, (14,), POS_NAN)], None, None, 14),
]


@pytest.mark.parametrize("case", NAN_CASES, ids=[c[0] for c in NAN_CASES])
def test_nan_signs_in_conv1_are_the_gathers(small_16wave, case):
    """The ReLU is an integer maximum on the float bits, so the SIGN of a NaN -- one that was stored, or one that inf - inf makes -- decides
    whether a channel becomes 0 or stays NaN (and the score ends as nan_to_num's 0).  One special value per model, in one (tap, letter,
    channel): rows without that letter under that tap score exactly what the model without the special scores, so most of the batch stays
    finite and a table that got the sign wrong would turn finite scores into 0 or the reverse.  What the table holds in the NaN windows is
    tied to what the gather's scores show."""
    eng = small_16wave
    name, edits, tap, letter, ch = case
    n = 427
    b, _ = rand_seqs(n, L, ALPHA, seed=31)
    eng.set_option("grid_blocks", 2)
    w = ref_np.synth_weights(ref_np.cnn_shapes(L, 4, F, H, K), 930)
    base_nat = _native.NativeModel(eng, 0, L, 4, F, H, K)
    base_nat.set_weights(w)
    base, _ = score_dev(eng, [base_nat], b, 0)
    assert (base != 0).all() and np.isfinite(base).all()
    for arr, idx, val in edits:
        w[arr][idx] = val
    nat = _native.NativeModel(eng, 0, L, 4, F, H, K)
    nat.set_weights(w)
    gather, _ = score_dev(eng, [nat], b, 0)
    table, took = score_dev(eng, [nat], b, 1)
    assert took == 1
    codes = LUT[b]                                        # (n, L)
    if tap is None:
        affected = np.ones(n, bool)
        nan_windows = np.ones(1024, bool)
        if name == "inf - inf":                           # tap 2 adds +inf or -inf to every window, tap 3 turns +inf into NaN where its letter is 2
            win = np.arange(1024)
            nan_windows = (((win >> 4) & 3) == 2) & (((win >> 6) & 3) == 2)
            affected = np.array([any(r[s + 2] == 2 and r[s + 3] == 2 for s in range(4)) for r in codes])
            plus_inf = np.array([any(r[s + 2] == 2 and r[s + 3] != 2 for s in range(4)) for r in codes])
            keep = ~plus_inf                              # (rows with a lone +inf are non-finite whatever the NaN's sign: not looked at)
            assert (affected & keep).sum() >= 5 and (~affected & keep).sum() >= 20
        else:
            keep = np.ones(n, bool)
    else:
        affected = np.array([any(r[s + tap] == letter for s in range(4)) for r in codes])
        nan_windows = ((np.arange(1024) >> (2 * tap)) & 3) == letter
        keep = np.ones(n, bool)
        assert affected.sum() >= 20 and (~affected).sum() >= 20, (affected.sum(), n)
    g, t = gather[keep, 0], table[keep, 0]
    aff = affected[keep]
    # rows the special value cannot reach: the base model's bits, in both forms
    if tap is not None and all(arr == 0 for arr, _, _ in edits):
        assert np.array_equal(g[~aff].view(np.uint32), base[keep, 0][~aff].view(np.uint32))
        assert np.array_equal(t[~aff].view(np.uint32), base[keep, 0][~aff].view(np.uint32))
    # rows it reaches: either the NaN survives the ReLU (positive sign) and every such score is nan_to_num's 0, or it becomes 0 and they are finite
    nan_kept = bool((g[aff] == 0).all())
    assert nan_kept or (g[aff] != 0).all(), "the gather's scores disagree about the NaN's sign"
    tab = nat.debug_conv1_table()
    entries = tab[nan_windows, ch]
    assert np.isnan(entries).all() if nan_kept else (entries.view(np.uint32) == 0).all(), (name, nan_kept)
    others = np.delete(tab, ch, axis=1)
    assert np.isfinite(others).all() and not np.isnan(tab[~nan_windows, ch]).any()
    assert np.array_equal(table.view(np.uint32), gather.view(np.uint32))
