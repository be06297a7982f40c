"""The conv2-prefix form of the unrolled seq_len = 8 CNN kernel (`cnn_conv2_prefix` = 1, 2; csrc/score_cnn_kernel.h C2P): a tile reads conv2's
accumulator after the first one or two valid taps of each position from the member's prefix tables and runs only the remaining taps.  The tables
are built on the device by the scoring kernel's own init_bias + mma_layer chain over the conv1 table's rows, so the scores are those of
depth 0 BIT FOR BIT -- for every possible row, after every way of replacing weights, and for weights that hold -0.0, denormals, infinities
and NaNs.  Depth 0 (all taps) is the reference throughout, never the table form itself.

The 16-wave form is put on small launches the way test_gpu_conv1_table.py does: `cnn_big_units` = 0, `cnn_quad` = 0, two or three workgroups
(`grid_blocks`), rows in device memory (score_dev)."""
import numpy as np
import pytest

from flexs_amd import _native
from flexs_amd.baselines import models as bm
from oracle import ref_np

from gpu_common import assert_scores, eng, make_native, rand_seqs  # noqa: F401  (eng: the session fixture)

pytestmark = pytest.mark.gpu

L, ALPHA, F, H, K = 8, "TGCA", 32, 100, 5
LUT = _native.make_lut(ALPHA)
DEPTHS = (1, 2)


@pytest.fixture()
def small_16wave(eng):
    shipped = eng.get_option("cnn_conv2_prefix")
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
        eng.set_option("cnn_conv2_prefix", shipped)


def score_dev(eng, natives, b, depth, table=1):
    """(N, M) scores of rows resident in device memory, and how many launches took the prefix form."""
    import torch

    n, M = b.shape[0], len(natives)
    d_in = torch.from_numpy(np.ascontiguousarray(b)).cuda()
    out = torch.full((n, M), float("nan"), device="cuda")
    eng.set_option("cnn_conv1_table", table)
    eng.set_option("cnn_conv2_prefix", depth)
    before = eng.get_option("conv2_prefix_launches")
    eng.score_dev(list(natives), d_in.data_ptr(), n, L, LUT, out.data_ptr(), None)
    eng.sync()
    return out.cpu().numpy(), eng.get_option("conv2_prefix_launches") - before


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_all_65536_rows(small_16wave):
    """Every possible row (4096 tiles), two members: every entry of every table is read in every position role it has."""
    eng = small_16wave
    natives, ws = zip(*[make_native(eng, "cnn", L, 4, H, F, K, seed=950 + m) for m in range(2)])
    i = np.arange(4 ** L)
    letters = np.stack([(i >> (2 * j)) & 3 for j in range(L)], axis=1)
    b = np.frombuffer(ALPHA.encode(), np.uint8)[letters]
    assert len({r.tobytes() for r in b}) == 4 ** L
    eng.set_option("grid_blocks", 3)
    full, took = score_dev(eng, natives, b, 0)
    assert took == 0
    for depth in DEPTHS:
        got, took = score_dev(eng, natives, b, depth)
        assert took == 1
        assert np.array_equal(bits(got), bits(full)), f"depth {depth}: {(bits(got) != bits(full)).sum()} scores differ"
    seqs = ["".join(ALPHA[c] for c in row) for row in letters]
    for m in range(2):
        assert_scores(full[:, m], ref_np.keras_fitness(seqs, ALPHA, "cnn", ws[m], exact=True), f"cnn L=8 all rows member {m}")


@pytest.mark.parametrize("M,blocks,n", [(1, 2, 427), (1, 2, 485), (1, 2, 496), (3, 2, 427), (3, 3, 411), (1, 2, 1), (1, 2, 16), (3, 3, 17),
                                        (3, 2, 1)])
@pytest.mark.parametrize("quad_tail", [1, 0])
def test_prefix_form_gives_the_full_walks_bits(small_16wave, M, blocks, n, quad_tail):
    eng = small_16wave
    natives, _ = zip(*[make_native(eng, "cnn", L, 4, H, F, K, seed=900 + m) for m in range(M)])
    b, _ = rand_seqs(n, L, ALPHA, seed=7 * n + M)
    eng.set_option("grid_blocks", blocks)
    eng.set_option("cnn_quad_tail", quad_tail)
    full, took = score_dev(eng, natives, b, 0)
    assert took == 0
    for depth in DEPTHS:
        got, took = score_dev(eng, natives, b, depth)
        assert took == 1, (depth, took)
        assert np.array_equal(bits(got), bits(full)), depth
        # without the conv1 table the launch silently takes the gather and all taps
        got, took = score_dev(eng, natives, b, depth, table=0)
        assert took == 0, (depth, took)
        assert np.array_equal(bits(got), bits(full)), depth


def test_bad_character_in_any_row_and_position(small_16wave):
    eng = small_16wave
    n = 427                                               # 13 + 14 tiles: main loop and quad round
    (nat, _), = [make_native(eng, "cnn", L, 4, H, F, K, seed=910)]
    b, _ = rand_seqs(n, L, ALPHA, seed=11)
    eng.set_option("grid_blocks", 2)
    want, _ = score_dev(eng, [nat], b, 0)
    for depth in (0,) + DEPTHS:
        for i, row in enumerate((0, 15, 16, 200, 207, 208 + 13 * 16 - 1, n - 12, n - 1)):
            bad = b.copy()
            bad[row, i % L] = ord("N")
            with pytest.raises(ValueError):
                score_dev(eng, [nat], bad, depth)
        for pos in range(L):
            bad = b.copy()
            bad[101, pos] = 0xFF
            with pytest.raises(ValueError):
                score_dev(eng, [nat], bad, depth)
        again, took = score_dev(eng, [nat], b, depth)
        assert took == (1 if depth else 0) and np.array_equal(bits(again), bits(want)), depth


def test_tables_follow_set_weights_and_train(small_16wave):
    """The tables are rebuilt wherever weights change: the scores of a model whose weights were replaced (set_weights; a short fit) are those
    of a fresh model that only ever saw the new weights, and those of depth 0."""
    eng = small_16wave
    n = 427
    b, seqs = rand_seqs(n, L, ALPHA, seed=23)
    eng.set_option("grid_blocks", 2)
    shapes = ref_np.cnn_shapes(L, 4, F, H, K)
    nat, _ = make_native(eng, "cnn", L, 4, H, F, K, seed=920)
    old = {d: score_dev(eng, [nat], b, d)[0] for d in DEPTHS}
    w_new = ref_np.synth_weights(shapes, 921)
    nat.set_weights(w_new)
    fresh_nat, _ = make_native(eng, "cnn", L, 4, H, F, K, seed=921)
    full, _ = score_dev(eng, [nat], b, 0)
    for depth in DEPTHS:
        replaced, took = score_dev(eng, [nat], b, depth)
        fresh, _ = score_dev(eng, [fresh_nat], b, depth)
        assert took == 1 and not np.array_equal(replaced, old[depth])
        assert np.array_equal(bits(replaced), bits(fresh)) and np.array_equal(bits(replaced), bits(full))
    assert_scores(full[:, 0], ref_np.keras_fitness(seqs, ALPHA, "cnn", w_new, exact=True), "cnn L=8 conv2 prefix after set_weights")

    cnn = bm.CNN(L, F, H, ALPHA, seed=3)
    cnn.epochs = 2
    before = {d: score_dev(eng, [cnn.native()], b, d)[0] for d in DEPTHS}
    labels = np.random.default_rng(5).normal(size=64).astype(np.float32)
    cnn.train(seqs[:64], labels, seed=9)
    trained_w = cnn.model.get_weights()
    assert any(not np.array_equal(a, c) for a, c in zip(trained_w, bm.CNN(L, F, H, ALPHA, seed=3).model.get_weights()))
    fresh_nat = _native.NativeModel(eng, 0, L, 4, F, H, K)
    fresh_nat.set_weights(trained_w)
    full, _ = score_dev(eng, [cnn.native()], b, 0)
    for depth in DEPTHS:
        trained, took = score_dev(eng, [cnn.native()], b, depth)
        fresh, _ = score_dev(eng, [fresh_nat], b, depth)
        assert took == 1 and not np.array_equal(trained, before[depth])
        assert np.array_equal(bits(trained), bits(fresh)) and np.array_equal(bits(trained), bits(full))


NEG_NAN = np.array([0xFFC00001], np.uint32).view(np.float32)[0]
POS_NAN = np.array([0x7FC00001], np.uint32).view(np.float32)[0]

# (name, [(array: 0 = conv1 kernel (K, A, F), 1 = conv1 bias, 2 = conv2 kernel (K, F, F), 3 = conv2 bias; index; value)])
SPECIAL_CASES = [
    ("-0.0 and denormals", [(0, (0, 0, 0), -0.0), (0, (1, 2, 2), 1e-40), (0, (2, 0, 2), -3e-41), (1, (3,), -1e-41),
                            (2, (0, 0, 0), -0.0), (2, (1, 5, 6), 1e-40), (2, (2, 7, 6), -3e-41), (2, (3, slice(None), 9), 0.0), (2, (3, 4, 9), 5e-42),
                            (2, (4, slice(None), 10), -0.0), (3, (1,), -0.0), (3, (3,), -1e-41), (3, (9,), 3e-42)]),
    ("+inf in a conv1 row", [(0, (2, 1, 4), np.inf)]),
    ("-inf in a conv1 row", [(0, (3, 3, 5), -np.inf)]),
    ("+inf in a conv2 block", [(2, (0, 3, 7), np.inf)]),
    ("-inf in a conv2 block", [(2, (2, 11, 8), -np.inf)]),
    ("+inf in the conv2 bias", [(3, (10,), np.inf)]),
    ("-inf in the conv2 bias", [(3, (12,), -np.inf)]),
    ("inf - inf across conv2 taps", [(2, (1, 2, 13), np.inf), (2, (2, 2, 13), -np.inf)]),
    ("+NaN in a conv1 row", [(0, (4, 0, 7), POS_NAN)]),
    ("-NaN in a conv1 row", [(0, (1, 3, 9), NEG_NAN)]),
    ("+NaN in a conv2 block", [(2, (0, 6, 3), POS_NAN)]),
    ("-NaN in a conv2 block", [(2, (3, 20, 17), NEG_NAN)]),
    ("+NaN in the conv2 bias", [(3, (14,), POS_NAN)]),
    ("-NaN in the conv2 bias", [(3, (8,), NEG_NAN)]),
]


@pytest.mark.parametrize("case", SPECIAL_CASES, ids=[c[0] for c in SPECIAL_CASES])
def test_special_values_give_depth_0s_bits(small_16wave, case):
    """-0.0, denormals, +-inf and a NaN of either sign in conv1 rows, conv2 blocks and the conv2 bias, one kind per model: every score of the
    batch (nan_to_num defines them all) has the bits of the full walk, main loop and quad round alike."""
    eng = small_16wave
    name, edits = case
    n = 427
    b, _ = rand_seqs(n, L, ALPHA, seed=31)
    eng.set_option("grid_blocks", 2)
    w = ref_np.synth_weights(ref_np.cnn_shapes(L, 4, F, H, K), 930)
    for arr, idx, val in edits:
        w[arr][idx] = val
    nat = _native.NativeModel(eng, 0, L, 4, F, H, K)
    nat.set_weights(w)
    full, _ = score_dev(eng, [nat], b, 0)
    assert not np.isnan(full).any()
    if name == "-0.0 and denormals":
        assert np.isfinite(full).all() and (full != 0).all()
    for depth in DEPTHS:
        got, took = score_dev(eng, [nat], b, depth)
        assert took == 1
        assert np.array_equal(bits(got), bits(full)), (name, depth, int((bits(got) != bits(full)).sum()))


@pytest.mark.parametrize("depth", DEPTHS)
def test_tables_read_back(eng, depth):
    """The tables as the device built them (fx_debug_conv2_prefix) against a float64 evaluation of the bias plus the 32 * depth products, with the
    conv1 table as read back from the device as input.  Bound: the standard forward bound of an f32 chain of n = 32 * depth + 1 terms (products
    rounded, then summed in any order), (n + 1) * 2^-24 * sum |terms|; no tuned tolerance."""
    w = ref_np.synth_weights(ref_np.cnn_shapes(L, 4, F, H, K), 940)
    nat = _native.NativeModel(eng, 0, L, 4, F, H, K)
    nat.set_weights(w)
    c1 = nat.debug_conv1_table().astype(np.float64)       # (1024, 32), post-ReLU
    got = nat.debug_conv2_prefix(depth)
    assert got.shape == (3, 4 ** (4 + depth), F) and got.dtype == np.float32
    w2, b2 = w[2].astype(np.float64), w[3].astype(np.float64)
    idx = np.arange(4 ** (4 + depth))
    n_terms = 32 * depth + 1
    for j0 in range(3):
        want = np.broadcast_to(b2, (idx.size, F)).copy()
        mag = np.abs(want)
        for d in range(depth):
            rows = c1[(idx >> (2 * d)) & 1023]            # window d of the entry
            want += rows @ w2[j0 + d]
            mag += np.abs(rows) @ np.abs(w2[j0 + d])
        err = np.abs(got[j0].astype(np.float64) - want)
        bound = (n_terms + 1) * 2.0 ** -24 * mag
        print(f"depth {depth} family {j0}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
        assert (err <= bound).all(), (depth, j0, float((err / bound).max()))
    # ... and 14-mers of the same alphabet, which never take the form, carry no tables
    with pytest.raises(_native.FxError):
        make_native(eng, "cnn", 14, 4, H, F, K, seed=1)[0].debug_conv2_prefix(depth)
