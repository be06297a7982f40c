"""The pooled-feature table form of K1 (`cnn_pool_table`; csrc/score_cnn_pooled.hip): a canonical seq_len = 8 member carries the global-max-pooled
conv features of all 4^8 rows, built by the conv kernel's own walk over the enumeration, and a launch whose members' tables are fresh runs only
the dense head.  The scores are those of `cnn_pool_table` = 0 BIT FOR BIT -- for every possible row, every shape of the work split, after every
way of replacing weights, and for weights that hold -0.0, denormals, infinities and NaNs.  Option 0 (the conv forms) is the reference
throughout, never the table form itself.

The 16-wave form is put on small launches the way test_gpu_conv2_prefix.py does: `cnn_big_units` = 0, `cnn_quad` = 0, two or three workgroups
(`grid_blocks`), rows in device memory, `cnn_pool_table` = 2 so that a small launch builds."""
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
    shipped = {k: eng.get_option(k) for k in ("cnn_pool_table", "cnn_conv2_prefix", "cnn_quad_tail", "cnn_conv1_table", "zero_copy_bytes", "zero_copy_mode")}
    eng.set_option("cnn_big_units", 0)
    eng.set_option("cnn_quad", 0)
    try:
        yield eng
    finally:
        eng.set_option("cnn_big_units", 12)
        eng.set_option("cnn_quad", 1)
        eng.set_option("grid_blocks", 0)
        for k, v in shipped.items():
            eng.set_option(k, v)


@pytest.fixture()
def shipped_options(eng):
    keys = ("cnn_pool_table", "cnn_conv2_prefix", "cnn_quad_tail")
    shipped = {k: eng.get_option(k) for k in keys}
    try:
        yield eng
    finally:
        for k, v in shipped.items():
            eng.set_option(k, v)


def counters(eng):
    return np.array([eng.get_option("pool_table_launches"), eng.get_option("pool_table_builds")])


def score_dev(eng, natives, b, pool):
    """(N, M) scores of rows resident in device memory; how many launch groups took the table form and how many tables were built."""
    import torch

    n, M = b.shape[0], len(natives)
    d_in = torch.from_numpy(np.ascontiguousarray(b)).cuda()
    out = torch.full((n, M), float("nan"), device="cuda")
    eng.set_option("cnn_pool_table", pool)
    before = counters(eng)
    eng.score_dev(list(natives), d_in.data_ptr(), n, L, LUT, out.data_ptr(), None)
    eng.sync()
    took, built = counters(eng) - before
    return out.cpu().numpy(), int(took), int(built)


def score_mean_planes(eng, natives, b, pool):
    """Member planes `stride` floats apart (more than the rows need) and the ensemble mean, one call."""
    import torch

    n, M = b.shape[0], len(natives)
    stride = ((n + 63) // 64) * 64 + 64
    d_in = torch.from_numpy(np.ascontiguousarray(b)).cuda()
    planes = torch.full((M, stride), float("nan"), device="cuda")
    mean = torch.full((n,), float("nan"), device="cuda")
    eng.set_option("cnn_pool_table", pool)
    before = counters(eng)
    eng.score_mean_planes_dev(list(natives), d_in.data_ptr(), n, L, LUT, planes.data_ptr(), stride, mean.data_ptr())
    eng.sync()
    return planes.cpu().numpy()[:, :n], mean.cpu().numpy(), int((counters(eng) - before)[0])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def all_rows():
    i = np.arange(4 ** L)
    letters = np.stack([(i >> (2 * j)) & 3 for j in range(L)], axis=1)
    return letters, np.frombuffer(ALPHA.encode(), np.uint8)[letters]


def test_every_row(small_16wave):
    """All 4^8 rows (row i of the batch is row i of the table) plus 48 repeats, two members: more rows than the enumeration, so option 1 builds.
    The table as read back is, row by row, what the conv-only kernel of the two-kernel path leaves for that sequence."""
    eng = small_16wave
    natives, ws = zip(*[make_native(eng, "cnn", L, 4, H, F, K, seed=960 + m) for m in range(2)])
    letters, b = all_rows()
    extra = np.random.default_rng(3).integers(0, 4 ** L, 48)
    b = np.concatenate([b, b[extra]])
    eng.set_option("grid_blocks", 3)
    want, took, built = score_dev(eng, natives, b, 0)
    assert (took, built) == (0, 0)
    got, took, built = score_dev(eng, natives, b, 1)
    assert (took, built) == (1, 2)
    assert np.array_equal(bits(got), bits(want)), f"{(bits(got) != bits(want)).sum()} scores differ"
    again, took, built = score_dev(eng, natives, b, 1)
    assert (took, built) == (1, 0) and np.array_equal(bits(again), bits(want))
    sample = np.random.default_rng(4).choice(4 ** L, 400, replace=False)
    seqs = ["".join(ALPHA[c] for c in letters[i]) for i in sample]
    for m in range(2):
        assert_scores(got[sample, m], ref_np.keras_fitness(seqs, ALPHA, "cnn", ws[m], exact=True), f"cnn L=8 pooled table member {m}")
    for m in range(2):
        table = natives[m].debug_pool_table()
        feats = natives[m].debug_conv_features(b[:4 ** L], LUT)
        assert table.shape == feats.shape == (4 ** L, 32)
        assert (table >= 0).all() and (table > 0).any()
        assert np.array_equal(bits(table), bits(feats)), f"member {m}: {(bits(table) != bits(feats)).any(axis=1).sum()} table rows differ from the conv-only path"


@pytest.mark.parametrize("M,blocks,n", [(1, 2, 1), (1, 2, 16), (3, 3, 17), (3, 2, 1), (1, 2, 427), (1, 2, 485), (1, 2, 496), (3, 2, 427), (3, 3, 411)])
def test_shapes_of_the_work_split(small_16wave, M, blocks, n):
    """Ragged last tiles, fewer tiles than waves, a member boundary inside a workgroup: the matrix, the strided planes with their mean, and the
    host call."""
    eng = small_16wave
    natives, _ = zip(*[make_native(eng, "cnn", L, 4, H, F, K, seed=970 + m) for m in range(M)])
    b, _ = rand_seqs(n, L, ALPHA, seed=5 * n + M)
    eng.set_option("grid_blocks", blocks)
    want, took, _ = score_dev(eng, natives, b, 0)
    assert took == 0
    got, took, built = score_dev(eng, natives, b, 2)
    assert (took, built) == (1, M)
    assert np.array_equal(bits(got), bits(want))
    planes0, mean0, took = score_mean_planes(eng, natives, b, 0)
    assert took == 0 and np.array_equal(bits(planes0.T), bits(want))
    planes, mean, took = score_mean_planes(eng, natives, b, 2)
    assert took == 1
    assert np.array_equal(bits(planes), bits(planes0)) and np.array_equal(bits(mean), bits(mean0))
    assert np.array_equal(bits(mean), bits(np.mean(want, axis=1)))
    # the host call: zero-copy (the rows stay in host memory: conv form), and copied to the device first
    for zc in (None, 0):
        if zc is not None:
            eng.set_option("zero_copy_bytes", 0)
            eng.set_option("zero_copy_mode", 0)
        for pool in (0, 2):
            eng.set_option("cnn_pool_table", pool)
            nm, mean_h = eng.score(list(natives), b, LUT, want_matrix=True, want_mean=True)
            assert np.array_equal(bits(nm), bits(want)) and np.array_equal(bits(mean_h), bits(mean0)), (zc, pool)


def test_policy_on_the_device(small_16wave):
    eng = small_16wave
    n = 427
    b, seqs = rand_seqs(n, L, ALPHA, seed=29)
    eng.set_option("grid_blocks", 2)
    shapes = ref_np.cnn_shapes(L, 4, F, H, K)
    nat, _ = make_native(eng, "cnn", L, 4, H, F, K, seed=980)
    want, _, _ = score_dev(eng, [nat], b, 0)
    with pytest.raises(_native.FxError):
        nat.debug_pool_table()                            # nothing has asked for it yet
    got, took, built = score_dev(eng, [nat], b, 1)        # a fresh model, a small launch: the conv form, nothing built
    assert (took, built) == (0, 0) and np.array_equal(bits(got), bits(want))
    got, took, built = score_dev(eng, [nat], b, 2)
    assert (took, built) == (1, 1) and np.array_equal(bits(got), bits(want))
    got, took, built = score_dev(eng, [nat], b, 1)        # the table is there: option 1 reads it at any size
    assert (took, built) == (1, 0) and np.array_equal(bits(got), bits(want))

    w_new = ref_np.synth_weights(shapes, 981)
    nat.set_weights(w_new)                                # stale, and nothing was built
    want_new, _, _ = score_dev(eng, [nat], b, 0)
    assert not np.array_equal(want_new, want)
    got, took, built = score_dev(eng, [nat], b, 1)
    assert (took, built) == (0, 0) and np.array_equal(bits(got), bits(want_new))
    got, took, built = score_dev(eng, [nat], b, 2)        # rebuilt
    assert (took, built) == (1, 1) and np.array_equal(bits(got), bits(want_new))
    fresh_nat, _ = make_native(eng, "cnn", L, 4, H, F, K, seed=981)
    fresh, took, built = score_dev(eng, [fresh_nat], b, 2)
    assert (took, built) == (1, 1) and np.array_equal(bits(fresh), bits(got))
    assert_scores(got[:, 0], ref_np.keras_fitness(seqs, ALPHA, "cnn", w_new, exact=True), "cnn L=8 pooled table after set_weights")

    cnn = bm.CNN(L, F, H, ALPHA, seed=3)
    cnn.epochs = 2
    before, took, built = score_dev(eng, [cnn.native()], b, 2)
    assert (took, built) == (1, 1)
    labels = np.random.default_rng(5).normal(size=64).astype(np.float32)
    cnn.train(seqs[:64], labels, seed=9)
    got, took, built = score_dev(eng, [cnn.native()], b, 1)     # after a fit: stale again
    assert (took, built) == (0, 0) and not np.array_equal(got, before)
    want_fit, _, _ = score_dev(eng, [cnn.native()], b, 0)
    assert np.array_equal(bits(got), bits(want_fit))
    got, took, built = score_dev(eng, [cnn.native()], b, 2)
    assert (took, built) == (1, 1) and np.array_equal(bits(got), bits(want_fit))
    fresh_nat = _native.NativeModel(eng, 0, L, 4, F, H, K)
    fresh_nat.set_weights(cnn.model.get_weights())
    fresh, _, _ = score_dev(eng, [fresh_nat], b, 2)
    assert np.array_equal(bits(fresh), bits(got))


def test_bad_character_in_any_row_and_position(small_16wave):
    eng = small_16wave
    n = 427                                               # 26 whole tiles and a ragged one of 11 rows: its 5 spare lanes raise nothing
    (nat, _), = [make_native(eng, "cnn", L, 4, H, F, K, seed=985)]
    b, _ = rand_seqs(n, L, ALPHA, seed=11)
    eng.set_option("grid_blocks", 2)
    want, _, _ = score_dev(eng, [nat], b, 0)
    got, took, _ = score_dev(eng, [nat], b, 2)
    assert took == 1 and np.array_equal(bits(got), bits(want))
    for i, row in enumerate((0, 15, 16, 200, 207, n - 12, n - 1)):
        bad = b.copy()
        bad[row, i % L] = ord("N")
        with pytest.raises(ValueError):
            score_dev(eng, [nat], bad, 2)
    for pos in range(L):
        bad = b.copy()
        bad[101, pos] = 0xFF
        with pytest.raises(ValueError):
            score_dev(eng, [nat], bad, 2)
        again, took, built = score_dev(eng, [nat], b, 2)  # the launch after an error is clean
        assert (took, built) == (1, 0) and np.array_equal(bits(again), bits(want)), pos


NEG_NAN = np.array([0xFFC00001], np.uint32).view(np.float32)[0]
POS_NAN = np.array([0x7FC00001], np.uint32).view(np.float32)[0]

# (name, [(array: 0 conv1 kernel (K, A, F), 1 its bias, 2 conv2 kernel (K, F, F), 3 its bias, 4 conv3 kernel (3, F, F), 5 its bias, 6 dense1 (F, H),
#          7 its bias, 8 dense2 (H, H), 9 its bias, 10 dense3 (H, 1), 11 its bias; index; value)])
SPECIAL_CASES = [
    ("-0.0 and denormals", [(0, (0, 0, 0), -0.0), (0, (1, 2, 2), 1e-40), (1, (3,), -1e-41), (2, (0, 0, 0), -0.0), (2, (1, 5, 6), 1e-40), (3, (3,), -1e-41),
                            (4, (0, 1, 2), -0.0), (4, (1, 7, 6), -3e-41), (5, (9,), 3e-42), (5, (4,), -0.0), (6, (3, 5), 1e-40), (6, (slice(None), 7), -0.0),
                            (7, (7,), -0.0), (7, (2,), 2e-41), (8, (4, 4), -2e-40), (9, (11,), -0.0), (10, (5, 0), 1e-40), (10, (6, 0), -0.0)]),
    ("+inf in a conv1 row", [(0, (2, 1, 4), np.inf)]),
    ("-inf in a conv1 row", [(0, (3, 3, 5), -np.inf)]),
    ("+inf in a conv2 block", [(2, (0, 3, 7), np.inf)]),
    ("-inf in a conv3 block", [(4, (2, 11, 8), -np.inf)]),
    ("+inf in a conv3 block", [(4, (1, 3, 20), np.inf)]),
    ("+inf in the conv3 bias", [(5, (10,), np.inf)]),
    ("-inf in the conv2 bias", [(3, (12,), -np.inf)]),
    ("inf - inf across conv3 taps", [(4, (0, 2, 13), np.inf), (4, (1, 2, 13), -np.inf)]),
    ("+inf in a dense block", [(6, (3, 40), np.inf)]),
    ("-inf in a dense bias", [(9, (17,), -np.inf)]),
    ("inf - inf in the last layer", [(7, (1,), np.inf), (7, (2,), np.inf), (10, (1, 0), 1.0), (10, (2, 0), -1.0)]),
    ("+NaN in a conv1 row", [(0, (4, 0, 7), POS_NAN)]),
    ("-NaN in a conv1 row", [(0, (1, 3, 9), NEG_NAN)]),
    ("+NaN in a conv2 block", [(2, (0, 6, 3), POS_NAN)]),
    ("-NaN in a conv3 block", [(4, (2, 20, 17), NEG_NAN)]),
    ("+NaN in the conv3 bias", [(5, (14,), POS_NAN)]),
    ("-NaN in the conv2 bias", [(3, (8,), NEG_NAN)]),
    ("+NaN in a dense block", [(8, (9, 60), POS_NAN)]),
    ("-NaN in a dense bias", [(7, (33,), NEG_NAN)]),
]


@pytest.mark.parametrize("case", SPECIAL_CASES, ids=[c[0] for c in SPECIAL_CASES])
def test_special_values_give_option_0s_bits(small_16wave, case):
    eng = small_16wave
    name, edits = case
    n = 427
    b, _ = rand_seqs(n, L, ALPHA, seed=31)
    eng.set_option("grid_blocks", 2)
    w = ref_np.synth_weights(ref_np.cnn_shapes(L, 4, F, H, K), 990)
    for arr, idx, val in edits:
        w[arr][idx] = val
    nat = _native.NativeModel(eng, 0, L, 4, F, H, K)
    nat.set_weights(w)
    want, _, _ = score_dev(eng, [nat], b, 0)
    assert not np.isnan(want).any()                       # (nan_to_num defines every score)
    if name == "-0.0 and denormals":
        assert np.isfinite(want).all() and (want != 0).all()
    got, took, built = score_dev(eng, [nat], b, 2)
    assert (took, built) == (1, 1)
    assert np.array_equal(bits(got), bits(want)), (name, int((bits(got) != bits(want)).sum()))


def test_mixed_groups(small_16wave):
    """canonical, H = 200, canonical: three launch groups, each decides for itself."""
    eng = small_16wave
    n = 427
    b, _ = rand_seqs(n, L, ALPHA, seed=41)
    eng.set_option("grid_blocks", 2)
    a, _ = make_native(eng, "cnn", L, 4, H, F, K, seed=995)
    wide, _ = make_native(eng, "cnn", L, 4, 200, F, K, seed=996)
    c, _ = make_native(eng, "cnn", L, 4, H, F, K, seed=997)
    want, took, _ = score_dev(eng, [a, wide, c], b, 0)
    assert took == 0
    got, took, built = score_dev(eng, [a, wide, c], b, 2)
    assert (took, built) == (2, 2)
    assert np.array_equal(bits(got), bits(want))
    with pytest.raises(_native.FxError):
        wide.debug_pool_table()
    c.set_weights(ref_np.synth_weights(ref_np.cnn_shapes(L, 4, F, H, K), 998))     # one group fresh, one stale
    want, _, _ = score_dev(eng, [a, wide, c], b, 0)
    got, took, built = score_dev(eng, [a, wide, c], b, 1)
    assert (took, built) == (1, 0) and np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("M,n", [(2, 70_016), (3, 100_000)])
def test_conv_forms_at_headline_size(shipped_options, M, n):
    """The large seq_len = 8 launches are answered from the table under the shipped options; with the table off, the conv forms they were built for
    still agree among themselves -- and with the table form."""
    eng = shipped_options
    natives, _ = zip(*[make_native(eng, "cnn", L, 4, H, F, K, seed=940 + m) for m in range(M)])
    b, _ = rand_seqs(n, L, ALPHA, seed=n)
    eng.set_option("cnn_quad_tail", 0)
    eng.set_option("cnn_conv2_prefix", 0)
    want, took, _ = score_dev(eng, natives, b, 0)
    assert took == 0
    for quad_tail in (0, 1):
        for depth in (0, 2):
            eng.set_option("cnn_quad_tail", quad_tail)
            eng.set_option("cnn_conv2_prefix", depth)
            before = eng.get_option("conv2_prefix_launches")
            got, took, _ = score_dev(eng, natives, b, 0)
            assert took == 0 and eng.get_option("conv2_prefix_launches") - before == (1 if depth else 0)
            assert np.array_equal(bits(got), bits(want)), (quad_tail, depth)
    got, took, built = score_dev(eng, natives, b, 1)
    assert (took, built) == (1, M) and np.array_equal(bits(got), bits(want))
