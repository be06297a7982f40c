"""The score-table form of K1 (`cnn_score_table`; csrc/score_cnn_lookup.hip): a canonical seq_len = 8 member carries its score for all 4^8 rows,
built by the head-only kernel's own walk over the enumeration, and a launch group whose members' tables are fresh is one table read per row and
member -- plus the ensemble mean where the group is the whole ensemble.  The scores are those of `cnn_pool_table` = 0 BIT FOR BIT (the `uint32`
view of the floats): the conv forms are the reference throughout, never a table form.

The 16-wave pick is put on small launches the way test_gpu_pool_table.py does: `cnn_big_units` = 0, `cnn_quad` = 0, `cnn_pool_table` = 2 so that
a small launch builds; rows in device memory.  The lookup kernel's workgroup is 256 threads, one row each."""
import numpy as np
import pytest

from flexs_amd import _native
from flexs_amd.baselines import models as bm
from oracle import ref_np

from gpu_common import eng, make_native, rand_seqs  # noqa: F401  (eng: the session fixture)

pytestmark = pytest.mark.gpu

L, ALPHA, F, H, K = 8, "TGCA", 32, 100, 5
LUT = _native.make_lut(ALPHA)
COUNTERS = ("pool_table_launches", "pool_table_builds", "score_table_launches", "score_table_builds")


@pytest.fixture()
def small_16wave(eng):
    shipped = {k: eng.get_option(k) for k in ("cnn_pool_table", "cnn_score_table")}
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
    shipped = {k: eng.get_option(k) for k in ("cnn_pool_table", "cnn_score_table")}
    try:
        yield eng
    finally:
        for k, v in shipped.items():
            eng.set_option(k, v)


def counters(eng):
    return np.array([eng.get_option(k) for k in COUNTERS])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def device_rows(b, offset=0):
    """The rows in device memory, `offset` bytes behind the start of an aligned buffer."""
    import torch

    buf = torch.zeros(b.size + offset + 16, dtype=torch.uint8, device="cuda")
    buf[offset:offset + b.size] = torch.from_numpy(np.ascontiguousarray(b).reshape(-1)).cuda()
    assert buf.data_ptr() % 16 == 0
    return buf


def score_dev(eng, natives, b, pool, score, offset=0):
    """(N, M) scores of rows resident in device memory, and the deltas of COUNTERS."""
    import torch

    n, M = b.shape[0], len(natives)
    d_in = device_rows(b, offset)
    out = torch.full((n, M), float("nan"), device="cuda")
    eng.set_option("cnn_pool_table", pool)
    eng.set_option("cnn_score_table", score)
    before = counters(eng)
    eng.score_dev(list(natives), d_in.data_ptr() + offset, n, L, LUT, out.data_ptr(), None)
    eng.sync()
    return out.cpu().numpy(), tuple(int(v) for v in counters(eng) - before)


def score_mean_planes(eng, natives, b, pool, score, offset=0):
    """Member planes `stride` floats apart (more than the rows need, NaN beforehand) and the ensemble mean, one call: the whole planes
    array, the mean, the deltas of COUNTERS and whether the scoring kernel wrote the mean."""
    import torch

    n, M = b.shape[0], len(natives)
    stride = ((n + 63) // 64) * 64 + 64
    d_in = device_rows(b, offset)
    planes = torch.full((M, stride), float("nan"), device="cuda")
    mean = torch.full((n,), float("nan"), device="cuda")
    eng.set_option("cnn_pool_table", pool)
    eng.set_option("cnn_score_table", score)
    before = counters(eng)
    eng.score_mean_planes_dev(list(natives), d_in.data_ptr() + offset, n, L, LUT, planes.data_ptr(), stride, mean.data_ptr())
    eng.sync()
    return planes.cpu().numpy(), mean.cpu().numpy(), tuple(int(v) for v in counters(eng) - before), bool(eng.get_option("fused_mean_done"))


def all_rows():
    i = np.arange(4 ** L)
    letters = np.stack([(i >> (2 * j)) & 3 for j in range(L)], axis=1)
    return np.frombuffer(ALPHA.encode(), np.uint8)[letters]


def test_every_row(small_16wave):
    """All 4^8 rows in table order plus 48 repeats, two members: more rows than the enumeration, so option 1 builds.  The table as read back
    is column m of the conv forms' scores."""
    eng = small_16wave
    natives, _ = zip(*[make_native(eng, "cnn", L, 4, H, F, K, seed=1960 + m) for m in range(2)])
    b = all_rows()
    b = np.concatenate([b, b[np.random.default_rng(3).integers(0, 4 ** L, 48)]])
    eng.set_option("grid_blocks", 3)
    want, delta = score_dev(eng, natives, b, 0, 1)
    assert delta == (0, 0, 0, 0)
    for nat in natives:
        with pytest.raises(_native.FxError):
            nat.debug_score_table()                       # nothing has asked for it yet
    got, delta = score_dev(eng, natives, b, 1, 1)
    assert delta == (1, 2, 1, 2)
    assert np.array_equal(bits(got), bits(want)), f"{(bits(got) != bits(want)).sum()} scores differ"
    again, delta = score_dev(eng, natives, b, 1, 1)       # a second call builds nothing
    assert delta == (1, 0, 1, 0) and np.array_equal(bits(again), bits(want))
    for m in range(2):
        table = natives[m].debug_score_table()
        assert table.shape == (4 ** L,) and table.dtype == np.float32
        assert np.array_equal(bits(table), bits(want[:4 ** L, m])), f"member {m}: {(bits(table) != bits(want[:4 ** L, m])).sum()} table entries differ"


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("n", [1, 16, 17, 255, 256, 257, 427])
def test_edges_of_the_lookups_work_split(small_16wave, n, M, blocks):
    """Around one workgroup of 256 rows, a ragged grid-stride tail, one member and three, one workgroup and three: the matrix, the strided
    planes with their padding, and the mean -- with the rows one byte off an aligned buffer."""
    eng = small_16wave
    natives, _ = zip(*[make_native(eng, "cnn", L, 4, H, F, K, seed=1970 + m) for m in range(M)])
    b, _ = rand_seqs(n, L, ALPHA, seed=7 * n + M)
    eng.set_option("grid_blocks", blocks)
    want, delta = score_dev(eng, natives, b, 0, 1)
    assert delta == (0, 0, 0, 0)
    planes0, mean0, _, fused0 = score_mean_planes(eng, natives, b, 0, 1)
    assert not fused0 and np.array_equal(bits(planes0[:, :n].T), bits(want))
    for offset in (0, 1):
        got, delta = score_dev(eng, natives, b, 2, 1, offset)
        assert delta[0] == 1 and delta[2] == 1, delta
        assert np.array_equal(bits(got), bits(want)), offset
        planes, mean, delta, fused = score_mean_planes(eng, natives, b, 2, 1, offset)
        assert delta == (1, 0, 1, 0)
        assert fused == (M > 1)
        assert np.array_equal(bits(planes[:, :n]), bits(planes0[:, :n])) and np.array_equal(bits(mean), bits(mean0)), offset
        assert np.array_equal(bits(mean), bits(np.mean(want, axis=1)))
        assert np.isnan(planes[:, n:]).all() and np.isnan(planes0[:, n:]).all()     # the padding beyond n: never written


def test_the_mean_kernel_is_gone_only_where_it_may_be(small_16wave):
    eng = small_16wave
    n = 427
    b, _ = rand_seqs(n, L, ALPHA, seed=43)
    eng.set_option("grid_blocks", 2)
    a, _ = make_native(eng, "cnn", L, 4, H, F, K, seed=1995)
    wide, _ = make_native(eng, "cnn", L, 4, 200, F, K, seed=1996)
    c, _ = make_native(eng, "cnn", L, 4, H, F, K, seed=1997)
    # all members in one group: the lookup writes the mean; the head-only kernel and the conv forms leave it to the mean kernel
    want, _ = score_dev(eng, [a, c], b, 0, 1)
    _, mean0, _, fused = score_mean_planes(eng, [a, c], b, 0, 1)
    assert not fused
    planes, mean, delta, fused = score_mean_planes(eng, [a, c], b, 2, 1)
    assert fused and delta == (1, 2, 1, 2)
    assert np.array_equal(bits(planes[:, :n].T), bits(want)) and np.array_equal(bits(mean), bits(mean0))
    assert np.array_equal(bits(mean), bits(np.mean(want, axis=1)))
    _, mean, delta, fused = score_mean_planes(eng, [a, c], b, 2, 0)
    assert not fused and delta == (1, 0, 0, 0) and np.array_equal(bits(mean), bits(mean0))
    # canonical, H = 200, canonical: three launch groups, two lookups, and the mean kernel behind them
    want, delta = score_dev(eng, [a, wide, c], b, 0, 1)
    assert delta == (0, 0, 0, 0)
    got, delta = score_dev(eng, [a, wide, c], b, 2, 1)
    assert delta == (2, 0, 2, 0) and np.array_equal(bits(got), bits(want))
    planes, mean, delta, fused = score_mean_planes(eng, [a, wide, c], b, 2, 1)
    assert not fused and delta == (2, 0, 2, 0)
    assert np.array_equal(bits(planes[:, :n].T), bits(want)) and np.array_equal(bits(mean), bits(np.mean(want, axis=1)))
    with pytest.raises(_native.FxError):
        wide.debug_score_table()


def test_stale_after_set_weights_and_after_a_fit(small_16wave):
    eng = small_16wave
    n = 427
    b, seqs = rand_seqs(n, L, ALPHA, seed=29)
    eng.set_option("grid_blocks", 2)
    shapes = ref_np.cnn_shapes(L, 4, F, H, K)
    nat, _ = make_native(eng, "cnn", L, 4, H, F, K, seed=1980)
    want, _ = score_dev(eng, [nat], b, 0, 1)
    got, delta = score_dev(eng, [nat], b, 2, 1)
    assert delta == (1, 1, 1, 1) and np.array_equal(bits(got), bits(want))
    nat.debug_score_table()

    nat.set_weights(ref_np.synth_weights(shapes, 1981))    # stale, and nothing is built
    want_new, _ = score_dev(eng, [nat], b, 0, 1)
    assert not np.array_equal(want_new, want)
    got, delta = score_dev(eng, [nat], b, 1, 1)            # a small launch: the conv form
    assert delta == (0, 0, 0, 0) and np.array_equal(bits(got), bits(want_new))
    with pytest.raises(_native.FxError):
        nat.debug_score_table()
    got, delta = score_dev(eng, [nat], b, 2, 1)            # both tables rebuilt
    assert delta == (1, 1, 1, 1) and np.array_equal(bits(got), bits(want_new))
    got, delta = score_dev(eng, [nat], b, 1, 1)            # the tables are there: option 1 reads them at any size
    assert delta == (1, 0, 1, 0) and np.array_equal(bits(got), bits(want_new))

    cnn = bm.CNN(L, F, H, ALPHA, seed=3)
    cnn.epochs = 2
    before, delta = score_dev(eng, [cnn.native()], b, 2, 1)
    assert delta == (1, 1, 1, 1)
    labels = np.random.default_rng(5).normal(size=64).astype(np.float32)
    cnn.train(seqs[:64], labels, seed=9)
    want_fit, _ = score_dev(eng, [cnn.native()], b, 0, 1)
    assert not np.array_equal(want_fit, before)
    got, delta = score_dev(eng, [cnn.native()], b, 1, 1)   # after a fit: stale again
    assert delta == (0, 0, 0, 0) and np.array_equal(bits(got), bits(want_fit))
    with pytest.raises(_native.FxError):
        cnn.native().debug_score_table()
    got, delta = score_dev(eng, [cnn.native()], b, 2, 1)
    assert delta == (1, 1, 1, 1) and np.array_equal(bits(got), bits(want_fit))


def test_bad_character_in_any_row_and_position(small_16wave):
    eng = small_16wave
    n = 427                                               # one whole workgroup of 256 rows and a ragged one
    (nat, _), = [make_native(eng, "cnn", L, 4, H, F, K, seed=1985)]
    b, _ = rand_seqs(n, L, ALPHA, seed=11)
    eng.set_option("grid_blocks", 2)
    want, _ = score_dev(eng, [nat], b, 0, 1)
    got, delta = score_dev(eng, [nat], b, 2, 1)
    assert delta[2] == 1 and np.array_equal(bits(got), bits(want))
    for i, row in enumerate((0, 200, 255, 256, n - 1)):   # a first, middle and last row
        bad = b.copy()
        bad[row, i % L] = ord("N")
        with pytest.raises(ValueError):
            score_dev(eng, [nat], bad, 2, 1)
        again, delta = score_dev(eng, [nat], b, 2, 1)     # the launch after an error is clean
        assert delta == (1, 0, 1, 0) and np.array_equal(bits(again), bits(want)), row
    for pos in range(L):
        bad = b.copy()
        bad[101, pos] = 0xFF
        with pytest.raises(ValueError):
            score_dev(eng, [nat], bad, 2, 1)
        again, delta = score_dev(eng, [nat], b, 2, 1)
        assert delta == (1, 0, 1, 0) and np.array_equal(bits(again), bits(want)), pos


NEG_NAN = np.array([0xFFC00001], np.uint32).view(np.float32)[0]

# (name, [(array: 0 conv1 kernel (K, A, F), 1 its bias, 2 conv2 kernel (K, F, F), 3 its bias, 4 conv3 kernel (3, F, F), 5 its bias, 6 dense1 (F, H),
#          7 its bias, 8 dense2 (H, H), 9 its bias, 10 dense3 (H, 1), 11 its bias; index; value)]): four of test_gpu_pool_table.py's SPECIAL_CASES
SPECIAL_CASES = [
    ("-0.0 and denormals", [(0, (0, 0, 0), -0.0), (0, (1, 2, 2), 1e-40), (1, (3,), -1e-41), (2, (0, 0, 0), -0.0), (2, (1, 5, 6), 1e-40), (3, (3,), -1e-41),
                            (4, (0, 1, 2), -0.0), (4, (1, 7, 6), -3e-41), (5, (9,), 3e-42), (5, (4,), -0.0), (6, (3, 5), 1e-40), (6, (slice(None), 7), -0.0),
                            (7, (7,), -0.0), (7, (2,), 2e-41), (8, (4, 4), -2e-40), (9, (11,), -0.0), (10, (5, 0), 1e-40), (10, (6, 0), -0.0)]),
    ("+inf in a dense block", [(6, (3, 40), np.inf)]),
    ("inf - inf in the last layer", [(7, (1,), np.inf), (7, (2,), np.inf), (10, (1, 0), 1.0), (10, (2, 0), -1.0)]),
    ("-NaN in a dense bias", [(7, (33,), NEG_NAN)]),
]


@pytest.mark.parametrize("case", SPECIAL_CASES, ids=[c[0] for c in SPECIAL_CASES])
def test_special_values_give_option_0s_bits(small_16wave, case):
    """The table stores what fx_nan_to_num made of the score."""
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
    want, _ = score_dev(eng, [nat], b, 0, 1)
    assert not np.isnan(want).any()                       # (nan_to_num defines every score)
    if name == "-0.0 and denormals":
        assert np.isfinite(want).all() and (want != 0).all()
    got, delta = score_dev(eng, [nat], b, 2, 1)
    assert delta == (1, 1, 1, 1)
    assert np.array_equal(bits(got), bits(want)), (name, int((bits(got) != bits(want)).sum()))
    assert not np.isnan(nat.debug_score_table()).any()


@pytest.mark.parametrize("M,blocks,n", [(3, 3, 17), (1, 2, 427), (3, 2, 427)])
def test_the_pooled_head_form_keeps_its_coverage(small_16wave, M, blocks, n):
    """`cnn_score_table` = 0: the head-only kernel scores, as before the option existed -- rows of test_gpu_pool_table.py's
    test_shapes_of_the_work_split, which under option 1 exercises the lookup."""
    eng = small_16wave
    natives, _ = zip(*[make_native(eng, "cnn", L, 4, H, F, K, seed=970 + m) for m in range(M)])
    b, _ = rand_seqs(n, L, ALPHA, seed=5 * n + M)
    eng.set_option("grid_blocks", blocks)
    want, delta = score_dev(eng, natives, b, 0, 0)
    assert delta == (0, 0, 0, 0)
    got, delta = score_dev(eng, natives, b, 2, 0)
    assert delta == (1, M, 0, 0)
    assert np.array_equal(bits(got), bits(want))
    planes0, mean0, _, _ = score_mean_planes(eng, natives, b, 0, 0)
    planes, mean, delta, fused = score_mean_planes(eng, natives, b, 2, 0)
    assert delta == (1, 0, 0, 0) and not fused
    assert np.array_equal(bits(planes[:, :n]), bits(planes0[:, :n])) and np.array_equal(bits(planes[:, :n].T), bits(want))
    assert np.array_equal(bits(mean), bits(mean0)) and np.array_equal(bits(mean), bits(np.mean(want, axis=1)))
    for nat in natives:
        with pytest.raises(_native.FxError):
            nat.debug_score_table()                       # option 0 builds no score table


def test_headline_size(shipped_options):
    """M = 3, n = 100 000 under the shipped options: both values of `cnn_score_table` give the conv forms' bits."""
    eng = shipped_options
    M, n = 3, 100_000
    pool = eng.get_option("cnn_pool_table")
    natives, _ = zip(*[make_native(eng, "cnn", L, 4, H, F, K, seed=1940 + m) for m in range(M)])
    b, _ = rand_seqs(n, L, ALPHA, seed=n)
    want, delta = score_dev(eng, natives, b, 0, 1)
    assert delta == (0, 0, 0, 0)
    planes0, mean0, _, _ = score_mean_planes(eng, natives, b, 0, 1)
    assert np.array_equal(bits(planes0[:, :n].T), bits(want))
    got, delta = score_dev(eng, natives, b, pool, 0)
    assert delta == (1, M, 0, 0) and np.array_equal(bits(got), bits(want))
    got, delta = score_dev(eng, natives, b, pool, 1)
    assert delta == (1, 0, 1, M) and np.array_equal(bits(got), bits(want))
    planes, mean, delta, fused = score_mean_planes(eng, natives, b, pool, 1)
    assert delta == (1, 0, 1, 0) and fused
    assert np.array_equal(bits(planes[:, :n]), bits(planes0[:, :n])) and np.array_equal(bits(mean), bits(mean0))
