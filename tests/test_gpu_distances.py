"""Edit-distance kernels (K4: csrc/mindist.hip with csrc/myers.h, served through csrc/fx_nam.hip) on the device at every width,
boundary and path, bit for bit against the plain DP (oracle.c_oracle per pair, `ref_np.min_distance` for the selection rule).

Lengths: tests/distance_cases.py LENGTH_FORMS -- both sides of every boundary the launchers have, each with the instantiation it
reaches.  Content, built per length as queries and keys (distance_cases.build_case; proven against the DP on the host by
tests/test_pack_sim.py before a GPU sees it):
  1. unrelated random rows over 4 and over 20 letters (distances near L);
  2. one letter repeated in the query against another letter in the key (distance exactly L, every carry propagates);
  3. one letter repeated in the query against the same letter in a shorter NUL-padded key;
  4. a key that is the query shifted by one, two and three positions;
  5. near-copies with 1-5 edits exactly at bit 63 / bit 0 of a word (positions 63, 64, 127, 128, ... and L - 1);
  6. ragged rows: a query whose own length fills its last word inside a wider row, an empty query, an empty key, a query of
     the full row width against a key of length 1;
  7. the selection rule placed by hand (distance_cases.selection_case, L <= 65, more than two 1024-row chunks).
Every comparison is `array_equal` / `==`: the results are integers (and float64 sums of exact quotients in a fixed order)."""
import numpy as np
import pytest

from flexs_amd import _native

import distance_cases as dc
from gpu_common import eng  # noqa: F401  (the module-scoped engine fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture
def opts(eng):
    """Sets engine options for one test and puts every one of them back afterwards."""
    saved = {k: eng.get_option(k) for k in ("dist_stage", "dist_bounded", "zero_copy_bytes")}
    assert saved["dist_stage"] == 1 and saved["dist_bounded"] == 1, "an earlier test left a distance option changed"

    def set_(**kw):
        for k, v in kw.items():
            assert k in saved
            eng.set_option(k, v)

    try:
        yield set_
    finally:
        for k, v in saved.items():
            eng.set_option(k, v)


def _cache(eng, L, k_rows):
    """A device cache appended in two pieces."""
    c = _native.NativeCache(eng, L)
    cut = max(1, len(k_rows) // 3)
    c.append(k_rows[:cut]); c.append(k_rows[cut:])
    assert len(c) == len(k_rows)
    return c


def _want_min(dist):
    sel = [dc.select(row) for row in dist]
    return np.array([d for d, _ in sel], np.int32), np.array([i for _, i in sel], np.int64)


def _check_min_dist(eng, opts, L, q_rows, k_rows, dists, tile):
    """eng.min_dist and NativeCache.min_dist, both modes, dist_stage 1 and 0, the distinct queries (one pass per block) and the
    same queries tiled `tile` times (four passes per block when L <= 768)."""
    C, nq = len(k_rows), len(q_rows)
    cache = _cache(eng, L, k_rows)
    if L <= dc.MAX_L:
        assert dc.passes(C, nq) == 1 and dc.passes(C, nq * tile) == 4, "the sizes no longer select both forms of fx_dist_passes"
    for mode in (0, 1):
        d_want, a_want = _want_min(dists[mode])
        for stage in (1, 0):
            opts(dist_stage=stage)
            for rep in sorted({1, tile}):
                q = np.tile(q_rows, (rep, 1))
                dw, aw = np.tile(d_want, rep), np.tile(a_want, rep)
                for what, (d, a) in (("engine", eng.min_dist(q, k_rows, mode)), ("cache", cache.min_dist(q, mode))):
                    assert np.array_equal(d, dw) and np.array_equal(a, aw), (L, mode, stage, rep, what)


@pytest.mark.parametrize("L", dc.LENGTHS)
def test_min_dist_every_width_and_boundary(eng, opts, L):
    case = dc.reference(L)
    tile = -(-dc.FOUR_PASS_AT // len(case.queries)) if L <= dc.MAX_L else 2
    _check_min_dist(eng, opts, L, case.q_rows, case.k_rows, case.dist, tile)


@pytest.mark.parametrize("L", dc.LENGTHS)
def test_distance_matrix_every_width_and_boundary(eng, opts, L):
    """NativeCache.distances == min(DP, 255): k_distances<W> staged and unstaged, one and four passes; launch_long<true> past 768."""
    case = dc.reference(L)
    cache = _cache(eng, L, case.k_rows)
    nq = len(case.queries)
    tile = -(-dc.FOUR_PASS_AT // nq)
    for mode in (0, 1):
        want = np.minimum(case.dist[mode], 255).astype(np.uint8)
        if L >= 256:
            assert (case.dist[mode] > 255).any() and (case.dist[mode] < 255).any(), "the case must hold clamped and unclamped entries"
        for stage in (1, 0):
            opts(dist_stage=stage)
            assert np.array_equal(cache.distances(case.q_rows, mode), want), (L, mode, stage)
        if L <= dc.MAX_L:                                                 # the same rows, four passes per block
            assert dc.passes(len(case.keys), nq) == 1 and dc.passes(len(case.keys), nq * tile) == 4
            opts(dist_stage=1)
            assert np.array_equal(cache.distances(np.tile(case.q_rows, (tile, 1)), mode), np.tile(want, (tile, 1))), (L, mode, "x4")


DENSITY_LENGTHS = (14,) + tuple(L for L in dc.LENGTHS if L <= 769)


@pytest.mark.parametrize("L", DENSITY_LENGTHS)
def test_density_every_radius(eng, opts, L):
    """NativeCache.density against the Python loop of dyna_ppo.py:106-114 over the DP: radius 1-3 through k_distances_bounded<K>
    (staged up to 160 bytes, unstaged beyond), radius 4 and dist_bounded = 0 through the exact matrix, 769 through launch_long<true>."""
    case = dc.reference(L)
    cache = _cache(eng, L, case.k_rows)
    fitness = np.random.default_rng(L).random(len(case.keys))
    for mode in (0, 1):
        near = case.dist[mode][0]                                         # the parent: keys at distance exactly radius and radius + 1
        assert all((near == d).any() for d in (1, 2, 3, 4, 5)), (L, mode)
        for radius in (1, 2, 3, 4):
            want = [dc.density(row, fitness, radius) for row in case.dist[mode]]
            for bounded in (1, 0):
                for stage in (1, 0):
                    opts(dist_bounded=bounded, dist_stage=stage)
                    dens, cnt = cache.density(case.q_rows, fitness, radius, mode)
                    assert [(float(x), int(n)) for x, n in zip(dens, cnt)] == want, (L, mode, radius, bounded, stage)


@pytest.mark.parametrize("L", (32, 33, 64, 65))
def test_selection_rule_placed_by_hand(eng, opts, L):
    """noisy_abstract_model.py:50-58: the FIRST key at distance 1 wins even when an exact hit comes earlier (the `d == 1 -> 0`
    remap of the 64-bit key), otherwise the first strict minimum -- across a 256-row block, across a 1024-row chunk, in the
    one-pass and in the four-pass form."""
    queries, keys, expected, what = dc.selection_case(L)
    q_rows, k_rows = dc.rows(queries, L), dc.rows(keys, L)
    dists = dc.dp_matrices(queries, keys, L)
    for mode in (0, 1):
        got = [dc.select(row) for row in dists[mode]]
        assert got == expected, [w for w, g, e in zip(what, got, expected) if g != e]     # the DP agrees with the placement
    assert len(keys) > 2 * dc.CHUNK
    _check_min_dist(eng, opts, L, q_rows, k_rows, dists, tile=-(-dc.FOUR_PASS_AT // (3 * len(queries))))


@pytest.mark.parametrize("L", (1536, 1537))
def test_strip_form_more_than_one_pass_of_256_rows(eng, opts, L):
    """k_min_dist_long over more than 256 keys (the same rows repeated: one DP per distinct pair): the block's second pass.  The
    three multi-strip queries of the case nine times over: a period of 3 puts blocks of different queries behind the same L2 (the
    device deals workgroups round its 8 XCDs), where a slip in the indexing of the strip boundary scratch can show."""
    case = dc.reference(L)
    rep = 11
    k_rows = np.tile(case.k_rows, (rep, 1))
    assert 256 < len(k_rows) <= dc.CHUNK
    assert all(len(q) > dc.MAX_L for q in case.queries[:3])
    q_rows = np.tile(case.q_rows[:3], (9, 1))
    dists = tuple(np.tile(d[:3], (9, rep)) for d in case.dist)
    _check_min_dist(eng, opts, L, q_rows, k_rows, dists, tile=1)
    cache = _cache(eng, L, k_rows)
    for mode in (0, 1):
        assert np.array_equal(cache.distances(q_rows, mode), np.minimum(dists[mode], 255).astype(np.uint8)), (L, mode)


# ------------------------------------------------------------------ the host paths around the kernels (fx_nam.hip)
def test_distances_copy_loop_beyond_zero_copy_bytes(eng, opts):
    """cache_distances: queries plus matrix beyond `zero_copy_bytes` take device scratch and copies instead of mapped memory."""
    L = 33
    case = dc.reference(L)
    cache = _cache(eng, L, case.k_rows)
    zc_default = eng.get_option("zero_copy_bytes")
    assert zc_default >= case.q_rows.size + len(case.queries) * len(case.keys) > 1024
    for mode in (0, 1):
        want = np.minimum(case.dist[mode], 255).astype(np.uint8)
        default = cache.distances(case.q_rows, mode)
        opts(zero_copy_bytes=1024)
        copied = cache.distances(case.q_rows, mode)
        opts(zero_copy_bytes=zc_default)
        assert np.array_equal(default, want) and np.array_equal(copied, want), mode


def test_density_in_several_query_blocks(eng, opts):
    """fx_cache_density walks the queries in blocks whose distance rows fit `zero_copy_bytes`: a last partial block, and a block of
    one query whose rows no longer fit (the copy loop with the exact matrix)."""
    L = 33
    case = dc.reference(L)
    cache = _cache(eng, L, case.k_rows)
    fitness = np.random.default_rng(5).random(len(case.keys))
    per_query = len(case.keys) + L                                        # fx_cache_density: queries per block = zero_copy_bytes / (C + L)
    nq = len(case.queries)
    zc_default = eng.get_option("zero_copy_bytes")
    assert zc_default // per_query >= nq == 8
    for radius in (2, 4):
        want = [dc.density(row, fitness, radius) for row in case.dist[0]]
        results = []
        for zc in (zc_default, 3 * per_query, per_query - 1):              # one block; 3 + 3 + 2 queries; 8 x 1
            opts(zero_copy_bytes=zc)
            dens, cnt = cache.density(case.q_rows, fitness, radius)
            results.append([(float(x), int(n)) for x, n in zip(dens, cnt)])
        opts(zero_copy_bytes=zc_default)
        assert results == [want] * 3, radius
    # the default option with more queries than one block holds
    q = np.tile(case.q_rows, (zc_default // per_query // nq + 1, 1))
    assert zc_default // per_query < len(q) < 2 * (zc_default // per_query)
    dens, cnt = cache.density(q, fitness, 2)
    want = [dc.density(row, fitness, 2) for row in case.dist[0]]
    assert [(float(x), int(n)) for x, n in zip(dens, cnt)] == want * (len(q) // nq)


def test_long_rows_query_batch_split(eng, opts):
    """launch_long keeps its boundary scratch below 256 MiB by launching the queries in batches: at L = 769 and one chunk of keys a
    batch is 1363 queries.  Three queries of the case (two of two strips, one of one) repeated past that, against the first keys
    of the case: `q0 > 0` in k_min_dist_long<false> and <true>.  (A period of 3: see test_strip_form_more_than_one_pass_of_256_rows.)"""
    L = 769
    case = dc.reference(L)
    C, nq, rep = 6, 3, 467
    k_rows, q_rows = case.k_rows[:C], case.q_rows[:nq]
    Q = rep * nq
    assert dc.long_query_batch(C, L, Q) < Q < 2 * dc.long_query_batch(C, L, Q)
    q = np.tile(q_rows, (rep, 1))
    cache = _cache(eng, L, k_rows)
    for mode in (0, 1):
        dist = case.dist[mode][:nq, :C]
        d_want, a_want = _want_min(dist)
        few = cache.min_dist(q_rows, mode)                               # one batch
        assert np.array_equal(few[0], d_want) and np.array_equal(few[1], a_want), mode
        d, a = cache.min_dist(q, mode)
        assert np.array_equal(d, np.tile(d_want, rep)) and np.array_equal(a, np.tile(a_want, rep)), mode
        assert np.array_equal(cache.distances(q, mode), np.tile(np.minimum(dist, 255).astype(np.uint8), (rep, 1))), mode
