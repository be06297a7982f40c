"""Mutant-neighbourhood screening on the device (`model.screen_mutants`, fx_screen_mutants): the parents go up, every single and
double mutant is written, scored and selected on the GPU.  Oracle: `host_top_k(model.get_fitness(strings), k)` of THE SAME model
over ball strings built here by the definition -- sequences by equality, scores by their bits, `parent_index == idx // B`, and
the read-only counter `mutant_rows_enumerated` grows by exactly P * B per call."""
import ctypes as C
import itertools

import numpy as np
import pytest

import flexs_amd
from flexs_amd import _native, synth
from flexs_amd.baselines import models as bm
from flexs_amd.utils.screen import host_top_k
from oracle import ref_np

from gpu_common import eng  # noqa: F401  (the module's engine fixture)
from screen_common import bits

pytestmark = pytest.mark.gpu

PROTEIN = "ACDEFGHIKLMNPQRSTVWY"
KS = (1, 100, 1999)


@pytest.fixture()
def shipped(eng):
    keys = ("screen_chunk_rows", "topk_small_rows", "cnn_pool_table")
    keep = {k: eng.get_option(k) for k in keys}
    try:
        yield eng
    finally:
        for k, v in keep.items():
            eng.set_option(k, v)


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


def cnn(L, alphabet, seed):
    m = bm.CNN(L, 32, 100, alphabet)
    m.model.set_weights(ref_np.synth_weights(ref_np.cnn_shapes(L, len(alphabet), 32, 100, 5), seed))
    return m


def cnn_ensemble(L=8, alphabet="TGCA", members=3, seed=1000):
    return flexs_amd.Ensemble([cnn(L, alphabet, seed + m) for m in range(members)])


def mlp(L, alphabet, seed=2000):
    m = bm.MLP(L, 100, alphabet)
    m.model.set_weights(ref_np.synth_weights(ref_np.mlp_shapes(L, len(alphabet), 100), seed))
    return m


def random_parents(P, L, alphabet, seed):
    return synth.bytes_to_strings(synth.random_sequence_bytes(P, L, alphabet, seed))


def members_of(model):
    return list(getattr(model, "models", [])) or [model]


def reset_costs(model):
    for m in [model] + members_of(model):
        m.cost = 0


class Case:
    """A model, its parents, the host-built rows and the model's own scores of them: computed once, never changed."""

    def __init__(self, model, parents, alphabet, radius):
        self.model, self.parents, self.alphabet, self.radius = model, list(parents), alphabet, radius
        self.L = len(parents[0])
        self.B = ball_size(self.L, len(alphabet), radius)
        self.seqs = [s for p in parents for s in ball(p, alphabet, radius)]
        assert len(self.seqs) == len(parents) * self.B
        self.scores = model.get_fitness(self.seqs)
        self.scores.setflags(write=False)
        self.engine = members_of(model)[0]._engine()

    def check(self, ks, large_expected=None):
        total = len(self.seqs)
        natives = [m.native() for m in members_of(self.model)]
        lut = members_of(self.model)[0]._lut
        out = None
        for k in ks:
            reset_costs(self.model)
            rows_before = self.engine.get_option("mutant_rows_enumerated")
            large_before = self.engine.get_option("topk_large_launches")
            got_seqs, got_val, parent_index = self.model.screen_mutants(self.parents, k, self.radius)
            assert self.engine.get_option("mutant_rows_enumerated") - rows_before == total
            if large_expected is not None:
                assert self.engine.get_option("topk_large_launches") - large_before == large_expected
            assert self.model.cost == total and all(m.cost == total for m in members_of(self.model))
            w_idx, w_val = host_top_k(self.scores, k)
            assert got_seqs == [self.seqs[i] for i in w_idx], k
            assert got_val.dtype == np.float32 and np.array_equal(bits(got_val), bits(w_val)), k
            assert parent_index.dtype == np.int64 and np.array_equal(parent_index, w_idx // self.B), k
            idx, rows, val = self.engine.screen_mutants(natives, _native.sequences_to_bytes(self.parents), self.alphabet, lut, self.radius, k)
            assert np.array_equal(idx, w_idx) and np.array_equal(bits(val), bits(w_val))
            assert synth.bytes_to_strings(rows) == got_seqs
            out = (got_seqs, got_val, parent_index)
        return out


_first = {}


def first_case():
    """3 x CNN, L = 8, "TGCA", radius 2, 5 random parents: 5 x 277 = 1385 rows."""
    if "case" not in _first:
        _first["case"] = Case(cnn_ensemble(), random_parents(5, 8, "TGCA", 90), "TGCA", 2)
        assert len(_first["case"].seqs) == 1385
    return _first["case"]


def test_cnn_ensemble_chunks_and_pool_table(shipped):
    case = first_case()
    assert shipped.get_option("screen_chunk_rows") == 1 << 22
    results = {}
    for pool in (1, 0):
        shipped.set_option("cnn_pool_table", pool)
        shipped.set_option("screen_chunk_rows", 1 << 22)
        case.check(KS)
        shipped.set_option("screen_chunk_rows", 304)        # 5 chunks: borders inside balls (277 rows) and between parents
        results[pool] = case.check(KS)
    assert results[0][0] == results[1][0] and np.array_equal(bits(results[0][1]), bits(results[1][1]))


@pytest.mark.parametrize("L", [5, 1])
def test_mlp_short_rows(shipped, L):
    """L no multiple of 4, several rows per 16-byte store, rows that straddle every store; L = 1 has no pairs (B = 4)."""
    shipped.set_option("screen_chunk_rows", 16)
    case = Case(mlp(L, "UGCA", seed=2200 + L), random_parents(3, L, "UGCA", 91), "UGCA", 2)
    assert case.B == (106 if L == 5 else 4)
    case.check((1, 7, 100, 1999))


def test_mlp_protein_radix_select_partial_last_chunk(shipped):
    shipped.set_option("screen_chunk_rows", 65536)
    case = Case(mlp(30, PROTEIN, seed=2300), random_parents(1, 30, PROTEIN, 92), PROTEIN, 2)
    assert len(case.seqs) == 157606 and 157606 % 65536 != 0
    case.check((1999,), large_expected=3)                   # every chunk (65536, 65536, 26534 rows) through the radix select


def test_cnn_protein_length_odd_rows(shipped):
    case = Case(cnn(237, PROTEIN, 1100), random_parents(2, 237, PROTEIN, 93), PROTEIN, 1)
    assert len(case.seqs) == 9008
    case.check((100,))


def tie_parents():
    s = random_parents(1, 8, "TGCA", 105)[0]               # (a seed for which test_ties_between_parents' cut of k = 101 separates two copies)
    t = s[:3] + ("G" if s[3] != "G" else "C") + s[4:]
    return [s, s, t]


def test_tie_structure_of_the_inputs():
    """No model: the same parent twice, and a third at Hamming distance 1.  Every row of ball 0 has its copy at the same place of
    ball 1; the third ball shares rows with them (at other places) and has rows of its own."""
    parents = tie_parents()
    balls = [list(ball(p, "TGCA", 2)) for p in parents]
    assert sum(a != b for a, b in zip(parents[0], parents[2])) == 1
    assert balls[0] == balls[1] and len(balls[0]) == len(set(balls[0])) == 277
    shared = set(balls[0]) & set(balls[2])
    assert 0 < len(shared) < 277 and set(balls[2]) - set(balls[0])
    counts = {}
    for b in balls:
        for s in b:
            counts[s] = counts.get(s, 0) + 1
    assert sorted(set(counts.values())) == [1, 2, 3]        # own rows of the third parent, pairs, triples


def test_ties_between_parents(shipped):
    shipped.set_option("screen_chunk_rows", 304)
    case = Case(cnn_ensemble(seed=1200), tie_parents(), "TGCA", 2)
    ranked = host_top_k(case.scores, 831)[0]
    assert case.seqs[ranked[100]] == case.seqs[ranked[101]]            # the cut of k = 101 falls between two copies of one sequence:
    assert ranked[100] // 277 == 0 and ranked[101] // 277 == 1         # parent 0's is kept, parent 1's is not
    assert bits(case.scores[ranked[100:102]])[0] == bits(case.scores[ranked[100:102]])[1]
    for k in (101, 831):
        seqs, val, parent_index = case.check((k,))
        seen = {}
        for rank, (s, p) in enumerate(zip(seqs, parent_index)):
            seen.setdefault(s, []).append((int(p), rank))
        for s, where in seen.items():                                   # copies are adjacent, the lower parent first
            assert [p for p, _ in where] == sorted(p for p, _ in where)
            assert [r for _, r in where] == list(range(where[0][1], where[0][1] + len(where)))
        from_0 = {s for s, p in zip(seqs, parent_index) if p == 0}
        from_1 = {s for s, p in zip(seqs, parent_index) if p == 1}
        assert from_1 <= from_0
        if k == 101:
            assert len(from_0 - from_1) == 1 and seqs[-1] in from_0 - from_1 and parent_index[-1] == 0
        else:
            assert from_0 == from_1


def test_errors_and_raw_abi(shipped):
    case = first_case()
    want = case.check((100,))
    ens = case.model
    # a foreign letter in a parent: ValueError after charging
    bad = list(case.parents)
    bad[3] = bad[3][:5] + "N" + bad[3][6:]
    for model in (ens, ens.models[0]):
        reset_costs(ens)
        with pytest.raises(ValueError):
            model.screen_mutants(bad, 100, 2)
        assert model.cost == 1385
        if model is ens:
            assert all(m.cost == 1385 for m in ens.models)
    reset_costs(ens)
    with pytest.raises(ValueError):                                     # a parent of another length: charged, then refused
        ens.screen_mutants(case.parents[:2] + ["TGCATGC"], 100, 1)
    assert ens.cost == 3 * 25
    # limits: refused before anything is charged
    reset_costs(ens)
    for k in (0, 4097):
        with pytest.raises(ValueError):
            ens.screen_mutants(case.parents, k, 2)
    for radius in (0, 3):
        with pytest.raises(ValueError):
            ens.screen_mutants(case.parents, 10, radius)
    with pytest.raises(ValueError):
        ens.screen_mutants([], 10, 2)
    assert ens.cost == 0 and all(m.cost == 0 for m in ens.models)
    gfp = cnn(237, PROTEIN, 1100)
    assert 212 * ball_size(237, 20, 2) <= 2 ** 31 - 1 < 213 * ball_size(237, 20, 2)
    with pytest.raises(ValueError):
        gfp.screen_mutants(random_parents(213, 237, PROTEIN, 95), 10, 2)
    assert gfp.cost == 0
    # the raw entry point: FX_EBADCHAR before any launch, nothing written; FX_ESHAPE for the sizes
    natives = [m.native() for m in ens.models]
    arr = (C.c_void_p * 3)(*[m.handle for m in natives])
    lut = ens.models[0]._lut
    al = np.frombuffer(b"TGCA", np.uint8).copy()

    def raw(parents, radius, k, A=4):
        b = _native.sequences_to_bytes(parents)
        idx = np.full(100, -1, np.int64)
        rows = np.full((100, 8), 7, np.uint8)
        val = np.full(100, np.nan, np.float32)
        n = C.c_int(-5)
        before = shipped.get_option("mutant_rows_enumerated")
        rc = shipped._lib.fx_screen_mutants(shipped.handle, arr, 3, _native._ptr(b), b.shape[0], 8, A, _native._ptr(al), _native._lut_ptr(lut),
                                            radius, k, _native._ptr(idx), _native._ptr(rows), _native._ptr(val), C.byref(n))
        untouched = (idx == -1).all() and (rows == 7).all() and np.isnan(val).all() and n.value == -5
        return rc, untouched, shipped.get_option("mutant_rows_enumerated") - before, (idx, rows, val, n.value)

    assert raw(bad, 2, 100)[:3] == (_native.FX_EBADCHAR, True, 0)
    for args in ((case.parents, 0, 100), (case.parents, 3, 100), (case.parents, 2, 0), (case.parents, 2, 4097)):
        assert raw(*args)[:3] == (_native.FX_ESHAPE, True, 0), args
    assert raw(case.parents, 2, 100, A=3)[:3] == (_native.FX_ESHAPE, True, 0)
    rc, untouched, grew, (idx, rows, val, n) = raw(case.parents, 2, 100)
    assert rc == _native.FX_OK and not untouched and grew == 1385 and n == 100
    # ... and the engine answers the first case with the same bits
    assert synth.bytes_to_strings(rows) == want[0] and np.array_equal(bits(val), bits(want[1])) and np.array_equal(idx // 277, want[2])
    again = case.check((100,))
    assert again[0] == want[0] and np.array_equal(bits(again[1]), bits(want[1])) and np.array_equal(again[2], want[2])
