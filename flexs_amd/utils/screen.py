"""Screening: score a batch -- or the model's whole sequence space, or the mutant neighbourhoods of a few parents -- and keep the
best few.

Every consumer of `get_fitness` in the reference ends with `np.argsort(preds)[: -batch : -1]` (adalead.py:173, cmaes.py:120,
cbas_dbas.py:199, random.py:84, genetic_algorithm.py:151).  `screen` / `screen_all` / `screen_mutants` do both steps; for device surrogates
(`KerasModel`, and `Ensemble` of them with the default mean) the scores stay on the GPU and only the k winners come back
(fx_score_topk / fx_screen_all / fx_screen_mutants, include/flexs_amd.h).  Anything else -- foreign `flexs.Model`s, a custom `combine_with`,
`NoisyAbstractModel`, no GPU -- goes through `get_fitness` and `host_top_k`.  ONE ordering rule everywhere:

  the min(k, N) best entries, best first; value order is NumPy's sort order read from the top (NaN above +inf, -0.0 == +0.0,
  denormals keep their own rank); among equal values the lower index wins and comes first; 1 <= k <= 4096.
"""
import itertools
from typing import List, Optional, Tuple

import numpy as np

from flexs_amd import _native

MAX_K = _native.SMALL_CALL_ROWS          # 4096
HOST_ENUMERATION_LIMIT = 1 << 24         # `screen_all` without the device path builds every string on the host: refuse more


def _check_k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError("k must be an integer")
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be 1 .. {MAX_K}, got {k}")
    return int(k)


def host_top_k(scores, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """The rule above in plain NumPy: (idx int64, scores[idx]).  Three sort keys, least significant first: the index, the
    negated value (NaNs replaced: they are ranked by the third key; -(+0.0) == -(-0.0) compare equal), "is not NaN"."""
    k = _check_k(k)
    x = np.asarray(scores).reshape(-1)
    v = x if x.dtype.kind == "f" else x.astype(np.float64)
    nan = np.isnan(v)
    order = np.lexsort((np.arange(v.size), -np.where(nan, 0, v), ~nan))[:min(k, v.size)].astype(np.int64)
    return order, x[order]


def _device_plan(model):
    """(engine, fx_models, L, alphabet, lut, models to charge) when `model` is scored by the fused device path, else None."""
    from flexs_amd.baselines.models.keras_model import KerasModel
    from flexs_amd.ensemble import Ensemble, _default_combine, _device_members

    if _native.lib().fx_device_count() < 1:
        return None
    if isinstance(model, KerasModel) and type(model)._fitness_function is KerasModel._fitness_function:
        return model._engine(), [model], model.model.L, model.alphabet, model._lut, [model]
    if (isinstance(model, Ensemble) and type(model)._fitness_function is Ensemble._fitness_function
            and model.combine_with is _default_combine and _device_members(model.models)
            and all(type(m)._fitness_function is KerasModel._fitness_function for m in model.models)):
        m0 = model.models[0]
        return m0._engine(), list(model.models), m0.model.L, m0.alphabet, m0._lut, [model] + list(model.models)
    return None


def screen(model, sequences, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """The k best of `sequences` under `model`: (positions in `sequences`, their scores), best first.  Charges `cost` as
    `model.get_fitness(sequences)` does (the model, and every member of an ensemble, by len(sequences))."""
    k = _check_k(k)
    plan = _device_plan(model)
    if plan is None:
        return host_top_k(model.get_fitness(sequences), k)
    engine, members, L, _, lut, charged = plan
    n = len(sequences)
    for m in charged:                                       # (before anything can raise, as the reference does: landscape.py:44)
        m.cost = m.cost + n
    seq_bytes = _native.sequences_to_bytes(sequences, L=L, staging=engine)
    if seq_bytes.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    return engine.score_topk([m.native() for m in members], seq_bytes, lut, k)


def _space_of(model, alphabet: Optional[str], seq_len: Optional[int]) -> Tuple[str, int]:
    for m in (model, *getattr(model, "models", ())):
        if alphabet is None:
            alphabet = getattr(m, "alphabet", None)
        if seq_len is None:
            seq_len = getattr(m, "seq_len", None)
    if alphabet is None or seq_len is None:
        raise ValueError("screen_all needs the model's alphabet and seq_len (pass alphabet=..., seq_len=...)")
    return alphabet, int(seq_len)


def screen_all(model, k: int, alphabet: Optional[str] = None, seq_len: Optional[int] = None) -> Tuple[List[str], np.ndarray]:
    """The model's optimum set: the k best of ALL len(alphabet) ** seq_len sequences, in the order of
    itertools.product(alphabet, repeat=seq_len) where scores tie: (sequences, scores), best first.  Device surrogates enumerate
    on the GPU (no string is built for a loser); every other model is asked through `get_fitness` about strings built here,
    which is refused beyond 2^24 sequences.  Charges `cost` by the size of the space."""
    k = _check_k(k)
    plan = _device_plan(model)
    if plan is not None:
        engine, members, L, alphabet, lut, charged = plan
        total = len(alphabet) ** L
        if total > 2 ** 31 - 1:
            raise ValueError(f"the sequence space ({len(alphabet)} ** {L}) has more than 2^31 - 1 rows")
        for m in charged:
            m.cost = m.cost + total
        _, rows, val = engine.screen_all([m.native() for m in members], L, alphabet, lut, k)
        return [r.tobytes().decode("latin-1") for r in rows], val
    alphabet, seq_len = _space_of(model, alphabet, seq_len)
    if len(alphabet) ** seq_len > HOST_ENUMERATION_LIMIT:
        raise ValueError(f"the sequence space ({len(alphabet)} ** {seq_len}) is too large to enumerate on the host (limit 2^24)")
    seqs = ["".join(p) for p in itertools.product(alphabet, repeat=seq_len)]
    idx, val = host_top_k(model.get_fitness(seqs), k)
    return [seqs[i] for i in idx], val


def mutant_ball(parent: str, alphabet: str, radius: int):
    """`parent`, then its single mutants, then (radius 2) its double mutants: positions in the order of
    itertools.combinations, letters in alphabet order with the parent's own letter skipped, the later position fastest.  This
    is the row order of `screen_mutants` and of fx_screen_mutants (csrc/mutant_rank.h)."""
    if radius not in (1, 2):
        raise ValueError(f"radius must be 1 or 2, got {radius}")
    yield parent
    for d in range(1, radius + 1):
        for pos in itertools.combinations(range(len(parent)), d):
            for letters in itertools.product(*[[c for c in alphabet if c != parent[p]] for p in pos]):
                t = list(parent)
                for p, c in zip(pos, letters):
                    t[p] = c
                yield "".join(t)


def mutant_ball_size(seq_len: int, alphabet_size: int, radius: int) -> int:
    """Rows of `mutant_ball`: 1 + L (A - 1), plus C(L, 2) (A - 1)^2 for radius 2."""
    if radius not in (1, 2):
        raise ValueError(f"radius must be 1 or 2, got {radius}")
    L, a1 = int(seq_len), int(alphabet_size) - 1
    return 1 + L * a1 + (L * (L - 1) // 2 * a1 * a1 if radius == 2 else 0)


def screen_mutants(model, parents, k: int, radius: int = 1,
                   alphabet: Optional[str] = None) -> Tuple[List[str], np.ndarray, np.ndarray]:
    """The k best among `parents` and all their mutants within Hamming distance `radius` (1 or 2): (sequences, scores,
    parent_index int64), best first.  Row `parent_number * B + i` is entry i of `mutant_ball(parent, alphabet, radius)`, B its
    size; duplicates (across parents, or a parent listed twice) are kept and tie in favour of the lower row.  Device surrogates
    get the P x L parent bytes only and write, score and select every row on the GPU (P * B <= 2^31 - 1); every other model is
    asked through `get_fitness` about strings built here, which is refused beyond 2^24 rows.  Charges `cost` by P * B."""
    k = _check_k(k)
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or radius not in (1, 2):
        raise ValueError(f"radius must be 1 or 2, got {radius!r}")
    radius = int(radius)
    parents = [parents] if isinstance(parents, str) else list(parents)
    if not parents:
        raise ValueError("screen_mutants needs at least one parent")
    plan = _device_plan(model)
    if plan is not None:
        engine, members, L, alphabet, lut, charged = plan
        ball = mutant_ball_size(L, len(alphabet), radius)
        total = len(parents) * ball
        if total > 2 ** 31 - 1:
            raise ValueError(f"{len(parents)} parents x {ball} mutants each are more than 2^31 - 1 rows")
        for m in charged:                                   # (before a bad parent can raise, as `screen` does)
            m.cost = m.cost + total
        parent_bytes = _native.sequences_to_bytes(parents, L=L)     # (ValueError for a parent of another length)
        idx, rows, val = engine.screen_mutants([m.native() for m in members], parent_bytes, alphabet, lut, radius, k)
        return [r.tobytes().decode("latin-1") for r in rows], val, idx // ball
    seq_len = next((m.seq_len for m in (model, *getattr(model, "models", ())) if getattr(m, "seq_len", None) is not None), len(parents[0]))
    alphabet, seq_len = _space_of(model, alphabet, seq_len)
    ball = mutant_ball_size(seq_len, len(alphabet), radius)
    total = len(parents) * ball
    if total > HOST_ENUMERATION_LIMIT:
        raise ValueError(f"{len(parents)} parents x {ball} mutants each are too many rows to enumerate on the host (limit 2^24)")
    bad = [p for p in parents if len(p) != seq_len or any(c not in alphabet for c in p)]
    if bad:                                                 # charged as the device path charges, then refused
        for m in (model, *getattr(model, "models", ())):
            m.cost = m.cost + total
        raise ValueError(f"parent {bad[0]!r} has not the length {seq_len} or a letter outside {alphabet!r}")
    seqs = [s for p in parents for s in mutant_ball(p, alphabet, radius)]
    idx, val = host_top_k(model.get_fitness(seqs), k)
    return [seqs[i] for i in idx], val, idx // ball
