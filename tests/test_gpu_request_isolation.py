"""A dispatch's request (csrc/fx_common.h FxRequest: layout, host rows, mean destination, launched-first part) does not outlive its
dispatch: the same five calls of one engine, made in the order a b c d e d c b a, give the second time the bits, the counter deltas
and the `fused_mean_done` they gave the first time -- whatever kind of request went before.  `np.array_equal` throughout, no tolerance.

  a  mean-only planes device call of 65 600 rows: the smallest round size above 4^8, so the table forms are asked for and, with the
     score tables on, the lookup kernel takes the mean
  b  the same rows as a row-major matrix device call
  c  get_fitness of 20 strings (explorer size: zero-copy, host rows)
  d  get_fitness of 16 400 strings, just above the 16 384 launched-first threshold
  e  d's strings with one character outside the alphabet: ValueError (a deferred error word, as test_gpu_launch_first.py raises it)"""
import numpy as np
import pytest

import flexs_amd
from flexs_amd import distributed as fd, synth
from flexs_amd.baselines import models as bm

from gpu_common import eng  # noqa: F401  (the module's engine: NaN-poisoned outputs, so an element no kernel wrote compares unequal)

pytestmark = pytest.mark.gpu

L, ALPHA, M = 8, "TGCA", 3
N_A, N_C, N_D = 65_600, 20, 16_400
READ_COUNTERS = ("conv1_table_launches", "conv2_prefix_launches", "pool_table_launches", "pool_table_builds", "score_table_launches",
                 "score_table_builds", "launch_first_calls", "launch_first_redone", "launch_relay_calls", "lp_armed_served")


def counters(e):
    c = e.counters()
    return tuple(c[k] for k in e.COUNTER_NAMES) + tuple(e.get_option(k) for k in READ_COUNTERS)


@pytest.mark.parametrize("tables", [1, 0], ids=["tables_on", "tables_off"])
def test_a_request_does_not_outlive_its_dispatch(eng, tables):  # noqa: F811
    import torch

    was = {k: eng.get_option(k) for k in ("cnn_pool_table", "cnn_score_table")}
    eng.set_option("cnn_pool_table", tables)      # 0: the conv forms and the separate mean kernel
    eng.set_option("cnn_score_table", tables)
    try:
        ens = flexs_amd.Ensemble([bm.CNN(L, 32, 100, ALPHA, seed=70 + m) for m in range(M)])
        natives, lut = [m.native() for m in ens.models], ens.models[0]._lut
        rows = synth.random_sequence_bytes(N_A, L, ALPHA, 11)
        few, many = synth.bytes_to_strings(rows[:N_C]), synth.bytes_to_strings(rows[N_C:N_C + N_D])
        broken = list(many)
        broken[N_D // 2] = "TGCAZGCA"
        stride = fd._stride_for(N_A)
        d_rows = torch.from_numpy(rows).cuda()
        planes, mean = torch.empty((M, stride), device="cuda"), torch.empty((N_A,), device="cuda")
        matrix = torch.empty((N_A, M), device="cuda")
        torch.cuda.synchronize()                  # (torch's stream is not the engine's: the upload has landed before a kernel reads it)

        def a():
            eng.score_mean_planes_dev(natives, d_rows.data_ptr(), N_A, L, lut, planes.data_ptr(), stride, mean.data_ptr())
            eng.sync()
            return np.concatenate([planes[:, :N_A].cpu().numpy().ravel(), mean.cpu().numpy()]), eng.get_option("fused_mean_done")

        def b():
            eng.score_dev(natives, d_rows.data_ptr(), N_A, L, lut, matrix.data_ptr(), None)
            eng.sync()
            return matrix.cpu().numpy(), None

        def c():
            return np.asarray(ens.get_fitness(few)).copy(), None

        def d():
            return np.asarray(ens.get_fitness(many)).copy(), None

        def e():
            with pytest.raises(ValueError):
                ens.get_fitness(broken)
            return None, None

        a()                                       # (builds the members' tables where they are on: both compared calls of `a` find them fresh)
        first = {}
        for name, call in (("a", a), ("b", b), ("c", c), ("d", d), ("e", e), ("d", d), ("c", c), ("b", b), ("a", a)):
            before = counters(eng)
            got, fused = call()
            delta = tuple(x - y for x, y in zip(counters(eng), before))
            if name == "e":
                continue
            assert not np.isnan(got).any(), f"{name}: {np.isnan(got).sum()} elements were never written"
            if name not in first:
                first[name] = (got, fused, delta)
                continue
            want, want_fused, want_delta = first[name]
            assert got.dtype == want.dtype and np.array_equal(got, want), f"{name}: the second call's bits differ from the first's"
            assert fused == want_fused, (name, fused, want_fused)
            assert delta == want_delta, (name, delta, want_delta)
        if tables:                                # (what `a` is there for: the lookup kernel wrote the mean; without tables the mean kernel did)
            assert first["a"][1] == 1
        else:
            assert first["a"][1] == 0
    finally:
        try:
            eng.sync()
        except ValueError:
            pass
        for k, v in was.items():
            eng.set_option(k, v)
