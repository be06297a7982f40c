"""The prepared step (`fx_step_create` / `fx_step_launch`, csrc/fx_step.hip; `_native.NativeStep`; engine option `step_call`): one resident
scoring step of `DistributedEnsemble.launch` issued through one short native call.  The step calls the planner the direct calls call, so the
yardstick is `np.array_equal` against `score_mean_planes_dev` / `score_planes_dev` on fresh buffers -- scores, mean, the untouched padding, the
engine's counters and `fused_mean_done` -- never a tolerance.

The lookup form (k_score_cnn_mfma_scoretab: 256 threads, one row each) is put on small launches the way test_gpu_score_table.py does:
`cnn_big_units` = 0, `cnn_quad` = 0, `cnn_pool_table` = 2, rows in device memory."""
import numpy as np
import pytest

from flexs_amd import _native, distributed as fd, synth
from flexs_amd.baselines import models as bm
from oracle import ref_np

from gpu_common import make_native

pytestmark = pytest.mark.gpu

L8, ALPHA, F, H, K = 8, "TGCA", 32, 100, 5
AAS = "ILVAGMFYWEDQNHCRKSTP"
LUT = _native.make_lut(ALPHA)
LUT_AA = _native.make_lut(AAS)
FILL = -7.0                     # what the buffers hold before a call: an element equal to it afterwards was not written
OPTION_COUNTERS = ("pool_table_launches", "pool_table_builds", "score_table_launches", "score_table_builds")
LOOKUP_NS = (1, 255, 256, 257, 1000)


@pytest.fixture()
def eng():
    """The engine without NaN poisoning (the padding must stay what it was), the lookup form reachable by small launches."""
    e = _native.Engine.get(0)
    keys = ("poison_outputs", "cnn_big_units", "cnn_quad", "cnn_pool_table", "cnn_score_table", "step_call")
    was = {k: e.get_option(k) for k in keys}
    e.set_option("poison_outputs", 0)
    e.set_option("cnn_big_units", 0)
    e.set_option("cnn_quad", 0)
    e.set_option("cnn_pool_table", 2)
    try:
        yield e
    finally:
        try:
            e.sync()
        except ValueError:
            pass
        for k, v in was.items():
            e.set_option(k, v)


def counters(e):
    c = e.counters()
    return np.array([c["device_calls"], c["sequences"], c["forwards"]] + [e.get_option(k) for k in OPTION_COUNTERS])


def dev(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()               # (torch's stream is not the engine's: the upload has landed before a kernel reads it)
    return t


def buffers(M, stride, n):
    import torch

    out = (torch.full((M, stride), FILL, device="cuda"), torch.full((max(n, 1),), FILL, device="cuda"))
    torch.cuda.synchronize()               # (... and the fills, before a kernel of the engine's stream writes there)
    return out


def refill(*tensors, value=FILL):
    import torch

    for t in tensors:
        t.fill_(value)
    torch.cuda.synchronize()


def read(ens, t):
    """A result of `finish` on the host: the engine's stream first (torch's default stream does not wait for it)."""
    ens.stream.synchronize()
    return t.cpu().numpy()


def direct(e, natives, d_in, n, L, lut, stride, mean=True):
    """planes, mean (or None), counter deltas, fused_mean_done of the direct call on fresh buffers."""
    planes, mu = buffers(len(natives), stride, n)
    before = counters(e)
    if mean:
        e.score_mean_planes_dev(natives, d_in.data_ptr(), n, L, lut, planes.data_ptr(), stride, mu.data_ptr())
    else:
        e.score_planes_dev(natives, d_in.data_ptr(), n, L, lut, planes.data_ptr(), stride)
    e.sync()
    return planes.cpu().numpy(), mu.cpu().numpy() if mean else None, tuple(counters(e) - before), e.get_option("fused_mean_done")


def stepped(e, natives, d_in, n, L, lut, stride, mean=True, step=None, bufs=None):
    """The same through a prepared step (a fresh one on fresh buffers unless given)."""
    planes, mu = bufs or buffers(len(natives), stride, n)
    if step is None:
        step = _native.NativeStep(e, natives, L, lut, planes.data_ptr(), stride, mu.data_ptr() if mean else None, None)
    before = counters(e)
    step.launch(d_in.data_ptr(), n)
    e.sync()
    return planes.cpu().numpy(), mu.cpu().numpy() if mean else None, tuple(counters(e) - before), e.get_option("fused_mean_done")


def cnn8(e, count=3, seed=4100):
    return [make_native(e, "cnn", L8, 4, H, F, K, seed=seed + m)[0] for m in range(count)]


# ------------------------------------------------------------------ the lookup form
def test_lookup_form_edges_of_the_workgroup(eng):
    natives = cnn8(eng)
    rows = synth.random_sequence_bytes(1000, L8, ALPHA, 7)
    d_all = dev(rows)
    direct(eng, natives, d_all, 1000, L8, LUT, fd._stride_for(1000))          # (builds the members' tables once)
    big = fd._stride_for(1000)
    shared_bufs = buffers(3, big, 1000)
    shared = _native.NativeStep(eng, natives, L8, LUT, shared_bufs[0].data_ptr(), big, shared_bufs[1].data_ptr(), None)
    for n in LOOKUP_NS:
        stride = fd._stride_for(n)
        d_in = dev(rows[:n])
        want_p, want_m, want_c, want_f = direct(eng, natives, d_in, n, L8, LUT, stride)
        assert want_c[0] == 1 and want_c[1] == n and want_c[2] == 3 * n and want_c[5] == 1, want_c     # one device call, answered by the lookup kernel
        assert not (want_p[:, :n] == FILL).any() and not (want_m[:n] == FILL).any()
        got_p, got_m, got_c, got_f = stepped(eng, natives, d_in, n, L8, LUT, stride)
        assert np.array_equal(got_p[:, :n], want_p[:, :n]) and np.array_equal(got_m[:n], want_m[:n]), n
        assert (got_p[:, n:] == FILL).all() and (want_p[:, n:] == FILL).all(), f"N = {n}: the padding was written"
        assert got_c == want_c and got_f == want_f == 1, (n, got_c, want_c, got_f, want_f)
        # ... and ONE step, created for the largest stride, launched with every N in turn
        refill(*shared_bufs)
        sh_p, sh_m, sh_c, _ = stepped(eng, natives, d_in, n, L8, LUT, big, step=shared, bufs=shared_bufs)
        assert np.array_equal(sh_p[:, :n], want_p[:, :n]) and np.array_equal(sh_m[:n], want_m[:n]) and sh_c == want_c, n
        assert (sh_p[:, n:] == FILL).all() and (sh_m[n:] == FILL).all(), n


def test_null_mean_equals_score_planes(eng):
    natives = cnn8(eng, seed=4200)
    n, stride = 257, fd._stride_for(257)
    d_in = dev(synth.random_sequence_bytes(n, L8, ALPHA, 8))
    direct(eng, natives, d_in, n, L8, LUT, stride, mean=False)
    want_p, _, want_c, _ = direct(eng, natives, d_in, n, L8, LUT, stride, mean=False)
    got_p, _, got_c, _ = stepped(eng, natives, d_in, n, L8, LUT, stride, mean=False)
    assert np.array_equal(got_p, want_p) and got_c == want_c
    assert not (got_p[:, :n] == FILL).any() and (got_p[:, n:] == FILL).all()


def test_zero_rows_enqueue_only_the_error_word(eng):
    import torch

    natives = cnn8(eng, seed=4250)
    planes, mu = buffers(3, 64, 1)
    word = torch.full((1,), FILL, device="cuda")
    torch.cuda.synchronize()
    step = _native.NativeStep(eng, natives, L8, LUT, planes.data_ptr(), 64, mu.data_ptr(), word.data_ptr())
    before = counters(eng)
    step.launch(0, 0)
    eng.sync()
    assert tuple(counters(eng) - before) == (0,) * 7
    assert (planes.cpu().numpy() == FILL).all() and float(word.cpu()[0]) == 0.0
    with pytest.raises(_native.FxError):
        step.launch(planes.data_ptr(), 65)                                      # more rows than the stride


# ------------------------------------------------------------------ the other forms
@pytest.mark.parametrize("kind,L,alphabet,M,n", [("cnn", 14, ALPHA, 3, 65), ("ge", 90, AAS, 2, 33)])
def test_non_lookup_forms(eng, kind, L, alphabet, M, n):
    A = len(alphabet)
    lut = _native.make_lut(alphabet)
    natives = [make_native(eng, kind, L, A, H, F if kind == "cnn" else 0, K if kind == "cnn" else 0, seed=4300 + m)[0] for m in range(M)]
    stride = fd._stride_for(n)
    d_in = dev(synth.random_sequence_bytes(n, L, alphabet, 9))
    direct(eng, natives, d_in, n, L, lut, stride)
    want_p, want_m, want_c, want_f = direct(eng, natives, d_in, n, L, lut, stride)
    assert want_c[5] == 0                                                      # (not the lookup kernel)
    got_p, got_m, got_c, got_f = stepped(eng, natives, d_in, n, L, lut, stride)
    assert np.array_equal(got_p, want_p) and np.array_equal(got_m, want_m) and got_c == want_c and got_f == want_f
    assert not (got_p[:, :n] == FILL).any() and not (got_m[:n] == FILL).any()


def _members(kind, L, alphabet, M, seed):
    out = []
    for m in range(M):
        mod = bm.CNN(L, F, H, alphabet, kernel_size=K) if kind == "cnn" else bm.MLP(L, H, alphabet)
        mod.model.set_weights(ref_np.synth_weights(mod.model.shapes(), seed + m))
        out.append(mod)
    return out


def test_seventeen_mlp_members_through_the_ensemble(eng):
    """M > 16 with a mean keeps its route (planes, transpose, the row-major reduction); both values of step_call give np.mean's bits."""
    members = _members("mlp", 14, ALPHA, 17, 4400)
    rows = synth.random_sequence_bytes(65, 14, ALPHA, 10)
    seqs = synth.bytes_to_strings(rows)
    got = {}
    for sc in (0, 1):
        eng.set_option("step_call", sc)
        got[sc] = fd.DistributedEnsemble(members, mode="sequence").get_fitness(seqs)
        got[sc, "matrix"] = fd.DistributedEnsemble(members, mode="sequence", combine_with=lambda x: x).get_fitness(seqs)
    assert got[0].shape == (65,) and np.array_equal(got[0], got[1]) and np.array_equal(got[0, "matrix"], got[1, "matrix"])
    assert np.array_equal(got[1], np.mean(got[1, "matrix"], axis=1))


# ------------------------------------------------------------------ what can go stale
def test_new_weights_other_options_another_lut(eng):
    natives = cnn8(eng, seed=4500)
    n, stride = 257, fd._stride_for(257)
    d_in = dev(synth.random_sequence_bytes(n, L8, ALPHA, 11))
    bufs = buffers(3, stride, n)
    step = _native.NativeStep(eng, natives, L8, LUT, bufs[0].data_ptr(), stride, bufs[1].data_ptr(), None)
    first = stepped(eng, natives, d_in, n, L8, LUT, stride, step=step, bufs=bufs)
    # new weights for one member: the same step object scores with them, and builds that member's score table again
    natives[1].set_weights(ref_np.synth_weights(ref_np.cnn_shapes(L8, 4, F, H, K), 4599))
    got_p, got_m, got_c, _ = stepped(eng, natives, d_in, n, L8, LUT, stride, step=step, bufs=bufs)
    assert got_c[6] == 1 and got_c[5] == 1, got_c
    want_p, want_m, _, _ = direct(eng, natives, d_in, n, L8, LUT, stride)
    assert np.array_equal(got_p[:, :n], want_p[:, :n]) and np.array_equal(got_m[:n], want_m[:n])
    assert not np.array_equal(got_p[1, :n], first[0][1, :n]) and np.array_equal(got_p[0, :n], first[0][0, :n])
    # the head-only kernel instead of the tables of scores: same bits, no lookup launch
    eng.set_option("cnn_score_table", 0)
    off_p, off_m, off_c, _ = stepped(eng, natives, d_in, n, L8, LUT, stride, step=step, bufs=bufs)
    eng.set_option("cnn_score_table", 1)
    assert off_c[5] == 0 and np.array_equal(off_p[:, :n], want_p[:, :n]) and np.array_equal(off_m[:n], want_m[:n])
    # another alphabet's LUT through the engine in between
    ge = make_native(eng, "ge", 90, 20, H, seed=4600)[0]
    d_aa = dev(synth.random_sequence_bytes(33, 90, AAS, 12))
    direct(eng, [ge], d_aa, 33, 90, LUT_AA, fd._stride_for(33), mean=False)
    refill(*bufs)
    lut_p, lut_m, _, _ = stepped(eng, natives, d_in, n, L8, LUT, stride, step=step, bufs=bufs)
    assert np.array_equal(lut_p[:, :n], want_p[:, :n]) and np.array_equal(lut_m[:n], want_m[:n])


def test_error_word_behind_the_scores(eng):
    import torch

    natives = cnn8(eng, seed=4700)
    n, stride = 257, fd._stride_for(257)
    rows = synth.random_sequence_bytes(n, L8, ALPHA, 13)
    bad = rows.copy()
    bad[200, 3] = ord("X")
    planes, mu = buffers(3, stride, n)
    word = torch.full((1,), FILL, device="cuda")
    torch.cuda.synchronize()
    step = _native.NativeStep(eng, natives, L8, LUT, planes.data_ptr(), stride, mu.data_ptr(), word.data_ptr())
    d_bad, d_ok = dev(bad), dev(rows)
    step.launch(d_bad.data_ptr(), n)
    torch.cuda.synchronize()
    assert float(word.cpu()[0]) != 0.0
    with pytest.raises(ValueError):
        eng.sync()
    step.launch(d_ok.data_ptr(), n)
    eng.sync()
    assert float(word.cpu()[0]) == 0.0
    want_p, want_m, _, _ = direct(eng, natives, d_ok, n, L8, LUT, stride)
    assert np.array_equal(planes.cpu().numpy()[:, :n], want_p[:, :n]) and np.array_equal(mu.cpu().numpy()[:n], want_m[:n])


# ------------------------------------------------------------------ lifetime
def test_a_destroyed_member_makes_the_step_dead(eng):
    natives = cnn8(eng, seed=4800)
    n, stride = 65, fd._stride_for(65)
    d_in = dev(synth.random_sequence_bytes(n, L8, ALPHA, 14))
    planes, mu = buffers(3, stride, n)
    step = _native.NativeStep(eng, natives, L8, LUT, planes.data_ptr(), stride, mu.data_ptr(), None)
    step.launch(d_in.data_ptr(), n)
    eng.sync()
    refill(planes)
    eng._lib.fx_model_destroy(natives[2].handle)
    natives[2].handle = None
    before = counters(eng)
    with pytest.raises(_native.FxError) as ex:
        step.launch(d_in.data_ptr(), n)
    assert ex.value.code == _native.FX_ESTATE
    eng.sync()
    assert tuple(counters(eng) - before) == (0,) * 7 and (planes.cpu().numpy() == FILL).all()      # nothing was enqueued
    step.destroy()                                                             # after the model ...
    step.destroy()
    # ... and before the models
    natives = cnn8(eng, seed=4810)
    step = _native.NativeStep(eng, natives, L8, LUT, planes.data_ptr(), stride, None, None)
    step.launch(d_in.data_ptr(), n)
    eng.sync()
    step.destroy()
    del natives, step


def test_create_refuses_what_the_direct_calls_refuse(eng):
    natives = cnn8(eng, seed=4900)
    planes, mu = buffers(3, 128, 64)
    with pytest.raises(ValueError):
        _native.NativeStep(eng, natives, 9, LUT, planes.data_ptr(), 128, mu.data_ptr(), None)           # seq_len is not the members'
    with pytest.raises(_native.FxError):
        _native.NativeStep(eng, natives, L8, LUT, planes.data_ptr(), 126, mu.data_ptr(), None)         # stride is no multiple of 4
    with pytest.raises(_native.FxError):
        _native.NativeStep(eng, natives, L8, LUT, planes.data_ptr() + 4, 128, mu.data_ptr(), None)     # planes are not 16-byte aligned
    with pytest.raises(_native.FxError):
        _native.NativeStep(eng, natives, L8, LUT_AA, planes.data_ptr(), 128, mu.data_ptr(), None)      # LUT entries beyond the alphabet


# ------------------------------------------------------------------ DistributedEnsemble without a process group
@pytest.fixture()
def ensemble_case(eng):
    members = _members("cnn", L8, ALPHA, 3, 5000)
    rows = {s: synth.random_sequence_bytes(1000, L8, ALPHA, s) for s in (21, 22)}
    natives = [m.native() for m in members]
    ref = {}
    for s, b in rows.items():
        p, mu, _, _ = direct(eng, natives, dev(b), 1000, L8, LUT, fd._stride_for(1000))
        ref[s] = (p[:, :1000].T.copy(), mu[:1000].copy())
    return members, rows, ref


def test_ensemble_both_slots_in_flight(eng, ensemble_case):
    members, rows, ref = ensemble_case
    for sc in (1, 0):
        eng.set_option("step_call", sc)
        ens = fd.DistributedEnsemble(members, mode="sequence")
        d = {s: dev(b) for s, b in rows.items()}
        order = [21, 22, 22, 21, 21]
        for i, s in enumerate(order):                                           # as bench.py drives it: launch(k), finish(k - 1)
            ens.launch(d[s], 1000, slot=i & 1, want="mean")
            if i:
                got = read(ens, ens.finish((i - 1) & 1))
                assert np.array_equal(got, ref[order[i - 1]][1]), (sc, i)
        last = ens.finish((len(order) - 1) & 1)
        again = ens.finish((len(order) - 1) & 1)                                # finish twice: the same result
        assert np.array_equal(read(ens, last), ref[order[-1]][1]) and np.array_equal(read(ens, again), read(ens, last))
        assert (ens._slots[0].step is not None) == bool(sc)
        eng.sync()


def test_ensemble_want_switches_numpy_then_resident_and_overwritten_buffers(eng, ensemble_case):
    import torch

    members, rows, ref = ensemble_case
    ens = fd.DistributedEnsemble(members, mode="sequence")
    d21 = dev(rows[21])
    for want in ("mean", "matrix", "mean", "matrix"):
        ens.launch(d21, 1000, 0, want)
        got = read(ens, ens.finish(0))
        assert np.array_equal(got, ref[21][0] if want == "matrix" else ref[21][1]), want
    ens.launch(rows[22], 1000, 0, "mean")                                       # a NumPy batch (uploaded), then a resident tensor
    assert np.array_equal(read(ens, ens.finish(0)), ref[22][1])
    first_step = ens._slots[0].step
    ens.launch(d21, 1000, 0, "mean")
    assert np.array_equal(read(ens, ens.finish(0)), ref[21][1])
    assert ens._slots[0].step is first_step and first_step is not None          # prepared once per key, members and LUT
    s = ens._slots[0]
    torch.cuda.synchronize()
    refill(s.planes, s.local, s.mean, value=float("nan"))                       # a caller overwrote the slot's buffers: every element is rewritten
    ens.launch(d21, 1000, 0, "mean")
    out = read(ens, ens.finish(0))
    assert not np.isnan(out).any() and np.array_equal(out, ref[21][1])
    assert not np.isnan(read(ens, s.planes[:, :1000])).any()
    # new weights for one member reach the prepared step through native()
    members[0].model.set_weights(ref_np.synth_weights(members[0].model.shapes(), 5099))
    ens.launch(d21, 1000, 0, "mean")
    moved = read(ens, ens.finish(0)).copy()
    want_p, want_m, _, _ = direct(eng, [m.native() for m in members], d21, 1000, L8, LUT, fd._stride_for(1000))
    assert np.array_equal(moved, want_m[:1000]) and not np.array_equal(moved, ref[21][1])
    assert np.array_equal(ens.get_fitness(synth.bytes_to_strings(rows[21])), want_m[:1000])
    eng.sync()
