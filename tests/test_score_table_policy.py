"""What a launch group does about its members' score tables (engine option `cnn_score_table`; fx_cnn_score_decide in
csrc/score_cnn_forms.h), pinned on the CPU through fx_debug_cnn_score_pick: the launcher's own pure functions on an engine of 256 CUs and
160 KiB of LDS that never sees a device.

The rule is layered on fx_cnn_pool_decide's answer and changes neither it nor the pick: where that answer is "conv" nothing changes; where
it is "table" or "build", option 1 brings the group's tables up to date as that answer says and launches the lookup kernel, option 0 the
head-only kernel.  Tables are therefore built exactly when pooled-feature tables were built before the option existed."""
import pytest

from flexs_amd import _native

CANON = dict(L=8, A=4, F=32, H=100, K=5)
UNROLLED8_W16, UNROLLED8_W8 = 5, 6                        # CnnFormId
W16_ANY_SIZE = {"cnn_big_units": 0}                       # the way the GPU tests put the 16-wave form on small launches
SIZES = (1_000, 65_536, 65_537, 100_000)


def decide(N, M=3, *, fresh, options=None, **kw):
    shape = dict(CANON, **{k: kw.pop(k) for k in list(kw) if k in CANON})
    return _native.debug_cnn_score_pick(shape["L"], shape["A"], shape["F"], shape["H"], shape["K"], N, M, fresh=fresh, options=options, **kw)


def pool_decide(N, M=3, *, fresh, options=None, **kw):
    return _native.debug_cnn_pool_pick(CANON["L"], CANON["A"], CANON["F"], CANON["H"], CANON["K"], N, M, fresh=fresh, options=options, **kw)


def expected(score, pool, fresh, N):
    """(form, build) written out from the issue's rule, not from the code."""
    if pool == 0:
        return "conv", False
    if fresh:
        return ("lookup" if score else "head"), False
    if pool == 2 or N > 4 ** 8:
        return ("lookup" if score else "head"), True
    return "conv", False


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("fresh", [False, True])
@pytest.mark.parametrize("pool", [0, 1, 2])
@pytest.mark.parametrize("score", [0, 1])
@pytest.mark.parametrize("M", [1, 3])
def test_both_options_freshness_and_size(score, pool, fresh, N, M):
    opts = dict(W16_ANY_SIZE, cnn_pool_table=pool, cnn_score_table=score)
    got = decide(N, M, fresh=fresh, options=opts)
    assert got["rc"] == "FX_OK" and got["id"] == UNROLLED8_W16
    assert (got["form"], got["build"]) == expected(score, pool, fresh, N), got
    # the pooled-table decision underneath is the one fx_debug_cnn_pool_pick reports, whatever cnn_score_table says
    below = pool_decide(N, M, fresh=fresh, options=opts)
    assert got["decision"] == below["decision"] == pool_decide(N, M, fresh=fresh, options=dict(W16_ANY_SIZE, cnn_pool_table=pool))["decision"]
    assert (got["form"] == "conv") == (below["decision"] == "conv")


def test_default_options_at_the_headline_and_below_it():
    """The headline launch (3 x 1e5) builds once, then looks up; exactly 4^8 rows do not build; the 8-wave pick never takes a table."""
    shipped = decide(100_000, 3, fresh=False)
    assert shipped["build"] and shipped["form"] in ("lookup", "head")
    for score, form in ((0, "head"), (1, "lookup")):
        opts = {"cnn_score_table": score}
        assert decide(100_000, 3, fresh=False, options=opts)["form"] == form and decide(100_000, 3, fresh=False, options=opts)["build"]
        got = decide(100_000, 3, fresh=True, options=opts)
        assert got["form"] == form and not got["build"]
        assert decide(65_536, 3, fresh=False, options=opts)["form"] == "conv"
        for fresh in (False, True):
            small = decide(1_000, 1, fresh=fresh, options=opts)
            assert small["id"] == UNROLLED8_W8 and small["form"] == "conv" and not small["build"], small
            assert decide(1_000, 1, fresh=fresh, options=dict(opts, cnn_pool_table=2))["form"] == "conv"
    for fresh in (False, True):
        small = decide(1_000, 1, fresh=fresh)
        assert small["id"] == UNROLLED8_W8 and small["form"] == "conv", small


@pytest.mark.parametrize("pool", [1, 2])
@pytest.mark.parametrize("fresh", [False, True])
def test_rows_that_are_not_resident_never_take_a_table(pool, fresh):
    opts = dict(W16_ANY_SIZE, cnn_pool_table=pool, cnn_score_table=1)
    for N in SIZES:
        assert decide(N, fresh=fresh, options=opts, rows_on=True)["form"] == "conv"       # launched first: the rows arrive while the kernel runs
        assert decide(N, fresh=fresh, options=opts, ascii_host=True)["form"] == "conv"    # zero-copy host call
        assert decide(N, fresh=fresh, options=dict(opts, cnn_stage_host=0), ascii_host=True)["form"] == "conv"


@pytest.mark.parametrize("shape", [dict(L=14), dict(H=200), dict(A=20), dict(K=3), dict(F=16)])
def test_other_shapes_have_no_table(shape):
    for fresh in (False, True):
        got = decide(100_000, fresh=fresh, options={"cnn_pool_table": 2, "cnn_score_table": 1}, **shape)
        assert got["form"] == "conv" and not got["build"], got


def test_the_pick_and_the_pooled_decision_are_unchanged():
    pick = _native.debug_cnn_form_pick(8, 4, 32, 100, 5, 100_000, 3)
    for score in (0, 1):
        assert _native.debug_cnn_form_pick(8, 4, 32, 100, 5, 100_000, 3, options={"cnn_score_table": score}) == pick
        for fresh in (False, True):
            assert pool_decide(100_000, fresh=fresh, options={"cnn_score_table": score}) == pool_decide(100_000, fresh=fresh)


def test_option_range():
    for bad in (-1, 2, 3):
        with pytest.raises(ValueError):
            decide(1000, fresh=True, options={"cnn_score_table": bad})
    with pytest.raises(ValueError):
        decide(1000, fresh=True, options={"cnn_score_table": 1, "cnn_pool_table": 3})
