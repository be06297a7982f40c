"""What a launch group does about its members' pooled-feature tables (engine option `cnn_pool_table`; fx_cnn_pool_decide in
csrc/score_cnn_forms.h), pinned on the CPU through fx_debug_cnn_pool_pick: the launcher's own pure function on an engine of 256 CUs and
160 KiB of LDS that never sees a device.

The rule: the head-only kernel stands in for the 16-wave unrolled seq_len = 8 form only, with the rows in device memory when the kernel
starts.  Fresh tables are used; stale ones are built first when the launch has MORE than 4^8 rows per member (option 1) or whatever its
size (option 2); otherwise the launch runs the conv form that fx_cnn_pick_fused names, which this option never changes."""
import pytest

from flexs_amd import _native

CANON = dict(L=8, A=4, F=32, H=100, K=5)
UNROLLED8_W16, UNROLLED8_W8 = 5, 6                        # CnnFormId
W16_ANY_SIZE = {"cnn_big_units": 0}                       # the way the GPU tests put the 16-wave form on small launches


def decide(N, M=3, *, fresh, options=None, **kw):
    shape = dict(CANON, **{k: kw.pop(k) for k in list(kw) if k in CANON})
    return _native.debug_cnn_pool_pick(shape["L"], shape["A"], shape["F"], shape["H"], shape["K"], N, M, fresh=fresh, options=options, **kw)


# (option, fresh, N) -> decision, for launches that take the 16-wave unrolled form at every one of these sizes
MATRIX = [
    (0, True, 65_536, "conv"), (0, True, 65_537, "conv"), (0, True, 5_000, "conv"), (0, True, 1_000, "conv"),
    (0, False, 65_536, "conv"), (0, False, 65_537, "conv"), (0, False, 5_000, "conv"), (0, False, 1_000, "conv"),
    (1, True, 65_536, "table"), (1, True, 65_537, "table"), (1, True, 5_000, "table"), (1, True, 1_000, "table"),
    (1, False, 65_536, "conv"), (1, False, 65_537, "build"), (1, False, 5_000, "conv"), (1, False, 1_000, "conv"),
    (2, True, 65_536, "table"), (2, True, 65_537, "table"), (2, True, 5_000, "table"), (2, True, 1_000, "table"),
    (2, False, 65_536, "build"), (2, False, 65_537, "build"), (2, False, 5_000, "build"), (2, False, 1_000, "build"),
]


@pytest.mark.parametrize("option,fresh,N,want", MATRIX)
@pytest.mark.parametrize("M", [1, 3])
def test_option_freshness_and_size(option, fresh, N, want, M):
    got = decide(N, M, fresh=fresh, options=dict(W16_ANY_SIZE, cnn_pool_table=option))
    assert got["rc"] == "FX_OK" and got["canonical"] and got["id"] == UNROLLED8_W16
    assert got["decision"] == want, got


def test_shipped_option_at_the_headline_and_below_it():
    """Default options: the headline launch (3 x 1e5) builds once and then reads the table; launches that take the 8-wave form never do."""
    assert decide(100_000, 3, fresh=False)["decision"] == "build"
    assert decide(100_000, 3, fresh=True)["decision"] == "table"
    assert decide(65_536, 3, fresh=False)["decision"] == "conv"          # exactly 4^8 rows: not MORE than the enumeration
    for fresh in (False, True):
        small = decide(1_000, 1, fresh=fresh)
        assert small["id"] == UNROLLED8_W8 and small["decision"] == "conv", small
        assert decide(5_000, 1, fresh=fresh, options={"cnn_pool_table": 2})["decision"] == "conv"   # 8-wave form: whatever the option


@pytest.mark.parametrize("option", [1, 2])
@pytest.mark.parametrize("fresh", [False, True])
def test_rows_that_are_not_resident_keep_the_conv_forms(option, fresh):
    opts = dict(W16_ANY_SIZE, cnn_pool_table=option)
    assert decide(100_000, fresh=fresh, options=opts, rows_on=True)["decision"] == "conv"      # launched first: the rows arrive while the kernel runs
    assert decide(100_000, fresh=fresh, options=opts, ascii_host=True)["decision"] == "conv"   # zero-copy host call
    assert decide(100_000, fresh=fresh, options=dict(opts, cnn_stage_host=0), ascii_host=True)["decision"] == "conv"


@pytest.mark.parametrize("shape", [dict(L=14), dict(H=200), dict(A=20), dict(L=14, H=200), dict(K=3), dict(F=16)])
@pytest.mark.parametrize("fresh", [False, True])
def test_other_shapes_have_no_table(shape, fresh):
    got = decide(100_000, fresh=fresh, options={"cnn_pool_table": 2}, **shape)
    assert not got["canonical"] and got["decision"] == "conv", got


def test_other_variants_of_the_canonical_shape_keep_their_form():
    for variant in (1, 4, 11):
        assert decide(100_000, fresh=True, options={"cnn_variant": variant, "cnn_pool_table": 2})["decision"] == "conv", variant
    assert decide(100_000, fresh=True, options={"cnn_variant": 7, "cnn_pool_table": 2})["decision"] == "table"


def test_the_fused_pick_is_unchanged():
    got = _native.debug_cnn_form_pick(8, 4, 32, 100, 5, 100_000, 3)
    assert (got["QT"], got["C1T"], got["C2P"], got["WAVES"], got["L1S"]) == (1, 1, 2, 16, 4), got
    for option in (0, 1, 2):
        assert _native.debug_cnn_form_pick(8, 4, 32, 100, 5, 100_000, 3, options={"cnn_pool_table": option}) == got


def test_option_range():
    with pytest.raises(ValueError):
        decide(1000, fresh=True, options={"cnn_pool_table": 3})
    with pytest.raises(ValueError):
        decide(1000, fresh=True, options={"cnn_pool_table": -1})
