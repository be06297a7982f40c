"""Which form of the fused CNN kernel a launch takes, pinned on the CPU through fx_debug_cnn_form_pick: the launchers' own pure
choice (csrc/score_cnn_forms.h) on an engine of 256 CUs and 160 KiB of LDS that never sees a device.  Every expectation restates a
line of the dispatch as it stood before the forms were named (commit e2ef66e: `mfma:N` = csrc/score_cnn_mfma.hip line N, `split:N` =
csrc/score_cnn_split.hip line N there); the small-launch kernel (score_cnn_quad.hip), which a launch tries first, is set aside."""
import pytest

from flexs_amd import _native

BASE = dict(A=4, K=5, FT=2, HT=7, NT=1, DENSE_LDS=1, WAVES=8, G1=1, L1S=0, PRIO=0, SEG=0, HEAD=1, STG=0, QT=0, C1T=0, C2P=0)
UNROLLED8_W16 = dict(WAVES=16, L1S=4, PRIO=1)
CONV = dict(HT=1, DENSE_LDS=0, HEAD=0)


def pick(L, N, M, *, A=4, F=32, H=100, K=5, **kw):
    return _native.debug_cnn_form_pick(L, A, F, H, K, N, M, **kw)


def check(got, want, **geometry):
    assert got["rc"] == "FX_OK", got
    fields = {k: got[k] for k in BASE}
    assert fields == {**BASE, **want}
    for k, v in geometry.items():
        assert got[k] == v, (k, got)


# (L, N, M), engine state, what differs from BASE, geometry -- the table of the issue that asked for this test
HEADLINE = (8, 100_000, 3)
ISSUE_ROWS = [
    # mfma:34 (auto -> variant 7), mfma:71
    (HEADLINE, {}, dict(UNROLLED8_W16, QT=1, C1T=1, C2P=2), dict(TG=6250)),
    (HEADLINE, dict(options={"cnn_conv2_prefix": 0}), dict(UNROLLED8_W16, QT=1, C1T=1), {}),          # mfma:72
    (HEADLINE, dict(options={"cnn_conv2_prefix": 1}), dict(UNROLLED8_W16, QT=1, C1T=1, C2P=1), {}),   # mfma:70
    (HEADLINE, dict(options={"cnn_conv1_table": 0}), dict(UNROLLED8_W16, QT=1), {}),                  # mfma:64, 67, 73
    (HEADLINE, dict(options={"cnn_quad_tail": 0}), dict(UNROLLED8_W16, C1T=1, C2P=2), {}),            # mfma:68, 76
    (HEADLINE, dict(rows_on=True), UNROLLED8_W16, {}),                                                # mfma:64, 68, 79
    (HEADLINE, dict(ascii_host=True, options={"cnn_stage_host": 1}), dict(UNROLLED8_W16, STG=1), {}),  # mfma:24
    ((8, 10_000, 1), {}, dict(L1S=4, PRIO=1), dict(TG=625)),                                          # mfma:37, 82 (variant 11)
    ((14, 100_000, 3), {}, dict(WAVES=16, L1S=10, PRIO=1), {}),                                       # mfma:38, 57
    ((14, 10_000, 1), {}, {}, {}),                                                                    # mfma:132
    ((50, 20, 3), {}, dict(SEG=1, WAVES=4), dict(seg_sb=5, TG=2)),                                    # mfma:106-122: eight-wave count 2, four-wave count 5
    ((50, 20, 3), dict(options={"cnn_seg_multi": 0}), dict(SEG=1), dict(seg_sb=1)),                   # mfma:97 (L1 >= 24), 125
]


@pytest.mark.parametrize("shape,state,want,geometry", ISSUE_ROWS)
def test_canonical_cnn(shape, state, want, geometry):
    check(pick(*shape, **state), want, **geometry)


# the other branches: (L, N, M), model, engine state, what differs from BASE, geometry
BIG, SMALL, LONG = (8, 100_000, 3), (8, 1000, 1), (50, 20, 3)
OTHER_ROWS = [
    # binary alphabet
    (BIG, dict(A=2), {}, dict(A=2, WAVES=16), {}),                                                    # mfma:266
    (SMALL, dict(A=2), {}, dict(A=2), {}),                                                            # mfma:266
    (LONG, dict(A=2), {}, dict(A=2, SEG=1), dict(seg_sb=0)),                                          # mfma:263-265
    # at most 16 filters
    (BIG, dict(F=16), {}, dict(FT=1, WAVES=16), {}),                                                  # mfma:278
    (SMALL, dict(F=16), {}, dict(FT=1), {}),                                                          # mfma:278
    (LONG, dict(F=16), {}, dict(FT=1, SEG=1), {}),                                                    # mfma:275-277 (8 * 1 * 64 * 16 bytes of slots)
    (BIG, dict(F=16, A=20), {}, dict(FT=1, A=20), {}),                                                # mfma:272: no 16-wave form
    # kernel sizes 3 and 7
    (BIG, dict(K=3), {}, dict(K=3, WAVES=16), {}),                                                    # mfma:290
    (SMALL, dict(K=3), {}, dict(K=3), {}),                                                            # mfma:290
    (LONG, dict(K=3), {}, dict(K=3, SEG=1), {}),                                                      # mfma:286-289
    ((20, 100_000, 3), dict(K=7), {}, dict(K=7), {}),                                                 # mfma:292: no 16-wave form
    (LONG, dict(K=7), {}, dict(K=7), {}),                                                             # mfma:292: no segmented form
    # hidden widths
    (BIG, dict(H=16), {}, dict(HT=1, WAVES=16), {}),                                                  # mfma:130
    (SMALL, dict(H=32), {}, dict(HT=2), {}),                                                          # mfma:132
    (LONG, dict(H=64), {}, dict(HT=4, SEG=1), dict(seg_sb=1)),                                        # mfma:95 (HT 7 only), 125
    (BIG, dict(H=128), {}, dict(HT=8), {}),                                                           # mfma:129, 132: no 16-wave form from 8 tiles on
    (BIG, dict(H=200), dict(options={"cnn_head_slab": 0}), dict(HT=13, DENSE_LDS=0), {}),             # mfma:12, 132: head from L2
    ((8, 1000, 1), dict(H=256), {}, dict(HT=16, DENSE_LDS=0), {}),                                    # mfma:296 (63 units: below 16 per CU), 132
    (LONG, dict(H=200), {}, dict(HT=13, DENSE_LDS=0, SEG=1), dict(seg_sb=1)),                         # mfma:126
    # forced variants and knobs
    (BIG, {}, dict(options={"cnn_variant": 1}), {}, {}),                                              # mfma:43
    (BIG, {}, dict(options={"cnn_variant": 4}), dict(WAVES=16), {}),                                  # mfma:54
    ((14, 1000, 1), {}, dict(options={"cnn_variant": 10}), dict(WAVES=16, L1S=10, PRIO=1), {}),       # mfma:57
    ((8, 10_000, 1), {}, dict(options={"cnn_big_units": 2}), dict(UNROLLED8_W16, QT=1, C1T=1, C2P=2), {}),   # mfma:297 (625 units >= 512)
    (LONG, {}, dict(options={"cnn_seg": 0}), {}, {}),                                                 # mfma:96, 132
    ((20, 20, 3), {}, dict(options={"cnn_seg": 1}), dict(SEG=1), dict(seg_sb=1)),                     # mfma:97 (forced), 105 (cnn_seg < 0 only), 125
    ((20, 20, 3), {}, {}, dict(SEG=1, WAVES=4), dict(seg_sb=2)),                                      # mfma:95, 97 (16 positions: enough when spread), 113
    ((20, 20, 3), {}, dict(options={"cnn_seg_multi": 0}), {}, {}),                                    # mfma:97 (... too few for one workgroup), 132
    # rows in host memory
    ((14, 100_000, 3), {}, dict(ascii_host=True), dict(WAVES=16, L1S=10, PRIO=1, STG=1), {}),         # mfma:25
    ((20, 100_000, 3), {}, dict(ascii_host=True), dict(WAVES=16, STG=1), {}),                         # mfma:26
    ((8, 10_000, 1), {}, dict(ascii_host=True), dict(L1S=4, PRIO=1, STG=1), {}),                      # mfma:27
    ((20, 10_000, 1), {}, dict(ascii_host=True), dict(STG=1), {}),                                    # mfma:28
    ((8, 20, 3), {}, dict(ascii_host=True), dict(L1S=4, PRIO=1), {}),                                 # mfma:22 (explorer size: no STG), 37
    (HEADLINE, {}, dict(ascii_host=True, options={"cnn_stage_host": 0}), dict(UNROLLED8_W16, QT=1, C1T=1, C2P=2), {}),   # mfma:18
]


@pytest.mark.parametrize("shape,model,state,want,geometry", OTHER_ROWS)
def test_other_branches(shape, model, state, want, geometry):
    check(pick(*shape, **model, **state), want, **geometry)


# the conv part of the two-kernel path
SPLIT_ROWS = [
    (BIG, dict(K=4), {}, dict(CONV, K=4), dict(TG=6250)),                                             # split:200
    (BIG, dict(H=200), {}, dict(CONV, WAVES=16, L1S=4, PRIO=1), {}),                                  # split:195-196
    ((14, 100_000, 3), dict(H=200), {}, dict(CONV, WAVES=16), {}),                                    # split:197
    (BIG, dict(H=200), dict(rows_on=True), CONV, {}),                                                 # split:195
    (LONG, dict(H=200), {}, dict(CONV, SEG=1), dict(seg_sb=0)),                                       # split:189-191
    (LONG, dict(K=7), {}, dict(CONV, K=7), {}),                                                       # split:185: no segmented form beyond five taps
    (LONG, dict(K=3, F=64), {}, dict(CONV, K=3, FT=4, SEG=1), {}),                                    # split:190 (8 * 4 * 64 * 16 bytes of slots)
    (BIG, dict(A=2, H=200), {}, dict(CONV, A=2), {}),                                                 # split:273
]


@pytest.mark.parametrize("shape,model,state,want,geometry", SPLIT_ROWS)
def test_split_path_conv_forms(shape, model, state, want, geometry):
    check(pick(*shape, path=1, **model, **state), want, **geometry)


def test_split_path_refusals_and_protein():
    assert pick(*BIG, path=1, K=6, F=64)["rc"] == "FX_EUNSUPPORTED"                                  # split:212
    got = pick(*BIG, path=1, A=20)                                                                    # split:251: score_cnn_pair.hip's conv kernel
    assert (got["rc"], got["pair_first"], got["id"]) == ("FX_OK", 1, 0)


@pytest.mark.parametrize("variant,L,text", [
    (7, 14, "cnn_variant 7 is a seq_len = 8 specialisation"),                                         # mfma:59
    (10, 8, "cnn_variant 10 is a seq_len = 14 specialisation"),                                       # mfma:56
    (11, 14, "cnn_variant 11 is a seq_len = 8 specialisation"),                                       # mfma:81
    (12, 8, "cnn_variant must be 0..11"),                                                             # mfma:83
])
def test_variant_errors(variant, L, text):
    got = pick(L, 100_000, 3, options={"cnn_variant": variant})
    assert (got["rc"], got["msg"]) == ("FX_EINVAL", text)


def test_ab_only_forms():
    got = pick(*HEADLINE, options={"cnn_variant": 5})
    if got["ab_build"]:
        check(got, dict(WAVES=16, L1S=4))                                                             # mfma:49: no s_setprio
        check(pick(*BIG, A=20), dict(A=20, WAVES=4, DENSE_LDS=0), pair_first=1)                       # mfma:318
    else:
        # the production library refuses the value where it always did: when the option is set (fx_engine.hip: ab_only_value)
        assert got["rc"] == "FX_EUNSUPPORTED" and "A/B build" in got["msg"]
        got = pick(*BIG, A=20)                                                                        # mfma:320
        assert (got["rc"], got["pair_first"]) == ("FX_EUNSUPPORTED", 1)


def test_shapes_without_a_fused_form():
    assert pick(*BIG, H=200)["rc"] == "FX_EUNSUPPORTED"                                               # mfma:296: the two-kernel path takes it
    assert pick(*BIG, K=4)["rc"] == "FX_EUNSUPPORTED"                                                 # mfma:221
    assert pick(*BIG, F=64)["rc"] == "FX_EUNSUPPORTED"                                                # mfma:220
    assert pick(*BIG, K=3, rows_on=True)["rc"] == "FX_EUNSUPPORTED"                                   # mfma:224
    assert pick(8, 100_000, 1000)["rc"] == "FX_EINVAL"                                                    # mfma:222
