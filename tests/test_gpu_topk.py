"""K8, the stand-alone top-k select (csrc/topk.hip; fx_topk_dev / fx_topk): both forms -- one workgroup sorting in LDS, and the
radix select with one launch per pass -- against the ordering rule's oracle (screen_common.oracle_order, not the code under
test), EXACTLY: indices with array_equal, values by their bits.  The form is forced with `topk_small_rows` and asserted through
`topk_large_launches`; outputs are pre-filled with -1 / NaN; every radix-select case runs twice and must repeat itself."""
import numpy as np
import pytest

from flexs_amd import _native

from gpu_common import eng  # noqa: F401  (the module's engine fixture)
from screen_common import bits, fills, ks_for, oracle_order, two_values

pytestmark = pytest.mark.gpu

T = 1000                                   # the threshold of the cases T - 1, T, T + 1
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, T - 1, T, T + 1, 8191, 8192, 8193, 100003, 1048577]


@pytest.fixture()
def shipped(eng):
    keep = eng.get_option("topk_small_rows")
    try:
        yield eng
    finally:
        eng.set_option("topk_small_rows", keep)


def select_dev(eng, d_x, n, k):
    """One fx_topk_dev call on scores resident in device memory -> (idx, val, radix selects it took)."""
    import torch

    d_idx = torch.full((k,), -1, dtype=torch.int64, device="cuda")
    d_val = torch.full((k,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    before = eng.get_option("topk_large_launches")
    count = eng.topk_dev(d_x.data_ptr(), n, k, d_idx.data_ptr(), d_val.data_ptr())
    eng.sync()
    assert count == min(k, n)
    idx, val = d_idx.cpu().numpy(), d_val.cpu().numpy()
    assert (idx[count:] == -1).all() and np.isnan(val[count:]).all(), "wrote past min(k, N)"
    return idx[:count], val[:count], eng.get_option("topk_large_launches") - before


def check(eng, x, ks, what, orders=None):
    """x against the oracle for every k, in every form that takes its size."""
    import torch

    n = x.shape[0]
    d_x = torch.from_numpy(x).cuda()
    full = oracle_order(x, max(ks)) if orders is None else orders
    for small_rows, large in ((8192, 0), (0, 1)):
        if not large and n > 8192:
            continue
        eng.set_option("topk_small_rows", small_rows)
        for k in ks:
            want = full[:k]
            for rep in range(2 if large else 1):
                idx, val, took = select_dev(eng, d_x, n, k)
                assert took == large, (what, n, k, "form")
                assert np.array_equal(idx, want), (what, n, k, "large" if large else "small", rep)
                assert np.array_equal(bits(val), bits(x[want])), (what, n, k, "values")


@pytest.mark.parametrize("n", SIZES)
def test_select_both_forms(shipped, n):
    ks = ks_for(n)
    for name, x in fills(n, 100 + n % 97).items():
        check(shipped, x, ks, name)
    for k in ks:                                            # (b): the k-th best inside the lower value's run
        check(shipped, two_values(n, k, 5 + k), [k], "b_two_values")


def test_threshold_picks_the_form(shipped):
    import torch

    eng = shipped
    eng.set_option("topk_small_rows", T)
    for n, large in ((T - 1, 0), (T, 0), (T + 1, 1)):
        x = np.random.default_rng(n).standard_normal(n).astype(np.float32)
        idx, val, took = select_dev(eng, torch.from_numpy(x).cuda(), n, 100)
        assert took == large, n
        assert np.array_equal(idx, oracle_order(x, 100)) and np.array_equal(bits(val), bits(x[idx]))
    assert eng.get_option("topk_small_rows") == T
    for bad in (-1, 8193):
        with pytest.raises(_native.FxError):
            eng.set_option("topk_small_rows", bad)


@pytest.mark.parametrize("n", [257, 70001])
def test_host_in_host_out(shipped, n):
    eng = shipped
    fl = fills(n, 9)
    for small_rows in (8192, 0):
        eng.set_option("topk_small_rows", small_rows)
        for name in ("c_normal", "d_specials"):
            x = fl[name]
            for k in (1, 100, 4096):
                before = eng.get_option("topk_large_launches")
                idx, val = eng.topk(x, k)
                assert eng.get_option("topk_large_launches") - before == (0 if n <= small_rows else 1)
                want = oracle_order(x, k)
                assert idx.dtype == np.int64 and val.dtype == np.float32
                assert np.array_equal(idx, want) and np.array_equal(bits(val), bits(x[want])), (name, n, k)


def test_arguments(shipped):
    import torch

    eng = shipped
    x = np.arange(10, dtype=np.float32)
    d_x = torch.from_numpy(x).cuda()
    d_idx = torch.full((16,), -1, dtype=torch.int64, device="cuda")
    d_val = torch.full((16,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    for bad in (0, -3, 4097):
        with pytest.raises(ValueError):
            eng.topk_dev(d_x.data_ptr(), 10, bad, d_idx.data_ptr(), d_val.data_ptr())
        with pytest.raises(ValueError):
            eng.topk(x, bad)
    with pytest.raises(ValueError):
        eng.topk_dev(d_x.data_ptr(), 2 ** 31, 5, d_idx.data_ptr(), d_val.data_ptr())      # refused before anything is read
    assert eng.topk_dev(d_x.data_ptr(), 0, 5, d_idx.data_ptr(), d_val.data_ptr()) == 0
    idx, val = eng.topk(np.zeros(0, np.float32), 5)
    assert idx.shape == (0,) and val.shape == (0,)
    eng.sync()
    assert (d_idx.cpu().numpy() == -1).all()
    idx, val = eng.topk(x, 4096)                                                            # k > N: all of them, best first
    assert idx.tolist() == list(range(9, -1, -1)) and val.tolist() == x[::-1].tolist()
