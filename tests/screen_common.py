"""Shared by the screening tests (test_screen_host.py, test_gpu_topk.py, test_gpu_screen.py): the ordering rule's oracle, the
crafted score arrays, and the tie-heavy GlobalEpistasis weights."""
import numpy as np

from oracle import ref_np

FLT_MAX = np.float32(3.4028235e38)
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -FLT_MAX, 1.0], np.float32)


def oracle_order(x, k):
    """The rule, as the issue states it (NOT the code under test): dense ranks (NaNs and +-0 collapse), then value descending,
    index ascending."""
    x = np.asarray(x).reshape(-1)
    r = np.unique(x, return_inverse=True)[1].reshape(-1)
    return np.lexsort((np.arange(x.size), -r.astype(np.int64)))[:min(k, x.size)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ks_for(n):
    """k of the issue's list, clipped to the legal range 1 .. min(4096, ...); 1061 (a prime) is ours."""
    return sorted({min(max(k, 1), 4096) for k in (1, 2, 100, 1061, 4096, n - 1, n, n + 1)})


def fills(n, seed):
    """name -> float32[n]: the crafted arrays (a), (c) - (h) of the issue; (b) depends on k: two_values()."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    out = {
        "a_all_equal": np.full(n, 0.25, np.float32),
        "c_normal": rng.standard_normal(n).astype(np.float32),
        "d_specials": SPECIALS[rng.integers(0, SPECIALS.size, n)],
        "e_ascending": i.astype(np.float32),                      # (exact below 2^24: strictly ascending)
        "e_descending": i[::-1].astype(np.float32),
        "f_every_997th": np.where(i % 997 == 0, 1.0, 0.0).astype(np.float32),
        "g_low_digit": (np.uint32(0x3F800000) + i.astype(np.uint32)).view(np.float32),
        "g_high_digit": (i.astype(np.uint32) << np.uint32(24)).view(np.float32),
        "h_negative": (-np.abs(rng.standard_normal(n)) - 1e-3).astype(np.float32),
    }
    assert (np.diff(out["e_ascending"]) > 0).all() and (out["h_negative"] < 0).all()
    return out


def two_values(n, k, seed):
    """(b): k // 2 entries of the upper value at random places, the lower value everywhere else: the k-th best lies inside the
    lower value's run."""
    x = np.full(n, 1.0, np.float32)
    x[np.random.default_rng(seed).permutation(n)[:k // 2]] = 2.0
    return x


def ge_clipped_weights(L, A, H, seed, bias):
    """GlobalEpistasis weights whose Dense(1, relu) first layer has bias `bias`: a negative one clips most rows to 0, and every row
    a member clips gets that member's one constant score -- long runs of bit-equal scores."""
    w = ref_np.synth_weights(ref_np.ge_shapes(L, A, H), seed)
    w[1] = np.full_like(w[1], bias)
    return w
