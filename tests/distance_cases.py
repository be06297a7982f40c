"""Inputs of the edit-distance tests, shared by the host twin (tests/test_pack_sim.py) and the device file
(tests/test_gpu_distances.py): the lengths on both sides of every boundary csrc/mindist.hip has, the content families built per
length, and their distances by the plain DP (oracle.c_oracle), computed once per length and handed out read-only.

Nothing here calls the code under test: the reference is `c_oracle.levenshtein` / `c_oracle.hamming` per pair and
`ref_np.min_distance` for the selection rule (noisy_abstract_model.py:42-60)."""
import functools

import numpy as np

from oracle import c_oracle, ref_np

DNA = b"ACGT"
AAS = b"ILVAGMFYWEDQNHCRKSTP"

# L -> (the form fx_launch_min_dist / fx_launch_distances pick, rows staged through LDS in a one-pass launch).  Compare with the
# `if (L <= 32)` / `switch ((L + 63) / 64)` of both launchers, FX_STAGE_MAX_L = 160 and FX_MINDIST_MAX_L = 768 (12 words).
LENGTH_FORMS = (
    (32, "W=1 uint32_t", True), (33, "W=1", True),
    (64, "W=1", True), (65, "W=2", True),
    (128, "W=2", True), (129, "W=3", True),
    (160, "W=3", True), (161, "W=3", False),            # last staged, first unstaged
    (192, "W=3", False), (193, "W=4", False),
    (256, "W=4", False), (257, "W=6", False),
    (384, "W=6", False), (385, "W=8", False),
    (512, "W=8", False), (513, "W=12", False),
    (768, "W=12", False), (769, "strips=2", False),     # FX_MINDIST_MAX_L, then k_min_dist_long
    (1536, "strips=2", False), (1537, "strips=3", False),
)
LENGTHS = tuple(row[0] for row in LENGTH_FORMS)
REGISTER_LENGTHS = tuple(L for L in LENGTHS if L <= 768)       # k_min_dist / k_distances / k_distances_bounded
STRIP_LENGTHS = tuple(L for L in LENGTHS if L > 768)           # k_min_dist_long
CHUNK, FOUR_PASS_AT, STAGE_MAX_L, MAX_L = 1024, 512, 160, 768


def launcher_form(L):
    """The launchers' choice restated (mindist.hip fx_launch_min_dist): what LENGTH_FORMS is checked against on the host."""
    if L > MAX_L:
        return "strips=%d" % ((L + MAX_L - 1) // MAX_L), False
    if L <= 32:
        return "W=1 uint32_t", L <= STAGE_MAX_L
    words = (L + 63) // 64
    return "W=%d" % {1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 6, 7: 8, 8: 8}.get(words, 12), L <= STAGE_MAX_L


def passes(C, Q):
    """mindist.hip fx_dist_passes, restated: cache rows per block = passes x 256."""
    return 1 if ((C + CHUNK - 1) // CHUNK) * Q < FOUR_PASS_AT else CHUNK // 256


def long_query_batch(C, L, Q):
    """mindist.hip launch_long, restated: queries per launch so that the boundary scratch stays below 256 MiB."""
    per_query = ((C + CHUNK - 1) // CHUNK) * 256 * L
    return max(1, min(Q, (256 << 20) // per_query))


def boundary_positions(L):
    """Bit 63 and bit 0 of every 64-bit word (31 / 32 for the 32-bit form), the first and the last symbol."""
    pos = {0, L - 1, 31, 32}
    for k in range(64, L + 1, 64):
        pos.update((k - 1, k))
    return sorted(p for p in pos if 0 <= p < L)


def word_boundary_length(L):
    """A length that fills its last word exactly and lies inside a row of L bytes: the largest multiple of 64 below L
    (32 below 65: the boundary of the 32-bit form)."""
    if L > 64:
        return (L - 1) // 64 * 64
    return 32 if L > 32 else L // 2


def n_keys(L):
    return 300 if L <= MAX_L else (260 if L == 769 else 26)


def _substitute(s, positions, alpha):
    b = bytearray(s)
    for p in positions:
        b[p] = alpha[(alpha.index(b[p]) + 1 + p % (len(alpha) - 1)) % len(alpha)]       # always another letter
    return bytes(b)


def _spread(L, k, tail):
    """k distinct positions, boundary positions first (from the end of the row when `tail`)."""
    b = boundary_positions(L)
    cand = (b[::-1] if tail else b) + [p for p in np.linspace(1, L - 2, 9).astype(int).tolist()]
    out = []
    for p in cand:
        if p not in out and 0 <= p < L:
            out.append(p)
    return out[:k]


def build_case(L):
    """(queries, keys) as byte strings of at most L symbols (no NUL: `rows` pads them), families 1-6 of the module docstring of
    tests/test_gpu_distances.py.  Deterministic per L."""
    rng = np.random.default_rng(1000 + L)

    def rand(alpha, n):
        return bytes(np.frombuffer(alpha, np.uint8)[rng.integers(0, len(alpha), n)])

    parent = rand(AAS, L)
    wb = word_boundary_length(L)
    dna = rand(DNA, L)
    # queries: unrelated rows (1), one letter repeated (2, 3), the parent of the shifted copies and near-copies (4, 5), ragged ones (6)
    queries = [parent, b"A" * L, _substitute(parent[:wb], [wb - 1], AAS), b""]
    if L <= MAX_L:
        queries += [dna, rand(AAS, L), parent[:L // 3] + parent[L // 3 + 1:], b"A" * wb]
    keys = [b"C" * L,                                                    # 2: distance exactly L from "AAA..."
            b"A" * (L - 1), b"A" * (L // 2), b"A", b"",                  # 3, 6: shorter NUL-padded keys, a key of length 1, an empty key
            parent[1:] + parent[:1], parent[2:] + parent[:2], parent[3:] + parent[:3]]      # 4: shifted by 1, 2, 3
    for k in (1, 2, 3, 4, 5):                                            # 5: k substitutions on word boundaries (distance k: radius and radius + 1)
        keys.append(_substitute(parent, _spread(L, k, True), AAS))
        keys.append(_substitute(parent, _spread(L, k, False), AAS))
    keys += [parent[:wb], parent, dna, parent[:-1], parent[1:], b"A" * wb, rand(DNA, L), rand(AAS, L)]
    assert len(keys) == 26
    if n_keys(L) > len(keys):
        bp = boundary_positions(L)
        for p in bp:                                                     # 5: one edit exactly at bit 63 / bit 0 of a word
            keys.append(_substitute(parent, [p], AAS))
            keys.append(parent[:p] + parent[p + 1:])
        for p0, p1 in zip(bp, bp[1:]):
            keys.append(_substitute(parent, [p0, p1], AAS))
        keys = keys[:n_keys(L)]
        i = 0
        while len(keys) < n_keys(L):                                     # 1: unrelated rows over 4 and over 20 letters, a few ragged
            n = L if i % 7 else int(rng.integers(1, L + 1))
            keys.append(rand(DNA if i % 2 else AAS, n))
            i += 1
    order = rng.permutation(len(keys))                                   # every family on both sides of the 256-row block boundary
    return queries, [keys[i] for i in order]


def rows(seqs, L):
    """Byte strings -> (n, L) uint8 rows, NUL-padded on the right (the row format of fx_min_dist / fx_cache_*)."""
    out = np.zeros((len(seqs), L), np.uint8)
    for i, s in enumerate(seqs):
        assert len(s) <= L and 0 not in s
        out[i, :len(s)] = np.frombuffer(s, np.uint8)
    return out


def dp_matrices(queries, keys, L):
    """(Levenshtein, Hamming) int64 matrices by the DP oracle, pair by pair; Hamming over the padded rows (a pad against a
    letter is a mismatch, as in the kernels' header comment)."""
    qr, kr = rows(queries, L), rows(keys, L)
    lev = np.array([[c_oracle.levenshtein(q, k) for k in keys] for q in queries], np.int64).reshape(len(queries), len(keys))
    ham = np.array([[c_oracle.hamming(q, k) for k in kr] for q in qr], np.int64).reshape(len(queries), len(keys))
    return lev, ham


class Case:
    def __init__(self, L):
        self.L = L
        self.queries, self.keys = build_case(L)
        self.q_rows, self.k_rows = rows(self.queries, L), rows(self.keys, L)
        self.dist = dp_matrices(self.queries, self.keys, L)             # [mode]: 0 = Levenshtein, 1 = Hamming
        for a in (self.q_rows, self.k_rows) + self.dist:
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def reference(L):
    """The case of length L with its DP distances: built once per session, shared, read-only."""
    return Case(L)


def select(dist_row):
    """noisy_abstract_model.py:42-60 over one query's DP distances: (distance, index) by `ref_np.min_distance`."""
    d, i = ref_np.min_distance(None, range(len(dist_row)), lambda _q, i: int(dist_row[i]))
    return int(d), int(i)


def density(dist_row, fitness, radius):
    """dyna_ppo.py:106-114 over one query's DP distances: (density, neighbour count)."""
    dens, cnt = 0, 0
    for i, d in enumerate(dist_row):
        if d != 0 and d <= radius:
            dens += fitness[i] / int(d)
            cnt += 1
    return float(dens), cnt


def selection_case(L, C=2100):
    """Family 7, placed by hand at row width L (>= 20): C full-length keys unrelated to every query except the placed ones.
    Returns (queries, keys, expected [(distance, index)], what each query pins)."""
    rng = np.random.default_rng(7000 + L)
    keys_alpha = AAS[:19]                                                # 'P' is in no key

    def rand():
        return bytes(np.frombuffer(keys_alpha, np.uint8)[rng.integers(0, 19, L)])

    keys = [rand() for _ in range(C)]
    a, b, c, d, e = (rand() for _ in range(5))
    mid = L // 2
    keys[3] = a; keys[300] = _substitute(a, [L - 1], keys_alpha); keys[1500] = _substitute(a, [0], keys_alpha)
    keys[5] = b; keys[1500 + 1] = _substitute(b, [mid], keys_alpha)
    keys[255] = _substitute(c, [0, L - 1], keys_alpha); keys[256] = _substitute(c, [1, mid], keys_alpha)
    keys[1023] = _substitute(d, [0, mid], keys_alpha); keys[1024] = _substitute(d, [2, L - 1], keys_alpha)
    keys[700] = e; keys[1200] = e
    queries = [a, b, c, d, e, b"P" * L]
    expected = [(1, 300), (1, 1501), (2, 255), (2, 1023), (0, 700), (L, 0)]
    what = ["exact hit at 3, first distance-1 key in the second 256-row block, another in the second 1024-row chunk",
            "exact hit at 5, the only distance-1 key in the second 1024-row chunk",
            "distance 2 on either side of the 256-row block boundary", "distance 2 on either side of the 1024-row chunk boundary",
            "two exact hits, nothing at distance 1", "no key closer than L"]
    return queries, keys, expected, what
