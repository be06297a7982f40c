"""Host side of the conv2 prefix tables (csrc/pack.cpp, fx_common.h; no GPU): where they lie behind a member's packed image, and which row
of them a conv position of a seq_len = 8 row reads (fx_c2p_row, the scoring kernel's own index function)."""
import numpy as np

from flexs_amd import _native

L, A, F, H, K = 8, 4, 32, 100, 5
PACKED_FLOATS = 26500             # the packed image of this shape before the tables existed (fx_debug_packed_size)


def test_packed_image_is_unchanged_and_tables_lie_behind_it():
    lay = _native.debug_pack_layout(_native.FX_CNN, L, A, F, H, K)
    tab = _native.debug_table_layout(_native.FX_CNN, L, A, F, H, K)
    assert _native.lib().fx_debug_packed_size(_native.FX_CNN, L, A, F, H, K) == PACKED_FLOATS
    assert tab["alloc_floats"] == PACKED_FLOATS == lay["total_floats"]
    # conv1 table, then depth 1 (3 families x 4^5 rows), then depth 2 (3 x 4^6), rows of 32 floats = whole 128-byte lines
    at = (PACKED_FLOATS + 31) // 32 * 32
    for off, size, rows in (("off_c1tab", "c1tab_floats", 1024), ("off_c2p1", "c2p1_floats", 3 * 4 ** 5), ("off_c2p2", "c2p2_floats", 3 * 4 ** 6)):
        assert tab[off] == at and tab[off] % 32 == 0, (off, tab)
        assert tab[size] == rows * 32, (size, tab)
        at += tab[size]
    assert tab["dev_floats"] == at and tab["dev_floats"] % 32 == 0
    assert tab["c2p1_floats"] * 4 == 3 * 128 * 1024 and tab["c2p2_floats"] * 4 == 3 * 512 * 1024
    assert tab["dev_floats"] * 4 < 2 ** 31                # the kernels address the buffer with 32-bit byte offsets


def test_other_shapes_carry_no_tables():
    for shape in ((_native.FX_CNN, 14, 4, 32, 100, 5), (_native.FX_CNN, 8, 4, 32, 200, 5), (_native.FX_CNN, 8, 20, 32, 100, 5),
                  (_native.FX_MLP, 8, 4, 0, 100, 0), (_native.FX_GE, 8, 4, 0, 100, 0)):
        tab = _native.debug_table_layout(*shape)
        assert tab["alloc_floats"] == _native.lib().fx_debug_packed_size(*shape)
        assert tab["dev_floats"] == tab["alloc_floats"], shape
        assert (tab["off_c1tab"], tab["off_c2p1"], tab["off_c2p2"]) == (-1, -1, -1), shape
        assert (tab["c1tab_floats"], tab["c2p1_floats"], tab["c2p2_floats"]) == (0, 0, 0), shape


def test_row_index_of_every_position_against_a_direct_enumeration():
    """conv2 is 'same' with five taps over the four conv1 outputs: tap j of position p reads out1[p + j - 2].  The row a position reads is
    (its first valid tap) * 4^(4 + depth) + the letters of its first `depth` windows as a base-4 number, lowest letter first."""
    rng = np.random.default_rng(0)
    codes = np.unique(np.concatenate([rng.integers(0, 4 ** 8, 3000), [0, 4 ** 8 - 1, 0x5555, 0xAAAA, 0x00FF, 0xFF00, 1, 1 << 15]]))
    seen = {1: set(), 2: set()}
    for c in codes:
        c = int(c)
        letters = [(c >> (2 * i)) & 3 for i in range(8)]
        for p in range(4):
            taps = [j for j in range(5) if 0 <= p + j - 2 < 4]
            j0, window = taps[0], p + taps[0] - 2
            assert (p, j0, window) in ((0, 2, 0), (1, 1, 0), (2, 0, 0), (3, 0, 1))
            for depth in (1, 2):
                assert taps[:depth] == list(range(j0, j0 + depth))          # the tabulated taps are valid and consecutive
                idx = sum(letters[window + i] * 4 ** i for i in range(4 + depth))
                row = _native.debug_conv2_prefix_row(c, p, depth)
                assert row == j0 * 4 ** (4 + depth) + idx, (c, p, depth)
                assert 0 <= row < 3 * 4 ** (4 + depth)
                seen[depth].add(row // 4 ** (4 + depth))
    assert seen == {1: {0, 1, 2}, 2: {0, 1, 2}}
    # whatever the codes word holds above its 16 bits, the row stays inside the tables
    for depth in (1, 2):
        for p in range(4):
            assert _native.debug_conv2_prefix_row(0xFFFFFFFF, p, depth) < 3 * 4 ** (4 + depth)
