// Key map and digit / prefix arithmetic of the top-k select (topk.hip, K8), as host + device inlines: the device kernels, the
// launcher and the stand-alone host check (tests/native/topk_keys_check.cpp) compile the same text.
//
// Ordering rule (include/flexs_amd.h, fx_topk_dev): value order is NumPy's sort order read from the top -- NaN above +inf,
// -0.0 == +0.0, denormals keep their own rank -- and among equal values the lower index wins.  A float becomes a 32-bit key that
// is monotone in that value order; key << 32 | (0xFFFFFFFF - index) is then a 64-bit key that is DISTINCT for every element and
// whose plain unsigned order is the whole rule: the k best entries are the k largest 64-bit keys, largest first.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FX_TOPK_HD __host__ __device__ inline
#else
#define FX_TOPK_HD inline
#endif

#define FX_TOPK_MAX_K 4096          // k of one select (= SMALL_CALL_ROWS of the Python layer)
#define FX_TOPK_SMALL_MAX 8192      // elements the one-workgroup form sorts (64 KiB of LDS): k winners, or 2k candidates of a merge
#define FX_TOPK_DIGIT_BITS 8
#define FX_TOPK_BINS (1 << FX_TOPK_DIGIT_BITS)
#define FX_TOPK_PASSES (64 / FX_TOPK_DIGIT_BITS)

// float bits -> key, larger = better.  Every NaN (either sign, any payload) becomes ONE key above +inf; -0.0 becomes +0.0.
// Positive floats keep their order with the sign bit set; negative floats are complemented (more negative = smaller key).
// The smallest key any input has is that of -inf, 0x007FFFFF: key 0 never occurs, so an all-zero 64-bit key is free as padding.
FX_TOPK_HD uint32_t fx_topk_key32(uint32_t bits) {
    if ((bits & 0x7FFFFFFFu) > 0x7F800000u) bits = 0x7FC00000u;
    if (bits == 0x80000000u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
FX_TOPK_HD uint64_t fx_topk_key64(uint32_t bits, uint32_t index) {
    return ((uint64_t)fx_topk_key32(bits) << 32) | (uint64_t)(0xFFFFFFFFu - index);
}
FX_TOPK_HD uint32_t fx_topk_index_of(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

// Radix select, most significant digit first: pass p looks at bits [shift, shift + 8) of the keys whose higher bits equal the
// prefix chosen so far.
FX_TOPK_HD int fx_topk_shift(int pass) { return 64 - FX_TOPK_DIGIT_BITS * (pass + 1); }
FX_TOPK_HD uint64_t fx_topk_mask(int pass) {       // the bits the passes before `pass` have fixed
    return pass <= 0 ? 0ull : ~0ull << (64 - FX_TOPK_DIGIT_BITS * pass);
}
FX_TOPK_HD bool fx_topk_matches(uint64_t key, uint64_t prefix, int pass) { return ((key ^ prefix) & fx_topk_mask(pass)) == 0; }
FX_TOPK_HD int fx_topk_digit(uint64_t key, int pass) { return (int)((key >> fx_topk_shift(pass)) & (FX_TOPK_BINS - 1)); }

// The bin that holds the want-th largest (want >= 1) of the keys counted in hist[0 .. 256): the highest bin b with
// (keys in bins above b) < want <= (keys in bins b and above).  *above = keys in the bins above it: they are all winners, and
// the select goes on inside bin b for the remaining want - *above.  -1 when fewer than `want` keys were counted.
FX_TOPK_HD int fx_topk_pick_bin(const uint32_t* hist, uint32_t want, uint32_t* above) {
    uint32_t acc = 0;
    for (int b = FX_TOPK_BINS - 1; b >= 0; --b) {
        if (acc + hist[b] >= want) { *above = acc; return b; }
        acc += hist[b];
    }
    *above = acc;
    return -1;
}
// The same pick dealt to 64 lanes, four bins each: lane l holds the counts c[0 .. 4) of bins 4l .. 4l + 3 and above_lane = the keys
// in the bins of the lanes above it.  True on the one lane whose bins hold the want-th largest key (no lane when want == 0 or
// too few keys were counted).
FX_TOPK_HD bool fx_topk_pick_lane(const uint32_t c[4], uint32_t above_lane, uint32_t want, int lane, int* bin, uint32_t* above) {
    uint32_t acc = above_lane;
    for (int j = 3; j >= 0; --j) {
        if (acc < want && acc + c[j] >= want) { *bin = 4 * lane + j; *above = acc; return true; }
        acc += c[j];
    }
    return false;
}
FX_TOPK_HD uint64_t fx_topk_extend(uint64_t prefix, int bin, int pass) { return prefix | ((uint64_t)bin << fx_topk_shift(pass)); }
