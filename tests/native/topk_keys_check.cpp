// Stand-alone host check of flexs_amd/csrc/topk_keys.h -- the key map and the digit / prefix / bin arithmetic the top-k select
// kernels (csrc/topk.hip) are compiled from.  Built with -fsanitize=address,undefined and run by tests/test_screen_host.py:
//   1. the 32-bit key is monotone in the ordering rule (NumPy's sort order: NaN above +inf, -0.0 == +0.0, denormals ranked) on
//      the edge values and on a few million random bit patterns, and equal exactly where the rule says "equal";
//   2. the 64-bit key breaks ties by the lower index and gives the index back;
//   3. a radix select written with the header's functions alone -- per-pass histograms, the serial and the 64-lane bin pick --
//      finds the k-th largest key of random, skewed and all-equal inputs; every histogram access goes through a bounds-checked
//      vector.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../flexs_amd/csrc/topk_keys.h"

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 16); }

static float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
static uint32_t to_bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

// the rule, stated on floats: -1 / 0 / +1 for "a ranks below / with / above b"
static int rule_cmp(float a, float b) {
    const bool na = std::isnan(a), nb = std::isnan(b);
    if (na || nb) return (int)na - (int)nb;
    return a < b ? -1 : (a > b ? 1 : 0);
}
static int key_cmp(uint32_t a, uint32_t b) { return a < b ? -1 : (a > b ? 1 : 0); }

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("topk_keys_check: FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

static int check_pair(uint32_t a, uint32_t b) {
    const int want = rule_cmp(from_bits(a), from_bits(b)), got = key_cmp(fx_topk_key32(a), fx_topk_key32(b));
    CHECK(want == got, "bits %08x vs %08x: rule %d, keys %d", a, b, want, got);
    return 0;
}

// the k-th largest (k >= 1) of keys[], by the passes of the device code
static int radix_kth(const std::vector<uint64_t>& keys, uint32_t k, uint64_t* out) {
    uint64_t prefix = 0;
    uint32_t want = k;
    for (int pass = 0; pass < FX_TOPK_PASSES; ++pass) {
        std::vector<uint32_t> hist(FX_TOPK_BINS, 0);
        for (uint64_t key : keys)
            if (fx_topk_matches(key, prefix, pass)) hist.at((size_t)fx_topk_digit(key, pass)) += 1;
        uint32_t above = 0;
        const int bin = fx_topk_pick_bin(hist.data(), want, &above);
        CHECK(bin >= 0 && bin < FX_TOPK_BINS, "pass %d: no bin for want %u", pass, want);
        // the same pick as the 64 lanes of a wave make it
        int found = 0, lane_bin = -1;
        uint32_t lane_above = 0;
        for (int lane = 0; lane < 64; ++lane) {
            uint32_t above_lane = 0;
            for (size_t b = (size_t)4 * lane + 4; b < hist.size(); ++b) above_lane += hist.at(b);
            int b2 = -1; uint32_t a2 = 0;
            if (fx_topk_pick_lane(&hist.at((size_t)4 * lane), above_lane, want, lane, &b2, &a2)) { ++found; lane_bin = b2; lane_above = a2; }
        }
        CHECK(found == 1 && lane_bin == bin && lane_above == above, "pass %d: lanes found %d, bin %d vs %d, above %u vs %u", pass, found, lane_bin, bin, lane_above, above);
        CHECK(above < want && want - above <= hist.at((size_t)bin), "pass %d: want %u, above %u, in bin %u", pass, want, above, hist.at((size_t)bin));
        prefix = fx_topk_extend(prefix, bin, pass);
        want -= above;
    }
    CHECK(want == 1, "keys are distinct: one key left, not %u", want);
    *out = prefix;
    return 0;
}

int main() {
    // 1. edge values, every pair
    const uint32_t edges[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007FFFFFu, 0x00800000u, 0x3F800000u, 0xBF800000u,
                              0x7F7FFFFFu, 0xFF7FFFFFu, 0x7F800000u, 0xFF800000u, 0x7FC00000u, 0xFFC00000u, 0x7F800001u, 0xFFFFFFFFu,
                              0x7FFFFFFFu, 0x33800000u, 0xB3800000u};
    for (uint32_t a : edges)
        for (uint32_t b : edges)
            if (check_pair(a, b)) return 1;
    CHECK(fx_topk_key32(0xFF800000u) == 0x007FFFFFu, "-inf is the smallest key");
    for (uint32_t a : edges) CHECK(fx_topk_key32(a) >= 0x007FFFFFu, "no key below -inf's (0 is the padding key)");
    // ... and a few million random pairs: raw bit patterns (NaNs and denormals included) and near neighbours
    for (int i = 0; i < 4000000; ++i) {
        const uint32_t a = (rnd() << 16) ^ rnd(), b = (i & 1) ? a + (rnd() % 5) - 2 : (rnd() << 16) ^ rnd();
        if (check_pair(a, b)) return 1;
        if (check_pair(a, a ^ 0x80000000u)) return 1;
    }
    // 2. ties go to the lower index; the index comes back
    for (int i = 0; i < 100000; ++i) {
        const uint32_t bits = (rnd() << 16) ^ rnd(), lo = rnd() % 0x7FFFFFFFu, hi = lo + 1 + rnd() % (0x7FFFFFFFu - lo);
        CHECK(fx_topk_key64(bits, lo) > fx_topk_key64(bits, hi), "equal values: index %u must beat %u", lo, hi);
        CHECK(fx_topk_index_of(fx_topk_key64(bits, hi)) == hi, "index round trip");
    }
    CHECK(fx_topk_key64(0x80000000u, 5) > fx_topk_key64(0x00000000u, 6) && fx_topk_key64(0x00000000u, 5) > fx_topk_key64(0x80000000u, 6), "-0.0 and +0.0 tie");
    CHECK(fx_topk_mask(0) == 0 && fx_topk_mask(1) == 0xFF00000000000000ull && fx_topk_mask(FX_TOPK_PASSES) == ~0ull, "prefix masks");
    CHECK(fx_topk_shift(0) == 56 && fx_topk_shift(FX_TOPK_PASSES - 1) == 0, "digit shifts");
    // 3. radix select against a sort
    const float pool[] = {0.f, -0.f, INFINITY, -INFINITY, NAN, 1e-45f, -3.4028235e38f, 1.f};
    for (int trial = 0; trial < 300; ++trial) {
        const int n = 1 + (int)(rnd() % 3000), fill = trial % 4;
        std::vector<uint64_t> keys((size_t)n);
        for (int i = 0; i < n; ++i) {
            uint32_t bits;
            if (fill == 0) bits = (rnd() << 16) ^ rnd();
            else if (fill == 1) bits = to_bits(pool[rnd() % 8]);
            else if (fill == 2) bits = to_bits(1.5f);
            else bits = to_bits((float)(int)(rnd() % 7) - 3.f);
            keys[(size_t)i] = fx_topk_key64(bits, (uint32_t)i);
        }
        std::vector<uint64_t> sorted = keys;
        std::sort(sorted.begin(), sorted.end(), [](uint64_t a, uint64_t b) { return a > b; });
        const uint32_t ks[] = {1u, (uint32_t)n, 1u + rnd() % (uint32_t)n, (uint32_t)std::min(n, 100)};
        for (uint32_t k : ks) {
            uint64_t kth = 0;
            if (radix_kth(keys, k, &kth)) return 1;
            CHECK(kth == sorted.at(k - 1), "trial %d (fill %d, n %d, k %u): k-th key %016llx, sort says %016llx", trial, fill, n, k,
                  (unsigned long long)kth, (unsigned long long)sorted.at(k - 1));
        }
    }
    std::printf("topk_keys_check: ok\n");
    return 0;
}
