// Ranking of a parent's mutant neighbourhood (fx_screen_mutants, include/flexs_amd.h "screening"), as host + device inlines: the
// enumeration kernel (topk.hip k_enumerate_mutants), the host code that rebuilds the winners' rows (fx_screen.hip) and the
// stand-alone host check (tests/native/mutant_rank_check.cpp) compile the same text.
//
// The ball of a parent s of length L over an alphabet of A letters, radius r in {1, 2}, in this order:
//   local 0                           s itself
//   then d = 1: for p in 0 .. L-1, for j1 in 0 .. A-2:                  s with s[p] := letter(p, j1)
//   then d = 2: for (p, q), p < q, in the order of itertools.combinations(range(L), 2), for j1, for j2 (j2 fastest):
//                                                                        s with s[p] := letter(p, j1), s[q] := letter(q, j2)
// letter(p, j) = the j-th letter of the alphabet, in alphabet order, with the parent's own letter at p skipped.
// Ball size B = 1 + L (A-1) [+ C(L, 2) (A-1)^2 for r = 2]; with P parents global row g = parent * B + local, P * B <= 2^31 - 1.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FX_MUT_HD __host__ __device__ inline
#else
#define FX_MUT_HD inline
#endif

#define FX_MUT_MAX_ROWS 0x7FFFFFFFll

struct FxMutant { int d, p, q, j1, j2; };          // d changed positions: p (d >= 1) and q > p (d = 2), unused fields = 0

// B, or -1 when the arguments are out of range or B > 2^31 - 1 (no intermediate exceeds 2^62).
FX_MUT_HD int64_t fx_mutant_ball_size(int64_t L, int64_t A, int radius) {
    if (L < 1 || A < 1 || A > 256 || L > FX_MUT_MAX_ROWS || radius < 1 || radius > 2) return -1;
    const int64_t a1 = A - 1;
    if (a1 == 0) return 1;
    int64_t B = 1 + L * a1;                                   // < 2^39
    if (B > FX_MUT_MAX_ROWS) return -1;
    if (radius == 2) {
        const int64_t pairs = L * (L - 1) / 2;                // < 2^61
        if (pairs > (FX_MUT_MAX_ROWS - B) / (a1 * a1)) return -1;
        B += pairs * a1 * a1;
    }
    return B;
}

// P * B, or -1 when it exceeds 2^31 - 1 (or an argument is out of range).
FX_MUT_HD int64_t fx_mutant_total_rows(int64_t P, int64_t B) {
    if (P < 1 || B < 1 || B > FX_MUT_MAX_ROWS || P > FX_MUT_MAX_ROWS / B) return -1;
    return P * B;
}

// Pairs (p', q') of itertools.combinations(range(L), 2) that come before the first pair with first position p.
FX_MUT_HD int64_t fx_mutant_pairs_before(int64_t L, int64_t p) { return p * (2 * L - p - 1) / 2; }

// Pair number c in [0, C(L, 2)) -> (p, q).  p is the largest position with pairs_before(p) <= c: a float square root guesses it,
// integer steps settle it (the guess is never relied upon).
FX_MUT_HD void fx_mutant_unrank_pair(int64_t L, int64_t c, int* p_out, int* q_out) {
    const float t = (float)(2 * L - 1);
    const float disc = t * t - 8.0f * (float)c;
    int64_t p = (int64_t)((t - __builtin_sqrtf(disc > 0.0f ? disc : 0.0f)) * 0.5f);
    if (p < 0) p = 0;
    if (p > L - 2) p = L - 2;
    while (p < L - 2 && fx_mutant_pairs_before(L, p + 1) <= c) ++p;
    while (p > 0 && fx_mutant_pairs_before(L, p) > c) --p;
    *p_out = (int)p;
    *q_out = (int)(p + 1 + (c - fx_mutant_pairs_before(L, p)));
}

// local in [0, B) -> what is changed.  (local >= 1 needs A >= 2; a d = 2 local needs L >= 2: both follow from local < B.)
FX_MUT_HD FxMutant fx_mutant_unrank(uint32_t local, int L, int A) {
    FxMutant m = {0, 0, 0, 0, 0};
    if (local == 0) return m;
    const uint32_t a1 = (uint32_t)(A - 1);
    uint32_t t = local - 1;
    const uint64_t singles = (uint64_t)L * a1;
    if (t < singles) {
        m.d = 1;
        m.p = (int)(t / a1);
        m.j1 = (int)(t - (uint32_t)m.p * a1);
        return m;
    }
    t -= (uint32_t)singles;
    const uint32_t aa = a1 * a1;
    const uint32_t c = t / aa, rem = t - c * aa;
    m.d = 2;
    fx_mutant_unrank_pair(L, (int64_t)c, &m.p, &m.q);
    m.j1 = (int)(rem / a1);
    m.j2 = (int)(rem - (uint32_t)m.j1 * a1);
    return m;
}

// The inverse (the host check's round trip).
FX_MUT_HD int64_t fx_mutant_rank(const FxMutant& m, int64_t L, int64_t A) {
    const int64_t a1 = A - 1;
    if (m.d == 0) return 0;
    if (m.d == 1) return 1 + (int64_t)m.p * a1 + m.j1;
    const int64_t c = fx_mutant_pairs_before(L, m.p) + (m.q - m.p - 1);
    return 1 + L * a1 + c * a1 * a1 + (int64_t)m.j1 * a1 + m.j2;
}

// Letter index j (own letter skipped) -> index into the alphabet.
FX_MUT_HD int fx_mutant_letter(int j, int own) { return j + (j >= own ? 1 : 0); }

// Bytes [16 u, 16 u + 16) of the flat byte stream of rows [row0, row0 + n) of the enumeration (byte b = column b % L of row
// b / L; global row = parent * B + local), little end first in lo then hi: what one thread of the enumeration kernel stores.  A
// unit holds the tail of one row, whole rows where L < 16, and the head of the next; each piece is the parent's bytes with the
// row's changed columns patched where they fall into it.  Bytes past row n - 1 (the tail pad) are alphabet[0].  parents / codes:
// P x L ASCII / letter indices; row0 + n <= P * B.
struct FxMutantUnit { uint64_t lo, hi; };
FX_MUT_HD FxMutantUnit fx_mutant_unit(int64_t u, int64_t row0, int64_t n, int L, int A, uint32_t B, const uint8_t* parents,
                                      const uint8_t* codes, const uint8_t* alphabet) {
    FxMutantUnit v = {0, 0};
    auto put = [&](int at, uint64_t byte) {
        if (at < 8) v.lo |= byte << (8 * at); else v.hi |= byte << (8 * (at - 8));
    };
    int64_t row = u * 16 / L;
    int col = (int)(u * 16 - row * L);
    int k = 0;
    while (k < 16) {
        if (row >= n) {
            for (; k < 16; ++k) put(k, alphabet[0]);
            break;
        }
        const uint32_t g = (uint32_t)(row0 + row);
        const uint32_t par = g / B;
        const FxMutant m = fx_mutant_unrank(g - par * B, L, A);
        const uint8_t* ps = parents + (uint64_t)par * (uint64_t)L;
        const uint8_t* pc = codes + (uint64_t)par * (uint64_t)L;
        const int take = 16 - k < L - col ? 16 - k : L - col;
        int cp = -1, cq = -1;                              // changed columns, where they fall into this piece
        uint64_t lp = 0, lq = 0;
        if (m.d >= 1 && m.p >= col && m.p < col + take) { cp = m.p; lp = alphabet[fx_mutant_letter(m.j1, pc[m.p])]; }
        if (m.d == 2 && m.q >= col && m.q < col + take) { cq = m.q; lq = alphabet[fx_mutant_letter(m.j2, pc[m.q])]; }
        for (int i = 0; i < take; ++i) {
            const int c = col + i;
            put(k + i, c == cp ? lp : c == cq ? lq : (uint64_t)ps[c]);
        }
        k += take;
        col = 0;
        ++row;
    }
    return v;
}

// Row g of the enumeration into out[0 .. L): the parent with at most two bytes changed (the host's rebuild of a winner's row).
FX_MUT_HD void fx_mutant_row(int64_t g, int L, int A, int64_t B, const uint8_t* parents, const uint8_t* codes, const uint8_t* alphabet,
                             uint8_t* out) {
    const int64_t par = g / B;
    const FxMutant m = fx_mutant_unrank((uint32_t)(g - par * B), L, A);
    const uint8_t* ps = parents + (uint64_t)par * (uint64_t)L;
    const uint8_t* pc = codes + (uint64_t)par * (uint64_t)L;
    for (int c = 0; c < L; ++c) out[c] = ps[c];
    if (m.d >= 1) out[m.p] = alphabet[fx_mutant_letter(m.j1, pc[m.p])];
    if (m.d == 2) out[m.q] = alphabet[fx_mutant_letter(m.j2, pc[m.q])];
}
