// Stand-alone host check of flexs_amd/csrc/mutant_rank.h (the ranking of a parent's mutant neighbourhood that the enumeration
// kernel, the host row rebuild and this program share).  Built and run by tests/test_screen_mutants_host.py:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -g -O1 mutant_rank_check.cpp -o mutant_rank_check
// 1. every L <= 40, A in {2, 4, 20}, radius 2: unranking local = 0 .. B-1 walks exactly the nested loops of the definition
//    (d, then positions as itertools.combinations, then letters, the later position fastest), and rank() inverts it;
// 2. L in {237, 1024, 4096}: the first and the last local of every first position p of the pairs, and both ends of the singles;
// 3. the size functions at the 2^31 - 1 limit;
// 4. the kernel's per-thread body (fx_mutant_unit) run here over whole chunks, in heap buffers of exactly the sizes the launcher
//    promises (so the sanitizer sees any byte read or written outside them): rows and tail pad against strings built by the
//    definition's nested loops, and fx_mutant_row (the host rebuild) against the same.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../flexs_amd/csrc/mutant_rank.h"

static long long g_checks = 0;
#define CHECK(c)                                                                      \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } \
    } while (0)

static bool same(const FxMutant& a, const FxMutant& b) { return a.d == b.d && a.p == b.p && a.q == b.q && a.j1 == b.j1 && a.j2 == b.j2; }

static void exhaustive(int L, int A) {
    const int64_t B = fx_mutant_ball_size(L, A, 2), B1 = fx_mutant_ball_size(L, A, 1);
    CHECK(B1 == 1 + (int64_t)L * (A - 1));
    CHECK(B == B1 + (int64_t)L * (L - 1) / 2 * (A - 1) * (A - 1));
    int64_t local = 0;
    auto expect = [&](FxMutant want) {
        CHECK(local < B);
        const FxMutant got = fx_mutant_unrank((uint32_t)local, L, A);
        CHECK(same(got, want));
        CHECK(fx_mutant_rank(got, L, A) == local);
        ++local;
    };
    expect(FxMutant{0, 0, 0, 0, 0});
    for (int p = 0; p < L; ++p)
        for (int j = 0; j < A - 1; ++j) expect(FxMutant{1, p, 0, j, 0});
    CHECK(local == B1);
    for (int p = 0; p < L; ++p)
        for (int q = p + 1; q < L; ++q)
            for (int j1 = 0; j1 < A - 1; ++j1)
                for (int j2 = 0; j2 < A - 1; ++j2) expect(FxMutant{2, p, q, j1, j2});
    CHECK(local == B);
}

static void edges(int L, int A) {
    const int64_t B = fx_mutant_ball_size(L, A, 2), B1 = fx_mutant_ball_size(L, A, 1);
    CHECK(B > 0 && B1 > 0);
    const int a1 = A - 1;
    auto at = [&](int64_t local, FxMutant want) {
        CHECK(local >= 0 && local < B);
        const FxMutant got = fx_mutant_unrank((uint32_t)local, L, A);
        CHECK(same(got, want));
        CHECK(fx_mutant_rank(got, L, A) == local);
    };
    at(0, FxMutant{0, 0, 0, 0, 0});
    at(1, FxMutant{1, 0, 0, 0, 0});
    at(B1 - 1, FxMutant{1, L - 1, 0, a1 - 1, 0});
    int64_t pairs = 0;
    for (int p = 0; p + 1 < L; ++p) {                      // pairs (p, p+1) .. (p, L-1)
        CHECK(fx_mutant_pairs_before(L, p) == pairs);
        at(B1 + pairs * a1 * a1, FxMutant{2, p, p + 1, 0, 0});
        pairs += L - 1 - p;
        at(B1 + pairs * a1 * a1 - 1, FxMutant{2, p, L - 1, a1 - 1, a1 - 1});
        int pp, qq;
        fx_mutant_unrank_pair(L, pairs - 1, &pp, &qq);
        CHECK(pp == p && qq == L - 1);
    }
    CHECK(pairs == (int64_t)L * (L - 1) / 2);
    CHECK(B1 + pairs * a1 * a1 == B);
}

// the definition, literally: every parent's ball as strings
static std::vector<std::string> balls(const std::vector<std::string>& parents, const std::string& al, int radius) {
    std::vector<std::string> out;
    for (const std::string& s : parents) {
        const int L = (int)s.size();
        out.push_back(s);
        for (int p = 0; p < L; ++p)
            for (char c : al)
                if (c != s[p]) { std::string t = s; t[p] = c; out.push_back(t); }
        if (radius < 2) continue;
        for (int p = 0; p < L; ++p)
            for (int q = p + 1; q < L; ++q)
                for (char c1 : al)
                    for (char c2 : al)
                        if (c1 != s[p] && c2 != s[q]) { std::string t = s; t[p] = c1; t[q] = c2; out.push_back(t); }
    }
    return out;
}

static void stream(int L, const std::string& al, int radius, int P, int64_t chunk, unsigned seed) {
    const int A = (int)al.size();
    std::vector<std::string> parents;
    for (int i = 0; i < P; ++i) {
        std::string s(L, ' ');
        for (int c = 0; c < L; ++c) { seed = seed * 1664525u + 1013904223u; s[c] = al[(seed >> 16) % A]; }
        parents.push_back(s);
    }
    const std::vector<std::string> want = balls(parents, al, radius);
    const int64_t B = fx_mutant_ball_size(L, A, radius), total = fx_mutant_total_rows(P, B);
    CHECK(total == (int64_t)want.size());
    const size_t pl = (size_t)P * L;
    uint8_t* par = (uint8_t*)std::malloc(pl);
    uint8_t* codes = (uint8_t*)std::malloc(pl);
    uint8_t* alpha = (uint8_t*)std::calloc(256, 1);
    std::memcpy(alpha, al.data(), A);
    for (int i = 0; i < P; ++i)
        for (int c = 0; c < L; ++c) { par[(size_t)i * L + c] = (uint8_t)parents[i][c]; codes[(size_t)i * L + c] = (uint8_t)al.find(parents[i][c]); }
    std::vector<uint8_t> row(L);
    for (int64_t g = 0; g < total; ++g) {
        fx_mutant_row(g, L, A, B, par, codes, alpha, row.data());
        CHECK(std::memcmp(row.data(), want[g].data(), L) == 0);
    }
    for (int64_t row0 = 0; row0 < total; row0 += chunk) {
        const int64_t n = chunk < total - row0 ? chunk : total - row0;
        const int64_t units = (n * L + 16 + 15) / 16;      // as fx_launch_enumerate_mutants
        CHECK(units * 16 <= n * L + 32 && units * 16 >= n * L + 16);
        uint8_t* out = (uint8_t*)std::malloc((size_t)units * 16);
        for (int64_t u = 0; u < units; ++u) {
            const FxMutantUnit v = fx_mutant_unit(u, row0, n, L, A, (uint32_t)B, par, codes, alpha);
            std::memcpy(out + u * 16, &v.lo, 8);           // (little-endian host, as the device)
            std::memcpy(out + u * 16 + 8, &v.hi, 8);
        }
        for (int64_t r = 0; r < n; ++r) CHECK(std::memcmp(out + r * L, want[row0 + r].data(), L) == 0);
        for (int64_t b = n * L; b < units * 16; ++b) CHECK(out[b] == (uint8_t)al[0]);
        std::free(out);
    }
    std::free(par); std::free(codes); std::free(alpha);
}

int main() {
    const std::string protein = "ACDEFGHIKLMNPQRSTVWY";
    stream(8, "TGCA", 2, 5, 1 << 22, 1);
    stream(8, "TGCA", 2, 5, 304, 2);
    stream(5, "UGCA", 2, 3, 16, 3);
    stream(1, "UGCA", 2, 3, 16, 4);
    stream(1, "UGCA", 1, 1, 16, 5);
    stream(2, "AB", 2, 2, 16, 6);
    stream(16, "TGCA", 2, 2, 48, 7);
    stream(17, "TGCA", 1, 3, 32, 8);
    stream(30, protein, 2, 1, 65536, 9);
    stream(237, protein, 1, 2, 4096, 10);
    stream(33, protein, 2, 2, 1008, 11);
    const int As[3] = {2, 4, 20};
    for (int L = 1; L <= 40; ++L)
        for (int A : As) exhaustive(L, A);
    const int Ls[3] = {237, 1024, 4096};
    for (int L : Ls)
        for (int A : As) {
            if (fx_mutant_ball_size(L, A, 2) < 0) { CHECK(L == 4096 && A == 20); continue; }   // (3.0e9 rows: refused, nothing to unrank)
            edges(L, A);
        }
    edges(65535, 2);                                      // B = 2147450881: the longest parent whose radius-2 ball fits

    // the sizes the issue quotes
    CHECK(fx_mutant_ball_size(90, 20, 2) == 1447516);
    CHECK(fx_mutant_ball_size(237, 20, 2) == 10100230);
    CHECK(fx_mutant_ball_size(237, 20, 1) == 4504);
    CHECK(fx_mutant_ball_size(8, 4, 2) == 277);
    CHECK(fx_mutant_ball_size(1, 4, 2) == 4);
    CHECK(fx_mutant_ball_size(5, 1, 2) == 1);
    // radius and argument range
    CHECK(fx_mutant_ball_size(8, 4, 0) == -1 && fx_mutant_ball_size(8, 4, 3) == -1);
    CHECK(fx_mutant_ball_size(0, 4, 1) == -1 && fx_mutant_ball_size(8, 0, 1) == -1 && fx_mutant_ball_size(8, 257, 1) == -1);
    // B itself at the limit: 1 + L * 2 = 2^31 - 1 fits, 1 + L * 1 = 2^31 does not
    CHECK(fx_mutant_ball_size(1073741823, 3, 1) == 2147483647ll);
    CHECK(fx_mutant_ball_size(2147483647ll, 2, 1) == -1);
    CHECK(fx_mutant_ball_size(2147483647ll, 256, 2) == -1);
    CHECK(fx_mutant_ball_size(65535, 2, 2) == 2147450881ll);
    CHECK(fx_mutant_ball_size(65536, 2, 2) == -1);                           // 1 + 65536 + 2147450880 = 2147516417
    // P * B = 2^31 - 1 (a prime: 1 x B or P x 1) passes, 2^31 is refused
    CHECK(fx_mutant_total_rows(1, 2147483647ll) == 2147483647ll);
    CHECK(fx_mutant_total_rows(2147483647ll, 1) == 2147483647ll);
    CHECK(fx_mutant_total_rows(2147483648ll, 1) == -1);
    CHECK(fx_mutant_total_rows(1, 2147483648ll) == -1);
    const int64_t B16 = fx_mutant_ball_size(21845, 4, 1);                    // 1 + 21845 * 3 = 2^16
    CHECK(B16 == 65536);
    CHECK(fx_mutant_total_rows(32768, B16) == -1);                           // 2^31
    CHECK(fx_mutant_total_rows(32767, B16) == 2147418112ll);
    CHECK(fx_mutant_total_rows(0, 5) == -1 && fx_mutant_total_rows(5, 0) == -1);
    CHECK(fx_mutant_total_rows(212, 10100230) == 2141248760ll);              // GFP, radius 2: 212 parents fit, 213 do not
    CHECK(fx_mutant_total_rows(213, 10100230) == -1);
    std::printf("mutant_rank_check: ok (%lld checks)\n", g_checks);
    return 0;
}
