// Stand-alone host check of csrc/fx_step_valid.h (the prepared step's per-call validity decision), built with the sanitizers:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -g -O1 step_valid_check.cpp -o step_valid_check
// No GPU, no HIP: the header is plain C++.  tests/test_step_valid_host.py compiles and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../flexs_amd/csrc/fx_step_valid.h"

static long long g_checks = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        ++g_checks;                                                                      \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

int main() {
    int engine_a = 0, engine_b = 0;                        // two addresses that stand for two engines
    const void* ea = &engine_a;
    const void* eb = &engine_b;

    for (int M = 1; M <= 17; ++M) {
        // exactly-sized heap arrays: a read past member M - 1 is the sanitizer's to find
        std::vector<FxStepMember> ok((size_t)M, FxStepMember{ea, 1});
        CHECK(fx_step_verdict(true, ea, ok.data(), M, 5, 5, true, 100, 128, true) == FX_STEP_GO);
        // the LUT: another generation, or no LUT on the engine at all, asks for the compare; never an error
        CHECK(fx_step_verdict(true, ea, ok.data(), M, 5, 6, true, 100, 128, true) == FX_STEP_GO_CHECK_LUT);
        CHECK(fx_step_verdict(true, ea, ok.data(), M, 0, 0, false, 100, 128, true) == FX_STEP_GO_CHECK_LUT);
        CHECK(fx_step_verdict(true, ea, ok.data(), M, ~0ull, 0, true, 100, 128, true) == FX_STEP_GO_CHECK_LUT);
        CHECK(fx_step_verdict(true, ea, ok.data(), M, ~0ull, ~0ull, true, 100, 128, true) == FX_STEP_GO);
        // rows: 0 <= N <= stride; N = 0 needs no input
        CHECK(fx_step_verdict(true, ea, ok.data(), M, 5, 5, true, 0, 128, false) == FX_STEP_GO);
        CHECK(fx_step_verdict(true, ea, ok.data(), M, 5, 5, true, 0, 0, false) == FX_STEP_GO);
        CHECK(fx_step_verdict(true, ea, ok.data(), M, 5, 5, true, 128, 128, true) == FX_STEP_GO);
        CHECK(fx_step_verdict(true, ea, ok.data(), M, 5, 5, true, 129, 128, true) == FX_STEP_BAD_ROWS);
        CHECK(fx_step_verdict(true, ea, ok.data(), M, 5, 5, true, -1, 128, true) == FX_STEP_BAD_ROWS);
        CHECK(fx_step_verdict(true, ea, ok.data(), M, 5, 5, true, INT64_MAX, INT64_MAX, true) == FX_STEP_GO);
        CHECK(fx_step_verdict(true, ea, ok.data(), M, 5, 5, true, INT64_MIN, INT64_MAX, true) == FX_STEP_BAD_ROWS);
        CHECK(fx_step_verdict(true, ea, ok.data(), M, 5, 5, true, 1, 128, false) == FX_STEP_NO_INPUT);
        // every single member stale in every way, every position
        for (int bad = 0; bad < M; ++bad) {
            std::vector<FxStepMember> v = ok;
            v[(size_t)bad].has_weights = 0;
            CHECK(fx_step_verdict(true, ea, v.data(), M, 5, 5, true, 100, 128, true) == FX_STEP_NO_WEIGHTS);
            v = ok;
            v[(size_t)bad].engine = eb;
            CHECK(fx_step_verdict(true, ea, v.data(), M, 5, 5, true, 100, 128, true) == FX_STEP_FOREIGN);
            v[(size_t)bad].engine = nullptr;
            CHECK(fx_step_verdict(true, ea, v.data(), M, 5, 5, true, 100, 128, true) == FX_STEP_FOREIGN);
            // the first stale member decides
            if (bad + 1 < M) {
                v = ok;
                v[(size_t)bad].has_weights = 0;
                v[(size_t)bad + 1].engine = eb;
                CHECK(fx_step_verdict(true, ea, v.data(), M, 5, 5, true, 100, 128, true) == FX_STEP_NO_WEIGHTS);
            }
        }
        // a member problem comes before a rows problem, a dead step before everything
        std::vector<FxStepMember> v = ok;
        v[0].has_weights = 0;
        CHECK(fx_step_verdict(true, ea, v.data(), M, 5, 5, true, -1, 128, false) == FX_STEP_NO_WEIGHTS);
    }
    // a dead step: the members are not read at all (null array, any M)
    CHECK(fx_step_verdict(false, ea, nullptr, 3, 5, 5, true, 100, 128, true) == FX_STEP_DEAD);
    CHECK(fx_step_verdict(true, nullptr, nullptr, 3, 5, 5, true, 100, 128, true) == FX_STEP_DEAD);
    CHECK(fx_step_verdict(false, nullptr, nullptr, 0, 0, 0, false, -1, 0, false) == FX_STEP_DEAD);
    // no members to look at (the library never creates such a step; the function must not read)
    CHECK(fx_step_verdict(true, ea, nullptr, 0, 1, 1, true, 4, 4, true) == FX_STEP_GO);
    std::printf("step_valid_check: ok (%lld checks)\n", g_checks);
    return 0;
}
