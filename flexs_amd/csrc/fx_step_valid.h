// The prepared step's per-call validity decision (fx_step.hip, fx_step_launch): what can go stale between two launches of one step, as a
// pure function of plain values -- O(M) integer compares, no HIP, no engine types -- so that the library and the stand-alone host check
// (tests/native/step_valid_check.cpp, built with the sanitizers) compile the same text.
// Everything else about a step -- the members' shapes against seq_len, the alphabet sizes, the 256-entry LUT range loop, the buffers'
// alignment -- is checked once, by fx_step_create.
#pragma once
#include <cstdint>

enum FxStepVerdict {
    FX_STEP_GO = 0,            // launch; the engine's device LUT is known to be this step's
    FX_STEP_GO_CHECK_LUT = 1,  // launch, but first let fx_upload_lut compare (and, if another call changed it, upload) the LUT
    FX_STEP_DEAD = 2,          // the engine or a member was destroyed: nothing the step holds may be touched
    FX_STEP_FOREIGN = 3,       // a member no longer belongs to the step's engine
    FX_STEP_NO_WEIGHTS = 4,    // a member has no weights
    FX_STEP_BAD_ROWS = 5,      // N < 0 or N > stride
    FX_STEP_NO_INPUT = 6,      // N > 0 rows at a null address
};

// what the step reads of one member per call (copied out of the fx_model only while the step is alive)
struct FxStepMember {
    const void* engine;        // the engine the member belongs to
    int has_weights;
};

// `alive`: no destroy has marked the step.  `members` is only read when alive (a dead step's member pointers dangle: the caller passes
// M = 0 or any array then).  lut_gen_seen: the engine's LUT generation when this step last made the engine's LUT its own;
// engine_lut_gen: the generation now (bumped by every upload of a different LUT); engine_lut_valid: the engine has uploaded one at all.
inline FxStepVerdict fx_step_verdict(bool alive, const void* step_engine, const FxStepMember* members, int M, uint64_t lut_gen_seen,
                                     uint64_t engine_lut_gen, bool engine_lut_valid, int64_t N, int64_t stride, bool have_rows) {
    if (!alive || !step_engine) return FX_STEP_DEAD;
    for (int m = 0; m < M; ++m) {
        if (members[m].engine != step_engine) return FX_STEP_FOREIGN;
        if (!members[m].has_weights) return FX_STEP_NO_WEIGHTS;
    }
    if (N < 0 || N > stride) return FX_STEP_BAD_ROWS;
    if (N > 0 && !have_rows) return FX_STEP_NO_INPUT;
    return (engine_lut_valid && lut_gen_seen == engine_lut_gen) ? FX_STEP_GO : FX_STEP_GO_CHECK_LUT;
}
