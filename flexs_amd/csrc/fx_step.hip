// C ABI of libflexs_amd.so: the PREPARED STEP (include/flexs_amd.h, "prepared step").  A caller that streams batches through the same members
// into the same buffers -- flexs_amd/distributed.py's launch / finish, one step per slot -- hands over once what stays the same between two
// steps (member handles, alphabet LUT, seq_len, planes, stride, mean and error-word destinations: fx_step_create validates them as
// fx_score_mean_planes_dev / fx_score_planes_dev do) and then issues a step with (rows, N).  fx_step_launch re-checks only what can go stale
// (fx_step_valid.h) and calls the SAME planner as the direct calls (score_then_mean / score_dispatch, fx_score.hip): every form decision,
// table build, counter and memset is theirs.  There is no cached launch here.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "fx_common.h"
#include "fx_internal.h"
#include "fx_step_valid.h"

struct fx_step {
    fx_engine* eng = nullptr;          // null once the engine is gone
    bool alive = false;                // false once the engine or one of the members is gone
    std::vector<fx_model*> models;
    std::vector<FxStepMember> view;    // (per call: what fx_step_verdict reads of the members)
    int L = 0;
    uint8_t lut[256];
    uint64_t lut_gen_seen = 0;         // fx_engine::lut_gen when the engine's LUT was last made (or found) this step's
    bool lut_seen = false;
    float* d_planes = nullptr;
    int64_t stride = 0;
    float* d_mean = nullptr;           // null: planes only (fx_score_planes_dev)
    float* d_err_word = nullptr;       // null: no error word behind the scores
};

extern "C" {

void fx_steps_forget_model(fx_model* m) {
    for (fx_step* s : m->eng->steps)
        if (std::find(s->models.begin(), s->models.end(), m) != s->models.end()) s->alive = false;
}

void fx_steps_forget_engine(fx_engine* e) {
    for (fx_step* s : e->steps) { s->alive = false; s->eng = nullptr; }
    e->steps.clear();
}

int fx_step_create(fx_engine* e, fx_model* const* models, int M, int L, const uint8_t lut[256], float* d_planes, int64_t stride,
                   float* d_mean, float* d_err_word, fx_step** out) {
    if (!out) return FX_EINVAL;
    *out = nullptr;
    int rc = validate_models(e, models, M, L, lut);
    if (rc) return rc;
    if (d_mean && M > 16) return fx_fail(e, FX_EINVAL, "fx_step_create: at most 16 members with a mean destination");
    if (stride < 0 || (stride & 3)) return fx_fail(e, FX_EINVAL, "fx_step_create: stride must be >= 0 and a multiple of 4");
    if (!d_planes || (reinterpret_cast<uintptr_t>(d_planes) & 15)) return fx_fail(e, FX_EINVAL, "fx_step_create: null or unaligned planes");
    if (((reinterpret_cast<uintptr_t>(d_mean) | reinterpret_cast<uintptr_t>(d_err_word)) & 3) != 0) return fx_fail(e, FX_EINVAL, "fx_step_create: unaligned destination");
    fx_step* s = new (std::nothrow) fx_step();
    if (!s) return FX_ENOMEM;
    s->eng = e;
    s->alive = true;
    s->models.assign(models, models + M);
    s->view.resize((size_t)M);
    s->L = L;
    std::memcpy(s->lut, lut, 256);
    s->d_planes = d_planes; s->stride = stride; s->d_mean = d_mean; s->d_err_word = d_err_word;
    e->steps.push_back(s);
    *out = s;
    return FX_OK;
}

int fx_step_launch(fx_step* s, const uint8_t* d_ascii, int64_t N) {
    if (!s) return FX_EINVAL;
    fx_engine* e = s->eng;
    const bool alive = s->alive && e;
    const int M = alive ? (int)s->models.size() : 0;
    for (int m = 0; m < M; ++m) s->view[m] = FxStepMember{s->models[m]->eng, s->models[m]->has_weights ? 1 : 0};
    const FxStepVerdict v = fx_step_verdict(alive, e, s->view.data(), M, s->lut_gen_seen, alive ? e->lut_gen : 0, alive && e->lut_valid && s->lut_seen,
                                            N, s->stride, d_ascii != nullptr);
    switch (v) {
        case FX_STEP_GO: case FX_STEP_GO_CHECK_LUT: break;
        case FX_STEP_DEAD: return fx_fail(e, FX_ESTATE, "fx_step_launch: the step's engine or one of its members was destroyed");
        case FX_STEP_FOREIGN: return fx_fail(e, FX_EINVAL, "model belongs to another engine");
        case FX_STEP_NO_WEIGHTS: return fx_fail(e, FX_ESTATE, "model weights were never set");
        case FX_STEP_BAD_ROWS: return fx_fail(e, FX_EINVAL, "fx_step_launch: N must be >= 0 and <= the step's stride");
        case FX_STEP_NO_INPUT: return fx_fail(e, FX_EINVAL, "null or unaligned buffer");
    }
    FX_HIP(e, hipSetDevice(e->device));
    int rc;
    if (N > 0) {
        if (v == FX_STEP_GO_CHECK_LUT) {
            // another call may have put its LUT on the device since: fx_upload_lut compares and, if so, uploads this step's again
            if ((rc = fx_upload_lut(e, s->lut))) return rc;
            s->lut_gen_seen = e->lut_gen;
            s->lut_seen = true;
        }
        e->counters.device_calls += 1; e->counters.sequences += N; e->counters.forwards += N * M;
        FxRequest rq; FxOutcome out;                       // (device rows)
        rq.stride = s->stride;
        rc = s->d_mean ? score_then_mean(e, s->models.data(), M, d_ascii, N, s->d_planes, s->d_mean, rq, out)
                       : score_dispatch(e, s->models.data(), M, d_ascii, N, s->d_planes, rq, out);
        if (rc) return rc;
    }
    return s->d_err_word ? fx_launch_error_word(e, s->d_err_word) : FX_OK;
}

int fx_step_destroy(fx_step* s) {
    if (!s) return FX_OK;
    if (s->eng) {
        auto& v = s->eng->steps;
        v.erase(std::remove(v.begin(), v.end(), s), v.end());
    }
    delete s;
    return FX_OK;
}

}  // extern "C"
