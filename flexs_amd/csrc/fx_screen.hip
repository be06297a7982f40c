// C ABI of libflexs_amd.so, screening (include/flexs_amd.h "screening"): the top-k select alone (fx_topk*), behind a scoring call
// (fx_score_topk*), over the model's whole sequence space (fx_screen_all) and over the single and double mutants of a list of parents
// (fx_screen_mutants; the order of a parent's neighbourhood: mutant_rank.h).  Kernels: topk.hip.
//
// Engine scratch slots used here (none of them by any other entry point): 6 the select's work area (topk.hip), 7 rows (an upload,
// or a chunk of the enumeration), 8 scores, 9 winners -- the (index, value) pairs a host call copies out, and the candidate
// buffers of fx_screen_all / fx_screen_mutants, 10 the parents of fx_screen_mutants (ASCII, letter indices, the alphabet).  They grow to the largest
// call and stay: nothing is allocated per call after the first of a size.
#include <algorithm>
#include <cstring>

#include "fx_common.h"
#include "fx_internal.h"
#include "mutant_rank.h"
#include "topk_keys.h"

namespace {

// fx_screen_all / host calls: two candidate buffers of 2k entries each (running winners followed by a chunk's), and each of them as
// indices + values
struct Winners {
    int64_t* idx[2];
    float* val[2];
};
int winners_buffers(fx_engine* e, Winners* w) {
    void* p = nullptr;
    const size_t cap = 2 * FX_TOPK_MAX_K;
    if (int rc = fx_scratch(e, 9, 2 * cap * (sizeof(int64_t) + sizeof(float)), &p)) return rc;
    w->idx[0] = (int64_t*)p;
    w->idx[1] = w->idx[0] + cap;
    w->val[0] = (float*)(w->idx[1] + cap);
    w->val[1] = w->val[0] + cap;
    return FX_OK;
}

int check_select(fx_engine* e, int64_t N, int k, int* out_count) {
    if (!e || !out_count) return FX_EINVAL;
    if (k < 1 || k > FX_TOPK_MAX_K) return fx_fail(e, FX_ESHAPE, "k must be 1 .. 4096");
    if (N < 0) return fx_fail(e, FX_EINVAL, "negative number of scores");
    if (N > 0x7FFFFFFFll) return fx_fail(e, FX_ESHAPE, "a select takes fewer than 2^31 scores");
    return FX_OK;
}

// scores of the members (M = 1) or their NumPy-order mean (M > 1) for N resident rows, into d_scores: fx_score_dev's own paths
int score_for_select(fx_engine* e, fx_model* const* models, int M, const uint8_t* d_ascii, int64_t N, int L, const uint8_t lut[256], float* d_scores) {
    return fx_score_dev(e, models, M, d_ascii, N, L, lut, M == 1 ? d_scores : nullptr, M == 1 ? nullptr : d_scores);
}

int copy_winners_out(fx_engine* e, const int64_t* d_idx, const float* d_val, int count, int64_t* idx, float* val) {
    FX_HIP(e, hipMemcpyAsync(idx, d_idx, sizeof(int64_t) * (size_t)count, hipMemcpyDeviceToHost, e->stream));
    FX_HIP(e, hipMemcpyAsync(val, d_val, sizeof(float) * (size_t)count, hipMemcpyDeviceToHost, e->stream));
    FX_HIP(e, hipStreamSynchronize(e->stream));
    e->counters.bytes_d2h += (int64_t)count * 12;
    return FX_OK;
}

}  // namespace

extern "C" {

int fx_topk_dev(fx_engine* e, const float* d_scores, int64_t N, int k, int64_t* d_idx, float* d_val, int* out_count) {
    if (int rc = check_select(e, N, k, out_count)) return rc;
    *out_count = (int)std::min<int64_t>(k, N);
    if (N == 0) return FX_OK;
    if (!d_scores || !d_idx || !d_val) return fx_fail(e, FX_EINVAL, "null buffer");
    FX_HIP(e, hipSetDevice(e->device));
    lp_disarm(e);                                          // (a pre-launched scoring instance holds most CUs until its idle limit)
    return fx_launch_topk(e, d_scores, N, *out_count, 0, d_idx, d_val);
}

int fx_topk(fx_engine* e, const float* scores, int64_t N, int k, int64_t* idx, float* val, int* out_count) {
    if (int rc = check_select(e, N, k, out_count)) return rc;
    *out_count = (int)std::min<int64_t>(k, N);
    if (N == 0) return FX_OK;
    if (!scores || !idx || !val) return fx_fail(e, FX_EINVAL, "null buffer");
    FX_HIP(e, hipSetDevice(e->device));
    lp_disarm(e);
    void* d_s = nullptr;
    Winners w;
    int rc;
    if ((rc = fx_scratch(e, 8, sizeof(float) * (size_t)N, &d_s))) return rc;
    if ((rc = winners_buffers(e, &w))) return rc;
    FX_HIP(e, hipMemcpyAsync(d_s, scores, sizeof(float) * (size_t)N, hipMemcpyHostToDevice, e->stream));
    e->counters.bytes_h2d += 4 * N;
    if ((rc = fx_launch_topk(e, (const float*)d_s, N, *out_count, 0, w.idx[0], w.val[0]))) return rc;
    return copy_winners_out(e, w.idx[0], w.val[0], *out_count, idx, val);
}

int fx_score_topk_dev(fx_engine* e, fx_model* const* models, int M, const uint8_t* d_ascii, int64_t N, int L, const uint8_t lut[256], int k,
                      int64_t* d_idx, float* d_val, int* out_count) {
    int rc = validate_models(e, models, M, L, lut);
    if (rc) return rc;
    if ((rc = check_select(e, N, k, out_count))) return rc;
    *out_count = (int)std::min<int64_t>(k, N);
    if (N == 0) return FX_OK;
    if (!d_ascii || !d_idx || !d_val) return fx_fail(e, FX_EINVAL, "null buffer");
    FX_HIP(e, hipSetDevice(e->device));
    void* d_s = nullptr;
    if ((rc = fx_scratch(e, 8, sizeof(float) * (size_t)N, &d_s))) return rc;
    if ((rc = score_for_select(e, models, M, d_ascii, N, L, lut, (float*)d_s))) return rc;
    return fx_launch_topk(e, (const float*)d_s, N, *out_count, 0, d_idx, d_val);
}

int fx_score_topk(fx_engine* e, fx_model* const* models, int M, const uint8_t* ascii, int64_t N, int L, const uint8_t lut[256], int k,
                  int64_t* idx, float* val, int* out_count) {
    int rc = validate_models(e, models, M, L, lut);
    if (rc) return rc;
    if ((rc = check_select(e, N, k, out_count))) return rc;
    *out_count = (int)std::min<int64_t>(k, N);
    if (N == 0) return FX_OK;
    if (!ascii || !idx || !val) return fx_fail(e, FX_EINVAL, "null buffer");
    FX_HIP(e, hipSetDevice(e->device));
    const size_t in_bytes = (size_t)N * (size_t)L;
    void *d_in = nullptr, *d_s = nullptr;
    Winners w;
    if ((rc = fx_scratch(e, 7, in_bytes + 16, &d_in))) return rc;
    if ((rc = fx_scratch(e, 8, sizeof(float) * (size_t)N, &d_s))) return rc;
    if ((rc = winners_buffers(e, &w))) return rc;
    FX_HIP(e, hipMemcpyAsync(d_in, ascii, in_bytes, hipMemcpyHostToDevice, e->stream));
    e->counters.host_calls += 1; e->counters.bytes_h2d += (int64_t)in_bytes;
    if ((rc = score_for_select(e, models, M, (const uint8_t*)d_in, N, L, lut, (float*)d_s))) return rc;
    if ((rc = fx_launch_topk(e, (const float*)d_s, N, *out_count, 0, w.idx[0], w.val[0]))) return rc;
    // a character outside the alphabet: FX_EBADCHAR, nothing written (as fx_score)
    FX_HIP(e, hipStreamSynchronize(e->stream));
    if ((rc = check_deferred(e))) return rc;
    return copy_winners_out(e, w.idx[0], w.val[0], *out_count, idx, val);
}

int fx_screen_all(fx_engine* e, fx_model* const* models, int M, int L, int A, const uint8_t* alphabet, const uint8_t lut[256], int k,
                  int64_t* idx, uint8_t* rows_kxL, float* val, int* out_count) {
    int rc = validate_models(e, models, M, L, lut);
    if (rc) return rc;
    if (!alphabet || !idx || !rows_kxL || !val || !out_count) return fx_fail(e, FX_EINVAL, "null buffer");
    if (k < 1 || k > FX_TOPK_MAX_K) return fx_fail(e, FX_ESHAPE, "k must be 1 .. 4096");
    if (A != models[0]->shape.A) return fx_fail(e, FX_ESHAPE, "alphabet size does not match the model's");
    for (int a = 0; a < A; ++a)
        if (lut[alphabet[a]] == 0xFF) return fx_fail(e, FX_EINVAL, "an alphabet letter is missing from the LUT");
    int64_t total = 1;
    for (int p = 0; p < L; ++p) {
        total *= A;
        if (total > 0x7FFFFFFFll) return fx_fail(e, FX_ESHAPE, "the sequence space has more than 2^31 - 1 rows");
    }
    FX_HIP(e, hipSetDevice(e->device));
    const int64_t chunk = std::min<int64_t>(e->screen_chunk_rows, (total + 15) / 16 * 16);
    void *d_rows = nullptr, *d_s = nullptr;
    Winners w;
    if ((rc = fx_scratch(e, 7, (size_t)chunk * (size_t)L + 16, &d_rows))) return rc;
    if ((rc = fx_scratch(e, 8, sizeof(float) * (size_t)chunk, &d_s))) return rc;
    if ((rc = winners_buffers(e, &w))) return rc;
    e->counters.host_calls += 1;
    int cur = 0, have = 0;                                 // buffer that holds the running winners, and how many
    for (int64_t row0 = 0; row0 < total; row0 += chunk) {
        const int64_t rows = std::min(chunk, total - row0);
        const int take = (int)std::min<int64_t>(k, rows);
        if ((rc = fx_launch_enumerate_rows(e, (uint8_t*)d_rows, row0, rows, L, A, alphabet))) return rc;
        if ((rc = score_for_select(e, models, M, (const uint8_t*)d_rows, rows, L, lut, (float*)d_s))) return rc;
        // the chunk's winners, with GLOBAL row numbers, behind the running ones; then the best k of both
        if ((rc = fx_launch_topk(e, (const float*)d_s, rows, take, row0, w.idx[cur] + have, w.val[cur] + have))) return rc;
        if (have == 0) { have = take; continue; }
        const int keep = std::min(k, have + take);
        if ((rc = fx_launch_topk_merge(e, w.idx[cur], w.val[cur], have + take, keep, w.idx[cur ^ 1], w.val[cur ^ 1]))) return rc;
        cur ^= 1;
        have = keep;
    }
    FX_HIP(e, hipStreamSynchronize(e->stream));
    if ((rc = check_deferred(e))) return rc;
    if ((rc = copy_winners_out(e, w.idx[cur], w.val[cur], have, idx, val))) return rc;
    for (int j = 0; j < have; ++j) {                       // the winners' rows from their numbers (no row of a loser ever leaves the device)
        int64_t v = idx[j];
        for (int p = L - 1; p >= 0; --p) { rows_kxL[(size_t)j * L + p] = alphabet[v % A]; v /= A; }
    }
    *out_count = have;
    return FX_OK;
}

int fx_screen_mutants(fx_engine* e, fx_model* const* models, int M, const uint8_t* parents_PxL, int64_t P, int L, int A, const uint8_t* alphabet,
                      const uint8_t lut[256], int radius, int k, int64_t* idx, uint8_t* rows_kxL, float* val, int* out_count) {
    int rc = validate_models(e, models, M, L, lut);
    if (rc) return rc;
    if (!parents_PxL || !alphabet || !idx || !rows_kxL || !val || !out_count) return fx_fail(e, FX_EINVAL, "null buffer");
    if (k < 1 || k > FX_TOPK_MAX_K) return fx_fail(e, FX_ESHAPE, "k must be 1 .. 4096");
    if (radius < 1 || radius > 2) return fx_fail(e, FX_ESHAPE, "radius must be 1 or 2");
    if (P < 1) return fx_fail(e, FX_ESHAPE, "at least one parent");
    if (A != models[0]->shape.A) return fx_fail(e, FX_ESHAPE, "alphabet size does not match the model's");
    for (int a = 0; a < A; ++a)
        if (lut[alphabet[a]] != a) return fx_fail(e, FX_EINVAL, "the alphabet does not match the LUT");
    const int64_t B = fx_mutant_ball_size(L, A, radius);
    const int64_t total = B < 0 ? -1 : fx_mutant_total_rows(P, B);
    if (total < 0) return fx_fail(e, FX_ESHAPE, "the parents' mutant neighbourhoods have more than 2^31 - 1 rows");
    // the kernel's inputs: parents | their letter indices | alphabet (256 bytes); a byte outside the LUT is refused here, before any launch
    const size_t pl = (size_t)P * (size_t)L;
    if (e->mutant_stage.size() < 2 * pl + 256) e->mutant_stage.resize(2 * pl + 256);
    uint8_t* stage = e->mutant_stage.data();
    for (size_t i = 0; i < pl; ++i) {
        const uint8_t code = lut[parents_PxL[i]];
        if (code == 0xFF || code >= A) return fx_fail(e, FX_EBADCHAR, "substring not found: character outside the alphabet");
        stage[i] = parents_PxL[i];
        stage[pl + i] = code;
    }
    for (int i = 0; i < 256; ++i) stage[2 * pl + i] = i < A ? alphabet[i] : 0;
    FX_HIP(e, hipSetDevice(e->device));
    const int64_t chunk = std::min<int64_t>(e->screen_chunk_rows, (total + 15) / 16 * 16);
    void *d_rows = nullptr, *d_s = nullptr, *d_par = nullptr;
    Winners w;
    if ((rc = fx_scratch(e, 7, (size_t)chunk * (size_t)L + 32, &d_rows))) return rc;
    if ((rc = fx_scratch(e, 8, sizeof(float) * (size_t)chunk, &d_s))) return rc;
    if ((rc = fx_scratch(e, 10, 2 * pl + 256, &d_par))) return rc;
    if ((rc = winners_buffers(e, &w))) return rc;
    FX_HIP(e, hipMemcpyAsync(d_par, stage, 2 * pl + 256, hipMemcpyHostToDevice, e->stream));
    e->counters.host_calls += 1; e->counters.bytes_h2d += (int64_t)(2 * pl + 256);
    const uint8_t* d_parents = (const uint8_t*)d_par;
    int cur = 0, have = 0;                                 // as fx_screen_all
    for (int64_t row0 = 0; row0 < total; row0 += chunk) {
        const int64_t rows = std::min(chunk, total - row0);
        const int take = (int)std::min<int64_t>(k, rows);
        if ((rc = fx_launch_enumerate_mutants(e, (uint8_t*)d_rows, row0, rows, L, A, B, P, d_parents, d_parents + pl, d_parents + 2 * pl))) return rc;
        if ((rc = score_for_select(e, models, M, (const uint8_t*)d_rows, rows, L, lut, (float*)d_s))) return rc;
        if ((rc = fx_launch_topk(e, (const float*)d_s, rows, take, row0, w.idx[cur] + have, w.val[cur] + have))) return rc;
        if (have == 0) { have = take; continue; }
        const int keep = std::min(k, have + take);
        if ((rc = fx_launch_topk_merge(e, w.idx[cur], w.val[cur], have + take, keep, w.idx[cur ^ 1], w.val[cur ^ 1]))) return rc;
        cur ^= 1;
        have = keep;
    }
    FX_HIP(e, hipStreamSynchronize(e->stream));
    if ((rc = check_deferred(e))) return rc;
    if ((rc = copy_winners_out(e, w.idx[cur], w.val[cur], have, idx, val))) return rc;
    for (int j = 0; j < have; ++j)                         // the winners' rows from their numbers: the parent with at most two bytes changed
        fx_mutant_row(idx[j], L, A, B, stage, stage + pl, alphabet, rows_kxL + (size_t)j * L);
    *out_count = have;
    return FX_OK;
}

}  // extern "C"
