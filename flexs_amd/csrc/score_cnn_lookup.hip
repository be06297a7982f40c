// K1 from a per-member table of scores (engine option cnn_score_table, the policy: fx_cnn_score_decide in score_cnn_forms.h).
//
// A seq_len = 8 row over four letters has 4^8 = 65 536 values and a member's score is a function of the row and the member's weights alone: a
// canonical member may carry its score for EVERY row, 65 536 floats (256 KiB, fx_model::d_scoretab), built by the head-only kernel's own walk over
// the enumeration of all rows from the pooled-feature table (the ENUM form of k_score_cnn_mfma_pooled, score_cnn_pooled.hip: the same bits).  A
// launch group whose members' tables are fresh is then this kernel: per row one 8-byte load, the LUT, and per member one 4-byte table read and
// one store.  The tables of a three-member ensemble are 768 KiB and stay in every XCD's L2.
//
// One row per thread, grid-stride; no workgroup waits for another, no atomics.  The thread that holds a row's scores of ALL the ensemble's members
// also writes their mean (np_mean_row16, the routine of k_ensemble_mean_planar and the quad form: the same bits), so the mean launch behind a
// mean-only call disappears.
#include "fx_common.h"
#include "np_sum.h"
#include "score_cnn_forms.h"

namespace {

constexpr int LOOKUP_THREADS = 256;

struct LookupArgs {
    const uint8_t* ascii;       // N x 8
    const uint8_t* lut;         // 256
    const float* tab[FX_MAX_M]; // score table per member: FX_POOL_ROWS floats
    float* out;
    float* mean;                // N floats, or nullptr: the members of this launch are not the whole ensemble, or nobody asked
    unsigned* err;
    int64_t N;
    int m_off;
    int64_t out_sn, out_sm;     // as CnnArgs
};

template <int M>
__global__ void __launch_bounds__(LOOKUP_THREADS) k_score_cnn_mfma_scoretab(LookupArgs p) {
    constexpr int L = 8;
    __shared__ __attribute__((aligned(16))) uint8_t lut_s[256];
    if (threadIdx.x < 64) reinterpret_cast<uint32_t*>(lut_s)[threadIdx.x] = reinterpret_cast<const uint32_t*>(p.lut)[threadIdx.x];
    __syncthreads();
    bool bad = false;
    for (int64_t n = (int64_t)blockIdx.x * LOOKUP_THREADS + threadIdx.x; n < p.N; n += (int64_t)gridDim.x * LOOKUP_THREADS) {
        unsigned long long rowq;                          // the whole row is ONE 8-byte load (any alignment)
        __builtin_memcpy(&rowq, p.ascii + n * L, 8);
        unsigned codes = 0;                               // two bits per letter of the row: the pooled kernel's index
#pragma unroll
        for (int j = 0; j < L; ++j) {
            unsigned c = lut_s[(int)((rowq >> (8 * j)) & 0xFFull)];
            if (c == 0xFF) { bad = true; c = 0; }
            codes |= c << (2 * j);
        }
        const unsigned at = codes & (unsigned)(FX_POOL_ROWS - 1);   // the mask keeps the read inside the table whatever the LUT holds
        float x[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) x[m] = m < M ? p.tab[m][at] : 0.f;
#pragma unroll
        for (int m = 0; m < M; ++m) p.out[n * p.out_sn + (p.m_off + m) * p.out_sm] = x[m];
        if (p.mean) p.mean[n] = np_mean_row16(x, M);
    }
    if (bad) fx_raise(p.err, FX_ERR_BADCHAR);
}

}  // namespace

int fx_launch_score_cnn_lookup(fx_engine* e, fx_model* const* models, int M, const uint8_t* d_ascii, int64_t N, float* d_out_NM, int Mtot, int m_off,
                               const FxRequest& rq, FxOutcome& out, bool build) {
    if (N == 0) return FX_OK;
    if (M < 1 || M > FX_MAX_M || models[0]->shape.L != 8) return FX_EUNSUPPORTED;
    if (int rc = fx_cnn_score_tables(e, models, M, rq, build)) return rc;
    LookupArgs a{};
    a.ascii = d_ascii; a.lut = e->d_lut; a.out = d_out_NM; a.err = e->d_err;
    for (int m = 0; m < M; ++m) a.tab[m] = models[m]->d_scoretab;
    a.N = N; a.m_off = m_off;
    fx_out_strides(a, rq, Mtot);
    // the whole ensemble in this launch and a mean asked for (score_then_mean): the thread that has a row's scores averages them
    const bool fuse = rq.mean_out && rq.stride && m_off == 0 && M == Mtot && M > 1;
    a.mean = fuse ? rq.mean_out : nullptr;
    // up to four workgroups per CU (the multi-GPU bench keeps CUs free through grid_blocks); never more than there are rows for
    int64_t blocks = e->grid_blocks > 0 ? e->grid_blocks : (int64_t)e->num_cus * 4;
    const int64_t need = (N + LOOKUP_THREADS - 1) / LOOKUP_THREADS;
    if (blocks > need) blocks = need;
    const dim3 grid((unsigned)blocks), block(LOOKUP_THREADS);
    switch (M) {
#define FX_LOOKUP_CASE(m) case m: hipLaunchKernelGGL(k_score_cnn_mfma_scoretab<m>, grid, block, 0, e->stream, a); break;
        FX_LOOKUP_CASE(1) FX_LOOKUP_CASE(2) FX_LOOKUP_CASE(3) FX_LOOKUP_CASE(4) FX_LOOKUP_CASE(5) FX_LOOKUP_CASE(6) FX_LOOKUP_CASE(7) FX_LOOKUP_CASE(8)
        FX_LOOKUP_CASE(9) FX_LOOKUP_CASE(10) FX_LOOKUP_CASE(11) FX_LOOKUP_CASE(12) FX_LOOKUP_CASE(13) FX_LOOKUP_CASE(14) FX_LOOKUP_CASE(15)
        FX_LOOKUP_CASE(16)
#undef FX_LOOKUP_CASE
        default: return FX_EUNSUPPORTED;
    }
    FX_HIP(e, hipGetLastError());
    if (fuse) out.mean_done = true;
    e->counters.pool_table_launches += 1;
    e->counters.score_table_launches += 1;
    return FX_OK;
}
