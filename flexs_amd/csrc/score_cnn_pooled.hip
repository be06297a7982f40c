// K1 from a per-member table of pooled features (round 6; engine option cnn_pool_table, the policy: fx_cnn_pool_decide in score_cnn_forms.h).
//
// A seq_len = 8 row over four letters has 4^8 = 65 536 values, and everything in front of the dense head -- LUT, conv1, conv2, conv3, ReLU, global
// max pool -- is a function of the row alone.  A canonical member (CNN(32, 100, k = 5), FxPackLayout::off_c1tab >= 0) may therefore carry what
// `gmax` holds when the head starts for EVERY row: 65 536 lines of 32 floats (8 MiB, fx_model::d_pooltab), built by the conv kernel's own walk
// over the enumeration of all rows (the PTB form of k_score_cnn_mfma, score_cnn_kernel.h: the same bits).  A launch whose members' tables are
// fresh then runs k_score_cnn_mfma_pooled: per tile one 8-byte row load, the LUT, one 128-byte table line per sequence, and the head's 231
// MFMAs of the 487 the conv2-prefix form issues.  The lines come from the Infinity Cache: 2 KiB per tile against the 12 KiB of the four prefix
// rows and two conv1 rows a tile of that form reads.
//
// The work split is K1's: member-major (member, tile) units cut over one workgroup per CU (fx_unit_range), the workgroup's tiles in shares per
// SIMD that the waves of a SIMD pull from (pull_tile), static wave priorities, s_setprio around the MFMA clusters, 16 waves.  Only the head's part
// of the packed image, [off_d1, total_floats), goes to LDS.  There is no quad round: a 19th tile on a SIMD costs one head here, less than a round.
#include "score_cnn_kernel.h"

namespace {

struct PooledArgs {
    const uint8_t* ascii;       // N x 8
    const uint8_t* lut;         // 256
    const float* w[FX_MAX_M];   // packed weights per member
    const float* tab[FX_MAX_M]; // pooled-feature table per member: FX_POOL_ROWS x 32 floats
    float* out;
    unsigned* err;
    int wave_prio;
    int64_t N, TG;
    int M, m_off;
    int64_t out_sn, out_sm;     // as CnnArgs
    int rlh;
    int off_d1, off_d2, off_db, head_floats;   // the head's part of the packed image: [off_d1, off_d1 + head_floats), whole f4
};

// ENUM: the builder of a member's score table (fx_model::d_scoretab).  The "batch" is the enumeration of all 4^8 rows, as in the conv kernel's
// PoolTableBuild form: the codes of lane sq of tile tg are the bits of 16 tg + sq -- no row, no LUT -- and everything behind them is the scoring
// walk itself, on the same table line: the table holds the bits a scoring launch writes for the row.
template <int WAVES, bool ENUM>
__global__ void __launch_bounds__(WAVES * 64) k_score_cnn_mfma_pooled(PooledArgs p) {
    constexpr int FT = 2, HT = 7, L = 8;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int g = lane >> 4, sq = lane & 15;
    uint8_t* lut_s = reinterpret_cast<uint8_t*>(smem + p.head_floats);
    int* next_tile = reinterpret_cast<int*>(smem + p.head_floats + 64);   // 4 work counters (one per SIMD), after the 256-byte LUT
    int* simd_waves = next_tile + 4;                                      // 4 wave counts (workgroup's waves per SIMD)

    if (p.wave_prio) fx_stagger_priority();
    const int simd = fx_simd_id();
    for (int i = tid; i < 64; i += blockDim.x)
        reinterpret_cast<uint32_t*>(lut_s)[i] = reinterpret_cast<const uint32_t*>(p.lut)[i];
    if (tid < 4) simd_waves[tid] = 0;

    int64_t u_lo, u_hi;
    fx_unit_range(p.TG, p.M, u_lo, u_hi);
    if (u_lo >= u_hi) return;
    const int m_first = (int)(u_lo / p.TG), m_last = (int)((u_hi - 1) / p.TG);
    bool bad = false;
    FxSimdShare share{0, 1, 1};

    for (int m = m_first; m <= m_last; ++m) {
        __syncthreads();                                 // previous member's readers are done
        const int64_t t_lo = (u_lo > (int64_t)m * p.TG ? u_lo : (int64_t)m * p.TG) - (int64_t)m * p.TG;
        const int64_t t_hi = (u_hi < (int64_t)(m + 1) * p.TG ? u_hi : (int64_t)(m + 1) * p.TG) - (int64_t)m * p.TG;
        if (tid < 4) next_tile[tid] = 0;
        if (m == m_first) fx_count_simd_wave(simd_waves, simd);      // (zeroed before the barrier above)
        fill_lds(reinterpret_cast<f4*>(smem), reinterpret_cast<const f4*>(p.w[m] + p.off_d1), p.head_floats / 4);
        __syncthreads();
        if (m == m_first) share = fx_simd_share(simd_waves, simd);
        const f4* w_d1 = reinterpret_cast<const f4*>(smem);
        const f4* w_d2 = reinterpret_cast<const f4*>(smem + (p.off_d2 - p.off_d1));
        const float* db = smem + (p.off_db - p.off_d1);
        const char* tab = reinterpret_cast<const char*>(p.tab[m]);
        const int64_t s_lo = t_lo + (t_hi - t_lo) * share.before / share.total;
        const int64_t s_hi = t_lo + (t_hi - t_lo) * (share.before + share.mine) / share.total;
        for (;;) {
            // the next tile of this wave's SIMD share
            int pulled = 0;
            if (lane == 0) pulled = atomicAdd(&next_tile[simd], 1);
            pulled = __builtin_amdgcn_readfirstlane(pulled);
            const int64_t tg = s_lo + pulled;
            if (tg >= s_hi) break;
            asm volatile("" ::: "memory");               // keep the weight reads inside the tile loop
            const int64_t n = tg * 16 + sq;
            unsigned codes = 0;                           // two bits per letter of the row
            if constexpr (ENUM) {
                codes = (unsigned)n;
            } else {
                unsigned long long rowq;                  // the whole row is ONE 8-byte load (any alignment); spare lanes of a ragged tile recompute row 0
                __builtin_memcpy(&rowq, p.ascii + (n < p.N ? n : 0) * L, 8);
#pragma unroll
                for (int j = 0; j < L; ++j) {
                    unsigned c = lut_s[(int)((rowq >> (8 * j)) & 0xFFull)];
                    if (c == 0xFF) { bad = true; c = 0; }
                    codes |= c << (2 * j);
                }
            }
            // the mask keeps the line inside the table whatever the LUT holds
            const char* line = tab + ((size_t)(codes & (unsigned)(FX_POOL_ROWS - 1)) << 7) + ((unsigned)g << 4);
            f4 gmax[FT][1];
#pragma unroll
            for (int t = 0; t < FT; ++t) gmax[t][0] = *reinterpret_cast<const f4*>(line + 64 * t);
            // ---- dense head: K1's calls in K1's order
            f4 h1[HT][1], h2[HT][1];
            init_bias<HT, 1>(db, h1, g);
            mma_layer<FT, HT, 1, true>(w_d1, gmax, h1, lane);
            relu_tiles<HT, 1>(h1);
            init_bias<HT, 1>(db + 16 * HT, h2, g);
            mma_layer<HT, HT, 1, true>(w_d2, h1, h2, lane, p.rlh);
            relu_tiles<HT, 1>(h2);
            float y[1];
            final_dot<HT, 1>(db + 32 * HT, db[48 * HT], h2, y, g);
            if (g == 0 && n < p.N) p.out[n * p.out_sn + (p.m_off + m) * p.out_sm] = fx_nan_to_num(y[0]);
        }
    }
    if (bad) fx_raise(p.err, FX_ERR_BADCHAR);
}

// One member's table: the PTB form over the enumeration of all rows, on e->stream (it reads the packed image only, not the other tables).
// Every CU takes part whatever grid_blocks says: that option shapes the scoring launches under test, not the build.
int build_pool_table(fx_engine* e, fx_model* m) {
    const FxShape& s = m->shape;
    const FxPackLayout& lay = m->layout;
    CnnArgs a{};
    a.lut = e->d_lut; a.err = e->d_err;
    a.wave_prio = (int)e->wave_prio;
    a.w[0] = m->d_packed;
    a.N = FX_POOL_ROWS; a.TG = FX_POOL_ROWS / 16; a.M = 1; a.Mtot = 1; a.L = s.L; a.rlh = 4;
    a.out_sn = 1; a.out_sm = 1;
    a.off_first = (int)lay.off_first; a.off_c2 = (int)lay.off_c2; a.off_c3 = (int)lay.off_c3;
    a.off_cb = (int)lay.off_cb; a.off_w1p = (int)lay.off_w1p; a.conv_floats = (int)lay.conv_floats; a.off_d1 = (int)lay.off_d1;
    a.off_d2 = (int)lay.off_d2; a.off_db = (int)lay.off_db; a.total_floats = (int)lay.total_floats;
    a.off_c1tab = -1; a.off_c2p = -1;
    a.pool_out = reinterpret_cast<f4*>(m->d_pooltab);
    const size_t lds = (size_t)lay.conv_floats * 4 + 256 + 48;
    if (lds > (size_t)e->max_lds) return FX_EUNSUPPORTED;
    const int64_t blocks = e->grid_blocks;
    e->grid_blocks = 0;
    FxOutcome out;                                       // (a launch of the build's own, outside any dispatch: the default request)
    const int rc = launch_g<CnnPoolTableBuild>(e, FxRequest{}, out, a, lds);
    e->grid_blocks = blocks;
    if (rc) return rc;
    m->pooltab_version = m->version;
    e->counters.pool_table_builds += 1;
    return FX_OK;
}

// Whether the head-only kernel serves this shape on this engine, and the LDS it asks for.
bool pooled_supported(const fx_engine* e, const FxRequest& rq, const FxPackLayout& lay, int M, size_t* lds) {
    const int64_t head_floats = lay.total_floats - lay.off_d1;
    *lds = (size_t)head_floats * 4 + 256 + 48;
    return !(M > FX_MAX_M || lay.off_c1tab < 0 || lay.off_d1 % 4 || head_floats % 4 || *lds > (size_t)e->max_lds || rq.rows_on);
}

// Every member's pooled-feature table fresh: the stale ones are built when `build`.  FX_EUNSUPPORTED: one is stale and stays so.
int fresh_pool_tables(fx_engine* e, fx_model* const* models, int M, bool build) {
    for (int m = 0; m < M; ++m) {
        fx_model* mo = models[m];
        if (mo->d_pooltab && mo->pooltab_version == mo->version) continue;
        if (!build) return FX_EUNSUPPORTED;
        if (!mo->d_pooltab && hipMalloc(&mo->d_pooltab, sizeof(float) * 32 * (size_t)FX_POOL_ROWS) != hipSuccess) {
            (void)hipGetLastError();                     // no table: the launch takes its conv form, without an error
            mo->d_pooltab = nullptr;
            return FX_EUNSUPPORTED;
        }
        if (int rc = build_pool_table(e, mo)) return rc;
    }
    return FX_OK;
}

// The head of `lay` on the rows (ENUM: on all 4^8 of them) for the members whose weights and tables `a` names, `blocks` workgroups at the most.
template <bool ENUM>
int launch_pooled(fx_engine* e, PooledArgs a, const FxPackLayout& lay, size_t lds, int64_t blocks) {
    constexpr int WAVES = 16;
    a.lut = e->d_lut; a.err = e->d_err;
    a.wave_prio = (int)e->wave_prio;
    a.TG = (a.N + 15) / 16;
    a.rlh = (lay.HTR == lay.HT) ? lay.RLH : 4;
    a.off_d1 = (int)lay.off_d1; a.off_d2 = (int)lay.off_d2; a.off_db = (int)lay.off_db; a.head_floats = (int)(lay.total_floats - lay.off_d1);
    auto kern = k_score_cnn_mfma_pooled<WAVES, ENUM>;
    static bool attr_set[64] = {};
    if (!attr_set[e->device & 63]) {
        FX_HIP(e, hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set[e->device & 63] = true;
    }
    const int64_t U = (int64_t)a.M * a.TG;
    if (blocks > U) blocks = U;                          // never more workgroups than work units
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(WAVES * 64), lds, e->stream, a);
    FX_HIP(e, hipGetLastError());
    return FX_OK;
}

// One member's score table from its fresh pooled-feature table: the head-only kernel over the enumeration of all rows, on e->stream behind the
// pooled table's own builder.  Every CU takes part whatever grid_blocks says, as in build_pool_table.
int build_score_table(fx_engine* e, fx_model* m, size_t lds) {
    PooledArgs a{};
    a.w[0] = m->d_packed; a.tab[0] = m->d_pooltab;
    a.out = m->d_scoretab;
    a.N = FX_POOL_ROWS; a.M = 1; a.m_off = 0;
    a.out_sn = 1; a.out_sm = 1;
    if (int rc = launch_pooled<true>(e, a, m->layout, lds, e->num_cus)) return rc;
    m->scoretab_version = m->version;
    e->counters.score_table_builds += 1;
    return FX_OK;
}

}  // namespace

int fx_launch_score_cnn_pooled(fx_engine* e, fx_model* const* models, int M, const uint8_t* d_ascii, int64_t N, float* d_out_NM, int Mtot, int m_off,
                               const FxRequest& rq, FxOutcome&, bool build) {
    if (N == 0) return FX_OK;
    const FxPackLayout& lay = models[0]->layout;
    size_t lds = 0;
    if (!pooled_supported(e, rq, lay, M, &lds)) return FX_EUNSUPPORTED;
    if (int rc = fresh_pool_tables(e, models, M, build)) return rc;
    PooledArgs a{};
    a.ascii = d_ascii; a.out = d_out_NM;
    for (int m = 0; m < M; ++m) { a.w[m] = models[m]->d_packed; a.tab[m] = models[m]->d_pooltab; }
    a.N = N; a.M = M; a.m_off = m_off;
    fx_out_strides(a, rq, Mtot);
    if (int rc = launch_pooled<false>(e, a, lay, lds, e->grid_blocks > 0 ? e->grid_blocks : e->num_cus)) return rc;
    e->counters.pool_table_launches += 1;
    return FX_OK;
}

int fx_cnn_score_tables(fx_engine* e, fx_model* const* models, int M, const FxRequest& rq, bool build_pool) {
    size_t lds = 0;
    if (!pooled_supported(e, rq, models[0]->layout, M, &lds)) return FX_EUNSUPPORTED;
    if (int rc = fresh_pool_tables(e, models, M, build_pool)) return rc;
    for (int m = 0; m < M; ++m) {
        fx_model* mo = models[m];
        if (mo->d_scoretab && mo->scoretab_version == mo->version) continue;
        if (!mo->d_scoretab && hipMalloc(&mo->d_scoretab, sizeof(float) * (size_t)FX_POOL_ROWS) != hipSuccess) {
            (void)hipGetLastError();                     // no table: the launch takes the head-only form, without an error
            mo->d_scoretab = nullptr;
            return FX_EUNSUPPORTED;
        }
        if (int rc = build_score_table(e, mo, lds)) return rc;
    }
    return FX_OK;
}

// The table of a model as it lies in device memory, for the tests.  Returns the floats copied; FX_ESTATE: none has been built for the current weights
extern "C" int64_t fx_debug_pool_table(fx_model* m, float* out, int64_t cap) {
    if (!m || !out) return FX_EINVAL;
    fx_engine* e = m->eng;
    if (m->layout.off_c1tab < 0) return FX_EUNSUPPORTED;
    if (!m->d_pooltab || m->pooltab_version != m->version) return fx_fail(e, FX_ESTATE, "the model has no fresh pooled-feature table");
    if (cap < (int64_t)32 * FX_POOL_ROWS) return FX_EINVAL;
    FX_HIP(e, hipSetDevice(e->device));
    FX_HIP(e, hipStreamSynchronize(e->stream));
    FX_HIP(e, hipMemcpy(out, m->d_pooltab, sizeof(float) * 32 * (size_t)FX_POOL_ROWS, hipMemcpyDeviceToHost));
    return (int64_t)32 * FX_POOL_ROWS;
}

// ... and its score table.  Returns the floats copied; FX_ESTATE: none has been built for the current weights
extern "C" int64_t fx_debug_score_table(fx_model* m, float* out, int64_t cap) {
    if (!m || !out) return FX_EINVAL;
    fx_engine* e = m->eng;
    if (m->layout.off_c1tab < 0) return FX_EUNSUPPORTED;
    if (!m->d_scoretab || m->scoretab_version != m->version) return fx_fail(e, FX_ESTATE, "the model has no fresh score table");
    if (cap < (int64_t)FX_POOL_ROWS) return FX_EINVAL;
    FX_HIP(e, hipSetDevice(e->device));
    FX_HIP(e, hipStreamSynchronize(e->stream));
    FX_HIP(e, hipMemcpy(out, m->d_scoretab, sizeof(float) * (size_t)FX_POOL_ROWS, hipMemcpyDeviceToHost));
    return (int64_t)FX_POOL_ROWS;
}
