// Dispatch of the fused CNN scoring kernels (template in score_cnn_kernel.h): fx_cnn_pick_fused (score_cnn_forms.h) chooses the form and the
// geometry without touching the device, this file fills the arguments and launches the named instantiation.
#include "score_cnn_kernel.h"

int fx_launch_score_cnn_mfma(fx_engine* e, fx_model* const* models, int M, const uint8_t* d_ascii,
                             int64_t N, float* d_out_NM, int Mtot, int m_off, const FxRequest& rq, FxOutcome& out) {
    if (N == 0) return FX_OK;
    const FxShape& s = models[0]->shape;
    const FxPackLayout& lay = models[0]->layout;
    for (int m = 0; m < M; ++m) {
        const FxShape& t = models[m]->shape;
        if (t.kind != FX_CNN || t.L != s.L || t.A != s.A || t.F != s.F || t.H != s.H || t.K != s.K)
            return FX_EUNSUPPORTED;                      // heterogeneous: caller scores them one by one
    }
    if (int rc = fx_cnn_fused_supported(e, rq, s, lay, M)) return rc;
    if (!rq.rows_on) {
        const int rc = fx_launch_score_cnn_quad(e, models, M, d_ascii, N, d_out_NM, Mtot, m_off, rq, out);
        if (rc != FX_EUNSUPPORTED) return rc;
    }

    CnnArgs a{};
    a.ascii = d_ascii; a.lut = e->d_lut; a.out = d_out_NM; a.err = e->d_err;
    if (int rc = fx_trace_buffer(e, &a.trace)) return rc;
    a.wave_prio = (int)e->wave_prio;
    a.stage_fill = (int)e->stage_fill;
    for (int m = 0; m < M; ++m) a.w[m] = models[m]->d_packed;
    fx_out_strides(a, rq, Mtot);
    a.N = N; a.M = M; a.Mtot = Mtot; a.m_off = m_off; a.L = s.L; a.rlh = (lay.HTR == lay.HT) ? lay.RLH : 4;
    a.off_first = (int)lay.off_first; a.off_c2 = (int)lay.off_c2; a.off_c3 = (int)lay.off_c3;
    a.off_cb = (int)lay.off_cb; a.off_w1p = (int)lay.off_w1p; a.conv_floats = (int)lay.conv_floats; a.off_d1 = (int)lay.off_d1;
    a.off_d2 = (int)lay.off_d2; a.off_db = (int)lay.off_db; a.total_floats = (int)lay.total_floats;
    a.off_c1tab = (int)lay.off_c1tab;
    a.off_c2p = e->cnn_conv2_prefix >= 1 && e->cnn_conv2_prefix <= FX_C2P_MAX_DEPTH ? (int)lay.off_c2p[e->cnn_conv2_prefix - 1] : -1;

#if defined(FX_AB)
    // mean-only call with the rows resident in device memory and every member in this launch: the last member to finish a tile averages
    // it (fx_fused_mean_tile) -- no mean kernel behind the launch.  (Rows that arrive while the kernel runs keep the mean kernel: a
    // starved launch is redone, and its tickets would be left half drawn.)
    if (e->fuse_mean_batch && rq.mean_out && rq.stride && m_off == 0 && M == Mtot && M > 1 && M < 8 && !rq.rows_on) {
        void* ws = nullptr;
        if (int rc = fx_zero_pool(e, (size_t)((N + 15) / 16) * sizeof(unsigned), &ws)) return rc;
        a.fm_mean = rq.mean_out;
        a.fm_cnt = (unsigned*)ws;
    }
#endif
    const CnnPick pk = fx_cnn_pick_fused(e, rq, s, lay, N, M);
    if (pk.pair_first && e->cnn_pair) {
        const int rc = fx_launch_score_cnn_pair(e, models, M, d_ascii, N, d_out_NM, Mtot, m_off, rq, out);
        if (rc != FX_EUNSUPPORTED) return rc;
    }
    if (pk.rc) return pk.msg ? fx_fail(e, pk.rc, pk.msg) : pk.rc;
    {
        // canonical seq_len = 8 members whose pooled-feature tables are fresh (or are built now): only the head runs (score_cnn_pooled.hip).  The
        // in-kernel timeline and the fused mean of the A/B build belong to the conv forms
        bool fresh = true;
        for (int m = 0; m < M; ++m) fresh = fresh && models[m]->d_pooltab && models[m]->pooltab_version == models[m]->version;
        CnnPoolDecision pool = fx_cnn_pool_decide(e, rq, lay, pk, N, fresh);
        if (a.trace) pool = CNN_POOL_NO;
#if defined(FX_AB)
        if (a.fm_mean) pool = CNN_POOL_NO;
#endif
        if (fx_cnn_score_decide(e, pool) == CNN_SCORE_LOOKUP) {
            // ... or nothing runs but a table read per row and member (score_cnn_lookup.hip)
            const int rc = fx_launch_score_cnn_lookup(e, models, M, d_ascii, N, d_out_NM, Mtot, m_off, rq, out, pool == CNN_POOL_BUILD);
            if (rc != FX_EUNSUPPORTED) return rc;       // (no score table could be had: the head-only form)
        }
        if (pool != CNN_POOL_NO) {
            const int rc = fx_launch_score_cnn_pooled(e, models, M, d_ascii, N, d_out_NM, Mtot, m_off, rq, out, pool == CNN_POOL_BUILD);
            if (rc != FX_EUNSUPPORTED) return rc;       // (no table could be had: the form picked above)
        }
    }
    a.TG = pk.TG;
    a.quad_tail = pk.qt ? 1 : 0;
    a.seg_sb = pk.seg_sb;
    if (pk.seg_sb > 1) {
        // a tile's workgroups meet in the zero pool (CnnArgs::seg_pool)
        const int64_t U = (int64_t)a.M * a.TG;
        void* ws = nullptr;
        const size_t pool_bytes = (size_t)U * 2 * 64 * 4 * sizeof(unsigned), cnt_bytes = (size_t)U * sizeof(unsigned);
        if (int rc = fx_zero_pool(e, pool_bytes + cnt_bytes, &ws)) return rc;
        a.seg_pool = (unsigned*)ws;
        a.seg_cnt = (unsigned*)((char*)ws + pool_bytes);
    }
    return fx_cnn_with_fused_form(pk, [&](auto form) { return launch_g<decltype(form)>(e, rq, out, a, pk.lds); });
}

#include "score_cnn_tables.h"   // fx_build_conv1_table, fx_build_conv2_prefix (why here: its first lines)
