// The forms of the fused CNN scoring kernel (k_score_cnn_mfma, score_cnn_kernel.h) and the choice among them.  Host code only, no HIP call:
// a form is a type with named fields, a launch is routed by a pure function (fx_cnn_pick_fused / fx_cnn_pick_conv) and a switch from its
// answer to the named type (fx_cnn_with_fused_form / fx_cnn_with_conv_form).  fx_debug_cnn_form_pick shows both to the CPU tests.
#pragma once
#include <type_traits>

#include "fx_common.h"

namespace {

// ---------------------------------------------------------------- forms
// The base form: CNN(17..32 filters, 97..112 hidden units, kernel size 5) on four letters, any sequence length, one tile per wave, 8 waves,
// whole member in LDS.  What each field means to the kernel: the comment at the head of score_cnn_kernel.h.
struct CnnForm {
    static constexpr int A = 4, K = 5, FT = 2, HT = 7, NT = 1;
    static constexpr bool DENSE_LDS = true;
    static constexpr int WAVES = 8;
    static constexpr bool G1 = true;
    static constexpr int L1S = 0;
    static constexpr bool PRIO = false, SEG = false, HEAD = true, STG = false, QT = false, C1T = false;
    static constexpr int C2P = 0;
    static constexpr bool PTB = false;
};
// A form shadows what it changes.  (A kernel is instantiated per TYPE: the switches below are the only place that spells these, so that one
// set of field values has one spelling.)
template <class F> struct Waves16 : F { static constexpr int WAVES = 16; };
template <class F> struct Waves4 : F { static constexpr int WAVES = 4; };
template <class F, int POSITIONS> struct Unrolled : F { static constexpr int L1S = POSITIONS; static constexpr bool PRIO = true; };
template <class F> struct NoPrio : F { static constexpr bool PRIO = false; };
template <class F> struct Segmented : F { static constexpr bool SEG = true; };
template <class F> struct HostStaged : F { static constexpr bool STG = true; };
template <class F> struct QuadTail : F { static constexpr bool QT = true; };
template <class F> struct Conv1Table : F { static constexpr bool C1T = true; };
template <class F, int DEPTH> struct Conv2Prefix : Conv1Table<F> { static constexpr int C2P = DEPTH; };   // (no C2P without C1T)
template <class F> struct PoolTableBuild : F { static constexpr bool PTB = true; };   // (a conv-only form: the rows are the tile indices, the features go to the member's table)
template <class F> struct Conv1Mfma : F { static constexpr bool G1 = false; };
template <class F> struct TwoTiles : F { static constexpr int NT = 2; };
template <class F> struct HeadFromL2 : F { static constexpr bool DENSE_LDS = false; };
template <class F> struct ConvOnly : F { static constexpr int HT = 1; static constexpr bool DENSE_LDS = false, HEAD = false; };
template <class F, int V> struct AlphabetOf : F { static constexpr int A = V; };
template <class F, int V> struct KernelOf : F { static constexpr int K = V; };
template <class F, int V> struct FilterTilesOf : F { static constexpr int FT = V; };
template <class F, int V> struct HiddenTilesOf : F { static constexpr int HT = V; };
template <class F, int V> using Alphabet = std::conditional_t<V == F::A, F, AlphabetOf<F, V>>;
template <class F, int V> using Kernel = std::conditional_t<V == F::K, F, KernelOf<F, V>>;
template <class F, int V> using FilterTiles = std::conditional_t<V == F::FT, F, FilterTilesOf<F, V>>;
template <class F, int V> using HiddenTiles = std::conditional_t<V == F::HT, F, HiddenTilesOf<F, V>>;

// The shipped forms by name.
using CnnGeneric8 = CnnForm;                                 // any length: ring windows, byte look-ahead, staged fill of small launches
using CnnGeneric16 = Waves16<CnnForm>;                       // ... four waves per SIMD: long launches
using CnnUnrolled8W16 = Unrolled<Waves16<CnnForm>, 4>;       // seq_len 8 (four conv positions) unrolled, s_setprio: the headline form
using CnnUnrolled8W8 = Unrolled<CnnForm, 4>;                 // ... its 8-wave sibling (256-register budget): small and mid-size launches
using CnnUnrolled14W16 = Unrolled<Waves16<CnnForm>, 10>;     // seq_len 14 (ten conv positions) unrolled
using CnnSeg8 = Segmented<CnnForm>;                          // the waves of a workgroup split one tile's positions
using CnnSeg4 = Segmented<Waves4<CnnForm>>;                  // ... in 4-wave workgroups, several per tile
template <int HT_> using CnnHidden8 = HiddenTiles<CnnForm, HT_>;                     // other hidden widths (HT_ tiles of 16 units)
template <int K_, int FT_> using CnnConv = ConvOnly<FilterTiles<Kernel<CnnForm, K_>, FT_>>;   // the split path's conv-only forms (score_cnn_split.hip)
using CnnPoolTableBuild = PoolTableBuild<Unrolled<Waves16<CnnConv<5, 2>>, 4>>;   // the builder of the pooled-feature table (score_cnn_pooled.hip): the unrolled conv-only walk over all 4^8 rows
using CnnBinary8 = Alphabet<CnnForm, 2>;                     // binary alphabet
using CnnNarrow8 = FilterTiles<CnnForm, 1>;                  // at most 16 filters
using CnnNarrowProtein8 = Alphabet<CnnNarrow8, 20>;
using CnnK3W8 = Kernel<CnnForm, 3>;
using CnnK7W8 = Kernel<CnnForm, 7>;
using CnnProteinW4 = Alphabet<HeadFromL2<Waves4<CnnForm>>, 20>;   // (A/B build) one wave per SIMD: 512 registers for the 19-tap window

// One name per way through the switches below (families take their parameter from CnnPick).
enum CnnFormId : int {
    CNN_NO_FORM = 0,            // nothing of this template is launched (an error, or the conv part of a protein CNN: score_cnn_pair.hip)
    CNN_GENERIC_W8,             // CnnHidden8<HT>, head from LDS or L2 (dense_lds); HT 7: host-staged (stg); MFMA conv1 (conv1_mfma, A/B build)
    CNN_GENERIC_W16,            // ... HT <= 7
    CNN_SEG_W8,                 // Segmented<CnnHidden8<HT>>, head from LDS or L2
    CNN_SEG_W4,
    CNN_UNROLLED8_W16,          // + quad tail (qt), conv1 table (c1t), conv2 prefix (c2p), or host-staged (stg)
    CNN_UNROLLED8_W8,           // or host-staged
    CNN_UNROLLED14_W16,         // or host-staged
    CNN_TWO_TILES_W4,           // A/B build
    CNN_TWO_TILES_W8,           // A/B build
    CNN_UNROLLED8_W16_NOPRIO,   // A/B build
    CNN_UNROLLED14_W16_NOPRIO,  // A/B build
    CNN_PROTEIN_W4,             // A/B build
    CNN_BINARY_W8, CNN_BINARY_W16, CNN_BINARY_SEG,
    CNN_NARROW_W8, CNN_NARROW_W16, CNN_NARROW_SEG, CNN_NARROW_PROTEIN_W8,
    CNN_K3_W8, CNN_K3_W16, CNN_K3_SEG, CNN_K7_W8,
    CNN_CONV_W8,                // CnnConv<K, FT>
    CNN_CONV_SEG,               // Segmented<CnnConv<K, FT>>, K <= 5
    CNN_CONV_W16, CNN_CONV_UNROLLED8_W16,   // CnnConv<5, 2>
    CNN_CONV_BINARY,
};

// What the pure part of a launcher answers: the form and the launch geometry, or a status.
struct CnnPick {
    int rc = FX_OK;
    const char* msg = nullptr;  // with FX_EINVAL: the text for fx_fail
    bool pair_first = false;    // protein alphabet: score_cnn_pair.hip is tried before this form (and is the only one in the production build)
    CnnFormId id = CNN_NO_FORM;
    int HT = 7, K = 5, FT = 2;  // the families' parameters
    bool dense_lds = true, stg = false, qt = false, c1t = false, conv1_mfma = false;
    int c2p = 0;
    int64_t TG = 0;             // CnnArgs::TG
    int seg_sb = 0;             // CnnArgs::seg_sb (> 1: the launcher takes the zero pool)
    size_t lds = 0;             // bytes of LDS before what launch_g adds for the form's own scratch
};

// ---------------------------------------------------------------- the two rules every branch shares
// at least `per_cu` work units (member x tile) per CU: with cnn_big_units, the size from which 16-wave workgroups pay
inline bool fx_cnn_units_per_cu(const fx_engine* e, int64_t U, int64_t per_cu) { return U >= (int64_t)e->num_cus * per_cu; }
// small enough (at most one unit per CU) ...
inline bool fx_cnn_small(const fx_engine* e, int64_t U) { return e->cnn_seg != 0 && U <= e->num_cus; }
// ... and long enough (from `min_l1` conv positions on, or forced) to cut a tile's positions over the waves of a workgroup, with room in LDS
// for the 8 waves' segment maxima beside the `lds` bytes of weights
inline bool fx_cnn_segmented(const fx_engine* e, int64_t U, int L1, int min_l1, size_t lds, int FT) {
    return fx_cnn_small(e, U) && (e->cnn_seg > 0 || L1 >= min_l1) && lds + (size_t)8 * FT * 64 * 16 <= (size_t)e->max_lds;
}

// ---------------------------------------------------------------- fused kernel (score_cnn_mfma.hip)
// The shapes the fused kernel covers at all; checked before score_cnn_quad.hip is tried.
inline int fx_cnn_fused_supported(const fx_engine* e, const FxRequest& rq, const FxShape& s, const FxPackLayout& lay, int M) {
    // num_filters 17..32 (two channel tiles; missing channels are zero padding of the packed blocks); kernel_size 5
    // everywhere, 3 and 7 for the canonical hidden width (97..112 units); everything else -> shape-agnostic kernels
    if ((lay.FT != 2 && !(lay.FT == 1 && s.K == 5 && lay.HT == 7)) || (s.A != 4 && s.A != 20 && s.A != 2)) return FX_EUNSUPPORTED;
    if (s.K != 5 && !((s.K == 3 || s.K == 7) && lay.HT == 7)) return FX_EUNSUPPORTED;
    if (M > FX_MAX_M) return FX_EINVAL;
    // a launched-first host call (rows arrive while the kernel runs): the whole-tile-per-wave forms of the 4-letter CNN only
    if (rq.rows_on && !(s.A == 4 && s.K == 5 && lay.FT == 2)) return FX_EUNSUPPORTED;
    return FX_OK;
}

inline CnnPick fx_cnn_pick_fused(const fx_engine* e, const FxRequest& rq, const FxShape& s, const FxPackLayout& lay, int64_t N, int M) {
    CnnPick pk;
    auto fail = [&](int rc, const char* msg = nullptr) { pk.rc = rc; pk.msg = msg; pk.id = CNN_NO_FORM; return pk; };
    auto form = [&](CnnFormId id, size_t lds) { pk.id = id; pk.lds = lds; return pk; };
    if (int rc = fx_cnn_fused_supported(e, rq, s, lay, M)) return fail(rc);
    const size_t max_lds = (size_t)e->max_lds;
    const size_t full = (size_t)lay.total_floats * 4 + 256 + 48, conv_only = (size_t)lay.conv_floats * 4 + 256 + 48;
    pk.TG = (N + 15) / 16;
    pk.K = s.K; pk.FT = lay.FT; pk.HT = lay.HT;
    pk.conv1_mfma = e->cnn_conv1_mfma != 0;
    const int64_t U = pk.TG * M;
    const int L1 = s.L - s.K + 1;
    const bool big = fx_cnn_units_per_cu(e, U, e->cnn_big_units);
    if (s.A == 2) {
        // binary alphabet (`BA = "01"`, sequence_utils.py:16): conv3 has ONE tap (kernel_size = len(alphabet) - 1);
        // canonical filter / hidden / kernel sizes only, first conv in gather form
        if (lay.FT != 2 || lay.HT != 7 || s.K != 5 || full > max_lds || e->cnn_conv1_mfma) return fail(FX_EUNSUPPORTED);
        if (fx_cnn_segmented(e, U, L1, 24, full, 2)) return form(CNN_BINARY_SEG, full);
        return form(big ? CNN_BINARY_W16 : CNN_BINARY_W8, full);
    }
    if (lay.FT == 1) {
        // num_filters <= 16: one channel tile (canonical hidden width and kernel size only)
        if (full > max_lds || e->cnn_conv1_mfma) return fail(FX_EUNSUPPORTED);
        if (s.A == 20) return form(CNN_NARROW_PROTEIN_W8, full);   // 19-tap window of one tile: 8 waves fit (no 16-wave, no segmented form)
        if (fx_cnn_segmented(e, U, L1, 24, full, 1)) return form(CNN_NARROW_SEG, full);
        return form(big ? CNN_NARROW_W16 : CNN_NARROW_W8, full);
    }
    if (s.A == 4 && s.K != 5) {
        // other kernel sizes: the generic-length kernels only (no unrolled specialisations, conv1 in gather form)
        if (full > max_lds || e->cnn_conv1_mfma) return fail(FX_EUNSUPPORTED);
        if (s.K == 7) return form(CNN_K7_W8, full);      // 7-tap window: shifting form, 256-register budget (no 16-wave, no segmented form)
        if (fx_cnn_segmented(e, U, L1, 24, full, 2)) return form(CNN_K3_SEG, full);
        return form(big ? CNN_K3_W16 : CNN_K3_W8, full);
    }
    if (s.A == 20) {
        // proteins: the two-waves-per-tile kernel (score_cnn_pair.hip); the single-wave window form (HT = 7 only) is the A/B baseline
        pk.pair_first = true;
#if defined(FX_AB)
        if (lay.HT != 7 || s.K != 5 || conv_only > max_lds) return fail(FX_EUNSUPPORTED);
        pk.dense_lds = false;
        return form(CNN_PROTEIN_W4, conv_only);          // 1 wave / SIMD: 512-VGPR budget for the 19-tap window (0.76 vs 0.92 of peak for the pair form)
#else
        return fail(FX_EUNSUPPORTED);                    // (the one-wave window form of the protein CNN lives in the A/B build)
#endif
    }

    // A = 4 (DNA / RNA), kernel size 5, two channel tiles: NT1 tiles; 16 waves (4 per SIMD) once every CU has plenty of tiles, else 8.
    // Hidden sizes other than the canonical 7 tiles get the auto geometry only; HT >= 8 needs the 256-register budget of 8-wave
    // workgroups for the dense head.
    const int HT = lay.HT;
    // more than 128 hidden units at batch size: the two-kernel path, whose head streams the H x H layer through LDS slabs (score_cnn_split.hip)
    if (HT >= 13 && e->cnn_head_slab && !rq.rows_on && fx_cnn_units_per_cu(e, U, 16)) return fail(FX_EUNSUPPORTED);
    if (HT != 1 && HT != 2 && HT != 4 && HT != 7 && HT != 8 && HT != 13 && HT != 16) return fail(FX_EUNSUPPORTED);
    int variant = (int)e->cnn_variant;
    const bool dl = full <= max_lds;                     // whole member in LDS, else dense head streams from L2
    const size_t lds = dl ? full : conv_only;
    if (lds > max_lds) return fail(FX_EUNSUPPORTED);
    pk.dense_lds = dl;
    if (HT == 7) {
        // the sequences lie in host memory (zero-copy host calls): the forms that copy a tile's bytes into LDS first (STG) -- same
        // walk, same bits -- where the scratch fits beside the weights (explorer-size launches keep their own forms below)
        if (rq.host_rows && e->cnn_stage_host && dl && (variant == 0 || variant == 7 || variant == 10 || variant == 11) &&
            lds + 16 * ((16 * (size_t)s.L + 15) / 16 * 16) <= max_lds && !fx_cnn_small(e, U)) {
            pk.stg = true;
            if (big) return form(s.L == 8 ? CNN_UNROLLED8_W16 : s.L == 14 ? CNN_UNROLLED14_W16 : CNN_GENERIC_W16, lds);
            return form(s.L == 8 ? CNN_UNROLLED8_W8 : CNN_GENERIC_W8, lds);
        }
        // canonical short landscapes get a fully unrolled position loop with s_setprio around the MFMA clusters
        // (+5 % and +2-4 % resp., interleaved A/B: profiles/archive/r1_run9, r1_run16, r1_run18):
        // TF-binding (L = 8) and the RNA landscapes (L = 14)
        if (dl && variant == 0 && big && s.L == 8) variant = 7;
        // ... and in 8-wave workgroups for small and mid-size launches (one or two waves per SIMD: the unrolled walk is
        // 5 % shorter per tile than the ring loop, profiles/archive/r2_trace_probe)
        if (dl && variant == 0 && !big && s.L == 8) variant = 11;
        if (dl && variant == 0 && big && s.L == 14) variant = 10;
        if (dl && variant != 0) {
            switch (variant) {
                case 1: return form(CNN_GENERIC_W8, lds);
#if defined(FX_AB)   // (two tiles per wave, and the unrolled forms without s_setprio: measured losers, A/B build only)
                case 2: pk.TG = (N + 31) / 32; return form(CNN_TWO_TILES_W4, lds);
                case 3: pk.TG = (N + 31) / 32; return form(CNN_TWO_TILES_W8, lds);
                case 5:                                  // variant 4 with the position loop unrolled (TF-binding: L = 8), no s_setprio (A/B baseline)
                    if (s.L != 8) return fail(FX_EINVAL, "cnn_variant 5 is the seq_len = 8 specialisation");
                    return form(CNN_UNROLLED8_W16_NOPRIO, lds);
                case 6:
                    if (s.L != 14) return fail(FX_EINVAL, "cnn_variant 6 is the seq_len = 14 specialisation");
                    return form(CNN_UNROLLED14_W16_NOPRIO, lds);
#endif
                case 4: return form(CNN_GENERIC_W16, lds);
                case 10:                                 // variant 6 with s_setprio (A/B)
                    if (s.L != 14) return fail(FX_EINVAL, "cnn_variant 10 is a seq_len = 14 specialisation");
                    return form(CNN_UNROLLED14_W16, lds);
                case 7:                                  // unrolled L = 8 specialisation with s_setprio (the default)
                    if (s.L != 8) return fail(FX_EINVAL, "cnn_variant 7 is a seq_len = 8 specialisation");
                    // ... with conv1 read from the member's table of windows instead of gathered (cnn_conv1_table = 0: A/B); not when the
                    // rows arrive while the kernel runs (the table's second round trip would stand behind the wait for the rows)
                    pk.c1t = e->cnn_conv1_table && !rq.rows_on && lay.off_c1tab >= 0;
                    // ... and conv2's first one or two taps per position read from the member's prefix tables (cnn_conv2_prefix; a form of
                    // the table form: every other launch silently runs all taps)
                    if (pk.c1t && e->cnn_conv2_prefix >= 1 && e->cnn_conv2_prefix <= FX_C2P_MAX_DEPTH && lay.off_c2p[e->cnn_conv2_prefix - 1] >= 0)
                        pk.c2p = (int)e->cnn_conv2_prefix;
                    // ... and the (tiles mod 4) last tiles of a workgroup walked by wave quads (round 6; cnn_quad_tail = 0: A/B)
                    pk.qt = e->cnn_quad_tail && !rq.rows_on && lds + (size_t)3 * 2 * 8 * 1024 <= max_lds;
                    return form(CNN_UNROLLED8_W16, lds);
                case 11:                                 // unrolled L = 8 form in 8-wave workgroups (256-register budget): small launches
                    if (s.L != 8) return fail(FX_EINVAL, "cnn_variant 11 is a seq_len = 8 specialisation");
                    return form(CNN_UNROLLED8_W8, lds);
                default: return fail(FX_EINVAL, "cnn_variant must be 0..11");
            }
        }
    }
    // small batch of long sequences (an explorer's 1-100 sequence call on an RNA landscape): the 8 waves of a
    // workgroup split one tile's positions instead of 7 of them idling
    // (one 8-wave workgroup per tile pays from 24 positions; spread over several 4-wave workgroups, from 13 -- shorter
    //  sequences take the quad form)
    const bool may_spread = HT == 7 && dl && e->cnn_seg < 0 && e->cnn_seg_multi;
    const bool multi = may_spread && 2 * U <= e->num_cus;
    if (!rq.rows_on && variant == 0 && !e->cnn_conv1_mfma && fx_cnn_segmented(e, U, L1, multi ? 13 : 24, lds, 2)) {
        // Long sequences: cut the positions over several workgroups as well (halo: 3 positions per side).  As many
        // segments (>= 2 positions) as one wave of the grid holds, from 4-wave workgroups -- one wave per SIMD -- when
        // that gives as many as 8-wave ones would (score_cnn_pair.hip has the measurements behind both rules).
        pk.seg_sb = 1;
        if (may_spread) {
            auto count = [&](int w) {
                int64_t sb = L1 / (w * 2);
                if (sb > 64 / w) sb = 64 / w;
                if (sb > e->num_cus / U) sb = e->num_cus / U;
                return sb < 1 ? (int64_t)1 : sb;
            };
            const int64_t sb8 = count(8), sb4 = count(4);
            pk.seg_sb = (int)(sb4 * 4 >= sb8 * 8 ? sb4 : sb8);
            if (sb4 * 4 >= sb8 * 8) return form(CNN_SEG_W4, lds);
        }
        return form(CNN_SEG_W8, lds);
    }
    return form(HT <= 7 && big ? CNN_GENERIC_W16 : CNN_GENERIC_W8, lds);
}

// fn(std::integral_constant<int, V>{}) for the V among Vs that equals v; FX_EUNSUPPORTED if there is none
template <int... Vs, class Fn>
int fx_cnn_lift(int v, Fn&& fn) {
    int rc = FX_EUNSUPPORTED;
    (void)((v == Vs ? (rc = fn(std::integral_constant<int, Vs>{}), true) : false) || ...);
    return rc;
}
// G1: the MFMA form of the one-hot conv1 -- 3-15 % slower than the LDS gather -- lives in the A/B build (`make ab`)
template <class F, class Fn>
int fx_cnn_with_conv1(const CnnPick& pk, Fn& fn) {
#if defined(FX_AB)
    if (pk.conv1_mfma) return fn(Conv1Mfma<F>{});
#endif
    return fn(F{});
}
template <class F, class Fn>
int fx_cnn_with_head(const CnnPick& pk, Fn& fn) { return pk.dense_lds ? fn(F{}) : fn(HeadFromL2<F>{}); }
// QT x C1T x C2P of the headline form: the eight combinations the three run-time decisions can make (C2P only on C1T)
template <class F, class Fn>
int fx_cnn_with_tables(const CnnPick& pk, Fn& fn) {
    if (!pk.c1t) return fn(F{});
    if (pk.c2p == 1) return fn(Conv2Prefix<F, 1>{});
    if (pk.c2p == 2) return fn(Conv2Prefix<F, 2>{});
    return fn(Conv1Table<F>{});
}
template <class F, class Fn>
int fx_cnn_with_tail_and_tables(const CnnPick& pk, Fn& fn) { return pk.qt ? fx_cnn_with_tables<QuadTail<F>>(pk, fn) : fx_cnn_with_tables<F>(pk, fn); }

// From the pick of fx_cnn_pick_fused to the named form: fn(Form{}) is called for exactly the forms score_cnn_mfma.hip launches.
template <class Fn>
int fx_cnn_with_fused_form(const CnnPick& pk, Fn&& fn) {
    switch (pk.id) {
        case CNN_GENERIC_W8:
            if (pk.stg) return fn(HostStaged<CnnGeneric8>{});
            return fx_cnn_lift<1, 2, 4, 7, 8, 13, 16>(pk.HT, [&](auto ht) {
                using F = CnnHidden8<decltype(ht)::value>;
                return pk.dense_lds ? fx_cnn_with_conv1<F>(pk, fn) : fx_cnn_with_conv1<HeadFromL2<F>>(pk, fn);
            });
        case CNN_GENERIC_W16:
            if (pk.stg) return fn(HostStaged<CnnGeneric16>{});
            return fx_cnn_lift<1, 2, 4, 7>(pk.HT, [&](auto ht) {
                using F = Waves16<CnnHidden8<decltype(ht)::value>>;
                return pk.dense_lds ? fx_cnn_with_conv1<F>(pk, fn) : fx_cnn_with_conv1<HeadFromL2<F>>(pk, fn);
            });
        case CNN_SEG_W8:
            return fx_cnn_lift<1, 2, 4, 7, 8, 13, 16>(pk.HT, [&](auto ht) { return fx_cnn_with_head<Segmented<CnnHidden8<decltype(ht)::value>>>(pk, fn); });
        case CNN_SEG_W4: return fn(CnnSeg4{});
        case CNN_UNROLLED8_W16: return pk.stg ? fn(HostStaged<CnnUnrolled8W16>{}) : fx_cnn_with_tail_and_tables<CnnUnrolled8W16>(pk, fn);
        case CNN_UNROLLED8_W8: return pk.stg ? fn(HostStaged<CnnUnrolled8W8>{}) : fn(CnnUnrolled8W8{});
        case CNN_UNROLLED14_W16: return pk.stg ? fn(HostStaged<CnnUnrolled14W16>{}) : fn(CnnUnrolled14W16{});
#if defined(FX_AB)
        case CNN_TWO_TILES_W4: return fx_cnn_with_conv1<TwoTiles<Waves4<CnnForm>>>(pk, fn);
        case CNN_TWO_TILES_W8: return fx_cnn_with_conv1<TwoTiles<CnnForm>>(pk, fn);
        case CNN_UNROLLED8_W16_NOPRIO: return fn(NoPrio<CnnUnrolled8W16>{});
        case CNN_UNROLLED14_W16_NOPRIO: return fn(NoPrio<CnnUnrolled14W16>{});
        case CNN_PROTEIN_W4: return fx_cnn_with_conv1<CnnProteinW4>(pk, fn);
#endif
        case CNN_BINARY_W8: return fn(CnnBinary8{});
        case CNN_BINARY_W16: return fn(Waves16<CnnBinary8>{});
        case CNN_BINARY_SEG: return fn(Segmented<CnnBinary8>{});
        case CNN_NARROW_W8: return fn(CnnNarrow8{});
        case CNN_NARROW_W16: return fn(Waves16<CnnNarrow8>{});
        case CNN_NARROW_SEG: return fn(Segmented<CnnNarrow8>{});
        case CNN_NARROW_PROTEIN_W8: return fn(CnnNarrowProtein8{});
        case CNN_K3_W8: return fn(CnnK3W8{});
        case CNN_K3_W16: return fn(Waves16<CnnK3W8>{});
        case CNN_K3_SEG: return fn(Segmented<CnnK3W8>{});
        case CNN_K7_W8: return fn(CnnK7W8{});
        default: return FX_EUNSUPPORTED;
    }
}

// ---------------------------------------------------------------- pooled-feature table (score_cnn_pooled.hip)
// A seq_len = 8 row over four letters has 4^8 values, and everything in front of the dense head is a function of the row alone: a canonical
// member (the shapes with a conv1 table, FxPackLayout::off_c1tab) may carry its global-max-pooled features for every row, FX_POOL_ROWS lines of 32
// floats, and a launch then runs only the head (k_score_cnn_mfma_pooled).  What a launch group does about it (engine option cnn_pool_table):
#define FX_POOL_ROWS 65536      // 4^8 rows, index = sum_j code[j] * 4^j: the 16-bit `codes` word of the C1T branch
enum CnnPoolDecision : int {
    CNN_POOL_NO = 0,            // the form fx_cnn_pick_fused named is launched, as without the option
    CNN_POOL_USE = 1,           // every member's table is fresh: the head-only kernel
    CNN_POOL_BUILD = 2,         // the stale members' tables are built first, then the head-only kernel
};
// `pk` is the launch's pick and is launched unchanged when the answer is CNN_POOL_NO.  The table form stands in for the 16-wave unrolled form
// only, with the rows in device memory when the kernel starts.  A stale table is built when the launch is longer than the enumeration (MORE
// than 4^8 rows per member: building is then no more conv work than the launch would do itself), or whatever its size with cnn_pool_table = 2.
inline CnnPoolDecision fx_cnn_pool_decide(const fx_engine* e, const FxRequest& rq, const FxPackLayout& lay, const CnnPick& pk, int64_t N, bool all_fresh) {
    if (e->cnn_pool_table <= 0 || lay.off_c1tab < 0) return CNN_POOL_NO;
    if (pk.rc || pk.id != CNN_UNROLLED8_W16 || pk.stg || rq.rows_on || rq.host_rows) return CNN_POOL_NO;
    if (all_fresh) return CNN_POOL_USE;
    return (e->cnn_pool_table >= 2 || N > FX_POOL_ROWS) ? CNN_POOL_BUILD : CNN_POOL_NO;
}

// ... and the score itself is a function of the row and the member's weights too: such a member may carry its SCORE for every row as well,
// FX_POOL_ROWS floats at the same index (fx_model::d_scoretab, built by the head-only kernel over the enumeration of all rows), and a launch is
// then one table read per row and member (k_score_cnn_mfma_scoretab, score_cnn_lookup.hip).  Engine option cnn_score_table, layered on the
// answer above: it never makes a launch take a table that cnn_pool_table would not, and never builds where that would not build.
enum CnnScoreDecision : int {
    CNN_SCORE_NO = 0,           // what fx_cnn_pool_decide answered runs as without the option: the conv form or the head-only kernel
    CNN_SCORE_LOOKUP = 1,       // the group's score tables are brought up to date (pooled-feature tables first, as `pool` says), then the lookup kernel
};
inline CnnScoreDecision fx_cnn_score_decide(const fx_engine* e, CnnPoolDecision pool) {
    return (pool != CNN_POOL_NO && e->cnn_score_table >= 1) ? CNN_SCORE_LOOKUP : CNN_SCORE_NO;
}

// ---------------------------------------------------------------- conv part of the two-kernel path (score_cnn_split.hip)
inline int fx_cnn_split_supported(const fx_engine* e, const FxShape& s, const FxPackLayout& lay, int M) {
    // (binary alphabet, sequence_utils.py:16's BA: the canonical conv shape only -- its fused kernel covers 97..112 hidden units, this path the rest)
    if ((s.A != 4 && s.A != 20 && s.A != 2) || lay.FT < 1 || lay.FT > 4 || s.K < 2 || s.K > 7 || s.H > 256 || M > FX_MAX_M ||
        e->cnn_conv1_mfma || (s.A == 20 && (lay.FT != 2 || !e->cnn_pair)) || (s.A == 2 && (lay.FT != 2 || s.K != 5)))
        return FX_EUNSUPPORTED;
    if (s.A != 20 && (size_t)lay.conv_floats * 4 + 256 + 48 > (size_t)e->max_lds) return FX_EUNSUPPORTED;
    return FX_OK;
}

// conv part only: one tile per wave, 8 waves, conv weights in LDS, first layer in gather form
inline CnnPick fx_cnn_pick_conv(const fx_engine* e, const FxRequest& rq, const FxShape& s, const FxPackLayout& lay, int64_t N, int M) {
    CnnPick pk;
    pk.rc = fx_cnn_split_supported(e, s, lay, M);
    pk.pair_first = s.A == 20;                           // protein alphabet: the conv part is the two-waves-per-tile kernel (score_cnn_pair.hip)
    if (pk.rc || pk.pair_first) return pk;
    pk.TG = (N + 15) / 16;
    pk.K = s.K; pk.FT = lay.FT; pk.HT = 1;
    pk.dense_lds = false;
    pk.lds = (size_t)lay.conv_floats * 4 + 256 + 48;
    const int64_t U = pk.TG * M;
    if (s.A == 2) { pk.id = CNN_CONV_BINARY; return pk; }
    if (s.K > 5 && lay.FT > 2) { pk.rc = FX_EUNSUPPORTED; return pk; }   // (3-4 channel tiles: the 6- and 7-tap windows do not fit the register file)
    // small batch of long sequences (an explorer's 1-100 sequence call): the 8 waves of a workgroup split one
    // tile's positions, as in the fused kernel -- bit-identical to the one-wave walk (K * 3 <= 16: the ring-window form)
    if (s.K * 3 <= 16 && fx_cnn_segmented(e, U, s.L - s.K + 1, 24, pk.lds, lay.FT)) pk.id = CNN_CONV_SEG;
    // batch launches (the wide-head path, round 6): four waves per SIMD, and the unrolled walk of the canonical short landscape
    else if (s.K == 5 && lay.FT == 2 && fx_cnn_units_per_cu(e, U, 16) && !rq.rows_on) pk.id = s.L == 8 ? CNN_CONV_UNROLLED8_W16 : CNN_CONV_W16;
    else pk.id = CNN_CONV_W8;
    return pk;
}

template <class Fn>
int fx_cnn_with_conv_form(const CnnPick& pk, Fn&& fn) {
    switch (pk.id) {
        case CNN_CONV_W8:
            return fx_cnn_lift<1, 2, 3, 4>(pk.FT, [&](auto ft) {
                return fx_cnn_lift<2, 3, 4, 5, 6, 7>(pk.K, [&](auto k) {
                    if constexpr (decltype(k)::value > 5 && decltype(ft)::value > 2) return (int)FX_EUNSUPPORTED;
                    else return fn(CnnConv<decltype(k)::value, decltype(ft)::value>{});
                });
            });
        case CNN_CONV_SEG:
            return fx_cnn_lift<1, 2, 3, 4>(pk.FT, [&](auto ft) {
                return fx_cnn_lift<2, 3, 4, 5>(pk.K, [&](auto k) { return fn(Segmented<CnnConv<decltype(k)::value, decltype(ft)::value>>{}); });
            });
        case CNN_CONV_W16: return fn(Waves16<CnnConv<5, 2>>{});
        case CNN_CONV_UNROLLED8_W16: return fn(Unrolled<Waves16<CnnConv<5, 2>>, 4>{});
        case CNN_CONV_BINARY: return fn(Alphabet<CnnConv<5, 2>, 2>{});
        default: return FX_EUNSUPPORTED;
    }
}

// The fields of a form in the order of the comment at the head of score_cnn_kernel.h (fx_debug_cnn_form_pick).
template <class F>
void fx_cnn_form_fields(int64_t* out16) {
    const int64_t v[16] = {F::A, F::K, F::FT, F::HT, F::NT, F::DENSE_LDS, F::WAVES, F::G1, F::L1S, F::PRIO, F::SEG, F::HEAD, F::STG, F::QT, F::C1T, F::C2P};
    for (int i = 0; i < 16; ++i) out16[i] = v[i];
}

}  // namespace
