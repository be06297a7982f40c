// The per-member tables of the fused CNN kernel's C1T / C2P forms (score_cnn_kernel.h), built on the device at fx_model_set_weights.
// Compiled as the tail of score_cnn_mfma.hip, not as a unit of its own: alone, k_build_conv2_prefix comes out of the compiler with another
// schedule and register assignment (same instructions) than in the module of the scoring kernels, where its tables were tested and measured.
#pragma once
#include "fx_common.h"
#include "mfma_common.h"

namespace {

// The conv1 table of one member (C1T): one thread per (window, four channels).  The arithmetic is the gather's, step for step -- the bias, then
// the kernel rows of taps 0 .. 4 added in that order as f4 sums, then relu4 on the float bits -- and it runs on the device that runs the
// gather, so infinities, NaNs (whose SIGN decides what the integer-max ReLU makes of them) and denormals come out as they do there.
__global__ void __launch_bounds__(256) k_build_conv1_table(const float* packed, int off_cb, int off_w1p, float* tab) {
    const int i = blockIdx.x * 256 + threadIdx.x;       // FX_C1T_WINDOWS x 8 threads
    const int w = i >> 3, q = i & 7;                    // channels 4q .. 4q + 3 = 16 mo + 4 g + r
    if (w >= FX_C1T_WINDOWS) return;
    f4 o = *reinterpret_cast<const f4*>(packed + off_cb + 4 * q);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int c = (w >> (2 * j)) & 3;
        o += *reinterpret_cast<const f4*>(packed + off_w1p + (j * 4 + c) * FX_C1_ROW(2) + 4 * q);
    }
    *reinterpret_cast<f4*>(tab + w * 32 + 4 * q) = relu4(o);
}

// The conv2 prefix tables of one member (C2P): one wave per 16 entries, lane (g, sq) = entry sq of the 16, channels 16 mo + 4 g + r -- the
// accumulator layout of a tile whose 16 sequences are the 16 entries.  The chain is the scoring kernel's: init_bias on the conv2 bias, then
// mma_layer<2, 2, 1> for tap j0 (and j0 + 1 at depth 2) over the packed conv2 blocks, with the conv1 table's row of the entry's window as the B
// operand in the (mi, r) order of a tile's win1 -- so every accumulator sees the MFMAs it sees in the full walk (a column of an MFMA depends on
// no other column) and the stored pre-ReLU bits are those a tile holds after its first taps.
template <int DEPTH>
__device__ __forceinline__ void fx_c2p_build_entries(const float* packed, int off_cb, int off_c2, const float* c1tab, float* tab, int j0, int idx,
                                                     int lane, int g) {
    f4 acc[2][1];
    init_bias<2, 1>(packed + off_cb + 16 * 2, acc, g);
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
        const int w = (idx >> (2 * d)) & (FX_C1T_WINDOWS - 1);       // window d of the entry = letters d .. d + 4
        f4 in[2][1];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) in[mi][0] = *reinterpret_cast<const f4*>(c1tab + w * 32 + 16 * mi + 4 * g);
        mma_layer<2, 2, 1>(reinterpret_cast<const f4*>(packed + off_c2) + (j0 + d) * 2 * 2 * 64, in, acc, lane);
    }
#pragma unroll
    for (int mo = 0; mo < 2; ++mo)
        *reinterpret_cast<f4*>(tab + ((int64_t)j0 * FX_C2P_ENTRIES(DEPTH) + idx) * 32 + 16 * mo + 4 * g) = acc[mo][0];
}
constexpr int FX_C2P_WAVES1 = FX_C2P_FAMILIES * FX_C2P_ENTRIES(1) / 16, FX_C2P_WAVES2 = FX_C2P_FAMILIES * FX_C2P_ENTRIES(2) / 16;
static_assert(FX_C2P_MAX_DEPTH == 2 && (FX_C2P_WAVES1 + FX_C2P_WAVES2) % 4 == 0, "k_build_conv2_prefix: both depths in one grid of whole 4-wave workgroups");
__global__ void __launch_bounds__(256) k_build_conv2_prefix(float* packed, int off_cb, int off_c2, int off_c1tab, int off_t1, int off_t2) {
    const int lane = threadIdx.x & 63, g = lane >> 4, sq = lane & 15;
    int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));   // the grid is exactly FX_C2P_WAVES1 + FX_C2P_WAVES2 waves
    if (wave < FX_C2P_WAVES1) {
        constexpr int per = FX_C2P_ENTRIES(1) / 16;
        fx_c2p_build_entries<1>(packed, off_cb, off_c2, packed + off_c1tab, packed + off_t1, wave / per, (wave % per) * 16 + sq, lane, g);
    } else {
        wave -= FX_C2P_WAVES1;
        constexpr int per = FX_C2P_ENTRIES(2) / 16;
        fx_c2p_build_entries<2>(packed, off_cb, off_c2, packed + off_c1tab, packed + off_t2, wave / per, (wave % per) * 16 + sq, lane, g);
    }
}

}  // namespace

int fx_build_conv2_prefix(fx_engine* e, fx_model* m) {
    const FxPackLayout& lay = m->layout;
    if (lay.off_c1tab < 0 || lay.off_c2p[0] < 0 || lay.off_c2p[1] < 0) return FX_OK;
    hipLaunchKernelGGL(k_build_conv2_prefix, dim3((FX_C2P_WAVES1 + FX_C2P_WAVES2) / 4), dim3(256), 0, e->stream, m->d_packed, (int)lay.off_cb,
                       (int)lay.off_c2, (int)lay.off_c1tab, (int)lay.off_c2p[0], (int)lay.off_c2p[1]);
    FX_HIP(e, hipGetLastError());
    return FX_OK;
}

int fx_build_conv1_table(fx_engine* e, fx_model* m) {
    const FxPackLayout& lay = m->layout;
    if (lay.off_c1tab < 0) return FX_OK;
    hipLaunchKernelGGL(k_build_conv1_table, dim3(FX_C1T_WINDOWS * 8 / 256), dim3(256), 0, e->stream, m->d_packed, (int)lay.off_cb,
                       (int)lay.off_w1p, m->d_packed + lay.off_c1tab);
    FX_HIP(e, hipGetLastError());
    return FX_OK;
}
