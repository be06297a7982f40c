// K8: top-k select over float32 scores in device memory, and the row enumerators of fx_screen_all and fx_screen_mutants
// (fx_screen.hip has the ABI).
//
// Every element becomes a 64-bit key (topk_keys.h) whose unsigned order is the whole ordering rule, ties included, and which no
// other element shares.  Two forms give the k largest keys, largest first:
//   small   one workgroup: keys into LDS, bitonic sort, every input element then looks its own rank up and, if it is below k,
//           writes its (index, value) there.  Also the merge of fx_screen_all (<= 2k candidates with GLOBAL row indices) and
//           the last step of the large form.
//   large   radix select, most significant digit first, ONE LAUNCH PER PASS: a workgroup counts the digits of the keys that
//           match the prefix chosen so far in an LDS histogram (per-wave aggregation in front of the LDS atomics: an all-equal
//           input is one add per wave) and adds its non-empty bins to the pass's global histogram (integer atomics: the sums do
//           not depend on arrival order).  The NEXT launch starts by picking the bin that holds the k-th key from that
//           histogram -- every workgroup does, from the same 256 counts, so nobody waits for anybody.  After eight passes the
//           k-th key is known exactly; a collect launch appends the keys at or above it (exactly k: keys are distinct) through an
//           atomic cursor in whatever order they arrive, and the small form sorts them.
// Nothing here waits for another workgroup: no spin, no grid barrier, no last-block hand-off.
#include "fx_common.h"
#include "fx_internal.h"
#include "mutant_rank.h"
#include "topk_keys.h"

namespace {

struct FxTopkState { unsigned long long prefix; unsigned want; unsigned pad; };   // before a pass: the digits chosen so far, winners still to find below them
struct FxTopkWork {                                  // the work area of one select (engine scratch)
    unsigned hist[FX_TOPK_PASSES][FX_TOPK_BINS];
    FxTopkState state[FX_TOPK_PASSES];
    unsigned cursor;
    unsigned pad[3];
    unsigned long long cand[FX_TOPK_MAX_K];
};

// The state before pass `done + 1` from the state before pass `done` and that pass's finished histogram.  Whole workgroup.
__device__ FxTopkState topk_next_state(const FxTopkWork* w, int done, FxTopkState* s_out) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        const FxTopkState prev = w->state[done];
        const uint4 c4 = reinterpret_cast<const uint4*>(w->hist[done])[lane];
        const unsigned c[4] = {c4.x, c4.y, c4.z, c4.w};
        const unsigned mine = c[0] + c[1] + c[2] + c[3];
        unsigned inc = mine;                                     // suffix sum over the lanes from this one up
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = __shfl_down(inc, o);
            if (lane + o < 64) inc += v;
        }
        if (lane == 0) *s_out = FxTopkState{prev.prefix, 0u, 0u};   // (fewer keys than wanted: cannot happen; nothing matches then)
        int bin; unsigned above;
        if (fx_topk_pick_lane(c, inc - mine, prev.want, lane, &bin, &above))
            *s_out = FxTopkState{fx_topk_extend(prev.prefix, bin, done), prev.want - above, 0u};
    }
    __syncthreads();
    return *s_out;
}

// One wave's votes into the workgroup's LDS histogram.  Up to four rounds of "the first live lane's digit: one add for all lanes
// that share it" -- an input of one, two or a few values costs a handful of LDS atomics per wave instead of 64 on one address --
// then whoever is left adds for itself.
__device__ __forceinline__ void topk_count(unsigned* s_hist, bool m, int d) {
    const int lane = threadIdx.x & 63;
    unsigned long long live = __ballot(m);
    for (int r = 0; r < 4 && live; ++r) {
        const int leader = __ffsll((long long)live) - 1;
        const int d0 = __shfl(d, leader);
        const unsigned long long same = __ballot(m && d == d0);
        if (lane == leader) atomicAdd(&s_hist[d0], (unsigned)__popcll(same));
        if (d == d0) m = false;
        live &= ~same;
    }
    if (m) atomicAdd(&s_hist[d], 1u);
}

__global__ __launch_bounds__(256) void k_topk_hist(const float* __restrict__ scores, int64_t N, int pass, unsigned want0, FxTopkWork* w) {
    __shared__ unsigned s_hist[FX_TOPK_BINS];
    __shared__ FxTopkState s_state;
    s_hist[threadIdx.x] = 0;
    FxTopkState S;
    if (pass == 0) { S = FxTopkState{0ull, want0, 0u}; __syncthreads(); }
    else S = topk_next_state(w, pass - 1, &s_state);
    if (blockIdx.x == 0 && threadIdx.x == 0) w->state[pass] = S;
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < N; base += step) {      // (workgroup-uniform trip count: the ballots see whole waves)
        const int64_t i = base + threadIdx.x;
        bool m = i < N;
        int d = 0;
        if (m) {
            const unsigned long long key = fx_topk_key64(__float_as_uint(scores[i]), (uint32_t)i);
            m = S.want != 0 && fx_topk_matches(key, S.prefix, pass);
            d = fx_topk_digit(key, pass);
        }
        topk_count(s_hist, m, d);
    }
    __syncthreads();
    const unsigned c = s_hist[threadIdx.x];
    if (c) atomicAdd(&w->hist[pass][threadIdx.x], c);
}

__global__ __launch_bounds__(256) void k_topk_collect(const float* __restrict__ scores, int64_t N, unsigned kk, FxTopkWork* w) {
    __shared__ FxTopkState s_state;
    const FxTopkState S = topk_next_state(w, FX_TOPK_PASSES - 1, &s_state);
    if (S.want == 0) return;
    const unsigned long long kth = S.prefix;
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += step) {
        const unsigned long long key = fx_topk_key64(__float_as_uint(scores[i]), (uint32_t)i);
        if (key >= kth) {
            const unsigned pos = atomicAdd(&w->cursor, 1u);
            if (pos < kk) w->cand[pos] = key;                    // (exactly kk keys qualify; the guard keeps a wrong count inside the buffer)
        }
    }
}

// mode 0: element i = (vals[i], index i)               -> out (idx_base + i, vals[i])            [stand-alone, small input]
// mode 1: element i = key cand[i] of scores `vals`     -> out (idx_base + index, vals[index])     [behind the collect launch]
// mode 2: element i = (vals[i], index gidx[i] < 2^31)  -> out (gidx[i], vals[i])                  [merge of fx_screen_all]
// n <= P <= FX_TOPK_SMALL_MAX, P a power of two; the first kk <= n entries of the sorted order are written.  limit = elements of
// `vals` (mode 1 reads vals at an index taken from a key: checked against it).
__global__ __launch_bounds__(1024) void k_topk_small(const float* __restrict__ vals, const int64_t* __restrict__ gidx,
                                                     const unsigned long long* __restrict__ cand, int mode, int n, int P, int kk,
                                                     int64_t limit, int64_t idx_base, int64_t* __restrict__ out_idx, float* __restrict__ out_val) {
    __shared__ unsigned long long s[FX_TOPK_SMALL_MAX];
    const int tid = threadIdx.x;
    auto key_of = [&](int i) -> unsigned long long {
        if (mode == 1) return cand[i];
        return fx_topk_key64(__float_as_uint(vals[i]), mode == 2 ? (uint32_t)gidx[i] : (uint32_t)i);
    };
    for (int i = tid; i < P; i += 1024) s[i] = i < n ? key_of(i) : 0ull;       // (0 is below every real key)
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += 1024) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int hi = lo | j;
                const bool desc = (lo & k2) == 0;
                const unsigned long long a = s[lo], b = s[hi];
                if ((a < b) == desc) { s[lo] = b; s[hi] = a; }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < n; i += 1024) {
        const unsigned long long q = key_of(i);
        int lo = 0, hi = P;                                                      // first position whose key is not above q: q's own
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s[mid] > q) lo = mid + 1; else hi = mid;
        }
        if (lo < kk) {
            const uint32_t index = fx_topk_index_of(q);
            if (mode == 1 && (int64_t)index >= limit) continue;
            out_idx[lo] = mode == 2 ? gidx[i] : idx_base + (int64_t)index;
            out_val[lo] = mode == 1 ? vals[index] : vals[i];
        }
    }
}

struct FxAlphabet { uint8_t c[256]; };

// Row v of the enumeration = the base-A digits of v, position 0 most significant, digit d -> alphabet[d]: the order of
// itertools.product(alphabet, repeat = L).  One thread per row; v < 2^31.
__global__ __launch_bounds__(256) void k_enumerate_rows(uint8_t* __restrict__ rows, int64_t row0, int64_t n, int L, unsigned A, FxAlphabet al) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += step) {
        unsigned v = (unsigned)(row0 + t);
        uint8_t* o = rows + t * L;
        for (int p = L - 1; p >= 0; --p) {
            const unsigned q = v / A;
            o[p] = al.c[v - q * A];
            v = q;
        }
    }
}

// Rows [row0, row0 + n) of the mutant enumeration (mutant_rank.h: global row = parent * B + local) as ONE FLAT BYTE STREAM: byte b
// of the chunk is column b % L of row b / L, and a thread produces the 16 consecutive bytes of unit u = b / 16 -- the tail of one
// row, whole rows where L < 16, the head of the next -- and stores them with one aligned 16-byte store, so a wave writes 1 KiB of
// consecutive addresses whatever L is (fx_mutant_unit, mutant_rank.h).  Each row piece is the parent's bytes (read through L2: a wave's pieces belong to one or
// two parents) with the row's at most two changed columns patched.  Units reach past the last row to the end of the 16-byte tail
// pad the scoring kernels may read: those bytes are the alphabet's first letter.  The caller's buffer holds 16 * units bytes.
__global__ __launch_bounds__(256) void k_enumerate_mutants(uint4* __restrict__ out, int64_t units, int64_t row0, int64_t n, int L, int A, uint32_t B,
                                                           const uint8_t* __restrict__ parents, const uint8_t* __restrict__ codes,
                                                           const uint8_t* __restrict__ alphabet) {
    __shared__ uint8_t s_al[256];
    s_al[threadIdx.x] = alphabet[threadIdx.x];
    __syncthreads();
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < units; u += step) {
        const FxMutantUnit v = fx_mutant_unit(u, row0, n, L, A, B, parents, codes, s_al);
        out[u] = make_uint4((uint32_t)v.lo, (uint32_t)(v.lo >> 32), (uint32_t)v.hi, (uint32_t)(v.hi >> 32));
    }
}

int grid_for(const fx_engine* e, int64_t N) {
    const int64_t want = (N + 255) / 256, cap = (int64_t)e->num_cus * 8;
    return (int)std::max<int64_t>(1, std::min(want, cap));
}

int pow2_at_least(int n) {
    int P = 64;
    while (P < n) P <<= 1;
    return P;
}

}  // namespace

// Work area of the large form: engine scratch slot 6, one fixed size (allocated by the first select of an engine).
static int topk_work(fx_engine* e, FxTopkWork** out) {
    void* p = nullptr;
    if (int rc = fx_scratch(e, 6, sizeof(FxTopkWork), &p)) return rc;
    *out = (FxTopkWork*)p;
    return FX_OK;
}

int fx_launch_topk(fx_engine* e, const float* d_scores, int64_t N, int kk, int64_t idx_base, int64_t* d_idx, float* d_val) {
    if (N < 1 || kk < 1 || kk > FX_TOPK_MAX_K || kk > N || N > 0x7FFFFFFFll) return fx_fail(e, FX_EINVAL, "fx_launch_topk: bad sizes");
    if (N <= e->topk_small_rows && N <= FX_TOPK_SMALL_MAX) {
        hipLaunchKernelGGL(k_topk_small, dim3(1), dim3(1024), 0, e->stream, d_scores, (const int64_t*)nullptr, (const unsigned long long*)nullptr, 0,
                           (int)N, pow2_at_least((int)N), kk, N, idx_base, d_idx, d_val);
        FX_HIP(e, hipGetLastError());
        return FX_OK;
    }
    FxTopkWork* w = nullptr;
    if (int rc = topk_work(e, &w)) return rc;
    FX_HIP(e, hipMemsetAsync(w, 0, sizeof(FxTopkWork), e->stream));
    const int grid = grid_for(e, N);
    for (int pass = 0; pass < FX_TOPK_PASSES; ++pass)
        hipLaunchKernelGGL(k_topk_hist, dim3(grid), dim3(256), 0, e->stream, d_scores, N, pass, (unsigned)kk, w);
    hipLaunchKernelGGL(k_topk_collect, dim3(grid), dim3(256), 0, e->stream, d_scores, N, (unsigned)kk, w);
    hipLaunchKernelGGL(k_topk_small, dim3(1), dim3(1024), 0, e->stream, d_scores, (const int64_t*)nullptr, (const unsigned long long*)w->cand, 1,
                       kk, pow2_at_least(kk), kk, N, idx_base, d_idx, d_val);
    FX_HIP(e, hipGetLastError());
    e->counters.topk_large_launches += 1;
    return FX_OK;
}

int fx_launch_topk_merge(fx_engine* e, const int64_t* d_gidx, const float* d_vals, int n, int kk, int64_t* d_idx, float* d_val) {
    if (n < 1 || n > FX_TOPK_SMALL_MAX || kk < 1 || kk > n) return fx_fail(e, FX_EINVAL, "fx_launch_topk_merge: bad sizes");
    hipLaunchKernelGGL(k_topk_small, dim3(1), dim3(1024), 0, e->stream, d_vals, d_gidx, (const unsigned long long*)nullptr, 2, n, pow2_at_least(n), kk,
                       (int64_t)n, (int64_t)0, d_idx, d_val);
    FX_HIP(e, hipGetLastError());
    return FX_OK;
}

int fx_launch_enumerate_rows(fx_engine* e, uint8_t* d_rows, int64_t row0, int64_t n, int L, int A, const uint8_t* alphabet) {
    if (n < 1 || L < 1 || A < 1 || A > 256 || row0 < 0 || row0 + n > 0x7FFFFFFFll) return fx_fail(e, FX_EINVAL, "fx_launch_enumerate_rows: bad sizes");
    FxAlphabet al;
    for (int i = 0; i < 256; ++i) al.c[i] = i < A ? alphabet[i] : 0;
    hipLaunchKernelGGL(k_enumerate_rows, dim3(grid_for(e, n)), dim3(256), 0, e->stream, d_rows, row0, n, L, (unsigned)A, al);
    FX_HIP(e, hipGetLastError());
    return FX_OK;
}

int fx_launch_enumerate_mutants(fx_engine* e, uint8_t* d_rows, int64_t row0, int64_t n, int L, int A, int64_t B, int64_t P,
                                const uint8_t* d_parents, const uint8_t* d_codes, const uint8_t* d_alphabet) {
    if (n < 1 || L < 1 || A < 1 || A > 256 || B < 1 || P < 1 || row0 < 0 || fx_mutant_total_rows(P, B) < row0 + n || ((uintptr_t)d_rows & 15))
        return fx_fail(e, FX_EINVAL, "fx_launch_enumerate_mutants: bad sizes");
    const int64_t units = (n * L + 16 + 15) / 16;          // the rows and the whole 16-byte tail pad: d_rows holds 16 * units <= n * L + 32 bytes
    hipLaunchKernelGGL(k_enumerate_mutants, dim3(grid_for(e, units)), dim3(256), 0, e->stream, (uint4*)d_rows, units, row0, n, L, A, (uint32_t)B,
                       d_parents, d_codes, d_alphabet);
    FX_HIP(e, hipGetLastError());
    e->counters.mutant_rows_enumerated += n;
    return FX_OK;
}
