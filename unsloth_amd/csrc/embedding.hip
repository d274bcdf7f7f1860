// Token embedding: out[t] = W[ids[t]] and its weight gradient dW[v] = sum over the tokens t with ids[t] == v of dY[t].
//
// Rows are moved as 16-byte vectors (8 x 16-bit), a lane owning vector c of a row. A row of H / 8 vectors is covered by a LANE
// GROUP of lpr = min(64, next power of two >= H / 8) lanes: a whole wave for H >= 512, a part of one for a narrow row, so that
// a 64-column embedding keeps eight groups of a wave busy with eight different rows instead of idling 56 lanes. Wider rows are cut
// into column chunks of lpr vectors (backward) or walked by the group (forward).
//
// forward   a lane group gathers EMB_FWD_ROWS rows at once: the ids of all of them first, then per vector column every row's
//           load is issued before the first store -- four independent 16-byte requests in flight per lane. 8192 x 4096 is
//           2048 waves in 512 workgroups. An id outside [0, V) reads nothing and stores a zero row.
//
// backward  over the ids SORTED (stable, with `order[i]` the token of sorted position i). A run is a maximal stretch of equal ids;
//           it is summed in fp32 in ascending position and rounded once, by one owner, with no atomics: the same bits every launch.
//             runs     work item = (block of EMB_PB sorted positions) x (column chunk). The item finds the run starts of its block
//                      by comparing neighbours, skips the positions at its front that continue an earlier item's run, and owns
//                      every run that starts in its block -- following it PAST the block's end, up to the end of the SEGMENT.
//             segments positions are also cut at the fixed multiples of EMB_SEG. A run that crosses such a cut is not followed
//                      across it: each side's piece is summed by the item that holds the piece's first position and stored in
//                      fp32 to ws[segment][0] (the piece entering the segment from the left) or ws[segment][1] (the piece leaving
//                      it to the right); a segment has at most one of each.
//             combine  one lane group per (segment, column chunk): where a run starts in the segment and leaves it, ws[s][1] and
//                      the ws[k][0] of the following segments are added in ascending k and stored. A fixed order again.
//           So a batch whose tokens all carry one id is n / EMB_SEG x H / 512 pieces of EMB_SEG rows, not one serial sum, while a
//           usual batch (runs of a few rows, one cut per 128 positions) pays two fp32 rows per segment for it.
//             zero     (mode 0) a lane per vocabulary row binary-searches the sorted ids; the wave then clears the rows nobody
//                      references (and the padding row). With `runs` and `combine` every element of dW is written exactly once.
#include "common.h"

namespace {

constexpr int EMB_THREADS = 256;
constexpr int EMB_FWD_ROWS = 4;      // rows a lane group gathers together
constexpr int EMB_PB = 16;           // sorted positions per work item of the backward
constexpr int EMB_SEG = 128;         // fixed cut of long runs (a multiple of EMB_PB)
constexpr int EMB_UNROLL = 4;        // rows of a run loaded before the first is added
static_assert(EMB_SEG % EMB_PB == 0, "a position block lies in one segment");

// log2 of the lanes per row: the smallest power of two >= nvec, at most a wave
inline int lane_group_log2(int nvec) {
    int lg = 0;
    while (lg < 6 && (1 << lg) < nvec) ++lg;
    return lg;
}

template <typename T>
__global__ void __launch_bounds__(EMB_THREADS) embedding_fwd_kernel(const long long* __restrict__ ids, long long n,
                                                                    const T* __restrict__ W, long long ldw, long long V,
                                                                    T* __restrict__ out, long long ld_out, int nvec, int lg) {
    const int lpr = 1 << lg, c0 = threadIdx.x & (lpr - 1);
    const long long group = (long long)blockIdx.x * (EMB_THREADS >> lg) + (threadIdx.x >> lg);
    const long long r0 = group * EMB_FWD_ROWS;
    if (r0 >= n) return;
    const T* src[EMB_FWD_ROWS];
#pragma unroll
    for (int k = 0; k < EMB_FWD_ROWS; ++k) {
        const long long id = (r0 + k < n) ? ids[r0 + k] : -1;
        src[k] = (id >= 0 && id < V) ? W + id * ldw : nullptr;
    }
    for (int c = c0; c < nvec; c += lpr) {
        Vec16<T> v[EMB_FWD_ROWS];
#pragma unroll
        for (int k = 0; k < EMB_FWD_ROWS; ++k) {
            if (src[k]) v[k] = ld16(src[k] + 8 * c);
            else v[k].raw = make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int k = 0; k < EMB_FWD_ROWS; ++k)
            if (r0 + k < n) st16(out + (r0 + k) * ld_out + 8 * c, v[k]);
    }
}

struct EmbBwd {
    const long long* ids;     // sorted
    const long long* order;   // order[i]: row of dY of sorted position i
    long long n;
    const void* dY;
    long long ld_dy;
    void* dW;
    long long ld_dw;
    long long V, pad;
    float* ws;                // [segments][2][H]
    int H, nvec, lg, ncc, mode;
};

__device__ __forceinline__ bool emb_counts(const EmbBwd& a, long long id) { return id >= 0 && id < a.V && id != a.pad; }

// the one rounding of a gradient row: rn(acc), or rn(fp32(dW) + acc) when accumulating
template <typename T>
__device__ __forceinline__ void emb_store(T* dst, const float* acc, int mode) {
    Vec16<T> o;
    if (mode) {
        o = ld16(dst);
#pragma unroll
        for (int q = 0; q < 8; ++q) o.e[q] = from_f32<T>(to_f32(o.e[q]) + acc[q]);
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) o.e[q] = from_f32<T>(acc[q]);
    }
    st16(dst, o);
}

template <typename T>
__device__ __forceinline__ Vec16<T> emb_row(const EmbBwd& a, const T* dYc, long long row) {
    Vec16<T> v;
    if ((unsigned long long)row < (unsigned long long)a.n) v = ld16(dYc + row * a.ld_dy);      // (a bad `order` reads nothing)
    else v.raw = make_uint4(0u, 0u, 0u, 0u);
    return v;
}

template <typename T>
__global__ void __launch_bounds__(EMB_THREADS) embedding_bwd_runs_kernel(EmbBwd a) {
    const int lpr = 1 << a.lg;
    const long long item = (long long)blockIdx.x * (EMB_THREADS >> a.lg) + (threadIdx.x >> a.lg);
    const long long pb = item / a.ncc;
    const int c = (int)(item % a.ncc) * lpr + (threadIdx.x & (lpr - 1));
    const long long p0 = pb * EMB_PB;
    if (p0 >= a.n || c >= a.nvec) return;
    const long long p1 = min(a.n, p0 + EMB_PB), seg = p0 / EMB_SEG, s0 = seg * EMB_SEG, s1 = min(a.n, s0 + EMB_SEG);
    const T* dYc = reinterpret_cast<const T*>(a.dY) + 8 * c;
    long long i = p0;
    if (i > s0) {                                          // the front of the block continues a piece that started before it
        const long long prev = a.ids[i - 1];
        while (i < p1 && a.ids[i] == prev) ++i;
    }
    while (i < p1) {
        const long long id = a.ids[i];
        long long e = i + 1;                               // the piece [i, e): to the end of the run or of the segment
        while (e < s1 && a.ids[e] == id) ++e;
        if (emb_counts(a, id)) {
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            long long j = i;
            for (; j + EMB_UNROLL <= e; j += EMB_UNROLL) {
                long long r[EMB_UNROLL];
                Vec16<T> v[EMB_UNROLL];
#pragma unroll
                for (int u = 0; u < EMB_UNROLL; ++u) r[u] = a.order[j + u];
#pragma unroll
                for (int u = 0; u < EMB_UNROLL; ++u) v[u] = emb_row(a, dYc, r[u]);
#pragma unroll
                for (int u = 0; u < EMB_UNROLL; ++u)
#pragma unroll
                    for (int q = 0; q < 8; ++q) acc[q] += to_f32(v[u].e[q]);
            }
            for (; j < e; ++j) {
                const Vec16<T> v = emb_row(a, dYc, a.order[j]);
#pragma unroll
                for (int q = 0; q < 8; ++q) acc[q] += to_f32(v.e[q]);
            }
            const bool head = i == s0 && i > 0 && a.ids[i - 1] == id;      // entered the segment from the left
            const bool tail = e == s1 && e < a.n && a.ids[e] == id;        // leaves it to the right
            if (head || tail) {
                float4* w = reinterpret_cast<float4*>(a.ws + (seg * 2 + (head ? 0 : 1)) * a.H + 8 * c);
                w[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
                w[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
            } else {
                emb_store(reinterpret_cast<T*>(a.dW) + id * a.ld_dw + 8 * c, acc, a.mode);
            }
        }
        i = e;
    }
}

template <typename T>
__global__ void __launch_bounds__(EMB_THREADS) embedding_bwd_combine_kernel(EmbBwd a) {
    const int lpr = 1 << a.lg;
    const long long item = (long long)blockIdx.x * (EMB_THREADS >> a.lg) + (threadIdx.x >> a.lg);
    const long long s = item / a.ncc;
    const int c = (int)(item % a.ncc) * lpr + (threadIdx.x & (lpr - 1));
    const long long s1 = (s + 1) * EMB_SEG;
    if (s1 >= a.n || c >= a.nvec) return;
    const long long id = a.ids[s1];
    if (a.ids[s1 - 1] != id || !emb_counts(a, id)) return;              // no run crosses the right edge of segment s
    if (s > 0 && a.ids[s * EMB_SEG - 1] == id) return;                  // it started further left: that segment combines it
    const float4* w = reinterpret_cast<const float4*>(a.ws + (s * 2 + 1) * a.H + 8 * c);
    float4 x = w[0], y = w[1];
    float acc[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
    for (long long k = s + 1; k * EMB_SEG < a.n && a.ids[k * EMB_SEG] == id; ++k) {
        w = reinterpret_cast<const float4*>(a.ws + (k * 2) * a.H + 8 * c);
        x = w[0];
        y = w[1];
        acc[0] += x.x; acc[1] += x.y; acc[2] += x.z; acc[3] += x.w;
        acc[4] += y.x; acc[5] += y.y; acc[6] += y.z; acc[7] += y.w;
    }
    emb_store(reinterpret_cast<T*>(a.dW) + id * a.ld_dw + 8 * c, acc, a.mode);
}

// mode 0: the rows of dW no run writes. Lane l of a wave looks row 64 * wave + l up in the sorted ids; the wave clears the misses.
template <typename T>
__global__ void __launch_bounds__(EMB_THREADS) embedding_bwd_zero_kernel(EmbBwd a) {
    const int lane = threadIdx.x & 63;
    const long long base = ((long long)blockIdx.x * (EMB_THREADS / UAMD_WAVE) + (threadIdx.x >> 6)) * UAMD_WAVE;
    const long long v = base + lane;
    bool clear = false;
    if (v < a.V) {
        long long lo = 0, hi = a.n;
        while (lo < hi) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (a.ids[mid] < v) lo = mid + 1;
            else hi = mid;
        }
        clear = !(lo < a.n && a.ids[lo] == v && v != a.pad);
    }
    unsigned long long todo = __ballot(clear);
    Vec16<T> z;
    z.raw = make_uint4(0u, 0u, 0u, 0u);
    while (todo) {
        const int b = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        T* row = reinterpret_cast<T*>(a.dW) + (base + b) * a.ld_dw;
        for (int c = lane; c < a.nvec; c += UAMD_WAVE) st16(row + 8 * c, z);
    }
}

inline bool emb_row_aligned(const void* p, int64_t ld) { return aligned16(p) && ld % 8 == 0; }
inline long long emb_blocks(long long items, int lg) {
    const long long per = EMB_THREADS >> lg;
    return (items + per - 1) / per;
}

}  // namespace

extern "C" int uamd_embedding_fwd(const int64_t* ids, int64_t n, const void* W, int64_t ldw, int64_t V, int H, void* out,
                                  int64_t ld_out, int dtype, void* stream) {
    if (n < 0 || V <= 0 || H <= 0 || H % 8 || (n > 0 && (!ids || !out)) || !W || ldw < H || ld_out < H) return UAMD_ERR_ARG;
    if (!emb_row_aligned(W, ldw) || !emb_row_aligned(out, ld_out)) return UAMD_ERR_ALIGN;
    if (n == 0) return UAMD_OK;
    const int nvec = H / 8, lg = lane_group_log2(nvec);
    const long long blocks = emb_blocks((n + EMB_FWD_ROWS - 1) / EMB_FWD_ROWS, lg);
    if (blocks > 0x7fffffffLL) return UAMD_ERR_ARG;
    UAMD_DISPATCH_HALF(dtype, hipLaunchKernelGGL(embedding_fwd_kernel<T>, dim3((unsigned)blocks), dim3(EMB_THREADS), 0,
                                                 (hipStream_t)stream, (const long long*)ids, (long long)n, (const T*)W,
                                                 (long long)ldw, (long long)V, (T*)out, (long long)ld_out, nvec, lg));
    return uamd_launch_status();
}

extern "C" int64_t uamd_embedding_bwd_workspace(int64_t n, int H) {
    if (n <= 0 || H <= 0) return 0;
    return (n + EMB_SEG - 1) / EMB_SEG * 2 * (int64_t)H;
}

extern "C" int uamd_embedding_bwd(const int64_t* sorted_ids, const int64_t* order, int64_t n, const void* dY, int64_t ld_dy,
                                  void* dW, int64_t ld_dw, int64_t V, int H, int64_t padding_idx, int mode, float* ws,
                                  int64_t ws_elems, int dtype, void* stream) {
    if (n < 0 || V <= 0 || H <= 0 || H % 8 || !dW || ld_dw < H || (mode != 0 && mode != 1)) return UAMD_ERR_ARG;
    if (n > 0 && (!sorted_ids || !order || !dY || !ws || ld_dy < H || ws_elems < uamd_embedding_bwd_workspace(n, H)))
        return UAMD_ERR_ARG;
    if (!emb_row_aligned(dW, ld_dw) || (n > 0 && (!emb_row_aligned(dY, ld_dy) || !aligned16(ws)))) return UAMD_ERR_ALIGN;
    EmbBwd a;
    a.ids = (const long long*)sorted_ids;
    a.order = (const long long*)order;
    a.n = n;
    a.dY = dY;
    a.ld_dy = ld_dy;
    a.dW = dW;
    a.ld_dw = ld_dw;
    a.V = V;
    a.pad = padding_idx;
    a.ws = ws;
    a.H = H;
    a.nvec = H / 8;
    a.lg = lane_group_log2(a.nvec);
    a.ncc = (a.nvec + (1 << a.lg) - 1) >> a.lg;
    a.mode = mode;
    const long long zero_blocks = (V + EMB_THREADS - 1) / EMB_THREADS;
    const long long run_blocks = emb_blocks((n + EMB_PB - 1) / EMB_PB * a.ncc, a.lg);
    const long long comb_blocks = emb_blocks((n + EMB_SEG - 1) / EMB_SEG * a.ncc, a.lg);
    if (zero_blocks > 0x7fffffffLL || run_blocks > 0x7fffffffLL) return UAMD_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    UAMD_DISPATCH_HALF(dtype, {
        if (mode == 0)
            hipLaunchKernelGGL(embedding_bwd_zero_kernel<T>, dim3((unsigned)zero_blocks), dim3(EMB_THREADS), 0, st, a);
        if (n > 0) {
            hipLaunchKernelGGL(embedding_bwd_runs_kernel<T>, dim3((unsigned)run_blocks), dim3(EMB_THREADS), 0, st, a);
            if (n > EMB_SEG)
                hipLaunchKernelGGL(embedding_bwd_combine_kernel<T>, dim3((unsigned)comb_blocks), dim3(EMB_THREADS), 0, st, a);
        }
    });
    return uamd_launch_status();
}
