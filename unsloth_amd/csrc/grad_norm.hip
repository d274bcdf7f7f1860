// Global L2 norm of a flat gradient buffer and the clipping factor, both left on the device (optim.FlatAdamW /
// full_finetune.ShardedAdamW with `max_grad_norm`; the reference clips through HF Trainer, max_grad_norm = 1.0 by default).
// The factor is read by the *_clip AdamW entry points (csrc/adamw.hip) straight from device memory, so nothing between the
// backward and the optimizer step waits for the host.
//
// Stage 1, uamd_grad_sumsq: P = uamd_grad_sumsq_parts(n) workgroups, one per PART of the buffer.
//   split   L = ceil(n / P) rounded up to 8 elements; part p owns the elements [p * L, min(n, (p + 1) * L)) (parts past the
//           end are empty and store 0). P and L depend on n alone -- not on the dtype, the device or the grid -- and with a
//           16-byte aligned base every boundary is a 16-byte address.
//   loads   a part's first elements up to the next 16-byte address and its last ones behind the last whole vector are read
//           as scalars (one element per thread), everything between as 16-byte vectors, thread t taking vectors t, t + 256,
//           ...; four vectors are loaded before the first is used (64 B in flight per lane, 16 KiB per workgroup). Plain
//           loads, not non-temporal ones: the AdamW pass that follows reads the same gradient again.
//   sums    every element is widened to fp64 FIRST and squared there: a 24-bit significand squared is exact in fp64, so the
//           only roundings are the fp64 additions (a square formed in fp32 loses up to 2^-20 of its value once it falls
//           below 2^-126, and overflows above 2^64: both are gradients a diverging run produces). Four accumulators per lane,
//           one per vector in flight, merged as (a0 + a1) + (a2 + a3); lanes through wave_sum_dpp_f64 (common.h), the four
//           waves through four LDS entries as (w0 + w1) + (w2 + w3); one fp64 partial per part.
//   order   nothing depends on which workgroup runs first: no atomics, no arrival counter. The partials are a fixed function
//           of (contents, n, address mod 16).
// Stage 2, uamd_grad_clip_coef: ONE wave adds any number of partial arrays (lane l takes entries l, l + 64, ... of each
//   array in turn, ascending; lanes merge as above) and forms torch's clip_grad_norm_ factor, see the kernel.
#include "common.h"

namespace {

#define UAMD_GN_THREADS 256
#define UAMD_GN_INFLIGHT 4                     // 16-byte vectors a lane loads before it uses the first
#define UAMD_GN_PART_MIN 8192                  // elements: below this a part is not worth a workgroup of its own
#define UAMD_GN_PART_CAP (256 * 4)             // 4 workgroups on each of an MI355X's 256 CUs; a constant, P must not vary by device

template <typename T>
__device__ __forceinline__ double add_sq(double acc, T x) {
    const double d = (double)to_f32(x);
    return __builtin_fma(d, d, acc);           // d * d is exact: the same bits as acc + d * d, one instruction
}

template <typename T>
__global__ void __launch_bounds__(UAMD_GN_THREADS) grad_sumsq_kernel(const T* __restrict__ g, int64_t n, int64_t part_len,
                                                                     double* __restrict__ partials) {
    constexpr int E = Vec16<T>::N;
    const int t = threadIdx.x;
    const int64_t lo_ = (int64_t)blockIdx.x * part_len, lo = lo_ < n ? lo_ : n;
    const int64_t hi = lo + part_len < n ? lo + part_len : n;
    const int64_t len = hi - lo;
    const T* base = g + lo;
    int64_t head = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(base) & 15)) & 15) / sizeof(T));
    if (head > len) head = len;
    const int64_t nv = (len - head) / E;       // whole 16-byte vectors
    const int64_t tail0 = head + nv * E;
    const T* vb = base + head;
    double acc[UAMD_GN_INFLIGHT] = {0.0, 0.0, 0.0, 0.0};
    if (t < head) acc[0] = add_sq(acc[0], base[t]);
    int64_t i = t;
    for (; i + (UAMD_GN_INFLIGHT - 1) * UAMD_GN_THREADS < nv; i += UAMD_GN_INFLIGHT * UAMD_GN_THREADS) {
        Vec16<T> v[UAMD_GN_INFLIGHT];
#pragma unroll
        for (int u = 0; u < UAMD_GN_INFLIGHT; ++u) v[u] = ld16(vb + (i + u * UAMD_GN_THREADS) * E);
#pragma unroll
        for (int u = 0; u < UAMD_GN_INFLIGHT; ++u)
#pragma unroll
            for (int j = 0; j < E; ++j) acc[u] = add_sq(acc[u], v[u].e[j]);
    }
    for (; i < nv; i += UAMD_GN_THREADS) {     // fewer than four vectors left for this lane
        const Vec16<T> v = ld16(vb + i * E);
#pragma unroll
        for (int j = 0; j < E; ++j) acc[0] = add_sq(acc[0], v.e[j]);
    }
    if (t < len - tail0) acc[1] = add_sq(acc[1], base[tail0 + t]);
    const double s = wave_sum_dpp_f64((acc[0] + acc[1]) + (acc[2] + acc[3]));
    __shared__ double red[UAMD_GN_THREADS / UAMD_WAVE];
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

#define UAMD_GN_MAX_ARRAYS 64
struct ClipArrays {
    const double* ptr[UAMD_GN_MAX_ARRAYS];
    int count[UAMD_GN_MAX_ARRAYS];
    int n;
};

// torch.nn.utils.clip_grad_norm_ (error_if_nonfinite = False): total_norm is an fp32 tensor there and the factor is formed
// from it, so here too: norm = fp32(sqrt(sumsq)), the fp64 root rounded once; coef = fp32(min(1, max_norm / (norm + 1e-6)))
// in fp64 FROM THE STORED norm, rounded once -- a caller that reads `norm` can reproduce `coef` bit for bit. The clamp is
// `c > 1 ? 1 : c`, not fmin: a NaN norm gives a NaN factor (torch.clamp keeps NaN), an infinite one gives 0.
__global__ void __launch_bounds__(UAMD_WAVE) grad_clip_coef_kernel(ClipArrays A, double max_norm, double* __restrict__ sumsq_out,
                                                                   float* __restrict__ norm_coef) {
    const int lane = threadIdx.x;
    double acc = 0.0;
    for (int a = 0; a < A.n; ++a) {
        const double* p = A.ptr[a];
        const int cnt = A.count[a];
        for (int j = lane; j < cnt; j += UAMD_WAVE) acc += p[j];
    }
    const double s = wave_sum_dpp_f64(acc);
    if (lane == 0) {
        if (sumsq_out) *sumsq_out = s;
        if (norm_coef) {
            const float norm = (float)sqrt(s);
            double c = max_norm / ((double)norm + 1e-6);
            if (c > 1.0) c = 1.0;
            norm_coef[0] = norm;
            norm_coef[1] = (float)c;
        }
    }
}

}  // namespace

extern "C" int uamd_grad_sumsq_parts(int64_t n) {
    int64_t p = (n + UAMD_GN_PART_MIN - 1) / UAMD_GN_PART_MIN;
    if (p > UAMD_GN_PART_CAP) p = UAMD_GN_PART_CAP;
    return (int)(p < 1 ? 1 : p);
}

extern "C" int uamd_grad_sumsq(const void* g, int64_t n, int dtype, double* partials, void* stream) {
    if (!partials || n < 0 || (!g && n > 0)) return UAMD_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(partials) & 7) return UAMD_ERR_ALIGN;
    const int P = uamd_grad_sumsq_parts(n);
    const int64_t part_len = ((n + P - 1) / P + 7) / 8 * 8;
    hipStream_t st = (hipStream_t)stream;
    UAMD_DISPATCH_FLOAT(dtype,
        if (reinterpret_cast<uintptr_t>(g) % sizeof(T)) return UAMD_ERR_ALIGN;
        hipLaunchKernelGGL((grad_sumsq_kernel<T>), dim3((unsigned)P), dim3(UAMD_GN_THREADS), 0, st, (const T*)g, n, part_len, partials))
    return uamd_launch_status();
}

extern "C" int uamd_grad_clip_coef(const double* const* arrays, const int* counts, int n_arrays, double max_norm,
                                   double* sumsq_out, float* norm_coef, void* stream) {
    if (!arrays || !counts || n_arrays < 1 || n_arrays > UAMD_GN_MAX_ARRAYS || (!sumsq_out && !norm_coef)) return UAMD_ERR_ARG;
    ClipArrays A;
    A.n = n_arrays;
    for (int a = 0; a < n_arrays; ++a) {
        if (!arrays[a] || counts[a] < 0) return UAMD_ERR_ARG;
        if (reinterpret_cast<uintptr_t>(arrays[a]) & 7) return UAMD_ERR_ALIGN;
        A.ptr[a] = arrays[a];
        A.count[a] = counts[a];
    }
    if ((reinterpret_cast<uintptr_t>(sumsq_out) & 7) || (reinterpret_cast<uintptr_t>(norm_coef) & 3)) return UAMD_ERR_ALIGN;
    hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(UAMD_WAVE), 0, (hipStream_t)stream, A, max_norm, sumsq_out, norm_coef);
    return uamd_launch_status();
}
