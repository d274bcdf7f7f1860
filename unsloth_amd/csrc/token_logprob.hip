// Log-probability and entropy of the token a decode step chose, from the step's own fp32 logits (the reference gets them from a
// second, teacher-forced forward over prompt + completion: get_per_token_logps_and_entropies; a serving engine returns them as
// `logprobs` beside the tokens). Per row b with z = logits[b] * (1 / temperature):
//   lp[b] = z[tok[b]] - logsumexp(z)          H[b] = logsumexp(z) - sum softmax(z) z
// over the WHOLE row: the temperature-scaled distribution before top-k / top-p / min-p, the one the teacher-forced forward scores.
//
// Two launches, nothing between them but the stream order (an arrival counter + fence pair in one launch is a 21 us tail on this
// device; two launches of this size are ~8 us):
//   part  grid (P, rows) x 256 threads. A row is cut into P <= 64 contiguous slices of at least 1024 logits (a multiple of 4, so
//         that every slice of a row starts at the row's own 16-byte phase); a workgroup streams its slice as 16-byte loads between
//         a scalar head and tail (a row may start at any 4-byte address). Each lane keeps the online triple of
//         cross_entropy_loss.hip -- m = max, s = sum exp(z - m), u = sum exp(z - m) (z - m), every term of u <= 0 -- and triples
//         merge by u <- e^(m - M) (u + (m - M) s), a side of weight 0 adding 0 (a -inf logit, an idle lane). Lanes merge on the
//         VALU (DPP, as lanes_sum), the four 16-lane rows of a wave through v_readlane, the four waves through 4 LDS entries;
//         thread 0 stores the slice's triple to ws[b][part]. No atomics, no fence, no counter.
//   final one 64-lane wave per row: lane p holds part p's triple, the same butterfly merges them -- a fixed order, whatever
//         order the parts ran in -- and lane 0 reads tok[b], that one logit, and stores lp and H at column *slot.
// The temperature (the sampler's DEVICE parameter block; NULL = 1) and the column (`slot`, DEVICE int32) are read by the kernels:
// a captured launch follows `sampling()` and writes to a moving column.
#include <math.h>

#include "common.h"

namespace {

constexpr int TLP_THREADS = 256, TLP_WAVES = TLP_THREADS / UAMD_WAVE;
constexpr int TLP_MAX_PARTS = 64, TLP_MAX_ROWS = 64, TLP_MIN_SPAN = 1024;

struct Tri { float m, s, u; };

__device__ __forceinline__ Tri tri_merge(Tri a, Tri b) {
    const float M = fmaxf(a.m, b.m);
    if (M == -INFINITY) return Tri{M, 0.f, 0.f};
    const float e1 = __expf(a.m - M), e2 = __expf(b.m - M);
    // a side whose weight is 0 adds nothing: for m_i == -inf the product (m_i - M) s_i would be -inf * 0
    const float ua = (e1 == 0.f) ? 0.f : e1 * (a.u + (a.m - M) * a.s);
    const float ub = (e2 == 0.f) ? 0.f : e2 * (b.u + (b.m - M) * b.s);
    return Tri{M, a.s * e1 + b.s * e2, ua + ub};
}

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ Tri tri_dpp_merge(Tri a) { return tri_merge(a, Tri{dpp_f32<CTRL>(a.m), dpp_f32<CTRL>(a.s), dpp_f32<CTRL>(a.u)}); }
__device__ __forceinline__ Tri tri_lane(Tri a, int lane) {
    return Tri{__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a.m), lane)),
               __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a.s), lane)),
               __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a.u), lane))};
}
// The triple of all 64 lanes, in every lane (all lanes must be active): the DPP steps of lanes_sum<16> leave each 16-lane row
// with its own result -- the merge is symmetric, so both lanes of a pair compute the same bits -- and the four rows merge in the
// order 0, 1, 2, 3.
__device__ __forceinline__ Tri tri_wave(Tri a) {
    a = tri_dpp_merge<0xb1>(a);       // quad_perm [1,0,3,2]
    a = tri_dpp_merge<0x4e>(a);       // quad_perm [2,3,0,1]
    a = tri_dpp_merge<0x141>(a);      // row_half_mirror
    a = tri_dpp_merge<0x140>(a);      // row_mirror
    Tri r = tri_lane(a, 0);
    r = tri_merge(r, tri_lane(a, 16));
    r = tri_merge(r, tri_lane(a, 32));
    return tri_merge(r, tri_lane(a, 48));
}

// 1 / temperature of the device block (anything but a positive temperature counts as 1, as in the sampler); NULL: 1
__device__ __forceinline__ float inv_temperature(const uamd_sample_params* prm) {
    if (!prm) return 1.f;
    const float T = prm->temperature;
    return (T > 0.f) ? 1.f / T : 1.f;
}

struct TlpArgs {
    const float* x;
    long long ld;
    int V, span;
    const uamd_sample_params* prm;
    float* ws;                        // [rows][TLP_MAX_PARTS][3]
};

// four scaled logits into a lane's triple: one rescale for the four (the vector step of the cross-entropy kernel)
__device__ __forceinline__ void absorb4(Tri& a, float t0, float t1, float t2, float t3) {
    const float t[4] = {t0, t1, t2, t3};
    const float M = fmaxf(a.m, fmaxf(fmaxf(t0, t1), fmaxf(t2, t3)));
    if (M == -INFINITY) return;
    const float e0 = __expf(a.m - M);
    float s = a.s * e0;
    float u = (e0 == 0.f) ? 0.f : e0 * (a.u + (a.m - M) * a.s);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float d = t[j] - M, e = __expf(d);
        s += e;
        u += (e == 0.f) ? 0.f : e * d;                    // z == -inf: 0, not 0 * -inf
    }
    a = Tri{M, s, u};
}

__global__ void __launch_bounds__(TLP_THREADS) token_logprob_part_kernel(TlpArgs a) {
    __shared__ Tri red[TLP_WAVES];
    const int tid = threadIdx.x, part = blockIdx.x, b = blockIdx.y;
    const float* row = a.x + (long long)b * a.ld;
    const float inv = inv_temperature(a.prm);
    const int lo = part * a.span, hi = min(a.V, lo + a.span);            // (the host: lo < V for every part of the grid)
    Tri acc = {-INFINITY, 0.f, 0.f};
    const int head = min(hi - lo, (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(row + lo) >> 2) & 3u)) & 3u));
    if (tid < head) acc = tri_merge(acc, Tri{row[lo + tid] * inv, 1.f, 0.f});
    const int vb = lo + head, nvec = (hi - vb) >> 2;
    const float4* v = reinterpret_cast<const float4*>(row + vb);
    int j = tid;
    for (; j + TLP_THREADS < nvec; j += 2 * TLP_THREADS) {               // both loads issued before either is consumed
        const float4 q0 = v[j], q1 = v[j + TLP_THREADS];
        absorb4(acc, q0.x * inv, q0.y * inv, q0.z * inv, q0.w * inv);
        absorb4(acc, q1.x * inv, q1.y * inv, q1.z * inv, q1.w * inv);
    }
    if (j < nvec) {
        const float4 q = v[j];
        absorb4(acc, q.x * inv, q.y * inv, q.z * inv, q.w * inv);
    }
    const int tb = vb + 4 * nvec;
    if (tid < hi - tb) acc = tri_merge(acc, Tri{row[tb + tid] * inv, 1.f, 0.f});
    acc = tri_wave(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        Tri r = red[0];
#pragma unroll
        for (int w = 1; w < TLP_WAVES; ++w) r = tri_merge(r, red[w]);
        float* o = a.ws + ((long long)b * TLP_MAX_PARTS + part) * 3;
        o[0] = r.m;
        o[1] = r.s;
        o[2] = r.u;
    }
}

__global__ void __launch_bounds__(UAMD_WAVE) token_logprob_final_kernel(TlpArgs a, int parts, const long long* __restrict__ tok,
                                                                        const int* __restrict__ slot, float* __restrict__ out_lp,
                                                                        float* __restrict__ out_ent, long long ld_out) {
    const int lane = threadIdx.x, b = blockIdx.x;
    Tri t = {-INFINITY, 0.f, 0.f};
    if (lane < parts) {
        const float* p = a.ws + ((long long)b * TLP_MAX_PARTS + lane) * 3;
        t = Tri{p[0], p[1], p[2]};
    }
    t = tri_wave(t);
    if (lane != 0) return;
    const long long col = *slot;
    if (col < 0 || col >= ld_out) return;                 // a column outside the row: nothing is stored
    const long long k = tok[b];
    const bool ok = k >= 0 && k < a.V;                    // a bad token: the read is clamped and the log-prob is NaN
    const float z = a.x[(long long)b * a.ld + (ok ? k : 0)] * inv_temperature(a.prm);
    // logsumexp(z) = m + ls. One lane per row: fp64 costs nothing here and leaves ONE rounding, the store's, behind the sums
    const double ls = log((double)t.s);
    out_lp[(long long)b * ld_out + col] = ok ? (float)(((double)z - (double)t.m) - ls) : NAN;
    if (out_ent) out_ent[(long long)b * ld_out + col] = (float)(ls - (double)t.u / (double)t.s);
}

}  // namespace

extern "C" int uamd_token_logprob_f32(const float* logits, int64_t ld, int rows, int V, const int64_t* tok,
                                      const uamd_sample_params* sparams, const int* slot, float* out_lp, float* out_ent,
                                      int64_t ld_out, float* ws, void* stream) {
    if (!logits || !tok || !slot || !out_lp || !ws || rows <= 0 || rows > TLP_MAX_ROWS || V <= 0 || V > (1 << 30) || (ld != 0 && ld < V) ||
        ld_out <= 0)
        return UAMD_ERR_ARG;
    // P = min(64, ceil(V / 1024)) slices of `span` logits, span a multiple of 4; the last slice may be short, none is empty
    const int fit = (V - 1) / TLP_MIN_SPAN + 1, want = fit < TLP_MAX_PARTS ? fit : TLP_MAX_PARTS;
    const int span = (((V + want - 1) / want) + 3) & ~3;
    const int parts = (V + span - 1) / span;
    TlpArgs a;
    a.x = logits;
    a.ld = (long long)ld;
    a.V = V;
    a.span = span;
    a.prm = sparams;
    a.ws = ws;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(token_logprob_part_kernel, dim3((unsigned)parts, (unsigned)rows), dim3(TLP_THREADS), 0, st, a);
    hipLaunchKernelGGL(token_logprob_final_kernel, dim3((unsigned)rows), dim3(UAMD_WAVE), 0, st, a, parts, (const long long*)tok, slot,
                       out_lp, out_ent, (long long)ld_out);
    return uamd_launch_status();
}
