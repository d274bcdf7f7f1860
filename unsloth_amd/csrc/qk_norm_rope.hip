// Per-head RMSNorm of q and k (Qwen3's q_norm / k_norm, one weight of D each) fused with the RoPE rotation, in place on the
// strided q|k views the q|k|v GEMM wrote; forward, backward and the decode step's cache append.
//
// A row is one (token, head) vector of D = 64 or 128 elements. D / 8 lanes share a row (16 at D = 128: one DPP row; 8 at
// D = 64: half of one), so a wave holds 4 or 8 rows at once. Lane i of a row owns columns 4i .. 4i+3 and D/2 + 4i .. D/2 + 4i+3:
// two 8-byte accesses, and both halves of each of its four rotary pairs (j, j + D/2) are lane-local. The sum of squares
// crosses the row's lanes by DPP (lanes_sum, common.h): no LDS, no barrier.
//
// Training kernels: a lane group takes ONE token and walks a chunk of HPC heads of it, so the token's cos / sin columns and
// both norm weights are loaded once per chunk; the wave's 4 (8) groups are 4 (8) consecutive tokens. Grid (token block, head
// chunk): 256 threads = 16 (32) tokens x 8 heads = 128 (256) rows per workgroup, 2560 workgroups at 8192 tokens x 40 heads.
// Loads of UNR heads are issued before the first of them is used.
//
// Rounding points of the forward = transformers' Qwen3RMSNorm followed by apply_rotary_pos_emb in a 16-bit dtype:
//   r = rsqrt(mean(x^2) + eps) in fp32; y = rn(x r); z = rn(y w); out = rope_pair(z) (each product and the sum rounded).
// The backward works in fp32 and rounds once at the store.
#include "common.h"

namespace {

template <typename T> struct Vec8 {
    union { uint2 raw; T e[4]; };
    __device__ __forceinline__ Vec8() {}
};

// the lane's 8 columns of the row at p (first its 4 of the lower half, then its 4 of the upper half)
template <typename T, int D>
__device__ __forceinline__ void load_cols(const T* p, int li, float* x) {
    Vec8<T> lo, hi;
    lo.raw = *reinterpret_cast<const uint2*>(p + 4 * li);
    hi.raw = *reinterpret_cast<const uint2*>(p + D / 2 + 4 * li);
#pragma unroll
    for (int j = 0; j < 4; ++j) { x[j] = to_f32(lo.e[j]); x[j + 4] = to_f32(hi.e[j]); }
}
template <typename T, int D>
__device__ __forceinline__ void store_cols(T* p, int li, const T* o) {
    Vec8<T> lo, hi;
#pragma unroll
    for (int j = 0; j < 4; ++j) { lo.e[j] = o[j]; hi.e[j] = o[j + 4]; }
    *reinterpret_cast<uint2*>(p + 4 * li) = lo.raw;
    *reinterpret_cast<uint2*>(p + D / 2 + 4 * li) = hi.raw;
}

// THE forward of one row, shared by the training kernel and the decode append: the same statements on the same inputs, so a
// token's key has the same bits whichever of the two wrote it. Every lane of the wave must be active (DPP). Returns r.
template <typename T, int D>
__device__ __forceinline__ float norm_rope_row(const float* x, const float* w, const float* c, const float* s, float eps, T* o) {
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += x[j] * x[j];
    ss = lanes_sum<D / 8>(ss);
    const float r = rsqrtf(ss * (1.0f / D) + eps);
    float z[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = round_to<T>(round_to<T>(x[j] * r) * w[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) rope_pair(z[j], z[j + 4], c[j], s[j], o[j], o[j + 4]);
    return r;
}

struct QkNormArgs {
    void* Q; int64_t q_bs, q_hs, q_ss;
    void* K; int64_t k_bs, k_hs, k_ss;
    const void* wq; const void* wk;
    const void* cos; int64_t cos_rs;
    const void* sin; int64_t sin_rs;
    const int32_t* idx;
    float* r;               // [n_tok, Hq + Hk]: written by the forward (NULL: not kept), read by the backward
    void* x_save;           // [n_tok, Hq + Hk, D] contiguous: the pre-norm rows, written by the forward (NULL: not kept), read by the backward
    int64_t n_tok;
    int seqlen, Hq, Hk;
    float eps;
};

constexpr int HPC = 8;      // heads per chunk (grid.y)
constexpr int UNR = 4;      // rows in flight per lane

// what a lane group needs of its token: the row pointers' token part, the table columns, both weights
template <typename T, int D>
struct TokenCtx {
    int64_t tok, b, t;
    bool live;
    int li;
    float c[4], s[4], wq[8], wk[8];
    __device__ __forceinline__ TokenCtx(const QkNormArgs& a) {
        constexpr int LPR = D / 8;
        li = threadIdx.x % LPR;
        tok = (int64_t)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
        live = tok < a.n_tok;
        if (!live) tok = a.n_tok - 1;       // every lane stays in the DPP sums; a group past the end stores nothing
        const int64_t pos = a.idx ? (int64_t)a.idx[tok] : tok % a.seqlen;
        load_w<T, 4>((const T*)a.cos + pos * a.cos_rs + 4 * li, c);
        load_w<T, 4>((const T*)a.sin + pos * a.sin_rs + 4 * li, s);
        load_cols<T, D>((const T*)a.wq, li, wq);
        load_cols<T, D>((const T*)a.wk, li, wk);
        b = tok / a.seqlen;
        t = tok - b * a.seqlen;
    }
    __device__ __forceinline__ T* row(const QkNormArgs& a, int h) const {
        return h < a.Hq ? (T*)a.Q + b * a.q_bs + (int64_t)h * a.q_hs + t * a.q_ss
                        : (T*)a.K + b * a.k_bs + (int64_t)(h - a.Hq) * a.k_hs + t * a.k_ss;
    }
};

template <typename T, int D>
__global__ void __launch_bounds__(256) qk_norm_rope_fwd_kernel(QkNormArgs a) {
    const TokenCtx<T, D> k(a);
    const int Htot = a.Hq + a.Hk;
    const int h0 = blockIdx.y * HPC, h1 = min(h0 + HPC, Htot);
    for (int hb = h0; hb < h1; hb += UNR) {
        float x[UNR][8];
#pragma unroll
        for (int u = 0; u < UNR; ++u) load_cols<T, D>(k.row(a, min(hb + u, h1 - 1)), k.li, x[u]);
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int h = hb + u;            // (wave-uniform; past the chunk: the last row again, computed and dropped)
            T o[8];
            const float r = norm_rope_row<T, D>(x[u], min(h, h1 - 1) < a.Hq ? k.wq : k.wk, k.c, k.s, a.eps, o);
            if (h < h1 && k.live) {
                store_cols<T, D>(k.row(a, h), k.li, o);
                const int64_t ri = k.tok * Htot + h;
                if (a.r && k.li == 0) a.r[ri] = r;
                if (a.x_save) {
                    T raw[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) raw[j] = from_f32<T>(x[u][j]);       // (exact: x came from T)
                    store_cols<T, D>((T*)a.x_save + ri * D, k.li, raw);
                }
            }
        }
    }
}

// dQ', dK' (gradients of the rotated outputs, in place) -> gradients of the pre-norm rows:
//   g = R(-pos) g'                              (the rotation with -sin)
//   dx = r (w g - xh mean(w g xh)),  xh = x r   (the RMSNorm input gradient; the norm weights are frozen)
template <typename T, int D>
__global__ void __launch_bounds__(256) qk_norm_rope_bwd_kernel(QkNormArgs a) {
    const TokenCtx<T, D> k(a);
    const int Htot = a.Hq + a.Hk;
    const int h0 = blockIdx.y * HPC, h1 = min(h0 + HPC, Htot);
    for (int hb = h0; hb < h1; hb += UNR) {
        float gp[UNR][8], x[UNR][8], rr[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int h = min(hb + u, h1 - 1);
            const int64_t ri = k.tok * Htot + h;
            load_cols<T, D>(k.row(a, h), k.li, gp[u]);
            load_cols<T, D>((const T*)a.x_save + ri * D, k.li, x[u]);
            rr[u] = a.r[ri];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int h = hb + u;
            const float* w = min(h, h1 - 1) < a.Hq ? k.wq : k.wk;
            float wg[8], xh[8], dot = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                wg[j] = w[j] * (gp[u][j] * k.c[j] + gp[u][j + 4] * k.s[j]);
                wg[j + 4] = w[j + 4] * (gp[u][j + 4] * k.c[j] - gp[u][j] * k.s[j]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) { xh[j] = x[u][j] * rr[u]; dot += wg[j] * xh[j]; }
            const float m = lanes_sum<D / 8>(dot) * (1.0f / D);
            T o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = from_f32<T>(rr[u] * (wg[j] - xh[j] * m));
            if (h < h1 && k.live) store_cols<T, D>(k.row(a, h), k.li, o);
        }
    }
}

// The decode step: uamd_rope_kv_append's contract with the per-head norm in front of the rotation. One wave per workgroup;
// workgroups [0, nqk) take 64 / (D / 8) consecutive q / k heads of row b each (norm_rope_row: the training kernel's bits),
// the workgroups behind them copy one v head each to the cache.
template <typename T, int D>
__global__ void __launch_bounds__(64) qk_norm_rope_append_kernel(T* __restrict__ qkv, int64_t ld_qkv, const T* __restrict__ wq,
                                                                  const T* __restrict__ wk, float eps, const T* __restrict__ cos_t,
                                                                  const T* __restrict__ sin_t, int64_t ld_cs,
                                                                  const int* __restrict__ kv_len, const int* __restrict__ rope_pos,
                                                                  T* __restrict__ kc, T* __restrict__ vc, int64_t c_sb, int64_t c_sh,
                                                                  int Hq, int Hk, int s_max, int nqk) {
    constexpr int LPR = D / 8, RPW = 64 / LPR;
    const int b = blockIdx.y;
    const int len = kv_len[b];
    if ((int)blockIdx.x >= nqk) {
        const int hv = blockIdx.x - nqk;
        if (len < s_max) {
            const T* v = qkv + (int64_t)b * ld_qkv + (int64_t)(Hq + Hk + hv) * D;
            T* vd = vc + (int64_t)b * c_sb + (int64_t)hv * c_sh + (int64_t)len * D;
            for (int j = threadIdx.x; j < D; j += 64) vd[j] = v[j];
        }
        return;
    }
    const int li = threadIdx.x % LPR;
    int h = blockIdx.x * RPW + threadIdx.x / LPR;
    const bool live = h < Hq + Hk;
    if (!live) h = Hq + Hk - 1;
    const int64_t pos = rope_pos ? rope_pos[b] : len;
    float c[4], s[4], w[8], x[8];
    load_w<T, 4>(cos_t + pos * ld_cs + 4 * li, c);
    load_w<T, 4>(sin_t + pos * ld_cs + 4 * li, s);
    load_cols<T, D>(h < Hq ? wq : wk, li, w);
    T* p = qkv + (int64_t)b * ld_qkv + (int64_t)h * D;
    load_cols<T, D>(p, li, x);
    T o[8];
    norm_rope_row<T, D>(x, w, c, s, eps, o);
    if (!live) return;
    store_cols<T, D>(p, li, o);
    if (h >= Hq && len < s_max) store_cols<T, D>(kc + (int64_t)b * c_sb + (int64_t)(h - Hq) * c_sh + (int64_t)len * D, li, o);
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

int check(const QkNormArgs& a, int D) {
    if (!a.Q || !a.K || !a.wq || !a.wk || !a.cos || !a.sin || a.Hq <= 0 || a.Hk <= 0 || a.seqlen <= 0) return UAMD_ERR_ARG;
    if (D != 64 && D != 128) return UAMD_ERR_ARG;
    if (a.n_tok < 0 || a.n_tok > 0x7fffffffLL) return UAMD_ERR_ARG;
    const int64_t strides[] = {a.q_bs, a.q_hs, a.q_ss, a.k_bs, a.k_hs, a.k_ss, a.cos_rs, a.sin_rs};
    for (int64_t s : strides)
        if (s & 3) return UAMD_ERR_ALIGN;
    if (!aligned8(a.Q) || !aligned8(a.K) || !aligned8(a.wq) || !aligned8(a.wk) || !aligned8(a.cos) || !aligned8(a.sin) ||
        !aligned8(a.x_save))
        return UAMD_ERR_ALIGN;
    return UAMD_OK;
}

template <typename T, int D>
int launch(const QkNormArgs& a, bool backward, hipStream_t st) {
    constexpr int TPB = 256 / (D / 8);          // tokens per workgroup
    dim3 grid((unsigned)((a.n_tok + TPB - 1) / TPB), (unsigned)((a.Hq + a.Hk + HPC - 1) / HPC));
    if (backward) hipLaunchKernelGGL((qk_norm_rope_bwd_kernel<T, D>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((qk_norm_rope_fwd_kernel<T, D>), grid, dim3(256), 0, st, a);
    return uamd_launch_status();
}

int dispatch(const QkNormArgs& a, int D, int dtype, bool backward, void* stream) {
    if (int rc = check(a, D)) return rc;
    if (a.n_tok == 0) return UAMD_OK;
    hipStream_t st = (hipStream_t)stream;
    UAMD_DISPATCH_HALF(dtype, return D == 128 ? launch<T, 128>(a, backward, st) : launch<T, 64>(a, backward, st))
    return UAMD_ERR_DTYPE;
}

}  // namespace

extern "C" int uamd_qk_norm_rope_fwd(void* Q, int64_t q_batch_stride, int64_t q_head_stride, int64_t q_seq_stride, void* K,
                                     int64_t k_batch_stride, int64_t k_head_stride, int64_t k_seq_stride, const void* q_weight,
                                     const void* k_weight, float eps, const void* cos, int64_t cos_row_stride, const void* sin,
                                     int64_t sin_row_stride, const int32_t* rope_indices, float* r, void* x_save, int batch,
                                     int seqlen, int n_heads_q, int n_heads_k, int head_dim, int dtype, void* stream) {
    QkNormArgs a;
    a.Q = Q; a.q_bs = q_batch_stride; a.q_hs = q_head_stride; a.q_ss = q_seq_stride;
    a.K = K; a.k_bs = k_batch_stride; a.k_hs = k_head_stride; a.k_ss = k_seq_stride;
    a.wq = q_weight; a.wk = k_weight; a.cos = cos; a.cos_rs = cos_row_stride; a.sin = sin; a.sin_rs = sin_row_stride;
    a.idx = rope_indices; a.r = r; a.x_save = x_save; a.n_tok = (int64_t)batch * seqlen; a.seqlen = seqlen;
    a.Hq = n_heads_q; a.Hk = n_heads_k; a.eps = eps;
    return dispatch(a, head_dim, dtype, false, stream);
}

extern "C" int uamd_qk_norm_rope_bwd(void* dQ, int64_t q_batch_stride, int64_t q_head_stride, int64_t q_seq_stride, void* dK,
                                     int64_t k_batch_stride, int64_t k_head_stride, int64_t k_seq_stride, const void* q_weight,
                                     const void* k_weight, const void* cos, int64_t cos_row_stride, const void* sin,
                                     int64_t sin_row_stride, const int32_t* rope_indices, const float* r, const void* x_saved,
                                     int batch, int seqlen, int n_heads_q, int n_heads_k, int head_dim, int dtype, void* stream) {
    if (!r || !x_saved) return UAMD_ERR_ARG;
    QkNormArgs a;
    a.Q = dQ; a.q_bs = q_batch_stride; a.q_hs = q_head_stride; a.q_ss = q_seq_stride;
    a.K = dK; a.k_bs = k_batch_stride; a.k_hs = k_head_stride; a.k_ss = k_seq_stride;
    a.wq = q_weight; a.wk = k_weight; a.cos = cos; a.cos_rs = cos_row_stride; a.sin = sin; a.sin_rs = sin_row_stride;
    a.idx = rope_indices; a.r = const_cast<float*>(r); a.x_save = const_cast<void*>(x_saved);
    a.n_tok = (int64_t)batch * seqlen; a.seqlen = seqlen; a.Hq = n_heads_q; a.Hk = n_heads_k; a.eps = 0.f;
    return dispatch(a, head_dim, dtype, true, stream);
}

extern "C" int uamd_qk_norm_rope_kv_append(void* qkv, int64_t ld_qkv, const void* q_weight, const void* k_weight, float eps,
                                           const void* cos_t, const void* sin_t, int64_t ld_cs, const int* kv_len,
                                           const int* rope_pos, void* k_cache, void* v_cache, int64_t cache_sb, int64_t cache_sh,
                                           int B, int Hq, int Hk, int D, int s_max, int dtype, void* stream) {
    if (!qkv || !q_weight || !k_weight || !cos_t || !sin_t || !kv_len || !k_cache || !v_cache || B <= 0 || Hq <= 0 || Hk <= 0 ||
        (D != 64 && D != 128))
        return UAMD_ERR_ARG;
    if ((ld_qkv & 3) || (ld_cs & 3) || (cache_sb & 3) || (cache_sh & 3) || !aligned8(qkv) || !aligned8(q_weight) ||
        !aligned8(k_weight) || !aligned8(cos_t) || !aligned8(sin_t) || !aligned8(k_cache))
        return UAMD_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int rpw = 64 / (D / 8), nqk = (Hq + Hk + rpw - 1) / rpw;
    const dim3 grid(nqk + Hk, B);
#define UAMD_APPEND(DD)                                                                                                        \
    hipLaunchKernelGGL((qk_norm_rope_append_kernel<T, DD>), grid, dim3(64), 0, st, (T*)qkv, ld_qkv, (const T*)q_weight,        \
                       (const T*)k_weight, eps, (const T*)cos_t, (const T*)sin_t, ld_cs, kv_len, rope_pos, (T*)k_cache,        \
                       (T*)v_cache, cache_sb, cache_sh, Hq, Hk, s_max, nqk)
    UAMD_DISPATCH_HALF(dtype, if (D == 128) UAMD_APPEND(128); else UAMD_APPEND(64))
#undef UAMD_APPEND
    return uamd_launch_status();
}
