// RMSNorm forward / backward for gfx950.
//
// Replaces the Triton kernels of the reference:
//   unsloth/kernels/rms_layernorm.py:21-59   _rms_layernorm_forward
//   unsloth/kernels/rms_layernorm.py:62-120  _rms_layernorm_backward
//   unsloth/kernels/rms_layernorm.py:123-159 _gemma_rms_layernorm_forward
//
// HBM-bound. The whole row lives in registers as 16-byte vectors (single HBM read, all loads issued before the first
// use), shared by TPR threads of a 256-thread block; UAMD_TUNE_RMS_VAR picks TPR:
//   1 (the default)  TPR = 256, one row per BLOCK: ITERS = n_cols / 2048 vectors per thread for 16-bit data (2 at hidden
//                    4096) and ONE LDS reduction. Few registers per thread -> 8 blocks per CU resident and several passes
//                    of blocks per launch, so the loads of one block overlap the stores of another.
//   0                TPR = 64, one row per WAVE, 4 rows per block: the reduction is a 6-step wave64 xor-shuffle, no LDS,
//                    no barrier, but all 8192 rows of a launch sit on the chip at once: one read phase, then one write
//                    phase. Kept for the parity tests of the two forms.
// The two forms sum a row in different (each fixed, run-to-run deterministic) orders; r is compared against the oracle
// with a tolerance. Rows that do not fit the register budget (or are not 16-byte aligned) take the generic block-per-row
// two-pass kernel.
#include "common.h"

namespace {

// ADD: the residual add in front of the norm is fused in -- h = T(x + res) (one rounding, what `residual + x`
// gives in torch), h is written to Hout (the next residual) and normalised (llama.py:823-844 does add, then norm,
// as two passes over the activations).
template <typename T, typename WT, int TPR, int ITERS, bool GEMMA, bool ADD>
__global__ void __launch_bounds__(256)
rms_fwd_rows(const T* __restrict__ X, const WT* __restrict__ W, T* __restrict__ Y,
             float* __restrict__ R, int64_t n_rows, int n_cols, int64_t xs, int64_t ys, float eps, int mode,
             const T* __restrict__ Res, T* __restrict__ Hout, int64_t rs, int64_t hs) {
    constexpr int VEC = Vec16<T>::N;
    __shared__ float red[TPR / 64];
    const unsigned t = TPR == 64 ? threadIdx.x & 63 : threadIdx.x;
    const int64_t row = TPR == 64 ? (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) : blockIdx.x;
    if (TPR == 64 && row >= n_rows) return;
    const T* x = X + row * xs;
    Vec16<T> xv[ITERS];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
        const int c = (t + TPR * i) * VEC;
        if (c < n_cols) xv[i] = ld16_m(x + c, mode);
        else xv[i].raw = make_uint4(0, 0, 0, 0);
    }
    if (ADD) {
        const T* res = Res + row * rs;
        T* h = Hout + row * hs;
        Vec16<T> rv[ITERS];
#pragma unroll
        for (int i = 0; i < ITERS; ++i) {
            const int c = (t + TPR * i) * VEC;
            if (c < n_cols) rv[i] = ld16_m(res + c, mode);
            else rv[i].raw = make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < ITERS; ++i) {
            const int c = (t + TPR * i) * VEC;
#pragma unroll
            for (int j = 0; j < VEC; ++j) xv[i].e[j] = from_f32<T>(to_f32(xv[i].e[j]) + to_f32(rv[i].e[j]));
            if (c < n_cols) st16(h + c, xv[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < ITERS; ++i)
#pragma unroll
        for (int j = 0; j < VEC; ++j) { float f = to_f32(xv[i].e[j]); ss += f * f; }
    ss = row_sum<TPR>(ss, red);
    const float inv = rsqrtf(ss / (float)n_cols + eps);
    if (t == 0) R[row] = inv;
    T* y = Y + row * ys;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
        const int c = (t + TPR * i) * VEC;
        if (c < n_cols) {
            Vec16<T> o;
            float wf[VEC];
            load_w<WT, VEC>(W + c, wf);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float normed = to_f32(xv[i].e[j]) * inv;
                if (GEMMA) {
                    o.e[j] = from_f32<T>(normed * (wf[j] + 1.0f));
                } else {
                    // rms_layernorm.py:56-58: normed.to(W.dtype) * W, product in W's dtype
                    o.e[j] = from_f32<T>(round_to<WT>(round_to<WT>(normed) * wf[j]));
                }
            }
            st16_m(y + c, o, mode);
        }
    }
}

// ADD: dX = T(T(rms_dx) + dRes): the gradient that reaches h = x + res from the residual path is added here
// instead of by a separate autograd accumulation pass (same two roundings as that pass).
template <typename T, typename WT, int TPR, int ITERS, bool GEMMA, bool ADD>
__global__ void __launch_bounds__(256)
rms_bwd_rows(const T* dY, T* dX, const T* __restrict__ X,
             const WT* __restrict__ W, const float* __restrict__ R, int64_t n_rows, int n_cols,
             int64_t dys, int64_t dxs, int64_t xs, int mode, const T* dRes, int64_t drs) {
    constexpr int VEC = Vec16<T>::N;
    // a row over a block leaves the registers to keep W (Gemma's +1 applied) and dRes from the first pass; over a wave
    // (4x the vectors per thread) the second pass loads them: the other choice changes either form's occupancy
    constexpr bool KEEP = TPR > 64;
    __shared__ float red[TPR / 64];
    const unsigned t = TPR == 64 ? threadIdx.x & 63 : threadIdx.x;
    const int64_t row = TPR == 64 ? (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) : blockIdx.x;
    if (TPR == 64 && row >= n_rows) return;
    const T* dy = dY + row * dys;
    const T* x = X + row * xs;
    Vec16<T> dv[ITERS], xv[ITERS], rv[KEEP && ADD ? ITERS : 1];
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
        const int c = (t + TPR * i) * VEC;
        if (c < n_cols) {
            dv[i] = ld16_m(dy + c, mode); xv[i] = ld16_m(x + c, mode);
            if (KEEP && ADD) rv[i] = ld16_m(dRes + row * drs + c, mode);
        } else { dv[i].raw = make_uint4(0, 0, 0, 0); xv[i].raw = make_uint4(0, 0, 0, 0); }
    }
    const float inv = R[row];
    float wf[KEEP ? ITERS : 1][VEC];
    float rsum = 0.f;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
        const int c = (t + TPR * i) * VEC;
        if (c < n_cols) {
            float* w = wf[KEEP ? i : 0];
            load_w<WT, VEC>(W + c, w);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                if (GEMMA) w[j] += 1.0f;
                rsum += to_f32(dv[i].e[j]) * w[j] * (to_f32(xv[i].e[j]) * inv);
            }
        }
    }
    rsum = row_sum<TPR>(rsum, red);
    const float n = (float)n_cols;
    T* dx = dX + row * dxs;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
        const int c = (t + TPR * i) * VEC;
        if (c < n_cols) {
            Vec16<T> o;
            float* w = wf[KEEP ? i : 0];
            if (!KEEP) load_w<WT, VEC>(W + c, w);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                if (GEMMA && !KEEP) w[j] += 1.0f;
                const float dyw = to_f32(dv[i].e[j]) * w[j];
                const float normed = to_f32(xv[i].e[j]) * inv;
                // rms_layernorm.py:112
                o.e[j] = from_f32<T>(inv / n * (n * dyw - normed * rsum));
            }
            if (ADD) {
                if (!KEEP) rv[0] = ld16_m(dRes + row * drs + c, mode);
#pragma unroll
                for (int j = 0; j < VEC; ++j) o.e[j] = from_f32<T>(to_f32(o.e[j]) + to_f32(rv[KEEP ? i : 0].e[j]));
            }
            st16_m(dx + c, o, mode);
        }
    }
}

// Generic fallback: one 256-thread block per row, two passes (second pass hits L2).
template <typename T, typename WT, bool GEMMA>
__global__ void __launch_bounds__(256)
rms_fwd_block(const T* __restrict__ X, const WT* __restrict__ W, T* __restrict__ Y,
              float* __restrict__ R, int n_cols, int64_t xs, int64_t ys, float eps) {
    __shared__ float red[4];
    const int64_t row = blockIdx.x;
    const T* x = X + row * xs;
    float ss = 0.f;
    for (int c = threadIdx.x; c < n_cols; c += 256) { float f = to_f32(x[c]); ss += f * f; }
    ss = block_sum<4>(ss, red);
    const float inv = rsqrtf(ss / (float)n_cols + eps);
    if (threadIdx.x == 0) R[row] = inv;
    T* y = Y + row * ys;
    for (int c = threadIdx.x; c < n_cols; c += 256) {
        const float normed = to_f32(x[c]) * inv;
        if (GEMMA) y[c] = from_f32<T>(normed * (to_f32(W[c]) + 1.0f));
        else y[c] = from_f32<T>(round_to<WT>(round_to<WT>(normed) * to_f32(W[c])));
    }
}

template <typename T, typename WT, bool GEMMA>
__global__ void __launch_bounds__(256)
rms_bwd_block(const T* dY, T* dX, const T* __restrict__ X,
              const WT* __restrict__ W, const float* __restrict__ R, int n_cols, int64_t dys,
              int64_t dxs, int64_t xs) {
    __shared__ float red[4];
    const int64_t row = blockIdx.x;
    const T* dy = dY + row * dys;
    const T* x = X + row * xs;
    const float inv = R[row];
    float rs = 0.f;
    for (int c = threadIdx.x; c < n_cols; c += 256) {
        float w = to_f32(W[c]);
        if (GEMMA) w += 1.0f;
        rs += to_f32(dy[c]) * w * (to_f32(x[c]) * inv);
    }
    rs = block_sum<4>(rs, red);
    const float n = (float)n_cols;
    T* dx = dX + row * dxs;
    for (int c = threadIdx.x; c < n_cols; c += 256) {
        float w = to_f32(W[c]);
        if (GEMMA) w += 1.0f;
        const float dyw = to_f32(dy[c]) * w;  // same thread reads before it writes: alias-safe
        const float normed = to_f32(x[c]) * inv;
        dx[c] = from_f32<T>(inv / n * (n * dyw - normed * rs));
    }
}

// which vector form a launch takes (the row-block form's grid is one block per row: n_rows has to fit it). A row of
// `iters` vectors per lane of a wave is (iters + 3) / 4 per thread of a block.
static inline bool rms_row_per_block(int64_t n_rows) {
    return uamd_tuning_get(UAMD_TUNE_RMS_VAR) == 1 && n_rows <= 0x7fffffffLL;
}

// ADD: the fused residual add of uamd_add_rms_layernorm_fwd (Res, H and their row strides). It has no scalar form and no
// Gemma form: UAMD_ERR_ALIGN for what the vector kernels do not take, and the caller runs the two separate ops.
template <typename T, typename WT, bool GEMMA, bool ADD>
int launch_fwd(const void* X, const void* W, void* Y, float* R, int64_t n_rows, int n_cols, int64_t xs, int64_t ys,
               float eps, hipStream_t st, const void* Res, void* H, int64_t rs, int64_t hs) {
    static_assert(!(ADD && GEMMA), "the fused add has no Gemma form");
    constexpr int VEC = Vec16<T>::N;
    const bool vec_ok = (n_cols % VEC == 0) && (xs % VEC == 0) && (ys % VEC == 0) && aligned16(X) && aligned16(Y) &&
                        aligned16(W) && n_cols <= 64 * VEC * (ADD ? 8 : 16) &&
                        (!ADD || ((rs % VEC == 0) && (hs % VEC == 0) && aligned16(Res) && aligned16(H)));
    if (ADD && !vec_ok) return UAMD_ERR_ALIGN;
    const T* x = (const T*)X; const WT* w = (const WT*)W; T* y = (T*)Y;
    if (!vec_ok) {
        hipLaunchKernelGGL((rms_fwd_block<T, WT, GEMMA>), dim3((unsigned)n_rows), dim3(256), 0, st,
                           x, w, y, R, n_cols, xs, ys, eps);
        return uamd_launch_status();
    }
    const int iters = (n_cols + 64 * VEC - 1) / (64 * VEC);
    const int mode = uamd_tuning_get(UAMD_TUNE_STREAM_NT);
    auto launch = [&](auto tpr, auto it) {
        constexpr int TPR = decltype(tpr)::value;
        hipLaunchKernelGGL((rms_fwd_rows<T, WT, TPR, decltype(it)::value, GEMMA, ADD>),
                           dim3((unsigned)(TPR == 64 ? (n_rows + 3) / 4 : n_rows)), dim3(256), 0, st, x, w, y, R, n_rows,
                           n_cols, xs, ys, eps, mode, (const T*)Res, (T*)H, rs, hs);
    };
    auto block = [&](auto it) { launch(std::integral_constant<int, 256>{}, it); };
    auto wave = [&](auto it) { launch(std::integral_constant<int, 64>{}, it); };
    if (rms_row_per_block(n_rows)) {
        if constexpr (ADD) uamd_with_iters<1, 2>((iters + 3) / 4, block);
        else uamd_with_iters<1, 2, 4>((iters + 3) / 4, block);
    } else {
        if constexpr (ADD) uamd_with_iters<1, 2, 4, 8>(iters, wave);
        else uamd_with_iters<1, 2, 4, 8, 16>(iters, wave);
    }
    return uamd_launch_status();
}

// ADD: the fused dRes of uamd_add_rms_layernorm_bwd, under the same rule as the forward's.
template <typename T, typename WT, bool GEMMA, bool ADD>
int launch_bwd(const void* dY, void* dX, const void* X, const void* W, const float* R, int64_t n_rows, int n_cols,
               int64_t dys, int64_t dxs, int64_t xs, hipStream_t st, const void* dRes, int64_t drs) {
    static_assert(!(ADD && GEMMA), "the fused add has no Gemma form");
    constexpr int VEC = Vec16<T>::N;
    const bool vec_ok = (n_cols % VEC == 0) && (xs % VEC == 0) && (dys % VEC == 0) && (dxs % VEC == 0) && aligned16(X) &&
                        aligned16(dY) && aligned16(dX) && aligned16(W) && n_cols <= 64 * VEC * 8 &&
                        (!ADD || ((drs % VEC == 0) && aligned16(dRes)));
    if (ADD && !vec_ok) return UAMD_ERR_ALIGN;
    const T* dy = (const T*)dY; T* dx = (T*)dX; const T* x = (const T*)X; const WT* w = (const WT*)W;
    if (!vec_ok) {
        hipLaunchKernelGGL((rms_bwd_block<T, WT, GEMMA>), dim3((unsigned)n_rows), dim3(256), 0, st,
                           dy, dx, x, w, R, n_cols, dys, dxs, xs);
        return uamd_launch_status();
    }
    const int iters = (n_cols + 64 * VEC - 1) / (64 * VEC);
    const int mode = uamd_tuning_get(UAMD_TUNE_STREAM_NT);
    auto launch = [&](auto tpr, auto it) {
        constexpr int TPR = decltype(tpr)::value;
        hipLaunchKernelGGL((rms_bwd_rows<T, WT, TPR, decltype(it)::value, GEMMA, ADD>),
                           dim3((unsigned)(TPR == 64 ? (n_rows + 3) / 4 : n_rows)), dim3(256), 0, st, dy, dx, x, w, R,
                           n_rows, n_cols, dys, dxs, xs, mode, (const T*)dRes, drs);
    };
    if (rms_row_per_block(n_rows))
        uamd_with_iters<1, 2>((iters + 3) / 4, [&](auto it) { launch(std::integral_constant<int, 256>{}, it); });
    else
        uamd_with_iters<1, 2, 4, 8>(iters, [&](auto it) { launch(std::integral_constant<int, 64>{}, it); });
    return uamd_launch_status();
}

}  // namespace

// ---- weight gradient (full fine-tuning: the norm weights train; the reference's kernel returns no dW,
//      rms_layernorm.py:218-240, and leaves trainable norms to HF's torch RMSNorm + autograd):
//          dW[c] = sum_rows dY[row, c] * X[row, c] * r[row]          (Llama's w and Gemma's 1 + w alike)
// Column sums over all rows, HBM-bound (reads dY and X once). Two deterministic stages: (1) a grid of
// [column blocks] x [row chunks], thread = one 16-byte vector of columns, fp32 partial sums over the chunk's rows
// -> workspace[chunk][col]; (2) one thread per column adds the chunks in order. No atomics: bit-stable.
namespace {
// V: a thread owns one 16-byte vector of columns; !V (a width, a row stride or a pointer that is no multiple of 16 bytes): one
// column per thread, scalar loads, the same sums in the same order.
template <typename T, bool V>
__global__ void __launch_bounds__(256)
rms_dw_partial(const T* __restrict__ dY, const T* __restrict__ X, const float* __restrict__ R,
               float* __restrict__ part, int64_t n_rows, int n_cols, int64_t dys, int64_t xs, int rows_per_chunk) {
    constexpr int VEC = V ? Vec16<T>::N : 1;
    const int c = (blockIdx.x * 256 + threadIdx.x) * VEC;
    if (c >= n_cols) return;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
    const int64_t r1 = r0 + rows_per_chunk < n_rows ? r0 + rows_per_chunk : n_rows;
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
    for (int64_t row = r0; row < r1; ++row) {
        const float inv = R[row];
        if constexpr (V) {
            const Vec16<T> g = ld16(dY + row * dys + c);
            const Vec16<T> x = ld16(X + row * xs + c);
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[j] += to_f32(g.e[j]) * (to_f32(x.e[j]) * inv);
        } else {
            acc[0] += to_f32(dY[row * dys + c]) * (to_f32(X[row * xs + c]) * inv);
        }
    }
    float* out = part + (int64_t)blockIdx.y * n_cols + c;
#pragma unroll
    for (int j = 0; j < VEC; ++j) out[j] = acc[j];
}

template <typename WT>
__global__ void __launch_bounds__(256)
rms_dw_reduce(const float* __restrict__ part, WT* __restrict__ dW, int n_cols, int n_chunks, int accumulate) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cols) return;
    float s = 0.f;
    for (int k = 0; k < n_chunks; ++k) s += part[(int64_t)k * n_cols + c];
    if (accumulate) s += to_f32(dW[c]);
    dW[c] = from_f32<WT>(s);
}

template <typename T, typename WT>
int launch_dw(const void* dY, const void* X, const float* r, void* dW, float* ws, int64_t ws_elems, int64_t n_rows,
              int n_cols, int64_t dys, int64_t xs, int accumulate, hipStream_t st) {
    constexpr int VEC = Vec16<T>::N;
    const bool vec_ok = !((n_cols % VEC) || (dys % VEC) || (xs % VEC) || !aligned16(dY) || !aligned16(X));
    // the row chunks are those of the vector grid on either path
    const int col_blocks = ((n_cols + VEC - 1) / VEC + 255) / 256;
    // ~2048 blocks in flight (8 per CU), at least 8 rows per chunk, bounded by the workspace
    int64_t chunks = (2048 + col_blocks - 1) / col_blocks;
    if (chunks > (n_rows + 7) / 8) chunks = (n_rows + 7) / 8;
    if (chunks > ws_elems / n_cols) chunks = ws_elems / n_cols;
    if (chunks < 1) return UAMD_ERR_ARG;
    const int rows_per_chunk = (int)((n_rows + chunks - 1) / chunks);
    chunks = (n_rows + rows_per_chunk - 1) / rows_per_chunk;
    if (vec_ok)
        hipLaunchKernelGGL((rms_dw_partial<T, true>), dim3(col_blocks, (unsigned)chunks), dim3(256), 0, st, (const T*)dY,
                           (const T*)X, r, ws, n_rows, n_cols, dys, xs, rows_per_chunk);
    else
        hipLaunchKernelGGL((rms_dw_partial<T, false>), dim3((n_cols + 255) / 256, (unsigned)chunks), dim3(256), 0, st,
                           (const T*)dY, (const T*)X, r, ws, n_rows, n_cols, dys, xs, rows_per_chunk);
    hipLaunchKernelGGL((rms_dw_reduce<WT>), dim3((n_cols + 255) / 256), dim3(256), 0, st, ws, (WT*)dW, n_cols, (int)chunks,
                       accumulate);
    return uamd_launch_status();
}
}  // namespace

// dW[n_cols] (+)= sum over rows of dY * X * r. `workspace`: fp32 scratch of ws_elems >= n_cols elements (more = more row
// chunks in flight: 2048 / ceil(n_cols / (256 * vec)) chunks x n_cols saturates the chip). dW in w_dtype. Any width, row
// stride and pointer alignment: what is no multiple of 16 bytes takes scalar loads.
extern "C" int uamd_rms_layernorm_dw(const void* dY, const void* X, const float* r, void* dW, float* workspace,
                                     int64_t ws_elems, int64_t n_rows, int n_cols, int64_t dy_row_stride,
                                     int64_t x_row_stride, int accumulate, int x_dtype, int w_dtype, void* stream) {
    if (n_rows < 0 || n_cols <= 0 || !dY || !X || !r || !dW || !workspace) return UAMD_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (n_rows == 0) {
        if (!accumulate) return (int)hipMemsetAsync(dW, 0, (size_t)n_cols * (w_dtype == UAMD_F32 ? 4 : 2), st);
        return UAMD_OK;
    }
    UAMD_DISPATCH_NORM(x_dtype, w_dtype, return launch_dw<T, WT>(dY, X, r, dW, workspace, ws_elems, n_rows, n_cols,
                                                                 dy_row_stride, x_row_stride, accumulate, st))
}

extern "C" int uamd_rms_layernorm_fwd(const void* X, const void* W, void* Y, float* r,
                                      int64_t n_rows, int n_cols, int64_t x_row_stride,
                                      int64_t y_row_stride, float eps, int gemma, int x_dtype,
                                      int w_dtype, void* stream) {
    if (n_rows < 0 || n_cols <= 0) return UAMD_ERR_ARG;
    if (n_rows == 0) return UAMD_OK;
    hipStream_t st = (hipStream_t)stream;
    UAMD_DISPATCH_NORM(x_dtype, w_dtype, auto f = gemma ? launch_fwd<T, WT, true, false> : launch_fwd<T, WT, false, false>;
                       return f(X, W, Y, r, n_rows, n_cols, x_row_stride, y_row_stride, eps, st, nullptr, nullptr, 0, 0))
}

extern "C" int uamd_rms_layernorm_bwd(const void* dY, void* dX, const void* X, const void* W,
                                      const float* r, int64_t n_rows, int n_cols,
                                      int64_t dy_row_stride, int64_t dx_row_stride,
                                      int64_t x_row_stride, int gemma, int x_dtype, int w_dtype,
                                      void* stream) {
    if (n_rows < 0 || n_cols <= 0) return UAMD_ERR_ARG;
    if (n_rows == 0) return UAMD_OK;
    hipStream_t st = (hipStream_t)stream;
    UAMD_DISPATCH_NORM(x_dtype, w_dtype, auto f = gemma ? launch_bwd<T, WT, true, false> : launch_bwd<T, WT, false, false>;
                       return f(dY, dX, X, W, r, n_rows, n_cols, dy_row_stride, dx_row_stride, x_row_stride, st, nullptr, 0))
}

// h = X + Res (written to H), Y = rmsnorm(h) * W, r = rsqrt(mean h^2 + eps): residual add + norm in ONE pass
// (the reference runs them as two, llama.py:823-844). Rows up to 64*8 16-byte vectors, 16-byte aligned
// (otherwise UAMD_ERR_ALIGN: call the two separate ops). H may alias Res or X.
extern "C" int uamd_add_rms_layernorm_fwd(const void* X, const void* Res, const void* W, void* H, void* Y, float* r,
                                          int64_t n_rows, int n_cols, int64_t x_row_stride, int64_t res_row_stride,
                                          int64_t h_row_stride, int64_t y_row_stride, float eps, int x_dtype,
                                          int w_dtype, void* stream) {
    if (n_rows < 0 || n_cols <= 0 || !X || !Res || !H || !Y || !W || !r) return UAMD_ERR_ARG;
    if (n_rows == 0) return UAMD_OK;
    hipStream_t st = (hipStream_t)stream;
    UAMD_DISPATCH_NORM(x_dtype, w_dtype, return launch_fwd<T, WT, false, true>(
        X, W, Y, r, n_rows, n_cols, x_row_stride, y_row_stride, eps, st, Res, H, res_row_stride, h_row_stride))
}

// dX = rmsnorm_backward(dY; h, W, r) + dRes, dRes = the gradient arriving at h from the residual path. dX may
// alias dY (the reference's in-place contract, rms_layernorm.py:218) or dRes.
extern "C" int uamd_add_rms_layernorm_bwd(const void* dY, const void* dRes, void* dX, const void* H, const void* W,
                                          const float* r, int64_t n_rows, int n_cols, int64_t dy_row_stride,
                                          int64_t dres_row_stride, int64_t dx_row_stride, int64_t h_row_stride,
                                          int x_dtype, int w_dtype, void* stream) {
    if (n_rows < 0 || n_cols <= 0 || !dY || !dRes || !dX || !H || !W || !r) return UAMD_ERR_ARG;
    if (n_rows == 0) return UAMD_OK;
    hipStream_t st = (hipStream_t)stream;
    UAMD_DISPATCH_NORM(x_dtype, w_dtype, return launch_bwd<T, WT, false, true>(
        dY, dX, H, W, r, n_rows, n_cols, dy_row_stride, dx_row_stride, h_row_stride, st, dRes, dres_row_stride))
}
