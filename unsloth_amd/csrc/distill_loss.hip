// Full-vocabulary distillation loss between two logits matrices (TRL GKDTrainer.generalized_jsd_loss): forward KL, reverse KL
// and the generalized Jensen-Shannon divergence, per row, and the in-place gradient for the student logits.
//
// With a = t / tau (teacher), b = z / tau (student), p = softmax(a), q = softmax(b), per row:
//   beta == 0   forward KL   sum p (log p - log q)
//   beta == 1   reverse KL   sum q (log q - log p)
//   otherwise   JSD          beta KL(p || m) + (1 - beta) KL(q || m),   m = beta p + (1 - beta) q
// A row whose label is -100 contributes 0 and gets a zero gradient row. The teacher gets no gradient.
//
// FORWARD, one launch. The two KL forms are ONE pass over the row's two streams: every lane carries the online (max, sum)
// pair of both streams (the pair of ce_fwd_kernel) and, for the stream that weighs the sum (the teacher for the forward KL, the
// student for the reverse one; "w", the other one "o"), a third running sum
//   u = sum exp(w_i - m_w) (w_i - o_i)         u <- e^(m_w - M) u when the maximum moves to M
// so that at the end KL = U / S_w - lse_w + lse_o. A term of weight 0 adds 0 (a -inf logit in the weighing stream, an idle
// lane): never 0 * inf. Lanes merge through the wave shuffle, the four waves of a block through 4 LDS entries that every
// thread then folds in the same order. The JSD needs log m_i and therefore both lse first: the same block streams the row a
// second time (it is still in L2 / Infinity Cache) and sums p (log p - log m) and q (log q - log m) with
//   log m = mx + log(beta e^(log p - mx) + (1 - beta) e^(log q - mx)),  mx = max(log p, log q)      (one of the two e's is 1)
// which cannot underflow where p or q is representable. No atomics; one fixed order: the same bits on every launch.
//
// BACKWARD, one streaming pass, dz written over the student logits (the package's in-place contract, as ce_bwd_kernel), all
// arithmetic in fp32 and one rounding at the store. With g = dloss[row] / tau:
//   forward KL  (q - p) g
//   reverse KL  q ((log q - log p) - RKL) g
//   JSD         (1 - beta) q ((log q - log m) - KL(q || m)) g       (the beta term cancels)
// `kl_student` is the forward's fourth output: RKL for beta == 1, KL(q || m) for the JSD (the row loss alone does not give it).
//
// ROWS TO WORKGROUPS. A row of at most DL_WAVE_ROW_MAX_V logits is one WAVE's (four rows per 256-thread block, no LDS, no
// barrier): at V = 1000 a whole block would have work for 125 of its 256 lanes and pay a barrier per row. Longer rows: one block
// per row forward (the sums need the whole row), one block per (row, 4-vector-per-thread chunk) backward, as ce_bwd_kernel.
// Vector path (16-byte loads of both streams, scalar tail) when both base pointers are 16-byte aligned and both row strides a
// multiple of the vector; any other view takes the scalar instantiation.
#include "common.h"

namespace {

constexpr int DL_THREADS = 256;
constexpr int DL_WAVE_ROW_MAX_V = 4096;
enum { DL_FKL = 0, DL_RKL = 1, DL_JSD = 2 };

__device__ __forceinline__ bool row_live(const void* labels, int labels_i64, int64_t row) {
    if (!labels) return true;
    const int64_t l = labels_i64 ? ((const int64_t*)labels)[row] : (int64_t)((const int32_t*)labels)[row];
    return l != -100;
}

// per-lane state of a row: (m, s) of the weighing stream with its u, (m, s) of the other stream
struct RowState { float mw, sw, u, mo, so; };

__device__ __forceinline__ void pair_merge(float& m, float& s, float m2, float s2) {
    const float M = fmaxf(m, m2);
    if (M == -INFINITY) { m = M; s = 0.f; return; }
    s = s * __expf(m - M) + s2 * __expf(m2 - M);
    m = M;
}
// symmetric in its two sides: both lanes of a shuffle pair end with the same bits
__device__ __forceinline__ void kl_merge(float& m, float& s, float& u, float m2, float s2, float u2) {
    const float M = fmaxf(m, m2);
    if (M == -INFINITY) { m = M; s = 0.f; u = 0.f; return; }
    const float e1 = __expf(m - M), e2 = __expf(m2 - M);
    u = ((e1 == 0.f) ? 0.f : e1 * u) + ((e2 == 0.f) ? 0.f : e2 * u2);
    s = s * e1 + s2 * e2;
    m = M;
}

// N scaled logits of both streams into a lane's state: one rescale for the N (the vector step of ce_fwd_kernel)
template <bool KL, int N>
__device__ __forceinline__ void absorb(RowState& r, const float (&a)[N], const float (&b)[N]) {
    float la = a[0], lb = b[0];
#pragma unroll
    for (int j = 1; j < N; ++j) { la = fmaxf(la, a[j]); lb = fmaxf(lb, b[j]); }
    const float Ma = fmaxf(r.mw, la);
    if (Ma != -INFINITY) {
        const float e0 = __expf(r.mw - Ma);
        float sacc = r.sw * e0, uacc = 0.f;
        if constexpr (KL) uacc = (e0 == 0.f) ? 0.f : e0 * r.u;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float e = __expf(a[j] - Ma);
            sacc += e;
            if constexpr (KL) uacc += (e == 0.f) ? 0.f : e * (a[j] - b[j]);      // weight 0: 0, not 0 * inf
        }
        r.sw = sacc;
        r.mw = Ma;
        if constexpr (KL) r.u = uacc;
    }
    const float Mb = fmaxf(r.mo, lb);
    if (Mb != -INFINITY) {
        float sacc = r.so * __expf(r.mo - Mb);
#pragma unroll
        for (int j = 0; j < N; ++j) sacc += __expf(b[j] - Mb);
        r.so = sacc;
        r.mo = Mb;
    }
}

// log(beta e^lp + (1 - beta) e^lq) for max(lp, lq) finite
__device__ __forceinline__ float log_mix(float lp, float lq, float beta) {
    const float mx = fmaxf(lp, lq), r = __expf(fminf(lp, lq) - mx);
    const float arg = (lp >= lq) ? beta + (1.f - beta) * r : beta * r + (1.f - beta);
    return mx + __logf(arg);
}

template <int N>
__device__ __forceinline__ void jsd_absorb(float& A, float& B, const float (&b)[N], const float (&a)[N], float lse_q, float lse_p,
                                           float beta) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const float lq = b[j] - lse_q, lp = a[j] - lse_p;
        if (fmaxf(lp, lq) == -INFINITY) continue;
        const float lm = log_mix(lp, lq, beta), p = __expf(lp), q = __expf(lq);
        A += (p == 0.f) ? 0.f : p * (lp - lm);
        B += (q == 0.f) ? 0.f : q * (lq - lm);
    }
}

// f(w[N], o[N]) over the row's scaled logits, the lanes of a TPR-thread team interleaved: two 16-byte vectors of each stream per
// trip, all four loads issued before any is consumed, then the scalar tail (VECTOR) or the whole row element by element
template <typename T, bool VECTOR, int TPR, typename F>
__device__ __forceinline__ void stream_row(const T* w, const T* o, int vocab, int tid, float inv_tau, F&& f) {
    constexpr int VEC = Vec16<T>::N;
    int tail = 0;
    if constexpr (VECTOR) {
        const int nvec = vocab / VEC;
        auto one = [&](const Vec16<T>& vw, const Vec16<T>& vo) {
            float a[VEC], b[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) { a[j] = to_f32(vw.e[j]) * inv_tau; b[j] = to_f32(vo.e[j]) * inv_tau; }
            f(a, b);
        };
        int i = tid;
        for (; i + TPR < nvec; i += 2 * TPR) {
            const Vec16<T> w0 = ld16(w + (int64_t)i * VEC), o0 = ld16(o + (int64_t)i * VEC);
            const Vec16<T> w1 = ld16(w + (int64_t)(i + TPR) * VEC), o1 = ld16(o + (int64_t)(i + TPR) * VEC);
            one(w0, o0);
            one(w1, o1);
        }
        if (i < nvec) one(ld16(w + (int64_t)i * VEC), ld16(o + (int64_t)i * VEC));
        tail = nvec * VEC;
    }
    for (int c = tail + tid; c < vocab; c += TPR) {
        const float a[1] = {to_f32(w[c]) * inv_tau}, b[1] = {to_f32(o[c]) * inv_tau};
        f(a, b);
    }
}

// xw / xo: the weighing and the other stream (teacher, student for the forward KL; student, teacher otherwise), lse_w / lse_o
// their outputs. TPR threads per row: 64 (a wave, DL_THREADS / 64 rows per block) or DL_THREADS (one row per block).
template <typename T, bool VECTOR, bool JSD, int TPR>
__global__ void __launch_bounds__(DL_THREADS)
distill_fwd_kernel(const T* xw, int64_t rs_w, const T* xo, int64_t rs_o, float* __restrict__ loss, float* __restrict__ lse_w,
                   float* __restrict__ lse_o, float* __restrict__ kl_student, const void* __restrict__ labels, int labels_i64,
                   int64_t n_rows, int vocab, float beta, float inv_tau) {
    constexpr int WAVES = DL_THREADS / UAMD_WAVE;
    __shared__ float red[TPR == DL_THREADS ? WAVES : 1][5], red2[TPR == DL_THREADS ? WAVES : 1][2];
    const int tid = threadIdx.x % TPR;
    const int64_t row = (int64_t)blockIdx.x * (DL_THREADS / TPR) + threadIdx.x / TPR;
    if (row >= n_rows) return;                        // a whole wave (TPR == 64); never taken with one row per block
    if (!row_live(labels, labels_i64, row)) {         // uniform over the row's team, before any barrier
        if (tid == 0) { loss[row] = 0.f; lse_w[row] = 0.f; lse_o[row] = 0.f; kl_student[row] = 0.f; }
        return;
    }
    const T* w = xw + row * rs_w;
    const T* o = xo + row * rs_o;
    RowState r = {-INFINITY, 0.f, 0.f, -INFINITY, 0.f};
    stream_row<T, VECTOR, TPR>(w, o, vocab, tid, inv_tau, [&](const auto& a, const auto& b) { absorb<!JSD>(r, a, b); });
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const float mw = __shfl_xor(r.mw, s, 64), sw = __shfl_xor(r.sw, s, 64), mo = __shfl_xor(r.mo, s, 64), so = __shfl_xor(r.so, s, 64);
        if constexpr (JSD) pair_merge(r.mw, r.sw, mw, sw);
        else kl_merge(r.mw, r.sw, r.u, mw, sw, __shfl_xor(r.u, s, 64));
        pair_merge(r.mo, r.so, mo, so);
    }
    const int wave = threadIdx.x >> 6;
    if constexpr (TPR == DL_THREADS) {
        if ((threadIdx.x & 63) == 0) { red[wave][0] = r.mw; red[wave][1] = r.sw; red[wave][2] = r.u; red[wave][3] = r.mo; red[wave][4] = r.so; }
        __syncthreads();
        r = RowState{red[0][0], red[0][1], red[0][2], red[0][3], red[0][4]};      // every thread, the same order: the same bits
#pragma unroll
        for (int i = 1; i < WAVES; ++i) {
            if constexpr (JSD) pair_merge(r.mw, r.sw, red[i][0], red[i][1]);
            else kl_merge(r.mw, r.sw, r.u, red[i][0], red[i][1], red[i][2]);
            pair_merge(r.mo, r.so, red[i][3], red[i][4]);
        }
    }
    const float lw = r.mw + logf(r.sw), lo = r.mo + logf(r.so);
    if constexpr (!JSD) {
        if (tid == 0) {
            const float kl = (r.u / r.sw - lw) + lo;              // equal rows: u == 0 and lw == lo bit for bit -> exactly 0
            loss[row] = kl;
            kl_student[row] = kl;
            lse_w[row] = lw;
            lse_o[row] = lo;
        }
    } else {
        // w = student (q), o = teacher (p)
        float A = 0.f, B = 0.f;
        stream_row<T, VECTOR, TPR>(w, o, vocab, tid, inv_tau, [&](const auto& b, const auto& a) { jsd_absorb(A, B, b, a, lw, lo, beta); });
        A = wave_sum(A);
        B = wave_sum(B);
        if constexpr (TPR == DL_THREADS) {
            if ((threadIdx.x & 63) == 0) { red2[wave][0] = A; red2[wave][1] = B; }
            __syncthreads();
            A = red2[0][0];
            B = red2[0][1];
#pragma unroll
            for (int i = 1; i < WAVES; ++i) { A += red2[i][0]; B += red2[i][1]; }
        }
        if (tid == 0) {
            loss[row] = beta * A + (1.f - beta) * B;
            kl_student[row] = B;
            lse_w[row] = lw;
            lse_o[row] = lo;
        }
    }
}

struct GradRow { float lse_z, lse_t, klq, beta, g, inv_tau; bool live; };

template <typename T, int MODE>
__device__ __forceinline__ T distill_grad(T zin, T tin, const GradRow& R) {
    const float lq = to_f32(zin) * R.inv_tau - R.lse_z, lp = to_f32(tin) * R.inv_tau - R.lse_t;
    const float q = __expf(lq);
    float d;
    if constexpr (MODE == DL_FKL) {
        d = q - __expf(lp);
    } else if constexpr (MODE == DL_RKL) {
        d = (q == 0.f) ? 0.f : q * ((lq - lp) - R.klq);
    } else {
        d = (q == 0.f) ? 0.f : (1.f - R.beta) * (q * ((lq - log_mix(lp, lq, R.beta)) - R.klq));
    }
    return from_f32<T>(R.live ? d * R.g : 0.f);       // a masked row: exactly 0 whatever its logits hold
}

template <typename T, bool VECTOR, int MODE, int TPR>
__global__ void __launch_bounds__(DL_THREADS)
distill_bwd_kernel(T* xz, int64_t rs_z, const T* xt, int64_t rs_t, const float* __restrict__ dloss, int64_t dloss_stride,
                   const float* __restrict__ lse_z, const float* __restrict__ lse_t, const float* __restrict__ kl_student,
                   const void* __restrict__ labels, int labels_i64, int64_t n_rows, int vocab, float beta, float inv_tau, int chunk) {
    constexpr int VEC = Vec16<T>::N;
    const int tid = threadIdx.x % TPR;
    const int64_t row = (int64_t)blockIdx.x * (DL_THREADS / TPR) + threadIdx.x / TPR;
    if (row >= n_rows) return;
    T* z = xz + row * rs_z;
    const T* t = xt + row * rs_t;
    GradRow R;
    R.live = row_live(labels, labels_i64, row);
    R.lse_z = lse_z[row];
    R.lse_t = lse_t[row];
    R.klq = kl_student[row];
    R.beta = beta;
    R.inv_tau = inv_tau;
    R.g = R.live ? dloss[row * dloss_stride] * inv_tau : 0.f;
    const int c0 = (TPR == DL_THREADS) ? blockIdx.y * chunk : 0;
    const int c1 = (TPR == DL_THREADS) ? min(c0 + chunk, vocab) : vocab;
    int tail = c0;
    if constexpr (VECTOR) {
        // chunk is a multiple of VEC; a row's last chunk may end on a ragged tail
        const int cvec_end = c0 + ((c1 - c0) / VEC) * VEC;
        if (TPR == DL_THREADS && c0 + 4 * DL_THREADS * VEC <= cvec_end) {
            // a full chunk: all eight loads, then four computes + stores (the branch-free form of ce_bwd_kernel)
            const int cb = c0 + tid * VEC;
            Vec16<T> vz[4], vt[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { vz[k] = ld16(z + cb + k * DL_THREADS * VEC); vt[k] = ld16(t + cb + k * DL_THREADS * VEC); }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                Vec16<T> out;
#pragma unroll
                for (int j = 0; j < VEC; ++j) out.e[j] = distill_grad<T, MODE>(vz[k].e[j], vt[k].e[j], R);
                st16(z + cb + k * DL_THREADS * VEC, out);
            }
        } else {
            for (int c = c0 + tid * VEC; c < cvec_end; c += TPR * VEC) {
                const Vec16<T> vz = ld16(z + c), vt = ld16(t + c);
                Vec16<T> out;
#pragma unroll
                for (int j = 0; j < VEC; ++j) out.e[j] = distill_grad<T, MODE>(vz.e[j], vt.e[j], R);
                st16(z + c, out);
            }
        }
        tail = cvec_end;
    }
    for (int c = tail + tid; c < c1; c += TPR) z[c] = distill_grad<T, MODE>(z[c], t[c], R);
}

template <typename F>
void with_bool(bool b, F&& f) {
    if (b) f(std::integral_constant<bool, true>{}); else f(std::integral_constant<bool, false>{});
}

template <typename T>
bool both_vectorizable(const void* a, int64_t rs_a, const void* b, int64_t rs_b) {
    return aligned16(a) && aligned16(b) && rs_a % Vec16<T>::N == 0 && rs_b % Vec16<T>::N == 0;
}

int mode_of(float beta) { return beta == 0.f ? DL_FKL : beta == 1.f ? DL_RKL : DL_JSD; }

template <typename T>
int launch_fwd(const void* z, int64_t rs_z, const void* t, int64_t rs_t, float* loss, float* lse_z, float* lse_t, float* klq,
               const void* labels, int labels_i64, int64_t n_rows, int vocab, float beta, float tau, hipStream_t st) {
    const int mode = mode_of(beta);
    // the weighing stream first: the teacher for the forward KL, the student otherwise
    const bool tw = mode == DL_FKL;
    const T* xw = (const T*)(tw ? t : z);
    const T* xo = (const T*)(tw ? z : t);
    const int64_t rs_w = tw ? rs_t : rs_z, rs_o = tw ? rs_z : rs_t;
    float* lse_w = tw ? lse_t : lse_z;
    float* lse_o = tw ? lse_z : lse_t;
    const float inv_tau = 1.0f / tau;
    with_bool(both_vectorizable<T>(z, rs_z, t, rs_t), [&](auto vec) {
        with_bool(mode == DL_JSD, [&](auto jsd) {
            with_bool(vocab <= DL_WAVE_ROW_MAX_V, [&](auto wave_rows) {
                constexpr int TPR = decltype(wave_rows)::value ? UAMD_WAVE : DL_THREADS;
                constexpr int RPB = DL_THREADS / TPR;
                const dim3 grid((unsigned)((n_rows + RPB - 1) / RPB));
                hipLaunchKernelGGL((distill_fwd_kernel<T, decltype(vec)::value, decltype(jsd)::value, TPR>), grid, dim3(DL_THREADS), 0,
                                   st, xw, rs_w, xo, rs_o, loss, lse_w, lse_o, klq, labels, labels_i64, n_rows, vocab, beta, inv_tau);
            });
        });
    });
    return uamd_launch_status();
}

template <typename T, int MODE>
void launch_bwd_mode(void* z, int64_t rs_z, const void* t, int64_t rs_t, const float* dloss, int64_t ds, const float* lse_z,
                     const float* lse_t, const float* klq, const void* labels, int labels_i64, int64_t n_rows, int vocab,
                     float beta, float tau, hipStream_t st) {
    const float inv_tau = 1.0f / tau;
    const int chunk = DL_THREADS * Vec16<T>::N * 4;
    with_bool(both_vectorizable<T>(z, rs_z, t, rs_t), [&](auto vec) {
        with_bool(vocab <= DL_WAVE_ROW_MAX_V, [&](auto wave_rows) {
            constexpr int TPR = decltype(wave_rows)::value ? UAMD_WAVE : DL_THREADS;
            constexpr int RPB = DL_THREADS / TPR;
            const dim3 grid((unsigned)((n_rows + RPB - 1) / RPB), TPR == DL_THREADS ? (unsigned)((vocab + chunk - 1) / chunk) : 1u);
            hipLaunchKernelGGL((distill_bwd_kernel<T, decltype(vec)::value, MODE, TPR>), grid, dim3(DL_THREADS), 0, st, (T*)z, rs_z,
                               (const T*)t, rs_t, dloss, ds, lse_z, lse_t, klq, labels, labels_i64, n_rows, vocab, beta, inv_tau, chunk);
        });
    });
}

template <typename T>
int launch_bwd(void* z, int64_t rs_z, const void* t, int64_t rs_t, const float* dloss, int64_t ds, const float* lse_z,
               const float* lse_t, const float* klq, const void* labels, int labels_i64, int64_t n_rows, int vocab, float beta,
               float tau, hipStream_t st) {
#define L(MODE) launch_bwd_mode<T, MODE>(z, rs_z, t, rs_t, dloss, ds, lse_z, lse_t, klq, labels, labels_i64, n_rows, vocab, beta, tau, st)
    switch (mode_of(beta)) {
        case DL_FKL: L(DL_FKL); break;
        case DL_RKL: L(DL_RKL); break;
        default: L(DL_JSD); break;
    }
#undef L
    return uamd_launch_status();
}

bool args_ok(int64_t rs_z, int64_t rs_t, int64_t n_rows, int vocab, float beta, float tau) {
    return n_rows >= 0 && n_rows <= 0x7fffffffLL && vocab > 0 && vocab <= (1 << 30) && rs_z >= vocab && rs_t >= vocab &&
           beta >= 0.f && beta <= 1.f && tau > 0.f && tau <= 3.0e38f;
}

}  // namespace

// loss[row] = the divergence of the row (0 where labels[row] == -100; labels NULL: every row counts), lse_student / lse_teacher
// = logsumexp of the row's logits / temperature, kl_student = what the backward needs beside them (reverse KL: the loss; JSD:
// KL(q || m)). All fp32 [n_rows]. labels: int64 (labels_i64 != 0) or int32.
extern "C" int uamd_distill_loss_forward(const void* student, int64_t student_row_stride, const void* teacher,
                                         int64_t teacher_row_stride, float* loss, float* lse_student, float* lse_teacher,
                                         float* kl_student, const void* labels, int labels_i64, int64_t n_rows,
                                         int vocab_size, float beta, float temperature, int dtype, void* stream) {
    if (!args_ok(student_row_stride, teacher_row_stride, n_rows, vocab_size, beta, temperature)) return UAMD_ERR_ARG;
    if (n_rows == 0) return UAMD_OK;
    UAMD_DISPATCH_FLOAT(dtype, return (launch_fwd<T>(student, student_row_stride, teacher, teacher_row_stride, loss, lse_student,
                                                     lse_teacher, kl_student, labels, labels_i64, n_rows, vocab_size, beta,
                                                     temperature, (hipStream_t)stream)))
    return UAMD_ERR_DTYPE;
}

// student <- dloss[row] * d(loss[row]) / d(student logits), in place (same dtype); a zero row where labels[row] == -100.
extern "C" int uamd_distill_loss_backward(void* student, int64_t student_row_stride, const void* teacher,
                                          int64_t teacher_row_stride, const float* dloss, int64_t dloss_stride,
                                          const float* lse_student, const float* lse_teacher, const float* kl_student,
                                          const void* labels, int labels_i64, int64_t n_rows, int vocab_size, float beta,
                                          float temperature, int dtype, void* stream) {
    if (!args_ok(student_row_stride, teacher_row_stride, n_rows, vocab_size, beta, temperature)) return UAMD_ERR_ARG;
    if (n_rows == 0) return UAMD_OK;
    UAMD_DISPATCH_FLOAT(dtype, return (launch_bwd<T>(student, student_row_stride, teacher, teacher_row_stride, dloss, dloss_stride,
                                                     lse_student, lse_teacher, kl_student, labels, labels_i64, n_rows, vocab_size,
                                                     beta, temperature, (hipStream_t)stream)))
    return UAMD_ERR_DTYPE;
}
