// AdamW over ONE flat fp32 arena: parameters, gradients and both moments of all LoRA factors laid out back to back
// (unsloth_amd/optim.py FlatAdamW; gradients = dp.LoRAGradArena). One launch per optimizer step.
//
// Where it sits on the reference's path: the optimizer step that closes every training step of the benchmark
// (unsloth/trainer.py:445-623 builds torch / bitsandbytes optimizers through HF's Trainer; the tokens/s metric times
// forward + backward + this). torch's fused AdamW walks the 448 LoRA tensors in multi_tensor_apply chunks: 52 launches,
// 2.5 ms per step for 168 MB of parameters (profiles/r02z_bench_kernel_stats.csv) -- 8 streams of 168 MB are 0.22 ms of
// HBM time. The arithmetic is torch.optim.AdamW's (decoupled weight decay, bias-corrected moments; fp32 throughout):
//     p  -= lr * wd * p
//     m   = b1 * m + (1 - b1) * g
//     v   = b2 * v + (1 - b2) * g * g
//     p  -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)            bc1 = 1 - b1^t, bc2 = 1 - b2^t
// `grad_scale` multiplies g first (gradient clipping: the caller passes clip / norm, 1 = none); `zero_grad` != 0 writes
// zeros back into g in the same pass (the arena is ADDED into by uamd_lora_tn, so it must start every step at zero:
// this replaces a separate 168 MB fill).
// HBM-bound: 16 B read + 12 (16 with zero_grad) B written per parameter.
#include "common.h"

namespace {

struct AdamArgs {
    float* p; float* g; float* m; float* v;
    int64_t n;
    float lr_wd, b1, b2, omb1, omb2, eps, step_size, bc2_sqrt, grad_scale;
    int zero_grad;
};

// x - d, with x kept bit for bit when d is +-0: IEEE gives (-0) - (-0) = +0, and lr_wd * (-0) is -0, so a weight stored as
// -0.0 would come back as +0.0 from every step (torch's p.mul_(1 - lr * wd) keeps it). Every other value is unchanged.
__device__ __forceinline__ float sub_keep(float x, float d) { return d == 0.f ? x : x - d; }

__device__ __forceinline__ void adamw_one(float& p, float& g, float& m, float& v, const AdamArgs& a) {
    const float gr = g * a.grad_scale;
    // same association as torch's fused kernel (fused_adam_utils.cuh adam_math): ... - step_size * m / denom
    p = sub_keep(p, a.lr_wd * p);
    m = a.b1 * m + a.omb1 * gr;
    v = a.b2 * v + a.omb2 * gr * gr;
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = sub_keep(p, a.step_size * m / denom);
}

__global__ void __launch_bounds__(256) adamw_flat_kernel(AdamArgs a) {
    const int64_t n4 = a.n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 p = reinterpret_cast<const float4*>(a.p)[i];
        float4 g = reinterpret_cast<const float4*>(a.g)[i];
        float4 m = reinterpret_cast<const float4*>(a.m)[i];
        float4 v = reinterpret_cast<const float4*>(a.v)[i];
        adamw_one(p.x, g.x, m.x, v.x, a);
        adamw_one(p.y, g.y, m.y, v.y, a);
        adamw_one(p.z, g.z, m.z, v.z, a);
        adamw_one(p.w, g.w, m.w, v.w, a);
        reinterpret_cast<float4*>(a.p)[i] = p;
        reinterpret_cast<float4*>(a.m)[i] = m;
        reinterpret_cast<float4*>(a.v)[i] = v;
        if (a.zero_grad) reinterpret_cast<float4*>(a.g)[i] = float4{0.f, 0.f, 0.f, 0.f};
    }
    // tail (n % 4 elements): first threads of block 0
    const int64_t t = (n4 << 2) + threadIdx.x;
    if (blockIdx.x == 0 && t < a.n) {
        adamw_one(a.p[t], a.g[t], a.m[t], a.v[t], a);
        if (a.zero_grad) a.g[t] = 0.f;
    }
}

// Mixed-precision form for FULL fine-tuning (unsloth_amd/full_finetune.py): the fp32 master copy + moments of one
// rank's SHARD of a flat bucket, the gradient shard in the model's 16-bit dtype (what the reduce-scatter delivered), and
// the updated parameters written back in the 16-bit dtype into the bucket slice the all-gather then broadcasts.
// 14 B read + 14 B written per parameter.
template <typename T>
__global__ void __launch_bounds__(256) adamw_shard_kernel(AdamArgs a, const T* __restrict__ g16, T* __restrict__ p16) {
    const int64_t n4 = a.n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 p = reinterpret_cast<const float4*>(a.p)[i];
        float4 m = reinterpret_cast<const float4*>(a.m)[i];
        float4 v = reinterpret_cast<const float4*>(a.v)[i];
        union { uint2 raw; T e[4]; } gi, po;
        gi.raw = reinterpret_cast<const uint2*>(g16)[i];
        float g0 = to_f32(gi.e[0]), g1 = to_f32(gi.e[1]), g2 = to_f32(gi.e[2]), g3 = to_f32(gi.e[3]);
        adamw_one(p.x, g0, m.x, v.x, a);
        adamw_one(p.y, g1, m.y, v.y, a);
        adamw_one(p.z, g2, m.z, v.z, a);
        adamw_one(p.w, g3, m.w, v.w, a);
        reinterpret_cast<float4*>(a.p)[i] = p;
        reinterpret_cast<float4*>(a.m)[i] = m;
        reinterpret_cast<float4*>(a.v)[i] = v;
        po.e[0] = from_f32<T>(p.x); po.e[1] = from_f32<T>(p.y); po.e[2] = from_f32<T>(p.z); po.e[3] = from_f32<T>(p.w);
        reinterpret_cast<uint2*>(p16)[i] = po.raw;
    }
    const int64_t t = (n4 << 2) + threadIdx.x;
    if (blockIdx.x == 0 && t < a.n) {
        float g = to_f32(g16[t]);
        adamw_one(a.p[t], g, a.m[t], a.v[t], a);
        p16[t] = from_f32<T>(a.p[t]);
    }
}

// ---- 8-bit moments (bitsandbytes' block-wise 2-state AdamW, optim="adamw_8bit") ------------------------------------------
// exp_avg / exp_avg_sq are stored as one uint8 code per element + one fp32 absmax per 256-element block: value =
// code[idx] * absmax[blk], `code` a sorted 256-entry map (signed dynamic map for m, unsigned for v; passed in, like the NF4
// state's). Per block: decode -> adamw_one (the parameter moves with the NEW fp32 moments, before they are rounded) -> new
// absmax = max |m| / max v over the block -> idx = nearest map entry to m / absmax (true division; an exact tie takes the
// lower index, torch.bucketize's rule on the midpoints).
// One wave64 owns one block: 4 elements per lane (one float4 of p, one 32-bit word of each code array), the block maximum is
// a 64-lane shuffle reduction -- no LDS round trip, no barrier inside the loop. The two maps and their 255 midpoints each sit
// in LDS (4 KB); the encode is an 8-step lower-bound search over the midpoints.
// HBM: flat 10 B read + 10 B written per parameter (fp32: 16 + 16), shard 8 + 8 (fp32: 14 + 14).
struct Adam8Args {
    AdamArgs a;                               // a.m / a.v unused
    uint8_t* m8; uint8_t* v8;
    float* absmax_m; float* absmax_v;
    const float* code_m; const float* code_v;
    int64_t decay_begin, decay_end;           // weight decay applies to elements in [decay_begin, decay_end) only
};

#define UAMD_ADAM8_BLOCK 256

__device__ __forceinline__ uint32_t adam8_encode(float x, const float* __restrict__ mids) {
    // number of midpoints < x  ==  torch.bucketize(x, mids): 255 midpoints, 8 steps
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t s = 128; s > 0; s >>= 1)
        if (mids[pos + s - 1] < x) pos += s;
    return pos;
}

// T = float: the flat LoRA arena (fp32 gradient in a.g, zeroed when a.zero_grad); T = bf16 / fp16: a full fine-tuning shard
// (gradient g16, updated parameters rounded once into p16).
template <typename T>
__global__ void __launch_bounds__(256) adamw8_kernel(Adam8Args q, const T* __restrict__ g16, T* __restrict__ p16) {
    constexpr bool FLAT = std::is_same<T, float>::value;
    __shared__ float s_code[2][256];
    __shared__ float s_mids[2][256];
    {
        const int t = threadIdx.x;
        s_code[0][t] = q.code_m[t];
        s_code[1][t] = q.code_v[t];
        s_mids[0][t] = t < 255 ? (q.code_m[t] + q.code_m[t + 1]) * 0.5f : 0.f;
        s_mids[1][t] = t < 255 ? (q.code_v[t] + q.code_v[t + 1]) * 0.5f : 0.f;
    }
    __syncthreads();
    const AdamArgs a = q.a;
    AdamArgs a0 = a;                          // the same step without weight decay
    a0.lr_wd = 0.f;
    const int lane = threadIdx.x & 63;
    const int64_t n = a.n;
    const int64_t nblk = (n + UAMD_ADAM8_BLOCK - 1) / UAMD_ADAM8_BLOCK;
    const int64_t stride = (int64_t)gridDim.x * 4;
    for (int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); blk < nblk; blk += stride) {
        const int64_t e0 = blk * UAMD_ADAM8_BLOCK + 4 * lane;       // this lane's first element
        const bool full = e0 + 3 < n;                               // all four valid: vector accesses
        const float am = q.absmax_m[blk], av = q.absmax_v[blk];
        float p[4], g[4], m[4], v[4];
        union { uint32_t raw; uint8_t e[4]; } cm, cv;
        cm.raw = 0; cv.raw = 0;
        if (full) {
            const float4 pv = *reinterpret_cast<const float4*>(a.p + e0);
            p[0] = pv.x; p[1] = pv.y; p[2] = pv.z; p[3] = pv.w;
            cm.raw = *reinterpret_cast<const uint32_t*>(q.m8 + e0);
            cv.raw = *reinterpret_cast<const uint32_t*>(q.v8 + e0);
            if constexpr (FLAT) {
                const float4 gv = *reinterpret_cast<const float4*>(a.g + e0);
                g[0] = gv.x; g[1] = gv.y; g[2] = gv.z; g[3] = gv.w;
            } else {
                union { uint2 raw; T e[4]; } gi;
                gi.raw = *reinterpret_cast<const uint2*>(g16 + e0);
#pragma unroll
                for (int j = 0; j < 4; ++j) g[j] = to_f32(gi.e[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = e0 + j < n;
                p[j] = ok ? a.p[e0 + j] : 0.f;
                cm.e[j] = ok ? q.m8[e0 + j] : 0;
                cv.e[j] = ok ? q.v8[e0 + j] : 0;
                if constexpr (FLAT) g[j] = ok ? a.g[e0 + j] : 0.f;
                else g[j] = ok ? to_f32(g16[e0 + j]) : 0.f;
            }
        }
        float mx_m = 0.f, mx_v = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            m[j] = s_code[0][cm.e[j]] * am;
            v[j] = s_code[1][cv.e[j]] * av;
            const int64_t e = e0 + j;
            const bool dec = e >= q.decay_begin && e < q.decay_end;
            adamw_one(p[j], g[j], m[j], v[j], dec ? a : a0);
            if (e < n) {                                            // (elements past n never reach the block's scale)
                mx_m = fmaxf(mx_m, fabsf(m[j]));
                mx_v = fmaxf(mx_v, v[j]);
            }
        }
        mx_m = wave_max(mx_m);
        mx_v = wave_max(mx_v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // a block whose new absmax is 0 stores the code of 0.0 (x = 0 finds it in either map) and decodes to exactly 0
            cm.e[j] = (uint8_t)adam8_encode(mx_m > 0.f ? m[j] / mx_m : 0.f, s_mids[0]);
            cv.e[j] = (uint8_t)adam8_encode(mx_v > 0.f ? v[j] / mx_v : 0.f, s_mids[1]);
        }
        if (lane == 0) {
            q.absmax_m[blk] = mx_m;
            q.absmax_v[blk] = mx_v;
        }
        if (full) {
            *reinterpret_cast<float4*>(a.p + e0) = float4{p[0], p[1], p[2], p[3]};
            *reinterpret_cast<uint32_t*>(q.m8 + e0) = cm.raw;
            *reinterpret_cast<uint32_t*>(q.v8 + e0) = cv.raw;
            if constexpr (FLAT) {
                if (a.zero_grad) *reinterpret_cast<float4*>(a.g + e0) = float4{0.f, 0.f, 0.f, 0.f};
            } else {
                union { uint2 raw; T e[4]; } po;
#pragma unroll
                for (int j = 0; j < 4; ++j) po.e[j] = from_f32<T>(p[j]);
                *reinterpret_cast<uint2*>(p16 + e0) = po.raw;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (e0 + j < n) {
                    a.p[e0 + j] = p[j];
                    q.m8[e0 + j] = cm.e[j];
                    q.v8[e0 + j] = cv.e[j];
                    if constexpr (FLAT) {
                        if (a.zero_grad) a.g[e0 + j] = 0.f;
                    } else {
                        p16[e0 + j] = from_f32<T>(p[j]);
                    }
                }
            }
        }
    }
}

// the scalars both 8-bit entry points share with the fp32 ones (formed in double, rounded once: see uamd_adamw_flat)
static void adam8_scalars(AdamArgs& a, double lr, double beta1, double beta2, double eps, double weight_decay,
                          double bias_correction1, double bias_correction2_sqrt, double grad_scale) {
    a.lr_wd = (float)(lr * weight_decay); a.b1 = (float)beta1; a.b2 = (float)beta2;
    a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2); a.eps = (float)eps;
    a.step_size = (float)(lr / bias_correction1); a.bc2_sqrt = (float)bias_correction2_sqrt;
    a.grad_scale = (float)grad_scale;
}

static unsigned adam8_grid(int64_t n) {
    int64_t blocks = (n + 4 * UAMD_ADAM8_BLOCK - 1) / (4 * UAMD_ADAM8_BLOCK);       // 4 quant blocks per workgroup
    if (blocks > 256 * 16) blocks = 256 * 16;                                        // 16 per CU, grid-stride beyond
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

static inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace

extern "C" int uamd_adamw8_flat(float* p, float* g, uint8_t* m8, uint8_t* v8, float* absmax_m, float* absmax_v,
                                const float* code_m, const float* code_v, int64_t n, double lr, double beta1, double beta2,
                                double eps, double weight_decay, double bias_correction1, double bias_correction2_sqrt,
                                double grad_scale, int zero_grad, void* stream) {
    if (!p || !g || !m8 || !v8 || !absmax_m || !absmax_v || !code_m || !code_v || n < 0) return UAMD_ERR_ARG;
    if (!(bias_correction1 > 0.0) || !(bias_correction2_sqrt > 0.0)) return UAMD_ERR_ARG;
    if (!aligned16(p) || !aligned16(g) || !aligned4(m8) || !aligned4(v8)) return UAMD_ERR_ALIGN;
    if (n == 0) return UAMD_OK;
    Adam8Args q;
    q.a.p = p; q.a.g = g; q.a.m = nullptr; q.a.v = nullptr; q.a.n = n; q.a.zero_grad = zero_grad;
    adam8_scalars(q.a, lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2_sqrt, grad_scale);
    q.m8 = m8; q.v8 = v8; q.absmax_m = absmax_m; q.absmax_v = absmax_v; q.code_m = code_m; q.code_v = code_v;
    q.decay_begin = 0; q.decay_end = n;
    hipLaunchKernelGGL((adamw8_kernel<float>), dim3(adam8_grid(n)), dim3(256), 0, (hipStream_t)stream, q,
                       (const float*)nullptr, (float*)nullptr);
    return uamd_launch_status();
}

extern "C" int uamd_adamw8_shard(float* p32, const void* g16, void* p16, uint8_t* m8, uint8_t* v8, float* absmax_m,
                                 float* absmax_v, const float* code_m, const float* code_v, int64_t n, int64_t decay_begin,
                                 int64_t decay_end, double lr, double beta1, double beta2, double eps, double weight_decay,
                                 double bias_correction1, double bias_correction2_sqrt, double grad_scale, int dtype,
                                 void* stream) {
    if (!p32 || !g16 || !p16 || !m8 || !v8 || !absmax_m || !absmax_v || !code_m || !code_v || n < 0) return UAMD_ERR_ARG;
    if (!(bias_correction1 > 0.0) || !(bias_correction2_sqrt > 0.0)) return UAMD_ERR_ARG;
    if (!aligned16(p32) || !aligned4(m8) || !aligned4(v8) || (reinterpret_cast<uintptr_t>(g16) & 7) ||
        (reinterpret_cast<uintptr_t>(p16) & 7))
        return UAMD_ERR_ALIGN;
    if (n == 0) return UAMD_OK;
    Adam8Args q;
    q.a.p = p32; q.a.g = nullptr; q.a.m = nullptr; q.a.v = nullptr; q.a.n = n; q.a.zero_grad = 0;
    adam8_scalars(q.a, lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2_sqrt, grad_scale);
    q.m8 = m8; q.v8 = v8; q.absmax_m = absmax_m; q.absmax_v = absmax_v; q.code_m = code_m; q.code_v = code_v;
    q.decay_begin = decay_begin; q.decay_end = decay_end;
    hipStream_t st = (hipStream_t)stream;
    UAMD_DISPATCH_HALF(dtype, hipLaunchKernelGGL((adamw8_kernel<T>), dim3(adam8_grid(n)), dim3(256), 0, st, q, (const T*)g16, (T*)p16))
    return uamd_launch_status();
}

extern "C" int uamd_adamw_shard(float* p32, const void* g16, void* p16, float* m, float* v, int64_t n, double lr,
                                double beta1, double beta2, double eps, double weight_decay, double bias_correction1,
                                double bias_correction2_sqrt, double grad_scale, int dtype, void* stream) {
    if (!p32 || !g16 || !p16 || !m || !v || n < 0) return UAMD_ERR_ARG;
    if (!(bias_correction1 > 0.0) || !(bias_correction2_sqrt > 0.0)) return UAMD_ERR_ARG;
    if (!aligned16(p32) || !aligned16(m) || !aligned16(v) || (reinterpret_cast<uintptr_t>(g16) & 7) ||
        (reinterpret_cast<uintptr_t>(p16) & 7))
        return UAMD_ERR_ALIGN;
    if (n == 0) return UAMD_OK;
    AdamArgs a;
    a.p = p32; a.g = nullptr; a.m = m; a.v = v; a.n = n;
    a.lr_wd = (float)(lr * weight_decay); a.b1 = (float)beta1; a.b2 = (float)beta2;
    a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2); a.eps = (float)eps;
    a.step_size = (float)(lr / bias_correction1); a.bc2_sqrt = (float)bias_correction2_sqrt;
    a.grad_scale = (float)grad_scale; a.zero_grad = 0;
    const int64_t n4 = (n + 3) >> 2;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    if (blocks < 1) blocks = 1;
    hipStream_t st = (hipStream_t)stream;
    UAMD_DISPATCH_HALF(dtype, hipLaunchKernelGGL((adamw_shard_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, st, a, (const T*)g16, (T*)p16))
    return uamd_launch_status();
}

extern "C" int uamd_adamw_flat(float* p, float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                               double eps, double weight_decay, double bias_correction1, double bias_correction2_sqrt,
                               double grad_scale, int zero_grad, void* stream) {
    if (!p || !g || !m || !v || n < 0) return UAMD_ERR_ARG;
    if (!(bias_correction1 > 0.0) || !(bias_correction2_sqrt > 0.0)) return UAMD_ERR_ARG;
    if (!aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v)) return UAMD_ERR_ALIGN;
    if (n == 0) return UAMD_OK;
    AdamArgs a;
    a.p = p; a.g = g; a.m = m; a.v = v; a.n = n;
    // hyper-parameters arrive as doubles (Python floats) and every derived constant is formed in double, then rounded
    // once -- like torch, whose kernels receive 1 - beta as a double-computed scalar (1.0f - 0.999f is off by 1.3e-5)
    a.lr_wd = (float)(lr * weight_decay); a.b1 = (float)beta1; a.b2 = (float)beta2;
    a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2); a.eps = (float)eps;
    a.step_size = (float)(lr / bias_correction1); a.bc2_sqrt = (float)bias_correction2_sqrt;
    a.grad_scale = (float)grad_scale; a.zero_grad = zero_grad;
    const int64_t n4 = (n + 3) >> 2;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;            // 16 blocks per CU, grid-stride beyond
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(adamw_flat_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return uamd_launch_status();
}
