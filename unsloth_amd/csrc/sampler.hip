// Next-token sampling of the decode step on the device: HF's warper chain temperature -> top-k -> top-p -> min-p and the draw,
// one launch (the reference: TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper, MinPLogitsWarper and
// torch.multinomial inside HF's generate, reached from unsloth_fast_generate, llama.py:2167-2259).
//
// Every filter is a threshold on the scaled logit z = x / T, so nothing is sorted: one 1024-thread workgroup per row finds
//   * the k-th largest z by radix selection over an order-preserving 32-bit key, 8 bits per pass (counts), and
//   * the nucleus edge by the same selection weighted with the probability masses,
// and then walks the CDF of the kept set in vocabulary order. Masses are 64-bit FIXED POINT (exp(z - z_max) * 2^45, at least
// 1; V <= 2^18 terms cannot overflow) and are only ever added as integers -- in LDS histograms (ds_add_u64), in registers
// and across lanes -- so every sum is exact and independent of the order of arrival: the same logits, parameters, seed, draw
// counter and row give the same token bit for bit. The only rounding is the expf of each element.
//
// Passes over the row (513 KB at V = 128,256, streamed from L2 after the first): 1 (maximum, first count digit) + 1 when top-k
// is on + 2 when top-p is on + 1 (kept mass per wave segment), then two short ones over 1/16 and 1/256 of the row for the walk;
// digits 2-4 of a selection work on the first digit's bin gathered into LDS (three more passes each only when that bin holds
// more than 16,384 entries).
// A histogram is 256 bins x 32 copies (copy = lane mod 32): logits crowd into a handful of exponent bins, and lanes of one
// wave adding to ONE LDS address serialise.
#include <math.h>

#include "common.h"

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int S_THREADS = 1024, S_WAVES = S_THREADS / UAMD_WAVE, S_BINS = 256, S_COPIES = 32;
constexpr int S_HIST_BYTES = S_BINS * S_COPIES * (int)sizeof(u64);
constexpr int S_CAND = S_HIST_BYTES / (int)sizeof(u32);   // keys of one first-digit bin that fit the histogram space
constexpr int S_MAX_V = 1 << 18;          // 2^18 masses of at most 2^45 sum below 2^64; the walk's last stage: V / 256 <= 1024
constexpr float S_FIX_ONE = 0x1p45f;
constexpr float S_U_MAX = 0x1.fffffep-1f;  // 1 - 2^-24

struct SampleArgs {
    const float* x;
    long long ld;
    int V;
    const uamd_sample_params* prm;
    const u64* ctr;
    const float* u_in;
    long long* out;
    int* kept_out;
    float* thresh_out;
    float* u_out;
};

// z = x / T (IEEE division, -0 folded into +0 so that equal values have equal keys); false for -inf, +inf and NaN
__device__ __forceinline__ bool scaled(float x, float T, float& z) {
    z = x / T;
    if (z == 0.f) z = 0.f;
    return fabsf(z) < INFINITY;
}
// order-preserving key of a finite float: a < b <=> key(a) < key(b); every finite key is above 0
__device__ __forceinline__ u32 okey(float z) {
    const u32 b = __float_as_uint(z);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key_value(u32 k) { return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k); }
// fixed-point mass of a finite z <= zmax: never 0, so every kept token can be drawn and u = 0 gives the first kept one
__device__ __forceinline__ u64 mass(float z, float zmax) {
    const u64 q = (u64)(expf(z - zmax) * S_FIX_ONE);
    return q ? q : 1ull;
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ u64 wave_scan_u64(u64 v, int lane) {          // inclusive
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// Philox4x32-10 (Salmon et al., Random123); returns the first output word
__device__ __forceinline__ u32 philox_x0(u32 c0, u32 c1, u32 c2, u32 c3, u32 k0, u32 k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const u32 hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const u32 hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// f(z) for every finite scaled logit of row[lo, hi), the elements dealt to `nt` threads (this one: t) as 16-byte vectors between a
// scalar head and tail (a row may start at any 4-byte address): a scalar loop keeps a quarter of the bytes in flight and is
// bound by the load latency
template <typename F>
__device__ __forceinline__ void for_each_z(const float* __restrict__ row, int lo, int hi, int t, int nt, float T, F&& f) {
    if (hi <= lo) return;
    auto one = [&](float x) {
        float z;
        if (scaled(x, T, z)) f(z);
    };
    const int head = min(hi - lo, (int)((4u - (u32)((reinterpret_cast<uintptr_t>(row + lo) >> 2) & 3u)) & 3u));
    if (t < head) one(row[lo + t]);
    const int b = lo + head, nvec = (hi - b) >> 2;
    const float4* v = reinterpret_cast<const float4*>(row + b);
#pragma unroll 4
    for (int j = t; j < nvec; j += nt) {
        const float4 q = v[j];
        one(q.x);
        one(q.y);
        one(q.z);
        one(q.w);
    }
    const int tb = b + 4 * nvec;
    if (t < hi - tb) one(row[tb + t]);
}

struct Sel { u64 above; int bin; };

// The bin b, scanning from the largest key down, with above(b) < target <= above(b) + tot[b], above(b) = `above` + the totals
// of the bins over b. Wave 0 works; sel->bin must be -1 on entry and stays -1 when no bin qualifies.
__device__ __forceinline__ void select_desc(const u64* tot, u64 above, u64 target, Sel* sel) {
    if (threadIdx.x >= UAMD_WAVE) return;
    const int lane = threadIdx.x;
    u64 v[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = tot[S_BINS - 1 - (4 * lane + j)]; sum += v[j]; }
    u64 run = above + wave_scan_u64(sum, lane) - sum;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (run < target && target <= run + v[j]) { sel->bin = S_BINS - 1 - (4 * lane + j); sel->above = run; }
        run += v[j];
    }
}

// Digits 2-4 of a selection without three more passes over the row: ONE pass gathers the keys of the first digit's bin
// (`prefix`) into LDS -- the histogram space, free between digits; a few hundred to a few thousand keys of 128,256 for logits
// of any spread -- and the three digits are selected from there (one histogram, `tot`: few entries, little contention; the mass
// of an entry is recomputed from its key, which IS z). False, with nothing changed, when the bin holds more than S_CAND keys
// (long runs of equal or near-equal logits): the caller then walks the row per digit.
template <bool MASS>
__device__ __forceinline__ bool select_in_lds(const float* __restrict__ row, int V, float T, float zmax, u32* cand, int* ncand,
                                              u64* tot, Sel* sel, u32& prefix, u64& above, u64 target) {
    const int tid = threadIdx.x;
    if (tid == 0) *ncand = 0;
    __syncthreads();
    const u32 first = prefix;
    for_each_z(row, 0, V, tid, S_THREADS, T, [&](float z) {
        const u32 key = okey(z);
        if ((key >> 24) != first) return;
        const int i = atomicAdd(ncand, 1);
        if (i < S_CAND) cand[i] = key;
    });
    __syncthreads();
    const int n = *ncand;
    if (n > S_CAND) return false;
    for (int shift = 16; shift >= 0; shift -= 8) {
        if (tid < S_BINS) tot[tid] = 0;
        __syncthreads();
        if (tid == 0) sel->bin = -1;
        for (int i = tid; i < n; i += S_THREADS) {
            const u32 key = cand[i];
            if ((key >> (shift + 8)) == prefix) atomicAdd(&tot[(key >> shift) & 255u], MASS ? mass(key_value(key), zmax) : 1ull);
        }
        __syncthreads();
        select_desc(tot, above, target, sel);
        __syncthreads();
        prefix = (prefix << 8) | (u32)(sel->bin & 255);   // (a bin always qualifies: target <= above + the bin's total)
        above = sel->above;
    }
    return true;
}

// tot[b] = sum of the copies of bin b (rotated start: the 32 lanes of a half-wave read 32 different banks)
template <typename H>
__device__ __forceinline__ void fold_copies(const H* hist, u64* tot) {
    if (threadIdx.x < S_BINS) {
        u64 s = 0;
        for (int c = 0; c < S_COPIES; ++c) s += hist[threadIdx.x * S_COPIES + ((c + threadIdx.x) & (S_COPIES - 1))];
        tot[threadIdx.x] = s;
    }
}

__global__ void __launch_bounds__(S_THREADS) sample_kernel(SampleArgs a) {
    extern __shared__ u64 hist64[];                       // [S_BINS][S_COPIES]; the count passes use it as u32
    u32* hist32 = reinterpret_cast<u32*>(hist64);
    __shared__ u64 tot[S_BINS];
    __shared__ u64 wsum[S_WAVES], wsum2[S_WAVES], wsum3[S_WAVES];
    __shared__ u32 wcnt[S_WAVES], wmin[S_WAVES];
    __shared__ float red[S_WAVES];
    __shared__ Sel sel;
    __shared__ int hit, ncand;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, copy = tid & (S_COPIES - 1);
    const int r = blockIdx.x, V = a.V;
    const float* row = a.x + (long long)r * a.ld;
    float T = a.prm->temperature;
    if (!(T > 0.f)) T = 1.f;
    const int k = a.prm->top_k;
    const float top_p = a.prm->top_p, min_p = a.prm->min_p;
    const bool topk_on = k > 0 && k < V, topp_on = top_p < 1.f;

    float u;
    if (a.u_in) {
        u = a.u_in[r];
    } else {
        const u64 seed = a.prm->seed, draw = a.ctr[0];
        u = (float)(philox_x0((u32)draw, (u32)(draw >> 32), (u32)r, 0u, (u32)seed, (u32)(seed >> 32)) >> 8) * 0x1p-24f;
    }
    if (!(u >= 0.f)) u = 0.f;
    if (u > S_U_MAX) u = S_U_MAX;

    // ---- pass 1: the maximum and, for top-k, the counts of the first digit ------------------------------------------------
    if (topk_on) {
        for (int i = tid; i < S_BINS * S_COPIES; i += S_THREADS) hist32[i] = 0;
        __syncthreads();
    }
    float m = -INFINITY;
    for_each_z(row, 0, V, tid, S_THREADS, T, [&](float z) {
        m = fmaxf(m, z);
        if (topk_on) atomicAdd(&hist32[(okey(z) >> 24) * S_COPIES + copy], 1u);
    });
    const float zmax = block_max<S_WAVES>(m, red);
    if (zmax == -INFINITY) {                              // nothing finite in the row
        if (tid == 0) {
            a.out[r] = 0;
            if (a.kept_out) a.kept_out[r] = 0;
            if (a.thresh_out) a.thresh_out[r] = NAN;
            if (a.u_out) a.u_out[r] = u;
        }
        return;
    }

    // ---- top-k: the key of the k-th largest z, four digits of counts ------------------------------------------------------
    u32 key_k = 0;
    if (topk_on) {
        u64 above = 0;
        u32 prefix = 0;
        bool found = true;
        for (int shift = 24; shift >= 0 && found; shift -= 8) {
            if (shift == 16 && select_in_lds<false>(row, V, T, zmax, hist32, &ncand, tot, &sel, prefix, above, (u64)k)) break;
            if (shift != 24) {
                for (int i = tid; i < S_BINS * S_COPIES; i += S_THREADS) hist32[i] = 0;
                __syncthreads();
                for_each_z(row, 0, V, tid, S_THREADS, T, [&](float z) {
                    const u32 key = okey(z);
                    if ((key >> (shift + 8)) == prefix) atomicAdd(&hist32[((key >> shift) & 255u) * S_COPIES + copy], 1u);
                });
                __syncthreads();
            }
            fold_copies(hist32, tot);
            if (tid == 0) sel.bin = -1;
            __syncthreads();
            select_desc(tot, above, (u64)k, &sel);
            __syncthreads();
            found = sel.bin >= 0;                         // false only in the first digit: fewer than k finite entries, all stay
            if (found) { prefix = (prefix << 8) | (u32)sel.bin; above = sel.above; }
        }
        if (found) key_k = prefix;
    }

    // ---- top-p over the top-k survivors: the smallest key whose mass strictly above it is below top_p * M, four digits of
    //      masses; M (the survivors' mass) comes out of the first of these passes --------------------------------------------
    u32 key_p = 0;
    if (topp_on) {
        u64 above = 0, target = 0;
        u32 prefix = 0;
        bool found = true;
        for (int shift = 24; shift >= 0 && found; shift -= 8) {
            if (shift == 16 && select_in_lds<true>(row, V, T, zmax, hist32, &ncand, tot, &sel, prefix, above, target)) break;
            for (int i = tid; i < S_BINS * S_COPIES; i += S_THREADS) hist64[i] = 0;
            __syncthreads();
            u64 mk = 0;
            for_each_z(row, 0, V, tid, S_THREADS, T, [&](float z) {
                const u32 key = okey(z);
                if (shift != 24 && (key >> (shift + 8)) != prefix) return;           // (the exp only for the digit's own entries)
                const u64 q = mass(z, zmax);
                if (shift == 24 && key >= key_k) mk += q;
                atomicAdd(&hist64[((key >> shift) & 255u) * S_COPIES + copy], q);
            });
            if (shift == 24) {
                mk = wave_sum_u64(mk);
                if (lane == 0) wsum[wave] = mk;
            }
            __syncthreads();
            fold_copies(hist64, tot);
            if (tid == 0) sel.bin = -1;
            __syncthreads();
            if (shift == 24) {
                u64 M = 0;
                for (int w = 0; w < S_WAVES; ++w) M += wsum[w];
                // a token goes iff the mass of the survivors at or below it is <= (1 - top_p) M: it stays iff the mass strictly
                // above it is < M - floor((1 - top_p) M); the largest z always stays
                const double d = (1.0 - (double)top_p) * (double)M;
                const u64 drop = d >= (double)M ? M : (u64)d;
                target = M - drop;
                if (target == 0) target = 1;
            }
            select_desc(tot, above, target, &sel);
            __syncthreads();
            found = sel.bin >= 0;
            if (found) { prefix = (prefix << 8) | (u32)sel.bin; above = sel.above; }
        }
        if (found) key_p = prefix;
    }

    // ---- min-p: p_i >= min_p * p_max <=> z_i >= z_max + ln(min_p) ---------------------------------------------------------
    u32 key_m = 0;
    if (min_p > 0.f) {
        float t = zmax + logf(fminf(min_p, 1.f));
        if (t == 0.f) t = 0.f;
        if (fabsf(t) < INFINITY) key_m = okey(t);
    }
    const u32 thr = max(key_k, max(key_p, key_m));

    // ---- the kept set: count, smallest member and mass, per wave segment of the vocabulary -------------------------------
    const int seg = (((V + S_WAVES - 1) / S_WAVES) + 63) & ~63;          // <= 16384
    const int sub = ((seg / S_WAVES) + 63) & ~63;                         // <= 1024
    {
        const int lo = wave * seg, hi = min(V, lo + seg);
        u64 s = 0;
        u32 c = 0, mn = 0xFFFFFFFFu;
        for_each_z(row, lo, hi, lane, UAMD_WAVE, T, [&](float z) {
            const u32 key = okey(z);
            if (key < thr) return;
            s += mass(z, zmax);
            ++c;
            mn = min(mn, key);
        });
        s = wave_sum_u64(s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            c += __shfl_xor(c, o, 64);
            mn = min(mn, (u32)__shfl_xor(mn, o, 64));
        }
        if (lane == 0) { wsum[wave] = s; wcnt[wave] = c; wmin[wave] = mn; }
        if (tid == 0) hit = -1;
    }
    __syncthreads();
    u64 W = 0;
    u32 kept = 0, minkey = 0xFFFFFFFFu;
    for (int w = 0; w < S_WAVES; ++w) { W += wsum[w]; kept += wcnt[w]; minkey = min(minkey, wmin[w]); }

    // ---- the draw: the smallest kept index whose inclusive prefix mass exceeds u W ---------------------------------------
    u64 target = (u64)((double)u * (double)W);
    if (target >= W) target = W - 1;                      // (W >= 1: the largest z is always kept)
    u64 P = 0;
    int ws = 0;
    for (; ws < S_WAVES - 1; ++ws) {
        if (target < P + wsum[ws]) break;
        P += wsum[ws];
    }
    const int base = ws * seg, end = min(V, base + seg);
    {
        const int lo = base + wave * sub, hi = min(end, lo + sub);
        u64 s = 0;
        for (int i = lo + lane; i < hi; i += 64) {
            float z;
            if (!scaled(row[i], T, z)) continue;
            if (okey(z) >= thr) s += mass(z, zmax);
        }
        s = wave_sum_u64(s);
        if (lane == 0) wsum2[wave] = s;
    }
    __syncthreads();
    int ss = 0;
    for (; ss < S_WAVES - 1; ++ss) {
        if (target < P + wsum2[ss]) break;
        P += wsum2[ss];
    }
    {
        const int i = base + ss * sub + tid;
        u64 q = 0;
        if (tid < sub && i < end) {
            float z;
            if (scaled(row[i], T, z) && okey(z) >= thr) q = mass(z, zmax);
        }
        const u64 incl = wave_scan_u64(q, lane);
        if (lane == 63) wsum3[wave] = incl;
        __syncthreads();
        u64 before = P;
        for (int w = 0; w < wave; ++w) before += wsum3[w];
        if (q && before + incl > target && before + incl - q <= target) hit = i;
    }
    __syncthreads();
    if (tid == 0) {
        a.out[r] = hit >= 0 ? hit : 0;
        if (a.kept_out) a.kept_out[r] = (int)kept;
        if (a.thresh_out) a.thresh_out[r] = key_value(minkey);
        if (a.u_out) a.u_out[r] = u;
    }
}

}  // namespace

extern "C" int uamd_sample_f32(const float* logits, int64_t ld, int rows, int V, const uamd_sample_params* params,
                               const uint64_t* ctr, const float* u_in, int64_t* out, int* kept_out, float* thresh_out,
                               float* u_out, void* stream) {
    if (!logits || !params || !out || (!ctr && !u_in) || rows <= 0 || V <= 0 || V > S_MAX_V || (ld != 0 && ld < V))
        return UAMD_ERR_ARG;
    SampleArgs a;
    a.x = logits;
    a.ld = (long long)ld;
    a.V = V;
    a.prm = params;
    a.ctr = (const u64*)ctr;
    a.u_in = u_in;
    a.out = (long long*)out;
    a.kept_out = kept_out;
    a.thresh_out = thresh_out;
    a.u_out = u_out;
    return uamd_launch_lds<sample_kernel>(dim3((unsigned)rows), dim3(S_THREADS), S_HIST_BYTES, (hipStream_t)stream, a);
}
