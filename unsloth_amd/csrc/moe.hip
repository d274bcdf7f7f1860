// Mixture-of-experts expert block for gfx950: routing plan, ragged grouped GEMM with the permutation fused into its loads
// and stores, and the top-k combine.
//
// Replaces transformers' Qwen3MoeExperts.forward (modeling_qwen3_moe.py): a Python loop over the experts that were hit
// -- torch.where, F.linear, index_add_ per expert, a host sync per layer, the sum over the k slots of a token in 16 bits.
//
// Notation: T tokens, k experts per token, S = T k slots, slot f = t k + j (the flat index into top_k_index), E experts.
// "Sorted order" lists the slots expert by expert, ascending f inside an expert; rows[s] is the slot at sorted position s.
//
// Kernels here:
//   * moe_count_kernel / moe_scan_kernel / moe_rank_kernel: the plan. 256 slots per block; the per-(chunk, expert) counts
//     are integer LDS atomics (a count does not depend on arrival order), the rank of a slot inside its chunk is counted
//     from the ids themselves (the slots of the chunk with the same id and a lower index), so `rows` is stable and the same
//     on every run. One block then turns the counts into segment offsets and the row-tile map.
//   * moe_gemm_kernel<T, NN>: C[c_row(s)] (+)= row_scale(s) * (A[a_row(s)] @ op(W_e)) for every live row tile. The
//     128 x 128 x 64 tile, 4 waves (2 x 2), registers -> LDS staging, XOR swizzle and one barrier per K step of gemm.hip;
//     each thread computes its own four A source rows once (s, or rows[s] / k: the token's row feeds all of its k slots),
//     so the gather costs no extra instruction in the K loop. A tile never straddles two experts: a segment's last tile is
//     masked, rows past the segment's end are staged as zeros and never stored, and a wave whose 64-row half of the tile
//     is wholly past the end issues no LDS read and no MFMA (it only keeps the barriers).
//     NN form (W_e is [K, N], the backward's contraction over the weight's rows): the B tile is a [64 k][128 n] LDS image,
//     256 bytes per k-row, and the MFMA operand -- 8 consecutive k of one n per lane -- comes out of it through two
//     ds_read_b64_tr_b16. Bank swizzle: the 32-byte granule of a k-row is XORed with (k & 3) | ((k >> 3) & 1) << 2, so the
//     8 k-rows a 32-lane half of the transposing read touches fall into the 8 different granules of the 256-byte bank row.
//   * moe_combine_fwd_kernel / moe_combine_bwd_kernel: out[t] = sum_j w[t, j] Y[t k + j] in fp32 in j order, one rounding;
//     dw[t, j] = <dOut[t], Y[t k + j]> in fp32, one wave per slot, fixed order. No atomics.
//
// A slot whose id is outside [0, E) (HF's sentinel for a masked expert is id == E) is in no segment and no tile; its rows
// of the sorted and of the flat buffers are never written, and the combine kernels skip it by its id.
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((address_space(3))) s16x4_t lds_s16x4;

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = BM * BK * 2;          // 16 KiB per operand per stage
constexpr int SMEM_BYTES = 4 * TILE_BYTES;       // A, B x 2 stages = 64 KiB
constexpr int CHUNK = 256;                       // slots per block of the plan kernels
constexpr int MAX_E = 256;

// ------------------------------------------------------------------------------------------------------------ plan
__device__ __forceinline__ int load_id(const void* ids, int idx64, int64_t f) {
    if (idx64) {
        const int64_t v = reinterpret_cast<const int64_t*>(ids)[f];
        return (v >= 0 && v < MAX_E) ? (int)v : -1;
    }
    return reinterpret_cast<const int32_t*>(ids)[f];
}

// cnt[chunk][e] = slots of the chunk routed to e
__global__ void __launch_bounds__(CHUNK) moe_count_kernel(const void* ids, int idx64, int64_t S, int E, int32_t* cnt) {
    __shared__ int hist[MAX_E];
    const int tid = threadIdx.x;
    hist[tid] = 0;
    __syncthreads();
    const int64_t f = (int64_t)blockIdx.x * CHUNK + tid;
    if (f < S) {
        const int e = load_id(ids, idx64, f);
        if (e >= 0 && e < E) atomicAdd(&hist[e], 1);
    }
    __syncthreads();
    if (tid < E) cnt[(int64_t)blockIdx.x * E + tid] = hist[tid];
}

// One block. cnt[chunk][e] -> slots of e in the chunks before `chunk`; offsets[E + 1]; tiles = {live count, (expert, first
// sorted row) per row tile}.
__global__ void __launch_bounds__(MAX_E) moe_scan_kernel(int32_t* cnt, int nchunks, int E, int32_t* offsets, int32_t* tiles) {
    __shared__ int total[MAX_E], seg0[MAX_E], tile0[MAX_E];
    const int e = threadIdx.x;
    int run = 0;
    if (e < E)
        for (int c = 0; c < nchunks; ++c) {
            const int v = cnt[(int64_t)c * E + e];
            cnt[(int64_t)c * E + e] = run;
            run += v;
        }
    total[e] = run;
    __syncthreads();
    if (e == 0) {
        int s = 0, t = 0;
        for (int i = 0; i < E; ++i) {
            seg0[i] = s;
            tile0[i] = t;
            offsets[i] = s;
            s += total[i];
            t += (total[i] + BM - 1) / BM;
        }
        offsets[E] = s;
        tiles[0] = t;
    }
    __syncthreads();
    if (e < E)
        for (int i = 0, n = (run + BM - 1) / BM; i < n; ++i) {
            tiles[1 + 2 * (tile0[e] + i)] = e;
            tiles[2 + 2 * (tile0[e] + i)] = seg0[e] + i * BM;
        }
}

// rows[offsets[e] + (slots of e before the chunk) + (slots of e in the chunk below f)] = f
__global__ void __launch_bounds__(CHUNK) moe_rank_kernel(const void* ids, int idx64, int64_t S, int E, const int32_t* cnt,
                                                         const int32_t* offsets, int32_t* rows) {
    __shared__ int sid[CHUNK];
    const int tid = threadIdx.x;
    const int64_t f = (int64_t)blockIdx.x * CHUNK + tid;
    int e = -1;
    if (f < S) e = load_id(ids, idx64, f);
    if (e >= E) e = -1;
    sid[tid] = e;
    __syncthreads();
    if (e < 0) return;
    int rank = 0;
    for (int j = 0; j < tid; ++j) rank += sid[j] == e;
    rows[offsets[e] + cnt[(int64_t)blockIdx.x * E + e] + rank] = (int32_t)f;
}

// ------------------------------------------------------------------------------------------------------------ GEMM
template <typename T> struct Mfma;
template <> struct Mfma<bf16_t> {
    typedef bf16x8_t frag;
    static __device__ __forceinline__ f32x4_t run(frag a, frag b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <> struct Mfma<f16_t> {
    typedef f16x8_t frag;
    static __device__ __forceinline__ f32x4_t run(frag a, frag b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};

struct MoeGemmArgs {
    const void* A;
    const void* W;
    void* C;
    const int32_t* offsets;
    const int32_t* rows;
    const int32_t* tiles;
    const float* row_scale;
    int64_t lda, ldw, expert_stride, ldc;
    int N, K, topk, tiles_n;
    int gather_a, scatter_c, accumulate;
};

__device__ __forceinline__ int swz(int row, int slot) {      // byte offset inside a [128 rows][64 k] 16-bit tile
    return row * 128 + ((slot ^ ((row >> 1) & 7)) << 4);
}
__device__ __forceinline__ int nn_gran(int krow) { return (krow & 3) | (((krow >> 3) & 1) << 2); }
__device__ __forceinline__ int swz_nn(int krow, int slot) {  // byte offset inside a [64 k][128 n] 16-bit tile
    return krow * 256 + ((((slot >> 1) ^ nn_gran(krow)) << 5) | ((slot & 1) << 4));
}

template <typename T, bool NN>
__global__ void __launch_bounds__(256, 2) moe_gemm_kernel(MoeGemmArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typedef typename Mfma<T>::frag frag_t;
    // ---- block -> (row tile, n tile); n fastest, so the blocks of one A tile run together and the row tiles of one expert
    //      follow each other while its weights are still in cache. Tiles at or past the live count touch nothing.
    const int tile = blockIdx.x / p.tiles_n;
    if (tile >= p.tiles[0]) return;
    const int n0 = (blockIdx.x - tile * p.tiles_n) * BN;
    const int expert = p.tiles[1 + 2 * tile], s0 = p.tiles[2 + 2 * tile];
    const int nrows = min(BM, p.offsets[expert + 1] - s0);           // live rows of this tile, >= 1

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int N = p.N, K = p.K;
    const bool wave_live = wm * 64 < nrows;                           // wave-uniform

    // ---- this thread's four A source rows (tile rows (tid >> 3) + 32 i): NULL = past the segment's end, staged as zeros
    const T* a_src[4];
    const int kc = tid & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (tid >> 3) + i * 32;
        a_src[i] = nullptr;
        if (r < nrows) {
            const int64_t row = p.gather_a ? p.rows[s0 + r] / p.topk : s0 + r;
            a_src[i] = (const T*)p.A + row * p.lda + kc * 8;
        }
    }
    const T* Wg = (const T*)p.W + (int64_t)expert * p.expert_stride;

    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int nk = K / BK;                                            // host: K % 64 == 0
    uint4 ra[4], rb[4];
    auto load_tile = [&](int kt) {
        const int k0 = kt * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            ra[i] = a_src[i] ? *reinterpret_cast<const uint4*>(a_src[i] + k0) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + i * 256;
            if (NN) {                                                 // [64 k][128 n]: k-row c >> 4, 8 columns per slot
                const int krow = c >> 4, n = n0 + (c & 15) * 8;
                rb[i] = n < N ? *reinterpret_cast<const uint4*>(Wg + (int64_t)(k0 + krow) * p.ldw + n) : make_uint4(0, 0, 0, 0);
            } else {                                                  // [128 n][64 k]
                const int n = n0 + (c >> 3);
                rb[i] = n < N ? *reinterpret_cast<const uint4*>(Wg + (int64_t)n * p.ldw + k0 + kc * 8) : make_uint4(0, 0, 0, 0);
            }
        }
    };
    auto store_tile = [&](int buf) {
        unsigned char* sa = smem + buf * 2 * TILE_BYTES;
        unsigned char* sb = sa + TILE_BYTES;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + i * 256;
            *reinterpret_cast<uint4*>(sa + swz(c >> 3, kc)) = ra[i];
            *reinterpret_cast<uint4*>(sb + (NN ? swz_nn(c >> 4, c & 15) : swz(c >> 3, kc))) = rb[i];
        }
    };
    // NN fragment address: k-row ks * 32 + l4 * 8 + (l15 >> 2) (+ 4 for the second read), granule wn * 4 + j; the lane's own
    // address supplies columns 4 (l15 & 3) .. + 3 of that k-row, the transposing read hands back column l15 of four k-rows
    const int nn_f = (l15 >> 2) | ((l4 & 1) << 2);
    const int nn_lane = (l4 * 8 + (l15 >> 2)) * 256 + (l15 & 3) * 8;

    load_tile(0);
    store_tile(0);
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) load_tile(kt + 1);
        unsigned char* sa = smem + cur * 2 * TILE_BYTES;
        unsigned char* sb = sa + TILE_BYTES;
        if (wave_live) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                frag_t af[4], bf[4];
                const int slot = ks * 4 + l4;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    union { uint4 r; frag_t f; } u;
                    u.r = *reinterpret_cast<const uint4*>(sa + swz(wm * 64 + i * 16 + l15, slot));
                    af[i] = u.f;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (NN) {
                        union { s16x4_t h[2]; frag_t f; } u;
                        unsigned char* a0 = sb + ks * (32 * 256) + nn_lane + (((wn * 4 + j) ^ nn_f) << 5);
                        u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a0);
                        u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + 4 * 256));
                        bf[j] = u.f;
                    } else {
                        union { uint4 r; frag_t f; } u;
                        u.r = *reinterpret_cast<const uint4*>(sb + swz(wn * 64 + j * 16 + l15, slot));
                        bf[j] = u.f;
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = Mfma<T>::run(bf[j], af[i], acc[i][j]);
            }
        }
        if (kt + 1 < nk) store_tile(cur ^ 1);
        __syncthreads();
    }

    // ---- epilogue: lane holds C[m][n .. n + 3], m = wm * 64 + i * 16 + l15, n = n0 + wn * 64 + j * 16 + 4 l4. N % 8 == 0,
    //      so a quad is wholly inside or wholly outside N; ldc % 8 == 0 and C 16-byte aligned, so the store is one uint2.
    auto epi = [&](auto acc_c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = wm * 64 + i * 16 + l15;
            if (m >= nrows) continue;
            const int slot_f = (p.scatter_c || p.row_scale) ? p.rows[s0 + m] : 0;
            const float scale = p.row_scale ? p.row_scale[slot_f] : 1.0f;
            T* crow = (T*)p.C + (int64_t)(p.scatter_c ? slot_f : s0 + m) * p.ldc;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = n0 + wn * 64 + j * 16 + l4 * 4;
                if (n >= N) continue;
                union { uint2 raw; T e[4]; } o;
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r] * scale;
                if (decltype(acc_c)::value) {
                    o.raw = *reinterpret_cast<const uint2*>(crow + n);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] += to_f32(o.e[r]);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) o.e[r] = from_f32<T>(v[r]);
                *reinterpret_cast<uint2*>(crow + n) = o.raw;
            }
        }
    };
    if (p.accumulate) epi(std::integral_constant<bool, true>{});
    else epi(std::integral_constant<bool, false>{});
}

// ------------------------------------------------------------------------------------------------------------ combine
// One thread per 8 columns of a token: out[t, c .. c + 7] = sum_j w[t, j] * Y[t k + j, c .. c + 7], j ascending, fp32.
template <typename T>
__global__ void __launch_bounds__(256) moe_combine_fwd_kernel(const T* __restrict__ Y, int64_t ldy, const float* __restrict__ w,
                                                              const void* ids, int idx64, int E, T* __restrict__ out,
                                                              int64_t ldo, int64_t Tn, int k, int H) {
    const int hv = H >> 3;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= Tn * hv) return;
    const int64_t t = idx / hv;
    const int c = (int)(idx - t * hv) * 8;
    float acc[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = 0.f;
    for (int j = 0; j < k; ++j) {
        const int64_t f = t * k + j;
        if (ids) {
            const int e = load_id(ids, idx64, f);
            if (e < 0 || e >= E) continue;
        }
        const float wj = w ? w[f] : 1.0f;
        const Vec16<T> y = ld16(Y + f * ldy + c);
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r] += wj * to_f32(y.e[r]);
    }
    Vec16<T> o;
#pragma unroll
    for (int r = 0; r < 8; ++r) o.e[r] = from_f32<T>(acc[r]);
    st16(out + t * ldo + c, o);
}

// One wave per slot: dw[f] = <dOut[f / k], Y[f]>, lane partial sums over its columns ascending, then the wave sum.
template <typename T>
__global__ void __launch_bounds__(256) moe_combine_bwd_kernel(const T* __restrict__ dOut, int64_t ldd, const T* __restrict__ Y,
                                                              int64_t ldy, const void* ids, int idx64, int E,
                                                              float* __restrict__ dw, int64_t S, int k, int H) {
    const int lane = threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= S) return;
    bool live = true;
    if (ids) {
        const int e = load_id(ids, idx64, f);
        live = e >= 0 && e < E;
    }
    float acc = 0.f;
    if (live) {
        const T* d = dOut + (f / k) * ldd;
        const T* y = Y + f * ldy;
        for (int c = lane * 8; c < H; c += 64 * 8) {
            const Vec16<T> a = ld16(d + c), b = ld16(y + c);
#pragma unroll
            for (int r = 0; r < 8; ++r) acc += to_f32(a.e[r]) * to_f32(b.e[r]);
        }
        acc = wave_sum(acc);
    }
    if (lane == 0) dw[f] = acc;
}

template <typename T, bool NN>
int launch_moe_gemm(const MoeGemmArgs& a, int64_t blocks, hipStream_t st) {
    return uamd_launch_lds<&moe_gemm_kernel<T, NN>>(dim3((unsigned)blocks), dim3(256), SMEM_BYTES, st, a);
}

}  // namespace

// Upper bound of the row tiles of any routing of S slots over E experts (the live count is only known on the device).
extern "C" int64_t uamd_moe_max_tiles(int64_t S, int E) { return (S + BM - 1) / BM + E; }

extern "C" int64_t uamd_moe_plan_workspace(int64_t S, int E) { return ((S + CHUNK - 1) / CHUNK) * (int64_t)E; }

extern "C" int uamd_moe_plan(const void* top_k_index, int idx64, int64_t S, int E, int32_t* offsets, int32_t* rows,
                             int32_t* tiles, int32_t* ws, int64_t ws_elems, void* stream) {
    if (S <= 0 || S > 0x7fffffffLL || E < 1 || E > MAX_E || !top_k_index || !offsets || !rows || !tiles || !ws) return UAMD_ERR_ARG;
    if (ws_elems < uamd_moe_plan_workspace(S, E)) return UAMD_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int nchunks = (int)((S + CHUNK - 1) / CHUNK);
    hipLaunchKernelGGL(moe_count_kernel, dim3(nchunks), dim3(CHUNK), 0, st, top_k_index, idx64, S, E, ws);
    hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(MAX_E), 0, st, ws, nchunks, E, offsets, tiles);
    hipLaunchKernelGGL(moe_rank_kernel, dim3(nchunks), dim3(CHUNK), 0, st, top_k_index, idx64, S, E, (const int32_t*)ws,
                       (const int32_t*)offsets, rows);
    return uamd_launch_status();
}

extern "C" int uamd_moe_gemm(const void* A, int64_t lda, const void* W, int64_t ldw, int64_t expert_stride, void* C, int64_t ldc,
                             const int32_t* offsets, const int32_t* rows, const int32_t* tiles, const float* row_scale,
                             int64_t S, int E, int N, int K, int topk, int form_nn, int gather_a, int scatter_c, int accumulate,
                             int dtype, void* stream) {
    if (S <= 0 || S > 0x7fffffffLL || E < 1 || E > MAX_E || N <= 0 || K <= 0 || topk < 1 || !A || !W || !C || !offsets || !rows || !tiles)
        return UAMD_ERR_ARG;
    if ((K & 63) || (N & 7)) return UAMD_ERR_ARG;
    if ((lda & 7) || (ldw & 7) || (ldc & 7) || (expert_stride & 7) || !aligned16(A) || !aligned16(W) || !aligned16(C))
        return UAMD_ERR_ALIGN;
    MoeGemmArgs a;
    a.A = A; a.W = W; a.C = C; a.offsets = offsets; a.rows = rows; a.tiles = tiles; a.row_scale = row_scale;
    a.lda = lda; a.ldw = ldw; a.expert_stride = expert_stride; a.ldc = ldc;
    a.N = N; a.K = K; a.topk = topk; a.tiles_n = (N + BN - 1) / BN;
    a.gather_a = gather_a; a.scatter_c = scatter_c; a.accumulate = accumulate;
    const int64_t blocks = uamd_moe_max_tiles(S, E) * a.tiles_n;
    if (blocks > 0x7fffffffLL) return UAMD_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    UAMD_DISPATCH_HALF(dtype, return form_nn ? launch_moe_gemm<T, true>(a, blocks, st) : launch_moe_gemm<T, false>(a, blocks, st))
    return UAMD_ERR_DTYPE;
}

extern "C" int uamd_moe_combine_fwd(const void* Y, int64_t ldy, const float* w, const void* top_k_index, int idx64, int E,
                                    void* out, int64_t ld_out, int64_t T_, int k, int H, int dtype, void* stream) {
    if (T_ <= 0 || k < 1 || H <= 0 || (H & 7) || !Y || !out || T_ * k > 0x7fffffffLL) return UAMD_ERR_ARG;
    if ((ldy & 7) || (ld_out & 7) || !aligned16(Y) || !aligned16(out)) return UAMD_ERR_ALIGN;
    const int64_t blocks = (T_ * (H >> 3) + 255) / 256;
    if (blocks > 0x7fffffffLL) return UAMD_ERR_ARG;
    UAMD_DISPATCH_HALF(dtype, hipLaunchKernelGGL(moe_combine_fwd_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                                                 (const T*)Y, ldy, w, top_k_index, idx64, E, (T*)out, ld_out, T_, k, H))
    return uamd_launch_status();
}

extern "C" int uamd_moe_combine_bwd(const void* dOut, int64_t ld_dout, const void* Y, int64_t ldy, const void* top_k_index,
                                    int idx64, int E, float* dw, int64_t T_, int k, int H, int dtype, void* stream) {
    if (T_ <= 0 || k < 1 || H <= 0 || (H & 7) || !dOut || !Y || !dw || T_ * k > 0x7fffffffLL) return UAMD_ERR_ARG;
    if ((ld_dout & 7) || (ldy & 7) || !aligned16(dOut) || !aligned16(Y)) return UAMD_ERR_ALIGN;
    const int64_t S = T_ * k;
    UAMD_DISPATCH_HALF(dtype, hipLaunchKernelGGL(moe_combine_bwd_kernel<T>, dim3((unsigned)((S + 3) / 4)), dim3(256), 0,
                                                 (hipStream_t)stream, (const T*)dOut, ld_dout, (const T*)Y, ldy, top_k_index, idx64,
                                                 E, dw, S, k, H))
    return uamd_launch_status();
}
