// Single-token decode kernels for gfx950: NF4 / 16-bit GEMV with the LoRA term, fused RoPE + KV-cache append, and
// split-KV ("flash decoding") GQA attention over the cache.
//
// Where they sit on the reference's path (decode): LlamaAttention_fast_forward_inference,
// fast_swiglu_inference and LlamaModel_fast_forward_inference (unsloth/models/llama.py:352-569, :572-606, :1249-1364),
// which run every linear of a one-token step through fast_linear_forward -> fast_gemv
// (unsloth/kernels/utils.py:1082-1125, :872-977: bitsandbytes' cgemm_4bit_inference_naive_{fp16,bf16} after a separate
// cdequantize_blockwise_fp32 launch for the nested absmax), RoPE as six in-place torch ops on temporaries
// (llama.py:468-490), the cache append as two permuted copies (:494-497) and attention as matmul / softmax / matmul
// over the whole cache (:533-543).
//
// All of it is HBM- and launch-bound (one token reads every weight once: 0.516 B/param NF4, 2 B/param 16-bit), so:
//   * GEMV: one wave owns whole output rows; a lane's 16-byte load covers 32 NF4 codes (8 dense elements) of the row and
//     always the SAME columns, so its slice of x stays in registers (packed 16-bit pairs) for every row the wave visits;
//     decode + multiply-accumulate is one LDS lookup and one v_dot2c_f32_{bf16,f16} per BYTE of NF4: the lookup table
//     maps a byte to its two decoded values as a packed pair, replicated 32 x in LDS so that lane l only ever touches
//     bank l % 32 (a 256-entry table hit with random indices would serialise 3-4 x on bank conflicts). The nested
//     absmax is decoded in the same kernel (no second launch), applied once per 32 codes in fp32; the LoRA term
//     s * B (A x) and the bias are folded into the wave reduction (lane r adds s * B[n][r] * t[r]). Several
//     projections that share x (q|k|v, gate|up) are ONE launch.
//   * RoPE + append: one launch rotates the new q and k (same arithmetic as the training kernel: fp32, one rounding)
//     and writes k, v at position kv_len[b] of the cache [B, Hk, S_max, D] -- positions come from DEVICE memory, so the
//     whole step is replayable as a hipGraph.
//   * attention: grid (split, kv head, batch); the G query heads of a KV head share every K / V row read; each split
//     keeps an online-softmax partial (m, l, o[D]) that a second tiny kernel combines. The split count is fixed at
//     capture time; splits past the current length exit immediately. n samples of one prompt (uamd_attn_decode_shared) keep
//     the prompt's K / V once: a prefix scan scores the n * G query rows of a (prompt, kv head) against one fetch of every
//     prompt key on the MFMA, the scan above runs over each row's own suffix, and the same kernel combines both.
#include "nf4_decode.h"

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
typedef __attribute__((ext_vector_type(4))) float rows_f32x4;

namespace {

template <typename T> struct Dot2;
template <> struct Dot2<bf16_t> {
    static __device__ __forceinline__ float run(uint32_t a, uint32_t b, float c) {
        union { uint32_t u; bf16x2_t v; } x, y;
        x.u = a; y.u = b;
        return __builtin_amdgcn_fdot2_f32_bf16(x.v, y.v, c, false);
    }
};
template <> struct Dot2<f16_t> {
    static __device__ __forceinline__ float run(uint32_t a, uint32_t b, float c) {
        union { uint32_t u; f16x2_t v; } x, y;
        x.u = a; y.u = b;
        return __builtin_amdgcn_fdot2(x.v, y.v, c, false);
    }
};

template <typename T>
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
    union { T h[2]; uint32_t u; } v;
    v.h[0] = from_f32<T>(lo);
    v.h[1] = from_f32<T>(hi);
    return v.u;
}

// Reductions on the VALU only (DPP), no LDS round trips: a ds_bpermute-based __shfl_xor costs ~100+ cycles of latency per
// step, and a decode step is nothing but latency. lanes_sum<16>: every lane ends with the sum over its 16-lane row
// (quad swaps, then the two mirror patterns pair each lane with the partial sum it is missing); lanes_sum<8> stops after
// row_half_mirror, where every lane holds the sum of its 8-lane half row.
#define UAMD_DPP_ADD(v, CTRL) ((v) + __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, (v)), (CTRL), 0xf, 0xf, true)))
template <int LANES>
__device__ __forceinline__ float lanes_sum(float v) {
    static_assert(LANES == 8 || LANES == 16, "half a DPP row or a whole one");
    v = UAMD_DPP_ADD(v, 0xb1);      // quad_perm [1,0,3,2]
    v = UAMD_DPP_ADD(v, 0x4e);      // quad_perm [2,3,0,1]
    v = UAMD_DPP_ADD(v, 0x141);     // row_half_mirror
    if constexpr (LANES == 16) v = UAMD_DPP_ADD(v, 0x140);     // row_mirror
    return v;
}
__device__ __forceinline__ float row16_sum(float v) { return lanes_sum<16>(v); }
__device__ __forceinline__ float wave_sum_dpp(float v) {            // wave-uniform total of all 64 lanes
    v = row16_sum(v);
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0)) +
           __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16)) +
           __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32)) +
           __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
}

// -DUAMD_DECODE_TRACE: s_memtime stamps at the phase boundaries of gemv_kernel and attn_decode_fused_kernel, 16 per wave
// (tools/decode_trace.py); never in the shipped library.
#ifdef UAMD_DECODE_TRACE
__device__ unsigned long long* g_dec_trace = nullptr;
#define DSTAMP(I)                                                                                  \
    do {                                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        dts[(I)] = __builtin_amdgcn_s_memtime();                                                   \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                         \
        __builtin_amdgcn_sched_barrier(0);                                                         \
    } while (0)
#define DTRACE_DECL unsigned long long dts[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, __builtin_amdgcn_s_memrealtime(), 0, 0}
#define DTRACE_FLUSH(NBLK_LINEAR, WAVES)                                                           \
    do {                                                                                           \
        if (g_dec_trace && (threadIdx.x & 63) == 0) {                                              \
            unsigned long long* d = g_dec_trace + ((size_t)(NBLK_LINEAR) * (WAVES) + (threadIdx.x >> 6)) * 16; \
            dts[14] = __builtin_amdgcn_s_memrealtime();      /* 100 MHz: calibrates the s_memtime ticks of dts[0..12] */ \
            dts[15] = 1ull + (__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)) & 0xf);    /* HW_REG_XCC_ID[3:0] */ \
            for (int i_ = 0; i_ < 16; ++i_) d[i_] = dts[i_];                                       \
        }                                                                                          \
    } while (0)
#else
#define DSTAMP(I) do { } while (0)
#define DTRACE_DECL do { } while (0)
#define DTRACE_FLUSH(A, B) do { } while (0)
#endif

#define UAMD_GEMV_MAX_GROUPS 4
struct GemvArgs {
    const void* x;
    int K, n_groups, bs_shift, total_rows;         // blocksize = 1 << bs_shift
    int n_tb;                                      // leading workgroups that compute t = A x (pro.a_rows) instead of weight rows
    // what the load phase needs of each group, apart from g[] so that the kernel fetches it as ONE batch of scalar loads:
    // hA = absmax_f32 (meta bit 8 set) or absmax_u8; meta = log2(blocksize2) | direct << 8 | lora_b_f32 << 9 | R << 16 (R = 0
    // without an adapter)
    const void* hW[UAMD_GEMV_MAX_GROUPS];
    const void* hA[UAMD_GEMV_MAX_GROUPS];
    const void* hA2[UAMD_GEMV_MAX_GROUPS];
    const void* hB[UAMD_GEMV_MAX_GROUPS];
    int64_t hldw[UAMD_GEMV_MAX_GROUPS];
    int hldb[UAMD_GEMV_MAX_GROUPS];
    int hmeta[UAMD_GEMV_MAX_GROUPS];
    int hN[UAMD_GEMV_MAX_GROUPS];
    // a wave's trip = RB adjacent rows of ONE group (a group's last trip may be short), so the group is chosen once per trip:
    // group g owns trips [trip_start[g], trip_start[g + 1]). glu: a trip is RB / 2 rows n of gate and up each.
    int trip_start[UAMD_GEMV_MAX_GROUPS + 1];
    int total_trips;
    int t_ks, t_kp;                                // t = A x: K parts per row (power of 2 <= 8), columns per part (multiple of 512)
    int row_start[UAMD_GEMV_MAX_GROUPS + 1];
    uamd_gemv_group g[UAMD_GEMV_MAX_GROUPS];
    uamd_gemv_prologue pro;                        // mode 0 / a_rows NULL = the plain kernel
};

// One block = 8 waves sharing the decode table and the token x in LDS; a wave takes RB ADJACENT rows per trip and
// issues every global load of the trip (weights, absmax codes) before anything else -- on the first trip even before
// the table is built -- so 4-8 KB per wave are in flight while the fixed costs are paid. NIT = iterations over K.
//
// t = A x of the LoRA factors inside the launch (pro.a_rows): the first n_tb workgroups take no weight rows; their waves
// compute the rows of t and publish each as ONE 8-byte store {fp32 value, tag} (device scope, so it is never torn and needs
// no fence). The tag is the CALLER's: a value no earlier launch on this workspace has used (pro.tag, a host counter, plus
// UAMD_TAG_STRIDE x *pro.tag_dev for launches replayed from a hipGraph -- the decode engine's step counter), so granules of
// earlier launches never match and nothing is cleared or counted between launches. (The first version took the tag from an
// epoch word that the launch's LAST workgroup advanced: an arrival counter on one word, 512 returning atomics = 6-10 us at
// the end of every gate|up / down launch, profiles/r04x_decode_phase_trace.txt.) A weight-row wave polls the granules once,
// after the dot products of its first rows (bounded spin; the producers wait for nobody, so they always get there).
constexpr int GEMV_THREADS = 512;
// Group fields: `p.g[gi].F` per ROW with a run-time gi made every access a scalar load whose ADDRESS waited for the previous one
// -- ~20 dependent round trips (2.5 us) stood between the kernel's entry and its first weight load
// (profiles/r04u_decode_phase_trace.txt). Now a trip belongs to ONE group: its fields are fetched once per trip from the h* arrays
// (independent scalar loads at a run-time index, one wait), and kept as integers so that the loads built on them are typed
// global (gptr) rather than flat.
#define OPQ(V) asm volatile("" : "+s"(V))          /* pin a wave-uniform value in scalar registers at this point */
// a 64-bit value as a GLOBAL pointer (an integer cast to a plain pointer is a flat address: flat_load, which also counts on
// lgkmcnt and drags a wait behind every row)
template <typename V> __device__ __forceinline__ const __attribute__((address_space(1))) V* gptr(uint64_t a) {
    return (const __attribute__((address_space(1))) V*)a;
}
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {          // a wave-uniform 64-bit value, pinned to scalar registers
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
template <typename T> __device__ __forceinline__ float bits16_to_f32(uint32_t b) {
    union { uint16_t u; T h; } v;
    v.u = (uint16_t)b;
    return to_f32(v.h);
}
template <typename T, bool NF4, int NIT, int RB>
__global__ void __launch_bounds__(GEMV_THREADS, NIT <= 16 ? 4 : 2) gemv_kernel(GemvArgs p) {     // <= 16: 2 blocks per CU
    constexpr int PAIRS = NF4 ? 16 : 4;              // 16-bit pairs of x per 16-byte weight load
    constexpr int ELEMS = 2 * PAIRS;                 // columns per lane per iteration
    extern __shared__ __attribute__((aligned(16))) unsigned char gemv_smem[];
    // layout: x [NIT * 64 * ELEMS] T | code2 [4][256] float | lut2 [256][32] u32 (NF4 only)
    T* xs = reinterpret_cast<T*>(gemv_smem);
    float* code2 = reinterpret_cast<float*>(gemv_smem + NIT * 64 * ELEMS * sizeof(T));
    uint32_t* lut2 = reinterpret_cast<uint32_t*>(code2 + UAMD_GEMV_MAX_GROUPS * 256);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    int K = p.K;
    OPQ(K);
    DTRACE_DECL;
    DSTAMP(0);
    {   // every 64-byte line of the ~0.9 KB kernarg segment in ONE batch of scalar loads: left to the compiler they are fetched
        // as they are needed, ~8 dependent scalar-cache misses in a row before the first weight load goes out
        const __attribute__((address_space(4))) int* ka =
            (const __attribute__((address_space(4))) int*)__builtin_amdgcn_kernarg_segment_ptr();
        int touch = 0;
#pragma unroll
        for (int o = 0; o < (int)sizeof(GemvArgs); o += 64) touch |= ka[o / 4];
        asm volatile("" ::"s"(touch));
    }
    DSTAMP(10);
    // columns past K: x is zero there, so the lane may read any valid address instead (no branches in the row loop)
    int koff[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        const int k0 = (i * 64 + lane) * ELEMS;
        koff[i] = k0 < K ? k0 : 0;
    }
    const int n_tb = p.n_tb;
    const bool t_block = (int)blockIdx.x < n_tb;
    const int nwaves = ((int)gridDim.x - n_tb) * (GEMV_THREADS / 64);
    // the launch's tag (see above): a host constant plus, under a hipGraph, a device counter the caller advances per replay
    // (the device half is loaded unconditionally from a valid address and only combined where the tag is first needed -- behind
    //  the first rows' dot products / the t row: a load in an `if` is waited for where the `if` ends, i.e. right here)
    const int* const tag_src = p.pro.tag_dev ? p.pro.tag_dev : reinterpret_cast<const int*>(p.hW[0]);
    const unsigned tag_raw = (unsigned)__builtin_nontemporal_load(tag_src);
    const unsigned tag_mul = p.pro.tag_dev ? UAMD_TAG_STRIDE : 0u;
#define UAMD_GEMV_TAG (p.pro.tag + tag_raw * tag_mul)
    int gis[RB], ns[RB];
    float direct[RB];                                // 1: single-level fp32 absmax, 0: nested
    uint4 w[RB][NIT];
    uint32_t a8[RB][NIT];
    float a2[RB][NIT];
    uint32_t braw[RB];                               // lane j: B[n][j] of the row's adapter (raw bits), loaded with the weights
    int n_groups = p.n_groups, glu = p.pro.glu, total_trips = p.total_trips, bs_shift = p.bs_shift;
    // every kernarg scalar the load phase uses, fetched HERE and pinned: left alone, the compiler re-loads them from the kernarg
    // segment where each row needs them -- ten scalar-cache round trips in a row inside load_rows (1.6 us of the 2.9 us between
    // a wave's entry and its last load going out, profiles/r04am_decode_phase_trace.txt)
    int ts1 = p.trip_start[1], ts2 = p.trip_start[2], ts3 = p.trip_start[3];
    uint64_t gW0 = (uint64_t)p.hW[0], gW1 = (uint64_t)p.hW[1], gB0 = (uint64_t)p.hB[0], gB1 = (uint64_t)p.hB[1];
    uint64_t gA0 = (uint64_t)p.hA[0], gA1 = (uint64_t)p.hA[1], gA20 = (uint64_t)p.hA2[0], gA21 = (uint64_t)p.hA2[1];
    int gM0 = p.hmeta[0], gM1 = p.hmeta[1], gL0 = p.hldb[0], gL1 = p.hldb[1], gN0 = p.hN[0];
    int64_t gD0 = p.hldw[0], gD1 = p.hldw[1];
    OPQ(n_groups); OPQ(glu); OPQ(total_trips); OPQ(bs_shift); OPQ(ts1); OPQ(ts2); OPQ(ts3);
    OPQ(gW0); OPQ(gW1); OPQ(gB0); OPQ(gB1); OPQ(gM0); OPQ(gM1); OPQ(gL0); OPQ(gL1); OPQ(gN0);
    if (NF4) { OPQ(gA0); OPQ(gA1); OPQ(gA20); OPQ(gA21); } else { OPQ(gD0); OPQ(gD1); }
    int t_gi = 0;                                    // the current trip's group (glu: row r belongs to group r & 1)
    bool valid[RB];
    auto load_rows = [&](int trip, int r_lo, int r_hi) {      // rows [r_lo, r_hi) of the trip (compile-time bounds after inlining)
        int gi = 0;
        if (1 < n_groups && trip >= ts1) gi = 1;
        if (2 < n_groups && trip >= ts2) gi = 2;
        if (3 < n_groups && trip >= ts3) gi = 3;
        t_gi = gi;
        // the trip's group, fetched ONCE: independent scalar loads at a run-time index, one wait for all of them
        // (glu: both groups, picked by the compile-time parity of r below)
        const int n0 = glu ? trip * (RB / 2) : (trip - p.trip_start[gi]) * RB;
        const uint64_t sW = (uint64_t)p.hW[gi], sB = (uint64_t)p.hB[gi];
        const int sMeta = p.hmeta[gi], sLdb = p.hldb[gi], sN = p.hN[gi];
        uint64_t sA = 0, sA2 = 0;
        int64_t sLdw = 0;
        if constexpr (NF4) { sA = (uint64_t)p.hA[gi]; sA2 = (uint64_t)p.hA2[gi]; } else { sLdw = p.hldw[gi]; }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            if (r < r_lo || r >= r_hi) continue;
            const int gr = r & 1;
            const uint64_t gW = glu ? (gr ? gW1 : gW0) : sW, gB = glu ? (gr ? gB1 : gB0) : sB;
            const int meta = glu ? (gr ? gM1 : gM0) : sMeta, ldb = glu ? (gr ? gL1 : gL0) : sLdb, Ng = glu ? gN0 : sN;
            const int nraw = glu ? n0 + (r >> 1) : n0 + r;
            valid[r] = nraw < Ng;
            // (readfirstlane: the row is wave-uniform by construction; said explicitly, its 64-bit products stay on the scalar unit
            //  even where the control flow around the lane-dependent B load would otherwise pull them into vector registers)
            const int nrow = __builtin_amdgcn_readfirstlane(min(nraw, Ng - 1));   // past the group's end: its last row again, not stored
            gis[r] = glu ? gr : gi;
            ns[r] = nrow;
            const bool dir = (meta >> 8) & 1;
            direct[r] = dir ? 1.f : 0.f;
            braw[r] = 0;
            // addresses: everything that depends on the ROW is wave-uniform (scalar unit, 64 bits); a lane adds a 32-bit byte
            // offset, so every load is `global_load ..., v_off, s[base]` (14 vector instructions per load before, 64-bit)
            if constexpr (NF4) {
                const uint64_t gA = glu ? (gr ? gA1 : gA0) : sA, gA2 = glu ? (gr ? gA21 : gA20) : sA2;
                const uint64_t rowbase = uniform64((uint64_t)nrow * (uint64_t)K);   // first code of the row (K % 32 == 0)
                const uint64_t wrow = uniform64(gW + (rowbase >> 1));
                const uint64_t blk_row = rowbase >> bs_shift;                        // first absmax block the row touches
                const uint32_t rem = (uint32_t)(rowbase - (blk_row << bs_shift));    // codes of that block before the row
                const uint64_t arow = uniform64(gA + blk_row * (dir ? 4u : 1u));
                const uint32_t bs2 = meta & 0xff;
#pragma unroll
                for (int i = 0; i < NIT; ++i) {
                    a8[r][i] = 0;
                    const uamd_u32x4 v = __builtin_nontemporal_load(gptr<uamd_u32x4>(wrow + (uint32_t)(koff[i] >> 1)));
                    w[r][i] = make_uint4(v[0], v[1], v[2], v[3]);
                    const uint32_t dblk = (rem + (uint32_t)koff[i]) >> bs_shift;    // absmax block relative to blk_row
                    if (dir) {
                        a2[r][i] = *gptr<float>(arow + dblk * 4u);
                    } else {
                        a8[r][i] = *gptr<uint8_t>(arow + dblk);
                        // nested: the fp32 absmax-of-absmax of block (blk_row + dblk) >> bs2; the uniform part again on the base
                        const uint64_t b2row = blk_row >> bs2;
                        const uint32_t rem2 = (uint32_t)(blk_row - (b2row << bs2));
                        a2[r][i] = *gptr<float>(uniform64(gA2 + b2row * 4u) + (((rem2 + dblk) >> bs2) << 2));
                    }
                }
            } else {
                const int64_t ldw = glu ? (gr ? gD1 : gD0) : sLdw;
                const uint64_t wrow = uniform64(gW + (uint64_t)((int64_t)nrow * ldw) * sizeof(T));
#pragma unroll
                for (int i = 0; i < NIT; ++i) {
                    a8[r][i] = 0;
                    a2[r][i] = 0.f;
                    const uamd_u32x4 v = *gptr<uamd_u32x4>(wrow + (uint32_t)(koff[i] * (int)sizeof(T)));
                    w[r][i] = make_uint4(v[0], v[1], v[2], v[3]);
                }
            }
            if (gB && lane < (meta >> 16)) {
                const bool f32 = (meta >> 9) & 1;
                const uint64_t brow = gB + (uint64_t)((int64_t)nrow * ldb) * (f32 ? 4u : 2u);
                if (f32) braw[r] = *gptr<uint32_t>(brow + (uint32_t)(lane * 4));
                else braw[r] = *gptr<uint16_t>(brow + (uint32_t)(lane * 2));
            }
        }
    };
    // ---- the prologue's own operands FIRST (the token / residual / norm weight vectors, the nested-absmax map): vmcnt retires
    //      loads in issue order, so behind 24 weight loads these few L2 hits waited for the whole HBM round trip and the block's
    //      set-up (staging, table, barrier) started when it should have been over (profiles/r04y_decode_phase_trace.txt)
    constexpr int VPT = (NIT * 64 * ELEMS / 8 + GEMV_THREADS - 1) / GEMV_THREADS;      // 16-byte vectors of x per thread
    const int mode = p.pro.mode;
    const T* const xp = (const T*)p.x;
    union V8 { uint4 r; T e[8]; };
    V8 pa[VPT], pb[VPT], pw[VPT];
    uint4 pwf[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
    float c2v[2] = {0.f, 0.f};
    const bool pre = mode == 0 || VPT == 1;              // operands in registers (mode 1 / 2 of longer rows: the LDS version below)
    const bool use_a = pre && xp != nullptr, use_b = pre && mode != 0, use_w = pre && mode == 2 && !p.pro.w_f32;
    {
        // BRANCH-FREE: a load inside `if (mode == ..)` has to be complete where the branches join, i.e. every arm ended in an
        // s_waitcnt and the weight loads below started a memory round trip late. Every vector is loaded from a valid address
        // (the real one, or element 0 of the weights when the mode has no such operand) and zeroed afterwards if unused.
        const T* const dummy = (const T*)p.hW[0];
        const bool use_wf = VPT == 1 && mode == 2 && p.pro.w_f32;
        const T* const src_a = use_a ? xp : dummy;
        const T* const src_b = use_b ? (mode == 1 ? (const T*)p.pro.x2 : (const T*)p.pro.res) : dummy;
        const T* const src_w = use_w ? (const T*)p.pro.norm_w : dummy;
        const float* const src_wf = use_wf ? (const float*)p.pro.norm_w : (const float*)dummy;
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
            const int v = tid + k * GEMV_THREADS;
            const bool in = v * 8 < K;                                                       // K % 8 == 0 (host)
            pa[k].r = *reinterpret_cast<const uint4*>(src_a + (use_a && in ? v * 8 : 0));
            pb[k].r = *reinterpret_cast<const uint4*>(src_b + (use_b && in ? v * 8 : 0));
            pw[k].r = *reinterpret_cast<const uint4*>(src_w + (use_w && in ? v * 8 : 0));
            if (VPT == 1) {
                pwf[0] = *reinterpret_cast<const uint4*>(src_wf + (use_wf && in ? v * 8 : 0));
                pwf[1] = *reinterpret_cast<const uint4*>(src_wf + (use_wf && in ? v * 8 + 4 : 0));
            }
        }
    }
    DSTAMP(11);
    if (NF4) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int i = tid + q * GEMV_THREADS;             // 4 groups x 256 entries
            const int gi = i >> 8;
            const float* c2 = gi == 0 ? p.g[0].code2 : gi == 1 ? p.g[1].code2 : gi == 2 ? p.g[2].code2 : p.g[3].code2;
            if (gi < p.n_groups && c2) c2v[q] = c2[i & 255];
        }
    }
    const float nf_hi = kNF4[(tid >> 4) & 15], nf_lo = kNF4[tid & 15];      // (constant MEMORY: two more loads that belong up here)
    DSTAMP(12);
    int trip = t_block ? total_trips : ((int)blockIdx.x - n_tb) * (GEMV_THREADS / 64) + wave_u;
    if (trip < total_trips) load_rows(trip, 0, RB);
    // t workgroups: wave (row r, part q of KS) of t = A x streams its <= 8 vectors of the A row NOW, with everything else of the
    // launch -- A does not depend on the token -- into the registers a weight-row wave uses for its weights
    const int KS = p.t_ks, Kp = p.t_kp;                    // parts per row (1, 2, 4, 8: adjacent waves of one block), columns per part
    const int t_wi = (int)blockIdx.x * (GEMV_THREADS / 64) + wave_u;
    const int t_r = t_wi / KS, t_q = t_wi - t_r * KS;
    const bool t_wave = t_block && p.pro.a_rows && t_r < p.pro.Rt;
    uint4* const wflat = &w[0][0];
    if (t_wave) {
        const T* arow = (const T*)p.pro.a_rows + (int64_t)t_r * p.pro.ld_a;
        const int k_end = min(K, (t_q + 1) * Kp);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k0 = t_q * Kp + (j * 64 + lane) * 8;
            wflat[j] = make_uint4(0, 0, 0, 0);
            if (k0 < k_end) wflat[j] = *reinterpret_cast<const uint4*>(arow + k0);
        }
    }
    DSTAMP(1);
    // ---- block setup while those loads fly: x (zero-padded; optionally PRODUCED here: SwiGLU of two vectors, or
    //      residual add + RMSNorm), t = A x of the LoRA factors, the nested-absmax maps, the byte -> value-pair table
    float* tl = reinterpret_cast<float*>(gemv_smem + NIT * 64 * ELEMS * sizeof(T) + UAMD_GEMV_MAX_GROUPS * 256 * 4 +
                                          (NF4 ? 256 * 32 * 4 : 0));          // [64 ranks x 4 groups] + 8 + 8 reduction slots
#pragma unroll
    for (int k = 0; k < VPT; ++k) {                        // operands a mode does not have, and vectors past K: zero (the loads above
        const int v = tid + k * GEMV_THREADS;              // were unconditional; their first USE is down here, behind the weights)
        const bool in = v * 8 < K;
        if (!(use_a && in)) pa[k].r = make_uint4(0, 0, 0, 0);
        if (!(use_b && in)) pb[k].r = make_uint4(0, 0, 0, 0);
        if (!(use_w && in)) pw[k].r = make_uint4(0, 0, 0, 0);
    }
    {
        const int nvec = NIT * 64 * ELEMS / 8;
        if (mode == 0) {
#pragma unroll
            for (int k = 0; k < VPT; ++k) {
                const int v = tid + k * GEMV_THREADS;
                if (v < nvec) reinterpret_cast<uint4*>(xs)[v] = pa[k].r;
            }
        } else if (mode == 1) {
            // x = (e * sigmoid(e)).to(T) * g: the SwiGLU of fast_swiglu_inference (llama.py:572-606), rounding points of
            // the training kernel (csrc/glu.hip); p.x = e (gate), pro.x2 = g (up)
            const T* gp = (const T*)p.pro.x2;
            for (int v = tid; v < nvec; v += GEMV_THREADS) {
                V8 a, b, o;
                o.r = make_uint4(0, 0, 0, 0);
                if (v * 8 < K) {
                    if (VPT == 1) {
                        a = pa[0];
                        b = pb[0];
                    } else {
                        a.r = *reinterpret_cast<const uint4*>(xp + v * 8);
                        b.r = *reinterpret_cast<const uint4*>(gp + v * 8);
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float e = to_f32(a.e[j]);
                        const float f = e * uamd_sigmoid(e);
                        o.e[j] = from_f32<T>(round_to<T>(f) * to_f32(b.e[j]));
                    }
                }
                reinterpret_cast<uint4*>(xs)[v] = o.r;
            }
        } else {
            // x = rmsnorm(h) * w, h = T(a + res) (a = p.x may be NULL: h = res): fast_rms_layernorm_inference after the
            // residual add of the decoder layer (llama.py:352-606), rounding points of csrc/rms_layernorm.hip. Every block
            // normalises the whole row for itself; block 0 also writes h (the next residual) to pro.h_out.
            const T* rp = (const T*)p.pro.res;
            T* hp = (T*)p.pro.h_out;
            if constexpr (VPT == 1) {            // K <= 4096 (NF4: the hidden size of every 7-8 B model): h and w stay in registers
                const int v = tid;
                V8 hv = pb[0];
                float ss = 0.f;
                if (v * 8 < K) {
                    if (xp) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) hv.e[j] = from_f32<T>(to_f32(pa[0].e[j]) + to_f32(hv.e[j]));
                    }
                    if (hp && blockIdx.x == 0) *reinterpret_cast<uint4*>(hp + v * 8) = hv.r;
#pragma unroll
                    for (int j = 0; j < 8; ++j) { const float f = to_f32(hv.e[j]); ss += f * f; }
                }
                ss = wave_sum_dpp(ss);
                if (lane == 0) tl[256 + wave_u] = ss;
                __syncthreads();
                float tot = 0.f;
#pragma unroll
                for (int w = 0; w < GEMV_THREADS / 64; ++w) tot += tl[256 + w];
                const float inv = rsqrtf(tot / (float)K + p.pro.eps);
                if (v < nvec) {
                    V8 o;
                    o.r = make_uint4(0, 0, 0, 0);
                    if (v * 8 < K) {
                        const float wfl[8] = {__uint_as_float(pwf[0].x), __uint_as_float(pwf[0].y), __uint_as_float(pwf[0].z),
                                              __uint_as_float(pwf[0].w), __uint_as_float(pwf[1].x), __uint_as_float(pwf[1].y),
                                              __uint_as_float(pwf[1].z), __uint_as_float(pwf[1].w)};
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const float normed = to_f32(hv.e[j]) * inv;
                            if (p.pro.w_f32) {
                                o.e[j] = from_f32<T>(normed * wfl[j]);
                            } else {                                    // (x * r).to(W.dtype) * W, product in W's dtype
                                o.e[j] = from_f32<T>(round_to<T>(round_to<T>(normed) * to_f32(pw[0].e[j])));
                            }
                        }
                    }
                    reinterpret_cast<uint4*>(xs)[v] = o.r;
                }
            } else {                             // longer rows: two passes over LDS (the register version costs an occupancy step)
                float ss = 0.f;
                for (int v = tid; v < nvec; v += GEMV_THREADS) {
                    V8 a, b;
                    b.r = make_uint4(0, 0, 0, 0);
                    if (v * 8 < K) {
                        b.r = *reinterpret_cast<const uint4*>(rp + v * 8);
                        if (xp) {
                            a.r = *reinterpret_cast<const uint4*>(xp + v * 8);
#pragma unroll
                            for (int j = 0; j < 8; ++j) b.e[j] = from_f32<T>(to_f32(a.e[j]) + to_f32(b.e[j]));
                        }
                        if (hp && blockIdx.x == 0) *reinterpret_cast<uint4*>(hp + v * 8) = b.r;
#pragma unroll
                        for (int j = 0; j < 8; ++j) { const float f = to_f32(b.e[j]); ss += f * f; }
                    }
                    reinterpret_cast<uint4*>(xs)[v] = b.r;                              // h for now
                }
                ss = wave_sum_dpp(ss);
                if (lane == 0) tl[256 + wave_u] = ss;
                __syncthreads();
                float tot = 0.f;
#pragma unroll
                for (int w = 0; w < GEMV_THREADS / 64; ++w) tot += tl[256 + w];
                const float inv = rsqrtf(tot / (float)K + p.pro.eps);
                for (int v = tid; v < nvec; v += GEMV_THREADS) {
                    if (v * 8 >= K) continue;
                    V8 h;
                    h.r = reinterpret_cast<uint4*>(xs)[v];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float normed = to_f32(h.e[j]) * inv;
                        if (p.pro.w_f32) {
                            h.e[j] = from_f32<T>(normed * ((const float*)p.pro.norm_w)[v * 8 + j]);
                        } else {                                        // (x * r).to(W.dtype) * W, product in W's dtype
                            h.e[j] = from_f32<T>(round_to<T>(round_to<T>(normed) * to_f32(((const T*)p.pro.norm_w)[v * 8 + j])));
                        }
                    }
                    reinterpret_cast<uint4*>(xs)[v] = h.r;
                }
            }
        }
        if (NF4) {
#pragma unroll
            for (int q = 0; q < 2; ++q) code2[tid + q * GEMV_THREADS] = c2v[q];
            if (tid < 256) {       // thread e builds entry e (high nibble = even element): 32 copies = 8 x 16 bytes
                const uint32_t v = pack2<T>(nf_hi, nf_lo);
                uint4* dst = reinterpret_cast<uint4*>(lut2 + tid * 32);
#pragma unroll
                for (int c = 0; c < 8; ++c) dst[c] = make_uint4(v, v, v, v);
            }
        }
    }
    DSTAMP(2);
    __syncthreads();
    DSTAMP(3);
    // ---- t = A x for the stacked LoRA A rows of the launch's projections ([Rt, K], activation dtype), by the first n_tb
    //      workgroups: (row, K part) per wave from the vectors loaded at entry, published as {value, tag}
    unsigned long long* gran = reinterpret_cast<unsigned long long*>(p.pro.sync);
    if (t_block && p.pro.a_rows) {
        float acc = 0.f;
        if (t_wave) {
            const int k_end = min(K, (t_q + 1) * Kp);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k0 = t_q * Kp + (j * 64 + lane) * 8;
                if (k0 < k_end) {
                    union { uint4 r; uint32_t w[4]; } av, xv;
                    av.r = wflat[j];
                    xv.r = *reinterpret_cast<const uint4*>(xs + k0);
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc = Dot2<T>::run(av.w[q], xv.w[q], acc);
                }
            }
            acc = wave_sum_dpp(acc);
        }
        if (KS > 1) {                                   // parts of a row -> its part-0 wave, through LDS, summed in part order
            if (lane == 0) tl[256 + 8 + wave_u] = acc;
            __syncthreads();
            if (t_wave && t_q == 0) {
                acc = 0.f;
                for (int q = 0; q < KS; ++q) acc += tl[256 + 8 + wave_u + q];
            }
        }
        DSTAMP(4);
        if (t_wave && t_q == 0 && lane == 0)
            __hip_atomic_store(gran + t_r, ((unsigned long long)UAMD_GEMV_TAG << 32) | (unsigned long long)__float_as_uint(acc),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    bool have_t = false;
    auto fetch_t = [&]() {                            // the launch's t into LDS (every wave for itself; identical values)
        const unsigned tag = UAMD_GEMV_TAG;
        for (int i = lane; i < p.pro.Rt; i += 64) {
            unsigned long long v = 0;
            bool ok = false;
            for (int spin = 0; spin < (1 << 18); ++spin) {
                v = __hip_atomic_load(gran + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok = (unsigned)(v >> 32) == tag;
                if (ok) break;
                __builtin_amdgcn_s_sleep(4);
            }
            tl[i] = ok ? __uint_as_float((unsigned)v) : __builtin_nanf("");
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    const uint32_t* lut_lane = lut2 + (lane & 31);
    const uint4* x_lane = reinterpret_cast<const uint4*>(xs) + lane * (PAIRS / 4);

    for (bool first = true; trip < total_trips; trip += nwaves, first = false) {
        // per-trip (glu: per-parity) fields of the compute phase: scalar selects, once
        const int cgi = t_gi;
        const float sOff = p.g[cgi].offset, sScale = p.g[cgi].lora_scale;
        const int sMeta = p.hmeta[cgi];
        const int sToff = p.pro.t_off[cgi];
        const float* sLt = p.g[cgi].lora_t;
        float acc[RB];
        int n_s[RB];
        bool v_s[RB];
        const bool more = trip + nwaves < total_trips;
        // the rows in two halves: the next trip's loads go out as soon as the registers of a half are free, i.e. half of them
        // have the other half's dot products to hide behind (they used to be issued after the whole trip)
        constexpr int HB = RB >= 2 ? RB / 2 : RB;
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int gr = r & 1;
            const float g_offset = glu ? p.g[gr].offset : sOff;
            acc[r] = 0.f;
#pragma unroll
            for (int i = 0; i < NIT; ++i) {
                const uint32_t ww[4] = {w[r][i].x, w[r][i].y, w[r][i].z, w[r][i].w};
                uint32_t xv[PAIRS];
#pragma unroll
                for (int q = 0; q < PAIRS / 4; ++q) {
                    const uint4 t4 = x_lane[i * 64 * (PAIRS / 4) + q];
                    xv[4 * q] = t4.x; xv[4 * q + 1] = t4.y; xv[4 * q + 2] = t4.z; xv[4 * q + 3] = t4.w;
                }
                if (NF4) {
                    // branch-free (a branch here splits the row into basic blocks and the dot products sink past all of them)
                    const float a_nested = code2[(glu ? gr : cgi) * 256 + a8[r][i]] * a2[r][i] + g_offset;
                    const float a = direct[r] * a2[r][i] + (1.f - direct[r]) * a_nested;       // direct is exactly 0 or 1
                    uint32_t dec[16];                        // all 16 table reads of the load first: one LDS latency, not 16
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int b = 0; b < 4; ++b) dec[4 * q + b] = lut_lane[((ww[q] >> (8 * b)) & 0xffu) * 32];
                    float l0 = 0.f, l1 = 0.f;
#pragma unroll
                    for (int j = 0; j < 16; j += 2) {
                        l0 = Dot2<T>::run(dec[j], xv[j], l0);
                        l1 = Dot2<T>::run(dec[j + 1], xv[j + 1], l1);
                    }
                    acc[r] += a * (l0 + l1);
                } else {
                    float l0 = Dot2<T>::run(ww[0], xv[0], 0.f), l1 = Dot2<T>::run(ww[1], xv[1], 0.f);
                    l0 = Dot2<T>::run(ww[2], xv[2], l0);
                    l1 = Dot2<T>::run(ww[3], xv[3], l1);
                    acc[r] += l0 + l1;
                }
                if (NIT > 2) __builtin_amdgcn_sched_barrier(0);    // keep the table / x reads of later iterations from piling up in registers
            }
            // LoRA: lane j adds s * B[n][j] * t[j]  (t = A x, fp32, from the preceding GEMV launch over the A rows)
            const int g_meta = glu ? p.hmeta[gr] : sMeta;
            const int g_R = g_meta >> 16;
            if (g_R > 0) {
                // t from the preceding launch (lora_t) or from this launch's t workgroups (pro.a_rows: rows t_off[g] ..)
                if (p.pro.a_rows && !have_t) { DSTAMP(5); fetch_t(); have_t = true; DSTAMP(6); }
                if (lane < g_R) {
                    const int toff = glu ? p.pro.t_off[gr] : sToff;
                    const float tv = p.pro.a_rows ? tl[toff + lane] : (glu ? p.g[gr].lora_t : sLt)[lane];
                    const float bv = ((g_meta >> 9) & 1) ? __uint_as_float(braw[r]) : bits16_to_f32<T>(braw[r]);
                    acc[r] += (glu ? p.g[gr].lora_scale : sScale) * bv * tv;
                }
            }
            n_s[r] = ns[r];
            v_s[r] = valid[r];
            if (more && (r + 1) % HB == 0) load_rows(trip + nwaves, r + 1 - HB, r + 1);
        }
        float tot[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) tot[r] = wave_sum_dpp(acc[r]);
        if (first) DSTAMP(7);
        if (lane == 0) {
            if (RB >= 2 && p.pro.glu) {
                // h[n] = (e * sigmoid(e)).to(T) * g with e, g rounded to T first: what uamd_swiglu_fg makes of the two stored rows
#pragma unroll
                for (int r = 0; r + 1 < RB; r += 2) {
                    if (!v_s[r]) break;
                    float e = tot[r], gg = tot[r + 1];
                    if (p.g[0].bias) e += to_f32(((const T*)p.g[0].bias)[n_s[r]]);
                    if (p.g[1].bias) gg += to_f32(((const T*)p.g[1].bias)[n_s[r]]);
                    e = round_to<T>(e);
                    gg = round_to<T>(gg);
                    // fp16: each of the two scalar products stays an fp32 value of its own on its way to the conversion (an empty
                    // asm, no instruction). hipcc otherwise folds product and conversion into v_fma_mixlo_f16 -- one rounding, and
                    // -0 + 0 = +0 inside the fma: h came out as +0 where uamd_swiglu_fg returns -0 (every e <= -17 or so). The note
                    // in front of fwd_one in glu.hip; tests/test_gpu_glu_sweep.py holds both SwiGLU sites of this file to that
                    // kernel's bits on every 16-bit e.
                    float f = e * uamd_sigmoid(e);
                    if constexpr (std::is_same<T, f16_t>::value) asm("" : "+v"(f));
                    float hv = round_to<T>(f) * gg;
                    if constexpr (std::is_same<T, f16_t>::value) asm("" : "+v"(hv));
                    ((T*)p.g[0].y)[n_s[r]] = from_f32<T>(hv);
                }
            } else {
                const void* gb = p.g[cgi].bias;
                void* gy = p.g[cgi].y;
                const int yf = p.g[cgi].y_f32;
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    if (!v_s[r]) break;
                    float v = tot[r];
                    if (gb) v += to_f32(((const T*)gb)[n_s[r]]);
                    if (yf) ((float*)gy)[n_s[r]] = v;
                    else ((T*)gy)[n_s[r]] = from_f32<T>(v);
                }
            }
        }
    }
    DSTAMP(8);
    DSTAMP(9);
    DTRACE_FLUSH(blockIdx.x, GEMV_THREADS / 64);
}

template <typename T, bool NF4, int NIT, int RB>
int launch_gemv_n(const GemvArgs& a0, hipStream_t st) {
    constexpr int ELEMS = NF4 ? 32 : 8;
    const int lds = NIT * 64 * ELEMS * (int)sizeof(T) + UAMD_GEMV_MAX_GROUPS * 256 * 4 + (NF4 ? 256 * 32 * 4 : 0) + (256 + 16) * 4;
    if (lds > 48 * 1024)
        if (int rc = uamd_lds_optin<&gemv_kernel<T, NF4, NIT, RB>>(lds)) return rc;
    if (a0.pro.glu && RB < 2) return UAMD_ERR_ARG;                // a wave needs the gate row and the up row in one trip
    GemvArgs a = a0;
    int trips = 0;
    for (int i = 0; i < UAMD_GEMV_MAX_GROUPS; ++i) {
        a.trip_start[i] = trips;
        if (i < a.n_groups && !a.pro.glu) trips += (a.hN[i] + RB - 1) / RB;
    }
    if (a.pro.glu) trips = (a.hN[0] + RB / 2 - 1) / (RB / 2 > 0 ? RB / 2 : 1);
    a.trip_start[UAMD_GEMV_MAX_GROUPS] = trips;
    a.total_trips = trips;
    int blocks = (trips + GEMV_THREADS / 64 - 1) / (GEMV_THREADS / 64);     // one trip per wave until the chip is full
    if (blocks > 512 - a.n_tb) blocks = 512 - a.n_tb;             // 2 blocks (16 waves) per CU, the t workgroups included: a 513th
    if (blocks < 1) blocks = 1;                                   // block starts when another one ends, i.e. costs a whole round
    hipLaunchKernelGGL((gemv_kernel<T, NF4, NIT, RB>), dim3(blocks + a.n_tb), dim3(GEMV_THREADS), lds, st, a);
    return uamd_launch_status();
}

template <typename T, bool NF4>
int launch_gemv(const GemvArgs& a, hipStream_t st) {
    constexpr int ELEMS = NF4 ? 32 : 8;
    const int nit = (a.K + 64 * ELEMS - 1) / (64 * ELEMS);
    if constexpr (NF4) {                             // K <= 4096 | 8192 | 16384
        if (nit <= 2) return launch_gemv_n<T, true, 2, 4>(a, st);
        if (nit <= 4) return launch_gemv_n<T, true, 4, 2>(a, st);
        if (nit <= 8) return launch_gemv_n<T, true, 8, 1>(a, st);
    } else {                                         // K <= 4096 | 8192 | 16384
        if (nit <= 8) return launch_gemv_n<T, false, 8, 2>(a, st);
        if (nit <= 16) return launch_gemv_n<T, false, 16, 1>(a, st);
        if (nit <= 32) return launch_gemv_n<T, false, 32, 1>(a, st);
    }
    return UAMD_ERR_ARG;                             // larger K: the caller splits it
}

// ---------------------------------------------------------------------------------------------------------------
// uamd_gemv_rows: the GEMV for M = 1 .. 16 token rows that share ONE pass over the weights (a decode step of a batch).
//
//   * v_mfma_f32_16x16x32: the A operand is 16 weight rows, the B operand the token rows (rows >= M are zero fragments), the
//     accumulator D[n][m] fp32. Lane l feeds row l & 15 of both operands at the 8 k slots of quad l >> 4; the order in which
//     columns meet the slots is free as long as both operands agree, so a lane's 16-byte weight load -- 32 consecutive NF4
//     codes of one row inside one absmax block, or 8 dense elements -- goes straight from memory into fragments: no LDS
//     round trip for the weights.
//   * NF4: byte -> packed pair of levels through the GEMV's bank-replicated table, times the block's absmax in fp32, rounded
//     once to T (an MFMA sums over the four quads, i.e. over two absmax blocks: the scale cannot wait for the accumulator).
//   * One workgroup = 8 waves = RT adjacent 16-row tiles of one group. The waves split K: wave w takes the 128-column
//     chunks w, w + 8, ..., so the eight of them read 512 contiguous bytes of a row side by side, and a wave's X fragments
//     serve its RT tiles. Loads run one stage (a chunk of every tile) ahead of the MFMAs.
//   * The eight partial tiles meet in LDS and are summed in wave order 0 .. 7: the value of Y[m][n] is a fixed sequence of
//     operations on row m and weight row n alone -- it depends neither on M, nor on m, nor on the other token rows, nor on RT
//     (the MFMA computes each D element from its own A row and B column). A NaN in one token row stays in its column of D.
//   * The epilogue (all 512 threads, one output each per pass) adds the LoRA term s * B[n, :] . t[m, :] (t fp32, from an
//     earlier launch over the stacked A rows) and the bias, and stores to y + m * ldy + n.
//   * uamd_gemv_rows64, M = 17 .. 64: MT = 2 | 4 token tiles of 16 rows. Every weight fragment is decoded once and feeds MT
//     MFMAs against MT token fragments into acc[RT][MT]; chunk-to-wave assignment, MFMA order per accumulator, the wave-order
//     sum and the epilogue are those of MT = 1, so Y[m][n] has the bits the 16-row launch gives that token row -- it does
//     not depend on MT either. Registers: two stages of 16 MT token-fragment registers are not to be had (MT = 4: 128), so
//     only the weights are double-buffered and ONE set of token fragments is requested right before the next stage's
//     weights; the widest instances (RT MT >= 8: 64 accumulator + 64 fragment registers, up to 221 VGPRs, 64 - 128 KiB of
//     partial tiles) take one workgroup per CU rather than spill -- none uses scratch (tests/test_decode_batch64_host.py).
//     The MT = 1 instances are the code they were (profiles/rows64_mt1_device_asm_diff.txt).
constexpr int ROWS_THREADS = 512, ROWS_WAVES = ROWS_THREADS / 64, ROWS_CHUNK = 128;
struct GemvRowsArgs {
    const void* x;
    int64_t ldx, ldy, ldt;
    int M, K, n_groups, bs_shift;
    int blk_start[UAMD_GEMV_MAX_GROUPS + 1];       // group g owns workgroups [blk_start[g], blk_start[g + 1])
    uamd_gemv_group g[UAMD_GEMV_MAX_GROUPS];       // (blocksize2 as a shift)
};

template <typename T> struct RowsMfma;
template <> struct RowsMfma<bf16_t> {
    typedef __attribute__((ext_vector_type(8))) __bf16 frag;
    static __device__ __forceinline__ rows_f32x4 run(frag a, frag b, rows_f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <> struct RowsMfma<f16_t> {
    typedef __attribute__((ext_vector_type(8))) _Float16 frag;
    static __device__ __forceinline__ rows_f32x4 run(frag a, frag b, rows_f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};

template <typename T, bool NF4, int RT, int MT>
__global__ void __launch_bounds__(ROWS_THREADS) gemv_rows_kernel(GemvRowsArgs p) {
    typedef typename RowsMfma<T>::frag frag;
    constexpr int WV = NF4 ? 1 : 4;                  // 16-byte weight loads per lane, tile and chunk
    extern __shared__ __attribute__((aligned(16))) unsigned char rows_smem[];
    // layout: code2 [256] float | lut2 [256][32] u32 (NF4); after the K loop the partial tiles [8][RT][MT][64] x 16 bytes from 0
    float* code2 = reinterpret_cast<float*>(rows_smem);
    uint32_t* lut2 = reinterpret_cast<uint32_t*>(rows_smem + 1024);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int K = p.K, M = p.M;
    int gi = 0;
    if (1 < p.n_groups && (int)blockIdx.x >= p.blk_start[1]) gi = 1;
    if (2 < p.n_groups && (int)blockIdx.x >= p.blk_start[2]) gi = 2;
    if (3 < p.n_groups && (int)blockIdx.x >= p.blk_start[3]) gi = 3;
    const uamd_gemv_group& g = p.g[gi];
    const int N = g.N;
    const int n0 = ((int)blockIdx.x - p.blk_start[gi]) * 16 * RT;
    const bool dir = NF4 && g.absmax_f32 != nullptr;
    if (NF4 && tid < 256) {
        code2[tid] = (!dir && g.code2) ? g.code2[tid] : 0.f;
        const uint32_t v = pack2<T>(kNF4[tid >> 4], kNF4[tid & 15]);       // high nibble = even element
        uint4* dst = reinterpret_cast<uint4*>(lut2 + tid * 32);
#pragma unroll
        for (int c = 0; c < 8; ++c) dst[c] = make_uint4(v, v, v, v);
    }
    // a lane's rows: weight row n0 + 16 t + r of tile t (past the group's end: its last row again, never stored) and token row
    // 16 u + r of token tile u (rows >= M: row 0's address, the fragment zeroed -- such rows are not read)
    bool mok[MT];
    const T* xrow[MT];
#pragma unroll
    for (int u = 0; u < MT; ++u) {
        mok[u] = 16 * u + r < M;
        xrow[u] = (const T*)p.x + (int64_t)(mok[u] ? 16 * u + r : 0) * p.ldx;
    }
    int64_t wrow[RT];                                // NF4: first code of the row; dense: first element
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        const int n = min(n0 + 16 * t + r, N - 1);
        wrow[t] = (int64_t)n * (NF4 ? (int64_t)K : g.ldw);
    }
    // nested or single-level absmax without a branch in the loop: the byte load of the single-level case reads the weights
    const uint8_t* const pa8 = dir ? (const uint8_t*)g.W : g.absmax_u8;
    const float* const pa2 = dir ? g.absmax_f32 : g.absmax2;
    const int sh2 = dir ? 0 : g.blocksize2;
    const float offset = g.offset;
    const int nch = (K + ROWS_CHUNK - 1) / ROWS_CHUNK;
    auto col_of = [&](int c, int j) { return NF4 ? c * ROWS_CHUNK + q * 32 + j * 8 : c * ROWS_CHUNK + j * 32 + q * 8; };

    struct Stage {
        uint4 w[RT][WV];
        uint32_t a8[RT];
        float a2[RT];
        uint4 x[4];                                  // (MT = 1 only)
    };
    // The token fragments of a chunk. One token tile: they travel with the chunk's weights, a stage ahead. More tiles: 16 MT
    // registers a stage are not to be had twice, so ONE set is loaded (from L2: all workgroups read the same X) right before
    // the next stage's weights are requested -- the wait for it leaves those in flight -- and serves the RT weight tiles.
    struct XFrags { uint4 x[MT][4]; };
    auto load_x = [&](XFrags& f, int c) {
#pragma unroll
        for (int u = 0; u < MT; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = col_of(c, j);
                f.x[u][j] = *reinterpret_cast<const uint4*>(xrow[u] + (col < K ? col : 0));
            }
    };
    auto load = [&](Stage& s, int c) {
        if constexpr (MT == 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = col_of(c, j);
                s.x[j] = *reinterpret_cast<const uint4*>(xrow[0] + (col < K ? col : 0));
            }
        }
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            if constexpr (NF4) {
                const int col = col_of(c, 0);
                const int64_t e = wrow[t] + (col < K ? col : 0);
                const uamd_u32x4 v = __builtin_nontemporal_load(
                    reinterpret_cast<const uamd_u32x4*>((const uint8_t*)g.W + (e >> 1)));
                s.w[t][0] = make_uint4(v[0], v[1], v[2], v[3]);
                const int64_t blk = e >> p.bs_shift;
                s.a8[t] = pa8[blk];
                s.a2[t] = pa2[blk >> sh2];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int col = col_of(c, j);
                    const uamd_u32x4 v = __builtin_nontemporal_load(
                        reinterpret_cast<const uamd_u32x4*>((const T*)g.W + wrow[t] + (col < K ? col : 0)));
                    s.w[t][j] = make_uint4(v[0], v[1], v[2], v[3]);
                }
                s.a8[t] = 0;
                s.a2[t] = 0.f;
            }
        }
    };
    rows_f32x4 acc[RT][MT];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int u = 0; u < MT; ++u) acc[t][u] = rows_f32x4{0.f, 0.f, 0.f, 0.f};
    const uint32_t* const lut_lane = lut2 + (lane & 31);
    union F { uint4 u; uint32_t w[4]; frag f; };
    XFrags xf;                                       // (MT > 1)
    auto compute = [&](const Stage& s, int c) {
        F xb[MT][4];
        bool in[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            in[j] = col_of(c, j) < K;
            if constexpr (MT == 1) {
                xb[0][j].u = (mok[0] && in[j]) ? s.x[j] : make_uint4(0, 0, 0, 0);
            } else {
#pragma unroll
                for (int u = 0; u < MT; ++u) xb[u][j].u = (mok[u] && in[j]) ? xf.x[u][j] : make_uint4(0, 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            if constexpr (NF4) {
                // columns past K: the weights are a real row's (finite values), the token fragment is zero
                const float am = dir ? s.a2[t] : code2[s.a8[t]] * s.a2[t] + offset;
                const uint32_t ww[4] = {s.w[t][0].x, s.w[t][0].y, s.w[t][0].z, s.w[t][0].w};
                uint32_t dec[16];                            // all 16 table reads first: one LDS latency, not 16
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int b = 0; b < 4; ++b) dec[4 * j + b] = lut_lane[((ww[j] >> (8 * b)) & 0xffu) * 32];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    F a;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const uint32_t pr = dec[4 * j + b];
                        a.w[b] = pack2<T>(bits16_to_f32<T>(pr & 0xffffu) * am, bits16_to_f32<T>(pr >> 16) * am);
                    }
#pragma unroll
                    for (int u = 0; u < MT; ++u) acc[t][u] = RowsMfma<T>::run(a.f, xb[u][j].f, acc[t][u]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    F a;                                     // columns past K: zero (the bits read there may be a NaN's)
                    a.u = in[j] ? s.w[t][j] : make_uint4(0, 0, 0, 0);
#pragma unroll
                    for (int u = 0; u < MT; ++u) acc[t][u] = RowsMfma<T>::run(a.f, xb[u][j].f, acc[t][u]);
                }
            }
        }
    };
    Stage s0, s1;
    int c = wave;
    if (c < nch) load(s0, c);
    if (NF4) __syncthreads();                        // the tables
    for (; c < nch; c += 2 * ROWS_WAVES) {
        const bool more = c + ROWS_WAVES < nch;
        if constexpr (MT > 1) load_x(xf, c);
        if (more) load(s1, c + ROWS_WAVES);
        compute(s0, c);
        if (more) {
            if constexpr (MT > 1) load_x(xf, c + ROWS_WAVES);
            if (c + 2 * ROWS_WAVES < nch) load(s0, c + 2 * ROWS_WAVES);
            compute(s1, c + ROWS_WAVES);
        }
    }
    // ---- the eight partial tiles -> LDS -> summed in wave order
    __syncthreads();                                 // (the tables are dead)
    rows_f32x4* red = reinterpret_cast<rows_f32x4*>(rows_smem);
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int u = 0; u < MT; ++u) red[((wave * RT + t) * MT + u) * 64 + lane] = acc[t][u];
    __syncthreads();
    const float* redf = reinterpret_cast<const float*>(rows_smem);
    const int R = g.lora_b ? g.R : 0;
    for (int o = tid; o < RT * MT * 256; o += ROWS_THREADS) {
        const int nl = o & 15, mc = (o >> 4) & 15, tu = o >> 8;      // tu = t * MT + u
        const int m = 16 * (tu % MT) + mc;
        const int n = n0 + 16 * (tu / MT) + nl;
        if (m >= M || n >= N) continue;
        const int src = ((nl >> 2) * 16 + mc) * 4 + (nl & 3);       // D[row nl][col mc]: lane (nl / 4) * 16 + mc, register nl % 4
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < ROWS_WAVES; ++w) v += redf[(w * RT * MT + tu) * 256 + src];
        if (R > 0) {
            const float* tv = g.lora_t + (int64_t)m * p.ldt;
            float l = 0.f;
            if (g.lora_b_f32) {
                const float* bv = (const float*)g.lora_b + (int64_t)n * g.ld_lb;
                for (int j = 0; j < R; ++j) l += bv[j] * tv[j];
            } else {
                const T* bv = (const T*)g.lora_b + (int64_t)n * g.ld_lb;
                for (int j = 0; j < R; ++j) l += to_f32(bv[j]) * tv[j];
            }
            v += g.lora_scale * l;
        }
        if (g.bias) v += to_f32(((const T*)g.bias)[n]);
        if (g.y_f32) ((float*)g.y)[(int64_t)m * p.ldy + n] = v;
        else ((T*)g.y)[(int64_t)m * p.ldy + n] = from_f32<T>(v);
    }
}

template <typename T, bool NF4, int RT, int MT = 1>
int launch_gemv_rows_rt(GemvRowsArgs a, hipStream_t st) {
    int blocks = 0;
    for (int i = 0; i < UAMD_GEMV_MAX_GROUPS; ++i) {
        a.blk_start[i] = blocks;
        if (i < a.n_groups) blocks += (a.g[i].N + 16 * RT - 1) / (16 * RT);
    }
    a.blk_start[UAMD_GEMV_MAX_GROUPS] = blocks;
    const int tables = NF4 ? 1024 + 256 * 32 * 4 : 0, red = ROWS_WAVES * RT * MT * 64 * 16;
    const int lds = tables > red ? tables : red;
    if (lds > 48 * 1024)
        if (int rc = uamd_lds_optin<&gemv_rows_kernel<T, NF4, RT, MT>>(lds)) return rc;
    hipLaunchKernelGGL((gemv_rows_kernel<T, NF4, RT, MT>), dim3(blocks), dim3(ROWS_THREADS), lds, st, a);
    return uamd_launch_status();
}

// RT: as many tiles per workgroup (token fragments shared) as still leave two workgroups for every CU
template <typename T, bool NF4>
int launch_gemv_rows(const GemvRowsArgs& a, hipStream_t st) {
    int tiles = 0;
    for (int i = 0; i < a.n_groups; ++i) tiles += (a.g[i].N + 15) / 16;
    const int want = 2 * uamd_cu_count_or_256();
    if constexpr (NF4) {
        if (tiles >= 4 * want) return launch_gemv_rows_rt<T, true, 4>(a, st);
    }
    if (tiles >= 2 * want) return launch_gemv_rows_rt<T, NF4, 2>(a, st);
    return launch_gemv_rows_rt<T, NF4, 1>(a, st);
}

// 17 .. 64 token rows: MT = 2 (M <= 32) or 4 token tiles against every decoded weight fragment. A workgroup reads all of X
// (from L2) beside 16 RT weight rows -- M / (4 RT) bytes of X per NF4 byte -- so RT depends on MT as well as on the tile count.
// Measured on the Llama-3-8B projections with RT forced ("RT by MT"; us per launch at M = 64, RT = 1 / 2 / 4):
// q|k|v (384 tiles) 71.5 / 65.6 / 87.6, o (256) 49.5 / 61.8 / 83.3, gate|up (1792) 192 / 177 / 147, down (256, K = 14336)
// 135 / 156 / 191 -- MT = 4 takes the larger RT down to 192 workgroups (3/4 of the CUs) and loses below (128, 96). At M = 32
// the same table is flat within 2 % between the rule of the narrow launches (two workgroups per CU) and its neighbours, and
// worse beyond them: MT = 2 keeps that rule.
template <typename T, bool NF4, int MT>
int launch_gemv_rows_mt(const GemvRowsArgs& a, hipStream_t st) {
    int tiles = 0;
    for (int i = 0; i < a.n_groups; ++i) tiles += (a.g[i].N + 15) / 16;
    const int want = MT == 2 ? 2 * uamd_cu_count_or_256() : 3 * uamd_cu_count_or_256() / 4;
    if constexpr (NF4) {
        if (tiles >= 4 * want) return launch_gemv_rows_rt<T, true, 4, MT>(a, st);
    }
    if (tiles >= 2 * want) return launch_gemv_rows_rt<T, NF4, 2, MT>(a, st);
    return launch_gemv_rows_rt<T, NF4, 1, MT>(a, st);
}
template <typename T, bool NF4>
int launch_gemv_rows_wide(const GemvRowsArgs& a, hipStream_t st) {
    if (a.M <= 16) return launch_gemv_rows<T, NF4>(a, st);
    return a.M <= 32 ? launch_gemv_rows_mt<T, NF4, 2>(a, st) : launch_gemv_rows_mt<T, NF4, 4>(a, st);
}

// ---------------------------------------------------------------------------------------------------------------
// RoPE (rotate-half, the training kernel's arithmetic and rounding points) on the new token's q and k, and the
// append of k, v to the cache at position kv_len[b]. qkv: [B, (Hq + 2 Hk) D] as the fused q|k|v GEMV wrote it.
//
// One rotated pair. Rounding points of the training kernel for 16-bit tables (csrc/rope_embedding.hip rotate<T, NATIVE>, i.e.
// the reference's Triton arithmetic in the cos / sin dtype): every product and the sum are rounded to T.
template <typename T>
__device__ __forceinline__ void rope_pair(float x1, float x2, float c, float s, T& r1, T& r2) {
    r1 = from_f32<T>(round_to<T>(x1 * c) - round_to<T>(x2 * s));
    r2 = from_f32<T>(round_to<T>(x2 * c) + round_to<T>(x1 * s));
}
template <typename T>
__global__ void __launch_bounds__(64) rope_append_kernel(T* __restrict__ qkv, int64_t ld_qkv, const T* __restrict__ cos_t,
                                                         const T* __restrict__ sin_t, int64_t ld_cs,
                                                         const int* __restrict__ kv_len, const int* __restrict__ rope_pos,
                                                         T* __restrict__ kc, T* __restrict__ vc, int64_t c_sb,
                                                         int64_t c_sh, int Hq, int Hk, int D, int s_max) {
    const int h = blockIdx.x, b = blockIdx.y;            // h: q heads, then k heads, then v heads of the fused row
    const int half = D >> 1;
    const int len = kv_len[b];
    const int pos = rope_pos ? rope_pos[b] : len;
    T* v = qkv + (int64_t)b * ld_qkv + (int64_t)h * D;
    if (h < Hq + Hk) {
        T* kd = (h >= Hq && len < s_max) ? kc + (int64_t)b * c_sb + (int64_t)(h - Hq) * c_sh + (int64_t)len * D : nullptr;
        for (int j = threadIdx.x; j < half; j += 64) {
            const float c = to_f32(cos_t[(int64_t)pos * ld_cs + j]), s = to_f32(sin_t[(int64_t)pos * ld_cs + j]);
            T r1, r2;
            rope_pair(to_f32(v[j]), to_f32(v[j + half]), c, s, r1, r2);
            v[j] = r1;
            v[j + half] = r2;
            if (kd) { kd[j] = r1; kd[j + half] = r2; }
        }
    } else if (len < s_max) {
        T* vd = vc + (int64_t)b * c_sb + (int64_t)(h - Hq - Hk) * c_sh + (int64_t)len * D;
        for (int j = threadIdx.x; j < D; j += 64) vd[j] = v[j];
    }
}

// uamd_rope_kv_append_span: row b * R + j of qkv is the j-th new token of sequence b -- RoPE position and cache slot
// kv_len[b] + j, statement for statement the arithmetic of rope_append_kernel, so R successive appends give the same bits. (A
// body of its own: a device function shared with rope_append_kernel changed that kernel's instruction stream.)
template <typename T>
__global__ void __launch_bounds__(64) rope_append_span_kernel(T* __restrict__ qkv, int64_t ld_qkv, const T* __restrict__ cos_t,
                                                              const T* __restrict__ sin_t, int64_t ld_cs,
                                                              const int* __restrict__ kv_len, T* __restrict__ kc,
                                                              T* __restrict__ vc, int64_t c_sb, int64_t c_sh, int R, int Hq,
                                                              int Hk, int D, int s_max) {
    const int h = blockIdx.x, row = blockIdx.y;          // h: q heads, then k heads, then v heads of the fused row
    const int b = row / R;
    const int half = D >> 1;
    const int len = kv_len[b] + (row - b * R);
    T* v = qkv + (int64_t)row * ld_qkv + (int64_t)h * D;
    if (h < Hq + Hk) {
        T* kd = (h >= Hq && len < s_max) ? kc + (int64_t)b * c_sb + (int64_t)(h - Hq) * c_sh + (int64_t)len * D : nullptr;
        for (int j = threadIdx.x; j < half; j += 64) {
            const float c = to_f32(cos_t[(int64_t)len * ld_cs + j]), s = to_f32(sin_t[(int64_t)len * ld_cs + j]);
            T r1, r2;
            rope_pair(to_f32(v[j]), to_f32(v[j + half]), c, s, r1, r2);
            v[j] = r1;
            v[j + half] = r2;
            if (kd) { kd[j] = r1; kd[j + half] = r2; }
        }
    } else if (len < s_max) {
        T* vd = vc + (int64_t)b * c_sb + (int64_t)(h - Hq - Hk) * c_sh + (int64_t)len * D;
        for (int j = threadIdx.x; j < D; j += 64) vd[j] = v[j];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Split-KV decode attention, head dim DD = 128 or 64. Block (split, kvh, b) = 4 waves; a key is DD / 8 lanes x 16 B, so a
// wave-load (all 64 lanes, 1 KiB) covers 4 keys at DD = 128 and 8 at DD = 64; every such lane group keeps, for each of the G
// query heads, an online-softmax partial over its keys with the output restricted to the lane's 8 head-dim columns.
// Partials: [B, Hq, nsplit, DD + 2] fp32 (o[DD], m, l).
template <int DD> struct DecGeo {
    static_assert(DD == 64 || DD == 128, "decode attention: head dim 64 or 128");
    static constexpr int LPK = DD / 8;          // lanes per key, 8 columns (16 B) each
    static constexpr int KPW = 64 / LPK;        // keys per wave-load
    static constexpr int KPB = 4 * KPW;         // keys per block-load: the loop stride and the alignment of a split's start
};

// Shared by the three launches (attn_decode_kernel -> attn_decode_combine_kernel) and the single one
// (attn_decode_fused_kernel):

// offset of the partial of (bh = b * Hq + query head, split)
template <int DD>
__device__ __forceinline__ int64_t part_index(int64_t bh, int nsplit, int split) { return (bh * nsplit + split) * (DD + 2); }

// THE online-softmax merge: (m, l) takes in a second partial (mo, lo), both in the exp2 domain; the caller scales its own
// values by a and the other partial's by c. mr: with nothing but masked keys on both sides (max -inf) the factors are
// exp2(-inf - 0) = 0 instead of exp2(-inf + inf) = NaN.
__device__ __forceinline__ void softmax_merge(float& m, float& l, float mo, float lo, float& a, float& c) {
    const float mn = fmaxf(m, mo);
    const float mr = mn == -INFINITY ? 0.f : mn;
    a = __builtin_amdgcn_exp2f(m - mr);
    c = __builtin_amdgcn_exp2f(mo - mr);
    l = l * a + lo * c;
    m = mn;
}

// The key slots of a wave merged by shuffles (lanes with the same column slice), then the wave's (m, l, o) into LDS.
template <int G, int DD>
__device__ __forceinline__ void waves_to_lds(float (&m)[G], float (&l)[G], float (&o)[G][8], float (&red)[4][G][2],
                                             float (&red_o)[4][G][DD], int lane, int wave) {
    constexpr int LPK = DecGeo<DD>::LPK;
    const int lc = lane % LPK;
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int off = LPK; off <= 32; off <<= 1) {
            const float mo = __shfl_xor(m[g], off, 64), lo = __shfl_xor(l[g], off, 64);
            float a, c;
            softmax_merge(m[g], l[g], mo, lo, a, c);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[g][j] = o[g][j] * a + __shfl_xor(o[g][j], off, 64) * c;
        }
        if (lane < LPK) {
            if (lc == 0) { red[wave][g][0] = m[g]; red[wave][g][1] = l[g]; }
#pragma unroll
            for (int j = 0; j < 8; ++j) red_o[wave][g][lc * 8 + j] = o[g][j];
        }
    }
}

// ... and, after the barrier, the block's partial (mm, ll, oo) of head g, column d over its 4 waves.
template <int G, int DD>
__device__ __forceinline__ void block_partial(const float (&red)[4][G][2], const float (&red_o)[4][G][DD], int g, int d,
                                              float& mm, float& ll, float& oo) {
    mm = -INFINITY;
#pragma unroll
    for (int s = 0; s < 4; ++s) mm = fmaxf(mm, red[s][g][0]);
    const float mr = mm == -INFINITY ? 0.f : mm;
    ll = 0.f; oo = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float a = __builtin_amdgcn_exp2f(red[s][g][0] - mr);
        ll += red[s][g][1] * a;
        oo += red_o[s][g][d] * a;
    }
}

// Column d of a head's output from its plain partials pp[nsplit][DD + 2]: running (max, sum, value) over the splits in a fixed
// order; 4 splits' loads in flight at a time.
template <int DD>
__device__ __forceinline__ float combine_splits(const float* pp, int nsplit, int d) {
    float mm = -INFINITY, ll = 0.f, oo = 0.f;
    for (int s0 = 0; s0 < nsplit; s0 += 4) {
        float ms[4], ls[4], os[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int s = min(s0 + j, nsplit - 1);
            ms[j] = s0 + j < nsplit ? pp[s * (DD + 2) + DD] : -INFINITY;
            ls[j] = pp[s * (DD + 2) + DD + 1];
            os[j] = pp[s * (DD + 2) + d];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float a, c;
            softmax_merge(mm, ll, ms[j], ls[j], a, c);
            oo = oo * a + os[j] * c;
        }
    }
    return ll > 0.f ? oo / ll : 0.f;
}

template <typename T, int G, int DD>
__global__ void __launch_bounds__(256) attn_decode_kernel(const T* __restrict__ q, int64_t q_sb, const T* __restrict__ kc,
                                                          const T* __restrict__ vc, int64_t c_sb, int64_t c_sh,
                                                          const int* __restrict__ kv_len, float* __restrict__ part,
                                                          int Hq, int nsplit, int split_keys, int window,
                                                          float scale_log2, int len_add) {
    const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int LPK = DecGeo<DD>::LPK, KPW = DecGeo<DD>::KPW, KPB = DecGeo<DD>::KPB;
    const int grp = lane / LPK, lc = lane % LPK;          // key slot of the wave-load, 8-column slice
    const int len = kv_len[b] + len_add;                  // keys 0 .. len-1 are valid (the new token included)
    const int first = (window > 0 && len > window) ? len - window : 0;
    const int s0 = split * split_keys, s1 = min(s0 + split_keys, len);
    __shared__ float red[4][G][2];                        // [wave][head][m, l]
    __shared__ float red_o[4][G][DD];
    float m[G], l[G], o[G][8];
    float qv[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        m[g] = -INFINITY; l[g] = 0.f;
        const T* qp = q + (int64_t)b * q_sb + (int64_t)(kvh * G + g) * DD + lc * 8;
        const Vec16<T> v = ld16(qp);
#pragma unroll
        for (int j = 0; j < 8; ++j) { qv[g][j] = to_f32(v.e[j]) * scale_log2; o[g][j] = 0.f; }
    }
    const T* kb = kc + (int64_t)b * c_sb + (int64_t)kvh * c_sh;
    const T* vb = vc + (int64_t)b * c_sb + (int64_t)kvh * c_sh;
    for (int k0 = max(s0, first & ~(KPB - 1)) + wave * KPW; k0 < s1; k0 += KPB) {
        const int key = k0 + grp;
        const bool valid = key < s1 && key >= first;
        const int kl = valid ? key : (len > 0 ? len - 1 : 0);
        const Vec16<T> kk = ld16(kb + (int64_t)kl * DD + lc * 8);
        const Vec16<T> vv = ld16(vb + (int64_t)kl * DD + lc * 8);
        float s[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) a += qv[g][j] * to_f32(kk.e[j]);
            a = lanes_sum<LPK>(a);                        // the key's lanes all get q . k
            s[g] = valid ? a : -INFINITY;
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float alpha, pe;
            softmax_merge(m[g], l[g], s[g], 1.f, alpha, pe);      // the key as a partial of its own: (s, 1)
#pragma unroll
            for (int j = 0; j < 8; ++j) o[g][j] = o[g][j] * alpha + pe * to_f32(vv.e[j]);
        }
    }
    waves_to_lds<G, DD>(m, l, o, red, red_o, lane, wave);
    __syncthreads();
    for (int i = tid; i < G * DD; i += 256) {
        const int g = i / DD, d = i - g * DD;
        float mm, ll, oo;
        block_partial<G, DD>(red, red_o, g, d, mm, ll, oo);
        float* pp = part + part_index<DD>((int64_t)b * Hq + kvh * G + g, nsplit, split);
        pp[d] = oo;
        if (d == 0) { pp[DD] = mm; pp[DD + 1] = ll; }
    }
}

template <typename T, int DD>
__global__ void __launch_bounds__(DD) attn_decode_combine_kernel(const float* __restrict__ part, T* __restrict__ out,
                                                                  int64_t o_sb, int Hq, int nsplit) {
    const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
    const float* pp = part + part_index<DD>((int64_t)b * Hq + h, nsplit, 0);
    out[(int64_t)b * o_sb + (int64_t)h * DD + d] = from_f32<T>(combine_splits<DD>(pp, nsplit, d));
}

// ---------------------------------------------------------------------------------------------------------------
// Shared-prompt decode attention (uamd_attn_decode_shared), the prefix scan: the n samples of prompt p share ONE prompt cache
// pk / pv [P, Hk, S_p, DD], so the R = n * G query rows of (p, kv head) -- sample i, head g of the group: row i * G + g -- are
// scored against every prompt key from one fetch of it. Block (prompt split, kvh, p) = 4 waves:
//   * the split's keys come in fills of SH_CK = 128: every thread loads its 16-byte pieces of K and V (all loads of a fill in
//     flight at once; keys outside [oldest key any row of the group attends, min(split end, L_p)) are not loaded and enter as
//     zeros), K goes to LDS row-major, V transposed ([column][key], two keys per 32-bit word), one barrier;
//   * the rows are cut into tiles of 16; wave w owns tiles w and w + 4 for the whole split (no merge across waves). Rows >= R
//     of the last tile are zero fragments: never loaded, never stored;
//   * per 32 keys and tile: S^T = K Q^T as 2 x DD / 32 v_mfma_f32_16x16x32 (A = 16 keys from LDS, B = the tile's Q fragments,
//     raw 16-bit q), which leaves lane (row, j) with the row's scores of keys 4 j .. 4 j + 3 of both 16-key halves -- exactly
//     the 8 contraction slots the lane feeds to O^T += V^T P^T (A = 16 columns of V^T from LDS, B = P), DD / 16 more MFMAs.
//     The contraction order of the keys is permuted the same way on both operands, nothing is shuffled.
// Roundings: q . k is the MFMA's fp32 accumulation of exact 16-bit products; the score is that times scale * log2 e in fp32;
// running max and sum are fp32 in the exp2 domain (softmax_merge); P = exp2(s - m) is rounded ONCE to the activation type, the
// sum l adds the ROUNDED P (a row whose mass sits on one key returns that V row exactly); P V accumulates in fp32. The partial
// (o, m, l) is fp32; the combine rounds the output once. A row's partial is a fixed sequence of operations on its own query
// (one B column of every MFMA), its own new_len and the prompt's cache: no other row's data enters it, a NaN query stays in
// its row.
constexpr int SH_CK = 128;
template <int DD> struct SharedGeo {
    static constexpr int KROW = DD + 8;                    // elements of a K row in LDS (16 bytes of padding)
    static constexpr int VROW = SH_CK / 2 + 2;             // 32-bit words of a V^T row: key pairs, 8 bytes of padding
    static constexpr int LDS = SH_CK * KROW * 2 + DD * VROW * 4;
};

template <typename T, int DD>
__global__ void __launch_bounds__(256) attn_decode_prefix_kernel(const T* __restrict__ q, int64_t q_sb, const T* __restrict__ pk,
                                                                 const T* __restrict__ pv, int64_t p_sb, int64_t p_sh,
                                                                 const int* __restrict__ prompt_len,
                                                                 const int* __restrict__ new_len, float* __restrict__ part,
                                                                 int n_share, int G, int Hq, int nsplit, int split_keys,
                                                                 int window, float scale_log2, int len_add) {
    typedef typename RowsMfma<T>::frag frag;
    union F { uint4 u; uint2 h[2]; uint32_t w[4]; frag f; };
    constexpr int LPK = DecGeo<DD>::LPK, KROW = SharedGeo<DD>::KROW, VROW = SharedGeo<DD>::VROW;
    constexpr int KIT = SH_CK * LPK / 256, VIT = KIT / 2;  // 16-byte K loads / V key pairs of a thread per fill
    constexpr int QF = DD / 32, OT = DD / 16;              // Q fragments of a row; 16-column tiles of O^T
    extern __shared__ __attribute__((aligned(16))) unsigned char sh_smem[];
    T* const Ks = reinterpret_cast<T*>(sh_smem);
    uint32_t* const Vt = reinterpret_cast<uint32_t*>(sh_smem + SH_CK * KROW * 2);
    const int split = blockIdx.x, kvh = blockIdx.y, p = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, qq = lane >> 4;
    const int R = n_share * G;
    const int Lp = prompt_len[p];
    int first_min = 0;                                     // the oldest key any row of the group attends
    if (window > 0) {
        int mn = new_len[p * n_share];
        for (int i = 1; i < n_share; ++i) mn = min(mn, new_len[p * n_share + i]);
        first_min = max(0, Lp + mn + len_add - window);
    }
    const int s0 = split * split_keys, s1 = min(s0 + split_keys, Lp);
    // the wave's two tiles: lane (r, qq) works for row 16 t + r
    bool rok[2];
    int first[2];
    int64_t bh[2];
    F qf[2][QF];
    float m[2], l[2];
    rows_f32x4 o[2][OT];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
        const int row = (wave + 4 * ti) * 16 + r;
        rok[ti] = row < R;
        const int smp = rok[ti] ? row / G : 0, g = rok[ti] ? row - smp * G : 0;
        const int b = p * n_share + smp;
        first[ti] = window > 0 ? max(0, Lp + new_len[b] + len_add - window) : 0;
        bh[ti] = (int64_t)b * Hq + kvh * G + g;
        const T* qp = q + (int64_t)b * q_sb + (int64_t)(kvh * G + g) * DD + qq * 8;
#pragma unroll
        for (int j = 0; j < QF; ++j)
            qf[ti][j].u = rok[ti] ? *reinterpret_cast<const uint4*>(qp + j * 32) : make_uint4(0, 0, 0, 0);
        m[ti] = -INFINITY; l[ti] = 0.f;
#pragma unroll
        for (int dt = 0; dt < OT; ++dt) o[ti][dt] = rows_f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const T* const kb = pk + (int64_t)p * p_sb + (int64_t)kvh * p_sh;
    const T* const vb = pv + (int64_t)p * p_sb + (int64_t)kvh * p_sh;
    const int live0 = max(s0, first_min);                  // keys [live0, s1) are loaded
    const int c_first = s0 + (live0 - s0) / SH_CK * SH_CK; // the first fill with a live key (fills start on the split's grid)
    for (int c0 = c_first; c0 < s1; c0 += SH_CK) {
        if (c0 != c_first) __syncthreads();                // the previous fill is still being read
        uint4 kr[KIT], vr[VIT][2];
#pragma unroll
        for (int it = 0; it < KIT; ++it) {
            const int i = tid + 256 * it, key = c0 + i / LPK, lc = i % LPK;
            kr[it] = (key >= live0 && key < s1) ? *reinterpret_cast<const uint4*>(kb + (int64_t)key * DD + lc * 8)
                                                : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int it = 0; it < VIT; ++it) {
            const int i = tid + 256 * it, key = c0 + 2 * (i / LPK), lc = i % LPK;
#pragma unroll
            for (int e = 0; e < 2; ++e)
                vr[it][e] = (key + e >= live0 && key + e < s1)
                                ? *reinterpret_cast<const uint4*>(vb + (int64_t)(key + e) * DD + lc * 8) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int it = 0; it < KIT; ++it) {
            const int i = tid + 256 * it;
            *reinterpret_cast<uint4*>(Ks + (i / LPK) * KROW + (i % LPK) * 8) = kr[it];
        }
#pragma unroll
        for (int it = 0; it < VIT; ++it) {
            const int i = tid + 256 * it, kp = i / LPK, lc = i % LPK;
            const uint32_t a[4] = {vr[it][0].x, vr[it][0].y, vr[it][0].z, vr[it][0].w};
            const uint32_t b[4] = {vr[it][1].x, vr[it][1].y, vr[it][1].z, vr[it][1].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {                  // columns lc * 8 + 2 j, + 1: (even key, odd key) per word
                Vt[(lc * 8 + 2 * j) * VROW + kp] = (a[j] & 0xffffu) | (b[j] << 16);
                Vt[(lc * 8 + 2 * j + 1) * VROW + kp] = (a[j] >> 16) | (b[j] & 0xffff0000u);
            }
        }
        __syncthreads();
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
            if ((wave + 4 * ti) * 16 >= R) continue;       // (wave-uniform)
            for (int kg = 0; kg < SH_CK / 32; ++kg) {
                const int k0 = c0 + kg * 32;
                if (k0 + 32 <= live0 || k0 >= s1) continue;
                rows_f32x4 sc[2];
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    sc[hf] = rows_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int j = 0; j < QF; ++j) {
                        F a;
                        a.u = *reinterpret_cast<const uint4*>(Ks + (kg * 32 + hf * 16 + r) * KROW + j * 32 + qq * 8);
                        sc[hf] = RowsMfma<T>::run(a.f, qf[ti][j].f, sc[hf]);
                    }
                }
                // lane (row r, qq): keys k0 + 16 hf + 4 qq + e
                float s[8], mx = -INFINITY;
#pragma unroll
                for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int key = k0 + hf * 16 + qq * 4 + e;
                        s[hf * 4 + e] = (key >= first[ti] && key < s1) ? sc[hf][e] * scale_log2 : -INFINITY;
                        mx = fmaxf(mx, s[hf * 4 + e]);
                    }
                mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                float alpha, unused;
                softmax_merge(m[ti], l[ti], mx, 0.f, alpha, unused);      // l: the lane's own keys, summed over qq at the end
                const float mr = m[ti] == -INFINITY ? 0.f : m[ti];
                float pr[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    pr[e] = round_to<T>(__builtin_amdgcn_exp2f(s[e] - mr));
                    l[ti] += pr[e];
                }
                F pf;
#pragma unroll
                for (int e = 0; e < 4; ++e) pf.w[e] = pack2<T>(pr[2 * e], pr[2 * e + 1]);
#pragma unroll
                for (int dt = 0; dt < OT; ++dt) {
                    F a;                                   // V^T[column 16 dt + r][the lane's 8 keys]
                    const uint32_t* vp = Vt + (dt * 16 + r) * VROW + kg * 16 + qq * 2;
                    a.h[0] = *reinterpret_cast<const uint2*>(vp);
                    a.h[1] = *reinterpret_cast<const uint2*>(vp + 8);
                    o[ti][dt] = RowsMfma<T>::run(a.f, pf.f, o[ti][dt] * alpha);
                }
            }
        }
    }
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
        float ll = l[ti];                                  // fixed order: (qq, qq ^ 1), then (.., .. ^ 2)
        ll += __shfl_xor(ll, 16, 64);
        ll += __shfl_xor(ll, 32, 64);
        if (!rok[ti]) continue;
        float* pp = part + part_index<DD>(bh[ti], nsplit, split);
#pragma unroll
        for (int dt = 0; dt < OT; ++dt)
#pragma unroll
            for (int e = 0; e < 4; ++e) pp[dt * 16 + qq * 4 + e] = o[ti][dt][e];
        if (qq == 0) { pp[DD] = m[ti]; pp[DD + 1] = ll; }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// One fill of the span scan, the prefix scan's statement for statement: keys [c0, c0 + SH_CK) of a (sequence, kv head) cache kb /
// vb into LDS -- K row-major, V transposed with two keys per word; keys outside [live0, s1) are not loaded and enter as zeros.
// The caller's barrier follows. (attn_decode_prefix_kernel keeps its own copy: calling this from it changed its instruction
// stream, and its outputs are pinned bit for bit.)
template <typename T, int DD>
__device__ __forceinline__ void shared_fill(T* const Ks, uint32_t* const Vt, const T* const kb, const T* const vb, int c0,
                                            int live0, int s1, int tid) {
    constexpr int LPK = DecGeo<DD>::LPK, KROW = SharedGeo<DD>::KROW, VROW = SharedGeo<DD>::VROW;
    constexpr int KIT = SH_CK * LPK / 256, VIT = KIT / 2;  // 16-byte K loads / V key pairs of a thread per fill
    uint4 kr[KIT], vr[VIT][2];
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
        const int i = tid + 256 * it, key = c0 + i / LPK, lc = i % LPK;
        kr[it] = (key >= live0 && key < s1) ? *reinterpret_cast<const uint4*>(kb + (int64_t)key * DD + lc * 8)
                                            : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int it = 0; it < VIT; ++it) {
        const int i = tid + 256 * it, key = c0 + 2 * (i / LPK), lc = i % LPK;
#pragma unroll
        for (int e = 0; e < 2; ++e)
            vr[it][e] = (key + e >= live0 && key + e < s1)
                            ? *reinterpret_cast<const uint4*>(vb + (int64_t)(key + e) * DD + lc * 8) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
        const int i = tid + 256 * it;
        *reinterpret_cast<uint4*>(Ks + (i / LPK) * KROW + (i % LPK) * 8) = kr[it];
    }
#pragma unroll
    for (int it = 0; it < VIT; ++it) {
        const int i = tid + 256 * it, kp = i / LPK, lc = i % LPK;
        const uint32_t a[4] = {vr[it][0].x, vr[it][0].y, vr[it][0].z, vr[it][0].w};
        const uint32_t b[4] = {vr[it][1].x, vr[it][1].y, vr[it][1].z, vr[it][1].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {                  // columns lc * 8 + 2 j, + 1: (even key, odd key) per word
            Vt[(lc * 8 + 2 * j) * VROW + kp] = (a[j] & 0xffffu) | (b[j] << 16);
            Vt[(lc * 8 + 2 * j + 1) * VROW + kp] = (a[j] >> 16) | (b[j] & 0xffff0000u);
        }
    }
}

// Span decode attention (uamd_attn_decode_span): sequence b has just appended R tokens at cache slots kv_len[b] .. kv_len[b] +
// R - 1 (a draft span being verified); its R * G query rows of a kv head -- token j, head g of the group: row j * G + g, q row
// b * R + j -- are scored against ONE fetch of the cache. Row (j, g) attends keys [max(0, t_j - window), t_j), t_j = kv_len[b] +
// j + 1: the old cache in full and a causal triangle over the R new keys. The prefix scan's structure throughout -- fills of
// SH_CK keys (shared_fill), 16-row tiles, wave w owns tiles w and w + 4, S^T and O^T on v_mfma_f32_16x16x32, the same rounding
// points (P rounded once, the sum over the rounded P) -- with a key range PER ROW:
//   * a score outside the row's [first, end) is -inf by a select (a NaN key there never enters the row); a row without a key in a
//     32-key group leaves the group with (m, l, o) unchanged in value: exp2(-inf - mr) = 0 with mr = 0 for an empty row, never
//     exp2(-inf + inf); a row without a key in the split is stored as (-inf, 0, 0);
//   * O^T += V^T P^T shares V among the 16 rows of a tile, and 0 * NaN = NaN: a group that is not inside the range of EVERY row
//     of the tile (the triangle, a window's start) runs the product once per token j of the tile with the V fragment masked to
//     j's keys -- bit masks, no arithmetic -- and every lane keeps the pass of its own row's token. A row's partial stays a fixed
//     sequence of operations on its own query, its own range and the cache keys inside it.
template <typename T, int DD>
__global__ void __launch_bounds__(256) attn_decode_span_kernel(const T* __restrict__ q, int64_t q_sb, const T* __restrict__ kc,
                                                               const T* __restrict__ vc, int64_t c_sb, int64_t c_sh,
                                                               const int* __restrict__ kv_len, float* __restrict__ part, int R,
                                                               int G, int Hq, int nsplit, int split_keys, int window,
                                                               float scale_log2) {
    typedef typename RowsMfma<T>::frag frag;
    union F { uint4 u; uint2 h[2]; uint32_t w[4]; frag f; };
    constexpr int KROW = SharedGeo<DD>::KROW, VROW = SharedGeo<DD>::VROW;
    constexpr int QF = DD / 32, OT = DD / 16;              // Q fragments of a row; 16-column tiles of O^T
    extern __shared__ __attribute__((aligned(16))) unsigned char sh_smem[];
    T* const Ks = reinterpret_cast<T*>(sh_smem);
    uint32_t* const Vt = reinterpret_cast<uint32_t*>(sh_smem + SH_CK * KROW * 2);
    const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, qq = lane >> 4;
    const int NR = R * G;
    const int len0 = kv_len[b];
    const int first_min = window > 0 ? max(0, len0 + 1 - window) : 0;      // the oldest key any row attends (token 0's)
    const int s0 = split * split_keys, s1 = min(s0 + split_keys, len0 + R);
    // the wave's two tiles: lane (r, qq) works for row 16 t + r
    bool rok[2];
    int jrow[2], first[2], end[2], jlo[2], jhi[2];
    int64_t bh[2];
    F qf[2][QF];
    float m[2], l[2];
    rows_f32x4 o[2][OT];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
        const int row0 = (wave + 4 * ti) * 16, row = row0 + r;
        rok[ti] = row < NR;
        const int j = rok[ti] ? row / G : 0, g = rok[ti] ? row - j * G : 0;
        jrow[ti] = j;
        jlo[ti] = min(R - 1, row0 / G);                    // the tokens of the tile's rows (wave-uniform)
        jhi[ti] = min(R - 1, (row0 + 15) / G);
        first[ti] = window > 0 ? max(0, len0 + j + 1 - window) : 0;
        end[ti] = min(len0 + j + 1, s1);
        bh[ti] = ((int64_t)b * R + j) * Hq + kvh * G + g;
        const T* qp = q + ((int64_t)b * R + j) * q_sb + (int64_t)(kvh * G + g) * DD + qq * 8;
#pragma unroll
        for (int jf = 0; jf < QF; ++jf)
            qf[ti][jf].u = rok[ti] ? *reinterpret_cast<const uint4*>(qp + jf * 32) : make_uint4(0, 0, 0, 0);
        m[ti] = -INFINITY; l[ti] = 0.f;
#pragma unroll
        for (int dt = 0; dt < OT; ++dt) o[ti][dt] = rows_f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const T* const kb = kc + (int64_t)b * c_sb + (int64_t)kvh * c_sh;
    const T* const vb = vc + (int64_t)b * c_sb + (int64_t)kvh * c_sh;
    const int live0 = max(s0, first_min);                  // keys [live0, s1) are loaded
    const int c_first = s0 + (live0 - s0) / SH_CK * SH_CK; // the first fill with a live key (fills start on the split's grid)
    for (int c0 = c_first; c0 < s1; c0 += SH_CK) {
        if (c0 != c_first) __syncthreads();                // the previous fill is still being read
        shared_fill<T, DD>(Ks, Vt, kb, vb, c0, live0, s1, tid);
        __syncthreads();
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
            if ((wave + 4 * ti) * 16 >= NR) continue;      // (wave-uniform)
            const int t_lo = len0 + jlo[ti] + 1;           // the shortest range's end, the latest range's start of the tile
            const int f_hi = window > 0 ? max(0, len0 + jhi[ti] + 1 - window) : 0;
            for (int kg = 0; kg < SH_CK / 32; ++kg) {
                const int k0 = c0 + kg * 32;
                if (k0 + 32 <= live0 || k0 >= s1) continue;
                rows_f32x4 sc[2];
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    sc[hf] = rows_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int jf = 0; jf < QF; ++jf) {
                        F a;
                        a.u = *reinterpret_cast<const uint4*>(Ks + (kg * 32 + hf * 16 + r) * KROW + jf * 32 + qq * 8);
                        sc[hf] = RowsMfma<T>::run(a.f, qf[ti][jf].f, sc[hf]);
                    }
                }
                // lane (row r, qq): keys k0 + 16 hf + 4 qq + e
                float s[8], mx = -INFINITY;
#pragma unroll
                for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int key = k0 + hf * 16 + qq * 4 + e;
                        s[hf * 4 + e] = (key >= first[ti] && key < end[ti]) ? sc[hf][e] * scale_log2 : -INFINITY;
                        mx = fmaxf(mx, s[hf * 4 + e]);
                    }
                mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                float alpha, unused;
                softmax_merge(m[ti], l[ti], mx, 0.f, alpha, unused);      // l: the lane's own keys, summed over qq at the end
                const float mr = m[ti] == -INFINITY ? 0.f : m[ti];
                float pr[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    pr[e] = round_to<T>(__builtin_amdgcn_exp2f(s[e] - mr));
                    l[ti] += pr[e];
                }
                F pf;
#pragma unroll
                for (int e = 0; e < 4; ++e) pf.w[e] = pack2<T>(pr[2 * e], pr[2 * e + 1]);
                // every loaded key of the group inside every row's range: one product for the tile (keys outside [live0, s1) are
                // zeros in LDS)
                const bool whole = k0 >= f_hi && min(k0 + 32, s1) <= t_lo;      // (wave-uniform)
#pragma unroll
                for (int dt = 0; dt < OT; ++dt) {
                    F a;                                   // V^T[column 16 dt + r][the lane's 8 keys]
                    const uint32_t* vp = Vt + (dt * 16 + r) * VROW + kg * 16 + qq * 2;
                    a.h[0] = *reinterpret_cast<const uint2*>(vp);
                    a.h[1] = *reinterpret_cast<const uint2*>(vp + 8);
                    const rows_f32x4 oa = o[ti][dt] * alpha;
                    if (whole) {
                        o[ti][dt] = RowsMfma<T>::run(a.f, pf.f, oa);
                    } else {
                        rows_f32x4 on = oa;
                        for (int jj = jlo[ti]; jj <= jhi[ti]; ++jj) {
                            const int ke = min(len0 + jj + 1, s1), kf = window > 0 ? max(0, len0 + jj + 1 - window) : 0;
                            F am;
#pragma unroll
                            for (int w = 0; w < 4; ++w) {  // word w: keys k0 + 16 (w / 2) + 4 qq + 2 (w % 2), + 1
                                const int key = k0 + (w >> 1) * 16 + qq * 4 + (w & 1) * 2;
                                const uint32_t keep = ((key >= kf && key < ke) ? 0xffffu : 0u) |
                                                      ((key + 1 >= kf && key + 1 < ke) ? 0xffff0000u : 0u);
                                am.w[w] = a.w[w] & keep;
                            }
                            const rows_f32x4 acc = RowsMfma<T>::run(am.f, pf.f, oa);
                            if (jrow[ti] == jj) on = acc;
                        }
                        o[ti][dt] = on;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
        float ll = l[ti];                                  // fixed order: (qq, qq ^ 1), then (.., .. ^ 2)
        ll += __shfl_xor(ll, 16, 64);
        ll += __shfl_xor(ll, 32, 64);
        if (!rok[ti]) continue;
        float* pp = part + part_index<DD>(bh[ti], nsplit, split);
#pragma unroll
        for (int dt = 0; dt < OT; ++dt)
#pragma unroll
            for (int e = 0; e < 4; ++e) pp[dt * 16 + qq * 4 + e] = o[ti][dt][e];
        if (qq == 0) { pp[DD] = m[ti]; pp[DD + 1] = ll; }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Prompt-lookup drafts (uamd_ngram_draft, uamd_accept_greedy): the two tiny kernels that turn the span step into speculative
// decoding of ONE sequence from its own context. Plain C++; every input and counter lives on the device, so draft -> R-row
// step -> argmax -> accept replays as one hipGraph.
//
// The draft. For n = n_max .. 1: suffix = hist[len - n, len); among the starts i with i + n <= len - 1 (the match is followed
// by at least one token) and hist[i, i + n) == suffix the LARGEST wins, and the first n with a match wins. tok[0] = the last
// token, tok[1 .. n_draft] = what followed the match (at most K), the other slots 0.
__global__ void __launch_bounds__(256) ngram_draft_kernel(const long long* __restrict__ hist, const int* __restrict__ hist_len,
                                                          int cap, int n_max, int K, long long* __restrict__ tok,
                                                          int* __restrict__ n_draft) {
    __shared__ int best;
    const int tid = threadIdx.x;
    const int len = min(*hist_len, cap);
    int at = -1, n_hit = 0;
    for (int n = min(n_max, len - 1); n >= 1 && at < 0; --n) {
        if (tid == 0) best = -1;
        __syncthreads();
        for (int i = tid; i + n <= len - 1; i += 256) {
            bool same = true;
            for (int e = 0; e < n; ++e) same = same && hist[i + e] == hist[len - n + e];
            if (same) atomicMax(&best, i);
        }
        __syncthreads();
        at = best;
        n_hit = n;
        __syncthreads();                                   // everyone has read `best` before the next n clears it
    }
    const int from = at + n_hit;
    const int nd = at >= 0 ? min(K, len - from) : 0;
    if (tid == 0) *n_draft = nd;
    if (tid <= K) tok[tid] = tid == 0 ? (len > 0 ? hist[len - 1] : 0) : (tid <= nd ? hist[from + tid - 1] : 0);
}

// The verdict. tok[0 .. K] were the step's token rows, a[j] the arg-max of row j's logits, i.e. the model's token AFTER
// tok[0 .. j]. m = the number of leading drafts with tok[j] == a[j - 1]; a[0 .. m] are emitted. Nothing follows an emitted eos
// and no more than `remaining` tokens are emitted. Lane 0 of one wave does it all (K <= 15).
__global__ void __launch_bounds__(64) accept_greedy_kernel(const long long* __restrict__ tok, const long long* __restrict__ a, int K,
                                                           const long long* __restrict__ eos, int n_eos,
                                                           long long* __restrict__ hist, int cap, int* __restrict__ hist_len,
                                                           int* __restrict__ kv_len, int* __restrict__ remaining,
                                                           int* __restrict__ done, const int* __restrict__ n_draft,
                                                           long long* __restrict__ stats) {
    if (threadIdx.x != 0) return;
    const int rem = *remaining, len = *hist_len;
    if (*done || rem <= 0 || len >= cap) { *done = 1; return; }
    auto is_eos = [&](long long t) {
        bool hit = false;
        for (int e = 0; e < n_eos; ++e) hit = hit || eos[e] == t;
        return hit;
    };
    int m = 0;
    bool stop = is_eos(a[0]);
    while (!stop && m < K && m + 1 < rem && len + m + 1 < cap && tok[m + 1] == a[m]) {
        ++m;
        stop = is_eos(a[m]);
    }
    for (int j = 0; j <= m; ++j) hist[len + j] = a[j];
    *hist_len = len + m + 1;
    *kv_len += m + 1;
    *remaining = rem - (m + 1);
    if (stop || rem - (m + 1) <= 0) *done = 1;
    stats[0] += 1;
    stats[1] += *n_draft;
    stats[2] += m;
    stats[3] += m + 1;
}

// ---------------------------------------------------------------------------------------------------------------
// FP8 KV cache (opt-in; the format is defined once, in include/unsloth_amd.h): a cache row -- one (sequence, KV head, position)
// vector of DD values -- is DD bytes of OCP e4m3fn codes plus ONE fp32 scale, amax / 448. Half the bytes of a 16-bit row (plus
// 4), which is what a decode step of a batch at a long context reads. The lane geometry is DecGeo's throughout: DD / 8 lanes
// per row, 8 columns each -- a 16-byte load of the 16-bit source, an 8-byte load or store of the codes.
//
// THE quantiser of a row, shared by the two writers (kv_store_fp8_kernel: prefill; rope_append_fp8_kernel: the token step), so a
// key appended by a step and the same key stored by prefill are the same bytes. x: the lane's 8 columns, already rounded to the
// activation type, as fp32; every lane of the row's group gets the row's scale back and returns its 8 codes. Both divisions are
// IEEE (no fast-math in this build), the conversion is v_cvt_pk_fp8_f32: round to nearest even, the sign of zero kept. A row
// with a non-finite element gets scale = NaN (its codes are unspecified): every score against that key is NaN.
template <int LPK>
__device__ __forceinline__ float lanes_max(float v) {
    static_assert(LPK == 8 || LPK == 16, "half a DPP row or a whole one");
#define UAMD_DPP_MAX(v, CTRL) fmaxf((v), __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, (v)), (CTRL), 0xf, 0xf, true)))
    v = UAMD_DPP_MAX(v, 0xb1);      // quad_perm [1,0,3,2]
    v = UAMD_DPP_MAX(v, 0x4e);      // quad_perm [2,3,0,1]
    v = UAMD_DPP_MAX(v, 0x141);     // row_half_mirror
    if constexpr (LPK == 16) v = UAMD_DPP_MAX(v, 0x140);     // row_mirror
#undef UAMD_DPP_MAX
    return v;
}
constexpr float FP8_MAX = 448.f;                     // largest finite e4m3fn value
template <int LPK>
__device__ __forceinline__ uint2 quant_row_fp8(const float (&x)[8], float& scale) {
    float am = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float a = fabsf(x[j]);
        am = a < INFINITY ? fmaxf(am, a) : INFINITY;       // NaN or inf: the row's amax becomes inf (fmaxf would drop a NaN)
    }
    am = lanes_max<LPK>(am);
    scale = am == INFINITY ? __builtin_nanf("") : (am > 0.f ? am / FP8_MAX : 1.f);
    int lo = 0, hi = 0;
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = fminf(fmaxf(x[j] / scale, -FP8_MAX), FP8_MAX);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], hi, true);
    return make_uint2((uint32_t)lo, (uint32_t)hi);
}
// Prefill's writer: rows (b, h, t), t < T, of a strided 16-bit [B, Hk, T, DD] tensor (unit stride along DD: the transpose(1, 2)
// view of the projection output, no contiguous copy) -> positions [0, T) of the code and scale caches. A wave-load covers KPW
// rows (one lane group each), a block KPB; rows past the end are loaded from the last row and not stored.
template <typename T, int DD>
__global__ void __launch_bounds__(256) kv_store_fp8_kernel(const T* __restrict__ src, int64_t s_sb, int64_t s_sh, int64_t s_st,
                                                           uint8_t* __restrict__ codes, float* __restrict__ scales,
                                                           int64_t c_sb, int64_t c_sh, int Hk, int Tn, int64_t rows) {
    constexpr int LPK = DecGeo<DD>::LPK, KPW = DecGeo<DD>::KPW, KPB = DecGeo<DD>::KPB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane % LPK;
    const int64_t row = (int64_t)blockIdx.x * KPB + wave * KPW + lane / LPK;
    const bool valid = row < rows;
    const int64_t r = valid ? row : rows - 1;
    const int t = (int)(r % Tn);
    const int h = (int)((r / Tn) % Hk);
    const int64_t b = r / ((int64_t)Tn * Hk);
    const Vec16<T> v = ld16(src + b * s_sb + h * s_sh + t * s_st + lc * 8);
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = to_f32(v.e[j]);
    float scale;
    const uint2 c = quant_row_fp8<LPK>(x, scale);
    if (valid) {
        *reinterpret_cast<uint2*>(codes + b * c_sb + h * c_sh + (int64_t)t * DD + lc * 8) = c;
        if (lc == 0) scales[(b * c_sb + h * c_sh) / DD + t] = scale;
    }
}

// The token step's writer: rope_append_kernel with an FP8 cache. q and k are rotated in place in the fused row with rope_pair's
// rounding points; what is quantised is what that kernel would have stored -- the rotated k rounded to T, the raw v. The row
// goes through LDS once to change hands from rope_pair's layout (a lane owns columns j and j + DD / 2) to the quantiser's (8
// adjacent columns); every lane group quantises the same row, group 0 stores.
template <typename T, int DD>
__global__ void __launch_bounds__(64) rope_append_fp8_kernel(T* __restrict__ qkv, int64_t ld_qkv, const T* __restrict__ cos_t,
                                                             const T* __restrict__ sin_t, int64_t ld_cs,
                                                             const int* __restrict__ kv_len, const int* __restrict__ rope_pos,
                                                             uint8_t* __restrict__ kc, float* __restrict__ ks,
                                                             uint8_t* __restrict__ vc, float* __restrict__ vs, int64_t c_sb,
                                                             int64_t c_sh, int Hq, int Hk, int s_max) {
    constexpr int LPK = DecGeo<DD>::LPK, half = DD / 2;
    const int h = blockIdx.x, b = blockIdx.y;            // h: q heads, then k heads, then v heads of the fused row
    const int lane = threadIdx.x;
    const int len = kv_len[b];
    const int pos = rope_pos ? rope_pos[b] : len;
    T* v = qkv + (int64_t)b * ld_qkv + (int64_t)h * DD;
    __shared__ __attribute__((aligned(16))) T row[DD];
    if (h < Hq + Hk) {
        for (int j = lane; j < half; j += 64) {
            const float c = to_f32(cos_t[(int64_t)pos * ld_cs + j]), s = to_f32(sin_t[(int64_t)pos * ld_cs + j]);
            T r1, r2;
            rope_pair(to_f32(v[j]), to_f32(v[j + half]), c, s, r1, r2);
            v[j] = r1;
            v[j + half] = r2;
            row[j] = r1;
            row[j + half] = r2;
        }
        if (h < Hq) return;
    } else {
        for (int j = lane; j < DD; j += 64) row[j] = v[j];
    }
    __syncthreads();
    if (len < 0 || len >= s_max) return;                 // a full cache: nothing is written (as rope_append_kernel)
    const bool is_k = h < Hq + Hk;
    const int kvh = is_k ? h - Hq : h - Hq - Hk;
    const int lc = lane % LPK;
    const Vec16<T> rv = ld16(row + lc * 8);
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = to_f32(rv.e[j]);
    float scale;
    const uint2 c = quant_row_fp8<LPK>(x, scale);
    if (lane < LPK) {
        const int64_t base = (int64_t)b * c_sb + (int64_t)kvh * c_sh;
        *reinterpret_cast<uint2*>((is_k ? kc : vc) + base + (int64_t)len * DD + lc * 8) = c;
        if (lc == 0) (is_k ? ks : vs)[base / DD + len] = scale;
    }
}

// attn_decode_kernel over the FP8 cache: the same grid, key range, key -> (wave, lane group) assignment, block merge
// (waves_to_lds, block_partial) and partial layout, so attn_decode_combine_kernel finishes it unchanged. What differs:
//   * a lane's 8 columns of a key are 8 bytes, converted by v_cvt_pk_f32_fp8 (exact); the score is (sum_j q_j code_j) x k_scale,
//     the key's softmax weight is multiplied by v_scale ONCE and then meets the 8 converted codes. All fp32; the only rounding
//     to T is the combine's store;
//   * a trip is 128 keys: the NI block-loads of codes and scales of K and of V (8 at DD = 128, 4 at DD = 64) are all issued
//     before the first is used -- at the engine's 128-key splits a workgroup has its whole split in flight at once, where a
//     loop of one block-load per trip pays one HBM round trip each (the note in front of attn_decode_fused_kernel);
//   * the trip's keys are accumulated in chunks of CH = 2 block-loads, the way attn_decode_fused_kernel does it for a whole trip
//     (one running-max rescale per head and chunk, not one per key), and products run two columns at a time (v_pk_fma_f32 --
//     the conversion delivers pairs). With half the bytes per key it is the per-key arithmetic and the number of workgroups a CU
//     holds that bound this kernel, not HBM alone: key-at-a-time (36 vector instructions per key and head, 112 VGPRs at G = 4)
//     the step of 16 sequences at context 8192 took 9.76 ms, with CH = 2 (125 VGPRs: still four workgroups per CU) 9.32, with
//     the whole trip as one chunk (170 VGPRs: fewer instructions, three workgroups) 10.97; the 16-bit cache: 11.0 - 11.2.
typedef __attribute__((ext_vector_type(2))) float dec_f32x2;
__device__ __forceinline__ void fp8x8_to_f32x2(uint2 c, dec_f32x2 (&f)[4]) {
    f[0] = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, false);
    f[1] = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, true);
    f[2] = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, false);
    f[3] = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, true);
}
template <typename T, int G, int DD>
__global__ void __launch_bounds__(256) attn_decode_fp8_kernel(const T* __restrict__ q, int64_t q_sb, const uint8_t* __restrict__ kc,
                                                              const uint8_t* __restrict__ vc, const float* __restrict__ ks,
                                                              const float* __restrict__ vs, int64_t c_sb, int64_t c_sh,
                                                              const int* __restrict__ kv_len, float* __restrict__ part,
                                                              int Hq, int nsplit, int split_keys, int window,
                                                              float scale_log2, int len_add) {
    const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int LPK = DecGeo<DD>::LPK, KPW = DecGeo<DD>::KPW, KPB = DecGeo<DD>::KPB;
    constexpr int NI = 128 / KPB, CH = 2;
    const int grp = lane / LPK, lc = lane % LPK;
    const int len = kv_len[b] + len_add;
    const int first = (window > 0 && len > window) ? len - window : 0;
    const int s0 = split * split_keys, s1 = min(s0 + split_keys, len);
    __shared__ float red[4][G][2];
    __shared__ float red_o[4][G][DD];
    float m[G], l[G];
    dec_f32x2 o2[G][4], qv[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        m[g] = -INFINITY; l[g] = 0.f;
        const T* qp = q + (int64_t)b * q_sb + (int64_t)(kvh * G + g) * DD + lc * 8;
        const Vec16<T> v = ld16(qp);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            qv[g][j] = dec_f32x2{to_f32(v.e[2 * j]) * scale_log2, to_f32(v.e[2 * j + 1]) * scale_log2};
            o2[g][j] = dec_f32x2{0.f, 0.f};
        }
    }
    const int64_t base = (int64_t)b * c_sb + (int64_t)kvh * c_sh;
    const uint8_t* kb = kc + base;
    const uint8_t* vb = vc + base;
    const float* ksb = ks + base / DD;
    const float* vsb = vs + base / DD;
    const int safe = len > 0 ? len - 1 : 0;               // the row a masked lane loads (weight zero)
    for (int k0 = max(s0, first & ~(KPB - 1)) + wave * KPW; k0 < s1; k0 += NI * KPB) {
        uint2 kk[NI], vv[NI];
        float ksc[NI], vsc[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int key = k0 + i * KPB + grp;
            const int kl = (key < s1 && key >= first) ? key : safe;
            kk[i] = *reinterpret_cast<const uint2*>(kb + (int64_t)kl * DD + lc * 8);
            vv[i] = *reinterpret_cast<const uint2*>(vb + (int64_t)kl * DD + lc * 8);
            ksc[i] = ksb[kl];
            vsc[i] = vsb[kl];
        }
        // the trip's keys in chunks of CH block-loads: scores of the chunk, ONE running-max rescale per head and chunk, then the
        // chunk's keys accumulate; a key's weight meets v_scale once
#pragma unroll
        for (int c0 = 0; c0 < NI; c0 += CH) {
            if (k0 + c0 * KPB >= s1) break;               // (wave-uniform) the split ends inside the trip
            float sc[CH][G];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int i = c0 + c;
                const int key = k0 + i * KPB + grp;
                const bool valid = key < s1 && key >= first;
                dec_f32x2 kf[4];
                fp8x8_to_f32x2(kk[i], kf);
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    dec_f32x2 a2 = qv[g][0] * kf[0];
#pragma unroll
                    for (int j = 1; j < 4; ++j) a2 = __builtin_elementwise_fma(qv[g][j], kf[j], a2);
                    const float a = lanes_sum<LPK>(a2[0] + a2[1]) * ksc[i];  // the key's lanes all get (q . codes) x k_scale
                    sc[c][g] = valid ? a : -INFINITY;
                }
            }
            float mr[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float mc = sc[0][g];
#pragma unroll
                for (int c = 1; c < CH; ++c) mc = fmaxf(mc, sc[c][g]);
                const float mn = fmaxf(m[g], mc);
                mr[g] = mn == -INFINITY ? 0.f : mn;       // nothing but masked keys so far: exp2(-inf - 0) = 0, not exp2(nan)
                const float alpha = __builtin_amdgcn_exp2f(m[g] - mr[g]);
                m[g] = mn;
                l[g] *= alpha;
#pragma unroll
                for (int j = 0; j < 4; ++j) o2[g][j] *= alpha;
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int i = c0 + c;
                dec_f32x2 vf[4];
                fp8x8_to_f32x2(vv[i], vf);
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const float pe = __builtin_amdgcn_exp2f(sc[c][g] - mr[g]);
                    l[g] += pe;
                    const float w = pe * vsc[i];
#pragma unroll
                    for (int j = 0; j < 4; ++j) o2[g][j] = __builtin_elementwise_fma(dec_f32x2{w, w}, vf[j], o2[g][j]);
                }
            }
        }
    }
    float o[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) { o[g][2 * j] = o2[g][j][0]; o[g][2 * j + 1] = o2[g][j][1]; }
    waves_to_lds<G, DD>(m, l, o, red, red_o, lane, wave);
    __syncthreads();
    for (int i = tid; i < G * DD; i += 256) {
        const int g = i / DD, d = i - g * DD;
        float mm, ll, oo;
        block_partial<G, DD>(red, red_o, g, d, mm, ll, oo);
        float* pp = part + part_index<DD>((int64_t)b * Hq + kvh * G + g, nsplit, split);
        pp[d] = oo;
        if (d == 0) { pp[DD] = mm; pp[DD + 1] = ll; }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// RoPE + cache append + split-KV attention + combine as ONE launch (uamd_attn_decode_fused). The rotation (rope_pair), the
// merge of a block's partials (softmax_merge, waves_to_lds, block_partial), the partial layout (part_index) and the combine
// (combine_splits) are the functions rope_append_kernel -> attn_decode_kernel -> attn_decode_combine_kernel call, and the key
// partition is the same. What differs:
//   * the keys of a split are accumulated chunk-wise (one running-max rescale per NI keys of a lane group instead of one per
//     key), so the result equals the three launches' to fp32 rounding, and bit for bit where a split holds one block-load of
//     keys. The trip stays written out here: as a shared function the compiler schedules its G = 7, D = 128 instance, at the
//     register limit, measurably slower;
//   * every block rotates the G query heads of its KV head itself from the raw q|k|v row (G x D/2 pairs; qkv is not written);
//   * the block whose split owns position len0 = kv_len[b] rotates the new k, appends k and v to the cache and takes both
//     from LDS when its loop reaches that key (a store followed by a load of the same line in one kernel would depend on the
//     vector cache's write policy);
//   * all K / V loads of a 128-key trip (NI wave-loads of each: 8 at D = 128, 4 at D = 64, where a wave-load covers twice the
//     keys) are issued before the first one is used: a loop of one block-load per trip pays one HBM round trip each, eight in
//     a row;
//   * the combine. Launches of up to 256 blocks (context 4096 at 8 KV heads): partials travel as 8-byte {value, tag}
//     granules (one device-scope store each, never torn, no fence; the caller's launch tag as in gemv_kernel) and every block
//     combines ITS 1 / nsplit of the G x D outputs, polling the granules of all splits in split order. Larger launches
//     (not certainly resident at once): plain partials, release fence, arrival counter; the last block of a (batch, KV head)
//     combines everything after an acquire fence -- measured at 21 us for this tail (buffer_wbl2 4.5 us, the atomic's round
//     trip 5.5 us, the cold re-read of the partials 9.5 us; profiles/r04u_decode_phase_trace.txt), the price of the two
//     launches it replaces.
struct AttnDecFusedArgs {
    const void* qkv; int64_t ld_qkv;
    const void* cos_t; const void* sin_t; int64_t ld_cs;
    const int* kv_len; const int* rope_pos;
    void* kc; void* vc; int64_t c_sb, c_sh;
    float* part; int* counters;
    void* out; int64_t o_sb;
    int Hq, Hk, s_max, nsplit, split_keys, window;
    float scale_log2;
    int gran;            // 1: partials travel as {value, tag} granules and every block combines its share (whole launch resident)
    unsigned tag;
    const int* tag_dev;
};
template <typename T, int G, int DD>
__global__ void __launch_bounds__(256) attn_decode_fused_kernel(AttnDecFusedArgs a) {
    constexpr int NI = 128 / DecGeo<DD>::KPB;             // wave-loads of K (and of V) in flight: 128 keys per block trip
    const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int LPK = DecGeo<DD>::LPK, KPW = DecGeo<DD>::KPW, KPB = DecGeo<DD>::KPB;
    const int grp = lane / LPK, lc = lane % LPK;
    const int len0 = a.kv_len[b];                         // keys already in the cache = index of the new one
    const int pos = a.rope_pos ? a.rope_pos[b] : len0;
    const int len = len0 + 1;
    const int first = (a.window > 0 && len > a.window) ? len - a.window : 0;
    const int s0 = split * a.split_keys, s1 = min(s0 + a.split_keys, len);
    const bool own = len0 >= s0 && len0 < s0 + a.split_keys;
    unsigned tag = a.tag;                                   // the caller's launch tag (see gemv_kernel)
    if (a.tag_dev) tag += (unsigned)*a.tag_dev * UAMD_TAG_STRIDE;
    DTRACE_DECL;
    DSTAMP(0);
    __shared__ float q_s[G][DD];
    __shared__ __attribute__((aligned(16))) T kn[DD];
    __shared__ __attribute__((aligned(16))) T vn[DD];
    __shared__ float red[4][G][2];
    __shared__ float red_o[4][G][DD];
    __shared__ int last_s;
    const T* row = (const T*)a.qkv + (int64_t)b * a.ld_qkv;
    const T* cs = (const T*)a.cos_t + (int64_t)pos * a.ld_cs;
    const T* sn = (const T*)a.sin_t + (int64_t)pos * a.ld_cs;
    constexpr int HALF = DD / 2;
    static_assert(HALF <= 64 && 64 + DD <= 256, "wave 0 rotates the new k, the lanes from wave 1 on copy the new v");
    for (int i = tid; i < G * HALF; i += 256) {
        const int g = i / HALF, j = i - g * HALF;
        const T* v = row + (int64_t)(kvh * G + g) * DD;
        const float c = to_f32(cs[j]), s = to_f32(sn[j]);
        T r1, r2;
        rope_pair(to_f32(v[j]), to_f32(v[j + HALF]), c, s, r1, r2);
        q_s[g][j] = to_f32(r1) * a.scale_log2;
        q_s[g][j + HALF] = to_f32(r2) * a.scale_log2;
    }
    if (own) {
        if (tid < HALF) {
            const int j = tid;
            const T* v = row + (int64_t)(a.Hq + kvh) * DD;
            const float c = to_f32(cs[j]), s = to_f32(sn[j]);
            T r1, r2;
            rope_pair(to_f32(v[j]), to_f32(v[j + HALF]), c, s, r1, r2);
            kn[j] = r1;
            kn[j + HALF] = r2;
            if (len0 < a.s_max) {
                T* kd = (T*)a.kc + (int64_t)b * a.c_sb + (int64_t)kvh * a.c_sh + (int64_t)len0 * DD;
                kd[j] = r1;
                kd[j + HALF] = r2;
            }
        } else if (tid >= 64 && tid < 64 + DD) {
            const int d = tid - 64;
            const T val = row[(int64_t)(a.Hq + a.Hk + kvh) * DD + d];
            vn[d] = val;
            if (len0 < a.s_max) ((T*)a.vc)[(int64_t)b * a.c_sb + (int64_t)kvh * a.c_sh + (int64_t)len0 * DD + d] = val;
        }
    }
    DSTAMP(1);
    __syncthreads();
    DSTAMP(2);
    float m[G], l[G], o[G][8];
    float qv[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        m[g] = -INFINITY; l[g] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { qv[g][j] = q_s[g][lc * 8 + j]; o[g][j] = 0.f; }
    }
    const T* kb = (const T*)a.kc + (int64_t)b * a.c_sb + (int64_t)kvh * a.c_sh;
    const T* vb = (const T*)a.vc + (int64_t)b * a.c_sb + (int64_t)kvh * a.c_sh;
    const int safe = len0 > 0 ? len0 - 1 : 0;
    for (int base = max(s0, first & ~(KPB - 1)) + wave * KPW; base < s1; base += KPB * NI) {
        Vec16<T> kk[NI], vv[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int key = base + KPB * i + grp;
            const bool cached = key < s1 && key >= first && key != len0;
            const int kl = cached ? key : safe;
            kk[i] = ld16(kb + (int64_t)kl * DD + lc * 8);
            vv[i] = ld16(vb + (int64_t)kl * DD + lc * 8);
        }
        DSTAMP(3);
#ifdef UAMD_DECODE_TRACE
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        DSTAMP(4);
#endif
        // pass 1: the scores of the chunk's keys, all (key, head) pairs independent of each other (the one-key-at-a-time online
        // softmax this replaces was a single dependent chain per head: 3.9 us for 8 keys with one wave per SIMD to hide nothing
        // behind, profiles/r04z_decode_phase_trace.txt)
        float sc[NI][G];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int key = base + KPB * i + grp;
            const bool valid = key < s1 && key >= first;
            if (own && key == len0) {
                kk[i] = *reinterpret_cast<const Vec16<T>*>(kn + lc * 8);
                vv[i] = *reinterpret_cast<const Vec16<T>*>(vn + lc * 8);
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float acc = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) acc += qv[g][j] * to_f32(kk[i].e[j]);
                acc = lanes_sum<LPK>(acc);
                sc[i][g] = valid ? acc : -INFINITY;
            }
        }
        // pass 2: one rescale per head and chunk, then the chunk's keys accumulate independently
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float mc = sc[0][g];
#pragma unroll
            for (int i = 1; i < NI; ++i) mc = fmaxf(mc, sc[i][g]);
            const float mn = fmaxf(m[g], mc);
            const float mr = mn == -INFINITY ? 0.f : mn;
            const float alpha = __builtin_amdgcn_exp2f(m[g] - mr);
            m[g] = mn;
            float ls = l[g] * alpha;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[g][j] *= alpha;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const float pe = __builtin_amdgcn_exp2f(sc[i][g] - mr);
                ls += pe;
#pragma unroll
                for (int j = 0; j < 8; ++j) o[g][j] += pe * to_f32(vv[i].e[j]);
            }
            l[g] = ls;
        }
    }
    DSTAMP(5);
    waves_to_lds<G, DD>(m, l, o, red, red_o, lane, wave);
    __syncthreads();
    for (int i = tid; i < G * DD; i += 256) {
        const int g = i / DD, d = i - g * DD;
        float mm, ll, oo;
        block_partial<G, DD>(red, red_o, g, d, mm, ll, oo);
        const int64_t at = part_index<DD>((int64_t)b * a.Hq + kvh * G + g, a.nsplit, split);
        if (a.gran) {       // {value, tag} granules: one 8-byte device-scope store each, no fence
            unsigned long long* pg = reinterpret_cast<unsigned long long*>(a.part) + at;
            const unsigned long long hi = (unsigned long long)tag << 32;
            __hip_atomic_store(pg + d, hi | __float_as_uint(oo), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (d == 0) {
                __hip_atomic_store(pg + DD, hi | __float_as_uint(mm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(pg + DD + 1, hi | __float_as_uint(ll), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else {
            float* pp = a.part + at;
            pp[d] = oo;
            if (d == 0) { pp[DD] = mm; pp[DD + 1] = ll; }
        }
    }
    if (a.gran) {
        // ---- every block of the (batch, KV head) combines ITS share of the G x D outputs from the granules of all splits, in
        //      split order (combine_splits' arithmetic). All blocks of the launch are resident (the host checks), and
        //      each has published before it polls: nobody waits for a block that has not started. Polls are bounded.
        DSTAMP(6);
        const int chunk = (G * DD + a.nsplit - 1) / a.nsplit;
        const int i_end = min((split + 1) * chunk, G * DD);
        for (int i = split * chunk + tid; i < i_end; i += 256) {
            const int g = i / DD, d = i - g * DD;
            const unsigned long long* pg = reinterpret_cast<const unsigned long long*>(a.part) +
                                           part_index<DD>((int64_t)b * a.Hq + kvh * G + g, a.nsplit, 0);
            float mm = -INFINITY, ll = 0.f, oo = 0.f;
            for (int sb = 0; sb < a.nsplit; sb += 8) {
                unsigned long long gm[8], gl[8], go[8];
                for (int spin = 0; spin < (1 << 18); ++spin) {
                    bool ok = true;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int sp = min(sb + j, a.nsplit - 1);
                        gm[j] = __hip_atomic_load(pg + sp * (DD + 2) + DD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        gl[j] = __hip_atomic_load(pg + sp * (DD + 2) + DD + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        go[j] = __hip_atomic_load(pg + sp * (DD + 2) + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        ok = ok && (unsigned)(gm[j] >> 32) == tag && (unsigned)(gl[j] >> 32) == tag && (unsigned)(go[j] >> 32) == tag;
                    if (ok) break;
                    __builtin_amdgcn_s_sleep(2);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (sb + j >= a.nsplit) break;
                    const float msj = (unsigned)(gm[j] >> 32) == tag ? __uint_as_float((unsigned)gm[j]) : __builtin_nanf("");
                    const float lsj = __uint_as_float((unsigned)gl[j]), osj = __uint_as_float((unsigned)go[j]);
                    float aa, c;
                    softmax_merge(mm, ll, msj, lsj, aa, c);
                    oo = oo * aa + osj * c;
                }
            }
            ((T*)a.out)[(int64_t)b * a.o_sb + (int64_t)(kvh * G + g) * DD + d] = from_f32<T>(ll > 0.f ? oo / ll : 0.f);
        }
        DSTAMP(9);
        DSTAMP(10);
        DTRACE_FLUSH((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x, 4);
        return;
    }
    // ---- arrival; the last block of this (batch, KV head) combines
    DSTAMP(6);
    __threadfence();
    DSTAMP(7);
    __syncthreads();
    int* cnt = a.counters + (int64_t)b * a.Hk + kvh;
    if (tid == 0) {
        const int old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_s = old == a.nsplit - 1;
    }
    __syncthreads();
    DSTAMP(8);
    if (!last_s) {
        DTRACE_FLUSH((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x, 4);
        return;
    }
    __threadfence();
    DSTAMP(9);
    for (int i = tid; i < G * DD; i += 256) {
        const int g = i / DD, d = i - g * DD;
        const float* pp = a.part + part_index<DD>((int64_t)b * a.Hq + kvh * G + g, a.nsplit, 0);
        ((T*)a.out)[(int64_t)b * a.o_sb + (int64_t)(kvh * G + g) * DD + d] = from_f32<T>(combine_splits<DD>(pp, a.nsplit, d));
    }
    if (tid == 0) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    DSTAMP(10);
    DTRACE_FLUSH((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x, 4);
}

}  // namespace

#ifdef UAMD_DECODE_TRACE
extern "C" int uamd_debug_decode_trace(unsigned long long* buf) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_dec_trace), &buf, sizeof(buf));
}
#endif

// y_g[n] = W_g[n, :] . x  (+ s_g * B_g[n, :] . t_g + bias_g[n]) for up to 4 row groups sharing x (one token).
// nf4 != 0: W_g is bitsandbytes-format NF4 (packed [N, K/2], absmax per `blocksize` codes, nested when absmax_u8 is
// given: all groups of a launch share code2). Replaces fast_gemv / the bsz == 1 branch of fast_linear_forward
// (unsloth/kernels/utils.py:872-977, :1082-1125) in ONE launch instead of cdequantize_blockwise_fp32 +
// cgemm_4bit_inference_naive + mv + addmv.
static int gemv_entry(const void* x, int K, const uamd_gemv_group* groups, int n_groups, int nf4, int blocksize,
                      int dtype, void* stream, const uamd_gemv_prologue* pro) {
    const int mode = pro ? pro->mode : 0;
    if (!groups || n_groups < 1 || n_groups > UAMD_GEMV_MAX_GROUPS || K <= 0 || mode < 0 || mode > 2) return UAMD_ERR_ARG;
    if (!x && mode != 2) return UAMD_ERR_ARG;
    if ((K & 7) || (x && !aligned16(x))) return UAMD_ERR_ALIGN;
    if (mode == 1 && (!pro->x2 || !aligned16(pro->x2))) return UAMD_ERR_ARG;
    if (mode == 2 && (!pro->res || !pro->norm_w || !aligned16(pro->res) || (pro->h_out && !aligned16(pro->h_out)))) return UAMD_ERR_ARG;
    if (pro && pro->a_rows && (pro->Rt <= 0 || pro->Rt > 256 || (pro->ld_a & 7) || !aligned16(pro->a_rows) || !pro->sync ||
                               ((uintptr_t)pro->sync & 7) || (pro->tag == 0 && !pro->tag_dev))) return UAMD_ERR_ARG;
    const int glu = pro ? pro->glu : 0;
    if (glu && (n_groups != 2 || groups[0].N != groups[1].N || groups[0].y_f32 || K > 8192)) return UAMD_ERR_ARG;
    if (nf4 && (blocksize < 32 || (blocksize & 31) || (K & 31))) return UAMD_ERR_ARG;
    GemvArgs a;
    auto log2_exact = [](int v) { int sft = 0; while ((1 << sft) < v) ++sft; return (1 << sft) == v ? sft : -1; };
    a.x = x; a.K = K; a.n_groups = n_groups; a.bs_shift = nf4 ? log2_exact(blocksize) : 0;
    if (a.bs_shift < 0) return UAMD_ERR_ARG;
    int rows = 0;
    for (int i = 0; i < UAMD_GEMV_MAX_GROUPS; ++i) {
        a.row_start[i] = rows;
        if (i < n_groups) {
            const uamd_gemv_group& g = groups[i];
            if (!g.W || !g.y || g.N <= 0) return UAMD_ERR_ARG;
            if (!aligned16(g.W)) return UAMD_ERR_ALIGN;
            if (nf4) {
                if (!g.absmax_f32 && !(g.absmax_u8 && g.code2 && g.absmax2 && g.blocksize2 > 0)) return UAMD_ERR_ARG;
            } else if (g.ldw & 7) {
                return UAMD_ERR_ALIGN;
            }
            if ((g.lora_t || (pro && pro->a_rows && g.lora_b)) && (!g.lora_b || g.R <= 0 || g.R > 64)) return UAMD_ERR_ARG;
            if (pro && pro->a_rows && g.lora_b && (pro->t_off[i] < 0 || pro->t_off[i] + g.R > pro->Rt)) return UAMD_ERR_ARG;
            a.g[i] = g;
            if (!(g.lora_t || (pro && pro->a_rows))) a.g[i].lora_b = nullptr;      // (a B without any t: no LoRA term)
            if (nf4 && !g.absmax_f32) {
                a.g[i].blocksize2 = log2_exact(g.blocksize2);
                if (a.g[i].blocksize2 < 0) return UAMD_ERR_ARG;
            }
            rows += g.N;
        } else {
            a.g[i] = groups[0];
        }
        const uamd_gemv_group& h = a.g[i];
        const bool dir = nf4 && h.absmax_f32;
        a.hW[i] = h.W;
        a.hA[i] = dir ? (const void*)h.absmax_f32 : (const void*)h.absmax_u8;
        a.hA2[i] = h.absmax2;
        a.hB[i] = h.lora_b;                              // (already NULL when the group has no LoRA term)
        a.hldw[i] = h.ldw;
        if (h.lora_b && (h.ld_lb < 0 || h.ld_lb > 0x7fffffffLL)) return UAMD_ERR_ARG;
        a.hldb[i] = (int)h.ld_lb;
        a.hN[i] = h.N;
        a.hmeta[i] = (nf4 && !dir ? h.blocksize2 : 0) | (dir ? 1 << 8 : 0) | (h.lora_b_f32 ? 1 << 9 : 0) | ((h.lora_b ? h.R : 0) << 16);
    }
    a.row_start[UAMD_GEMV_MAX_GROUPS] = rows;
    a.total_rows = rows;                              // (glu: 2 N virtual rows, gate and up rows interleaved)
    a.n_tb = 0;
    a.t_ks = 1;
    a.t_kp = 4096;
    if (pro) {
        a.pro = *pro;
        if (pro->a_rows) {                            // a wave of a t workgroup holds <= 8 vectors (4096 columns) of its A row
            int ks = 1;
            while (ks < 8 && ks * 4096 < K) ks *= 2;
            if (ks * 4096 < K) return UAMD_ERR_ARG;      // K <= 32768
            a.t_ks = ks;
            a.t_kp = ((K + ks - 1) / ks + 511) / 512 * 512;
            a.n_tb = (pro->Rt * ks + GEMV_THREADS / 64 - 1) / (GEMV_THREADS / 64);
        }
    } else {
        a.pro.mode = 0; a.pro.x2 = nullptr; a.pro.res = nullptr; a.pro.norm_w = nullptr; a.pro.h_out = nullptr;
        a.pro.a_rows = nullptr; a.pro.ld_a = 0; a.pro.Rt = 0; a.pro.w_f32 = 0; a.pro.eps = 0.f; a.pro.glu = 0;
        a.pro.sync = nullptr; a.pro.tag = 0; a.pro.tag_dev = nullptr;
        for (int i = 0; i < UAMD_GEMV_MAX_GROUPS; ++i) a.pro.t_off[i] = 0;
    }
    hipStream_t st = (hipStream_t)stream;
    UAMD_DISPATCH_HALF(dtype, return nf4 ? launch_gemv<T, true>(a, st) : launch_gemv<T, false>(a, st))
    return UAMD_ERR_DTYPE;
}

extern "C" int uamd_gemv(const void* x, int K, const uamd_gemv_group* groups, int n_groups, int nf4, int blocksize,
                         int dtype, void* stream) {
    return gemv_entry(x, K, groups, n_groups, nf4, blocksize, dtype, stream, nullptr);
}

// uamd_gemv with the token PRODUCED inside the launch (one decoder-layer step = 5 launches instead of 14):
//   pro->mode 1: x = SwiGLU(x, x2)                       (fast_swiglu_inference, llama.py:572-606: down_proj's input)
//   pro->mode 2: h = x + res (x may be NULL), x' = rmsnorm(h) * norm_w; block 0 writes h to h_out   (the residual add +
//                fast_rms_layernorm_inference in front of q|k|v, gate|up and lm_head, llama.py:1249-1364)
//   pro->a_rows: t = A x for the stacked LoRA A rows [Rt, K], computed ONCE by the launch's first ceil(Rt / 8) workgroups
//                and handed to the others through pro->sync; group g reads t[t_off[g] ..]
//                (the `mv` of fast_linear_forward, utils.py:1107-1117, without a launch of its own)
//   pro->glu:    gate | up in, h = SwiGLU out (the launch of fast_swiglu_inference's elementwise kernel disappears)
extern "C" int uamd_gemv_fused(const void* x, int K, const uamd_gemv_group* groups, int n_groups, int nf4, int blocksize,
                               int dtype, void* stream, const uamd_gemv_prologue* pro) {
    return gemv_entry(x, K, groups, n_groups, nf4, blocksize, dtype, stream, pro);
}

// Y_g[m, n] = W_g[n, :] . X[m, :] (+ s_g * B_g[n, :] . T_g[m, :] + bias_g[n]) for M = 1 .. 16 token rows in ONE pass over the
// weights: the decode step of a batch (gemv_rows_kernel). The groups are uamd_gemv's; every group's y and lora_t address
// rows of stride ldy / ldt.
static int gemv_rows_entry(const void* x, int64_t ldx, int M, int max_m, int K, const uamd_gemv_group* groups, int n_groups,
                           int64_t ldy, int64_t ldt, int nf4, int blocksize, int dtype, void* stream) {
    if (!x || !groups || n_groups < 1 || n_groups > UAMD_GEMV_MAX_GROUPS || M < 1 || M > max_m || K <= 0 || K > 16384 || ldx < K ||
        ldy < 1 || ldt < 0)
        return UAMD_ERR_ARG;
    if (nf4 && (blocksize < 32 || (blocksize & 31) || (K & 31))) return UAMD_ERR_ARG;
    if ((K & 7) || (ldx & 7) || !aligned16(x)) return UAMD_ERR_ALIGN;
    auto log2_exact = [](int v) { int sft = 0; while ((1 << sft) < v) ++sft; return (1 << sft) == v ? sft : -1; };
    GemvRowsArgs a;
    a.x = x; a.ldx = ldx; a.ldy = ldy; a.ldt = ldt; a.M = M; a.K = K; a.n_groups = n_groups;
    a.bs_shift = nf4 ? log2_exact(blocksize) : 0;
    if (a.bs_shift < 0) return UAMD_ERR_ARG;
    for (int i = 0; i < UAMD_GEMV_MAX_GROUPS; ++i) {
        a.g[i] = groups[i < n_groups ? i : 0];
        if (i >= n_groups) continue;
        uamd_gemv_group& g = a.g[i];
        if (!g.W || !g.y || g.N <= 0) return UAMD_ERR_ARG;
        if (!aligned16(g.W)) return UAMD_ERR_ALIGN;
        if (nf4) {
            if (!g.absmax_f32 && !(g.absmax_u8 && g.code2 && g.absmax2 && g.blocksize2 > 0)) return UAMD_ERR_ARG;
            if (!g.absmax_f32 && (g.blocksize2 = log2_exact(g.blocksize2)) < 0) return UAMD_ERR_ARG;
        } else if (g.ldw < K) {
            return UAMD_ERR_ARG;
        } else if (g.ldw & 7) {
            return UAMD_ERR_ALIGN;
        }
        if (g.lora_t && (!g.lora_b || g.R <= 0 || g.R > 64 || g.ld_lb < g.R || ldt < g.R)) return UAMD_ERR_ARG;
        if (!g.lora_t) g.lora_b = nullptr;            // (a B without a t: no LoRA term)
    }
    hipStream_t st = (hipStream_t)stream;
    UAMD_DISPATCH_HALF(dtype, return nf4 ? launch_gemv_rows_wide<T, true>(a, st) : launch_gemv_rows_wide<T, false>(a, st))
    return UAMD_ERR_DTYPE;
}
extern "C" int uamd_gemv_rows(const void* x, int64_t ldx, int M, int K, const uamd_gemv_group* groups, int n_groups,
                              int64_t ldy, int64_t ldt, int nf4, int blocksize, int dtype, void* stream) {
    return gemv_rows_entry(x, ldx, M, 16, K, groups, n_groups, ldy, ldt, nf4, blocksize, dtype, stream);
}
// The same for M = 1 .. 64 (17 and up: the kernel's MT = 2 | 4 token-tile instances; M <= 16: uamd_gemv_rows' launch). Y[m, n]
// is bit for bit what uamd_gemv_rows stores for that token row and weight row.
extern "C" int uamd_gemv_rows64(const void* x, int64_t ldx, int M, int K, const uamd_gemv_group* groups, int n_groups,
                                int64_t ldy, int64_t ldt, int nf4, int blocksize, int dtype, void* stream) {
    return gemv_rows_entry(x, ldx, M, 64, K, groups, n_groups, ldy, ldt, nf4, blocksize, dtype, stream);
}

// RoPE on the new token's q, k (in place in the fused qkv row) + append of k, v at cache position kv_len[b]
// (replaces llama.py:468-497). cos / sin: [positions, >= D/2] tables; rope_pos NULL = kv_len.
extern "C" int uamd_rope_kv_append(void* qkv, int64_t ld_qkv, const void* cos_t, const void* sin_t, int64_t ld_cs,
                                   const int* kv_len, const int* rope_pos, void* k_cache, void* v_cache,
                                   int64_t cache_sb, int64_t cache_sh, int B, int Hq, int Hk, int D, int s_max,
                                   int dtype, void* stream) {
    if (!qkv || !cos_t || !sin_t || !kv_len || !k_cache || !v_cache || B <= 0 || Hq <= 0 || Hk <= 0 || D <= 0 || (D & 1))
        return UAMD_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    UAMD_DISPATCH_HALF(dtype, hipLaunchKernelGGL((rope_append_kernel<T>), dim3(Hq + 2 * Hk, B), dim3(64), 0, st, (T*)qkv, ld_qkv,
                                                 (const T*)cos_t, (const T*)sin_t, ld_cs, kv_len, rope_pos, (T*)k_cache,
                                                 (T*)v_cache, cache_sb, cache_sh, Hq, Hk, D, s_max))
    return uamd_launch_status();
}

namespace {
// What uamd_attn_decode and uamd_attn_decode_fused ask of the geometry and the cache alike; split_keys: a multiple of the keys
// per block-load (DecGeo<D>::KPB).
int attn_decode_check(int Hq, int Hk, int D, int nsplit, int split_keys, const void* k_cache, const void* v_cache,
                      int64_t cache_sb, int64_t cache_sh) {
    if (Hq % Hk || (D != 64 && D != 128) || nsplit <= 0 || split_keys <= 0) return UAMD_ERR_ARG;
    if (split_keys % (D == 64 ? DecGeo<64>::KPB : DecGeo<128>::KPB)) return UAMD_ERR_ARG;
    if (!aligned16(k_cache) || !aligned16(v_cache) || (cache_sb & 7) || (cache_sh & 7)) return UAMD_ERR_ALIGN;
    return UAMD_OK;
}

// f(T(), G, D as std::integral_constant) for the instantiations of the decode attention kernels: both 16-bit types, head dim
// 64 / 128 (checked before), every group size up to 8 (the kernels loop over their G query heads; Qwen2.5-7B / Qwen2-VL-7B:
// G = 7).
template <int N> using IntC = std::integral_constant<int, N>;
template <typename F>
int attn_decode_dispatch(int dtype, int D, int G, F&& f) {
    auto over_g = [&](auto t, auto dd) -> int {
        switch (G) {
            case 1: return f(t, IntC<1>(), dd); case 2: return f(t, IntC<2>(), dd); case 3: return f(t, IntC<3>(), dd);
            case 4: return f(t, IntC<4>(), dd); case 5: return f(t, IntC<5>(), dd); case 6: return f(t, IntC<6>(), dd);
            case 7: return f(t, IntC<7>(), dd); case 8: return f(t, IntC<8>(), dd);
            default: return UAMD_ERR_ARG;
        }
    };
    UAMD_DISPATCH_HALF(dtype, return D == 128 ? over_g(T(), IntC<128>()) : over_g(T(), IntC<64>()))
}

// How many blocks of attn_decode_fused_kernel<T, G, DD> are CERTAINLY resident at once on the current device: one per compute
// unit THIS device has (a CPX / SPX partition reports its own CU count), and none when a block does not fit a CU at all.
// The granule combine polls for the other splits' partials, so a launch larger than this must not take it (a block that
// starts only after another exits would be waited for in vain: 2^18 polls, then NaN). Cached per device and instantiation.
template <typename T, int G, int DD>
int attn_fused_resident_blocks() {
    static int cap[UAMD_DEVICE_SLOTS];
    const int dev = uamd_device_slot_or_neg();
    if (dev < 0) return 0;
    if (cap[dev] == 0) {
        int per_cu = 0;
        const int cus = uamd_cu_count();
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, attn_decode_fused_kernel<T, G, DD>, 256, 0) != hipSuccess || cus == 0) {
            (void)hipGetLastError();
            return 0;
        }
        cap[dev] = per_cu >= 1 ? cus : -1;
    }
    return cap[dev] > 0 ? cap[dev] : 0;
}
}  // namespace

// out[b, h, :] = softmax(q[b, h] . K[b, h / G, first..len) * scale) V  over the cache (len = kv_len[b] + len_add;
// window > 0: only the last `window` keys). partials: fp32 workspace [B, Hq, nsplit, D + 2]. Replaces
// llama.py:499-543 (expand + matmul + softmax + matmul, or SDPA).
extern "C" int uamd_attn_decode(const void* q, int64_t q_sb, const void* k_cache, const void* v_cache, int64_t cache_sb,
                                int64_t cache_sh, const int* kv_len, int len_add, float* partials, void* out,
                                int64_t out_sb, int B, int Hq, int Hk, int D, int nsplit, int split_keys, int window,
                                float scale, int dtype, void* stream) {
    if (!q || !k_cache || !v_cache || !kv_len || !partials || !out || B <= 0 || Hq <= 0 || Hk <= 0) return UAMD_ERR_ARG;
    if (int rc = attn_decode_check(Hq, Hk, D, nsplit, split_keys, k_cache, v_cache, cache_sb, cache_sh)) return rc;
    if (!aligned16(q) || (q_sb & 7)) return UAMD_ERR_ALIGN;
    const float sl2 = scale * 1.4426950408889634f;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nsplit, (unsigned)Hk, (unsigned)B);
    return attn_decode_dispatch(dtype, D, Hq / Hk, [&](auto t, auto g, auto dd) -> int {
        using T = decltype(t);
        constexpr int G = decltype(g)::value, DD = decltype(dd)::value;
        hipLaunchKernelGGL((attn_decode_kernel<T, G, DD>), grid, dim3(256), 0, st, (const T*)q, q_sb, (const T*)k_cache,
                           (const T*)v_cache, cache_sb, cache_sh, kv_len, partials, Hq, nsplit, split_keys, window, sl2, len_add);
        if (int rc = uamd_launch_status()) return rc;
        hipLaunchKernelGGL((attn_decode_combine_kernel<T, DD>), dim3(Hq, B), dim3(DD), 0, st, partials, (T*)out, out_sb, Hq, nsplit);
        return uamd_launch_status();
    });
}

// uamd_attn_decode for P groups of n_share rows that share their first prompt_len[p] keys (include/unsloth_amd.h). Three plain
// launches on one stream: attn_decode_prefix_kernel over the shared prompt caches -> partial slots [0, nsplit_prompt) of every
// row; attn_decode_kernel, as it is, over the per-row suffix caches with kv_len = new_len -> slots [nsplit_prompt, nsplit_prompt +
// nsplit_new) (the first-slot offset rides in the partials pointer, the total split count is the stride); the combine over all.
extern "C" int uamd_attn_decode_shared(const void* q, int64_t q_sb, const void* pk, const void* pv, int64_t p_sb, int64_t p_sh,
                                       const int* prompt_len, int n_share, const void* sk, const void* sv, int64_t s_sb,
                                       int64_t s_sh, const int* new_len, int len_add, float* partials, void* out, int64_t out_sb,
                                       int P, int Hq, int Hk, int D, int nsplit_prompt, int nsplit_new, int split_keys,
                                       int window, float scale, int dtype, void* stream) {
    if (!q || !prompt_len || !new_len || !partials || !out || P <= 0 || Hq <= 0 || Hk <= 0) return UAMD_ERR_ARG;
    if (n_share < 2 || n_share > 16) return UAMD_ERR_ARG;
    if (!pk || !pv || !sk || !sv) return UAMD_ERR_ARG;
    if (int rc = attn_decode_check(Hq, Hk, D, nsplit_prompt, split_keys, pk, pv, p_sb, p_sh)) return rc;
    if (int rc = attn_decode_check(Hq, Hk, D, nsplit_new, split_keys, sk, sv, s_sb, s_sh)) return rc;
    if (Hq / Hk > 8) return UAMD_ERR_ARG;
    if (!aligned16(q) || (q_sb & 7)) return UAMD_ERR_ALIGN;
    const float sl2 = scale * 1.4426950408889634f;
    hipStream_t st = (hipStream_t)stream;
    const int B = P * n_share, nsplit = nsplit_prompt + nsplit_new;
    return attn_decode_dispatch(dtype, D, Hq / Hk, [&](auto t, auto g, auto dd) -> int {
        using T = decltype(t);
        constexpr int G = decltype(g)::value, DD = decltype(dd)::value;
        if (int rc = uamd_launch_lds<&attn_decode_prefix_kernel<T, DD>>(
                dim3((unsigned)nsplit_prompt, (unsigned)Hk, (unsigned)P), dim3(256), SharedGeo<DD>::LDS, st, (const T*)q, q_sb,
                (const T*)pk, (const T*)pv, p_sb, p_sh, prompt_len, new_len, partials, n_share, G, Hq, nsplit, split_keys, window,
                sl2, len_add))
            return rc;
        hipLaunchKernelGGL((attn_decode_kernel<T, G, DD>), dim3((unsigned)nsplit_new, (unsigned)Hk, (unsigned)B), dim3(256), 0, st,
                           (const T*)q, q_sb, (const T*)sk, (const T*)sv, s_sb, s_sh, new_len,
                           partials + (int64_t)nsplit_prompt * (DD + 2), Hq, nsplit, split_keys, window, sl2, len_add);
        if (int rc = uamd_launch_status()) return rc;
        hipLaunchKernelGGL((attn_decode_combine_kernel<T, DD>), dim3(Hq, B), dim3(DD), 0, st, partials, (T*)out, out_sb, Hq, nsplit);
        return uamd_launch_status();
    });
}

// ---- a span of R new tokens per sequence in one step (include/unsloth_amd.h): the append, the attention, and the draft /
//      accept kernels of prompt-lookup decoding.
extern "C" int uamd_rope_kv_append_span(void* qkv, int64_t ld_qkv, const void* cos_t, const void* sin_t, int64_t ld_cs,
                                        const int* kv_len, void* k_cache, void* v_cache, int64_t cache_sb, int64_t cache_sh,
                                        int B, int R, int Hq, int Hk, int D, int s_max, int dtype, void* stream) {
    if (!qkv || !cos_t || !sin_t || !kv_len || !k_cache || !v_cache || B <= 0 || R <= 0 || Hq <= 0 || Hk <= 0 || D <= 0 || (D & 1))
        return UAMD_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    UAMD_DISPATCH_HALF(dtype, hipLaunchKernelGGL((rope_append_span_kernel<T>), dim3(Hq + 2 * Hk, B * R), dim3(64), 0, st, (T*)qkv,
                                                 ld_qkv, (const T*)cos_t, (const T*)sin_t, ld_cs, kv_len, (T*)k_cache,
                                                 (T*)v_cache, cache_sb, cache_sh, R, Hq, Hk, D, s_max))
    return uamd_launch_status();
}

extern "C" int uamd_attn_decode_span(const void* q, int64_t q_sb, const void* k_cache, const void* v_cache, int64_t cache_sb,
                                     int64_t cache_sh, const int* kv_len, int R, float* partials, void* out, int64_t out_sb,
                                     int B, int Hq, int Hk, int D, int nsplit, int split_keys, int window, float scale, int dtype,
                                     void* stream) {
    if (!q || !k_cache || !v_cache || !kv_len || !partials || !out || B <= 0 || Hq <= 0 || Hk <= 0) return UAMD_ERR_ARG;
    if (R < 1 || R > 16 || window < 0) return UAMD_ERR_ARG;
    if (int rc = attn_decode_check(Hq, Hk, D, nsplit, split_keys, k_cache, v_cache, cache_sb, cache_sh)) return rc;
    const int G = Hq / Hk;
    if (R * G > 128) return UAMD_ERR_ARG;
    if (!aligned16(q) || (q_sb & 7)) return UAMD_ERR_ALIGN;
    const float sl2 = scale * 1.4426950408889634f;
    hipStream_t st = (hipStream_t)stream;
    UAMD_DISPATCH_HALF(dtype, {
        auto launch = [&](auto dd) -> int {
            constexpr int DD = decltype(dd)::value;
            if (int rc = uamd_launch_lds<&attn_decode_span_kernel<T, DD>>(
                    dim3((unsigned)nsplit, (unsigned)Hk, (unsigned)B), dim3(256), SharedGeo<DD>::LDS, st, (const T*)q, q_sb,
                    (const T*)k_cache, (const T*)v_cache, cache_sb, cache_sh, kv_len, partials, R, G, Hq, nsplit, split_keys,
                    window, sl2))
                return rc;
            hipLaunchKernelGGL((attn_decode_combine_kernel<T, DD>), dim3(Hq, B * R), dim3(DD), 0, st, partials, (T*)out, out_sb, Hq,
                               nsplit);
            return uamd_launch_status();
        };
        return D == 128 ? launch(IntC<128>()) : launch(IntC<64>());
    })
}

extern "C" int uamd_ngram_draft(const int64_t* hist, const int* hist_len, int cap, int n_max, int K, int64_t* tok, int* n_draft,
                                void* stream) {
    if (!hist || !hist_len || !tok || !n_draft || cap <= 0 || n_max < 1 || K < 1 || K > 15) return UAMD_ERR_ARG;
    hipLaunchKernelGGL(ngram_draft_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const long long*)hist, hist_len, cap, n_max,
                       K, (long long*)tok, n_draft);
    return uamd_launch_status();
}

extern "C" int uamd_accept_greedy(const int64_t* tok, const int64_t* amax, int K, const int64_t* eos, int n_eos, int64_t* hist,
                                  int cap, int* hist_len, int* kv_len, int* remaining, int* done, const int* n_draft,
                                  int64_t* stats, void* stream) {
    if (!tok || !amax || !hist || !hist_len || !kv_len || !remaining || !done || !n_draft || !stats) return UAMD_ERR_ARG;
    if (K < 0 || K > 15 || n_eos < 0 || n_eos > 8 || (n_eos > 0 && !eos) || cap <= 0) return UAMD_ERR_ARG;
    hipLaunchKernelGGL(accept_greedy_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const long long*)tok,
                       (const long long*)amax, K, (const long long*)eos, n_eos, (long long*)hist, cap, hist_len, kv_len, remaining,
                       done, n_draft, (long long*)stats);
    return uamd_launch_status();
}

// ---- the FP8 KV cache (format: include/unsloth_amd.h). Codes [B, Hk, s_max, D] uint8 with strides (cache_sb, cache_sh, D, 1),
//      scales [B, Hk, s_max] fp32 with strides (cache_sb / D, cache_sh / D, 1).
static int fp8_cache_check(int D, const void* codes, const void* scales, int64_t cache_sb, int64_t cache_sh) {
    if (D != 64 && D != 128) return UAMD_ERR_ARG;
    if (!codes || !scales || cache_sb <= 0 || cache_sh <= 0) return UAMD_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(codes) & 7) || (reinterpret_cast<uintptr_t>(scales) & 3) || cache_sb % D || cache_sh % D)
        return UAMD_ERR_ALIGN;
    return UAMD_OK;
}

extern "C" int uamd_kv_store_fp8(const void* src, int64_t src_sb, int64_t src_sh, int64_t src_st, void* codes, float* scales,
                                 int64_t cache_sb, int64_t cache_sh, int B, int Hk, int Tn, int D, int s_max, int dtype,
                                 void* stream) {
    if (!src || B <= 0 || Hk <= 0 || Tn <= 0 || Tn > s_max) return UAMD_ERR_ARG;
    if (int rc = fp8_cache_check(D, codes, scales, cache_sb, cache_sh)) return rc;
    if (cache_sh < (int64_t)s_max * D || cache_sb < (int64_t)Hk * cache_sh) return UAMD_ERR_ARG;
    if (!aligned16(src) || (src_sb & 7) || (src_sh & 7) || (src_st & 7)) return UAMD_ERR_ALIGN;
    const int64_t rows = (int64_t)B * Hk * Tn;
    const int kpb = D == 128 ? DecGeo<128>::KPB : DecGeo<64>::KPB;
    const int64_t blocks = (rows + kpb - 1) / kpb;
    if (blocks > 0x7fffffff) return UAMD_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    UAMD_DISPATCH_HALF(dtype, {
        if (D == 128)
            hipLaunchKernelGGL((kv_store_fp8_kernel<T, 128>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)src, src_sb, src_sh,
                               src_st, (uint8_t*)codes, scales, cache_sb, cache_sh, Hk, Tn, rows);
        else
            hipLaunchKernelGGL((kv_store_fp8_kernel<T, 64>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)src, src_sb, src_sh,
                               src_st, (uint8_t*)codes, scales, cache_sb, cache_sh, Hk, Tn, rows);
    })
    return uamd_launch_status();
}

extern "C" int uamd_rope_kv_append_fp8(void* qkv, int64_t ld_qkv, const void* cos_t, const void* sin_t, int64_t ld_cs,
                                       const int* kv_len, const int* rope_pos, void* k_codes, void* v_codes, float* k_scales,
                                       float* v_scales, int64_t cache_sb, int64_t cache_sh, int B, int Hq, int Hk, int D,
                                       int s_max, int dtype, void* stream) {
    if (!qkv || !cos_t || !sin_t || !kv_len || B <= 0 || Hq <= 0 || Hk <= 0 || s_max <= 0) return UAMD_ERR_ARG;
    if (int rc = fp8_cache_check(D, k_codes, k_scales, cache_sb, cache_sh)) return rc;
    if (int rc = fp8_cache_check(D, v_codes, v_scales, cache_sb, cache_sh)) return rc;
    if (cache_sh < (int64_t)s_max * D || cache_sb < (int64_t)Hk * cache_sh) return UAMD_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(Hq + 2 * Hk), (unsigned)B);
    UAMD_DISPATCH_HALF(dtype, {
        if (D == 128)
            hipLaunchKernelGGL((rope_append_fp8_kernel<T, 128>), grid, dim3(64), 0, st, (T*)qkv, ld_qkv, (const T*)cos_t,
                               (const T*)sin_t, ld_cs, kv_len, rope_pos, (uint8_t*)k_codes, k_scales, (uint8_t*)v_codes, v_scales,
                               cache_sb, cache_sh, Hq, Hk, s_max);
        else
            hipLaunchKernelGGL((rope_append_fp8_kernel<T, 64>), grid, dim3(64), 0, st, (T*)qkv, ld_qkv, (const T*)cos_t,
                               (const T*)sin_t, ld_cs, kv_len, rope_pos, (uint8_t*)k_codes, k_scales, (uint8_t*)v_codes, v_scales,
                               cache_sb, cache_sh, Hq, Hk, s_max);
    })
    return uamd_launch_status();
}

extern "C" int uamd_attn_decode_fp8(const void* q, int64_t q_sb, const void* k_codes, const void* v_codes, const float* k_scales,
                                    const float* v_scales, int64_t cache_sb, int64_t cache_sh, const int* kv_len, int len_add,
                                    float* partials, void* out, int64_t out_sb, int B, int Hq, int Hk, int D, int nsplit,
                                    int split_keys, int window, float scale, int dtype, void* stream) {
    if (!q || !kv_len || !partials || !out || B <= 0 || Hq <= 0 || Hk <= 0) return UAMD_ERR_ARG;
    if (Hq % Hk || nsplit <= 0 || split_keys <= 0) return UAMD_ERR_ARG;
    if (int rc = fp8_cache_check(D, k_codes, k_scales, cache_sb, cache_sh)) return rc;
    if (int rc = fp8_cache_check(D, v_codes, v_scales, cache_sb, cache_sh)) return rc;
    if (split_keys % (D == 64 ? DecGeo<64>::KPB : DecGeo<128>::KPB)) return UAMD_ERR_ARG;
    if (!aligned16(q) || (q_sb & 7)) return UAMD_ERR_ALIGN;
    const float sl2 = scale * 1.4426950408889634f;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nsplit, (unsigned)Hk, (unsigned)B);
    return attn_decode_dispatch(dtype, D, Hq / Hk, [&](auto t, auto g, auto dd) -> int {
        using T = decltype(t);
        constexpr int G = decltype(g)::value, DD = decltype(dd)::value;
        hipLaunchKernelGGL((attn_decode_fp8_kernel<T, G, DD>), grid, dim3(256), 0, st, (const T*)q, q_sb, (const uint8_t*)k_codes,
                           (const uint8_t*)v_codes, k_scales, v_scales, cache_sb, cache_sh, kv_len, partials, Hq, nsplit,
                           split_keys, window, sl2, len_add);
        if (int rc = uamd_launch_status()) return rc;
        hipLaunchKernelGGL((attn_decode_combine_kernel<T, DD>), dim3(Hq, B), dim3(DD), 0, st, partials, (T*)out, out_sb, Hq, nsplit);
        return uamd_launch_status();
    });
}

extern "C" int uamd_attn_decode_fused(const void* qkv, int64_t ld_qkv, const void* cos_t, const void* sin_t, int64_t ld_cs,
                                      const int* kv_len, const int* rope_pos, void* k_cache, void* v_cache,
                                      int64_t cache_sb, int64_t cache_sh, float* partials, int* counters, void* out,
                                      int64_t out_sb, int B, int Hq, int Hk, int D, int s_max, int nsplit, int split_keys,
                                      int window, float scale, unsigned tag, const int* tag_dev, int dtype, void* stream) {
    if (!qkv || !cos_t || !sin_t || !kv_len || !k_cache || !v_cache || !partials || !counters || !out || B <= 0 || Hq <= 0 ||
        Hk <= 0 || s_max <= 0)
        return UAMD_ERR_ARG;
    if (int rc = attn_decode_check(Hq, Hk, D, nsplit, split_keys, k_cache, v_cache, cache_sb, cache_sh)) return rc;
    AttnDecFusedArgs a;
    a.qkv = qkv; a.ld_qkv = ld_qkv; a.cos_t = cos_t; a.sin_t = sin_t; a.ld_cs = ld_cs; a.kv_len = kv_len; a.rope_pos = rope_pos;
    a.kc = k_cache; a.vc = v_cache; a.c_sb = cache_sb; a.c_sh = cache_sh; a.part = partials; a.counters = counters;
    a.out = out; a.o_sb = out_sb; a.Hq = Hq; a.Hk = Hk; a.s_max = s_max; a.nsplit = nsplit; a.split_keys = split_keys;
    a.window = window; a.scale_log2 = scale * 1.4426950408889634f;
    // granule combine only when every block of the launch is certainly resident at once (one 256-thread block per CU of the
    // device this call runs on, attn_fused_resident_blocks): a block polls for the partials of its KV head's other splits
    const int64_t blocks = (int64_t)nsplit * Hk * B;
    const bool want_gran = tag != 0 || tag_dev;                                       // (no tag: the arrival-counter path)
    a.tag = tag;
    a.tag_dev = tag_dev;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nsplit, (unsigned)Hk, (unsigned)B);
    return attn_decode_dispatch(dtype, D, Hq / Hk, [&](auto t, auto g, auto dd) -> int {
        using T = decltype(t);
        constexpr int G = decltype(g)::value, DD = decltype(dd)::value;
        a.gran = (want_gran && blocks <= attn_fused_resident_blocks<T, G, DD>()) ? 1 : 0;
        hipLaunchKernelGGL((attn_decode_fused_kernel<T, G, DD>), grid, dim3(256), 0, st, a);
        return uamd_launch_status();
    });
}

// ---------------------------------------------------------------------------------------------------------------
// Greedy next token of the decode step: argmax over the fp32 logits row (the reference: `logits.argmax(-1)` in HF's generate).
// torch's reduce kernel takes 46 us for the 128,256 logits of one token (profiles/r04z_decode_kernel_stats.csv) -- 1.6 % of the
// step for half a megabyte. Two launches: 64 blocks find (max, first index) of their slices; one block finishes. Ties go to the
// SMALLEST index (torch returns the first maximal element on this path too).
namespace {
struct MaxIdx { float v; long long i; };
__device__ __forceinline__ MaxIdx better(MaxIdx a, MaxIdx b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
__device__ __forceinline__ MaxIdx wave_best(MaxIdx m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        MaxIdx t;
        t.v = __shfl_xor(m.v, o, 64);
        t.i = __shfl_xor(m.i, o, 64);
        m = better(m, t);
    }
    return m;
}
__global__ void __launch_bounds__(256) argmax_part_kernel(const float* __restrict__ x, long long n, float* __restrict__ pv,
                                                          long long* __restrict__ pi) {
    __shared__ float sv[4];
    __shared__ long long si[4];
    const float* row = x + (long long)blockIdx.y * n;
    MaxIdx m = {-INFINITY, n};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = row[i];
        if (v > m.v || (v == m.v && i < m.i) || m.i == n) { m.v = v; m.i = i; }       // (NaN never wins; all-NaN rows: index of the scan's start)
    }
    m = wave_best(m);
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = m.v; si[threadIdx.x >> 6] = m.i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) { MaxIdx t = {sv[w], si[w]}; m = better(m, t); }
        pv[blockIdx.y * gridDim.x + blockIdx.x] = m.v;
        pi[blockIdx.y * gridDim.x + blockIdx.x] = m.i;
    }
}
__global__ void __launch_bounds__(64) argmax_final_kernel(const float* __restrict__ pv, const long long* __restrict__ pi, int parts,
                                                          long long n, long long* __restrict__ out) {
    MaxIdx m = {-INFINITY, n};
    for (int i = threadIdx.x; i < parts; i += 64) { MaxIdx t = {pv[blockIdx.x * parts + i], pi[blockIdx.x * parts + i]}; m = better(m, t); }
    m = wave_best(m);
    if (threadIdx.x == 0) out[blockIdx.x] = m.i < n ? m.i : 0;
}
}  // namespace

// out[r] = argmax_i x[r, i] over `rows` contiguous fp32 rows of n entries; workspace: rows * 64 floats + rows * 64 int64.
extern "C" int uamd_argmax_f32(const float* x, int rows, int64_t n, float* ws_val, int64_t* ws_idx, int64_t* out, void* stream) {
    if (!x || !ws_val || !ws_idx || !out || rows <= 0 || n <= 0) return UAMD_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(argmax_part_kernel, dim3(64, (unsigned)rows), dim3(256), 0, st, x, (long long)n, ws_val, (long long*)ws_idx);
    hipLaunchKernelGGL(argmax_final_kernel, dim3((unsigned)rows), dim3(64), 0, st, ws_val, (const long long*)ws_idx, 64, (long long)n,
                       (long long*)out);
    return uamd_launch_status();
}
