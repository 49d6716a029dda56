// The fused cross-attention of fgs_attn.hip with 16-bit tensors (fp16 or bf16) on the 16-bit-input matrix cores
// (v_mfma_f32_32x32x16_f16 / _bf16): the distillation decoder's attention under mixed precision.  Definition, NaN rule and dropout's
// keep function are the fp32 entry points' (include/fgs.h); the numerical contract -- what is rounded to 16 bits and what is not --
// stands there under fgs_attn_half_*.  In short: every product takes 16-bit operands and accumulates in fp32; the scores, the online
// softmax, delta and the saved row constant are fp32; only P (before the value product) and dS (before the key / query products) are
// rounded, to nearest even; the outputs are rounded once at the store.  No float atomics, every sum in a fixed order.
//
// Lane maps of the 32x32x16 forms (lane l, l31 = l & 31, lh = l >> 5): lane l holds A[i = l31][k = 8 lh ... 8 lh + 7] and
// B[k = 8 lh ... 8 lh + 7][j = l31], eight 16-bit values each; result register r of lane l is C[row = crow(r, lh)][column = l31],
// crow(r, lh) = (r & 3) + 8 (r >> 2) + 4 lh, as for 32x32x2.
//
// The tiling is fgs_attn.hip's: 4 waves, 128 queries (keys in k_half_bwd_kv) per workgroup, the other side through LDS in tiles of
// FGS_ATTN_HALF_KEY_TILE = 32, S^T = K Q^T with the query on the lane, so maximum and sum are in-lane reductions plus one
// __shfl_xor(..., 32).  What differs from a transliteration:
//   first-stage products (S^T = K Q^T, dA^T = V dO^T; S = Q K^T, dA = dO V^T): the A operand is 8 consecutive channels of a tile row,
//     one 16-byte LDS read of the ROW-MAJOR image  rm[row][DP + 8]  (the 8 pad the row stride off the banks and keep it 16-byte aligned);
//     the B operand is the lane's own row in registers, DP / 16 groups of 8 channels (group s: channels 16 s + 8 lh ...);
//   second-stage products (O^T += V^T P^T, dQ^T += K^T dS^T, dV^T += dO^T A, dK^T += Q^T dS): the k index of an MFMA may be permuted
//     when both operands agree.  The lane's registers 8 t ... 8 t + 7 of S^T hold tile rows 16 t + 4 lh + {0..3} and 16 t + 8 + 4 lh +
//     {0..3}: rounded, they ARE the B operand of MFMA t (t = 0, 1), and the A operand is read in that order from the CHANNEL-MAJOR
//     image  cm[channel][32 + 4]  as two 8-byte reads.  The tile load writes both images where a kernel needs both.
//   global memory: rows are d 16-bit values.  16-byte loads and 8-byte stores only when d % 8 == 0 and every tensor's base is 16-byte
//     aligned (AttnGeom::vec, decided on the host); any other d or base runs the same loops element by element.
//
// Compiled with -ffp-contract=off (fresnel_amd/build.py), for fgs_attn.hip's reason: the backward's score S scale must be the forward's
// rounded product, not the inside of an FMA with the subtraction of `saved`.
#include "fgs_internal.h"

#include <math.h>

namespace {

constexpr int QB = FGS_ATTN_QUERY_BLOCK;     // queries per workgroup (forward, query-block backward)
constexpr int KT = FGS_ATTN_HALF_KEY_TILE;   // keys per LDS tile; queries per LDS tile of the key-block backward
constexpr int KB = FGS_ATTN_KEY_BLOCK;       // keys per workgroup of the key-block backward
constexpr int THREADS = 256;
constexpr int RP = 8, CP = 4;                // padding of a row-major / channel-major LDS row, in elements
static_assert(QB == (THREADS / 64) * 32 && KB == (THREADS / 64) * 32 && KT == 32, "a wave owns one 32-wide MFMA tile");

using f32x16 = __attribute__((ext_vector_type(16))) float;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

template <typename T> struct Vec;
template <> struct Vec<_Float16> { using v8 = f16x8; using v4 = f16x4; };
template <> struct Vec<__bf16> { using v8 = bf16x8; using v4 = bf16x4; };

__device__ __forceinline__ f32x16 mfma16(f16x8 a, f16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }

struct AttnGeom {
    int32_t B, N, M, H, d;
    float scale, inv_keep /* 1 / (1 - p) */, inv_m /* 1 / M */;
    uint32_t thr;  // round(p 2^24); 0 = no dropout
    int32_t vec;   // d % 8 == 0 and every tensor of the call starts on a 16-byte boundary
};

enum { ROW_OPEN = 0, ROW_MASKED = 1, ROW_BAD = 2, ROW_NONE = 3 };

__device__ __forceinline__ int crow(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// murmur3's 32-bit finaliser
__device__ __forceinline__ uint32_t fmix32(uint32_t x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}
// include/fgs.h: the keep rule, the fp32 kernels' to the letter.  row_hash = fmix32(row ^ seed_lo)
__device__ __forceinline__ bool kept(uint32_t row_hash, uint32_t m, uint32_t seed_hi, uint32_t thr) {
    return thr == 0u || (fmix32(row_hash ^ seed_hi ^ (m * 0x9E3779B1u)) >> 8) >= thr;  // (thr is uniform: no hash without dropout)
}
__device__ __forceinline__ void read_seed(const AttnGeom &g, const int64_t *__restrict__ seed, uint32_t &lo, uint32_t &hi) {
    lo = hi = 0u;
    if (g.thr) {
        const uint64_t s = (uint64_t)seed[0];
        lo = (uint32_t)s; hi = (uint32_t)(s >> 32);
    }
}

template <typename T>
__device__ __forceinline__ typename Vec<T>::v8 zero8() {
    typename Vec<T>::v8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (T)0.0f;
    return z;
}

// Tile rows [0, KT) of a row-major source (row r at src + r stride; it exists while r < rows and, with `flags`, while the row's flag
// is ROW_OPEN (open_only) or anything but ROW_NONE) -> rm[row][channel] and / or cm[channel][row]; zeros for every other row and
// for the channels beyond d.
template <typename T, int DP, bool RM, bool CM>
__device__ __forceinline__ void stage_tile(T (*rm)[DP + RP], T (*cm)[KT + CP], const T *__restrict__ src, size_t stride, int rows,
                                           const AttnGeom &g, const int *flags, bool open_only, int tid) {
    using v8 = typename Vec<T>::v8;
    if (g.vec) {
        constexpr int CH = DP / 8;
        for (int i = tid; i < KT * CH; i += THREADS) {
            const int r = i / CH, c0 = (i - r * CH) * 8;
            bool in = r < rows && c0 < g.d;
            if (in && flags != nullptr) in = open_only ? flags[r] == ROW_OPEN : flags[r] != ROW_NONE;
            v8 v = zero8<T>();
            if (in) v = *reinterpret_cast<const v8 *>(src + (size_t)r * stride + c0);
            if constexpr (RM) *reinterpret_cast<v8 *>(&rm[r][c0]) = v;
            if constexpr (CM) {
#pragma unroll
                for (int j = 0; j < 8; ++j) cm[c0 + j][r] = v[j];
            }
        }
    } else {
        for (int i = tid; i < KT * DP; i += THREADS) {
            const int r = i / DP, c = i - r * DP;
            bool in = r < rows && c < g.d;
            if (in && flags != nullptr) in = open_only ? flags[r] == ROW_OPEN : flags[r] != ROW_NONE;
            T v = (T)0.0f;
            if (in) v = src[(size_t)r * stride + c];
            if constexpr (RM) rm[r][c] = v;
            if constexpr (CM) cm[c][r] = v;
        }
    }
}

// the lane's own row as the B operand of the first-stage products: group s = channels 16 s + 8 lh ... + 7; zeros beyond d
template <typename T, int DP>
__device__ __forceinline__ void load_row(typename Vec<T>::v8 (&reg)[DP / 16], const T *__restrict__ row, bool live, const AttnGeom &g, int lh) {
    using v8 = typename Vec<T>::v8;
#pragma unroll
    for (int s = 0; s < DP / 16; ++s) {
        const int c0 = 16 * s + 8 * lh;
        v8 v = zero8<T>();
        if (live && c0 < g.d) {
            if (g.vec) v = *reinterpret_cast<const v8 *>(row + c0);
            else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (c0 + j < g.d) v[j] = row[c0 + j];
            }
        }
        reg[s] = v;
    }
}

// accumulators -> the lane's row, rounded once: registers 4 q ... 4 q + 3 of block cb are channels 32 cb + 8 q + 4 lh + {0..3}
template <typename T, int DP>
__device__ __forceinline__ void store_row(T *__restrict__ row, const f32x16 (&acc)[DP / 32], bool zero, const AttnGeom &g, int lh) {
    using v4 = typename Vec<T>::v4;
#pragma unroll
    for (int cb = 0; cb < DP / 32; ++cb)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            const int c0 = cb * 32 + 8 * qd + 4 * lh;
            v4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = zero ? (T)0.0f : (T)acc[cb][4 * qd + j];
            if (g.vec) {
                if (c0 < g.d) *reinterpret_cast<v4 *>(row + c0) = o;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c0 + j < g.d) row[c0 + j] = o[j];
            }
        }
}

// the A operand of second-stage MFMA t of channel row `crow_`: tile rows 16 t + 4 lh + {0..3}, 16 t + 8 + 4 lh + {0..3}
template <typename T>
__device__ __forceinline__ typename Vec<T>::v8 read_cm(const T *crow_, int t, int lh) {
    using v4 = typename Vec<T>::v4;
    const v4 lo = *reinterpret_cast<const v4 *>(crow_ + 16 * t + 4 * lh), hi = *reinterpret_cast<const v4 *>(crow_ + 16 * t + 8 + 4 * lh);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <typename T>
__device__ __forceinline__ typename Vec<T>::v8 round8(const float *x) {
    typename Vec<T>::v8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (T)x[j];  // round to nearest even
    return v;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------
template <typename T, int DP>
__global__ __launch_bounds__(THREADS) void k_half_fwd(AttnGeom g, const void *__restrict__ q_, const void *__restrict__ kv_,
                                                      const uint8_t *__restrict__ row_keep, const int64_t *__restrict__ seed,
                                                      void *__restrict__ out_, float *__restrict__ lse) {
    using v8 = typename Vec<T>::v8;
    const T *__restrict__ q = reinterpret_cast<const T *>(q_), *__restrict__ kv = reinterpret_cast<const T *>(kv_);
    T *__restrict__ out = reinterpret_cast<T *>(out_);
    __shared__ __attribute__((aligned(16))) T sK[KT][DP + RP];
    __shared__ __attribute__((aligned(16))) T sVt[DP][KT + CP];
    constexpr int CB = DP / 32, KS = DP / 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const uint32_t qblocks = ((uint32_t)g.N + QB - 1) / QB;
    const uint32_t bh = blockIdx.x / qblocks, qb = blockIdx.x - bh * qblocks;
    const int b = (int)(bh / (uint32_t)g.H), h = (int)(bh - (uint32_t)b * g.H);
    const int n = (int)(qb * QB) + wave * 32 + l31;
    const bool live = n < g.N;
    const bool masked = live && row_keep != nullptr && row_keep[(size_t)b * g.N + n] == 0;
    uint32_t seed_lo, seed_hi;
    read_seed(g, seed, seed_lo, seed_hi);
    const uint32_t row_hash = fmix32((bh * (uint32_t)g.N + (uint32_t)n) ^ seed_lo);
    const size_t kv_stride = (size_t)2 * g.H * g.d, to_v = (size_t)g.H * g.d;
    const T *kv_bh = kv + ((size_t)b * g.M * 2 * g.H + h) * g.d;  // key 0 of (b, h)

    v8 qreg[KS];
    load_row<T, DP>(qreg, q + (((size_t)b * g.N + (live ? n : 0)) * g.H + h) * g.d, live, g, lh);
    f32x16 O[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[cb][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;
    bool nan_seen = false;

    for (int m0 = 0; m0 < g.M; m0 += KT) {
        __syncthreads();  // the previous tile has been read
        stage_tile<T, DP, true, false>(sK, nullptr, kv_bh + (size_t)m0 * kv_stride, kv_stride, g.M - m0, g, nullptr, false, tid);
        stage_tile<T, DP, false, true>(nullptr, sVt, kv_bh + (size_t)m0 * kv_stride + to_v, kv_stride, g.M - m0, g, nullptr, false, tid);
        __syncthreads();
        f32x16 S;
#pragma unroll
        for (int r = 0; r < 16; ++r) S[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s) S = mfma16(*reinterpret_cast<const v8 *>(&sK[l31][16 * s + 8 * lh]), qreg[s], S);
        float sv[16], tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float x = masked ? -1e4f : S[r] * g.scale;
            if (m0 + crow(r, lh) >= g.M) x = -INFINITY;  // not a key: no part in the maximum, the NaN rule or the sum
            else nan_seen |= x != x;
            sv[r] = x;
            tmax = fmaxf(tmax, x);  // (drops a NaN: nan_seen has it)
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float m_new = fmaxf(m_run, tmax);
        const float m_use = m_new == -INFINITY ? 0.0f : m_new;  // every score so far is -Inf: p = 0, not exp(-Inf + Inf)
        const float alpha = __expf(m_run - m_use);
        float pk[16], rowsum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __expf(sv[r] - m_use);
            rowsum += p;
            pk[r] = kept(row_hash, (uint32_t)(m0 + crow(r, lh)), seed_hi, g.thr) ? p : 0.0f;
        }
        l_run = l_run * alpha + rowsum;
        m_run = m_new;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) O[cb][r] *= alpha;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const v8 pb = round8<T>(pk + 8 * t);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) O[cb] = mfma16(read_cm<T>(sVt[cb * 32 + l31], t, lh), pb, O[cb]);
        }
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32);
    nan_seen = (nan_seen ? 1 : 0) | __shfl_xor(nan_seen ? 1 : 0, 32);
    const bool bad = live && (nan_seen || m_run == INFINITY || m_run == -INFINITY);
    const float inv = g.inv_keep / l_tot;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[cb][r] = bad ? 0.0f : O[cb][r] * inv;
    if (__syncthreads_or(bad ? 1 : 0)) {
        // a bad row's probabilities are 1 / M each, without dropout: the sum of v with weight 1 (exact in 16 bits) on its own lanes
        // only, times 1 / M in fp32 behind the sweep
        for (int m0 = 0; m0 < g.M; m0 += KT) {
            __syncthreads();
            stage_tile<T, DP, false, true>(nullptr, sVt, kv_bh + (size_t)m0 * kv_stride + to_v, kv_stride, g.M - m0, g, nullptr, false, tid);
            __syncthreads();
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float one[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) one[j] = (bad && m0 + crow(8 * t + j, lh) < g.M) ? 1.0f : 0.0f;
                const v8 pb = round8<T>(one);
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) O[cb] = mfma16(read_cm<T>(sVt[cb * 32 + l31], t, lh), pb, O[cb]);
            }
        }
        if (bad) {
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) O[cb][r] *= g.inv_m;
        }
    }
    if (live) {
        store_row<T, DP>(out + (((size_t)b * g.N + n) * g.H + h) * g.d, O, false, g, lh);
        if (lh == 0) lse[(size_t)bh * g.N + n] = bad ? INFINITY : m_run + logf(l_tot);
    }
}

// ---- backward: delta ----------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(THREADS) void k_half_delta(AttnGeom g, const void *__restrict__ out_, const void *__restrict__ g_out_,
                                                        float *__restrict__ delta) {
    using v8 = typename Vec<T>::v8;
    const uint32_t t = blockIdx.x * (uint32_t)THREADS + threadIdx.x;  // (b N + n) H + h
    const uint32_t total = (uint32_t)g.B * (uint32_t)g.N * (uint32_t)g.H;
    if (t >= total) return;
    const uint32_t h = t % (uint32_t)g.H, bn = t / (uint32_t)g.H, b = bn / (uint32_t)g.N, n = bn - b * (uint32_t)g.N;
    const T *o = reinterpret_cast<const T *>(out_) + (size_t)t * g.d, *go = reinterpret_cast<const T *>(g_out_) + (size_t)t * g.d;
    float acc = 0.0f;
    if (g.vec) {
        for (int c = 0; c < g.d; c += 8) {
            const v8 a = *reinterpret_cast<const v8 *>(o + c), bb = *reinterpret_cast<const v8 *>(go + c);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = fmaf((float)a[j], (float)bb[j], acc);
        }
    } else {
        for (int c = 0; c < g.d; ++c) acc = fmaf((float)o[c], (float)go[c], acc);
    }
    delta[((size_t)b * g.H + h) * g.N + n] = acc;
}

// ---- backward by query blocks: g_q ----------------------------------------------------------------------------------------------------
template <typename T, int DP>
__global__ __launch_bounds__(THREADS) void k_half_bwd_q(AttnGeom g, const void *__restrict__ q_, const void *__restrict__ kv_,
                                                        const uint8_t *__restrict__ row_keep, const int64_t *__restrict__ seed,
                                                        const float *__restrict__ lse, const float *__restrict__ delta,
                                                        const void *__restrict__ g_out_, void *__restrict__ g_q_) {
    using v8 = typename Vec<T>::v8;
    const T *__restrict__ q = reinterpret_cast<const T *>(q_), *__restrict__ kv = reinterpret_cast<const T *>(kv_);
    const T *__restrict__ g_out = reinterpret_cast<const T *>(g_out_);
    T *__restrict__ g_q = reinterpret_cast<T *>(g_q_);
    __shared__ __attribute__((aligned(16))) T sK[KT][DP + RP];
    __shared__ __attribute__((aligned(16))) T sV[KT][DP + RP];
    __shared__ __attribute__((aligned(16))) T sKt[DP][KT + CP];
    constexpr int CB = DP / 32, KS = DP / 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const uint32_t qblocks = ((uint32_t)g.N + QB - 1) / QB;
    const uint32_t bh = blockIdx.x / qblocks, qb = blockIdx.x - bh * qblocks;
    const int b = (int)(bh / (uint32_t)g.H), h = (int)(bh - (uint32_t)b * g.H);
    const int n = (int)(qb * QB) + wave * 32 + l31;
    const bool live = n < g.N;
    const bool masked = live && row_keep != nullptr && row_keep[(size_t)b * g.N + n] == 0;
    uint32_t seed_lo, seed_hi;
    read_seed(g, seed, seed_lo, seed_hi);
    const uint32_t row_hash = fmix32((bh * (uint32_t)g.N + (uint32_t)n) ^ seed_lo);
    const float lse_n = live ? lse[(size_t)bh * g.N + n] : 0.0f, delta_n = live ? delta[(size_t)bh * g.N + n] : 0.0f;
    const bool constant = !live || masked || lse_n == INFINITY;  // nothing flows to this row's scores
    const size_t kv_stride = (size_t)2 * g.H * g.d, to_v = (size_t)g.H * g.d;
    const T *kv_bh = kv + ((size_t)b * g.M * 2 * g.H + h) * g.d;

    v8 qreg[KS], dreg[KS];
    {
        const size_t at = (((size_t)b * g.N + (live ? n : 0)) * g.H + h) * g.d;
        load_row<T, DP>(qreg, q + at, live, g, lh);
        load_row<T, DP>(dreg, g_out + at, live, g, lh);
    }
    f32x16 dQ[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) dQ[cb][r] = 0.0f;

    for (int m0 = 0; m0 < g.M; m0 += KT) {
        __syncthreads();
        stage_tile<T, DP, true, true>(sK, sKt, kv_bh + (size_t)m0 * kv_stride, kv_stride, g.M - m0, g, nullptr, false, tid);
        stage_tile<T, DP, true, false>(sV, nullptr, kv_bh + (size_t)m0 * kv_stride + to_v, kv_stride, g.M - m0, g, nullptr, false, tid);
        __syncthreads();
        f32x16 S, dA;
#pragma unroll
        for (int r = 0; r < 16; ++r) { S[r] = 0.0f; dA[r] = 0.0f; }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            S = mfma16(*reinterpret_cast<const v8 *>(&sK[l31][16 * s + 8 * lh]), qreg[s], S);
            dA = mfma16(*reinterpret_cast<const v8 *>(&sV[l31][16 * s + 8 * lh]), dreg[s], dA);
        }
        float ds[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + crow(r, lh);
            const float p = __expf(S[r] * g.scale - lse_n);
            const float c = kept(row_hash, (uint32_t)m, seed_hi, g.thr) ? g.inv_keep : 0.0f;
            const float v = p * (c * dA[r] - delta_n) * g.scale;
            ds[r] = (constant || m >= g.M) ? 0.0f : v;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const v8 db = round8<T>(ds + 8 * t);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) dQ[cb] = mfma16(read_cm<T>(sKt[cb * 32 + l31], t, lh), db, dQ[cb]);
        }
    }
    // (0 x a NaN key would be NaN: a constant row's zeros are written as such)
    if (live) store_row<T, DP>(g_q + (((size_t)b * g.N + n) * g.H + h) * g.d, dQ, constant, g, lh);
}

// ---- backward by key blocks: g_kv -------------------------------------------------------------------------------------------------------
template <typename T, int DP>
__global__ __launch_bounds__(THREADS) void k_half_bwd_kv(AttnGeom g, const void *__restrict__ q_, const void *__restrict__ kv_,
                                                         const uint8_t *__restrict__ row_keep, const int64_t *__restrict__ seed,
                                                         const float *__restrict__ lse, const float *__restrict__ delta,
                                                         const void *__restrict__ g_out_, void *__restrict__ g_kv_) {
    using v8 = typename Vec<T>::v8;
    const T *__restrict__ q = reinterpret_cast<const T *>(q_), *__restrict__ kv = reinterpret_cast<const T *>(kv_);
    const T *__restrict__ g_out = reinterpret_cast<const T *>(g_out_);
    T *__restrict__ g_kv = reinterpret_cast<T *>(g_kv_);
    __shared__ __attribute__((aligned(16))) T sQ[KT][DP + RP];
    __shared__ __attribute__((aligned(16))) T sD[KT][DP + RP];
    __shared__ __attribute__((aligned(16))) T sQt[DP][KT + CP];
    __shared__ __attribute__((aligned(16))) T sDt[DP][KT + CP];
    __shared__ float sLse[KT], sDelta[KT];
    __shared__ uint32_t sHash[KT];
    __shared__ int sFlag[KT];
    constexpr int CB = DP / 32, KS = DP / 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const uint32_t kblocks = ((uint32_t)g.M + KB - 1) / KB;
    const uint32_t bh = blockIdx.x / kblocks, kb = blockIdx.x - bh * kblocks;
    const int b = (int)(bh / (uint32_t)g.H), h = (int)(bh - (uint32_t)b * g.H);
    const int key = (int)(kb * KB) + wave * 32 + l31;
    const bool klive = key < g.M;
    uint32_t seed_lo, seed_hi;
    read_seed(g, seed, seed_lo, seed_hi);
    const size_t q_stride = (size_t)g.H * g.d;

    v8 kreg[KS], vreg[KS];
    {
        const size_t at = ((((size_t)b * g.M + (klive ? key : 0)) * 2) * g.H + h) * g.d, to_v = (size_t)g.H * g.d;
        load_row<T, DP>(kreg, kv + at, klive, g, lh);
        load_row<T, DP>(vreg, kv + at + to_v, klive, g, lh);
    }
    f32x16 dK[CB], dV[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dK[cb][r] = 0.0f; dV[cb][r] = 0.0f; }

    for (int n0 = 0; n0 < g.N; n0 += KT) {
        __syncthreads();  // the previous tile has been read
        if (tid < KT) {
            const int n = n0 + tid;
            int flag = ROW_NONE;
            float l = 0.0f, dl = 0.0f;
            if (n < g.N) {
                l = lse[(size_t)bh * g.N + n];
                dl = delta[(size_t)bh * g.N + n];
                flag = (row_keep != nullptr && row_keep[(size_t)b * g.N + n] == 0) ? ROW_MASKED : (l == INFINITY ? ROW_BAD : ROW_OPEN);
            }
            sFlag[tid] = flag; sLse[tid] = l; sDelta[tid] = dl;
            sHash[tid] = fmix32((bh * (uint32_t)g.N + (uint32_t)n) ^ seed_lo);
        }
        __syncthreads();
        // a masked or bad row sends nothing to the keys: its query row is staged as zeros (its own NaN must not reach dK as 0 x NaN)
        {
            const size_t at = (((size_t)b * g.N + n0) * g.H + h) * g.d;
            stage_tile<T, DP, true, true>(sQ, sQt, q + at, q_stride, g.N - n0, g, sFlag, true, tid);
            stage_tile<T, DP, true, true>(sD, sDt, g_out + at, q_stride, g.N - n0, g, sFlag, false, tid);
        }
        __syncthreads();
        f32x16 S, dA;
#pragma unroll
        for (int r = 0; r < 16; ++r) { S[r] = 0.0f; dA[r] = 0.0f; }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            S = mfma16(*reinterpret_cast<const v8 *>(&sQ[l31][16 * s + 8 * lh]), kreg[s], S);
            dA = mfma16(*reinterpret_cast<const v8 *>(&sD[l31][16 * s + 8 * lh]), vreg[s], dA);
        }
        float a[16], ds[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qi = crow(r, lh), flag = sFlag[qi];
            // a masked row's scores are all -1e4: exactly uniform (max + ln(sum) near -1e4 could not give 1 / M to better than 5e-4)
            const float p = flag == ROW_MASKED ? g.inv_m : __expf(S[r] * g.scale - sLse[qi]);
            const float c = kept(sHash[qi], (uint32_t)key, seed_hi, g.thr) ? g.inv_keep : 0.0f;
            const float av = c * p, dv = p * (c * dA[r] - sDelta[qi]) * g.scale;
            const bool none = flag == ROW_NONE || !klive;
            a[r] = none ? 0.0f : (flag == ROW_BAD ? g.inv_m : av);
            ds[r] = (none || flag != ROW_OPEN) ? 0.0f : dv;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const v8 ab = round8<T>(a + 8 * t), db = round8<T>(ds + 8 * t);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                dV[cb] = mfma16(read_cm<T>(sDt[cb * 32 + l31], t, lh), ab, dV[cb]);
                dK[cb] = mfma16(read_cm<T>(sQt[cb * 32 + l31], t, lh), db, dK[cb]);
            }
        }
    }
    if (klive) {
        T *gk = g_kv + ((((size_t)b * g.M + key) * 2) * g.H + h) * g.d;
        store_row<T, DP>(gk, dK, false, g, lh);
        store_row<T, DP>(gk + (size_t)g.H * g.d, dV, false, g, lh);
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
int geometry(int32_t batch, int32_t queries, int32_t keys, int32_t heads, int32_t head_dim, AttnGeom *g, const char *who) {
    if (batch < 1 || queries < 1 || keys < 1 || heads < 1 || head_dim < 1) {
        fgs_set_error("%s: invalid dims B=%d N=%d M=%d H=%d d=%d", who, batch, queries, keys, heads, head_dim);
        return FGS_EINVAL;
    }
    if (head_dim > FGS_ATTN_MAX_HEAD_DIM) {
        fgs_set_error("%s: head_dim = %d > %d is not supported", who, head_dim, FGS_ATTN_MAX_HEAD_DIM);
        return FGS_EUNSUPPORTED;
    }
    if ((uint64_t)batch * (uint64_t)heads * (uint64_t)queries >= (1ull << 31) ||
        (uint64_t)batch * (uint64_t)heads * (((uint64_t)keys + KB - 1) / KB) >= (1ull << 31)) {
        fgs_set_error("%s: B x H x N = %d x %d x %d (M = %d) is beyond the supported size", who, batch, heads, queries, keys);
        return FGS_EUNSUPPORTED;
    }
    g->B = batch; g->N = queries; g->M = keys; g->H = heads; g->d = head_dim;
    g->scale = 1.0f; g->inv_keep = 1.0f; g->inv_m = 1.0f / (float)keys; g->thr = 0u; g->vec = 0;
    return FGS_OK;
}

int set_call(AttnGeom *g, int32_t dtype, float scale, float dropout_p, const int64_t *seed, const char *who) {
    if (dtype != FGS_ATTN_F16 && dtype != FGS_ATTN_BF16) {
        fgs_set_error("%s: dtype = %d is neither FGS_ATTN_F16 nor FGS_ATTN_BF16", who, dtype);
        return FGS_EINVAL;
    }
    if (!(dropout_p >= 0.0f && dropout_p < 1.0f)) {
        fgs_set_error("%s: dropout_p = %g is not in [0, 1)", who, (double)dropout_p);
        return FGS_EINVAL;
    }
    g->scale = scale;
    g->thr = (uint32_t)lrintf(dropout_p * 16777216.0f);
    g->inv_keep = 1.0f / (1.0f - dropout_p);
    if (g->thr && !seed) { fgs_set_error("%s: dropout_p > 0 needs a seed", who); return FGS_EINVAL; }
    return FGS_OK;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

size_t rows_bytes(const AttnGeom &g) { return ((size_t)g.B * g.H * g.N * sizeof(float) + 255) & ~(size_t)255; }

#define HALF_WIDTHS(kernel, T, grid, ...)                                                                              \
    do {                                                                                                               \
        if (g.d <= 32) hipLaunchKernelGGL((kernel<T, 32>), dim3(grid), dim3(THREADS), 0, st, __VA_ARGS__);             \
        else if (g.d <= 64) hipLaunchKernelGGL((kernel<T, 64>), dim3(grid), dim3(THREADS), 0, st, __VA_ARGS__);        \
        else hipLaunchKernelGGL((kernel<T, 128>), dim3(grid), dim3(THREADS), 0, st, __VA_ARGS__);                      \
    } while (0)
#define HALF_DISPATCH(kernel, grid, ...)                                                \
    do {                                                                                \
        if (dtype == FGS_ATTN_F16) HALF_WIDTHS(kernel, _Float16, grid, __VA_ARGS__);    \
        else HALF_WIDTHS(kernel, __bf16, grid, __VA_ARGS__);                            \
    } while (0)

}  // namespace

extern "C" {

int fgs_attn_half_workspace_bytes(int32_t batch, int32_t queries, int32_t keys, int32_t heads, int32_t head_dim, size_t *saved_bytes,
                                  size_t *scratch_bytes) {
    AttnGeom g;
    int rc = geometry(batch, queries, keys, heads, head_dim, &g, "fgs_attn_half_workspace_bytes");
    if (rc) return rc;
    if (!saved_bytes || !scratch_bytes) { fgs_set_error("fgs_attn_half_workspace_bytes: null output pointer"); return FGS_EINVAL; }
    *saved_bytes = rows_bytes(g);    // max + ln(sum) per (b, h, n), fp32
    *scratch_bytes = rows_bytes(g);  // delta per (b, h, n), fp32
    return FGS_OK;
}

int fgs_attn_half_forward(int32_t dtype, int32_t batch, int32_t queries, int32_t keys, int32_t heads, int32_t head_dim, float scale,
                          float dropout_p, const void *q, const void *kv, const uint8_t *row_keep, const int64_t *seed, void *out,
                          void *saved, void *stream) {
    AttnGeom g;
    int rc = geometry(batch, queries, keys, heads, head_dim, &g, "fgs_attn_half_forward");
    if (rc) return rc;
    if ((rc = set_call(&g, dtype, scale, dropout_p, seed, "fgs_attn_half_forward"))) return rc;
    if (!q || !kv || !out || !saved) {
        fgs_set_error("fgs_attn_half_forward: null pointer argument (row_keep may be NULL, and seed when dropout_p is 0)");
        return FGS_EINVAL;
    }
    g.vec = head_dim % 8 == 0 && aligned16(q) && aligned16(kv) && aligned16(out);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint32_t grid = (uint32_t)batch * heads * (((uint32_t)queries + QB - 1) / QB);
    HALF_DISPATCH(k_half_fwd, grid, g, q, kv, row_keep, seed, out, reinterpret_cast<float *>(saved));
    FGS_LAUNCH_CHECK("k_half_fwd");
    return FGS_OK;
}

int fgs_attn_half_backward(int32_t dtype, int32_t batch, int32_t queries, int32_t keys, int32_t heads, int32_t head_dim, float scale,
                           float dropout_p, const void *q, const void *kv, const uint8_t *row_keep, const int64_t *seed,
                           const void *out, const void *saved, const void *g_out, void *g_q, void *g_kv, void *scratch, void *stream) {
    AttnGeom g;
    int rc = geometry(batch, queries, keys, heads, head_dim, &g, "fgs_attn_half_backward");
    if (rc) return rc;
    if ((rc = set_call(&g, dtype, scale, dropout_p, seed, "fgs_attn_half_backward"))) return rc;
    if (!q || !kv || !out || !saved || !g_out || !g_q || !g_kv || !scratch) {
        fgs_set_error("fgs_attn_half_backward: null pointer argument (row_keep may be NULL, and seed when dropout_p is 0)");
        return FGS_EINVAL;
    }
    g.vec = head_dim % 8 == 0 && aligned16(q) && aligned16(kv) && aligned16(out) && aligned16(g_out) && aligned16(g_q) && aligned16(g_kv);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const float *lse = reinterpret_cast<const float *>(saved);
    float *delta = reinterpret_cast<float *>(scratch);
    const uint32_t rows = (uint32_t)batch * heads * (uint32_t)queries;
    if (dtype == FGS_ATTN_F16) hipLaunchKernelGGL(k_half_delta<_Float16>, dim3((rows + THREADS - 1) / THREADS), dim3(THREADS), 0, st, g, out, g_out, delta);
    else hipLaunchKernelGGL(k_half_delta<__bf16>, dim3((rows + THREADS - 1) / THREADS), dim3(THREADS), 0, st, g, out, g_out, delta);
    FGS_LAUNCH_CHECK("k_half_delta");
    const uint32_t qgrid = (uint32_t)batch * heads * (((uint32_t)queries + QB - 1) / QB);
    HALF_DISPATCH(k_half_bwd_q, qgrid, g, q, kv, row_keep, seed, lse, (const float *)delta, g_out, g_q);
    FGS_LAUNCH_CHECK("k_half_bwd_q");
    const uint32_t kgrid = (uint32_t)batch * heads * (((uint32_t)keys + KB - 1) / KB);
    HALF_DISPATCH(k_half_bwd_kv, kgrid, g, q, kv, row_keep, seed, lse, (const float *)delta, g_out, g_kv);
    FGS_LAUNCH_CHECK("k_half_bwd_kv");
    return FGS_OK;
}

}  // extern "C"
