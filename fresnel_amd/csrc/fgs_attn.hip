// Fused cross-attention of the distillation decoder (scripts/models/direct_slat_decoder.py, "DSD": CrossAttention, 63-182): the
// voxels' queries against the image patches' keys and values, flash-style -- the (B, H, N, M) score tensor is never stored.
// Definition, NaN rule and dropout's keep function: include/fgs.h.  fp32 end to end on the fp32-input matrix cores
// (v_mfma_f32_32x32x2_f32: exact fp32 FMA chains), no float atomics, every sum in a fixed order: two calls agree to the bit, and
// an image's result does not depend on the batch it sits in.
//
// Lane maps of the 32x32x2 form (lane l, l31 = l & 31, lh = l >> 5): A[i = l31][k = lh], B[k = lh][j = l31]; result register r of
// lane l is C[row = crow(r, lh)][column = l31], crow(r, lh) = (r & 3) + 8 (r >> 2) + 4 lh.
//
// k_attn_fwd.  A workgroup = 4 waves = FGS_ATTN_QUERY_BLOCK = 128 queries of one (b, h); a wave owns 32 of them, its query rows in
// registers.  The keys and values come through LDS in tiles of FGS_ATTN_KEY_TILE = 32, head dimension zero-padded to DP = 32 | 64 |
// 128, keys beyond M written as zeros.  Per tile S^T = K Q^T puts the query on the lane and 16 of the tile's keys in its registers
// (the lane pair l, l ^ 32 shares a query): maximum and sum are in-lane reductions plus one exchange, and P^T is already the B
// operand of O^T += V^T P^T when the V fragment is read in the key order crow(r, lh).  Online softmax; a row whose
// NaN-propagating maximum is not finite is found at the end of the sweep, and only a workgroup that holds such a row sweeps the
// values a second time, with 1 / M on that row's lanes and 0 on the others (a column of O^T belongs to one query).
//
// fgs_attn_backward.  k_attn_delta: delta = rowsum(g_out o out), one thread per (b, n, h).  k_attn_bwd_q: the forward's tiling;
// recomputes S^T, dA^T = V dO^T, forms dS^T = P^T o (c dA^T - delta) scale (c = keep / (1 - p)) and dQ^T += K^T dS^T.
// k_attn_bwd_kv: a workgroup = FGS_ATTN_KEY_BLOCK = 128 keys of one (b, h), a wave's 32 keys and values in registers with the KEY on the lane; it sweeps
// all queries in tiles of 32 through LDS: S = Q K^T, dA = dO V^T, then dV^T += dO^T A and dK^T += Q^T dS in accumulators.  Seven
// products where a form with atomics has five; in exchange nothing is summed across workgroups.
//
// Compiled with -ffp-contract=off (fresnel_amd/build.py): the backward's score S scale must be the forward's rounded product, not the
// inside of an FMA with the subtraction of `saved` -- a per-score mismatch of 2^-24 |score| does not cancel in sum_m dS_m.
#include "fgs_internal.h"

#include <math.h>

namespace {

constexpr int QB = FGS_ATTN_QUERY_BLOCK;  // queries per workgroup (forward, query-block backward)
constexpr int KT = FGS_ATTN_KEY_TILE;     // keys per LDS tile
constexpr int KB = FGS_ATTN_KEY_BLOCK;    // keys per workgroup of the key-block backward
constexpr int QT = 32;                    // queries per LDS tile of the key-block backward
constexpr int THREADS = 256;
static_assert(QB == (THREADS / 64) * 32 && KB == (THREADS / 64) * 32 && KT == 32 && QT == 32, "a wave owns one 32-wide MFMA tile");

using f32x16 = __attribute__((ext_vector_type(16))) float;

struct AttnGeom {
    int32_t B, N, M, H, d;
    float scale, inv_keep /* 1 / (1 - p) */, inv_m /* 1 / M */;
    uint32_t thr;  // round(p 2^24); 0 = no dropout
};

__device__ __forceinline__ int crow(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// murmur3's 32-bit finaliser
__device__ __forceinline__ uint32_t fmix32(uint32_t x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}
// include/fgs.h: the keep rule.  row_hash = fmix32(row ^ seed_lo)
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

// keys or values [m0, m0 + KT) of (b, h) -> dst[key][channel]; zeros beyond M and beyond d
template <int DP>
__device__ __forceinline__ void load_kv_tile(float (*dst)[DP + 2], const float *__restrict__ kv, const AttnGeom &g, int b, int h,
                                             int which, int m0, int tid) {
    for (int i = tid; i < KT * DP; i += THREADS) {
        const int key = i / DP, c = i - key * DP, m = m0 + key;
        float v = 0.0f;
        if (m < g.M && c < g.d) v = kv[((((size_t)b * g.M + m) * 2 + which) * g.H + h) * g.d + c];
        dst[key][c] = v;
    }
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(THREADS) void k_attn_fwd(AttnGeom g, const float *__restrict__ q, const float *__restrict__ kv,
                                                      const uint8_t *__restrict__ row_keep, const int64_t *__restrict__ seed,
                                                      float *__restrict__ out, float *__restrict__ lse) {
    __shared__ float sK[KT][DP + 2];
    __shared__ float sV[KT][DP + 2];
    constexpr int CB = DP / 32, KS = DP / 2;
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

    float qreg[KS];
    {
        const float *qrow = q + (((size_t)b * g.N + (live ? n : 0)) * g.H + h) * g.d;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int c = 2 * s + lh;
            qreg[s] = (live && c < g.d) ? qrow[c] : 0.0f;
        }
    }
    f32x16 O[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[cb][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;
    bool nan_seen = false;

    for (int m0 = 0; m0 < g.M; m0 += KT) {
        __syncthreads();  // the previous tile has been read
        load_kv_tile<DP>(sK, kv, g, b, h, 0, m0, tid);
        load_kv_tile<DP>(sV, kv, g, b, h, 1, m0, tid);
        __syncthreads();
        f32x16 S;
#pragma unroll
        for (int r = 0; r < 16; ++r) S[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s) S = __builtin_amdgcn_mfma_f32_32x32x2f32(sK[l31][2 * s + lh], qreg[s], S, 0, 0, 0);
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
        for (int r = 0; r < 16; ++r) {
            const int key = crow(r, lh);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) O[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(sV[key][cb * 32 + l31], pk[r], O[cb], 0, 0, 0);
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
        // a bad row's probabilities are 1 / M each, without dropout: the mean of v, on its own lanes only
        for (int m0 = 0; m0 < g.M; m0 += KT) {
            __syncthreads();
            load_kv_tile<DP>(sV, kv, g, b, h, 1, m0, tid);
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = crow(r, lh);
                const float p = (bad && m0 + key < g.M) ? g.inv_m : 0.0f;
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) O[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(sV[key][cb * 32 + l31], p, O[cb], 0, 0, 0);
            }
        }
    }
    if (live) {
        float *orow = out + (((size_t)b * g.N + n) * g.H + h) * g.d;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = cb * 32 + crow(r, lh);
                if (c < g.d) orow[c] = O[cb][r];
            }
        if (lh == 0) lse[(size_t)bh * g.N + n] = bad ? INFINITY : m_run + logf(l_tot);
    }
}

// ---- backward: delta ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_attn_delta(AttnGeom g, const float *__restrict__ out, const float *__restrict__ g_out,
                                                        float *__restrict__ delta) {
    const uint32_t t = blockIdx.x * (uint32_t)THREADS + threadIdx.x;  // (b N + n) H + h
    const uint32_t total = (uint32_t)g.B * (uint32_t)g.N * (uint32_t)g.H;
    if (t >= total) return;
    const uint32_t h = t % (uint32_t)g.H, bn = t / (uint32_t)g.H, b = bn / (uint32_t)g.N, n = bn - b * (uint32_t)g.N;
    const float *o = out + (size_t)t * g.d, *go = g_out + (size_t)t * g.d;
    float acc = 0.0f;
    for (int c = 0; c < g.d; ++c) acc = fmaf(o[c], go[c], acc);
    delta[((size_t)b * g.H + h) * g.N + n] = acc;
}

// ---- backward by query blocks: g_q ----------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(THREADS) void k_attn_bwd_q(AttnGeom g, const float *__restrict__ q, const float *__restrict__ kv,
                                                        const uint8_t *__restrict__ row_keep, const int64_t *__restrict__ seed,
                                                        const float *__restrict__ lse, const float *__restrict__ delta,
                                                        const float *__restrict__ g_out, float *__restrict__ g_q) {
    __shared__ float sK[KT][DP + 2];
    __shared__ float sV[KT][DP + 2];
    constexpr int CB = DP / 32, KS = DP / 2;
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

    float qreg[KS], dreg[KS];
    {
        const size_t at = (((size_t)b * g.N + (live ? n : 0)) * g.H + h) * g.d;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int c = 2 * s + lh;
            const bool in = live && c < g.d;
            qreg[s] = in ? q[at + c] : 0.0f;
            dreg[s] = in ? g_out[at + c] : 0.0f;
        }
    }
    f32x16 dQ[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) dQ[cb][r] = 0.0f;

    for (int m0 = 0; m0 < g.M; m0 += KT) {
        __syncthreads();
        load_kv_tile<DP>(sK, kv, g, b, h, 0, m0, tid);
        load_kv_tile<DP>(sV, kv, g, b, h, 1, m0, tid);
        __syncthreads();
        f32x16 S, dA;
#pragma unroll
        for (int r = 0; r < 16; ++r) { S[r] = 0.0f; dA[r] = 0.0f; }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            S = __builtin_amdgcn_mfma_f32_32x32x2f32(sK[l31][2 * s + lh], qreg[s], S, 0, 0, 0);
            dA = __builtin_amdgcn_mfma_f32_32x32x2f32(sV[l31][2 * s + lh], dreg[s], dA, 0, 0, 0);
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
        for (int r = 0; r < 16; ++r) {
            const int key = crow(r, lh);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) dQ[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(sK[key][cb * 32 + l31], ds[r], dQ[cb], 0, 0, 0);
        }
    }
    if (live) {
        float *grow = g_q + (((size_t)b * g.N + n) * g.H + h) * g.d;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = cb * 32 + crow(r, lh);
                if (c < g.d) grow[c] = constant ? 0.0f : dQ[cb][r];  // (0 x a NaN key would be NaN: the zero row is written as such)
            }
    }
}

// ---- backward by key blocks: g_kv -------------------------------------------------------------------------------------------------------
enum { ROW_OPEN = 0, ROW_MASKED = 1, ROW_BAD = 2, ROW_NONE = 3 };

template <int DP>
__global__ __launch_bounds__(THREADS) void k_attn_bwd_kv(AttnGeom g, const float *__restrict__ q, const float *__restrict__ kv,
                                                         const uint8_t *__restrict__ row_keep, const int64_t *__restrict__ seed,
                                                         const float *__restrict__ lse, const float *__restrict__ delta,
                                                         const float *__restrict__ g_out, float *__restrict__ g_kv) {
    __shared__ float sQ[QT][DP + 2];
    __shared__ float sD[QT][DP + 2];
    __shared__ float sLse[QT], sDelta[QT];
    __shared__ uint32_t sHash[QT];
    __shared__ int sFlag[QT];
    constexpr int CB = DP / 32, KS = DP / 2;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const uint32_t kblocks = ((uint32_t)g.M + KB - 1) / KB;
    const uint32_t bh = blockIdx.x / kblocks, kb = blockIdx.x - bh * kblocks;
    const int b = (int)(bh / (uint32_t)g.H), h = (int)(bh - (uint32_t)b * g.H);
    const int key = (int)(kb * KB) + wave * 32 + l31;
    const bool klive = key < g.M;
    uint32_t seed_lo, seed_hi;
    read_seed(g, seed, seed_lo, seed_hi);

    float kreg[KS], vreg[KS];
    {
        const size_t at = ((((size_t)b * g.M + (klive ? key : 0)) * 2) * g.H + h) * g.d, to_v = (size_t)g.H * g.d;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int c = 2 * s + lh;
            const bool in = klive && c < g.d;
            kreg[s] = in ? kv[at + c] : 0.0f;
            vreg[s] = in ? kv[at + to_v + c] : 0.0f;
        }
    }
    f32x16 dK[CB], dV[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dK[cb][r] = 0.0f; dV[cb][r] = 0.0f; }

    for (int n0 = 0; n0 < g.N; n0 += QT) {
        __syncthreads();  // the previous tile has been read
        if (tid < QT) {
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
        for (int i = tid; i < QT * DP; i += THREADS) {
            const int row = i / DP, c = i - row * DP, flag = sFlag[row];
            float qv = 0.0f, dv = 0.0f;
            if (flag != ROW_NONE && c < g.d) {
                const size_t at = (((size_t)b * g.N + (n0 + row)) * g.H + h) * g.d + c;
                dv = g_out[at];
                if (flag == ROW_OPEN) qv = q[at];
            }
            sQ[row][c] = qv;
            sD[row][c] = dv;
        }
        __syncthreads();
        f32x16 S, dA;
#pragma unroll
        for (int r = 0; r < 16; ++r) { S[r] = 0.0f; dA[r] = 0.0f; }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            S = __builtin_amdgcn_mfma_f32_32x32x2f32(sQ[l31][2 * s + lh], kreg[s], S, 0, 0, 0);
            dA = __builtin_amdgcn_mfma_f32_32x32x2f32(sD[l31][2 * s + lh], vreg[s], dA, 0, 0, 0);
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
        for (int r = 0; r < 16; ++r) {
            const int qi = crow(r, lh);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                dV[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(sD[qi][cb * 32 + l31], a[r], dV[cb], 0, 0, 0);
                dK[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(sQ[qi][cb * 32 + l31], ds[r], dK[cb], 0, 0, 0);
            }
        }
    }
    if (klive) {
        float *gk = g_kv + ((((size_t)b * g.M + key) * 2) * g.H + h) * g.d, *gv = gk + (size_t)g.H * g.d;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = cb * 32 + crow(r, lh);
                if (c < g.d) { gk[c] = dK[cb][r]; gv[c] = dV[cb][r]; }
            }
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
    g->scale = 1.0f; g->inv_keep = 1.0f; g->inv_m = 1.0f / (float)keys; g->thr = 0u;
    return FGS_OK;
}

int set_dropout(AttnGeom *g, float scale, float dropout_p, const int64_t *seed, const char *who) {
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

size_t rows_bytes(const AttnGeom &g) { return ((size_t)g.B * g.H * g.N * sizeof(float) + 255) & ~(size_t)255; }

#define ATTN_DISPATCH(kernel, grid, ...)                                                                        \
    do {                                                                                                        \
        if (g.d <= 32) hipLaunchKernelGGL(kernel<32>, dim3(grid), dim3(THREADS), 0, st, __VA_ARGS__);           \
        else if (g.d <= 64) hipLaunchKernelGGL(kernel<64>, dim3(grid), dim3(THREADS), 0, st, __VA_ARGS__);      \
        else hipLaunchKernelGGL(kernel<128>, dim3(grid), dim3(THREADS), 0, st, __VA_ARGS__);                    \
    } while (0)

}  // namespace

extern "C" {

int fgs_attn_workspace_bytes(int32_t batch, int32_t queries, int32_t keys, int32_t heads, int32_t head_dim, size_t *saved_bytes,
                             size_t *scratch_bytes) {
    AttnGeom g;
    int rc = geometry(batch, queries, keys, heads, head_dim, &g, "fgs_attn_workspace_bytes");
    if (rc) return rc;
    if (!saved_bytes || !scratch_bytes) { fgs_set_error("fgs_attn_workspace_bytes: null output pointer"); return FGS_EINVAL; }
    *saved_bytes = rows_bytes(g);    // max + ln(sum) per (b, h, n)
    *scratch_bytes = rows_bytes(g);  // delta per (b, h, n)
    return FGS_OK;
}

int fgs_attn_forward(int32_t batch, int32_t queries, int32_t keys, int32_t heads, int32_t head_dim, float scale, float dropout_p,
                     const float *q, const float *kv, const uint8_t *row_keep, const int64_t *seed, float *out, void *saved,
                     void *stream) {
    AttnGeom g;
    int rc = geometry(batch, queries, keys, heads, head_dim, &g, "fgs_attn_forward");
    if (rc) return rc;
    if ((rc = set_dropout(&g, scale, dropout_p, seed, "fgs_attn_forward"))) return rc;
    if (!q || !kv || !out || !saved) {
        fgs_set_error("fgs_attn_forward: null pointer argument (row_keep may be NULL, and seed when dropout_p is 0)");
        return FGS_EINVAL;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint32_t grid = (uint32_t)batch * heads * (((uint32_t)queries + QB - 1) / QB);
    ATTN_DISPATCH(k_attn_fwd, grid, g, q, kv, row_keep, seed, out, reinterpret_cast<float *>(saved));
    FGS_LAUNCH_CHECK("k_attn_fwd");
    return FGS_OK;
}

int fgs_attn_backward(int32_t batch, int32_t queries, int32_t keys, int32_t heads, int32_t head_dim, float scale, float dropout_p,
                      const float *q, const float *kv, const uint8_t *row_keep, const int64_t *seed, const float *out,
                      const void *saved, const float *g_out, float *g_q, float *g_kv, void *scratch, void *stream) {
    AttnGeom g;
    int rc = geometry(batch, queries, keys, heads, head_dim, &g, "fgs_attn_backward");
    if (rc) return rc;
    if ((rc = set_dropout(&g, scale, dropout_p, seed, "fgs_attn_backward"))) return rc;
    if (!q || !kv || !out || !saved || !g_out || !g_q || !g_kv || !scratch) {
        fgs_set_error("fgs_attn_backward: null pointer argument (row_keep may be NULL, and seed when dropout_p is 0)");
        return FGS_EINVAL;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const float *lse = reinterpret_cast<const float *>(saved);
    float *delta = reinterpret_cast<float *>(scratch);
    const uint32_t rows = (uint32_t)batch * heads * (uint32_t)queries;
    hipLaunchKernelGGL(k_attn_delta, dim3((rows + THREADS - 1) / THREADS), dim3(THREADS), 0, st, g, out, g_out, delta);
    FGS_LAUNCH_CHECK("k_attn_delta");
    const uint32_t qgrid = (uint32_t)batch * heads * (((uint32_t)queries + QB - 1) / QB);
    ATTN_DISPATCH(k_attn_bwd_q, qgrid, g, q, kv, row_keep, seed, lse, (const float *)delta, g_out, g_q);
    FGS_LAUNCH_CHECK("k_attn_bwd_q");
    const uint32_t kgrid = (uint32_t)batch * heads * (((uint32_t)keys + KB - 1) / KB);
    ATTN_DISPATCH(k_attn_bwd_kv, kgrid, g, q, kv, row_keep, seed, lse, (const float *)delta, g_out, g_kv);
    FGS_LAUNCH_CHECK("k_attn_bwd_kv");
    return FGS_OK;
}

}  // extern "C"
