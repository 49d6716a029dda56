// Fused self-attention of the consistency view synthesizer's FresnelWaveAttention (scripts/models/consistency_view_synthesis.py,
// "CVS": 191-246): multi-head attention over the grid_h x grid_w tokens of a feature map with the interference term
// 0.1 cos(2 pi dist / (|wavelength| grid_h + 1e-6)) added to the logits, flash-style -- nothing of size N x N is stored.  Definition,
// bias chain and NaN behaviour: include/fgs.h.  The tiling, the lane maps and the online softmax are those of fgs_attn.hip (read its
// header comment first); what differs:
//
//  * packed input.  q, k and v of token n, head h are three rows of ONE tensor (B, N, 3, heads, d), read in place;
//  * the bias.  It depends on (|dy|, |dx|) only, so every workgroup builds the table T[|dy|][|dx|] = 0.1 cosf(phi) of grid_h grid_w
//    floats in LDS once (accurate cosf, IEEE divide and square root: the unit's flags, fresnel_amd/build.py) and adds T by lookup:
//    score = (S scale) + T, two roundings.  The tokens' grid coordinates come with the tile: one packed word per key (forward, g_q) or
//    per query (g_k, g_v) in LDS, the lane's own in registers -- no division per score;
//  * no mask, no dropout, no NaN cleaning: a row whose NaN-propagating maximum is not finite is written as NaN (torch's softmax), its
//    saved value is NaN, and the backward lets that propagate through its (b, h);
//  * dL/d wavelength.  k_wave_bwd_q holds a second table U = 0.1 sin(phi) phi and sums dS U (dS UNSCALED) per lane in double; a
//    fixed-shape tree gives one partial per workgroup, k_wave_fold adds the partials in a fixed order and applies
//    sign(lambda) grid_h / den.  No atomics: two calls agree to the bit.
//
// fgs_wave_attn_backward: k_wave_delta, k_wave_bwd_q (g_q + partials), k_wave_bwd_kv (g_k, g_v), k_wave_fold.
//
// Compiled with -ffp-contract=off: the backward recomputes p = exp(score - saved) and must round (S scale) + T as the forward did.
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

struct WaveGeom {
    int32_t B, GH, GW, N, H, d;
    float scale;
};

__device__ __forceinline__ int crow(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// a token's grid coordinates as one word: y << 16 | x
__device__ __forceinline__ int coords_of(int n, int gw) {
    const int y = n / gw;
    return (y << 16) | (n - y * gw);
}
// index of (|dy|, |dx|) in the tables
__device__ __forceinline__ int table_index(int a, int b, int gw) {
    return abs((a >> 16) - (b >> 16)) * gw + abs((a & 0xFFFF) - (b & 0xFFFF));
}

// include/fgs.h: the bias chain, every operation rounded on its own.  T[dy gw + dx] = 0.1 cosf(phi).  U = 0.1 sin(phi) phi is
// evaluated in DOUBLE from the same fp32 den and rounded once: the forward is defined with the fp32 phase, but the derivative is
// not -- at wavelength 1e-3 a phase of 7000 rad carries 2.4e-4 rad of fp32 rounding, which U's factor phi cos(phi) turns into a
// relative error of 2.4e-4 per term of a sum that cancels tenfold (g_wavelength 8.4e-4 from the fp64 value on a 16 x 8 grid with
// the fp32 U, 3.5e-5 with this one).  One double sine per table entry and workgroup, in the g_q launch only
template <bool WITH_U>
__device__ __forceinline__ void build_tables(float *__restrict__ sT, float *__restrict__ sU, const WaveGeom &g,
                                             const float *__restrict__ wavelength, int tid) {
    const float den = fabsf(wavelength[0]) * (float)g.GH + 1e-6f;
    for (int i = tid; i < g.N; i += THREADS) {
        const int dy = i / g.GW, dx = i - dy * g.GW;
        const float fy = (float)dy, fx = (float)dx;
        const float dist = sqrtf((fy * fy + fx * fx) + 1e-8f);
        const float phi = (6.2831855f * dist) / den;
        sT[i] = 0.1f * cosf(phi);
        if (WITH_U) {
            const double phid = (6.283185307179586 * sqrt((double)(fy * fy + fx * fx) + 1e-8)) / (double)den;
            sU[i] = (float)(0.1 * sin(phid) * phid);
        }
    }
}

// rows [t0, t0 + 32) of one of q, k, v (`base` points at token 0's row of it) -> dst[token][channel]; zeros beyond N and beyond d
template <int DP>
__device__ __forceinline__ void load_tile(float (*dst)[DP + 2], const float *__restrict__ base, size_t row_stride, const WaveGeom &g,
                                          int t0, int tid) {
    for (int i = tid; i < 32 * DP; i += THREADS) {
        const int row = i / DP, c = i - row * DP, t = t0 + row;
        float v = 0.0f;
        if (t < g.N && c < g.d) v = base[(size_t)t * row_stride + c];
        dst[row][c] = v;
    }
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(THREADS) void k_wave_fwd(WaveGeom g, const float *__restrict__ qkv, const float *__restrict__ wavelength,
                                                      float *__restrict__ out, float *__restrict__ lse) {
    __shared__ float sK[KT][DP + 2];
    __shared__ float sV[KT][DP + 2];
    __shared__ int sKc[KT];
    extern __shared__ __attribute__((aligned(16))) float sT[];  // g.N floats
    constexpr int CB = DP / 32, KS = DP / 2;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const uint32_t qblocks = ((uint32_t)g.N + QB - 1) / QB;
    const uint32_t bh = blockIdx.x / qblocks, qb = blockIdx.x - bh * qblocks;
    const int b = (int)(bh / (uint32_t)g.H), h = (int)(bh - (uint32_t)b * g.H);
    const int n = (int)(qb * QB) + wave * 32 + l31;
    const bool live = n < g.N;
    const int nc = coords_of(live ? n : 0, g.GW);
    const size_t hd = (size_t)g.H * g.d, rs = 3 * hd;
    const float *qkv_bh = qkv + (size_t)b * g.N * rs + (size_t)h * g.d;  // q of token 0; k at + hd, v at + 2 hd

    build_tables<false>(sT, nullptr, g, wavelength, tid);  // (the first tile's barrier publishes it)

    float qreg[KS];
    {
        const float *qrow = qkv_bh + (size_t)(live ? n : 0) * rs;
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

    for (int m0 = 0; m0 < g.N; m0 += KT) {
        __syncthreads();  // the previous tile has been read
        load_tile<DP>(sK, qkv_bh + hd, rs, g, m0, tid);
        load_tile<DP>(sV, qkv_bh + 2 * hd, rs, g, m0, tid);
        if (tid < KT) sKc[tid] = coords_of(m0 + tid < g.N ? m0 + tid : 0, g.GW);
        __syncthreads();
        f32x16 S;
#pragma unroll
        for (int r = 0; r < 16; ++r) S[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s) S = __builtin_amdgcn_mfma_f32_32x32x2f32(sK[l31][2 * s + lh], qreg[s], S, 0, 0, 0);
        float sv[16], tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = crow(r, lh);
            float x = S[r] * g.scale + sT[table_index(nc, sKc[key], g.GW)];
            if (m0 + key >= g.N) x = -INFINITY;  // not a key: no part in the maximum or the sum
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
            pk[r] = __expf(sv[r] - m_use);
            rowsum += pk[r];
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
    const bool bad = nan_seen || m_run == INFINITY || m_run == -INFINITY;  // torch's softmax of such a row: NaN
    const float inv = 1.0f / l_tot;
    if (live) {
        float *orow = out + (((size_t)b * g.N + n) * g.H + h) * g.d;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = cb * 32 + crow(r, lh);
                if (c < g.d) orow[c] = bad ? NAN : O[cb][r] * inv;  // (a column of O^T belongs to one query: the other rows are clean)
            }
        if (lh == 0) lse[(size_t)bh * g.N + n] = bad ? NAN : m_run + logf(l_tot);
    }
}

// ---- backward: delta ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_wave_delta(WaveGeom g, const float *__restrict__ out, const float *__restrict__ g_out,
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

// ---- backward by query blocks: g_q and this workgroup's part of sum dS U --------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(THREADS) void k_wave_bwd_q(WaveGeom g, const float *__restrict__ qkv, const float *__restrict__ wavelength,
                                                        const float *__restrict__ lse, const float *__restrict__ delta,
                                                        const float *__restrict__ g_out, float *__restrict__ g_qkv,
                                                        double *__restrict__ partial) {
    __shared__ float sK[KT][DP + 2];
    __shared__ float sV[KT][DP + 2];
    __shared__ int sKc[KT];
    __shared__ double sSum[THREADS];
    extern __shared__ __attribute__((aligned(16))) float sT[];  // T: g.N floats, then U: g.N floats
    float *sU = sT + g.N;
    constexpr int CB = DP / 32, KS = DP / 2;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const uint32_t qblocks = ((uint32_t)g.N + QB - 1) / QB;
    const uint32_t bh = blockIdx.x / qblocks, qb = blockIdx.x - bh * qblocks;
    const int b = (int)(bh / (uint32_t)g.H), h = (int)(bh - (uint32_t)b * g.H);
    const int n = (int)(qb * QB) + wave * 32 + l31;
    const bool live = n < g.N;
    const int nc = coords_of(live ? n : 0, g.GW);
    const size_t hd = (size_t)g.H * g.d, rs = 3 * hd;
    const float *qkv_bh = qkv + (size_t)b * g.N * rs + (size_t)h * g.d;
    const float lse_n = live ? lse[(size_t)bh * g.N + n] : 0.0f, delta_n = live ? delta[(size_t)bh * g.N + n] : 0.0f;

    build_tables<true>(sT, sU, g, wavelength, tid);

    float qreg[KS], dreg[KS];
    {
        const float *qrow = qkv_bh + (size_t)(live ? n : 0) * rs;
        const float *drow = g_out + (((size_t)b * g.N + (live ? n : 0)) * g.H + h) * g.d;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int c = 2 * s + lh;
            const bool in = live && c < g.d;
            qreg[s] = in ? qrow[c] : 0.0f;
            dreg[s] = in ? drow[c] : 0.0f;
        }
    }
    f32x16 dQ[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) dQ[cb][r] = 0.0f;
    double wsum = 0.0;  // this lane's sum of dS U: its query against 16 keys of every tile, in key order

    for (int m0 = 0; m0 < g.N; m0 += KT) {
        __syncthreads();
        load_tile<DP>(sK, qkv_bh + hd, rs, g, m0, tid);
        load_tile<DP>(sV, qkv_bh + 2 * hd, rs, g, m0, tid);
        if (tid < KT) sKc[tid] = coords_of(m0 + tid < g.N ? m0 + tid : 0, g.GW);
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
            const int key = crow(r, lh), at = table_index(nc, sKc[key], g.GW);
            const float p = __expf((S[r] * g.scale + sT[at]) - lse_n);
            const bool none = !live || m0 + key >= g.N;
            const float dsu = none ? 0.0f : p * (dA[r] - delta_n);
            wsum += (double)dsu * (double)sU[at];  // (exact product)
            ds[r] = dsu * g.scale;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = crow(r, lh);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) dQ[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(sK[key][cb * 32 + l31], ds[r], dQ[cb], 0, 0, 0);
        }
    }
    if (live) {
        float *grow = g_qkv + (size_t)b * g.N * rs + (size_t)n * rs + (size_t)h * g.d;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = cb * 32 + crow(r, lh);
                if (c < g.d) grow[c] = dQ[cb][r];
            }
    }
    sSum[tid] = wsum;
    __syncthreads();
    for (int w = THREADS / 2; w > 0; w >>= 1) {  // fixed shape: the same tree on every call
        if (tid < w) sSum[tid] += sSum[tid + w];
        __syncthreads();
    }
    if (tid == 0) partial[blockIdx.x] = sSum[0];
}

// ---- backward by key blocks: g_k, g_v -------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(THREADS) void k_wave_bwd_kv(WaveGeom g, const float *__restrict__ qkv, const float *__restrict__ wavelength,
                                                         const float *__restrict__ lse, const float *__restrict__ delta,
                                                         const float *__restrict__ g_out, float *__restrict__ g_qkv) {
    __shared__ float sQ[QT][DP + 2];
    __shared__ float sD[QT][DP + 2];
    __shared__ float sLse[QT], sDelta[QT];
    __shared__ int sQc[QT];
    extern __shared__ __attribute__((aligned(16))) float sT[];  // g.N floats
    constexpr int CB = DP / 32, KS = DP / 2;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const uint32_t kblocks = ((uint32_t)g.N + KB - 1) / KB;
    const uint32_t bh = blockIdx.x / kblocks, kb = blockIdx.x - bh * kblocks;
    const int b = (int)(bh / (uint32_t)g.H), h = (int)(bh - (uint32_t)b * g.H);
    const int key = (int)(kb * KB) + wave * 32 + l31;
    const bool klive = key < g.N;
    const int kc = coords_of(klive ? key : 0, g.GW);
    const size_t hd = (size_t)g.H * g.d, rs = 3 * hd;
    const float *qkv_bh = qkv + (size_t)b * g.N * rs + (size_t)h * g.d;
    const float *go_bh = g_out + (size_t)b * g.N * hd + (size_t)h * g.d;

    build_tables<false>(sT, nullptr, g, wavelength, tid);

    float kreg[KS], vreg[KS];
    {
        const float *krow = qkv_bh + (size_t)(klive ? key : 0) * rs + hd;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int c = 2 * s + lh;
            const bool in = klive && c < g.d;
            kreg[s] = in ? krow[c] : 0.0f;
            vreg[s] = in ? krow[hd + c] : 0.0f;
        }
    }
    f32x16 dK[CB], dV[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dK[cb][r] = 0.0f; dV[cb][r] = 0.0f; }

    for (int n0 = 0; n0 < g.N; n0 += QT) {
        __syncthreads();  // the previous tile has been read
        load_tile<DP>(sQ, qkv_bh, rs, g, n0, tid);
        load_tile<DP>(sD, go_bh, hd, g, n0, tid);
        if (tid < QT) {
            const int n = n0 + tid;
            const bool in = n < g.N;
            sLse[tid] = in ? lse[(size_t)bh * g.N + n] : 0.0f;
            sDelta[tid] = in ? delta[(size_t)bh * g.N + n] : 0.0f;
            sQc[tid] = coords_of(in ? n : 0, g.GW);
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
            const int qi = crow(r, lh);
            const float p = __expf((S[r] * g.scale + sT[table_index(sQc[qi], kc, g.GW)]) - sLse[qi]);
            const bool none = n0 + qi >= g.N || !klive;
            a[r] = none ? 0.0f : p;
            ds[r] = none ? 0.0f : (p * (dA[r] - sDelta[qi])) * g.scale;
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
        float *gk = g_qkv + (size_t)b * g.N * rs + (size_t)key * rs + hd + (size_t)h * g.d, *gv = gk + hd;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = cb * 32 + crow(r, lh);
                if (c < g.d) { gk[c] = dK[cb][r]; gv[c] = dV[cb][r]; }
            }
    }
}

// ---- backward: the partials in a fixed order, then dL/d wavelength ------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_wave_fold(int32_t parts, WaveGeom g, const double *__restrict__ partial,
                                                       const float *__restrict__ wavelength, float *__restrict__ g_wavelength) {
    __shared__ double sSum[THREADS];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < parts; i += THREADS) acc += partial[i];
    sSum[tid] = acc;
    __syncthreads();
    for (int w = THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) sSum[tid] += sSum[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        const float lam = wavelength[0];
        const float den = fabsf(lam) * (float)g.GH + 1e-6f;
        const double sign = lam > 0.0f ? 1.0 : (lam < 0.0f ? -1.0 : (lam == 0.0f ? 0.0 : (double)lam));  // |.| has gradient 0 at 0; NaN stays
        *g_wavelength = (float)(sign * ((double)g.GH / (double)den) * sSum[0]);
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
int geometry(int32_t batch, int32_t grid_h, int32_t grid_w, int32_t heads, int32_t head_dim, WaveGeom *g, const char *who) {
    if (batch < 1 || grid_h < 1 || grid_w < 1 || heads < 1 || head_dim < 1) {
        fgs_set_error("%s: invalid dims B=%d grid=%dx%d H=%d d=%d", who, batch, grid_h, grid_w, heads, head_dim);
        return FGS_EINVAL;
    }
    if (head_dim > FGS_ATTN_MAX_HEAD_DIM) {
        fgs_set_error("%s: head_dim = %d > %d is not supported", who, head_dim, FGS_ATTN_MAX_HEAD_DIM);
        return FGS_EUNSUPPORTED;
    }
    if ((uint64_t)grid_h * (uint64_t)grid_w > FGS_WAVE_ATTN_MAX_TOKENS) {
        fgs_set_error("%s: a grid of %d x %d tokens is beyond the supported %d (the bias tables live in LDS)", who, grid_h, grid_w,
                      FGS_WAVE_ATTN_MAX_TOKENS);
        return FGS_EUNSUPPORTED;
    }
    const int32_t tokens = grid_h * grid_w;
    if ((uint64_t)batch * (uint64_t)heads * (uint64_t)tokens >= (1ull << 31)) {
        fgs_set_error("%s: B x H x N = %d x %d x %d is beyond the supported size", who, batch, heads, tokens);
        return FGS_EUNSUPPORTED;
    }
    g->B = batch; g->GH = grid_h; g->GW = grid_w; g->N = tokens; g->H = heads; g->d = head_dim;
    g->scale = 1.0f;
    return FGS_OK;
}

int set_scale(WaveGeom *g, float scale, const char *who) {
    if (!isfinite(scale)) { fgs_set_error("%s: scale = %g is not finite", who, (double)scale); return FGS_EINVAL; }
    g->scale = scale;
    return FGS_OK;
}

size_t round256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
size_t rows_bytes(const WaveGeom &g) { return round256((size_t)g.B * g.H * g.N * sizeof(float)); }
uint32_t blocks_of(const WaveGeom &g, int per_block) { return (uint32_t)g.B * g.H * (((uint32_t)g.N + per_block - 1) / per_block); }

#define WAVE_DISPATCH(kernel, grid, lds, ...)                                                                   \
    do {                                                                                                        \
        if (g.d <= 32) hipLaunchKernelGGL(kernel<32>, dim3(grid), dim3(THREADS), lds, st, __VA_ARGS__);         \
        else if (g.d <= 64) hipLaunchKernelGGL(kernel<64>, dim3(grid), dim3(THREADS), lds, st, __VA_ARGS__);    \
        else hipLaunchKernelGGL(kernel<128>, dim3(grid), dim3(THREADS), lds, st, __VA_ARGS__);                  \
    } while (0)

}  // namespace

extern "C" {

int fgs_wave_attn_workspace_bytes(int32_t batch, int32_t grid_h, int32_t grid_w, int32_t heads, int32_t head_dim, size_t *saved_bytes,
                                  size_t *scratch_bytes) {
    WaveGeom g;
    int rc = geometry(batch, grid_h, grid_w, heads, head_dim, &g, "fgs_wave_attn_workspace_bytes");
    if (rc) return rc;
    if (!saved_bytes || !scratch_bytes) { fgs_set_error("fgs_wave_attn_workspace_bytes: null output pointer"); return FGS_EINVAL; }
    *saved_bytes = rows_bytes(g);                                                       // max + ln(sum) per (b, h, n)
    *scratch_bytes = rows_bytes(g) + round256((size_t)blocks_of(g, QB) * sizeof(double));  // delta per (b, h, n); one partial per query block
    return FGS_OK;
}

int fgs_wave_attn_forward(int32_t batch, int32_t grid_h, int32_t grid_w, int32_t heads, int32_t head_dim, float scale, const float *qkv,
                          const float *wavelength, float *out, void *saved, void *stream) {
    WaveGeom g;
    int rc = geometry(batch, grid_h, grid_w, heads, head_dim, &g, "fgs_wave_attn_forward");
    if (rc) return rc;
    if ((rc = set_scale(&g, scale, "fgs_wave_attn_forward"))) return rc;
    if (!qkv || !wavelength || !out || !saved) { fgs_set_error("fgs_wave_attn_forward: null pointer argument"); return FGS_EINVAL; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t table = (size_t)g.N * sizeof(float);
    WAVE_DISPATCH(k_wave_fwd, blocks_of(g, QB), table, g, qkv, wavelength, out, reinterpret_cast<float *>(saved));
    FGS_LAUNCH_CHECK("k_wave_fwd");
    return FGS_OK;
}

int fgs_wave_attn_backward(int32_t batch, int32_t grid_h, int32_t grid_w, int32_t heads, int32_t head_dim, float scale, const float *qkv,
                           const float *wavelength, const float *out, const void *saved, const float *g_out, float *g_qkv,
                           float *g_wavelength, void *scratch, void *stream) {
    WaveGeom g;
    int rc = geometry(batch, grid_h, grid_w, heads, head_dim, &g, "fgs_wave_attn_backward");
    if (rc) return rc;
    if ((rc = set_scale(&g, scale, "fgs_wave_attn_backward"))) return rc;
    if (!qkv || !wavelength || !out || !saved || !g_out || !g_qkv || !scratch) {
        fgs_set_error("fgs_wave_attn_backward: null pointer argument (only g_wavelength may be NULL)");
        return FGS_EINVAL;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const float *lse = reinterpret_cast<const float *>(saved);
    float *delta = reinterpret_cast<float *>(scratch);
    double *partial = reinterpret_cast<double *>(reinterpret_cast<char *>(scratch) + rows_bytes(g));
    const size_t table = (size_t)g.N * sizeof(float);
    const uint32_t rows = (uint32_t)batch * heads * (uint32_t)g.N, qgrid = blocks_of(g, QB);
    hipLaunchKernelGGL(k_wave_delta, dim3((rows + THREADS - 1) / THREADS), dim3(THREADS), 0, st, g, out, g_out, delta);
    FGS_LAUNCH_CHECK("k_wave_delta");
    WAVE_DISPATCH(k_wave_bwd_q, qgrid, 2 * table, g, qkv, wavelength, lse, (const float *)delta, g_out, g_qkv, partial);
    FGS_LAUNCH_CHECK("k_wave_bwd_q");
    WAVE_DISPATCH(k_wave_bwd_kv, blocks_of(g, KB), table, g, qkv, wavelength, lse, (const float *)delta, g_out, g_qkv);
    FGS_LAUNCH_CHECK("k_wave_bwd_kv");
    if (g_wavelength) {
        hipLaunchKernelGGL(k_wave_fold, dim3(1), dim3(THREADS), 0, st, (int32_t)qgrid, g, (const double *)partial, wavelength,
                           g_wavelength);
        FGS_LAUNCH_CHECK("k_wave_fold");
    }
    return FGS_OK;
}

}  // extern "C"
