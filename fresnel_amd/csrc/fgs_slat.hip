// Gaussian-parameter head of the reference's distillation decoders (scripts/models/direct_slat_decoder.py, "DSD": GaussianHead,
// 255-358, behind DirectSLatDecoder and MLPSLatDecoder): the map from the head MLP's raw (B, N, G, 14) output and the voxel
// coordinates to the (B, N G, 14) cloud that GaussianMatchingLoss scores, and its exact derivative.  In torch it is about twenty
// small launches with slice assignments into a zeros_like buffer and an isnan(...).any() that stops the host; at inference the
// reference runs it once per image on boolean-indexed rows.
//
// Definition: include/fgs.h.  A row is position 0..2, scale 3..5, quaternion 6..9, colour 10..12, opacity 13, in and out.  This unit
// is compiled without FMA contraction (fresnel_amd/build.py): the backward recomputes the forward from `raw`, and its clamp gates
// must be the forward's.
//
// k_slat_fwd.  The B N G rows are one flat list; a block takes HB = 256 consecutive rows, thread = one row.  A tile of 256 rows is
// 14 336 bytes, so tiles of a 16-byte aligned tensor stay 16-byte aligned although a row (56 bytes) is not: the tile goes through
// LDS at the odd row stride 15 with 16-byte global accesses (fgs_gaussrow.h) and comes back the same way.  The gains are read on
// the device.  One launch.
//
// Gated forward (inference).  k_slat_scan, one block per image: count -> scan over the image's keep bytes in chunks of 256 voxels
// (fgs_scan.h), as k_match_compact; it writes the image's count and, per voxel, where it goes: its rank among the kept voxels,
// or -(kept before it) - 1 for a dropped one.  k_slat_fwd<GATED> is the head itself, writing a kept voxel's G rows to its
// compacted place; a DROPPED voxel's threads write zero rows into the tail instead -- the image has as many dropped voxels as tail
// slots, dropped voxel number d goes to slot count + d -- so every row of `gaussians` is written exactly once, by one thread,
// without atomics and without a launch of its own for the zero-fill.  Compacted rows are not tile-aligned: each thread stores its
// row as seven 8-byte words.
//
// k_slat_bwd.  The forward's tiling; raw and upstream tiles through LDS, g_raw back through the raw tile: every element written.
// The two gain gradients are sums over all rows of products of two floats (exact in double): a fixed-shape block tree, one
// partial pair per block into `scratch`, and k_slat_fold (one block: thread t adds partials t, t + 256, ... , then a fixed tree)
// rounds each to fp32 once.  No atomics: two calls agree to the bit.
#include "fgs_gaussrow.h"  // tile copies (HB threads), normalize_bwd
#include "fgs_scan.h"

#include <math.h>

namespace {

constexpr int ROW = 14;             // floats per Gaussian, in and out
constexpr int RP = 15;              // its odd row stride in LDS
constexpr int FOLD_THREADS = 256;   // threads of k_slat_fold: thread t adds partials t, t + 256, ...
constexpr int MAX_G = 64;

struct SlatGeom {
    int32_t N, G;
    uint32_t rows;  // B N G
};

// clamp that keeps a NaN (fminf / fmaxf alone would drop it), as torch.clamp
__device__ __forceinline__ float clamp_(float x, float lo, float hi) { return x != x ? x : fminf(fmaxf(x, lo), hi); }

// What the backward needs of one row beside the outputs.  A `live` flag is false where the output element was written as 0 in
// place of a NaN (the whole quaternion at once): that output is a constant, nothing flows through it.
struct RowAux {
    float t[3];        // tanh of the clamped position channels
    bool pos_open[3];  // live and the position clamp passes the gradient (closed interval)
    float sp[3], dsp[3];  // softplus of the clamped scale channels and its derivative
    bool scale_open[3];
    float q[4], qn;    // clamped quaternion channels and their norm
    bool quat_live;
    float sg[4];       // the four sigmoids
    bool sg_live[4];
};

// one row of the head: x = 14 raw floats, ctr = the voxel's centre, pg = position_offset_scale, asf = |scale_factor|
__device__ __forceinline__ void row_fwd(const float *x, const float *ctr, float pg, float asf, float *o, RowAux &a) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float r = clamp_(x[c], -10.0f, 10.0f);
        a.t[c] = tanhf(r);
        const float u = ctr[c] + a.t[c] * pg;
        const float p = clamp_(u, -1.0f, 1.0f);
        a.pos_open[c] = u >= -1.0f && u <= 1.0f;  // (false for a NaN)
        o[c] = p != p ? 0.0f : p;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float r = clamp_(x[3 + c], -10.0f, 10.0f);
        const float z = expf(r);                  // r <= 10: below torch's softplus threshold of 20, never its linear branch
        a.sp[c] = log1pf(z);
        a.dsp[c] = z / (z + 1.0f);
        const float v = a.sp[c] * asf;
        const float s = clamp_(v, 1e-4f, 1.0f);
        a.scale_open[c] = v >= 1e-4f && v <= 1.0f;
        o[3 + c] = s != s ? 0.0f : s;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) a.q[c] = clamp_(x[6 + c], -10.0f, 10.0f);
    a.qn = sqrtf(((a.q[0] * a.q[0] + a.q[1] * a.q[1]) + a.q[2] * a.q[2]) + a.q[3] * a.q[3]);
    a.quat_live = a.qn == a.qn;  // a NaN component makes the norm NaN
    const float den = fmaxf(a.qn, EPS);
#pragma unroll
    for (int c = 0; c < 4; ++c) o[6 + c] = a.quat_live ? a.q[c] / den : 0.0f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float r = clamp_(x[10 + c], -10.0f, 10.0f);
        const float s = 1.0f / (1.0f + expf(-r));
        a.sg_live[c] = s == s;
        a.sg[c] = s;
        o[10 + c] = a.sg_live[c] ? s : 0.0f;
    }
}

// centre of a row's voxel: clamp(coordinate, 0, 63) / 64 * 2 - 1 (exact in fp32), whatever the decoder's max_resolution (DSD:327-328)
__device__ __forceinline__ void centre_of(const int32_t *__restrict__ coords, uint32_t voxel, float *ctr) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int32_t v = coords[(size_t)voxel * 4 + 1 + c];
        ctr[c] = (float)min(max(v, 0), 63) / 64.0f * 2.0f - 1.0f;
    }
}

// ---- gated forward: where every voxel goes ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HB) void k_slat_scan(int32_t N, const uint8_t *__restrict__ keep, int32_t *__restrict__ dest,
                                                  int32_t *__restrict__ counts) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint8_t *kb = keep + (size_t)b * N;
    int32_t *db = dest + (size_t)b * N;
    uint32_t base = 0;
    for (int i0 = 0; i0 < N; i0 += HB) {
        const int i = i0 + tid;
        const bool kept = i < N && kb[i] != 0;
        uint32_t tot;
        const uint32_t at = base + block_exclusive_scan_256(kept ? 1u : 0u, &tot);  // = the kept voxels before i
        if (i < N) db[i] = kept ? (int32_t)at : -(int32_t)at - 1;
        base += tot;
        __syncthreads();  // the scan's wave sums are reused by the next chunk
    }
    if (tid == 0) counts[b] = (int32_t)base;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------
template <bool GATED>
__global__ __launch_bounds__(HB) void k_slat_fwd(SlatGeom g, const float *__restrict__ raw, const int32_t *__restrict__ coords,
                                                 const float *__restrict__ gains, const int32_t *__restrict__ dest,
                                                 const int32_t *__restrict__ counts, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float lds[HB * RP];
    const int tid = threadIdx.x;
    const uint32_t r0 = blockIdx.x * (uint32_t)HB;
    const int nrows = (int)min((uint32_t)HB, g.rows - r0);
    rows_load<ROW, RP>(lds, raw + (size_t)r0 * ROW, nrows, tid);
    __syncthreads();
    const bool active = tid < nrows;
    const uint32_t row = r0 + tid;
    const uint32_t voxel = active ? row / (uint32_t)g.G : 0u;
    float o[ROW];
    bool zero_row = false;
    size_t out_row = row;
    if (GATED && active) {
        const uint32_t b = voxel / (uint32_t)g.N, i = voxel - b * (uint32_t)g.N, k = row - voxel * (uint32_t)g.G;
        const int32_t d = dest[voxel];
        zero_row = d < 0;
        // a kept voxel goes to its rank; dropped voxel number (i - kept before it) to the slot of that number behind the kept ones
        const uint32_t slot = zero_row ? (uint32_t)counts[b] + (i - (uint32_t)(-d - 1)) : (uint32_t)d;
        out_row = ((size_t)b * g.N + slot) * g.G + k;
    }
    if (active) {
        if (zero_row) {
#pragma unroll
            for (int c = 0; c < ROW; ++c) o[c] = 0.0f;
        } else {
            float x[ROW], ctr[3];
#pragma unroll
            for (int c = 0; c < ROW; ++c) x[c] = lds[tid * RP + c];
            centre_of(coords, voxel, ctr);
            RowAux a;
            row_fwd(x, ctr, gains[0], fabsf(gains[1]), o, a);
        }
    }
    if (GATED) {
        if (!active) return;
        float *dst = out + out_row * ROW;  // 56-byte rows: 8-byte aligned when the tensor is
        if ((reinterpret_cast<uintptr_t>(out) & 7u) == 0) {
#pragma unroll
            for (int c = 0; c < ROW; c += 2) *reinterpret_cast<float2 *>(dst + c) = make_float2(o[c], o[c + 1]);
        } else {
#pragma unroll
            for (int c = 0; c < ROW; ++c) dst[c] = o[c];
        }
    } else {
        if (active) {
#pragma unroll
            for (int c = 0; c < ROW; ++c) lds[tid * RP + c] = o[c];  // a thread's own row: nobody else reads it before the barrier
        }
        __syncthreads();
        rows_store<ROW, RP>(out + (size_t)r0 * ROW, lds, nrows, tid);
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HB) void k_slat_bwd(SlatGeom g, const float *__restrict__ raw, const int32_t *__restrict__ coords,
                                                 const float *__restrict__ gains, const float *__restrict__ up,
                                                 float *__restrict__ g_raw, double *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float l_raw[HB * RP];
    __shared__ __attribute__((aligned(16))) float l_up[HB * RP];
    const int tid = threadIdx.x;
    const uint32_t r0 = blockIdx.x * (uint32_t)HB;
    const int nrows = (int)min((uint32_t)HB, g.rows - r0);
    rows_load<ROW, RP>(l_raw, raw + (size_t)r0 * ROW, nrows, tid);
    rows_load<ROW, RP>(l_up, up + (size_t)r0 * ROW, nrows, tid);
    __syncthreads();
    double acc[2] = {0.0, 0.0};  // this row's share of dL/d position_offset_scale and of dL/d |scale_factor|
    if (tid < nrows) {
        float x[ROW], gu[ROW], gr[ROW], o[ROW], ctr[3];
#pragma unroll
        for (int c = 0; c < ROW; ++c) { x[c] = l_raw[tid * RP + c]; gu[c] = l_up[tid * RP + c]; }
        centre_of(coords, (r0 + tid) / (uint32_t)g.G, ctr);
        const float pg = gains[0], asf = fabsf(gains[1]);
        RowAux a;
        row_fwd(x, ctr, pg, asf, o, a);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            gr[c] = a.pos_open[c] ? gu[c] * ((1.0f - a.t[c] * a.t[c]) * pg) : 0.0f;
            if (a.pos_open[c]) acc[0] += (double)gu[c] * (double)a.t[c];
            gr[3 + c] = a.scale_open[c] ? gu[3 + c] * (a.dsp[c] * asf) : 0.0f;
            if (a.scale_open[c]) acc[1] += (double)gu[3 + c] * (double)a.sp[c];
        }
        if (a.quat_live) {
            normalize_bwd<4>(a.q, a.qn, gu + 6, gr + 6);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) gr[6 + c] = 0.0f;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) gr[10 + c] = a.sg_live[c] ? gu[10 + c] * (a.sg[c] * (1.0f - a.sg[c])) : 0.0f;
        // the clamp of raw to [-10, 10] passes the gradient on the closed interval; a NaN fails both compares
#pragma unroll
        for (int c = 0; c < ROW; ++c) l_raw[tid * RP + c] = (x[c] >= -10.0f && x[c] <= 10.0f) ? gr[c] : 0.0f;  // the thread's own row
    }
    __syncthreads();
    rows_store<ROW, RP>(g_raw + (size_t)r0 * ROW, l_raw, nrows, tid);
    // fixed-shape tree over the block, one sum at a time: the same association every call
    double *l_sum = reinterpret_cast<double *>(l_up);  // (every read of l_up lies before the barrier above)
    static_assert(HB * RP * sizeof(float) >= HB * sizeof(double), "the tree reuses the upstream tile's LDS");
    for (int s = 0; s < 2; ++s) {
        __syncthreads();
        l_sum[tid] = acc[s];
        __syncthreads();
        for (int w = HB / 2; w > 0; w >>= 1) {
            if (tid < w) l_sum[tid] += l_sum[tid + w];
            __syncthreads();
        }
        if (tid == 0) partial[(size_t)blockIdx.x * 2 + s] = l_sum[0];
    }
}

// the two sums in a fixed order; d|s|/ds = sign(s), 0 at 0 (and for a NaN)
__global__ __launch_bounds__(FOLD_THREADS) void k_slat_fold(uint32_t parts, const double *__restrict__ partial,
                                                            const float *__restrict__ gains, float *__restrict__ g_gains) {
    __shared__ double l_sum[FOLD_THREADS];
    const int tid = threadIdx.x;
    for (int s = 0; s < 2; ++s) {
        double a = 0.0;
        for (uint32_t t = tid; t < parts; t += FOLD_THREADS) a += partial[(size_t)t * 2 + s];
        l_sum[tid] = a;
        __syncthreads();
        for (int w = FOLD_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) l_sum[tid] += l_sum[tid + w];
            __syncthreads();
        }
        if (tid == 0) {
            const float sf = gains[1];
            const double sign = sf > 0.0f ? 1.0 : (sf < 0.0f ? -1.0 : 0.0);
            g_gains[s] = (float)(s == 0 ? l_sum[0] : l_sum[0] * sign);
        }
        __syncthreads();
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
int geometry(int32_t batch, int32_t voxels, int32_t per_voxel, SlatGeom *g, uint32_t *tiles, const char *who) {
    if (batch < 1 || voxels < 1 || per_voxel < 1) {
        fgs_set_error("%s: invalid dims B=%d N=%d G=%d", who, batch, voxels, per_voxel);
        return FGS_EINVAL;
    }
    if (per_voxel > MAX_G) { fgs_set_error("%s: G = %d > %d is not supported", who, per_voxel, MAX_G); return FGS_EUNSUPPORTED; }
    const uint64_t rows = (uint64_t)batch * (uint64_t)voxels * (uint64_t)per_voxel;
    if (rows >= (1ull << 31)) {
        fgs_set_error("%s: B x N x G = %d x %d x %d is beyond the supported size", who, batch, voxels, per_voxel);
        return FGS_EUNSUPPORTED;
    }
    g->N = voxels; g->G = per_voxel; g->rows = (uint32_t)rows;
    *tiles = (uint32_t)((rows + HB - 1) / HB);
    return FGS_OK;
}

}  // namespace

extern "C" {

int fgs_slat_workspace_bytes(int32_t batch, int32_t voxels, int32_t per_voxel, size_t *scratch_bytes) {
    SlatGeom g;
    uint32_t tiles;
    int rc = geometry(batch, voxels, per_voxel, &g, &tiles, "fgs_slat_workspace_bytes");
    if (rc) return rc;
    if (!scratch_bytes) { fgs_set_error("fgs_slat_workspace_bytes: null output pointer"); return FGS_EINVAL; }
    // the gated forward's destination per voxel | the backward's two block partials per tile: whichever is larger
    const size_t dest = (size_t)batch * voxels * sizeof(int32_t), sums = (size_t)tiles * 2 * sizeof(double);
    *scratch_bytes = ((dest > sums ? dest : sums) + 255) & ~(size_t)255;
    return FGS_OK;
}

int fgs_slat_head_forward(int32_t batch, int32_t voxels, int32_t per_voxel, const float *raw, const int32_t *coords, const float *gains, const uint8_t *keep,
                          float *gaussians, int32_t *counts, void *scratch, void *stream) {
    SlatGeom g;
    uint32_t tiles;
    int rc = geometry(batch, voxels, per_voxel, &g, &tiles, "fgs_slat_head_forward");
    if (rc) return rc;
    if (!raw || !coords || !gains || !gaussians || (keep && (!counts || !scratch))) {
        fgs_set_error("fgs_slat_head_forward: null pointer argument (keep may be NULL, and with it counts and scratch)");
        return FGS_EINVAL;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (keep) {
        int32_t *dest = reinterpret_cast<int32_t *>(scratch);
        hipLaunchKernelGGL(k_slat_scan, dim3(batch), dim3(HB), 0, st, voxels, keep, dest, counts);
        FGS_LAUNCH_CHECK("k_slat_scan");
        hipLaunchKernelGGL(k_slat_fwd<true>, dim3(tiles), dim3(HB), 0, st, g, raw, coords, gains, dest, counts, gaussians);
        FGS_LAUNCH_CHECK("k_slat_fwd (gated)");
    } else {
        hipLaunchKernelGGL(k_slat_fwd<false>, dim3(tiles), dim3(HB), 0, st, g, raw, coords, gains, (const int32_t *)nullptr,
                           (const int32_t *)nullptr, gaussians);
        FGS_LAUNCH_CHECK("k_slat_fwd");
    }
    return FGS_OK;
}

int fgs_slat_head_backward(int32_t batch, int32_t voxels, int32_t per_voxel, const float *raw, const int32_t *coords, const float *gains,
                           const float *g_gaussians, float *g_raw, float *g_gains, void *scratch, void *stream) {
    SlatGeom g;
    uint32_t tiles;
    int rc = geometry(batch, voxels, per_voxel, &g, &tiles, "fgs_slat_head_backward");
    if (rc) return rc;
    if (!raw || !coords || !gains || !g_gaussians || !g_raw || !scratch) {
        fgs_set_error("fgs_slat_head_backward: null pointer argument (only g_gains may be NULL)");
        return FGS_EINVAL;
    }
    double *partial = reinterpret_cast<double *>(scratch);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_slat_bwd, dim3(tiles), dim3(HB), 0, st, g, raw, coords, gains, g_gaussians, g_raw, partial);
    FGS_LAUNCH_CHECK("k_slat_bwd");
    if (g_gains) {
        hipLaunchKernelGGL(k_slat_fold, dim3(1), dim3(FOLD_THREADS), 0, st, tiles, partial, gains, g_gains);
        FGS_LAUNCH_CHECK("k_slat_fold");
    }
    return FGS_OK;
}

}  // extern "C"
