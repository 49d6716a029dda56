// GaussianMatchingLoss of the reference's distillation path (scripts/training/train_direct_decoder.py, "TDD" 158-357): the
// bidirectional Chamfer loss between a predicted and a target cloud of 14-float Gaussians.  The reference forms it from
// 2048 x 2048 cdist chunks in two nested Python loops per direction and image, with boolean-index assignments that synchronise
// the host at every step.  Here the forward is four launches and the backward one; nothing synchronises.
//
// Definition: include/fgs.h (active rows, canonical match by (d2, j), the terms, the gradient's expression order).  This unit is
// compiled without FMA contraction and with IEEE divide / sqrt (fresnel_amd/build.py): tests/match_checker.py restates the
// match lists and the gradient rows bit for bit.
//
// k_match_compact.  One block per (image, side).  count -> scan -> emit over the side's rows in chunks of 256 (fgs_scan.h):
// the active rows' positions go to x / y / z planes in `scratch`, their original indices beside them, in ascending order; the
// block also writes the side's active count and the -1 entries of the inactive rows' match list.  Inactive rows never enter
// the matching loop and its trip count is one uniform device value.
//
// k_match_nearest.  Block = 64 compacted queries of one image and direction (blockIdx.z), FOUR lanes per query, as
// k_nca_perceive.  The candidates stream through LDS as x / y / z planes in tiles of FGS_MATCH_TILE, padded with +inf to the
// tile's end (a padded candidate's d2 is +inf or NaN: it never wins).  The four lanes of a query take groups of four
// candidates in turn (one ds_read_b128 per plane and group; lanes that share a group read the same address: broadcasts).  A
// lane walks ascending j with a strict `<` (false for a NaN d2), so it keeps the lowest index among equals; a lane that took
// nothing (all its candidates at +inf) falls back to its first candidate at +inf; the four are merged by (d2, j) in two
// shuffle steps.  Lane 0 of every query had candidate 0, so the merged index is always an active row's.
//
// k_match_terms / k_match_finish.  A fixed grid per image strides the rows; every per-element value is formed in fp32 and added
// in double; a fixed-shape block tree; the block partials are added in block order by one thread per image, which forms the
// means and the weighted terms in double and rounds each to fp32 once.
//
// k_match_bwd.  Block = 64 DESTINATION predictions of one image, four lanes per destination (position | scale | colour |
// opacity and quaternion).  The forward-direction term of the row first; then the coverage terms of the targets matched to it.
// The inverted index is a bit matrix in LDS (bit j of row i: bwd[j] == i), built from the image's `bwd` list in chunks of
// BWD_CHUNK targets with integer LDS atomics (order-free) and walked in ascending j: no float atomics, any in-degree.
#include "fgs_internal.h"
#include "fgs_scan.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int ROW = 14;                    // floats per Gaussian: position 0..2, scale 3..5, quaternion 6..9, colour 10..12, opacity 13
constexpr int QB = 64;                     // queries / destinations per block
constexpr int QL = 4;                      // lanes per query / destination
constexpr int MT = QB * QL;                // threads of every kernel here
constexpr int TILE = FGS_MATCH_TILE;       // candidates per LDS tile
constexpr int GROUP = 4 * QL;              // candidates the lanes of one query take per round
constexpr int BWD_CHUNK = 4096;            // targets per bit-matrix chunk of k_match_bwd
constexpr int BWD_WORDS = BWD_CHUNK / 32;
constexpr int BWD_WP = BWD_WORDS | 1;      // odd row stride: the rows a wave reads at once sit on different banks
constexpr int NSUM = 9;                    // position, scale, colour, opacity, |dot| ; coverage position, scale, colour, opacity
constexpr int MAX_TERM_BLOCKS = 32;
constexpr int MAX_N = 65536, MAX_B = 65535;
static_assert(TILE % GROUP == 0 && TILE >= GROUP, "the candidate tile is a whole number of lane rounds");

struct Sections {  // `scratch`, in 256-byte steps
    size_t xyz[2], idx[2], partial, total;
};

__host__ __device__ inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

__host__ Sections sections(const FgsMatchDims *d, int term_blocks) {
    Sections s;
    size_t at = 0;
    const size_t n[2] = {(size_t)d->batch * d->num_pred, (size_t)d->batch * d->num_target};
    for (int side = 0; side < 2; ++side) {
        s.xyz[side] = at; at += up256(3 * n[side] * sizeof(float));
        s.idx[side] = at; at += up256(n[side] * sizeof(int32_t));
    }
    s.partial = at; at += up256((size_t)d->batch * term_blocks * NSUM * sizeof(double));
    s.total = at;
    return s;
}

int term_blocks_of(const FgsMatchDims *d) {
    const int n = d->num_pred > d->num_target ? d->num_pred : d->num_target;
    const int blocks = (n + MT - 1) / MT;
    return blocks < MAX_TERM_BLOCKS ? blocks : MAX_TERM_BLOCKS;
}

// the reference's zero-padding filter (TDD:268-273) behind the keep byte
__device__ __forceinline__ bool row_active(const float *__restrict__ r, const uint8_t *__restrict__ keep, int i) {
    if (keep && keep[i] == 0) return false;
    const float s = (fabsf(r[0]) + fabsf(r[1])) + fabsf(r[2]);
    return (s > 1e-6f) | (fabsf(r[13]) > 1e-6f);
}

// ---- compaction -------------------------------------------------------------------------------------------------------------
struct Side {
    const float *rows;       // (B, N, 14)
    const uint8_t *keep;     // (B, N) or null
    float *xyz;              // (B, 3, N) planes of the active rows
    int32_t *idx;            // (B, N) their original indices
    int32_t *match;          // (B, N) the side's match list: -1 for the inactive rows here
    int32_t N;
};

__global__ __launch_bounds__(MT) void k_match_compact(Side s0, Side s1, int32_t *__restrict__ counts_out, int32_t *__restrict__ counts_saved) {
    const int b = blockIdx.x, side = blockIdx.y, tid = threadIdx.x;
    const Side s = side ? s1 : s0;
    const int N = s.N;
    const float *rows = s.rows + (size_t)b * N * ROW;
    const uint8_t *keep = s.keep ? s.keep + (size_t)b * N : nullptr;
    float *px = s.xyz + (size_t)b * 3 * N, *py = px + N, *pz = py + N;
    int32_t *idx = s.idx + (size_t)b * N, *match = s.match + (size_t)b * N;
    uint32_t base = 0;
    for (int i0 = 0; i0 < N; i0 += MT) {
        const int i = i0 + tid;
        const bool act = i < N && row_active(rows + (size_t)i * ROW, keep, i);
        uint32_t tot;
        const uint32_t at = base + block_exclusive_scan_256(act ? 1u : 0u, &tot);
        if (act) {
            const float *r = rows + (size_t)i * ROW;
            px[at] = r[0]; py[at] = r[1]; pz[at] = r[2];
            idx[at] = i;
        } else if (i < N) {
            match[i] = -1;
        }
        base += tot;
        __syncthreads();  // the scan's wave sums are reused by the next chunk
    }
    if (tid == 0) {
        counts_out[b * 2 + side] = (int32_t)base;
        counts_saved[b * 2 + side] = (int32_t)base;
    }
}

// ---- matching ---------------------------------------------------------------------------------------------------------------
struct MatchSide {
    const float *xyz;        // (B, 3, N)
    const int32_t *idx;      // (B, N)
    int32_t *match;          // (B, N)
    int32_t N;
};

__device__ __forceinline__ float dist2(float xi, float yi, float zi, float xj, float yj, float zj) {
    const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
    return (dx * dx + dy * dy) + dz * dz;
}

__global__ __launch_bounds__(MT) void k_match_nearest(MatchSide s0, MatchSide s1, const int32_t *__restrict__ counts) {
    __shared__ __attribute__((aligned(16))) float lx[TILE];
    __shared__ __attribute__((aligned(16))) float ly[TILE];
    __shared__ __attribute__((aligned(16))) float lz[TILE];
    const int b = blockIdx.y, dir = blockIdx.z, tid = threadIdx.x;
    const MatchSide qs = dir ? s1 : s0, cs = dir ? s0 : s1;  // dir 0: predictions -> targets
    const int nq = counts[b * 2 + dir], nc = counts[b * 2 + 1 - dir];
    const int p0 = blockIdx.x * QB;
    if (p0 >= nq) return;
    const int ql = tid >> 2, q = tid & 3;
    const int qi = min(p0 + ql, nq - 1);  // (lanes past the end work on the last query and drop the result: the merge needs every lane)
    const int32_t *qidx = qs.idx + (size_t)b * qs.N;
    int32_t *match = qs.match + (size_t)b * qs.N;
    if (nc == 0) {  // a skipped image: its active queries get -1 as well
        if (q == 0 && p0 + ql < nq) match[qidx[qi]] = -1;
        return;
    }
    const float *qx = qs.xyz + (size_t)b * 3 * qs.N, *qy = qx + qs.N, *qz = qy + qs.N;
    const float *cx = cs.xyz + (size_t)b * 3 * cs.N, *cy = cx + cs.N, *cz = cy + cs.N;
    const float xi = qx[qi], yi = qy[qi], zi = qz[qi];
    float bd = INFINITY;
    int bj = INT_MAX;
    for (int t0 = 0; t0 < nc; t0 += TILE) {
        __syncthreads();
        for (int e = tid; e < TILE; e += MT) {
            const int j = t0 + e;
            const bool in = j < nc;
            lx[e] = in ? cx[j] : INFINITY; ly[e] = in ? cy[j] : INFINITY; lz[e] = in ? cz[j] : INFINITY;
        }
        __syncthreads();
        const int len = min(TILE, (nc - t0 + GROUP - 1) / GROUP * GROUP);
        for (int jb = 4 * q; jb < len; jb += GROUP) {
            const float4 x4 = *reinterpret_cast<const float4 *>(lx + jb), y4 = *reinterpret_cast<const float4 *>(ly + jb),
                         z4 = *reinterpret_cast<const float4 *>(lz + jb);
            const float v0 = dist2(xi, yi, zi, x4.x, y4.x, z4.x), v1 = dist2(xi, yi, zi, x4.y, y4.y, z4.y),
                        v2 = dist2(xi, yi, zi, x4.z, y4.z, z4.z), v3 = dist2(xi, yi, zi, x4.w, y4.w, z4.w);
            const int j = t0 + jb;
            // ascending j, strict `<`: the lowest index among equals stays; false for a NaN d2
            if (v0 < bd) { bd = v0; bj = j; }
            if (v1 < bd) { bd = v1; bj = j + 1; }
            if (v2 < bd) { bd = v2; bj = j + 2; }
            if (v3 < bd) { bd = v3; bj = j + 3; }
        }
    }
    // every candidate of this lane at +inf (NaN counts as +inf): the first of them is the smallest (inf, j)
    if (bj == INT_MAX && 4 * q < nc) bj = 4 * q;
#pragma unroll
    for (int step = 1; step <= 2; step <<= 1) {
        const float od = __shfl_down(bd, step);
        const int oj = __shfl_down(bj, step);
        if ((od < bd) | ((od == bd) & (oj < bj))) { bd = od; bj = oj; }
    }
    if (q == 0 && p0 + ql < nq) match[qidx[qi]] = (cs.idx + (size_t)b * cs.N)[bj];
}

// ---- terms ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sq(float a, float b) { const float d = a - b; return d * d; }

// |q^a . q^b| with q^ = q / max(|q|, 1e-8)
__device__ __forceinline__ float clamp_norm(const float *q) {
    const float n = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    return n < 1e-8f ? 1e-8f : n;
}

__device__ __forceinline__ float unit_dot(const float *a, const float *b, float ca, float cb) {
    return (((a[0] / ca) * (b[0] / cb) + (a[1] / ca) * (b[1] / cb)) + (a[2] / ca) * (b[2] / cb)) + (a[3] / ca) * (b[3] / cb);
}

__device__ __forceinline__ void load_row(float *r, const float *__restrict__ src) {
    const float2 *s2 = reinterpret_cast<const float2 *>(src);  // rows are 56 bytes apart: 8-byte aligned
#pragma unroll
    for (int c = 0; c < ROW / 2; ++c) { const float2 v = s2[c]; r[2 * c] = v.x; r[2 * c + 1] = v.y; }
}

__global__ __launch_bounds__(MT) void k_match_terms(int32_t Np, int32_t Nt, const float *__restrict__ pred, const float *__restrict__ target,
                                                    const int32_t *__restrict__ fwd, const int32_t *__restrict__ bwd,
                                                    double *__restrict__ partial) {
    __shared__ double l_sum[NSUM][MT];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int stride = gridDim.x * MT;
    const float *P = pred + (size_t)b * Np * ROW, *T = target + (size_t)b * Nt * ROW;
    const int32_t *f = fwd + (size_t)b * Np, *w = bwd + (size_t)b * Nt;
    double acc[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) acc[k] = 0.0;
    float p[ROW], t[ROW];
    for (int i = blockIdx.x * MT + tid; i < Np; i += stride) {
        const int m = f[i];
        if (m < 0) continue;
        load_row(p, P + (size_t)i * ROW); load_row(t, T + (size_t)m * ROW);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            acc[0] += (double)sq(p[c], t[c]); acc[1] += (double)sq(p[3 + c], t[3 + c]); acc[2] += (double)sq(p[10 + c], t[10 + c]);
        }
        acc[3] += (double)sq(p[13], t[13]);
        acc[4] += (double)fabsf(unit_dot(p + 6, t + 6, clamp_norm(p + 6), clamp_norm(t + 6)));
    }
    for (int j = blockIdx.x * MT + tid; j < Nt; j += stride) {
        const int m = w[j];
        if (m < 0) continue;
        load_row(t, T + (size_t)j * ROW); load_row(p, P + (size_t)m * ROW);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            acc[5] += (double)sq(t[c], p[c]); acc[6] += (double)sq(t[3 + c], p[3 + c]); acc[7] += (double)sq(t[10 + c], p[10 + c]);
        }
        acc[8] += (double)sq(t[13], p[13]);
    }
#pragma unroll
    for (int k = 0; k < NSUM; ++k) l_sum[k][tid] = acc[k];
    __syncthreads();
    for (int h = MT / 2; h > 0; h >>= 1) {  // fixed-shape tree: the same association every call
        if (tid < h) {
#pragma unroll
            for (int k = 0; k < NSUM; ++k) l_sum[k][tid] += l_sum[k][tid + h];
        }
        __syncthreads();
    }
    if (tid < NSUM) partial[((size_t)b * gridDim.x + blockIdx.x) * NSUM + tid] = l_sum[tid][0];
}

__global__ __launch_bounds__(64) void k_match_finish(FgsMatchDims d, int32_t blocks, const double *__restrict__ partial,
                                                     const int32_t *__restrict__ counts, float *__restrict__ terms) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= d.batch) return;
    float *out = terms + (size_t)b * 8;
    const int np = counts[b * 2], nt = counts[b * 2 + 1];
    if (np == 0 || nt == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) out[k] = 0.0f;
        return;
    }
    double s[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) s[k] = 0.0;
    for (int t = 0; t < blocks; ++t) {  // block partials in block order
#pragma unroll
        for (int k = 0; k < NSUM; ++k) s[k] += partial[((size_t)b * blocks + t) * NSUM + k];
    }
    const double p3 = 3.0 * (double)np, p1 = (double)np, t3 = 3.0 * (double)nt, t1 = (double)nt;
    const double pos = s[0] / p3, scale = s[1] / p3, color = s[2] / p3, opacity = s[3] / p1, rot = 1.0 - s[4] / p1;
    const double cov = ((2.0 * (s[5] / t3) + 0.5 * (s[6] / t3)) + 0.5 * (s[7] / t3)) + 2.0 * (s[8] / t1);
    const double batch = (((((double)d.w_pos * pos + (double)d.w_scale * scale) + (double)d.w_rot * rot) + (double)d.w_color * color) +
                          (double)d.w_opacity * opacity) + (double)d.w_coverage * cov;
    out[0] = (float)pos; out[1] = (float)scale; out[2] = (float)rot; out[3] = (float)color; out[4] = (float)opacity;
    out[5] = (float)cov; out[6] = (float)batch; out[7] = 0.0f;
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MT) void k_match_bwd(FgsMatchDims d, float inv_b, const float *__restrict__ pred, const float *__restrict__ target,
                                                  const int32_t *__restrict__ fwd, const int32_t *__restrict__ bwd,
                                                  const int32_t *__restrict__ counts, const float *__restrict__ g_total,
                                                  float *__restrict__ g_pred) {
    __shared__ uint32_t rows[QB * BWD_WP];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int Np = d.num_pred, Nt = d.num_target;
    const int i0 = blockIdx.x * QB;
    const int npts = min(QB, Np - i0);
    const int il = tid >> 2, q = tid & 3;
    const int i = i0 + il;
    const float *P = pred + (size_t)b * Np * ROW, *T = target + (size_t)b * Nt * ROW;
    const int32_t *w = bwd + (size_t)b * Nt;
    const int np = counts[b * 2], nt = counts[b * 2 + 1];
    const int m = il < npts ? fwd[(size_t)b * Np + i] : -1;
    const bool live = (m >= 0) & (np > 0) & (nt > 0);
    // the lane's channels: q 0 position, 1 scale, 2 colour, 3 opacity (and the quaternion's forward term)
    const int c0 = q == 0 ? 0 : q == 1 ? 3 : q == 2 ? 10 : 13;
    const int nch = q == 3 ? 1 : 3;
    float g[3] = {0.0f, 0.0f, 0.0f}, gq[4] = {0.0f, 0.0f, 0.0f, 0.0f}, p[3] = {0.0f, 0.0f, 0.0f};
    float cc = 0.0f;  // the lane's coverage coefficient
    if (live) {
        const float gs = *g_total * inv_b;
        const float a3 = 2.0f / (float)(3 * np), a1 = 2.0f / (float)np, r1 = 1.0f / (float)np;
        const float b3 = 2.0f / (float)(3 * nt), b1 = 2.0f / (float)nt;
        const float gc = gs * d.w_coverage;
        const float wq = q == 0 ? d.w_pos : q == 1 ? d.w_scale : q == 2 ? d.w_color : d.w_opacity;
        const float kf = (gs * wq) * (q == 3 ? a1 : a3);
        cc = (gc * (q == 0 || q == 3 ? 2.0f : 0.5f)) * (q == 3 ? b1 : b3);
        const float *pr = P + (size_t)i * ROW, *tr = T + (size_t)m * ROW;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c < nch) {
                p[c] = pr[c0 + c];
                g[c] = kf * (p[c] - tr[c0 + c]);
            }
        }
        if (q == 3) {
            const float *qp = pr + 6, *qt = tr + 6;
            const float n = sqrtf(((qp[0] * qp[0] + qp[1] * qp[1]) + qp[2] * qp[2]) + qp[3] * qp[3]);
            const float cp = n < 1e-8f ? 1e-8f : n, ct = clamp_norm(qt);
            const float dot = unit_dot(qp, qt, cp, ct);
            const float sgn = (float)((dot > 0.0f) - (dot < 0.0f));
            const float e = -(((gs * d.w_rot) * r1) * sgn);
            float gh[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) gh[c] = e * (qt[c] / ct);
            if (n < 1e-8f) {  // the clamp is active: nothing flows through the norm
#pragma unroll
                for (int c = 0; c < 4; ++c) gq[c] = gh[c] / cp;
            } else {
                const float u = ((gh[0] * qp[0] + gh[1] * qp[1]) + gh[2] * qp[2]) + gh[3] * qp[3];
                const float v = ((u / cp) / cp) / n;
#pragma unroll
                for (int c = 0; c < 4; ++c) gq[c] = gh[c] / cp - qp[c] * v;
            }
        }
    }
    for (int j0 = 0; j0 < Nt; j0 += BWD_CHUNK) {
        const int len = min(BWD_CHUNK, Nt - j0);
        __syncthreads();
        for (int e = tid; e < QB * BWD_WP; e += MT) rows[e] = 0u;
        __syncthreads();
        for (int e = tid; e < len; e += MT) {
            const uint32_t r = (uint32_t)(w[j0 + e] - i0);
            if (r < (uint32_t)npts) atomicOr(&rows[r * BWD_WP + (e >> 5)], 1u << (e & 31));
        }
        __syncthreads();
        if (live) {
            const uint32_t *row = rows + il * BWD_WP;
            const int words = (len + 31) >> 5;
            for (int wd = 0; wd < words; ++wd) {
                uint32_t bits = row[wd];
                while (bits) {
                    const int j = j0 + wd * 32 + __builtin_ctz(bits);
                    bits &= bits - 1;
                    const float *tr = T + (size_t)j * ROW + c0;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        if (c < nch) g[c] = g[c] + cc * (p[c] - tr[c]);
                    }
                }
            }
        }
    }
    if (il < npts) {
        float *out = g_pred + ((size_t)b * Np + i) * ROW;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c < nch) out[c0 + c] = g[c];
        }
        if (q == 3) {
#pragma unroll
            for (int c = 0; c < 4; ++c) out[6 + c] = gq[c];
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
int check_dims(const FgsMatchDims *d, const char *who) {
    if (!d) { fgs_set_error("%s: null dims", who); return FGS_EINVAL; }
    if (d->batch < 1 || d->num_pred < 1 || d->num_target < 1) {
        fgs_set_error("%s: invalid dims B=%d Np=%d Nt=%d", who, d->batch, d->num_pred, d->num_target);
        return FGS_EINVAL;
    }
    if (d->batch > MAX_B || d->num_pred > MAX_N || d->num_target > MAX_N) {
        fgs_set_error("%s: B=%d Np=%d Nt=%d is beyond the supported shapes (B <= %d, Np, Nt <= %d)", who, d->batch, d->num_pred,
                      d->num_target, MAX_B, MAX_N);
        return FGS_EUNSUPPORTED;
    }
    return FGS_OK;
}

struct Saved { int32_t *fwd, *bwd, *counts; };
Saved saved_of(const FgsMatchDims *d, void *saved) {
    Saved s;
    s.fwd = reinterpret_cast<int32_t *>(saved);
    s.bwd = s.fwd + (size_t)d->batch * d->num_pred;
    s.counts = s.bwd + (size_t)d->batch * d->num_target;
    return s;
}

}  // namespace

extern "C" {

int fgs_match_workspace_bytes(const FgsMatchDims *dims, size_t *saved_bytes, size_t *scratch_bytes) {
    int rc = check_dims(dims, "fgs_match_workspace_bytes");
    if (rc) return rc;
    if (!saved_bytes || !scratch_bytes) { fgs_set_error("fgs_match_workspace_bytes: null output pointer"); return FGS_EINVAL; }
    // fwd (B, Np), bwd (B, Nt), counts (B, 2): int32, every element written by the forward
    *saved_bytes = ((size_t)dims->batch * ((size_t)dims->num_pred + (size_t)dims->num_target + 2)) * sizeof(int32_t);
    *scratch_bytes = sections(dims, term_blocks_of(dims)).total;
    return FGS_OK;
}

int fgs_match_forward(const FgsMatchDims *dims, const float *pred, const float *target, const uint8_t *pred_keep,
                      const uint8_t *target_keep, float *terms, int32_t *counts, void *saved, void *scratch, void *stream) {
    int rc = check_dims(dims, "fgs_match_forward");
    if (rc) return rc;
    if (!pred || !target || !terms || !counts || !saved || !scratch) { fgs_set_error("fgs_match_forward: null pointer argument"); return FGS_EINVAL; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int blocks = term_blocks_of(dims);
    const Sections sec = sections(dims, blocks);
    char *base = reinterpret_cast<char *>(scratch);
    const Saved sv = saved_of(dims, saved);
    Side side[2];
    side[0] = Side{pred, pred_keep, reinterpret_cast<float *>(base + sec.xyz[0]), reinterpret_cast<int32_t *>(base + sec.idx[0]), sv.fwd, dims->num_pred};
    side[1] = Side{target, target_keep, reinterpret_cast<float *>(base + sec.xyz[1]), reinterpret_cast<int32_t *>(base + sec.idx[1]), sv.bwd, dims->num_target};
    hipLaunchKernelGGL(k_match_compact, dim3(dims->batch, 2), dim3(MT), 0, st, side[0], side[1], counts, sv.counts);
    FGS_LAUNCH_CHECK("k_match_compact");
    const MatchSide m0{side[0].xyz, side[0].idx, sv.fwd, dims->num_pred}, m1{side[1].xyz, side[1].idx, sv.bwd, dims->num_target};
    const int nmax = dims->num_pred > dims->num_target ? dims->num_pred : dims->num_target;
    hipLaunchKernelGGL(k_match_nearest, dim3((nmax + QB - 1) / QB, dims->batch, 2), dim3(MT), 0, st, m0, m1, sv.counts);
    FGS_LAUNCH_CHECK("k_match_nearest");
    double *partial = reinterpret_cast<double *>(base + sec.partial);
    hipLaunchKernelGGL(k_match_terms, dim3(blocks, dims->batch), dim3(MT), 0, st, dims->num_pred, dims->num_target, pred, target, sv.fwd,
                       sv.bwd, partial);
    FGS_LAUNCH_CHECK("k_match_terms");
    hipLaunchKernelGGL(k_match_finish, dim3((dims->batch + 63) / 64), dim3(64), 0, st, *dims, blocks, partial, sv.counts, terms);
    FGS_LAUNCH_CHECK("k_match_finish");
    return FGS_OK;
}

int fgs_match_backward(const FgsMatchDims *dims, const float *pred, const float *target, const void *saved, const float *g_total,
                       float *g_pred, void *scratch, void *stream) {
    int rc = check_dims(dims, "fgs_match_backward");
    if (rc) return rc;
    if (!pred || !target || !saved || !g_total || !g_pred) { fgs_set_error("fgs_match_backward: null pointer argument"); return FGS_EINVAL; }
    (void)scratch;  // the inverted index is built in LDS
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const Saved sv = saved_of(dims, const_cast<void *>(saved));
    const float inv_b = 1.0f / (float)dims->batch;
    hipLaunchKernelGGL(k_match_bwd, dim3((dims->num_pred + QB - 1) / QB, dims->batch), dim3(MT), 0, st, *dims, inv_b, pred, target, sv.fwd,
                       sv.bwd, sv.counts, g_total, g_pred);
    FGS_LAUNCH_CHECK("k_match_bwd");
    return FGS_OK;
}

}  // extern "C"
