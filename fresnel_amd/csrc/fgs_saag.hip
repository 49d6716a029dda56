// The two stages of the reference's SAAGRefinementNet (GDM:424-570, --experiment 1) that are not GEMMs: building the MLP's input
// (B, N, C + 14) from the feature grid and the SAAG cloud, and the residual head behind the MLP with its derivative.  N is the size
// of the SAAG cloud (tens of thousands), so both are bandwidth problems: the torch sequence writes or reads a tensor of the
// input's size three times (sample, permuted copy, concatenation); k_saag_inputs writes it once.
//
// k_saag_inputs<V>.  One WAVE per Gaussian, four Gaussians at a time per block of 256 threads, SPB Gaussians per block.  Every
// lane of the wave computes the Gaussian's sample point (the same few flops; the position is one broadcast read), then the lanes
// walk the channels: lane l takes channels V l, V l + 1, ... (+ 64 V).  With the training loop's channel-last view (channel
// stride 1: a texel's C channels are contiguous) the wave reads each of the four texel rows and writes the output row as
// consecutive lanes on consecutive addresses, V = 2 floats per lane where C is even and the pointers are 8-byte aligned (an
// output row is C + 14 floats: 1592 bytes at C = 384, a multiple of 8 and not of 16), V = 1 otherwise.  Lanes 0..13 then write
// the 14 SAAG parameters behind the features.  No LDS: nothing is shared between lanes.
// A CONTIGUOUS CHANNEL-FIRST tensor takes the same kernel with its own strides (the "second access pattern" of include/fgs.h):
// no transposed copy, no workspace; a lane's four reads are then 4-byte gathers a plane apart, served from L2 (one image's
// 37 x 37 x 384 grid is 2.1 MB), and the writes stay coalesced.  Both layouts evaluate the same expression per element: their
// outputs are bit-equal.
// Sampling (GDM:491-496 + F.grid_sample(bilinear, border, align_corners=False)): u = clamp((x / max(z, 0.1) + 2) / 4, 0, 1),
// ix = clip(u W - 0.5, 0, W - 1), corners from floor(ix); a corner outside the grid (index W or H, reached at ix = W - 1) has
// weight 0 and is NOT READ.
//
// k_saag_refine_fwd / k_saag_refine_bwd.  Thread = one Gaussian, block = a tile of 256 consecutive Gaussians of the flat (B N)
// axis; a fixed grid of at most MAX_PARTIALS blocks strides over the tiles.  A tile of every tensor is one contiguous piece of
// memory, copied whole through LDS (16 B per lane where the piece starts on a 16-byte address, fgs_gaussrow.h); the 16-float raw
// rows sit in LDS at stride 17, the 3-float rows at stride 3: a thread reading its own row meets no bank conflict.
// The backward recomputes the forward from `raw` with the same device functions (-ffp-contract=off, fresnel_amd/build.py):
// clamp gates (closed intervals) and the quaternion branch are the forward's.  The four gain gradients are sums of products of
// two floats, exact in double: a thread adds its Gaussians' products in tile order, the block folds its 256 sums in a
// fixed-shape tree, one partial per block and gain goes to `scratch`, and k_saag_gain_sum adds the partials in block order,
// multiplies by residual_scale and rounds to fp32 once.  No atomics: two calls agree to the bit.
#include "fgs_gaussrow.h"

#include <math.h>

namespace {

constexpr int SPB = 16;             // Gaussians per block of k_saag_inputs (four waves, four Gaussians each)
constexpr int MAX_PARTIALS = 1024;  // most blocks of the refine kernels = partial sums per gain
constexpr float NORM_EPS = 1e-12f;  // F.normalize's default eps (GDM:534)

struct SaagGeom {
    int32_t B, N, C, H, W;
    int64_t sb, sc, sy, sx;  // element strides of the features: batch, channel, row, column
    float residual_scale;
};
struct SaagCloud { const float *pos, *scale, *rot, *color, *opa; };

// ---- stage 1: the MLP's input ---------------------------------------------------------------------------------------------------
// V channels per lane and access
template <int V> struct Vec;
template <> struct Vec<1> { using T = float; };
template <> struct Vec<2> { using T = float2; };
__device__ __forceinline__ float lane_of(const float &v, int) { return v; }
__device__ __forceinline__ float lane_of(const float2 &v, int k) { return k == 0 ? v.x : v.y; }
__device__ __forceinline__ void set_lane_of(float &v, int, float x) { v = x; }
__device__ __forceinline__ void set_lane_of(float2 &v, int k, float x) { if (k == 0) v.x = x; else v.y = x; }

struct Sample { int x0, y0; float nw, ne, sw, se; bool right, below; };

__device__ __forceinline__ float unit_coord(float p, float z) {
    const float u = (p / fmaxf(z, 0.1f) + 2.0f) / 4.0f;
    return fminf(fmaxf(u, 0.0f), 1.0f);
}

__device__ __forceinline__ Sample sample_point(float x, float y, float z, int W, int H) {
    const float ix = fminf(fmaxf(unit_coord(x, z) * (float)W - 0.5f, 0.0f), (float)(W - 1));
    const float iy = fminf(fmaxf(unit_coord(y, z) * (float)H - 0.5f, 0.0f), (float)(H - 1));
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    Sample s;
    s.x0 = (int)fx0; s.y0 = (int)fy0;
    const float wx1 = ix - fx0, wx0 = (fx0 + 1.0f) - ix, wy1 = iy - fy0, wy0 = (fy0 + 1.0f) - iy;
    s.nw = wx0 * wy0; s.ne = wx1 * wy0; s.sw = wx0 * wy1; s.se = wx1 * wy1;
    // NaN coordinates: fmaxf / fminf drop the NaN, so x0, y0 are in range whatever the input
    s.x0 = min(max(s.x0, 0), W - 1); s.y0 = min(max(s.y0, 0), H - 1);
    s.right = s.x0 + 1 < W; s.below = s.y0 + 1 < H;
    return s;
}

template <int V>
__global__ __launch_bounds__(HB) void k_saag_inputs(SaagGeom g, const float *__restrict__ feat, SaagCloud in, float *__restrict__ out) {
    using T = typename Vec<V>::T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int row_w = g.C + 14;
    const float *fb = feat + (size_t)b * g.sb;
    for (int i = wave; i < SPB; i += HB / 64) {
        const int n = blockIdx.x * SPB + i;
        if (n >= g.N) break;  // (wave-uniform)
        const size_t pt = (size_t)b * g.N + n;
        const Sample s = sample_point(in.pos[3 * pt], in.pos[3 * pt + 1], in.pos[3 * pt + 2], g.W, g.H);
        const float *t00 = fb + (size_t)s.y0 * g.sy + (size_t)s.x0 * g.sx;
        float *o = out + pt * row_w;
        for (int c = lane * V; c < g.C; c += 64 * V) {
            const float *t = t00 + (size_t)c * g.sc;
            float acc[V];
            T v = *reinterpret_cast<const T *>(t);
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] = lane_of(v, k) * s.nw;
            if (s.right) {
                v = *reinterpret_cast<const T *>(t + g.sx);
#pragma unroll
                for (int k = 0; k < V; ++k) acc[k] += lane_of(v, k) * s.ne;
            }
            if (s.below) {
                v = *reinterpret_cast<const T *>(t + g.sy);
#pragma unroll
                for (int k = 0; k < V; ++k) acc[k] += lane_of(v, k) * s.sw;
                if (s.right) {
                    v = *reinterpret_cast<const T *>(t + g.sy + g.sx);
#pragma unroll
                    for (int k = 0; k < V; ++k) acc[k] += lane_of(v, k) * s.se;
                }
            }
            T r;
#pragma unroll
            for (int k = 0; k < V; ++k) set_lane_of(r, k, acc[k]);
            *reinterpret_cast<T *>(o + c) = r;
        }
        if (lane < 14) {  // [position 3 | scale 3 | rotation 4 | colour 3 | opacity 1]
            float v;
            if (lane < 3) v = in.pos[3 * pt + lane];
            else if (lane < 6) v = in.scale[3 * pt + lane - 3];
            else if (lane < 10) v = in.rot[4 * pt + lane - 6];
            else if (lane < 13) v = in.color[3 * pt + lane - 10];
            else v = in.opa[pt];
            o[g.C + lane] = v;
        }
    }
}

// ---- stage 2: the residual head -------------------------------------------------------------------------------------------------
struct RefineOut { float *pos, *scale, *rot, *color, *opa, *pd, *sd, *cd, *od; };
struct RefineUp { const float *pos, *scale, *rot, *color, *opa, *pd, *sd, *cd, *od; };

// delta = raw gain residual_scale, rounded as the reference's expression (GDM:515-519)
__device__ __forceinline__ float delta_of(float r, float gain, float rs) { return r * gain * rs; }

// Hamilton product a (x) b, (w, x, y, z) (GDM:555-570)
__device__ __forceinline__ void quat_mul(const float *a, const float *b, float *p) {
    p[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    p[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    p[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    p[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

// dL/da of p = a (x) b
__device__ __forceinline__ void quat_mul_bwd_left(const float *gp, const float *b, float *ga) {
    ga[0] = gp[0] * b[0] + gp[1] * b[1] + gp[2] * b[2] + gp[3] * b[3];
    ga[1] = -gp[0] * b[1] + gp[1] * b[0] - gp[2] * b[3] + gp[3] * b[2];
    ga[2] = -gp[0] * b[2] + gp[1] * b[3] + gp[2] * b[0] - gp[3] * b[1];
    ga[3] = -gp[0] * b[3] - gp[1] * b[2] + gp[2] * b[1] + gp[3] * b[0];
}

__device__ __forceinline__ float norm4(const float *p) { return sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3]); }

// adjoint of p / max(|p|, 1e-12): through the norm where it is not clamped; the norm's own subgradient at 0 is 0
__device__ __forceinline__ void normalize12_bwd(const float *p, float n, const float *g, float *gp) {
    if (n >= NORM_EPS) {
        const float gdotp = g[0] * p[0] + g[1] * p[1] + g[2] * p[2] + g[3] * p[3];
        const float w = gdotp / (n * n * n);
#pragma unroll
        for (int i = 0; i < 4; ++i) gp[i] = g[i] / n - p[i] * w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) gp[i] = g[i] / NORM_EPS;
    }
}

__device__ __forceinline__ float clamp01(float u) { return fminf(fmaxf(u, 0.0f), 1.0f); }
__device__ __forceinline__ float gate01(float u) { return (u >= 0.0f && u <= 1.0f) ? 1.0f : 0.0f; }  // closed, as torch.clamp's backward

__global__ __launch_bounds__(HB) void k_saag_refine_fwd(int32_t total, int32_t tiles, float rs, const float *__restrict__ raw,
                                                        SaagCloud in, const float *__restrict__ gains, RefineOut out) {
    __shared__ __attribute__((aligned(16))) float l_raw[HB * 17];
    __shared__ __attribute__((aligned(16))) float l_a[HB * 14];   // SAAG rows in, the five refined tensors out
    __shared__ __attribute__((aligned(16))) float l_d[HB * 10];   // the four deltas out
    const int tid = threadIdx.x;
    const float g_pos = gains[0], g_scale = gains[1], g_color = gains[2], g_opa = gains[3];
    float *a_pos = l_a, *a_scale = l_a + 3 * HB, *a_rot = l_a + 6 * HB, *a_color = l_a + 10 * HB, *a_opa = l_a + 13 * HB;
    float *d_pos = l_d, *d_scale = l_d + 3 * HB, *d_color = l_d + 6 * HB, *d_opa = l_d + 9 * HB;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t g0 = (size_t)tile * HB;
        const int ng = min(HB, total - tile * HB);
        rows_load<16, 17>(l_raw, raw + g0 * 16, ng, tid);
        tile_load(a_pos, in.pos + g0 * 3, ng * 3, tid);
        tile_load(a_scale, in.scale + g0 * 3, ng * 3, tid);
        tile_load(a_rot, in.rot + g0 * 4, ng * 4, tid);
        tile_load(a_color, in.color + g0 * 3, ng * 3, tid);
        tile_load(a_opa, in.opa + g0, ng, tid);
        __syncthreads();
        if (tid < ng) {  // a thread reads and overwrites its own rows only
            float r[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) r[c] = l_raw[tid * 17 + c];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float pd = delta_of(r[c], g_pos, rs), sd = delta_of(r[3 + c], g_scale, rs), cd = delta_of(r[12 + c], g_color, rs);
                d_pos[3 * tid + c] = pd; d_scale[3 * tid + c] = sd; d_color[3 * tid + c] = cd;
                a_pos[3 * tid + c] = a_pos[3 * tid + c] + pd;
                a_scale[3 * tid + c] = a_scale[3 * tid + c] * expf(sd);
                a_color[3 * tid + c] = clamp01(a_color[3 * tid + c] + cd);
            }
            const float od = delta_of(r[15], g_opa, rs);
            d_opa[tid] = od;
            a_opa[tid] = clamp01(a_opa[tid] + od);
            Rot rot;
            float qd[4], qs[4], p[4];
            rot_fwd(r + 6, r + 9, rot, qd);
#pragma unroll
            for (int i = 0; i < 4; ++i) qs[i] = a_rot[4 * tid + i];
            quat_mul(qd, qs, p);
            const float den = fmaxf(norm4(p), NORM_EPS);
#pragma unroll
            for (int i = 0; i < 4; ++i) a_rot[4 * tid + i] = p[i] / den;
        }
        __syncthreads();
        tile_store(out.pos + g0 * 3, a_pos, ng * 3, tid);
        tile_store(out.scale + g0 * 3, a_scale, ng * 3, tid);
        tile_store(out.rot + g0 * 4, a_rot, ng * 4, tid);
        tile_store(out.color + g0 * 3, a_color, ng * 3, tid);
        tile_store(out.opa + g0, a_opa, ng, tid);
        tile_store(out.pd + g0 * 3, d_pos, ng * 3, tid);
        tile_store(out.sd + g0 * 3, d_scale, ng * 3, tid);
        tile_store(out.cd + g0 * 3, d_color, ng * 3, tid);
        tile_store(out.od + g0, d_opa, ng, tid);
        __syncthreads();  // the next tile's loads overwrite what the stores read
    }
}

__global__ __launch_bounds__(HB) void k_saag_refine_bwd(int32_t total, int32_t tiles, float rs, const float *__restrict__ raw,
                                                        SaagCloud in, const float *__restrict__ gains, RefineUp up,
                                                        float *__restrict__ g_raw, double *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float l_raw[HB * 17];
    __shared__ __attribute__((aligned(16))) float l_a[HB * 14];   // SAAG rows
    __shared__ __attribute__((aligned(16))) float l_u[HB * 24];   // upstream gradients: 14 of the refined tensors, 10 of the deltas
    const int tid = threadIdx.x;
    const float g_pos = gains[0], g_scale = gains[1], g_color = gains[2], g_opa = gains[3];
    const float *a_scale = l_a + 3 * HB, *a_rot = l_a + 6 * HB, *a_color = l_a + 10 * HB, *a_opa = l_a + 13 * HB;
    float *u_pos = l_u, *u_scale = l_u + 3 * HB, *u_rot = l_u + 6 * HB, *u_color = l_u + 10 * HB, *u_opa = l_u + 13 * HB;
    float *u_pd = l_u + 14 * HB, *u_sd = l_u + 17 * HB, *u_cd = l_u + 20 * HB, *u_od = l_u + 23 * HB;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};  // this thread's share of dL/d gains / residual_scale: pos, scale, colour, opacity
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t g0 = (size_t)tile * HB;
        const int ng = min(HB, total - tile * HB);
        rows_load<16, 17>(l_raw, raw + g0 * 16, ng, tid);
        // (positions are not needed: d positions / d pos_delta = 1)
        tile_load(l_a + 3 * HB, in.scale + g0 * 3, ng * 3, tid);
        tile_load(l_a + 6 * HB, in.rot + g0 * 4, ng * 4, tid);
        tile_load(l_a + 10 * HB, in.color + g0 * 3, ng * 3, tid);
        tile_load(l_a + 13 * HB, in.opa + g0, ng, tid);
        if (up.pos) tile_load(u_pos, up.pos + g0 * 3, ng * 3, tid);
        if (up.scale) tile_load(u_scale, up.scale + g0 * 3, ng * 3, tid);
        if (up.rot) tile_load(u_rot, up.rot + g0 * 4, ng * 4, tid);
        if (up.color) tile_load(u_color, up.color + g0 * 3, ng * 3, tid);
        if (up.opa) tile_load(u_opa, up.opa + g0, ng, tid);
        if (up.pd) tile_load(u_pd, up.pd + g0 * 3, ng * 3, tid);
        if (up.sd) tile_load(u_sd, up.sd + g0 * 3, ng * 3, tid);
        if (up.cd) tile_load(u_cd, up.cd + g0 * 3, ng * 3, tid);
        if (up.od) tile_load(u_od, up.od + g0, ng, tid);
        __syncthreads();
        if (tid < ng) {
            float r[16], gr[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) { r[c] = l_raw[tid * 17 + c]; gr[c] = 0.0f; }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                // dL/d pos_delta, scale_delta, color_delta: through the refined tensor plus the delta's own upstream gradient
                float G = up.pos ? u_pos[3 * tid + c] : 0.0f;
                if (up.pd) G += u_pd[3 * tid + c];
                gr[c] = G * rs * g_pos;
                acc[0] += (double)G * (double)r[c];
                G = 0.0f;
                if (up.scale) {
                    const float sd = delta_of(r[3 + c], g_scale, rs);
                    G = u_scale[3 * tid + c] * (a_scale[3 * tid + c] * expf(sd));
                }
                if (up.sd) G += u_sd[3 * tid + c];
                gr[3 + c] = G * rs * g_scale;
                acc[1] += (double)G * (double)r[3 + c];
                G = 0.0f;
                if (up.color) G = u_color[3 * tid + c] * gate01(a_color[3 * tid + c] + delta_of(r[12 + c], g_color, rs));
                if (up.cd) G += u_cd[3 * tid + c];
                gr[12 + c] = G * rs * g_color;
                acc[2] += (double)G * (double)r[12 + c];
            }
            {
                float G = 0.0f;
                if (up.opa) G = u_opa[tid] * gate01(a_opa[tid] + delta_of(r[15], g_opa, rs));
                if (up.od) G += u_od[tid];
                gr[15] = G * rs * g_opa;
                acc[3] += (double)G * (double)r[15];
            }
            if (up.rot) {
                Rot rot;
                float qd[4], qs[4], p[4], gq[4], gp[4], gqd[4];
                rot_fwd(r + 6, r + 9, rot, qd);
#pragma unroll
                for (int i = 0; i < 4; ++i) { qs[i] = a_rot[4 * tid + i]; gq[i] = u_rot[4 * tid + i]; }
                quat_mul(qd, qs, p);
                normalize12_bwd(p, norm4(p), gq, gp);
                quat_mul_bwd_left(gp, qs, gqd);
                rot_bwd(r + 6, r + 9, rot, gqd, gr + 6, gr + 9);
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) l_raw[tid * 17 + c] = gr[c];  // a thread's own row
        }
        __syncthreads();
        rows_store<16, 17>(g_raw + g0 * 16, l_raw, ng, tid);
        __syncthreads();  // the next tile's loads overwrite what the stores read
    }
    // fixed-shape tree over the block, one gain at a time: the same association every call
    double *l_sum = reinterpret_cast<double *>(l_u);  // (every read of l_u lies before the loop's last barrier)
    for (int k = 0; k < 4; ++k) {
        l_sum[tid] = acc[k];
        __syncthreads();
        for (int w = HB / 2; w > 0; w >>= 1) {
            if (tid < w) l_sum[tid] += l_sum[tid + w];
            __syncthreads();
        }
        if (tid == 0) partial[(size_t)blockIdx.x * 4 + k] = l_sum[0];
        __syncthreads();
    }
}

// dL/d gains = residual_scale x the block partials, added in block order; rounded to fp32 once
__global__ __launch_bounds__(64) void k_saag_gain_sum(int32_t blocks, float rs, const double *__restrict__ partial,
                                                      float *__restrict__ g_gains) {
    const int k = threadIdx.x;
    if (blockIdx.x != 0 || k >= 4) return;
    double s = 0.0;
    for (int t = 0; t < blocks; ++t) s += partial[(size_t)t * 4 + k];
    g_gains[k] = (float)(s * (double)rs);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
int check_dims(const FgsSaagDims *d, SaagGeom *g, bool with_features, const char *who) {
    if (!d) { fgs_set_error("%s: null dims", who); return FGS_EINVAL; }
    if (d->batch < 1 || d->points < 1 || d->channels < 1 || d->grid_h < 1 || d->grid_w < 1) {
        fgs_set_error("%s: invalid dims B=%d N=%d C=%d grid=%dx%d", who, d->batch, d->points, d->channels, d->grid_h, d->grid_w);
        return FGS_EINVAL;
    }
    if (d->batch > 65535 || (uint64_t)d->batch * (uint64_t)d->points * (uint64_t)(d->channels + 14) >= (1ull << 31)) {
        fgs_set_error("%s: B=%d N=%d C=%d is beyond the supported size (B <= 65535, B N (C + 14) < 2^31)", who, d->batch, d->points,
                      d->channels);
        return FGS_EUNSUPPORTED;
    }
    g->B = d->batch; g->N = d->points; g->C = d->channels; g->H = d->grid_h; g->W = d->grid_w;
    g->sb = d->feat_stride_batch; g->sc = d->feat_stride_channel; g->sy = d->feat_stride_row;
    g->sx = d->feat_stride_channel == 1 ? d->channels : 1;
    g->residual_scale = d->residual_scale;
    if (with_features) {
        // the two layouts: channel-last (a texel's channels contiguous) | channel-first (a row's texels contiguous); rows and
        // images may be padded, never overlapping
        const int64_t row = g->sc == 1 ? (int64_t)g->W * g->C : (int64_t)g->W;
        const int64_t image = g->sc == 1 ? (int64_t)g->H * g->sy : (int64_t)g->C * g->sc;
        if (g->sc < 1 || g->sy < row || (g->sc != 1 && g->sc < (int64_t)g->H * g->sy) || g->sb < image) {
            fgs_set_error("%s: feature strides (batch %lld, channel %lld, row %lld) fit neither a channel-last nor a channel-first "
                          "(B, %d, %d, %d) tensor", who, (long long)g->sb, (long long)g->sc, (long long)g->sy, g->C, g->H, g->W);
            return FGS_EINVAL;
        }
    }
    return FGS_OK;
}

int32_t refine_blocks(const SaagGeom &g, int32_t *tiles) {
    *tiles = (int32_t)(((int64_t)g.B * g.N + HB - 1) / HB);
    return *tiles < MAX_PARTIALS ? *tiles : MAX_PARTIALS;
}

bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" {

int fgs_saag_workspace_bytes(const FgsSaagDims *dims, size_t *scratch_bytes) {
    SaagGeom g;
    int rc = check_dims(dims, &g, false, "fgs_saag_workspace_bytes");
    if (rc) return rc;
    if (!scratch_bytes) { fgs_set_error("fgs_saag_workspace_bytes: null output pointer"); return FGS_EINVAL; }
    int32_t tiles;
    *scratch_bytes = (((size_t)refine_blocks(g, &tiles) * 4 * sizeof(double)) + 255) & ~(size_t)255;
    return FGS_OK;
}

int fgs_saag_inputs_forward(const FgsSaagDims *dims, const float *features, const float *positions, const float *scales,
                            const float *rotations, const float *colors, const float *opacities, float *mlp_inputs, void *stream) {
    SaagGeom g;
    int rc = check_dims(dims, &g, true, "fgs_saag_inputs_forward");
    if (rc) return rc;
    if (!features || !positions || !scales || !rotations || !colors || !opacities || !mlp_inputs) {
        fgs_set_error("fgs_saag_inputs_forward: null pointer argument");
        return FGS_EINVAL;
    }
    SaagCloud in{positions, scales, rotations, colors, opacities};
    const dim3 grid((g.N + SPB - 1) / SPB, g.B);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // two channels per lane: channel-last, C even (every texel and every output row then starts on an even element) and both
    // base pointers 8-byte aligned
    const bool pairs = g.sc == 1 && g.C % 2 == 0 && g.sy % 2 == 0 && g.sb % 2 == 0 && aligned8(features) && aligned8(mlp_inputs);
    if (pairs) hipLaunchKernelGGL(k_saag_inputs<2>, grid, dim3(HB), 0, st, g, features, in, mlp_inputs);
    else hipLaunchKernelGGL(k_saag_inputs<1>, grid, dim3(HB), 0, st, g, features, in, mlp_inputs);
    FGS_LAUNCH_CHECK("k_saag_inputs");
    return FGS_OK;
}

int fgs_saag_refine_forward(const FgsSaagDims *dims, const float *raw, const float *positions, const float *scales,
                            const float *rotations, const float *colors, const float *opacities, const float *gains,
                            float *o_positions, float *o_scales, float *o_rotations, float *o_colors, float *o_opacities,
                            float *pos_delta, float *scale_delta, float *color_delta, float *opacity_delta, void *stream) {
    SaagGeom g;
    int rc = check_dims(dims, &g, false, "fgs_saag_refine_forward");
    if (rc) return rc;
    if (!raw || !positions || !scales || !rotations || !colors || !opacities || !gains || !o_positions || !o_scales || !o_rotations ||
        !o_colors || !o_opacities || !pos_delta || !scale_delta || !color_delta || !opacity_delta) {
        fgs_set_error("fgs_saag_refine_forward: null pointer argument");
        return FGS_EINVAL;
    }
    int32_t tiles;
    const int32_t blocks = refine_blocks(g, &tiles);
    SaagCloud in{positions, scales, rotations, colors, opacities};
    RefineOut out{o_positions, o_scales, o_rotations, o_colors, o_opacities, pos_delta, scale_delta, color_delta, opacity_delta};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_saag_refine_fwd, dim3(blocks), dim3(HB), 0, st, g.B * g.N, tiles, g.residual_scale, raw, in, gains, out);
    FGS_LAUNCH_CHECK("k_saag_refine_fwd");
    return FGS_OK;
}

int fgs_saag_refine_backward(const FgsSaagDims *dims, const float *raw, const float *scales, const float *rotations,
                             const float *colors, const float *opacities, const float *gains, const float *g_positions,
                             const float *g_scales, const float *g_rotations, const float *g_colors, const float *g_opacities,
                             const float *g_pos_delta, const float *g_scale_delta, const float *g_color_delta,
                             const float *g_opacity_delta, float *g_raw, float *g_gains, void *scratch, void *stream) {
    SaagGeom g;
    int rc = check_dims(dims, &g, false, "fgs_saag_refine_backward");
    if (rc) return rc;
    if (!raw || !scales || !rotations || !colors || !opacities || !gains || !g_raw || !g_gains || !scratch) {
        fgs_set_error("fgs_saag_refine_backward: null pointer argument (only the nine upstream gradients may be NULL)");
        return FGS_EINVAL;
    }
    int32_t tiles;
    const int32_t blocks = refine_blocks(g, &tiles);
    SaagCloud in{nullptr, scales, rotations, colors, opacities};
    RefineUp up{g_positions, g_scales, g_rotations, g_colors, g_opacities, g_pos_delta, g_scale_delta, g_color_delta, g_opacity_delta};
    double *partial = reinterpret_cast<double *>(scratch);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_saag_refine_bwd, dim3(blocks), dim3(HB), 0, st, g.B * g.N, tiles, g.residual_scale, raw, in, gains, up, g_raw,
                       partial);
    FGS_LAUNCH_CHECK("k_saag_refine_bwd");
    hipLaunchKernelGGL(k_saag_gain_sum, dim3(1), dim3(64), 0, st, blocks, g.residual_scale, partial, g_gains);
    FGS_LAUNCH_CHECK("k_saag_gain_sum");
    return FGS_OK;
}

}  // extern "C"
