// Gaussian-parameter head of the reference's patch decoders (DirectPatchDecoder GDM:845-922, FibonacciPatchDecoder
// GDM:1674-1723, rotation_6d_to_quaternion GDM:186-276): the elementwise map from the MLP's raw (B, P, K_full, 16 | 19) output to
// the renderer's inputs, and its exact derivative.  The reference spends ~45 elementwise torch kernels on it forward and twice
// that backward; here it is ONE launch each way (plus a B-thread launch that finishes dL/d opacity_mod).
//
// Thread mapping.  A block takes TP consecutive points of one image, TP x K_full <= 256 rows of `raw`; thread = one row
// (point, k).  The block's rows are one contiguous piece of `raw` and its Gaussians one contiguous piece of every output, so
// all global traffic is whole-tile copies with consecutive lanes on consecutive addresses -- 16 B per lane where the piece
// starts on a 16-byte address (always for C = 16 with K = K_full; for C = 19 and the 3-float outputs when the tile's first
// element does), 4 B per lane otherwise -- staged through LDS: the 64- / 76-byte rows and 12-byte output rows would otherwise
// be strided 4-byte accesses.  Raw rows sit in LDS at an odd stride (17 | 19 words), 3-float outputs at stride 3: a thread
// reading or writing its own row meets no bank conflict.  Rows k >= K (progressive growing, GDM:790-792) idle in the
// forward and write zeros to g_raw in the backward.
//
// Sums.  No atomics: dL/d base_z and dL/d edge (sums over a point's K Gaussians) are added in k order by the point's first
// thread -- a point never straddles blocks; dL/d opacity_mod is a fixed-shape tree over the block, one partial per block
// in `scratch`, added in tile order by k_head_mod_sum.  Results repeat bit for bit.
//
// Nothing is saved between forward and backward: the backward recomputes the forward from `raw` with the same device
// functions (and -ffp-contract=off, fresnel_amd/build.py), so its clamp gates and quaternion branch are the forward's.
#include "fgs_gaussrow.h"  // tile copies (HB threads), rot_fwd / rot_bwd, EPS: shared with fgs_saag.hip

namespace {

constexpr int UP_FLOATS = 17;  // upstream-gradient / output floats of one Gaussian: 3 + 3 + 4 + 3 + 1 + 3
constexpr float TWO_PI = 6.283185307179586f;

struct HeadGeom {
    int32_t P, KF, K, TP;
    float xy_gain, edge_scale, edge_boost;
};
struct HeadIn { const float *raw, *base_xy, *base_z, *pose, *opacity_mod, *edge; };
struct HeadOut { float *pos, *scale, *rot, *color, *opa, *phase; };
struct HeadUp { const float *pos, *scale, *rot, *color, *opa, *phase; };

// ---- the map, piece by piece ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoid_(float x) { return 1.0f / (1.0f + expf(-x)); }

// scale channel (GDM:864-867): clamp(softplus(clamp(r, -10, 20) + 1) * 0.15, 1e-6, 2); *ds = d scale / d r
__device__ __forceinline__ float scale_fwd(float r, float *ds) {
    const float u = fminf(fmaxf(r, -10.0f), 20.0f) + 1.0f;
    float sp, dsp;
    if (u > 20.0f) {  // torch's softplus: linear above the threshold
        sp = u; dsp = 1.0f;
    } else {
        const float z = expf(u);
        sp = log1pf(z); dsp = z / (z + 1.0f);
    }
    const float s = sp * 0.15f;
    if (ds) *ds = (r >= -10.0f && r <= 20.0f && s >= 1e-6f && s <= 2.0f) ? dsp * 0.15f : 0.0f;
    return fminf(fmaxf(s, 1e-6f), 2.0f);
}

// opacity chain (GDM:876, 893-894, 912): sigmoid, + boost * edge clamped to [0, 1], * opacity_mod clamped to [0, 1].
// d_raw / d_edge / d_mod: derivatives of the result (closed-interval clamp gates)
__device__ __forceinline__ float opacity_fwd(float r, bool has_edge, float e, float boost, bool has_mod, float m,
                                             float *d_raw, float *d_edge, float *d_mod) {
    const float o0 = sigmoid_(r);
    float o = o0, chain = 1.0f, de = 0.0f, dm = 0.0f;
    if (has_edge) {
        const float u = o0 + boost * e;
        const float gate = (u >= 0.0f && u <= 1.0f) ? 1.0f : 0.0f;
        o = fminf(fmaxf(u, 0.0f), 1.0f);
        chain = gate;
        de = gate * boost;
    }
    if (has_mod) {
        const float u = o * m;
        const float gate = (u >= 0.0f && u <= 1.0f) ? 1.0f : 0.0f;
        dm = gate * o;
        chain *= gate * m;
        de *= gate * m;
        o = fminf(fmaxf(u, 0.0f), 1.0f);
    }
    if (d_raw) { *d_raw = chain * o0 * (1.0f - o0); *d_edge = de; *d_mod = dm; }
    return o;
}

// ---- forward --------------------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(HB) void k_head_fwd(HeadGeom g, HeadIn in, HeadOut out) {
    constexpr int CP = C | 1;
    static_assert(CP >= (C == 19 ? UP_FLOATS : UP_FLOATS - 3), "the output tiles reuse the raw tile's LDS");
    __shared__ __attribute__((aligned(16))) float lds[HB * CP];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int p0 = blockIdx.x * g.TP;
    const int npts = min(g.TP, g.P - p0);
    const int nrows = npts * g.KF;
    const size_t pt0 = (size_t)b * g.P + p0;
    rows_load<C, CP>(lds, in.raw + pt0 * g.KF * C, nrows, tid);
    __syncthreads();
    const int lp = tid / g.KF, k = tid - lp * g.KF;
    const bool active = tid < nrows && k < g.K;
    float r[C];
    if (active) {
#pragma unroll
        for (int c = 0; c < C; ++c) r[c] = lds[tid * CP + c];
    }
    __syncthreads();  // every row is in registers: the tile's LDS now takes the outputs
    float *l_pos = lds, *l_scale = lds + 3 * HB, *l_rot = lds + 6 * HB, *l_color = lds + 10 * HB, *l_opa = lds + 13 * HB,
          *l_phase = lds + 14 * HB;
    if (active) {
        const int lg = lp * g.K + k;
        const size_t pt = pt0 + lp;
        const bool has_edge = in.edge != nullptr;
        const float e = has_edge ? in.edge[pt] : 0.0f;
        // positions (GDM:847-860): z is the depth's, the grid / spiral point moves by xy_gain * raw
        float x = in.base_xy[2 * (p0 + lp)] + r[0] * g.xy_gain;
        float y = in.base_xy[2 * (p0 + lp) + 1] + r[1] * g.xy_gain;
        float z = in.base_z[pt];
        if (in.pose) {  // rotate_positions_for_pose (GDM:96-104): azimuth about Y, then elevation about X
            const float ca = in.pose[4 * b], sa = in.pose[4 * b + 1], ce = in.pose[4 * b + 2], se = in.pose[4 * b + 3];
            const float xr = x * ca + z * sa, zr = -x * sa + z * ca;
            const float yr = y * ce - zr * se, zf = y * se + zr * ce;
            x = xr; y = yr; z = zf;
        }
        l_pos[3 * lg] = x; l_pos[3 * lg + 1] = y; l_pos[3 * lg + 2] = z;
        const float shrink = has_edge ? 1.0f - g.edge_scale * e : 1.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float s = scale_fwd(r[3 + c], nullptr);
            l_scale[3 * lg + c] = has_edge ? s * shrink : s;
            l_color[3 * lg + c] = sigmoid_(r[12 + c]);
        }
        Rot rot;
        float q[4];
        rot_fwd(r + 6, r + 9, rot, q);
        *reinterpret_cast<float4 *>(l_rot + 4 * lg) = make_float4(q[0], q[1], q[2], q[3]);
        l_opa[lg] = opacity_fwd(r[15], has_edge, e, g.edge_boost, in.opacity_mod != nullptr,
                                in.opacity_mod ? in.opacity_mod[b] : 1.0f, nullptr, nullptr, nullptr);
        if constexpr (C == 19) {
#pragma unroll
            for (int c = 0; c < 3; ++c) l_phase[3 * lg + c] = sigmoid_(r[16 + c]) * TWO_PI;
        }
    }
    __syncthreads();
    const int ng = npts * g.K;
    const size_t g0 = pt0 * g.K;
    tile_store(out.pos + g0 * 3, l_pos, ng * 3, tid);
    tile_store(out.scale + g0 * 3, l_scale, ng * 3, tid);
    tile_store(out.rot + g0 * 4, l_rot, ng * 4, tid);
    tile_store(out.color + g0 * 3, l_color, ng * 3, tid);
    tile_store(out.opa + g0, l_opa, ng, tid);
    if constexpr (C == 19) tile_store(out.phase + g0 * 3, l_phase, ng * 3, tid);
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(HB) void k_head_bwd(HeadGeom g, HeadIn in, HeadUp up, float *g_raw, float *g_base_z, float *g_edge,
                                                 float *partial) {
    constexpr int CP = C | 1;
    __shared__ __attribute__((aligned(16))) float l_raw[HB * CP];
    __shared__ __attribute__((aligned(16))) float l_up[HB * UP_FLOATS];
    __shared__ float l_z[HB], l_e[HB], l_m[HB];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int p0 = blockIdx.x * g.TP;
    const int npts = min(g.TP, g.P - p0);
    const int nrows = npts * g.KF;
    const int ng = npts * g.K;
    const size_t pt0 = (size_t)b * g.P + p0;
    const size_t g0 = pt0 * g.K;
    float *u_pos = l_up, *u_scale = l_up + 3 * HB, *u_rot = l_up + 6 * HB, *u_color = l_up + 10 * HB, *u_opa = l_up + 13 * HB,
          *u_phase = l_up + 14 * HB;
    rows_load<C, CP>(l_raw, in.raw + pt0 * g.KF * C, nrows, tid);
    if (up.pos) tile_load(u_pos, up.pos + g0 * 3, ng * 3, tid);
    if (up.scale) tile_load(u_scale, up.scale + g0 * 3, ng * 3, tid);
    if (up.rot) tile_load(u_rot, up.rot + g0 * 4, ng * 4, tid);
    if (up.color) tile_load(u_color, up.color + g0 * 3, ng * 3, tid);
    if (up.opa) tile_load(u_opa, up.opa + g0, ng, tid);
    if constexpr (C == 19) {
        if (up.phase) tile_load(u_phase, up.phase + g0 * 3, ng * 3, tid);
    }
    __syncthreads();
    const int lp = tid / g.KF, k = tid - lp * g.KF;
    const bool active = tid < nrows && k < g.K;
    float gz = 0.0f, ge = 0.0f, gm = 0.0f;
    if (active) {
        const int lg = lp * g.K + k;
        const size_t pt = pt0 + lp;
        float r[C], gr[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { r[c] = l_raw[tid * CP + c]; gr[c] = 0.0f; }
        const bool has_edge = in.edge != nullptr;
        const float e = has_edge ? in.edge[pt] : 0.0f;
        if (up.pos) {
            float gx = u_pos[3 * lg], gy = u_pos[3 * lg + 1];
            gz = u_pos[3 * lg + 2];
            if (in.pose) {
                const float ca = in.pose[4 * b], sa = in.pose[4 * b + 1], ce = in.pose[4 * b + 2], se = in.pose[4 * b + 3];
                const float gyy = gy * ce + gz * se, gzr = -gy * se + gz * ce;
                const float gxx = gx * ca - gzr * sa;
                gz = gx * sa + gzr * ca;
                gx = gxx; gy = gyy;
            }
            gr[0] = gx * g.xy_gain;
            gr[1] = gy * g.xy_gain;  // raw[2] is not used (z is locked to the depth, GDM:850): its gradient stays 0
        }
        if (up.scale) {
            const float shrink = has_edge ? 1.0f - g.edge_scale * e : 1.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float ds;
                const float s = scale_fwd(r[3 + c], &ds);
                const float gs = u_scale[3 * lg + c];
                gr[3 + c] = has_edge ? gs * shrink * ds : gs * ds;
                if (has_edge) ge -= gs * s * g.edge_scale;
            }
        }
        if (up.rot) {
            Rot rot;
            float q[4], gq[4];
            rot_fwd(r + 6, r + 9, rot, q);
#pragma unroll
            for (int i = 0; i < 4; ++i) gq[i] = u_rot[4 * lg + i];
            rot_bwd(r + 6, r + 9, rot, gq, gr + 6, gr + 9);
        }
        if (up.color) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float s = sigmoid_(r[12 + c]);
                gr[12 + c] = u_color[3 * lg + c] * s * (1.0f - s);
            }
        }
        if (up.opa) {
            float d_raw, d_edge, d_mod;
            opacity_fwd(r[15], has_edge, e, g.edge_boost, in.opacity_mod != nullptr, in.opacity_mod ? in.opacity_mod[b] : 1.0f,
                        &d_raw, &d_edge, &d_mod);
            const float go = u_opa[lg];
            gr[15] = go * d_raw;
            ge += go * d_edge;
            gm = go * d_mod;
        }
        if constexpr (C == 19) {
            if (up.phase) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float s = sigmoid_(r[16 + c]);
                    gr[16 + c] = u_phase[3 * lg + c] * TWO_PI * s * (1.0f - s);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) l_raw[tid * CP + c] = gr[c];  // a thread's own row: nobody else reads it before the barrier
    } else if (tid < nrows) {
#pragma unroll
        for (int c = 0; c < C; ++c) l_raw[tid * CP + c] = 0.0f;   // the K_full - K unused Gaussians
    }
    l_z[tid] = gz; l_e[tid] = ge; l_m[tid] = gm;
    __syncthreads();
    rows_store<C, CP>(g_raw + pt0 * g.KF * C, l_raw, nrows, tid);
    if (tid < nrows && k == 0) {  // the point's K contributions in k order
        float sz = 0.0f, se = 0.0f;
        for (int kk = 0; kk < g.K; ++kk) { sz += l_z[tid + kk]; se += l_e[tid + kk]; }
        if (g_base_z) g_base_z[pt0 + lp] = sz;
        if (g_edge) g_edge[pt0 + lp] = se;
    }
    if (partial) {  // fixed-shape tree: the same association every call
        for (int w = HB / 2; w > 0; w >>= 1) {
            if (tid < w) l_m[tid] += l_m[tid + w];
            __syncthreads();
        }
        if (tid == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = l_m[0];
    }
}

// dL/d opacity_mod[b] = the image's tile partials, added in tile order
__global__ __launch_bounds__(64) void k_head_mod_sum(int32_t B, int32_t tiles, const float *partial, float *g_mod) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    float s = 0.0f;
    for (int t = 0; t < tiles; ++t) s += partial[(size_t)b * tiles + t];
    g_mod[b] = s;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
int geometry(const FgsHeadDims *d, HeadGeom *g, int32_t *tiles, const char *who) {
    if (!d) { fgs_set_error("%s: null dims", who); return FGS_EINVAL; }
    if (d->batch < 1 || d->points < 1 || d->k_full < 1 || d->k_used < 1 || d->k_used > d->k_full ||
        (d->channels != 16 && d->channels != 19)) {
        fgs_set_error("%s: invalid dims B=%d P=%d K_full=%d K=%d C=%d", who, d->batch, d->points, d->k_full, d->k_used, d->channels);
        return FGS_EINVAL;
    }
    if ((uint64_t)d->batch * (uint64_t)d->points * (uint64_t)d->k_full * (uint64_t)d->channels >= (1ull << 31) || d->batch > 65535) {
        fgs_set_error("%s: B x P x K_full x C = %d x %d x %d x %d is beyond the supported size", who, d->batch, d->points, d->k_full,
                      d->channels);
        return FGS_EUNSUPPORTED;
    }
    if (d->k_full > 64) { fgs_set_error("%s: K_full = %d > 64 is not supported", who, d->k_full); return FGS_EUNSUPPORTED; }
    // points per tile: as many as fit 256 rows, with TP x K_full a multiple of 4 so that tiles of an aligned image stay aligned
    const int32_t step = d->k_full % 4 == 0 ? 1 : (d->k_full % 2 == 0 ? 2 : 4);
    int32_t tp = HB / d->k_full / step * step;
    g->P = d->points; g->KF = d->k_full; g->K = d->k_used; g->TP = tp;
    g->xy_gain = d->xy_gain; g->edge_scale = d->edge_scale_factor; g->edge_boost = d->edge_opacity_boost;
    *tiles = (d->points + tp - 1) / tp;
    return FGS_OK;
}

}  // namespace

extern "C" {

int fgs_head_workspace_bytes(const FgsHeadDims *dims, size_t *scratch_bytes) {
    HeadGeom g;
    int32_t tiles;
    int rc = geometry(dims, &g, &tiles, "fgs_head_workspace_bytes");
    if (rc) return rc;
    if (!scratch_bytes) { fgs_set_error("fgs_head_workspace_bytes: null output pointer"); return FGS_EINVAL; }
    *scratch_bytes = (((size_t)dims->batch * tiles * sizeof(float)) + 255) & ~(size_t)255;
    return FGS_OK;
}

int fgs_head_forward(const FgsHeadDims *dims, const float *raw, const float *base_xy, const float *base_z, const float *pose,
                     const float *opacity_mod, const float *edge, float *positions, float *scales, float *rotations,
                     float *colors, float *opacities, float *phases, void *stream) {
    HeadGeom g;
    int32_t tiles;
    int rc = geometry(dims, &g, &tiles, "fgs_head_forward");
    if (rc) return rc;
    if (!raw || !base_xy || !base_z || !positions || !scales || !rotations || !colors || !opacities ||
        (dims->channels == 19 && !phases)) {
        fgs_set_error("fgs_head_forward: null pointer argument");
        return FGS_EINVAL;
    }
    HeadIn in{raw, base_xy, base_z, pose, opacity_mod, edge};
    HeadOut out{positions, scales, rotations, colors, opacities, phases};
    const dim3 grid(tiles, dims->batch);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dims->channels == 19) hipLaunchKernelGGL(k_head_fwd<19>, grid, dim3(HB), 0, st, g, in, out);
    else hipLaunchKernelGGL(k_head_fwd<16>, grid, dim3(HB), 0, st, g, in, out);
    FGS_LAUNCH_CHECK("k_head_fwd");
    return FGS_OK;
}

int fgs_head_backward(const FgsHeadDims *dims, const float *raw, const float *pose, const float *opacity_mod, const float *edge,
                      const float *g_positions, const float *g_scales, const float *g_rotations, const float *g_colors,
                      const float *g_opacities, const float *g_phases, float *g_raw, float *g_base_z, float *g_edge,
                      float *g_opacity_mod, void *scratch, void *stream) {
    HeadGeom g;
    int32_t tiles;
    int rc = geometry(dims, &g, &tiles, "fgs_head_backward");
    if (rc) return rc;
    if (!raw || !g_raw) { fgs_set_error("fgs_head_backward: null raw / g_raw"); return FGS_EINVAL; }
    if ((g_edge && !edge) || (g_opacity_mod && !opacity_mod) || (g_opacity_mod && !scratch)) {
        fgs_set_error("fgs_head_backward: g_edge needs edge, g_opacity_mod needs opacity_mod and scratch");
        return FGS_EINVAL;
    }
    HeadIn in{raw, nullptr, nullptr, pose, opacity_mod, edge};
    HeadUp up{g_positions, g_scales, g_rotations, g_colors, g_opacities, dims->channels == 19 ? g_phases : nullptr};
    float *partial = g_opacity_mod ? reinterpret_cast<float *>(scratch) : nullptr;
    const dim3 grid(tiles, dims->batch);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dims->channels == 19) hipLaunchKernelGGL(k_head_bwd<19>, grid, dim3(HB), 0, st, g, in, up, g_raw, g_base_z, g_edge, partial);
    else hipLaunchKernelGGL(k_head_bwd<16>, grid, dim3(HB), 0, st, g, in, up, g_raw, g_base_z, g_edge, partial);
    FGS_LAUNCH_CHECK("k_head_bwd");
    if (g_opacity_mod) {
        hipLaunchKernelGGL(k_head_mod_sum, dim3((dims->batch + 63) / 64), dim3(64), 0, st, dims->batch, tiles, partial, g_opacity_mod);
        FGS_LAUNCH_CHECK("k_head_mod_sum");
    }
    return FGS_OK;
}

}  // extern "C"
