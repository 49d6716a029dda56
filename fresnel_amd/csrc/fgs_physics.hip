// Parameter head of the reference's PhysicsDirectPatchDecoder (GDM:955-1147) with its physics-derived phase (PhysicsFresnelZones
// depth_to_phase, scripts/utils/fresnel_zones.py:555-575): the map from the MLP's raw (B, P, K_full, 16) output to the wave
// renderer's inputs, and its exact derivative.  In torch it is about 40 small launches each way.
//
// The head differs from fgs_head.hip's in three ways: scales are softplus(raw + 1) 0.15 WITHOUT clamps, there is no pose, edge or
// opacity modulation, and the phase is one scalar per Gaussian computed from the depth: with z = base_z of the Gaussian's patch,
//     D = (z_max - z_min) + 1e-8      u = (z - z_min) / D      lambda = clamp(|wavelength_raw|, lambda_min, lambda_max)
//     phase = fmod((2 pi / lambda) |u - focal_depth|, 2 pi)
// every operation rounded to fp32 on its own (include/fgs.h), z_min / z_max over all B x P patches.  The phase is a patch's: it
// is computed once per patch, by the patch's thread, and its K Gaussians copy it.
//
// Forward, two launches.  k_phys_range finds z_min, z_max and how many patches hold each (the tie counts the backward divides by):
// ONE block of 1024 threads up to RANGE_BLOCK_ITEMS = 16 384 values (the workload's B x P is 10 952: 11 loads per thread, one
// tree) writes the 16-byte result directly; beyond that up to RANGE_MAX_BLOCKS blocks stride over the values, write one partial
// each into `scratch`, and k_phys_range_fold folds the partials.  Its own launch rather than a recomputation per block of
// k_phys_fwd: the 350 head blocks of the workload would each read all 44 KB again and sit through the same tree before their
// first store.  A NaN anywhere makes z_min and z_max NaN (fminf alone would drop it), and with them every phase, as torch.
// k_phys_fwd is k_head_fwd's tiling: a block takes TP consecutive patches of one image, TP x K_full <= 256 rows of `raw`, thread =
// one row; whole-tile copies through LDS (fgs_gaussrow.h).
//
// Backward, three launches; it recomputes the forward from `raw` and the 16-byte range.  k_phys_bwd writes g_raw and, per patch,
// dL/dz through the position and through u (the patch's K upstream gradients added in k order by the patch's first thread), and
// three block partials in double: S1 = sum g_u, S2 = sum g_u u, S3 = sum G |u - f| (g_u = G c sgn(u - f), G the patch's summed
// phase gradient; products of two floats, exact in double; fixed-shape block tree).  k_phys_sums adds the partials in a fixed
// order (thread t takes partials t, t + 256, ...; fixed tree) and forms g_z_min = (S2 - S1) / D, g_z_max = -S2 / D and
// dL/d wavelength_raw = -S3 c / lambda x [lambda_min <= |raw| <= lambda_max] x sign(raw).  k_phys_depth finishes dL/d base_z: it
// adds g_u / D (g_u per patch rides in `scratch`) and g_z_min / n_min, g_z_max / n_max for every patch that holds the minimum /
// maximum -- torch's min() / max() share their gradient equally among ties -- in double, rounded once.  No atomics anywhere: two
// calls agree to the bit.
#include "fgs_gaussrow.h"  // tile copies (HB threads), rot_fwd / rot_bwd

#include <math.h>

namespace {

constexpr int UP_FLOATS = 15;             // upstream-gradient / output floats of one Gaussian: 3 + 3 + 4 + 3 + 1 + 1
constexpr float TWO_PI = 6.283185307179586f;
constexpr int RANGE_THREADS = 1024;       // threads per block of k_phys_range
constexpr int RANGE_BLOCK_ITEMS = 16384;  // most values of a single-block range call: 16 per thread
constexpr int RANGE_MAX_BLOCKS = 32;      // most blocks (= partials) of a multi-block range call
constexpr int SUM_THREADS = 256;          // threads of k_phys_sums: thread t adds partials t, t + 256, ...
constexpr size_t SCRATCH_HEAD = 256;      // bytes in front of the partials: the two tie shares (doubles)

struct PhysGeom {
    int32_t P, KF, K, TP;
    float xy_gain, focal, lmin, lmax;
};
struct PhysRange { float zmin, zmax; int32_t nmin, nmax; };  // the 16 bytes `range` holds
struct PhysOut { float *pos, *scale, *rot, *color, *opa, *phase; };
struct PhysUp { const float *pos, *scale, *rot, *color, *opa, *phase; };

// ---- the map, piece by piece ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoid_(float x) { return 1.0f / (1.0f + expf(-x)); }

// scale channel (GDM:1104): softplus(r + 1) * 0.15, no clamps; *ds = d scale / d r
__device__ __forceinline__ float scale_fwd(float r, float *ds) {
    const float u = r + 1.0f;
    float sp, dsp;
    if (u > 20.0f) {  // torch's softplus: linear above the threshold
        sp = u; dsp = 1.0f;
    } else {
        const float z = expf(u);
        sp = log1pf(z); dsp = z / (z + 1.0f);
    }
    if (ds) *ds = dsp * 0.15f;
    return sp * 0.15f;
}

// lambda = clamp(|raw|, lmin, lmax) (NaN stays NaN, as torch.clamp), c = 2 pi / lambda; open: the clamp passes the gradient
struct Wave { float lam, c; bool open; };
__device__ __forceinline__ Wave wave_of(float raw, float lmin, float lmax) {
    const float a = fabsf(raw);
    Wave w;
    w.lam = a != a ? a : fminf(fmaxf(a, lmin), lmax);
    w.c = TWO_PI / w.lam;
    w.open = a >= lmin && a <= lmax;
    return w;
}

// the phase of one patch; D, u and pd = |u - f| for the backward
__device__ __forceinline__ float phase_fwd(float z, const PhysRange &rg, float c, float f, float *D, float *u, float *pd) {
    *D = (rg.zmax - rg.zmin) + 1e-8f;
    *u = (z - rg.zmin) / *D;
    *pd = fabsf(*u - f);
    return fmodf(c * *pd, TWO_PI);
}

// ---- range ----------------------------------------------------------------------------------------------------------------------
// (min, max, counts) of two pieces; a NaN minimum marks a piece that met a NaN
__device__ __forceinline__ PhysRange range_join(const PhysRange &a, const PhysRange &b) {
    PhysRange r;
    if (a.zmin != a.zmin || b.zmin != b.zmin) {
        r.zmin = r.zmax = __builtin_nanf(""); r.nmin = r.nmax = 0;
        return r;
    }
    r.zmin = fminf(a.zmin, b.zmin);
    r.zmax = fmaxf(a.zmax, b.zmax);
    r.nmin = (a.zmin == r.zmin ? a.nmin : 0) + (b.zmin == r.zmin ? b.nmin : 0);
    r.nmax = (a.zmax == r.zmax ? a.nmax : 0) + (b.zmax == r.zmax ? b.nmax : 0);
    return r;
}

// fixed-shape tree over the block's T pieces (T a power of two); the result is l[0]
template <int T>
__device__ __forceinline__ void range_tree(PhysRange *l, int tid) {
    for (int w = T / 2; w > 0; w >>= 1) {
        if (tid < w) l[tid] = range_join(l[tid], l[tid + w]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(RANGE_THREADS) void k_phys_range(int32_t n, const float *__restrict__ z, PhysRange *__restrict__ out) {
    __shared__ PhysRange l[RANGE_THREADS];
    const int tid = threadIdx.x;
    PhysRange r{INFINITY, -INFINITY, 0, 0};  // the empty piece: neutral in range_join
    for (int64_t i = (int64_t)blockIdx.x * RANGE_THREADS + tid; i < n; i += (int64_t)gridDim.x * RANGE_THREADS) {
        const float v = z[i];
        r = range_join(r, PhysRange{v, v, 1, 1});
    }
    l[tid] = r;
    __syncthreads();
    range_tree<RANGE_THREADS>(l, tid);
    if (tid == 0) out[blockIdx.x] = l[0];
}

__global__ __launch_bounds__(64) void k_phys_range_fold(int32_t parts, const PhysRange *__restrict__ partial, PhysRange *__restrict__ out) {
    __shared__ PhysRange l[64];
    static_assert(RANGE_MAX_BLOCKS <= 64, "one partial per thread");
    const int tid = threadIdx.x;
    l[tid] = tid < parts ? partial[tid] : PhysRange{INFINITY, -INFINITY, 0, 0};
    __syncthreads();
    range_tree<64>(l, tid);
    if (tid == 0) *out = l[0];
}

// ---- forward --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HB) void k_phys_fwd(PhysGeom g, const float *__restrict__ raw, const float *__restrict__ base_xy,
                                                 const float *__restrict__ base_z, const float *__restrict__ wavelength_raw,
                                                 const PhysRange *__restrict__ range, PhysOut out) {
    __shared__ __attribute__((aligned(16))) float lds[HB * 17];
    __shared__ float l_z[HB], l_ph[HB];  // per patch of the tile (at most HB of them, K_full = 1)
    static_assert(17 >= UP_FLOATS, "the output tiles reuse the raw tile's LDS");
    const int tid = threadIdx.x, b = blockIdx.y;
    const int p0 = blockIdx.x * g.TP;
    const int npts = min(g.TP, g.P - p0);
    const int nrows = npts * g.KF;
    const size_t pt0 = (size_t)b * g.P + p0;
    rows_load<16, 17>(lds, raw + pt0 * g.KF * 16, nrows, tid);
    if (tid < npts) {  // the patch's depth and phase, once
        const PhysRange rg = *range;
        const Wave w = wave_of(*wavelength_raw, g.lmin, g.lmax);
        const float z = base_z[pt0 + tid];
        float D, u, pd;
        l_z[tid] = z;
        l_ph[tid] = phase_fwd(z, rg, w.c, g.focal, &D, &u, &pd);
    }
    __syncthreads();
    const int lp = tid / g.KF, k = tid - lp * g.KF;
    const bool active = tid < nrows && k < g.K;
    float r[16];
    if (active) {
#pragma unroll
        for (int c = 0; c < 16; ++c) r[c] = lds[tid * 17 + c];
    }
    __syncthreads();  // every row is in registers: the tile's LDS now takes the outputs
    float *l_pos = lds, *l_scale = lds + 3 * HB, *l_rot = lds + 6 * HB, *l_color = lds + 10 * HB, *l_opa = lds + 13 * HB,
          *l_phase = lds + 14 * HB;
    if (active) {
        const int lg = lp * g.K + k;
        // positions (GDM:1097-1101): z is the depth's, the grid point moves by xy_gain * raw
        l_pos[3 * lg] = base_xy[2 * (p0 + lp)] + r[0] * g.xy_gain;
        l_pos[3 * lg + 1] = base_xy[2 * (p0 + lp) + 1] + r[1] * g.xy_gain;
        l_pos[3 * lg + 2] = l_z[lp];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            l_scale[3 * lg + c] = scale_fwd(r[3 + c], nullptr);
            l_color[3 * lg + c] = sigmoid_(r[12 + c]);
        }
        Rot rot;
        float q[4];
        rot_fwd(r + 6, r + 9, rot, q);
        *reinterpret_cast<float4 *>(l_rot + 4 * lg) = make_float4(q[0], q[1], q[2], q[3]);
        l_opa[lg] = sigmoid_(r[15]);
        l_phase[lg] = l_ph[lp];
    }
    __syncthreads();
    const int ng = npts * g.K;
    const size_t g0 = pt0 * g.K;
    tile_store(out.pos + g0 * 3, l_pos, ng * 3, tid);
    tile_store(out.scale + g0 * 3, l_scale, ng * 3, tid);
    tile_store(out.rot + g0 * 4, l_rot, ng * 4, tid);
    tile_store(out.color + g0 * 3, l_color, ng * 3, tid);
    tile_store(out.opa + g0, l_opa, ng, tid);
    tile_store(out.phase + g0, l_phase, ng, tid);
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HB) void k_phys_bwd(PhysGeom g, const float *__restrict__ raw, const float *__restrict__ base_z,
                                                 const float *__restrict__ wavelength_raw, const PhysRange *__restrict__ range,
                                                 PhysUp up, float *__restrict__ g_raw, float *__restrict__ g_base_z,
                                                 double *__restrict__ partial, float *__restrict__ g_u) {
    __shared__ __attribute__((aligned(16))) float l_raw[HB * 17];
    __shared__ __attribute__((aligned(16))) float l_up[HB * UP_FLOATS];
    __shared__ float l_gz[HB], l_gp[HB];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int p0 = blockIdx.x * g.TP;
    const int npts = min(g.TP, g.P - p0);
    const int nrows = npts * g.KF;
    const int ng = npts * g.K;
    const size_t pt0 = (size_t)b * g.P + p0;
    const size_t g0 = pt0 * g.K;
    float *u_pos = l_up, *u_scale = l_up + 3 * HB, *u_rot = l_up + 6 * HB, *u_color = l_up + 10 * HB, *u_opa = l_up + 13 * HB,
          *u_phase = l_up + 14 * HB;
    rows_load<16, 17>(l_raw, raw + pt0 * g.KF * 16, nrows, tid);
    if (up.pos) tile_load(u_pos, up.pos + g0 * 3, ng * 3, tid);
    if (up.scale) tile_load(u_scale, up.scale + g0 * 3, ng * 3, tid);
    if (up.rot) tile_load(u_rot, up.rot + g0 * 4, ng * 4, tid);
    if (up.color) tile_load(u_color, up.color + g0 * 3, ng * 3, tid);
    if (up.opa) tile_load(u_opa, up.opa + g0, ng, tid);
    if (up.phase) tile_load(u_phase, up.phase + g0, ng, tid);
    __syncthreads();
    const int lp = tid / g.KF, k = tid - lp * g.KF;
    const bool active = tid < nrows && k < g.K;
    float gz = 0.0f, gp = 0.0f;
    if (active) {
        const int lg = lp * g.K + k;
        float r[16], gr[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) { r[c] = l_raw[tid * 17 + c]; gr[c] = 0.0f; }
        if (up.pos) {
            gr[0] = u_pos[3 * lg] * g.xy_gain;
            gr[1] = u_pos[3 * lg + 1] * g.xy_gain;  // raw[2] is not used (z is locked to the depth, GDM:1100): its gradient stays 0
            gz = u_pos[3 * lg + 2];
        }
        if (up.scale) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float ds;
                scale_fwd(r[3 + c], &ds);
                gr[3 + c] = u_scale[3 * lg + c] * ds;
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
            const float s = sigmoid_(r[15]);
            gr[15] = u_opa[lg] * s * (1.0f - s);
        }
        if (up.phase) gp = u_phase[lg];
#pragma unroll
        for (int c = 0; c < 16; ++c) l_raw[tid * 17 + c] = gr[c];  // a thread's own row: nobody else reads it before the barrier
    } else if (tid < nrows) {
#pragma unroll
        for (int c = 0; c < 16; ++c) l_raw[tid * 17 + c] = 0.0f;   // the K_full - K unused Gaussians
    }
    l_gz[tid] = gz; l_gp[tid] = gp;
    __syncthreads();
    rows_store<16, 17>(g_raw + pt0 * g.KF * 16, l_raw, nrows, tid);
    double acc[3] = {0.0, 0.0, 0.0};  // this thread's patch: g_u, g_u u, G |u - f|
    if (tid < nrows && k == 0) {  // the patch's K contributions in k order
        float sz = 0.0f, G = 0.0f;
        for (int kk = 0; kk < g.K; ++kk) { sz += l_gz[tid + kk]; G += l_gp[tid + kk]; }
        float gu = 0.0f;
        if (up.phase) {
            const PhysRange rg = *range;
            const Wave w = wave_of(*wavelength_raw, g.lmin, g.lmax);
            float D, u, pd;
            phase_fwd(base_z[pt0 + lp], rg, w.c, g.focal, &D, &u, &pd);
            const float sgn = u > g.focal ? 1.0f : (u < g.focal ? -1.0f : 0.0f);  // |.| has gradient 0 at 0
            gu = (G * w.c) * sgn;
            acc[0] = (double)gu; acc[1] = (double)gu * (double)u; acc[2] = (double)G * (double)pd;
        }
        if (g_base_z) g_base_z[pt0 + lp] = sz;  // k_phys_depth adds g_u / D and the tie shares, in double
        g_u[pt0 + lp] = gu;
    }
    // fixed-shape tree over the block, one sum at a time: the same association every call
    double *l_sum = reinterpret_cast<double *>(l_up);  // (every read of l_up lies before the barrier above)
    static_assert(HB * UP_FLOATS * sizeof(float) >= HB * sizeof(double), "the tree reuses the upstream tile's LDS");
    for (int s = 0; s < 3; ++s) {
        __syncthreads();
        l_sum[tid] = acc[s];
        __syncthreads();
        for (int w = HB / 2; w > 0; w >>= 1) {
            if (tid < w) l_sum[tid] += l_sum[tid + w];
            __syncthreads();
        }
        if (tid == 0) partial[((size_t)b * gridDim.x + blockIdx.x) * 3 + s] = l_sum[0];
    }
}

// the three sums in a fixed order, then g_z_min / n_min, g_z_max / n_max (to `shares`) and dL/d wavelength_raw
__global__ __launch_bounds__(SUM_THREADS) void k_phys_sums(int32_t parts, PhysGeom g, const double *__restrict__ partial,
                                                           const float *__restrict__ wavelength_raw,
                                                           const PhysRange *__restrict__ range, double *__restrict__ shares,
                                                           float *__restrict__ g_wavelength_raw) {
    __shared__ double l_sum[SUM_THREADS];
    __shared__ double total[3];
    const int tid = threadIdx.x;
    for (int s = 0; s < 3; ++s) {
        double a = 0.0;
        for (int t = tid; t < parts; t += SUM_THREADS) a += partial[(size_t)t * 3 + s];
        l_sum[tid] = a;
        __syncthreads();
        for (int w = SUM_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) l_sum[tid] += l_sum[tid + w];
            __syncthreads();
        }
        if (tid == 0) total[s] = l_sum[0];
        __syncthreads();
    }
    if (tid != 0) return;
    const PhysRange rg = *range;
    const float raw = *wavelength_raw;
    const Wave w = wave_of(raw, g.lmin, g.lmax);
    const double D = (double)((rg.zmax - rg.zmin) + 1e-8f);
    shares[0] = (total[1] - total[0]) / D / (double)rg.nmin;
    shares[1] = -total[1] / D / (double)rg.nmax;
    if (g_wavelength_raw) {
        const double sign = raw > 0.0f ? 1.0 : (raw < 0.0f ? -1.0 : 0.0);  // |.| has gradient 0 at 0
        *g_wavelength_raw = w.open ? (float)(-total[2] * (double)w.c / (double)w.lam * sign) : 0.0f;
    }
}

// dL/d base_z = the position's part (already there) + g_u / D + the tie shares: torch's min() / max() give their gradient in equal
// shares to every element that holds the extremum.  Formed in double and rounded once: the phase part of sum dL/d base_z cancels
// exactly in exact arithmetic (u does not move when every z moves), and here it cancels to the last rounding -- where z is constant
// (D = 1e-8) the terms are 1e8 times the upstream gradient.
__global__ __launch_bounds__(HB) void k_phys_depth(int32_t n, const float *__restrict__ base_z, const PhysRange *__restrict__ range,
                                                   const double *__restrict__ shares, const float *__restrict__ g_u,
                                                   float *__restrict__ g_base_z) {
    const int64_t i = (int64_t)blockIdx.x * HB + threadIdx.x;
    if (i >= n) return;
    const PhysRange rg = *range;
    const float z = base_z[i];
    double v = (double)g_base_z[i] + (double)g_u[i] / (double)((rg.zmax - rg.zmin) + 1e-8f);
    if (z == rg.zmin) v += shares[0];
    if (z == rg.zmax) v += shares[1];
    g_base_z[i] = (float)v;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
int geometry(const FgsPhysicsDims *d, PhysGeom *g, int32_t *tiles, const char *who) {
    if (!d) { fgs_set_error("%s: null dims", who); return FGS_EINVAL; }
    if (d->batch < 1 || d->points < 1 || d->k_full < 1 || d->k_used < 1 || d->k_used > d->k_full) {
        fgs_set_error("%s: invalid dims B=%d P=%d K_full=%d K=%d", who, d->batch, d->points, d->k_full, d->k_used);
        return FGS_EINVAL;
    }
    if (!(d->wavelength_min > 0.0f) || !(d->wavelength_max >= d->wavelength_min)) {
        fgs_set_error("%s: the wavelength clamp [%g, %g] must satisfy 0 < min <= max", who, d->wavelength_min, d->wavelength_max);
        return FGS_EINVAL;
    }
    if ((uint64_t)d->batch * (uint64_t)d->points * (uint64_t)d->k_full * 16ull >= (1ull << 31) || d->batch > 65535) {
        fgs_set_error("%s: B x P x K_full x 16 = %d x %d x %d x 16 is beyond the supported size", who, d->batch, d->points, d->k_full);
        return FGS_EUNSUPPORTED;
    }
    if (d->k_full > 64) { fgs_set_error("%s: K_full = %d > 64 is not supported", who, d->k_full); return FGS_EUNSUPPORTED; }
    // patches per tile: as many as fit 256 rows, with TP x K_full a multiple of 4 so that tiles of an aligned image stay aligned
    const int32_t step = d->k_full % 4 == 0 ? 1 : (d->k_full % 2 == 0 ? 2 : 4);
    const int32_t tp = HB / d->k_full / step * step;
    g->P = d->points; g->KF = d->k_full; g->K = d->k_used; g->TP = tp;
    g->xy_gain = d->xy_gain; g->focal = d->focal_depth; g->lmin = d->wavelength_min; g->lmax = d->wavelength_max;
    *tiles = (d->points + tp - 1) / tp;
    return FGS_OK;
}

int32_t range_blocks(int64_t n) {
    const int64_t blocks = (n + RANGE_BLOCK_ITEMS - 1) / RANGE_BLOCK_ITEMS;
    return (int32_t)(blocks < RANGE_MAX_BLOCKS ? blocks : RANGE_MAX_BLOCKS);
}

}  // namespace

extern "C" {

int fgs_physics_workspace_bytes(const FgsPhysicsDims *dims, size_t *scratch_bytes) {
    PhysGeom g;
    int32_t tiles;
    int rc = geometry(dims, &g, &tiles, "fgs_physics_workspace_bytes");
    if (rc) return rc;
    if (!scratch_bytes) { fgs_set_error("fgs_physics_workspace_bytes: null output pointer"); return FGS_EINVAL; }
    // the backward's: tie shares | three block partials per tile | g_u per patch;  the forward's range partials fit the front
    const size_t sums = (size_t)dims->batch * tiles * 3 * sizeof(double), gu = (size_t)dims->batch * dims->points * sizeof(float);
    const size_t need = sums + gu > RANGE_MAX_BLOCKS * sizeof(PhysRange) ? sums + gu : RANGE_MAX_BLOCKS * sizeof(PhysRange);
    *scratch_bytes = (SCRATCH_HEAD + need + 255) & ~(size_t)255;
    return FGS_OK;
}

int fgs_physics_forward(const FgsPhysicsDims *dims, const float *raw, const float *base_xy, const float *base_z,
                        const float *wavelength_raw, float *positions, float *scales, float *rotations, float *colors,
                        float *opacities, float *phases, void *range, void *scratch, void *stream) {
    PhysGeom g;
    int32_t tiles;
    int rc = geometry(dims, &g, &tiles, "fgs_physics_forward");
    if (rc) return rc;
    if (!raw || !base_xy || !base_z || !wavelength_raw || !positions || !scales || !rotations || !colors || !opacities || !phases ||
        !range || !scratch) {
        fgs_set_error("fgs_physics_forward: null pointer argument");
        return FGS_EINVAL;
    }
    const int64_t n = (int64_t)dims->batch * dims->points;
    const int32_t rb = range_blocks(n);
    PhysRange *rg = reinterpret_cast<PhysRange *>(range);
    PhysRange *parts = reinterpret_cast<PhysRange *>(reinterpret_cast<char *>(scratch) + SCRATCH_HEAD);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_phys_range, dim3(rb), dim3(RANGE_THREADS), 0, st, (int32_t)n, base_z, rb == 1 ? rg : parts);
    FGS_LAUNCH_CHECK("k_phys_range");
    if (rb > 1) {
        hipLaunchKernelGGL(k_phys_range_fold, dim3(1), dim3(64), 0, st, rb, parts, rg);
        FGS_LAUNCH_CHECK("k_phys_range_fold");
    }
    PhysOut out{positions, scales, rotations, colors, opacities, phases};
    hipLaunchKernelGGL(k_phys_fwd, dim3(tiles, dims->batch), dim3(HB), 0, st, g, raw, base_xy, base_z, wavelength_raw, rg, out);
    FGS_LAUNCH_CHECK("k_phys_fwd");
    return FGS_OK;
}

int fgs_physics_backward(const FgsPhysicsDims *dims, const float *raw, const float *base_z, const float *wavelength_raw,
                         const void *range, const float *g_positions, const float *g_scales, const float *g_rotations,
                         const float *g_colors, const float *g_opacities, const float *g_phases, float *g_raw, float *g_base_z,
                         float *g_wavelength_raw, void *scratch, void *stream) {
    PhysGeom g;
    int32_t tiles;
    int rc = geometry(dims, &g, &tiles, "fgs_physics_backward");
    if (rc) return rc;
    if (!raw || !base_z || !wavelength_raw || !range || !g_raw || !scratch) {
        fgs_set_error("fgs_physics_backward: null pointer argument (only the six upstream gradients, g_base_z and g_wavelength_raw "
                      "may be NULL)");
        return FGS_EINVAL;
    }
    const PhysRange *rg = reinterpret_cast<const PhysRange *>(range);
    double *shares = reinterpret_cast<double *>(scratch);
    double *partial = reinterpret_cast<double *>(reinterpret_cast<char *>(scratch) + SCRATCH_HEAD);
    float *g_u = reinterpret_cast<float *>(partial + (size_t)dims->batch * tiles * 3);
    PhysUp up{g_positions, g_scales, g_rotations, g_colors, g_opacities, g_phases};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_phys_bwd, dim3(tiles, dims->batch), dim3(HB), 0, st, g, raw, base_z, wavelength_raw, rg, up, g_raw, g_base_z,
                       partial, g_u);
    FGS_LAUNCH_CHECK("k_phys_bwd");
    if (!g_base_z && !g_wavelength_raw) return FGS_OK;
    hipLaunchKernelGGL(k_phys_sums, dim3(1), dim3(SUM_THREADS), 0, st, dims->batch * tiles, g, partial, wavelength_raw, rg, shares,
                       g_wavelength_raw);
    FGS_LAUNCH_CHECK("k_phys_sums");
    if (g_base_z && g_phases) {
        const int64_t n = (int64_t)dims->batch * dims->points;
        hipLaunchKernelGGL(k_phys_depth, dim3((uint32_t)((n + HB - 1) / HB)), dim3(HB), 0, st, (int32_t)n, base_z, rg, shares, g_u,
                           g_base_z);
        FGS_LAUNCH_CHECK("k_phys_depth");
    }
    return FGS_OK;
}

}  // extern "C"
