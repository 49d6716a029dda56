// Per-pixel block of the training loss (TGD:873-953; include/fgs.h "fgs_pixel_loss_*"): density-weighted L1, the
// Fresnel-zone boundary emphasis term and the normalised-depth L1, with their gradients.
//
//   k_pixel_stage1   one pass over rendered / target (3 planes each), density, target_depth, rendered_depth: per-block
//                    double partials of  sum w |r - t|,  sum mask sum_c |r - t|,  sum x,  sum y
//   k_pixel_stage2   the two depth maps again: sum (x - mean_x)^2, sum (y - mean_y)^2
//   k_pixel_stage3   the two depth maps again: sum |u - v|, sum sgn(u - v), sum sgn(u - v) u
//   k_pixel_final    one block after each of them: the blocks' partials summed in a fixed order into the named `stats`
//                    slots, and the terms that are complete written to `out`
//   k_pixel_bwd      pointwise: g_rendered and g_rendered_depth from the inputs and `stats`; no reduction
//
// Memory-bound streaming kernels: grid-stride over groups of V consecutive pixels of one image (V = 4: 16-byte loads, when
// H x W is a multiple of 4 and every pointer is 16-byte aligned; else V = 1), 256 threads, at most 2048 blocks.  No atomics:
// a thread sums its pixels in order, a block its threads in a fixed order, k_pixel_final the blocks in a fixed order, all
// in double -- two runs give the same bits.  The unit is compiled without fast-math (NaN / Inf must reach the sums: the
// step's NaN/Inf skip reads them) and without FMA contraction (stage 3 and the backward must form u and v identically:
// the backward's sgn(u - v) has to be the one that was summed).
#include <math.h>
#include <initializer_list>
#include "fgs_internal.h"

namespace {

constexpr int NT = 256;           // threads per block
constexpr int MAX_GRID = 2048;    // 256 CUs x 8 blocks
constexpr int MAXB = FGS_PIXEL_MAX_BOUNDARIES;
constexpr int MAXK = 4;           // sums per stage

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Geo {
    uint32_t images, hw, npix;    // npix = images x hw (3 npix < 2^31)
    double n_global;              // npix x world
    int flags;
    float vlm_weight;
};

struct Table {                    // zone boundaries: kernel argument, read with uniform indices
    float b[MAXB];
    int n, hard;
    float thr, sharp;
};

struct Final {                    // what k_pixel_final does with sum k: stats[slot[k]] = sum; out[out_idx[k]] = sum x scale[k]
    int K, slot[MAXK], out_idx[MAXK];
    double scale[MAXK];
    int zero_out;                 // an output index to clear, or -1
};

int make_geo(const FgsPixelLossDims *d, Geo *g, Table *tb, const char *who) {
    if (!d) { fgs_set_error("%s: null dims", who); return FGS_EINVAL; }
    const int terms = FGS_PIXEL_RGB | FGS_PIXEL_BOUNDARY | FGS_PIXEL_DEPTH;
    if (d->images < 1 || d->height < 1 || d->width < 1 || d->world < 1 || (d->flags & ~31) || !(d->flags & terms) ||
        ((d->flags & FGS_PIXEL_DENSITY) && !(d->flags & FGS_PIXEL_RGB))) {
        fgs_set_error("%s: invalid dims (images %d, %d x %d, world %d, flags %d): at least one of the terms rgb (1), boundary (4), "
                      "depth (16); density weighting (2) goes with rgb", who, d->images, d->height, d->width, d->world, d->flags);
        return FGS_EINVAL;
    }
    const uint64_t npix = (uint64_t)d->images * (uint64_t)d->height * (uint64_t)d->width;
    if (3 * npix >= (1ull << 31)) { fgs_set_error("%s: batch too large (%llu pixels)", who, (unsigned long long)npix); return FGS_EINVAL; }
    if (npix * (uint64_t)d->world < 2) {
        fgs_set_error("%s: images x H x W x world = %llu: the unbiased std needs at least 2 values", who,
                      (unsigned long long)(npix * (uint64_t)d->world));
        return FGS_EINVAL;
    }
    if ((d->flags & FGS_PIXEL_DENSITY) && !isfinite(d->vlm_weight)) {
        fgs_set_error("%s: vlm_weight is not finite", who);
        return FGS_EINVAL;
    }
    tb->n = 0;
    tb->hard = (d->flags & FGS_PIXEL_HARD_MASK) ? 1 : 0;
    tb->thr = tb->sharp = 0.0f;
    for (int k = 0; k < MAXB; ++k) tb->b[k] = 0.0f;
    if (d->flags & FGS_PIXEL_BOUNDARY) {
        if (d->num_boundaries < 1 || d->num_boundaries > MAXB) {
            fgs_set_error("%s: %d zone boundaries: 1 ... %d", who, d->num_boundaries, MAXB);
            return FGS_EINVAL;
        }
        if (!(d->threshold > 0.0f) || !isfinite(d->threshold)) {
            fgs_set_error("%s: boundary threshold %g must be positive", who, (double)d->threshold);
            return FGS_EINVAL;
        }
        for (int k = 0; k < d->num_boundaries; ++k) {
            if (!isfinite(d->boundaries[k]) || (k && !(d->boundaries[k] > d->boundaries[k - 1]))) {
                fgs_set_error("%s: zone boundaries must be finite and strictly increasing (entry %d)", who, k);
                return FGS_EINVAL;
            }
            tb->b[k] = d->boundaries[k];
        }
        tb->n = d->num_boundaries;
        tb->thr = d->threshold;
        tb->sharp = (float)(10.0 / (double)d->threshold);  // (the reference forms 10 / threshold in double, then multiplies in fp32)
    }
    g->images = (uint32_t)d->images;
    g->hw = (uint32_t)d->height * (uint32_t)d->width;
    g->npix = (uint32_t)npix;
    g->n_global = (double)npix * (double)d->world;
    g->flags = d->flags;
    g->vlm_weight = d->vlm_weight;
    return FGS_OK;
}

// blocks of a grid-stride launch over `groups` work items
unsigned grid_for(size_t groups) {
    const size_t b = (groups + NT - 1) / NT;
    return (unsigned)(b < 1 ? 1 : b > MAX_GRID ? MAX_GRID : b);
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <int V>
__device__ __forceinline__ void ld(float (&o)[V], const float *__restrict__ p) {
    if constexpr (V == 4) {
        const float4 x = *reinterpret_cast<const float4 *>(p);
        o[0] = x.x; o[1] = x.y; o[2] = x.z; o[3] = x.w;
    } else {
        o[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void st(float *__restrict__ p, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}

// FresnelZones.compute_boundary_mask in fp32: distance to the nearest boundary, soft (sigmoid) or hard
__device__ __forceinline__ float zone_mask(float d, const Table &tb) {
    float md = fabsf(d - tb.b[0]);
    for (int k = 1; k < tb.n; ++k) {
        const float x = fabsf(d - tb.b[k]);
        md = x < md ? x : md;
    }
    if (tb.hard) return md < tb.thr ? 1.0f : 0.0f;
    return 1.0f / (1.0f + expf(-(tb.sharp * (tb.thr - md))));
}

__device__ __forceinline__ float sgnf(float a, float b) { return (float)((a > b) - (a < b)); }

// The depth normalisation, from the (cross-rank summed) statistics.  Stage 3 and the backward take u and v from here.
struct DepthNorm {
    double mx, my, isx, isy, gate;
    __device__ __forceinline__ double u(float x) const { return ((double)x - mx) * isx; }
    __device__ __forceinline__ double v(float y) const { return ((double)y - my) * isy; }
};
__device__ __forceinline__ DepthNorm depth_norm(const double *__restrict__ stats, double n) {
    DepthNorm d;
    d.mx = stats[FGS_PIXEL_STAT_SUM_X] / n;
    d.my = stats[FGS_PIXEL_STAT_SUM_Y] / n;
    const double sx = sqrt(stats[FGS_PIXEL_STAT_SSD_X] / (n - 1.0)), sy = sqrt(stats[FGS_PIXEL_STAT_SSD_Y] / (n - 1.0));
    d.gate = sx >= 1e-4 ? 1.0 : 0.0;          // torch.clamp(std, min=1e-4): no gradient through a clamped std
    d.isx = 1.0 / (sx < 1e-4 ? 1e-4 : sx);    // (a NaN std stays NaN)
    d.isy = 1.0 / (sy < 1e-4 ? 1e-4 : sy);
    return d;
}

// K sums of a block in a fixed order (wave shuffles, then the wave totals in order) -> part[k * gridDim.x + blockIdx.x]
template <int K>
__device__ __forceinline__ void block_sums(double (&v)[K], double *__restrict__ part) {
    __shared__ double ws[K][NT / 64];
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
        if ((threadIdx.x & 63u) == 0) ws[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double t = 0.0;
        for (int w = 0; w < NT / 64; ++w) t += ws[threadIdx.x][w];
        part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
    }
}

template <int V>
__global__ __launch_bounds__(NT) void k_pixel_stage1(Geo g, Table tb, const float *__restrict__ R, const float *__restrict__ T,
                                                     const float *__restrict__ X, const float *__restrict__ Y,
                                                     const float *__restrict__ D, double *__restrict__ part) {
    const bool want_rgb = g.flags & FGS_PIXEL_RGB, want_bnd = g.flags & FGS_PIXEL_BOUNDARY;
    const bool want_den = g.flags & FGS_PIXEL_DENSITY, want_dep = g.flags & FGS_PIXEL_DEPTH;
    const float w0 = 1.0f - g.vlm_weight;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};  // rgb, boundary, sum x, sum y
    const uint32_t groups = g.npix / V;
    for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < groups; i += gridDim.x * NT) {
        const uint32_t p = i * V, img = p / g.hw, q = p - img * g.hw;
        const uint32_t base = img * 3u * g.hw + q;
        float r[3][V], t[3][V], den[V], x[V], y[V];
        if (want_rgb || want_bnd) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ld<V>(r[c], R + base + c * g.hw);
                ld<V>(t[c], T + base + c * g.hw);
            }
        }
        if (want_den) ld<V>(den, D + p);
        if (want_bnd || want_dep) ld<V>(y, Y + p);
        if (want_dep) ld<V>(x, X + p);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (want_rgb || want_bnd) {
                const float a = (fabsf(r[0][j] - t[0][j]) + fabsf(r[1][j] - t[1][j])) + fabsf(r[2][j] - t[2][j]);
                if (want_rgb) acc[0] += (double)(want_den ? a * (w0 + g.vlm_weight * den[j]) : a);
                if (want_bnd) acc[1] += (double)(a * zone_mask(y[j], tb));
            }
            if (want_dep) {
                acc[2] += (double)x[j];
                acc[3] += (double)y[j];
            }
        }
    }
    block_sums<4>(acc, part);
}

template <int V>
__global__ __launch_bounds__(NT) void k_pixel_stage2(uint32_t npix, double n, const double *__restrict__ stats,
                                                     const float *__restrict__ X, const float *__restrict__ Y,
                                                     double *__restrict__ part) {
    const double mx = stats[FGS_PIXEL_STAT_SUM_X] / n, my = stats[FGS_PIXEL_STAT_SUM_Y] / n;
    double acc[2] = {0.0, 0.0};
    const uint32_t groups = npix / V;
    for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < groups; i += gridDim.x * NT) {
        float x[V], y[V];
        ld<V>(x, X + i * V);
        ld<V>(y, Y + i * V);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const double dx = (double)x[j] - mx, dy = (double)y[j] - my;
            acc[0] += dx * dx;
            acc[1] += dy * dy;
        }
    }
    block_sums<2>(acc, part);
}

template <int V>
__global__ __launch_bounds__(NT) void k_pixel_stage3(uint32_t npix, double n, const double *__restrict__ stats,
                                                     const float *__restrict__ X, const float *__restrict__ Y,
                                                     double *__restrict__ part) {
    const DepthNorm dn = depth_norm(stats, n);
    double acc[3] = {0.0, 0.0, 0.0};  // sum |u - v|, sum sgn, sum sgn u
    const uint32_t groups = npix / V;
    for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < groups; i += gridDim.x * NT) {
        float x[V], y[V];
        ld<V>(x, X + i * V);
        ld<V>(y, Y + i * V);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const double u = dn.u(x[j]), v = dn.v(y[j]);
            const double s = (double)((u > v) - (u < v));
            acc[0] += fabs(u - v);
            acc[1] += s;
            acc[2] += s * u;
        }
    }
    block_sums<3>(acc, part);
}

// thread t sums blocks t, t + NT, ... in order, then the threads in a fixed order
__global__ __launch_bounds__(NT) void k_pixel_final(Final f, int nblk, const double *__restrict__ part,
                                                    double *__restrict__ stats, float *__restrict__ out) {
    __shared__ double ws[NT / 64];
    for (int k = 0; k < f.K; ++k) {
        double v = 0.0;
        for (int b = threadIdx.x; b < nblk; b += NT) v += part[(size_t)k * nblk + b];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((threadIdx.x & 63u) == 0) ws[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int w = 0; w < NT / 64; ++w) t += ws[w];
            stats[f.slot[k]] = t;
            if (f.out_idx[k] >= 0) out[f.out_idx[k]] = (float)(t * f.scale[k]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && f.zero_out >= 0) out[f.zero_out] = 0.0f;
}

template <int V>
__global__ __launch_bounds__(NT) void k_pixel_bwd(Geo g, Table tb, const float *__restrict__ R, const float *__restrict__ T,
                                                  const float *__restrict__ X, const float *__restrict__ Y,
                                                  const float *__restrict__ D, const double *__restrict__ stats,
                                                  const float *__restrict__ g_rgb, const float *__restrict__ g_bnd,
                                                  const float *__restrict__ g_dep, float *__restrict__ GR,
                                                  float *__restrict__ GX) {
    const bool want_rgb = (g.flags & FGS_PIXEL_RGB) && g_rgb, want_bnd = (g.flags & FGS_PIXEL_BOUNDARY) && g_bnd;
    const bool want_den = g.flags & FGS_PIXEL_DENSITY, want_dep = GX != nullptr;
    const float inv_cnt = (float)(1.0 / (3.0 * (double)g.npix));
    const float gr = want_rgb ? *g_rgb * inv_cnt : 0.0f, gb = want_bnd ? *g_bnd * inv_cnt : 0.0f;
    const float w0 = 1.0f - g.vlm_weight;
    DepthNorm dn = {};
    double gd = 0.0, c0 = 0.0, c1 = 0.0;
    const double inv_local = 1.0 / (double)g.npix;
    if (want_dep) {
        dn = depth_norm(stats, g.n_global);
        gd = g_dep ? (double)*g_dep * dn.isx : 0.0;
        c0 = stats[FGS_PIXEL_STAT_SGN] * inv_local / g.n_global;                          // Q / N
        c1 = dn.gate * stats[FGS_PIXEL_STAT_SGN_U] * inv_local / (g.n_global - 1.0);      // gate P / (N - 1)
    }
    const uint32_t groups = g.npix / V;
    for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < groups; i += gridDim.x * NT) {
        const uint32_t p = i * V, img = p / g.hw, q = p - img * g.hw;
        const uint32_t base = img * 3u * g.hw + q;
        float r[3][V], t[3][V], den[V], x[V], y[V];
        if (GR) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ld<V>(r[c], R + base + c * g.hw);
                ld<V>(t[c], T + base + c * g.hw);
            }
            if (want_rgb && want_den) ld<V>(den, D + p);
        }
        if ((GR && want_bnd) || want_dep) ld<V>(y, Y + p);
        if (want_dep) ld<V>(x, X + p);
        if (GR) {
            float coef[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                coef[j] = want_rgb ? (want_den ? gr * (w0 + g.vlm_weight * den[j]) : gr) : 0.0f;
                if (want_bnd) coef[j] += gb * zone_mask(y[j], tb);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float o[V];
#pragma unroll
                for (int j = 0; j < V; ++j) o[j] = sgnf(r[c][j], t[c][j]) * coef[j];
                st<V>(GR + base + c * g.hw, o);
            }
        }
        if (want_dep) {
            float o[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const double u = dn.u(x[j]), v = dn.v(y[j]);
                const double s = (double)((u > v) - (u < v));
                o[j] = (float)(gd * (s * inv_local - c0 - c1 * u));
            }
            st<V>(GX + p, o);
        }
    }
}

int vec_width(const Geo &g, std::initializer_list<const void *> ptrs) {
    if (g.hw % 4) return 1;
    for (const void *p : ptrs)
        if (p && !aligned16(p)) return 1;
    return 4;
}

size_t scratch_bytes_of(const Geo &g) { return align256((size_t)MAXK * grid_for(g.npix) * sizeof(double)); }

int launch_final(const Final &f, int nblk, const double *part, double *stats, float *out, hipStream_t st) {
    hipLaunchKernelGGL(k_pixel_final, dim3(1), dim3(NT), 0, st, f, nblk, part, stats, out);
    FGS_LAUNCH_CHECK("k_pixel_final");
    return FGS_OK;
}

int check_depth_stage(const Geo &g, const float *x, const float *y, const void *stats, const void *scratch, const char *who) {
    if (!(g.flags & FGS_PIXEL_DEPTH)) {
        fgs_set_error("%s: flags %d carry no depth term (FGS_PIXEL_DEPTH)", who, g.flags);
        return FGS_EINVAL;
    }
    if (!x || !y || !stats || !scratch) {
        fgs_set_error("%s: null pointer", who);
        return FGS_EINVAL;
    }
    return FGS_OK;
}

int check_inputs(const Geo &g, const float *r, const float *t, const float *x, const float *y, const float *den, const char *who) {
    if ((g.flags & (FGS_PIXEL_RGB | FGS_PIXEL_BOUNDARY)) && (!r || !t)) {
        fgs_set_error("%s: the rgb / boundary term needs rendered and target", who);
        return FGS_EINVAL;
    }
    if ((g.flags & FGS_PIXEL_DENSITY) && !den) {
        fgs_set_error("%s: FGS_PIXEL_DENSITY set but density is NULL", who);
        return FGS_EINVAL;
    }
    if ((g.flags & FGS_PIXEL_BOUNDARY) && !y) {
        fgs_set_error("%s: FGS_PIXEL_BOUNDARY set but target_depth is NULL", who);
        return FGS_EINVAL;
    }
    if ((g.flags & FGS_PIXEL_DEPTH) && (!x || !y)) {
        fgs_set_error("%s: FGS_PIXEL_DEPTH set but rendered_depth / target_depth is NULL", who);
        return FGS_EINVAL;
    }
    return FGS_OK;
}

}  // namespace

extern "C" {

int fgs_pixel_loss_workspace_bytes(const FgsPixelLossDims *dims, size_t *stats_bytes, size_t *scratch_bytes) {
    Geo g;
    Table tb;
    if (int rc = make_geo(dims, &g, &tb, "fgs_pixel_loss_workspace_bytes")) return rc;
    if (stats_bytes) *stats_bytes = align256(FGS_PIXEL_STAT_SLOTS * sizeof(double));
    if (scratch_bytes) *scratch_bytes = scratch_bytes_of(g);
    return FGS_OK;
}

int fgs_pixel_loss_stage1(const FgsPixelLossDims *dims, const float *rendered, const float *target,
                          const float *rendered_depth, const float *target_depth, const float *density, float *out,
                          void *stats, void *scratch, void *stream) {
    Geo g;
    Table tb;
    if (int rc = make_geo(dims, &g, &tb, "fgs_pixel_loss_stage1")) return rc;
    if (int rc = check_inputs(g, rendered, target, rendered_depth, target_depth, density, "fgs_pixel_loss_stage1")) return rc;
    if (!out || !stats || !scratch) {
        fgs_set_error("fgs_pixel_loss_stage1: null pointer (out / stats / scratch)");
        return FGS_EINVAL;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double *part = reinterpret_cast<double *>(scratch);
    const int V = vec_width(g, {rendered, target, rendered_depth, target_depth, density});
    const unsigned grid = grid_for(g.npix / V);
    if (V == 4)
        hipLaunchKernelGGL(k_pixel_stage1<4>, dim3(grid), dim3(NT), 0, st, g, tb, rendered, target, rendered_depth, target_depth,
                           density, part);
    else
        hipLaunchKernelGGL(k_pixel_stage1<1>, dim3(grid), dim3(NT), 0, st, g, tb, rendered, target, rendered_depth, target_depth,
                           density, part);
    FGS_LAUNCH_CHECK("k_pixel_stage1");
    Final f = {};
    f.K = 4;
    const int slots[4] = {FGS_PIXEL_STAT_RGB, FGS_PIXEL_STAT_BOUNDARY, FGS_PIXEL_STAT_SUM_X, FGS_PIXEL_STAT_SUM_Y};
    const double inv = 1.0 / (3.0 * (double)g.npix);  // boundary: mean over pixels of (sum_c / 3)
    for (int k = 0; k < 4; ++k) {
        f.slot[k] = slots[k];
        f.out_idx[k] = k < 2 ? k : -1;
        f.scale[k] = inv;
    }
    f.zero_out = 2;
    return launch_final(f, (int)grid, part, reinterpret_cast<double *>(stats), out, st);
}

int fgs_pixel_loss_stage2(const FgsPixelLossDims *dims, const float *rendered_depth, const float *target_depth,
                          void *stats, void *scratch, void *stream) {
    Geo g;
    Table tb;
    if (int rc = make_geo(dims, &g, &tb, "fgs_pixel_loss_stage2")) return rc;
    if (int rc = check_depth_stage(g, rendered_depth, target_depth, stats, scratch, "fgs_pixel_loss_stage2")) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double *part = reinterpret_cast<double *>(scratch), *sd = reinterpret_cast<double *>(stats);
    const int V = (g.npix % 4 == 0 && aligned16(rendered_depth) && aligned16(target_depth)) ? 4 : 1;
    const unsigned grid = grid_for(g.npix / V);
    if (V == 4)
        hipLaunchKernelGGL(k_pixel_stage2<4>, dim3(grid), dim3(NT), 0, st, g.npix, g.n_global, sd, rendered_depth, target_depth, part);
    else
        hipLaunchKernelGGL(k_pixel_stage2<1>, dim3(grid), dim3(NT), 0, st, g.npix, g.n_global, sd, rendered_depth, target_depth, part);
    FGS_LAUNCH_CHECK("k_pixel_stage2");
    Final f = {};
    f.K = 2;
    f.slot[0] = FGS_PIXEL_STAT_SSD_X;
    f.slot[1] = FGS_PIXEL_STAT_SSD_Y;
    f.out_idx[0] = f.out_idx[1] = -1;
    f.zero_out = -1;
    return launch_final(f, (int)grid, part, sd, nullptr, st);
}

int fgs_pixel_loss_stage3(const FgsPixelLossDims *dims, const float *rendered_depth, const float *target_depth, float *out,
                          void *stats, void *scratch, void *stream) {
    Geo g;
    Table tb;
    if (int rc = make_geo(dims, &g, &tb, "fgs_pixel_loss_stage3")) return rc;
    if (int rc = check_depth_stage(g, rendered_depth, target_depth, stats, scratch, "fgs_pixel_loss_stage3")) return rc;
    if (!out) { fgs_set_error("fgs_pixel_loss_stage3: null pointer (out)"); return FGS_EINVAL; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double *part = reinterpret_cast<double *>(scratch), *sd = reinterpret_cast<double *>(stats);
    const int V = (g.npix % 4 == 0 && aligned16(rendered_depth) && aligned16(target_depth)) ? 4 : 1;
    const unsigned grid = grid_for(g.npix / V);
    if (V == 4)
        hipLaunchKernelGGL(k_pixel_stage3<4>, dim3(grid), dim3(NT), 0, st, g.npix, g.n_global, sd, rendered_depth, target_depth, part);
    else
        hipLaunchKernelGGL(k_pixel_stage3<1>, dim3(grid), dim3(NT), 0, st, g.npix, g.n_global, sd, rendered_depth, target_depth, part);
    FGS_LAUNCH_CHECK("k_pixel_stage3");
    Final f = {};
    f.K = 3;
    f.slot[0] = FGS_PIXEL_STAT_DEPTH;
    f.slot[1] = FGS_PIXEL_STAT_SGN;
    f.slot[2] = FGS_PIXEL_STAT_SGN_U;
    f.out_idx[0] = 2;
    f.out_idx[1] = f.out_idx[2] = -1;
    f.scale[0] = 1.0 / (double)g.npix;
    f.zero_out = -1;
    return launch_final(f, (int)grid, part, sd, out, st);
}

int fgs_pixel_loss_forward(const FgsPixelLossDims *dims, const float *rendered, const float *target,
                           const float *rendered_depth, const float *target_depth, const float *density, float *out,
                           void *stats, void *scratch, void *stream) {
    if (int rc = fgs_pixel_loss_stage1(dims, rendered, target, rendered_depth, target_depth, density, out, stats, scratch, stream))
        return rc;
    if (!(dims->flags & FGS_PIXEL_DEPTH)) return FGS_OK;
    if (int rc = fgs_pixel_loss_stage2(dims, rendered_depth, target_depth, stats, scratch, stream)) return rc;
    return fgs_pixel_loss_stage3(dims, rendered_depth, target_depth, out, stats, scratch, stream);
}

int fgs_pixel_loss_backward(const FgsPixelLossDims *dims, const float *rendered, const float *target,
                            const float *rendered_depth, const float *target_depth, const float *density,
                            const void *stats, const float *g_rgb, const float *g_boundary, const float *g_depth,
                            float *g_rendered, float *g_rendered_depth, void *stream) {
    Geo g;
    Table tb;
    if (int rc = make_geo(dims, &g, &tb, "fgs_pixel_loss_backward")) return rc;
    if (int rc = check_inputs(g, rendered, target, rendered_depth, target_depth, density, "fgs_pixel_loss_backward")) return rc;
    if (!stats || (!g_rendered && !g_rendered_depth)) {
        fgs_set_error("fgs_pixel_loss_backward: null pointer (stats, or both gradients)");
        return FGS_EINVAL;
    }
    if ((g_rendered && !(g.flags & (FGS_PIXEL_RGB | FGS_PIXEL_BOUNDARY))) || (g_rendered_depth && !(g.flags & FGS_PIXEL_DEPTH))) {
        fgs_set_error("fgs_pixel_loss_backward: a gradient was requested for a term the flags (%d) do not carry", g.flags);
        return FGS_EINVAL;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const double *sd = reinterpret_cast<const double *>(stats);
    const int V = vec_width(g, {rendered, target, rendered_depth, target_depth, density, g_rendered, g_rendered_depth});
    const unsigned grid = grid_for(g.npix / V);
    if (V == 4)
        hipLaunchKernelGGL(k_pixel_bwd<4>, dim3(grid), dim3(NT), 0, st, g, tb, rendered, target, rendered_depth, target_depth, density,
                           sd, g_rgb, g_boundary, g_depth, g_rendered, g_rendered_depth);
    else
        hipLaunchKernelGGL(k_pixel_bwd<1>, dim3(grid), dim3(NT), 0, st, g, tb, rendered, target, rendered_depth, target_depth, density,
                           sd, g_rgb, g_boundary, g_depth, g_rendered, g_rendered_depth);
    FGS_LAUNCH_CHECK("k_pixel_bwd");
    return FGS_OK;
}

}  // extern "C"
