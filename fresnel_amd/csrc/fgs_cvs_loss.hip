// Pixel terms of the consistency view synthesizer's losses (QualityAwareCVSLoss, ConsistencyLoss; include/fgs.h "fgs_cvs_*"): the
// depth-Laplacian quality mask, the mask-weighted L1, the EMA-consistency L1 / MSE, the depth-edge boundary term and the
// mask-weighted total-variation penalty, with the gradient to pred; and the Euler step that feeds the EMA forward.
//
//   k_cvs_mask    the quality mask of a depth plane alone
//   k_cvs_fwd     one pass over pred / target / ema (C planes each) and depth: the mask (written to `saved`), the boundary bits, and
//                 per-block double partials of the six sums (l1, consistency, boundary x / y, gradient x / y)
//   k_cvs_final   one block: the blocks' partials summed in a fixed order, scaled, the four terms written to `out`
//   k_cvs_bwd     a gather: every element of g_pred written once by the thread that owns it, from pred / target / ema, the
//                 saved mask, depth and the four upstream gradients on the device; no reduction
//   k_cvs_euler   x_prev and t_prev of the consistency loss's Euler step
//
// Memory-bound streaming kernels in the manner of fgs_pixel_loss.hip: grid-stride over groups of V consecutive pixels of one ROW
// of one image (V = 4: 16-byte accesses, when W is a multiple of 4 and every pointer is 16-byte aligned; else V = 1), the C planes
// in a loop, 256 threads, at most 2048 blocks.  The neighbours a group does not hold itself (the column to its left and right, the
// rows above and below) come from global memory through the caches.  No atomics: a thread sums its items in order, a block its
// threads in a fixed order, k_cvs_final the blocks in a fixed order, all in double -- two runs give the same bits.  The unit is
// compiled without fast-math (a NaN / Inf in pred reaches every term it enters, as in torch), without FMA contraction and with
// IEEE division: every operation on the data is rounded on its own, as include/fgs.h defines the terms.
#include <math.h>
#include <initializer_list>
#include "fgs_internal.h"

namespace {

constexpr int NT = FGS_CVS_THREADS;         // threads per block
constexpr int MAX_GRID = FGS_CVS_MAX_GRID;  // 256 CUs x 8 blocks
constexpr int K = 6;                        // sums of the forward: l1, consistency, boundary x, boundary y, gradient x, gradient y
constexpr float EDGE = 0.01f;               // the boundary term's depth step (QAL:281-282): "> 0.01" on fp32 is "> 0.01f"

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Geo {
    uint32_t images, channels, height, width, hw, npix;  // npix = images x hw; images x channels x hw < 2^31
    int flags;
    float thr, sharp;
};

struct Scale {  // k_cvs_final: out[0] = s[0] sc[0], out[1] = s[1] sc[1], out[2] = s[2] sc[2] + s[3] sc[3], out[3] = s[4] sc[4] + s[5] sc[5]
    double sc[K];
};

struct Dims {  // the entry points' leading scalars
    int32_t images, channels, height, width, flags;
    float threshold, sharpness;
};

int make_geo(const Dims &dd, Geo *g, const char *who) {
    const Dims *d = &dd;
    const int all = FGS_CVS_QUALITY | FGS_CVS_CONS_L1 | FGS_CVS_CONS_MSE | FGS_CVS_BOUNDARY | FGS_CVS_GRADIENT;
    if (d->images < 1 || d->channels < 1 || d->height < 1 || d->width < 1 || (d->flags & ~all) ||
        ((d->flags & FGS_CVS_CONS_L1) && (d->flags & FGS_CVS_CONS_MSE))) {
        fgs_set_error("%s: invalid dims (images %d, channels %d, %d x %d, flags %d): every extent >= 1; flags quality (1), consistency "
                      "L1 (2) or MSE (4) but not both, boundary (8), gradient (16)", who, d->images, d->channels, d->height, d->width,
                      d->flags);
        return FGS_EINVAL;
    }
    const uint64_t n = (uint64_t)d->images * (uint64_t)d->channels * (uint64_t)d->height * (uint64_t)d->width;
    if (n >= (1ull << 31)) { fgs_set_error("%s: batch too large (%llu elements, 2^31 at most)", who, (unsigned long long)n); return FGS_EINVAL; }
    if ((d->flags & (FGS_CVS_BOUNDARY | FGS_CVS_GRADIENT)) && (d->height < 2 || d->width < 2)) {
        fgs_set_error("%s: the boundary and gradient terms are means over the H - 1 / W - 1 interior differences: %d x %d has none",
                      who, d->height, d->width);
        return FGS_EINVAL;
    }
    if ((d->flags & FGS_CVS_QUALITY) && (!isfinite(d->threshold) || !isfinite(d->sharpness))) {
        fgs_set_error("%s: threshold / sharpness of the quality mask are not finite", who);
        return FGS_EINVAL;
    }
    g->images = (uint32_t)d->images;
    g->channels = (uint32_t)d->channels;
    g->height = (uint32_t)d->height;
    g->width = (uint32_t)d->width;
    g->hw = g->height * g->width;
    g->npix = g->images * g->hw;
    g->flags = d->flags;
    g->thr = d->threshold;
    g->sharp = d->sharpness;
    return FGS_OK;
}

// blocks of a grid-stride launch over `groups` work items
unsigned grid_for(size_t groups) {
    const size_t b = (groups + NT - 1) / NT;
    return (unsigned)(b < 1 ? 1 : b > MAX_GRID ? MAX_GRID : b);
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int vec_width(uint32_t row, std::initializer_list<const void *> ptrs) {
    if (row % 4) return 1;
    for (const void *p : ptrs)
        if (p && !aligned16(p)) return 1;
    return 4;
}

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

__device__ __forceinline__ float sgnf(float a, float b) { return (float)((a > b) - (a < b)); }

// element j + 1 / j - 1 of a group, or the scalar read beside it
template <int V>
__device__ __forceinline__ float right_of(const float (&v)[V], int j, float beside) { return j + 1 < V ? v[j + 1 < V ? j + 1 : j] : beside; }
template <int V>
__device__ __forceinline__ float left_of(const float (&v)[V], int j, float beside) { return j > 0 ? v[j > 0 ? j - 1 : 0] : beside; }

// where a work item sits: group i of V pixels -> image, row, first column, offset in the image's plane
struct Pos {
    uint32_t img, y, x, q;
};
template <int V>
__device__ __forceinline__ Pos locate(const Geo &g, uint32_t i) {
    Pos p;
    const uint32_t p0 = i * V;
    p.img = p0 / g.hw;
    p.q = p0 - p.img * g.hw;
    p.y = p.q / g.width;
    p.x = p.q - p.y * g.width;
    return p;
}

// The depth values a group needs, read once: its own pixels, the rows above and below (circular, torch.roll) and the columns to its
// left and right (circular).  The boundary bits use the same right column and lower row where those are interior.
template <int V>
struct DepthTile {
    float c[V], up[V], dn[V], left, right;
};
template <int V>
__device__ __forceinline__ DepthTile<V> depth_tile(const Geo &g, const float *__restrict__ d, const Pos &p) {
    DepthTile<V> t;
    const uint32_t ym = p.y == 0 ? g.height - 1 : p.y - 1, yp = p.y == g.height - 1 ? 0 : p.y + 1;
    const uint32_t xm = p.x == 0 ? g.width - 1 : p.x - 1, xp = p.x + V >= g.width ? 0 : p.x + V;
    ld<V>(t.c, d + p.q);
    ld<V>(t.up, d + ym * g.width + p.x);
    ld<V>(t.dn, d + yp * g.width + p.x);
    t.left = d[p.y * g.width + xm];
    t.right = d[p.y * g.width + xp];
    return t;
}

// m = sigmoid(-sharpness (|lap| - threshold)), lap = (((up + down) + left) + right) - 4 d
template <int V>
__device__ __forceinline__ void quality_mask(const Geo &g, const DepthTile<V> &t, float (&m)[V]) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float l = left_of<V>(t.c, j, t.left), r = right_of<V>(t.c, j, t.right);
        const float lap = fabsf((((t.up[j] + t.dn[j]) + l) + r) - 4.0f * t.c[j]);
        const float z = -g.sharp * (lap - g.thr);
        m[j] = 1.0f / (1.0f + expf(-z));
    }
}

// bx = |d[y, x] - d[y, x + 1]| > 0.01f for x < W - 1, by = |d[y, x] - d[y + 1, x]| > 0.01f for y < H - 1; 0 outside
template <int V>
__device__ __forceinline__ void boundary_bits(const Geo &g, const DepthTile<V> &t, const Pos &p, float (&bx)[V], float (&by)[V]) {
    const bool has_dn = p.y + 1 < g.height;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float r = right_of<V>(t.c, j, t.right);
        bx[j] = (p.x + j + 1 < g.width && fabsf(t.c[j] - r) > EDGE) ? 1.0f : 0.0f;
        by[j] = (has_dn && fabsf(t.c[j] - t.dn[j]) > EDGE) ? 1.0f : 0.0f;
    }
}

// K sums of a block in a fixed order (wave shuffles, then the wave totals in order) -> part[k * gridDim.x + blockIdx.x]
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
__global__ __launch_bounds__(NT) void k_cvs_mask(Geo g, const float *__restrict__ D, float *__restrict__ M) {
    const uint32_t groups = g.npix / V;
    for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < groups; i += gridDim.x * NT) {
        const Pos p = locate<V>(g, i);
        const DepthTile<V> t = depth_tile<V>(g, D + p.img * g.hw, p);
        float m[V];
        quality_mask<V>(g, t, m);
        st<V>(M + i * V, m);
    }
}

template <int V>
__global__ __launch_bounds__(NT) void k_cvs_fwd(Geo g, const float *__restrict__ P, const float *__restrict__ T,
                                                const float *__restrict__ D, const float *__restrict__ E, float *__restrict__ M,
                                                double *__restrict__ part) {
    const bool want_q = g.flags & FGS_CVS_QUALITY, want_bnd = g.flags & FGS_CVS_BOUNDARY, want_grad = g.flags & FGS_CVS_GRADIENT;
    const bool cons_l1 = g.flags & FGS_CVS_CONS_L1, cons_mse = g.flags & FGS_CVS_CONS_MSE;
    double acc[K] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const uint32_t groups = g.npix / V;
    for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < groups; i += gridDim.x * NT) {
        const Pos p = locate<V>(g, i);
        const bool has_dn = p.y + 1 < g.height, has_right = p.x + V < g.width;
        float m[V], bx[V], by[V];
#pragma unroll
        for (int j = 0; j < V; ++j) { m[j] = 1.0f; bx[j] = by[j] = 0.0f; }
        if (want_q || want_bnd) {
            const DepthTile<V> t = depth_tile<V>(g, D + p.img * g.hw, p);
            if (want_q) {
                quality_mask<V>(g, t, m);
                st<V>(M + i * V, m);
            }
            if (want_bnd) boundary_bits<V>(g, t, p, bx, by);
        }
        float err[V];  // sum_c |p - t|
#pragma unroll
        for (int j = 0; j < V; ++j) err[j] = 0.0f;
        const uint32_t base = p.img * g.channels * g.hw + p.q;
        for (uint32_t c = 0; c < g.channels; ++c) {
            const uint32_t o = base + c * g.hw;
            float pc[V], tc[V], ec[V], pd[V], pr = 0.0f;
            ld<V>(pc, P + o);
            ld<V>(tc, T + o);
            if (cons_l1 || cons_mse) ld<V>(ec, E + o);
            if (want_grad) {
                if (has_dn) ld<V>(pd, P + o + g.width);
                if (has_right) pr = P[o + V];
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float a = fabsf(pc[j] - tc[j]);
                acc[0] += (double)(a * m[j]);
                err[j] += a;
                if (cons_l1) acc[1] += (double)fabsf(pc[j] - ec[j]);
                if (cons_mse) {
                    const float df = pc[j] - ec[j];
                    acc[1] += (double)(df * df);
                }
                if (want_grad) {
                    if (p.x + j + 1 < g.width) acc[4] += (double)(fabsf(pc[j] - right_of<V>(pc, j, pr)) * m[j]);
                    if (has_dn) acc[5] += (double)(fabsf(pc[j] - pd[j]) * m[j]);
                }
            }
        }
        if (want_bnd) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float pe = err[j] / (float)g.channels;   // mean over the channels
                if (p.x + j + 1 < g.width) acc[2] += (double)(pe * bx[j]);   // (a product, not a branch: a NaN error reaches the term
                if (has_dn) acc[3] += (double)(pe * by[j]);                  //  through a zero bit too, as in torch)
            }
        }
    }
    block_sums(acc, part);
}

// thread t sums blocks t, t + NT, ... in order, then the threads in a fixed order
__global__ __launch_bounds__(NT) void k_cvs_final(Scale s, int flags, int nblk, const double *__restrict__ part,
                                                  float *__restrict__ out) {
    __shared__ double ws[NT / 64];
    __shared__ double tot[K];
    for (int k = 0; k < K; ++k) {
        double v = 0.0;
        for (int b = threadIdx.x; b < nblk; b += NT) v += part[(size_t)k * nblk + b];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((threadIdx.x & 63u) == 0) ws[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int w = 0; w < NT / 64; ++w) t += ws[w];
            tot[k] = t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = (float)(tot[0] * s.sc[0]);
        out[1] = (flags & (FGS_CVS_CONS_L1 | FGS_CVS_CONS_MSE)) ? (float)(tot[1] * s.sc[1]) : 0.0f;
        out[2] = (flags & FGS_CVS_BOUNDARY) ? (float)(tot[2] * s.sc[2] + tot[3] * s.sc[3]) : 0.0f;
        out[3] = (flags & FGS_CVS_GRADIENT) ? (float)(tot[4] * s.sc[4] + tot[5] * s.sc[5]) : 0.0f;
    }
}

template <int V>
__global__ __launch_bounds__(NT) void k_cvs_bwd(Geo g, Scale s, const float *__restrict__ P, const float *__restrict__ T,
                                                const float *__restrict__ D, const float *__restrict__ E,
                                                const float *__restrict__ M, const float *__restrict__ g_terms,
                                                float *__restrict__ G) {
    const bool want_q = g.flags & FGS_CVS_QUALITY, want_bnd = g.flags & FGS_CVS_BOUNDARY, want_grad = g.flags & FGS_CVS_GRADIENT;
    const bool cons_l1 = g.flags & FGS_CVS_CONS_L1, cons_mse = g.flags & FGS_CVS_CONS_MSE;
    // the upstream gradient of a term that is off is never read
    const float k0 = g_terms[0] * (float)s.sc[0];
    const float k1 = (cons_l1 || cons_mse) ? g_terms[1] * (float)s.sc[1] : 0.0f;
    const float k2x = want_bnd ? g_terms[2] * (float)(s.sc[2] / (double)g.channels) : 0.0f;
    const float k2y = want_bnd ? g_terms[2] * (float)(s.sc[3] / (double)g.channels) : 0.0f;
    const float k3x = want_grad ? g_terms[3] * (float)s.sc[4] : 0.0f, k3y = want_grad ? g_terms[3] * (float)s.sc[5] : 0.0f;
    const uint32_t groups = g.npix / V;
    for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < groups; i += gridDim.x * NT) {
        const Pos p = locate<V>(g, i);
        const bool has_dn = p.y + 1 < g.height, has_up = p.y > 0, has_right = p.x + V < g.width, has_left = p.x > 0;
        float m[V], mu[V], ml = 1.0f, bx[V], by[V];
#pragma unroll
        for (int j = 0; j < V; ++j) { m[j] = mu[j] = 1.0f; bx[j] = by[j] = 0.0f; }
        if (want_q) {
            const float *mp = M + i * V;
            ld<V>(m, mp);
            if (want_grad) {
                if (has_up) ld<V>(mu, mp - g.width);
                if (has_left) ml = mp[-1];
            }
        }
        if (want_bnd) {
            const DepthTile<V> t = depth_tile<V>(g, D + p.img * g.hw, p);
            boundary_bits<V>(g, t, p, bx, by);
        }
        float coef[V];  // of sgn(p, t)
#pragma unroll
        for (int j = 0; j < V; ++j) coef[j] = k0 * m[j] + (k2x * bx[j] + k2y * by[j]);
        const uint32_t base = p.img * g.channels * g.hw + p.q;
        for (uint32_t c = 0; c < g.channels; ++c) {
            const uint32_t o = base + c * g.hw;
            float pc[V], tc[V], ec[V], pd[V], pu[V], pr = 0.0f, pl = 0.0f, out[V];
            ld<V>(pc, P + o);
            ld<V>(tc, T + o);
            if (cons_l1 || cons_mse) ld<V>(ec, E + o);
            if (want_grad) {
                if (has_dn) ld<V>(pd, P + o + g.width);
                if (has_up) ld<V>(pu, P + o - g.width);
                if (has_right) pr = P[o + V];
                if (has_left) pl = P[o - 1];
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                float r = sgnf(pc[j], tc[j]) * coef[j];
                if (cons_l1) r += k1 * sgnf(pc[j], ec[j]);
                if (cons_mse) r += k1 * (2.0f * (pc[j] - ec[j]));
                if (want_grad) {
                    const float right = right_of<V>(pc, j, pr), left = left_of<V>(pc, j, pl);
                    const float m_left = left_of<V>(m, j, ml);
                    float tx = 0.0f, ty = 0.0f;
                    if (p.x + j + 1 < g.width) tx = m[j] * sgnf(pc[j], right);
                    if (p.x + j > 0) tx -= m_left * sgnf(left, pc[j]);
                    if (has_dn) ty = m[j] * sgnf(pc[j], pd[j]);
                    if (has_up) ty -= mu[j] * sgnf(pu[j], pc[j]);
                    r += k3x * tx + k3y * ty;
                }
                out[j] = r;
            }
            st<V>(G + o, out);
        }
    }
}

// x_prev = clamp(a' x0 + ((1 - a') / ((1 - a) + 1e-8f)) (noisy - a x0), -1, 1) (CVS:916-926); n = channels x hw elements per image
template <int V>
__global__ __launch_bounds__(NT) void k_cvs_euler(uint32_t images, uint32_t n, int32_t steps, const float *__restrict__ sac,
                                                  const long long *__restrict__ timestep, const float *__restrict__ X0,
                                                  const float *__restrict__ N, float *__restrict__ XP, float *__restrict__ TP) {
    const uint32_t groups = images * (n / V), per = n / V;
    for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < groups; i += gridDim.x * NT) {
        const uint32_t img = i / per;
        long long t = timestep[img];
        t = t < 0 ? 0 : t > (long long)(steps - 1) ? (long long)(steps - 1) : t;   // clamped into the table: memory-safe
        const long long tp = t > 0 ? t - 1 : 0;
        const float a = sac[t], ap = sac[tp];
        const float ratio = (1.0f - ap) / ((1.0f - a) + 1e-8f);
        float x0[V], nz[V], o[V];
        ld<V>(x0, X0 + i * V);
        ld<V>(nz, N + i * V);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float v = ap * x0[j] + ratio * (nz[j] - a * x0[j]);
            o[j] = v < -1.0f ? -1.0f : v > 1.0f ? 1.0f : v;   // (a NaN passes through, as torch.clamp lets it)
        }
        st<V>(XP + i * V, o);
        if (i - img * per == 0) TP[img] = (float)tp;
    }
}

Scale make_scale(const Geo &g) {
    const double B = g.images, C = g.channels, H = g.height, W = g.width;
    Scale s;
    s.sc[0] = s.sc[1] = 1.0 / (B * C * H * W);
    const bool pairs = g.height > 1 && g.width > 1;   // (the terms that use the others are refused without)
    s.sc[2] = pairs ? 1.0 / (B * H * (W - 1.0)) : 0.0;
    s.sc[3] = pairs ? 1.0 / (B * (H - 1.0) * W) : 0.0;
    s.sc[4] = pairs ? 1.0 / (B * C * H * (W - 1.0)) : 0.0;
    s.sc[5] = pairs ? 1.0 / (B * C * (H - 1.0) * W) : 0.0;
    return s;
}

size_t saved_bytes_of(const Geo &g) { return (g.flags & FGS_CVS_QUALITY) ? align256((size_t)g.npix * sizeof(float)) : 0; }
size_t scratch_bytes_of(const Geo &g) { return align256((size_t)K * grid_for(g.npix) * sizeof(double)); }

int check_inputs(const Geo &g, const float *pred, const float *target, const float *depth, const float *ema, const void *saved,
                 const char *who) {
    if (!pred || !target) { fgs_set_error("%s: null pointer (pred / target)", who); return FGS_EINVAL; }
    if ((g.flags & (FGS_CVS_QUALITY | FGS_CVS_BOUNDARY)) && !depth) {
        fgs_set_error("%s: the quality mask and the boundary term need depth", who);
        return FGS_EINVAL;
    }
    if ((g.flags & (FGS_CVS_CONS_L1 | FGS_CVS_CONS_MSE)) && !ema) {
        fgs_set_error("%s: the consistency term needs ema", who);
        return FGS_EINVAL;
    }
    if ((g.flags & FGS_CVS_QUALITY) && !saved) {
        fgs_set_error("%s: FGS_CVS_QUALITY set but saved is NULL", who);
        return FGS_EINVAL;
    }
    return FGS_OK;
}

}  // namespace

extern "C" {

int fgs_cvs_loss_workspace_bytes(int32_t images, int32_t channels, int32_t height, int32_t width, int32_t flags, size_t *saved_bytes,
                                 size_t *scratch_bytes) {
    Geo g;
    if (int rc = make_geo(Dims{images, channels, height, width, flags, 0.0f, 0.0f}, &g, "fgs_cvs_loss_workspace_bytes")) return rc;
    if (saved_bytes) *saved_bytes = saved_bytes_of(g);
    if (scratch_bytes) *scratch_bytes = scratch_bytes_of(g);
    return FGS_OK;
}

int fgs_cvs_quality_mask(int32_t images, int32_t height, int32_t width, float threshold, float sharpness, const float *depth,
                         float *mask, void *stream) {
    Geo g;
    if (int rc = make_geo(Dims{images, 1, height, width, FGS_CVS_QUALITY, threshold, sharpness}, &g, "fgs_cvs_quality_mask")) return rc;
    if (!depth || !mask) { fgs_set_error("fgs_cvs_quality_mask: null pointer"); return FGS_EINVAL; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int V = vec_width(g.width, {depth, mask});
    const unsigned grid = grid_for(g.npix / V);
    if (V == 4) hipLaunchKernelGGL(k_cvs_mask<4>, dim3(grid), dim3(NT), 0, st, g, depth, mask);
    else hipLaunchKernelGGL(k_cvs_mask<1>, dim3(grid), dim3(NT), 0, st, g, depth, mask);
    FGS_LAUNCH_CHECK("k_cvs_mask");
    return FGS_OK;
}

int fgs_cvs_loss_forward(int32_t images, int32_t channels, int32_t height, int32_t width, int32_t flags, float threshold,
                         float sharpness, const float *pred, const float *target, const float *depth, const float *ema,
                         float *out, void *saved, void *scratch, void *stream) {
    Geo g;
    if (int rc = make_geo(Dims{images, channels, height, width, flags, threshold, sharpness}, &g, "fgs_cvs_loss_forward")) return rc;
    if (int rc = check_inputs(g, pred, target, depth, ema, saved, "fgs_cvs_loss_forward")) return rc;
    if (!out || !scratch) { fgs_set_error("fgs_cvs_loss_forward: null pointer (out / scratch)"); return FGS_EINVAL; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double *part = reinterpret_cast<double *>(scratch);
    float *mask = reinterpret_cast<float *>(saved);
    const bool cons = g.flags & (FGS_CVS_CONS_L1 | FGS_CVS_CONS_MSE), dep = g.flags & (FGS_CVS_QUALITY | FGS_CVS_BOUNDARY);
    const int V = vec_width(g.width, {pred, target, dep ? depth : nullptr, cons ? ema : nullptr, (g.flags & FGS_CVS_QUALITY) ? saved : nullptr});
    const unsigned grid = grid_for(g.npix / V);
    if (V == 4) hipLaunchKernelGGL(k_cvs_fwd<4>, dim3(grid), dim3(NT), 0, st, g, pred, target, depth, ema, mask, part);
    else hipLaunchKernelGGL(k_cvs_fwd<1>, dim3(grid), dim3(NT), 0, st, g, pred, target, depth, ema, mask, part);
    FGS_LAUNCH_CHECK("k_cvs_fwd");
    hipLaunchKernelGGL(k_cvs_final, dim3(1), dim3(NT), 0, st, make_scale(g), g.flags, (int)grid, part, out);
    FGS_LAUNCH_CHECK("k_cvs_final");
    return FGS_OK;
}

int fgs_cvs_loss_backward(int32_t images, int32_t channels, int32_t height, int32_t width, int32_t flags, float threshold,
                          float sharpness, const float *pred, const float *target, const float *depth, const float *ema,
                          const void *saved, const float *g_terms, float *g_pred, void *stream) {
    Geo g;
    if (int rc = make_geo(Dims{images, channels, height, width, flags, threshold, sharpness}, &g, "fgs_cvs_loss_backward")) return rc;
    if (int rc = check_inputs(g, pred, target, depth, ema, saved, "fgs_cvs_loss_backward")) return rc;
    if (!g_terms || !g_pred) { fgs_set_error("fgs_cvs_loss_backward: null pointer (g_terms / g_pred)"); return FGS_EINVAL; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const float *mask = reinterpret_cast<const float *>(saved);
    const bool cons = g.flags & (FGS_CVS_CONS_L1 | FGS_CVS_CONS_MSE);
    const int V = vec_width(g.width, {pred, target, (g.flags & FGS_CVS_BOUNDARY) ? depth : nullptr, cons ? ema : nullptr,
                                      (g.flags & FGS_CVS_QUALITY) ? saved : nullptr, g_pred});
    const unsigned grid = grid_for(g.npix / V);
    if (V == 4) hipLaunchKernelGGL(k_cvs_bwd<4>, dim3(grid), dim3(NT), 0, st, g, make_scale(g), pred, target, depth, ema, mask, g_terms, g_pred);
    else hipLaunchKernelGGL(k_cvs_bwd<1>, dim3(grid), dim3(NT), 0, st, g, make_scale(g), pred, target, depth, ema, mask, g_terms, g_pred);
    FGS_LAUNCH_CHECK("k_cvs_bwd");
    return FGS_OK;
}

int fgs_cvs_euler_step(int32_t images, int32_t channels, int32_t hw, int32_t steps, const float *sqrt_alphas_cumprod,
                       const int64_t *timestep, const float *x0_pred, const float *noisy, float *x_prev, float *t_prev,
                       void *stream) {
    if (images < 1 || channels < 1 || hw < 1 || steps < 1) {
        fgs_set_error("fgs_cvs_euler_step: invalid dims (images %d, channels %d, hw %d, steps %d): every one >= 1", images, channels, hw, steps);
        return FGS_EINVAL;
    }
    const uint64_t total = (uint64_t)images * (uint64_t)channels * (uint64_t)hw;
    if (total >= (1ull << 31)) { fgs_set_error("fgs_cvs_euler_step: batch too large (%llu elements, 2^31 at most)", (unsigned long long)total); return FGS_EINVAL; }
    if (!sqrt_alphas_cumprod || !timestep || !x0_pred || !noisy || !x_prev || !t_prev) {
        fgs_set_error("fgs_cvs_euler_step: null pointer");
        return FGS_EINVAL;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint32_t n = (uint32_t)channels * (uint32_t)hw;
    const int V = vec_width(n, {x0_pred, noisy, x_prev});
    const unsigned grid = grid_for(total / V);
    const long long *ts = reinterpret_cast<const long long *>(timestep);
    if (V == 4) hipLaunchKernelGGL(k_cvs_euler<4>, dim3(grid), dim3(NT), 0, st, (uint32_t)images, n, steps, sqrt_alphas_cumprod, ts, x0_pred, noisy, x_prev, t_prev);
    else hipLaunchKernelGGL(k_cvs_euler<1>, dim3(grid), dim3(NT), 0, st, (uint32_t)images, n, steps, sqrt_alphas_cumprod, ts, x0_pred, noisy, x_prev, t_prev);
    FGS_LAUNCH_CHECK("k_cvs_euler");
    return FGS_OK;
}

}  // extern "C"
