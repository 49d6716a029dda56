// Fused GroupNorm -> SiLU of the consistency view synthesizer's U-Net (scripts/models/consistency_view_synthesis.py, "CVS": ResBlock,
// 90-134; AttentionBlock's norms; out_conv), with the broadcast add of the time embedding folded into the read:
//     u = x + channel_bias[b, c];  y = weight[c] (u - mean) rstd + bias[c];  out = y sigmoid(y)  |  y.
// Definition, moments' algorithm, NaN behaviour and buffer contract: include/fgs.h.  Neither u nor y is ever stored: the backward
// recomputes xhat, y and sigmoid(y) from x.
//
// The work split.  There are only `groups B` groups (128 at the workload's batch, against 256 CUs) and a group spans up to 524 288
// floats, so nothing here is "one workgroup per group".  The unit of work is a SEGMENT: up to FGS_GN_SEGMENT consecutive floats of
// ONE channel row (b, c), cut at row-relative multiples of FGS_GN_SEGMENT.  One wave owns one segment, a workgroup is four
// independent waves (no barrier, no LDS), and there are B C ceil(HW / FGS_GN_SEGMENT) of them: 8192 at (4, 128, 256, 256).  A
// segment has ONE channel: weight, bias and channel_bias are three scalars per wave, and no element needs a division to find them.
// The cuts are relative to the row, so an image's segments -- and with them every order of summation -- do not depend on the batch
// the image sits in.
//
// Addressing.  Segment s of row r starts at float r HW + s FGS_GN_SEGMENT.  With HW % 4 == 0 every segment starts on a 16-byte
// boundary (the entry points refuse base pointers that do not) and is read as float4; with any other HW (35 with 3 channels per
// group: groups start at odd offsets) rows start anywhere, and the SAME loops run in their scalar form, a lane on consecutive floats.
// A misaligned address never reaches a vector load.
//
// Forward, two launches:
//   k_gn_moments  a wave holds its segment in registers (64 floats per lane), sums it, and sums the squares of the differences from
//                 the segment's own mean (two passes over registers, with the first-order correction of the mean's rounding) -> one
//                 (mean, M2) pair of doubles per segment;
//   k_gn_apply    every wave first folds ITS GROUP's pairs (Chan's pairwise update in double: a lane over every 64th pair, then a
//                 fixed-shape tree over the lanes; cpg ceil(HW / SEGMENT) pairs, 64 or 128 at the workload's shapes), the group's
//                 first wave writes (mean, rstd) to `saved`, then the wave normalises and activates its segment.
// Backward, four launches:
//   k_gn_bwd_sums    per segment: sum g_y, sum g_y xhat, sum xhat (fp32 per lane, double across the lanes);
//   k_gn_bwd_fold    one wave per (b, group): per channel the segments' sums in order (double), the group's two means
//                    c1 = mean(weight g_y), c2 = mean(weight g_y xhat), and g_channel_bias;
//   k_gn_bwd_params  one thread per channel: g_weight, g_bias as sums over the batch, in order, in double;
//   k_gn_bwd_apply   per segment: g_x = rstd (weight g_y - c1 - xhat c2).
// No atomics anywhere, every sum has one shape: two calls agree to the bit.
#include "fgs_internal.h"

#include <math.h>
#include <type_traits>

namespace {

constexpr uint32_t SEG = FGS_GN_SEGMENT;   // floats per wave
constexpr int THREADS = 256;               // four waves, four segments
constexpr uint32_t WAVES = THREADS / 64;
constexpr int PER_LANE = SEG / 64;         // floats a lane holds in k_gn_moments
static_assert(SEG % 256 == 0 && PER_LANE == 64, "a lane of k_gn_moments holds 16 float4");

struct GnGeom {
    uint32_t B, C, HW, G, cpg, KS /* segments per row */, units /* B C KS */;
    int32_t act;
    float eps;
    double inv_m;   // 1 / (cpg HW)
};

struct Unit {
    uint32_t row, k, n, base, lane;
};

__device__ __forceinline__ bool unit_of(const GnGeom &g, Unit *u) {
    const uint32_t unit = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (unit >= g.units) return false;
    u->lane = threadIdx.x & 63u;
    u->row = unit / g.KS;
    u->k = unit - u->row * g.KS;
    u->n = min(SEG, g.HW - u->k * SEG);
    u->base = u->row * g.HW + u->k * SEG;
    return true;
}

template <class T>
__device__ __forceinline__ T wave_sum(T v) {   // xor butterfly: one shape, the same bits in every lane
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// f(offset, width): `width` consecutive floats of the segment starting `offset` floats into it; width 4 (float4, HW % 4 == 0) or 1
template <bool VEC, class F>
__device__ __forceinline__ void for_each_piece(uint32_t n, uint32_t lane, F &&f) {
    if (VEC) {
        const uint32_t slots = n >> 2;
        if (slots == SEG / 4) {   // wave-uniform: a full segment, unguarded
#pragma unroll 4
            for (uint32_t j = 0; j < SEG / 256; ++j) f(4u * (lane + 64u * j), std::integral_constant<int, 4>{});
        } else {
            for (uint32_t v = lane; v < slots; v += 64u) f(4u * v, std::integral_constant<int, 4>{});
        }
    } else {
        for (uint32_t i = lane; i < n; i += 64u) f(i, std::integral_constant<int, 1>{});
    }
}

template <int W>
__device__ __forceinline__ void load_w(const float *__restrict__ p, float (&v)[W]) {
    if constexpr (W == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[0];
    }
}
template <int W>
__device__ __forceinline__ void store_w(float *__restrict__ p, const float (&v)[W]) {
    if constexpr (W == 4) *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}

__device__ __forceinline__ float sigmoidf(float y) { return 1.0f / (1.0f + expf(-y)); }
__device__ __forceinline__ float activate(float y, int act) { return act ? y * sigmoidf(y) : y; }
// dL/dy from dL/dout: g s (1 + y (1 - s)), s = sigmoid(y)
__device__ __forceinline__ float grad_y(float y, float g, int act) {
    if (!act) return g;
    const float s = sigmoidf(y);
    return g * (s * (1.0f + y * (1.0f - s)));
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(THREADS) void k_gn_moments(GnGeom g, const float *__restrict__ x, const float *__restrict__ channel_bias,
                                                        double2 *__restrict__ partial) {
    Unit u;
    if (!unit_of(g, &u)) return;
    const float add = channel_bias ? channel_bias[u.row] : 0.0f;
    const float *__restrict__ px = x + u.base;
    float r[PER_LANE];
    float s = 0.0f;
    if (VEC) {
        const uint32_t slots = u.n >> 2;
#pragma unroll
        for (int j = 0; j < PER_LANE / 4; ++j) {
            const uint32_t v = u.lane + 64u * j;
            float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (v < slots) {
                t = *reinterpret_cast<const float4 *>(px + 4u * v);
                t.x += add; t.y += add; t.z += add; t.w += add;
            }
            r[4 * j] = t.x; r[4 * j + 1] = t.y; r[4 * j + 2] = t.z; r[4 * j + 3] = t.w;
            s += (t.x + t.y) + (t.z + t.w);
        }
    } else {
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j) {
            const uint32_t i = u.lane + 64u * j;
            r[j] = i < u.n ? px[i] + add : 0.0f;
            s += r[j];
        }
    }
    const float mu = wave_sum(s) / (float)u.n;   // the segment's mean, to fp32 rounding: a shift, not the result
    float d = 0.0f, q = 0.0f;
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j) {
        const uint32_t i = VEC ? 4u * (u.lane + 64u * (j >> 2)) : u.lane + 64u * j;   // (VEC: a slot is valid as a whole)
        const float e = i < u.n ? r[j] - mu : 0.0f;
        d += e;
        q += e * e;
    }
    const double dn = (double)u.n, ds = wave_sum((double)d), qs = wave_sum((double)q);
    if (u.lane == 0) {
        const double m2 = qs - ds * ds / dn;   // sum (u - mean)^2 about the TRUE mean mu + ds / n
        partial[blockIdx.x * WAVES + (threadIdx.x >> 6)] = make_double2((double)mu + ds / dn, m2 < 0.0 ? 0.0 : m2);
    }
}

struct Moments {
    double n, mean, m2;
};
// Chan, Golub, LeVeque: the moments of A followed by B
__device__ __forceinline__ Moments chan(const Moments &a, const Moments &b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    Moments r;
    r.n = a.n + b.n;
    const double delta = b.mean - a.mean;
    r.mean = a.mean + delta * (b.n / r.n);
    r.m2 = a.m2 + b.m2 + delta * delta * (a.n * b.n / r.n);
    return r;
}

// the moments of group (b, grp) from its cpg KS pairs, the same bits in every wave that asks
__device__ __forceinline__ void group_moments(const GnGeom &g, const double2 *__restrict__ partial, uint32_t bg, uint32_t lane,
                                              float *mean, float *rstd) {
    const uint32_t count = g.cpg * g.KS;
    const double2 *__restrict__ p = partial + (size_t)bg * count;
    Moments acc = {0.0, 0.0, 0.0};
    for (uint32_t i = lane; i < count; i += 64u) {
        const uint32_t k = i % g.KS;
        const double2 t = p[i];
        const Moments b = {(double)min(SEG, g.HW - k * SEG), t.x, t.y};
        acc = chan(acc, b);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Moments b;
        b.n = __shfl_down(acc.n, off, 64);
        b.mean = __shfl_down(acc.mean, off, 64);
        b.m2 = __shfl_down(acc.m2, off, 64);
        acc = chan(acc, b);   // (lanes >= off compute garbage nobody reads)
    }
    const double mean_d = __shfl(acc.mean, 0, 64), m2 = __shfl(acc.m2, 0, 64);
    *mean = (float)mean_d;
    *rstd = (float)(1.0 / sqrt(m2 * g.inv_m + (double)g.eps));
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void k_gn_apply(GnGeom g, const float *__restrict__ x, const float *__restrict__ channel_bias,
                                                      const float *__restrict__ weight, const float *__restrict__ bias,
                                                      const double2 *__restrict__ partial, float *__restrict__ out,
                                                      float *__restrict__ saved) {
    Unit u;
    if (!unit_of(g, &u)) return;
    const uint32_t b = u.row / g.C, c = u.row - b * g.C, grp = c / g.cpg, bg = b * g.G + grp;
    float mean, rstd;
    group_moments(g, partial, bg, u.lane, &mean, &rstd);
    if (u.k == 0 && c == grp * g.cpg && u.lane == 0) {
        saved[2 * bg] = mean;
        saved[2 * bg + 1] = rstd;
    }
    const float add = channel_bias ? channel_bias[u.row] : 0.0f, w = weight[c], bs = bias[c];
    const float *__restrict__ px = x + u.base;
    float *__restrict__ po = out + u.base;
    const int act = g.act;
    for_each_piece<VEC>(u.n, u.lane, [&](uint32_t off, auto width) {
        constexpr int W = decltype(width)::value;
        float v[W];
        load_w<W>(px + off, v);
#pragma unroll
        for (int i = 0; i < W; ++i) v[i] = activate(((v[i] + add) - mean) * rstd * w + bs, act);
        store_w<W>(po + off, v);
    });
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
struct Sums3 {
    double a, bx, xs;   // sum g_y, sum g_y xhat, sum xhat
};

template <bool VEC>
__global__ __launch_bounds__(THREADS) void k_gn_bwd_sums(GnGeom g, const float *__restrict__ x, const float *__restrict__ channel_bias,
                                                         const float *__restrict__ weight, const float *__restrict__ bias,
                                                         const float *__restrict__ saved, const float *__restrict__ g_out,
                                                         Sums3 *__restrict__ partial) {
    Unit u;
    if (!unit_of(g, &u)) return;
    const uint32_t b = u.row / g.C, c = u.row - b * g.C, bg = b * g.G + c / g.cpg;
    const float mean = saved[2 * bg], rstd = saved[2 * bg + 1];
    const float add = channel_bias ? channel_bias[u.row] : 0.0f, w = weight[c], bs = bias[c];
    const float *__restrict__ px = x + u.base;
    const float *__restrict__ pg = g_out + u.base;
    const int act = g.act;
    float a = 0.0f, bx = 0.0f, xs = 0.0f;
    for_each_piece<VEC>(u.n, u.lane, [&](uint32_t off, auto width) {
        constexpr int W = decltype(width)::value;
        float v[W], go[W];
        load_w<W>(px + off, v);
        load_w<W>(pg + off, go);
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const float xhat = ((v[i] + add) - mean) * rstd;
            const float gy = grad_y(xhat * w + bs, go[i], act);
            a += gy;
            bx += gy * xhat;
            xs += xhat;
        }
    });
    const double as = wave_sum((double)a), bxs = wave_sum((double)bx), xss = wave_sum((double)xs);
    if (u.lane == 0) partial[blockIdx.x * WAVES + (threadIdx.x >> 6)] = Sums3{as, bxs, xss};
}

// one wave per (b, group)
__global__ __launch_bounds__(THREADS) void k_gn_bwd_fold(GnGeom g, const float *__restrict__ weight, const float *__restrict__ saved,
                                                         const Sums3 *__restrict__ partial, Sums3 *__restrict__ chan_sums,
                                                         float2 *__restrict__ coef, float *__restrict__ g_channel_bias) {
    const uint32_t bg = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (bg >= g.B * g.G) return;
    const uint32_t b = bg / g.G, grp = bg - b * g.G, row0 = b * g.C + grp * g.cpg;
    double s1 = 0.0, s2 = 0.0;
    for (uint32_t cc = lane; cc < g.cpg; cc += 64u) {
        const Sums3 *__restrict__ p = partial + (size_t)(row0 + cc) * g.KS;
        Sums3 t = {0.0, 0.0, 0.0};
        for (uint32_t k = 0; k < g.KS; ++k) {
            t.a += p[k].a;
            t.bx += p[k].bx;
            t.xs += p[k].xs;
        }
        chan_sums[row0 + cc] = t;
        const double w = (double)weight[grp * g.cpg + cc];
        s1 += w * t.a;
        s2 += w * t.bx;
    }
    const double c1 = wave_sum(s1) * g.inv_m, c2 = wave_sum(s2) * g.inv_m;
    if (lane == 0) coef[bg] = make_float2((float)c1, (float)c2);
    if (g_channel_bias) {
        const double rstd = (double)saved[2 * bg + 1];
        for (uint32_t cc = lane; cc < g.cpg; cc += 64u) {   // (a lane reads back what it wrote itself)
            const Sums3 t = chan_sums[row0 + cc];
            const double w = (double)weight[grp * g.cpg + cc];
            g_channel_bias[row0 + cc] = (float)(rstd * (w * t.a - (double)g.HW * c1 - t.xs * c2));
        }
    }
}

__global__ __launch_bounds__(THREADS) void k_gn_bwd_params(GnGeom g, const Sums3 *__restrict__ chan_sums, float *__restrict__ g_weight,
                                                           float *__restrict__ g_bias) {
    const uint32_t c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= g.C) return;
    double gw = 0.0, gb = 0.0;
    for (uint32_t b = 0; b < g.B; ++b) {
        const Sums3 t = chan_sums[b * g.C + c];
        gw += t.bx;
        gb += t.a;
    }
    g_weight[c] = (float)gw;
    g_bias[c] = (float)gb;
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void k_gn_bwd_apply(GnGeom g, const float *__restrict__ x, const float *__restrict__ channel_bias,
                                                          const float *__restrict__ weight, const float *__restrict__ bias,
                                                          const float *__restrict__ saved, const float2 *__restrict__ coef,
                                                          const float *__restrict__ g_out, float *__restrict__ g_x) {
    Unit u;
    if (!unit_of(g, &u)) return;
    const uint32_t b = u.row / g.C, c = u.row - b * g.C, bg = b * g.G + c / g.cpg;
    const float mean = saved[2 * bg], rstd = saved[2 * bg + 1];
    const float2 cf = coef[bg];
    const float add = channel_bias ? channel_bias[u.row] : 0.0f, w = weight[c], bs = bias[c];
    const float *__restrict__ px = x + u.base;
    const float *__restrict__ pg = g_out + u.base;
    float *__restrict__ po = g_x + u.base;
    const int act = g.act;
    for_each_piece<VEC>(u.n, u.lane, [&](uint32_t off, auto width) {
        constexpr int W = decltype(width)::value;
        float v[W], go[W];
        load_w<W>(px + off, v);
        load_w<W>(pg + off, go);
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const float xhat = ((v[i] + add) - mean) * rstd;
            const float gy = grad_y(xhat * w + bs, go[i], act);
            v[i] = rstd * ((w * gy - cf.x) - xhat * cf.y);
        }
        store_w<W>(po + off, v);
    });
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
int geometry(int32_t batch, int32_t channels, int32_t hw, int32_t groups, GnGeom *g, const char *who) {
    if (batch < 1 || channels < 1 || hw < 1 || groups < 1 || channels % groups) {
        fgs_set_error("%s: invalid dims B=%d C=%d HW=%d groups=%d (all >= 1, groups dividing C)", who, batch, channels, hw, groups);
        return FGS_EINVAL;
    }
    if ((uint64_t)batch * (uint64_t)channels * (uint64_t)hw >= (1ull << 31)) {
        fgs_set_error("%s: B x C x HW = %d x %d x %d is beyond the supported size (2^31 elements)", who, batch, channels, hw);
        return FGS_EUNSUPPORTED;
    }
    g->B = batch; g->C = channels; g->HW = hw; g->G = groups; g->cpg = channels / groups;
    g->KS = ((uint32_t)hw + SEG - 1) / SEG;
    g->units = (uint32_t)batch * channels * g->KS;
    g->act = 1;
    g->eps = 1e-5f;
    g->inv_m = 1.0 / ((double)g->cpg * (double)hw);
    return FGS_OK;
}

int set_mode(GnGeom *g, int32_t act, float eps, const char *who) {
    if (act != 0 && act != 1) { fgs_set_error("%s: act = %d is neither 0 (none) nor 1 (SiLU)", who, act); return FGS_EINVAL; }
    if (!isfinite(eps) || !(eps > 0.0f)) { fgs_set_error("%s: eps = %g is not a finite positive number", who, (double)eps); return FGS_EINVAL; }
    g->act = act;
    g->eps = eps;
    return FGS_OK;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

size_t round256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
size_t saved_size(const GnGeom &g) { return round256((size_t)g.B * g.G * 2 * sizeof(float)); }
size_t unit_sums_size(const GnGeom &g) { return round256((size_t)g.units * sizeof(Sums3)); }   // (>= the forward's double2 per segment)
size_t chan_sums_size(const GnGeom &g) { return round256((size_t)g.B * g.C * sizeof(Sums3)); }
size_t coef_size(const GnGeom &g) { return round256((size_t)g.B * g.G * sizeof(float2)); }
uint32_t unit_blocks(const GnGeom &g) { return (g.units + WAVES - 1) / WAVES; }

#define GN_DISPATCH(kernel, ...)                                                                                    \
    do {                                                                                                            \
        if (g.HW % 4 == 0) hipLaunchKernelGGL(kernel<true>, dim3(unit_blocks(g)), dim3(THREADS), 0, st, __VA_ARGS__);  \
        else hipLaunchKernelGGL(kernel<false>, dim3(unit_blocks(g)), dim3(THREADS), 0, st, __VA_ARGS__);               \
    } while (0)

}  // namespace

extern "C" {

int fgs_gn_silu_workspace_bytes(int32_t batch, int32_t channels, int32_t hw, int32_t groups, size_t *saved_bytes, size_t *scratch_bytes) {
    GnGeom g;
    int rc = geometry(batch, channels, hw, groups, &g, "fgs_gn_silu_workspace_bytes");
    if (rc) return rc;
    if (!saved_bytes || !scratch_bytes) { fgs_set_error("fgs_gn_silu_workspace_bytes: null output pointer"); return FGS_EINVAL; }
    *saved_bytes = saved_size(g);
    *scratch_bytes = unit_sums_size(g) + chan_sums_size(g) + coef_size(g);
    return FGS_OK;
}

int fgs_gn_silu_forward(int32_t batch, int32_t channels, int32_t hw, int32_t groups, int32_t act, float eps, const float *x,
                        const float *channel_bias, const float *weight, const float *bias, float *out, void *saved, void *scratch,
                        void *stream) {
    GnGeom g;
    int rc = geometry(batch, channels, hw, groups, &g, "fgs_gn_silu_forward");
    if (rc) return rc;
    if ((rc = set_mode(&g, act, eps, "fgs_gn_silu_forward"))) return rc;
    if (!x || !weight || !bias || !out || !saved || !scratch) {
        fgs_set_error("fgs_gn_silu_forward: null pointer argument (only channel_bias may be NULL)");
        return FGS_EINVAL;
    }
    if (!aligned16(x) || !aligned16(out) || !aligned16(scratch)) {
        fgs_set_error("fgs_gn_silu_forward: x, out and scratch must be 16-byte aligned");
        return FGS_EINVAL;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double2 *partial = reinterpret_cast<double2 *>(scratch);
    GN_DISPATCH(k_gn_moments, g, x, channel_bias, partial);
    FGS_LAUNCH_CHECK("k_gn_moments");
    GN_DISPATCH(k_gn_apply, g, x, channel_bias, weight, bias, (const double2 *)partial, out, reinterpret_cast<float *>(saved));
    FGS_LAUNCH_CHECK("k_gn_apply");
    return FGS_OK;
}

int fgs_gn_silu_backward(int32_t batch, int32_t channels, int32_t hw, int32_t groups, int32_t act, float eps, const float *x,
                         const float *channel_bias, const float *weight, const float *bias, const void *saved, const float *g_out,
                         float *g_x, float *g_channel_bias, float *g_weight, float *g_bias, void *scratch, void *stream) {
    GnGeom g;
    int rc = geometry(batch, channels, hw, groups, &g, "fgs_gn_silu_backward");
    if (rc) return rc;
    if ((rc = set_mode(&g, act, eps, "fgs_gn_silu_backward"))) return rc;
    if (!x || !weight || !bias || !saved || !g_out || !g_x || !g_weight || !g_bias || !scratch) {
        fgs_set_error("fgs_gn_silu_backward: null pointer argument (only channel_bias and g_channel_bias may be NULL)");
        return FGS_EINVAL;
    }
    if (!aligned16(x) || !aligned16(g_out) || !aligned16(g_x) || !aligned16(scratch)) {
        fgs_set_error("fgs_gn_silu_backward: x, g_out, g_x and scratch must be 16-byte aligned");
        return FGS_EINVAL;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const float *sv = reinterpret_cast<const float *>(saved);
    char *base = reinterpret_cast<char *>(scratch);
    Sums3 *unit_sums = reinterpret_cast<Sums3 *>(base);
    Sums3 *chan_sums = reinterpret_cast<Sums3 *>(base + unit_sums_size(g));
    float2 *coef = reinterpret_cast<float2 *>(base + unit_sums_size(g) + chan_sums_size(g));
    GN_DISPATCH(k_gn_bwd_sums, g, x, channel_bias, weight, bias, sv, g_out, unit_sums);
    FGS_LAUNCH_CHECK("k_gn_bwd_sums");
    hipLaunchKernelGGL(k_gn_bwd_fold, dim3((g.B * g.G + WAVES - 1) / WAVES), dim3(THREADS), 0, st, g, weight, sv,
                       (const Sums3 *)unit_sums, chan_sums, coef, g_channel_bias);
    FGS_LAUNCH_CHECK("k_gn_bwd_fold");
    hipLaunchKernelGGL(k_gn_bwd_params, dim3((g.C + THREADS - 1) / THREADS), dim3(THREADS), 0, st, g, (const Sums3 *)chan_sums, g_weight,
                       g_bias);
    FGS_LAUNCH_CHECK("k_gn_bwd_params");
    GN_DISPATCH(k_gn_bwd_apply, g, x, channel_bias, weight, bias, sv, (const float2 *)coef, g_out, g_x);
    FGS_LAUNCH_CHECK("k_gn_bwd_apply");
    return FGS_OK;
}

}  // extern "C"
