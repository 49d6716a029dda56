// SAAG surface-aligned Gaussian clouds from depth (include/fgs.h, "SAAG surface-aligned Gaussian clouds"): the reference's
// PointCloud::from_depth + center + normalize + to_surface_gaussians (src/core/pointcloud.cpp, PC below) with
// DepthMap::compute_surface_info (src/core/image.cpp:157-225, IM below) as a count -> scan -> scatter compaction.
//
//   k_surface_range    (RB, B) blocks   per-block min / max of the image's depth                       -> part1
//   k_surface_points   (PB, B) blocks   one point per thread: raw position, kept?, Sobel magnitude;
//                                       per-block bounds of the kept positions and their max gradient   -> part2
//   k_surface_image    (B) blocks       folds part1 / part2 into the image's constants (range, the two
//                                       centres, the scale, max_gradient)                               -> img
//   k_surface_count    (PB, B) blocks   per-point decisions -> one flag byte per point, block sums      -> flags, bsum
//   k_surface_scan     (B) blocks       exclusive scan of the image's PB block sums on top of the earlier
//                                       images' total                                                    -> boff, offsets
//   k_surface_emit     (PB, B) blocks   row offset = block base + scan of the block's counts; every thread writes its point's rows
//                                       (a thread per ROW, fed from LDS, was tried: coalesced stores, but every row then redoes the
//                                       view frame and its divides, and the kernel is bound by that arithmetic: 233 us against 193)
// Feature-guided SAAG (include/fgs.h): k_surface_emit<true> is the same emit with six parameters read per patch of a guide map, and
//   k_surface_guided_backward (Hp Wp S, B) blocks of one wave   dL/d maps as a gather: a patch owns a rectangle of grid points
//   k_surface_guided_fold                                        adds the S partials of a patch that was split (S > 1 only)
//
// Compiled with -ffp-contract=off and IEEE divide / sqrt, and written in the reference's operation order: every value that feeds a
// decision (drop, skip, thresholds, guards, the wrap direction's flip) is the fp32 value a literal restatement computes
// (tests/surface_checker.py).  No atomics: the reductions are min / max trees of fixed shape, the row order comes from the scan.
// GLM semantics used (GLM 1.0.1 as commonly documented, not read from its source here): dot sums left to right, length = sqrt(dot),
// normalize(v) = v * (1 / sqrt(dot)), v / s divides every component, angleAxis(a, v) = (cos(a/2), v sin(a/2)),
// mix(a, b, t) = a (1 - t) + b t, slerp as in fgs.h.
#include "fgs_internal.h"
#include "fgs_scan.h"  // block_exclusive_scan_256
#include <float.h>
#include <math.h>

namespace {

constexpr int SB = 256;                   // threads per block: one point (or a strided share of the pixels) each
constexpr int RANGE_MAX_BLOCKS = 64;      // per image; <= SB so that one block folds them with one load per thread
constexpr int RANGE_BLOCK_ITEMS = 4096;
constexpr size_t IMG_FLOATS = 16;
constexpr size_t PART2_FLOATS = 8;
enum { IC_MIN_D = 0, IC_RANGE, IC_C1X, IC_C1Y, IC_C1Z, IC_C2X, IC_C2Y, IC_C2Z, IC_SCALE, IC_DO_SCALE, IC_MAX_GRAD };

struct SurfGeom {
    int32_t B, H, W, sub, gw, gh, P, PB, RB;
    float fx, fy, cx, cy;
};

struct SurfLayout {
    size_t flags, part1, part2, img, bsum, boff, total;
};

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator-(V3 a) { return v3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ V3 operator/(V3 a, float s) { return v3(a.x / s, a.y / s, a.z / s); }
__device__ __forceinline__ float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float length3(V3 a) { return sqrtf(dot3(a, a)); }
__device__ __forceinline__ V3 normalize3(V3 a) { return a * (1.0f / sqrtf(dot3(a, a))); }
__device__ __forceinline__ V3 cross3(V3 x, V3 y) {
    return v3(x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y);
}
// std::clamp / std::min / std::max as the C++ library defines them (they differ from fminf / fmaxf on NaN only)
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (hi < v ? hi : v); }

struct Quat { float w, x, y, z; };

// quaternion_from_normal, PC:101-118
__device__ __forceinline__ Quat angle_axis(float angle, V3 v) {
    const float h = angle * 0.5f, s = sinf(h);
    Quat q; q.w = cosf(h); q.x = v.x * s; q.y = v.y * s; q.z = v.z * s;
    return q;
}
__device__ Quat quat_from_normal(V3 n) {
    const V3 up = v3(0.0f, 0.0f, 1.0f);
    const V3 axis = cross3(up, n);
    const float d = dot3(up, n);
    if (length3(axis) < 1e-6f) {
        if (d > 0.0f) { Quat q; q.w = 1.0f; q.x = q.y = q.z = 0.0f; return q; }
        return angle_axis(3.14159265358979323846f, v3(1.0f, 0.0f, 0.0f));
    }
    return angle_axis(acosf(clampf(d, -1.0f, 1.0f)), normalize3(axis));
}
// glm::slerp(identity, q, t), PC:226
__device__ Quat slerp_from_identity(Quat q, float t) {
    float c = q.w;  // dot((1,0,0,0), q)
    if (c < 0.0f) { q.w = -q.w; q.x = -q.x; q.y = -q.y; q.z = -q.z; c = -c; }
    Quat r;
    if (c > 1.0f - FLT_EPSILON) {
        const float u = 1.0f - t;
        r.w = 1.0f * u + q.w * t; r.x = 0.0f * u + q.x * t; r.y = 0.0f * u + q.y * t; r.z = 0.0f * u + q.z * t;
    } else {
        const float a = acosf(c), s0 = sinf((1.0f - t) * a), s1 = sinf(t * a), s = sinf(a);
        r.w = (s0 * 1.0f + s1 * q.w) / s; r.x = (s0 * 0.0f + s1 * q.x) / s;
        r.y = (s0 * 0.0f + s1 * q.y) / s; r.z = (s0 * 0.0f + s1 * q.z) / s;
    }
    return r;
}

// pseudo_random, PC:190-194
__device__ __forceinline__ float pseudo_random(uint32_t x, uint32_t y, int i, uint32_t seed) {
    uint32_t h = (x * 374761393u + y * 668265263u + (uint32_t)i * 2147483647u + seed) ^ 0x85ebca6bu;
    h = ((h >> 16) ^ h) * 0x7feb352du;
    return (float)(h & 0xFFFFu) / 65535.0f;
}

// min and max over the block's 256 threads, every thread gets both (fminf / fmaxf: NaN operands are ignored)
__device__ __forceinline__ void block_min_max(float &mn, float &mx) {
    __shared__ float red[8];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    __syncthreads();  // the previous call's readers are done
    if ((threadIdx.x & 63u) == 0) { red[threadIdx.x >> 6] = mn; red[4 + (threadIdx.x >> 6)] = mx; }
    __syncthreads();
    mn = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    mx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
}

// at_safe: zero outside the frame (IM:167-176)
__device__ __forceinline__ float at_safe(const float *__restrict__ d, int W, int H, int x, int y) {
    return (x >= 0 && x < W && y >= 0 && y < H) ? d[(size_t)y * W + x] : 0.0f;
}
// Sobel gradient, IM:179-180
__device__ __forceinline__ void sobel(const float *__restrict__ d, int W, int H, int x, int y, float &gx, float &gy) {
    const float d00 = at_safe(d, W, H, x - 1, y - 1), d10 = at_safe(d, W, H, x, y - 1), d20 = at_safe(d, W, H, x + 1, y - 1);
    const float d01 = at_safe(d, W, H, x - 1, y), d21 = at_safe(d, W, H, x + 1, y);
    const float d02 = at_safe(d, W, H, x - 1, y + 1), d12 = at_safe(d, W, H, x, y + 1), d22 = at_safe(d, W, H, x + 1, y + 1);
    gx = (-d00 + d20 - 2.0f * d01 + 2.0f * d21 - d02 + d22) / 8.0f;
    gy = (-d00 - 2.0f * d10 - d20 + d02 + 2.0f * d12 + d22) / 8.0f;
}

// one point of from_depth (PC:38-51): -> kept?
__device__ __forceinline__ bool raw_point(const SurfGeom &g, float depth_scale, float d, float min_d, float range, uint32_t x, uint32_t y,
                                          float &conf, V3 &pos) {
    const float nd = (d - min_d) / range;
    const float z = (1.0f - nd) * depth_scale;
    conf = nd;
    pos = v3(((float)x - g.cx) / g.fx * z, (g.cy - (float)y) / g.fy * z, -z);
    return !(z < 0.01f * depth_scale);
}

__device__ __forceinline__ void fold_range(const SurfGeom &g, const float *__restrict__ part1, uint32_t b, float &min_d, float &range) {
    float mn = INFINITY, mx = -INFINITY;
    if ((int)threadIdx.x < g.RB) {
        mn = part1[((size_t)b * g.RB + threadIdx.x) * 2];
        mx = part1[((size_t)b * g.RB + threadIdx.x) * 2 + 1];
    }
    block_min_max(mn, mx);
    min_d = mn;
    range = mx - mn;
    if (range < 1e-6f) range = 1.0f;  // PC:30-31
}

__global__ __launch_bounds__(SB) void k_surface_range(SurfGeom g, const float *__restrict__ depth, float *__restrict__ part1) {
    const uint32_t b = blockIdx.y, hw = (uint32_t)g.H * (uint32_t)g.W;
    const float *d = depth + (size_t)b * hw;
    float mn = INFINITY, mx = -INFINITY;
    for (uint32_t i = blockIdx.x * SB + threadIdx.x; i < hw; i += (uint32_t)g.RB * SB) {
        const float v = d[i];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    block_min_max(mn, mx);
    if (threadIdx.x == 0) {
        part1[((size_t)b * g.RB + blockIdx.x) * 2] = mn;
        part1[((size_t)b * g.RB + blockIdx.x) * 2 + 1] = mx;
    }
}

__global__ __launch_bounds__(SB) void k_surface_points(SurfGeom g, float depth_scale, const float *__restrict__ depth,
                                                       const float *__restrict__ part1, float *__restrict__ part2) {
    const uint32_t b = blockIdx.y, idx = blockIdx.x * SB + threadIdx.x;
    const float *d = depth + (size_t)b * g.H * g.W;
    float min_d, range;
    fold_range(g, part1, b, min_d, range);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, mg = 0.0f, unused = 0.0f;
    if (idx < (uint32_t)g.P) {
        const uint32_t x = (idx % g.gw) * g.sub, y = (idx / g.gw) * g.sub;
        float conf;
        V3 p;
        if (raw_point(g, depth_scale, d[(size_t)y * g.W + x], min_d, range, x, y, conf, p)) {
            lo[0] = hi[0] = p.x; lo[1] = hi[1] = p.y; lo[2] = hi[2] = p.z;
            float gx, gy;
            sobel(d, g.W, g.H, (int)x, (int)y, gx, gy);
            mg = sqrtf(gx * gx + gy * gy);  // IM:183; PC:197-203 starts from 0
        }
    }
    block_min_max(lo[0], hi[0]);
    block_min_max(lo[1], hi[1]);
    block_min_max(lo[2], hi[2]);
    block_min_max(unused, mg);
    if (threadIdx.x == 0) {
        float *o = part2 + ((size_t)b * g.PB + blockIdx.x) * PART2_FLOATS;
        o[0] = lo[0]; o[1] = hi[0]; o[2] = lo[1]; o[3] = hi[1]; o[4] = lo[2]; o[5] = hi[2]; o[6] = mg; o[7] = 0.0f;
    }
}

__global__ __launch_bounds__(SB) void k_surface_image(SurfGeom g, float normalize_extent, const float *__restrict__ part1,
                                                      const float *__restrict__ part2, float *__restrict__ img) {
    const uint32_t b = blockIdx.x;
    float min_d, range;
    fold_range(g, part1, b, min_d, range);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, mg = 0.0f, unused = 0.0f;
    for (uint32_t i = threadIdx.x; i < (uint32_t)g.PB; i += SB) {
        const float *p = part2 + ((size_t)b * g.PB + i) * PART2_FLOATS;
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], p[2 * k]); hi[k] = fmaxf(hi[k], p[2 * k + 1]); }
        mg = fmaxf(mg, p[6]);
    }
    block_min_max(lo[0], hi[0]);
    block_min_max(lo[1], hi[1]);
    block_min_max(lo[2], hi[2]);
    block_min_max(unused, mg);
    if (threadIdx.x != 0) return;
    float *o = img + (size_t)b * IMG_FLOATS;
    float c1[3] = {0.0f, 0.0f, 0.0f}, c2[3] = {0.0f, 0.0f, 0.0f}, scale = 1.0f, do_scale = 0.0f;
    if (normalize_extent > 0.0f && lo[0] <= hi[0]) {  // a kept point exists (PC:449, 461)
        float ext[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c1[k] = (lo[k] + hi[k]) * 0.5f;                     // center(), PC:453
            const float lo1 = lo[k] - c1[k], hi1 = hi[k] - c1[k];  // the bounds of the shifted points: p - c is monotone in p
            c2[k] = (lo1 + hi1) * 0.5f;                          // normalize()'s own center(), PC:464
            ext[k] = (hi1 - c2[k]) - (lo1 - c2[k]);              // PC:469
        }
        const float me = fmaxf(fmaxf(ext[0], ext[1]), ext[2]);
        if (!(me < 1e-6f)) { scale = normalize_extent / me; do_scale = 1.0f; }  // PC:472-475
    }
    if (mg < 1e-6f) mg = 1.0f;  // PC:204
    o[IC_MIN_D] = min_d; o[IC_RANGE] = range;
    o[IC_C1X] = c1[0]; o[IC_C1Y] = c1[1]; o[IC_C1Z] = c1[2];
    o[IC_C2X] = c2[0]; o[IC_C2Y] = c2[1]; o[IC_C2Z] = c2[2];
    o[IC_SCALE] = scale; o[IC_DO_SCALE] = do_scale; o[IC_MAX_GRAD] = mg;
    for (int k = IC_MAX_GRAD + 1; k < (int)IMG_FLOATS; ++k) o[k] = 0.0f;
}

// center(); normalize(extent) applied to one raw position
__device__ __forceinline__ V3 placed(V3 p, float normalize_extent, const float *__restrict__ ic) {
    if (normalize_extent > 0.0f) {
        p = p - v3(ic[IC_C1X], ic[IC_C1Y], ic[IC_C1Z]);
        p = p - v3(ic[IC_C2X], ic[IC_C2Y], ic[IC_C2Z]);
        if (ic[IC_DO_SCALE] != 0.0f) p = p * ic[IC_SCALE];
    }
    return p;
}

// the view-aligned frame of the walls and of compute_wrap_direction (PC:128-139, 299-307): gradient direction -> 3-D
__device__ __forceinline__ V3 gradient_3d(V3 view_dir, float dir_x, float dir_y) {
    const V3 world_up = v3(0.0f, 1.0f, 0.0f);
    V3 right = normalize3(cross3(world_up, view_dir));
    if (length3(right) < 1e-6f) right = v3(1.0f, 0.0f, 0.0f);
    const V3 up = cross3(view_dir, right);
    return right * dir_x + up * dir_y;
}

__device__ __forceinline__ uint32_t rows_of(uint32_t f, const FgsSurfaceParams &prm) {
    return ((f & FGS_SURFACE_BASE) ? 1u : 0u) + ((f & FGS_SURFACE_BACK) ? 1u : 0u) +
           ((f & FGS_SURFACE_WALLS) ? (uint32_t)prm.shell_wall_segments : 0u) +
           ((f & FGS_SURFACE_WRAPS) ? (uint32_t)prm.wrap_layers : 0u) +
           ((f & FGS_SURFACE_FILLS) ? (uint32_t)prm.density_extra_count : 0u);
}

__global__ __launch_bounds__(SB) void k_surface_count(SurfGeom g, FgsSurfaceParams prm, const float *__restrict__ depth,
                                                      const float *__restrict__ img, uint8_t *__restrict__ flags,
                                                      uint32_t *__restrict__ bsum) {
    const uint32_t b = blockIdx.y, idx = blockIdx.x * SB + threadIdx.x;
    const float *d = depth + (size_t)b * g.H * g.W;
    const float *ic = img + (size_t)b * IMG_FLOATS;
    uint32_t f = 0;
    if (idx < (uint32_t)g.P) {
        const uint32_t x = (idx % g.gw) * g.sub, y = (idx / g.gw) * g.sub;
        float conf;
        V3 p;
        if (raw_point(g, prm.depth_scale, d[(size_t)y * g.W + x], ic[IC_MIN_D], ic[IC_RANGE], x, y, conf, p)) {
            f = FGS_SURFACE_KEPT;
            if (!(conf < prm.min_confidence)) {  // PC:208
                f |= FGS_SURFACE_BASE;
                p = placed(p, prm.normalize_extent, ic);
                float gx, gy;
                sobel(d, g.W, g.H, (int)x, (int)y, gx, gy);
                const float mag = sqrtf(gx * gx + gy * gy);
                float dir_x = 0.0f, dir_y = 0.0f;
                if (mag > 1e-6f) { dir_x = gx / mag; dir_y = gy / mag; }  // IM:186-190
                const float ng = mag / ic[IC_MAX_GRAD];                   // PC:235
                if (prm.shell_enabled && ng > prm.shell_edge_threshold) {  // PC:268
                    f |= FGS_SURFACE_BACK;
                    if (prm.shell_connect_walls) {
                        const V3 tangent = gradient_3d(normalize3(p), dir_x, dir_y);
                        if (length3(tangent) > 0.1f) f |= FGS_SURFACE_WALLS;  // PC:309
                    }
                }
                if (prm.wrap_enabled && ng > prm.wrap_edge_threshold && sqrtf(dir_x * dir_x + dir_y * dir_y) > 0.1f)  // PC:348-353
                    f |= FGS_SURFACE_WRAPS;
                if (prm.density_enabled && ng > prm.density_gradient_threshold) f |= FGS_SURFACE_FILLS;  // PC:399
            }
        }
        flags[(size_t)b * g.P + idx] = (uint8_t)f;
    }
    uint32_t tot;
    block_exclusive_scan_256(rows_of(f, prm), &tot);
    if (threadIdx.x == 0) bsum[(size_t)b * g.PB + blockIdx.x] = tot;
}

// one block per image: exclusive scan of the image's PB block sums into `boff`, on top of the sum of all earlier images' block
// sums (which every block adds up for itself: B x PB loads at most, no dependency between the blocks); offsets[b] = that base,
// and the last image's block adds offsets[B] = the total
__global__ __launch_bounds__(SB) void k_surface_scan(uint32_t pb, const uint32_t *__restrict__ bsum, uint32_t *__restrict__ boff,
                                                     int32_t *__restrict__ offsets) {
    const uint32_t b = blockIdx.x, first = b * pb;
    uint32_t part = 0, carry;
    for (uint32_t i = threadIdx.x; i < first; i += SB) part += bsum[i];
    block_exclusive_scan_256(part, &carry);
    __syncthreads();
    if (threadIdx.x == 0) offsets[b] = (int32_t)carry;
    for (uint32_t base = 0; base < pb; base += SB) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < pb ? bsum[first + i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan_256(v, &tot);
        if (i < pb) boff[first + i] = carry + ex;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0 && b + 1 == gridDim.x) offsets[b + 1] = (int32_t)carry;
}

struct SurfOut {
    float *pos, *scale, *rot, *color, *opacity;
    int64_t capacity;
};

__device__ __forceinline__ void put_row(const SurfOut &o, uint32_t row, V3 p, V3 s, Quat q, V3 c, float op) {
    if ((int64_t)row >= o.capacity) return;  // never true after the total check; keeps a corrupted scratch inside the buffers
    const size_t r = row;
    o.pos[r * 3] = p.x; o.pos[r * 3 + 1] = p.y; o.pos[r * 3 + 2] = p.z;
    o.scale[r * 3] = s.x; o.scale[r * 3 + 1] = s.y; o.scale[r * 3 + 2] = s.z;
    o.rot[r * 4] = q.w; o.rot[r * 4 + 1] = q.x; o.rot[r * 4 + 2] = q.y; o.rot[r * 4 + 3] = q.z;
    o.color[r * 3] = c.x; o.color[r * 3 + 1] = c.y; o.color[r * 3 + 2] = c.z;
    o.opacity[r] = op;
}

// The six parameters a guide may modulate per patch (include/fgs.h, "Feature-guided SAAG"), as the point sees them.
struct SurfEff {
    float aspect_ratio, edge_threshold, edge_shrink, normal_strength, base_size, opacity;
};
struct SurfGuide {
    const float *mods;  // (B, 6, Hp, Wp)
    int32_t Hp, Wp;
};
__device__ __forceinline__ SurfEff plain_params(const FgsSurfaceParams &prm) {
    SurfEff e;
    e.aspect_ratio = prm.aspect_ratio; e.edge_threshold = prm.edge_threshold; e.edge_shrink = prm.edge_shrink;
    e.normal_strength = prm.normal_strength; e.base_size = prm.base_size; e.opacity = prm.opacity;
    return e;
}
// the patch of pixel (x, y): integer division on PIXEL coordinates (W Wp and H Hp are below 2^31)
__device__ __forceinline__ size_t patch_of(const SurfGeom &g, const SurfGuide &gd, uint32_t b, uint32_t x, uint32_t y) {
    const uint32_t px = (x * (uint32_t)gd.Wp) / (uint32_t)g.W, py = (y * (uint32_t)gd.Hp) / (uint32_t)g.H;
    return ((size_t)b * 6 * gd.Hp + py) * gd.Wp + px;
}
// one fp32 operation each, rounded on its own; m = (1, 0, 1, 1, 1, 1) leaves every parameter's bits alone
__device__ __forceinline__ SurfEff guided_params(const FgsSurfaceParams &prm, const float *__restrict__ m, size_t plane) {
    SurfEff e;
    e.aspect_ratio = prm.aspect_ratio * m[0];
    e.edge_threshold = prm.edge_threshold + m[plane];
    e.edge_shrink = prm.edge_shrink * m[2 * plane];
    e.normal_strength = prm.normal_strength * m[3 * plane];
    e.base_size = prm.base_size * m[4 * plane];
    e.opacity = prm.opacity * m[5 * plane];
    return e;
}

// GUIDED: fgs_surface_emit_guided -- the six parameters come from the point's patch, and point_rows gets every point's first row
template <bool GUIDED>
__global__ __launch_bounds__(SB) void k_surface_emit(SurfGeom g, FgsSurfaceParams prm, const float *__restrict__ depth,
                                                     const float *__restrict__ color, const float *__restrict__ img,
                                                     const uint8_t *__restrict__ flags, const uint32_t *__restrict__ boff,
                                                     const int32_t *__restrict__ offsets, int32_t *__restrict__ status, SurfGuide guide,
                                                     int32_t *__restrict__ point_rows, SurfOut out) {
    const bool overflow = (int64_t)offsets[g.B] > out.capacity;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *status = overflow ? 1 : 0;
    if (overflow) return;
    const uint32_t b = blockIdx.y, idx = blockIdx.x * SB + threadIdx.x;
    const uint32_t f = idx < (uint32_t)g.P ? flags[(size_t)b * g.P + idx] : 0u;
    uint32_t tot;
    uint32_t row = boff[(size_t)b * g.PB + blockIdx.x] + block_exclusive_scan_256(rows_of(f, prm), &tot);
    if (GUIDED && idx < (uint32_t)g.P) point_rows[(size_t)b * g.P + idx] = (f & FGS_SURFACE_BASE) ? (int32_t)row : -1;
    if (!(f & FGS_SURFACE_BASE)) return;

    const size_t hw = (size_t)g.H * g.W;
    const float *d = depth + (size_t)b * hw;
    const float *ic = img + (size_t)b * IMG_FLOATS;
    const uint32_t x = (idx % g.gw) * g.sub, y = (idx / g.gw) * g.sub;
    const SurfEff e = GUIDED ? guided_params(prm, guide.mods + patch_of(g, guide, b, x, y), (size_t)guide.Hp * guide.Wp)
                             : plain_params(prm);
    float conf;
    V3 pos;
    raw_point(g, prm.depth_scale, d[(size_t)y * g.W + x], ic[IC_MIN_D], ic[IC_RANGE], x, y, conf, pos);
    pos = placed(pos, prm.normalize_extent, ic);
    V3 col = v3(0.7f, 0.7f, 0.7f);  // PC:54
    if (color) {
        const float *c = color + (size_t)b * 3 * hw + (size_t)y * g.W + x;
        col = v3(c[0], c[hw], c[2 * hw]);
    }
    // compute_surface_info, IM:179-207
    float gx, gy;
    sobel(d, g.W, g.H, (int)x, (int)y, gx, gy);
    const float mag = sqrtf(gx * gx + gy * gy);
    float dir_x = 0.0f, dir_y = 0.0f;
    if (mag > 1e-6f) { dir_x = gx / mag; dir_y = gy / mag; }
    V3 normal = v3(-gx * prm.gradient_scale, -gy * prm.gradient_scale, 1.0f);
    const float nlen = length3(normal);
    normal = nlen > 1e-6f ? normal / nlen : v3(0.0f, 0.0f, 1.0f);

    // the base Gaussian, PC:225-261
    const Quat rotation = slerp_from_identity(quat_from_normal(normal), e.normal_strength);
    const float base = e.base_size * (0.5f + 0.5f * conf);
    const float tangent_scale = base, normal_scale = base / e.aspect_ratio;
    const float ng = mag / ic[IC_MAX_GRAD];
    float edge_factor = 1.0f;
    if (ng > e.edge_threshold) {
        float t = (ng - e.edge_threshold) / (1.0f - e.edge_threshold);
        t = clampf(t, 0.0f, 1.0f);
        edge_factor = 1.0f - t * (1.0f - e.edge_shrink);
    }
    const V3 scale = v3(tangent_scale * edge_factor, tangent_scale * edge_factor, normal_scale * edge_factor);
    const float final_opacity = e.opacity * conf * (0.7f + 0.3f * edge_factor);
    put_row(out, row++, pos, scale, rotation, col, final_opacity);

    // volumetric shell: back surface and side walls, PC:268-343
    if (f & FGS_SURFACE_BACK) {
        const V3 view_dir = normalize3(pos);
        const V3 back_pos = pos + view_dir * prm.shell_thickness;
        put_row(out, row++, back_pos, scale, quat_from_normal(view_dir), col * prm.shell_back_darken,
                final_opacity * prm.shell_back_opacity);
        if (f & FGS_SURFACE_WALLS) {
            V3 tangent = gradient_3d(view_dir, dir_x, dir_y);
            tangent = tangent / length3(tangent);
            const Quat wall_rot = quat_from_normal(normalize3(cross3(view_dir, tangent)));
            const float seg_opacity = final_opacity * prm.shell_wall_opacity;
            const V3 wall_scale = scale * 0.9f;
            for (int seg = 1; seg < prm.shell_wall_segments + 1; ++seg) {
                const float t = (float)seg / (float)(prm.shell_wall_segments + 1);
                put_row(out, row++, pos * (1.0f - t) + back_pos * t, wall_scale, wall_rot, col, seg_opacity);
            }
        }
    }
    // silhouette wrapping, PC:348-394 with compute_wrap_direction, PC:122-157
    if (f & FGS_SURFACE_WRAPS) {
        const V3 view_dir = normalize3(pos);
        const V3 grad_3d = gradient_3d(view_dir, dir_x, dir_y);
        V3 wrap = cross3(normal, grad_3d);
        if (dot3(wrap, view_dir) < 0.0f) wrap = -wrap;
        const float wrap_len = length3(wrap);
        const V3 wrap_dir = wrap_len < 1e-6f ? normalize3(grad_3d) : wrap / wrap_len;
        const Quat wrap_rot = quat_from_normal(-wrap_dir);
        const float wrap_base = base * 0.8f;
        const V3 wrap_scale = v3(wrap_base, wrap_base, wrap_base / prm.wrap_aspect);
        for (int layer = 0; layer < prm.wrap_layers; ++layer) {
            const float offset = (float)(layer + 1) * prm.wrap_layer_spacing * e.base_size;
            put_row(out, row++, pos + wrap_dir * offset, wrap_scale, wrap_rot, col,
                    final_opacity * powf(prm.wrap_opacity_falloff, (float)(layer + 1)));
        }
    }
    // adaptive density, PC:399-427
    if (f & FGS_SURFACE_FILLS) {
        const float jitter = prm.density_position_jitter * base;
        const float extra_opacity = final_opacity * prm.density_opacity_scale;
        for (int i = 0; i < prm.density_extra_count; ++i) {
            const float rx = (pseudo_random(x, y, i * 3 + 0, prm.seed) - 0.5f) * 2.0f;
            const float ry = (pseudo_random(x, y, i * 3 + 1, prm.seed) - 0.5f) * 2.0f;
            const float rz = (pseudo_random(x, y, i * 3 + 2, prm.seed) - 0.5f) * 2.0f;
            const float size_var = 1.0f + (pseudo_random(x, y, i * 3 + 100, prm.seed) - 0.5f) * prm.density_size_variance * 2.0f;
            put_row(out, row++, pos + v3(rx, ry, rz) * jitter, scale * size_var * 0.8f, rotation, col, extra_opacity);
        }
    }
}

// ---- the guided emit's backward: dL/d mods, include/fgs.h "Feature-guided SAAG" -------------------------------------------------------
// d slerp_from_identity(q, t) / dt, each branch differentiated as written
__device__ Quat slerp_from_identity_dt(Quat q, float t) {
    float c = q.w;
    if (c < 0.0f) { q.w = -q.w; q.x = -q.x; q.y = -q.y; q.z = -q.z; c = -c; }
    Quat r;
    if (c > 1.0f - FLT_EPSILON) {
        r.w = q.w - 1.0f; r.x = q.x; r.y = q.y; r.z = q.z;
    } else {
        const float a = acosf(c), s = sinf(a), d0 = -a * cosf((1.0f - t) * a), d1 = a * cosf(t * a);
        r.w = (d0 + d1 * q.w) / s; r.x = d1 * q.x / s; r.y = d1 * q.y / s; r.z = d1 * q.z / s;
    }
    return r;
}

struct SurfGrads {
    const float *pos, *scale, *rot, *opacity;  // upstream gradients of the rows; NULL = zeros
};
__device__ __forceinline__ V3 grad3(const float *__restrict__ g, size_t r) { return g ? v3(g[r * 3], g[r * 3 + 1], g[r * 3 + 2]) : v3(0.0f, 0.0f, 0.0f); }
__device__ __forceinline__ float grad1(const float *__restrict__ g, size_t r) { return g ? g[r] : 0.0f; }

constexpr int GB = 64;                  // one wave per (patch, split, image)
constexpr int GUIDE_THREAD_POINTS = 4;  // points a lane walks before a patch is split over more waves
constexpr int GUIDE_MAX_SPLITS = 256;

// grid points whose pixel coordinate lies in patch p of n over `size` pixels: indices [lo, hi) of the subsample grid
__device__ __forceinline__ void patch_span(int32_t p, int32_t n, int32_t size, int32_t sub, int32_t grid, int32_t &lo, int32_t &hi) {
    const int64_t x0 = ((int64_t)p * size + n - 1) / n, x1 = ((int64_t)(p + 1) * size + n - 1) / n;  // pixels [x0, x1): x n / size == p
    lo = (int32_t)((x0 + sub - 1) / sub);
    hi = (int32_t)((x1 + sub - 1) / sub);
    if (hi > grid) hi = grid;
    if (lo > hi) lo = hi;
}

// One wave per (patch, split, image): lane l of split s takes the patch's grid points s GB + l, + S GB, ... in row-major order,
// recomputes each point's forward, folds the upstream gradients of its rows into six partials; a butterfly of fixed shape sums
// the wave.  S == 1: the sums are g_mods; else they go to `dst` = partials (B, Hp Wp, S, 6) for k_surface_guided_fold.
__global__ __launch_bounds__(GB) void k_surface_guided_backward(SurfGeom g, FgsSurfaceParams prm, const float *__restrict__ depth,
                                                                const float *__restrict__ img, const uint8_t *__restrict__ flags,
                                                                const int32_t *__restrict__ offsets, SurfGuide guide, int32_t S,
                                                                const int32_t *__restrict__ point_rows, SurfGrads gr,
                                                                float *__restrict__ dst) {
    const uint32_t b = blockIdx.y, patch = blockIdx.x / (uint32_t)S, split = blockIdx.x % (uint32_t)S;
    const int32_t py = (int32_t)(patch / (uint32_t)guide.Wp), px = (int32_t)(patch % (uint32_t)guide.Wp);
    const size_t plane = (size_t)guide.Hp * guide.Wp;
    int32_t gx0, gx1, gy0, gy1;
    patch_span(px, guide.Wp, g.W, g.sub, g.gw, gx0, gx1);
    patch_span(py, guide.Hp, g.H, g.sub, g.gh, gy0, gy1);
    const uint32_t nx = (uint32_t)(gx1 - gx0), n = nx * (uint32_t)(gy1 - gy0);
    const SurfEff e = guided_params(prm, guide.mods + ((size_t)b * 6 * guide.Hp + py) * guide.Wp + px, plane);
    const float *d = depth + (size_t)b * g.H * g.W;
    const float *ic = img + (size_t)b * IMG_FLOATS;
    const int64_t total = offsets[g.B];
    float acc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t k = split * GB + threadIdx.x; k < n; k += (uint32_t)S * GB) {
        const uint32_t idx = (uint32_t)(gy0 + (int32_t)(k / nx)) * (uint32_t)g.gw + (uint32_t)(gx0 + (int32_t)(k % nx));
        const uint32_t f = flags[(size_t)b * g.P + idx];
        if (!(f & FGS_SURFACE_BASE)) continue;
        const int64_t first = point_rows[(size_t)b * g.P + idx];
        if (first < 0 || first + (int64_t)rows_of(f, prm) > total) continue;  // never true for the emit's point_rows: keeps the reads inside
        size_t r = (size_t)first;
        const uint32_t x = (idx % g.gw) * g.sub, y = (idx / g.gw) * g.sub;
        float conf;
        V3 pos;
        raw_point(g, prm.depth_scale, d[(size_t)y * g.W + x], ic[IC_MIN_D], ic[IC_RANGE], x, y, conf, pos);
        pos = placed(pos, prm.normalize_extent, ic);
        float gx, gy;
        sobel(d, g.W, g.H, (int)x, (int)y, gx, gy);
        const float mag = sqrtf(gx * gx + gy * gy);
        float dir_x = 0.0f, dir_y = 0.0f;
        if (mag > 1e-6f) { dir_x = gx / mag; dir_y = gy / mag; }
        V3 normal = v3(-gx * prm.gradient_scale, -gy * prm.gradient_scale, 1.0f);
        const float nlen = length3(normal);
        normal = nlen > 1e-6f ? normal / nlen : v3(0.0f, 0.0f, 1.0f);
        // the forward's values, as k_surface_emit computes them
        const float c1 = 0.5f + 0.5f * conf, base = e.base_size * c1, normal_scale = base / e.aspect_ratio;
        const float ng = mag / ic[IC_MAX_GRAD];
        float edge_factor = 1.0f, t = 0.0f;
        bool edge = false, inside = false;
        if (ng > e.edge_threshold) {
            edge = true;
            t = (ng - e.edge_threshold) / (1.0f - e.edge_threshold);
            inside = !(t < 0.0f) && !(1.0f < t);  // the clamp passes its gradient on the closed interval
            t = clampf(t, 0.0f, 1.0f);
            edge_factor = 1.0f - t * (1.0f - e.edge_shrink);
        }
        // upstream gradients, row by row in emit order, folded into: the shared scale (Gs), the shared rotation (Gq),
        // final_opacity (Gfo), `base` beyond the shared scale (Gbase) and base_size' through the wrap offsets (Gbs)
        V3 Gs = grad3(gr.scale, r);
        Quat Gq;
        Gq.w = Gq.x = Gq.y = Gq.z = 0.0f;
        if (gr.rot) { Gq.w = gr.rot[r * 4]; Gq.x = gr.rot[r * 4 + 1]; Gq.y = gr.rot[r * 4 + 2]; Gq.z = gr.rot[r * 4 + 3]; }
        float Gfo = grad1(gr.opacity, r), Gbase = 0.0f, Gbs = 0.0f;
        ++r;
        if (f & FGS_SURFACE_BACK) {
            Gs = Gs + grad3(gr.scale, r);
            Gfo += grad1(gr.opacity, r) * prm.shell_back_opacity;
            ++r;
            if (f & FGS_SURFACE_WALLS)
                for (int seg = 1; seg < prm.shell_wall_segments + 1; ++seg, ++r) {
                    Gs = Gs + grad3(gr.scale, r) * 0.9f;
                    Gfo += grad1(gr.opacity, r) * prm.shell_wall_opacity;
                }
        }
        if (f & FGS_SURFACE_WRAPS) {
            const V3 view_dir = normalize3(pos);
            const V3 grad_3d = gradient_3d(view_dir, dir_x, dir_y);
            V3 wrap = cross3(normal, grad_3d);
            if (dot3(wrap, view_dir) < 0.0f) wrap = -wrap;
            const float wrap_len = length3(wrap);
            const V3 wrap_dir = wrap_len < 1e-6f ? normalize3(grad_3d) : wrap / wrap_len;
            for (int layer = 0; layer < prm.wrap_layers; ++layer, ++r) {
                const V3 gs = grad3(gr.scale, r);
                Gbase += (gs.x + gs.y) * 0.8f + gs.z * (0.8f / prm.wrap_aspect);
                Gbs += dot3(grad3(gr.pos, r), wrap_dir) * ((float)(layer + 1) * prm.wrap_layer_spacing);
                Gfo += grad1(gr.opacity, r) * powf(prm.wrap_opacity_falloff, (float)(layer + 1));
            }
        }
        if (f & FGS_SURFACE_FILLS)
            for (int i = 0; i < prm.density_extra_count; ++i, ++r) {
                const float rx = (pseudo_random(x, y, i * 3 + 0, prm.seed) - 0.5f) * 2.0f;
                const float ry = (pseudo_random(x, y, i * 3 + 1, prm.seed) - 0.5f) * 2.0f;
                const float rz = (pseudo_random(x, y, i * 3 + 2, prm.seed) - 0.5f) * 2.0f;
                const float size_var = 1.0f + (pseudo_random(x, y, i * 3 + 100, prm.seed) - 0.5f) * prm.density_size_variance * 2.0f;
                Gs = Gs + grad3(gr.scale, r) * (size_var * 0.8f);
                Gbase += dot3(grad3(gr.pos, r), v3(rx, ry, rz)) * prm.density_position_jitter;
                Gfo += grad1(gr.opacity, r) * prm.density_opacity_scale;
                if (gr.rot) { Gq.w += gr.rot[r * 4]; Gq.x += gr.rot[r * 4 + 1]; Gq.y += gr.rot[r * 4 + 2]; Gq.z += gr.rot[r * 4 + 3]; }
            }
        // scale = (base, base, base / aspect') edge_factor;  final_opacity = opacity' conf (0.7 + 0.3 edge_factor)
        const float d_tangent = (Gs.x + Gs.y) * edge_factor, d_normal = Gs.z * edge_factor;
        const float d_ef = (Gs.x + Gs.y) * base + Gs.z * normal_scale + Gfo * (e.opacity * conf) * 0.3f;
        const float d_base = d_tangent + d_normal / e.aspect_ratio + Gbase;
        acc[0] += d_normal * (-normal_scale / e.aspect_ratio) * prm.aspect_ratio;
        if (edge) {
            if (inside) {  // dt / d threshold' = (ng - 1) / (1 - threshold')^2
                const float u = 1.0f - e.edge_threshold;
                acc[1] += -d_ef * (1.0f - e.edge_shrink) * ((ng - 1.0f) / (u * u));
            }
            acc[2] += d_ef * t * prm.edge_shrink;
        }
        if (gr.rot) {
            const Quat dq = slerp_from_identity_dt(quat_from_normal(normal), e.normal_strength);
            acc[3] += (Gq.w * dq.w + Gq.x * dq.x + Gq.y * dq.y + Gq.z * dq.z) * prm.normal_strength;
        }
        acc[4] += (d_base * c1 + Gbs) * prm.base_size;
        acc[5] += Gfo * (conf * (0.7f + 0.3f * edge_factor)) * prm.opacity;
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 64);
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            if (S == 1) dst[((size_t)b * 6 + c) * plane + patch] = acc[c];
            else dst[(((size_t)b * plane + patch) * S + split) * 6 + c] = acc[c];
        }
    }
}

// one thread per (patch, image): the S partials summed in split order
__global__ __launch_bounds__(SB) void k_surface_guided_fold(uint32_t plane, int32_t S, const float *__restrict__ part,
                                                            float *__restrict__ g_mods) {
    const uint32_t b = blockIdx.y, patch = blockIdx.x * SB + threadIdx.x;
    if (patch >= plane) return;
    float acc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const float *p = part + ((size_t)b * plane + patch) * S * 6;
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[c] += p[(size_t)s * 6 + c];
#pragma unroll
    for (int c = 0; c < 6; ++c) g_mods[((size_t)b * 6 + c) * plane + patch] = acc[c];
}

int geometry(const FgsSurfaceDims *d, const FgsSurfaceParams *p, SurfGeom *g, SurfLayout *L, const char *who) {
    if (!d || !p) { fgs_set_error("%s: null dims or params", who); return FGS_EINVAL; }
    if (d->batch < 1 || d->batch > 65535 || d->height < 1 || d->width < 1 ||
        (uint64_t)d->batch * (uint64_t)d->height * (uint64_t)d->width >= (1ull << 31)) {
        fgs_set_error("%s: invalid dims B=%d H=%d W=%d", who, d->batch, d->height, d->width);
        return FGS_EINVAL;
    }
    if (p->subsample < 1) { fgs_set_error("%s: invalid params: subsample = %d < 1", who, p->subsample); return FGS_EINVAL; }
    if (p->shell_wall_segments < 0 || p->wrap_layers < 0 || p->density_extra_count < 0) {
        fgs_set_error("%s: invalid params: negative layer count (wall_segments %d, wrap_layers %d, extra_count %d)", who,
                      p->shell_wall_segments, p->wrap_layers, p->density_extra_count);
        return FGS_EINVAL;
    }
    g->B = d->batch; g->H = d->height; g->W = d->width; g->sub = p->subsample;
    g->gw = (d->width + p->subsample - 1) / p->subsample;
    g->gh = (d->height + p->subsample - 1) / p->subsample;
    g->P = g->gw * g->gh;
    g->PB = (g->P + SB - 1) / SB;
    const int64_t hw = (int64_t)d->height * d->width, rb = (hw + RANGE_BLOCK_ITEMS - 1) / RANGE_BLOCK_ITEMS;
    g->RB = (int32_t)(rb < RANGE_MAX_BLOCKS ? rb : RANGE_MAX_BLOCKS);
    const uint64_t fan = 2ull + (uint64_t)p->shell_wall_segments + (uint64_t)p->wrap_layers + (uint64_t)p->density_extra_count;
    if ((uint64_t)d->batch * (uint64_t)g->P * fan >= (1ull << 31)) {
        fgs_set_error("%s: invalid dims: B x P x rows per point = %d x %d x %llu is beyond 2^31", who, d->batch, g->P,
                      (unsigned long long)fan);
        return FGS_EINVAL;
    }
    // PC:22-25 with the viewer's focal length (viewer.cpp:364-367) as the default
    g->fx = p->fx > 0.0f ? p->fx : (float)d->width * 0.8f;
    g->fy = p->fy > 0.0f ? p->fy : g->fx;
    g->cx = p->cx > 0.0f ? p->cx : (float)d->width * 0.5f;
    g->cy = p->cy > 0.0f ? p->cy : (float)d->height * 0.5f;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t bp = (size_t)d->batch * g->P, bpb = (size_t)d->batch * g->PB;
    L->flags = FGS_SURFACE_STATE_OFFSET;
    L->part1 = up(L->flags + bp);
    L->part2 = up(L->part1 + (size_t)d->batch * g->RB * 2 * sizeof(float));
    L->img = up(L->part2 + bpb * PART2_FLOATS * sizeof(float));
    L->bsum = up(L->img + (size_t)d->batch * IMG_FLOATS * sizeof(float));
    L->boff = up(L->bsum + bpb * sizeof(uint32_t));
    L->total = up(L->boff + bpb * sizeof(uint32_t));
    return FGS_OK;
}

// the guide's shape (host only, before anything touches the device); *splits: waves per patch of the backward
int guide_geometry(const SurfGeom &g, int32_t mods_h, int32_t mods_w, int32_t *splits, const char *who) {
    if (mods_h < 1 || mods_w < 1) { fgs_set_error("%s: invalid guide: mods_h = %d, mods_w = %d (both >= 1)", who, mods_h, mods_w); return FGS_EINVAL; }
    if ((int64_t)g.W * mods_w >= (1ll << 31) || (int64_t)g.H * mods_h >= (1ll << 31)) {
        fgs_set_error("%s: invalid guide: W x mods_w = %d x %d or H x mods_h = %d x %d is beyond 2^31", who, g.W, mods_w, g.H, mods_h);
        return FGS_EINVAL;
    }
    if ((uint64_t)g.B * 6ull * (uint64_t)mods_h * (uint64_t)mods_w >= (1ull << 31)) {
        fgs_set_error("%s: invalid guide: B x 6 x mods_h x mods_w = %d x 6 x %d x %d is beyond 2^31", who, g.B, mods_h, mods_w);
        return FGS_EINVAL;
    }
    // the most grid points a patch can own: ceil(W / Wp) pixels hold at most ceil(that / subsample) multiples of subsample
    const int64_t pw = ((int64_t)g.W + mods_w - 1) / mods_w, ph = ((int64_t)g.H + mods_h - 1) / mods_h;
    const int64_t pts = ((pw + g.sub - 1) / g.sub) * ((ph + g.sub - 1) / g.sub);
    int64_t s = (pts + (int64_t)GB * GUIDE_THREAD_POINTS - 1) / ((int64_t)GB * GUIDE_THREAD_POINTS);
    s = s < 1 ? 1 : (s > GUIDE_MAX_SPLITS ? GUIDE_MAX_SPLITS : s);
    if ((uint64_t)mods_h * (uint64_t)mods_w * (uint64_t)s >= (1ull << 31)) {
        fgs_set_error("%s: invalid guide: mods_h x mods_w x %lld waves per patch is beyond 2^31", who, (long long)s);
        return FGS_EINVAL;
    }
    *splits = (int32_t)s;
    return FGS_OK;
}

}  // namespace

extern "C" {

int fgs_surface_workspace_bytes(const FgsSurfaceDims *dims, const FgsSurfaceParams *params, size_t *scratch_bytes) {
    SurfGeom g;
    SurfLayout L;
    int rc = geometry(dims, params, &g, &L, "fgs_surface_workspace_bytes");
    if (rc) return rc;
    if (!scratch_bytes) { fgs_set_error("fgs_surface_workspace_bytes: null output pointer"); return FGS_EINVAL; }
    *scratch_bytes = L.total;
    return FGS_OK;
}

int fgs_surface_count(const FgsSurfaceDims *dims, const FgsSurfaceParams *params, const float *depth, void *scratch,
                      int32_t *offsets, void *stream) {
    SurfGeom g;
    SurfLayout L;
    int rc = geometry(dims, params, &g, &L, "fgs_surface_count");
    if (rc) return rc;
    if (!depth || !scratch || !offsets) { fgs_set_error("fgs_surface_count: null pointer argument"); return FGS_EINVAL; }
    char *s = reinterpret_cast<char *>(scratch);
    float *part1 = reinterpret_cast<float *>(s + L.part1), *part2 = reinterpret_cast<float *>(s + L.part2);
    float *img = reinterpret_cast<float *>(s + L.img);
    uint32_t *bsum = reinterpret_cast<uint32_t *>(s + L.bsum);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_surface_range, dim3(g.RB, g.B), dim3(SB), 0, st, g, depth, part1);
    FGS_LAUNCH_CHECK("k_surface_range");
    hipLaunchKernelGGL(k_surface_points, dim3(g.PB, g.B), dim3(SB), 0, st, g, params->depth_scale, depth, part1, part2);
    FGS_LAUNCH_CHECK("k_surface_points");
    hipLaunchKernelGGL(k_surface_image, dim3(g.B), dim3(SB), 0, st, g, params->normalize_extent, part1, part2, img);
    FGS_LAUNCH_CHECK("k_surface_image");
    hipLaunchKernelGGL(k_surface_count, dim3(g.PB, g.B), dim3(SB), 0, st, g, *params, depth, img,
                       reinterpret_cast<uint8_t *>(s + L.flags), bsum);
    FGS_LAUNCH_CHECK("k_surface_count");
    hipLaunchKernelGGL(k_surface_scan, dim3(g.B), dim3(SB), 0, st, (uint32_t)g.PB, bsum, reinterpret_cast<uint32_t *>(s + L.boff), offsets);
    FGS_LAUNCH_CHECK("k_surface_scan");
    return FGS_OK;
}

int fgs_surface_emit(const FgsSurfaceDims *dims, const FgsSurfaceParams *params, const float *depth, const float *color,
                     void *scratch, const int32_t *offsets, float *o_positions, float *o_scales, float *o_rotations,
                     float *o_colors, float *o_opacities, int64_t capacity, void *stream) {
    SurfGeom g;
    SurfLayout L;
    int rc = geometry(dims, params, &g, &L, "fgs_surface_emit");
    if (rc) return rc;
    if (capacity < 0) { fgs_set_error("fgs_surface_emit: invalid capacity %lld", (long long)capacity); return FGS_EINVAL; }
    // (a capacity of 0 rows may come with null outputs: nothing can be written)
    if (!depth || !scratch || !offsets || (capacity > 0 && (!o_positions || !o_scales || !o_rotations || !o_colors || !o_opacities))) {
        fgs_set_error("fgs_surface_emit: null pointer argument");
        return FGS_EINVAL;
    }
    char *s = reinterpret_cast<char *>(scratch);
    SurfOut out{o_positions, o_scales, o_rotations, o_colors, o_opacities, capacity};
    hipLaunchKernelGGL(k_surface_emit<false>, dim3(g.PB, g.B), dim3(SB), 0, reinterpret_cast<hipStream_t>(stream), g, *params, depth, color,
                       reinterpret_cast<const float *>(s + L.img), reinterpret_cast<const uint8_t *>(s + L.flags),
                       reinterpret_cast<const uint32_t *>(s + L.boff), offsets, reinterpret_cast<int32_t *>(s), SurfGuide{nullptr, 0, 0},
                       static_cast<int32_t *>(nullptr), out);
    FGS_LAUNCH_CHECK("k_surface_emit");
    return FGS_OK;
}

int fgs_surface_emit_guided(const FgsSurfaceDims *dims, const FgsSurfaceParams *params, const float *depth, const float *color,
                            void *scratch, const int32_t *offsets, const float *mods, int32_t mods_h, int32_t mods_w,
                            float *o_positions, float *o_scales, float *o_rotations, float *o_colors, float *o_opacities,
                            int32_t *point_rows, int64_t capacity, void *stream) {
    SurfGeom g;
    SurfLayout L;
    int32_t splits;
    int rc = geometry(dims, params, &g, &L, "fgs_surface_emit_guided");
    if (rc) return rc;
    rc = guide_geometry(g, mods_h, mods_w, &splits, "fgs_surface_emit_guided");
    if (rc) return rc;
    if (capacity < 0) { fgs_set_error("fgs_surface_emit_guided: invalid capacity %lld", (long long)capacity); return FGS_EINVAL; }
    if (!depth || !scratch || !offsets || !mods || !point_rows ||
        (capacity > 0 && (!o_positions || !o_scales || !o_rotations || !o_colors || !o_opacities))) {
        fgs_set_error("fgs_surface_emit_guided: null pointer argument");
        return FGS_EINVAL;
    }
    char *s = reinterpret_cast<char *>(scratch);
    SurfOut out{o_positions, o_scales, o_rotations, o_colors, o_opacities, capacity};
    hipLaunchKernelGGL(k_surface_emit<true>, dim3(g.PB, g.B), dim3(SB), 0, reinterpret_cast<hipStream_t>(stream), g, *params, depth, color,
                       reinterpret_cast<const float *>(s + L.img), reinterpret_cast<const uint8_t *>(s + L.flags),
                       reinterpret_cast<const uint32_t *>(s + L.boff), offsets, reinterpret_cast<int32_t *>(s),
                       SurfGuide{mods, mods_h, mods_w}, point_rows, out);
    FGS_LAUNCH_CHECK("k_surface_emit<guided>");
    return FGS_OK;
}

int fgs_surface_guided_backward_bytes(const FgsSurfaceDims *dims, const FgsSurfaceParams *params, int32_t mods_h, int32_t mods_w,
                                      size_t *bytes) {
    SurfGeom g;
    SurfLayout L;
    int32_t splits;
    int rc = geometry(dims, params, &g, &L, "fgs_surface_guided_backward_bytes");
    if (rc) return rc;
    rc = guide_geometry(g, mods_h, mods_w, &splits, "fgs_surface_guided_backward_bytes");
    if (rc) return rc;
    if (!bytes) { fgs_set_error("fgs_surface_guided_backward_bytes: null output pointer"); return FGS_EINVAL; }
    *bytes = splits == 1 ? 0 : (size_t)g.B * mods_h * mods_w * splits * 6 * sizeof(float);
    return FGS_OK;
}

int fgs_surface_guided_backward(const FgsSurfaceDims *dims, const FgsSurfaceParams *params, const float *depth, const void *scratch,
                                const int32_t *offsets, const float *mods, int32_t mods_h, int32_t mods_w, const int32_t *point_rows,
                                const float *g_positions, const float *g_scales, const float *g_rotations, const float *g_opacities,
                                float *g_mods, void *bwd_scratch, void *stream) {
    SurfGeom g;
    SurfLayout L;
    int32_t splits;
    int rc = geometry(dims, params, &g, &L, "fgs_surface_guided_backward");
    if (rc) return rc;
    rc = guide_geometry(g, mods_h, mods_w, &splits, "fgs_surface_guided_backward");
    if (rc) return rc;
    if (!depth || !scratch || !offsets || !mods || !point_rows || !g_mods || (splits > 1 && !bwd_scratch)) {
        fgs_set_error("fgs_surface_guided_backward: null pointer argument");
        return FGS_EINVAL;
    }
    const char *s = reinterpret_cast<const char *>(scratch);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint32_t plane = (uint32_t)mods_h * (uint32_t)mods_w;
    float *part = reinterpret_cast<float *>(bwd_scratch);
    hipLaunchKernelGGL(k_surface_guided_backward, dim3(plane * (uint32_t)splits, g.B), dim3(GB), 0, st, g, *params, depth,
                       reinterpret_cast<const float *>(s + L.img), reinterpret_cast<const uint8_t *>(s + L.flags), offsets,
                       SurfGuide{mods, mods_h, mods_w}, splits, point_rows, SurfGrads{g_positions, g_scales, g_rotations, g_opacities},
                       splits == 1 ? g_mods : part);
    FGS_LAUNCH_CHECK("k_surface_guided_backward");
    if (splits > 1) {
        hipLaunchKernelGGL(k_surface_guided_fold, dim3((plane + SB - 1) / SB, g.B), dim3(SB), 0, st, plane, splits, part, g_mods);
        FGS_LAUNCH_CHECK("k_surface_guided_fold");
    }
    return FGS_OK;
}

}  // extern "C"
