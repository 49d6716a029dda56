// Structural similarity loss on the rendered batch (pytorch_msssim.ssim, the SSIM term of the reference's training loss,
// TGD:904): Gaussian-window "valid" SSIM of (B, C, H, W) fp32 planes, Wang et al. 2004.
//
//   k_ssim_fwd      one block per 64 x 32 tile of OUTPUT (valid) pixels of one plane: X and Y staged in LDS with their
//                   (taps - 1) halo, horizontal pass of the five moments (x, y, x^2, y^2, xy) into LDS, vertical pass in
//                   registers, S per pixel, one double partial sum per block; on request the backward's factor maps
//                   dS/dmu_x, dS/dE[x^2] (= dS/dE[y^2]), dS/dE[xy] and, for dY, dS/dmu_y (unscaled)
//   k_ssim_reduce   one block: per-plane mean of S from the partials (double, fixed order), optional relu, the mean
//                   over the batch (scalar) or over the channels (per image)
//   k_ssim_bwd      one block per 64 x 32 tile of INPUT pixels: each factor map staged in LDS and filtered with the
//                   mirrored taps (the transpose of the valid filter = zero-padded full convolution), then
//                   dX = s (G0 + 2 X G1 + Y G2), dY = s (G3 + 2 Y G1 + X G2), s = the plane's weight of the mean
//
// Both filters are one code shape, the valid correlation of a staged (32 + n - 1) x (64 + n - 1) region with n taps: the
// backward passes the taps reversed.  11 taps are compiled in (the fast path, every loop static); any odd count up to 15
// takes the general path.  No atomics: partial sums are summed in block order, so results repeat bit for bit.
#include "fgs_internal.h"

namespace {

constexpr int MAXT = 15;          // largest window (FgsSsimDims.taps)
constexpr int TW = 64;            // tile width: one wave's lanes
constexpr int TH = 32;            // tile height
constexpr int NTHR = 512;         // 8 waves: a wave row of 64 columns x 4 rows per thread in the vertical pass
constexpr int RPT = TH / (NTHR / TW);  // rows per thread in the vertical pass
constexpr int RT = 256;           // threads of the reduction kernel
static_assert(RPT == 4, "vertical pass layout");

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Taps { float w[MAXT]; };

struct Geo {
    int planes, H, W, Ho, Wo, tiles_x, tiles_y;
    int nmaps;              // factor maps in `saved`: 0, 3 (dX) or 4 (dY, and dX with them)
    size_t map_stride;      // floats between two maps
};

int make_geo(const FgsSsimDims *d, Geo *g, const char *who) {
    if (!d) { fgs_set_error("%s: null dims", who); return FGS_EINVAL; }
    if (d->images < 1 || d->channels < 1 || d->num_taps < 1 || d->num_taps > MAXT || !(d->num_taps & 1) ||
        d->height < d->num_taps || d->width < d->num_taps || (d->flags & ~15) || !(d->c1 >= 0.0f) || !(d->c2 >= 0.0f)) {
        fgs_set_error("%s: invalid dims (images %d, channels %d, %d x %d, %d taps, flags %d): the window must be odd, at most %d "
                      "taps and no larger than the frame", who, d->images, d->channels, d->height, d->width, d->num_taps,
                      d->flags, MAXT);
        return FGS_EINVAL;
    }
    g->planes = d->images * d->channels;
    g->H = d->height;
    g->W = d->width;
    g->Ho = d->height - d->num_taps + 1;
    g->Wo = d->width - d->num_taps + 1;
    g->tiles_x = (g->Wo + TW - 1) / TW;
    g->tiles_y = (g->Ho + TH - 1) / TH;
    g->nmaps = (d->flags & FGS_SSIM_GRAD_Y) ? 4 : (d->flags & FGS_SSIM_GRAD_X) ? 3 : 0;
    g->map_stride = align256((size_t)g->planes * g->Ho * g->Wo * sizeof(float)) / sizeof(float);
    const size_t blocks = (size_t)g->planes * g->tiles_x * g->tiles_y;
    const size_t bwd_blocks = (size_t)g->planes * ((g->W + TW - 1) / TW) * ((g->H + TH - 1) / TH);
    if (blocks >= (1ull << 31) || bwd_blocks >= (1ull << 31) || (size_t)g->planes * g->H * g->W >= (1ull << 40)) {
        fgs_set_error("%s: batch too large", who);
        return FGS_EINVAL;
    }
    return FGS_OK;
}

size_t cs_bytes(const Geo &g) { return align256((size_t)g.planes * sizeof(double)); }

// The staged region of a tile: rows [r0, r0 + TH + n - 1) x columns [c0, c0 + TW + n - 1) of one H x W plane, zero outside
// the plane, stored densely (pitch TW + n - 1).  Split in two so that a block issues every global load of its staging before
// the first LDS store (one memory latency per tile, not one per loop trip).  IT: loop trips for the largest n.
template <int IT>
__device__ __forceinline__ void stage_load(float (&v)[IT], const float *__restrict__ src, int H, int W, int r0, int c0, int n) {
    const int cols = TW + n - 1, total = (TH + n - 1) * cols;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = threadIdx.x + it * NTHR;
        const int rr = i / cols, cc = i - rr * cols;
        const int gr = r0 + rr, gc = c0 + cc;
        v[it] = (i < total && gr >= 0 && gr < H && gc >= 0 && gc < W) ? src[(size_t)gr * W + gc] : 0.0f;
    }
}
template <int IT>
__device__ __forceinline__ void stage_store(float *dst, const float (&v)[IT], int n) {
    const int total = (TH + n - 1) * (TW + n - 1);
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = threadIdx.x + it * NTHR;
        if (i < total) dst[i] = v[it];
    }
}
constexpr int stage_trips(int kt) { return ((TH + kt - 1) * (TW + kt - 1) + NTHR - 1) / NTHR; }

// block sum of one double per thread in a fixed order (wave shuffles, then the wave totals in order); result in thread 0
__device__ __forceinline__ double block_sum(double v, double *ws) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63u) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < NTHR / 64; ++w) t += ws[w];
    return t;
}

// ---- forward --------------------------------------------------------------------------------------------------------
// NT: compiled-in tap count (11), or 0 = runtime count n <= MAXT.  Output pixel (y, x) of a plane covers input rows
// y .. y + n - 1 and columns x .. x + n - 1.
template <int NT>
__global__ __launch_bounds__(NTHR) void k_ssim_fwd(Geo g, Taps taps, int n_rt, float c1, float c2,
                                                   const float *__restrict__ X, const float *__restrict__ Y,
                                                   float *__restrict__ maps, double *__restrict__ part) {
    constexpr int KT = NT ? NT : MAXT;        // static loop bound
    constexpr int SR = TH + KT - 1;           // staged rows
    constexpr int IT = stage_trips(KT);
    __shared__ float sx[SR * (TW + KT - 1)], sy[SR * (TW + KT - 1)];
    __shared__ float sm[5][SR * TW];          // horizontal moments: x, y, x^2, y^2, xy
    __shared__ double ws[NTHR / 64];
    const int n = NT ? NT : n_rt;
    const int tiles = g.tiles_x * g.tiles_y;
    const int plane = blockIdx.x / tiles, tile = blockIdx.x - plane * tiles;
    const int r0 = (tile / g.tiles_x) * TH, c0 = (tile % g.tiles_x) * TW;
    const size_t poff = (size_t)plane * g.H * g.W;
    {
        float vx[IT], vy[IT];
        stage_load(vx, X + poff, g.H, g.W, r0, c0, n);
        stage_load(vy, Y + poff, g.H, g.W, r0, c0, n);
        stage_store(sx, vx, n);
        stage_store(sy, vy, n);
    }
    __syncthreads();
    const int rows = TH + n - 1, sp = TW + n - 1;
    for (int i = threadIdx.x; i < rows * TW; i += NTHR) {
        const int rr = i >> 6, cc = i & 63;
        const float *px = sx + rr * sp + cc, *py = sy + rr * sp + cc;
        float mx = 0.f, my = 0.f, mxx = 0.f, myy = 0.f, mxy = 0.f;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            if (NT == 0 && k >= n) break;
            const float x = px[k], y = py[k], w = taps.w[k];
            mx += w * x;
            my += w * y;
            mxx += w * (x * x);
            myy += w * (y * y);
            mxy += w * (x * y);
        }
        sm[0][i] = mx; sm[1][i] = my; sm[2][i] = mxx; sm[3][i] = myy; sm[4][i] = mxy;
    }
    __syncthreads();
    // vertical pass: thread (tx, ty) owns column tx, rows ty*4 .. ty*4+3 of the tile; staged row ty*4 + j feeds local
    // output row o through tap j - o (static in both paths: j and o are unrolled, only the guard reads n)
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    float acc[RPT][5];
#pragma unroll
    for (int o = 0; o < RPT; ++o)
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[o][m] = 0.f;
#pragma unroll
    for (int j = 0; j < RPT + KT - 1; ++j) {
        if (NT == 0 && j >= RPT + n - 1) break;
        const int idx = (ty * RPT + j) * TW + tx;
        const float v[5] = {sm[0][idx], sm[1][idx], sm[2][idx], sm[3][idx], sm[4][idx]};
#pragma unroll
        for (int o = 0; o < RPT; ++o) {
            const int k = j - o;
            if (k < 0 || k >= KT || (NT == 0 && k >= n)) continue;
            const float w = taps.w[k];
#pragma unroll
            for (int m = 0; m < 5; ++m) acc[o][m] += w * v[m];
        }
    }
    const int x = c0 + tx;
    const size_t plane_px = (size_t)g.Ho * g.Wo;
    double ssum = 0.0;
#pragma unroll
    for (int o = 0; o < RPT; ++o) {
        const int y = r0 + ty * RPT + o;
        if (y >= g.Ho || x >= g.Wo) continue;
        const float mux = acc[o][0], muy = acc[o][1];
        const float mux2 = mux * mux, muy2 = muy * muy, muxy = mux * muy;
        const float sxx = acc[o][2] - mux2, syy = acc[o][3] - muy2, sxy = acc[o][4] - muxy;
        const float a1 = 2.f * muxy + c1, b1 = mux2 + muy2 + c1, a2 = 2.f * sxy + c2, b2 = sxx + syy + c2;
        const float s = (a1 / b1) * (a2 / b2);  // luminance x contrast-structure, as pytorch_msssim forms it
        ssum += (double)s;
        if (g.nmaps) {
            const float ia1 = 1.f / a1, ib1 = 1.f / b1, ia2 = 1.f / a2, ib2 = 1.f / b2;
            const size_t q = (size_t)plane * plane_px + (size_t)y * g.Wo + x;
            maps[q] = s * (2.f * muy * ia1 - 2.f * mux * ib1 - 2.f * muy * ia2 + 2.f * mux * ib2);    // dS/dmu_x
            maps[g.map_stride + q] = -s * ib2;                                                          // dS/dE[x^2]
            maps[2 * g.map_stride + q] = 2.f * s * ia2;                                                 // dS/dE[xy]
            if (g.nmaps == 4)
                maps[3 * g.map_stride + q] = s * (2.f * mux * ia1 - 2.f * muy * ib1 - 2.f * mux * ia2 + 2.f * muy * ib2);
        }
    }
    const double t = block_sum(ssum, ws);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// per-plane means -> cs (double, in `saved`), then the requested output.  Wave w sums planes 8w .. 8w + 7, then 32 on.
// The relu clips what compares <= 0, so a NaN mean reaches the output (the training step's NaN skip reads it).
__global__ __launch_bounds__(RT) void k_ssim_reduce(int images, int channels, int tiles, double inv_count, int flags,
                                                    const double *__restrict__ part, double *__restrict__ cs,
                                                    float *__restrict__ out) {
    constexpr int U = 8;  // planes per wave and trip: their loads are in flight together
    const int planes = images * channels, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int p0 = wave * U; p0 < planes; p0 += (RT / 64) * U) {
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = 0.0;
        for (int i = lane; i < tiles; i += 64)
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (p0 + u < planes) v[u] += part[(size_t)(p0 + u) * tiles + i];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v[u] += __shfl_down(v[u], o, 64);
            if (lane == 0 && p0 + u < planes) cs[p0 + u] = v[u] * inv_count;
        }
    }
    __syncthreads();
    const bool relu = flags & FGS_SSIM_NONNEGATIVE;
    if (flags & FGS_SSIM_PER_IMAGE) {
        for (int b = threadIdx.x; b < images; b += RT) {
            double v = 0.0;
            for (int c = 0; c < channels; ++c) {
                const double s = cs[b * channels + c];
                v += (relu && s <= 0.0) ? 0.0 : s;  // (as torch.relu: a NaN mean stays NaN)
            }
            out[b] = (float)(v / channels);
        }
    } else {  // thread t sums planes t, t + RT, ... in order, then the threads in a fixed order: no serial chain of loads
        double v = 0.0;
        for (int p = threadIdx.x; p < planes; p += RT) v += (relu && cs[p] <= 0.0) ? 0.0 : cs[p];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        __shared__ double ws[RT / 64];
        if (lane == 0) ws[wave] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int w = 0; w < RT / 64; ++w) t += ws[w];
            out[0] = (float)(t / planes);
        }
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------
// taps reversed on the host: G(p) = sum_k w[k] M(p - k) = sum_k wr[k] M(p - (n - 1) + k), a valid correlation of the map
// region that starts n - 1 rows / columns before the tile (zero outside the Ho x Wo map).
template <int NT>
__global__ __launch_bounds__(NTHR) void k_ssim_bwd(Geo g, Taps rtaps, int n_rt, int images, int channels, int flags,
                                                   const float *__restrict__ X, const float *__restrict__ Y,
                                                   const float *__restrict__ maps, const double *__restrict__ cs,
                                                   const float *__restrict__ g_out, float *__restrict__ g_x,
                                                   float *__restrict__ g_y) {
    constexpr int KT = NT ? NT : MAXT;
    constexpr int SR = TH + KT - 1;
    constexpr int IT = stage_trips(KT);
    __shared__ float sst[SR * (TW + KT - 1)]; // one staged map at a time
    __shared__ float sh[4][SR * TW];          // horizontal results of every map
    const int n = NT ? NT : n_rt;
    const int tiles_x = (g.W + TW - 1) / TW, tiles = tiles_x * ((g.H + TH - 1) / TH);
    const int plane = blockIdx.x / tiles, tile = blockIdx.x - plane * tiles;
    const int r0 = (tile / tiles_x) * TH, c0 = (tile % tiles_x) * TW;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int x = c0 + tx;
    const size_t poff = (size_t)plane * g.H * g.W;
    // the plane's weight in the loss: d loss / d cs[plane] (mean over the batch or over the channels, relu mask) / count
    const bool per_image = flags & FGS_SSIM_PER_IMAGE;
    const float gsel = g_out[per_image ? plane / channels : 0];
    const double cval = cs[plane];
    const bool live = !((flags & FGS_SSIM_NONNEGATIVE) && cval <= 0.0);  // (a NaN mean is not clipped: relu'(NaN) = 1 in torch)
    const float s = live ? (float)((double)gsel / ((per_image ? (double)channels : (double)images * channels) *
                                                  (double)g.Ho * (double)g.Wo)) : 0.0f;
    if (!live) {  // a clipped plane: its gradient is exactly zero (block-uniform branch)
        for (int o = 0; o < RPT; ++o) {
            const int y = r0 + ty * RPT + o;
            if (y >= g.H || x >= g.W) continue;
            if (g_x) g_x[poff + (size_t)y * g.W + x] = 0.f;
            if (g_y) g_y[poff + (size_t)y * g.W + x] = 0.f;
        }
        return;
    }
    const int nm = g_y ? 4 : 3;  // dX alone reads maps 0..2
    const int rows = TH + n - 1, sp = TW + n - 1;
    const size_t plane_px = (size_t)g.Ho * g.Wo;
    // every global load up front: the four maps' staging, and X / Y of this thread's output pixels
    float vm[4][IT];
#pragma unroll
    for (int m = 0; m < 4; ++m)
        if (m < nm) stage_load(vm[m], maps + m * g.map_stride + (size_t)plane * plane_px, g.Ho, g.Wo, r0 - (n - 1), c0 - (n - 1), n);
    float xv[RPT], yv[RPT];
#pragma unroll
    for (int o = 0; o < RPT; ++o) {
        const int y = r0 + ty * RPT + o;
        const bool in = y < g.H && x < g.W;
        xv[o] = in ? X[poff + (size_t)y * g.W + x] : 0.f;
        yv[o] = in ? Y[poff + (size_t)y * g.W + x] : 0.f;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (m >= nm) break;
        stage_store(sst, vm[m], n);
        __syncthreads();
        for (int i = threadIdx.x; i < rows * TW; i += NTHR) {
            const int rr = i >> 6, cc = i & 63;
            const float *p = sst + rr * sp + cc;
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                if (NT == 0 && k >= n) break;
                a += rtaps.w[k] * p[k];
            }
            sh[m][i] = a;
        }
        __syncthreads();  // the staging buffer is refilled by the next map
    }
    float acc[RPT][4];
#pragma unroll
    for (int o = 0; o < RPT; ++o)
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[o][m] = 0.f;
#pragma unroll
    for (int j = 0; j < RPT + KT - 1; ++j) {
        if (NT == 0 && j >= RPT + n - 1) break;
        const int idx = (ty * RPT + j) * TW + tx;
        float v[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) v[m] = (m < nm) ? sh[m][idx] : 0.f;
#pragma unroll
        for (int o = 0; o < RPT; ++o) {
            const int k = j - o;
            if (k < 0 || k >= KT || (NT == 0 && k >= n)) continue;
            const float w = rtaps.w[k];
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[o][m] += w * v[m];
        }
    }
#pragma unroll
    for (int o = 0; o < RPT; ++o) {
        const int y = r0 + ty * RPT + o;
        if (y >= g.H || x >= g.W) continue;
        const size_t q = poff + (size_t)y * g.W + x;
        if (g_x) g_x[q] = s * (acc[o][0] + 2.f * xv[o] * acc[o][1] + yv[o] * acc[o][2]);
        if (g_y) g_y[q] = s * (acc[o][3] + 2.f * yv[o] * acc[o][1] + xv[o] * acc[o][2]);
    }
}

}  // namespace

extern "C" {

int fgs_ssim_workspace_bytes(const FgsSsimDims *dims, size_t *saved_bytes, size_t *scratch_bytes) {
    Geo g;
    if (int rc = make_geo(dims, &g, "fgs_ssim_workspace_bytes")) return rc;
    if (saved_bytes) *saved_bytes = cs_bytes(g) + (size_t)g.nmaps * g.map_stride * sizeof(float);
    if (scratch_bytes) *scratch_bytes = align256((size_t)g.planes * g.tiles_x * g.tiles_y * sizeof(double));
    return FGS_OK;
}

int fgs_ssim_forward(const FgsSsimDims *dims, const float *x, const float *y, float *out, void *saved, void *scratch,
                     void *stream) {
    Geo g;
    if (int rc = make_geo(dims, &g, "fgs_ssim_forward")) return rc;
    if (!x || !y || !out || !saved || !scratch) {
        fgs_set_error("fgs_ssim_forward: null pointer");
        return FGS_EINVAL;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    Taps t;
    for (int k = 0; k < MAXT; ++k) t.w[k] = k < dims->num_taps ? dims->taps[k] : 0.0f;
    double *cs = reinterpret_cast<double *>(saved);
    float *maps = reinterpret_cast<float *>(reinterpret_cast<char *>(saved) + cs_bytes(g));
    double *part = reinterpret_cast<double *>(scratch);
    const int tiles = g.tiles_x * g.tiles_y;
    const dim3 grid((unsigned)((size_t)g.planes * tiles));
    if (dims->num_taps == 11)
        hipLaunchKernelGGL(k_ssim_fwd<11>, grid, dim3(NTHR), 0, st, g, t, 11, dims->c1, dims->c2, x, y, maps, part);
    else
        hipLaunchKernelGGL(k_ssim_fwd<0>, grid, dim3(NTHR), 0, st, g, t, dims->num_taps, dims->c1, dims->c2, x, y, maps,
                           part);
    FGS_LAUNCH_CHECK("k_ssim_fwd");
    hipLaunchKernelGGL(k_ssim_reduce, dim3(1), dim3(RT), 0, st, dims->images, dims->channels, tiles,
                       1.0 / ((double)g.Ho * (double)g.Wo), dims->flags, part, cs, out);
    FGS_LAUNCH_CHECK("k_ssim_reduce");
    return FGS_OK;
}

int fgs_ssim_backward(const FgsSsimDims *dims, const float *x, const float *y, const void *saved, const float *g_out,
                      float *g_x, float *g_y, void *scratch, void *stream) {
    (void)scratch;  // the backward needs no scratch: the per-plane weights are derived in every block from `saved`
    Geo g;
    if (int rc = make_geo(dims, &g, "fgs_ssim_backward")) return rc;
    if (!x || !y || !saved || !g_out || (!g_x && !g_y)) {
        fgs_set_error("fgs_ssim_backward: null pointer");
        return FGS_EINVAL;
    }
    if ((g_y && g.nmaps < 4) || (g_x && g.nmaps < 3)) {
        fgs_set_error("fgs_ssim_backward: the forward saved no factor maps for the requested gradient (flags %d)", dims->flags);
        return FGS_EINVAL;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int n = dims->num_taps;
    Taps rt;
    for (int k = 0; k < MAXT; ++k) rt.w[k] = k < n ? dims->taps[n - 1 - k] : 0.0f;
    const double *cs = reinterpret_cast<const double *>(saved);
    const float *maps = reinterpret_cast<const float *>(reinterpret_cast<const char *>(saved) + cs_bytes(g));
    const dim3 grid((unsigned)((size_t)g.planes * ((g.W + TW - 1) / TW) * ((g.H + TH - 1) / TH)));
    if (n == 11)
        hipLaunchKernelGGL(k_ssim_bwd<11>, grid, dim3(NTHR), 0, st, g, rt, 11, dims->images, dims->channels, dims->flags,
                           x, y, maps, cs, g_out, g_x, g_y);
    else
        hipLaunchKernelGGL(k_ssim_bwd<0>, grid, dim3(NTHR), 0, st, g, rt, n, dims->images, dims->channels, dims->flags,
                           x, y, maps, cs, g_out, g_x, g_y);
    FGS_LAUNCH_CHECK("k_ssim_bwd");
    return FGS_OK;
}

}  // extern "C"
