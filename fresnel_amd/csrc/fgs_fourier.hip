// FourierGaussianRenderer (fgs_fourier_*; DR:1500-1774): a dense, order-independent sum of ISOTROPIC Gaussians over the whole
// frame, normalised by the per-image maximum and composed with the background.  No bbox, no sort, no lists.
//
// The footprint factors, exp(-((x-u)^2 + (y-v)^2)/s) = Gx[i][x] Gy[i][y], so one channel of the accumulated image is a matrix
// product over the Gaussian index,
//     F_c (H x W) = Gy^T (H x N) diag(w_c) Gx (N x W),      w_c = colour_c x opacity,
// and runs on the fp32-input matrix cores (v_mfma_f32_32x32x2_f32: products and sums are fp32 FMA chains, exact fp32).  The
// backward has the same shape: P_ck (H x N) = E_c (H x W) (Gx dx^k)^T for k = 0, 1, 2 on the matrix cores, then a contraction
// of P with Gy, Gy dy, Gy dy^2 over the rows gives every Gaussian's dL/dw_c and the moments behind dL/du, dL/dv, dL/ds.
// The factor tables are built per K-chunk in LDS; nothing of size N x (H + W) goes to HBM.
//
// Compiled with -ffp-contract=off: forward and backward recompute the per-pixel chain (divide by the maximum, background
// weight, clamps) with the same roundings, so the backward's clamp masks are the forward's.  The MFMAs are unaffected.
//
// `saved` (const through the backward):  rec  float [B][N][8]   u, v, 1/s, w_r, w_g, w_b, visible (uint32), opacity
//                                        F    float [B][3][H][W] the un-normalised accumulation
//                                        scal       [B][2]       per image: the maximum m (float), its flat index in
//                                                                (3, H, W) (uint32; ties: the lowest index)
// `scratch`: per-block maxima, the gradient image E, the partial sums of sum(g F), the per-Gaussian sums.
#include "fgs_internal.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int FR = FGS_FOURIER_REC_FLOATS;
constexpr int FT = 64;   // forward: output tile edge of a block (2 x 2 waves of 32 x 32)
constexpr int KC = 32;   // forward: Gaussians per K-chunk
constexpr int BG = 32;   // backward: Gaussians per block (the columns of its MFMA tiles)
constexpr int BT = 32;   // backward: rows per y-tile and columns per x-chunk of E
constexpr int RB = 32;   // backward: blocks per image of the sum(g F) reduction

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct FourierPlan {
    FgsFourierDims d;
    size_t HW, tiles;
    size_t v_rec, v_F, v_scal, v_total;
    size_t c_part, c_E, c_psum, c_rows, c_total;
};

int make_fourier_plan(const FgsFourierDims *d, FourierPlan *p) {
    if (!d) { fgs_set_error("null dims"); return FGS_EINVAL; }
    if (d->batch < 1 || d->batch > 65535 || d->num_gaussians < 1 || d->width < 1 || d->height < 1 || d->width > 16384 ||
        d->height > 16384 || (d->num_cameras != 1 && d->num_cameras != d->batch) ||
        !(d->background[0] == d->background[0]) || !(d->background[1] == d->background[1]) ||
        !(d->background[2] == d->background[2])) {
        fgs_set_error("invalid Fourier dims: B=%d N=%d W=%d H=%d num_cameras=%d", d->batch, d->num_gaussians, d->width,
                      d->height, d->num_cameras);
        return FGS_EINVAL;
    }
    const size_t B = (size_t)d->batch, N = (size_t)d->num_gaussians, HW = (size_t)d->width * (size_t)d->height;
    if (B * N >= (1ull << 27)) { fgs_set_error("B*N too large"); return FGS_EINVAL; }
    if (3 * HW >= (1ull << 31) || B * 3 * HW >= (1ull << 40)) { fgs_set_error("frame too large"); return FGS_EINVAL; }
    p->d = *d;
    p->HW = HW;
    p->tiles = (size_t)((d->width + FT - 1) / FT) * (size_t)((d->height + FT - 1) / FT);
    if (p->tiles > 65535) { fgs_set_error("frame too large"); return FGS_EINVAL; }
    size_t o = 0;
    p->v_rec = o; o = align256(o + B * N * FR * 4);
    p->v_F = o; o = align256(o + B * 3 * HW * 4);
    p->v_scal = o; o = align256(o + B * 2 * 4);
    p->v_total = o;
    o = 0;
    p->c_part = o; o = align256(o + B * p->tiles * 8);
    p->c_E = o; o = align256(o + B * 3 * HW * 4);
    p->c_psum = o; o = align256(o + B * RB * 8);
    p->c_rows = o; o = align256(o + B * N * 12 * 4);
    p->c_total = o;
    return FGS_OK;
}

// ---- maximum with arg-max, ties to the lowest flat index ----
__device__ __forceinline__ void best_merge(float &v, uint32_t &i, float ov, uint32_t oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
// block of 256 threads; the result is valid in every thread
__device__ __forceinline__ void best_block(float &v, uint32_t &i) {
    __shared__ float sv[4];
    __shared__ uint32_t si[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const uint32_t oi = (uint32_t)__shfl_xor((int)i, o, 64);
        best_merge(v, i, ov, oi);
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) { sv[wave] = v; si[wave] = i; }
    __syncthreads();
    v = sv[0]; i = si[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) best_merge(v, i, sv[w], si[w]);
}

// ---- forward product: F_c = Gy^T diag(w_c) Gx ----
// grid (tiles_x, tiles_y, B), 256 threads: a block owns a 64 x 64 tile of the frame, wave (wy, wx) its 32 x 32 quarter with
// one accumulator per channel.  Per chunk of KC Gaussians the block builds Gy[k][64 rows] and Gx[k][64 columns] in LDS (zero
// for culled Gaussians, the tail of N and pixels outside the frame), then every wave issues KC / 2 x 3 MFMAs:
// A[i = row][k] = Gy (shared by the channels), B[k][j = column] = w_c Gx.
__global__ __launch_bounds__(256) void k_fourier_fwd(int32_t N, int32_t W, int32_t H, const float *__restrict__ frec,
                                                     float *__restrict__ F, float2 *__restrict__ part) {
    __shared__ float sGy[KC][FT], sGx[KC][FT], sRec[KC][FR];
    const int32_t b = blockIdx.z, x0 = blockIdx.x * FT, y0 = blockIdx.y * FT;
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wx = wave & 1, wy = wave >> 1;
    const int32_t l31 = lane & 31, lh = lane >> 5;
    const float *__restrict__ rec = frec + (size_t)b * N * FR;
    f32x16 acc0, acc1, acc2;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; acc2[r] = 0.0f; }
    // thread -> one pixel coordinate of the tile (64 rows, then 64 columns) and every second Gaussian of the chunk
    const int32_t q = threadIdx.x & (2 * FT - 1), kpar = threadIdx.x >> 7;
    const bool isx = q >= FT;
    const int32_t px = isx ? x0 + q - FT : y0 + q;
    const bool inside = px < (isx ? W : H);
    for (int32_t k0 = 0; k0 < N; k0 += KC) {
        {   // the chunk's records: one coalesced load, one word per thread (zeros behind the tail of N: culled)
            const size_t word = (size_t)k0 * FR + threadIdx.x;
            (&sRec[0][0])[threadIdx.x] = word < (size_t)N * FR ? rec[word] : 0.0f;
        }
        __syncthreads();
#pragma unroll 4
        for (int32_t k = kpar; k < KC; k += 2) {
            const float dd = (float)px - sRec[k][isx ? FR_U : FR_V];
            const float val = (inside && __float_as_uint(sRec[k][FR_VIS]) != 0u) ? expf(-(dd * dd) * sRec[k][FR_IS]) : 0.0f;
            if (isx) sGx[k][q - FT] = val; else sGy[k][q] = val;
        }
        __syncthreads();
#pragma unroll 4
        for (int32_t kk = 0; kk < KC; kk += 2) {
            const int32_t k = kk + lh;
            const float a = sGy[k][wy * 32 + l31], gx = sGx[k][wx * 32 + l31];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, sRec[k][FR_WR] * gx, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, sRec[k][FR_WG] * gx, acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, sRec[k][FR_WB] * gx, acc2, 0, 0, 0);
        }
        __syncthreads();  // the records and factors may be overwritten
    }
    // C layout: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int32_t x = x0 + wx * 32 + l31;
    const size_t HW = (size_t)W * H;
    float *__restrict__ Fb = F + (size_t)b * 3 * HW;
    float bv = -INFINITY;
    uint32_t bi = 0xFFFFFFFFu;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int32_t y = y0 + wy * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (x < W && y < H) {
            const uint32_t pix = (uint32_t)y * (uint32_t)W + (uint32_t)x;
            Fb[pix] = acc0[r]; Fb[HW + pix] = acc1[r]; Fb[2 * HW + pix] = acc2[r];
            best_merge(bv, bi, acc0[r], pix);
            best_merge(bv, bi, acc1[r], (uint32_t)HW + pix);
            best_merge(bv, bi, acc2[r], 2u * (uint32_t)HW + pix);
        }
    }
    best_block(bv, bi);
    if (threadIdx.x == 0)
        part[(size_t)b * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] = make_float2(bv, __uint_as_float(bi));
}

// ---- per-pixel chain of DR:1741-1751 and its adjoint ----
struct Pix { float pre[3], d; bool norm; };
__device__ __forceinline__ float clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }  // NaN stays NaN
__device__ __forceinline__ void pixel_chain(const float f[3], float m, const float bg[3], Pix &o) {
    o.norm = m > 1e-8f;
    const float fn0 = o.norm ? f[0] / m : f[0], fn1 = o.norm ? f[1] / m : f[1], fn2 = o.norm ? f[2] / m : f[2];
    o.d = 1.0f - ((fn0 + fn1) + fn2);
    const float bgw = clamp01(o.d);
    o.pre[0] = fn0 + bg[0] * bgw; o.pre[1] = fn1 + bg[1] * bgw; o.pre[2] = fn2 + bg[2] * bgw;
}
// gradient w.r.t. the normalised image; both clamps pass it on the closed interval
__device__ __forceinline__ void pixel_adjoint(const Pix &o, const float g[3], const float bg[3], float gfn[3]) {
    float gp[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) gp[c] = (o.pre[c] >= 0.0f && o.pre[c] <= 1.0f) ? g[c] : 0.0f;
    const float gbgw = (gp[0] * bg[0] + gp[1] * bg[1]) + gp[2] * bg[2];
    const float gtot = (o.d >= 0.0f && o.d <= 1.0f) ? -gbgw : 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) gfn[c] = gp[c] + gtot;
}

// grid (ceil(HW / 256), B).  Every block folds the image's per-tile maxima (a few words), block 0 records the result in
// `saved`; then normalisation, background, clamp.
__global__ __launch_bounds__(256) void k_fourier_output(uint32_t HW, uint32_t tiles, float bg0, float bg1, float bg2,
                                                        const float2 *__restrict__ part, const float *__restrict__ F,
                                                        float *__restrict__ scal, float *__restrict__ out) {
    const uint32_t b = blockIdx.y;
    float m = -INFINITY;
    uint32_t mi = 0xFFFFFFFFu;
    for (uint32_t j = threadIdx.x; j < tiles; j += 256) {
        const float2 t = part[(size_t)b * tiles + j];
        best_merge(m, mi, t.x, __float_as_uint(t.y));
    }
    best_block(m, mi);
    if (blockIdx.x == 0 && threadIdx.x == 0) { scal[2 * b] = m; scal[2 * b + 1] = __uint_as_float(mi); }
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const float *__restrict__ Fb = F + (size_t)b * 3 * HW;
    const float f[3] = {Fb[p], Fb[HW + p], Fb[2 * (size_t)HW + p]}, bg[3] = {bg0, bg1, bg2};
    Pix o;
    pixel_chain(f, m, bg, o);
    float *__restrict__ ob = out + (size_t)b * 3 * HW;
    ob[p] = clamp01(o.pre[0]); ob[HW + p] = clamp01(o.pre[1]); ob[2 * (size_t)HW + p] = clamp01(o.pre[2]);
}

// ---- backward, image part ----
// S = sum over the image of gfn F (the gradient that reaches the maximum is -S / m^2): RB block partials per image in double,
// fixed order.  grid (RB, B).
__global__ __launch_bounds__(256) void k_fourier_gsum(uint32_t HW, float bg0, float bg1, float bg2,
                                                      const float *__restrict__ F, const float *__restrict__ scal,
                                                      const float *__restrict__ g_rgb, double *__restrict__ psum) {
    const uint32_t b = blockIdx.y;
    const float m = scal[2 * b], bg[3] = {bg0, bg1, bg2};
    const float *__restrict__ Fb = F + (size_t)b * 3 * HW, *__restrict__ gb = g_rgb + (size_t)b * 3 * HW;
    double s = 0.0;
    for (uint32_t p = blockIdx.x * 256 + threadIdx.x; p < HW; p += RB * 256) {
        const float f[3] = {Fb[p], Fb[HW + p], Fb[2 * (size_t)HW + p]}, g[3] = {gb[p], gb[HW + p], gb[2 * (size_t)HW + p]};
        Pix o;
        float gfn[3];
        pixel_chain(f, m, bg, o);
        pixel_adjoint(o, g, bg, gfn);
        s += ((double)gfn[0] * f[0] + (double)gfn[1] * f[1]) + (double)gfn[2] * f[2];
    }
    __shared__ double sd[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63u) == 0) sd[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) psum[b * RB + blockIdx.x] = (sd[0] + sd[1]) + (sd[2] + sd[3]);
}

// E = dL/dF: gfn / m plus, on the arg-max element, -S / m^2; gfn itself where the image was not normalised (m <= 1e-8).
// grid (ceil(HW / 256), B).
__global__ __launch_bounds__(256) void k_fourier_grad_image(uint32_t HW, float bg0, float bg1, float bg2,
                                                            const float *__restrict__ F, const float *__restrict__ scal,
                                                            const double *__restrict__ psum, const float *__restrict__ g_rgb,
                                                            float *__restrict__ E) {
    const uint32_t b = blockIdx.y;
    const float m = scal[2 * b], bg[3] = {bg0, bg1, bg2};
    const uint32_t mi = __float_as_uint(scal[2 * b + 1]);
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const float *__restrict__ Fb = F + (size_t)b * 3 * HW, *__restrict__ gb = g_rgb + (size_t)b * 3 * HW;
    const float f[3] = {Fb[p], Fb[HW + p], Fb[2 * (size_t)HW + p]}, g[3] = {gb[p], gb[HW + p], gb[2 * (size_t)HW + p]};
    Pix o;
    float gfn[3];
    pixel_chain(f, m, bg, o);
    pixel_adjoint(o, g, bg, gfn);
    float *__restrict__ Eb = E + (size_t)b * 3 * HW;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float e = o.norm ? gfn[c] / m : gfn[c];
        if (o.norm && mi == (uint32_t)c * HW + p) {
            double s = 0.0;
            for (int j = 0; j < RB; ++j) s += psum[b * RB + j];
            e += (float)(-s / ((double)m * (double)m));
        }
        Eb[(size_t)c * HW + p] = e;
    }
}

// ---- backward product and contraction ----
// grid (ceil(N / BG), B), 192 threads: a block owns BG Gaussians for the WHOLE frame (no atomics, one fixed summation order),
// wave c channel c.  Per y-tile of BT rows the wave accumulates P_k[row][Gaussian] = sum_x E_c[row][x] Gx[g][x] dx^k, k = 0, 1, 2,
// over x-chunks of BT columns: A[i = row][k = x] = E_c from an LDS tile, B[k = x][j = Gaussian] = Gx dx^k from an LDS table the
// three waves share.  The accumulator layout puts the Gaussian on the lane and 16 rows in the registers, so the contraction
// with Gy, Gy dy, Gy dy^2 over the rows is a per-lane loop; the two half-waves are combined by one shuffle at the end.
__global__ __launch_bounds__(192) void k_fourier_bwd(int32_t N, int32_t W, int32_t H, const float *__restrict__ frec,
                                                     const float *__restrict__ E, float *__restrict__ sums) {
    __shared__ float sE[3][BT][BT + 1];
    __shared__ float sGx[BT][BG];
    __shared__ float sM[3][BG][5];
    __shared__ float sRec[BG][FR];
    const int32_t b = blockIdx.y, g0 = blockIdx.x * BG;
    const int32_t lane = threadIdx.x & 63, c = threadIdx.x >> 6, l31 = lane & 31, lh = lane >> 5;
    const float *__restrict__ rec = frec + (size_t)b * N * FR;
    const int32_t g = g0 + l31;
    for (int32_t e = threadIdx.x; e < BG * FR; e += 192) {  // the block's records (zeros behind the tail of N: culled)
        const size_t word = (size_t)g0 * FR + e;
        (&sRec[0][0])[e] = word < (size_t)N * FR ? rec[word] : 0.0f;
    }
    __syncthreads();
    // a culled Gaussian's record is all zeros: zero Gx rows (by the flag), finite Gy
    const float u = sRec[l31][FR_U], v = sRec[l31][FR_V], is = sRec[l31][FR_IS];
    const float *__restrict__ Ec = E + ((size_t)b * 3 + c) * (size_t)W * H;
    float m00 = 0.0f, m01 = 0.0f, m02 = 0.0f, m10 = 0.0f, m20 = 0.0f;
    for (int32_t y0 = 0; y0 < H; y0 += BT) {
        f32x16 p0, p1, p2;
#pragma unroll
        for (int r = 0; r < 16; ++r) { p0[r] = 0.0f; p1[r] = 0.0f; p2[r] = 0.0f; }
        // this wave's E tile: column l31, rows lh, lh + 2, ...; the next tile is loaded while the MFMAs of this one run
        float et[BT / 2];
        auto load_tile = [&](int32_t x0) {
#pragma unroll
            for (int j = 0; j < BT / 2; ++j) {
                const int32_t y = y0 + lh + 2 * j, x = x0 + l31;
                et[j] = (y < H && x < W) ? Ec[(size_t)y * W + x] : 0.0f;
            }
        };
        load_tile(0);
        for (int32_t x0 = 0; x0 < W; x0 += BT) {
            __syncthreads();  // the previous chunk's operands have been read
#pragma unroll
            for (int j = 0; j < BT / 2; ++j) sE[c][lh + 2 * j][l31] = et[j];
            for (int32_t e = threadIdx.x; e < BT * BG; e += 192) {
                const int32_t xx = e / BG, gg = e % BG, x = x0 + xx;
                const float dd = (float)x - sRec[gg][FR_U];
                sGx[xx][gg] = (x < W && __float_as_uint(sRec[gg][FR_VIS]) != 0u) ? expf(-(dd * dd) * sRec[gg][FR_IS]) : 0.0f;
            }
            __syncthreads();
            if (x0 + BT < W) load_tile(x0 + BT);
#pragma unroll 4
            for (int32_t kk = 0; kk < BT; kk += 2) {
                const int32_t kx = kk + lh;
                const float a = sE[c][l31][kx], gx = sGx[kx][l31];
                const float dx = (float)(x0 + kx) - u, b1 = gx * dx, b2 = b1 * dx;
                p0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, gx, p0, 0, 0, 0);
                p1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, p1, 0, 0, 0);
                p2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b2, p2, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int32_t y = y0 + (r & 3) + 8 * (r >> 2) + 4 * lh;  // (rows beyond the frame: P is zero there)
            const float dy = (float)y - v, gy = expf(-(dy * dy) * is), gyd = gy * dy;
            m00 += gy * p0[r]; m01 += gyd * p0[r]; m02 += (gyd * dy) * p0[r];
            m10 += gy * p1[r]; m20 += gy * p2[r];
        }
    }
    m00 += __shfl_xor(m00, 32, 64); m01 += __shfl_xor(m01, 32, 64); m02 += __shfl_xor(m02, 32, 64);
    m10 += __shfl_xor(m10, 32, 64); m20 += __shfl_xor(m20, 32, 64);
    if (lh == 0) { sM[c][l31][0] = m00; sM[c][l31][1] = m01; sM[c][l31][2] = m02; sM[c][l31][3] = m10; sM[c][l31][4] = m20; }
    __syncthreads();
    if (threadIdx.x < BG && g < N) {
        // G = exp(-(dx^2 + dy^2) / s), T = sum_c w_c E_c: dL/du = 2 / s sum T G dx, dL/ds = 1 / s^2 sum T G (dx^2 + dy^2)
        float su = 0.0f, sv = 0.0f, sr = 0.0f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float w = sRec[l31][FR_WR + ch];
            su += w * sM[ch][l31][3]; sv += w * sM[ch][l31][1]; sr += w * (sM[ch][l31][4] + sM[ch][l31][2]);
        }
        float4 *o = reinterpret_cast<float4 *>(sums + ((size_t)b * N + g) * 12);
        o[0] = make_float4((2.0f * is) * su, (2.0f * is) * sv, (is * is) * sr, sM[0][l31][0]);
        o[1] = make_float4(sM[1][l31][0], sM[2][l31][0], 0.0f, 0.0f);
        o[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

}  // namespace

extern "C" {

int fgs_fourier_workspace_bytes(const FgsFourierDims *dims, size_t *saved_bytes, size_t *scratch_bytes) {
    FourierPlan p;
    const int rc = make_fourier_plan(dims, &p);
    if (rc) return rc;
    if (saved_bytes) *saved_bytes = p.v_total;
    if (scratch_bytes) *scratch_bytes = p.c_total;
    return FGS_OK;
}

int fgs_fourier_forward(const FgsFourierDims *dims, const float *cameras, const float *pos, const float *scale,
                        const float *quat, const float *color, const float *opacity, float *out_rgb, void *saved,
                        void *scratch, void *stream) {
    FourierPlan p;
    int rc = make_fourier_plan(dims, &p);
    if (rc) return rc;
    const void *ptrs[] = {cameras, pos, scale, quat, color, opacity, out_rgb, saved, scratch};
    for (int i = 0; i < 9; ++i)
        if (!ptrs[i]) { fgs_set_error("fgs_fourier_forward: null pointer argument #%d", i); return FGS_EINVAL; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char *sv = reinterpret_cast<char *>(saved), *sc = reinterpret_cast<char *>(scratch);
    const int32_t B = p.d.batch, N = p.d.num_gaussians, W = p.d.width, H = p.d.height;
    float *rec = reinterpret_cast<float *>(sv + p.v_rec), *F = reinterpret_cast<float *>(sv + p.v_F);
    float2 *part = reinterpret_cast<float2 *>(sc + p.c_part);
    fgs_stage_begin(ST_PROJECT, st);
    if ((rc = fgs_launch_fourier_project(B, N, W, H, p.d.num_cameras, cameras, pos, scale, quat, color, opacity, rec, st)))
        return rc;
    fgs_stage_end(ST_PROJECT, st);
    fgs_stage_begin(ST_SPLAT_FWD, st);
    hipLaunchKernelGGL(k_fourier_fwd, dim3((unsigned)((W + FT - 1) / FT), (unsigned)((H + FT - 1) / FT), (unsigned)B),
                       dim3(256), 0, st, N, W, H, rec, F, part);
    FGS_LAUNCH_CHECK("k_fourier_fwd");
    fgs_stage_end(ST_SPLAT_FWD, st);
    fgs_stage_begin(ST_FIELD_FWD, st);
    hipLaunchKernelGGL(k_fourier_output, dim3((unsigned)((p.HW + 255) / 256), (unsigned)B), dim3(256), 0, st,
                       (uint32_t)p.HW, (uint32_t)p.tiles, p.d.background[0], p.d.background[1], p.d.background[2], part, F,
                       reinterpret_cast<float *>(sv + p.v_scal), out_rgb);
    FGS_LAUNCH_CHECK("k_fourier_output");
    fgs_stage_end(ST_FIELD_FWD, st);
    return FGS_OK;
}

int fgs_fourier_backward(const FgsFourierDims *dims, const float *cameras, const float *pos, const float *scale,
                         const float *quat, const float *color, const float *opacity, const void *saved, void *scratch,
                         const float *g_rgb, float *g_pos, float *g_scale, float *g_quat, float *g_color,
                         float *g_opacity, void *stream) {
    FourierPlan p;
    int rc = make_fourier_plan(dims, &p);
    if (rc) return rc;
    const void *ptrs[] = {cameras, pos, scale, quat, color, opacity, saved, scratch, g_rgb, g_pos, g_scale, g_quat, g_color,
                          g_opacity};
    for (int i = 0; i < 14; ++i)
        if (!ptrs[i]) { fgs_set_error("fgs_fourier_backward: null pointer argument #%d", i); return FGS_EINVAL; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const char *sv = reinterpret_cast<const char *>(saved);
    char *sc = reinterpret_cast<char *>(scratch);
    const int32_t B = p.d.batch, N = p.d.num_gaussians, W = p.d.width, H = p.d.height;
    const float *rec = reinterpret_cast<const float *>(sv + p.v_rec), *F = reinterpret_cast<const float *>(sv + p.v_F);
    const float *scal = reinterpret_cast<const float *>(sv + p.v_scal);
    float *E = reinterpret_cast<float *>(sc + p.c_E), *rows = reinterpret_cast<float *>(sc + p.c_rows);
    double *psum = reinterpret_cast<double *>(sc + p.c_psum);
    const float *bg = p.d.background;
    fgs_stage_begin(ST_FIELD_BWD, st);
    hipLaunchKernelGGL(k_fourier_gsum, dim3(RB, (unsigned)B), dim3(256), 0, st, (uint32_t)p.HW, bg[0], bg[1], bg[2], F, scal,
                       g_rgb, psum);
    FGS_LAUNCH_CHECK("k_fourier_gsum");
    hipLaunchKernelGGL(k_fourier_grad_image, dim3((unsigned)((p.HW + 255) / 256), (unsigned)B), dim3(256), 0, st,
                       (uint32_t)p.HW, bg[0], bg[1], bg[2], F, scal, psum, g_rgb, E);
    FGS_LAUNCH_CHECK("k_fourier_grad_image");
    fgs_stage_end(ST_FIELD_BWD, st);
    fgs_stage_begin(ST_SPLAT_BWD, st);
    hipLaunchKernelGGL(k_fourier_bwd, dim3((unsigned)((N + BG - 1) / BG), (unsigned)B), dim3(192), 0, st, N, W, H, rec, E,
                       rows);
    FGS_LAUNCH_CHECK("k_fourier_bwd");
    fgs_stage_end(ST_SPLAT_BWD, st);
    fgs_stage_begin(ST_PROJECT_BWD, st);
    if ((rc = fgs_launch_fourier_project_bwd(B, N, p.d.num_cameras, cameras, pos, scale, quat, color, rec, rows, g_pos,
                                             g_scale, g_quat, g_color, g_opacity, st)))
        return rc;
    fgs_stage_end(ST_PROJECT_BWD, st);
    return FGS_OK;
}

}  // extern "C"
