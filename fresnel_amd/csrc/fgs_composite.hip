// Stage 3: front-to-back per-pixel alpha compositing, forward and backward.
// Replaces the reference's per-Gaussian Python loop (DR:582-667) and its autograd replay.
//
// Work decomposition (CDNA4, wave64): ONE WAVE owns one 16x16 tile of one image.  The tile is
// cut into four 8x8 sub-tiles; lane l owns pixel (l&7, l>>3) of EACH sub-tile, so a wave
// instruction covers exactly one sub-tile.  For every Gaussian of the tile's depth-sorted list
// the wave tests the Gaussian's integer bbox against the four sub-tile rectangles with scalar
// code and runs the per-pixel blend only for the sub-tiles it touches (wave-uniform branches:
// no divergence, 8x8 work granularity).  The list is staged through LDS 64 records at a time
// (lane j fetches record j with three 16-byte loads; the loop reads each record back once as
// three wave-uniform ds_read_b128 broadcasts and keeps it in registers across the sub-tiles).
//
// Reference semantics kept exactly: rectangular bbox support (DR:594-600), integer pixel
// coordinates (DR:603-607), alpha clamp [0, 0.99] (DR:647), additive accumulated alpha with
// T = 1 - A (DR:650-658), no early termination.
//
// Bound: VALU + transcendental (about 25 VALU + 1 v_exp_f32 per Gaussian-pixel forward, ~60
// backward); HBM traffic is the 52-byte id+record gather per duplicate plus per-pixel state.
#include <type_traits>
#include "fgs_internal.h"
#include "fgs_wave.h"

#if (defined(FGS_BWD_DYN_LDS) || defined(FGS_BWD_WIDE_WAVES) || defined(FGS_PHASE_SCAN) || defined(FGS_CKPT_NT) || defined(FGS_PHASE_WAVE_BLOCKS) || \
     defined(FGS_BWD_UNIT_TRACE) || defined(FGS_BWD_TILE_ORDER) || defined(FGS_FWD_HEAD_ENTRIES)) && !defined(FGS_EXPERIMENT_BUILD)
#error "work-split / timing switches of this unit are for experiment builds: python -m fresnel_amd.build --define ... (sets FGS_EXPERIMENT_BUILD; fgs_version() then says so)"
#endif

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));
constexpr float FGS_SATURATION_EPS = 2.98023223876953125e-8f;  // 2^-25: 1 - T rounds to 1.0f below it
constexpr float NEG_HALF_LOG2E = -0.72134752044448170368f;  // exp(-m/2) = exp2(m * this)
constexpr float ALPHA_MAX = 0.99f;                          // DR:647
constexpr float INV_ALPHA_MAX = 1.0f / 0.99f;
constexpr float PHASE_KAPPA = 2.0f * 3.14159f;              // DR:642 uses the literal 3.14159

// cos / sin of x = kappa * pd, pd in [0, 0.5], i.e. x in [0, pi]: polynomials in y = x - pi/2 (|y| <= pi/2), all plain FMAs.  The
// hardware v_cos_f32 / v_sin_f32 (__cosf / __sinf) are only good to ~1e-5 absolute, which showed up as 1e-5 image error and > 1e-4
// gradient error at phase_amplitude 0.6.  Round 5: MINIMAX coefficients (fit on [0, (pi/2)^2] in y^2 with the constant term held at
// 1; approximation error 4.8e-9 / 2.4e-10, fp32 evaluation error 1.3e-7 / 1.2e-7 over the interval -- that of the Taylor
// polynomials of degree 11 / 12 they replace) of degree 9 / 10: one FMA less per evaluation, three per list entry of the backward.
__device__ __forceinline__ float phase_cos(float x) {
    const float y = x - 1.57079632679489661923f, y2 = y * y;  // cos(x) = -sin(y),  sin(y) = y (1 + y^2 p(y^2))
    float p = 2.6089300414764439e-6f;
    p = p * y2 - 1.9811111665926607e-4f;
    p = p * y2 + 8.3330881539788702e-3f;
    p = p * y2 - 1.6666660461917662e-1f;
    return -(y + y * (y2 * p));
}
__device__ __forceinline__ float phase_sin(float x) {
    const float y = x - 1.57079632679489661923f, y2 = y * y;  // sin(x) = cos(y) = 1 + y^2 p(y^2)
    float p = -2.6077082524225105e-7f;
    p = p * y2 + 2.4761885011562826e-5f;
    p = p * y2 - 1.3888403485377396e-3f;
    p = p * y2 + 4.1666640726419513e-2f;
    p = p * y2 - 4.9999999549521157e-1f;
    return 1.0f + y2 * p;
}
constexpr int CH = 64;                                      // records per LDS chunk (one per lane)

// The blend kernels' alpha (fgs_internal.h, "opacity fold"): every forward whose checkpoints k_composite_bwd restarts from,
// and the backward itself, form a' = alpha / 0.99 with these two functions, so the backward recomputes the forward's T to the bit.
// lop of a staged opacity >= 0: log2(op / 0.99); -inf for opacity 0 (a' = exp2(-inf) = 0: this unit is built with
// -fno-finite-math-only and must stay so).  Negative and NaN opacities never reach a pass (stage_decode_w).
__device__ __forceinline__ float blend_lop(float opacity) { return __builtin_log2f(opacity / ALPHA_MAX); }
// a' = clamp01(exp2(e)) on the lanes of the mask, e = m' + lop: v_exp_f32 ... clamp (v_med3(x, 0, 1) of the v_exp's result
// folds into its clamp modifier) and one v_and
__device__ __forceinline__ float blend_alpha1(float e, uint32_t mask) {
    return __uint_as_float(__float_as_uint(__builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(e), 0.0f, 1.0f)) & mask);
}

// (x < 1) ? v : 0, the 1.0 an inline constant (1 > x): select_lt (fgs_wave.h) without a VGPR for the limit
__device__ __forceinline__ float select_lt1(float x, float v) {
    float o;
    asm("v_cmp_gt_f32 vcc, 1.0, %1\n\tv_cndmask_b32 %0, 0, %2, vcc" : "=v"(o) : "v"(x), "v"(v) : "vcc");
    return o;
}

struct TileCtx {
    uint32_t tile, b, tx, ty, X0, Y0, start, end;
};

__device__ __forceinline__ TileCtx tile_ctx_of(uint32_t tile, uint32_t tiles, uint32_t tiles_x,
                                               const uint32_t *__restrict__ ranges, uint32_t tile_w = FGS_TILE) {
    TileCtx c;
    c.tile = tile;
    c.b = c.tile / tiles;
    const uint32_t t = c.tile - c.b * tiles;
    c.ty = t / tiles_x;
    c.tx = t - c.ty * tiles_x;
    c.X0 = c.tx * tile_w;
    c.Y0 = c.ty * FGS_TILE;
    c.start = ranges[2 * c.tile];
    c.end = ranges[2 * c.tile + 1];
    return c;
}

__device__ __forceinline__ TileCtx tile_ctx(uint32_t tiles, uint32_t tiles_x,
                                            const uint32_t *__restrict__ tile_order,
                                            const uint32_t *__restrict__ ranges, uint32_t tile_w = FGS_TILE) {
    return tile_ctx_of(tile_order ? tile_order[blockIdx.x] : blockIdx.x, tiles, tiles_x, ranges, tile_w);
}

// Checkpoints are a write-once / read-once stream (307 MB per config-3 step against 12.6 MB of records).  Non-temporal
// stores / loads for them (FGS_CKPT_NT=1) were measured in round 3 and are OFF: WRITE_SIZE of the forward ROSE from 450
// to 547 MB per launch (the nt stores reach the fabric as more, smaller writes), the backward got 1 % slower, and what
// actually evicted `rec` from L2 was the launch order, not the checkpoint stream (see order_groups in k_blend_fwd_parts: FETCH_SIZE
// 330 -> 62 MB).
#ifndef FGS_CKPT_NT
#define FGS_CKPT_NT 0
#endif
__device__ __forceinline__ void nt_store(float *p, float v) {
#if FGS_CKPT_NT
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}
__device__ __forceinline__ float nt_load(const float *p) {
#if FGS_CKPT_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

// The staged record of a list entry, as ALL THREE blend kernels park it in LDS (k_composite_fwd, k_blend_fwd_parts, k_composite_bwd):
// the backward's recomputed a', w and T are the forward's to the bit because the three stage through this one function.
//   q0 = (u, v, K a, K (b + c)), q1 = (K d, lop, 0.99 r, 0.99 g), q2 = (0.99 b, 0.99 depth, cbits, flags)   (stage_decode_w, fgs_wave.h)
// with the conic in exp2 units (K = -log2(e) / 2) and lop passed in: blend_lop(opacity) by the forwards; by the backward
// FGS_FOLD_FLOOR_LOG2 for the opacities fgs_opacity_floored names, blend_lop(opacity) for the rest.
// alpha = min(G op, 0.99) = 0.99 a', a' = clamp01(G op') with op' = op / 0.99, and G op' = exp2(m' + log2 op'): the list loop adds
// lop = log2 op' to the row term of the exponent (the FMA that forms it costs what the multiply did) and takes a' from the v_exp
// itself with the FREE clamp modifier -- no per-pixel multiply, no v_min (4.3 issue cycles on gfx950).  The 0.99 rides on the
// colours / depth (w c = (a' T)(0.99 c)) and on the transmittance update (T -= 0.99 a' T, one v_fmac with a literal).
// The backward's list loop works with w' = a' T = w / 0.99 and colours c' = 0.99 c, so that w q = w' q', and its dalpha is
// 0.99 dL/dalpha.  The pass has a' where it had G, so it accumulates dG = dalpha a' = op dL/dalpha G.
// ROW CONTRACT with k_row_sum (fgs_project.hip), X = the sums of dL/dalpha G {dx, dy, dx^2, dx dy, dy^2, 1}:
//   moment rows and the sum-dG row = opacity X, colour / depth rows = 1 / 0.99 x theirs;
//   opacities below the floor of fgs_opacity_floored (fgs_internal.h; exactly 0 included, whose dL/dopacity is not
//   zero): the EXACT lop = -64 is folded instead of theirs, a' = 2^-64 G, and the rows are
//   0.99 2^-64 X and (2^-64 / op') / 0.99 x (colour, depth).
// A floored entry's a' is not the forward's (which folds the true lop, -inf for opacity 0): both are below
// 5.5e-20, where T (1 - 0.99 a') rounds to T and w q moves S by less than 1e-19 |q|.
__device__ __forceinline__ void blend_stage_fold(float4 &q0, float4 &q1, float4 &q2, uint32_t flags, uint32_t cbits, float lop) {
    q0.z *= NEG_HALF_LOG2E; q0.w *= NEG_HALF_LOG2E; q1.x *= NEG_HALF_LOG2E;
    q1.y = lop;
    q1.z *= ALPHA_MAX; q1.w *= ALPHA_MAX; q2.x *= ALPHA_MAX; q2.y *= ALPHA_MAX;
    q2.z = __uint_as_float(cbits); q2.w = __uint_as_float(flags);
}

// Per-pixel epilogue of the three forwards (k_composite_fwd, k_blend_fwd_parts, k_phase_fwd), pixel at offset o = y W + x of image b:
// the saved state (planes C_r, C_g, C_b, A, D of pix_state; plane 5, Phi, belongs to the phase path, whose forward adds it: nobody
// reads it on the blend path), the clamped image and the depth.  A and T = 1 - A are the caller's: each forward rounds them its way.
__device__ __forceinline__ void pixel_store(float *__restrict__ pix_state, float *__restrict__ out_rgb, float *__restrict__ out_depth,
                                            uint32_t b, size_t HW, size_t o, float bg0, float bg1, float bg2, float Cr, float Cg,
                                            float Cb, float A, float T, float D) {
    float *ps = pix_state + (size_t)b * 6 * HW + o;
    nt_store(ps, Cr); nt_store(ps + HW, Cg); nt_store(ps + 2 * HW, Cb); nt_store(ps + 3 * HW, A); nt_store(ps + 4 * HW, D);
    float *img = out_rgb + (size_t)b * 3 * HW + o;
    nt_store(img, fminf(fmaxf(Cr + T * bg0, 0.0f), 1.0f));
    nt_store(img + HW, fminf(fmaxf(Cg + T * bg1, 0.0f), 1.0f));
    nt_store(img + 2 * HW, fminf(fmaxf(Cb + T * bg2, 0.0f), 1.0f));
    nt_store(out_depth + (size_t)b * HW + o, D);
}

// Per-pixel prologue of the two backwards (k_composite_bwd, k_phase_bwd): the forward's saved state and the upstream gradients of the
// pixel at offset o of image b.  The image's clamp passes its gradient on the CLOSED interval [0, 1] of the unclamped value, which is
// re-formed from the saved state as pixel_store formed it.  Each kernel builds its own S / Abar from these.
struct PixelGrad { float gr, gg, gb, gd, Cr, Cg, Cb, Tf, D; };
__device__ __forceinline__ PixelGrad pixel_grad_load(const float *__restrict__ pix_state, const float *__restrict__ g_rgb,
                                                     const float *__restrict__ g_depth, uint32_t b, size_t HW, size_t o, float bg0,
                                                     float bg1, float bg2) {
    const float *ps = pix_state + (size_t)b * 6 * HW + o;
    PixelGrad g;
    g.Cr = ps[0]; g.Cg = ps[HW]; g.Cb = ps[2 * HW]; g.Tf = 1.0f - ps[3 * HW]; g.D = ps[4 * HW];
    const float pr = g.Cr + g.Tf * bg0, pg = g.Cg + g.Tf * bg1, pb = g.Cb + g.Tf * bg2;
    const float *gi = g_rgb + (size_t)b * 3 * HW + o;
    g.gr = (pr >= 0.0f && pr <= 1.0f) ? gi[0] : 0.0f;  // clamp backward, closed interval
    g.gg = (pg >= 0.0f && pg <= 1.0f) ? gi[HW] : 0.0f;
    g.gb = (pb >= 0.0f && pb <= 1.0f) ? gi[2 * HW] : 0.0f;
    g.gd = g_depth[(size_t)b * HW + o];
    return g;
}

// Row-split forward of the blend path (FgsDims.saturation_skip and fwd_variant < 0; the default is the depth-split
// k_blend_fwd_parts below, the phase path has its own kernels, k_phase_fwd / k_phase_bwd).  FWD_WAVES waves per tile: with 2,
// wave w owns sub-tiles 2w and 2w+1, the upper / lower half of the tile (the forward has no cross-lane reduction, so the
// split is free and halves the serial length of the longest lists); 1 when the launch has enough tiles to fill the chip
// several times over.  All waves of a block share the LDS-staged chunk of the list.
//
// Per-record work is decided once, at staging time, in parallel over the chunk: stage_decode_w (fgs_wave.h) leaves a flags
// word (touched sub-tiles, row bits) and the column bits; in the list loop a lane turns its column / row bit into an all-ones /
// zero mask with v_bfe_i32 and and-s it onto a' = alpha / 0.99 -- no per-pixel compare / select (issue costs: DESIGN.md section 4).
// SKIP: FgsDims.saturation_skip (separate instantiation).

template <int FWD_WAVES, bool SKIP>
__global__ __launch_bounds__(64 * FWD_WAVES) void k_composite_fwd(
    uint32_t tiles, uint32_t tiles_x, uint32_t W, uint32_t H, float bg0, float bg1, float bg2,
    const uint32_t *__restrict__ tile_order, const uint32_t *__restrict__ ranges,
    const uint32_t *__restrict__ dup_ids, const float *__restrict__ rec,
    float *__restrict__ pix_state, float *__restrict__ out_rgb,
    float *__restrict__ out_depth, const uint32_t *__restrict__ seg_off, float *__restrict__ seg_ckpt, float t_eps) {
    // records per LDS chunk: one per thread, but never more than a depth segment on the blend path
    constexpr int FCH = (64 * FWD_WAVES > FGS_SEG) ? FGS_SEG : 64 * FWD_WAVES;
    static_assert(FGS_SEG % FCH == 0, "segment boundaries must fall on chunk boundaries");
    __shared__ float4 sh0[FCH], sh1[FCH], sh2[FCH];
    const TileCtx c = tile_ctx(tiles, tiles_x, tile_order, ranges);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = FWD_WAVES > 1 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0u;
    const uint32_t lx = lane & 7u, ly = lane >> 3;
    constexpr int NS = 4 / FWD_WAVES;  // sub-tiles per wave
    // running transmittance T (w = alpha T; T -= w)
    float T[NS], Cr[NS], Cg[NS], Cb[NS], Dm[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) { T[s] = 1.0f; Cr[s] = 0; Cg[s] = 0; Cb[s] = 0; Dm[s] = 0; }
    // sub-tile rows / columns per wave: 4 sub-tiles = 2 x 2, 2 = one row of two, 1 = a single sub-tile
    constexpr int NR = NS == 4 ? 2 : 1, NC = NS == 1 ? 1 : 2;
    const uint32_t row0 = NS == 4 ? 0u : (NS == 2 ? wave : wave >> 1), col0 = NS == 1 ? (wave & 1u) : 0u;
    // this lane's column bit in the staged column bits / row bit in the flags
    const uint32_t shx = lx + 8u * col0, shy = 16u + ly + 8u * row0;
    uint32_t alive = 15u;  // sub-tiles still being composited (saturation_skip)
    uint32_t live_segments = (c.end - c.start + FGS_SEG - 1) / FGS_SEG;
    float fx0 = (float)(c.X0 + lx + 8u * col0), fx1 = (float)(c.X0 + lx + 8u * col0 + 8u), fy0 = (float)(c.Y0 + ly + 8u * row0);
    asm("" : "+v"(fx0), "+v"(fx1), "+v"(fy0));  // hoisted for good: no v_cvt in the list loop
    for (uint32_t base = c.start; base < c.end; base += FCH) {
        const uint32_t n = min((uint32_t)FCH, c.end - base);
        if (base != c.start && ((base - c.start) % FGS_SEG) == 0) {
            // state in front of this depth segment: the backward work unit (tile, segment) restarts from it
            float *ck = seg_ckpt + ((size_t)seg_off[c.tile] + (base - c.start) / FGS_SEG) * (5 * 256) + lane;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const uint32_t sg = wave * NS + s;
                ck[(0 * 4 + sg) * 64] = Cr[s]; ck[(1 * 4 + sg) * 64] = Cg[s]; ck[(2 * 4 + sg) * 64] = Cb[s];
                ck[(3 * 4 + sg) * 64] = 1.0f - T[s]; ck[(4 * 4 + sg) * 64] = Dm[s];
            }
        }
        if (SKIP && ((base - c.start) % FGS_SEG) == 0) {
            // FgsDims.saturation_skip: at every segment boundary, sub-tiles whose transmittance (as the backward
            // will see it, 1 - A) is below t_eps for all 64 pixels stop being composited; when the whole tile is
            // saturated the list walk ends and the number of live segments is left for the backward
            uint32_t aw = 0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                float acc = 1.0f - T[s];
                asm("" : "+v"(acc));  // keep 1 - (1 - T): what the checkpoint stores, not T itself
                if (__ballot(1.0f - acc >= t_eps) != 0ull) aw |= 1u << (wave * NS + s);
            }
            alive = aw;
            if (!__syncthreads_or(aw != 0u)) { live_segments = (base - c.start) / FGS_SEG; break; }
        }
        if (threadIdx.x < n) {
            const uint32_t gid = dup_ids[base + threadIdx.x];
            const float4 *r = reinterpret_cast<const float4 *>(rec + (size_t)gid * FGS_REC_FLOATS);
            float4 q0 = r[0], q1 = r[1], q2 = r[2];
            uint32_t flags, cbits;  // flags: touched sub-tiles (none when the opacity is negative), row bits; cbits: column bits
            stage_decode_w<2>(c.X0, c.Y0, __float_as_uint(q2.z), __float_as_uint(q2.w), q1.y, flags, cbits);
            blend_stage_fold(q0, q1, q2, flags, cbits, blend_lop(q1.y));
            sh0[threadIdx.x] = q0; sh1[threadIdx.x] = q1; sh2[threadIdx.x] = q2;
        }
        __syncthreads();
        for (uint32_t j = 0; j < n; ++j) {
            const float4 q0 = sh0[j], q1 = sh1[j], q2 = sh2[j];
            {
                // Non-phase blend.  Most list entries touch only one or two of a wave's sub-tiles, so nothing is
                // precomputed beyond the row terms; bbox membership = the lane's column / row bit of the staged
                // column bits / flags as an all-ones / zero mask (v_bfe_i32) and-ed onto a' (no compare / select).
                const uint32_t msk = __builtin_amdgcn_readfirstlane(__float_as_uint(q2.w)) & (SKIP ? alive : 15u);
                if (!(msk & (((1u << NS) - 1u) << (wave * NS)))) continue;
                const uint32_t cbits = __float_as_uint(q2.z), rbits = __float_as_uint(q2.w);
#pragma unroll
                for (int row = 0; row < NR; ++row) {
                    if (NS == 4 && !((msk >> (2 * row)) & 3u)) continue;
                    const float dy = (NS == 4 && row) ? fy0 + 8.0f - q0.y : fy0 - q0.y;
                    const float bdy = q0.w * dy, cyy = fmaf(q1.x * dy, dy, q1.y);  // lop included
                    const uint32_t my = (uint32_t)__builtin_amdgcn_sbfe((int)rbits, shy + 8u * row, 1);
#pragma unroll
                    for (int col = 0; col < NC; ++col) {
                        const int s = NC * row + col;  // index into this wave's state
                        const uint32_t sg = wave * NS + s;
                        if (NS > 1 && !((msk >> sg) & 1u)) continue;  // scalar branch: sub-tile not touched
                        const float dx = (col ? fx1 : fx0) - q0.x;
                        const float t = q0.z * dx + bdy;
                        const uint32_t mk = my & (uint32_t)__builtin_amdgcn_sbfe((int)cbits, shx + 8u * col, 1);
                        const float a1 = blend_alpha1(t * dx + cyy, mk);  // alpha / 0.99
                        const float w = a1 * T[s];                       // (alpha T) / 0.99
                        Cr[s] += w * q1.z; Cg[s] += w * q1.w; Cb[s] += w * q2.x; Dm[s] += w * q2.y;
                        T[s] = fmaf(w, -ALPHA_MAX, T[s]);
                    }
                }
                continue;
            }
        }
        __syncthreads();
    }
    // live-segment count for the backward, parked in the (otherwise unused) checkpoint slot of segment 0
    if (SKIP && threadIdx.x == 0 && c.end > c.start)
        reinterpret_cast<uint32_t *>(seg_ckpt + (size_t)seg_off[c.tile] * (5 * 256))[0] = live_segments;
    const size_t HW = (size_t)W * H;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const uint32_t sg = wave * NS + s;
        const uint32_t px = c.X0 + 8u * (sg & 1) + lx, py = c.Y0 + 8u * (sg >> 1) + ly;
        if (px < W && py < H) {
            const float Af = 1.0f - T[s];
            pixel_store(pix_state, out_rgb, out_depth, c.b, HW, (size_t)py * W + px, bg0, bg1, bg2, Cr[s], Cg[s], Cb[s], Af,
                        1.0f - Af /* T as the backward will see it */, Dm[s]);
        }
    }
}

// Depth-split forward of the blend path.  Alpha compositing is associative: a list cut into parts can be
// composited part by part from T = 1 and the partial results composed afterwards,
//     (C, T) o (C', T') = (C + T C', T T').
// NP waves per tile; wave p composites list part p (a whole number of FGS_SEG segments, ALL FOUR sub-tiles per
// lane), staging its own 64-record chunks in wave-private LDS -- no block barrier inside the list walk.  Compared
// with splitting a tile by sub-tile rows (k_composite_fwd) every list entry is read from LDS by ONE wave instead of
// all of them and its row terms are formed once, at the same serial length per wave.
// Checkpoints: a wave stores its LOCAL state at the segment boundaries inside its part.  After the walk wave 0
// composes the parts in order and leaves the ABSOLUTE state in the checkpoint slot of every part's first segment;
// the backward unit of a later segment of part p > 0 re-bases its local checkpoint with that slot
// (k_composite_bwd, `fwd_parts`).  Hand-over between the waves goes through the checkpoint slots themselves
// (the slot of the next part's first segment; the last part uses the tile's slot 0, which nothing else reads).
// Behind the head launch (REST) the hand-over goes through LDS instead, part by part: see the chain in the kernel.
struct BlendState { float Cr, Cg, Cb, T, D; };
__device__ __forceinline__ BlendState compose(const BlendState &a, const BlendState &b) {
    return {a.Cr + a.T * b.Cr, a.Cg + a.T * b.Cg, a.Cb + a.T * b.Cb, a.T * b.T, a.D + a.T * b.D};
}
// [5][NS][64] slot (NS = 4 sub-tiles of a 16 x 16 tile, 8 of a 32 x 16 tile), this lane's cell; PL = NS * 64
template <int PL = 256>
__device__ __forceinline__ void ckpt_store(float *ck, const BlendState &v) {
    nt_store(ck, v.Cr); nt_store(ck + PL, v.Cg); nt_store(ck + 2 * PL, v.Cb); nt_store(ck + 3 * PL, 1.0f - v.T); nt_store(ck + 4 * PL, v.D);
}
template <int PL = 256>
__device__ __forceinline__ BlendState ckpt_load(const float *ck) {
    return {nt_load(ck), nt_load(ck + PL), nt_load(ck + 2 * PL), 1.0f - nt_load(ck + 3 * PL), nt_load(ck + 4 * PL)};
}

// One chunk (<= 64 list entries from `base`) of a wave's walk in the depth-split forward, k_blend_fwd_parts and k_blend_fwd_head:
// stage the chunk in the wave's own LDS rows, then composite it onto the lane's four sub-tile states.
struct BlendLane { uint32_t shx, shy; float fx0, fx1, fy0; };  // the lane's column / row bit in cbits / flags and its pixel coordinates
__device__ __forceinline__ void blend_fwd_chunk(float4 *__restrict__ w0, float4 *__restrict__ w1, float4 *__restrict__ w2, uint32_t lane,
                                                uint32_t base, uint32_t n, uint32_t X0, uint32_t Y0, const uint32_t *__restrict__ dup_ids,
                                                const float *__restrict__ rec, const BlendLane &ln, float (&T)[4], float (&Cr)[4],
                                                float (&Cg)[4], float (&Cb)[4], float (&Dm)[4]) {
    // staging COMPACTS the chunk: only the records that touch this wave's 16 x 16 pixels are parked (in list order),
    // so the list loop below has no skip test -- on 32 x 16 tiles ~15 % of a list's entries touch only the other half
    float4 q0, q1, q2;
    uint32_t flags = 0, cbits = 0;
    if (lane < n) {
        const uint32_t gid = dup_ids[base + lane];
        const float4 *r = reinterpret_cast<const float4 *>(rec + (size_t)gid * FGS_REC_FLOATS);
        q0 = r[0]; q1 = r[1]; q2 = r[2];
        stage_decode_w<2>(X0, Y0, __float_as_uint(q2.z), __float_as_uint(q2.w), q1.y, flags, cbits);
    }
    const unsigned long long tmask = __ballot((flags & 15u) != 0u);
    const uint32_t nt = (uint32_t)__popcll(tmask);
    if (flags & 15u) {
        const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(tmask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)tmask, 0u));
        blend_stage_fold(q0, q1, q2, flags, cbits, blend_lop(q1.y));
        w0[slot] = q0; w1[slot] = q1; w2[slot] = q2;
    }
    __builtin_amdgcn_wave_barrier();  // wave-private LDS: one wave's LDS instructions execute in order
    for (uint32_t j = 0; j < nt; ++j) {
        const uint32_t fl = __builtin_amdgcn_readfirstlane(__float_as_uint(w2[j].w));  // stage_decode_w flags
        const uint32_t msk = fl & 15u;
        const float4 q0 = w0[j], q1 = w1[j], q2 = w2[j];
        // (Skipping the lane masks for entries whose bbox covers the tile, or the min for opacities <= 0.98, behind
        // wave-uniform branches -- what pays in the backward -- made this loop 10 % SLOWER: 0.68 -> 0.75 ms at config 3;
        // its passes are too short to amortise a branch.)
        const uint32_t cbits = __float_as_uint(q2.z), rbits = __float_as_uint(q2.w);
        // the lane's two column masks once per entry (3.3 sub-tile passes per entry on average: -2.8 %)
        const uint32_t mxc[2] = {(uint32_t)__builtin_amdgcn_sbfe((int)cbits, ln.shx, 1), (uint32_t)__builtin_amdgcn_sbfe((int)cbits, ln.shx + 8u, 1)};
        // ... and its two column offsets (3.3 passes per entry: one subtraction per pass would be more)
        float dxc[2] = {ln.fx0 - q0.x, ln.fx1 - q0.x};
        asm("" : "+v"(dxc[0]), "+v"(dxc[1]));
#pragma unroll
        for (int row = 0; row < 2; ++row) {
            if (!((msk >> (2 * row)) & 3u)) continue;
            const float dy = row ? ln.fy0 + 8.0f - q0.y : ln.fy0 - q0.y;
            const float bdy = q0.w * dy, cyy = fmaf(q1.x * dy, dy, q1.y);  // the row's part of the exponent, lop included
            const uint32_t my = (uint32_t)__builtin_amdgcn_sbfe((int)rbits, ln.shy + 8u * row, 1);
#pragma unroll
            for (int col = 0; col < 2; ++col) {
                const int s = 2 * row + col;
                if (!((msk >> s) & 1u)) continue;  // scalar branch: sub-tile not touched
                const float dx = dxc[col];
                const float t = q0.z * dx + bdy;
                const uint32_t mk = my & mxc[col];
                const float a1 = blend_alpha1(t * dx + cyy, mk);  // alpha / 0.99, zero outside the bbox
                const float w = a1 * T[s];  // (alpha T) / 0.99
                Cr[s] += w * q1.z; Cg[s] += w * q1.w; Cb[s] += w * q2.x; Dm[s] += w * q2.y;
                T[s] = fmaf(w, -ALPHA_MAX, T[s]);
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// WIDE = 1: 32 x 16 tiles (FgsSavedLayout.tile_w = 32; the backward then has eight sub-tiles per lane and ~0.6x as many
// list entries, reductions and gradient rows).  The forward keeps its 16 x 16 register budget -- holding eight sub-tiles per
// lane here cost 99 VGPRs, 4-5 waves per SIMD and +5 ... 35 % -- by giving every list part TWO waves, one per 16 x 16 half
// of the tile: a wave stages the part's records with the flags of ITS half and skips the entries that do not touch it, so
// its work is that of the 16 x 16 tile's list plus one LDS read and a branch per skipped entry.
template <int NP, int WIDE, bool REST>
__global__ __launch_bounds__(64 * NP * (1 + WIDE)) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_blend_fwd_parts(  // 64 VGPRs: -2.6 %
    uint32_t tiles, uint32_t tiles_x, uint32_t W, uint32_t H, float bg0, float bg1, float bg2,
    const uint32_t *__restrict__ tile_order, const uint32_t *__restrict__ ranges,
    const uint32_t *__restrict__ dup_ids, const float *__restrict__ rec, float *__restrict__ pix_state,
    float *__restrict__ out_rgb, float *__restrict__ out_depth, const uint32_t *__restrict__ seg_off,
    float *__restrict__ seg_ckpt, uint32_t seg_len, uint32_t order_groups, const uint32_t *__restrict__ fwd_open, uint32_t head_segs,
    uint32_t prewalk) {
    constexpr int NW = NP * (1 + WIDE);                   // waves per block
    constexpr int TSX = WIDE ? 4 : 2;                     // sub-tile columns of the whole tile
    constexpr int PL = 2 * TSX * 64, SLOT = 5 * PL;       // floats per checkpoint plane / slot: [5][2 TSX][64]
    __shared__ float4 shb[3][NW][64];                     // the waves' staging rows; behind the walks the hand-over chain's states (REST)
    float4 (&sh0)[NW][64] = shb[0], (&sh1)[NW][64] = shb[1], (&sh2)[NW][64] = shb[2];
    // launch order: tile_order holds the tiles of XCD group 0 heavy-first, then group 1's, ... (fgs_bin.hip tile_group);
    // blocks are dealt round-robin over the XCDs, so XCD g walks group g -- one image (or band of tile rows) per L2
    const uint32_t slot_in_order = order_groups > 1u ? fgs_xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
    const TileCtx c = tile_ctx_of(tile_order[slot_in_order], tiles, tiles_x, ranges, 8u * TSX);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t part = WIDE ? wave >> 1 : wave, half = WIDE ? wave & 1u : 0u;
    // REST: the launch behind k_blend_fwd_head (below).  A half that the head closed or finished has its pixels and every
    // checkpoint slot the backward will read already (a closed half: its closing slot alone, saved.fwd_close): its waves touch
    // nothing -- they neither read nor write a slot -- and only keep the block's barrier; a block without an open half leaves.
    bool mine = true;
    if (REST) {
        const uint32_t open0 = fwd_open[2u * c.tile], open1 = WIDE ? fwd_open[2u * c.tile + 1u] : 0u;
        if (!(open0 | open1)) return;
        mine = (half ? open1 : open0) != 0u;
    }
    const uint32_t X0 = c.X0 + 16u * half;                // this wave's 16 x 16 half of the tile
    const uint32_t lx = lane & 7u, ly = lane >> 3;
    const uint32_t nseg = (c.end - c.start + seg_len - 1) / seg_len;
    const uint32_t spp = (nseg + NP - 1) / NP;  // segments per part
    const uint32_t first_seg = part * spp;
    const bool active = first_seg < nseg;
    const uint32_t pstart = c.start + first_seg * seg_len;
    const uint32_t pend = active ? min(c.end, pstart + spp * seg_len) : pstart;
    // this lane's cells of a checkpoint slot: sub-tile (row, 2 half + col) of the tile's 2 x TSX grid
    float *slot0 = seg_ckpt + (size_t)seg_off[c.tile] * SLOT + 2u * half * 64u + lane;
    auto cell = [](int s) { return ((s >> 1) * TSX + (s & 1)) * 64; };
    float T[4], Cr[4], Cg[4], Cb[4], Dm[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) { T[s] = 1.0f; Cr[s] = 0; Cg[s] = 0; Cb[s] = 0; Dm[s] = 0; }
    BlendLane ln = {lx, 16u + ly, (float)(X0 + lx), (float)(X0 + lx + 8u), (float)(c.Y0 + ly)};
    asm("" : "+v"(ln.fx0), "+v"(ln.fx1), "+v"(ln.fy0));
    uint32_t wstart = pstart;  // where this wave's walk begins
    if (REST && part == 0 && mine) {
        // part 0 of an open half resumes behind the head's min(spp, head_segs) segments, from the state the head left in the slot
        // in front of the next one -- with T ITSELF in the A plane (1 - (1 - T) is not T), which is put right here
        const uint32_t hs = min(spp, head_segs);
        float *ck = slot0 + (size_t)hs * SLOT;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float *k = ck + cell(s);
            Cr[s] = nt_load(k); Cg[s] = nt_load(k + PL); Cb[s] = nt_load(k + 2 * PL); T[s] = nt_load(k + 3 * PL); Dm[s] = nt_load(k + 4 * PL);
            nt_store(k + 3 * PL, 1.0f - T[s]);
        }
        wstart = c.start + hs * seg_len;
    }
    // PRE-WALKED tile (REST, the head launch ran its pre-walk blocks, a list of at most NP segments: spp == 1): the hand-over slots of
    // parts 1.. hold their local results already -- those waves neither walk nor store, they keep the barrier; part 0 composes as ever
    const bool walked = REST && NP > 1 && prewalk != 0u && nseg <= (uint32_t)NP && part != 0u;
    const uint32_t wend = ((!REST || mine) && !walked) ? pend : wstart;
    for (uint32_t base = wstart; base < wend; base += 64) {
        const uint32_t n = min(64u, wend - base);
        if (base != wstart && ((base - c.start) % seg_len) == 0) {  // LOCAL state in front of this segment
            float *ck = slot0 + (size_t)((base - c.start) / seg_len) * SLOT;
#pragma unroll
            for (int s = 0; s < 4; ++s) ckpt_store<PL>(ck + cell(s), BlendState{Cr[s], Cg[s], Cb[s], T[s], Dm[s]});
        }
        blend_fwd_chunk(sh0[wave], sh1[wave], sh2[wave], lane, base, n, X0, c.Y0, dup_ids, rec, ln, T, Cr, Cg, Cb, Dm);
    }
    // ---- hand the part results over and compose them (the part-0 wave of each half) ----
    const uint32_t last = nseg ? (nseg - 1) / spp : 0u;
    if (REST && NP > 1 && nseg > spp) {
        // REST: the parts of an open half hand over through LDS, part by part in list order.  The wave of part q takes the absolute
        // state in front of its part from the half's LDS cells, composes it with its own local result -- held in registers as the
        // checkpoint planes would hold it, A = 1 - T, and taken as 1 - A: the operands, the expression, the order and so the bits of
        // the composition through the slots -- stores the absolute state in front of part q + 1 into that part's first slot (what the backward
        // reads) and passes it on; the wave of the last part stores the pixels.  No local result travels through memory, the loads
        // and stores of the parts belong to different waves, and no wave waits for a store to come back before its load.
        static_assert(NP < 2 || 20 * 64 * (1 + WIDE) * sizeof(float) <= sizeof(shb), "the hand-over states need the staging rows' room");
        float *xf = reinterpret_cast<float *>(&shb[0][0][0]) + half * (20u * 64u) + lane;
        const bool chained = mine && part <= last;
        if (chained && part != 0) {
            if (walked) {  // the pre-walk's result, from the hand-over slot it stored (this part's own store below comes later)
                const float *ck = (part == last) ? slot0 : slot0 + (size_t)((part + 1) * spp) * SLOT;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float *k = ck + cell(s);
                    Cr[s] = nt_load(k); Cg[s] = nt_load(k + PL); Cb[s] = nt_load(k + 2 * PL); T[s] = nt_load(k + 3 * PL); Dm[s] = nt_load(k + 4 * PL);
                }
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    float a = 1.0f - T[s];
                    asm("" : "+v"(a));  // opaque, as a value loaded from the plane is: 1 - (1 - T) is not T and must not be folded to it
                    T[s] = a;
                }
            }
        }  // a later part now holds A = 1 - T where T was: what its hand-over slot's A plane holds, and ckpt_load's expression below
        __syncthreads();  // every walk of the block is over: the staging rows are free
        for (uint32_t q = 0; q <= last; ++q) {
            if (chained && part == q) {
                float *nxt = slot0 + (size_t)((q + 1) * spp) * SLOT;  // the first slot of part q + 1
                if (q != 0) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const float *x = xf + (5 * s) * 64;
                        const float aT = x[192], bT = 1.0f - T[s];
                        const BlendState acc = compose(BlendState{x[0], x[64], x[128], aT, x[256]}, BlendState{Cr[s], Cg[s], Cb[s], bT, Dm[s]});
                        Cr[s] = acc.Cr; Cg[s] = acc.Cg; Cb[s] = acc.Cb; T[s] = acc.T; Dm[s] = acc.D;
                        // The A plane of the slot is ONE fma, 1 - a.T b.T, beside the rounded product a.T b.T that is carried on: that is
                        // how the composition through the slots comes out of the compiler (ckpt_store of compose's result under this
                        // unit's contraction), and the two differ by an ulp of A wherever T is not small.  Written out here.
                        if (q != last) {
                            float *k = nxt + cell(s);
                            nt_store(k, acc.Cr); nt_store(k + PL, acc.Cg); nt_store(k + 2 * PL, acc.Cb);
                            nt_store(k + 3 * PL, __builtin_fmaf(-bT, aT, 1.0f)); nt_store(k + 4 * PL, acc.D);
                        }
                        __builtin_amdgcn_sched_barrier(0);  // one sub-tile's five reads at a time: all twenty in flight beside the state spill
                    }
                } else if (min(spp, head_segs) != spp) {
                    // (part 0 that resumed at its own end walked nothing: slot spp holds this very state since the A plane was put right)
#pragma unroll
                    for (int s = 0; s < 4; ++s) ckpt_store<PL>(nxt + cell(s), BlendState{Cr[s], Cg[s], Cb[s], T[s], Dm[s]});
                }
                if (q != last) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        float *x = xf + (5 * s) * 64;
                        x[0] = Cr[s]; x[64] = Cg[s]; x[128] = Cb[s]; x[192] = T[s]; x[256] = Dm[s];
                    }
                }
            }
            if (q != last) __syncthreads();
        }
        if (!chained || part != last) return;
    } else if (NP > 1 && nseg > spp) {  // more than one part, without the head launch: the hand-over goes through the slots
        if (active && part != 0) {
            float *ck = (part == last) ? slot0 : slot0 + (size_t)((part + 1) * spp) * SLOT;
#pragma unroll
            for (int s = 0; s < 4; ++s) ckpt_store<PL>(ck + cell(s), BlendState{Cr[s], Cg[s], Cb[s], T[s], Dm[s]});
        }
        __threadfence_block();
        __syncthreads();
        if (part != 0) return;
        // part 0: its own result is the absolute state in front of part 1
        {
            float *ck = slot0 + (size_t)spp * SLOT;
#pragma unroll
            for (int s = 0; s < 4; ++s) ckpt_store<PL>(ck + cell(s), BlendState{Cr[s], Cg[s], Cb[s], T[s], Dm[s]});
        }
        for (uint32_t pp = 1; pp <= last; ++pp) {
            const float *src = (pp == last) ? slot0 : slot0 + (size_t)((pp + 1) * spp) * SLOT;
            float *dst = slot0 + (size_t)((pp + 1) * spp) * SLOT;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const BlendState acc = compose(BlendState{Cr[s], Cg[s], Cb[s], T[s], Dm[s]}, ckpt_load<PL>(src + cell(s)));
                Cr[s] = acc.Cr; Cg[s] = acc.Cg; Cb[s] = acc.Cb; T[s] = acc.T; Dm[s] = acc.D;
                if (pp != last) ckpt_store<PL>(dst + cell(s), acc);
            }
        }
    } else if (part != 0 || (REST && !mine)) {
        return;
    }
    const size_t HW = (size_t)W * H;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const uint32_t px = X0 + 8u * (s & 1) + lx, py = c.Y0 + 8u * (s >> 1) + ly;
        if (px < W && py < H)
            pixel_store(pix_state, out_rgb, out_depth, c.b, HW, (size_t)py * W + px, bg0, bg1, bg2, Cr[s], Cg[s], Cb[s], 1.0f - T[s],
                        T[s], Dm[s]);
    }
}

// The exiting forward (FgsDims.fwd_variant without FGS_FWD_EXIT_OFF; automatic from 8192 tile halves per launch): k_blend_fwd_head, then k_blend_fwd_parts<NP, WIDE, true> for what it leaves open.
//
// ABSORBING STATE.  The update of a pixel's state by a list entry is w' = a' T (0 <= a' <= 1), X <- fma(w', x', X) for the four
// accumulators X = C_r, C_g, C_b, D with the staged multipliers x' (0.99 colour, 0.99 depth), T <- fma(w', -0.99, T): T never
// grows.  With K >= |x'| for every entry that can still come, |w' x'| <= T K, and once
//     T <= 2^-26   and   T K < 2^-26 |X|   for each of the four X
// every later addend is below a quarter ulp of X: fma returns X itself (round to nearest, either sign, also at a binade
// boundary), 1 - T is 1.0f, and pixel_store's C + T bg is C (K_colour covers |bg| as well).  The state the caller sees -- C, D,
// A = 1 -- is then a fixed point of the rest of the list, and the SAME fixed point under the depth split: a later part's lump
// T_abs C_p has |C_p| <= K (sum of w') <= K (1 + eps), which the factor of two between a quarter and half an ulp covers, as it
// covers the rounding of the test itself.  The comparisons are strict: a zero accumulator or a NaN / infinite bound closes nothing.
// K is per image and from the data (k_project's per-block maxima, folded here); nothing assumes colours <= 1.
// A tile half is CLOSED when the test holds on every in-frame pixel of its four sub-tiles (pixels outside the frame keep T = 1 for
// ever and do not veto).
//
// One wave per 16 x 16 tile half walks the first min(spp, head_segs) segments of part 0 -- the whole list when there is one part --
// and tests at every 64-entry chunk boundary.  Part 0's state is absolute, so stopping there keeps the parent's association.
//   closed, or the list ended: the wave stores the pixels; fwd_open[tile][half] = 0.  A half closed after `done` entries stores its
//     closing state (C, A = 1 - T = 1.0f, D) into ONE slot, k = ceil(done / seg_len) -- the first slot its walk did not reach -- and
//     leaves k in fwd_close[tile][half] (0xFFFFFFFF when k is no slot of the tile: the closing fell into the last segment; and for
//     every half that did not close).  k <= min(spp, head_segs): slot k belongs to part 0 or is the first slot of part 1, an ABSOLUTE
//     state where the backward reads it.  The half's cells of the slots behind k are never written: k_composite_bwd restarts every
//     unit of the half with segment >= k from slot k (see there why those are the bits a full walk leaves), the rest kernel's
//     waves of a closed half touch nothing, and no other kernel reads checkpoint slots.
//   still open: its state goes into the slot in front of the next segment (the slot part 0 writes there anyway), T itself in the
//     A plane, and fwd_open[tile][half] = 1: part 0's wave of the rest kernel resumes from it, the other parts run as they did.
// head_segs bounds the launch for scenes that never saturate: one wave per half for a quarter of the longest list would leave
// most of the chip waiting.
//
// PRE-WALK (FgsPlan.fwd_prewalk; np > 1).  Parts 1.. of a list of at most np segments (spp == 1, the head's reach is segment 0) start
// from T = 1 and need nothing of part 0, so they need not wait for the rest launch: behind the head blocks -- from the next multiple
// of 8 on, so that a block's index modulo 8 still names its XCD -- the launch has one block per (launch slot, part p = 1 .. np - 1),
// of the head's shape: one wave per half, the same LDS.  A block of a longer list (nseg > np) or of a part the list does not have
// (p >= nseg) leaves behind its scalar loads.  Any other walks its one segment through blend_fwd_chunk and stores the local result
// into the hand-over slot of k_blend_fwd_parts: slot p + 1, slot 0 for the last part -- bit for bit what that kernel's wave of the
// part stores there.  It reads no mark and no slot and writes nothing else.  The rest launch then composes only.  Why no bit moves:
//   the head blocks are the code they were, so fwd_open and fwd_close are the words they were;
//   an open half's hand-over slots hold what the rest launch's own waves would have stored, and the same composition follows;
//   a half the head closed has k = 1 (one segment of reach): the pre-walk writes slots 2.. and slot 0 of ITS cells, behind the closing
//     slot, which k_composite_bwd and k_bwd_tail_verdict never read for such a half (they read slot k alone), and the rest launch's
//     waves of a closed half touch nothing;
//   nothing writes slot 1 but the head.
// Measured (DESIGN_LOG.md 30): the walk costs the VALU-bound head launch more than it saves the rest launch (config 3 forward
// 0.180 -> 0.206 ms); automatic is OFF, FGS_FWD_PREWALK_ON turns it on.
template <int WIDE>
__global__ __launch_bounds__(64 * (1 + WIDE)) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_blend_fwd_head(
    uint32_t tiles, uint32_t tiles_x, uint32_t W, uint32_t H, float bg0, float bg1, float bg2,
    const uint32_t *__restrict__ tile_order, const uint32_t *__restrict__ ranges,
    const uint32_t *__restrict__ dup_ids, const float *__restrict__ rec, float *__restrict__ pix_state,
    float *__restrict__ out_rgb, float *__restrict__ out_depth, const uint32_t *__restrict__ seg_off,
    float *__restrict__ seg_ckpt, uint32_t seg_len, uint32_t order_groups, uint32_t *__restrict__ fwd_open, uint32_t head_segs,
    uint32_t np, const uint32_t *__restrict__ fwd_max, uint32_t max_recs, uint32_t *__restrict__ fwd_close, uint32_t head_blocks) {
    constexpr int NW = 1 + WIDE;
    constexpr int TSX = WIDE ? 4 : 2;
    constexpr int PL = 2 * TSX * 64, SLOT = 5 * PL;
    __shared__ float4 sh0[NW][64], sh1[NW][64], sh2[NW][64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t half = WIDE ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0u;
    const uint32_t lx = lane & 7u, ly = lane >> 3;
    if (blockIdx.x >= head_blocks) {
        // PRE-WALK (see above): block j of the range behind the head blocks, which begins at a multiple of 8 so that j & 7 is the
        // block's XCD; XCD g takes (launch slot, part) pairs of ITS group of the tile order, heavy-first, the parts of a tile in a row
        const uint32_t pad = (head_blocks + 7u) & ~7u;
        if (blockIdx.x < pad) return;
        const uint32_t j = blockIdx.x - pad, i = j >> 3;
        const uint32_t bid = (j & 7u) + 8u * (i / (np - 1u)), part = 1u + i % (np - 1u);
        if (bid >= head_blocks) return;  // the groups are not all of one size
        const TileCtx c = tile_ctx_of(tile_order[order_groups > 1u ? fgs_xcd_remap(bid, head_blocks) : bid], tiles, tiles_x, ranges, 8u * TSX);
        const uint32_t nseg = (c.end - c.start + seg_len - 1) / seg_len;
        if (nseg > np || part >= nseg) return;  // spp > 1: the rest launch's walk; no such part
        const uint32_t X0 = c.X0 + 16u * half;
        float *slot0 = seg_ckpt + (size_t)seg_off[c.tile] * SLOT + 2u * half * 64u + lane;
        auto cell = [](int s) { return ((s >> 1) * TSX + (s & 1)) * 64; };
        float T[4], Cr[4], Cg[4], Cb[4], Dm[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) { T[s] = 1.0f; Cr[s] = 0; Cg[s] = 0; Cb[s] = 0; Dm[s] = 0; }
        BlendLane ln = {lx, 16u + ly, (float)(X0 + lx), (float)(X0 + lx + 8u), (float)(c.Y0 + ly)};
        asm("" : "+v"(ln.fx0), "+v"(ln.fx1), "+v"(ln.fy0));
        const uint32_t pstart = c.start + part * seg_len, pend = min(c.end, pstart + seg_len);  // spp == 1: segment `part`
        for (uint32_t base = pstart; base < pend; base += 64u)
            blend_fwd_chunk(sh0[half], sh1[half], sh2[half], lane, base, min(64u, pend - base), X0, c.Y0, dup_ids, rec, ln, T, Cr, Cg, Cb, Dm);
        float *ck = (part == nseg - 1u) ? slot0 : slot0 + (size_t)(part + 1u) * SLOT;  // k_blend_fwd_parts' hand-over slot
#pragma unroll
        for (int s = 0; s < 4; ++s) ckpt_store<PL>(ck + cell(s), BlendState{Cr[s], Cg[s], Cb[s], T[s], Dm[s]});
        return;
    }
    const uint32_t slot_in_order = order_groups > 1u ? fgs_xcd_remap(blockIdx.x, head_blocks) : blockIdx.x;
    const TileCtx c = tile_ctx_of(tile_order[slot_in_order], tiles, tiles_x, ranges, 8u * TSX);
    const uint32_t X0 = c.X0 + 16u * half;
    const uint32_t len = c.end - c.start;
    const uint32_t nseg = (len + seg_len - 1) / seg_len;
    const uint32_t spp = (nseg + np - 1) / np;
    const uint32_t hs = np == 1u ? nseg : min(spp, head_segs);  // segments of part 0 this wave walks at most
    const uint32_t hlen = min(len, hs * seg_len);
    float *slot0 = seg_ckpt + (size_t)seg_off[c.tile] * SLOT + 2u * half * 64u + lane;
    auto cell = [](int s) { return ((s >> 1) * TSX + (s & 1)) * 64; };
    // the image's bound: maxima of bit patterns (fgs_project.hip), the background's channels among the colours
    uint32_t kcb = 0u, kdb = 0u;
    {
        const uint32_t *fm = fwd_max + (size_t)c.b * max_recs * 2u;
        for (uint32_t i = lane; i < max_recs; i += 64u) { kcb = max(kcb, fm[2u * i]); kdb = max(kdb, fm[2u * i + 1u]); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { kcb = max(kcb, (uint32_t)__shfl_xor(kcb, o, 64)); kdb = max(kdb, (uint32_t)__shfl_xor(kdb, o, 64)); }
        kcb = max(max(kcb, __float_as_uint(bg0) & 0x7FFFFFFFu), max(__float_as_uint(bg1) & 0x7FFFFFFFu, __float_as_uint(bg2) & 0x7FFFFFFFu));
    }
    const float Kc = __uint_as_float(__builtin_amdgcn_readfirstlane(kcb)), Kd = __uint_as_float(__builtin_amdgcn_readfirstlane(kdb));  // scalars
    bool inframe[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) inframe[s] = X0 + 8u * (s & 1) + lx < W && c.Y0 + 8u * (s >> 1) + ly < H;
    float T[4], Cr[4], Cg[4], Cb[4], Dm[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) { T[s] = 1.0f; Cr[s] = 0; Cg[s] = 0; Cb[s] = 0; Dm[s] = 0; }
    BlendLane ln = {lx, 16u + ly, (float)(X0 + lx), (float)(X0 + lx + 8u), (float)(c.Y0 + ly)};
    asm("" : "+v"(ln.fx0), "+v"(ln.fx1), "+v"(ln.fy0));
    constexpr float Q = 1.490116119384765625e-8f;  // 2^-26
    uint32_t done = 0;  // entries walked
    bool closed = false;
    while (done < hlen && !closed) {
        if (done != 0u && (done % seg_len) == 0) {  // state in front of this segment (part 0: absolute)
            float *ck = slot0 + (size_t)(done / seg_len) * SLOT;
#pragma unroll
            for (int s = 0; s < 4; ++s) ckpt_store<PL>(ck + cell(s), BlendState{Cr[s], Cg[s], Cb[s], T[s], Dm[s]});
        }
        const uint32_t n = min(64u, hlen - done);
        blend_fwd_chunk(sh0[half], sh1[half], sh2[half], lane, c.start + done, n, X0, c.Y0, dup_ids, rec, ln, T, Cr, Cg, Cb, Dm);
        done += n;
        bool veto = false;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float tc = T[s] * Kc;
            const bool ok = T[s] <= Q && tc < Q * fabsf(Cr[s]) && tc < Q * fabsf(Cg[s]) && tc < Q * fabsf(Cb[s]) && T[s] * Kd < Q * fabsf(Dm[s]);
            veto |= inframe[s] && !ok;
        }
        closed = __ballot(veto) == 0ull;
    }
    const bool finished = closed || done == len;
    // the closing slot: the first slot the walk did not reach (closed => done >= 64, so kclose >= 1; kclose <= hs <= spp: a slot of part 0 or
    // the first slot of part 1 -- absolute in the backward's sense either way)
    const uint32_t kclose = (done + seg_len - 1) / seg_len;
    const bool close_slot = closed && kclose < nseg;
    if (lane == 0) {
        fwd_open[2u * c.tile + half] = finished ? 0u : 1u;
        fwd_close[2u * c.tile + half] = close_slot ? kclose : 0xFFFFFFFFu;
    }
    if (!WIDE && lane == 1) fwd_close[2u * c.tile + 1u] = 0xFFFFFFFFu;  // (the backward of 16 x 16 tiles reads index 0 only)
    if (!finished) {
        float *ck = slot0 + (size_t)hs * SLOT;  // done == hs * seg_len < len
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float *k = ck + cell(s);
            nt_store(k, Cr[s]); nt_store(k + PL, Cg[s]); nt_store(k + 2 * PL, Cb[s]); nt_store(k + 3 * PL, T[s]); nt_store(k + 4 * PL, Dm[s]);
        }
        return;
    }
    const size_t HW = (size_t)W * H;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const uint32_t px = X0 + 8u * (s & 1) + lx, py = c.Y0 + 8u * (s >> 1) + ly;
        if (px < W && py < H)
            pixel_store(pix_state, out_rgb, out_depth, c.b, HW, (size_t)py * W + px, bg0, bg1, bg2, Cr[s], Cg[s], Cb[s], 1.0f - T[s],
                        T[s], Dm[s]);
    }
    // the closing state into the ONE slot behind the walk; the half's cells of every later slot stay unwritten and unread
    if (close_slot) {
        float *ck = slot0 + (size_t)kclose * SLOT;
#pragma unroll
        for (int s = 0; s < 4; ++s) ckpt_store<PL>(ck + cell(s), BlendState{Cr[s], Cg[s], Cb[s], T[s], Dm[s]});
    }
}

// Backward, front-to-back.  For pixel p and Gaussian i:
//   dL/dalpha_i = T_i q_i - S_i / (1 - alpha_i),  q_i = gI.c_i + gD d_i,
//   S_i = T_fin (gI.bg) + sum_{j>i} w_j q_j = T_fin (gI.bg) + Total - sum_{j<=i} w_j q_j,
// with Total = gI.C_acc + gD.D_acc known from the forward's saved per-pixel state, so the
// sweep runs in the SAME order as the forward and T_i is recomputed exactly (no division-
// based transmittance recovery, no saved per-pair state).
//
// Gradient accumulation is atomic-free and deterministic: each lane sums its (up to four)
// pixels' contributions to the ten per-Gaussian sums, the wave adds them up through LDS in a fixed
// order (addtid_park + wave_sum_addtid_finish, fgs_wave.h) and ten lanes store ONE 48-byte row at the duplicate's
// emission slot (dup_off[gaussian] + index of this tile inside the Gaussian's tile rectangle).  A
// Gaussian's rows are contiguous and k_project_bwd sums them in a fixed order.
//
// Work unit = (tile, depth segment of FGS_SEG list entries): the unit restarts from the forward's
// per-pixel checkpoint in front of its segment, so units are independent and of bounded length.
// DEAD UNITS (round 10).  Once the forward's transmittance is <= 2^-25 its accumulated alpha rounds to 1.0f, so a later unit
// restarts with T == +0.0f exactly and keeps it (fma(+0, -0.99, +0) = +0).  A unit ALL of whose in-frame pixels restart so
// (one ballot in the prologue, from the T the prologue holds anyway: 78 % of config 3's units, 33 % of config 2's, 90 % of the
// decoder-like scene's) is walked by composite_bwd_dead_walk, whose pass leaves out the terms that are exact zeros there --
// w = a' T, the four ops of q, the S update, T q, the T update, the four colour / depth sums: 11 plain VALU + v_exp + v_rcp per pass
// instead of 19 + 2 -- and forms the rest in exactly the instruction forms of the general pass, so the gradient rows are the
// same bits.  The one thing not reproduced is the SIGN of a dalpha that is an exact zero (S == +0: no upstream gradient on the
// pixel); it can show only as the sign of a row value that is an exact zero on every pixel of the tile.  Every other unit takes
// the general walk, which is the loop it was, instruction for instruction.
// WHAT S IS IN A DEAD UNIT (round 16; DESIGN_LOG.md 27).  S = Total - (checkpoint sum), both formed by the prologue as the same FMA
// chain over (C, D).  Where the restart state is the pixel's FINAL state bit for bit, S = X - X = +0 EXACTLY.  That is so (a) behind a
// half's closing slot (saved.fwd_close: k_blend_fwd_head stores slot and pix_state from the same registers) and (b) without the
// exiting forward, from the entry on behind which no later entry moves C or D any more -- the state is a fixed point, every later
// checkpoint holds it.  Measured: 99.8 % of config 3's dead units, 97 % of config 2's, all but one of the decoder-like scene's hold
// S == +-0 on every lane (profiles/r16_ab_bwd_zero_units.txt).  In a dead unit IN FRONT of that point -- T already rounds to zero, C
// or D still move by an ulp -- S is the rounding residue of Total - sum w q: small, not zero.  Skipping or zeroing dead units on
// T == 0 ALONE is therefore wrong on those units (0.1 - 1 % of the units of the benchmark scenes, kinds (b) and (c) of the profile),
// and five attempts at it failed their checks.  Round 16 tests S itself: a dead
// unit whose S is +-0 on every lane of every sub-tile gets its rows from composite_bwd_zero_rows without a walk, a dead unit with
// some such sub-tiles walks with those masked, and a unit with a residue anywhere is walked where the residue is -- the predicate
// reads the very bits the dead walk would multiply by, so it is right whatever the reason for the zero
// (FGS_BWD_ZERO_OFF in FgsDims.fwd_variant: every dead unit walked in full, the same bits).
// ONE VERDICT PER CLOSED TILE (round 17; DESIGN_LOG.md 28).  92 % of config 3's zero units are TAIL units -- behind the closing slot of
// every half of their tile -- and all tail units of a tile run the same prologue on the same addresses.  k_bwd_tail_verdict runs it
// once per tile in front of this kernel; a tail unit of a tile whose verdict is "zero units" leaves before its prologue and writes
// NO rows, and k_row_sum does not read them (see both kernels).  Zero units in front of a closing, and every unit where the plan
// has no tail verdict (FgsPlan.bwd_tail), still decide for themselves and store their rows with composite_bwd_zero_rows.
// ZERO SUB-TILES OF A GENERAL UNIT (round 18; DESIGN_LOG.md 29; FgsPlan.bwd_sub, bit 1 of the kernel's zero_units).  A unit is general as
// soon as ONE in-frame pixel restarts with T != 0, and then walked every touched sub-tile of every entry -- also the sub-tiles of a
// half that closed earlier than the other, of a closed half beside one whose list ends open, and single sub-tiles that saturated
// before their half did: 11.3 % of the general units' passes at config 3, 21 % in the decoder-like scene
// (profiles/r18_ab_bwd_zero_subtiles.txt).  The prologue now takes out of `alive` every sub-tile s with T[s] == +0 BY ITS BITS on every
// in-frame lane and S[s] == +-0 on EVERY lane (composite_bwd_zero_subtiles; lanes outside the frame hold T = 1, S = +0, g = 0 and do
// not veto on T).  The list loop is the parent's, instruction for instruction: it has always formed msk = fl & alive.  An entry whose
// mask becomes empty runs no pass, parks ten sums and stores its row as before.  Why no output bit changes, against the instructions
// the general pass compiles to (v_mul w; v_fma S; v_mul, v_fmac dalpha; v_fmamk T; v_mul / v_fmac sums):
//   w = T a' = (+0) a' = +0                       a' = clamp01(exp2(..)) & mask lies in [0, 1] whatever the record holds;
//   S' = fma(-w, q, S) = +-0                      q = fma chain of g and the entry's colours / depth, FINITE: a non-finite upstream
//                                                 gradient makes the prologue's S a NaN or an infinity, never +-0 -- NaN x C = NaN,
//                                                 Inf x C = Inf for C != 0 (and Inf - Inf = NaN against the checkpoint sum), Inf x 0 =
//                                                 NaN for a colour state that is exactly zero -- so such a sub-tile is not in the set;
//                                                 a non-finite colour or depth of the ENTRY is the dead walk's premise too (DEAD UNITS:
//                                                 that walk never forms q) and, as there, differs from the full walk only for an entry
//                                                 behind a closing that the forward never composited;
//   dalpha = fma(q, T, S' rcp(a' - 1 / 0.99)) = +-0   the divisor lies in [-1.0102, -0.0101], its reciprocal is finite;
//   the clamp select returns dalpha or +0;  dG = dalpha a' = +-0;  T' = fma(w, -0.99, T) = -0 + +0 = +0: the sub-tile stays zero
//   for the whole unit, and S stays +-0;
//   every moment and colour / depth term = (+-0) x finite = +-0 (dx, dy finite: see composite_bwd_zero_rows), ADDED to a sum
//   by v_fmac: x + (+-0) = x for x != 0, and +0 + (-0) = +0.
// The one place where a bit of a lane's sum can differ is the FIRST pass of a sub-tile row (s = 0 and s = NSX): the compiler knows
// that the row's sums start at zero and ASSIGNS them (v_mul where the others have v_fmac; -ffast-math knows no signed zero), so a zero
// sub-tile 0 could leave -0 in a sum that is +0 without its pass.  A later non-zero term erases the difference; otherwise it is the sign
// of a lane value that is an exact zero, which survives the fold (products with dya / dyb, sums) and the wave's total only as the sign
// of a row value that is an exact zero on EVERY lane -- and k_row_sum adds the rows to sums that start at +0 and are never -0
// (fgs_project.hip, ROWS NOT WRITTEN), so the seven outputs are the same bits.  That is the dead walk's statement about the sign of an
// exact zero (DEAD UNITS), not more.  A general unit always keeps a live sub-tile, so `alive` never becomes empty here.
// The predicate costs eight ballots per unit; at opacity 0.05, where it never fires, config 3's step and the backward's stage time
// are inside the parent's spread (profiles/r18_ab_bwd_zero_subtiles.txt).
// Six waves per SIMD (80 VGPRs): the loop is bound by VALU issue with dependent chains in every pass (exp -> alpha -> w
// -> S -> rcp -> dalpha), and the sixth wave buys 4 % (1.37 -> 1.31 ms at config 3); a seventh needs spills and loses 35 %.
// NSX = sub-tile columns of the tile: 2 (16 x 16 tiles) or 4 (32 x 16 tiles: eight sub-tiles per lane, ~0.6x as many list
// entries, reductions and gradient rows; 5 waves per SIMD instead of 6 -- the loop is issue-bound, not latency-bound).
// LDS of k_composite_bwd, at file scope: the kernel and the dead unit's walk (a function of its own, below) name the same arrays
__shared__ float4 bwd_sh0[CH], bwd_sh1[CH], bwd_sh2[CH];
__shared__ uint32_t bwd_she[CH];
// per-lane partial sums of one list entry (ten values) -- on 32 x 16 tiles also of a PAIR of a dead unit's entries (six values each:
// cells 0-5 and 6-11).  One array per tile shape, so that k_composite_bwd<2> keeps its 6048 bytes: with twelve pitches (6592 bytes)
// config 2's backward measured 3.3 % slower -- its 24 one-wave blocks per CU apparently no longer fit the LDS (DESIGN_LOG.md 22)
__shared__ __attribute__((aligned(16))) float bwd_red[10 * FGS_RED_PITCH];
__shared__ __attribute__((aligned(16))) float bwd_red_pairs[12 * FGS_RED_PITCH];
#define FGS_BWD_G __attribute__((address_space(1)))  /* global memory, also where the pointer arrives as a function argument */
#ifdef FGS_BWD_UNIT_TRACE
// experiment builds: [0] the zero sub-tiles of a general unit (whether or not the walk masks them), [1] its sub-tile passes with
// none masked, [2] those of them that lie in [0] -- counted by the general walk, recorded by the kernel (scratch/profile/bwd_zero_units.py)
__shared__ uint32_t bwd_trace_sub[3];
#endif

// The chunk / list loop of k_composite_bwd over the unit's entries [c.start, c.end), in two instantiations: DEAD = false the general
// walk, inlined into the kernel; DEAD = true the walk of a dead unit (see the kernel), whose pass computes only what is not an exact
// zero there (see `dead_passes`; g*, T are not read).  Staging, the LDS record layout, the emission slot, the deferred reduction and the row
// store are the same code in both.
template <int NSX, bool DEAD>
__device__ __forceinline__ void composite_bwd_walk(const TileCtx &c, uint32_t lane, uint32_t lx, uint32_t ly, uint32_t dcap, uint32_t alive,
                                                   const uint32_t *__restrict__ dup_ids, const float *__restrict__ rec,
                                                   const uint32_t *__restrict__ dup_off, float *__restrict__ grad_rows,
                                                   const float (&gr)[2 * NSX], const float (&gg)[2 * NSX], const float (&gb)[2 * NSX],
                                                   const float (&gd)[2 * NSX], float (&S)[2 * NSX], float (&T)[2 * NSX]) {
    constexpr int NS = 2 * NSX;
    // geometric sums per sub-tile row, folded once per list entry (below).  32 x 16 tiles only: with at most four passes per
    // entry the fold costs what the passes save, and 16 x 16 tiles measured 0.8 % SLOWER that way (DESIGN_LOG.md 15)
    constexpr bool ROW_MOMENTS = NSX == 4;
    auto &sh0 = bwd_sh0; auto &sh1 = bwd_sh1; auto &sh2 = bwd_sh2; auto &she = bwd_she;
    auto &red = *[]() { if constexpr (NSX == 4) return &bwd_red_pairs; else return &bwd_red; }();
    const uint32_t shx = lx, shy = 16u + ly;  // this lane's column bit in the staged column bits / row bit in the flags
    float fx0 = (float)(c.X0 + lx), fy0 = (float)(c.Y0 + ly);
    asm("" : "+v"(fx0), "+v"(fy0));  // hoisted for good: no v_cvt in the list loop
    // The reduction of a list entry's ten sums is DEFERRED by one entry: the passes of entry j end with the sums parked in `red`
    // (addtid_park), and the read-back, the adds and the row store happen at the top of entry j + 1, where their LDS reads travel
    // together with that entry's record reads -- one exposed LDS round trip per entry instead of three (record; parked sums; row
    // index).  One wave's LDS instructions execute in order, so the read-back of entry j is served before entry j + 1 parks its own
    // sums in the same cells.  e_prev: row of the entry whose sums are parked (none yet: no row passes e < dcap).
    uint32_t e_prev = ~0u;
#ifdef FGS_BWD_UNIT_TRACE
    [[maybe_unused]] uint32_t trace_passes = 0u, trace_zero_passes = 0u;
#endif
    auto reduce_parked = [&]() {
        const float tot = wave_sum_addtid_finish(red, lane, 10u);
        // (16-float rows: all sixteen quads' last lanes store, lanes >= 40 a zero -- one whole 64-byte line)
        if ((lane & 3u) == 3u && lane < 4u * FGS_BLEND_ROW_FLOATS && e_prev < dcap) ((FGS_BWD_G float *)grad_rows)[(size_t)e_prev * FGS_BLEND_ROW_FLOATS + (lane >> 2)] = tot;
    };
    // ---- the list loop of a DEAD unit (round 11; DESIGN_LOG.md 22) ----
    // T == +0 on every pixel that is not masked: w = a' T = +0, S keeps its value (S -= w q), the colour / depth sums are exact
    // zeros and dalpha = T q - S r = -(S r) (T q = +-0; q is finite, or S is already NaN: a non-finite colour or upstream gradient
    // reaches S through the forward's saved state in the prologue).  So a dead entry has SIX sums, not ten, and -- S being read-only,
    // T constant -- needs nothing from the entry before it.  On 32 x 16 tiles the walk therefore takes its entries in PAIRS: entries
    // j, j + 1 of a chunk (CH is even: only a unit's last entry can be single) share one reduction round and one row store.  A parks
    // its sums in value cells 0-5 of `red`, B in 6-11; one wave_sum_addtid_finish over 12 values -- the same 16-partial sums and DPP
    // steps per value -- leaves value k in the quad-last lane of quad k < 12, which stores float k % 6 of row e[k / 6]; lanes 48-55,
    // whose `tot` is +0.0f, store floats 6-9 of the two rows (the sum of 64 parked +0 is +0: the bits of the rows are unchanged).
    // Still deferred by one round: the read-back travels with the next pair's records.  16 x 16 tiles take one entry per round (six
    // values, lanes 24-27 the zeros): the two pitches more of LDS cost their kernel 3.3 %, which is more than the pairing saves.
    // (Running a wholly touched sub-tile row's passes as one branch-free block, select hoisted, was built and measured 0.5 % SLOWER.)
    // What a pass computes is written in exactly the forms the general pass compiles to (contraction is on in this unit, and nothing
    // makes two copies of one expression contract alike): exponent = two FMAs; -(S r) = S rcp(a' - 1 / 0.99); every moment an FMA onto
    // its sum, from the ROUNDED dG and dG dx; the fold's three dy sums as the FMAs the general walk's fold contracts to.  The rows are
    // the general walk's to the bit (but for the sign of an exact zero: see the kernel).
    constexpr bool PAIRS = NSX == 4;
    constexpr uint32_t DSUMS = 6, DROWS = PAIRS ? 2 : 1, DZERO = FGS_BLEND_ROW_FLOATS - DSUMS;  // sums / rows per round, zero floats per row
    static_assert(4 * DSUMS * DROWS + DROWS * DZERO <= 64, "dead walk: one lane per zero float behind the sums' lanes");
    [[maybe_unused]] uint32_t e_prevB = ~0u;  // row of the parked pair's second entry (none: no row passes e < dcap)
    [[maybe_unused]] auto reduce_parked_dead = [&]() {
        const float tot = wave_sum_addtid_finish(red, lane, DSUMS * DROWS);  // lanes >= 4 DSUMS DROWS: +0.0f
        const uint32_t k = lane >> 2, z = lane - 4u * DSUMS * DROWS;
        const bool sum_lane = (lane & 3u) == 3u && k < DSUMS * DROWS, zero_lane = lane >= 4u * DSUMS * DROWS && z < DROWS * DZERO;
        const bool second = sum_lane ? k >= DSUMS : z >= DZERO;  // this lane stores into the pair's second row
        const uint32_t col = sum_lane ? (second ? k - DSUMS : k) : DSUMS + (second ? z - DZERO : z);
        const uint32_t e = PAIRS && second ? e_prevB : e_prev;
        if ((sum_lane || zero_lane) && e < dcap) ((FGS_BWD_G float *)grad_rows)[(size_t)e * FGS_BLEND_ROW_FLOATS + col] = tot;
    };
    // what the passes of one entry read: formed for both entries of a pair before either's passes run
    struct DeadTerms {
        float ca, dya, dyb, bdya, bdyb, cyya, cyyb, dxs[NSX];
        uint32_t mxs[NSX], my0, my1, msk, cflag;
    };
    [[maybe_unused]] auto dead_terms = [&](const float4 &q0, const float4 &q1, const float4 &q2, const uint32_t fl) {
        DeadTerms t;
        t.msk = fl & alive;
        t.cflag = fl & 256u;  // clear: the clamp-gradient select (a scalar, tested where it is used: see the general walk)
        asm("" : "+s"(t.cflag));
        const uint32_t cbits = __float_as_uint(q2.z), rbits = __float_as_uint(q2.w);
        const float cbc = q0.w, cd = q1.x, lop = q1.y;
        t.ca = q0.z;
        const float dxa = fx0 - q0.x;
        t.dya = fy0 - q0.y; t.dyb = t.dya + 8.0f;
        t.bdya = cbc * t.dya; t.bdyb = cbc * t.dyb; t.cyya = fmaf(cd * t.dya, t.dya, lop); t.cyyb = fmaf(cd * t.dyb, t.dyb, lop);
        asm("" : "+v"(t.bdya), "+v"(t.bdyb), "+v"(t.cyya), "+v"(t.cyyb));
#pragma unroll
        for (int col = 0; col < NSX; ++col) {
            t.mxs[col] = (uint32_t)__builtin_amdgcn_sbfe((int)cbits, shx + 8u * col, 1);
            t.dxs[col] = dxa + 8.0f * col;
        }
        t.my0 = (uint32_t)__builtin_amdgcn_sbfe((int)rbits, shy, 1); t.my1 = (uint32_t)__builtin_amdgcn_sbfe((int)rbits, shy + 8u, 1);
        return t;
    };
    // the passes and the fold of one dead entry: its six sums {mx, my, ca, cbc, cd, op} (see the general walk for what they are)
    [[maybe_unused]] auto dead_passes = [&](const DeadTerms &t, float (&vals)[DSUMS]) {
        float v_mx = 0, v_my = 0, v_ca = 0, v_cbc = 0, v_cd = 0, v_op = 0;
        float mA[2] = {0.0f, 0.0f}, mB[2] = {0.0f, 0.0f}, mC[2] = {0.0f, 0.0f};  // per sub-tile row (ROW_MOMENTS)
        auto pass = [&](const int s) {
            const int col = s % NSX, row = s / NSX;
            const float dx = t.dxs[col], dy = row ? t.dyb : t.dya;
            const uint32_t mk = t.mxs[col] & (row ? t.my1 : t.my0);
            const float tt = __builtin_fmaf(dx, t.ca, row ? t.bdyb : t.bdya);
            const float a1 = blend_alpha1(__builtin_fmaf(tt, dx, row ? t.cyyb : t.cyya), mk);
            float dalpha = S[s] * __builtin_amdgcn_rcpf(a1 - INV_ALPHA_MAX);
            uint32_t cf = t.cflag;
            asm("" : "+s"(cf));  // an opaque scalar per use: one s_cmp + branch, nothing on the vector side
            if (!cf) dalpha = select_lt1(a1, dalpha);
            // (opaque products: under fast-math the first pass of a row, whose sums start from zero, otherwise re-associates
            // (dG dx) dx into (dx dx) dG -- another rounding than the general pass's)
            float dG = dalpha * a1;
            asm("" : "+v"(dG));
            if constexpr (ROW_MOMENTS) {
                mA[row] = __builtin_fmaf(dalpha, a1, mA[row]);
                float dmx = dG * dx;
                asm("" : "+v"(dmx));
                mB[row] = __builtin_fmaf(dG, dx, mB[row]); mC[row] = __builtin_fmaf(dmx, dx, mC[row]);
            } else {
                v_op = __builtin_fmaf(dalpha, a1, v_op);
                float dmx = dG * dx, dmy = dG * dy;
                asm("" : "+v"(dmx), "+v"(dmy));
                v_mx = __builtin_fmaf(dG, dx, v_mx); v_my = __builtin_fmaf(dG, dy, v_my);
                v_ca = __builtin_fmaf(dmx, dx, v_ca); v_cbc = __builtin_fmaf(dmx, dy, v_cbc); v_cd = __builtin_fmaf(dmy, dy, v_cd);
            }
        };
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (!((t.msk >> s) & 1u)) continue;  // scalar branch: sub-tile not touched
            pass(s);
        }
        if constexpr (ROW_MOMENTS) {  // the general walk's fold, its three dy sums written as what they contract to there
            v_op = mA[0] + mA[1]; v_mx = mB[0] + mB[1]; v_ca = mC[0] + mC[1];
            float t0 = t.dya * mA[0], t1 = t.dyb * mA[1];
            asm("" : "+v"(t0), "+v"(t1));
            float p0 = t0 * t.dya, pb = mB[0] * t.dya;
            asm("" : "+v"(p0), "+v"(pb));
            v_my = __builtin_fmaf(mA[1], t.dyb, t0);
            v_cd = __builtin_fmaf(t1, t.dyb, p0);
            v_cbc = __builtin_fmaf(mB[1], t.dyb, pb);
        }
        vals[0] = v_mx; vals[1] = v_my; vals[2] = v_ca; vals[3] = v_cbc; vals[4] = v_cd; vals[5] = v_op;
    };
    // one staged chunk of n entries.  The second record of a single entry (n odd: j + 1 = n <= CH - 1) is read from LDS like any
    // other but has no flags (no pass runs) and no row (nothing is stored).
    [[maybe_unused]] auto dead_chunk = [&](const uint32_t n) {
        for (uint32_t j = 0; j < n; j += DROWS) {
            const float4 a0 = sh0[j], a1 = sh1[j], a2 = sh2[j];
            uint32_t eA = __builtin_amdgcn_readfirstlane(she[j]), eB = ~0u;
            float4 b0 = a0, b1 = a1, b2 = a2;
            if constexpr (PAIRS) {
                b0 = sh0[j + 1]; b1 = sh1[j + 1]; b2 = sh2[j + 1];
                eB = __builtin_amdgcn_readfirstlane(she[j + 1]);
            }
            reduce_parked_dead();  // the previous round's sums
            asm volatile("" : "+s"(eA), "+s"(eB));  // taken here, with the records (see the general walk)
            const bool paired = PAIRS && j + 1 < n;
            e_prev = eA; e_prevB = paired ? eB : ~0u;
            const uint32_t flA = __builtin_amdgcn_readfirstlane(__float_as_uint(a2.w));
            const DeadTerms ta = dead_terms(a0, a1, a2, flA);
            float va[DSUMS];
            if constexpr (PAIRS) {
                const uint32_t flB = paired ? __builtin_amdgcn_readfirstlane(__float_as_uint(b2.w)) : 0u;
                const DeadTerms tb = dead_terms(b0, b1, b2, flB);
                float vb[DSUMS];
                dead_passes(ta, va);
                addtid_park(red, va);
                dead_passes(tb, vb);
                addtid_park(red + DSUMS * FGS_RED_PITCH, vb);
            } else {
                dead_passes(ta, va);
                addtid_park(red, va);
            }
        }
    };
    for (uint32_t base = c.start; base < c.end; base += CH) {
        // the list loop's trip count, pinned to an SGPR: left to itself the compiler keeps it in a VGPR (it is compared with `lane`
        // here) and counts the list loop down with a v_add_u32 / v_cmp_eq_u32 pair per entry
        const uint32_t n = __builtin_amdgcn_readfirstlane(min((uint32_t)CH, c.end - base));
        // The staging's own lane id, formed afresh per chunk behind an asm volatile so that NOTHING derived from it is loop-invariant.
        // With `lane` here the staging's LDS addresses and 64-bit index pairs are hoisted out of the chunk loop and held across the list
        // loop; at 96 VGPRs the allocator then spills them, and with them the gradient row's lane address, which it reloads INSIDE the
        // list loop (one scratch load per entry: DESIGN_LOG.md 18, 21).  Check after a compiler change: no scratch instruction in a list loop.
        uint32_t sl;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(sl));
        if (sl < n) {
            const uint32_t gid = ((FGS_BWD_G const uint32_t *)dup_ids)[base + sl];
            const float4 *r = reinterpret_cast<const float4 *>(rec + (size_t)gid * FGS_REC_FLOATS);
            float4 q2 = r[2];
            const uint32_t bbx = __float_as_uint(q2.z), bby = __float_as_uint(q2.w);
            she[sl] = fgs_emission_slot<8 * NSX>(c.tx, c.ty, gid, bbx, bby, dup_off);
            float4 q0 = r[0], q1 = r[1];
            // m = a dx^2 + (b+c) dx dy + d dy^2 >= 0 everywhere (so G <= 1): positive definite, with a margin
            // that covers the fp32 rounding of m
            const bool conic_ok = q0.z > 0.0f && q1.x > 0.0f && 3.996f * q0.z * q1.x > q0.w * q0.w;
            uint32_t flags, cbits;
            stage_decode_w<NSX>(c.X0, c.Y0, bbx, bby, q1.y, flags, cbits, conic_ok);
            // (blend_stage_fold: the forward's record, but for the floored opacities' lop -- see there, with the row contract)
            blend_stage_fold(q0, q1, q2, flags, cbits, fgs_opacity_floored(q1.y) ? FGS_FOLD_FLOOR_LOG2 : blend_lop(q1.y));
            sh0[sl] = q0; sh1[sl] = q1; sh2[sl] = q2;
        }
        __syncthreads();
        if constexpr (DEAD) dead_chunk(n);
        for (uint32_t j = 0; !DEAD && j < n; ++j) {  // the general walk's list loop
            const float4 q0 = sh0[j], q1 = sh1[j], q2 = sh2[j];
            uint32_t e = __builtin_amdgcn_readfirstlane(she[j]);
            reduce_parked();  // the previous entry's sums
            asm volatile("" : "+s"(e));  // taken here, with the record: left to the end of the entry it waits for the parking stores
            e_prev = e;
            const uint32_t fl = __builtin_amdgcn_readfirstlane(__float_as_uint(q2.w));  // stage_decode_w flags
            const uint32_t msk = fl & alive;
#ifdef FGS_BWD_UNIT_TRACE
            trace_passes += __builtin_popcount(fl & ((1u << NS) - 1u)); trace_zero_passes += __builtin_popcount(fl & bwd_trace_sub[0]);
#endif
            const uint32_t cbits = __float_as_uint(q2.z), rbits = __float_as_uint(q2.w);  // column bits; row bits at 16+
            const float ca = q0.z, cbc = q0.w, cd = q1.x, lop = q1.y;  // conic pre-multiplied by K = -log2(e)/2; log2(opacity / 0.99)
            // terms shared by the sub-tiles of a column / row, formed once per list entry; the row's term of the exponent carries lop
            const float dxa = fx0 - q0.x, dya = fy0 - q0.y, dyb = dya + 8.0f;
            float bdya = cbc * dya, bdyb = cbc * dyb, cyya = fmaf(cd * dya, dya, lop), cyyb = fmaf(cd * dyb, dyb, lop);
            asm("" : "+v"(bdya), "+v"(bdyb), "+v"(cyya), "+v"(cyyb));  // keep the row terms: do not recompute them per sub-tile
            // bbox membership: the lane's column / row bits of the staged pixel bits become all-ones / zero masks
            // (v_bfe_i32) and zero G with a bit-and -- no per-pixel compare / select (issue costs: DESIGN.md).
            // per-lane partial sums over this lane's (up to 2 NSX) pixels: moments of dG = dalpha a' about the Gaussian's mean, sum dG
            // {dx, dy, dx^2, dx dy, dy^2, 1}; the ln2 and K factors of the chain through m' = K m and the factors of the
            // row contract (blend_stage_fold) are applied once per Gaussian in k_row_sum.  ROW_MOMENTS (32 x 16 tiles): a lane's pixels lie on TWO values of dy
            // (dya, dyb: one per sub-tile row), so a pass accumulates only the row's A_r = sum dG, B_r = sum dG dx, C_r = sum dG dx^2 (five
            // ops instead of nine) and the dy factors are applied once per list entry, in the fold behind the passes:
            //   {1, dx, dx^2} = A0 + A1, B0 + B1, C0 + C1;  dy = dya A0 + dyb A1;  dx dy = dya B0 + dyb B1;
            //   dy^2 = dya (dya A0) + dyb (dyb A1).
            // Still central moments, with the pass's own dx / dy: nothing is taken about a far origin.  (RAW moments
            // about the tile origin -- one FMA each with per-lane constants -- were 4 % faster but lose the second
            // moments of sub-pixel Gaussians to cancellation in fp32: up to 4e-2 on dL/dscale in the randomized sweeps.)
            // An untouched row's sums stay zero and add exact zeros in the fold.
            float v_mx = 0, v_my = 0, v_ca = 0, v_cbc = 0, v_cd = 0, v_op = 0, v_r = 0, v_g = 0, v_b = 0, v_d = 0;
            float mA[2] = {0.0f, 0.0f}, mB[2] = {0.0f, 0.0f}, mC[2] = {0.0f, 0.0f};  // per sub-tile row (ROW_MOMENTS)
            {   // ONE code path for every kind of entry; what differs is handled by a wave-uniform branch around two
                // ops: `clamp` (flag bit 8 clear: opacity > 0.98 or a doubtful conic): the clamp-gradient select.
                // (Four specialised instantiations of this loop body made the compiler carry T and S through eight
                // v_mov per list entry and were 5 % slower.)
                uint32_t cflag = fl & 256u;  // clear: `clamp`.  Kept as a scalar and tested where it is used: as a bool the
                asm("" : "+s"(cflag));       // compiler materialised it through a v_cndmask / v_cmp pair per list entry
                // the lane masks of every entry, also of those whose bbox covers the tile (all bits set): skipping the four
                // v_bfe behind a branch needed four v_mov of the default and was 0.9 % slower
                uint32_t mxs[NSX];
                float dxs[NSX];
#pragma unroll
                for (int col = 0; col < NSX; ++col) {
                    mxs[col] = (uint32_t)__builtin_amdgcn_sbfe((int)cbits, shx + 8u * col, 1);
                    dxs[col] = dxa + 8.0f * col;
                }
                const uint32_t my0 = (uint32_t)__builtin_amdgcn_sbfe((int)rbits, shy, 1), my1 = (uint32_t)__builtin_amdgcn_sbfe((int)rbits, shy + 8u, 1);
                // One sub-tile pass.  A lambda called from the unrolled sub-tile loop, not the loop's body: the same arithmetic, but
                // the compiler then updates the sums in place (v_fmac where it had v_fma into a copy) and spills one dword of
                // k_composite_bwd<4> instead of five -- 2.9 fewer VALU instructions per list entry (DESIGN_LOG.md 17)
                auto pass = [&](const int s, const uint32_t mk) {
                    // a' is zeroed outside the bbox: w and every gradient term below then vanish by themselves
                    const int col = s % NSX, row = s / NSX;
                    const float dx = dxs[col], dy = row ? dyb : dya;
                    const float t = ca * dx + (row ? bdyb : bdya);
                    const float a1 = blend_alpha1(t * dx + (row ? cyyb : cyya), mk);  // alpha / 0.99: v_exp ... clamp, v_and
                    const float w = a1 * T[s];  // w / 0.99
                    const float q = gr[s] * q1.z + gg[s] * q1.w + gb[s] * q2.x + gd[s] * q2.y;  // 0.99 q
                    S[s] -= w * q;
                    // 0.99 dL/dalpha: 0.99 / (1 - alpha) = 1 / (1 / 0.99 - a')
                    float dalpha = T[s] * q - S[s] * __builtin_amdgcn_rcpf(INV_ALPHA_MAX - a1);
                    T[s] = fmaf(w, -ALPHA_MAX, T[s]);
                    uint32_t cf = cflag;
                    asm("" : "+s"(cf));  // an opaque scalar per use: one s_cmp + branch, nothing on the vector side
                    if (!cf) dalpha = select_lt1(a1, dalpha);  // the clamp binds where G op / 0.99 reaches 1
                    const float dG = dalpha * a1;  // op' x (0.99 dL/dalpha G): the opacity is already in the rows
                    if constexpr (ROW_MOMENTS) {
                        mA[row] += dG;
                        const float dmx = dG * dx;
                        mB[row] += dmx; mC[row] += dmx * dx;
                    } else {
                        v_op += dG;
                        const float dmx = dG * dx, dmy = dG * dy;
                        v_mx += dmx; v_my += dmy;
                        v_ca += dmx * dx; v_cbc += dmx * dy; v_cd += dmy * dy;
                    }
                    v_r += w * gr[s]; v_g += w * gg[s]; v_b += w * gb[s]; v_d += w * gd[s];
                };
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (!((msk >> s) & 1u)) continue;  // scalar branch: sub-tile not touched
                    pass(s, mxs[s % NSX] & (s / NSX ? my1 : my0));
                }
                if constexpr (ROW_MOMENTS) {  // fold the rows: once per list entry, ten ops
                    v_op = mA[0] + mA[1]; v_mx = mB[0] + mB[1]; v_ca = mC[0] + mC[1];
                    const float t0 = dya * mA[0], t1 = dyb * mA[1];
                    v_my = t0 + t1;
                    v_cd = dya * t0 + dyb * t1;
                    v_cbc = dya * mB[0] + dyb * mB[1];
                }
            }
            // ---- park the ten sums (fgs_wave.h); the next entry, or the end of the unit, adds them up over the 64 lanes in a fixed
            // order and stores them straight into this duplicate's gradient row: no atomics, bitwise reproducible ----
            {
                const float vals[10] = {v_mx, v_my, v_ca, v_cbc, v_cd, v_op, v_r, v_g, v_b, v_d};
                addtid_park(red, vals);
            }
        }
        __syncthreads();
    }
    if constexpr (DEAD) reduce_parked_dead(); else reduce_parked();  // the unit's last entry (or pair)
#ifdef FGS_BWD_UNIT_TRACE
    if (!DEAD) { bwd_trace_sub[1] = trace_passes; bwd_trace_sub[2] = trace_zero_passes; }
#endif
}

// The dead unit's walk as a function of its own, CALLED by the kernel: inlined next to the general walk it cost that walk registers
// (scratch traffic in front of every chunk, +1 % on a launch without a dead unit; DESIGN_LOG.md 21).  It needs S and the tile alone.
template <int NSX>
struct BwdDeadArgs {
    TileCtx c;
    uint32_t dcap;
    uint32_t alive;  // sub-tiles whose S is not an exact zero on every lane (all of them with FGS_BWD_ZERO_OFF): see the kernel
    const uint32_t *dup_ids; const float *rec; const uint32_t *dup_off; float *grad_rows;
    float S[2 * NSX];
};
template <int NSX>
__device__ __attribute__((noinline)) void composite_bwd_dead_walk(BwdDeadArgs<NSX> a) {
    const uint32_t lane = threadIdx.x;
    float z[2 * NSX] = {}, T[2 * NSX] = {};
    // (function arguments arrive in VGPRs: the mask is wave-uniform and goes back to an SGPR, so that the passes stay scalar branches)
    const uint32_t alive = __builtin_amdgcn_readfirstlane(a.alive);
    composite_bwd_walk<NSX, true>(a.c, lane, lane & 7u, lane >> 3, a.dcap, alive, a.dup_ids, a.rec, a.dup_off, a.grad_rows, z, z, z, z,
                                  a.S, T);
}

// ZERO UNIT (round 16): a dead unit whose S is +-0 on every lane of every sub-tile.  Its rows are written here, one lane per list
// entry, without a walk -- unless the unit is a TAIL unit of a tile that k_bwd_tail_verdict gave a rank (round 17): such a unit never
// gets here, its rows stay unwritten and k_row_sum leaves them out, which is the same sum because the rows written here are +-0 and
// k_row_sum's accumulators are never -0.  The rows are the bits composite_bwd_dead_walk gives, because in that walk every pass forms
//   dalpha = S rcp(a' - 1 / 0.99) = +-0          a' = clamp01(exp2(..)) & mask is a number in [0, 1] WHATEVER the record holds (the
//                                                 clamp turns a NaN exponent into 0), so the divisor lies in [-1.0102, -0.0101];
//   dalpha = select_lt1(..) = that or +0;  dG = dalpha a' = +-0;  every moment = fma(+-0, dx or dy, sum) with dx, dy FINITE:
//                                                 k_project lists a Gaussian only when u + r > 0, u - r < W, v + r > 0, v - r < H
//                                                 hold with r <= max_radius, which no NaN or infinite u, v passes;
// and a sum that starts at +0 stays +0 under such additions (+0 + -0 = +0 in round-to-nearest): all six sums of a lane are +0 behind
// the passes, the four colour / depth floats are the walk's stored +0.  16 x 16 tiles: the sums ARE the row's values, all +0.
// 32 x 16 tiles: the fold forms v_my = fma(mA1, dyb, dya mA0) and v_cbc = fma(mB1, dyb, mB0 dya) from sums that are +0, i.e. a sum of
// two zeros with the signs of dyb and dya: -0 on a lane with dyb < 0 (then dya < 0 too, dyb = dya + 8 being the larger), +0 elsewhere;
// v_cd = fma(dyb mA1, dyb, (dya mA0) dya) adds two squares' signs, +0, and the other three are +0 + +0.  The wave's total of a value is
// -0 exactly when every lane's is; dyb = (fy0 - v) + 8 grows with the lane's row, so that is when the lanes of the last row, ly = 7,
// have it: floats 1 and 3 of the row are -0.0f when ((float)(Y0 + 7) - v) + 8.0f < 0 in fp32, rounded as the walk rounds it, and
// everything else is +0.0f.  (An entry without a touched sub-tile runs no pass and the same fold.)
// The row's bits are stored as integers, the subtraction kept from the addition by an opaque value: this unit is compiled with
// -ffast-math, which knows no signed zero and may re-associate.  A function of its own for the reason given above.
template <int NSX>
__device__ __attribute__((noinline)) void composite_bwd_zero_rows(TileCtx c, uint32_t dcap, const uint32_t *__restrict__ dup_ids,
                                                                  const float *__restrict__ rec, const uint32_t *__restrict__ dup_off,
                                                                  float *__restrict__ grad_rows) {
    static_assert(FGS_BLEND_ROW_FLOATS % 2 == 0 && FGS_BLEND_ROW_FLOATS >= 4, "zero rows: stored as pairs, floats 1 and 3 in the first two");
    const float fy7 = (float)(c.Y0 + 7u);
    for (uint32_t i = c.start + threadIdx.x; i < c.end; i += 64) {
        const uint32_t gid = dup_ids[i];
        const float *r = rec + (size_t)gid * FGS_REC_FLOATS;
        const float4 q2 = reinterpret_cast<const float4 *>(r)[2];
        const uint32_t e = fgs_emission_slot<8 * NSX>(c.tx, c.ty, gid, __float_as_uint(q2.z), __float_as_uint(q2.w), dup_off);
        uint32_t zy = 0u;  // bits of floats 1 and 3
        if constexpr (NSX == 4) {
            float dya = fy7 - r[1];
            asm("" : "+v"(dya));
            if (dya + 8.0f < 0.0f) zy = 0x80000000u;
        }
        if (e < dcap) {
            uint2 *row = reinterpret_cast<uint2 *>(grad_rows + (size_t)e * FGS_BLEND_ROW_FLOATS);
            row[0] = make_uint2(0u, zy); row[1] = make_uint2(0u, zy);
#pragma unroll
            for (int q = 2; q < FGS_BLEND_ROW_FLOATS / 2; ++q) row[q] = make_uint2(0u, 0u);
        }
    }
}

// The per-pixel prologue of a backward unit (tile c, segment `seg`, unit = its checkpoint slot): upstream gradients, S and T of this
// lane's pixel in each of the tile's sub-tiles; returns whether an in-frame pixel of this lane restarts with T != 0.  ONE function
// for k_composite_bwd and k_bwd_tail_verdict: the verdict kernel's S and T are a unit's own, bit for bit, because they are this code.
// `kclose`: the closing slots of the tile's 16 x 16 halves (0xFFFFFFFF: none); `rebase_seg`: first segment of this segment's list
// part if its checkpoint is part-local, else seg.
template <int NSX>
__device__ __forceinline__ bool composite_bwd_prologue(const TileCtx &c, uint32_t unit, uint32_t seg, uint32_t rebase_seg,
                                                       const uint32_t (&kclose)[NSX / 2], uint32_t lane, uint32_t lx, uint32_t ly,
                                                       uint32_t W, uint32_t H, float bg0, float bg1, float bg2,
                                                       const float *__restrict__ seg_ckpt, const float *__restrict__ pix_state,
                                                       const float *__restrict__ g_rgb, const float *__restrict__ g_depth,
                                                       float (&gr)[2 * NSX], float (&gg)[2 * NSX], float (&gb)[2 * NSX],
                                                       float (&gd)[2 * NSX], float (&S)[2 * NSX], float (&T)[2 * NSX]) {
    constexpr int NS = 2 * NSX, PL = NS * 64, SLOT = 5 * PL;  // sub-tiles per tile, floats per checkpoint plane / slot
    const size_t HW = (size_t)W * H;
    bool live_px = false;  // an in-frame pixel of this lane restarts with T != 0
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const uint32_t px = c.X0 + 8u * (s % NSX) + lx, py = c.Y0 + 8u * (s / NSX) + ly;
        gr[s] = gg[s] = gb[s] = gd[s] = S[s] = 0.0f;
        T[s] = 1.0f;
        if (px < W && py < H) {
            const PixelGrad g = pixel_grad_load(pix_state, g_rgb, g_depth, c.b, HW, (size_t)py * W + px, bg0, bg1, bg2);
            gr[s] = g.gr; gg[s] = g.gg; gb[s] = g.gb; gd[s] = g.gd;
            // (Total, written out as the FMA chain it has always compiled to -- like the checkpoint sum below.  The two chains take
            // their terms in the SAME order, so a restart state that equals the final state bit for bit, with Tf = +0, gives
            // S = X - X = +0 exactly: the zero units below rest on that by construction, not on the compiler's choice)
            const float bgs = __builtin_fmaf(gb[s], bg2, __builtin_fmaf(gg[s], bg1, gr[s] * bg0));
            S[s] = __builtin_fmaf(bgs, g.Tf, __builtin_fmaf(gd[s], g.D, __builtin_fmaf(gb[s], g.Cb, __builtin_fmaf(gg[s], g.Cg, gr[s] * g.Cr))));
        }
        if (seg) {
            // restart from the forward's state in front of this segment: T, and S minus the part of Total that
            // belongs to the list entries before it.  After a depth-split forward (k_blend_fwd_parts, fwd_parts
            // waves per tile) the checkpoint of a segment inside part p > 0 is local to that part and is re-based
            // with the absolute state kept in the slot of the part's first segment.
            // CLOSED HALF (the exiting forward, k_blend_fwd_head): the half of this sub-tile stopped its walk in front of slot k =
            // kclose and left its closing state (C, A = 1.0f, D) there, absolute; its cells of the later slots are not written.
            // A unit of segment >= k restarts from slot k as it is.  Those are the bits a full walk's slots give: behind a closing
            // the state is a fixed point, so a later slot of part 0 and a later part's first slot hold the closing state itself;
            // an inner slot of a later part holds a local state (C_p, T_p, D_p) that the re-basing turns into
            // compose(closing, local) = (C + T' C_p, T' T_p, D + T' D_p) with T' = 1 - 1.0f = +0: T = +0, and C + 0 = C also in
            // sign, because the strict comparisons of the absorbing test exclude a zero accumulator on an in-frame pixel (and
            // the local state is finite: a non-finite multiplier makes the bound NaN or infinite, which closes nothing).  Lanes outside the frame carry (0, T = 1, 0) in
            // every slot either way.  Per s the half is a compile-time constant and the test a scalar one.
            const bool behind = seg >= kclose[(s % NSX) >> 1];
            const size_t own = behind ? (size_t)unit - seg + kclose[(s % NSX) >> 1] : (size_t)unit;
            BlendState st = ckpt_load<PL>(seg_ckpt + own * SLOT + s * 64 + lane);
            if (rebase_seg != seg && !behind) {
                const size_t slot = (size_t)unit - seg + rebase_seg;
                st = compose(ckpt_load<PL>(seg_ckpt + slot * SLOT + s * 64 + lane), st);
            }
            T[s] = st.T;
            // (the sum written out in the order it has always been formed in: under fast-math the compiler is free to re-associate
            // it, and did as soon as the code behind the prologue changed -- S, and every geometry row, moved by an ulp)
            S[s] -= __builtin_fmaf(gd[s], st.D, __builtin_fmaf(gb[s], st.Cb, __builtin_fmaf(gg[s], st.Cg, gr[s] * st.Cr)));
            if (px < W && py < H && T[s] != 0.0f) live_px = true;  // (a NaN checkpoint is live: the general walk carries it)
        }
    }
    return live_px;
}

// The zero-unit test of a DEAD unit (k_composite_bwd, at its call): the sub-tiles that hold an S that is not +-0 on some lane, by the
// integer test (a NaN is not a zero; lanes outside the frame hold +0).  0: a ZERO UNIT.
template <int NSX>
__device__ __forceinline__ uint32_t composite_bwd_nonzero_subtiles(const float (&S)[2 * NSX]) {
    uint32_t walk = 0u;
#pragma unroll
    for (int s = 0; s < 2 * NSX; ++s)
        if (__ballot((__float_as_uint(S[s]) & 0x7FFFFFFFu) != 0u) != 0ull) walk |= 1u << s;
    return walk;
}

// The zero sub-tiles of a GENERAL unit (k_composite_bwd, at its call; see ZERO SUB-TILES OF A GENERAL UNIT there): sub-tile s is in the
// set when no lane vetoes -- an in-frame lane whose T[s] is not +0 by its BITS (a NaN, and a -0, veto), or any lane whose S[s] is not
// +-0 by the integer test of composite_bwd_nonzero_subtiles (a NaN vetoes).  Lanes outside the frame (T = 1, S = +0) do not veto on T,
// as in the dead-unit test.  One ballot per sub-tile, in the prologue only.
template <int NSX>
__device__ __forceinline__ uint32_t composite_bwd_zero_subtiles(const TileCtx &c, uint32_t lx, uint32_t ly, uint32_t W, uint32_t H,
                                                                const float (&S)[2 * NSX], const float (&T)[2 * NSX]) {
    uint32_t zero = 0u;
#pragma unroll
    for (int s = 0; s < 2 * NSX; ++s) {
        const uint32_t px = c.X0 + 8u * (s % NSX) + lx, py = c.Y0 + 8u * (s / NSX) + ly;
        const bool veto = (px < W && py < H && __float_as_uint(T[s]) != 0u) || (__float_as_uint(S[s]) & 0x7FFFFFFFu) != 0u;
        if (__ballot(veto) == 0ull) zero |= 1u << s;
    }
    return zero;
}

// ONE VERDICT PER CLOSED TILE (round 17; FgsPlan.bwd_tail).  A TAIL unit of a tile lies behind the closing slot of EVERY 16 x 16 half
// (seg >= kclose[h] for all h, every kclose[h] a slot): its prologue restarts every sub-tile from the halves' closing slots, whatever
// its own segment -- all tail units of a tile read the same addresses, form the same S and T and reach the same zero-unit verdict
// (measured: 92 % of config 3's zero units are tail units, 26 600 prologues per launch where one per tile says it all;
// profiles/r17_ab_bwd_tail_verdict.txt).  This kernel, one wave per tile in front of k_composite_bwd, runs that prologue ONCE, for the
// tile's first tail unit, seg = max_h kclose[h], and applies the tests a unit applies: dead (every in-frame pixel restarts at
// T == +0) and S +-0 on every lane.  zero_from[tile] = the DEPTH RANK (saved.rank_of) of that unit's first list entry if they hold,
// else 0xFFFFFFFF -- also for a tile without a tail: an open half, a closing in the last segment (fwd_close says 0xFFFFFFFF), an empty
// list (every list after a capacity overflow).  Every word is written by every launch; k_bwd_tail_min then leaves each image's smallest.  A tail unit of a tile with a rank returns
// from k_composite_bwd at once and writes no rows; its entries are exactly the tile's entries of rank >= zero_from[tile] (the lists of the
// direct binning are in ascending rank), and k_row_sum leaves those rows out (fgs_project.hip).
template <int NSX>
__global__ __launch_bounds__(64) void k_bwd_tail_verdict(
    uint32_t ntiles, uint32_t tiles, uint32_t tiles_x, uint32_t W, uint32_t H, float bg0, float bg1, float bg2, uint32_t dcap,
    const uint32_t *__restrict__ counters, const uint32_t *__restrict__ seg_off, const float *__restrict__ seg_ckpt,
    const uint32_t *__restrict__ ranges, const uint32_t *__restrict__ dup_ids, const float *__restrict__ pix_state,
    const float *__restrict__ g_rgb, const float *__restrict__ g_depth, const uint32_t *__restrict__ fwd_close,
    const uint32_t *__restrict__ rank_of, uint32_t *__restrict__ zero_from) {
    constexpr int NS = 2 * NSX;
    const uint32_t tile = blockIdx.x;
    if (tile >= ntiles) return;
    const uint32_t lane = threadIdx.x;
    uint32_t verdict = 0xFFFFFFFFu;
    const TileCtx c = tile_ctx_of(tile, tiles, tiles_x, ranges, 8u * NSX);
    const uint32_t seg_len = counters[4];
    uint32_t kclose[NSX / 2], seg = 0u;
#pragma unroll
    for (int h = 0; h < NSX / 2; ++h) { kclose[h] = fwd_close[2u * tile + h]; seg = max(seg, kclose[h]); }  // an open half: 0xFFFFFFFF
    // (seg >= 1 for a closed half; the bounds below hold by the forward's construction and are tested all the same: the first entry
    // of the unit must be an entry of the list, and of the buffer)
    const uint32_t len = c.end - c.start;
    const bool tail = c.end > c.start && seg_len != 0u && seg != 0xFFFFFFFFu && seg != 0u && (unsigned long long)seg * seg_len < len &&
                      (unsigned long long)c.start + (unsigned long long)seg * seg_len < dcap;
    if (tail) {
        float gr[NS], gg[NS], gb[NS], gd[NS], S[NS], T[NS];
        const bool live_px = composite_bwd_prologue<NSX>(c, seg_off[tile] + seg, seg, seg, kclose, lane, lane & 7u, lane >> 3, W, H, bg0, bg1,
                                                         bg2, seg_ckpt, pix_state, g_rgb, g_depth, gr, gg, gb, gd, S, T);
        if (__ballot(live_px) == 0ull && composite_bwd_nonzero_subtiles<NSX>(S) == 0u) verdict = rank_of[dup_ids[c.start + seg * seg_len]];
    }
    if (lane == 0) zero_from[tile] = verdict;
}

// The smallest word of each image's tiles, behind the tiles' words: zero_from[images * tiles + b].  One block per image, behind
// k_bwd_tail_verdict.  k_row_sum looks nothing up for a Gaussian of a lower rank (every Gaussian where nothing closes).  5.4 us per
// launch at config 3 (8 blocks of 4096 words), beside 25.7 us of the verdict kernel (profiles/r17_profile_bwd_tail_verdict.txt).
__global__ __launch_bounds__(256) void k_bwd_tail_min(uint32_t tiles, uint32_t *__restrict__ zero_from) {
    __shared__ uint32_t part[4];
    const uint32_t *z = zero_from + (size_t)blockIdx.x * tiles;
    uint32_t m = 0xFFFFFFFFu;
    for (uint32_t t = threadIdx.x; t < tiles; t += 256u) m = min(m, z[t]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = min(m, (uint32_t)__shfl_xor(m, o, 64));
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) zero_from[(size_t)gridDim.x * tiles + blockIdx.x] = min(min(part[0], part[1]), min(part[2], part[3]));
}

#ifndef FGS_BWD_WIDE_WAVES
#define FGS_BWD_WIDE_WAVES 5  /* waves per SIMD of k_composite_bwd<4>; re-measured in round 3 under the clause scheduler: see DESIGN_LOG.md 10.3 */
#endif
#ifndef FGS_BWD_DYN_LDS
#define FGS_BWD_DYN_LDS 0  /* experiment builds: unused dynamic LDS per block, to cap the waves per SIMD below what the registers allow */
#endif
// Experiment builds.  FGS_BWD_TILE_ORDER: the units launch in unit (= tile) order, unit_order is not read -- the order before the
// table existed.  FGS_BWD_UNIT_TRACE: every launch slot records wall_clock64() (100 MHz) at entry and exit, its unit and whether it
// took the dead walk (1: every sub-tile, 4: some masked, 3: a zero unit's rows without a walk, 5: a tail unit that left on its tile's verdict), three 64-bit words per slot in a buffer the launcher owns; fgs_bwd_unit_trace() copies the last launch's out
// (scratch/profile/bwd_unit_drain.py turns it into the drain profile of profiles/r12_ab_bwd_unit_order.txt).
#ifdef FGS_BWD_UNIT_TRACE
#define FGS_BWD_TRACE_PARAM , unsigned long long *__restrict__ trace
#define FGS_BWD_TRACE_EXIT(dead)                                                                                        \
    do {                                                                                                                \
        if (threadIdx.x == 0) {                                                                                         \
            trace[3 * (size_t)blockIdx.x + 1] = wall_clock64();                                                         \
            trace[3 * (size_t)blockIdx.x + 2] = (unsigned long long)unit | ((unsigned long long)(dead) << 32) | (1ull << 63); \
        }                                                                                                               \
    } while (0)
#else
#define FGS_BWD_TRACE_PARAM
#define FGS_BWD_TRACE_EXIT(dead) do { } while (0)
#endif
template <int NSX>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NSX == 2 ? 6 : FGS_BWD_WIDE_WAVES, NSX == 2 ? 6 : FGS_BWD_WIDE_WAVES))) void k_composite_bwd(
    uint32_t tiles, uint32_t tiles_x, uint32_t W, uint32_t H, float bg0, float bg1, float bg2, uint32_t dcap,
    const uint32_t *__restrict__ counters, const uint32_t *__restrict__ seg_off,
    const uint32_t *__restrict__ seg_tile, const float *__restrict__ seg_ckpt, const uint32_t *__restrict__ ranges,
    const uint32_t *__restrict__ dup_ids, const float *__restrict__ rec, const uint32_t *__restrict__ dup_off,
    const float *__restrict__ pix_state, const float *__restrict__ g_rgb, const float *__restrict__ g_depth,
    float *__restrict__ grad_rows, float t_eps, const uint32_t *__restrict__ unit_order,
    const uint32_t *__restrict__ fwd_close, uint32_t zero_units, const uint32_t *__restrict__ zero_from FGS_BWD_TRACE_PARAM) {
    // work unit = (tile, depth segment): blockIdx.x indexes the unit list built by k_tile_order; the grid is
    // sized from the capacity, surplus blocks leave at once
    constexpr int NS = 2 * NSX, PL = NS * 64, SLOT = 5 * PL;  // sub-tiles per tile, floats per checkpoint plane / slot
    const uint32_t num_units = counters[2];
    if (blockIdx.x >= num_units) return;
#ifdef FGS_BWD_UNIT_TRACE
    if (threadIdx.x == 0) trace[3 * (size_t)blockIdx.x] = wall_clock64();
#endif
    // units are listed tile by tile: an XCD gets a contiguous run of them, so neighbouring tiles -- which share
    // Gaussians, and write adjacent 40-byte gradient rows -- meet in one L2.  Inside its run an XCD takes the full units first and
    // the partial ones last, longest first (unit_order, fgs_bin.hip k_unit_order): the short units fill the launch's drain
#ifdef FGS_BWD_TILE_ORDER
    const uint32_t unit = fgs_xcd_remap(blockIdx.x, num_units);
#else
    const uint32_t unit = unit_order[fgs_xcd_remap(blockIdx.x, num_units)];
#endif
    // the split the forward ran with, as the forward recorded it (k_tile_order): segment length, and the number of
    // list parts of the depth-split forward (> 1: checkpoints inside a later part are part-local)
    const uint32_t seg_len = counters[4];
    const uint32_t fwd_parts = (int32_t)counters[5] > 1 ? counters[5] : 0u;
    const uint32_t unit_tile = seg_tile[unit];
    // the closing slots of the tile's 16 x 16 halves (saved.fwd_close; null without the exiting forward: no half has one).  They
    // depend on the tile alone and are loaded here, beside seg_off and the ranges, not behind them
    uint32_t kclose[NSX / 2];
#pragma unroll
    for (int h = 0; h < NSX / 2; ++h) kclose[h] = 0xFFFFFFFFu;
    if (fwd_close) {
#pragma unroll
        for (int h = 0; h < NSX / 2; ++h) kclose[h] = fwd_close[2u * unit_tile + h];
    }
    const uint32_t seg = unit - seg_off[unit_tile];
    // TAIL UNIT (FgsPlan.bwd_tail; zero_from is null without it): behind the closing slot of EVERY half of its tile (an open half's
    // 0xFFFFFFFF is behind no segment).  k_bwd_tail_verdict ran this unit's prologue -- the one every tail unit of the tile runs -- and
    // left a rank where the unit is a zero unit: it then writes no rows (k_row_sum does not read them) and leaves here.  A tail
    // unit of a tile whose verdict was no, and every other unit, goes on as it always did.
    if (zero_from) {
        bool tail = true;
#pragma unroll
        for (int h = 0; h < NSX / 2; ++h) tail = tail && seg >= kclose[h];
        if (tail && zero_from[unit_tile] != 0xFFFFFFFFu) {
            FGS_BWD_TRACE_EXIT(5);
            return;
        }
    }
    TileCtx c = tile_ctx_of(unit_tile, tiles, tiles_x, ranges, 8u * NSX);
    uint32_t rebase_seg = seg;  // first segment of this segment's list part if its checkpoint is part-local
    if (fwd_parts > 1) {
        const uint32_t nseg = (c.end - c.start + seg_len - 1) / seg_len;
        const uint32_t spp = (nseg + fwd_parts - 1) / fwd_parts, first = seg / spp * spp;
        if (first != 0) rebase_seg = first;
    }
    c.start += seg * seg_len;
    c.end = min(c.end, c.start + seg_len);
    const uint32_t lane = threadIdx.x;
    const uint32_t lx = lane & 7u, ly = lane >> 3;
    if (t_eps > 0.0f) {
        // FgsDims.saturation_skip: the forward stopped walking this tile's list after `live` segments (count
        // parked in the checkpoint slot of segment 0); the entries of a dead segment get all-zero gradient rows
        const uint32_t live = reinterpret_cast<const uint32_t *>(seg_ckpt + (size_t)seg_off[unit_tile] * SLOT)[0];
        if (seg >= live) {
            for (uint32_t i = c.start + lane; i < c.end; i += 64) {
                const uint32_t gid = dup_ids[i];
                const float4 q2 = reinterpret_cast<const float4 *>(rec + (size_t)gid * FGS_REC_FLOATS)[2];
                const uint32_t e = fgs_emission_slot<8 * NSX>(c.tx, c.ty, gid, __float_as_uint(q2.z), __float_as_uint(q2.w), dup_off);
                if (e < dcap) {
                    float2 *row = reinterpret_cast<float2 *>(grad_rows + (size_t)e * FGS_BLEND_ROW_FLOATS);
#pragma unroll
                    for (int q = 0; q < FGS_BLEND_ROW_FLOATS / 2; ++q) row[q] = make_float2(0.0f, 0.0f);
                }
            }
            FGS_BWD_TRACE_EXIT(2);
            return;
        }
    }
    // T: running transmittance (w = alpha T, T -= w: one instruction less per pixel than T = 1 - A, A += w)
    // S: T_fin (gI.bg) + sum over not-yet-visited w q
    float gr[NS], gg[NS], gb[NS], gd[NS], S[NS], T[NS];
    const bool live_px = composite_bwd_prologue<NSX>(c, unit, seg, rebase_seg, kclose, lane, lx, ly, W, H, bg0, bg1, bg2, seg_ckpt, pix_state,
                                                     g_rgb, g_depth, gr, gg, gb, gd, S, T);
    // DEAD UNIT: every in-frame pixel of the tile restarts with T == +0.0f (the forward's A rounded to 1.0f: its T <= 2^-25) and
    // keeps it for the whole unit (fma(+0, -0.99, +0) = +0).  Lanes outside the frame (T = 1, g = 0, S = 0) do not veto: the
    // bboxes are clipped to the frame (k_project), so stage_decode_w's column / row bits mask their a' to zero and they add
    // exact zeros in either walk.  Never with FgsDims.saturation_skip, never for a tile's first segment (T = 1).
    const bool dead_unit = seg != 0 && !(t_eps > 0.0f) && __ballot(live_px) == 0ull;
    uint32_t alive = (1u << NS) - 1u;  // sub-tiles still composited (FgsDims.saturation_skip; 16 x 16 tiles only)
    if (t_eps > 0.0f) {
        alive = 0u;
#pragma unroll
        for (int s = 0; s < NS; ++s)
            if (__ballot(T[s] >= t_eps) != 0ull) alive |= 1u << s;  // T = 1 - A of the checkpoint, as in the forward
    }
    if (dead_unit) {
        // Which sub-tiles of the dead unit hold an S that is not +-0 on some lane (a NaN is not a zero; lanes outside the frame hold
        // +0).  dalpha = -(S r) is the ONLY thing a dead pass gives its sums, so a sub-tile without such a lane adds exact zeros and
        // its passes are left out (sums that start at +0 keep their bits); a unit without any is a ZERO UNIT and gets its rows from
        // composite_bwd_zero_rows.  The test reads the bits the walk would multiply by -- it does not ask WHY S is zero (the unit
        // lies behind its halves' closings: see DEAD UNITS above; or no gradient reaches the pixels).
        uint32_t walk = (1u << NS) - 1u;
        if (zero_units & 1u) {
            walk = composite_bwd_nonzero_subtiles<NSX>(S);
            if (walk == 0u) {
                composite_bwd_zero_rows<NSX>(c, dcap, dup_ids, rec, dup_off, grad_rows);
                FGS_BWD_TRACE_EXIT(3);
                return;
            }
        }
        BwdDeadArgs<NSX> a;
        a.c = c; a.dcap = dcap; a.alive = walk; a.dup_ids = dup_ids; a.rec = rec; a.dup_off = dup_off; a.grad_rows = grad_rows;
#pragma unroll
        for (int s = 0; s < NS; ++s) a.S[s] = S[s];
        composite_bwd_dead_walk<NSX>(a);
        FGS_BWD_TRACE_EXIT(walk == (1u << NS) - 1u ? 1 : 4);
        return;
    }
    // ZERO SUB-TILES OF A GENERAL UNIT (round 18; bit 1 of zero_units = FgsPlan.bwd_sub): they leave `alive`, which the list loop
    // applies to every entry's flags anyway -- the loop itself is the parent's.  Never for segment 0, never with saturation_skip.
#ifdef FGS_BWD_UNIT_TRACE
    bwd_trace_sub[0] = seg != 0 && !(t_eps > 0.0f) ? composite_bwd_zero_subtiles<NSX>(c, lx, ly, W, H, S, T) : 0u;
#endif
    if ((zero_units & 2u) && seg != 0 && !(t_eps > 0.0f)) alive &= ~composite_bwd_zero_subtiles<NSX>(c, lx, ly, W, H, S, T);
    composite_bwd_walk<NSX, false>(c, lane, lx, ly, dcap, alive, dup_ids, rec, dup_off, grad_rows, gr, gg, gb, gd, S, T);
    FGS_BWD_TRACE_EXIT((unsigned long long)bwd_trace_sub[1] << 3 | (unsigned long long)bwd_trace_sub[2] << 16 | (unsigned long long)(bwd_trace_sub[0] != 0u) << 29);
}

// ---------------------------------------------------------------------------------------------------------------------
// Phase-blending path (BASELINE config 4).  alpha_i depends on the running weighted-mean phase
// Phi_{i-1} (DR:629-667): a true recurrence per pixel, a serial cos / divide chain -- latency-bound, so the unit of work is
// small: ONE WAVE PER 8 x 8 SUB-TILE (four per 16 x 16 tile, in one block so that they share the tile's list through the
// CU's caches), and -- round 4 -- the four waves no longer share anything else:
//   * every wave scans the tile's list 64 entries at a time, tests the bboxes against ITS sub-tile and parks only the
//     records that touch it, COMPACTED and in list order, in wave-private LDS (ballot + mbcnt).  No block barrier in the list
//     walk (round 3: one per 64 entries, the four waves of a tile waiting for the slowest), no scalar mask walk over
//     untouched entries;
//   * checkpoints (A, Phi) for the backward are taken every FGS_PHASE_CKPT TOUCHED entries of a scan block (round 3: every 8
//     list positions that held at least one touched entry -- at ~40 % touched entries that was 7.9 checkpoints per 64
//     entries for 3.2 entries each; now ceil(25 / 8) ~ 3.6): half the checkpoint traffic and twice the entries per
//     restart.  Slot of group g of the scan block at list offset o: start / 8 + o / 8 + g + tile (g < 8: the capacity
//     of fgs_make_plan is unchanged), plane w = A of sub-tile w, plane 4 + w = Phi.
// bbox membership is a per-lane bit-and with masks from the staged column / row bits (v_bfe_i32), as on the blend path.
#ifndef FGS_PHASE_SCAN
#define FGS_PHASE_SCAN 64  /* list entries per scan block (a multiple of FGS_PHASE_CKPT, <= 64) */
#endif
static_assert(FGS_PHASE_SCAN <= 64 && FGS_PHASE_SCAN % FGS_PHASE_CKPT == 0, "scan block");
#ifndef FGS_PHASE_WAVE_BLOCKS
#define FGS_PHASE_WAVE_BLOCKS 0  /* 1 (experiment): every sub-tile wave is a workgroup of its own -- see phase_wave_block */
#endif
// FGS_PHASE_WAVE_BLOCKS: grid = 4 x (tiles rounded up to 8) single-wave blocks.  Blocks are dealt round-robin over the 8 XCDs;
// block L serves launch slot (L / 32) * 8 + L % 8 as sub-tile wave (L / 8) % 4, so the four waves of a tile land on ONE XCD
// (they share the tile's list through its L2) and consecutive slots of the heavy-first order spread over all eight.
__device__ __forceinline__ bool phase_wave_block(uint32_t total_slots, uint32_t &slot, uint32_t &wave) {
    const uint32_t L = blockIdx.x;
    slot = (L >> 5) * 8u + (L & 7u);
    wave = (L >> 3) & 3u;
    return slot < total_slots;
}
struct PhaseRec {                 // one compacted list entry in wave-private LDS
    float4 a[FGS_PHASE_SCAN];     // u, v, conic a, conic b + c
    float4 b[FGS_PHASE_SCAN];     // conic d, opacity, colour r, g
    float4 c[FGS_PHASE_SCAN];     // colour b, depth, phase, pixel bits (bits 0-7: columns sx + i inside the bbox, 8-15: rows sy + i)
};

// scan step shared by the two kernels: lane j < n looks at list entry base + j; returns the ballot of the entries that touch
// the sub-tile at (sx, sy) and parks those, compacted, in `st`.  K = factor on the conic (forward: exp2 units)
template <bool FWD>
__device__ __forceinline__ unsigned long long phase_scan(PhaseRec &st, uint32_t *rows, uint32_t gid, bool have, uint32_t sx,
                                                         uint32_t sy, const TileCtx &c,
                                                         const float *__restrict__ rec, const float *__restrict__ phase,
                                                         const uint32_t *__restrict__ dup_off) {
    float4 q0, q1, q2;
    uint32_t bits = 0, e = 0;
    if (have) {
        const float4 *r = reinterpret_cast<const float4 *>(rec + (size_t)gid * FGS_REC_FLOATS);
        q0 = r[0]; q1 = r[1]; q2 = r[2];
        const uint32_t bbx = __float_as_uint(q2.z), bby = __float_as_uint(q2.w);
        const int x0 = (int)(bbx & 0xFFFFu), x1 = (int)(bbx >> 16), y0 = (int)(bby & 0xFFFFu), y1 = (int)(bby >> 16);
        const int lx0 = max(x0 - (int)sx, 0), lx1 = min(x1 - (int)sx, 8), ly0 = max(y0 - (int)sy, 0), ly1 = min(y1 - (int)sy, 8);
        const uint32_t cm = lx1 > lx0 ? ((1u << (lx1 - lx0)) - 1u) << lx0 : 0u;
        const uint32_t rm = ly1 > ly0 ? ((1u << (ly1 - ly0)) - 1u) << ly0 : 0u;
        bits = (cm && rm) ? (cm | (rm << 8)) : 0u;
        // this duplicate's emission slot: its four gradient rows (one per sub-tile wave) are 4 e .. 4 e + 3 (k_project_bwd)
        if (!FWD) e = fgs_emission_slot<FGS_TILE>(c.tx, c.ty, gid, bbx, bby, dup_off);
    }
    const unsigned long long touched = __ballot(bits != 0u);
    if (bits) {
        const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(touched >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)touched, 0u));
        // conic in exp2 units, forward AND backward (round 5: the backward's re-run and reverse sweep then evaluate G with the forward's
        // own operation order -- and one multiply less per evaluation)
        q0.z *= NEG_HALF_LOG2E; q0.w *= NEG_HALF_LOG2E; q1.x *= NEG_HALF_LOG2E;
        st.a[slot] = q0; st.b[slot] = q1;
        st.c[slot] = make_float4(q2.x, q2.y, phase[gid], __uint_as_float(bits));
        if (!FWD) rows[slot] = e;
    }
    __builtin_amdgcn_wave_barrier();  // wave-private LDS: one wave's LDS instructions execute in order
    return touched;
}

// One step of the phase recurrence (DR:629-667) at this lane's pixel (fpx, fpy) = sub-tile pixel (lx, ly), for the parked entry
// (q0, q1, q2) of a PhaseRec: advances (A, Ph) and returns w = alpha (1 - A_{i-1}).  Called by the forward AND by the re-run loop of
// the backward, whose adjoint is exact only because its re-run reproduces the forward's (A_{i-1}, Phi_{i-1}) to the bit.  (The
// backward's reverse sweep keeps its own code: it needs the intermediates.)
// One source is necessary for that, NOT sufficient: this unit is built with -ffast-math, and the order in which the compiler sums the
// three terms of mm follows the order of the loads around the call.  Both callers therefore read the record into locals first and pass
// those; called on the LDS references directly, the re-run rounded c dy before (b + c) dx, the forward the other way round, and the
// gradients moved by an ulp or two (DESIGN_LOG.md 19).  After a change here, compare both kernels' exponent code or their outputs.
__device__ __forceinline__ float phase_step(const float4 &q0, const float4 &q1, const float4 &q2, uint32_t lx, uint32_t ly, float fpx,
                                            float fpy, float base_amp, float amp, float &A, float &Ph) {
    const uint32_t bits = __float_as_uint(q2.w);
    const uint32_t mk = (uint32_t)__builtin_amdgcn_sbfe((int)bits, lx, 1) & (uint32_t)__builtin_amdgcn_sbfe((int)bits, 8u + ly, 1);
    const float dx = fpx - q0.x, dy = fpy - q0.y;
    const float mm = (q0.z * dx) * dx + (q0.w * dx) * dy + (q1.x * dy) * dy;  // conic staged in exp2 units
    float alpha = __builtin_amdgcn_exp2f(mm) * q1.y;
    float pd = fabsf(q2.z - Ph);
    pd = fminf(pd, 1.0f - pd);
    alpha *= base_amp + amp * phase_cos(pd * PHASE_KAPPA);
    alpha = __builtin_amdgcn_fmed3f(alpha, 0.0f, ALPHA_MAX);
    alpha = __uint_as_float(__float_as_uint(alpha) & mk);   // zero outside the bbox: w = pc = 0, nothing moves
    const float w = alpha * (1.0f - A);
    A += w;
    const float pc = w / fmaxf(A, 1e-6f);
    Ph = Ph * (1.0f - pc) + q2.z * pc;
    return w;
}

__global__ __launch_bounds__(FGS_PHASE_WAVE_BLOCKS ? 64 : 256) void k_phase_fwd(
    uint32_t tiles, uint32_t tiles_x, uint32_t W, uint32_t H, float bg0, float bg1, float bg2, float amp,
    const uint32_t *__restrict__ tile_order, const uint32_t *__restrict__ ranges, const uint32_t *__restrict__ dup_ids,
    const float *__restrict__ rec, const float *__restrict__ phase, float *__restrict__ pix_state,
    float *__restrict__ phase_ckpt, float *__restrict__ out_rgb, float *__restrict__ out_depth, uint32_t total_slots) {
    constexpr int PCK = FGS_PHASE_CKPT;
    __shared__ PhaseRec st4[FGS_PHASE_WAVE_BLOCKS ? 1 : 4];
#if FGS_PHASE_WAVE_BLOCKS
    uint32_t pslot, wave;
    if (!phase_wave_block(total_slots, pslot, wave)) return;
    const TileCtx c = tile_ctx_of(tile_order[pslot], tiles, tiles_x, ranges);
    const uint32_t lane = threadIdx.x & 63u;
    PhaseRec &st = st4[0];
#else
    const TileCtx c = tile_ctx(tiles, tiles_x, tile_order, ranges);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    PhaseRec &st = st4[wave];
#endif
    const uint32_t lx = lane & 7u, ly = lane >> 3;
    const uint32_t sx = c.X0 + 8u * (wave & 1u), sy = c.Y0 + 8u * (wave >> 1);
    float fpx = (float)(sx + lx), fpy = (float)(sy + ly);
    asm("" : "+v"(fpx), "+v"(fpy));  // hoisted for good: no v_cvt in the list loop
    float A = 0.0f, Ph = 0.0f, Cr = 0.0f, Cg = 0.0f, Cb = 0.0f, Dm = 0.0f;
    const float base_amp = 1.0f - amp;
    constexpr uint32_t SCAN = FGS_PHASE_SCAN;
    uint32_t gid_next = (lane < SCAN && c.start + lane < c.end) ? dup_ids[c.start + lane] : 0u;
    for (uint32_t base = c.start; base < c.end; base += SCAN) {
        const uint32_t gid = gid_next;
        const bool have = lane < SCAN && base + lane < c.end;
        if (lane < SCAN && base + SCAN + lane < c.end) gid_next = dup_ids[base + SCAN + lane];  // the next block's ids travel under this one's work
        const unsigned long long touched = phase_scan<true>(st, nullptr, gid, have, sx, sy, c, rec, phase, nullptr);
        const uint32_t nt = (uint32_t)__popcll(touched);
        for (uint32_t j0 = 0; j0 < nt; j0 += PCK) {
            const size_t slot = (size_t)(c.start / PCK) + (base - c.start + j0) / PCK + c.tile;
            float *ck = phase_ckpt + slot * 512 + lane;
            ck[wave * 64] = A; ck[(4 + wave) * 64] = Ph;
            const uint32_t m = min((uint32_t)PCK, nt - j0);
#pragma unroll
            for (int k = 0; k < PCK; ++k) {
                if (k >= (int)m) break;  // wave-uniform
                const float4 q0 = st.a[j0 + k], q1 = st.b[j0 + k], q2 = st.c[j0 + k];
                const float w = phase_step(q0, q1, q2, lx, ly, fpx, fpy, base_amp, amp, A, Ph);
                Cr += w * q1.z; Cg += w * q1.w; Cb += w * q2.x; Dm += w * q2.y;
            }
        }
        __builtin_amdgcn_wave_barrier();  // the next scan block overwrites the parked records
    }
    const uint32_t px = sx + lx, py = sy + ly;
    if (px < W && py < H) {
        const size_t HW = (size_t)W * H, o = (size_t)py * W + px;
        pixel_store(pix_state, out_rgb, out_depth, c.b, HW, o, bg0, bg1, bg2, Cr, Cg, Cb, A, 1.0f - A, Dm);
        nt_store(pix_state + (size_t)c.b * 6 * HW + o + 5 * HW, Ph);
    }
}

// (Round 5 measured and removed three experiment switches of this kernel -- parking G / the interference factor in the re-run, checkpoint
// groups of sixteen, the re-run interleaved with the sweep: profiles/r05_ab_phase_variants.txt; the code of the first two is in commit c134f2a.)
// Backward of the phase recurrence (the reference cannot backprop this path at all, §0.6 -- the contract is the
// exact adjoint of the forward recurrence DR:629-667).  The recurrence cannot be inverted back-to-front, so the wave walks
// its sub-tile's touched entries in REVERSE checkpoint groups: re-runs the forward inside a group from the group's (A, Phi)
// checkpoint, keeping (A_{i-1}, Phi_{i-1}) of its entries in registers (both loops over a group are fully unrolled), then
// sweeps the group back-to-front with the per-pixel adjoints Abar (init -gI.bg) and Phibar.  Every touched (entry, sub-tile)
// gets its OWN gradient row (row 4 e + w; k_project_bwd repeats the integer test and never reads the rows of untouched
// sub-tiles): no cross-wave reduction.
__global__ __launch_bounds__(FGS_PHASE_WAVE_BLOCKS ? 64 : 256) void k_phase_bwd(
    uint32_t tiles, uint32_t tiles_x, uint32_t W, uint32_t H, float bg0, float bg1, float bg2, float amp,
    uint32_t dcap, const uint32_t *__restrict__ tile_order, const uint32_t *__restrict__ ranges,
    const uint32_t *__restrict__ dup_ids, const float *__restrict__ rec, const float *__restrict__ phase,
    const uint32_t *__restrict__ dup_off, const float *__restrict__ pix_state,
    const float *__restrict__ phase_ckpt, const float *__restrict__ g_rgb, const float *__restrict__ g_depth,
    float *__restrict__ grad_rows, uint32_t total_slots) {
    constexpr int PCK = FGS_PHASE_CKPT;
    constexpr int NWB = FGS_PHASE_WAVE_BLOCKS ? 1 : 4;
    __shared__ PhaseRec st4[NWB];
    __shared__ uint32_t rows4[NWB][FGS_PHASE_SCAN];
    __shared__ __attribute__((aligned(16))) float red4[NWB][11 * FGS_RED_PITCH];  // reduction scratch, one per wave
#if FGS_PHASE_WAVE_BLOCKS
    uint32_t pslot, wave;
    if (!phase_wave_block(total_slots, pslot, wave)) return;
    const TileCtx c = tile_ctx_of(tile_order[pslot], tiles, tiles_x, ranges);
    const uint32_t lane = threadIdx.x & 63u;
    PhaseRec &st = st4[0];
    uint32_t *rows = rows4[0];
    float *red = red4[0];
#else
    const TileCtx c = tile_ctx(tiles, tiles_x, tile_order, ranges);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    PhaseRec &st = st4[wave];
    uint32_t *rows = rows4[wave];
    float *red = red4[wave];
#endif
    const uint32_t lx = lane & 7u, ly = lane >> 3;
    const size_t HW = (size_t)W * H;
    const uint32_t sx = c.X0 + 8u * (wave & 1u), sy = c.Y0 + 8u * (wave >> 1);
    const uint32_t px = sx + lx, py = sy + ly;
    float fpx = (float)px, fpy = (float)py;
    asm("" : "+v"(fpx), "+v"(fpy));
    float gr = 0.0f, gg = 0.0f, gb = 0.0f, gd = 0.0f, Abar = 0.0f, Pbar = 0.0f;
    if (px < W && py < H) {
        const PixelGrad g = pixel_grad_load(pix_state, g_rgb, g_depth, c.b, HW, (size_t)py * W + px, bg0, bg1, bg2);
        gr = g.gr; gg = g.gg; gb = g.gb; gd = g.gd;
        Abar = -(gr * bg0 + gg * bg1 + gb * bg2);  // d/dA of (1 - A) * bg
    }
    const float base_amp = 1.0f - amp, neg_amp_kappa = -(amp * PHASE_KAPPA);
    const uint32_t total = c.end - c.start;
    constexpr uint32_t SCAN = FGS_PHASE_SCAN;
    const uint32_t nblocks = (total + SCAN - 1u) / SCAN;
    uint32_t gid_next = 0u;
    if (nblocks) {
        const uint32_t i = c.start + (nblocks - 1u) * SCAN + lane;
        if (lane < SCAN && i < c.end) gid_next = dup_ids[i];
    }
    for (uint32_t bi = nblocks; bi-- > 0;) {
        const uint32_t base = c.start + bi * SCAN;
        const uint32_t gid = gid_next;
        const bool have = lane < SCAN && base + lane < c.end;
        if (bi && lane < SCAN) gid_next = dup_ids[base - SCAN + lane];  // the block in front of this one: always full
        const unsigned long long touched = phase_scan<false>(st, rows, gid, have, sx, sy, c, rec, phase, dup_off);
        const uint32_t nt = (uint32_t)__popcll(touched);
        const uint32_t ngroups = (nt + PCK - 1) / PCK;
        for (uint32_t g = ngroups; g-- > 0;) {
            const uint32_t j0 = g * PCK;
            const uint32_t m = min((uint32_t)PCK, nt - j0);
            const size_t slot = (size_t)(c.start / PCK) + (bi * SCAN + j0) / PCK + c.tile;
            const float *ck = phase_ckpt + slot * 512 + lane;
            float Af = ck[wave * 64], Pf = ck[(4 + wave) * 64];
            // ---- forward re-run of the group: park (A_{i-1}, Phi_{i-1}) ----
            float sA[PCK], sP[PCK];
#pragma unroll
            for (int k = 0; k < PCK; ++k) {
                sA[k] = 0.0f; sP[k] = 0.0f;
                if (k >= (int)m) continue;  // wave-uniform
                const float4 q0 = st.a[j0 + k], q1 = st.b[j0 + k], q2 = st.c[j0 + k];
                sA[k] = Af; sP[k] = Pf;
                phase_step(q0, q1, q2, lx, ly, fpx, fpy, base_amp, amp, Af, Pf);
            }
            // ---- reverse sweep of the group ----
#pragma unroll
            for (int k = PCK - 1; k >= 0; --k) {
                if (k >= (int)m) continue;  // wave-uniform
                const float4 q0 = st.a[j0 + k], q1 = st.b[j0 + k], q2 = st.c[j0 + k];
                const uint32_t e = rows[j0 + k];
                const uint32_t bits = __float_as_uint(q2.w);
                const uint32_t mk = (uint32_t)__builtin_amdgcn_sbfe((int)bits, lx, 1) & (uint32_t)__builtin_amdgcn_sbfe((int)bits, 8u + ly, 1);
                const float ca = q0.z, cbc = q0.w, cd = q1.x, op = q1.y, ph = q2.z;
                const float Aprev = sA[k], Pprev = sP[k];
                const float dx = fpx - q0.x, dy = fpy - q0.y;
                const float dphi = ph - Pprev;
                const float pd0 = fabsf(dphi);
                const float pd = fminf(pd0, 1.0f - pd0);
                // G zeroed outside the bbox: raw, alpha, w, pc and every gradient term of this pixel then vanish by themselves
                const float mm = (ca * dx) * dx + (cbc * dx) * dy + (cd * dy) * dy;
                const float G = __uint_as_float(__float_as_uint(__builtin_amdgcn_exp2f(mm)) & mk);
                const float inter = base_amp + amp * phase_cos(pd * PHASE_KAPPA);
                // (parking G and `inter` of the re-run instead of recomputing them costs 14 VGPRs = one wave per SIMD and
                // was 7 % slower in round 2: this kernel lives on occupancy)
                const float Gop = G * op, Gint = G * inter;
                const float raw = Gop * inter;
                const float alpha = __builtin_amdgcn_fmed3f(raw, 0.0f, ALPHA_MAX);
                const float T = 1.0f - Aprev;
                const float w = alpha * T;
                const float Ai = Aprev + w;
                const float rA = __builtin_amdgcn_rcpf(fmaxf(Ai, 1e-6f));
                const float pc = w * rA;
                const float Pb = __uint_as_float(__float_as_uint(Pbar) & mk);  // Phibar reaches this entry only inside its bbox
                float v_ph = Pb * pc;
                const float pcbar = Pb * dphi;
                // d pc/d w, direct (1/A_i) plus through A_i (-w/A_i^2), equals A_{i-1}/A_i^2: kept in that cancellation-free
                // form (the two parts cancel to ~0 for a pixel's first contribution)
                // (below the 1e-6 clamp of A_i, pc = w / 1e-6: d pc/d w = 1 / 1e-6 = rA and no dependence on A_{i-1}; selected per lane
                // -- a divergent branch cost a save / restore of the exec mask per entry)
                const float rA2 = rA * rA;
                float dpc_dw, dpc_dA;
                select2_ge(Ai, 1e-6f, Aprev * rA2, w * rA2, rA, dpc_dw, dpc_dA);  // (one compare, both selects adjacent: issue costs)
                const float wbar = Abar + (gr * q1.z + gg * q1.w + gb * q2.x + gd * q2.y) + pcbar * dpc_dw;
                const float v_r = w * gr, v_g = w * gg, v_b = w * gb, v_d = w * gd;
                const float abar = wbar * T;
                Abar = (Abar - pcbar * dpc_dA) - wbar * alpha;  // (outside the bbox: w = alpha = pcbar = 0, Abar unchanged)
                // clamp passes the gradient on the closed interval [0, 0.99]: exactly where clamping changed nothing (alpha == raw;
                // one compare instead of two)
                const float rbar = select_eq(alpha, raw, abar);
                const float v_op = rbar * Gint;
                const float pdbar = (rbar * Gop) * neg_amp_kappa * phase_sin(PHASE_KAPPA * pd);
                // d pd/d dphi = sign(1/2 - |dphi|) sign(dphi), 0 on either tie: the sign of x = (1/2 - |dphi|) dphi, formed by saturating
                // x 2^100 to [-1, 1] (exactly +-1 for |x| >= 2^-100, exactly 0 for x = 0; four compares and four selects before round 5).
                // (pd0 < 1 - pd0 is pd0 < 1/2 for every fp32 pd0 in [0, 1]: 1 - pd0 rounds to >= 1/2 below one half and is exact above.)
                const float t_ph = pdbar * __builtin_amdgcn_fmed3f(((0.5f - pd0) * dphi) * 1.2676506e30f, -1.0f, 1.0f);
                v_ph += t_ph;
                Pbar -= Pb * pc + t_ph;  // = Pb (1 - pc) - pd0bar sg inside the bbox, unchanged outside (Pb = G = 0 there)
                const float dm = rbar * raw;  // -2 dL/dm: the -1/2 rides on the per-Gaussian sums (k_project_bwd)
                const float dmx = dm * dx, dmy = dm * dy;
                // slots 0 / 1: the FIRST MOMENTS of dL/dm; k_project_bwd turns their per-Gaussian sums into those of dL/dm' (m' = K m, the
                // blend path's convention: x 1 / K = -2 ln2, once per Gaussian since round 5) and forms dL/d(u, v) = -K conic_sym (moments)
                // in double (the same chain as the blend backward's rows)
                const float vals[11] = {dmx, dmy, dmx * dx, dmx * dy, dmy * dy, v_op, v_r, v_g, v_b, v_d, v_ph};  // (slots 0-4: moments of -2 dL/dm, rescaled in k_project_bwd)
                const float tot = wave_sum_addtid<11>(red, vals, lane);
                if ((lane & 3u) == 3u && lane < 44u && e < dcap)
                    grad_rows[((size_t)e * 4 + wave) * FGS_GROW_FLOATS + (lane >> 2)] = tot;
            }
        }
        __builtin_amdgcn_wave_barrier();  // the next scan block overwrites the parked records
    }
}

}  // namespace

// Kernel variants are template instantiations selected by the plan (fgs_make_plan: FgsPlan.fwd_parts / fwd_waves,
// a pure function of the FgsDims; FgsDims.fwd_variant overrides for A/B runs and the variant-agreement tests).
// typed pointer at a byte offset of a workspace (FgsSavedLayout offsets into `saved`, FgsPlan.s_* into `scratch`)
template <typename T>
static T *fgs_at(const char *base, size_t offset) {
    return reinterpret_cast<T *>(const_cast<char *>(base) + offset);
}

// List entries of part 0 that k_blend_fwd_head walks at most (in whole segments, one at least).  The halves of the benchmark scenes
// that close at all close within 384 entries (DESIGN_LOG.md 24); a longer head only lengthens the launch for scenes that never do.
#ifndef FGS_FWD_HEAD_ENTRIES
#define FGS_FWD_HEAD_ENTRIES 384u
#endif

int fgs_launch_composite_fwd(const FgsPlan &p, const float *phase, char *saved, float *out_rgb,
                             float *out_depth, hipStream_t st) {
    const uint32_t grid = (uint32_t)p.d.batch * p.tiles;
    const uint32_t tiles = (uint32_t)p.tiles, tiles_x = (uint32_t)p.L.tiles_x, W = (uint32_t)p.d.width, H = (uint32_t)p.d.height;
    const float bg0 = p.d.background[0], bg1 = p.d.background[1], bg2 = p.d.background[2];
    const uint32_t *ranges = fgs_at<const uint32_t>(saved, p.L.ranges), *dup_ids = fgs_at<const uint32_t>(saved, p.L.dup_ids);
    const uint32_t *tile_order = fgs_at<const uint32_t>(saved, p.L.tile_order), *seg_off = fgs_at<const uint32_t>(saved, p.L.seg_off);
    const float *rec = fgs_at<const float>(saved, p.L.rec);
    float *pix = fgs_at<float>(saved, p.L.pix_state), *seg_ckpt = fgs_at<float>(saved, p.L.seg_ckpt);
    if (p.d.use_phase) {  // one wave per 8 x 8 sub-tile, four per block
        float *phase_ckpt = fgs_at<float>(saved, p.L.phase_ckpt);
        hipLaunchKernelGGL(k_phase_fwd, dim3(FGS_PHASE_WAVE_BLOCKS ? (grid + 7u) / 8u * 32u : grid), dim3(FGS_PHASE_WAVE_BLOCKS ? 64 : 256), 0, st,
                           tiles, tiles_x, W, H, bg0, bg1, bg2, p.d.phase_amplitude, tile_order, ranges, dup_ids, rec, phase, pix,
                           phase_ckpt, out_rgb, out_depth, grid);
        FGS_LAUNCH_CHECK("k_phase_fwd");
        return FGS_OK;
    }
    const float t_eps = p.d.saturation_skip ? FGS_SATURATION_EPS : 0.0f;
    const int fw = p.fwd_waves;
    if (const int np = p.fwd_parts) {
        const uint32_t seg_len = (uint32_t)p.L.seg_len, order_groups = (uint32_t)p.order_groups;
        // The exiting forward: the head kernel (one wave per tile half over the front of part 0), then the parts kernel for the
        // halves it left open.  One part: the head walks the whole list and there is nothing left.
        const bool exiting = p.fwd_exit;
        const uint32_t prewalk = p.fwd_prewalk ? 1u : 0u;  // only with `exiting` and np > 1 (fgs_make_plan)
        uint32_t *fwd_open = exiting ? fgs_at<uint32_t>(saved, p.L.fwd_open) : nullptr;
        const uint32_t head_segs = FGS_FWD_HEAD_ENTRIES / seg_len > 0u ? FGS_FWD_HEAD_ENTRIES / seg_len : 1u;
        if (exiting) {
            const uint32_t *fwd_max = fgs_at<const uint32_t>(saved, p.s_fwd_max);
            const uint32_t max_recs = ((uint32_t)p.d.num_gaussians + 255u) / 256u;
            uint32_t *fwd_close = fgs_at<uint32_t>(saved, p.L.fwd_close);
            // the pre-walk blocks (FgsPlan.fwd_prewalk) stand behind the head blocks, from the next multiple of 8 on: per XCD
            // ceil(grid / 8) launch slots x (np - 1) parts; the surplus ones leave at once
            uint32_t head_grid = grid;
            if (prewalk) {
                const uint64_t want = (uint64_t)((grid + 7u) & ~7u) + (uint64_t)((grid + 7u) / 8u) * 8u * (uint32_t)(np - 1);
                if (want > 0x7FFFFFFFull) { fgs_set_error("k_blend_fwd_head: the pre-walk grid exceeds 2^31 blocks"); return FGS_EINVAL; }
                head_grid = (uint32_t)want;
            }
#define FGS_HEAD_LAUNCH(WD)                                                                                               \
    hipLaunchKernelGGL((k_blend_fwd_head<WD>), dim3(head_grid), dim3(64 * (1 + WD)), 0, st, tiles, tiles_x, W, H, bg0, bg1, bg2, tile_order, \
                       ranges, dup_ids, rec, pix, out_rgb, out_depth, seg_off, seg_ckpt, seg_len, order_groups, fwd_open, head_segs, \
                       (uint32_t)np, fwd_max, max_recs, fwd_close, grid)
            if (p.tile_w == 32) FGS_HEAD_LAUNCH(1); else FGS_HEAD_LAUNCH(0);
#undef FGS_HEAD_LAUNCH
            FGS_LAUNCH_CHECK("k_blend_fwd_head");
            if (np == 1) return FGS_OK;
        }
#define FGS_PARTS_LAUNCH(NP, WD)                                                                                          \
    do {                                                                                                                  \
        if (exiting)                                                                                                      \
            hipLaunchKernelGGL((k_blend_fwd_parts<NP, WD, true>), dim3(grid), dim3(64 * NP * (1 + WD)), 0, st, tiles, tiles_x, W, H, bg0, \
                               bg1, bg2, tile_order, ranges, dup_ids, rec, pix, out_rgb, out_depth, seg_off, seg_ckpt, seg_len,   \
                               order_groups, fwd_open, head_segs, prewalk);                                                        \
        else                                                                                                              \
            hipLaunchKernelGGL((k_blend_fwd_parts<NP, WD, false>), dim3(grid), dim3(64 * NP * (1 + WD)), 0, st, tiles, tiles_x, W, H, bg0, \
                               bg1, bg2, tile_order, ranges, dup_ids, rec, pix, out_rgb, out_depth, seg_off, seg_ckpt, seg_len,   \
                               order_groups, fwd_open, head_segs, prewalk);                                                        \
    } while (0)
        if (p.tile_w == 32) {
            if (np == 1) FGS_PARTS_LAUNCH(1, 1); else if (np == 2) FGS_PARTS_LAUNCH(2, 1); else if (np == 4) FGS_PARTS_LAUNCH(4, 1);
            else FGS_PARTS_LAUNCH(8, 1);
        } else {
            if (np == 1) FGS_PARTS_LAUNCH(1, 0); else if (np == 2) FGS_PARTS_LAUNCH(2, 0); else if (np == 4) FGS_PARTS_LAUNCH(4, 0);
            else if (np == 8) FGS_PARTS_LAUNCH(8, 0); else FGS_PARTS_LAUNCH(16, 0);
        }
#undef FGS_PARTS_LAUNCH
        FGS_LAUNCH_CHECK("k_blend_fwd_parts");
        return FGS_OK;
    }
#define FGS_FWD_LAUNCH(FW, SK)                                                                                            \
    hipLaunchKernelGGL((k_composite_fwd<FW, SK>), dim3(grid), dim3(64 * FW), 0, st, tiles, tiles_x, W, H, bg0, bg1, bg2, tile_order, \
                       ranges, dup_ids, rec, pix, out_rgb, out_depth, seg_off, seg_ckpt, t_eps)
    if (t_eps > 0.0f) {  // FgsDims.saturation_skip: separate instantiation, the default path carries no trace of it
        if (fw == 1) FGS_FWD_LAUNCH(1, true); else if (fw == 4) FGS_FWD_LAUNCH(4, true); else FGS_FWD_LAUNCH(2, true);
    } else {
        if (fw == 1) FGS_FWD_LAUNCH(1, false); else if (fw == 4) FGS_FWD_LAUNCH(4, false); else FGS_FWD_LAUNCH(2, false);
    }
#undef FGS_FWD_LAUNCH
    FGS_LAUNCH_CHECK("k_composite_fwd");
    return FGS_OK;
}

#ifdef FGS_BWD_UNIT_TRACE
static unsigned long long *g_bwd_trace = nullptr;
static uint32_t g_bwd_trace_slots = 0, g_bwd_trace_last = 0;
// experiment builds only: the records of the last k_composite_bwd launch, three words per launch slot (entry clock, exit clock,
// unit | walk << 32 | 1 << 63; all zero for the surplus slots); returns the number of slots copied, or -1
extern "C" long fgs_bwd_unit_trace(unsigned long long *host, size_t slots) {
    if (!g_bwd_trace || hipDeviceSynchronize() != hipSuccess) return -1;
    const size_t n = slots < g_bwd_trace_last ? slots : g_bwd_trace_last;
    if (hipMemcpy(host, g_bwd_trace, n * 24, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (long)n;
}
#endif

int fgs_launch_composite_bwd(const FgsPlan &p, const float *phase, const char *saved, char *scratch,
                             const float *g_rgb, const float *g_depth, float *g_phase, hipStream_t st) {
    (void)g_phase;  // dL/dphase travels in the gradient rows and is written by k_project_bwd
    const uint32_t grid = (uint32_t)p.d.batch * p.tiles;
    const uint32_t tiles = (uint32_t)p.tiles, tiles_x = (uint32_t)p.L.tiles_x, W = (uint32_t)p.d.width, H = (uint32_t)p.d.height;
    const uint32_t dcap = (uint32_t)p.L.dup_capacity;
    const float bg0 = p.d.background[0], bg1 = p.d.background[1], bg2 = p.d.background[2];
    const uint32_t *ranges = fgs_at<const uint32_t>(saved, p.L.ranges), *dup_ids = fgs_at<const uint32_t>(saved, p.L.dup_ids);
    const uint32_t *dup_off = fgs_at<const uint32_t>(saved, p.L.dup_off);
    const float *rec = fgs_at<const float>(saved, p.L.rec), *pix = fgs_at<const float>(saved, p.L.pix_state);
    float *grad_rows = fgs_at<float>(scratch, p.s_grows);
    if (p.d.use_phase) {
        const uint32_t *tile_order = fgs_at<const uint32_t>(saved, p.L.tile_order);
        const float *phase_ckpt = fgs_at<const float>(saved, p.L.phase_ckpt);
        hipLaunchKernelGGL(k_phase_bwd, dim3(FGS_PHASE_WAVE_BLOCKS ? (grid + 7u) / 8u * 32u : grid), dim3(FGS_PHASE_WAVE_BLOCKS ? 64 : 256), 0, st,
                           tiles, tiles_x, W, H, bg0, bg1, bg2, p.d.phase_amplitude, dcap, tile_order, ranges, dup_ids, rec, phase,
                           dup_off, pix, phase_ckpt, g_rgb, g_depth, grad_rows, grid);
        FGS_LAUNCH_CHECK("k_phase_bwd");
        return FGS_OK;
    }
    const uint32_t ugrid = (uint32_t)p.L.seg_capacity;  // surplus blocks exit at once (measured: free)
    const uint32_t *counters = fgs_at<const uint32_t>(saved, p.L.counters), *seg_off = fgs_at<const uint32_t>(saved, p.L.seg_off);
    const uint32_t *seg_tile = fgs_at<const uint32_t>(saved, p.L.seg_tile);
    const float *seg_ckpt = fgs_at<const float>(saved, p.L.seg_ckpt);
    const float t_eps = p.d.saturation_skip ? FGS_SATURATION_EPS : 0.0f;
    if (!p.has_unit_order) { fgs_set_error("k_composite_bwd: the plan has no unit_order table"); return FGS_EINVAL; }
    const uint32_t *unit_order = fgs_at<const uint32_t>(saved, p.L.unit_order);
    // the closing slots of the exiting forward's closed halves; null where that forward did not run (the plan is a pure function of
    // the dims: the forward's choice)
    const uint32_t *fwd_close = p.fwd_exit ? fgs_at<const uint32_t>(saved, p.L.fwd_close) : nullptr;
    // one verdict per closed tile, in front of the units (FgsPlan.bwd_tail): every word of zero_from is written by this launch
    uint32_t *zero_from = p.bwd_tail ? fgs_at<uint32_t>(scratch, p.s_zero_from) : nullptr;
    if (zero_from) {
        const uint32_t *rank_of = fgs_at<const uint32_t>(saved, p.L.rank_of);
#define FGS_VERDICT_LAUNCH(NSXV)                                                                                          \
    hipLaunchKernelGGL(k_bwd_tail_verdict<NSXV>, dim3(grid), dim3(64), 0, st, grid, tiles, tiles_x, W, H, bg0, bg1, bg2, dcap, counters, \
                       seg_off, seg_ckpt, ranges, dup_ids, pix, g_rgb, g_depth, fwd_close, rank_of, zero_from)
        if (p.tile_w == 32) FGS_VERDICT_LAUNCH(4); else FGS_VERDICT_LAUNCH(2);
#undef FGS_VERDICT_LAUNCH
        FGS_LAUNCH_CHECK("k_bwd_tail_verdict");
        hipLaunchKernelGGL(k_bwd_tail_min, dim3((uint32_t)p.d.batch), dim3(256), 0, st, tiles, zero_from);
        FGS_LAUNCH_CHECK("k_bwd_tail_min");
    }
#ifdef FGS_BWD_UNIT_TRACE
    if (g_bwd_trace_slots < ugrid) {
        if (g_bwd_trace) (void)hipFree(g_bwd_trace);
        g_bwd_trace = nullptr; g_bwd_trace_slots = 0;
        if (hipMalloc(&g_bwd_trace, (size_t)ugrid * 24) != hipSuccess) { fgs_set_error("unit trace: hipMalloc"); return FGS_ELAUNCH; }
        g_bwd_trace_slots = ugrid;
    }
    if (hipMemsetAsync(g_bwd_trace, 0, (size_t)ugrid * 24, st) != hipSuccess) { fgs_set_error("unit trace: memset"); return FGS_ELAUNCH; }
    g_bwd_trace_last = ugrid;
#define FGS_BWD_TRACE_ARG , g_bwd_trace
#else
#define FGS_BWD_TRACE_ARG
#endif
#define FGS_BWD_LAUNCH(NSXV)                                                                                              \
    hipLaunchKernelGGL(k_composite_bwd<NSXV>, dim3(ugrid), dim3(64), FGS_BWD_DYN_LDS, st, tiles, tiles_x, W, H, bg0, bg1, bg2, dcap, \
                       counters, seg_off, seg_tile, seg_ckpt, ranges, dup_ids, rec, dup_off, pix, g_rgb, g_depth, grad_rows, t_eps, unit_order, fwd_close, \
                       (uint32_t)p.bwd_zero | (p.bwd_sub ? 2u : 0u) /* zero_units: bit 0 zero rows, bit 1 zero sub-tiles of general units */, (const uint32_t *)zero_from FGS_BWD_TRACE_ARG)
    if (p.tile_w == 32) FGS_BWD_LAUNCH(4); else FGS_BWD_LAUNCH(2);
#undef FGS_BWD_LAUNCH
#undef FGS_BWD_TRACE_ARG
    FGS_LAUNCH_CHECK("k_composite_bwd");
    return FGS_OK;
}
