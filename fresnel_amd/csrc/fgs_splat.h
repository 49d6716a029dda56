// What the two splat renderers share: the angular-spectrum renderer (fgs_asm.hip) and the WaveFieldRenderer
// (fgs_wavefield.hip).  The order-independent splat k_asm_splat<BWD, WAVE, NP> and its two host launchers, the phasor
// table, asm_plane_empty, the two-level per-image reductions, and the small host helpers of both plans.
// NOT here: anything only one renderer uses (transfer functions, transforms, output stages -- they look alike but round
// differently on purpose) and no non-template __global__: it would be emitted into both units' code objects.
// Everything sits in an anonymous namespace: each including unit gets its own copy, compiled with that unit's flags
// (build.py gives both the same: SPLAT_FLAGS).
#pragma once
#include "fgs_internal.h"
#include "fgs_wave.h"

namespace {

// an (image, plane) pair -- or, with `tiles` = lists per image, an image -- with no list entry at all: seg_off is the
// exclusive scan of every list's depth-segment count in key order (key = (b P + p) T + t; k_tile_post writes it on both
// list-building paths, [lists + 1] entries), so a key range without entries is a range without units.  (NOT `ranges`: the
// radix path leaves the ranges of empty lists zeroed.)
__device__ __forceinline__ bool asm_plane_empty(const uint32_t *__restrict__ seg_off, uint32_t bp, uint32_t tiles) {
    return seg_off[(size_t)(bp + 1u) * tiles] == seg_off[(size_t)bp * tiles];
}

constexpr float NEG_HALF_LOG2E = -0.72134752044448170368f;
constexpr int ACH = 64;
constexpr int ASM_FWD_PARTS = 4;  // list parts (waves) per (image, plane, tile) in the forward splat
constexpr uint32_t ASM_ONE_WAVE_LISTS = 24576;  // from this many lists per launch on: one wave per list in the forward splat (measured: 16 384 lists 0.105 ms with four parts vs 0.139 with one, 131 072 lists 0.83 vs 0.345)
constexpr int RED_BLOCKS = 128;   // blocks (= partials) per image of the per-image scalar reductions, see below

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

int check_ptrs(const void *const *ptrs, int n, const char *who) {
    for (int i = 0; i < n; ++i)
        if (!ptrs[i]) { fgs_set_error("%s: null pointer argument #%d", who, i); return FGS_EINVAL; }
    return FGS_OK;
}

// the FgsDims of the projection + binning plan under a splat renderer (no phase blending, every other tuning field automatic)
FgsDims splat_base_dims(int32_t batch, int32_t num_gaussians, int32_t width, int32_t height, float max_radius,
                        const float background[3], int32_t num_cameras, int32_t bin_mode) {
    FgsDims d{};
    d.batch = batch; d.num_gaussians = num_gaussians; d.width = width; d.height = height;
    d.max_radius = max_radius;
    for (int i = 0; i < 3; ++i) d.background[i] = background[i];
    d.use_phase = 0; d.phase_amplitude = 0.0f; d.num_cameras = num_cameras;
    d.bin_mode = bin_mode;
    return d;
}

// ccs[g] = (c_r cos phi_r, c_g cos phi_g, c_b cos phi_b, c_r sin phi_r | c_g sin phi_g, c_b sin phi_b, 0, 0)  DR:1274-1283
__device__ __forceinline__ void asm_phasors_block(uint32_t blk, uint32_t total, int phase_channels,
                                                  const float *__restrict__ color, const float *__restrict__ phase,
                                                  float *__restrict__ ccs) {
    const uint32_t g = blk * 256 + threadIdx.x;
    if (g >= total) return;
    float cc[3], cs[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float ph = phase_channels == 3 ? phase[3 * (size_t)g + c] : phase[g];
        float sn, co;
        sincosf(ph, &sn, &co);
        const float col = color[3 * (size_t)g + c];
        cc[c] = col * co; cs[c] = col * sn;
    }
    float4 *o = reinterpret_cast<float4 *>(ccs + (size_t)g * 8);
    o[0] = make_float4(cc[0], cc[1], cc[2], cs[0]);
    o[1] = make_float4(cs[1], cs[2], 0.0f, 0.0f);
}

// One wave per (image, plane, tile); lane = one pixel of each of the four 8x8 sub-tiles.
// BWD = false: accumulate field += a * c * (cos phi, sin phi) with a = exp(-m/2) * opacity (DR:1263-1283).
// BWD = true : read the field gradient and reduce the twelve per-Gaussian sums into a gradient row.
// WAVE = true (WaveFieldRenderer, DR:832-891): a single layer, and additionally the amplitude-weighted
// depth sums (sum a*depth, sum a) in `dw`; gradient rows are 16 floats wide (slot 12 = dL/ddepth).
// NP = waves per block of the forward (list parts), 1 for the backward.  `ccs` = the Gaussians' phasors c cos(phi),
// c sin(phi) per channel ([B*N][8] floats, k_asm_phasors): the accurate sincosf runs once per Gaussian instead of three
// times per (tile, plane) duplicate at staging time, forward and backward.
template <bool BWD, bool WAVE, int NP>
__global__ __launch_bounds__(64 * NP) void k_asm_splat(
    uint32_t tiles, uint32_t tiles_x, uint32_t P, uint32_t W, uint32_t H, uint32_t dcap,
    const uint32_t *__restrict__ tile_order, const uint32_t *__restrict__ ranges,
    const uint32_t *__restrict__ dup_ids, const float *__restrict__ rec, const float *__restrict__ ccs,
    const uint32_t *__restrict__ dup_off, float2 *__restrict__ field, float *__restrict__ grad_rows,
    float2 *__restrict__ dw, const uint32_t *__restrict__ counters, const uint32_t *__restrict__ seg_off,
    const uint32_t *__restrict__ seg_tile, uint32_t seg_len) {
    // Forward: the splat is a plain sum, so the list is cut into NP parts, one per wave (own LDS staging, no block
    // barrier in the walk) and the partial fields are added in part order at the end -- a launch of few, long lists is
    // latency-bound by the longest (NP = 4); a launch with enough lists to fill the chip (the ASM renderer's (image,
    // plane, tile) lists of a few dozen entries) runs one wave per list with 4 KB of LDS instead of 35 (NP = 1).
    // Backward: one wave per depth-segment unit.
    static_assert(!BWD || NP == 1, "the backward is one wave per unit");
    __shared__ float4 sh0[NP * ACH], sh1[NP * ACH], sh2[NP * ACH], sh3[NP * ACH];
    __shared__ uint32_t shm[NP * ACH], she[BWD ? ACH : 1];
    __shared__ float part[NP == 1 ? 1 : (NP - 1) * (WAVE ? 32 : 24) * 64];
    __shared__ __attribute__((aligned(16))) float red[BWD ? 13 * FGS_RED_PITCH : 4];  // wave_sum_addtid scratch (backward)
    // Forward: one block per (image, plane, tile), longest lists first.  Backward: the splat carries no state
    // along a list, so the work unit is a depth segment of FGS_SEG list entries (unit list of k_tile_order;
    // the grid is sized from the capacity, surplus blocks leave at once) -- balanced however uneven the lists.
    uint32_t key, seg = 0;
    if (BWD) {
        const uint32_t nunits = counters[2];
        if (blockIdx.x >= nunits) return;
        // units in DESCENDING key order: the row transform in front of this kernel wrote the planes in ascending order, the last
        // 256 MB of them are still in the memory-side cache (-1 %: the kernel is VALU-bound)
        const uint32_t unit = nunits - 1u - blockIdx.x;
        key = seg_tile[unit];
        seg = unit - seg_off[key];
    } else {
#ifdef FGS_SPLAT_ORDER_GROUPS
        key = tile_order ? tile_order[NP == 1 ? fgs_xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x] : blockIdx.x;  // (b*P + p)*T + t
#else
        key = tile_order ? tile_order[blockIdx.x] : blockIdx.x;  // (b*P + p)*T + t
#endif
    }
    const uint32_t bp = key / tiles, t = key - bp * tiles;
    const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
    const uint32_t X0 = tx * FGS_TILE, Y0 = ty * FGS_TILE;
    const uint32_t lane = threadIdx.x & 63u, lx = lane & 7u, ly = lane >> 3;
    const uint32_t wave = NP > 1 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0u;
    const uint32_t wofs = wave * ACH;  // this wave's slice of the staging arrays
    float fx0 = (float)(X0 + lx), fy0 = (float)(Y0 + ly);
    asm("" : "+v"(fx0), "+v"(fy0));  // hoisted for good
    uint32_t start = ranges[2 * key] + seg * seg_len;
    uint32_t end = BWD ? min(ranges[2 * key + 1], start + seg_len) : ranges[2 * key + 1];
    if (NP > 1) {  // this wave's part of the list (whole chunks)
        const uint32_t per = ((end - start + NP * ACH - 1) / (NP * ACH)) * ACH;
        start = min(end, start + wave * per);
        end = min(end, start + per);
    }
    const size_t HW = (size_t)W * H;
    float2 *fbase = field + (size_t)bp * 3 * HW;  // [b][p][c][y][x]
    float re[4][3], im[4][3];  // FWD: accumulators.  BWD: field gradient at this lane's pixels
    float wd[4], ww[4];        // WAVE: sum a*depth, sum a   (BWD: their gradients)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const uint32_t px = X0 + 8u * (s & 1) + lx, py = Y0 + 8u * (s >> 1) + ly;
        wd[s] = 0.0f; ww[s] = 0.0f;
        if (WAVE && BWD && px < W && py < H) {
            const float2 g = dw[(size_t)bp * HW + (size_t)py * W + px];
            wd[s] = g.x; ww[s] = g.y;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            re[s][c] = 0.0f; im[s][c] = 0.0f;
            if (BWD && px < W && py < H) {
                const float2 g = fbase[(size_t)c * HW + (size_t)py * W + px];
                re[s][c] = g.x; im[s][c] = g.y;
            }
        }
    }
    for (uint32_t base = start; base < end; base += ACH) {
        const uint32_t n = min((uint32_t)ACH, end - base);
        if (lane < n) {
            const uint32_t gid = dup_ids[base + lane];
            const float4 *r = reinterpret_cast<const float4 *>(rec + (size_t)gid * FGS_REC_FLOATS);
            const float4 q0 = r[0], q1 = r[1], q2 = r[2];
            const uint32_t bbx = __float_as_uint(q2.z), bby = __float_as_uint(q2.w);
            // touched sub-tiles + the pixel bits of the tile (bit i: column X0 + i inside the bbox, bit 16 + i: row Y0 + i): in the
            // list loop a lane turns its column / row bits into all-ones / zero masks (v_bfe_i32) and and-s them onto G -- no
            // per-pixel compare / select, as on the blend path (issue costs: DESIGN.md section 4)
            uint32_t sflags, cbits;
            stage_decode_w<2>(X0, Y0, bbx, bby, 1.0f, sflags, cbits);
            const uint32_t pbits = cbits | (sflags & 0xFFFF0000u);
            shm[wofs + lane] = sflags & 15u;
            if (BWD) she[lane] = fgs_emission_slot<FGS_TILE>(tx, ty, gid, bbx, bby, dup_off);
            const float4 *pz = reinterpret_cast<const float4 *>(ccs + (size_t)gid * 8);
            const float4 z0 = pz[0], z1 = pz[1];  // cc[0..2], cs[0] | cs[1..2]
            // conic pre-multiplied by K = -log2(e) / 2: G = exp2(K m) without a multiply per pixel (the backward's
            // dL/dconic = -1/2 dG/dm' ... is formed from the unscaled moments, below)
            sh0[wofs + lane] = make_float4(q0.x, q0.y, q0.z * NEG_HALF_LOG2E, q0.w * NEG_HALF_LOG2E);  // u, v, K ca, K cbc
            sh1[wofs + lane] = make_float4(q1.x * NEG_HALF_LOG2E, q1.y, __uint_as_float(pbits), 0.0f);   // K cd, op, pixel bits
            sh2[wofs + lane] = z0;
            sh3[wofs + lane] = make_float4(z1.x, z1.y, q2.y, 0.0f);  // .z = depth (WAVE)
        }
        __builtin_amdgcn_wave_barrier();  // wave-private staging: one wave's LDS instructions execute in order
        for (uint32_t j = 0; j < n; ++j) {
            const float4 q0 = sh0[wofs + j], q1 = sh1[wofs + j], q2 = sh2[wofs + j], q3 = sh3[wofs + j];
            const uint32_t msk = __builtin_amdgcn_readfirstlane(shm[wofs + j]);
            const uint32_t pbits = __float_as_uint(q1.z);
            const uint32_t mxs[2] = {(uint32_t)__builtin_amdgcn_sbfe((int)pbits, lx, 1), (uint32_t)__builtin_amdgcn_sbfe((int)pbits, lx + 8u, 1)};
            const uint32_t mys[2] = {(uint32_t)__builtin_amdgcn_sbfe((int)pbits, 16u + ly, 1), (uint32_t)__builtin_amdgcn_sbfe((int)pbits, 24u + ly, 1)};
            const float ca = q0.z, cbc = q0.w, cd = q1.x, op = q1.y;
            const float cc[3] = {q2.x, q2.y, q2.z}, cs[3] = {q2.w, q3.x, q3.y};
            float v_u = 0, v_v = 0, v_ca = 0, v_cbc = 0, v_cd = 0, v_op = 0, v_dep = 0;
            float v_cc[3] = {0, 0, 0}, v_cs[3] = {0, 0, 0};
            const float dz = q3.z;
            // the lane's two column / row offsets once per entry (no int -> float conversion in the list loop)
            const float dxs[2] = {fx0 - q0.x, fx0 + 8.0f - q0.x}, dys[2] = {fy0 - q0.y, fy0 + 8.0f - q0.y};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (!((msk >> s) & 1u)) continue;
                const float dx = dxs[s & 1], dy = dys[s >> 1];
                // (this unit is compiled with -ffp-contract=off -- build.py -- so the FMAs of the two VALU-bound loops, this one and
                // the column butterflies of fgs_colfft.h, are written out: sums of same-signed or well-separated terms, where
                // fusing is harmless; measured: dL/dlambda of K5 / G9 / G16 unchanged, config 5 back from 1.99 to 1.89 ms)
                const float m = fmaf(ca * dx, dx, fmaf(cbc * dx, dy, (cd * dy) * dy));  // K m
                const float G = __uint_as_float(__float_as_uint(__builtin_amdgcn_exp2f(m)) & (mxs[s & 1] & mys[s >> 1]));
                const float a = G * op;  // amplitude, DR:1270-1271 (no clamp on this path)
                if (!BWD) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) { re[s][c] = fmaf(a, cc[c], re[s][c]); im[s][c] = fmaf(a, cs[c], im[s][c]); }
                    if (WAVE) { wd[s] = fmaf(a, dz, wd[s]); ww[s] += a; }  // DR:890-891
                } else {
                    float da = 0.0f;
                    if (WAVE) { da = fmaf(wd[s], dz, ww[s]); v_dep = fmaf(a, wd[s], v_dep); }
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        da = fmaf(cc[c], re[s][c], fmaf(cs[c], im[s][c], da));
                        v_cc[c] = fmaf(a, re[s][c], v_cc[c]); v_cs[c] = fmaf(a, im[s][c], v_cs[c]);
                    }
                    // moments of t = dL/da G about the Gaussian's mean: {1, dx, dy, dx^2, dx dy, dy^2}.  The chain through
                    // a = G op and m (dL/dm = -1/2 t op; dL/d(u, v) = -dL/dm (2 ca dx + cbc dy, cbc dx + 2 cd dy), linear in the
                    // first moments) is applied once per Gaussian, in double, by k_project_bwd: 7 VALU per pass instead of 13
                    const float t = da * G;
                    v_op += t;
                    const float tx = t * dx, ty = t * dy;
                    v_u += tx; v_v += ty;
                    v_ca = fmaf(tx, dx, v_ca); v_cbc = fmaf(tx, dy, v_cbc); v_cd = fmaf(ty, dy, v_cd);
                }
            }
            if (BWD) {
                constexpr int NV = WAVE ? 13 : 12;
                float vals[NV] = {v_u, v_v, v_ca, v_cbc, v_cd, v_op, v_cc[0], v_cc[1], v_cc[2], v_cs[0], v_cs[1], v_cs[2]};
                if (WAVE) vals[NV - 1] = v_dep;
                const float tot = wave_sum_addtid<NV>(red, vals, lane);  // conflict-free parking, as in the blend backward
                const uint32_t e = she[j];
                if ((lane & 3u) == 3u && lane < 4u * NV && e < dcap)
                    grad_rows[(size_t)e * (WAVE ? 16 : FGS_GROW_FLOATS) + (lane >> 2)] = tot;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (!BWD && NP > 1) {
        // add the partial fields in part order (wave 0 = part 0 accumulates parts 1, 2, ...): deterministic
        constexpr int NF = WAVE ? 32 : 24;
        if (wave != 0) {
            float *pp = part + ((size_t)(wave - 1) * NF) * 64 + lane;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int c = 0; c < 3; ++c) { pp[(s * 6 + c) * 64] = re[s][c]; pp[(s * 6 + 3 + c) * 64] = im[s][c]; }
                if (WAVE) { pp[(24 + 2 * s) * 64] = wd[s]; pp[(25 + 2 * s) * 64] = ww[s]; }
            }
        }
        __syncthreads();
        if (wave != 0) return;
        for (int w = 1; w < NP; ++w) {
            const float *pp = part + ((size_t)(w - 1) * NF) * 64 + lane;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int c = 0; c < 3; ++c) { re[s][c] += pp[(s * 6 + c) * 64]; im[s][c] += pp[(s * 6 + 3 + c) * 64]; }
                if (WAVE) { wd[s] += pp[(24 + 2 * s) * 64]; ww[s] += pp[(25 + 2 * s) * 64]; }
            }
        }
    }
    if (!BWD) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint32_t px = X0 + 8u * (s & 1) + lx, py = Y0 + 8u * (s >> 1) + ly;
            if (px < W && py < H) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    fbase[(size_t)c * HW + (size_t)py * W + px] = make_float2(re[s][c], im[s][c]);
                if (WAVE) dw[(size_t)bp * HW + (size_t)py * W + px] = make_float2(wd[s], ww[s]);
            }
        }
    }
}

// ---- per-image scalars (maximum, dL/dM, number of maxima, dL/dlambda) as TWO-LEVEL reductions -------------------
// One partial per block, RED_BLOCKS blocks per image; the consumers' blocks fold the partials themselves (one value per
// thread, fixed order).  Round 1 reduced these with one device-scope atomic per wave on a single address per image;
// such atomics serialise at ~50 ns each on this part: k_asm_output_bwd1 took 54 us for one image and 419 us for
// eight, k_asm_max 26 / 191 us -- both read 6-9 MB per image -- and the float sums came out in arrival order.

__device__ __forceinline__ float block_max_256(float v) {  // all 256 threads call; every thread gets the result
    __shared__ float wmax[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    __syncthreads();  // (protects wmax against the previous use)
    if ((threadIdx.x & 63u) == 0) wmax[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}
__device__ __forceinline__ float2 block_sum2_256(float a, float b) {  // fixed order: xor tree, then waves 0..3
    __shared__ float2 wsum[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
    __syncthreads();
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = make_float2(a, b);
    __syncthreads();
    return make_float2((wsum[0].x + wsum[1].x) + (wsum[2].x + wsum[3].x), (wsum[0].y + wsum[1].y) + (wsum[2].y + wsum[3].y));
}
// maximum of an image's RED_BLOCKS block maxima (every thread of the block gets it)
__device__ __forceinline__ float image_max(const float *__restrict__ pmax, int b) {
    static_assert(RED_BLOCKS <= 256, "one partial per thread");
    return block_max_256(threadIdx.x < RED_BLOCKS ? pmax[(size_t)b * RED_BLOCKS + threadIdx.x] : 0.0f);
}

// (gM, count) of image b from the block partials (every thread of the block gets them)
__device__ __forceinline__ float2 image_sums(const float2 *__restrict__ psum, int b) {
    const float2 v = threadIdx.x < RED_BLOCKS ? psum[(size_t)b * RED_BLOCKS + threadIdx.x] : make_float2(0.0f, 0.0f);
    return block_sum2_256(v.x, v.y);
}


// ---- host launchers of k_asm_splat (the callers check the launch: FGS_LAUNCH_CHECK under their own kernel names) ----
// Forward: one block per (image, plane, tile) list of the binning in `sv`; one wave per list once the launch has enough
// lists to fill the chip, else four list parts per list.  `dw`: WAVE only.
template <bool WAVE>
void launch_splat_fwd(const FgsPlan &base, char *sv, uint32_t P, const float *ccs, float2 *field, float2 *dw, hipStream_t st) {
    const uint32_t grid = (uint32_t)base.d.batch * P * (uint32_t)base.tiles;
    const bool one_wave = grid >= ASM_ONE_WAVE_LISTS;
    auto *kernel = one_wave ? k_asm_splat<false, WAVE, 1> : k_asm_splat<false, WAVE, ASM_FWD_PARTS>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * (one_wave ? 1 : ASM_FWD_PARTS)), 0, st, (uint32_t)base.tiles,
                       (uint32_t)base.L.tiles_x, P, (uint32_t)base.d.width, (uint32_t)base.d.height,
                       (uint32_t)base.L.dup_capacity, reinterpret_cast<const uint32_t *>(sv + base.L.tile_order),
                       reinterpret_cast<const uint32_t *>(sv + base.L.ranges),
                       reinterpret_cast<const uint32_t *>(sv + base.L.dup_ids),
                       reinterpret_cast<const float *>(sv + base.L.rec), ccs,
                       reinterpret_cast<const uint32_t *>(sv + base.L.dup_off), field, (float *)nullptr, dw,
                       (const uint32_t *)nullptr, (const uint32_t *)nullptr, (const uint32_t *)nullptr, 0u);
}

// Backward: one wave per depth-segment unit (the grid is sized from the capacity); `field` holds the field gradient, `dw`
// (WAVE only) the gradient of the depth sums; gradient rows -> `rows`.
template <bool WAVE>
void launch_splat_bwd(const FgsPlan &base, char *sv, uint32_t P, const float *ccs, float2 *field, float *rows, float2 *dw,
                      hipStream_t st) {
    const uint32_t grid = (uint32_t)base.L.seg_capacity;  // depth-segment units
    hipLaunchKernelGGL((k_asm_splat<true, WAVE, 1>), dim3(grid), dim3(64), 0, st, (uint32_t)base.tiles,
                       (uint32_t)base.L.tiles_x, P, (uint32_t)base.d.width, (uint32_t)base.d.height,
                       (uint32_t)base.L.dup_capacity, reinterpret_cast<const uint32_t *>(sv + base.L.tile_order),
                       reinterpret_cast<const uint32_t *>(sv + base.L.ranges),
                       reinterpret_cast<const uint32_t *>(sv + base.L.dup_ids),
                       reinterpret_cast<const float *>(sv + base.L.rec), ccs,
                       reinterpret_cast<const uint32_t *>(sv + base.L.dup_off), field, rows, dw,
                       reinterpret_cast<const uint32_t *>(sv + base.L.counters),
                       reinterpret_cast<const uint32_t *>(sv + base.L.seg_off),
                       reinterpret_cast<const uint32_t *>(sv + base.L.seg_tile), (uint32_t)base.L.seg_len);
}

}  // namespace
