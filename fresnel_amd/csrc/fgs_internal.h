// Internal declarations shared by the HIP translation units of libfgs_hip.so.
// gfx950 (MI355X, CDNA4) only: wave64, 160 KiB LDS/CU, 256 CUs in 8 XCDs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fgs.h"

#include "fgs_plan.h"

#define FGS_LAUNCH_CHECK(what)                                              \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) {                                            \
            fgs_set_error("%s: %s", what, hipGetErrorString(e__));          \
            return FGS_ELAUNCH;                                             \
        }                                                                   \
    } while (0)

enum FgsStage { ST_PROJECT = 0, ST_DEPTH_SORT, ST_DUP_EMIT, ST_TILE_SORT, ST_TILE_RANGES, ST_COMPOSITE_FWD,
                ST_COMPOSITE_BWD, ST_PROJECT_BWD, ST_SPLAT_FWD, ST_FIELD_FWD, ST_FIELD_BWD, ST_SPLAT_BWD };
static_assert(ST_SPLAT_BWD + 1 == FGS_NUM_STAGES, "stage list and FGS_NUM_STAGES disagree");
void fgs_stage_begin(int stage, hipStream_t st);  // no-ops unless fgs_stage_timing_enable(1)
void fgs_stage_end(int stage, hipStream_t st);

// ---- stage launchers (each enqueues on `st`, returns FGS_OK / FGS_ELAUNCH) ----
// plane_* != 0 selects the ASM variant: additionally writes saved.layer = nearest depth plane
// (DR:1136-1148) of each Gaussian
int fgs_launch_project(const FgsPlan &p, const float *cams, const float *pos, const float *scale,
                       const float *quat, const float *color, const float *opacity, char *saved,
                       hipStream_t st, int num_planes = 0, float plane_near = 0.0f, float plane_far = 0.0f,
                       uint32_t *zero_words = nullptr /* cleared on the side: the depth sort's hand-off words */, uint32_t zero_count = 0);
int fgs_launch_project_bwd(const FgsPlan &p, const float *cams, const float *pos, const float *scale,
                           const float *quat, const char *saved, const float *grad_rows, float *g_pos,
                           float *g_scale, float *g_quat, float *g_color, float *g_opacity, float *g_phase,
                           hipStream_t st, float *row_sums = nullptr /* scratch [B*N][12]: blend path row totals */,
                           const uint32_t *zero_from = nullptr /* scratch [B*tiles] of this backward's k_bwd_tail_verdict (FgsPlan.bwd_tail) */);

// the row-sum stage of the blend path's projection backward alone (k_row_sum): fgs_launch_project_bwd's first kernel, and fgs_row_sum
int fgs_launch_row_sum(const FgsPlan &p, const char *saved, const float *grad_rows, float *row_sums,
                       const uint32_t *zero_from /* [B*tiles] words, then one per image (their smallest); null: no table */, hipStream_t st);

int fgs_launch_asm_project_bwd(const FgsPlan &p, const float *cams, const float *pos, const float *scale,
                               const float *quat, const float *color, const float *phase, int phase_channels,
                               const char *saved, const float *grad_rows, float *g_pos, float *g_scale,
                               float *g_quat, float *g_color, float *g_opacity, float *g_phase, hipStream_t st,
                               bool wave_rows = false);

// FourierGaussianRenderer (fgs_fourier.hip).  Record of one Gaussian: FGS_FOURIER_REC_FLOATS floats, all zero but the opacity
// when it is culled.  `sums` [B*N][12]: dL/du, dL/dv, dL/d(a + d), dL/dw[3] (w = colour x opacity), six zeros.
#define FGS_FOURIER_REC_FLOATS 8
enum { FR_U = 0, FR_V, FR_IS /* 1 / s */, FR_WR, FR_WG, FR_WB, FR_VIS /* uint32 1 | 0 */, FR_OP };
int fgs_launch_fourier_project(int32_t B, int32_t N, int32_t W, int32_t H, int32_t num_cameras, const float *cams,
                               const float *pos, const float *scale, const float *quat, const float *color,
                               const float *opacity, float *frec, hipStream_t st);
int fgs_launch_fourier_project_bwd(int32_t B, int32_t N, int32_t num_cameras, const float *cams, const float *pos,
                                   const float *scale, const float *quat, const float *color, const float *frec,
                                   const float *sums, float *g_pos, float *g_scale, float *g_quat, float *g_color,
                                   float *g_opacity, hipStream_t st);

// Stable LSD radix sort of (key,val) uint32 pairs over `num_segs` independent segments.
// Segment s covers elements [s*seg_stride, s*seg_stride + len) with len = seg_len (host) or
// *seg_len_dev (device, single segment).  Sorts bits [0, key_bits).  The sorted result is
// left in (keys_sorted, vals_sorted); in/alt buffers are clobbered.
struct FgsRadixSort {
    uint32_t *keys_in, *vals_in, *keys_alt, *vals_alt;
    uint32_t *vals_final;            // nullable: where the last pass writes vals
    uint32_t seg_len;
    const uint32_t *seg_len_dev;
    uint32_t seg_capacity, seg_stride, num_segs, key_bits;
    uint32_t *hist;
    hipStream_t st;
    const uint32_t *keys_first;      // nullable: the first pass reads its keys from there (read-only) instead of keys_in
    uint32_t index_payload_mod;      // != 0: the first pass generates the payload (element index modulo it) instead of reading vals_in
    const uint32_t *key_stats;       // depth sort: k_project's per-block OR / AND of the visible keys: sort by the bits that vary,
                                     // skip the passes nobody needs
    uint32_t key_recs;               // records per segment
    int pass_mode;                   // FgsDims.sort_mode >> 1.  0 = automatic: host-known segments of <= 8192 keys by ONE launch,
                                     // all passes in LDS; larger ones with `key_range` by the bucket sort (one bucket pass over
                                     // memory, then every bucket in LDS), else by the two-launch 8-bit passes | 1 = fused passes (one
                                     // launch each), 11-bit digits, up to 64 K keys | 2 = fused passes, 8-bit digits | 3 = fused
                                     // passes, 8-bit digits, per-block histograms HANDED OFF between the blocks through `hist` (which
                                     // the caller cleared beforehand: fgs_sort.hip) | 4 = the two-launch passes at any size | 5 = as
                                     // automatic
    const uint32_t *key_range;       // depth sort: k_project's records again (smallest visible key in the fourth word, the largest
                                     // behind the records), `key_recs` per segment: what the bucket sort takes its digit from
    uint32_t *bucket_tab;            // scratch of num_segs * FGS_SORT_BUCKET_WORDS words for the bucket sort
    uint32_t *keys_sorted;           // out: which buffer holds the sorted keys (nullptr: none does -- fgs_sort.hip)
    uint32_t *vals_sorted;           // out: ... the sorted payload
};
int fgs_launch_radix_sort(FgsRadixSort &s);

int fgs_launch_binning(const FgsPlan &p, char *saved, char *scratch, hipStream_t st);

// Batched in-place 2-D C2C FFT of `batch` H x W complex fields (fgs_fft.hip: plans cached per (device, H, W, batch),
// built on first use; `work` = caller's work area of fgs_fft_work_bytes bytes).  dir: HIPFFT_FORWARD (-1) /
// HIPFFT_BACKWARD (+1), both unnormalised.
int fgs_fft_work_bytes(int H, int W, int batch, size_t *bytes);
int fgs_fft_exec(int H, int W, int batch, float2 *data, int dir, void *work, hipStream_t st);
int fgs_fft_rows_exec(int W, int rows, float2 *data, int dir, void *work, hipStream_t st);  // 1-D, along rows of length W
int fgs_fft_rows_work_bytes(int W, int rows, size_t *bytes);
// 2-D transform, rocFFT rows + our own column pass for power-of-two heights 64 ... 1024 (else rocFFT's 2-D plan)
int fgs_fft2_work_bytes(int H, int W, int batch, size_t *bytes);
int fgs_fft2_exec(int H, int W, int batch, float2 *data, int dir, void *work, hipStream_t st);
// inverse transform of images x 3 fields + per-image block maxima of sqrt(|u inv_hw|^2 + 1e-8) (fgs_fft.hip); *fused tells whether amax was written
int fgs_fft2_inverse_with_max(int H, int W, int images, float2 *data, void *work, float *amax, int slots, float inv_hw,
                              bool *fused, hipStream_t st);
int fgs_launch_composite_fwd(const FgsPlan &p, const float *phase, char *saved, float *out_rgb,
                             float *out_depth, hipStream_t st);
int fgs_launch_composite_bwd(const FgsPlan &p, const float *phase, const char *saved, char *scratch,
                             const float *g_rgb, const float *g_depth, float *g_phase, hipStream_t st);
int fgs_launch_count_pairs(const FgsPlan &p, const char *saved, uint64_t *out, hipStream_t st);

// ---- small device helpers ----
__device__ __forceinline__ uint32_t fgs_lane() { return threadIdx.x & 63u; }

// XCD-aware block remap (cdna_hip_programming.md T1).  Workgroups are dealt round-robin over the 8 XCDs, each with
// its own L2, so blocks bid and bid + 1 never share an L2.  remap(bid) gives every XCD a CONTIGUOUS range of
// logical work items: neighbours in the work list (adjacent depth-rank blocks of one image, adjacent tiles) then hit
// the same L2 -- shared records are fetched once and, more importantly, partial-line writes to neighbouring
// addresses (4-byte list entries, 40-byte gradient rows) merge in that L2 instead of reaching HBM as masked
// partial writes from several XCDs.  Bijective on [0, nwg) for any nwg; placement only, never correctness.
__device__ __forceinline__ uint32_t fgs_xcd_remap(uint32_t bid, uint32_t nwg) {
    const uint32_t q = nwg >> 3, r = nwg & 7u, xcd = bid & 7u, i = bid >> 3;
    return (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + i;
}

// Opacity fold of the blend kernels (fgs_composite.hip) and the row contract that follows from it (k_row_sum, fgs_project.hip).
// alpha / 0.99 = clamp01(G op'), op' = opacity / 0.99, is formed as clamp01(exp2(m' + log2 op')): the opacity rides on the
// exponent's per-row term and the per-pixel multiply is gone.  The backward then accumulates dL/dalpha . a' = op' . dL/dalpha . G
// where it had dL/dalpha . G: its moment rows already carry the opacity, and its sum-dG row (dL/dopacity) has to be DIVIDED by
// the opacity -- impossible at opacity 0, whose dL/dopacity is not zero.  So the backward folds a FLOOR: for op' < 2^-64 it takes
// lop = -64 exactly, a' = 2^-64 G, and k_row_sum takes the exact power of two out again and puts the true opacity where it belongs.
// Why 2^-64, and no multiplier in the pass that would restore the true alpha of a floored entry:
//  * alpha <= 0.99 x 2^-64 = 5.4e-20 is below every fp32 effect on the transmittance (T (1 - alpha) rounds to T from alpha <
//    2^-25 on), so the backward may run with 2^-64 G where the forward ran with the smaller true alpha.  With a floor such as
//    2^-16 the true alpha would have to be restored per pixel, and a second per-pixel value (alpha next to the factor of dG)
//    live across the backward's wave-uniform clamp block costs the common class a v_mov per pass -- what the fold saves;
//  * 2^-64 G, dalpha 2^-64 G and their moments stay normal fp32 numbers down to G = 2^-60, further than a bbox reaches;
//  * the price is the rounding of the exponent m' + lop: half an ulp of a number below 2 |lop|, times ln 2, relative in alpha --
//    1.3e-6 for op' >= 2^-16 (the size of the forward's parity with the oracle before the fold, 2e-6), at most 5.3e-6 for
//    opacities down to the floor, whose alpha is below 1.6e-5 to begin with; the forward folds the true lop of any opacity anyway.
// The test is on the fp32 opacity ITSELF against an exact constant, so that translation units with different floating-point
// flags (fast-math reciprocals there, IEEE division here) cannot disagree about a Gaussian.  (Negative and NaN opacities count
// as floored; they never reach a pass and their rows are zero.)
constexpr float FGS_FOLD_FLOOR_LOG2 = -64.0f;
constexpr float FGS_FOLD_FLOOR = 5.42101086242752217e-20f;            // 2^-64
constexpr float FGS_FOLD_MIN_OPACITY = 0.99f * FGS_FOLD_FLOOR;        // exact: a power-of-two multiple of 0.99f
__host__ __device__ __forceinline__ bool fgs_opacity_floored(float opacity) { return !(opacity >= FGS_FOLD_MIN_OPACITY); }

// Emission slot of a duplicate = where its gradient row(s) go: a Gaussian's duplicates occupy the slots dup_off[gid] ... in
// row-major order of the tiles of its bbox's tile rectangle (tiles TW pixels wide, FGS_TILE high; bbx = x0 | x1 << 16, bby likewise,
// the record's integer bbox [x0, x1) x [y0, y1)).  ASSIGNED by the binning (k_dup_emit, k_mask_emit* of fgs_bin.hip: dup_off and the
// emission order); USED by the backwards, which write the row of tile (tx, ty) there (k_composite_bwd with TW = 8 NSX, k_phase_bwd
// through phase_scan -- rows 4 e ... 4 e + 3, one per sub-tile wave -- and k_asm_splat<BWD> with TW = FGS_TILE); CONSUMED by
// k_project_bwd / k_row_sum (fgs_project.hip), which sum a Gaussian's contiguous rows in a fixed order.
template <int TW>
__device__ __forceinline__ uint32_t fgs_emission_slot(uint32_t tx, uint32_t ty, uint32_t gid, uint32_t bbx, uint32_t bby,
                                                      const uint32_t *__restrict__ dup_off) {
    const uint32_t tx0 = (bbx & 0xFFFFu) / TW, tx1 = ((bbx >> 16) - 1) / TW, ty0 = (bby & 0xFFFFu) / FGS_TILE;
    return dup_off[gid] + (ty - ty0) * (tx1 - tx0 + 1) + (tx - tx0);
}

// order-preserving map float -> uint32 (ascending), -0.0 folded into +0.0
__device__ __forceinline__ uint32_t fgs_float_key(float f) {
    f = f + 0.0f;
    uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// A product or sum the compiler must not fuse into a neighbouring operation: the value passes through an empty asm, which makes
// it opaque.  (hipcc's __fmul_rn / __fadd_rn are plain operators -- they do NOT stop FMA contraction -- and a
// `#pragma clang fp contract(off)` does not either in a unit compiled with the default -ffp-contract=fast: the AMDGPU backend
// fuses under the global setting.  Found in round 4: a "separately rounded" expression written with the intrinsics came out
// as v_mul + v_fmac in fgs_fft.hip.)
__device__ __forceinline__ float fgs_rounded(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

// kz^2 = (1/l)^2 - FX^2 - FY^2 exactly as the reference's fp32 expression evaluates it (DR:993): every product and every
// difference rounded on its own, whatever the translation unit's contraction setting.  Near the evanescent boundary the
// difference cancels to a few ulps of 1/l^2 and dkz/dlambda = -1 / (l^3 kz) weights exactly those frequencies most, so the
// forward table, the recurrence factor D, both dL/dlambda kernels and the standalone propagator (fgs_spectral.hip) take kz^2
// from this ONE function: forward and adjoint agree on kz to the bit.
__device__ __forceinline__ float fgs_kz2(float il, float fx, float fy) {
    const float a = fgs_rounded(il * il), b = fgs_rounded(fx * fx), c = fgs_rounded(fy * fy);
    return fgs_rounded(fgs_rounded(a - b) - c);
}

// |U|^2 of one complex sample of the ASM renderer's total field and sqrt(|U|^2 + 1e-8) (DR:1316-1319), every operation rounded on
// its own.  The per-image maximum of the latter is found in one translation unit (the inverse column FFT's epilogue, fgs_fft.hip)
// and COMPARED FOR EQUALITY with recomputed values in another (k_asm_output_bwd*, torch.max's gradient goes to the pixels that
// equal the maximum): producer and consumers take the value from here, so they agree to the bit whatever their units' flags.
__device__ __forceinline__ float fgs_asm_intensity(float2 u, float inv_hw) {
    const float ur = fgs_rounded(u.x * inv_hw), ui = fgs_rounded(u.y * inv_hw);
    return fgs_rounded(fgs_rounded(ur * ur) + fgs_rounded(ui * ui));
}
__device__ __forceinline__ float fgs_asm_amplitude(float intensity) { return sqrtf(fgs_rounded(intensity + 1e-8f)); }
