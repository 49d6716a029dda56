/*
 * fgs.h -- C ABI of the MI355X-native Gaussian-splatting rasterizer (libfgs_hip.so).
 *
 * The reference (CalebisGross/fresnel) has no FFI for this path: its boundary is the
 * Python call surface of scripts/models/differentiable_renderer.py ("DR"):
 *     TileBasedRenderer.__init__   DR:434-450
 *     TileBasedRenderer.forward    DR:489-499 -> (3,H,W) [, (H,W)]   DR:684-686
 *     Camera                       DR:24-52
 *     ASMWaveFieldRenderer.forward DR:1150-1161
 * This header is what a binding for that surface calls (see INTEGRATION.md for the
 * ctypes stub).  Conventions:
 *   - plain pointers and sizes only; every data pointer is DEVICE memory (HBM) unless
 *     marked host; all tensors contiguous fp32 in the reference's layouts, with a leading
 *     batch dimension B (one reference call == B = 1);
 *   - functions enqueue work on `stream` and return; they never allocate, never
 *     synchronise and are re-entrant per (stream, workspace);
 *   - return 0 on success, negative FGS_E* on error; fgs_last_error() gives the text.
 *
 * Buffer contract (every compute entry; checked by tests/test_workspace_hygiene.py):
 *   - The caller owns and sizes `saved`, `scratch`, `stats` (fgs_*_workspace_bytes) and every output / gradient tensor.
 *     Their content on entry is UNDEFINED: a call never depends on it (no buffer has to be cleared, a `scratch` that
 *     served another call of any shape may be handed over as it is) and never writes outside the reported sizes.
 *   - Every element of every output and gradient tensor is written by the call that returns it (culled Gaussians,
 *     unselected rows and terms that were not requested get zeros).  Of `saved` only the part a call uses is written:
 *     unused capacity (list entries beyond the duplicate count, segment slots beyond the unit count) stays undefined.
 *   - Alignment: give `saved`, `scratch` and `stats` at least 256 bytes (the sections inside them are laid out in 256-byte
 *     steps and read with 16-byte loads) and input, output and gradient tensors at least 16 bytes.  The tests hand out
 *     512-byte aligned buffers, as torch's allocator does; no smaller alignment is exercised.
 *   - Inputs are never modified.  `saved` goes unchanged through fgs_backward and fgs_ssim_backward (so a second
 *     fgs_ssim_backward on it is valid), through fgs_fourier_backward (likewise) and `stats` through
 *     fgs_pixel_loss_backward; fgs_asm_backward and
 *     fgs_spectral_loss_backward CONSUME `saved` (fields / spectra are overwritten by their gradients), and
 *     fgs_wave_backward takes it non-const as well: one backward per forward there.  (By their signatures fgs_count_pairs
 *     takes `saved` and fgs_helmholtz_loss_backward `residual` as const; no test looks at those two.)
 *   - Duplicate-capacity overflow (fgs_forward with FgsDims.dup_capacity below what the scene needs: saved.counters[3] >
 *     FgsSavedLayout.dup_capacity) is a DEFINED outcome of a successful call, not an error return -- the entry points never
 *     synchronise, so only the device knows.  No byte outside the reported sizes is written and no index taken from an unwritten
 *     list entry is ever dereferenced.  counters[1] = 1 and counters[3] = the demand; every (image, tile) list is empty (`ranges`
 *     all [s, s); seg_off[B * T] = counters[2] = 0 on the blend path); every element of out_rgb and out_depth, for every image of
 *     the call, is the quiet NaN 0x7FC00000.  fgs_backward on such a `saved` writes zero to every element of every gradient tensor
 *     and walks no list; `saved` stays const through it.  The next call on the same stream and scratch is unaffected.
 */
#ifndef FGS_H
#define FGS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FGS_OK 0
#define FGS_EINVAL (-1)    /* bad dims / null pointer */
#define FGS_ELAUNCH (-2)   /* HIP launch error */
#define FGS_EUNSUPPORTED (-3)

#define FGS_TILE 16        /* tile height in pixels, and the width unless FgsSavedLayout.tile_w says 32 */
#define FGS_SEG 128        /* largest depth segment: list entries per backward work unit; a call uses
                              FgsSavedLayout.seg_len (64 for small problems, else FGS_SEG)            */
#define FGS_FWD_EXIT_OFF 0x100 /* FgsDims.fwd_variant flags (values >= 0 only): the exiting depth-split forward off / forced on */
#define FGS_FWD_EXIT_ON 0x200
#define FGS_BWD_ZERO_OFF 0x400 /* FgsDims.fwd_variant flags (values >= 0 only): the blend backward's zero rows for dead units off / forced on */
#define FGS_BWD_ZERO_ON 0x800
#define FGS_BWD_TAIL_OFF 0x2000 /* FgsDims.fwd_variant flags (values >= 0 only): the blend backward's one verdict per closed tile off / forced on */
#define FGS_BWD_TAIL_ON 0x4000
#define FGS_BWD_SUB_OFF 0x8000 /* FgsDims.fwd_variant flags (values >= 0 only): the blend backward's zero sub-tiles of general units off / forced on */
#define FGS_BWD_SUB_ON 0x10000
#define FGS_FWD_PREWALK_OFF 0x40000 /* FgsDims.fwd_variant flags (values >= 0 only): the exiting forward's pre-walk of short lists' later parts off / forced on */
#define FGS_FWD_PREWALK_ON 0x80000
#define FGS_TUNE_AUTO 0    /* FgsDims.seg_len / fwd_variant / bin_mode: let the library choose        */
#ifndef FGS_PHASE_CKPT
#define FGS_PHASE_CKPT 8   /* phase path: entries of a sub-tile's (compacted) list between (A, Phi) checkpoints */
#endif
#define FGS_CAMERA_FLOATS 24

/* Problem shape.  Mirrors TileBasedRenderer.__init__ (DR:434-450). */
typedef struct FgsDims {
    int32_t batch;          /* B images rendered by one call                       */
    int32_t num_gaussians;  /* N Gaussians per image                               */
    int32_t width, height;  /* image_width, image_height                 DR:445-446 */
    float max_radius;       /* radius cap in pixels (default 64)         DR:439,485 */
    float background[3];    /*                                            DR:447    */
    int32_t use_phase;      /* use_phase_blending && phases given        DR:629     */
    float phase_amplitude;  /*                                            DR:442    */
    int32_t num_cameras;    /* 1 (shared, TGD:1209-1223) or B                       */
    int32_t saturation_skip; /* 0 (default): every list entry is composited, like the reference (no early-out).
                                1: at every FGS_SEG-th list entry, 8x8 sub-tiles whose transmittance has fallen
                                below 2^-25 for all their pixels (accumulated alpha == 1.0f in fp32) stop being
                                composited, forward and backward; what is dropped is < 3e-8 * |colour| per pixel.
                                Blend path only (ignored with use_phase).                                      */
    /* Tuning overrides.  0 (FGS_TUNE_AUTO) everywhere = the measured-fastest choice for the launch size; the
     * settings only change how the work is split, never what is computed (results agree to fp32 rounding, the
     * integer stages bit for bit -- tests/test_hip_parity.py).  The library reads NO environment variables: a
     * forward and its backward agree because both derive the plan from the same FgsDims, and the forward also
     * records (seg_len, fwd_variant) in saved.counters[4..5], which the backward kernels read. */
    int32_t seg_len;        /* list entries per depth segment: 0 | a multiple of 64 up to 512 (saturation_skip: 128) */
    int32_t fwd_variant;    /* forward work split: 0 | 1, 2, 4, 8, 16 = depth-split forward with that many list parts
                               per tile (16 x 16 tiles; at most 8 on 32 x 16 tiles) | -1, -2, -4 = row-split forward with that many waves per tile.
                               Phase path: one work split (0 or 4).
                               A value >= 0 may carry ONE of two flags, FGS_FWD_EXIT_OFF | FGS_FWD_EXIT_ON (below): the exiting
                               form of the depth-split forward -- a tile half's list walk stops once the state of every
                               in-frame pixel is a fixed point of the blend update for every entry that can still come, the
                               same bits (k_blend_fwd_head, fgs_composite.hip).  No flag = automatic: on for launches of
                               >= 8192 16 x 16 tile halves.  OFF: every entry is walked, by k_blend_fwd_parts alone (tests and
                               A/B runs); ON: forced.  Like every tuning override the flags change how the work is split, never
                               what is computed.  (FgsDims itself cannot grow: dup_capacity stays its last field.)
                               Beside them a value >= 0 may carry ONE of FGS_BWD_ZERO_OFF | FGS_BWD_ZERO_ON.  The blend backward (k_composite_bwd) writes
                               the gradient rows of a work unit whose pixels all restart at zero transmittance AND whose
                               remaining-sum S is an exact zero on every lane as zeros without walking the unit, and skips the
                               sub-tiles of the other such units whose S is all zero: the very bits the full walk computes
                               (those rows are sums of products with S).  No flag = automatic: on for launches of
                               >= 8192 16 x 16 tile halves.  OFF: every such unit is walked in full; ON: forced at any size
                               (tests and A/B runs).
                               Beside them a value >= 0 may carry ONE of FGS_BWD_TAIL_OFF | FGS_BWD_TAIL_ON.  Where the exiting forward,
                               the zero rows above, the direct binning and the blend backward's unit table all exist, one wave
                               per tile (k_bwd_tail_verdict) decides for ALL the units behind the closing slots of every half of
                               its tile whether they are such zero units; if so they return without writing rows and k_row_sum
                               leaves those rows out of its sums (adding +-0 to a sum that is never -0 changes no bit).  No flag
                               = automatic: on wherever the four exist.  OFF: every unit decides for itself and writes its rows;
                               ON: as automatic (it cannot create what the plan lacks).
                               Beside them a value >= 0 may carry ONE of FGS_BWD_SUB_OFF | FGS_BWD_SUB_ON.  A work unit of the blend
                               backward that is NOT such a dead unit still leaves out the 8 x 8 sub-tiles in which every in-frame
                               pixel restarts at zero transmittance and the remaining-sum S is an exact zero on every lane: their
                               passes add exact zeros to sums that start at +0.  No flag = automatic: on wherever the zero rows
                               above are on.  OFF: every touched sub-tile is composited; ON: forced at any size.
                               Beside them a value >= 0 may carry ONE of FGS_FWD_PREWALK_OFF | FGS_FWD_PREWALK_ON.  Where the exiting
                               forward runs with more than one list part, the later parts of a list of at most that many
                               segments are walked by extra blocks of the head launch (they start from T = 1 and need nothing
                               of part 0), and the rest launch only composes them: the same hand-over slots, the same bits.
                               No flag = automatic = OFF: the walk measured slower inside the head launch than in the rest
                               launch at the benchmark's default size.  ON: on where the exiting forward runs with more than one
                               part (tests and A/B runs); ignored elsewhere.
                               No flag is available with the row-split forward (values < 0).       */
    int32_t bin_mode;       /* tile binning: 0 | 1 = direct (column / row rank masks) | 2 = emit + stable radix sort */
    int32_t tile_w;         /* tile width in pixels: 0 | 16 | 32 (tiles are always 16 rows high).  0 = automatic:
                               32 on the blend path with the depth-split forward for frames >= 512 pixels wide
                               in calls of >= 3072 16 x 16 tiles, 16 elsewhere (FgsSavedLayout.tile_w tells)    */
    int32_t sort_mode;      /* depth sort.  Bit 0: 0 = radix passes over the 32 key bits | 1 = "zone keys" (BASELINE config 4,
                               --use_fresnel_zones: depths snapped to a few values): the keys are compressed to the bits that
                               vary over an image's visible Gaussians and only the passes those need do any work -- the same
                               order for ANY depths, faster when they vary in few bits.  NOT chosen automatically: what the
                               depths look like is known on the device only (fgs_sort.hip).
                               Bits 1-3 (work split, never the result): 0 = automatic -- images of <= 8192 Gaussians are sorted by
                               ONE launch, all passes in the LDS of one compute unit per image (round 5); larger ones by the
                               bucket sort (ONE pass over memory on a digit that spreads the image's visible keys between their
                               minimum and maximum over 255 buckets, then every bucket sorted in LDS: 4 launches), or with
                               bit 0 set by the two-launch 8-bit passes of rounds 1-4 on the compressed keys | 2 = one launch per pass, 11-bit digits, every block
                               recounting its image (<= 65 536 Gaussians) | 4 = the same with 8-bit digits | 6 = 8-bit digits,
                               the blocks' digit counts handed off between them instead of recounted (bounded wait) | 8 = the
                               two-launch passes for any size | 10 = as automatic.  Valid values: 0 ... 11.                 */
    uint32_t dup_capacity;  /* capacity hint: room for this many (tile, Gaussian) duplicates in the lists and in everything sized by
                               them (dup_ids, segment tables and checkpoints, phase checkpoints, sort buffers, gradient rows).
                               0 = the worst case B * N * (tiles a Gaussian of max_radius can touch); a value at or above the
                               worst case is treated as 0.  Never changes a tuning choice: a call whose duplicates fit computes
                               bit for bit what the unhinted call computes.  One that does not fit OVERFLOWS -- a defined outcome
                               of a successful call, see the buffer contract above; saved.counters[3] then tells how much room
                               the scene needs.  (Last field: the layout of every field before it is that of fgs-hip 0.2.) */
} FgsDims;

/* Camera record on the DEVICE: FGS_CAMERA_FLOATS floats per camera (Camera, DR:27-52):
 *   [0..15] view matrix row-major (world->camera), [16] fx, [17] fy, [18] cx, [19] cy,
 *   [20] near, [21] far, [22..23] unused. */

/* Byte offsets of the sections of the `saved` buffer (forward -> backward state and
 * the integer stages the parity tests inspect).  All sections 256-byte aligned. */
typedef struct FgsSavedLayout {
    size_t total_bytes;
    size_t rec;        /* float  [B][N][12]: u,v, conic(a, b+c, d), opacity, r,g,b, depth,
                                              bits(x0|x1<<16), bits(y0|y1<<16)            */
    size_t depth_key;  /* uint32 [B][N]: order-preserving depth bits, 0xFFFFFFFF = culled */
    size_t tile_count; /* uint32 [B][N]: tiles touched (0 = culled or empty bbox)         */
    size_t order;      /* uint32 [B][N]: Gaussian ids in canonical depth order (DR:527)   */
    size_t dup_off;    /* uint32 [B][N]: first duplicate slot of each Gaussian (emission
                                         order = image, depth rank, tile row, tile column)   */
    size_t counters;   /* uint32 [16]: [0] total duplicates D (clamped to dup_capacity), [1] overflow flag,
                                       [2] depth-segment units U, [3] duplicates the call NEEDS (unclamped, saturating at
                                       0xFFFFFFFF; == [0] when the call fits), [4] seg_len and [5] fwd_variant the forward
                                       ran with; [2], [4], [5] are written on the non-phase path only (with use_phase
                                       there are no depth segments and the three words stay undefined), [6..15] are
                                       never written */
    size_t ranges;     /* uint32 [B*T][2]: [start,end) into dup_ids per (image,tile)      */
    size_t tile_order; /* uint32 [B*T]: (image,tile) indices, longest lists first: the launch
                                         order of the composite kernels (scheduling only)    */
    size_t dup_ids;    /* uint32 [Dcap]: b*N+n per duplicate, sorted by (image,tile), depth
                                         order inside a tile                              */
    size_t pix_state;  /* float  [B][6][H][W]: C_r,C_g,C_b (pre-bg, pre-clamp), A, D, Phi */
    size_t phase_ckpt; /* float  [slots][8][64] (use_phase only): per-pixel (A, Phi) of a tile's four 8 x 8 sub-tiles (planes w and
                          4 + w) in front of every 8th entry THAT TOUCHES sub-tile w within a 64-entry block of the
                          tile's list; slot = start/8 + block offset/8 + group + tile                     */
    size_t dup_capacity; /* Dcap (elements, not bytes): the worst case, or FgsDims.dup_capacity below it */
    int32_t tiles_x, tiles_y;
    /* Depth segments (non-phase path): a tile's list is cut into segments of FGS_SEG entries; each
     * segment is one work unit of the backward, so a launch is balanced however uneven the lists are. */
    size_t seg_off;    /* uint32 [B*T+1]: first unit of each (image,tile); [B*T] = number of units U
                                          (also counters[2])                                        */
    size_t seg_tile;   /* uint32 [Ucap]: (image,tile) of each unit; segment index = unit - seg_off    */
    size_t seg_ckpt;   /* float  [Ucap][5][4][64]: per-pixel C_r,C_g,C_b,A,D of the tile at the START
                                          of each unit with segment index >= 1 (written by the forward; with the
                                          exiting forward, see fwd_close for the slots behind a closing)   */
    size_t seg_capacity; /* Ucap = Dcap / seg_len + B*T                                             */
    int32_t seg_len;     /* list entries per depth segment for these dims: 64 when B*N <= 200 000 (more,
                            shorter work units for launches that would not fill the chip), else 128   */
    int32_t tile_w;      /* tile width in pixels (16 | 32; tiles_x counts tiles of this width); a tile has
                            tile_w / 8 x 2 sub-tiles of 8 x 8 pixels, and seg_ckpt slots hold 5 x that many x 64 floats */
    size_t unit_order;   /* uint32 [Ucap], U valid: launch slot -> unit of the blend backward (scheduling only).  The slots
                            are cut into the eight contiguous ranges the XCDs walk; a range keeps the units it has in unit
                            order, but lists its full units (seg_len entries) first, in increasing index, and then its
                            partial units, longest first by quarter-octave of their entry count.  Exists only on the blend
                            path (no phase, one layer); == total_bytes elsewhere.  Not written when U == 0 */
    size_t fwd_open;     /* uint32 [B*T][2]: 1 where the exiting forward's head kernel left that 16 x 16 half of the tile open for the
                            rest kernel, else 0 (index 1 is written on 32 x 16 tiles only).  Exists with the depth-split forward
                            where the exit is on (FgsDims.fwd_variant flags); == total_bytes elsewhere */
    size_t fwd_close;    /* uint32 [B*T][2]: the CLOSING SLOT of that 16 x 16 half of the tile.  A half whose walk the head kernel
                            stopped at `done` entries because its pixels absorb every later entry has k = ceil(done / seg_len);
                            where k is less than the tile's number of segments, the word is k, seg_ckpt slot seg_off + k holds the
                            half's closing state (C, A = 1, D) as an ABSOLUTE state, the half's cells of every later slot of the tile
                            are NOT WRITTEN, and the backward restarts every unit of segment >= k of that half from slot k.
                            0xFFFFFFFF everywhere else: a half left open, a list that ended, a closing inside the last segment,
                            index 1 on 16 x 16 tiles.  Behind the per-block maxima that follow fwd_open; exists where fwd_open
                            exists; == total_bytes elsewhere */
    size_t rank_of;      /* uint32 [B][N]: depth rank of each Gaussian within its image, the inverse of `order` (written beside
                            dup_off by the direct binning).  k_bwd_tail_verdict turns the first list entry behind a tile's closing
                            slots into the rank threshold that k_row_sum compares a Gaussian's rank with.  Behind fwd_close;
                            exists only with the tail verdict of the blend backward (FGS_BWD_TAIL_* above); == total_bytes elsewhere */
} FgsSavedLayout;

/* Sizes of the two caller-provided device buffers.  `saved` must stay untouched between
 * fgs_forward and the matching fgs_backward; `scratch` may be reused immediately. */
int fgs_workspace_bytes(const FgsDims *dims, size_t *saved_bytes, size_t *scratch_bytes);
int fgs_saved_layout(const FgsDims *dims, FgsSavedLayout *layout);

/* Replaces TileBasedRenderer.forward (DR:489-686) for B images at once.
 *   pos (B,N,3)  scale (B,N,3)  quat (B,N,4 wxyz, unnormalised ok)  color (B,N,3)
 *   opacity (B,N)  phase (B,N) or NULL
 *   out_rgb (B,3,H,W) clamped to [0,1]; out_depth (B,H,W). */
int fgs_forward(const FgsDims *dims, const float *cameras, const float *pos, const float *scale,
                const float *quat, const float *color, const float *opacity, const float *phase,
                float *out_rgb, float *out_depth, void *saved, void *scratch, void *stream);

/* Replaces autograd through DR:519-686: gradients of sum(out_rgb*g_rgb)+sum(out_depth*g_depth).
 * g_* outputs are fully overwritten (zeros for culled Gaussians).  g_phase may be NULL
 * when dims->use_phase == 0. */
int fgs_backward(const FgsDims *dims, const float *cameras, const float *pos, const float *scale,
                 const float *quat, const float *color, const float *opacity, const float *phase,
                 const void *saved, void *scratch, const float *g_rgb, const float *g_depth,
                 float *g_pos, float *g_scale, float *g_quat, float *g_color, float *g_opacity,
                 float *g_phase, void *stream);

/* Number of composited Gaussian-pixels of the last forward on this `saved` buffer
 * (SURVEY §8d unit of work): enqueues a reduction that writes one uint64 to
 * `out_pairs` (device). */
int fgs_count_pairs(const FgsDims *dims, const void *saved, uint64_t *out_pairs, void *stream);

/* The row-sum stage of fgs_backward's projection backward ALONE (blend path): per Gaussian the sum of its gradient rows, in the
 * stage's fixed order, with the stage's factors -> row_sums [B*N][12] floats (ten used), by input index.  Reads of `saved` only
 * rec, order, dup_off and tile_count (FgsSavedLayout); grad_rows [dup_capacity][10] floats.  zero_from: NULL, or B * tiles words
 * (per tile the depth rank from which on a Gaussian's row of that tile is left out, 0xFFFFFFFF: none) followed by B words, each
 * image's smallest -- the table fgs_backward builds for itself where the plan has the tail verdict.  For tests and tools: the order
 * of the additions is the contract (tests/test_row_sum_prefetch_order.py). */
int fgs_row_sum(const FgsDims *dims, const void *saved, const float *grad_rows, const uint32_t *zero_from, float *row_sums,
                void *stream);

/* ------------------------------------------------------------------------------------------
 * Angular-spectrum wave-field renderer: replaces ASMWaveFieldRenderer.forward (DR:1150-1344)
 * and AngularSpectrumPropagator (DR:929-1065).  Gaussians are splatted as complex amplitudes
 * onto num_planes depth planes (DR:1233-1283), every plane/channel is propagated to the focal
 * plane with the angular-spectrum transfer function H = exp(i 2 pi z sqrt(max(1/l^2-fx^2-fy^2,0)))
 * (DR:989-999) using batched hipFFT/rocFFT transforms, summed (one inverse FFT per channel, by
 * linearity), converted to intensity, normalised by the per-image maximum and composed with
 * the background (DR:1315-1332).
 *   phase       (B,N) or (B,N,3) radians (phase_channels = 1 | 3)        DR:1181, 1274-1275
 *   wavelengths (3,) DEVICE floats, shared by the batch                   DR:1160
 *   out_rgb     (B,3,H,W)
 * fgs_asm_backward writes gradients of sum(out_rgb*g_rgb) w.r.t. all Gaussian inputs, the
 * phases and the three wavelengths (dkz/dlambda is taken as 0 where 1/l^2-fx^2-fy^2 <= 0; the
 * reference's autograd returns NaN/inf when a frequency lands exactly on that boundary).
 * fgs_asm_backward CONSUMES `saved` (the plane fields / spectra in it are overwritten by their
 * gradients): one backward per forward.
 * The first call for a shape builds the hipFFT plans (host work); later calls only enqueue. */
typedef struct FgsAsmDims {
    int32_t batch, num_gaussians, width, height;
    float max_radius;        /* DR:1087 */
    float background[3];     /* DR:1086 */
    int32_t num_planes;      /* num_depth_planes, DR:1088 */
    float depth_near, depth_far; /* depth_range, DR:1089 */
    float focal_depth;       /* DR:1090 */
    double pixel_pitch;      /* DR:1091.  DOUBLE, like the Python float the reference hands to torch.fft.fftfreq(n, d): the frequency
                                grid is k * (float)(1.0 / (n * d)), and a pitch rounded to fp32 first moves that factor by an ulp
                                for some (n, d) -- 96 samples at 1/200 -- which the near-evanescent terms of dL/dlambda feel */
    int32_t phase_channels;  /* 1: phases (B,N); 3: phases (B,N,3) */
    int32_t num_cameras;     /* 1 or B */
    int32_t bin_mode;        /* list building, as FgsDims.bin_mode: 0 = automatic | 1 = direct (rank masks; the depth order is
                                grouped by plane and a (plane, tile) list is a rank range of the masks) | 2 = emit + stable
                                radix sort over (image, plane, tile) keys.  Same lists either way (tests)                 */
} FgsAsmDims;

int fgs_asm_workspace_bytes(const FgsAsmDims *dims, size_t *saved_bytes, size_t *scratch_bytes);
int fgs_asm_forward(const FgsAsmDims *dims, const float *cameras, const float *pos, const float *scale,
                    const float *quat, const float *color, const float *opacity, const float *phase,
                    const float *wavelengths, float *out_rgb, void *saved, void *scratch, void *stream);
int fgs_asm_backward(const FgsAsmDims *dims, const float *cameras, const float *pos, const float *scale,
                     const float *quat, const float *color, const float *opacity, const float *phase,
                     const float *wavelengths, void *saved, void *scratch, const float *g_rgb,
                     float *g_pos, float *g_scale, float *g_quat, float *g_color, float *g_opacity,
                     float *g_phase, float *g_wavelengths, void *stream);

/* ------------------------------------------------------------------------------------------
 * WaveFieldRenderer (DR:689-926; selected by --use_wave_rendering / --use_qsr, TGD:1891-1897):
 * order-independent complex amplitude accumulation U = sum a c exp(i phi) (DR:832-887), intensity
 * -> sqrt -> per-image max normalisation -> background where the total amplitude is low
 * (DR:893-914); depth map = sum(a depth) / (sum a + 1e-8) (DR:889-891, 924).
 *   phase (B,N) or (B,N,3) radians; out_rgb (B,3,H,W); out_depth (B,H,W). */
typedef struct FgsWaveDims {
    int32_t batch, num_gaussians, width, height;
    float max_radius;
    float background[3];
    int32_t phase_channels;  /* 1 | 3 */
    int32_t num_cameras;     /* 1 or B */
} FgsWaveDims;

int fgs_wave_workspace_bytes(const FgsWaveDims *dims, size_t *saved_bytes, size_t *scratch_bytes);
int fgs_wave_forward(const FgsWaveDims *dims, const float *cameras, const float *pos, const float *scale,
                     const float *quat, const float *color, const float *opacity, const float *phase,
                     float *out_rgb, float *out_depth, void *saved, void *scratch, void *stream);
int fgs_wave_backward(const FgsWaveDims *dims, const float *cameras, const float *pos, const float *scale,
                      const float *quat, const float *color, const float *opacity, const float *phase,
                      void *saved, void *scratch, const float *g_rgb, const float *g_depth, float *g_pos,
                      float *g_scale, float *g_quat, float *g_color, float *g_opacity, float *g_phase,
                      void *stream);

/* ------------------------------------------------------------------------------------------
 * FourierGaussianRenderer (DR:1500-1774; --experiment 4 --use_phase_blending, TGD:1877-1890): a dense, order-independent sum of
 * ISOTROPIC Gaussians over the whole frame.  Per image, in fp32:
 *   visible   near < depth < far, -W < u < 2W, -H < v < 2H (strict, DR:1641-1643); others contribute nothing, zero gradients
 *   footprint sigma = sqrt((a + d) / 2 + 1e-8) of the raw 2-D covariance, s = 2 sigma^2 + 1e-8 (DR:1667-1670, DR:1726)
 *   F_c       = sum_i colour_ic opacity_i exp(-((x - u_i)^2 + (y - v_i)^2) / s_i) on integer pixel coordinates (DR:1723-1736),
 *               evaluated as the matrix product Gy^T diag(w_c) Gx of the separable factors on the fp32 matrix cores
 *   m         = max over (c, y, x) of F; F /= m when m > 1e-8 (DR:1741-1743; decided on the device); the gradient flows
 *               through m to the arg-max element (ties: the lowest flat index)
 *   out       = clamp(F + background_c clamp(1 - sum_c F_c, 0, 1), 0, 1) (DR:1746-1751); both clamps pass the gradient on the
 *               closed interval
 * No visible Gaussian: out = clamp(background), every gradient zero.  Phases, wavelengths and the depth map do not enter
 * (DR:1758-1764: the depth map is all zeros; the binding returns it).  Pointer order of fgs_wave_*, without phase and depth.
 * `saved` layout (256-byte aligned sections, in this order; CONST through fgs_fourier_backward, which may be repeated on it):
 *   rec   float  [B][N][8]    u, v, 1 / s, w_r, w_g, w_b (w = colour x opacity), visible (uint32 1 | 0), opacity;
 *                             a culled Gaussian's record is all zeros but the opacity
 *   F     float  [B][3][H][W] the un-normalised accumulation
 *   scal         [B][2]       m (float) and its flat index in (3, H, W) (uint32)
 * Every element of out_rgb and of the five gradient tensors is written.  The backward uses no atomics: its results are
 * bitwise reproducible from run to run. */
typedef struct FgsFourierDims {
    int32_t batch, num_gaussians, width, height;
    float background[3];
    int32_t num_cameras;     /* 1 or B */
} FgsFourierDims;

int fgs_fourier_workspace_bytes(const FgsFourierDims *dims, size_t *saved_bytes, size_t *scratch_bytes);
int fgs_fourier_forward(const FgsFourierDims *dims, const float *cameras, const float *pos, const float *scale,
                        const float *quat, const float *color, const float *opacity, float *out_rgb, void *saved,
                        void *scratch, void *stream);
int fgs_fourier_backward(const FgsFourierDims *dims, const float *cameras, const float *pos, const float *scale,
                         const float *quat, const float *color, const float *opacity, const void *saved, void *scratch,
                         const float *g_rgb, float *g_pos, float *g_scale, float *g_quat, float *g_color,
                         float *g_opacity, void *stream);

/* ------------------------------------------------------------------------------------------
 * Standalone angular-spectrum propagation: replaces AngularSpectrumPropagator.propagate (DR:1000-1065) and its
 * autograd.  field / out / g_* are (C, H, W) interleaved complex64 (the reference's (H, W, C) layout is permuted by
 * the binding); z = DEVICE scalar propagation distance; wavelengths = DEVICE (C,).  `spectrum` (C,H,W complex) receives
 * fft2(field) and is what the backward needs; scratch from fgs_asm_propagate_workspace_bytes.  band_limit: clamp
 * 1/l^2 - fx^2 - fy^2 at 0 (DR:993-994).  dL/dwavelength is taken as 0 where the clamp binds (see fgs_asm_backward). */
int fgs_asm_propagate_workspace_bytes(int32_t height, int32_t width, int32_t channels, size_t *scratch_bytes);
int fgs_asm_propagate_forward(int32_t height, int32_t width, int32_t channels, double pixel_pitch, int32_t band_limit,
                              const float *field, const float *z, const float *wavelengths, float *out,
                              float *spectrum, void *scratch, void *stream);
int fgs_asm_propagate_backward(int32_t height, int32_t width, int32_t channels, double pixel_pitch, int32_t band_limit,
                               const float *spectrum, const float *z, const float *wavelengths, const float *g_out,
                               float *g_field, float *g_z, float *g_wavelengths, void *scratch, void *stream);

/* ------------------------------------------------------------------------------------------
 * Spectral / stencil losses on the rendered batch.
 * mode 0 = FrequencyDomainLoss (TGD:428-522): mean over (B,C,H,W) of w (|fft2(rendered)| - |fft2(target)|)^2, w = 1
 *          below the radial frequency `cutoff`, `high_weight` above.
 * mode 1 = PhaseRetrievalLoss (TGD:342-425): the same with w = 1 on the fields sqrt(max(I, 1e-8)) exp(i phi),
 *          phi = (2 pi / wavelength) |depth - focal_depth|; depth (B,H,W), wavelength = DEVICE scalar.
 * loss / g_loss / g_wavelength are DEVICE scalars.  The backward CONSUMES `saved` (spectra -> their gradients).
 * g_target / g_depth may be NULL. */
typedef struct FgsSpectralDims {
    int32_t images, channels, height, width;
    int32_t mode;
    float cutoff, high_weight;   /* mode 0 */
    float focal_depth;           /* mode 1 */
    int32_t reserved;            /* must be 0 */
} FgsSpectralDims;
int fgs_spectral_workspace_bytes(const FgsSpectralDims *dims, size_t *saved_bytes, size_t *scratch_bytes);
int fgs_spectral_loss_forward(const FgsSpectralDims *dims, const float *rendered, const float *target,
                              const float *depth, const float *wavelength, float *loss, void *saved, void *scratch,
                              void *stream);
int fgs_spectral_loss_backward(const FgsSpectralDims *dims, const float *rendered, const float *target,
                               const float *depth, const float *wavelength, void *saved, void *scratch,
                               const float *g_loss, float *g_rendered, float *g_target, float *g_depth,
                               float *g_wavelength, void *stream);
/* wave_equation_loss (TGD:781-835): mean squared Helmholtz residual lap(U) + (2 pi / wavelength)^2 U of `images`
 * fields (H,W) with the periodic 5-point Laplacian on a grid of spacing pixel_spacing.  residual (images,H,W) is
 * written by the forward and read by the backward; scratch = fgs_reduction_scratch_bytes() bytes. */
int fgs_helmholtz_loss_forward(int32_t images, int32_t height, int32_t width, float wavelength, float pixel_spacing,
                               const float *field, float *loss, float *residual, void *scratch, void *stream);
int fgs_helmholtz_loss_backward(int32_t images, int32_t height, int32_t width, float wavelength, float pixel_spacing,
                                const float *residual, const float *g_loss, float *g_field, void *stream);
size_t fgs_reduction_scratch_bytes(void);

/* SSIM (pytorch_msssim.ssim, the SSIM term of the reference's training loss, TGD:904): Gaussian-window "valid" SSIM of
 * images x channels planes height x width (fp32, contiguous), Wang et al. 2004.  taps[0..num_taps) = the 1-D window
 * (odd count <= 15; applied along H, then W), c1 = (K1 data_range)^2, c2 = (K2 data_range)^2.
 * out: a DEVICE scalar (the mean of the per-plane means), or (images,) with FGS_SSIM_PER_IMAGE (the mean over channels);
 * FGS_SSIM_NONNEGATIVE clips the per-plane means at zero first.  FGS_SSIM_GRAD_X / _Y make the forward save the
 * backward's per-pixel factor maps in `saved` (without either, only the per-plane means: no-grad forward).
 * The backward reads `saved` and does not modify it (a second backward through the same forward is valid); g_out has the
 * shape of out; g_x may be NULL, g_y may be NULL (not both), g_y needs FGS_SSIM_GRAD_Y; scratch is not read (may be NULL). */
#define FGS_SSIM_MAX_TAPS 15
#define FGS_SSIM_GRAD_X 1
#define FGS_SSIM_GRAD_Y 2
#define FGS_SSIM_NONNEGATIVE 4
#define FGS_SSIM_PER_IMAGE 8
typedef struct FgsSsimDims {
    int32_t images, channels, height, width;
    float taps[FGS_SSIM_MAX_TAPS];
    int32_t num_taps;
    float c1, c2;
    int32_t flags;               /* FGS_SSIM_* */
} FgsSsimDims;
int fgs_ssim_workspace_bytes(const FgsSsimDims *dims, size_t *saved_bytes, size_t *scratch_bytes);
int fgs_ssim_forward(const FgsSsimDims *dims, const float *x, const float *y, float *out, void *saved, void *scratch,
                     void *stream);
int fgs_ssim_backward(const FgsSsimDims *dims, const float *x, const float *y, const void *saved, const float *g_out,
                      float *g_x, float *g_y, void *scratch, void *stream);

/* Per-pixel block of the training loss (TGD:873-953): three means over this process's images (fp32, contiguous, DEVICE)
 *   rgb       mean over images x 3 x H x W of w |rendered - target|, w = (1 - vlm_weight) + vlm_weight density with
 *             FGS_PIXEL_DENSITY (density (images,1,H,W), TGD:877-888), else w = 1 (TGD:890)
 *   boundary  mean over images x H x W of mask mean_c |rendered - target| (TGD:945-951); mask =
 *             sigmoid((10 / threshold) (threshold - min_k |target_depth - boundaries[k]|)), or (min_k ... < threshold)
 *             with FGS_PIXEL_HARD_MASK (the reference's FresnelZones.compute_boundary_mask)
 *   depth     mean over images x H x W of |u - v|, u = (rendered_depth - mean) / max(std, 1e-4), v the same of
 *             target_depth (TGD:922-928); mean and unbiased two-pass std are taken over N = images x H x W x world
 *             pixels: every rank's batch
 * out = float[3] {rgb, boundary, depth}; a term that is not requested is written as 0.
 *
 * stats = double[FGS_PIXEL_STAT_SLOTS] (fgs_pixel_loss_workspace_bytes: stats_bytes).  The mean, the std and the gradient's
 * two global sums are three DEPENDENT reductions, so the forward is staged; every stage reads and writes named slots:
 *   stage1  one pass over all inputs    writes RGB, BOUNDARY (local sums), SUM_X, SUM_Y and out[0], out[1] (out[2] = 0)
 *   stage2  reads SUM_X, SUM_Y          writes SSD_X, SSD_Y = sum (x - mean)^2 of rendered_depth / target_depth
 *   stage3  reads SUM_*, SSD_*          writes DEPTH (local sum |u - v|), SGN = sum sgn(u - v), SGN_U = sum sgn(u - v) u, out[2]
 * SUM_*, SSD_*, SGN and SGN_U are CROSS-RANK slots: a data-parallel caller (world > 1) sum-all-reduces SUM_X..SUM_Y after
 * stage1, SSD_X..SSD_Y after stage2 and SGN..SGN_U after stage3 (each pair is contiguous); the backward then needs no
 * collective.  Stages 2 and 3 are only needed (and only valid) with FGS_PIXEL_DEPTH.  fgs_pixel_loss_forward enqueues the
 * stages back to back: the single-process case (world = 1).
 *
 * Backward: ONE pointwise launch, no reduction; reads the inputs and stats, modifies neither.  g_rgb / g_boundary /
 * g_depth: DEVICE scalars, the upstream gradients of the three terms (NULL = 0).  sgn(a - b) = (a > b) - (a < b): 0 on a tie.
 *   g_rendered       = sgn(rendered - target) (g_rgb w + g_boundary mask) / (images x 3 x H x W)
 *   g_rendered_depth = g_depth (q - Q / N - gate P u / (N - 1)) / s,  q = sgn(u - v) / (images x H x W),
 *                      Q = SGN / (images x H x W), P = SGN_U / (images x H x W), s = max(std, 1e-4), gate = (std >= 1e-4)
 * which, with the cross-rank slots summed, is the gradient of the SUM of the ranks' depth terms (what differentiable
 * all-reduces of the statistics give).  g_rendered may be NULL without FGS_PIXEL_RGB and _BOUNDARY, g_rendered_depth
 * without FGS_PIXEL_DEPTH.  A NaN / Inf in rendered or rendered_depth makes the term it enters non-finite. */
#define FGS_PIXEL_MAX_BOUNDARIES 65
#define FGS_PIXEL_RGB 1
#define FGS_PIXEL_DENSITY 2      /* needs FGS_PIXEL_RGB */
#define FGS_PIXEL_BOUNDARY 4
#define FGS_PIXEL_HARD_MASK 8
#define FGS_PIXEL_DEPTH 16
#define FGS_PIXEL_STAT_RGB 0
#define FGS_PIXEL_STAT_BOUNDARY 1
#define FGS_PIXEL_STAT_DEPTH 2
#define FGS_PIXEL_STAT_SUM_X 3   /* x = rendered_depth */
#define FGS_PIXEL_STAT_SUM_Y 4   /* y = target_depth */
#define FGS_PIXEL_STAT_SSD_X 5
#define FGS_PIXEL_STAT_SSD_Y 6
#define FGS_PIXEL_STAT_SGN 7
#define FGS_PIXEL_STAT_SGN_U 8
#define FGS_PIXEL_STAT_SLOTS 16  /* 9 used */
typedef struct FgsPixelLossDims {
    int32_t images, height, width;
    int32_t flags;               /* FGS_PIXEL_*: at least one term */
    int32_t world;               /* ranks whose batches share the depth statistics (>= 1); images x H x W x world >= 2 */
    float vlm_weight;            /* FGS_PIXEL_DENSITY */
    float threshold;             /* FGS_PIXEL_BOUNDARY: > 0 */
    int32_t num_boundaries;      /* FGS_PIXEL_BOUNDARY: 1 ... 65, strictly increasing */
    float boundaries[FGS_PIXEL_MAX_BOUNDARIES];
} FgsPixelLossDims;
int fgs_pixel_loss_workspace_bytes(const FgsPixelLossDims *dims, size_t *stats_bytes, size_t *scratch_bytes);
int fgs_pixel_loss_stage1(const FgsPixelLossDims *dims, const float *rendered, const float *target,
                          const float *rendered_depth, const float *target_depth, const float *density, float *out,
                          void *stats, void *scratch, void *stream);
int fgs_pixel_loss_stage2(const FgsPixelLossDims *dims, const float *rendered_depth, const float *target_depth,
                          void *stats, void *scratch, void *stream);
int fgs_pixel_loss_stage3(const FgsPixelLossDims *dims, const float *rendered_depth, const float *target_depth, float *out,
                          void *stats, void *scratch, void *stream);
int fgs_pixel_loss_forward(const FgsPixelLossDims *dims, const float *rendered, const float *target,
                           const float *rendered_depth, const float *target_depth, const float *density, float *out,
                           void *stats, void *scratch, void *stream);
int fgs_pixel_loss_backward(const FgsPixelLossDims *dims, const float *rendered, const float *target,
                            const float *rendered_depth, const float *target_depth, const float *density,
                            const void *stats, const float *g_rgb, const float *g_boundary, const float *g_depth,
                            float *g_rendered, float *g_rendered_depth, void *stream);

/* Gaussian-parameter head of the reference's patch decoders (DirectPatchDecoder GDM:845-922, FibonacciPatchDecoder
 * GDM:1674-1723, rotation_6d_to_quaternion GDM:186-276): the elementwise map from the decoder MLP's raw output to the
 * renderers' inputs, and its derivative.  All tensors fp32, contiguous, DEVICE.
 *   raw          (B, P, K_full, C)  C = 16: xyz offset 3 (z unused), scale 3, rotation-6D 6, colour 3, opacity 1; C = 19: + phase 3.
 *                                   Only the first K = k_used Gaussians of every point are used; N = P x K
 *   base_xy      (P, 2)             grid / spiral coordinates        base_z  (B, P)  depth_offset - 2 depth
 *   pose         (B, 4) or NULL     cos az, sin az, cos el, sin el: positions turn about Y by az, then about X by el
 *   opacity_mod  (B,)   or NULL     opacity = clamp(opacity x opacity_mod, 0, 1)
 *   edge         (B, P) or NULL     scales x (1 - edge_scale_factor edge), opacity = clamp(opacity + edge_opacity_boost edge, 0, 1),
 *                                   before opacity_mod
 *   outputs      positions (B,N,3)  = (base_xy + xy_gain raw[0:2], base_z), turned by pose
 *                scales    (B,N,3)  = clamp(softplus(clamp(raw, -10, 20) + 1) 0.15, 1e-6, 2)   (softplus linear above 20)
 *                rotations (B,N,4)  unit w,x,y,z: Gram-Schmidt of the two 3-vectors (F.normalize eps 1e-6, b2 + 1e-8 before its
 *                                   normalisation, b3 = (0,0,1) when |b1 x b2| < 1e-6), matrix -> quaternion by the branch
 *                                   trace > 0 | R00 largest | R11 > R22 | else, normalised
 *                colors (B,N,3), opacities (B,N) sigmoids;  phases (B,N,3) = 2 pi sigmoid, C = 19 only (else NULL)
 * Backward: recomputes the forward from raw (nothing is saved); clamps pass the gradient on the closed interval; only the
 * selected quaternion branch is differentiated.  Any upstream gradient may be NULL (= 0).  g_raw (B, P, K_full, C): every
 * element written (zeros for channel 2 and for the K_full - K unused Gaussians).  g_base_z (B, P), g_edge (B, P; needs edge),
 * g_opacity_mod (B,; needs opacity_mod and scratch of fgs_head_workspace_bytes): each may be NULL; sums in a fixed order, no
 * atomics: results repeat bit for bit.  scratch is written, never read before it is written.  K_full <= 64, B <= 65535. */
typedef struct FgsHeadDims {
    int32_t batch, points, k_full, k_used;
    int32_t channels;            /* 16 | 19 */
    float xy_gain;               /* 0.25 grid decoder (GDM:848), 0.15 spiral decoder (GDM:1675) */
    float edge_scale_factor, edge_opacity_boost;   /* used with edge */
} FgsHeadDims;
int fgs_head_workspace_bytes(const FgsHeadDims *dims, size_t *scratch_bytes);
int fgs_head_forward(const FgsHeadDims *dims, const float *raw, const float *base_xy, const float *base_z, const float *pose,
                     const float *opacity_mod, const float *edge, float *positions, float *scales, float *rotations,
                     float *colors, float *opacities, float *phases, void *stream);
int fgs_head_backward(const FgsHeadDims *dims, const float *raw, const float *pose, const float *opacity_mod, const float *edge,
                      const float *g_positions, const float *g_scales, const float *g_rotations, const float *g_colors,
                      const float *g_opacities, const float *g_phases, float *g_raw, float *g_base_z, float *g_edge,
                      float *g_opacity_mod, void *scratch, void *stream);

/* ------------------------------------------------------------------------------------------
 * Neighbour perception and state update of the reference's NCAGaussianDecoder (scripts/models/nca_gaussian_decoder.py,
 * "NCA": _nca_step 232-286).  state (B, N, D) fp32, channels 0..2 the position.
 *
 * Canonical neighbours (this library's definition; torch.topk leaves the order of ties open and cdist changes its arithmetic
 * with the point count): d2(i, j) = (dx dx + dy dy) + dz dz of the coordinate differences, every operation rounded to fp32; a
 * NaN d2 counts as +inf; the neighbours of i are the k points j != i with the smallest (d2, j), in ascending (d2, j) order.
 * Self is excluded by index.  For ANY input, NaN and Inf included, the k indices written for a point are in [0, N), distinct
 * and different from the point's own.
 *
 * fgs_nca_perceive_forward:  perception (B, N, (k+1) D) = the point's own row, then its k neighbours' rows (the input of the
 *     reference's `perception` network, NCA:247-264); neighbors (B, N, k) int32 -- all that the backward needs (`saved`).
 * fgs_nca_perceive_backward: g_state[b, j, :] = g_perception[b, j, 0:D] + sum of g_perception[b, i, (s+1) D : (s+2) D] over all
 *     (i, s) with neighbors[b, i, s] = j, added in ascending (i, s) order after the self term.  No float atomics: two calls
 *     agree to the bit.  Any in-degree 0 ... N - 1.  Nothing flows through the indices (the reference discards topk's values).
 *     The inverted index is built in LDS: the call needs no scratch.  Entries of `neighbors` outside [0, N) are ignored.
 * fgs_nca_update_forward:    new_state = state + step_size (delta mask), mask = (uniform < update_prob) per point; rounded as
 *     torch's expression (three roundings, no FMA).  uniform (B, N) or NULL = eval mode: no mask (NCA:276-284).  step_size: one
 *     DEVICE float.
 * fgs_nca_update_backward:   g_delta = (g_new_state step_size) mask;  *g_step_size = sum of g_new_state (delta mask), exact
 *     products added in double in a fixed order (fixed grid, fixed-shape block tree, block partials in block order in `scratch`
 *     of fgs_nca_workspace_bytes), rounded to fp32 once: repeats bit for bit.  dL/dstate is g_new_state itself: not written.
 * Shapes: 1 <= k <= 16, k + 1 <= N <= 4096, 3 <= D <= 64, B <= 65535, B N (k+1) D < 2^31; otherwise FGS_EINVAL (bad dims, null
 * pointers) / FGS_EUNSUPPORTED before anything touches the device. */
typedef struct FgsNcaDims {
    int32_t batch, points, state_dim, k;
} FgsNcaDims;
int fgs_nca_workspace_bytes(const FgsNcaDims *dims, size_t *scratch_bytes);
int fgs_nca_perceive_forward(const FgsNcaDims *dims, const float *state, float *perception, int32_t *neighbors, void *stream);
int fgs_nca_perceive_backward(const FgsNcaDims *dims, const int32_t *neighbors, const float *g_perception, float *g_state,
                              void *stream);
int fgs_nca_update_forward(const FgsNcaDims *dims, const float *state, const float *delta, const float *step_size,
                           const float *uniform, float update_prob, float *new_state, void *stream);
int fgs_nca_update_backward(const FgsNcaDims *dims, const float *delta, const float *step_size, const float *uniform,
                            float update_prob, const float *g_new_state, float *g_delta, float *g_step_size, void *scratch,
                            void *stream);

/* ------------------------------------------------------------------------------------------
 * The two stages of the reference's SAAGRefinementNet (scripts/models/gaussian_decoder_models.py, GDM:424-570; --experiment 1)
 * that are not GEMMs.  All tensors fp32, DEVICE; everything but `features` contiguous.
 *   SAAG cloud   positions (B,N,3), scales (B,N,3), rotations (B,N,4) w,x,y,z (not necessarily unit), colors (B,N,3),
 *                opacities (B,N)
 *   features     (B, C, grid_h, grid_w) addressed by element strides: feat_stride_batch, feat_stride_channel, feat_stride_row; the
 *                column stride is C when feat_stride_channel = 1 (channel-last memory, the (B, h, w, C) tensor of the training loop
 *                seen through permute(0, 3, 1, 2): sampled in place, no copy) and 1 otherwise (channel-first memory: the same
 *                kernel with these strides -- 4-byte gathers a plane apart instead of coalesced rows, no workspace, bit-equal
 *                results).  Rows, planes and images may be padded, not overlapping.
 * fgs_saag_inputs_forward:  mlp_inputs (B, N, C + 14), row = [C sampled features | position 3 | scale 3 | rotation 4 | colour 3 |
 *     opacity 1].  Sampling (GDM:491-496 + F.grid_sample(bilinear, padding_mode='border', align_corners=False)):
 *     u = clamp((x / max(z, 0.1) + 2) / 4, 0, 1), v likewise from y; ix = clip(u grid_w - 0.5, 0, grid_w - 1), iy likewise with
 *     grid_h; x0 = floor(ix), weights (x0 + 1 - ix, ix - x0) x (y0 + 1 - iy, iy - y0), summed in the order (x0,y0), (x0+1,y0),
 *     (x0,y0+1), (x0+1,y0+1).  A corner outside the grid (index grid_w or grid_h, reached at ix = grid_w - 1) contributes nothing
 *     and is NOT READ.  Forward only: every input is dataset data.
 * fgs_saag_refine_forward:  raw (B,N,16) = [position 3 | scale 3 | rotation-6D 6 | colour 3 | opacity 1], gains = 4 DEVICE floats
 *     (pos, scale, colour, opacity: nothing is read on the host, the call is capturable), rs = residual_scale (GDM:515-540):
 *       pos_delta = raw gain rs, positions = saag + pos_delta;     scale_delta likewise, scales = saag exp(scale_delta)
 *       rotations = normalize(q_delta (x) q_saag), q_delta = the head's rotation_6d_to_quaternion (with its +1e-8), (x) the
 *                   Hamilton product (GDM:555-570), normalize = p / max(|p|, 1e-12)
 *       color_delta likewise, colors = clamp(saag + color_delta, 0, 1);   opacity_delta (B,N,1), opacities (B,N) likewise
 * fgs_saag_refine_backward: recomputes the forward from raw (nothing is saved); the clamps pass the gradient on the closed
 *     interval [0, 1]; only the selected quaternion branch is differentiated.  Each of the nine upstream gradients may be NULL
 *     (= 0).  g_raw (B,N,16): every element written.  g_gains[4] = sums over B N 3 (or B N) products of two floats, exact in
 *     double, added in a fixed order (fixed grid, fixed-shape block tree, block partials in block order from `scratch` of
 *     fgs_saag_workspace_bytes), times rs, rounded to fp32 once.  No atomics: two calls agree to the bit.  scratch is written,
 *     never read before it is written.  No gradient for the SAAG tensors.
 * Shapes: B, N, C, grid_h, grid_w >= 1, B <= 65535, B N (C + 14) < 2^31; otherwise FGS_EINVAL (bad dims or strides, null
 * pointers) / FGS_EUNSUPPORTED before anything touches the device.  The refine entries ignore C's grid and strides. */
typedef struct FgsSaagDims {
    int32_t batch, points, channels, grid_h, grid_w;
    int64_t feat_stride_batch, feat_stride_channel, feat_stride_row;   /* in elements */
    float residual_scale;
} FgsSaagDims;
int fgs_saag_workspace_bytes(const FgsSaagDims *dims, size_t *scratch_bytes);
int fgs_saag_inputs_forward(const FgsSaagDims *dims, const float *features, const float *positions, const float *scales,
                            const float *rotations, const float *colors, const float *opacities, float *mlp_inputs, void *stream);
int fgs_saag_refine_forward(const FgsSaagDims *dims, const float *raw, const float *positions, const float *scales,
                            const float *rotations, const float *colors, const float *opacities, const float *gains,
                            float *o_positions, float *o_scales, float *o_rotations, float *o_colors, float *o_opacities,
                            float *pos_delta, float *scale_delta, float *color_delta, float *opacity_delta, void *stream);
int fgs_saag_refine_backward(const FgsSaagDims *dims, const float *raw, const float *scales, const float *rotations,
                             const float *colors, const float *opacities, const float *gains, const float *g_positions,
                             const float *g_scales, const float *g_rotations, const float *g_colors, const float *g_opacities,
                             const float *g_pos_delta, const float *g_scale_delta, const float *g_color_delta,
                             const float *g_opacity_delta, float *g_raw, float *g_gains, void *scratch, void *stream);

/* ------------------------------------------------------------------------------------------
 * Parameter head of the reference's PhysicsDirectPatchDecoder (scripts/models/gaussian_decoder_models.py, GDM:955-1147) with the
 * physics-derived phase of PhysicsFresnelZones.depth_to_phase (scripts/utils/fresnel_zones.py:555-575).  All tensors fp32,
 * contiguous, DEVICE.
 *   raw             (B, P, K_full, 16)  xyz offset 3 (z unused), scale 3, rotation-6D 6, colour 3, opacity 1; the first K = k_used
 *                                       Gaussians of every patch are used; N = P x K, Gaussian n = p K + k
 *   base_xy         (P, 2) grid coordinates       base_z  (B, P)  depth_offset - 2 depth
 *   wavelength_raw  one DEVICE float: never read on the host, so the calls can be captured in a graph
 *   outputs         positions (B,N,3) = (base_xy + xy_gain raw[0:2], base_z);  scales (B,N,3) = softplus(raw + 1) 0.15 (softplus
 *                   linear above 20; NO clamps);  rotations (B,N,4) as the head's above;  colors (B,N,3), opacities (B,N) sigmoids
 *                   phases (B,N) radians in [0, 2 pi]: with z the Gaussian's base_z and z_min, z_max over all B x P values,
 *                       D = (z_max - z_min) + 1e-8        u = (z - z_min) / D        lambda = min(max(|wavelength_raw|, wavelength_min), wavelength_max)
 *                       c = fp32(2 pi) / lambda           pd = |u - focal_depth|     phase = fmod(c pd, fp32(2 pi))
 *                   every operation rounded to fp32 on its own (IEEE divide, no FMA): torch's fp32 result, bit for bit.
 *                   A NaN in base_z makes z_min and z_max NaN and with them EVERY phase (as torch's min / max); the other outputs
 *                   are NaN only where their own inputs are.
 *   range           16 bytes, written by the forward and read by the backward (all that is saved): float z_min, z_max; int32 n_min,
 *                   n_max = how many of the B x P values equal z_min / z_max (0 when NaN)
 * fgs_physics_forward:  two launches (range, head) while B x P <= 16 384, three beyond (the range in up to 32 blocks, then a fold).
 * fgs_physics_backward: recomputes the forward from raw, base_z and range.  Any of the six upstream gradients may be NULL (= 0).
 *     g_raw (B, P, K_full, 16): every element written (zeros for channel 2 and for the K_full - K unused Gaussians).
 *     g_base_z (B, P) or NULL = the patch's K position-z gradients + g_u / D + [z = z_min] g_z_min / n_min + [z = z_max] g_z_max /
 *       n_max, with G = the patch's K phase gradients (both sums added in k order), g_u = (G c) sgn(u - focal_depth) (sgn(0) = 0),
 *       g_z_min = (S2 - S1) / D, g_z_max = -S2 / D, S1 = sum g_u, S2 = sum g_u u: torch's min() / max() share their gradient
 *       equally among tied elements.
 *     g_wavelength_raw, one float, or NULL = -S3 c / lambda x sign(wavelength_raw) where wavelength_min <= |wavelength_raw| <=
 *       wavelength_max (closed interval; sign(0) = 0), else 0;  S3 = sum G pd.
 *     S1, S2, S3 are sums over the B x P patches of products of two floats, exact in double, added in a fixed order (fixed-shape
 *     block tree, block partials from `scratch` added in a fixed order) and rounded to fp32 once.  No atomics: two calls agree
 *     to the bit.  scratch (fgs_physics_workspace_bytes; both calls) is written, never read before it is written.
 * Shapes: B, P >= 1, 1 <= K <= K_full <= 64, B <= 65535, B P K_full 16 < 2^31, 0 < wavelength_min <= wavelength_max; otherwise
 * FGS_EINVAL (bad dims, null pointers) / FGS_EUNSUPPORTED before anything touches the device. */
typedef struct FgsPhysicsDims {
    int32_t batch, points, k_full, k_used;
    float xy_gain;                 /* 0.25 (GDM:1098) */
    float focal_depth;             /* of the normalised depth u, 0.5 by default */
    float wavelength_min, wavelength_max;   /* 0.01, 0.5 (fresnel_zones.py:429-430) */
} FgsPhysicsDims;
int fgs_physics_workspace_bytes(const FgsPhysicsDims *dims, size_t *scratch_bytes);
int fgs_physics_forward(const FgsPhysicsDims *dims, const float *raw, const float *base_xy, const float *base_z,
                        const float *wavelength_raw, float *positions, float *scales, float *rotations, float *colors,
                        float *opacities, float *phases, void *range, void *scratch, void *stream);
int fgs_physics_backward(const FgsPhysicsDims *dims, const float *raw, const float *base_z, const float *wavelength_raw,
                         const void *range, const float *g_positions, const float *g_scales, const float *g_rotations,
                         const float *g_colors, const float *g_opacities, const float *g_phases, float *g_raw, float *g_base_z,
                         float *g_wavelength_raw, void *scratch, void *stream);

/* ------------------------------------------------------------------------------------------
 * SAAG surface-aligned Gaussian clouds from depth: the producer of the `{name}_saag.bin` caches that --experiment 1 refines.
 * Mirrors the reference's C++ application: PointCloud::from_depth (src/core/pointcloud.cpp:8-76), center / normalize (:433-479),
 * to_surface_gaussians (:100-431), DepthMap::compute_surface_info (src/core/image.cpp:157-225), driven as the viewer drives them
 * (src/viewer/viewer.cpp:354-428).  Forward only.  All tensors fp32, contiguous, DEVICE.
 *   depth      (B, H, W)     already curve-adjusted (the caller applies pow(depth, depth_exponent))
 *   color      (B, 3, H, W)  or NULL = grey 0.7
 *   points     one per (x, y) with x = 0, s, 2 s ... < W and y likewise (s = subsample), row-major: P = ceil(W / s) ceil(H / s) per image
 *   outputs    positions (N,3), scales (N,3), rotations (N,4) w,x,y,z, colors (N,3), opacities (N,): the images' clouds one after the
 *              other; image b owns the rows offsets[b] ... offsets[b + 1] - 1, N = offsets[B].  offsets: B + 1 DEVICE int32.
 * Per image: [min_d, max_d] over ALL pixels, range = max_d - min_d (1 when < 1e-6f).  Per point: u = (d - min_d) / range (also the
 * confidence), z = (1 - u) depth_scale, dropped when z < 0.01f depth_scale; X = (x - cx) / fx z, Y = (cy - y) / fy z, Z = -z.  With
 * normalize_extent > 0 the kept points are centred on their bounding box's centre, centred AGAIN (normalize() centres itself), then
 * scaled by normalize_extent / (largest extent) unless that extent is < 1e-6f.  (p - c is monotone in p, so the second and third
 * bounding boxes are the first one shifted: one reduction, the same bits as three.)  Sobel gradient (gx, gy) of the depth at the point's
 * pixel with ZERO outside the frame (border pixels carry large gradients, as in the reference); max_gradient = largest
 * sqrt(gx gx + gy gy) over the KEPT points, those skipped below included (1 when < 1e-6f).  Rows of a point, in this order:
 *   nothing when confidence < min_confidence; else 1 base;
 *   + 1 back when shell_enabled and g > shell_edge_threshold (g = gradient magnitude / max_gradient), + wall_segments walls when also
 *     connect_walls and the wall tangent is longer than 0.1;
 *   + wrap_layers wraps when wrap_enabled, g > wrap_edge_threshold and the gradient direction is longer than 0.1;
 *   + extra_count fills when density_enabled and g > density_gradient_threshold (jitter: the reference's integer hash of pixel, index, seed).
 * Every quantity behind these decisions is built from + - * / sqrt min max only, each rounded to fp32 on its own (no FMA, IEEE
 * divide and sqrt, the reference's operation order): counts and row order are exact.  Rotations and wrap opacities go through
 * acos / sin / cos / pow and agree with another implementation to a few ulps.
 * Defaults of fx, fy, cx, cy: fx <= 0 means 0.8f W (the viewer's), fy <= 0 means fx; cx <= 0, cy <= 0 mean W / 2, H / 2.
 *
 * Two phases, so that the caller sizes the outputs and the library never allocates or synchronises:
 * fgs_surface_count:  five launches (depth range, point bounds + max gradient, per-image fold, per-point decisions + block sums,
 *     scan of the block sums).  Writes offsets (all B + 1) and, in scratch, what the emit needs.  scratch + FGS_SURFACE_STATE_OFFSET
 *     holds one byte per point, image-major (B P bytes): FGS_SURFACE_KEPT | _BASE | _BACK | _WALLS | _WRAPS | _FILLS; the rest of
 *     scratch is private.  scratch is written, never read before it is written.
 * fgs_surface_emit:   one launch.  Reads depth, color, offsets and the scratch of the count call with the SAME dims and params; writes
 *     every row below offsets[B] and nothing else.  `capacity` = the rows the caller allocated: when offsets[B] > capacity the kernel
 *     writes NO row and sets the first int32 of scratch to 1 (else 0).  The total lives on the device, so the return value cannot
 *     report that case without a synchronisation: the caller, who read offsets[B] to size the outputs, compares it first (as
 *     fresnel_amd.surface does, which raises).  No atomics anywhere: two calls agree to the bit, and a batch equals its single images.
 * NaN / Inf depth pixels: min_d / max_d ignore NaN (fminf / fmaxf); a NaN confidence fails both the drop and the skip compare, so
 *     the point is kept and emits its base row; NaN gradients fail every threshold compare.  Float outputs may then be non-finite,
 *     in that image only.  offsets stays monotone, a point never emits more than 2 + wall_segments + wrap_layers + extra_count rows,
 *     and nothing is written outside the rows below offsets[B].
 * Shapes: B, H, W >= 1, B <= 65535, B H W < 2^31, subsample >= 1, wall_segments, wrap_layers, extra_count >= 0,
 * B P (2 + wall_segments + wrap_layers + extra_count) < 2^31; otherwise FGS_EINVAL (bad dims or params, null pointers) before anything
 * touches the device. */
typedef struct FgsSurfaceDims {
    int32_t batch, height, width;
} FgsSurfaceDims;
typedef struct FgsSurfaceParams {
    float fx, fy, cx, cy;              /* <= 0: see above */
    float depth_scale;                 /* 2.5  (viewer.hpp:143) */
    int32_t subsample;                 /* 1 */
    float opacity;                     /* 0.9 */
    float normalize_extent;            /* 3.0 (viewer.cpp:385-386); <= 0: neither centred nor normalised */
    /* SurfaceGaussianParams (pointcloud.hpp:18-26) */
    float base_size;                   /* 0.008 */
    float aspect_ratio;                /* 5 */
    float edge_threshold;              /* 0.15 */
    float edge_shrink;                 /* 0.3 */
    float min_confidence;              /* 0.1 */
    float gradient_scale;              /* 50 */
    float normal_strength;             /* 1 */
    /* SilhouetteWrapParams (pointcloud.hpp:35-43) */
    int32_t wrap_enabled;              /* 1 */
    float wrap_edge_threshold;         /* 0.15 */
    int32_t wrap_layers;               /* 3 */
    float wrap_layer_spacing;          /* 0.5 */
    float wrap_opacity_falloff;        /* 0.7 */
    float wrap_max_angle;              /* 75; carried for completeness: the reference never reads it */
    float wrap_aspect;                 /* 2 */
    /* VolumetricShellParams (pointcloud.hpp:54-63) */
    int32_t shell_enabled;             /* 1 */
    float shell_thickness;             /* 0.3 */
    float shell_back_opacity;          /* 0.6 */
    float shell_back_darken;           /* 0.8 */
    int32_t shell_connect_walls;       /* 1 */
    int32_t shell_wall_segments;       /* 3 */
    float shell_wall_opacity;          /* 0.5 */
    float shell_edge_threshold;        /* 0.1 */
    /* AdaptiveDensityParams (pointcloud.hpp:72-80) */
    int32_t density_enabled;           /* 1 */
    float density_gradient_threshold;  /* 0.08 */
    int32_t density_extra_count;       /* 4 */
    float density_position_jitter;     /* 0.6 */
    float density_size_variance;       /* 0.3 */
    float density_opacity_scale;       /* 0.7 */
    uint32_t seed;                     /* 12345 */
} FgsSurfaceParams;
#define FGS_SURFACE_STATE_OFFSET 64
#define FGS_SURFACE_KEPT 1
#define FGS_SURFACE_BASE 2
#define FGS_SURFACE_BACK 4
#define FGS_SURFACE_WALLS 8
#define FGS_SURFACE_WRAPS 16
#define FGS_SURFACE_FILLS 32
int fgs_surface_workspace_bytes(const FgsSurfaceDims *dims, const FgsSurfaceParams *params, size_t *scratch_bytes);
int fgs_surface_count(const FgsSurfaceDims *dims, const FgsSurfaceParams *params, const float *depth, void *scratch,
                      int32_t *offsets, void *stream);
int fgs_surface_emit(const FgsSurfaceDims *dims, const FgsSurfaceParams *params, const float *depth, const float *color,
                     void *scratch, const int32_t *offsets, float *o_positions, float *o_scales, float *o_rotations,
                     float *o_colors, float *o_opacities, int64_t capacity, void *stream);

/* Feature-guided SAAG (the reference's experiment 3, FeatureGuidedSAAG, scripts/models/gaussian_decoder_models.py:1422-1490): the emit
 * above with six of its parameters modulated per patch of a guide map, and the gradient of the rows with respect to that map.
 *   mods       (B, 6, Hp, Wp) fp32 contiguous DEVICE; channels in the order of the decoder's dict:
 *              aspect_ratio_mult, edge_threshold_add, edge_shrink_mult, normal_strength_mult, base_size_mult, opacity_mult
 *   patch      the point at pixel (x, y) reads m = mods[b, :, (y Hp) / H, (x Wp) / W]: integer division on PIXEL coordinates
 *   effective  aspect_ratio' = aspect_ratio * m[0]     edge_threshold' = edge_threshold + m[1]    edge_shrink' = edge_shrink * m[2]
 *              normal_strength' = normal_strength * m[3]   base_size' = base_size * m[4]          opacity' = opacity * m[5]
 *              one fp32 operation each, rounded on its own.  Everything else is fgs_surface_emit in its operation order; the effective
 *              values are read by base, normal_scale and edge_factor, by final_opacity, by the slerp parameter (not clamped:
 *              normal_strength' may exceed 1), by wrap_base and the wrap offset (layer + 1) wrap_layer_spacing base_size', and by the
 *              fill jitter.  None of the six feeds a count decision: fgs_surface_count, the flags, the offsets and the row order are
 *              those of the plain cloud.  With m = (1, 0, 1, 1, 1, 1) everywhere the guided emit is BIT-EQUAL to fgs_surface_emit.
 * fgs_surface_emit_guided: one launch on fgs_surface_emit's grid, after fgs_surface_count with the same dims and params.  Also writes
 *     point_rows (B P int32): the first row of every point that has its BASE flag, -1 for every other point.  Capacity and status as
 *     fgs_surface_emit (offsets[B] > capacity: nothing is written, point_rows included, and the first int32 of scratch is 1).
 * fgs_surface_guided_backward: g_mods (B, 6, Hp, Wp) = dL/d mods from the upstream gradients of positions, scales, rotations and
 *     opacities (any may be NULL = zeros; colours carry no gradient).  EVERY element of g_mods is written, a patch without a point
 *     gets exact zeros.  Recomputes each point's forward from depth, mods, the count's scratch (read only) and point_rows; nothing
 *     else is saved.  At the kinks the derivative follows the branch the forward took: `ng > edge_threshold'` is strict; the clamp
 *     of t passes its gradient on the closed interval [0, 1] (as torch.clamp); the lerp and slerp branches of slerp(identity, q, t)
 *     are each differentiated as written.  Covered: base_size through the scales of all five row kinds and the positions of wrap
 *     and fill rows; aspect_ratio through scale.z of base, back, wall and fill rows; edge_threshold and edge_shrink through
 *     edge_factor into those rows' scales and every row's opacity; normal_strength through the rotations of base and fill rows;
 *     opacity through every row's opacity.
 *     One wave per (patch, image) walks the patch's rectangle of grid points and sums six partials in a fixed order; a patch that
 *     can own more than 256 grid points is split over up to 256 waves whose partials a second launch adds in split order, through
 *     bwd_scratch (fgs_surface_guided_backward_bytes; 0 bytes and NULL allowed when no patch is split).  NO atomics: two calls agree
 *     to the bit, and a batch equals its single images to the bit.  fp32, not built to the emit's operation order: agreement
 *     with an fp64 differentiation is to fp32 rounding.
 * Shapes: those of fgs_surface_emit, and mods_h, mods_w >= 1, W mods_w < 2^31, H mods_h < 2^31, B 6 mods_h mods_w < 2^31, mods and
 * point_rows (and g_mods) non-null; otherwise FGS_EINVAL with a message before anything touches the device. */
int fgs_surface_emit_guided(const FgsSurfaceDims *dims, const FgsSurfaceParams *params, const float *depth, const float *color,
                            void *scratch, const int32_t *offsets, const float *mods, int32_t mods_h, int32_t mods_w,
                            float *o_positions, float *o_scales, float *o_rotations, float *o_colors, float *o_opacities,
                            int32_t *point_rows, int64_t capacity, void *stream);
int fgs_surface_guided_backward_bytes(const FgsSurfaceDims *dims, const FgsSurfaceParams *params, int32_t mods_h, int32_t mods_w,
                                      size_t *bytes);
int fgs_surface_guided_backward(const FgsSurfaceDims *dims, const FgsSurfaceParams *params, const float *depth, const void *scratch,
                                const int32_t *offsets, const float *mods, int32_t mods_h, int32_t mods_w, const int32_t *point_rows,
                                const float *g_positions, const float *g_scales, const float *g_rotations, const float *g_opacities,
                                float *g_mods, void *bwd_scratch, void *stream);

/* ------------------------------------------------------------------------------------------
 * GaussianMatchingLoss of the reference's distillation path (scripts/training/train_direct_decoder.py, "TDD" 158-357): the
 * bidirectional Chamfer loss between a predicted and a target cloud.  pred (B, Np, 14), target (B, Nt, 14) fp32 contiguous; a
 * row is position 0..2, scale 3..5, quaternion 6..9, colour 10..12, opacity 13.  pred_keep (B, Np), target_keep (B, Nt): uint8,
 * NULL = all ones.
 *
 * Active rows.  A row is active iff its keep byte is non-zero and (|x| + |y|) + |z| > 1e-6f || |opacity| > 1e-6f, the sums
 * rounded to fp32, a NaN comparing false (the reference's zero-padding filter, TDD:268-273).  n_p, n_t: the active counts of an
 * image.  An image with n_p == 0 or n_t == 0 is SKIPPED: all its terms are 0, its match entries -1, its gradient rows 0; it
 * still counts in the division by B (TDD:263-276, 347).
 *
 * Canonical match (this library's definition; the reference takes the minimum of cdist chunk by chunk with a strict `<`):
 * d2(i, j) = (dx dx + dy dy) + dz dz of the coordinate differences, every operation rounded to fp32; a NaN d2 counts as +inf;
 * the match of an active query is the active candidate with the smallest (d2, j) -- the lowest index wins ties.  Inactive
 * queries get -1.  For ANY input, NaN and Inf included, a written index is -1 or an active row's index.  fwd (B, Np):
 * predictions -> targets; bwd (B, Nt): targets -> predictions.
 *
 * Terms of a non-skipped image (t_m: the matched target of a prediction; p_m: the matched prediction of a target):
 *     position, scale, colour   mean over the 3 n_p elements of (p - t_m)^2      opacity   mean over the n_p elements
 *     rotation                  1 - mean_i |q^p . q^t|, q^ = q / max(|q|, 1e-8f), |q| = sqrt(((q0 q0 + q1 q1) + q2 q2) + q3 q3),
 *                               the dot product (((a0 b0 + a1 b1) + a2 b2) + a3 b3) of the divided components
 *     coverage                  2 cov_position + 0.5 cov_scale + 0.5 cov_colour + 2 cov_opacity, the same four means over the n_t
 *                               targets against p_m
 *     batch                     w_pos position + w_scale scale + w_rot rotation + w_color colour + w_opacity opacity + w_coverage coverage
 * Every per-element value ((p - t)^2, |dot|) is formed in fp32; the sums are accumulated in double in a fixed order (fixed grid,
 * fixed-shape block tree, block partials in block order); means, coverage and batch are formed in double from those sums and
 * each is rounded to fp32 once.  terms (B, 8): position, scale, rotation, colour, opacity, coverage, batch, 0.
 * total = sum_b batch_b / B is the caller's (fresnel_amd/losses.py).
 *
 * Gradient: dL/dpred only, for L = *g_total x total.  Nothing flows through the indices; the target gets none.  Inactive rows and
 * skipped images get exact zeros.  Every operation below is rounded to fp32 on its own (no FMA), divisions and the square
 * root IEEE.  Per image:
 *     gs = *g_total x (1.0f / (float)B)
 *     a3 = 2.0f / (float)(3 n_p)   a1 = 2.0f / (float)n_p   r1 = 1.0f / (float)n_p   b3 = 2.0f / (float)(3 n_t)   b1 = 2.0f / (float)n_t
 *     k_position = (gs w_pos) a3, k_scale = (gs w_scale) a3, k_colour = (gs w_color) a3, k_opacity = (gs w_opacity) a1
 *     gc = gs w_coverage;  c_position = (gc 2.0f) b3, c_scale = (gc 0.5f) b3, c_colour = (gc 0.5f) b3, c_opacity = (gc 2.0f) b1
 * Row i, active, t = target[fwd[i]], channel c of group X in {position, scale, colour, opacity}:
 *     g[c] = k_X (p[c] - t[c]);  then for every target j with bwd[j] == i, in ascending j:  g[c] = g[c] + c_X (p[c] - target[j][c])
 * (any in-degree 0 ... n_t, no float atomics: two calls agree to the bit).  Quaternion: n = |q_p|, cp = n < 1e-8f ? 1e-8f : n,
 * ct likewise of t; dot as above; s = (dot > 0) - (dot < 0) (torch's subgradient: 0 at 0); e = -(((gs w_rot) r1) s);
 * gh[c] = e (t_q[c] / ct);  where the clamp is active (n < 1e-8f) it passes no gradient: g_q[c] = gh[c] / cp;  elsewhere
 * u = ((gh0 q0 + gh1 q1) + gh2 q2) + gh3 q3, v = ((u / cp) / cp) / n, g_q[c] = gh[c] / cp - q[c] v.
 *
 * saved: fwd (B, Np), bwd (B, Nt), counts (B, 2) = (n_p, n_t), int32, in this order without padding; every element is written by
 * the forward and it goes unchanged through the backward.  counts (B, 2) is the same pair as an output.  The backward needs no
 * scratch (NULL is accepted).  FGS_MATCH_TILE: the candidates per LDS tile of the matching kernel -- the size at which its inner
 * loop starts over (the tests put Nt on and beside it).
 * Shapes: 1 <= Np, Nt <= 65536, B <= 65535; otherwise FGS_EINVAL (bad dims, null pointers) / FGS_EUNSUPPORTED before anything
 * touches the device.  Neither call synchronises the host or allocates. */
#define FGS_MATCH_TILE 1024
typedef struct FgsMatchDims {
    int32_t batch, num_pred, num_target;
    float w_pos, w_scale, w_rot, w_color, w_opacity, w_coverage;
} FgsMatchDims;
int fgs_match_workspace_bytes(const FgsMatchDims *dims, size_t *saved_bytes, size_t *scratch_bytes);
int fgs_match_forward(const FgsMatchDims *dims, const float *pred, const float *target, const uint8_t *pred_keep,
                      const uint8_t *target_keep, float *terms, int32_t *counts, void *saved, void *scratch, void *stream);
int fgs_match_backward(const FgsMatchDims *dims, const float *pred, const float *target, const void *saved, const float *g_total,
                       float *g_pred, void *scratch, void *stream);

/* ------------------------------------------------------------------------------------------
 * Gaussian-parameter head of the reference's distillation decoders (scripts/models/direct_slat_decoder.py, "DSD": GaussianHead,
 * 255-358, behind DirectSLatDecoder and MLPSLatDecoder).  raw (B, N, G, 14) fp32 contiguous: the head MLP's output, G Gaussians per
 * voxel; coords (B, N, 4) int32, columns 1..3 = x, y, z; gains: two DEVICE floats, position_offset_scale and scale_factor, never
 * read on the host (the calls can be captured in a graph).  gaussians (B, N G, 14), row n G + k = Gaussian k of voxel n; a row is
 * position 0..2, scale 3..5, quaternion 6..9, colour 10..12, opacity 13 -- GaussianMatchingLoss's layout above.  Per Gaussian, with
 * r = clamp(raw, -10, 10) (+-Inf clamp to +-10, a NaN stays) and centre = clamp(coordinate, 0, 63) / 64 * 2 - 1 whatever the
 * decoder's max_resolution:
 *     position    clamp(centre + tanh(r[0:3]) position_offset_scale, -1, 1)
 *     scale       clamp(softplus(r[3:6]) |scale_factor|, 1e-4, 1)
 *     quaternion  r[6:10] / max(|r[6:10]|, 1e-6),  |q| = sqrt(((q0 q0 + q1 q1) + q2 q2) + q3 q3)
 *     colour, opacity   sigmoid(r[10:14])
 * every operation rounded to fp32 on its own (no FMA).
 *
 * NaN rule (a STATED DIFFERENCE from torch).  The reference looks for NaN on the host (isnan(...).any()) and then replaces every NaN
 * output by 0 (nan_to_num).  Here nothing is read on the host: an output element that would be NaN is written as 0, all four
 * components of a quaternion when any of its raw components is NaN -- the same forward values.  Such an output is a constant of the
 * backward: the raw elements behind it get g_raw = 0 and it adds nothing to the gain gradients, where torch's gradient is
 * NaN-tainted.
 *
 * Gradient.  Every clamp passes the gradient on the closed interval: raw in [-10, 10], the unclamped position in [-1, 1], the
 * unclamped scale in [1e-4, 1].  d|s|/ds = sign(s), 0 at 0.  Quaternion: through the norm where |q| >= 1e-6, else g / 1e-6 per
 * component (the norm is behind the clamp; an all-zero quaternion gives output 0 and gradient g 1e6).
 *     g_raw (B, N, G, 14): every element written.
 *     g_gains, two floats, or NULL: dL/d position_offset_scale = sum g tanh(r) over the open position elements and
 *       dL/d scale_factor = sign(scale_factor) sum g softplus(r) over the open scale elements; the products are exact in double,
 *       added in a fixed order (fixed-shape block tree, one partial pair per block of 256 rows in `scratch`, folded by one block:
 *       thread t adds partials t, t + 256, ..., then a fixed tree) and rounded to fp32 once.  No atomics: two calls agree to the bit.
 * The backward recomputes the forward from raw: nothing is saved.
 *
 * Gated forward (keep (B, N) uint8, non-NULL; inference).  gaussians is packed: the Gaussians of image b's kept voxels (keep byte
 * non-zero), in ascending voxel order, are rows [0, counts[b] G); every row behind them is zero.  counts (B,) int32 = kept VOXELS
 * per image.  Two launches: a scan (one block per image) that writes counts and every voxel's destination to `scratch`, and the head
 * writing each row at its place -- a dropped voxel's threads write the zero rows of the tail, so every row is written exactly once
 * and no atomic is used.  A kept row is bit for bit the ungated call's row of that Gaussian.
 *
 * fgs_slat_head_forward: one launch ungated (keep, counts and scratch may be NULL), two gated.  fgs_slat_head_backward: two
 * launches (one when g_gains is NULL).  scratch (fgs_slat_workspace_bytes; the gated forward and the backward) is written, never
 * read before it is written.  Every output element is written; inputs are never modified.  Neither call synchronises the host or
 * allocates.
 * Shapes: batch = B, voxels = N, per_voxel = G go as three plain integers, as in fgs_gather_* and fgs_asm_propagate_*, not in a dims
 * structure: the set of structures this header declares is closed (tests/test_call_layer.py holds it, and its ctypes side, at
 * fifteen), and three integers need none.  B, N, G >= 1, G <= 64,
 * B N G < 2^31; otherwise FGS_EINVAL (bad dims, null pointers) / FGS_EUNSUPPORTED before anything touches the device. */
int fgs_slat_workspace_bytes(int32_t batch, int32_t voxels, int32_t per_voxel /* B, N, G; B*N*G < 2^31, G <= 64 */, size_t *scratch_bytes);
int fgs_slat_head_forward(int32_t batch, int32_t voxels, int32_t per_voxel, const float *raw, const int32_t *coords,
                          const float *gains /* 2, device */, const uint8_t *keep /* (B,N) or NULL */, float *gaussians,
                          int32_t *counts /* (B,), with keep */, void *scratch, void *stream);
int fgs_slat_head_backward(int32_t batch, int32_t voxels, int32_t per_voxel, const float *raw, const int32_t *coords,
                           const float *gains, const float *g_gaussians, float *g_raw, float *g_gains /* 2, or NULL */, void *scratch,
                           void *stream);

/* ------------------------------------------------------------------------------------------
 * Fused cross-attention of the distillation decoder (DSD: CrossAttention, 63-182): the voxels' queries against the image patches'
 * keys and values, flash-style -- nothing of size N x M is stored.  The inputs are what the module's two Linear layers produce:
 *   q   (B, N, H d) fp32 contiguous, the output of `self.q`;
 *   kv  (B, M, 2, H, d) fp32 contiguous, the output of `self.kv`: kv[:, :, 0] the keys, kv[:, :, 1] the values (DSD:109);
 *   out (B, N, H d), the tensor behind `.transpose(1, 2).reshape(B, N, D)`, ready for `self.proj`.
 * For image b, head h, query n:
 *   scores      s_m = scale <q, k_m> for m < M (the product is formed first, then scaled, as the reference does);
 *   masked row  row_keep (B, N) bytes, may be NULL: where it is 0 every score is -1e4 (the reference's masked_fill).  Such a row
 *               attends uniformly, its output is the mean of v (dropout applies to it), it contributes to g_kv through v only,
 *               and its g_q row is zero;
 *   softmax     p = softmax(s - max(s));
 *   NaN rule    a row is BAD iff its NaN-propagating maximum is not finite: some score is NaN or +Inf, or all are -Inf.  A bad
 *               row's probabilities are 1 / M each (the reference's nan_to_num(nan = 1 / M) behind its softmax), WITHOUT dropout
 *               (the reference drops first and cleans second: the NaN stays NaN and becomes 1 / M unscaled).  A masked row is
 *               never bad: the fill replaces its scores.  Stated difference, as for fgs_slat_*: a bad row is a constant of the
 *               backward -- it contributes to g_kv through v only and its g_q row is zero, where torch's gradient is NaN-tainted;
 *   dropout     dropout_p in [0, 1), 0 = none: p_m <- keep(b, h, n, m) p_m / (1 - dropout_p).  keep is a pure function of a 64-bit
 *               seed -- ONE DEVICE int64, never read on the host; may be NULL when dropout_p is 0 -- and the indices.  With
 *               fmix(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16 (murmur3's finaliser, uint32
 *               arithmetic), lo / hi the seed's low / high 32 bits and row = (b H + h) N + n:
 *                   x = fmix(fmix(row ^ lo) ^ hi ^ (m * 0x9E3779B1));      keep iff (x >> 8) >= T,
 *               T = dropout_p (as fp32) x 2^24 rounded to nearest, ties to even.  tests/attn_checker.py restates it in numpy.
 *               The backward regenerates the mask from the same seed;
 *   output      out = sum_m p_m v_m.  A NaN in v reaches the output as in torch.
 * Backward, with a_m the probabilities after dropout, c_m = keep / (1 - dropout_p), dA_m = <g_out, v_m>, delta = <g_out, out>:
 * dS_m = p_m (c_m dA_m - delta) on open rows and 0 on masked and bad ones; g_q = scale sum_m dS_m k_m; g_k(m) = scale sum_n dS_nm q_n;
 * g_v(m) = sum_n a_nm g_out_n.
 *
 * fp32 end to end on the fp32-input matrix cores (exact fp32 FMA chains).  fgs_attn_forward: ONE launch; a workgroup owns
 * FGS_ATTN_QUERY_BLOCK queries of one (b, h) and walks the keys in LDS tiles of FGS_ATTN_KEY_TILE with an online softmax; any
 * head_dim <= FGS_ATTN_MAX_HEAD_DIM runs zero-padded to 32, 64 or 128.  saved: one float per (b, h, n), max + ln(sum), +Inf for a
 * bad row.  fgs_attn_backward: three launches (delta; g_q by query blocks; g_kv by blocks of FGS_ATTN_KEY_BLOCK keys that sweep all
 * queries) --
 * no float atomics, nothing summed across workgroups, so two calls agree to the bit and an image's result does not depend on
 * its batch.  `out` is the forward's output.  Every element of out, saved, g_q (zero rows included) and g_kv (both halves) is
 * written; scratch is written before it is read; inputs are never modified.  No call synchronises the host or allocates; with
 * a seed TENSOR the calls can be captured (the seed is read at replay).
 * The backward recomputes p = exp(s - saved) with s rounded exactly as in the forward (the unit is compiled without FMA contraction).
 * Shapes go as plain integers (the set of structures of this header is closed): batch = B, queries = N, keys = M, heads = H,
 * head_dim = d, all >= 1; d <= 128; B H N < 2^31; 0 <= dropout_p < 1; otherwise FGS_EINVAL / FGS_EUNSUPPORTED before anything
 * touches the device. */
#define FGS_ATTN_QUERY_BLOCK 128
#define FGS_ATTN_KEY_TILE 32
#define FGS_ATTN_KEY_BLOCK 128
#define FGS_ATTN_MAX_HEAD_DIM 128
int fgs_attn_workspace_bytes(int32_t batch, int32_t queries, int32_t keys, int32_t heads, int32_t head_dim, size_t *saved_bytes,
                             size_t *scratch_bytes);
int fgs_attn_forward(int32_t batch, int32_t queries, int32_t keys, int32_t heads, int32_t head_dim, float scale, float dropout_p,
                     const float *q, const float *kv, const uint8_t *row_keep /* (B,N) or NULL */,
                     const int64_t *seed /* 1, device; NULL with dropout_p 0 */, float *out, void *saved, void *stream);
int fgs_attn_backward(int32_t batch, int32_t queries, int32_t keys, int32_t heads, int32_t head_dim, float scale, float dropout_p,
                      const float *q, const float *kv, const uint8_t *row_keep, const int64_t *seed, const float *out,
                      const void *saved, const float *g_out, float *g_q, float *g_kv, void *scratch, void *stream);

/* ------------------------------------------------------------------------------------------
 * The fused cross-attention with 16-bit tensors, for the distillation step under mixed precision (csrc/fgs_attn_half.hip).
 * dtype selects fp16 (FGS_ATTN_F16) or bf16 (FGS_ATTN_BF16); q, kv, out, g_out, g_q, g_kv are tensors of that ONE type with the
 * shapes and layouts of fgs_attn_*; row_keep, seed, saved (one FP32 per (b, h, n): max + ln(sum), +Inf for a bad row) and scratch
 * (delta, fp32) are as there.
 *
 * DEFINITION: the result is fgs_attn_*'s definition above, evaluated on the 16-bit inputs.  Masked rows, the NaN rule -- decided
 * on the fp32 scores -- and dropout's keep function of (seed, b, h, n, m) are unchanged: the same seed keeps the same elements in
 * every precision.
 *
 * NUMERICAL CONTRACT (the roundings are error against the definition, not part of it):
 *   - every matrix product takes 16-bit operands and accumulates in fp32 in the matrix cores' accumulators;
 *   - scores are never rounded to 16 bits: the scale, the -1e4 row fill, the online softmax (maximum, exp, running sum, rescale),
 *     delta = <g_out, out> (on the stored, rounded `out`) and `saved` are fp32;
 *   - only the operands of the second-stage products are rounded to the 16-bit type, to nearest even: P (after dropout's keep, before
 *     the fp32 normalisation 1 / ((1 - dropout_p) sum)) ahead of O^T += V^T P^T, the probabilities a = c p ahead of dV^T += dO^T A, and
 *     dS = p (c dA - delta) scale ahead of dQ^T += K^T dS^T and dK^T += Q^T dS.  A bad row's 1 / M is applied in fp32 to an exact sum
 *     of v in the forward; in g_v it is a rounded operand like any other probability;
 *   - out, g_q, g_kv are rounded once, at the store.
 * Stated differences from torch's op sequence under autocast: (1) a score beyond 65504 is finite here, where torch's fp16 product
 * overflows to Inf and the row falls to its nan_to_num (1 / M each): a row with one dominant such score returns that key's value
 * row here and the mean of v there; (2) dS in fp16 can underflow for small upstream gradients -- what a gradient scaler is for; bf16
 * needs none.
 *
 * Determinism and buffers as fgs_attn_*: one launch forward, three backward, no float atomics, every sum in a fixed order, bitwise
 * repeatable, an image's out / g_q / g_kv do not depend on its batch, nothing read on the host, capturable; every element of out,
 * saved, g_q and g_kv is written, scratch is written before it is read, the initial content of any of them is irrelevant, inputs are
 * never modified.  The key tile (and the query tile of the key-block backward) is FGS_ATTN_HALF_KEY_TILE; query and key blocks are
 * FGS_ATTN_QUERY_BLOCK and FGS_ATTN_KEY_BLOCK; head_dim runs zero-padded to 32, 64 or 128.  Rows are read with 16-byte loads and
 * written with 8-byte stores when head_dim % 8 == 0 and every 16-bit tensor of the call starts on a 16-byte boundary; any other
 * head_dim or base (a tensor needs 2-byte alignment only) runs the same loops element by element, with the same results.
 * saved_bytes = scratch_bytes = 4 B H N rounded up to 256.  Limits and errors as fgs_attn_*, plus FGS_EINVAL for an unknown dtype;
 * all of it before anything touches the device. */
#define FGS_ATTN_F16 1
#define FGS_ATTN_BF16 2
#define FGS_ATTN_HALF_KEY_TILE 32
int fgs_attn_half_workspace_bytes(int32_t batch, int32_t queries, int32_t keys, int32_t heads, int32_t head_dim, size_t *saved_bytes,
                                  size_t *scratch_bytes);
int fgs_attn_half_forward(int32_t dtype, int32_t batch, int32_t queries, int32_t keys, int32_t heads, int32_t head_dim, float scale,
                          float dropout_p, const void *q, const void *kv, const uint8_t *row_keep /* (B,N) or NULL */,
                          const int64_t *seed /* 1, device; NULL with dropout_p 0 */, void *out, void *saved, void *stream);
int fgs_attn_half_backward(int32_t dtype, int32_t batch, int32_t queries, int32_t keys, int32_t heads, int32_t head_dim, float scale,
                           float dropout_p, const void *q, const void *kv, const uint8_t *row_keep, const int64_t *seed,
                           const void *out, const void *saved, const void *g_out, void *g_q, void *g_kv, void *scratch, void *stream);

/* ------------------------------------------------------------------------------------------
 * Fused wave self-attention of the consistency view synthesizer (scripts/models/consistency_view_synthesis.py, "CVS":
 * FresnelWaveAttention, 191-246): multi-head self-attention over the N = grid_h grid_w tokens of a feature map, with an interference
 * term that depends on the two tokens' grid distance added to the logits, flash-style -- nothing of size N x N is stored.
 *   qkv         (B, N, 3, H, d) fp32 contiguous, the output of `to_qkv` as it is (chunk(3, -1), then view(B, N, H, d)): qkv[:, :, 0]
 *               the queries, [:, :, 1] the keys, [:, :, 2] the values.  Read in place;
 *   token n     sits at y = n / grid_w, x = n % grid_w;
 *   wavelength  ONE DEVICE float (the module's learnable scalar), read by the kernels, never on the host;
 *   out         (B, N, H d), the tensor behind `.transpose(1, 2).reshape(B, N, H d)`, ready for `to_out`.
 * For image b, head h, query n and key m, with dy, dx the tokens' coordinate differences and lambda = wavelength:
 *   score       s(n, m) = (<q_n, k_m> scale) + bias(n, m): the product is formed first, then scaled; the bias is NOT scaled;
 *   bias        every operation rounded to fp32 on its own, in the reference's order (CVS:229-238), divide and square root IEEE,
 *               cosf / sinf the accurate ones (phases reach hundreds of radians at the default wavelength):
 *                   dist = sqrtf((dy*dy + dx*dx) + 1e-8f)
 *                   den  = fabsf(lambda) * (float)grid_h + 1e-6f        -- grid_h, not grid_w, whatever the grid's shape
 *                   phi  = (6.2831855f * dist) / den
 *                   bias = 0.1f * cosf(phi)
 *   softmax     p = softmax(s - max(s)) as in fgs_attn_*, without mask and without dropout (the module has neither);
 *   NaN         the module has no nan_to_num and none is added.  A row whose NaN-propagating maximum is not finite (a NaN or +Inf
 *               score, or every score -Inf) gets a NaN output row, as torch's softmax gives, and its `saved` value is NaN; the other
 *               rows keep the bits of a clean run.  The backward lets it propagate as torch does: NaN in that (b, h)'s g_qkv and
 *               in g_wavelength; every other (b, h) keeps the bits of a clean run;
 *   output      out = sum_m p_m v_m.
 * Backward, with dA(n, m) = <g_out_n, v_m>, delta_n = <g_out_n, out_n>: dS(n, m) = p (dA - delta); g_q = scale sum_m dS k_m;
 * g_k(m) = scale sum_n dS q_n; g_v(m) = sum_n p g_out_n; and, dS entering UNSCALED,
 *   g_wavelength = sign(lambda) grid_h / den  sum_{b, h, n, m} dS(n, m) 0.1 sin(phi(n, m)) phi(n, m),
 * which is 0 at lambda == 0 (torch's subgradient of abs).  In this factor phi = 6.283185307179586 sqrt((dy*dy + dx*dx) + 1e-8) / den is
 * evaluated in double (den the fp32 value above) and 0.1 sin(phi) phi rounded to fp32 once: the fp32 rounding of a phase of
 * thousands of radians, harmless behind the cosine of the forward, is multiplied by phi here.  The sum is formed in double: per lane,
 * per workgroup in a fixed-shape tree, and over the workgroups in a fixed order by one small launch.
 *
 * fp32 end to end on the fp32-input matrix cores with the tiling of fgs_attn_* (FGS_ATTN_QUERY_BLOCK queries per workgroup, key
 * tiles of FGS_ATTN_KEY_TILE, key blocks of FGS_ATTN_KEY_BLOCK in the backward, head_dim zero-padded to 32, 64 or 128).  The bias
 * depends on (|dy|, |dx|) only: each workgroup builds a table of grid_h grid_w floats in LDS once and adds it by lookup.
 * fgs_wave_attn_forward: ONE launch.  saved: one float per (b, h, n), max + ln(sum).  fgs_wave_attn_backward: four launches (delta;
 * g_q by query blocks, with the wavelength partials; g_k and g_v by key blocks that sweep all queries; the fold -- three when
 * g_wavelength is NULL).  No float atomics, nothing summed across workgroups except by the fold: two calls agree to the bit in every
 * output, and out and g_qkv of an image do not depend on the batch it sits in (g_wavelength sums over the batch).  The backward
 * recomputes p = exp(s - saved) with s rounded exactly as in the forward (the unit is compiled without FMA contraction).
 * saved_bytes: 4 B H N rounded up to 256.  scratch_bytes: the same (delta) plus 8 B H ceil(N / FGS_ATTN_QUERY_BLOCK) rounded up to 256
 * (the partials).  Every element of out, saved, g_qkv (all three thirds) and g_wavelength is written; scratch is written before it
 * is read; inputs are never modified.  No call synchronises the host or allocates: the calls can be captured, and a replay reads
 * the wavelength again.
 * Shapes go as plain integers: batch = B, grid_h, grid_w, heads = H, head_dim = d, all >= 1; d <= FGS_ATTN_MAX_HEAD_DIM;
 * grid_h grid_w <= FGS_WAVE_ATTN_MAX_TOKENS (the tables live in LDS); B H N < 2^31; scale finite; otherwise FGS_EINVAL (bad dims,
 * null pointers, scale) / FGS_EUNSUPPORTED before anything touches the device. */
#define FGS_WAVE_ATTN_MAX_TOKENS 4096
int fgs_wave_attn_workspace_bytes(int32_t batch, int32_t grid_h, int32_t grid_w, int32_t heads, int32_t head_dim, size_t *saved_bytes,
                                  size_t *scratch_bytes);
int fgs_wave_attn_forward(int32_t batch, int32_t grid_h, int32_t grid_w, int32_t heads, int32_t head_dim, float scale,
                          const float *qkv, const float *wavelength /* 1, device */, float *out, void *saved, void *stream);
int fgs_wave_attn_backward(int32_t batch, int32_t grid_h, int32_t grid_w, int32_t heads, int32_t head_dim, float scale,
                           const float *qkv, const float *wavelength, const float *out, const void *saved, const float *g_out,
                           float *g_qkv, float *g_wavelength /* 1, or NULL */, void *scratch, void *stream);

/* ------------------------------------------------------------------------------------------
 * Fused GroupNorm -> SiLU of the consistency view synthesizer's U-Net (CVS: ResBlock, 90-134; the norms of AttentionBlock and of
 * out_conv), with the broadcast add of the time embedding folded into the read.  For x (B, C, HW) fp32 contiguous (NCHW),
 * `groups` dividing C, cpg = C / groups, m = cpg HW; group (b, g) is the cpg ADJACENT channels g cpg ... of image b:
 *   u    = x + channel_bias[b, c]                    (channel_bias (B, C), or NULL -> u = x)
 *   mean = sum_group(u) / m,  var = sum_group((u - mean)^2) / m  (biased),  rstd = 1 / sqrt(var + eps)  (eps INSIDE the root)
 *   y    = weight[c] (u - mean) rstd + bias[c]
 *   out  = y sigmoid(y)   (act = 1, SiLU)   |   out = y   (act = 0)
 * Backward, exact: with s = sigmoid(y), g_y = g_out s (1 + y (1 - s)) (act 0: g_y = g_out), xhat = (u - mean) rstd:
 *   g_weight[c] = sum_{b, hw} g_y xhat;   g_bias[c] = sum_{b, hw} g_y;
 *   g_u = rstd (weight g_y - mean_group(weight g_y) - xhat mean_group(weight g_y xhat));   g_x = g_u;
 *   g_channel_bias[b, c] = sum_hw g_u.
 * Neither u nor y is ever stored: `saved` holds (mean, rstd) per (b, group) and nothing of the activation's size; the backward
 * recomputes xhat, y and sigmoid(y) from x.
 * Moments (this is the definition): TWO-PASS sums of segments, combined pairwise.  A segment is up to FGS_GN_SEGMENT consecutive
 * floats of one channel row, cut at row-relative multiples of FGS_GN_SEGMENT.  Per segment, held in registers: the fp32 sum gives a
 * shift mu; d = sum(u - mu) and q = sum((u - mu)^2) follow in fp32 per lane and in double across the lanes; the segment's pair is
 * (mu + d / n, q - d^2 / n) in double -- exact in mu, so the fp32 rounding of mu does not enter.  A group's pairs are combined by
 * Chan's update in double in a fixed order; mean and rstd are rounded to fp32 once.  E[u^2] - mean^2 is formed nowhere: a group whose
 * mean is 30 standard deviations from zero has the moments of the centred one.
 * The work is cut by segments, not by groups: one wave per segment, B C ceil(HW / FGS_GN_SEGMENT) of them; the cuts are relative to
 * the row, so out, g_x and g_channel_bias of an image do not depend on the batch it sits in.  With HW % 4 == 0 the segments are read
 * and written as float4; with any other HW (groups then start at offsets that are not 16-byte aligned) the same loops run scalar.
 * fgs_gn_silu_forward: two launches (segment moments; fold at the head of the apply launch).  fgs_gn_silu_backward: four (segment
 * sums; per (b, group) fold with g_channel_bias; g_weight and g_bias over the batch, in order, in double; apply).  No float atomics,
 * nothing summed across waves except in a fixed order: two calls agree to the bit in every output.
 * NaN: as in torch, a non-finite value makes its group's output non-finite (and the g_weight / g_bias of its channels); every other
 * (b, group) keeps the bits of a clean run in out, g_x and g_channel_bias.
 * saved_bytes: 8 B groups rounded up to 256.  scratch_bytes: 24 per segment + 24 B C + 8 B groups, each rounded up to 256.  Every
 * element of out, g_x, g_channel_bias, g_weight, g_bias and of saved's B groups pairs is written; scratch is written before it is
 * read; inputs are never modified.  No call synchronises the host or allocates: the calls can be captured.
 * Shapes go as plain integers: batch, channels, hw, groups >= 1, channels % groups == 0; act 0 | 1; eps finite and > 0; x, out, g_out,
 * g_x and scratch 16-byte aligned; B C HW < 2^31 (32-bit indices); otherwise FGS_EINVAL (dims, act, eps, null or misaligned pointers)
 * / FGS_EUNSUPPORTED (size) before anything touches the device. */
#define FGS_GN_SEGMENT 4096
int fgs_gn_silu_workspace_bytes(int32_t batch, int32_t channels, int32_t hw, int32_t groups, size_t *saved_bytes,
                                size_t *scratch_bytes);
int fgs_gn_silu_forward(int32_t batch, int32_t channels, int32_t hw, int32_t groups, int32_t act, float eps, const float *x,
                        const float *channel_bias /* (B,C) or NULL */, const float *weight, const float *bias, float *out,
                        void *saved, void *scratch, void *stream);
int fgs_gn_silu_backward(int32_t batch, int32_t channels, int32_t hw, int32_t groups, int32_t act, float eps, const float *x,
                         const float *channel_bias, const float *weight, const float *bias, const void *saved, const float *g_out,
                         float *g_x, float *g_channel_bias /* (B,C) or NULL */, float *g_weight, float *g_bias, void *scratch,
                         void *stream);

/* ------------------------------------------------------------------------------------------
 * Pixel terms of the consistency view synthesizer's losses (QualityAwareCVSLoss, scripts/models/quality_aware_losses.py "QAL";
 * ConsistencyLoss, CVS:844-941) and the Euler step of the latter.  All tensors fp32, contiguous, DEVICE: pred, target, ema and
 * g_pred (B, C, H, W); depth, mask and saved's plane (B, 1, H, W); B = images, C = channels.  Shapes and flags go as plain integers.
 * All arithmetic on the data is in fp32, each operation rounded on its own (no FMA contraction, IEEE division); the sums are in double.
 *
 * Mask (QAL:21-68).  lap = |(((d[y-1] + d[y+1]) + d[x-1]) + d[x+1]) - 4 d|, the neighbour indices taken modulo H / W as torch.roll
 * does: with H == 1 a vertical neighbour is the pixel itself, with H == 2 both are the same row; likewise W.
 *   m = sigmoid(-sharpness (lap - threshold)) = 1 / (1 + exp(sharpness (lap - threshold)))
 * Without FGS_CVS_QUALITY m = 1 and depth is not read for it.  fgs_cvs_loss_forward writes m to `saved` when the flag is set and
 * fgs_cvs_loss_backward reads it from there; nothing else of the images' size is kept.  fgs_cvs_quality_mask writes the same plane
 * alone; a pixel's m depends on its own image only.
 *
 * Terms, out = float[4]; a term that is not requested is written as 0.
 *   out[0] l1_weighted  mean over B C H W of m |p - t|                                                        (always)
 *   out[1] consistency  mean over B C H W of |p - e| (FGS_CVS_CONS_L1, QAL:265) or of (p - e)^2 (FGS_CVS_CONS_MSE, CVS:935);
 *                       the two flags exclude each other.  With m = 1 and the MSE form the same kernels serve ConsistencyLoss
 *   out[2] boundary     (FGS_CVS_BOUNDARY, QAL:275-291)  pe = (sum_c |p - t|) / C;
 *                       bx[y, x] = (|d[y, x] - d[y, x+1]| > 0.01f), by[y, x] = (|d[y, x] - d[y+1, x]| > 0.01f), over the W - 1 /
 *                       H - 1 interior differences, no wrap.  (torch's `tensor > 0.01` on fp32 is exactly "greater than the fp32
 *                       value of 0.01": no fp32 value lies between that and the double 0.01.)
 *                       term = sum(pe bx) / (B H (W-1)) + sum(pe by) / (B (H-1) W); pe bx is a PRODUCT: a NaN pe reaches the
 *                       term through a zero bit too, as in torch
 *   out[3] gradient     (FGS_CVS_GRADIENT, QAL:71-100)  sum |p[y, x] - p[y, x+1]| m[y, x] / (B C H (W-1))
 *                       + sum |p[y, x] - p[y+1, x]| m[y, x] / (B C (H-1) W)
 *
 * Backward: ONE launch, a gather -- every element of g_pred is written exactly once by the thread that owns it.  g_terms = DEVICE
 * float[4], the upstream gradients of the four terms, read on the device (the entry of a term that is off is not read): the call
 * can be captured and its caller never reads the host.  sgn(a, b) = (a > b) - (a < b): 0 on a tie, decided by comparison and never
 * by the sign of a difference (which may be a flushed denormal).  g_pred[b, c, y, x] is the sum of
 *   g0 sgn(p, t) m / (B C H W)
 *   g1 sgn(p, e) / (B C H W)                    | g1 2 (p - e) / (B C H W) with FGS_CVS_CONS_MSE
 *   g2 sgn(p, t) / C (bx[y, x] [x < W-1] / (B H (W-1)) + by[y, x] [y < H-1] / (B (H-1) W))
 *   g3 (([x < W-1] m[y, x] sgn(p[y, x], p[y, x+1]) - [x > 0] m[y, x-1] sgn(p[y, x-1], p[y, x])) / (B C H (W-1))
 *       + ([y < H-1] m[y, x] sgn(p[y, x], p[y+1, x]) - [y > 0] m[y-1, x] sgn(p[y-1, x], p[y, x])) / (B C (H-1) W))
 * The gradient reaches pred only (the reference's op sequence would also differentiate depth, target and ema; the product wrapper
 * refuses such inputs with backend "hip").
 *
 * Kernels.  A work item is a group of V consecutive pixels of one row of one image, looping over the C planes; mask and boundary bits
 * are computed once per pixel.  V = 4 (16-byte accesses) when W % 4 == 0 and every pointer of the call is 16-byte aligned, else V = 1.
 * FGS_CVS_THREADS threads, grid-stride, at most FGS_CVS_MAX_GRID blocks.  Neighbour reads of depth, pred and mask go to global memory
 * through the caches.  A thread sums its items in order, a block its threads in a fixed order, a one-block final kernel the blocks
 * in a fixed order, in double; no atomics: two runs give the same bits.  fgs_cvs_loss_forward: two launches (the pass, the final
 * kernel); fgs_cvs_loss_backward, fgs_cvs_quality_mask, fgs_cvs_euler_step: one each.  No fast-math: a NaN / Inf in pred makes every
 * term it enters non-finite and no other (m comes from depth alone).
 * saved_bytes: 4 B H W rounded up to 256 with FGS_CVS_QUALITY, else 0 (saved may then be NULL).  scratch_bytes: 6 doubles per block
 * of the largest grid, rounded up to 256.  Every element of out[4], g_pred, mask and saved's plane is written; scratch is written
 * before it is read; inputs are never modified.  No call synchronises the host or allocates.
 * Checks, on the host, before anything touches the device: every extent >= 1; B C H W < 2^31; known flags, not both consistency forms;
 * with FGS_CVS_BOUNDARY or FGS_CVS_GRADIENT H >= 2 and W >= 2 (the reference returns NaN there, the mean of an empty tensor);
 * threshold and sharpness finite with FGS_CVS_QUALITY; depth non-NULL with FGS_CVS_QUALITY or _BOUNDARY, ema with a consistency
 * form; otherwise FGS_EINVAL.
 *
 * Euler step (CVS:916-926).  t = timestep[b] (int64), a = sac[t], a' = sac[max(t - 1, 0)], sac = sqrt_alphas_cumprod, float[steps]:
 *   x_prev = clamp(a' x0 + ((1 - a') / ((1 - a) + 1e-8f)) (noisy - a x0), -1, 1)   in this association order, torch's
 *   t_prev[b] = float(max(t - 1, 0))
 * over (images, channels, hw) tensors; V = 4 when channels hw % 4 == 0 and x0_pred, noisy and x_prev are 16-byte aligned.  A timestep
 * outside [0, steps) is clamped into the table: memory-safe, and a difference from torch, which would assert. */
#define FGS_CVS_QUALITY 1
#define FGS_CVS_CONS_L1 2
#define FGS_CVS_CONS_MSE 4       /* exclusive with FGS_CVS_CONS_L1 */
#define FGS_CVS_BOUNDARY 8
#define FGS_CVS_GRADIENT 16
#define FGS_CVS_THREADS 256
#define FGS_CVS_MAX_GRID 2048
int fgs_cvs_loss_workspace_bytes(int32_t images, int32_t channels, int32_t height, int32_t width, int32_t flags,
                                 size_t *saved_bytes, size_t *scratch_bytes);
int fgs_cvs_quality_mask(int32_t images, int32_t height, int32_t width, float threshold, float sharpness, const float *depth,
                         float *mask, void *stream);
int fgs_cvs_loss_forward(int32_t images, int32_t channels, int32_t height, int32_t width, int32_t flags, float threshold,
                         float sharpness, const float *pred, const float *target, const float *depth /* or NULL */,
                         const float *ema /* or NULL */, float *out /* 4 */, void *saved, void *scratch, void *stream);
int fgs_cvs_loss_backward(int32_t images, int32_t channels, int32_t height, int32_t width, int32_t flags, float threshold,
                          float sharpness, const float *pred, const float *target, const float *depth, const float *ema,
                          const void *saved, const float *g_terms /* 4 */, float *g_pred, void *stream);
int fgs_cvs_euler_step(int32_t images, int32_t channels, int32_t hw, int32_t steps, const float *sqrt_alphas_cumprod,
                       const int64_t *timestep, const float *x0_pred, const float *noisy, float *x_prev,
                       float *t_prev /* images */, void *stream);

/* ------------------------------------------------------------------------------------------
 * Importance-subsampling hand-off between decoder and rasterizer (--stochastic_k; reference
 * scripts/training/train_gaussian_decoder.py:1160-1187): the n_out Gaussians whose indices torch.multinomial
 * drew (DEVICE int64 (n_out,), unique, shared by the batch) are gathered out of every (B, n_in, .) tensor into
 * (B, n_out, .) in one launch; the backward scatters the (B, n_out, .) gradients back and zero-fills the rest.
 *   phase_channels 0 (no phases) | 1 (B,N) | 3 (B,N,3). */
int fgs_gather_forward(int32_t batch, int32_t n_in, int32_t n_out, int32_t phase_channels, const int64_t *indices,
                       const float *pos, const float *scale, const float *quat, const float *color,
                       const float *opacity, const float *phase, float *o_pos, float *o_scale, float *o_quat,
                       float *o_color, float *o_opacity, float *o_phase, void *stream);
int fgs_gather_backward(int32_t batch, int32_t n_in, int32_t n_out, int32_t phase_channels, const int64_t *indices,
                        const float *g_o_pos, const float *g_o_scale, const float *g_o_quat, const float *g_o_color,
                        const float *g_o_opacity, const float *g_o_phase, float *g_pos, float *g_scale, float *g_quat,
                        float *g_color, float *g_opacity, float *g_phase, void *stream);

/* Per-stage hipEvent timers (profiling aid; SURVEY §5 "tracing").  When enabled, every stage
 * launched by the fgs_*_forward / fgs_*_backward entry points is bracketed by an event pair on the caller's
 * stream.  fgs_stage_timing_read synchronises on the recorded events, ADDS the elapsed milliseconds per
 * stage to ms[FGS_NUM_STAGES] and the number of launches to count[FGS_NUM_STAGES], and clears
 * the record.  Stage order: project, depth_sort, dup_emit, tile_sort, tile_ranges, composite_fwd,
 * composite_bwd, project_bwd, and for the splat renderers (ASM / wave field): splat_fwd, field_fwd (FFTs,
 * transfer function, plane sum, normalisation and output), field_bwd (their adjoints), splat_bwd.
 * The Fourier renderer reports its projection under project, the forward product under splat_fwd, maximum and output under
 * field_fwd, the gradient image under field_bwd, the backward product under splat_bwd and the adjoint under project_bwd.
 * enable: 0 = off, 1 = all stages, otherwise a mask with bit (stage + 1) per selected stage -- every event
 * pair costs a few microseconds of stream time, so a benchmark times only the kernel it reports.
 * (The only entry points that allocate or synchronise; never called by the product path.) */
#define FGS_NUM_STAGES 12
int fgs_stage_timing_enable(int enable);
int fgs_stage_timing_read(float *ms, int32_t *count);

const char *fgs_last_error(void);
const char *fgs_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FGS_H */
