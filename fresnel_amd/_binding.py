"""ctypes binding of libfgs_hip.so (include/fgs.h).  No torch types cross this boundary:
only raw device pointers, sizes and the HIP stream handle.

The product path FAILS LOUDLY when the HIP library is missing -- there is no CPU fallback.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FGS_LIB", os.path.join(_HERE, "_lib", "libfgs_hip.so"))  # FGS_LIB: A/B builds

FGS_CAMERA_FLOATS = 24
FGS_TILE = 16

# every symbol include/fgs.h declares (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = [
    "fgs_workspace_bytes", "fgs_saved_layout", "fgs_forward", "fgs_backward", "fgs_count_pairs",
    "fgs_last_error", "fgs_version", "fgs_stage_timing_enable", "fgs_stage_timing_read",
    "fgs_asm_workspace_bytes", "fgs_asm_forward", "fgs_asm_backward",
    "fgs_wave_workspace_bytes", "fgs_wave_forward", "fgs_wave_backward",
    "fgs_fourier_workspace_bytes", "fgs_fourier_forward", "fgs_fourier_backward",
    "fgs_gather_forward", "fgs_gather_backward",
    "fgs_asm_propagate_workspace_bytes", "fgs_asm_propagate_forward", "fgs_asm_propagate_backward",
    "fgs_spectral_workspace_bytes", "fgs_spectral_loss_forward", "fgs_spectral_loss_backward",
    "fgs_helmholtz_loss_forward", "fgs_helmholtz_loss_backward", "fgs_reduction_scratch_bytes",
    "fgs_ssim_workspace_bytes", "fgs_ssim_forward", "fgs_ssim_backward",
    "fgs_pixel_loss_workspace_bytes", "fgs_pixel_loss_stage1", "fgs_pixel_loss_stage2", "fgs_pixel_loss_stage3",
    "fgs_pixel_loss_forward", "fgs_pixel_loss_backward",
    "fgs_head_workspace_bytes", "fgs_head_forward", "fgs_head_backward",
    "fgs_nca_workspace_bytes", "fgs_nca_perceive_forward", "fgs_nca_perceive_backward", "fgs_nca_update_forward",
    "fgs_nca_update_backward",
    "fgs_saag_workspace_bytes", "fgs_saag_inputs_forward", "fgs_saag_refine_forward", "fgs_saag_refine_backward",
    "fgs_physics_workspace_bytes", "fgs_physics_forward", "fgs_physics_backward",
    "fgs_surface_workspace_bytes", "fgs_surface_count", "fgs_surface_emit",
    "fgs_surface_emit_guided", "fgs_surface_guided_backward_bytes", "fgs_surface_guided_backward",
    "fgs_match_workspace_bytes", "fgs_match_forward", "fgs_match_backward",
]

STAGES = ["project", "depth_sort", "dup_emit", "tile_sort", "tile_ranges", "composite_fwd",
          "composite_bwd", "project_bwd", "splat_fwd", "field_fwd", "field_bwd", "splat_bwd"]


FWD_EXIT_OFF, FWD_EXIT_ON = 0x100, 0x200  # include/fgs.h: flags of FgsDims.fwd_variant


class FgsDims(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("num_gaussians", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("max_radius", ctypes.c_float), ("background", ctypes.c_float * 3),
                ("use_phase", ctypes.c_int32), ("phase_amplitude", ctypes.c_float),
                ("num_cameras", ctypes.c_int32), ("saturation_skip", ctypes.c_int32),
                ("seg_len", ctypes.c_int32), ("fwd_variant", ctypes.c_int32), ("bin_mode", ctypes.c_int32),
                ("tile_w", ctypes.c_int32), ("sort_mode", ctypes.c_int32), ("dup_capacity", ctypes.c_uint32)]


class FgsSavedLayout(ctypes.Structure):
    _fields_ = [("total_bytes", ctypes.c_size_t), ("rec", ctypes.c_size_t),
                ("depth_key", ctypes.c_size_t), ("tile_count", ctypes.c_size_t),
                ("order", ctypes.c_size_t), ("dup_off", ctypes.c_size_t), ("counters", ctypes.c_size_t),
                ("ranges", ctypes.c_size_t), ("tile_order", ctypes.c_size_t), ("dup_ids", ctypes.c_size_t),
                ("pix_state", ctypes.c_size_t), ("phase_ckpt", ctypes.c_size_t),
                ("dup_capacity", ctypes.c_size_t),
                ("tiles_x", ctypes.c_int32), ("tiles_y", ctypes.c_int32),
                ("seg_off", ctypes.c_size_t), ("seg_tile", ctypes.c_size_t), ("seg_ckpt", ctypes.c_size_t),
                ("seg_capacity", ctypes.c_size_t), ("seg_len", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("unit_order", ctypes.c_size_t), ("fwd_open", ctypes.c_size_t),
                ("fwd_close", ctypes.c_size_t)]


class FgsAsmDims(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("num_gaussians", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("max_radius", ctypes.c_float), ("background", ctypes.c_float * 3),
                ("num_planes", ctypes.c_int32), ("depth_near", ctypes.c_float),
                ("depth_far", ctypes.c_float), ("focal_depth", ctypes.c_float),
                ("pixel_pitch", ctypes.c_double), ("phase_channels", ctypes.c_int32),
                ("num_cameras", ctypes.c_int32), ("bin_mode", ctypes.c_int32)]


class FgsWaveDims(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("num_gaussians", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("max_radius", ctypes.c_float), ("background", ctypes.c_float * 3),
                ("phase_channels", ctypes.c_int32), ("num_cameras", ctypes.c_int32)]


class FgsFourierDims(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("num_gaussians", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("background", ctypes.c_float * 3), ("num_cameras", ctypes.c_int32)]


class FgsSpectralDims(ctypes.Structure):
    _fields_ = [("images", ctypes.c_int32), ("channels", ctypes.c_int32), ("height", ctypes.c_int32),
                ("width", ctypes.c_int32), ("mode", ctypes.c_int32), ("cutoff", ctypes.c_float),
                ("high_weight", ctypes.c_float), ("focal_depth", ctypes.c_float), ("reserved", ctypes.c_int32)]


FGS_SSIM_MAX_TAPS = 15
FGS_SSIM_GRAD_X, FGS_SSIM_GRAD_Y, FGS_SSIM_NONNEGATIVE, FGS_SSIM_PER_IMAGE = 1, 2, 4, 8


class FgsSsimDims(ctypes.Structure):
    _fields_ = [("images", ctypes.c_int32), ("channels", ctypes.c_int32), ("height", ctypes.c_int32),
                ("width", ctypes.c_int32), ("taps", ctypes.c_float * FGS_SSIM_MAX_TAPS), ("num_taps", ctypes.c_int32),
                ("c1", ctypes.c_float), ("c2", ctypes.c_float), ("flags", ctypes.c_int32)]


FGS_PIXEL_MAX_BOUNDARIES = 65
FGS_PIXEL_RGB, FGS_PIXEL_DENSITY, FGS_PIXEL_BOUNDARY, FGS_PIXEL_HARD_MASK, FGS_PIXEL_DEPTH = 1, 2, 4, 8, 16
# slots of the pixel loss's `stats` array of doubles (include/fgs.h); the CROSS-RANK pairs a data-parallel caller sums after
# stage 1, 2 and 3
(FGS_PIXEL_STAT_RGB, FGS_PIXEL_STAT_BOUNDARY, FGS_PIXEL_STAT_DEPTH, FGS_PIXEL_STAT_SUM_X, FGS_PIXEL_STAT_SUM_Y,
 FGS_PIXEL_STAT_SSD_X, FGS_PIXEL_STAT_SSD_Y, FGS_PIXEL_STAT_SGN, FGS_PIXEL_STAT_SGN_U) = range(9)
FGS_PIXEL_STAT_SLOTS = 16
FGS_PIXEL_CROSS_RANK = {1: slice(3, 5), 2: slice(5, 7), 3: slice(7, 9)}


class FgsPixelLossDims(ctypes.Structure):
    _fields_ = [("images", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("world", ctypes.c_int32), ("vlm_weight", ctypes.c_float),
                ("threshold", ctypes.c_float), ("num_boundaries", ctypes.c_int32),
                ("boundaries", ctypes.c_float * FGS_PIXEL_MAX_BOUNDARIES)]


class FgsHeadDims(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("points", ctypes.c_int32), ("k_full", ctypes.c_int32),
                ("k_used", ctypes.c_int32), ("channels", ctypes.c_int32), ("xy_gain", ctypes.c_float),
                ("edge_scale_factor", ctypes.c_float), ("edge_opacity_boost", ctypes.c_float)]


class FgsNcaDims(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("points", ctypes.c_int32), ("state_dim", ctypes.c_int32), ("k", ctypes.c_int32)]


class FgsSaagDims(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("points", ctypes.c_int32), ("channels", ctypes.c_int32),
                ("grid_h", ctypes.c_int32), ("grid_w", ctypes.c_int32),
                ("feat_stride_batch", ctypes.c_int64), ("feat_stride_channel", ctypes.c_int64),
                ("feat_stride_row", ctypes.c_int64), ("residual_scale", ctypes.c_float)]


class FgsPhysicsDims(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("points", ctypes.c_int32), ("k_full", ctypes.c_int32), ("k_used", ctypes.c_int32),
                ("xy_gain", ctypes.c_float), ("focal_depth", ctypes.c_float),
                ("wavelength_min", ctypes.c_float), ("wavelength_max", ctypes.c_float)]


FGS_PHYSICS_RANGE_BYTES = 16  # float z_min, z_max; int32 n_min, n_max (include/fgs.h)


class FgsSurfaceDims(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32)]


class FgsSurfaceParams(ctypes.Structure):
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("depth_scale", ctypes.c_float), ("subsample", ctypes.c_int32), ("opacity", ctypes.c_float),
                ("normalize_extent", ctypes.c_float),
                ("base_size", ctypes.c_float), ("aspect_ratio", ctypes.c_float), ("edge_threshold", ctypes.c_float),
                ("edge_shrink", ctypes.c_float), ("min_confidence", ctypes.c_float), ("gradient_scale", ctypes.c_float),
                ("normal_strength", ctypes.c_float),
                ("wrap_enabled", ctypes.c_int32), ("wrap_edge_threshold", ctypes.c_float), ("wrap_layers", ctypes.c_int32),
                ("wrap_layer_spacing", ctypes.c_float), ("wrap_opacity_falloff", ctypes.c_float),
                ("wrap_max_angle", ctypes.c_float), ("wrap_aspect", ctypes.c_float),
                ("shell_enabled", ctypes.c_int32), ("shell_thickness", ctypes.c_float), ("shell_back_opacity", ctypes.c_float),
                ("shell_back_darken", ctypes.c_float), ("shell_connect_walls", ctypes.c_int32),
                ("shell_wall_segments", ctypes.c_int32), ("shell_wall_opacity", ctypes.c_float),
                ("shell_edge_threshold", ctypes.c_float),
                ("density_enabled", ctypes.c_int32), ("density_gradient_threshold", ctypes.c_float),
                ("density_extra_count", ctypes.c_int32), ("density_position_jitter", ctypes.c_float),
                ("density_size_variance", ctypes.c_float), ("density_opacity_scale", ctypes.c_float), ("seed", ctypes.c_uint32)]


FGS_SURFACE_STATE_OFFSET = 64
(FGS_SURFACE_KEPT, FGS_SURFACE_BASE, FGS_SURFACE_BACK, FGS_SURFACE_WALLS, FGS_SURFACE_WRAPS, FGS_SURFACE_FILLS) = (1, 2, 4, 8, 16, 32)


FGS_MATCH_TILE = 1024  # candidates per LDS tile of the matching kernel (include/fgs.h)


class FgsMatchDims(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("num_pred", ctypes.c_int32), ("num_target", ctypes.c_int32),
                ("w_pos", ctypes.c_float), ("w_scale", ctypes.c_float), ("w_rot", ctypes.c_float),
                ("w_color", ctypes.c_float), ("w_opacity", ctypes.c_float), ("w_coverage", ctypes.c_float)]


class FgsError(RuntimeError):
    pass


_lib = None


def load():
    """Load libfgs_hip.so; raise (never fall back) if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FgsError(
            f"{LIB_PATH} not found: build it with `python -m fresnel_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the HIP rasterizer.")
    # torch first: it carries the process's HIP runtime (libamdhip64.so.7); loading ours before
    # it would bring up a second runtime from /opt/rocm that cannot see torch's device context.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    vp, cp = ctypes.c_void_p, ctypes.POINTER
    lib.fgs_last_error.restype = ctypes.c_char_p
    lib.fgs_version.restype = ctypes.c_char_p
    if b"EXPERIMENT" in lib.fgs_version():  # an A/B build selected through FGS_LIB: say so, once, where nobody can miss it
        import sys
        sys.stderr.write(f"fresnel_amd: loaded {LIB_PATH}: {lib.fgs_version().decode()}\n")
    lib.fgs_workspace_bytes.argtypes = [cp(FgsDims), cp(ctypes.c_size_t), cp(ctypes.c_size_t)]
    lib.fgs_saved_layout.argtypes = [cp(FgsDims), cp(FgsSavedLayout)]
    lib.fgs_forward.argtypes = [cp(FgsDims)] + [vp] * 12
    lib.fgs_backward.argtypes = [cp(FgsDims)] + [vp] * 18
    lib.fgs_count_pairs.argtypes = [cp(FgsDims), vp, vp, vp]
    lib.fgs_stage_timing_enable.argtypes = [ctypes.c_int]
    lib.fgs_stage_timing_read.argtypes = [cp(ctypes.c_float), cp(ctypes.c_int32)]
    lib.fgs_stage_timing_enable.restype = ctypes.c_int
    lib.fgs_stage_timing_read.restype = ctypes.c_int
    lib.fgs_asm_workspace_bytes.argtypes = [cp(FgsAsmDims), cp(ctypes.c_size_t), cp(ctypes.c_size_t)]
    lib.fgs_asm_forward.argtypes = [cp(FgsAsmDims)] + [vp] * 12
    lib.fgs_asm_backward.argtypes = [cp(FgsAsmDims)] + [vp] * 19
    lib.fgs_wave_workspace_bytes.argtypes = [cp(FgsWaveDims), cp(ctypes.c_size_t), cp(ctypes.c_size_t)]
    lib.fgs_wave_forward.argtypes = [cp(FgsWaveDims)] + [vp] * 12
    lib.fgs_wave_backward.argtypes = [cp(FgsWaveDims)] + [vp] * 18
    lib.fgs_fourier_workspace_bytes.argtypes = [cp(FgsFourierDims), cp(ctypes.c_size_t), cp(ctypes.c_size_t)]
    lib.fgs_fourier_forward.argtypes = [cp(FgsFourierDims)] + [vp] * 10
    lib.fgs_fourier_backward.argtypes = [cp(FgsFourierDims)] + [vp] * 15
    for fn in (lib.fgs_fourier_workspace_bytes, lib.fgs_fourier_forward, lib.fgs_fourier_backward):
        fn.restype = ctypes.c_int
    i32 = ctypes.c_int32
    lib.fgs_gather_forward.argtypes = [i32, i32, i32, i32] + [vp] * 14
    lib.fgs_gather_backward.argtypes = [i32, i32, i32, i32] + [vp] * 14
    lib.fgs_gather_forward.restype = lib.fgs_gather_backward.restype = ctypes.c_int
    f32 = ctypes.c_float
    lib.fgs_asm_propagate_workspace_bytes.argtypes = [i32, i32, i32, cp(ctypes.c_size_t)]
    lib.fgs_asm_propagate_forward.argtypes = [i32, i32, i32, ctypes.c_double, i32] + [vp] * 7   # (the pitch is a double: fgs.h)
    lib.fgs_asm_propagate_backward.argtypes = [i32, i32, i32, ctypes.c_double, i32] + [vp] * 9
    lib.fgs_spectral_workspace_bytes.argtypes = [cp(FgsSpectralDims), cp(ctypes.c_size_t), cp(ctypes.c_size_t)]
    lib.fgs_spectral_loss_forward.argtypes = [cp(FgsSpectralDims)] + [vp] * 8
    lib.fgs_spectral_loss_backward.argtypes = [cp(FgsSpectralDims)] + [vp] * 12
    lib.fgs_helmholtz_loss_forward.argtypes = [i32, i32, i32, f32, f32] + [vp] * 5
    lib.fgs_helmholtz_loss_backward.argtypes = [i32, i32, i32, f32, f32] + [vp] * 4
    lib.fgs_reduction_scratch_bytes.argtypes = []
    lib.fgs_ssim_workspace_bytes.argtypes = [cp(FgsSsimDims), cp(ctypes.c_size_t), cp(ctypes.c_size_t)]
    lib.fgs_ssim_forward.argtypes = [cp(FgsSsimDims)] + [vp] * 6
    lib.fgs_ssim_backward.argtypes = [cp(FgsSsimDims)] + [vp] * 8
    lib.fgs_reduction_scratch_bytes.restype = ctypes.c_size_t
    pd = cp(FgsPixelLossDims)
    lib.fgs_pixel_loss_workspace_bytes.argtypes = [pd, cp(ctypes.c_size_t), cp(ctypes.c_size_t)]
    lib.fgs_pixel_loss_stage1.argtypes = [pd] + [vp] * 9
    lib.fgs_pixel_loss_stage2.argtypes = [pd] + [vp] * 5
    lib.fgs_pixel_loss_stage3.argtypes = [pd] + [vp] * 6
    lib.fgs_pixel_loss_forward.argtypes = [pd] + [vp] * 9
    lib.fgs_pixel_loss_backward.argtypes = [pd] + [vp] * 12
    for fn in (lib.fgs_pixel_loss_workspace_bytes, lib.fgs_pixel_loss_stage1, lib.fgs_pixel_loss_stage2,
               lib.fgs_pixel_loss_stage3, lib.fgs_pixel_loss_forward, lib.fgs_pixel_loss_backward):
        fn.restype = ctypes.c_int
    lib.fgs_head_workspace_bytes.argtypes = [cp(FgsHeadDims), cp(ctypes.c_size_t)]
    lib.fgs_head_forward.argtypes = [cp(FgsHeadDims)] + [vp] * 13
    lib.fgs_head_backward.argtypes = [cp(FgsHeadDims)] + [vp] * 16
    for fn in (lib.fgs_head_workspace_bytes, lib.fgs_head_forward, lib.fgs_head_backward):
        fn.restype = ctypes.c_int
    nd = cp(FgsNcaDims)
    lib.fgs_nca_workspace_bytes.argtypes = [nd, cp(ctypes.c_size_t)]
    lib.fgs_nca_perceive_forward.argtypes = [nd] + [vp] * 4
    lib.fgs_nca_perceive_backward.argtypes = [nd] + [vp] * 4
    lib.fgs_nca_update_forward.argtypes = [nd] + [vp] * 4 + [f32, vp, vp]
    lib.fgs_nca_update_backward.argtypes = [nd] + [vp] * 3 + [f32] + [vp] * 5
    for fn in (lib.fgs_nca_workspace_bytes, lib.fgs_nca_perceive_forward, lib.fgs_nca_perceive_backward,
               lib.fgs_nca_update_forward, lib.fgs_nca_update_backward):
        fn.restype = ctypes.c_int
    sd = cp(FgsSaagDims)
    lib.fgs_saag_workspace_bytes.argtypes = [sd, cp(ctypes.c_size_t)]
    lib.fgs_saag_inputs_forward.argtypes = [sd] + [vp] * 8
    lib.fgs_saag_refine_forward.argtypes = [sd] + [vp] * 17
    lib.fgs_saag_refine_backward.argtypes = [sd] + [vp] * 19
    for fn in (lib.fgs_saag_workspace_bytes, lib.fgs_saag_inputs_forward, lib.fgs_saag_refine_forward,
               lib.fgs_saag_refine_backward):
        fn.restype = ctypes.c_int
    phd = cp(FgsPhysicsDims)
    lib.fgs_physics_workspace_bytes.argtypes = [phd, cp(ctypes.c_size_t)]
    lib.fgs_physics_forward.argtypes = [phd] + [vp] * 13
    lib.fgs_physics_backward.argtypes = [phd] + [vp] * 15
    for fn in (lib.fgs_physics_workspace_bytes, lib.fgs_physics_forward, lib.fgs_physics_backward):
        fn.restype = ctypes.c_int
    sfd, sfp = cp(FgsSurfaceDims), cp(FgsSurfaceParams)
    lib.fgs_surface_workspace_bytes.argtypes = [sfd, sfp, cp(ctypes.c_size_t)]
    lib.fgs_surface_count.argtypes = [sfd, sfp] + [vp] * 4
    lib.fgs_surface_emit.argtypes = [sfd, sfp] + [vp] * 9 + [ctypes.c_int64, vp]
    lib.fgs_surface_emit_guided.argtypes = [sfd, sfp] + [vp] * 5 + [ctypes.c_int32] * 2 + [vp] * 6 + [ctypes.c_int64, vp]
    lib.fgs_surface_guided_backward_bytes.argtypes = [sfd, sfp, ctypes.c_int32, ctypes.c_int32, cp(ctypes.c_size_t)]
    lib.fgs_surface_guided_backward.argtypes = [sfd, sfp] + [vp] * 4 + [ctypes.c_int32] * 2 + [vp] * 8
    for fn in (lib.fgs_surface_workspace_bytes, lib.fgs_surface_count, lib.fgs_surface_emit, lib.fgs_surface_emit_guided,
               lib.fgs_surface_guided_backward_bytes, lib.fgs_surface_guided_backward):
        fn.restype = ctypes.c_int
    md = cp(FgsMatchDims)
    lib.fgs_match_workspace_bytes.argtypes = [md, cp(ctypes.c_size_t), cp(ctypes.c_size_t)]
    lib.fgs_match_forward.argtypes = [md] + [vp] * 9
    lib.fgs_match_backward.argtypes = [md] + [vp] * 7
    for fn in (lib.fgs_match_workspace_bytes, lib.fgs_match_forward, lib.fgs_match_backward):
        fn.restype = ctypes.c_int
    for fn in (lib.fgs_asm_propagate_workspace_bytes, lib.fgs_asm_propagate_forward, lib.fgs_asm_propagate_backward,
               lib.fgs_spectral_workspace_bytes, lib.fgs_spectral_loss_forward, lib.fgs_spectral_loss_backward,
               lib.fgs_helmholtz_loss_forward, lib.fgs_helmholtz_loss_backward,
               lib.fgs_ssim_workspace_bytes, lib.fgs_ssim_forward, lib.fgs_ssim_backward):
        fn.restype = ctypes.c_int
    for fn in (lib.fgs_asm_workspace_bytes, lib.fgs_asm_forward, lib.fgs_asm_backward,
               lib.fgs_wave_workspace_bytes, lib.fgs_wave_forward, lib.fgs_wave_backward):
        fn.restype = ctypes.c_int
    for fn in (lib.fgs_workspace_bytes, lib.fgs_saved_layout, lib.fgs_forward, lib.fgs_backward,
               lib.fgs_count_pairs):
        fn.restype = ctypes.c_int
    _lib = lib
    return lib


def version():
    """fgs_version() of the loaded library (experiment builds list their defines there)."""
    return load().fgs_version().decode()


def check(rc, what):
    if rc != 0:
        raise FgsError(f"{what} failed (rc={rc}): {load().fgs_last_error().decode()}")


def make_dims(batch, num_gaussians, width, height, max_radius=64.0, background=(0.0, 0.0, 0.0),
              use_phase=False, phase_amplitude=0.25, num_cameras=1, saturation_skip=False, tuning=None, dup_capacity=0):
    """`tuning`: optional dict of FgsDims overrides {seg_len, fwd_variant, bin_mode, tile_w, sort_mode} (0 / absent = automatic), and
    `fwd_exit`: 0 | 1 | -1 = the exiting depth-split forward automatic | on | off -- the FGS_FWD_EXIT_ON / _OFF flag of FgsDims.fwd_variant.
    `dup_capacity`: room for that many (tile, Gaussian) duplicates instead of the worst case (0 = worst case; a call that needs
    more overflows: NaN images, zero gradients, saved.counters[1] = 1 -- include/fgs.h)."""
    if isinstance(dup_capacity, bool) or int(dup_capacity) != dup_capacity or not 0 <= int(dup_capacity) <= 0xFFFFFFFF:
        raise FgsError(f"dup_capacity must be an integer in [0, 2^32), got {dup_capacity!r}")
    d = FgsDims()
    d.batch, d.num_gaussians, d.width, d.height = int(batch), int(num_gaussians), int(width), int(height)
    d.max_radius = float(max_radius)
    for i in range(3):
        d.background[i] = float(background[i])
    d.use_phase = 1 if use_phase else 0
    d.phase_amplitude = float(phase_amplitude)
    d.num_cameras = int(num_cameras)
    d.saturation_skip = 1 if saturation_skip else 0
    tuning = dict(tuning or {})
    fwd_exit = int(tuning.pop("fwd_exit", 0))
    for k, v in tuning.items():
        if k not in ("seg_len", "fwd_variant", "bin_mode", "tile_w", "sort_mode"):
            raise FgsError(f"unknown tuning field {k!r}")
        setattr(d, k, int(v))
    if fwd_exit not in (0, 1, -1) or (fwd_exit and d.fwd_variant < 0):
        raise FgsError(f"fwd_exit must be 0, 1 or -1, and 0 with the row-split forward (fwd_variant < 0), got {fwd_exit!r}")
    d.fwd_variant |= {0: 0, 1: FWD_EXIT_ON, -1: FWD_EXIT_OFF}[fwd_exit]
    d.dup_capacity = int(dup_capacity)
    return d


def workspace_bytes(dims):
    s, c = ctypes.c_size_t(0), ctypes.c_size_t(0)
    check(load().fgs_workspace_bytes(ctypes.byref(dims), ctypes.byref(s), ctypes.byref(c)),
          "fgs_workspace_bytes")
    return s.value, c.value


def saved_layout(dims):
    L = FgsSavedLayout()
    check(load().fgs_saved_layout(ctypes.byref(dims), ctypes.byref(L)), "fgs_saved_layout")
    return L


def stage_timing_enable(on=True, stages=None):
    """on=True: every stage; stages=[names]: only those (each event pair costs a few microseconds of stream time)."""
    mask = 1 if on else 0
    if on and stages is not None:
        mask = 0
        for name in stages:
            mask |= 1 << (STAGES.index(name) + 1)
    check(load().fgs_stage_timing_enable(mask), "fgs_stage_timing_enable")


def stage_timing_read():
    """-> {stage: (total_ms, launches)} accumulated since the previous read."""
    n = len(STAGES)
    ms = (ctypes.c_float * n)()
    cnt = (ctypes.c_int32 * n)()
    check(load().fgs_stage_timing_read(ms, cnt), "fgs_stage_timing_read")
    return {STAGES[i]: (float(ms[i]), int(cnt[i])) for i in range(n)}
