"""ctypes binding of libfgs_hip.so (include/fgs.h).  No torch types cross this boundary:
only raw device pointers, sizes and the HIP stream handle.

The product path FAILS LOUDLY when the HIP library is missing -- there is no CPU fallback.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FGS_LIB", os.path.join(_HERE, "_lib", "libfgs_hip.so"))  # FGS_LIB: A/B builds

FGS_CAMERA_FLOATS = 24
FGS_TILE = 16

# Every symbol include/fgs.h declares, as the header writes it: return type, then the parameters in order.  A comma-separated group
# is a kind and the names that share it, as in C's `int32_t height, width`; `stream` is the trailing `void *stream`.  Kinds: pointer to
# a named struct (`FgsDims*`), `size_t*`, any other pointer (`ptr`), the header's scalar types; `str` is `const char *`.  load()
# makes argtypes and restype from this table, tests/test_call_layer.py holds it against the header name by name.
_PROTOTYPES = """
int fgs_workspace_bytes(FgsDims* dims, size_t* saved_bytes scratch_bytes)
int fgs_saved_layout(FgsDims* dims, FgsSavedLayout* layout)
int fgs_forward(FgsDims* dims, ptr cameras pos scale quat color opacity phase out_rgb out_depth saved scratch, stream)
int fgs_backward(FgsDims* dims, ptr cameras pos scale quat color opacity phase saved scratch g_rgb g_depth g_pos g_scale g_quat g_color
                 g_opacity g_phase, stream)
int fgs_count_pairs(FgsDims* dims, ptr saved out_pairs, stream)
int fgs_row_sum(FgsDims* dims, ptr saved grad_rows zero_from row_sums, stream)
int fgs_asm_workspace_bytes(FgsAsmDims* dims, size_t* saved_bytes scratch_bytes)
int fgs_asm_forward(FgsAsmDims* dims, ptr cameras pos scale quat color opacity phase wavelengths out_rgb saved scratch, stream)
int fgs_asm_backward(FgsAsmDims* dims, ptr cameras pos scale quat color opacity phase wavelengths saved scratch g_rgb g_pos g_scale
                     g_quat g_color g_opacity g_phase g_wavelengths, stream)
int fgs_wave_workspace_bytes(FgsWaveDims* dims, size_t* saved_bytes scratch_bytes)
int fgs_wave_forward(FgsWaveDims* dims, ptr cameras pos scale quat color opacity phase out_rgb out_depth saved scratch, stream)
int fgs_wave_backward(FgsWaveDims* dims, ptr cameras pos scale quat color opacity phase saved scratch g_rgb g_depth g_pos g_scale
                      g_quat g_color g_opacity g_phase, stream)
int fgs_fourier_workspace_bytes(FgsFourierDims* dims, size_t* saved_bytes scratch_bytes)
int fgs_fourier_forward(FgsFourierDims* dims, ptr cameras pos scale quat color opacity out_rgb saved scratch, stream)
int fgs_fourier_backward(FgsFourierDims* dims, ptr cameras pos scale quat color opacity saved scratch g_rgb g_pos g_scale g_quat
                         g_color g_opacity, stream)
int fgs_asm_propagate_workspace_bytes(int32_t height width channels, size_t* scratch_bytes)
int fgs_asm_propagate_forward(int32_t height width channels, double pixel_pitch, int32_t band_limit, ptr field z wavelengths out
                              spectrum scratch, stream)
int fgs_asm_propagate_backward(int32_t height width channels, double pixel_pitch, int32_t band_limit, ptr spectrum z wavelengths
                               g_out g_field g_z g_wavelengths scratch, stream)
int fgs_spectral_workspace_bytes(FgsSpectralDims* dims, size_t* saved_bytes scratch_bytes)
int fgs_spectral_loss_forward(FgsSpectralDims* dims, ptr rendered target depth wavelength loss saved scratch, stream)
int fgs_spectral_loss_backward(FgsSpectralDims* dims, ptr rendered target depth wavelength saved scratch g_loss g_rendered g_target
                               g_depth g_wavelength, stream)
int fgs_helmholtz_loss_forward(int32_t images height width, float wavelength pixel_spacing, ptr field loss residual scratch, stream)
int fgs_helmholtz_loss_backward(int32_t images height width, float wavelength pixel_spacing, ptr residual g_loss g_field, stream)
size_t fgs_reduction_scratch_bytes()
int fgs_ssim_workspace_bytes(FgsSsimDims* dims, size_t* saved_bytes scratch_bytes)
int fgs_ssim_forward(FgsSsimDims* dims, ptr x y out saved scratch, stream)
int fgs_ssim_backward(FgsSsimDims* dims, ptr x y saved g_out g_x g_y scratch, stream)
int fgs_pixel_loss_workspace_bytes(FgsPixelLossDims* dims, size_t* stats_bytes scratch_bytes)
int fgs_pixel_loss_stage1(FgsPixelLossDims* dims, ptr rendered target rendered_depth target_depth density out stats scratch, stream)
int fgs_pixel_loss_stage2(FgsPixelLossDims* dims, ptr rendered_depth target_depth stats scratch, stream)
int fgs_pixel_loss_stage3(FgsPixelLossDims* dims, ptr rendered_depth target_depth out stats scratch, stream)
int fgs_pixel_loss_forward(FgsPixelLossDims* dims, ptr rendered target rendered_depth target_depth density out stats scratch, stream)
int fgs_pixel_loss_backward(FgsPixelLossDims* dims, ptr rendered target rendered_depth target_depth density stats g_rgb g_boundary
                            g_depth g_rendered g_rendered_depth, stream)
int fgs_head_workspace_bytes(FgsHeadDims* dims, size_t* scratch_bytes)
int fgs_head_forward(FgsHeadDims* dims, ptr raw base_xy base_z pose opacity_mod edge positions scales rotations colors opacities
                     phases, stream)
int fgs_head_backward(FgsHeadDims* dims, ptr raw pose opacity_mod edge g_positions g_scales g_rotations g_colors g_opacities g_phases
                      g_raw g_base_z g_edge g_opacity_mod scratch, stream)
int fgs_nca_workspace_bytes(FgsNcaDims* dims, size_t* scratch_bytes)
int fgs_nca_perceive_forward(FgsNcaDims* dims, ptr state perception neighbors, stream)
int fgs_nca_perceive_backward(FgsNcaDims* dims, ptr neighbors g_perception g_state, stream)
int fgs_nca_update_forward(FgsNcaDims* dims, ptr state delta step_size uniform, float update_prob, ptr new_state, stream)
int fgs_nca_update_backward(FgsNcaDims* dims, ptr delta step_size uniform, float update_prob, ptr g_new_state g_delta g_step_size
                            scratch, stream)
int fgs_saag_workspace_bytes(FgsSaagDims* dims, size_t* scratch_bytes)
int fgs_saag_inputs_forward(FgsSaagDims* dims, ptr features positions scales rotations colors opacities mlp_inputs, stream)
int fgs_saag_refine_forward(FgsSaagDims* dims, ptr raw positions scales rotations colors opacities gains o_positions o_scales
                            o_rotations o_colors o_opacities pos_delta scale_delta color_delta opacity_delta, stream)
int fgs_saag_refine_backward(FgsSaagDims* dims, ptr raw scales rotations colors opacities gains g_positions g_scales g_rotations
                             g_colors g_opacities g_pos_delta g_scale_delta g_color_delta g_opacity_delta g_raw g_gains scratch, stream)
int fgs_physics_workspace_bytes(FgsPhysicsDims* dims, size_t* scratch_bytes)
int fgs_physics_forward(FgsPhysicsDims* dims, ptr raw base_xy base_z wavelength_raw positions scales rotations colors opacities phases
                        range scratch, stream)
int fgs_physics_backward(FgsPhysicsDims* dims, ptr raw base_z wavelength_raw range g_positions g_scales g_rotations g_colors
                         g_opacities g_phases g_raw g_base_z g_wavelength_raw scratch, stream)
int fgs_surface_workspace_bytes(FgsSurfaceDims* dims, FgsSurfaceParams* params, size_t* scratch_bytes)
int fgs_surface_count(FgsSurfaceDims* dims, FgsSurfaceParams* params, ptr depth scratch offsets, stream)
int fgs_surface_emit(FgsSurfaceDims* dims, FgsSurfaceParams* params, ptr depth color scratch offsets o_positions o_scales o_rotations
                     o_colors o_opacities, int64_t capacity, stream)
int fgs_surface_emit_guided(FgsSurfaceDims* dims, FgsSurfaceParams* params, ptr depth color scratch offsets mods, int32_t mods_h mods_w,
                            ptr o_positions o_scales o_rotations o_colors o_opacities point_rows, int64_t capacity, stream)
int fgs_surface_guided_backward_bytes(FgsSurfaceDims* dims, FgsSurfaceParams* params, int32_t mods_h mods_w, size_t* bytes)
int fgs_surface_guided_backward(FgsSurfaceDims* dims, FgsSurfaceParams* params, ptr depth scratch offsets mods, int32_t mods_h mods_w,
                                ptr point_rows g_positions g_scales g_rotations g_opacities g_mods bwd_scratch, stream)
int fgs_match_workspace_bytes(FgsMatchDims* dims, size_t* saved_bytes scratch_bytes)
int fgs_match_forward(FgsMatchDims* dims, ptr pred target pred_keep target_keep terms counts saved scratch, stream)
int fgs_match_backward(FgsMatchDims* dims, ptr pred target saved g_total g_pred scratch, stream)
int fgs_slat_workspace_bytes(int32_t batch voxels per_voxel, size_t* scratch_bytes)
int fgs_slat_head_forward(int32_t batch voxels per_voxel, ptr raw coords gains keep gaussians counts scratch, stream)
int fgs_slat_head_backward(int32_t batch voxels per_voxel, ptr raw coords gains g_gaussians g_raw g_gains scratch, stream)
int fgs_attn_workspace_bytes(int32_t batch queries keys heads head_dim, size_t* saved_bytes scratch_bytes)
int fgs_attn_forward(int32_t batch queries keys heads head_dim, float scale dropout_p, ptr q kv row_keep seed out saved, stream)
int fgs_attn_backward(int32_t batch queries keys heads head_dim, float scale dropout_p, ptr q kv row_keep seed out saved g_out g_q
                      g_kv scratch, stream)
int fgs_attn_half_workspace_bytes(int32_t batch queries keys heads head_dim, size_t* saved_bytes scratch_bytes)
int fgs_attn_half_forward(int32_t dtype batch queries keys heads head_dim, float scale dropout_p, ptr q kv row_keep seed out saved,
                          stream)
int fgs_attn_half_backward(int32_t dtype batch queries keys heads head_dim, float scale dropout_p, ptr q kv row_keep seed out saved
                           g_out g_q g_kv scratch, stream)
int fgs_wave_attn_workspace_bytes(int32_t batch grid_h grid_w heads head_dim, size_t* saved_bytes scratch_bytes)
int fgs_wave_attn_forward(int32_t batch grid_h grid_w heads head_dim, float scale, ptr qkv wavelength out saved, stream)
int fgs_wave_attn_backward(int32_t batch grid_h grid_w heads head_dim, float scale, ptr qkv wavelength out saved g_out g_qkv
                           g_wavelength scratch, stream)
int fgs_gn_silu_workspace_bytes(int32_t batch channels hw groups, size_t* saved_bytes scratch_bytes)
int fgs_gn_silu_forward(int32_t batch channels hw groups act, float eps, ptr x channel_bias weight bias out saved scratch, stream)
int fgs_gn_silu_backward(int32_t batch channels hw groups act, float eps, ptr x channel_bias weight bias saved g_out g_x g_channel_bias
                         g_weight g_bias scratch, stream)
int fgs_cvs_loss_workspace_bytes(int32_t images channels height width flags, size_t* saved_bytes scratch_bytes)
int fgs_cvs_quality_mask(int32_t images height width, float threshold sharpness, ptr depth mask, stream)
int fgs_cvs_loss_forward(int32_t images channels height width flags, float threshold sharpness, ptr pred target depth ema out saved
                         scratch, stream)
int fgs_cvs_loss_backward(int32_t images channels height width flags, float threshold sharpness, ptr pred target depth ema saved
                          g_terms g_pred, stream)
int fgs_cvs_euler_step(int32_t images channels hw steps, ptr sqrt_alphas_cumprod timestep x0_pred noisy x_prev t_prev, stream)
int fgs_gather_forward(int32_t batch n_in n_out phase_channels, ptr indices pos scale quat color opacity phase o_pos o_scale o_quat
                       o_color o_opacity o_phase, stream)
int fgs_gather_backward(int32_t batch n_in n_out phase_channels, ptr indices g_o_pos g_o_scale g_o_quat g_o_color g_o_opacity
                        g_o_phase g_pos g_scale g_quat g_color g_opacity g_phase, stream)
int fgs_stage_timing_enable(int enable)
int fgs_stage_timing_read(ptr ms count)
str fgs_last_error()
str fgs_version()
"""


def _parse_prototypes(text):
    """-> {symbol: (return kind, ((kind, name), ...))}, in the order written."""
    table = {}
    for ret, name, params in re.findall(r"(\S+) (fgs_\w+)\(([^)]*)\)", text):
        flat = []
        for kind, *names in (group.split() for group in params.split(",") if group.strip()):
            flat += [(kind, n) for n in names or [kind]]  # a bare `stream` is its own name
        table[name] = (ret, tuple(flat))
    return table


SIGNATURES = _parse_prototypes(_PROTOTYPES)
EXPORTED_SYMBOLS = list(SIGNATURES)  # (checked against the header by tests/test_abi.py)

STAGES = ["project", "depth_sort", "dup_emit", "tile_sort", "tile_ranges", "composite_fwd",
          "composite_bwd", "project_bwd", "splat_fwd", "field_fwd", "field_bwd", "splat_bwd"]


FWD_EXIT_OFF, FWD_EXIT_ON = 0x100, 0x200  # include/fgs.h: flags of FgsDims.fwd_variant
BWD_ZERO_OFF, BWD_ZERO_ON = 0x400, 0x800  # include/fgs.h: flags of FgsDims.fwd_variant
BWD_TAIL_OFF, BWD_TAIL_ON = 0x2000, 0x4000  # include/fgs.h: flags of FgsDims.fwd_variant
BWD_SUB_OFF, BWD_SUB_ON = 0x8000, 0x10000  # include/fgs.h: flags of FgsDims.fwd_variant
FWD_PREWALK_OFF, FWD_PREWALK_ON = 0x40000, 0x80000  # include/fgs.h: flags of FgsDims.fwd_variant


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
                ("fwd_close", ctypes.c_size_t), ("rank_of", ctypes.c_size_t)]


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


# the fused cross-attention's seams (include/fgs.h; tests/test_call_layer.py holds every macro restated here against the header):
# queries per workgroup, keys per LDS tile, keys per workgroup of the key-block backward, largest head dimension
FGS_ATTN_QUERY_BLOCK, FGS_ATTN_KEY_TILE, FGS_ATTN_KEY_BLOCK, FGS_ATTN_MAX_HEAD_DIM = 128, 32, 128, 128
# its 16-bit form (csrc/fgs_attn_half.hip): the `dtype` argument's two values, keys per LDS tile
FGS_ATTN_F16, FGS_ATTN_BF16, FGS_ATTN_HALF_KEY_TILE = 1, 2, 32
FGS_WAVE_ATTN_MAX_TOKENS = 4096
FGS_GN_SEGMENT = 4096  # floats of one channel row per wave of the fused GroupNorm-SiLU: longer rows are cut there (include/fgs.h)

# the fused CVS loss (include/fgs.h): flags of its terms; threads per block and the largest grid of its streaming kernels
FGS_CVS_QUALITY, FGS_CVS_CONS_L1, FGS_CVS_CONS_MSE, FGS_CVS_BOUNDARY, FGS_CVS_GRADIENT = 1, 2, 4, 8, 16
FGS_CVS_THREADS, FGS_CVS_MAX_GRID = 256, 2048


class FgsError(RuntimeError):
    pass


_lib = None

_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t, "str": ctypes.c_char_p,
            "ptr": ctypes.c_void_p, "stream": ctypes.c_void_p}


def _ctype(kind):
    """The ctypes type of a kind of the table: `FgsDims*` and `size_t*` are typed pointers, every other pointer a c_void_p."""
    if kind.endswith("*"):
        return ctypes.POINTER(_SCALARS.get(kind[:-1]) or globals()[kind[:-1]])
    return _SCALARS[kind]


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
    for name, (ret, params) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ctype(ret), [_ctype(kind) for kind, _ in params]
    if b"EXPERIMENT" in lib.fgs_version():  # an A/B build selected through FGS_LIB: say so, once, where nobody can miss it
        import sys
        sys.stderr.write(f"fresnel_amd: loaded {LIB_PATH}: {lib.fgs_version().decode()}\n")
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
    `fwd_exit`: 0 | 1 | -1 = the exiting depth-split forward automatic | on | off -- the FGS_FWD_EXIT_ON / _OFF flag of FgsDims.fwd_variant,
    `bwd_zero`: 0 | 1 | -1 = the blend backward's zero rows for dead units with S == 0 automatic | on | off -- the FGS_BWD_ZERO_ON / _OFF flag of FgsDims.fwd_variant.
    `bwd_tail`: 0 | 1 | -1 = the blend backward's one verdict per closed tile automatic (on where the plan has what it needs) | the same | off
    -- the FGS_BWD_TAIL_ON / _OFF flag of FgsDims.fwd_variant.
    `bwd_sub`: 0 | 1 | -1 = the blend backward's zero sub-tiles of general units automatic (on wherever bwd_zero is) | on | off
    -- the FGS_BWD_SUB_ON / _OFF flag of FgsDims.fwd_variant.
    `fwd_prewalk`: 0 | 1 | -1 = the exiting forward's head launch walks the later parts of short lists automatic (off: it measured slower) |
    on (where the exiting forward runs with more than one part) | off -- the FGS_FWD_PREWALK_ON / _OFF flag of FgsDims.fwd_variant.
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
    bwd_zero = int(tuning.pop("bwd_zero", 0))
    bwd_tail = int(tuning.pop("bwd_tail", 0))
    bwd_sub = int(tuning.pop("bwd_sub", 0))
    fwd_prewalk = int(tuning.pop("fwd_prewalk", 0))
    for k, v in tuning.items():
        if k not in ("seg_len", "fwd_variant", "bin_mode", "tile_w", "sort_mode"):
            raise FgsError(f"unknown tuning field {k!r}")
        setattr(d, k, int(v))
    if fwd_exit not in (0, 1, -1) or (fwd_exit and d.fwd_variant < 0):
        raise FgsError(f"fwd_exit must be 0, 1 or -1, and 0 with the row-split forward (fwd_variant < 0), got {fwd_exit!r}")
    if bwd_zero not in (0, 1, -1) or (bwd_zero and d.fwd_variant < 0):
        raise FgsError(f"bwd_zero must be 0, 1 or -1, and 0 with the row-split forward (fwd_variant < 0), got {bwd_zero!r}")
    if bwd_tail not in (0, 1, -1) or (bwd_tail and d.fwd_variant < 0):
        raise FgsError(f"bwd_tail must be 0, 1 or -1, and 0 with the row-split forward (fwd_variant < 0), got {bwd_tail!r}")
    if bwd_sub not in (0, 1, -1) or (bwd_sub and d.fwd_variant < 0):
        raise FgsError(f"bwd_sub must be 0, 1 or -1, and 0 with the row-split forward (fwd_variant < 0), got {bwd_sub!r}")
    if fwd_prewalk not in (0, 1, -1) or (fwd_prewalk and d.fwd_variant < 0):
        raise FgsError(f"fwd_prewalk must be 0, 1 or -1, and 0 with the row-split forward (fwd_variant < 0), got {fwd_prewalk!r}")
    d.fwd_variant |= ({0: 0, 1: FWD_EXIT_ON, -1: FWD_EXIT_OFF}[fwd_exit] | {0: 0, 1: BWD_ZERO_ON, -1: BWD_ZERO_OFF}[bwd_zero]
                      | {0: 0, 1: BWD_TAIL_ON, -1: BWD_TAIL_OFF}[bwd_tail] | {0: 0, 1: BWD_SUB_ON, -1: BWD_SUB_OFF}[bwd_sub]
                      | {0: 0, 1: FWD_PREWALK_ON, -1: FWD_PREWALK_OFF}[fwd_prewalk])
    d.dup_capacity = int(dup_capacity)
    return d


_SIZE_OUTS = {name: sum(kind == "size_t*" for kind, _ in params) for name, (_, params) in SIGNATURES.items()}


def sizes(name, *args):
    """Call a `*_workspace_bytes` / `*_backward_bytes` entry point: `args` are its inputs (structures go by reference, scalars as
    they are), the trailing `size_t *` outputs are the table's.  -> the one size as an int, or the two as a tuple of ints.
    The hipFFT-backed queries (fgs_asm_, fgs_asm_propagate_, fgs_spectral_workspace_bytes) build and cache the current device's
    plan and return ITS work size: their callers make the tensors' device current first (`_hip.on_device`)."""
    n = _SIZE_OUTS[name]
    out = [ctypes.c_size_t(0) for _ in range(n)]
    check(getattr(load(), name)(*[ctypes.byref(a) if isinstance(a, ctypes.Structure) else a for a in args],
                                *[ctypes.byref(o) for o in out]), name)
    return out[0].value if n == 1 else tuple(o.value for o in out)


def workspace_bytes(dims):
    return sizes("fgs_workspace_bytes", dims)


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
