"""ctypes front-end of the CPU ORACLE (test infrastructure only -- see fgs_oracle.c).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import
this module.  The product package (fresnel_amd) never does.

Reference followed: scripts/models/differentiable_renderer.py (TileBasedRenderer,
DR:412-686; compute_2d_covariance DR:123-195).
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libfgs_oracle.so")
_SO64 = os.path.join(_HERE, "_build", "libfgs_oracle_f64.so")
# Precision of the restatement in use: float32 (the oracle; canonical fp32) or -- inside `with fp64():` -- the sed-widened fp64
# REFEREE build (oracle/Makefile): what the reference computes with torch's default dtype switched to float64.
_REAL = np.float32
_CREAL = ctypes.c_float


class OrCamera(ctypes.Structure):
    _fields_ = [("view", ctypes.c_float * 16), ("fx", ctypes.c_float), ("fy", ctypes.c_float),
                ("cx", ctypes.c_float), ("cy", ctypes.c_float), ("width", ctypes.c_int32),
                ("height", ctypes.c_int32), ("near_", ctypes.c_float), ("far_", ctypes.c_float)]


class OrCamera64(ctypes.Structure):
    _fields_ = [("view", ctypes.c_double * 16), ("fx", ctypes.c_double), ("fy", ctypes.c_double),
                ("cx", ctypes.c_double), ("cy", ctypes.c_double), ("width", ctypes.c_int32),
                ("height", ctypes.c_int32), ("near_", ctypes.c_double), ("far_", ctypes.c_double)]


def build(force=False):
    src = os.path.join(_HERE, "fgs_oracle.c")
    if force or any(not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src) for so in (_SO, _SO64)):
        subprocess.check_call(["make", "-C", _HERE, "-s"])
    return _SO


_lib = None
_lib64 = None


def _load(path):
    l = ctypes.CDLL(path)
    l.fgs_or_count_pairs.restype = ctypes.c_int64
    l.fgs_or_tile_lists.restype = ctypes.c_int64
    l.fgs_or_render_fwd_bwd.restype = ctypes.c_int64
    return l


def lib():
    global _lib, _lib64
    if _REAL is np.float64:
        if _lib64 is None:
            build()
            _lib64 = _load(_SO64)
        return _lib64
    if _lib is None:
        _lib = _load(build())
    return _lib


class fp64:
    """`with fgs_oracle.fp64(): r = render(...); g = render_backward(r, gI, gD)` -- the same calls on the fp64 referee build
    (arrays come back as float64; cameras made by make_camera carry their unrounded doubles; render() keeps the fp32 run's
    integer stages).  This is a TRUE fp64 evaluation -- an independent numpy fp64 loop agrees with it to 3e-13.  The reference's OWN
    run under torch's default dtype float64 (the `f64_*` arrays of the G14 / K fixtures) is NOT: its pixel grid is a hard-coded
    float32 arange (DR:603-607) and `local_x - mean[0]`, `a * dx * dx`, `gauss_val * opacity` combine it with 0-dim float64
    tensors, which do not promote a dimensioned float32 tensor -- the per-pixel Gaussian is evaluated in fp32 there, with the
    mean and the inverse covariance rounded to fp32.  The two differ by what that costs: 8.5e-6 (G14 30:1), 9e-5 (100:1),
    5.8e-4 (500:1) on the image, 1e-6 on well-conditioned scenes (found in round 5 while pinning this build against the fixtures)."""

    def __enter__(self):
        global _REAL, _CREAL
        self._old = (_REAL, _CREAL)
        _REAL, _CREAL = np.float64, ctypes.c_double

    def __exit__(self, *a):
        global _REAL, _CREAL
        _REAL, _CREAL = self._old


def _camref(cam):
    return ctypes.byref(cam._f64 if _REAL is np.float64 else cam)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _f32(a):
    """contiguous array in the precision in use (float32 unless inside `with fp64()`)."""
    return np.ascontiguousarray(a, dtype=_REAL)


def make_camera(view, fx, fy, cx, cy, width, height, near=0.01, far=100.0):
    cam = OrCamera()
    v = _f32(view).reshape(16)
    for i in range(16):
        cam.view[i] = float(v[i])
    cam.fx, cam.fy, cam.cx, cam.cy = float(fx), float(fy), float(cx), float(cy)
    cam.width, cam.height = int(width), int(height)
    cam.near_, cam.far_ = float(near), float(far)
    c64 = OrCamera64()
    v64 = np.asarray(view, dtype=np.float64).reshape(16)
    for i in range(16):
        c64.view[i] = float(v64[i])
    c64.fx, c64.fy, c64.cx, c64.cy = float(fx), float(fy), float(cx), float(cy)
    c64.width, c64.height = int(width), int(height)
    c64.near_, c64.far_ = float(near), float(far)
    cam._f64 = c64
    return cam


def project(pos, scale, quat, cam, max_radius=64.0):
    pos, scale, quat = _f32(pos), _f32(scale), _f32(quat)
    N = pos.shape[0]
    out = dict(cov2d=np.zeros((N, 4), _REAL), mean2d=np.zeros((N, 2), _REAL),
               depth=np.zeros(N, _REAL), radius=np.zeros(N, _REAL),
               visible=np.zeros(N, np.uint8), bbox=np.zeros((N, 4), np.int32),
               conic=np.zeros((N, 3), _REAL))
    lib().fgs_or_project(ctypes.c_int32(N), _p(pos), _p(scale), _p(quat), _camref(cam),
                         _CREAL(max_radius), _p(out["cov2d"]), _p(out["mean2d"]),
                         _p(out["depth"]), _p(out["radius"]), _p(out["visible"]), _p(out["bbox"]),
                         _p(out["conic"]))
    return out


def depth_order(depth, visible):
    N = depth.shape[0]
    order = np.zeros(N, np.int32)
    vs = np.zeros(N, np.int32)
    V = ctypes.c_int32(0)
    lib().fgs_or_depth_order(ctypes.c_int32(N), _p(_f32(depth)), _p(np.ascontiguousarray(visible, np.uint8)),
                             _p(order), _p(vs), ctypes.byref(V))
    return order, vs[:V.value].copy()


def count_pairs(vis_sorted, bbox):
    return int(lib().fgs_or_count_pairs(ctypes.c_int32(len(vis_sorted)),
                                        _p(np.ascontiguousarray(vis_sorted, np.int32)),
                                        _p(np.ascontiguousarray(bbox, np.int32))))


def tile_lists(vis_sorted, bbox, W, H, ts=16, tile_w=None):
    """Per-tile lists in depth order; tiles are ts x ts, or tile_w x ts when tile_w is given."""
    vs = np.ascontiguousarray(vis_sorted, np.int32)
    bb = np.ascontiguousarray(bbox, np.int32)
    tw = ts if tile_w is None else int(tile_w)
    T = ((W + tw - 1) // tw) * ((H + ts - 1) // ts)
    ts = tw | (ts << 16)
    ranges = np.zeros(T + 1, np.int64)
    D = lib().fgs_or_tile_lists(ctypes.c_int32(len(vs)), _p(vs), _p(bb), ctypes.c_int32(W),
                                ctypes.c_int32(H), ctypes.c_int32(ts), _p(ranges), None)
    ids = np.zeros(max(int(D), 1), np.int32)
    lib().fgs_or_tile_lists(ctypes.c_int32(len(vs)), _p(vs), _p(bb), ctypes.c_int32(W),
                            ctypes.c_int32(H), ctypes.c_int32(ts), _p(ranges), _p(ids))
    return ranges, ids[:int(D)]


class Rendered:
    """Everything the oracle's forward produced (kept for its backward)."""


def render(pos, scale, quat, color, opacity, cam, bg=(0.0, 0.0, 0.0), max_radius=64.0,
           phases=None, phase_amp=0.25, keep_pairs=True, proj=None):
    """Oracle forward for ONE image: returns Rendered with .image (3,H,W), .depth (H,W).
    proj: composite THIS projection (a dict as project() returns, e.g. an earlier run's with a bbox moved) instead of projecting
    the Gaussians; the depth order is taken from its depths and visibility.  Default: project here, as always."""
    global _REAL, _CREAL
    r = Rendered()
    r.pos, r.scale, r.quat = _f32(pos), _f32(scale), _f32(quat)
    r.color, r.opacity = _f32(color), _f32(opacity)
    r.cam, r.bg, r.max_radius = cam, _f32(bg), float(max_radius)
    r.phases = None if phases is None else _f32(phases)
    r.phase_amp = float(phase_amp)
    W, H = cam.width, cam.height
    r.proj = project(r.pos, r.scale, r.quat, cam, max_radius) if proj is None else {
        k: np.ascontiguousarray(v, dtype=v.dtype if k in ("visible", "bbox") else _REAL) for k, v in proj.items()}
    if proj is None and _REAL is np.float64:
        # the fp64 REFEREE keeps the fp32 run's INTEGER stages (visibility, bboxes, depth order) -- like the reference-derived fp64 runs
        # of the K1 / K2 fixtures (tests/golden/make_goldens.py phase_restatement) -- so that it differs from the fp32 run by arithmetic
        # precision alone, not by a bbox edge that lands on the other side of a pixel
        keep = (_REAL, _CREAL)
        _REAL, _CREAL = np.float32, ctypes.c_float
        try:
            p32 = project(r.pos.astype(np.float32), r.scale.astype(np.float32), r.quat.astype(np.float32), cam, max_radius)
            o32, v32 = depth_order(p32["depth"], p32["visible"])
        finally:
            _REAL, _CREAL = keep
        r.proj["visible"], r.proj["bbox"] = p32["visible"], p32["bbox"]
        r.order, r.vis_sorted = o32, v32
    else:
        r.order, r.vis_sorted = depth_order(r.proj["depth"], r.proj["visible"])
    r.P = count_pairs(r.vis_sorted, r.proj["bbox"])
    r.image = np.zeros((3, H, W), _REAL)
    r.depth = np.zeros((H, W), _REAL)
    r.state = np.zeros((5, H, W), _REAL)
    r.pair_T = np.zeros(max(r.P, 1), _REAL) if keep_pairs else None
    r.pair_phi = np.zeros(max(r.P, 1), _REAL) if (keep_pairs and phases is not None) else None
    lib().fgs_or_composite_fwd(
        ctypes.c_int32(len(r.vis_sorted)), _p(r.vis_sorted), _p(r.proj["mean2d"]), _p(r.proj["conic"]),
        _p(r.color), _p(r.opacity), _p(r.proj["depth"]), _p(r.proj["bbox"]), _p(r.phases),
        _CREAL(r.phase_amp), ctypes.c_int32(W), ctypes.c_int32(H), _p(r.bg), _p(r.image),
        _p(r.depth), _p(r.state), _p(r.pair_T), _p(r.pair_phi))
    return r


def render_backward(r, gI, gD):
    """Oracle backward for the image produced by render(); returns dict of grads."""
    gI, gD = _f32(gI), _f32(gD)
    N = r.pos.shape[0]
    W, H = r.cam.width, r.cam.height
    g_mean = np.zeros((N, 2), _REAL)
    g_conic = np.zeros((N, 3), _REAL)
    g_color = np.zeros((N, 3), _REAL)
    g_op = np.zeros(N, _REAL)
    g_dep = np.zeros(N, _REAL)
    g_ph = np.zeros(N, _REAL) if r.phases is not None else None
    lib().fgs_or_composite_bwd(
        ctypes.c_int32(len(r.vis_sorted)), _p(r.vis_sorted), _p(r.proj["mean2d"]), _p(r.proj["conic"]),
        _p(r.color), _p(r.opacity), _p(r.proj["depth"]), _p(r.proj["bbox"]), _p(r.phases),
        _CREAL(r.phase_amp), ctypes.c_int32(W), ctypes.c_int32(H), _p(r.bg), _p(r.state),
        _p(r.pair_T), _p(r.pair_phi), _p(gI), _p(gD), _p(g_mean), _p(g_conic), _p(g_color), _p(g_op),
        _p(g_dep), _p(g_ph))
    g_pos = np.zeros((N, 3), _REAL)
    g_scale = np.zeros((N, 3), _REAL)
    g_quat = np.zeros((N, 4), _REAL)
    lib().fgs_or_project_bwd(ctypes.c_int32(N), _p(r.pos), _p(r.scale), _p(r.quat), _camref(r.cam),
                             _p(r.proj["visible"]), _p(g_mean), _p(g_conic), _p(g_dep), _p(g_pos),
                             _p(g_scale), _p(g_quat))
    out = dict(positions=g_pos, scales=g_scale, rotations=g_quat, colors=g_color, opacities=g_op,
               mean2d=g_mean, conic=g_conic, depth=g_dep)
    if g_ph is not None:
        out["phases"] = g_ph
    return out


def render_fwd_bwd_timed(pos, scale, quat, color, opacity, cam, gI, gD, bg=(0.0, 0.0, 0.0),
                         max_radius=64.0):
    """One fused forward+backward inside C (bench.py cpu_baseline leg). Returns pairs P."""
    pos, scale, quat, color, opacity = map(_f32, (pos, scale, quat, color, opacity))
    N = pos.shape[0]
    W, H = cam.width, cam.height
    img = np.zeros((3, H, W), _REAL)
    dep = np.zeros((H, W), _REAL)
    gp, gs, gq = np.zeros((N, 3), _REAL), np.zeros((N, 3), _REAL), np.zeros((N, 4), _REAL)
    gc, go = np.zeros((N, 3), _REAL), np.zeros(N, _REAL)
    P = lib().fgs_or_render_fwd_bwd(ctypes.c_int32(N), _p(pos), _p(scale), _p(quat), _p(color), _p(opacity),
                                    _camref(cam), _CREAL(max_radius), _p(_f32(bg)), _p(_f32(gI)),
                                    _p(_f32(gD)), _p(img), _p(dep), _p(gp), _p(gs), _p(gq), _p(gc), _p(go))
    return int(P), img, dep
