"""Checker of the SAAG surface-cloud generator (fgs_surface_count / fgs_surface_emit, fresnel_amd.surface): a restatement of the
reference's C++ in NumPy fp32, one image at a time, in the C++'s operation order.

Cited as PC = src/core/pointcloud.cpp, IM = src/core/image.cpp, VW = src/viewer/viewer.cpp of the reference.  The reference
itself cannot be run where this project is developed (it needs GLM, Vulkan and a configure-time fetch), so no fixture comes from
it: what pins this file is tests/test_surface_checker.py, whose expected values are worked out by hand.

Every statement works on ALL points of the image at once (arrays of fp32, one element per point) instead of looping over the
points: an element-wise NumPy fp32 operation is the same correctly rounded IEEE operation as the scalar one, so the values are
those of a point loop, and a 96 x 96 frame takes a second instead of a minute.  Branches become masks (np.where); the emit
ORDER (PC:206-428: per point base, back, walls, wraps, fills) is restored when the rows are gathered.  Operands are np.float32
throughout -- no Python float enters an expression, whatever the NumPy version's promotion rules.

GLM semantics restated here -- GLM 1.0.1's definitions as commonly documented, NOT read from its source (it is not available):
    dot(a, b)       a.x b.x + a.y b.y + a.z b.z, summed left to right
    length(v)       sqrt(dot(v, v))
    normalize(v)    v * (1 / sqrt(dot(v, v)))
    v / s           every component divided by s
    cross(x, y)     (x.y y.z - y.y x.z,  x.z y.x - y.z x.x,  x.x y.y - y.x x.y)
    angleAxis(a, v) (cos(a / 2), v sin(a / 2))
    slerp(x, y, t)  c = dot(x, y); y, c negated if c < 0; c > 1 - FLT_EPSILON: component-wise mix; else
                    (sin((1 - t) th) x + sin(t th) y) / sin(th), th = acos(c)
    mix(a, b, t)    a (1 - t) + b t
std::min / std::max / std::clamp compare with <, which differs from fmin / fmax for NaN only; the range, the bounds and
max_gradient are DEFINED to ignore NaN (include/fgs.h), np.fmin / np.fmax here.

`mutate` switches exactly one rule off (tests/test_surface_checker.py proves that each is pinned):
    "edge_clamp"           the Sobel neighbourhood clamps to the frame instead of reading zero outside it
    "non_strict"           the three gradient thresholds compare with >= instead of >
    "skip_before_maxgrad"  max_gradient runs over the points that pass the confidence skip only
    "center_once"          the cloud is centred once (normalize() without its own center())
"""
import numpy as np

F = np.float32
ZERO, HALF, ONE, TWO = F(0.0), F(0.5), F(1.0), F(2.0)
FLT_EPSILON = np.finfo(np.float32).eps
PI = F(3.14159265358979323846)

KEPT, BASE, BACK, WALLS, WRAPS, FILLS = 1, 2, 4, 8, 16, 32            # per-point flag bits (include/fgs.h)
K_BASE, K_BACK, K_WALL, K_WRAP, K_FILL = 0, 1, 2, 3, 4                # row kinds
MUTATIONS = ("edge_clamp", "non_strict", "skip_before_maxgrad", "center_once")

# the viewer's settings (viewer.hpp:139-178) over the structs' own defaults (pointcloud.hpp:18-80)
DEFAULTS = dict(
    fx=0.0, fy=0.0, cx=0.0, cy=0.0, depth_scale=2.5, subsample=1, opacity=0.9, normalize_extent=3.0,
    base_size=0.008, aspect_ratio=5.0, edge_threshold=0.15, edge_shrink=0.3, min_confidence=0.1, gradient_scale=50.0,
    normal_strength=1.0,
    wrap_enabled=True, wrap_edge_threshold=0.15, wrap_layers=3, wrap_layer_spacing=0.5, wrap_opacity_falloff=0.7,
    wrap_max_angle=75.0, wrap_aspect=2.0,
    shell_enabled=True, shell_thickness=0.3, shell_back_opacity=0.6, shell_back_darken=0.8, shell_connect_walls=True,
    shell_wall_segments=3, shell_wall_opacity=0.5, shell_edge_threshold=0.1,
    density_enabled=True, density_gradient_threshold=0.08, density_extra_count=4, density_position_jitter=0.6,
    density_size_variance=0.3, density_opacity_scale=0.7, seed=12345)


def params_dict(params=None, **overrides):
    """DEFAULTS <- `params` (a dict, or any object with these attributes) <- overrides."""
    p = dict(DEFAULTS)
    if params is not None:
        src = params if isinstance(params, dict) else {k: getattr(params, k) for k in DEFAULTS if hasattr(params, k)}
        unknown = set(src) - set(DEFAULTS)
        assert not unknown, f"unknown parameters {sorted(unknown)}"
        p.update(src)
    unknown = set(overrides) - set(DEFAULTS)
    assert not unknown, f"unknown parameters {sorted(unknown)}"
    p.update(overrides)
    return p


# ---- GLM ----------------------------------------------------------------------------------------------------------------------
def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def length3(a):
    return np.sqrt(dot3(a, a))


def scale3(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def div3(a, s):
    return (a[0] / s, a[1] / s, a[2] / s)


def add3(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def normalize3(a):
    return scale3(a, ONE / np.sqrt(dot3(a, a)))


def cross3(x, y):
    return (x[1] * y[2] - y[1] * x[2], x[2] * y[0] - y[2] * x[0], x[0] * y[1] - y[0] * x[1])


def where3(m, a, b):
    return tuple(np.where(m, a[i], b[i]) for i in range(3))


def const3(like, x, y, z):
    return (np.full_like(like, F(x)), np.full_like(like, F(y)), np.full_like(like, F(z)))


def angle_axis(angle, v):
    h = angle * HALF
    s = np.sin(h)
    return (np.cos(h), v[0] * s, v[1] * s, v[2] * s)


def clamp(v, lo, hi):
    """std::clamp: v < lo ? lo : hi < v ? hi : v"""
    return np.where(v < lo, lo, np.where(hi < v, hi, v))


def quaternion_from_normal(n):
    """PC:101-118 -> (w, x, y, z)"""
    up = const3(n[0], 0, 0, 1)
    axis = cross3(up, n)
    d = dot3(up, n)
    axis_len = length3(axis)
    general = angle_axis(np.arccos(clamp(d, F(-1.0), ONE)), normalize3(axis))
    flipped = angle_axis(np.full_like(d, PI), const3(d, 1, 0, 0))
    ident = (np.ones_like(d), np.zeros_like(d), np.zeros_like(d), np.zeros_like(d))
    par = axis_len < F(1e-6)
    return tuple(np.where(par, np.where(d > ZERO, ident[i], flipped[i]), general[i]) for i in range(4))


def slerp_from_identity(q, t):
    """glm::slerp(identity, q, t), PC:226"""
    c = q[0]  # dot((1, 0, 0, 0), q)
    neg = c < ZERO
    q = tuple(np.where(neg, -q[i], q[i]) for i in range(4))
    c = np.where(neg, -c, c)
    u = ONE - t
    x = (ONE, ZERO, ZERO, ZERO)
    lerp = tuple(x[i] * u + q[i] * t for i in range(4))
    a = np.arccos(c)
    s0, s1, s = np.sin((ONE - t) * a), np.sin(t * a), np.sin(a)
    gen = tuple((s0 * x[i] + s1 * q[i]) / s for i in range(4))
    near = c > ONE - FLT_EPSILON
    return tuple(np.where(near, lerp[i], gen[i]) for i in range(4))


def pseudo_random(x, y, i, seed):
    """PC:190-194: uint32 arithmetic (here in uint64, masked), then / 65535.0f.  x, y: integer arrays."""
    m = np.uint64(0xFFFFFFFF)
    x, y = np.asarray(x).astype(np.uint64), np.asarray(y).astype(np.uint64)
    iu = np.uint64(int(i) & 0xFFFFFFFF)
    h = (x * np.uint64(374761393) + y * np.uint64(668265263) + iu * np.uint64(2147483647) + np.uint64(int(seed) & 0xFFFFFFFF)) & m
    h = h ^ np.uint64(0x85EBCA6B)
    h = (((h >> np.uint64(16)) ^ h) * np.uint64(0x7FEB352D)) & m
    return (h & np.uint64(0xFFFF)).astype(np.float32) / F(65535.0)


# ---- image.cpp ------------------------------------------------------------------------------------------------------------------
def sobel(depth, xs, ys, mutate=None):
    """(gx, gy) of IM:164-180 at the pixels (xs, ys); at_safe reads zero outside the frame."""
    H, W = depth.shape

    def at(x, y):
        if mutate == "edge_clamp":
            return depth[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(inside, depth[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], ZERO)

    d00, d10, d20 = at(xs - 1, ys - 1), at(xs, ys - 1), at(xs + 1, ys - 1)
    d01, d21 = at(xs - 1, ys), at(xs + 1, ys)
    d02, d12, d22 = at(xs - 1, ys + 1), at(xs, ys + 1), at(xs + 1, ys + 1)
    gx = (-d00 + d20 - TWO * d01 + TWO * d21 - d02 + d22) / F(8.0)
    gy = (-d00 - TWO * d10 - d20 + d02 + TWO * d12 + d22) / F(8.0)
    return gx, gy


def _bounds(pos):
    return tuple(np.fmin.reduce(c) for c in pos), tuple(np.fmax.reduce(c) for c in pos)


def _center(pos):
    """PointCloud::center, PC:448-458"""
    lo, hi = _bounds(pos)
    return tuple(pos[k] - (lo[k] + hi[k]) * HALF for k in range(3))


def place_points(pos, normalize_extent, mutate=None):
    """center(); normalize(extent) as the viewer calls them (VW:385-386) on pos = (x, y, z) arrays of a non-empty cloud;
    normalize() centres once more before it measures the extent (PC:460-479).  normalize_extent <= 0: untouched."""
    normalize_extent = F(normalize_extent)
    if not (normalize_extent > ZERO):
        return pos
    pos = _center(pos)
    if mutate != "center_once":
        pos = _center(pos)                                           # normalize() centres first, PC:464
    lo, hi = _bounds(pos)
    ext = [hi[k] - lo[k] for k in range(3)]
    max_extent = np.fmax(np.fmax(ext[0], ext[1]), ext[2])
    if not (max_extent < F(1e-6)):                                   # PC:472
        pos = scale3(pos, normalize_extent / max_extent)
    return pos


def surface_cloud(depth, color=None, params=None, mutate=None, **overrides):
    """One image: depth (H, W) fp32 (curve already applied), color (3, H, W) fp32 or None -> dict of
        positions (N,3), scales (N,3), rotations (N,4) wxyz, colors (N,3), opacities (N,)      the rows, in emit order
        kinds (N,)  K_BASE ... K_FILL       point (N,)  the row's grid point
        flags (P,)  per grid point, the KEPT ... FILLS bits      counts (P,)  rows per grid point
        max_gradient, min_d, range"""
    assert mutate is None or mutate in MUTATIONS
    p = params_dict(params, **overrides)
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    H, W = depth.shape
    sub = int(p["subsample"])
    fp = {k: F(v) for k, v in p.items() if isinstance(v, float)}
    with np.errstate(all="ignore"):
        # ---- from_depth, PC:8-76, driven as VW:363-377 ------------------------------------------------------------------------
        fx = fp["fx"] if fp["fx"] > ZERO else F(W) * F(0.8)
        fy = fp["fy"] if fp["fy"] > ZERO else fx
        cx = fp["cx"] if fp["cx"] > ZERO else F(W) * HALF
        cy = fp["cy"] if fp["cy"] > ZERO else F(H) * HALF
        ds = fp["depth_scale"]
        min_d, max_d = np.fmin.reduce(depth.reshape(-1)), np.fmax.reduce(depth.reshape(-1))
        rng = max_d - min_d
        if rng < F(1e-6):
            rng = ONE
        gy_, gx_ = np.meshgrid(np.arange(0, H, sub), np.arange(0, W, sub), indexing="ij")
        xs_all, ys_all = gx_.reshape(-1), gy_.reshape(-1)          # row-major: y outer, x inner (PC:36-37)
        P = xs_all.size
        d = depth[ys_all, xs_all]
        nd = (d - min_d) / rng
        z = (ONE - nd) * ds
        keep = ~(z < F(0.01) * ds)                                   # PC:46
        flags = np.where(keep, KEPT, 0).astype(np.uint8)
        sel = np.nonzero(keep)[0]
        xs, ys, z, conf = xs_all[sel], ys_all[sel], z[sel], nd[sel]
        pos = ((xs.astype(np.float32) - cx) / fx * z, (cy - ys.astype(np.float32)) / fy * z, -z)   # PC:49-51
        n_pt = sel.size
        empty = dict(positions=np.zeros((0, 3), np.float32), scales=np.zeros((0, 3), np.float32),
                     rotations=np.zeros((0, 4), np.float32), colors=np.zeros((0, 3), np.float32),
                     opacities=np.zeros(0, np.float32), kinds=np.zeros(0, np.int32), point=np.zeros(0, np.int64),
                     flags=flags, counts=np.zeros(P, np.int32), max_gradient=ONE, min_d=min_d, range=rng)
        if n_pt == 0:                                                # VW:379-382
            return empty
        if color is None:
            col = const3(z, 0.7, 0.7, 0.7)                           # PC:54
        else:
            color = np.ascontiguousarray(color, dtype=np.float32)
            col = tuple(color[c][ys, xs] for c in range(3))

        # ---- center(); normalize(extent), VW:385-386, PC:448-479 ---------------------------------------------------------------
        pos = place_points(pos, fp["normalize_extent"], mutate)

        # ---- compute_surface_info, IM:157-207 ------------------------------------------------------------------------------------
        gx, gy = sobel(depth, xs, ys, mutate)
        mag = np.sqrt(gx * gx + gy * gy)
        has_dir = mag > F(1e-6)
        dir_x, dir_y = np.where(has_dir, gx / mag, ZERO), np.where(has_dir, gy / mag, ZERO)
        normal = (-gx * fp["gradient_scale"], -gy * fp["gradient_scale"], np.ones_like(gx))
        nlen = length3(normal)
        normal = where3(nlen > F(1e-6), div3(normal, nlen), const3(gx, 0, 0, 1))

        # ---- to_surface_gaussians, PC:159-431 ----------------------------------------------------------------------------------------
        emits = ~(conf < fp["min_confidence"])                        # PC:208
        pool = mag[emits] if mutate == "skip_before_maxgrad" else mag   # PC:197-203: over ALL points of the cloud
        max_gradient = np.fmax.reduce(np.concatenate([np.zeros(1, np.float32), pool]))
        if max_gradient < F(1e-6):
            max_gradient = ONE
        gt = np.greater_equal if mutate == "non_strict" else np.greater

        rotation = slerp_from_identity(quaternion_from_normal(normal), fp["normal_strength"])
        base = fp["base_size"] * (HALF + HALF * conf)
        tangent_scale, normal_scale = base, base / fp["aspect_ratio"]
        ng = mag / max_gradient
        t = clamp((ng - fp["edge_threshold"]) / (ONE - fp["edge_threshold"]), ZERO, ONE)
        edge_factor = np.where(ng > fp["edge_threshold"], ONE - t * (ONE - fp["edge_shrink"]), ONE)
        scale = (tangent_scale * edge_factor, tangent_scale * edge_factor, normal_scale * edge_factor)
        final_opacity = fp["opacity"] * conf * (F(0.7) + F(0.3) * edge_factor)

        L_wall, L_wrap, L_fill = int(p["shell_wall_segments"]), int(p["wrap_layers"]), int(p["density_extra_count"])
        fan = 2 + L_wall + L_wrap + L_fill
        rows = np.zeros((n_pt, fan, 14), np.float32)
        valid = np.zeros((n_pt, fan), bool)
        kinds = np.zeros((n_pt, fan), np.int32)

        def put(slot, mask, kind, ps, sc, q, c, op):
            vals = list(ps) + list(sc) + list(q) + list(c) + [op]
            for j, v in enumerate(vals):
                rows[:, slot, j] = np.broadcast_to(v, (n_pt,))
            valid[:, slot] = mask
            kinds[:, slot] = kind

        put(0, emits, K_BASE, pos, scale, rotation, col, final_opacity)                         # PC:253-261

        # the view-aligned frame shared by the walls (PC:299-307) and compute_wrap_direction (PC:128-139)
        view_dir = normalize3(pos)
        world_up = const3(z, 0, 1, 0)
        right = normalize3(cross3(world_up, view_dir))
        right = where3(length3(right) < F(1e-6), const3(z, 1, 0, 0), right)
        up = cross3(view_dir, right)
        grad_3d = add3(scale3(right, dir_x), scale3(up, dir_y))

        # volumetric shell, PC:268-343
        shell = emits & bool(p["shell_enabled"]) & gt(ng, fp["shell_edge_threshold"])
        back_pos = add3(pos, scale3(view_dir, fp["shell_thickness"]))
        put(1, shell, K_BACK, back_pos, scale, quaternion_from_normal(view_dir), scale3(col, fp["shell_back_darken"]),
            final_opacity * fp["shell_back_opacity"])
        tangent_len = length3(grad_3d)
        walls = shell & bool(p["shell_connect_walls"]) & (tangent_len > F(0.1))
        tangent = div3(grad_3d, tangent_len)
        wall_rot = quaternion_from_normal(normalize3(cross3(view_dir, tangent)))
        for seg in range(1, L_wall + 1):
            tt = F(seg) / F(L_wall + 1)
            wall_pos = add3(scale3(pos, ONE - tt), scale3(back_pos, tt))                      # glm::mix
            put(1 + seg, walls, K_WALL, wall_pos, scale3(scale, F(0.9)), wall_rot, col, final_opacity * fp["shell_wall_opacity"])

        # silhouette wrapping, PC:348-394, compute_wrap_direction PC:122-157
        dir_len = np.sqrt(dir_x * dir_x + dir_y * dir_y)
        wraps = emits & bool(p["wrap_enabled"]) & gt(ng, fp["wrap_edge_threshold"]) & (dir_len > F(0.1))
        wrap = cross3(normal, grad_3d)
        flip = dot3(wrap, view_dir) < ZERO
        wrap = where3(flip, tuple(-c for c in wrap), wrap)
        wrap_len = length3(wrap)
        wrap_dir = where3(wrap_len < F(1e-6), normalize3(grad_3d), div3(wrap, wrap_len))
        wrap_rot = quaternion_from_normal(tuple(-c for c in wrap_dir))
        wrap_base = base * F(0.8)
        wrap_scale = (wrap_base, wrap_base, wrap_base / fp["wrap_aspect"])
        for layer in range(L_wrap):
            offset = F(layer + 1) * fp["wrap_layer_spacing"] * fp["base_size"]
            wrap_op = final_opacity * np.power(fp["wrap_opacity_falloff"], F(layer + 1))
            put(2 + L_wall + layer, wraps, K_WRAP, add3(pos, scale3(wrap_dir, offset)), wrap_scale, wrap_rot, col, wrap_op)

        # adaptive density, PC:399-427
        fills = emits & bool(p["density_enabled"]) & gt(ng, fp["density_gradient_threshold"])
        jitter = fp["density_position_jitter"] * base
        for i in range(L_fill):
            r = [(pseudo_random(xs, ys, i * 3 + k, p["seed"]) - HALF) * TWO for k in range(3)]
            size_var = ONE + (pseudo_random(xs, ys, i * 3 + 100, p["seed"]) - HALF) * fp["density_size_variance"] * TWO
            put(2 + L_wall + L_wrap + i, fills, K_FILL, add3(pos, scale3(tuple(r), jitter)),
                scale3(scale3(scale, size_var), F(0.8)), rotation, col, final_opacity * fp["density_opacity_scale"])

    flags[sel] |= (np.where(emits, BASE, 0) | np.where(shell, BACK, 0) | np.where(walls, WALLS, 0) | np.where(wraps, WRAPS, 0) |
                   np.where(fills, FILLS, 0)).astype(np.uint8)
    counts = np.zeros(P, np.int32)
    counts[sel] = valid.sum(axis=1)
    flat = rows[valid]                                               # boolean gather in row-major order = the emit order
    point = np.broadcast_to(sel[:, None], valid.shape)[valid]
    return dict(positions=flat[:, 0:3].copy(), scales=flat[:, 3:6].copy(), rotations=flat[:, 6:10].copy(),
                colors=flat[:, 10:13].copy(), opacities=flat[:, 13].copy(), kinds=kinds[valid], point=point,
                flags=flags, counts=counts, max_gradient=max_gradient, min_d=min_d, range=rng)


def surface_clouds(depth, color=None, params=None, **overrides):
    """A batch: depth (B, H, W), color (B, 3, H, W) or None -> list of surface_cloud dicts."""
    return [surface_cloud(depth[b], None if color is None else color[b], params, **overrides) for b in range(depth.shape[0])]


def rows_per_flag(flags, params=None, **overrides):
    """Row count of every grid point from its flag byte -- how the scan counts (fgs_surface.hip rows_of)."""
    p = params_dict(params, **overrides)
    f = np.asarray(flags).astype(np.int64)
    return ((f & BASE) != 0) * 1 + ((f & BACK) != 0) * 1 + ((f & WALLS) != 0) * int(p["shell_wall_segments"]) + \
        ((f & WRAPS) != 0) * int(p["wrap_layers"]) + ((f & FILLS) != 0) * int(p["density_extra_count"])
