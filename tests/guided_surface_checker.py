"""Checker of the feature-guided SAAG emit (fgs_surface_emit_guided / fgs_surface_guided_backward, include/fgs.h "Feature-guided
SAAG"): tests/surface_checker.py's emit restated in torch with PER-POINT parameters, so that autograd differentiates it.

Two kinds of values, kept apart:
  * what no guide map can change -- positions, confidence, Sobel gradient, normal, the quaternion of the normal, the view frame, the
    wrap direction, the jitter, the flags -- is computed in NumPy fp32 exactly as surface_checker does (its helpers, its operation
    order): the kernel reproduces these bit for bit.  The BRANCH MASKS are taken from this fp32 restatement too: the strict
    `ng > edge_threshold'` compare, the clamp interval of t, slerp's `c > 1 - FLT_EPSILON` and (inside quaternion_from_normal) the
    `length(axis) < 1e-6` test.  Each mask is what the fp32 forward decides, whatever the dtype of the run;
  * the smooth arithmetic that reads the effective parameters runs in the requested dtype (torch.float32 or torch.float64) under
    autograd, on those constants.  Parameters and literals are the fp32 values the kernel holds (0.7f, not 0.7).
The derivative follows the branch the forward took: a clamped t is a constant, except on the closed interval [0, 1].

`mutate` switches exactly one rule off (tests/test_guided_surface_checker.py proves that each is pinned):
    "patch_from_grid"   the patch comes from the subsample-grid index, (gx Wp) / grid_w, instead of the pixel, (x Wp) / W
    "non_strict"        the edge compare is `ng >= edge_threshold'`
    "clamp_open"        the clamp's gradient is dropped at t == 1 (an open upper end)
"""
import numpy as np
import torch

import surface_checker as C

F = np.float32
MOD_KEYS = ("aspect_ratio_mult", "edge_threshold_add", "edge_shrink_mult", "normal_strength_mult", "base_size_mult", "opacity_mult")
IDENTITY = (1.0, 0.0, 1.0, 1.0, 1.0, 1.0)
MUTATIONS = ("patch_from_grid", "non_strict", "clamp_open")
KEYS = ("positions", "scales", "rotations", "colors", "opacities")


def identity_mods(Hp, Wp, dtype=torch.float32):
    return torch.tensor(IDENTITY, dtype=dtype).reshape(6, 1, 1).repeat(1, Hp, Wp)


def patch_of(xs, ys, W, H, Wp, Hp, sub=1, mutate=None):
    """(py, px) of the pixels (xs, ys): integer division on pixel coordinates."""
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    if mutate == "patch_from_grid":
        gw, gh = (W + sub - 1) // sub, (H + sub - 1) // sub
        return ((ys // sub) * Hp) // gh, ((xs // sub) * Wp) // gw
    return (ys * Hp) // H, (xs * Wp) // W


def _geometry(depth, color, p):
    """Everything of surface_checker.surface_cloud that precedes the guided parameters, for the KEPT points, in NumPy fp32 and in
    that function's operation order (see there for the citations)."""
    with np.errstate(all="ignore"):
        return _geometry_of(np.ascontiguousarray(depth, dtype=np.float32), color, p)


def _geometry_of(depth, color, p):
    ZERO, HALF, ONE, TWO = C.ZERO, C.HALF, C.ONE, C.TWO
    H, W = depth.shape
    sub = int(p["subsample"])
    fp = {k: F(v) for k, v in p.items() if isinstance(v, float)}
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
    xs_all, ys_all = gx_.reshape(-1), gy_.reshape(-1)
    nd = (depth[ys_all, xs_all] - min_d) / rng
    z = (ONE - nd) * ds
    sel = np.nonzero(~(z < F(0.01) * ds))[0]
    g = dict(P=xs_all.size, sel=sel)
    if sel.size == 0:
        return g
    xs, ys, z, conf = xs_all[sel], ys_all[sel], z[sel], nd[sel]
    pos = ((xs.astype(np.float32) - cx) / fx * z, (cy - ys.astype(np.float32)) / fy * z, -z)
    col = C.const3(z, 0.7, 0.7, 0.7) if color is None else tuple(np.ascontiguousarray(color, np.float32)[c][ys, xs] for c in range(3))
    pos = C.place_points(pos, fp["normalize_extent"])
    gx, gy = C.sobel(depth, xs, ys)
    mag = np.sqrt(gx * gx + gy * gy)
    has_dir = mag > F(1e-6)
    dir_x, dir_y = np.where(has_dir, gx / mag, ZERO), np.where(has_dir, gy / mag, ZERO)
    normal = (-gx * fp["gradient_scale"], -gy * fp["gradient_scale"], np.ones_like(gx))
    nlen = C.length3(normal)
    normal = C.where3(nlen > F(1e-6), C.div3(normal, nlen), C.const3(gx, 0, 0, 1))
    max_gradient = np.fmax.reduce(np.concatenate([np.zeros(1, np.float32), mag]))
    if max_gradient < F(1e-6):
        max_gradient = ONE
    view_dir = C.normalize3(pos)
    right = C.normalize3(C.cross3(C.const3(z, 0, 1, 0), view_dir))
    right = C.where3(C.length3(right) < F(1e-6), C.const3(z, 1, 0, 0), right)
    up = C.cross3(view_dir, right)
    grad_3d = C.add3(C.scale3(right, dir_x), C.scale3(up, dir_y))
    back_pos = C.add3(pos, C.scale3(view_dir, fp["shell_thickness"]))
    tangent = C.div3(grad_3d, C.length3(grad_3d))
    wrap = C.cross3(normal, grad_3d)
    wrap = C.where3(C.dot3(wrap, view_dir) < ZERO, tuple(-c for c in wrap), wrap)
    wrap_len = C.length3(wrap)
    wrap_dir = C.where3(wrap_len < F(1e-6), C.normalize3(grad_3d), C.div3(wrap, wrap_len))
    L_wall, L_fill = int(p["shell_wall_segments"]), int(p["density_extra_count"])
    wall_pos = []
    for seg in range(1, L_wall + 1):
        tt = F(seg) / F(L_wall + 1)
        wall_pos.append(C.add3(C.scale3(pos, ONE - tt), C.scale3(back_pos, tt)))
    fill_r, fill_var = [], []
    for i in range(L_fill):
        fill_r.append(tuple((C.pseudo_random(xs, ys, i * 3 + k, p["seed"]) - HALF) * TWO for k in range(3)))
        fill_var.append(ONE + (C.pseudo_random(xs, ys, i * 3 + 100, p["seed"]) - HALF) * fp["density_size_variance"] * TWO)
    g.update(xs=xs, ys=ys, conf=conf, pos=pos, col=col, c1=HALF + HALF * conf, ng=mag / max_gradient,
             q=C.quaternion_from_normal(normal), back_pos=back_pos, back_rot=C.quaternion_from_normal(view_dir),
             back_col=C.scale3(col, fp["shell_back_darken"]), wall_pos=wall_pos,
             wall_rot=C.quaternion_from_normal(C.normalize3(C.cross3(view_dir, tangent))), wrap_dir=wrap_dir,
             wrap_rot=C.quaternion_from_normal(tuple(-c for c in wrap_dir)), fill_r=fill_r, fill_var=fill_var)
    return g


def clamp_interval(t32, mutate=None):
    """Where the clamp of t passes its gradient: the closed interval [0, 1], decided on the fp32 value."""
    return ~(t32 < C.ZERO) & (~(C.ONE < t32) if mutate != "clamp_open" else (t32 < C.ONE))


def edge_factor(ng, threshold32, threshold, shrink, mutate=None):
    """edge_factor of the points with normalized gradient `ng` (fp32 array): threshold32 the fp32 effective threshold (array, decides
    the branches), `threshold` and `shrink` the effective values as tensors of the run's dtype.  -> (edge_factor, edge mask)."""
    dt = threshold.dtype
    ngt = torch.from_numpy(ng).to(dt)
    with np.errstate(all="ignore"):
        edge = (ng >= threshold32) if mutate == "non_strict" else (ng > threshold32)
        t32 = (ng - threshold32) / (C.ONE - threshold32)
        inside = clamp_interval(t32, mutate)
        clamped = torch.from_numpy(C.clamp(t32, C.ZERO, C.ONE)).to(dt)
    t = torch.where(torch.from_numpy(inside), (ngt - threshold) / (1.0 - threshold), clamped)
    return torch.where(torch.from_numpy(edge), 1.0 - t * (1.0 - shrink), torch.ones_like(t)), edge


def slerp_from_identity(q, t):
    """glm::slerp(identity, q, t) for q = four fp32 arrays and t a tensor: the sign flip and the branch from fp32, each branch
    differentiated as written."""
    dt = t.dtype
    neg = q[0] < C.ZERO
    q = tuple(np.where(neg, -c, c) for c in q)
    near = torch.from_numpy(q[0] > C.ONE - C.FLT_EPSILON)
    qt = [torch.from_numpy(np.ascontiguousarray(c)).to(dt) for c in q]
    u = 1.0 - t
    x = (1.0, 0.0, 0.0, 0.0)
    lerp = [x[i] * u + qt[i] * t for i in range(4)]
    c = torch.where(near, torch.full_like(qt[0], 0.5), qt[0])      # the unused branch stays finite (and out of the gradient)
    a = torch.acos(c)
    s0, s1, s = torch.sin((1.0 - t) * a), torch.sin(t * a), torch.sin(a)
    gen = [(s0 * x[i] + s1 * qt[i]) / s for i in range(4)]
    return [torch.where(near, lerp[i], gen[i]) for i in range(4)]


def guided_cloud(depth, color, mods, params=None, dtype=torch.float32, mutate=None, **overrides):
    """One image: depth (H, W) fp32 (curve applied), color (3, H, W) or None, mods (6, Hp, Wp) tensor (may require grad) -> dict of
        positions (N,3), scales (N,3), rotations (N,4), colors (N,3), opacities (N,)   tensors of `dtype`, in emit order
        kinds (N,), point (N,), flags (P,), counts (P,)                                 NumPy, as surface_checker.surface_cloud
        point_rows (P,) int32   first row of every point with a base row, -1 elsewhere"""
    assert mutate is None or mutate in MUTATIONS
    p = C.params_dict(params, **overrides)
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    H, W = depth.shape
    Hp, Wp = int(mods.shape[1]), int(mods.shape[2])
    plain = C.surface_cloud(depth, color, p)                          # flags, counts, kinds, row order: no guide can change them
    counts = plain["counts"].astype(np.int64)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    point_rows = np.where((plain["flags"] & C.BASE) != 0, first, -1).astype(np.int32)
    out = dict(kinds=plain["kinds"], point=plain["point"], flags=plain["flags"], counts=plain["counts"], point_rows=point_rows)
    g = _geometry(depth, color, p)
    if g["sel"].size == 0 or plain["kinds"].size == 0:
        out.update(positions=torch.zeros(0, 3, dtype=dtype), scales=torch.zeros(0, 3, dtype=dtype), rotations=torch.zeros(0, 4, dtype=dtype),
                   colors=torch.zeros(0, 3, dtype=dtype), opacities=torch.zeros(0, dtype=dtype))
        if mods.requires_grad:                                         # an empty cloud still hangs on the maps (with zero gradient)
            for k in KEYS:
                out[k] = out[k] + 0.0 * mods.to(dtype).sum()
        return out
    sel, n_pt = g["sel"], g["sel"].size
    fl = plain["flags"][sel]
    emits, shell, walls = (fl & C.BASE) != 0, (fl & C.BACK) != 0, (fl & C.WALLS) != 0
    wraps, fills = (fl & C.WRAPS) != 0, (fl & C.FILLS) != 0

    def K(v):                                                          # the fp32 value the kernel holds, as a Python float
        return float(F(v))

    def T(a):
        # (a constant of a row that is NOT emitted may be NaN -- the wrap direction of a point without a gradient direction --;
        # it is zeroed so that the row's zero upstream gradient does not become 0 x NaN.  An emitted row's constants are finite.)
        a = np.array(np.broadcast_to(a, (n_pt,)))
        return torch.from_numpy(np.where(np.isfinite(a), a, np.zeros_like(a))).to(dtype)

    def T3(v):
        return [T(c) for c in v]

    # ---- effective parameters per point --------------------------------------------------------------------------------------------
    py, px = patch_of(g["xs"], g["ys"], W, H, Wp, Hp, int(p["subsample"]), mutate)
    m = mods.to(dtype)[:, torch.from_numpy(py), torch.from_numpy(px)]                       # (6, n_pt)
    m32 = mods.detach().to(torch.float32).numpy()[:, py, px]
    aspect, threshold, shrink = K(p["aspect_ratio"]) * m[0], K(p["edge_threshold"]) + m[1], K(p["edge_shrink"]) * m[2]
    strength, base_size, opacity = K(p["normal_strength"]) * m[3], K(p["base_size"]) * m[4], K(p["opacity"]) * m[5]
    threshold32 = F(p["edge_threshold"]) + m32[1]

    # ---- the emit, PC:225-427, on them -----------------------------------------------------------------------------------------------
    conf = T(g["conf"])
    rotation = slerp_from_identity(g["q"], strength)
    base = base_size * T(g["c1"])
    normal_scale = base / aspect
    ef, _ = edge_factor(g["ng"], threshold32, threshold, shrink, mutate)
    scale = [base * ef, base * ef, normal_scale * ef]
    final_opacity = opacity * conf * (K(0.7) + K(0.3) * ef)
    pos, col = T3(g["pos"]), T3(g["col"])

    L_wall, L_wrap, L_fill = int(p["shell_wall_segments"]), int(p["wrap_layers"]), int(p["density_extra_count"])
    slots, valid = [], []

    def put(mask, ps, sc, q, c, op):
        slots.append(torch.stack(list(ps) + list(sc) + list(q) + list(c) + [op], dim=1))
        valid.append(mask)

    put(emits, pos, scale, rotation, col, final_opacity)
    put(shell, T3(g["back_pos"]), scale, [T(c) for c in g["back_rot"]], T3(g["back_col"]), final_opacity * K(p["shell_back_opacity"]))
    wall_rot = [T(c) for c in g["wall_rot"]]
    for seg in range(L_wall):
        put(walls, T3(g["wall_pos"][seg]), [c * K(0.9) for c in scale], wall_rot, col, final_opacity * K(p["shell_wall_opacity"]))
    wrap_dir, wrap_rot = T3(g["wrap_dir"]), [T(c) for c in g["wrap_rot"]]
    wrap_base = base * K(0.8)
    wrap_scale = [wrap_base, wrap_base, wrap_base / K(p["wrap_aspect"])]
    for layer in range(L_wrap):
        offset = K(F(layer + 1) * F(p["wrap_layer_spacing"])) * base_size
        falloff = K(np.power(F(p["wrap_opacity_falloff"]), F(layer + 1)))
        put(wraps, [pos[k] + wrap_dir[k] * offset for k in range(3)], wrap_scale, wrap_rot, col, final_opacity * falloff)
    jitter = K(p["density_position_jitter"]) * base
    for i in range(L_fill):
        r, var = T3(g["fill_r"][i]), T(g["fill_var"][i])
        put(fills, [pos[k] + r[k] * jitter for k in range(3)], [c * var * K(0.8) for c in scale], rotation, col,
            final_opacity * K(p["density_opacity_scale"]))

    rows = torch.stack(slots, dim=1)                                   # (n_pt, fan, 14)
    flat = rows[torch.from_numpy(np.stack(valid, axis=1))]             # row-major boolean gather = the emit order
    assert flat.shape[0] == plain["kinds"].size
    out.update(positions=flat[:, 0:3], scales=flat[:, 3:6], rotations=flat[:, 6:10], colors=flat[:, 10:13], opacities=flat[:, 13])
    return out


def guided_clouds(depth, color, mods, params=None, dtype=torch.float32, **overrides):
    """A batch: depth (B,H,W), color (B,3,H,W) or None, mods (B,6,Hp,Wp) tensor -> list of guided_cloud dicts."""
    return [guided_cloud(depth[b], None if color is None else color[b], mods[b], params, dtype, **overrides)
            for b in range(depth.shape[0])]
