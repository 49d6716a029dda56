"""fp64 statement of the fused CVS loss's definition (include/fgs.h, fgs_cvs_*): the quality mask, the four terms, g_pred and the
Euler step, in NumPy; and the input recipe of its tests.  A plain module: the tests of the checker hold it against the reference's
fixtures (tests/test_cvs_loss_checker.py), the GPU tests hold the kernels against it (tests/test_hip_cvs_loss.py).

`rules` changes ONE rule of the definition at a time, for the tests that prove the fixtures can tell: border "wrap" | "clamp";
compare ">" | ">="; divisor "W-1" | "W"; mask_at "x" | "x+1"; tie 0 | 1.
"""
import numpy as np

EDGE = float(np.float32(0.01))   # torch's `fp32 tensor > 0.01` is "greater than the fp32 value of 0.01"
EPS = float(np.float32(1e-8))
RULES = dict(border="wrap", compare=">", divisor="W-1", mask_at="x", tie=0)
TERMS = ("l1_weighted", "consistency", "boundary", "gradient")


def _rules(rules):
    out = dict(RULES)
    out.update(rules or {})
    assert set(out) == set(RULES), f"unknown rule in {rules}"
    return out


def _shift(d, step, axis, border):
    """d at index + step along `axis`: circular (torch.roll(d, -step)) or clamped to the border."""
    if border == "wrap":
        return np.roll(d, -step, axis=axis)
    idx = np.clip(np.arange(d.shape[axis]) + step, 0, d.shape[axis] - 1)
    return np.take(d, idx, axis=axis)


def quality_mask(depth, threshold=0.01, sharpness=100.0, rules=None):
    """m = sigmoid(-sharpness (lap - threshold)); threshold and sharpness are the fp32 values the entry points take."""
    r = _rules(rules)
    d = np.asarray(depth, np.float64)
    thr, sharp = float(np.float32(threshold)), float(np.float32(sharpness))
    lap = np.abs((((_shift(d, -1, -2, r["border"]) + _shift(d, 1, -2, r["border"])) + _shift(d, -1, -1, r["border"]))
                  + _shift(d, 1, -1, r["border"])) - 4.0 * d)
    z = -sharp * (lap - thr)
    with np.errstate(over="ignore"):
        return np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))


def sgn(a, b, tie=0):
    return (a > b).astype(np.float64) - (a < b).astype(np.float64) + tie * (a == b).astype(np.float64)


def boundary_bits(depth, rules=None):
    """bx (B, 1, H, W-1), by (B, 1, H-1, W) as 0 / 1."""
    r = _rules(rules)
    d = np.asarray(depth, np.float64)
    dx, dy = np.abs(d[..., :, :-1] - d[..., :, 1:]), np.abs(d[..., :-1, :] - d[..., 1:, :])
    if r["compare"] == ">":
        return (dx > EDGE).astype(np.float64), (dy > EDGE).astype(np.float64)
    return (dx >= EDGE).astype(np.float64), (dy >= EDGE).astype(np.float64)


def loss(pred, target, depth=None, ema=None, *, quality=True, consistency="l1", boundary=False, gradient=False, threshold=0.01,
         sharpness=100.0, g_terms=None, rules=None):
    """-> dict(mask (B, 1, H, W), terms float64[4], g_pred (with g_terms: the four upstream gradients)).  A term that is off is 0."""
    r = _rules(rules)
    p, t = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    Bn, C, H, W = p.shape
    n = float(Bn * C * H * W)
    m = quality_mask(depth, threshold, sharpness, rules) if quality else np.ones((Bn, 1, H, W))
    terms = np.zeros(4)
    a = np.abs(p - t)
    terms[0] = (m * a).sum() / n
    if consistency is not None:
        e = np.asarray(ema, np.float64)
        terms[1] = (np.abs(p - e).sum() if consistency == "l1" else ((p - e) ** 2).sum()) / n
    Wd, Hd = (W - 1, H - 1) if r["divisor"] == "W-1" else (W, H - 1)
    if boundary:
        bx, by = boundary_bits(depth, rules)
        pe = a.mean(axis=1, keepdims=True)
        terms[2] = (pe[..., :, :-1] * bx).sum() / (Bn * H * Wd) + (pe[..., :-1, :] * by).sum() / (Bn * Hd * W)
    if gradient:
        mx = m[..., :, :-1] if r["mask_at"] == "x" else m[..., :, 1:]
        my = m[..., :-1, :] if r["mask_at"] == "x" else m[..., 1:, :]
        terms[3] = ((np.abs(p[..., :, :-1] - p[..., :, 1:]) * mx).sum() / (Bn * C * H * Wd)
                    + (np.abs(p[..., :-1, :] - p[..., 1:, :]) * my).sum() / (Bn * C * Hd * W))
    out = dict(mask=m, terms=terms)
    if g_terms is not None:
        g0, g1, g2, g3 = (float(v) for v in g_terms)
        s_pt = sgn(p, t, r["tie"])
        g = g0 * s_pt * m / n
        if consistency == "l1":
            g = g + g1 * sgn(p, e, r["tie"]) / n
        elif consistency == "mse":
            g = g + g1 * 2.0 * (p - e) / n
        if boundary:
            coef = np.zeros((Bn, 1, H, W))
            coef[..., :, :-1] += bx / (Bn * H * Wd)
            coef[..., :-1, :] += by / (Bn * Hd * W)
            g = g + g2 * s_pt / C * coef
        if gradient:
            sx = sgn(p[..., :, :-1], p[..., :, 1:], r["tie"]) * mx / (Bn * C * H * Wd)
            sy = sgn(p[..., :-1, :], p[..., 1:, :], r["tie"]) * my / (Bn * C * Hd * W)
            tv = np.zeros_like(p)
            tv[..., :, :-1] += sx
            tv[..., :, 1:] -= sx
            tv[..., :-1, :] += sy
            tv[..., 1:, :] -= sy
            g = g + g3 * tv
        out["g_pred"] = g
    return out


def euler_step(x0_pred, noisy, sqrt_alphas_cumprod, timestep):
    """-> x_prev (B, C, H, W), t_prev (B,) in fp64; a timestep outside the table is clamped into it."""
    sac = np.asarray(sqrt_alphas_cumprod, np.float64)
    t = np.clip(np.asarray(timestep, np.int64), 0, sac.size - 1)
    tp = np.maximum(t - 1, 0)
    a, ap = sac[t][:, None, None, None], sac[tp][:, None, None, None]
    x0, nz = np.asarray(x0_pred, np.float64), np.asarray(noisy, np.float64)
    x = ap * x0 + ((1.0 - ap) / ((1.0 - a) + EPS)) * (nz - a * x0)
    return np.clip(x, -1.0, 1.0), tp.astype(np.float64)


# ---- the input recipe: ties and seams exact in fp32 ---------------------------------------------------------------------------------
def make_case(shape, seed, edge_pair=False):
    """fp32 arrays pred, target, ema (B, C, H, W), depth (B, 1, H, W), g_terms (4,).

    pred, target, ema: 0.5 randn rounded to multiples of 2^-8; target equals pred at every fifth element (sgn = 0 occurs), ema equals
    pred at every seventh, and pred[x + 1] = pred[x] / pred[y + 1] = pred[y] at every eleventh / thirteenth position that has such a
    neighbour.  depth: a ramp of 2^-9 per pixel along x and y (restarting every 128 pixels), a step of 0.2 at mid-width, integer noise in [-4, 4] times 2^-10,
    clamped to [0, 1]: the Laplacian straddles the 0.01 threshold and a share of the differences are boundaries.  edge_pair: one
    x-pair and one y-pair of depths is (0, 0.01f) -- a difference EQUAL to the boundary threshold, which is not a boundary."""
    rs = np.random.RandomState(seed)
    Bn, C, H, W = shape
    grid = lambda v: (np.round(v * 256.0) / 256.0).astype(np.float32)
    pred, target, ema = (grid(0.5 * rs.randn(*shape)) for _ in range(3))
    flat = pred.reshape(-1)
    target.reshape(-1)[::5] = flat[::5]
    ema.reshape(-1)[2::7] = flat[2::7]
    if W > 1:
        idx = np.arange(3, flat.size - 1, 11)
        idx = idx[idx % W != W - 1]
        flat[idx + 1] = flat[idx]
    if H > 1:
        idx = np.arange(5, flat.size - W, 13)
        idx = idx[(idx // W) % H != H - 1]
        flat[idx + W] = flat[idx]
    yy, xx = np.mgrid[0:H, 0:W]
    depth = ((xx + yy) % 128) * 2.0 ** -9 + 0.2 * (xx >= W // 2) + 0.25
    depth = depth[None, None] + rs.randint(-4, 5, size=(Bn, 1, H, W)) * 2.0 ** -10
    depth = np.clip(depth, 0.0, 1.0).astype(np.float32)
    if edge_pair and H >= 3 and W >= 3:
        depth[0, 0, 1, 0], depth[0, 0, 1, 1] = 0.0, np.float32(0.01)
        depth[-1, 0, H - 2, W - 1], depth[-1, 0, H - 1, W - 1] = np.float32(0.01), 0.0
    g_terms = (0.5 + rs.rand(4)).astype(np.float32) * np.array([1, -1, 1, 1], np.float32)
    return dict(pred=pred, target=target, ema=ema, depth=depth, g_terms=g_terms)
