"""CPU restatement of the GaussianMatchingLoss contract of include/fgs.h (fgs_match_*): the active rows, the canonical match
lists, the terms evaluated in float64 from float32 elements, and the gradient rows in the header's expression order (numpy
float32 arithmetic rounds every operation on its own and divides / takes roots IEEE, as the kernels' unit is compiled to do), so
that lists and gradient rows can be compared bit for bit.  The keyword switches are the mutations of tests/test_match_checker.py;
their defaults are the contract."""
import numpy as np

F = np.float32
TINY = F(1e-6)
QMIN = F(1e-8)
WEIGHTS = dict(position=10.0, scale=5.0, rotation=2.0, color=5.0, opacity=3.0, coverage=1.0)  # the reference's defaults
KEYS = ("position", "scale", "rotation", "color", "opacity", "coverage")                    # terms[:, 0:6]; [:, 6] is batch


def _w(weights):
    w = dict(WEIGHTS)
    w.update(weights or {})
    return {k: F(v) for k, v in w.items()}


def active(rows, keep=None, use_filter=True):
    """(..., N) bool: keep byte non-zero and (|x| + |y|) + |z| > 1e-6f or |opacity| > 1e-6f."""
    rows = np.asarray(rows, F)
    with np.errstate(all="ignore"):
        s = (np.abs(rows[..., 0]) + np.abs(rows[..., 1])) + np.abs(rows[..., 2])
        act = (s > TINY) | (np.abs(rows[..., 13]) > TINY)
    if not use_filter:
        act = np.ones_like(act)
    if keep is not None:
        act = act & (np.asarray(keep) != 0)
    return act


def d2_matrix(q, c):
    """(len(q), len(c)) float32: (dx dx + dy dy) + dz dz, NaN -> +inf."""
    with np.errstate(all="ignore"):
        d = q[:, None, :].astype(F) - c[None, :, :].astype(F)
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    d2[np.isnan(d2)] = np.inf
    return d2


def _nearest(q, c, highest=False):
    out = np.empty(len(q), np.int64)
    for s in range(0, len(q), 256):
        d2 = d2_matrix(q[s:s + 256], c)
        out[s:s + 256] = (len(c) - 1 - np.argmin(d2[:, ::-1], axis=1)) if highest else np.argmin(d2, axis=1)
    return out


def matches(pred, target, pred_keep=None, target_keep=None, highest_wins=False, use_filter=True):
    """-> fwd (B, Np) int32, bwd (B, Nt) int32, counts (B, 2) int32."""
    pred, target = np.asarray(pred, F), np.asarray(target, F)
    B, Np, Nt = pred.shape[0], pred.shape[1], target.shape[1]
    fwd, bwd = np.full((B, Np), -1, np.int32), np.full((B, Nt), -1, np.int32)
    counts = np.zeros((B, 2), np.int32)
    for b in range(B):
        ip = np.nonzero(active(pred[b], None if pred_keep is None else pred_keep[b], use_filter))[0]
        it = np.nonzero(active(target[b], None if target_keep is None else target_keep[b], use_filter))[0]
        counts[b] = (len(ip), len(it))
        if len(ip) == 0 or len(it) == 0:
            continue
        fwd[b, ip] = it[_nearest(pred[b, ip, :3], target[b, it, :3], highest_wins)]
        bwd[b, it] = ip[_nearest(target[b, it, :3], pred[b, ip, :3], highest_wins)]
    return fwd, bwd, counts


def relative_gap(pred, target, pred_keep=None, target_keep=None):
    """The smallest (second - nearest) / second d2 over all active queries of both directions (float64 distances)."""
    pred, target = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    gap = np.inf
    for b in range(pred.shape[0]):
        ip = np.nonzero(active(pred[b], None if pred_keep is None else pred_keep[b]))[0]
        it = np.nonzero(active(target[b], None if target_keep is None else target_keep[b]))[0]
        for q, c in ((pred[b, ip, :3], target[b, it, :3]), (target[b, it, :3], pred[b, ip, :3])):
            if len(q) == 0 or len(c) < 2:
                continue
            d2 = np.sort(((q[:, None, :] - c[None, :, :]) ** 2).sum(-1), axis=1)
            gap = min(gap, float(((d2[:, 1] - d2[:, 0]) / d2[:, 1]).min()))
    return gap


def _clamped_norm(q):
    with np.errstate(all="ignore"):
        n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        return n, np.where(n < QMIN, QMIN, n).astype(F)


def _unit_dot(a, b, ca, cb):
    with np.errstate(all="ignore"):
        return (((a[:, 0] / ca) * (b[:, 0] / cb) + (a[:, 1] / ca) * (b[:, 1] / cb)) + (a[:, 2] / ca) * (b[:, 2] / cb)) + (a[:, 3] / ca) * (b[:, 3] / cb)


def _msq(a, b, cols):
    with np.errstate(all="ignore"):
        d = a[:, cols] - b[:, cols]
        return (d * d).astype(np.float64).sum() / (d.shape[0] * d.shape[1])


def terms(pred, target, fwd, bwd, counts, weights=None):
    """(B, 8) float64: position, scale, rotation, colour, opacity, coverage, batch, 0 -- float32 elements, float64 sums."""
    pred, target = np.asarray(pred, F), np.asarray(target, F)
    w = {k: np.float64(v) for k, v in _w(weights).items()}
    out = np.zeros((pred.shape[0], 8), np.float64)
    P, S, C, O = slice(0, 3), slice(3, 6), slice(10, 13), slice(13, 14)
    for b in range(pred.shape[0]):
        if counts[b, 0] == 0 or counts[b, 1] == 0:
            continue
        i = np.nonzero(fwd[b] >= 0)[0]
        p, t = pred[b, i], target[b, fwd[b, i]]
        pos, scale, color, opacity = _msq(p, t, P), _msq(p, t, S), _msq(p, t, C), _msq(p, t, O)
        dot = _unit_dot(p[:, 6:10], t[:, 6:10], _clamped_norm(p[:, 6:10])[1], _clamped_norm(t[:, 6:10])[1])
        rot = 1.0 - np.abs(dot).astype(np.float64).sum() / len(i)
        j = np.nonzero(bwd[b] >= 0)[0]
        t, p = target[b, j], pred[b, bwd[b, j]]
        cov = ((2.0 * _msq(t, p, P) + 0.5 * _msq(t, p, S)) + 0.5 * _msq(t, p, C)) + 2.0 * _msq(t, p, O)
        batch = ((((w["position"] * pos + w["scale"] * scale) + w["rotation"] * rot) + w["color"] * color) + w["opacity"] * opacity) + w["coverage"] * cov
        out[b, :7] = (pos, scale, rot, color, opacity, cov, batch)
    return out


def total(terms_, counts=None, by_non_skipped=False):
    """sum_b batch_b / B (float64); `by_non_skipped`: the mutation that divides by the images that were not skipped."""
    n = terms_.shape[0]
    if by_non_skipped:
        n = max(1, int(((counts[:, 0] > 0) & (counts[:, 1] > 0)).sum()))
    return np.asarray(terms_, np.float64)[:, 6].sum() / n


def grad_rows(pred, target, fwd, bwd, counts, weights=None, g_total=1.0, coverage_grad=True, by_non_skipped=False):
    """(B, Np, 14) float32: d(g_total x total) / dpred in the header's expression order."""
    pred, target = np.asarray(pred, F), np.asarray(target, F)
    w = _w(weights)
    B, Np = pred.shape[:2]
    n_img = B if not by_non_skipped else max(1, int(((counts[:, 0] > 0) & (counts[:, 1] > 0)).sum()))
    g = np.zeros((B, Np, 14), F)
    groups = (("position", slice(0, 3), 3, F(2.0)), ("scale", slice(3, 6), 3, F(0.5)), ("color", slice(10, 13), 3, F(0.5)),
              ("opacity", slice(13, 14), 1, F(2.0)))
    with np.errstate(all="ignore"):
        gs = F(g_total) * (F(1.0) / F(n_img))
        for b in range(B):
            n_p, n_t = int(counts[b, 0]), int(counts[b, 1])
            if n_p == 0 or n_t == 0:
                continue
            a = {3: F(2.0) / F(3 * n_p), 1: F(2.0) / F(n_p)}
            c = {3: F(2.0) / F(3 * n_t), 1: F(2.0) / F(n_t)}
            r1 = F(1.0) / F(n_p)
            gc = gs * w["coverage"]
            i = np.nonzero(fwd[b] >= 0)[0]
            p, t = pred[b, i], target[b, fwd[b, i]]
            row = np.zeros((len(i), 14), F)
            for name, cols, width, _ in groups:
                row[:, cols] = ((gs * w[name]) * a[width]) * (p[:, cols] - t[:, cols])
            qp, qt = p[:, 6:10], t[:, 6:10]
            n, cp = _clamped_norm(qp)
            ct = _clamped_norm(qt)[1]
            dot = _unit_dot(qp, qt, cp, ct)
            sgn = (dot > 0).astype(F) - (dot < 0).astype(F)
            e = -(((gs * w["rotation"]) * r1) * sgn)
            gh = e[:, None] * (qt / ct[:, None])
            u = ((gh[:, 0] * qp[:, 0] + gh[:, 1] * qp[:, 1]) + gh[:, 2] * qp[:, 2]) + gh[:, 3] * qp[:, 3]
            v = ((u / cp) / cp) / n
            through = gh / cp[:, None] - qp * v[:, None]
            row[:, 6:10] = np.where((n < QMIN)[:, None], gh / cp[:, None], through)
            g[b, i] = row
            if not coverage_grad:
                continue
            for j in np.nonzero(bwd[b] >= 0)[0]:  # ascending j
                m = bwd[b, j]
                for name, cols, width, k in groups:
                    g[b, m, cols] = g[b, m, cols] + ((gc * k) * c[width]) * (pred[b, m, cols] - target[b, j, cols])
    return g


def evaluate(pred, target, pred_keep=None, target_keep=None, weights=None, g_total=1.0, highest_wins=False, use_filter=True,
             coverage_grad=True, by_non_skipped=False):
    """Everything at once -> dict(fwd, bwd, counts, terms (B, 8) float64, total float64, grad (B, Np, 14) float32)."""
    fwd, bwd, counts = matches(pred, target, pred_keep, target_keep, highest_wins, use_filter)
    t = terms(pred, target, fwd, bwd, counts, weights)
    return dict(fwd=fwd, bwd=bwd, counts=counts, terms=t, total=total(t, counts, by_non_skipped),
                grad=grad_rows(pred, target, fwd, bwd, counts, weights, g_total, coverage_grad, by_non_skipped))
