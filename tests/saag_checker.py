"""The two non-GEMM stages of the SAAG refinement decoder, restated from their formulas in plain torch (test infrastructure, like
head_checker.py; independent of fresnel_amd/decoder.py).  Runs in the dtype it is asked for -- fp32 or fp64 -- and is differentiated
by autograd.  Formulas (reference scripts/models/gaussian_decoder_models.py:489-570 and F.grid_sample(bilinear, border,
align_corners=False)):

    inputs     u = clamp((x / max(z, 0.1) + 2) / 4, 0, 1), v from y;  ix = clip(u W - 0.5, 0, W - 1), iy = clip(v H - 0.5, 0, H - 1);
               x0 = floor(ix), weights (x0 + 1 - ix, ix - x0) x (y0 + 1 - iy, iy - y0); a corner outside the grid contributes
               nothing (a hand-written gather, not grid_sample);  row = [C features | position | scale | rotation | colour | opacity]
    deltas     raw x gain x residual_scale             positions  saag + delta         scales  saag exp(delta)
    rotations  n(q_delta (x) q_saag), q_delta = head_checker.quaternion(raw[6:12]), (x) the Hamilton product, n(p) = p / max(|p|, 1e-12)
    colors, opacities   clamp(saag + delta, 0, 1), gradient on the closed interval

`rules` switches ONE rule to a plausible wrong one (tests/test_saag_mirror.py shows that the GPU tests' seam inputs tell them apart):
    "no_half_pixel"  ix = u W            "swap_xy"  x indexes the height       "no_border_clip"  ix is not clipped to [0, W - 1]
    "open_gate"      the clamps pass the gradient on the OPEN interval          "product_order"   q_saag (x) q_delta
"""
import torch

from head_checker import branch_info, quaternion  # noqa: F401  (branch_info: re-used by the tests)

OUTPUTS = ("positions", "scales", "rotations", "colors", "opacities", "pos_delta", "scale_delta", "color_delta", "opacity_delta")
RULES = ("no_half_pixel", "swap_xy", "no_border_clip", "open_gate", "product_order")


def sample_coords(positions, H, W, rules=()):
    """-> ix, iy (B, N): continuous texel coordinates along the grid's width and height."""
    z = positions[..., 2].clamp(min=0.1)
    u = ((positions[..., 0] / z + 2) / 4).clamp(0, 1)
    v = ((positions[..., 1] / z + 2) / 4).clamp(0, 1)
    if "swap_xy" in rules:
        u, v = v, u
    off = 0.0 if "no_half_pixel" in rules else 0.5
    ix, iy = u * W - off, v * H - off
    if "no_border_clip" not in rules:
        ix, iy = ix.clamp(0, W - 1), iy.clamp(0, H - 1)
    return ix, iy


def mlp_inputs(features, positions, scales, rotations, colors, opacities, dtype=torch.float64, rules=()):
    """features (B, C, H, W) in any memory layout -> (B, N, C + 14)"""
    f, p = features.to(dtype), positions.to(dtype)
    Bn, C, H, W = f.shape
    ix, iy = sample_coords(p, H, W, rules)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    wx, wy = (x0 + 1 - ix, ix - x0), (y0 + 1 - iy, iy - y0)
    flat = f.reshape(Bn, C, H * W)
    out = torch.zeros(Bn, p.shape[1], C, dtype=dtype, device=f.device)
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0.long() + dx, y0.long() + dy
            inside = ((xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)).to(dtype)
            idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).unsqueeze(1).expand(-1, C, -1)   # (B, C, N)
            texel = torch.gather(flat, 2, idx).permute(0, 2, 1)                                     # (B, N, C)
            out = out + texel * (wx[dx] * wy[dy] * inside).unsqueeze(-1)
    return torch.cat([out, p, scales.to(dtype), rotations.to(dtype), colors.to(dtype), opacities.to(dtype).unsqueeze(-1)], dim=-1)


def quat_mul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


class _ClampOpen(torch.autograd.Function):
    """clamp(x, 0, 1) whose backward passes the gradient on the OPEN interval (the wrong rule "open_gate")."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return x.clamp(0, 1)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return g * ((x > 0) & (x < 1)).to(g.dtype)


def refine(raw, positions, scales, rotations, colors, opacities, gains, residual_scale=0.1, rules=()):
    """raw (B, N, 16) in the dtype to compute in; gains (4,) -> dict of OUTPUTS"""
    dt = raw.dtype
    p, s, q, c, o, g = (t.to(dt) for t in (positions, scales, rotations, colors, opacities, gains))
    pd, sd = raw[..., 0:3] * g[0] * residual_scale, raw[..., 3:6] * g[1] * residual_scale
    cd, od = raw[..., 12:15] * g[2] * residual_scale, raw[..., 15:16] * g[3] * residual_scale
    qd = quaternion(raw[..., 6:12])
    prod = quat_mul(q, qd) if "product_order" in rules else quat_mul(qd, q)
    rot = prod / torch.linalg.vector_norm(prod, dim=-1, keepdim=True).clamp(min=1e-12)
    clamp = _ClampOpen.apply if "open_gate" in rules else (lambda t: t.clamp(0, 1))
    return dict(positions=p + pd, scales=s * torch.exp(sd), rotations=rot, colors=clamp(c + cd), opacities=clamp(o + od.squeeze(-1)),
                pos_delta=pd, scale_delta=sd, color_delta=cd, opacity_delta=od)
