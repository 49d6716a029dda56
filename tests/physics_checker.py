"""The parameter head of the physics-phase decoder, restated from its formulas in plain torch (test infrastructure, like
head_checker.py; independent of fresnel_amd/decoder.py).  Runs in the dtype of `raw` -- fp32 or fp64 -- and is differentiated by
autograd.  Formulas (reference scripts/models/gaussian_decoder_models.py:1071-1147, scripts/utils/fresnel_zones.py:463-467, 553-575):

    positions  (base_x + g raw0, base_y + g raw1, base_z)            scales  softplus(raw + 1) 0.15 (linear above 20), NO clamps
    rotations  head_checker.quaternion                               colors, opacities  sigmoid
    phases     z = base_z of the patch;  u = (z - z_min) / ((z_max - z_min) + 1e-8), z_min / z_max over the whole (B, P);
               lambda = clamp(|wavelength_raw|, lambda_min, lambda_max), gradient on the closed interval, |.| with gradient 0 at 0;
               phase = wrap((2 pi / lambda) |u - focal_depth|)

`tie_rule`: how the gradient of z_min / z_max reaches elements that are tied for the extremum --
    "equal"  equal shares to all of them (torch's min() / max(); the rule)       "first"  all of it to the first one (a wrong rule)
`wrap_rule`: "mod" phase mod 2 pi (the rule) | "none" the unwrapped phase (a wrong rule: only equal modulo 2 pi)
"""
import math

import torch

from head_checker import branch_info, quaternion  # noqa: F401  (branch_info: re-used by the tests)

OUTPUTS = ("positions", "scales", "rotations", "colors", "opacities", "phases")
TIE_RULES = ("equal", "first")
WRAP_RULES = ("mod", "none")
TWO_PI = 2 * math.pi


class _Extremum(torch.autograd.Function):
    """min or max of a tensor whose gradient goes to the tied elements by `tie_rule`."""

    @staticmethod
    def forward(ctx, z, largest, tie_rule):
        v = z.max() if largest else z.min()
        mask = (z == v)
        if tie_rule == "first":
            first = torch.zeros_like(mask).flatten()
            first[int(mask.flatten().to(torch.uint8).argmax())] = True
            mask = first.view_as(mask)
        ctx.save_for_backward(mask)
        return v

    @staticmethod
    def backward(ctx, g):
        mask, = ctx.saved_tensors
        m = mask.to(g.dtype)
        return g * m / m.sum(), None, None


def circular_distance(a, b):
    """Distance of two phases on the circle: min(|d|, 2 pi - |d|) of d = (a - b) mod 2 pi, in fp64."""
    d = torch.remainder(a.double() - b.double(), TWO_PI)
    return torch.minimum(d, TWO_PI - d)


def phase_of(base_z, wavelength_raw, focal_depth=0.5, wavelength_min=0.01, wavelength_max=0.5, tie_rule="equal", wrap_rule="mod"):
    """base_z (B, P), wavelength_raw 0-dim, both in the dtype to compute in -> (B, P) phases"""
    assert tie_rule in TIE_RULES and wrap_rule in WRAP_RULES
    z_min, z_max = _Extremum.apply(base_z, False, tie_rule), _Extremum.apply(base_z, True, tie_rule)
    u = (base_z - z_min) / ((z_max - z_min) + 1e-8)
    lam = torch.clamp(torch.abs(wavelength_raw), wavelength_min, wavelength_max)
    phase = (TWO_PI / lam) * torch.abs(u - focal_depth)
    return torch.remainder(phase, TWO_PI) if wrap_rule == "mod" else phase


def head(raw, base_xy, base_z, wavelength_raw, num_gaussians=None, focal_depth=0.5, wavelength_min=0.01, wavelength_max=0.5,
         xy_gain=0.25, tie_rule="equal", wrap_rule="mod"):
    """raw (B,P,K_full,16) in the dtype to compute in; base_xy (P,2); base_z (B,P); wavelength_raw 0-dim.
    -> dict of OUTPUTS, (B, P K, .)"""
    Bn, P, KF, _ = raw.shape
    K = KF if num_gaussians is None else max(1, min(int(num_gaussians), KF))
    o = raw[:, :, :K]
    dt = raw.dtype
    bz = base_z.to(dt)
    x = base_xy.to(dt)[None, :, None, 0] + xy_gain * o[..., 0]
    y = base_xy.to(dt)[None, :, None, 1] + xy_gain * o[..., 1]
    z = bz[:, :, None].expand(Bn, P, K)
    u = o[..., 3:6] + 1
    scales = torch.where(u > 20, u, torch.log1p(torch.exp(torch.clamp(u, max=20)))) * 0.15
    phase = phase_of(bz, wavelength_raw.to(dt), focal_depth, wavelength_min, wavelength_max, tie_rule, wrap_rule)
    N = P * K
    return dict(positions=torch.stack([x, y, z], -1).reshape(Bn, N, 3), scales=scales.reshape(Bn, N, 3),
                rotations=quaternion(o[..., 6:12]).reshape(Bn, N, 4), colors=torch.sigmoid(o[..., 12:15]).reshape(Bn, N, 3),
                opacities=torch.sigmoid(o[..., 15]).reshape(Bn, N), phases=phase[:, :, None].expand(Bn, P, K).reshape(Bn, N))


def formula_upstream(shape, salt):
    """A reproducible upstream gradient in (0, 1): 0.5 + 0.49 cos(0.7548776662 i + salt) over the flat index i, formed in fp64 and
    rounded to fp32 (fixtures too large to store their upstream gradients name this formula instead)."""
    n = int(torch.tensor(shape).prod()) if len(shape) else 1
    i = torch.arange(n, dtype=torch.float64)
    return (0.5 + 0.49 * torch.cos(0.7548776662 * i + float(salt))).to(torch.float32).reshape(shape)
