"""Checker of the per-pixel losses (tests/test_pixel_loss.py): the per-pixel part of the reference's compute_losses
(TGD:873-953) restated in plain torch, in the dtype of its inputs (the tests run it in fp64, and in fp32 against the
fixture G17, which the reference's own code produced), and the closed-form gradients the HIP backward implements."""
import torch
import torch.nn.functional as F


def boundary_table(num_zones=8, depth_range=(0.0, 1.0)):
    """FresnelZones' zone_boundaries buffer: built in fp32 (fresnel_zones.py:80-83)."""
    return torch.linspace(depth_range[0], depth_range[1], num_zones + 1)


def boundary_mask(depth, num_zones=8, depth_range=(0.0, 1.0), threshold=0.02, soft=True):
    """FresnelZones.compute_boundary_mask (fresnel_zones.py:160-180)."""
    b = boundary_table(num_zones, depth_range).to(depth.dtype)
    md = (depth.unsqueeze(-1) - b).abs().min(dim=-1)[0]
    if soft:
        return torch.sigmoid((10.0 / threshold) * (threshold - md))
    return (md < threshold).to(depth.dtype)


def density_weight(density, vlm_weight, size, dtype):
    """(1 - vlm_weight) + vlm_weight * density, the map resized like TGD:881-885 (in fp32, as the product resizes it)."""
    if density.shape[-2:] != tuple(size):
        density = F.interpolate(density.float(), size=tuple(size), mode="bilinear", align_corners=False)
    return (1.0 - vlm_weight) + vlm_weight * density.to(dtype)


def normalise(x, mean=None, std=None):
    """(x - mean) / clamp(std, 1e-4) with torch's unbiased std (TGD:924-927); mean / std given: those of a larger batch."""
    mean = x.mean() if mean is None else mean
    std = x.std() if std is None else std
    return (x - mean) / torch.clamp(std, min=1e-4)


def ref_pixel_losses(rendered, target, rendered_depth=None, target_depth=None, density=None, vlm_weight=0.5, zones=None):
    """dict of the terms "rgb", "boundary" (with `zones` = dict(num_zones, depth_range, threshold, soft) and a target
    depth) and "depth" (with both depth maps)."""
    out = {}
    a = (rendered - target).abs()
    if density is not None and vlm_weight > 0:
        out["rgb"] = (a * density_weight(density, vlm_weight, rendered.shape[-2:], rendered.dtype)).mean()
    else:
        out["rgb"] = a.mean()
    if zones is not None and target_depth is not None:
        out["boundary"] = (a.mean(dim=1) * boundary_mask(target_depth, **zones)).mean()
    if rendered_depth is not None and target_depth is not None:
        out["depth"] = (normalise(rendered_depth) - normalise(target_depth)).abs().mean()
    return out


def sgn(a, b):
    """(a > b) - (a < b): 0 on a tie, by comparison (what torch.sign(a - b) gives when a - b is exact)."""
    return (a > b).to(a.dtype) - (a < b).to(a.dtype)


def closed_form_grads(rendered, target, rendered_depth, target_depth, w, mask, g_rgb, g_boundary, g_depth, glob=None):
    """The gradients fgs_pixel_loss_backward writes (include/fgs.h).  w: the rgb weight map (B,1,H,W) or None; mask: the
    boundary mask (B,H,W) or None.  glob = (N, mean_x, std_x, mean_y, std_y, SGN, SGN_U): the global batch's statistics
    and sign sums when this is one rank's shard; None: taken from this batch."""
    Bn, C, H, W = rendered.shape
    coef = torch.zeros(Bn, 1, H, W, dtype=rendered.dtype)
    if g_rgb is not None:
        coef = coef + g_rgb * (w if w is not None else 1.0)
    if g_boundary is not None and mask is not None:
        coef = coef + g_boundary * mask.unsqueeze(1)
    g_r = sgn(rendered, target) * coef / rendered.numel()
    if rendered_depth is None or g_depth is None:
        return g_r, None
    n_local = rendered_depth.numel()
    if glob is None:
        N, mx, sx, my, sy = n_local, rendered_depth.mean(), rendered_depth.std(), target_depth.mean(), target_depth.std()
    else:
        N, mx, sx, my, sy = glob[:5]
    s = torch.clamp(sx, min=1e-4)
    gate = (sx >= 1e-4).to(rendered.dtype)
    u = (rendered_depth - mx) / s
    v = (target_depth - my) / torch.clamp(sy, min=1e-4)
    sg = sgn(u, v)
    SGN, SGN_U = (sg.sum(), (sg * u).sum()) if glob is None else glob[5:]
    Q, P = SGN / n_local, SGN_U / n_local
    return g_r, g_depth * (sg / n_local - Q / N - gate * P * u / (N - 1)) / s
