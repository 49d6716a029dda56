"""A literal torch restatement of the fused GroupNorm -> SiLU's definition (include/fgs.h, fgs_gn_silu_*), for any dtype and device.
Not a test: tests/test_gn_checker.py holds it against torch's op sequence add -> F.group_norm -> F.silu, tests/test_hip_gn_silu.py
holds the kernels against it.  The backward is the definition's too, written out (`backward`), not autograd's.

`wrong=` makes one deliberate mistake, so that the tests can show their cases tell them apart:
    unbiased_var      the variance divided by m - 1
    eps_outside       rstd = 1 / (sqrt(var) + eps)
    bias_after_norm   channel_bias added to the normalised value instead of to x
    silu_grad_short   SiLU's derivative without the y (1 - s) term (backward only)
    strided_groups    group g holds the channels g, g + groups, g + 2 groups, ... instead of cpg adjacent ones
"""
import torch

WRONG_RULES = ("unbiased_var", "eps_outside", "bias_after_norm", "silu_grad_short", "strided_groups")


def _grouped(t, groups, wrong):
    """(B, C, HW) -> (B, groups, cpg, HW), the group's channels along axis 2."""
    Bn, C, HW = t.shape
    if wrong == "strided_groups":
        return t.view(Bn, C // groups, groups, HW).transpose(1, 2)
    return t.view(Bn, groups, C // groups, HW)


def _ungrouped(t, wrong):
    Bn, G, cpg, HW = t.shape
    if wrong == "strided_groups":
        return t.transpose(1, 2).reshape(Bn, G * cpg, HW)
    return t.reshape(Bn, G * cpg, HW)


def _parts(x, groups, weight, bias, channel_bias, eps, wrong):
    assert wrong is None or wrong in WRONG_RULES, wrong
    Bn, C = x.shape[:2]
    x3 = x.reshape(Bn, C, -1)
    u = x3 if channel_bias is None or wrong == "bias_after_norm" else x3 + channel_bias[:, :, None]
    ug = _grouped(u, groups, wrong)
    m = ug.shape[2] * ug.shape[3]
    mean = ug.sum(dim=(2, 3), keepdim=True) / m
    var = ((ug - mean) ** 2).sum(dim=(2, 3), keepdim=True) / (m - 1 if wrong == "unbiased_var" else m)
    rstd = 1.0 / (torch.sqrt(var) + eps) if wrong == "eps_outside" else 1.0 / torch.sqrt(var + eps)
    xhat = _ungrouped((ug - mean) * rstd, wrong)
    if channel_bias is not None and wrong == "bias_after_norm":
        xhat = xhat + channel_bias[:, :, None]
    y = weight[None, :, None] * xhat + bias[None, :, None]
    return xhat, y, rstd, m


def forward(x, groups, weight, bias, channel_bias=None, act=1, eps=1e-5, wrong=None):
    """x (B, C, ...), weight, bias (C,), channel_bias (B, C) or None -> out, x's shape."""
    _, y, _, _ = _parts(x, groups, weight, bias, channel_bias, eps, wrong)
    return (y * torch.sigmoid(y) if act else y).reshape(x.shape)


def backward(x, groups, weight, bias, g_out, channel_bias=None, act=1, eps=1e-5, wrong=None):
    """-> dict(g_x, g_channel_bias (None without channel_bias), g_weight, g_bias), the definition's formulas."""
    Bn, C = x.shape[:2]
    xhat, y, rstd, m = _parts(x, groups, weight, bias, channel_bias, eps, wrong)
    g3 = g_out.reshape(Bn, C, -1)
    if act:
        s = torch.sigmoid(y)
        g_y = g3 * s * (1 + (0 if wrong == "silu_grad_short" else y * (1 - s)))
    else:
        g_y = g3
    wg = weight[None, :, None] * g_y
    mean1 = _grouped(wg, groups, wrong).sum(dim=(2, 3), keepdim=True) / m
    mean2 = _grouped(wg * xhat, groups, wrong).sum(dim=(2, 3), keepdim=True) / m
    g_u = _ungrouped(rstd * (_grouped(wg, groups, wrong) - mean1 - _grouped(xhat, groups, wrong) * mean2), wrong)
    return dict(g_x=g_u.reshape(x.shape), g_channel_bias=None if channel_bias is None else g_u.sum(dim=2),
                g_weight=(g_y * xhat).sum(dim=(0, 2)), g_bias=g_y.sum(dim=(0, 2)))


def op_sequence(x, groups, weight, bias, channel_bias=None, act=1, eps=1e-5):
    """torch's own ops, in the reference's order: the broadcast add, F.group_norm, F.silu."""
    u = x if channel_bias is None else x + channel_bias[(..., *([None] * (x.dim() - 2)))]
    y = torch.nn.functional.group_norm(u, groups, weight, bias, eps)
    return torch.nn.functional.silu(y) if act else y
