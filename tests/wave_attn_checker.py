"""A literal torch restatement of the fused wave self-attention's definition (include/fgs.h, fgs_wave_attn_*), for any dtype and
device.  Not a test: tests/test_wave_attn_checker.py holds it against the reference's fixtures W1 and W2,
tests/test_hip_wave_attn.py holds the kernels against it.

    attend(qkv, grid, wavelength, num_heads, wrong=None)
        qkv (B, N, 3 H d) or (B, N, 3, H, d), grid = (grid_h, grid_w), wavelength a one-element tensor -> (B, N, H d);
        differentiable in qkv and wavelength.  Every operation of the bias chain is one torch operation in qkv's dtype, in the
        header's order.  wrong: one rule got wrong on purpose (WRONG_RULES) -- what the fixtures must be able to tell.
    scores(qkv, grid, wavelength, num_heads) -> (B, H, N, N), the logits (for tests that need to know them).
"""
import torch

WRONG_RULES = ("qkv_head_major", "grid_transposed", "width_in_denominator", "amplitude_one", "bias_scaled", "no_bias")


def bias(grid, wavelength, dtype, device, wrong=None):
    """(N, N): 0.1 cos(phi) between token n = y grid_w + x and token m."""
    gh, gw = grid
    n = torch.arange(gh * gw, device=device)
    if wrong == "grid_transposed":      # token n at y = n % grid_h, x = n // grid_h
        y, x = n % gh, n // gh
    else:
        y, x = n // gw, n % gw
    dy = (y.unsqueeze(0) - y.unsqueeze(1)).to(dtype)
    dx = (x.unsqueeze(0) - x.unsqueeze(1)).to(dtype)
    dist = torch.sqrt((dy * dy + dx * dx) + 1e-8)
    den = wavelength.abs().reshape(()) * float(gw if wrong == "width_in_denominator" else gh) + 1e-6
    two_pi = torch.tensor(6.283185307179586, dtype=dtype, device=device)   # 6.2831855f in fp32
    phi = (two_pi * dist) / den
    return (1.0 if wrong == "amplitude_one" else 0.1) * torch.cos(phi)


def _split(qkv, num_heads, wrong=None):
    Bn, N = qkv.shape[:2]
    d = qkv[0, 0].numel() // 3 // num_heads
    if wrong == "qkv_head_major":       # (heads, 3, d) instead of (3, heads, d)
        return qkv.reshape(Bn, N, num_heads, 3, d).permute(3, 0, 2, 1, 4), d
    return qkv.reshape(Bn, N, 3, num_heads, d).permute(2, 0, 3, 1, 4), d


def scores(qkv, grid, wavelength, num_heads, wrong=None):
    (q, k, _), d = _split(qkv, num_heads, wrong)
    s = q @ k.transpose(-2, -1)
    if wrong == "no_bias":
        return s * d ** -0.5
    b = bias(grid, wavelength.to(qkv.dtype), qkv.dtype, qkv.device, wrong)
    if wrong == "bias_scaled":          # the bias added before the scaling
        return (s + b) * d ** -0.5
    return s * d ** -0.5 + b


def attend(qkv, grid, wavelength, num_heads, wrong=None):
    assert wrong is None or wrong in WRONG_RULES, wrong
    assert grid[0] * grid[1] == qkv.shape[1]
    Bn, N = qkv.shape[:2]
    (_, _, v), d = _split(qkv, num_heads, wrong)
    s = scores(qkv, grid, wavelength, num_heads, wrong)
    p = torch.softmax(s, dim=-1)
    return (p @ v).transpose(1, 2).reshape(Bn, N, num_heads * d)
