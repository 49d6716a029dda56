"""The attention block of the consistency view synthesizer (scripts/models/consistency_view_synthesis.py, "CVS").

`GroupNorm32`, `CrossAttention`, `FresnelWaveAttention` and `AttentionBlock` mirror the reference's classes of the same names:
constructor arguments and defaults, module tree, parameter names and returned tensors are the reference's, so its state dicts load
with strict=True.  The rest of the U-Net (ResBlock, sampling, pose encoder, the synthesizer and its losses) is not here.

The attention between FresnelWaveAttention's Linear layers is `fresnel_wave_attention`: self-attention over the H x W tokens of a
feature map with the interference term 0.1 cos(2 pi dist / (|wavelength| H + 1e-6)) added to the logits.  backend "torch" is the
reference's op sequence, which stores the (N, N) distances, phases and cosines and two (B, heads, N, N) tensors; backend "hip" is the
fused, flash-style kernel set of csrc/fgs_wave_attn.hip (definition: include/fgs.h, fgs_wave_attn_*): the packed `to_qkv` output is
read in place, the bias comes from a table of H W floats in LDS, nothing of size N x N is stored, and dL/d wavelength is a
deterministic reduction.  CUDA/ROCm tensors only, no fallback.

The CVS `CrossAttention` with backend "hip" needs no kernel of its own: its keys and values, projected by the concatenated
to_k / to_v weights, have exactly the layout `fresnel_amd.slat.cross_attention(backend="hip")` reads (csrc/fgs_attn.hip).

Every attention module has a `backend` attribute, "torch" by default; `AttentionBlock(..., attn_backend="hip")` sets both.
"""
import math
from typing import Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _binding as B
from . import _hip as hip
from .slat import cross_attention

ATTN_BACKENDS = ("torch", "hip")
_f32c = hip.f32c


def _check_attn_backend(attn_backend):
    if attn_backend not in ATTN_BACKENDS:
        raise ValueError(f"unknown attn_backend {attn_backend!r}: one of {ATTN_BACKENDS}")
    return attn_backend


def _wave_attention_torch(qkv, grid, wavelength, num_heads):
    """The reference's op sequence between `to_qkv` and `to_out` (CVS:215-243)."""
    Bn, N, C3 = qkv.shape
    H, W = grid
    d = C3 // 3 // num_heads
    q, k, v = map(lambda t: t.view(Bn, -1, num_heads, d).transpose(1, 2), qkv.chunk(3, dim=-1))
    dots = torch.matmul(q, k.transpose(-1, -2)) * d ** -0.5
    positions = torch.stack(torch.meshgrid(torch.arange(H, device=qkv.device), torch.arange(W, device=qkv.device), indexing='ij'),
                            dim=-1).float().view(-1, 2)
    pos_diff = positions.unsqueeze(0) - positions.unsqueeze(1)
    distances = torch.sqrt((pos_diff ** 2).sum(-1) + 1e-8)
    phase = 2 * math.pi * distances / (wavelength.abs() * H + 1e-6)
    interference = torch.cos(phase)
    dots = dots + interference.unsqueeze(0).unsqueeze(0) * 0.1
    attn = F.softmax(dots, dim=-1)
    out = torch.matmul(attn, v)
    return out.transpose(1, 2).reshape(Bn, -1, num_heads * d)


class _WaveAttnHip(torch.autograd.Function):
    """fgs_wave_attn_forward / _backward.  Saved: qkv, the wavelength, the output and one float per (b, h, n).  Nothing synchronises
    with the host; the wavelength is read on the device."""

    @staticmethod
    def forward(ctx, qkv, wavelength, grid, num_heads):
        dev = qkv.device
        Bn, N, C3 = qkv.shape
        C = C3 // 3
        dims = (Bn, grid[0], grid[1], num_heads, C // num_heads)
        scale = float((C // num_heads) ** -0.5)
        qkv_, wl_ = _f32c(qkv), _f32c(wavelength)
        saved_bytes, _ = B.sizes("fgs_wave_attn_workspace_bytes", *dims)
        out = torch.empty((Bn, N, C), dtype=torch.float32, device=dev)
        saved = torch.empty(saved_bytes, dtype=torch.uint8, device=dev)
        hip.call(dev, "fgs_wave_attn_forward", *dims, scale, qkv_, wl_, out, saved)
        ctx.dims, ctx.scale = dims, scale
        ctx.save_for_backward(qkv_, wl_, out, saved)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        qkv_, wl_, out, saved = ctx.saved_tensors
        dev = qkv_.device
        g_qkv = torch.empty_like(qkv_)
        g_wl = torch.empty_like(wl_) if ctx.needs_input_grad[1] else None
        _, scratch_bytes = B.sizes("fgs_wave_attn_workspace_bytes", *ctx.dims)
        scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        hip.call(dev, "fgs_wave_attn_backward", *ctx.dims, ctx.scale, qkv_, wl_, out, saved, _f32c(g_out), g_qkv, g_wl, scratch)
        return g_qkv, g_wl, None, None


def fresnel_wave_attention(qkv: torch.Tensor, grid: Tuple[int, int], wavelength: torch.Tensor, num_heads: int, *,
                           backend: str = "torch") -> torch.Tensor:
    """The attention of the reference's FresnelWaveAttention between its Linear layers (CVS:215-243): qkv (B, N, 3 C), the output of
    `to_qkv` (queries, keys, values in thirds of the last axis, each (heads, d)); grid = (H, W) with H W == N, token n at y = n // W,
    x = n % W; wavelength a one-element tensor -> (B, N, C), ready for `to_out`.  Scores d^-0.5 <q, k> + 0.1 cos(2 pi dist /
    (|wavelength| H + 1e-6)), dist = sqrt(dy^2 + dx^2 + 1e-8); softmax; no mask, no dropout, no NaN cleaning.

    backend "torch": the reference's op sequence, any device.  backend "hip": csrc/fgs_wave_attn.hip -- one launch forward, four
    backward, fp32 on the matrix cores, the bias from a table in LDS, nothing of size N x N stored, bitwise repeatable, the
    wavelength read on the device; CUDA/ROCm tensors only, d <= 128, H W <= 4096, inputs cast to fp32 under autocast, no double
    backward."""
    _check_attn_backend(backend)
    if isinstance(num_heads, bool) or int(num_heads) != num_heads or num_heads < 1:
        raise ValueError(f"num_heads must be a positive integer, got {num_heads!r}")
    num_heads = int(num_heads)
    if qkv.dim() != 3 or qkv.shape[-1] % (3 * num_heads) or 0 in qkv.shape:
        raise ValueError(f"qkv must be (B, N, 3 C) with C a multiple of num_heads = {num_heads} and no empty axis, got {tuple(qkv.shape)}")
    Bn, N, C3 = qkv.shape
    try:
        H, W = (int(s) for s in grid)
    except (TypeError, ValueError):
        raise ValueError(f"grid must be a pair (H, W), got {grid!r}") from None
    if H < 1 or W < 1 or H * W != N:
        raise ValueError(f"grid {H} x {W} does not hold the N = {N} tokens of qkv")
    if not torch.is_tensor(wavelength) or wavelength.numel() != 1:
        raise ValueError("wavelength must be a one-element tensor")
    if backend == "torch":
        return _wave_attention_torch(qkv, (H, W), wavelength, num_heads)
    who = "fresnel_wave_attention (backend 'hip')"
    d = C3 // 3 // num_heads
    if d > B.FGS_ATTN_MAX_HEAD_DIM:
        raise ValueError(f"{who}: head dimension {d} > {B.FGS_ATTN_MAX_HEAD_DIM} is not supported")
    if N > B.FGS_WAVE_ATTN_MAX_TOKENS:
        raise ValueError(f"{who}: a grid of {H} x {W} tokens is beyond the supported {B.FGS_WAVE_ATTN_MAX_TOKENS}")
    if Bn * num_heads * N >= 2 ** 31:
        raise ValueError(f"{who}: B x H x N = {Bn} x {num_heads} x {N} is beyond the supported size")
    if not qkv.is_contiguous():
        raise ValueError(f"{who}: qkv must be contiguous -- the Linear layer's output as it is, not a permuted view")
    for t in (qkv, wavelength):
        hip.need_cuda(t, who)
        if t.device != qkv.device:
            raise B.FgsError(f"{who}: tensors on {t.device} and {qkv.device}")
    return _WaveAttnHip.apply(qkv, wavelength, (H, W), num_heads)


# ---- the modules ------------------------------------------------------------------------------------------------------------------
class GroupNorm32(nn.GroupNorm):
    """GroupNorm computed in float32 (CVS:83-87)."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return super().forward(x.float()).type(x.dtype)


class CrossAttention(nn.Module):
    """Cross-attention of a feature map x (B, C, H, W) to `context` (B, M, context_dim) (CVS:137-188).  `backend` (an attribute,
    "torch" as in the reference): "hip" projects keys and values with the concatenated to_k / to_v weights -- (B, M, 2, heads,
    dim_head), the layout `slat.cross_attention(backend="hip")` reads -- and runs ONE fused call; autograd routes the weight gradients
    back through the concatenation.  (That kernel's NaN rule, include/fgs.h, applies: a row with non-finite scores attends uniformly
    where the reference gives NaN.)"""

    def __init__(self, query_dim: int, context_dim: int, heads: int = 8, dim_head: int = 64):
        super().__init__()
        self.heads = heads
        self.dim_head = dim_head
        inner_dim = heads * dim_head
        self.to_q = nn.Linear(query_dim, inner_dim, bias=False)
        self.to_k = nn.Linear(context_dim, inner_dim, bias=False)
        self.to_v = nn.Linear(context_dim, inner_dim, bias=False)
        self.to_out = nn.Linear(inner_dim, query_dim)
        self.scale = dim_head ** -0.5
        self.backend = "torch"

    def forward(self, x: torch.Tensor, context: torch.Tensor) -> torch.Tensor:
        Bn, C, H, W = x.shape
        x_flat = x.view(Bn, C, -1).permute(0, 2, 1)
        q = self.to_q(x_flat)
        if _check_attn_backend(self.backend) == "hip":
            kv = F.linear(context, torch.cat([self.to_k.weight, self.to_v.weight]))
            out = cross_attention(q, kv.view(Bn, -1, 2, self.heads, self.dim_head), self.heads, backend="hip")
        else:
            k = self.to_k(context)
            v = self.to_v(context)
            q = q.view(Bn, -1, self.heads, self.dim_head).transpose(1, 2)
            k = k.view(Bn, -1, self.heads, self.dim_head).transpose(1, 2)
            v = v.view(Bn, -1, self.heads, self.dim_head).transpose(1, 2)
            attn = torch.matmul(q, k.transpose(-1, -2)) * self.scale
            attn = F.softmax(attn, dim=-1)
            out = torch.matmul(attn, v)
            out = out.transpose(1, 2).reshape(Bn, -1, self.heads * self.dim_head)
        out = self.to_out(out)
        return out.permute(0, 2, 1).view(Bn, C, H, W)


class FresnelWaveAttention(nn.Module):
    """Self-attention over the tokens of a feature map with a learnable-wavelength interference term on the logits (CVS:191-246).
    `backend` (an attribute, "torch" as in the reference): "hip" runs `fresnel_wave_attention(..., backend="hip")`, ONE fused call
    on the `to_qkv` output as it is."""

    def __init__(self, dim: int, heads: int = 8):
        super().__init__()
        self.heads = heads
        self.dim_head = dim // heads
        self.scale = self.dim_head ** -0.5
        self.to_qkv = nn.Linear(dim, dim * 3, bias=False)
        self.to_out = nn.Linear(dim, dim)
        self.wavelength = nn.Parameter(torch.tensor(0.1))
        self.backend = "torch"

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        Bn, C, H, W = x.shape
        x_flat = x.view(Bn, C, -1).permute(0, 2, 1)
        out = fresnel_wave_attention(self.to_qkv(x_flat), (H, W), self.wavelength, self.heads, backend=self.backend)
        out = self.to_out(out)
        return out.permute(0, 2, 1).view(Bn, C, H, W)


class AttentionBlock(nn.Module):
    """x + self_attn(norm1(x)), then x + cross_attn(norm2(x), context) (CVS:249-288).  `use_fresnel=False` makes the self-attention
    a CrossAttention of the feature map to its own tokens.  `attn_backend` sets the `backend` of both attention modules."""

    def __init__(self, channels: int, context_dim: int, use_fresnel: bool = True, attn_backend: str = "torch"):
        super().__init__()
        self.norm1 = GroupNorm32(32, channels)
        if use_fresnel:
            self.self_attn = FresnelWaveAttention(channels)
        else:
            self.self_attn = CrossAttention(channels, channels)
        self.norm2 = GroupNorm32(32, channels)
        self.cross_attn = CrossAttention(channels, context_dim)
        self.self_attn.backend = self.cross_attn.backend = _check_attn_backend(attn_backend)

    def forward(self, x: torch.Tensor, context: torch.Tensor) -> torch.Tensor:
        h = self.norm1(x)
        if isinstance(self.self_attn, FresnelWaveAttention):
            h = self.self_attn(h)
        else:
            h_flat = h.view(h.shape[0], h.shape[1], -1).permute(0, 2, 1)
            h = self.self_attn(h, h_flat)
        x = x + h
        h = self.norm2(x)
        h = self.cross_attn(h, context)
        x = x + h
        return x
