"""The distillation decoders: what PRODUCES the cloud that GaussianMatchingLoss (fresnel_amd/losses.py) scores against a TRELLIS target.

`DirectSLatDecoder` and `MLPSLatDecoder` mirror the reference's classes of the same names (scripts/models/direct_slat_decoder.py,
"DSD") with everything they are built from -- `PositionalEncoding3D`, `CrossAttention` (with its chunked path), `SparseTransformerBlock`,
`OccupancyHead`, `GaussianHead`: constructor arguments and defaults, module tree, registration order and returned values are the
reference's, so its checkpoints load with strict=True.  Embeddings, attention and MLPs are torch modules; the Gaussian-parameter head
behind the head MLP is `slat_gaussian_head`: the reference's torch expressions (backend "torch", runs anywhere) or the fused HIP
kernels of csrc/fgs_slat.hip (backend "hip", CUDA/ROCm tensors only, no fallback).

The attention between CrossAttention's Linear layers is `cross_attention`: the reference's op sequence (backend "torch") or the fused,
flash-style HIP kernels of csrc/fgs_attn.hip (backend "hip": no score tensor, device-side dropout, bitwise repeatable); `DirectSLatDecoder`
selects it with `attn_backend`, independently of the head.  Under mixed precision the fused attention has a 16-bit form
(csrc/fgs_attn_half.hip: fp16 or bf16 tensors, fp32 scores and softmax), selected with `compute_dtype` / `attn_dtype`.

Both decoders take one extra keyword, `head_backend`.  With "torch" every host check of the reference stays (its
`isnan(...).any()` tests and the per-image loop of the occupancy-gated inference).  With "hip" nothing in a training forward reads
the host: the reference's conditional `nan_to_num` calls run unconditionally (the same values), the head applies the NaN rule of
include/fgs.h on the device, and the gated inference is one compacting launch pair and ONE host copy of the per-image counts.
"""
import ctypes
from typing import Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable
from torch.utils.checkpoint import checkpoint

from . import _binding as B
from . import _hip as hip

HEAD_BACKENDS = ("torch", "hip")
_f32c = hip.f32c


def _check_backend(head_backend):
    if head_backend not in HEAD_BACKENDS:
        raise ValueError(f"unknown head_backend {head_backend!r}: one of {HEAD_BACKENDS}")
    return head_backend


def _refuse_grad(backend_of, tensors):
    for name, t in tensors:
        if t.requires_grad and torch.is_grad_enabled():
            raise ValueError(f"{backend_of} with a keep mask is the inference path and produces no gradient for {name}; call it under "
                             "torch.no_grad(), or without `keep` to differentiate")


def _clean(x, host_checks, **kw):
    """The reference's `if isnan(x).any() [or isinf(x).any()]: x = nan_to_num(x, ...)`.  Without host checks the replacement runs
    unconditionally: the same values (it is the identity on clean data) and no synchronisation."""
    if not host_checks:
        return torch.nan_to_num(x, **kw)
    dirty = torch.isnan(x).any() or ("posinf" in kw and torch.isinf(x).any())
    return torch.nan_to_num(x, **kw) if dirty else x


# ---- the head ---------------------------------------------------------------------------------------------------------------------
def _slat_head_torch(raw, coords, position_offset_scale, scale_factor):
    """The reference's GaussianHead behind its MLP (DSD:318-358), restated: the same operations in the same order on raw (B, N, G, 14),
    the host's look for NaN and nan_to_num included; the five groups are concatenated where the reference assigns slices."""
    Bn, N, G, _ = raw.shape
    r = raw.clamp(-10.0, 10.0)
    centre = (coords[:, :, 1:4].float().clamp(0, 63) / 64.0 * 2 - 1).unsqueeze(2).expand(-1, -1, G, -1)
    position = (centre + torch.tanh(r[..., :3]) * position_offset_scale).clamp(-1.0, 1.0)
    scale = (F.softplus(r[..., 3:6]) * scale_factor.abs()).clamp(1e-4, 1.0)
    q = r[..., 6:10]
    rotation = q / q.norm(dim=-1, keepdim=True).clamp(min=1e-6)
    colour_opacity = torch.sigmoid(r[..., 10:14])
    out = torch.cat([position, scale, rotation, colour_opacity], dim=-1).reshape(Bn, N * G, 14)
    return torch.nan_to_num(out, nan=0.0) if torch.isnan(out).any() else out


def _pack_torch(gaussians, keep, G):
    """The gated result from the ungated one, image by image: kept voxels' rows in front, zeros behind."""
    Bn, NG, _ = gaussians.shape
    packed = torch.zeros_like(gaussians)
    counts = keep.sum(dim=1).to(torch.int32)
    for b in range(Bn):
        rows = gaussians[b].reshape(NG // G, G, 14)[keep[b]].reshape(-1, 14)
        packed[b, :rows.shape[0]] = rows
    return packed, counts


def _coords_i32(coords):
    """(B, N, 4) int32 contiguous.  Clamped BEFORE the cast, so an int64 or float value beyond int32 lands on the clamp it would meet
    anyway; float coordinates are truncated towards zero, as the positional encoding's `.long()` truncates them."""
    if coords.dtype is torch.int32 and coords.is_contiguous():
        return coords
    return coords.detach().clamp(0, 63).to(torch.int32).contiguous()


def _gains(position_offset_scale, scale_factor):
    return torch.stack([position_offset_scale.detach().reshape(()).float(), scale_factor.detach().reshape(()).float()])


class _SlatHeadHip(torch.autograd.Function):
    """fgs_slat_head_forward / _backward.  Nothing but the inputs is saved: the backward recomputes from `raw`.  The gains are read on
    the device: nothing synchronises with the host."""

    @staticmethod
    def forward(ctx, raw, position_offset_scale, scale_factor, coords):
        dev = raw.device
        Bn, N, G, _ = raw.shape
        d = (Bn, N, G)
        raw_, gains = _f32c(raw), _gains(position_offset_scale, scale_factor)
        out = torch.empty((Bn, N * G, 14), dtype=torch.float32, device=dev)
        hip.call(dev, "fgs_slat_head_forward", *d, raw_, coords, gains, None, out, None, None)
        ctx.dims = d
        ctx.gain_shapes = (position_offset_scale.shape, scale_factor.shape)
        ctx.save_for_backward(raw_, coords, gains)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        raw_, coords, gains = ctx.saved_tensors
        d = ctx.dims
        dev = raw_.device
        g_raw = torch.empty_like(raw_)
        want_gains = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        g_gains = torch.empty((2,), dtype=torch.float32, device=dev) if want_gains else None
        scratch = torch.empty(B.sizes("fgs_slat_workspace_bytes", *d), dtype=torch.uint8, device=dev)
        hip.call(dev, "fgs_slat_head_backward", *d, raw_, coords, gains, _f32c(g_out), g_raw, g_gains, scratch)
        g_pos = g_gains[0].reshape(ctx.gain_shapes[0]) if ctx.needs_input_grad[1] else None
        g_sf = g_gains[1].reshape(ctx.gain_shapes[1]) if ctx.needs_input_grad[2] else None
        return (g_raw if ctx.needs_input_grad[0] else None), g_pos, g_sf, None   # (the entry point always writes g_raw)


def _slat_head_gated_hip(raw, coords, position_offset_scale, scale_factor, keep):
    dev = raw.device
    Bn, N, G, _ = raw.shape
    d = (Bn, N, G)
    keep_ = keep.detach().contiguous().view(torch.uint8)  # a bool's byte is 0 or 1
    packed = torch.empty((Bn, N * G, 14), dtype=torch.float32, device=dev)
    counts = torch.empty((Bn,), dtype=torch.int32, device=dev)
    scratch = torch.empty(B.sizes("fgs_slat_workspace_bytes", *d), dtype=torch.uint8, device=dev)
    hip.call(dev, "fgs_slat_head_forward", *d, _f32c(raw), coords, _gains(position_offset_scale, scale_factor), keep_, packed, counts,
             scratch)
    return packed, counts


def slat_gaussian_head(raw: torch.Tensor, coords: torch.Tensor, position_offset_scale: torch.Tensor, scale_factor: torch.Tensor, *,
                       keep: Optional[torch.Tensor] = None, backend: str = "torch"):
    """The head of the reference's distillation decoders (DSD:318-358): the head MLP's raw output (B, N, G x 14) or (B, N, G, 14)
    and the voxel coordinates (B, N, 4) -- int32, int64 or float, columns 1:4 = x, y, z -- to the Gaussian cloud (B, N x G, 14), a row
    being position 3 | scale 3 | quaternion 4 | colour 3 | opacity 1.  With r = clamp(raw, -10, 10) and centre = clamp(coordinate, 0,
    63) / 64 x 2 - 1: position = clamp(centre + tanh(r) position_offset_scale, -1, 1); scale = clamp(softplus(r) |scale_factor|,
    1e-4, 1); quaternion = r / max(|r|, 1e-6); colour and opacity = sigmoid(r).  The two gains are 0-dim tensors on raw's device.
    Gradients flow to raw and to both gains.

    keep (B, N) bool selects the gated, inference-only form: -> (packed (B, N x G, 14), counts (B,) int32) with the Gaussians of
    image b's kept voxels in ascending voxel order in rows [0, counts[b] x G) and zeros behind; inputs that require grad are refused.

    backend "torch": the reference's expressions, its `isnan(...).any()` check and nan_to_num included, any device.  backend
    "hip": csrc/fgs_slat.hip -- one launch forward (two gated), two backward, bitwise repeatable, nothing read on the host
    (the ungated pair is capturable); CUDA/ROCm tensors only.  Its NaN rule (include/fgs.h): the forward values are the torch
    backend's (a NaN output is written as 0), but such an output is a constant of the backward -- g_raw is 0 there and the gain
    gradients get nothing from it, where torch's gradient is NaN-tainted.  Float coordinates are truncated to whole numbers there.
    Under autocast raw is cast to fp32."""
    if backend not in HEAD_BACKENDS:
        raise ValueError(f"unknown head backend {backend!r}: one of {HEAD_BACKENDS}")
    if raw.dim() == 3 and raw.shape[-1] % 14 == 0 and raw.shape[-1] > 0:
        raw = raw.reshape(raw.shape[0], raw.shape[1], raw.shape[-1] // 14, 14)
    if raw.dim() != 4 or raw.shape[-1] != 14:
        raise ValueError(f"raw must be (B, N, G x 14) or (B, N, G, 14), got {tuple(raw.shape)}")
    Bn, N, G, _ = raw.shape
    if tuple(coords.shape) != (Bn, N, 4):
        raise ValueError(f"coords must be ({Bn}, {N}, 4) with columns 1:4 = x, y, z, got {tuple(coords.shape)}")
    if coords.dtype not in (torch.int32, torch.int64) and not coords.is_floating_point():
        raise ValueError(f"coords must be int32, int64 or float, got {coords.dtype}")
    for name, t in (("position_offset_scale", position_offset_scale), ("scale_factor", scale_factor)):
        if not torch.is_tensor(t) or t.numel() != 1:
            raise ValueError(f"{name} must be a tensor that holds one value, got {tuple(t.shape) if torch.is_tensor(t) else type(t)}")
    if keep is not None:
        if keep.dtype is not torch.bool or tuple(keep.shape) != (Bn, N):
            raise ValueError(f"keep must be a ({Bn}, {N}) bool mask, got {tuple(keep.shape)} {keep.dtype}")
        _refuse_grad("slat_gaussian_head", (("raw", raw), ("position_offset_scale", position_offset_scale), ("scale_factor", scale_factor)))
    if backend == "hip":
        for t in (raw, coords, position_offset_scale, scale_factor) + ((keep,) if keep is not None else ()):
            hip.need_cuda(t, "slat_gaussian_head (backend 'hip')")
            if t.device != raw.device:
                raise B.FgsError(f"slat_gaussian_head (backend 'hip'): tensors on {t.device} and {raw.device}")
        if G > 64:
            raise B.FgsError(f"slat_gaussian_head (backend 'hip'): G = {G} > 64 Gaussians per voxel is not supported")
        ci = _coords_i32(coords)
        if keep is not None:
            return _slat_head_gated_hip(raw, ci, position_offset_scale, scale_factor, keep)
        return _SlatHeadHip.apply(raw, position_offset_scale, scale_factor, ci)
    if torch.is_autocast_enabled():
        raw = raw.float()
    gaussians = _slat_head_torch(raw, coords, position_offset_scale.reshape(()), scale_factor.reshape(()))
    return _pack_torch(gaussians, keep, G) if keep is not None else gaussians


# ---- the attention ----------------------------------------------------------------------------------------------------------------
ATTN_BACKENDS = ("torch", "hip")


def _check_attn_backend(attn_backend):
    if attn_backend not in ATTN_BACKENDS:
        raise ValueError(f"unknown attn_backend {attn_backend!r}: one of {ATTN_BACKENDS}")
    return attn_backend


def _attend_torch(q, k, v, scale, mask, drop, host_checks):
    """The reference's attention of one block of queries (DSD:118-146): q (B, H, n, d), k and v (B, H, M, d) -> (B, n, H d).  `drop`
    maps the probabilities to the dropped ones."""
    Bn, H, n, d = q.shape
    attn = (q @ k.transpose(-2, -1)) * scale
    if mask is not None:
        attn = attn.masked_fill(~mask.unsqueeze(1).unsqueeze(-1), -1e4)
    attn = attn - attn.max(dim=-1, keepdim=True).values
    attn = attn.softmax(dim=-1)
    attn = drop(attn)
    attn = _clean(attn, host_checks, nan=1.0 / attn.shape[-1])
    return (attn @ v).transpose(1, 2).reshape(Bn, n, H * d)


class _CrossAttnHip(torch.autograd.Function):
    """fgs_attn_forward / _backward.  Saved: the inputs, the output and one float per (b, h, n); the backward regenerates the
    dropout mask from the seed tensor.  Nothing synchronises with the host."""

    @staticmethod
    def forward(ctx, q, kv, row_keep, seed, num_heads, dropout_p):
        dev = q.device
        Bn, N, D = q.shape
        dims = (Bn, N, kv.shape[1], num_heads, D // num_heads)
        scale = float((D // num_heads) ** -0.5)
        q_, kv_ = _f32c(q), _f32c(kv)
        saved_bytes, _ = B.sizes("fgs_attn_workspace_bytes", *dims)
        out = torch.empty((Bn, N, D), dtype=torch.float32, device=dev)
        saved = torch.empty(saved_bytes, dtype=torch.uint8, device=dev)
        hip.call(dev, "fgs_attn_forward", *dims, scale, dropout_p, q_, kv_, row_keep, seed, out, saved)
        ctx.dims, ctx.scale, ctx.dropout_p = dims, scale, dropout_p
        ctx.save_for_backward(q_, kv_, row_keep, seed, out, saved)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        q_, kv_, row_keep, seed, out, saved = ctx.saved_tensors
        dev = q_.device
        g_q, g_kv = torch.empty_like(q_), torch.empty_like(kv_)
        _, scratch_bytes = B.sizes("fgs_attn_workspace_bytes", *ctx.dims)
        scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        hip.call(dev, "fgs_attn_backward", *ctx.dims, ctx.scale, ctx.dropout_p, q_, kv_, row_keep, seed, out, saved, _f32c(g_out), g_q,
                 g_kv, scratch)
        return g_q, g_kv, None, None, None, None


# the 16-bit compute dtypes of the fused attention -> the library's `dtype` argument (include/fgs.h)
ATTN_HALF_DTYPES = {torch.float16: B.FGS_ATTN_F16, torch.bfloat16: B.FGS_ATTN_BF16}


def _check_compute_dtype(compute_dtype, allow_autocast=False):
    if compute_dtype is None or compute_dtype in ATTN_HALF_DTYPES or (allow_autocast and compute_dtype == "autocast"):
        return compute_dtype
    raise ValueError(f"unknown attention compute dtype {compute_dtype!r}: None (fp32), torch.float16 or torch.bfloat16"
                     + (', or "autocast"' if allow_autocast else ""))


class _CrossAttnHalfHip(torch.autograd.Function):
    """fgs_attn_half_forward / _backward on 16-bit q and kv (contiguous, of one dtype: `cross_attention` sees to it).  Saved: the
    inputs, the 16-bit output and one fp32 per (b, h, n).  Nothing synchronises with the host."""

    @staticmethod
    def forward(ctx, q, kv, row_keep, seed, num_heads, dropout_p):
        dev = q.device
        Bn, N, D = q.shape
        dims = (Bn, N, kv.shape[1], num_heads, D // num_heads)
        scale = float((D // num_heads) ** -0.5)
        code = ATTN_HALF_DTYPES[q.dtype]
        saved_bytes, _ = B.sizes("fgs_attn_half_workspace_bytes", *dims)
        out = torch.empty((Bn, N, D), dtype=q.dtype, device=dev)
        saved = torch.empty(saved_bytes, dtype=torch.uint8, device=dev)
        hip.call(dev, "fgs_attn_half_forward", code, *dims, scale, dropout_p, q, kv, row_keep, seed, out, saved)
        ctx.dims, ctx.scale, ctx.dropout_p, ctx.code = dims, scale, dropout_p, code
        ctx.save_for_backward(q, kv, row_keep, seed, out, saved)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        q, kv, row_keep, seed, out, saved = ctx.saved_tensors
        dev = q.device
        if g_out.dtype != q.dtype or not g_out.is_contiguous():
            g_out = g_out.to(q.dtype).contiguous()
        g_q, g_kv = torch.empty_like(q), torch.empty_like(kv)
        _, scratch_bytes = B.sizes("fgs_attn_half_workspace_bytes", *ctx.dims)
        scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        hip.call(dev, "fgs_attn_half_backward", ctx.code, *ctx.dims, ctx.scale, ctx.dropout_p, q, kv, row_keep, seed, out, saved, g_out,
                 g_q, g_kv, scratch)
        return g_q, g_kv, None, None, None, None


def cross_attention(q: torch.Tensor, kv: torch.Tensor, num_heads: int, *, mask: Optional[torch.Tensor] = None,
                    dropout_p: float = 0.0, seed: Optional[torch.Tensor] = None, backend: str = "torch",
                    compute_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """The attention of the reference's CrossAttention between its Linear layers (DSD:105-146): q (B, N, D), the output of the query
    projection, and kv (B, M, 2, H, d) or (B, M, 2 D), the output of the key/value projection (keys kv[:, :, 0], values kv[:, :, 1],
    D = H d) -> (B, N, D), ready for the output projection.  Scores scale <q, k> with scale = d^-0.5; `mask` (B, N) bool: a False
    row has every score filled with -1e4, so it attends uniformly (its output is the mean of v); softmax; dropout of the
    probabilities with `dropout_p` in [0, 1) (0 = none; the caller decides whether it is training); a NaN probability becomes 1 / M.

    backend "torch": the reference's op sequence, any device; dropout is torch's own (`seed` is not used).  backend "hip":
    csrc/fgs_attn.hip -- one launch forward, three backward, fp32 on the matrix cores, nothing of size N x M stored, bitwise
    repeatable, nothing read on the host; CUDA/ROCm tensors only, d <= 128, inputs cast to fp32 under autocast, no double
    backward.  Its NaN rule (include/fgs.h): a row whose scores hold a NaN or +Inf, or are all -Inf, gets 1 / M each without
    dropout -- the reference's values -- but is a constant of the backward (zero g_q row, g_kv through v only) where torch's
    gradient is NaN-tainted.  Its dropout keeps element (b, h, n, m) by a stated counter-based function of `seed` (include/fgs.h),
    a one-element int64 tensor on q's device; with dropout_p > 0 and no seed one is drawn by torch.randint on the device (it
    follows torch.manual_seed, and nothing is read on the host).

    `compute_dtype` (backend "hip" only).  None: the fp32 kernels and an fp32 `out`, under autocast as well.  torch.float16 /
    torch.bfloat16: csrc/fgs_attn_half.hip -- the same definition on 16-bit tensors: q and kv are used in place when they already are
    contiguous tensors of that dtype (under autocast the Linear layers' outputs are) and cast once otherwise, `out` has that dtype,
    the gradients reach q and kv in their own dtypes, an upstream gradient of another dtype or layout is cast once; still one launch
    forward and three backward, whatever the autocast state.  Products take 16-bit operands and accumulate in fp32, the scores and the
    softmax stay fp32, only the probabilities and dS are rounded ahead of the second products (the contract: include/fgs.h).  Stated
    differences from torch under autocast: an fp16 score beyond 65504 stays finite here (torch's overflows and its row becomes 1 / M
    each); dS in fp16 can underflow for small upstream gradients, which is what a GradScaler is for.  With backend "torch" the
    caller's autocast decides the precision, so a compute_dtype there is a ValueError."""
    _check_attn_backend(backend)
    _check_compute_dtype(compute_dtype)
    if backend == "torch" and compute_dtype is not None:
        raise ValueError("cross_attention (backend 'torch'): compute_dtype is for backend 'hip'; here the caller's autocast decides")
    if isinstance(num_heads, bool) or int(num_heads) != num_heads or num_heads < 1:
        raise ValueError(f"num_heads must be a positive integer, got {num_heads!r}")
    num_heads = int(num_heads)
    if q.dim() != 3 or q.shape[-1] % num_heads or 0 in q.shape:
        raise ValueError(f"q must be (B, N, D) with D a multiple of num_heads = {num_heads} and no empty axis, got {tuple(q.shape)}")
    Bn, N, D = q.shape
    d = D // num_heads
    if kv.dim() == 3 and kv.shape[-1] == 2 * D:
        kv = kv.reshape(kv.shape[0], kv.shape[1], 2, num_heads, d)
    if kv.dim() != 5 or kv.shape[0] != Bn or tuple(kv.shape[2:]) != (2, num_heads, d) or kv.shape[1] < 1:
        raise ValueError(f"kv must be ({Bn}, M, 2, {num_heads}, {d}) or ({Bn}, M, {2 * D}) with M >= 1, got {tuple(kv.shape)}")
    if mask is not None and (mask.dtype is not torch.bool or tuple(mask.shape) != (Bn, N)):
        raise ValueError(f"mask must be a ({Bn}, {N}) bool tensor, got {tuple(mask.shape)} {mask.dtype}")
    dropout_p = ctypes.c_float(dropout_p).value   # as the library sees it: fp32 (1 - 1e-9 is 1.0 there)
    if not 0.0 <= dropout_p < 1.0:
        raise ValueError(f"dropout_p must be in [0, 1), got {dropout_p!r}")
    if backend == "torch":
        k, v = kv.permute(2, 0, 3, 1, 4)
        qh = q.reshape(Bn, N, num_heads, d).permute(0, 2, 1, 3)
        drop = (lambda a: F.dropout(a, dropout_p, training=True)) if dropout_p > 0.0 else (lambda a: a)
        return _attend_torch(qh, k, v, d ** -0.5, mask, drop, False)
    who = "cross_attention (backend 'hip')"
    if d > B.FGS_ATTN_MAX_HEAD_DIM:
        raise ValueError(f"{who}: head dimension {d} > {B.FGS_ATTN_MAX_HEAD_DIM} is not supported")
    if Bn * num_heads * N >= 2 ** 31:
        raise ValueError(f"{who}: B x H x N = {Bn} x {num_heads} x {N} is beyond the supported size")
    if compute_dtype is None and (not kv.is_contiguous() or not q.is_contiguous()):
        raise ValueError(f"{who}: q and kv must be contiguous -- the Linear layers' outputs as they are, not a permuted view")
    if seed is not None and (not torch.is_tensor(seed) or seed.dtype is not torch.int64 or seed.numel() != 1):
        raise ValueError(f"{who}: seed must be a one-element int64 tensor on q's device")
    for t in (q, kv) + tuple(t for t in (mask, seed) if t is not None):
        hip.need_cuda(t, who)
        if t.device != q.device:
            raise B.FgsError(f"{who}: tensors on {t.device} and {q.device}")
    if dropout_p > 0.0 and seed is None:
        seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=q.device)
    row_keep = None if mask is None else mask.detach().contiguous().view(torch.uint8)  # a bool's byte is 0 or 1
    if compute_dtype is not None:
        # (a differentiable cast: autograd returns the gradient in the tensor's own dtype and layout)
        q, kv = (t if t.dtype == compute_dtype and t.is_contiguous() else t.to(compute_dtype).contiguous() for t in (q, kv))
        return _CrossAttnHalfHip.apply(q, kv, row_keep, seed if dropout_p > 0.0 else None, num_heads, dropout_p)
    return _CrossAttnHip.apply(q, kv, row_keep, seed if dropout_p > 0.0 else None, num_heads, dropout_p)


# ---- the modules ------------------------------------------------------------------------------------------------------------------
class PositionalEncoding3D(nn.Module):
    """Learnable per-axis embeddings of a voxel's coordinates (DSD:24-60): d_model // 3 channels for x and for y, the rest for z;
    coordinates clamp to [0, max_resolution - 1] and truncate to whole numbers.  coords (B, N, 4) or (N, 4), columns 1:4 = x, y, z."""

    def __init__(self, d_model: int, max_resolution: int = 64):
        super().__init__()
        self.d_model = d_model
        self.max_resolution = max_resolution
        self.pos_embed_x = nn.Embedding(max_resolution, d_model // 3)
        self.pos_embed_y = nn.Embedding(max_resolution, d_model // 3)
        self.pos_embed_z = nn.Embedding(max_resolution, d_model - 2 * (d_model // 3))

    def forward(self, coords: torch.Tensor) -> torch.Tensor:
        top = self.max_resolution - 1
        x, y, z = (coords[..., i].clamp(0, top).long() for i in (1, 2, 3))
        return torch.cat([self.pos_embed_x(x), self.pos_embed_y(y), self.pos_embed_z(z)], dim=-1)


class CrossAttention(nn.Module):
    """Cross-attention from the voxels (queries) to the image features (keys, values) (DSD:63-182).  More than `chunk_size` queries
    are processed in chunks.  `mask` (B, N) masks whole QUERY rows with -1e4: every score of a padded voxel is the same, so it
    attends uniformly (the reference's behaviour, kept).  `host_checks` (an attribute, True as in the reference): test for NaN on
    the host before replacing it; False replaces unconditionally.  `backend` (an attribute, "torch" as in the reference): "hip" runs
    `cross_attention(..., backend="hip")` -- the query projection once for all N and ONE fused call whatever `chunk_size` is, with
    attention dropout active iff the module is training and `attn_drop.p > 0`.  `compute_dtype` (an attribute, None by default; read
    with backend "hip" only): None runs the fp32 kernels; torch.float16 / torch.bfloat16 run the 16-bit kernels of
    `cross_attention(..., compute_dtype=...)` on the Linear layers' outputs as they are -- under autocast in that dtype they already
    have it, so nothing is copied; "autocast" means torch.get_autocast_dtype("cuda") while CUDA autocast is enabled and fp32
    otherwise."""

    def __init__(self, dim: int, num_heads: int = 8, qkv_bias: bool = True, attn_drop: float = 0.0, proj_drop: float = 0.0,
                 chunk_size: int = 1024):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.chunk_size = chunk_size
        self.q = nn.Linear(dim, dim, bias=qkv_bias)
        self.kv = nn.Linear(dim, dim * 2, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.host_checks = True
        self.backend = "torch"
        self.compute_dtype = None

    def _hip_compute_dtype(self):
        """The attribute resolved for this call: None (fp32) or a 16-bit dtype."""
        cd = _check_compute_dtype(self.compute_dtype, allow_autocast=True)
        if cd != "autocast":
            return cd
        if not torch.is_autocast_enabled("cuda"):
            return None
        cd = torch.get_autocast_dtype("cuda")
        return cd if cd in ATTN_HALF_DTYPES else None

    def _attend(self, x, k, v, mask):
        """One block of queries x (B, n, D) against all keys -> (B, n, D), before the output projection."""
        Bn, n, D = x.shape
        q = self.q(x).reshape(Bn, n, self.num_heads, self.head_dim).permute(0, 2, 1, 3)
        return _attend_torch(q, k, v, self.scale, mask, self.attn_drop, self.host_checks)

    def forward(self, x: torch.Tensor, context: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        Bn, N, D = x.shape
        M = context.shape[1]
        if _check_attn_backend(self.backend) == "hip":
            p = self.attn_drop.p if self.training else 0.0
            x = cross_attention(self.q(x), self.kv(context).reshape(Bn, M, 2, self.num_heads, self.head_dim), self.num_heads,
                                mask=mask, dropout_p=p, backend="hip", compute_dtype=self._hip_compute_dtype())
            if x.dtype != self.proj.weight.dtype and not torch.is_autocast_enabled("cuda"):
                x = x.to(self.proj.weight.dtype)   # a 16-bit compute_dtype outside autocast: the projection runs in its own dtype
            return self.proj_drop(self.proj(x))
        kv = self.kv(context).reshape(Bn, M, 2, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4)
        k, v = kv[0], kv[1]
        if N > self.chunk_size:
            x = torch.cat([self._attend(x[:, i:i + self.chunk_size], k, v, None if mask is None else mask[:, i:i + self.chunk_size])
                           for i in range(0, N, self.chunk_size)], dim=1)
        else:
            x = self._attend(x, k, v, mask)
        return self.proj_drop(self.proj(x))


class SparseTransformerBlock(nn.Module):
    """Pre-norm block (DSD:185-221): x + cross_attn(norm1(x), norm2(context)), then x + mlp(norm3(x))."""

    def __init__(self, dim: int, num_heads: int = 8, mlp_ratio: float = 4.0, drop: float = 0.0, attn_drop: float = 0.0):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.cross_attn = CrossAttention(dim, num_heads, attn_drop=attn_drop, proj_drop=drop)
        self.norm2 = nn.LayerNorm(dim)
        self.norm3 = nn.LayerNorm(dim)
        mlp_hidden = int(dim * mlp_ratio)
        self.mlp = nn.Sequential(nn.Linear(dim, mlp_hidden), nn.GELU(), nn.Dropout(drop), nn.Linear(mlp_hidden, dim), nn.Dropout(drop))

    def forward(self, x: torch.Tensor, context: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = x + self.cross_attn(self.norm1(x), self.norm2(context), mask)
        return x + self.mlp(self.norm3(x))


class OccupancyHead(nn.Module):
    """Per-voxel occupancy logit (DSD:224-252): (B, N, hidden) -> (B, N)."""

    def __init__(self, hidden_dim: int = 512):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(hidden_dim, hidden_dim // 2), nn.ReLU(), nn.Linear(hidden_dim // 2, 1))
        nn.init.zeros_(self.mlp[-1].bias)
        nn.init.normal_(self.mlp[-1].weight, std=0.01)

    def forward(self, voxel_features: torch.Tensor) -> torch.Tensor:
        return self.mlp(voxel_features).squeeze(-1)


class GaussianHead(nn.Module):
    """The output head (DSD:255-358): a three-layer MLP to G x 14 raw values per voxel, then `slat_gaussian_head` with the two
    learnable gains.  `backend` (an attribute, "torch" as in the reference) selects the head's backend and, with "hip", drops the
    host's look at the input."""

    def __init__(self, in_dim: int, hidden_dim: int = 256, num_gaussians_per_voxel: int = 32, init_offset_scale: float = 0.5):
        super().__init__()
        self.num_gaussians = num_gaussians_per_voxel
        out_dim = num_gaussians_per_voxel * 14
        self.head = nn.Sequential(nn.Linear(in_dim, hidden_dim), nn.GELU(), nn.Linear(hidden_dim, hidden_dim), nn.GELU(),
                                  nn.Linear(hidden_dim, out_dim))
        self.position_offset_scale = nn.Parameter(torch.tensor(init_offset_scale))
        self.scale_factor = nn.Parameter(torch.tensor(0.01))
        nn.init.zeros_(self.head[-1].bias)
        nn.init.normal_(self.head[-1].weight, std=0.01)
        self.backend = "torch"

    def raw(self, x: torch.Tensor) -> torch.Tensor:
        """The head MLP behind the reference's input cleaning: (B, N, D) -> (B, N, G x 14)."""
        return self.head(_clean(x, self.backend == "torch", nan=0.0, posinf=1.0, neginf=-1.0))

    def forward(self, x: torch.Tensor, coords: torch.Tensor, keep: Optional[torch.Tensor] = None):
        return slat_gaussian_head(self.raw(x), coords, self.position_offset_scale, self.scale_factor, keep=keep, backend=self.backend)


class DirectSLatDecoder(nn.Module):
    """The reference's DirectSLatDecoder (DSD:361-556): image features and sparse voxel coordinates -> Gaussians, by transformer
    blocks whose voxel queries cross-attend to the projected features.  Same constructor arguments and defaults, `_init_weights`,
    forward signature and returned dict: `gaussians` (B, N x G, 14) and, with predict_occupancy, `occupancy_logits` (B, N); with
    apply_occupancy_mask=True `gaussians` is a list of (n_b, 14) tensors, one per image, beside `n_gaussians` and `occupancy_mask`.
    Kept quirks: coordinates clamp to [0, 63] and centres are c / 64 x 2 - 1 whatever `max_resolution` is; `coord_mask` masks query
    rows; the dropout modules stay.

    `head_backend` "torch": the reference's op sequence with every host check.  "hip": the fused head (fresnel_amd.slat docstring);
    the gated inference computes keep = (sigmoid(logits) > threshold) & coord_mask, runs the head MLP on ALL voxels, calls the gated
    head once and reads the per-image counts with one host copy; the list entries are views of the packed tensor.  ONE RESTRICTION
    against the reference there: the gated head is inference-only, so on "hip" `forward(..., apply_occupancy_mask=True)` must run
    under `torch.no_grad()` (a ValueError says so otherwise); the reference and the "torch" backend also accept it with grad enabled.

    `attn_backend` "torch": the reference's chunked attention.  "hip": every block's cross-attention is the fused kernel of
    `cross_attention` (no score tensor, no chunking, device-side dropout).  The two backends are independent.

    `attn_dtype` sets every block's `CrossAttention.compute_dtype` (read with attn_backend "hip"): None, torch.float16,
    torch.bfloat16 or "autocast" -- the 16-bit fused attention whenever the model runs under CUDA autocast, fp32 otherwise."""

    def __init__(self, feature_dim: int = 1024, hidden_dim: int = 512, num_layers: int = 6, num_heads: int = 8,
                 num_gaussians_per_voxel: int = 8, max_resolution: int = 64, dropout: float = 0.1, use_checkpoint: bool = False,
                 predict_occupancy: bool = True, occupancy_threshold: float = 0.5, head_backend: str = "torch",
                 attn_backend: str = "torch", attn_dtype=None):
        super().__init__()
        self.head_backend = _check_backend(head_backend)
        self.attn_backend = _check_attn_backend(attn_backend)
        self.attn_dtype = _check_compute_dtype(attn_dtype, allow_autocast=True)
        self.feature_dim = feature_dim
        self.hidden_dim = hidden_dim
        self.num_gaussians_per_voxel = num_gaussians_per_voxel
        self.use_checkpoint = use_checkpoint
        self.predict_occupancy = predict_occupancy
        self.occupancy_threshold = occupancy_threshold
        self.feature_proj = nn.Linear(feature_dim, hidden_dim)
        self.pos_encoding = PositionalEncoding3D(hidden_dim, max_resolution)
        self.voxel_embed = nn.Parameter(torch.randn(1, 1, hidden_dim) * 0.02)
        self.blocks = nn.ModuleList([SparseTransformerBlock(hidden_dim, num_heads=num_heads, mlp_ratio=4.0, drop=dropout,
                                                            attn_drop=dropout) for _ in range(num_layers)])
        self.norm = nn.LayerNorm(hidden_dim)
        self.occupancy_head = OccupancyHead(hidden_dim) if predict_occupancy else None
        self.gaussian_head = GaussianHead(hidden_dim, hidden_dim, num_gaussians_per_voxel)
        self._init_weights()
        self.gaussian_head.backend = head_backend
        for block in self.blocks:
            block.cross_attn.host_checks = head_backend == "torch"
            block.cross_attn.backend = attn_backend
            block.cross_attn.compute_dtype = attn_dtype

    def _init_weights(self):
        """Every Linear gets Xavier-uniform weights -- gain 0.1 where the module's path contains "q", "kv" or "proj", 0.5 elsewhere --
        and a zero bias; LayerNorms are reset to (1, 0); embeddings are drawn from N(0, 0.02^2).  Modules are visited in
        registration order, so the draws are the reference's under the same seed (DSD:436-451).  Its test is a substring test on the
        whole path and is kept as it is: "occupancy_head.mlp.0" contains a "q" and gets 0.1 too."""
        small = ("q", "kv", "proj")
        for path, m in self.named_modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight, gain=0.1 if any(tag in path for tag in small) else 0.5)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.LayerNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Embedding):
                nn.init.normal_(m.weight, mean=0.0, std=0.02)

    def forward(self, features: torch.Tensor, coords: torch.Tensor, coord_mask: Optional[torch.Tensor] = None,
                apply_occupancy_mask: bool = False) -> Dict[str, torch.Tensor]:
        Bn, N, _ = coords.shape
        host = self.head_backend == "torch"
        features = _clean(features, host, nan=0.0, posinf=1.0, neginf=-1.0)
        coords = coords.clone()
        coords[:, :, 1:4] = coords[:, :, 1:4].clamp(0, 63)
        context = _clean(self.feature_proj(features), host, nan=0.0)
        x = self.voxel_embed.expand(Bn, N, -1) + self.pos_encoding(coords)
        for block in self.blocks:
            if self.use_checkpoint and self.training:
                x = checkpoint(block, x, context, coord_mask, use_reentrant=False)
            else:
                x = block(x, context, coord_mask)
            x = _clean(x, host, nan=0.0)
        x = self.norm(x)
        result = {}
        if self.predict_occupancy and self.occupancy_head is not None:
            occupancy_logits = self.occupancy_head(x)
            result["occupancy_logits"] = occupancy_logits
            if apply_occupancy_mask:
                occupancy_mask = torch.sigmoid(occupancy_logits) > self.occupancy_threshold
                result["occupancy_mask"] = occupancy_mask
                G = self.num_gaussians_per_voxel
                if host:
                    gaussians_list = []
                    for b in range(Bn):
                        mask_b = occupancy_mask[b]
                        if coord_mask is not None:
                            mask_b = mask_b & coord_mask[b]
                        if mask_b.sum() == 0:
                            gaussians_list.append(torch.zeros(0, 14, device=x.device))
                        else:
                            gaussians_list.append(self.gaussian_head(x[b:b + 1, mask_b], coords[b:b + 1, mask_b]).squeeze(0))
                else:
                    keep = occupancy_mask if coord_mask is None else occupancy_mask & coord_mask
                    packed, counts = self.gaussian_head(x, coords, keep=keep)
                    gaussians_list = [packed[b, :n * G] for b, n in enumerate(counts.tolist())]  # the one host copy
                result["gaussians"] = gaussians_list
                result["n_gaussians"] = [g.shape[0] for g in gaussians_list]
            else:
                result["gaussians"] = self.gaussian_head(x, coords)
        else:
            result["gaussians"] = self.gaussian_head(x, coords)
        return result

    def enable_checkpointing(self):
        self.use_checkpoint = True

    def disable_checkpointing(self):
        self.use_checkpoint = False


class MLPSLatDecoder(nn.Module):
    """The reference's MLPSLatDecoder (DSD:559-625): the mean-pooled, projected image feature plus the positional encoding through
    `num_layers` Linear / LayerNorm / GELU layers, then the Gaussian head.  Same constructor arguments and defaults (its default
    initialisation: no `_init_weights`); returns the (B, N x G, 14) tensor; `coord_mask` is accepted and unused, as there."""

    def __init__(self, feature_dim: int = 1024, hidden_dim: int = 512, num_layers: int = 4, num_gaussians_per_voxel: int = 32,
                 max_resolution: int = 64, head_backend: str = "torch"):
        super().__init__()
        self.head_backend = _check_backend(head_backend)
        self.feature_dim = feature_dim
        self.hidden_dim = hidden_dim
        self.num_gaussians_per_voxel = num_gaussians_per_voxel
        self.feature_proj = nn.Linear(feature_dim, hidden_dim)
        self.pos_encoding = PositionalEncoding3D(hidden_dim, max_resolution)
        layers = []
        for _ in range(num_layers):
            layers.extend([nn.Linear(hidden_dim, hidden_dim), nn.LayerNorm(hidden_dim), nn.GELU()])
        self.mlp = nn.Sequential(*layers)
        self.gaussian_head = GaussianHead(hidden_dim, hidden_dim, num_gaussians_per_voxel)
        self.gaussian_head.backend = head_backend

    def forward(self, features: torch.Tensor, coords: torch.Tensor, coord_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        N = coords.shape[1]
        global_feat = self.feature_proj(features.mean(dim=1, keepdim=True)).expand(-1, N, -1)
        x = self.mlp(global_feat + self.pos_encoding(coords))
        return self.gaussian_head(x, coords)
