"""The losses of the consistency view synthesizer: mirrors of the reference's scripts/models/quality_aware_losses.py ("QAL") and of
ConsistencyLoss (scripts/models/consistency_view_synthesis.py, CVS:844-941), with a fused HIP backend for their pixel terms.

`compute_depth_laplacian`, `compute_quality_mask`, `compute_gradient_penalty`, `get_consistency_weight_schedule`,
`visualize_quality_mask`, `QualityAwareCVSLoss` and `ConsistencyLoss` have the reference's names, arguments, defaults, returned keys
and quirks (the optional `lpips` import with its warning; `perceptual_net`'s module tree and state-dict keys; a `total` that starts as
the float 0.0).  `compute_quality_mask` and `visualize_quality_mask` take `backend=` as a keyword, the two classes have a `backend`
attribute (and constructor keyword), "torch" by default.  The three functions without a kernel of their own (the Laplacian alone, the
gradient penalty of a given mask, the schedule) are torch / Python only.

backend "torch": the reference's op sequence, any device.  backend "hip": the pixel terms run in csrc/fgs_cvs_loss.hip (definition:
include/fgs.h, fgs_cvs_*) -- `cvs_quality_terms`, two launches forward and one backward instead of several dozen element-wise
launches and as many full-size temporaries, and `consistency_euler_step`, one launch; LPIPS, `perceptual_net` and the weighted sum
stay in torch.  Stated differences of "hip": the gradient reaches `pred` only (a `depth`, `target` or `ema` that requires grad raises
ValueError; with "torch" it gets a gradient); with the boundary or gradient term on, H >= 2 and W >= 2 are required (the reference
returns NaN there, the mean of an empty tensor); inputs must be fp32, contiguous, on one device, with B C H W < 2^31; a timestep
outside the schedule is clamped into it.  All checks are on the host and read no device data: nothing here synchronises.
"""
from typing import Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _binding as B
from . import _hip as hip

BACKENDS = ("torch", "hip")
CONSISTENCY_FORMS = (None, "l1", "mse")
TERMS = ("l1_weighted", "consistency", "boundary", "gradient")


def _check_backend(backend):
    if backend not in BACKENDS:
        raise ValueError(f"unknown backend {backend!r}: one of {BACKENDS}")
    return backend


# ---- the reference's functions ------------------------------------------------------------------------------------------------------
def compute_depth_laplacian(depth: torch.Tensor) -> torch.Tensor:
    """|d[y-1] + d[y+1] + d[x-1] + d[x+1] - 4 d| with circular neighbours (QAL:21-41).  depth (B, 1, H, W) -> the same shape."""
    laplacian = (torch.roll(depth, 1, dims=-2) + torch.roll(depth, -1, dims=-2) + torch.roll(depth, 1, dims=-1)
                 + torch.roll(depth, -1, dims=-1) - 4 * depth)
    return torch.abs(laplacian)


def compute_quality_mask(rendered_depth: torch.Tensor, threshold: float = 0.01, sharpness: float = 100.0, *,
                         backend: str = "torch") -> torch.Tensor:
    """sigmoid(-sharpness (laplacian - threshold)) (QAL:44-68): (B, 1, H, W) in [0, 1], 1 = high quality.  backend "hip": the plane
    fgs_cvs_quality_mask writes, one launch; no gradient to the depth (one that requires grad raises ValueError)."""
    if _check_backend(backend) == "torch":
        return torch.sigmoid(-sharpness * (compute_depth_laplacian(rendered_depth) - threshold))
    who = "compute_quality_mask (backend 'hip')"
    if rendered_depth.dim() < 2 or 0 in rendered_depth.shape:
        raise ValueError(f"{who}: rendered_depth must be (..., H, W) with no empty axis, got {tuple(rendered_depth.shape)}")
    _check_hip_tensors(who, rendered_depth, rendered_depth=rendered_depth)
    if rendered_depth.requires_grad:
        raise ValueError(f"{who}: rendered_depth requires grad, but the kernel gives no gradient (detach it, or use backend 'torch')")
    H, W = rendered_depth.shape[-2:]
    mask = torch.empty(rendered_depth.shape, dtype=torch.float32, device=rendered_depth.device)
    hip.call(rendered_depth.device, "fgs_cvs_quality_mask", rendered_depth.numel() // (H * W), H, W, float(threshold), float(sharpness),
             rendered_depth, mask)
    return mask


def compute_gradient_penalty(image: torch.Tensor, quality_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Total variation of `image` (B, C, H, W), weighted by the mask at the left / upper pixel of every difference (QAL:71-100)."""
    grad_x = torch.abs(image[:, :, :, :-1] - image[:, :, :, 1:])
    grad_y = torch.abs(image[:, :, :-1, :] - image[:, :, 1:, :])
    if quality_mask is not None:
        return (grad_x * quality_mask[:, :, :, :-1]).mean() + (grad_y * quality_mask[:, :, :-1, :]).mean()
    return grad_x.mean() + grad_y.mean()


def get_consistency_weight_schedule(epoch: int, total_epochs: int, schedule_type: str = 'progressive') -> float:
    """The consistency weight of an epoch (QAL:107-146): 'constant' 1; 'progressive' 0.1 / 0.3 / 1.0 below 33 % / below 66 % / from
    66 % of the epochs on; 'warmup' linear to 1 over the first half."""
    if schedule_type == 'constant':
        return 1.0
    elif schedule_type == 'progressive':
        progress = epoch / total_epochs
        if progress < 0.33:
            return 0.1
        elif progress < 0.66:
            return 0.3
        else:
            return 1.0
    elif schedule_type == 'warmup':
        return min(1.0, epoch / (total_epochs * 0.5))
    else:
        raise ValueError(f"Unknown schedule type: {schedule_type}")


def visualize_quality_mask(depth: torch.Tensor, threshold: float = 0.01, sharpness: float = 100.0, *,
                           backend: str = "torch") -> torch.Tensor:
    """(B, 3, H, W): red = 1 - quality, green = quality (QAL:309-333)."""
    quality_mask = compute_quality_mask(depth, threshold, sharpness, backend=backend)
    vis = torch.zeros(quality_mask.shape[0], 3, quality_mask.shape[2], quality_mask.shape[3], device=quality_mask.device)
    vis[:, 0, :, :] = 1.0 - quality_mask[:, 0, :, :]
    vis[:, 1, :, :] = quality_mask[:, 0, :, :]
    return vis


# ---- the fused pixel terms -----------------------------------------------------------------------------------------------------------
def _check_hip_tensors(who, first, **tensors):
    """Host-side contract of the kernels: fp32, contiguous, on the first tensor's CUDA/ROCm device, fewer than 2^31 elements."""
    for name, t in tensors.items():
        if t is None:
            continue
        if not torch.is_tensor(t):
            raise ValueError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
        hip.need_cuda(t, who)
        if t.device != first.device:
            raise ValueError(f"{who}: {name} is on {t.device}, not on {first.device}")
        if t.dtype is not torch.float32:
            raise ValueError(f"{who}: {name} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous (shape {tuple(t.shape)}, strides {t.stride()})")
        if t.numel() >= 2 ** 31:
            raise ValueError(f"{who}: {name} has {t.numel()} elements, beyond the supported size (2^31)")


def _flags(quality, consistency, boundary, gradient):
    return ((B.FGS_CVS_QUALITY if quality else 0) | {None: 0, "l1": B.FGS_CVS_CONS_L1, "mse": B.FGS_CVS_CONS_MSE}[consistency]
            | (B.FGS_CVS_BOUNDARY if boundary else 0) | (B.FGS_CVS_GRADIENT if gradient else 0))


class _CvsTermsHip(torch.autograd.Function):
    """fgs_cvs_loss_forward / _backward.  Saved: the inputs and, with the quality mask, its (B, 1, H, W) plane -- nothing else of
    the images' size.  The upstream gradients of the four terms stay on the device."""

    @staticmethod
    def forward(ctx, pred, target, depth, ema, flags, threshold, sharpness):
        dev = pred.device
        dims = (*pred.shape, flags)
        pred_ = pred.detach()
        saved_bytes, scratch_bytes = B.sizes("fgs_cvs_loss_workspace_bytes", *dims)
        out = torch.empty(4, dtype=torch.float32, device=dev)
        saved = torch.empty(saved_bytes, dtype=torch.uint8, device=dev) if saved_bytes else None
        scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        hip.call(dev, "fgs_cvs_loss_forward", *dims, threshold, sharpness, pred_, target, depth, ema, out, saved, scratch)
        ctx.dims, ctx.threshold, ctx.sharpness = dims, threshold, sharpness
        ctx.save_for_backward(pred_, target, depth, ema, saved)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        pred_, target, depth, ema, saved = ctx.saved_tensors
        g_terms = hip.f32c(g_out)
        g_pred = torch.empty_like(pred_)
        hip.call(pred_.device, "fgs_cvs_loss_backward", *ctx.dims, ctx.threshold, ctx.sharpness, pred_, target, depth, ema, saved, g_terms,
                 g_pred)
        return g_pred, None, None, None, None, None, None


def _terms_torch(pred, target, depth, ema, quality, consistency, boundary, gradient, threshold, sharpness):
    """The reference's op sequence (QAL:232-297; CVS:905, 935 with quality off and the MSE form)."""
    quality_mask = compute_quality_mask(depth, threshold=threshold, sharpness=sharpness) if quality else None
    l1_pixelwise = F.l1_loss(pred, target, reduction='none')
    zero = l1_pixelwise.new_zeros(())
    terms = [(l1_pixelwise * quality_mask).mean() if quality else l1_pixelwise.mean(), zero, zero, zero]
    if consistency == "l1":
        terms[1] = F.l1_loss(pred, ema.detach())
    elif consistency == "mse":
        terms[1] = F.mse_loss(pred, ema.detach())
    if boundary:
        depth_grad_x = torch.abs(depth[:, :, :, :-1] - depth[:, :, :, 1:])
        depth_grad_y = torch.abs(depth[:, :, :-1, :] - depth[:, :, 1:, :])
        boundary_mask_x = (depth_grad_x > 0.01).to(pred.dtype)
        boundary_mask_y = (depth_grad_y > 0.01).to(pred.dtype)
        pixel_error = torch.abs(pred - target).mean(dim=1, keepdim=True)
        terms[2] = (pixel_error[:, :, :, :-1] * boundary_mask_x).mean() + (pixel_error[:, :, :-1, :] * boundary_mask_y).mean()
    if gradient:
        terms[3] = compute_gradient_penalty(pred, quality_mask)
    return torch.stack(terms)


def cvs_quality_terms(pred: torch.Tensor, target: torch.Tensor, depth: Optional[torch.Tensor], ema: Optional[torch.Tensor], *,
                      quality: bool = True, consistency: Optional[str] = "l1", boundary: bool = False, gradient: bool = False,
                      threshold: float = 0.01, sharpness: float = 100.0, backend: str = "torch") -> torch.Tensor:
    """The pixel terms of the CVS losses as one tensor of four, (l1_weighted, consistency, boundary, gradient), that carries the
    graph to `pred`; a term that is off is 0.

    pred, target, ema (B, C, H, W); depth (B, 1, H, W), needed with `quality` (the depth-Laplacian mask weights the L1 and the
    gradient term) and `boundary`.  consistency: None | "l1" (QualityAwareCVSLoss: mean |pred - ema|) | "mse" (ConsistencyLoss: mean
    (pred - ema)^2); `ema` is detached.  backend "torch": the reference's op sequence.  backend "hip": csrc/fgs_cvs_loss.hip, two
    launches forward and one backward, bitwise repeatable, capturable; gradient to `pred` only -- see the module's stated differences."""
    _check_backend(backend)
    if consistency not in CONSISTENCY_FORMS:
        raise ValueError(f"unknown consistency form {consistency!r}: one of {CONSISTENCY_FORMS}")
    if not torch.is_tensor(pred) or pred.dim() != 4 or 0 in pred.shape:
        raise ValueError(f"pred must be a (B, C, H, W) tensor with no empty axis, got {tuple(pred.shape) if torch.is_tensor(pred) else pred!r}")
    Bn, C, H, W = pred.shape
    if not torch.is_tensor(target) or target.shape != pred.shape:
        raise ValueError(f"target must have pred's shape {tuple(pred.shape)}")
    if consistency is not None and (not torch.is_tensor(ema) or ema.shape != pred.shape):
        raise ValueError(f"the consistency term needs ema of pred's shape {tuple(pred.shape)}")
    if (quality or boundary) and (not torch.is_tensor(depth) or tuple(depth.shape) != (Bn, 1, H, W)):
        raise ValueError(f"the quality mask and the boundary term need depth of shape {(Bn, 1, H, W)}")
    quality, boundary, gradient = bool(quality), bool(boundary), bool(gradient)
    threshold, sharpness = float(threshold), float(sharpness)
    if consistency is None:
        ema = None
    if not (quality or boundary):
        depth = None
    if backend == "torch":
        return _terms_torch(pred, target, depth, ema, quality, consistency, boundary, gradient, threshold, sharpness)
    who = "cvs_quality_terms (backend 'hip')"
    _check_hip_tensors(who, pred, pred=pred, target=target, depth=depth, ema=ema)
    for name, t in (("target", target), ("depth", depth), ("ema", ema)):
        if t is not None and t.requires_grad:
            raise ValueError(f"{who}: {name} requires grad, but the gradient reaches pred only (detach it, or use backend 'torch')")
    if (boundary or gradient) and (H < 2 or W < 2):
        raise ValueError(f"{who}: the boundary and gradient terms need H >= 2 and W >= 2, got {H} x {W}")
    return _CvsTermsHip.apply(pred, target, depth, ema, _flags(quality, consistency, boundary, gradient), threshold, sharpness)


def consistency_euler_step(x0_pred: torch.Tensor, noisy: torch.Tensor, sqrt_alphas_cumprod: torch.Tensor, timestep: torch.Tensor, *,
                           backend: str = "torch"):
    """One Euler step from x_t towards the prediction (CVS:916-926): with a = sqrt_alphas_cumprod[t], a' = sqrt_alphas_cumprod[t'],
    t' = max(t - 1, 0): x_t' = clamp(a' x0 + (1 - a') / (1 - a + 1e-8) (noisy - a x0), -1, 1) -> (x_t', t'.float()).  Carries no
    graph: in the reference it only feeds the no_grad EMA forward.  backend "hip": fgs_cvs_euler_step, one launch; fp32 contiguous
    inputs, an int64 timestep; a timestep outside the table is clamped into it (torch would assert)."""
    _check_backend(backend)
    x0_pred, noisy = x0_pred.detach(), noisy.detach()
    if backend == "torch":
        t_prev = torch.clamp(timestep - 1, min=0)
        alpha_t = sqrt_alphas_cumprod[timestep][:, None, None, None]
        alpha_t_prev = sqrt_alphas_cumprod[t_prev][:, None, None, None]
        x_t_prev = alpha_t_prev * x0_pred + (1 - alpha_t_prev) / (1 - alpha_t + 1e-8) * (noisy - alpha_t * x0_pred)
        return torch.clamp(x_t_prev, -1, 1), t_prev.float()
    who = "consistency_euler_step (backend 'hip')"
    if x0_pred.dim() != 4 or 0 in x0_pred.shape or noisy.shape != x0_pred.shape:
        raise ValueError(f"{who}: x0_pred and noisy must be (B, C, H, W) of one shape, got {tuple(x0_pred.shape)} and {tuple(noisy.shape)}")
    Bn, C, H, W = x0_pred.shape
    _check_hip_tensors(who, x0_pred, x0_pred=x0_pred, noisy=noisy, sqrt_alphas_cumprod=sqrt_alphas_cumprod)
    if sqrt_alphas_cumprod.dim() != 1 or sqrt_alphas_cumprod.numel() < 1:
        raise ValueError(f"{who}: sqrt_alphas_cumprod must be a non-empty 1-D table, got {tuple(sqrt_alphas_cumprod.shape)}")
    if (not torch.is_tensor(timestep) or timestep.dtype is not torch.int64 or tuple(timestep.shape) != (Bn,) or not timestep.is_contiguous()
            or timestep.device != x0_pred.device):
        raise ValueError(f"{who}: timestep must be a contiguous int64 tensor of shape ({Bn},) on {x0_pred.device}")
    x_prev = torch.empty_like(x0_pred)
    t_prev = torch.empty(Bn, dtype=torch.float32, device=x0_pred.device)
    hip.call(x0_pred.device, "fgs_cvs_euler_step", Bn, C, H * W, sqrt_alphas_cumprod.numel(), sqrt_alphas_cumprod, timestep, x0_pred,
             noisy, x_prev, t_prev)
    return x_prev, t_prev


# ---- the reference's classes --------------------------------------------------------------------------------------------------------
class QualityAwareCVSLoss(nn.Module):
    """The loss of CVS training on Gaussian-rendered targets (QAL:153-302): quality-weighted L1, optional LPIPS, the L1 consistency
    with the EMA prediction, and the optional boundary and gradient terms.  -> {l1_weighted, [perceptual], [consistency], [boundary],
    [gradient], total}.  `backend` (a keyword and an attribute, "torch" as in the reference): with "hip" the pixel terms are ONE
    `cvs_quality_terms` call."""

    def __init__(self, lambda_l1: float = 1.0, lambda_perceptual: float = 0.5, lambda_consistency: float = 1.0,
                 lambda_boundary: float = 0.0, lambda_gradient: float = 0.0, use_quality_weighting: bool = True,
                 quality_threshold: float = 0.01, quality_sharpness: float = 100.0, backend: str = "torch"):
        super().__init__()
        self.lambda_l1 = lambda_l1
        self.lambda_perceptual = lambda_perceptual
        self.lambda_consistency = lambda_consistency
        self.lambda_boundary = lambda_boundary
        self.lambda_gradient = lambda_gradient
        self.use_quality_weighting = use_quality_weighting
        self.quality_threshold = quality_threshold
        self.quality_sharpness = quality_sharpness
        self.backend = _check_backend(backend)
        self.lpips_fn = None
        if lambda_perceptual > 0:
            try:
                import lpips
                self.lpips_fn = lpips.LPIPS(net='vgg').eval()
                for param in self.lpips_fn.parameters():
                    param.requires_grad = False
            except ImportError:
                print("Warning: lpips not installed. Perceptual loss disabled.")
                self.lambda_perceptual = 0.0

    def _perceptual(self, cvs_pred, synthetic_target):
        if next(self.lpips_fn.parameters()).device != cvs_pred.device:
            self.lpips_fn = self.lpips_fn.to(cvs_pred.device)
        return self.lpips_fn(cvs_pred, synthetic_target).mean()

    def forward(self, cvs_pred: torch.Tensor, synthetic_target: torch.Tensor, synthetic_depth: torch.Tensor,
                ema_pred: Optional[torch.Tensor] = None, consistency_weight_override: Optional[float] = None) -> Dict[str, torch.Tensor]:
        losses = {}
        total = 0.0
        want_boundary, want_gradient = self.lambda_boundary > 0, self.lambda_gradient > 0
        if _check_backend(self.backend) == "hip":
            terms = cvs_quality_terms(cvs_pred, synthetic_target, synthetic_depth, None if ema_pred is None else ema_pred.detach(),
                                      quality=self.use_quality_weighting, consistency=None if ema_pred is None else "l1",
                                      boundary=want_boundary, gradient=want_gradient, threshold=self.quality_threshold,
                                      sharpness=self.quality_sharpness, backend="hip")
            l1_weighted, consistency, boundary_loss, gradient_penalty = terms.unbind(0)
        else:
            if self.use_quality_weighting:
                quality_mask = compute_quality_mask(synthetic_depth, threshold=self.quality_threshold, sharpness=self.quality_sharpness)
            else:
                quality_mask = torch.ones_like(synthetic_depth)
            l1_pixelwise = F.l1_loss(cvs_pred, synthetic_target, reduction='none')
            l1_weighted = (l1_pixelwise * quality_mask).mean()
        losses['l1_weighted'] = l1_weighted
        total = total + self.lambda_l1 * l1_weighted
        if self.lambda_perceptual > 0 and self.lpips_fn is not None:
            perceptual = self._perceptual(cvs_pred, synthetic_target)
            losses['perceptual'] = perceptual
            total = total + self.lambda_perceptual * perceptual
        if ema_pred is not None:
            if self.backend == "torch":
                consistency = F.l1_loss(cvs_pred, ema_pred.detach())
            losses['consistency'] = consistency
            cons_weight = consistency_weight_override if consistency_weight_override is not None else self.lambda_consistency
            total = total + cons_weight * consistency
        if want_boundary:
            if self.backend == "torch":
                depth_grad_x = torch.abs(synthetic_depth[:, :, :, :-1] - synthetic_depth[:, :, :, 1:])
                depth_grad_y = torch.abs(synthetic_depth[:, :, :-1, :] - synthetic_depth[:, :, 1:, :])
                boundary_mask_x = (depth_grad_x > 0.01).float()
                boundary_mask_y = (depth_grad_y > 0.01).float()
                pixel_error = torch.abs(cvs_pred - synthetic_target).mean(dim=1, keepdim=True)
                boundary_loss = ((pixel_error[:, :, :, :-1] * boundary_mask_x).mean()
                                 + (pixel_error[:, :, :-1, :] * boundary_mask_y).mean())
            losses['boundary'] = boundary_loss
            total = total + self.lambda_boundary * boundary_loss
        if want_gradient:
            if self.backend == "torch":
                gradient_penalty = compute_gradient_penalty(cvs_pred, quality_mask)
            losses['gradient'] = gradient_penalty
            total = total + self.lambda_gradient * gradient_penalty
        losses['total'] = total
        return losses


class ConsistencyLoss(nn.Module):
    """The from-scratch consistency loss (CVS:844-941): L1 to the target, an L1 between `perceptual_net` features, and the MSE between
    the prediction and the EMA model's prediction one Euler step earlier.  -> {l1, perceptual, [consistency], total}, every entry
    already weighted.  `backend` (a keyword and an attribute, "torch" as in the reference): with "hip" the Euler step is ONE
    `consistency_euler_step` call and L1 and MSE ONE `cvs_quality_terms` call; `perceptual_net` and the EMA forward stay in torch."""

    def __init__(self, lambda_consistency: float = 1.0, lambda_reconstruction: float = 1.0, lambda_perceptual: float = 0.5,
                 backend: str = "torch"):
        super().__init__()
        self.lambda_consistency = lambda_consistency
        self.lambda_reconstruction = lambda_reconstruction
        self.lambda_perceptual = lambda_perceptual
        self.backend = _check_backend(backend)
        self.perceptual_net = nn.Sequential(
            nn.Conv2d(3, 64, 3, padding=1), nn.ReLU(),
            nn.Conv2d(64, 64, 3, padding=1), nn.ReLU(),
            nn.MaxPool2d(2),
            nn.Conv2d(64, 128, 3, padding=1), nn.ReLU(),
            nn.Conv2d(128, 128, 3, padding=1), nn.ReLU(),
            nn.MaxPool2d(2),
            nn.Conv2d(128, 256, 3, padding=1), nn.ReLU(),
        )

    def perceptual_loss(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return F.l1_loss(self.perceptual_net(pred), self.perceptual_net(target))

    def forward(self, model_output: Dict[str, torch.Tensor], ema_model: Optional[nn.Module] = None, model: Optional[nn.Module] = None,
                input_features: Optional[torch.Tensor] = None, R_rel: Optional[torch.Tensor] = None,
                t_rel: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        x0_pred, target = model_output['x0_pred'], model_output['target']
        noisy, timestep = model_output['noisy'], model_output['timestep']
        fused = _check_backend(self.backend) == "hip"
        with_ema = ema_model is not None and model is not None
        x0_ema = None
        if with_ema:
            x_t_prev, t_prev = consistency_euler_step(x0_pred, noisy, model.sqrt_alphas_cumprod, timestep, backend=self.backend)
            with torch.no_grad():
                image_cond = ema_model.image_adapter(input_features)
                pose_cond = ema_model.pose_encoder(R_rel, t_rel)
                x0_ema = ema_model.unet(x_t_prev, t_prev, image_cond, pose_cond).detach()
        if fused:
            terms = cvs_quality_terms(x0_pred, target, None, x0_ema, quality=False, consistency="mse" if with_ema else None,
                                      backend="hip")
            l1_loss, consistency_loss = terms[0], terms[1]
        else:
            l1_loss = F.l1_loss(x0_pred, target)
            consistency_loss = F.mse_loss(x0_pred, x0_ema) if with_ema else None
        losses = {}
        losses['l1'] = l1_loss * self.lambda_reconstruction
        losses['perceptual'] = self.perceptual_loss(x0_pred, target) * self.lambda_perceptual
        if with_ema:
            losses['consistency'] = consistency_loss * self.lambda_consistency
        losses['total'] = sum(losses.values())
        return losses
