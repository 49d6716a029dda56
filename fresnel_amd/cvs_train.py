"""One training step of the consistency view synthesizer (the reference's scripts/training/train_cvs.py, "TCV": CVSTrainer.train_step):
the synthesizer (fresnel_amd/cvs.py) predicts the target view from a noised copy of it, QualityAwareCVSLoss or ConsistencyLoss
(fresnel_amd/cvs_losses.py) scores the prediction, an exponential moving average of the weights gives the consistency target.

With `loss_backend` "hip" nothing from the losses onward synchronises with the host: the pixel terms and the Euler step run their fused
kernels, whose checks read no device data, and the losses come back as detached device tensors -- unlike the reference, which calls
`.item()` on each.  Not kept from the reference's loop: the two dataset classes, the learning-rate warm-up and scheduler, validation,
checkpoint files and the command line.
"""
from dataclasses import dataclass
from typing import Dict

import torch

from .cvs import update_ema
from .cvs_losses import ConsistencyLoss, QualityAwareCVSLoss, get_consistency_weight_schedule


@dataclass
class CVSTrainConfig:
    """The reference's TrainingConfig entries that a step reads (TCV:72-101, same names and defaults), and the loss backend."""
    epochs: int = 100
    gradient_clip: float = 1.0
    ema_decay: float = 0.9999
    lambda_consistency: float = 1.0
    lambda_reconstruction: float = 1.0
    lambda_perceptual: float = 0.5
    use_gaussian_targets: bool = False
    quality_weighting: bool = True
    progressive_consistency: bool = True
    lambda_boundary: float = 0.0
    lambda_gradient: float = 0.0
    loss_backend: str = "torch"


def make_cvs_loss(cfg: CVSTrainConfig):
    """The loss module CVSTrainer builds for `cfg` (TCV:380-399): QualityAwareCVSLoss with Gaussian targets, else ConsistencyLoss."""
    if cfg.use_gaussian_targets:
        return QualityAwareCVSLoss(lambda_l1=cfg.lambda_reconstruction, lambda_perceptual=cfg.lambda_perceptual,
                                   lambda_consistency=cfg.lambda_consistency, lambda_boundary=cfg.lambda_boundary,
                                   lambda_gradient=cfg.lambda_gradient, use_quality_weighting=cfg.quality_weighting,
                                   backend=cfg.loss_backend)
    return ConsistencyLoss(lambda_consistency=cfg.lambda_consistency, lambda_reconstruction=cfg.lambda_reconstruction,
                           lambda_perceptual=cfg.lambda_perceptual, backend=cfg.loss_backend)


def cvs_losses(model, ema_model, batch, loss_fn, cfg: CVSTrainConfig, epoch: int) -> Dict[str, torch.Tensor]:
    """Forward and losses of one batch, both paths of train_step (TCV:457-510).  batch: `input_image`, `target_image`, `features`,
    `R_rel`, `t_rel` and, with `use_gaussian_targets`, `target_depth`.  Quality-aware path: the EMA model's prediction of the same
    batch under no_grad is the consistency target, weighted by the progressive schedule of `epoch` when `progressive_consistency`.
    Standard path: ConsistencyLoss runs the EMA model itself, one Euler step earlier.  `loss_fn.backend` is set to `loss_backend`."""
    loss_fn.backend = cfg.loss_backend
    input_image, target_image, features = batch['input_image'], batch['target_image'], batch['features']
    R_rel, t_rel = batch['R_rel'], batch['t_rel']
    output = model(input_image, features, R_rel, t_rel, target_image=target_image)
    if cfg.use_gaussian_targets:
        with torch.no_grad():
            ema_output = ema_model(input_image, features, R_rel, t_rel, target_image=target_image)
        consistency_weight = None
        if cfg.progressive_consistency:
            consistency_weight = get_consistency_weight_schedule(epoch, cfg.epochs, schedule_type='progressive')
        return loss_fn(cvs_pred=output['x0_pred'], synthetic_target=target_image, synthetic_depth=batch['target_depth'],
                       ema_pred=ema_output['x0_pred'], consistency_weight_override=consistency_weight)
    return loss_fn(output, ema_model=ema_model, model=model, input_features=features, R_rel=R_rel, t_rel=t_rel)


def cvs_step(model, ema_model, batch, optimizer, loss_fn, cfg: CVSTrainConfig, epoch: int) -> Dict[str, torch.Tensor]:
    """model.train(), forward, losses, zero_grad, backward, clip_grad_norm_(gradient_clip) when positive, optimizer step, update_ema
    (TCV:457-528).  -> the losses, detached, on the device."""
    model.train()
    losses = cvs_losses(model, ema_model, batch, loss_fn, cfg, epoch)
    optimizer.zero_grad()
    losses['total'].backward()
    if cfg.gradient_clip > 0:
        torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.gradient_clip)
    optimizer.step()
    update_ema(model, ema_model, cfg.ema_decay)
    return {k: v.detach() for k, v in losses.items()}
