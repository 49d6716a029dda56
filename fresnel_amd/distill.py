"""One training step of the distillation path (the reference's scripts/training/train_direct_decoder.py, "TDD"): a distillation
decoder (fresnel_amd/slat.py) predicts a Gaussian cloud from image features and voxel coordinates, GaussianMatchingLoss
(fresnel_amd/losses.py) scores it against the TRELLIS target, an occupancy term teaches WHICH voxels hold Gaussians.

With `head_backend` and `match_backend` on "hip" nothing in `distill_step` synchronises with the host: the decoder's NaN cleaning
is unconditional, the head and the matching loss run their fused kernels, the occupancy term is written without boolean indexing, and
the losses come back as detached device tensors.  Not kept from the reference's loop: the substitution of a dummy loss for a NaN / Inf
total (TDD:543-547, a host read), AMP / GradScaler, the dataset classes and RenderLoss.
"""
from dataclasses import dataclass
from typing import Dict

import torch
import torch.nn.functional as F


@dataclass
class DistillConfig:
    """The reference's TrainingConfig entries that a step reads (TDD:116-124, same names and defaults), and the two backends."""
    grad_clip: float = 1.0
    position_weight: float = 1.0
    scale_weight: float = 1.0
    rotation_weight: float = 0.5
    color_weight: float = 1.0
    opacity_weight: float = 5.0
    occupancy_weight: float = 2.0
    head_backend: str = "torch"
    match_backend: str = "torch"


def distill_losses(output, batch, matching_loss, cfg: DistillConfig) -> Dict[str, torch.Tensor]:
    """The losses of one batch as train_epoch forms them (TDD:500-528).  output: the decoder's dict (a bare tensor, MLPSLatDecoder's,
    counts as its `gaussians`); batch: `gaussians` (B, Nt, 14), `gaussian_mask` (B, Nt), `coord_mask` (B, N) and, optionally,
    `occupancy_target` (B, N).  -> the matching loss's seven keys, and with occupancy logits and a target `occupancy` = BCE with
    logits over the valid voxels -- sum(bce x coord_mask) / sum(coord_mask), the reference's mean over boolean-indexed entries
    without the indexing -- added to `total` with `occupancy_weight`."""
    if torch.is_tensor(output):
        output = {"gaussians": output}
    pred = output["gaussians"]
    if cfg.head_backend == "torch" and torch.isnan(pred).any():  # the reference's double-check (TDD:504-505); the hip head emits no NaN
        pred = torch.nan_to_num(pred, nan=0.0)
    losses = dict(matching_loss(pred, batch["gaussians"], pred_mask=None, target_mask=batch.get("gaussian_mask")))
    logits, target = output.get("occupancy_logits"), batch.get("occupancy_target")
    if logits is not None and target is not None:
        valid = batch["coord_mask"].to(logits.dtype)
        bce = F.binary_cross_entropy_with_logits(logits, target.to(logits.dtype), reduction="none")
        losses["occupancy"] = (bce * valid).sum() / valid.sum()
        losses["total"] = losses["total"] + cfg.occupancy_weight * losses["occupancy"]
    return losses


def distill_step(model, batch, optimizer, matching_loss, cfg: DistillConfig) -> Dict[str, torch.Tensor]:
    """zero_grad, forward, losses, backward, clip_grad_norm_(grad_clip), optimizer step (TDD:486-559 without AMP).  -> the losses,
    detached, on the device."""
    optimizer.zero_grad()
    output = model(batch["features"], batch["coords"], batch.get("coord_mask"))
    losses = distill_losses(output, batch, matching_loss, cfg)
    losses["total"].backward()
    torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.grad_clip)
    optimizer.step()
    return {k: v.detach() for k, v in losses.items()}
