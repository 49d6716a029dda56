"""One training step of the distillation path (the reference's scripts/training/train_direct_decoder.py, "TDD"): a distillation
decoder (fresnel_amd/slat.py) predicts a Gaussian cloud from image features and voxel coordinates, GaussianMatchingLoss
(fresnel_amd/losses.py) scores it against the TRELLIS target, an occupancy term teaches WHICH voxels hold Gaussians.

With `head_backend` and `match_backend` on "hip" nothing in the fp32 `distill_step` synchronises with the host: the decoder's NaN
cleaning is unconditional, the head and the matching loss run their fused kernels, the occupancy term is written without boolean
indexing, and the losses come back as detached device tensors.

Mixed precision is kept from the reference's loop (its `use_amp`, on by default: TDD:495-559).  `DistillConfig.amp_dtype` runs the
forward and the losses under `torch.autocast("cuda", dtype=amp_dtype)`; a `scaler` (torch.amp.GradScaler) makes the backward the
reference's sequence scale -> backward -> unscale_ -> clip_grad_norm_ -> step -> update.  The reference's configuration is
amp_dtype=torch.float16 with a scaler; bf16 needs none.  A decoder built with attn_backend="hip", attn_dtype="autocast" then runs
the 16-bit fused attention on the Linear layers' 16-bit outputs as they are; the fused head and the matching loss keep casting
their inputs to fp32.  Where the AMP step still synchronises: `GradScaler.step` reads its found-inf flag on the host (one
`.item()` per step) unless the optimizer takes the scaling itself (fused AdamW does: it skips on the device); with bf16 and no scaler
nothing is read on the host.

Not kept from the reference's loop: the substitution of a dummy loss for a NaN / Inf total (TDD:543-547, a host read), the dataset
classes and RenderLoss.
"""
from dataclasses import dataclass
from typing import Dict, Optional

import torch
import torch.nn.functional as F


@dataclass
class DistillConfig:
    """The reference's TrainingConfig entries that a step reads (TDD:116-124, same names and defaults), the two backends, and
    `amp_dtype`: None (fp32, the default here) or the autocast dtype of the step -- the reference's use_amp=True is torch.float16."""
    grad_clip: float = 1.0
    position_weight: float = 1.0
    scale_weight: float = 1.0
    rotation_weight: float = 0.5
    color_weight: float = 1.0
    opacity_weight: float = 5.0
    occupancy_weight: float = 2.0
    head_backend: str = "torch"
    match_backend: str = "torch"
    amp_dtype: Optional[torch.dtype] = None


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


def distill_step(model, batch, optimizer, matching_loss, cfg: DistillConfig, scaler=None) -> Dict[str, torch.Tensor]:
    """zero_grad, forward, losses, backward, clip_grad_norm_(grad_clip), optimizer step (TDD:486-559).  -> the losses, detached, on
    the device.  With cfg.amp_dtype the forward and the losses run under CUDA autocast in that dtype; with a `scaler` (a
    torch.amp.GradScaler; needs amp_dtype) the backward is scale(total).backward(), unscale_(optimizer), the clip, scaler.step(optimizer),
    scaler.update() (TDD:550-555): a step whose gradients overflowed leaves the parameters alone and halves the scale.  With neither,
    the plain fp32 step."""
    if scaler is not None and cfg.amp_dtype is None:
        raise ValueError("distill_step: a scaler needs cfg.amp_dtype (the reference scales only under autocast)")
    optimizer.zero_grad()
    if cfg.amp_dtype is None:
        output = model(batch["features"], batch["coords"], batch.get("coord_mask"))
        losses = distill_losses(output, batch, matching_loss, cfg)
    else:
        with torch.autocast("cuda", dtype=cfg.amp_dtype):
            output = model(batch["features"], batch["coords"], batch.get("coord_mask"))
            losses = distill_losses(output, batch, matching_loss, cfg)
    if scaler is None:
        losses["total"].backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.grad_clip)
        optimizer.step()
    else:
        scaler.scale(losses["total"]).backward()
        scaler.unscale_(optimizer)
        torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.grad_clip)
        scaler.step(optimizer)
        scaler.update()
    return {k: v.detach() for k, v in losses.items()}
