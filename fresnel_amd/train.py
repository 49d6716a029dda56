#!/usr/bin/env python3
"""Training harness around the HIP rasterizer: this repo's counterpart of the reference's
scripts/training/train_gaussian_decoder.py ("TGD") for the path BASELINE.json names.

Kept from TGD (same flag names / defaults / behaviour):
  flags             --experiment --data_dir --output_dir --batch_size --epochs --lr --image_size
                    --gaussians_per_patch --max_images --use_fresnel_zones --num_fresnel_zones
                    --use_phase_blending --phase_amplitude --resume            TGD:1401-1545
                    --use_edge_aware --edge_scale_factor --stochastic_k --progressive_schedule --train_resolution
                    --fast_mode --multi_pose_augmentation --pose_range_elevation/azimuth --frontal_prob
                    --use_pose_encoding                                         TGD:1455-1461, 1524-1545
  data              ImageDataset over --data_dir with the `features/` caches (fresnel_amd/data.py, TGD:525-675);
                    synthetic stand-in data only when --data_dir holds no images
  hand-off          progressive Gaussians-per-patch, importance subsampling of K Gaussians, one orbit camera per
                    batch (fresnel_amd/handoff.py, TGD:1069-1207)
  decoder           --decoder standin (default: PatchGaussianDecoder, own head) | direct | fibonacci: mirrors of the reference's
                    DirectPatchDecoder / FibonacciPatchDecoder (its keys: --resume takes its checkpoints), constructed as at
                    TGD:1814-1840; --experiment 4 implies fibonacci; --head_backend hip runs their head as fused HIP kernels;
                    --experiment 5 implies nca: NCAGaussianDecoder (TGD:1841-1849; --nca_steps, --nca_neighbors, --nca_step_size),
                    --nca_backend hip runs its neighbour perception and update as HIP kernels (csrc/fgs_nca.hip);
                    --experiment 1 implies saag: SAAGRefinementNet refines the dataset's SAAG clouds (`{name}_saag.bin`; a dummy
                    cloud of 1000 Gaussians where a batch has none, TGD:1043-1067), the residual regulariser --residual_weight
                    (TGD:932-939) joins the loss, --saag_backend hip runs its input gather and residual head as HIP kernels
                    (csrc/fgs_saag.hip);
                    --experiment 3 --decoder guided_saag: FeatureGuidedSAAG (GDM:1422-1490) predicts six per-patch parameter maps
                    and fresnel_amd.surface.guided_surface_gaussians builds every batch image's SAAG cloud from its own depth map
                    under them (csrc/fgs_surface.hip, differentiable with respect to the maps; --surface_subsample); refused with
                    --hip_graph, --stochastic_k and --fast_mode; bare --experiment 3 (the reference's dummy-cloud step, TGD:1135-1152) stays refused;
                    --decoder physics: PhysicsDirectPatchDecoder (TGD:1803-1810; --wavelength, --learnable_wavelength,
                    --focal_depth, --use_diffraction_placement), the reference's decoder for --use_wave_rendering without
                    --use_qsr: (B,N) phases computed from the depth; --head_backend hip runs its head as HIP kernels
                    (csrc/fgs_physics.hip); called without elevation / azimuth (the class takes neither)
  renderer choice   TileBasedRenderer(res, res, use_phase_blending, phase_amplitude)   TGD:1898-1907;
                    --experiment 4 --use_phase_blending: FourierGaussianRenderer(res, res, 0.65, 0.55, 0.45)  TGD:1877-1890
  camera            fx = fy = 0.8*res, cx = cy = res/2, view = I                       TGD:1910-1917
  step              decoder -> render -> stack -> L1 + normalised-depth L1 (SSIM / LPIPS only when
                    those packages exist, as TGD:53-65; --ssim_backend hip computes the SSIM term with this
                    package's HIP kernels, fresnel_amd/losses.py, whether pytorch_msssim exists or not); the L1 weighted by
                    the VLM density maps with --use_vlm_guidance / --vlm_weight (TGD:875-888) and the Fresnel-zone boundary
                    emphasis term with --use_fresnel_zones --boundary_weight W (TGD:941-953; W defaults to 0 here, 0.1 in the
                    reference); --pixel_loss_backend hip takes L1, boundary and depth terms from one family of HIP kernels
                    (fresnel_amd/losses.py pixel_losses) -> NaN/Inf skip -> backward ->
                    clip_grad_norm_(1.0) -> AdamW(lr, weight_decay=1e-5) ; CosineAnnealingLR
                                                                    TGD:890, 922-930, 1255-1266, 1970-1971
  data order        a fresh permutation of the images every epoch (DataLoader(shuffle=True), TGD:1760-1767), drawn
                    from seed + epoch so that every rank draws the same one; the last, partial batch is kept when it
                    divides over the ranks; batches are decoded ahead of the step by worker processes / a prefetch thread
                    into pinned memory
  checkpoints       {epoch, model_state_dict, optimizer_state_dict, losses, config}    TGD:1304-1310
  metrics           print every log_interval batches (TGD:1275-1281); training_history_exp{E}.json (TGD:1317-1323) with
                    the per-epoch losses plus step ms, composited Gaussian-pixels/s and the rasterizer's stage ms
Changed on purpose:
  * the per-image Python loop TGD:1209-1223 becomes ONE batched renderer call;
  * NO host synchronisation inside a step: loss terms stay on the device and are fetched once per log_interval; the
    NaN/Inf batch skip (TGD:1255-1258) is decided on the device -- the flag rides in the gradient bucket's all-reduce
    and the fused AdamW step takes it as `found_inf` (weights, moments and step count untouched, exactly a skipped
    batch).  The reference syncs ~5 times per Gaussian (.item(), DR:584-597) plus once per loss term;
  * image-wise data parallelism: one process per GPU, the batch is sharded by image and the
    decoder gradients are all-reduced once per step over RCCL (fresnel_amd/dist.py);
  * no dataset preprocessing tooling (DINOv2 / depth extraction): caches are read when present; when --data_dir has
    no images the harness fabricates images/features like TGD:1748-1758 / TGD:613-630 do when files are missing.

    python -m fresnel_amd.train --experiment 2 --epochs 1                      # 1 GPU
    python -m torch.distributed.run --nproc-per-node 8 -m fresnel_amd.train    # 8 GPUs, DP
"""
import argparse
import inspect
import json
import math
import os
import queue
import threading
import time
from dataclasses import asdict, dataclass
from pathlib import Path
from typing import Callable, Dict, Optional

import torch
import torch.nn.functional as F
from torch.optim import AdamW
from torch.optim.lr_scheduler import CosineAnnealingLR

import numpy as np

from .decoder import (HEAD_BACKENDS, NCA_BACKENDS, SAAG_BACKENDS, DirectPatchDecoder, FeatureGuidedSAAG, FibonacciPatchDecoder,
                      NCAGaussianDecoder, PatchGaussianDecoder, PhysicsDirectPatchDecoder, SAAGRefinementNet)
from .data import collate_host_items
from .dist import DPContext
from .handoff import HFTSConfig, camera_for_batch, importance_subsample, sample_training_pose

try:  # optional perceptual losses, exactly like TGD:53-65
    from pytorch_msssim import ssim as ssim_fn
    SSIM_AVAILABLE = True
except ImportError:
    SSIM_AVAILABLE = False


@dataclass
class TrainingConfig:  # subset of TGD:97-162 that this path uses; same names and defaults
    experiment: int = 2
    data_dir: str = "images"
    output_dir: str = "checkpoints"
    batch_size: int = 4
    epochs: int = 100
    lr: float = 1e-4
    weight_decay: float = 1e-5
    image_size: int = 256
    feature_size: int = 37
    feature_dim: int = 384
    rgb_weight: float = 1.0
    depth_weight: float = 0.1
    ssim_weight: float = 0.5
    ssim_backend: str = "msssim"  # "msssim": pytorch_msssim's term when the package is importable, none otherwise (TGD:53-65);
                                  # "hip": the same term from fresnel_amd.losses.ssim (HIP kernels, needs a GPU)
    use_vlm_guidance: bool = False   # weight the L1 term by the dataset's VLM density maps (TGD:140-141, 875-888)
    vlm_weight: float = 0.5
    boundary_weight: float = 0.0     # Fresnel-zone boundary emphasis term (TGD:146, 941-953), active under use_fresnel_zones.
                                     # The reference's default is 0.1; it is 0 here so that runs configured before the term
                                     # existed compute what they computed: pass --boundary_weight 0.1 for the reference's loss
    pixel_loss_backend: str = "torch"  # "torch": L1 / boundary / depth terms as torch expressions; "hip": the same terms from
                                       # fresnel_amd.losses.pixel_losses (HIP kernels, needs a GPU)
    gaussians_per_patch: int = 4
    max_images: Optional[int] = None
    use_fresnel_zones: bool = False
    num_fresnel_zones: int = 8
    use_phase_blending: bool = False
    phase_amplitude: float = 0.25
    use_edge_aware: bool = False      # smaller / more opaque Gaussians at depth edges (TGD:147-151)
    edge_scale_factor: float = 0.5
    edge_opacity_boost: float = 0.2
    multi_pose_augmentation: bool = False  # one random orbit pose per batch (TGD:155-159)
    pose_range_elevation: tuple = (-30.0, 45.0)
    pose_range_azimuth: tuple = (0.0, 360.0)
    frontal_prob: float = 0.3
    use_pose_encoding: bool = False
    use_wave_rendering: bool = False  # WaveFieldRenderer (TGD:178, 1891-1897); --use_qsr implies it
    # spectral / stencil losses after the renderer (TGD:191, 225-229; fresnel_amd/losses.py)
    wave_equation_weight: float = 0.0
    wavelength: float = 0.05
    learnable_wavelength: bool = False   # --decoder physics: the command line's default (TGD:1473)
    focal_depth: float = 0.5
    use_physics_zones: bool = False      # parsed as the reference parses it; selects nothing by itself here
    use_diffraction_placement: bool = False
    use_phase_retrieval_loss: bool = False
    phase_retrieval_weight: float = 0.1
    use_frequency_loss: bool = False
    frequency_loss_weight: float = 0.1
    device: str = "cuda" if torch.cuda.is_available() else "cpu"
    log_interval: int = 10
    save_interval: int = 10
    seed: int = 0
    steps_per_epoch: int = 8  # synthetic-data mode only
    num_workers: int = 4      # host threads decoding the NEXT batches (DataLoader(num_workers=4), TGD:1760-1767)
    hip_graph: bool = False   # replay the whole step (decoder, rasterizer, losses, backward, all-reduce, clip, AdamW) from
                              # ONE captured HIP graph: the library never allocates or synchronises and the step has no
                              # host decision left, so it is capturable; pays when the step is host-launch-bound
    decoder: str = "standin"  # "standin": PatchGaussianDecoder (own head, shapes and ranges of the reference only) | "direct" |
                              # "fibonacci": mirrors of the reference's DirectPatchDecoder / FibonacciPatchDecoder (fresnel_amd/
                              # decoder.py: its state_dict keys, its head); --experiment 4 implies "fibonacci" (TGD:1829-1841)
    head_backend: str = "torch"  # Gaussian-parameter head of "direct" / "fibonacci": torch expressions | "hip" (csrc/fgs_head.hip)
    n_spiral_points: int = 377   # "fibonacci" / "nca": points of the golden-angle spiral (TGD:1427)
    # "nca" (--experiment 5, TGD:1842-1849): steps and neighbours of the automaton (TGD:1435-1440), the backend of its neighbour
    # perception and update (torch: cdist / topk / gather | hip: csrc/fgs_nca.hip), and the INITIAL value of the learnable step
    # size -- the reference parses --nca_step_size and never passes it on (TGD:1844-1849); the default is the class's own 0.1
    nca_steps: int = 16
    nca_neighbors: int = 6
    nca_backend: str = "torch"
    nca_step_size: float = 0.1
    # "saag" (--experiment 1, TGD:1043-1067): backend of SAAGRefinementNet's input gather and residual head (torch: the
    # reference's ops | hip: csrc/fgs_saag.hip) and the weight of the residual regulariser (TGD:120, 932-939)
    saag_backend: str = "torch"
    # "guided_saag" (--experiment 3 --decoder guided_saag): FeatureGuidedSAAG's maps modulate the SAAG generator, which builds every
    # batch image's cloud from its own depth map on one point per surface_subsample x surface_subsample pixels (4: 4 096 points
    # and at most 49 152 rows at 256 x 256 -- a setting, not a measured optimum)
    surface_subsample: int = 4
    residual_weight: float = 0.01
    workspace: str = "worst"  # rasterizer workspaces: "worst" (sized for the radius cap) | "adaptive" (sized by the duplicates
                              # the previous steps needed, TileBasedRenderer(workspace="adaptive"); a step whose scene outgrew
                              # the capacity renders NaN and is dropped by the NaN/Inf skip, the next one has room)


class SyntheticDataset:
    """Stand-in for TGD's ImageDataset when no caches exist: random images, zero-mean random
    features, smooth random depth (TGD:613-630 returns zero features/depth for missing caches;
    TGD:1748-1758 fabricates random PNGs).  Deterministic in the GLOBAL sample index so every DP
    configuration sees the same data."""

    def __init__(self, n_items, cfg: TrainingConfig):
        self.n, self.cfg = n_items, cfg

    def get(self, idx):
        g = torch.Generator().manual_seed(self.cfg.seed * 1_000_003 + idx)
        S, Fs = self.cfg.image_size, self.cfg.feature_size
        low = torch.rand(3, 8, 8, generator=g)
        image = F.interpolate(low[None], size=(S, S), mode="bilinear", align_corners=False)[0]
        feats = torch.randn(Fs, Fs, self.cfg.feature_dim, generator=g) * 0.5
        dlow = torch.rand(1, 4, 4, generator=g)
        depth = F.interpolate(dlow[None], size=(S, S), mode="bilinear", align_corners=False)[0]
        if self.cfg.use_vlm_guidance:  # a smooth density map in [0.5, 1.5], the range ImageDataset produces (TGD:659-661)
            vlow = torch.rand(1, 6, 6, generator=g)
            density = 0.5 + F.interpolate(vlow[None], size=(S, S), mode="bilinear", align_corners=False)[0]
            return image, feats, depth, density
        return image, feats, depth

    def __len__(self):
        return self.n

    def host_item(self, idx):
        return self.get(idx)

    def batch(self, indices, device):
        items = [self.get(i) for i in indices]
        return tuple(torch.stack(t).to(device) for t in zip(*items))


def epoch_batches(n_items: int, batch_size: int, world: int, seed: int, epoch: int):
    """Global batches of one epoch as index lists: a fresh permutation per epoch (DataLoader(shuffle=True),
    TGD:1760-1767) from a generator seeded with seed + epoch -- every rank draws the SAME permutation and takes its
    shard of each batch.  The last, partial batch is kept, as the reference keeps it, when it divides over the ranks
    (equal shards: the mean of shard means stays the global mean); otherwise it is dropped."""
    perm = torch.randperm(n_items, generator=torch.Generator().manual_seed(seed + epoch)).tolist()
    out = [perm[i:i + batch_size] for i in range(0, n_items - batch_size + 1, batch_size)]
    tail = perm[len(out) * batch_size:]
    if tail and len(tail) % world == 0:
        out.append(tail)
    return out


class BatchPrefetcher:
    """Iterates device batches for a list of index lists, decoding AHEAD of the training step: `num_workers` host
    threads load items (PIL decode / LANCZOS resize / cache reads release the GIL), a producer thread stacks them into
    pinned memory, at most `depth` batches wait in the queue, and the copy to the GPU is asynchronous.  The reference
    gets the same overlap from DataLoader(num_workers=4, pin_memory=True) worker processes (TGD:1760-1767)."""

    def __init__(self, data, index_lists, device, num_workers=4, depth=2):
        self.data, self.lists, self.device = data, index_lists, torch.device(device)
        self.q = queue.Queue(maxsize=max(1, depth))
        self.pin = self.device.type == "cuda"
        self.workers = max(1, int(num_workers))
        self.stop = threading.Event()
        self.thread = threading.Thread(target=self._produce, daemon=True)
        self.thread.start()

    def _put(self, item):
        """Queue `item` unless the consumer has gone away (close()): never blocks for good."""
        while not self.stop.is_set():
            try:
                self.q.put(item, timeout=0.1)
                return True
            except queue.Full:
                pass
        return False

    def _produce(self):
        from concurrent.futures import ThreadPoolExecutor
        try:
            with ThreadPoolExecutor(self.workers) as pool:
                for idx in self.lists:
                    if self.stop.is_set():
                        return
                    items = list(pool.map(self.data.host_item, idx))
                    batch = collate_host_items(items, getattr(self.data, "saag_tensors", 0))
                    if self.pin:
                        batch = tuple(t.pin_memory() for t in batch)
                    if not self._put(batch):
                        return
            self._put(None)
        except BaseException as e:  # surfaces in the consumer, not in a dead thread
            self._put(e)

    def close(self):
        """Stop the producer and drop what it queued (pinned batches).  Called when the consumer leaves the loop for
        any reason -- exhaustion, `break`, an exception in the training step -- so no thread is left blocked in `put`."""
        self.stop.set()
        while True:
            try:
                self.q.get_nowait()
            except queue.Empty:
                break
        self.thread.join(timeout=5.0)

    def __iter__(self):
        try:
            while True:
                b = self.q.get()
                if b is None:
                    return
                if isinstance(b, BaseException):
                    raise b
                yield tuple(t.to(self.device, non_blocking=True) for t in b)
        finally:
            self.close()


def _global_mean_std(x, dp):
    """mean and unbiased std (torch.std default, as TGD:922-925 uses) of x over the GLOBAL batch, TWO-PASS like
    torch.std: the sum is all-reduced for the mean, then the sum of squared deviations (the one-pass
    sum x^2 - n mean^2 loses digits to cancellation for ~2 M depth values whose mean is far from zero).  Both
    all-reduces are differentiable, so an N-rank step normalises the depth loss exactly like the 1-rank step."""
    dist_on = dp is not None and dp.enabled
    n = x.numel() * (dp.world if dist_on else 1)
    s1 = x.sum()
    if dist_on:
        s1 = dp.global_sum(s1.reshape(1))[0]
    mean = s1 / n
    s2 = ((x - mean) ** 2).sum()
    if dist_on:
        s2 = dp.global_sum(s2.reshape(1))[0]
    return mean, torch.sqrt(s2 / max(n - 1, 1))


SSIM_BACKENDS = ("msssim", "hip")
PIXEL_LOSS_BACKENDS = ("torch", "hip")


def _ssim_term_fn(cfg: TrainingConfig):
    """The SSIM function of the step, or None: pytorch_msssim's when importable (cfg.ssim_backend "msssim", the
    reference's behaviour), the HIP kernels' always ("hip")."""
    if cfg.ssim_backend == "msssim":
        return ssim_fn if SSIM_AVAILABLE else None
    if cfg.ssim_backend == "hip":
        from .losses import ssim as hip_ssim
        return hip_ssim
    raise ValueError(f"unknown ssim_backend {cfg.ssim_backend!r}: one of {SSIM_BACKENDS}")


RESIDUAL_KEYS = ("pos_delta", "scale_delta", "color_delta", "opacity_delta")
SAAG_NAMES = ("positions", "scales", "rotations", "colors", "opacities")
DUMMY_SAAG_POINTS = 1000


def create_dummy_saag(batch_size: int, num_gaussians: int, device, generator: Optional[torch.Generator] = None):
    """The stand-in cloud of the reference's training script (TGD:760-778) for a batch without SAAG binaries: positions
    N(0, 0.5) with z moved to -2, scales 0.05, identity quaternions, uniform colours, opacity 0.8 -- drawn on `device` from
    `generator` (the step's), in the reference's order (positions, then colours).  -> the five tensors in SAAG_NAMES order."""
    positions = torch.randn(batch_size, num_gaussians, 3, device=device, generator=generator) * 0.5
    positions[..., 2] -= 2
    rotations = torch.zeros(batch_size, num_gaussians, 4, device=device)
    rotations[..., 0] = 1
    colors = torch.rand(batch_size, num_gaussians, 3, device=device, generator=generator)
    return (positions, torch.full((batch_size, num_gaussians, 3), 0.05, device=device), rotations, colors,
            torch.full((batch_size, num_gaussians), 0.8, device=device))


GUIDED_PAD_Z = -1.0e6  # a padding row's position: beyond the far plane of every training camera (far = 100)


def guided_saag_clouds(model, feats, depth, images, cfg: "TrainingConfig"):
    """The --experiment 3 step's Gaussians: FeatureGuidedSAAG turns the batch's features (B,37,37,C) into six parameter maps,
    surface.guided_surface_gaussians builds every image's SAAG cloud from its OWN depth map (B,1,S,S) and target image under
    those maps (HIP, differentiable with respect to the maps; one host read, of the row offsets; the viewer's parameters except
    that the cloud is left un-normalised, in the training camera's frame), and the clouds are padded to
    the batch's largest count with rows the rasterizer culls (depth past the far plane, opacity 0): they reach no tile and get
    no gradient.  -> dict of (B,N,.) tensors for the renderer.  (The reference's step, TGD:1135-1152, renders a 500-point random
    cloud scaled by the mean of two of the maps instead: four maps never get a gradient there.)"""
    from .surface import KEYS, SurfaceGaussianParams, guided_surface_gaussians
    mods = model(feats.permute(0, 3, 1, 2))
    # normalize_extent 0: the generator's un-normalised points are the depth map's own unprojection under fx = 0.8 W, cx = W / 2 --
    # the training camera (TGD:1910-1917) -- so every Gaussian lands on the pixel it came from.  (The viewer's centring and
    # normalisation would put the cloud AROUND that camera: half of it behind the near plane, the frame's border outside the view.)
    params = SurfaceGaussianParams(subsample=cfg.surface_subsample, normalize_extent=0.0)
    clouds = guided_surface_gaussians(depth.detach(), images.detach(), mods, params)
    n = max(max(c["positions"].shape[0] for c in clouds), 1)
    out = {}
    for k in KEYS:
        rows = []
        for c in clouds:
            t = c[k]
            pad = t.new_zeros((n - t.shape[0],) + tuple(t.shape[1:]))
            if k == "positions":
                pad[:, 2] = GUIDED_PAD_Z
            elif k == "scales":
                pad.fill_(1e-3)
            elif k == "rotations":
                pad[:, 0] = 1.0
            rows.append(torch.cat([t, pad]) if pad.shape[0] else t)
        out[k] = torch.stack(rows)
    return out


def compute_losses(rendered, target, rendered_depth, target_depth, cfg: TrainingConfig, dp=None, vlm_density=None, residuals=None):
    """L1 + SSIM term + normalised depth L1 + zone-boundary term (TGD:875-953).  The SSIM term, cfg.ssim_weight * (1 - SSIM(clamp(rendered,
    0, 1), target)), comes from pytorch_msssim when that package is importable and is left out otherwise
    (cfg.ssim_backend "msssim", TGD:53-65), or from fresnel_amd.losses.ssim's HIP kernels (cfg.ssim_backend "hip", CUDA/ROCm
    tensors only).  The L1 is weighted by (1 - vlm_weight) + vlm_weight * vlm_density when a density map (B,1,h,w) is given,
    cfg.use_vlm_guidance is set and cfg.vlm_weight > 0 (TGD:875-888); the boundary term, cfg.boundary_weight * mean(mask *
    mean_c |rendered - target|) with the mask of cfg.num_fresnel_zones zones on (0, 1), is added under cfg.use_fresnel_zones
    when cfg.boundary_weight > 0 and a target depth exists (TGD:943-953, 1952-1959).  cfg.pixel_loss_backend "hip" takes the
    L1, boundary and depth terms from fresnel_amd.losses.pixel_losses (CUDA/ROCm tensors only; under data parallelism two or
    three small sum all-reduces forward and none backward), "torch" from the expressions below.  Returns (total, terms):
    `terms` holds the individual losses as DETACHED 0-d DEVICE tensors -- nothing here
    synchronises with the host (the reference's `.item()` per term, TGD:891-1001, would cost a device round trip each).
    residuals (--experiment 1; None for every other step): the decoder's pos_delta / scale_delta / color_delta / opacity_delta;
    cfg.residual_weight * sum_k mean|residuals[k]| is added and reported as terms["residual"] (TGD:932-939)."""
    d: Dict[str, torch.Tensor] = {}
    if cfg.pixel_loss_backend not in PIXEL_LOSS_BACKENDS:
        raise ValueError(f"unknown pixel_loss_backend {cfg.pixel_loss_backend!r}: one of {PIXEL_LOSS_BACKENDS}")
    use_vlm = vlm_density is not None and cfg.use_vlm_guidance and cfg.vlm_weight > 0
    use_boundary = cfg.use_fresnel_zones and cfg.boundary_weight > 0 and target_depth is not None
    px = None
    if cfg.pixel_loss_backend == "hip":
        if not rendered.is_cuda:
            raise ValueError("pixel_loss_backend 'hip' needs the rendered batch on a GPU: the HIP pixel-loss kernels have no CPU fallback")
        from .losses import pixel_losses
        dist_on = dp is not None and dp.enabled
        px = pixel_losses(rendered, target, rendered_depth, target_depth, density=vlm_density if use_vlm else None,
                          vlm_weight=cfg.vlm_weight, zones=cfg.num_fresnel_zones if use_boundary else None,
                          reduce_fn=dp.sum_in_place if dist_on else None, world=dp.world if dist_on else 1)
        rgb = px["rgb"]
    elif use_vlm:
        w = vlm_density.detach()
        if w.shape[-2:] != rendered.shape[-2:]:
            w = F.interpolate(w, size=rendered.shape[-2:], mode="bilinear", align_corners=False)
        rgb = (torch.abs(rendered - target) * ((1.0 - cfg.vlm_weight) + cfg.vlm_weight * w)).mean()
    else:
        rgb = F.l1_loss(rendered, target)
    d["rgb"] = rgb.detach()
    total = cfg.rgb_weight * rgb
    ssim_term = _ssim_term_fn(cfg) if cfg.ssim_weight > 0 else None
    if ssim_term is not None:
        if cfg.ssim_backend == "hip" and not rendered.is_cuda:
            raise ValueError("ssim_backend 'hip' needs the rendered batch on a GPU: the HIP SSIM kernels have no CPU fallback")
        s = 1.0 - ssim_term(torch.clamp(rendered, 0, 1), target, data_range=1.0, size_average=True)
        d["ssim"] = s.detach()
        total = total + cfg.ssim_weight * s
    if px is not None:
        if "depth" in px:
            d["depth"] = px["depth"].detach()
            total = total + cfg.depth_weight * px["depth"]
    elif rendered_depth is not None and target_depth is not None:
        rd_mean, rd_std = _global_mean_std(rendered_depth, dp)
        td_mean, td_std = _global_mean_std(target_depth, dp)
        dl = F.l1_loss((rendered_depth - rd_mean) / torch.clamp(rd_std, min=1e-4),
                       (target_depth - td_mean) / torch.clamp(td_std, min=1e-4))
        d["depth"] = dl.detach()
        total = total + cfg.depth_weight * dl
    if residuals is not None:  # TGD:932-939
        reg = sum(residuals[k].abs().mean() for k in RESIDUAL_KEYS if k in residuals)
        d["residual"] = reg.detach()
        total = total + cfg.residual_weight * reg
    if use_boundary:  # TGD:943-953
        if px is not None:
            bl = px["boundary"]
        else:
            from .losses import fresnel_boundary_mask
            mask = fresnel_boundary_mask(target_depth, cfg.num_fresnel_zones, (0.0, 1.0))
            bl = (torch.abs(rendered - target).mean(dim=1) * mask).mean()
        d["boundary"] = bl.detach()
        total = total + cfg.boundary_weight * bl
    if cfg.wave_equation_weight > 0:  # TGD:957-964
        from .losses import wave_equation_loss
        we = wave_equation_loss(rendered, cfg.wavelength, pixel_spacing=1.0 / cfg.image_size)
        d["wave_eq"] = we.detach()
        total = total + cfg.wave_equation_weight * we
    if cfg.use_phase_retrieval_loss and target_depth is not None:  # TGD:972-983
        pr = _loss_module("phase", cfg)(rendered, target, target_depth)
        d["phase_retrieval"] = pr.detach()
        total = total + cfg.phase_retrieval_weight * pr
    if cfg.use_frequency_loss:  # TGD:990-996
        fq = _loss_module("freq", cfg)(rendered, target)
        d["frequency"] = fq.detach()
        total = total + cfg.frequency_loss_weight * fq
    d["total"] = total.detach()
    return total, d


_LOSS_MODULES: Dict[str, torch.nn.Module] = {}


def _loss_module(kind: str, cfg: TrainingConfig):
    """One PhaseRetrievalLoss / FrequencyDomainLoss per process (TGD:1683-1690 builds them once)."""
    if kind not in _LOSS_MODULES:
        from .losses import FrequencyDomainLoss, PhaseRetrievalLoss
        _LOSS_MODULES[kind] = PhaseRetrievalLoss(wavelength=cfg.wavelength) if kind == "phase" else FrequencyDomainLoss()
    return _LOSS_MODULES[kind]


def default_renderer_factory(cfg: TrainingConfig, device, res: Optional[int] = None):
    """The product renderer: HIP TileBasedRenderer + the reference camera (TGD:1898-1917), at the effective training
    resolution (HFTS --train_resolution / --fast_mode, TGD:1643, 1880-1887)."""
    from .renderer import Camera, TileBasedRenderer
    res = res or cfg.image_size
    if cfg.experiment == 4 and cfg.use_phase_blending:  # TGD:1877-1890
        from .renderer import FourierGaussianRenderer
        renderer = FourierGaussianRenderer(res, res, wavelength_r=0.65, wavelength_g=0.55, wavelength_b=0.45,
                                           learnable_wavelengths=True).to(device)
    elif cfg.use_wave_rendering:  # TGD:1891-1897
        from .renderer import WaveFieldRenderer
        renderer = WaveFieldRenderer(res, res).to(device)
    else:                       # TGD:1898-1906
        renderer = TileBasedRenderer(res, res, use_phase_blending=cfg.use_phase_blending,
                                     phase_amplitude=cfg.phase_amplitude, workspace=cfg.workspace).to(device)
        if cfg.use_fresnel_zones:
            # the decoder snaps depths to `num_fresnel_zones` values (GDM:834-841): the zone-key depth sort then needs one
            # radix pass instead of four (FgsDims.sort_mode, fgs_sort.hip); a work-split choice, the order is the same
            renderer.tuning = dict(renderer.tuning or {})
            renderer.tuning.setdefault("sort_mode", 1)  # (merged: an existing tuning, or an explicit sort_mode=0, is kept -- ADVICE r4)
    camera = Camera(fx=res * 0.8, fy=res * 0.8, cx=res / 2, cy=res / 2, width=res, height=res)
    return renderer, camera


class StepResult:
    """What one train_step leaves behind, all on the device: `terms` (name -> 0-d tensor, this rank's shard; "total"
    is the mean over the ranks) and `skipped` (0-d float: 1.0 when the global batch was skipped for a NaN/Inf loss).
    `to_host()` is the only place that synchronises."""

    def __init__(self, terms, skipped):
        self.terms, self.skipped = terms, skipped

    def to_host(self):
        keys = sorted(self.terms)
        vals = torch.stack([self.terms[k].float() for k in keys] + [self.skipped.float()]).tolist()  # one transfer
        if vals[-1] > 0:
            return None
        return dict(zip(keys, vals[:-1]))


def make_optimizer(model, cfg: TrainingConfig):
    """AdamW(lr, weight_decay) as TGD:1970, FUSED: one multi-tensor kernel per step, and it takes the skip flag as a
    device tensor (`found_inf`, the mechanism GradScaler uses), so the NaN/Inf batch skip needs no host decision.
    With cfg.hip_graph the learning rate is a device tensor too (capturable): the cosine schedule then reaches a
    replayed graph by an in-place fill instead of a host scalar baked into the capture."""
    params = list(model.parameters())
    try:
        if cfg.hip_graph and params and params[0].is_cuda:
            return AdamW(params, lr=torch.tensor(cfg.lr, device=params[0].device), weight_decay=cfg.weight_decay,
                         fused=True, capturable=True)
        return AdamW(params, lr=cfg.lr, weight_decay=cfg.weight_decay, fused=True)
    except (RuntimeError, TypeError):  # a device without the fused kernel: plain AdamW, the skip costs one sync
        return AdamW(params, lr=cfg.lr, weight_decay=cfg.weight_decay)


class GraphedTrainStep:
    """train_step captured ONCE in a HIP graph (torch.cuda.CUDAGraph) and replayed per batch: the step's ~200 kernel
    launches (decoder MLP, the rasterizer's ~20 kernels each way, losses, clip, fused AdamW, the all-reduce) cost one
    graph launch on the host.  Possible because nothing in the step allocates behind torch's back, synchronises or takes
    a host decision (the NaN/Inf skip is `found_inf` on the device).  Inputs are copied into static buffers; the
    StepResult's tensors are static too (overwritten by the next replay -- read them before it).
    Eager fallback (`matches` is False): a batch of another shape (the epoch's tail batch)."""

    def __init__(self, model, renderer, camera, optimizer, cfg, dp, example_batch, epoch=0, train_res=None):
        self.static = tuple(torch.empty_like(t) for t in example_batch)
        for s_, t in zip(self.static, example_batch):
            s_.copy_(t)
        args = (model, renderer, camera, self.static, optimizer, cfg, dp)
        kw = dict(hfts=None, epoch=epoch, train_res=train_res, pose_rng=None, sample_gen=None)
        # warm-up on a side stream (plan caches, optimizer state, allocator), then put parameters and optimizer state
        # back: the capture must not cost the run three optimizer steps
        params = [p.detach().clone() for p in model.parameters()]
        had_state = len(optimizer.state) > 0
        saved_state = None
        if had_state:
            saved_state = {id(p): {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
                           for p, st in optimizer.state.items()}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                train_step(*args, **kw)
        torch.cuda.current_stream().wait_stream(side)
        with torch.no_grad():
            for p, q in zip(model.parameters(), params):
                p.copy_(q)
            for p, st in optimizer.state.items():
                for k, v in st.items():
                    if torch.is_tensor(v):
                        v.copy_(saved_state[id(p)][k]) if had_state else v.zero_()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.result = train_step(*args, **kw)

    def matches(self, batch) -> bool:
        return all(s_.shape == t.shape and s_.dtype == t.dtype for s_, t in zip(self.static, batch))

    def __call__(self, batch):
        for s_, t in zip(self.static, batch):
            s_.copy_(t, non_blocking=True)
        self.graph.replay()
        return self.result


def train_step(model, renderer, camera, batch, optimizer, cfg: TrainingConfig, dp: DPContext,
               hfts: Optional[HFTSConfig] = None, epoch: int = 0, train_res: Optional[int] = None,
               pose_rng: Optional[np.random.RandomState] = None, sample_gen: Optional[torch.Generator] = None):
    """One optimizer step on this rank's image shard, without a host synchronisation.  Returns a StepResult."""
    saag = None
    if cfg.decoder == "saag":  # the batch's SAAG clouds ride behind the step's tensors when every image has one (collate_host_items)
        n_step = 4 if cfg.use_vlm_guidance else 3
        batch, saag = batch[:n_step], (tuple(batch[n_step:]) if len(batch) == n_step + len(SAAG_NAMES) else None)
    if cfg.use_vlm_guidance:
        images, feats, depth, density = batch
    else:
        (images, feats, depth), density = batch, None
    res = train_res or cfg.image_size
    # progressive Gaussian growing (TGD:1069-1076) and the batch's pose (TGD:1078-1098)
    num_gaussians = hfts.get_gaussians_per_patch(epoch, cfg.epochs, cfg.gaussians_per_patch) if hfts is not None else None
    el, az, _ = sample_training_pose(cfg.multi_pose_augmentation, cfg.use_pose_encoding, cfg.frontal_prob,
                                     cfg.pose_range_elevation, cfg.pose_range_azimuth, pose_rng)
    el_t = torch.full((feats.shape[0],), el, device=feats.device) if el is not None else None
    az_t = torch.full((feats.shape[0],), az, device=feats.device) if az is not None else None
    mirror = cfg.decoder != "standin"  # the reference's decoders take channel-first features (TGD:1100) and emit (B,N,3) radians
    residuals = None
    if cfg.decoder == "saag":  # TGD:1043-1067: frontal camera, no progressive K, no pose arguments
        el = az = None
        if saag is None:
            saag = create_dummy_saag(feats.shape[0], DUMMY_SAAG_POINTS, feats.device, generator=sample_gen)
        out = model(feats.permute(0, 3, 1, 2), *saag)  # (a view: the hip backend samples the patch-major tensor in place)
        residuals = {k: out.pop(k) for k in RESIDUAL_KEYS}  # taken before any subsampling (TGD:1067 against :1154)
    elif cfg.decoder == "guided_saag":  # frontal camera, no progressive K, no pose arguments, as experiment 1
        el = az = None
        out = guided_saag_clouds(model, feats, depth, images, cfg)
    elif cfg.decoder == "physics":  # the class's forward takes no pose arguments (the reference's call at TGD:1100 raises TypeError)
        out = model(feats.permute(0, 3, 1, 2), depth, num_gaussians=num_gaussians)
    else:
        out = model(feats.permute(0, 3, 1, 2) if mirror else feats, depth, num_gaussians=num_gaussians, elevation=el_t, azimuth=az_t)
    out.pop("edge_strength", None)
    if not (cfg.use_phase_blending or cfg.use_wave_rendering):
        out.pop("phases", None)
    # stochastic Gaussian rendering: K Gaussians by opacity importance, gathered on the device (TGD:1154-1187)
    if hfts is not None and cfg.decoder != "guided_saag":  # (refused with K < N for guided_saag: run_training)
        out, _ = importance_subsample(out, hfts.get_stochastic_k(out["positions"].shape[1]), generator=sample_gen)
    phases = out.get("phases")
    if cfg.use_wave_rendering and phases is not None and not mirror:
        phases = phases * (2.0 * math.pi)  # wave renderers take radians (DR:772), the stand-in decoder emits [0,1]
    # (the physics decoder's (B,N) radians go on as they are;
    # a mirror's (B,N,3) phases go on as they are: radians for the wave renderer, ignored by the Fourier renderer; on the
    # TileBasedRenderer phase path the renderer's RuntimeError for (N,3) phases surfaces, as in the reference -- SURVEY section 0.4)
    render_camera = camera_for_batch(camera, el, az, res, cfg.multi_pose_augmentation)  # TGD:1196-1207
    # ONE batched call replaces the per-image loop of TGD:1209-1223
    rendered, rdepth = renderer(out["positions"], out["scales"], out["rotations"], out["colors"],
                                out["opacities"], render_camera, return_depth=True, phases=phases)
    target = F.interpolate(images, size=(res, res), mode="bilinear", align_corners=False)
    tdepth = F.interpolate(depth, size=(res, res), mode="bilinear", align_corners=False).squeeze(1)
    loss, terms = compute_losses(rendered, target, rdepth, tdepth, cfg, dp, vlm_density=density, residuals=residuals)
    # NaN/Inf batch skip (TGD:1255-1258), decided on the device and by ALL ranks together: the flag and the loss ride
    # behind the gradients in the one all-reduce of the step
    bad = (~torch.isfinite(loss.detach())).float()
    if dp.enabled:
        dp.adopt(list(model.parameters()))  # .grad = slices of the flat bucket, zeroed in one launch: nothing to pack later
    else:
        optimizer.zero_grad(set_to_none=True)
    loss.backward()
    extra = torch.stack([bad, torch.nan_to_num(loss.detach().float(), nan=0.0, posinf=0.0, neginf=0.0)])
    extra = dp.allreduce_gradients(list(model.parameters()), extra=extra)
    skipped = (extra[0] > 0).float()
    terms["total"] = extra[1] / dp.world
    torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)  # TGD:1264 (foreach, no host sync)
    if getattr(optimizer, "_step_supports_amp_scaling", False) and optimizer.defaults.get("fused"):
        optimizer.grad_scale, optimizer.found_inf = None, skipped.reshape(())  # skipped batch: the fused step is a no-op
        optimizer.step()
    elif not bool(skipped):  # non-fused optimizer: the skip is a host decision (one sync)
        optimizer.step()
    return StepResult(terms, skipped)


DECODERS = ("standin", "direct", "fibonacci", "nca", "saag", "physics", "guided_saag")


def make_decoder(cfg: TrainingConfig):
    """The step's decoder: the stand-in (default), or a mirror of the reference's class constructed as its training script
    constructs it (TGD:1814-1828 experiment 2, TGD:1832-1840 experiment 4, TGD:1842-1849 experiment 5, TGD:1786 experiment 1)."""
    phase_out = cfg.use_phase_blending or cfg.use_wave_rendering
    if cfg.decoder == "standin":
        return PatchGaussianDecoder(cfg.feature_dim, cfg.gaussians_per_patch, grid=cfg.feature_size,
                                    use_fresnel_zones=cfg.use_fresnel_zones,
                                    num_fresnel_zones=cfg.num_fresnel_zones,
                                    use_phase_output=phase_out,
                                    use_edge_aware=cfg.use_edge_aware, edge_scale_factor=cfg.edge_scale_factor,
                                    edge_opacity_boost=cfg.edge_opacity_boost)
    if cfg.decoder == "guided_saag":  # the class's defaults (GDM:1440-1445)
        return FeatureGuidedSAAG(feature_dim=cfg.feature_dim)
    if cfg.decoder == "saag":
        if cfg.saag_backend not in SAAG_BACKENDS:
            raise ValueError(f"unknown saag_backend {cfg.saag_backend!r}: one of {SAAG_BACKENDS}")
        return SAAGRefinementNet(feature_dim=cfg.feature_dim, backend=cfg.saag_backend)  # (the class's defaults, as TGD:1786)
    if cfg.head_backend not in HEAD_BACKENDS:
        raise ValueError(f"unknown head_backend {cfg.head_backend!r}: one of {HEAD_BACKENDS}")
    if cfg.decoder == "physics":  # TGD:1803-1810
        if cfg.use_pose_encoding:
            raise ValueError("--decoder physics cannot be combined with --use_pose_encoding: PhysicsDirectPatchDecoder has no pose "
                             "inputs (GDM:1032-1038)")
        return PhysicsDirectPatchDecoder(feature_dim=cfg.feature_dim, gaussians_per_patch=cfg.gaussians_per_patch,
                                         wavelength=cfg.wavelength, learnable_wavelength=cfg.learnable_wavelength,
                                         focal_depth=cfg.focal_depth, use_diffraction_placement=cfg.use_diffraction_placement,
                                         head_backend=cfg.head_backend)
    if cfg.decoder == "direct":
        return DirectPatchDecoder(feature_dim=cfg.feature_dim, gaussians_per_patch=cfg.gaussians_per_patch,
                                  use_fresnel_zones=cfg.use_fresnel_zones, num_fresnel_zones=cfg.num_fresnel_zones,
                                  use_edge_aware=cfg.use_edge_aware, use_phase_output=phase_out,
                                  edge_scale_factor=cfg.edge_scale_factor, edge_opacity_boost=cfg.edge_opacity_boost,
                                  use_pose_encoding=cfg.use_pose_encoding, head_backend=cfg.head_backend)
    if cfg.decoder == "fibonacci":
        return FibonacciPatchDecoder(feature_dim=cfg.feature_dim, n_spiral_points=cfg.n_spiral_points, gaussians_per_point=1,
                                     use_fresnel_zones=cfg.use_fresnel_zones, num_fresnel_zones=cfg.num_fresnel_zones,
                                     use_phase_output=phase_out, use_pose_encoding=cfg.use_pose_encoding,
                                     head_backend=cfg.head_backend)
    if cfg.decoder == "nca":  # TGD:1842-1849
        model = NCAGaussianDecoder(feature_dim=cfg.feature_dim, n_points=cfg.n_spiral_points, n_steps=cfg.nca_steps,
                                   k_neighbors=cfg.nca_neighbors, nca_backend=cfg.nca_backend, head_backend=cfg.head_backend)
        with torch.no_grad():
            model.step_size.fill_(cfg.nca_step_size)
        return model
    raise ValueError(f"unknown decoder {cfg.decoder!r}: one of {DECODERS}")


def load_checkpoint(model, optimizer, ck, cfg: TrainingConfig) -> int:
    """Restore model and optimizer from a checkpoint dict {epoch, model_state_dict, optimizer_state_dict} (TGD:1304-1310);
    -> the epoch to start at.  A mirror decoder also takes the REFERENCE's checkpoints: the state dict loads strictly (same
    keys), and of the optimizer only the per-parameter state and the learning rate are taken -- the parameters are registered
    in the reference's order, so its AdamW moments land on the right tensors -- while this harness's own group options (the
    fused step that takes the NaN/Inf skip flag) stay."""
    model.load_state_dict(ck["model_state_dict"])
    osd = ck["optimizer_state_dict"]
    if cfg.decoder != "standin":
        ours = optimizer.state_dict()
        for g_ours, g_ck in zip(ours["param_groups"], osd["param_groups"]):
            for k in ("lr", "initial_lr"):
                if k in g_ck:
                    g_ours[k] = g_ck[k]
        osd = {"state": osd["state"], "param_groups": ours["param_groups"]}
    optimizer.load_state_dict(osd)
    return ck["epoch"] + 1


def save_checkpoint(model, optimizer, epoch, losses, cfg: TrainingConfig):
    os.makedirs(cfg.output_dir, exist_ok=True)
    ckpt = {"epoch": epoch, "model_state_dict": model.state_dict(),
            "optimizer_state_dict": optimizer.state_dict(), "losses": losses, "config": asdict(cfg)}
    path = Path(cfg.output_dir) / f"decoder_exp{cfg.experiment}_epoch{epoch}.pt"
    torch.save(ckpt, path)
    return path


def make_dataset(cfg: TrainingConfig, log=print):
    """ImageDataset over --data_dir (with its `features/` caches) when it holds images; otherwise the synthetic
    stand-in (the reference fabricates test images itself when the directory is empty, TGD:1748-1758)."""
    if cfg.data_dir and os.path.isdir(cfg.data_dir):
        from .data import ImageDataset
        ds = ImageDataset(cfg.data_dir, cfg.image_size, max_images=cfg.max_images, feature_dim=cfg.feature_dim,
                          load_vlm_density=cfg.use_vlm_guidance, load_saag=cfg.decoder == "saag")
        if len(ds) > 0:
            if ds[0]["features"].shape[-1] != cfg.feature_size:
                raise ValueError(f"feature caches are 37x37 patch grids; got feature_size={cfg.feature_size}")
            log(f"Found {len(ds)} images in {cfg.data_dir}")
            return ds, len(ds)
        log(f"No images in {cfg.data_dir}: synthetic data")
    n_items = cfg.max_images or cfg.batch_size * cfg.steps_per_epoch
    return SyntheticDataset(n_items, cfg), n_items


def check_workspace_options(workspace: str, hip_graph: bool):
    """--workspace adaptive learns the duplicate capacity from step to step; a captured graph would freeze the capacity of the
    step it was captured at (and replay no readback), so the two are refused together."""
    if workspace not in ("worst", "adaptive"):
        raise ValueError(f"unknown workspace {workspace!r}: one of ('worst', 'adaptive')")
    if workspace == "adaptive" and hip_graph:
        raise ValueError("--workspace adaptive cannot be combined with --hip_graph: a captured graph freezes the duplicate "
                         "capacity; use --workspace worst with --hip_graph")


def _workspace_metrics(renderer):
    """(MB of `saved` + `scratch` of the last rasterizer call of every shape, overflows seen): host values, no synchronisation."""
    stats = renderer.workspace_stats() if hasattr(renderer, "workspace_stats") else {}
    return sum(v["bytes"] for v in stats.values()) / 2.0 ** 20, sum(v["overflows"] for v in stats.values())


def _make_renderer(renderer_factory, cfg, device, train_res):
    """Factories take (cfg, device) or (cfg, device, res): chosen from the signature (a TypeError raised INSIDE a
    three-argument factory must not be mistaken for a two-argument one)."""
    try:
        params = inspect.signature(renderer_factory).parameters.values()
        takes_res = len(params) >= 3 or any(p.kind == p.VAR_POSITIONAL for p in params)
    except (TypeError, ValueError):
        takes_res = True
    return renderer_factory(cfg, device, train_res) if takes_res else renderer_factory(cfg, device)


def save_training_history(history: Dict[str, list], cfg: TrainingConfig):
    """training_history_exp{E}.json (TGD:1317-1323): one list per loss term, one entry per epoch, plus this repo's
    step ms, composited Gaussian-pixels/s (whole job) and the rasterizer's stage ms."""
    os.makedirs(cfg.output_dir, exist_ok=True)
    path = Path(cfg.output_dir) / f"training_history_exp{cfg.experiment}.json"
    with open(path, "w") as f:
        json.dump(history, f, indent=2)
    return path


def run_training(cfg: TrainingConfig, dp: Optional[DPContext] = None,
                 renderer_factory: Callable = default_renderer_factory, resume: Optional[str] = None,
                 log=print, hfts: Optional[HFTSConfig] = None):
    device = torch.device(cfg.device)
    if cfg.ssim_backend not in SSIM_BACKENDS:
        raise ValueError(f"unknown ssim_backend {cfg.ssim_backend!r}: one of {SSIM_BACKENDS}")
    if cfg.ssim_backend == "hip" and device.type != "cuda":
        raise ValueError("ssim_backend 'hip' needs a GPU device: the HIP SSIM kernels have no CPU fallback")
    if cfg.pixel_loss_backend not in PIXEL_LOSS_BACKENDS:
        raise ValueError(f"unknown pixel_loss_backend {cfg.pixel_loss_backend!r}: one of {PIXEL_LOSS_BACKENDS}")
    if cfg.pixel_loss_backend == "hip" and device.type != "cuda":
        raise ValueError("pixel_loss_backend 'hip' needs a GPU device: the HIP pixel-loss kernels have no CPU fallback")
    check_workspace_options(cfg.workspace, cfg.hip_graph)
    dp = dp or DPContext(device=device if device.type == "cuda" else None)
    if cfg.batch_size % dp.world != 0:  # fail fast, before any rank can stall in a collective (see DPContext.shard)
        raise ValueError(f"--batch_size {cfg.batch_size} is not a multiple of the {dp.world} ranks")
    torch.manual_seed(cfg.seed)
    if cfg.decoder != "standin" and cfg.head_backend == "hip" and device.type != "cuda":
        raise ValueError("head_backend 'hip' needs a GPU device: the HIP head kernels have no CPU fallback")
    if cfg.decoder == "nca" and cfg.nca_backend == "hip" and device.type != "cuda":
        raise ValueError("nca_backend 'hip' needs a GPU device: the HIP perception / update kernels have no CPU fallback")
    if cfg.decoder == "saag" and cfg.saag_backend == "hip" and device.type != "cuda":
        raise ValueError("saag_backend 'hip' needs a GPU device: the HIP input / refinement kernels have no CPU fallback")
    if cfg.decoder == "saag" and cfg.hip_graph:
        raise ValueError("--experiment 1 cannot be combined with --hip_graph: the size of the SAAG cloud follows the files, so "
                         "the step's shapes change from batch to batch")
    if cfg.decoder == "guided_saag":
        if device.type != "cuda":
            raise ValueError("--decoder guided_saag needs a GPU device: the SAAG generator's HIP kernels have no CPU fallback")
        if cfg.hip_graph:
            raise ValueError("--decoder guided_saag cannot be combined with --hip_graph: a host read of the row offsets sizes the "
                             "cloud of every batch")
        if hfts is not None and (hfts.stochastic_k is not None or hfts.fast_mode):
            raise ValueError("--decoder guided_saag cannot be combined with --stochastic_k / --fast_mode: the sampled indices are "
                             "shared by the batch, and the batch's clouds differ in size")
    model = make_decoder(cfg).to(device)
    dp.broadcast_parameters(model)
    train_res = hfts.get_effective_train_resolution(cfg.image_size) if hfts is not None else cfg.image_size
    renderer, camera = _make_renderer(renderer_factory, cfg, device, train_res)
    # host-side draws that every rank must make identically (the pose is shared by the global batch; the K sampled
    # indices differ per rank like any other per-shard quantity)
    pose_rng = np.random.RandomState(cfg.seed + 7919)
    sample_gen = torch.Generator(device=device).manual_seed(cfg.seed * 104729 + dp.rank) if device.type == "cuda" else None
    optimizer = make_optimizer(model, cfg)
    scheduler = CosineAnnealingLR(optimizer, T_max=cfg.epochs)
    start_epoch = 0
    if resume:
        start_epoch = load_checkpoint(model, optimizer, torch.load(resume, map_location=device), cfg)
    data, n_items = make_dataset(cfg, log if dp.rank == 0 else (lambda *a: None))
    # metrics beyond the losses: composited Gaussian-pixels counted on the device by the renderer,
    # the rasterizer's stage timers sampled on the logged steps
    pair_counter = None
    stage_timers = None
    if device.type == "cuda" and hasattr(renderer, "pair_counter"):
        pair_counter = torch.zeros(3, dtype=torch.int64, device=device)  # [pairs, tile duplicates, Gaussians]
        renderer.pair_counter = pair_counter
        from . import _binding as stage_timers
    history: Dict[str, list] = {}
    epoch_history = []
    # one captured graph for the whole run: needs a step whose host side is the same every time (no per-batch pose, no
    # per-epoch Gaussian count / K-subset schedule)
    use_graph = bool(cfg.hip_graph) and device.type == "cuda" and hfts is None and not cfg.multi_pose_augmentation
    if cfg.hip_graph and not use_graph and dp.rank == 0:
        log("  --hip_graph ignored: the step changes from batch to batch (HFTS schedule / per-batch pose) or runs on the CPU")
    graphed = None
    for epoch in range(start_epoch, cfg.epochs):
        model.train()
        batches = epoch_batches(n_items, cfg.batch_size, dp.world, cfg.seed, epoch)
        shards = []
        for gb in batches:
            lo, hi = dp.shard(len(gb))  # image-wise shard of the global batch
            shards.append(gb[lo:hi])
        acc: Dict[str, torch.Tensor] = {}
        n_ok = torch.zeros((), device=device)
        if pair_counter is not None:
            pair_counter.zero_()
            stage_timers.stage_timing_read()
        t0 = time.perf_counter()
        for bi, batch in enumerate(BatchPrefetcher(data, shards, device, cfg.num_workers)):
            logged = bi % cfg.log_interval == 0
            if use_graph and graphed is None and len(shards[bi]) * dp.world == cfg.batch_size:
                graphed = GraphedTrainStep(model, renderer, camera, optimizer, cfg, dp, batch, epoch=epoch, train_res=train_res)
            if graphed is not None and graphed.matches(batch):
                res = graphed(batch)  # (stage timers are event pairs recorded at launch time: not inside a replayed graph)
            else:
                if stage_timers is not None and logged:
                    stage_timers.stage_timing_enable(True)
                res = train_step(model, renderer, camera, batch, optimizer, cfg, dp, hfts=hfts, epoch=epoch,
                                 train_res=train_res, pose_rng=pose_rng, sample_gen=sample_gen)
                if stage_timers is not None and logged:
                    stage_timers.stage_timing_enable(False)
            ok = 1.0 - res.skipped
            n_ok = n_ok + ok
            for k, v in res.terms.items():  # device-side sums over the batches that were not skipped
                acc[k] = acc.get(k, 0.0) + torch.where(ok > 0, v.float(), torch.zeros_like(v, dtype=torch.float32))
            if logged:  # the only host round trip inside the epoch: once per log_interval (TGD:1275-1281)
                ld = res.to_host()
                if dp.rank == 0:
                    if ld is None:
                        log(f"  Warning: NaN/Inf loss at batch {bi}, skipping")
                    else:
                        log(f"  Batch {bi}/{len(shards)} | Loss: {ld['total']:.4f} | RGB: {ld['rgb']:.4f}")
        scheduler.step()
        keys = sorted(acc)
        extra = [pair_counter[i].double() for i in range(3)] if pair_counter is not None else []
        vals = torch.stack([acc[k].double() for k in keys] + [n_ok.double()] + extra)
        if dp.enabled and pair_counter is not None:
            import torch.distributed as tdist  # whole-job pair / duplicate counts (the losses are this rank's shard, as before)
            tdist.all_reduce(vals[-3:], op=tdist.ReduceOp.SUM)
        vals = vals.tolist()  # epoch end: one transfer (also the sync that closes the epoch's clock)
        elapsed = time.perf_counter() - t0
        nb = vals[len(keys)]
        losses = {k: v / nb for k, v in zip(keys, vals)} if nb > 0 else {}
        epoch_history.append(losses)
        steps = max(len(shards), 1)
        metrics = {"step_ms": elapsed / steps * 1e3, "skipped_batches": len(shards) - int(nb)}
        metrics["workspace_mb"], metrics["capacity_overflows"] = _workspace_metrics(renderer)
        if pair_counter is not None:
            pairs, dups, gauss = vals[-3], vals[-2], vals[-1]
            metrics["pairs_per_s"] = pairs / max(elapsed, 1e-9)
            # ALGORITHMIC HBM bytes of the rasterizer per second, whole job, forward + backward: the per-stage figures of
            # DESIGN.md section 4 / bench.py -- 304 B per Gaussian (projection 112, depth sort 72, lists 8, projection
            # adjoint 112), 188 B per tile duplicate (lists 4, record gather 52 + 52, gradient row 40 + 40) and 72 B per
            # pixel (state, outputs, upstream gradients) -- over the epoch's wall time (which includes the decoder)
            n_img = sum(len(sh) for sh in shards) * dp.world
            metrics["hbm_gbs_algorithmic"] = (304.0 * gauss + 188.0 * dups + 72.0 * n_img * train_res * train_res) / max(elapsed, 1e-9) / 1e9
            st = stage_timers.stage_timing_read()
            metrics["stage_ms"] = {k: v[0] / v[1] for k, v in st.items() if v[1]}
        for k, v in list(losses.items()) + list(metrics.items()):
            if isinstance(v, dict):
                for kk, vv in v.items():
                    history.setdefault(k, {}).setdefault(kk, []).append(vv)
            else:
                history.setdefault(k, []).append(v)
        if dp.rank == 0:
            log(f"Epoch {epoch + 1}/{cfg.epochs} | Time: {elapsed:.1f}s | {metrics['step_ms']:.2f} ms/step | "
                + " ".join(f"{k}={v:.4f}" for k, v in losses.items()))
            if (epoch + 1) % cfg.save_interval == 0 or epoch + 1 == cfg.epochs:
                save_checkpoint(model, optimizer, epoch, losses, cfg)
    if dp.rank == 0 and history:
        save_training_history(history, cfg)
    return model, epoch_history


def arg_parser() -> argparse.ArgumentParser:
    """The command line of `main` (TGD:1401-1545 names and defaults)."""
    ap = argparse.ArgumentParser(description="Train the Gaussian decoder through the HIP rasterizer")
    c = TrainingConfig()
    ap.add_argument("--experiment", type=int, default=c.experiment)
    ap.add_argument("--data_dir", default=c.data_dir)
    ap.add_argument("--output_dir", default=c.output_dir)
    ap.add_argument("--batch_size", type=int, default=c.batch_size)
    ap.add_argument("--epochs", type=int, default=c.epochs)
    ap.add_argument("--lr", type=float, default=c.lr)
    ap.add_argument("--image_size", type=int, default=c.image_size)
    ap.add_argument("--gaussians_per_patch", type=int, default=c.gaussians_per_patch)
    ap.add_argument("--max_images", type=int, default=None)
    ap.add_argument("--use_fresnel_zones", type=int, nargs="?", const=8, default=0,
                    help="quantise depth into N zones (TGD flag; bare flag = 8)")
    ap.add_argument("--num_fresnel_zones", type=int, default=c.num_fresnel_zones)
    ap.add_argument("--boundary_weight", type=float, default=c.boundary_weight,
                    help="zone-boundary emphasis term under --use_fresnel_zones (TGD:146; the reference's default is 0.1)")
    ap.add_argument("--use_vlm_guidance", action="store_true", help="weight the L1 term by the VLM density maps (TGD:1443)")
    ap.add_argument("--vlm_weight", type=float, default=c.vlm_weight, help="TGD:1445")
    ap.add_argument("--use_phase_blending", action="store_true")
    ap.add_argument("--phase_amplitude", type=float, default=c.phase_amplitude)
    ap.add_argument("--use_edge_aware", action="store_true", help="smaller Gaussians at depth edges (TGD:1455)")
    ap.add_argument("--edge_scale_factor", type=float, default=c.edge_scale_factor, help="TGD:1461")
    ap.add_argument("--train_resolution", type=int, default=None, help="HFTS render resolution (TGD:1524)")
    ap.add_argument("--progressive_schedule", action="store_true", help="HFTS progressive Gaussian growing (TGD:1526)")
    ap.add_argument("--stochastic_k", type=int, default=None, help="HFTS: render K importance-sampled Gaussians (TGD:1528)")
    ap.add_argument("--fast_mode", action="store_true", help="HFTS preset: 64x64, progressive, K=256 (TGD:1530)")
    ap.add_argument("--multi_pose_augmentation", action="store_true", help="random orbit pose per batch (TGD:1536)")
    ap.add_argument("--pose_range_elevation", type=float, nargs=2, default=[-30, 45], help="degrees (TGD:1538)")
    ap.add_argument("--pose_range_azimuth", type=float, nargs=2, default=[0, 360], help="degrees (TGD:1540)")
    ap.add_argument("--frontal_prob", type=float, default=c.frontal_prob, help="TGD:1542")
    ap.add_argument("--use_pose_encoding", action="store_true", help="TGD:1544 (pose-dependent decoder output)")
    ap.add_argument("--use_wave_rendering", action="store_true", help="WaveFieldRenderer (TGD:1469)")
    ap.add_argument("--use_qsr", action="store_true", help="macro flag: implies --use_wave_rendering (TGD:1550-1553)")
    ap.add_argument("--wave_equation_weight", type=float, default=c.wave_equation_weight, help="TGD:1483")
    ap.add_argument("--wavelength", type=float, default=c.wavelength)
    ap.add_argument("--learnable_wavelength", dest="learnable_wavelength", action="store_true", default=c.learnable_wavelength,
                    help="--decoder physics: the wavelength is a parameter (TGD:1473)")
    ap.add_argument("--no_learnable_wavelength", dest="learnable_wavelength", action="store_false")
    ap.add_argument("--focal_depth", type=float, default=c.focal_depth, help="focal plane of the physics phase (TGD:1479)")
    ap.add_argument("--use_physics_zones", action="store_true", help="TGD:1475 (recorded; selects no decoder by itself here)")
    ap.add_argument("--use_diffraction_placement", action="store_true",
                    help="TGD:1477: --decoder physics carries the Fresnel-integral tables (never evaluated, as in the reference)")
    ap.add_argument("--use_phase_retrieval_loss", action="store_true", help="TGD:1494 (--use_qsr implies it, TGD:1553)")
    ap.add_argument("--phase_retrieval_weight", type=float, default=c.phase_retrieval_weight)
    ap.add_argument("--use_frequency_loss", action="store_true", help="TGD:1498")
    ap.add_argument("--frequency_loss_weight", type=float, default=c.frequency_loss_weight)
    ap.add_argument("--resume", default=None)
    ap.add_argument("--hip_graph", action="store_true", help="replay the whole training step from one captured HIP graph")
    ap.add_argument("--workspace", default=c.workspace, choices=["worst", "adaptive"],
                    help="rasterizer workspaces sized for the worst case (default) or by the duplicates the previous steps needed")
    ap.add_argument("--renderer", default="hip", choices=["hip"],
                    help="only the HIP rasterizer ships; there is no CPU fallback")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ssim_backend", default=c.ssim_backend, choices=list(SSIM_BACKENDS),
                    help="SSIM term: pytorch_msssim when importable (default, as the reference) or this package's HIP kernels")
    ap.add_argument("--pixel_loss_backend", default=c.pixel_loss_backend, choices=list(PIXEL_LOSS_BACKENDS),
                    help="L1 / boundary / depth terms: torch expressions (default) or this package's fused HIP kernels")
    ap.add_argument("--decoder", default=c.decoder, choices=list(DECODERS),
                    help="the stand-in decoder (default) or a mirror of the reference's DirectPatchDecoder / FibonacciPatchDecoder "
                         "(loads its checkpoints); --experiment 4 implies fibonacci; physics: PhysicsDirectPatchDecoder, the "
                         "reference's decoder for --use_wave_rendering without --use_qsr")
    ap.add_argument("--head_backend", default=c.head_backend, choices=list(HEAD_BACKENDS),
                    help="Gaussian-parameter head of --decoder direct / fibonacci: torch expressions (default) or the fused HIP kernels")
    ap.add_argument("--n_spiral_points", type=int, default=c.n_spiral_points, help="TGD:1427 (--decoder fibonacci / nca)")
    ap.add_argument("--nca_steps", type=int, default=c.nca_steps, help="NCA iterations (TGD:1435; --experiment 5)")
    ap.add_argument("--nca_neighbors", type=int, default=c.nca_neighbors, help="k nearest neighbours every point perceives (TGD:1437)")
    ap.add_argument("--nca_step_size", type=float, default=c.nca_step_size,
                    help="initial value of the learnable step size (the reference parses this flag, TGD:1439, and never uses it)")
    ap.add_argument("--saag_backend", default=c.saag_backend, choices=list(SAAG_BACKENDS),
                    help="input gather and residual head of --experiment 1: the reference's torch ops (default) or the fused HIP kernels")
    ap.add_argument("--surface_subsample", type=int, default=c.surface_subsample,
                    help="--decoder guided_saag: one SAAG point per K x K pixels of the depth map (default 4: 4 096 points and at most "
                         "49 152 Gaussians per 256 x 256 image; a setting, not a measured optimum)")
    ap.add_argument("--residual_weight", type=float, default=c.residual_weight,
                    help="weight of the residual regulariser of --experiment 1 (TGD:120)")
    ap.add_argument("--nca_backend", default=c.nca_backend, choices=list(NCA_BACKENDS),
                    help="neighbour perception and update of --experiment 5: the reference's torch ops (default) or the fused HIP kernels")
    return ap


def config_from_args(a) -> TrainingConfig:
    """The TrainingConfig of a parsed command line (no device yet).  --experiment 1 trains the SAAG refinement net
    (TGD:1043-1067), --experiment 2 a patch-grid decoder, --experiment 4 the Fibonacci decoder (TGD:1829-1841), with
    --use_phase_blending through the Fourier renderer (TGD:1877-1890), --experiment 5 the NCA decoder (TGD:1841-1849) through the
    TileBasedRenderer; --experiment 3 --decoder guided_saag the feature-guided SAAG generator (FeatureGuidedSAAG, GDM:1422-1490,
    through surface.guided_surface_gaussians).  Bare --experiment 3 stays refused: it names the reference's step (TGD:1135-1152),
    which renders a random dummy cloud and is not offered here."""
    if a.experiment == 3 and a.decoder != "guided_saag":
        raise SystemExit("--experiment 3 alone names the reference's dummy-cloud step, which this repo does not offer: pass "
                         "--experiment 3 --decoder guided_saag to train the feature-guided SAAG generator")
    if a.experiment not in (1, 2, 3, 4, 5):
        raise SystemExit("only --experiment 1 (SAAG refinement), --experiment 2 (patch-grid decoder), --experiment 3 --decoder "
                         "guided_saag (feature-guided SAAG), --experiment 4 (Fibonacci decoder) and --experiment 5 (NCA decoder) "
                         "are on this repo's hot path")
    decoder = a.decoder
    if a.experiment == 3:
        if a.hip_graph:
            raise SystemExit("--decoder guided_saag cannot be combined with --hip_graph: a host read of the row offsets sizes the "
                             "cloud of every batch")
        if a.stochastic_k is not None or a.fast_mode:
            raise SystemExit("--decoder guided_saag cannot be combined with --stochastic_k / --fast_mode: the sampled indices are "
                             "shared by the batch, and the batch's clouds differ in size")
        if a.surface_subsample < 1:
            raise SystemExit("--surface_subsample must be at least 1")
    elif decoder == "guided_saag":
        raise SystemExit("--decoder guided_saag is --experiment 3")
    elif a.experiment == 1:
        if decoder in ("direct", "fibonacci", "nca"):
            raise SystemExit(f"--experiment 1 trains the SAAG refinement net: --decoder {decoder} contradicts it")
        if a.hip_graph:
            raise SystemExit("--experiment 1 cannot be combined with --hip_graph: the size of the SAAG cloud follows the files, "
                             "so the step's shapes change from batch to batch")
        decoder = "saag"
    elif decoder == "saag":
        raise SystemExit("--decoder saag is --experiment 1")
    elif decoder == "physics" and a.experiment != 2:
        raise SystemExit("--decoder physics is an --experiment 2 decoder (TGD:1779-1782)")
    elif a.experiment == 4:
        if decoder in ("direct", "nca"):
            raise SystemExit(f"--experiment 4 trains the Fibonacci decoder: --decoder {decoder} contradicts it")
        decoder = "fibonacci"
    elif a.experiment == 5:
        if decoder in ("direct", "fibonacci"):
            raise SystemExit(f"--experiment 5 trains the NCA decoder: --decoder {decoder} contradicts it")
        decoder = "nca"
    elif decoder == "fibonacci":
        raise SystemExit("--decoder fibonacci is --experiment 4")
    elif decoder == "nca":
        raise SystemExit("--decoder nca is --experiment 5")
    return TrainingConfig(experiment=a.experiment, data_dir=a.data_dir, output_dir=a.output_dir,
                          batch_size=a.batch_size, epochs=a.epochs, lr=a.lr, image_size=a.image_size,
                          gaussians_per_patch=a.gaussians_per_patch, max_images=a.max_images,
                          use_fresnel_zones=bool(a.use_fresnel_zones),
                          num_fresnel_zones=a.use_fresnel_zones or a.num_fresnel_zones,
                          use_phase_blending=a.use_phase_blending, phase_amplitude=a.phase_amplitude,
                          use_edge_aware=a.use_edge_aware, edge_scale_factor=a.edge_scale_factor,
                          multi_pose_augmentation=a.multi_pose_augmentation,
                          pose_range_elevation=tuple(a.pose_range_elevation), pose_range_azimuth=tuple(a.pose_range_azimuth),
                          frontal_prob=a.frontal_prob, use_pose_encoding=a.use_pose_encoding,
                          use_wave_rendering=a.use_wave_rendering or a.use_qsr,
                          wave_equation_weight=a.wave_equation_weight, wavelength=a.wavelength,
                          use_phase_retrieval_loss=a.use_phase_retrieval_loss or a.use_qsr,
                          phase_retrieval_weight=a.phase_retrieval_weight,
                          use_frequency_loss=a.use_frequency_loss, frequency_loss_weight=a.frequency_loss_weight,
                          seed=a.seed, hip_graph=a.hip_graph,
                          ssim_backend=a.ssim_backend, boundary_weight=a.boundary_weight,
                          use_vlm_guidance=a.use_vlm_guidance, vlm_weight=a.vlm_weight,
                          pixel_loss_backend=a.pixel_loss_backend, workspace=a.workspace,
                          decoder=decoder, head_backend=a.head_backend, n_spiral_points=a.n_spiral_points,
                          nca_steps=a.nca_steps, nca_neighbors=a.nca_neighbors, nca_backend=a.nca_backend,
                          nca_step_size=a.nca_step_size, saag_backend=a.saag_backend, residual_weight=a.residual_weight,
                          surface_subsample=a.surface_subsample,
                          learnable_wavelength=a.learnable_wavelength, focal_depth=a.focal_depth,
                          use_physics_zones=a.use_physics_zones, use_diffraction_placement=a.use_diffraction_placement)


def main(argv=None):
    a = arg_parser().parse_args(argv)
    try:
        check_workspace_options(a.workspace, a.hip_graph)
    except ValueError as e:
        raise SystemExit(str(e))
    cfg = config_from_args(a)
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("fresnel_amd.train needs a GPU: the HIP rasterizer has no CPU fallback")
    torch.cuda.set_device(local_rank)
    cfg.device = f"cuda:{local_rank}"
    hfts = HFTSConfig(train_resolution=a.train_resolution, progressive_schedule=a.progressive_schedule,
                      stochastic_k=a.stochastic_k, fast_mode=a.fast_mode)
    dp = DPContext(device=torch.device(cfg.device))
    try:
        return run_training(cfg, dp, resume=a.resume, hfts=hfts if hfts.enabled else None)  # (model, per-epoch losses)
    finally:
        dp.shutdown()


if __name__ == "__main__":
    main()
