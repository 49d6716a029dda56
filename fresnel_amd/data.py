"""Dataset side of the training harness: this repo's counterpart of the reference's ImageDataset
(scripts/training/train_gaussian_decoder.py:525-675) for the tensors the rasterizer path consumes.

    ImageDataset(data_dir, image_size, feature_cache_dir=None, max_images=None, feature_dim=384, load_vlm_density=False)[i] ->
        {'image' (3,S,S) in [0,1], 'features' (feature_dim,37,37), 'depth' (1,S,S), 'has_saag', 'saag_*', 'name'}
        and, with load_vlm_density, 'vlm_density' (1,S,S) + 'has_vlm_density'

Same file discovery (jpg / jpeg / png / webp, both cases, sorted, max_images prefix), the same cache file names and
layouts (fresnel_amd/io.py), the same fall-backs (zero features / zero depth / empty SAAG when a cache is missing).
The VLM density maps (`features/{name}_vlm_density.npy`, a square grid; TGD:649-663) are read with load_vlm_density: resized to
the image with corner-aligned bilinear interpolation -- what the reference's scipy.ndimage.zoom(order=1) computes -- plus 0.5,
and all ones when the file is missing or unreadable.  Colour-jitter augmentation is not part of the rasterizer path and is left out.
"""
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np
import torch

from . import io as fio


def collate_host_items(items, saag_tensors: int = 0):
    """Stack the per-item tuples of `host_item` into one batch tuple.  The last `saag_tensors` (5, or 0) entries of every item are
    its SAAG cloud, empty (0 Gaussians) where the image has no `_saag.bin`: they join the batch only when EVERY item has a cloud
    and all clouds have the same count; otherwise they are left out and the step draws the dummy cloud (train_step).  (The
    reference stacks whatever the items hold in its default collate, TGD:1760-1767, and would crash there on unequal counts;
    it falls back to the dummy cloud only when the stacked clouds are empty, TGD:1046-1056.)"""
    cols = list(zip(*items))
    step, saag = (cols[:-saag_tensors], cols[-saag_tensors:]) if saag_tensors else (cols, [])
    batch = [torch.stack(t) for t in step]
    if saag:
        counts = {int(t.shape[0]) for t in saag[0]}
        if len(counts) == 1 and counts != {0}:
            batch += [torch.stack(t) for t in saag]
    return tuple(batch)


class ImageDataset:
    def __init__(self, data_dir: str, image_size: int = 256, feature_cache_dir: Optional[str] = None,
                 max_images: Optional[int] = None, feature_dim: int = 384, load_vlm_density: bool = False,
                 load_saag: bool = False):
        self.data_dir = Path(data_dir)
        self.image_size = image_size
        self.feature_cache_dir = Path(feature_cache_dir) if feature_cache_dir else self.data_dir / "features"
        self.feature_dim = feature_dim
        self.load_vlm_density = load_vlm_density
        self.saag_tensors = 5 if load_saag else 0  # host_item appends the SAAG cloud (--experiment 1); 0: it returns what it returned
        self.feature_suffix = fio.feature_cache_suffix(feature_dim)
        paths: List[Path] = []
        for ext in ["*.jpg", "*.jpeg", "*.png", "*.webp"]:
            paths.extend(self.data_dir.glob(ext))
            paths.extend(self.data_dir.glob(ext.upper()))
        self.image_paths = sorted(paths)
        if max_images is not None and len(self.image_paths) > max_images:
            self.image_paths = self.image_paths[:max_images]

    def __len__(self) -> int:
        return len(self.image_paths)

    def _step_tensors(self, idx: int):
        """image, features (C,37,37), depth of item `idx` -- the three tensors a training step consumes."""
        from PIL import Image
        path = self.image_paths[idx]
        name = path.stem
        S = self.image_size
        img = Image.open(path).convert("RGB").resize((S, S), Image.Resampling.LANCZOS)
        image = (torch.from_numpy(np.array(img)).float() / 255.0).permute(2, 0, 1)
        fpath = self.feature_cache_dir / f"{name}{self.feature_suffix}"
        dpath = self.feature_cache_dir / f"{name}_depth.bin"
        features = (fio.load_feature_cache(str(fpath), self.feature_dim) if fpath.exists()
                    else torch.zeros(self.feature_dim, fio.FEATURE_GRID, fio.FEATURE_GRID))
        depth = fio.load_depth_cache(str(dpath), S) if dpath.exists() else torch.zeros(1, S, S)
        return name, image, features, depth

    def vlm_density(self, name: str):
        """(density (1,S,S), found): the VLM density grid of image `name` at the image size, in [0.5, 1.5] for a grid in
        [0, 1] (TGD:649-663); uniform weighting (ones) when the file is missing or cannot be used."""
        S = self.image_size
        path = self.feature_cache_dir / f"{name}_vlm_density.npy"
        if path.exists():
            try:
                grid = torch.from_numpy(np.load(path)).double()
                if grid.dim() != 2 or grid.shape[0] != grid.shape[1] or grid.shape[0] < 1:
                    raise ValueError(f"density grid of shape {tuple(grid.shape)}")
                if grid.shape[0] == 1:
                    full = grid.expand(S, S)
                else:  # zoom(order=1) samples the grid corner to corner
                    full = torch.nn.functional.interpolate(grid[None, None], size=(S, S), mode="bilinear", align_corners=True)[0, 0]
                return (0.5 + full).float().unsqueeze(0).contiguous(), True
            except Exception:  # as the reference: an unreadable map means uniform weighting, not a failed run
                pass
        return torch.ones(1, S, S), False

    def saag_cloud(self, name: str):
        """(has_saag, {saag_positions (N,3), saag_scales (N,3), saag_rotations (N,4), saag_colors (N,3), saag_opacities (N,)}) of
        image `name`: the `{name}_saag.bin` cache, or empty tensors (N = 0) when there is none (TGD:632-647)."""
        spath = self.feature_cache_dir / f"{name}_saag.bin"
        if spath.exists():
            saag = fio.load_gaussians_from_binary(str(spath))
            return True, {"saag_" + k: saag[k].float() for k in ("positions", "scales", "rotations", "colors", "opacities")}
        return False, dict(saag_positions=torch.zeros(0, 3), saag_scales=torch.zeros(0, 3), saag_rotations=torch.zeros(0, 4),
                           saag_colors=torch.zeros(0, 3), saag_opacities=torch.zeros(0))

    def __getitem__(self, idx: int) -> Dict[str, torch.Tensor]:
        name, image, features, depth = self._step_tensors(idx)
        has_saag, cloud = self.saag_cloud(name)
        item = {"image": image, "features": features, "depth": depth, "has_saag": has_saag, "name": name}
        item.update(cloud)
        if self.load_vlm_density:
            item["vlm_density"], item["has_vlm_density"] = self.vlm_density(name)
        return item

    def host_item(self, idx: int):
        """(image (3,S,S), features (37,37,C) patch-major as the decoder takes them, depth (1,S,S)[, density (1,S,S)]) on the host: what the
        training loop's prefetch threads load ahead of the step (fresnel_amd/train.py BatchPrefetcher)."""
        name, image, features, depth = self._step_tensors(idx)  # (not self[idx]: the SAAG binaries are part of an --experiment 1 step only)
        item = (image, features.permute(1, 2, 0).contiguous(), depth)
        if self.load_vlm_density:  # the fourth tensor of a --use_vlm_guidance step
            item += (self.vlm_density(name)[0],)
        if self.saag_tensors:  # load_saag: the five SAAG tensors behind them, empty where the image has no cloud
            cloud = self.saag_cloud(name)[1]
            item += tuple(cloud["saag_" + k] for k in ("positions", "scales", "rotations", "colors", "opacities"))
        return item

    def batch(self, indices, device):
        """(images (B,3,S,S), features (B,37,37,C) patch-major as the decoder takes them, depth (B,1,S,S)[, density (B,1,S,S)])
        [, the five SAAG tensors: with load_saag, when every item has a cloud and all clouds have the same count]."""
        if self.saag_tensors:
            return tuple(t.to(device) for t in collate_host_items([self.host_item(i) for i in indices], self.saag_tensors))
        items = [self[i] for i in indices]
        images = torch.stack([it["image"] for it in items]).to(device)
        feats = torch.stack([it["features"].permute(1, 2, 0) for it in items]).to(device)
        depth = torch.stack([it["depth"] for it in items]).to(device)
        if self.load_vlm_density:
            return images, feats, depth, torch.stack([it["vlm_density"] for it in items]).to(device)
        return images, feats, depth
