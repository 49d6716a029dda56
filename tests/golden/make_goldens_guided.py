#!/usr/bin/env python3
"""Generate the FeatureGuidedSAAG fixture (tests/golden/FG1_guided_mods.npz) by running the reference's own class.

Imports the reference's decoder models from /root/reference/scripts (read-only) and runs its FeatureGuidedSAAG with feature_dim 8,
hidden_dim 4 on seeded features (2, 8, 5, 7), with a seeded NON-ZERO last layer (the class zero-initialises it, which would make
every map constant).  Stored, in fp32 and in fp64: the state dict, the features, the six maps and the gradients of the parameters
under a seeded linear functional of the maps.  Nothing of the reference is copied: the fixture holds numbers only.

    python tests/golden/make_goldens_guided.py        (where the reference is present)
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference/scripts"
if not os.path.isdir(REF):
    sys.exit("make_goldens_guided.py: /root/reference is absent; goldens can only be generated where the reference is present")
sys.path.insert(0, REF)
from models.gaussian_decoder_models import FeatureGuidedSAAG  # noqa: E402  (the reference, read-only)

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("aspect_ratio_mult", "edge_threshold_add", "edge_shrink_mult", "normal_strength_mult", "base_size_mult", "opacity_mult")


def main():
    g = torch.Generator().manual_seed(20240603)
    model = FeatureGuidedSAAG(feature_dim=8, num_params=6, hidden_dim=4)
    with torch.no_grad():
        for p in model.parameters():                      # every layer seeded, the last one NON-ZERO
            p.copy_(torch.randn(p.shape, generator=g) * 0.6)
    features = torch.randn(2, 8, 5, 7, generator=g)
    weights = torch.randn(6, 2, 5, 7, generator=g)        # the linear functional: sum_k <weights[k], map_k>
    out = {"features": features.numpy(), "weights": weights.numpy(), "keys": np.array(KEYS)}
    for name, p in model.state_dict().items():
        out["state." + name] = p.detach().numpy().copy()
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        m = FeatureGuidedSAAG(feature_dim=8, num_params=6, hidden_dim=4).to(dt)
        m.load_state_dict({k: v.to(dt) for k, v in model.state_dict().items()}, strict=True)
        maps = m(features.to(dt))
        assert tuple(maps) == KEYS, tuple(maps)
        loss = sum((weights[i].to(dt) * maps[k]).sum() for i, k in enumerate(KEYS))
        loss.backward()
        for k in KEYS:
            out[f"{tag}.map.{k}"] = maps[k].detach().numpy()
        for name, p in m.named_parameters():
            out[f"{tag}.grad.{name}"] = p.grad.numpy().copy()
    path = os.path.join(HERE, "FG1_guided_mods.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
