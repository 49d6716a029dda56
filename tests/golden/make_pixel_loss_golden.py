#!/usr/bin/env python3
"""Generator of G17_pixel_losses_48x40.npz (runs ONLY in the build container, never on the GPU box).

G17: the per-pixel part of the reference's training loss -- VLM-density-weighted L1, normalised-depth L1 and the
Fresnel-zone boundary emphasis term (scripts/training/train_gaussian_decoder.py compute_losses, lines 838-1003, with
scripts/utils/fresnel_zones.py FresnelZones) -- on a (3, 3, 48, 40) batch, values and input gradients.

As for G11 (make_goldens.py loss_goldens) the training module cannot be imported whole (torchvision), so the definitions
under test -- TrainingConfig, PhaseRetrievalLoss, FrequencyDomainLoss, wave_equation_loss, compute_losses -- are parsed
out of the file with `ast` and executed in a namespace that holds what they use, with SSIM_AVAILABLE = LPIPS_AVAILABLE =
False; FresnelZones is imported from its module.  The reference's own code runs; nothing of it is stored: the fixture
holds inputs, the three terms, the total and both gradients.

Records:
  a_*  use_vlm_guidance (vlm_weight 0.5, density at 24 x 20, resized by the reference) + use_fresnel_zones (8 zones on
       (0, 1), boundary_weight 0.1) + depth
  b_*  the same inputs without density and without zones: plain L1 + depth
Both share the inputs; rendered[0, :, :6, :5] = target[0, :, :6, :5] = 0 is a block of exact ties.
"""
import ast
import os
import sys

REF = "/root/reference/scripts"
if not os.path.isdir(REF):
    sys.exit("make_pixel_loss_golden.py: /root/reference is absent; goldens can only be generated in the build container")
sys.path.insert(0, REF)

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from utils.fresnel_zones import FresnelZones  # noqa: E402  (the reference, read-only)

OUT = os.path.dirname(os.path.abspath(__file__))


def reference_namespace():
    import dataclasses
    import typing
    path = os.path.join(REF, "training", "train_gaussian_decoder.py")
    tree = ast.parse(open(path).read())
    want = {"TrainingConfig", "PhaseRetrievalLoss", "FrequencyDomainLoss", "wave_equation_loss", "compute_losses"}
    body = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in want]
    assert {n.name for n in body} == want
    ns = dict(torch=torch, nn=nn, F=F, np=np, dataclass=dataclasses.dataclass, field=dataclasses.field,
              SSIM_AVAILABLE=False, LPIPS_AVAILABLE=False)
    ns.update({k: getattr(typing, k) for k in ("Tuple", "Optional", "Dict", "List", "Any", "Union")})
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def main():
    torch.set_num_threads(8)
    ns = reference_namespace()
    rs = np.random.RandomState(1717)
    Bn, H, W = 3, 48, 40
    target = rs.uniform(0.0, 1.0, (Bn, 3, H, W)).astype(np.float32)
    rendered = np.clip(target + rs.normal(0.0, 0.4, (Bn, 3, H, W)), 0.0, 1.2).astype(np.float32)
    rendered[0, :, :6, :5] = 0.0  # exact ties: a clamped render of 0 over a target of 0
    target[0, :, :6, :5] = 0.0
    target_depth = rs.uniform(0.0, 1.0, (Bn, H, W)).astype(np.float32)
    rendered_depth = (0.3 + 2.0 * target_depth + rs.normal(0.0, 0.5, (Bn, H, W))).astype(np.float32)
    density = (0.5 + rs.uniform(0.0, 1.0, (Bn, 1, H // 2, W // 2))).astype(np.float32)
    rec = dict(rendered=rendered, target=target, rendered_depth=rendered_depth, target_depth=target_depth, density=density,
               vlm_weight=np.float32(0.5), boundary_weight=np.float32(0.1), num_zones=np.int32(8),
               tie_block=np.array([0, 6, 5], np.int32))

    def run(tag, cfg, vlm, zones):
        r = torch.tensor(rendered, requires_grad=True)
        d = torch.tensor(rendered_depth, requires_grad=True)
        total, terms = ns["compute_losses"](r, torch.tensor(target), d, torch.tensor(target_depth), config=cfg,
                                            vlm_density=vlm, fresnel_zones=zones)
        total.backward()
        for k in ("rgb", "depth", "boundary"):
            if k in terms:
                rec[f"{tag}_{k}"] = np.float32(terms[k])
        rec[f"{tag}_total"] = np.float32(total.item())
        rec[f"{tag}_grad_rendered"] = r.grad.numpy()
        rec[f"{tag}_grad_rendered_depth"] = d.grad.numpy()
        print(tag, {k: v for k, v in terms.items()})

    cfg_a = ns["TrainingConfig"](use_vlm_guidance=True, vlm_weight=0.5, use_fresnel_zones=True, num_fresnel_zones=8)
    assert abs(cfg_a.boundary_weight - 0.1) < 1e-12 and cfg_a.depth_weight == 0.1 and cfg_a.rgb_weight == 1.0
    zones = FresnelZones(cfg_a.num_fresnel_zones, (0.0, 1.0), soft_boundaries=True)  # as TGD:1952-1959
    run("a", cfg_a, torch.tensor(density), zones)
    run("b", ns["TrainingConfig"](), None, None)
    rec["meta_torch"] = np.array(torch.__version__)
    rec["meta_numpy"] = np.array(np.__version__)
    rec["meta_device"] = np.array("cpu")
    path = os.path.join(OUT, "G17_pixel_losses_48x40.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
