"""Fixtures of the decoder mirrors and their Gaussian-parameter head: the reference's DirectPatchDecoder and FibonacciPatchDecoder
(scripts/models/gaussian_decoder_models.py, GDM:622-948, 1493-1747) run on the CPU in eval mode.  Runs only where the reference is
present (FRESNEL_REFERENCE = its checkout); the fixtures hold data only:

    ctor            the constructor's keyword arguments, as JSON                      class_name
    sd.<key>        the state dict
    in.<name>       features, depth, elevation, azimuth, num_gaussians (those that were passed)
    raw             the MLP's output, captured by a forward hook, as (B, P, K_full, C)
    out.<name>      every entry of the returned dict                                  g.<name>  the upstream gradient of that entry
    grad.raw, grad.features, grad.sd.<parameter>     gradients of sum_name sum(out.<name> x g.<name>); zeros where autograd gave none

  H1 DirectPatchDecoder    feature_dim 8, hidden [16, 8], K_full 3 used 2, features (2,8,5,7), depth (2,1,24,24), two poses, all five
                           options on (zones, edge-aware, phases, pose encoding, depth fusion)
  H2 FibonacciPatchDecoder 55 points, phases, pose encoding, zones
  H3 DirectPatchDecoder    no depth, no options, 16 channels

Two things are pinned harness-side while the reference runs:
  * the random sign it adds to b2 before normalising (GDM:208, 1e-8 sign(randn)) is +1 -- the draw this repository's head fixes
    (DESIGN.md section 7);
  * its DepthEncoder pools to a fixed 37 x 37 grid (GDM:613), which only fits 37 x 37 features; the pool goes to the fixture's
    small feature grid instead (the same operation on the reference's own grid).
The last layer's weights are scaled up so that the raw outputs spread over a few units, and a seed is taken only if no used
Gaussian sits within 1e-3 of a quaternion-branch boundary (tests/head_checker.py branch_info): q and -q are the same rotation
but not the same numbers.
"""
import contextlib
import json
import os
import sys

REF = os.environ.get("FRESNEL_REFERENCE", "")
if not os.path.isdir(os.path.join(REF, "scripts")):
    sys.exit("make_goldens_head.py: set FRESNEL_REFERENCE to a checkout of the reference; fixtures can only be generated where it is present")
sys.path.insert(0, os.path.join(REF, "scripts"))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import models.gaussian_decoder_models as gdm  # noqa: E402  (the reference, read-only)
import head_checker as hc  # noqa: E402

torch.set_num_threads(8)
META = dict(torch=torch.__version__, numpy=np.__version__, device="cpu")


@contextlib.contextmanager
def pinned(grid):
    randn_like, pool = torch.randn_like, gdm.F.adaptive_avg_pool2d
    torch.randn_like = lambda t, **kw: torch.ones_like(t)
    gdm.F.adaptive_avg_pool2d = lambda x, size: pool(x, grid if tuple(size) == (37, 37) else size)
    try:
        yield
    finally:
        torch.randn_like, gdm.F.adaptive_avg_pool2d = randn_like, pool


def run(cls, ctor, shapes, seed, num_gaussians=None, posed=True, with_depth=True):
    torch.manual_seed(seed)
    model = getattr(gdm, cls)(**ctor).eval()
    with torch.no_grad():
        last = model.mlp.net[-1]
        last.weight.mul_(6.0)
        last.bias.copy_(torch.randn_like(last.bias))
    g = torch.Generator().manual_seed(seed + 1)
    Bn = shapes["features"][0]
    inputs = dict(features=torch.randn(*shapes["features"], generator=g))
    if with_depth:
        inputs["depth"] = torch.rand(*shapes["depth"], generator=g)
    if posed:
        inputs["elevation"] = (torch.rand(Bn, generator=g) - 0.4) * 1.2
        inputs["azimuth"] = torch.rand(Bn, generator=g) * 6.0
    inputs["features"].requires_grad_(True)
    captured = {}

    def hook(_m, _i, out):
        out.retain_grad()
        captured["raw"] = out

    h = model.mlp.register_forward_hook(hook)
    kw = dict(inputs)
    if num_gaussians is not None:
        kw["num_gaussians"] = num_gaussians
    with pinned(tuple(shapes["features"][2:])):
        out = model(**kw)
        ups = {k: torch.randn(v.shape, generator=g) for k, v in out.items()}
        sum((out[k] * ups[k]).sum() for k in out).backward()
    h.remove()
    KF = ctor.get("gaussians_per_patch", ctor.get("gaussians_per_point", 1))
    C = model.output_per_gaussian
    raw = captured["raw"]
    P = raw.shape[0] // Bn
    rec = dict(class_name=np.array(cls), ctor=np.array(json.dumps(ctor)), raw=raw.detach().reshape(Bn, P, KF, C).numpy(),
               seed=np.int32(seed))
    rec["grad.raw"] = raw.grad.reshape(Bn, P, KF, C).numpy()
    rec["grad.features"] = inputs["features"].grad.numpy()
    for k, v in inputs.items():
        rec["in." + k] = v.detach().numpy()
    if num_gaussians is not None:
        rec["in.num_gaussians"] = np.int32(num_gaussians)
    for k, v in model.state_dict().items():
        rec["sd." + k] = v.numpy()
    for k, p in model.named_parameters():
        rec["grad.sd." + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    for k in out:
        rec["out." + k] = out[k].detach().numpy()
        rec["g." + k] = ups[k].numpy()
    for k, v in META.items():
        rec["meta_" + k] = np.array(v)
    K = KF if num_gaussians is None else min(num_gaussians, KF)
    _, trace, gap = hc.branch_info(raw.detach().double().reshape(Bn, P, KF, C)[:, :, :K, 6:12])
    branch = hc.branch_info(raw.detach().double().reshape(Bn, P, KF, C)[:, :, :K, 6:12])[0]
    near = (trace.abs() < 1e-3) | ((branch != 0) & (gap < 1e-3))
    return rec, int(near.sum())


def main():
    small = dict(features=(2, 8, 5, 7), depth=(2, 1, 24, 24))
    cases = [
        ("H1_head_direct_all", "DirectPatchDecoder",
         dict(feature_dim=8, gaussians_per_patch=3, hidden_dims=[16, 8], use_fresnel_zones=True, num_fresnel_zones=8,
              use_edge_aware=True, use_phase_output=True, use_pose_encoding=True, pose_embed_dim=16, use_depth_fusion=True,
              depth_feature_dim=4), small, dict(num_gaussians=2)),
        ("H2_head_fibonacci55", "FibonacciPatchDecoder",
         dict(feature_dim=8, n_spiral_points=55, gaussians_per_point=1, hidden_dims=[16, 8], use_fresnel_zones=True,
              num_fresnel_zones=8, use_phase_output=True, use_pose_encoding=True, pose_embed_dim=16), small, {}),
        ("H3_head_direct_plain", "DirectPatchDecoder",
         dict(feature_dim=8, gaussians_per_patch=2, hidden_dims=[16]), dict(features=(3, 8, 6, 4)),
         dict(posed=False, with_depth=False)),
    ]
    for k, (name, cls, ctor, shapes, kw) in enumerate(cases):
        seed = 500 + 10 * k
        while True:
            rec, near = run(cls, ctor, shapes, seed, **kw)
            if near == 0:
                break
            seed += 1
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **rec)
        print(f"{name}: seed {seed}, {os.path.getsize(path) / 1024:.0f} KB, raw std {rec['raw'].std():.2f}")


if __name__ == "__main__":
    main()
