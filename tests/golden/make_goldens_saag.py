"""Fixtures of the SAAG refinement decoder: the reference's SAAGRefinementNet (scripts/models/gaussian_decoder_models.py,
GDM:424-570) run on the CPU in eval mode.  Runs only where the reference is present (FRESNEL_REFERENCE = its checkout); the
fixtures hold data only:

    ctor            the constructor's keyword arguments, as JSON
    sd.<key>        the state dict
    in.<name>       features, saag_positions, saag_scales, saag_rotations, saag_colors, saag_opacities
    raw             the MLP's output, captured by a forward hook, as (B, N, 16)
    out.<name>      every entry of the returned dict                                  g.<name>  the upstream gradient of that entry
    grad.raw, grad.sd.<parameter>     gradients of sum_name sum(out.<name> x g.<name>); zeros where autograd gave none

  R1 feature_dim 8, hidden [16, 8], features (2, 8, 5, 7), N = 50: z on both sides of 0.1, non-unit SAAG quaternions, some colours and
     opacities exactly 0 and 1
  R2 feature_dim 32, a 37 x 37 grid, B = 1, N = 200, drawn as the training script's create_dummy_saag draws (z about -2, identity
     quaternions, opacity 0.8): most sample coordinates sit on the 0 / 1 clamps
  R3 feature_dim 7 (odd row width 21), grid (3, 4), B = 3, N = 65

Pinned harness-side while the reference runs: the random sign it adds to b2 before normalising (GDM:208, 1e-8 sign(randn)) is +1 --
the draw this repository's rotation code fixes.  The last layer's weights are scaled up so that the raw outputs
spread over a few units, the four gains are moved off their initial values, and a seed is taken only if no Gaussian sits within
1e-3 of a quaternion-branch boundary (tests/head_checker.py branch_info): q and -q are the same rotation but not the same numbers.
"""
import contextlib
import json
import os
import sys

REF = os.environ.get("FRESNEL_REFERENCE", "")
if not os.path.isdir(os.path.join(REF, "scripts")):
    sys.exit("make_goldens_saag.py: set FRESNEL_REFERENCE to a checkout of the reference; fixtures can only be generated where it is present")
sys.path.insert(0, os.path.join(REF, "scripts"))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import models.gaussian_decoder_models as gdm  # noqa: E402  (the reference, read-only)
import head_checker as hc  # noqa: E402

torch.set_num_threads(8)
META = dict(torch=torch.__version__, numpy=np.__version__, device="cpu")
CLOUD = ("positions", "scales", "rotations", "colors", "opacities")


@contextlib.contextmanager
def pinned():
    randn_like = torch.randn_like
    torch.randn_like = lambda t, **kw: torch.ones_like(t)
    try:
        yield
    finally:
        torch.randn_like = randn_like


def cloud_mixed(Bn, N, g):
    """z on both sides of 0.1 (and exactly 0.1), non-unit quaternions, colours and opacities with exact 0 and 1."""
    pos = torch.randn(Bn, N, 3, generator=g)
    pos[..., 2] = torch.rand(Bn, N, generator=g) * 1.2 - 0.3
    pos[:, 0, 2] = 0.1
    rot = torch.randn(Bn, N, 4, generator=g) * 1.5
    col, opa = torch.rand(Bn, N, 3, generator=g), torch.rand(Bn, N, generator=g)
    col[:, 1::7], col[:, 2::7] = 0.0, 1.0
    opa[:, 3::5], opa[:, 4::5] = 0.0, 1.0
    return dict(positions=pos, scales=torch.rand(Bn, N, 3, generator=g) * 0.2 + 0.01, rotations=rot, colors=col, opacities=opa)


def cloud_dummy(Bn, N, g):
    """The distribution of the training script's create_dummy_saag (TGD:760-778)."""
    pos = torch.randn(Bn, N, 3, generator=g) * 0.5
    pos[..., 2] -= 2
    rot = torch.zeros(Bn, N, 4)
    rot[..., 0] = 1
    return dict(positions=pos, scales=torch.ones(Bn, N, 3) * 0.05, rotations=rot, colors=torch.rand(Bn, N, 3, generator=g),
                opacities=torch.ones(Bn, N) * 0.8)


def run(ctor, feat_shape, N, cloud_fn, seed):
    torch.manual_seed(seed)
    model = gdm.SAAGRefinementNet(**ctor).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        last = model.mlp.net[-1]
        last.weight.mul_(6.0)
        last.bias.copy_(torch.randn(last.bias.shape, generator=g))
        for p in (model.pos_scale, model.scale_scale, model.color_scale, model.opacity_scale):
            p.mul_(0.5 + 3.0 * float(torch.rand((), generator=g)))
    Bn = feat_shape[0]
    features = torch.randn(*feat_shape, generator=g)
    cloud = cloud_fn(Bn, N, g)
    captured = {}

    def hook(_m, _i, out):
        out.retain_grad()
        captured["raw"] = out

    h = model.mlp.register_forward_hook(hook)
    with pinned():
        out = model(features, *[cloud[k] for k in CLOUD])
        ups = {k: torch.randn(v.shape, generator=g) for k, v in out.items()}
        sum((out[k] * ups[k]).sum() for k in out).backward()
    h.remove()
    raw = captured["raw"]
    rec = dict(class_name=np.array("SAAGRefinementNet"), ctor=np.array(json.dumps(ctor)), seed=np.int32(seed),
               raw=raw.detach().reshape(Bn, N, 16).numpy())
    rec["grad.raw"] = raw.grad.reshape(Bn, N, 16).numpy()
    rec["in.features"] = features.numpy()
    for k in CLOUD:
        rec["in.saag_" + k] = cloud[k].numpy()
    for k, v in model.state_dict().items():
        rec["sd." + k] = v.numpy()
    for k, p in model.named_parameters():
        rec["grad.sd." + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    for k in out:
        rec["out." + k] = out[k].detach().numpy()
        rec["g." + k] = ups[k].numpy()
    for k, v in META.items():
        rec["meta_" + k] = np.array(v)
    branch, trace, gap = hc.branch_info(raw.detach().double().reshape(Bn, N, 16)[..., 6:12])
    near = (trace.abs() < 1e-3) | ((branch != 0) & (gap < 1e-3))
    return rec, int(near.sum())


def main():
    cases = [
        ("R1_saag_mixed", dict(feature_dim=8, hidden_dims=[16, 8]), (2, 8, 5, 7), 50, cloud_mixed),
        ("R2_saag_dummy37", dict(feature_dim=32, hidden_dims=[16, 8]), (1, 32, 37, 37), 200, cloud_dummy),
        ("R3_saag_odd", dict(feature_dim=7, hidden_dims=[16, 8], residual_scale=0.25), (3, 7, 3, 4), 65, cloud_mixed),
    ]
    for k, (name, ctor, feat_shape, N, cloud_fn) in enumerate(cases):
        seed = 800 + 10 * k
        while True:
            rec, near = run(ctor, feat_shape, N, cloud_fn, seed)
            if near == 0:
                break
            seed += 1
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **rec)
        print(f"{name}: seed {seed}, {os.path.getsize(path) / 1024:.0f} KB, raw std {rec['raw'].std():.2f}")


if __name__ == "__main__":
    main()
