"""Fixtures of the physics-phase decoder: the reference's PhysicsDirectPatchDecoder (scripts/models/gaussian_decoder_models.py,
GDM:955-1147) run on the CPU in eval mode, once in fp32 and once as a double copy of the same module.  Runs only where the
reference is present (FRESNEL_REFERENCE = its checkout); the fixtures hold data only:

    ctor, num_gaussians   the constructor's keyword arguments as JSON; the forward's num_gaussians (-1: None)
    sd.<key>              the state dict
    in.features, in.depth the inputs (no in.depth: depth=None)
    patches               the patches p whose Gaussians the per-Gaussian entries below hold (all of them in P1 and P2)
    raw                   the MLP's output, captured by a forward hook, (B, len(patches), K_full, 16)
    out.<name>            every entry of the returned dict at those patches' Gaussians;  out.phases_full: the phases of ALL Gaussians
    g.<name>              the upstream gradient of every entry, whole (P1, P2); P3 stores none: g_formula = 1 says that it is
                          physics_checker.formula_upstream(shape, salt = position of <name> in OUTPUTS), as in P1 and P2
    grad.raw, grad.sd.<parameter>      gradients of sum_name sum(out.<name> x g.<name>); zeros where autograd gave none
    f64.out.<name>, f64.out.phases_full, f64.grad.raw, f64.grad.sd.<parameter>     the same from the double copy
    dev.<entry>           max |fp32 - fp64| of that entry (out.*, grad.raw, grad.sd.*); for phases the largest CIRCULAR distance
    sum_abs_g_base_z      sum |dL/d base_z| of the double run: the scale that grad.sd.depth_offset (= sum dL/d base_z, whose phase
                          part cancels) is judged by

  P1 feature_dim 8, hidden [16, 8], grid 5 x 7, B 2, K_full 3, num_gaussians 2; the depth has a block of exact zeros in image 0 and
     a block of exact ones in image 1: minimum and maximum are each held by several patches.  _wavelength_raw 0.05
  P2 the same module with depth=None, B 1: z is constant, every phase the same number, no gradient to depth_offset
  P3 feature_dim 32, hidden [16, 8], grid 37 x 37, B 1, K 8; _wavelength_raw -0.02 (negative; unwrapped phase up to 157),
     learnable_wavelength=False, use_diffraction_placement=True.  10 952 Gaussians x 15 outputs x (value, gradient, double copy) do
     not fit a committed file: the per-Gaussian entries hold every 16th patch, the phases are whole, and the parameter gradients
     (sums over ALL Gaussians) cover the rest

Pinned harness-side while the reference runs: the random sign it adds to b2 before normalising (GDM:208, 1e-8 sign(randn)) is +1 --
the draw this repository's rotation code fixes.  The last layer's weights are scaled up so that the raw outputs
spread over a few units, and a seed is taken only if no stored Gaussian sits within 1e-3 of a quaternion-branch boundary
(tests/head_checker.py branch_info; and none at all within 1e-5): q and -q are the same rotation but not the same numbers.
"""
import contextlib
import copy
import json
import os
import sys

REF = os.environ.get("FRESNEL_REFERENCE", "")
if not os.path.isdir(os.path.join(REF, "scripts")):
    sys.exit("make_goldens_physics.py: set FRESNEL_REFERENCE to a checkout of the reference; fixtures can only be generated where it is present")
sys.path.insert(0, os.path.join(REF, "scripts"))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import models.gaussian_decoder_models as gdm  # noqa: E402  (the reference, read-only)
import head_checker as hc  # noqa: E402
import physics_checker as pc  # noqa: E402

torch.set_num_threads(8)
META = dict(torch=torch.__version__, numpy=np.__version__, device="cpu")


@contextlib.contextmanager
def pinned():
    randn_like = torch.randn_like
    torch.randn_like = lambda t, **kw: torch.ones_like(t)
    try:
        yield
    finally:
        torch.randn_like = randn_like


def tied_depth(Bn, h, w, g):
    """Random depth in (0.05, 0.95) with a block of exact zeros in image 0 and a block of exact ones in the last image, each wide
    enough that several cells of the bilinearly reduced grid are exactly 0 / 1."""
    d = torch.rand(Bn, 1, h, w, generator=g) * 0.9 + 0.05
    d[0, 0, : h // 2, : w // 2] = 0.0
    d[-1, 0, h // 2:, w // 2:] = 1.0
    return d


def one_run(model, features, depth, num_gaussians, dtype):
    model = copy.deepcopy(model).to(dtype)
    captured = {}

    def hook(_m, _i, out):
        out.retain_grad()
        captured["raw"] = out

    h = model.mlp.register_forward_hook(hook)
    with pinned():
        out = model(features.to(dtype), None if depth is None else depth.to(dtype), num_gaussians=num_gaussians)
        ups = {k: pc.formula_upstream(v.shape, pc.OUTPUTS.index(k)) for k, v in out.items()}
        sum((out[k] * ups[k].to(dtype)).sum() for k in out).backward()
    h.remove()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}
    return {k: v.detach() for k, v in out.items()}, ups, captured["raw"].detach(), captured["raw"].grad, grads


def run(ctor, grid, Bn, num_gaussians, with_depth, wavelength_raw, patch_step, seed):
    torch.manual_seed(seed)
    model = gdm.PhysicsDirectPatchDecoder(**ctor).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        last = model.mlp.net[-1]
        last.weight.mul_(6.0)
        last.bias.copy_(torch.randn(last.bias.shape, generator=g))
        model.fresnel_zones._wavelength_raw.fill_(wavelength_raw)
        model.depth_offset.add_(0.25)
    H, W = grid
    KF = ctor["gaussians_per_patch"]
    K = KF if num_gaussians is None else min(num_gaussians, KF)
    features = torch.randn(Bn, ctor["feature_dim"], H, W, generator=g)
    depth = tied_depth(Bn, 4 * H, 4 * W, g) if with_depth else None
    out, ups, raw, g_raw, grads = one_run(model, features, depth, num_gaussians, torch.float32)
    out64, _, _, g_raw64, grads64 = one_run(model, features, depth, num_gaussians, torch.float64)
    P = H * W
    patches = torch.arange(0, P, patch_step)
    gauss = (patches[:, None] * K + torch.arange(K)[None, :]).flatten()
    rec = dict(class_name=np.array("PhysicsDirectPatchDecoder"), ctor=np.array(json.dumps(ctor)), seed=np.int32(seed),
               num_gaussians=np.int32(-1 if num_gaussians is None else num_gaussians), patches=patches.numpy().astype(np.int32),
               g_formula=np.int32(1 if patch_step > 1 else 0))
    rec["in.features"] = features.numpy()
    if depth is not None:
        rec["in.depth"] = depth.numpy()
    for k, v in model.state_dict().items():
        rec["sd." + k] = v.numpy()

    def rows(t):  # (B P, K_full 16) -> (B, patches, K_full, 16)
        return t.reshape(Bn, P, KF, 16)[:, patches]

    rec["raw"] = rows(raw).numpy()
    # entry -> (fp32, fp64) as stored, (fp32, fp64) whole: the deviation is the whole tensor's
    entries = {"grad.raw": ((rows(g_raw), rows(g_raw64)), (g_raw, g_raw64)),
               "out.phases_full": ((out["phases"], out64["phases"]),) * 2}
    for k in out:
        entries["out." + k] = ((out[k][:, gauss], out64[k][:, gauss]), (out[k], out64[k]))
        if patch_step == 1:
            rec["g." + k] = ups[k].numpy()
    for k in grads:
        entries["grad.sd." + k] = ((grads[k], grads64[k]),) * 2
    for k, ((a, b), (fa, fb)) in entries.items():
        rec[k], rec["f64." + k] = a.numpy(), b.numpy()
        dev = pc.circular_distance(fa, fb) if "phases" in k else (fa.double() - fb).abs()
        rec["dev." + k] = np.float64(dev.max())
    # dL/d base_z of the double run: the scale of grad.sd.depth_offset
    bz = torch.zeros(Bn, P, dtype=torch.float64)
    if depth is not None:
        dg = torch.nn.functional.interpolate(depth.double(), (H, W), mode="bilinear", align_corners=False).reshape(Bn, P)
        bz = (model.depth_offset.detach().double() + dg * (-2)).requires_grad_(True)
        o = pc.head(raw.double().reshape(Bn, P, KF, 16), torch.zeros(P, 2), bz, model.fresnel_zones._wavelength_raw.detach().double(),
                    num_gaussians=num_gaussians)
        sum((o[k] * ups[k].double()).sum() for k in ("positions", "phases")).backward()
        bz = bz.grad
    rec["sum_abs_g_base_z"] = np.float64(bz.abs().sum())
    for k, v in META.items():
        rec["meta_" + k] = np.array(v)
    branch, trace, gap = hc.branch_info(raw.double().reshape(Bn, P, KF, 16)[:, :, :K, 6:12])
    def near(margin):
        return (trace.abs() < margin) | ((branch != 0) & (gap < margin))

    # P3: 1e-3 for the Gaussians whose values are stored; among all 10 952 some always sit that close, and only the parameter
    # gradients see them: 1e-5 there, a hundred times fp32's resolution
    return rec, int(near(1e-3)[:, patches].sum()) + int(near(1e-5).sum())


def main():
    small = dict(feature_dim=8, gaussians_per_patch=3, hidden_dims=[16, 8])
    cases = [
        ("P1_physics_ties", small, (5, 7), 2, 2, True, 0.05, 1),
        ("P2_physics_nodepth", small, (5, 7), 1, 2, False, 0.05, 1),
        ("P3_physics_grid37", dict(feature_dim=32, gaussians_per_patch=8, hidden_dims=[16, 8], learnable_wavelength=False,
                                   use_diffraction_placement=True), (37, 37), 1, None, True, -0.02, 16),
    ]
    seed = 900
    while True:  # P2 is "the same module" as P1: one seed for both
        runs = [run(*c[1:], seed) for c in cases[:2]]
        if all(near == 0 for _, near in runs):
            break
        seed += 1
        assert seed < 1100, 'no seed without a Gaussian near a branch boundary'
    done = [(cases[0][0], seed, runs[0][0]), (cases[1][0], seed, runs[1][0])]
    seed = 920
    while True:
        rec, near = run(*cases[2][1:], seed)
        if near == 0:
            break
        seed += 1
        assert seed < 1100, 'no seed without a Gaussian near a branch boundary'
    done.append((cases[2][0], seed, rec))
    for name, seed, rec in done:
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **rec)
        print(f"{name}: seed {seed}, {os.path.getsize(path) / 1024:.0f} KB, raw std {rec['raw'].std():.2f}, phase deviation "
              f"{rec['dev.out.phases_full']:.2e}, sum |g_base_z| {rec['sum_abs_g_base_z']:.3e}")


if __name__ == "__main__":
    main()
