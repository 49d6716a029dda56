"""The fused HIP Gaussian-parameter head (csrc/fgs_head.hip, fresnel_amd.decoder.gaussian_head backend "hip") on the GPU: parity
with the reference's fixtures H1-H3 and with the restated head (tests/head_checker.py) in fp32 and fp64 under the 1e-4-of-maximum
rule, degenerate rows, bitwise repeatability, the copy-free hand-off to the renderers and one captured training step."""
import math

import pytest
import torch

import head_checker as hc
from helpers import rel_to_max
from test_decoder_mirror import FIXTURES, assert_matches_fixture, build_mirror, fixture, head_inputs, run_mirror

gpu = pytest.mark.gpu
TOL = 1e-4
GROUPS = dict(position=slice(0, 3), scale=slice(3, 6), rotation=slice(6, 12), color=slice(12, 15), opacity=slice(15, 16),
              phase=slice(16, 19))


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _hip_head(args, ups, dev, skip_grad=()):
    """gaussian_head(backend 'hip') on CPU argument tensors -> outputs, gradients (CPU)."""
    from fresnel_amd.decoder import gaussian_head
    t = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in args.items()}
    leaves = {}
    for k in ("raw", "base_z", "opacity_mod", "edge"):
        if t.get(k) is not None:
            t[k] = leaves[k] = t[k].detach().clone().requires_grad_(True)
    out = gaussian_head(t.pop("raw"), t.pop("base_xy"), t.pop("base_z"), **t, backend="hip")
    sum((out[k] * ups[k].to(dev)).sum() for k in out if k not in skip_grad).backward()
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in out.items()}, {k: (v.grad if v.grad is not None else torch.zeros_like(v)).cpu() for k, v in leaves.items()}


def _checker(args, ups, dtype, skip_grad=()):
    t = {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in args.items()}
    leaves = {}
    for k in ("raw", "base_z", "opacity_mod", "edge"):
        if t.get(k) is not None:
            t[k] = leaves[k] = t[k].detach().clone().requires_grad_(True)
    out = hc.head(t.pop("raw"), t.pop("base_xy"), t.pop("base_z"), **t)
    sum((out[k] * ups[k].to(dtype)).sum() for k in out if k not in skip_grad).backward()
    return {k: v.detach() for k, v in out.items()}, {k: v.grad for k, v in leaves.items()}


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_hip_head_on_the_fixtures_raw_outputs(name):
    dev = _dev()
    fx = fixture(name)
    model, _ = build_mirror(fx)
    args = head_inputs(model, fx)
    args["raw"] = torch.from_numpy(fx["raw"])
    ups = {k: torch.from_numpy(fx["g." + k]) for k in hc.OUTPUTS if "g." + k in fx.files}
    out, grads = _hip_head(args, ups, dev)
    for k, v in out.items():
        e = rel_to_max(v.numpy(), fx["out." + k])
        print(f"{name}: {k} {e:.2e}")
        assert e <= TOL, f"{name}: {k} is {e:.2e} of its maximum away from the reference"
    e = rel_to_max(grads["raw"].numpy(), fx["grad.raw"])
    print(f"{name}: grad raw {e:.2e}")
    assert e <= TOL, f"{name}: the raw gradient is {e:.2e} of its maximum away from the reference"


@gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_mirror_with_hip_head_reproduces_every_fixture_gradient(name):
    dev = _dev()
    fx = fixture(name)
    model, _ = build_mirror(fx, head_backend="hip", device=dev)
    out, grads, raw = run_mirror(model, fx, dev)
    torch.cuda.synchronize()
    assert_matches_fixture(fx, out, grads, raw, name + " (hip head)")


# ---- random parity against the checker ---------------------------------------------------------------------------------------------
def _random_case(Bn, P, KF, K, C, pose, mod, edge, seed):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(Bn, P, KF, C, generator=g)
    raw[..., 3:6] *= 8.0   # both scale clamps and the softplus switch
    raw[..., 15] *= 4.0
    args = dict(raw=raw, base_xy=torch.rand(P, 2, generator=g) * 2 - 1, base_z=-2.0 - 2.0 * torch.rand(Bn, P, generator=g),
                num_gaussians=K, xy_gain=0.15 if KF == 1 else 0.25, edge_scale_factor=0.5, edge_opacity_boost=0.2)
    if pose:
        el, az = torch.linspace(-0.4, 0.7, Bn), torch.linspace(0.3, 5.0, Bn)   # a different pose per image
        args["pose"] = torch.stack([torch.cos(az), torch.sin(az), torch.cos(el), torch.sin(el)], -1)
    if mod:
        args["opacity_mod"] = 0.5 + torch.rand(Bn, generator=g)
    if edge:
        args["edge"] = torch.rand(Bn, P, generator=g)
    N = P * K
    ups = dict(positions=torch.randn(Bn, N, 3, generator=g), scales=torch.randn(Bn, N, 3, generator=g),
               rotations=torch.randn(Bn, N, 4, generator=g), colors=torch.randn(Bn, N, 3, generator=g),
               opacities=torch.randn(Bn, N, generator=g))
    if C == 19:
        ups["phases"] = torch.randn(Bn, N, 3, generator=g)
    return args, ups


def _near_boundary(args):
    """Gaussians (B, P K) whose quaternion branch the fp64 checker decides by less than 1e-3: |trace|, or outside branch 1 the
    smallest diagonal difference."""
    raw = args["raw"].double()
    K = args["num_gaussians"]
    branch, trace, gap = hc.branch_info(raw[:, :, :K, 6:12])
    near = (trace.abs() < 1e-3) | ((branch != 0) & (gap < 1e-3))
    return near.reshape(raw.shape[0], -1), branch.reshape(raw.shape[0], -1)


def _compare(tag, out, grads, ref_out, ref_grads, near, K):
    for k, v in out.items():
        a, b = v.double(), ref_out[k].double()
        if k == "rotations":
            nrm = a.norm(dim=-1)
            assert float((nrm - 1).abs().max()) <= 1e-5
            both = torch.minimum((a - b).abs().amax(-1), (a + b).abs().amax(-1))
            assert float(both[near].max() if near.any() else 0.0) <= TOL, f"{tag}: a left-out quaternion matches neither q nor -q"
            a, b = a[~near], b[~near]
        e = rel_to_max(a.numpy(), b.numpy())
        print(f"{tag}: {k} {e:.2e}")
        assert e <= TOL, f"{tag}: {k} is {e:.2e} of its maximum away"
    for k, v in grads.items():
        a, b = v.double(), ref_grads[k].double()
        if k != "raw":
            e = rel_to_max(a.numpy(), b.numpy())
            print(f"{tag}: grad {k} {e:.2e}")
            assert e <= TOL, f"{tag}: the gradient of {k} is {e:.2e} of its maximum away"
            continue
        assert not a[:, :, K:].any(), f"{tag}: g_raw of the unused Gaussians is not zero"
        keep = (~near).reshape(a.shape[0], a.shape[1], K)
        for name, sl in GROUPS.items():
            if sl.start >= a.shape[-1]:
                continue
            ga, gb = a[:, :, :K, sl], b[:, :, :K, sl]
            if name == "rotation":
                ga, gb = ga[keep], gb[keep]
            e = rel_to_max(ga.numpy(), gb.numpy())
            print(f"{tag}: grad raw[{name}] {e:.2e}")
            assert e <= TOL, f"{tag}: the {name} channels of g_raw are {e:.2e} of their maximum away"


CASES = {
    "under_one_wave": dict(Bn=1, P=55, KF=1, K=1, C=19, pose=True, mod=True, edge=False),
    "strided_rows": dict(Bn=2, P=35, KF=3, K=2, C=16, pose=False, mod=False, edge=True),
    "blocks": dict(Bn=3, P=377, KF=4, K=3, C=19, pose=True, mod=True, edge=True),
    "blocks_plain": dict(Bn=3, P=377, KF=4, K=3, C=19, pose=False, mod=False, edge=False),
    "pose_only": dict(Bn=2, P=35, KF=3, K=2, C=16, pose=True, mod=False, edge=False),
    "mod_only": dict(Bn=2, P=35, KF=3, K=2, C=16, pose=False, mod=True, edge=False),
}


@gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_random_parity_with_the_checker(case):
    dev = _dev()
    c = CASES[case]
    args, ups = _random_case(seed=700 + sorted(CASES).index(case), **c)
    near, branch = _near_boundary(args)
    share = float(near.float().mean())
    print(f"{case}: {share * 100:.2f} % of the Gaussians are near a branch boundary; branches "
          f"{[round(float((branch == i).float().mean()), 3) for i in range(4)]}")
    assert share <= 0.02
    if near.numel() >= 1000:  # (a case of a few dozen Gaussians cannot promise a share per branch)
        assert all(float((branch == i).float().mean()) >= 0.10 for i in range(4))
    out, grads = _hip_head(args, ups, dev)
    for dtype in (torch.float64, torch.float32):
        ref_out, ref_grads = _checker(args, ups, dtype)
        _compare(f"{case} vs {str(dtype)[6:]}", out, grads, ref_out, ref_grads, near, c["K"])


@gpu
def test_null_phase_gradient():
    """No upstream gradient for the phases (they never reach the Fourier renderer's image): the phase channels of g_raw are
    zero, everything else is what it is with the gradient present."""
    dev = _dev()
    args, ups = _random_case(Bn=2, P=55, KF=2, K=2, C=19, pose=True, mod=True, edge=True, seed=731)
    near, _ = _near_boundary(args)
    out, grads = _hip_head(args, ups, dev, skip_grad=("phases",))
    ref_out, ref_grads = _checker(args, ups, torch.float64, skip_grad=("phases",))
    assert not grads["raw"][..., 16:19].any()
    _compare("null phase gradient", out, grads, ref_out, ref_grads, near, 2)
    # only the phases flow: every other upstream gradient is null
    only = ("positions", "scales", "rotations", "colors", "opacities")
    out, grads = _hip_head(args, ups, dev, skip_grad=only)
    ref_out, ref_grads = _checker(args, ups, torch.float64, skip_grad=only)
    assert not grads["raw"][..., :16].any() and grads["raw"][..., 16:19].any()
    assert rel_to_max(grads["raw"].numpy(), ref_grads["raw"].numpy()) <= TOL
    assert not grads["base_z"].any() and not grads["edge"].any() and not grads["opacity_mod"].any()


@gpu
def test_degenerate_rows_stay_finite():
    dev = _dev()
    args, ups = _random_case(Bn=1, P=8, KF=1, K=1, C=19, pose=True, mod=True, edge=True, seed=741)
    raw = args["raw"]
    raw[0, 0, 0, 6:9] = 0.0                                   # a1 = 0
    raw[0, 1, 0, 9:12] = raw[0, 1, 0, 6:9] * -2.5             # a2 parallel to a1
    raw[0, 2, 0, 9:12] = 0.0                                  # a2 = 0
    raw[0, 3, 0, 6:12] = 0.0                                  # both
    raw[0, 4, 0, 3:6] = 30.0
    raw[0, 5, 0, 3:6] = -30.0
    raw[0, 6, 0, 15] = 10.0                                   # opacity near 1 ...
    args["opacity_mod"] = torch.full((1,), 1.5)               # ... times 1.5: clamped
    out, grads = _hip_head(args, ups, dev)
    for k, v in list(out.items()) + list(grads.items()):
        assert bool(torch.isfinite(v).all()), k
    assert float((out["rotations"].norm(dim=-1) - 1).abs().max()) <= 1e-5
    assert float(out["opacities"][0, 6]) == 1.0 and float(grads["raw"][0, 6, 0, 15]) == 0.0
    assert torch.allclose(out["scales"][0, 4] / (1 - 0.5 * args["edge"][0, 4]), torch.full((3,), 2.0))
    assert not grads["raw"][0, 4:6, 0, 3:6].any()              # outside the clamps: no gradient


@gpu
def test_two_calls_are_bit_identical():
    dev = _dev()
    args, ups = _random_case(Bn=3, P=377, KF=4, K=3, C=19, pose=True, mod=True, edge=True, seed=751)
    a_out, a_grads = _hip_head(args, ups, dev)
    b_out, b_grads = _hip_head(args, ups, dev)
    for k in a_out:
        assert torch.equal(a_out[k].view(torch.int32), b_out[k].view(torch.int32)), k
    for k in a_grads:
        assert torch.equal(a_grads[k].view(torch.int32), b_grads[k].view(torch.int32)), k


def test_entry_points_validate_arguments():
    """Host-side argument checks: no kernel is launched, so this one runs without a GPU too."""
    import ctypes
    from fresnel_amd import _binding as B
    lib = B.load()
    nb = ctypes.c_size_t(0)
    good = B.FgsHeadDims(2, 35, 3, 2, 16, 0.25, 0.5, 0.2)
    assert lib.fgs_head_workspace_bytes(ctypes.byref(good), ctypes.byref(nb)) == 0 and nb.value >= 2 * 4
    for bad in (B.FgsHeadDims(2, 35, 3, 4, 16, 0.25, 0.5, 0.2), B.FgsHeadDims(2, 35, 3, 2, 17, 0.25, 0.5, 0.2),
                B.FgsHeadDims(0, 35, 3, 2, 16, 0.25, 0.5, 0.2)):
        assert lib.fgs_head_workspace_bytes(ctypes.byref(bad), ctypes.byref(nb)) == -1
    assert lib.fgs_head_workspace_bytes(ctypes.byref(B.FgsHeadDims(2, 35, 65, 2, 16, 0.25, 0.5, 0.2)), ctypes.byref(nb)) == -3
    assert lib.fgs_head_forward(ctypes.byref(good), *([None] * 13)) == -1
    assert lib.fgs_head_backward(ctypes.byref(good), *([None] * 16)) == -1


# ---- hand-off and the training step ---------------------------------------------------------------------------------------------
@gpu
def test_mirrors_hand_their_outputs_to_the_renderers_without_a_copy():
    from fresnel_amd.decoder import DirectPatchDecoder, FibonacciPatchDecoder
    from fresnel_amd.renderer import Camera, FourierGaussianRenderer, TileBasedRenderer
    dev = _dev()
    torch.manual_seed(3)
    cam = Camera(fx=64 * 0.8, fy=64 * 0.8, cx=32, cy=32, width=64, height=64)
    feats, depth = torch.randn(2, 16, 6, 6, device=dev) * 0.5, torch.rand(2, 1, 32, 32, device=dev)
    cases = ((DirectPatchDecoder(16, 2, [32], head_backend="hip"), TileBasedRenderer(64, 64), False),
             (FibonacciPatchDecoder(16, 55, 1, [32], use_phase_output=True, head_backend="hip"),
              FourierGaussianRenderer(64, 64, wavelength_r=0.65, wavelength_g=0.55, wavelength_b=0.45), True))
    for model, ren, with_phases in cases:
        model, ren = model.to(dev).train(), ren.to(dev)
        out = model(feats, depth)
        for k in hc.OUTPUTS[:5] + (("phases",) if with_phases else ()):
            t = out[k]
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), k
            assert t.detach().contiguous().float().data_ptr() == t.data_ptr(), k   # what the renderer's wrapper takes: the same memory
        img = ren(out["positions"], out["scales"], out["rotations"], out["colors"], out["opacities"], cam,
                  phases=out.get("phases") if with_phases else None)
        assert img.shape == (2, 3, 64, 64) and bool(torch.isfinite(img).all())
        (img * torch.linspace(0, 1, 64, device=dev)).sum().backward()
        g = model.mlp.net[0].weight.grad
        assert g is not None and bool(torch.isfinite(g).all()) and bool(g.any()), type(model).__name__


@gpu
def test_one_captured_training_step_of_experiment_4():
    """--experiment 4 --use_phase_blending --head_backend hip on synthetic data at 64 x 64: the step captured in a HIP graph.  The
    first replay repeats the eager step of an identical model on the same batch: the same kernels in the same order, so the
    figures are expected equal to the bit; the bound leaves room for a library choosing another algorithm under capture
    (fp32 rounding of sums: 1e-6 relative on the loss, 1e-5 relative / 1e-7 absolute on the parameters)."""
    import copy
    from fresnel_amd import train
    from fresnel_amd.dist import DPContext
    from fresnel_amd.renderer import FourierGaussianRenderer
    dev = _dev()
    a = train.arg_parser().parse_args(["--experiment", "4", "--use_phase_blending", "--head_backend", "hip", "--hip_graph",
                                       "--image_size", "64", "--batch_size", "2", "--n_spiral_points", "55", "--lr", "2e-3"])
    cfg = train.config_from_args(a)
    cfg.device, cfg.feature_size, cfg.feature_dim = "cuda:0", 6, 16
    torch.manual_seed(0)
    eager = train.make_decoder(cfg).to(dev).train()
    for m in eager.modules():   # dropout draws differ between two runs: off, the step is then a function of the batch alone
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    twin = copy.deepcopy(eager)
    renderer, camera = train.default_renderer_factory(cfg, dev, 64)
    assert isinstance(renderer, FourierGaussianRenderer)
    dp = DPContext(device=dev)
    batch = train.SyntheticDataset(4, cfg).batch([0, 1], dev)
    res = train.train_step(eager, renderer, camera, batch, train.make_optimizer(eager, cfg), cfg, dp)
    want = res.to_host()
    assert want is not None and math.isfinite(want["total"])
    graphed = train.GraphedTrainStep(twin, renderer, camera, train.make_optimizer(twin, cfg), cfg, dp, batch)
    got = graphed(batch).to_host()
    assert got is not None and math.isfinite(got["total"])
    print(f"eager loss {want['total']:.9f}, first replay {got['total']:.9f}")
    assert abs(got["total"] - want["total"]) <= 1e-6 * abs(want["total"])
    moved = 0.0
    for (k, p), q in zip(eager.named_parameters(), twin.parameters()):
        assert torch.allclose(q, p, rtol=1e-5, atol=1e-7), k
        moved = max(moved, float((p - q).detach().abs().max()))
    print(f"largest parameter difference eager / replay: {moved:.2e}")
    assert eager.mlp.net[0].weight.grad is not None
