"""PhysicsDirectPatchDecoder / PhysicsFresnelZones / physics_head (torch backend) against the reference's fixtures P1-P3
(tests/golden/make_goldens_physics.py), the restated head (tests/physics_checker.py) against the same fixtures with one rule
changed at a time, and the training script's new decoder choice and flags.  CPU only.

Judging (the project's rule): a tensor passes within 1e-4 of its maximum of the reference's fp32 OR fp64 result, else within twice
the reference's own fp32-to-fp64 deviation of its fp64 result.  Phases are judged by circular distance and by the second form
alone.  grad.sd.depth_offset is the sum of dL/d base_z, whose phase part cancels: judged at 1e-4 of sum |dL/d base_z|."""
import json
import math
import os

import numpy as np
import pytest
import torch

import physics_checker as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("P1_physics_ties", "P2_physics_nodepth", "P3_physics_grid37")
TOL = 1e-4
_CACHE = {}


def fixture(name):
    if name not in _CACHE:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
            _CACHE[name] = {k: z[k] for k in z.files}
    return _CACHE[name]


def build_mirror(fx, head_backend="torch", device="cpu"):
    from fresnel_amd.decoder import PhysicsDirectPatchDecoder
    model = PhysicsDirectPatchDecoder(**json.loads(str(fx["ctor"])), head_backend=head_backend).eval()
    sd = {k[3:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("sd.")}
    model.load_state_dict(sd, strict=True)
    return model.to(device)


def fixture_upstream(fx, name, shape):
    return torch.from_numpy(fx["g." + name]) if "g." + name in fx else pc.formula_upstream(shape, pc.OUTPUTS.index(name))


def run_mirror(model, fx, device="cpu"):
    """-> outputs, parameter gradients, dL/d raw (B, P, K_full, 16); all on the CPU"""
    captured = {}

    def hook(_m, _i, out):
        out.retain_grad()
        captured["raw"] = out

    h = model.mlp.register_forward_hook(hook)
    ng = int(fx["num_gaussians"])
    depth = torch.from_numpy(fx["in.depth"]).to(device) if "in.depth" in fx else None
    feats = torch.from_numpy(fx["in.features"]).to(device)
    out = model(feats, depth, num_gaussians=None if ng < 0 else ng)
    sum((out[k] * fixture_upstream(fx, k, out[k].shape).to(device)).sum() for k in out).backward()
    h.remove()
    Bn, _, H, W = feats.shape
    grads = {k: (p.grad.cpu() if p.grad is not None else torch.zeros(p.shape)) for k, p in model.named_parameters()}
    return ({k: v.detach().cpu() for k, v in out.items()}, grads,
            captured["raw"].grad.reshape(Bn, H * W, model.gaussians_per_patch, 16).cpu())


def judge(tag, got, fx, key, scale=None):
    """The project's rule for one entry of a fixture; `scale` replaces the tensor's own maximum."""
    a = np.asarray(got, dtype=np.float64)
    r32, r64, dev = fx[key].astype(np.float64), fx["f64." + key], float(fx["dev." + key])
    if "phases" in key:
        d = float(pc.circular_distance(torch.from_numpy(a), torch.from_numpy(r64)).max())
        print(f"{tag}: {key} circular {d:.2e} (allowed {2 * dev:.2e})")
        assert d <= 2 * dev, f"{tag}: {key} is {d:.2e} from the fp64 phases on the circle, the reference's fp32 run {dev:.2e}"
        return
    top = scale if scale is not None else max(float(np.abs(r64).max()), 1e-30)
    e32, e64 = float(np.abs(a - r32).max()), float(np.abs(a - r64).max())
    print(f"{tag}: {key} {e32 / top:.2e} / {e64 / top:.2e} of {top:.3e} (fp32 / fp64), referee {dev / top:.2e}")
    assert min(e32, e64) <= TOL * top or e64 <= 2 * dev, \
        f"{tag}: {key} is {e32:.3e} / {e64:.3e} from the reference's fp32 / fp64 result (scale {top:.3e}, its own deviation {dev:.3e})"


def assert_matches_fixture(fx, out, grads, g_raw, tag):
    K = out["phases"].shape[1] // (fx["in.features"].shape[2] * fx["in.features"].shape[3])
    patches = torch.from_numpy(fx["patches"].astype(np.int64))
    gauss = (patches[:, None] * K + torch.arange(K)[None, :]).flatten()
    for k in pc.OUTPUTS:
        judge(tag, out[k][:, gauss].numpy(), fx, "out." + k)
    judge(tag, out["phases"].numpy(), fx, "out.phases_full")
    judge(tag, g_raw[:, patches].numpy(), fx, "grad.raw")
    for k, g in grads.items():
        judge(tag, g.numpy(), fx, "grad.sd." + k, scale=float(fx["sum_abs_g_base_z"]) if k == "depth_offset" and "in.depth" in fx else None)


# ---- the mirror on the fixtures ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_reference_state_dict_loads_strictly_and_reproduces_the_fixture(name):
    fx = fixture(name)
    model = build_mirror(fx)
    ctor = json.loads(str(fx["ctor"]))
    assert [k for k in model.state_dict()] == [k[3:] for k in fx if k.startswith("sd.")]   # the reference's keys in its order
    assert isinstance(model.fresnel_zones._wavelength_raw, torch.nn.Parameter) == ctor.get("learnable_wavelength", True)
    assert ("diffraction._C_lut" in model.state_dict()) == ctor.get("use_diffraction_placement", False)
    out, grads, g_raw = run_mirror(model, fx)
    assert out["phases"].dim() == 2 and float(out["phases"].min()) >= 0 and float(out["phases"].max()) <= 2 * math.pi
    assert_matches_fixture(fx, out, grads, g_raw, name)


def test_parameter_order_is_the_references():
    from fresnel_amd.decoder import PhysicsDirectPatchDecoder
    names = [k for k, _ in PhysicsDirectPatchDecoder(8, 2, [4], use_diffraction_placement=True).named_parameters()]
    assert names == ["depth_offset", "mlp.net.0.weight", "mlp.net.0.bias", "mlp.net.3.weight", "mlp.net.3.bias",
                     "fresnel_zones._wavelength_raw"]


def test_own_fresnel_integral_tables_equal_the_references():
    from fresnel_amd.decoder import PhysicsDirectPatchDecoder
    fx = fixture("P3_physics_grid37")
    sd = PhysicsDirectPatchDecoder(**json.loads(str(fx["ctor"]))).state_dict()
    for k in ("_w_lut", "_C_lut", "_S_lut"):
        assert sd["diffraction." + k].shape == (1000,)
        assert float((sd["diffraction." + k] - torch.from_numpy(fx["sd.diffraction." + k])).abs().max()) <= 1e-5


def test_no_depth_gives_one_phase_and_no_gradient_to_the_offset():
    fx = fixture("P2_physics_nodepth")
    model = build_mirror(fx)
    out, grads, _ = run_mirror(model, fx)
    assert float(out["phases"].max()) == float(out["phases"].min())
    lam = abs(float(fx["sd.fresnel_zones._wavelength_raw"]))
    want = torch.tensor((2 * math.pi / lam * 0.5) % (2 * math.pi))   # u = 0, |u - 0.5| = 0.5: 10 turns at 0.05, on the wrap point
    assert float(pc.circular_distance(out["phases"][0, 0], want)) <= 1e-4
    assert not grads["depth_offset"].any()


# ---- the checker, and what one changed rule does to it -------------------------------------------------------------------------------
def _checker_on_fixture(fx, dtype, **rules):
    """physics_checker.head on P1's stored raw -> phases, dL/d base_z, dL/d wavelength_raw"""
    sd = lambda k: torch.from_numpy(fx["sd." + k])   # noqa: E731
    feats, depth = torch.from_numpy(fx["in.features"]), torch.from_numpy(fx["in.depth"])
    Bn, _, H, W = feats.shape
    dg = torch.nn.functional.interpolate(depth, (H, W), mode="bilinear", align_corners=False).reshape(Bn, H * W)
    base_z = (sd("depth_offset") + dg * (-2)).to(dtype).requires_grad_(True)
    lam = sd("fresnel_zones._wavelength_raw").to(dtype).requires_grad_(True)
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    out = pc.head(torch.from_numpy(fx["raw"]).to(dtype), torch.stack([xs, ys], -1).reshape(H * W, 2), base_z, lam,
                  num_gaussians=int(fx["num_gaussians"]), **rules)
    (out["phases"] * torch.from_numpy(fx["g.phases"]).to(dtype)).sum().backward()
    return out, base_z.grad, lam.grad


def test_checker_reproduces_p1_in_both_precisions():
    fx = fixture("P1_physics_ties")
    for dtype, pre in ((torch.float32, ""), (torch.float64, "f64.")):
        out, _, _ = _checker_on_fixture(fx, dtype)
        for k in pc.OUTPUTS:
            want = torch.from_numpy(fx[pre + "out." + k])
            if k == "phases":
                assert float(pc.circular_distance(out[k].detach(), want).max()) <= 2 * float(fx["dev.out.phases"])
            else:
                assert float((out[k].detach().double() - want.double()).abs().max()) <= TOL * float(want.abs().max()), (dtype, k)


def test_ties_are_real_and_the_first_only_rule_misses_by_ten_tolerances():
    """P1's minimum and maximum are each held by several patches.  With the right rule the checker's dL/d base_z sums to the
    fixture's dL/d depth_offset part; giving the whole share to the first tied element moves dL/d base_z by far more than 10 x 1e-4
    of its maximum."""
    fx = fixture("P1_physics_ties")
    _, gz, _ = _checker_on_fixture(fx, torch.float64)
    _, gz_first, _ = _checker_on_fixture(fx, torch.float64, tie_rule="first")
    bz = _checker_on_fixture(fx, torch.float64)[0]["positions"][..., 2]
    assert int((bz == bz.min()).sum()) >= 4 and int((bz == bz.max()).sum()) >= 4
    miss = float((gz - gz_first).abs().max()) / float(gz.abs().max())
    print(f"first-only tie rule: dL/d base_z moves by {miss:.2e} of its maximum")
    assert miss >= 10 * TOL
    # both rules hand out the same total
    assert abs(float(gz.sum() - gz_first.sum())) <= 1e-9 * float(gz.abs().sum())


def test_unwrapped_phase_matches_only_on_the_circle():
    fx = fixture("P1_physics_ties")
    wrapped = _checker_on_fixture(fx, torch.float64)[0]["phases"].detach()
    plain = _checker_on_fixture(fx, torch.float64, wrap_rule="none")[0]["phases"].detach()
    assert float(pc.circular_distance(wrapped, plain).max()) <= 1e-9
    assert float((wrapped - plain).abs().max()) >= 2 * math.pi - 1e-9 >= 10 * 2 * float(fx["dev.out.phases"])
    # and the plain difference of the reference's own two precisions is a whole turn somewhere, or small everywhere: the circular one is small
    assert float(fx["dev.out.phases_full"]) < 1e-3


def test_wavelength_gradient_of_the_checker_is_the_fixtures():
    fx = fixture("P1_physics_ties")
    feats = fx["in.features"]
    _, _, g_lam = _checker_on_fixture(fx, torch.float64)
    # the fixture's gradient holds the phase part alone too: no other output depends on the wavelength
    want = float(fx["f64.grad.sd.fresnel_zones._wavelength_raw"])
    assert abs(float(g_lam) - want) <= TOL * abs(want), (float(g_lam), want, feats.shape)


# ---- PhysicsFresnelZones ------------------------------------------------------------------------------------------------------------
def test_fresnel_zone_methods():
    from fresnel_amd.decoder import PhysicsFresnelZones
    fz = PhysicsFresnelZones(num_zones=4, wavelength=0.08, focal_depth=0.5)
    assert isinstance(fz._wavelength_raw, torch.nn.Parameter) and abs(float(fz.wavelength) - 0.08) < 1e-8
    b = fz.compute_zone_boundaries()
    want = torch.sqrt(torch.arange(5.0) / 4)    # sqrt(n lambda f) / sqrt(4 lambda f)
    assert b.shape == (5,) and float((b - want).abs().max()) <= 1e-6
    depth = torch.tensor([0.0, 0.4, 0.5, 0.6, 0.75, 0.9, 1.0])
    assert fz.get_zone_index(depth).tolist() == [0, 0, 0, 1, 2, 3, 3]     # boundaries 0.5, 0.7071, 0.8660
    assert torch.allclose(fz.get_zone_phase(torch.tensor([0, 1, 2, 3])), torch.tensor([0.0, math.pi, 0.0, math.pi]))
    assert torch.allclose(fz.compute_path_difference(depth), (depth - 0.5).abs())
    assert torch.allclose(fz.depth_to_phase(depth), 2 * math.pi / 0.08 * (depth - 0.5).abs(), rtol=1e-6)
    assert torch.equal(fz(depth), fz.depth_to_phase(depth))
    allv = fz(depth, return_all=True)
    assert sorted(allv) == ["boundaries", "path_difference", "phase", "wavelength", "zone_idx", "zone_phase"]
    for raw, lam in ((0.005, 0.01), (-0.2, 0.2), (3.0, 0.5)):   # the clamp, and the sign
        assert abs(float(PhysicsFresnelZones(wavelength=raw).wavelength) - lam) < 1e-8
    fixed = PhysicsFresnelZones(learnable_wavelength=False)
    assert not list(fixed.parameters()) and list(fixed.state_dict()) == ["_wavelength_raw"]
    assert "learnable=False" in repr(fixed)


# ---- physics_head's argument checks ---------------------------------------------------------------------------------------------------
def test_physics_head_checks_its_arguments():
    from fresnel_amd import _binding as B
    from fresnel_amd.decoder import physics_head
    raw, xy, z, lam = torch.zeros(1, 4, 2, 16), torch.zeros(4, 2), torch.zeros(1, 4), torch.tensor(0.05)
    assert physics_head(raw, xy, z, lam, num_gaussians=1)["phases"].shape == (1, 4)
    for bad in (dict(raw=torch.zeros(1, 4, 2, 19)), dict(base_xy=torch.zeros(3, 2)), dict(base_z=torch.zeros(2, 4)),
                dict(wavelength_raw=torch.zeros(2)), dict(backend="triton")):
        kw = dict(raw=raw, base_xy=xy, base_z=z, wavelength_raw=lam)
        backend = bad.pop("backend", "torch")
        kw.update(bad)
        with pytest.raises(ValueError):
            physics_head(kw["raw"], kw["base_xy"], kw["base_z"], kw["wavelength_raw"], backend=backend)
    with pytest.raises(B.FgsError, match="no CPU fallback"):
        physics_head(raw, xy, z, lam, backend="hip")


# ---- the training script ----------------------------------------------------------------------------------------------------------------
def _cfg(argv):
    from fresnel_amd import train
    return train.config_from_args(train.arg_parser().parse_args(argv))


def test_flags_and_defaults_are_the_references():
    from fresnel_amd import train
    from fresnel_amd.decoder import PatchGaussianDecoder, PhysicsDirectPatchDecoder
    assert "physics" in train.DECODERS
    c = _cfg([])
    assert (c.decoder, c.learnable_wavelength, c.focal_depth, c.use_physics_zones, c.use_diffraction_placement) == \
        ("standin", False, 0.5, False, False)
    # no flag switches the decoder by itself
    for flags in (["--use_wave_rendering"], ["--use_physics_zones"], ["--use_diffraction_placement"], ["--learnable_wavelength"]):
        assert _cfg(flags).decoder == "standin" and isinstance(train.make_decoder(_cfg(flags)), PatchGaussianDecoder)
    c = _cfg(["--decoder", "physics", "--use_wave_rendering", "--learnable_wavelength", "--wavelength", "0.08", "--focal_depth", "0.25",
              "--use_diffraction_placement", "--gaussians_per_patch", "3", "--head_backend", "hip"])
    m = train.make_decoder(c)
    assert isinstance(m, PhysicsDirectPatchDecoder) and m.head_backend == "hip" and m.gaussians_per_patch == 3
    assert isinstance(m.fresnel_zones._wavelength_raw, torch.nn.Parameter) and abs(float(m.fresnel_zones._wavelength_raw) - 0.08) < 1e-8
    assert m.fresnel_zones.focal_depth == 0.25 and "diffraction._S_lut" in m.state_dict()
    m = train.make_decoder(_cfg(["--decoder", "physics", "--learnable_wavelength", "--no_learnable_wavelength"]))
    assert not isinstance(m.fresnel_zones._wavelength_raw, torch.nn.Parameter) and m.diffraction is None
    with pytest.raises(SystemExit):
        _cfg(["--decoder", "physics", "--experiment", "4"])


def test_pose_encoding_is_refused():
    from fresnel_amd import train
    with pytest.raises(ValueError, match="use_pose_encoding"):
        train.make_decoder(_cfg(["--decoder", "physics", "--use_pose_encoding"]))


def test_forward_keeps_the_references_signature():
    import inspect
    from fresnel_amd.decoder import PhysicsDirectPatchDecoder
    assert list(inspect.signature(PhysicsDirectPatchDecoder.forward).parameters) == ["self", "features", "depth", "image_size", "num_gaussians"]
    with pytest.raises(TypeError):
        PhysicsDirectPatchDecoder(8, 1, [4])(torch.zeros(1, 8, 2, 2), None, elevation=torch.zeros(1), azimuth=torch.zeros(1))
