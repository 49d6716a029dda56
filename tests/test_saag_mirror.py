"""The SAAG refinement decoder (--experiment 1) on the CPU: the mirror with the torch backend and the restated stages
(tests/saag_checker.py) against the reference's fixtures R1-R3 under the 1e-4-of-maximum rule, checkpoint keys, argument and flag
checks, the residual term of the loss, the batch rule, host-side validation of the C entries, and self-tests showing that the seam
inputs of the GPU tests (tests/test_hip_saag.py imports them from here) tell the checker's rules apart."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import saag_checker as sc
from helpers import GOLDEN, rel_to_max

FIXTURES = ["R1_saag_mixed", "R2_saag_dummy37", "R3_saag_odd"]
CLOUD = ("positions", "scales", "rotations", "colors", "opacities")
GAINS = ("pos_scale", "scale_scale", "color_scale", "opacity_scale")
TOL = 1e-4


def fixture(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def build_mirror(fx, backend="torch", device="cpu"):
    from fresnel_amd.decoder import SAAGRefinementNet
    model = SAAGRefinementNet(**json.loads(str(fx["ctor"])), backend=backend)
    sd = {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sd.")}
    model.load_state_dict(sd, strict=True)
    return model.to(device).eval(), sd


def fixture_cloud(fx, device="cpu"):
    return [torch.from_numpy(fx["in.saag_" + k]).to(device) for k in CLOUD]


def fixture_gains(fx, device="cpu", dtype=torch.float32):
    return torch.tensor([float(fx["sd." + k]) for k in GAINS], dtype=dtype, device=device)


def run_mirror(model, fx, device="cpu"):
    """-> outputs, parameter gradients, raw gradient (all CPU) of sum_k sum(out[k] g[k])"""
    captured = {}

    def hook(_m, _i, out):
        out.retain_grad()
        captured["raw"] = out

    h = model.mlp.register_forward_hook(hook)
    model.zero_grad(set_to_none=True)
    out = model(torch.from_numpy(fx["in.features"]).to(device), *fixture_cloud(fx, device))
    sum((out[k] * torch.from_numpy(fx["g." + k]).to(device)).sum() for k in out).backward()
    h.remove()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).cpu() for k, p in model.named_parameters()}
    return {k: v.detach().cpu() for k, v in out.items()}, grads, captured["raw"].grad.cpu().reshape(fx["raw"].shape)


def assert_matches_fixture(fx, out, grads, g_raw, what):
    assert sorted(out) == sorted(sc.OUTPUTS)
    for k, v in out.items():
        e = rel_to_max(v.numpy(), fx["out." + k])
        assert v.shape == fx["out." + k].shape and e <= TOL, f"{what}: {k} is {e:.2e} of its maximum away from the reference"
    e = rel_to_max(g_raw.numpy(), fx["grad.raw"])
    assert e <= TOL, f"{what}: the raw gradient is {e:.2e} of its maximum away"
    for k, g in grads.items():
        e = rel_to_max(g.numpy(), fx["grad.sd." + k])
        assert e <= TOL, f"{what}: the gradient of {k} is {e:.2e} of its maximum away"


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_mirror_torch_backend_reproduces_the_reference(name):
    fx = fixture(name)
    model, sd = build_mirror(fx)
    assert sorted(sd) == sorted(["mlp.net.%d.%s" % (i, w) for i in (0, 3, 6) for w in ("weight", "bias")] + list(GAINS))
    assert list(model.state_dict()) == [k[3:] for k in fx.files if k.startswith("sd.")]   # and in the reference's order
    out, grads, g_raw = run_mirror(model, fx)
    assert_matches_fixture(fx, out, grads, g_raw, name)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", FIXTURES)
def test_checker_reproduces_the_reference(name, dtype):
    fx = fixture(name)
    model, _ = build_mirror(fx)
    cloud = fixture_cloud(fx)
    # stage 1: the restated gather feeds the reference's MLP weights; the raw output must be the fixture's
    inputs = sc.mlp_inputs(torch.from_numpy(fx["in.features"]), *cloud, dtype=dtype)
    with torch.no_grad():
        raw = model.to(dtype).mlp(inputs)
    e = rel_to_max(raw.numpy(), fx["raw"])
    assert e <= TOL, f"{name}: the MLP behind the restated inputs is {e:.2e} of its maximum away from the reference's raw output"
    # stage 2 from the fixture's raw
    raw = torch.from_numpy(fx["raw"]).to(dtype).requires_grad_(True)
    gains = fixture_gains(fx, dtype=dtype).requires_grad_(True)
    out = sc.refine(raw, *cloud, gains, residual_scale=model.residual_scale)
    sum((out[k] * torch.from_numpy(fx["g." + k]).to(dtype)).sum() for k in out).backward()
    for k, v in out.items():
        e = rel_to_max(v.detach().numpy(), fx["out." + k])
        assert e <= TOL, f"{name}: checker {k} is {e:.2e} of its maximum away"
    assert rel_to_max(raw.grad.numpy(), fx["grad.raw"]) <= TOL
    for i, k in enumerate(GAINS):
        assert abs(float(gains.grad[i]) - float(fx["grad.sd." + k])) <= TOL * max(abs(float(fx["grad.sd." + k])), 1e-30), k


def test_fixtures_hold_what_they_promise():
    r1, r2 = fixture("R1_saag_mixed"), fixture("R2_saag_dummy37")
    z = r1["in.saag_positions"][..., 2]
    assert (z < 0.1).any() and (z > 0.1).any() and (z == np.float32(0.1)).any()
    assert np.abs(np.linalg.norm(r1["in.saag_rotations"], axis=-1) - 1).max() > 0.1
    for k in ("colors", "opacities"):
        assert (r1["in.saag_" + k] == 0).any() and (r1["in.saag_" + k] == 1).any()
    ix, iy = sc.sample_coords(torch.from_numpy(r2["in.saag_positions"]).double(), 37, 37)
    share = float(((ix == 0) | (ix == 36)).double().mean() + ((iy == 0) | (iy == 36)).double().mean()) / 2
    assert share > 0.5, share   # the dummy cloud's z is about -2: x / 0.1 leaves [-2, 2] for most Gaussians
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 300 * 1024


# ---- arguments and flags ------------------------------------------------------------------------------------------------------------
def _small_cloud(Bn=2, N=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(Bn, N, 3, generator=g), torch.rand(Bn, N, 3, generator=g), torch.randn(Bn, N, 4, generator=g),
            torch.rand(Bn, N, 3, generator=g), torch.rand(Bn, N, generator=g)]


def test_arguments_are_checked_and_hip_refuses_cpu_tensors():
    from fresnel_amd import _binding as B
    from fresnel_amd.decoder import SAAGRefinementNet, saag_mlp_inputs, saag_refine_head
    cloud = _small_cloud()
    feats, raw, gains = torch.randn(2, 4, 3, 3), torch.randn(2, 5, 16), torch.tensor([0.05, 0.1, 0.1, 0.1])
    assert saag_mlp_inputs(feats, *cloud).shape == (2, 5, 18)
    assert sorted(saag_refine_head(raw, *cloud, gains)) == sorted(sc.OUTPUTS)
    with pytest.raises(ValueError):
        saag_mlp_inputs(feats, *cloud, backend="triton")
    with pytest.raises(ValueError):
        saag_refine_head(raw, *cloud, gains, backend="eager")
    with pytest.raises(ValueError):
        SAAGRefinementNet(backend="cuda")
    with pytest.raises(ValueError):
        saag_mlp_inputs(feats[0], *cloud)
    with pytest.raises(ValueError):
        saag_mlp_inputs(feats, cloud[0], cloud[1][:, :4], *cloud[2:])
    with pytest.raises(ValueError):
        saag_refine_head(raw[..., :15], *cloud, gains)
    with pytest.raises(ValueError):
        saag_refine_head(raw, *cloud, gains[:3])
    with pytest.raises(B.FgsError):
        saag_mlp_inputs(feats, *cloud, backend="hip")
    with pytest.raises(B.FgsError):
        saag_refine_head(raw, *cloud, gains, backend="hip")


def test_train_cli_selects_the_saag_decoder():
    from fresnel_amd import train
    from fresnel_amd.decoder import SAAGRefinementNet
    ap = train.arg_parser()
    cfg = train.config_from_args(ap.parse_args(["--experiment", "1"]))
    assert cfg.decoder == "saag" and cfg.saag_backend == "torch" and cfg.residual_weight == 0.01
    cfg = train.config_from_args(ap.parse_args(["--experiment", "1", "--saag_backend", "hip", "--residual_weight", "0.5"]))
    assert cfg.saag_backend == "hip" and cfg.residual_weight == 0.5
    model = train.make_decoder(cfg)
    assert isinstance(model, SAAGRefinementNet) and model.backend == "hip" and model.mlp.net[0].in_features == 398
    for argv in (["--experiment", "1", "--decoder", "direct"], ["--experiment", "1", "--decoder", "nca"],
                 ["--experiment", "2", "--decoder", "saag"], ["--experiment", "5", "--decoder", "saag"],
                 ["--experiment", "1", "--hip_graph"], ["--experiment", "3"]):
        with pytest.raises(SystemExit):
            train.config_from_args(ap.parse_args(argv))
    with pytest.raises(SystemExit):
        ap.parse_args(["--experiment", "1", "--saag_backend", "triton"])
    assert train.config_from_args(ap.parse_args(["--experiment", "2"])).decoder == "standin"
    cfg = train.config_from_args(ap.parse_args(["--experiment", "1", "--saag_backend", "hip"]))
    cfg.device = "cpu"
    with pytest.raises(ValueError, match="saag_backend"):
        train.run_training(cfg)


def test_residual_term_of_the_loss():
    from fresnel_amd import train
    cfg = train.TrainingConfig(ssim_weight=0.0, residual_weight=0.3)
    g = torch.Generator().manual_seed(5)
    rendered, target = torch.rand(2, 3, 8, 8, generator=g).requires_grad_(True), torch.rand(2, 3, 8, 8, generator=g)
    res = {k: torch.randn(2, 7, 1 if k == "opacity_delta" else 3, generator=g).requires_grad_(True) for k in train.RESIDUAL_KEYS}
    base, base_terms = train.compute_losses(rendered, target, None, None, cfg)
    total, terms = train.compute_losses(rendered, target, None, None, cfg, residuals=res)
    reg = sum(res[k].abs().mean() for k in ("pos_delta", "scale_delta", "color_delta", "opacity_delta"))   # TGD:934-937
    assert "residual" not in base_terms and torch.equal(terms["residual"], reg.detach())
    assert torch.allclose(total, base + 0.3 * reg, rtol=1e-6, atol=0)
    total.backward()
    assert torch.allclose(res["opacity_delta"].grad, 0.3 * torch.sign(res["opacity_delta"].detach()) / 14, rtol=1e-6, atol=0)


# ---- the batch rule ---------------------------------------------------------------------------------------------------------------
def _write_dataset(root, counts, S=16, C=384):
    """Images img0.png ... with feature caches; counts[i] = size of image i's SAAG cloud, None: no `_saag.bin`."""
    from PIL import Image
    from fresnel_amd import io as fio
    os.makedirs(root / "features")   # (creates `root` as well)
    rng = np.random.RandomState(3)
    for i, n in enumerate(counts):
        Image.fromarray(rng.randint(0, 255, (S, S, 3), dtype=np.uint8)).save(root / f"img{i}.png")
        rng.randn(37, 37, C).astype(np.float32).tofile(root / "features" / f"img{i}_dinov2.bin")
        if n is not None:
            g = torch.Generator().manual_seed(40 + i)
            fio.save_gaussians_to_binary(str(root / "features" / f"img{i}_saag.bin"), dict(
                positions=torch.randn(n, 3, generator=g), scales=torch.rand(n, 3, generator=g) * 0.1 + 0.01,
                rotations=torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=-1),
                colors=torch.rand(n, 3, generator=g), opacities=torch.rand(n, generator=g)))


def test_batch_gains_the_saag_cloud_only_when_every_item_has_one_of_the_same_size(tmp_path):
    from fresnel_amd import train
    from fresnel_amd.data import ImageDataset, collate_host_items
    _write_dataset(tmp_path, [12, 12, None, 9])
    plain = ImageDataset(str(tmp_path), 16)
    ds = ImageDataset(str(tmp_path), 16, load_saag=True)
    assert len(plain.host_item(0)) == 3 and len(ds.host_item(0)) == 8 and ds.host_item(2)[3].shape == (0, 3)
    assert [tuple(t.shape) for t in ds.host_item(0)[3:]] == [(12, 3), (12, 3), (12, 4), (12, 3), (12,)]
    assert torch.equal(ds.host_item(0)[3], ds[0]["saag_positions"])
    both = ds.batch([0, 1], "cpu")
    assert len(both) == 8 and both[3].shape == (2, 12, 3) and both[7].shape == (2, 12)
    assert len(ds.batch([0, 2], "cpu")) == 3      # one item without a cloud
    assert len(ds.batch([0, 3], "cpu")) == 3      # unequal counts
    assert len(ds.batch([2, 2], "cpu")) == 3      # none
    assert len(plain.batch([0, 1], "cpu")) == 3
    assert len(collate_host_items([plain.host_item(0), plain.host_item(1)])) == 3
    # the prefetcher applies the same rule
    got = [len(b) for b in train.BatchPrefetcher(ds, [[0, 1], [1, 3]], "cpu", num_workers=1)]
    assert got == [8, 3]


def test_dummy_cloud_has_the_reference_distribution():
    from fresnel_amd import train
    pos, scl, rot, col, opa = train.create_dummy_saag(3, 1000, "cpu", generator=torch.Generator().manual_seed(1))
    assert pos.shape == (3, 1000, 3) and rot.shape == (3, 1000, 4) and opa.shape == (3, 1000)
    assert abs(float(pos[..., 2].mean()) + 2) < 0.05 and abs(float(pos[..., :2].std()) - 0.5) < 0.05
    assert bool((scl == 0.05).all()) and bool((opa == 0.8).all()) and bool((rot[..., 0] == 1).all()) and not rot[..., 1:].any()
    assert 0 <= float(col.min()) and float(col.max()) < 1


# ---- the C entries, host side --------------------------------------------------------------------------------------------------------
def test_entry_points_validate_arguments_without_a_gpu():
    from fresnel_amd import _binding as B
    lib = B.load()
    nb = ctypes.c_size_t(0)

    def dims(Bn=2, N=50, C=8, H=5, W=7, strides=None, rs=0.1):
        return B.FgsSaagDims(Bn, N, C, H, W, *(strides or (C * H * W, H * W, W)), rs)

    good = dims()
    assert lib.fgs_saag_workspace_bytes(ctypes.byref(good), ctypes.byref(nb)) == 0 and nb.value >= 32 and nb.value % 256 == 0
    big = dims(N=100_000)
    assert lib.fgs_saag_workspace_bytes(ctypes.byref(big), ctypes.byref(nb)) == 0 and nb.value == 782 * 32 + (-782 * 32) % 256
    assert lib.fgs_saag_workspace_bytes(ctypes.byref(good), None) == -1
    assert lib.fgs_saag_workspace_bytes(None, ctypes.byref(nb)) == -1
    for bad in (dims(Bn=0), dims(N=0), dims(C=0), dims(H=0), dims(W=0)):
        assert lib.fgs_saag_workspace_bytes(ctypes.byref(bad), ctypes.byref(nb)) == -1
        assert lib.fgs_saag_inputs_forward(ctypes.byref(bad), *([None] * 8)) == -1
    for unsupported in (dims(Bn=65536, N=1), dims(Bn=8, N=1 << 20, C=384)):      # B > 65535;  B N (C + 14) >= 2^31
        assert lib.fgs_saag_workspace_bytes(ctypes.byref(unsupported), ctypes.byref(nb)) == -3
        assert lib.fgs_saag_refine_forward(ctypes.byref(unsupported), *([None] * 17)) == -3
    assert lib.fgs_saag_workspace_bytes(ctypes.byref(dims(Bn=8, N=32768, C=384, H=37, W=37)), ctypes.byref(nb)) == 0
    # null pointers
    assert lib.fgs_saag_inputs_forward(ctypes.byref(good), *([None] * 8)) == -1 and b"null" in lib.fgs_last_error()
    assert lib.fgs_saag_refine_forward(ctypes.byref(good), *([None] * 17)) == -1
    assert lib.fgs_saag_refine_backward(ctypes.byref(good), *([None] * 19)) == -1
    # strides that fit neither layout: rows shorter than the grid's width, overlapping planes / images
    for strides in ((8 * 35, 35, 6), (8 * 35, 34, 7), (8 * 35 - 1, 35, 7), (8 * 35, 1, 8 * 7 - 1), (5 * 56 - 1, 1, 56), (280, 0, 7)):
        assert lib.fgs_saag_inputs_forward(ctypes.byref(dims(strides=strides)), *([None] * 8)) == -1, strides
        assert b"strides" in lib.fgs_last_error()
    # channel-last strides pass the dims check and stop at the null pointers
    assert lib.fgs_saag_inputs_forward(ctypes.byref(dims(strides=(5 * 7 * 8, 1, 7 * 8))), *([None] * 8)) == -1
    assert b"null" in lib.fgs_last_error()


# ---- seam inputs of the GPU tests, and the proof that they tell the rules apart -------------------------------------------------------
SEAM_GRID = (4, 8)   # powers of two: u W - 0.5 is then EXACTLY the texel index at a texel centre, in fp32 as in fp64


def linear_features(C, H, W, Bn=1):
    """f[b, c, y, x] = a_c x + b_c y + d_c (+ b): bilinear sampling at (ix, iy) gives a_c ix + b_c iy + d_c up to rounding."""
    a = torch.arange(1, C + 1, dtype=torch.float64) * 0.5
    b = -torch.arange(1, C + 1, dtype=torch.float64) * 0.75 - 2.0
    d = torch.linspace(-1, 1, C, dtype=torch.float64)
    x, y = torch.arange(W, dtype=torch.float64), torch.arange(H, dtype=torch.float64)
    f = a.view(C, 1, 1) * x.view(1, 1, W) + b.view(C, 1, 1) * y.view(1, H, 1) + d.view(C, 1, 1)
    f = f.unsqueeze(0) + torch.arange(Bn, dtype=torch.float64).view(Bn, 1, 1, 1)
    return f.float(), (a, b, d)


def linear_answer(coef, ix, iy, Bn):
    a, b, d = coef
    return a * ix.unsqueeze(-1) + b * iy.unsqueeze(-1) + d + torch.arange(Bn, dtype=torch.float64).view(Bn, 1, 1)


def seam_positions(H, W):
    """(1, N, 3) positions: u and v exactly 0 and exactly 1, every texel centre, z exactly 0.1, one ulp either side, 0 and negative,
    and a few general points.  With z = 1: u = (x + 2) / 4, so x = 4 u - 2."""
    one = np.float32(0.1)
    pts = [(-2.0, -2.0, 1.0), (2.0, 2.0, 1.0), (-2.0, 2.0, 1.0), (2.0, -2.0, 1.0), (-5.0, 7.0, 1.0), (9.0, -3.0, 1.0)]
    for j in range(H):
        for i in range(W):
            pts.append((4.0 * (i + 0.5) / W - 2.0, 4.0 * (j + 0.5) / H - 2.0, 1.0))
    for z in (one, np.nextafter(one, np.float32(1)), np.nextafter(one, np.float32(0)), 0.0, -1.5, -0.05):
        pts += [(0.03, -0.07, float(z)), (-0.11, 0.02, float(z)), (0.19, 0.16, float(z))]
    g = torch.Generator().manual_seed(17)
    rnd = torch.cat([torch.rand(24, 2, generator=g) * 4.4 - 2.2, torch.ones(24, 1)], -1)
    return torch.cat([torch.tensor(pts, dtype=torch.float32), rnd]).unsqueeze(0)


def gate_seam_inputs():
    """raw exactly 0 in the delta channels against SAAG colours and opacities exactly 0 and 1: every clamp sits on a closed end of
    its interval.  Random rotation channels and non-unit SAAG quaternions.  -> raw, the SAAG cloud, gains"""
    N = 8
    g = torch.Generator().manual_seed(23)
    raw = torch.zeros(1, N, 16)
    raw[..., 6:12] = torch.randn(1, N, 6, generator=g)
    col, opa = torch.zeros(1, N, 3), torch.zeros(1, N)
    col[:, 1::2], opa[:, 1::2] = 1.0, 1.0
    return raw, [torch.randn(1, N, 3, generator=g), torch.rand(1, N, 3, generator=g) * 0.1 + 0.01,
                 torch.randn(1, N, 4, generator=g), col, opa], torch.tensor([0.05, 0.1, 0.1, 0.1])


def _refine_grads(raw, cloud, gains, rules=()):
    raw = raw.double().requires_grad_(True)
    gains = gains.double().requires_grad_(True)
    out = sc.refine(raw, *cloud, gains, rules=rules)
    g = torch.Generator().manual_seed(29)
    sum((v * (torch.rand(v.shape, generator=g).double() + 0.5)).sum() for v in out.values()).backward()
    return {k: v.detach() for k, v in out.items()}, raw.grad, gains.grad


@pytest.mark.parametrize("rule", ["no_half_pixel", "swap_xy", "no_border_clip"])
def test_sampling_seams_tell_the_sampling_rules_apart(rule):
    (H, W), C = SEAM_GRID, 3
    feats, coef = linear_features(C, H, W)
    pos = seam_positions(H, W)
    cloud = [pos] + _small_cloud(1, pos.shape[1])[1:]
    ix, iy = sc.sample_coords(pos.double(), H, W)
    want = linear_answer(coef, ix, iy, 1)
    right = sc.mlp_inputs(feats, *cloud)[..., :C]
    assert rel_to_max(right.numpy(), want.numpy()) <= 1e-12     # the checker's gather IS the known answer on linear features
    wrong = sc.mlp_inputs(feats, *cloud, rules=(rule,))[..., :C]
    assert rel_to_max(wrong.numpy(), want.numpy()) >= 10 * TOL, rule


def test_gate_seams_tell_closed_from_open_clamp_gates():
    raw, cloud, gains = gate_seam_inputs()
    _, g_closed, gg_closed = _refine_grads(raw, cloud, gains)
    _, g_open, gg_open = _refine_grads(raw, cloud, gains, rules=("open_gate",))
    # (the open gate loses the part that comes through the clamped tensors; the deltas' own upstream gradients remain)
    assert bool((g_closed[..., 12:16] != 0).all())
    assert rel_to_max(g_open[..., 12:16].numpy(), g_closed[..., 12:16].numpy()) >= 10 * TOL


def test_non_unit_saag_quaternions_tell_the_product_orders_apart():
    raw, cloud, gains = gate_seam_inputs()
    right, g_right, _ = _refine_grads(raw, cloud, gains)
    wrong, g_wrong, _ = _refine_grads(raw, cloud, gains, rules=("product_order",))
    assert rel_to_max(wrong["rotations"].numpy(), right["rotations"].numpy()) >= 10 * TOL
    assert rel_to_max(g_wrong[..., 6:12].numpy(), g_right[..., 6:12].numpy()) >= 10 * TOL
