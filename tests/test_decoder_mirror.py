"""The mirrors of the reference's DirectPatchDecoder / FibonacciPatchDecoder (fresnel_amd/decoder.py) and the restated head
(tests/head_checker.py) against the fixtures H1-H3 (tests/golden/make_goldens_head.py), on the CPU: strict loading of the
reference's state dict, every output and every recorded gradient within 1e-4 of the tensor's maximum, and
the training command line's decoder / renderer selection."""
import json
import os

import numpy as np
import pytest
import torch

import head_checker as hc
from helpers import GOLDEN, rel_to_max

TOL = 1e-4
FIXTURES = ["H1_head_direct_all", "H2_head_fibonacci55", "H3_head_direct_plain"]


def _path(name):
    return os.path.join(GOLDEN, name + ".npz")


def fixture(name):
    return np.load(_path(name))


def build_mirror(fx, head_backend="torch", device="cpu"):
    from fresnel_amd import decoder
    ctor = json.loads(str(fx["ctor"]))
    model = getattr(decoder, str(fx["class_name"]))(**ctor, head_backend=head_backend)
    sd = {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sd.")}
    model.load_state_dict(sd, strict=True)
    return model.eval().to(device), sd


def mirror_inputs(fx, device="cpu"):
    kw = {k[3:]: torch.from_numpy(fx[k]).to(device) for k in fx.files if k.startswith("in.") and k != "in.num_gaussians"}
    if "in.num_gaussians" in fx.files:
        kw["num_gaussians"] = int(fx["in.num_gaussians"])
    kw["features"].requires_grad_(True)
    return kw


def run_mirror(model, fx, device="cpu"):
    """-> outputs, gradients {raw, features, sd.<parameter>} of sum(out x g), like the fixture's."""
    kw = mirror_inputs(fx, device)
    captured = {}

    def hook(_m, _i, out):
        out.retain_grad()
        captured["raw"] = out

    h = model.mlp.register_forward_hook(hook)
    out = model(**kw)
    h.remove()
    model.zero_grad(set_to_none=True)
    sum((out[k] * torch.from_numpy(fx["g." + k]).to(device)).sum() for k in out).backward()
    grads = {"raw": captured["raw"].grad.reshape(fx["raw"].shape), "features": kw["features"].grad}
    for k, p in model.named_parameters():
        grads["sd." + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    return out, grads, captured["raw"].detach().reshape(fx["raw"].shape)


def assert_matches_fixture(fx, out, grads, raw, what):
    assert sorted(out) == sorted(k[4:] for k in fx.files if k.startswith("out.")), what
    assert rel_to_max(raw.cpu().numpy(), fx["raw"]) <= TOL, f"{what}: raw"
    for k, v in out.items():
        assert v.shape == fx["out." + k].shape, f"{what}: shape of {k}"
        e = rel_to_max(v.detach().cpu().numpy(), fx["out." + k])
        assert e <= TOL, f"{what}: output {k} is {e:.2e} of its maximum away"
    assert sorted(grads) == sorted(k[5:] for k in fx.files if k.startswith("grad.")), what
    for k, v in grads.items():
        e = rel_to_max(v.detach().cpu().numpy(), fx["grad." + k])
        assert e <= TOL, f"{what}: gradient {k} is {e:.2e} of its maximum away"


def head_inputs(model, fx, device="cpu"):
    """The arguments the mirror hands to gaussian_head on the fixture's inputs (its torch modules run; the head does not)."""
    from fresnel_amd import decoder
    seen = {}
    real = decoder.gaussian_head

    def spy(raw, base_xy, base_z, **kw):
        seen.update(kw, raw=raw, base_xy=base_xy, base_z=base_z)
        return real(raw, base_xy, base_z, **dict(kw, backend="torch"))

    decoder.gaussian_head = spy
    try:
        with torch.no_grad():
            model(**mirror_inputs(fx, device))
    finally:
        decoder.gaussian_head = real
    seen.pop("backend")
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in seen.items()}


@pytest.mark.parametrize("name", FIXTURES)
def test_mirror_torch_backend_reproduces_the_reference(name):
    fx = fixture(name)
    model, sd = build_mirror(fx)
    # registration order is the reference's: its optimizer state is keyed by position
    assert [k for k, _ in model.named_parameters()] == [k[8:] for k in fx.files if k.startswith("grad.sd.")]
    assert list(model.state_dict()) == list(sd)
    out, grads, raw = run_mirror(model, fx)
    assert_matches_fixture(fx, out, grads, raw, name)
    assert all(v.is_contiguous() and v.dtype == torch.float32 for v in out.values())


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_checker_reproduces_the_reference_head(name, dtype):
    fx = fixture(name)
    model, _ = build_mirror(fx)
    hin = head_inputs(model, fx)
    raw = torch.from_numpy(fx["raw"]).to(dtype).requires_grad_(True)
    args = {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in hin.items() if k not in ("raw",)}
    out = hc.head(raw, args.pop("base_xy"), args.pop("base_z"), **args)
    sum((out[k] * torch.from_numpy(fx["g." + k]).to(dtype)).sum() for k in out).backward()
    for k, v in out.items():
        e = rel_to_max(v.detach().numpy(), fx["out." + k])
        assert e <= TOL, f"{name}: checker output {k} is {e:.2e} of its maximum away"
    # the head's share of d/d raw is the whole of it: raw reaches the outputs through the head alone
    e = rel_to_max(raw.grad.numpy(), fx["grad.raw"])
    assert e <= TOL, f"{name}: checker gradient of raw is {e:.2e} of its maximum away"
    K = out["opacities"].shape[1] // raw.shape[1]
    assert not raw.grad[:, :, K:].any() and not raw.grad[..., 2].any()


def test_state_dict_of_the_other_class_does_not_load_strictly():
    fx1, fx2 = fixture("H1_head_direct_all"), fixture("H2_head_fibonacci55")
    direct, sd_direct = build_mirror(fx1)
    fib, sd_fib = build_mirror(fx2)
    with pytest.raises(RuntimeError, match="spiral_x"):
        direct.load_state_dict(sd_fib, strict=True)
    with pytest.raises(RuntimeError, match="edge_detector"):
        fib.load_state_dict(sd_direct, strict=True)


def test_head_backend_is_validated_and_hip_refuses_cpu_tensors():
    from fresnel_amd import _binding
    from fresnel_amd.decoder import DirectPatchDecoder, gaussian_head
    with pytest.raises(ValueError, match="head_backend"):
        DirectPatchDecoder(8, 2, [8], head_backend="triton")
    raw, xy, z = torch.randn(1, 4, 2, 16), torch.zeros(4, 2), torch.zeros(1, 4)
    with pytest.raises(_binding.FgsError, match="no CPU fallback"):
        gaussian_head(raw, xy, z, backend="hip")
    with pytest.raises(ValueError, match="16 . 19"):
        gaussian_head(torch.randn(1, 4, 2, 15), xy, z)


def test_train_cli_selects_decoder_and_renderer():
    from fresnel_amd import train
    from fresnel_amd.decoder import DirectPatchDecoder, FibonacciPatchDecoder, PatchGaussianDecoder
    ap = train.arg_parser()
    cfg = train.config_from_args(ap.parse_args(["--experiment", "4", "--use_phase_blending", "--head_backend", "hip"]))
    assert (cfg.experiment, cfg.decoder, cfg.head_backend, cfg.n_spiral_points) == (4, "fibonacci", "hip", 377)
    cfg.feature_dim, cfg.head_backend = 8, "torch"
    model = train.make_decoder(cfg)
    assert isinstance(model, FibonacciPatchDecoder) and model.use_phase_output and model.gaussians_per_point == 1
    assert model.n_spiral_points == 377
    cfg = train.config_from_args(ap.parse_args([]))  # defaults: today's behaviour
    assert (cfg.experiment, cfg.decoder, cfg.head_backend) == (2, "standin", "torch")
    cfg.feature_dim = 8
    assert isinstance(train.make_decoder(cfg), PatchGaussianDecoder)
    cfg = train.config_from_args(ap.parse_args(["--decoder", "direct", "--use_edge_aware", "--gaussians_per_patch", "2"]))
    cfg.feature_dim = 8
    model = train.make_decoder(cfg)
    assert isinstance(model, DirectPatchDecoder) and model.edge_detector is not None and model.gaussians_per_patch == 2
    for bad in (["--experiment", "3"], ["--experiment", "4", "--decoder", "direct"], ["--decoder", "fibonacci"]):
        with pytest.raises(SystemExit):
            train.config_from_args(ap.parse_args(bad))
    with pytest.raises(SystemExit):
        train.main(["--experiment", "3"])


def test_experiment_4_renderer_factory_is_the_fourier_renderer():
    """TGD:1877-1890.  The renderer classes are constructed on the CPU: no kernel runs."""
    from fresnel_amd import renderer, train
    ap = train.arg_parser()
    cfg = train.config_from_args(ap.parse_args(["--experiment", "4", "--use_phase_blending"]))
    ren, cam = train.default_renderer_factory(cfg, torch.device("cpu"), 64)
    assert isinstance(ren, renderer.FourierGaussianRenderer) and (ren.width, ren.height) == (64, 64)
    assert isinstance(ren.wavelengths, torch.nn.Parameter)
    assert torch.allclose(ren.wavelengths.detach(), torch.tensor([0.65, 0.55, 0.45]))
    assert (cam.fx, cam.cx) == (64 * 0.8, 32)
    cfg = train.config_from_args(ap.parse_args(["--experiment", "4"]))
    assert isinstance(train.default_renderer_factory(cfg, torch.device("cpu"), 64)[0], renderer.TileBasedRenderer)


def test_reference_style_checkpoint_resumes_into_a_mirror():
    """A checkpoint as the reference writes it (TGD:1304-1310; plain AdamW) restores a mirror and this harness's optimizer:
    moments by position, learning rate carried, the harness's own group options kept."""
    from fresnel_amd import train
    fx = fixture("H2_head_fibonacci55")
    src, sd = build_mirror(fx)
    opt_ref = torch.optim.AdamW(src.parameters(), lr=3e-5, weight_decay=1e-5)
    _, grads, _ = run_mirror(src, fx)
    opt_ref.step()
    ck = {"epoch": 6, "model_state_dict": src.state_dict(), "optimizer_state_dict": opt_ref.state_dict()}
    dst, _ = build_mirror(fx)
    cfg = train.TrainingConfig(decoder="fibonacci", device="cpu")
    opt = train.make_optimizer(dst, cfg)
    own = {k: v for k, v in opt.param_groups[0].items() if k not in ("params", "lr", "initial_lr")}
    assert train.load_checkpoint(dst, opt, ck, cfg) == 7
    assert all(torch.equal(a, b) for a, b in zip(dst.state_dict().values(), src.state_dict().values()))
    assert opt.param_groups[0]["lr"] == 3e-5
    assert {k: v for k, v in opt.param_groups[0].items() if k not in ("params", "lr", "initial_lr")} == own
    for p, q in zip(dst.parameters(), src.parameters()):
        if q in opt_ref.state:
            assert torch.equal(opt.state[p]["exp_avg"], opt_ref.state[q]["exp_avg"])
