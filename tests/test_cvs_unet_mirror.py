"""The mirrors of the consistency view synthesizer's remaining classes (fresnel_amd/cvs.py: ResBlock, ConsistencyUNet,
ConsistencyViewSynthesizer and their parts) against the reference's fixtures R1, R2 and U1 (tests/golden/make_goldens_cvs_unet.py), on
the CPU with norm_backend "torch": they load with strict=True and reproduce output and gradients within 1e-4 of the tensor's maximum
in fp32 and fp64, reproduce the initial state dict under the fixture's seed bit for bit, and the default-config synthesizer has the
reference's keys and shapes (cvs_keys.json); forward's dict, the noising identity, generate's shapes and the three utilities."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, rel_to_max
from test_attn_checker import ref64
from test_decoder_mirror import TOL
from test_wave_attn_checker import _Fixture, cvs_fixture, state_dict_of

RES_FIXTURES = ["cvs_R1", "cvs_R2"]
_MERGED = {}


def unet_fixture(name):
    """R2's conv2 weight gradient lives in a file of its own (the size cap): read together."""
    if name not in _MERGED:
        fx = _Fixture(cvs_fixture(name))
        if name == "cvs_R2":
            fx.update(cvs_fixture("cvs_R2_convgrads"))
        _MERGED[name] = fx
    return _MERGED[name]


def _keep_norms_fp32(module):
    from fresnel_amd import cvs
    for sub in module.modules():   # GroupNorm32 computes in float32 whatever it is given: its parameters stay fp32 (the fixtures' fp64 run)
        if isinstance(sub, cvs.GroupNorm32):
            sub.float()
    return module


def build_res(fx, dtype=torch.float32):
    from fresnel_amd import cvs
    module = cvs.ResBlock(**json.loads(str(fx["ctor"])))
    module.load_state_dict(state_dict_of(fx), strict=True)
    return _keep_norms_fp32(module.eval().to(dtype))


def run_res(module, fx, dtype=torch.float32, device="cpu"):
    x = torch.from_numpy(fx["x"]).to(device, dtype).requires_grad_(True)
    t_emb = torch.from_numpy(fx["t_emb"]).to(device, dtype).requires_grad_(True)
    out = module(x, t_emb)
    (out * torch.from_numpy(fx["g"]).to(device, dtype)).sum().backward()
    res = {"out": out.detach(), "grad.x": x.grad, "grad.t_emb": t_emb.grad}
    res.update({"grad.sd." + k: p.grad for k, p in module.named_parameters()})
    return res


def build_synth(fx, dtype=torch.float32, **kw):
    """The mirror under the fixture's seed: its initial state dict IS the state dict of the fixture's runs."""
    from fresnel_amd import cvs
    ctor = json.loads(str(fx["ctor"]))
    config = cvs.CVSConfig(**{k: tuple(v) if isinstance(v, list) else v for k, v in ctor.items()})
    torch.manual_seed(int(fx["seed"]))
    return _keep_norms_fp32(cvs.ConsistencyViewSynthesizer(config, **kw).eval().to(dtype))


def run_synth(module, fx, dtype=torch.float32, device="cpu"):
    features = torch.from_numpy(fx["features"]).to(device, dtype).requires_grad_(True)
    noisy = torch.from_numpy(fx["noisy"]).to(device, dtype).requires_grad_(True)
    R_rel, t_rel = (torch.from_numpy(fx[k]).to(device, dtype) for k in ("R_rel", "t_rel"))
    image_cond = module.image_adapter(features)
    torch.set_default_dtype(dtype)   # the pose encoder builds its ray origin with torch.zeros, as the reference does
    try:
        pose_cond = module.pose_encoder(R_rel, t_rel)
    finally:
        torch.set_default_dtype(torch.float32)
    out = module.unet(noisy, torch.from_numpy(fx["timestep"]).to(device, dtype), image_cond, pose_cond)
    (out * torch.from_numpy(fx["g"]).to(device, dtype)).sum().backward()
    res = {"image_cond": image_cond[:, ::8].detach(), "pose_cond": pose_cond.detach(), "out": out.detach(), "grad.noisy": noisy.grad,
           "grad.features": features.grad}
    res.update({"grad.sd." + k: p.grad for k, p in module.named_parameters() if p.dim() == 1 or k.endswith("wavelength")})
    return res


def assert_matches_unet_fixture(fx, res, what, tol=TOL):
    """Every stored tensor within `tol` of its maximum of the reference's fp32 or fp64 run; the gradients the fixture lists as
    `cancelling` (mathematically zero, rounding noise in both of the reference's runs) are not stored and must be as small here."""
    stored = [k for k in fx if k in ("out", "image_cond", "pose_cond") or k.startswith("grad.")]
    cancelling = json.loads(str(fx["cancelling"]))
    assert sorted(res) == sorted(stored + cancelling), what
    for key in stored:
        got = res[key].detach().cpu().double().numpy()
        assert got.shape == fx[key].shape, f"{what}: shape of {key}"
        e = min(rel_to_max(got, fx[key]), rel_to_max(got, ref64(fx, key)))
        assert e <= tol, f"{what}: {key} is {e:.2e} of its maximum away from the reference's fp32 and fp64 runs"
    for key in cancelling:
        assert float(res[key].abs().max()) < 1e-4, f"{what}: {key} should cancel"


# ---- ResBlock -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", RES_FIXTURES)
def test_resblock_mirror_loads_and_reproduces_the_fixture(name, dtype):
    fx = unet_fixture(name)
    module = build_res(fx, dtype)
    assert module.norm_backend == "torch"
    assert_matches_unet_fixture(fx, run_res(module, fx, dtype), name)


def test_fixtures_are_what_they_are_for():
    r1, r2, u1 = (unet_fixture(n) for n in RES_FIXTURES + ["cvs_U1"])
    assert r1["x"].shape == (2, 32, 5, 7) and r1["out"].shape == (2, 64, 5, 7) and "sd.skip.weight" in r1
    assert r2["x"].shape == (1, 96, 3, 5) and not any(k.startswith("sd.skip") for k in r2)
    for fx in (r1, r2):   # perturbed norms on the binary grid; every gradient stored, none cancelling
        for k in ("sd.norm1.weight", "sd.norm1.bias", "sd.norm2.weight", "sd.norm2.bias"):
            assert np.ptp(fx[k]) > 0.25 and np.array_equal(fx[k] * 128, np.rint(fx[k] * 128))
        assert json.loads(str(fx["cancelling"])) == []
        assert sorted(k[8:] for k in fx if k.startswith("grad.sd.")) == sorted(k[3:] for k in fx if k.startswith("sd."))
    assert u1["features"].shape == (2, 3, 3, 384) and u1["image_cond"].shape == (2, 32, 384) and u1["pose_cond"].shape == (2, 16, 384)
    assert u1["out"].shape == u1["noisy"].shape == (2, 3, 16, 16) and not any(k.startswith("sd.") for k in u1)
    assert sum(k.startswith("grad.sd.") and k.endswith("wavelength") for k in u1) == 3   # encoder_attns.1, mid_attn, decoder_attns.0
    cap = os.path.getsize(os.path.join(GOLDEN, "attn_A1.npz"))
    for name in RES_FIXTURES + ["cvs_R2_convgrads", "cvs_U1"]:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= cap
    for fx in (r1, r2, u1):
        assert 0 < rel_to_max(fx["out"], ref64(fx, "out")) < 0.1 * TOL
        assert all(np.isfinite(v).all() for v in fx.values() if v.dtype.kind == "f")


@pytest.mark.parametrize("name", RES_FIXTURES)
def test_resblock_mirror_reproduces_the_initial_state_dict_bit_for_bit(name):
    from fresnel_amd import cvs
    fx = unet_fixture(name)
    torch.manual_seed(int(fx["seed"]))
    sd = cvs.ResBlock(**json.loads(str(fx["ctor"]))).state_dict()
    assert list(sd) == [k[7:] for k in fx if k.startswith("sd0sha.")] == [k[3:] for k in fx if k.startswith("sd.")]
    for k, v in sd.items():
        assert hashlib.sha256(v.numpy().tobytes()).hexdigest() == str(fx["sd0sha." + k]), k


# ---- the synthesizer --------------------------------------------------------------------------------------------------------------------
def test_synthesizer_mirror_reproduces_the_initial_state_dict_bit_for_bit():
    fx = unet_fixture("cvs_U1")
    module = build_synth(fx)
    sd = module.state_dict()
    assert list(sd) == [k[7:] for k in fx if k.startswith("sd0sha.")]
    for k, v in sd.items():
        assert hashlib.sha256(v.numpy().tobytes()).hexdigest() == str(fx["sd0sha." + k]), k
    # the None entries stay where the reference has them, and at least one AttentionBlock sits outside the middle
    assert [a is None for a in module.unet.encoder_attns] == [True, False] and [a is None for a in module.unet.decoder_attns] == [False]
    twin = build_synth(fx, norm_backend="hip", attn_backend="hip")
    assert list(twin.state_dict()) == list(sd)   # the keywords add no state
    from fresnel_amd import cvs
    blocks = [m for m in twin.modules() if isinstance(m, (cvs.ResBlock, cvs.AttentionBlock))]
    assert len(blocks) == 8 + 3 and all(m.norm_backend == "hip" for m in blocks) and twin.unet.norm_backend == "hip"
    assert all(m.backend == "hip" for m in twin.modules() if hasattr(m, "backend"))
    assert all(m.norm_backend == "torch" for m in module.modules() if hasattr(m, "norm_backend"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_synthesizer_mirror_reproduces_the_fixture(dtype):
    fx = unet_fixture("cvs_U1")
    assert_matches_unet_fixture(fx, run_synth(build_synth(fx, dtype), fx, dtype), "cvs_U1")


def test_default_config_mirror_has_the_reference_keys_and_shapes():
    from fresnel_amd import cvs
    with open(os.path.join(GOLDEN, "cvs_keys.json")) as f:
        want = [(k, tuple(shape)) for k, shape in json.load(f)]
    with torch.device("meta"):
        module = cvs.ConsistencyViewSynthesizer()
    assert [(k, tuple(v.shape)) for k, v in module.state_dict().items()] == want
    assert module.config.channels == [128, 256, 384, 512] and cvs.CVSConfig().attention_resolutions == (16, 8)
    # with the defaults no stage runs at 16 or 8: the only AttentionBlock is mid_attn
    assert all(a is None for a in list(module.unet.encoder_attns) + list(module.unet.decoder_attns))
    assert sum(isinstance(m, cvs.ResBlock) for m in module.modules()) == 22
    for name in ("betas", "alphas", "alphas_cumprod", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"):
        assert name in dict(module.named_buffers()) and (name, (1000,)) in want


def _small():
    from fresnel_amd import cvs
    torch.manual_seed(5)
    config = cvs.CVSConfig(image_size=8, base_channels=32, channel_mult=(1,), num_res_blocks=1, attention_resolutions=(), time_embed_dim=32,
                           pose_embed_dim=32)
    Bn = 2
    inputs = (torch.randn(Bn, 3, 8, 8), torch.randn(Bn, 2, 2, 384), torch.eye(3).expand(Bn, 3, 3), torch.randn(Bn, 3))
    return cvs.ConsistencyViewSynthesizer(config).eval(), inputs


def test_forward_returns_the_reference_dict_and_the_noising_identity():
    model, inputs = _small()
    target = torch.randn(2, 3, 8, 8)
    t = torch.tensor([3, 900])
    with torch.no_grad():
        res = model(*inputs, target_image=target, timestep=t)
        assert list(res) == ["x0_pred", "target", "noisy", "noise", "timestep"]
        assert res["x0_pred"].shape == target.shape and res["target"] is target and res["timestep"] is t
        want = (model.sqrt_alphas_cumprod[t][:, None, None, None] * target
                + model.sqrt_one_minus_alphas_cumprod[t][:, None, None, None] * res["noise"])
        assert torch.equal(res["noisy"], want)
        drawn = model(*inputs, target_image=target)["timestep"]
        assert drawn.shape == (2,) and drawn.dtype is torch.int64 and bool(((drawn >= 0) & (drawn < 1000)).all())
        assert list(model(*inputs)) == ["generated"] and model(*inputs)["generated"].shape == (2, 3, 8, 8)
    noise = torch.randn(2, 3, 8, 8)
    noisy, back = model.add_noise(target, t, noise)
    assert back is noise and torch.equal(noisy, model.sqrt_alphas_cumprod[t][:, None, None, None] * target
                                         + model.sqrt_one_minus_alphas_cumprod[t][:, None, None, None] * noise)
    # the schedule: the clamped cosine betas and what follows from them
    assert model.betas.min() == torch.tensor(0.0001) and model.betas.max() == torch.tensor(0.9999)   # both clamps are reached
    assert torch.equal(model.alphas_cumprod, torch.cumprod(1.0 - model.betas, dim=0))
    assert torch.equal(model.sqrt_one_minus_alphas_cumprod, torch.sqrt(1.0 - model.alphas_cumprod))


@pytest.mark.parametrize("steps", [1, 3])
def test_generate_returns_an_image(steps):
    model, inputs = _small()
    out = model.generate(*inputs, num_steps=steps)
    assert out.shape == (2, 3, 8, 8) and not out.requires_grad and bool(torch.isfinite(out).all())


def test_ema_and_relative_pose_are_their_one_line_definitions():
    from fresnel_amd import cvs
    model, _ = _small()
    ema = cvs.create_ema_model(model)
    assert type(ema) is type(model) and not any(p.requires_grad for p in ema.parameters())
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), ema.state_dict().values()))
    before = [p.detach().clone() for p in ema.parameters()]
    with torch.no_grad():
        for p in model.parameters():
            p.add_(1.0)
    cvs.update_ema(model, ema, decay=0.75)
    for p, p_ema, old in zip(model.parameters(), ema.parameters(), before):
        assert torch.equal(p_ema, (old * 0.75).add(p.detach(), alpha=0.25))
    g = torch.Generator().manual_seed(6)
    Rs, Rt = (torch.linalg.qr(torch.randn(2, 3, 3, generator=g))[0] for _ in range(2))
    ts, tt = torch.randn(2, 3, generator=g), torch.randn(2, 3, generator=g)
    R_rel, t_rel = cvs.get_relative_pose(Rs, ts, Rt, tt)
    assert torch.equal(R_rel, torch.bmm(Rt, Rs.transpose(-1, -2)))
    assert torch.equal(t_rel, tt - torch.bmm(R_rel, ts.unsqueeze(-1)).squeeze(-1))
    # the pose encoder's helpers: Gram-Schmidt gives a rotation, Pluecker coordinates of a ray through the origin have no moment
    enc = cvs.PluckerPoseEncoder(32, 384)
    R = enc.rotation_6d_to_matrix(torch.randn(4, 6, generator=g))
    assert torch.allclose(R.transpose(1, 2) @ R, torch.eye(3).expand(4, 3, 3), atol=1e-5)
    pl = enc.compute_plucker(torch.zeros(4, 3), torch.randn(4, 3, generator=g))
    assert torch.allclose(pl[:, :3].norm(dim=-1), torch.ones(4), atol=1e-6) and not bool(pl[:, 3:].any())
    assert cvs.SinusoidalPosEmbed(32)(torch.tensor([0.0, 5.0])).shape == (2, 32)
