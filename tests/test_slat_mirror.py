"""The mirrors of the reference's DirectSLatDecoder / MLPSLatDecoder (fresnel_amd/slat.py) with head_backend "torch" against the
fixtures S1-S4 (tests/golden/make_goldens_slat.py), on the CPU: strict loading of the reference's state dict, every output and every
recorded gradient within 1e-4 of the tensor's maximum (the tolerance of tests/test_decoder_mirror.py), the initial state dict under
the fixture's seed bit for bit, the gated inference's list lengths, argument validation, and distill_losses against the reference's
boolean-indexed occupancy term."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import GOLDEN, rel_to_max
from test_decoder_mirror import TOL

FIXTURES = ["slat_S1", "slat_S3", "slat_S4"]   # the differentiated ones; slat_S2 is the gated inference of S1's model


def fixture(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def build_mirror(fx, head_backend="torch", device="cpu"):
    from fresnel_amd import slat
    ctor = json.loads(str(fx["ctor"]))
    model = getattr(slat, str(fx["class_name"]))(**ctor, head_backend=head_backend)
    sd = {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sd.")}
    model.load_state_dict(sd, strict=True)
    return model.eval().to(device), sd


def mirror_inputs(fx, device="cpu"):
    args = [torch.from_numpy(fx["in." + k]).to(device) for k in ("features", "coords", "coord_mask") if "in." + k in fx.files]
    args[0].requires_grad_(True)
    return args


def run_mirror(model, fx, device="cpu"):
    """-> outputs, gradients {raw, features, sd.<parameter>} of sum(out x g), like the fixture's, and the captured raw."""
    args = mirror_inputs(fx, device)
    captured = {}

    def hook(_m, _i, out):
        out.retain_grad()
        captured["raw"] = out

    h = model.gaussian_head.head.register_forward_hook(hook)
    out = model(*args)
    h.remove()
    if torch.is_tensor(out):
        out = {"gaussians": out}
    model.zero_grad(set_to_none=True)
    sum((out[k] * torch.from_numpy(fx["g." + k]).to(device)).sum() for k in out).backward()
    grads = {"raw": captured["raw"].grad.reshape(fx["raw"].shape), "features": args[0].grad}
    for k, p in model.named_parameters():
        grads["sd." + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    return out, grads, captured["raw"].detach().reshape(fx["raw"].shape)


def assert_matches_fixture(fx, out, grads, raw, what, tol=TOL):
    assert sorted(out) == sorted(k[4:] for k in fx.files if k.startswith("out.")), what
    assert rel_to_max(raw.cpu().numpy(), fx["raw"]) <= tol, f"{what}: raw"
    for k, v in out.items():
        assert v.shape == fx["out." + k].shape, f"{what}: shape of {k}"
        e = rel_to_max(v.detach().cpu().numpy(), fx["out." + k])
        assert e <= tol, f"{what}: output {k} is {e:.2e} of its maximum away"
    assert sorted(grads) == sorted(k[5:] for k in fx.files if k.startswith("grad.")), what
    for k, v in grads.items():
        e = rel_to_max(v.detach().cpu().numpy(), fx["grad." + k])
        assert e <= tol, f"{what}: gradient {k} is {e:.2e} of its maximum away"


def run_gated(model, fx, device="cpu"):
    with torch.no_grad():
        return model(*[torch.from_numpy(fx["in." + k]).to(device) for k in ("features", "coords", "coord_mask")],
                     apply_occupancy_mask=True)


def assert_matches_gated_fixture(fx, out, what, tol=TOL):
    want_n = [int(n) for n in fx["out.n_gaussians"]]
    assert sorted(out) == ["gaussians", "n_gaussians", "occupancy_logits", "occupancy_mask"], what
    assert out["n_gaussians"] == want_n and [int(g.shape[0]) for g in out["gaussians"]] == want_n, what
    assert np.array_equal(out["occupancy_mask"].cpu().numpy(), fx["out.occupancy_mask"]), what
    assert rel_to_max(out["occupancy_logits"].cpu().numpy(), fx["out.occupancy_logits"]) <= tol, what
    for b, g in enumerate(out["gaussians"]):
        assert tuple(g.shape) == (want_n[b], 14)
        e = float(np.abs(g.cpu().numpy() - fx[f"out.gaussians.{b}"]).max()) if want_n[b] else 0.0
        assert e <= tol, f"{what}: image {b} is {e:.2e} away"


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_mirror_torch_backend_reproduces_the_reference(name):
    fx = fixture(name)
    model, sd = build_mirror(fx)
    # registration order is the reference's: its optimizer state is keyed by position
    assert [k for k, _ in model.named_parameters()] == [k[8:] for k in fx.files if k.startswith("grad.sd.")]
    assert list(model.state_dict()) == list(sd)
    out, grads, raw = run_mirror(model, fx)
    assert_matches_fixture(fx, out, grads, raw, name)
    assert ("occupancy_logits" in out) == (name == "slat_S1")   # predict_occupancy=False (S4) yields none; the MLP decoder has none
    assert out["gaussians"].dtype == torch.float32 and out["gaussians"].is_contiguous()


def test_fixtures_put_every_gate_to_work():
    """What the fixtures are for: raw crosses +-10, positions clamp at both ends, scales at both ends (S1), N passes the query chunk."""
    fx = fixture("slat_S1")
    raw, out = fx["raw"], fx["out.gaussians"]
    assert (raw > 10).any() and (raw < -10).any()
    assert (out[..., :3] == 1).any() and (out[..., :3] == -1).any()
    assert (out[..., 3:6] == 1).any() and (out[..., 3:6] == np.float32(1e-4)).any()
    assert (fx["in.coords"][..., 1:] < 0).any() and (fx["in.coords"][..., 1:] > 63).any()
    assert int((~fx["in.coord_mask"][1]).sum()) == 2 and fx["in.coord_mask"][0].all()
    assert float(fx["sd.gaussian_head.scale_factor"]) < 0
    assert fixture("slat_S4")["in.coords"].shape[1] == 1030 > 1024
    assert all(os.path.getsize(os.path.join(GOLDEN, n + ".npz")) < 300 * 1024 for n in FIXTURES + ["slat_S2"])


def test_initial_state_dict_is_the_references_bit_for_bit():
    from fresnel_amd.slat import DirectSLatDecoder
    fx = fixture("slat_S1")
    torch.manual_seed(int(fx["init_seed"]))
    model = DirectSLatDecoder(**json.loads(str(fx["ctor"])))
    want = {k[5:]: fx[k] for k in fx.files if k.startswith("init.")}
    sd = model.state_dict()
    assert list(sd) == list(want)
    for k, v in sd.items():
        assert np.array_equal(v.numpy().view(np.int32), want[k].view(np.int32)), k


def test_gated_inference_reproduces_the_per_image_lists():
    fx = fixture("slat_S2")
    model, _ = build_mirror(fx)
    out = run_gated(model, fx)
    assert_matches_gated_fixture(fx, out, "slat_S2")
    assert 0 < sum(out["n_gaussians"]) < 2 * 7 * 3   # a mixed mask: something kept, something dropped


def test_dropout_modules_stay():
    model, _ = build_mirror(fixture("slat_S1"))
    drops = [m for m in model.modules() if isinstance(m, torch.nn.Dropout)]
    assert len(drops) == 2 * 4 and all(d.p == 0.1 for d in drops)   # per block: attention, projection and two in the MLP


# ---- validation --------------------------------------------------------------------------------------------------------------------
def test_arguments_are_validated_without_a_gpu():
    from fresnel_amd import _binding
    from fresnel_amd.slat import DirectSLatDecoder, MLPSLatDecoder, slat_gaussian_head
    for cls in (DirectSLatDecoder, MLPSLatDecoder):
        with pytest.raises(ValueError, match="head_backend"):
            cls(8, 12, 1, head_backend="triton")
    raw, coords = torch.randn(2, 5, 3 * 14), torch.zeros(2, 5, 4, dtype=torch.int64)
    pg, sf = torch.tensor(0.5), torch.tensor(0.01)
    assert tuple(slat_gaussian_head(raw, coords, pg, sf).shape) == (2, 15, 14)
    assert tuple(slat_gaussian_head(raw.reshape(2, 5, 3, 14), coords.float(), pg, sf).shape) == (2, 15, 14)
    with pytest.raises(ValueError, match="G x 14"):
        slat_gaussian_head(torch.randn(2, 5, 3 * 14 + 1), coords, pg, sf)
    with pytest.raises(ValueError, match="G x 14"):
        slat_gaussian_head(torch.randn(2, 5, 3, 13), coords, pg, sf)
    with pytest.raises(ValueError, match="coords"):
        slat_gaussian_head(raw, coords[:, :4], pg, sf)
    with pytest.raises(ValueError, match="coords"):
        slat_gaussian_head(raw, coords[..., :3], pg, sf)
    with pytest.raises(ValueError, match="coords"):
        slat_gaussian_head(raw, coords.bool(), pg, sf)
    with pytest.raises(ValueError, match="one value"):
        slat_gaussian_head(raw, coords, torch.ones(2), sf)
    with pytest.raises(ValueError, match="backend"):
        slat_gaussian_head(raw, coords, pg, sf, backend="triton")
    keep = torch.ones(2, 5, dtype=torch.bool)
    with pytest.raises(ValueError, match="keep"):
        slat_gaussian_head(raw, coords, pg, sf, keep=keep[:, :4])
    with pytest.raises(ValueError, match="keep"):
        slat_gaussian_head(raw, coords, pg, sf, keep=keep.float())
    for backend in ("torch", "hip"):   # refused before the backend is looked at
        with pytest.raises(ValueError, match="no gradient for raw"):
            slat_gaussian_head(raw.clone().requires_grad_(True), coords, pg, sf, keep=keep, backend=backend)
        with pytest.raises(ValueError, match="no gradient for scale_factor"):
            slat_gaussian_head(raw, coords, pg, sf.clone().requires_grad_(True), keep=keep, backend=backend)
    with pytest.raises(_binding.FgsError, match="no CPU fallback"):
        slat_gaussian_head(raw, coords, pg, sf, backend="hip")
    with pytest.raises(_binding.FgsError, match="no CPU fallback"):
        slat_gaussian_head(raw, coords, pg, sf, keep=keep, backend="hip")


def test_gated_torch_backend_packs_kept_voxels_in_front():
    from fresnel_amd.slat import slat_gaussian_head
    g = torch.Generator().manual_seed(5)
    raw, coords = torch.randn(2, 6, 2, 14, generator=g), torch.randint(0, 64, (2, 6, 4), generator=g)
    keep = torch.tensor([[1, 0, 1, 1, 0, 0], [0, 0, 0, 0, 0, 1]], dtype=torch.bool)
    pg, sf = torch.tensor(0.5), torch.tensor(0.3)
    full = slat_gaussian_head(raw, coords, pg, sf).reshape(2, 6, 2, 14)
    packed, counts = slat_gaussian_head(raw, coords, pg, sf, keep=keep)
    assert counts.tolist() == [3, 1] and counts.dtype == torch.int32
    assert torch.equal(packed[0, :6], full[0, [0, 2, 3]].reshape(6, 14)) and torch.equal(packed[1, :2], full[1, 5])
    assert not packed[0, 6:].any() and not packed[1, 2:].any()


# ---- distill -----------------------------------------------------------------------------------------------------------------------
def matching_loss_of(cfg, **kw):
    """The loss as the reference's main() builds it (TDD:801-807): the five attribute weights from the config, the rest defaults."""
    from fresnel_amd.losses import GaussianMatchingLoss
    return GaussianMatchingLoss(position_weight=cfg.position_weight, scale_weight=cfg.scale_weight, rotation_weight=cfg.rotation_weight,
                                color_weight=cfg.color_weight, opacity_weight=cfg.opacity_weight, backend=cfg.match_backend, **kw)


def _distill_batch(fx, g):
    features, coords, coord_mask = (torch.from_numpy(fx["in." + k]) for k in ("features", "coords", "coord_mask"))
    target = torch.rand(2, 9, 14, generator=g)
    return dict(features=features, coords=coords, coord_mask=coord_mask, gaussians=target,
                gaussian_mask=torch.ones(2, 9, dtype=torch.bool), occupancy_target=(torch.rand(2, 7, generator=g) > 0.5).float())


def test_distill_losses_restate_the_references_occupancy_term():
    from fresnel_amd import distill
    cfg = distill.DistillConfig()
    assert (cfg.grad_clip, cfg.position_weight, cfg.scale_weight, cfg.rotation_weight, cfg.color_weight, cfg.opacity_weight,
            cfg.occupancy_weight, cfg.head_backend, cfg.match_backend) == (1.0, 1.0, 1.0, 0.5, 1.0, 5.0, 2.0, "torch", "torch")
    fx = fixture("slat_S1")
    model, _ = build_mirror(fx)
    batch = _distill_batch(fx, torch.Generator().manual_seed(11))
    loss = matching_loss_of(cfg)
    assert (loss.position_weight, loss.rotation_weight, loss.opacity_weight, loss.coverage_weight) == (1.0, 0.5, 5.0, 1.0)
    out = model(batch["features"], batch["coords"], batch["coord_mask"])
    got = distill.distill_losses(out, batch, loss, cfg)
    match = loss(out["gaussians"], batch["gaussians"], pred_mask=None, target_mask=batch["gaussian_mask"])
    m = batch["coord_mask"]
    occ = F.binary_cross_entropy_with_logits(out["occupancy_logits"][m], batch["occupancy_target"][m])   # TDD:520-526
    assert sorted(got) == sorted(list(match) + ["occupancy"])
    occ, total = float(occ.detach()), float(match["total"].detach())
    assert abs(float(got["occupancy"].detach()) - occ) <= 1e-6 * occ
    assert abs(float(got["total"].detach()) - (total + 2.0 * occ)) <= 1e-6 * (total + 2.0 * occ)
    # padded voxels do not count: changing their logits' target changes nothing
    batch["occupancy_target"][1, -2:] = 1 - batch["occupancy_target"][1, -2:]
    assert float(distill.distill_losses(out, batch, loss, cfg)["occupancy"].detach()) == float(got["occupancy"].detach())
    # without a target (or without logits) the total is the matching loss's
    del batch["occupancy_target"]
    assert sorted(distill.distill_losses(out, batch, loss, cfg)) == sorted(match)


def test_distill_step_on_the_cpu_updates_the_model_and_returns_detached_losses():
    from fresnel_amd import distill
    cfg = distill.DistillConfig()
    fx = fixture("slat_S1")
    model, _ = build_mirror(fx)
    batch = _distill_batch(fx, torch.Generator().manual_seed(12))
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    before = [p.detach().clone() for p in model.parameters()]
    losses = distill.distill_step(model, batch, opt, matching_loss_of(cfg), cfg)
    assert all(not v.requires_grad and v.dim() == 0 for v in losses.values()) and "occupancy" in losses
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    from fresnel_amd.slat import MLPSLatDecoder
    mlp = MLPSLatDecoder(12, 20, 2, 3)   # its bare tensor counts as `gaussians`; no logits, no occupancy term
    opt = torch.optim.AdamW(mlp.parameters(), lr=1e-3)
    assert "occupancy" not in distill.distill_step(mlp, batch, opt, matching_loss_of(cfg), cfg)
