"""CPU tests of fresnel_amd.losses.GaussianMatchingLoss (backend "torch", the restatement of the reference's op sequence) against
the fixtures of the reference's own class (tests/golden/match_M{1,2,3}.npz), in float32 and float64 with the recorded draws
replayed: the seven values and d total / d pred within 1e-4 of each tensor's max; the match lists exactly."""
import inspect

import numpy as np
import pytest
import torch

import match_cases as MC

TOL = MC.TOL


def _inputs(fx, dtype):
    pred = torch.from_numpy(fx["pred"]).to(dtype).requires_grad_(True)
    target = torch.from_numpy(fx["target"]).to(dtype)
    pm = torch.from_numpy(fx["pred_mask"]).bool() if "pred_mask" in fx else None
    tm = torch.from_numpy(fx["target_mask"]).bool() if "target_mask" in fx else None
    return pred, target, pm, tm


@pytest.mark.parametrize("prefix, dtype", [("", torch.float32), ("f64.", torch.float64)], ids=["f32", "f64"])
@pytest.mark.parametrize("name", MC.FIXTURES)
def test_mirror_matches_the_reference(name, prefix, dtype):
    from fresnel_amd.losses import GaussianMatchingLoss
    fx = MC.fixture(name)
    pred, target, pm, tm = _inputs(fx, dtype)
    loss = GaussianMatchingLoss(**fx["ctor"])
    with MC.replayed_randperm(fx["draws"]) as left:
        out = loss(pred, target, pm, tm)
    assert not left, "the mirror drew fewer permutations than the reference"
    assert tuple(out) == MC.OUT_KEYS and all(v.dim() == 0 and v.dtype == dtype for v in out.values())
    out["total"].backward()
    err = MC.fixture_errors(fx, {k: v.detach().numpy() for k, v in out.items()}, pred.grad.numpy(), prefix)
    print(name, {k: f"{v:.1e}" for k, v in err.items()})
    assert max(err.values()) <= TOL, err


@pytest.mark.parametrize("name", MC.FIXTURES[:2])
def test_torch_lists_are_the_references(name):
    from fresnel_amd.losses import gaussian_matching_terms, nearest_matches
    fx = MC.fixture(name)
    pred, target, pm, tm = _inputs(fx, torch.float32)
    fwd, bwd, counts = nearest_matches(pred.detach(), target, pm, tm)
    assert fwd.dtype == bwd.dtype == counts.dtype == torch.int32
    assert np.array_equal(fwd.numpy(), fx["fwd"]) and np.array_equal(bwd.numpy(), fx["bwd"])
    took_part = np.stack([fx["pred_keep"].sum(1), fx["target_keep"].sum(1)], 1)  # all zero for a skipped image
    live = ~(counts.numpy() == 0).any(1)
    assert np.array_equal(counts.numpy()[live], took_part[live]) and not took_part[~live].any()
    terms, total = gaussian_matching_terms(pred, target, pm, tm)
    assert terms.shape == (pred.shape[0], 8) and not terms[:, 7].any()
    assert MC.rel_to_max(total.detach().numpy(), fx["out.total"]) <= TOL
    skipped = (counts == 0).any(1)
    assert not terms[skipped].any() and (fwd[skipped] == -1).all()


def test_all_images_skipped_gives_zeros():
    from fresnel_amd.losses import GaussianMatchingLoss
    out = GaussianMatchingLoss()(torch.rand(2, 5, 14), torch.zeros(2, 6, 14))
    assert tuple(out) == MC.OUT_KEYS and all(float(v) == 0.0 for v in out.values())


def test_constructor_defaults_are_the_references():
    from fresnel_amd.losses import GaussianMatchingLoss
    sig = inspect.signature(GaussianMatchingLoss.__init__)
    got = {k: p.default for k, p in sig.parameters.items() if k != "self"}
    assert got == dict(position_weight=10.0, scale_weight=5.0, rotation_weight=2.0, color_weight=5.0, opacity_weight=3.0,
                       coverage_weight=1.0, max_match_points=4096, chunk_size=2048, backend="torch", generator=None)
    assert list(got)[:8] == ["position_weight", "scale_weight", "rotation_weight", "color_weight", "opacity_weight", "coverage_weight",
                             "max_match_points", "chunk_size"]
    m = GaussianMatchingLoss()
    assert m.backend == "torch" and not list(m.parameters())


def test_hip_backend_refuses_cpu_tensors_and_target_gradients():
    from fresnel_amd import _binding as B
    from fresnel_amd.losses import GaussianMatchingLoss, gaussian_matching_terms, nearest_matches
    pred, target = torch.rand(1, 5, 14), torch.rand(1, 6, 14)
    with pytest.raises(B.FgsError, match="no CPU fallback"):
        GaussianMatchingLoss(backend="hip")(pred, target)
    with pytest.raises(B.FgsError):
        gaussian_matching_terms(pred, target, backend="hip")
    with pytest.raises(B.FgsError):
        nearest_matches(pred, target, backend="hip")
    with pytest.raises(ValueError, match="no gradient for target"):
        GaussianMatchingLoss(backend="hip")(pred, target.clone().requires_grad_(True))
    # a mask on another device than the clouds: the kernels would read its address on the GPU, so it is refused by name (and
    # before anything else looks for a GPU, so that this machine can tell)
    for kw in (dict(pred_mask=torch.ones(1, 5, dtype=torch.bool, device="meta")), dict(target_mask=torch.ones(1, 6, dtype=torch.uint8, device="meta"))):
        for call in (GaussianMatchingLoss(backend="hip"), lambda *a, **k: gaussian_matching_terms(*a, backend="hip", **k),
                     lambda *a, **k: nearest_matches(*a, backend="hip", **k)):
            with pytest.raises(B.FgsError, match=f"{list(kw)[0]} is on meta"):
                call(pred, target, **kw)
    with pytest.raises(B.FgsError):
        GaussianMatchingLoss(backend="triton")
    with pytest.raises(B.FgsError):
        GaussianMatchingLoss()(torch.rand(1, 5, 13), target)
    with pytest.raises(B.FgsError):
        GaussianMatchingLoss()(pred, target, pred_mask=torch.ones(1, 4))
    # the torch backend differentiates with respect to the target as autograd does
    t = target.clone().requires_grad_(True)
    GaussianMatchingLoss()(pred, t)["total"].backward()
    assert t.grad is not None and bool(t.grad.any())
