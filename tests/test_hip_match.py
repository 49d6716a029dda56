"""GPU tests of the fused GaussianMatchingLoss (csrc/fgs_match.hip through fresnel_amd.losses, backend "hip") against
tests/match_checker.py, the CPU restatement of include/fgs.h.  In every case: the match lists and the counts are equal, the
gradient rows are bit-equal, the terms are within 1e-6 relative of the checker's float64 evaluation on the same lists (rotation:
1e-6 absolute), and a second call repeats every output bit for bit.

The 1e-6 is derived, not measured: a term is a sum of non-negative float32 values that kernel and checker form with the same
operations -- at most four roundings of 2^-24 each against exact arithmetic, and none against each other -- added in float64
(order-dependent at 1e-16) and rounded to float32 once (6e-8).  `rotation` is 1 - mean: its bound is absolute."""
import numpy as np
import pytest
import torch

import match_cases as MC
import match_checker as mc

gpu = pytest.mark.gpu
G = 0.7  # the upstream gradient of `total`
REL = 1e-6


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run_hip(pred, target, pk=None, tk=None, weights=None, g=G):
    """-> dict of numpy arrays: fwd, bwd, counts, terms (B, 8) float32, total, grad."""
    from fresnel_amd import losses
    dev = _dev()
    w = [mc._w(weights)[k] for k in mc.KEYS]
    p, t = _t(pred, dev).requires_grad_(True), _t(target, dev)
    terms, total = losses.gaussian_matching_terms(p, t, _t(pk, dev), _t(tk, dev), weights=w, backend="hip")
    (total * g).backward()
    fwd, bwd, counts = losses.nearest_matches(p.detach(), t, _t(pk, dev), _t(tk, dev), backend="hip")
    torch.cuda.synchronize()
    return dict(fwd=fwd.cpu().numpy(), bwd=bwd.cpu().numpy(), counts=counts.cpu().numpy(), terms=terms.detach().cpu().numpy(),
                total=total.detach().cpu().numpy(), grad=p.grad.cpu().numpy())


def same_bits(a, b):
    """Bit-equal floats; a NaN equals any NaN (numpy and the device may differ in its payload)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    return a.shape == b.shape and bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


def assert_case(pred, target, pk=None, tk=None, weights=None):
    ev = mc.evaluate(pred, target, pk, tk, weights, g_total=np.float32(G))
    got, again = run_hip(pred, target, pk, tk, weights), run_hip(pred, target, pk, tk, weights)
    Bn, Np, Nt = pred.shape[0], pred.shape[1], target.shape[1]
    assert got["fwd"].shape == (Bn, Np) and got["bwd"].shape == (Bn, Nt) and got["grad"].shape == pred.shape
    # in range for any input: -1 or an active row of the other side
    for lst, n, act in ((got["fwd"], Nt, mc.active(target, tk)), (got["bwd"], Np, mc.active(pred, pk))):
        assert lst.min() >= -1 and lst.max() < n
        for b in range(Bn):
            assert act[b][lst[b][lst[b] >= 0]].all()
    for k in ("fwd", "bwd", "counts"):
        assert np.array_equal(got[k], ev[k]), k
    bad = ~((got["grad"].view(np.int32) == ev["grad"].view(np.int32)) | (np.isnan(got["grad"]) & np.isnan(ev["grad"])))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4], got["grad"][bad][:4], ev["grad"][bad][:4])
    want = ev["terms"]
    err = np.abs(got["terms"].astype(np.float64) - want)
    print("terms: largest relative error", float(np.nanmax(err / np.maximum(np.abs(want), 1e-300) * (want != 0))), "rotation abs", float(np.nanmax(err[:, 2])))
    cols = [0, 1, 3, 4, 5, 6, 7]
    assert bool(((err[:, cols] <= REL * np.abs(want[:, cols])) | (np.isnan(got["terms"][:, cols]) & np.isnan(want[:, cols]))).all())
    assert bool(((err[:, 2] <= REL) | (np.isnan(got["terms"][:, 2]) & np.isnan(want[:, 2]))).all())
    assert abs(float(got["total"]) - ev["total"]) <= REL * abs(ev["total"]) or (np.isnan(got["total"]) and np.isnan(ev["total"]))
    for k in got:
        assert same_bits(got[k], again[k]), f"the second call differs in {k}"
    return ev, got


@gpu
@pytest.mark.parametrize("Bn,Np,Nt", [(1, 1, 1), (2, 64, 70), (2, 65, 63), (3, 300, 500)], ids=["1x1x1", "np64", "np65", "three_blocks"])
def test_smallest_shapes(Bn, Np, Nt):
    assert_case(*MC.random_case(100 + Np, Bn, Np, Nt))


@gpu
@pytest.mark.parametrize("delta", [-1, 0, 1], ids=["tile_minus_1", "tile", "tile_plus_1"])
def test_candidate_tile_seam(delta):
    """Nt (and, in the other direction, the candidate count Np of the second call) on and beside the LDS candidate tile."""
    from fresnel_amd import _binding as B
    n = B.FGS_MATCH_TILE + delta
    assert_case(*MC.random_case(200 + delta, 1, 130, n))
    pred, target = MC.random_case(210 + delta, 1, n, 90)
    pk = np.ones((1, n), np.uint8)
    pk[0, 5] = 0  # the compacted candidates end one before the seam
    assert_case(pred, target, pk, None)


@gpu
def test_exact_ties_lattice_and_coincident_points():
    ev, _ = assert_case(*MC.lattice_case())
    assert not np.array_equal(ev["fwd"], mc.matches(*MC.lattice_case(), highest_wins=True)[0])
    ev, _ = assert_case(*MC.coincident_case())
    assert (ev["fwd"][0, :20] == np.where(np.arange(20) == 10, 3, np.arange(20))).all()  # the lowest of the coincident candidates


@gpu
def test_hub_prediction_collects_every_target():
    pred, target = MC.hub_case()
    ev, got = assert_case(pred, target)
    assert (got["bwd"] == 17).all() and (got["fwd"] >= 0).all()
    forward_only = mc.grad_rows(pred, target, ev["fwd"], ev["bwd"], ev["counts"], g_total=np.float32(G), coverage_grad=False)
    differs = (got["grad"] != forward_only).any(-1)[0]
    assert differs[17] and differs.sum() == 1  # in-degree 3000 on one row, 0 on the 64 others


@gpu
def test_masks_and_skipped_images_equal_their_single_images():
    pred, target, pk, tk = MC.skipping_case()
    ev, got = assert_case(pred, target, pk, tk)
    assert (got["counts"][0, 0], got["counts"][2, 1]) == (0, 0) and got["counts"][1].min() > 0
    for b in (0, 2):
        assert (got["fwd"][b] == -1).all() and (got["bwd"][b] == -1).all() and not got["terms"][b].any() and not got["grad"][b].any()
    assert float(got["total"]) == np.float32(np.float64(got["terms"][1, 6]) / 3)
    g1 = np.float32(G) * (np.float32(1) / np.float32(3))  # the per-image factor of the batch of three, handed to a batch of one
    for b in range(3):
        one = run_hip(pred[b:b + 1], target[b:b + 1], pk[b:b + 1], tk[b:b + 1], g=float(g1))
        for k in ("fwd", "bwd", "counts", "terms", "grad"):
            assert same_bits(one[k][0], got[k][b]), (b, k)


@gpu
def test_filter_seam():
    pred, target = MC.filter_seam_case()
    ev, got = assert_case(pred, target)
    assert list(got["fwd"][0, :4] >= 0) == [False, True, False, True] and tuple(got["counts"][0]) == (10, 10)
    assert not got["grad"][0, 0].any() and not got["grad"][0, 2].any() and got["grad"][0, 1].any()


@gpu
def test_quaternion_edge_cases():
    pred, target = MC.quaternion_case()
    ev, got = assert_case(pred, target)
    assert (got["fwd"][0] == np.arange(8)).all() and np.isfinite(got["grad"]).all()
    assert not got["grad"][0, 0, 6:10].any()          # zero quaternion: q^p = 0, dot = 0, sign(0) = 0
    assert got["grad"][0, 1, 6] != 0                  # norm 1e-9, under the clamp: gh / 1e-8 with nothing through the norm, so the
    #                                                   gradient keeps its component ALONG q (an unclamped one is orthogonal to q)
    assert not got["grad"][0, 2, 6:10].any()          # dot exactly 0: sign(0) = 0
    assert not got["grad"][0, 3, 6:10].any()          # zero target quaternion: q^t = 0


@gpu
def test_nan_and_inf_stay_in_range_and_reach_the_total():
    pred, target = MC.nan_inf_case()
    ev, got = assert_case(pred, target)  # (the range check is in there)
    assert np.isnan(got["total"]) and np.isnan(got["terms"][0, 0]) and got["fwd"][1, 2] == -1


@gpu
def test_default_sizes():
    pred, target = MC.random_case(300, 2, 4096, 8192)
    pred[1, 4000:] = 0.0
    assert_case(pred, target)


@gpu
@pytest.mark.parametrize("name", MC.FIXTURES)
def test_reference_fixtures_through_the_module(name):
    """The reference's own results under the project's parity rule (1e-4 of each tensor's max, float32 and float64 runs).  The
    subsampled fixture is given as the masks of the rows the recorded draws kept: row order does not enter the definition."""
    from fresnel_amd.losses import GaussianMatchingLoss
    dev = _dev()
    fx = MC.fixture(name)
    ctor = {k: v for k, v in fx["ctor"].items() if k != "max_match_points"}
    pk, tk = MC.fixture_masks(fx)
    p = _t(fx["pred"], dev).requires_grad_(True)
    out = GaussianMatchingLoss(backend="hip", **ctor)(p, _t(fx["target"], dev), _t(pk, dev), _t(tk, dev))
    assert tuple(out) == MC.OUT_KEYS
    out["total"].backward()
    for prefix in ("", "f64."):
        err = MC.fixture_errors(fx, {k: v.detach().cpu().numpy() for k, v in out.items()}, p.grad.cpu().numpy(), prefix)
        print(name, prefix or "f32.", {k: f"{v:.1e}" for k, v in err.items()})
        assert max(err.values()) <= MC.TOL, err


@gpu
def test_subsampling_keeps_exactly_k_active_rows():
    from fresnel_amd import losses
    dev = _dev()
    pred, target = MC.random_case(400, 2, 300, 700)
    pred[0, 100:130] = 0.0
    pm = np.ones((2, 300), np.uint8)
    pm[1, ::5] = 0
    K = 128
    act = mc.active(pred, pm)
    assert act.sum(1).min() > K

    def keep(seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        return losses._subsample_keep(_t(pred, dev), _t(pm, dev), K, g).cpu().numpy()

    a, b, c = keep(1), keep(1), keep(2)
    assert a.dtype == np.bool_ and (a.sum(1) == K).all() and not (a & ~act).any()
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    # fewer active rows than the cap: all of them survive; within the cap nothing is drawn and the mask comes back as it is
    few = pm.copy()
    few[0, 50:] = 0
    got = losses._subsample_keep(_t(pred, dev), _t(few, dev), K, torch.Generator(device=dev).manual_seed(3)).cpu().numpy()
    assert np.array_equal(got[0], mc.active(pred, few)[0]) and got[1].sum() == K
    m = _t(pm, dev)
    assert losses._subsample_keep(_t(pred, dev), m, 300, None) is m and losses._subsample_keep(_t(pred, dev), None, 300, None) is None
    # the module: 128 predictions and 256 targets per image take part, the same seed gives the same loss
    def total(seed):
        loss = losses.GaussianMatchingLoss(max_match_points=K, backend="hip", generator=torch.Generator(device=dev).manual_seed(seed))
        return float(loss(_t(pred, dev), _t(target, dev), _t(pm, dev))["total"])

    g = torch.Generator(device=dev).manual_seed(1)
    pk = losses._subsample_keep(_t(pred, dev), _t(pm, dev), K, g)
    tk = losses._subsample_keep(_t(target, dev), None, 2 * K, g)
    _, _, counts = losses.nearest_matches(_t(pred, dev), _t(target, dev), pk, tk, backend="hip")
    assert (counts.cpu().numpy() == [K, 2 * K]).all()
    want = mc.evaluate(pred, target, pk.cpu().numpy(), tk.cpu().numpy())["total"]
    assert abs(total(1) - want) <= 1e-6 * want and total(1) == total(1) and total(1) != total(2)


@gpu
@pytest.mark.parametrize("subsample", [False, True], ids=["within_the_cap", "subsampled"])
def test_module_makes_no_host_synchronisation(subsample):
    """Forward + backward of the module on "hip" under torch's sync debug mode, with bool masks (the reference's kind), once with
    the row counts within the cap and once with both sides subsampled."""
    from fresnel_amd.losses import GaussianMatchingLoss
    dev = _dev()
    pred, target, pk, tk = MC.skipping_case()
    p, t = _t(pred, dev).requires_grad_(True), _t(target, dev)
    pm, tm = _t(pk, dev).bool(), _t(tk, dev).bool()
    loss = GaussianMatchingLoss(max_match_points=32 if subsample else 4096, backend="hip", generator=torch.Generator(device=dev).manual_seed(4))
    loss(p, t, pm, tm)["total"].backward()  # library load, first launches
    p.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = loss(p, t, pm, tm)
        out["total"].backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(out) == MC.OUT_KEYS and float(out["total"]) > 0 and bool(p.grad.any()) and not bool(p.grad[0].any())


@gpu
def test_masks_on_another_device_are_refused():
    from fresnel_amd import _binding as B
    from fresnel_amd import losses
    dev = _dev()
    pred, target, pk, tk = MC.skipping_case()
    p, t = _t(pred, dev), _t(target, dev)
    with pytest.raises(B.FgsError, match="pred_mask is on cpu"):
        losses.GaussianMatchingLoss(backend="hip")(p, t, torch.from_numpy(pk).bool())
    with pytest.raises(B.FgsError, match="target_mask is on cpu"):
        losses.nearest_matches(p, t, None, torch.from_numpy(tk), backend="hip")
    with pytest.raises(B.FgsError, match="target is on cpu"):
        losses.gaussian_matching_terms(p, t.cpu(), backend="hip")
