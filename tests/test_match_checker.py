"""CPU tests of tests/match_checker.py, the restatement of the GaussianMatchingLoss contract (include/fgs.h, fgs_match_*), against
the fixtures the reference's own class produced (tests/golden/match_M{1,2,3}.npz), and of fgs_match_*'s argument validation.
  * the checker's match lists equal the reference's float32 and float64 lists exactly;
  * its terms and gradient are within 1e-4 of each tensor's max of both runs (the project's parity rule);
  * mutations of the definition are caught: each moves the comparison by at least 10 x that tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import match_cases as MC
import match_checker as mc

TOL = MC.TOL


@pytest.mark.parametrize("name", MC.FIXTURES)
def test_checker_matches_reference_fixture(name):
    fx = MC.fixture(name)
    assert float(fx["min_gap"]) >= 5e-4
    ev, worst = MC.checker_on_fixture(fx)
    for p in ("", "f64."):
        assert np.array_equal(ev["fwd"], fx[p + "fwd"]) and np.array_equal(ev["bwd"], fx[p + "bwd"])
        err = MC.fixture_errors(fx, MC.out_of(ev), ev["grad"], p)
        print(name, p or "f32.", {k: f"{v:.1e}" for k, v in err.items()})
        assert max(err.values()) <= TOL, (name, p, err)
    assert worst <= TOL
    took_part = np.stack([fx["pred_keep"].sum(1), fx["target_keep"].sum(1)], 1)  # all zero for a skipped image
    skipped = (ev["counts"] == 0).any(1)
    assert np.array_equal(ev["counts"][~skipped], took_part[~skipped]) and not took_part[skipped].any()


def test_fixtures_hold_what_they_are_for():
    m1, m2, m3 = (MC.fixture(n) for n in MC.FIXTURES)
    assert "target_mask" in m1 and not mc.active(m1["pred"]).all() and not mc.active(m1["target"]).all()
    assert m2["pred"].shape[0] == 3 and not m2["target_mask"][2].any() and (m2["fwd"][2] == -1).all() and (m2["grad"][2] == 0).all()
    ev, _ = MC.checker_on_fixture(m2)
    assert np.float32(ev["terms"][1, 0]) == np.float32(MC.out_of(ev)["position"]) and ev["terms"][2].sum() == 0
    assert m3["ctor"]["max_match_points"] == 32 and len(m3["draws"]) == 4
    assert (m3["pred_keep"].sum(1) == 32).all() and (m3["target_keep"].sum(1) == 64).all()


def test_mutation_no_validity_filter_is_caught():
    assert max(MC.checker_on_fixture(MC.fixture(n), use_filter=False)[1] for n in MC.FIXTURES) >= 10 * TOL
    # (the masks of the subsampled fixture already name the rows that took part: only the zero-padded fixtures can tell)
    assert MC.checker_on_fixture(MC.fixture("match_M1"), use_filter=False)[1] >= 10 * TOL


def test_mutation_coverage_without_gradient_is_caught():
    assert all(MC.checker_on_fixture(MC.fixture(n), coverage_grad=False)[1] >= 10 * TOL for n in MC.FIXTURES)


def test_mutation_division_by_the_non_skipped_count_is_caught():
    worst = {n: MC.checker_on_fixture(MC.fixture(n), by_non_skipped=True)[1] for n in MC.FIXTURES}
    assert worst["match_M2"] >= 10 * TOL and worst["match_M1"] <= TOL and worst["match_M3"] <= TOL


def test_mutation_highest_index_wins_is_caught_on_the_lattice():
    """Exact ties: the reference's op sequence (strict `<` within cdist's row minimum and across chunks) keeps the lowest index;
    so does the canonical match.  Integer and half-integer coordinates make every distance exact in either arithmetic."""
    from fresnel_amd import losses
    pred, target = MC.lattice_case()
    p = torch.from_numpy(pred).requires_grad_(True)
    fwd, bwd, counts = losses.nearest_matches(p.detach(), torch.from_numpy(target), backend="torch")
    terms, total = losses.gaussian_matching_terms(p, torch.from_numpy(target), backend="torch")
    total.backward()
    good, bad = mc.evaluate(pred, target), mc.evaluate(pred, target, highest_wins=True)
    assert np.array_equal(good["fwd"], fwd.numpy()) and np.array_equal(good["bwd"], bwd.numpy()) and np.array_equal(good["counts"], counts.numpy())
    assert not np.array_equal(bad["fwd"], good["fwd"]) and not np.array_equal(bad["bwd"], good["bwd"])
    # four candidates tie for every interior point
    d2 = mc.d2_matrix(pred[0, :, :3], target[0, :, :3])
    assert ((d2 == d2.min(1, keepdims=True)).sum(1) == 4).sum() >= 24
    err = lambda ev: max(MC.rel_to_max(ev["grad"], p.grad.numpy()), MC.rel_to_max(ev["terms"], terms.detach().numpy()))  # noqa: E731
    assert err(good) <= TOL and err(bad) >= 10 * TOL


def test_checker_properties():
    pred, target, pk, tk = MC.skipping_case()
    ev = mc.evaluate(pred, target, pk, tk, g_total=0.7)
    assert (ev["fwd"][0] == -1).all() and (ev["bwd"][0] == -1).all() and (ev["fwd"][2] == -1).all() and (ev["bwd"][2] == -1).all()
    assert not ev["terms"][0].any() and not ev["terms"][2].any() and ev["terms"][1, 6] > 0
    assert not ev["grad"][0].any() and not ev["grad"][2].any() and not ev["grad"][1][ev["fwd"][1] < 0].any()
    assert ev["total"] == ev["terms"][1, 6] / 3
    act = mc.active(MC.filter_seam_case()[0])[0]
    assert list(act[:4]) == [False, True, False, True] and act[4:].all()
    # the gradient is the derivative of the terms: central differences in float64 on a small cloud without near-ties
    fx = MC.fixture("match_M1")
    p64 = fx["pred"].astype(np.float64)
    ev = mc.evaluate(fx["pred"], fx["target"], *MC.fixture_masks(fx))
    b, i, c = 1, int(np.nonzero(ev["fwd"][1] >= 0)[0][3]), 7
    assert abs(ev["grad"][b, i, c]) > 0
    vals = []
    for h in (1e-3, -1e-3):
        q = p64.copy()
        q[b, i, c] += h
        q32 = q.astype(np.float32)
        vals.append(mc.total(mc.terms(q32, fx["target"], ev["fwd"], ev["bwd"], ev["counts"])))
    assert abs((vals[0] - vals[1]) / 2e-3 - ev["grad"][b, i, c]) <= 2e-3 * abs(ev["grad"][b, i, c]) + 1e-6


def _dims(Bn=2, Np=8, Nt=9):
    from fresnel_amd import _binding as Bd
    d = Bd.FgsMatchDims()
    d.batch, d.num_pred, d.num_target = Bn, Np, Nt
    return d


def test_entry_points_validate_arguments_without_a_gpu():
    from fresnel_amd import _binding as Bd
    lib = Bd.load()
    s, c = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.fgs_match_workspace_bytes(ctypes.byref(_dims()), ctypes.byref(s), ctypes.byref(c)) == 0
    assert s.value == 4 * 2 * (8 + 9 + 2) and c.value > 0 and c.value % 256 == 0
    for bad in (_dims(Bn=0), _dims(Np=0), _dims(Nt=0)):
        assert lib.fgs_match_workspace_bytes(ctypes.byref(bad), ctypes.byref(s), ctypes.byref(c)) == -1
    for big in (_dims(Bn=65536), _dims(Np=65537), _dims(Nt=65537)):
        assert lib.fgs_match_workspace_bytes(ctypes.byref(big), ctypes.byref(s), ctypes.byref(c)) == -3
    assert lib.fgs_match_workspace_bytes(ctypes.byref(_dims(Np=65536, Nt=65536)), ctypes.byref(s), ctypes.byref(c)) == 0
    assert lib.fgs_match_workspace_bytes(ctypes.byref(_dims()), None, None) == -1
    assert lib.fgs_match_forward(ctypes.byref(_dims()), *([None] * 9)) == -1 and b"null" in lib.fgs_last_error()
    assert lib.fgs_match_backward(ctypes.byref(_dims()), *([None] * 7)) == -1
    assert lib.fgs_match_forward(ctypes.byref(_dims(Np=70000)), *([None] * 9)) == -3
    assert Bd.FGS_MATCH_TILE == 1024
    import os
    import re
    from helpers import ROOT
    hdr = open(os.path.join(ROOT, "include", "fgs.h")).read()
    assert int(re.search(r"#define FGS_MATCH_TILE (\d+)", hdr).group(1)) == Bd.FGS_MATCH_TILE
