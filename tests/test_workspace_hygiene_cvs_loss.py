"""Workspace and output-buffer hygiene of the fused CVS loss's entry points -- fgs_cvs_loss_workspace_bytes, fgs_cvs_loss_forward,
fgs_cvs_loss_backward, fgs_cvs_quality_mask, fgs_cvs_euler_step -- through the product wrappers (fresnel_amd.cvs_losses, backend "hip"):
guard bytes around every buffer and the three fill patterns (tests/workspace_guard.py), at three of the seam shapes of
tests/test_hip_cvs_loss.py: scalar groups, one float4 group per row, and a one-pixel axis.  Asserts A (guards intact after forward and
backward), B (outputs bitwise identical under every fill pattern and unpatched: every element of out[4] -- terms that were not requested
included, as 0 --, g_pred, the mask, x_prev and t_prev is written, and nothing is read before it is written: the block partials in
scratch, the mask plane in saved) and C (inputs untouched) of tests/test_workspace_hygiene.py."""
import numpy as np
import pytest
import torch

import cvs_loss_checker as ck
import workspace_guard as WG
from test_hip_cvs_loss import ALL, DEFAULT, MSE, NO_PAIRS, _dev, _id
from test_workspace_hygiene import _leaf, _sync_check

gpu = pytest.mark.gpu

CASES = [((2, 3, 5, 7), ALL), ((2, 3, 5, 7), dict(quality=False, consistency=None, boundary=False, gradient=False)),
         ((2, 3, 4, 4), ALL), ((2, 3, 4, 4), MSE), ((1, 3, 1, 9), DEFAULT), ((1, 3, 1, 9), NO_PAIRS[2])]


@gpu
@pytest.mark.parametrize("shape, combo", CASES, ids=["x".join(map(str, s)) + "-" + _id(c) for s, c in CASES])
def test_quality_terms_buffers(shape, combo):
    from fresnel_amd import cvs_losses as L
    dev = _dev()
    inp = {k: torch.from_numpy(v).to(dev) for k, v in ck.make_case(shape, 6100 + sum(shape), edge_pair=True).items()}

    def fn(guard):
        pred = _leaf(inp["pred"])
        terms = L.cvs_quality_terms(pred, inp["target"], inp["depth"], inp["ema"], backend="hip", **combo)
        _sync_check(guard, "after the forward")
        terms.backward(inp["g_terms"])
        _sync_check(guard, "after the backward")
        return dict(terms=terms.detach(), g_pred=pred.grad)

    runs = WG.run_patterns(fn, inp, [L])
    ff = runs["ff"]   # under the NaN fill everything is finite: nothing of the fill is left or was read
    assert all(bool(torch.isfinite(v).all()) for v in ff.values()) and bool(ff["g_pred"].any())
    on = (True, combo["consistency"] is not None, combo["boundary"], combo["gradient"])
    assert [bool(v != 0) for v in ff["terms"]] == list(on)   # unrequested terms are WRITTEN, as 0


@gpu
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 3, 4, 4), (1, 3, 1, 9)], ids=lambda s: "x".join(map(str, s)))
def test_quality_mask_and_euler_step_buffers(shape):
    from fresnel_amd import cvs_losses as L
    dev = _dev()
    case = ck.make_case(shape, 6200 + sum(shape))
    inp = {k: torch.from_numpy(case[k]).to(dev) for k in ("pred", "ema", "depth")}
    inp["sac"] = torch.from_numpy(np.sqrt(np.cumprod(1.0 - np.linspace(1e-4, 0.02, 30))).astype(np.float32)).to(dev)
    inp["timestep"] = torch.tensor([0, 29][:shape[0]], device=dev)

    def fn(guard):
        mask = L.compute_quality_mask(inp["depth"], backend="hip")
        _sync_check(guard, "after the mask")
        x_prev, t_prev = L.consistency_euler_step(inp["pred"], inp["ema"], inp["sac"], inp["timestep"], backend="hip")
        _sync_check(guard, "after the Euler step")
        return dict(mask=mask, x_prev=x_prev, t_prev=t_prev)

    runs = WG.run_patterns(fn, inp, [L])
    ff = runs["ff"]
    assert all(bool(torch.isfinite(v).all()) for v in ff.values())
    assert ff["t_prev"].tolist() == [0.0, 28.0][:shape[0]] and bool(ff["mask"].any()) and bool(ff["x_prev"].any())
