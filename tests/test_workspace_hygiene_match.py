"""Workspace and output-buffer hygiene of the matching-loss entry points (fgs_match_workspace_bytes, fgs_match_forward /
_backward), through the product wrapper (fresnel_amd.losses, backend "hip"): guard bytes around every buffer and the three fill
patterns (tests/workspace_guard.py).  Asserts A (guards intact after forward and backward), B (terms, counts, saved and g_pred
bitwise identical under every fill pattern and unpatched: every element is written -- the list entries and gradient rows of
inactive rows and skipped images included -- and nothing, the compaction scratch and the partial sums included, is read before
it is written) and C (inputs untouched) of tests/test_workspace_hygiene.py."""
import numpy as np
import pytest
import torch

import match_cases as MC
import workspace_guard as WG
from test_hip_match import _dev, _t
from test_workspace_hygiene import _leaf, _sync_check

gpu = pytest.mark.gpu


def _defaults():
    pred, target = MC.random_case(500, 2, 4096, 8192)
    pred[0, 4000:] = 0.0
    return pred, target, None, None


def _hub():
    return MC.hub_case() + (None, None)


CASES = {"defaults": _defaults, "hub_65x3000": _hub, "skipped_image": MC.skipping_case}


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_match_buffers(case):
    from fresnel_amd import losses
    dev = _dev()
    pred, target, pk, tk = CASES[case]()
    inp = dict(pred=_t(pred, dev), target=_t(target, dev), pred_keep=_t(pk, dev), target_keep=_t(tk, dev),
               g_total=torch.tensor(0.7, device=dev))

    def fn(guard):
        p = _leaf(inp["pred"])
        total, terms, counts, saved = losses._match_hip(p, inp["target"], inp["pred_keep"], inp["target_keep"], losses.MATCH_WEIGHTS)
        _sync_check(guard, "after the forward")
        total.backward(inp["g_total"])
        _sync_check(guard, "after the backward")
        return dict(total=total.detach().reshape(1), terms=terms, counts=counts, saved=saved, grad_pred=p.grad)

    runs = WG.run_patterns(fn, inp, [losses])
    zero = runs["zero"]
    Bn, Np, Nt = pred.shape[0], pred.shape[1], target.shape[1]
    assert zero["saved"].numel() == Bn * (Np + Nt + 2) and zero["saved"].dtype == torch.int32
    assert np.array_equal(zero["saved"][-2 * Bn:].cpu().numpy().reshape(Bn, 2), zero["counts"].cpu().numpy())
    assert bool(torch.isfinite(zero["terms"]).all()) and bool(torch.isfinite(zero["grad_pred"]).all()) and bool(zero["grad_pred"].any())
    assert int(zero["saved"].min()) >= -1 and int(zero["saved"][:Bn * Np].max()) < Nt and int(zero["saved"][Bn * Np:Bn * (Np + Nt)].max()) < Np
