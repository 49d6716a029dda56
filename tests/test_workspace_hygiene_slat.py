"""Workspace and output-buffer hygiene of fgs_slat_workspace_bytes / fgs_slat_head_forward / fgs_slat_head_backward, through the
product wrapper (fresnel_amd.slat.slat_gaussian_head, backend "hip"), ungated and gated: guard bytes around every buffer and the
three fill patterns (tests/workspace_guard.py).  Asserts A (guards intact after forward and backward), B (outputs and gradients
bitwise identical under every fill pattern and unpatched: every element is written -- the zero tail of the packed cloud and the
zeros of g_raw behind closed gates included -- and nothing is read before it is written) and C (inputs untouched) of
tests/test_workspace_hygiene.py."""
import pytest
import torch

import workspace_guard as WG
from test_hip_slat import _case, _dev, _keep
from test_workspace_hygiene import _leaf, _sync_check

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("shape", [(3, 377, 8), (2, 35, 3), (1, 55, 1), (1, 2049, 32)],
                         ids=["blocks", "odd_rows", "under_one_block", "fold_second_pass"])
def test_slat_head_buffers(shape):
    from fresnel_amd import slat
    dev = _dev()
    Bn, N, G = shape
    raw, coords, up = _case(Bn, N, G, 1800 + N)
    inp = dict(raw=raw.to(dev), coords=coords.to(dev, torch.int32), up=up.to(dev), pg=torch.tensor(0.5, device=dev),
               sf=torch.tensor(-0.3, device=dev))

    def fn(guard):
        r, pg, sf = _leaf(inp["raw"]), _leaf(inp["pg"]), _leaf(inp["sf"])
        out = slat.slat_gaussian_head(r, inp["coords"], pg, sf, backend="hip")
        _sync_check(guard, "after the forward")
        (out * inp["up"]).sum().backward()
        _sync_check(guard, "after the backward")
        return dict(out=out.detach(), grad_raw=r.grad, grad_pg=pg.grad, grad_sf=sf.grad)

    runs = WG.run_patterns(fn, inp, [slat])
    zero = runs["zero"]
    assert all(bool(torch.isfinite(v).all()) for v in zero.values()) and all(bool(v.any()) for v in zero.values())
    assert bool((zero["grad_raw"][inp["raw"].abs() > 10] == 0).all())   # behind the closed gate: written zeros


@gpu
@pytest.mark.parametrize("N", [1, 257, 513])
@pytest.mark.parametrize("pattern", ["none", "alternating", "empty_beside_full"])
def test_slat_gated_head_buffers(N, pattern):
    from fresnel_amd import slat
    dev = _dev()
    G = 3
    raw, coords, _ = _case(2, N, G, 1900 + N)
    inp = dict(raw=raw.to(dev), coords=coords.to(dev, torch.int32), keep=_keep(pattern, N).to(dev), pg=torch.tensor(0.5, device=dev),
               sf=torch.tensor(-0.3, device=dev))

    def fn(guard):
        packed, counts = slat.slat_gaussian_head(inp["raw"], inp["coords"], inp["pg"], inp["sf"], keep=inp["keep"], backend="hip")
        _sync_check(guard, "after the gated forward")
        return dict(packed=packed, counts=counts)

    runs = WG.run_patterns(fn, inp, [slat])
    counts = runs["zero"]["counts"]
    assert counts.tolist() == inp["keep"].sum(dim=1).tolist()
    for b in range(2):
        assert not runs["ff"]["packed"][b, int(counts[b]) * G:].any()   # the tail is written zero under the NaN fill as well
