"""Workspace and output-buffer hygiene of fgs_physics_forward / fgs_physics_backward (and fgs_physics_workspace_bytes), through
the product wrapper (fresnel_amd.decoder physics_head, backend "hip"): guard bytes around every buffer and the three fill patterns
(tests/workspace_guard.py).  Asserts A (guards intact after the forward and the backward), B (outputs and gradients bitwise
identical under every fill pattern and unpatched: every element is written and nothing -- the range partials, the 16-byte range and
the scratch of the three sums included -- is read before it is written) and C (inputs untouched) of tests/test_workspace_hygiene.py."""
import pytest
import torch

import workspace_guard as WG
from test_hip_physics import _case, _dev, _ups
from test_workspace_hygiene import _leaf, _sync_check

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("shape", [(3, 257, 8, 8), (2, 35, 3, 2), (1, 1, 1, 1), (1, 16385, 1, 1)],
                         ids=["tiles", "unused_k", "single", "two_range_blocks"])
def test_physics_buffers(shape):
    from fresnel_amd import decoder
    dev = _dev()
    Bn, P, KF, K = shape
    c = _case(Bn, P, KF, 960 + KF)
    inp = dict(raw=c["raw"].to(dev), base_xy=c["xy"].to(dev), base_z=c["z"].to(dev), wavelength_raw=c["lam"].to(dev))
    inp.update({"g_" + k: v.to(dev) for k, v in _ups(Bn, P * K, c["g"]).items()})

    def fn(guard):
        t_raw, t_z, t_lam = _leaf(inp["raw"]), _leaf(inp["base_z"]), _leaf(inp["wavelength_raw"])
        out = decoder.physics_head(t_raw, inp["base_xy"], t_z, t_lam, num_gaussians=K, backend="hip")
        _sync_check(guard, "after the forward")
        res = {k: v.detach() for k, v in out.items()}
        sum((out[k] * inp["g_" + k]).sum() for k in out).backward()
        _sync_check(guard, "after the backward")
        res.update(grad_raw=t_raw.grad, grad_base_z=t_z.grad, grad_wavelength_raw=t_lam.grad)
        return res

    runs = WG.run_patterns(fn, inp, [decoder])
    zero = runs["zero"]
    assert all(bool(torch.isfinite(v).all()) for v in zero.values())
    assert zero["phases"].shape == (Bn, P * K) and zero["grad_wavelength_raw"].shape == ()
