"""Workspace and output-buffer hygiene of fgs_saag_inputs_forward / fgs_saag_refine_forward / fgs_saag_refine_backward (and
fgs_saag_workspace_bytes), through the product wrappers (fresnel_amd.decoder saag_mlp_inputs / saag_refine_head, backend "hip"):
guard bytes around every buffer and the three fill patterns (tests/workspace_guard.py).  Asserts A (guards intact after the gather,
the forward and the backward), B (outputs and gradients bitwise identical under every fill pattern and unpatched: every element is
written and nothing -- the scratch of the gain reduction included -- is read before it is written) and C (inputs untouched) of
tests/test_workspace_hygiene.py."""
import pytest
import torch

import workspace_guard as WG
from test_hip_saag import _channel_last, _dev, _random_case
from test_workspace_hygiene import _leaf, _sync_check

gpu = pytest.mark.gpu
CLOUD = ("positions", "scales", "rotations", "colors", "opacities")


@gpu
@pytest.mark.parametrize("shape", [dict(Bn=3, N=257, C=8, grid=(5, 7)), dict(Bn=2, N=65, C=7, grid=(3, 4)),
                                   dict(Bn=1, N=1, C=1, grid=(1, 1)), dict(Bn=1, N=300_000, C=2, grid=(3, 4))],
                         ids=["blocks_even_c", "odd_c", "single", "more_tiles_than_blocks"])
def test_saag_buffers(shape):
    from fresnel_amd import decoder
    dev = _dev()
    raw, cloud, gains, ups, feats = _random_case(seed=950 + shape["C"], **shape)
    inp = dict(raw=raw.to(dev), gains=gains.to(dev), features=_channel_last(feats, dev))
    inp.update({k: v.to(dev) for k, v in zip(CLOUD, cloud)})
    inp.update({"g_" + k: v.to(dev) for k, v in ups.items()})

    def fn(guard):
        t_raw, t_gains = _leaf(inp["raw"]), _leaf(inp["gains"])
        d = [inp[k] for k in CLOUD]
        res = {"mlp_inputs": decoder.saag_mlp_inputs(inp["features"], *d, backend="hip")}
        _sync_check(guard, "after the gather")
        out = decoder.saag_refine_head(t_raw, *d, t_gains, residual_scale=0.1, backend="hip")
        _sync_check(guard, "after the forward")
        res.update({k: v.detach() for k, v in out.items()})
        sum((out[k] * inp["g_" + k]).sum() for k in out).backward()
        _sync_check(guard, "after the backward")
        res.update(grad_raw=t_raw.grad, grad_gains=t_gains.grad)
        return res

    runs = WG.run_patterns(fn, inp, [decoder])
    zero = runs["zero"]
    assert all(bool(torch.isfinite(v).all()) for v in zero.values())
    if shape["N"] > 1:   # (a single Gaussian may sit on a clamp: a colour of exactly 0 is a written value)
        assert all(bool(v.any()) for v in zero.values())
    assert zero["mlp_inputs"].shape == (shape["Bn"], shape["N"], shape["C"] + 14) and zero["grad_gains"].shape == (4,)
