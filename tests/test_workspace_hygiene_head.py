"""Workspace and output-buffer hygiene of fgs_head_workspace_bytes / _forward / _backward, through the product wrapper
(fresnel_amd.decoder.gaussian_head, backend "hip"): guard bytes around every buffer and the three fill patterns
(tests/workspace_guard.py).  Asserts A (guards intact after forward and backward), B (outputs and gradients bitwise identical
under every fill pattern and unpatched: every element is written -- the zero part of g_raw included -- and nothing is read before
it is written) and C (inputs untouched) of tests/test_workspace_hygiene.py."""
import pytest
import torch

import workspace_guard as WG
from test_hip_head import _dev, _random_case
from test_workspace_hygiene import _leaf, _sync_check

gpu = pytest.mark.gpu
LEAVES = ("raw", "base_z", "opacity_mod", "edge")


@gpu
@pytest.mark.parametrize("shape", [dict(Bn=3, P=377, KF=4, K=3, C=19, pose=True, mod=True, edge=True),
                                   dict(Bn=2, P=35, KF=3, K=2, C=16, pose=False, mod=False, edge=False),
                                   dict(Bn=2, P=55, KF=1, K=1, C=19, pose=True, mod=False, edge=True)],
                         ids=["blocks_all_inputs", "strided_plain", "under_one_wave"])
def test_head_buffers(shape):
    from fresnel_amd import decoder
    dev = _dev()
    args, ups = _random_case(seed=900 + shape["P"], **shape)
    scalars = {k: v for k, v in args.items() if not torch.is_tensor(v)}
    inp = {k: v.to(dev) for k, v in args.items() if torch.is_tensor(v)}
    inp.update({"g_" + k: v.to(dev) for k, v in ups.items()})

    def fn(guard):
        t = {k: (_leaf(inp[k]) if k in LEAVES else inp[k]) for k in args if k in inp}
        out = decoder.gaussian_head(t["raw"], t["base_xy"], t["base_z"], pose=t.get("pose"), opacity_mod=t.get("opacity_mod"),
                                    edge=t.get("edge"), backend="hip", **scalars)
        _sync_check(guard, "after the forward")
        res = {k: v.detach() for k, v in out.items()}
        sum((out[k] * inp["g_" + k]).sum() for k in out).backward()
        _sync_check(guard, "after the backward")
        res.update({"grad_" + k: t[k].grad for k in LEAVES if k in t})
        return res

    runs = WG.run_patterns(fn, inp, [decoder])
    zero = runs["zero"]
    assert all(bool(torch.isfinite(v).all()) for v in zero.values())
    assert all(bool(v.any()) for v in zero.values())
    K = shape["K"]
    for run in runs.values():
        assert not run["grad_raw"][:, :, K:].any() and not run["grad_raw"][..., 2].any()
