"""Workspace and output-buffer hygiene of fgs_gn_silu_workspace_bytes / fgs_gn_silu_forward / fgs_gn_silu_backward, through the
product wrapper (fresnel_amd.cvs.group_norm_act, backend "hip"): guard bytes around every buffer and the three fill patterns
(tests/workspace_guard.py), at four of the seam shapes of tests/test_hip_gn_silu.py -- the misaligned one (span 105) and a split one
(a last segment of one float4) among them -- with and without channel_bias.  Asserts A (guards intact after forward and backward), B
(output and gradients bitwise identical under every fill pattern and unpatched: every element is written -- a row's tail, a
segment's tail, g_channel_bias, g_weight and g_bias -- and nothing is read before it is written: the segment pairs, the channel sums
and the group coefficients in scratch, (mean, rstd) in saved) and C (inputs untouched) of tests/test_workspace_hygiene.py."""
import pytest
import torch

import workspace_guard as WG
from test_gn_checker import gn_case
from test_hip_gn_silu import S, _dev
from test_workspace_hygiene import _leaf, _sync_check

gpu = pytest.mark.gpu

SHAPES = [(2, 96, 5, 7), (1, 64, 1, S + 4), (3, 96, 1, 3), (2, 64, 1, 2)]


@gpu
@pytest.mark.parametrize("with_bias", [True, False], ids=["cb", "nocb"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_group_norm_act_buffers(shape, with_bias):
    from fresnel_amd import cvs
    dev = _dev()
    case = gn_case(shape, 32, 5900 + sum(shape), with_bias)
    inp = {k: (case[k].to(dev) if case[k] is not None else None) for k in ("x", "weight", "bias", "channel_bias", "g_out")}

    def fn(guard):
        x, w, b = _leaf(inp["x"]), _leaf(inp["weight"]), _leaf(inp["bias"])
        cb = _leaf(inp["channel_bias"]) if with_bias else None
        out = cvs.group_norm_act(x, 32, w, b, channel_bias=cb, backend="hip")
        _sync_check(guard, "after the forward")
        out.backward(inp["g_out"])
        _sync_check(guard, "after the backward")
        res = dict(out=out.detach(), g_x=x.grad, g_weight=w.grad, g_bias=b.grad)
        if with_bias:
            res["g_channel_bias"] = cb.grad
        return res

    runs = WG.run_patterns(fn, inp, [cvs])
    ff = runs["ff"]   # under the NaN fill everything is finite: nothing of the fill is left or was read
    assert all(bool(torch.isfinite(v).all()) for v in ff.values())
    assert all(bool(ff[k].any()) for k in ("out", "g_x", "g_weight", "g_bias"))
