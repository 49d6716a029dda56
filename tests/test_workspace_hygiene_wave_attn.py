"""Workspace and output-buffer hygiene of fgs_wave_attn_workspace_bytes / fgs_wave_attn_forward / fgs_wave_attn_backward, through
the product wrapper (fresnel_amd.cvs.fresnel_wave_attention, backend "hip"): guard bytes around every buffer and the three fill
patterns (tests/workspace_guard.py), at four of the seam shapes of tests/test_hip_wave_attn.py.  Asserts A (guards intact after
forward and backward), B (output and gradients bitwise identical under every fill pattern and unpatched: every element is written --
the padding of the tiles never shows, g_wavelength and all three thirds of g_qkv are written -- and nothing is read before it is
written) and C (inputs untouched) of tests/test_workspace_hygiene.py."""
import pytest
import torch

import workspace_guard as WG
from test_hip_wave_attn import KT, QB, _case, _dev
from test_workspace_hygiene import _leaf, _sync_check

gpu = pytest.mark.gpu

SHAPES = [(2, 3, 3, 43, 5), (1, 2, 1, QB - 1, 33), (1, 1, 1, 1, 64), (2, 1, 1, KT + 1, 128)]


@gpu
@pytest.mark.parametrize("Bn,H,gh,gw,d", SHAPES, ids=[f"B{b}H{h}-{gh}x{gw}-d{d}" for b, h, gh, gw, d in SHAPES])
def test_wave_attention_buffers(Bn, H, gh, gw, d):
    from fresnel_amd import cvs
    dev = _dev()
    qkv, up = _case(Bn, H, gh, gw, d, 3800 + gh + gw + d)
    inp = dict(qkv=qkv.to(dev), up=up.to(dev), wavelength=torch.tensor(0.1, device=dev))

    def fn(guard):
        ql, wl = _leaf(inp["qkv"]), _leaf(inp["wavelength"])
        out = cvs.fresnel_wave_attention(ql, (gh, gw), wl, H, backend="hip")
        _sync_check(guard, "after the forward")
        out.backward(inp["up"])
        _sync_check(guard, "after the backward")
        return dict(out=out.detach(), g_qkv=ql.grad, g_wavelength=wl.grad)

    runs = WG.run_patterns(fn, inp, [cvs])
    ff = runs["ff"]   # under the NaN fill: g_wavelength and the k and v thirds of g_qkv are written
    thirds = ff["g_qkv"].reshape(Bn, gh * gw, 3, H * d)
    assert all(bool(torch.isfinite(v).all()) for v in ff.values()) and bool(ff["out"].any())
    assert bool(thirds[:, :, 2].any())
    if gh * gw > 1:   # (one token: the softmax of one score is constant, g_q, g_k and g_wavelength are zero up to rounding)
        assert bool(thirds[:, :, 1].any()) and float(ff["g_wavelength"]) != 0.0
