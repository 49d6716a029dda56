"""Workspace and output-buffer hygiene of fgs_attn_half_workspace_bytes / fgs_attn_half_forward / fgs_attn_half_backward, through the
product wrapper (fresnel_amd.slat.cross_attention, backend "hip", compute_dtype fp16 / bf16): guard bytes around every buffer and
the three fill patterns (tests/workspace_guard.py), at one shape that takes the vector loads and stores (head_dim % 8 == 0) and one
that takes the element-wise form, on the seams of the query block and the key tile, with and without mask and dropout.  Asserts A
(guards intact after forward and backward), B (output and gradients bitwise identical under every fill pattern and unpatched: every
element is written -- the zero rows of g_q behind masked rows and both halves of g_kv included -- and nothing is read before it is
written) and C (inputs untouched) of tests/test_workspace_hygiene.py."""
import pytest
import torch

import workspace_guard as WG
from test_hip_attn import QB, _case, _dev, _mask
from test_workspace_hygiene import _leaf, _sync_check

from fresnel_amd import _binding as B

gpu = pytest.mark.gpu
KT = B.FGS_ATTN_HALF_KEY_TILE

SHAPES = [(2, 2, QB + 1, KT + 1, 16), (1, 3, QB - 1, 2 * KT - 1, 33)]


@gpu
@pytest.mark.parametrize("Bn,H,N,M,d", SHAPES, ids=["vector", "elementwise"])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("masked", [False, True], ids=["open", "masked"])
@pytest.mark.parametrize("p", [0.0, 0.5], ids=["nodrop", "drop"])
def test_half_attention_buffers(Bn, H, N, M, d, dt, masked, p):
    from fresnel_amd import slat
    dev = _dev()
    q, kv, up = (t.to(dt) for t in _case(Bn, H, N, M, d, 2300 + N + M + d))
    inp = dict(q=q.to(dev), kv=kv.to(dev), up=up.to(dev), mask=_mask(Bn, N, N).to(dev) if masked else None,
               seed=torch.tensor([2301], dtype=torch.int64, device=dev) if p else None)

    def fn(guard):
        ql, kvl = _leaf(inp["q"]), _leaf(inp["kv"])
        out = slat.cross_attention(ql, kvl, H, mask=inp["mask"], dropout_p=p, seed=inp["seed"], backend="hip", compute_dtype=dt)
        _sync_check(guard, "after the forward")
        out.backward(inp["up"])
        _sync_check(guard, "after the backward")
        return dict(out=out.detach(), g_q=ql.grad, g_kv=kvl.grad)

    runs = WG.run_patterns(fn, inp, [slat])
    zero = runs["zero"]
    assert all(v.dtype is dt for v in zero.values())
    assert all(bool(torch.isfinite(v).all()) for v in zero.values()) and bool(zero["out"].any()) and bool(zero["g_kv"][:, :, 1].any())
    if masked:
        assert not runs["ff"]["g_q"][~inp["mask"]].any()   # behind a masked row: written zeros, under the NaN fill as well
