"""Workspace and output-buffer hygiene of fgs_attn_workspace_bytes / fgs_attn_forward / fgs_attn_backward, through the product
wrapper (fresnel_amd.slat.cross_attention, backend "hip"): guard bytes around every buffer and the three fill patterns
(tests/workspace_guard.py), at shapes on the seams of the query block, the key tile, the key block and the compiled head widths, with
and without mask and dropout.  Asserts A (guards intact after forward and backward), B (output and gradients bitwise identical
under every fill pattern and unpatched: every element is written -- the padding of the tiles never shows, the zero rows of g_q
behind masked rows and both halves of g_kv are written -- and nothing is read before it is written) and C (inputs untouched) of
tests/test_workspace_hygiene.py."""
import pytest
import torch

import workspace_guard as WG
from test_hip_attn import KB, KT, QB, _case, _dev, _mask
from test_workspace_hygiene import _leaf, _sync_check

gpu = pytest.mark.gpu

SHAPES = [(2, 3, QB + 1, KT + 1, 5), (1, 2, QB - 1, KT - 1, 33), (1, 1, 1, 1, 64), (2, 1, 37, KB + 1, 128), (1, 2, 2 * QB, 2 * KT, 32)]


@gpu
@pytest.mark.parametrize("Bn,H,N,M,d", SHAPES, ids=[f"B{b}H{h}N{n}M{m}d{d}" for b, h, n, m, d in SHAPES])
@pytest.mark.parametrize("masked", [False, True], ids=["open", "masked"])
@pytest.mark.parametrize("p", [0.0, 0.5], ids=["nodrop", "drop"])
def test_attention_buffers(Bn, H, N, M, d, masked, p):
    from fresnel_amd import slat
    dev = _dev()
    q, kv, up = _case(Bn, H, N, M, d, 2100 + N + M + d)
    inp = dict(q=q.to(dev), kv=kv.to(dev), up=up.to(dev), mask=_mask(Bn, N, N).to(dev) if masked else None,
               seed=torch.tensor([2101], dtype=torch.int64, device=dev) if p else None)

    def fn(guard):
        ql, kvl = _leaf(inp["q"]), _leaf(inp["kv"])
        out = slat.cross_attention(ql, kvl, H, mask=inp["mask"], dropout_p=p, seed=inp["seed"], backend="hip")
        _sync_check(guard, "after the forward")
        out.backward(inp["up"])
        _sync_check(guard, "after the backward")
        return dict(out=out.detach(), g_q=ql.grad, g_kv=kvl.grad)

    runs = WG.run_patterns(fn, inp, [slat])
    zero = runs["zero"]
    assert all(bool(torch.isfinite(v).all()) for v in zero.values()) and bool(zero["out"].any()) and bool(zero["g_kv"][:, :, 1].any())
    if masked:
        assert not runs["ff"]["g_q"][~inp["mask"]].any()   # behind a masked row: written zeros, under the NaN fill as well
