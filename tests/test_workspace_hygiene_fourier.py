"""Workspace and output-buffer hygiene of fgs_fourier_workspace_bytes / _forward / _backward, through the product wrapper:
guard bytes around every buffer and the three fill patterns (tests/workspace_guard.py), with the helpers of
tests/test_workspace_hygiene.py.  Asserts A (guards intact after forward and backward), B (image and gradients bitwise
identical under every fill pattern and unpatched) and C (inputs untouched) of that file."""
import numpy as np
import pytest
import torch

from helpers import synth_aniso
from test_workspace_hygiene import GRADS, _dev, _leaf, _run, _sync_check, _up

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("W,H,Bn", [(56, 40, 2), (128, 128, 1)])
def test_fourier_renderer_buffers(W, H, Bn):
    from fresnel_amd.renderer import Camera, FourierGaussianRenderer
    dev = _dev()
    rs = np.random.RandomState(1200 + W)
    per = [synth_aniso(150, 1201 + W + b, opacity_max=1.1) for b in range(Bn)]
    inp = {k: _up(np.stack([p[i] for p in per])) for i, k in enumerate(GRADS)}
    inp["gI"] = _up(rs.standard_normal((Bn, 3, H, W)).astype(np.float32))
    cam = Camera(0.8 * W, 0.8 * W, W / 2, H / 2, W, H)
    ren = FourierGaussianRenderer(W, H, background=(0.05, 0.1, 0.15)).to(dev)

    def fn(guard):
        ts = [_leaf(inp[k]) for k in GRADS]
        img = ren(*ts, cam)
        _sync_check(guard, "after the forward")
        out = dict(image=img.detach())
        (img * inp["gI"]).sum().backward()
        _sync_check(guard, "after the backward")
        out.update({"grad_" + k: t.grad for k, t in zip(GRADS, ts)})
        return out

    runs = _run(fn, inp)
    assert all(bool(torch.isfinite(v).all()) for v in runs["zero"].values())
    assert all(bool(v.any()) for v in runs["zero"].values())
