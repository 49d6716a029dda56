"""Workspace and output-buffer hygiene of the NCA entry points (fgs_nca_workspace_bytes, fgs_nca_perceive_forward / _backward,
fgs_nca_update_forward / _backward), through the product wrappers (fresnel_amd.decoder.nca_perceive / nca_update, backend "hip"):
guard bytes around every buffer and the three fill patterns (tests/workspace_guard.py).  Asserts A (guards intact after forward
and backward), B (outputs and gradients bitwise identical under every fill pattern and unpatched: every element is written --
the rows of points that are nobody's neighbour included -- and nothing, the update's scratch included, is read before it is
written) and C (inputs untouched) of tests/test_workspace_hygiene.py."""
import pytest
import torch

import workspace_guard as WG
from test_hip_nca import _dev
from test_workspace_hygiene import _leaf, _sync_check

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("Bn,N,k,D", [(3, 377, 6, 16), (2, 65, 16, 7), (1, 4096, 2, 6)], ids=["flagship", "odd_d_second_block", "largest_n"])
def test_perceive_buffers(Bn, N, k, D):
    from fresnel_amd import decoder
    dev = _dev()
    g = torch.Generator().manual_seed(700 + N)
    inp = dict(state=torch.randn(Bn, N, D, generator=g).to(dev), g_perception=torch.randn(Bn, N, (k + 1) * D, generator=g).to(dev))

    def fn(guard):
        state = _leaf(inp["state"])
        perception, nbr = decoder.nca_perceive(state, k, backend="hip")
        _sync_check(guard, "after the forward")
        perception.backward(inp["g_perception"])
        _sync_check(guard, "after the backward")
        return dict(perception=perception.detach(), neighbors=nbr, grad_state=state.grad)

    runs = WG.run_patterns(fn, inp, [decoder])
    zero = runs["zero"]
    assert bool(torch.isfinite(zero["perception"]).all()) and bool(torch.isfinite(zero["grad_state"]).all())
    assert int(zero["neighbors"].min()) >= 0 and int(zero["neighbors"].max()) < N


@gpu
@pytest.mark.parametrize("Bn,N,D,masked", [(3, 377, 16, True), (2, 65, 7, True), (5, 4096, 64, False)],
                         ids=["flagship_train", "odd_d_train", "grid_stride_eval"])
def test_update_buffers(Bn, N, D, masked):
    from fresnel_amd import decoder
    dev = _dev()
    g = torch.Generator().manual_seed(800 + N)
    inp = dict(state=torch.randn(Bn, N, D, generator=g).to(dev), delta=torch.randn(Bn, N, D, generator=g).to(dev),
               step_size=torch.tensor(0.21).to(dev), g_new=torch.randn(Bn, N, D, generator=g).to(dev))
    if masked:
        inp["uniform"] = torch.rand(Bn, N, 1, generator=g).to(dev)

    def fn(guard):
        t = {k: _leaf(inp[k]) for k in ("state", "delta", "step_size")}
        new = decoder.nca_update(t["state"], t["delta"], t["step_size"], inp.get("uniform"), 0.5, backend="hip")
        _sync_check(guard, "after the forward")
        new.backward(inp["g_new"])
        _sync_check(guard, "after the backward")
        return dict(new_state=new.detach(), grad_delta=t["delta"].grad, grad_step_size=t["step_size"].grad.reshape(1))

    runs = WG.run_patterns(fn, inp, [decoder])
    assert all(bool(torch.isfinite(v).all()) and bool(v.any()) for v in runs["zero"].values())
