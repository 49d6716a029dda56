"""tests/wave_attn_checker.py and the mirrors of fresnel_amd/cvs.py against the reference's fixtures W1-W4
(tests/golden/make_goldens_cvs.py), on the CPU: the checker reproduces W1 and W2 -- output, grad.x, every parameter gradient and
grad.wavelength -- within 1e-4 of the tensor's maximum in fp32 and in fp64; each of its six deliberate mistakes misses W1's output by
at least ten times that; the mirrors load W1-W4 with strict=True, reproduce them with backend "torch" and reproduce the initial state
dict under the fixture's seed bit for bit; arguments are validated and the library refuses bad shapes without a GPU."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wave_attn_checker as WC
from helpers import GOLDEN, rel_to_max
from test_attn_checker import assert_matches_attn_fixture, ref64
from test_decoder_mirror import TOL

WAVE_FIXTURES = ["cvs_W1", "cvs_W2"]
BLOCK_FIXTURES = ["cvs_W3", "cvs_W4"]
_CACHE = {}


class _Fixture(dict):
    """The arrays of an .npz, read once; `files` as numpy's NpzFile has it (test_attn_checker.py's helpers read it)."""
    files = property(lambda self: list(self))


def cvs_fixture(name):
    if name not in _CACHE:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
            _CACHE[name] = _Fixture((k, z[k]) for k in z.files)
    return _CACHE[name]


def state_dict_of(fx, dtype=torch.float32):
    return {k[3:]: torch.from_numpy(fx[k]).to(dtype) for k in fx if k.startswith("sd.")}


def run_wave(fx, attend_fn, dtype=torch.float32, device="cpu"):
    """FresnelWaveAttention around the attention -- to_qkv and to_out with the fixture's weights -- with `attend_fn(qkv, grid,
    wavelength, heads)` between them -> output, gradients {x, sd.<parameter>} of sum(out x g)."""
    heads = json.loads(str(fx["ctor"]))["heads"]
    sd = {k: v.to(device).requires_grad_(True) for k, v in state_dict_of(fx, dtype).items()}
    x = torch.from_numpy(fx["x"]).to(device, dtype).requires_grad_(True)
    Bn, C, H, W = x.shape
    qkv = F.linear(x.view(Bn, C, -1).permute(0, 2, 1), sd["to_qkv.weight"])
    out = F.linear(attend_fn(qkv, (H, W), sd["wavelength"], heads).to(dtype), sd["to_out.weight"], sd["to_out.bias"])
    out = out.permute(0, 2, 1).view(Bn, C, H, W)
    (out * torch.from_numpy(fx["g"]).to(device, dtype)).sum().backward()
    grads = {"x": x.grad}
    grads.update({"sd." + k: v.grad for k, v in sd.items()})
    return out.detach(), grads


def build_mirror(fx, dtype=torch.float32, **kw):
    from fresnel_amd import cvs
    ctor = json.loads(str(fx["ctor"]))
    module = (cvs.FresnelWaveAttention if str(fx["kind"]) == "wave" else cvs.AttentionBlock)(**ctor, **kw)
    module.load_state_dict(state_dict_of(fx), strict=True)
    module = module.eval().to(dtype)
    for sub in module.modules():   # GroupNorm32 computes in float32 whatever it is given: its parameters stay fp32 (make_goldens_cvs.py)
        if isinstance(sub, cvs.GroupNorm32):
            sub.float()
    return module


def run_mirror(module, fx, dtype=torch.float32, device="cpu"):
    x = torch.from_numpy(fx["x"]).to(device, dtype).requires_grad_(True)
    context = torch.from_numpy(fx["context"]).to(device, dtype).requires_grad_(True) if "context" in fx else None
    out = module(x) if context is None else module(x, context)
    (out * torch.from_numpy(fx["g"]).to(device, dtype)).sum().backward()
    grads = {"x": x.grad}
    if context is not None:
        grads["context"] = context.grad
    grads.update({"sd." + k: p.grad for k, p in module.named_parameters()})
    return out.detach(), grads


# ---- the checker against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", WAVE_FIXTURES)
def test_checker_reproduces_the_reference(name, dtype):
    fx = cvs_fixture(name)
    out, grads = run_wave(fx, WC.attend, dtype)
    assert "sd.wavelength" in grads and float(grads["sd.wavelength"]) != 0.0
    assert_matches_attn_fixture(fx, out, grads, name)


def test_fixtures_are_what_they_are_for():
    w1, w2, w3, w4 = (cvs_fixture(n) for n in WAVE_FIXTURES + BLOCK_FIXTURES)
    assert w1["x"].shape == (2, 64, 5, 7) and json.loads(str(w1["ctor"])) == dict(dim=64, heads=8) and float(w1["sd.wavelength"]) == np.float32(0.1)
    assert w2["x"].shape == (1, 96, 16, 16) and json.loads(str(w2["ctor"])) == dict(dim=96, heads=2) and float(w2["sd.wavelength"]) == np.float32(-0.07)
    assert w3["x"].shape == (2, 32, 4, 6) and w3["context"].shape == (2, 9, 8) and json.loads(str(w3["ctor"]))["use_fresnel"] is True
    assert w4["x"].shape == (2, 32, 4, 6) and json.loads(str(w4["ctor"]))["use_fresnel"] is False and "sd.self_attn.to_k.weight" in w4
    cap = os.path.getsize(os.path.join(GOLDEN, "attn_A1.npz"))
    for name, fx in zip(WAVE_FIXTURES + BLOCK_FIXTURES, (w1, w2, w3, w4)):
        assert 0 < rel_to_max(fx["out"], ref64(fx, "out")) < 0.1 * TOL   # the two precisions agree far inside the tolerance
        assert sorted("d64." + k for k in fx if k == "out" or k.startswith("grad.")) == sorted(k for k in fx if k.startswith("d64."))
        assert all(np.isfinite(v).all() for v in fx.values() if v.dtype.kind == "f")
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= cap
    for fx in (w1, w2, w3):   # the reference's own fp32 grad.wavelength: within a quarter of the tolerance of its fp64 value
        key = [k for k in fx if k.startswith("grad.") and k.endswith("wavelength")][0]
        assert abs(float(fx[key]) - float(ref64(fx, key))) <= 2.5e-5 * abs(float(ref64(fx, key)))


@pytest.mark.parametrize("wrong", WC.WRONG_RULES)
def test_each_wrong_rule_misses_w1(wrong):
    fx = cvs_fixture("cvs_W1")
    out, _ = run_wave(fx, lambda *a: WC.attend(*a, wrong=wrong), torch.float64)
    miss = min(rel_to_max(out.numpy(), fx["out"]), rel_to_max(out.numpy(), ref64(fx, "out")))
    print(f"{wrong}: out misses W1 by {miss:.2e}")
    assert miss >= 10 * TOL, f"{wrong}: W1 does not tell ({miss:.2e})"


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", WAVE_FIXTURES + BLOCK_FIXTURES)
def test_mirror_loads_and_reproduces_the_fixture(name, dtype):
    fx = cvs_fixture(name)
    module = build_mirror(fx, dtype)
    assert all(m.backend == "torch" for m in module.modules() if hasattr(m, "backend"))
    out, grads = run_mirror(module, fx, dtype)
    assert_matches_attn_fixture(fx, out, grads, name)


@pytest.mark.parametrize("name", WAVE_FIXTURES + BLOCK_FIXTURES)
def test_mirror_reproduces_the_initial_state_dict_bit_for_bit(name):
    from fresnel_amd import cvs
    fx = cvs_fixture(name)
    torch.manual_seed(int(fx["seed"]))
    module = (cvs.FresnelWaveAttention if str(fx["kind"]) == "wave" else cvs.AttentionBlock)(**json.loads(str(fx["ctor"])))
    sd = module.state_dict()
    assert list(sd) == [k[7:] for k in fx if k.startswith("sd0sha.")] == [k[3:] for k in fx if k.startswith("sd.")]
    for k, v in sd.items():
        assert hashlib.sha256(v.numpy().tobytes()).hexdigest() == str(fx["sd0sha." + k]), k
    # the keywords add no state, and the keys are the reference's
    twin = type(module)(**json.loads(str(fx["ctor"])), **({} if str(fx["kind"]) == "wave" else dict(attn_backend="hip")))
    assert list(twin.state_dict()) == list(sd)
    if name == "cvs_W3":
        assert {"norm1.weight", "self_attn.wavelength", "self_attn.to_qkv.weight", "self_attn.to_out.bias", "norm2.bias",
                "cross_attn.to_q.weight", "cross_attn.to_k.weight", "cross_attn.to_v.weight", "cross_attn.to_out.weight"} <= set(sd)
        assert twin.self_attn.backend == "hip" and twin.cross_attn.backend == "hip"


def test_function_with_backend_torch_is_the_checker():
    from fresnel_amd import cvs
    fx = cvs_fixture("cvs_W1")
    a, ga = run_wave(fx, lambda *args: cvs.fresnel_wave_attention(*args), torch.float64)
    b, gb = run_wave(fx, WC.attend, torch.float64)
    # not to fp64 rounding: the reference's positions are `.float()`, so its distances, phases and cosines are fp32 values in an
    # fp64 run too (a 0-dim fp64 wavelength does not promote them), where the checker forms them in the run's dtype
    assert rel_to_max(a.numpy(), b.numpy()) <= 0.1 * TOL
    for k in ga:
        assert rel_to_max(ga[k].numpy(), gb[k].numpy()) <= 0.1 * TOL, k


# ---- validation -------------------------------------------------------------------------------------------------------------------------
def test_arguments_are_validated_without_a_gpu():
    from fresnel_amd import _binding, cvs
    qkv, wl = torch.randn(2, 35, 3 * 16), torch.tensor(0.1)
    assert cvs.fresnel_wave_attention(qkv, (5, 7), wl, 4).shape == (2, 35, 16)
    with pytest.raises(ValueError, match="attn_backend"):
        cvs.fresnel_wave_attention(qkv, (5, 7), wl, 4, backend="triton")
    with pytest.raises(ValueError, match="attn_backend"):
        cvs.AttentionBlock(32, 8, attn_backend="triton")
    for grid in ((5, 8), (7, 6), (35,), (0, 35)):
        with pytest.raises(ValueError, match="grid"):
            cvs.fresnel_wave_attention(qkv, grid, wl, 4)
    with pytest.raises(ValueError, match="num_heads"):
        cvs.fresnel_wave_attention(qkv, (5, 7), wl, 0)
    with pytest.raises(ValueError, match="qkv must be"):
        cvs.fresnel_wave_attention(qkv, (5, 7), wl, 5)
    with pytest.raises(ValueError, match="wavelength"):
        cvs.fresnel_wave_attention(qkv, (5, 7), torch.ones(2), 4)
    # the hip backend's limits are refused before anything is launched -- and before the device is looked at
    with pytest.raises(ValueError, match="head dimension 129"):
        cvs.fresnel_wave_attention(torch.randn(1, 4, 3 * 129), (2, 2), wl, 1, backend="hip")
    with pytest.raises(ValueError, match="beyond the supported 4096"):
        cvs.fresnel_wave_attention(torch.randn(1, 4097, 3), (1, 4097), wl, 1, backend="hip")
    with pytest.raises(ValueError, match="contiguous"):
        cvs.fresnel_wave_attention(torch.randn(2, 3 * 16, 35).transpose(1, 2), (5, 7), wl, 4, backend="hip")
    with pytest.raises(_binding.FgsError, match="no CPU fallback"):
        cvs.fresnel_wave_attention(qkv, (5, 7), wl, 4, backend="hip")
    for module, args in ((cvs.FresnelWaveAttention(16, heads=4), (torch.randn(2, 16, 5, 7),)),
                         (cvs.CrossAttention(16, 8, heads=2, dim_head=4), (torch.randn(2, 16, 5, 7), torch.randn(2, 3, 8))),
                         (cvs.AttentionBlock(32, 8, attn_backend="hip"), (torch.randn(2, 32, 5, 7), torch.randn(2, 3, 8)))):
        module.backend = "hip"
        with pytest.raises(_binding.FgsError, match="no CPU fallback"):
            module(*args)
    module = cvs.FresnelWaveAttention(16, heads=4)
    module.backend = "triton"
    with pytest.raises(ValueError, match="attn_backend"):
        module(torch.randn(2, 16, 5, 7))


def test_the_library_refuses_bad_wave_attention_shapes_without_a_gpu():
    """rc = FGS_EINVAL / FGS_EUNSUPPORTED with a message, before anything touches the device."""
    from fresnel_amd import _binding as B
    # saved: one float per (b, h, n), rounded up to 256 B; scratch: the same plus one double per (b, h, query block), rounded up
    assert B.sizes("fgs_wave_attn_workspace_bytes", 2, 5, 7, 8, 8) == (2304, 2304 + 256)
    assert B.sizes("fgs_wave_attn_workspace_bytes", 4, 32, 32, 8, 64) == (131072, 131072 + 2048)
    assert B.sizes("fgs_wave_attn_workspace_bytes", 1, 64, 64, 1, 128) == (16384, 16384 + 256)        # the limit itself is supported
    for dims, match in (((2, 5, 7, 8, 129), "head_dim"), ((0, 5, 7, 8, 8), "invalid dims"), ((2, 5, 0, 8, 8), "invalid dims"),
                        ((2, 0, 7, 8, 8), "invalid dims"), ((1, 64, 65, 1, 8), "beyond the supported 4096"),
                        ((1, 1 << 16, 1 << 16, 1, 8), "beyond the supported 4096"), ((1 << 12, 64, 64, 1 << 7, 8), "beyond the supported size")):
        with pytest.raises(B.FgsError, match=match):
            B.sizes("fgs_wave_attn_workspace_bytes", *dims)
    lib = B.load()
    assert lib.fgs_wave_attn_forward(1, 2, 2, 1, 8, 1.0, None, None, None, None, None) == -1
    assert b"null" in lib.fgs_last_error()
    assert lib.fgs_wave_attn_backward(1, 2, 2, 1, 8, 1.0, *([None] * 9)) == -1
    assert b"null" in lib.fgs_last_error()
    assert lib.fgs_wave_attn_forward(1, 2, 2, 1, 8, float("inf"), None, None, None, None, None) == -1
    assert b"scale" in lib.fgs_last_error()
    assert lib.fgs_wave_attn_forward(1, 2, 2, 1, 200, 1.0, None, None, None, None, None) == -3
    assert b"head_dim = 200" in lib.fgs_last_error()
    from test_call_layer import _header, header_defines
    assert B.FGS_WAVE_ATTN_MAX_TOKENS == header_defines(_header())["FGS_WAVE_ATTN_MAX_TOKENS"]
