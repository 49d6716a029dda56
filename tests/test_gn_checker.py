"""tests/gn_checker.py and `fresnel_amd.cvs.group_norm_act` on the CPU: the checker -- forward and written-out backward -- agrees
with torch's op sequence add -> F.group_norm -> F.silu and its autograd within 1e-4 of the tensor's maximum (TOL of
tests/test_decoder_mirror.py) in fp32 and fp64; each of its five deliberate mistakes misses some tensor by at least ten times that;
backend "torch" IS the op sequence, bit for bit; arguments are validated and the library refuses bad shapes without a GPU."""
import math

import pytest
import torch

import gn_checker as GC
from helpers import rel_to_max
from test_decoder_mirror import TOL

TENSORS = ("out", "g_x", "g_channel_bias", "g_weight", "g_bias")


def gn_case(shape, groups, seed, with_bias=True, offset=0.0, scale=1.0):
    """Random x, norm weight / bias, channel bias and upstream gradient for x of `shape` = (B, C, ...)."""
    g = torch.Generator().manual_seed(seed)
    Bn, C = shape[:2]
    return dict(x=offset + scale * torch.randn(*shape, generator=g), weight=1.0 + 0.3 * torch.randn(C, generator=g),
                bias=0.3 * torch.randn(C, generator=g), channel_bias=scale * 0.5 * torch.randn(Bn, C, generator=g) if with_bias else None,
                g_out=torch.randn(*shape, generator=g), groups=groups)


def run_checker(case, act, dtype=torch.float64, eps=1e-5, wrong=None):
    t = {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in case.items()}
    args = (t["x"], t["groups"], t["weight"], t["bias"])
    res = GC.backward(*args, t["g_out"], channel_bias=t["channel_bias"], act=act, eps=eps, wrong=wrong)
    res["out"] = GC.forward(*args, channel_bias=t["channel_bias"], act=act, eps=eps, wrong=wrong)
    return res


def run_autograd(case, act, fn, dtype=torch.float32, device="cpu", eps=1e-5):
    """fn(x, groups, weight, bias, channel_bias, act, eps) -> out, differentiated by autograd against the case's g_out."""
    leaves = {k: case[k].to(device, dtype).requires_grad_(True) for k in ("x", "weight", "bias", "channel_bias") if case[k] is not None}
    out = fn(leaves["x"], case["groups"], leaves["weight"], leaves["bias"], leaves.get("channel_bias"), act, eps)
    out.backward(case["g_out"].to(device, dtype))
    return dict(out=out.detach(), g_x=leaves["x"].grad, g_channel_bias=leaves["channel_bias"].grad if "channel_bias" in leaves else None,
                g_weight=leaves["weight"].grad, g_bias=leaves["bias"].grad)


def distances(got, want):
    return {k: rel_to_max(got[k].detach().cpu().double().numpy(), want[k].detach().cpu().double().numpy())
            for k in TENSORS if want[k] is not None}


CASES = [((2, 64, 5, 7), 32, True), ((2, 96, 5, 7), 32, True), ((3, 96, 1, 3), 32, False), ((1, 128, 16), 32, True), ((2, 12, 4, 4), 3, True)]


@pytest.mark.parametrize("act", [1, 0], ids=["silu", "none"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("shape,groups,with_bias", CASES, ids=[f"{'x'.join(map(str, s))}-g{g}-{'cb' if b else 'nocb'}" for s, g, b in CASES])
def test_checker_agrees_with_the_op_sequence(shape, groups, with_bias, dtype, act):
    case = gn_case(shape, groups, 4000 + sum(shape), with_bias)
    want = run_autograd(case, act, lambda x, G, w, b, cb, a, eps: GC.op_sequence(x, G, w, b, cb, a, eps), dtype)
    got = run_checker(case, act, dtype)
    assert (got["g_channel_bias"] is None) == (not with_bias)
    for k, e in distances(got, want).items():
        print(f"{shape} {dtype} act {act}: {k} {e:.2e}")
        assert e <= TOL, f"{k}: the checker is {e:.2e} of the maximum away from the op sequence"


@pytest.mark.parametrize("wrong", GC.WRONG_RULES)
def test_each_wrong_rule_misses(wrong):
    """(2, 96, 5, 7): m = 105 (so the unbiased variance differs by 1 / 105), three channels per group (so strided groups differ),
    x spread 0.02 (so that eps is a tenth of the variance and its place shows)."""
    case = gn_case((2, 96, 5, 7), 32, 4100, scale=0.02)
    right, bad = run_checker(case, 1), run_checker(case, 1, wrong=wrong)
    miss = max(distances(bad, right).values())
    print(f"{wrong}: misses by {miss:.2e}")
    assert miss >= 10 * TOL, f"{wrong}: the case does not tell ({miss:.2e})"
    if wrong == "silu_grad_short":
        assert distances(bad, right)["out"] == 0.0   # a mistake of the backward alone


@pytest.mark.parametrize("act", ["silu", "none"])
@pytest.mark.parametrize("with_bias", [True, False], ids=["cb", "nocb"])
def test_backend_torch_is_the_op_sequence_bit_for_bit(with_bias, act):
    from fresnel_amd import cvs
    case = gn_case((2, 96, 5, 7), 32, 4200, with_bias)
    a = run_autograd(case, act, lambda x, G, w, b, cb, a_, eps: cvs.group_norm_act(x, G, w, b, channel_bias=cb, act=a_, eps=eps), torch.float32)
    b = run_autograd(case, int(act == "silu"), lambda x, G, w, b_, cb, a_, eps: GC.op_sequence(x, G, w, b_, cb, a_, eps), torch.float32)
    for k in TENSORS:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k
    # any dtype: computed in float32, returned in x's dtype
    half = cvs.group_norm_act(case["x"].to(torch.float64), 32, case["weight"], case["bias"], act=act)
    assert half.dtype is torch.float64 and torch.equal(half, cvs.group_norm_act(case["x"], 32, case["weight"], case["bias"], act=act).double())


def test_arguments_are_validated_without_a_gpu():
    from fresnel_amd import _binding, cvs
    x, w, b = torch.randn(2, 64, 5, 7), torch.ones(64), torch.zeros(64)
    assert cvs.group_norm_act(x, 32, w, b).shape == x.shape
    for kw, match in ((dict(backend="triton"), "norm_backend"), (dict(act="relu"), "act"), (dict(eps=0.0), "eps"), (dict(eps=float("nan")), "eps"),
                      (dict(eps=-1e-5), "eps"), (dict(channel_bias=torch.zeros(2, 63)), "channel_bias"), (dict(channel_bias=torch.zeros(64)), "channel_bias")):
        with pytest.raises(ValueError, match=match):
            cvs.group_norm_act(x, 32, w, b, **kw)
    for groups in (0, 5, 2.5, True):
        with pytest.raises(ValueError, match="num_groups"):
            cvs.group_norm_act(x, groups, w, b)
    with pytest.raises(ValueError, match="x must be"):
        cvs.group_norm_act(torch.randn(64), 32, w, b)
    with pytest.raises(ValueError, match="x must be"):
        cvs.group_norm_act(torch.randn(2, 64, 0), 32, w, b)
    with pytest.raises(ValueError, match="weight"):
        cvs.group_norm_act(x, 32, torch.ones(32), b)
    with pytest.raises(ValueError, match="bias"):
        cvs.group_norm_act(x, 32, w, None)
    # the hip backend never falls back
    with pytest.raises(_binding.FgsError, match="no CPU fallback"):
        cvs.group_norm_act(x, 32, w, b, backend="hip")
    for module, args in ((cvs.ResBlock(32, 64, 16), (torch.randn(2, 32, 5, 7), torch.randn(2, 16))),
                         (cvs.AttentionBlock(32, 8, norm_backend="hip"), (torch.randn(2, 32, 5, 7), torch.randn(2, 3, 8)))):
        module.norm_backend = "hip"
        with pytest.raises(_binding.FgsError, match="no CPU fallback"):
            module(*args)
        module.norm_backend = "triton"
        with pytest.raises(ValueError, match="norm_backend"):
            module(*args)
    with pytest.raises(ValueError, match="norm_backend"):
        cvs.AttentionBlock(32, 8, norm_backend="triton")
    with pytest.raises(ValueError, match="norm_backend"):
        cvs.ConsistencyUNet(cvs.CVSConfig(image_size=8, base_channels=32, channel_mult=(1,), num_res_blocks=1), norm_backend="triton")


def test_the_library_refuses_bad_group_norm_shapes_without_a_gpu():
    """rc = FGS_EINVAL / FGS_EUNSUPPORTED with a message, before anything touches the device."""
    from fresnel_amd import _binding as B
    S = B.FGS_GN_SEGMENT
    # saved: (mean, rstd) per (b, group); scratch: 24 bytes per segment, 24 per (b, c), 8 per (b, group); each rounded up to 256
    assert B.sizes("fgs_gn_silu_workspace_bytes", 2, 64, 35, 32) == (512, 24 * 128 + 24 * 128 + 512)
    assert B.sizes("fgs_gn_silu_workspace_bytes", 4, 128, 65536, 32) == (1024, 24 * 512 * (65536 // S) + 24 * 512 + 1024)
    assert B.sizes("fgs_gn_silu_workspace_bytes", 1, 32, S + 1, 32)[1] == 24 * 64 + 24 * 32 + 256   # one float over: two segments a row
    for dims, match in (((0, 64, 35, 32), "invalid dims"), ((2, 0, 35, 32), "invalid dims"), ((2, 64, 0, 32), "invalid dims"),
                        ((2, 64, 35, 0), "invalid dims"), ((2, 64, 35, 48), "invalid dims"), ((2, 48, 35, 32), "invalid dims"),
                        ((1 << 10, 1 << 10, 1 << 11, 32), "beyond the supported size")):
        with pytest.raises(B.FgsError, match=match):
            B.sizes("fgs_gn_silu_workspace_bytes", *dims)
    lib = B.load()
    fwd, bwd = [None] * 8, [None] * 12
    assert lib.fgs_gn_silu_forward(2, 64, 35, 32, 1, 1e-5, *fwd) == -1
    assert b"null" in lib.fgs_last_error()
    assert lib.fgs_gn_silu_backward(2, 64, 35, 32, 1, 1e-5, *bwd) == -1
    assert b"null" in lib.fgs_last_error()
    for eps in (0.0, -1e-5, float("inf"), float("nan")):
        assert lib.fgs_gn_silu_forward(2, 64, 35, 32, 1, eps, *fwd) == -1
        assert b"eps" in lib.fgs_last_error()
        assert lib.fgs_gn_silu_backward(2, 64, 35, 32, 1, eps, *bwd) == -1
        assert b"eps" in lib.fgs_last_error()
    assert lib.fgs_gn_silu_forward(2, 64, 35, 32, 2, 1e-5, *fwd) == -1
    assert b"act" in lib.fgs_last_error()
    assert lib.fgs_gn_silu_forward(2, 64, 35, 48, 1, 1e-5, *fwd) == -1
    assert b"invalid dims" in lib.fgs_last_error()
    assert lib.fgs_gn_silu_forward(1 << 10, 1 << 10, 1 << 11, 32, 1, 1e-5, *fwd) == -3
    assert b"beyond the supported size" in lib.fgs_last_error()
    # a pointer that is not 16-byte aligned is refused by its value alone (nothing is read)
    assert lib.fgs_gn_silu_forward(1, 32, 4, 32, 1, 1e-5, 4100, None, 4096, 4096, 4096, 4096, 4096, None) == -1
    assert b"aligned" in lib.fgs_last_error()
    from test_call_layer import _header, header_defines
    assert B.FGS_GN_SEGMENT == header_defines(_header())["FGS_GN_SEGMENT"]
    assert math.log2(S) == int(math.log2(S)) and S % 256 == 0
