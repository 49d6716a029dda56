"""The fused GroupNorm -> SiLU (csrc/fgs_gn_silu.hip, fresnel_amd.cvs.group_norm_act backend "hip") on the GPU: parity with
tests/gn_checker.py (fp64, CPU) at the seams, with and without channel_bias, for act 1 and act 0; the offset, small-scale and
degenerate-span cases; NaN containment; repeatability, batch independence and capture; the limits; the reference's fixtures R1, R2 and U1
through the modules with norm_backend "hip"; the memory a ResBlock's training step no longer keeps.  The tolerance is 1e-4 of the
tensor's maximum (tests/test_decoder_mirror.py) throughout.

SEAMS, as x shapes (B, C, H, W) at 32 groups.  S = FGS_GN_SEGMENT is the kernels' one cut: a wave owns up to S consecutive floats of one
channel row, longer rows are cut at multiples of S; rows of HW % 4 == 0 are read as float4, all others scalar:

    (2, 64, 5, 7)       span 70, scalar          | (2, 96, 5, 7)   span 105: odd, groups start at misaligned offsets, scalar
    (3, 96, 1, 3)       rows of 3                | (2, 160, 3, 43) five channels per group, rows of 129
    (2, 64, 1, 2)       span 4                   | (1, 1024, 16, 16)  32 channels per group (the decoder's concatenation), float4
    (1, 64, 1, S)       exactly one segment, float4, the unguarded loop
    (1, 64, 1, S + 1)   one segment + 1 element: a last segment of ONE element, scalar
    (1, 64, 1, S + 4)   a last segment of one float4
    (1, 64, 1, 2 S)     two full segments        | (1, 64, 1, 16385)  four segments + 1 element
    (1, 128, 256, 256)  once: the workload's own span, 16 segments a row, 64 pairs folded per group
"""

import pytest
import torch

import gn_checker as GC
from test_cvs_unet_mirror import (RES_FIXTURES, assert_matches_unet_fixture, build_res, build_synth, run_res, run_synth, unet_fixture)
from test_decoder_mirror import TOL
from test_gn_checker import TENSORS, distances, gn_case, run_checker
from test_hip_wave_attn import _Calls, _dev, _same_bits

from fresnel_amd import _binding as B

gpu = pytest.mark.gpu
S = B.FGS_GN_SEGMENT
EPS = 1e-5


def _hip(case, act, dev, eps=EPS):
    from fresnel_amd.cvs import group_norm_act
    leaves = {k: case[k].to(dev).requires_grad_(True) for k in ("x", "weight", "bias", "channel_bias") if case[k] is not None}
    out = group_norm_act(leaves["x"], case["groups"], leaves["weight"], leaves["bias"], channel_bias=leaves.get("channel_bias"),
                         act="silu" if act else "none", eps=eps, backend="hip")
    out.backward(case["g_out"].to(dev))
    torch.cuda.synchronize()
    return dict(out=out.detach().cpu(), g_x=leaves["x"].grad.cpu(), g_weight=leaves["weight"].grad.cpu(), g_bias=leaves["bias"].grad.cpu(),
                g_channel_bias=leaves["channel_bias"].grad.cpu() if "channel_bias" in leaves else None)


def _compare(tag, got, want, keys=TENSORS):
    for k, e in distances(got, want).items():
        if k in keys:
            print(f"{tag}: {k} {e:.2e}")
            assert e <= TOL, f"{tag}: {k} is {e:.2e} of its maximum away from the fp64 checker"


def _all_modes(shape, seed, dev, **kw):
    """with and without channel_bias, act 1 and act 0, against the fp64 checker"""
    for with_bias in (True, False):
        case = gn_case(shape, 32, seed, with_bias, **kw)
        for act in (1, 0):
            got = _hip(case, act, dev)
            assert (got["g_channel_bias"] is None) == (not with_bias)
            _compare(f"{shape} {'cb' if with_bias else 'nocb'} act {act}", got, run_checker(case, act))


# ---- parity with the checker, at the seams ---------------------------------------------------------------------------------------------
SEAMS = [(2, 64, 5, 7), (2, 96, 5, 7), (3, 96, 1, 3), (2, 160, 3, 43), (2, 64, 1, 2), (1, 1024, 16, 16),
         (1, 64, 1, S), (1, 64, 1, S + 1), (1, 64, 1, S + 4), (1, 64, 1, 2 * S), (1, 64, 1, 16385)]
assert 16385 == 4 * S + 1


@gpu
@pytest.mark.parametrize("shape", SEAMS, ids=["x".join(map(str, s)) for s in SEAMS])
def test_parity_with_the_checker_at_the_seams(shape):
    _all_modes(shape, 5000 + sum(shape), _dev())


@gpu
def test_parity_at_the_workloads_own_span():
    shape = (1, 128, 256, 256)
    case = gn_case(shape, 32, 5100, True)
    _compare(f"{shape}", _hip(case, 1, _dev()), run_checker(case, 1))


# ---- special cases ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_mean_thirty_deviations_from_zero():
    """x = 30 + randn: E[u^2] - mean^2 in fp32 loses the variance's digits (900 against 1); the two-pass moments do not."""
    _all_modes((1, 64, 16, 16), 5200, _dev(), offset=30.0)


@gpu
def test_a_spread_that_eps_dominates():
    """x = 1e-3 randn: var = 1e-6 against eps = 1e-5."""
    _all_modes((1, 64, 16, 16), 5300, _dev(), scale=1e-3)


def _weight_gy_max(case, act):
    t = {k: (v.double() if torch.is_tensor(v) else v) for k, v in case.items()}
    _, y, _, _ = GC._parts(t["x"], t["groups"], t["weight"], t["bias"], t["channel_bias"], EPS, None)
    g3 = t["g_out"].reshape(y.shape)
    s = torch.sigmoid(y)
    g_y = g3 * s * (1 + y * (1 - s)) if act else g3
    return float((t["weight"][None, :, None] * g_y).abs().max())


DEGENERATE = [((2, 32, 5, 7), ("g_channel_bias",)),                  # one channel per group: g_channel_bias is mathematically zero
              ((2, 32, 1, 1), ("g_x", "g_channel_bias")),            # span 1: g_x is zero as well
              ((2, 64, 1, 1), ("g_x", "g_channel_bias"))]            # span 2: g_x is a cancellation (torch's own fp32 run: 1.7e-4 away)


@gpu
@pytest.mark.parametrize("shape,cancelling", DEGENERATE, ids=["x".join(map(str, s)) for s, _ in DEGENERATE])
def test_degenerate_spans(shape, cancelling):
    """Not tolerance cases: what cancels is required to be finite and within TOL eps^-1/2 max|weight g_y| of zero -- the bound of a
    difference of two equal terms under rstd <= eps^-1/2; everything else is judged by TOL as usual.

    Span 2 cancels only where the pair's spread is far above sqrt(eps): exactly, g_x = +-rstd^3 eps (w1 g_y1 - w2 g_y2) / 2, which
    for a pair 0.02 apart is 10 (w1 g_y1 - w2 g_y2) / 2 -- a gradient, not a cancellation (plain randn inputs hold such pairs: the
    kernel then returns 3.7 where the bound is 0.07, and so does the fp64 checker).  So the span-2 case draws its pairs at least 4
    apart (channels alternately above +2 and below -2), where rstd^3 eps < 1e-6 and the statement holds."""
    dev = _dev()
    case = gn_case(shape, 32, 5400 + sum(shape), True)
    if shape == (2, 64, 1, 1):
        sign = torch.tensor([1.0, -1.0]).repeat(32)[None, :, None, None]
        case["x"] = sign * (2.0 + case["x"].abs())
        case["channel_bias"] = 0.25 * case["channel_bias"]
    for act in (1, 0):
        got, want = _hip(case, act, dev), run_checker(case, act)
        _compare(f"{shape} act {act}", got, want, keys=[k for k in TENSORS if k not in cancelling])
        bound = TOL * EPS ** -0.5 * _weight_gy_max(case, act)
        for k in cancelling:
            worst = float(got[k].abs().max())
            print(f"{shape} act {act}: |{k}| max {worst:.2e}, bound {bound:.2e}")
            assert bool(torch.isfinite(got[k]).all()) and worst <= bound, k
        if shape == (2, 32, 1, 1):   # a one-element group normalises to zero: the output is the activated bias
            bias = case["bias"].double()
            want_out = (bias * torch.sigmoid(bias) if act else bias)[None, :, None, None].expand(shape)
            assert float((got["out"].double() - want_out).abs().max()) <= TOL * float(want_out.abs().max())


# ---- NaN -------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", [(2, 96, 5, 7), (2, 64, 1, S + 4)], ids=["2x96x5x7", "split"])
def test_one_nan_stays_in_its_group(shape):
    dev = _dev()
    case = gn_case(shape, 32, 5500, True)
    clean = _hip(case, 1, dev)
    Bn, C = shape[:2]
    cpg = C // 32
    b, grp = 1, 1
    dirty_case = dict(case, x=case["x"].clone())
    dirty_case["x"].reshape(Bn, C, -1)[b, grp * cpg + cpg - 1, -1] = float("nan")   # the group's last element
    dirty = _hip(dirty_case, 1, dev)
    for k in ("out", "g_x"):
        c, d = (t[k].reshape(Bn, 32, -1) for t in (clean, dirty))
        assert bool(torch.isnan(d[b, grp]).all()), f"{k}: the group of the NaN"
        rest = torch.ones(Bn, 32, dtype=torch.bool)
        rest[b, grp] = False
        assert _same_bits(d[rest], c[rest]), f"{k}: another group moved"
    cb_c, cb_d = (t["g_channel_bias"].reshape(Bn, 32, cpg) for t in (clean, dirty))
    assert bool(torch.isnan(cb_d[b, grp]).all()) and _same_bits(cb_d[rest], cb_c[rest])
    for k in ("g_weight", "g_bias"):   # as torch: the NaN reaches the parameters of its group's channels, and only those
        c, d = (t[k].reshape(32, cpg) for t in (clean, dirty))
        others = torch.arange(32) != grp
        assert bool(torch.isnan(d[grp]).all()) and _same_bits(d[others], c[others])
    assert all(bool(torch.isfinite(v).all()) for v in clean.values())


# ---- repeatability and capture ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", [(3, 96, 5, 7), (3, 64, 1, S + 4)], ids=["3x96x5x7", "split"])
def test_two_calls_and_batch_against_single_images(shape):
    dev = _dev()
    case = gn_case(shape, 32, 5600, True)
    a, b = _hip(case, 1, dev), _hip(case, 1, dev)
    assert all(_same_bits(a[k], b[k]) for k in a)
    total = {k: 0.0 for k in ("g_weight", "g_bias")}
    for i in range(shape[0]):
        one = _hip({k: (v[i:i + 1] if k in ("x", "channel_bias", "g_out") else v) for k, v in case.items()}, 1, dev)
        assert all(_same_bits(a[k][i:i + 1], one[k]) for k in ("out", "g_x", "g_channel_bias")), f"image {i} depends on its batch"
        for k in total:
            total[k] = total[k] + one[k].double()
    for k, v in total.items():
        assert float((a[k].double() - v).abs().max()) <= TOL * float(v.abs().max()), k


@gpu
def test_captured_graph_follows_inputs_changed_in_place():
    from fresnel_amd.cvs import group_norm_act
    dev = _dev()
    case = gn_case((2, 96, 5, 7), 32, 5700, True)
    other = gn_case((2, 96, 5, 7), 32, 5701, True)
    leaves = {k: case[k].to(dev).requires_grad_(True) for k in ("x", "weight", "bias", "channel_bias")}
    up = case["g_out"].to(dev)

    def step():
        out = group_norm_act(leaves["x"], 32, leaves["weight"], leaves["bias"], channel_bias=leaves["channel_bias"], backend="hip")
        out.backward(up)
        return out

    def eager(values):
        with torch.no_grad():
            for k, t in leaves.items():
                t.copy_(values[k])
        for t in leaves.values():
            t.grad = None
        out = step()
        torch.cuda.synchronize()
        return [out.detach().clone()] + [t.grad.detach().clone() for t in leaves.values()]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        want_old = eager(case)
        want_new = eager(other)
        eager(case)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not torch.equal(want_old[0], want_new[0])
    for t in leaves.values():
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        for k, t in leaves.items():
            t.copy_(other[k])
            t.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for name, x, y in zip(["out"] + ["g_" + k for k in leaves], [captured] + [t.grad for t in leaves.values()], want_new):
        assert _same_bits(x, y), f"{name}: the replay does not follow the inputs"


# ---- limits ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_limits_raise_without_a_launch():
    from fresnel_amd import cvs
    dev = _dev()
    w, b = torch.ones(32, device=dev), torch.zeros(32, device=dev)
    with _Calls() as calls:
        with pytest.raises(ValueError, match="beyond the supported size"):
            cvs.group_norm_act(torch.zeros(1, device=dev).expand(2, 32, 1 << 25), 32, w, b, backend="hip")   # 2^31 elements, no memory
        with pytest.raises(ValueError, match="num_groups"):
            cvs.group_norm_act(torch.zeros(2, 32, 4, device=dev), 5, w, b, backend="hip")
        with pytest.raises(ValueError, match="eps"):
            cvs.group_norm_act(torch.zeros(2, 32, 4, device=dev), 32, w, b, eps=0.0, backend="hip")
        with pytest.raises(B.FgsError, match="no CPU fallback"):
            cvs.group_norm_act(torch.zeros(2, 32, 4, device=dev), 32, w.cpu(), b, backend="hip")
        assert calls.names == []
        # the library's own refusal (what the wrapper's checks stand in front of), as a clean error
        buf = torch.empty(4096, device=dev)
        with pytest.raises(B.FgsError, match="invalid dims"):
            calls.real(dev, "fgs_gn_silu_forward", 1, 48, 4, 32, 1, 1e-5, buf, None, buf, buf, buf, buf, buf)
        with pytest.raises(B.FgsError, match="aligned"):
            calls.real(dev, "fgs_gn_silu_forward", 1, 32, 4, 32, 1, 1e-5, buf[1:], None, buf, buf, buf, buf, buf)


# ---- the modules ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", RES_FIXTURES)
def test_resblock_fixture_with_norm_backend_hip(name):
    dev = _dev()
    fx = unet_fixture(name)
    module = build_res(fx).to(dev)
    module.norm_backend = "hip"
    x, t_emb = torch.from_numpy(fx["x"]).to(dev), torch.from_numpy(fx["t_emb"]).to(dev)
    with _Calls() as calls, torch.no_grad():
        module(x, t_emb)
    assert calls.names == ["fgs_gn_silu_forward"] * 2   # norm1 -> SiLU; conv1 + embedding -> norm2 -> SiLU
    assert_matches_unet_fixture(fx, run_res(module, fx, device=dev), name + " (hip)")


@gpu
@pytest.mark.parametrize("attn_backend", ["torch", "hip"])
def test_synthesizer_fixture_with_norm_backend_hip(attn_backend):
    dev = _dev()
    fx = unet_fixture("cvs_U1")
    module = build_synth(fx, norm_backend="hip", attn_backend=attn_backend).to(dev)
    with _Calls() as calls:
        res = run_synth(module, fx, device=dev)
    # 8 ResBlocks x 2, 3 AttentionBlocks x 2, out_conv
    assert calls.names.count("fgs_gn_silu_forward") == 23 == calls.names.count("fgs_gn_silu_backward")
    assert ("fgs_wave_attn_forward" in calls.names) == (attn_backend == "hip")
    assert_matches_unet_fixture(fx, res, f"cvs_U1 (norm hip, attn {attn_backend})")


# ---- memory ----------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_resblock_training_step_keeps_two_activations_fewer():
    """ResBlock(128, 128, 256) on (1, 128, 192, 192): one activation is T = 18.9 MB.  With "torch" the two normalised tensors (and
    the sum conv1 + embedding) are kept for the backward; with "hip" they never exist.  Required: the peak rises by at least T less
    (two tensors fewer; one T is the margin for the allocator)."""
    from fresnel_amd import cvs
    dev = _dev()
    torch.manual_seed(5800)
    module = cvs.ResBlock(128, 128, 256).to(dev).train()
    x0, t_emb = torch.randn(1, 128, 192, 192, device=dev), torch.randn(1, 256, device=dev)
    T = x0.numel() * 4
    rise = {}
    for backend in ("hip", "torch", "hip", "torch"):   # (the first pair warms MIOpen's workspaces and the allocator)
        module.norm_backend = backend
        module.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        module(x, t_emb).sum().backward()
        torch.cuda.synchronize()
        rise[backend] = torch.cuda.max_memory_allocated() - base
        del x
    print(f"memory rise: hip {rise['hip'] / 2 ** 20:.1f} MiB, torch {rise['torch'] / 2 ** 20:.1f} MiB, one activation {T / 2 ** 20:.1f} MiB")
    assert rise["hip"] <= rise["torch"] - T, rise
