"""The fused cross-attention (csrc/fgs_attn.hip, fresnel_amd.slat.cross_attention backend "hip") on the GPU: the reference's fixtures
A1-A3 and S1, S2, S4 through the kernels, random parity with tests/attn_checker.py (fp64, CPU) at the seams of the query block, the
key tile and the compiled head widths, the online softmax's seams, masked rows, the NaN rule, dropout against the stated keep rule,
repeatability, capture, limits, memory, and a distillation step with head, match and attention on "hip".  The tolerance is 1e-4 of
the tensor's maximum (tests/test_decoder_mirror.py) throughout."""
import json

import numpy as np
import pytest
import torch

import attn_checker as AC
from helpers import rel_to_max
from test_attn_checker import ATTN_FIXTURES, assert_matches_attn_fixture, attn_fixture, run_through
from test_decoder_mirror import TOL
from test_slat_mirror import (assert_matches_fixture, assert_matches_gated_fixture, fixture, matching_loss_of, run_gated, run_mirror)

from fresnel_amd import _binding as B

gpu = pytest.mark.gpu
QB, KT, KB = B.FGS_ATTN_QUERY_BLOCK, B.FGS_ATTN_KEY_TILE, B.FGS_ATTN_KEY_BLOCK


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _case(Bn, H, N, M, d, seed, spread=1.5):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(Bn, N, H * d, generator=g) * spread
    kv = torch.randn(Bn, M, 2, H, d, generator=g)
    return q, kv, torch.randn(Bn, N, H * d, generator=g)


def _mask(Bn, N, seed):
    m = torch.rand(Bn, N, generator=torch.Generator().manual_seed(seed)) > 0.25
    m[0, 0] = False
    return m


def _hip(q, kv, H, up, dev, mask=None, dropout_p=0.0, seed=None):
    from fresnel_amd.slat import cross_attention
    ql, kvl = q.to(dev).requires_grad_(True), kv.to(dev).requires_grad_(True)
    seed_t = None if seed is None else torch.tensor([seed], dtype=torch.int64, device=dev)
    out = cross_attention(ql, kvl, H, mask=None if mask is None else mask.to(dev), dropout_p=dropout_p, seed=seed_t, backend="hip")
    out.backward(up.to(dev))
    torch.cuda.synchronize()
    return dict(out=out.detach().cpu(), g_q=ql.grad.cpu(), g_kv=kvl.grad.cpu())


def _checker(q, kv, H, up, dtype=torch.float64, **kw):
    ql, kvl = q.clone().to(dtype).requires_grad_(True), kv.clone().to(dtype).requires_grad_(True)
    out = AC.attend(ql, kvl, H, **kw)
    out.backward(up.to(dtype))
    return dict(out=out.detach(), g_q=ql.grad, g_kv=kvl.grad)


def _compare(tag, got, want, tol=TOL):
    for k in ("out", "g_q", "g_kv"):
        e = rel_to_max(got[k].double().numpy(), want[k].double().numpy())
        print(f"{tag}: {k} {e:.2e}")
        assert e <= tol, f"{tag}: {k} is {e:.2e} of its maximum away from the checker"


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the reference's fixtures through the kernels --------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ATTN_FIXTURES)
def test_fixture_through_cross_attention_hip(name):
    from fresnel_amd.slat import cross_attention
    fx = attn_fixture(name)
    out, grads = run_through(fx, lambda q, kv, H, mask: cross_attention(q, kv, H, mask=mask, backend="hip"), device=_dev())
    assert_matches_attn_fixture(fx, out, grads, name)


@gpu
@pytest.mark.parametrize("name", ATTN_FIXTURES)
def test_fixture_through_the_module_with_backend_hip(name):
    from fresnel_amd.slat import CrossAttention
    dev = _dev()
    fx = attn_fixture(name)
    module = CrossAttention(**json.loads(str(fx["ctor"])))
    module.load_state_dict({k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sd.")}, strict=True)
    module = module.to(dev).eval()
    module.backend = "hip"
    x, context = (torch.from_numpy(fx[k]).to(dev).requires_grad_(True) for k in ("x", "context"))
    mask = torch.from_numpy(fx["mask"]).to(dev) if "mask" in fx.files else None
    calls = []
    import fresnel_amd.slat as slat
    real = slat.hip.call
    # (`call` re-enters itself once with the device guard held: count the outer calls)
    slat.hip.call = lambda dev_, name_, *a: (calls.append(name_) if type(dev_) is not slat.hip.on_device else None, real(dev_, name_, *a))[1]
    try:
        out = module(x, context, mask)
    finally:
        slat.hip.call = real
    assert calls == ["fgs_attn_forward"]   # ONE call whatever chunk_size is (A3: 50 queries, chunks of 16)
    (out * torch.from_numpy(fx["g"]).to(dev)).sum().backward()
    grads = {"x": x.grad, "context": context.grad}
    grads.update({"sd." + k: p.grad for k, p in module.named_parameters()})
    assert_matches_attn_fixture(fx, out.detach(), grads, name + " (module)")


@gpu
@pytest.mark.parametrize("name", ["slat_S1", "slat_S4"])
def test_decoder_with_attn_backend_hip_reproduces_the_fixture(name):
    from fresnel_amd import slat
    dev = _dev()
    fx = fixture(name)
    model = slat.DirectSLatDecoder(**json.loads(str(fx["ctor"])), attn_backend="hip")
    model.load_state_dict({k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sd.")}, strict=True)
    model = model.eval().to(dev)
    assert all(b.cross_attn.backend == "hip" for b in model.blocks) and model.gaussian_head.backend == "torch"
    out, grads, raw = run_mirror(model, fx, dev)   # S4: N = 1030 in one call
    assert_matches_fixture(fx, out, grads, raw, name + " (attn hip)")


@gpu
def test_gated_inference_with_attn_backend_hip_reproduces_the_lists():
    from fresnel_amd import slat
    dev = _dev()
    fx = fixture("slat_S2")
    sd = {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sd.")}
    for head_backend in ("torch", "hip"):   # the two backends are independent
        model = slat.DirectSLatDecoder(**json.loads(str(fx["ctor"])), head_backend=head_backend, attn_backend="hip")
        model.load_state_dict(sd, strict=True)
        assert_matches_gated_fixture(fx, run_gated(model.eval().to(dev), fx, dev), f"slat_S2 (attn hip, head {head_backend})")


# ---- random parity with the checker, at the seams -----------------------------------------------------------------------------------------
SEAMS = ([("M", 1, 2, 37, M, 32) for M in (1, KT - 1, KT, KT + 1, 2 * KT + 3, KB - 1, KB + 1)]
         + [("N", 1, 2, N, 2 * KT + 3, 5) for N in (1, QB - 1, QB, QB + 1)]
         + [("d", 1, 2, 37, KT + 1, d) for d in (5, 32, 33, 64, 128)]
         + [("BH", Bn, H, QB + 1, KT + 1, 33) for Bn, H in ((1, 1), (2, 3))])


@gpu
@pytest.mark.parametrize("axis,Bn,H,N,M,d", SEAMS, ids=[f"{a}-B{b}H{h}N{n}M{m}d{d}" for a, b, h, n, m, d in SEAMS])
@pytest.mark.parametrize("masked", [False, True], ids=["open", "masked"])
def test_random_parity_with_the_checker(axis, Bn, H, N, M, d, masked):
    q, kv, up = _case(Bn, H, N, M, d, 2000 + 7 * N + 3 * M + d)
    mask = _mask(Bn, N, N + M) if masked else None
    _compare(f"{axis} B{Bn} H{H} N{N} M{M} d{d}", _hip(q, kv, H, up, _dev(), mask=mask), _checker(q, kv, H, up, mask=mask))


# ---- the online softmax's seams -------------------------------------------------------------------------------------------------------
def _scored(scores, seed, gains):
    """q, kv (one image, one head, d = 32) whose scores scale <q, k> are `scores` (M,) times the row's gain, up to fp32 rounding:
    the query's first channel carries the gain, the key's first channel the score; the other channels are small noise on the keys."""
    g = torch.Generator().manual_seed(seed)
    N, M, d = len(gains), scores.shape[0], 32
    q = torch.zeros(1, N, d, dtype=torch.float64)
    q[0, :, 0] = torch.tensor(gains, dtype=torch.float64)
    kv = torch.randn(1, M, 2, 1, d, generator=g, dtype=torch.float64)
    kv[0, :, 0, 0, 1:] *= 0.01
    kv[0, :, 0, 0, 0] = scores.double() * d ** 0.5
    return q.float(), kv.float(), torch.randn(1, N, d, generator=g)


@gpu
@pytest.mark.parametrize("kind", ["max_in_first_tile", "max_in_last_tile_only", "all_equal", "near_plus_80", "near_minus_80"])
def test_online_softmax_seams(kind):
    """Every tensor of every case within TOL of its maximum.  The spike cases run five rows with gains 0.1 ... 2: the spike is +3 in
    the first row -- an unsaturated softmax, whose g_q is of ordinary size and is what the tensor's maximum comes from -- and +17
    ... +60 in the others, whose g_q is below 1e-6 of that.  The +-80 cases are where the backward's recomputed score must be rounded
    as the forward's was: with the product S scale fused into the subtraction of the saved row constant, every score is off by up
    to 2^-24 x 80 against the forward's, and since every key's first channel is nearly the same number here (229 against a spread of
    3), g_q -- a cancelling sum over the keys -- came out 6e-5 off where the tolerance is 1.1e-5 (fresnel_amd/build.py)."""
    M = 2 * KT + 3
    g = torch.Generator().manual_seed(31)
    s = torch.rand(M, generator=g) * 0.5
    gains = [1.0, 1.25, 1.5, 1.75, 2.0]
    if kind == "max_in_first_tile":
        s[3] = 30.0
        gains = [0.1, 0.575, 1.05, 1.525, 2.0]
    elif kind == "max_in_last_tile_only":
        s[M - 1] = 30.0
        gains = [0.1, 0.575, 1.05, 1.525, 2.0]
    elif kind == "all_equal":
        s[:] = 0.75
    elif kind == "near_plus_80":
        s = 40.0 + s     # row gains 1 ... 2: scores from +40 to +81
    elif kind == "near_minus_80":
        s = -40.0 - s
    N = len(gains)
    q, kv, up = _scored(s, 32, gains)
    got, want = _hip(q, kv, 1, up, _dev()), _checker(q, kv, 1, up)
    assert bool(torch.isfinite(got["out"]).all()) and bool(torch.isfinite(got["g_q"]).all()) and bool(torch.isfinite(got["g_kv"]).all())
    _compare(kind, got, want)
    if kind == "max_in_last_tile_only":   # with gain 2 the spike takes everything: the output is the last value row
        assert rel_to_max(got["out"][0, -1].numpy(), kv[0, M - 1, 1, 0].numpy()) <= TOL
        assert float(want["g_q"][0, 0].abs().max()) > 0.1 * float(want["g_q"].abs().max())   # the unsaturated row counts
    if kind == "all_equal":
        assert rel_to_max(got["out"][0].numpy(), kv[0, :, 1, 0].mean(dim=0).expand(N, 32).numpy()) <= TOL


# ---- masked rows ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_masked_rows_attend_uniformly_and_send_nothing_to_queries_or_keys():
    Bn, H, N, M, d = 2, 3, QB + 5, KT + 7, 10
    q, kv, up = _case(Bn, H, N, M, d, 41)
    mask = _mask(Bn, N, 42)
    got = _hip(q, kv, H, up, _dev(), mask=mask)
    mean_v = kv[:, :, 1].mean(dim=1).reshape(Bn, 1, H * d).expand(Bn, N, H * d)
    assert rel_to_max(got["out"][~mask].numpy(), mean_v[~mask].numpy()) <= TOL
    assert not got["g_q"][~mask].any() and got["g_q"][mask].any()                       # exactly zero rows
    _compare("masked", got, _checker(q, kv, H, up, mask=mask))
    # through the values only: with every row masked the keys get nothing at all, the values get mean-weighted upstream rows
    none = torch.zeros(Bn, N, dtype=torch.bool)
    got = _hip(q, kv, H, up, _dev(), mask=none)
    assert not got["g_kv"][:, :, 0].any() and not got["g_q"].any()
    want_v = (up.reshape(Bn, N, H, d).sum(dim=1, keepdim=True) / M).expand(Bn, M, H, d)
    assert rel_to_max(got["g_kv"][:, :, 1].numpy(), want_v.numpy()) <= TOL


# ---- the NaN rule --------------------------------------------------------------------------------------------------------------------------
def _nan_case(kind):
    Bn, H, N, M, d = 2, 2, 40, KT + 5, 6
    q, kv, up = _case(Bn, H, N, M, d, 51)
    bad = torch.zeros(Bn, H, N, dtype=torch.bool)
    dtype = torch.float64
    if kind == "nan_key":
        kv[0, 2, 0, 0, 1] = float("nan")
        bad[0, 0] = True
    elif kind == "inf_query":
        q[1, 7, d + 2] = float("inf")          # image 1, row 7, head 1
        bad[1, 1, 7] = True
    elif kind == "all_keys_minus_inf":
        q[0, :, d:] = q[0, :, d:].abs() + 0.1  # head 1 of image 0: positive queries, every key -Inf -> every score -Inf
        kv[0, :, 0, 1, :] = float("-inf")
        bad[0, 1] = True
    else:                                      # products that overflow in fp32 (the checker runs in fp32 there)
        q[1, 3, 0] = 3e38                      # times a key channel beyond +-1.2: +-Inf; the other rows see ordinary keys
        kv[1, 0, 0, 0, 0], kv[1, 1, 0, 0, 0] = 4.0, -4.0
        bad[1, 0, 3] = True
        dtype = torch.float32
    return q, kv, up, bad, dtype


@gpu
@pytest.mark.parametrize("kind", ["nan_key", "inf_query", "all_keys_minus_inf", "overflowing_products"])
def test_nan_rule(kind):
    q, kv, up, bad, dtype = _nan_case(kind)
    Bn, H, N = bad.shape
    d, M = q.shape[2] // H, kv.shape[1]
    got = _hip(q, kv, H, up, _dev(), dropout_p=0.2, seed=77)
    keep = AC.keep_mask(77, Bn, H, N, M, 0.2)
    want = _checker(q, kv, H, up, dtype=dtype, keep=keep, dropout_p=0.2, nan_rule=True)
    assert all(bool(torch.isfinite(t).all()) for t in want.values())
    _compare(kind, got, want)                                                           # other rows are untouched
    out, g_q = got["out"].reshape(Bn, N, H, d).transpose(1, 2), got["g_q"].reshape(Bn, N, H, d).transpose(1, 2)
    mean_v = kv[:, :, 1].mean(dim=1).unsqueeze(2).expand(Bn, H, N, d)                   # uniform, without dropout
    assert rel_to_max(out[bad].numpy(), mean_v[bad].numpy()) <= TOL
    assert not g_q[bad].any() and g_q[~bad].any() and bool(torch.isfinite(got["g_kv"]).all())


@gpu
def test_a_nan_value_reaches_the_outputs_torch_reaches():
    from fresnel_amd.slat import cross_attention
    dev = _dev()
    q, kv, _ = _case(2, 2, 40, KT + 5, 6, 61)
    kv[1, 9, 1, 0, 4] = float("nan")
    got = cross_attention(q.to(dev), kv.to(dev), 2, backend="hip").cpu()
    want = cross_attention(q.to(dev), kv.to(dev), 2, backend="torch").cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and int(torch.isnan(got).sum()) == 40   # image 1, head 0, channel 4
    assert rel_to_max(torch.nan_to_num(got).numpy(), torch.nan_to_num(want).numpy()) <= TOL


# ---- dropout ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("p", [0.2, 0.5])
def test_dropout_obeys_the_stated_keep_rule(p):
    Bn, H, N, M, d = 2, 3, QB + 3, 2 * KT + 3, 33
    q, kv, up = _case(Bn, H, N, M, d, 71)
    mask = _mask(Bn, N, 72)                                                             # masked rows get dropout too
    seed = -0x0123456789ABCDEF                                                          # both halves, and the sign bit
    got = _hip(q, kv, H, up, _dev(), mask=mask, dropout_p=p, seed=seed)
    want = _checker(q, kv, H, up, mask=mask, keep=AC.keep_mask(seed, Bn, H, N, M, p), dropout_p=p)
    _compare(f"dropout {p}", got, want)
    again = _hip(q, kv, H, up, _dev(), mask=mask, dropout_p=p, seed=seed)
    assert all(_same_bits(got[k], again[k]) for k in got)
    other = _hip(q, kv, H, up, _dev(), mask=mask, dropout_p=p, seed=seed + 1)
    assert not torch.equal(got["out"], other["out"])
    plain = _checker(q, kv, H, up, mask=mask)
    assert rel_to_max(got["out"].double().numpy(), plain["out"].numpy()) > 100 * TOL    # and it is not the undropped result


@gpu
def test_module_dropout_follows_training_mode_and_manual_seed():
    from fresnel_amd.slat import CrossAttention
    dev = _dev()
    torch.manual_seed(81)
    module = CrossAttention(24, 3, attn_drop=0.5).to(dev)
    module.backend = "hip"
    x, context = torch.randn(2, 50, 24, device=dev), torch.randn(2, 9, 24, device=dev)
    module.eval()
    a, b = module(x, context), module(x, context)
    module.attn_drop.p = 0.0
    assert _same_bits(a, b) and _same_bits(a, module(x, context))                       # eval() ignores p
    module.attn_drop.p = 0.5
    module.train()
    torch.manual_seed(82)
    t1 = module(x, context)
    t2 = module(x, context)
    torch.manual_seed(82)
    t3 = module(x, context)
    assert not torch.equal(t1, a) and not torch.equal(t1, t2) and _same_bits(t1, t3)    # drawn on the device, follows manual_seed


@gpu
def test_checkpointing_with_dropout_gives_the_uncheckpointed_gradients():
    from fresnel_amd.slat import DirectSLatDecoder
    dev = _dev()
    torch.manual_seed(91)
    ctor = dict(feature_dim=12, hidden_dim=20, num_layers=2, num_heads=4, num_gaussians_per_voxel=2, dropout=0.2, attn_backend="hip")
    plain, ckpt = DirectSLatDecoder(**ctor), DirectSLatDecoder(**ctor, use_checkpoint=True)
    ckpt.load_state_dict(plain.state_dict())
    g = torch.Generator().manual_seed(92)
    features, coords = torch.randn(2, 5, 12, generator=g).to(dev), torch.randint(0, 64, (2, 40, 4), generator=g).to(dev)
    grads = []
    for model in (plain, ckpt):
        model = model.to(dev).train()
        torch.manual_seed(93)
        out = model(features, coords)
        (out["gaussians"].square().sum() + out["occupancy_logits"].sum()).backward()
        grads.append({k: p.grad.cpu() for k, p in model.named_parameters()})
    for k in grads[0]:
        e = rel_to_max(grads[1][k].numpy(), grads[0][k].numpy())
        assert e <= TOL, f"{k}: the checkpointed run's gradient is {e:.2e} of its maximum away"
    assert any(v.any() for v in grads[0].values())


# ---- repeatability and capture ---------------------------------------------------------------------------------------------------------------
@gpu
def test_two_calls_and_batch_against_single_images_are_bit_identical():
    Bn, H, N, M, d = 3, 2, QB + 9, KB + 5, 33
    q, kv, up = _case(Bn, H, N, M, d, 101)
    mask = _mask(Bn, N, 102)
    dev = _dev()
    a, b = _hip(q, kv, H, up, dev, mask=mask), _hip(q, kv, H, up, dev, mask=mask)
    assert all(_same_bits(a[k], b[k]) for k in a)
    for i in range(Bn):
        one = _hip(q[i:i + 1], kv[i:i + 1], H, up[i:i + 1], dev, mask=mask[i:i + 1])
        assert all(_same_bits(a[k][i:i + 1], one[k]) for k in a), f"image {i} depends on its batch"


@gpu
def test_captured_graph_follows_queries_changed_in_place():
    from fresnel_amd.slat import cross_attention
    dev = _dev()
    q_c, kv_c, up_c = _case(2, 2, QB + 1, KT + 1, 10, 111)
    q2 = _case(2, 2, QB + 1, KT + 1, 10, 112)[0].to(dev)
    q, kv, up = q_c.to(dev).requires_grad_(True), kv_c.to(dev).requires_grad_(True), up_c.to(dev)
    q1 = q.detach().clone()
    mask = _mask(2, QB + 1, 113).to(dev)
    leaves = (q, kv)

    def step():
        out = cross_attention(q, kv, 2, mask=mask, backend="hip")
        out.backward(up)
        return out

    def eager(values):
        with torch.no_grad():
            q.copy_(values)
        for t in leaves:
            t.grad = None
        out = step()
        torch.cuda.synchronize()
        return [out.detach().clone()] + [t.grad.detach().clone() for t in leaves]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager(q1)
        want_new = eager(q2)
        eager(q1)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in leaves:
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        q.copy_(q2)
        for t in leaves:
            t.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for name, x, y in zip(("out", "g_q", "g_kv"), [captured] + [t.grad for t in leaves], want_new):
        assert _same_bits(x, y), f"{name}: the replay does not follow the new queries"


# ---- limits --------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_limits_raise_without_a_launch():
    import fresnel_amd.slat as slat
    dev = _dev()
    calls = []
    real = slat.hip.call
    slat.hip.call = lambda *a: (calls.append(a[1]), real(*a))[1]
    try:
        with pytest.raises(ValueError, match="head dimension 129"):
            slat.cross_attention(torch.randn(1, 3, 129, device=dev), torch.randn(1, 2, 2, 1, 129, device=dev), 1, backend="hip")
        q, kv = torch.randn(2, 5, 12, device=dev), torch.randn(2, 4, 2, 3, 4, device=dev)
        with pytest.raises(ValueError, match="dropout_p"):
            slat.cross_attention(q, kv, 3, dropout_p=1.0, backend="hip")
        with pytest.raises(ValueError, match="contiguous"):
            slat.cross_attention(q, torch.randn(2, 2, 4, 3, 4, device=dev).transpose(1, 2), 3, backend="hip")
        with pytest.raises(B.FgsError, match="no CPU fallback"):
            slat.cross_attention(q, kv, 3, mask=torch.ones(2, 5, dtype=torch.bool), backend="hip")
    finally:
        slat.hip.call = real
    assert calls == []
    # the library's own refusal (what the wrapper's checks stand in front of), as a clean error
    out, saved = torch.empty(1, 3, 129, device=dev), torch.empty(256, dtype=torch.uint8, device=dev)
    with pytest.raises(B.FgsError, match="head_dim = 129"):
        real(dev, "fgs_attn_forward", 1, 3, 2, 1, 129, 1.0, 0.0, out, torch.empty(1, 2, 2, 1, 129, device=dev), None, None, out, saved)
    with pytest.raises(B.FgsError, match="needs a seed"):
        real(dev, "fgs_attn_forward", 1, 3, 2, 1, 8, 1.0, 0.5, out, out, None, None, out, saved)


@gpu
def test_under_autocast_the_inputs_are_cast_to_fp32():
    from fresnel_amd.slat import cross_attention
    dev = _dev()
    q, kv, up = _case(1, 2, 20, 9, 8, 121)
    want = _checker(q.bfloat16().float(), kv.bfloat16().float(), 2, up)
    ql, kvl = q.to(dev).bfloat16().requires_grad_(True), kv.to(dev).bfloat16().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = cross_attention(ql, kvl, 2, backend="hip")
    assert out.dtype == torch.float32
    out.backward(up.to(dev))
    assert ql.grad.dtype == torch.bfloat16 and kvl.grad.dtype == torch.bfloat16
    assert rel_to_max(out.detach().cpu().double().numpy(), want["out"].numpy()) <= TOL


# ---- memory ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_no_score_tensor_is_allocated():
    from fresnel_amd.slat import cross_attention
    dev = _dev()
    Bn, H, N, M, d = 1, 8, 2048, 1369, 64
    scores = Bn * H * N * M * 4
    g = torch.Generator().manual_seed(131)
    q0, kv0, up = (torch.randn(*s, generator=g).to(dev) for s in ((Bn, N, H * d), (Bn, M, 2, H, d), (Bn, N, H * d)))
    rise = {}
    for backend in ("hip", "torch"):
        q, kv = q0.clone().requires_grad_(True), kv0.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = cross_attention(q, kv, H, backend=backend)
        out.backward(up)
        torch.cuda.synchronize()
        rise[backend] = torch.cuda.max_memory_allocated() - base
        del out, q, kv
    print(f"memory rise: hip {rise['hip'] / 2 ** 20:.1f} MiB, torch {rise['torch'] / 2 ** 20:.1f} MiB, one score tensor {scores / 2 ** 20:.1f} MiB")
    assert rise["hip"] < scores / 4, rise
    assert rise["torch"] > scores / 4, rise


# ---- a distillation step ------------------------------------------------------------------------------------------------------------------------
def _distill_setup(dev, dropout):
    from fresnel_amd.slat import DirectSLatDecoder
    torch.manual_seed(1800)
    ctor = dict(feature_dim=12, hidden_dim=20, num_layers=2, num_heads=4, num_gaussians_per_voxel=2, dropout=dropout)
    model = DirectSLatDecoder(**ctor)
    with torch.no_grad():
        model.gaussian_head.head[-1].weight.mul_(40.0)
        model.gaussian_head.scale_factor.fill_(0.2)
    g = torch.Generator().manual_seed(1801)
    Bn, N = 2, 40
    coords = torch.randint(0, 64, (Bn, N, 4), generator=g)
    coord_mask = torch.ones(Bn, N, dtype=torch.bool)
    coord_mask[1, -3:] = False
    target = torch.rand(Bn, 64, 14, generator=g)
    target[..., :3] = target[..., :3] * 2 - 1
    batch = dict(features=torch.randn(Bn, 5, 12, generator=g), coords=coords, coord_mask=coord_mask, gaussians=target,
                 gaussian_mask=torch.ones(Bn, 64, dtype=torch.bool), occupancy_target=(torch.rand(Bn, N, generator=g) > 0.5).float())
    twin = DirectSLatDecoder(**ctor, head_backend="hip", attn_backend="hip")
    twin.load_state_dict(model.state_dict(), strict=True)
    return model.to(dev).train(), twin.to(dev).train(), {k: v.to(dev) for k, v in batch.items()}


@gpu
def test_distill_step_with_head_match_and_attention_on_hip():
    from fresnel_amd import distill
    dev = _dev()
    cfg_t, cfg_h = distill.DistillConfig(), distill.DistillConfig(head_backend="hip", match_backend="hip")
    loss_t, loss_h = (matching_loss_of(c, max_match_points=4096) for c in (cfg_t, cfg_h))
    # dropout 0: the step is the all-torch step
    model_t, model_h, batch = _distill_setup(dev, 0.0)
    # plain SGD: Adam would turn the rounding noise of a gradient that is zero in exact arithmetic (the key bias: softmax ignores a
    # shift of the scores) into a full-size step whose sign is the noise's
    opt_t, opt_h = (torch.optim.SGD(m.parameters(), lr=0.05) for m in (model_t, model_h))
    first_t = distill.distill_step(model_t, batch, opt_t, loss_t, cfg_t)
    first_h = distill.distill_step(model_h, batch, opt_h, loss_h, cfg_h)
    torch.cuda.synchronize()
    assert abs(float(first_h["total"]) - float(first_t["total"])) <= TOL * abs(float(first_t["total"]))
    for (k, p), r in zip(model_h.named_parameters(), model_t.parameters()):
        e = rel_to_max(p.detach().cpu().numpy(), r.detach().cpu().numpy())
        assert e <= TOL, f"parameter {k} after one step is {e:.2e} of its maximum away from the all-torch step's"
    # training mode with dropout 0.1: nothing reads the host, the losses are finite
    _, model_h, batch = _distill_setup(dev, 0.1)
    opt_h = torch.optim.AdamW(model_h.parameters(), lr=2e-3)
    distill.distill_step(model_h, batch, opt_h, loss_h, cfg_h)   # (first use: lazy initialisations may synchronise)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = [distill.distill_step(model_h, batch, opt_h, loss_h, cfg_h) for _ in range(3)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(np.isfinite(float(v)) for step in losses for v in step.values())
