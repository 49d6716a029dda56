"""tests/attn_checker.py against the reference's CrossAttention fixtures A1-A3 (tests/golden/make_goldens_attn.py), on the CPU: the
checker reproduces output and every gradient within 1e-4 of the tensor's maximum in fp32 and in fp64, each of its five deliberate
mistakes misses a fixture by at least ten times that, the dropout keep rule has the stated statistics, and the new keywords of
fresnel_amd/slat.py change nothing by default."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_checker as AC
from helpers import GOLDEN, rel_to_max
from test_decoder_mirror import TOL

ATTN_FIXTURES = ["attn_A1", "attn_A2", "attn_A3"]


def attn_fixture(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def ref64(fx, key):
    """The reference's fp64 run of `key` (out, grad.x, ...): the fp32 run plus the recorded difference (make_goldens_attn.py)."""
    return fx[key].astype(np.float64) + fx["d64." + key].astype(np.float64) * float(fx["u64." + key])


def run_through(fx, attend_fn, dtype=torch.float32, device="cpu"):
    """The module around the attention -- the q, kv and proj Linear layers with the fixture's weights -- with `attend_fn(q, kv, H,
    mask)` between them -> output, gradients {x, context, sd.<parameter>} of sum(out x g)."""
    ctor = json.loads(str(fx["ctor"]))
    sd = {k[3:]: torch.from_numpy(fx[k]).to(device, dtype).requires_grad_(True) for k in fx.files if k.startswith("sd.")}
    x = torch.from_numpy(fx["x"]).to(device, dtype).requires_grad_(True)
    context = torch.from_numpy(fx["context"]).to(device, dtype).requires_grad_(True)
    mask = torch.from_numpy(fx["mask"]).to(device) if "mask" in fx.files else None
    H = ctor["num_heads"]
    q = F.linear(x, sd["q.weight"], sd["q.bias"])
    kv = F.linear(context, sd["kv.weight"], sd["kv.bias"]).reshape(x.shape[0], context.shape[1], 2, H, x.shape[2] // H)
    out = F.linear(attend_fn(q, kv, H, mask).to(dtype), sd["proj.weight"], sd["proj.bias"])
    (out * torch.from_numpy(fx["g"]).to(device, dtype)).sum().backward()
    grads = {"x": x.grad, "context": context.grad}
    grads.update({"sd." + k: v.grad for k, v in sd.items()})
    return out.detach(), grads


def worst_miss(fx, out, grads):
    """The largest distance, in the tensor's maximum, of any tensor from the NEARER of the fixture's fp32 and fp64 runs."""
    worst = 0.0
    for key, got in [("out", out)] + [("grad." + k, v) for k, v in grads.items()]:
        got = got.detach().cpu().double().numpy()
        worst = max(worst, min(rel_to_max(got, fx[key]), rel_to_max(got, ref64(fx, key))))
    return worst


def assert_matches_attn_fixture(fx, out, grads, what, tol=TOL):
    assert sorted(grads) == sorted(k[5:] for k in fx.files if k.startswith("grad.")), what
    for key, got in [("out", out)] + [("grad." + k, v) for k, v in grads.items()]:
        got = got.detach().cpu().double().numpy()
        assert got.shape == fx[key].shape, f"{what}: shape of {key}"
        e = min(rel_to_max(got, fx[key]), rel_to_max(got, ref64(fx, key)))
        assert e <= tol, f"{what}: {key} is {e:.2e} of its maximum away from the reference's fp32 and fp64 runs"


# ---- the checker against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", ATTN_FIXTURES)
def test_checker_reproduces_the_reference(name, dtype):
    fx = attn_fixture(name)
    out, grads = run_through(fx, lambda q, kv, H, mask: AC.attend(q, kv, H, mask=mask), dtype)
    assert_matches_attn_fixture(fx, out, grads, name)
    out, grads = run_through(fx, lambda q, kv, H, mask: AC.attend(q, kv, H, mask=mask, nan_rule=True), dtype)   # no row is bad
    assert_matches_attn_fixture(fx, out, grads, name + " (nan_rule)")


def test_fixtures_are_what_they_are_for():
    a1, a2, a3 = (attn_fixture(n) for n in ATTN_FIXTURES)
    assert a1["x"].shape == (2, 70, 128) and a1["context"].shape[1] == 45 and json.loads(str(a1["ctor"]))["num_heads"] == 2
    assert a2["x"].shape[1:] == (33, 96) and a2["context"].shape[1] == 3 and json.loads(str(a2["ctor"]))["num_heads"] == 3
    assert a3["x"].shape[1:] == (50, 40) and json.loads(str(a3["ctor"])) == dict(dim=40, num_heads=4, chunk_size=16)
    assert (~a1["mask"]).any(axis=1).all() and (~a3["mask"]).any() and "mask" not in a2.files
    for fx in (a1, a2, a3):   # the two precisions agree far inside the tolerance: either is a reference
        assert 0 < rel_to_max(fx["out"], ref64(fx, "out")) < 0.1 * TOL
        assert sorted("d64." + k for k in fx.files if k == "out" or k.startswith("grad.")) == sorted(k for k in fx.files if k.startswith("d64."))
        assert all(np.isfinite(fx[k]).all() for k in fx.files if fx[k].dtype.kind == "f")
    assert all(os.path.getsize(os.path.join(GOLDEN, n + ".npz")) < 1024 * 1024 for n in ATTN_FIXTURES)


@pytest.mark.parametrize("wrong", AC.WRONG_RULES)
def test_each_wrong_rule_misses_a_fixture(wrong):
    misses = {}
    for name in ATTN_FIXTURES:
        fx = attn_fixture(name)
        out, grads = run_through(fx, lambda q, kv, H, mask: AC.attend(q, kv, H, mask=mask, wrong=wrong), torch.float64)
        misses[name] = worst_miss(fx, out, grads)
    assert max(misses.values()) >= 10 * TOL, f"{wrong}: no fixture tells ({misses})"


# ---- the keep rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.2, 0.5])
def test_keep_mask_keeps_the_stated_fraction(p):
    Bn, H, N, M = 2, 4, 50, 64
    keep = AC.keep_mask(1234567890123, Bn, H, N, M, p)
    n = keep.size
    assert keep.shape == (Bn, H, N, M) and keep.dtype == np.bool_ and n >= 25000
    sigma = (p * (1 - p) / n) ** 0.5
    assert abs(keep.mean() - (1 - p)) <= 5 * sigma, (keep.mean(), 1 - p, sigma)
    # per key column and per row as well: no axis is degenerate
    assert np.abs(keep.mean(axis=(0, 1, 2)) - (1 - p)).max() <= 5 * (p * (1 - p) / (Bn * H * N)) ** 0.5
    assert np.abs(keep.mean(axis=3) - (1 - p)).max() <= 5 * (p * (1 - p) / M) ** 0.5


def test_keep_mask_depends_on_seed_head_and_row():
    a = AC.keep_mask(7, 1, 2, 3, 256, 0.5)
    assert not np.array_equal(a, AC.keep_mask(8, 1, 2, 3, 256, 0.5))                # the low half of the seed
    assert not np.array_equal(a, AC.keep_mask(7 + (1 << 32), 1, 2, 3, 256, 0.5))    # the high half
    assert not np.array_equal(a[0, 0], a[0, 1]) and not np.array_equal(a[0, 0, 0], a[0, 0, 1])
    assert np.array_equal(a, AC.keep_mask(7, 1, 2, 3, 256, 0.5))
    assert np.array_equal(AC.keep_mask(-1, 1, 2, 3, 256, 0.5), AC.keep_mask(2 ** 64 - 1, 1, 2, 3, 256, 0.5))   # int64 -1: its bit pattern
    assert AC.keep_mask(7, 2, 2, 5, 300, 0.0).all()
    assert AC.keep_threshold(0.5) == 1 << 23 and AC.keep_threshold(0.0) == 0
    # row = (b H + h) N + n: a batch's second image continues the first's rows
    assert np.array_equal(AC.keep_mask(7, 2, 2, 3, 64, 0.2)[0], AC.keep_mask(7, 1, 2, 3, 64, 0.2)[0])


def test_checker_dropout_and_nan_rule_do_what_the_definition_says():
    g = torch.Generator().manual_seed(3)
    q, kv = torch.randn(1, 4, 6, generator=g, dtype=torch.float64), torch.randn(1, 5, 2, 2, 3, generator=g, dtype=torch.float64)
    keep = AC.keep_mask(5, 1, 2, 4, 5, 0.5)
    plain = AC.attend(q, kv, 2)
    assert torch.allclose(AC.attend(q, kv, 2, keep=np.ones_like(keep), dropout_p=0.0), plain)
    dropped = AC.attend(q, kv, 2, keep=keep, dropout_p=0.5)
    assert not torch.allclose(dropped, plain)
    # a NaN key: every row is bad -> the mean of v, a zero g_q, a finite g_kv through v only
    kv_bad = kv.clone()
    kv_bad[0, 2, 0, 1, 0] = float("nan")
    qg, kvg = q.clone().requires_grad_(True), kv_bad.clone().requires_grad_(True)
    out = AC.attend(qg, kvg, 2, keep=keep, dropout_p=0.5, nan_rule=True)
    assert torch.allclose(out[:, :, 3:], kv_bad[:, :, 1, 1].mean(dim=1, keepdim=True).expand(1, 4, 3))   # head 1: uniform, no dropout
    out.sum().backward()
    assert not qg.grad[:, :, 3:].any() and bool(torch.isfinite(kvg.grad).all()) and not kvg.grad[:, :, 0, 1].any()
    assert torch.isnan(AC.attend(q, kv_bad, 2)[:, :, 3:]).all()                      # without the rule: what softmax makes of it


# ---- the new keywords change nothing by default ------------------------------------------------------------------------------------------
def test_mirror_with_attn_backend_torch_is_the_mirror_bit_for_bit():
    from fresnel_amd import slat
    from test_slat_mirror import fixture, mirror_inputs
    fx = fixture("slat_S1")
    ctor = json.loads(str(fx["ctor"]))
    sd = {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sd.")}
    outs = []
    for kw in ({}, dict(attn_backend="torch")):
        model = slat.DirectSLatDecoder(**ctor, **kw)
        model.load_state_dict(sd, strict=True)
        assert all(b.cross_attn.backend == "torch" for b in model.blocks) and model.attn_backend == "torch"
        args = mirror_inputs(fx)
        out = model.eval()(*args)
        sum(v.sum() for v in out.values()).backward()
        outs.append((out, args[0].grad))
    for k in outs[0][0]:
        assert torch.equal(outs[0][0][k], outs[1][0][k]), k
    assert torch.equal(outs[0][1], outs[1][1])
    assert list(slat.DirectSLatDecoder(**ctor, attn_backend="hip").state_dict()) == list(sd)   # the keyword adds no state


def test_attention_arguments_are_validated_without_a_gpu():
    from fresnel_amd import _binding, slat
    with pytest.raises(ValueError, match="attn_backend"):
        slat.DirectSLatDecoder(8, 12, 1, attn_backend="triton")
    q, kv = torch.randn(2, 5, 12), torch.randn(2, 4, 2, 3, 4)
    mask = torch.ones(2, 5, dtype=torch.bool)
    mask[1, 2] = False
    out = slat.cross_attention(q, kv, 3, mask=mask)
    assert torch.allclose(out, AC.attend(q, kv, 3, mask=mask), atol=1e-6)
    assert torch.equal(out, slat.cross_attention(q, kv.reshape(2, 4, 24), 3, mask=mask))
    assert torch.allclose(out[1, 2], kv[1, :, 1].mean(dim=0).reshape(12), atol=1e-6)              # a masked row: the mean of v
    for bad, match in ((dict(backend="triton"), "attn_backend"), (dict(dropout_p=1.0), "dropout_p"), (dict(dropout_p=-0.1), "dropout_p"),
                       (dict(mask=mask.float()), "mask"), (dict(mask=mask[:, :4]), "mask")):
        with pytest.raises(ValueError, match=match):
            slat.cross_attention(q, kv, 3, **bad)
    with pytest.raises(ValueError, match="num_heads"):
        slat.cross_attention(q, kv, 5)
    with pytest.raises(ValueError, match="kv must be"):
        slat.cross_attention(q, kv[:, :, :, :2], 3)
    # the hip backend's limits are refused before anything is launched -- and before the device is looked at
    with pytest.raises(ValueError, match="head dimension 129"):
        slat.cross_attention(torch.randn(1, 3, 129), torch.randn(1, 2, 2, 1, 129), 1, backend="hip")
    with pytest.raises(ValueError, match="dropout_p"):
        slat.cross_attention(q, kv, 3, dropout_p=1.0, backend="hip")
    with pytest.raises(ValueError, match="contiguous"):
        slat.cross_attention(q, torch.randn(2, 2, 4, 3, 4).transpose(1, 2), 3, backend="hip")
    with pytest.raises(ValueError, match="dropout_p"):   # 1 - 1e-9 is 1.0 in fp32, which is what the library sees
        slat.cross_attention(q, kv, 3, dropout_p=1.0 - 1e-9, backend="hip")
    with pytest.raises(ValueError, match="seed"):
        slat.cross_attention(q, kv, 3, dropout_p=0.1, seed=torch.zeros(1), backend="hip")
    with pytest.raises(_binding.FgsError, match="no CPU fallback"):
        slat.cross_attention(q, kv, 3, backend="hip")
    module = slat.CrossAttention(12, 3)
    module.backend = "hip"
    with pytest.raises(_binding.FgsError, match="no CPU fallback"):
        module(torch.randn(2, 5, 12), torch.randn(2, 4, 12))
    module.backend = "triton"
    with pytest.raises(ValueError, match="attn_backend"):
        module(torch.randn(2, 5, 12), torch.randn(2, 4, 12))


def test_the_library_refuses_bad_attention_shapes_without_a_gpu():
    """rc = FGS_EINVAL / FGS_EUNSUPPORTED with a message, before anything touches the device."""
    from fresnel_amd import _binding as B
    assert B.sizes("fgs_attn_workspace_bytes", 2, 70, 45, 2, 64) == (1280, 1280)      # one float per (b, h, n), rounded up to 256 B
    for dims, match in (((2, 70, 45, 2, 129), "head_dim"), ((0, 70, 45, 2, 64), "invalid dims"), ((2, 70, 0, 2, 64), "invalid dims"),
                        ((1 << 15, 1 << 15, 4, 2, 64), "beyond")):
        with pytest.raises(B.FgsError, match=match):
            B.sizes("fgs_attn_workspace_bytes", *dims)
    lib = B.load()
    assert lib.fgs_attn_forward(1, 4, 4, 1, 8, 1.0, 1.0, None, None, None, None, None, None, None) == -1
    assert b"dropout_p" in lib.fgs_last_error()
    assert lib.fgs_attn_forward(1, 4, 4, 1, 8, 1.0, 0.0, None, None, None, None, None, None, None) == -1
    assert b"null" in lib.fgs_last_error()
    assert lib.fgs_attn_backward(1, 4, 4, 1, 8, 1.0, float("nan"), *([None] * 11)) == -1
    # the seams the GPU tests sit on are the header's, which the kernels compile against: no value is retyped on the way
    from test_call_layer import _header, header_defines
    defines = header_defines(_header())
    for name in ("FGS_ATTN_QUERY_BLOCK", "FGS_ATTN_KEY_TILE", "FGS_ATTN_KEY_BLOCK", "FGS_ATTN_MAX_HEAD_DIM"):
        assert getattr(B, name) == defines[name], name
    src = open(os.path.join(os.path.dirname(B.__file__), "csrc", "fgs_attn.hip")).read()
    for name in ("QB = FGS_ATTN_QUERY_BLOCK;", "KT = FGS_ATTN_KEY_TILE;", "KB = FGS_ATTN_KEY_BLOCK;", "head_dim > FGS_ATTN_MAX_HEAD_DIM"):
        assert name in src, name
