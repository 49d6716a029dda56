"""The 16-bit fused cross-attention (csrc/fgs_attn_half.hip, fresnel_amd.slat.cross_attention backend "hip" with compute_dtype fp16 /
bf16) on the GPU, and the distillation step under AMP.

THE RULE.  out, g_q and g_kv are compared with tests/attn_checker.py in fp64 on the 16-bit inputs converted to fp64, as max|a - b| /
max|b| (helpers.rel_to_max).  No tolerance is fixed: for each tensor the fused path's error may be at most TWICE the error of the
referee -- the reference's op sequence, cross_attention(backend="torch"), under torch.autocast("cuda", dtype) on the same GPU and
inputs (the project's referee margin).  With dropout the referee is the same op sequence with the stated keep mask in place of
torch's own draw.  At every parity case the referee's own error must first be at most 16 half-ulps of the dtype (16 x 2^-9 for bf16,
16 x 2^-12 for fp16), so that the rule is not vacuous.  Every judged case prints both errors.

Two places where exact arithmetic gives an all-zero tensor, so that the rule has no error of the referee to scale:
  - M = 1: g_q and g_k are identically zero (a softmax over one key).  The kernels form dS = p (dA - delta) with dA from the matrix
    cores and delta from a separate fused-multiply-add chain over the stored output, which agree only to fp32 rounding unless the sum
    has one term; the M = 1 cases therefore run at d = 1, where both are the same single exact product.
  - the fp16 overflow case is judged against the checker alone, as stated in include/fgs.h.
Bounds that do not come from the referee are derived where they are used, from the formats' precision: a value rounded once to 16
bits is within 2^-8 (bf16) / 2^-11 (fp16) of itself, i.e. 2 of the half-ulps above, relative to the tensor's maximum."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_checker as AC
from helpers import rel_to_max
from test_attn_checker import ATTN_FIXTURES, attn_fixture
from test_hip_attn import QB, KB, _case, _dev, _mask, _scored
from test_slat_mirror import matching_loss_of

from fresnel_amd import _binding as B

gpu = pytest.mark.gpu
KT = B.FGS_ATTN_HALF_KEY_TILE
DTYPES = [torch.bfloat16, torch.float16]
both = pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
HALF_ULP = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}
ROUND_ONCE = 2.5   # in HALF_ULP units: one rounding at the store (2) plus the fp32 accumulation's and normalisation's share
KEYS = ("out", "g_q", "g_kv")


def _name(dt):
    return "bf16" if dt is torch.bfloat16 else "fp16"


def _rounded(dt, *tensors):
    return tuple(t.to(dt) for t in tensors)


def _fused(q, kv, H, up, dev, mask=None, dropout_p=0.0, seed=None, dt=None):
    """q, kv, up: 16-bit CPU tensors -> the fused path's out, g_q, g_kv on the CPU, in the 16-bit dtype."""
    from fresnel_amd.slat import cross_attention
    ql, kvl = q.to(dev).requires_grad_(True), kv.to(dev).requires_grad_(True)
    seed_t = None if seed is None else torch.tensor([seed], dtype=torch.int64, device=dev)
    out = cross_attention(ql, kvl, H, mask=None if mask is None else mask.to(dev), dropout_p=dropout_p, seed=seed_t, backend="hip",
                          compute_dtype=dt if dt is not None else q.dtype)
    out.backward(up.to(dev))
    torch.cuda.synchronize()
    return dict(out=out.detach().cpu(), g_q=ql.grad.cpu(), g_kv=kvl.grad.cpu())


def _referee(q, kv, H, up, dev, mask=None, keep=None, dropout_p=0.0):
    """The reference's op sequence under autocast in the inputs' dtype.  keep (B, H, N, M) bool: dropout with that mask."""
    from fresnel_amd import slat
    dt = q.dtype
    ql, kvl = q.to(dev).requires_grad_(True), kv.to(dev).requires_grad_(True)
    mask_d = None if mask is None else mask.to(dev)
    with torch.autocast("cuda", dtype=dt):
        if keep is None:
            out = slat.cross_attention(ql, kvl, H, mask=mask_d, backend="torch")
        else:
            Bn, N, D = q.shape
            keep_d = torch.from_numpy(np.asarray(keep)).to(dev)
            k, v = kvl.permute(2, 0, 3, 1, 4)
            qh = ql.reshape(Bn, N, H, D // H).permute(0, 2, 1, 3)
            out = slat._attend_torch(qh, k, v, (D // H) ** -0.5, mask_d, lambda a: a * keep_d.to(a.dtype) / (1.0 - dropout_p), False)
    out.backward(up.to(dev).to(out.dtype))
    torch.cuda.synchronize()
    return dict(out=out.detach().cpu(), g_q=ql.grad.cpu(), g_kv=kvl.grad.cpu())


def _checker(q, kv, H, up, **kw):
    ql, kvl = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    out = AC.attend(ql, kvl, H, **kw)
    out.backward(up.double())
    return dict(out=out.detach(), g_q=ql.grad, g_kv=kvl.grad)


def _judge(tag, dt, got, ref, want, parity=False):
    """The rule.  Prints one line per tensor: the fused path's error, the referee's, their ratio."""
    lines, failures = [], []
    for k in KEYS:
        w = want[k].double().numpy()
        e, r = rel_to_max(got[k].double().numpy(), w), rel_to_max(ref[k].double().numpy(), w)
        lines.append(f"RULE {_name(dt)} {tag}: {k} fused {e:.3e} referee {r:.3e} ratio {e / r if r > 0 else (0.0 if e == 0 else float('inf')):.2f}")
        if parity and r > 16 * HALF_ULP[dt]:
            failures.append(f"{k}: the referee's own error {r:.3e} is beyond 16 half-ulps ({16 * HALF_ULP[dt]:.3e}): not a parity input")
        if e > 2.0 * r:
            failures.append(f"{k}: the fused path is {e:.3e} of the maximum away from the checker, the referee {r:.3e}")
    print("\n".join(lines))
    assert not failures, f"{_name(dt)} {tag}: " + "; ".join(failures)


def _rule_case(tag, dt, q, kv, H, up, parity=False, mask=None, dropout_p=0.0, seed=None):
    """fp32 CPU tensors -> rounded to dt, run through the three paths, judged.  -> (the fused path's tensors, the 16-bit inputs)."""
    dev = _dev()
    q, kv, up = _rounded(dt, q, kv, up)
    keep = None if not dropout_p else AC.keep_mask(seed, q.shape[0], H, q.shape[1], kv.shape[1], dropout_p)
    got = _fused(q, kv, H, up, dev, mask=mask, dropout_p=dropout_p, seed=seed)
    ref = _referee(q, kv, H, up, dev, mask=mask, keep=keep, dropout_p=dropout_p)
    want = _checker(q, kv, H, up, mask=mask, keep=keep, dropout_p=dropout_p)
    assert all(got[k].dtype is dt for k in KEYS)
    _judge(tag, dt, got, ref, want, parity=parity)
    return got, (q, kv, up)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ---- the lane map ---------------------------------------------------------------------------------------------------------------------
@gpu
@both
def test_one_mfma_tile_product(dt):
    """One 32 x 32 x 16 tile in every product: B 1, H 1, N 32, M 32, d 16.  Every query row carries a 1 in a channel of its own
    (3 n + 1 mod 16) over a small three-valued pattern, keys and values are distinct small integers (all exact in bf16): a transposed
    operand, a permuted k index on one side only or a wrong result-register map moves `out` by whole units, where the rule allows
    a few 1e-3."""
    n, c, m = torch.arange(32).reshape(32, 1), torch.arange(16).reshape(1, 16), torch.arange(32).reshape(32, 1)
    q = (0.25 * ((n + c) % 3 - 1)).float()
    q[torch.arange(32), (3 * torch.arange(32) + 1) % 16] = 1.0
    k = ((7 * m + 3 * c) % 13 - 6).float()
    v = ((5 * m + 11 * c) % 31 - 15).float()
    kv = torch.stack([k, v], dim=1).reshape(1, 32, 2, 1, 16)
    up = (((n + 2 * c) % 5) - 2).float().reshape(1, 32, 16)
    for t in (q, k, v, up):
        assert torch.equal(t.to(dt).float(), t)
    got, _ = _rule_case("one tile", dt, q.reshape(1, 32, 16), kv, 1, up)
    # and it is far from the result with the value rows reversed (a sanity check of the pattern itself)
    wrong = _checker(q.reshape(1, 32, 16).to(dt), torch.stack([k, v.flip(0)], dim=1).reshape(1, 32, 2, 1, 16).to(dt), 1, up.to(dt))
    assert rel_to_max(got["out"].double().numpy(), wrong["out"].numpy()) > 0.05


# ---- random parity at the seams -----------------------------------------------------------------------------------------------------------
# every N of {1, 31, 32, 33, 127, 128, 129, 257}, every M of {1, 7, 8, 9, 15, 16, 17, KT - 1, KT, KT + 1, 2 KT + 1, 127, 128, 129} and every
# d of {1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 64, 65, 96, 127, 128} at least once; M = 1 at d = 1 (module docstring)
SEAMS = [(1, 1, 1, 1, 1), (2, 3, 31, 7, 7), (1, 2, 32, 8, 8), (1, 1, 33, 9, 9), (1, 2, 127, 15, 15), (2, 1, 128, 16, 16),
         (1, 1, 129, 17, 17), (1, 1, 257, KT - 1, 24), (1, 2, 1, KT, 31), (1, 1, 31, KT + 1, 32), (2, 3, 32, 2 * KT + 1, 33),
         (1, 1, 33, 127, 64), (1, 1, 127, 128, 65), (1, 2, 128, 129, 96), (1, 1, 129, 1, 1), (1, 1, 257, 7, 127), (1, 1, 1, 8, 128),
         (1, 3, 31, 129, 128), (2, 2, 32, KT - 1, 64), (1, 1, 33, KT, 96), (1, 2, 127, KT + 1, 8), (1, 1, 128, 2 * KT + 1, 16),
         (1, 1, 129, 15, 32), (2, 1, 257, 129, 33), (1, 1, 32, 16, 1), (1, 1, 128, 128, 128), (1, 2, 33, 17, 65), (1, 1, 31, 9, 127),
         (1, 1, 257, 2 * KT + 1, 64), (1, 3, 129, 127, 7)]


def test_the_seam_set_covers_every_listed_size():
    assert {s[2] for s in SEAMS} == {1, 31, 32, 33, 127, 128, 129, 257}
    assert {s[3] for s in SEAMS} == {1, 7, 8, 9, 15, 16, 17, KT - 1, KT, KT + 1, 2 * KT + 1, 127, 128, 129}
    assert {s[4] for s in SEAMS} == {1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 64, 65, 96, 127, 128}
    assert all(b <= 2 and h <= 3 for b, h, *_ in SEAMS) and len(SEAMS) == 30


@gpu
@both
@pytest.mark.parametrize("Bn,H,N,M,d", SEAMS, ids=[f"B{b}H{h}N{n}M{m}d{d}" for b, h, n, m, d in SEAMS])
def test_random_parity_at_the_seams(dt, Bn, H, N, M, d):
    q, kv, up = _case(Bn, H, N, M, d, 3000 + 7 * N + 3 * M + d)
    _rule_case(f"seam B{Bn} H{H} N{N} M{M} d{d}", dt, q, kv, H, up, parity=True)


@gpu
@both
@pytest.mark.parametrize("which", ["inputs", "g_out"])
def test_a_two_byte_aligned_base_takes_the_elementwise_form_with_the_same_bits(dt, which):
    """q and kv (or the upstream gradient) as contiguous views one element into their storage: d = 16 would take the 16-byte loads,
    the base forbids them.  Judged by the rule, and bit for bit the aligned call's result (the same loops, the same roundings)."""
    from fresnel_amd.slat import cross_attention
    dev = _dev()
    Bn, H, N, M, d = 2, 2, QB + 3, KT + 5, 16
    q, kv, up = _rounded(dt, *_case(Bn, H, N, M, d, 3101))

    def off_by_one(t):
        buf = torch.empty(t.numel() + 1, dtype=dt, device=dev)
        view = buf[1:].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.storage_offset() == 1 and view.data_ptr() % 16 == 2
        return view

    ql, kvl, g = q.to(dev), kv.to(dev), up.to(dev)
    if which == "inputs":
        ql, kvl = off_by_one(ql), off_by_one(kvl)
    else:
        g = off_by_one(g)
    ql, kvl = ql.detach().requires_grad_(True), kvl.detach().requires_grad_(True)
    assert ql.data_ptr() % 16 == (2 if which == "inputs" else 0)
    out = cross_attention(ql, kvl, H, backend="hip", compute_dtype=dt)
    out.backward(g)
    torch.cuda.synchronize()
    got = dict(out=out.detach().cpu(), g_q=ql.grad.cpu(), g_kv=kvl.grad.cpu())
    _judge(f"misaligned {which}", dt, got, _referee(q, kv, H, up, dev), _checker(q, kv, H, up), parity=True)
    aligned = _fused(q, kv, H, up, dev)
    assert all(_same_bits(got[k], aligned[k]) for k in KEYS)


# ---- the online softmax's seams -------------------------------------------------------------------------------------------------------------
@gpu
@both
@pytest.mark.parametrize("kind", ["max_in_first_tile", "max_in_last_tile", "max_in_last_valid_key", "all_equal"])
def test_online_softmax_seams(dt, kind):
    """Three tiles, the last one partial (M = 2 KT + 3); five rows whose gain scales the scores, so that a spike of +30 is +3 in the
    first row (an unsaturated softmax) and +60 in the last (the spike takes everything)."""
    M = 2 * KT + 3
    s = torch.rand(M, generator=torch.Generator().manual_seed(31)) * 0.5
    gains = [0.1, 0.575, 1.05, 1.525, 2.0]
    if kind == "max_in_first_tile":
        s[3] = 30.0
    elif kind == "max_in_last_tile":
        s[2 * KT] = 30.0
    elif kind == "max_in_last_valid_key":
        s[M - 1] = 30.0
    else:
        s[:] = 0.75
        gains = [1.0, 1.25, 1.5, 1.75, 2.0]
    q, kv, up = _scored(s, 32, gains)
    got, (q16, kv16, _) = _rule_case(kind, dt, q, kv, 1, up)
    assert all(bool(torch.isfinite(got[k]).all()) for k in KEYS)
    v = kv16[0, :, 1, 0].double()
    if kind == "all_equal":   # the key's first channel is one number: equal scores exactly, the output is the mean of v rounded once
        assert rel_to_max(got["out"][0].double().numpy(), v.mean(dim=0).expand(5, 32).numpy()) <= ROUND_ONCE * HALF_ULP[dt]
    elif kind == "max_in_last_valid_key":   # with gain 2 the spike's p is 1 and every other p underflows: that value row, exactly
        assert torch.equal(got["out"][0, -1], kv16[0, M - 1, 1, 0])


# ---- beyond fp16 ----------------------------------------------------------------------------------------------------------------------------
@gpu
def test_scores_beyond_the_fp16_range_stay_finite():
    """fp16 only; the stated difference (include/fgs.h).  The product <q, k> of the spike key is 4e6 and its score 7e5, far beyond
    65504: fp32 here, so p is exactly 1 on that key and exactly 0 elsewhere (the other scores are 0: exp(-7e5) underflows) and `out` is
    that key's value row to the bit; torch's fp16 product is Inf, the row NaN, and nan_to_num makes it the mean of v.  Judged
    against the checker alone.  g_v is one fp32 sum of upstream rows rounded once; g_q and g_k are zero in exact arithmetic and
    fp32 rounding noise of dA - delta here, only required to be finite."""
    dt, dev = torch.float16, _dev()
    N, M, d, spike = 40, KT + 9, 32, KT + 2
    g = torch.Generator().manual_seed(3201)
    q = torch.zeros(1, N, d)
    q[0, :, 0] = 2000.0
    kv = torch.randn(1, M, 2, 1, d, generator=g)
    kv[0, :, 0, 0, 0] = 0.0
    kv[0, spike, 0, 0, 0] = 2000.0
    up = torch.randn(1, N, d, generator=g)
    q, kv, up = _rounded(dt, q, kv, up)
    got, want = _fused(q, kv, 1, up, dev), _checker(q, kv, 1, up)
    assert torch.equal(got["out"], kv[0, spike, 1, 0].expand(1, N, d))
    assert rel_to_max(got["out"].double().numpy(), want["out"].numpy()) == 0.0
    assert all(bool(torch.isfinite(got[k]).all()) for k in KEYS)
    e = rel_to_max(got["g_kv"][:, :, 1].double().numpy(), want["g_kv"][:, :, 1].numpy())
    print(f"beyond fp16: g_v {e:.3e}")
    assert e <= ROUND_ONCE * HALF_ULP[dt]
    ref = _referee(q, kv, 1, up, dev)["out"]
    mean_v = kv[0, :, 1, 0].double().mean(dim=0).expand(1, N, d)
    assert rel_to_max(ref.double().numpy(), mean_v.numpy()) <= 16 * HALF_ULP[dt]   # torch: the mean of v


# ---- masked rows ------------------------------------------------------------------------------------------------------------------------------
@gpu
@both
def test_masked_rows_attend_uniformly(dt):
    Bn, H, N, M, d = 2, 3, QB + 5, KT + 7, 10
    q, kv, up = _case(Bn, H, N, M, d, 3301)
    mask = _mask(Bn, N, 3302)
    got, (q16, kv16, up16) = _rule_case("masked", dt, q, kv, H, up, mask=mask)
    # p is exactly 1 for every key (all scores -1e4), the sum of v is an fp32 sum of 16-bit values, 1 / M is applied in fp32: the mean of
    # v, rounded once
    mean_v = kv16[:, :, 1].double().mean(dim=1).reshape(Bn, 1, H * d).expand(Bn, N, H * d)
    assert rel_to_max(got["out"][~mask].double().numpy(), mean_v[~mask].numpy()) <= ROUND_ONCE * HALF_ULP[dt]
    assert not got["g_q"][~mask].any() and got["g_q"][mask].any()   # exactly zero rows


# ---- the NaN rule -----------------------------------------------------------------------------------------------------------------------------
@gpu
@both
@pytest.mark.parametrize("kind", ["nan_in_q", "inf_score", "all_scores_minus_inf"])
def test_nan_rule(dt, kind):
    Bn, H, N, M, d = 2, 2, 40, KT + 5, 6
    q, kv, up = _rounded(dt, *_case(Bn, H, N, M, d, 3401))
    clean_q = q.clone()
    bad = torch.zeros(Bn, H, N, dtype=torch.bool)
    if kind == "nan_in_q":
        q[1, 7, d + 2] = float("nan")           # image 1, row 7, head 1
        bad[1, 1, 7] = True
    elif kind == "inf_score":
        q[1, 7, d + 2] = float("inf")
        bad[1, 1, 7] = True
    else:
        q[0, :, d:] = q[0, :, d:].abs() + 0.1   # head 1 of image 0: positive queries, every key -Inf -> every score -Inf
        kv[0, :, 0, 1, :] = float("-inf")
        bad[0, 1] = True
    dev = _dev()
    got = _fused(q, kv, H, up, dev, dropout_p=0.2, seed=77)
    out, g_q = got["out"].reshape(Bn, N, H, d).transpose(1, 2), got["g_q"].reshape(Bn, N, H, d).transpose(1, 2)
    mean_v = kv[:, :, 1].double().mean(dim=1).unsqueeze(2).expand(Bn, H, N, d)        # 1 / M each, without dropout
    e = rel_to_max(out[bad].double().numpy(), mean_v[bad].numpy())
    print(f"NaN rule {_name(dt)} {kind}: bad rows' out {e:.3e}")
    assert e <= ROUND_ONCE * HALF_ULP[dt]                                              # an fp32 sum of v times 1 / M, rounded once
    assert not g_q[bad].any() and g_q[~bad].any()
    assert bool(torch.isfinite(got["g_kv"]).all()) and bool(torch.isfinite(got["out"]).all()) and bool(torch.isfinite(got["g_q"]).all())
    if kind != "all_scores_minus_inf":
        # the other rows of the bad row's workgroup: bit for bit the call without the bad value
        clean = _fused(clean_q, kv, H, up, dev, dropout_p=0.2, seed=77)
        c_out, c_g_q = clean["out"].reshape(Bn, N, H, d).transpose(1, 2), clean["g_q"].reshape(Bn, N, H, d).transpose(1, 2)
        assert _same_bits(out[~bad], c_out[~bad]) and _same_bits(g_q[~bad], c_g_q[~bad])
        assert not _same_bits(out[bad], c_out[bad])


# ---- dropout ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@both
@pytest.mark.parametrize("p", [0.2, 0.5])
def test_dropout_obeys_the_stated_keep_rule(dt, p):
    Bn, H, N, M, d = 2, 3, QB + 3, 2 * KT + 3, 33
    q, kv, up = _case(Bn, H, N, M, d, 3501)
    seed = -0x0123456789ABCDEF                                                          # both halves, and the sign bit
    got, (q16, kv16, up16) = _rule_case(f"dropout {p}", dt, q, kv, H, up, dropout_p=p, seed=seed)
    again = _fused(q16, kv16, H, up16, _dev(), dropout_p=p, seed=seed)
    assert all(_same_bits(got[k], again[k]) for k in KEYS)
    other = _fused(q16, kv16, H, up16, _dev(), dropout_p=p, seed=seed + 1)
    assert not torch.equal(got["out"], other["out"])


@gpu
@pytest.mark.parametrize("p", [0.2, 0.5])
def test_the_kept_set_is_the_stated_one_in_every_precision(p):
    """Value rows are one-hot (key m in channel m, M = d): out[n, m] is key m's dropped probability, nonzero iff the key is kept
    (the scores are within +-3 of each other: no probability underflows).  The kept set is keep_mask's, and the fp32 kernels' for
    the same seed."""
    from fresnel_amd.slat import cross_attention
    dev = _dev()
    Bn, H, N, M, d, seed = 2, 2, QB + 7, 16, 16, 0x5EED0123456789
    g = torch.Generator().manual_seed(3601)
    q = torch.randn(Bn, N, H * d, generator=g) * 0.5
    kv = torch.randn(Bn, M, 2, H, d, generator=g) * 0.5
    kv[:, :, 1] = torch.eye(M).reshape(1, M, 1, d).expand(Bn, M, H, d)
    want = torch.from_numpy(AC.keep_mask(seed, Bn, H, N, M, p))
    seed_t = torch.tensor([seed], dtype=torch.int64, device=dev)
    sets = {}
    for dt in (None, torch.bfloat16, torch.float16):
        src = (q, kv) if dt is None else _rounded(dt, q, kv)
        out = cross_attention(src[0].to(dev), src[1].to(dev), H, dropout_p=p, seed=seed_t, backend="hip", compute_dtype=dt)
        sets[dt] = (out.float().cpu().reshape(Bn, N, H, d).permute(0, 2, 1, 3) != 0)
        assert torch.equal(sets[dt], want), dt
    assert abs((1.0 - float(want.float().mean())) - p) < 0.05   # (and the mask drops about p)


# ---- dtypes and launches --------------------------------------------------------------------------------------------------------------------------
def _recording(slat, calls):
    real = slat.hip.call
    # (`call` re-enters itself once with the device guard held: record the outer calls)
    slat.hip.call = lambda dev_, name_, *a: (calls.append(name_) if type(dev_) is not slat.hip.on_device else None, real(dev_, name_, *a))[1]
    return real


@gpu
@both
def test_dtypes_and_launches(dt):
    import fresnel_amd.slat as slat
    dev = _dev()
    q, kv, up = _case(2, 2, 40, 9, 8, 3701)
    calls = []
    real = _recording(slat, calls)
    try:
        # 16-bit tensors in, used as they are
        ql, kvl = q.to(dev, dt).requires_grad_(True), kv.to(dev, dt).requires_grad_(True)
        out = slat.cross_attention(ql, kvl, 2, backend="hip", compute_dtype=dt)
        assert calls == ["fgs_attn_half_forward"] and out.dtype is dt
        del calls[:]
        out.backward(up.to(dev, dt))
        assert calls == ["fgs_attn_half_backward"] and ql.grad.dtype is dt and kvl.grad.dtype is dt
        # fp32 tensors in: cast once, the gradients come back in fp32; an fp32 upstream gradient is cast once
        del calls[:]
        qf, kvf = q.to(dev).requires_grad_(True), kv.to(dev).requires_grad_(True)
        out32 = slat.cross_attention(qf, kvf, 2, backend="hip", compute_dtype=dt)
        (out32.float() * up.to(dev)).sum().backward()
        assert calls == ["fgs_attn_half_forward", "fgs_attn_half_backward"]
        assert out32.dtype is dt and qf.grad.dtype is torch.float32 and kvf.grad.dtype is torch.float32
        assert torch.equal(out32, out)   # the cast is the rounding the 16-bit leaves had
        # the module: "autocast" follows the autocast state; None stays fp32 inside autocast
        torch.manual_seed(3702)
        module = slat.CrossAttention(16, 2).to(dev).eval()
        module.backend, module.compute_dtype = "hip", "autocast"
        x, context = torch.randn(2, 40, 16, device=dev, requires_grad=True), torch.randn(2, 9, 16, device=dev)
        del calls[:]
        with torch.autocast("cuda", dtype=dt):
            y = module(x, context)
        assert calls == ["fgs_attn_half_forward"] and y.dtype is dt
        del calls[:]
        y.float().sum().backward()
        assert calls == ["fgs_attn_half_backward"] and x.grad.dtype is torch.float32
        del calls[:]
        y32 = module(x, context)
        assert calls == ["fgs_attn_forward"] and y32.dtype is torch.float32
        module.compute_dtype = None
        del calls[:]
        with torch.autocast("cuda", dtype=dt):
            inner = slat.cross_attention(ql, kvl, 2, backend="hip")
            module(x, context)
        assert calls == ["fgs_attn_forward", "fgs_attn_forward"] and inner.dtype is torch.float32
        # an explicit dtype needs no autocast: the projection then runs in the module's own dtype
        module.compute_dtype = dt
        del calls[:]
        y_explicit = module(x, context)
        assert calls == ["fgs_attn_half_forward"] and y_explicit.dtype is torch.float32
    finally:
        slat.hip.call = real


# ---- repeatability, batching, capture -----------------------------------------------------------------------------------------------------------------
@gpu
@both
def test_two_calls_and_batch_against_single_images_are_bit_identical(dt):
    Bn, H, N, M, d = 3, 2, QB + 9, KB + 5, 33
    q, kv, up = _rounded(dt, *_case(Bn, H, N, M, d, 3801))
    mask = _mask(Bn, N, 3802)
    dev = _dev()
    a, b = _fused(q, kv, H, up, dev, mask=mask), _fused(q, kv, H, up, dev, mask=mask)
    assert all(_same_bits(a[k], b[k]) for k in KEYS)
    for i in range(Bn):
        one = _fused(q[i:i + 1], kv[i:i + 1], H, up[i:i + 1], dev, mask=mask[i:i + 1])
        assert all(_same_bits(a[k][i:i + 1], one[k]) for k in KEYS), f"image {i} depends on its batch"


@gpu
@both
def test_a_captured_graph_reproduces_the_eager_bits(dt):
    """Warm-up on a side stream, capture of forward + backward (one linear chain of four launches), two replays."""
    from fresnel_amd.slat import cross_attention
    dev = _dev()
    q_c, kv_c, up_c = _rounded(dt, *_case(2, 2, QB + 1, KT + 1, 24, 3901))
    q, kv, up = q_c.to(dev).requires_grad_(True), kv_c.to(dev).requires_grad_(True), up_c.to(dev)
    mask = _mask(2, QB + 1, 3902).to(dev)
    seed = torch.tensor([3903], dtype=torch.int64, device=dev)

    def step():
        out = cross_attention(q, kv, 2, mask=mask, dropout_p=0.2, seed=seed, backend="hip", compute_dtype=dt)
        out.backward(up)
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            q.grad = kv.grad = None
            eager_out = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want = [eager_out.detach().clone(), q.grad.detach().clone(), kv.grad.detach().clone()]
    q.grad = kv.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        with torch.no_grad():
            captured.zero_()
            q.grad.zero_()
            kv.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, x, y in zip(KEYS, (captured, q.grad, kv.grad), want):
            assert _same_bits(x.cpu(), y.cpu()), f"{name}: the replay differs from the eager call"


# ---- memory ---------------------------------------------------------------------------------------------------------------------------------------
@gpu
@both
def test_no_score_tensor_is_allocated(dt):
    from fresnel_amd.slat import cross_attention
    dev = _dev()
    Bn, H, N, M, d = 1, 8, 2048, 1369, 64
    scores = Bn * H * N * M * 2                                   # one (H, N, M) tensor of the 16-bit type
    g = torch.Generator().manual_seed(4001)
    q0, kv0, up = (torch.randn(*s, generator=g).to(dev, dt) for s in ((Bn, N, H * d), (Bn, M, 2, H, d), (Bn, N, H * d)))
    io = 2 * (3 * q0.numel() + 2 * kv0.numel())                   # q, out, g_q; kv, g_kv
    q, kv = q0.clone().requires_grad_(True), kv0.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = cross_attention(q, kv, H, backend="hip", compute_dtype=dt)
    out.backward(up)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"memory rise {_name(dt)}: {rise / 2 ** 20:.1f} MiB; one 16-bit score tensor {scores / 2 ** 20:.1f} MiB, inputs and outputs {io / 2 ** 20:.1f} MiB")
    assert rise < scores + io, rise
    assert rise < scores / 4, rise                                # in fact: the outputs and two fp32 values per row, nothing else


# ---- the reference's fixtures ---------------------------------------------------------------------------------------------------------------------------
@gpu
@both
@pytest.mark.parametrize("name", ATTN_FIXTURES)
def test_fixture_inputs_through_the_half_kernels(dt, name):
    """The fixture's module, weights, inputs and mask: q and kv are its Linear layers' outputs rounded to the 16-bit type, the upstream
    gradient is the fixture's pulled back through its output projection.  The fixtures record fp32 results, to which the fp32
    tolerance applies and a 16-bit run cannot be held: judged by the rule."""
    fx = attn_fixture(name)
    H = json.loads(str(fx["ctor"]))["num_heads"]
    sd = {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sd.")}
    x, context = torch.from_numpy(fx["x"]), torch.from_numpy(fx["context"])
    q = F.linear(x, sd["q.weight"], sd["q.bias"])
    kv = F.linear(context, sd["kv.weight"], sd["kv.bias"]).reshape(x.shape[0], context.shape[1], 2, H, x.shape[2] // H)
    up = torch.from_numpy(fx["g"]) @ sd["proj.weight"]
    mask = torch.from_numpy(fx["mask"]) if "mask" in fx.files else None
    _rule_case(f"fixture {name}", dt, q, kv, H, up, mask=mask)


# ---- the distillation step under AMP ---------------------------------------------------------------------------------------------------------------------
def _amp_setup(dev, seed=4100):
    """The tiny decoder as its constructor initialises it.  (With the head's last layer scaled by 40, as the fp32 step's test does, the
    bias gradients overflow fp16 until GradScaler's scale has fallen to 8192 -- with torch's attention just the same -- and the first
    three steps are skips: profiles/cross_attention_half.txt, section 3.)"""
    from fresnel_amd.slat import DirectSLatDecoder
    torch.manual_seed(seed)
    model = DirectSLatDecoder(feature_dim=12, hidden_dim=48, num_layers=2, num_heads=2, num_gaussians_per_voxel=2, dropout=0.1,
                              head_backend="hip", attn_backend="hip", attn_dtype="autocast")
    g =torch.Generator().manual_seed(seed + 1)
    Bn, N, M = 2, 40, 12
    coord_mask = torch.ones(Bn, N, dtype=torch.bool)
    coord_mask[1, -3:] = False
    target = torch.rand(Bn, 64, 14, generator=g)
    target[..., :3] = target[..., :3] * 2 - 1
    batch = dict(features=torch.randn(Bn, M, 12, generator=g), coords=torch.randint(0, 64, (Bn, N, 4), generator=g), coord_mask=coord_mask,
                 gaussians=target, gaussian_mask=torch.ones(Bn, 64, dtype=torch.bool),
                 occupancy_target=(torch.rand(Bn, N, generator=g) > 0.5).float())
    return model.to(dev).train(), {k: v.to(dev) for k, v in batch.items()}


def _amp_steps(dt, scaler, steps):
    import fresnel_amd.slat as slat
    from fresnel_amd import distill
    dev = _dev()
    model, batch = _amp_setup(dev)
    cfg = distill.DistillConfig(head_backend="hip", match_backend="hip", amp_dtype=dt)
    loss = matching_loss_of(cfg, max_match_points=4096)
    opt = torch.optim.AdamW(model.parameters(), lr=2e-3)
    before = [p.detach().clone() for p in model.parameters()]
    calls = []
    real = _recording(slat, calls)
    try:
        losses = [distill.distill_step(model, batch, opt, loss, cfg, scaler=scaler) for _ in range(steps)]
    finally:
        slat.hip.call = real
    torch.cuda.synchronize()
    return model, before, losses, calls


@gpu
def test_distill_step_fp16_with_a_scaler():
    model, before, losses, calls = _amp_steps(torch.float16, torch.amp.GradScaler("cuda"), 3)
    assert all(np.isfinite(float(v)) for step in losses for v in step.values())
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert calls.count("fgs_attn_half_forward") == 6 and calls.count("fgs_attn_half_backward") == 6 and "fgs_attn_forward" not in calls


@gpu
def test_distill_step_bf16_without_a_scaler():
    model, before, losses, calls = _amp_steps(torch.bfloat16, None, 3)
    assert all(np.isfinite(float(v)) for step in losses for v in step.values())
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert calls.count("fgs_attn_half_forward") == 6 and calls.count("fgs_attn_half_backward") == 6 and "fgs_attn_forward" not in calls


@gpu
def test_distill_step_goes_through_the_scaler():
    """A scale of 2^60 overflows the first fp16 backward: unscale_ (before the clip) finds the Inf, scaler.step skips the optimizer, update
    halves the scale.  A step that called optimizer.step() itself, or clipped before unscaling, would move the parameters (to NaN)."""
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 60)
    model, before, losses, _ = _amp_steps(torch.float16, scaler, 1)
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert scaler.get_scale() == 2.0 ** 59
    assert np.isfinite(float(losses[0]["total"]))   # (the forward is not scaled)


# ---- limits ------------------------------------------------------------------------------------------------------------------------------------------------
@gpu
@both
def test_limits_raise_without_a_launch(dt):
    import fresnel_amd.slat as slat
    dev = _dev()
    calls = []
    real = slat.hip.call
    slat.hip.call = lambda *a: (calls.append(a[1]), real(*a))[1]
    try:
        with pytest.raises(ValueError, match="head dimension 129"):
            slat.cross_attention(torch.randn(1, 3, 129, device=dev), torch.randn(1, 2, 2, 1, 129, device=dev), 1, backend="hip",
                                 compute_dtype=dt)
        big = torch.empty(1, 1, 16, dtype=dt, device=dev).expand(1, 2 ** 27, 16)      # B H N = 2^31, no memory behind it
        with pytest.raises(ValueError, match="beyond the supported size"):
            slat.cross_attention(big, torch.empty(1, 1, 2, 16, 1, dtype=dt, device=dev), 16, backend="hip", compute_dtype=dt)
        q, kv = torch.randn(2, 5, 12, device=dev), torch.randn(2, 4, 2, 3, 4, device=dev)
        with pytest.raises(ValueError, match="dropout_p"):
            slat.cross_attention(q, kv, 3, dropout_p=1.0, backend="hip", compute_dtype=dt)
    finally:
        slat.hip.call = real
    assert calls == []
    # the library's own refusals, as clean errors
    code = slat.ATTN_HALF_DTYPES[dt]
    out, saved = torch.empty(1, 3, 129, dtype=dt, device=dev), torch.empty(256, dtype=torch.uint8, device=dev)
    with pytest.raises(B.FgsError, match="head_dim = 129"):
        real(dev, "fgs_attn_half_forward", code, 1, 3, 2, 1, 129, 1.0, 0.0, out, out, None, None, out, saved)
    with pytest.raises(B.FgsError, match="needs a seed"):
        real(dev, "fgs_attn_half_forward", code, 1, 3, 2, 1, 8, 1.0, 0.5, out, out, None, None, out, saved)
    with pytest.raises(B.FgsError, match="dtype = 7"):
        real(dev, "fgs_attn_half_forward", 7, 1, 3, 2, 1, 8, 1.0, 0.0, out, out, None, None, out, saved)
    with pytest.raises(B.FgsError, match="null pointer"):
        real(dev, "fgs_attn_half_backward", code, 1, 3, 2, 1, 8, 1.0, 0.0, out, out, None, None, out, saved, None, out, out, saved)
