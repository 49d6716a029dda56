"""A literal torch restatement of the fused cross-attention's definition (include/fgs.h, fgs_attn_*), for any dtype and device, and
the numpy restatement of its dropout keep rule.  Not a test: tests/test_attn_checker.py holds it against the reference's fixtures,
tests/test_hip_attn.py holds the kernels against it.

    attend(q, kv, num_heads, mask=None, keep=None, dropout_p=0.0, nan_rule=False, wrong=None)
        q (B, N, H d), kv (B, M, 2, H, d) -> (B, N, H d); differentiable in q and kv.
        mask (B, N) bool: a False row has every score -1e4.  keep (B, H, N, M) bool (tensor or array): the dropout mask, applied as
        p keep / (1 - dropout_p).  nan_rule: a row whose NaN-propagating maximum is not finite gets 1 / M each, without dropout, and
        is a constant of the backward; without it the row is whatever softmax makes of it (NaN), as before the reference's cleaning.
        wrong: one rule got wrong on purpose (WRONG_RULES) -- what the fixtures must be able to tell.
    keep_mask(seed, B, H, N, M, dropout_p) -> (B, H, N, M) numpy bool, the keep rule in uint32 arithmetic.
"""
import numpy as np
import torch

WRONG_RULES = ("scale_dim", "heads_interleaved", "kv_swapped", "kv_head_major", "masked_rows_zero")


def fmix32(x):
    """murmur3's 32-bit finaliser on a numpy uint32 array."""
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def keep_threshold(dropout_p):
    """T = dropout_p (as fp32) x 2^24, rounded to nearest, ties to even (the product is exact in fp32)."""
    return int(np.rint(np.float64(np.float32(dropout_p)) * 16777216.0))


def keep_mask(seed, B, H, N, M, dropout_p):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)
    with np.errstate(over="ignore"):
        row = np.arange(B * H * N, dtype=np.uint32).reshape(B, H, N, 1)       # (b H + h) N + n
        row_hash = fmix32(row ^ lo)
        m = np.arange(M, dtype=np.uint32).reshape(1, 1, 1, M) * np.uint32(0x9E3779B1)
        x = fmix32(row_hash ^ hi ^ m)
    return (x >> np.uint32(8)) >= np.uint32(keep_threshold(dropout_p))


def attend(q, kv, num_heads, mask=None, keep=None, dropout_p=0.0, nan_rule=False, wrong=None):
    assert wrong is None or wrong in WRONG_RULES, wrong
    Bn, N, D = q.shape
    M, H = kv.shape[1], num_heads
    d = D // H
    if wrong == "heads_interleaved":
        qh = q.reshape(Bn, N, d, H).permute(0, 3, 1, 2)
        kvh = kv.reshape(Bn, M, 2, d, H).permute(2, 0, 4, 1, 3)
    elif wrong == "kv_head_major":
        qh = q.reshape(Bn, N, H, d).permute(0, 2, 1, 3)
        kvh = kv.reshape(Bn, M, H, 2, d).permute(3, 0, 2, 1, 4)
    else:
        qh = q.reshape(Bn, N, H, d).permute(0, 2, 1, 3)
        kvh = kv.reshape(Bn, M, 2, H, d).permute(2, 0, 3, 1, 4)
    k, v = (kvh[1], kvh[0]) if wrong == "kv_swapped" else (kvh[0], kvh[1])          # (B, H, M, d)
    scale = (D if wrong == "scale_dim" else d) ** -0.5
    row_open = None if mask is None else mask.to(q.device).reshape(Bn, 1, N, 1)

    def scores(qh_):
        s_ = (qh_ @ k.transpose(-2, -1)) * scale
        return s_ if row_open is None else s_.masked_fill(~row_open, -1e4)

    bad = None
    if nan_rule:
        with torch.no_grad():
            s0 = scores(qh)
            top = torch.where(torch.isnan(s0).any(dim=-1, keepdim=True), torch.full_like(s0[..., :1], float("nan")),
                              s0.max(dim=-1, keepdim=True).values)
            bad = ~torch.isfinite(top)                                               # (B, H, N, 1)
        qh = torch.where(bad, torch.zeros_like(qh), qh)                              # a bad row is a constant of the backward
    s = scores(qh)
    if bad is not None:
        s = torch.where(bad, torch.zeros_like(s), s)
    p = torch.softmax(s - s.max(dim=-1, keepdim=True).values, dim=-1)
    if keep is not None:
        keep_t = torch.as_tensor(np.asarray(keep) if not torch.is_tensor(keep) else keep).to(q.device)
        p = p * keep_t.to(p.dtype) / (1.0 - dropout_p)
    if bad is not None:
        p = torch.where(bad, torch.full_like(p, 1.0 / M), p)
    out = p @ v                                                                      # (B, H, N, d)
    if wrong == "masked_rows_zero" and row_open is not None:
        out = out * row_open.to(out.dtype)
    if wrong == "heads_interleaved":
        return out.permute(0, 2, 3, 1).reshape(Bn, N, D)
    return out.transpose(1, 2).reshape(Bn, N, D)
