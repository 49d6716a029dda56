"""The host side of the 16-bit fused cross-attention and of the AMP distillation step, without a GPU: the header and the binding
carry the three entry points and the two dtype constants, `cross_attention` / `CrossAttention` / `DirectSLatDecoder` /
`DistillConfig` / `distill_step` take and validate the new arguments, and with both new arguments None the step is today's step
bit for bit."""
import copy
import re

import pytest
import torch

from helpers import ROOT
from test_slat_mirror import _distill_batch, build_mirror, fixture, matching_loss_of

from fresnel_amd import _binding as B

NAMES = ("fgs_attn_half_workspace_bytes", "fgs_attn_half_forward", "fgs_attn_half_backward")


def test_header_and_binding_carry_the_entry_points_and_constants():
    txt = open(f"{ROOT}/include/fgs.h").read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in B.SIGNATURES and name in B.EXPORTED_SYMBOLS
    for macro, value in (("FGS_ATTN_F16", 1), ("FGS_ATTN_BF16", 2)):
        assert re.search(rf"^#define {macro} {value}\s*$", code, flags=re.M), macro
        assert getattr(B, macro) == value
    m = re.search(r"^#define FGS_ATTN_HALF_KEY_TILE (\d+)\s*$", code, flags=re.M)
    assert m and int(m[1]) == B.FGS_ATTN_HALF_KEY_TILE and int(m[1]) in (32, 64)
    # dtype leads the two launching calls; the pointer lists are the fp32 entry points'
    for half, full in (("fgs_attn_half_forward", "fgs_attn_forward"), ("fgs_attn_half_backward", "fgs_attn_backward")):
        assert B.SIGNATURES[half] == ("int", (("int32_t", "dtype"),) + B.SIGNATURES[full][1])
    assert B.SIGNATURES[NAMES[0]] == ("int", B.SIGNATURES["fgs_attn_workspace_bytes"][1])


def test_cross_attention_validates_compute_dtype():
    from fresnel_amd.slat import cross_attention
    q, kv = torch.randn(1, 3, 8), torch.randn(1, 2, 2, 2, 4)
    assert cross_attention(q, kv, 2, backend="torch", compute_dtype=None).shape == (1, 3, 8)
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match="compute_dtype"):
            cross_attention(q, kv, 2, backend="torch", compute_dtype=dt)
    for bad in (torch.float64, torch.float32, "bfloat16", "autocast"):
        for backend in ("torch", "hip"):
            with pytest.raises(ValueError, match="compute dtype"):
                cross_attention(q, kv, 2, backend=backend, compute_dtype=bad)
    # a good dtype on the hip backend gets as far as the device check: there is no CPU fallback
    with pytest.raises(B.FgsError, match="no CPU fallback"):
        cross_attention(q, kv, 2, backend="hip", compute_dtype=torch.bfloat16)


def test_modules_carry_and_validate_the_attention_dtype():
    from fresnel_amd.slat import CrossAttention, DirectSLatDecoder
    module = CrossAttention(8, 2)
    assert module.compute_dtype is None
    ctor = dict(feature_dim=6, hidden_dim=12, num_layers=2, num_heads=2, num_gaussians_per_voxel=2)
    assert all(b.cross_attn.compute_dtype is None for b in DirectSLatDecoder(**ctor).blocks)
    for dt in (torch.float16, torch.bfloat16, "autocast"):
        model = DirectSLatDecoder(**ctor, attn_backend="hip", attn_dtype=dt)
        assert model.attn_dtype == dt and all(b.cross_attn.compute_dtype == dt for b in model.blocks)
    for bad in ("nope", torch.float64, 16):
        with pytest.raises(ValueError, match="compute dtype"):
            DirectSLatDecoder(**ctor, attn_dtype=bad)
    # the torch backend never reads the attribute; the hip backend validates it at the call
    module.compute_dtype = "nope"
    assert module(torch.randn(1, 3, 8), torch.randn(1, 2, 8)).shape == (1, 3, 8)
    module.backend = "hip"
    with pytest.raises(ValueError, match="compute dtype"):
        module(torch.randn(1, 3, 8), torch.randn(1, 2, 8))
    # "autocast" outside autocast is fp32: the call gets as far as the device check of the fp32 path
    module.compute_dtype = "autocast"
    assert module._hip_compute_dtype() is None
    with pytest.raises(B.FgsError, match="no CPU fallback"):
        module(torch.randn(1, 3, 8), torch.randn(1, 2, 8))


def test_distill_config_and_the_scaler_check():
    from fresnel_amd import distill
    assert distill.DistillConfig().amp_dtype is None
    assert distill.DistillConfig(amp_dtype=torch.float16).amp_dtype is torch.float16

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"touched: {name}")

        def __call__(self, *a, **kw):
            raise AssertionError("called")

    with pytest.raises(ValueError, match="amp_dtype"):
        distill.distill_step(Untouchable(), Untouchable(), Untouchable(), Untouchable(), distill.DistillConfig(), scaler=object())


def test_without_amp_the_step_is_the_earlier_step_bit_for_bit():
    from fresnel_amd import distill
    cfg = distill.DistillConfig()
    fx = fixture("slat_S1")
    model, _ = build_mirror(fx)
    model.train()
    twin = copy.deepcopy(model)
    batch = _distill_batch(fx, torch.Generator().manual_seed(12))
    loss = matching_loss_of(cfg)
    opt, opt_twin = (torch.optim.AdamW(m.parameters(), lr=1e-3) for m in (model, twin))
    for step in range(2):
        torch.manual_seed(500 + step)   # (the dropout modules draw from the global generator)
        got = distill.distill_step(model, batch, opt, loss, cfg, scaler=None)
        torch.manual_seed(500 + step)
        # the step as it stood before AMP, literally
        opt_twin.zero_grad()
        output = twin(batch["features"], batch["coords"], batch.get("coord_mask"))
        losses = distill.distill_losses(output, batch, loss, cfg)
        losses["total"].backward()
        torch.nn.utils.clip_grad_norm_(twin.parameters(), cfg.grad_clip)
        opt_twin.step()
        want = {k: v.detach() for k, v in losses.items()}
        assert sorted(got) == sorted(want) and all(torch.equal(got[k], want[k]) for k in want)
        for (k, p), r in zip(model.named_parameters(), twin.parameters()):
            assert torch.equal(p.detach(), r.detach()), k
    assert any(not torch.equal(p.detach(), torch.from_numpy(fx["sd." + k])) for k, p in model.named_parameters())
