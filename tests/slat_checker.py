"""The head of the distillation decoders (the reference's GaussianHead, scripts/models/direct_slat_decoder.py:318-358) restated
literally in torch ops, for any dtype and device: the yardstick of csrc/fgs_slat.hip (tests/test_hip_slat.py) and itself held
against the reference's fixtures S1-S4 (tests/test_slat_checker.py).

`head(raw, coords, position_offset_scale, scale_factor)` -> (B, N G, 14); `gated(...)` -> (packed, counts).  `wrong` names ONE rule
to get wrong on purpose (tests/test_slat_checker.py proves that the fixtures notice each):
    open_gate        an open instead of a closed gate at raw = +-10 (a gradient rule: only the backward differs)
    no_abs           |scale_factor| without the abs
    div63            coordinate / 63 for / 64
    no_coord_clamp   the clamp of the coordinates to [0, 63] dropped
    clamp_first      the position clamp applied to the centre, before the offset is added
    no_norm_floor    the quaternion norm without its 1e-6 floor
The NaN rule of the hip backend is `nan_rule=True`: an output that would be NaN is 0 AND a constant (nothing flows through it);
False is torch's nan_to_num, whose gradient is NaN-tainted.
"""
import torch
import torch.nn.functional as F

WRONG = ("open_gate", "no_abs", "div63", "no_coord_clamp", "clamp_first", "no_norm_floor")
GROUPS = {"position": slice(0, 3), "scale": slice(3, 6), "rotation": slice(6, 10), "colour": slice(10, 13), "opacity": slice(13, 14)}


class _OpenClamp(torch.autograd.Function):
    """clamp whose gradient passes on the OPEN interval only (the wrong rule)."""

    @staticmethod
    def forward(ctx, x, lo, hi):
        ctx.save_for_backward((x > lo) & (x < hi))
        return x.clamp(lo, hi)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


def head(raw, coords, position_offset_scale, scale_factor, wrong=None, nan_rule=False):
    assert wrong is None or wrong in WRONG, wrong
    if raw.dim() == 3:
        raw = raw.reshape(raw.shape[0], raw.shape[1], raw.shape[2] // 14, 14)
    Bn, N, G, _ = raw.shape
    dt = raw.dtype
    r = _OpenClamp.apply(raw, -10.0, 10.0) if wrong == "open_gate" else raw.clamp(-10.0, 10.0)
    xyz = coords[:, :, 1:4].to(dt)
    if wrong != "no_coord_clamp":
        xyz = xyz.clamp(0, 63)
    centre = (xyz / (63.0 if wrong == "div63" else 64.0) * 2 - 1).unsqueeze(2).expand(-1, -1, G, -1)
    offset = torch.tanh(r[..., :3]) * position_offset_scale.to(dt)
    position = centre.clamp(-1.0, 1.0) + offset if wrong == "clamp_first" else (centre + offset).clamp(-1.0, 1.0)
    gain = scale_factor.to(dt) if wrong == "no_abs" else scale_factor.to(dt).abs()
    scale = (F.softplus(r[..., 3:6]) * gain).clamp(1e-4, 1.0)
    quat = r[..., 6:10]
    norm = quat.norm(dim=-1, keepdim=True)
    rotation = quat / (norm if wrong == "no_norm_floor" else norm.clamp(min=1e-6))
    rest = torch.sigmoid(r[..., 10:14])
    out = torch.cat([position, scale, rotation, rest], dim=-1)
    if nan_rule:   # where(): the NaN branch gets no gradient and taints nobody
        bad = torch.isnan(out)
        bad = torch.cat([bad[..., :6], bad[..., 6:10].any(dim=-1, keepdim=True).expand(-1, -1, -1, 4), bad[..., 10:]], dim=-1)
        safe = torch.where(torch.isnan(raw), torch.zeros_like(raw), raw)
        if bool(bad.any()):
            clean = head(safe, coords, position_offset_scale, scale_factor, wrong=wrong).reshape(Bn, N, G, 14)
            out = torch.where(bad, torch.zeros_like(clean), clean)
    else:
        out = torch.nan_to_num(out, nan=0.0)
    return out.reshape(Bn, N * G, 14)


def gated(raw, coords, position_offset_scale, scale_factor, keep, **kw):
    """-> packed (B, N G, 14): the rows of image b's kept voxels, ascending, in front, zeros behind; counts (B,) int32."""
    out = head(raw, coords, position_offset_scale, scale_factor, **kw)
    Bn, NG, _ = out.shape
    N = keep.shape[1]
    G = NG // N
    packed = torch.zeros_like(out)
    for b in range(Bn):
        rows = out[b].reshape(N, G, 14)[keep[b]].reshape(-1, 14)
        packed[b, :rows.shape[0]] = rows
    return packed, keep.sum(dim=1).to(torch.int32)
