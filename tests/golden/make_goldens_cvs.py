"""Fixtures of the consistency view synthesizer's attention block: the reference's FresnelWaveAttention and AttentionBlock
(scripts/models/consistency_view_synthesis.py, CVS:191-288) run on the CPU, once in fp32 and once in fp64 on the same numbers.  Runs
only where the reference is present (FRESNEL_REFERENCE = its checkout); the fixtures hold data only:

    kind, ctor           "wave" (FresnelWaveAttention) | "block" (AttentionBlock); the constructor's keyword arguments, as JSON
    seed                 torch.manual_seed(seed) before the constructor gives the initial state dict
    sd0sha.<key>         SHA-256 of the bytes of every tensor of that initial state dict (what the mirror must reproduce bit for
                         bit; the digests instead of the tensors keep W4, with two 512-wide attentions, inside the size cap)
    sd.<key>             the state dict the runs used: the initial one widened (to_qkv x 3) and put on a binary grid, the wavelength as stated
    x, context           the inputs (context: block fixtures only), g the upstream gradient of the output
    out, grad.x, grad.context, grad.sd.<parameter>              the fp32 run: output and gradients of sum(out x g)
    d64.<key>, u64.<key>  the fp64 run of every <key> above, stored as its DIFFERENCE from the fp32 run: int16 counts of the unit
                          u64.<key> = max|fp64 value| x 2^-28 (tests/golden/make_goldens_attn.py; `ref64` of
                          tests/test_attn_checker.py puts the run together again).  In the block fixtures' fp64 run the two
                          GroupNorm32 keep fp32 parameters: the class casts its input to float32 whatever it is given

  W1  FresnelWaveAttention(64, heads=8), B 2, grid 5 x 7, wavelength 0.1.  Non-square on purpose: only then do the token order and
      "H, not W, in the denominator" show
  W2  FresnelWaveAttention(96, heads=2) (d = 48, a zero-padded head width), B 1, grid 16 x 16 (two query and two key blocks),
      wavelength -0.07
  W3  AttentionBlock(32, 8, use_fresnel=True), B 2, grid 4 x 6, context M 9 (the cross-attention's inner matrices are 512 wide
      whatever the channels: 32 channels and context dimension 8 keep them inside the size cap)
  W4  as W3 with use_fresnel=False

Inputs, upstream gradient and weights lie on a binary grid (multiples of 1/8 and of 1/128).  The to_qkv weights are drawn three
times wider than their initialisation, so that the softmax is far from uniform.  A seed is taken only if every self-attention score
is finite and the reference's own fp32 grad.wavelength is within 2.5e-5 of its fp64 value (a quarter of the tests' tolerance): the
script asserts both per candidate and takes the next seed otherwise.
"""
import hashlib
import json
import os
import sys

REF = os.environ.get("FRESNEL_REFERENCE", "")
if not os.path.isdir(os.path.join(REF, "scripts")):
    sys.exit("make_goldens_cvs.py: set FRESNEL_REFERENCE to a checkout of the reference; fixtures can only be generated where it is present")
sys.path.insert(0, os.path.join(REF, "scripts"))
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import models.consistency_view_synthesis as cvs  # noqa: E402  (the reference, read-only)

torch.set_num_threads(8)
META = dict(torch=torch.__version__, numpy=np.__version__, device="cpu")
CAP = os.path.getsize(os.path.join(HERE, "attn_A1.npz"))


def grid(t, step):
    return torch.round(t / step) * step


class Retry(Exception):
    pass


def build(kind, ctor):
    return cvs.FresnelWaveAttention(**ctor) if kind == "wave" else cvs.AttentionBlock(**ctor)


def wave_scores(att, h):
    """The logits of a FresnelWaveAttention for its input h (B, C, H, W), restated from CVS:211-238."""
    Bn, C, H, W = h.shape
    qkv = att.to_qkv(h.view(Bn, C, -1).permute(0, 2, 1)).chunk(3, dim=-1)
    q, k, _ = (t.view(Bn, -1, att.heads, att.dim_head).transpose(1, 2) for t in qkv)
    pos = torch.stack(torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij"), dim=-1).to(h.dtype).view(-1, 2)
    dist = torch.sqrt(((pos.unsqueeze(0) - pos.unsqueeze(1)) ** 2).sum(-1) + 1e-8)
    return q @ k.transpose(-1, -2) * att.scale + torch.cos(2 * np.pi * dist / (att.wavelength.abs() * H + 1e-6)) * 0.1


def run(kind, ctor, Bn, gh, gw, M, wavelength, seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    module = build(kind, ctor).eval()
    rec = dict(kind=np.array(kind), ctor=np.array(json.dumps(ctor)), seed=np.int32(seed))
    for k, v in module.state_dict().items():
        rec["sd0sha." + k] = np.array(hashlib.sha256(v.numpy().tobytes()).hexdigest())
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("wavelength"):
                p.fill_(wavelength)
                continue
            wide = 3.0 if "to_qkv" in name else 1.0
            p.copy_(grid(p * wide + (0.05 * torch.randn(p.shape, generator=g) if p.dim() == 1 else 0.0), 1.0 / 128))
    C = ctor["dim"] if kind == "wave" else ctor["channels"]
    x = grid(torch.randn(Bn, C, gh, gw, generator=g), 0.125)
    up = grid(torch.randn(Bn, C, gh, gw, generator=g), 0.125)
    rec.update(x=x.numpy(), g=up.numpy())
    context = None
    if kind == "block":
        context = grid(torch.randn(Bn, M, ctor["context_dim"], generator=g), 0.125)
        rec["context"] = context.numpy()
    for k, v in module.state_dict().items():
        rec["sd." + k] = v.numpy()
    for k, v in META.items():
        rec["meta_" + k] = np.array(v)
    for dtype in (torch.float32, torch.float64):
        m = build(kind, ctor).eval().to(dtype)
        m.load_state_dict({k: v.to(dtype) for k, v in module.state_dict().items()})
        for sub in m.modules():   # GroupNorm32 computes in float32 whatever it is given (x.float()): its parameters stay fp32
            if isinstance(sub, cvs.GroupNorm32):
                sub.float()
        xi = x.clone().to(dtype).requires_grad_(True)
        ci = None if context is None else context.clone().to(dtype).requires_grad_(True)
        out = m(xi) if kind == "wave" else m(xi, ci)
        (out * up.to(dtype)).sum().backward()
        with torch.no_grad():
            att = m if kind == "wave" else m.self_attn
            if isinstance(att, cvs.FresnelWaveAttention):
                if not bool(torch.isfinite(wave_scores(att, xi if kind == "wave" else m.norm1(xi))).all()):
                    raise Retry("a score is not finite")
        res = {"out": out.detach(), "grad.x": xi.grad}
        if ci is not None:
            res["grad.context"] = ci.grad
        res.update({"grad.sd." + k: p.grad for k, p in m.named_parameters()})
        for k, v in res.items():
            if dtype is torch.float32:
                rec[k] = v.numpy()
            else:
                v = v.numpy()
                unit = float(np.abs(v).max()) * 2.0 ** -28
                counts = np.rint((v - rec[k].astype(np.float64)) / unit)
                if np.abs(counts).max() > 32767:
                    raise Retry(f"{k}: the fp32 run is too far from the fp64 run for int16 counts")
                rec["d64." + k], rec["u64." + k] = counts.astype(np.int16), np.float64(unit)
                if k.endswith("wavelength") and abs(float(rec[k]) - float(v)) > 2.5e-5 * abs(float(v)):
                    raise Retry(f"{k}: fp32 {float(rec[k])!r} is more than 2.5e-5 from fp64 {float(v)!r}")
    return rec


def main():
    cases = [
        ("cvs_W1", "wave", dict(dim=64, heads=8), (2, 5, 7, 0), 0.1, 1200),
        ("cvs_W2", "wave", dict(dim=96, heads=2), (1, 16, 16, 0), -0.07, 1220),
        ("cvs_W3", "block", dict(channels=32, context_dim=8, use_fresnel=True), (2, 4, 6, 9), 0.1, 1240),
        ("cvs_W4", "block", dict(channels=32, context_dim=8, use_fresnel=False), (2, 4, 6, 9), 0.1, 1260),
    ]
    for name, kind, ctor, shape, wavelength, seed in cases:
        while True:
            try:
                rec = run(kind, ctor, *shape, wavelength, seed)
                break
            except Retry as why:
                print(f"{name}: seed {seed} refused ({why}); taking the next")
                seed += 1
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **rec)
        size = os.path.getsize(path)
        assert size <= CAP, f"{name}: {size} bytes is larger than attn_A1.npz ({CAP})"
        print(f"{name}: seed {seed}, {size / 1024:.0f} KB, |out| max {np.abs(rec['out']).max():.3f}, "
              f"fp32 vs fp64 {np.abs(rec['d64.out']).max() * 2.0 ** -28:.1e}")


if __name__ == "__main__":
    main()
