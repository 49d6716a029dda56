"""Fixtures of the cross-attention: the reference's CrossAttention (scripts/models/direct_slat_decoder.py, DSD:63-182) run on the
CPU in eval mode, once in fp32 and once in fp64 on the same numbers.  Runs only where the reference is present (FRESNEL_REFERENCE =
its checkout); the fixtures hold data only:

    ctor                 the constructor's keyword arguments, as JSON
    sd.<key>             the state dict
    x, context, mask     the inputs (mask: (B, N) bool, or absent), g the upstream gradient of the output
    out, grad.x, grad.context, grad.sd.<parameter>              the fp32 run: output and gradients of sum(out x g)
    d64.<key>, u64.<key>  the fp64 run of every <key> above (out, grad.x, ...), stored as its DIFFERENCE from the fp32 run: int16
                          counts of the unit u64.<key> = max|fp64 value| x 2^-28, so fp64 value = <key> + d64.<key> x u64.<key> to
                          2e-9 of the tensor's maximum (1/50 000 of the tolerance the tests use) at a quarter of the bytes.  The script
                          asserts that every count fits; tests/test_attn_checker.py `ref64` puts the run together again

  A1  dim 128, 2 heads (d = 64), B 2, N 70, M 45; masked rows in both images
  A2  dim 96, 3 heads (d = 32), B 2, N 33, M 3; no mask
  A3  dim 40, 4 heads (d = 10), chunk_size 16 with N 50, so the reference's chunked path wrote it; B 2, M 9; masked rows

Inputs, upstream gradient and weights lie on a binary grid (multiples of 1/8 and of 1/128): exact in both precisions, and the
archive compresses.  The q and kv weights are drawn three times wider than the default initialisation so that the softmax is far
from uniform and a wrong scale, a wrong head split or exchanged keys and values show (tests/test_attn_checker.py).  A seed is taken
only if every score is finite -- no row is bad in the sense of include/fgs.h -- which the script asserts.
"""
import json
import os
import sys

REF = os.environ.get("FRESNEL_REFERENCE", "")
if not os.path.isdir(os.path.join(REF, "scripts")):
    sys.exit("make_goldens_attn.py: set FRESNEL_REFERENCE to a checkout of the reference; fixtures can only be generated where it is present")
sys.path.insert(0, os.path.join(REF, "scripts"))
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import models.direct_slat_decoder as dsd  # noqa: E402  (the reference, read-only)

torch.set_num_threads(8)
META = dict(torch=torch.__version__, numpy=np.__version__, device="cpu")


def grid(t, step):
    return torch.round(t / step) * step


def run(ctor, Bn, N, M, masked, seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    dim = ctor["dim"]
    module = dsd.CrossAttention(**ctor).eval()
    with torch.no_grad():
        for name, p in module.named_parameters():
            wide = 3.0 if name.split(".")[0] in ("q", "kv") else 1.0
            p.copy_(grid(p * wide + (0.05 * torch.randn(p.shape, generator=g) if p.dim() == 1 else 0.0), 1.0 / 128))
    x = grid(torch.randn(Bn, N, dim, generator=g), 0.125)
    context = grid(torch.randn(Bn, M, dim, generator=g), 0.125)
    up = grid(torch.randn(Bn, N, dim, generator=g), 0.125)
    mask = None
    if masked:
        mask = torch.ones(Bn, N, dtype=torch.bool)
        for b, rows in enumerate(masked):
            mask[b, rows] = False
    rec = dict(ctor=np.array(json.dumps(ctor)), seed=np.int32(seed), x=x.numpy(), context=context.numpy(), g=up.numpy())
    if mask is not None:
        rec["mask"] = mask.numpy()
    for k, v in module.state_dict().items():
        rec["sd." + k] = v.numpy()
    for k, v in META.items():
        rec["meta_" + k] = np.array(v)
    for dtype, tag in ((torch.float32, ""), (torch.float64, "64")):
        m = dsd.CrossAttention(**ctor).eval().to(dtype)
        m.load_state_dict({k: v.to(dtype) for k, v in module.state_dict().items()})
        xi, ci = x.clone().to(dtype).requires_grad_(True), context.clone().to(dtype).requires_grad_(True)
        out = m(xi, ci, mask)
        (out * up.to(dtype)).sum().backward()
        with torch.no_grad():   # no row is bad: every score is finite
            H, d = m.num_heads, m.head_dim
            qh = m.q(xi).reshape(Bn, N, H, d).permute(0, 2, 1, 3)
            kh = m.kv(ci).reshape(Bn, M, 2, H, d).permute(2, 0, 3, 1, 4)[0]
            assert bool(torch.isfinite((qh @ kh.transpose(-2, -1)) * m.scale).all()), "a bad row: take another seed"
        run = {"out": out.detach(), "grad.x": xi.grad, "grad.context": ci.grad}
        run.update({"grad.sd." + k: p.grad for k, p in m.named_parameters()})
        for k, v in run.items():
            if dtype is torch.float32:
                rec[k] = v.numpy()
            else:
                v = v.numpy()
                unit = float(np.abs(v).max()) * 2.0 ** -28
                counts = np.rint((v - rec[k].astype(np.float64)) / unit)
                assert np.abs(counts).max() <= 32767, f"{k}: the fp32 run is too far from the fp64 run for int16 counts"
                rec["d64." + k], rec["u64." + k] = counts.astype(np.int16), np.float64(unit)
    return rec


def main():
    cases = [
        ("attn_A1", dict(dim=128, num_heads=2), (2, 70, 45), ([3, 31, 32, 69], [0, 64]), 1100),
        ("attn_A2", dict(dim=96, num_heads=3), (2, 33, 3), None, 1120),
        ("attn_A3", dict(dim=40, num_heads=4, chunk_size=16), (2, 50, 9), ([15, 16, 49], [0]), 1140),
    ]
    for name, ctor, shape, masked, seed in cases:
        rec = run(ctor, *shape, masked, seed)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **rec)
        print(f"{name}: seed {seed}, {os.path.getsize(path) / 1024:.0f} KB, |out| max {np.abs(rec['out']).max():.3f}, "
              f"fp32 vs fp64 {np.abs(rec['d64.out']).max() * 2.0 ** -28:.1e}")


if __name__ == "__main__":
    main()
