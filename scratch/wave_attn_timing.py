"""Timing and memory of fresnel_wave_attention (fresnel_amd/cvs.py), backend "torch" (the reference's op sequence) against "hip"
(csrc/fgs_wave_attn.hip), on one GPU, at the two shapes the reference's configurations run it at; peak memory of an
AttentionBlock(512, 384) training step with both backends; and slat.cross_attention (backend "hip") at its README shape, the figure
that must not move.  Both backends in one process, alternating round by round, device events around `calls` back-to-back calls after
3 untimed ones.  Writes profiles/wave_attention.txt-style text to stdout.

    python scratch/wave_attn_timing.py [--rounds 7] [--calls 20] [--only wave|block|cross]

`--only cross` imports nothing of fresnel_amd.cvs, so it also runs in a checkout of the commit before that module existed: the
same-visit comparison of the cross-attention on the two commits.
"""
import argparse
import statistics

import torch

SHAPES = [(4, 32, 32, 512, 8), (8, 16, 16, 512, 8)]   # (B, grid_h, grid_w, C, heads): --image_size 256 middle block; fast mode at 128^2
BLOCK = dict(B=4, grid=(32, 32), channels=512, context_dim=384, M=1369)
CROSS = dict(B=4, N=4000, M=1369, hidden=512, heads=8)   # the README's cross-attention shape


def timed(fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def row(what, t, h):
    print(f"  {what:34s} {statistics.median(t):13.4f} {min(t):8.4f}..{max(t):.4f} {statistics.median(h):12.4f} {min(h):8.4f}..{max(h):.4f}")


def wave(dev, a):
    from fresnel_amd.cvs import fresnel_wave_attention
    g = torch.Generator(device=dev).manual_seed(1)
    for Bn, gh, gw, C, heads in SHAPES:
        N = gh * gw
        qkv = torch.randn(Bn, N, 3 * C, device=dev, generator=g).requires_grad_(True)
        wl = torch.tensor(0.1, device=dev).requires_grad_(True)
        up = torch.randn(Bn, N, C, device=dev, generator=g)
        fns = {}
        for backend in ("torch", "hip"):
            def fwd(backend=backend):
                with torch.no_grad():
                    return fresnel_wave_attention(qkv, (gh, gw), wl, heads, backend=backend)

            def both(backend=backend):
                qkv.grad = wl.grad = None
                fresnel_wave_attention(qkv, (gh, gw), wl, heads, backend=backend).backward(up)

            fns[backend, "forward"], fns[backend, "forward + backward"] = fwd, both
        with torch.no_grad():
            ref = fns["torch", "forward"]()
            e = float((fns["hip", "forward"]() - ref).abs().max() / ref.abs().max())
        grads = {}
        for backend in ("torch", "hip"):
            fns[backend, "forward + backward"]()
            grads[backend] = float(wl.grad)
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                times[k].append(timed(fn, a.calls))
        print(f"\nfresnel_wave_attention, B {Bn}, grid {gh} x {gw} (N {N}), C {C}, {heads} heads (d {C // heads}); eager, {a.calls} calls per "
              f"figure; outputs {e:.1e} of the maximum apart, g_wavelength torch {grads['torch']:.6g} hip {grads['hip']:.6g}")
        print(f"  {'':34s} {'torch median':>13s} {'min..max':>17s} {'hip median':>12s} {'min..max':>17s}")
        for what in ("forward", "forward + backward"):
            row(what, times["torch", what], times["hip", what])


def block(dev, a):
    from fresnel_amd.cvs import AttentionBlock
    g = torch.Generator(device=dev).manual_seed(2)
    Bn, (gh, gw), C = BLOCK["B"], BLOCK["grid"], BLOCK["channels"]
    x = torch.randn(Bn, C, gh, gw, device=dev, generator=g)
    context = torch.randn(Bn, BLOCK["M"], BLOCK["context_dim"], device=dev, generator=g)
    print(f"\nAttentionBlock({C}, {BLOCK['context_dim']}) training forward + backward, B {Bn}, grid {gh} x {gw}, context M {BLOCK['M']}: peak of "
          "torch.cuda.max_memory_allocated above the allocation before the step, and ms per step (5 steps after 1 + 3 untimed)")
    for backend in ("torch", "hip"):
        torch.manual_seed(3)
        model = AttentionBlock(C, BLOCK["context_dim"], attn_backend=backend).to(dev).train()

        def step():
            model.zero_grad(set_to_none=True)
            model(x, context).square().mean().backward()

        step()
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ms = timed(step, 5)
        peak = torch.cuda.max_memory_allocated() - base
        print(f"  attn_backend {backend:5s}  peak {peak / 2 ** 20:9.1f} MiB   {ms:9.3f} ms per step")
        del model
        torch.cuda.empty_cache()


def cross(dev, a):
    from fresnel_amd import _binding
    from fresnel_amd.slat import cross_attention
    c = CROSS
    g = torch.Generator(device=dev).manual_seed(1)
    q = torch.randn(c["B"], c["N"], c["hidden"], device=dev, generator=g).requires_grad_(True)
    kv = torch.randn(c["B"], c["M"], 2, c["heads"], c["hidden"] // c["heads"], device=dev, generator=g).requires_grad_(True)
    up = torch.randn(c["B"], c["N"], c["hidden"], device=dev, generator=g)

    def fwd():
        with torch.no_grad():
            return cross_attention(q, kv, c["heads"], backend="hip")

    def both():
        q.grad = kv.grad = None
        cross_attention(q, kv, c["heads"], backend="hip").backward(up)

    times = {"forward": [], "forward + backward": []}
    for _ in range(a.rounds):
        times["forward"].append(timed(fwd, a.calls))
        times["forward + backward"].append(timed(both, a.calls))
    print(f"\nslat.cross_attention backend hip, B {c['B']}, N {c['N']}, M {c['M']}, hidden {c['hidden']}, {c['heads']} heads; eager, "
          f"{a.calls} calls per figure; library {_binding.LIB_PATH}")
    for what, t in times.items():
        print(f"  {what:34s} median {statistics.median(t):9.4f}   min..max {min(t):8.4f}..{max(t):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--only", choices=("wave", "block", "cross"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wave_attn_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}; {a.rounds} rounds, backends alternating; ms per call")
    for name, part in (("wave", wave), ("block", block), ("cross", cross)):
        if a.only in (None, name):
            part(dev, a)


if __name__ == "__main__":
    main()
