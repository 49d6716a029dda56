"""Timing of fresnel_amd.cvs.group_norm_act, backend "hip" (csrc/fgs_gn_silu.hip) against the torch op sequence (add, group_norm,
silu), on one GPU, at the four activation shapes of the consistency view synthesizer's U-Net at B 4; and a whole ConsistencyUNet
training step at the reference's defaults, B 4, with both norm_backends: time and peak memory.  Both backends in one process,
alternating round by round, device events around `calls` back-to-back calls after 3 untimed ones.  Writes
profiles/group_norm_silu.txt-style text to stdout.

    PYTHONPATH=. python scratch/gn_silu_timing.py [--rounds 7] [--calls 10] [--only norm|unet]

Achieved bandwidth counts ALGORITHMIC bytes: one read and one write of the activation forward (8 bytes per element), against the
6.29 TB/s a float4 copy measures on this part.
"""
import argparse
import statistics

import torch

SHAPES = [(4, 128, 256, 256), (4, 256, 256, 256), (4, 512, 32, 32), (4, 1024, 32, 32)]
COPY_TBS = 6.29


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


def spread(t):
    return f"{statistics.median(t):9.4f} {min(t):8.4f}..{max(t):<8.4f}"


def norm(dev, a):
    from fresnel_amd.cvs import group_norm_act
    g = torch.Generator(device=dev).manual_seed(1)
    for shape in SHAPES:
        Bn, C = shape[:2]
        x = torch.randn(*shape, device=dev, generator=g).requires_grad_(True)
        cb = torch.randn(Bn, C, device=dev, generator=g).requires_grad_(True)
        w = (1 + 0.1 * torch.randn(C, device=dev, generator=g)).requires_grad_(True)
        b = (0.1 * torch.randn(C, device=dev, generator=g)).requires_grad_(True)
        up = torch.randn(*shape, device=dev, generator=g)
        leaves = (x, cb, w, b)
        fns = {}
        for backend in ("torch", "hip"):
            def fwd(backend=backend):
                with torch.no_grad():
                    return group_norm_act(x, 32, w, b, channel_bias=cb, backend=backend)

            def both(backend=backend):
                for t in leaves:
                    t.grad = None
                group_norm_act(x, 32, w, b, channel_bias=cb, backend=backend).backward(up)

            fns[backend, "forward"], fns[backend, "forward + backward"] = fwd, both
        with torch.no_grad():
            ref = fns["torch", "forward"]()
            e = float((fns["hip", "forward"]() - ref).abs().max() / ref.abs().max())
            del ref
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                times[k].append(timed(fn, a.calls))
        nbytes = 8 * x.numel()
        print(f"\ngroup_norm_act {shape}, 32 groups, channel_bias, SiLU; eager, {a.calls} calls per figure; outputs {e:.1e} of the maximum apart")
        print(f"  {'':20s} {'torch median':>12s} {'min..max':>18s} {'hip median':>12s} {'min..max':>18s}")
        for what in ("forward", "forward + backward"):
            print(f"  {what:20s} {spread(times['torch', what])}   {spread(times['hip', what])}")
        for backend in ("torch", "hip"):
            tbs = nbytes / (statistics.median(times[backend, "forward"]) * 1e-3) / 1e12
            print(f"  forward, {backend:5s}: {tbs:5.2f} TB/s of algorithmic bytes (one read + one write), {100 * tbs / COPY_TBS:4.1f} % of the {COPY_TBS} TB/s copy")
        del x, up
        torch.cuda.empty_cache()


def unet(dev, a):
    from fresnel_amd.cvs import ConsistencyUNet, CVSConfig
    config = CVSConfig()
    g = torch.Generator(device=dev).manual_seed(2)
    Bn, size, D = 4, config.image_size, config.cross_attention_dim
    x = torch.randn(Bn, 3, size, size, device=dev, generator=g)
    t = torch.tensor([10.0, 300.0, 600.0, 999.0], device=dev)
    image_cond = torch.randn(Bn, 256, D, device=dev, generator=g)
    pose_cond = torch.randn(Bn, 16, D, device=dev, generator=g)
    print(f"\nConsistencyUNet at the defaults (image_size {size}, channels {config.channels}), training forward + backward, B {Bn}, fp32, "
          "attn_backend torch: ms per step (3 steps after 1 + 3 untimed) and peak of torch.cuda.max_memory_allocated above the allocation "
          "before the step")
    for backend in ("torch", "hip"):
        torch.manual_seed(3)
        model = ConsistencyUNet(config, norm_backend=backend).to(dev).train()

        def step():
            model.zero_grad(set_to_none=True)
            model(x, t, image_cond, pose_cond).square().mean().backward()

        step()
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ms = timed(step, 3)
        peak = torch.cuda.max_memory_allocated() - base
        print(f"  norm_backend {backend:5s}  {ms:9.2f} ms per step   peak {peak / 2 ** 30:7.2f} GiB")
        del model
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--only", choices=("norm", "unet"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gn_silu_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}; {a.rounds} rounds, backends alternating; ms per call")
    for name, part in (("norm", norm), ("unet", unet)):
        if a.only in (None, name):
            part(dev, a)


if __name__ == "__main__":
    main()
