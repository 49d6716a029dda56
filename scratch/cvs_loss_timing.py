"""Timing of the fused CVS loss, backend "hip" (csrc/fgs_cvs_loss.hip through fresnel_amd.cvs_losses) against the "torch" op sequence, on
one GPU: QualityAwareCVSLoss forward and forward + backward at three shapes and two configurations (the trainer's default: quality mask,
L1, consistency L1; and all four terms), the Euler step alone, and one whole cvs_step at the default model configuration, B 4, with both
loss backends.  Both backends in one process, alternating round by round, device events around `calls` back-to-back calls after 3
untimed ones.  Writes profiles/cvs_loss.txt-style text to stdout.

    PYTHONPATH=. python scratch/cvs_loss_timing.py [--rounds 7] [--calls 10] [--only loss|euler|step]

Achieved bandwidth counts ALGORITHMIC bytes of the forward: one read of pred, target, ema and depth (4 (3 C + 1) bytes per pixel),
against the 6.29 TB/s a float4 copy measures on this part (profiles/group_norm_silu.txt).  Launch counts: device activities (kernels and
copies) of one call, as torch.profiler sees them.
"""
import argparse
import statistics

import torch

SHAPES = [(4, 3, 256, 256), (8, 3, 128, 128), (8, 3, 512, 512)]
CONFIGS = {"default (mask, L1, consistency)": dict(), "all four terms": dict(lambda_boundary=0.5, lambda_gradient=0.25)}
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


def overlap(a, b):
    return "overlap" if min(a) <= max(b) and min(b) <= max(a) else "apart"


def launches(fn):
    """Device activities of one call (None where the profiler gives none)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        return n or None
    except Exception:
        return None


def inputs(shape, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    Bn, C, H, W = shape
    pred = (0.5 * torch.randn(*shape, device=dev, generator=g)).requires_grad_(True)
    target = 0.5 * torch.randn(*shape, device=dev, generator=g)
    ema = pred.detach() + 0.1 * torch.randn(*shape, device=dev, generator=g)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    depth = ((xx + yy) % 128) * 2.0 ** -9 + 0.2 * (xx >= W // 2) + 0.25
    depth = (depth[None, None] + torch.randint(-4, 5, (Bn, 1, H, W), device=dev, generator=g) * 2.0 ** -10).clamp(0, 1).float()
    return pred, target, depth, ema


def loss(dev, a):
    from fresnel_amd.cvs_losses import QualityAwareCVSLoss
    for shape in SHAPES:
        pred, target, depth, ema = inputs(shape, dev, 1)
        nbytes = 4 * (3 * pred.numel() + depth.numel())
        for title, kw in CONFIGS.items():
            fns, mods = {}, {}
            for backend in ("torch", "hip"):
                mods[backend] = QualityAwareCVSLoss(lambda_perceptual=0.0, backend=backend, **kw)

                def fwd(backend=backend):
                    with torch.no_grad():
                        return mods[backend](pred, target, depth, ema, consistency_weight_override=0.3)["total"]

                def both(backend=backend):
                    pred.grad = None
                    mods[backend](pred, target, depth, ema, consistency_weight_override=0.3)["total"].backward()

                fns[backend, "forward"], fns[backend, "forward + backward"] = fwd, both
            ref = fns["torch", "forward"]()
            e = float((fns["hip", "forward"]() - ref).abs() / ref.abs())
            grads = {}
            for backend in ("torch", "hip"):
                fns[backend, "forward + backward"]()
                grads[backend] = pred.grad.clone()
            eg = float((grads["hip"] - grads["torch"]).abs().max() / grads["torch"].abs().max())
            times = {k: [] for k in fns}
            for _ in range(a.rounds):
                for k, fn in fns.items():
                    times[k].append(timed(fn, a.calls))
            counts = {k: launches(fn) for k, fn in fns.items()}
            print(f"\nQualityAwareCVSLoss {shape}, {title}; eager, {a.calls} calls per figure; totals {e:.1e} apart, gradients {eg:.1e} of the maximum apart")
            print(f"  {'':20s} {'torch median':>12s} {'min..max':>18s} {'hip median':>12s} {'min..max':>18s}   ranges    launches torch / hip")
            for what in ("forward", "forward + backward"):
                print(f"  {what:20s} {spread(times['torch', what])}   {spread(times['hip', what])}   {overlap(times['torch', what], times['hip', what]):8s}  "
                      f"{counts['torch', what]} / {counts['hip', what]}")
            for backend in ("torch", "hip"):
                tbs = nbytes / (statistics.median(times[backend, "forward"]) * 1e-3) / 1e12
                print(f"  forward, {backend:5s}: {tbs:5.2f} TB/s of algorithmic bytes (one read of pred, target, ema, depth: {nbytes / 1e6:.1f} MB), "
                      f"{100 * tbs / COPY_TBS:4.1f} % of the {COPY_TBS} TB/s copy")
        del pred, target, depth, ema
        torch.cuda.empty_cache()


def euler(dev, a):
    from fresnel_amd.cvs_losses import consistency_euler_step
    sac = torch.sqrt(torch.cumprod(1.0 - torch.linspace(1e-4, 0.02, 1000, device=dev), dim=0))
    for shape in SHAPES:
        pred, _, _, noisy = inputs(shape, dev, 2)
        timestep = torch.randint(0, 1000, (shape[0],), device=dev)
        fns = {backend: (lambda backend=backend: consistency_euler_step(pred, noisy, sac, timestep, backend=backend)) for backend in ("torch", "hip")}
        e = float((fns["hip"]()[0] - fns["torch"]()[0]).abs().max())
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                times[k].append(timed(fn, a.calls))
        counts = {k: launches(fn) for k, fn in fns.items()}
        print(f"\nconsistency_euler_step {shape}; eager, {a.calls} calls per figure; x_prev {e:.1e} apart")
        print(f"  {'':20s} {spread(times['torch'])}   {spread(times['hip'])}   {overlap(times['torch'], times['hip']):8s}  launches {counts['torch']} / {counts['hip']}")


def step(dev, a):
    from fresnel_amd import cvs, cvs_train
    config = cvs.CVSConfig()
    Bn, size = 4, config.image_size
    g = torch.Generator(device=dev).manual_seed(3)
    _, target, depth, _ = inputs((Bn, 3, size, size), dev, 3)
    batch = dict(input_image=0.5 * torch.randn(Bn, 3, size, size, device=dev, generator=g), target_image=target.clamp(-1, 1),
                 features=torch.randn(Bn, 16, 16, 384, device=dev, generator=g), R_rel=torch.eye(3, device=dev).expand(Bn, 3, 3).contiguous(),
                 t_rel=0.1 * torch.randn(Bn, 3, device=dev, generator=g), target_depth=depth)
    print(f"\ncvs_step at the defaults (image_size {size}, channels {config.channels}), quality-aware path, B {Bn}, fp32, model backends torch: "
          "ms per step (3 steps after 1 + 3 untimed), median and min..max of the rounds")
    times = {}
    for backend in ("torch", "hip"):
        cfg = cvs_train.CVSTrainConfig(use_gaussian_targets=True, loss_backend=backend)
        torch.manual_seed(4)
        model = cvs.ConsistencyViewSynthesizer(config).to(dev)
        ema = cvs.create_ema_model(model).to(dev)
        loss_fn = cvs_train.make_cvs_loss(cfg)
        optimizer = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.01)
        one = lambda: cvs_train.cvs_step(model, ema, batch, optimizer, loss_fn, cfg, epoch=0)
        one()
        times[backend] = [timed(one, 3) for _ in range(min(a.rounds, 3))]
        print(f"  loss_backend {backend:5s}  {spread(times[backend])}")
        del model, ema, optimizer
        torch.cuda.empty_cache()
    print(f"  ranges {overlap(times['torch'], times['hip'])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--only", choices=("loss", "euler", "step"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cvs_loss_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}; {a.rounds} rounds, backends alternating; ms per call")
    for name, part in (("loss", loss), ("euler", euler), ("step", step)):
        if a.only in (None, name):
            part(dev, a)


if __name__ == "__main__":
    main()
