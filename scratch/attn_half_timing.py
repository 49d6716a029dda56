"""Timing and memory of the 16-bit fused cross-attention (csrc/fgs_attn_half.hip; cross_attention(..., backend="hip",
compute_dtype=fp16 | bf16)) on one GPU, at the reference's training shape, against two baselines taken in the same process:
  1. the fp32 fused path (csrc/fgs_attn.hip, compute_dtype=None) on fp32 tensors;
  2. the reference's op sequence (backend "torch") under torch.autocast in that dtype, queries in chunks of 1024 as its
     CrossAttention runs them.
Then the peak memory of a six-block training forward + backward of DirectSLatDecoder, and the whole distill_step under AMP (fp16 with a
GradScaler, bf16 without) against the fp32 step with every backend on "hip" and against the AMP step with the attention on "torch".
Eager mode, device events around `calls` back-to-back calls after 3 untimed ones, the variants alternating round by round; median
(min..max) over the rounds.  Writes profiles/cross_attention_half.txt-style text to stdout.

    python scratch/attn_half_timing.py [--rounds 7] [--calls 20]
"""
import argparse
import statistics

import torch

from fresnel_amd import distill
from fresnel_amd.losses import GaussianMatchingLoss
from fresnel_amd.slat import DirectSLatDecoder, cross_attention

BN, N, M, HIDDEN, HEADS, CHUNK = 4, 4000, 1369, 512, 8, 1024   # batch_size 4, max_coords 4000, 37 x 37 patches
NAMES = {torch.float16: "fp16", torch.bfloat16: "bf16"}


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


def show(what, t):
    print(f"  {what:58s} {statistics.median(t):9.4f}  ({min(t):.4f}..{max(t):.4f})")


def attend(q, kv, how, dt):
    if how == "hip":
        return cross_attention(q, kv, HEADS, backend="hip", compute_dtype=dt)
    with torch.autocast("cuda", dtype=dt):
        return torch.cat([cross_attention(q[:, i:i + CHUNK], kv, HEADS, backend="torch") for i in range(0, N, CHUNK)], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_half_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}; {a.rounds} rounds, variants alternating; ms per call, median (min..max)")
    g = torch.Generator(device=dev).manual_seed(1)
    d = HIDDEN // HEADS
    q32 = torch.randn(BN, N, HIDDEN, device=dev, generator=g)
    kv32 = torch.randn(BN, M, 2, HEADS, d, device=dev, generator=g)
    up32 = torch.randn(BN, N, HIDDEN, device=dev, generator=g)
    fns = {}
    for name, dt, how in [("fp32 fused (hip)", None, "hip")] + [(f"{NAMES[t]} {h}", t, h) for t in NAMES for h in ("hip", "torch")]:
        cast = (lambda t: t) if dt is None else (lambda t, dt=dt: t.to(dt))
        q, kv, up = cast(q32).requires_grad_(True), cast(kv32).requires_grad_(True), cast(up32)

        def fwd(q=q, kv=kv, how=how, dt=dt):
            with torch.no_grad():
                return attend(q, kv, how, dt)

        def both(q=q, kv=kv, up=up, how=how, dt=dt):
            q.grad = kv.grad = None
            attend(q, kv, how, dt).backward(up)

        fns[name, "forward"], fns[name, "forward + backward"] = fwd, both
    times = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, a.calls))
    ref = fns["fp32 fused (hip)", "forward"]().double()
    print(f"\nattention alone, B {BN}, N {N}, M {M}, hidden {HIDDEN}, {HEADS} heads (d {d}); eager, {a.calls} calls per figure; torch under "
          f"autocast in chunks of {CHUNK} queries")
    for what in ("forward", "forward + backward"):
        print(f" {what}")
        for name in dict.fromkeys(k[0] for k in fns):
            show(name, times[name, what])
    for t in NAMES:
        e = {h: float((fns[f"{NAMES[t]} {h}", "forward"]().double() - ref).abs().max() / ref.abs().max()) for h in ("hip", "torch")}
        print(f"  {NAMES[t]} forward against the fp32 fused output (which saw unrounded inputs), of the maximum: hip {e['hip']:.1e}, torch {e['torch']:.1e}")

    # a six-block training forward + backward: peak memory above what is allocated before the step
    ctor = dict(feature_dim=1024, hidden_dim=HIDDEN, num_layers=6, num_heads=HEADS, num_gaussians_per_voxel=8)
    features = torch.randn(BN, M, 1024, device=dev, generator=g)
    coords = torch.randint(0, 64, (BN, N, 4), device=dev, generator=g)
    mask = torch.ones(BN, N, dtype=torch.bool, device=dev)
    print(f"\nDirectSLatDecoder training forward + backward (6 blocks, dropout 0.1, no checkpointing, B {BN}, N {N}, M {M}): peak of "
          "torch.cuda.max_memory_allocated above the allocation before the step, and ms per step (3 steps after 1 untimed)")
    for label, backend, amp in [("fp32, attn hip", "hip", None)] + [(f"autocast {NAMES[t]}, attn {b}", b, t) for t in NAMES for b in ("hip", "torch")]:
        torch.manual_seed(2)
        model = DirectSLatDecoder(**ctor, attn_backend=backend, attn_dtype="autocast").to(dev).train()

        def step():
            model.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=amp or torch.float16, enabled=amp is not None):
                out = model(features, coords, mask)
                loss = out["gaussians"].float().square().mean() + out["occupancy_logits"].float().square().mean()
            loss.backward()

        step()
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ms = timed(step, 3)
        peak = torch.cuda.max_memory_allocated() - base
        print(f"  {label:28s}  peak {peak / 2 ** 30:7.2f} GiB   {ms:9.2f} ms per step")
        del model
        torch.cuda.empty_cache()

    # the whole distillation step
    target = torch.rand(BN, 8192, 14, device=dev, generator=g)
    target[..., :3] = target[..., :3] * 2 - 1
    batch = dict(features=features, coords=coords, coord_mask=mask, gaussians=target,
                 gaussian_mask=torch.ones(BN, 8192, dtype=torch.bool, device=dev),
                 occupancy_target=(torch.rand(BN, N, device=dev, generator=g) > 0.5).float())
    steps = {}
    for label, attn, amp, scaled in [("fp32, all hip", "hip", None, False), ("fp16 + GradScaler, attn hip", "hip", torch.float16, True),
                                     ("fp16 + GradScaler, attn torch", "torch", torch.float16, True),
                                     ("bf16, attn hip", "hip", torch.bfloat16, False), ("bf16, attn torch", "torch", torch.bfloat16, False)]:
        torch.manual_seed(3)
        model = DirectSLatDecoder(**ctor, head_backend="hip", attn_backend=attn, attn_dtype="autocast").to(dev).train()
        cfg = distill.DistillConfig(head_backend="hip", match_backend="hip", amp_dtype=amp)
        loss = GaussianMatchingLoss(position_weight=cfg.position_weight, scale_weight=cfg.scale_weight, rotation_weight=cfg.rotation_weight,
                                    color_weight=cfg.color_weight, opacity_weight=cfg.opacity_weight, backend="hip")
        opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
        scaler = torch.amp.GradScaler("cuda") if scaled else None
        steps[label] = lambda model=model, cfg=cfg, loss=loss, opt=opt, scaler=scaler: distill.distill_step(model, batch, opt, loss, cfg, scaler=scaler)
    t3 = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            t3[k].append(timed(fn, 5))
    print(f"\ndistill_step (6 blocks, hidden {HIDDEN}, G 8, B {BN}, N {N}, M {M}, 8192 target Gaussians, head and match on hip, AdamW); eager, "
          "5 steps per figure")
    for k in steps:
        show(k, t3[k])


if __name__ == "__main__":
    main()
