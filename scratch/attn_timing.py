"""Timing and memory of cross_attention (fresnel_amd/slat.py), backend "torch" (the reference's op sequence, queries in chunks of
1024 as its CrossAttention runs them) against "hip" (csrc/fgs_attn.hip), on one GPU; peak memory of a six-block training forward +
backward of DirectSLatDecoder with both attention backends; and the decoder's occupancy-gated inference (fused head) with both.
Both backends in one process, alternating round by round, device events around `calls` back-to-back calls after 3 untimed ones.
Writes profiles/cross_attention.txt-style text to stdout.

    python scratch/attn_timing.py [--rounds 7] [--calls 20]
"""
import argparse
import statistics

import torch

from fresnel_amd.slat import DirectSLatDecoder, cross_attention

BN, N, M, HIDDEN, HEADS, CHUNK = 4, 4000, 1369, 512, 8, 1024   # the reference's training shape (batch_size 4, max_coords 4000, 37 x 37 patches)


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


def attend(q, kv, backend):
    if backend == "hip":
        return cross_attention(q, kv, HEADS, backend="hip")
    return torch.cat([cross_attention(q[:, i:i + CHUNK], kv, HEADS, backend="torch") for i in range(0, N, CHUNK)], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}; {a.rounds} rounds, backends alternating; ms per call")
    g = torch.Generator(device=dev).manual_seed(1)
    q = torch.randn(BN, N, HIDDEN, device=dev, generator=g).requires_grad_(True)
    kv = torch.randn(BN, M, 2, HEADS, HIDDEN // HEADS, device=dev, generator=g).requires_grad_(True)
    up = torch.randn(BN, N, HIDDEN, device=dev, generator=g)
    fns = {}
    for backend in ("torch", "hip"):
        def fwd(backend=backend):
            with torch.no_grad():
                return attend(q, kv, backend)

        def both(backend=backend):
            q.grad = kv.grad = None
            attend(q, kv, backend).backward(up)

        fns[backend, "forward"], fns[backend, "forward + backward"] = fwd, both
    with torch.no_grad():
        e = float((attend(q, kv, "hip") - attend(q, kv, "torch")).abs().max() / attend(q, kv, "torch").abs().max())
    times = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, a.calls))
    print(f"\nattention alone, B {BN}, N {N}, M {M}, hidden {HIDDEN}, {HEADS} heads (d {HIDDEN // HEADS}); eager, {a.calls} calls per figure; "
          f"torch in chunks of {CHUNK} queries; outputs {e:.1e} of the maximum apart")
    print(f"  {'':34s} {'torch median':>13s} {'min..max':>17s} {'hip median':>12s} {'min..max':>17s}")
    for what in ("forward", "forward + backward"):
        row(what, times["torch", what], times["hip", what])

    # a six-block training forward + backward: peak memory above what is allocated before the step
    ctor = dict(feature_dim=1024, hidden_dim=HIDDEN, num_layers=6, num_heads=HEADS, num_gaussians_per_voxel=8)
    features = torch.randn(BN, M, 1024, device=dev, generator=g)
    coords = torch.randint(0, 64, (BN, N, 4), device=dev, generator=g)
    mask = torch.ones(BN, N, dtype=torch.bool, device=dev)
    print(f"\nDirectSLatDecoder training forward + backward (6 blocks, dropout 0.1, no checkpointing, B {BN}, N {N}, M {M}): peak of "
          "torch.cuda.max_memory_allocated above the allocation before the step, and ms per step (3 steps after 1 untimed)")
    for backend in ("torch", "hip"):
        torch.manual_seed(2)
        model = DirectSLatDecoder(**ctor, attn_backend=backend).to(dev).train()

        def step():
            model.zero_grad(set_to_none=True)
            out = model(features, coords, mask)
            (out["gaussians"].square().mean() + out["occupancy_logits"].square().mean()).backward()

        step()
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ms = timed(step, 3)
        peak = torch.cuda.max_memory_allocated() - base
        print(f"  attn_backend {backend:5s}  peak {peak / 2 ** 30:7.2f} GiB   {ms:9.2f} ms per step")
        del model
        torch.cuda.empty_cache()

    # occupancy-gated inference with the fused head: the attention backend is the only difference
    models = {}
    for backend in ("torch", "hip"):
        torch.manual_seed(2)
        m = DirectSLatDecoder(**ctor, head_backend="hip", attn_backend=backend)
        with torch.no_grad():
            m.occupancy_head.mlp[-1].weight.mul_(50.0)
        models[backend] = m.to(dev).eval()
    kept = {}

    def infer(m, name):
        def fn():
            with torch.no_grad():
                kept[name] = m(features, coords, mask, apply_occupancy_mask=True)["n_gaussians"]
        return fn

    runs = {k: infer(m, k) for k, m in models.items()}
    t2 = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            t2[k].append(timed(fn, 10))
    print(f"\nDirectSLatDecoder gated inference (hidden {HIDDEN}, 6 layers, M {M}, B {BN}, N {N}, G 8, head_backend hip); eager, 10 calls per figure")
    print(f"  kept Gaussians per image: attn torch {kept['torch']}, attn hip {kept['hip']}")
    row("forward(apply_occupancy_mask=True)", t2["torch"], t2["hip"])


if __name__ == "__main__":
    main()
