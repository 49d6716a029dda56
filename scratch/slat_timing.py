"""Timing of slat_gaussian_head (fresnel_amd/slat.py), backend "torch" against "hip", on one GPU, and of DirectSLatDecoder's
occupancy-gated inference with both head backends.  The torch backend reads the host (isnan(...).any()), so it cannot be captured:
both backends are timed EAGERLY, device events around `calls` back-to-back calls, alternating, `rounds` times; the hip backend's
ungated pair is also timed as a graph replay (its device time without Python).  Writes profiles/slat_head.txt-style text to stdout.

    python scratch/slat_timing.py [--rounds 7] [--calls 100]
"""
import argparse
import statistics

import torch

from fresnel_amd.slat import DirectSLatDecoder, slat_gaussian_head

SHAPE = (4, 4000, 8)   # the reference's training default: batch_size 4, max_coords 4000, 8 Gaussians per voxel


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


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def row(what, t, h):
    print(f"  {what:34s} {statistics.median(t):13.4f} {min(t):8.4f}..{max(t):.4f} {statistics.median(h):12.4f} {min(h):8.4f}..{max(h):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slat_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    Bn, N, G = SHAPE
    print(f"device: {torch.cuda.get_device_name(0)}; {a.rounds} rounds, backends alternating; ms per call")
    g = torch.Generator(device=dev).manual_seed(1)
    raw = (torch.randn(Bn, N, G * 14, device=dev, generator=g) * 4).requires_grad_(True)
    coords = torch.randint(0, 64, (Bn, N, 4), device=dev, generator=g)
    pg, sf = torch.tensor(0.5, device=dev, requires_grad=True), torch.tensor(0.01, device=dev, requires_grad=True)
    up = torch.randn(Bn, N * G, 14, device=dev, generator=g)
    fns = {}
    for backend in ("torch", "hip"):
        def fwd(backend=backend):
            with torch.no_grad():
                return slat_gaussian_head(raw, coords, pg, sf, backend=backend)

        def both(backend=backend):
            out = slat_gaussian_head(raw, coords, pg, sf, backend=backend)
            for t in (raw, pg, sf):
                t.grad = None
            (out * up).sum().backward()

        fns[backend, "forward"], fns[backend, "forward + backward"] = fwd, both
    times = {k: [] for k in fns}
    graphs = {what: capture(fns["hip", what]) for what in ("forward", "forward + backward")}
    replay = {what: [] for what in graphs}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, a.calls))
        for what, gr in graphs.items():
            replay[what].append(timed(gr.replay, 2 * a.calls))
    print(f"\nhead alone, B {Bn}, N {N}, G {G} ({N * G} Gaussians per image); eager, {a.calls} calls per figure")
    print(f"  {'':34s} {'torch median':>13s} {'min..max':>17s} {'hip median':>12s} {'min..max':>17s}")
    for what in ("forward", "forward + backward"):
        row(what, times["torch", what], times["hip", what])
    print("  hip as a graph replay (no Python between the launches):")
    for what, t in replay.items():
        print(f"  {what:34s} {'':13s} {'':17s} {statistics.median(t):12.4f} {min(t):8.4f}..{max(t):.4f}")

    # occupancy-gated inference of the whole decoder: the reference's sizes, an untrained model (its mask is mixed)
    torch.manual_seed(2)
    model = DirectSLatDecoder(feature_dim=1024, hidden_dim=512, num_layers=6, num_heads=8, num_gaussians_per_voxel=G).to(dev).eval()
    with torch.no_grad():
        model.occupancy_head.mlp[-1].weight.mul_(50.0)
    twin = DirectSLatDecoder(feature_dim=1024, hidden_dim=512, num_layers=6, num_heads=8, num_gaussians_per_voxel=G, head_backend="hip")
    twin.load_state_dict(model.state_dict())
    twin = twin.to(dev).eval()
    features = torch.randn(Bn, 1369, 1024, device=dev, generator=g)
    mask = torch.ones(Bn, N, dtype=torch.bool, device=dev)
    kept = {}

    def infer(m, name):
        def fn():
            with torch.no_grad():
                out = m(features, coords, mask, apply_occupancy_mask=True)
            kept[name] = out["n_gaussians"]
        return fn

    runs = {"torch": infer(model, "torch"), "hip": infer(twin, "hip")}
    t2 = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            t2[k].append(timed(fn, 10))
    print(f"\nDirectSLatDecoder gated inference (hidden 512, 6 layers, M 1369, B {Bn}, N {N}, G {G}); eager, 10 calls per figure")
    print(f"  kept Gaussians per image: torch {kept['torch']}, hip {kept['hip']}")
    row("forward(apply_occupancy_mask=True)", t2["torch"], t2["hip"])


if __name__ == "__main__":
    main()
