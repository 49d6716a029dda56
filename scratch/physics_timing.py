"""Timing of physics_head (fresnel_amd/decoder.py), backend "torch" against "hip", on one GPU: forward, and forward + backward,
each replayed from a captured graph.  Both backends are timed in the same process, alternating, `rounds` times; the table gives
the median and the spread of the rounds.  Writes profiles/physics_head.txt-style text to stdout.

    python scratch/physics_timing.py [--rounds 7] [--replays 200]
"""
import argparse
import statistics

import torch

from fresnel_amd.decoder import physics_head

SHAPES = ((8, 1369, 8), (8, 1369, 24))


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


def time_graph(graph, replays):
    for _ in range(20):
        graph.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / replays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("physics_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}; {a.rounds} rounds x {a.replays} graph replays, backends alternating; ms per replay")
    for Bn, P, K in SHAPES:
        g = torch.Generator(device=dev).manual_seed(1)
        raw = torch.randn(Bn, P, K, 16, device=dev, generator=g, requires_grad=True)
        xy = torch.rand(P, 2, device=dev, generator=g)
        z = (-2 - 2 * torch.rand(Bn, P, device=dev, generator=g)).requires_grad_(True)
        lam = torch.tensor(0.05, device=dev, requires_grad=True)
        ups = None
        graphs = {}
        for backend in ("torch", "hip"):
            def fwd(backend=backend):
                with torch.no_grad():
                    return physics_head(raw, xy, z, lam, backend=backend)

            def both(backend=backend):
                out = physics_head(raw, xy, z, lam, backend=backend)
                for t in (raw, z, lam):
                    t.grad = None
                sum((out[k] * ups[k]).sum() for k in out).backward()

            if ups is None:
                ups = {k: torch.rand(v.shape, device=dev, generator=g) for k, v in fwd().items()}
            graphs[backend, "forward"], graphs[backend, "forward + backward"] = capture(fwd), capture(both)
        times = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, gr in graphs.items():
                times[k].append(time_graph(gr, a.replays))
        print(f"\nB {Bn}, P {P}, K {K} (N = {P * K} Gaussians per image)")
        print(f"  {'':20s} {'torch median':>13s} {'min..max':>17s} {'hip median':>12s} {'min..max':>17s}")
        for what in ("forward", "forward + backward"):
            t, h = times["torch", what], times["hip", what]
            print(f"  {what:20s} {statistics.median(t):13.4f} {min(t):8.4f}..{max(t):.4f} {statistics.median(h):12.4f} {min(h):8.4f}..{max(h):.4f}")


if __name__ == "__main__":
    main()
