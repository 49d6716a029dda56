"""Timing record of the NCA decoder (a record, not a gate): forward + backward of fresnel_amd.decoder.NCAGaussianDecoder at the
reference's defaults (377 points, k = 6, 16 steps, 384-channel 37 x 37 features) and 16 images, training mode, with nca_backend
"hip" (csrc/fgs_nca.hip) against "torch" -- the reference's own cdist / topk / gather sequence -- eager and replayed from a HIP
graph, on the same GPU in the same process, the variants alternating window by window.

    python scratch/nca_timing.py [--out profiles/nca_decoder.txt] [--steps 20] [--warmup 5] [--rounds 7] [--head_backend torch]

One figure = the median (min ... max) over `rounds` windows of the mean time of `steps` back-to-back forward + backward calls
between two device events.  The MLPs and the head are the same code under both backends (rocBLAS through torch; the head backend
is held fixed), so the difference is the neighbour perception and the update.  Needs a GPU; there is no fallback."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from fresnel_amd.decoder import NCAGaussianDecoder  # noqa: E402


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nca_decoder.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--head_backend", default="torch")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nca_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = torch.Generator(dev).manual_seed(1)
    features = torch.randn(a.batch, 384, 37, 37, device=dev, generator=g).requires_grad_(True)
    depth = torch.rand(a.batch, 1, 64, 64, device=dev, generator=g)
    models = {}
    for backend in ("torch", "hip"):
        torch.manual_seed(2)
        m = NCAGaussianDecoder(nca_backend=backend, head_backend=a.head_backend).to(dev).train()
        with torch.no_grad():  # a trained automaton moves its points: the fresh one's last layer is zero
            m.update_rule[-1].weight.normal_(0.0, 0.15)
        models[backend] = m
    ups = None

    def step(backend):
        nonlocal ups
        m = models[backend]
        out = m(features, depth)
        if ups is None:
            ups = {k: torch.randn(v.shape, device=dev, generator=g) for k, v in out.items()}
        # one backward through all outputs with the upstream gradients handed over directly: no extra kernels in the window
        return torch.autograd.grad(list(out.values()), [features] + list(m.parameters()), [ups[k] for k in out], allow_unused=True)

    variants, graphs = {}, {}
    for backend in ("torch", "hip"):
        variants[backend + " eager"] = (lambda b=backend: step(b))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for backend in ("torch", "hip"):
            for _ in range(3):
                step(backend)
    torch.cuda.current_stream().wait_stream(side)
    for backend in ("torch", "hip"):
        graphs[backend] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[backend]):
            step(backend)
        variants[backend + " graph"] = graphs[backend].replay
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            ms[k].append(window(fn, a.steps))
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines = [f"NCA decoder (NCAGaussianDecoder), forward + backward, {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"B={a.batch}, 377 points, k=6, 16 steps, state 16, hidden 128, features (B, 384, 37, 37), training mode, head_backend "
             f"{a.head_backend} under both",
             f"each figure: median (min ... max) over {a.rounds} windows of the mean of {a.steps} back-to-back calls between two device "
             f"events, after {a.warmup} warm-up calls; the four variants alternate window by window; warm clocks, windows of tens of "
             "milliseconds: not thermally sustained", ""]
    for k in variants:
        lines.append(f"  {k:12s} {med[k]:8.3f} ms ({min(ms[k]):.3f} ... {max(ms[k]):.3f}; spread {max(ms[k]) - min(ms[k]):.3f})")
    for mode in ("eager", "graph"):
        t, h = "torch " + mode, "hip " + mode
        spread = max(max(ms[t]) - min(ms[t]), max(ms[h]) - min(ms[h]))
        lines.append(f"  {mode}: hip saves {med[t] - med[h]:.3f} ms of {med[t]:.3f} ({med[t] / med[h]:.2f}x); largest spread over rounds "
                     f"{spread:.3f} ms -> {'faster by more than the spread' if min(ms[t]) - max(ms[h]) > 0 else 'NOT separated from the spread'}")
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
