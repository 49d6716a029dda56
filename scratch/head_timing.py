"""Timing record of the decoders' Gaussian-parameter head (a record, not a gate): forward + backward of
fresnel_amd.decoder.gaussian_head with backend "hip" (csrc/fgs_head.hip) against backend "torch" -- the reference's expressions in
torch ops -- eager and replayed from a HIP graph, on the same GPU in the same process, alternating.

    python scratch/head_timing.py [--out profiles/decoder_head.txt] [--steps 200] [--warmup 20] [--rounds 5]

One figure = the median over `rounds` windows of the mean time of `steps` back-to-back forward + backward calls between two
device events (a single call is a few tens of microseconds: timing calls one by one would measure the event pair).  The
algorithmic bytes are computed from the shapes.  Needs a GPU; there is no fallback."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from fresnel_amd.decoder import gaussian_head  # noqa: E402

HBM_TBS = 8.0  # MI355X peak HBM bandwidth, TB/s


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_head.txt"))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="16x1369x4x19,16x377x1x19")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("head_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    lines = [f"Decoder head (gaussian_head), forward + backward, {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"each figure: median (min ... max) over {a.rounds} windows of the mean of {a.steps} back-to-back calls between two device "
             f"events, after {a.warmup} warm-up calls; the three variants alternate window by window; warm clocks, windows of "
             "milliseconds: not thermally sustained",
             "inputs: raw ~ N(0,1), pose, opacity_mod and edge present (every option of DirectPatchDecoder on); the upstream "
             "gradients of all outputs present", ""]
    for shp in a.shapes.split(","):
        Bn, P, K, C = [int(v) for v in shp.split("x")]
        g = torch.Generator(dev).manual_seed(1)
        raw = torch.randn(Bn, P, K, C, device=dev, generator=g).requires_grad_(True)
        xy = torch.rand(P, 2, device=dev, generator=g) * 2 - 1
        base_z = (-2 - 2 * torch.rand(Bn, P, device=dev, generator=g)).requires_grad_(True)
        az, el = torch.rand(Bn, device=dev, generator=g) * 6, torch.rand(Bn, device=dev, generator=g) - 0.5
        pose = torch.stack([torch.cos(az), torch.sin(az), torch.cos(el), torch.sin(el)], -1)
        mod = (0.5 + torch.rand(Bn, device=dev, generator=g)).requires_grad_(True)
        edge = torch.rand(Bn, P, device=dev, generator=g).requires_grad_(True)
        N = P * K
        ups = dict(positions=torch.randn(Bn, N, 3, device=dev, generator=g), scales=torch.randn(Bn, N, 3, device=dev, generator=g),
                   rotations=torch.randn(Bn, N, 4, device=dev, generator=g), colors=torch.randn(Bn, N, 3, device=dev, generator=g),
                   opacities=torch.randn(Bn, N, device=dev, generator=g), phases=torch.randn(Bn, N, 3, device=dev, generator=g))
        leaves = [raw, base_z, mod, edge]

        def step(backend):
            out = gaussian_head(raw, xy, base_z, pose=pose, opacity_mod=mod, edge=edge, backend=backend)
            # one backward through all outputs with the upstream gradients handed over directly: no extra kernels in the window
            return torch.autograd.grad([out[k] for k in ups if k in out], leaves, [ups[k] for k in ups if k in out])

        g_hip, g_torch = step("hip"), step("torch")
        errs = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(g_hip, g_torch)]
        # the torch form replayed from a HIP graph: its launch overhead gone, its ~130 kernels still there
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step("torch")
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step("torch")
        variants = {"hip": lambda: step("hip"), "torch eager": lambda: step("torch"), "torch graph": graph.replay}
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                ms[k].append(window(fn, a.steps))
        med = {k: statistics.median(v) for k, v in ms.items()}
        # algorithmic bytes: forward reads raw + small inputs, writes the outputs; backward reads raw and the upstream gradients,
        # writes g_raw (+ the small gradients)
        out_f = 17 if C == 19 else 14
        nbytes = 4.0 * Bn * P * K * (C + out_f + C + out_f + C)
        lines += [f"B={Bn}, P={P}, K={K}, C={C}: {Bn * N} Gaussians, {nbytes / 1e6:.2f} MB algorithmic traffic forward + backward"]
        for k in variants:
            lines.append(f"  {k:12s} {med[k] * 1e3:9.1f} us ({min(ms[k]) * 1e3:.1f} ... {max(ms[k]) * 1e3:.1f})"
                         + (f"   hip is {med[k] / med['hip']:.1f}x faster" if k != "hip" else
                            f"   {nbytes / med[k] / 1e9:.3f} TB/s = {nbytes / med[k] / 1e9 / HBM_TBS * 100:.1f} % of the {HBM_TBS} TB/s HBM peak "
                            "(launch-bound: two to three launches and the autograd node dominate)"))
        lines += ["  hip vs torch gradients (raw, base_z, opacity_mod, edge), max |diff| / max: " + " ".join(f"{e:.1e}" for e in errs), ""]
        print("\n".join(lines[-6:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
