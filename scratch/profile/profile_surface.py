"""hipEvent timing of the surface-cloud generator (fgs_surface_count + fgs_surface_emit), the source of
profiles/surface_gaussians.txt:

    python scratch/profile/profile_surface.py [--commit C] [--out profiles/surface_gaussians.txt]

Shapes 256^2 and 512^2, subsample 1, the viewer's defaults, B = 1 and 8; 5 warm-ups, 20 timed runs, median.  A timed run is the
six launches back to back on one stream between two events: the outputs are allocated beforehand with the total of a first run,
so nothing is read on the host in between.  The depth is synthetic: a smooth bowl cut by a grid of steps, about a fifth of the
pixels next to an edge.  Algorithmic bytes = depth (4 B / pixel, once) + colour (12 B / pixel, once) + 56 B per emitted row +
the per-point scratch (1 B flags written and read)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from fresnel_amd import surface  # noqa: E402

HBM_BYTES_PER_S = 8e12


def synthetic_depth(S, batch):
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    out = []
    for b in range(batch):
        cell = 19 + b                     # a step every `cell` pixels in x and y, seen by 2 of `cell` pixels per axis: 1 - (17/19)^2 = 20 %
        d = 0.2 + 0.5 * ((xx - S / 2) ** 2 + (yy - S / 2) ** 2) / (S * S / 2.0) + 0.15 * (((xx // cell) + (yy // cell)) % 2)
        out.append(np.clip(d, 0.0, 1.0) ** 0.7)
    return np.stack(out).astype(np.float32)


def measure(S, batch, dev, warmup=5, runs=20):
    depth = torch.from_numpy(synthetic_depth(S, batch)).to(dev)
    color = torch.rand(batch, 3, S, S, device=dev)
    params = surface.SurfaceGaussianParams()
    state = surface.count(depth, color, params)
    out = surface.emit(state)
    total = state.offsets_host[-1]
    flags = state.flags()
    edge_share = float(((flags & 4) != 0).float().mean())      # points past the shell threshold: "edge pixels"
    times = []
    for i in range(warmup + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st = surface.count(depth, color, params)
        surface.emit_raw(st, out, total)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1) * 1e3)
    med = statistics.median(times)
    points = batch * S * S
    nbytes = points * 4 + points * 12 + total * 56 + points * 2
    bound_us = nbytes / HBM_BYTES_PER_S * 1e6
    return dict(S=S, B=batch, rows=total, edge_share=edge_share, median_us=med, min_us=min(times), max_us=max(times), bytes=nbytes,
                bound_us=bound_us, fraction=bound_us / med)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="S,B: that shape alone (for a kernel trace)")
    ap.add_argument("--commit", default="?", help="the commit the measured tree sits on (goes into the header line)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    commit = args.commit
    lines = [f"surface_gaussians: hipEvent median of fgs_surface_count + fgs_surface_emit (6 launches), 20 runs after 5 warm-ups, "
             f"{torch.cuda.get_device_name(0)}; tree on top of commit {commit}",
             "subsample 1, viewer defaults, colour image present; 'bound' = algorithmic bytes / 8 TB/s",
             f"{'shape':>10} {'B':>2} {'Gaussians':>10} {'edge pts':>8} {'median us':>10} {'min':>8} {'max':>8} {'MB':>8} {'bound us':>9} {'of 8 TB/s':>9}"]
    shapes = [tuple(int(v) for v in args.only.split(","))] if args.only else [(S, b) for S in (256, 512) for b in (1, 8)]
    for S, batch in shapes:
        if True:
            r = measure(S, batch, dev)
            lines.append(f"{S:>6}^2   {batch:>2} {r['rows']:>10} {r['edge_share']:>8.1%} {r['median_us']:>10.1f} {r['min_us']:>8.1f} "
                         f"{r['max_us']:>8.1f} {r['bytes'] / 1e6:>8.2f} {r['bound_us']:>9.2f} {r['fraction']:>9.1%}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
