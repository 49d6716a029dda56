"""hipEvent timing of the feature-guided SAAG emit and its backward (fgs_surface_emit_guided, fgs_surface_guided_backward), the
source of profiles/surface_guided.txt:

    python scratch/profile/profile_surface_guided.py [--commit C] [--out profiles/surface_guided.txt] [--train]
    rocprofv3 --kernel-trace --stats -d DIR -- python scratch/profile/profile_surface_guided.py --only 512,8,1     (the per-kernel split)

Shapes 256^2 and 512^2, B = 1 and 8, subsample 1 and 4, 37 x 37 patches, the viewer's defaults, random maps inside the decoder's
ranges; 5 warm-ups, 20 timed runs, median with min and max.  The depth is profile_surface.py's.
  emit      fgs_surface_emit (the parent's kernel, untouched) and fgs_surface_emit_guided on the same count state, timed alternately
            in one process, each launch alone between two events.  Added algorithmic traffic of the guided emit, computed: 4 B
            written per point (point_rows) + 24 B read per patch, against 56 B per row.
  backward  fgs_surface_guided_backward alone between two events.  Algorithmic bytes, computed: 44 B of upstream gradient per row,
            the depth (4 B / pixel), flags (1 B / point) and point_rows (4 B / point) once, g_mods written (24 B / patch).
  --train   one --experiment 3 --decoder guided_saag step (image size 256, batch 8, subsample 4, synthetic data) beside an
            --experiment 1 step on a dummy cloud of the same size per image: for orientation only."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fresnel_amd import surface  # noqa: E402
from profile_surface import synthetic_depth  # noqa: E402

HBM_BYTES_PER_S = 8e12
HP = WP = 37


def random_mods(batch, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(batch, 6, HP, WP, generator=g) * 2.0 - 1.0
    centre = torch.tensor([1.0, 0.0, 1.0, 1.0, 1.0, 1.0]).reshape(1, 6, 1, 1)
    width = torch.tensor([0.5, 0.1, 0.3, 0.3, 0.5, 0.3]).reshape(1, 6, 1, 1)
    return (centre + width * u).to(dev).contiguous()


def timed(fn, warmup, runs):
    out = []
    for i in range(warmup + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3)
    return out


def measure(S, batch, sub, dev, warmup=5, runs=20):
    depth = torch.from_numpy(synthetic_depth(S, batch)).to(dev)
    color = torch.rand(batch, 3, S, S, device=dev)
    params = surface.SurfaceGaussianParams(subsample=sub)
    state = surface.count(depth, color, params)
    plain_out = surface.emit(state)
    total = state.offsets_host[-1]
    mods = random_mods(batch, dev)
    guided_out = {k: torch.empty_like(v) for k, v in plain_out.items()}
    rows = torch.empty(batch, state.points_per_image, dtype=torch.int32, device=dev)
    plain_t, guided_t = [], []
    for i in range(warmup + runs):                      # alternately, so that both see the same clocks and cache state
        p = timed(lambda: surface.emit_raw(state, plain_out, total), 0, 1)
        g = timed(lambda: surface.emit_guided_raw(state, mods, guided_out, rows, total), 0, 1)
        if i >= warmup:
            plain_t += p
            guided_t += g
    grads = dict(g_positions=torch.randn(total, 3, device=dev), g_scales=torch.randn(total, 3, device=dev),
                 g_rotations=torch.randn(total, 4, device=dev), g_opacities=torch.randn(total, device=dev))
    bwd_t = timed(lambda: surface.guided_backward(state, mods, rows, **grads), warmup, runs)
    points = batch * state.points_per_image
    patches = batch * HP * WP
    added = points * 4 + patches * 24
    bwd_bytes = total * 44 + batch * S * S * 4 + points * 5 + patches * 24
    return dict(S=S, B=batch, sub=sub, rows=total, points=points, plain=plain_t, guided=guided_t, bwd=bwd_t, added_share=added / (total * 56),
                bwd_bytes=bwd_bytes)


def fmt(ts):
    return f"{statistics.median(ts):>8.1f} {min(ts):>7.1f} {max(ts):>7.1f}"


def train_steps(dev, lines, steps=10, warmup=3):
    from fresnel_amd import train
    from fresnel_amd.dist import DPContext

    def run(argv, saag_points=None):
        cfg = train.config_from_args(train.arg_parser().parse_args(argv))
        cfg.device = "cuda:0"
        torch.manual_seed(0)
        model = train.make_decoder(cfg).to(dev).train()
        renderer, camera = train.default_renderer_factory(cfg, dev, cfg.image_size)
        opt = train.make_optimizer(model, cfg)
        dp = DPContext(device=dev)
        data = train.SyntheticDataset(8 * (steps + warmup), cfg)
        ts = []
        for i in range(warmup + steps):
            batch = data.batch(list(range(8 * i, 8 * i + 8)), dev)
            if saag_points:
                batch = tuple(batch) + tuple(train.create_dummy_saag(8, saag_points, dev))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            train.train_step(model, renderer, camera, batch, opt, cfg, dp)
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                ts.append(e0.elapsed_time(e1))
        return ts

    from fresnel_amd.surface import SurfaceGaussianParams, surface_gaussians
    cfg = train.config_from_args(train.arg_parser().parse_args(["--experiment", "3", "--decoder", "guided_saag", "--image_size", "256", "--batch_size", "8"]))
    probe = train.SyntheticDataset(8, cfg).batch(list(range(8)), dev)
    counts = [c["positions"].shape[0] for c in surface_gaussians(probe[2], probe[0], SurfaceGaussianParams(subsample=4, normalize_extent=0.0))]
    n = max(counts)
    t3 = run(["--experiment", "3", "--decoder", "guided_saag", "--image_size", "256", "--batch_size", "8", "--surface_subsample", "4"])
    t1 = run(["--experiment", "1", "--image_size", "256", "--batch_size", "8", "--saag_backend", "hip"], saag_points=n)
    lines.append("")
    lines.append(f"training step, image size 256, batch 8, synthetic data, {steps} steps after {warmup} warm-ups, ms (median min max); orientation only")
    lines.append(f"  --experiment 3 --decoder guided_saag --surface_subsample 4 (clouds of {min(counts)} ... {n} rows, padded to {n}): "
                 f"{statistics.median(t3):.2f} {min(t3):.2f} {max(t3):.2f}")
    lines.append(f"  --experiment 1 --saag_backend hip on a dummy cloud of {n} Gaussians per image:                       "
                 f"{statistics.median(t1):.2f} {min(t1):.2f} {max(t1):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="S,B,subsample: that shape alone (for a kernel trace)")
    ap.add_argument("--train", action="store_true", help="also time the experiment-3 and experiment-1 training steps")
    ap.add_argument("--commit", default="?", help="the commit the measured tree sits on (goes into the header line)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"surface_guided: hipEvent times in us (median min max) of single launches, 20 runs after 5 warm-ups, {torch.cuda.get_device_name(0)}; "
             f"measured on the tree on top of commit {args.commit}",
             "37 x 37 patches, viewer defaults, colour image present, random maps inside the decoder's ranges",
             "emit: fgs_surface_emit (the parent's kernel) and fgs_surface_emit_guided alternately on one count state; 'added' = computed extra "
             "traffic of the guided emit (4 B / point + 24 B / patch) over 56 B / row",
             "backward: fgs_surface_guided_backward; 'of 8 TB/s' = computed bytes (44 B / row + depth + flags + point_rows + g_mods) / 8 TB/s / median",
             f"{'shape':>8} {'B':>2} {'sub':>3} {'rows':>9} | {'plain emit':>24} | {'guided emit':>24} | {'ratio':>6} {'added':>6} | "
             f"{'backward':>24} {'MB':>7} {'of 8 TB/s':>9}"]
    if args.only:
        shapes = [tuple(int(v) for v in args.only.split(","))]
    else:
        shapes = [(S, b, sub) for S in (256, 512) for b in (1, 8) for sub in (1, 4)]
    for S, batch, sub in shapes:
        r = measure(S, batch, sub, dev)
        mp, mg, mb = statistics.median(r["plain"]), statistics.median(r["guided"]), statistics.median(r["bwd"])
        lines.append(f"{S:>5}^2 {batch:>3} {sub:>3} {r['rows']:>9} | {fmt(r['plain'])} | {fmt(r['guided'])} | {mg / mp:>6.3f} {r['added_share']:>6.2%} | "
                     f"{fmt(r['bwd'])} {r['bwd_bytes'] / 1e6:>7.2f} {r['bwd_bytes'] / HBM_BYTES_PER_S * 1e6 / mb:>9.1%}")
    if args.train:
        train_steps(dev, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
