"""Workspace sizes and step times with a duplicate-capacity hint (FgsDims.dup_capacity; DESIGN.md "Capacity and overflow").

    python scratch/profile/workspace_capacity.py memory            # host arithmetic: fgs_workspace_bytes, no GPU
    python scratch/profile/workspace_capacity.py gpu [--steps 200]  # MI355X: step time hinted vs worst, peak memory

`memory` prints, for the five scenes of the bench records (duplicate counts D = tile_duplicates_rank0 of BENCH_r05.json and
profiles/r05_bench_*.json), saved + scratch at the worst case and at the capacity CapacityTracker reaches for D.
`gpu` runs forward + backward through TileBasedRenderer at config 2, 3 and 4 shapes (bench.py's scenes): legs of --steps steps
between device events, worst / adaptive / worst again in ONE process after warm-up (the two worst legs give the spread), and
torch.cuda.max_memory_allocated over 20 adaptive steps after the first, next to the worst-case figure.
Every line says whether it is computed or measured."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SCENES = [  # name, make_dims arguments, recorded duplicates
    ("config 2 (16 x 8192 @ 256^2)", dict(batch=16, num_gaussians=8192, width=256, height=256), 1_234_017),
    ("config 3 (8 x 32768 @ 512^2)", dict(batch=8, num_gaussians=32768, width=512, height=512), 4_099_112),
    ("config 3 decoder-like (8 x 32761)", dict(batch=8, num_gaussians=32761, width=512, height=512), 10_309_213),
    ("config 3, 64 images", dict(batch=64, num_gaussians=32768, width=512, height=512), 32_809_440),
    ("config 4 (phase, 16 x 8192 @ 256^2)", dict(batch=16, num_gaussians=8192, width=256, height=256, use_phase=True,
                                               tuning=dict(sort_mode=1)), 548_498),
]


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "?"
    except OSError:
        return "?"


def memory():
    from fresnel_amd import _binding as B
    from fresnel_amd.renderer import CapacityTracker
    print(f"# COMPUTED (fgs_workspace_bytes, {B.version()}); margin {CapacityTracker.margin}, window {CapacityTracker.window}")
    print(f"{'scene':38s} {'D':>11s} {'worst cap':>11s} {'saved+scratch GB':>17s} {'capacity':>11s} {'saved+scratch GB':>17s} {'ratio':>6s}")
    for name, kw, D in SCENES:
        d0 = B.make_dims(**kw)
        worst = int(B.saved_layout(d0).dup_capacity)
        s0, c0 = B.workspace_bytes(d0)
        t = CapacityTracker(worst)
        t.observe(D)
        cap = t.capacity()
        s1, c1 = B.workspace_bytes(B.make_dims(dup_capacity=cap, **kw))
        print(f"{name:38s} {D:11d} {worst:11d} {s0 / 1e9:8.3f}+{c0 / 1e9:<8.3f} {cap or worst:11d} {s1 / 1e9:8.3f}+{c1 / 1e9:<8.3f} "
              f"{(s1 + c1) / (s0 + c0):6.3f}")


def gpu(steps):
    import torch
    import bench
    from fresnel_amd import renderer as R
    if not torch.cuda.is_available():
        raise SystemExit("the gpu mode needs an MI355X: no fallback")
    dev = torch.device("cuda:0")
    print(f"# MEASURED on {torch.cuda.get_device_name(0)}; legs of {steps} steps between device events, one process")
    for wl in ("config2", "config3", "config4"):
        N, S, Bn = bench.WORKLOADS[wl]
        cfg_id = int(wl[-1])
        pos, scale, quat, col, opa = bench.synth_batch(Bn, N, 1000 * cfg_id, dev)
        phases = None
        if wl == "config4":
            g = torch.Generator().manual_seed(977)
            zone = torch.randint(0, 8, (Bn, N), generator=g).float().to(dev)
            pos[..., 2] = -2.0 - 2.0 * (zone + 0.5) / 8.0
            scale = scale * (0.5 + 0.5 * torch.rand(Bn, N, 1, generator=g).to(dev))
            phases = torch.rand(Bn, N, generator=g).to(dev).requires_grad_(True)
        leaves = [t.requires_grad_(True) for t in (pos, scale, quat, col, opa)] + ([phases] if phases is not None else [])
        g = torch.Generator().manual_seed(4242)
        gI = torch.randn(Bn, 3, S, S, generator=g).to(dev)
        gD = (torch.randn(Bn, S, S, generator=g) * 0.1).to(dev)
        cam = R.Camera(0.8 * S, 0.8 * S, S / 2, S / 2, S, S)
        rens = {}
        for mode in ("worst", "adaptive"):
            rens[mode] = R.TileBasedRenderer(S, S, use_phase_blending=wl == "config4", phase_amplitude=0.25, workspace=mode).to(dev)
            if wl == "config4":
                rens[mode].tuning = dict(sort_mode=1)

        def step(ren):
            for t in leaves:
                t.grad = None
            img, dep = ren(*leaves[:5], cam, return_depth=True, phases=phases)
            torch.autograd.backward([img, dep], [gI, gD])
            return img

        def leg(ren):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                step(ren)
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / steps

        peak = {}
        for mode in ("worst", "adaptive"):  # warm-up, and the peak-memory figure of each mode
            R.release_scratch()
            torch.cuda.empty_cache()
            first = step(rens[mode])
            torch.cuda.synchronize()
            del first
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            for _ in range(20):
                step(rens[mode])
            torch.cuda.synchronize()
            peak[mode] = (torch.cuda.max_memory_allocated(), base)
        st = next(iter(rens["adaptive"].workspace_stats().values()))
        legs = [("worst", leg(rens["worst"])), ("adaptive", leg(rens["adaptive"])), ("worst", leg(rens["worst"])),
                ("adaptive", leg(rens["adaptive"]))]
        img_w, img_a = step(rens["worst"]).detach().clone(), step(rens["adaptive"]).detach().clone()
        torch.cuda.synchronize()
        same = torch.equal(img_w, img_a)
        st = next(iter(rens["adaptive"].workspace_stats().values()))
        print(f"{wl}: demand {st['last_demand']}, capacity {st['capacity']}, overflows {st['overflows']}, images bitwise equal: {same}")
        print("  step ms: " + ", ".join(f"{m} {v:.4f}" for m, v in legs))
        print(f"  peak allocated over 20 steps after the first: worst {peak['worst'][0] / 1e9:.3f} GB, adaptive {peak['adaptive'][0] / 1e9:.3f} GB"
              f"  (resident before the steps: {peak['worst'][1] / 1e9:.3f} / {peak['adaptive'][1] / 1e9:.3f} GB)")
        R.release_scratch()
        del rens, leaves, gI, gD
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["memory", "gpu"])
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    print(f"# workspace_capacity.py {a.mode}, commit {commit()} (+ working tree)")
    memory() if a.mode == "memory" else gpu(a.steps)
