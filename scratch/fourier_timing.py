"""Timing record of the Fourier renderer (a record, not a gate): forward + backward of fresnel_amd's FourierGaussianRenderer
against the dense torch restatement (tests/fourier_checker.py -- what a user of the library had before the HIP class existed)
on the same GPU in the same process, and the share of the fp32 matrix peak the two product kernels reach.

    python scratch/fourier_timing.py [--out profiles/fourier_renderer.txt] [--steps 20] [--warmup 5]

Step times: device events around forward + backward, median over the steps after the warm-up.  Kernel times of the two product
kernels: the library's per-stage event pairs (splat_fwd = k_fourier_fwd, splat_bwd = k_fourier_bwd), in a pass of their own.
Needs a GPU; there is no fallback."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fourier_checker as fc  # noqa: E402
from fresnel_amd import _binding as B  # noqa: E402
from fresnel_amd.renderer import Camera, FourierGaussianRenderer  # noqa: E402
from helpers import synth_aniso  # noqa: E402

PEAK_TF = 157.3  # fp32-input MFMA, MI355X


def scene(N, Bn, dev):
    per = [synth_aniso(N, 4000 + b, opacity_max=1.0) for b in range(Bn)]
    return [torch.from_numpy(np.stack([p[i] for p in per])).to(dev) for i in range(5)]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fourier_renderer.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="377x256x16,8192x256x16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fourier_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    lines = [f"Fourier renderer, forward + backward, {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"median (min ... max) of {a.steps} steps after {a.warmup} warm-up steps, device events; warm clocks, windows of well "
             "under a second per figure: not thermally sustained",
             "baseline = tests/fourier_checker.py (dense torch, one image per call like the reference) on the same GPU, same process", ""]
    for shp in a.shapes.split(","):
        N, R, Bn = [int(v) for v in shp.split("x")]
        ts = [t.requires_grad_(True) for t in scene(N, Bn, dev)]
        gI = torch.randn(Bn, 3, R, R, device=dev, generator=torch.Generator(dev).manual_seed(1))
        cam = Camera(0.8 * R, 0.8 * R, R / 2, R / 2, R, R)
        intr = (cam.fx, cam.fy, cam.cx, cam.cy, cam.near, cam.far)
        view = cam.view_matrix.numpy()
        ren = FourierGaussianRenderer(R, R).to(dev)

        def hip():
            for t in ts:
                t.grad = None
            (ren(*ts, cam) * gI).sum().backward()

        def dense():
            for t in ts:
                t.grad = None
            for b in range(Bn):
                (fc.render(*[t[b] for t in ts], view, intr, R, R)[0] * gI[b]).sum().backward()

        hip()
        g_hip = [t.grad.clone() for t in ts]
        img_hip = ren(*ts, cam).detach()
        dense()
        img_dense = torch.stack([fc.render(*[t[b].detach() for t in ts], view, intr, R, R)[0] for b in range(Bn)])
        errs = [float((img_hip - img_dense).abs().max() / img_dense.abs().max())]
        errs += [float((x - t.grad).abs().max() / t.grad.abs().max()) for x, t in zip(g_hip, ts)]
        t_hip = timed(hip, a.steps, a.warmup)
        t_dense = timed(dense, a.steps, max(1, a.warmup // 2))
        B.stage_timing_enable(True, stages=["splat_fwd", "splat_bwd"])
        for _ in range(a.steps):
            hip()
        st = B.stage_timing_read()
        B.stage_timing_enable(False)
        k_fwd, k_bwd = st["splat_fwd"][0] / st["splat_fwd"][1], st["splat_bwd"][0] / st["splat_bwd"][1]
        fl_fwd, fl_bwd = 2.0 * 3 * N * R * R * Bn, 2.0 * 9 * N * R * R * Bn
        lines += [f"{N} Gaussians, {R} x {R}, {Bn} images",
                  f"  HIP class            {t_hip[0]:9.3f} ms ({t_hip[1]:.3f} ... {t_hip[2]:.3f})",
                  f"  dense torch checker  {t_dense[0]:9.3f} ms ({t_dense[1]:.3f} ... {t_dense[2]:.3f})   ratio {t_dense[0] / t_hip[0]:.1f}x",
                  f"  k_fourier_fwd  {k_fwd:8.4f} ms  {fl_fwd / k_fwd / 1e9:7.2f} TF = {fl_fwd / k_fwd / 1e9 / PEAK_TF * 100:5.1f} % of the {PEAK_TF} TF fp32 matrix peak "
                  f"(2 x 3 N H W B = {fl_fwd:.3g} flop, compute-bound)",
                  f"  k_fourier_bwd  {k_bwd:8.4f} ms  {fl_bwd / k_bwd / 1e9:7.2f} TF = {fl_bwd / k_bwd / 1e9 / PEAK_TF * 100:5.1f} % "
                  f"(2 x 9 N H W B = {fl_bwd:.3g} flop, compute-bound)",
                  "  HIP vs dense, max |diff| / max: image %.1e, gradients %s" % (errs[0], " ".join(f"{e:.1e}" for e in errs[1:])), ""]
        print("\n".join(lines[-7:]), flush=True)
        del ts, gI
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
