"""Fixtures of the Fourier renderer: the reference's FourierGaussianRenderer (scripts/models/differentiable_renderer.py,
DR:1500-1774) run on the CPU, its image and the five input gradients stored as .npz in the G-series format (inputs, camera,
background, seed of the upstream gradient gI, image, gradients, generating-stack metadata).  Runs only where the reference is
present; the fixtures hold data only.

  F1 SAAG N=256 @128x128, background 0
  F2 anisotropic N=300 @96x96, opacities up to 1.3 (the final clamp is active), background (.1,.2,.3)
  F3 N=377 @64x64 (the Fibonacci count), constructed with the training script's wavelengths (TGD:1886-1888)
  F4 N=64 on a 56x40 frame (non-square, no multiple of a matrix-core tile)
  F5 every Gaussian behind the camera
  F6 "dim": opacities ~1e-10, so the maximum stays <= 1e-8 and nothing is normalised

The gradient through the image maximum lands on one element; a scene whose two brightest elements are closer than rounding
would pin noise, so F1-F4 take the first seed whose relative gap is >= 1e-3 (F5, F6: no gradient flows through the maximum).
"""
import os
import sys

REF = "/root/reference/scripts"
if not os.path.isdir(REF):
    sys.exit("make_goldens_fourier.py: the reference is absent; fixtures can only be generated where it is present")
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from models.differentiable_renderer import Camera, FourierGaussianRenderer  # noqa: E402  (the reference, read-only)
import helpers  # noqa: E402

torch.set_num_threads(8)
META = dict(torch=torch.__version__, numpy=np.__version__, device="cpu")
MIN_GAP = 1e-3


def run(arrs, W, H, bg, seed_up, ctor):
    cam = Camera(fx=0.8 * W, fy=0.8 * W, cx=W / 2, cy=H / 2, width=W, height=H)
    ren = FourierGaussianRenderer(W, H, background=bg, **ctor)
    leaves = [torch.from_numpy(a).clone().requires_grad_(True) for a in arrs]
    img = ren(*leaves, cam)
    gI = helpers.upstream_grads(seed_up, H, W)[0]
    (img * torch.from_numpy(gI)).sum().backward()
    assert ren.wavelengths.grad is None
    rec = dict(positions=arrs[0], scales=arrs[1], rotations=arrs[2], colors=arrs[3], opacities=arrs[4],
               view=cam.view_matrix.numpy().astype(np.float32),
               intr=np.array([cam.fx, cam.fy, cam.cx, cam.cy, cam.near, cam.far], dtype=np.float64),
               size=np.array([W, H], dtype=np.int32), background=np.array(bg, dtype=np.float32),
               seed_up=np.int32(seed_up), upstream_shape=np.array([H, W], np.int32), upstream_has_gD=np.uint8(0),
               image=img.detach().numpy())
    for n, t in zip(["positions", "scales", "rotations", "colors", "opacities"], leaves):
        rec["grad_" + n] = (t.grad if t.grad is not None else torch.zeros_like(t)).numpy()
    for k, v in META.items():
        rec["meta_" + k] = np.array(v)
    return rec


def raw_gap(arrs, W, H):
    """Gap of the two largest elements of the un-normalised image (tests/fourier_checker.py restates the accumulation)."""
    import fourier_checker as fc
    cam = Camera(fx=0.8 * W, fy=0.8 * W, cx=W / 2, cy=H / 2, width=W, height=H)
    with torch.no_grad():
        _, raw = fc.render(*[torch.from_numpy(a) for a in arrs], cam.view_matrix.numpy(),
                           (cam.fx, cam.fy, cam.cx, cam.cy, cam.near, cam.far), W, H)
    return fc.argmax_gap(raw)


def main():
    cases = [
        ("F1_fourier_saag256_128", lambda s: helpers.synth_saag(256, s), 128, 128, (0.0, 0.0, 0.0), {}),
        ("F2_fourier_aniso300_96", lambda s: helpers.synth_aniso(300, s, opacity_max=1.3), 96, 96, (0.1, 0.2, 0.3), {}),
        ("F3_fourier_fib377_64", lambda s: helpers.synth_aniso(377, s), 64, 64, (0.0, 0.0, 0.0),
         dict(wavelength_r=0.65, wavelength_g=0.55, wavelength_b=0.45, learnable_wavelengths=True)),
        ("F4_fourier_n64_56x40", lambda s: helpers.synth_aniso(64, s), 56, 40, (0.1, 0.2, 0.3), {}),
    ]
    for k, (name, make, W, H, bg, ctor) in enumerate(cases):
        seed = 200 + 10 * k
        while True:
            arrs = make(seed)
            gap = raw_gap(arrs, W, H)
            if gap >= MIN_GAP:
                break
            seed += 1
        rec = run(arrs, W, H, bg, 300 + k, ctor)
        rec["seed"] = np.int32(seed)
        rec["argmax_gap"] = np.float64(gap)
        save(rec, name)
    arrs = list(helpers.synth_aniso(64, 240))
    arrs[0] = arrs[0].copy()
    arrs[0][:, 2] = np.abs(arrs[0][:, 2]) + 0.5  # z > 0: behind the camera, which looks down -z
    save(run(tuple(arrs), 64, 64, (0.1, 0.2, 0.3), 304, {}), "F5_fourier_behind64_64")
    arrs = list(helpers.synth_aniso(128, 250))
    arrs[4] = (arrs[4] * 1e-10).astype(np.float32)
    rec = run(tuple(arrs), 64, 64, (0.1, 0.2, 0.3), 305, {})
    save(rec, "F6_fourier_dim128_64")


def save(rec, name):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **rec)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KB" + (f", gap {float(rec['argmax_gap']):.2e}" if "argmax_gap" in rec else ""))


if __name__ == "__main__":
    main()
