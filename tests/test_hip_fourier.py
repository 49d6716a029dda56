"""GPU tests of the Fourier renderer (fgs_fourier_*, fresnel_amd.renderer.FourierGaussianRenderer) against fixtures the
reference's FourierGaussianRenderer produced (tests/golden/F*_fourier_*.npz) and against the dense torch checker
(tests/fourier_checker.py).  The project's standing rule: image and all five gradients within 1e-4 of the tensor's maximum.
The shapes are the smallest at which the kernels can still go wrong: frames that are no multiple of the 32 x 32 matrix-core
tile or of the 64 x 64 block tile, more than one block, N below / at / above the 32-Gaussian K-chunk."""
import numpy as np
import pytest
import torch

import fourier_cases as FC
from helpers import rel_to_max, synth_aniso, upstream_grads

gpu = pytest.mark.gpu
TOL = 1e-4


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _camera(view, intr, W, H):
    from fresnel_amd.renderer import Camera
    fx, fy, cx, cy, near, far = [float(v) for v in intr]
    cam = Camera(fx, fy, cx, cy, W, H, near, far)
    cam.set_view(torch.from_numpy(np.asarray(view, np.float32)))
    return cam


def _render(arrs, cams, W, H, bg, gI, ren=None, **fw):
    """-> image, [five gradients] as numpy (arrs: (N,.) per image or (B,N,.) batched; cams: one Camera or a list)."""
    from fresnel_amd.renderer import FourierGaussianRenderer
    dev = _dev()
    ren = ren if ren is not None else FourierGaussianRenderer(W, H, background=tuple(bg)).to(dev)
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True) for a in arrs]
    img = ren(*ts, cams, **fw)
    (img * torch.from_numpy(np.ascontiguousarray(gI)).to(dev)).sum().backward()
    assert ren.wavelengths.grad is None
    return img.detach().cpu().numpy(), [t.grad.cpu().numpy() for t in ts]


def _compare(what, img, grads, ref32, ref64=None, opacity_scale=None):
    """1e-4 of max against the reference's fp32 run or, where given, its fp64 run.  `opacity_scale`: the scale the opacity
    gradient is measured against instead of its own maximum (the single-Gaussian case, see there)."""
    assert np.isfinite(img).all() and all(np.isfinite(g).all() for g in grads), what
    for k, got, i in zip(["image"] + FC.GRADS, [img] + grads, range(6)):
        want = ref32[0] if i == 0 else ref32[1][i - 1]
        if k == "opacities" and opacity_scale is not None:
            err = float(np.abs(got - want).max() / opacity_scale)
        else:
            err = rel_to_max(got, want)
        if ref64 is not None:
            err = min(err, rel_to_max(got, ref64[0] if i == 0 else ref64[1][i - 1]))
        print(f"{what} {k}: {err:.2e}")
        assert err <= TOL, f"{what} {k}: {err:.2e} > {TOL:.0e}"


@gpu
@pytest.mark.parametrize("name", FC.FIXTURES)
def test_fixture_parity(name):
    """Image and the five gradients within 1e-4 of max of the reference's own run; return_depth gives zeros; phases are
    ignored; the wavelengths get no gradient."""
    from fresnel_amd.renderer import FourierGaussianRenderer
    s = FC.fixture_scene(name)
    g, W, H = s["g"], s["W"], s["H"]
    cam = _camera(s["view"], s["intr"], W, H)
    img, grads = _render(s["arrs"], cam, W, H, s["bg"], s["gI"])
    _compare(name, img, grads, (g["image"], [g["grad_" + k] for k in FC.GRADS]))
    if "behind" in name:
        assert all(not np.any(x) for x in grads)
    dev = _dev()
    ren = FourierGaussianRenderer(W, H, tuple(s["bg"]), 0.65, 0.55, 0.45, True).to(dev)
    ts = [torch.from_numpy(a).to(dev) for a in s["arrs"]]
    ph = torch.rand(ts[0].shape[0], device=dev) * 6.28
    img2, dep = ren(positions=ts[0], scales=ts[1], rotations=ts[2], colors=ts[3], opacities=ts[4], camera=cam,
                    return_depth=True, phases=ph)
    assert dep.shape == (H, W) and not bool(dep.any()) and not dep.requires_grad
    assert np.array_equal(img2.cpu().numpy(), img)


@gpu
@pytest.mark.parametrize("cameras", [1, 3])
def test_batch_with_a_culled_image_equals_single_images(cameras):
    """Three 56 x 40 images, the middle one entirely culled (its maximum is 0: not normalised, zero gradients), with one
    camera and with three: every image and gradient is bit-equal to the same image rendered alone."""
    W, H, N, bg = 56, 40, 64, (0.1, 0.2, 0.3)
    scenes = [list(synth_aniso(N, 7700 + b)) for b in range(3)]
    scenes[1][0] = scenes[1][0].copy()
    scenes[1][0][:, 2] = np.abs(scenes[1][0][:, 2]) + 3.0  # behind every camera below
    views = [np.eye(4, dtype=np.float32) for _ in range(3)]
    if cameras == 3:
        views[1][:3, 3] = (0.1, -0.05, 0.3)
        views[2][:3, 3] = (-0.2, 0.1, -0.4)
    cams = [_camera(v, FC.intrinsics(W, H), W, H) for v in views]
    gI = np.stack([upstream_grads(7800 + b, H, W)[0] for b in range(3)])
    batch = [np.stack([s[i] for s in scenes]) for i in range(5)]
    img, grads = _render(batch, cams if cameras == 3 else cams[0], W, H, bg, gI)
    assert img.shape == (3, 3, H, W)
    for b in range(3):
        one_img, one_grads = _render(scenes[b], cams[b], W, H, bg, gI[b])
        assert np.array_equal(img[b], one_img), b
        for k, gb, g1 in zip(FC.GRADS, grads, one_grads):
            assert np.array_equal(gb[b], g1), (b, k)
    assert np.array_equal(img[1], np.broadcast_to(np.array(bg, np.float32).reshape(3, 1, 1), (3, H, W)))
    assert all(not np.any(g[1]) for g in grads) and all(np.any(g[0]) and np.any(g[2]) for g in grads)


@gpu
@pytest.mark.parametrize("N,W,H", FC.SMALL_CASES)
def test_chunk_boundaries_and_partial_tiles(N, W, H):
    """N below, just under and just over the 32-Gaussian K-chunk, frames that are no multiple of a tile, against the fp64
    checker at 1e-4 of max.  A SINGLE Gaussian's image is normalised by its own peak, so the opacity cancels out of it and
    dL/dopacity = sum_c dL/dw_c colour_c is analytically zero: the checker's fp64 value is rounding noise (1e-17) and "of the
    tensor's max" is no scale.  There the same 1e-4 is taken of the size of the terms that cancel,
    sum_c |dL/dw_c colour_c| = sum_c |dL/dcolour_c colour_c| / opacity (from the fp64 run), as for any other sum."""
    s = FC.small_scene(N, W, H)
    img, grads = _render(s["arrs"], _camera(s["view"], s["intr"], W, H), W, H, s["bg"], s["gI"])
    r64 = FC.checker_run("small", (N, W, H), True)
    scale = None
    if N == 1:
        scale = float(np.abs(r64[2][3][0] * s["arrs"][3][0]).sum() / abs(s["arrs"][4][0]))
        assert scale > 0
    _compare(f"N={N} {W}x{H}", img, grads, (r64[0], r64[2]), opacity_scale=scale)


@gpu
def test_backward_is_reproducible_and_saved_is_const():
    """Two backward calls on one `saved` buffer (a retained graph) and two full runs give bitwise-equal gradients."""
    from fresnel_amd.renderer import FourierGaussianRenderer
    s = FC.fixture_scene("F4_fourier_n64_56x40")
    dev, W, H = _dev(), s["W"], s["H"]
    cam = _camera(s["view"], s["intr"], W, H)
    ren = FourierGaussianRenderer(W, H, background=tuple(s["bg"])).to(dev)
    ts = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in s["arrs"]]
    gI = torch.from_numpy(s["gI"]).to(dev)
    loss = (ren(*ts, cam) * gI).sum()
    first = torch.autograd.grad(loss, ts, retain_graph=True)
    torch.empty(1 << 22, device=dev).fill_(float("nan"))  # the allocator hands the second backward other scratch content
    second = torch.autograd.grad(loss, ts)
    for k, a, b in zip(FC.GRADS, first, second):
        assert torch.equal(a, b), k
    _, again = _render(s["arrs"], cam, W, H, s["bg"], s["gI"])
    for k, a, b in zip(FC.GRADS, first, again):
        assert np.array_equal(a.cpu().numpy(), b), k


@gpu
@pytest.mark.parametrize("seed", FC.RANDOM_SEEDS)
def test_random_scene_against_checker(seed):
    """24 seeded anisotropic scenes, N <= 128, frames <= 64 x 64, random orbit views: 1e-4 against the checker's fp32 or fp64
    run.  A seed whose arg-max gap is under 1e-3 is skipped (the gradient through the maximum would pin noise); at most 2 of
    the 24 may be: tests/test_fourier_checker.py checks that on the CPU (none is, as the scenes stand)."""
    if FC.random_gap(seed) < FC.MIN_GAP:
        pytest.skip("arg-max gap below 1e-3")
    s = FC.random_scene(seed)
    img, grads = _render(s["arrs"], _camera(s["view"], s["intr"], s["W"], s["H"]), s["W"], s["H"], s["bg"], s["gI"])
    r32, r64 = FC.checker_run("random", seed, False), FC.checker_run("random", seed, True)
    _compare(f"seed {seed}", img, grads, (r32[0], r32[2]), (r64[0], r64[2]))
