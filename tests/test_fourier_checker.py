"""CPU tests of the Fourier renderer's test infrastructure and argument validation:
  * tests/fourier_checker.py (the dense torch restatement) against every fixture the reference's own class produced;
  * the 24 seeded random scenes of tests/test_hip_fourier.py stay within the cap of skipped seeds (arg-max gap < 1e-3);
  * fgs_fourier_* refuse bad dims and null pointers without touching a GPU; the module refuses CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch

import fourier_cases as FC
from helpers import rel_to_max

TOL = 1e-4


@pytest.mark.parametrize("name", FC.FIXTURES)
def test_checker_matches_reference_fixture(name):
    s = FC.fixture_scene(name)
    g = s["g"]
    img, raw, grads = FC.checker_run("fixture", name, False)
    assert rel_to_max(img, g["image"]) <= TOL
    for k, got in zip(FC.GRADS, grads):
        want = g["grad_" + k]
        err = rel_to_max(got, want)
        print(f"{name} grad_{k}: {err:.2e}")
        assert err <= TOL, (name, k, err)
    if name in FC.GAPPED:
        assert float(g["argmax_gap"]) >= FC.MIN_GAP
        assert FC.fc.argmax_gap(torch.from_numpy(raw)) >= FC.MIN_GAP
    if "behind" in name:
        assert all(not np.any(g["grad_" + k]) for k in FC.GRADS)
        assert np.array_equal(g["image"], np.broadcast_to(g["background"].reshape(3, 1, 1), g["image"].shape))
    if "dim" in name:
        assert 0 < raw.max() <= 1e-8  # nothing is normalised
        assert any(np.any(g["grad_" + k]) for k in FC.GRADS)


def test_checker_fp64_agrees_with_fp32():
    a, b = FC.checker_run("fixture", FC.FIXTURES[3], False), FC.checker_run("fixture", FC.FIXTURES[3], True)
    assert rel_to_max(a[0], b[0]) <= 1e-5
    for x, y in zip(a[2], b[2]):
        assert rel_to_max(x, y) <= 1e-4


def test_random_seeds_stay_within_the_skip_cap():
    skipped = [s for s in FC.RANDOM_SEEDS if FC.random_gap(s) < FC.MIN_GAP]
    print("skipped seeds:", skipped)
    assert len(FC.RANDOM_SEEDS) == 24 and len(skipped) <= FC.MAX_SKIPPED


def _dims(B=1, N=8, W=16, H=16, cams=1, bg=(0.0, 0.0, 0.0)):
    from fresnel_amd import _binding as Bd
    d = Bd.FgsFourierDims()
    d.batch, d.num_gaussians, d.width, d.height, d.num_cameras = B, N, W, H, cams
    for i in range(3):
        d.background[i] = bg[i]
    return d


@pytest.mark.parametrize("kw", [dict(B=0), dict(N=0), dict(W=0), dict(H=-3), dict(B=2, cams=3), dict(B=3, cams=2), dict(cams=0),
                                dict(W=20000), dict(B=70000), dict(bg=(float("nan"), 0.0, 0.0))])
def test_fourier_entries_refuse_bad_dims(kw):
    from fresnel_amd import _binding as Bd
    lib = Bd.load()
    d = _dims(**kw)
    s, c = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert lib.fgs_fourier_workspace_bytes(ctypes.byref(d), ctypes.byref(s), ctypes.byref(c)) == -1
    assert (s.value, c.value) == (7, 7)
    one = ctypes.c_void_p(256)  # never dereferenced: the dims are refused first
    assert lib.fgs_fourier_forward(ctypes.byref(d), *([one] * 9), None) == -1
    assert lib.fgs_fourier_backward(ctypes.byref(d), *([one] * 14), None) == -1
    assert lib.fgs_last_error()


def test_fourier_entries_refuse_null_pointers_and_size_their_buffers():
    from fresnel_amd import _binding as Bd
    lib = Bd.load()
    assert lib.fgs_fourier_workspace_bytes(None, None, None) == -1
    d = _dims(B=2, N=65, W=56, H=40, cams=2)
    s, c = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.fgs_fourier_workspace_bytes(ctypes.byref(d), ctypes.byref(s), ctypes.byref(c)) == 0
    # saved: records, the raw image, the per-image maximum; scratch: at least the gradient image and the per-Gaussian sums
    assert s.value >= 2 * 65 * 8 * 4 + 2 * 3 * 56 * 40 * 4 + 2 * 8 and s.value % 256 == 0
    assert c.value >= 2 * 3 * 56 * 40 * 4 + 2 * 65 * 12 * 4 and c.value % 256 == 0
    one = ctypes.c_void_p(256)
    for k in range(9):
        args = [one] * 9
        args[k] = None
        assert lib.fgs_fourier_forward(ctypes.byref(d), *args, None) == -1, k
    for k in range(14):
        args = [one] * 14
        args[k] = None
        assert lib.fgs_fourier_backward(ctypes.byref(d), *args, None) == -1, k
    assert lib.fgs_fourier_forward(None, *([one] * 9), None) == -1


def test_module_surface_and_cpu_refusal():
    from fresnel_amd._binding import FgsError
    from fresnel_amd.renderer import Camera, FourierGaussianRenderer
    ren = FourierGaussianRenderer(64, 48)
    assert (ren.width, ren.height, ren.focal_depth, ren.learnable_wavelengths) == (64, 48, 0.5, True)
    assert isinstance(ren.wavelengths, torch.nn.Parameter)
    assert torch.allclose(ren.wavelengths.detach(), torch.tensor([0.0635, 0.05, 0.041]))
    assert torch.equal(ren.background, torch.zeros(3))
    fixed = FourierGaussianRenderer(64, 48, (0.1, 0.2, 0.3), 0.65, 0.55, 0.45, False, 0.7)
    assert not isinstance(fixed.wavelengths, torch.nn.Parameter) and "wavelengths" in dict(fixed.named_buffers())
    assert fixed.focal_depth == 0.7 and list(fixed.parameters()) == []
    assert torch.allclose(fixed._get_constrained_wavelengths(), torch.tensor([0.5, 0.5, 0.45]))
    assert "learnable=False" in fixed.extra_repr() and "size=(48, 64)" in repr(fixed)
    s = FC.small_scene(31, 33, 17)
    ts = [torch.from_numpy(a) for a in s["arrs"]]
    with pytest.raises(FgsError):
        FourierGaussianRenderer(33, 17)(*ts, Camera(26.4, 26.4, 16.5, 8.5, 33, 17))
