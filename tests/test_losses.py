"""spectral / stencil losses.

CPU: the torch formulation (oracle/torch_losses.py, the checker) against the reference fixtures G11, and the checker's
FrequencyDomainLoss against closed forms for single-bin images on, just inside and just outside the cutoff circle.
GPU: the product (fresnel_amd/losses.py -> fgs_spectral_loss_* / fgs_helmholtz_loss_* in libfgs_hip.so) against the
same fixtures (loss and every gradient <= 1e-4), and against the checker (float64, with the referee rule of
helpers.assert_with_referee) on a matrix of shapes that runs every instance of fgs_fft2_exec's own column pass
(k_colfft_plain, forward in the losses' forward and inverse in their backward) and the grid-stride loops of the reductions
past their first pass; the mask-boundary known answers; edge values (the 1e-8 clamp, depth at the focal plane, an all-zero
spectrum, rendered == target, phases of hundreds of radians); the training call pattern (no gradient for target / depth);
bitwise repeatability at 8 x 3 x 512^2; and wave_equation_loss on training-size and degenerate periodic grids."""
import numpy as np
import pytest
import torch

from helpers import assert_with_referee, load_golden, rel_to_max

TOL = 1e-4


def _cases(mod, dev):
    P, Fq, helm = mod.PhaseRetrievalLoss, mod.FrequencyDomainLoss, mod.wave_equation_loss
    return {
        "phase": (lambda r, t, d: P(wavelength=0.05, focal_depth=0.5)(r, t, d), ("rendered", "target", "depth")),
        "phase_wl": (lambda r, t, d: P()(r, t, d.unsqueeze(1), wavelength=torch.tensor(0.0635, device=dev)),
                     ("rendered", "target", "depth")),
        "freq": (lambda r, t: Fq(cutoff=0.1, high_weight=2.0)(r, t), ("rendered", "target")),
        "freq_c25": (lambda r, t: Fq(cutoff=0.25, high_weight=0.5)(r, t), ("rendered", "target")),
        "helm": (lambda u: helm(u, 0.05), ("rendered",)),
        "helm3": (lambda u: helm(u, 0.0635, pixel_spacing=1.0 / 128.0), ("depth",)),
    }


def _run(mod, dev):
    g = load_golden("G11_losses_48x40")
    for tag, (fn, names) in _cases(mod, dev).items():
        ts = [torch.tensor(g[n], device=dev, requires_grad=True) for n in names]
        loss = fn(*ts)
        loss.backward()
        ref = float(g[tag + "_loss"])
        assert abs(loss.item() - ref) <= TOL * abs(ref), (tag, loss.item(), ref)
        for i, t in enumerate(ts):
            assert rel_to_max(t.grad.cpu().numpy(), g[f"{tag}_grad{i}"]) <= TOL, (tag, i)


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires an MI355X (torch.cuda unavailable)")
    return torch.device("cuda:0")


def test_checker_matches_reference_fixtures_cpu():
    from oracle import torch_losses
    _run(torch_losses, torch.device("cpu"))


def test_product_losses_refuse_cpu_tensors():
    from fresnel_amd import _binding as B
    from fresnel_amd.losses import FrequencyDomainLoss, PhaseRetrievalLoss, wave_equation_loss
    x = torch.rand(1, 3, 8, 8)
    for fn in (lambda: FrequencyDomainLoss()(x, x), lambda: PhaseRetrievalLoss()(x, x, x[:, 0]),
               lambda: wave_equation_loss(x, 0.05)):
        with pytest.raises(B.FgsError):
            fn()


@pytest.mark.gpu
def test_hip_losses_match_reference_fixtures_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires an MI355X (torch.cuda unavailable)")
    from fresnel_amd import losses
    _run(losses, torch.device("cuda:0"))


@pytest.mark.gpu
def test_hip_losses_match_checker_at_render_size_gpu():
    """B = 3 images of 3 x 160 x 96 (non-square, not a power of two), learnable wavelength: loss and the gradients
    with respect to rendered, target, depth and the wavelength against the torch formulation run in float64."""
    from fresnel_amd import losses
    from oracle import torch_losses
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(3)
    Bn, H, W = 3, 160, 96
    rendered = rs.uniform(0, 1, (Bn, 3, H, W)).astype(np.float32)
    rendered[1, :, :7, :5] = 0.0
    target = rs.uniform(0, 1, (Bn, 3, H, W)).astype(np.float32)
    depth = rs.uniform(0.1, 2.5, (Bn, H, W)).astype(np.float32)

    def run(mod, dtype, device):
        r, t, d = [torch.tensor(a, dtype=dtype, device=device, requires_grad=True) for a in (rendered, target, depth)]
        wl = torch.tensor(0.0575, dtype=dtype, device=device, requires_grad=True)
        total = (mod.PhaseRetrievalLoss(focal_depth=0.7)(r, t, d, wavelength=wl) * 1.5 +
                 mod.FrequencyDomainLoss(cutoff=0.2, high_weight=3.0)(r, t) * 0.25 +
                 mod.wave_equation_loss(r, 0.05, pixel_spacing=1.0 / 96) * 1e-9)
        total.backward()
        return [float(total)] + [x.grad.detach().cpu().double().numpy() for x in (r, t, d, wl)]

    got = run(losses, torch.float32, dev)
    ref = run(torch_losses, torch.float64, torch.device("cpu"))
    assert abs(got[0] - ref[0]) <= TOL * abs(ref[0])
    for a, b, name in zip(got[1:], ref[1:], ["rendered", "target", "depth", "wavelength"]):
        assert rel_to_max(a, b) <= TOL, name


# ---- spectral losses on the column-FFT path ---------------------------------------------------------------------------
# fgs_fft2_exec runs rocFFT on the rows and k_colfft_plain<LOGN, TC, INV> on the columns when H is 64 ... 1024 (a power of
# two): TC = 16 columns per block for LOGN 6-9, TC = 8 for LOGN 10; INV = false in the losses' forward, true in their
# backward.  A width that is not a multiple of TC leaves the last tile partial (lanes past W load zeros and store nothing).
# The reductions run at most 1024 blocks of 256 threads and grid-stride over the rest: k_spec_reduce over B C H W elements,
# k_spec_unpack over B H W pixels -- a second pass from 262 145 elements on.
#   name                     (B, C, H, W)       column pass                        k_spec_reduce / k_spec_unpack passes
#   train_4x3x256x256        training default   <8, 16> both ways, full tiles      3 / 1
#   profiled_8x3x512x512     DESIGN.md §4       <9, 16> both ways, full tiles      24 / 8
#   fast_2x3x64x64           --fast_mode        <6, 16> both ways, full tiles      1 / 1
#   c1_3x1x128x100           C = 1              <7, 16> both ways, partial tile    1 / 1
#   h1024_1x3x1024x36        LOGN 10            <10, 8> both ways, partial tile    1 / 1
#   prime_2x3x512x97         prime width        <9, 16> both ways, partial tile    2 / 1
#   narrow_1x1x64x12         W below one tile   <6, 16> both ways, one partial     1 / 1
#   rocfft2d_2x3x96x200      control            rocFFT's 2-D plan                  1 / 1
# value: ((B, C, H, W), FrequencyDomainLoss (cutoff, high_weight), PhaseRetrievalLoss (focal_depth, wavelength),
#         depth given as (B, 1, H, W))
SPECTRAL_CASES = {
    "train_4x3x256x256": ((4, 3, 256, 256), (0.1, 2.0), (0.5, 0.05), False),
    "profiled_8x3x512x512": ((8, 3, 512, 512), (0.15, 3.0), (0.7, 0.0575), False),
    "fast_2x3x64x64": ((2, 3, 64, 64), (0.25, 0.5), (1.0, 0.0635), True),
    "c1_3x1x128x100": ((3, 1, 128, 100), (0.2, 4.0), (0.3, 0.041), False),
    "h1024_1x3x1024x36": ((1, 3, 1024, 36), (0.05, 1.5), (0.9, 0.07), False),
    "prime_2x3x512x97": ((2, 3, 512, 97), (0.3, 0.25), (0.45, 0.05), False),
    "narrow_1x1x64x12": ((1, 1, 64, 12), (0.35, 2.5), (0.6, 0.052), False),
    "rocfft2d_2x3x96x200": ((2, 3, 96, 200), (0.12, 5.0), (0.8, 0.06), False),
}
G_LOSS = 0.75  # upstream gradient of every spectral-loss call below (the kernels scale by it)


def _spectral_inputs(shape, seed, depth4=False):
    Bn, C, H, W = shape
    rs = np.random.RandomState(seed)
    rendered = rs.uniform(0, 1, shape).astype(np.float32)
    target = rs.uniform(0, 1, shape).astype(np.float32)
    depth = rs.uniform(0.1, 2.5, (Bn, 1, H, W) if depth4 else (Bn, H, W)).astype(np.float32)
    return rendered, target, depth


def _spectral(mod, kind, params, arrays, dtype, device, need=(True, True, True, True)):
    """loss and gradients of FrequencyDomainLoss(cutoff, high_weight) (kind "freq": rendered, target) or
    PhaseRetrievalLoss(focal_depth) with a wavelength tensor (kind "phase": rendered, target, depth, wavelength), times G_LOSS;
    `need`: which inputs require a gradient (None in the result for the others)."""
    r, t, d = [torch.tensor(a, dtype=dtype, device=device, requires_grad=n) for a, n in zip(arrays, need)]
    if kind == "freq":
        loss = mod.FrequencyDomainLoss(cutoff=params[0], high_weight=params[1])(r, t)
        ins = (r, t)
    else:
        wl = torch.tensor(params[1], dtype=dtype, device=device, requires_grad=need[3])
        loss = mod.PhaseRetrievalLoss(focal_depth=params[0])(r, t, d, wavelength=wl)
        ins = (r, t, d, wl)
    (loss * G_LOSS).backward()
    return [loss.detach().cpu().double().numpy()] + [None if x.grad is None else x.grad.detach().cpu().double().numpy()
                                                     for x in ins]


def _assert_spectral_matches_checker(kind, params, arrays, where, arrays64=None):
    """The HIP loss against the checker: loss within 1e-4 relative and every gradient within 1e-4 of its max of the checker's
    float32 run, or -- where that run is itself more than 5e-5 from the float64 one -- the referee rule."""
    from fresnel_amd import losses
    from oracle import torch_losses
    cpu = torch.device("cpu")
    got = _spectral(losses, kind, params, arrays, torch.float32, _dev())
    r32 = _spectral(torch_losses, kind, params, arrays, torch.float32, cpu)
    r64 = _spectral(torch_losses, kind, params, arrays if arrays64 is None else arrays64, torch.float64, cpu)
    names = ["loss", "rendered", "target", "depth", "wavelength"]
    for a, b32, b64, name in zip(got, r32, r64, names):
        assert np.isfinite(a).all(), (where, name)
        assert_with_referee(a, b32, b64, f"{where} {kind} {name}")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["freq", "phase"])
@pytest.mark.parametrize("name", list(SPECTRAL_CASES))
def test_hip_spectral_losses_match_checker_gpu(name, kind):
    """FrequencyDomainLoss / PhaseRetrievalLoss (learnable wavelength) at the shapes of the table above: every
    k_colfft_plain instance in both directions (LOGN 6, 7, 8, 9 with 16-column tiles, LOGN 10 with 8-column tiles; full and
    partial tiles, a width below one tile), the grid-stride loops of k_spec_reduce (up to 24 passes) and k_spec_unpack (up to 8),
    C = 1 and the (B, 1, H, W) depth form, and rocFFT's 2-D plan as the control."""
    shape, freq, phase, depth4 = SPECTRAL_CASES[name]
    arrays = _spectral_inputs(shape, 20 + list(SPECTRAL_CASES).index(name), depth4)
    _assert_spectral_matches_checker(kind, freq if kind == "freq" else phase, arrays, name)


@pytest.mark.gpu
def test_hip_spectral_losses_are_bitwise_repeatable_gpu():
    """8 x 3 x 512^2 (grid-stride loops, 1024 partial sums): two calls give bitwise-identical losses and gradients -- the
    reductions are deterministic (fixed block partials summed in block order), as fgs_spectral.hip states."""
    dev = _dev()
    from fresnel_amd import losses
    shape, freq, phase, _ = SPECTRAL_CASES["profiled_8x3x512x512"]
    arrays = _spectral_inputs(shape, 5)
    for kind, params in (("freq", freq), ("phase", phase)):
        a = _spectral(losses, kind, params, arrays, torch.float32, dev)
        b = _spectral(losses, kind, params, arrays, torch.float32, dev)
        for x, y, what in zip(a, b, ["loss", "rendered", "target", "depth", "wavelength"]):
            assert np.array_equal(x, y), (kind, what)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(4, 3, 256, 256), (2, 3, 96, 200)])
def test_hip_spectral_losses_training_call_pattern_gpu(shape):
    """Training passes target and depth without requires_grad (the backward gets g_target = g_depth = NULL) and the
    wavelength as the module's Python float: dL/drendered is bitwise the gradient of the all-requires_grad call, and
    target.grad / depth.grad stay None."""
    dev = _dev()
    from fresnel_amd import losses
    rendered, target, depth = _spectral_inputs(shape, 6)
    # all inputs require a gradient
    full_f = _spectral(losses, "freq", (0.1, 2.0), (rendered, target, depth), torch.float32, dev)
    full_p = _spectral(losses, "phase", (0.5, 0.05), (rendered, target, depth), torch.float32, dev)
    # the training call
    r = torch.tensor(rendered, device=dev, requires_grad=True)
    t, d = torch.tensor(target, device=dev), torch.tensor(depth, device=dev)
    loss_f = losses.FrequencyDomainLoss(cutoff=0.1, high_weight=2.0)(r, t)
    (loss_f * G_LOSS).backward()
    assert t.grad is None
    assert np.array_equal(loss_f.detach().cpu().double().numpy(), full_f[0])
    assert np.array_equal(r.grad.cpu().double().numpy(), full_f[1])
    r = torch.tensor(rendered, device=dev, requires_grad=True)
    loss_p = losses.PhaseRetrievalLoss(wavelength=0.05, focal_depth=0.5)(r, t, d)
    (loss_p * G_LOSS).backward()
    assert t.grad is None and d.grad is None
    assert np.array_equal(loss_p.detach().cpu().double().numpy(), full_p[0])
    assert np.array_equal(r.grad.cpu().double().numpy(), full_p[1])


# ---- mask-boundary known answers --------------------------------------------------------------------------------------
# target = c0, rendered = c0 + eps cos(2 pi (kx x / W + ky y / H)): the spectra differ at +-(kx, ky) only, by eps H W / 2
# (F_t is zero there, F_r real and positive), so with n = B C H W and w the mask weight of the bin (the same at -(kx, ky))
#   loss = w eps^2 H W / 2,     dL/drendered = 2 w eps cos(2 pi (kx x / W + ky y / H)) / (B C)   (times the upstream gradient).
# (dL/dtarget is not a known answer: |F_t| = 0 at the bin, where |.| has no derivative.)  The probes are bins whose float32
# radius sqrt(u^2 + v^2) -- u, v from fftfreq in float32, each product and the sum rounded -- EQUALS the float32 cutoff (the
# checker's `<` gives them high_weight), plus one just inside and one just outside.  (24, 7) / (7, 24) at 100 x 100, cutoff
# 0.25: the radius is the cutoff when the two squares are rounded separately and falls just below it when one of them is fused
# into the sum (fma(u, u, v v), resp. fma(v, v, u u)).  The expected weight is that of IEEE float32 arithmetic (numpy: products
# and sum rounded, sqrt correctly rounded, then `<`), which the checker's mask equals on every probe but one: (6, 10) at 50 x 40
# (radius 0.25 in exact arithmetic) has a float32 radius^2 one ulp below 0.0625 whose exact square root lies 2^-53 below the
# midpoint between 0.25 and the float under it.  A correctly rounded sqrt (IEEE, numpy, the kernel's) puts that bin inside the
# circle; a sqrt with an error just over half an ulp rounds it onto the circle -- and the checker's mask at that bin has been
# seen to differ between host CPUs.
# (H, W, cutoff, [(kx, ky), ...])
MASK_PROBES = [
    (100, 100, 0.1, [(6, 8), (8, 6), (10, 0), (5, 8), (7, 8)]),
    (256, 256, 0.078125, [(12, 16), (20, 0), (19, 0), (21, 0), (12, 15), (12, 17)]),
    (50, 40, 0.25, [(6, 10), (10, 0), (9, 0), (11, 0)]),
    (100, 100, 0.25, [(24, 7), (7, 24), (23, 7), (25, 7)]),
]
MASK_HIGH_WEIGHT = 3.0
MASK_C0, MASK_EPS = 0.5, 0.25


def _mask_probe(H, W, kx, ky, shape_bc=(1, 3)):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    wave = np.cos(2.0 * np.pi * (kx * x / W + ky * y / H))
    rendered = np.broadcast_to(MASK_C0 + MASK_EPS * wave, shape_bc + (H, W)).copy()
    target = np.full(shape_bc + (H, W), MASK_C0)
    return rendered, target, wave


def _mask_closed_form(H, W, w, wave, shape_bc=(1, 3)):
    loss = w * MASK_EPS ** 2 * H * W / 2.0
    grad = np.broadcast_to(2.0 * w * MASK_EPS * wave / (shape_bc[0] * shape_bc[1]), shape_bc + (H, W))
    return loss, grad


def _radius32(H, W, kx, ky):
    """(sqrt(u^2 + v^2), u^2 + v^2) in IEEE float32, u and v as torch.fft.fftfreq forms them."""
    def f(k, n):
        return np.float32(k if k < (n + 1) // 2 else k - n) * (np.float32(1.0) / np.float32(n))
    u, v = f(kx, W), f(ky, H)
    r2 = np.float32(u * u) + np.float32(v * v)
    return np.sqrt(r2), r2


def _weight32(H, W, cutoff, kx, ky):
    return 1.0 if _radius32(H, W, kx, ky)[0] < np.float32(cutoff) else MASK_HIGH_WEIGHT


def _sqrt_tie(r2):
    """The exact square root of the float32 `r2` lies within 2^-40 (relative) of a midpoint between two floats."""
    from fractions import Fraction
    r = np.sqrt(r2)
    for n in (np.nextafter(r, np.float32(0)), np.nextafter(r, np.float32(1))):
        m = (Fraction(float(r)) + Fraction(float(n))) / 2
        if abs(Fraction(float(r2)) - m * m) <= m * m / 2 ** 40:
            return True
    return False


def test_checker_frequency_mask_boundary_known_answers_cpu():
    """The checker's FrequencyDomainLoss in float64 gives the closed form with the weights of its own float32 mask at every
    probe; that mask is IEEE float32's (bins exactly on the float32 circle get high_weight) except at the one probe whose
    float32 radius is a rounding tie of the square root."""
    from oracle import torch_losses
    on_circle, ties = 0, 0
    for H, W, cutoff, bins in MASK_PROBES:
        mod = torch_losses.FrequencyDomainLoss(cutoff=cutoff, high_weight=MASK_HIGH_WEIGHT)
        mask = mod._weight(H, W, torch.device("cpu"))
        assert mask.dtype == torch.float32
        for kx, ky in bins:
            w = float(mask[ky, kx])
            assert w == float(mask[(H - ky) % H, (W - kx) % W])
            radius, r2 = _radius32(H, W, kx, ky)
            if _sqrt_tie(r2):
                ties += 1
            else:
                assert w == _weight32(H, W, cutoff, kx, ky), (H, W, cutoff, kx, ky)
            if radius == np.float32(cutoff):
                assert w == MASK_HIGH_WEIGHT, (H, W, cutoff, kx, ky)
                on_circle += 1
            rendered, target, wave = _mask_probe(H, W, kx, ky)
            r = torch.tensor(rendered, dtype=torch.float64, requires_grad=True)
            loss = mod(r, torch.tensor(target, dtype=torch.float64))
            loss.backward()
            want_loss, want_grad = _mask_closed_form(H, W, w, wave)
            assert abs(loss.item() - want_loss) <= 1e-9 * want_loss, (H, W, kx, ky, loss.item(), want_loss)
            assert rel_to_max(r.grad.numpy(), want_grad) <= 1e-9, (H, W, kx, ky)
    assert on_circle == 7 and ties == 1


@pytest.mark.gpu
@pytest.mark.parametrize("probe", range(len(MASK_PROBES)))
def test_hip_frequency_mask_boundary_known_answers_gpu(probe):
    """The HIP FrequencyDomainLoss at the mask-boundary probes: loss within 1e-4 relative and dL/drendered within 1e-4 of its
    max of the closed form with the IEEE float32 weights, the checker's (a bin on the circle that moved across the `<` would
    change its weight from high_weight = 3 to 1).  256 x 256 runs on the column path, the others on rocFFT's 2-D plan."""
    dev = _dev()
    from fresnel_amd import losses
    H, W, cutoff, bins = MASK_PROBES[probe]
    for kx, ky in bins:
        rendered, target, wave = _mask_probe(H, W, kx, ky)
        r = torch.tensor(rendered, dtype=torch.float32, device=dev, requires_grad=True)
        loss = losses.FrequencyDomainLoss(cutoff=cutoff, high_weight=MASK_HIGH_WEIGHT)(
            r, torch.tensor(target, dtype=torch.float32, device=dev))
        (loss * G_LOSS).backward()
        want_loss, want_grad = _mask_closed_form(H, W, _weight32(H, W, cutoff, kx, ky), wave)
        assert abs(loss.item() - want_loss) <= TOL * want_loss, (H, W, cutoff, kx, ky, loss.item(), want_loss)
        assert rel_to_max(r.grad.cpu().double().numpy(), G_LOSS * want_grad) <= TOL, (H, W, cutoff, kx, ky)


# ---- edge values ------------------------------------------------------------------------------------------------------
CLAMP = np.float32(1e-8)  # PhaseRetrievalLoss: sqrt(clamp(I, min=1e-8)); the gradient passes on [1e-8, inf)


def _edge_inputs(shape, seed, focal):
    """Random images with pixels at 0, exactly at the clamp 1e-8 and negative (in rendered and target, partly at the same
    pixels), depth with pixels exactly at the focal plane; plus the float64 copies for the checker's float64 run, in which
    the clamp pixels hold the float64 1e-8 (float32(1e-8) is below it: there the float64 clamp would cut the gradient that
    the float32 clamp passes)."""
    rendered, target, depth = _spectral_inputs(shape, seed)
    rs = np.random.RandomState(seed + 1)
    for img in (rendered, target):
        sel = rs.randint(0, 4, img.shape)
        img[sel == 0] = np.where(rs.uniform(size=img.shape) < 0.5, 0.0, -rs.uniform(0, 0.5, img.shape))[sel == 0]
        img[sel == 1] = CLAMP
    rendered[0, :, :4, :4] = CLAMP  # overlapping edge pixels
    target[0, :, :4, :4] = 0.0
    depth[rs.uniform(size=depth.shape) < 0.2] = focal
    r64, t64 = [np.where(a == CLAMP, 1e-8, a.astype(np.float64)) for a in (rendered, target)]
    return (rendered, target, depth), (r64, t64, depth.astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (2, 3, 96, 200)])
def test_hip_spectral_losses_edge_values_gpu(shape):
    """Pixels at 0, at exactly 1e-8 and negative, depth pixels exactly at focal_depth (sign 0): both losses against the
    checker; the PhaseRetrievalLoss gradient is exactly 0 at every pixel below the clamp (clamp(min) passes none there) and
    the depth gradient exactly 0 on the focal plane (|.|'(0) = 0, as torch)."""
    focal = 0.5
    arrays, arrays64 = _edge_inputs(shape, 7, focal)
    _assert_spectral_matches_checker("freq", (0.2, 3.0), arrays, f"edges {shape}", arrays64)
    got = _assert_spectral_matches_checker("phase", (focal, 0.05), arrays, f"edges {shape}", arrays64)
    rendered, target, depth = arrays
    for img, grad, what in ((rendered, got[1], "rendered"), (target, got[2], "target")):
        below = img < CLAMP
        assert below.sum() > 0 and (img == CLAMP).sum() > 0
        assert (grad[below] == 0.0).all(), what
        assert (grad[img == CLAMP] != 0.0).all(), what
    assert (got[3][depth == focal] == 0.0).all()


@pytest.mark.gpu
def test_hip_spectral_losses_all_zero_and_identical_images_gpu():
    """An all-zero rendered batch (FrequencyDomainLoss: |F_r| = 0 everywhere, whose gradient is 0, as torch's): finite
    gradients, dL/drendered exactly 0, dL/dtarget as the checker's.  rendered == target (both losses, column path and rocFFT's
    2-D plan): loss exactly 0 and every gradient exactly 0."""
    dev = _dev()
    from fresnel_amd import losses
    for shape in ((2, 3, 64, 64), (2, 3, 96, 200)):
        rendered, target, depth = _spectral_inputs(shape, 8)
        zero = np.zeros_like(rendered)
        got = _assert_spectral_matches_checker("freq", (0.1, 2.0), (zero, target, depth), f"zero {shape}")
        assert (got[1] == 0.0).all() and np.abs(got[2]).max() > 0
        for kind, params in (("freq", (0.1, 2.0)), ("phase", (0.5, 0.05))):
            same = _spectral(losses, kind, params, (rendered, rendered, depth), torch.float32, dev)
            assert float(same[0]) == 0.0, (shape, kind)
            for g in same[1:]:
                assert (g == 0.0).all(), (shape, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 128, 128), (2, 3, 96, 200)])
def test_hip_phase_loss_large_phases_gpu(shape):
    """Phases of several hundred radians (wavelength 0.02, |depth - focal| up to 2.5: up to 785 rad), under the referee
    rule: the checker's own float32 run drifts from its float64 run there."""
    rendered, target, _ = _spectral_inputs(shape, 9)
    depth = np.random.RandomState(10).uniform(0.0, 3.0, (shape[0],) + shape[2:]).astype(np.float32)
    _assert_spectral_matches_checker("phase", (0.5, 0.02), (rendered, target, depth), f"large phases {shape}")


# ---- Helmholtz residual -----------------------------------------------------------------------------------------------
# value: (field shape, wavelength, pixel_spacing).  k_helmholtz grid-strides over the elements past 262 144 (3 passes at
# 4 x 3 x 256^2, 2 at 2 x 512^2); H = 1, W = 1 and H = W = 2 are the degenerate periodic stencils (both neighbours along an
# axis are the pixel itself, resp. the same pixel).
HELMHOLTZ_CASES = {
    "train_4x3x256x256": ((4, 3, 256, 256), 0.05, 1.0 / 256.0),
    "3d_2x512x512": ((2, 512, 512), 0.0635, 1.0 / 512.0),
    "h1_2x3x1x7": ((2, 3, 1, 7), 0.05, 1.0 / 64.0),
    "w1_3x6x1": ((3, 6, 1), 0.041, 1.0 / 32.0),
    "h1w1_2x3x1x1": ((2, 3, 1, 1), 0.05, 1.0 / 16.0),
    "h2w2_3x2x2": ((3, 2, 2), 0.07, 1.0 / 48.0),
    "3x5_2x3x3x5": ((2, 3, 3, 5), 0.0575, 1.0 / 64.0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HELMHOLTZ_CASES))
def test_hip_helmholtz_loss_matches_checker_gpu(name):
    """wave_equation_loss against the checker in float64, (B, H, W) and (B, C, H, W) inputs: loss within 1e-4 relative,
    dL/dU within 1e-4 of its max."""
    dev = _dev()
    from fresnel_amd import losses
    from oracle import torch_losses
    shape, wl, h = HELMHOLTZ_CASES[name]
    u0 = np.random.RandomState(11 + list(HELMHOLTZ_CASES).index(name)).uniform(-1, 1, shape).astype(np.float32)

    def run(mod, dtype, device):
        u = torch.tensor(u0, dtype=dtype, device=device, requires_grad=True)
        loss = mod.wave_equation_loss(u, wl, pixel_spacing=h)
        (loss * G_LOSS).backward()
        return loss.item(), u.grad.detach().cpu().double().numpy()

    got, ref = run(losses, torch.float32, dev), run(torch_losses, torch.float64, torch.device("cpu"))
    assert abs(got[0] - ref[0]) <= TOL * abs(ref[0]), (name, got[0], ref[0])
    assert rel_to_max(got[1], ref[1]) <= TOL, name
