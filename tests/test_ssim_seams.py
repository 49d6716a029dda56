"""SSIM kernels (csrc/fgs_ssim.hip) at their window, tile and reduction seams, against the fp64 checker
(tests/ssim_checker.py).

What tests/test_ssim.py cannot see, and what closes it here:

* The gradient's frame border.  An end tap of the default window is ~1e-3, so the outermost ring of dX is ~1e-3 of the
  tensor's max and a corner ~1e-6: "1e-4 of the tensor's max" passes a zeroed corner and a 5 % error along a whole row.
  `covered_error` divides both sides by the window weight that covers each pixel (`coverage`) before taking the same
  ratio of maxima, so a border pixel weighs as much as an interior one; the gate stays 1e-4.  The CPU part shows that the
  measure catches such mutants and that an fp32 restatement of the checker stays below 1e-5 under it on every case of the
  table below -- which is what makes 1e-4 a fair gate for the kernels.
* Orientation.  The forward is a correlation and the backward reverses the taps on the host; a Gaussian window hides an
  error in either.  Every seam runs with the asymmetric `ramp(n)` as well.
* Tile seams (64 x 32 tiles of OUTPUT pixels forward, of INPUT pixels backward), every odd tap count 1 ... 15 (the
  runtime-count path; 11 is compiled in), later trips of the reduction kernel's loops (more than 8, 32, 256 planes, more
  than 256 images, more than 64 tiles per plane), bright nearly flat planes (E[x^2] - mu^2 cancels in fp32), a NaN pixel
  (torch.relu keeps a NaN plane mean NaN; so must the kernels), and strided inputs.

GPU gates: loss within 1e-5 absolute of the checker, covered_error(dX), covered_error(dY) <= 1e-4, and the plain
rel-to-max <= 1e-4.  The one exception is the cancellation test, whose bound is 4 x the fp32 restatement's own distance
from fp64, computed in the test."""
import functools

import pytest
import torch

from helpers import rel_to_max
from ssim_checker import (box, closed_form_grads, coverage, covered_error, gauss_window, ramp, ref_ssim, ref_ssim_fp32)

GATE = 1e-4


# ---- the seam table ---------------------------------------------------------------------------------------------------
def _window(spec):
    kind, n = spec
    return {"gauss": gauss_window, "ramp": ramp, "box": box}[kind](n)


def _win_kw(spec):
    """How the window reaches ssim() / ref_ssim(): the Gaussian by `win_size` (the product builds its own taps)."""
    return dict(win_size=spec[1]) if spec[0] == "gauss" else dict(win=_window(spec))


def _table():
    t = {}

    def add(name, shape, spec, inputs="noisy", **kw):
        assert name not in t
        t[name] = (shape, spec, dict(data_range=1.0, **kw), inputs)

    # C1: forward tile seams, 11 taps (the compiled-in path): Ho x Wo output pixels around one tile of 32 x 64
    for Ho, Wo in ((32, 64), (32, 65), (33, 64), (33, 65), (1, 65), (33, 1), (31, 63), (31, 129), (33, 129), (1, 1), (32, 1),
                   (1, 63)):
        for spec in (("gauss", 11), ("ramp", 11)):
            add(f"fwd_{Ho}x{Wo}_{spec[0]}", (2, 2, Ho + 10, Wo + 10), spec)
    # C2: backward tile seams: the backward tiles the H x W input
    for H, W in ((31, 63), (32, 64), (32, 65), (33, 64), (33, 65), (64, 128), (65, 129), (31, 129)):
        for spec in (("gauss", 11), ("ramp", 11)):
            add(f"bwd_{H}x{W}_{spec[0]}", (2, 2, H, W), spec)
    # C3: every tap count (the runtime-count path but for 11): one output row / column past a tile both ways, a single
    # output row, a single output column.  n = 1: the window is [1], every variance is exactly 0, S is the luminance term.
    for n in (1, 3, 5, 7, 9, 13, 15):
        for spec in (("gauss", n), ("ramp", n)):
            for H, W in ((n + 32, n + 64), (n, n + 64), (n + 32, n)):
                add(f"taps{n}_{H}x{W}_{spec[0]}", (2, 2, H, W), spec)
    # C4: the box window: full weight on the end taps
    add("box11_43x75", (2, 2, 43, 75), ("box", 11))
    add("box11_11x75", (2, 2, 11, 75), ("box", 11))
    # C5: trips of the reduction kernel: 9 planes (the 8-plane unroll's guard), 33 (a wave's second trip), 257 planes and
    # images (the second trip of the mean's and of the per-image loop), 260 planes of 5 x 3 output pixels
    for (Bn, C), (H, W) in (((3, 3), (11, 11)), ((11, 3), (11, 11)), ((257, 1), (11, 11)), ((65, 4), (15, 13))):
        for size_average in (True, False):
            for nonneg in (False, True):
                add(f"reduce_{Bn}x{C}_{'mean' if size_average else 'per_image'}{'_nonneg' if nonneg else ''}", (Bn, C, H, W),
                    ("gauss", 11), "anti" if nonneg else "noisy", size_average=size_average, nonnegative_ssim=nonneg)
    # C6: more than 64 tiles per plane: the second trip over a plane's partial sums
    add("tiles65_11x4107", (1, 1, 11, 4107), ("gauss", 11))
    add("tiles84_171x843", (1, 2, 171, 843), ("gauss", 11))
    return t


TABLE = _table()


def _anti(p):
    """Planes made anti-correlated (y = 1 - x) by the "anti" inputs: every third, so each trip of each loop meets both kinds."""
    return p % 3 == 1


def _inputs(shape, inputs, seed=40):
    """x = rand, y = clamp(x + s randn, 0, 1) with the noise scale s = 0.25 (0.5 ... 1.5) drawn per plane, so that the planes'
    SSIM means differ; a random upstream gradient is drawn by the caller from the same generator."""
    g = torch.Generator().manual_seed(seed)
    Bn, C = shape[:2]
    x = torch.rand(shape, generator=g)
    scale = 0.25 * (0.5 + torch.rand(Bn, C, 1, 1, generator=g))
    y = (x + scale * torch.randn(shape, generator=g)).clamp(0, 1)
    if inputs == "anti":
        sel = _anti(torch.arange(Bn * C)).reshape(Bn, C)
        y[sel] = 1.0 - x[sel]
    return x, y, g


def _checker_run(fn, x, y, g_out, kw):
    xr, yr = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    loss = fn(xr, yr, **kw)
    loss.backward(g_out.to(loss.dtype))
    return loss.detach(), xr.grad, yr.grad


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and the fp64 checker's answers for one table entry, computed once and shared (read-only) by the tests."""
    shape, spec, kw, inputs = TABLE[name]
    kw = dict(kw, **_win_kw(spec))
    x, y, g = _inputs(shape, inputs)
    g_out = torch.rand((shape[0],) if not kw.get("size_average", True) else (), generator=g) + 0.5
    loss, gx, gy = _checker_run(ref_ssim, x.double(), y.double(), g_out, kw)
    cs = ref_ssim(x.double(), y.double(), per_channel=True, **{k: v for k, v in kw.items() if k != "nonnegative_ssim"})
    return dict(x=x, y=y, g_out=g_out, kw=kw, loss=loss, gx=gx, gy=gy, cs=cs, cov=coverage(shape[2], shape[3], _window(spec)))


# ---- CPU --------------------------------------------------------------------------------------------------------------
def test_windows_and_coverage():
    for n in (1, 3, 11, 15):
        for w in (ramp(n), box(n), gauss_window(n)):
            assert w.dtype == torch.float32 and w.numel() == n and abs(float(w.double().sum()) - 1.0) < 1e-6
    assert torch.equal(gauss_window(1), torch.ones(1)) and torch.equal(ramp(1), torch.ones(1))
    assert float(ramp(5)[4]) == pytest.approx(5.0 / 15.0) and not torch.equal(ramp(5), ramp(5).flip(0))
    # separable: the outer product of the 1-D coverages; interior = (sum of taps)^2, corner = first tap squared
    w = ramp(5).double()
    cov = coverage(12, 9, ramp(5))
    c1 = lambda L: torch.stack([w[max(0, p - (L - 5)):min(4, p) + 1].sum() for p in range(L)])
    assert cov.shape == (12, 9) and cov.dtype == torch.float64
    assert float((cov - torch.outer(c1(12), c1(9))).abs().max()) < 1e-15
    assert abs(float(cov[6, 4]) - 1.0) < 1e-6 and abs(float(cov[0, 0]) - float(w[0]) ** 2) < 1e-15 and float(cov.min()) > 0
    # covered_error: an error of e x coverage everywhere scores e / max|ref / cov|... and a perfect answer 0
    ref = torch.rand(1, 1, 12, 9, dtype=torch.float64) * cov
    assert covered_error(ref, ref, cov) == 0.0
    assert covered_error(ref + 1e-3 * cov, ref, cov) == pytest.approx(1e-3 / float((ref / cov).abs().max()), rel=1e-9)


@pytest.mark.parametrize("n", [3, 5, 11, 15])
def test_closed_form_equals_autograd_with_an_asymmetric_window(n):
    """The closed form the kernels implement against the checker's autograd under ramp(n): with a window that is not its
    own mirror image, the orientation of the transposed filter is part of the statement."""
    g = torch.Generator().manual_seed(41)
    x = torch.rand(2, 2, 23, 29, generator=g, dtype=torch.float64)
    y = (x + 0.2 * torch.randn(x.shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    for size_average in (True, False):
        kw = dict(data_range=1.0, size_average=size_average, win=ramp(n))
        g_out = torch.rand((2,) if not size_average else (), generator=g, dtype=torch.float64) + 0.5
        _, gx, gy = _checker_run(ref_ssim, x, y, g_out, kw)
        cx, cy = closed_form_grads(x, y, g_out, **kw)
        assert float((cx - gx).abs().max()) <= 1e-12 * max(1.0, float(gx.abs().max()))
        assert float((cy - gy).abs().max()) <= 1e-12 * max(1.0, float(gy.abs().max()))


def test_covered_error_catches_what_rel_to_max_passes():
    """Mutants of the REFERENCE gradient at 2x3x43x75 with the default window: a zeroed corner and a top row off by 5 % pass
    the plain 1e-4-of-max rule; all of them score above 1e-2 under covered_error."""
    g = torch.Generator().manual_seed(42)
    x = torch.rand(2, 3, 43, 75, generator=g, dtype=torch.float64)
    y = (x + 0.25 * torch.randn(x.shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    g_out = torch.tensor(1.0, dtype=torch.float64)
    _, gx, _ = _checker_run(ref_ssim, x, y, g_out, dict(data_range=1.0))
    cov = coverage(43, 75, gauss_window())
    assert covered_error(gx, gx, cov) == 0.0
    corner, row, col = gx.clone(), gx.clone(), gx.clone()
    corner[..., 0, 0] = 0.0
    row[..., 0, :] *= 1.05
    col[..., :, -1] = 0.0
    for name, m, hidden in (("corner", corner, True), ("row", row, True), ("column", col, False)):
        plain, cover = rel_to_max(m.numpy(), gx.numpy()), covered_error(m, gx, cov)
        print(f"mutant {name}: rel_to_max {plain:.2e}, covered_error {cover:.2e}")
        assert cover > 1e-2, name
        if hidden:
            assert plain < 1e-4, name  # the gap the new measure closes
    # a backward that does not mirror the taps (a correlation where the transpose is a convolution): invisible with the
    # Gaussian window, gross with ramp(11)
    w = ramp(11)
    _, gx, gy = _checker_run(ref_ssim, x, y, g_out, dict(data_range=1.0, win=w))
    bx, by = closed_form_grads(x, y, g_out, data_range=1.0, win=w, win_t=w.flip(0))
    cov = coverage(43, 75, w)
    print(f"unflipped taps, ramp(11): covered_error {covered_error(bx, gx, cov):.2e} / {covered_error(by, gy, cov):.2e}")
    assert covered_error(bx, gx, cov) > 1e-2 and covered_error(by, gy, cov) > 1e-2
    _, gx, _ = _checker_run(ref_ssim, x, y, g_out, dict(data_range=1.0))
    sx, _ = closed_form_grads(x, y, g_out, data_range=1.0, win=gauss_window(), win_t=gauss_window().flip(0))
    assert covered_error(sx, gx, coverage(43, 75, gauss_window())) < 1e-9


@pytest.mark.parametrize("name", list(TABLE))
def test_fp32_restatement_stays_within_the_gate(name):
    """The condition that makes 1e-4 a meaningful gate for the kernels: the checker's arithmetic in fp32 is within 1e-5
    (covered_error) of fp64 on both gradients, and within 1e-6 on the loss, at every case of the GPU table."""
    c = _case(name)
    loss, gx, gy = _checker_run(ref_ssim_fp32, c["x"], c["y"], c["g_out"], c["kw"])
    assert loss.dtype == torch.float32 and gx.dtype == torch.float32
    e_l = float((loss.double() - c["loss"]).abs().max())
    e_x, e_y = covered_error(gx, c["gx"], c["cov"]), covered_error(gy, c["gy"], c["cov"])
    print(f"{name}: fp32 restatement loss {e_l:.2e}, dX {e_x:.2e}, dY {e_y:.2e} (covered)")
    assert e_l <= 1e-6 and e_x <= 1e-5 and e_y <= 1e-5
    # the clipping cases: no plane mean sits where fp32 and fp64 could disagree about its sign
    assert float(c["cs"].abs().min()) > 1e-3
    if c["kw"].get("nonnegative_ssim"):
        sel = _anti(torch.arange(c["cs"].numel())).reshape(c["cs"].shape)
        assert bool((c["cs"][sel] < 0).all()) and bool((c["cs"][~sel] > 0).all())


# ---- GPU --------------------------------------------------------------------------------------------------------------
def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires an MI355X (torch.cuda unavailable)")
    return torch.device("cuda:0")


def _hip_run(x, y, g_out, kw):
    from fresnel_amd.losses import ssim
    dev = _dev()
    xd, yd = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    loss = ssim(xd, yd, **kw)
    loss.backward(g_out.to(dev))
    return loss.detach().cpu(), xd.grad.cpu(), yd.grad.cpu()


def _gates(what, got, want, cov):
    """The common gates; `got` / `want` = (loss, dX, dY).  Returns the figures."""
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape and got[2].shape == want[2].shape
    e_l = float((got[0].double() - want[0]).abs().max())
    fig = [e_l]
    for t, (a, b) in (("dX", (got[1], want[1])), ("dY", (got[2], want[2]))):
        fig += [covered_error(a, b, cov), rel_to_max(a.double().numpy(), b.numpy())]
    print(f"{what}: loss {e_l:.2e}; dX covered {fig[1]:.2e} plain {fig[2]:.2e}; dY covered {fig[3]:.2e} plain {fig[4]:.2e}")
    assert e_l <= 1e-5, (what, got[0], want[0])
    assert max(fig[1:]) <= GATE, (what, fig)
    return fig


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_hip_ssim_seams(name):
    c = _case(name)
    got = _hip_run(c["x"], c["y"], c["g_out"], c["kw"])
    _gates(name, got, (c["loss"], c["gx"], c["gy"]), c["cov"])
    if c["kw"].get("nonnegative_ssim"):
        clipped = c["cs"] <= 0
        assert bool(clipped.any()) and not bool(clipped.all())
        for gt in got[1:]:
            assert bool((gt[clipped] == 0).all()) and bool((gt[~clipped].flatten(1).abs().max(1)[0] > 0).all())


CANCELLATION = {
    # bright, nearly flat planes: E[x^2] ~ 4e4 against a variance of 0.25
    "r255_200_pm_0.5": (255.0, 200.0, 0.5),
    # the same at data_range 1: E[x^2] ~ 0.81 against a variance of 4e-6
    "r1_0.9_pm_0.002": (1.0, 0.9, 0.002),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CANCELLATION))
def test_hip_ssim_under_cancellation_tracks_the_fp32_restatement(name):
    """E[x^2] - mu^2 in fp32 on bright, nearly flat planes: any fp32 formulation loses digits here, the reference included,
    so the bound is not the 1e-4 gate but 4 x the fp32 restatement's own distance from fp64 on the same inputs (the factor:
    another summation order -- the kernels filter W then H, the restatement H then W -- and FMA contraction)."""
    data_range, level, sd = CANCELLATION[name]
    g = torch.Generator().manual_seed(43)
    shape = (2, 3, 43, 75)
    x = (level + sd * torch.randn(shape, generator=g)).float()
    y = (x + sd * torch.randn(shape, generator=g)).float()
    g_out = torch.rand((), generator=g) + 0.5
    kw = dict(data_range=data_range)
    cov = coverage(43, 75, gauss_window())
    want = _checker_run(ref_ssim, x.double(), y.double(), g_out, kw)
    r32 = _checker_run(ref_ssim_fp32, x, y, g_out, kw)
    got = _hip_run(x, y, g_out, kw)
    figures = []
    for what, a in (("fp32 restatement", r32), ("kernels", got)):
        f = (float((a[0].double() - want[0]).abs()), covered_error(a[1], want[1], cov), covered_error(a[2], want[2], cov))
        print(f"{name}: {what}: loss {f[0]:.3e}, dX {f[1]:.3e}, dY {f[2]:.3e} (covered) from fp64")
        figures.append(f)
    for k, what in enumerate(("loss", "dX", "dY")):
        assert figures[1][k] <= 4.0 * figures[0][k], (name, what, figures)


@pytest.mark.gpu
@pytest.mark.parametrize("nonneg", [False, True])
@pytest.mark.parametrize("size_average", [True, False])
def test_hip_ssim_nan_pixel_follows_the_checker(size_average, nonneg):
    """One NaN pixel well inside one plane of x.  Whatever the fp64 torch checker does, the kernels do: the plane's mean is
    NaN (torch.relu keeps it NaN), so the scalar loss, or that image's entry, is NaN; the gradient is NaN exactly where the
    checker's is (the (2n - 1)^2 pixels whose windows meet the NaN's windows) and meets the gates everywhere else."""
    shape, pos = (3, 3, 43, 75), (1, 1, 20, 37)
    x, y, g = _inputs(shape, "anti" if nonneg else "noisy", seed=44)
    x[pos] = float("nan")
    g_out = torch.rand((shape[0],) if not size_average else (), generator=g) + 0.5
    kw = dict(data_range=1.0, size_average=size_average, nonnegative_ssim=nonneg)
    want = _checker_run(ref_ssim, x.double(), y.double(), g_out, kw)
    got = _hip_run(x, y, g_out, kw)
    # what the checker does, stated: the NaN reaches the loss with and without the relu, and a 21 x 21 patch of one plane
    nan_l = torch.isnan(want[0])
    assert bool(nan_l.all()) if size_average else nan_l.tolist() == [False, True, False]
    for w in want[1:]:
        patch = torch.zeros(shape, dtype=torch.bool)
        patch[pos[0], pos[1], pos[2] - 10:pos[2] + 11, pos[3] - 10:pos[3] + 11] = True
        assert torch.equal(torch.isnan(w), patch)
    assert torch.equal(torch.isnan(got[0]), nan_l), (got[0], want[0])
    assert torch.equal(torch.isnan(got[1]), torch.isnan(want[1])) and torch.equal(torch.isnan(got[2]), torch.isnan(want[2]))
    clean = lambda t: torch.nan_to_num(t, nan=0.0)
    _gates(f"nan mean={size_average} nonneg={nonneg}", tuple(clean(t) for t in got), tuple(clean(t) for t in want),
           coverage(43, 75, gauss_window()))
    if nonneg:  # the clipped planes stay exactly zero beside the NaN plane
        cs = ref_ssim(torch.nan_to_num(x, nan=0.5).double(), y.double(), data_range=1.0, per_channel=True)
        cs[pos[0], pos[1]] = float("nan")
        assert bool((cs <= 0).any())
        for gt in got[1:]:
            assert bool((gt[cs <= 0] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["crop_view", "channels_last"])
def test_hip_ssim_strided_inputs_give_the_contiguous_bits(layout):
    dev = _dev()
    from fresnel_amd.losses import ssim
    Bn, C, H, W = 2, 3, 43, 75
    g = torch.Generator().manual_seed(45)
    if layout == "crop_view":
        big = torch.rand(Bn, C, H + 9, W + 11, generator=g).to(dev)
        xv = big[..., 3:3 + H, 5:5 + W]
    else:
        xv = torch.rand(Bn, C, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    assert not xv.is_contiguous() and xv.shape == (Bn, C, H, W)
    y = (xv.cpu() + 0.25 * torch.randn(Bn, C, H, W, generator=g)).clamp(0, 1).to(dev)
    res = []
    for a in (xv, xv.contiguous()):
        a = a.detach().requires_grad_(True)
        assert a.stride() == (xv.stride() if len(res) == 0 else xv.contiguous().stride())
        b = y.clone().requires_grad_(True)
        loss = ssim(a, b, data_range=1.0, win=ramp(11))
        loss.backward()
        assert a.grad.shape == (Bn, C, H, W) and b.grad.shape == (Bn, C, H, W)
        res.append((loss.detach(), a.grad, b.grad))
    assert all(torch.equal(p, q) for p, q in zip(*res))
    assert float(res[0][1].abs().max()) > 0
