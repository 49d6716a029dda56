"""SSIM loss (fresnel_amd/losses.py ssim / SSIM -> fgs_ssim_* in libfgs_hip.so, csrc/fgs_ssim.hip): the SSIM term of the
reference's training loss, `pytorch_msssim.ssim(clamp(rendered, 0, 1), target, data_range=1.0)` (TGD:904).

The checker (tests/ssim_checker.py) restates pytorch_msssim.ssim in fp64 torch (the package is not a dependency): separable
Gaussian window applied "valid" with grouped conv2d along H then W, C1 = (K1 R)^2, C2 = (K2 R)^2, per-channel means,
optional relu, mean.
CPU: the checker against the definition's known answers and torch's gradcheck; the closed-form backward the kernels
implement against the checker's autograd; the library's SSIM ABI and the API's argument checks; the training step's
default SSIM behaviour.  GPU: the product against the checker (loss <= 1e-5 absolute, every gradient <= 1e-4 of its
tensor's max), determinism, graph capture and the training step with --ssim_backend hip."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from helpers import rel_to_max
from ssim_checker import closed_form_grads, gauss_window, ref_ssim


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_checker_known_answers():
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 3, 20, 24, generator=g, dtype=torch.float64)
    assert abs(float(ref_ssim(x, x, data_range=1.0)) - 1.0) < 1e-12
    # constant planes a, b: sigma = 0, so S = (2ab + C1) / (a^2 + b^2 + C1) at every pixel (with the window renormalised
    # in fp64: the fp32 taps sum to 1 only to ~1e-7, which leaves sigma^2 ~ a^2 1e-7)
    w64 = gauss_window().double()
    w64 /= w64.sum()
    for a, b, R in ((0.3, 0.7, 1.0), (10.0, 200.0, 255.0), (0.5, 0.5, 1.0)):
        c1 = (0.01 * R) ** 2
        got = ref_ssim(torch.full((1, 2, 13, 17), a, dtype=torch.float64), torch.full((1, 2, 13, 17), b, dtype=torch.float64),
                       data_range=R, win=w64)
        assert abs(float(got) - (2 * a * b + c1) / (a * a + b * b + c1)) < 1e-12
    # a window that sums to 1 (the reference's eval helper builds one summing to ~2.07: not this definition)
    assert abs(float(gauss_window().sum()) - 1.0) < 1e-6


@pytest.mark.parametrize("size_average", [True, False])
def test_checker_gradcheck(size_average):
    g = torch.Generator().manual_seed(1)
    x = torch.rand(1, 2, 13, 17, generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.rand(1, 2, 13, 17, generator=g, dtype=torch.float64, requires_grad=True)
    for nonneg in (False, True):
        fn = lambda a, b: ref_ssim(a, b, data_range=1.0, size_average=size_average, win_size=7, nonnegative_ssim=nonneg)
        assert torch.autograd.gradcheck(fn, (x, y), eps=1e-6, atol=1e-8)


@pytest.mark.parametrize("case", ["mean", "per_image", "nonneg", "win7_sigma2_r255"])
def test_closed_form_backward_equals_autograd(case):
    g = torch.Generator().manual_seed(2)
    kw = dict(data_range=1.0, size_average=True, nonnegative_ssim=False)
    win = gauss_window()
    x = torch.rand(3, 2, 23, 29, generator=g, dtype=torch.float64)
    y = (x + 0.2 * torch.randn(x.shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    if case == "per_image":
        kw["size_average"] = False
    elif case == "nonneg":
        kw["nonnegative_ssim"] = True
        y[:, 0] = 1.0 - x[:, 0]  # anti-correlated planes: negative SSIM, clipped
    elif case == "win7_sigma2_r255":
        win, kw["data_range"] = gauss_window(7, 2.0), 255.0
        x, y = x * 255, y * 255
    x.requires_grad_(True)
    y.requires_grad_(True)
    loss = ref_ssim(x, y, win=win, **kw)
    g_out = torch.rand(loss.shape, generator=g, dtype=torch.float64) + 0.5
    gx, gy = torch.autograd.grad(loss, (x, y), g_out)
    cx, cy = closed_form_grads(x.detach(), y.detach(), g_out, win=win, **kw)
    assert float((cx - gx).abs().max()) <= 1e-12 * max(1.0, float(gx.abs().max()))
    assert float((cy - gy).abs().max()) <= 1e-12 * max(1.0, float(gy.abs().max()))
    if case == "nonneg":
        assert float(gx[:, 0].abs().max()) == 0.0 and float(gx[:, 1].abs().max()) > 0.0


@pytest.fixture(scope="module")
def lib():
    from fresnel_amd import build
    from fresnel_amd import _binding as B
    build.build()
    return B.load()


def _dims(B, images, channels, H, W, taps=11, flags=0):
    d = B.FgsSsimDims()
    d.images, d.channels, d.height, d.width = images, channels, H, W
    for i, w in enumerate(gauss_window(taps).tolist()):
        d.taps[i] = w
    d.num_taps, d.c1, d.c2, d.flags = taps, 1e-4, 9e-4, flags
    return d


def test_library_exports_the_ssim_entry_points(lib):
    for n in ("fgs_ssim_workspace_bytes", "fgs_ssim_forward", "fgs_ssim_backward"):
        assert hasattr(lib, n)


def test_ssim_workspace_arithmetic(lib):
    from fresnel_amd import _binding as B

    def a256(v):
        return (v + 255) // 256 * 256

    def ws(*args, **kw):
        s, c = ctypes.c_size_t(0), ctypes.c_size_t(0)
        B.check(lib.fgs_ssim_workspace_bytes(ctypes.byref(_dims(B, *args, **kw)), ctypes.byref(s), ctypes.byref(c)), "ws")
        return s.value, c.value

    for (n, C, H, W, taps), flags in (((8, 3, 512, 512, 11), 0), ((8, 3, 512, 512, 11), B.FGS_SSIM_GRAD_X),
                                      ((2, 3, 48, 40, 7), B.FGS_SSIM_GRAD_X | B.FGS_SSIM_GRAD_Y),
                                      ((3, 3, 67, 131, 11), B.FGS_SSIM_GRAD_Y | B.FGS_SSIM_PER_IMAGE),
                                      ((1, 1, 11, 11, 11), B.FGS_SSIM_GRAD_X | B.FGS_SSIM_NONNEGATIVE)):
        Ho, Wo, planes = H - taps + 1, W - taps + 1, n * C
        nmaps = 4 if flags & B.FGS_SSIM_GRAD_Y else 3 if flags & B.FGS_SSIM_GRAD_X else 0
        tiles = -(-Ho // 32) * -(-Wo // 64)
        assert ws(n, C, H, W, taps, flags) == (a256(planes * 8) + nmaps * a256(planes * Ho * Wo * 4), a256(planes * tiles * 8))
    for bad in (dict(taps=10), dict(taps=17), dict(H=10), dict(W=6, taps=7), dict(flags=16), dict(images=0)):
        args = dict(images=1, channels=3, H=32, W=32, taps=11, flags=0)
        args.update(bad)
        s, c = ctypes.c_size_t(0), ctypes.c_size_t(0)
        d = _dims(B, args["images"], args["channels"], args["H"], args["W"], min(args["taps"], 15), args["flags"])
        d.num_taps = args["taps"]
        assert lib.fgs_ssim_workspace_bytes(ctypes.byref(d), ctypes.byref(s), ctypes.byref(c)) < 0, bad


def test_ssim_argument_checks():
    from fresnel_amd import _binding as B
    from fresnel_amd.losses import SSIM, ssim
    x = torch.rand(1, 3, 32, 32)
    with pytest.raises(B.FgsError, match="no CPU fallback"):
        ssim(x, x)
    with pytest.raises(B.FgsError, match="no CPU fallback"):
        SSIM()(x, x)
    with pytest.raises(B.FgsError, match="odd"):
        ssim(x, x, win_size=10)
    with pytest.raises(B.FgsError, match="odd"):
        SSIM(win_size=10)
    with pytest.raises(B.FgsError, match="smaller"):
        ssim(torch.rand(1, 3, 10, 32), torch.rand(1, 3, 10, 32))
    with pytest.raises(B.FgsError, match="smaller"):
        SSIM()(torch.rand(1, 3, 32, 9), torch.rand(1, 3, 32, 9))
    with pytest.raises(B.FgsError, match="same dimensions"):
        ssim(x, torch.rand(1, 3, 32, 31))
    with pytest.raises(B.FgsError, match="same dimensions"):
        SSIM()(x, torch.rand(2, 3, 32, 32))
    v = torch.rand(1, 3, 16, 32, 32)
    with pytest.raises(B.FgsError, match="4-d"):
        ssim(v, v)
    with pytest.raises(B.FgsError, match="4-d"):
        SSIM()(v, v)
    with pytest.raises(B.FgsError, match="at most 15"):
        ssim(x, x, win_size=17)


def test_training_keeps_the_default_ssim_term():
    from fresnel_amd import train as T
    assert T.TrainingConfig().ssim_backend == "msssim"
    g = torch.Generator().manual_seed(4)
    r, t = torch.rand(2, 3, 32, 32, generator=g), torch.rand(2, 3, 32, 32, generator=g)
    rd, td = torch.rand(2, 32, 32, generator=g), torch.rand(2, 32, 32, generator=g)
    cfg = T.TrainingConfig(image_size=32)
    total, d = T.compute_losses(r, t, rd, td, cfg)
    # what the step computed before the backend switch existed, written out
    want = cfg.rgb_weight * F.l1_loss(r, t)
    keys = {"rgb", "depth", "total"}
    if T.SSIM_AVAILABLE:
        want = want + cfg.ssim_weight * (1.0 - T.ssim_fn(torch.clamp(r, 0, 1), t, data_range=1.0, size_average=True))
        keys.add("ssim")
    (rm, rs), (tm, ts) = T._global_mean_std(rd, None), T._global_mean_std(td, None)
    rn, tn = (rd - rm) / torch.clamp(rs, min=1e-4), (td - tm) / torch.clamp(ts, min=1e-4)
    want = want + cfg.depth_weight * F.l1_loss(rn, tn)
    assert set(d) == keys
    assert torch.equal(total, want)
    # the HIP backend: parsed from the command line, refused on the CPU with a clear message
    assert T.arg_parser().parse_args([]).ssim_backend == "msssim"
    assert T.arg_parser().parse_args(["--ssim_backend", "hip"]).ssim_backend == "hip"
    with pytest.raises(SystemExit):
        T.arg_parser().parse_args(["--ssim_backend", "torch"])
    with pytest.raises(ValueError, match="no CPU fallback"):
        T.compute_losses(r, t, rd, td, T.TrainingConfig(image_size=32, ssim_backend="hip"))
    with pytest.raises(ValueError, match="needs a GPU"):
        T.run_training(T.TrainingConfig(image_size=32, ssim_backend="hip", device="cpu"), log=lambda *a: None)


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires an MI355X (torch.cuda unavailable)")
    return torch.device("cuda:0")


GPU_CASES = {
    "2x3x48x40": ((2, 3, 48, 40), dict(data_range=1.0)),
    "single_output_pixel": ((1, 1, 11, 11), dict(data_range=1.0)),
    "ragged_3x3x67x131": ((3, 3, 67, 131), dict(data_range=1.0)),
    "config3_8x3x512x512": ((8, 3, 512, 512), dict(data_range=1.0)),
    "win7": ((2, 3, 48, 40), dict(data_range=1.0, win_size=7)),
    "sigma2": ((2, 3, 48, 40), dict(data_range=1.0, win_sigma=2.0)),
    "win7_sigma2_r255_per_image": ((2, 3, 70, 90), dict(data_range=255, win_size=7, win_sigma=2.0, size_average=False)),
    "per_image": ((4, 3, 64, 80), dict(data_range=1.0, size_average=False)),
    "win15_1d": ((2, 2, 40, 70), dict(data_range=1.0, win=gauss_window(15, 3.0))),
    "grad_y": ((2, 3, 67, 131), dict(data_range=1.0, grad_y=True)),
    "grad_y_per_image": ((2, 3, 48, 40), dict(data_range=1.0, grad_y=True, size_average=False)),
}


def _pair(shape, seed, data_range=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g)
    y = (x + 0.25 * torch.randn(shape, generator=g)).clamp(0, 1)
    return x * data_range, y * data_range


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_hip_ssim_matches_checker(name):
    from fresnel_amd.losses import ssim
    dev = _dev()
    shape, kw = GPU_CASES[name]
    kw = dict(kw)
    grad_y = kw.pop("grad_y", False)
    x, y = _pair(shape, 10, kw.get("data_range", 1.0))
    xd, yd = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(grad_y)
    loss = ssim(xd, yd, **kw)
    g_out = torch.rand(loss.shape) + 0.5
    loss.backward(g_out.to(dev))
    xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(grad_y)
    ref = ref_ssim(xr, yr, **kw)
    ref.backward(g_out.double())
    assert loss.shape == ref.shape
    assert float((loss.detach().cpu().double() - ref.detach()).abs().max()) <= 1e-5, (name, loss, ref)
    assert rel_to_max(xd.grad.cpu().numpy(), xr.grad.numpy()) <= 1e-4, name
    if grad_y:
        assert rel_to_max(yd.grad.cpu().numpy(), yr.grad.numpy()) <= 1e-4, name
    else:
        assert yd.grad is None


@pytest.mark.gpu
def test_hip_ssim_nonnegative_clips_planes_to_zero_gradient():
    from fresnel_amd.losses import ssim
    dev = _dev()
    x, y = _pair((3, 3, 48, 64), 11)
    y[:, 1] = 1.0 - x[:, 1]  # anti-correlated: negative SSIM on every channel-1 plane
    y[0] = 1.0 - x[0]       # and on all of image 0
    for size_average in (True, False):
        xd, yd = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
        loss = ssim(xd, yd, data_range=1.0, size_average=size_average, nonnegative_ssim=True)
        loss.backward(torch.ones_like(loss))
        xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(True)
        ref = ref_ssim(xr, yr, data_range=1.0, size_average=size_average, nonnegative_ssim=True)
        ref.backward(torch.ones_like(ref))
        cs = ref_ssim(x.double(), y.double(), data_range=1.0, per_channel=True)
        assert bool((cs[:, 1] < 0).all()) and bool((cs[0] < 0).all()) and bool((cs[1:, [0, 2]] > 0).all())
        assert float((loss.detach().cpu().double() - ref.detach()).abs().max()) <= 1e-5
        for t, r in ((xd, xr), (yd, yr)):
            gt = t.grad.cpu()
            assert rel_to_max(gt.numpy(), r.grad.numpy()) <= 1e-4
            clipped = (cs <= 0)
            assert bool((gt[clipped] == 0).all()) and float(gt[~clipped].abs().max()) > 0


@pytest.mark.gpu
def test_hip_ssim_repeats_bitwise_and_handles_identity_layout_and_retained_graphs():
    from fresnel_amd.losses import SSIM, ssim
    dev = _dev()
    x, y = _pair((4, 3, 96, 80), 12)
    x, y = x.to(dev), y.to(dev)

    def run(a, b, **kw):
        a = a.detach().clone().requires_grad_(True)
        b = b.detach().clone().requires_grad_(True)
        loss = ssim(a, b, data_range=1.0, **kw)
        loss.backward(torch.ones_like(loss))
        return loss.detach(), a.grad, b.grad

    r1, r2 = run(x, y), run(x, y)
    assert all(torch.equal(p, q) for p, q in zip(r1, r2))
    # ssim(x, x) = 1 and the gradient vanishes (fp32 rounding only, against the gradient of a perturbed pair)
    one = run(x, x)
    assert abs(float(one[0]) - 1.0) <= 1e-6
    assert float(one[1].abs().max()) <= 1e-4 * float(r1[1].abs().max())
    # non-contiguous inputs: the same values, the same result
    xt = x.transpose(2, 3).contiguous().transpose(2, 3)
    assert not xt.is_contiguous()
    rn = run(xt, y)
    assert torch.equal(rn[0], r1[0]) and torch.equal(rn[1], r1[1]) and torch.equal(rn[2], r1[2])
    # other dtypes are cast to fp32 on entry; the gradient comes back in the input's dtype
    rh = ssim(x.double(), y.double(), data_range=1.0)
    assert torch.equal(rh.detach(), r1[0])
    # the module form
    assert torch.equal(SSIM(data_range=1.0, channel=3)(x, y), r1[0])
    # a second backward through a retained graph: `saved` is not consumed
    a = x.detach().clone().requires_grad_(True)
    loss = ssim(a, y, data_range=1.0)
    loss.backward(retain_graph=True)
    g1 = a.grad.clone()
    a.grad = None
    loss.backward()
    assert torch.equal(a.grad, g1) and torch.equal(g1, r1[1])
    # no_grad: no factor maps, the same value
    with torch.no_grad():
        assert torch.equal(ssim(x, y, data_range=1.0), r1[0])


@pytest.mark.gpu
def test_hip_ssim_graph_capture_replays_the_eager_result():
    from fresnel_amd.losses import ssim
    dev = _dev()
    x0, y0 = _pair((2, 3, 128, 96), 13)
    x = x0.to(dev).requires_grad_(True)
    y = y0.to(dev)

    def fwd_bwd():
        loss = ssim(x, y, data_range=1.0)
        (gx,) = torch.autograd.grad(loss, (x,))
        return loss.detach(), gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            eager = fwd_bwd()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = fwd_bwd()
    with torch.no_grad():
        x.copy_(torch.rand_like(x))
        graph.replay()
        x.copy_(x0.to(dev))
        graph.replay()
    torch.cuda.synchronize()
    eager = fwd_bwd()
    assert torch.equal(static[0], eager[0]) and torch.equal(static[1], eager[1])


@pytest.mark.gpu
def test_training_step_with_hip_ssim():
    """--ssim_backend hip: the term is 1 - SSIM(clamp(rendered), target) (checked against the checker), the step stays
    free of host synchronisation, and the graph-replayed step trains like the eager one."""
    import numpy as np
    from fresnel_amd.dist import DPContext
    from fresnel_amd.train import (PatchGaussianDecoder, StepResult, SyntheticDataset, TrainingConfig, compute_losses,
                                   default_renderer_factory, make_optimizer, run_training, train_step)
    dev = _dev()
    # the term on a batch
    g = torch.Generator().manual_seed(14)
    r = torch.rand(2, 3, 64, 64, generator=g) * 1.2 - 0.1  # outside [0, 1] in places: the clamp matters
    t = torch.rand(2, 3, 64, 64, generator=g)
    rd, td = torch.rand(2, 64, 64, generator=g), torch.rand(2, 64, 64, generator=g)
    cfg = TrainingConfig(image_size=64, device="cuda:0", ssim_backend="hip")
    rr = r.to(dev).requires_grad_(True)
    total, d = compute_losses(rr, t.to(dev), rd.to(dev), td.to(dev), cfg)
    want = 1.0 - float(ref_ssim(r.clamp(0, 1).double(), t.double(), data_range=1.0))
    assert abs(float(d["ssim"]) - want) <= 1e-5
    base, _ = compute_losses(rr, t.to(dev), rd.to(dev), td.to(dev), TrainingConfig(image_size=64, device="cuda:0", ssim_weight=0.0))
    assert abs(float(total.detach()) - float(base.detach()) - cfg.ssim_weight * float(d["ssim"])) <= 1e-5
    total.backward()
    assert float(rr.grad.abs().max()) > 0

    # no host synchronisation inside the step
    cfg = TrainingConfig(batch_size=2, epochs=1, lr=1e-3, image_size=64, feature_size=6, feature_dim=16, gaussians_per_patch=4,
                         device="cuda:0", ssim_backend="hip")
    torch.manual_seed(0)
    model = PatchGaussianDecoder(cfg.feature_dim, cfg.gaussians_per_patch, grid=cfg.feature_size).to(dev)
    renderer, camera = default_renderer_factory(cfg, dev)
    opt = make_optimizer(model, cfg)
    dp = DPContext(device=dev)
    data = SyntheticDataset(8, cfg)
    rng = np.random.RandomState(0)
    batches = [data.batch([2 * i, 2 * i + 1], dev) for i in range(2)]
    train_step(model, renderer, camera, batches[0], opt, cfg, dp, pose_rng=rng)
    torch.cuda.synchronize()
    before = [p.detach().clone() for p in model.parameters()]
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = train_step(model, renderer, camera, batches[1], opt, cfg, dp, pose_rng=rng)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert isinstance(res, StepResult)
    ld = res.to_host()
    assert ld is not None and {"rgb", "depth", "ssim", "total"} <= set(ld) and 0.0 < ld["ssim"] < 2.0
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))

    # the graph-captured step trains like the eager step
    def run(graph, tag):
        c = TrainingConfig(batch_size=2, epochs=3, lr=2e-3, image_size=64, feature_size=6, feature_dim=16, gaussians_per_patch=4,
                           device="cuda:0", steps_per_epoch=4, save_interval=100, output_dir=str(tag), log_interval=1000,
                           hip_graph=graph, ssim_backend="hip")
        return run_training(c, log=lambda *a: None)

    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        m_e, h_e = run(False, tmp + "/e")
        m_g, h_g = run(True, tmp + "/g")
    assert len(h_g) == 3
    for a, b in zip(h_e, h_g):
        assert set(a) == set(b) and "ssim" in a
        for k in a:
            assert abs(a[k] - b[k]) <= 1e-4 * max(1.0, abs(a[k])), (k, a[k], b[k])
    for p, q in zip(m_e.parameters(), m_g.parameters()):
        assert torch.allclose(p, q, rtol=1e-3, atol=1e-5)
