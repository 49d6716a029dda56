"""Per-pixel losses (fresnel_amd/losses.py pixel_losses -> fgs_pixel_loss_* in libfgs_hip.so, csrc/fgs_pixel_loss.hip): the
VLM-density-weighted L1, the Fresnel-zone boundary emphasis term and the normalised-depth L1 of the reference's
compute_losses (TGD:873-953), their training flags and the dataset's density maps.

The checker (tests/pixel_loss_checker.py) restates the terms in torch.  CPU: the checker and the training loop's torch
backend against the fixture G17 (the reference's own compute_losses on a (3,3,48,40) batch); the closed-form gradients the
kernels implement against the checker's fp64 autograd, including a batch split over two "ranks"; mask known answers; the
library's ABI and argument checks; flags and defaults; the dataset.  GPU: the product against the fp64 checker (terms
<= 1e-5 absolute, gradients <= 1e-4 of the tensor's max), exact ties, determinism, NaN propagation, two emulated ranks
through the staged calls, the two backends of compute_losses, and the training step.

Depth gradient near ties: d|u - v|/du flips sign where u = v, so a pixel whose fp64 |u - v| is below 1e-5 may land on
either side in fp32 and its gradient element then differs by 2 / (n s).  Such pixels are left out of the 1e-4 comparison
(they must be finite and at most twice the checker's maximum, and at most 1e-4 of all pixels may be left out)."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pixel_loss_checker as C
from helpers import load_golden, rel_to_max

ZONES = dict(num_zones=8, depth_range=(0.0, 1.0), threshold=0.02, soft=True)


# ---- CPU: the fixture ------------------------------------------------------------------------------------------------
def _g17(tag):
    g = load_golden("G17_pixel_losses_48x40")
    t = {k: torch.from_numpy(np.asarray(g[k])) for k in ("rendered", "target", "rendered_depth", "target_depth", "density")}
    want = {k: float(g[f"{tag}_{k}"]) for k in ("rgb", "depth", "total")}
    if tag == "a":
        want["boundary"] = float(g["a_boundary"])
    grads = torch.from_numpy(np.asarray(g[f"{tag}_grad_rendered"])), torch.from_numpy(np.asarray(g[f"{tag}_grad_rendered_depth"]))
    return g, t, want, grads


@pytest.mark.parametrize("tag", ["a", "b"])
def test_checker_matches_the_reference_fixture(tag):
    g, t, want, (gr, gd) = _g17(tag)
    r, rd = t["rendered"].clone().requires_grad_(True), t["rendered_depth"].clone().requires_grad_(True)
    terms = C.ref_pixel_losses(r, t["target"], rd, t["target_depth"], t["density"] if tag == "a" else None, float(g["vlm_weight"]),
                               ZONES if tag == "a" else None)
    assert set(terms) == set(want) - {"total"}
    total = terms["rgb"] + 0.1 * terms["depth"] + (float(g["boundary_weight"]) * terms["boundary"] if tag == "a" else 0.0)
    total.backward()
    for k, v in terms.items():
        assert abs(float(v.detach()) - want[k]) <= 1e-6 * abs(want[k]), (k, float(v.detach()), want[k])
    assert abs(float(total.detach()) - want["total"]) <= 1e-6 * abs(want["total"])
    assert rel_to_max(r.grad.numpy(), gr.numpy()) <= 1e-6 and rel_to_max(rd.grad.numpy(), gd.numpy()) <= 1e-6
    # the block of exact ties carries exactly zero gradient in the reference
    i, h, w = [int(v) for v in g["tie_block"]]
    assert float(gr[i, :, :h, :w].abs().max()) == 0.0 and float(gr.abs().max()) > 0.0


@pytest.mark.parametrize("tag", ["a", "b"])
def test_torch_backend_matches_the_reference_fixture(tag):
    from fresnel_amd import train as T
    g, t, want, (gr, gd) = _g17(tag)
    cfg = T.TrainingConfig(image_size=48, ssim_weight=0.0)  # (the fixture was made without pytorch_msssim)
    if tag == "a":
        cfg = T.TrainingConfig(image_size=48, ssim_weight=0.0, use_vlm_guidance=True, vlm_weight=float(g["vlm_weight"]),
                               use_fresnel_zones=True, num_fresnel_zones=int(g["num_zones"]),
                               boundary_weight=float(g["boundary_weight"]))
    r, rd = t["rendered"].clone().requires_grad_(True), t["rendered_depth"].clone().requires_grad_(True)
    total, terms = T.compute_losses(r, t["target"], rd, t["target_depth"], cfg, vlm_density=t["density"] if tag == "a" else None)
    total.backward()
    assert set(terms) == set(want)
    for k in want:
        assert abs(float(terms[k]) - want[k]) <= 1e-6 * abs(want[k]), (k, float(terms[k]), want[k])
    assert rel_to_max(r.grad.numpy(), gr.numpy()) <= 1e-6 and rel_to_max(rd.grad.numpy(), gd.numpy()) <= 1e-6
    # the density map and the zones do nothing unless their switches are on (TGD:875, 943)
    off, terms_off = T.compute_losses(t["rendered"], t["target"], t["rendered_depth"], t["target_depth"],
                                      T.TrainingConfig(image_size=48, ssim_weight=0.0, boundary_weight=0.1), vlm_density=t["density"])
    assert set(terms_off) == {"rgb", "depth", "total"} and abs(float(off) - float(np.asarray(g["b_total"]))) <= 1e-6


def test_product_mask_is_the_checkers_and_known_answers():
    from fresnel_amd.losses import fresnel_boundary_mask
    d = torch.tensor([0.0, 0.125, 0.5, 1.0, 0.0625, 0.4375, 0.13, 0.2, -0.3, 1.4])
    soft = fresnel_boundary_mask(d)
    sig = lambda z: 1.0 / (1.0 + math.exp(-z))
    assert torch.allclose(soft[:4], torch.full((4,), sig(10.0)), atol=1e-6)              # on a boundary
    assert torch.allclose(soft[4:6], torch.full((2,), sig(10.0 - 500.0 * 0.0625)), rtol=1e-4, atol=1e-12)  # mid-zone
    assert abs(float(soft[6]) - sig(500.0 * (0.02 - 0.005))) <= 1e-4                    # 0.005 from 0.125
    hard = fresnel_boundary_mask(d, soft=False)
    assert hard.tolist() == [1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 9, 11, generator=g) * 1.4 - 0.2
    for kw in (dict(), dict(soft=False), dict(num_zones=5, depth_range=(0.1, 2.0), threshold=0.05)):
        assert torch.equal(fresnel_boundary_mask(x, **kw), C.boundary_mask(x, **kw))
    assert fresnel_boundary_mask(x).shape == x.shape


# ---- CPU: the closed forms -------------------------------------------------------------------------------------------
def _inputs(shape, seed, dtype=torch.float64, half_density=True, tie_block=True):
    Bn, H, W = shape
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(Bn, 3, H, W, generator=g)
    r = (t + 0.25 * torch.randn(Bn, 3, H, W, generator=g)).clamp(0, 1)
    if tie_block:
        r[0, :, :5, :7] = 0.0
        t[0, :, :5, :7] = 0.0
    td = torch.rand(Bn, H, W, generator=g)
    rd = 0.3 + 2.0 * td + 0.5 * torch.randn(Bn, H, W, generator=g)
    den = 0.5 + torch.rand(Bn, 1, (H // 2) if half_density else H, (W // 2) if half_density else W, generator=g)
    return tuple(v.to(dtype) for v in (r, t, rd, td, den))


def test_closed_form_gradients_equal_autograd():
    r, t, rd, td, den = _inputs((3, 23, 29), 5)
    for soft in (True, False):
        zones = dict(ZONES, soft=soft)
        rr, rdd = r.clone().requires_grad_(True), rd.clone().requires_grad_(True)
        terms = C.ref_pixel_losses(rr, t, rdd, td, den, 0.5, zones)
        g = dict(rgb=torch.tensor(0.7, dtype=torch.float64), boundary=torch.tensor(1.3, dtype=torch.float64),
                 depth=torch.tensor(0.45, dtype=torch.float64))
        sum(g[k] * terms[k] for k in g).backward()
        w = C.density_weight(den, 0.5, r.shape[-2:], r.dtype)
        c_r, c_d = C.closed_form_grads(r, t, rd, td, w, C.boundary_mask(td, **zones), g["rgb"], g["boundary"], g["depth"])
        assert float((c_r - rr.grad).abs().max()) <= 1e-12 and float((c_d - rdd.grad).abs().max()) <= 1e-12
        assert float(c_r[0, :, :5, :7].abs().max()) == 0.0 and float(c_r.abs().max()) > 0


def test_closed_form_depth_gradient_over_two_ranks():
    """Two "ranks" hold half the batch each; mean, std, Q, P, N are global.  The formula reproduces autograd of the SUM of
    the ranks' local terms -- what differentiable all-reduces of the statistics compute."""
    r, t, rd, td, _ = _inputs((4, 19, 21), 6, tie_block=False)
    leaf = rd.clone().requires_grad_(True)
    u, v = C.normalise(leaf), C.normalise(td)
    halves = [slice(0, 2), slice(2, 4)]
    (sum((u[h] - v[h]).abs().mean() for h in halves) * 0.8).backward()
    sg = C.sgn(u.detach(), v)
    glob = (rd.numel(), rd.mean(), rd.std(), td.mean(), td.std(), sg.sum(), (sg * u.detach()).sum())
    for h in halves:
        _, c_d = C.closed_form_grads(r[h], t[h], rd[h], td[h], None, None, None, None, torch.tensor(0.8, dtype=torch.float64), glob)
        assert float((c_d - leaf.grad[h]).abs().max()) <= 1e-12
    # and the halves' terms average to the whole batch's term
    whole = C.ref_pixel_losses(r, t, rd, td)["depth"]
    assert abs(float(sum((u[h] - v[h]).abs().mean() for h in halves).detach()) / 2 - float(whole)) <= 1e-12


def test_constant_depth_clamps_the_std_and_gates_the_gradient():
    r, t, rd, td, _ = _inputs((2, 9, 8), 7)
    const = torch.full_like(rd, 0.37)
    leaf = const.clone().requires_grad_(True)
    loss = C.ref_pixel_losses(r, t, leaf, td)["depth"]
    loss.backward()
    # u = 0 everywhere, so the term is mean |v|; q - Q / N sums to zero and, v being symmetric enough, is small but NOT zero
    assert abs(float(loss.detach()) - float(C.normalise(td).abs().mean())) <= 1e-12
    _, c_d = C.closed_form_grads(r, t, const, td, None, None, None, None, torch.tensor(1.0, dtype=torch.float64))
    assert float((c_d - leaf.grad).abs().max()) <= 1e-12
    assert abs(float(c_d.sum())) <= 1e-9  # the gate removes the std's path; the mean's path leaves a zero-sum gradient
    # both maps constant: every pixel ties (u = v = 0) and the gradient is exactly zero
    leaf = const.clone().requires_grad_(True)
    C.ref_pixel_losses(r, t, leaf, torch.full_like(td, 0.5))["depth"].backward()
    _, c_d = C.closed_form_grads(r, t, const, torch.full_like(td, 0.5), None, None, None, None, torch.tensor(1.0, dtype=torch.float64))
    assert float(leaf.grad.abs().max()) == 0.0 and float(c_d.abs().max()) == 0.0


# ---- CPU: the library's ABI ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from fresnel_amd import build
    from fresnel_amd import _binding as B
    build.build()
    return B.load()


def _dims(B, images=2, H=48, W=40, flags=None, world=1, zones=8, threshold=0.02, vlm_weight=0.5):
    d = B.FgsPixelLossDims()
    d.images, d.height, d.width, d.world = images, H, W, world
    d.flags = B.FGS_PIXEL_RGB | B.FGS_PIXEL_DENSITY | B.FGS_PIXEL_BOUNDARY | B.FGS_PIXEL_DEPTH if flags is None else flags
    d.vlm_weight, d.threshold = vlm_weight, threshold
    table = torch.linspace(0.0, 1.0, zones + 1).tolist() if zones >= 0 else []
    for i, v in enumerate(table[:B.FGS_PIXEL_MAX_BOUNDARIES]):
        d.boundaries[i] = v
    d.num_boundaries = len(table)
    return d


def _ws(lib, d):
    s, c = ctypes.c_size_t(0), ctypes.c_size_t(0)
    return lib.fgs_pixel_loss_workspace_bytes(ctypes.byref(d), ctypes.byref(s), ctypes.byref(c)), s.value, c.value


def test_library_exports_the_pixel_loss_entry_points(lib):
    from fresnel_amd import _binding as B
    names = ["fgs_pixel_loss_workspace_bytes", "fgs_pixel_loss_stage1", "fgs_pixel_loss_stage2", "fgs_pixel_loss_stage3",
             "fgs_pixel_loss_forward", "fgs_pixel_loss_backward"]
    for n in names:
        assert hasattr(lib, n) and n in B.EXPORTED_SYMBOLS
    assert ctypes.sizeof(B.FgsPixelLossDims) == 4 * (8 + B.FGS_PIXEL_MAX_BOUNDARIES)
    assert B.FGS_PIXEL_CROSS_RANK == {1: slice(B.FGS_PIXEL_STAT_SUM_X, B.FGS_PIXEL_STAT_SUM_Y + 1),
                                      2: slice(B.FGS_PIXEL_STAT_SSD_X, B.FGS_PIXEL_STAT_SSD_Y + 1),
                                      3: slice(B.FGS_PIXEL_STAT_SGN, B.FGS_PIXEL_STAT_SGN_U + 1)}


def test_pixel_loss_workspace_sizes(lib):
    from fresnel_amd import _binding as B
    prev = 0
    for images, H, W in ((1, 1, 2), (1, 16, 16), (3, 37, 53), (2, 128, 128), (16, 256, 256), (8, 512, 512), (64, 512, 512)):
        rc, stats, scratch = _ws(lib, _dims(B, images, H, W))
        assert rc == 0 and stats >= B.FGS_PIXEL_STAT_SLOTS * 8 and stats % 256 == 0
        assert scratch > 0 and scratch % 256 == 0 and scratch >= prev  # grows with the batch up to the grid cap
        prev = scratch
    assert _ws(lib, _dims(B, 8, 512, 512))[2] > _ws(lib, _dims(B, 1, 16, 16))[2]
    assert _ws(lib, _dims(B, 64, 512, 512))[2] <= 4 * 2048 * 8  # capped grid: 2048 blocks x 4 sums
    # the size does not depend on which terms are on
    assert _ws(lib, _dims(B, 3, 37, 53, flags=B.FGS_PIXEL_DEPTH)) == _ws(lib, _dims(B, 3, 37, 53))


def test_pixel_loss_invalid_arguments_are_refused_without_a_gpu(lib):
    from fresnel_amd import _binding as B
    ALL = B.FGS_PIXEL_RGB | B.FGS_PIXEL_DENSITY | B.FGS_PIXEL_BOUNDARY | B.FGS_PIXEL_DEPTH
    bad_dims = [dict(images=0), dict(H=0), dict(W=-1), dict(world=0), dict(flags=0), dict(flags=32 | 1),
                dict(flags=B.FGS_PIXEL_DENSITY | B.FGS_PIXEL_DEPTH),           # density weighting without the rgb term
                dict(flags=B.FGS_PIXEL_HARD_MASK),                              # no term at all
                dict(images=1, H=1, W=1),                                       # B H W world < 2
                dict(zones=-1), dict(zones=65),                                 # zero / 66 boundaries
                dict(threshold=0.0), dict(threshold=-0.02), dict(threshold=float("nan")),
                dict(vlm_weight=float("inf")), dict(images=1 << 14, H=1 << 9, W=1 << 9)]
    for bad in bad_dims:
        rc, _, _ = _ws(lib, _dims(B, **bad))
        assert rc == -1, bad
        assert lib.fgs_last_error()
    assert _ws(lib, _dims(B, images=1, H=1, W=1, world=2))[0] == 0            # two ranks of one pixel: N = 2
    assert _ws(lib, _dims(B, zones=64))[0] == 0 and _ws(lib, _dims(B, zones=0))[0] == 0
    assert lib.fgs_pixel_loss_workspace_bytes(None, None, None) == -1
    for k, v in ((3, 0.25), (5, float("nan")), (8, 0.875)):                     # non-increasing / non-finite table
        d = _dims(B)
        d.boundaries[k] = v
        assert _ws(lib, d)[0] == -1, (k, v)
    # a table is only read with the boundary term
    d = _dims(B, flags=B.FGS_PIXEL_RGB | B.FGS_PIXEL_DEPTH, zones=-1, threshold=0.0)
    assert _ws(lib, d)[0] == 0

    # null pointers and flags without their tensor: refused before anything is enqueued (no device is touched)
    p = ctypes.c_void_p(256)  # never dereferenced: every call below fails validation first
    d = ctypes.byref(_dims(B))
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        assert lib.fgs_pixel_loss_stage1(d, *args, p, p, p, None) == -1, args   # rendered, target, depths, density
        assert lib.fgs_pixel_loss_forward(d, *args, p, p, p, None) == -1, args
        assert lib.fgs_pixel_loss_backward(d, *args, p, p, p, p, p, p, None) == -1, args
    for outs in ((None, p, p), (p, None, p), (p, p, None)):                    # out, stats, scratch
        assert lib.fgs_pixel_loss_stage1(d, p, p, p, p, p, *outs, None) == -1
        assert lib.fgs_pixel_loss_forward(d, p, p, p, p, p, *outs, None) == -1
    assert b"null" in lib.fgs_last_error().lower()
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.fgs_pixel_loss_stage2(d, *args, None) == -1
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        assert lib.fgs_pixel_loss_stage3(d, *args, None) == -1
    assert lib.fgs_pixel_loss_backward(d, p, p, p, p, p, None, p, p, p, p, p, None) == -1       # stats
    assert lib.fgs_pixel_loss_backward(d, p, p, p, p, p, p, p, p, p, None, None, None) == -1    # no gradient asked for
    # stages 2 and 3 exist only with the depth term; a gradient needs its term
    nd = ctypes.byref(_dims(B, flags=B.FGS_PIXEL_RGB))
    assert lib.fgs_pixel_loss_stage2(nd, p, p, p, p, None) == -1 and lib.fgs_pixel_loss_stage3(nd, p, p, p, p, p, None) == -1
    assert lib.fgs_pixel_loss_backward(nd, p, p, None, None, None, p, p, None, None, None, p, None) == -1
    dd = ctypes.byref(_dims(B, flags=B.FGS_PIXEL_DEPTH))
    assert lib.fgs_pixel_loss_backward(dd, None, None, p, p, None, p, None, None, p, p, None, None) == -1
    assert ALL == 23


def test_pixel_losses_argument_checks():
    from fresnel_amd import _binding as B
    from fresnel_amd.losses import pixel_losses
    x = torch.rand(2, 3, 16, 16)
    with pytest.raises(B.FgsError, match="no CPU fallback"):
        pixel_losses(x, x)
    with pytest.raises(B.FgsError, match="one shape"):
        pixel_losses(x, torch.rand(2, 3, 16, 15))
    with pytest.raises(B.FgsError, match="one shape"):
        pixel_losses(torch.rand(2, 1, 16, 16), torch.rand(2, 1, 16, 16))
    with pytest.raises(B.FgsError, match="reduce_fn"):
        pixel_losses(x, x, world=2)
    with pytest.raises(B.FgsError, match="zones"):
        pixel_losses(x, x, zones="eight")


# ---- CPU: flags, defaults, the unchanged default loss ---------------------------------------------------------------
def test_training_flags_and_the_unchanged_default_loss():
    from fresnel_amd import train as T
    c = T.TrainingConfig()
    assert (c.use_vlm_guidance, c.vlm_weight, c.boundary_weight, c.pixel_loss_backend) == (False, 0.5, 0.0, "torch")
    a = T.arg_parser().parse_args([])
    assert (a.use_vlm_guidance, a.vlm_weight, a.boundary_weight, a.pixel_loss_backend) == (False, 0.5, 0.0, "torch")
    a = T.arg_parser().parse_args(["--use_vlm_guidance", "--vlm_weight", "0.3", "--boundary_weight", "0.1", "--pixel_loss_backend",
                                   "hip", "--use_fresnel_zones"])
    assert (a.use_vlm_guidance, a.vlm_weight, a.boundary_weight, a.pixel_loss_backend, a.use_fresnel_zones) == (True, 0.3, 0.1, "hip", 8)
    with pytest.raises(SystemExit):
        T.arg_parser().parse_args(["--pixel_loss_backend", "triton"])
    g = torch.Generator().manual_seed(4)
    r, t = torch.rand(2, 3, 32, 32, generator=g), torch.rand(2, 3, 32, 32, generator=g)
    rd, td = torch.rand(2, 32, 32, generator=g), torch.rand(2, 32, 32, generator=g)
    cfg = T.TrainingConfig(image_size=32, ssim_weight=0.0)
    total, d = T.compute_losses(r, t, rd, td, cfg)
    (rm, rs), (tm, ts) = T._global_mean_std(rd, None), T._global_mean_std(td, None)
    want = cfg.rgb_weight * F.l1_loss(r, t) + cfg.depth_weight * F.l1_loss((rd - rm) / torch.clamp(rs, min=1e-4),
                                                                            (td - tm) / torch.clamp(ts, min=1e-4))
    assert set(d) == {"rgb", "depth", "total"} and torch.equal(total, want)
    assert torch.equal(total, d["rgb"] + 0.1 * d["depth"])
    # zones alone (boundary_weight 0, the default) and a density map without the switch change nothing
    same, d2 = T.compute_losses(r, t, rd, td, T.TrainingConfig(image_size=32, ssim_weight=0.0, use_fresnel_zones=True),
                                vlm_density=torch.rand(2, 1, 32, 32, generator=g))
    assert torch.equal(same, total) and set(d2) == set(d)
    # the boundary term needs the zones: boundary_weight alone adds nothing (TGD:943, fresnel_zones is None)
    same, d3 = T.compute_losses(r, t, rd, td, T.TrainingConfig(image_size=32, ssim_weight=0.0, boundary_weight=0.1))
    assert torch.equal(same, total) and set(d3) == set(d)
    tot_b, d4 = T.compute_losses(r, t, rd, td, T.TrainingConfig(image_size=32, ssim_weight=0.0, boundary_weight=0.1, use_fresnel_zones=True))
    assert set(d4) == set(d) | {"boundary"} and float(d4["boundary"]) > 0
    assert abs(float(tot_b) - float(total) - 0.1 * float(d4["boundary"])) <= 1e-6
    # the HIP backend is refused on the CPU with a clear message
    with pytest.raises(ValueError, match="no CPU fallback"):
        T.compute_losses(r, t, rd, td, T.TrainingConfig(image_size=32, pixel_loss_backend="hip"))
    with pytest.raises(ValueError, match="needs a GPU"):
        T.run_training(T.TrainingConfig(image_size=32, pixel_loss_backend="hip", device="cpu"), log=lambda *a: None)
    with pytest.raises(ValueError, match="unknown pixel_loss_backend"):
        T.compute_losses(r, t, rd, td, T.TrainingConfig(image_size=32, pixel_loss_backend="eager"))


def test_synthetic_dataset_density_map():
    from fresnel_amd import train as T
    base = T.SyntheticDataset(4, T.TrainingConfig(image_size=32, feature_size=6, feature_dim=16))
    vlm = T.SyntheticDataset(4, T.TrainingConfig(image_size=32, feature_size=6, feature_dim=16, use_vlm_guidance=True))
    a, b = base.get(2), vlm.get(2)
    assert len(a) == 3 and len(b) == 4 and all(torch.equal(x, y) for x, y in zip(a, b))  # the other tensors are unchanged
    assert b[3].shape == (1, 32, 32) and float(b[3].min()) >= 0.5 and float(b[3].max()) <= 1.5
    assert torch.equal(b[3], vlm.get(2)[3]) and not torch.equal(b[3], vlm.get(3)[3])
    assert [tuple(t.shape) for t in vlm.batch([0, 1], "cpu")] == [(2, 3, 32, 32), (2, 6, 6, 16), (2, 1, 32, 32), (2, 1, 32, 32)]


# ---- CPU: the dataset's density maps ---------------------------------------------------------------------------------
def _image_dir(tmp_path, names, S=24):
    from PIL import Image
    (tmp_path / "features").mkdir()
    rs = np.random.RandomState(0)
    for n in names:
        Image.fromarray(rs.randint(0, 255, (S, S, 3), dtype=np.uint8)).save(tmp_path / f"{n}.png")
    return tmp_path


def test_image_dataset_reads_vlm_density(tmp_path):
    from fresnel_amd.data import ImageDataset
    root = _image_dir(tmp_path, ["a", "b", "c", "d"])
    grid = np.array([[0.0, 1.0], [0.5, 0.25]], np.float64)
    np.save(root / "features" / "a_vlm_density.npy", grid)
    big = np.random.RandomState(1).uniform(0, 1, (7, 7)).astype(np.float32)
    np.save(root / "features" / "b_vlm_density.npy", big)
    np.save(root / "features" / "d_vlm_density.npy", np.zeros((3, 4)))  # not square: unusable, uniform weighting
    S = 9
    ds = ImageDataset(str(root), S, load_vlm_density=True, feature_dim=16)
    it = ds[0]
    assert it["name"] == "a" and it["has_vlm_density"] and it["vlm_density"].shape == (1, S, S) and it["vlm_density"].dtype == torch.float32
    # known answer: corner-aligned bilinear, so the corners are the grid's corners + 0.5 and the centre is its mean + 0.5
    m = it["vlm_density"][0]
    assert torch.allclose(torch.stack([m[0, 0], m[0, -1], m[-1, 0], m[-1, -1]]), torch.tensor([0.5, 1.5, 1.0, 0.75]), atol=1e-6)
    assert abs(float(m[4, 4]) - (0.5 + grid.mean())) <= 1e-6 and abs(float(m[0, 4]) - 1.0) <= 1e-6 and abs(float(m[2, 0]) - 0.625) <= 1e-6
    # missing file / unusable file: ones
    assert not ds[2]["has_vlm_density"] and torch.equal(ds[2]["vlm_density"], torch.ones(1, S, S))
    assert not ds[3]["has_vlm_density"] and torch.equal(ds[3]["vlm_density"], torch.ones(1, S, S))
    # the step's tuples carry the fourth tensor only when enabled
    assert len(ds.host_item(1)) == 4 and torch.equal(ds.host_item(1)[3], ds[1]["vlm_density"])
    b = ds.batch([0, 1, 2], "cpu")
    assert len(b) == 4 and b[3].shape == (3, 1, S, S) and torch.equal(b[3][2], torch.ones(1, S, S))
    plain = ImageDataset(str(root), S, feature_dim=16)
    assert len(plain.host_item(0)) == 3 and len(plain.batch([0, 1], "cpu")) == 3 and "vlm_density" not in plain[0]
    for x, y in zip(plain.host_item(0), ds.host_item(0)):
        assert torch.equal(x, y)


def test_image_dataset_density_equals_scipy_zoom(tmp_path):
    zoom = pytest.importorskip("scipy.ndimage").zoom
    from fresnel_amd.data import ImageDataset
    root = _image_dir(tmp_path, ["a"])
    for n, S in ((7, 32), (16, 64), (14, 37), (5, 5)):
        grid = np.random.RandomState(n).uniform(0, 1, (n, n))
        np.save(root / "features" / "a_vlm_density.npy", grid)
        got = ImageDataset(str(root), S, load_vlm_density=True, feature_dim=16)[0]["vlm_density"][0].numpy()
        want = (0.5 + zoom(grid, S / n, order=1)).astype(np.float32)  # TGD:656-662
        assert got.shape == want.shape and float(np.abs(got - want).max()) <= 1e-6


# ---- GPU -------------------------------------------------------------------------------------------------------------
def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires an MI355X (torch.cuda unavailable)")
    return torch.device("cuda:0")


SHAPES = {"16x3x256x256": (16, 256, 256), "8x3x512x512": (8, 512, 512), "3x3x37x53": (3, 37, 53)}
COMBOS = {  # density, zones, rendered depth, target depth
    "rgb": (False, None, False, False),
    "rgb_density": (True, None, False, False),
    "rgb_boundary": (False, ZONES, False, True),
    "rgb_depth": (False, None, True, True),
    "rgb_density_depth": (True, None, True, True),
    "rgb_boundary_depth": (False, ZONES, True, True),
    "all_soft": (True, ZONES, True, True),
    "all_hard": (True, dict(ZONES, soft=False), True, True),
    "all_5zones_wide": (True, dict(num_zones=5, depth_range=(0.1, 0.9), threshold=0.05, soft=True), True, True),
}


def _check_depth_grad(got, ref, u_minus_v, what):
    """The module docstring's rule for the depth gradient."""
    got, ref = got.double().cpu(), ref.double()
    near = u_minus_v.abs() < 1e-5
    share = float(near.double().mean())
    print(f"{what}: depth-gradient pixels left out {int(near.sum())} of {near.numel()} ({share:.2e})")
    assert share <= 1e-4, (what, share)
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) <= 2.0 * float(ref.abs().max())
    err = float((got - ref)[~near].abs().max()) / float(ref.abs().max())
    print(f"{what}: depth gradient {err:.3e} of max")
    assert err <= 1e-4, (what, err)


def _reference(r, t, rd, td, den, zones, g):
    """fp64 checker: terms and gradients for upstream gradients g (dict), u - v of the depth term."""
    rr = r.double().requires_grad_(True)
    rdd = rd.double().requires_grad_(True) if rd is not None else None
    terms = C.ref_pixel_losses(rr, t.double(), rdd, td.double() if td is not None else None, den, 0.5, zones)
    sum(g[k] * v for k, v in terms.items()).backward()
    umv = None
    if rd is not None:
        umv = C.normalise(rd.double()) - C.normalise(td.double())
    return {k: float(v.detach()) for k, v in terms.items()}, rr.grad, rdd.grad if rdd is not None else None, umv


@pytest.mark.gpu
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_hip_pixel_losses_match_the_checker(shape, combo):
    from fresnel_amd.losses import pixel_losses
    dev = _dev()
    use_den, zones, use_rd, use_td = COMBOS[combo]
    # (seed: the left-out share is a property of the inputs -- it is counted on the fp64 checker alone -- and ONE near tie among
    # the 5 883 pixels of the smallest shape would already be 1.7e-4 of them; this seed's inputs have none there)
    r, t, rd, td, den = _inputs(SHAPES[shape], 30, dtype=torch.float32)
    rd, td, den = rd if use_rd else None, td if use_td else None, den if use_den else None
    g = dict(rgb=0.9, boundary=0.35, depth=0.2)
    want, w_gr, w_gd, umv = _reference(r, t, rd, td, den, zones, g)
    rr = r.to(dev).requires_grad_(True)
    rdd = rd.to(dev).requires_grad_(True) if use_rd else None
    terms = pixel_losses(rr, t.to(dev), rdd, td.to(dev) if use_td else None, den.to(dev) if use_den else None, 0.5, zones)
    assert set(terms) == set(want) and all(v.dim() == 0 for v in terms.values())
    sum(g[k] * v for k, v in terms.items()).backward()
    for k in want:
        err = abs(float(terms[k].detach()) - want[k])
        print(f"{shape} {combo}: {k} {float(terms[k].detach()):.7f} checker {want[k]:.7f} |diff| {err:.2e}")
        assert err <= 1e-5, (k, float(terms[k].detach()), want[k])
    err = rel_to_max(rr.grad.cpu().numpy(), w_gr.numpy())
    print(f"{shape} {combo}: rendered gradient {err:.3e} of max")
    assert err <= 1e-4
    assert float(rr.grad[0, :, :5, :7].abs().max()) == 0.0  # the block of exact ties: exactly zero
    if use_rd:
        _check_depth_grad(rdd.grad, w_gd, umv, f"{shape} {combo}")


# Shapes past the grid cap (2048 blocks x 256 threads = 524 288 work items a trip): every larger shape above is one trip.
#   1x725x725: H W is odd, so the loads are scalar; 525 625 pixels, 1 337 threads take a second trip.
#   1x1448x1452: H W is a multiple of 4, so the loads are 16 bytes; 525 624 groups of 4 pixels, 1 336 threads take a second trip.
# A skipped or doubly counted trip moves a term by ~7e-4 and leaves gradient pixels wrong by the whole maximum.  (Seed 30: 5 of
# 525 625 and 14 of 2 102 496 pixels are near ties on the fp64 checker, 9.5e-6 and 6.7e-6 of them, within the 1e-4 cap.)
SECOND_TRIP_SHAPES = {"1x3x725x725_scalar": (1, 725, 725), "1x3x1448x1452_vector": (1, 1448, 1452)}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SECOND_TRIP_SHAPES))
def test_hip_pixel_losses_second_grid_stride_trip(shape):
    from fresnel_amd.losses import pixel_losses
    dev = _dev()
    Bn, H, W = SECOND_TRIP_SHAPES[shape]
    groups = Bn * H * W // (4 if (H * W) % 4 == 0 else 1)
    assert 2048 * 256 < groups < 2 * 2048 * 256 and 3 * Bn * H * W < 2 ** 31
    use_den, zones, use_rd, use_td = COMBOS["all_soft"]
    r, t, rd, td, den = _inputs((Bn, H, W), 30, dtype=torch.float32)
    g = dict(rgb=0.9, boundary=0.35, depth=0.2)
    want, w_gr, w_gd, umv = _reference(r, t, rd, td, den, zones, g)
    rr, rdd = r.to(dev).requires_grad_(True), rd.to(dev).requires_grad_(True)
    terms = pixel_losses(rr, t.to(dev), rdd, td.to(dev), den.to(dev), 0.5, zones)
    assert set(terms) == set(want) == {"rgb", "boundary", "depth"}
    sum(g[k] * v for k, v in terms.items()).backward()
    for k in want:
        err = abs(float(terms[k].detach()) - want[k])
        print(f"{shape}: {k} {float(terms[k].detach()):.7f} checker {want[k]:.7f} |diff| {err:.2e}")
        assert err <= 1e-5, (k, float(terms[k].detach()), want[k])
    err = rel_to_max(rr.grad.cpu().numpy(), w_gr.numpy())
    print(f"{shape}: rendered gradient {err:.3e} of max")
    assert err <= 1e-4
    assert float(rr.grad[0, :, :5, :7].abs().max()) == 0.0  # the block of exact ties: exactly zero
    _check_depth_grad(rdd.grad, w_gd, umv, shape)


@pytest.mark.gpu
def test_hip_pixel_losses_single_terms_and_unaligned_views():
    """The staged API with the rgb term off (boundary alone, depth alone), and inputs whose pointers are not 16-byte aligned
    (the scalar-load path at a shape whose rows would otherwise take 16-byte loads)."""
    from fresnel_amd import losses as L
    dev = _dev()
    r, t, rd, td, den = _inputs((2, 24, 32), 21, dtype=torch.float32)
    g = dict(rgb=1.0, boundary=1.0, depth=1.0)
    want, w_gr, w_gd, umv = _reference(r, t, rd, td, None, ZONES, g)
    one = torch.ones((), device=dev)
    st = L.pixel_loss_begin(r.to(dev), t.to(dev), None, td.to(dev), zones=ZONES, rgb=False)
    out = L.pixel_loss_forward(st).clone()
    assert float(out[0]) == 0.0 and float(out[2]) == 0.0 and abs(float(out[1]) - want["boundary"]) <= 1e-5
    g_r, g_d = L.pixel_loss_backward(st, None, one, None)
    b_only = _reference(r, t, None, td, None, ZONES, dict(rgb=0.0, boundary=1.0))[1]
    assert g_d is None and rel_to_max(g_r.cpu().numpy(), b_only.numpy()) <= 1e-4
    st = L.pixel_loss_begin(r.to(dev), t.to(dev), rd.to(dev), td.to(dev), rgb=False)
    out = L.pixel_loss_forward(st).clone()
    assert float(out[0]) == 0.0 and float(out[1]) == 0.0 and abs(float(out[2]) - want["depth"]) <= 1e-5
    g_r, g_d = L.pixel_loss_backward(st, None, None, one)
    assert g_r is None
    _check_depth_grad(g_d, w_gd, umv, "depth alone")

    def shifted(x):  # the same values at an address 4 bytes past a 16-byte boundary
        buf = torch.empty(x.numel() + 1, device=dev)
        buf[1:].copy_(x.reshape(-1))
        v = buf[1:].view(x.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    for which in ("rendered", "depth"):
        rr = (shifted(r) if which == "rendered" else r.to(dev)).requires_grad_(True)
        rdd = (shifted(rd) if which == "depth" else rd.to(dev)).requires_grad_(True)
        terms = L.pixel_losses(rr, t.to(dev), rdd, td.to(dev), None, 0.5, ZONES)
        sum(terms.values()).backward()
        for k in want:
            assert abs(float(terms[k].detach()) - want[k]) <= 1e-5
        assert rel_to_max(rr.grad.cpu().numpy(), w_gr.numpy()) <= 1e-4
        _check_depth_grad(rdd.grad, w_gd, umv, f"unaligned {which}")


@pytest.mark.gpu
def test_hip_pixel_losses_repeat_bitwise_and_leave_their_state_intact():
    from fresnel_amd import losses as L
    dev = _dev()
    r, t, rd, td, den = (v.to(dev) for v in _inputs((4, 96, 80), 22, dtype=torch.float32))

    def run():
        rr, rdd = r.clone().requires_grad_(True), rd.clone().requires_grad_(True)
        terms = L.pixel_losses(rr, t, rdd, td, den, 0.5, ZONES)
        (terms["rgb"] + 0.1 * terms["boundary"] + 0.1 * terms["depth"]).backward()
        return [terms[k].detach().clone() for k in ("rgb", "boundary", "depth")] + [rr.grad, rdd.grad]
    a, b = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the backward modifies neither the statistics nor the inputs: a second backward gives the same bits
    st = L.pixel_loss_begin(r, t, rd, td, den, 0.5, ZONES)
    L.pixel_loss_forward(st)
    stats, out = st.stats.clone(), st.out.clone()
    g = [torch.tensor(v, device=dev) for v in (1.0, 0.1, 0.1)]
    g1 = L.pixel_loss_backward(st, *g)
    g2 = L.pixel_loss_backward(st, *g)
    assert torch.equal(stats[:9], st.stats[:9]) and torch.equal(out, st.out)
    assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1]) and torch.equal(g1[0], a[3]) and torch.equal(g1[1], a[4])
    # a retained graph can be differentiated twice
    rr = r.clone().requires_grad_(True)
    loss = L.pixel_losses(rr, t, rd, td)["rgb"]
    loss.backward(retain_graph=True)
    first = rr.grad.clone()
    rr.grad = None
    loss.backward()
    assert torch.equal(first, rr.grad)
    # no_grad: the same values
    with torch.no_grad():
        again = L.pixel_losses(r, t, rd, td, den, 0.5, ZONES)
    assert all(torch.equal(again[k], v) for k, v in zip(("rgb", "boundary", "depth"), a[:3]))


@pytest.mark.gpu
def test_hip_pixel_losses_propagate_nan_and_inf():
    """The step's device-side NaN/Inf skip reads the loss: a non-finite value anywhere in the rendered batch must reach it."""
    from fresnel_amd.losses import pixel_losses
    dev = _dev()
    r, t, rd, td, den = (v.to(dev) for v in _inputs((2, 40, 52), 23, dtype=torch.float32))
    for bad in (float("nan"), float("inf"), float("-inf")):
        for pos in ((0, 0, 0, 0), (1, 2, 39, 51), (1, 1, 17, 30)):
            x = r.clone()
            x[pos] = bad
            terms = pixel_losses(x, t, rd, td, den, 0.5, ZONES)
            assert not math.isfinite(float(terms["rgb"])), (bad, pos)
            assert not math.isfinite(float(terms["boundary"])), (bad, pos)
            assert math.isfinite(float(terms["depth"]))
            assert not math.isfinite(float(pixel_losses(x, t, None, td, None, 0.5, dict(ZONES, soft=False))["boundary"]))
        for pos in ((0, 0, 0), (1, 39, 51), (1, 20, 3)):
            x = rd.clone()
            x[pos] = bad
            terms = pixel_losses(r, t, x, td, den, 0.5, ZONES)
            assert not math.isfinite(float(terms["depth"])), (bad, pos)
            assert math.isfinite(float(terms["rgb"])) and math.isfinite(float(terms["boundary"]))


@pytest.mark.gpu
def test_hip_pixel_losses_two_emulated_ranks():
    """Two "ranks" on one GPU through the staged calls: each holds half the batch (world = 2) and the cross-rank slots are
    summed between the stages, as the data-parallel step's all-reduce does.  The gradients equal the single call's on the
    whole batch; the local terms average to the global ones."""
    from fresnel_amd import losses as L
    dev = _dev()
    r, t, rd, td, den = (v.to(dev) for v in _inputs((4, 64, 72), 24, dtype=torch.float32))
    whole = L.pixel_loss_begin(r, t, rd, td, den, 0.5, ZONES)
    L.pixel_loss_forward(whole)
    g = [torch.tensor(v, device=dev) for v in (0.8, 0.3, 0.6)]
    w_r, w_d = L.pixel_loss_backward(whole, *g)
    halves = [L.pixel_loss_begin(r[h], t[h], rd[h], td[h], den[h], 0.5, ZONES, world=2) for h in (slice(0, 2), slice(2, 4))]
    for stage in (1, 2, 3):
        for s in halves:
            L.pixel_loss_stage(s, stage)
        total = halves[0].cross_rank(stage) + halves[1].cross_rank(stage)
        for s in halves:
            s.cross_rank(stage).copy_(total)
    # the whole batch's loss is the mean of the ranks' losses: each rank's upstream gradient is half the whole's
    parts = [L.pixel_loss_backward(s, *[v / 2 for v in g]) for s in halves]
    h_r, h_d = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    e_r, e_d = rel_to_max(h_r.cpu().numpy(), w_r.cpu().numpy()), rel_to_max(h_d.cpu().numpy(), w_d.cpu().numpy())
    print(f"two ranks vs one call: rendered gradient {e_r:.2e}, depth gradient {e_d:.2e} of max")
    assert e_r <= 1e-6 and e_d <= 1e-6
    mean_out = (halves[0].out.double() + halves[1].out.double()) / 2
    assert float((mean_out - whole.out.double()).abs().max()) <= 1e-6
    # the same through pixel_losses' reduce_fn: a "sum over ranks" of two identical ranks doubles every cross-rank slot,
    # which is the whole batch r ++ r: statistics, terms and gradients of the duplicated batch
    dup = L.pixel_losses(r.clone().requires_grad_(True), t, rd.clone().requires_grad_(True), td, den, 0.5, ZONES,
                         reduce_fn=lambda v: v.mul_(2), world=2)
    both = L.pixel_losses(torch.cat([r, r]), torch.cat([t, t]), torch.cat([rd, rd]), torch.cat([td, td]), torch.cat([den, den]), 0.5, ZONES)
    for k in ("rgb", "boundary", "depth"):
        assert abs(float(dup[k].detach()) - float(both[k])) <= 1e-6, k


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["3x3x37x53", "16x3x256x256"])
def test_compute_losses_backends_agree(shape):
    """pixel_loss_backend "hip" against "torch" on the same device tensors, every term on.  The bounds are the project's
    (1e-5 absolute on terms, 1e-4 of max on gradients: both backends are fp32 formulations of one expression, so this is
    the statement each makes against the fp64 checker).  Measured on the MI355X (this test prints the figures,
    profiles/pixel_loss_gputest.txt): terms agree to <= 1.5e-8 (boundary 3.7e-9, rgb 1.5e-8, depth 0), the rendered gradient
    to 9.6e-8 / 6.6e-8 of max at 3x3x37x53 / 16x3x256x256, the depth gradient to 1.2e-7 / 1.5e-7 of max with 0 of 5 883 /
    13 of 1 048 576 near-tie pixels left out."""
    from fresnel_amd.train import TrainingConfig, compute_losses
    dev = _dev()
    r, t, rd, td, den = _inputs(SHAPES[shape], 25, dtype=torch.float32)
    umv = C.normalise(rd.double()) - C.normalise(td.double())
    res = {}
    for backend in ("torch", "hip"):
        cfg = TrainingConfig(image_size=SHAPES[shape][1], device="cuda:0", ssim_weight=0.0, use_vlm_guidance=True, use_fresnel_zones=True,
                             boundary_weight=0.1, pixel_loss_backend=backend)
        rr, rdd = r.to(dev).requires_grad_(True), rd.to(dev).requires_grad_(True)
        total, terms = compute_losses(rr, t.to(dev), rdd, td.to(dev), cfg, vlm_density=den.to(dev))
        total.backward()
        res[backend] = (terms, rr.grad, rdd.grad)
    (ta, gra, gda), (tb, grb, gdb) = res["torch"], res["hip"]
    assert set(ta) == set(tb) == {"rgb", "depth", "boundary", "total"}
    for k in ta:
        gap = abs(float(ta[k]) - float(tb[k]))
        print(f"{shape}: backends' {k} {float(ta[k]):.7f} / {float(tb[k]):.7f} gap {gap:.2e}")
        assert gap <= 1e-5, k
    gap = rel_to_max(grb.cpu().numpy(), gra.cpu().numpy())
    print(f"{shape}: backends' rendered gradient gap {gap:.2e} of max")
    assert gap <= 1e-4
    _check_depth_grad(gdb, gda.cpu(), umv, f"{shape} backends")


@pytest.mark.gpu
def test_training_step_with_hip_pixel_losses():
    """--pixel_loss_backend hip --use_vlm_guidance --use_fresnel_zones --boundary_weight 0.1: the eager step and the replayed
    graph stay free of host synchronisation, and a few epochs on synthetic data reduce the loss with the boundary term in
    the history."""
    import tempfile
    from fresnel_amd.dist import DPContext
    from fresnel_amd.train import (GraphedTrainStep, PatchGaussianDecoder, StepResult, SyntheticDataset, TrainingConfig,
                                   default_renderer_factory, make_optimizer, run_training, train_step)
    dev = _dev()
    kw = dict(lr=2e-3, image_size=64, feature_size=6, feature_dim=16, gaussians_per_patch=4, device="cuda:0", batch_size=2,
              pixel_loss_backend="hip", use_vlm_guidance=True, use_fresnel_zones=True, boundary_weight=0.1)
    cfg = TrainingConfig(epochs=1, hip_graph=True, **kw)
    torch.manual_seed(0)
    model = PatchGaussianDecoder(cfg.feature_dim, cfg.gaussians_per_patch, grid=cfg.feature_size, use_fresnel_zones=True,
                                 num_fresnel_zones=cfg.num_fresnel_zones).to(dev)
    renderer, camera = default_renderer_factory(cfg, dev)
    opt = make_optimizer(model, cfg)
    dp = DPContext(device=dev)
    data = SyntheticDataset(8, cfg)
    rng = np.random.RandomState(0)
    batches = [data.batch([2 * i, 2 * i + 1], dev) for i in range(3)]
    assert len(batches[0]) == 4
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
    assert ld is not None and {"rgb", "depth", "boundary", "total"} <= set(ld) and all(math.isfinite(v) for v in ld.values())
    assert ld["boundary"] > 0 and any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
    # the captured step: replays without a host synchronisation
    graphed = GraphedTrainStep(model, renderer, camera, opt, cfg, dp, batches[0])
    torch.cuda.synchronize()
    before = [p.detach().clone() for p in model.parameters()]
    torch.cuda.set_sync_debug_mode("error")
    try:
        assert graphed.matches(batches[2])
        res = graphed(batches[2])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ld = res.to_host()
    assert ld is not None and ld["boundary"] > 0 and any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
    # a poisoned batch is skipped on the device: the fused terms carry the NaN to the skip flag
    before = [p.detach().clone() for p in model.parameters()]
    bad = (batches[2][0] * float("nan"),) + tuple(batches[2][1:])
    assert train_step(model, renderer, camera, bad, opt, cfg, dp, pose_rng=rng).to_host() is None
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))

    with tempfile.TemporaryDirectory() as tmp:
        c = TrainingConfig(epochs=3, steps_per_epoch=4, save_interval=100, output_dir=tmp, log_interval=1000, hip_graph=True, **kw)
        _, hist = run_training(c, log=lambda *a: None)
        # the torch backend with the same terms, captured too (its zone table must not be uploaded inside the capture)
        c = TrainingConfig(epochs=3, steps_per_epoch=4, save_interval=100, output_dir=tmp + "/t", log_interval=1000, hip_graph=True,
                           **dict(kw, pixel_loss_backend="torch"))
        _, hist_t = run_training(c, log=lambda *a: None)
    assert len(hist) == 3 and all({"rgb", "depth", "boundary", "total"} <= set(h) for h in hist)
    print("hip pixel-loss training, total per epoch:", [round(h["total"], 5) for h in hist])
    print("torch pixel-loss training, total per epoch:", [round(h["total"], 5) for h in hist_t])
    assert hist[-1]["total"] < hist[0]["total"]
    # the two backends train alike: the bound the repository uses for the eager against the captured step, whose
    # difference -- fp32 rounding of the same expressions -- is of the same kind
    for a, b in zip(hist_t, hist):
        assert set(a) == set(b)
        for k in a:
            assert abs(a[k] - b[k]) <= 1e-4 * max(1.0, abs(a[k])), (k, a[k], b[k])
