"""The blend kernels fold the opacity into the exponent of the Gaussian: alpha / 0.99 = clamp01(exp2(m' + log2(opacity / 0.99)))
(k_blend_fwd_parts, k_composite_fwd, k_composite_bwd, fgs_composite.hip), the backward accumulates dL/dalpha . alpha where it had
dL/dalpha . G, and k_row_sum (fgs_project.hip) takes the opacity out of the sum-dG row again.  What can go wrong depends on the
OPACITY: exactly 0 (log2 = -inf; dL/dopacity is not zero), opacities below and at the floor of the fold (0.99 x 2^-64,
fgs_opacity_floored in fgs_internal.h: the backward folds the exact power of two there and k_row_sum divides it out), tiny ones
(0.99 x 2^-17 ... 2^-15), the clamp threshold 0.98 of the backward's fast class, opacities at and above 0.99 where the clamp of the
exponential binds, and a negative one.  Such Gaussians are placed by hand; the ones whose alpha is (next to) zero lie frontmost and
cover the frame, so that their dL/dopacity is among the largest of the scene and the 1e-4-of-max statement sees it (asserted on
the oracle's output).  Needles and edge-on discs put degenerate conics through the same code, a crowded scene with 64-entry depth
segments the checkpoint restart and the re-base, and the kernels must stay deterministic.

Statement: image, depth and all five input gradients within 1e-4 of max of the C oracle, the fp64 referee judging where
helpers.referee selects it, on 16 x 16 and on 32 x 16 tiles."""
import functools

import numpy as np
import pytest
import torch

from helpers import assert_with_referee, synth_aniso

pytestmark = pytest.mark.gpu

GRADS = ["positions", "scales", "rotations", "colors", "opacities"]
BG = (0.05, 0.1, 0.15)
FW, FH, FOCAL, ZMEAN = 64, 32, 51.2, -2.0  # 2 x 2 tiles of 32 x 16, 4 x 2 of 16 x 16
ALPHA_MAX = np.float32(0.99)
# TINY: alpha zero or next to zero -- frontmost and covering the frame; BOUNDARY: a few pixels across, behind
TINY = [0.0, 1e-30, float(ALPHA_MAX * np.float32(2.0 ** -65)), float(ALPHA_MAX * np.float32(2.0 ** -17))]
BOUNDARY = [float(ALPHA_MAX * np.float32(2.0 ** -64)), float(ALPHA_MAX * np.float32(2.0 ** -63)),  # the floor of the fold
            float(ALPHA_MAX * np.float32(2.0 ** -16)), float(ALPHA_MAX * np.float32(2.0 ** -15)),
            0.3, 0.98, float(np.nextafter(np.float32(0.98), np.float32(1.0))), 0.99, 1.0, 1.3, -0.1]
N_FILL = 12  # further Gaussians behind the frontmost ones, opacities in (0.2, 0.9)


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _place(u, v, z, r, axes):
    """position and scale of a Gaussian whose projected mean is (u, v) and whose bbox radius is ~r pixels"""
    pos = ((u - FW / 2) * -z / FOCAL, -(v - FH / 2) * -z / FOCAL, z)
    return pos, r / 3.0 * -z / FOCAL * np.asarray(axes)


def _boundary_scene():
    rs = np.random.RandomState(7100)
    opac = TINY + BOUNDARY + list(rs.uniform(0.2, 0.9, N_FILL))
    N = len(opac)
    pos, scale = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32)
    for i in range(N):
        if i < len(TINY):  # frontmost, covering the frame (radius well beyond its diagonal), slightly different from one another
            pos[i], scale[i] = _place(30.0 + 1.5 * i, 15.0 + 0.7 * i, -1.0 - 0.02 * i, 90.0 + 5.0 * i, (1.0, 0.8, 0.9))
        else:      # a few pixels across, spread over the frame, behind
            u, v = rs.uniform(4.0, FW - 4.0), rs.uniform(4.0, FH - 4.0)
            pos[i], scale[i] = _place(u, v, ZMEAN - 0.03 * i, rs.uniform(5.0, 12.0), np.array([1.0, 0.5, 0.75])[rs.permutation(3)])
    quat = rs.standard_normal((N, 4)).astype(np.float32)
    color = (0.1 + 0.4 * rs.random_sample((N, 3))).astype(np.float32)
    # bright in front of a dim scene; with zero-mean upstream gradients dL/dopacity of a frame-covering Gaussian (a sum over 2048
    # pixels) comes out about twice that of the largest Gaussian a few pixels across: the 1e-4-of-max statement sees both kinds
    color[:len(TINY)] = 0.95
    gI = rs.standard_normal((3, FH, FW)).astype(np.float32)
    gD = (rs.standard_normal((FH, FW)) * 0.1).astype(np.float32) + 0.05
    return [pos, scale, quat, color, np.asarray(opac, np.float32)], gI, gD


def _oracle_pair(arrs, W, H, fx, cx, cy, gI, gD):
    """(fp32 oracle forward, fp32 gradients, fp64 forward, fp64 gradients) of one image."""
    from oracle import fgs_oracle as orc
    ocam = orc.make_camera(np.eye(4, dtype=np.float32), fx, fx, cx, cy, W, H)
    r32 = orc.render(*arrs, ocam, bg=BG)
    g32 = orc.render_backward(r32, gI, gD)
    with orc.fp64():
        r64 = orc.render(*arrs, ocam, bg=BG)
        g64 = orc.render_backward(r64, gI, gD)
    return r32, g32, r64, g64


@functools.lru_cache(maxsize=None)
def _boundary_reference():
    arrs, gI, gD = _boundary_scene()
    return (arrs, gI, gD) + _oracle_pair(arrs, FW, FH, FOCAL, FW / 2, FH / 2, gI, gD)


def _hip(arrs, W, H, fx, cx, cy, gI, gD, tuning):
    """image, depth and the gradients of all five inputs through the renderer; arrays are (N, .) or (B, N, .)."""
    from fresnel_amd.renderer import Camera, TileBasedRenderer
    dev = _cuda()
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True) for a in arrs]
    ren = TileBasedRenderer(W, H, background=BG)
    ren.tuning = dict(tuning)
    img, dep = ren(*ts, Camera(fx, fx, cx, cy, W, H), return_depth=True)
    ((img * torch.from_numpy(gI).to(dev)).sum() + (dep * torch.from_numpy(gD).to(dev)).sum()).backward()
    out = {k: t.grad.detach().cpu().numpy() for k, t in zip(GRADS, ts)}
    out["image"], out["depth"] = img.detach().cpu().numpy(), dep.detach().cpu().numpy()
    return out


def _assert_all(got, r32, g32, r64, g64, what):
    assert_with_referee(got["image"], r32.image, r64.image, f"{what} image")
    assert_with_referee(got["depth"], r32.depth, r64.depth, f"{what} depth")
    for k in GRADS:
        assert_with_referee(got[k], g32[k], g64[k], f"{what} grad_{k}")


def _max_g_op(r, i):
    """largest G x opacity over the integer pixels of Gaussian i's bbox, from the oracle's projected mean and conic"""
    x0, x1, y0, y1 = [int(v) for v in r.proj["bbox"][i]]
    u, v = [float(t) for t in r.proj["mean2d"][i]]
    ca, cbc, cd = [float(t) for t in r.proj["conic"][i]]
    dx, dy = np.meshgrid(np.arange(x0, x1) - u, np.arange(y0, y1) - v)
    return float(np.exp(-0.5 * (ca * dx * dx + cbc * dx * dy + cd * dy * dy)).max() * float(r.opacity[i]))


@pytest.mark.parametrize("tile_w", [16, 32])
def test_class_boundaries_vs_oracle(tile_w):
    arrs, gI, gD, r32, g32, r64, g64 = _boundary_reference()
    opac = arrs[4]
    n_front = len(TINY)
    assert r32.proj["visible"].all() and len(opac) - n_front >= 20
    # the (next to) transparent Gaussians are frontmost and cover the frame ...
    assert list(r32.vis_sorted[:n_front]) == list(range(n_front)), r32.vis_sorted[:n_front]
    for i in range(n_front):
        x0, x1, y0, y1 = [int(v) for v in r32.proj["bbox"][i]]
        assert x0 <= 0 and y0 <= 0 and x1 >= FW and y1 >= FH, (i, r32.proj["bbox"][i])
    # ... so that the oracle's dL/dopacity of each is among the largest of the scene: the 1e-4-of-max statement sees it
    gmax = float(np.abs(g32["opacities"]).max())
    for i in range(n_front):
        assert abs(float(g32["opacities"][i])) >= 0.1 * gmax, (i, float(g32["opacities"][i]), gmax)
    assert float(np.abs(g32["opacities"][n_front:]).max()) >= 0.1 * gmax  # ... and does not lose sight of the others
    # both sides of the fold's floor and of the backward's fast-class threshold are in the scene
    floor = float(ALPHA_MAX * np.float32(2.0 ** -64))
    assert (opac[opac >= 0] < floor).sum() >= 3 and (opac == np.float32(floor)).sum() == 1 and (opac == np.float32(0.98)).sum() == 1
    # the clamp binds for the opacities 1.0 and 1.3
    for op in (1.0, 1.3):
        (i,) = np.nonzero(opac == np.float32(op))[0]
        assert _max_g_op(r32, i) > 0.99, (op, _max_g_op(r32, i))
    got = _hip(arrs, FW, FH, FOCAL, FW / 2, FH / 2, gI, gD, dict(tile_w=tile_w))
    _assert_all(got, r32, g32, r64, g64, f"boundaries tile_w={tile_w}")
    (neg,) = np.nonzero(opac < 0)[0]
    for k in GRADS:  # alpha clamps to 0 with zero gradient
        assert not np.any(got[k][neg]), (k, got[k][neg])
        assert not np.any(g32[k][neg]), k


# ---- degenerate conics: needles (s, s/r, s/r) and edge-on discs (s, s, s/r), the recipe of the G14 fixtures ----
NW, NH, NN = 48, 24, 48


def _needle_scene(ratio):
    rs = np.random.RandomState(7200 + ratio)
    pos = (rs.standard_normal((NN, 3)) * 0.4).astype(np.float32)
    pos[:, 2] -= 2
    smax = 0.1 + 0.3 * rs.random_sample(NN)
    scale = np.stack([smax, smax / ratio, smax / ratio], 1)
    scale[NN // 2:, 1] = smax[NN // 2:]  # second half: discs
    scale = np.stack([s[rs.permutation(3)] for s in scale]).astype(np.float32)  # the thin axis is not always the same one
    quat = rs.standard_normal((NN, 4)).astype(np.float32)
    color = rs.random_sample((NN, 3)).astype(np.float32)
    opacity = (0.2 + 0.8 * rs.random_sample(NN)).astype(np.float32)
    # every kind of opacity among the needles AND among the discs
    special = [0.0, 1e-30, float(ALPHA_MAX * np.float32(2.0 ** -17)), 1e-3, 0.985, 1.0, 1.3]
    for half in (0, NN // 2):
        opacity[half:half + len(special)] = special
    gI = rs.standard_normal((3, NH, NW)).astype(np.float32)
    gD = (rs.standard_normal((NH, NW)) * 0.1).astype(np.float32)
    return [pos, scale, quat, color, opacity], gI, gD


NEEDLE_CAM = (0.8 * NW, NW / 2, NH / 2)


@functools.lru_cache(maxsize=None)
def _needle_reference(ratio):
    arrs, gI, gD = _needle_scene(ratio)
    return (arrs, gI, gD) + _oracle_pair(arrs, NW, NH, *NEEDLE_CAM, gI, gD)


@pytest.mark.parametrize("tile_w", [16, 32])
@pytest.mark.parametrize("ratio", [30, 100])
def test_needles_and_discs_vs_oracle(ratio, tile_w):
    arrs, gI, gD, r32, g32, r64, g64 = _needle_reference(ratio)
    vis = r32.proj["visible"].astype(bool)
    assert vis[:NN // 2].sum() >= 12 and vis[NN // 2:].sum() >= 12, vis  # needles and discs on the frame
    got = _hip(arrs, NW, NH, *NEEDLE_CAM, gI, gD, dict(tile_w=tile_w))
    _assert_all(got, r32, g32, r64, g64, f"needles ratio={ratio} tile_w={tile_w}")


# ---- crowded: 300 anisotropic Gaussians on a frame that is no multiple of the tile, depth segments of 64 entries ----
CW, CH, CN, SEG = 48, 24, 300, 64
CROWD_SMAX = (0.02, 0.2)
CROWD_CAM = (0.9 * CW, CW / 2 + 1.3, CH / 2 - 0.7)  # focal length, cx, cy


def _crowd_scene(smax):
    seed = 7300 + int(round(smax * 100))
    rs = np.random.RandomState(seed + 1)
    arrs = list(synth_aniso(CN, seed, opacity_max=1.0, smax=smax))
    # opacities across every class: a third of the Gaussians log-uniform in [1e-30, 1e-3] or exactly 0, some above 0.98 and above 1
    k = rs.permutation(CN)
    arrs[4][k[:80]] = (10.0 ** rs.uniform(-30.0, -3.0, 80)).astype(np.float32)
    arrs[4][k[80:100]] = 0.0
    arrs[4][k[100:120]] = rs.uniform(0.98, 1.3, 20).astype(np.float32)
    gI = rs.standard_normal((3, CH, CW)).astype(np.float32)
    gD = (rs.standard_normal((CH, CW)) * 0.1).astype(np.float32)
    return arrs, gI, gD


@functools.lru_cache(maxsize=None)
def _crowd_reference(smax):
    arrs, gI, gD = _crowd_scene(smax)
    return (arrs, gI, gD) + _oracle_pair(arrs, CW, CH, *CROWD_CAM, gI, gD)


@functools.lru_cache(maxsize=None)
def _crowd_hip(smax, tile_w):
    arrs, gI, gD = _crowd_scene(smax)
    return _hip(arrs, CW, CH, *CROWD_CAM, gI, gD, dict(tile_w=tile_w, seg_len=SEG))


@pytest.mark.parametrize("tile_w", [16, 32])
@pytest.mark.parametrize("smax", CROWD_SMAX)
def test_crowded_short_segments_vs_oracle(smax, tile_w):
    from oracle import fgs_oracle as orc
    arrs, gI, gD, r32, g32, r64, g64 = _crowd_reference(smax)
    ranges, _ = orc.tile_lists(r32.vis_sorted, r32.proj["bbox"], CW, CH, tile_w=tile_w)
    longest = int(np.diff(ranges).max())
    assert longest > (2 * SEG if smax > 0.1 else SEG), longest  # several depth segments (smax 0.2: at least three) in a tile
    floor = float(ALPHA_MAX * np.float32(2.0 ** -64))
    op = arrs[4][r32.proj["visible"].astype(bool)]
    assert (op == 0).sum() >= 5 and ((op > 0) & (op < floor)).sum() >= 5 and ((op >= floor) & (op < 1e-3)).sum() >= 5 and (op > 0.98).sum() >= 5
    _assert_all(_crowd_hip(smax, tile_w), r32, g32, r64, g64, f"crowded smax={smax} tile_w={tile_w}")


@pytest.mark.parametrize("tile_w", [16, 32])
def test_crowded_is_deterministic_and_batch_equals_single_images(tile_w):
    scenes = [_crowd_scene(s) for s in CROWD_SMAX]
    single = [_crowd_hip(s, tile_w) for s in CROWD_SMAX]
    keys = GRADS + ["image", "depth"]
    for (arrs, gI, gD), first in zip(scenes, single):
        again = _hip(arrs, CW, CH, *CROWD_CAM, gI, gD, dict(tile_w=tile_w, seg_len=SEG))
        for k in keys:
            assert np.array_equal(first[k], again[k]), k
    batch = _hip([np.stack([sc[0][i] for sc in scenes]) for i in range(5)], CW, CH, *CROWD_CAM,
                 np.stack([sc[1] for sc in scenes]), np.stack([sc[2] for sc in scenes]), dict(tile_w=tile_w, seg_len=SEG))
    for b in range(2):
        for k in keys:
            assert np.array_equal(batch[k][b], single[b][k]), (b, k)
