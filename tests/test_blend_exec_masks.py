"""Bbox membership in the blend kernels (k_blend_fwd_parts, k_composite_bwd, fgs_composite.hip): a lane of an 8 x 8 sub-tile pass
contributes iff its pixel lies inside the Gaussian's bbox, decided from the column / row bits that the staging leaves per list
entry (stage_decode_w, fgs_wave.h).  The scenes were written for a form of the kernels that applies membership as the EXEC mask
of the pass, built on the scalar unit; that form was measured slower than the per-lane masks on both tile shapes and is not in
the tree (DESIGN_LOG.md 17) -- the scenes check the per-lane masks just as well, and stay for whoever changes how membership is
decided.  What can go wrong is MEMBERSHIP, so the Gaussians are placed by hand: bbox edges on every residue mod 8, in both halves
of a 32-wide tile and in both sub-tile rows; bboxes of a single pixel, a single column and a single row at the corners of
sub-tiles; bboxes that cover the frame and bboxes inside one 16 x 16 half of a 32 x 16 tile; bboxes cut by the frame; and a crowded
frame with 64-entry depth segments (checkpoint restart and re-base).
(No scene with a non-finite upstream gradient outside a bbox: with per-lane masks the lanes outside the bbox execute and add
a' = 0 times their terms, so an Inf there becomes a NaN in the Gaussian's row -- as before; only passes under an EXEC mask would
leave it out.)

A bbox is the square [trunc(u - r), trunc(u + r) + 1) x [trunc(v - r), trunc(v + r) + 1) clipped to the frame, r = 3 sqrt(largest
eigenvalue of the projected covariance): the Gaussians here are flat (third axis 1e-3 of the others) and turned about the viewing
axis only, so that r is 3 x the larger in-plane scale in pixels whatever the position, and a bbox can be put where it is wanted.
Every placement is asserted on the CPU from the oracle's bboxes before anything runs on the GPU.

Statement: image, depth and all five input gradients within 1e-4 of max of the C oracle, the fp64 referee judging where
helpers.referee selects it, on 64 x 32 and 40 x 24 frames (the second with partial tiles at the right and bottom edge), on 16 x 16
and on 32 x 16 tiles; every scene bitwise reproducible."""
import functools

import numpy as np
import pytest
import torch

from helpers import assert_with_referee

pytestmark = pytest.mark.gpu

GRADS = ["positions", "scales", "rotations", "colors", "opacities"]
BG = (0.05, 0.1, 0.15)
FOCAL = 51.2
FRAMES = [(64, 32), (40, 24)]
TILE_WS = [16, 32]
SEG = 64
RESIDUE_SEED = 0  # (chosen so that check_residues holds on both frames)


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _build(W, H, items, seed, round_ones=False):
    """items: (u, v, r) -- projected mean and bbox radius in pixels.  Flat Gaussians (in-plane axes r / 3 and 0.6 r / 3 pixels),
    turned about the viewing axis, at distinct depths (item 0 frontmost), opacity in [0.3, 0.9].  round_ones: both in-plane axes r / 3."""
    rs = np.random.RandomState(seed)
    N = len(items)
    pos, scale, quat = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32), np.zeros((N, 4), np.float32)
    for i, (u, v, r) in enumerate(items):
        z = -2.0 - 0.004 * i
        s = r / 3.0 * -z / FOCAL
        pos[i] = ((u - W / 2) * -z / FOCAL, -(v - H / 2) * -z / FOCAL, z)
        scale[i] = (s, 0.6 * s, 1e-3 * s) if i % 2 else (0.6 * s, s, 1e-3 * s)
        if round_ones:
            scale[i, :2] = s
        th = rs.uniform(0.0, np.pi)
        quat[i] = (np.cos(th / 2), 0.0, 0.0, np.sin(th / 2))
    color = (0.2 + 0.7 * rs.random_sample((N, 3))).astype(np.float32)
    opacity = rs.uniform(0.3, 0.9, N).astype(np.float32)
    gI = rs.standard_normal((3, H, W)).astype(np.float32)
    gD = (rs.standard_normal((H, W)) * 0.1).astype(np.float32) + 0.05
    return [pos, scale, quat, color, opacity], gI, gD


# ---- the scenes: lists of (u, v, r) ----
def _items_residues(W, H):
    """48 small Gaussians, means stepped by a non-integer stride along both axes (the rows in another order), radii 1 ... 6"""
    rs = np.random.RandomState(RESIDUE_SEED)
    rows, radii = rs.permutation(48), rs.uniform(1.0, 6.0, 48)
    return [(1.5 + (W - 3.0) * (i + 0.37) / 48.0, 1.5 + (H - 3.0) * (rows[i] + 0.61) / 48.0, radii[i]) for i in range(48)]


def _lane_pixels(W, H):
    """pixels at sub-tile corners (lanes 0, 7, 56, 63) in different sub-tiles, at the frame's far corner, and interior ones"""
    return [(0, 0), (8, 8), (23, 0), (16, 15), (31, 15), (7, 7), (24, 8), (W - 1, H - 1), (W - 1, 0), (0, H - 1),
            (11, 5), (28, 12), (W - 5, H - 3), (19, 18)]


def _items_lanes(W, H):
    # 1 x 1: the mean just inside a pixel's cell, r = 0.0035 (the 1e-4 regularisation of the covariance keeps G ~ 0.85 there)
    items = [(px + 0.004, py + 0.004, 0.0035) for px, py in _lane_pixels(W, H)]
    r = 3.4  # 2 r + 1 ~ 8 pixels; the frame cuts the other axis down to one
    items += [(-r + 0.5, 12.3, r), (W - 0.9 + r, 3.7, r),     # 1 x 8: column 0, rows 8 ... 15; column W - 1, rows 0 ... 7
              (12.3, -r + 0.5, r), (19.7, H - 0.9 + r, r)]    # 8 x 1: row 0, columns 8 ... 15; row H - 1, columns 16 ... 23
    return items


def _items_covers(W, H):
    items = [(W / 2 + 1.3, H / 2 - 0.7, 60.0), (W / 2 - 3.1, H / 2 + 2.2, 55.0), (W / 2, H / 2, 63.0)]  # the whole frame
    # inside one 16 x 16 half of a 32 x 16 tile (and inside one 16 x 16 tile): the other half-wave must skip them
    if (W, H) == (64, 32):
        cells = [(cx, cy, r) for cy in (8, 24) for cx in (8, 24, 40, 56) for r in (3.0, 5.5)]
    else:  # 40 x 24: the cells at the right and at the bottom edge are 8 pixels wide / high
        cells = [(cx, 8, r) for cx in (8, 24) for r in (3.0, 5.5)] + [(36, 8, 3.2), (8, 20, 3.2), (24, 20, 3.2), (36, 20, 3.2)]
    return items + [(cx + 0.1 * (k % 3) - 0.2, cy - 0.1 * (k % 4) + 0.3, r) for k, (cx, cy, r) in enumerate(cells)]


def _items_offframe(W, H):
    return [(-2.2, 10.3, 5.0), (W + 1.4, 14.6, 6.0), (20.3, -3.1, 5.0), (30.7, H + 2.2, 6.0), (-1.2, -1.4, 4.0), (W + 1.1, H + 0.8, 5.0),
            (-0.6, H + 0.7, 3.0), (W + 0.3, -0.9, 4.5), (1.2, 1.7, 6.0), (W - 1.8, H - 2.1, 6.0), (W / 2, 0.4, 2.5), (W / 2 + 7, H - 0.6, 3.5),
            (0.3, H / 2, 2.0), (W - 0.7, H / 2 + 3, 4.0), (W / 2, H / 2, 3.0)]


def _items_restart(W, H):
    rs = np.random.RandomState(8405)
    return [(rs.uniform(0.0, W), rs.uniform(0.0, H), rs.uniform(2.0, 6.0)) for _ in range(300)]


SCENES = {"residues": (_items_residues, {}), "lanes": (_items_lanes, {}), "covers": (_items_covers, {}),
          "offframe": (_items_offframe, {}), "restart": (_items_restart, dict(seg_len=SEG))}


@functools.lru_cache(maxsize=None)
def _scene(name, W, H):
    return _build(W, H, SCENES[name][0](W, H), 8400 + sorted(SCENES).index(name) + W, round_ones=name == "lanes")


def _oracle_pair(arrs, W, H, gI, gD):
    from oracle import fgs_oracle as orc
    ocam = orc.make_camera(np.eye(4, dtype=np.float32), FOCAL, FOCAL, W / 2, H / 2, W, H)
    r32 = orc.render(*arrs, ocam, bg=BG)
    g32 = orc.render_backward(r32, gI, gD)
    with orc.fp64():
        r64 = orc.render(*arrs, ocam, bg=BG)
        g64 = orc.render_backward(r64, gI, gD)
    return r32, g32, r64, g64


@functools.lru_cache(maxsize=None)
def _reference(name, W, H):
    arrs, gI, gD = _scene(name, W, H)
    return _oracle_pair(arrs, W, H, gI, gD)


def _hip(arrs, W, H, gI, gD, tuning):
    from fresnel_amd.renderer import Camera, TileBasedRenderer
    dev = _cuda()
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True) for a in arrs]
    ren = TileBasedRenderer(W, H, background=BG)
    ren.tuning = dict(tuning)
    img, dep = ren(*ts, Camera(FOCAL, FOCAL, W / 2, H / 2, W, H), return_depth=True)
    ((img * torch.from_numpy(gI).to(dev)).sum() + (dep * torch.from_numpy(gD).to(dev)).sum()).backward()
    out = {k: t.grad.detach().cpu().numpy() for k, t in zip(GRADS, ts)}
    out["image"], out["depth"] = img.detach().cpu().numpy(), dep.detach().cpu().numpy()
    return out


@functools.lru_cache(maxsize=None)
def _hip_scene(name, W, H, tile_w):
    arrs, gI, gD = _scene(name, W, H)
    return _hip(arrs, W, H, gI, gD, dict(tile_w=tile_w, **SCENES[name][1]))


def _bboxes(name, W, H):
    r32 = _reference(name, W, H)[0]
    assert r32.proj["visible"].all(), (name, W, H, np.nonzero(~r32.proj["visible"].astype(bool))[0])
    return np.asarray(r32.proj["bbox"], np.int64)  # x0, x1, y0, y1 per Gaussian


# ---- what each scene is there for, asserted on the CPU from the oracle's bboxes ----
def check_residues(W, H):
    bb = _bboxes("residues", W, H)
    assert len(bb) == 48 and ((bb[:, 1] - bb[:, 0]) <= 14).all() and ((bb[:, 1] - bb[:, 0]) >= 2).all()
    for k, what in enumerate(("x0", "x1", "y0", "y1")):
        assert set(bb[:, k] % 8) == set(range(8)), (what, sorted(set(bb[:, k] % 8)))  # every column / row mask value ...
    for k in (0, 1):  # ... in both 16-pixel halves of a 32-wide tile (x1 is one past the last column)
        assert {int(h) for h in (bb[:, k] - k) % 32 // 16} == {0, 1}, k
    for k in (2, 3):  # ... and in both sub-tile rows
        assert {int(h) for h in (bb[:, k] - (k - 2)) % 16 // 8} == {0, 1}, k


def check_lanes(W, H):
    bb = _bboxes("lanes", W, H)
    px = _lane_pixels(W, H)
    for i, (x, y) in enumerate(px):
        assert tuple(bb[i]) == (x, x + 1, y, y + 1), (i, bb[i])
    lanes = {8 * (y % 8) + x % 8 for x, y in px}
    assert {0, 7, 56, 63} <= lanes and any(l % 8 not in (0, 7) and l // 8 not in (0, 7) for l in lanes)
    n = len(px)
    assert tuple(bb[n]) == (0, 1, 8, 16) and tuple(bb[n + 1]) == (W - 1, W, 0, 8), bb[n:n + 2]    # 1 x 8
    assert tuple(bb[n + 2]) == (8, 16, 0, 1) and tuple(bb[n + 3]) == (16, 24, H - 1, H), bb[n + 2:]  # 8 x 1
    # every one of them puts something on the frame that the 1e-4-of-max statement on the image sees
    r32 = _reference("lanes", W, H)[0]
    op = _scene("lanes", W, H)[0][4]
    for i in range(len(bb)):
        x0, x1, y0, y1 = bb[i]
        u, v = [float(t) for t in r32.proj["mean2d"][i]]
        ca, cbc, cd = [float(t) for t in r32.proj["conic"][i]]
        dx, dy = np.meshgrid(np.arange(x0, x1) - u, np.arange(y0, y1) - v)
        assert float(np.exp(-0.5 * (ca * dx * dx + cbc * dx * dy + cd * dy * dy)).max()) * float(op[i]) > 2e-3, i


def check_covers(W, H):
    bb = _bboxes("covers", W, H)
    assert (bb[:3] == (0, W, 0, H)).all(), bb[:3]  # the full-mask path: all 64 lanes of every sub-tile
    inner = bb[3:]
    assert len(inner) >= 8
    # inside one 16 x 16 cell: one half of a 32 x 16 tile
    assert (inner[:, 0] // 16 == (inner[:, 1] - 1) // 16).all() and (inner[:, 2] // 16 == (inner[:, 3] - 1) // 16).all(), inner
    assert {int(h) for h in inner[:, 0] % 32 // 16} == {0, 1}  # left halves and right halves


def check_offframe(W, H):
    bb = _bboxes("offframe", W, H)
    for k, edge in enumerate((0, W, 0, H)):  # bboxes cut by the frame on each side
        assert (bb[:, k] == edge).sum() >= 3, (k, bb[:, k])
    assert ((bb[:, 1] > bb[:, 0]) & (bb[:, 3] > bb[:, 2])).all()


def check_restart(W, H, tile_w):
    from oracle import fgs_oracle as orc
    r32 = _reference("restart", W, H)[0]
    ranges, _ = orc.tile_lists(r32.vis_sorted, r32.proj["bbox"], W, H, tile_w=tile_w)
    longest = int(np.diff(ranges).max())
    assert longest > SEG, longest  # a checkpoint restart in at least one tile ...
    if (W, H) == (40, 24):
        assert longest > 2 * SEG, longest  # ... and on the small frame three segments or more
    return longest


CHECKS = {"residues": check_residues, "lanes": check_lanes, "covers": check_covers, "offframe": check_offframe}


def _assert_all(got, ref, what):
    r32, g32, r64, g64 = ref
    assert_with_referee(got["image"], r32.image, r64.image, f"{what} image")
    assert_with_referee(got["depth"], r32.depth, r64.depth, f"{what} depth")
    for k in GRADS:
        assert_with_referee(got[k], g32[k], g64[k], f"{what} grad_{k}")


@pytest.mark.parametrize("tile_w", TILE_WS)
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_vs_oracle(name, frame, tile_w):
    W, H = frame
    if name == "restart":
        check_restart(W, H, tile_w)
    else:
        CHECKS[name](W, H)
    _assert_all(_hip_scene(name, W, H, tile_w), _reference(name, W, H), f"{name} {W}x{H} tile_w={tile_w}")


@pytest.mark.parametrize("tile_w", TILE_WS)
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_is_deterministic(name, frame, tile_w):
    W, H = frame
    arrs, gI, gD = _scene(name, W, H)
    first = _hip_scene(name, W, H, tile_w)
    again = _hip(arrs, W, H, gI, gD, dict(tile_w=tile_w, **SCENES[name][1]))
    for k in GRADS + ["image", "depth"]:
        assert np.array_equal(first[k], again[k]), k
