"""The blend backward accumulates the moments of dL/dG per sub-tile ROW of a tile (sum dG, sum dG dx, sum dG dx^2 for the
lane's two values of dy) and folds the rows once per list entry (k_composite_bwd, fgs_composite.hip).  What can go wrong there
depends on WHICH sub-tiles of a tile a Gaussian touches -- only the upper row, only the lower row, one sub-tile column, both rows --
and on the size of the Gaussian against a pixel (the second moments of a sub-pixel Gaussian are tiny against |dG| * tile size^2),
so Gaussians are placed by hand such that every such pattern occurs; the patterns are verified on the CPU from the oracle's
bboxes.  A crowded scene with short depth segments takes the checkpoint restart and re-base through the same code, and the
kernel must stay deterministic.

Statement: all five input gradients within 1e-4 of max of the C oracle, the fp64 referee judging where helpers.referee selects
it, on 16 x 16 and on 32 x 16 tiles."""
import functools

import numpy as np
import pytest
import torch

from helpers import assert_with_referee, synth_aniso

pytestmark = pytest.mark.gpu

GRADS = ["positions", "scales", "rotations", "colors", "opacities"]
BG = (0.15, 0.3, 0.45)
FW, FH, FOCAL, ZMEAN = 64, 32, 51.2, -2.0  # the hand-placed frame: 2 x 2 tiles of 32 x 16, 4 x 2 of 16 x 16
# pixel radius of the bbox (3 sigma) of the hand-placed Gaussians: a few pixels / sub-pixel.  sigma = FOCAL * scale / |z|, so the
# sub-pixel radius 1.2 px is a largest scale of 1.2 / 3 * 2 / 51.2 = 0.0156 world units (sigma 0.4 px); the other two axes are smaller
R_SMALL, R_SUB = 2.6, 1.2

# name -> [(u, v, bbox radius in px or None = the case's default)]: projected means on the 64 x 32 frame
PLACES = {
    "row0": [(5.3, 3.6, None), (20.5, 4.4, None), (45.2, 19.5, None)],               # pixel rows 0-7 of a tile
    "row1": [(9.5, 11.7, None), (37.4, 12.2, None), (58.6, 27.5, None)],             # pixel rows 8-15
    "cols": [(4.0, 7.9, None), (12.1, 4.0, None), (19.8, 12.0, None), (27.9, 8.3, None)],  # one 8-pixel column each, all four
    "rows_straddled": [(16.2, 7.8, None), (48.9, 24.1, None)],                       # across the row-7/8 boundary
    "tiles_straddled": [(32.2, 15.9, None), (31.6, 16.3, None)],                     # across a tile boundary in x and y
    "frame": [(32.0, 16.0, 80.0), (20.0, 10.0, None)],                               # [0] covers the whole frame
}


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _placed_scene(place, sub):
    """Gaussians whose projected means are PLACES[place] and whose bbox radius is ~r pixels: anisotropic, randomly rotated."""
    rs = np.random.RandomState(sorted(PLACES).index(place) * 2 + int(sub) + 500)
    pts = PLACES[place]
    N = len(pts)
    pos, scale = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32)
    for i, (u, v, r) in enumerate(pts):
        z = ZMEAN - 0.05 * i
        r = (R_SUB if sub else R_SMALL) if (r is None or sub) else r
        pos[i] = ((u - FW / 2) * -z / FOCAL, -(v - FH / 2) * -z / FOCAL, z)
        scale[i] = r / 3.0 * -z / FOCAL * np.array([1.0, 0.5, 0.75])[rs.permutation(3)]
    quat = rs.standard_normal((N, 4)).astype(np.float32)
    color = rs.random_sample((N, 3)).astype(np.float32)
    opacity = rs.uniform(0.3, 1.0, N).astype(np.float32)
    gI = rs.standard_normal((3, FH, FW)).astype(np.float32)
    gD = (rs.standard_normal((FH, FW)) * 0.1).astype(np.float32) + 0.05
    return [pos, scale, quat, color, opacity], gI, gD


def _oracle_pair(arrs, W, H, fx, cx, cy, gI, gD):
    """(fp32 oracle forward, fp32 gradients, fp64 gradients) of one image."""
    from oracle import fgs_oracle as orc
    ocam = orc.make_camera(np.eye(4, dtype=np.float32), fx, fx, cx, cy, W, H)
    r32 = orc.render(*arrs, ocam, bg=BG)
    g32 = orc.render_backward(r32, gI, gD)
    with orc.fp64():
        g64 = orc.render_backward(orc.render(*arrs, ocam, bg=BG), gI, gD)
    return r32, g32, g64


@functools.lru_cache(maxsize=None)
def _placed_reference(place, sub):
    arrs, gI, gD = _placed_scene(place, sub)
    return (arrs, gI, gD) + _oracle_pair(arrs, FW, FH, FOCAL, FW / 2, FH / 2, gI, gD)


def _touched_patterns(bbox, tile_w):
    """{(tile x, tile y): (row bits, column bits)} of one bbox [x0, x1) x [y0, y1): the 8-pixel rows (2) and columns (tile_w / 8)
    of every tile that the bbox intersects -- the touched sub-tiles of the tile are their outer product."""
    x0, x1, y0, y1 = [int(v) for v in bbox]
    out = {}
    for ty in range(y0 // 16, (y1 - 1) // 16 + 1):
        for tx in range(x0 // tile_w, (x1 - 1) // tile_w + 1):
            rows = sum(1 << r for r in range(2) if y0 < ty * 16 + 8 * r + 8 and y1 > ty * 16 + 8 * r)
            cols = sum(1 << c for c in range(tile_w // 8) if x0 < tx * tile_w + 8 * c + 8 and x1 > tx * tile_w + 8 * c)
            out[(tx, ty)] = (rows, cols)
    return out


def _check_patterns(place, sub, bboxes, visible, tile_w):
    """The touched patterns the case was built for really occur (oracle bboxes; asserted, never skipped)."""
    assert visible.all(), (place, sub)
    pats = [_touched_patterns(b, tile_w) for b in bboxes]
    every = [p for d in pats for p in d.values()]
    ncol = tile_w // 8
    if sub:  # sub-pixel: the bbox spans at most 4 pixels
        assert all(b[1] - b[0] <= 4 and b[3] - b[2] <= 4 for b in bboxes), (place, bboxes)
    if place == "row0":
        assert every and all(rows == 1 for rows, _ in every), every
    elif place == "row1":
        assert every and all(rows == 2 for rows, _ in every), every
    elif place == "cols":
        assert all(len(d) == 1 for d in pats), pats
        assert [1 << (i % ncol) for i in range(4)] == [next(iter(d.values()))[1] for d in pats], pats
        assert {rows for rows, _ in every} == {1, 2, 3}, every  # ... and in the upper, the lower and both rows
    elif place == "rows_straddled":
        assert every and all(rows == 3 for rows, _ in every), every
    elif place == "tiles_straddled":
        assert all(len(d) == 4 for d in pats), pats
        assert sorted(pats[0].values()) == sorted([(2, 1 << (ncol - 1)), (2, 1), (1, 1 << (ncol - 1)), (1, 1)]), pats
    elif place == "frame" and not sub:
        assert len(pats[0]) == (FW // tile_w) * (FH // 16) and set(pats[0].values()) == {(3, (1 << ncol) - 1)}, pats[0]


def _hip_grads(arrs, W, H, fx, cx, cy, gI, gD, tuning):
    """Gradients of all five inputs through the renderer; arrays are (N, .) or (B, N, .)."""
    from fresnel_amd.renderer import Camera, TileBasedRenderer
    dev = _cuda()
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True) for a in arrs]
    ren = TileBasedRenderer(W, H, background=BG)
    ren.tuning = dict(tuning)
    img, dep = ren(*ts, Camera(fx, fx, cx, cy, W, H), return_depth=True)
    ((img * torch.from_numpy(gI).to(dev)).sum() + (dep * torch.from_numpy(gD).to(dev)).sum()).backward()
    return {k: t.grad.detach().cpu().numpy() for k, t in zip(GRADS, ts)}


@pytest.mark.parametrize("tile_w", [16, 32])
@pytest.mark.parametrize("sub", [False, True], ids=["small", "subpixel"])
@pytest.mark.parametrize("place", sorted(PLACES))
def test_hand_placed_gaussians_vs_oracle(place, sub, tile_w):
    arrs, gI, gD, r32, g32, g64 = _placed_reference(place, sub)
    assert 1 <= len(arrs[0]) <= 4
    if sub:
        assert float(arrs[1].max()) <= 0.02
    _check_patterns(place, sub, r32.proj["bbox"], r32.proj["visible"].astype(bool), tile_w)
    got = _hip_grads(arrs, FW, FH, FOCAL, FW / 2, FH / 2, gI, gD, dict(tile_w=tile_w))
    for k in GRADS:
        assert np.abs(g32[k]).max() > 0, (place, k)  # the case exercises this gradient at all
        assert_with_referee(got[k], g32[k], g64[k], f"{place} sub={sub} tile_w={tile_w} grad_{k}")


# ---- crowded: 300 anisotropic Gaussians on a frame that is no multiple of the tile, depth segments of 64 entries ----
CW, CH, CN, SEG = 48, 24, 300, 64
CROWD_SMAX = (0.02, 0.2)


def _crowd_scene(smax):
    seed = 900 + int(round(smax * 100))
    rs = np.random.RandomState(seed + 1)
    arrs = list(synth_aniso(CN, seed, opacity_max=1.0, smax=smax))
    gI = rs.standard_normal((3, CH, CW)).astype(np.float32)
    gD = (rs.standard_normal((CH, CW)) * 0.1).astype(np.float32)
    return arrs, gI, gD


CROWD_CAM = (0.9 * CW, CW / 2 + 1.3, CH / 2 - 0.7)  # focal length, cx, cy


@functools.lru_cache(maxsize=None)
def _crowd_reference(smax):
    arrs, gI, gD = _crowd_scene(smax)
    return (arrs, gI, gD) + _oracle_pair(arrs, CW, CH, *CROWD_CAM, gI, gD)


@functools.lru_cache(maxsize=None)
def _crowd_hip(smax, tile_w):
    arrs, gI, gD = _crowd_scene(smax)
    return _hip_grads(arrs, CW, CH, *CROWD_CAM, gI, gD, dict(tile_w=tile_w, seg_len=SEG))


@pytest.mark.parametrize("tile_w", [16, 32])
@pytest.mark.parametrize("smax", CROWD_SMAX)
def test_crowded_short_segments_vs_oracle(smax, tile_w):
    from oracle import fgs_oracle as orc
    arrs, gI, gD, r32, g32, g64 = _crowd_reference(smax)
    ranges, _ = orc.tile_lists(r32.vis_sorted, r32.proj["bbox"], CW, CH, tile_w=tile_w)
    longest = int(np.diff(ranges).max())
    assert longest > (2 * SEG if smax > 0.1 else SEG), longest  # several depth segments (smax 0.2: at least three) in a tile
    got = _crowd_hip(smax, tile_w)
    for k in GRADS:
        assert_with_referee(got[k], g32[k], g64[k], f"crowded smax={smax} tile_w={tile_w} grad_{k}")


@pytest.mark.parametrize("tile_w", [16, 32])
def test_crowded_is_deterministic_and_batch_equals_single_images(tile_w):
    scenes = [_crowd_scene(s) for s in CROWD_SMAX]
    single = [_crowd_hip(s, tile_w) for s in CROWD_SMAX]
    for (arrs, gI, gD), first in zip(scenes, single):
        again = _hip_grads(arrs, CW, CH, *CROWD_CAM, gI, gD, dict(tile_w=tile_w, seg_len=SEG))
        for k in GRADS:
            assert np.array_equal(first[k], again[k]), k
    batch = _hip_grads([np.stack([sc[0][i] for sc in scenes]) for i in range(5)], CW, CH, *CROWD_CAM,
                       np.stack([sc[1] for sc in scenes]), np.stack([sc[2] for sc in scenes]), dict(tile_w=tile_w, seg_len=SEG))
    for b in range(2):
        for k in GRADS:
            assert np.array_equal(batch[k][b], single[b][k]), (b, k)
