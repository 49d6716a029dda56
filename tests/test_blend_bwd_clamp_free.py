"""Clamp-gradient select and per-entry reduction of k_composite_bwd (fgs_composite.hip) at the seams of its loops: work-unit starts,
64-entry chunk boundaries, a unit's last (partial) chunk.

The scenes were written for a form of the kernel that picks, once per work unit (tile, depth segment), one of two copies of its
chunk / list loop -- a unit none of whose entries can reach the alpha clamp (stage_decode_w's flag bit 8 set on every entry:
opacity <= 0.98 and a conic that is positive definite with a margin) running a copy without the clamp-flag test and the
clamp-gradient select.  That form was measured slower and is not in the tree (DESIGN_LOG.md 18).  The scenes stay: a wrong unit
predicate shows as a gradient through a pixel where alpha sits on the clamp (1 / (1 - 0.99) = 100 x S there), and they put the one
entry whose clamp binds where such a predicate -- or anything else that treats the first / last entry of a chunk or of a unit
specially -- is most easily wrong.  What IS in the tree and has exactly those seams: the ten sums of a list entry are reduced
and stored one entry late, at the top of the next entry, across chunk boundaries, the last entry of a unit behind the loop.

Geometry (the same in every scene): 220 small Gaussians with their means inside the tile at the frame's origin -- list position
in that tile = index, on 16 x 16 and on 32 x 16 tiles -- and 60 larger ones behind them all over the frame.  Depth segments of
64 (also the default at this size) and of 128 entries: 4 and 2 units in the crowded tile, the second unit of 128 with a last
chunk of 28.  Entry K of the crowded tile's list is entry K % seg_len of unit K // seg_len:
    K = 128: first entry of a unit (of unit 1 of 128, of unit 2 of 64);   K = 63 / 64: the chunk boundary inside unit 0 of 128 (last
    entry of unit 0 / first of unit 1 of 64);   K = 200: the last chunk of unit 1 of 128 only (unit 3 of 64).
Scenes: `free` all opacities 0.8 (no entry flagged); `all` every opacity 0.995 with the means on pixel centres (alpha on the
clamp there; every entry flagged); `one@K` entry K at 0.995 on a pixel centre, the rest 0.8; `conic@64` entry 64 a needle
at 45 degrees whose conic fails 3.996 a d > (b + c)^2, opacity 0.5, between the pixel centres (see _scene); `op098@64` / `op098next@64` entry 64 at float32 0.98 (not
flagged) / the next float above (flagged).  Every placement and every flag is asserted on the CPU from the oracle's projection.

Statement: image, depth and the five input gradients within 1e-4 of max of the C oracle (fp64 referee where helpers.referee
selects it), 64 x 32 and 40 x 24 frames, both tile shapes; every scene bitwise reproducible."""
import functools

import numpy as np
import pytest
import torch

from helpers import assert_with_referee, referee

pytestmark = pytest.mark.gpu

GRADS = ["positions", "scales", "rotations", "colors", "opacities"]
BG = (0.05, 0.1, 0.15)
FOCAL = 51.2
FRAMES = [(64, 32), (40, 24)]
TILE_WS = [16, 32]
TUNINGS = {"segdefault": {}, "seg64": dict(seg_len=64), "seg128": dict(seg_len=128)}
N_CROWD, N_REST = 220, 60
CENTRE = (8, 8)  # the pixel of the marked entry: its bbox stays inside the crowded tile on both tile shapes
OP_NEXT = float(np.nextafter(np.float32(0.98), np.float32(1.0)))
SCENES = ["free", "all", "one@128", "one@63", "one@64", "one@200", "conic@64", "op098@64", "op098next@64"]


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _marked(name):
    return int(name.split("@")[1]) if "@" in name else None


@functools.lru_cache(maxsize=None)
def _scene(name, W, H):
    """Flat Gaussians turned about the viewing axis, item 0 frontmost (the construction of test_blend_exec_masks._build): bbox radius
    r pixels = 3 x the larger in-plane axis."""
    rs = np.random.RandomState(9100 + W)
    N = N_CROWD + N_REST
    u = np.concatenate([rs.uniform(1.5, 14.5, N_CROWD), rs.uniform(0.0, W, N_REST)])
    v = np.concatenate([rs.uniform(1.5, 14.5, N_CROWD), rs.uniform(0.0, H, N_REST)])
    r = np.concatenate([rs.uniform(1.0, 1.8, N_CROWD), rs.uniform(2.0, 5.0, N_REST)])
    th = rs.uniform(0.0, np.pi, N)
    color = (0.2 + 0.7 * rs.random_sample((N, 3))).astype(np.float32)
    gI = rs.standard_normal((3, H, W)).astype(np.float32)
    gD = (rs.standard_normal((H, W)) * 0.1).astype(np.float32) + 0.05
    opacity = np.full(N, 0.8, np.float32)
    minor = np.full(N, 0.6)
    k = _marked(name)
    if name == "all":
        opacity[:] = 0.995
        u, v = np.floor(u), np.floor(v)  # means on pixel centres: G = 1 there
    if k is not None:
        u[k], v[k], r[k] = CENTRE[0], CENTRE[1], 3.0
        opacity[k] = {"one": 0.995, "conic": 0.5, "op098": 0.98, "op098next": OP_NEXT}[name.split("@")[0]]
        if name.startswith("conic"):
            # A needle at 45 degrees, 2 x 0.02 pixels in standard deviations: the eigenvalue ratio of its covariance (with the projection's
            # 1e-4 regularisation) is 1.25e-4, half of the 2.5e-4 below which 3.996 a d > (b + c)^2 fails.  Any conic that fails it is a
            # needle of 63 : 1 or thinner; where such a needle crosses pixel centres its quadratic form cancels to 1 / 4000 of its terms and
            # its position / scale / rotation gradients (which grow as 1 / width and are the largest of the frame as soon as the needle shows
            # at all) are not a 1e-4 quantity for ANY fp32 evaluation: over a sweep of lengths, widths and offsets the oracle's own fp32 run
            # was up to 2e-3 of max from its fp64 run, and above 5e-5 in nearly every setting where the needle held 1 % of a tensor or more.  What this scene is for
            # is the FLAG of an entry in a unit's list, not fp32 needles (the random sweeps have those, under the referee), so the needle
            # runs BETWEEN the pixel centres (0.21 pixels = 10 widths from the nearest): in the list, in the sub-tile passes, flagged,
            # and adding nothing.  check_scene asserts that the oracle's fp32 run is adequate here (within 5e-5 of its fp64 run).
            u[k], r[k], th[k], minor[k] = CENTRE[0] + 0.3, 6.0, np.pi / 4, 1e-2
    z = -2.0 - 0.004 * np.arange(N)
    s = r / 3.0 * -z / FOCAL
    pos = np.stack([(u - W / 2) * -z / FOCAL, -(v - H / 2) * -z / FOCAL, z], 1).astype(np.float32)
    scale = np.stack([s, minor * s, 1e-3 * s], 1).astype(np.float32)
    quat = np.stack([np.cos(th / 2), 0 * th, 0 * th, np.sin(th / 2)], 1).astype(np.float32)
    return [pos, scale, quat, color, opacity], gI, gD


@functools.lru_cache(maxsize=None)
def _reference(name, W, H):
    from oracle import fgs_oracle as orc
    arrs, gI, gD = _scene(name, W, H)
    ocam = orc.make_camera(np.eye(4, dtype=np.float32), FOCAL, FOCAL, W / 2, H / 2, W, H)
    r32 = orc.render(*arrs, ocam, bg=BG)
    g32 = orc.render_backward(r32, gI, gD)
    with orc.fp64():
        r64 = orc.render(*arrs, ocam, bg=BG)
        g64 = orc.render_backward(r64, gI, gD)
    return r32, g32, r64, g64


def _flagged(r32, opacity):
    """stage_decode_w's clamp flag (bit 8) CLEAR, from the oracle's fp32 conics: opacity > 0.98 or a doubtful conic"""
    a, bc, d = [np.asarray(r32.proj["conic"], np.float32)[:, i] for i in range(3)]
    conic_ok = (a > 0) & (d > 0) & (np.float32(3.996) * a * d > bc * bc)
    return ~((opacity <= np.float32(0.98)) & conic_ok)


def _alpha_at(r32, opacity, i, px, py):
    mu, mv = [float(t) for t in r32.proj["mean2d"][i]]
    a, bc, d = [float(t) for t in r32.proj["conic"][i]]
    dx, dy = px - mu, py - mv
    return float(opacity[i]) * float(np.exp(-0.5 * (a * dx * dx + bc * dx * dy + d * dy * dy)))


def check_scene(name, W, H, tile_w, seg_len):
    """the placement the scene is there for, from the oracle's projection and tile lists; returns the units (tile, segment) that
    hold a flagged entry"""
    from oracle import fgs_oracle as orc
    r32 = _reference(name, W, H)[0]
    opacity = _scene(name, W, H)[0][4]
    assert r32.proj["visible"].all()
    assert len(opacity) <= 300
    ranges, ids = orc.tile_lists(r32.vis_sorted, r32.proj["bbox"], W, H, tile_w=tile_w)
    first = ids[ranges[0]:ranges[1]]
    assert len(first) >= N_CROWD > 3 * 64 and (first[:N_CROWD] == np.arange(N_CROWD)).all()  # list position = index, >= 4 chunks
    fl = _flagged(r32, opacity)
    units = {(t, int(j) // seg_len) for t in range(len(ranges) - 1) for j in np.nonzero(fl[ids[ranges[t]:ranges[t + 1]]])[0]}
    all_units = {(t, s) for t in range(len(ranges) - 1) for s in range(-(-int(ranges[t + 1] - ranges[t]) // seg_len))}
    k = _marked(name)
    if name == "free":
        assert not fl.any() and len(all_units) > 4
    elif name == "all":
        assert fl.all() and units == all_units
        px, py = np.rint(r32.proj["mean2d"][:, 0]), np.rint(r32.proj["mean2d"][:, 1])
        assert all(_alpha_at(r32, opacity, i, px[i], py[i]) > 0.99 for i in range(len(fl)))  # the clamp binds at every centre
    elif name == "op098@64":
        assert opacity[k] == np.float32(0.98) and not fl.any()
    else:
        assert fl[k] and fl.sum() == 1, np.nonzero(fl)[0]
        assert units == {(0, k // seg_len)} and len(all_units) > 4  # the only unit of the frame with a flagged entry
        x0, x1, y0, y1 = r32.proj["bbox"][k]
        assert 0 <= x0 and x1 <= 16 and 0 <= y0 and y1 <= 16 and x0 <= CENTRE[0] < x1 and y0 <= CENTRE[1] < y1
        al = _alpha_at(r32, opacity, k, *CENTRE)
        if name.startswith("conic"):
            assert x1 - x0 >= 12 and y1 - y0 >= 12 and al < 1e-12  # its bbox takes the entry through all four sub-tile passes of the 16 x 16 tile
            _, g32, _, g64 = _reference(name, W, H)
            assert all(referee(g32[g], g64[g])[2] <= 5e-5 for g in GRADS)  # fp32 is adequate for the reference itself
        elif name.startswith("one"):
            assert al > 0.99 and _alpha_at(r32, opacity, k, CENTRE[0] + 1, CENTRE[1]) < 0.99  # binds at the centre, not beside it
        else:
            assert opacity[k] == np.nextafter(np.float32(0.98), np.float32(1.0)) and al < 0.99
    return units


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
def _hip_scene(name, W, H, tile_w, seg):
    arrs, gI, gD = _scene(name, W, H)
    return _hip(arrs, W, H, gI, gD, dict(tile_w=tile_w, **TUNINGS[seg]))


@pytest.mark.parametrize("seg", sorted(TUNINGS))
@pytest.mark.parametrize("tile_w", TILE_WS)
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("name", SCENES)
def test_scene_vs_oracle(name, frame, tile_w, seg):
    W, H = frame
    check_scene(name, W, H, tile_w, TUNINGS[seg].get("seg_len", 64))  # (64 is the default at this size: fgs_plan.cpp)
    got = _hip_scene(name, W, H, tile_w, seg)
    r32, g32, r64, g64 = _reference(name, W, H)
    what = f"{name} {W}x{H} tile_w={tile_w} {seg}"
    assert_with_referee(got["image"], r32.image, r64.image, f"{what} image")
    assert_with_referee(got["depth"], r32.depth, r64.depth, f"{what} depth")
    for k in GRADS:
        assert_with_referee(got[k], g32[k], g64[k], f"{what} grad_{k}")


@pytest.mark.parametrize("seg", sorted(TUNINGS))
@pytest.mark.parametrize("tile_w", TILE_WS)
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("name", SCENES)
def test_scene_is_deterministic(name, frame, tile_w, seg):
    W, H = frame
    arrs, gI, gD = _scene(name, W, H)
    first = _hip_scene(name, W, H, tile_w, seg)
    again = _hip(arrs, W, H, gI, gD, dict(tile_w=tile_w, **TUNINGS[seg]))
    for k in GRADS + ["image", "depth"]:
        assert np.array_equal(first[k], again[k]), k
