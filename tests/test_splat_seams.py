"""Seams of the two splat renderers (WaveFieldRenderer, ASMWaveFieldRenderer: k_asm_splat<BWD, WAVE, NP> of fgs_splat.h, the output
stages of fgs_wavefield.hip / fgs_asm.hip, the plane loop of k_project and modes 1 / 2 of k_project_bwd): what the frontal goldens and the
random scenes of test_hip_asm.py never place on purpose.  Scenes are the flat, hand-turned Gaussians of test_blend_exec_masks._build
(a bbox lands where it is wanted) at depths chosen here; every placement property is asserted on the CPU from the oracle's bboxes.

  membership  residues / lanes / covers / offframe items of test_blend_exec_masks with its CPU checks (restated here on this oracle's
              bboxes), on 64 x 32 and 37 x 21 (sub-tiles
              cut by the frame on both axes); the ASM renderer with 2 planes, alternate Gaussians on either, so that both (image,
              plane, tile) lists of a tile are populated.  `counts` (112 x 48, 7 x 3 tiles: a 64 x 32 frame has no 5, 7 or 9 tiles
              in a rectangle): tile counts 1 ... 9, every residue mod 8 -- the two-rows-in-flight loop and the tail of
              k_project_bwd<1|2>.  `capped`: round Gaussians of 3 sigma radius 9 ... 20 px under max_radius 4 (bbox side 9) and of
              15 ... 20 px under 7.5 (side 16): G >= 0.2 on each outermost pixel line, a one-pixel membership error is O(0.1).
              (9 ... 15 px under 7.5 would leave 0.02 there, so that cap takes the upper part of the range.)
  lists       64 x 32, one call of three images; per tile a depth-ordered label sequence (test_phase_seams._items_groups).  List
              lengths 0, 1, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257, 333 -- the forward's four list parts are empty, hold one
              entry or run two chunks; the backward's 64-entry units at every seam --, an empty list between two non-empty ones,
              lists whose entries all miss a sub-tile (the `msk` skip), opacities x min(1, 8 / L).  ASM: those lists on plane 0
              and a handful on plane 1.
  seg128      B = 2, N = 100 001 on 32 x 16: B N > 200 000 makes fgs_make_plan choose 128-entry backward units (asserted on the
              host from fgs_saved_layout).  All but 641 Gaussians sit behind the camera; the visible ones form lists of 127, 128,
              129 and 257 entries.
  onewave     (wave-field) B = 384 images of 128 x 128: see ONE_WAVE_B.
  cameras     B = 3, 72 x 40, N = 200, both renderers (ASM with 4 planes; the wave-field run with a depth-map gradient, the dL/ddepth
              slot of its 16-float rows through the view matrix in k_project_bwd<2>): one orbit camera per image (num_cameras = B), fx != fy, principal point
              off centre; and the three scenes through one shared camera.  Image b of the batched call is bitwise the single call.
  planes      (ASM) identity view, depth = -z exactly.  (a) P = 5 over (0.5, 2.5): depths on every plane, on every midpoint (exact
              ties in fp32: the first minimum wins), at 0.3 and 3.0.  (b) the defaults, P = 16 over (0.1, 2.0): per k the fp32 plane
              value, the fp32 midpoint of planes k and k + 1 and the floats one ulp either side of it.  The oracle's plane_idx
              (fp32 torch.linspace, first argmin) is the expected assignment; placements for which its fp64 run chooses another
              plane are dropped (PLANES_DROPPED says which).
  norm        64 x 32, background != 0.  dim: peak <= 0.8 (M = 1, no gradient through the maximum).  bright: peak >= 1.25, runner-up
              <= 0.99 peak, pixels with summed amplitude >= 1.1 and <= 0.9 and none within 1e-3 of the clamp at 1.  tie (wave-field):
              grey colours and scalar phases, the three channels of the peak pixel equal bit for bit: the maximum's gradient is
              shared by exactly three elements (torch spreads the gradient of max() evenly over ties; the oracle is the judge).

Statements (the project's own): image within 1e-4 absolute; depth map and every gradient within TOL = 1e-4 of the tensor's maximum of
the fp32 oracle; dL/dlambda through helpers.assert_wavelength_grad with the fp64 run.  test_oracle_spread asserts per scene and
per-image tensor that the oracle's own fp32-fp64 spread is <= 5e-5, the bound under which helpers.referee_tolerance calls fp32
adequate; the tensors of REFEREED are judged by helpers.assert_with_referee instead.  (dL/dlambda, one vector per call, is not in
test_oracle_spread: assert_wavelength_grad takes the referee decision itself from the two oracle runs.)  Every gradient finite, exact zeros for culled Gaussians, a second
run bitwise equal (the backward has no atomics); and -- CPU only -- the statement fails when the oracle is given one seam error of
each kind.  profiles/splat_seams.txt holds the spreads, the errors on the MI355X and what the CPU checks found."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import test_blend_exec_masks as em
import test_phase_seams as ps
from helpers import ROOT, assert_wavelength_grad, assert_with_referee, referee, rel_to_max

gpu = pytest.mark.gpu

TOL = 1e-4
SPREAD_MAX = 5e-5
BG, FOCAL = em.BG, em.FOCAL
GRADS = em.GRADS + ["phases"]
WL = np.array([0.0635, 0.05, 0.041], np.float32)
FRAMES = [(64, 32), (37, 21)]
KINDS = ["wave", "asm"]
TWO_PLANES = dict(num_planes=2, depth_range=(0.5, 1.5), focal_depth=1.0, pixel_pitch=1.0 / 256.0)  # plane 0 below depth 1.0
# ASM_ONE_WAVE_LISTS (fgs_splat.h) = 24 576 lists per launch select k_asm_splat<false, true, 1>.  One plane, 128 x 128 = 64 tiles:
# 24 576 / 64 = 384 images reach it exactly; 383 images (24 512 lists) are the last call with four list parts.
ONE_WAVE_LISTS = 24576
ONE_WAVE_FRAME = 128
ONE_WAVE_B = ONE_WAVE_LISTS // ((ONE_WAVE_FRAME // 16) ** 2)

# (scene, tensor) pairs whose oracle spread exceeds SPREAD_MAX for every seed tried (LANES_SEEDS says why): judged by helpers.referee
# -- the fp64 run, tolerance from the spread.  Spreads with the seeds in use: 1.5e-4 / 1.2e-4 (64 x 32), 5.5e-5 / 5.7e-5 / 1.0e-4
REFEREED = {"lanes-64x32-asm": ("positions", "scales"), "lanes-37x21-asm": ("positions", "scales", "phases")}


class Cam:
    def __init__(self, W, H, view=None, fx=FOCAL, fy=FOCAL, cx=None, cy=None):
        self.view = np.eye(4, dtype=np.float32) if view is None else np.asarray(view, np.float32)
        self.fx, self.fy, self.cx, self.cy = fx, fy, W / 2 if cx is None else cx, H / 2 if cy is None else cy


class Image:
    """one image: the five input arrays, phases, upstream gradients, and which Gaussians are culled by placement"""

    def __init__(self, arrs, phases, gI, gD, culled):
        self.arrs, self.phases, self.gI, self.gD, self.culled = arrs, phases, gI, gD, culled


class Scene:
    """kind: 'wave' | 'asm'.  batch: the images of the call as indices into `images` (reference() runs the oracle once per image)"""

    def __init__(self, kind, W, H, images, cams=None, batch=None, max_radius=64.0, asm=None, **extra):
        self.kind, self.W, self.H, self.images, self.max_radius = kind, W, H, images, float(max_radius)
        self.cams = cams or [Cam(W, H)]
        self.batch = list(range(len(images))) if batch is None else batch
        self.asm = dict(asm or TWO_PLANES)
        self.__dict__.update(extra)
        assert len({im.arrs[0].shape[0] for im in images}) == 1 and len(self.cams) in (1, len(self.batch))


def _alternate(n, lo=0.6, hi=1.2, step=1e-4):
    """depths for TWO_PLANES: even items on plane 0, odd items on plane 1, each set in item order"""
    return [(lo if i % 2 == 0 else hi) + step * i for i in range(n)]


def _image(W, H, items, seed, depths, round_ones=False, pad_to=None, rgb_phase=True):
    """em._build's Gaussians moved along their viewing rays to `depths` (the projection is unchanged by that)"""
    n_on = len(items)
    items, depths = list(items), list(depths)
    while pad_to is not None and len(items) < pad_to:  # (a batch has one N: the rest is culled by placement, off the frame)
        items.append(ps._off(W, H)[len(items) % 2])
        depths.append(0.9)
    arrs, gI, gD = em._build(W, H, items, seed, round_ones=round_ones)
    d = np.asarray(depths, np.float64)
    uv = np.array([(u, v) for u, v, _ in items], np.float64)
    z0 = -arrs[0][:, 2].astype(np.float64)
    arrs[0] = np.stack([(uv[:, 0] - W / 2) * d / FOCAL, -(uv[:, 1] - H / 2) * d / FOCAL, -d], 1).astype(np.float32)
    arrs[1] = (arrs[1].astype(np.float64) * (d / z0)[:, None]).astype(np.float32)
    rs = np.random.RandomState(seed + 7919)
    ph = (rs.random_sample((len(items), 3) if rgb_phase else len(items)) * 2 * np.pi).astype(np.float32)
    culled = np.arange(len(items)) >= n_on
    return Image(arrs, ph, gI, gD, culled)


# ---- membership ----
MEMBERSHIP = ["residues", "lanes", "covers", "offframe"]
COUNTS_FRAME = (112, 48)
CAPS = {"capped4": (4.0, 9.0, 9), "capped7.5": (7.5, 15.0, 16)}  # max_radius, smallest 3 sigma radius, bbox side where the frame does not cut
LANES_UPSTREAM = ps.LANES_UPSTREAM
# (colours, opacities, upstream gradients.  Wave-field: chosen so that test_oracle_spread holds.  ASM: propagation spreads a one-pixel
# Gaussian over the frame, scaling the upstream gradient on its pixel does not reach its rows, and dL/dpositions / dL/dscales stay
# 1e-4 ... 9e-4 apart between the oracle's two runs for every seed tried (8409, 8415, 8420 ... 8423): the seeds with the smallest
# spread, and REFEREED)
LANES_SEEDS = {("wave", 64): 8409, ("wave", 37): 8409, ("asm", 64): 8423, ("asm", 37): 8415}


def _items_counts(W, H):
    """bboxes over 1 ... 9 tiles of a 7 x 3 tile frame: (u, v, r); the frame cuts the large ones down to one or two tile rows"""
    return [(8.2, 8.3, 3.0), (16.1, 8.2, 3.0), (40.3, -6.2, 10.0), (32.2, 16.3, 4.0), (56.0, -25.0, 34.0), (40.3, 16.2, 10.0),
            (56.3, -45.0, 50.0), (56.4, -6.0, 24.0), (56.2, 24.4, 20.0), (100.4, 40.3, 5.0), (70.7, 30.2, 2.0)]


def _items_capped(W, H, lo):
    rs = np.random.RandomState(77 + W)
    return [(rs.uniform(-2.0, W + 2.0), rs.uniform(-2.0, H + 2.0), rs.uniform(lo, 20.0)) for _ in range(40)]


def _membership_scene(kind, name, W, H):
    cap = 64.0
    if name in CAPS:
        cap, lo, _ = CAPS[name]
        items, seed, round_ones = _items_capped(W, H, lo), 8460 + W, True
    elif name == "counts":
        items, seed, round_ones = _items_counts(W, H), 8450, False
    else:
        items, round_ones = em.SCENES[name][0](W, H), name == "lanes"
        seed = LANES_SEEDS[kind, W] if name == "lanes" else 8400 + sorted(em.SCENES).index(name) + W
        if name == "lanes":
            # a wide one behind them all: alone on its pixels a Gaussian's intensity does not depend on its phase, and dL/dphase
            # of a scene without overlap is rounding noise throughout
            items = items + [(W / 2 + 0.3, H / 2 + 0.2, 60.0)]
    im = _image(W, H, items + ps._off(W, H), seed, _alternate(len(items) + 2), round_ones=round_ones)
    im.culled[:] = np.arange(len(items) + 2) >= len(items)
    if name in CAPS:  # forty overlapping discs: keep the summed amplitude of the order of 1
        im.arrs[4][:len(items)] *= 0.25
    if name == "lanes":  # (test_phase_seams._membership_scene: the one-pixel Gaussians' derivatives are 1e3 x everyone else's)
        for px, py in em._lane_pixels(W, H):
            im.gI[:, py, px] *= LANES_UPSTREAM
            im.gD[py, px] *= LANES_UPSTREAM
    return Scene(kind, W, H, [im], max_radius=cap, name=name)


# ---- lists ----
LIST_SEQS = [  # three images, tiles row-major (4 x 2); labels as in test_phase_seams.SEQS_64x32
    [[0] * 64 + [1] * 63 + [4] + [2] * 64 + [3] * 64 + [4],      # 257
     [4] * 65,
     [],                                                          # an empty list between two non-empty ones
     [1] * 100 + [2] * 27,                                        # 127, sub-tiles 0 and 3 never touched
     [2],
     [3] * 63,
     [0] * 32 + [1] * 32 + [2] * 32 + [3] * 32,                   # 128
     [4] * 3 + [0] * 61],                                         # 64
    [[4] * 64,
     [0] * 129,
     [1] * 96 + [3] * 96,                                         # 192
     [],
     [2] * 97 + [4] * 96,                                         # 193
     [0] * 3,
     [3] * 9 + [0],
     [1] * 7],
    [[],
     [0] * 64 + [1] * 64 + [2] * 64 + [3] * 64,                   # 256
     [4] * 10 + [0] * 80 + [1] * 80 + [2] * 80 + [3] * 80 + [4] * 3,  # 333
     [3],
     [2] * 12 + [4] * 3 + [0] * 2,
     [1] * 8 + [3] * 16,
     [4] * 7 + [0],
     [2] * 6],
]
LIST_SEQS_PLANE1 = [  # ASM: what sits on plane 1 of the same tiles
    [[], [4], [0] * 5, [], [4] * 65, [], [1] * 2, []],
    [[2] * 3, [], [], [4] * 2, [], [3], [], [0] * 64],
    [[4] * 4, [], [1], [], [], [2] * 63, [], [4]],
]
LIST_LENGTHS = {0, 1, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257}


def _lists_scene(kind):
    W, H = 64, 32
    built = []
    for b in range(3):
        items, tiles = ps._items_groups(W, H, LIST_SEQS[b], np.random.RandomState(4000 + b))
        depths = [0.6 + 1e-4 * i for i in range(len(items))]
        scale = [min(1.0, 8.0 / len(LIST_SEQS[b][t])) for t in tiles]
        if kind == "asm":
            more, tiles1 = ps._items_groups(W, H, LIST_SEQS_PLANE1[b], np.random.RandomState(4100 + b))
            depths += [1.2 + 1e-4 * i for i in range(len(more))]
            scale += [min(1.0, 8.0 / len(LIST_SEQS_PLANE1[b][t])) for t in tiles1]
            items = items + more
        built.append((items, depths, scale))
    N = max(len(items) for items, _, _ in built) + 2
    images = []
    for b, (items, depths, scale) in enumerate(built):
        im = _image(W, H, items, 4200 + b, depths, pad_to=N, rgb_phase=False)
        im.arrs[4][:len(items)] *= np.array(scale, np.float32)
        images.append(im)
    return Scene(kind, W, H, images)


# ---- seg128 ----
SEG128_B, SEG128_N = 2, 100001
SEG128_SEQS = [[[0] * 30 + [4] * 40 + [3] * 57, [1] * 64 + [2] * 64],                    # 127, 128
               [[4] * 129, [0] * 64 + [1] * 64 + [4] + [2] * 64 + [3] * 64]]             # 129, 257


@functools.lru_cache(maxsize=None)
def _seg128_images():
    W, H, N = 32, 16, SEG128_N
    images = []
    for b, seqs in enumerate(SEG128_SEQS):
        rs = np.random.RandomState(5000 + b)
        items, tiles = ps._items_groups(W, H, seqs, rs)
        n = len(items)
        small = _image(W, H, items, 5100 + b, [1.2 + 1e-4 * i for i in range(n)], rgb_phase=False)
        small.arrs[4] *= np.array([8.0 / len(seqs[t]) for t in tiles], np.float32)
        where = np.sort(np.concatenate([[0, N - 1], 1 + rs.choice(N - 2, n - 2, replace=False)]))  # item order = depth order
        pos = np.stack([rs.uniform(-1, 1, N), rs.uniform(-1, 1, N), np.full(N, 1.0)], 1).astype(np.float32)  # z = +1: behind the camera
        scale = np.full((N, 3), 0.05, np.float32)
        quat = np.tile(np.array([1, 0, 0, 0], np.float32), (N, 1))
        color = rs.random_sample((N, 3)).astype(np.float32)
        opacity = np.full(N, 0.5, np.float32)
        phases = (rs.random_sample(N) * 2 * np.pi).astype(np.float32)
        arrs = [pos, scale, quat, color, opacity]
        for a, s in zip(arrs, small.arrs):
            a[where] = s
        phases[where] = small.phases
        culled = np.ones(N, bool)
        culled[where] = False
        images.append(Image(arrs, phases, small.gI, small.gD, culled))
    return images


def _seg128_scene(kind):
    return Scene(kind, 32, 16, _seg128_images())  # ASM: every visible Gaussian on plane 1, plane 0 is empty


# ---- one wave per list ----
def _onewave_scene(B):
    S = ONE_WAVE_FRAME
    images = []
    for j in range(4):
        rs = np.random.RandomState(6000 + j)
        items = [(rs.uniform(0, S), rs.uniform(0, S), rs.uniform(2.0, 7.0)) for _ in range(160)]
        if j == 3:  # 135 small ones inside tile (3, 3): three chunks of its list
            items[:135] = [(48 + rs.uniform(3.0, 13.0), 48 + rs.uniform(3.0, 13.0), rs.uniform(0.8, 2.4)) for _ in range(135)]
        im = _image(S, S, items, 6100 + j, [0.6 + 1e-3 * i for i in range(160)], rgb_phase=j % 2 == 0)
        if j == 3:
            im.arrs[4][:135] *= 8.0 / 135
        images.append(im)
    # (one phase layout per call: scenes 1 and 3 repeat their scalar phase per channel)
    for im in images:
        if im.phases.ndim == 1:
            im.phases = np.repeat(im.phases[:, None], 3, 1)
    return Scene("wave", S, S, images, batch=[b % 4 for b in range(B)])


# ---- cameras ----
CAMERA_SEEDS = [7000, 7003, 7002]  # (chosen so that test_oracle_spread holds through the image's own camera and through camera 0; 7001: 8.8e-5 on dL/drotations)


def _camera_scene(kind, shared):
    from fresnel_amd.renderer import create_camera_from_pose
    from helpers import synth_aniso
    W, H, N = 72, 40, 200
    cams = []
    for el, az in [(0.3, 0.5), (-0.2, -0.9), (0.5, 2.4)]:
        view = create_camera_from_pose(el, az, 64).view_matrix.numpy()
        cams.append(Cam(W, H, view, fx=60.0, fy=52.0, cx=W / 2 + 3.5, cy=H / 2 - 2.25))
    images = []
    for b in range(3):
        arrs = list(synth_aniso(N, CAMERA_SEEDS[b], opacity_max=0.9, spread=0.3, zmean=0.0, smin=0.03, smax=0.1))
        rs = np.random.RandomState(7100 + b)
        ph = (rs.random_sample((N, 3)) * 2 * np.pi).astype(np.float32)
        gI = rs.standard_normal((3, H, W)).astype(np.float32)
        gD = (rs.standard_normal((H, W)) * 0.1).astype(np.float32) + 0.05  # (wave-field: dL/ddepth, slot 12 of its rows, through the view)
        images.append(Image(arrs, ph, gI, gD, np.zeros(N, bool)))
    return Scene(kind, W, H, images, cams=cams[:1] if shared else cams,
                 asm=dict(num_planes=4, depth_range=(1.4, 2.6), focal_depth=2.0, pixel_pitch=1.0 / 256.0))


# ---- planes ----
PLANE_CASES = {"a": dict(num_planes=5, depth_range=(0.5, 2.5), focal_depth=1.0, pixel_pitch=1.0 / 256.0),
               "b": dict(num_planes=16, depth_range=(0.1, 2.0), focal_depth=0.5, pixel_pitch=1.0 / 256.0)}
# placements (what, k) for which the oracle's fp64 run (fp64 torch.linspace) chooses another plane than its fp32 run: left out
PLANES_DROPPED = {"a": [], "b": [("mid", 4), ("mid", 5), ("mid", 6)]}


def _nearest(depths, cfg, dtype):
    planes = torch.linspace(cfg["depth_range"][0], cfg["depth_range"][1], cfg["num_planes"], dtype=dtype)
    d = torch.tensor(np.asarray(depths, np.float32)).to(dtype)
    return (d.unsqueeze(1) - planes.unsqueeze(0)).abs().argmin(dim=1).numpy()


def plane_placements(case):
    """[(what, k, fp32 depth)]"""
    cfg = PLANE_CASES[case]
    p = torch.linspace(cfg["depth_range"][0], cfg["depth_range"][1], cfg["num_planes"]).numpy()
    out = [("plane", k, p[k]) for k in range(len(p))]
    for k in range(len(p) - 1):
        mid = np.float32((p[k] + p[k + 1]) * np.float32(0.5))
        out.append(("mid", k, mid))
        if case == "b":
            out += [("mid-", k, np.nextafter(mid, np.float32(0))), ("mid+", k, np.nextafter(mid, np.float32(9)))]
    if case == "a":
        out += [("below", 0, np.float32(0.3)), ("above", len(p) - 1, np.float32(3.0))]
    return out


def _planes_scene(case):
    W, H = 48, 32
    cfg = PLANE_CASES[case]
    places = plane_placements(case)
    same = _nearest([d for _, _, d in places], cfg, torch.float32) == _nearest([d for _, _, d in places], cfg, torch.float64)
    dropped = [(w, k) for (w, k, _), s in zip(places, same) if not s]
    kept = [p for p, s in zip(places, same) if s]
    rs = np.random.RandomState(8000 + len(places))
    per = 3 if case == "a" else 2
    items, depths, what = [], [], []
    for w, k, d in kept:
        for _ in range(per):
            items.append((rs.uniform(2.0, W - 2.0), rs.uniform(2.0, H - 2.0), rs.uniform(3.0, 6.0)))
            depths.append(d)
            what.append((w, k))
    im = _image(W, H, items, 8100 + len(places), depths)
    assert np.array_equal(-im.arrs[0][:, 2], np.asarray(depths, np.float32))  # depth = -z, the placement's float itself
    return Scene("asm", W, H, [im], asm=cfg, what=what, dropped=dropped, case=case)


# ---- normalisation ----
NORM_GAIN = {("wave", "dim"): 0.35, ("wave", "bright"): 1.0, ("wave", "tie"): 1.0,
             ("asm", "dim"): 0.35, ("asm", "bright"): 2.74}  # (asm bright: of 2.0 ... 3.2 in steps of 0.02 the gain that keeps every pixel furthest from the clamp at 1: 2.4e-3)
NORM_SEED = {"wave": 0, "asm": 0}


def _norm_scene(kind, regime):
    W, H = 64, 32
    rs = np.random.RandomState(9000 + NORM_SEED[kind])
    items = [(20.3, 12.2, 9.0)] + [(rs.uniform(30.0, W), rs.uniform(0.0, H), rs.uniform(3.0, 6.0)) for _ in range(9)]
    im = _image(W, H, items + ps._off(W, H), 9100 + NORM_SEED[kind], _alternate(len(items) + 2), round_ones=True, rgb_phase=regime != "tie")
    im.culled[:] = np.arange(len(items) + 2) >= len(items)
    im.arrs[4][0], im.arrs[3][0] = 1.6, (0.9, 0.7, 0.8)  # the one that sets the peak; the others stay well below it
    im.arrs[4][1:len(items)] *= 0.5
    if regime == "tie":
        im.arrs[3][:] = im.arrs[3][:, :1]
    im.arrs[4] *= NORM_GAIN[kind, regime]
    return Scene(kind, W, H, [im], regime=regime)


CASES = {}
for _k in KINDS:
    for _W, _H in FRAMES:
        for _n in MEMBERSHIP + list(CAPS):
            CASES[f"{_n}-{_W}x{_H}-{_k}"] = functools.partial(_membership_scene, _k, _n, _W, _H)
    CASES[f"counts-{COUNTS_FRAME[0]}x{COUNTS_FRAME[1]}-{_k}"] = functools.partial(_membership_scene, _k, "counts", *COUNTS_FRAME)
    CASES[f"lists-64x32-{_k}"] = functools.partial(_lists_scene, _k)
    CASES[f"seg128-32x16-{_k}"] = functools.partial(_seg128_scene, _k)
    for _r in ("dim", "bright") + (("tie",) if _k == "wave" else ()):
        CASES[f"norm_{_r}-64x32-{_k}"] = functools.partial(_norm_scene, _k, _r)
for _B in (ONE_WAVE_B, ONE_WAVE_B - 1):
    CASES[f"onewave{_B}-128x128-wave"] = functools.partial(_onewave_scene, _B)
for _k in KINDS:
    CASES[f"cameras_each-72x40-{_k}"] = functools.partial(_camera_scene, _k, False)
    CASES[f"cameras_shared-72x40-{_k}"] = functools.partial(_camera_scene, _k, True)
for _c in PLANE_CASES:
    CASES[f"planes_{_c}-48x32-asm"] = functools.partial(_planes_scene, _c)
KEYS = sorted(CASES)


@functools.lru_cache(maxsize=None)
def scene(key):
    return CASES[key]()


def _ocam(sc, b):
    from oracle import fgs_oracle as orc
    c = sc.cams[b if len(sc.cams) > 1 else 0]
    return orc.make_camera(c.view, c.fx, c.fy, c.cx, c.cy, sc.W, sc.H)


def oracle_run(sc, j, f64=False, cam_of=None, **over):
    """the oracle on image j of the scene (through camera `cam_of`, default j), fp32 or fp64 (projection included)"""
    from oracle import asm_oracle
    im = sc.images[j]
    kw = dict(bg=BG, max_radius=sc.max_radius, grad_out=im.gI)
    if f64:
        kw.update(dtype=torch.float64, project_f64=True)
    kw.update(over)
    cam = _ocam(sc, j if cam_of is None else cam_of)
    if sc.kind == "wave":
        return asm_oracle.render_wave(*im.arrs, im.phases, cam, grad_depth=im.gD, **kw)
    return asm_oracle.render(*im.arrs, im.phases, WL, cam, **sc.asm, **kw)


_SHARED = {"onewave383-128x128-wave": "onewave384-128x128-wave"}  # the same four images: one oracle run for both calls


@functools.lru_cache(maxsize=None)
def reference(key):
    """per image of the scene (r32, r64): the oracle in fp32 and in fp64 (dtype=torch.float64, project_f64=True); left unchanged by
    everything that reads it"""
    if key in _SHARED:
        return reference(_SHARED[key])
    sc = scene(key)
    out = []
    for j in range(len(sc.images)):
        r32 = oracle_run(sc, j)
        # the fp64 run keeps the fp32 run's integer stage, as fgs_oracle.fp64 does: hand-placed means put u +- r on an integer, where
        # the fp64 projection truncates to the other side (covers, offframe) -- that is another scene, not a rounding error
        out.append((r32, oracle_run(sc, j, f64=True, bbox=r32["proj"]["bbox"])))
    return out


def _hip(sc):
    """one call of len(sc.batch) images, forward and backward -> arrays with a leading image axis"""
    from fresnel_amd.renderer import ASMWaveFieldRenderer, Camera, WaveFieldRenderer
    dev = ps._cuda()
    ims = [sc.images[j] for j in sc.batch]
    ts = [torch.from_numpy(np.stack([im.arrs[i] for im in ims])).to(dev).requires_grad_(True) for i in range(5)]
    ph = torch.from_numpy(np.stack([im.phases for im in ims])).to(dev).requires_grad_(True)
    cams = []
    for c in sc.cams:
        cams.append(Camera(c.fx, c.fy, c.cx, c.cy, sc.W, sc.H))
        cams[-1].set_view(torch.from_numpy(c.view.copy()))
    cam = cams[0] if len(cams) == 1 else cams
    gI = torch.from_numpy(np.stack([im.gI for im in ims])).to(dev)
    leaves = dict(zip(GRADS, ts + [ph]))
    out = {}
    if sc.kind == "wave":
        ren = WaveFieldRenderer(sc.W, sc.H, background=BG, max_radius=sc.max_radius).to(dev)
        img, dep = ren(*ts, cam, return_depth=True, phases=ph)
        gD = torch.from_numpy(np.stack([im.gD for im in ims])).to(dev)
        ((img * gI).sum() + (dep * gD).sum()).backward()
        out["depth"] = dep.detach().cpu().numpy()
    else:
        a = sc.asm
        ren = ASMWaveFieldRenderer(sc.W, sc.H, background=BG, max_radius=sc.max_radius, num_depth_planes=a["num_planes"],
                                   depth_range=a["depth_range"], focal_depth=a["focal_depth"], pixel_pitch=a["pixel_pitch"]).to(dev)
        leaves["wavelengths"] = torch.from_numpy(WL).to(dev).requires_grad_(True)
        img = ren(*ts, cam, phases=ph, wavelengths_rgb=leaves["wavelengths"])
        (img * gI).sum().backward()
    out.update({k: t.grad.detach().cpu().numpy() for k, t in leaves.items()})
    out["image"] = img.detach().cpu().numpy()
    return out


@functools.lru_cache(maxsize=None)
def hip(key):
    return _hip(scene(key))


# ---- what the scenes place (CPU, from the oracle's bboxes) ----
def _bb(r):
    return np.asarray(r["proj"]["bbox"], np.int64)


def _G(proj, n, box):
    x0, x1, y0, y1 = box
    u, v = [float(t) for t in proj["mean2d"][n]]
    ca, cbc, cd = [float(t) for t in proj["conic"][n]]
    dx, dy = np.meshgrid(np.arange(x0, x1) - u, np.arange(y0, y1) - v)
    return np.exp(-0.5 * (ca * dx * dx + cbc * dx * dy + cd * dy * dy))


def tile_counts(bb):
    ok = (bb[:, 1] > bb[:, 0]) & (bb[:, 3] > bb[:, 2])
    n = ((bb[:, 1] - 1) // 16 - bb[:, 0] // 16 + 1) * ((bb[:, 3] - 1) // 16 - bb[:, 2] // 16 + 1)
    return np.where(ok, n, 0)


@functools.lru_cache(maxsize=None)
def lists(key):
    """per image and plane (one plane for the wave-field renderer): list lengths per tile and, per tile, the set of sub-tiles
    that each entry touches (a 4-bit mask per entry, in list order)"""
    from oracle import fgs_oracle as orc
    sc = scene(key)
    out = []
    for r32, _ in reference(key):
        proj = r32["proj"]
        bb = _bb(r32)
        _, vs = orc.depth_order(proj["depth"], proj["visible"])
        plane = r32["plane_idx"] if sc.kind == "asm" else np.zeros(len(bb), int)
        per_plane = []
        for p in range(sc.asm["num_planes"] if sc.kind == "asm" else 1):
            ranges, ids = orc.tile_lists(vs[plane[vs] == p], proj["bbox"], sc.W, sc.H)
            masks = []
            for t in range(len(ranges) - 1):
                seg = ids[ranges[t]:ranges[t + 1]]
                m = np.zeros(len(seg), int)
                for w in range(4):
                    sx, sy = ps._sub_rect(sc.W, sc.H, t, w)
                    m |= ((bb[seg, 0] < sx + 8) & (bb[seg, 1] > sx) & (bb[seg, 2] < sy + 8) & (bb[seg, 3] > sy)).astype(int) << w
                masks.append(m)
            per_plane.append(dict(length=np.diff(ranges), masks=masks, ids=[ids[ranges[t]:ranges[t + 1]] for t in range(len(ranges) - 1)]))
        out.append(per_plane)
    return out


def _both_planes(key):
    """ASM membership scenes: alternate Gaussians on either plane, both lists of some tile populated"""
    sc = scene(key)
    if sc.kind != "asm":
        return
    r32 = reference(key)[0][0]
    vis = r32["proj"]["visible"].astype(bool)
    assert np.array_equal(r32["plane_idx"][vis], (np.arange(len(vis)) % 2)[vis])
    L = lists(key)[0]
    assert ((L[0]["length"] > 0) & (L[1]["length"] > 0)).any()


def _check_residues(W, H, bb, proj, op):
    assert len(bb) == 48 and ((bb[:, 1] - bb[:, 0]) <= 14).all() and ((bb[:, 1] - bb[:, 0]) >= 2).all()
    for k, what in enumerate(("x0", "x1", "y0", "y1")):
        assert set(bb[:, k] % 8) == set(range(8)), (what, sorted(set(bb[:, k] % 8)))  # every residue mod 8 on all four edges ...
    for k in (0, 1):  # ... in both sub-tile columns of a tile (x1 is one past the last column)
        assert {int(h) for h in (bb[:, k] - k) % 16 // 8} == {0, 1}, k
    for k in (2, 3):  # ... and in both sub-tile rows
        assert {int(h) for h in (bb[:, k] - (k - 2)) % 16 // 8} == {0, 1}, k


def _check_lanes(W, H, bb, proj, op):
    px = em._lane_pixels(W, H)
    for i, (x, y) in enumerate(px):
        assert tuple(bb[i]) == (x, x + 1, y, y + 1), (i, bb[i])  # 1 x 1
    lanes = {8 * (y % 8) + x % 8 for x, y in px}
    assert {0, 7, 56, 63} <= lanes and any(l % 8 not in (0, 7) and l // 8 not in (0, 7) for l in lanes)  # sub-tile corners, interior
    n = len(px)
    assert tuple(bb[n]) == (0, 1, 8, 16) and tuple(bb[n + 1]) == (W - 1, W, 0, 8), bb[n:n + 2]      # 1 x 8
    assert tuple(bb[n + 2]) == (8, 16, 0, 1) and tuple(bb[n + 3]) == (16, 24, H - 1, H), bb[n + 2:]  # 8 x 1
    for i in range(len(bb)):  # every one of them puts an amplitude on the frame that the 1e-4 statement sees
        assert float(_G(proj, i, bb[i]).max()) * float(op[i]) > 2e-3, i


def _check_covers(W, H, bb, proj, op):
    assert (bb[:3] == (0, W, 0, H)).all(), bb[:3]  # frame-covering: all 64 lanes of every sub-tile
    inner = bb[3:]
    assert len(inner) >= 8
    assert (inner[:, 0] // 16 == (inner[:, 1] - 1) // 16).all() and (inner[:, 2] // 16 == (inner[:, 3] - 1) // 16).all(), inner  # inside one tile
    assert {int(h) for h in inner[:, 0] % 32 // 16} == {0, 1}


def _check_offframe(W, H, bb, proj, op):
    for k, edge in enumerate((0, W, 0, H)):  # bboxes cut by the frame on each side
        assert (bb[:, k] == edge).sum() >= 3, (k, bb[:, k])
    assert ((bb[:, 1] > bb[:, 0]) & (bb[:, 3] > bb[:, 2])).all()


MEMBERSHIP_CHECKS = {"residues": _check_residues, "lanes": _check_lanes, "covers": _check_covers, "offframe": _check_offframe}


def check_membership(key):
    sc = scene(key)
    name, W, H = sc.name, sc.W, sc.H
    r32, r64 = reference(key)[0]
    bb = _bb(r32)
    n = int((~sc.images[0].culled).sum())
    vis = r32["proj"]["visible"].astype(bool)
    assert vis[:n].all() and not vis[n:].any() and np.array_equal(r64["proj"]["visible"], r32["proj"]["visible"])
    _both_planes(key)
    found = {}
    if name in MEMBERSHIP:
        # test_blend_exec_masks's checks restated on THIS oracle run (the same items at other depths: where it puts u +- r on an
        # integer, a bbox edge of covers / offframe lands one pixel to the other side here)
        mine = bb[:len(em.SCENES[name][0](W, H))]
        MEMBERSHIP_CHECKS[name](W, H, mine, r32["proj"], sc.images[0].arrs[4])
        found["bboxes unlike test_blend_exec_masks's"] = int((mine != em._bboxes(name, W, H)).any(1).sum())
    elif name == "counts":
        tc = tile_counts(bb[:n])
        assert set(tc) >= set(range(1, 10)) and {int(c) % 8 for c in tc} == set(range(8)), sorted(tc)
        found["tile counts"] = sorted(int(c) for c in tc)
    else:
        cap, lo, side = CAPS[name]
        uncut = (bb[:n, 0] > 0) & (bb[:n, 1] < W) & (bb[:n, 2] > 0) & (bb[:n, 3] < H)
        assert uncut.sum() >= 3 and (~uncut).sum() >= 3, uncut.sum()
        assert (r32["proj"]["radius"][:n] == np.float32(cap)).all()  # the cap binds on every one of them
        assert ((bb[:n, 1] - bb[:n, 0])[uncut] == side).all() and ((bb[:n, 3] - bb[:n, 2])[uncut] == side).all(), bb[:n][uncut]
        weakest = 1.0
        for i in np.nonzero(uncut)[0]:
            x0, x1, y0, y1 = bb[i]
            for box in ((x0, x0 + 1, y0, y1), (x1 - 1, x1, y0, y1), (x0, x1, y0, y0 + 1), (x0, x1, y1 - 1, y1)):
                weakest = min(weakest, float(_G(r32["proj"], i, box).max()))
        assert weakest >= 0.2, weakest  # of a peak of at most 1: the Gaussian is still bright where the cap cuts it
        found.update(uncut=int(uncut.sum()), weakest_outermost_line=round(weakest, 3))
    return found


def check_lists(key):
    sc = scene(key)
    Ls = lists(key)
    seen, skipped, between = set(), 0, 0
    for b, per_plane in enumerate(Ls):
        want = [LIST_SEQS[b]] + ([LIST_SEQS_PLANE1[b]] if sc.kind == "asm" else [])
        assert len(per_plane) == len(want)
        for L, seqs in zip(per_plane, want):
            # no bbox leaves its tile, so every list is its sequence: label w touches sub-tile w alone, label 4 all four
            assert [int(n) for n in L["length"]] == [len(s) for s in seqs], (key, b, L["length"])
            for m, s in zip(L["masks"], seqs):
                assert [int(x) for x in m] == [15 if lab == 4 else 1 << lab for lab in s], (key, b)
                skipped += bool(len(s)) and int(np.bitwise_or.reduce(m)) != 15
            n = [int(x) for x in L["length"]]
            between += sum(1 for i in range(1, len(n) - 1) if n[i] == 0 and n[i - 1] and n[i + 1])
            seen |= set(n)
    assert seen >= LIST_LENGTHS and max(seen) > 320, sorted(seen)
    assert skipped >= 3 and between >= 1, (skipped, between)
    return dict(lengths=sorted(seen), lists_missing_a_subtile=skipped)


def seg_len_of(B, N, W, H):
    """FgsSavedLayout.seg_len of the plan under a splat renderer: the FgsDims of splat_base_dims (fgs_splat.h) -- no phase
    blending, one camera, every tuning field automatic"""
    from fresnel_amd import _binding as Bd
    return int(Bd.saved_layout(Bd.make_dims(B, N, W, H, max_radius=64.0, background=BG, num_cameras=1)).seg_len)


def check_seg128(key):
    sc = scene(key)
    assert len(sc.images) == SEG128_B and sc.images[0].arrs[0].shape[0] == SEG128_N
    assert seg_len_of(SEG128_B, SEG128_N, sc.W, sc.H) == 128  # B N > 200 000 ...
    assert seg_len_of(SEG128_B, 100000, sc.W, sc.H) == 64     # ... and not at 200 000
    seen = []
    for b, (per_plane, (r32, r64)) in enumerate(zip(lists(key), reference(key))):
        vis = r32["proj"]["visible"].astype(bool)
        assert np.array_equal(vis, ~sc.images[b].culled) and np.array_equal(r64["proj"]["visible"], r32["proj"]["visible"])
        assert (sc.images[b].arrs[0][~vis, 2] > 0).all()  # culled = behind the camera
        L = per_plane[-1]
        assert [int(n) for n in L["length"]] == [len(s) for s in SEG128_SEQS[b]]
        if sc.kind == "asm":
            assert not per_plane[0]["length"].any()
        seen += [int(n) for n in L["length"]]
        assert vis[0] and vis[-1]
    assert sorted(seen) == [127, 128, 129, 257]
    return dict(lengths=seen, visible=[int((~im.culled).sum()) for im in sc.images])


def check_onewave(key):
    sc = scene(key)
    tiles = (sc.W // 16) * (sc.H // 16)
    lists_in_call = len(sc.batch) * tiles
    src = open(os.path.join(ROOT, "fresnel_amd", "csrc", "fgs_splat.h")).read()
    assert int(re.search(r"ASM_ONE_WAVE_LISTS\s*=\s*(\d+)", src).group(1)) == ONE_WAVE_LISTS
    assert (lists_in_call >= ONE_WAVE_LISTS) == (len(sc.batch) == ONE_WAVE_B) and lists_in_call in (ONE_WAVE_LISTS, ONE_WAVE_LISTS - tiles)
    assert sc.batch == [b % 4 for b in range(len(sc.batch))]
    longest = [int(per_plane[0]["length"].max()) for per_plane in lists(key)]
    assert longest[3] > 128 and max(longest[:3]) <= 64, longest  # three chunks in one list of scene 3
    for r32, _ in reference(key):
        assert r32["proj"]["visible"].all()
    return dict(lists=lists_in_call, longest=longest)


def check_cameras(key):
    sc = scene(key)
    for c in sc.cams:
        assert c.fx != c.fy and abs(c.cx - sc.W / 2) >= 2 and abs(c.cy - sc.H / 2) >= 2 and not np.allclose(c.view, np.eye(4), atol=0.1)
    assert len(sc.cams) == (1 if "shared" in key else 3)
    used = set()
    for r32, r64 in reference(key):
        vis = r32["proj"]["visible"].astype(bool)
        assert vis.sum() >= 150 and np.array_equal(r64["proj"]["visible"], r32["proj"]["visible"])
        if sc.kind == "asm":
            assert np.array_equal(r32["plane_idx"][vis], r64["plane_idx"][vis])
            used |= set(int(p) for p in r32["plane_idx"][vis])
    if sc.kind == "wave":
        assert all(im.gD is not None and np.abs(im.gD).min() > 0 for im in sc.images)  # a depth-map gradient on every pixel
    else:
        assert len(used) >= 3, used
    return dict(planes=sorted(used), visible=[int(r["proj"]["visible"].sum()) for r, _ in reference(key)])


def check_planes(key):
    sc = scene(key)
    cfg = sc.asm
    assert sc.dropped == PLANES_DROPPED[sc.case], sc.dropped
    r32, r64 = reference(key)[0]
    assert r32["proj"]["visible"].all()
    depth = np.asarray(r32["proj"]["depth"], np.float32)
    assert np.array_equal(depth, -sc.images[0].arrs[0][:, 2]) and np.array_equal(r64["proj"]["depth"], depth.astype(np.float64))
    assert np.array_equal(r32["plane_idx"], r64["plane_idx"])  # both runs choose the same plane for every Gaussian
    assert np.array_equal(r32["plane_idx"], _nearest(depth, cfg, torch.float32))
    p = torch.linspace(cfg["depth_range"][0], cfg["depth_range"][1], cfg["num_planes"]).numpy()
    ties = 0
    for (w, k), d, got in zip(sc.what, depth, r32["plane_idx"]):
        if w in ("plane", "below", "above"):
            assert got == k, (w, k, got)
        elif w == "mid":
            tie = np.float32(abs(d - p[k])) == np.float32(abs(d - p[k + 1]))
            ties += bool(tie)
            assert got in (k, k + 1) and (not tie or got == k), (w, k, got)  # an exact tie: the first minimum
        else:
            assert got == (k if w == "mid-" else k + 1), (w, k, got)
    if sc.case == "a":
        assert ties == 3 * (cfg["num_planes"] - 1)  # every midpoint of case (a) is an exact tie in fp32
    assert set(r32["plane_idx"]) == set(range(cfg["num_planes"]))
    return dict(exact_ties=ties, gaussians=len(depth), dropped=sc.dropped)


def check_norm(key):
    sc = scene(key)
    r32, r64 = reference(key)[0]
    t32, t64 = r32["tasq"], r64["tasq"]
    found = dict(peak32=r32["peak"], peak64=r64["peak"], runner_up=r32["runner_up"], peak_count=r32["peak_count"],
                 tasq=(float(t32.min()), float(t32.max())), nearest_to_clamp=float(np.abs(t32 - 1.0).min()))
    assert any(b != 0 for b in BG)
    if sc.regime == "dim":
        assert r64["peak"] <= 0.8 and r32["peak"] <= 0.8, found
    else:
        for r in (r32, r64):
            assert r["peak"] >= 1.25 and r["runner_up"] <= 0.99 * r["peak"], found
            assert (r["tasq"] >= 1.1).any() and (r["tasq"] <= 0.9).any() and (np.abs(r["tasq"] - 1.0) > 1e-3).all(), found
        assert r32["peak_count"] == (3 if sc.regime == "tie" else 1), found
    return found


def check_placement(key):
    fam = key.split("-")[0]
    if fam == "lists":
        return check_lists(key)
    if fam == "seg128":
        return check_seg128(key)
    if fam.startswith("onewave"):
        return check_onewave(key)
    if fam.startswith("cameras"):
        return check_cameras(key)
    if fam.startswith("planes"):
        return check_planes(key)
    if fam.startswith("norm"):
        return check_norm(key)
    return check_membership(key)


# ---- the statement ----
def _err(name, x, ref):
    return float(np.abs(np.asarray(x, np.float64) - ref).max()) if name == "image" else rel_to_max(x, ref)


def _compared(sc, ref_j):
    """(name, fp32 reference, fp64 reference) of every per-image tensor the statement compares"""
    r32, r64 = ref_j
    out = [("image", r32["image"], r64["image"])]
    if sc.kind == "wave":
        out.append(("depth", r32["depth"], r64["depth"]))
    return out + [(k, r32["grad_" + k], r64["grad_" + k]) for k in GRADS]


def spreads(key):
    sc = scene(key)
    return {(j, name): _err(name, a32, a64) for j, ref_j in enumerate(reference(key)) for name, a32, a64 in _compared(sc, ref_j)}


def distances(key, got, ref=None, batch=None):
    """{(image of the scene, tensor): (distance, tolerance)}, the largest over the images of the call that repeat a scene image"""
    sc = scene(key)
    ref = reference(key) if ref is None else ref
    out = {}
    for b, j in enumerate(sc.batch if batch is None else batch):
        for name, a32, a64 in _compared(sc, ref[j]):
            x = got[name][b]
            if name in REFEREED.get(key, ()):
                want, tol, _ = referee(a32, a64)  # (the tolerance that helpers.assert_with_referee applies, and its verdict:)
                try:
                    err = assert_with_referee(x, a32, a64, f"{key} image {j} {name}")
                except AssertionError:
                    err = rel_to_max(x, want)  # refused: the distance from the run that referees (beyond the tolerance)
            else:
                err, tol = _err(name, x, a32), TOL
            out[j, name] = (max(err, out.get((j, name), (0.0, tol))[0]), tol)
    return out


def statement_fails(dist):
    return {k: v for k, v in dist.items() if not v[0] <= v[1]}


def wavelength_grad(key, got):
    """dL/dlambda is shared by the call: the sum over its images, judged by helpers.assert_wavelength_grad with the fp64 run"""
    sc = scene(key)
    want = sum(np.asarray(reference(key)[j][0]["grad_wavelengths"], np.float64) for j in sc.batch)
    want64 = sum(np.asarray(reference(key)[j][1]["grad_wavelengths"], np.float64) for j in sc.batch)
    return assert_wavelength_grad(got["wavelengths"], want, key, want64=want64)


@pytest.mark.parametrize("key", KEYS)
def test_placement(key):
    check_placement(key)


@pytest.mark.parametrize("key", KEYS)
def test_oracle_spread(key):
    """fp32 is an adequate reference on these scenes: the oracle's own fp32-fp64 spread is <= 5e-5 on every compared tensor, except
    for the (scene, tensor) pairs of REFEREED."""
    bad = {k: v for k, v in spreads(key).items() if not v <= SPREAD_MAX and k[1] not in REFEREED.get(key, ())}
    assert not bad, bad


def _as_got(rs):
    """oracle results of the images of a call in the layout of _hip's"""
    names = ["image"] + (["depth"] if "depth" in rs[0] else [])
    out = {k: np.stack([r[k] for r in rs]) for k in names}
    out.update({k: np.stack([r["grad_" + k] for r in rs]) for k in GRADS})
    return out


def test_statement_sees_a_seam_error():
    """The oracle with ONE seam error of each kind fails the statement (the unperturbed override reproduces the run)."""
    # a bbox edge of the residues scene one pixel out: the Gaussian with the most weight in the line of pixels beyond an edge
    for key in ("residues-64x32-wave", "residues-64x32-asm"):
        sc = scene(key)
        r32 = reference(key)[0][0]
        bb = _bb(r32)
        best = (0.0, None, None)
        for n in np.nonzero(r32["proj"]["visible"])[0]:
            x0, x1, y0, y1 = bb[n]
            for edge, box in ((0, (x0 - 1, x0, y0, y1)), (1, (x1, x1 + 1, y0, y1)), (2, (x0, x1, y0 - 1, y0)), (3, (x0, x1, y1, y1 + 1))):
                if 0 < bb[n, edge] < (sc.W, sc.H)[edge // 2]:
                    best = max(best, (float(sc.images[0].arrs[4][n]) * float(_G(r32["proj"], n, box).max()), int(n), edge))
        weight, n, edge = best
        moved = bb.copy()
        moved[n, edge] += 1 if edge % 2 else -1
        same = oracle_run(sc, 0, bbox=bb)
        assert np.array_equal(same["image"], r32["image"]) and np.array_equal(same["grad_colors"], r32["grad_colors"])
        dist = distances(key, _as_got([oracle_run(sc, 0, bbox=moved)]))
        print(key, "Gaussian", n, "edge", edge, "weight beyond it", weight, statement_fails(dist))
        assert statement_fails(dist), f"{key}: a bbox edge one pixel out went unnoticed"
    # entry 64 of a 65-entry list dropped (what a forward part or a backward unit one entry short does)
    for key in ("lists-64x32-wave", "lists-64x32-asm"):
        sc = scene(key)
        b, t = 0, 1
        L = lists(key)[b][0]
        assert L["length"][t] == 65
        n = int(L["ids"][t][64])
        r32 = reference(key)[b][0]
        assert tile_counts(_bb(r32)[n:n + 1])[0] == 1  # in this list alone
        dropped = _bb(r32).copy()
        dropped[n] = 0
        dist = distances(key, _as_got([oracle_run(sc, b, bbox=dropped)]), batch=[b])
        print(key, "Gaussian", n, statement_fails(dist))
        assert statement_fails(dist), f"{key}: a dropped list entry went unnoticed"
    # one Gaussian of the planes scenes on the neighbouring plane
    for key in ("planes_a-48x32-asm", "planes_b-48x32-asm"):
        sc = scene(key)
        r32 = reference(key)[0][0]
        n = [w for w, _ in sc.what].index("mid")  # a midpoint Gaussian: the first minimum k -> k + 1
        idx = r32["plane_idx"].copy()
        idx[n] += 1
        same = oracle_run(sc, 0, plane_idx=r32["plane_idx"])
        assert np.array_equal(same["image"], r32["image"])
        dist = distances(key, _as_got([oracle_run(sc, 0, plane_idx=idx)]))
        print(key, "Gaussian", n, statement_fails(dist))
        assert statement_fails(dist), f"{key}: a Gaussian on the neighbouring plane went unnoticed"
    # the maximum's gradient given to one of the three tied elements
    key = "norm_tie-64x32-wave"
    dist = distances(key, _as_got([oracle_run(scene(key), 0, max_to_first=True)]))
    print(key, statement_fails(dist))
    assert np.array_equal(oracle_run(scene(key), 0, max_to_first=True)["image"], reference(key)[0][0]["image"])
    assert statement_fails(dist), "the tie's share given to one element went unnoticed"


@gpu
@pytest.mark.parametrize("key", KEYS)
def test_scene_vs_oracle(key):
    check_placement(key)
    got = hip(key)
    dist = distances(key, got)
    print(key, {f"{j}:{n}": f"{e:.1e}/{t:.0e}" for (j, n), (e, t) in dist.items()})
    assert not statement_fails(dist), statement_fails(dist)
    if scene(key).kind == "asm":
        wavelength_grad(key, got)


@gpu
@pytest.mark.parametrize("key", KEYS)
def test_every_row_finite_and_culled_rows_zero(key):
    sc = scene(key)
    got = hip(key)
    for k in GRADS:
        assert np.isfinite(got[k]).all(), k
        for b, j in enumerate(sc.batch):
            assert not got[k][b, sc.images[j].culled].any(), (k, b)
    assert np.isfinite(got["image"]).all()
    if key.split("-")[0] in MEMBERSHIP + ["lists", "seg128"]:
        assert all(im.culled.sum() >= 2 for im in sc.images)


@gpu
@pytest.mark.parametrize("key", KEYS)
def test_scene_is_deterministic(key):
    first, again = hip(key), _hip(scene(key))
    for k in first:
        assert np.array_equal(first[k], again[k]), k


@gpu
@pytest.mark.parametrize("B", [ONE_WAVE_B, ONE_WAVE_B - 1])
def test_replicas_of_a_scene_are_bitwise_equal(B):
    """the 96 (95) images of the call that repeat one scene: every per-image tensor bit for bit that of the first of them"""
    key = f"onewave{B}-128x128-wave"
    got = hip(key)
    for k in ["image", "depth"] + GRADS:
        for b in range(4, B):
            assert np.array_equal(got[k][b], got[k][b % 4]), (k, b)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_batched_cameras_equal_single_calls(kind):
    """image b of the call with one camera per image is, bit for bit, the single-image call with camera b"""
    key = f"cameras_each-72x40-{kind}"
    sc = scene(key)
    got = hip(key)
    for b in range(3):
        one = _hip(Scene(kind, sc.W, sc.H, [sc.images[b]], cams=[sc.cams[b]], asm=sc.asm))
        for k in ["image"] + (["depth"] if kind == "wave" else []) + GRADS:
            assert np.array_equal(got[k][b], one[k][0]), (b, k)
