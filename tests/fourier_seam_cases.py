"""Scenes of tests/test_fourier_seams.py: the Fourier renderer on the boundaries its kernels cut at (fgs_fourier.hip,
k_fourier_project): the closed-interval clamps, the `m > 1e-8` normalisation switch, arg-max ties, the strided fold of more than
256 per-tile maxima, several tiles per image of a batch, frames on and one over the 32 / 64 tile edges, the six visibility bounds.
Every scene is built by code and judged against the dense torch checker (tests/fourier_checker.py, tie="lowest").

Two devices make the seams exact:
  * the EXACT CAMERA: identity view, fx = fy a power of two, cx, cy and the depth powers of two (or small integers): a Gaussian at
    ((px - cx) / fx z, -(py - cy) / fy z, -z) projects to the integer pixel (px, py) with every product exact, in fp32 and fp64;
  * DELTA Gaussians: scale 1e-4 x 64 / fx under that camera gives s ~ 8e-5 and exp(-1 / s) == 0: the Gaussian adds colour x opacity
    to ONE pixel and nothing to any other, so F, the maximum, its index, d and pre are known by hand.

A case is a dict: images (a list of scenes in the layout of fourier_cases: arrs, view, intr, W, H, bg, gI), family, and the facts
its tests assert (hand values of F, the arg-max index, the culled rows, ...).  Checker runs are computed once and shared."""
import functools

import numpy as np
import torch

import fourier_checker as fc
from fourier_cases import MIN_GAP
from helpers import synth_aniso, upstream_grads

EYE = np.eye(4, dtype=np.float32)
FT = 64          # forward tile edge of k_fourier_fwd
MAX_TRIES = 5    # reseeding bound of the random scenes
F32 = np.float32


def exact_intr(f, cx, cy, near=0.5, far=100.0):
    return (float(f), float(f), float(cx), float(cy), float(near), float(far))


def at_pixel(px, py, intr, depth=1.0):
    """Position that the exact camera projects to pixel (px, py) at `depth`."""
    fx, fy, cx, cy = intr[:4]
    return [(px - cx) / fx * depth, -(py - cy) / fy * depth, -depth]


def deltas(items, intr):
    """Delta Gaussians: items = [(px, py, colour, opacity)] -> the five arrays."""
    n = len(items)
    pos = np.array([at_pixel(px, py, intr) for px, py, _, _ in items], F32)
    scale = np.full((n, 3), 1e-4 * 64.0 / intr[0], F32)
    quat = np.tile(np.array([1, 0, 0, 0], F32), (n, 1))
    color = np.array([c for _, _, c, _ in items], F32)
    opacity = np.array([o for _, _, _, o in items], F32)
    return [pos, scale, quat, color, opacity]


def hand_image(items, W, H):
    """The un-normalised image of delta Gaussians, by hand: colour x opacity (one fp32 product) on their pixels."""
    Fh = np.zeros((3, H, W), F32)
    for px, py, c, o in items:
        Fh[:, py, px] += np.array(c, F32) * F32(o)
    return Fh


def wide(n, seed, centre, spread, smin, smax, opacity_max, depth=1.0):
    """n wide anisotropic Gaussians with random rotations around `centre` (world x, y) at `depth`."""
    pos, scale, quat, color, opacity = synth_aniso(n, seed, opacity_max=opacity_max, spread=spread, zmean=0.0, smin=smin, smax=smax)
    pos[:, 0] += centre[0]
    pos[:, 1] += centre[1]
    pos[:, 2] = -depth
    return [pos, scale, quat, color, opacity]


def cat(*sets):
    return [np.concatenate([s[i] for s in sets]).astype(F32) for i in range(5)]


def flat_index(c, px, py, W, H):
    return c * W * H + py * W + px


def tile_of(index, W, H):
    pix = index % (W * H)
    return (pix // W) // FT * ((W + FT - 1) // FT) + (pix % W) // FT


def one_pixel_gI(px, py, W, H, values=(0.75, -0.5, 1.25)):
    g = np.zeros((3, H, W), F32)
    g[:, py, px] = values
    return g


def _scene(arrs, intr, W, H, bg, gI, view=EYE):
    return dict(arrs=arrs, view=np.asarray(view, F32), intr=intr, W=W, H=H, bg=[float(b) for b in bg], gI=gI)


# ---- 1. closed-interval clamps ------------------------------------------------------------------------------------------------
CLAMP_W, CLAMP_H, CLAMP_BG = 64, 32, (1.0, 0.25, 0.5)
CLAMP_INTR = exact_intr(64, 32, 16)
# name -> (px, py, colour, opacity); what the pixel holds after normalisation by m = 1 (pixel A) under CLAMP_BG
CLAMP_ITEMS = {
    "A": (3, 2, (1.0, 0.0, 0.0), 1.0),        # the maximum; d == 0 and pre_r == 1
    "B": (40, 5, (0.5, 0.5, 0.0), 1.0),       # d == 0 exactly (and pre_b == 0)
    "C": (10, 20, (0.5, 0.0, 0.0), 1.0),      # d = 0.5, pre_r = 0.5 + 1 x 0.5 == 1 exactly
    "D": (50, 30, (0.0, -0.25, 0.0), 1.0),    # d = 1.25: the inner clamp blocks; pre_g = -0.25 + 0.25 x 1 == 0 exactly
    "Z": (20, 10, (0.5, 0.25, 0.75), 0.0),    # opacity 0: the pixel is empty, d == 1 exactly, and dL/dopacity sees its gradient
    "E": (33, 17, (0.5, -0.25, 0.0), 1.0),    # d = 0.75, pre_r = 1.25 > 1, pre_g = -0.0625 < 0
    "G": (63, 31, (0.25, 0.0, -0.125), 2.0),  # opacity above 1: F = (0.5, 0, -0.25), d = 0.75, pre_r = 1.25 > 1
}
CLAMP_PIXELS = dict({k: v[:2] for k, v in CLAMP_ITEMS.items()}, none=(0, 0))  # "none": no Gaussian at all, every gradient zero
CLAMP_KEYS = ["clamp-" + k for k in list(CLAMP_PIXELS) + ["dense"]]


def _clamp_case(which):
    items = list(CLAMP_ITEMS.values())
    W, H = CLAMP_W, CLAMP_H
    gI = upstream_grads(9700, H, W)[0] if which == "dense" else one_pixel_gI(*CLAMP_PIXELS[which], W, H)
    return dict(family="clamp", images=[_scene(deltas(items, CLAMP_INTR), CLAMP_INTR, W, H, CLAMP_BG, gI)],
                hand=[hand_image(items, W, H)], m=[1.0], index=[flat_index(0, 3, 2, W, H)])


# ---- 2. normalisation switch --------------------------------------------------------------------------------------------------
NORM_AT = F32(1e-8)                               # m == 1e-8f: NOT normalised (the test is m > 1e-8f)
NORM_ABOVE = np.nextafter(NORM_AT, F32(1.0))      # one ulp above: normalised
NORM_KEYS = ["norm-at", "norm-above", "norm-at-bg", "norm-above-bg"]


def _norm_case(which):
    W, H, intr = 64, 32, exact_intr(64, 32, 16)
    op = NORM_ABOVE if "above" in which else NORM_AT
    items = [(5, 7, (1.0, 0.5, 0.25), op)]
    bg = (0.2, 0.3, 0.1) if which.endswith("bg") else (0.0, 0.0, 0.0)
    return dict(family="norm", images=[_scene(deltas(items, intr), intr, W, H, bg, upstream_grads(9710, H, W)[0])],
                hand=[hand_image(items, W, H)], m=[float(op)], index=[flat_index(0, 5, 7, W, H)],
                normalised="above" in which, single=True)


# ---- 3. arg-max ties ----------------------------------------------------------------------------------------------------------
RED, GREY, BLUE = (1.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 0.0, 1.0)
# key -> (W, H, f, cx, cy, items, (channel, px, py) of the expected arg-max)
TIES = {
    # one grey Gaussian: a tie of the three channels, the index is the pixel in channel 0
    "tie-grey": (64, 32, 64, 32, 16, [(37, 21, GREY, 1.0)], (0, 37, 21)),
    # rows 4-7 of a 32 x 32 quarter sit in lanes 32-63 of its wave, rows 8-11 in lanes 0-31: the lower index in the UPPER half-wave
    "tie-halfwave": (64, 32, 64, 32, 16, [(20, 10, RED, 1.0), (3, 5, RED, 1.0)], (0, 3, 5)),
    # wave 1 (columns 32-63, rows 0-31) holds the lower index, wave 0 the higher one
    "tie-waves": (64, 64, 64, 32, 32, [(5, 10, RED, 1.0), (40, 3, RED, 1.0)], (0, 40, 3)),
    # 130 x 70 is 3 x 2 tiles: tile 2 (scheduled after tile 0) holds the lower index; and the reverse
    "tie-tiles-late-low": (130, 70, 128, 64, 32, [(5, 1, RED, 1.0), (129, 0, RED, 1.0)], (0, 129, 0)),
    "tie-tiles-early-low": (130, 70, 128, 64, 32, [(129, 1, RED, 1.0), (5, 0, RED, 1.0)], (0, 5, 0)),
    # channel 0 beats channel 2 whatever the pixels: blue in tile 0, red in the last tile; and both in one wave
    "tie-channels-tiles": (130, 70, 128, 64, 32, [(2, 1, BLUE, 1.0), (129, 69, RED, 1.0)], (0, 129, 69)),
    "tie-channels-wave": (64, 32, 64, 32, 16, [(2, 1, BLUE, 1.0), (9, 30, RED, 1.0)], (0, 9, 30)),
}
TIE_KEYS = list(TIES)


def _tie_case(key):
    W, H, f, cx, cy, items, (c, px, py) = TIES[key]
    intr = exact_intr(f, cx, cy)
    return dict(family="tie", images=[_scene(deltas(items, intr), intr, W, H, (0.1, 0.2, 0.3), upstream_grads(9720, H, W)[0])],
                hand=[hand_image(items, W, H)], m=[1.0], index=[flat_index(c, px, py, W, H)],
                single=len(items) == 1, normalised=True)


# ---- 4. more than 256 tiles ---------------------------------------------------------------------------------------------------
MANY_W = MANY_H = 1025                      # 17 x 17 = 289 tiles of 64 x 64: the fold's second strided trip
MANY_INTR = exact_intr(1024, 512, 512)
# key -> (items of the deltas, (channel, px, py) of the maximum)
MANY = {
    "many-tile288": ([(1024, 1024, (1.0, 0.5, 0.25), 1.0), (3, 5, (0.5, 1.0, 0.25), 0.6)], (0, 1024, 1024)),
    "many-tile259-blue": ([(300, 1000, (0.25, 0.5, 1.0), 1.0), (1024, 1024, (1.0, 0.5, 0.25), 0.6)], (2, 300, 1000)),
}
MANY_KEYS = list(MANY)


def _many_case(key):
    items, (c, px, py) = MANY[key]
    W, H = MANY_W, MANY_H
    # two wide Gaussians (sigma ~ 100-200 pixels), dim, so that position, scale and rotation gradients are non-zero
    wides = wide(2, 9730, (-0.1, 0.05), 0.2, 0.1, 0.2, 0.3)
    return dict(family="many", images=[_scene(cat(deltas(items, MANY_INTR), wides), MANY_INTR, W, H, (0.1, 0.2, 0.3),
                                              upstream_grads(9731, H, W)[0])],
                index=[flat_index(c, px, py, W, H)], tile=[tile_of(flat_index(c, px, py, W, H), W, H)])


# ---- 5. a batch with several tiles per image ----------------------------------------------------------------------------------
BATCH_W, BATCH_H = 130, 70                  # 3 x 2 tiles
BATCH_INTR = exact_intr(128, 64, 32)
BATCH_BLOBS = [((129, 69), 1.5), ((128, 10), 0.7), ((20, 66), 1.2)]  # (pixel under the identity view, opacity): tiles 5, 2, 3
BATCH_KEYS = ["batch-1cam", "batch-3cams"]


def batch_views(cameras):
    views = [EYE.copy() for _ in range(3)]
    if cameras == 3:  # whole pixels (1 / 128 of a world unit at depth 1), so that the blobs stay centred on a pixel
        views[1][0, 3] = 1.0 / 128
        views[2][1, 3] = -2.0 / 128
    return views


def _batch_case(key):
    W, H = BATCH_W, BATCH_H
    views = batch_views(3 if key == "batch-3cams" else 1)
    images = []
    for b, ((px, py), op) in enumerate(BATCH_BLOBS):
        blob = [np.array([at_pixel(px, py, BATCH_INTR)], F32), np.full((1, 3), 0.02, F32), np.array([[1, 0, 0, 0]], F32),
                np.array([[1.0, 0.6, 0.3][b:] + [1.0, 0.6, 0.3][:b]], F32), np.array([op], F32)]
        images.append(_scene(cat(wide(7, 9740 + b, (0.0, 0.0), 0.25, 0.05, 0.2, 0.3), blob), BATCH_INTR, W, H, (0.1, 0.2, 0.3),
                             upstream_grads(9745 + b, H, W)[0], view=views[b]))
    return dict(family="batch", images=images, tile=[5, 2, 3])


# ---- 6. tile and chunk edges ---------------------------------------------------------------------------------------------------
# (W, H, N, hand-placed arg-max pixel or None): frames on a 32 / 64 multiple, one over, one-pixel frames; N at and around the
# 32-Gaussian chunk of both kernels
EDGES = [(1, 1, 33, None), (1, 70, 32, None), (70, 1, 64, None), (32, 32, 33, None), (31, 33, 32, None), (64, 64, 64, None),
         (63, 65, 33, (30, 64)),    # the arg-max in the one-pixel-high last row of the edge tiles
         (65, 63, 32, (64, 31)),    # ... in the one-pixel-wide last column
         (129, 65, 64, None), (96, 33, 33, None)]
EDGE_KEYS = [f"edge-{w}x{h}-n{n}" for w, h, n, _ in EDGES]


def edge_intr(W, H):
    f = 0.8 * max(W, H, 16)
    return (f, f, W / 2, H / 2, 0.01, 100.0)


def edge_scene(W, H, N, place, seed):
    """Wide anisotropic Gaussians as fourier_cases.small_scene, spread over the frame's own aspect (a 1-pixel-wide frame culls
    everything beyond -W < u < 2W); with `place`, Gaussian 0 is a bright narrow one on that pixel."""
    arrs = list(synth_aniso(N, seed, opacity_max=1.0, spread=0.35, zmean=-2.0, smin=0.02, smax=0.12))
    side = max(W, H, 16)
    arrs[0][:, 0] *= W / side
    arrs[0][:, 1] *= H / side
    intr = edge_intr(W, H)
    if place is not None:
        arrs[0][0] = at_pixel(place[0], place[1], intr, depth=2.0)
        arrs[1][0] = 0.03
        arrs[3][0] = (1.0, 0.3, 0.2)
        arrs[4][0] = 24.0  # tops the sum of the wide ones (test_placement checks where the arg-max is)
    return _scene(arrs, intr, W, H, (0.1, 0.2, 0.3), upstream_grads(9760 + N, H, W)[0])


@functools.lru_cache(maxsize=None)
def edge_seed(W, H, N, place):
    """-> (scene, tries): reseeded until the arg-max gap is at least MIN_GAP, at most MAX_TRIES times."""
    for t in range(MAX_TRIES):
        s = edge_scene(W, H, N, place, 9750 + 7 * N + W + 1000 * t)
        with torch.no_grad():
            raw = fc.render(*[torch.from_numpy(a) for a in s["arrs"]], s["view"], s["intr"], W, H)[1]
        if fc.argmax_gap(raw) >= MIN_GAP:
            return s, t + 1
    raise AssertionError(f"no seed with an arg-max gap of {MIN_GAP} in {MAX_TRIES} tries: {W}x{H} N={N}")


def _edge_case(key):
    W, H, N, place = EDGES[EDGE_KEYS.index(key)]
    s, tries = edge_seed(W, H, N, place)
    return dict(family="edge", images=[s], tries=tries, place=place)


# ---- 7. visibility bounds -----------------------------------------------------------------------------------------------------
VIS_W, VIS_H = 64, 32
VIS_INTR = exact_intr(64, 32, 16, near=1.0, far=4.0)
# bound -> position ON it: u = 32 x + 32 and v = -32 y + 16 at depth 2; depth = -z.  One ulp inside: nextafter towards `inward`.
VIS_BOUNDS = {
    "u_lo": ((-3.0, 0.25, -2.0), 0, 0.0),      # u == -W
    "u_hi": ((3.0, 0.25, -2.0), 0, 0.0),       # u == 2W
    "v_lo": ((0.25, 1.5, -2.0), 1, 0.0),       # v == -H
    "v_hi": ((0.25, -1.5, -2.0), 1, 0.0),      # v == 2H
    "near": ((0.125, 0.0625, -1.0), 2, -2.0),  # depth == near
    "far": ((0.5, -0.25, -4.0), 2, 0.0),       # depth == far
}
VIS_KEYS = ["vis-" + k for k in VIS_BOUNDS] + ["vis-all-on-bounds"]


def vis_gaussians(positions, seed):
    n = len(positions)
    _, _, quat, color, _ = synth_aniso(n, seed)
    scale = np.tile(np.array([2.0, 1.5, 1.0], F32), (n, 1))  # sigma ~ W at depth 2: one just inside 2W still reaches the frame
    return [np.array(positions, F32), scale, quat, 0.25 + 0.75 * color, np.full(n, 0.8, F32)]


def inside(bound):
    p, axis, inward = VIS_BOUNDS[bound]
    q = np.array(p, F32)
    q[axis] = np.nextafter(q[axis], F32(inward))
    return q


def _vis_case(key):
    W, H = VIS_W, VIS_H
    gI = upstream_grads(9770, H, W)[0]
    if key == "vis-all-on-bounds":
        arrs = vis_gaussians([p for p, _, _ in VIS_BOUNDS.values()], 9771)
        return dict(family="vis", images=[_scene(arrs, VIS_INTR, W, H, (1.5, 0.25, -0.25), gI)], culled=list(range(6)))
    bound = key[4:]
    # Gaussian 0 ON the bound, 1 one ulp inside it (same colour, scale, rotation, opacity), 2 in the middle of the frame
    arrs = vis_gaussians([VIS_BOUNDS[bound][0], inside(bound), (0.1, -0.05, -2.0)], 9772)
    for a in arrs[1:]:
        a[1] = a[0]
    return dict(family="vis", images=[_scene(arrs, VIS_INTR, W, H, (0.1, 0.2, 0.3), gI)], culled=[0], bound=bound)


def nonfinite_scenes():
    """(scene with a NaN and a +Inf position next to three visible Gaussians, the same scene without those two, their rows)."""
    W, H = VIS_W, VIS_H
    arrs = vis_gaussians([(0.1, -0.05, -2.0), (0.0, 0.0, -2.0), (-0.6, 0.2, -1.5), (0.0, 0.0, -2.0), (0.7, 0.1, -3.0)], 9773)
    arrs[0][1, 1] = np.nan
    arrs[0][3, 0] = np.inf
    keep = [0, 2, 4]
    gI = upstream_grads(9774, H, W)[0]
    return (_scene(arrs, VIS_INTR, W, H, (0.1, 0.2, 0.3), gI), _scene([a[keep] for a in arrs], VIS_INTR, W, H, (0.1, 0.2, 0.3), gI),
            keep, [1, 3])


# ---- registry ------------------------------------------------------------------------------------------------------------------
FAMILIES = {"clamp": CLAMP_KEYS, "norm": NORM_KEYS, "tie": TIE_KEYS, "many": MANY_KEYS, "batch": BATCH_KEYS, "edge": EDGE_KEYS,
            "vis": VIS_KEYS}
KEYS = [k for ks in FAMILIES.values() for k in ks]


@functools.lru_cache(maxsize=None)
def case(key):
    fam = key.split("-")[0]
    build = dict(clamp=lambda: _clamp_case(key[6:]), norm=lambda: _norm_case(key), tie=lambda: _tie_case(key),
                 many=lambda: _many_case(key), batch=lambda: _batch_case(key), edge=lambda: _edge_case(key),
                 vis=lambda: _vis_case(key))[fam]
    return build()


def run_checker(s, f64, **kw):
    return fc.render_with_grads(s["arrs"], s["view"], s["intr"], s["W"], s["H"], s["bg"], s["gI"],
                                dtype=torch.float64 if f64 else torch.float32, tie="lowest", **kw)


@functools.lru_cache(maxsize=None)
def reference(key):
    """Per image of the case: (fp32 run, fp64 run) of the checker with tie="lowest", each (image, raw, [five gradients]); computed
    once per process and shared read-only."""
    return [(run_checker(s, False), run_checker(s, True)) for s in case(key)["images"]]


def tile_maxima(raw, W, H):
    """What k_fourier_fwd leaves per 64 x 64 tile, in tile order: (maximum, its flat index in (3, H, W); ties: the lowest)."""
    out = []
    idx = np.arange(3 * H * W).reshape(3, H, W)
    for y0 in range(0, H, FT):
        for x0 in range(0, W, FT):
            v, i = raw[:, y0:y0 + FT, x0:x0 + FT].reshape(-1), idx[:, y0:y0 + FT, x0:x0 + FT].reshape(-1)
            top = v.max()
            out.append((float(top), int(i[v == top].min())))
    return out


def inspect_fourier_saved(img, B, N, W, H):
    """What fgs_fourier_forward left in `saved` (layout: include/fgs.h; each part on a 256-byte step), read from the autograd
    graph of a FourierGaussianRenderer output BEFORE its backward: the binding keeps `saved` as the last saved tensor.
    -> rec (B, N, 8) float32, visible (B, N) uint32, F (B, 3, H, W), m (B,) float32, index (B,) uint32."""
    todo, node = [img.grad_fn], None
    while todo:
        f = todo.pop()
        if type(f).__name__ == "FourierRendererBackward":
            node = f
            break
        todo += [n for n, _ in f.next_functions if n is not None]
    assert node is not None, "no FourierRenderer node in the graph"
    raw = node.saved_tensors[-1].cpu().numpy()
    assert raw.dtype == np.uint8

    def step(x):
        return (x + 255) & ~255
    o_F = step(B * N * 8 * 4)
    o_scal = step(o_F + B * 3 * H * W * 4)
    assert raw.size == step(o_scal + B * 2 * 4), (raw.size, o_scal)
    rec = raw[:B * N * 32].view(F32).reshape(B, N, 8)
    scal = raw[o_scal:o_scal + B * 8].view(F32).reshape(B, 2)
    return dict(rec=rec, visible=rec[:, :, 6].copy().view(np.uint32), F=raw[o_F:o_F + B * 3 * H * W * 4].view(F32).reshape(B, 3, H, W),
                m=scal[:, 0].copy(), index=scal[:, 1].copy().view(np.uint32))
