"""Zero sub-tiles of GENERAL units of k_composite_bwd (fgs_composite.hip; tuning key bwd_sub = the FGS_BWD_SUB_ON / _OFF flag of
FgsDims.fwd_variant; automatic follows bwd_zero, so every call here forces fwd_exit = 1 and bwd_zero = 1 and bwd_sub follows).

A unit with one live pixel takes the general walk.  Its 8 x 8 sub-tiles in which every in-frame lane restarts with T == +0 (by its
bits) and every lane holds S == +-0 leave the unit's `alive` mask: their passes would add exact zeros to sums that start at +0.  The
seven outputs are the same BITS either way, so what can go wrong is the PREDICATE -- a sub-tile with a residue or a NaN in S, or
with one live lane, taken for zero loses gradients -- and the bookkeeping of an entry whose mask becomes empty (it still stores its
row).  Every scene is therefore compared bitwise with the bwd_sub = -1 call, the bwd_zero = -1 call, a second run and two runs whose
whole scratch buffer was filled with NaN bits / zeros in front of the backward; image, depth and gradients pass the referee
against the C oracle; and a numpy restatement of the kernel's prologue over the call's OWN saved state (checkpoints, fwd_close,
pix_state) and the upstream gradients counts the (general unit, sub-tile) pairs the predicate takes out -- a scene meant to mask
something fails when that count is zero, a scene meant to mask nothing in some sub-tile fails when it is in the set.

Scenes.  Flat saturating GROUPS of 24 entries (sigma 200 px, bbox radius capped at 64: alpha >= 0.75 inside the bbox, T <= 4e-15
behind a group -- tests/test_blend_bwd_dead_units.py) whose bbox is a rectangle anchored at the frame's borders, a crowd of 190 small
Gaussians inside ONE tile behind them, 30 more all over the frame, six anchors in the far corner.
  sub        one 8 x 8 sub-tile of the crowded tile saturated by the frontmost group, its neighbours open; the crowd behind holds
             entries that touch ONLY the zero sub-tile (their mask is empty, the row is still stored), entries that touch it and a live
             one, and entries that touch only live ones -- counted from the oracle's bboxes, each kind at least once.  On 40 x 24 the
             crowded tile is the frame's last tile of row 0: partly out of frame.
  h0first    32 x 16: half 0 saturated by the frontmost group, half 1 by a second group ONE SEGMENT later;  h1first: the reverse.
  h0open     half 0 saturated, half 1 never: the list ends with one half open beside a closed one.
  residue    the `zero` scene of tests/test_blend_bwd_zero_units.py: T == 0 without a closing.
  gzero      `sub` with the upstream gradients exactly zero on a LIVE sub-tile: S == +-0 there, T != 0 -- it stays.
  nan / inf  a NaN / an Inf upstream gradient on a pixel of the saturated sub-tile: S is NaN there, the sub-tile stays.
  infzero    every colour's red channel exactly 0 and an Inf red gradient on such a pixel: Inf x 0 = NaN in S, the sub-tile stays.
  twin       opacity 0.05: nothing saturates.  batch: `sub` and its twin in ONE call -- the same tile differs between the images.
  A unit of segment 0 is never masked (T = 1 on every lane; the kernel does not even look), and the capacity overflow runs under
  tests/workspace_guard.py's fills with the switch on and off.

CPU half: the predicate on hand-made states (a residue, a NaN, a -0 in T, lanes outside the frame), a numpy model of one entry's
sums with the +-0 terms of masked sub-tiles left out against all terms -- bit for bit as the source states them (sums from +0), and
for the form the compiler gives the first pass of a sub-tile row (the sum is ASSIGNED, so it can hold -0) equal up to the sign of
an exact zero per row and bit for bit behind k_row_sum's accumulation from +0 --, and the flag pair with the plan's rule."""
import functools

import numpy as np
import pytest
import torch

import test_blend_bwd_dead_units as D
import test_blend_bwd_zero_units as Z
import test_blend_fwd_close_slot as CS  # noqa: F401  (the closing-slot rule the prologue model follows is stated and tested there)
from helpers import assert_with_referee

GRADS, OUTS = Z.GRADS, Z.OUTS
FRAMES = [(64, 32), (40, 24)]
SEGS = {"s64": dict(seg_len=64), "s128": dict(seg_len=128)}
N_FRONT, N_CROWD, N_REST, N_ANCHOR = D.N_FRONT, D.N_CROWD, D.N_REST, D.N_ANCHOR
BAD_AT = (3, 2)  # pixel of the saturated sub-tile, relative to its origin, that carries the NaN / Inf gradient
gpu = pytest.mark.gpu
f32 = np.float32


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def _origin(name, W, H, tile_w):
    """the crowded tile's origin: tile 0, but for the `sub` family on 40 x 24 the last tile of row 0 (partly out of frame)"""
    if name in ("sub", "gzero", "nan", "inf", "infzero", "twin") and (W, H) == (40, 24):
        return (-(-W // tile_w) - 1) * tile_w, 0
    return 0, 0


def _crowded_tile(name, W, H, tile_w):
    X0, Y0 = _origin(name, W, H, tile_w)
    return (Y0 // 16) * -(-W // tile_w) + X0 // tile_w


def _rect_mean(rect, W, H):
    """mean (u, v) of a capped-radius Gaussian whose clipped bbox is rect = (x0, x1, y0, y1); every side either lies on the frame's
    border or is set by the cap: trunc(u - 64) = x0 with x1 clipped, or trunc(u + 64) + 1 = x1 with x0 clipped"""
    def axis(lo, hi, size):
        if lo <= 0 and hi >= size:
            return size / 2.0
        if lo <= 0:
            assert hi <= 2 * D.RCAP
            return hi - D.RCAP - 0.5
        assert hi >= size and size <= lo + 2 * D.RCAP + 1
        return lo + D.RCAP + 0.5
    return axis(rect[0], rect[1], W), axis(rect[2], rect[3], H)


def _groups(name, W, H, tile_w, seg_len):
    """[(first list position, rectangle)] of the saturating groups"""
    X0, Y0 = _origin(name, W, H, tile_w)
    if name in ("sub", "gzero", "nan", "inf", "infzero", "twin"):
        # sub-tile 0 of the crowded tile: x in [X0, X0 + 8) -- from the frame's left border, or up to its right one --, y in [0, 8)
        return [(0, (0, 8, 0, 8) if X0 == 0 else (X0, W, 0, 8))]
    lo, hi = (0, 16, 0, H), (16, W, 0, H)
    if name == "h0first":
        return [(0, lo), (seg_len, hi)]
    if name == "h1first":
        return [(0, hi), (seg_len, lo)]
    if name == "h0open":
        return [(0, lo)]
    raise AssertionError(name)


@functools.lru_cache(maxsize=None)
def _scene(name, W, H, tile_w, seg_len):
    """-> (the five arrays, gI, gD).  Item 0 is frontmost; list position = index in the crowded tile for groups and crowd."""
    if name == "residue":
        arrs, gI, gD, _ = Z._scene("zero", W, H, tile_w)
        return [a.copy() for a in arrs], gI, gD
    rs = np.random.RandomState(7100 + W + 3 * tile_w)
    X0, Y0 = _origin(name, W, H, tile_w)
    cw, ch = min(16, W - X0), min(16, H - Y0)
    n_list = N_FRONT + N_CROWD
    u = X0 + rs.uniform(1.2, cw - 1.2, n_list)
    v = Y0 + rs.uniform(1.2, ch - 1.2, n_list)
    sig = rs.uniform(1.0, 1.8, n_list) / 3.0  # pixel sigma of the crowd
    flat = np.zeros(n_list, bool)
    for first, rect in _groups(name, W, H, tile_w, seg_len):
        gu, gv = _rect_mean(rect, W, H)
        sl = slice(first, first + N_FRONT)
        u[sl], v[sl], sig[sl], flat[sl] = gu + rs.uniform(-0.2, 0.2, N_FRONT), gv + rs.uniform(-0.2, 0.2, N_FRONT), D.SIGMA, True
    ru, rv, rsig = rs.uniform(0.0, W, N_REST), rs.uniform(0.0, H, N_REST), rs.uniform(2.0, 5.0, N_REST) / 3.0
    ax, ay = (3.5, H - 3.5) if X0 else (W - 3.5, H - 3.5)  # the corner away from the crowded tile
    au, av = ax + rs.uniform(-0.5, 0.5, N_ANCHOR), ay + rs.uniform(-0.5, 0.5, N_ANCHOR)
    asig = rs.uniform(2.0, 2.5, N_ANCHOR) / 3.0
    u, v, sig = np.r_[u, ru, au], np.r_[v, rv, av], np.r_[sig, rsig, asig]
    flat = np.r_[flat, np.zeros(N_REST + N_ANCHOR, bool)]
    N = len(u)
    z = -2.0 - 0.004 * np.arange(N)
    z[N - N_ANCHOR:] = -1.9 - 0.004 * np.arange(N_ANCHOR)
    s = sig * -z / D.FOCAL
    th = rs.uniform(0.0, np.pi, N)
    pos = np.stack([(u - W / 2) * -z / D.FOCAL, -(v - H / 2) * -z / D.FOCAL, z], 1).astype(f32)
    scale = np.stack([s, np.where(flat, 1.0, 0.6) * s, 1e-3 * s], 1).astype(f32)
    quat = np.stack([np.cos(th / 2), 0 * th, 0 * th, np.sin(th / 2)], 1).astype(f32)
    color = (0.2 + 0.7 * rs.random_sample((N, 3))).astype(f32)
    opacity = np.full(N, 0.8, f32)
    gI = rs.standard_normal((3, H, W)).astype(f32)
    gD = (rs.standard_normal((H, W)) * 0.1).astype(f32) + f32(0.05)
    bx, by = X0 + BAD_AT[0], Y0 + BAD_AT[1]
    if name == "twin":
        opacity[:] = 0.05
    if name == "gzero":  # a LIVE sub-tile (row 1 of column 0: in frame on both frames) without any upstream gradient
        gI[:, Y0 + 8:Y0 + 16, X0:X0 + 8] = 0.0
        gD[Y0 + 8:Y0 + 16, X0:X0 + 8] = 0.0
    if name == "nan":
        gI[1, by, bx] = np.nan
    if name == "inf":
        gD[by, bx] = np.inf
    if name == "infzero":
        color[:, 0] = 0.0
        gI[0, by, bx] = np.inf
    return [pos, scale, quat, color, opacity], gI, gD


@functools.lru_cache(maxsize=None)
def _reference(name, W, H, tile_w, seg_len):
    from oracle import fgs_oracle as orc
    arrs, gI, gD = _scene(name, W, H, tile_w, seg_len)
    ocam = Z._ocam(W, H)
    r32 = orc.render(*arrs, ocam, bg=D.BG)
    g32 = orc.render_backward(r32, gI, gD)
    with orc.fp64():
        r64 = orc.render(*arrs, ocam, bg=D.BG)
        g64 = orc.render_backward(r64, gI, gD)
    return r32, g32, r64, g64


# ---- the kernel's prologue and predicate, restated in numpy ------------------------------------------------------------------------
def _fma(a, b, c):
    """fp32 fma through float64: the product of two floats is exact there"""
    with np.errstate(all="ignore"):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def zero_subtile(T, S, inframe):
    """composite_bwd_zero_subtiles for one sub-tile: no in-frame lane whose T is not +0 BY ITS BITS, no lane whose S is not +-0"""
    tb, sb = np.asarray(T, f32).view(np.uint32), np.asarray(S, f32).view(np.uint32)
    return not (((tb != 0) & inframe) | ((sb & np.uint32(0x7FFFFFFF)) != 0)).any()


def predicted_masks(sv, gI, gD, W, H):
    """{(image, tile, seg): (kind, set of zero sub-tiles)} for every unit of segment >= 1, from the call's saved state: kind is
    'dead' (every in-frame pixel restarts at T == 0: not this path's) or 'general'.  composite_bwd_prologue, term for term."""
    tile_w, seg_len, parts = sv["tile_w"], sv["seg_len"], sv["parts"]
    nsx = tile_w // 8
    ns, PL = 2 * nsx, 2 * nsx * 64
    SLOT = 5 * PL
    ck, ps = sv["ckpt"], sv["pix_state"]
    Bn, Tn = sv["ranges"].shape[:2]
    bg = [f32(x) for x in D.BG]
    ly, lx = np.divmod(np.arange(64), 8)

    def load(slot, s):
        o = slot * SLOT + s * 64
        c = [ck[o + p * PL:o + p * PL + 64] for p in range(5)]
        return dict(Cr=c[0], Cg=c[1], Cb=c[2], T=(f32(1.0) - c[3]).astype(f32), D=c[4])

    def chain(g, st):
        return _fma(g[3], st["D"], _fma(g[2], st["Cb"], _fma(g[1], st["Cg"], (g[0] * st["Cr"]).astype(f32))))

    out = {}
    with np.errstate(all="ignore"):
        for b in range(Bn):
            for t in range(Tn):
                lo, hi = sv["ranges"][b, t]
                nseg = -(-int(hi - lo) // seg_len)
                base = int(sv["seg_off"][b * Tn + t])
                X0, Y0 = (t % sv["tiles_x"]) * tile_w, (t // sv["tiles_x"]) * 16
                for seg in range(1, nseg):
                    rebase = seg
                    if parts > 1:
                        spp = -(-nseg // parts)
                        first = seg // spp * spp
                        if first != 0:
                            rebase = first
                    Ts, Ss, ins = [], [], []
                    for s in range(ns):
                        px, py = X0 + 8 * (s % nsx) + lx, Y0 + 8 * (s // nsx) + ly
                        inf_ = (px < W) & (py < H)
                        qx, qy = np.minimum(px, W - 1), np.minimum(py, H - 1)
                        fin = dict(Cr=ps[b, 0, qy, qx], Cg=ps[b, 1, qy, qx], Cb=ps[b, 2, qy, qx], D=ps[b, 4, qy, qx])
                        Tf = (f32(1.0) - ps[b, 3, qy, qx]).astype(f32)
                        g = []
                        for c in range(3):
                            p = (fin[("Cr", "Cg", "Cb")[c]] + Tf * bg[c]).astype(f32)
                            g.append(np.where((p >= 0) & (p <= 1), gI[b, c, qy, qx], f32(0)).astype(f32))
                        g.append(gD[b, qy, qx].astype(f32))
                        g = [np.where(inf_, x, f32(0)).astype(f32) for x in g]
                        bgs = _fma(g[2], bg[2], _fma(g[1], bg[1], (g[0] * bg[0]).astype(f32)))
                        S = np.where(inf_, _fma(bgs, Tf, chain(g, fin)), f32(0)).astype(f32)
                        k = -1 if sv["fwd_close"] is None else int(sv["fwd_close"][b, t, (s % nsx) >> 1])
                        behind = 0 <= k <= seg
                        st = load(base + (k if behind else seg), s)
                        if rebase != seg and not behind:
                            a = load(base + rebase, s)
                            st = dict(Cr=_fma(a["T"], st["Cr"], a["Cr"]), Cg=_fma(a["T"], st["Cg"], a["Cg"]), Cb=_fma(a["T"], st["Cb"], a["Cb"]),
                                      T=(a["T"] * st["T"]).astype(f32), D=_fma(a["T"], st["D"], a["D"]))
                        Ts.append(st["T"]); Ss.append((S - chain(g, st)).astype(f32)); ins.append(inf_)
                    live = any(((Ts[s] != 0) & ins[s]).any() for s in range(ns))
                    zero = {s for s in range(ns) if zero_subtile(Ts[s], Ss[s], ins[s])}
                    out[(b, t, seg)] = ("general" if live else "dead", zero)
    return out


def _touched(bbox, X0, Y0, tile_w):
    """the sub-tiles of the tile at (X0, Y0) that a bbox (x0, x1, y0, y1) touches"""
    nsx = tile_w // 8
    return {r * nsx + c for r in range(2) for c in range(nsx)
            if bbox[0] < X0 + 8 * c + 8 and bbox[1] > X0 + 8 * c and bbox[2] < Y0 + 8 * r + 8 and bbox[3] > Y0 + 8 * r}


# ---- GPU half ----------------------------------------------------------------------------------------------------------------------
def _run(arrs, W, H, gI, gD, tuning, batch=False, poison=None):
    """one forward + backward -> (the seven outputs, the saved state the prologue model reads).  `poison`: the 32-bit word the
    WHOLE scratch buffer of the backward is filled with in front of it."""
    from fresnel_amd import _binding as B
    from fresnel_amd import renderer as R
    dev = D._cuda()
    if not batch:
        arrs, gI, gD = [a[None] for a in arrs], gI[None], gD[None]
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True) for a in arrs]
    ren = R.TileBasedRenderer(W, H, background=D.BG)
    ren.tuning = dict(tuning)
    img, dep = ren(*ts, R.Camera(D.FOCAL, D.FOCAL, W / 2, H / 2, W, H), return_depth=True)
    dims, raw = img.grad_fn.dims, img.grad_fn.saved_tensors[-1]
    st = R.inspect_saved(raw, dims)
    L = st["layout"]
    slot = 5 * 2 * (int(L.tile_w) // 8) * 64
    num = lambda t: t.cpu().numpy().astype(np.int64)  # noqa: E731
    counters = num(st["counters"])
    saved = dict(ranges=num(st["ranges"]), seg_off=num(st["seg_off"]), seg_len=int(L.seg_len), tile_w=int(L.tile_w),
                 tiles_x=int(L.tiles_x), counters=counters, parts=int(counters[5]) if int(counters[5]) > 1 else 0,
                 fwd_close=num(st["fwd_close"]) if "fwd_close" in st else None, pix_state=st["pix_state"].cpu().numpy(),
                 ckpt=raw[L.seg_ckpt:L.seg_ckpt + int(counters[2]) * slot * 4].view(torch.float32).cpu().numpy())
    scratch_bytes = B.workspace_bytes(dims)[1]
    if poison is not None:
        R._scratch_for(dev, scratch_bytes)[:scratch_bytes].view(torch.int32).fill_(poison)
    ((img * torch.from_numpy(gI).to(dev)).sum() + (dep * torch.from_numpy(gD).to(dev)).sum()).backward()
    out = {k: t.grad.detach().cpu().numpy() for k, t in zip(GRADS, ts)}
    out["image"], out["depth"] = img.detach().cpu().numpy(), dep.detach().cpu().numpy()
    if not batch:
        out = {k: v[0] for k, v in out.items()}
    return out, saved


def _check_bits(arrs, W, H, gI, gD, tuning, what, batch=False):
    got, saved = _run(arrs, W, H, gI, gD, tuning, batch)
    for off in (dict(bwd_sub=-1), dict(bwd_zero=-1)):
        Z._same_bits(got, _run(arrs, W, H, gI, gD, dict(tuning, **off), batch)[0], f"{what} against {off}:")
    Z._same_bits(got, _run(arrs, W, H, gI, gD, tuning, batch)[0], what + " second run:")
    for word in (0x7FC00000, 0):
        Z._same_bits(got, _run(arrs, W, H, gI, gD, tuning, batch, poison=word)[0], f"{what} scratch filled with {word:#x}:")
    return got, saved


# (scene, tile widths, frames, segment lengths)
GRID = [("sub", (16, 32), FRAMES, ("s64", "s128")),
        ("h0first", (32,), FRAMES, ("s64", "s128")), ("h1first", (32,), FRAMES, ("s64", "s128")), ("h0open", (32, 16), FRAMES, ("s64",)),
        ("residue", (16, 32), [(64, 32)], ("s64",)), ("gzero", (16, 32), [(64, 32)], ("s64",)), ("gzero", (32,), [(40, 24)], ("s128",)),
        ("nan", (16, 32), [(64, 32)], ("s64",)), ("nan", (32,), [(40, 24)], ("s128",)),
        ("inf", (16, 32), [(64, 32)], ("s64",)), ("inf", (16,), [(40, 24)], ("s128",)),
        ("infzero", (16, 32), [(64, 32)], ("s64",)), ("infzero", (32,), [(40, 24)], ("s64",)),
        ("twin", (32,), [(64, 32)], ("s64",))]
CASES = [(n, tw, fr, sg) for n, tws, frs, sgs in GRID for tw in tws for fr in frs for sg in sgs]


@gpu
@pytest.mark.parametrize("name,tile_w,frame,seg", CASES, ids=lambda c: c if isinstance(c, str) else (f"{c[0]}x{c[1]}" if isinstance(c, tuple) else str(c)))
def test_scene_bitwise_referee_and_predicted_masks(name, tile_w, frame, seg):
    W, H = frame
    seg_len = SEGS[seg]["seg_len"]
    arrs, gI, gD = _scene(name, W, H, tile_w, seg_len)
    tuning = dict(tile_w=tile_w, fwd_exit=1, bwd_zero=1, **SEGS[seg])
    what = f"{name} {W}x{H} tile_w={tile_w} {seg}"
    got, saved = _check_bits(arrs, W, H, gI, gD, tuning, what)
    assert saved["seg_len"] == seg_len and saved["tile_w"] == tile_w, what
    r32, g32, r64, g64 = _reference(name, W, H, tile_w, seg_len) if name != "residue" else Z._reference("zero", W, H, tile_w)
    assert_with_referee(got["image"], r32.image, r64.image, f"{what} image")
    assert_with_referee(got["depth"], r32.depth, r64.depth, f"{what} depth")
    if name in ("nan", "inf", "infzero"):
        assert not all(np.isfinite(got[k]).all() for k in GRADS), what  # the bad gradient arrived
    else:
        for k in GRADS:
            assert_with_referee(got[k], g32[k], g64[k], f"{what} grad_{k}")
    # ---- what the predicate takes out, from the call's own saved state ----
    masks = predicted_masks(saved, gI[None], gD[None], W, H)
    assert all(seg_ >= 1 for (_, _, seg_) in masks)  # a unit of segment 0 is never masked: T = 1, the kernel does not look
    general = {k: z for k, (kind, z) in masks.items() if kind == "general"}
    pairs = sum(len(z) for z in general.values())
    print(f"{what}: {len(masks)} units behind segment 0, {len(general)} general, {pairs} (general unit, zero sub-tile) pairs")
    if name == "residue":
        return
    ct = _crowded_tile(name, W, H, tile_w)
    X0, Y0 = _origin(name, W, H, tile_w)
    mine = {seg_: z for (b, t, seg_), z in general.items() if t == ct}
    nsx = tile_w // 8
    inframe_subs = {s for s in range(2 * nsx) if X0 + 8 * (s % nsx) < W and Y0 + 8 * (s // nsx) < H}
    if name == "twin":
        assert pairs == 0 and masks and len(general) == len(masks), what  # nothing saturates: every unit general, nothing zero
        return
    if name == "h0open" and tile_w == 16:
        # 16 x 16 tiles: the saturated half IS tile 0, whose later units are dead (not this path's); no other tile has a later unit
        assert not mine and pairs == 0 and all(kind == "dead" for kind, _ in masks.values()), (what, masks)
        return
    assert mine, f"{what}: the crowded tile has no general unit behind segment 0"
    if name in ("sub", "gzero"):
        assert all(0 in z for z in mine.values()), (what, mine)  # the saturated sub-tile is zero in every later unit
        assert all(not (z & inframe_subs - {0}) for z in mine.values()), (what, mine)  # and no in-frame neighbour is
        if name == "gzero":
            assert all(nsx not in z for z in mine.values()), (what, mine)  # S == 0 without T == 0 is not enough
        # the three kinds of entries behind the first segment, from the oracle's bboxes (list position = index in the crowded tile)
        bbox = r32.proj["bbox"]
        kinds = {"only": 0, "both": 0, "live": 0}
        for j in range(seg_len, N_FRONT + N_CROWD):
            tch = _touched(bbox[j], X0, Y0, tile_w) & inframe_subs
            if tch:
                kinds["only" if tch == {0} else ("both" if 0 in tch else "live")] += 1
        assert min(kinds.values()) >= 1, (what, kinds)
    if name in ("nan", "inf", "infzero"):
        assert all(0 not in z for z in mine.values()), (what, mine)  # S is NaN on one lane: the sub-tile stays
        assert not any(z & inframe_subs for z in mine.values()), (what, mine)
    if name in ("h0first", "h1first", "h0open"):
        half0 = {s for s in range(2 * nsx) if (s % nsx) < 2}
        first = half0 if name != "h1first" else set(range(2 * nsx)) - half0
        assert 1 in mine and mine[1] & inframe_subs == first & inframe_subs, (what, mine)  # the unit behind the first group: one half zero
        if name == "h0open":
            assert all(z & inframe_subs == first & inframe_subs for z in mine.values()), (what, mine)
        k = saved["fwd_close"][0, ct]
        print(f"{what}: fwd_close of the crowded tile {k.tolist()}")
        assert pairs > 0, what
    if name in ("sub", "gzero"):
        assert pairs > 0, what


@gpu
@pytest.mark.parametrize("seg", sorted(SEGS))
@pytest.mark.parametrize("tile_w", [16, 32])
def test_two_images_whose_same_tile_differs(tile_w, seg):
    """`sub` and its opacity-0.05 twin in ONE call: image 0 masks the sub-tile, image 1 does not; each is bit-equal to its single call"""
    W, H = 64, 32
    seg_len = SEGS[seg]["seg_len"]
    a, gI, gD = _scene("sub", W, H, tile_w, seg_len)
    b = _scene("twin", W, H, tile_w, seg_len)[0]
    tuning = dict(tile_w=tile_w, fwd_exit=1, bwd_zero=1, **SEGS[seg])
    stack = [np.stack([x, y]) for x, y in zip(a, b)]
    gI2, gD2 = np.stack([gI, gI]), np.stack([gD, gD])
    both, saved = _check_bits(stack, W, H, gI2, gD2, tuning, f"batch {tuning}", batch=True)
    masks = predicted_masks(saved, gI2, gD2, W, H)
    per_image = [sum(len(z) for (b_, _, _), (kind, z) in masks.items() if b_ == i and kind == "general") for i in range(2)]
    assert per_image[0] > 0 and per_image[1] == 0, per_image
    for i, arrs in enumerate((a, b)):
        single = _run(arrs, W, H, gI, gD, tuning)[0]
        for k in OUTS:
            assert both[k][i].tobytes() == single[k].tobytes(), (tuning, i, k)


@gpu
@pytest.mark.parametrize("tuning", [dict(tile_w=32, seg_len=64, fwd_exit=1, bwd_zero=1), dict(tile_w=16, seg_len=128, fwd_variant=1, fwd_exit=1, bwd_zero=1)],
                         ids=["tw32-seg64", "tw16-seg128-v1"])
def test_capacity_overflow_under_the_guard_fills(tuning):
    """every list empty: no unit exists, no prologue reads a fill -- switch on and off"""
    import test_workspace_capacity as C
    import workspace_guard as WG
    Dn = C._oracle_duplicates("aniso", tuning["tile_w"])
    inp = C._inputs()
    for extra in (dict(bwd_sub=1), dict(bwd_sub=-1)):
        call = C._Call(inp, workspace=Dn // 4, tuning=dict(tuning, **extra))
        runs = WG.run_patterns(call, inp, C._mods())
        assert int(call.layout.dup_capacity) == Dn // 4
        for name, out in runs.items():
            assert int(out["st_counters"][1]) == 1 and int(out["st_list_len"].abs().sum()) == 0, name
            for k in ("image", "depth"):
                assert bool((out[k].view(torch.int32) == C.QNAN).all()), (name, k)
            for k in [g for g in out if g.startswith("grad_")]:
                assert not bool(out[k].view(torch.int32).any()), (name, k)


# ---- CPU half ----------------------------------------------------------------------------------------------------------------------
def test_cpu_predicate_on_hand_made_states():
    z, one = np.zeros(64, f32), np.ones(64, f32)
    inside = np.ones(64, bool)
    assert zero_subtile(z, z, inside)
    assert zero_subtile(z, -z, inside)                                   # S == -0 is a zero
    S = z.copy(); S[17] = f32(1e-30)
    assert not zero_subtile(z, S, inside)                                # a residue, however small
    S[17] = f32(1e-45)
    assert S[17] != 0 and not zero_subtile(z, S, inside)                 # a denormal is not a zero (integer test)
    S[17] = np.nan
    assert not zero_subtile(z, S, inside)                                # a NaN is not a zero
    T = z.copy(); T[5] = f32(2.0 ** -60)
    assert not zero_subtile(T, z, inside)                                # one live lane
    T[5] = f32(-0.0)
    assert not zero_subtile(T, z, inside)                                # T == -0 is not +0 by its bits: it vetoes (the safe side)
    T[5] = np.nan
    assert not zero_subtile(T, z, inside)
    half = np.arange(64) % 8 < 4                                         # lanes outside the frame carry T = 1, S = +0: no veto
    assert zero_subtile(np.where(half, z, one), z, half)
    assert not zero_subtile(np.where(half, z, one), z, inside)
    assert zero_subtile(one, z, np.zeros(64, bool))                      # a sub-tile wholly outside the frame
    S = z.copy(); S[63] = f32(3.0)
    assert not zero_subtile(np.where(half, z, one), S, half)             # S vetoes on EVERY lane


def _entry_rows(nsx, touched, masked, a1, S, T, q, g, dx, dya, assign_first):
    """One list entry's ten per-lane sums as the general walk forms them (fgs_composite.hip, `pass` and the fold), for 64 lanes.
    a1, S, T, q [ns][64], g [ns][4][64], dx [nsx][64], dya [64].  Sub-tiles in `masked` run no pass.  assign_first: the compiled form of
    a sub-tile row's FIRST pass (s = 0 and s = nsx), which ASSIGNS the row's sums where the source adds to +0."""
    ns = 2 * nsx
    dyb = (dya + f32(8.0)).astype(f32)
    zero = np.zeros(64, f32)
    mA, mB, mC = [zero.copy(), zero.copy()], [zero.copy(), zero.copy()], [zero.copy(), zero.copy()]
    col = [zero.copy() for _ in range(4)]
    S, T = [x.copy() for x in S], [x.copy() for x in T]
    R = f32(1.0) / f32(0.99)
    with np.errstate(all="ignore"):
        for s in range(ns):
            if s not in touched or s in masked:
                continue
            row, c = s // nsx, s % nsx
            w = (a1[s] * T[s]).astype(f32)
            S[s] = _fma(-w, q[s], S[s])
            r = (f32(1.0) / (a1[s] - R).astype(f32)).astype(f32)
            dalpha = _fma(q[s], T[s], (S[s] * r).astype(f32))
            T[s] = _fma(w, f32(-0.99), T[s])
            dG = (dalpha * a1[s]).astype(f32)
            dmx = (dG * dx[c]).astype(f32)
            first = assign_first and c == 0
            mA[row] = dG if first else _fma(dalpha, a1[s], mA[row])
            mB[row] = dmx if first else _fma(dG, dx[c], mB[row])
            mC[row] = (dmx * dx[c]).astype(f32) if first else _fma(dmx, dx[c], mC[row])
            for i in range(4):
                col[i] = (w * g[s][i]).astype(f32) if (assign_first and s == 0) else _fma(w, g[s][i], col[i])
        t0, t1 = (dya * mA[0]).astype(f32), (dyb * mA[1]).astype(f32)
        vals = [(mB[0] + mB[1]).astype(f32), _fma(mA[1], dyb, t0), (mC[0] + mC[1]).astype(f32), _fma(mB[1], dyb, (mB[0] * dya).astype(f32)),
                _fma(t1, dyb, (t0 * dya).astype(f32)), (mA[0] + mA[1]).astype(f32)] + col
        tot = []
        for v in vals:  # the wave's total: a fixed order of additions (the order does not matter for what is stated below)
            x = v[0]
            for lane in range(1, 64):
                x = f32(x + v[lane])
            tot.append(x)
    return np.asarray(tot, f32)


def _row_sum(rows):
    """k_row_sum's accumulation: moments in float64, colour / depth sums in float32, all from +0"""
    m, c = np.zeros(6, np.float64), np.zeros(4, f32)
    for r in rows:
        m = m + r[:6].astype(np.float64)
        c = (c + r[6:]).astype(f32)
    return m.tobytes() + c.tobytes()


@pytest.mark.parametrize("nsx", [2, 4])
def test_cpu_entry_sums_without_the_zero_terms(nsx):
    """entries over a unit with zero sub-tiles (T = +0, S = +-0) and live ones: leaving the zero sub-tiles' passes out changes no bit
    of the rows as the source states them; in the compiled form only the sign of an exact zero, which k_row_sum's sums absorb"""
    ns = 2 * nsx
    rs = np.random.RandomState(5 + nsx)
    zero_subs = {0, nsx} if nsx == 2 else {0, 1, 4, 5}
    seen_neg_first, seen_sign_only = False, False
    for trial in range(40):
        T = [np.zeros(64, f32) if s in zero_subs else rs.uniform(0.0, 1.0, 64).astype(f32) for s in range(ns)]
        S = [np.where(rs.random_sample(64) < 0.5, f32(0.0), f32(-0.0)).astype(f32) if s in zero_subs else rs.standard_normal(64).astype(f32) for s in range(ns)]
        g = [[(rs.standard_normal(64) * (-1 if trial % 2 else 1)).astype(f32) for _ in range(4)] for _ in range(ns)]
        if trial % 4 == 1:  # every gradient negative on the zero sub-tiles: T q = -0 on every lane, dalpha = -0 - (+0 r) = -0 first
            for s in zero_subs:
                g[s] = [-np.abs(x) for x in g[s]]
                S[s] = np.zeros(64, f32)
        cq = rs.uniform(0.2, 0.9, 4).astype(f32)
        q = [_fma(g[s][3], cq[3], _fma(g[s][2], cq[2], _fma(g[s][1], cq[1], (g[s][0] * cq[0]).astype(f32)))) for s in range(ns)]
        a1 = [rs.uniform(0.0, 1.0, 64).astype(f32) * (rs.random_sample(64) < 0.8) for _ in range(ns)]  # (a' = 0 outside the bbox)
        a1 = [x.astype(f32) for x in a1]
        u, v = f32(rs.uniform(-3, 8 * nsx + 3)), f32(rs.uniform(-12, 28))  # centres above, inside and below the tile: dya, dyb of both signs
        ly, lx = np.divmod(np.arange(64), 8)
        dx = [(lx.astype(f32) + f32(8 * c) - u).astype(f32) for c in range(nsx)]
        dya = (ly.astype(f32) - v).astype(f32)
        touched = set(range(ns)) if trial % 3 else zero_subs | {ns - 1}
        if trial % 5 == 2:
            touched = set(zero_subs)  # an entry whose mask becomes empty: it still parks ten sums and stores its row
        for assign in (False, True):
            full = _entry_rows(nsx, touched, set(), a1, S, T, q, g, dx, dya, assign)
            lean = _entry_rows(nsx, touched, zero_subs, a1, S, T, q, g, dx, dya, assign)
            if not assign:
                assert full.tobytes() == lean.tobytes(), (nsx, trial, full, lean)
            else:
                assert np.array_equal(full, lean), (nsx, trial, full, lean)  # equal as numbers: at most the sign of an exact zero
                seen_sign_only |= full.tobytes() != lean.tobytes()
                other = rs.standard_normal((3, 10)).astype(f32)
                assert _row_sum([full] + list(other)) == _row_sum([lean] + list(other))
                assert _row_sum([full]) == _row_sum([lean])  # a Gaussian with this one row: +0 + (-0) = +0
        if touched == zero_subs and trial % 4 == 1:
            seen_neg_first = True
    assert seen_neg_first  # the -0 first addend was among the trials
    assert seen_sign_only  # ... and the compiled form does show the sign the sums absorb


def test_cpu_switch_is_a_flag_of_fwd_variant_and_follows_bwd_zero():
    from fresnel_amd import _binding as B
    kw = dict(batch=2, num_gaussians=100, width=64, height=32)
    d = B.make_dims(**kw, tuning=dict(bwd_sub=-1, fwd_variant=2, fwd_exit=1, bwd_zero=1))
    assert d.fwd_variant == 2 | B.FWD_EXIT_ON | B.BWD_ZERO_ON | B.BWD_SUB_OFF
    assert B.make_dims(**kw, tuning=dict(bwd_sub=1)).fwd_variant == B.BWD_SUB_ON
    assert B.make_dims(**kw).fwd_variant == 0
    assert not (B.BWD_SUB_OFF | B.BWD_SUB_ON) & (B.FWD_EXIT_OFF | B.FWD_EXIT_ON | B.BWD_ZERO_OFF | B.BWD_ZERO_ON | B.BWD_TAIL_OFF | B.BWD_TAIL_ON | 0x1F)
    # the switch changes no layout and no workspace size, whatever bwd_zero is
    for zero in (1, -1, 0):
        sizes = {(B.workspace_bytes(dd), B.saved_layout(dd).total_bytes, B.saved_layout(dd).unit_order)
                 for dd in (B.make_dims(**kw, tuning=dict(tile_w=32, fwd_exit=1, bwd_zero=zero, bwd_sub=s)) for s in (0, 1, -1))}
        assert len(sizes) == 1, (zero, sizes)
    for bad in (dict(bwd_sub=2), dict(bwd_sub=-2), dict(bwd_sub=1, fwd_variant=-1), dict(bwd_sub=-1, fwd_variant=-2)):
        with pytest.raises(B.FgsError):
            B.make_dims(**kw, tuning=bad)
    both = B.make_dims(**kw)
    both.fwd_variant = B.BWD_SUB_ON | B.BWD_SUB_OFF  # both flags at once: refused by the plan
    with pytest.raises(B.FgsError):
        B.workspace_bytes(both)
    unknown = B.make_dims(**kw)
    unknown.fwd_variant = 0x20000
    with pytest.raises(B.FgsError):
        B.workspace_bytes(unknown)
