"""Dead work units of k_composite_bwd (fgs_composite.hip): a unit (tile, depth segment) all of whose in-frame pixels restart with
T == 0.0f (the forward's accumulated alpha rounded to 1.0f) walks its list with a pass that leaves out every term that is an exact
zero there (w, q, the S and T updates, the colour / depth sums); every other unit takes the general walk.  The rows, and with them
every output, are the same bits either way, so what can go wrong is the PREDICATE: a unit with one live pixel taken for dead loses
that pixel's colour and geometry gradients.  The scenes put the live pixels where a predicate is most easily wrong.

Geometry.  Saturating GROUPS of N_FRONT = 24 entries each, frontmost in every list: sigma = 200 pixels with the bbox radius capped
at max_radius = 64, so inside its bbox a group member has G >= 0.94 and alpha >= 0.75 -- behind a whole group T <= 0.25^24 = 4e-15 --
and its bbox is a half-plane of the frame (x < X, x >= X, y < Y, y >= Y; x >= 0 for the whole frame).  Behind them N_CROWD = 190 small
Gaussians with their means inside ONE tile (the crowded tile: list position = index there, on 16 x 16 and on 32 x 16 tiles), every
sixth of them a PROBE centred in the scene's open region, 30 more all over the frame, and six ANCHORS in front of everything in the
far corner of the frame (in none of the crowded tile's lists: they give every tensor a maximum of ordinary size).  Depth segments of 64 and 128 entries;
fwd_variant 1, 2 and automatic: with 2 parts and segments of 64 the crowded tile's segment 1 is part-local without re-basing (part
0), segment 2 is a part's first (absolute) and segment 3 is re-based -- all three restart forms.

Every scene first asserts its dead / live pattern on the CPU (check_scene), from the oracle's projection and orc.tile_lists, by an
fp32 emulation of T at the segment boundaries, WITH MARGIN: a dead pixel has T < 2^-40, a live one T > 2^-20 (or is untouched), a
unit is dead (all in-frame pixels dead), live (one live pixel) or ambiguous -- and no unit of any scene is ambiguous, so the pattern
cannot depend on the kernel's own rounding.

Families:
  dead        one whole-frame group (x >= 0): every later unit of every tile restarts dead.  grad_colors of the Gaussians that lie wholly in
              dead units is EXACTLY zero (also with the general walk: w = a' * 0).  The crowded tile's last chunk is partial.
  col / row   the group's bbox stops one pixel column (row) short of the crowded tile's edge, probes stand in it: every unit of the
              crowded tile behind the group is live through that column alone, and every such unit holds a probe whose reference
              grad_colors is >= 1e-2 of max (the probes shadow one another: the smallest of them holds 1e-3 ... 2e-2).
  sub@p       the same with the 8 x 8 sub-tile p of the crowded tile left open by up to three half-plane groups (4 / 8 positions).
  seam@K      a column scene whose open column is closed by a second group G2 whose LAST entry is list position K = 63, 64, 65 (the
              boundary of 64-entry segments) or 127, 128: the unit behind the boundary restarts dead although up to two entries of
              the saturating group lie inside it.  seamin@64: G2 BEGINS at the boundary -- the unit restarts live and goes dead
              inside, the next one restarts dead: the predicate belongs to the restart.  (One entry scales T by >= 0.01 = 2^-6.6 and
              the margins are 2^-20 apart: no single entry can flip a restart with margin, so the seams move a whole group.)
  edge        the crowd in the last tile of the frame -- partial on 40 x 24 -- whose in-frame pixels are dead and whose out-of-frame
              lanes keep T = 1.
  flags in a dead unit: clamp@150 (opacity 0.995 on a pixel centre), op0@150 (opacity 0: the floored lop), bigdg (the first and last
              entries of every dead unit at either segment length -- positions 64, 127, 128, 191, 192, 213 -- are the largest of the crowd:
              deferred-reduction seams).
  batch       two images in one call, the dead scene and the same geometry at opacity 0.05 (no unit dead): bit-equal to the two
              single calls.

Statement for every scene: image, depth and the five gradients pass assert_with_referee against the C oracle (fp32 and fp64 runs);
each scene run twice is bitwise equal (in the same test).

CPU half (no GPU): the emulation with a CHANGED predicate.  "T < 2^-20 counts as dead" changes the pattern of no scene -- that is what
the margin is for; "lanes outside the frame veto" turns the partial tiles' dead units of `edge` live, and "the part-local state
instead of the re-based one" the re-based segment of `dead` (fwd_variant 2): the scenes tell those predicates from the kernel's, but
both err on the safe side -- a dead unit sent down the general walk computes the same bits, only slower -- so no gradient statement
can fail for them.  The predicate that can lose gradients is one that overlooks live lanes; `overlooks the open region` sends the
col / row / sub units down the dead walk, and the colour gradients that walk leaves out there are >= 10 x the tolerance (1e-3 of max)."""
import functools

import numpy as np
import pytest
import torch

from helpers import assert_with_referee

GRADS = ["positions", "scales", "rotations", "colors", "opacities"]
BG = (0.05, 0.1, 0.15)
FOCAL = 51.2
FRAMES = [(64, 32), (40, 24)]
TILE_WS = [16, 32]
TUNINGS = {"s64": dict(seg_len=64), "s64v1": dict(seg_len=64, fwd_variant=1), "s64v2": dict(seg_len=64, fwd_variant=2),
           "s128": dict(seg_len=128)}
N_FRONT, N_CROWD, N_REST, N_ANCHOR = 24, 190, 30, 6
SIGMA, RCAP = 200.0, 64.0
T_DEAD, T_LIVE = np.float32(2.0 ** -40), np.float32(2.0 ** -20)
CENTRE = (8, 8)
SCENES = (["dead", "col", "row"] + [f"sub@{p}" for p in range(8)] + [f"seam@{k}" for k in (63, 64, 65, 127, 128)]
          + ["seamin@64", "edge", "clamp@150", "op0@150", "bigdg"])
CASES = [(n, w) for n in SCENES for w in TILE_WS if not (n.startswith("sub@") and int(n[4:]) >= 4 and w == 16)]
BIGDG_AT = (64, 127, 128, 191, 192, 213)  # 213 = the crowded tile's last list entry in `bigdg` (24 + 190 entries)


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _arg(name):
    return int(name.split("@")[1]) if "@" in name else None


def _crowded_origin(name, W, H, tile_w):
    if name != "edge":
        return 0, 0
    return (-(-W // tile_w) - 1) * tile_w, (-(-H // 16) - 1) * 16


def _open_rect(name, tile_w):
    """the region of the crowded tile that the front groups leave untouched: (x0, x1, y0, y1), or None"""
    fam = name.split("@")[0]
    if fam in ("col", "seam", "seamin"):
        return tile_w - 1, tile_w, 0, 16
    if fam == "row":
        return 0, tile_w, 15, 16
    if fam == "sub":
        p, nsx = _arg(name), tile_w // 8
        c, r = p % nsx, p // nsx
        return 8 * c, 8 * c + 8, 8 * r, 8 * r + 8
    return None


def _groups(name, tile_w):
    """the saturating groups in front of the crowd, each a half-plane of the frame: (axis, side, X) = pixels with x < X ('lo') or
    x >= X ('hi') along the axis"""
    rect = _open_rect(name, tile_w)
    if rect is None:
        return [("x", "hi", 0)]  # the whole frame, as the half-plane x >= 0: mean beside the frame like every other group's
    x0, x1, y0, y1 = rect
    g = []
    if y0 > 0:
        g.append(("y", "lo", y0))
    if y1 < 16:
        g.append(("y", "hi", y1))
    if x0 > 0:
        g.append(("x", "lo", x0))
    if name.startswith("sub@") and x1 < tile_w:  # (only groups that reach into the crowded tile: list position = index there)
        g.append(("x", "hi", x1))
    return g


def _n_front(name):
    """entries per saturating group: 21 where up to three groups stand in front (63 entries: no boundary of a 64-entry segment
    falls inside them; 0.25^21 = 2e-13 is still below 2^-40), 24 elsewhere"""
    return 21 if name.startswith("sub@") else N_FRONT


def _group_mean(g, W, H):
    """mean (u, v) of a capped-radius Gaussian whose bbox is the group's half-plane: trunc(u - 64) = X resp. trunc(u + 64) + 1 = X"""
    u, v = W / 2.0, H / 2.0
    if g[0] == "all":
        return u, v
    m = g[2] + RCAP + 0.5 if g[1] == "hi" else g[2] - RCAP - 0.5
    return (m, v) if g[0] == "x" else (u, m)


@functools.lru_cache(maxsize=None)
def _scene(name, W, H, tile_w, opacity_all=None):
    """Flat Gaussians turned about the viewing axis, item 0 frontmost (the construction of test_blend_bwd_clamp_free._scene).
    Returns the five arrays, the upstream gradients and the probes' indices."""
    rs = np.random.RandomState(9300 + W)
    X0, Y0 = _crowded_origin(name, W, H, tile_w)
    cw, ch = min(tile_w, W - X0, 16), min(16, H - Y0)  # the crowd stays in the part of the tile that both tile shapes share
    groups = _groups(name, tile_w)
    rect = _open_rect(name, tile_w)
    u, v, r, op, kind = [], [], [], [], []
    for g in groups:
        gu, gv = _group_mean(g, W, H)
        for _ in range(_n_front(name)):
            u.append(gu + rs.uniform(-0.2, 0.2)); v.append(gv + rs.uniform(-0.2, 0.2)); r.append(3 * SIGMA); op.append(0.8); kind.append("front")
    n_front = len(u)
    crowd_u = X0 + rs.uniform(1.5, cw - 1.5, N_CROWD)
    crowd_v = Y0 + rs.uniform(1.5, ch - 1.5, N_CROWD)
    crowd_r = rs.uniform(1.0, 1.8, N_CROWD)
    for j in range(N_CROWD):
        if rect is not None and j % 6 == 0:  # a probe: on a pixel centre of the open region
            u.append(float(rs.randint(rect[0], rect[1]))); v.append(float(rs.randint(rect[2], rect[3]))); r.append(2.5)
            kind.append("probe")
        else:
            u.append(crowd_u[j]); v.append(crowd_v[j]); r.append(crowd_r[j]); kind.append("crowd")
        op.append(0.8)
    fam, k = name.split("@")[0], _arg(name)
    if fam in ("seam", "seamin"):  # G2 closes the open column: the half-plane x >= tile_w - 1, at list positions first .. first + 23
        first = k - N_FRONT + 1 if fam == "seam" else k
        gu, gv = _group_mean(("x", "hi", tile_w - 1), W, H)
        for j in range(first, first + N_FRONT):
            u[j], v[j], r[j], kind[j] = gu + rs.uniform(-0.2, 0.2), gv + rs.uniform(-0.2, 0.2), 3 * SIGMA, "front2"
    if fam == "clamp":
        u[k], v[k], r[k], op[k] = X0 + CENTRE[0], Y0 + CENTRE[1], 3.0, 0.995
    if fam == "op0":
        u[k], v[k], r[k], op[k] = X0 + CENTRE[0], Y0 + CENTRE[1], 3.0, 0.0
    if fam == "bigdg":
        for j in BIGDG_AT:
            u[j], v[j], r[j] = X0 + CENTRE[0] + 0.3, Y0 + CENTRE[1] - 0.2, 6.0
    for _ in range(N_REST):
        ru, rv = rs.uniform(0.0, W), rs.uniform(0.0, H)
        if fam == "bigdg":  # below the crowded tile's rows (bbox radius <= 5): its list ends with the crowd, at position 213
            rv = H - 3.0 + 3.0 * rv / H
        u.append(ru); v.append(rv); r.append(rs.uniform(2.0, 5.0)); op.append(0.8); kind.append("rest")
    # ANCHORS: a few ordinary Gaussians in FRONT of everything (nearest depths, last indices), in the corner of the frame opposite the
    # crowded tile and in none of its lists.  Without them the dead scenes have no gradient of ordinary size at all -- every tensor's
    # maximum is the flat groups' own, tiny one -- and "1e-4 of max" is then a statement about the rounding residue S of the dead units
    # (the kernel's rows there are small, not zero): such scenes missed grad_scales by 1.2e-4 ... 3.5e-4 identically with and without
    # the dead walk.
    ax, ay = (3.5, 3.5) if name == "edge" else (W - 3.5, H - 3.5)
    for _ in range(N_ANCHOR):
        u.append(ax + rs.uniform(-0.5, 0.5)); v.append(ay + rs.uniform(-0.5, 0.5)); r.append(rs.uniform(2.0, 2.5)); op.append(0.8); kind.append("anchor")
    u, v, r = np.asarray(u), np.asarray(v), np.asarray(r)
    N = len(u)
    assert N <= 300
    th = rs.uniform(0.0, np.pi, N)
    minor = np.where(r > 100, 1.0, 0.6)
    color = (0.2 + 0.7 * rs.random_sample((N, 3))).astype(np.float32)
    gI = rs.standard_normal((3, H, W)).astype(np.float32)
    gD = (rs.standard_normal((H, W)) * 0.1).astype(np.float32) + 0.05
    if rect is not None:  # the upstream gradient is eight times larger on the open region: what a probe gathers there is then >= 1e-2
        gI[:, Y0 + rect[2]:Y0 + rect[3], X0 + rect[0]:X0 + rect[1]] *= 8  # of the groups' own sums over the whole frame, in every unit
    opacity = np.asarray(op, np.float32)
    if opacity_all is not None:
        opacity[:] = opacity_all
    z = -2.0 - 0.004 * np.arange(N)
    z[N - N_ANCHOR:] = -1.9 - 0.004 * np.arange(N_ANCHOR)
    s = r / 3.0 * -z / FOCAL
    pos = np.stack([(u - W / 2) * -z / FOCAL, -(v - H / 2) * -z / FOCAL, z], 1).astype(np.float32)
    scale = np.stack([s, minor * s, 1e-3 * s], 1).astype(np.float32)
    quat = np.stack([np.cos(th / 2), 0 * th, 0 * th, np.sin(th / 2)], 1).astype(np.float32)
    probes = tuple(i for i, kd in enumerate(kind) if kd == "probe")
    return [pos, scale, quat, color, opacity], gI, gD, probes, n_front


@functools.lru_cache(maxsize=None)
def _reference(name, W, H, tile_w, opacity_all=None):
    from oracle import fgs_oracle as orc
    arrs, gI, gD = _scene(name, W, H, tile_w, opacity_all)[:3]
    ocam = orc.make_camera(np.eye(4, dtype=np.float32), FOCAL, FOCAL, W / 2, H / 2, W, H)
    r32 = orc.render(*arrs, ocam, bg=BG)
    g32 = orc.render_backward(r32, gI, gD)
    with orc.fp64():
        r64 = orc.render(*arrs, ocam, bg=BG)
        g64 = orc.render_backward(r64, gI, gD)
    return r32, g32, r64, g64


@functools.lru_cache(maxsize=None)
def _emulate(name, W, H, tile_w, seg_len, parts, opacity_all=None):
    """fp32 emulation of the forward's T at the segment boundaries of every tile with more than one segment.
    Returns (units, lists, gcol): units[(tile, seg)] = dict(T=re-based restart T [16, tile_w], Tpart=the part-local state where the
    kernel re-bases (else T), inframe=mask, start=list offset); lists[tile] = the tile's Gaussian indices; gcol[(tile, j)] = the
    colour gradient (3,) that list entry j of the tile gathers from the tile's pixels (float64)."""
    from oracle import fgs_oracle as orc
    r32 = _reference(name, W, H, tile_w, opacity_all)[0]
    arrs, gI = _scene(name, W, H, tile_w, opacity_all)[:2]
    opacity = arrs[4]
    assert r32.proj["visible"].all()
    ranges, ids = orc.tile_lists(r32.vis_sorted, r32.proj["bbox"], W, H, tile_w=tile_w)
    mean, conic, bbox = r32.proj["mean2d"].astype(np.float32), r32.proj["conic"].astype(np.float32), r32.proj["bbox"]
    tiles_x = -(-W // tile_w)
    units, lists, gcol = {}, {}, {}
    for t in range(len(ranges) - 1):
        lst = ids[ranges[t]:ranges[t + 1]]
        lists[t] = lst
        nseg = -(-len(lst) // seg_len)
        X0, Y0 = (t % tiles_x) * tile_w, (t // tiles_x) * 16
        xs, ys = X0 + np.arange(tile_w), Y0 + np.arange(16)
        inframe = (xs < W)[None, :] & (ys < H)[:, None]
        gIt = np.zeros((3, 16, tile_w))
        gIt[:, :min(16, H - Y0), :min(tile_w, W - X0)] = gI[:, Y0:Y0 + 16, X0:X0 + tile_w]
        spp = -(-nseg // parts) if parts > 1 else nseg
        T = np.ones((16, tile_w), np.float32)
        Tpart = T.copy()
        for j, i in enumerate(lst):
            if j and j % seg_len == 0:
                s = j // seg_len
                first_of_part = parts > 1 and s % spp == 0
                if first_of_part:
                    Tpart = np.ones_like(T)
                rebased = parts > 1 and s >= spp and not first_of_part
                units[(t, s)] = dict(T=T.copy(), Tpart=Tpart.copy() if rebased else T.copy(), inframe=inframe, start=j)
            dx, dy = (xs.astype(np.float32) - mean[i, 0])[None, :], (ys.astype(np.float32) - mean[i, 1])[:, None]
            q = conic[i, 0] * dx * dx + conic[i, 1] * dx * dy + conic[i, 2] * dy * dy
            al = np.minimum(np.float32(0.99), opacity[i] * np.exp(np.float32(-0.5) * q)).astype(np.float32)
            inb = ((xs >= bbox[i, 0]) & (xs < bbox[i, 1]))[None, :] & ((ys >= bbox[i, 2]) & (ys < bbox[i, 3]))[:, None]
            al = np.where(inb, al, np.float32(0))
            gcol[(t, j)] = (gIt * (al * T).astype(np.float64)[None]).sum((1, 2))
            T = (T * (np.float32(1) - al)).astype(np.float32)
            Tpart = (Tpart * (np.float32(1) - al)).astype(np.float32)
    return units, lists, gcol


def classify(unit, thr_dead=T_DEAD, veto_outside=False, part_local=False, overlook=None):
    """'dead' / 'live' / 'ambiguous' of one emulated unit.  The changed predicates of the CPU half: thr_dead = 2^-20 (a pixel below it
    counts as dead), veto_outside (lanes outside the frame, T = 1, take part), part_local (the checkpoint's own state where the
    kernel re-bases it), overlook (a pixel mask that the predicate does not look at)."""
    T = unit["Tpart"] if part_local else unit["T"]
    look = np.ones_like(unit["inframe"]) if veto_outside else unit["inframe"].copy()
    if overlook is not None:
        look &= ~overlook
    if (T[look] > T_LIVE).any():
        return "live"
    return "dead" if (T[look] < thr_dead).all() else "ambiguous"


def _pattern(name, W, H, tile_w, seg_len, parts, opacity_all=None, **changed):
    units = _emulate(name, W, H, tile_w, seg_len, parts, opacity_all)[0]
    return {k: classify(u, **changed) for k, u in units.items()}


def _parts_of(tuning):
    return tuning.get("fwd_variant", 0) if tuning.get("fwd_variant", 0) > 1 else 0


def _crowded_tile(name, W, H, tile_w):
    X0, Y0 = _crowded_origin(name, W, H, tile_w)
    return (Y0 // 16) * -(-W // tile_w) + X0 // tile_w


def _open_mask(name, tile_w):
    rect = _open_rect(name, tile_w)
    m = np.zeros((16, tile_w), bool)
    if rect is not None:
        m[rect[2]:rect[3], rect[0]:rect[1]] = True
    return m


def check_scene(name, W, H, tile_w, tuning, opacity_all=None):
    """the dead / live pattern the scene is there for, with margin; returns {(tile, seg): 'dead' | 'live'}.  Patterns are asserted
    for the split the tuning names; with fwd_variant automatic the predicate reads the re-based state whatever the split is."""
    seg_len, parts = tuning["seg_len"], _parts_of(tuning)
    units, lists, _ = _emulate(name, W, H, tile_w, seg_len, parts, opacity_all)
    pat = {k: classify(u) for k, u in units.items()}
    assert "ambiguous" not in pat.values(), {k: v for k, v in pat.items() if v == "ambiguous"}
    probes, n_front = _scene(name, W, H, tile_w, opacity_all)[3:5]
    ct = _crowded_tile(name, W, H, tile_w)
    lst = lists[ct]
    n_list = n_front + N_CROWD
    assert len(lst) >= n_list and (lst[:n_list] == np.arange(n_list)).all()  # list position = index in the crowded tile
    mine = sorted(s for (t, s) in pat if t == ct)
    assert len(mine) >= 1 and len(lst) > 192  # four segments of 64 at least: all three restart forms under fwd_variant 2
    fam, k = name.split("@")[0], _arg(name)
    if opacity_all is not None:
        assert set(pat.values()) == {"live"}
        return pat
    behind = [s for s in mine if units[(ct, s)]["start"] >= n_front]
    assert behind
    if fam in ("dead", "edge", "clamp", "op0", "bigdg"):
        assert set(pat.values()) == {"dead"} and len(pat) >= (2 if seg_len == 64 else 1)
        assert (len(lst) - units[(ct, mine[-1])]["start"]) % 64 != 0  # the last chunk of the crowded tile's last unit is partial
        if fam == "edge" and (W, H) == (40, 24):
            assert not units[(ct, mine[0])]["inframe"].all()  # a partial tile: lanes outside the frame keep T = 1
            assert (units[(ct, mine[0])]["T"][~units[(ct, mine[0])]["inframe"]] == 1).all()
        if fam == "bigdg":  # the first and the last entry of EVERY dead unit of the crowded tile, at either segment length
            assert len(lst) == n_list == BIGDG_AT[-1] + 1
            for s_ in mine:
                assert units[(ct, s_)]["start"] in BIGDG_AT and min(units[(ct, s_)]["start"] + seg_len, len(lst)) - 1 in BIGDG_AT
        if fam in ("clamp", "op0"):
            assert units[(ct, k // seg_len)]["start"] <= k and k // seg_len >= 1  # the flagged entry lies in a dead unit
        if fam == "clamp":
            r32, op = _reference(name, W, H, tile_w)[0], _scene(name, W, H, tile_w)[0][4]
            X0, Y0 = _crowded_origin(name, W, H, tile_w)
            a, bc, d = [float(x) for x in r32.proj["conic"][k]]
            dx, dy = X0 + CENTRE[0] - float(r32.proj["mean2d"][k][0]), Y0 + CENTRE[1] - float(r32.proj["mean2d"][k][1])
            assert float(op[k]) * np.exp(-0.5 * (a * dx * dx + bc * dx * dy + d * dy * dy)) > 0.99  # the clamp binds at the centre
    else:
        open_mask = _open_mask(name, tile_w)
        g32 = _reference(name, W, H, tile_w)[1]["colors"]
        assert len(probes) >= 20
        closed_at = {"seam": lambda: k + 1, "seamin": lambda: k + N_FRONT}.get(fam, lambda: None)()  # list position behind G2's last entry
        for s in behind:
            un = units[(ct, s)]
            if closed_at is not None and un["start"] + 2 >= closed_at:  # (up to two entries of G2 may lie behind the boundary)
                assert pat[(ct, s)] == "dead", (name, s)
                continue
            if closed_at is not None and un["start"] > closed_at - N_FRONT:
                continue  # a boundary inside G2: classified with margin above, whichever way
            assert pat[(ct, s)] == "live", (name, s)
            live = (un["T"] > T_LIVE) & un["inframe"]
            assert (live == (open_mask & un["inframe"])).all()  # live through the open region alone: no front group touches it
            assert (un["T"][un["inframe"] & ~open_mask] < T_DEAD).all()
            # ... and what a predicate that took this unit for dead would lose is large: a probe IN this unit (list position = index)
            # whose reference grad_colors is >= 1e-2 of max.  (Not every probe: they stand on a few pixels of the open region and
            # shadow one another, the smallest holds 1e-3 ... 2e-2 of max.)
            # seam / seamin: the entries of the closing group G2 count as well (behind them the column is shut).  A unit that
            # holds fewer than six of the crowd's positions -- the tail of the list -- need not hold a probe.
            here = range(un["start"], min(un["start"] + seg_len, n_list))
            mine_here = [i for i in here if i in probes or closed_at is not None]
            if len(here) >= 6:
                assert mine_here and np.abs(g32[mine_here]).max() >= 1e-2 * np.abs(g32).max(), (name, s)
        if fam == "seam":  # the unit behind the boundary the seam is named for restarts dead
            named = [s for s in behind if units[(ct, s)]["start"] in (64, 128) and abs(units[(ct, s)]["start"] - (k + 1)) <= 2]
            if seg_len == 64 or k >= 127:
                assert named and all(pat[(ct, s)] == "dead" for s in named)
            assert pat[(ct, behind[0])] == "live" or units[(ct, behind[0])]["start"] + 2 >= closed_at
        if fam == "seamin" and seg_len == 64:
            assert pat[(ct, 1)] == "live" and pat[(ct, 2)] == "dead"  # restarts live, goes dead inside; the next restarts dead
    return pat


def _wholly_dead(name, W, H, tile_w, tuning):
    """Gaussians all of whose list entries lie in dead units"""
    seg_len = tuning["seg_len"]
    units, lists, _ = _emulate(name, W, H, tile_w, seg_len, _parts_of(tuning))
    pat = {k: classify(u) for k, u in units.items()}
    N = len(_scene(name, W, H, tile_w)[0][4])
    ok, seen = np.ones(N, bool), np.zeros(N, bool)
    for t, lst in lists.items():
        for j, i in enumerate(lst):
            seen[i] = True
            if pat.get((t, j // seg_len)) != "dead":
                ok[i] = False
    return np.nonzero(ok & seen)[0]


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
def _hip_scene(name, W, H, tile_w, tun, opacity_all=None):
    arrs, gI, gD = _scene(name, W, H, tile_w, opacity_all)[:3]
    return _hip(arrs, W, H, gI, gD, dict(tile_w=tile_w, **TUNINGS[tun]))


gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("tun", sorted(TUNINGS))
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("name,tile_w", CASES)
def test_scene_vs_oracle(name, tile_w, frame, tun):
    W, H = frame
    check_scene(name, W, H, tile_w, TUNINGS[tun])
    got = _hip_scene(name, W, H, tile_w, tun)
    r32, g32, r64, g64 = _reference(name, W, H, tile_w)
    what = f"{name} {W}x{H} tile_w={tile_w} {tun}"
    assert_with_referee(got["image"], r32.image, r64.image, f"{what} image")
    assert_with_referee(got["depth"], r32.depth, r64.depth, f"{what} depth")
    for k in GRADS:
        assert_with_referee(got[k], g32[k], g64[k], f"{what} grad_{k}")
    if name == "dead":  # w = a' T = 0 in a dead unit: pins the colour sums, whichever walk wrote them
        idx = _wholly_dead(name, W, H, tile_w, TUNINGS[tun])
        assert len(idx) >= 64 and not got["colors"][idx].any(), what  # (segments of 128: the crowded tile's entries from 128 on)
    arrs, gI, gD = _scene(name, W, H, tile_w)[:3]  # the scene once more: bitwise the same
    again = _hip(arrs, W, H, gI, gD, dict(tile_w=tile_w, **TUNINGS[tun]))
    for k in GRADS + ["image", "depth"]:
        assert np.array_equal(got[k], again[k]), f"{what} {k}: second run differs"


@gpu
@pytest.mark.parametrize("tun", sorted(TUNINGS))
@pytest.mark.parametrize("tile_w", TILE_WS)
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_batch_equals_single_calls(frame, tile_w, tun):
    """one saturating image and one that never saturates in ONE call: dead and general units side by side in a launch"""
    W, H = frame
    pat_a = check_scene("dead", W, H, tile_w, TUNINGS[tun])
    pat_b = check_scene("dead", W, H, tile_w, TUNINGS[tun], opacity_all=0.05)
    assert set(pat_a.values()) == {"dead"} and set(pat_b.values()) == {"live"}
    a, gI, gD = _scene("dead", W, H, tile_w)[:3]
    b = _scene("dead", W, H, tile_w, 0.05)[0]
    both = _hip([np.stack([x, y]) for x, y in zip(a, b)], W, H, np.stack([gI, gI]), np.stack([gD, gD]), dict(tile_w=tile_w, **TUNINGS[tun]))
    for i, single in enumerate((_hip_scene("dead", W, H, tile_w, tun), _hip_scene("dead", W, H, tile_w, tun, 0.05))):
        for k in GRADS + ["image", "depth"]:
            assert np.array_equal(both[k][i], single[k]), (i, k)
    r32, g32, r64, g64 = _reference("dead", W, H, tile_w, 0.05)
    for k in GRADS:
        assert_with_referee(both[k][1], g32[k], g64[k], f"batch image 1 grad_{k}")


# ---- CPU half: the emulation with a changed predicate ----
CPU_FRAMES = [(64, 32), (40, 24)]


@pytest.mark.parametrize("tun", ["s64v2", "s128"])  # (the GPU tests assert the pattern of every tuning they run)
@pytest.mark.parametrize("frame", CPU_FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("name,tile_w", CASES)
def test_cpu_patterns_hold_and_ignore_the_threshold(name, tile_w, frame, tun):
    """every scene's pattern holds with margin, and counting T < 2^-20 as dead changes the pattern of no unit"""
    W, H = frame
    pat = check_scene(name, W, H, tile_w, TUNINGS[tun])
    assert _pattern(name, W, H, tile_w, TUNINGS[tun]["seg_len"], _parts_of(TUNINGS[tun]), thr_dead=T_LIVE) == pat


@pytest.mark.parametrize("tile_w", TILE_WS)
def test_cpu_outside_lanes_must_not_veto(tile_w):
    """`edge` on the 40 x 24 frame: with the lanes outside the frame taking part, the partial tiles' dead units turn live"""
    pat = check_scene("edge", 40, 24, tile_w, TUNINGS["s64"])
    veto = _pattern("edge", 40, 24, tile_w, 64, 0, veto_outside=True)
    ct = _crowded_tile("edge", 40, 24, tile_w)
    flipped = [k for k in pat if pat[k] == "dead" and veto[k] == "live"]
    assert flipped and all(k in flipped for k in pat if k[0] == ct)


@pytest.mark.parametrize("frame", CPU_FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("tile_w", TILE_WS)
def test_cpu_predicate_reads_the_rebased_state(tile_w, frame):
    """`dead` under fwd_variant 2 with segments of 64: the re-based segment of the crowded tile (part-local checkpoint composed with
    its part's first slot) is dead, its part-local state alone is live; the other two restart forms read one slot"""
    W, H = frame
    pat = check_scene("dead", W, H, tile_w, TUNINGS["s64v2"])
    local = _pattern("dead", W, H, tile_w, 64, 2, part_local=True)
    ct = _crowded_tile("dead", W, H, tile_w)
    nseg = 1 + max(s for (t, s) in pat if t == ct)
    spp = -(-nseg // 2)
    rebased = [(ct, s) for s in range(1, nseg) if s > spp]
    assert nseg >= 4 and rebased
    for k in pat:
        assert (local[k] == "live") == (k in rebased) if k[0] == ct else True, k
        assert pat[k] == "dead"


@pytest.mark.parametrize("frame", CPU_FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("name,tile_w", [c for c in CASES if c[0].split("@")[0] in ("col", "row", "sub")])
def test_cpu_overlooked_live_lanes_lose_gradients(name, tile_w, frame):
    """a predicate that overlooks the open region calls the crowded tile's live units dead, and the colour gradients that the dead
    walk leaves out there are >= 10 x the tolerance of the family's statement (1e-4 of max) -- the emulation's sums agree with the
    oracle's grad_colors to 1e-4 of max themselves"""
    W, H = frame
    tuning = TUNINGS["s64"]
    pat = check_scene(name, W, H, tile_w, tuning)
    wrong = _pattern(name, W, H, tile_w, 64, 0, overlook=_open_mask(name, tile_w))
    ct = _crowded_tile(name, W, H, tile_w)
    lost_units = [k for k in pat if k[0] == ct and pat[k] == "live" and wrong[k] == "dead"]
    assert lost_units
    units, lists, gcol = _emulate(name, W, H, tile_w, 64, 0)
    g32 = _reference(name, W, H, tile_w)[1]["colors"]
    total = np.zeros_like(g32, dtype=np.float64)
    for (t, j), g in gcol.items():
        total[lists[t][j]] += g
    assert np.abs(total - g32).max() <= 1e-4 * np.abs(g32).max()
    lost = max(np.abs(gcol[(t, j)]).max() for (t, s) in lost_units for j in range(units[(t, s)]["start"], min(len(lists[t]), units[(t, s)]["start"] + 64)))
    assert lost >= 10 * 1e-4 * np.abs(g32).max(), lost / np.abs(g32).max()
