"""Dead work units of k_composite_bwd walked TWO LIST ENTRIES PER ROUND (fgs_composite.hip, 32 x 16 tiles): entries j, j + 1 of a
staged chunk park six sums each side by side, one reduction serves both, quad k < 12 stores float k % 6 of row e[k / 6] and eight
idle lanes store the rows' four colour / depth floats as literal zeros; a unit's last entry can be single.  16 x 16 tiles walk one
entry per round through the same code.  What can go wrong is OWNERSHIP -- which row a sum lands in, a row written twice or never,
the single tail -- at the seams of the pairing: the end of a unit, the 64-record chunk boundary, and entries of unlike kind side by
side.  The scenes put those seams into dead units and say so on the CPU before anything runs.

Geometry (as tests/test_blend_bwd_dead_units.py, whose helpers this file imports): one saturating group of 24 entries whose bbox is
the whole frame, frontmost in every list -- behind it T <= 0.25^24 -- then the CROWD under test, every member of which touches the
tile at the frame's origin (list position = index there, on either tile shape), and six ordinary anchors in front of everything in
the far corner (in none of the crowded tile's lists: they give every tensor a maximum of ordinary size).  No other Gaussians: the
crowded tile's list is exactly 24 + crowd entries long.

Families:
  tail@k      k = 1, 2, 3, 63, 64, 65, 66, 127, 128: the list is 128 + k entries long, so with segments of 128 the crowded tile's
              last unit holds k entries and with segments of 64 it holds (k - 1) % 64 + 1 = 1, 2, 3, 63 or 64 -- the single last
              entry (odd counts), a pair that ends on the chunk boundary (64, 128), an entry alone in the second chunk (65).
  pairs       from list position 128 on (a dead unit at either segment length; pairs are (even, odd) positions), runs X Y Y X, so
              that X is the first AND the second member of a pair with Y, for: every sub-tile touched x exactly one touched (each of
              the tile's sub-tiles); a whole sub-tile row (either row) x the first sub-tile column alone; clamp-flagged (opacity
              0.995 on a pixel centre) x not flagged; opacity 0 and a negative opacity (no flag, no sub-tile) x an ordinary entry,
              and the two side by side; the largest member of the crowd x an ordinary entry.
Every case: check_scene asserts, from the oracle's projection and tile lists by an fp32 emulation of T with the dead-unit file's
margins (dead: T < 2^-40 on every in-frame pixel), that every unit of the crowded tile behind the group is dead, that the last one
holds exactly the intended number of entries, and for `pairs` that every run's entries have exactly the intended sub-tile pattern
and flags.  Then image, depth and the five gradients against the C oracle under the referee; a second run bitwise equal; and
grad_colors of the Gaussians that lie wholly in dead units EXACTLY zero -- the literal zeros of floats 6-9.  Frames 64 x 32 and
40 x 24, both tile widths, segments of 64 and 128, fwd_variant 1, 2 and automatic.
  rows        tests/workspace_guard.py around every buffer of the call (the gradient rows live in the scratch buffer): guards
              intact -- nothing written outside -- and all outputs bitwise equal under the three fills and unpatched, which holds
              only if every row that k_project_bwd sums was written (an unwritten row still holds the fill).
  batch       `pairs` and the same geometry at opacity 0.05 (no unit dead) in ONE call: bit-equal to the two single calls.

CPU half.  The VALUES of a dead unit's rows cannot tell a wrong pairing from the right one against the oracle: every pixel has
T = 0 there, the exact sums are zero and what the kernel stores is the rounding residue of S (test_cpu_dead_rows_are_residues bounds
what the exact arithmetic gives: nothing).  What tells them apart is which cells get written, so the CPU half runs a model of the
round's store map (quad k -> float k % 6 of row e[k / 6], lanes 48-55 -> floats 6-9) over the dead units the scenes really contain
and shows that the right map writes every cell of every entry's row exactly once, while
  * `B's sums stored to A's row` leaves B's row unwritten in every unit with a pair (the `rows` test's fill survives), and
  * `the single tail stored twice` -- the second row index left over from the round before -- writes a row twice in every unit that
    ends with a single entry behind a pair (counts 3, 63, 65, 127), and with zeros where that row's own residue belongs.
A third wrong version in the round's plan, a row-block selector taken for a partly touched row, has nothing to check: the straight-line pass
groups were measured slower and are not in the kernel (DESIGN_LOG.md 22), and a pass run for an untouched sub-tile adds exact zeros
in any case (the lane masks zero a' outside the bbox)."""
import functools

import numpy as np
import pytest
import torch

import workspace_guard as WG
from helpers import assert_with_referee
from test_blend_bwd_dead_units import BG, FOCAL, GRADS, N_ANCHOR, N_FRONT, SIGMA, T_DEAD, TUNINGS, _cuda, _group_mean, _hip, _parts_of, classify

FRAMES = [(64, 32), (40, 24)]
TILE_WS = [16, 32]
TAILS = (1, 2, 3, 63, 64, 65, 66, 127, 128)
SCENES = [f"tail@{k}" for k in TAILS] + ["pairs"]
PAIRS_AT = 128  # first list position of the `pairs` runs


def _runs(tile_w):
    """the X Y Y X runs of `pairs`, in list order: (X, Y) kinds"""
    ns = 2 * (tile_w // 8)
    return ([("all", f"one@{p}") for p in range(ns)] + [("row@0", "col@0"), ("row@1", "col@0"), ("clamp", "crowd"), ("op0", "crowd"),
            ("neg", "crowd"), ("op0", "neg"), ("big", "crowd")])


def _kinds(name, tile_w):
    """kind of every crowd entry, in list order behind the front group"""
    if name.startswith("tail@"):
        return ["crowd"] * (128 + int(name[5:]) - N_FRONT)
    kinds = ["crowd"] * (PAIRS_AT - N_FRONT)
    for x, y in _runs(tile_w):
        kinds += [x, y, y, x]
    return kinds + ["crowd"] * 3  # (an odd tail behind the runs)


def _place(kind, tile_w, rs):
    """(u, v, bbox radius, opacity) of one crowd entry; the bbox is the square of that radius about (u, v), clipped to the frame"""
    if kind == "crowd":
        return rs.uniform(2.5, 12.5), rs.uniform(2.5, 12.5), rs.uniform(1.0, 1.8), 0.8  # (bbox inside the 16 x 16 corner: in no other tile)
    if kind == "all":  # the whole tile, with four pixels to spare
        return tile_w / 2.0, 8.0, tile_w / 2.0 + 5.0, 0.8
    if kind.startswith("one@"):  # inside one 8 x 8 sub-tile
        p, nsx = int(kind[4:]), tile_w // 8
        return 8.0 * (p % nsx) + 4.0, 8.0 * (p // nsx) + 4.0, 2.5, 0.8
    if kind == "row@0":  # from above the frame down to y ~ 4: every column of sub-tile row 0, nothing of row 1
        return tile_w / 2.0, 4.5 - 22.0, 22.0, 0.8
    if kind == "row@1":  # from y ~ 11 downwards
        return tile_w / 2.0, 11.5 + 22.0, 22.0, 0.8
    if kind == "col@0":  # from the left of the frame up to x ~ 4: both rows of sub-tile column 0
        return 4.5 - 13.0, 8.0, 13.0, 0.8
    if kind == "clamp":
        return 8.0, 8.0, 3.0, 0.995
    if kind == "op0":
        return 8.0, 8.0, 3.0, 0.0
    if kind == "neg":
        return 8.0, 8.0, 3.0, -0.3
    if kind == "big":
        return 8.3, 7.8, 6.0, 0.8
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _scene(name, W, H, tile_w, opacity_all=None):
    """flat Gaussians turned about the viewing axis, item 0 frontmost (the construction of the dead-unit file's _scene)"""
    rs = np.random.RandomState(9700 + W + tile_w)
    u, v, r, op, minor = [], [], [], [], []
    gu, gv = _group_mean(("x", "hi", 0), W, H)  # the whole frame as the half-plane x >= 0
    for _ in range(N_FRONT):
        u.append(gu + rs.uniform(-0.2, 0.2)); v.append(gv + rs.uniform(-0.2, 0.2)); r.append(3 * SIGMA); op.append(0.8); minor.append(1.0)
    kinds = _kinds(name, tile_w)
    for kd in kinds:
        pu, pv, pr, po = _place(kd, tile_w, rs)
        u.append(pu); v.append(pv); r.append(pr); op.append(po); minor.append(0.6 if kd in ("crowd", "big", "clamp", "op0", "neg") else 1.0)
    for _ in range(N_ANCHOR):  # ordinary Gaussians in front of everything, in the far corner
        u.append(W - 3.5 + rs.uniform(-0.5, 0.5)); v.append(H - 3.5 + rs.uniform(-0.5, 0.5)); r.append(rs.uniform(2.0, 2.5)); op.append(0.8); minor.append(0.6)
    u, v, r, minor = np.asarray(u), np.asarray(v), np.asarray(r), np.asarray(minor)
    N = len(u)
    assert N <= 300
    th = rs.uniform(0.0, np.pi, N)
    color = (0.2 + 0.7 * rs.random_sample((N, 3))).astype(np.float32)
    gI = rs.standard_normal((3, H, W)).astype(np.float32)
    gD = (rs.standard_normal((H, W)) * 0.1).astype(np.float32) + 0.05
    opacity = np.asarray(op, np.float32)
    if opacity_all is not None:
        opacity[:] = opacity_all
    z = -2.0 - 0.004 * np.arange(N)
    z[N - N_ANCHOR:] = -1.9 - 0.004 * np.arange(N_ANCHOR)
    s = r / 3.0 * -z / FOCAL
    pos = np.stack([(u - W / 2) * -z / FOCAL, -(v - H / 2) * -z / FOCAL, z], 1).astype(np.float32)
    scale = np.stack([s, minor * s, 1e-3 * s], 1).astype(np.float32)
    quat = np.stack([np.cos(th / 2), 0 * th, 0 * th, np.sin(th / 2)], 1).astype(np.float32)
    return [pos, scale, quat, color, opacity], gI, gD, tuple(kinds)


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
    """fp32 emulation of the forward's T at the segment boundaries (the dead-unit file's _emulate, on this file's scenes).
    -> (units, lists, touched): units[(tile, seg)] = dict(T, Tpart, inframe, start) as classify() reads them; lists[tile] = the
    tile's Gaussian indices; touched[j] = the set of 8 x 8 sub-tiles (row * nsx + col) of the crowded tile that the bbox of its list
    entry j meets."""
    from oracle import fgs_oracle as orc
    r32 = _reference(name, W, H, tile_w, opacity_all)[0]
    opacity = _scene(name, W, H, tile_w, opacity_all)[0][4]
    assert r32.proj["visible"].all()
    ranges, ids = orc.tile_lists(r32.vis_sorted, r32.proj["bbox"], W, H, tile_w=tile_w)
    mean, conic, bbox = r32.proj["mean2d"].astype(np.float32), r32.proj["conic"].astype(np.float32), r32.proj["bbox"]
    tiles_x, nsx = -(-W // tile_w), tile_w // 8
    units, lists = {}, {}
    for t in range(len(ranges) - 1):
        lst = ids[ranges[t]:ranges[t + 1]]
        lists[t] = lst
        nseg = -(-len(lst) // seg_len)
        X0, Y0 = (t % tiles_x) * tile_w, (t // tiles_x) * 16
        xs, ys = X0 + np.arange(tile_w), Y0 + np.arange(16)
        inframe = (xs < W)[None, :] & (ys < H)[:, None]
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
            al = np.minimum(np.float32(0.99), np.maximum(np.float32(0), opacity[i] * np.exp(np.float32(-0.5) * q))).astype(np.float32)
            inb = ((xs >= bbox[i, 0]) & (xs < bbox[i, 1]))[None, :] & ((ys >= bbox[i, 2]) & (ys < bbox[i, 3]))[:, None]
            al = np.where(inb, al, np.float32(0))
            T = (T * (np.float32(1) - al)).astype(np.float32)
            Tpart = (Tpart * (np.float32(1) - al)).astype(np.float32)
    touched = []
    for i in lists[0]:
        x0, x1, y0, y1 = [int(b) for b in bbox[i]]
        touched.append(frozenset(rr * nsx + cc for rr in range(2) for cc in range(nsx)
                                 if max(x0, 8 * cc) < min(x1, 8 * cc + 8, W) and max(y0, 8 * rr) < min(y1, 8 * rr + 8, H)))
    return units, lists, touched


def _want_touched(kind, tile_w):
    nsx = tile_w // 8
    if kind in ("all",):
        return frozenset(range(2 * nsx))
    if kind.startswith("one@"):
        return frozenset([int(kind[4:])])
    if kind.startswith("row@"):
        return frozenset(int(kind[4:]) * nsx + c for c in range(nsx))
    if kind == "col@0":
        return frozenset([0, nsx])
    return None  # crowd, clamp, op0, neg, big: wherever the bbox falls (the kernel clears a negative opacity's sub-tiles itself)


def check_scene(name, W, H, tile_w, tuning, opacity_all=None):
    """the scene holds what it is named for, with margin: -> (units of the crowded tile behind the group, their entry counts)"""
    seg_len, parts = tuning["seg_len"], _parts_of(tuning)
    units, lists, touched = _emulate(name, W, H, tile_w, seg_len, parts, opacity_all)
    arrs, _, _, kinds = _scene(name, W, H, tile_w, opacity_all)
    pat = {k: classify(u) for k, u in units.items()}
    lst = lists[0]
    n_list = N_FRONT + len(kinds)
    assert len(lst) == n_list and (lst == np.arange(n_list)).all()  # list position = index, and nothing else in the crowded tile
    mine = sorted(s for (t, s) in pat if t == 0)
    counts = {s: min(units[(0, s)]["start"] + seg_len, n_list) - units[(0, s)]["start"] for s in mine}
    if opacity_all is not None:
        assert set(pat.values()) == {"live"}
        return mine, counts
    assert mine and set(pat.values()) == {"dead"}, pat  # every later unit of every tile: T < 2^-40 on every in-frame pixel
    assert all((units[(0, s)]["T"][units[(0, s)]["inframe"]] < T_DEAD).all() for s in mine)
    if name.startswith("tail@"):
        k = int(name[5:])
        assert n_list == 128 + k and counts[mine[-1]] == (k if seg_len == 128 else (k - 1) % 64 + 1), (counts, k)
        assert seg_len == 128 or counts[mine[-1]] in (1, 2, 3, 63, 64)
    else:
        opacity = arrs[4]
        pos = PAIRS_AT
        assert all(units[(0, s)]["start"] % 2 == 0 for s in mine) and PAIRS_AT % seg_len == 0  # pairs are (even, odd); a unit starts at the runs
        for x, y in _runs(tile_w):
            for off, kd in enumerate((x, y, y, x)):  # (x, y) is a pair and (y, x) is the next
                j = pos + off
                assert kinds[j - N_FRONT] == kd and pat[(0, j // seg_len)] == "dead"
                want = _want_touched(kd, tile_w)
                assert want is None or touched[j] == want, (kd, j, sorted(touched[j]), sorted(want))
                assert touched[j], (kd, j)  # every entry of a run meets the crowded tile
                assert (opacity[j] > 0.98) == (kd == "clamp") and (opacity[j] == 0) == (kd == "op0") and (opacity[j] < 0) == (kd == "neg")
            pos += 4
        r32 = _reference(name, W, H, tile_w)[0]  # the clamp binds at the flagged entry's centre pixel
        j = N_FRONT + kinds.index("clamp")
        a, bc, d = [float(c) for c in r32.proj["conic"][j]]
        dx, dy = 8.0 - float(r32.proj["mean2d"][j][0]), 8.0 - float(r32.proj["mean2d"][j][1])
        assert float(opacity[j]) * np.exp(-0.5 * (a * dx * dx + bc * dx * dy + d * dy * dy)) > 0.99
        big = N_FRONT + kinds.index("big")  # ... and `big` has the largest bbox among the crowd's ordinary members
        area = lambda i: (int(r32.proj["bbox"][i][1]) - int(r32.proj["bbox"][i][0])) * (int(r32.proj["bbox"][i][3]) - int(r32.proj["bbox"][i][2]))
        assert all(area(big) > area(N_FRONT + i) for i, kd in enumerate(kinds) if kd == "crowd")
    return mine, counts


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


@functools.lru_cache(maxsize=None)
def _hip_scene(name, W, H, tile_w, tun, opacity_all=None):
    arrs, gI, gD = _scene(name, W, H, tile_w, opacity_all)[:3]
    return _hip(arrs, W, H, gI, gD, dict(tile_w=tile_w, **TUNINGS[tun]))


gpu = pytest.mark.gpu
_frame_ids = dict(ids=lambda f: f"{f[0]}x{f[1]}")


@gpu
@pytest.mark.parametrize("tun", sorted(TUNINGS))
@pytest.mark.parametrize("frame", FRAMES, **_frame_ids)
@pytest.mark.parametrize("tile_w", TILE_WS)
@pytest.mark.parametrize("name", SCENES)
def test_scene_vs_oracle(name, tile_w, frame, tun):
    W, H = frame
    mine, counts = check_scene(name, W, H, tile_w, TUNINGS[tun])
    got = _hip_scene(name, W, H, tile_w, tun)
    r32, g32, r64, g64 = _reference(name, W, H, tile_w)
    what = f"{name} {W}x{H} tile_w={tile_w} {tun}"
    assert_with_referee(got["image"], r32.image, r64.image, f"{what} image")
    assert_with_referee(got["depth"], r32.depth, r64.depth, f"{what} depth")
    for k in GRADS:
        assert np.isfinite(got[k]).all(), f"{what} grad_{k}"
        assert_with_referee(got[k], g32[k], g64[k], f"{what} grad_{k}")
    # w = a' T = 0 in a dead unit: floats 6-9 of its rows are zeros.  At least the last unit's entries that meet no other tile (all but
    # the all / row / col kinds, which reach into tiles whose short lists are one live unit) lie wholly in dead units
    idx = _wholly_dead(name, W, H, tile_w, TUNINGS[tun])
    kinds, last = _scene(name, W, H, tile_w)[3], _emulate(name, W, H, tile_w, TUNINGS[tun]["seg_len"], _parts_of(TUNINGS[tun]))[0][(0, mine[-1])]["start"]
    local = [j for j in range(last, N_FRONT + len(kinds)) if kinds[j - N_FRONT].split("@")[0] not in ("all", "row", "col")]
    assert local and set(local) <= set(idx.tolist()) and not got["colors"][idx].any(), what
    arrs, gI, gD = _scene(name, W, H, tile_w)[:3]
    again = _hip(arrs, W, H, gI, gD, dict(tile_w=tile_w, **TUNINGS[tun]))
    for k in GRADS + ["image", "depth"]:
        assert np.array_equal(got[k], again[k]), f"{what} {k}: second run differs"


@gpu
@pytest.mark.parametrize("tun", ["s128", "s64", "s64v2"])
@pytest.mark.parametrize("tile_w", TILE_WS)
@pytest.mark.parametrize("name", ["tail@1", "tail@65", "tail@128", "pairs"])
def test_rows_written_once_and_nothing_else(name, tile_w, tun):
    """every buffer of the call between guards and filled with 0x00 / 0x00000001 / 0xFF words, then unpatched: the guards stay
    intact and every output is the same bits -- no row that is summed was left unwritten, whatever the unit's entry count"""
    from fresnel_amd import handoff, losses, renderer
    from fresnel_amd.renderer import Camera, TileBasedRenderer
    W, H = 40, 24
    check_scene(name, W, H, tile_w, TUNINGS[tun])
    arrs, gI, gD = _scene(name, W, H, tile_w)[:3]
    dev = _cuda()
    inp = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in zip(GRADS, arrs)}
    inp["gI"], inp["gD"] = torch.from_numpy(gI).to(dev), torch.from_numpy(gD).to(dev)

    def fn(guard):
        ts = [inp[k].detach().requires_grad_(True) for k in GRADS]
        ren = TileBasedRenderer(W, H, background=BG)
        ren.tuning = dict(tile_w=tile_w, **TUNINGS[tun])
        img, dep = ren(*ts, Camera(FOCAL, FOCAL, W / 2, H / 2, W, H), return_depth=True)
        ((img * inp["gI"]).sum() + (dep * inp["gD"]).sum()).backward()
        torch.cuda.synchronize()
        if isinstance(guard, WG.WorkspaceGuard):
            assert guard.records, "no allocation of the wrapper went through the guard"
        out = {"grad_" + k: t.grad for k, t in zip(GRADS, ts)}
        out["image"], out["depth"] = img.detach(), dep.detach()
        return out

    runs = WG.run_patterns(fn, inp, [renderer, losses, handoff])
    ref = _hip_scene(name, W, H, tile_w, tun)
    for k in GRADS:
        assert np.array_equal(runs["unpatched"]["grad_" + k].cpu().numpy(), ref[k]), k


@gpu
@pytest.mark.parametrize("tun", sorted(TUNINGS))
@pytest.mark.parametrize("tile_w", TILE_WS)
@pytest.mark.parametrize("frame", FRAMES, **_frame_ids)
def test_batch_equals_single_calls(frame, tile_w, tun):
    """`pairs` and the same geometry at opacity 0.05 in ONE call: pair rounds and the general walk side by side in a launch"""
    W, H = frame
    check_scene("pairs", W, H, tile_w, TUNINGS[tun])
    check_scene("pairs", W, H, tile_w, TUNINGS[tun], opacity_all=0.05)
    a, gI, gD = _scene("pairs", W, H, tile_w)[:3]
    b = _scene("pairs", W, H, tile_w, 0.05)[0]
    both = _hip([np.stack([x, y]) for x, y in zip(a, b)], W, H, np.stack([gI, gI]), np.stack([gD, gD]), dict(tile_w=tile_w, **TUNINGS[tun]))
    for i, single in enumerate((_hip_scene("pairs", W, H, tile_w, tun), _hip_scene("pairs", W, H, tile_w, tun, 0.05))):
        for k in GRADS + ["image", "depth"]:
            assert np.array_equal(both[k][i], single[k]), (i, k)
    r32, g32, r64, g64 = _reference("pairs", W, H, tile_w, 0.05)
    for k in GRADS:
        assert_with_referee(both[k][1], g32[k], g64[k], f"batch image 1 grad_{k}")


# ---- CPU half ----
ROW_FLOATS, SUMS = 10, 6


def store_map(n, pairs, wrong=None):
    """Model of the dead walk's row stores over one unit of n entries (rows 0 .. n - 1; chunks of 64; `pairs`: two entries per round).
    -> writes[row][float] = list of what was stored there: ('sum', entry, k) or ('zero',).  wrong = 'b_to_a': the second member's
    sums go to the first member's row; 'tail_twice': a single last entry's round keeps the second row index of the round before."""
    writes = [[[] for _ in range(ROW_FLOATS)] for _ in range(n)]
    stale = None
    for base in range(0, n, 64):
        cn = min(64, n - base)
        for j in range(0, cn, 2 if pairs else 1):
            a = base + j
            b = base + j + 1 if pairs and j + 1 < cn else None
            rows = [(a, a)]  # (row, whose sums)
            if b is not None:
                rows.append((a if wrong == "b_to_a" else b, b))
                stale = b
            elif pairs and wrong == "tail_twice" and stale is not None:
                rows.append((stale, None))  # the round's second half ran no pass: zeros
            for row, who in rows:
                for k in range(SUMS):
                    writes[row][k].append(("sum", who, k) if who is not None else ("zero",))
                for k in range(SUMS, ROW_FLOATS):
                    writes[row][k].append(("zero",))
    return writes


def _audit(writes):
    """(cells never written, cells written more than once, cells that hold another entry's sum or a zero where a sum belongs)"""
    never = sum(1 for row in writes for c in row if not c)
    twice = sum(1 for row in writes for c in row if len(c) > 1)
    alien = sum(1 for r, row in enumerate(writes) for k, c in enumerate(row) if c and k < SUMS and c[-1] != ("sum", r, k))
    return never, twice, alien


CPU_CASES = [(n, w, f, t) for n in SCENES for w in TILE_WS for f in FRAMES for t in ("s64", "s128")]


@pytest.mark.parametrize("name,tile_w,frame,tun", CPU_CASES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_cpu_store_map_owns_every_row_once(name, tile_w, frame, tun):
    """the right map, on the entry counts of the scene's dead units: every cell of every row written exactly once, with its own sum"""
    W, H = frame
    mine, counts = check_scene(name, W, H, tile_w, TUNINGS[tun])
    for s in mine:
        for pairs in (False, True):
            assert _audit(store_map(counts[s], pairs)) == (0, 0, 0), (s, counts[s], pairs)


def test_cpu_wrong_pairings_are_told_apart():
    """over the scenes' dead units (64 x 32, both segment lengths): `b_to_a` leaves a row unwritten in EVERY unit with a pair;
    `tail_twice` writes a row twice, zeros over its own sums, in the units that end with a single entry behind a pair -- and the
    scenes hold such units with 3, 63, 65 and 127 entries"""
    seen_b, seen_t = set(), set()
    for name in SCENES:
        for tun in ("s64", "s128"):
            mine, counts = check_scene(name, 64, 32, 32, TUNINGS[tun])
            for s in mine:
                n = counts[s]
                never, twice, alien = _audit(store_map(n, True, "b_to_a"))
                assert (never >= ROW_FLOATS) == (n >= 2) and (alien >= SUMS) == (n >= 2), (name, tun, n)
                seen_b.add(n)
                never, twice, alien = _audit(store_map(n, True, "tail_twice"))
                hit = n % 2 == 1 and n > 1  # a single entry with a pair before it in the unit (65: in the chunk before)
                assert (twice == ROW_FLOATS and alien == SUMS) == hit and never == 0, (name, tun, n)
                if hit:
                    seen_t.add(n)
    assert {2, 3, 63, 64, 65, 66, 127, 128} <= seen_b and {3, 63, 65, 127} <= seen_t, (sorted(seen_b), sorted(seen_t))


@pytest.mark.parametrize("tile_w", TILE_WS)
def test_cpu_dead_rows_are_residues(tile_w):
    """why values cannot referee ownership: with T < 2^-40 on every pixel, what a dead unit's entry can add to any pixel's colour is
    below 2^-40 of an opaque entry's -- the reference gradients of the Gaussians that lie wholly in dead units are below 1e-9 of
    the tensor's maximum, five orders under the tolerance, whichever row their sums were stored in"""
    idx = _wholly_dead("pairs", 64, 32, tile_w, TUNINGS["s64"])
    g64 = _reference("pairs", 64, 32, tile_w)[3]
    assert len(idx) >= 64
    for k in GRADS:
        assert np.abs(g64[k][idx]).max() <= 1e-9 * np.abs(g64[k]).max(), k
