"""The exiting depth-split forward (tuning key fwd_exit = the FGS_FWD_EXIT_ON / _OFF flag of FgsDims.fwd_variant;
k_blend_fwd_head + k_blend_fwd_parts<.., REST>, fgs_composite.hip): a 16 x 16 tile half stops walking its list once the state of every in-frame pixel ABSORBS every entry that can still come,

    T <= 2^-26   and   T K_X < 2^-26 |X|   for X in {C_r, C_g, C_b, D},

K_colour = the image's largest |0.99 colour channel| (and |background|), K_depth = its largest |0.99 depth|, tested at every 64-entry
chunk boundary of the first min(segments per part, 384 / seg_len) segments of list part 0.  Closing must not change one bit, so what
can go wrong is the TEST (a half closed that a later entry would still have moved) and the BOOKKEEPING behind it (pixels, checkpoint
slots of the closed half, the hand-over of an open half to the rest kernel).  The scenes put entries where either is most easily wrong.

Geometry: the scenes of tests/test_blend_bwd_dead_units.py (saturating half-plane groups of 24 entries in front of a crowd of 190
small Gaussians in ONE tile, list position = index there), changed where a family says so.

Families:
  dead, edge      one whole-frame group: every half with a list of >= 64 entries closes at its first boundary (edge: the crowd in the
                  frame's last tile, partial on 40 x 24, whose out-of-frame lanes keep T = 1 and do not veto).
  seam@K          the open column of the crowded tile is shut by a second group whose LAST entry is list position K = 63, 64, 65, 127,
                  128: the half closes at the boundary at or next behind the group -- as in the dead-units test one entry scales T by
                  >= 2^-6.6 and the margins are 2^-20 apart, so a seam moves a whole group and up to two of its entries may lie behind
                  the boundary.  seamin@128: the group BEGINS at 128, the half closes at 192.  Under fwd_variant 2 with segments of
                  64 (part 0 = 128 entries) seam@127 closes with the last chunk of part 0 and seamin@128 behind it (the later parts
                  must run); under fwd_variant 4 seam@63 / seam@127 are that pair.
  col, sub@0      one half closed, the other open through one pixel column / one 8 x 8 sub-tile (32 x 16 tiles; on 16 x 16 the one half
                  stays open).
  zero            every colour's green channel is exactly 0: C_g == 0 can never absorb anything by the strict test, nothing closes.
  dark            the front group has colour 2^-20 and brings T to ~2^-30 only; a bright, wide entry follows.  T <= 2^-26 holds, the
                  colour test does not (T K ~ 2^-30 against 2^-26 C ~ 2^-46): nothing closes, and a test of T alone would lose the
                  bright entry (CPU half).
  c50             the same T ~ 2^-30 under ordinary colours, and a later wide entry of colour 50: with the bound from the data
                  (K = 49.5) nothing closes; with a bound fixed at 1 the crowded tile would close in front of that entry (CPU half).
  nan             a NaN colour behind the closing group: the bound is NaN, nothing closes, NaN appears exactly as with the exit off.
  short, culled   a list shorter than one segment; a call with every Gaussian behind the camera.
  batch           `dead` and `c50` in one call (different maxima per image): bit-equal to the single calls.
  overflow        a capacity overflow under tests/workspace_guard.py's three fills (every list empty; the head still stores pixels).
The background is non-zero in every scene (0.05, 0.1, 0.15).

Every scene first asserts on the CPU (check_scene), from the oracle's projection and lists by an fp32 emulation of the kernel's
T-form update, which halves close and where, WITH MARGIN: at every boundary in front of a half's closing the half is open even under
a test four times laxer that accepts T up to 2^-20, at its closing it is closed under T < 2^-40 and products 2^8 smaller -- no half of
any scene is ambiguous, so the pattern cannot depend on the kernel's own rounding.  The emulation also keeps each closed half's
state and walks on: not one bit of C or D moves afterwards.

On the GPU, for frames of 64 x 32 and 40 x 24, both tile shapes, segments of 64 and 128, fwd_variant 1, 2, 4 and automatic, with
fwd_exit = 1 (automatic turns the exit on for launches of >= 8192 tile halves only -- test_cpu_automatic_follows_the_launch_size):
image, depth and the five gradients against the C oracle under the referee; the same seven arrays bitwise (NaN-aware) against the
same call with fwd_exit = -1; two runs bitwise equal.

CPU half: the same emulation under a CHANGED test.  A threshold of 2^-24 (`graded`: T = 2^-24.7 in front of a clamped entry of the
largest colour -- its addend is above half an ulp of C), a bound fixed at 1 (`c50`) and a test of T alone (`dark`) each close a half
whose frozen state then differs from the full walk's; the test as stated differs on no scene.
"""
import functools

import numpy as np
import pytest
import torch

import test_blend_bwd_dead_units as D
from helpers import assert_with_referee

GRADS = D.GRADS
FRAMES = [(64, 32), (40, 24)]
TILE_WS = [16, 32]
TUNINGS = {"s64": dict(seg_len=64), "s64v1": dict(seg_len=64, fwd_variant=1), "s64v2": dict(seg_len=64, fwd_variant=2),
           "s64v4": dict(seg_len=64, fwd_variant=4), "s128": dict(seg_len=128), "s128v2": dict(seg_len=128, fwd_variant=2)}
HEAD_ENTRIES = 384  # FGS_FWD_HEAD_ENTRIES (fgs_composite.hip)
SCENES = ["dead", "edge"] + [f"seam@{k}" for k in (63, 64, 65, 127, 128)] + ["seamin@128", "col", "sub@0", "zero", "dark", "c50", "nan",
                                                                             "short", "culled"]
N_DIM = 14        # front entries left at opacity 0.8 in `dark` / `c50`: T = (0.2 .. 0.25)^14 = 2^-32.5 .. 2^-28
WIDE_AT = 100     # list position of the wide entry of `c50` / `nan` (behind the first chunk boundary)
Q26, Q24, Q20, Q34, Q40 = (np.float32(2.0 ** -k) for k in (26, 24, 20, 34, 40))
A99 = np.float32(0.99)


def _base(name):
    return {"zero": "dead", "dark": "dead", "c50": "dead", "nan": "dead", "short": "dead", "culled": "dead", "graded": "dead"}.get(name, name)


@functools.lru_cache(maxsize=None)
def _scene(name, W, H, tile_w):
    """the five arrays (copies), gI, gD of a scene"""
    arrs, gI, gD, _, n_front = D._scene(_base(name), W, H, tile_w)
    pos, scale, quat, color, opacity = [a.copy() for a in arrs]
    N = len(opacity)
    if name == "zero":
        color[:, 1] = 0.0
    if name in ("dark", "c50"):
        opacity[N_DIM:n_front] = 0.0
    if name == "dark":
        color[:n_front] = np.float32(2.0 ** -20)
        color[n_front] = 1.0
        scale[n_front, :2] *= 4.0
    if name == "c50":
        color[WIDE_AT] = 50.0
        scale[WIDE_AT, :2] *= 4.0
    if name == "nan":
        color[WIDE_AT, 0] = np.nan
        scale[WIDE_AT, :2] *= 4.0
    if name == "graded":
        # CPU half only.  Every colour 0.9; the front group brings T to ~2^-25 (11 entries at 0.8, one at GRADED_OP, the rest at 0);
        # the deepest Gaussian of the scene (the last of every list) becomes a clamped entry -- opacity 1 on a pixel centre, a' = 1 --
        # on the crowded tile's pixel where T is largest
        color[:] = 0.9
        opacity[11] = GRADED_OP
        opacity[12:n_front] = 0.0
        j = N - D.N_ANCHOR - 1
        z = float(pos[j, 2])
        (u, v), r = GRADED_UV, 2.5
        pos[j] = [(u - W / 2) * -z / D.FOCAL, -(v - H / 2) * -z / D.FOCAL, z]
        scale[j] = [r / 3.0 * -z / D.FOCAL, r / 3.0 * -z / D.FOCAL, 1e-3 * r / 3.0 * -z / D.FOCAL]
        opacity[j] = 1.0
    if name == "short":
        keep = np.r_[0:40, N - D.N_ANCHOR:N]
        pos, scale, quat, color, opacity = [a[keep] for a in (pos, scale, quat, color, opacity)]
    if name == "culled":
        pos[:, 2] = -pos[:, 2]  # behind the camera
    return [pos, scale, quat, color, opacity], gI, gD


# `graded`: with these the crowded tile's largest T at its first boundary is 2^-24.67, on pixel (0, 0).  The changed test closes there
# (T K_c < 2^-24 C needs T < 2^-24.0, T K_d < 2^-24 D needs T < 2^-24.56) and the clamped entry's addend T K_c = 2^-24.84 is above
# half an ulp of C = 0.9 (2^-25): the window for T is (2^-24.83, 2^-24.56).
GRADED_OP = 0.83
GRADED_UV = (0.0, 0.0)


@functools.lru_cache(maxsize=None)
def _reference(name, W, H, tile_w, backward=True):
    from oracle import fgs_oracle as orc
    arrs, gI, gD = _scene(name, W, H, tile_w)
    ocam = orc.make_camera(np.eye(4, dtype=np.float32), D.FOCAL, D.FOCAL, W / 2, H / 2, W, H)
    r32 = orc.render(*arrs, ocam, bg=D.BG)
    if not backward:
        return r32, None, None, None
    g32 = orc.render_backward(r32, gI, gD)
    with orc.fp64():
        r64 = orc.render(*arrs, ocam, bg=D.BG)
        g64 = orc.render_backward(r64, gI, gD)
    return r32, g32, r64, g64


def _fma(a, b, c):
    """fp32 fma through fp64 (the product of two fp32 values is exact there)"""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)


def _holds(st, reg, inframe, Kc, Kd, q, qT):
    """the absorbing test on the pixels `reg` of the frame: T <= qT and T K < q |X|, on every in-frame pixel (none: holds)"""
    Cr, Cg, Cb, Dm, T = (a[reg][inframe] for a in st)
    with np.errstate(invalid="ignore", over="ignore"):
        tc, td = T * Kc, T * Kd
        ok = (T <= qT) & (tc < q * np.abs(Cr)) & (tc < q * np.abs(Cg)) & (tc < q * np.abs(Cb)) & (td < q * np.abs(Dm))
    return bool(ok.all())


RULES = {  # name -> (K_colour override, q, qT, colour / depth products tested)
    "stated": (None, Q26, Q26, True),
    "thr24": (None, Q24, Q24, True),
    "k1": (1.0, Q26, Q26, True),
    "t_only": (None, Q26, Q26, False),
}


@functools.lru_cache(maxsize=None)
def _emulate(name, W, H, tile_w):
    """Walk the whole frame in depth order with the kernel's T-form update (a pixel's state after a tile-list prefix is its state
    after the global prefix: only entries whose bbox holds the pixel move it, and they are in its tile's list).  At every 64-entry
    boundary of every tile list, per 16 x 16 half: the margin class ('open' / 'closed' / 'ambiguous') and whether each rule of
    RULES holds; per rule the half's state at its first closing is kept and compared, at the end, with the full walk's.
    -> dict(bounds={(tile, half): [(position, class, {rule: holds})]}, moved={rule: [(tile, half)]}, lens={tile: entries})"""
    from oracle import fgs_oracle as orc
    r32 = _reference(name, W, H, tile_w, backward=False)[0]
    arrs = _scene(name, W, H, tile_w)[0]
    color, opacity = arrs[3], arrs[4]
    mean, conic, bbox, depth = (r32.proj[k] for k in ("mean2d", "conic", "bbox", "depth"))
    mean, conic, depth = mean.astype(np.float32), conic.astype(np.float32), depth.astype(np.float32)
    order = [int(i) for i in r32.vis_sorted]
    ranges, ids = orc.tile_lists(r32.vis_sorted, bbox, W, H, tile_w=tile_w)
    tiles_x = -(-W // tile_w)
    step_of = {g: k for k, g in enumerate(order)}
    events, lens = {}, {}
    listed = np.zeros(len(opacity), bool)
    for t in range(len(ranges) - 1):
        lst = [int(i) for i in ids[ranges[t]:ranges[t + 1]]]
        lens[t] = len(lst)
        listed[lst] = True
        assert [step_of[g] for g in lst] == sorted(step_of[g] for g in lst)  # a tile list is a subsequence of the depth order
        for b in range(64, len(lst), 64):
            events.setdefault(step_of[lst[b - 1]], []).append((t, b))
    with np.errstate(invalid="ignore"):
        cm = np.abs(A99 * color[listed]) if listed.any() else np.zeros((1, 3), np.float32)
        Kc = np.float32(np.nan) if np.isnan(cm).any() else max(np.float32(cm.max()), np.float32(max(abs(x) for x in D.BG)))
        Kd = np.float32(np.abs(A99 * depth[listed]).max()) if listed.any() else np.float32(0)
    st = [np.zeros((H, W), np.float32) for _ in range(4)] + [np.ones((H, W), np.float32)]
    bounds, frozen = {}, {r: {} for r in RULES}

    def region(t, h):
        X0, Y0 = (t % tiles_x) * tile_w + 16 * h, (t // tiles_x) * 16
        reg = (slice(Y0, min(Y0 + 16, H)), slice(X0, min(X0 + 16, W)))
        return reg, np.ones((max(0, min(Y0 + 16, H) - Y0), max(0, min(X0 + 16, W) - X0)), bool)

    for k, i in enumerate(order):
        x0, x1, y0, y1 = (int(v) for v in bbox[i])
        if x0 < x1 and y0 < y1:
            reg = (slice(y0, y1), slice(x0, x1))
            dx = (np.arange(x0, x1).astype(np.float32) - mean[i, 0])[None, :]
            dy = (np.arange(y0, y1).astype(np.float32) - mean[i, 1])[:, None]
            qd = conic[i, 0] * dx * dx + conic[i, 1] * dx * dy + conic[i, 2] * dy * dy
            with np.errstate(invalid="ignore", over="ignore"):
                al = np.minimum(A99, np.float32(opacity[i]) * np.exp(np.float32(-0.5) * qd)).astype(np.float32)
                w = (np.minimum(al / A99, np.float32(1)) * st[4][reg]).astype(np.float32)
                for c in range(3):
                    st[c][reg] = _fma(w, A99 * color[i, c], st[c][reg])
                st[3][reg] = _fma(w, A99 * depth[i], st[3][reg])
                st[4][reg] = _fma(w, -A99, st[4][reg])
        for (t, b) in events.get(k, []):
            for h in range(tile_w // 16):
                reg, inf = region(t, h)
                sure_closed = _holds(st, reg, inf, Kc, Kd, Q34, Q40)
                sure_open = not _holds(st, reg, inf, Kc, Kd, Q24, Q20)
                cls = "closed" if sure_closed else ("open" if sure_open else "ambiguous")
                holds = {}
                for r, (kov, q, qT, prod) in RULES.items():
                    kc = Kc if kov is None else np.float32(kov)
                    holds[r] = _holds(st, reg, inf, kc, Kd, q, qT) if prod else bool((st[4][reg][inf] <= qT).all())
                    if holds[r] and (t, h) not in frozen[r]:
                        frozen[r][(t, h)] = [a[reg].copy() for a in st[:4]]
                bounds.setdefault((t, h), []).append((b, cls, holds))
    moved = {r: [] for r in RULES}
    for r in RULES:
        for (t, h), fz in frozen[r].items():
            reg, _ = region(t, h)
            if any(a[reg].tobytes() != f.tobytes() for a, f in zip(st[:4], fz)):
                moved[r].append((t, h))
    return dict(bounds=bounds, moved=moved, lens=lens)


def _closing(bl):
    """first boundary at which a half closes under the stated test, with the margin classes of every boundary up to it"""
    for b, cls, holds in bl:
        if holds["stated"]:
            return b, cls
        assert cls == "open", (b, cls)
    return None, None


def _expected(name, tile_w, half):
    """closing position of the crowded tile's halves: a number, None (stays open), or 'any'"""
    fam, k = name.split("@")[0], D._arg(name)
    if fam in ("dead", "edge"):
        return 64
    if fam in ("seam", "seamin"):
        col_half = tile_w // 16 - 1  # the open column is the tile's last
        if half != col_half:
            return 64
        return 64 * ((k + 61) // 64) if fam == "seam" else k + 64
    if fam == "col":
        return None if half == tile_w // 16 - 1 else 64
    if fam == "sub":
        return None if half == 0 else 64
    return None


def check_scene(name, W, H, tile_w):
    """which halves close, and where, with margin; -> {(tile, half): closing position | None}"""
    em = _emulate(name, W, H, tile_w)
    closes = {}
    for key, bl in em["bounds"].items():
        pos, cls = _closing(bl)
        assert pos is None or cls == "closed", (name, key, pos, cls)  # closed WITH margin where it closes
        closes[key] = pos
    assert not em["moved"]["stated"], (name, em["moved"]["stated"])  # nothing moves behind a closing
    if name in ("short", "culled"):
        assert not em["bounds"] and (name == "short" or not any(em["lens"].values())) and all(n < 64 for n in em["lens"].values())
        return closes
    ct = D._crowded_tile(_base(name), W, H, tile_w)
    assert em["lens"][ct] > 192
    for h in range(tile_w // 16):
        assert closes[(ct, h)] == _expected(name, tile_w, h), (name, tile_w, h, closes[(ct, h)])
    if name in ("zero", "dark", "c50", "nan"):
        assert all(v is None for v in closes.values()), (name, closes)
    if name in ("dead", "edge"):
        assert all(v == 64 for v in closes.values())
    return closes


def _head_len(n, seg_len, parts):
    nseg = -(-n // seg_len)
    spp = -(-nseg // parts)
    return min(n, (nseg if parts == 1 else min(spp, max(1, HEAD_ENTRIES // seg_len))) * seg_len), min(n, spp * seg_len)


def test_cpu_closings_fall_on_both_sides_of_part_0():
    """the pairs the docstring names: a half that closes with the last chunk of part 0, and one that closes one boundary behind it"""
    for tile_w in TILE_WS:
        for W, H in FRAMES:
            for inside, behind, seg_len, parts in (("seam@127", "seamin@128", 64, 2), ("seam@63", "seam@127", 64, 4), ("seam@127", "seamin@128", 128, 2)):
                for name, want_in in ((inside, True), (behind, False)):
                    closes = check_scene(name, W, H, tile_w)
                    ct = D._crowded_tile(name, W, H, tile_w)
                    h = tile_w // 16 - 1
                    head, part0 = _head_len(_emulate(name, W, H, tile_w)["lens"][ct], seg_len, parts)
                    assert head == part0  # the head covers part 0 here
                    assert (closes[(ct, h)] == part0) if want_in else (closes[(ct, h)] > part0), (name, tile_w, seg_len, parts)


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("tile_w", TILE_WS)
@pytest.mark.parametrize("name", SCENES)
def test_cpu_patterns_hold_with_margin(name, tile_w, frame):
    check_scene(name, frame[0], frame[1], tile_w)


@pytest.mark.parametrize("tile_w", TILE_WS)
def test_cpu_changed_tests_are_told_apart(tile_w):
    """a threshold of 2^-24, a bound fixed at 1 and a test of T alone each close a half that a later entry still moves"""
    W, H = 64, 32
    for name, rule in (("graded", "thr24"), ("c50", "k1"), ("dark", "t_only")):
        em = _emulate(name, W, H, tile_w)
        ct = D._crowded_tile("dead", W, H, tile_w)
        assert (ct, 0) in em["moved"][rule], (name, rule, em["moved"][rule])
        assert not em["moved"]["stated"]
        assert all(not holds["stated"] for b, cls, holds in em["bounds"][(ct, 0)])


def test_cpu_automatic_follows_the_launch_size():
    """fwd_exit = 0 turns the exit on from 8192 tile halves per launch; 1 and -1 force it; only the depth-split forward has it"""
    from fresnel_amd import _binding as B

    def on(*dims, **kw):
        L = B.saved_layout(B.make_dims(*dims, **kw))
        return L.fwd_open < L.total_bytes

    assert on(8, 32768, 512, 512) and on(8, 32768, 512, 512, tuning=dict(tile_w=16))  # config 3: 4096 x 2 and 8192 x 1 halves
    assert not on(16, 8192, 256, 256) and not on(7, 32768, 512, 512)                    # config 2: 4096
    assert on(16, 8192, 256, 256, tuning=dict(fwd_exit=1)) and not on(8, 32768, 512, 512, tuning=dict(fwd_exit=-1))
    assert on(2, 100, 64, 32, tuning=dict(fwd_exit=1, fwd_variant=1))
    assert not on(2, 100, 64, 32, use_phase=True, tuning=dict(fwd_exit=1)) and not on(2, 100, 64, 32, saturation_skip=True, tuning=dict(fwd_exit=1))
    d = B.make_dims(2, 100, 64, 32, tuning=dict(fwd_exit=-1, fwd_variant=2))
    assert d.fwd_variant == 2 | B.FWD_EXIT_OFF and B.make_dims(2, 100, 64, 32, tuning=dict(fwd_exit=1)).fwd_variant == B.FWD_EXIT_ON
    for bad in (dict(fwd_exit=2), dict(fwd_exit=-2), dict(fwd_exit=1, fwd_variant=-2)):  # (the row-split forward has no exit)
        with pytest.raises(B.FgsError):
            B.make_dims(2, 100, 64, 32, tuning=bad)
    with pytest.raises(B.FgsError):  # both flags at once
        B.workspace_bytes(B.make_dims(2, 100, 64, 32, tuning=dict(fwd_variant=B.FWD_EXIT_ON | B.FWD_EXIT_OFF)))


# ---- GPU ----
gpu = pytest.mark.gpu


def _hip(name, W, H, tile_w, tuning, fwd_exit=1):
    arrs, gI, gD = _scene(name, W, H, tile_w)
    return D._hip(arrs, W, H, gI, gD, dict(tile_w=tile_w, fwd_exit=fwd_exit, **tuning))


def _same_bits(a, b, what):
    for k in GRADS + ["image", "depth"]:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{what} {k}"


@gpu
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("tile_w", TILE_WS)
@pytest.mark.parametrize("name", SCENES)
def test_scene_vs_oracle_and_exit_off(name, tile_w, frame):
    W, H = frame
    check_scene(name, W, H, tile_w)
    r32, g32, r64, g64 = _reference(name, W, H, tile_w)
    for tun, tuning in TUNINGS.items():
        what = f"{name} {W}x{H} tile_w={tile_w} {tun}"
        got = _hip(name, W, H, tile_w, tuning)
        _same_bits(got, _hip(name, W, H, tile_w, tuning, fwd_exit=-1), what + " against fwd_exit=-1:")
        _same_bits(got, _hip(name, W, H, tile_w, tuning), what + " second run:")
        if name == "nan":  # (the image's clamp turns a NaN into 0 and the gradients take NaNs of their own: the statement is the
            continue       # bitwise one above, NaN payloads included)
        if name == "culled":
            assert all(np.array_equal(got["image"][c], np.full((H, W), np.float32(D.BG[c]))) for c in range(3)), what
            assert not any(got[k].any() for k in GRADS) and not got["depth"].any(), what
            continue
        assert_with_referee(got["image"], r32.image, r64.image, f"{what} image")
        assert_with_referee(got["depth"], r32.depth, r64.depth, f"{what} depth")
        for k in GRADS:
            assert_with_referee(got[k], g32[k], g64[k], f"{what} grad_{k}")


@gpu
@pytest.mark.parametrize("tile_w", TILE_WS)
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_marks_match_the_cpu_pattern(frame, tile_w):
    """saved.fwd_open, the word the head kernel leaves per tile half, is what the emulation says: 0 where the half closed inside the
    head's reach or its list ended there, 1 where the rest kernel has to go on"""
    from fresnel_amd.renderer import Camera, TileBasedRenderer, inspect_saved
    W, H = frame
    dev = D._cuda()
    seen = set()
    for name in ("dead", "col", "sub@0", "seam@127", "seamin@128", "zero", "short"):
        closes = check_scene(name, W, H, tile_w)
        lens = _emulate(name, W, H, tile_w)["lens"]
        for tun in ("s64v2", "s64v4", "s128v2", "s64v1"):
            seg_len, parts = TUNINGS[tun]["seg_len"], TUNINGS[tun]["fwd_variant"]
            ts = [torch.from_numpy(np.ascontiguousarray(a[None])).to(dev) for a in _scene(name, W, H, tile_w)[0]]  # (a batch of one)
            ren = TileBasedRenderer(W, H, background=D.BG)
            ren.tuning = dict(tile_w=tile_w, fwd_exit=1, **TUNINGS[tun])
            img = ren(*[t.requires_grad_(True) for t in ts], Camera(D.FOCAL, D.FOCAL, W / 2, H / 2, W, H), return_depth=True)[0]
            node = img.grad_fn
            marks = inspect_saved(node.saved_tensors[-1], node.dims)["fwd_open"][0].cpu().numpy()
            for t, n in lens.items():
                head = _head_len(n, seg_len, parts)[0]
                for h in range(tile_w // 16):
                    pos = closes.get((t, h))
                    want = int(head < n and not (pos is not None and pos <= head))
                    assert int(marks[t, h]) == want, (name, tun, t, h, n, pos, head, int(marks[t, h]))
                    seen.add((want, pos is not None))
    assert seen >= {(0, True), (0, False), (1, True), (1, False)}  # closed in the head / list ended; closes behind it / never closes


@gpu
@pytest.mark.parametrize("tile_w", TILE_WS)
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_batch_equals_single_calls(frame, tile_w):
    """`dead` (every half closes, K ~ 0.9) and `c50` (nothing closes, K = 49.5) in ONE call: the bound is per image"""
    W, H = frame
    assert all(v == 64 for v in check_scene("dead", W, H, tile_w).values())
    assert all(v is None for v in check_scene("c50", W, H, tile_w).values())
    a, gI, gD = _scene("dead", W, H, tile_w)
    b = _scene("c50", W, H, tile_w)[0]
    for tun in ("s64", "s64v2", "s128"):
        both = D._hip([np.stack([x, y]) for x, y in zip(a, b)], W, H, np.stack([gI, gI]), np.stack([gD, gD]),
                      dict(tile_w=tile_w, fwd_exit=1, **TUNINGS[tun]))
        for i, single in enumerate((_hip("dead", W, H, tile_w, TUNINGS[tun]), _hip("c50", W, H, tile_w, TUNINGS[tun]))):
            for k in GRADS + ["image", "depth"]:
                assert both[k][i].tobytes() == single[k].tobytes(), (tun, i, k)


@gpu
@pytest.mark.parametrize("tuning", [dict(tile_w=32, seg_len=64, fwd_exit=1), dict(tile_w=16, seg_len=128, fwd_variant=1, fwd_exit=1)],
                         ids=["tw32-seg64", "tw16-seg128-v1"])
def test_capacity_overflow_under_the_guard_fills(tuning):
    """every list empty: the head kernel still owns every pixel and mark, and nothing reads a fill"""
    import test_workspace_capacity as C
    import workspace_guard as WG
    Dn = C._oracle_duplicates("aniso", tuning["tile_w"])
    inp = C._inputs()
    call = C._Call(inp, workspace=Dn // 4, tuning=tuning)
    runs = WG.run_patterns(call, inp, C._mods())
    assert int(call.layout.dup_capacity) == Dn // 4
    for name, out in runs.items():
        assert int(out["st_counters"][1]) == 1 and int(out["st_list_len"].abs().sum()) == 0, name
        for k in ("image", "depth"):
            assert bool((out[k].view(torch.int32) == C.QNAN).all()), (name, k)
        for k in [g for g in out if g.startswith("grad_")]:
            assert not bool(out[k].view(torch.int32).any()), (name, k)
