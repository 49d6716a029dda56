"""Zero units of k_composite_bwd (fgs_composite.hip; tuning key bwd_zero = the FGS_BWD_ZERO_ON / _OFF flag of FgsDims.fwd_variant;
automatic turns the path on for launches of >= 8192 tile halves only, so every call here forces it with bwd_zero = 1).

A DEAD unit (every in-frame pixel restarts with T == +0.0f) whose S is +-0 on every lane of every sub-tile gets its gradient rows
written as zeros without a walk; a dead unit with only SOME sub-tiles all-zero walks with those sub-tiles masked.  S is exactly zero
behind a half's closing (the exiting forward stores the closing slot and the pixel's final state from the same registers, and the
prologue forms Total and the checkpoint sum as the same FMA chain), a rounding residue in a dead unit in FRONT of a closing.  The
rows are the bits the full dead walk gives, so every statement here is BITWISE against the same call with bwd_zero = -1, and what can
go wrong is (1) the predicate -- a unit with a non-zero (or NaN) S taken for zero loses gradients --, (2) the sign of a zero: on
32 x 16 tiles the walk's fold makes row floats 1 and 3 (sum dG dy, sum dG dx dy) -0.0f when ((float)(Y0 + 7) - v) + 8.0f < 0 in fp32 --
the Gaussian's centre below the tile's last row -- and +0.0f otherwise, every other float and every float on 16 x 16 tiles +0.0f --,
(3) the one-lane-per-entry row store at the ends of a list.

Scenes: the geometry of tests/test_blend_bwd_dead_units.py (D) and tests/test_blend_fwd_absorbed.py (A): a saturating whole-frame group
of 24 entries in front of a crowd of 190 small Gaussians in ONE tile (list position = index there).  With the exit on, every half of
`dead` closes at list position 64 (A.check_scene), so every later unit is a zero unit.
  rows        `dead` with crowd entries behind position 64 moved BELOW the crowded tile's rows (v = 18.5: -0), ABOVE them (v = -1.5),
              left inside, and onto v = Y0 + 15 exactly and one fp32 step either side of it -- the -0 rule's boundary, v read back from the
              oracle's projection, which is k_project's bit for bit.
  special     opacity 0, a negative opacity and a clamp-flagged entry (opacity 0.995 on a pixel centre) in a zero unit.
  len@L       the crowded tile's list cut or padded to 128 + L entries, L = 1, 2, 63, 64, 65, 127, 128: last units of every length
              at which the row store's lane loop ends differently (64-entry segments: L mod 64).
  seam@127, seamin@128 (D / A scenes)  one half of the 32 x 16 crowded tile closes at 64, the other later or -- where the head kernel
              does not reach (fwd_variant 4) -- never: dead units with ONE half behind its closing (the sub-tile mask).
  col, row, sub@0 (D scenes)  a dead-looking unit with one open column / row / sub-tile that carries a probe whose reference grad_colors is
              >= 1e-2 of max: it is live, must not take the zero path, and the probe's gradient passes the referee.
  zero        (A scene: green channel 0, nothing ever closes) and EVERY scene with fwd_exit = -1: dead units in front of any closing,
              T == 0 and S a residue.
  nan / inf   a NaN, an Inf upstream gradient on ONE closed pixel of `dead`: S is NaN there, the unit keeps the dead walk; the gradients
              are compared bitwise with the switch-off run (no referee: they hold NaNs), image and depth against the oracle.
  overflow    a capacity overflow under tests/workspace_guard.py's three fills.
  batch       `dead` and its opacity-0.05 twin (no dead unit) in one call, bit-equal to the single calls.
Grid: frames 64 x 32 and 40 x 24, both tile shapes, segments of 64 and 128, fwd_exit 1 and -1.  For every case: the seven outputs
bitwise equal to the bwd_zero = -1 call and to a second run, the referee against the C oracle, and -- PATH TAKEN -- saved.fwd_close,
seg_off and ranges of the very call say that the crowded tile holds the units the scene claims (all halves behind their closing: zero
units; one half: mixed; none: the full dead walk or the general one).

CPU half: the fold of the dead walk emulated in numpy float32 over the scenes' projected records gives the sign rule, and "every float
+0" is told apart from it by the rows scene on 32 x 16 tiles."""
import functools

import numpy as np
import pytest
import torch

import test_blend_bwd_dead_units as D
import test_blend_fwd_absorbed as A
from helpers import assert_with_referee

GRADS = D.GRADS
OUTS = GRADS + ["image", "depth"]
FRAMES = [(64, 32), (40, 24)]
TILE_WS = [16, 32]
SEGS = {"s64": dict(seg_len=64), "s128": dict(seg_len=128)}
EXITS = [1, -1]
LENS = (1, 2, 63, 64, 65, 127, 128)
ROW_AT = {"below": (70, 131, 200), "above": (72, 133, 201), "on": (74, 135), "under": (75, 136), "over": (76, 137)}  # crowd positions >= 64
SPECIAL_AT = {"op0": 150, "opneg": 151, "clamp": 152}
BAD_PIXEL = (5, 6)  # (x, y) of the pixel whose upstream gradient is NaN / Inf: in the crowded tile of `dead` on every frame
gpu = pytest.mark.gpu
f32 = np.float32


def _ocam(W, H):
    from oracle import fgs_oracle as orc
    return orc.make_camera(np.eye(4, dtype=np.float32), D.FOCAL, D.FOCAL, W / 2, H / 2, W, H)


def _place(arrs, j, u, v, r, W, H):
    """Gaussian j at pixel (u, v) with bbox radius ~r, its depth kept (D._scene's construction)"""
    pos, scale = arrs[0], arrs[1]
    z = float(pos[j, 2])
    s = r / 3.0 * -z / D.FOCAL
    pos[j] = [(u - W / 2) * -z / D.FOCAL, -(v - H / 2) * -z / D.FOCAL, z]
    scale[j] = [s, 0.6 * s, 1e-3 * s]


def _projected_v(arrs, j, W, H):
    from oracle import fgs_oracle as orc
    return f32(orc.project(arrs[0][j:j + 1], arrs[1][j:j + 1], arrs[2][j:j + 1], _ocam(W, H))["mean2d"][0, 1])


def _set_v_exact(arrs, j, target, W, H):
    """step pos.y of Gaussian j by fp32 neighbours until the projection (the oracle's = k_project's, bit for bit) gives v == target"""
    target = f32(target)
    for _ in range(4000):
        v = _projected_v(arrs, j, W, H)
        if v == target:
            return
        # v = cy - y f / -z falls as y grows
        arrs[0][j, 1] = np.nextafter(arrs[0][j, 1], f32(-np.inf) if v < target else f32(np.inf))
    raise AssertionError((j, float(target)))


@functools.lru_cache(maxsize=None)
def _scene(name, W, H, tile_w):
    """-> (the five arrays, gI, gD, claim): claim = what the crowded tile's units behind the first are, with the exit on --
    'zero', 'mixed' (32 x 16 tiles; 'zero' / other on 16 x 16), 'live', 'residue' -- or None where the scene says nothing"""
    fam = name.split("@")[0]
    if fam in ("seam", "seamin", "col", "row", "sub"):
        arrs, gI, gD = D._scene(name, W, H, tile_w)[:3]
        return [a.copy() for a in arrs], gI, gD, ("live" if fam in ("col", "row", "sub") else "mixed")
    if name == "zero":
        arrs, gI, gD = A._scene("zero", W, H, tile_w)
        return [a.copy() for a in arrs], gI, gD, "residue"
    arrs, gI, gD, _, n_front = D._scene("dead", W, H, tile_w)
    arrs, gI, gD = [a.copy() for a in arrs], gI.copy(), gD.copy()
    pos, scale, quat, color, opacity = arrs
    if name == "rows":
        for j in ROW_AT["below"]:
            _place(arrs, j, 6.0 + 0.37 * (j % 5), 18.5, 4.5, W, H)   # bbox rows 14 .. 23: in the tile, centre below it
        for j in ROW_AT["above"]:
            _place(arrs, j, 7.0 + 0.41 * (j % 5), -1.5, 4.5, W, H)   # bbox rows 0 .. 3, centre above the frame
        for key, step in (("on", 0), ("under", -1), ("over", 1)):
            for j in ROW_AT[key]:
                _place(arrs, j, 5.0 + 0.29 * (j % 7), 15.0, 3.0, W, H)
                t = f32(15.0)
                t = np.nextafter(t, f32(np.inf)) if step > 0 else (np.nextafter(t, f32(-np.inf)) if step < 0 else t)
                _set_v_exact(arrs, j, t, W, H)
    if name == "special":
        for key, j in SPECIAL_AT.items():
            _place(arrs, j, D.CENTRE[0], D.CENTRE[1], 3.0, W, H)
        opacity[SPECIAL_AT["op0"]], opacity[SPECIAL_AT["opneg"]], opacity[SPECIAL_AT["clamp"]] = 0.0, -0.3, 0.995
    if fam == "len":
        n = 128 + int(name[4:])
        n_list, N = n_front + D.N_CROWD, len(opacity)
        anchors = np.arange(N - D.N_ANCHOR, N)
        if n <= n_list:
            keep = np.r_[0:n, anchors]
            arrs = [a[keep] for a in arrs]
        else:  # pad: copies of crowd entries behind everything else of the list (deeper; same pixel position and size)
            src = n_front + 6 + np.arange(n - n_list)
            extra = [a[src].copy() for a in arrs]
            z_new = -2.0 - 0.004 * (N + np.arange(len(src)))
            k = (z_new / extra[0][:, 2]).astype(np.float32)
            extra[0] = (extra[0] * k[:, None]).astype(np.float32)
            extra[1] = (extra[1] * k[:, None]).astype(np.float32)
            keep = np.r_[0:n_list, anchors]
            arrs = [np.concatenate([a[keep[:n_list]], e, a[anchors]]) for a, e in zip(arrs, extra)]
    if name in ("nan", "inf"):
        gI[1, BAD_PIXEL[1], BAD_PIXEL[0]] = np.nan if name == "nan" else np.inf
    return arrs, gI, gD, "zero"


@functools.lru_cache(maxsize=None)
def _reference(name, W, H, tile_w):
    from oracle import fgs_oracle as orc
    arrs, gI, gD, _ = _scene(name, W, H, tile_w)
    ocam = _ocam(W, H)
    r32 = orc.render(*arrs, ocam, bg=D.BG)
    g32 = orc.render_backward(r32, gI, gD)
    with orc.fp64():
        r64 = orc.render(*arrs, ocam, bg=D.BG)
        g64 = orc.render_backward(r64, gI, gD)
    return r32, g32, r64, g64


def _same_bits(a, b, what):
    for k in OUTS:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{what} {k}"


def _run(arrs, W, H, gI, gD, tuning, batch=False):
    """D._hip, which also returns what saved.fwd_close / seg_off / ranges of the call say"""
    from fresnel_amd.renderer import Camera, TileBasedRenderer, inspect_saved
    dev = D._cuda()
    if not batch:  # a batch of one: the module's batched call, whose autograd node holds the saved state
        arrs, gI, gD = [a[None] for a in arrs], gI[None], gD[None]
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True) for a in arrs]
    ren = TileBasedRenderer(W, H, background=D.BG)
    ren.tuning = dict(tuning)
    img, dep = ren(*ts, Camera(D.FOCAL, D.FOCAL, W / 2, H / 2, W, H), return_depth=True)
    st = inspect_saved(img.grad_fn.saved_tensors[-1], img.grad_fn.dims)
    saved = dict(ranges=st["ranges"].cpu().numpy().astype(np.int64), seg_off=st["seg_off"].cpu().numpy().astype(np.int64),
                 seg_len=int(st["layout"].seg_len), units=int(st["counters"][2]),
                 fwd_close=st["fwd_close"].cpu().numpy().astype(np.int64) if "fwd_close" in st else None)
    ((img * torch.from_numpy(gI).to(dev)).sum() + (dep * torch.from_numpy(gD).to(dev)).sum()).backward()
    out = {k: t.grad.detach().cpu().numpy() for k, t in zip(GRADS, ts)}
    out["image"], out["depth"] = img.detach().cpu().numpy(), dep.detach().cpu().numpy()
    if not batch:
        out = {k: v[0] for k, v in out.items()}
    return out, saved


def unit_kinds(saved, image, tile, tile_w):
    """the units of a tile behind its first, from the call's own saved state: 'closed' (every half behind its closing slot -- S is
    exactly zero: a zero unit), 'half' (one of two), 'open' (none).  Also checks that seg_off counts ceil(n / seg_len) units."""
    lo, hi = saved["ranges"][image, tile]
    n, seg_len = int(hi - lo), saved["seg_len"]
    T = saved["ranges"].shape[1]
    nseg = -(-n // seg_len)
    assert saved["seg_off"][image * T + tile + 1] - saved["seg_off"][image * T + tile] == max(nseg, 1 if n == 0 else nseg) or n == 0
    halves = tile_w // 16
    kinds = []
    for seg in range(1, nseg):
        behind = 0
        for h in range(halves):
            k = -1 if saved["fwd_close"] is None else int(saved["fwd_close"][image, tile, h])
            behind += int(0 <= k <= seg)
        kinds.append("closed" if behind == halves else ("half" if behind else "open"))
    return kinds, n


CASES = ["rows", "special", "seam@127", "seamin@128", "col", "row", "sub@0", "zero", "nan", "inf"] + [f"len@{L}" for L in LENS]


@gpu
@pytest.mark.parametrize("seg", sorted(SEGS))
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("tile_w", TILE_WS)
@pytest.mark.parametrize("name", CASES)
def test_scene_bitwise_referee_and_path(name, tile_w, frame, seg):
    W, H = frame
    arrs, gI, gD, claim = _scene(name, W, H, tile_w)
    r32, g32, r64, g64 = _reference(name, W, H, tile_w)
    fam = name.split("@")[0]
    ct = D._crowded_tile("dead", W, H, tile_w)
    # seam / seamin with segments of 64: four list parts (the head kernel walks 64 entries: the column's half never closes) and one
    # (it walks the whole list: both halves close, one behind the other)
    splits = [dict()] + ([dict(fwd_variant=4), dict(fwd_variant=1)] if fam in ("seam", "seamin") and seg == "s64" else [])
    seen = set()
    for split in splits:
        for fwd_exit in EXITS:
            tuning = dict(tile_w=tile_w, fwd_exit=fwd_exit, bwd_zero=1, **SEGS[seg], **split)
            what = f"{name} {W}x{H} tile_w={tile_w} {seg} {split} fwd_exit={fwd_exit}"
            got, saved = _run(arrs, W, H, gI, gD, tuning)
            off, _ = _run(arrs, W, H, gI, gD, dict(tuning, bwd_zero=-1))
            _same_bits(got, off, what + " against bwd_zero=-1:")
            _same_bits(got, _run(arrs, W, H, gI, gD, tuning)[0], what + " second run:")
            assert_with_referee(got["image"], r32.image, r64.image, f"{what} image")
            assert_with_referee(got["depth"], r32.depth, r64.depth, f"{what} depth")
            if name in ("nan", "inf"):
                assert not np.isfinite(got["colors"]).all() or not np.isfinite(got["positions"]).all(), what  # the bad gradient arrived
            else:
                for k in GRADS:
                    assert_with_referee(got[k], g32[k], g64[k], f"{what} grad_{k}")
            # ---- path taken: what the call's own saved state says about the crowded tile's units ----
            kinds, n = unit_kinds(saved, 0, ct, tile_w)
            seen.update(kinds)
            if fam == "len":
                L = int(name[4:])
                assert n == 128 + L and len(kinds) == -(-n // saved["seg_len"]) - 1, (what, n)
            if fwd_exit == -1:
                assert kinds and set(kinds) == {"open"}, (what, kinds)  # no closing slot: dead units hold residues (or live ones)
            elif claim == "zero":
                assert kinds and set(kinds) == {"closed"}, (what, kinds)  # every unit behind the first is a zero unit
            elif claim in ("live", "residue"):
                want = {"open"} if tile_w == 16 or claim == "residue" else {"half"}  # (32 x 16: the other half closes -- the units are LIVE)
                assert kinds and set(kinds) <= want | {"open"}, (what, kinds)
                assert "closed" not in kinds, (what, kinds)
    if claim == "mixed" and tile_w == 32:
        # units with one half behind its closing and the other not (yet), and units behind both; the emulation of the dead-units
        # test says, with margin, that the crowded tile's units behind the second group are dead
        # (segments of 64: with 128 the crowded tile has ONE later unit, which in seamin@128 restarts live)
        if seg == "s64":
            assert "half" in seen and "closed" in seen, (name, seg, seen)
            pat = D._pattern(name, W, H, tile_w, 64, 0)
            mine = sorted(s_ for (t, s_) in pat if t == ct)
            assert pat[(ct, mine[-1])] == "dead" and "ambiguous" not in pat.values(), (name, seg, pat)
    if claim == "live":
        D.check_scene(name, W, H, tile_w, dict(SEGS[seg]))  # live through the open region alone, with a probe >= 1e-2 of max in every unit
    if claim == "residue":
        assert set(D.check_scene("dead", W, H, tile_w, dict(SEGS[seg])).values()) == {"dead"}  # (the geometry of `dead`: T == 0, never closed)


@gpu
@pytest.mark.parametrize("seg", sorted(SEGS))
@pytest.mark.parametrize("tile_w", TILE_WS)
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_batch_equals_single_calls(frame, tile_w, seg):
    """a saturating image (every later unit a zero unit) and its opacity-0.05 twin (no dead unit) in ONE call"""
    W, H = frame
    a, gI, gD = D._scene("dead", W, H, tile_w)[:3]
    b = D._scene("dead", W, H, tile_w, 0.05)[0]
    ct = D._crowded_tile("dead", W, H, tile_w)
    for fwd_exit in EXITS:
        tuning = dict(tile_w=tile_w, fwd_exit=fwd_exit, bwd_zero=1, **SEGS[seg])
        both, saved = _run([np.stack([x, y]) for x, y in zip(a, b)], W, H, np.stack([gI, gI]), np.stack([gD, gD]), tuning, batch=True)
        off, _ = _run([np.stack([x, y]) for x, y in zip(a, b)], W, H, np.stack([gI, gI]), np.stack([gD, gD]), dict(tuning, bwd_zero=-1), batch=True)
        _same_bits(both, off, f"batch {tuning} against bwd_zero=-1:")
        for i, arrs in enumerate((a, b)):
            single = _run(arrs, W, H, gI, gD, tuning)[0]
            for k in OUTS:
                assert both[k][i].tobytes() == single[k].tobytes(), (tuning, i, k)
        k0, k1 = unit_kinds(saved, 0, ct, tile_w)[0], unit_kinds(saved, 1, ct, tile_w)[0]
        assert k0 and k1 and set(k1) == {"open"} and set(k0) == ({"closed"} if fwd_exit == 1 else {"open"}), (tuning, k0, k1)
        r32, g32, r64, g64 = D._reference("dead", W, H, tile_w, 0.05)
        for k in GRADS:
            assert_with_referee(both[k][1], g32[k], g64[k], f"batch image 1 grad_{k}")


@gpu
@pytest.mark.parametrize("tuning", [dict(tile_w=32, seg_len=64, fwd_exit=1), dict(tile_w=16, seg_len=128, fwd_variant=1, fwd_exit=1)],
                         ids=["tw32-seg64", "tw16-seg128-v1"])
def test_capacity_overflow_under_the_guard_fills(tuning):
    """every list empty: no unit reads a fill, with the zero rows on and off"""
    import test_workspace_capacity as C
    import workspace_guard as WG
    Dn = C._oracle_duplicates("aniso", tuning["tile_w"])
    inp = C._inputs()
    for extra in (dict(bwd_zero=1), dict(bwd_zero=-1)):
        call = C._Call(inp, workspace=Dn // 4, tuning=dict(tuning, **extra))
        runs = WG.run_patterns(call, inp, C._mods())
        assert int(call.layout.dup_capacity) == Dn // 4
        for name, out in runs.items():
            assert int(out["st_counters"][1]) == 1 and int(out["st_list_len"].abs().sum()) == 0, name
            for k in ("image", "depth"):
                assert bool((out[k].view(torch.int32) == C.QNAN).all()), (name, k)
            for k in [g for g in out if g.startswith("grad_")]:
                assert not bool(out[k].view(torch.int32).any()), (name, k)


# ---- CPU half: the dead walk's fold over all-zero sums, in numpy float32 ----
def fold_signs(v, Y0, tile_w):
    """Row floats {mx, my, ca, cbc, cd, op} of a zero unit's entry with centre row v on the tile at Y0, as the dead walk forms them:
    per lane the sums behind the passes are +0 (fma(+-0, finite, +0) = +0); 32 x 16 tiles fold the two sub-tile rows, 16 x 16 tiles
    store the sums.  The wave's total of 64 lanes is -0 exactly when every lane's value is."""
    z = f32(0.0)
    if tile_w == 16:
        return np.zeros(6, f32)
    lanes = []
    with np.errstate(all="ignore"):
        for ly in range(8):
            dya = f32(f32(Y0 + ly) - f32(v))
            dyb = f32(dya + f32(8.0))
            mA0 = mA1 = mB0 = mB1 = mC0 = mC1 = z
            t0, t1 = f32(dya * mA0), f32(dyb * mA1)
            p0, pb = f32(t0 * dya), f32(mB0 * dya)
            v_my = f32(f32(mA1 * dyb) + t0)      # fma of exact zeros: the sum of two signed zeros
            v_cd = f32(f32(t1 * dyb) + p0)
            v_cbc = f32(f32(mB1 * dyb) + pb)
            lanes.append([f32(mB0 + mB1), v_my, f32(mC0 + mC1), v_cbc, v_cd, f32(mA0 + mA1)])
    lanes = np.asarray(lanes, f32)
    tot = lanes[0].copy()
    for row in lanes[1:]:
        tot = (tot + row).astype(f32)  # (-0) + (-0) = -0, anything else +0: the order of the adds does not matter
    return tot


def rule_signs(v, Y0, tile_w):
    """the rule composite_bwd_zero_rows applies"""
    out = np.zeros(6, f32)
    if tile_w == 32 and f32(f32(f32(Y0 + 7) - f32(v)) + f32(8.0)) < 0:
        out[1] = out[3] = f32(-0.0)
    return out


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("tile_w", TILE_WS)
def test_cpu_sign_rule_is_the_fold(tile_w, frame):
    """over every record of `rows` and `special` and every tile row, the rule gives the fold's bits; the scene holds both signs on
    32 x 16 tiles, and the three entries at the boundary fall as v > Y0 + 15 says"""
    from oracle import fgs_oracle as orc
    W, H = frame
    signs = set()
    for name in ("rows", "special"):
        arrs = _scene(name, W, H, tile_w)[0]
        v = orc.project(arrs[0], arrs[1], arrs[2], _ocam(W, H))["mean2d"][:, 1].astype(f32)
        for Y0 in range(0, H, 16):
            for j in range(len(v)):
                a, b = fold_signs(v[j], Y0, tile_w), rule_signs(v[j], Y0, tile_w)
                assert a.tobytes() == b.tobytes(), (name, j, float(v[j]), Y0)
                if name == "rows" and Y0 == 0 and j >= 64:
                    signs.add(bool(np.signbit(a[1])))
        if name == "rows":
            for key, want in (("below", True), ("above", False), ("on", False), ("under", False), ("over", True)):
                for j in ROW_AT[key]:
                    assert bool(np.signbit(rule_signs(v[j], 0, 32)[1])) == want, (key, j, float(v[j]))
            assert v[ROW_AT["on"][0]] == f32(15.0) and v[ROW_AT["over"][0]] == np.nextafter(f32(15.0), f32(np.inf))
            assert v[ROW_AT["under"][0]] == np.nextafter(f32(15.0), f32(-np.inf))
    assert signs == ({True, False} if tile_w == 32 else {False})


def test_cpu_all_plus_zero_is_told_apart():
    """a model that writes +0.0f everywhere differs from the fold on 32 x 16 tiles in the rows scene (the entries below the tile),
    and nowhere on 16 x 16 tiles"""
    from oracle import fgs_oracle as orc
    for W, H in FRAMES:
        for tile_w in TILE_WS:
            arrs = _scene("rows", W, H, tile_w)[0]
            v = orc.project(arrs[0], arrs[1], arrs[2], _ocam(W, H))["mean2d"][:, 1].astype(f32)
            wrong = [j for j in sum(ROW_AT.values(), ()) if fold_signs(v[j], 0, tile_w).tobytes() != np.zeros(6, f32).tobytes()]
            assert (sorted(wrong) == sorted(ROW_AT["below"] + ROW_AT["over"])) if tile_w == 32 else not wrong, (W, H, tile_w, wrong)


def test_cpu_switch_is_a_flag_of_fwd_variant():
    from fresnel_amd import _binding as B
    d = B.make_dims(2, 100, 64, 32, tuning=dict(bwd_zero=-1, fwd_variant=2, fwd_exit=1))
    assert d.fwd_variant == 2 | B.FWD_EXIT_ON | B.BWD_ZERO_OFF
    assert B.make_dims(2, 100, 64, 32).fwd_variant == 0
    on, off = B.make_dims(2, 100, 64, 32, tuning=dict(tile_w=32)), B.make_dims(2, 100, 64, 32, tuning=dict(tile_w=32, bwd_zero=-1))
    assert B.workspace_bytes(on) == B.workspace_bytes(off)  # the switch changes no layout
    La, Lb = B.saved_layout(on), B.saved_layout(off)
    assert (La.total_bytes, La.unit_order, La.fwd_close) == (Lb.total_bytes, Lb.unit_order, Lb.fwd_close)
    assert B.make_dims(2, 100, 64, 32, tuning=dict(bwd_zero=1)).fwd_variant == B.BWD_ZERO_ON
    for bad in (dict(bwd_zero=2), dict(bwd_zero=-2), dict(bwd_zero=-1, fwd_variant=-2), dict(bwd_zero=1, fwd_variant=-1)):
        with pytest.raises(B.FgsError):
            B.make_dims(2, 100, 64, 32, tuning=bad)
    for bad in (0x1000, B.BWD_ZERO_ON | B.BWD_ZERO_OFF):  # an unknown flag bit; both flags at once
        with pytest.raises(B.FgsError):
            B.workspace_bytes(B.make_dims(2, 100, 64, 32, tuning=dict(fwd_variant=bad)))
    import re, os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fgs.h")).read()
    assert int(re.search(r"#define FGS_BWD_ZERO_OFF (0x[0-9a-fA-F]+)", text).group(1), 16) == B.BWD_ZERO_OFF
    assert int(re.search(r"#define FGS_BWD_ZERO_ON (0x[0-9a-fA-F]+)", text).group(1), 16) == B.BWD_ZERO_ON
