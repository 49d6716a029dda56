"""One verdict per closed tile in the blend backward (k_bwd_tail_verdict, k_composite_bwd and k_row_sum; tuning key bwd_tail = the
FGS_BWD_TAIL_ON / _OFF flag of FgsDims.fwd_variant).  The path exists where the exiting forward, the zero rows, the direct binning and
the backward's unit table do, so every call here forces fwd_exit = 1 and bwd_zero = 1.

A TAIL unit lies behind the closing slot of EVERY 16 x 16 half of its tile (saved.fwd_close).  All tail units of a tile restart from
the same slots and reach the same zero-unit verdict, so one wave per tile forms it once and leaves in zero_from[tile] (a section of
the backward's scratch) the DEPTH RANK of the tile's first tail entry -- or 0xFFFFFFFF: no tail, or the verdict is no.  A tail unit of
a tile with a rank returns without writing its rows, and k_row_sum adds row k of a Gaussian of rank r only if r < zero_from[tile of
row k].  The rows left out were +-0 and the sums never hold -0, so every output is the same BITS as with the path off.  What can go
wrong: (1) a verdict that says zero where S is not (lost gradients), (2) the row -> tile mapping or the rank comparison off by one
(a live row dropped, or a row read that nobody wrote: the poison runs), (3) per-image ranks mixed with flat indices, (4) a table word
left unwritten.

Scenes (geometry of tests/test_blend_bwd_dead_units.py, D, and tests/test_blend_bwd_zero_units.py, Z: a whole-frame saturating group of
24 entries in front of a crowd of 190 small Gaussians in ONE tile, list position = index there; every half of the crowded tile closes
at list position 64, the other tiles' lists end inside their first segment):
  big         `dead` with the crowded tile's entries 63, 64, 127, 128 -- the first tail entry and the one in front of it at either
              segment length -- and 100 made LARGE: their rectangles cover the open neighbour tiles too, where they gather non-zero
              gradients, so of one Gaussian's rows some are skipped and some read; one Gaussian moved off the frame (no tiles).
  seam@127    one half of the 32 x 16 crowded tile closes, the other later or never (fwd_variant 4): no tail while a half is open.
  cut@100     the crowded tile's list cut to 100 entries: a tail of 36 entries with segments of 64, a closing in the LAST segment
              (no tail) with segments of 128.
  len@L       last tail units of 1, 63, 64 and 65 entries.
  edge        the crowd in the frame's last tile, partly out of frame on 40 x 24.
  nan / inf   a NaN / Inf upstream gradient on a closed pixel: the verdict is no, rows are written, compared as bits.
  twin        opacity 0.05: nothing closes, every word is 0xFFFFFFFF.
  batch       two images whose crowded tile has different thresholds; overflow: every list empty.
For every scene: the seven outputs bitwise equal to the bwd_tail = -1 call, the bwd_zero = -1 call, a second run, and two runs whose
whole scratch buffer -- gradient rows and zero_from included -- was filled with NaN bits / with zeros before the backward; the referee
against the C oracle; zero_from read back equals what saved.fwd_close, seg_off, ranges, order and dup_ids of the very call predict.

CPU half: k_row_sum's sum order in numpy (four lanes, float64 moments, float32 colour sums) with the rows of rank >= threshold left
out equals the full sum bit for bit, -0 rows included; the row -> tile mapping is the inverse of fgs_emission_slot's formula."""
import functools

import numpy as np
import pytest
import torch

import test_blend_bwd_dead_units as D
import test_blend_bwd_zero_units as Z
from helpers import assert_with_referee

GRADS, OUTS = Z.GRADS, Z.OUTS
FRAMES = [(64, 32), (40, 24)]
TILE_WS = [16, 32]
SEGS = {"s64": dict(seg_len=64), "s128": dict(seg_len=128)}
BIG_AT = (63, 64, 127, 128)
HUGE_AT = 100
CASES = ["big", "seam@127", "cut@100", "len@1", "len@63", "len@64", "len@65", "edge", "nan", "inf", "twin"]
NONE = -1  # 0xFFFFFFFF as int32
gpu = pytest.mark.gpu
f32 = np.float32


def _cut(arrs, n):
    """the crowded tile's list cut to its first n entries (the anchors, in no list of that tile, stay)"""
    N = len(arrs[4])
    keep = np.r_[0:n, N - D.N_ANCHOR:N]
    return [a[keep] for a in arrs]


@functools.lru_cache(maxsize=None)
def _scene(name, W, H, tile_w):
    """-> (the five arrays, gI, gD, crowded tile)"""
    if name in ("seam@127", "nan", "inf") or name.startswith("len@"):
        arrs, gI, gD, _ = Z._scene(name, W, H, tile_w)
        return arrs, gI, gD, D._crowded_tile("dead", W, H, tile_w)
    if name == "edge":
        arrs, gI, gD = D._scene("edge", W, H, tile_w)[:3]
        return [a.copy() for a in arrs], gI, gD, D._crowded_tile("edge", W, H, tile_w)
    arrs, gI, gD = D._scene("dead", W, H, tile_w, 0.05 if name == "twin" else None)[:3]
    arrs = [a.copy() for a in arrs]
    if name in ("big", "moved"):
        for j in BIG_AT:
            Z._place(arrs, j, 9.0 + 0.31 * (j % 4), 8.0 + 0.27 * (j % 3), 20.0, W, H)
        Z._place(arrs, HUGE_AT, 10.0, 9.0, 40.0, W, H)
        rest0 = D.N_FRONT + D.N_CROWD
        Z._place(arrs, rest0, -900.0, 7.0, 3.0, W, H)  # off the frame: no tiles, no rows
    if name == "moved":  # an entry in FRONT of the closing leaves the crowded tile: every later list position shifts by one
        Z._place(arrs, 30, W - 4.0, H - 4.0, 1.5, W, H)
    if name == "cut@100":
        arrs = _cut(arrs, 100)
    return arrs, gI, gD, D._crowded_tile("dead", W, H, tile_w)


@functools.lru_cache(maxsize=None)
def _reference(name, W, H, tile_w):
    from oracle import fgs_oracle as orc
    arrs, gI, gD, _ = _scene(name, W, H, tile_w)
    ocam = Z._ocam(W, H)
    r32 = orc.render(*arrs, ocam, bg=D.BG)
    g32 = orc.render_backward(r32, gI, gD)
    with orc.fp64():
        r64 = orc.render(*arrs, ocam, bg=D.BG)
        g64 = orc.render_backward(r64, gI, gD)
    return r32, g32, r64, g64


def _run(arrs, W, H, gI, gD, tuning, batch=False, poison=None):
    """one forward + backward; -> (the seven outputs, what the call's saved state says, zero_from as the backward left it or None).
    `poison`: the 32-bit word the WHOLE scratch buffer the backward will use is filled with in front of it."""
    from fresnel_amd import _binding as B
    from fresnel_amd import renderer as R
    dev = D._cuda()
    if not batch:
        arrs, gI, gD = [a[None] for a in arrs], gI[None], gD[None]
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True) for a in arrs]
    ren = R.TileBasedRenderer(W, H, background=D.BG)
    ren.tuning = dict(tuning)
    img, dep = ren(*ts, R.Camera(D.FOCAL, D.FOCAL, W / 2, H / 2, W, H), return_depth=True)
    dims = img.grad_fn.dims
    st = R.inspect_saved(img.grad_fn.saved_tensors[-1], dims)
    L = st["layout"]
    num = lambda t: t.cpu().numpy().astype(np.int64)  # noqa: E731
    saved = dict(ranges=num(st["ranges"]), seg_off=num(st["seg_off"]), seg_len=int(L.seg_len), order=num(st["order"]),
                 dup_ids=num(st["dup_ids"]), counters=num(st["counters"]), tile_w=int(L.tile_w), tiles_x=int(L.tiles_x),
                 fwd_close=num(st["fwd_close"]) if "fwd_close" in st else None,
                 rank_of=num(st["rank_of"]) if "rank_of" in st else None)
    scratch_bytes = B.workspace_bytes(dims)[1]
    buf = R._scratch_for(dev, scratch_bytes)  # the cached buffer the backward takes
    if poison is not None:
        buf[:scratch_bytes].view(torch.int32).fill_(poison)
    ((img * torch.from_numpy(gI).to(dev)).sum() + (dep * torch.from_numpy(gD).to(dev)).sum()).backward()
    out = {k: t.grad.detach().cpu().numpy() for k, t in zip(GRADS, ts)}
    out["image"], out["depth"] = img.detach().cpu().numpy(), dep.detach().cpu().numpy()
    zero_from = None
    if saved["rank_of"] is not None:  # the scratch layout's last section, 256-byte aligned: [B * tiles] words, then each image's smallest
        Bn, T = saved["ranges"].shape[:2]
        nb = ((Bn * T + Bn) * 4 + 255) // 256 * 256
        words = buf[scratch_bytes - nb:scratch_bytes - nb + (Bn * T + Bn) * 4].view(torch.int32).cpu().numpy().astype(np.int64)
        zero_from = words[:Bn * T].reshape(Bn, T)
        smallest = (zero_from & 0xFFFFFFFF).min(axis=1)  # as unsigned words: 0xFFFFFFFF where no tile has a rank
        assert np.array_equal(words[Bn * T:] & 0xFFFFFFFF, smallest), (words[Bn * T:].tolist(), smallest.tolist())
    if not batch:
        out = {k: v[0] for k, v in out.items()}
    return out, saved, zero_from


def predicted_zero_from(saved, gI, gD, W, H):
    """zero_from from the call's own saved state: per tile the rank of the list entry at position (largest closing slot) x seg_len
    when every half has a closing slot and every upstream gradient on the tile's in-frame pixels is finite (behind its closing a
    pixel restarts from its final state: T = +0 and S = X - X = +0 whatever the finite gradient is; a NaN or Inf makes S NaN)"""
    rg, fc, seg_len, tile_w = saved["ranges"], saved["fwd_close"], saved["seg_len"], saved["tile_w"]
    Bn, T = rg.shape[:2]
    N = saved["order"].shape[1]
    rank = np.empty_like(saved["order"])
    for b in range(Bn):
        rank[b, saved["order"][b]] = np.arange(N)
    assert np.array_equal(saved["rank_of"], rank), "saved.rank_of is not the inverse of saved.order"
    want = np.full((Bn, T), NONE, np.int64)
    kinds = set()
    for b in range(Bn):
        for t in range(T):
            lo, hi = rg[b, t]
            kc = fc[b, t, :tile_w // 16]
            if hi <= lo:
                kinds.add("empty")
                continue
            if (kc < 0).any():
                kinds.add("open" if (kc < 0).all() else "half")
                continue
            first = int(kc.max())
            assert 1 <= first and lo + first * seg_len < hi, "a closing slot is a slot of the tile"
            ty, tx = divmod(t, saved["tiles_x"])
            px = (slice(None), slice(16 * ty, min(16 * ty + 16, H)), slice(tile_w * tx, min(tile_w * tx + tile_w, W)))
            if not (np.isfinite(gI[b][px]).all() and np.isfinite(gD[b][px[1:]]).all()):
                kinds.add("no")
                continue
            g = saved["dup_ids"][lo + first * seg_len]
            assert g // N == b
            want[b, t] = rank[b, g - b * N]
            kinds.add("yes")
    return want, kinds


def _check(name, arrs, gI, gD, W, H, tuning, what, batch=False):
    got, saved, zf = _run(arrs, W, H, gI, gD, tuning, batch)
    assert zf is not None, f"{what}: the plan has no tail verdict"
    for off in (dict(bwd_tail=-1), dict(bwd_zero=-1)):
        ref, saved_off, zf_off = _run(arrs, W, H, gI, gD, dict(tuning, **off), batch)
        assert zf_off is None and saved_off["rank_of"] is None, (what, off)
        Z._same_bits(got, ref, f"{what} against {off}:")
    Z._same_bits(got, _run(arrs, W, H, gI, gD, tuning, batch)[0], what + " second run:")
    for word in (0x7FC00000, 0):
        again, _, zf2 = _run(arrs, W, H, gI, gD, tuning, batch, poison=word)
        Z._same_bits(got, again, f"{what} scratch filled with {word:#x}:")
        assert np.array_equal(zf, zf2), (what, word)
    gIb, gDb = (gI, gD) if batch else (gI[None], gD[None])
    want, kinds = predicted_zero_from(saved, gIb, gDb, W, H)
    assert np.array_equal(zf, want), (what, zf.tolist(), want.tolist())
    return got, saved, zf, kinds


@gpu
@pytest.mark.parametrize("seg", sorted(SEGS))
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("tile_w", TILE_WS)
@pytest.mark.parametrize("name", CASES)
def test_scene_bitwise_referee_and_table(name, tile_w, frame, seg):
    W, H = frame
    arrs, gI, gD, ct = _scene(name, W, H, tile_w)
    r32, g32, r64, g64 = _reference(name, W, H, tile_w)
    splits = [dict()] + ([dict(fwd_variant=4), dict(fwd_variant=1)] if name == "seam@127" and seg == "s64" else [])
    seen = set()
    for split in splits:
        tuning = dict(tile_w=tile_w, fwd_exit=1, bwd_zero=1, **SEGS[seg], **split)
        what = f"{name} {W}x{H} tile_w={tile_w} {seg} {split}"
        got, saved, zf, kinds = _check(name, arrs, gI, gD, W, H, tuning, what)
        seen |= kinds
        assert_with_referee(got["image"], r32.image, r64.image, f"{what} image")
        assert_with_referee(got["depth"], r32.depth, r64.depth, f"{what} depth")
        if name in ("nan", "inf"):
            assert not np.isfinite(got["colors"]).all() or not np.isfinite(got["positions"]).all(), what
            assert zf[0, ct] == NONE and "no" in kinds, (what, zf.tolist())
        else:
            for k in GRADS:
                assert_with_referee(got[k], g32[k], g64[k], f"{what} grad_{k}")
        lo, hi = saved["ranges"][0, ct]
        n, seg_len = int(hi - lo), saved["seg_len"]
        if name == "twin":
            assert (zf == NONE).all() and (saved["fwd_close"] == NONE).all(), what
        if name == "big":
            # the crowded tile's threshold is the rank of list position seg_len (every half closes at 64: slot 1); the entry in
            # front of it and the large one behind it have rows in other tiles, which have no tail: read there, skipped here
            assert zf[0, ct] >= 0 and (np.delete(zf[0], ct) == NONE).all(), (what, zf.tolist())
            N = saved["order"].shape[1]
            ids = saved["dup_ids"]
            first, before = int(ids[lo + seg_len]), int(ids[lo + seg_len - 1])
            assert saved["rank_of"][0, first] == zf[0, ct] and saved["rank_of"][0, before] == zf[0, ct] - 1, what
            for j in (first, before, HUGE_AT):
                tiles_of_j = [t for t in range(zf.shape[1]) if j in ids[saved["ranges"][0, t, 0]:saved["ranges"][0, t, 1]]]
                assert ct in tiles_of_j and len(tiles_of_j) > 1, (what, j, tiles_of_j)
            for j in BIG_AT + (HUGE_AT,):
                assert np.abs(got["colors"][j]).max() > 0 and np.abs(got["positions"][j]).max() > 0, (what, j)
            rest0 = D.N_FRONT + D.N_CROWD
            assert not got["colors"][rest0].any() and not any((ids[:int(saved["counters"][0])] % N == rest0).tolist()), what
        if name == "cut@100":
            assert n == 100
            assert (zf[0, ct] >= 0) == (seg_len == 64), (what, zf.tolist())  # segments of 128: the closing fell into the last segment
        if name.startswith("len@"):
            L = int(name[4:])
            assert n == 128 + L and zf[0, ct] >= 0 and n % seg_len == L % seg_len, (what, n)  # the last tail unit's length
        if name == "edge":
            assert zf[0, ct] >= 0 and (W % tile_w != 0 or H % 16 != 0) == ((W, H) == (40, 24)), what
    if name == "seam@127" and tile_w == 32 and seg == "s64":
        assert "half" in seen and "yes" in seen, seen  # one half open: no tail; both closed (one part): a tail


@gpu
@pytest.mark.parametrize("seg", sorted(SEGS))
@pytest.mark.parametrize("tile_w", TILE_WS)
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_two_images_with_different_thresholds(frame, tile_w, seg):
    """image 1's crowded tile lost an entry in front of the closing, so the same tile index has another first tail entry: its rank
    is the image's own, not a flat index, and each image is bit-equal to its single call"""
    W, H = frame
    a, gI, gD, ct = _scene("big", W, H, tile_w)
    b = _scene("moved", W, H, tile_w)[0]
    tuning = dict(tile_w=tile_w, fwd_exit=1, bwd_zero=1, **SEGS[seg])
    stack = [np.stack([x, y]) for x, y in zip(a, b)]
    both, saved, zf, kinds = _check("batch", stack, np.stack([gI, gI]), np.stack([gD, gD]), W, H, tuning, f"batch {tuning}", batch=True)
    assert zf[0, ct] >= 0 and zf[1, ct] >= 0 and zf[0, ct] != zf[1, ct], zf.tolist()
    for i, arrs in enumerate((a, b)):
        single, _, zf1 = _run(arrs, W, H, gI, gD, tuning)
        assert np.array_equal(zf1[0], zf[i]), (i, zf1.tolist(), zf.tolist())
        for k in OUTS:
            assert both[k][i].tobytes() == single[k].tobytes(), (tuning, i, k)


@gpu
@pytest.mark.parametrize("tuning", [dict(tile_w=32, seg_len=64), dict(tile_w=16, seg_len=128, fwd_variant=1)], ids=["tw32-seg64", "tw16-seg128-v1"])
def test_capacity_overflow_under_the_guard_fills(tuning):
    """every list empty: no verdict reads a fill, no unit exists, every gradient is the contract's zero -- path on and off"""
    import test_workspace_capacity as C
    import workspace_guard as WG
    Dn = C._oracle_duplicates("aniso", tuning["tile_w"])
    inp = C._inputs()
    for extra in (dict(), dict(bwd_tail=-1)):
        call = C._Call(inp, workspace=Dn // 4, tuning=dict(tuning, fwd_exit=1, bwd_zero=1, **extra))
        runs = WG.run_patterns(call, inp, C._mods())
        assert (call.layout.rank_of < call.layout.total_bytes) == (not extra)  # (the call records its layout when it runs)
        assert int(call.layout.dup_capacity) == Dn // 4
        for name, out in runs.items():
            assert int(out["st_counters"][1]) == 1 and int(out["st_list_len"].abs().sum()) == 0, name
            for k in ("image", "depth"):
                assert bool((out[k].view(torch.int32) == C.QNAN).all()), (name, k)
            for k in [g for g in out if g.startswith("grad_")]:
                assert not bool(out[k].view(torch.int32).any()), (name, k)


# ---- CPU half ----
def row_sum(rows, keep):
    """k_row_sum's arithmetic for one Gaussian: lane `sub` of four adds rows sub, sub + 4, ... in that order (moments in float64,
    colour / depth sums in float32, all from +0), then the totals of lanes (0, 1) and (2, 3) are added pairwise and those two.
    (The factors the kernel applies between the lane sums and the shuffles act on the lane totals and are left out.)"""
    lanes64 = np.zeros((4, 6), np.float64)
    lanes32 = np.zeros((4, 4), f32)
    for k in range(len(rows)):
        if keep[k]:
            lanes64[k % 4] += rows[k, :6].astype(np.float64)
            lanes32[k % 4] = (lanes32[k % 4] + rows[k, 6:]).astype(f32)
    tot = np.concatenate([lanes64.astype(f32), lanes32], 1)
    pair = np.stack([(tot[0] + tot[1]).astype(f32), (tot[2] + tot[3]).astype(f32)])
    return (pair[0] + pair[1]).astype(f32)


@pytest.mark.parametrize("cnt", [1, 3, 4, 5, 9, 15, 40])
def test_cpu_row_sum_without_the_zero_rows_is_the_full_sum(cnt):
    """rows of rank >= the threshold are +-0 rows (floats 1 and 3 -0 for some): leaving them out changes no bit of any total --
    also when EVERY row of a lane, or of the Gaussian, is left out (the total is +0, never -0)"""
    rs = np.random.RandomState(1700 + cnt)
    for trial in range(40):
        rows = (rs.standard_normal((cnt, 10)) * 10.0 ** rs.randint(-20, 6, (cnt, 1))).astype(f32)
        zero = rs.random_sample(cnt) < (0.0, 0.4, 0.8, 1.0)[trial % 4]
        rows[zero] = 0.0
        neg = zero & (rs.random_sample(cnt) < 0.5)
        rows[neg, 1] = rows[neg, 3] = f32(-0.0)
        full, part = row_sum(rows, np.ones(cnt, bool)), row_sum(rows, ~zero)
        assert full.tobytes() == part.tobytes(), (cnt, trial)
        if zero.all():
            assert part.tobytes() == np.zeros(10, f32).tobytes(), (cnt, trial)
    # what the statement rests on: a sum that starts at +0 is never -0, and +-0 added to it changes nothing
    assert f32(0.0) + f32(-0.0) == 0 and not np.signbit(f32(0.0) + f32(-0.0)) and not np.signbit(np.float64(0.0) + np.float64(f32(-0.0)))
    x = f32(1.5e-40)
    assert (x + f32(-0.0)).tobytes() == x.tobytes() and (f32(-x) + f32(0.0)).tobytes() == f32(-x).tobytes()


def emission_slot(tx, ty, bbx, bby, tile_w):
    """fgs_emission_slot (fgs_internal.h) without dup_off"""
    tx0, tx1, ty0 = (bbx & 0xFFFF) // tile_w, ((bbx >> 16) - 1) // tile_w, (bby & 0xFFFF) // 16
    return (ty - ty0) * (tx1 - tx0 + 1) + (tx - tx0)


def row_tile(k, bbx, bby, tile_w, tiles_x):
    """k_row_sum's tile of row k (fgs_project.hip)"""
    tx0 = (bbx & 0xFFFF) // tile_w
    t0 = (bby & 0xFFFF) // 16 * tiles_x + tx0
    rw = max(((bbx >> 16) - 1) // tile_w - tx0 + 1, 1)
    ky = int(f32(f32(f32(k) + f32(0.5)) * f32(f32(1.0) / f32(rw))))  # the kernel's quotient: no integer division
    return t0 + ky * tiles_x + (k - ky * rw)


def test_cpu_row_quotient_in_fp32_is_the_integer_quotient():
    """(row + 0.5) * (1 / rw) in float32, truncated, is row // rw for every row a Gaussian can have and every rectangle width"""
    rows = np.arange(0, 1 << 16, dtype=np.int64)
    for rw in list(range(1, 130)) + [255, 256, 257, 1000, 2048]:
        q = ((rows.astype(f32) + f32(0.5)) * (f32(1.0) / f32(rw))).astype(f32).astype(np.int64)
        assert np.array_equal(q, rows // rw), rw


@pytest.mark.parametrize("tile_w", TILE_WS)
@pytest.mark.parametrize("rect", [(1, 1), (1, 4), (4, 1), (3, 5)], ids=lambda r: f"{r[0]}x{r[1]}")
def test_cpu_row_index_to_tile_is_the_inverse_of_the_emission_slot(rect, tile_w):
    w, h = rect
    tiles_x = 9
    for tx0, ty0 in ((0, 0), (2, 3), (9 - w, 1)):
        for x0 in (tx0 * tile_w, tx0 * tile_w + tile_w - 1):          # bbox [x0, x1) x [y0, y1): first pixel anywhere in its tile,
            for x1 in ((tx0 + w - 1) * tile_w + 1, (tx0 + w) * tile_w):  # one past the last pixel anywhere in the last tile
                if x1 <= x0:
                    continue
                for y0, y1 in ((ty0 * 16 + 15, (ty0 + h - 1) * 16 + 16), (ty0 * 16, (ty0 + h - 1) * 16 + 1)):
                    if y1 <= y0:
                        continue
                    bbx, bby = x0 | (x1 << 16), y0 | (y1 << 16)
                    seen = []
                    for ty in range(ty0, ty0 + h):
                        for tx in range(tx0, tx0 + w):
                            k = emission_slot(tx, ty, bbx, bby, tile_w)
                            assert row_tile(k, bbx, bby, tile_w, tiles_x) == ty * tiles_x + tx, (rect, tile_w, tx, ty, k)
                            seen.append(k)
                    assert seen == list(range(w * h))  # emission order: tile row, then tile column


def test_cpu_switch_and_layout():
    import os
    import re
    from fresnel_amd import _binding as B
    kw = dict(batch=2, num_gaussians=100, width=64, height=32)
    on = B.make_dims(**kw, tuning=dict(tile_w=32, fwd_exit=1, bwd_zero=1))
    assert B.make_dims(**kw, tuning=dict(bwd_tail=1)).fwd_variant == B.BWD_TAIL_ON
    assert B.make_dims(**kw, tuning=dict(bwd_tail=-1, fwd_variant=2)).fwd_variant == 2 | B.BWD_TAIL_OFF
    Lon, (sv_on, sc_on) = B.saved_layout(on), B.workspace_bytes(on)
    tiles = Lon.tiles_x * Lon.tiles_y
    assert Lon.fwd_close < Lon.rank_of < Lon.total_bytes and Lon.rank_of % 256 == 0 and Lon.total_bytes - Lon.rank_of >= 4 * 2 * 100
    # where one of the four is missing -- and with the switch off -- nothing changes and no table exists; forcing it on adds nothing
    for miss in (dict(bwd_tail=-1), dict(bwd_zero=-1), dict(fwd_exit=-1), dict(bin_mode=2), dict(bwd_zero=-1, bwd_tail=1)):
        d = B.make_dims(**kw, tuning=dict(dict(tile_w=32, fwd_exit=1, bwd_zero=1), **miss))
        L, (sv, sc) = B.saved_layout(d), B.workspace_bytes(d)
        assert L.rank_of == L.total_bytes, miss
        if "bin_mode" in miss:  # (the radix binning has sort buffers of its own size)
            continue
        assert sc_on - sc == ((tiles * 2 + 2) * 4 + 255) // 256 * 256, miss  # a word per tile and one per image
        if "fwd_exit" not in miss:
            assert sv_on - sv == (2 * 100 * 4 + 255) // 256 * 256 and (L.unit_order, L.fwd_close) == (Lon.unit_order, Lon.fwd_close), miss
    same = B.make_dims(**kw, tuning=dict(tile_w=32, fwd_exit=1, bwd_zero=1, bwd_tail=1))
    assert B.workspace_bytes(same) == (sv_on, sc_on)
    auto_small = B.make_dims(**kw, tuning=dict(tile_w=32))  # below 8192 tile halves neither the exit nor the zero rows are on
    assert B.saved_layout(auto_small).rank_of == B.saved_layout(auto_small).total_bytes
    flagship = B.make_dims(batch=8, num_gaussians=32768, width=512, height=512)
    Lf = B.saved_layout(flagship)
    assert Lf.rank_of < Lf.total_bytes
    for bad in (dict(bwd_tail=2), dict(bwd_tail=-2), dict(bwd_tail=1, fwd_variant=-1)):
        with pytest.raises(B.FgsError):
            B.make_dims(**kw, tuning=bad)
    with pytest.raises(B.FgsError):  # both flags at once
        B.workspace_bytes(B.make_dims(**kw, tuning=dict(fwd_variant=B.BWD_TAIL_ON | B.BWD_TAIL_OFF)))
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fgs.h")).read()
    assert int(re.search(r"#define FGS_BWD_TAIL_OFF (0x[0-9a-fA-F]+)", text).group(1), 16) == B.BWD_TAIL_OFF
    assert int(re.search(r"#define FGS_BWD_TAIL_ON (0x[0-9a-fA-F]+)", text).group(1), 16) == B.BWD_TAIL_ON
