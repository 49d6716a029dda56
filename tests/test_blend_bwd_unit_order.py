"""Launch order of the blend backward's work units (saved.unit_order, built by k_unit_order of fgs_bin.hip, read by k_composite_bwd as
unit_order[fgs_xcd_remap(blockIdx.x, U)]).

A work unit is one (tile, depth segment): a list of `len` entries has len // seg_len FULL units and, unless seg_len divides len, one
PARTIAL unit, its last.  The U launch slots are cut into the eight contiguous SLICES that fgs_xcd_remap deals to the XCDs; a slice
keeps the units it holds in unit (= tile) order, and lists its full units first, in increasing index, then its partial units,
longest first by quarter-octave of their entry count (any order inside a quarter-octave).  The table is placement only: every unit
runs the same code on the same inputs, so what can go wrong is the TABLE -- a unit listed twice (another never runs: its gradient
rows keep whatever the buffer held), a slot past U, a slice boundary off by one.

Scenes.  Small flat Gaussians whose bboxes lie inside ONE tile each, so a tile's list length is the number of Gaussians put there:
the lengths are written down per scene in units of the segment length L (`SPECS`), for the first four tiles of the frame; every other
tile stays empty.  The CPU half asserts those lengths on the oracle's tile lists, and states the order in numpy with its invariants.
The saturating scene with dead units behind it is test_blend_bwd_dead_units' `dead`.

Statement for every scene (GPU): the table's invariants on inspect_saved; seg_off / seg_tile tile-ordered as ever; image, depth and
the five gradients pass assert_with_referee against the C oracle (fp32 and fp64 runs); a second run is bitwise equal."""
import functools

import numpy as np
import pytest
import torch

import workspace_guard as WG
from helpers import assert_with_referee
from test_blend_bwd_dead_units import _reference as dead_reference
from test_blend_bwd_dead_units import _scene as dead_scene

gpu = pytest.mark.gpu
GRADS = ["positions", "scales", "rotations", "colors", "opacities"]
BG = (0.05, 0.1, 0.15)
FOCAL = 51.2

# list lengths of the first four tiles as functions of the segment length L
SPECS = {
    "seamsA": lambda L: [L, 2 * L, L + 1, L - 1],          # exactly one / two segments, one entry more, one entry fewer
    "seamsB": lambda L: [1, 0, 2 * L - 1, 3],              # a single entry, an empty tile between occupied ones
    "all_partial": lambda L: [L // 2, 1, L + 3, 5],
    "none_partial": lambda L: [L, 0, 2 * L, L],
    "culled": lambda L: [0, 0, 0, 0],                      # U = 0 (the scene's Gaussians stand behind the camera)
    "u1": lambda L: [0, 0, 7, 0],
    "u7": lambda L: [L + 1, 2 * L + 1, 1, L],              # 2 + 3 + 1 + 1 units: seven slices of one unit, one empty
    "u8": lambda L: [L + 1, 2 * L + 1, 1, 2 * L],          # 2 + 3 + 1 + 2
    "u9": lambda L: [L + 1, 2 * L + 1, L + 5, 2 * L],      # 2 + 3 + 2 + 2: the first slice holds two units
    "many": lambda L: [5 * L + 7, 3 * L, 4 * L + 40, 2 * L + L - 1],  # 6 + 3 + 5 + 3 = 17: slices mix full and partial units of several tiles
}
# (frame, tile_w, seg_len, bin_mode): every pair of (tile shape, segment length), (tile shape, list builder), (frame, tile shape)
CONFIGS = [((64, 32), 16, 64, 1), ((64, 32), 32, 128, 2), ((40, 24), 16, 128, 1), ((40, 24), 32, 64, 2), ((64, 32), 16, 64, 2),
           ((40, 24), 32, 128, 1)]
CASES = [(n, c) for n in SPECS for c in CONFIGS if not (n == "many" and c[2] == 128)]  # (`many` at L = 128 is 2 000 Gaussians)


def _id(c):
    return f"{c[0][0]}x{c[0][1]}-tw{c[1]}-s{c[2]}-bin{c[3]}"


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


# ---- the order, stated in numpy ----
def xcd_remap(bid, n):
    q, r, xcd, i = n >> 3, n & 7, bid & 7, bid >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + i


def slice_bounds(U):
    """nine boundaries of the eight contiguous slot ranges fgs_xcd_remap(., U) deals to the XCDs"""
    q, r = U >> 3, U & 7
    return [g * (q + 1) if g < r else r * (q + 1) + (g - r) * q for g in range(9)]


def quarter_octave(n):
    """quarter-octave of n >= 1 as the kernels count it (length_bucket of fgs_bin.hip): 4 x the exponent + the two bits behind the
    leading one"""
    lg = int(n).bit_length() - 1
    return 4 * lg + (((n >> (lg - 2)) if lg >= 2 else (n << (2 - lg))) & 3)


def unit_lengths(lens, seg_len):
    """entry count of every unit, in unit order (tile by tile)"""
    out = []
    for n in lens:
        out += [seg_len] * (int(n) // seg_len) + ([int(n) % seg_len] if int(n) % seg_len else [])
    return np.asarray(out, np.int64)


def model_order(lens, seg_len):
    """one table that satisfies the statement: inside a slice full units by index, then partial ones by decreasing quarter-octave"""
    ul = unit_lengths(lens, seg_len)
    b = slice_bounds(len(ul))
    order = []
    for g in range(8):
        mine = list(range(b[g], b[g + 1]))
        order += [u for u in mine if ul[u] == seg_len]
        order += sorted((u for u in mine if ul[u] != seg_len), key=lambda u: -quarter_octave(ul[u]))
    return np.asarray(order, np.int64)


def check_order(order, lens, seg_len):
    """the invariants of a table `order` (slot -> unit) for lists of the lengths `lens`"""
    ul = unit_lengths(lens, seg_len)
    U = len(ul)
    order = np.asarray(order, np.int64)
    assert order.shape == (U,)
    assert np.array_equal(np.sort(order), np.arange(U)), "not a permutation of the units"
    b = slice_bounds(U)
    assert b[0] == 0 and b[8] == U
    for g in range(8):
        mine = order[b[g]:b[g + 1]]
        assert np.array_equal(np.sort(mine), np.arange(b[g], b[g + 1])), f"slice {g} does not hold the units the tile order gave it"
        full = ul[mine] == seg_len
        nfull = int(full.sum())
        assert full[:nfull].all(), f"slice {g}: a partial unit in front of a full one"
        assert (np.diff(mine[:nfull]) > 0).all(), f"slice {g}: full units out of index order"
        qo = [quarter_octave(n) for n in ul[mine[nfull:]]]
        assert all(x >= y for x, y in zip(qo, qo[1:])), f"slice {g}: partial units not longest first: {ul[mine[nfull:]]}"


# ---- CPU half ----
@pytest.mark.parametrize("U", [0, 1, 7, 8, 9, 15, 16, 17, 34056, 1000003])
def test_cpu_slices_are_what_the_remap_deals(U):
    b = slice_bounds(U)
    assert b[0] == 0 and b[8] == U and all(0 <= b[g + 1] - b[g] - (U >> 3) <= 1 for g in range(8))
    n = min(U, 4096)  # (every block of a small launch, the first and last blocks of a large one)
    for bid in list(range(n)) + list(range(max(U - n, 0), U)):
        g = bid & 7
        assert b[g] <= xcd_remap(bid, U) < b[g + 1] and xcd_remap(bid, U) == b[g] + (bid >> 3)
    if U <= 4096:
        assert sorted(xcd_remap(bid, U) for bid in range(U)) == list(range(U))


def test_cpu_quarter_octaves():
    assert [quarter_octave(n) for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 63, 64, 127)] == [0, 4, 6, 8, 9, 10, 11, 12, 12, 13, 23, 24, 27]
    assert all(quarter_octave(n) <= 4 * np.log2(n) < quarter_octave(n) + 1.4 for n in range(1, 600))
    assert all(quarter_octave(n + 1) >= quarter_octave(n) for n in range(1, 600))


@pytest.mark.parametrize("seg_len", [64, 128])
def test_cpu_model_order_satisfies_the_statement(seg_len):
    rs = np.random.RandomState(12)
    draws = [SPECS[n](seg_len) for n in SPECS] + [SPECS[n](seg_len) * 8 for n in ("seamsA", "seamsB", "all_partial", "none_partial")]
    draws += [rs.randint(0, 5 * seg_len, size=rs.randint(1, 70)) for _ in range(40)]
    draws += [np.full(50, seg_len), np.full(50, seg_len - 1), np.zeros(9, int), [1] * 9, [seg_len] * 3 + [3] * 30]
    for lens in draws:
        order = model_order(lens, seg_len)
        check_order(order, lens, seg_len)
    # a table that breaks each clause is caught
    lens = SPECS["many"](seg_len)
    good = model_order(lens, seg_len)
    for bad in (np.arange(len(good)), good[::-1], np.r_[good[1:], good[:1]], np.r_[good[:-1], good[:1]]):
        with pytest.raises(AssertionError):
            check_order(bad, lens, seg_len)


# ---- scenes ----
def _tile_grid(W, H, tile_w):
    return -(-W // tile_w), -(-H // 16)


@functools.lru_cache(maxsize=None)
def _scene(name, W, H, tile_w, seg_len, rot=0):
    """five arrays, upstream gradients and the list length of every tile; `rot` rotates the spec over the four tiles (batches)"""
    rs = np.random.RandomState(7700 + W + 13 * rot)
    tx, ty = _tile_grid(W, H, tile_w)
    spec = SPECS[name](seg_len)
    spec = spec[rot % 4:] + spec[:rot % 4]
    lens = np.zeros(tx * ty, np.int64)
    lens[:4] = spec
    u, v = [], []
    for t, n in enumerate(lens):
        X0, Y0 = (t % tx) * tile_w, (t // tx) * 16
        cw, ch = min(tile_w, W - X0), min(16, H - Y0)
        u += list(X0 + rs.uniform(3.5, cw - 3.5, n))
        v += list(Y0 + rs.uniform(3.5, ch - 3.5, n))
    if name == "culled":  # something to cull: on the frame, but behind the camera
        u, v = list(rs.uniform(4, W - 4, 40)), list(rs.uniform(4, H - 4, 40))
    N = len(u)
    perm = rs.permutation(N)  # depth order unrelated to the tile order
    u, v = np.asarray(u)[perm], np.asarray(v)[perm]
    z = (2.0 + 0.002 * np.arange(N)) * (1.0 if name == "culled" else -1.0)
    r = rs.uniform(1.2, 1.5, N)  # 3 sigma in pixels
    s = r / 3.0 * np.abs(z) / FOCAL
    th = rs.uniform(0.0, np.pi, N)
    pos = np.stack([(u - W / 2) * np.abs(z) / FOCAL, -(v - H / 2) * np.abs(z) / FOCAL, z], 1).astype(np.float32)
    scale = np.stack([s, 0.7 * s, 1e-3 * s], 1).astype(np.float32)
    quat = np.stack([np.cos(th / 2), 0 * th, 0 * th, np.sin(th / 2)], 1).astype(np.float32)
    color = (0.2 + 0.7 * rs.random_sample((N, 3))).astype(np.float32)
    opacity = rs.uniform(0.01, 0.05, N).astype(np.float32)
    gI = rs.standard_normal((3, H, W)).astype(np.float32)
    gD = (rs.standard_normal((H, W)) * 0.1).astype(np.float32) + 0.05
    return [pos, scale, quat, color, opacity], gI, gD, lens


@functools.lru_cache(maxsize=None)
def _reference(name, W, H, tile_w, seg_len, rot=0):
    from oracle import fgs_oracle as orc
    arrs, gI, gD = _scene(name, W, H, tile_w, seg_len, rot)[:3]
    ocam = orc.make_camera(np.eye(4, dtype=np.float32), FOCAL, FOCAL, W / 2, H / 2, W, H)
    r32 = orc.render(*arrs, ocam, bg=BG)
    g32 = orc.render_backward(r32, gI, gD)
    with orc.fp64():
        r64 = orc.render(*arrs, ocam, bg=BG)
        g64 = orc.render_backward(r64, gI, gD)
    return r32, g32, r64, g64


def _oracle_lens(arrs, W, H, tile_w):
    from oracle import fgs_oracle as orc
    ocam = orc.make_camera(np.eye(4, dtype=np.float32), FOCAL, FOCAL, W / 2, H / 2, W, H)
    p = orc.project(arrs[0], arrs[1], arrs[2], ocam, 64.0)
    _, vs = orc.depth_order(p["depth"], p["visible"])
    ranges, _ = orc.tile_lists(vs, p["bbox"], W, H, 16, tile_w=tile_w)
    return np.diff(np.asarray(ranges, np.int64))


@pytest.mark.parametrize("name,cfg", CASES, ids=[f"{n}-{_id(c)}" for n, c in CASES])
def test_cpu_scenes_have_the_lists_they_are_named_for(name, cfg):
    (W, H), tile_w, seg_len, _ = cfg
    arrs, _, _, lens = _scene(name, W, H, tile_w, seg_len)
    assert np.array_equal(_oracle_lens(arrs, W, H, tile_w), lens)
    ul = unit_lengths(lens, seg_len)
    want_units = dict(culled=0, u1=1, u7=7, u8=8, u9=9, many=17).get(name)
    assert want_units is None or len(ul) == want_units
    if name == "all_partial":
        assert (lens[:4] % seg_len != 0).all()
    if name == "none_partial":
        assert (lens % seg_len == 0).all() and len(ul) == 4
    if name == "seamsA":
        assert list(lens[:4]) == [seg_len, 2 * seg_len, seg_len + 1, seg_len - 1]
    assert (lens[4:] == 0).all() and len(lens) >= 4


# ---- GPU half ----
def _hip(arrs, W, H, gI, gD, tuning, workspace="worst", guard=None):
    """forward + backward of a batch ([B, N, .] arrays; one camera); outputs, and the integer stages of the forward"""
    from fresnel_amd import renderer as R
    dev = _cuda()
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True) for a in arrs]
    ren = R.TileBasedRenderer(W, H, background=BG, workspace=workspace)
    ren.tuning = dict(tuning)
    img, dep = ren(*ts, R.Camera(FOCAL, FOCAL, W / 2, H / 2, W, H), return_depth=True)
    node = img.grad_fn
    saved, dims = node.saved_tensors[-1], node.dims
    st = R.inspect_saved(saved, dims)
    L = st["layout"]
    assert int(L.seg_len) == tuning["seg_len"] and int(L.tile_w) == tuning["tile_w"]
    assert "unit_order" in st and L.seg_ckpt <= L.unit_order < L.total_bytes and L.unit_order % 256 == 0
    assert L.total_bytes - L.unit_order >= 4 * L.seg_capacity
    cnt = st["counters"].cpu().numpy()
    U = int(cnt[2])
    rg = st["ranges"].cpu().numpy().astype(np.int64)
    stages = dict(U=U, overflow=int(cnt[1]), lens=(rg[..., 1] - rg[..., 0]).reshape(-1), seg_off=st["seg_off"].cpu().numpy(),
                  seg_tile=st["seg_tile"][:U].cpu().numpy(), unit_order=st["unit_order"][:U].cpu().numpy(),
                  table_words=st["unit_order"].clone(), capacity=int(L.seg_capacity))
    before = saved.clone()
    ((img * torch.from_numpy(gI).to(dev)).sum() + (dep * torch.from_numpy(gD).to(dev)).sum()).backward()
    torch.cuda.synchronize()
    if guard is not None:
        guard.check("after the backward")
    assert torch.equal(saved, before), "fgs_backward modified `saved`"
    out = {k: t.grad.detach().cpu().numpy() for k, t in zip(GRADS, ts)}
    out["image"], out["depth"] = img.detach().cpu().numpy(), dep.detach().cpu().numpy()
    return out, stages


def _check_stages(stg, lens, seg_len):
    """seg_off / seg_tile as they have always been (tile-ordered), and the table's invariants"""
    lens = np.asarray(lens, np.int64)
    assert stg["overflow"] == 0 and np.array_equal(stg["lens"], lens)
    nseg = -(-lens // seg_len)
    U = int(nseg.sum())
    assert stg["U"] == U <= stg["capacity"]
    assert np.array_equal(stg["seg_off"], np.concatenate([[0], np.cumsum(nseg)]))
    assert np.array_equal(stg["seg_tile"], np.repeat(np.arange(len(lens)), nseg))
    check_order(stg["unit_order"], lens, seg_len)


def _tuning(tile_w, seg_len, bin_mode):
    return dict(tile_w=tile_w, seg_len=seg_len, bin_mode=bin_mode)


@functools.lru_cache(maxsize=None)
def _hip_single(name, W, H, tile_w, seg_len, bin_mode, rot=0):
    arrs, gI, gD = _scene(name, W, H, tile_w, seg_len, rot)[:3]
    return _hip([a[None] for a in arrs], W, H, gI[None], gD[None], _tuning(tile_w, seg_len, bin_mode))


def _assert_oracle(got, b, ref, what):
    r32, g32, r64, g64 = ref
    assert_with_referee(got["image"][b], r32.image, r64.image, f"{what} image")
    assert_with_referee(got["depth"][b], r32.depth, r64.depth, f"{what} depth")
    for k in GRADS:
        assert_with_referee(got[k][b], g32[k], g64[k], f"{what} grad_{k}")


@gpu
@pytest.mark.parametrize("name,cfg", CASES, ids=[f"{n}-{_id(c)}" for n, c in CASES])
def test_table_and_results(name, cfg):
    (W, H), tile_w, seg_len, bin_mode = cfg
    lens = _scene(name, W, H, tile_w, seg_len)[3]
    got, stg = _hip_single(name, W, H, tile_w, seg_len, bin_mode)
    what = f"{name} {_id(cfg)}"
    _check_stages(stg, lens, seg_len)
    _assert_oracle(got, 0, _reference(name, W, H, tile_w, seg_len), what)
    arrs, gI, gD = _scene(name, W, H, tile_w, seg_len)[:3]
    again, stg2 = _hip([a[None] for a in arrs], W, H, gI[None], gD[None], _tuning(tile_w, seg_len, bin_mode))
    _check_stages(stg2, lens, seg_len)
    for k in GRADS + ["image", "depth"]:
        assert np.array_equal(got[k], again[k]), f"{what} {k}: second run differs"


@gpu
@pytest.mark.parametrize("images", [2, 8])
@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[3]], ids=_id)
@pytest.mark.parametrize("name", ["seamsA", "all_partial"])
def test_batches(name, cfg, images):
    """several images in one call (image b = the scene with its spec rotated by b tiles): the slices cross images; the batch is
    bit-equal to its single calls, and every image passes against the oracle"""
    (W, H), tile_w, seg_len, bin_mode = cfg
    scenes = [_scene(name, W, H, tile_w, seg_len, b % 4) for b in range(images)]
    arrs = [np.stack([s[0][i] for s in scenes]) for i in range(5)]
    got, stg = _hip(arrs, W, H, np.stack([s[1] for s in scenes]), np.stack([s[2] for s in scenes]), _tuning(tile_w, seg_len, bin_mode))
    _check_stages(stg, np.concatenate([s[3] for s in scenes]), seg_len)
    assert stg["U"] >= 8 and stg["U"] % 8 != 0 or images == 8
    for b in range(images):
        single = _hip_single(name, W, H, tile_w, seg_len, bin_mode, b % 4)[0]
        for k in GRADS + ["image", "depth"]:
            assert np.array_equal(got[k][b], single[k][0]), (b, k)
        _assert_oracle(got, b, _reference(name, W, H, tile_w, seg_len, b % 4), f"{name} {_id(cfg)} image {b} of {images}")


@gpu
@pytest.mark.parametrize("frame,tile_w,seg_len,bin_mode", [((64, 32), 32, 64, 1), ((40, 24), 16, 64, 2), ((64, 32), 16, 128, 1)],
                         ids=["64x32-tw32-s64-bin1", "40x24-tw16-s64-bin2", "64x32-tw16-s128-bin1"])
def test_saturating_scene_with_dead_units(frame, tile_w, seg_len, bin_mode):
    """test_blend_bwd_dead_units' `dead`: a whole-frame saturating group in front, every later unit of every tile restarts dead --
    dead and general units, full and partial, in one table; and as a two-image batch with its never-saturating twin"""
    W, H = frame
    arrs, gI, gD = dead_scene("dead", W, H, tile_w)[:3]
    lens = _oracle_lens(arrs, W, H, tile_w)
    ul = unit_lengths(lens, seg_len)
    assert (ul == seg_len).any() and (ul != seg_len).any() and len(ul) >= 7
    tun = _tuning(tile_w, seg_len, bin_mode)
    got, stg = _hip([a[None] for a in arrs], W, H, gI[None], gD[None], tun)
    _check_stages(stg, lens, seg_len)
    _assert_oracle(got, 0, dead_reference("dead", W, H, tile_w), f"dead {W}x{H} tw{tile_w} s{seg_len}")
    twin = dead_scene("dead", W, H, tile_w, 0.05)[0]
    both, stg2 = _hip([np.stack([x, y]) for x, y in zip(arrs, twin)], W, H, np.stack([gI, gI]), np.stack([gD, gD]), tun)
    _check_stages(stg2, np.concatenate([lens, _oracle_lens(twin, W, H, tile_w)]), seg_len)
    alone = _hip([a[None] for a in twin], W, H, gI[None], gD[None], tun)[0]
    for k in GRADS + ["image", "depth"]:
        assert np.array_equal(both[k][0], got[k][0]) and np.array_equal(both[k][1], alone[k][0]), k
    _assert_oracle(both, 1, dead_reference("dead", W, H, tile_w, 0.05), "dead twin at opacity 0.05")


@gpu
@pytest.mark.parametrize("bin_mode", [1, 2])
def test_capacity_overflow_leaves_the_table_alone(bin_mode):
    """a duplicate capacity below what the scene needs: no list, no unit, and not one word of the table written -- under the guard's
    fills the whole section still holds the fill, and the guards around `saved` are intact"""
    from fresnel_amd import handoff, losses, renderer
    (W, H), tile_w, seg_len = (64, 32), 16, 64
    arrs, gI, gD, lens = _scene("seamsA", W, H, tile_w, seg_len)
    assert lens.sum() > 5
    for pattern in WG.PATTERNS:
        with WG.WorkspaceGuard(pattern, [renderer, losses, handoff]) as guard:
            got, stg = _hip([a[None] for a in arrs], W, H, gI[None], gD[None], _tuning(tile_w, seg_len, bin_mode), workspace=5, guard=guard)
            guard.check(f"at the end of the {pattern[0]} run")
        assert stg["overflow"] == 1 and stg["U"] == 0 and not stg["lens"].any() and stg["seg_off"][-1] == 0
        words = stg["table_words"]
        assert words.numel() == stg["capacity"] > 0 and bool((words == pattern[1]).all()), f"pattern {pattern[0]}: the table was written"
        for k in GRADS:
            assert not got[k].any()
