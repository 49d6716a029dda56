"""fgs_surface_count / fgs_surface_emit through fresnel_amd.surface on the GPU, judged against tests/surface_checker.py (pinned by
tests/test_surface_checker.py): offsets, the per-point state and the row kinds bit for bit, every float tensor within the
project's rule (1e-4 of the tensor's largest magnitude).  The tensors built from exact operations only -- colours, base positions,
base scales -- have their largest difference printed (pytest -s / -rP)."""
import functools

import numpy as np
import pytest
import torch

import surface_checker as C
import workspace_guard as WG
from helpers import rel_to_max

gpu = pytest.mark.gpu
KEYS = ("positions", "scales", "rotations", "colors", "opacities")
TOL = 1e-4


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


# ---- inputs (already curve-adjusted depths: the tests call count / emit, below the pow of surface_gaussians) ---------------------------
def _depth(H, W, seed, kind="mixed"):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    if kind == "checker":    # checkerboard plus ramp: an edge every 4 pixels, fan-out up to 12 almost everywhere
        d = ((xx // 4 + yy // 4) % 2) * 0.3 + xx / (2.0 * W) + 0.1
    elif kind == "plateaus":  # piecewise constant, dyadic levels: flat interiors have gx = gy = 0 exactly -> normal (0, 0, 1)
        d = 0.25 + 0.25 * ((xx >= W // 3).astype(np.float32) + (yy >= H // 2).astype(np.float32))
        d[0, 0] = 0.0
    elif kind == "constant":
        d = np.full((H, W), 0.5)
    else:                     # a smooth bowl, two steps and a little noise
        d = 0.15 + 0.5 * ((xx - W / 2) ** 2 + (yy - H / 2) ** 2) / max((W / 2) ** 2 + (H / 2) ** 2, 1.0)
        d = d + 0.2 * (xx > 0.6 * W) + 0.1 * (yy > 0.3 * H) + 0.02 * rs.random_sample((H, W))
    return np.ascontiguousarray(d, dtype=np.float32)


def _color(H, W, seed):
    return np.random.RandomState(seed).random_sample((3, H, W)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(H, W, seed, kind="mixed", with_color=True):
    return _depth(H, W, seed, kind), (_color(H, W, seed + 1) if with_color else None)


_REFS = {}


def _reference(key, depth, color, overrides):
    """The checker's cloud of one image, computed once per (inputs, parameters) and never modified."""
    k = (key, tuple(sorted(overrides.items())))
    if k not in _REFS:
        ref = C.surface_cloud(depth, color, **overrides)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[k] = ref
    return _REFS[k]


def _params(overrides):
    from fresnel_amd.surface import SurfaceGaussianParams
    return SurfaceGaussianParams(**overrides)


def _generate(depths, colors, overrides, dev):
    """count + emit on a batch -> (offsets list, flags (B,P) uint8, dict of numpy outputs, state)"""
    from fresnel_amd import surface
    depth = torch.from_numpy(np.stack(depths)).to(dev)
    color = None if colors[0] is None else torch.from_numpy(np.stack(colors)).to(dev)
    state = surface.count(depth, color, _params(overrides))
    out = surface.emit(state)
    torch.cuda.synchronize()
    return state.offsets_host, state.flags().cpu().numpy(), {k: out[k].cpu().numpy() for k in KEYS}, state


def _kinds_from_flags(flags, overrides):
    p = C.params_dict(**overrides)
    kinds = []
    for f in flags:
        if f & C.BASE:
            kinds.append(C.K_BASE)
        if f & C.BACK:
            kinds.append(C.K_BACK)
        if f & C.WALLS:
            kinds += [C.K_WALL] * p["shell_wall_segments"]
        if f & C.WRAPS:
            kinds += [C.K_WRAP] * p["wrap_layers"]
        if f & C.FILLS:
            kinds += [C.K_FILL] * p["density_extra_count"]
    return np.array(kinds, np.int32)


def _judge(what, refs, offsets, flags, out, overrides):
    """One batch against its per-image references."""
    want_offsets = np.concatenate([[0], np.cumsum([r["kinds"].size for r in refs])]).tolist()
    assert offsets == want_offsets, f"{what}: offsets {offsets} != {want_offsets}"
    for b, ref in enumerate(refs):
        assert np.array_equal(flags[b], ref["flags"]), f"{what}[{b}]: per-point state differs at {np.nonzero(flags[b] != ref['flags'])[0][:8]}"
        assert np.array_equal(C.rows_per_flag(flags[b], **overrides), ref["counts"]), f"{what}[{b}]: per-point counts"
        assert np.array_equal(_kinds_from_flags(flags[b], overrides), ref["kinds"]), f"{what}[{b}]: row kinds"
        lo, hi = offsets[b], offsets[b + 1]
        got = {k: out[k][lo:hi] for k in KEYS}
        assert all(np.isfinite(ref[k]).all() for k in KEYS), f"{what}[{b}]: the reference is not finite"
        for k in KEYS:
            err = rel_to_max(got[k], ref[k])
            assert err <= TOL, f"{what}[{b}] {k}: {err:.2e} > {TOL:.0e}"
        base = ref["kinds"] == C.K_BASE
        exact = dict(colors=np.abs(got["colors"] - ref["colors"]), base_positions=np.abs(got["positions"] - ref["positions"])[base],
                     base_scales=np.abs(got["scales"] - ref["scales"])[base])
        print(f"{what}[{b}]: {hi - lo} rows; max |difference| of the exact-operation tensors: " +
              ", ".join(f"{k} {float(v.max()) if v.size else 0.0:.3g}" for k, v in exact.items()) +
              "; rotations {:.2e}, opacities {:.2e} of max".format(rel_to_max(got["rotations"], ref["rotations"]),
                                                                   rel_to_max(got["opacities"], ref["opacities"])))


def _check_case(name, H, W, depth_seed, kind="mixed", with_color=True, dev=None, **overrides):
    depth, color = _inputs(H, W, depth_seed, kind, with_color)
    ref = _reference((H, W, depth_seed, kind, with_color), depth, color, overrides)
    offsets, flags, out, _ = _generate([depth], [color], overrides, dev or _dev())
    _judge(name, [ref], offsets, flags, out, overrides)
    return ref, out


# ---- frame and subsample seams -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("H, W, sub", [(1, 1, 1), (1, 7, 1), (7, 1, 1), (37, 53, 1), (64, 64, 1), (64, 64, 2), (64, 64, 3)],
                         ids=["1x1", "1x7", "7x1", "37x53", "64x64", "64x64_sub2", "64x64_sub3"])
def test_frames_and_subsampling(H, W, sub):
    ref, _ = _check_case(f"{H}x{W}/{sub}", H, W, 11 + H, subsample=sub)
    if H * W > 1:
        assert ref["kinds"].size > 0


@gpu
def test_scan_across_blocks_and_65536_rows():
    """96 x 96 checkerboard plus ramp: 9 216 points (36 blocks of 256), fan-out up to 12, more than 65 536 rows."""
    ref, _ = _check_case("96x96 checker", 96, 96, 3, kind="checker")
    assert ref["counts"].size > 9000 and int(ref["counts"].max()) == 12 and ref["kinds"].size > 65536


# ---- parameter seams, all on the 37 x 53 frame ---------------------------------------------------------------------------------------------
PARAM_CASES = {
    "shell_off": dict(shell_enabled=False), "wrap_off": dict(wrap_enabled=False), "density_off": dict(density_enabled=False),
    "no_wall_segments": dict(shell_wall_segments=0), "no_wrap_layers": dict(wrap_layers=0), "no_extra": dict(density_extra_count=0),
    "no_walls": dict(shell_connect_walls=False),
    "strength_0": dict(normal_strength=0.0), "strength_half": dict(normal_strength=0.5), "strength_1": dict(normal_strength=1.0),
    "not_normalised": dict(normalize_extent=0.0),
    "intrinsics": dict(fx=40.0, fy=45.0, cx=20.5, cy=13.25, depth_scale=2.0, seed=99, wrap_layers=5, density_extra_count=2),
}


@gpu
@pytest.mark.parametrize("case", sorted(PARAM_CASES))
def test_parameters(case):
    _check_case(case, 37, 53, 48, **PARAM_CASES[case])


@gpu
def test_without_colour_image():
    _, out = _check_case("grey", 37, 53, 48, with_color=False)
    assert np.unique(out["colors"][:, 0]).size <= 2      # 0.7 and the darkened back surfaces


@gpu
def test_identity_branch_of_quaternion_from_normal():
    """Flat interiors of a piecewise-constant depth: gx = gy = 0 exactly, normal (0, 0, 1), rotation exactly the identity."""
    ref, out = _check_case("plateaus", 24, 30, 2, kind="plateaus")
    ident = (ref["kinds"] == C.K_BASE) & (ref["rotations"] == np.array([1, 0, 0, 0], np.float32)).all(axis=1)
    assert ident.sum() > 100
    assert (out["rotations"][ident] == np.array([1, 0, 0, 0], np.float32)).all()


# ---- batches, repeatability -----------------------------------------------------------------------------------------------------------------
def _batch3():
    """Three unequal images of one frame size; the middle one emits nothing (constant depth: confidence 0 everywhere)."""
    return [_inputs(37, 53, 48), (_depth(37, 53, 0, "constant"), _color(37, 53, 9)), _inputs(37, 53, 50)]


@gpu
def test_batch_with_an_empty_image_equals_single_calls_and_repeats():
    dev = _dev()
    items = _batch3()
    refs = [_reference(("batch3", i), d, c, {}) for i, (d, c) in enumerate(items)]
    assert refs[1]["kinds"].size == 0 and refs[0]["kinds"].size != refs[2]["kinds"].size
    offsets, flags, out, _ = _generate([d for d, _ in items], [c for _, c in items], {}, dev)
    _judge("batch of three", refs, offsets, flags, out, {})
    assert offsets[1] == offsets[2]
    again = _generate([d for d, _ in items], [c for _, c in items], {}, dev)
    assert again[0] == offsets and np.array_equal(again[1], flags)
    for k in KEYS:
        assert np.array_equal(again[2][k].view(np.int32), out[k].view(np.int32)), f"{k}: two runs differ"
    for b, (d, c) in enumerate(items):
        o1, f1, out1, _ = _generate([d], [c], {}, dev)
        assert o1 == [0, offsets[b + 1] - offsets[b]] and np.array_equal(f1[0], flags[b])
        for k in KEYS:
            assert np.array_equal(out1[k].view(np.int32), out[k][offsets[b]:offsets[b + 1]].view(np.int32)), f"image {b} {k}: batch != single"


# ---- capacity ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_capacity_below_the_total_is_an_error_and_writes_nothing():
    from fresnel_amd import _binding as B
    from fresnel_amd import surface
    dev = _dev()
    depth, color = _inputs(37, 53, 48)
    state = surface.count(torch.from_numpy(depth[None]).to(dev), torch.from_numpy(color[None]).to(dev), _params({}))
    good = surface.emit(state)
    total = state.offsets_host[-1]
    assert total > 0 and state.status() == 0

    def poisoned():
        return {k: torch.full_like(good[k][:total - 1], -123.0) for k in KEYS}

    outs = poisoned()
    with pytest.raises(B.FgsError, match="capacity"):            # the public entry: an error, nothing launched
        surface.emit(state, capacity=total - 1, outputs=outs)
    surface.emit_raw(state, outs, total - 1)                      # the C entry itself: the kernel refuses, and says so
    torch.cuda.synchronize()
    assert state.status() == 1
    assert all(bool((outs[k] == -123.0).all()) for k in KEYS)
    assert state.offsets.cpu().tolist() == state.offsets_host     # and the state is intact: a proper emit still works
    more = surface.emit(state, capacity=total + 5, outputs={k: torch.full((total + 5,) + good[k].shape[1:], -123.0, device=dev) for k in KEYS})
    torch.cuda.synchronize()
    assert state.status() == 0
    for k in KEYS:
        assert torch.equal(more[k][:total], good[k]) and bool((more[k][total:] == -123.0).all())


# ---- NaN / +Inf depth pixels: the outcome include/fgs.h defines --------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_depth_pixels(bad):
    """offsets monotone, never more rows per point than 2 + walls + wraps + fills (12), nothing written outside the rows below
    the total; a NaN pixel's own point is kept and emits its base row; the other image of the batch is untouched by it."""
    from fresnel_amd import surface
    dev = _dev()
    clean, color = _inputs(37, 53, 48)
    dirty = clean.copy()
    dirty[5, 7] = bad
    dirty[20, 30] = bad
    depth = torch.from_numpy(np.stack([dirty, clean])).to(dev)
    col = torch.from_numpy(np.stack([color, color])).to(dev)
    state = surface.count(depth, col, _params({}))
    offsets = state.offsets.cpu().tolist()
    P = 37 * 53
    assert offsets[0] == 0 and offsets[0] <= offsets[1] <= offsets[2] and offsets[2] <= 12 * 2 * P
    flags = state.flags().cpu().numpy()
    rows = C.rows_per_flag(flags)
    assert rows.max() <= 12 and [int(rows[0].sum()), int(rows[1].sum())] == [offsets[1], offsets[2] - offsets[1]]
    if bad != bad:
        assert flags[0, 5 * 53 + 7] & C.BASE and flags[0, 20 * 53 + 30] & C.BASE
    total = offsets[2]
    outs = {k: torch.full((total + 64,) + ((3,) if k in ("positions", "scales", "colors") else (4,) if k == "rotations" else ()),
                          -123.0, device=dev) for k in KEYS}
    surface.emit(state, capacity=total + 64, outputs=outs)
    torch.cuda.synchronize()
    for k in KEYS:
        assert bool((outs[k][total:] == -123.0).all()), f"{k}: written beyond the total"
    ref = _reference((37, 53, 48, "mixed", True), clean, color, {})
    assert np.array_equal(flags[1], ref["flags"])
    for k in KEYS:
        assert rel_to_max(outs[k][offsets[1]:total].cpu().numpy(), ref[k]) <= TOL


# ---- buffer hygiene -----------------------------------------------------------------------------------------------------------------------
@gpu
def test_surface_buffers():
    """Guard bytes around scratch, offsets and the five outputs, the three fill patterns, inputs untouched, every row below the
    total written (tests/workspace_guard.py): a batch with an empty image, subsample 3 on a frame it does not divide, a colour
    image, more wrap layers than the default."""
    from fresnel_amd import surface
    dev = _dev()
    items = _batch3()
    inp = dict(depth=torch.from_numpy(np.stack([d for d, _ in items])).to(dev),
               image=torch.from_numpy(np.stack([c for _, c in items])).to(dev))
    params = _params(dict(subsample=3, wrap_layers=4))

    def fn(guard):
        state = surface.count(inp["depth"], inp["image"], params)
        torch.cuda.synchronize()
        if isinstance(guard, WG.WorkspaceGuard):
            assert len(guard.records) == 2, "scratch and offsets must come from the guarded allocator"
        guard.check("after the count")
        out = surface.emit(state)
        torch.cuda.synchronize()
        if isinstance(guard, WG.WorkspaceGuard):
            assert len(guard.records) == 7
        guard.check("after the emit")
        return dict(out, offsets=state.offsets, flags=state.flags())

    runs = WG.run_patterns(fn, inp, [surface])
    zero = runs["zero"]
    assert zero["positions"].shape[0] == int(zero["offsets"][-1]) > 0
    assert all(bool(torch.isfinite(zero[k]).all()) for k in KEYS)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
E2E_PARAMS = dict(base_size=0.03)


def e2e_depth():
    """64 x 64 depth in [0, 1] (before the curve): a tilted plane with a raised square."""
    yy, xx = np.mgrid[0:64, 0:64].astype(np.float32)
    d = 0.3 + 0.4 * xx / 63.0 + 0.1 * yy / 63.0
    d[20:44, 20:44] += 0.15
    return np.ascontiguousarray(d, dtype=np.float32)


def e2e_camera():
    from fresnel_amd.renderer import create_camera_from_pose
    # in front of the normalised cloud (extent 3 around the origin), zoomed so that it fills the frame: the oracle's image of the
    # checker's cloud then differs from the background on 72 % of the pixels
    return create_camera_from_pose(0.0, 0.0, 64, focal_length_mult=2.2, distance=5.0)


def e2e_covered_share(image, background=0.0):
    return float((np.abs(np.asarray(image) - background).max(axis=0) > 1e-3).mean())


def test_e2e_scene_meets_its_condition_on_the_cpu_oracle():
    """The condition of the GPU test below -- the rendered cloud differs from the background on more than half the pixels -- holds
    for the CHECKER's cloud rendered by the C oracle: the scene was chosen so, before the kernel ever ran."""
    from oracle import fgs_oracle as orc
    cloud = C.surface_cloud(e2e_depth() ** np.float32(0.7), None, **E2E_PARAMS)
    cam = e2e_camera()
    ocam = orc.make_camera(cam.view_matrix.numpy(), cam.fx, cam.fy, cam.cx, cam.cy, 64, 64)
    r = orc.render(cloud["positions"], cloud["scales"], cloud["rotations"], cloud["colors"], cloud["opacities"], ocam, keep_pairs=False)
    assert np.isfinite(r.image).all() and e2e_covered_share(r.image) > 0.5, e2e_covered_share(r.image)


@gpu
def test_end_to_end_file_round_trip_and_render(tmp_path):
    from fresnel_amd import io as fio
    from fresnel_amd import surface
    from fresnel_amd.data import ImageDataset
    from fresnel_amd.renderer import TileBasedRenderer
    dev = _dev()
    depth = torch.from_numpy(e2e_depth()).to(dev)
    cloud, = surface.surface_gaussians(depth[None], None, _params(E2E_PARAMS))
    (tmp_path / "features").mkdir()
    fio.save_gaussians_to_binary(str(tmp_path / "features" / "scene_saag.bin"), cloud)
    has, loaded = ImageDataset(str(tmp_path), image_size=64, load_saag=True).saag_cloud("scene")
    assert has
    for k in KEYS:
        assert torch.equal(loaded["saag_" + k].view(torch.int32), cloud[k].cpu().view(torch.int32)), f"{k}: the round trip changed bits"
    assert cloud["positions"].shape[0] > 4096
    image = TileBasedRenderer(64, 64)(*[cloud[k] for k in KEYS], e2e_camera()).detach().cpu().numpy()
    assert image.shape == (3, 64, 64)
    assert np.isfinite(image).all()
    assert e2e_covered_share(image) > 0.5, e2e_covered_share(image)
