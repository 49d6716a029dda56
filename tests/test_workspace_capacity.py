"""FgsDims.dup_capacity: rasterizer workspaces sized by a duplicate-capacity hint (include/fgs.h, DESIGN.md "capacity and overflow").

CPU: the plan arithmetic with and without a hint, argument handling of make_dims / render_batch / TileBasedRenderer / train.py.
GPU, on one 96 x 80 two-image scene whose duplicate count D comes from the CPU oracle (never from the library under test):

  exact fit   dup_capacity = D (and D + 1, 2 D): under the guard-and-poison harness, bitwise the unhinted call, within 1e-4 of the
              fp64 oracle, counters[0] == counters[3] == D -- the worst case's slack hides a kernel that over-reads a list tail or
              assumes room for one more segment;
  overflow    dup_capacity in {D - 1, D // 4, 1}: guards intact, inputs untouched, flag and demand set, every list empty, every
              output word the quiet NaN, every gradient zero, the same under every fill pattern; the next unhinted call on the
              same stream and the same cached scratch is bitwise its fresh result;
  adaptive    TileBasedRenderer(workspace="adaptive") learns the capacity without a host synchronisation, survives a scene that
              outgrows it (one NaN call, then room) and lets go of the worst-case scratch;
  training    --workspace adaptive trains bit for bit like --workspace worst with smaller workspaces.

The shapes are the smallest at which the arithmetic changes branch: lists of 118 ... 162 entries are multi-segment at seg_len 64
and at 128 (32 x 16 tiles), 30 tiles per image are more than one block of every list kernel's waves, N = 300 is not a multiple of
the 256-rank blocks."""
import functools

import numpy as np
import pytest
import torch

import workspace_guard as WG
from helpers import rel_to_max, synth_aniso, synth_decoder_like

gpu = pytest.mark.gpu
TOL = 1e-4
GRADS = ["positions", "scales", "rotations", "colors", "opacities"]
W, H, N, BN = 96, 80, 300, 2
BG = (0.1, 0.2, 0.3)
QNAN = 0x7FC00000


# =================================================================================================================================
# CPU: plan arithmetic
# =================================================================================================================================
PLAN_DIMS = {
    "config3": dict(batch=8, num_gaussians=32768, width=512, height=512),
    "config3-tw16": dict(batch=8, num_gaussians=32768, width=512, height=512, tuning=dict(tile_w=16)),
    "96x80": dict(batch=BN, num_gaussians=N, width=W, height=H),
    "96x80-tw32-radix": dict(batch=BN, num_gaussians=N, width=W, height=H, tuning=dict(tile_w=32, bin_mode=2, seg_len=128)),
    "phase": dict(batch=16, num_gaussians=8192, width=256, height=256, use_phase=True),
    "saturation_skip": dict(batch=BN, num_gaussians=N, width=W, height=H, saturation_skip=True),
}
LAYOUT_FIELDS = ["total_bytes", "rec", "depth_key", "tile_count", "order", "dup_off", "counters", "ranges", "tile_order", "dup_ids",
                 "pix_state", "phase_ckpt", "dup_capacity", "tiles_x", "tiles_y", "seg_off", "seg_tile", "seg_ckpt", "seg_capacity",
                 "seg_len", "tile_w"]


def _layout_tuple(L):
    return tuple(int(getattr(L, f)) for f in LAYOUT_FIELDS)


@pytest.mark.parametrize("name", list(PLAN_DIMS))
def test_no_hint_and_hints_at_or_above_the_worst_case_give_todays_layout(name):
    from fresnel_amd import _binding as B
    kw = PLAN_DIMS[name]
    d0 = B.make_dims(**kw)
    assert d0.dup_capacity == 0
    L0, bytes0 = B.saved_layout(d0), B.workspace_bytes(d0)
    worst = int(L0.dup_capacity)
    for c in (worst, worst + 1, 2 * worst, 0xFFFFFFFF):
        d = B.make_dims(dup_capacity=c, **kw)
        assert _layout_tuple(B.saved_layout(d)) == _layout_tuple(L0), c
        assert B.workspace_bytes(d) == bytes0, c


@pytest.mark.parametrize("name", list(PLAN_DIMS))
def test_a_hint_below_the_worst_case_sizes_every_list_section(name):
    from fresnel_amd import _binding as B
    kw = PLAN_DIMS[name]
    L0 = B.saved_layout(B.make_dims(**kw))
    saved0, scratch0 = B.workspace_bytes(B.make_dims(**kw))
    worst = int(L0.dup_capacity)
    lists = kw["batch"] * L0.tiles_x * L0.tiles_y
    prev = (0, 0)
    hints = sorted({1, 2, 63, 64, 65, 1000, worst // 4, worst // 2, worst - 65, worst - 1})
    for c in [h for h in hints if 0 < h < worst]:
        d = B.make_dims(dup_capacity=c, **kw)
        L = B.saved_layout(d)
        assert L.dup_capacity == c
        if kw.get("use_phase"):
            assert L.seg_capacity == 0
        else:
            assert L.seg_capacity == c // L.seg_len + lists
        # the tuning never depends on the hint
        assert (L.tile_w, L.seg_len, L.tiles_x, L.tiles_y) == (L0.tile_w, L0.seg_len, L0.tiles_x, L0.tiles_y)
        offs = [L.rec, L.depth_key, L.tile_count, L.order, L.dup_off, L.counters, L.ranges, L.tile_order, L.dup_ids, L.pix_state,
                L.phase_ckpt]
        assert offs == sorted(offs) and all(o % 256 == 0 for o in offs) and offs[-1] <= L.total_bytes
        assert L.seg_off % 256 == 0 and L.seg_tile % 256 == 0 and L.seg_ckpt % 256 == 0
        assert L.phase_ckpt <= L.seg_off <= L.seg_tile <= L.seg_ckpt <= L.total_bytes
        assert L.pix_state - L.dup_ids >= 4 * c, "dup_ids has room for the capacity"
        saved, scratch = B.workspace_bytes(d)
        assert saved == L.total_bytes
        assert saved <= saved0 and scratch <= scratch0 and saved >= prev[0] and scratch >= prev[1], "non-decreasing in the hint"
        # sections are laid out in 256-byte steps (64 list entries) and the tile sort's histogram in blocks of 1024 keys, so a hint
        # within such a step of the worst case may cost the same bytes; from half the worst case down both buffers are smaller
        if c <= worst // 2 and worst >= 1024:
            assert saved < saved0 and scratch < scratch0, (c, saved, saved0, scratch, scratch0)
        prev = (saved, scratch)


def test_config3_workspaces_at_the_recorded_duplicate_count():
    """Config 3 needs 4 099 112 duplicates (BENCH_r05.json): the tracker settles on 5 242 880, a third of the worst case, and
    every list-dependent byte shrinks with it (the records, keys and pixel state do not: profiles/workspace_capacity.txt)."""
    from fresnel_amd import _binding as B
    from fresnel_amd.renderer import CapacityTracker
    kw = PLAN_DIMS["config3"]
    s0, c0 = B.workspace_bytes(B.make_dims(**kw))
    t = CapacityTracker(int(B.saved_layout(B.make_dims(**kw)).dup_capacity))
    t.observe(4_099_112)
    cap = t.capacity()
    assert 1.25 * 4_099_112 <= cap <= 1.25 * 4_099_112 * 1.125 + 1 and cap == 5_242_880
    s1, c1 = B.workspace_bytes(B.make_dims(dup_capacity=cap, **kw))
    print(f"config 3: saved + scratch {s0 + c0} -> {s1 + c1} bytes at capacity {cap}")
    L0, L1 = B.saved_layout(B.make_dims(**kw)), B.saved_layout(B.make_dims(dup_capacity=cap, **kw))
    assert s1 < s0 and c1 < c0
    # dup_ids alone: 4 bytes per entry of capacity
    assert (L0.pix_state - L0.dup_ids) - (L1.pix_state - L1.dup_ids) == 4 * (int(L0.dup_capacity) - cap)


# =================================================================================================================================
# CPU: argument handling
# =================================================================================================================================
def test_make_dims_validates_the_capacity():
    from fresnel_amd import _binding as B
    assert B.make_dims(2, 100, 64, 48, dup_capacity=123).dup_capacity == 123
    assert B.make_dims(2, 100, 64, 48).dup_capacity == 0
    assert B.FgsDims._fields_[-1][0] == "dup_capacity", "appended: every earlier field keeps its offset"
    assert B.FgsDims.dup_capacity.offset == B.FgsDims.sort_mode.offset + 4
    for bad in (-1, 1 << 32, 1.5, True, "7"):
        with pytest.raises((B.FgsError, TypeError, ValueError)):
            B.make_dims(2, 100, 64, 48, dup_capacity=bad)
    assert "0.3" in B.version()


def test_renderer_workspace_argument():
    from fresnel_amd import renderer as R
    r = R.TileBasedRenderer(64, 48)
    assert r.workspace_mode == "worst" and r.dup_capacity == 0 and r.workspace_stats() == {}
    a = R.TileBasedRenderer(64, 48, workspace="adaptive")
    assert a.workspace_mode == "adaptive" and a.dup_capacity == 0 and a.workspace_stats() == {}
    f = R.TileBasedRenderer(64, 48, workspace=5000)
    assert f.workspace_mode == "fixed" and f.dup_capacity == 5000
    for bad in ("best", "", 0, -3, 2.5, True, None, 1 << 32):
        with pytest.raises(ValueError):
            R.TileBasedRenderer(64, 48, workspace=bad)
    # the call-shape cache is keyed by the capacity as well
    cfg = R._Cfg(64, 48, (0.1, 0.2, 0.3), 64, False, 0.25)
    a0, a1 = R._dims_for(2, 100, cfg, False, 1), R._dims_for(2, 100, cfg, False, 1, 777)
    assert a0 is R._dims_for(2, 100, cfg, False, 1, 0) and a1 is R._dims_for(2, 100, cfg, False, 1, 777) and a0 is not a1
    assert a0[0].dup_capacity == 0 and a1[0].dup_capacity == 777 and a1[1] < a0[1] and a1[2] < a0[2]
    assert R._shape_key(2, 100, cfg, False, 1) + (777,) in R._DIMS_CACHE
    # render_batch: a fixed capacity or a renderer's policy object, not both; CPU tensors are refused as ever
    from fresnel_amd import _binding as B
    z = [torch.zeros(1, 4, 3), torch.ones(1, 4, 3), torch.ones(1, 4, 4), torch.ones(1, 4, 3), torch.ones(1, 4)]
    cam = R.Camera(25.6, 25.6, 16, 16, 32, 32)
    with pytest.raises(ValueError):
        R.render_batch(*z, cam, 32, 32, dup_capacity=10, workspace=R._Workspace("adaptive"))
    with pytest.raises(B.FgsError):
        R.render_batch(*z, cam, 32, 32, dup_capacity=10, cam_tensor=torch.zeros(1, 24))


def test_train_refuses_adaptive_workspaces_under_graph_capture(tmp_path):
    from fresnel_amd import train as T
    a = T.arg_parser().parse_args([])
    assert a.workspace == "worst" and T.TrainingConfig().workspace == "worst"
    assert T.arg_parser().parse_args(["--workspace", "adaptive"]).workspace == "adaptive"
    with pytest.raises(SystemExit):
        T.arg_parser().parse_args(["--workspace", "sometimes"])
    T.check_workspace_options("adaptive", False)
    T.check_workspace_options("worst", True)
    with pytest.raises(ValueError, match="hip_graph"):
        T.check_workspace_options("adaptive", True)
    with pytest.raises(SystemExit, match="hip_graph"):  # the argument check comes before anything looks for a GPU
        T.main(["--workspace", "adaptive", "--hip_graph"])
    cfg = T.TrainingConfig(workspace="adaptive", hip_graph=True, device="cpu", output_dir=str(tmp_path))
    with pytest.raises(ValueError, match="hip_graph"):
        T.run_training(cfg, log=lambda *a: None)


# =================================================================================================================================
# GPU: the scene, its oracle and the call
# =================================================================================================================================
def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _mods():
    from fresnel_amd import handoff, losses, renderer
    return [renderer, losses, handoff]


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _leaf(t):
    return t.detach().requires_grad_(True)


def _pad(a, n):
    """Pad a five-array scene to n Gaussians with ones behind the camera (culled: no duplicate, zero gradient)."""
    pos, scale, quat, col, opa = a
    k = n - pos.shape[0]
    if k <= 0:
        return a
    far = np.tile(np.array([[0.0, 0.0, 1.5]], np.float32), (k, 1))
    one = lambda shape: np.full(shape, 0.5, np.float32)
    return (np.concatenate([pos, far]), np.concatenate([scale, one((k, 3)) * 0.1]), np.concatenate([quat, one((k, 4))]),
            np.concatenate([col, one((k, 3))]), np.concatenate([opa, one(k)]))


@functools.lru_cache(maxsize=None)
def _scene(kind="aniso", n=N):
    """numpy inputs: five (B,n,.) arrays, phases, upstream gradients.  Read-only: shared by every test."""
    per = []
    for b in range(BN):
        if kind == "opaque":  # long lists that saturate: what saturation_skip skips
            a = synth_aniso(N, 11 + b, opacity_max=1.3, spread=0.2, smin=0.1, smax=0.3)
        elif kind == "decoder":
            a = synth_decoder_like(400, 21 + b)
        else:
            a = synth_aniso(N, 11 + b)
        per.append(_pad(a, n))
    out = dict(zip(GRADS, [np.stack([p[i] for p in per]) for i in range(5)]))
    rs = np.random.RandomState(77)
    out["phases"] = rs.random_sample((BN, out["positions"].shape[1])).astype(np.float32)
    out["gI"] = rs.standard_normal((BN, 3, H, W)).astype(np.float32)
    out["gD"] = (rs.standard_normal((BN, H, W)) * 0.1).astype(np.float32)
    for v in out.values():
        v.setflags(write=False)
    return out


def _oracle_camera():
    from oracle import fgs_oracle as orc
    return orc.make_camera(np.eye(4, dtype=np.float32), 0.8 * W, 0.8 * W, W / 2, H / 2, W, H)


def _camera():
    from fresnel_amd.renderer import Camera
    return Camera(0.8 * W, 0.8 * W, W / 2, H / 2, W, H)


@functools.lru_cache(maxsize=None)
def _oracle_duplicates(kind, tile_w, n=N):
    """D of the scene from the CPU oracle: project -> depth order -> tile lists."""
    from oracle import fgs_oracle as orc
    arrs, cam, total = _scene(kind, n), _oracle_camera(), 0
    for b in range(BN):
        p = orc.project(arrs["positions"][b], arrs["scales"][b], arrs["rotations"][b], cam, 64.0)
        _, vs = orc.depth_order(p["depth"], p["visible"])
        ranges, _ = orc.tile_lists(vs, p["bbox"], W, H, 16, tile_w=tile_w)
        total += int(ranges[-1])
    return total


@functools.lru_cache(maxsize=None)
def _oracle_runs(kind, phase, n=N):
    """Per image: fp64 oracle image, depth and gradients."""
    from oracle import fgs_oracle as orc
    arrs, cam, res = _scene(kind, n), _oracle_camera(), []
    for b in range(BN):
        a = [arrs[k][b] for k in GRADS]
        with orc.fp64():
            r = orc.render(*a, cam, bg=BG, max_radius=64.0, phases=arrs["phases"][b] if phase else None, phase_amp=0.25)
            g = orc.render_backward(r, arrs["gI"][b], arrs["gD"][b])
        res.append((r.image, r.depth, g))
    return res


def test_the_scene_is_the_one_the_shapes_were_chosen_for():
    """CPU cross-check of the figures the test shapes rest on: multi-segment lists at every tile width, worst case far above D."""
    from fresnel_amd import _binding as B
    assert _oracle_duplicates("aniso", 16) == 1526 + 1501 and _oracle_duplicates("aniso", 32) == 1050 + 1065
    assert int(B.saved_layout(B.make_dims(BN, N, W, H, tuning=dict(tile_w=16))).dup_capacity) == 18000
    assert int(B.saved_layout(B.make_dims(BN, N, W, H, tuning=dict(tile_w=32))).dup_capacity) == 9000
    assert _oracle_duplicates("aniso", 16, 400) == 3027, "culled padding adds no duplicate"
    assert _oracle_duplicates("decoder", 16, 400) > 3840 > 3027, "the decoder-like scene outgrows the learnt capacity"


def _stages(saved, dims):
    """Integer stages a forward defines (as tests/test_workspace_hygiene.py masks them), for a call that fits OR overflowed: after
    an overflow no list exists, so list entries and segment units are empty and dup_ids is wholly undefined."""
    from fresnel_amd import renderer as R
    st = R.inspect_saved(saved, dims)
    key = st["depth_key"].clone()
    vis = key != -1
    nv = vis.sum(dim=1, keepdim=True)
    order = st["order"].clone()
    order[torch.arange(order.shape[1], device=order.device)[None, :] >= nv] = -1
    bbox = st["rec"][:, :, 10:12].contiguous().view(torch.int32).clone()
    bbox[~vis] = 0
    rg = st["ranges"]
    lens = rg[..., 1] - rg[..., 0]
    starts = torch.where(lens > 0, rg[..., 0], torch.zeros_like(lens))
    cnt = st["counters"].clone()
    overflow = int(cnt[1]) != 0
    D = 0 if overflow else int(cnt[0])
    assert 0 <= D <= st["layout"].dup_capacity
    out = dict(st_key=key, st_order=order, st_bbox=bbox, st_list_len=lens.clone(), st_list_start=starts,
               st_dup_ids=st["dup_ids"][:D].clone(), st_counters=cnt[[0, 1, 3]].clone(), st_dup_off=st["dup_off"].clone(),
               st_tile_count=st["tile_count"].clone())
    if st["layout"].seg_capacity:
        U = int(cnt[2])
        assert 0 <= U <= st["layout"].seg_capacity and int(st["seg_off"][-1]) == U
        out.update(st_seg_counters=cnt[[2, 4, 5]].clone(), st_seg_off=st["seg_off"].clone(), st_seg_tile=st["seg_tile"][:U].clone())
    return out, st


def _sync_check(guard, when):
    torch.cuda.synchronize()
    if isinstance(guard, WG.WorkspaceGuard):
        assert guard.records, f"no allocation of the wrapper went through the guard {when}"
    guard.check(when)


class _Call:
    """One forward / backward of the blend or phase renderer on persistent device inputs."""

    def __init__(self, inp, workspace="worst", tuning=None, phase=False, sat=False):
        self.inp, self.workspace, self.tuning, self.phase, self.sat = inp, workspace, tuning, phase, sat
        self.layout = None

    def __call__(self, guard):
        from fresnel_amd.renderer import TileBasedRenderer
        inp = self.inp
        ts = [_leaf(inp[k]) for k in GRADS]
        ph = _leaf(inp["phases"]) if self.phase else None
        ren = TileBasedRenderer(W, H, background=BG, max_radius=64, use_phase_blending=self.phase, phase_amplitude=0.25,
                                saturation_skip=self.sat, workspace=self.workspace)
        ren.tuning = self.tuning
        img, dep = ren(*ts, _camera(), return_depth=True, phases=ph)
        node = img.grad_fn
        saved, dims = node.saved_tensors[-1], node.dims
        _sync_check(guard, "after the forward")
        out = dict(image=img.detach(), depth=dep.detach())
        stages, st = _stages(saved, dims)
        out.update(stages)
        self.layout, self.dims = st["layout"], dims
        before = saved.clone()
        ((img * inp["gI"]).sum() + (dep * inp["gD"]).sum()).backward()
        _sync_check(guard, "after the backward")
        assert torch.equal(saved, before), "fgs_backward modified `saved`"
        for k, t in zip(GRADS, ts):
            out["grad_" + k] = t.grad
        if ph is not None:
            out["grad_phases"] = ph.grad
        return out


def _inputs(kind="aniso", n=N):
    return {k: _up(v) for k, v in _scene(kind, n).items()}


def _variant(id_, **kw):
    return pytest.param(kw, id=id_)


FIT_VARIANTS = [
    _variant(f"tw{tw}-bin{bm}-seg{sl}", tuning=dict(tile_w=tw, bin_mode=bm, seg_len=sl)) for tw in (16, 32) for bm in (1, 2) for sl in (64, 128)
] + [
    _variant("phase-bin1", phase=True, tuning=dict(bin_mode=1)),
    _variant("phase-bin2", phase=True, tuning=dict(bin_mode=2)),
    _variant("saturation_skip-opaque", sat=True, kind="opaque"),
]


def _check_fit(v, capacity_of):
    """A hinted call that fits: the four guarded runs agree bitwise, with the unhinted call too, and with the oracle to 1e-4."""
    kind, phase = v.get("kind", "aniso"), bool(v.get("phase"))
    tile_w = (v.get("tuning") or {}).get("tile_w", 16)
    D = _oracle_duplicates(kind, tile_w)
    cap = capacity_of(D)
    inp = _inputs(kind)
    call = _Call(inp, workspace=cap, tuning=v.get("tuning"), phase=phase, sat=bool(v.get("sat")))
    runs = WG.run_patterns(call, inp, _mods())
    z = runs["zero"]
    L = call.layout
    assert int(L.dup_capacity) == cap and int(call.dims.dup_capacity) == cap and int(L.tile_w) == tile_w
    c0, flag, c3 = (int(x) for x in z["st_counters"])
    print(f"D oracle {D}, capacity {cap}: counters[0] {c0} [1] {flag} [3] {c3}")
    assert flag == 0 and c0 == c3 == D
    # the same call without the hint
    ref_call = _Call(inp, workspace="worst", tuning=v.get("tuning"), phase=phase, sat=bool(v.get("sat")))
    with WG._NoGuard(_mods()) as none:
        ref = {k: t.detach().clone() for k, t in ref_call(none).items()}
    assert int(ref_call.dims.dup_capacity) == 0 and int(ref_call.layout.dup_capacity) > cap
    assert (ref_call.layout.seg_len, ref_call.layout.tile_w) == (L.seg_len, L.tile_w)
    WG.assert_outputs_match(ref, z, "unhinted", "hinted")
    for b, (image, depth, g) in enumerate(_oracle_runs(kind, phase)):
        pairs = [("image", z["image"][b], image), ("depth", z["depth"][b], depth)] + [("grad_" + k, z["grad_" + k][b], g[k]) for k in GRADS]
        if phase:
            pairs.append(("grad_phases", z["grad_phases"][b], g["phases"]))
        for k, got, want in pairs:
            err = rel_to_max(got.cpu().numpy(), want)
            print(f"{k} image {b}: {err:.2e} of max vs the fp64 oracle")
            assert err <= TOL, (k, b, err)


@gpu
@pytest.mark.parametrize("v", FIT_VARIANTS)
def test_exact_fit_is_bitwise_the_unhinted_call(v):
    """dup_capacity == D: not one list entry, segment slot, checkpoint or gradient row to spare."""
    _check_fit(v, lambda D: D)


@gpu
@pytest.mark.parametrize("v,extra", [
    pytest.param(dict(tuning=dict(tile_w=16, bin_mode=1, seg_len=64)), "plus-one", id="D+1-tw16-bin1-seg64"),
    pytest.param(dict(tuning=dict(tile_w=32, bin_mode=2, seg_len=128)), "double", id="2D-tw32-bin2-seg128"),
])
def test_a_capacity_with_room_is_bitwise_the_unhinted_call(v, extra):
    _check_fit(v, (lambda D: D + 1) if extra == "plus-one" else (lambda D: 2 * D))


OVERFLOW_PATHS = {
    "blend-bin1": dict(tuning=dict(tile_w=16, bin_mode=1)),
    "blend-bin2": dict(tuning=dict(tile_w=16, bin_mode=2)),
    "phase": dict(phase=True),
}


@functools.lru_cache(maxsize=None)
def _fresh_unhinted(path):
    """The unhinted call of the scene on a fresh scratch buffer (computed once per path)."""
    v = OVERFLOW_PATHS[path]
    call = _Call(_inputs(), workspace="worst", tuning=v.get("tuning"), phase=bool(v.get("phase")))
    with WG._NoGuard(_mods()) as none:
        return {k: t.detach().clone() for k, t in call(none).items()}


@gpu
@pytest.mark.parametrize("cap_of", ["D-1", "D//4", "1"])
@pytest.mark.parametrize("path", list(OVERFLOW_PATHS))
def test_overflow_is_defined_and_memory_safe(path, cap_of):
    from fresnel_amd import renderer as R
    v = OVERFLOW_PATHS[path]
    phase = bool(v.get("phase"))
    D = _oracle_duplicates("aniso", 16)
    cap = {"D-1": D - 1, "D//4": D // 4, "1": 1}[cap_of]
    inp = _inputs()
    call = _Call(inp, workspace=cap, tuning=v.get("tuning"), phase=phase)
    # guards after the forward and after the backward, inputs untouched, `saved` const, the four runs bitwise equal
    runs = WG.run_patterns(call, inp, _mods())
    L = call.layout
    assert int(L.dup_capacity) == cap
    for name, out in runs.items():
        c0, flag, c3 = (int(x) for x in out["st_counters"])
        assert flag == 1 and c3 == D and c0 == cap, (name, c0, flag, c3)
        assert int(out["st_list_len"].abs().sum()) == 0, f"{name}: a list is not empty"
        if not phase:
            assert int(out["st_seg_counters"][0]) == 0 and int(out["st_seg_off"][-1]) == 0
        for k in ("image", "depth"):
            words = out[k].view(torch.int32)
            assert bool((words == QNAN).all()), f"{name}: {k} holds a word that is not the quiet NaN"
            assert words.numel() == BN * (3 if k == "image" else 1) * H * W
        for k in [g for g in out if g.startswith("grad_")]:
            assert not bool(out[k].view(torch.int32).any()), f"{name}: {k} is not exactly zero"
    # the overflow left no state behind: on the same stream and the same cached scratch buffer, an unhinted call of the scene
    fresh = _fresh_unhinted(path)
    ref_call = _Call(inp, workspace="worst", tuning=v.get("tuning"), phase=phase)
    none = WG._NoGuard(_mods())
    ref_call(none)  # warms the stream's scratch at the worst-case size
    bufs = list(R._SCRATCH.values())
    assert len(bufs) == 1
    ts = [inp[k] for k in GRADS]
    img, dep = R.render_batch(*[_leaf(t) for t in ts], _camera(), W, H, BG, 64, phases=_leaf(inp["phases"]) if phase else None,
                              use_phase_blending=phase, tuning=v.get("tuning"), dup_capacity=cap)
    ((img * inp["gI"]).sum() + (dep * inp["gD"]).sum()).backward()
    assert bool((img.detach().view(torch.int32) == QNAN).all())
    after = ref_call(none)
    assert list(R._SCRATCH.values())[0] is bufs[0], "the three calls shared one scratch buffer"
    WG.assert_outputs_match(fresh, after, "fresh", "after-the-overflow")
    R.release_scratch()


@gpu
def test_adaptive_renderer_learns_overflows_once_and_recovers():
    from fresnel_amd import renderer as R
    from fresnel_amd import _binding as B
    n = 400
    D = _oracle_duplicates("aniso", 16, n)
    inp_a, inp_b = _inputs("aniso", n), _inputs("decoder", n)
    worst = int(B.saved_layout(B.make_dims(BN, n, W, H)).dup_capacity)
    worst_saved, worst_scratch = B.workspace_bytes(B.make_dims(BN, n, W, H))
    R.release_scratch()
    ren = R.TileBasedRenderer(W, H, background=BG, workspace="adaptive")
    cam = _camera()

    def step(inp):
        ts = [_leaf(inp[k]) for k in GRADS]
        img, dep = ren(*ts, cam, return_depth=True)
        node = img.grad_fn
        dims, saved_bytes = node.dims, node.saved_tensors[-1].numel()  # the backward frees the saved tensors
        ((img * inp["gI"]).sum() + (dep * inp["gD"]).sum()).backward()
        out = dict(image=img.detach(), depth=dep.detach())
        out.update({"grad_" + k: t.grad for k, t in zip(GRADS, ts)})
        return out, dims, saved_bytes

    out1, dims1, saved1 = step(inp_a)
    assert dims1.dup_capacity == 0 and saved1 == worst_saved, "the first call of a shape runs at the worst case"
    torch.cuda.synchronize()
    # the second call: capacity learnt from the first one's readback -- and neither its forward nor its backward synchronises
    torch.cuda.set_sync_debug_mode("error")
    try:
        out2, dims2, saved2 = step(inp_a)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    cap2 = int(dims2.dup_capacity)
    print(f"D {D}, learnt capacity {cap2}, worst case {worst}; saved {saved1} -> {saved2} bytes")
    assert D <= cap2 < worst and cap2 == R.quantise_capacity(int(np.ceil(1.25 * D))) == 3840
    assert saved2 < saved1
    WG.assert_outputs_match(out1, out2, "worst-case call", "adaptive call")
    scratch = list(R._SCRATCH.values())
    assert len(scratch) == 1 and scratch[0].numel() < worst_scratch, "the worst-case scratch of call 1 was let go"
    torch.cuda.synchronize()
    # a scene that needs more than the learnt capacity: one NaN image ...
    Db = _oracle_duplicates("decoder", 16, n)
    assert Db > cap2
    out3, dims3, _ = step(inp_b)
    assert int(dims3.dup_capacity) == cap2
    assert bool((out3["image"].view(torch.int32) == QNAN).all()) and bool((out3["depth"].view(torch.int32) == QNAN).all())
    assert all(not bool(out3["grad_" + k].view(torch.int32).any()) for k in GRADS)
    torch.cuda.synchronize()
    # ... and the next call has room
    out4, dims4, _ = step(inp_b)
    assert Db <= int(dims4.dup_capacity) < worst
    for b, (image, depth, g) in enumerate(_oracle_runs("decoder", False, n)):
        for k, got, want in [("image", out4["image"][b], image), ("depth", out4["depth"][b], depth)] + \
                            [("grad_" + k, out4["grad_" + k][b], g[k]) for k in GRADS]:
            assert bool(torch.isfinite(got).all()), k
            err = rel_to_max(got.cpu().numpy(), want)
            print(f"{k} image {b}: {err:.2e} of max vs the fp64 oracle")
            assert err <= TOL, (k, b, err)
    stats = ren.workspace_stats()
    assert len(stats) == 1
    (s,) = stats.values()
    assert s["overflows"] == 1 and s["last_demand"] == Db and s["capacity"] == int(dims4.dup_capacity)
    assert s["bytes"] == sum(B.workspace_bytes(dims4)) < worst_saved + worst_scratch
    R.release_scratch()


@gpu
def test_training_with_adaptive_workspaces_matches_the_worst_case_run(tmp_path):
    """One step per epoch, so the epoch history is the per-step loss: bitwise equal, nothing skipped, smaller workspaces from the
    second step on."""
    import json
    from fresnel_amd.train import TrainingConfig, run_training
    _dev()
    hist = {}
    for mode in ("worst", "adaptive"):
        cfg = TrainingConfig(batch_size=2, epochs=4, lr=1e-3, image_size=64, feature_size=6, feature_dim=16, gaussians_per_patch=4,
                             device="cuda:0", steps_per_epoch=1, save_interval=100, output_dir=str(tmp_path / mode), log_interval=1000,
                             workspace=mode, seed=3)
        run_training(cfg, log=lambda *a: None)
        hist[mode] = json.load(open(tmp_path / mode / "training_history_exp2.json"))
    w, a = hist["worst"], hist["adaptive"]
    print("workspace_mb worst", w["workspace_mb"], "adaptive", a["workspace_mb"])
    for k in ("total", "rgb"):
        assert len(w[k]) == 4 and w[k] == a[k], f"per-step {k} losses differ: {w[k]} vs {a[k]}"
    assert w["skipped_batches"] == a["skipped_batches"] == [0] * 4
    assert w["capacity_overflows"] == a["capacity_overflows"] == [0] * 4
    assert len(set(w["workspace_mb"])) == 1 and a["workspace_mb"][0] <= w["workspace_mb"][0]
    assert all(x < w["workspace_mb"][0] for x in a["workspace_mb"][1:]), (a["workspace_mb"], w["workspace_mb"])
