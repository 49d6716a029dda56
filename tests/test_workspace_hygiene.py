"""Workspace and output-buffer hygiene of every HIP entry point, through the product wrappers (tests/workspace_guard.py).

include/fgs.h promises that the initial content of `saved`, `scratch`, `stats` and of every output is irrelevant, that the
sizes fgs_*_workspace_bytes report are enough, that outputs are fully overwritten and that inputs (and, where it says so,
`saved`) are left alone.  Each case below runs forward and backward under the three fill patterns and once unpatched, and asserts

  A  every guard byte around every buffer is intact after the forward and again after the backward;
  B  every returned tensor, every gradient and the defined part of the integer stages are bitwise identical in all four runs
     (an element the kernels never wrote, or a word read before it was written, fails this);
  C  every input is bitwise what it was; `saved` is unchanged by fgs_backward and by fgs_ssim_backward (whose second backward
     gives the same gradients); fgs_gather_backward leaves the unselected rows exactly zero;
  D  a small call on a scratch buffer warmed by a larger call and then filled with each pattern, and calls interleaved on one
     stream, give the bitwise results of their own fresh runs;
  E  the scenes no other test has (capacity exactly reached; few Gaussians with 1025 ... 1027 lists) also agree with the CPU
     oracle: values within 1e-4 of the maximum of its fp64 run, integer stages bit for bit.

All entries went through the patched allocation sites of their wrappers; none needed a raw ctypes call.  The shapes are small
and chosen where fgs_plan.cpp's layout arithmetic changes branch (which use of the borrowed sort buffer is the largest, tile
width, list builder, forward split, segment length, sort passes)."""
import numpy as np
import pytest
import torch

import workspace_guard as WG
from helpers import rel_to_max, synth_aniso
from sweep_support import check_integer_stages

gpu = pytest.mark.gpu
TOL = 1e-4
GRADS = ["positions", "scales", "rotations", "colors", "opacities"]
WAVELENGTHS = np.array([0.07, 0.052, 0.043], np.float32)


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
    """A leaf that SHARES the input's memory: what the wrapper reads is what the untouched-input check looks at."""
    return t.detach().requires_grad_(True)


def _run(fn, inputs, **kw):
    return WG.run_patterns(fn, inputs, _mods(), **kw)


def _sync_check(guard, when):
    torch.cuda.synchronize()
    if isinstance(guard, WG.WorkspaceGuard):
        # a wrapper that stops allocating through the patched sites would go unguarded without anybody noticing
        assert guard.records, f"no allocation of the wrapper went through the guard {when}"
    guard.check(when)


# =================================================================================================================================
# blend / phase renderer
# =================================================================================================================================
def _blend_scene(c):
    """numpy inputs of one blend case: five (B,N,.) arrays [, phases], upstream gradients, per-image views."""
    Bn, N, W, H = c["B"], c["N"], c["W"], c["H"]
    rs = np.random.RandomState(c["seed"])
    kind = c.get("scene", "aniso")
    per = []
    for b in range(Bn):
        if kind == "full":  # large and central: every Gaussian covers every tile of the 40 x 24 frame
            pos = np.concatenate([rs.standard_normal((N, 2)) * 0.15, -2.0 + 0.2 * rs.uniform(-1, 1, (N, 1))], 1).astype(np.float32)
            scale = rs.uniform(0.5, 0.8, (N, 3)).astype(np.float32)
            quat = rs.standard_normal((N, 4)).astype(np.float32)
            col = rs.random_sample((N, 3)).astype(np.float32)
            opa = (rs.random_sample(N) * 0.05).astype(np.float32)
            a = (pos, scale, quat, col, opa)
        elif kind == "opaque":  # long lists that saturate: what saturation_skip skips
            a = synth_aniso(N, c["seed"] + b, opacity_max=1.3, spread=0.2, smin=0.1, smax=0.3)
        else:
            a = synth_aniso(N, c["seed"] + b, opacity_max=c.get("opacity_max", 1.0), smax=c.get("smax", 0.13))
        if c.get("behind") == b:  # this image entirely behind the camera: zero duplicates
            a[0][:, 2] = np.abs(a[0][:, 2]) + 0.5
        per.append(a)
    arrs = [np.stack([p[i] for p in per]) for i in range(5)]
    out = dict(zip(GRADS, arrs))
    if c.get("phase"):
        out["phases"] = rs.random_sample((Bn, N)).astype(np.float32)
    out["gI"] = rs.standard_normal((Bn, 3, H, W)).astype(np.float32)
    out["gD"] = (rs.standard_normal((Bn, H, W)) * 0.1).astype(np.float32)
    views = []
    for b in range(Bn if c.get("cams") == "per" else 1):
        V = np.eye(4, dtype=np.float32)
        a = 0.15 * (b - 1) if c.get("cams") == "per" else 0.0
        V[0, 0], V[0, 2], V[2, 0], V[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
        V[0, 3] = 0.1 * b
        views.append(V)
    return out, views


def _blend_cameras(c, views):
    from fresnel_amd.renderer import Camera
    W, H = c["W"], c["H"]
    cams = []
    for V in views:
        cam = Camera(0.8 * W, 0.8 * W, W / 2, H / 2, W, H)
        cam.set_view(torch.from_numpy(V))
        cams.append(cam)
    return cams if c.get("cams") == "per" else cams[0]


def _oracle_cameras(c, views):
    from oracle import fgs_oracle as orc
    W, H = c["W"], c["H"]
    return [orc.make_camera(V, 0.8 * W, 0.8 * W, W / 2, H / 2, W, H) for V in views]


def _defined_stages(saved, dims):
    """The part of the integer stages in `saved` that a forward defines: visibility keys, bboxes of the visible Gaussians, the
    depth order of the visible ones, per-tile list lengths and (for non-empty lists) starts, list entries up to the total
    length, the duplicate count and overflow flag and, where the path has depth segments, their tables and counters.  Unused
    capacity is legitimately undefined and is masked out."""
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
    D = int(st["counters"][0])
    assert int(st["counters"][1]) == 0, "duplicate capacity overflow flag set"
    assert 0 <= D <= st["layout"].dup_capacity
    out = dict(st_key=key, st_order=order, st_bbox=bbox, st_list_len=lens.clone(), st_list_start=starts,
               st_dup_ids=st["dup_ids"][:D].clone(), st_counters=st["counters"][:2].clone())
    if st["layout"].seg_capacity:
        # the depth segments and their counters ([2] units, [4] seg_len, [5] fwd_variant) exist on the non-phase path only:
        # with use_phase nothing writes or reads those words (include/fgs.h)
        U = int(st["counters"][2])
        assert 0 <= U <= st["layout"].seg_capacity and int(st["seg_off"][-1]) == U
        out.update(st_seg_counters=st["counters"][[2, 4, 5]].clone(), st_seg_off=st["seg_off"].clone(),
                   st_seg_tile=st["seg_tile"][:U].clone())
    return out, st


def _numpy_stages(st, img, dep):
    out = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in st.items()}
    out["image"], out["depth"] = img.detach().cpu().numpy(), dep.detach().cpu().numpy()
    return out


class _BlendCall:
    """One forward / backward of the blend renderer on persistent device inputs, in two halves (for the interleaved case)."""

    def __init__(self, c, inp, cams):
        self.c, self.inp, self.cams = c, inp, cams
        self.keep = None  # numpy integer stages of the last forward (assertion E)

    def forward(self, guard):
        from fresnel_amd.renderer import TileBasedRenderer
        c, inp = self.c, self.inp
        self.ts = [_leaf(inp[k]) for k in GRADS]
        self.ph = _leaf(inp["phases"]) if c.get("phase") else None
        ren = TileBasedRenderer(c["W"], c["H"], background=c.get("bg", (0.1, 0.2, 0.3)), max_radius=c.get("maxr", 64),
                                use_phase_blending=bool(c.get("phase")), phase_amplitude=0.25,
                                saturation_skip=bool(c.get("sat")))
        ren.tuning = c.get("tuning")
        self.img, self.dep = ren(*self.ts, self.cams, return_depth=True, phases=self.ph)
        node = self.img.grad_fn
        self.saved, self.dims = node.saved_tensors[-1], node.dims
        _sync_check(guard, "after the forward")
        self.out = dict(image=self.img.detach(), depth=self.dep.detach())
        stages, st = _defined_stages(self.saved, self.dims)
        self.out.update(stages)
        self.keep = _numpy_stages(st, self.img, self.dep)
        self.saved_before = self.saved.clone()

    def backward(self, guard):
        ((self.img * self.inp["gI"]).sum() + (self.dep * self.inp["gD"]).sum()).backward()
        _sync_check(guard, "after the backward")
        # `saved` is const in fgs_backward, and the wrapper allows no second backward that would notice
        assert torch.equal(self.saved, self.saved_before), "fgs_backward modified `saved`"
        for k, t in zip(GRADS, self.ts):
            self.out["grad_" + k] = t.grad
        if self.ph is not None:
            self.out["grad_phases"] = self.ph.grad
        return self.out

    def __call__(self, guard):
        self.forward(guard)
        return self.backward(guard)


def _blend_setup(c):
    arrs, views = _blend_scene(c)
    inp = {k: _up(v) for k, v in arrs.items()}
    return arrs, views, inp, _BlendCall(c, inp, _blend_cameras(c, views))


def _case(id_, **kw):
    kw.setdefault("seed", 1000 + sum(map(ord, id_)))
    return pytest.param(kw, id=id_)


_FRAMES = [(1, 1, 1), (3, 13, 48), (1, 100, 72), (3, 200, 136)]  # (B, W, H)
BLEND_CASES = [
    _case(f"ragged-N{N}-B{Bn}-{W}x{H}-tw{tw}", N=N, B=Bn, W=W, H=H, tuning=dict(tile_w=tw))
    for N in (1, 63, 257, 777) for (Bn, W, H) in _FRAMES for tw in (16, 32)
] + [
    _case("wide-tiles-automatic", N=2048, B=3, W=512, H=512, expect_tile_w=32, smax=0.05),
] + [
    _case(f"bin{bm}-seg{sl}", N=777, B=3, W=200, H=136, tuning=dict(bin_mode=bm, seg_len=sl)) for bm in (1, 2) for sl in (64, 128)
] + [
    _case(f"fwd_variant{fv}", N=777, B=2, W=100, H=72, tuning=dict(fwd_variant=fv)) for fv in (1, 2, 4, 8, 16, -1, -2, -4)
] + [
    _case("saturation_skip", N=777, B=2, W=100, H=72, sat=True, scene="opaque"),
    _case("phase-N257", N=257, B=1, W=100, H=72, phase=True),
    _case("phase-N777-B3", N=777, B=3, W=200, H=136, phase=True),
] + [
    _case(f"sort_mode{sm}", N=9000, B=2, W=128, H=96, tuning=dict(sort_mode=sm), smax=0.04, opacity_max=0.5) for sm in range(12)
] + [
    _case("per-image-cameras", N=777, B=3, W=100, H=72, cams="per", opacity_max=1.3),
    _case("max_radius4", N=777, B=3, W=200, H=136, maxr=4),
    _case("max_radius64", N=777, B=3, W=200, H=136, maxr=64, smax=0.4),
    _case("one-image-behind-the-camera", N=257, B=3, W=100, H=72, behind=1),
]
# scenes no other test covers: also checked against the CPU oracle (assertion E)
FULL_CASE = dict(N=300, B=2, W=40, H=24, maxr=64, scene="full", seed=4024)
STAR_CASES = [
    pytest.param(FULL_CASE, id="capacity-exactly-reached"),
    _case("four-gaussians-1025-lists", N=4, B=1, W=656, H=400, opacity_max=0.9),   # 41 x 25 tiles
    _case("four-gaussians-1026-lists", N=4, B=2, W=432, H=304, opacity_max=0.9),   # 2 x 27 x 19 tiles
    _case("four-gaussians-1027-lists", N=4, B=1, W=208, H=1264, opacity_max=0.9),  # 13 x 79 tiles
]


def _oracle_runs(c, arrs, views):
    """Per image: (fp32 Rendered, fp64 Rendered, fp64 gradients)."""
    from oracle import fgs_oracle as orc
    ocams = _oracle_cameras(c, views)
    res = []
    for b in range(c["B"]):
        cam = ocams[b if len(ocams) > 1 else 0]
        a = [arrs[k][b] for k in GRADS]
        kw = dict(bg=c.get("bg", (0.1, 0.2, 0.3)), max_radius=float(c.get("maxr", 64)))
        r32 = orc.render(*a, cam, **kw)
        with orc.fp64():
            r64 = orc.render(*a, cam, **kw)
            g64 = orc.render_backward(r64, arrs["gI"][b], arrs["gD"][b])
        res.append((r32, r64, g64))
    return res


def _oracle_duplicates(c, arrs, views, tile_w=16):
    """Total length of the oracle's tile lists over the batch, and the smallest number of tiles one visible Gaussian touches."""
    from oracle import fgs_oracle as orc
    ocams = _oracle_cameras(c, views)
    total, fewest = 0, None
    for b in range(c["B"]):
        r = orc.render(*[arrs[k][b] for k in GRADS], ocams[b if len(ocams) > 1 else 0], bg=(0, 0, 0), max_radius=float(c.get("maxr", 64)))
        ranges, ids = orc.tile_lists(r.vis_sorted, r.proj["bbox"], c["W"], c["H"], 16, tile_w=tile_w)
        total += int(ranges[-1])
        per = np.bincount(np.asarray(ids[:ranges[-1]]), minlength=c["N"])
        fewest = int(per.min()) if fewest is None else min(fewest, int(per.min()))
    return total, fewest


def test_capacity_full_scene_reaches_dup_capacity_exactly():
    """CPU: in the capacity-full scene (40 x 24 frame = 3 x 2 tiles, max_radius 64) the oracle's tile lists hold every Gaussian
    in every tile, and their total length IS FgsSavedLayout.dup_capacity: one more duplicate would not fit."""
    from fresnel_amd import _binding as B
    c = FULL_CASE
    arrs, views = _blend_scene(c)
    L = B.saved_layout(B.make_dims(c["B"], c["N"], c["W"], c["H"], c["maxr"]))
    assert (L.tiles_x, L.tiles_y, L.tile_w) == (3, 2, 16)
    total, fewest = _oracle_duplicates(c, arrs, views)
    assert fewest == 6
    assert total == c["B"] * c["N"] * 6 == L.dup_capacity


@gpu
@pytest.mark.parametrize("c", BLEND_CASES)
def test_blend_renderer_buffers(c):
    """A, B, C for fgs_forward / fgs_backward at the shapes and tunings where the plan arithmetic changes branch."""
    _, _, inp, call = _blend_setup(c)
    runs = _run(call, inp)
    if "expect_tile_w" in c:
        assert int(call.keep["layout"].tile_w) == c["expect_tile_w"]
    if c.get("tuning", {}).get("tile_w"):
        assert int(call.keep["layout"].tile_w) == c["tuning"]["tile_w"]
    if c.get("behind") is not None:
        b = c["behind"]
        z = runs["zero"]
        assert bool((z["st_key"][b] == -1).all()) and int(z["st_list_len"][b].sum()) == 0
        assert all(not bool(z["grad_" + k][b].any()) for k in GRADS), "culled Gaussians must get zero gradients"


@gpu
@pytest.mark.parametrize("c", STAR_CASES)
def test_blend_renderer_buffers_new_scenes_vs_oracle(c):
    """A, B, C and E: capacity exactly reached (every Gaussian in every tile: D == dup_capacity), and four Gaussians with
    1025 / 1026 / 1027 lists per call -- the case the comment on FgsPlan.tile_table_words names (the tile tables borrow a sort
    buffer that B * N words once sized)."""
    arrs, views, inp, call = _blend_setup(c)
    runs = _run(call, inp)
    z = runs["zero"]
    st = call.keep
    L = st["layout"]
    if c.get("scene") == "full":
        assert int(z["st_counters"][0]) == L.dup_capacity == c["B"] * c["N"] * 6
    else:
        assert c["B"] * L.tiles_x * L.tiles_y == {656: 1025, 432: 1026, 208: 1027}[c["W"]]
    # the last run's stages are the unpatched run's; B made them equal to the zero run's
    for b, (r32, r64, g64) in enumerate(_oracle_runs(c, arrs, views)):
        check_integer_stages(st, b, r32, c["W"], c["H"])
        for k, got, want in [("image", z["image"][b], r64.image), ("depth", z["depth"][b], r64.depth)] + \
                            [("grad_" + k, z["grad_" + k][b], g64[k]) for k in GRADS]:
            err = rel_to_max(got.cpu().numpy(), want)
            print(f"{k} image {b}: {err:.2e} of max vs the fp64 oracle")
            assert err <= TOL, (k, b, err)


@gpu
def test_stale_scratch_from_a_larger_call():
    """D: renderer._SCRATCH keeps one buffer per stream and hands it to calls of every shape.  Warm it with a larger call, fill
    it in place with each pattern, then make the smaller call: bitwise the smaller call's own fresh result."""
    from fresnel_amd import renderer as R
    big = dict(N=3000, B=3, W=200, H=136, seed=51)
    small = dict(N=63, B=1, W=13, H=48, seed=52)
    _, _, inp_b, call_b = _blend_setup(big)
    _, _, inp_s, call_s = _blend_setup(small)
    R.release_scratch()
    fresh = {k: v.clone() for k, v in call_s(WG._NoGuard(_mods())).items()}

    def fn(guard):
        R.release_scratch()
        call_b(guard)
        bufs = list(R._SCRATCH.values())
        assert len(bufs) == 1
        big_bytes = bufs[0].numel()
        guard.poison(bufs[0])
        out = call_s(guard)
        assert list(R._SCRATCH.values())[0] is bufs[0] and bufs[0].numel() == big_bytes, "the smaller call must reuse the buffer"
        return out

    runs = _run(fn, dict(inp_s, **{"big_" + k: v for k, v in inp_b.items()}), keep_scratch=True)
    # every run -- stale scratch filled with each pattern, and the unpatched "big then small" -- against the fresh small call
    assert list(runs) == ["zero", "one", "ff", "unpatched"]
    for name, out in runs.items():
        WG.assert_outputs_match(fresh, out, "fresh", "stale-" + name)


@gpu
def test_interleaved_calls_on_one_stream():
    """D: forward A, forward B (another shape), backward A, backward B on one stream and one shared scratch buffer equal the
    separate runs bitwise."""
    ca = dict(N=777, B=3, W=200, H=136, seed=61)
    cb = dict(N=257, B=1, W=100, H=72, seed=62, tuning=dict(tile_w=32))
    _, _, inp_a, call_a = _blend_setup(ca)
    _, _, inp_b, call_b = _blend_setup(cb)
    none = WG._NoGuard(_mods())
    sep_a = {k: v.clone() for k, v in call_a(none).items()}
    sep_b = {k: v.clone() for k, v in call_b(none).items()}

    def fn(guard):
        call_a.forward(guard)
        call_b.forward(guard)
        out = {"a_" + k: v for k, v in call_a.backward(guard).items()}
        out.update({"b_" + k: v for k, v in call_b.backward(guard).items()})
        return out

    runs = _run(fn, dict({"a_" + k: v for k, v in inp_a.items()}, **{"b_" + k: v for k, v in inp_b.items()}))
    want = dict({"a_" + k: v for k, v in sep_a.items()}, **{"b_" + k: v for k, v in sep_b.items()})
    WG.assert_outputs_match(want, runs["unpatched"], "separate", "interleaved")


# =================================================================================================================================
# ASM and wave-field renderers
# =================================================================================================================================
def _splat_scene(W, H, N, Bn, C, seed, planes=None, P=6, near=0.3, far=2.2):
    rs = np.random.RandomState(seed)
    per = []
    depth_of = np.linspace(near, far, P)
    for b in range(Bn):
        pos, scale, quat, col, opa = synth_aniso(N, seed + 1 + b, opacity_max=0.9, smin=0.03, smax=0.1)
        pos[:, 1] *= H / W * 0.6 if H > W else 1.0
        if planes is not None and P > 1:  # Gaussians in a few chosen planes only: the others stay empty
            pl = rs.choice(planes[b % len(planes)], N)
            pos[:, 2] = -(depth_of[pl] + rs.uniform(-0.25, 0.25, N) * (far - near) / (P - 1)).astype(np.float32)
        else:
            pos[:, 2] = -rs.uniform(near, far - 0.2, N).astype(np.float32)
        per.append((pos, scale, quat, col, opa))
    arrs = dict(zip(GRADS, [np.stack([p[i] for p in per]) for i in range(5)]))
    arrs["phases"] = (rs.random_sample((Bn, N, 3) if C == 3 else (Bn, N)) * 2 * np.pi).astype(np.float32)
    arrs["gI"] = rs.standard_normal((Bn, 3, H, W)).astype(np.float32)
    arrs["gD"] = (rs.standard_normal((Bn, H, W)) * 0.1).astype(np.float32)
    arrs["wl"] = WAVELENGTHS.copy()
    return arrs


SPLAT_FRAMES = [(72, 64, 1), (96, 256, 1), (40, 1024, 1), (160, 96, 2)]  # (W, H, B): column-FFT set + a non-square batch
ASM_CASES = [pytest.param(dict(W=W, H=H, B=Bn, C=C), id=f"{W}x{H}-B{Bn}-C{C}") for (W, H, Bn) in SPLAT_FRAMES for C in (1, 3)] + [
    pytest.param(dict(W=96, H=64, B=2, C=3, P=16, planes=[[0, 1, 2, 3, 13], [5, 6]], near=0.4, far=2.4), id="empty-planes"),
    pytest.param(dict(W=96, H=64, B=2, C=1, P=1), id="single-plane"),
    pytest.param(dict(W=136, H=72, B=2, C=3, P=11, bin_mode=2), id="radix-binning"),
]


@gpu
@pytest.mark.parametrize("c", ASM_CASES)
def test_asm_renderer_buffers(c):
    """A, B, C for fgs_asm_forward / fgs_asm_backward (the backward consumes `saved` by contract, so `saved` is not compared)."""
    from fresnel_amd.renderer import ASMWaveFieldRenderer, Camera
    dev = _dev()
    W, H, Bn, P = c["W"], c["H"], c["B"], c.get("P", 6)
    near, far = c.get("near", 0.3), c.get("far", 2.2)
    inp = {k: _up(v) for k, v in _splat_scene(W, H, 240, Bn, c["C"], 700 + W + H, c.get("planes"), P, near, far).items()}
    inp.pop("gD")
    f = 0.8 * min(W, H)
    cam = Camera(f, f, W / 2, H / 2, W, H)
    ren = ASMWaveFieldRenderer(W, H, background=(0.05, 0.1, 0.15), num_depth_planes=P, depth_range=(near, far), focal_depth=0.9,
                               pixel_pitch=1.0 / 200.0).to(dev)
    if "bin_mode" in c:
        ren.bin_mode = c["bin_mode"]

    def fn(guard):
        ts = [_leaf(inp[k]) for k in GRADS]
        ph, wl = _leaf(inp["phases"]), _leaf(inp["wl"])
        img = ren(*ts, cam, phases=ph, wavelengths_rgb=wl)
        _sync_check(guard, "after the forward")
        out = dict(image=img.detach())
        (img * inp["gI"]).sum().backward()
        _sync_check(guard, "after the backward")
        out.update({"grad_" + k: t.grad for k, t in zip(GRADS, ts)})
        out.update(grad_phases=ph.grad, grad_wavelengths=wl.grad)
        return out

    runs = _run(fn, inp)
    assert all(bool(torch.isfinite(v).all()) for v in runs["zero"].values())


@gpu
@pytest.mark.parametrize("W,H,Bn", SPLAT_FRAMES)
@pytest.mark.parametrize("C", [1, 3])
def test_wave_renderer_buffers(W, H, Bn, C):
    """A, B, C for fgs_wave_forward / fgs_wave_backward."""
    from fresnel_amd.renderer import Camera, WaveFieldRenderer
    dev = _dev()
    inp = {k: _up(v) for k, v in _splat_scene(W, H, 240, Bn, C, 800 + W + H).items()}
    inp.pop("wl")
    f = 0.8 * min(W, H)
    cam = Camera(f, f, W / 2, H / 2, W, H)
    ren = WaveFieldRenderer(W, H, background=(0.05, 0.1, 0.15)).to(dev)

    def fn(guard):
        ts = [_leaf(inp[k]) for k in GRADS]
        ph = _leaf(inp["phases"])
        img, dep = ren(*ts, cam, return_depth=True, phases=ph)
        _sync_check(guard, "after the forward")
        out = dict(image=img.detach(), depth=dep.detach())
        ((img * inp["gI"]).sum() + (dep * inp["gD"]).sum()).backward()
        _sync_check(guard, "after the backward")
        out.update({"grad_" + k: t.grad for k, t in zip(GRADS, ts)})
        out.update(grad_phases=ph.grad)
        return out

    runs = _run(fn, inp)
    assert all(bool(torch.isfinite(v).all()) for v in runs["zero"].values())


# =================================================================================================================================
# propagator
# =================================================================================================================================
@gpu
@pytest.mark.parametrize("band_limit", [True, False])
@pytest.mark.parametrize("H,W,C", [(64, 12, 1), (128, 100, 3), (256, 256, 3)])
def test_propagator_buffers(H, W, C, band_limit):
    """A, B, C for fgs_asm_propagate_forward / backward incl. the gradients of z and the wavelengths.  Without the band limit
    the pitch is 1/16 (no evanescent bin at these wavelengths: finite results)."""
    from fresnel_amd.renderer import AngularSpectrumPropagator
    dev = _dev()
    rs = np.random.RandomState(H + W + C)
    cplx = lambda: (rs.standard_normal((H, W, C)) + 1j * rs.standard_normal((H, W, C))).astype(np.complex64)
    inp = dict(field=_up(cplx()), g=_up(cplx()), z=torch.tensor(0.37, device=dev), wl=_up(WAVELENGTHS[:C]))
    prop = AngularSpectrumPropagator(H, W, pixel_pitch=1.0 / 200.0 if band_limit else 1.0 / 16.0, band_limit=band_limit).to(dev)

    def fn(guard):
        f, z, wl = _leaf(inp["field"]), _leaf(inp["z"]), _leaf(inp["wl"])
        out = prop.propagate(f, z, wl)
        _sync_check(guard, "after the forward")
        res = dict(out=out.detach())
        (out * inp["g"].conj()).real.sum().backward()
        _sync_check(guard, "after the backward")
        res.update(grad_field=f.grad, grad_z=z.grad, grad_wl=wl.grad)
        return res

    runs = _run(fn, inp)
    assert all(bool(torch.isfinite(torch.view_as_real(v) if v.is_complex() else v).all()) for v in runs["zero"].values())


# =================================================================================================================================
# spectral and Helmholtz losses
# =================================================================================================================================
LOSS_SHAPES = [(2, 3, 64, 64), (2, 3, 96, 200)]


def _loss_inputs(shape, seed):
    Bn, C, H, W = shape
    rs = np.random.RandomState(seed)
    return dict(rendered=_up(rs.random_sample(shape).astype(np.float32)), target=_up(rs.random_sample(shape).astype(np.float32)),
                depth=_up(rs.uniform(0.2, 1.0, (Bn, H, W)).astype(np.float32)), wl=torch.tensor(0.05, device=_dev()))


@gpu
@pytest.mark.parametrize("shape", LOSS_SHAPES)
@pytest.mark.parametrize("grad_target", [False, True])
def test_frequency_loss_buffers(shape, grad_target):
    from fresnel_amd.losses import FrequencyDomainLoss
    inp = _loss_inputs(shape, 11)
    inp.pop("depth"), inp.pop("wl")

    def fn(guard):
        r = _leaf(inp["rendered"])
        t = _leaf(inp["target"]) if grad_target else inp["target"]
        loss = FrequencyDomainLoss(cutoff=0.1, high_weight=2.0)(r, t)
        _sync_check(guard, "after the forward")
        out = dict(loss=loss.detach())
        loss.backward()
        _sync_check(guard, "after the backward")
        out.update(grad_rendered=r.grad, grad_target=t.grad if grad_target else None)
        return out

    _run(fn, inp)


@gpu
@pytest.mark.parametrize("shape", LOSS_SHAPES)
@pytest.mark.parametrize("grad_depth,grad_wl", [(False, False), (True, False), (False, True), (True, True)])
def test_phase_retrieval_loss_buffers(shape, grad_depth, grad_wl):
    from fresnel_amd.losses import PhaseRetrievalLoss
    inp = _loss_inputs(shape, 12)

    def fn(guard):
        r = _leaf(inp["rendered"])
        d = _leaf(inp["depth"]) if grad_depth else inp["depth"]
        wl = _leaf(inp["wl"]) if grad_wl else inp["wl"]
        loss = PhaseRetrievalLoss(focal_depth=0.5)(r, inp["target"], d, wl)
        _sync_check(guard, "after the forward")
        out = dict(loss=loss.detach())
        loss.backward()
        _sync_check(guard, "after the backward")
        out.update(grad_rendered=r.grad, grad_depth=d.grad if grad_depth else None, grad_wl=wl.grad if grad_wl else None)
        return out

    _run(fn, inp)


@gpu
@pytest.mark.parametrize("shape", LOSS_SHAPES + [(3, 64, 64)])
def test_helmholtz_loss_buffers(shape):
    from fresnel_amd.losses import wave_equation_loss
    inp = dict(field=_up(np.random.RandomState(13).standard_normal(shape).astype(np.float32)))

    def fn(guard):
        u = _leaf(inp["field"])
        loss = wave_equation_loss(u, 0.05)
        _sync_check(guard, "after the forward")
        out = dict(loss=loss.detach())
        loss.backward()
        _sync_check(guard, "after the backward")
        out.update(grad_field=u.grad)
        return out

    _run(fn, inp)


# =================================================================================================================================
# SSIM
# =================================================================================================================================
@gpu
@pytest.mark.parametrize("shape", [(2, 3, 37, 52), (1, 3, 11, 14)])  # the second: one window position along H (smaller is refused)
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("gx,gy", [(True, False), (False, True), (True, True), (False, False)])
def test_ssim_buffers(shape, per_image, gx, gy):
    """A, B, C for fgs_ssim_forward / backward; the backward leaves `saved` bitwise unchanged and a second backward through the
    same forward gives the same gradients."""
    from fresnel_amd.losses import ssim
    rs = np.random.RandomState(21)
    inp = dict(x=_up(rs.random_sample(shape).astype(np.float32)), y=_up(rs.random_sample(shape).astype(np.float32)))
    inp["g"] = _up(rs.standard_normal(shape[0]).astype(np.float32))

    def fn(guard):
        x = _leaf(inp["x"]) if gx else inp["x"]
        y = _leaf(inp["y"]) if gy else inp["y"]
        s = ssim(x, y, data_range=1.0, size_average=not per_image)
        _sync_check(guard, "after the forward")
        out = dict(ssim=s.detach())
        if not (gx or gy):
            assert not s.requires_grad
            return out
        saved = s.grad_fn.saved_tensors[2]
        before = saved.clone()
        loss = (s * inp["g"]).sum() if per_image else s * 0.7
        loss.backward(retain_graph=True)
        _sync_check(guard, "after the backward")
        assert torch.equal(saved, before), "fgs_ssim_backward modified `saved`"
        first = [t.grad.clone() if t.requires_grad else None for t in (x, y)]
        for t in (x, y):
            t.grad = None
        loss.backward()
        _sync_check(guard, "after the second backward")
        assert torch.equal(saved, before), "the second fgs_ssim_backward modified `saved`"
        for name, t, g1 in zip("xy", (x, y), first):
            if g1 is not None:
                assert WG.same_bits(t.grad, g1), f"second backward: other gradient of {name}"
        out.update(grad_x=x.grad if gx else None, grad_y=y.grad if gy else None)
        return out

    _run(fn, inp)


def test_ssim_refuses_a_frame_narrower_than_the_window():
    """The wrapper does not accept a frame smaller than the window (it raises before it looks at the device), so there is no
    such GPU case."""
    from fresnel_amd import _binding as B
    from fresnel_amd.losses import ssim
    with pytest.raises(B.FgsError, match="smaller than the 11-tap window"):
        ssim(torch.zeros(1, 3, 16, 10), torch.zeros(1, 3, 16, 10))


# =================================================================================================================================
# pixel losses
# =================================================================================================================================
# what fresnel_amd.train.compute_losses can ask of pixel_losses: (density, zones, rendered_depth, target_depth); the last three:
# a depth map that has no partner (the training script always has a target depth, so a renderer without depth output and no
# zones gives the first two of them) enables no term and must leave no trace
PIXEL_COMBOS = [(False, False, False, False), (True, False, False, False), (False, True, False, True), (True, True, False, True),
                (False, False, True, True), (True, False, True, True), (False, True, True, True), (True, True, True, True),
                (False, False, False, True), (True, False, False, True), (False, False, True, False)]


@gpu
@pytest.mark.parametrize("shape", [(2, 23, 29), (3, 64, 48)])
@pytest.mark.parametrize("den,zones,rd,td", PIXEL_COMBOS)
def test_pixel_losses_buffers(shape, den, zones, rd, td):
    from fresnel_amd.losses import pixel_losses
    Bn, H, W = shape
    rs = np.random.RandomState(31)
    inp = dict(rendered=_up(rs.random_sample((Bn, 3, H, W)).astype(np.float32)), target=_up(rs.random_sample((Bn, 3, H, W)).astype(np.float32)),
               rendered_depth=_up(rs.random_sample((Bn, H, W)).astype(np.float32)), target_depth=_up(rs.random_sample((Bn, H, W)).astype(np.float32)),
               density=_up(rs.random_sample((Bn, 1, H, W)).astype(np.float32)))

    def fn(guard):
        r = _leaf(inp["rendered"])
        d = _leaf(inp["rendered_depth"]) if rd else None
        terms = pixel_losses(r, inp["target"], d, inp["target_depth"] if td else None, density=inp["density"] if den else None,
                             vlm_weight=0.5, zones=8 if zones else None)
        _sync_check(guard, "after the forward")
        assert set(terms) == {"rgb"} | ({"boundary"} if zones and td else set()) | ({"depth"} if rd and td else set())
        out = {k: v.detach() for k, v in terms.items()}
        sum(w * terms[k] for w, k in zip((1.0, 0.1, 0.5), ("rgb", "boundary", "depth")) if k in terms).backward()
        _sync_check(guard, "after the backward")
        out.update(grad_rendered=r.grad, grad_depth=d.grad if rd else None)
        return out

    _run(fn, inp)


@gpu
@pytest.mark.parametrize("term", ["depth", "boundary", "boundary-hard"])
def test_pixel_losses_single_term_buffers(term):
    """The staged API with the rgb term off: the depth term alone, the boundary term alone (soft and hard mask).  `out` is three
    floats whatever is requested: a term that is not requested is written as 0, under every fill."""
    from fresnel_amd import losses as L
    Bn, H, W = 2, 23, 29
    rs = np.random.RandomState(32)
    inp = dict(rendered=_up(rs.random_sample((Bn, 3, H, W)).astype(np.float32)), target=_up(rs.random_sample((Bn, 3, H, W)).astype(np.float32)),
               rendered_depth=_up(rs.random_sample((Bn, H, W)).astype(np.float32)), target_depth=_up(rs.random_sample((Bn, H, W)).astype(np.float32)))
    one = torch.ones((), device=_dev())

    def fn(guard):
        if term == "depth":
            st = L.pixel_loss_begin(inp["rendered"], inp["target"], inp["rendered_depth"], inp["target_depth"], rgb=False)
        else:
            st = L.pixel_loss_begin(inp["rendered"], inp["target"], None, inp["target_depth"],
                                    zones=L.FresnelZoneSpec(soft=term == "boundary"), rgb=False)
        out3 = L.pixel_loss_forward(st)
        _sync_check(guard, "after the forward")
        stats_before = st.stats.clone()
        g_r, g_d = L.pixel_loss_backward(st, one, one, one)
        _sync_check(guard, "after the backward")
        assert WG.same_bits(st.stats, stats_before), "fgs_pixel_loss_backward modified `stats`"
        return dict(out=out3, grad_rendered=g_r, grad_depth=g_d)

    runs = _run(fn, inp)
    z = runs["zero"]["out"]
    assert [float(v) != 0.0 for v in z] == [False, term != "depth", term == "depth"]


# =================================================================================================================================
# gather
# =================================================================================================================================
@gpu
@pytest.mark.parametrize("pc", [0, 1, 3])
@pytest.mark.parametrize("Bn,n_in,n_out", [(1, 50, 50), (4, 50, 1), (4, 300, 77), (1, 300, 299)])
def test_gather_buffers(pc, Bn, n_in, n_out):
    """A, B, C for fgs_gather_forward / backward; after the backward the unselected rows of every gradient are exactly zero and
    the selected rows are the upstream gradients."""
    from fresnel_amd.handoff import _GatherGaussians
    rs = np.random.RandomState(41 + pc)
    trail = [(3,), (3,), (4,), (3,), ()] + ([(3,) if pc == 3 else ()] if pc else [])
    names = GRADS + (["phases"] if pc else [])
    inp = {k: _up(rs.standard_normal((Bn, n_in) + t).astype(np.float32)) for k, t in zip(names, trail)}
    inp.update({"g_" + k: _up(rs.standard_normal((Bn, n_out) + t).astype(np.float32)) for k, t in zip(names, trail)})
    idx = rs.permutation(n_in)[:n_out].astype(np.int64)
    inp["indices"] = _up(idx)

    def fn(guard):
        ts = [_leaf(inp[k]) for k in names]
        outs = _GatherGaussians.apply(inp["indices"], *ts[:5], ts[5] if pc else None)
        _sync_check(guard, "after the forward")
        assert (outs[5] is None) == (pc == 0)
        res = {"out_" + k: o.detach() for k, o in zip(names, outs)}
        sum((o * inp["g_" + k]).sum() for k, o in zip(names, outs)).backward()
        _sync_check(guard, "after the backward")
        res.update({"grad_" + k: t.grad for k, t in zip(names, ts)})
        return res

    runs = _run(fn, inp)
    rest = _up(np.setdiff1d(np.arange(n_in), idx))
    idx = inp["indices"]
    for name, out in runs.items():
        for k in names:
            assert torch.equal(out["out_" + k], inp[k][:, idx]), (name, k)
            g = out["grad_" + k]
            assert torch.equal(g[:, idx], inp["g_" + k]), (name, k)
            assert not bool(g[:, rest].view(torch.int32).any()), f"{name}: unselected rows of grad_{k} are not exactly zero"
