"""fgs_surface_emit_guided / fgs_surface_guided_backward through fresnel_amd.surface on the GPU: identity maps against the plain emit
bit for bit, patch seams by exact dyadic scaling, forward and backward against tests/guided_surface_checker.py (pinned by
tests/test_guided_surface_checker.py), batches, buffer hygiene, the autograd path from FeatureGuidedSAAG's parameters and one
--experiment 3 training step.

Tolerances.  Float tensors of the forward: 1e-4 of the tensor's largest magnitude against the checker's fp64 run (the project's
rule).  g_mods and parameter gradients: the same, or -- where the checker's own fp32 run is more than 5e-5 of the largest magnitude
from its fp64 run -- at most twice as far from fp64 as that fp32 run (the README's referee rule); no more elements may be decided
by the referee than the checker's fp32 run itself needs, and no element is left out."""
import functools
import math

import numpy as np
import pytest
import torch

import guided_surface_checker as G
import surface_checker as C
import workspace_guard as WG
from helpers import rel_to_max

gpu = pytest.mark.gpu
KEYS = ("positions", "scales", "rotations", "colors", "opacities")
GRAD_KEYS = ("positions", "scales", "rotations", "opacities")
WIDTH = dict(positions=3, scales=3, rotations=4, colors=3, opacities=0)
TOL = 1e-4


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


# ---- inputs: the depth kinds of tests/test_surface_gpu.py, restated ----------------------------------------------------------------------
def _depth(H, W, seed, kind="mixed"):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    if kind == "checker":
        d = ((xx // 4 + yy // 4) % 2) * 0.3 + xx / (2.0 * W) + 0.1
    elif kind == "plateaus":
        d = 0.25 + 0.25 * ((xx >= W // 3).astype(np.float32) + (yy >= H // 2).astype(np.float32))
        d[0, 0] = 0.0
    elif kind == "constant":
        d = np.full((H, W), 0.5)
    else:
        d = 0.15 + 0.5 * ((xx - W / 2) ** 2 + (yy - H / 2) ** 2) / max((W / 2) ** 2 + (H / 2) ** 2, 1.0)
        d = d + 0.2 * (xx > 0.6 * W) + 0.1 * (yy > 0.3 * H) + 0.02 * rs.random_sample((H, W))
    return np.ascontiguousarray(d, dtype=np.float32)


def _color(H, W, seed):
    return np.random.RandomState(seed).random_sample((3, H, W)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(H, W, seed, kind="mixed"):
    d, c = _depth(H, W, seed, kind), _color(H, W, seed + 1)
    d.setflags(write=False)
    c.setflags(write=False)
    return d, c


def _random_mods(B, Hp, Wp, seed):
    """Seeded maps inside the decoder's ranges: 1 +- 0.5, +- 0.1, 1 +- 0.3, 1 +- 0.3, 1 +- 0.5, 1 +- 0.3."""
    u = np.random.RandomState(seed).uniform(-1.0, 1.0, (B, 6, Hp, Wp))
    centre = np.array(G.IDENTITY).reshape(1, 6, 1, 1)
    width = np.array([0.5, 0.1, 0.3, 0.3, 0.5, 0.3]).reshape(1, 6, 1, 1)
    return (centre + width * u).astype(np.float32)


def _identity_mods(B, Hp, Wp):
    return np.broadcast_to(np.array(G.IDENTITY, np.float32).reshape(1, 6, 1, 1), (B, 6, Hp, Wp)).copy()


def _params(overrides):
    from fresnel_amd.surface import SurfaceGaussianParams
    return SurfaceGaussianParams(**overrides)


def _count(depths, colors, overrides, dev):
    from fresnel_amd import surface
    depth = torch.from_numpy(np.stack(depths)).to(dev)
    color = None if colors[0] is None else torch.from_numpy(np.stack(colors)).to(dev)
    return surface.count(depth, color, _params(overrides))


def _emit_guided(state, mods, dev):
    from fresnel_amd import surface
    out = surface.emit_guided(state, torch.from_numpy(mods).to(dev))
    torch.cuda.synchronize()
    return out


def _upstream(total, seed):
    rs = np.random.RandomState(seed)
    return {k: rs.standard_normal((total, WIDTH[k]) if WIDTH[k] else (total,)).astype(np.float32) for k in GRAD_KEYS}


GRAD_COMBOS = ("all",) + GRAD_KEYS


def _checker_grads(depths, colors, mods, overrides, upstream, dtype):
    """d sum_k <upstream_k, rows_k> / d mods through the checker, for every combination of GRAD_COMBOS -> {combo: (B,6,Hp,Wp) fp64}."""
    m = torch.from_numpy(mods).to(dtype).requires_grad_(True)
    clouds = G.guided_clouds(np.stack(depths), None if colors[0] is None else np.stack(colors), m, dtype=dtype, **overrides)
    terms, lo = {}, 0
    for k in GRAD_KEYS:
        terms[k] = 0.0
    for c in clouds:
        n = c["positions"].shape[0]
        for k in GRAD_KEYS:
            terms[k] = terms[k] + (torch.from_numpy(upstream[k][lo:lo + n]).to(dtype) * c[k]).sum()
        lo += n
    out = {}
    for combo in GRAD_COMBOS:
        loss = sum(terms.values()) if combo == "all" else terms[combo]
        g, = torch.autograd.grad(loss, m, retain_graph=True, allow_unused=True)
        out[combo] = (torch.zeros_like(m) if g is None else g).double().numpy()
    return out, clouds


_GRAD_REFS = {}


def _grad_reference(key, depths, colors, mods, overrides, upstream_seed):
    """The checker's fp64 and fp32 gradients of one case, computed once and never modified."""
    if key not in _GRAD_REFS:
        plain_total = sum(C.surface_cloud(d, c, **overrides)["kinds"].size for d, c in zip(depths, colors))
        up = _upstream(plain_total, upstream_seed)
        g64, clouds = _checker_grads(depths, colors, mods, overrides, up, torch.float64)
        g32, _ = _checker_grads(depths, colors, mods, overrides, up, torch.float32)
        for d in (g64, g32):
            for v in d.values():
                v.setflags(write=False)
        _GRAD_REFS[key] = (up, g64, g32, clouds)
    return _GRAD_REFS[key]


def _judge_grad(what, got, g64, g32):
    """The tolerance rule of this file's docstring; prints the figures before it asserts."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all() and np.isfinite(g64).all() and np.isfinite(g32).all(), f"{what}: non-finite gradient"
    m = float(np.abs(g64).max())
    m = m if m > 0 else 1.0
    err, e32 = np.abs(got - g64), np.abs(g32 - g64)
    plain = err <= TOL * m
    referee = ~plain & (e32 > 5e-5 * m) & (err <= 2.0 * e32)
    needs32 = int((e32 > TOL * m).sum())
    print(f"{what}: max |g| {m:.3e}; error {err.max() / m:.2e} of max (checker fp32: {e32.max() / m:.2e}); "
          f"{int(referee.sum())} element(s) by the referee rule, the checker's fp32 run needs {needs32}; {got.size} elements, none left out")
    bad = ~(plain | referee)
    assert not bad.any(), f"{what}: {int(bad.sum())} element(s) outside the rule, worst {float((err / m)[bad].max()):.2e} of max"
    assert int(referee.sum()) <= needs32, f"{what}: {int(referee.sum())} elements by the referee rule, the checker's fp32 run needs {needs32}"


# ---- 1. identity maps are the plain emit, bit for bit ------------------------------------------------------------------------------------
FRAMES = [(64, 64, 1), (64, 64, 2), (64, 64, 3), (37, 53, 1), (1, 1, 1), (1, 7, 1), (7, 1, 1)]


@gpu
@pytest.mark.parametrize("Hp, Wp", [(37, 37), (1, 1)], ids=["37x37", "1x1"])
@pytest.mark.parametrize("H, W, sub", FRAMES, ids=[f"{h}x{w}_sub{s}" for h, w, s in FRAMES])
def test_identity_maps_are_the_plain_emit_bit_for_bit(H, W, sub, Hp, Wp):
    from fresnel_amd import surface
    dev = _dev()
    depth, color = _inputs(H, W, 11 + H)
    state = _count([depth], [color], dict(subsample=sub), dev)
    plain = surface.emit(state)
    guided = _emit_guided(state, _identity_mods(1, Hp, Wp), dev)
    assert state.status() == 0
    if H * W > 1:
        assert plain["positions"].shape[0] > 0
    for k in KEYS:
        assert torch.equal(guided[k].view(torch.int32), plain[k].view(torch.int32)), f"{k}: identity maps changed bits"
    flags = state.flags().cpu().numpy()[0]
    first = np.concatenate([[0], np.cumsum(C.rows_per_flag(flags, subsample=sub))[:-1]])
    assert np.array_equal(guided["point_rows"].cpu().numpy()[0], np.where((flags & C.BASE) != 0, first, -1))


# ---- 2. patch seams, without the checker ---------------------------------------------------------------------------------------------------
SEAMS = {
    "64px_over_37": (64, 64, 1, 37, 37),
    "53px_over_5": (37, 53, 1, 5, 5),
    "7px_over_37": (1, 7, 1, 37, 37),
    "sub3_empty_patches": (64, 64, 3, 37, 37),
}


@gpu
@pytest.mark.parametrize("case", sorted(SEAMS))
def test_patch_seams_by_exact_dyadic_scaling(case):
    """opacity_mult and base_size_mult take {1, 0.5, 2} in patterns that differ between neighbouring patches; a power of two
    commutes with every rounding, so each base row's opacity and tangent scale is the plain emit's value times its patch's."""
    from fresnel_amd import surface
    H, W, sub, Hp, Wp = SEAMS[case]
    dev = _dev()
    depth, color = _inputs(H, W, 11 + H)
    state = _count([depth], [color], dict(subsample=sub), dev)
    plain = {k: v.cpu().numpy() for k, v in surface.emit(state).items()}
    vals = np.array([1.0, 0.5, 2.0], np.float32)
    py, px = np.mgrid[0:Hp, 0:Wp]
    mods = _identity_mods(1, Hp, Wp)
    mods[0, 5] = vals[(px + 2 * py) % 3]
    mods[0, 4] = vals[(2 * px + py + 1) % 3]
    out = _emit_guided(state, mods, dev)
    rows = out["point_rows"].cpu().numpy()[0]
    gw = (W + sub - 1) // sub
    idx = np.nonzero(rows >= 0)[0]
    assert idx.size > 0
    xs, ys = (idx % gw) * sub, (idx // gw) * sub
    ppy, ppx = (ys * Hp) // H, (xs * Wp) // W
    if case == "sub3_empty_patches":
        owned = np.zeros((Hp, Wp), bool)
        owned[ppy, ppx] = True
        assert not owned.all(), "the case must leave some patches without a grid point"
    assert np.unique(ppx).size > 1 or W == 1
    r = rows[idx]
    op, sc = out["opacities"].cpu().numpy(), out["scales"].cpu().numpy()
    assert np.array_equal(op[r], plain["opacities"][r] * mods[0, 5][ppy, ppx]), "opacity: a base row read another patch"
    assert np.array_equal(sc[r, 0], plain["scales"][r, 0] * mods[0, 4][ppy, ppx]), "tangent scale: a base row read another patch"
    assert np.array_equal(out["positions"].cpu().numpy()[r], plain["positions"][r])
    assert np.array_equal(out["colors"].cpu().numpy(), plain["colors"])


# ---- 3. forward against the checker --------------------------------------------------------------------------------------------------------
FORWARD = {
    "64x64_mixed_37x37": (64, 64, "mixed", 37, 37, {}),
    "37x53_checker_sub2_5x5": (37, 53, "checker", 5, 5, dict(subsample=2)),
    "24x30_plateaus_strength_half": (24, 30, "plateaus", 37, 37, dict(normal_strength=0.5)),
}


@gpu
@pytest.mark.parametrize("case", sorted(FORWARD))
def test_forward_against_the_checker(case):
    H, W, kind, Hp, Wp, overrides = FORWARD[case]
    dev = _dev()
    depth, color = _inputs(H, W, 48, kind)
    mods = _random_mods(1, Hp, Wp, 7)
    ref = G.guided_cloud(depth, color, torch.from_numpy(mods[0]), dtype=torch.float64, **overrides)
    state = _count([depth], [color], overrides, dev)
    out = _emit_guided(state, mods, dev)
    assert state.offsets_host == [0, ref["kinds"].size] and ref["kinds"].size > 0
    assert np.array_equal(state.flags().cpu().numpy()[0], ref["flags"])
    assert np.array_equal(out["point_rows"].cpu().numpy()[0], ref["point_rows"])
    for k in KEYS:
        want = ref[k].numpy()
        assert np.isfinite(want).all()
        err = rel_to_max(out[k].cpu().numpy(), want)
        print(f"{case} {k}: {err:.2e} of max")
        assert err <= TOL, f"{case} {k}: {err:.2e} > {TOL:.0e}"


# ---- 4. backward against the checker's fp64 autograd -------------------------------------------------------------------------------------
def _plateau_threshold():
    """The fp32 normalized gradient of the plateaus' interior step points: edge_threshold is set to it, and edge_threshold_add to 0 on
    every other patch row, so that points sit EXACTLY on ng == edge_threshold' (the strict compare: edge_factor 1, no gradient)."""
    depth, color = _inputs(64, 64, 2, "plateaus")
    g = G._geometry(depth, color, C.params_dict())
    vals, counts = np.unique(g["ng"][g["ng"] > 0], return_counts=True)
    return float(vals[np.argmax(counts)])


BACKWARD = {
    # name: (H, W, kind, Hp, Wp, overrides)
    "64x64_mixed": (64, 64, "mixed", 37, 37, {}),
    "64x64_checker": (64, 64, "checker", 37, 37, {}),
    "64x64_plateaus": (64, 64, "plateaus", 37, 37, "plateau"),
    "64x64_sub3_empty_patches": (64, 64, "mixed", 37, 37, dict(subsample=3)),
    "33x47_one_patch_split_and_fold": (33, 47, "mixed", 1, 1, {}),
    "1x1": (1, 1, "mixed", 1, 1, {}),
}


def _backward_case(case):
    H, W, kind, Hp, Wp, overrides = BACKWARD[case]
    depth, color = _inputs(H, W, 2 if kind == "plateaus" else 48, kind)
    mods = _random_mods(1, Hp, Wp, 21)
    if overrides == "plateau":
        overrides = dict(edge_threshold=_plateau_threshold())
        mods[0, 1, 0::2] = 0.0
    up, g64, g32, clouds = _grad_reference(case, [depth], [color], mods, overrides, 5)
    return depth, color, mods, overrides, up, g64, g32, clouds


@pytest.mark.parametrize("case", sorted(BACKWARD))
def test_backward_cases_meet_their_conditions_on_the_cpu(case):
    """Before the kernel runs: the checker's gradients are finite on the chosen seeds, every channel is reached (where the cloud has
    rows), the plateaus case holds points exactly on the threshold and on the lerp branch, the subsample-3 case holds empty
    patches, and the checker's fp32 run meets the rule it referees (no element left out)."""
    depth, color, mods, overrides, up, g64, g32, clouds = _backward_case(case)
    for combo in GRAD_COMBOS:
        _judge_grad(f"{case} checker fp32 {combo}", g32[combo], g64[combo], g32[combo])
    if clouds[0]["kinds"].size:
        assert all(np.abs(g64["all"][0, c]).max() > 0 for c in range(6)), "a channel without any gradient"
        assert np.abs(g64["rotations"][0, 3]).max() > 0 and not g64["rotations"][0, [0, 1, 2, 4, 5]].any()
        assert not g64["positions"][0, [0, 1, 2, 3, 5]].any() and not g64["opacities"][0, [0, 3, 4]].any()
    if case == "64x64_plateaus":
        g = G._geometry(depth, color, C.params_dict(**overrides))
        py, px = G.patch_of(g["xs"], g["ys"], 64, 64, 37, 37)
        th32 = np.float32(overrides["edge_threshold"]) + mods[0, 1][py, px]
        emits = (clouds[0]["flags"][g["sel"]] & C.BASE) != 0
        assert int((emits & (g["ng"] == th32)).sum()) > 10, "no point exactly on the threshold"
        assert int((emits & (g["q"][0] == 1.0)).sum()) > 100, "no point on the lerp branch"
    if case == "64x64_sub3_empty_patches":
        assert int((np.abs(g64["all"][0]).max(axis=0) == 0).sum()) > 100


@gpu
@pytest.mark.parametrize("case", sorted(BACKWARD))
def test_backward_against_the_checker(case):
    from fresnel_amd import surface
    H, W, kind, Hp, Wp, _ = BACKWARD[case]
    depth, color, mods, overrides, up, g64, g32, clouds = _backward_case(case)
    dev = _dev()
    state = _count([depth], [color], overrides, dev)
    m = torch.from_numpy(mods).to(dev)
    out = _emit_guided(state, mods, dev)
    assert np.array_equal(out["point_rows"].cpu().numpy()[0], clouds[0]["point_rows"])
    gpu_up = {k: torch.from_numpy(up[k]).to(dev) for k in GRAD_KEYS}
    for combo in GRAD_COMBOS:
        kw = {"g_" + k: gpu_up[k] for k in GRAD_KEYS if combo in ("all", k)}      # the others: None -> NULL
        got = surface.guided_backward(state, m, out["point_rows"], **kw)
        torch.cuda.synchronize()
        assert got.shape == m.shape
        _judge_grad(f"{case} {combo}", got.cpu().numpy(), g64[combo], g32[combo])
        if case == "64x64_sub3_empty_patches" and combo == "all":
            empty = np.abs(g64["all"][0]).max(axis=0) == 0
            assert not got.cpu().numpy()[0][:, empty].any(), "an empty patch must get exact zeros"
    # the autograd path hands the same call the same gradients
    m2 = m.clone().requires_grad_(True)
    o2 = surface.emit_guided(state, m2)
    sum((gpu_up[k] * o2[k]).sum() for k in GRAD_KEYS).backward()
    want = surface.guided_backward(state, m, out["point_rows"], **{"g_" + k: gpu_up[k] for k in GRAD_KEYS})
    assert torch.equal(m2.grad.view(torch.int32), want.view(torch.int32))


# ---- 5. a batch equals its single images, and repeats ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Hp, Wp", [(5, 5), (1, 1)], ids=["5x5", "1x1_split"])
def test_batch_equals_single_calls_and_repeats(Hp, Wp):
    from fresnel_amd import surface
    dev = _dev()
    items = [_inputs(37, 53, 48), (_depth(37, 53, 0, "constant"), _color(37, 53, 9)), _inputs(37, 53, 50)]
    mods = _random_mods(3, Hp, Wp, 33)

    whole = _count([d for d, _ in items], [c for _, c in items], {}, dev)
    surface.emit(whole)
    up = _upstream(whole.offsets_host[-1], 5)                           # one set of upstream gradients; a single image takes its rows

    def run(depths, colors, mm, lo_hi=None):
        state = _count(depths, colors, {}, dev)
        out = _emit_guided(state, mm, dev)
        sl = slice(0, state.offsets_host[-1]) if lo_hi is None else slice(*lo_hi)
        g = surface.guided_backward(state, torch.from_numpy(mm).to(dev), out["point_rows"],
                                    **{"g_" + k: torch.from_numpy(np.ascontiguousarray(up[k][sl])).to(dev) for k in GRAD_KEYS})
        torch.cuda.synchronize()
        return state.offsets_host, {k: out[k].cpu() for k in KEYS + ("point_rows",)}, g.cpu()

    off, out, g = run([d for d, _ in items], [c for _, c in items], mods)
    assert off[1] == off[2] and off[-1] == whole.offsets_host[-1] > 0
    off2, out2, g2 = run([d for d, _ in items], [c for _, c in items], mods)
    assert off2 == off and torch.equal(g2.view(torch.int32), g.view(torch.int32)), "two runs differ"
    for k in KEYS:
        assert torch.equal(out2[k].view(torch.int32), out[k].view(torch.int32)), f"{k}: two runs differ"
    assert not g[1].any(), "the constant image emits nothing: its maps get exact zeros"
    for b, (d, c) in enumerate(items):
        o1, out1, g1 = run([d], [c], mods[b:b + 1], (off[b], off[b + 1]))
        assert o1 == [0, off[b + 1] - off[b]]
        for k in KEYS:
            assert torch.equal(out1[k].view(torch.int32), out[k][off[b]:off[b + 1]].view(torch.int32)), f"image {b} {k}: batch != single"
        rows = out["point_rows"][b]
        assert torch.equal(out1["point_rows"][0], torch.where(rows >= 0, rows - off[b], rows))
        assert torch.equal(g1[0].view(torch.int32), g[b].view(torch.int32)), f"image {b}: the batch's gradient is not the single call's"


# ---- 6. buffer hygiene and validation -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Hp, Wp, sub", [(5, 7, 3), (1, 1, 1)], ids=["5x7_sub3", "1x1_split"])
def test_guided_buffers(Hp, Wp, sub):
    """Guard bytes and the three fill patterns around every caller-owned buffer of the three entry points: the five outputs and
    point_rows of the emit, g_mods and (when a patch is split) the backward's scratch; inputs and the count's scratch untouched by the
    backward; every element of point_rows and g_mods written."""
    from fresnel_amd import surface
    dev = _dev()
    items = [_inputs(37, 53, 48), (_depth(37, 53, 0, "constant"), _color(37, 53, 9)), _inputs(37, 53, 50)]
    params = _params(dict(subsample=sub, wrap_layers=4))
    probe = surface.count(torch.from_numpy(np.stack([d for d, _ in items])).to(dev), None, params)
    total = int(probe.offsets.cpu()[-1])
    up = _upstream(total, 5)
    inp = dict(depth=torch.from_numpy(np.stack([d for d, _ in items])).to(dev),
               image=torch.from_numpy(np.stack([c for _, c in items])).to(dev),
               mods=torch.from_numpy(_random_mods(3, Hp, Wp, 3)).to(dev), **{"g_" + k: torch.from_numpy(up[k]).to(dev) for k in GRAD_KEYS})
    n_bwd = ctypes_bytes(probe, Hp, Wp)
    assert (n_bwd > 0) == (Hp * Wp == 1), "the 1 x 1 case must take the split-and-fold path, the other must not"

    def fn(guard):
        state = surface.count(inp["depth"], inp["image"], params)
        torch.cuda.synchronize()
        guard.check("after the count")
        n0 = len(guard.records) if isinstance(guard, WG.WorkspaceGuard) else 0
        out = surface.emit_guided(state, inp["mods"])
        torch.cuda.synchronize()
        if isinstance(guard, WG.WorkspaceGuard):
            assert len(guard.records) == n0 + 6, "the five outputs and point_rows must come from the guarded allocator"
        guard.check("after the guided emit")
        scratch = state.scratch.clone()
        g_mods = surface.guided_backward(state, inp["mods"], out["point_rows"], **{k: inp[k] for k in inp if k.startswith("g_")})
        torch.cuda.synchronize()
        if isinstance(guard, WG.WorkspaceGuard):
            assert len(guard.records) == n0 + 6 + 1 + (1 if n_bwd else 0), "g_mods (and the backward's scratch) must be guarded"
        guard.check("after the backward")
        assert torch.equal(state.scratch, scratch), "the backward modified the count's scratch"
        return dict(out, g_mods=g_mods, offsets=state.offsets)

    runs = WG.run_patterns(fn, inp, [surface])
    zero = runs["zero"]
    assert zero["positions"].shape[0] == total > 0 and bool(torch.isfinite(zero["g_mods"]).all())
    assert bool((zero["point_rows"] >= -1).all()) and bool((zero["point_rows"] < total).all())


def ctypes_bytes(state, Hp, Wp):
    import ctypes
    from fresnel_amd import _binding as B
    n = ctypes.c_size_t(12345)
    B.check(B.load().fgs_surface_guided_backward_bytes(ctypes.byref(state.dims), ctypes.byref(state.cparams), Hp, Wp, ctypes.byref(n)), "bytes")
    return n.value


@gpu
def test_capacity_below_the_total_writes_nothing():
    from fresnel_amd import _binding as B
    from fresnel_amd import surface
    dev = _dev()
    depth, color = _inputs(37, 53, 48)
    state = _count([depth], [color], {}, dev)
    mods = torch.from_numpy(_random_mods(1, 5, 5, 3)).to(dev)
    good = _emit_guided(state, mods.cpu().numpy(), dev)
    total = state.offsets_host[-1]
    assert total > 0 and state.status() == 0
    outs = {k: torch.full_like(good[k][:total - 1], -123.0) for k in KEYS}
    rows = torch.full_like(good["point_rows"], -77)
    surface.emit_guided_raw(state, mods, outs, rows, total - 1)          # the C entry itself: the kernel refuses, and says so
    torch.cuda.synchronize()
    assert state.status() == 1
    assert all(bool((outs[k] == -123.0).all()) for k in KEYS) and bool((rows == -77).all())
    with pytest.raises(B.FgsError, match="capacity"):
        surface._emit_guided_detached(state, mods, capacity=total - 1)
    again = _emit_guided(state, mods.cpu().numpy(), dev)                  # the state is intact
    assert state.status() == 0
    for k in KEYS:
        assert torch.equal(again[k], good[k])


@gpu
def test_guided_entries_validate_their_arguments():
    """FGS_EINVAL with a message, before anything touches the device: the guide's shape, its 2^31 bounds, null mods / point_rows."""
    import ctypes
    from fresnel_amd import _binding as B
    from fresnel_amd import surface
    dev = _dev()
    depth, color = _inputs(37, 53, 48)
    state = _count([depth], [color], {}, dev)
    lib = B.load()
    EINVAL = -1                                                          # FGS_EINVAL (include/fgs.h)

    def last_error():
        return lib.fgs_last_error().decode()

    dims, cp = ctypes.byref(state.dims), ctypes.byref(state.cparams)
    n = ctypes.c_size_t(0)
    for hp, wp in ((0, 5), (5, 0), (-1, 5), (5, 2 ** 31 // 53 + 1), (2 ** 31 // 37 + 1, 5), (40000, 40000)):
        assert lib.fgs_surface_guided_backward_bytes(dims, cp, hp, wp, ctypes.byref(n)) == EINVAL, (hp, wp)
        assert "guide" in last_error()
    assert lib.fgs_surface_guided_backward_bytes(dims, cp, 5, 5, None) == EINVAL
    assert lib.fgs_surface_guided_backward_bytes(dims, cp, 37, 37, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.fgs_surface_guided_backward_bytes(dims, cp, 1, 1, ctypes.byref(n)) == 0 and n.value == 8 * 6 * 4   # 1 961 points: 8 waves
    mods = torch.from_numpy(_random_mods(1, 5, 5, 3)).to(dev)
    out = _emit_guided(state, mods.cpu().numpy(), dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    outs = [p(out[k]) for k in KEYS]
    args = [dims, cp, p(state.depth), p(state.color), p(state.scratch), p(state.offsets)]
    total = state.offsets_host[-1]
    assert lib.fgs_surface_emit_guided(*args, None, 5, 5, *outs, p(out["point_rows"]), total, None) == EINVAL
    assert "null" in last_error()
    assert lib.fgs_surface_emit_guided(*args, p(mods), 5, 5, *outs, None, total, None) == EINVAL
    assert lib.fgs_surface_emit_guided(*args, p(mods), 0, 5, *outs, p(out["point_rows"]), total, None) == EINVAL
    assert lib.fgs_surface_emit_guided(*args, p(mods), 5, 5, *outs, p(out["point_rows"]), -1, None) == EINVAL
    g = torch.empty_like(mods)
    bargs = [dims, cp, p(state.depth), p(state.scratch), p(state.offsets)]
    assert lib.fgs_surface_guided_backward(*bargs, p(mods), 5, 5, p(out["point_rows"]), None, None, None, None, None, None, None) == EINVAL
    assert lib.fgs_surface_guided_backward(*bargs, None, 5, 5, p(out["point_rows"]), None, None, None, None, p(g), None, None) == EINVAL
    assert lib.fgs_surface_guided_backward(*bargs, p(mods), 5, 5, None, None, None, None, None, p(g), None, None) == EINVAL
    one = torch.from_numpy(_random_mods(1, 1, 1, 3)).to(dev)             # a split patch needs its scratch
    assert lib.fgs_surface_guided_backward(*bargs, p(one), 1, 1, p(out["point_rows"]), None, None, None, None, p(g), None, None) == EINVAL
    with pytest.raises(B.FgsError):
        surface.emit_guided(state, torch.zeros(2, 6, 5, 5, device=dev))   # the batch of the maps is not the depth's
    with pytest.raises(B.FgsError):
        surface.emit_guided(state, torch.zeros(1, 6, 5, 5))              # CPU maps: no fallback
    with pytest.raises(B.FgsError):
        surface.guided_surface_gaussians(torch.tensor(depth, device=dev).requires_grad_(True), None, mods)


# ---- 7. end to end through autograd ---------------------------------------------------------------------------------------------------------
def _e2e_pipeline_checker(state_dict, features, depths, colors, weights, dtype):
    from fresnel_amd.decoder import FeatureGuidedSAAG
    model = FeatureGuidedSAAG(feature_dim=8, hidden_dim=4).to(dtype)
    model.load_state_dict({k: v.to(dtype) for k, v in state_dict.items()}, strict=True)
    maps = model(features.to(dtype))
    mods = torch.stack([maps[k] for k in G.MOD_KEYS], dim=1)
    clouds = G.guided_clouds(depths, colors, mods, dtype=dtype)
    loss, lo = 0.0, 0
    for c in clouds:
        n = c["positions"].shape[0]
        loss = loss + sum((torch.from_numpy(weights[k][lo:lo + n]).to(dtype) * c[k]).sum() for k in GRAD_KEYS)
        lo += n
    loss.backward()
    return {k: p.grad.double().numpy() for k, p in model.named_parameters()}


@gpu
def test_end_to_end_parameter_gradients():
    """FeatureGuidedSAAG (non-zero last layer) -> guided_surface_gaussians -> a seeded linear functional: the parameter gradients are
    those of the same pipeline through the checker."""
    from fresnel_amd import surface
    from fresnel_amd.decoder import FeatureGuidedSAAG
    dev = _dev()
    torch.manual_seed(3)
    model = FeatureGuidedSAAG(feature_dim=8, hidden_dim=4)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.randn(p.shape) * 0.6)
    features = torch.randn(2, 8, 5, 7)
    raw = np.stack([_depth(40, 48, 48), _depth(40, 48, 3, "checker")])     # depths in [0, 1] before the curve
    colors = np.stack([_color(40, 48, 1), _color(40, 48, 2)])
    d_gpu = torch.from_numpy(raw).to(dev)
    curved = d_gpu.float().pow(0.7).cpu().numpy()                        # the bits surface_gaussians feeds the kernels
    state_dict = {k: v.detach().clone() for k, v in model.state_dict().items()}
    gm = FeatureGuidedSAAG(feature_dim=8, hidden_dim=4).to(dev)
    gm.load_state_dict(state_dict, strict=True)
    clouds = surface.guided_surface_gaussians(d_gpu, torch.from_numpy(colors).to(dev), gm(features.to(dev)))
    total = sum(c["positions"].shape[0] for c in clouds)
    assert len(clouds) == 2 and total > 2000
    weights = _upstream(total, 9)
    loss, lo = 0.0, 0
    for c in clouds:
        n = c["positions"].shape[0]
        loss = loss + sum((torch.from_numpy(weights[k][lo:lo + n]).to(dev) * c[k]).sum() for k in GRAD_KEYS)
        lo += n
    loss.backward()
    torch.cuda.synchronize()
    g64 = _e2e_pipeline_checker(state_dict, features, curved, colors, weights, torch.float64)
    g32 = _e2e_pipeline_checker(state_dict, features, curved, colors, weights, torch.float32)
    for name, p in gm.named_parameters():
        assert np.abs(g64[name]).max() > 0
        _judge_grad(f"e2e {name}", p.grad.cpu().numpy(), g64[name], g32[name])


# ---- 8. a training step ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_two_training_steps_of_experiment_3():
    """--experiment 3 --decoder guided_saag at 64 x 64, subsample 2, B = 2, synthetic data: the loss is finite; after the first step
    net.2.weight has a gradient and all six channels of net.2.bias have one (the reference's step gives four of them none); after
    the second step every parameter has moved."""
    from fresnel_amd import train
    from fresnel_amd.decoder import FeatureGuidedSAAG
    from fresnel_amd.dist import DPContext
    from fresnel_amd.renderer import TileBasedRenderer
    dev = _dev()
    a = train.arg_parser().parse_args(["--experiment", "3", "--decoder", "guided_saag", "--image_size", "64", "--surface_subsample", "2",
                                       "--batch_size", "2", "--lr", "2e-3"])
    cfg = train.config_from_args(a)
    cfg.device, cfg.feature_size, cfg.feature_dim = "cuda:0", 6, 16
    torch.manual_seed(0)
    model = train.make_decoder(cfg).to(dev).train()
    assert isinstance(model, FeatureGuidedSAAG)
    renderer, camera = train.default_renderer_factory(cfg, dev, 64)
    assert isinstance(renderer, TileBasedRenderer)
    opt = train.make_optimizer(model, cfg)
    dp = DPContext(device=dev)
    data = train.SyntheticDataset(4, cfg)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    res = train.train_step(model, renderer, camera, data.batch([0, 1], dev), opt, cfg, dp)
    ld = res.to_host()
    assert ld is not None and math.isfinite(ld["total"]) and math.isfinite(ld["rgb"])
    gw, gb = model.net[2].weight.grad, model.net[2].bias.grad
    print("net.2.bias.grad after the first step:", gb.tolist())
    assert gw is not None and bool(gw.any()) and bool(torch.isfinite(gw).all())
    assert gb.shape == (6,) and bool((gb != 0).all()), f"a channel without a gradient: {gb.tolist()}"
    res = train.train_step(model, renderer, camera, data.batch([2, 3], dev), opt, cfg, dp)
    ld = res.to_host()
    assert ld is not None and math.isfinite(ld["total"])
    for k, p in model.named_parameters():
        assert not torch.equal(p.detach(), before[k]), f"{k} did not move in two steps"
