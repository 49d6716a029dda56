"""The fused HIP head of the distillation decoders (csrc/fgs_slat.hip; fresnel_amd.slat slat_gaussian_head and the decoders with
head_backend "hip") on the GPU: the reference's fixtures S1-S4 (raw in, and through the mirrors), random parity with the restated
head (tests/slat_checker.py) in fp32 and fp64 at the tile and fold seams, the gate / norm / coordinate / NaN seams, the gated
compaction, bitwise repeatability, one captured forward + backward whose replay follows gains changed in place, and a distillation
step with both backends on "hip" against the all-"torch" step.

Judging: every column group (position, scale, rotation, colour, opacity) on its own, within 1e-4 of the group's maximum; where the
checker's own fp32 run is more than 5e-5 from its fp64 run the fp64 run referees (helpers.assert_with_referee)."""
import numpy as np
import pytest
import torch

import slat_checker as sc
from helpers import assert_with_referee, rel_to_max
from test_slat_mirror import (FIXTURES, assert_matches_fixture, assert_matches_gated_fixture, build_mirror, fixture, matching_loss_of,
                              run_gated, run_mirror)

gpu = pytest.mark.gpu
TOL = 1e-4
HB, FOLD_THREADS = 256, 256   # csrc/fgs_slat.hip: rows per block of k_slat_fwd / k_slat_bwd; partials one pass of k_slat_fold takes
GAINS = [(p, s) for p in (0.5, 0.0, -0.7, 2.0) for s in (0.01, 0.0, -0.3)]


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _case(Bn, N, G, seed, spread=4.0):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(Bn, N, G, 14, generator=g) * spread   # a good share beyond +-10, most of it inside
    coords = torch.randint(-4, 70, (Bn, N, 4), generator=g)
    return raw, coords, torch.randn(Bn, N * G, 14, generator=g)


def _hip(raw, coords, gains, up, dev, coords_dtype=None):
    """-> out, dL/d raw, dL/d position_offset_scale, dL/d scale_factor (CPU) of the hip backend."""
    from fresnel_amd.slat import slat_gaussian_head
    r = raw.detach().to(dev).requires_grad_(True)
    pg, sf = (torch.tensor(float(v), device=dev, requires_grad=True) for v in gains)
    c = coords.to(dev) if coords_dtype is None else coords.to(dev, coords_dtype)
    out = slat_gaussian_head(r, c, pg, sf, backend="hip")
    (out * up.to(dev)).sum().backward()
    torch.cuda.synchronize()
    return out.detach().cpu(), r.grad.cpu(), pg.grad.cpu(), sf.grad.cpu()


def _checker(raw, coords, gains, up, dtype, **kw):
    r = raw.detach().to(dtype, copy=True).requires_grad_(True)   # an own leaf
    pg, sf = (torch.tensor(float(v), dtype=dtype, requires_grad=True) for v in gains)
    out = sc.head(r, coords, pg, sf, **kw)
    (out * up.to(dtype)).sum().backward()
    return out.detach(), r.grad, pg.grad, sf.grad


def _compare(tag, got, w32, w64):
    for i, name in ((0, "out"), (1, "grad raw")):
        a, b, c = (t[i].reshape(-1, 14).numpy() for t in (got, w32, w64))
        for group, cols in sc.GROUPS.items():
            assert_with_referee(a[:, cols], b[:, cols], c[:, cols], f"{tag}: {name} {group}")
    for i, name in ((2, "grad position_offset_scale"), (3, "grad scale_factor")):
        assert_with_referee(got[i].numpy(), w32[i].numpy(), w64[i].numpy(), f"{tag}: {name}")
    norms = got[0][..., 6:10].norm(dim=-1)
    assert float((norms - 1).abs().max()) <= 1e-5, f"{tag}: quaternion norms"


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_raw_through_the_hip_head(name):
    dev = _dev()
    fx = fixture(name)
    raw, coords, up = (torch.from_numpy(fx[k]) for k in ("raw", "in.coords", "g.gaussians"))
    gains = (float(fx["sd.gaussian_head.position_offset_scale"]), float(fx["sd.gaussian_head.scale_factor"]))
    out, g_raw, g_pg, g_sf = _hip(raw, coords, gains, up, dev)
    for group, cols in sc.GROUPS.items():
        e = rel_to_max(out.numpy()[..., cols], fx["out.gaussians"][..., cols])
        assert e <= TOL, f"{name}: {group} is {e:.2e} of its maximum away"
        e = rel_to_max(g_raw.numpy()[..., cols], fx["grad.raw"][..., cols])
        assert e <= TOL, f"{name}: grad raw {group} is {e:.2e} of its maximum away"
    assert rel_to_max(g_pg.numpy(), fx["grad.sd.gaussian_head.position_offset_scale"]) <= TOL
    assert rel_to_max(g_sf.numpy(), fx["grad.sd.gaussian_head.scale_factor"]) <= TOL
    assert float((out[..., 6:10].norm(dim=-1) - 1).abs().max()) <= 1e-5


@gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_module_with_hip_head_reproduces_the_fixture(name):
    dev = _dev()
    fx = fixture(name)
    out, grads, raw = run_mirror(build_mirror(fx, head_backend="hip", device=dev)[0], fx, dev)
    torch.cuda.synchronize()
    assert_matches_fixture(fx, out, grads, raw, name + " (hip)")


@gpu
def test_gated_inference_with_hip_head_reproduces_the_lists():
    dev = _dev()
    fx = fixture("slat_S2")
    out = run_gated(build_mirror(fx, head_backend="hip", device=dev)[0], fx, dev)
    assert_matches_gated_fixture(fx, out, "slat_S2 (hip)")
    base = out["gaussians"][0]._base if out["gaussians"][0]._base is not None else out["gaussians"][0]
    assert all((g._base if g._base is not None else g).data_ptr() == base.data_ptr() for g in out["gaussians"])   # views of one tensor


# ---- random parity -------------------------------------------------------------------------------------------------------------------
def _tile_seam_n(G):
    n = HB // G
    return [n - 1, n, n + 1]   # N x G one below / on / one above 256 (G 1), or straddling it as closely as whole voxels allow


@gpu
@pytest.mark.parametrize("Bn", [1, 3])
@pytest.mark.parametrize("G", [1, 3, 8, 32])
def test_random_parity_with_the_checker(Bn, G):
    dev = _dev()
    sizes = [1] + _tile_seam_n(G) + [1030]
    for k, N in enumerate(sizes):
        gains = GAINS[(k + 5 * [1, 3, 8, 32].index(G) + 3 * Bn) % len(GAINS)]
        raw, coords, up = _case(Bn, N, G, 1000 + 37 * G + N)
        got = _hip(raw, coords, gains, up, dev)
        _compare(f"B{Bn} N{N} G{G} gains {gains}", got, _checker(raw, coords, gains, up, torch.float32),
                 _checker(raw, coords, gains, up, torch.float64))


@gpu
@pytest.mark.parametrize("gains", GAINS, ids=[f"pos{p}_scale{s}" for p, s in GAINS])
def test_every_pair_of_gains(gains):
    dev = _dev()
    raw, coords, up = _case(3, 33, 8, 1100)
    got = _hip(raw, coords, gains, up, dev)
    _compare(f"gains {gains}", got, _checker(raw, coords, gains, up, torch.float32), _checker(raw, coords, gains, up, torch.float64))
    if gains[1] == 0.0:   # |0| has gradient 0; every scale sits on its lower clamp
        assert float(got[3]) == 0.0 and bool((got[0][..., 3:6] == 1e-4).all()) and not got[1][..., 3:6].any()
    if gains[0] == 0.0:
        assert not got[1][..., 0:3].any()


@gpu
@pytest.mark.parametrize("blocks", [FOLD_THREADS - 1, FOLD_THREADS, FOLD_THREADS + 1])
def test_fold_seam_of_the_gain_gradients(blocks):
    """G 32: 8 voxels fill a block of 256 rows.  255 / 256 / 257 block partials: one pass of k_slat_fold short, full, and one over."""
    dev = _dev()
    N = (blocks - 1) * 8 + 1 if blocks == FOLD_THREADS + 1 else blocks * 8
    assert (N * 32 + HB - 1) // HB == blocks
    raw, coords, up = _case(1, N, 32, 1200 + blocks)
    up[0, -1, :6] = 50.0   # the last row carries weight, behind open gates: a fold that drops its tail misses it
    raw[0, -1, -1, :6], coords[0, -1, 1:] = 0.3, 32
    gains = (0.5, -0.3)
    got = _hip(raw, coords, gains, up, dev)
    _compare(f"{blocks} partials", got, _checker(raw, coords, gains, up, torch.float32), _checker(raw, coords, gains, up, torch.float64))


# ---- seams -------------------------------------------------------------------------------------------------------------------------
@gpu
def test_raw_on_and_one_ulp_outside_the_gate():
    dev = _dev()
    ten = torch.tensor(10.0)
    above, below = torch.nextafter(ten, torch.tensor(float("inf"))), torch.nextafter(-ten, torch.tensor(float("-inf")))
    raw = torch.zeros(1, 4, 1, 14)
    raw[0, 0], raw[0, 1], raw[0, 2], raw[0, 3] = 10.0, -10.0, above, below
    raw[..., :3] = 0.3   # (tanh'(10) is below fp32's reach: the position channels cannot show the gate)
    coords = torch.full((1, 4, 4), 32)
    up = torch.ones(1, 4, 14)
    up[..., 6:10] = torch.tensor([1.0, -2.0, 3.0, -4.0])   # not along q: the normalisation lets it through
    gains = (0.5, 0.05)
    got = _hip(raw, coords, gains, up, dev)
    w32, w64 = _checker(raw, coords, gains, up, torch.float32), _checker(raw, coords, gains, up, torch.float64)
    _compare("gate", got, w32, w64)
    g = got[1][0, :, 0]
    assert bool((g[0, 6:] != 0).all()) and bool((g[1, 6:] != 0).all()), "the closed gate passes the gradient AT +-10"
    assert not g[2, 3:].any() and not g[3, 3:].any(), "one ulp outside: no gradient"
    assert torch.equal(got[0][0, 0], got[0][0, 2]) and torch.equal(got[0][0, 1], got[0][0, 3])   # the forward clamps


@gpu
def test_quaternion_norm_floor():
    dev = _dev()
    raw, coords, up = _case(1, 6, 1, 1300)
    raw[0, 0, 0, 6:10] = 0.0                                   # all zero: output 0, gradient g 1e6
    raw[0, 1, 0, 6:10] = torch.tensor([3e-7, -2e-7, 1e-7, 0])  # norm 3.7e-7 < 1e-6: q / 1e-6, gradient g / 1e-6
    gains = (0.5, 0.01)
    got = _hip(raw, coords, gains, up, dev)
    assert not got[0][0, 0, 6:10].any()
    assert torch.allclose(got[1][0, 0, 0, 6:10], up[0, 0, 6:10] * 1e6, rtol=1e-6)
    assert torch.allclose(got[0][0, 1, 6:10], raw[0, 1, 0, 6:10] * 1e6, rtol=1e-6)
    assert torch.allclose(got[1][0, 1, 0, 6:10], up[0, 1, 6:10] * 1e6, rtol=1e-6)
    w64 = _checker(raw, coords, gains, up, torch.float64)
    for i in (0, 1):
        assert rel_to_max(got[1][0, i, 0, 6:10].numpy(), w64[1][0, i, 0, 6:10].numpy()) <= TOL, i
    others = torch.tensor([2, 3, 4, 5])
    assert float((got[0][0, others, 6:10].norm(dim=-1) - 1).abs().max()) <= 1e-5


@gpu
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.float32], ids=["int32", "int64", "float"])
def test_coordinates_beyond_the_grid_in_every_dtype(dtype):
    dev = _dev()
    raw, coords, up = _case(2, 9, 3, 1310)
    coords[0, 0, 1:], coords[0, 1, 1:], coords[1, 2, 1:] = torch.tensor([-1, 0, 64]), torch.tensor([63, -500, 1000]), torch.tensor([2 ** 20, 5, -7])
    if dtype is torch.int64:
        coords[1, 3, 1:] = torch.tensor([2 ** 40, -2 ** 40, 2 ** 32 + 5])   # beyond int32: clamped before the cast, never wrapped
    gains = (0.05, 0.3)   # small offsets: the centres show
    got = _hip(raw, coords, gains, up, dev, coords_dtype=dtype)
    _compare(f"coords {dtype}", got, _checker(raw, coords, gains, up, torch.float32), _checker(raw, coords, gains, up, torch.float64))


@gpu
def test_fractional_float_coordinates_are_truncated_on_hip():
    """The documented difference: the C ABI takes int32 coordinates, so the hip backend truncates a fractional float coordinate towards
    zero (as the positional encoding does on both backends) where the torch backend, like the reference's head, keeps the fraction."""
    from fresnel_amd.slat import slat_gaussian_head
    dev = _dev()
    raw, coords, up = _case(2, 9, 3, 1315)
    whole = coords.clamp(3, 60).float()   # away from both ends: with offsets of 0.05 no position meets its clamp
    frac = whole.clone()
    frac[..., 1:] += 0.7                       # 3.7 -> 3; the largest, 60.7 -> 60
    frac[0, 0, 1:] = torch.tensor([-0.7, 63.9, 64.2])   # -> 0 (towards zero), 63, clamp to 63
    whole[0, 0, 1:] = torch.tensor([0.0, 63.0, 63.0])
    gains = (0.05, 0.3)
    a, b = _hip(raw, frac, gains, up, dev), _hip(raw, whole, gains, up, dev)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    with torch.no_grad():
        kept = slat_gaussian_head(raw.to(dev), frac.to(dev), torch.tensor(0.05, device=dev), torch.tensor(0.3, device=dev)).cpu()
    shift = (kept - a[0])[..., :3].reshape(2, 9, 3, 3)[:, 1:]   # torch keeps the 0.7: centres 0.7 / 32 further out (small offsets, no clamp)
    assert float((shift - 0.7 / 32).abs().max()) <= 1e-5


@gpu
def test_nan_and_inf_follow_the_stated_rule():
    from fresnel_amd.slat import slat_gaussian_head
    dev = _dev()
    raw, coords, up = _case(2, 40, 3, 1320)
    clean = raw.clone()
    nan, inf = float("nan"), float("inf")
    raw[0, 3, 1, 1] = nan        # one position component
    raw[0, 7, 0, 8] = nan        # one quaternion component
    raw[1, 20, 2, 13] = nan      # opacity
    raw[1, 5, 0, 0], raw[1, 5, 0, 4], raw[1, 5, 0, 12] = inf, -inf, inf
    raw[1, 6, 1, 7] = -inf
    gains = (0.5, -0.3)
    got = _hip(raw, coords, gains, up, dev)
    # the forward equals the torch backend's (the reference's nan_to_num), NaN places exactly 0
    with torch.no_grad():
        want = slat_gaussian_head(raw.to(dev), coords.to(dev), torch.tensor(0.5, device=dev), torch.tensor(-0.3, device=dev)).cpu()
    assert not bool(torch.isnan(want).any())
    out = got[0].reshape(2, 40, 3, 14)
    assert float((got[0] - want).abs().max()) <= 1e-6
    assert float(out[0, 3, 1, 1]) == 0.0 and not out[0, 7, 0, 6:10].any() and float(out[1, 20, 2, 13]) == 0.0
    # gradients: finite everywhere, zero exactly where the rule says (and behind the +-Inf, which sit outside the gate)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    g = got[1]
    assert float(g[0, 3, 1, 1]) == 0.0 and not g[0, 7, 0, 6:10].any() and float(g[1, 20, 2, 13]) == 0.0
    assert float(g[1, 5, 0, 0]) == 0.0 and float(g[1, 5, 0, 4]) == 0.0 and float(g[1, 5, 0, 12]) == 0.0 and float(g[1, 6, 1, 7]) == 0.0
    # every other element is the clean run's, bit for bit (the quaternion of the -Inf row changes as a whole: compare it by value)
    ref = _hip(clean, coords, gains, up, dev)
    touched = torch.zeros_like(raw, dtype=torch.bool)
    touched[0, 3, 1, 1] = touched[1, 20, 2, 13] = touched[1, 5, 0, 0] = touched[1, 5, 0, 4] = touched[1, 5, 0, 12] = True
    touched[0, 7, 0, 6:10] = touched[1, 6, 1, 6:10] = True
    assert torch.equal(out[~touched], ref[0].reshape(raw.shape)[~touched]) and torch.equal(g[~touched], ref[1][~touched])
    # against the checker under the same rule, gains included
    w32, w64 = (_checker(raw, coords, gains, up, d, nan_rule=True) for d in (torch.float32, torch.float64))
    for i, name in ((2, "grad position_offset_scale"), (3, "grad scale_factor")):
        assert_with_referee(got[i].numpy(), w32[i].numpy(), w64[i].numpy(), f"nan: {name}")
    assert rel_to_max(g.numpy(), w64[1].numpy()) <= TOL


# ---- gated -------------------------------------------------------------------------------------------------------------------------
PATTERNS = ("none", "all", "alternating", "last", "empty_beside_full")


def _keep(pattern, N):
    keep = torch.zeros(2, N, dtype=torch.bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "alternating":
        keep[0, ::2], keep[1, 1::2] = True, True
    elif pattern == "last":
        keep[:, -1] = True
    elif pattern == "empty_beside_full":
        keep[1] = True
    return keep


@gpu
@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
def test_gated_forward_compacts_kept_voxels(N):
    from fresnel_amd.slat import slat_gaussian_head
    dev = _dev()
    G = 3
    raw, coords, _ = _case(2, N, G, 1400 + N)
    r, c = raw.to(dev), coords.to(dev)
    pg, sf = torch.tensor(0.5, device=dev), torch.tensor(-0.3, device=dev)
    full = slat_gaussian_head(r, c, pg, sf, backend="hip").reshape(2, N, G, 14)
    for pattern in PATTERNS:
        keep = _keep(pattern, N).to(dev)
        packed, counts = slat_gaussian_head(r, c, pg, sf, keep=keep, backend="hip")
        torch.cuda.synchronize()
        assert counts.dtype == torch.int32 and counts.tolist() == keep.sum(dim=1).tolist(), pattern
        assert tuple(packed.shape) == (2, N * G, 14)
        for b in range(2):
            n = int(counts[b]) * G
            assert torch.equal(packed[b, :n].view(torch.int32), full[b][keep[b]].reshape(n, 14).view(torch.int32)), (pattern, b)
            assert not packed[b, n:].any(), (pattern, b)
    with pytest.raises(ValueError, match="no gradient for raw"):
        slat_gaussian_head(r.clone().requires_grad_(True), c, pg, sf, keep=keep, backend="hip")
    with pytest.raises(ValueError, match="no gradient for position_offset_scale"):
        slat_gaussian_head(r, c, pg.clone().requires_grad_(True), sf, keep=keep, backend="hip")


# ---- repeatability -----------------------------------------------------------------------------------------------------------------
@gpu
def test_two_calls_and_batch_against_single_images_are_bit_identical():
    dev = _dev()
    raw, coords, up = _case(3, 1030, 8, 1500)
    gains = (0.5, -0.3)
    a, b = _hip(raw, coords, gains, up, dev), _hip(raw, coords, gains, up, dev)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    for i in range(3):
        one = _hip(raw[i:i + 1], coords[i:i + 1], gains, up[i:i + 1], dev)
        assert torch.equal(one[0].view(torch.int32), a[0][i:i + 1].view(torch.int32)), i
        assert torch.equal(one[1].view(torch.int32), a[1][i:i + 1].view(torch.int32)), i


@gpu
def test_under_autocast_raw_is_cast_to_fp32():
    from fresnel_amd.slat import slat_gaussian_head
    dev = _dev()
    raw, coords, up = _case(2, 33, 3, 1550)
    half = raw.to(dev, torch.bfloat16).requires_grad_(True)
    pg, sf = torch.tensor(0.5, device=dev), torch.tensor(-0.3, device=dev)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = slat_gaussian_head(half, coords.to(dev), pg, sf, backend="hip")
    (out * up.to(dev)).sum().backward()
    full = half.detach().float().requires_grad_(True)
    want = slat_gaussian_head(full, coords.to(dev), pg, sf, backend="hip")
    (want * up.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert out.dtype is torch.float32 and torch.equal(out.view(torch.int32), want.view(torch.int32))
    assert half.grad.dtype is torch.bfloat16 and torch.equal(half.grad, full.grad.to(torch.bfloat16))


# ---- capture -----------------------------------------------------------------------------------------------------------------------
@gpu
def test_captured_graph_follows_gains_changed_in_place():
    from fresnel_amd.slat import slat_gaussian_head
    dev = _dev()
    raw_c, coords_c, up_c = _case(2, 70, 3, 1600)
    raw, pg, sf = raw_c.to(dev).requires_grad_(True), torch.tensor(0.5, device=dev, requires_grad=True), torch.tensor(0.05, device=dev, requires_grad=True)
    coords, up = coords_c.to(dev), up_c.to(dev)
    leaves = (raw, pg, sf)

    def step():
        out = slat_gaussian_head(raw, coords, pg, sf, backend="hip")
        (out * up).sum().backward()
        return out

    def eager(p, s):
        with torch.no_grad():
            pg.fill_(p)
            sf.fill_(s)
        for t in leaves:
            t.grad = None
        out = step()
        torch.cuda.synchronize()
        return [out.detach().clone()] + [t.grad.detach().clone() for t in leaves]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager(0.5, 0.05)
        want_new = eager(-0.2, -0.4)
        eager(0.5, 0.05)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in leaves:
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        pg.fill_(-0.2)
        sf.fill_(-0.4)
        for t in leaves:
            t.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = [captured] + [t.grad for t in leaves]
    for name, a, b in zip(("out", "grad raw", "grad position_offset_scale", "grad scale_factor"), got, want_new):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: the replay does not follow the new gains"
    assert float(want_new[3]) != 0.0 and float(want_new[2]) != 0.0


# ---- a distillation step -----------------------------------------------------------------------------------------------------------
def _distill_setup(dev):
    from fresnel_amd.slat import DirectSLatDecoder
    torch.manual_seed(1700)
    ctor = dict(feature_dim=12, hidden_dim=20, num_layers=2, num_heads=4, num_gaussians_per_voxel=2, dropout=0.0)
    model = DirectSLatDecoder(**ctor)
    with torch.no_grad():   # raw spread of a few units: gates open and closed, as in training after a while
        model.gaussian_head.head[-1].weight.mul_(40.0)
        model.gaussian_head.scale_factor.fill_(0.2)
    g = torch.Generator().manual_seed(1701)
    Bn, N = 2, 16
    coords = torch.randint(0, 64, (Bn, N, 4), generator=g)
    coord_mask = torch.ones(Bn, N, dtype=torch.bool)
    coord_mask[1, -3:] = False
    target = torch.rand(Bn, 64, 14, generator=g)   # continuous draws: no two rows tie
    target[..., :3] = target[..., :3] * 2 - 1
    batch = dict(features=torch.randn(Bn, 5, 12, generator=g), coords=coords, coord_mask=coord_mask, gaussians=target,
                 gaussian_mask=torch.ones(Bn, 64, dtype=torch.bool), occupancy_target=(torch.rand(Bn, N, generator=g) > 0.5).float())
    twin = DirectSLatDecoder(**ctor, head_backend="hip")
    twin.load_state_dict(model.state_dict(), strict=True)
    return model.to(dev).train(), twin.to(dev).train(), {k: v.to(dev) for k, v in batch.items()}


@gpu
def test_distill_step_on_hip_matches_the_torch_step_and_learns():
    from fresnel_amd import distill
    dev = _dev()
    model_t, model_h, batch = _distill_setup(dev)
    cfg_t = distill.DistillConfig()
    cfg_h = distill.DistillConfig(head_backend="hip", match_backend="hip")
    loss_t, loss_h = (matching_loss_of(c, max_match_points=4096) for c in (cfg_t, cfg_h))
    opt_t, opt_h = (torch.optim.AdamW(m.parameters(), lr=2e-3) for m in (model_t, model_h))
    first_t = distill.distill_step(model_t, batch, opt_t, loss_t, cfg_t)
    first_h = distill.distill_step(model_h, batch, opt_h, loss_h, cfg_h)
    torch.cuda.synchronize()
    assert sorted(first_h) == sorted(first_t) and "occupancy" in first_h
    assert abs(float(first_h["total"]) - float(first_t["total"])) <= TOL * abs(float(first_t["total"]))
    for (k, p), q in zip(model_h.named_parameters(), model_t.parameters()):   # the step's gradients (clipped), still on the parameters
        e = rel_to_max(p.grad.cpu().numpy(), q.grad.cpu().numpy())
        print(f"distill step: grad {k} {e:.2e}")
        assert e <= TOL, f"gradient of {k} is {e:.2e} of its maximum away from the all-torch step's"
    # nothing in a hip / hip step reads the host
    torch.cuda.set_sync_debug_mode("error")
    try:
        totals = [distill.distill_step(model_h, batch, opt_h, loss_h, cfg_h)["total"] for _ in range(4)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    totals = [float(first_h["total"])] + [float(t) for t in totals]
    print("distill totals:", totals)
    assert all(np.isfinite(totals)) and totals[-1] < totals[0], totals
