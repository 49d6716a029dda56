"""The fused HIP head of the physics-phase decoder (csrc/fgs_physics.hip; fresnel_amd.decoder physics_head /
PhysicsDirectPatchDecoder with head_backend "hip") on the GPU: the reference's fixtures P1-P3, random parity with the restated head
(tests/physics_checker.py) in fp32 and fp64, the seams of the range and sum stages, known answers, ties of the minimum and maximum,
the wavelength clamp, NaN, absent upstream gradients, bitwise repeatability, one captured forward + backward whose replay follows
an in-place change of the wavelength, and a short training run.

Judging: within 1e-4 of the maximum of the checker's fp32 OR fp64 result, else within twice the checker's own fp32-to-fp64 deviation
of its fp64 result; phases by circular distance and the second form alone."""
import math

import pytest
import torch

import physics_checker as pc
from test_physics_mirror import FIXTURES, assert_matches_fixture, build_mirror, fixture, run_mirror

gpu = pytest.mark.gpu
TOL = 1e-4
# the kernel's constants (csrc/fgs_physics.hip), named here next to the seams they make
RANGE_THREADS, RANGE_BLOCK_ITEMS, RANGE_MAX_BLOCKS = 1024, 16384, 32   # k_phys_range: one block up to 16 384 values, 32 blocks at most
HB, SUM_THREADS = 256, 256                                             # rows per tile of k_phys_bwd; threads of k_phys_sums


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _case(Bn, P, KF, seed, lam=0.05, z=None):
    """Seeded inputs with no Gaussian within 1e-3 of a quaternion-branch boundary (the tests assert the share is 0); upstream gradients
    come from rand: the wavelength gradient is then a sum of terms of one sign."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(Bn, P, KF, 16, generator=g)
    while True:   # no seed leaves 6000 Gaussians all clear of the quaternion-branch boundaries: redraw the rotations of those that are not
        near = _near(raw, KF).reshape(Bn, P, KF)
        if not near.any():
            break
        raw[near] = torch.cat([raw[near][:, :6], torch.randn(int(near.sum()), 6, generator=g), raw[near][:, 12:]], dim=1)
    xy = torch.rand(P, 2, generator=g) * 2 - 1
    z = (-2.0 - 2.0 * torch.rand(Bn, P, generator=g)) if z is None else z
    return dict(raw=raw, xy=xy, z=z, lam=torch.tensor(float(lam)), g=g)


def _ups(Bn, N, g):
    shapes = dict(positions=(Bn, N, 3), scales=(Bn, N, 3), rotations=(Bn, N, 4), colors=(Bn, N, 3), opacities=(Bn, N), phases=(Bn, N))
    return {k: torch.rand(s, generator=g) for k, s in shapes.items()}


def _run(c, ups, K, backend, dev=None, dtype=torch.float32, use=None, **kw):
    """-> outputs, dL/d raw, dL/d base_z, dL/d wavelength_raw (CPU); backend "hip" | "checker"."""
    if backend == "hip":
        from fresnel_amd.decoder import physics_head
        raw, z, lam = (c[k].to(dev).requires_grad_(True) for k in ("raw", "z", "lam"))
        out = physics_head(raw, c["xy"].to(dev), z, lam, num_gaussians=K, backend="hip", **kw)
    else:
        raw, z, lam = (c[k].detach().to(dtype, copy=True).requires_grad_(True) for k in ("raw", "z", "lam"))   # own leaves
        if use == ("phases",):   # the phase alone: the large seam cases need not restate half a million quaternions
            Bn, P = z.shape
            out = dict(phases=pc.phase_of(z, lam, **kw)[:, :, None].expand(Bn, P, K).reshape(Bn, P * K))
        else:
            out = pc.head(raw, c["xy"], z, lam, num_gaussians=K, **kw)
    sum((out[k] * ups[k].to(out[k].device, out[k].dtype)).sum() for k in (use or out)).backward()
    if backend == "hip":
        torch.cuda.synchronize()
    zero = lambda t: (t.grad if t.grad is not None else torch.zeros_like(t)).detach().cpu().clone()   # noqa: E731
    return {k: v.detach().cpu() for k, v in out.items()}, zero(raw), zero(z), zero(lam)


def _near(raw, K):
    branch, trace, gap = pc.branch_info(raw.double()[:, :, :K, 6:12])
    return ((trace.abs() < 1e-3) | ((branch != 0) & (gap < 1e-3))).flatten(1)


def _judge(tag, name, got, w32, w64, circular=False):
    got, w32, w64 = got.double(), w32.double(), w64.double()
    if circular:
        d, dev = float(pc.circular_distance(got, w64).max()), float(pc.circular_distance(w32, w64).max())
        print(f"{tag}: {name} circular {d:.2e} (checker's own {dev:.2e})")
        assert d <= 2 * dev, f"{tag}: {name} is {d:.2e} from the fp64 phases on the circle, the checker's fp32 run {dev:.2e}"
        return
    top = max(float(w64.abs().max()), 1e-30)
    e32, e64, dev = float((got - w32).abs().max()), float((got - w64).abs().max()), float((w32 - w64).abs().max())
    print(f"{tag}: {name} {e32 / top:.2e} / {e64 / top:.2e} of {top:.3e}, checker's own {dev / top:.2e}")
    assert min(e32, e64) <= TOL * top or e64 <= 2 * dev, f"{tag}: {name} is {e32:.3e} / {e64:.3e} away (scale {top:.3e}, referee {dev:.3e})"


def _compare(tag, got, w32, w64):
    for k in pc.OUTPUTS:
        _judge(tag, k, got[0][k], w32[0][k], w64[0][k], circular=(k == "phases"))
    for i, name in ((1, "grad raw"), (2, "grad base_z"), (3, "grad wavelength_raw")):
        _judge(tag, name, got[i], w32[i], w64[i])


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_module_with_hip_head_reproduces_the_fixture(name):
    dev = _dev()
    fx = fixture(name)
    out, grads, g_raw = run_mirror(build_mirror(fx, head_backend="hip", device=dev), fx, dev)
    torch.cuda.synchronize()
    assert_matches_fixture(fx, out, grads, g_raw, name + " (hip)")


# ---- random parity ------------------------------------------------------------------------------------------------------------------
SHAPES = {"b1_p1_k1of1": (1, 1, 1, 1, 700), "b2_p35_k2of3": (2, 35, 3, 2, 701), "b3_p257_k8of8": (3, 257, 8, 8, 702),
          "b1_p1369_k5of8": (1, 1369, 8, 5, 703)}


@gpu
@pytest.mark.parametrize("case", sorted(SHAPES))
def test_random_parity_with_the_checker(case):
    dev = _dev()
    Bn, P, KF, K, seed = SHAPES[case]
    c = _case(Bn, P, KF, seed)
    assert float(_near(c["raw"], K).float().mean()) == 0.0, "choose a seed without a Gaussian near a quaternion-branch boundary"
    ups = _ups(Bn, P * K, c["g"])
    # the wavelength gradient is -(c / lambda) sum G |u - f|: every term has one sign, sum |terms| / |sum terms| = 1 < 10
    terms = ups["phases"].double().reshape(Bn, P, K).sum(-1) * pc.phase_of(c["z"].double(), c["lam"].double(), wrap_rule="none")
    assert float(terms.abs().sum()) / max(abs(float(terms.sum())), 1e-300) < 10 or P == 1
    got = _run(c, ups, K, "hip", dev)
    _compare(case, got, _run(c, ups, K, "checker", dtype=torch.float32), _run(c, ups, K, "checker", dtype=torch.float64))
    assert not got[1][:, :, :, 2].any() and not got[1][:, :, K:].any()   # channel 2 and the unused Gaussians: written zeros


# ---- seams of the range and sum stages -------------------------------------------------------------------------------------------------
def _phase_case(n, seed, KF=1):
    """B x P = n patches of K_full Gaussians with the extremes in the LAST two patches: a stage that drops its tail misses them."""
    c = _case(1, n, KF, seed)
    if n >= 2:
        c["z"][0, -1], c["z"][0, -2] = -7.0, 3.0
    return c


@gpu
@pytest.mark.parametrize("n", [RANGE_THREADS, RANGE_THREADS + 1, RANGE_BLOCK_ITEMS, RANGE_BLOCK_ITEMS + 1,
                               RANGE_MAX_BLOCKS * RANGE_BLOCK_ITEMS, RANGE_MAX_BLOCKS * RANGE_BLOCK_ITEMS + 1,
                               HB * SUM_THREADS, HB * SUM_THREADS + 1])
def test_range_stage_seams(n):
    """One block's threads / one past; the single-block limit / one past (two blocks and the fold); the most values that get a
    block each / one past (the block count stays at its cap); K_full 1 puts 256 patches in a tile: 256 x 256 patches are 256
    partials of k_phys_sums / one past."""
    dev = _dev()
    c = _phase_case(n, 710)
    ups = dict(phases=torch.rand(1, n, generator=c["g"]))
    got = _run(c, ups, 1, "hip", dev, use=("phases",))
    w32, w64 = (_run(c, ups, 1, "checker", dtype=d, use=("phases",)) for d in (torch.float32, torch.float64))
    _judge(f"n={n}", "phases", got[0]["phases"], w32[0]["phases"], w64[0]["phases"], circular=True)
    _judge(f"n={n}", "grad base_z", got[2], w32[2], w64[2])
    _judge(f"n={n}", "grad wavelength_raw", got[3], w32[3], w64[3])


@gpu
@pytest.mark.parametrize("P", [HB // 64 * SUM_THREADS, HB // 64 * SUM_THREADS + 1, 2 * (HB // 64), 2 * (HB // 64) + 1])
def test_sum_stage_seams_with_the_largest_patches(P):
    """K_full 64: four patches per tile.  1024 patches are 256 partials, 1025 one more (a tile of one patch)."""
    dev = _dev()
    c = _phase_case(P, 711, KF=64)
    ups = _ups(1, P * 64, c["g"])
    got = _run(c, ups, 64, "hip", dev, use=("positions", "phases"))
    w32, w64 = (_run(c, ups, 64, "checker", dtype=d, use=("positions", "phases")) for d in (torch.float32, torch.float64))
    _judge(f"P={P}", "grad base_z", got[2], w32[2], w64[2])
    _judge(f"P={P}", "grad wavelength_raw", got[3], w32[3], w64[3])


# ---- known answers --------------------------------------------------------------------------------------------------------------------
@gpu
def test_three_depths_have_their_known_phases():
    """z = -4, -3, -2: u = 0, 1/2, 1; lambda 0.4, f 0.5: phase = (2 pi / 0.4) x (1/2, 0, 1/2) = 2.5 pi -> (pi/2, 0, pi/2); the middle
    element sits on u == f: no phase gradient reaches it."""
    dev = _dev()
    c = _case(1, 3, 1, 720, lam=0.4, z=torch.tensor([[-4.0, -3.0, -2.0]]))
    ups = dict(phases=torch.tensor([[0.3, 0.9, 0.6]]))
    out, _, g_z, g_lam = _run(c, ups, 1, "hip", dev, use=("phases",))
    want = torch.tensor([[math.pi / 2, 0.0, math.pi / 2]])
    assert float(pc.circular_distance(out["phases"], want).max()) <= 1e-5 and float(out["phases"][0, 1]) == 0.0
    # against the checker's fp32 run: in fp64 D keeps its 1e-8, u = 0.4999999975 and the middle element is NOT on u == f
    w = _run(c, ups, 1, "checker", dtype=torch.float32, use=("phases",))
    assert float(w[2][0, 1]) == 0.0
    _judge("known", "grad base_z", g_z, w[2], w[2])
    _judge("known", "grad wavelength_raw", g_lam, w[3], w[3])
    # the middle element: nothing through its own u, and it holds neither extreme
    assert float(g_z[0, 1]) == 0.0


# ---- ties ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("held_by", [1, 2, "all"])
def test_tied_extremes_share_their_gradient_equally(held_by):
    """Minimum and maximum held by 1, by 2 (one in each batch image) and by all elements (z constant: D = 1e-8)."""
    dev = _dev()
    Bn, P, K = 2, 9, 2
    c = _case(Bn, P, K, 730)
    if held_by == "all":
        c["z"][:] = -2.5
    else:
        c["z"][0, 3], c["z"][1, 5] = -6.0, 1.0
        if held_by == 2:
            c["z"][1, 7], c["z"][0, 0] = -6.0, 1.0     # the second holder sits in the other image
    ups = dict(phases=torch.rand(Bn, P * K, generator=c["g"]))
    got = _run(c, ups, K, "hip", dev, use=("phases",))
    w32, w64 = (_run(c, ups, K, "checker", dtype=d, use=("phases",)) for d in (torch.float32, torch.float64))
    _judge(f"ties {held_by}", "grad base_z", got[2], w32[2], w64[2])
    # the shares: dL/d base_z minus its local part g_u / D, from the fp64 checker with the tie gradient switched off by detaching
    z64 = c["z"].detach().double().requires_grad_(True)
    zmin, zmax = z64.detach().min(), z64.detach().max()
    u = (z64 - zmin) / ((zmax - zmin) + 1e-8)
    lam = c["lam"].double()
    ph = (2 * math.pi / lam) * (u - 0.5).abs()
    (ph[:, :, None].expand(Bn, P, K).reshape(Bn, P * K) * ups["phases"].double()).sum().backward()
    local = z64.grad
    shares, want = got[2].double() - local, w64[2] - local
    top = float(w64[2].abs().max())
    lo, hi = (c["z"] == c["z"].min()), (c["z"] == c["z"].max())
    n = Bn * P if held_by == "all" else held_by
    assert int(lo.sum()) == n and int(hi.sum()) == n
    assert float((shares - want).abs().max()) <= TOL * top
    assert float(shares[~(lo | hi)].abs().max() if (~(lo | hi)).any() else 0.0) <= TOL * top
    if held_by != "all":   # equal shares that sum to g_z_min and g_z_max (the fp64 checker's)
        for m in (lo, hi):
            assert float((shares[m] - shares[m][0]).abs().max()) <= TOL * top
            assert abs(float(shares[m].sum()) - float(want[m].sum())) <= TOL * top


# ---- the wavelength clamp -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("raw_value", [0.005, 0.6, 0.01, 0.5, -0.05, 0.0])
def test_wavelength_seams(raw_value):
    dev = _dev()
    c = _case(2, 35, 3, 740, lam=raw_value)
    ups = dict(phases=torch.rand(2, 70, generator=c["g"]))
    got = _run(c, ups, 2, "hip", dev, use=("phases",))
    w32, w64 = (_run(c, ups, 2, "checker", dtype=d, use=("phases",)) for d in (torch.float32, torch.float64))
    _judge(f"raw {raw_value}", "phases", got[0]["phases"], w32[0]["phases"], w64[0]["phases"], circular=True)
    if raw_value in (0.005, 0.6, 0.0):      # clamped (and |.| at 0): exactly no gradient
        assert float(got[3]) == 0.0
    elif raw_value in (0.01, 0.5):          # the closed interval passes the gradient; fp32 0.01 is below double 0.01: judged against the fp32 run
        assert float(w32[3]) != 0.0
        assert abs(float(got[3]) - float(w32[3])) <= TOL * abs(float(w32[3]))
    else:
        assert float(got[3]) > 0.0          # sign(raw) = -1 turns the negative gradient of lambda around
        _judge(f"raw {raw_value}", "grad wavelength_raw", got[3], w32[3], w64[3])


# ---- NaN ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_one_nan_depth_makes_every_phase_nan_and_nothing_else():
    dev = _dev()
    c = _case(2, 35, 3, 701)
    clean = _run(c, _ups(2, 70, c["g"]), 2, "hip", dev)[0]
    c["z"][1, 17] = float("nan")
    out = _run(c, _ups(2, 70, c["g"]), 2, "hip", dev)[0]
    assert bool(torch.isnan(out["phases"]).all())
    for k in ("scales", "rotations", "colors", "opacities"):
        assert torch.equal(out[k], clean[k]), k
    nan_pos = torch.isnan(out["positions"])
    want = torch.zeros(2, 35, 2, 3, dtype=torch.bool)
    want[1, 17, :, 2] = True
    assert torch.equal(nan_pos, want.reshape(2, 70, 3))
    assert torch.equal(out["positions"][~nan_pos], clean["positions"][~nan_pos])


# ---- absent upstream gradients ----------------------------------------------------------------------------------------------------------------
@gpu
def test_every_upstream_gradient_absent_in_turn_and_all_but_one_absent():
    dev = _dev()
    c = _case(2, 35, 3, 701)
    ups = _ups(2, 70, c["g"])
    for k in pc.OUTPUTS:
        for use in (tuple(n for n in pc.OUTPUTS if n != k), (k,)):
            got = _run(c, ups, 2, "hip", dev, use=use)
            w32, w64 = (_run(c, ups, 2, "checker", dtype=d, use=use) for d in (torch.float32, torch.float64))
            tag = f"without {k}" if len(use) > 1 else f"only {k}"
            for i, name in ((1, "grad raw"), (2, "grad base_z"), (3, "grad wavelength_raw")):
                _judge(tag, name, got[i], w32[i], w64[i])


# ---- repeatability and capture ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", [(3, 257, 8, 8), (1, RANGE_BLOCK_ITEMS + 1, 1, 1)])
def test_two_calls_are_bit_identical(shape):
    dev = _dev()
    Bn, P, KF, K = shape
    c = _case(Bn, P, KF, 702)
    ups = _ups(Bn, P * K, c["g"])
    a, b = _run(c, ups, K, "hip", dev), _run(c, ups, K, "hip", dev)
    for k in pc.OUTPUTS:
        assert torch.equal(a[0][k].view(torch.int32), b[0][k].view(torch.int32)), k
    for i in (1, 2, 3):
        assert torch.equal(a[i].view(torch.int32), b[i].view(torch.int32)), i


@gpu
def test_captured_graph_follows_the_wavelength_changed_in_place():
    from fresnel_amd.decoder import physics_head
    dev = _dev()
    c = _case(2, 35, 3, 701)
    K = 2
    ups = {k: v.to(dev) for k, v in _ups(2, 70, c["g"]).items()}
    raw, z, lam = (c[k].to(dev).requires_grad_(True) for k in ("raw", "z", "lam"))
    xy = c["xy"].to(dev)

    def step():
        out = physics_head(raw, xy, z, lam, num_gaussians=K, backend="hip")
        sum((out[k] * ups[k]).sum() for k in out).backward()
        return out

    def eager(value):
        with torch.no_grad():
            lam.fill_(value)
        for t in (raw, z, lam):
            t.grad = None
        out = step()
        torch.cuda.synchronize()
        return [out["phases"].detach().clone()] + [t.grad.detach().clone() for t in (raw, z, lam)]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager(0.05)
        want_new = eager(0.11)
        eager(0.05)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in (raw, z, lam):
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        lam.fill_(0.11)
        for t in (raw, z, lam):
            t.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = [captured["phases"]] + [t.grad for t in (raw, z, lam)]
    for name, a, b in zip(("phases", "grad raw", "grad base_z", "grad wavelength_raw"), got, want_new):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: the replay does not follow the new wavelength"


# ---- training ---------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_physics_decoder_trains_through_the_wave_renderer(tmp_path):
    from fresnel_amd import train
    _dev()
    model, history = train.main(["--decoder", "physics", "--use_wave_rendering", "--head_backend", "hip", "--learnable_wavelength",
                                 "--image_size", "64", "--batch_size", "2", "--max_images", "2", "--epochs", "2",
                                 "--data_dir", str(tmp_path / "no_images"), "--output_dir", str(tmp_path / "out")])
    assert len(history) == 2 and all(math.isfinite(h["total"]) for h in history)
    g = model.fresnel_zones._wavelength_raw.grad
    assert g is not None and bool(torch.isfinite(g)) and float(g) != 0.0
