"""What pins tests/guided_surface_checker.py (no GPU): identity maps give surface_checker's cloud, one hand-worked derivative per
guide channel, and one mutation per rule.

TOL = 1e-6 absolute: the hand-worked values below are of magnitude <= 1 and are computed in fp64 from fp32-rounded parameters
(0.7f and 0.7 differ by 1e-8), so 1e-6 is two orders above what separates a right answer from its expected value and four below
the smallest derivative asserted here."""
import math

import numpy as np
import pytest
import torch

import guided_surface_checker as G
import surface_checker as C

F = np.float32
TOL = 1e-6


def f32(v):
    return float(F(v))


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def ramp_case():
    """8 x 8, depth = x / 8.  Column 7 is dropped (z = 0), column 0 has confidence 0.  Interior pixels: gx = 4 (2 / 8) / 8 = 0.125,
    gy = 0.  The largest gradient of a kept point is at (6, 0) and (6, 7): gx = 3 (2 / 8) / 8 = 0.09375, |gy| = (5 + 12 + 7) / 64 =
    0.375, max_gradient = sqrt(0.09375^2 + 0.375^2)."""
    return np.tile(np.arange(8, dtype=np.float32) / F(8.0), (8, 1))


RAMP_PARAMS = dict(shell_enabled=False, wrap_enabled=False, density_enabled=False)
RAMP_POINT = (4, 3)            # x, y: interior


def ramp_hand():
    """The forward quantities of RAMP_POINT by hand, in fp64 on the fp32 parameters."""
    conf = (4 / 8) / (7 / 8)                                  # (d - min) / range, range = 7 / 8
    c1 = 0.5 + 0.5 * conf
    ng = 0.125 / math.sqrt(0.09375 ** 2 + 0.375 ** 2)
    et, es = f32(0.15), f32(0.3)
    t = (ng - et) / (1 - et)
    ef = 1 - t * (1 - es)
    theta = math.acos(1 / math.sqrt(1 + 6.25 ** 2))           # normal = normalize(-0.125 x 50, 0, 1): tilted by theta about -y
    return dict(conf=conf, c1=c1, ng=ng, et=et, es=es, t=t, ef=ef, theta=theta, base=f32(0.008) * c1)


def step_case():
    """tests/test_surface_checker.py's 9 x 9 step, restated: columns 0 | 1-3 | 4-8 at 0 | 0.25 | 0.75 and a spike of 4.75 at (6, 4).
    max_gradient = 1 exactly (at (5, 4): gx = 1), so the normalized gradient is the magnitude itself: interior points of column 1
    have ng = 0.125 exactly, (5, 4) has ng = 1 exactly."""
    d = np.full((9, 9), 0.75, np.float32)
    d[:, 0] = 0.0
    d[:, 1:4] = 0.25
    d[4, 6] = 4.75
    return d


STEP_PARAMS = dict(edge_threshold=0.125, shell_edge_threshold=0.125, wrap_edge_threshold=0.125, density_gradient_threshold=0.125,
                   min_confidence=0.03125)


def _base_row(cloud, W, sub, x, y):
    gw = (W + sub - 1) // sub
    row = int(cloud["point_rows"][(y // sub) * gw + x // sub])
    assert row >= 0 and cloud["kinds"][row] == C.K_BASE
    return row


def _grad_of(depth, params, pick, mods=None, mutate=None):
    """d pick(cloud) / d mods (6, Hp, Wp) in fp64."""
    mods = (G.identity_mods(1, 1, torch.float64) if mods is None else mods.double()).clone().requires_grad_(True)
    cloud = G.guided_cloud(depth, None, mods, dtype=torch.float64, mutate=mutate, **params)
    pick(cloud).backward()
    return mods.grad


# ---- identity maps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["step", "ramp", "random_sub2"])
def test_identity_maps_give_the_plain_checker_cloud(case):
    if case == "step":
        depth, params, hw = step_case(), STEP_PARAMS, (1, 1)
    elif case == "ramp":
        depth, params, hw = ramp_case(), RAMP_PARAMS, (3, 5)
    else:
        rs = np.random.RandomState(5)
        depth, params, hw = rs.random_sample((13, 17)).astype(np.float32), dict(subsample=2, normal_strength=0.5), (37, 37)
    color = np.random.RandomState(6).random_sample((3,) + depth.shape).astype(np.float32)
    ref = C.surface_cloud(depth, color, **params)
    got = G.guided_cloud(depth, color, G.identity_mods(*hw), **params)
    assert ref["kinds"].size > 0
    for k in G.KEYS:
        a = got[k].numpy()
        assert a.dtype == np.float32 and a.shape == ref[k].shape
        assert np.abs(a - ref[k]).max() <= TOL, (k, np.abs(a - ref[k]).max())
    for k in ("positions", "colors", "scales"):                      # + - * / only: the same fp32 operations, the same bits
        assert np.array_equal(got[k].numpy(), ref[k]), k
    base = np.nonzero(ref["kinds"] == C.K_BASE)[0]
    assert np.array_equal(got["point_rows"][ref["point"][base]], base)
    assert (got["point_rows"] >= 0).sum() == base.size


# ---- one hand-worked point per channel -------------------------------------------------------------------------------------------------
def test_edge_factor_derivatives_by_hand():
    """ng = 0.5, threshold' = 0.25, shrink' = 0.5: t = 1/3, edge_factor = 1 - t (1 - shrink') = 5/6;
    d / d shrink' = t = 1/3;  d / d threshold' = -(1 - shrink') (ng - 1) / (1 - threshold')^2 = 0.5 x 0.5 / 0.5625 = 4/9."""
    th = torch.tensor([0.25], dtype=torch.float64, requires_grad=True)
    sh = torch.tensor([0.5], dtype=torch.float64, requires_grad=True)
    ef, edge = G.edge_factor(np.array([0.5], np.float32), np.array([0.25], np.float32), th, sh)
    ef.sum().backward()
    assert bool(edge[0]) and abs(float(ef.detach()) - 5 / 6) <= TOL
    assert abs(float(sh.grad) - 1 / 3) <= TOL and abs(float(th.grad) - 4 / 9) <= TOL


def test_slerp_derivative_by_hand_in_both_branches():
    """slerp branch: q = (cos a, sin a, 0, 0) with a = pi / 3 gives slerp(identity, q, t) = (cos t a, sin t a, 0, 0), so at t = 1/2
    d / dt = (-a sin(a / 2), a cos(a / 2), 0, 0) = (-pi / 6, pi sqrt(3) / 6, 0, 0).
    lerp branch: q = (1, 2^-10, 0, 0) has c = 1 > 1 - FLT_EPSILON: the result is (1 - t) identity + t q, d / dt = q - identity =
    (0, 2^-10, 0, 0) for every t."""
    a = math.pi / 3
    q = tuple(np.array([v], np.float32) for v in (math.cos(a), math.sin(a), 0.0, 0.0))
    t = torch.tensor([0.5], dtype=torch.float64, requires_grad=True)
    r = G.slerp_from_identity(q, t)
    want_r = (math.cos(a / 2), math.sin(a / 2), 0.0, 0.0)
    want_d = (-math.pi / 6, math.pi * math.sqrt(3) / 6, 0.0, 0.0)
    for i in range(4):
        assert abs(float(r[i].detach()) - want_r[i]) <= TOL
        g, = torch.autograd.grad(r[i].sum(), t, retain_graph=True)
        assert abs(float(g) - want_d[i]) <= TOL, (i, float(g))
    q = tuple(np.array([v], np.float32) for v in (1.0, 2.0 ** -10, 0.0, 0.0))
    t = torch.tensor([1.25], dtype=torch.float64, requires_grad=True)   # not clamped: a strength above 1 extrapolates
    r = G.slerp_from_identity(q, t)
    for i, want in enumerate((0.0, 2.0 ** -10, 0.0, 0.0)):
        g, = torch.autograd.grad(r[i].sum(), t, retain_graph=True)
        assert abs(float(g) - want) <= TOL and math.isfinite(float(g))
    assert abs(float(r[1].detach()) - 1.25 * 2.0 ** -10) <= TOL


CHANNEL_CASES = {
    # channel: (tensor, component, the derivative at identity maps by hand)
    "aspect_ratio": ("scales", 2, lambda h: -(h["base"] / f32(5.0)) * h["ef"]),                       # z = base / (5 m) ef
    "edge_threshold": ("scales", 0, lambda h: h["base"] * -(1 - h["es"]) * (h["ng"] - 1) / (1 - h["et"]) ** 2),
    "edge_shrink": ("scales", 0, lambda h: h["base"] * h["t"] * h["es"]),                              # x = base (1 - t (1 - es m))
    "normal_strength": ("rotations", 2, lambda h: -(h["theta"] / 2) * math.cos(h["theta"] / 2)),       # y = -sin(m theta / 2)
    "base_size": ("scales", 0, lambda h: h["base"] * h["ef"]),                                         # x = 0.008 m c1 ef
    "opacity": ("opacities", None, lambda h: f32(0.9) * h["conf"] * (f32(0.7) + f32(0.3) * h["ef"])),
}
CHANNEL_ORDER = ("aspect_ratio", "edge_threshold", "edge_shrink", "normal_strength", "base_size", "opacity")


@pytest.mark.parametrize("channel", CHANNEL_ORDER)
def test_one_hand_worked_point_per_channel(channel):
    """The base row of RAMP_POINT under a 1 x 1 guide at the identity: the derivative of one of its components with respect to the
    channel, from the formulas of include/fgs.h; the other five channels get exactly what their formulas say too (zero for a
    component they do not reach)."""
    key, comp, want = CHANNEL_CASES[channel]
    h = ramp_hand()
    x, y = RAMP_POINT

    def pick(cloud):
        row = _base_row(cloud, 8, 1, x, y)
        return cloud[key][row] if comp is None else cloud[key][row, comp]

    g = _grad_of(ramp_case(), RAMP_PARAMS, pick).reshape(6)
    c = CHANNEL_ORDER.index(channel)
    assert abs(float(g[c]) - want(h)) <= TOL, (channel, float(g[c]), want(h))
    assert abs(want(h)) > 1e-4                                       # a real derivative, not a zero that anything matches
    reaches = {"scales": {0: (1, 2, 4), 2: (0, 1, 2, 4)}, "rotations": {2: (3,)}, "opacities": {None: (1, 2, 5)}}[key][comp]
    for other in range(6):
        assert (float(g[other]) != 0.0) == (other in reaches), (channel, other, float(g[other]))


def test_forward_values_of_the_hand_worked_point():
    h = ramp_hand()
    cloud = G.guided_cloud(ramp_case(), None, G.identity_mods(1, 1, torch.float64), dtype=torch.float64, **RAMP_PARAMS)
    row = _base_row(cloud, 8, 1, *RAMP_POINT)
    assert abs(float(cloud["scales"][row, 0]) - h["base"] * h["ef"]) <= TOL
    assert abs(float(cloud["rotations"][row, 0]) - math.cos(h["theta"] / 2)) <= 1e-5     # (q itself is an fp32 constant)
    assert abs(float(cloud["rotations"][row, 2]) + math.sin(h["theta"] / 2)) <= 1e-5


# ---- one mutation per rule -----------------------------------------------------------------------------------------------------------
def _seam_scene():
    """10 x 10, subsample 3 (grid x = 0, 3, 6, 9), 5 patches per axis: pixel 6 lies in patch (6 x 5) / 10 = 3, while its grid index 2 of
    4 would give (2 x 5) / 4 = 2.  opacity_mult = 2^-(px) distinguishes them by a factor of two, exactly."""
    depth = (np.add.outer(np.arange(10), np.arange(10)) / 40.0 + 0.1).astype(np.float32)
    mods = G.identity_mods(5, 5, torch.float64)
    mods[5] = (2.0 ** -torch.arange(5, dtype=torch.float64)).reshape(1, 5).repeat(5, 1)
    return depth, dict(subsample=3), mods


def test_patch_comes_from_the_pixel_and_the_mutation_is_caught():
    depth, params, mods = _seam_scene()
    plain = C.surface_cloud(depth, None, **params)
    gw = 4
    row = int(np.cumsum(plain["counts"])[0 * gw + 2 - 1])            # first row of grid point (gx 2, gy 0) = pixel (6, 0)
    assert plain["point"][row] == 2 and plain["kinds"][row] == C.K_BASE
    want = float(plain["opacities"][row]) * 2.0 ** -3                 # patch 3: exact, a power of two commutes with rounding
    got = G.guided_cloud(depth, None, mods, **params)
    bad = G.guided_cloud(depth, None, mods, mutate="patch_from_grid", **params)
    assert abs(float(got["opacities"][row]) - want) <= TOL
    assert abs(float(bad["opacities"][row]) - want) >= 10 * TOL, "the mutation must fail this answer by ten tolerances"
    assert float(bad["opacities"][row]) == float(plain["opacities"][row]) * 2.0 ** -2


def test_edge_compare_is_strict_and_the_mutation_is_caught():
    """Column 1 of the step scene sits exactly on ng == edge_threshold' = 0.125: the forward takes edge_factor = 1, so the derivative
    of its scale with respect to edge_threshold_add is exactly 0.  With >= the forward value is the same (t = 0) but the branch
    is differentiated: base x -(1 - 0.3) (0.125 - 1) / 0.875^2 = 0.8 base."""
    x, y = 1, 2

    def pick(cloud):
        return cloud["scales"][_base_row(cloud, 9, 1, x, y), 0]

    g = _grad_of(step_case(), STEP_PARAMS, pick).reshape(6)
    assert float(g[1]) == 0.0 and float(g[2]) == 0.0
    bad = _grad_of(step_case(), STEP_PARAMS, pick, mutate="non_strict").reshape(6)
    conf = 0.25 / 4.75
    want_bad = f32(0.008) * (0.5 + 0.5 * conf) * (1 - f32(0.3)) * 0.875 / 0.875 ** 2
    assert abs(float(bad[1]) - want_bad) <= TOL
    assert abs(float(bad[1]) - 0.0) >= 10 * TOL, "the mutation must fail this answer by ten tolerances"


def test_clamp_passes_its_gradient_on_the_closed_interval():
    """The rule at the upper end.  t = (ng - th) / (1 - th) reaches 1 exactly where ng == 1 exactly -- the point that holds the
    image's largest gradient, (5, 4) of the step scene -- and nowhere else in fp32: 1 - ng >= 2^-24 for any other point, so
    (1 - ng) / (1 - th) cannot round away.  There dt / d th = (ng - 1) / (1 - th)^2 = 0: the gradient the closed interval lets
    through is itself zero, and dropping it (mutation "clamp_open") changes NO first-order answer.  So, unlike the other two
    rules, this one cannot be pinned by a derivative that the mutation gets wrong by ten tolerances; what is pinned instead:
    the point exists and is decided by the rule (the mutation moves it out of the interval), d / d edge_shrink is t = 1 there
    under both, and the derivative with respect to the threshold is 0 (to fp64 rounding) under both, as the algebra says.  The closed
    interval still matters to an implementation that writes the derivative differently (-1 / (1 - th) and (ng - th) /
    (1 - th)^2 summed in fp32 leave rounding residue): the GPU tests compare the kernel with this checker at exactly such
    points (depth kind `plateaus`)."""
    x, y = 5, 4
    ng = np.array([1.0], np.float32)
    th32 = np.array([0.125], np.float32)
    th = torch.tensor([0.125], dtype=torch.float64, requires_grad=True)
    sh = torch.tensor([0.3], dtype=torch.float64, requires_grad=True)
    for mutate in (None, "clamp_open"):
        ef, _ = G.edge_factor(ng, th32, th, sh, mutate)
        g_th, g_sh = torch.autograd.grad(ef.sum(), (th, sh), allow_unused=True)
        assert abs(float(ef.detach()) - 0.3) <= TOL and abs(float(g_sh) - 1.0) <= TOL
        assert g_th is None or abs(float(g_th)) <= 1e-12
    # the rule decides that point: inside the interval under the rule, outside under the mutation
    one = np.array([1.0], np.float32)
    assert bool(G.clamp_interval(one)[0]) and not bool(G.clamp_interval(one, "clamp_open")[0])
    assert bool(G.clamp_interval(np.array([0.0], np.float32), "clamp_open")[0])

    def pick(cloud):
        return cloud["scales"][_base_row(cloud, 9, 1, x, y), 0]

    g = _grad_of(step_case(), STEP_PARAMS, pick).reshape(6)
    conf = 0.75 / 4.75
    assert abs(float(g[1])) <= 1e-12                                 # zero up to the fp64 residue of -1 / u + u / u^2
    assert abs(float(g[2]) - f32(0.008) * (0.5 + 0.5 * conf) * 1.0 * f32(0.3)) <= TOL


def test_every_mutation_is_exercised():
    assert set(G.MUTATIONS) == {"patch_from_grid", "non_strict", "clamp_open"}
    with pytest.raises(AssertionError):
        G.guided_cloud(ramp_case(), None, G.identity_mods(1, 1), mutate="nonsense")


# ---- the referee rule of the GPU tests holds for the checker itself, on the GPU tests' seeds --------------------------------------------
def test_gradient_is_finite_on_flat_and_degenerate_points():
    """Constant depth (an empty cloud) and a 1 x 1 frame: the gradient exists and is zero / finite."""
    for depth in (np.full((4, 5), 0.5, np.float32), np.full((1, 1), 0.25, np.float32)):
        mods = G.identity_mods(2, 2, torch.float64).requires_grad_(True)
        cloud = G.guided_cloud(depth, None, mods, dtype=torch.float64)
        sum(cloud[k].sum() for k in G.KEYS).backward()
        assert mods.grad is not None and bool(torch.isfinite(mods.grad).all())
