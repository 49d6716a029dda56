"""The fused HIP stages of the SAAG refinement decoder (csrc/fgs_saag.hip; fresnel_amd.decoder saag_mlp_inputs / saag_refine_head /
SAAGRefinementNet with backend "hip") on the GPU: the reference's fixtures R1-R3, random parity with the restated stages
(tests/saag_checker.py) in fp32 and fp64 under the 1e-4-of-maximum rule, sampling seams with known answers, the two feature
layouts, clamp-gate and degenerate-quaternion seams, bitwise repeatability, one captured forward + backward and a short training
run of --experiment 1."""
import math

import pytest
import torch

import saag_checker as sc
import workspace_guard as WG
from helpers import rel_to_max
from test_saag_mirror import (FIXTURES, GAINS, SEAM_GRID, assert_matches_fixture, build_mirror, fixture, fixture_cloud, fixture_gains,
                              gate_seam_inputs, linear_answer, linear_features, run_mirror, seam_positions)

gpu = pytest.mark.gpu
TOL = 1e-4
GROUPS = dict(position=slice(0, 3), scale=slice(3, 6), rotation=slice(6, 12), color=slice(12, 15), opacity=slice(15, 16))


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _channel_last(feats, dev):
    """(B, C, H, W) values held as the training loop holds them: a (B, H, W, C) tensor seen through permute(0, 3, 1, 2)."""
    v = feats.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not v.is_contiguous() or v.shape[1] == 1 or v.shape[2] * v.shape[3] == 1
    return v


def _hip_inputs(feats, cloud, dev, layout="last"):
    from fresnel_amd.decoder import saag_mlp_inputs
    f = _channel_last(feats, dev) if layout == "last" else feats.to(dev).contiguous()
    out = saag_mlp_inputs(f, *[t.to(dev) for t in cloud], backend="hip")
    torch.cuda.synchronize()
    return out.cpu()


def _hip_refine(raw, cloud, gains, ups, dev, rs=0.1, use=None):
    """saag_refine_head(backend 'hip') on CPU argument tensors -> outputs, g_raw, g_gains (CPU); `use`: the outputs that get an
    upstream gradient (all by default; the others' stay undefined: NULL in the C call)."""
    from fresnel_amd.decoder import saag_refine_head
    raw_d, gains_d = raw.to(dev).requires_grad_(True), gains.to(dev).requires_grad_(True)
    out = saag_refine_head(raw_d, *[t.to(dev) for t in cloud], gains_d, residual_scale=rs, backend="hip")
    sum((out[k] * ups[k].to(dev)).sum() for k in (use or out)).backward()
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in out.items()}, raw_d.grad.cpu(), gains_d.grad.cpu()


def _checker_refine(raw, cloud, gains, ups, dtype, rs=0.1, use=None):
    raw_c, gains_c = raw.to(dtype).requires_grad_(True), gains.to(dtype).requires_grad_(True)
    out = sc.refine(raw_c, *cloud, gains_c, residual_scale=rs)
    sum((out[k] * ups[k].to(dtype)).sum() for k in (use or out)).backward()
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)   # noqa: E731  (rotations alone do not reach the gains)
    return {k: v.detach() for k, v in out.items()}, zero(raw_c), zero(gains_c)


def _ups(out_shapes, g):
    return {k: torch.randn(s, generator=g) for k, s in out_shapes.items()}


def _shapes(Bn, N):
    return dict(positions=(Bn, N, 3), scales=(Bn, N, 3), rotations=(Bn, N, 4), colors=(Bn, N, 3), opacities=(Bn, N),
                pos_delta=(Bn, N, 3), scale_delta=(Bn, N, 3), color_delta=(Bn, N, 3), opacity_delta=(Bn, N, 1))


def _random_case(Bn, N, seed, C=None, grid=None):
    """raw FIRST from the seeded generator (the near-boundary shares were checked for exactly these draws), then the cloud: z on
    both sides of 0.1, non-unit quaternions, colours and opacities that reach both clamps with the larger gains below."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(Bn, N, 16, generator=g)
    pos = torch.randn(Bn, N, 3, generator=g)
    pos[..., 2] = torch.rand(Bn, N, generator=g) * 1.5 - 0.4
    cloud = [pos, torch.rand(Bn, N, 3, generator=g) * 0.2 + 0.01, torch.randn(Bn, N, 4, generator=g) * 1.5,
             torch.rand(Bn, N, 3, generator=g), torch.rand(Bn, N, generator=g)]
    gains = torch.tensor([0.7, 1.3, 2.5, 3.0])
    ups = _ups(_shapes(Bn, N), g)
    feats = torch.randn(Bn, C, grid[0], grid[1], generator=g) if C else None
    return raw, cloud, gains, ups, feats


def _near_boundary(raw):
    branch, trace, gap = sc.branch_info(raw.double()[..., 6:12])
    return (trace.abs() < 1e-3) | ((branch != 0) & (gap < 1e-3))


def _compare_refine(tag, got, want, near):
    out, g_raw, g_gains = got
    ref_out, ref_raw, ref_gains = want
    for k, v in out.items():
        a, b = v.double(), ref_out[k].double()
        if k == "rotations":
            both = torch.minimum((a - b).abs().amax(-1), (a + b).abs().amax(-1))
            assert float(both[near].max() if near.any() else 0.0) <= TOL * max(float(b.abs().max()), 1e-30), \
                f"{tag}: a left-out quaternion matches neither q nor -q"
            a, b = a[~near], b[~near]
        e = rel_to_max(a.numpy(), b.numpy())
        print(f"{tag}: {k} {e:.2e}")
        assert e <= TOL, f"{tag}: {k} is {e:.2e} of its maximum away"
    for name, sl in GROUPS.items():
        ga, gb = g_raw.double()[..., sl], ref_raw.double()[..., sl]
        if name == "rotation":
            ga, gb = ga[~near], gb[~near]
        e = rel_to_max(ga.numpy(), gb.numpy())
        print(f"{tag}: grad raw[{name}] {e:.2e}")
        assert e <= TOL, f"{tag}: the {name} channels of g_raw are {e:.2e} of their maximum away"
    e = rel_to_max(g_gains.double().numpy(), ref_gains.double().numpy())
    print(f"{tag}: grad gains {e:.2e}")
    assert e <= TOL, f"{tag}: the gain gradients are {e:.2e} of their maximum away"


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_hip_stages_on_the_fixtures(name):
    dev = _dev()
    fx = fixture(name)
    model, _ = build_mirror(fx)
    cloud = fixture_cloud(fx)
    inputs = _hip_inputs(torch.from_numpy(fx["in.features"]), cloud, dev)
    with torch.no_grad():
        raw = model.mlp(inputs)   # the reference's weights on the CPU: only the gather under test is the GPU's
    e = rel_to_max(raw.numpy(), fx["raw"])
    print(f"{name}: raw behind the hip inputs {e:.2e}")
    assert e <= TOL
    ups = {k: torch.from_numpy(fx["g." + k]) for k in sc.OUTPUTS}
    out, g_raw, g_gains = _hip_refine(torch.from_numpy(fx["raw"]), cloud, fixture_gains(fx), ups, dev, rs=model.residual_scale)
    for k, v in out.items():
        e = rel_to_max(v.numpy(), fx["out." + k])
        print(f"{name}: {k} {e:.2e}")
        assert e <= TOL, f"{name}: {k} is {e:.2e} of its maximum away from the reference"
    e = rel_to_max(g_raw.numpy(), fx["grad.raw"])
    print(f"{name}: grad raw {e:.2e}")
    assert e <= TOL
    for i, k in enumerate(GAINS):
        want = float(fx["grad.sd." + k])
        print(f"{name}: grad {k} {float(g_gains[i]):.6e} against {want:.6e}")
        assert abs(float(g_gains[i]) - want) <= TOL * max(abs(float(fx["grad.sd." + n])) for n in GAINS)


@gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_module_with_hip_backend_reproduces_every_fixture_gradient(name):
    dev = _dev()
    fx = fixture(name)
    model, _ = build_mirror(fx, backend="hip", device=dev)
    out, grads, g_raw = run_mirror(model, fx, dev)
    torch.cuda.synchronize()
    assert_matches_fixture(fx, out, grads, g_raw, name + " (hip)")


# ---- random parity against the checker ---------------------------------------------------------------------------------------------
CASES = {
    "c1_1x1_n1": dict(Bn=1, N=1, C=1, grid=(1, 1), seed=600),
    "c7_3x4_n63": dict(Bn=3, N=63, C=7, grid=(3, 4), seed=601),
    "c8_5x7_n64": dict(Bn=1, N=64, C=8, grid=(5, 7), seed=602),
    "c7_5x7_n65": dict(Bn=3, N=65, C=7, grid=(5, 7), seed=603),
    "c8_3x4_n255": dict(Bn=1, N=255, C=8, grid=(3, 4), seed=604),
    "c1_37x37_n256": dict(Bn=3, N=256, C=1, grid=(37, 37), seed=605),
    "c8_37x37_n257": dict(Bn=1, N=257, C=8, grid=(37, 37), seed=606),
    "default_c384_37x37_n1000": dict(Bn=2, N=1000, C=384, grid=(37, 37), seed=607),
}


@gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_random_parity_with_the_checker(case):
    dev = _dev()
    c = CASES[case]
    raw, cloud, gains, ups, feats = _random_case(**c)
    near = _near_boundary(raw)
    share = float(near.float().mean())
    print(f"{case}: {share * 100:.2f} % of the Gaussians are near a branch boundary")
    assert share <= 0.01
    inputs = _hip_inputs(feats, cloud, dev)
    got = _hip_refine(raw, cloud, gains, ups, dev)
    for dtype in (torch.float64, torch.float32):
        tag = f"{case} vs {str(dtype)[6:]}"
        want = sc.mlp_inputs(feats, *cloud, dtype=dtype)
        assert inputs.shape == want.shape
        e = rel_to_max(inputs[..., :c["C"]].double().numpy(), want[..., :c["C"]].double().numpy())
        print(f"{tag}: sampled features {e:.2e}")
        assert e <= TOL, f"{tag}: the sampled features are {e:.2e} of their maximum away"
        assert torch.equal(inputs[..., c["C"]:], sc.mlp_inputs(feats, *cloud, dtype=torch.float32)[..., c["C"]:])  # copies: exact
        _compare_refine(tag, got, _checker_refine(raw, cloud, gains, ups, dtype), near)


# ---- sampling seams ---------------------------------------------------------------------------------------------------------------
def _guarded(t, dev):
    """`t` on the device at the very END of a guarded allocation (tests/workspace_guard.py): the bytes behind its last element are
    the 0xFF pattern -- NaN as floats, so a read past the end shows in the value even under weight 0."""
    guard = WG.WorkspaceGuard("ff", [])
    buf = guard.allocate(tuple(t.shape), t.dtype, dev)
    buf.copy_(t.to(dev))
    return buf, guard


@gpu
@pytest.mark.parametrize("layout", ["last", "first"])
def test_sampling_seams_have_their_known_answers(layout):
    """Features linear in the texel indices: the bilinear result is a_c ix + b_c iy + d_c.  u, v exactly 0 and 1 (the last texel,
    whose right / lower neighbour at index W / H lies in the guard and must not be read), texel centres (the texel itself, bit
    for bit), z exactly 0.1, one ulp either side, 0 and negative."""
    from fresnel_amd.decoder import saag_mlp_inputs
    dev = _dev()
    (H, W), C = SEAM_GRID, 3
    feats, coef = linear_features(C, H, W)
    pos = seam_positions(H, W)
    N = pos.shape[1]
    g = torch.Generator().manual_seed(31)
    cloud = [pos, torch.rand(1, N, 3, generator=g), torch.randn(1, N, 4, generator=g), torch.rand(1, N, 3, generator=g),
             torch.rand(1, N, generator=g)]
    if layout == "last":
        buf, guard = _guarded(feats.permute(0, 2, 3, 1).contiguous(), dev)
        view = buf.permute(0, 3, 1, 2)
    else:
        view, guard = _guarded(feats, dev)
    out = saag_mlp_inputs(view, *[t.to(dev) for t in cloud], backend="hip")
    torch.cuda.synchronize()
    guard.check("after the gather")
    out = out.cpu()
    assert bool(torch.isfinite(out).all()), "a texel outside the grid was read (the guard's NaN shows)"
    ix, iy = sc.sample_coords(pos.double(), H, W)
    want = linear_answer(coef, ix, iy, 1)
    e = rel_to_max(out[..., :C].double().numpy(), want.numpy())
    print(f"{layout}: linear features {e:.2e}")
    assert e <= TOL
    # rows 0..5: the corners -- the first / last texel itself
    f = feats[0]
    for row, (y, x) in enumerate([(0, 0), (H - 1, W - 1), (H - 1, 0), (0, W - 1), (H - 1, 0), (0, W - 1)]):
        assert torch.equal(out[0, row, :C], f[:, y, x]), (row, out[0, row, :C], f[:, y, x])
    # rows 6 .. 6 + H W - 1: the texel centres, bit for bit
    centres = out[0, 6:6 + H * W, :C].reshape(H, W, C).permute(2, 0, 1)
    assert torch.equal(centres, f)
    # (the rows behind them: z exactly 0.1, one ulp either side, 0 and negative, and general points -- covered by `want` above)


@gpu
def test_one_by_one_grid_returns_its_texel():
    dev = _dev()
    g = torch.Generator().manual_seed(37)
    feats = torch.randn(2, 5, 1, 1, generator=g)
    pos = seam_positions(1, 1).expand(2, -1, -1).contiguous()
    N = pos.shape[1]
    cloud = [pos, torch.rand(2, N, 3, generator=g), torch.randn(2, N, 4, generator=g), torch.rand(2, N, 3, generator=g),
             torch.rand(2, N, generator=g)]
    out = _hip_inputs(feats, cloud, dev)
    assert torch.equal(out[..., :5], feats.reshape(2, 1, 5).expand(2, N, 5))


@gpu
@pytest.mark.parametrize("shape", [dict(Bn=2, N=65, C=7, grid=(3, 4)), dict(Bn=2, N=257, C=8, grid=(5, 7)),
                                   dict(Bn=1, N=64, C=384, grid=(37, 37))], ids=["odd_c7", "even_c8", "c384"])
def test_both_feature_layouts_give_the_same_bits(shape):
    dev = _dev()
    _, cloud, _, _, feats = _random_case(seed=640 + shape["N"], **shape)
    a, b = _hip_inputs(feats, cloud, dev, "last"), _hip_inputs(feats, cloud, dev, "first")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # a features tensor in neither layout goes through one contiguous copy: the same values again
    from fresnel_amd.decoder import saag_mlp_inputs
    wide = torch.zeros(feats.shape[0], feats.shape[1], feats.shape[2], feats.shape[3] + 3, device=dev)
    wide[..., :feats.shape[3]] = feats.to(dev)
    c = saag_mlp_inputs(wide[..., :feats.shape[3]], *[t.to(dev) for t in cloud], backend="hip").cpu()
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))


@gpu
def test_hip_backend_refuses_inputs_that_require_grad():
    from fresnel_amd.decoder import saag_mlp_inputs, saag_refine_head
    dev = _dev()
    raw, cloud, gains, _, feats = _random_case(Bn=1, N=8, seed=609, C=4, grid=(3, 3))
    d = [t.to(dev) for t in cloud]
    with pytest.raises(ValueError, match="torch"):
        saag_mlp_inputs(feats.to(dev).requires_grad_(True), *d, backend="hip")
    with pytest.raises(ValueError, match="torch"):
        saag_mlp_inputs(feats.to(dev), d[0].clone().requires_grad_(True), *d[1:], backend="hip")
    with pytest.raises(ValueError, match="torch"):
        saag_refine_head(raw.to(dev), *d[:4], d[4].clone().requires_grad_(True), gains.to(dev), backend="hip")


# ---- head seams -------------------------------------------------------------------------------------------------------------------
@gpu
def test_closed_clamp_gates_pass_the_gradient_at_exactly_0_and_1():
    dev = _dev()
    raw, cloud, gains = gate_seam_inputs()
    ups = _ups(_shapes(1, raw.shape[1]), torch.Generator().manual_seed(41))
    got = _hip_refine(raw, cloud, gains, ups, dev)
    want = _checker_refine(raw, cloud, gains, ups, torch.float64)
    assert torch.equal(got[0]["colors"], cloud[3]) and torch.equal(got[0]["opacities"], cloud[4])
    _compare_refine("closed gates", got, want, _near_boundary(raw))
    # through the clamped tensors alone: the gradient is the upstream gradient times gain x residual_scale, not 0
    only = ("colors", "opacities")
    _, g_raw, g_gains = _hip_refine(raw, cloud, gains, ups, dev, use=only)
    _, w_raw, w_gains = _checker_refine(raw, cloud, gains, ups, torch.float64, use=only)
    assert bool((g_raw[..., 12:16] != 0).all()) and not g_raw[..., :12].any()
    assert rel_to_max(g_raw.double().numpy(), w_raw.numpy()) <= TOL


@gpu
def test_sums_one_ulp_outside_the_unit_interval_get_no_gradient():
    """gain = residual_scale = 1: delta = raw.  1 + 2^-23 is the float above 1, 0 - 2^-149 the float below 0."""
    dev = _dev()
    N = 6
    g = torch.Generator().manual_seed(43)
    raw = torch.randn(1, N, 16, generator=g)
    col, opa = torch.zeros(1, N, 3), torch.zeros(1, N)
    col[:, ::2], opa[:, ::2] = 1.0, 1.0
    raw[:, ::2, 12:16] = 2.0 ** -23
    raw[:, 1::2, 12:16] = -(2.0 ** -149)
    assert float(raw[0, 1, 12]) < 0 and float((col + raw[..., 12:15]).max()) > 1 and float((col + raw[..., 12:15]).min()) < 0
    cloud = [torch.randn(1, N, 3, generator=g), torch.rand(1, N, 3, generator=g) + 0.1, torch.randn(1, N, 4, generator=g), col, opa]
    ups = _ups(_shapes(1, N), g)
    out, g_raw, g_gains = _hip_refine(raw, cloud, torch.ones(4), ups, dev, rs=1.0, use=("colors", "opacities"))
    assert torch.equal(out["colors"], col) and torch.equal(out["opacities"], opa)
    assert not g_raw.any(), g_raw[..., 12:16]
    assert not g_gains.any(), g_gains
    assert torch.equal(out["color_delta"], raw[..., 12:15]) and torch.equal(out["opacity_delta"], raw[..., 15:16])


@gpu
def test_zero_saag_quaternion_and_zero_or_negative_gains():
    dev = _dev()
    raw, cloud, _, ups, _ = _random_case(Bn=2, N=65, seed=603)
    cloud[2][0, :5] = 0.0       # q_delta (x) 0 = 0: normalize's clamp, not a division by zero
    near = _near_boundary(raw)
    for gains in (torch.tensor([0.7, 1.3, 2.5, 3.0]), torch.zeros(4), torch.tensor([-0.7, -1.3, -2.5, -3.0]),
                  torch.tensor([0.0, -1.0, 2.0, 0.0])):
        got = _hip_refine(raw, cloud, gains, ups, dev)
        for t in list(got[0].values()) + [got[1], got[2]]:
            assert bool(torch.isfinite(t).all())
        assert not got[0]["rotations"][0, :5].any() and not got[1][0, :5, 6:12].any()
        _compare_refine(f"gains {gains.tolist()}", got, _checker_refine(raw, cloud, gains, ups, torch.float64), near)


@gpu
def test_every_upstream_gradient_absent_in_turn_and_all_but_one_absent():
    dev = _dev()
    raw, cloud, gains, ups, _ = _random_case(Bn=1, N=65, seed=603)
    assert not _near_boundary(raw).any()   # (checked for this seed: the whole g_raw is compared, rotation channels included)
    for k in sc.OUTPUTS:
        for use in (tuple(n for n in sc.OUTPUTS if n != k), (k,)):
            _, g_raw, g_gains = _hip_refine(raw, cloud, gains, ups, dev, use=use)
            _, w_raw, w_gains = _checker_refine(raw, cloud, gains, ups, torch.float64, use=use)
            tag = f"without {k}" if len(use) > 1 else f"only {k}"
            assert rel_to_max(g_raw.double().numpy(), w_raw.numpy()) <= TOL, tag
            assert rel_to_max(g_gains.double().numpy(), w_gains.numpy()) <= TOL, tag


# ---- repeatability and capture ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N", [257, 100_000])
def test_two_calls_are_bit_identical(N):
    dev = _dev()
    raw, cloud, gains, ups, feats = _random_case(Bn=1, N=N, seed=608 if N > 257 else 606, C=8, grid=(5, 7))
    a_in, b_in = _hip_inputs(feats, cloud, dev), _hip_inputs(feats, cloud, dev)
    assert torch.equal(a_in.view(torch.int32), b_in.view(torch.int32))
    a, b = _hip_refine(raw, cloud, gains, ups, dev), _hip_refine(raw, cloud, gains, ups, dev)
    for k in a[0]:
        assert torch.equal(a[0][k].view(torch.int32), b[0][k].view(torch.int32)), k
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    if N > 257:  # the gain reduction spans 391 blocks; against sums in fp64
        _, _, want = _checker_refine(raw, cloud, gains, ups, torch.float64)
        for i, k in enumerate(GAINS):
            print(f"grad {k}: {float(a[2][i]):.8e} against {float(want[i]):.8e}")
            assert abs(float(a[2][i]) - float(want[i])) <= TOL * abs(float(want[i])), k


@gpu
def test_more_tiles_than_blocks_matches_the_checker():
    """300 000 Gaussians are 1172 tiles for the refine kernels' fixed grid of at most 1024 blocks: some blocks take a second tile."""
    dev = _dev()
    raw, cloud, gains, ups, _ = _random_case(Bn=1, N=300_000, seed=611)
    near = _near_boundary(raw)
    assert float(near.float().mean()) <= 0.01
    _compare_refine("300k", _hip_refine(raw, cloud, gains, ups, dev), _checker_refine(raw, cloud, gains, ups, torch.float64), near)


@gpu
def test_captured_forward_and_backward_replays_the_eager_bits():
    from fresnel_amd.decoder import SAAGRefinementNet
    dev = _dev()
    _, cloud, _, _, feats = _random_case(Bn=2, N=257, seed=606, C=8, grid=(5, 7))
    torch.manual_seed(5)
    model = SAAGRefinementNet(8, [16, 8], dropout=0.0, backend="hip").to(dev).train()
    f = _channel_last(feats, dev)
    d = [t.to(dev) for t in cloud]
    g = torch.Generator().manual_seed(47)
    ups = {k: v.to(dev) for k, v in _ups(_shapes(2, 257), g).items()}

    def step():
        out = model(f, *d)
        sum((out[k] * ups[k]).sum() for k in out).backward()
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            eager = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want = {k: v.detach().clone() for k, v in eager.items()}
    want_grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    del eager   # (with it the warm-up's autograd graph, whose nodes belong to the side stream)
    model.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for k, p in model.named_parameters():
        p.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(captured[k].view(torch.int32), want[k].view(torch.int32)), k
    for k, p in model.named_parameters():
        assert torch.equal(p.grad.view(torch.int32), want_grads[k].view(torch.int32)), k


# ---- training ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_experiment_1_trains_with_either_backend(tmp_path):
    from fresnel_amd import train
    _dev()
    runs = {}
    for backend in ("hip", "torch"):
        argv = ["--experiment", "1", "--saag_backend", backend, "--image_size", "64", "--batch_size", "2", "--max_images", "2",
                "--epochs", "4", "--lr", "1e-3", "--data_dir", str(tmp_path / "no_images"), "--output_dir", str(tmp_path / backend)]
        model, history = train.main(argv)
        assert len(history) == 4
        for h in history:
            assert math.isfinite(h["total"]) and "residual" in h and h["residual"] > 0
        torch.manual_seed(0)
        fresh = train.make_decoder(train.config_from_args(train.arg_parser().parse_args(argv)))
        for (k, p), q in zip(model.named_parameters(), fresh.parameters()):
            if k in GAINS or k == "mlp.net.0.weight":
                assert not torch.equal(p.detach().cpu(), q.detach()), f"{backend}: {k} has not moved"
        runs[backend] = history
    a, b = runs["hip"][0]["total"], runs["torch"][0]["total"]
    print(f"first step: hip {a:.8f}, torch {b:.8f}")
    assert abs(a - b) <= 1e-4 * abs(b)


@gpu
@pytest.mark.parametrize("backend", ["hip", "torch"])
def test_experiment_1_trains_on_a_data_dir_with_saag_files(tmp_path, monkeypatch, backend):
    """Two images whose `_saag.bin` clouds have the same size: the batch carries them, and the dummy cloud is never drawn."""
    from fresnel_amd import train
    from test_saag_mirror import _write_dataset
    _dev()
    _write_dataset(tmp_path / "data", [40, 40], S=32)

    def no_dummy(*a, **k):
        raise AssertionError("the batch holds SAAG clouds of equal size: the dummy cloud must not be drawn")

    monkeypatch.setattr(train, "create_dummy_saag", no_dummy)
    model, history = train.main(["--experiment", "1", "--saag_backend", backend, "--image_size", "64", "--batch_size", "2",
                                 "--epochs", "2", "--data_dir", str(tmp_path / "data"), "--output_dir", str(tmp_path / "out")])
    assert len(history) == 2 and all(math.isfinite(h["total"]) and h["residual"] > 0 for h in history)
