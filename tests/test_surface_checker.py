"""Pins tests/surface_checker.py -- the only judge of the HIP surface-cloud generator, since the reference's C++ cannot be run --
by answers derived by hand from the reference's source, and proves by mutation that each rule is pinned.  Also the parts of
fresnel_amd.surface that need no GPU: argument validation of the C entry points and the command line.

Expected values are worked out HERE, from the formulae, with their own fp32 arithmetic; nothing is taken from the checker."""
import ctypes
import io
import os

import numpy as np
import pytest

import surface_checker as C

F = np.float32
ONE = F(1.0)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def ramp_case():
    """8 x 8, depth = x / 8 (dyadic).  Column 7 is the far plane (u = 1, z = 0: dropped), column 0 has confidence 0 (skipped)."""
    return np.tile(np.arange(8, dtype=np.float32) / F(8.0), (8, 1))


RAMP_PARAMS = dict(shell_enabled=False, wrap_enabled=False, density_enabled=False)


def step_case():
    """9 x 9 vertical step: column 0 = 0 (the minimum: confidence 0), columns 1-3 = 0.25, columns 4-8 = 0.75, and one spike of 4.75
    at (x 6, y 4) (the maximum: dropped).  The spike's horizontal neighbour (5, 4) has gx = 2 (4.75 - 0.75) / 8 = 1, gy = 0: the
    largest gradient, so max_gradient = 1 EXACTLY and normalized_grad is the gradient magnitude itself."""
    d = np.full((9, 9), 0.75, np.float32)
    d[:, 0] = 0.0
    d[:, 1:4] = 0.25
    d[4, 6] = 4.75
    return d


STEP_PARAMS = dict(edge_threshold=0.125, shell_edge_threshold=0.125, wrap_edge_threshold=0.125, density_gradient_threshold=0.125,
                   min_confidence=0.03125)
# Rows per pixel.  12 = base + back + 3 walls + 3 wraps + 4 fills, 1 = base only, 0 = nothing.  By hand (zero outside the frame):
#   column 0: confidence 0 -> nothing.                     the spike (6, 4): z = 0 -> dropped.
#   interior rows: x = 1: gx = 4 x 0.25 / 8 = 0.125 == the threshold -> base only (strict >);  x = 2, 5, 6, 7: flat -> base only;
#     x = 3, 4: gx = 4 x 0.5 / 8 = 0.25 -> all;  x = 8: the zero padding on the right, |gx| = 4 x 0.75 / 8 = 0.375 -> all.
#   rows 0 and 8: gy from the padding: (1, 0): gx = gy = 0.09375, magnitude 0.1326 -> all;  (2, 0): gx = 0, gy = 4 x 0.25 / 8 =
#     0.125 == the threshold -> base only;  x >= 3: gy >= 0.1875 -> all.
#   rows 3-5, x = 5 ... 7: next to the spike, magnitude >= 0.5 -> all.
STEP_COUNTS = [
    [0, 12, 1, 12, 12, 12, 12, 12, 12],
    [0, 1, 1, 12, 12, 1, 1, 1, 12],
    [0, 1, 1, 12, 12, 1, 1, 1, 12],
    [0, 1, 1, 12, 12, 12, 12, 12, 12],
    [0, 1, 1, 12, 12, 12, 0, 12, 12],
    [0, 1, 1, 12, 12, 12, 12, 12, 12],
    [0, 1, 1, 12, 12, 1, 1, 1, 12],
    [0, 1, 1, 12, 12, 1, 1, 1, 12],
    [0, 12, 1, 12, 12, 12, 12, 12, 12],
]
KIND_ORDER = [C.K_BASE, C.K_BACK] + [C.K_WALL] * 3 + [C.K_WRAP] * 3 + [C.K_FILL] * 4


def confidence_case():
    """5 x 5: column 0 = 0 (the minimum: confidence 0 < min_confidence, but KEPT), column 1 = 1 (the maximum: dropped), the rest
    0.5.  The largest gradient of a kept point is column 0's, rows 1-3: gx = 4 x 1 / 8 = 0.5 -- at points that emit nothing."""
    d = np.full((5, 5), 0.5, np.float32)
    d[:, 0] = 0.0
    d[:, 1] = 1.0
    return d


def two_point_positions():
    """x in {1, 1 + 3 ulp}: lo + hi = 2 + 3 x 2^-23 rounds (tie to even) to 2 + 2^-21, so the first centre is 1 + 2^-22 and the
    shifted bounds are -2^-22 and +2^-23: NOT symmetric.  The second centre is (-2^-22 + 2^-23) / 2 = -2^-24 and leaves
    -3 x 2^-24 and +3 x 2^-24.  (Extent 6 x 2^-24 < 1e-6: not scaled.)"""
    x = np.array([1.0, 1.0 + 3 * 2.0 ** -23], np.float32)
    return (x, np.zeros(2, np.float32), np.zeros(2, np.float32))


def base_row(cloud, x, y, width):
    rows = np.nonzero((cloud["point"] == y * width + x) & (cloud["kinds"] == C.K_BASE))[0]
    assert rows.size == 1
    return int(rows[0])


# ---- known answers, each against `mutate` (None = the checker as it is) --------------------------------------------------------------
def check_constant(mutate=None):
    c = C.surface_cloud(np.full((6, 5), 0.5, np.float32), mutate=mutate)
    assert c["positions"].shape == (0, 3) and c["opacities"].shape == (0,) and int(c["counts"].sum()) == 0
    assert (c["flags"] == C.KEPT).all()      # u = 0: z = depth_scale, kept; confidence 0 < 0.1, skipped


def check_ramp(mutate=None):
    p = C.params_dict(**RAMP_PARAMS)
    c = C.surface_cloud(ramp_case(), mutate=mutate, **RAMP_PARAMS)
    counts = c["counts"].reshape(8, 8)
    assert (counts[:, 0] == 0).all() and (counts[:, 1:7] == 1).all() and (counts[:, 7] == 0).all()
    assert (c["kinds"] == C.K_BASE).all() and c["positions"].shape == (48, 3)
    # max_gradient: the kept border pixel (6, 0): gx = 3 x 0.25 / 8 = 0.09375, gy = (5/8 + 2 x 6/8 + 7/8) / 8 = 0.375 (dyadic: exact)
    max_gradient = np.sqrt(F(0.09375) * F(0.09375) + F(0.375) * F(0.375))
    assert c["max_gradient"] == max_gradient
    base_size, opacity, aspect = F(p["base_size"]), F(p["opacity"]), F(p["aspect_ratio"])
    thr, shrink, gscale = F(p["edge_threshold"]), F(p["edge_shrink"]), F(p["gradient_scale"])
    for x in range(1, 7):
        for y in range(1, 7):            # interior: gx = 4 x (2 / 8) / 8 = 0.125 exactly, gy = 0
            r = base_row(c, x, y, 8)
            conf = (F(x) / F(8.0) - F(0.0)) / F(0.875)
            ng = F(0.125) / max_gradient
            assert ng > thr
            t = (ng - thr) / (ONE - thr)
            edge_factor = ONE - t * (ONE - shrink)
            base = base_size * (F(0.5) + F(0.5) * conf)
            expect_scale = np.array([base * edge_factor, base * edge_factor, base / aspect * edge_factor], np.float32)
            assert (c["scales"][r] == expect_scale).all(), (x, y)
            assert c["opacities"][r] == opacity * conf * (F(0.7) + F(0.3) * edge_factor), (x, y)
            # the rotation takes (0, 0, 1) to the normal normalize(-gx scale, 0, 1)
            n = np.array([-0.125 * float(gscale), 0.0, 1.0])
            n /= np.linalg.norm(n)
            w, qx, qy, qz = (float(v) for v in c["rotations"][r])
            rotated = np.array([2 * (qx * qz + w * qy), 2 * (qy * qz - w * qx), 1 - 2 * (qx * qx + qy * qy)])
            assert np.abs(rotated - n).max() < 1e-6, (x, y, rotated, n)
            assert (c["colors"][r] == F(0.7)).all()


def check_step(mutate=None):
    c = C.surface_cloud(step_case(), mutate=mutate, **STEP_PARAMS)
    assert c["max_gradient"] == ONE
    assert c["counts"].reshape(9, 9).tolist() == STEP_COUNTS
    start = 0
    for pt, n in enumerate(c["counts"]):                    # rows in point order, kinds in the reference's order
        assert (c["point"][start:start + n] == pt).all()
        assert c["kinds"][start:start + n].tolist() == KIND_ORDER[:n]
        start += n
    assert start == c["kinds"].size == sum(map(sum, STEP_COUNTS))


def check_confidence_order(mutate=None):
    p = C.params_dict()
    c = C.surface_cloud(confidence_case(), mutate=mutate)
    assert (c["counts"].reshape(5, 5)[:, 0] == 0).all() and (c["flags"].reshape(5, 5)[:, 0] == C.KEPT).all()
    assert c["max_gradient"] == F(0.5)
    # pixel (2, 2): gx = 4 x (0.5 - 1) / 8 = -0.25 -> normalized 0.25 / 0.5; its base scale shows which maximum was used
    r = base_row(c, 2, 2, 5)
    thr, shrink = F(p["edge_threshold"]), F(p["edge_shrink"])
    t = (F(0.25) / F(0.5) - thr) / (ONE - thr)
    edge_factor = ONE - t * (ONE - shrink)
    base = F(p["base_size"]) * (F(0.5) + F(0.5) * F(0.5))
    assert c["scales"][r][0] == base * edge_factor


def check_center_twice(mutate=None):
    pos = C.place_points(two_point_positions(), 3.0, mutate)
    assert pos[0].tolist() == [-3 * 2.0 ** -24, 3 * 2.0 ** -24]
    assert C.place_points(two_point_positions(), 0.0, mutate)[0].tolist() == [1.0, 1.0 + 3 * 2.0 ** -23]   # <= 0: untouched


def test_constant_depth_gives_an_empty_cloud():
    check_constant()


def test_exact_ramp():
    check_ramp()


def test_step_edge_counts_and_kind_order():
    check_step()


def test_max_gradient_runs_over_points_below_min_confidence():
    check_confidence_order()


def test_cloud_is_centred_twice():
    check_center_twice()


def test_hash():
    """pseudo_random (PC:190-194) against values worked out with Python integers."""
    def by_hand(x, y, i, seed):
        h = ((x * 374761393 + y * 668265263 + (i % 2 ** 32) * 2147483647 + seed) % 2 ** 32) ^ 0x85EBCA6B
        h = (((h >> 16) ^ h) * 0x7FEB352D) % 2 ** 32
        return h & 0xFFFF
    for args, low16 in (((3, 5, 7, 12345), 25663), ((0, 0, 0, 0), 31104), ((511, 257, 112, 4294967295), 35748)):
        assert by_hand(*args) == low16
        got = C.pseudo_random(np.array([args[0]]), np.array([args[1]]), args[2], args[3])
        assert got.dtype == np.float32 and got[0] == F(low16) / F(65535.0)


# ---- mutations: one rule changed, and a known-answer check above fails -----------------------------------------------------------
@pytest.mark.parametrize("mutate, check", [("edge_clamp", check_step), ("edge_clamp", check_ramp), ("non_strict", check_step),
                                           ("skip_before_maxgrad", check_confidence_order), ("center_once", check_center_twice)],
                         ids=["edge_clamp-step", "edge_clamp-ramp", "non_strict-step", "skip_before_maxgrad", "center_once"])
def test_mutation_is_caught(mutate, check):
    check()
    with pytest.raises(AssertionError):
        check(mutate)


def test_every_mutation_is_exercised():
    assert set(C.MUTATIONS) == {"edge_clamp", "non_strict", "skip_before_maxgrad", "center_once"}


def test_checker_defaults_match_the_dataclass():
    import dataclasses
    from fresnel_amd.surface import SurfaceGaussianParams
    assert {f.name: f.default for f in dataclasses.fields(SurfaceGaussianParams)} == C.DEFAULTS
    assert list(C.params_dict(SurfaceGaussianParams(wrap_layers=2)).items()) == list(dict(C.DEFAULTS, wrap_layers=2).items())


# ---- the C entry points reject bad arguments before touching a device ----------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from fresnel_amd import build
    return ctypes.CDLL(build.build())


def test_surface_entries_validate_arguments_without_a_gpu(lib):
    from fresnel_amd import _binding as B
    from fresnel_amd.surface import SurfaceGaussianParams
    lib.fgs_last_error.restype = ctypes.c_char_p
    vp, cp = ctypes.c_void_p, ctypes.POINTER
    lib.fgs_surface_workspace_bytes.argtypes = [cp(B.FgsSurfaceDims), cp(B.FgsSurfaceParams), cp(ctypes.c_size_t)]
    lib.fgs_surface_count.argtypes = [cp(B.FgsSurfaceDims), cp(B.FgsSurfaceParams)] + [vp] * 4
    lib.fgs_surface_emit.argtypes = [cp(B.FgsSurfaceDims), cp(B.FgsSurfaceParams)] + [vp] * 9 + [ctypes.c_int64, vp]
    n = ctypes.c_size_t(0)
    ok, good = B.FgsSurfaceDims(2, 37, 53), SurfaceGaussianParams().to_c()

    def ws(dims, params):
        return lib.fgs_surface_workspace_bytes(ctypes.byref(dims), ctypes.byref(params), ctypes.byref(n))

    assert ws(ok, good) == 0 and n.value >= 64 + 2 * 37 * 53
    for bad in (B.FgsSurfaceDims(0, 8, 8), B.FgsSurfaceDims(1, 0, 8), B.FgsSurfaceDims(1, 8, -1), B.FgsSurfaceDims(70000, 8, 8),
                B.FgsSurfaceDims(8, 32768, 16384)):
        assert ws(bad, good) == -1
        assert b"invalid dims" in lib.fgs_last_error()
    for field, value in (("subsample", 0), ("shell_wall_segments", -1), ("wrap_layers", -2), ("density_extra_count", -1)):
        p = SurfaceGaussianParams(**{field: value}).to_c()
        assert ws(ok, p) == -1
        assert b"invalid params" in lib.fgs_last_error()
    assert ws(B.FgsSurfaceDims(64, 4096, 4096), SurfaceGaussianParams(wrap_layers=100).to_c()) == -1   # rows beyond 2^31
    assert lib.fgs_surface_workspace_bytes(None, ctypes.byref(good), ctypes.byref(n)) == -1
    assert lib.fgs_surface_workspace_bytes(ctypes.byref(ok), None, ctypes.byref(n)) == -1
    assert lib.fgs_surface_workspace_bytes(ctypes.byref(ok), ctypes.byref(good), None) == -1
    assert lib.fgs_surface_count(ctypes.byref(ok), ctypes.byref(good), None, None, None, None) == -1
    assert b"null" in lib.fgs_last_error()
    assert lib.fgs_surface_count(ctypes.byref(B.FgsSurfaceDims(0, 8, 8)), ctypes.byref(good), None, None, None, None) == -1
    assert lib.fgs_surface_emit(ctypes.byref(ok), ctypes.byref(good), *([None] * 9), 10, None) == -1
    assert b"null" in lib.fgs_last_error()
    assert lib.fgs_surface_emit(ctypes.byref(ok), ctypes.byref(SurfaceGaussianParams(subsample=0).to_c()), *([None] * 9), 10, None) == -1


def test_python_wrapper_refuses_cpu_tensors_and_gradients(lib):
    import torch
    from fresnel_amd import _binding as B
    from fresnel_amd import surface
    with pytest.raises(B.FgsError):
        surface.surface_gaussians(torch.zeros(1, 8, 8))
    with pytest.raises(B.FgsError):
        surface.surface_gaussians(torch.zeros(1, 8, 8, requires_grad=True))
    with pytest.raises(B.FgsError):
        surface.workspace_bytes(1, 8, 8, surface.SurfaceGaussianParams(subsample=0))
    with pytest.raises(B.FgsError):
        surface.SurfaceGaussianParams(wrap_layers=1.5).to_c()
    assert surface.workspace_bytes(1, 8, 8) > 64 and surface.SurfaceGaussianParams().max_rows_per_point() == 12


# ---- command line --------------------------------------------------------------------------------------------------------------
def test_cli_arguments():
    from fresnel_amd import surface
    ap = surface.build_parser()
    a = ap.parse_args(["--data_dir", "D"])
    assert surface.params_from_args(a) == surface.SurfaceGaussianParams()
    assert a.image_size == 256 and a.batch_size == 8 and not a.overwrite and a.depth_exponent == 0.7
    a = ap.parse_args(["--data_dir", "D", "--image_size", "64", "--subsample", "2", "--batch_size", "1", "--overwrite",
                       "--shell_enabled", "0", "--wrap_layers", "5", "--base_size", "0.01", "--seed", "7"])
    p = surface.params_from_args(a)
    assert a.overwrite and a.image_size == 64 and a.batch_size == 1
    assert p == surface.SurfaceGaussianParams(subsample=2, shell_enabled=False, wrap_layers=5, base_size=0.01, seed=7)
    with pytest.raises(SystemExit):
        ap.parse_args([])                                   # --data_dir is required
    assert "batch size 1" in " ".join(ap.format_help().split())   # (argparse wraps the text)


def test_cli_writes_clouds_and_refuses_to_overwrite(tmp_path):
    import torch
    from PIL import Image
    from fresnel_amd import io as fio
    from fresnel_amd import surface
    from fresnel_amd.data import ImageDataset
    (tmp_path / "features").mkdir()
    rng = np.random.default_rng(5)
    for name in ("a", "b", "c"):
        Image.fromarray(rng.integers(0, 255, (16, 16, 3), dtype=np.uint8)).save(tmp_path / f"{name}.png")
    for name in ("a", "b"):                                  # c has no depth cache: skipped
        rng.random((16, 16), dtype=np.float32).tofile(tmp_path / "features" / f"{name}_depth.bin")
    calls = []

    def stub(depth, image, params, depth_exponent):
        calls.append((tuple(depth.shape), tuple(image.shape), params.subsample, depth_exponent))
        return [dict(positions=torch.full((n + 1, 3), float(len(calls))), scales=torch.ones(n + 1, 3), rotations=torch.ones(n + 1, 4),
                     colors=torch.zeros(n + 1, 3), opacities=torch.ones(n + 1)) for n in range(depth.shape[0])]

    argv = ["--data_dir", str(tmp_path), "--image_size", "16", "--subsample", "2"]
    out = io.StringIO()
    assert surface.main(argv, generator=stub, out=out) == 0
    assert calls == [((2, 16, 16), (2, 3, 16, 16), 2, 0.7)]
    lines = out.getvalue().splitlines()
    assert lines[0].startswith("c: no c_depth.bin") and lines[1].startswith("a: 1 Gaussians") and lines[2].startswith("b: 2 Gaussians")
    ds = ImageDataset(str(tmp_path), image_size=16, load_saag=True)
    has, cloud = ds.saag_cloud("b")
    assert has and cloud["saag_positions"].shape == (2, 3) and not ds.saag_cloud("c")[0]
    before = (tmp_path / "features" / "a_saag.bin").read_bytes()
    assert surface.main(argv, generator=stub, out=io.StringIO()) == 2 and len(calls) == 1        # refused: nothing generated
    assert (tmp_path / "features" / "a_saag.bin").read_bytes() == before
    assert surface.main(argv + ["--overwrite", "--batch_size", "1"], generator=stub, out=io.StringIO()) == 0 and len(calls) == 3
    assert fio.load_gaussians_from_binary(str(tmp_path / "features" / "a_saag.bin"))["positions"][0, 0] == 2.0
