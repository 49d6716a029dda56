"""The Fourier renderer (fgs_fourier_*, k_fourier_project, fresnel_amd.renderer.FourierGaussianRenderer) on the boundaries its
kernels cut at; the scenes are tests/fourier_seam_cases.py, the reference is the dense torch checker (tests/fourier_checker.py) with
the library's tie rule (tie="lowest").  Seven families:
  clamp  delta Gaussians that put d == 0, d == 1, pre == 0 and pre == 1 on a pixel EXACTLY (and d > 1, pre > 1, pre < 0 next to
         them), each with a gI on that pixel alone: both clamps pass the gradient on the closed interval;
  norm   the maximum ON 1e-8f (not normalised) and one ulp above (normalised);
  tie    equal maxima across channels, half-waves, waves and tiles: the arg-max is the lowest flat index, bit-reproducibly;
  many   1025 x 1025 = 289 tiles, the maximum in tile 288 / 259: the fold's second strided trip, the flat index 2 HW + pix;
  batch  three 130 x 70 images (6 tiles each), the maxima in different tiles: bit-equal to the images rendered alone;
  edge   frames on a 32 / 64 multiple, one row or column over, 1 x 1, 1 x n, n x 1; N of 32, 33, 64; the arg-max in the
         one-pixel-wide last column / row of an edge tile;
  vis    a Gaussian ON each of the six visibility bounds (culled: zero record, zero gradient rows) next to one a single fp32 ulp
         inside it (visible); every Gaussian on a bound; NaN and +Inf positions.
The statement is the project's standing rule: image and each of the five gradients within 1e-4 of the tensor's maximum of the
checker's fp32 run (the CPU test below shows that its fp32-fp64 spread is <= 5e-5 on every tensor compared so, the 1025 x 1025
frames included, so none needs helpers.assert_with_referee).  A tensor whose fp64 reference is identically zero has no scale: exact zeros are asserted.
The single-Gaussian opacity gradient is judged as in tests/test_hip_fourier.py.  The CPU tests at the end run the checker with ONE
rule changed per family and require the statement to fail by a wide margin."""
import numpy as np
import pytest
import torch

import fourier_cases as FC
import fourier_checker as fc
import fourier_seam_cases as SC
from helpers import rel_to_max

gpu = pytest.mark.gpu
TOL = 1e-4
SPREAD_MAX = 5e-5
NAMES = ["image"] + FC.GRADS


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def _opacity_scale(s, r64):
    """A single normalised Gaussian: dL/dopacity is analytically zero, 1e-4 is taken of the terms that cancel (test_hip_fourier)."""
    return float(np.abs(r64[2][3][0] * s["arrs"][3][0]).sum() / abs(float(s["arrs"][4][0])))


def rule(key, j, name):
    c = SC.case(key)
    r64 = SC.reference(key)[j][1]
    w64 = r64[0] if name == "image" else r64[2][FC.GRADS.index(name)]
    if name == "opacities" and c.get("single") and c.get("normalised"):
        return "scale"
    if not np.any(w64):
        return "zero"
    return "fp32"


def distances(key, got):
    """got: per image (image, [five gradients]) -> {(image index, tensor): (distance, tolerance)}."""
    out = {}
    for j, ((r32, r64), (img, grads)) in enumerate(zip(SC.reference(key), got)):
        for i, name in enumerate(NAMES):
            x = img if i == 0 else grads[i - 1]
            w32, w64 = (r32[0], r64[0]) if i == 0 else (r32[2][i - 1], r64[2][i - 1])
            how = rule(key, j, name)
            if not np.isfinite(x).all():
                err, tol = np.inf, TOL
            elif how == "zero":
                err, tol = (np.inf if np.any(x) else 0.0), 0.0
            elif how == "scale":
                err, tol = float(np.abs(x - w64).max() / _opacity_scale(SC.case(key)["images"][j], r64)), TOL
            else:
                err, tol = rel_to_max(x, w32), TOL
            out[(j, name)] = (err, tol)
    return out


def failures(dist):
    return {k: v for k, v in dist.items() if not v[0] <= v[1]}


def fails_widely(dist):
    """some tensor is at least 10 x its tolerance out (non-zero where exact zeros are required)"""
    return {k: v for k, v in dist.items() if v[0] >= 10 * v[1] and v[0] > 0}


def show(key, dist):
    print(key, {f"{j}:{n}": f"{e:.1e}/{t:.0e}" for (j, n), (e, t) in dist.items()})


# ---- CPU: the scenes are what they claim to be -----------------------------------------------------------------------------------
def _project(s, dtype):
    ts = [torch.tensor(a, dtype=dtype) for a in s["arrs"][:3]]
    return fc.project(*ts, torch.as_tensor(s["view"], dtype=dtype), *[float(v) for v in s["intr"][:4]])


def test_exact_camera_and_delta_gaussians():
    """The exact camera gives integer means and depth 1 in fp32 and fp64; the raw image of delta Gaussians holds the hand values
    and no other non-zero element; 1.5 / nextafter(1.5, 0) / -1.5 land on 2W / below it / on -W."""
    for key in SC.CLAMP_KEYS[:1] + SC.NORM_KEYS + SC.TIE_KEYS:
        c = SC.case(key)
        s = c["images"][0]
        for dt in (torch.float32, torch.float64):
            _, mean, depth = _project(s, dt)
            assert torch.equal(mean, mean.round()) and bool((depth == 1).all()), key
        for r in SC.reference(key)[0]:
            assert np.array_equal(r[1], c["hand"][0].astype(r[1].dtype)), key
    intr = SC.exact_intr(64, 32, 16)
    x = np.array([1.5, np.nextafter(np.float32(1.5), np.float32(0)), -1.5], np.float32)
    s = dict(arrs=[np.stack([x, np.zeros(3, np.float32), -np.ones(3, np.float32)], 1), np.ones((3, 3), np.float32),
                   np.tile(np.array([1, 0, 0, 0], np.float32), (3, 1))], view=SC.EYE, intr=intr)
    for dt in (torch.float32, torch.float64):
        u = _project(s, dt)[1][:, 0]
        assert float(u[0]) == 128.0 and 127.9999 < float(u[1]) < 128.0 and float(u[2]) == -64.0


@pytest.mark.parametrize("key", SC.KEYS)
def test_placement(key):
    """The facts a case states about itself, from the checker's fp32 and fp64 runs."""
    c = SC.case(key)
    for j, (s, runs) in enumerate(zip(c["images"], SC.reference(key))):
        W, H = s["W"], s["H"]
        for r in runs:
            raw = r[1]
            flat = raw.reshape(-1)
            first = int(np.nonzero(flat == flat.max())[0][0])
            if "index" in c:
                assert first == c["index"][j], (key, first)
            if "tile" in c:
                assert SC.tile_of(first, W, H) == c["tile"][j], (key, first)
            if "m" in c:
                assert float(flat.max()) == c["m"][j]
            if c["family"] in ("many", "batch", "edge"):
                assert fc.argmax_gap(torch.from_numpy(raw)) >= FC.MIN_GAP, key
            if c.get("place"):
                assert (first % (W * H) % W, first % (W * H) // W) == c["place"], key
            if c["family"] == "vis":
                _, mean, depth = _project(s, torch.from_numpy(raw).dtype)
                fx, fy, cx, cy, near, far = s["intr"]
                vis = ((depth > near) & (depth < far) & (mean[:, 0] > -W) & (mean[:, 0] < 2 * W) & (mean[:, 1] > -H)
                       & (mean[:, 1] < 2 * H)).numpy()
                assert [n for n in range(len(vis)) if not vis[n]] == c["culled"], key
    if c["family"] == "edge":
        print(key, "tries", c["tries"])
        assert c["tries"] <= SC.MAX_TRIES
    if c["family"] == "many":
        assert c["tile"][0] >= 256 and len(SC.tile_maxima(SC.reference(key)[0][0][1], SC.MANY_W, SC.MANY_H)) == 289
    if c["family"] == "batch":
        tops = [float(r32[1].max()) for r32, _ in SC.reference(key)]
        assert tops[1] < tops[0] and tops[1] < tops[2] and len(set(tops)) == 3 and len(set(c["tile"])) == 3
    if c["family"] == "norm":
        m = np.float32(c["m"][0])
        assert (m == SC.NORM_ABOVE) == c["normalised"] and SC.NORM_AT == np.float32(1e-8) and SC.NORM_ABOVE > SC.NORM_AT
        for r in SC.reference(key)[0]:  # both dtypes take the same side of the threshold
            assert (float(r[0].max()) == 1.0) == c["normalised"], key


def test_vis_bounds_are_exact():
    """ON the bound means equality in fp32; the neighbour is one fp32 ulp inside."""
    for bound, (p, axis, inward) in SC.VIS_BOUNDS.items():
        s = SC.case("vis-" + bound)["images"][0]
        _, mean, depth = _project(s, torch.float32)
        on = {"u_lo": mean[0, 0] == -SC.VIS_W, "u_hi": mean[0, 0] == 2 * SC.VIS_W, "v_lo": mean[0, 1] == -SC.VIS_H,
              "v_hi": mean[0, 1] == 2 * SC.VIS_H, "near": depth[0] == 1.0, "far": depth[0] == 4.0}[bound]
        assert bool(on), bound
        q = s["arrs"][0]
        assert q[1, axis] == np.nextafter(q[0, axis], np.float32(inward)) and q[1, axis] != q[0, axis]


@pytest.mark.parametrize("key", SC.KEYS)
def test_checker_spread(key):
    """fp32 is an adequate reference: the checker's fp32-fp64 spread is <= 5e-5 of max on every tensor compared against the
    fp32 run; a zero reference is zero in both runs."""
    bad = {}
    for j, (r32, r64) in enumerate(SC.reference(key)):
        for i, name in enumerate(NAMES):
            w32, w64 = (r32[0], r64[0]) if i == 0 else (r32[2][i - 1], r64[2][i - 1])
            how = rule(key, j, name)
            if how == "zero":
                assert not np.any(w32), (key, name)
            elif how == "fp32":
                spread = rel_to_max(w32, w64)
                print(f"{key} {j}:{name} spread {spread:.1e}")
                if not spread <= SPREAD_MAX:
                    bad[(j, name)] = spread
    assert not bad, bad


def test_checker_defaults_are_unchanged():
    """tie=None is the default and is the checker as it was (raw.max(), restated below rule by rule): bit-equal on every fixture;
    without a tie (the gapped fixtures) tie="lowest" gives the same values too."""
    for name in FC.FIXTURES:
        s = FC.fixture_scene(name)
        base = FC.checker_run("fixture", name, False)
        args = (s["arrs"], s["view"], s["intr"], s["W"], s["H"], s["bg"], s["gI"])
        runs = [fc.render_with_grads(*args, tie=None), variant(s, pick="even")]
        if name in FC.GAPPED:
            runs.append(fc.render_with_grads(*args, tie="lowest"))
        for r in runs:
            assert np.array_equal(r[0], base[0]) and np.array_equal(r[1], base[1]), name
            for a, b in zip(r[2], base[2]):
                assert np.array_equal(a, b), name
    with pytest.raises(ValueError):
        fc.render_with_grads(*args, tie="highest")


# ---- the checker with one rule changed (test code: the changed rules are nobody's product) ------------------------------------------
def _clamp(x, open_interval):
    if not open_interval:
        return torch.clamp(x, 0, 1)
    return torch.where((x > 0) & (x < 1), x, x.detach().clamp(0, 1))


def variant(s, f64=False, clamp="closed", thresh=">", nonstrict=None, pick="lowest"):
    """fourier_checker.render_with_grads restated with its rules as options.
    clamp "closed" | "open"; thresh ">" | ">=" (against 1e-8f); nonstrict: a visibility bound that admits equality;
    pick: where the maximum is taken -- "even" (raw.max()), "lowest", "highest", or a function raw (numpy) -> (flat index, value
    or None): the index the gradient lands on and, where not None, a constant that replaces the maximum's value."""
    dt = torch.float64 if f64 else torch.float32
    leaves = [torch.tensor(a, dtype=dt, requires_grad=True) for a in s["arrs"]]
    pos, scale, quat, color, opacity = leaves
    W, H = s["W"], s["H"]
    fx, fy, cx, cy, near, far = [float(v) for v in s["intr"]]
    bgt = torch.tensor([float(b) for b in s["bg"]], dtype=dt).view(3, 1, 1)
    cov, mean, depth = fc.project(pos, scale, quat, torch.as_tensor(s["view"], dtype=dt), fx, fy, cx, cy)
    vis = torch.ones_like(depth, dtype=torch.bool)
    for name, x, b, above in (("near", depth, near, True), ("far", depth, far, False), ("u_lo", mean[:, 0], -W, True),
                              ("u_hi", mean[:, 0], 2 * W, False), ("v_lo", mean[:, 1], -H, True), ("v_hi", mean[:, 1], 2 * H, False)):
        ok = (x > b) if above else (x < b)
        vis = vis & ((ok | (x == b)) if name == nonstrict else ok)
    raw = torch.zeros(3, H, W, dtype=dt) + (color.sum() + opacity.sum() + pos.sum()) * 0.0
    if bool(vis.any()):
        mean, cov, color, opacity = mean[vis], cov[vis], color[vis], opacity[vis]
        sigma = torch.sqrt((cov[:, 0, 0] + cov[:, 1, 1]) / 2 + 1e-8)
        sv = 2 * sigma ** 2 + 1e-8
        X = torch.arange(W, dtype=dt).view(1, 1, W)
        Y = torch.arange(H, dtype=dt).view(1, H, 1)
        d2 = (X - mean[:, 0].view(-1, 1, 1)) ** 2 + (Y - mean[:, 1].view(-1, 1, 1)) ** 2
        g = torch.exp(-d2 / sv.view(-1, 1, 1)) * opacity.view(-1, 1, 1)
        raw = raw + torch.einsum("nc,nhw->chw", color, g)
        flat = raw.reshape(-1)
        if pick == "even":
            m = raw.max()
        else:
            with torch.no_grad():
                if callable(pick):
                    index, value = pick(raw.numpy())
                else:
                    ties = torch.nonzero(flat == flat.max())
                    index, value = int(ties[0] if pick == "lowest" else ties[-1]), None
            m = flat[index] if value is None else flat[index] * 0 + value
        normalise = bool(m > 1e-8) if thresh == ">" else bool(m >= float(np.float32(1e-8)))
        img = raw / m if normalise else raw
        bgw = _clamp(1.0 - img.sum(0, keepdim=True), clamp == "open")
        img = _clamp(img + bgt * bgw, clamp == "open")
    else:
        img = bgt.expand(3, H, W).clamp(0, 1) + raw
    (img * torch.as_tensor(s["gI"], dtype=dt)).sum().backward()
    grads = [(t.grad if t.grad is not None else torch.zeros_like(t)).numpy() for t in leaves]
    return img.detach().numpy(), raw.detach().numpy(), grads


def _variant_got(key, **kw):
    return [(r[0], r[2]) for r in (variant(s, **kw) for s in SC.case(key)["images"])]


def test_variant_restates_the_checker():
    """With no rule changed the restatement reproduces the checker's runs bit for bit, and meets the statement with distance 0."""
    for key in ("clamp-dense", "norm-above-bg", "tie-waves", "batch-3cams", "vis-u_hi", "vis-all-on-bounds", "edge-65x63-n32"):
        for f64 in (False, True):
            for s, runs in zip(SC.case(key)["images"], SC.reference(key)):
                got, want = variant(s, f64=f64), runs[1 if f64 else 0]
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), key
                assert all(np.array_equal(a, b) for a, b in zip(got[2], want[2])), key
        assert all(e == 0 for e, _ in distances(key, _variant_got(key)).values())


def test_statement_sees_open_interval_clamps():
    """Open-interval clamps fail every one-pixel case that sits on a seam (at least 10 x the tolerance), and the dense one; the
    cases off the seams (E, G: pre beyond the interval; none) are the same under both."""
    for key in SC.CLAMP_KEYS:
        dist = distances(key, _variant_got(key, clamp="open"))
        show(key, dist)
        if key[6:] in ("E", "G", "none"):
            assert not failures(dist), key
        else:
            assert fails_widely(dist), f"{key}: open-interval clamps went unnoticed"


def test_statement_sees_a_non_strict_threshold():
    """`>=` in place of `>` normalises the image whose maximum is 1e-8f: at least 10 x the tolerance out; one ulp above, no change."""
    for key in SC.NORM_KEYS:
        dist = distances(key, _variant_got(key, thresh=">="))
        show(key, dist)
        if SC.case(key)["normalised"]:
            assert not failures(dist), key
        else:
            assert fails_widely(dist) and dist[(0, "image")][0] >= 10 * TOL, f"{key}: >= at the threshold went unnoticed"


def test_statement_sees_other_tie_rules():
    """The maximum's gradient on the HIGHEST tied index, or split evenly: at least 10 x the tolerance out on every tie scene."""
    for key in SC.TIE_KEYS:
        for pick in ("highest", "even"):
            dist = distances(key, _variant_got(key, pick=pick))
            show(f"{key} {pick}", dist)
            assert fails_widely(dist), f"{key}: tie rule '{pick}' went unnoticed"


def test_statement_sees_a_fold_that_stops_at_256_tiles():
    """A fold of the per-tile maxima that ignores tiles from 256 on normalises by a dimmer element: at least 10 x the tolerance."""
    for key in SC.MANY_KEYS:
        def pick(raw):
            return max(SC.tile_maxima(raw, SC.MANY_W, SC.MANY_H)[:256], key=lambda t: (t[0], -t[1]))[1], None
        dist = distances(key, _variant_got(key, pick=pick))
        show(key, dist)
        assert fails_widely(dist) and dist[(0, "image")][0] >= 10 * TOL, f"{key}: a fold of 256 tiles went unnoticed"


def test_statement_sees_a_batch_stride_of_one_tile():
    """Image b folding part[b + j] instead of part[b x tiles + j] takes other images' tiles for its own: at least 10 x the tolerance."""
    for key in SC.BATCH_KEYS:
        c = SC.case(key)
        part = [t for r32, _ in SC.reference(key) for t in SC.tile_maxima(r32[1], SC.BATCH_W, SC.BATCH_H)]
        got = []
        for b, s in enumerate(c["images"]):
            def pick(raw, b=b):
                k = max(range(b, b + 6), key=lambda k: (part[k][0], -part[k][1]))
                return part[k][1], (None if k // 6 == b else part[k][0])  # another image's maximum is a constant to this one
            r = variant(s, pick=pick)
            got.append((r[0], r[2]))
        dist = distances(key, got)
        show(key, dist)
        assert not failures({k: v for k, v in dist.items() if k[0] == 0})  # image 0 folds its own tiles
        assert fails_widely({k: v for k, v in dist.items() if k[0] == 1}), f"{key}: a batch stride of one tile went unnoticed"
        assert fails_widely({k: v for k, v in dist.items() if k[0] == 2}), f"{key}: a batch stride of one tile went unnoticed"


def test_statement_sees_non_strict_visibility():
    """Equality admitted on one bound makes the Gaussian ON it visible: at least 10 x the tolerance on that bound's scene and on
    the all-culled scene (non-zero where exact zeros are required); the other bounds' scenes do not change."""
    for bound in SC.VIS_BOUNDS:
        for key in SC.VIS_KEYS:
            dist = distances(key, _variant_got(key, nonstrict=bound))
            if key in ("vis-" + bound, "vis-all-on-bounds"):
                show(f"{key} {bound}", dist)
                assert fails_widely(dist) and dist[(0, "image")][0] >= 10 * TOL, f"{key}: equality on {bound} went unnoticed"
            else:
                assert not failures(dist), (key, bound)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _camera(s):
    from fresnel_amd.renderer import Camera
    fx, fy, cx, cy, near, far = [float(v) for v in s["intr"]]
    cam = Camera(fx, fy, cx, cy, s["W"], s["H"], near, far)
    cam.set_view(torch.from_numpy(np.asarray(s["view"], np.float32)))
    return cam


def hip(images, one_camera=False):
    """One call of FourierGaussianRenderer on the images of a case (batched when there are several) -> per image (image, [five
    gradients]), and what the forward left in `saved` (fourier_seam_cases.inspect_fourier_saved)."""
    from fresnel_amd.renderer import FourierGaussianRenderer
    dev, s0, B = _dev(), images[0], len(images)
    W, H = s0["W"], s0["H"]
    ren = FourierGaussianRenderer(W, H, background=tuple(s0["bg"])).to(dev)
    arrs = [np.stack([s["arrs"][i] for s in images]) if B > 1 else s0["arrs"][i] for i in range(5)]
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True) for a in arrs]
    cams = _camera(s0) if B == 1 or one_camera else [_camera(s) for s in images]
    img = ren(*ts, cams)
    saved = SC.inspect_fourier_saved(img, B, s0["arrs"][0].shape[0], W, H)
    gI = np.stack([s["gI"] for s in images]) if B > 1 else s0["gI"]
    (img * torch.from_numpy(np.ascontiguousarray(gI)).to(dev)).sum().backward()
    out, grads = img.detach().cpu().numpy(), [t.grad.cpu().numpy() for t in ts]
    if B == 1:
        return [(out, grads)], saved
    return [(out[b], [g[b] for g in grads]) for b in range(B)], saved


def _judge(key, got):
    dist = distances(key, got)
    show(key, dist)
    assert not failures(dist), failures(dist)


def _assert_saved(key, saved):
    """F, the maximum and its index in `saved` are the case's hand values, bit for bit."""
    c = SC.case(key)
    for j in range(len(c["images"])):
        if "hand" in c:
            assert np.array_equal(saved["F"][j], c["hand"][j]), key
        if "m" in c:
            assert saved["m"][j] == np.float32(c["m"][j]), (key, saved["m"][j])
        if "index" in c:
            assert int(saved["index"][j]) == c["index"][j], (key, int(saved["index"][j]))


@gpu
@pytest.mark.parametrize("key", SC.CLAMP_KEYS + SC.NORM_KEYS + SC.MANY_KEYS + SC.EDGE_KEYS)
def test_scene_against_checker(key):
    """clamp, norm, many, edge: `saved` holds the hand values (where the case has any), then the statement."""
    c = SC.case(key)
    got, saved = hip(c["images"])
    _assert_saved(key, saved)
    if c["family"] == "norm":
        peak = float(got[0][0].max())
        assert peak == 1.0 if c["normalised"] else peak < 0.31, peak
    if c["family"] in ("many", "edge"):  # no hand values: the maximum and its index are the checker's
        raw = SC.reference(key)[0][0][1]
        assert int(saved["index"][0]) == int(raw.argmax()), key
        assert rel_to_max(saved["F"][0], raw) <= TOL
    _judge(key, got)


@gpu
@pytest.mark.parametrize("key", SC.TIE_KEYS)
def test_tie_goes_to_the_lowest_flat_index(key):
    """The index in `saved`, the gradients against tie="lowest", and two runs bit-equal."""
    c = SC.case(key)
    got, saved = hip(c["images"])
    _assert_saved(key, saved)
    _judge(key, got)
    again, saved2 = hip(c["images"])
    assert np.array_equal(saved2["index"], saved["index"]) and np.array_equal(again[0][0], got[0][0])
    for name, a, b in zip(FC.GRADS, again[0][1], got[0][1]):
        assert np.array_equal(a, b), (key, name)


@gpu
@pytest.mark.parametrize("key", SC.BATCH_KEYS)
def test_batch_of_many_tiles_equals_single_images(key):
    """Three images of six tiles, maxima in different tiles, the middle one the dimmest: the batch meets the statement, and every
    image and gradient is bit-equal to the same image rendered alone."""
    c = SC.case(key)
    got, saved = hip(c["images"], one_camera=key == "batch-1cam")
    for b, (r32, _) in enumerate(SC.reference(key)):
        assert int(saved["index"][b]) == int(r32[1].argmax()), (key, b)
        assert SC.tile_of(int(saved["index"][b]), SC.BATCH_W, SC.BATCH_H) == c["tile"][b]
    _judge(key, got)
    for b, s in enumerate(c["images"]):
        one, saved1 = hip([s])
        assert np.array_equal(got[b][0], one[0][0]), (key, b)
        assert saved1["m"][0] == saved["m"][b] and saved1["index"][0] == saved["index"][b]
        for name, gb, g1 in zip(FC.GRADS, got[b][1], one[0][1]):
            assert np.array_equal(gb, g1), (key, b, name)


@gpu
@pytest.mark.parametrize("key", SC.VIS_KEYS)
def test_visibility_bounds(key):
    """A Gaussian ON a bound is culled: flag 0, a record of zeros but the opacity, five zero gradient rows.  One fp32 ulp inside it
    is visible: its record holds the checker's fp32 mean bit for bit (the exact camera), its gradients are non-zero and meet the
    statement.  With every Gaussian on a bound the image is the clamped background and every gradient is zero."""
    c = SC.case(key)
    s = c["images"][0]
    got, saved = hip(c["images"])
    rec, N = saved["rec"][0], s["arrs"][0].shape[0]
    _, mean, _ = _project(s, torch.float32)
    for n in range(N):
        if n in c["culled"]:
            assert saved["visible"][0][n] == 0 and not np.any(rec[n, :7]) and rec[n, 7] == s["arrs"][4][n], (key, n)
            assert all(not np.any(g[n]) for g in got[0][1]), (key, n)
        else:
            assert saved["visible"][0][n] == 1 and rec[n, 7] == s["arrs"][4][n], (key, n)
            if c.get("bound") in ("u_lo", "u_hi", "v_lo", "v_hi"):  # depth 2: every product of the projection is exact
                assert rec[n, 0] == mean[n, 0].item() and rec[n, 1] == mean[n, 1].item(), (key, n, rec[n, :2])
            assert all(np.any(g[n]) for g in got[0][1]), (key, n)
    if key == "vis-all-on-bounds":
        want = np.broadcast_to(np.clip(np.array(s["bg"], np.float32), 0, 1).reshape(3, 1, 1), got[0][0].shape)
        assert np.array_equal(got[0][0], want) and not np.any(saved["F"]) and saved["m"][0] == 0
    _judge(key, got)


@gpu
def test_nan_and_inf_positions_are_culled_without_a_trace():
    """A NaN and a +Inf position between visible Gaussians (the checker cannot express this: its 0 x sum goes NaN): the image and
    the others' gradients are bit-equal to the scene without the two, their own rows are zero, everything is finite."""
    full, rest, keep, gone = SC.nonfinite_scenes()
    got, saved = hip([full])
    want, _ = hip([rest])
    assert np.isfinite(got[0][0]).all() and all(np.isfinite(g).all() for g in got[0][1])
    assert np.array_equal(got[0][0], want[0][0])
    for name, g, w in zip(FC.GRADS, got[0][1], want[0][1]):
        assert np.array_equal(g[keep], w), name
        assert not np.any(g[gone]), name
        assert np.any(w), name
    assert list(saved["visible"][0]) == [1, 0, 1, 0, 1] and not np.any(saved["rec"][0][gone][:, :7])
    assert np.isfinite(saved["rec"]).all() and np.isfinite(saved["F"]).all()
