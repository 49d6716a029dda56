"""The fused wave self-attention (csrc/fgs_wave_attn.hip, fresnel_amd.cvs.fresnel_wave_attention backend "hip") on the GPU: the
reference's fixtures W1-W4 through the kernels and the modules, random parity with tests/wave_attn_checker.py (fp64, CPU) at the seams,
the wavelength's seams, NaN propagation, repeatability, capture and memory.  The tolerance is 1e-4 of the tensor's maximum
(tests/test_decoder_mirror.py) throughout; for the scalar g_wavelength that is 1e-4 of its fp64 value.

SEAMS, as (B, heads, grid_h, grid_w, d).  N = grid_h grid_w against the query block QB = key block KB = 128 and the key tile KT = 32;
d against the compiled head widths 32 | 64 | 128:

    grid     1 x 1 (one token) | 1 x 33 (KT + 1) | 16 x 8 (N = 128 = QB = KB) | 3 x 43 (129 = QB + 1) | 1 x 127 (QB - 1)      at d = 5
    d        5 | 33 | 64 | 128                                                                                                   on 3 x 43
    B, heads (1, 1) | (2, 3)                                                                                                     on 3 x 43, d 33
    32 x 32  the workload's own grid (N 1024: eight query and key blocks), B 1, one head, d 64
    64 x 64  the largest supported grid with the widest head (d 128): the case with the most LDS per workgroup

The wavelength of a seam case is 3.2 / grid_h: |wavelength| grid_h = 3.2 is the reference's default 0.1 on the workload's own 32 x 32
grid, so every grid sees the workload's phase per unit distance (1.96 rad).  At one fixed wavelength the thin grids would not be
cases at all: with grid_h = 1 and wavelength 0.1 every phase is within 1e-5 of a multiple of 2 pi times the distance, sin(phi) is a
difference of nearly equal numbers, and the checker's OWN fp32 run has g_wavelength 7e-3 (1 x 33) from its fp64 run.  With 3.2 / grid_h
the checker's fp32 run is within 1.2e-5 of its fp64 run in every tensor of every seam case, an eighth of the tolerance.
"""
import json
import math

import pytest
import torch

import wave_attn_checker as WC
from helpers import rel_to_max
from test_decoder_mirror import TOL
from test_attn_checker import assert_matches_attn_fixture
from test_wave_attn_checker import BLOCK_FIXTURES, WAVE_FIXTURES, build_mirror, cvs_fixture, run_mirror, run_wave

from fresnel_amd import _binding as B

gpu = pytest.mark.gpu
QB, KT, KB = B.FGS_ATTN_QUERY_BLOCK, B.FGS_ATTN_KEY_TILE, B.FGS_ATTN_KEY_BLOCK
REFEREE = 5e-5   # the project's referee rule: where the checker's own fp32 run is further than this from its fp64 run ...


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _wl(gh):
    """The seam cases' wavelength (the module's docstring)."""
    return 3.2 / gh


def _case(Bn, H, gh, gw, d, seed, spread=1.5):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(Bn, gh * gw, 3, H, d, generator=g)
    qkv[:, :, 0] *= spread
    return qkv.reshape(Bn, gh * gw, 3 * H * d), torch.randn(Bn, gh * gw, H * d, generator=g)


def _hip(qkv, grid, wl, H, up, dev):
    from fresnel_amd.cvs import fresnel_wave_attention
    ql = qkv.to(dev).requires_grad_(True)
    wll = torch.tensor(float(wl), device=dev).requires_grad_(True)
    out = fresnel_wave_attention(ql, grid, wll, H, backend="hip")
    out.backward(up.to(dev))
    torch.cuda.synchronize()
    return dict(out=out.detach().cpu(), g_qkv=ql.grad.cpu(), g_wavelength=wll.grad.cpu())


_CHECKED = {}


def _checker(qkv, grid, wl, H, up, dtype=torch.float64, key=None):
    """The checker's run on the CPU; with `key`, computed once and shared (the result is not modified by anyone)."""
    if key is not None and (key, dtype) in _CHECKED:
        return _CHECKED[(key, dtype)]
    ql = qkv.clone().to(dtype).requires_grad_(True)
    wll = torch.tensor(float(torch.tensor(float(wl))), dtype=dtype).requires_grad_(True)   # the fp32 value of wl
    out = WC.attend(ql, grid, wll, H)
    out.backward(up.to(dtype))
    res = dict(out=out.detach(), g_qkv=ql.grad, g_wavelength=wll.grad)
    if key is not None:
        _CHECKED[(key, dtype)] = res
    return res


def _dist(got, want):
    return {k: rel_to_max(got[k].double().numpy(), want[k].double().numpy()) for k in ("out", "g_qkv", "g_wavelength")}


def _compare(tag, got, want, tol=TOL):
    for k, e in _dist(got, want).items():
        print(f"{tag}: {k} {e:.2e}")
        assert e <= tol, f"{tag}: {k} is {e:.2e} of its maximum away from the checker"


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class _Calls:
    """Counts the entry points that go through the call layer while active (`call` re-enters itself once with the device guard
    held: the outer calls are counted)."""

    def __enter__(self):
        from fresnel_amd import _hip
        self.hip, self.real, self.names = _hip, _hip.call, []
        _hip.call = lambda dev_, name_, *a: (self.names.append(name_) if type(dev_) is not _hip.on_device else None,
                                             self.real(dev_, name_, *a))[1]
        return self

    def __exit__(self, *exc):
        self.hip.call = self.real
        return False


# ---- the reference's fixtures through the kernels --------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", WAVE_FIXTURES)
def test_fixture_through_fresnel_wave_attention_hip(name):
    from fresnel_amd.cvs import fresnel_wave_attention
    fx = cvs_fixture(name)
    out, grads = run_wave(fx, lambda *a: fresnel_wave_attention(*a, backend="hip"), device=_dev())
    assert_matches_attn_fixture(fx, out, grads, name)


@gpu
@pytest.mark.parametrize("name", WAVE_FIXTURES)
def test_fixture_through_the_module_with_backend_hip(name):
    dev = _dev()
    fx = cvs_fixture(name)
    module = build_mirror(fx).to(dev)
    module.backend = "hip"
    x = torch.from_numpy(fx["x"]).to(dev)
    with _Calls() as calls, torch.no_grad():
        module(x)
    assert calls.names == ["fgs_wave_attn_forward"]   # ONE call per module forward
    out, grads = run_mirror(module, fx, device=dev)
    assert_matches_attn_fixture(fx, out, grads, name + " (module)")


@gpu
@pytest.mark.parametrize("name", BLOCK_FIXTURES)
def test_block_fixture_through_attention_block_hip(name):
    dev = _dev()
    fx = cvs_fixture(name)
    module = build_mirror(fx, attn_backend="hip").to(dev)
    assert module.self_attn.backend == "hip" and module.cross_attn.backend == "hip"
    x, context = torch.from_numpy(fx["x"]).to(dev), torch.from_numpy(fx["context"]).to(dev)
    with _Calls() as calls, torch.no_grad():
        module(x, context)
    first = "fgs_wave_attn_forward" if json.loads(str(fx["ctor"]))["use_fresnel"] else "fgs_attn_forward"
    assert calls.names == [first, "fgs_attn_forward"]
    out, grads = run_mirror(module, fx, device=dev)
    assert_matches_attn_fixture(fx, out, grads, name + " (block)")


# ---- random parity with the checker, at the seams -----------------------------------------------------------------------------------------
SEAMS = ([(1, 2, gh, gw, 5) for gh, gw in ((1, 1), (1, KT + 1), (16, 8), (3, 43), (1, QB - 1))]
         + [(1, 2, 3, 43, d) for d in (33, 64, 128)]
         + [(Bn, H, 3, 43, 33) for Bn, H in ((1, 1), (2, 3))]
         + [(1, 1, 32, 32, 64), (1, 1, 64, 64, 128)])
assert 16 * 8 == QB == KB and 3 * 43 == QB + 1


@gpu
@pytest.mark.parametrize("Bn,H,gh,gw,d", SEAMS, ids=[f"B{b}H{h}-{gh}x{gw}-d{d}" for b, h, gh, gw, d in SEAMS])
def test_random_parity_with_the_checker(Bn, H, gh, gw, d):
    qkv, up = _case(Bn, H, gh, gw, d, 3000 + 7 * gh + 3 * gw + d)
    tag = f"B{Bn} H{H} {gh}x{gw} d{d}"
    want = _checker(qkv, (gh, gw), _wl(gh), H, up)
    if gh * gw > 1:
        assert float(want["g_wavelength"]) != 0.0
    _compare(tag, _hip(qkv, (gh, gw), _wl(gh), H, up, _dev()), want)


@gpu
def test_scores_spread_to_sixty_exercise_the_rescale():
    """Queries 15 times wider at d = 33: scores reach +-61 (asserted: 55 ... 70), the running maximum moves from tile to tile."""
    Bn, H, gh, gw, d = 1, 2, 3, 43, 33
    qkv, up = _case(Bn, H, gh, gw, d, 3100, spread=15.0)
    s = WC.scores(qkv.double(), (gh, gw), torch.tensor(_wl(gh), dtype=torch.float64), H)
    assert 55.0 < float(s.abs().max()) < 70.0, float(s.abs().max())
    _compare("spread", _hip(qkv, (gh, gw), _wl(gh), H, up, _dev()), _checker(qkv, (gh, gw), _wl(gh), H, up))


# ---- the wavelength's seams -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("wl,grid", [(-0.07, (5, 7)), (-0.07, (16, 8)), (-0.07, (16, 16)), (1e-3, (5, 7)), (1e-3, (16, 8)), (1e-3, (8, 8))],
                         ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_wavelength_seams(wl, grid):
    """-0.07: the sign of the subgradient, the tolerance 1e-4 as everywhere (on grids where the checker's own fp32 run is within
    3.3e-5 of its fp64 run in every tensor; on 3 x 43 its g_wavelength is 1.8e-4 away at this wavelength, which is no case for a
    tolerance of 1e-4).  1e-3: phases in the thousands of radians, where fp32 resolves a phase to 1e-4 rad only.  There the referee
    rule applies, per tensor: where the checker's OWN fp32 run is more than 5e-5 from its fp64 run, the kernel may be at most twice as
    far from the fp64 run as that fp32 run; everywhere else the tolerance is 1e-4 as usual.  The tensors the rule decided are
    printed.  The grids at 1e-3 are small on purpose: the checker's fp32 run is itself not reproducible from CPU to CPU at these
    phases (16 x 8: g_wavelength 8.4e-4 from the fp64 run on one host, 3.6e-4 on another; out 1.6e-5 and 6.8e-6), so "twice the
    fp32 run" is a bound that moves by a factor of two with the host; on 3 x 43, where the fp32 run's OUTPUT is 2.2e-4 ... 3.1e-4
    away, the host would decide the verdict."""
    Bn, H, d = 2, 2, 5
    qkv, up = _case(Bn, H, *grid, d, 3200 + grid[0])
    got = _hip(qkv, grid, wl, H, up, _dev())
    want64, want32 = _checker(qkv, grid, wl, H, up), _checker(qkv, grid, wl, H, up, dtype=torch.float32)
    own, far = _dist(want32, want64), _dist(got, want64)
    assert float(want64["g_wavelength"]) * wl != 0.0
    for k in far:
        refereed = wl == 1e-3 and own[k] > REFEREE
        bound = 2.0 * own[k] if refereed else TOL
        print(f"wavelength {wl} grid {grid}: {k} kernel {far[k]:.2e}, checker fp32 {own[k]:.2e}" + (" -- REFEREE RULE" if refereed else ""))
        assert far[k] <= bound, f"wavelength {wl} grid {grid}: {k} is {far[k]:.2e} from the fp64 run (bound {bound:.2e})"


@gpu
def test_wavelength_zero_is_finite_with_zero_gradient():
    qkv, up = _case(2, 2, 5, 7, 5, 3300)
    got = _hip(qkv, (5, 7), 0.0, 2, up, _dev())
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert float(got["g_wavelength"]) == 0.0 and bool(got["g_qkv"].any())
    # phi = 6.28 dist / 1e-6: an fp32 phase of 1e7 radians is resolved to a radian, so no run in another precision is a reference
    # for the bias here.  What holds whatever the cosines are: every bias lies in [-0.1, 0.1], so every probability is within a
    # factor e^+-0.2 of the unbiased one, and the output within (e^0.2 - 1) max|v| of the unbiased attention's
    ql = qkv.double()
    plain = WC.attend(ql, (5, 7), torch.tensor(0.0, dtype=torch.float64), 2, wrong="no_bias")
    v_max = float(ql.reshape(2, 35, 3, -1)[:, :, 2].abs().max())
    assert float((got["out"].double() - plain).abs().max()) <= (math.exp(0.2) - 1.0) * v_max


# ---- NaN ---------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_one_nan_query_propagates_through_its_head_only():
    Bn, H, gh, gw, d = 2, 2, 3, 43, 5
    N = gh * gw
    qkv, up = _case(Bn, H, gh, gw, d, 3400)
    dev = _dev()
    clean = _hip(qkv, (gh, gw), _wl(gh), H, up, dev)
    b, h, n = 1, 0, QB   # the first row of the second query block
    dirty_in = qkv.clone().reshape(Bn, N, 3, H, d)
    dirty_in[b, n, 0, h, 2] = float("nan")
    dirty = _hip(dirty_in.reshape(Bn, N, 3 * H * d), (gh, gw), _wl(gh), H, up, dev)
    out_c, out_d = (t["out"].reshape(Bn, N, H, d) for t in (clean, dirty))
    assert bool(torch.isnan(out_d[b, n, h]).all())
    rest = torch.ones(Bn, N, H, dtype=torch.bool)
    rest[b, n, h] = False
    assert _same_bits(out_d[rest], out_c[rest])   # every other row: the clean run's bits
    assert bool(torch.isnan(dirty["g_wavelength"]))
    g_c, g_d = (t["g_qkv"].reshape(Bn, N, 3, H, d).permute(0, 3, 1, 2, 4) for t in (clean, dirty))   # (B, H, N, 3, d)
    others = torch.ones(Bn, H, dtype=torch.bool)
    others[b, h] = False
    assert _same_bits(g_d[others], g_c[others])   # every other (b, h): the clean run's bits
    assert bool(torch.isnan(g_d[b, h, n, 0]).all()) and bool(torch.isnan(g_d[b, h, :, 1:]).all())   # as torch: the row's g_q, all g_k and g_v
    assert bool(torch.isfinite(clean["g_qkv"]).all()) and bool(torch.isfinite(clean["g_wavelength"]))


# ---- repeatability and capture ---------------------------------------------------------------------------------------------------------------
@gpu
def test_two_calls_and_batch_against_single_images():
    Bn, H, gh, gw, d = 3, 2, 3, 43, 33
    qkv, up = _case(Bn, H, gh, gw, d, 3500)
    dev = _dev()
    a, b = _hip(qkv, (gh, gw), _wl(gh), H, up, dev), _hip(qkv, (gh, gw), _wl(gh), H, up, dev)
    assert all(_same_bits(a[k], b[k]) for k in a)
    total = 0.0
    for i in range(Bn):
        one = _hip(qkv[i:i + 1], (gh, gw), _wl(gh), H, up[i:i + 1], dev)
        assert all(_same_bits(a[k][i:i + 1], one[k]) for k in ("out", "g_qkv")), f"image {i} depends on its batch"
        total += float(one["g_wavelength"].double())
    assert abs(float(a["g_wavelength"]) - total) <= TOL * abs(total)


@gpu
def test_captured_graph_follows_a_wavelength_changed_in_place():
    from fresnel_amd.cvs import fresnel_wave_attention
    dev = _dev()
    grid, H = (3, 43), 2
    qkv_c, up_c = _case(2, H, *grid, 10, 3600)
    qkv, up = qkv_c.to(dev).requires_grad_(True), up_c.to(dev)
    wl = torch.tensor(0.1, device=dev).requires_grad_(True)
    leaves = (qkv, wl)

    def step():
        out = fresnel_wave_attention(qkv, grid, wl, H, backend="hip")
        out.backward(up)
        return out

    def eager(value):
        with torch.no_grad():
            wl.fill_(value)
        for t in leaves:
            t.grad = None
        out = step()
        torch.cuda.synchronize()
        return [out.detach().clone()] + [t.grad.detach().clone() for t in leaves]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        want_old = eager(0.1)
        want_new = eager(0.23)
        eager(0.1)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not torch.equal(want_old[0], want_new[0])
    for t in leaves:
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        wl.fill_(0.23)
        for t in leaves:
            t.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for name, x, y in zip(("out", "g_qkv", "g_wavelength"), [captured] + [t.grad for t in leaves], want_new):
        assert _same_bits(x, y), f"{name}: the replay does not use the new wavelength"


# ---- limits --------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_limits_raise_without_a_launch():
    from fresnel_amd import cvs
    dev = _dev()
    wl = torch.tensor(0.1, device=dev)
    with _Calls() as calls:
        with pytest.raises(ValueError, match="head dimension 129"):
            cvs.fresnel_wave_attention(torch.randn(1, 4, 3 * 129, device=dev), (2, 2), wl, 1, backend="hip")
        with pytest.raises(ValueError, match="beyond the supported 4096"):
            cvs.fresnel_wave_attention(torch.randn(1, 4097, 3, device=dev), (4097, 1), wl, 1, backend="hip")
        with pytest.raises(B.FgsError, match="no CPU fallback"):
            cvs.fresnel_wave_attention(torch.randn(1, 4, 3, device=dev), (2, 2), torch.tensor(0.1), 1, backend="hip")
        assert calls.names == []
        # the library's own refusal (what the wrapper's checks stand in front of), as a clean error
        buf = torch.empty(4097 * 3, device=dev)
        with pytest.raises(B.FgsError, match="beyond the supported 4096"):
            calls.real(dev, "fgs_wave_attn_forward", 1, 4097, 1, 1, 1, 1.0, buf, wl, buf, buf)


# ---- memory ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_no_score_tensor_is_allocated():
    from fresnel_amd.cvs import fresnel_wave_attention
    dev = _dev()
    Bn, H, gh, gw, d = 1, 8, 32, 32, 64
    N = gh * gw
    scores = Bn * H * N * N * 4
    g = torch.Generator().manual_seed(3700)
    qkv0, up = torch.randn(Bn, N, 3 * H * d, generator=g).to(dev), torch.randn(Bn, N, H * d, generator=g).to(dev)
    rise = {}
    for backend in ("hip", "torch"):
        qkv, wl = qkv0.clone().requires_grad_(True), torch.tensor(0.1, device=dev).requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fresnel_wave_attention(qkv, (gh, gw), wl, H, backend=backend)
        out.backward(up)
        torch.cuda.synchronize()
        rise[backend] = torch.cuda.max_memory_allocated() - base
        del out, qkv, wl
    print(f"memory rise: hip {rise['hip'] / 2 ** 20:.1f} MiB, torch {rise['torch'] / 2 ** 20:.1f} MiB, one score tensor {scores / 2 ** 20:.1f} MiB")
    assert rise["hip"] < scores, rise
    assert rise["torch"] > scores, rise
