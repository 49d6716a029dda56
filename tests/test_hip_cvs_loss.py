"""The fused CVS loss on the GPU (csrc/fgs_cvs_loss.hip through fresnel_amd/cvs_losses.py, backend "hip") against the fp64 checker
(tests/cvs_loss_checker.py) within TOL = 1e-4 -- of a tensor's maximum, of a scalar term's value -- at the seam shapes of its work split:
scalar and float4 groups, one and two groups per row, H or W of 1 and 2 (rolls onto the pixel itself and onto one row), a pred that
starts 4 bytes into its storage, and per path one shape with more work items than the largest grid has threads; every flag combination
the two classes can produce; the threshold pair; NaN; the refusals; bitwise repeatability, batch independence of the mask, graph
capture, no host synchronisation; the classes against the reference's fixtures; one step with both loss backends."""
import itertools
import json

import numpy as np
import pytest
import torch

import cvs_loss_checker as ck
from helpers import rel_to_max
from test_cvs_loss_checker import QUALITY_FIXTURES
from test_cvs_loss_mirror import assert_matches, run_consistency, run_quality
from test_decoder_mirror import TOL
from test_wave_attn_checker import cvs_fixture

gpu = pytest.mark.gpu
KEYS = ("quality", "consistency", "boundary", "gradient")
# QualityAwareCVSLoss: quality weighting on / off, with / without an EMA prediction, boundary and gradient terms on / off;
# ConsistencyLoss: no mask, no EMA model or the MSE form
QUALITY_COMBOS = [dict(zip(KEYS, v)) for v in itertools.product((True, False), ("l1", None), (True, False), (True, False))]
CONSISTENCY_COMBOS = [dict(quality=False, consistency=c, boundary=False, gradient=False) for c in ("mse", None)]
ALL, DEFAULT, MSE = QUALITY_COMBOS[0], dict(quality=True, consistency="l1", boundary=False, gradient=False), CONSISTENCY_COMBOS[0]
NO_PAIRS = [DEFAULT, MSE, dict(quality=True, consistency=None, boundary=False, gradient=False)]   # shapes with H or W of 1


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _id(combo):
    return "+".join(([] if not combo["quality"] else ["q"]) + ([combo["consistency"]] if combo["consistency"] else [])
                    + (["b"] if combo["boundary"] else []) + (["g"] if combo["gradient"] else [])) or "l1only"


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _offset_copy(t):
    """The same values in a contiguous tensor that starts 4 bytes into its storage."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def run_hip(case, combo, dev, misalign=False):
    """cvs_quality_terms(backend 'hip') and its backward under the case's g_terms -> terms (4,), g_pred, device tensors."""
    from fresnel_amd import cvs_losses as L
    t = {k: torch.from_numpy(case[k]).to(dev) for k in ("pred", "target", "depth", "ema", "g_terms")}
    pred = (_offset_copy(t["pred"]) if misalign else t["pred"]).detach().requires_grad_(True)
    terms = L.cvs_quality_terms(pred, t["target"], t["depth"], t["ema"], backend="hip", **combo)
    terms.backward(t["g_terms"])
    return terms.detach(), pred.grad


def assert_parity(case, combo, dev, what, misalign=False):
    terms, g_pred = run_hip(case, combo, dev, misalign)
    want = ck.loss(case["pred"], case["target"], case["depth"], case["ema"], g_terms=case["g_terms"], **combo)
    got = terms.cpu().double().numpy()
    on = (True, combo["consistency"] is not None, combo["boundary"], combo["gradient"])
    for i, name in enumerate(ck.TERMS):
        if on[i]:
            assert abs(got[i] - want["terms"][i]) <= TOL * abs(want["terms"][i]), f"{what} {_id(combo)}: {name} {got[i]!r} vs {want['terms'][i]!r}"
        else:
            assert got[i] == 0.0, f"{what} {_id(combo)}: {name} is off and must be written as 0"
    e = rel_to_max(g_pred.cpu().double().numpy(), want["g_pred"])
    assert e <= TOL, f"{what} {_id(combo)}: g_pred is {e:.2e} of its maximum away"
    return terms, g_pred, want


def assert_mask_and_euler(case, dev, what, seed):
    """The mask plane and the Euler step of a case's shape against the checker."""
    from fresnel_amd import cvs_losses as L
    depth = torch.from_numpy(case["depth"]).to(dev)
    mask = L.compute_quality_mask(depth, backend="hip")
    assert mask.shape == depth.shape and rel_to_max(mask.cpu().double().numpy(), ck.quality_mask(case["depth"])) <= TOL, what
    odd = L.compute_quality_mask(depth, threshold=0.004, sharpness=37.5, backend="hip")
    assert rel_to_max(odd.cpu().double().numpy(), ck.quality_mask(case["depth"], 0.004, 37.5)) <= TOL, what
    rs = np.random.RandomState(seed)
    Bn = case["pred"].shape[0]
    sac = np.sqrt(np.cumprod(1.0 - np.linspace(1e-4, 0.02, 40))).astype(np.float32)
    timestep = np.concatenate([[0, 39, 1], rs.randint(0, 40, size=Bn)])[:Bn].astype(np.int64)
    x0, noisy = (2.0 * case["pred"]).astype(np.float32), case["ema"]
    x_prev, t_prev = L.consistency_euler_step(torch.from_numpy(x0).to(dev), torch.from_numpy(noisy).to(dev), torch.from_numpy(sac).to(dev),
                                              torch.from_numpy(timestep).to(dev), backend="hip")
    want_x, want_t = ck.euler_step(x0, noisy, sac, timestep)
    assert x_prev.shape == x0.shape and t_prev.shape == (Bn,) and t_prev.dtype is torch.float32
    assert rel_to_max(x_prev.cpu().double().numpy(), want_x) <= TOL and np.array_equal(t_prev.cpu().double().numpy(), want_t), what
    return mask, x_prev, t_prev


# ---- parity at the seam shapes ----------------------------------------------------------------------------------------------------------
PAIR_SHAPES = [(2, 3, 5, 7), (2, 3, 4, 4), (3, 1, 8, 8), (1, 3, 2, 8), (1, 3, 8, 2), (2, 3, 33, 64)]
LINE_SHAPES = [(1, 3, 1, 9), (1, 3, 9, 1), (1, 1, 1, 1)]


@gpu
@pytest.mark.parametrize("shape", PAIR_SHAPES[:2], ids=["x".join(map(str, s)) for s in PAIR_SHAPES[:2]])
def test_every_flag_combination_matches_the_checker(shape):
    """(2,3,5,7): scalar, odd.  (2,3,4,4): ONE float4 group per row -- both horizontal wrap neighbours lie in the thread's own group."""
    dev = _dev()
    case = ck.make_case(shape, 2100 + sum(shape), edge_pair=True)
    for combo in QUALITY_COMBOS + CONSISTENCY_COMBOS:
        assert_parity(case, combo, dev, str(shape))
    assert_mask_and_euler(case, dev, str(shape), 7)


@gpu
@pytest.mark.parametrize("shape", PAIR_SHAPES[2:], ids=["x".join(map(str, s)) for s in PAIR_SHAPES[2:]])
def test_seam_shapes_match_the_checker(shape):
    """(3,1,8,8): C = 1, two groups per row.  (1,3,2,8): H = 2, both vertical neighbours are the same row.  (1,3,8,2): W = 2, scalar.
    (2,3,33,64): more than one block."""
    dev = _dev()
    case = ck.make_case(shape, 2200 + sum(shape), edge_pair=True)
    for combo in (ALL, DEFAULT, MSE, dict(ALL, quality=False)):
        assert_parity(case, combo, dev, str(shape))
    assert_mask_and_euler(case, dev, str(shape), 8)


@gpu
@pytest.mark.parametrize("shape", LINE_SHAPES, ids=["x".join(map(str, s)) for s in LINE_SHAPES])
def test_one_pixel_axes_roll_onto_the_pixel_itself(shape):
    dev = _dev()
    case = ck.make_case(shape, 2300 + sum(shape))
    for combo in NO_PAIRS:
        assert_parity(case, combo, dev, str(shape))
    assert_mask_and_euler(case, dev, str(shape), 9)


@gpu
def test_a_pred_that_starts_four_bytes_into_its_storage_takes_the_scalar_path():
    """W % 4 == 0 and every other pointer aligned, but pred is not: the call reads it with 4-byte loads (the library picks the scalar
    path from the pointers it is given).  The gradient is elementwise, so it has the aligned call's bits on either path."""
    dev = _dev()
    case = ck.make_case((2, 3, 33, 64), 2400)
    _, g_off, _ = assert_parity(case, ALL, dev, "offset pred", misalign=True)
    _, g_al, _ = assert_parity(case, ALL, dev, "aligned pred")
    assert _same_bits(g_off, g_al)


@gpu
@pytest.mark.parametrize("path", ["scalar", "float4"])
def test_a_thread_loops_twice(path):
    """One single-channel shape per path with more work items than the largest grid has threads (the kernel's own constants)."""
    from fresnel_amd import _binding as B
    dev = _dev()
    threads = B.FGS_CVS_THREADS * B.FGS_CVS_MAX_GRID
    W, V = (725, 1) if path == "scalar" else (2052, 4)
    H = (threads * V) // W + 1
    assert W % 4 == (0 if V == 4 else 1) and threads < (H * W) // V < threads + 2 * W
    case = ck.make_case((1, 1, H, W), 2500 + V)
    assert_parity(case, ALL, dev, f"{path} (1,1,{H},{W})")
    from fresnel_amd import cvs_losses as L
    mask = L.compute_quality_mask(torch.from_numpy(case["depth"]).to(dev), backend="hip")
    assert rel_to_max(mask.cpu().double().numpy(), ck.quality_mask(case["depth"])) <= TOL
    x0 = torch.from_numpy(case["pred"]).to(dev)
    sac = torch.linspace(0.99, 0.1, 10, device=dev)
    x_prev, t_prev = L.consistency_euler_step(x0, torch.from_numpy(case["ema"]).to(dev), sac, torch.tensor([4], device=dev), backend="hip")
    want_x, _ = ck.euler_step(case["pred"], case["ema"], sac.cpu().numpy(), np.array([4]))
    assert rel_to_max(x_prev.cpu().double().numpy(), want_x) <= TOL and t_prev.item() == 3.0


@gpu
def test_the_trainers_own_shape():
    dev = _dev()
    case = ck.make_case((4, 3, 256, 256), 2600)
    assert_parity(case, DEFAULT, dev, "(4,3,256,256)")
    assert_parity(case, ALL, dev, "(4,3,256,256)")


@gpu
def test_the_threshold_pair_on_the_device():
    """Depth differences of exactly 0.01f are no boundary, of nextafter(0.01f) are: with |pred - target| = 1 everywhere the term counts
    the boundaries -- one of the two x-pairs, one of the two y-pairs."""
    from fresnel_amd import cvs_losses as L
    dev = _dev()
    at = np.float32(0.01)
    above = np.nextafter(at, np.float32(1.0))
    depth = np.array([[0.0, at], [above, 0.0]], np.float32).reshape(1, 1, 2, 2)
    pred, target = np.ones((1, 1, 2, 2), np.float32), np.zeros((1, 1, 2, 2), np.float32)
    terms = L.cvs_quality_terms(torch.from_numpy(pred).to(dev), torch.from_numpy(target).to(dev), torch.from_numpy(depth).to(dev), None,
                                quality=False, consistency=None, boundary=True, backend="hip")
    want = ck.loss(pred, target, depth, None, quality=False, consistency=None, boundary=True)["terms"]
    assert want[2] == 1.0 and terms[2].item() == 1.0 and terms[0].item() == 1.0


@gpu
def test_a_nan_in_pred_reaches_the_terms_it_enters_and_no_others():
    from fresnel_amd import cvs_losses as L
    dev = _dev()
    case = ck.make_case((2, 3, 5, 7), 2700, edge_pair=True)
    clean, _ = run_hip(case, ALL, dev)
    mask = L.compute_quality_mask(torch.from_numpy(case["depth"]).to(dev), backend="hip")
    inner = dict(case, pred=case["pred"].copy())
    inner["pred"][1, 2, 2, 3] = np.nan
    terms, _ = run_hip(inner, ALL, dev)
    assert not bool(torch.isfinite(terms).any())   # an interior pixel enters all four
    corner = dict(case, pred=case["pred"].copy())
    corner["pred"][0, 1, 4, 6] = np.inf   # the last pixel of an image has no right and no lower difference: the boundary term skips it
    terms, _ = run_hip(corner, ALL, dev)
    assert not bool(torch.isfinite(terms[[0, 1, 3]]).any()) and _same_bits(terms[2:3], clean[2:3])
    no_cons = dict(ALL, consistency=None)
    terms, _ = run_hip(corner, no_cons, dev)
    assert terms[1].item() == 0.0   # a term that is off stays 0 whatever pred holds
    assert _same_bits(L.compute_quality_mask(torch.from_numpy(case["depth"]).to(dev), backend="hip"), mask)   # m comes from depth alone


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_are_value_errors_raised_on_the_host():
    from fresnel_amd import _binding as B
    from fresnel_amd import cvs_losses as L
    dev = _dev()
    for shape in ((1, 3, 1, 9), (1, 3, 9, 1)):
        c = {k: torch.from_numpy(v).to(dev) for k, v in ck.make_case(shape, 1).items()}
        for extra in (dict(boundary=True), dict(gradient=True)):
            with pytest.raises(ValueError, match="H >= 2 and W >= 2"):
                L.cvs_quality_terms(c["pred"], c["target"], c["depth"], c["ema"], backend="hip", **extra)
    c = {k: torch.from_numpy(v).to(dev) for k, v in ck.make_case((2, 3, 6, 8), 2).items()}
    for name in ("depth", "target", "ema"):
        with pytest.raises(ValueError, match=f"{name} requires grad"):
            L.cvs_quality_terms(*[c[k].clone().requires_grad_(k == name) for k in ("pred", "target", "depth", "ema")], backend="hip")
    with pytest.raises(ValueError, match="requires grad"):
        L.compute_quality_mask(c["depth"].clone().requires_grad_(True), backend="hip")
    sliced = {k: torch.cat([v, v], dim=-1)[..., ::2] for k, v in c.items() if k != "g_terms"}
    assert not sliced["pred"].is_contiguous()
    for name in ("pred", "target", "depth", "ema"):
        args = [sliced[k] if k == name else c[k] for k in ("pred", "target", "depth", "ema")]
        with pytest.raises(ValueError, match=f"{name} must be contiguous"):
            L.cvs_quality_terms(*args, backend="hip")
    with pytest.raises(ValueError, match="must be contiguous"):
        L.compute_quality_mask(sliced["depth"], backend="hip")
    with pytest.raises(ValueError, match="must be float32"):
        L.cvs_quality_terms(c["pred"].double(), c["target"].double(), c["depth"].double(), c["ema"].double(), backend="hip")
    with pytest.raises(B.FgsError, match="no CPU fallback"):
        L.cvs_quality_terms(c["pred"].cpu(), c["target"].cpu(), c["depth"].cpu(), c["ema"].cpu(), backend="hip")
    sac = torch.linspace(0.9, 0.1, 5, device=dev)
    with pytest.raises(ValueError, match="int64"):
        L.consistency_euler_step(c["pred"], c["ema"], sac, torch.tensor([1, 2], device=dev, dtype=torch.int32), backend="hip")
    with pytest.raises(ValueError, match="must be contiguous"):
        L.consistency_euler_step(sliced["pred"], c["ema"], sac, torch.tensor([1, 2], device=dev), backend="hip")
    # a timestep outside the table is clamped into it: memory-safe, a stated difference from torch
    lo = L.consistency_euler_step(c["pred"], c["ema"], sac, torch.tensor([-3, 99], device=dev), backend="hip")
    hi = L.consistency_euler_step(c["pred"], c["ema"], sac, torch.tensor([0, 4], device=dev), backend="hip")
    assert _same_bits(lo[0], hi[0]) and lo[1].tolist() == hi[1].tolist() == [0.0, 3.0]
    # the library's own refusal, which the wrapper's checks stand in front of
    from fresnel_amd import _hip as hip
    buf = torch.empty(4096, device=dev)
    with pytest.raises(B.FgsError, match="interior differences"):
        hip.call(dev, "fgs_cvs_loss_forward", 1, 3, 1, 9, B.FGS_CVS_GRADIENT, 0.01, 100.0, buf, buf, None, None, buf, None, buf)
    with pytest.raises(B.FgsError, match="not both"):
        hip.call(dev, "fgs_cvs_loss_forward", 1, 3, 4, 4, B.FGS_CVS_CONS_L1 | B.FGS_CVS_CONS_MSE, 0.01, 100.0, buf, buf, None, buf, buf, None, buf)
    with pytest.raises(B.FgsError, match="need depth"):
        hip.call(dev, "fgs_cvs_loss_forward", 1, 3, 4, 4, B.FGS_CVS_BOUNDARY, 0.01, 100.0, buf, buf, None, None, buf, None, buf)


# ---- repeatability, batch independence, capture, synchronisation -------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 3, 33, 64)], ids=["scalar", "float4"])
def test_two_runs_are_bit_equal_in_every_output(shape):
    from fresnel_amd import cvs_losses as L
    dev = _dev()
    case = ck.make_case(shape, 2800, edge_pair=True)

    def everything():
        terms, g_pred = run_hip(case, ALL, dev)
        return (terms, g_pred) + assert_mask_and_euler(case, dev, str(shape), 3)

    first = everything()
    L.cvs_quality_terms(*[torch.randn(3, 2, 9, 12, device=dev) for _ in range(2)], torch.rand(3, 1, 9, 12, device=dev),
                        torch.randn(3, 2, 9, 12, device=dev), boundary=True, gradient=True, backend="hip")   # another call in between
    for a, b in zip(first, everything()):
        assert _same_bits(a, b)


@gpu
@pytest.mark.parametrize("shape", [(2, 1, 5, 7), (3, 1, 8, 8)], ids=["scalar", "float4"])
def test_the_mask_of_a_batch_is_bit_equal_to_its_single_images(shape):
    from fresnel_amd import cvs_losses as L
    dev = _dev()
    depth = torch.from_numpy(ck.make_case((shape[0], 3) + shape[2:], 2900)["depth"]).to(dev)
    whole = L.compute_quality_mask(depth, backend="hip")
    for b in range(shape[0]):
        assert _same_bits(L.compute_quality_mask(depth[b:b + 1].contiguous(), backend="hip"), whole[b:b + 1])
    assert not _same_bits(whole[0], whole[1])


@gpu
def test_forward_and_backward_replay_from_a_graph_with_the_eager_bits():
    """Captured in a torch.cuda.graph, then replayed after pred, target, depth, ema and g_terms changed in place."""
    from fresnel_amd import cvs_losses as L
    dev = _dev()
    shape = (2, 3, 12, 16)
    case, other = ck.make_case(shape, 3000), ck.make_case(shape, 3001)
    names = ("pred", "target", "depth", "ema", "g_terms")
    static = {k: torch.from_numpy(case[k]).to(dev) for k in names}
    static["pred"].requires_grad_(True)

    def step():
        terms = L.cvs_quality_terms(static["pred"], static["target"], static["depth"], static["ema"], backend="hip", **ALL)
        terms.backward(static["g_terms"])
        return terms

    def eager(values):
        with torch.no_grad():
            for k in names:
                static[k].copy_(torch.from_numpy(values[k]))
        static["pred"].grad = None
        terms = step()
        torch.cuda.synchronize()
        return terms.detach().clone(), static["pred"].grad.detach().clone()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        want_old = eager(case)
        want_new = eager(other)
        eager(case)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not _same_bits(want_old[0], want_new[0])
    static["pred"].grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        for k in names:
            static[k].copy_(torch.from_numpy(other[k]))
        static["pred"].grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(captured.detach(), want_new[0]) and _same_bits(static["pred"].grad, want_new[1])


@gpu
def test_the_loss_calls_make_no_host_synchronisation():
    from fresnel_amd import cvs_losses as L
    dev = _dev()
    c = {k: torch.from_numpy(v).to(dev) for k, v in ck.make_case((2, 3, 16, 16), 3100).items()}
    pred = c["pred"].clone().requires_grad_(True)
    quality = L.QualityAwareCVSLoss(lambda_perceptual=0.0, lambda_boundary=0.5, lambda_gradient=0.25, backend="hip")
    sac, timestep = torch.linspace(0.99, 0.1, 20, device=dev), torch.tensor([0, 19], device=dev)

    def calls():
        out = quality(pred, c["target"], c["depth"], c["ema"], consistency_weight_override=0.3)
        out["total"].backward()
        mask = L.compute_quality_mask(c["depth"], backend="hip")
        x_prev, t_prev = L.consistency_euler_step(pred, c["ema"], sac, timestep, backend="hip")
        terms = L.cvs_quality_terms(pred, c["target"], None, x_prev, quality=False, consistency="mse", backend="hip")
        terms.sum().backward()
        return out, mask, t_prev

    calls()   # library load, first launches
    pred.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, mask, t_prev = calls()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert list(out) == ["l1_weighted", "consistency", "boundary", "gradient", "total"] and bool(pred.grad.any())
    assert t_prev.tolist() == [0.0, 18.0] and mask.shape == (2, 1, 16, 16)


# ---- the classes against the reference's fixtures ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", QUALITY_FIXTURES)
def test_quality_loss_on_hip_reproduces_the_fixture(name):
    fx = cvs_fixture(name)
    assert_matches(fx, run_quality(fx, device=_dev(), backend="hip"), name + " (hip)")


@gpu
def test_consistency_loss_on_hip_reproduces_the_fixture():
    fx = cvs_fixture("cvs_loss_C1")
    assert_matches(fx, run_consistency(fx, device=_dev(), backend="hip"), "cvs_loss_C1 (hip)")


# ---- the step -----------------------------------------------------------------------------------------------------------------------------
@gpu
def test_step_with_the_hip_loss_matches_the_torch_loss_and_never_synchronises_from_the_losses_on(capsys):
    """cvs_step on the U1 configuration at 16 x 16, B 2, quality-aware path with the boundary and gradient terms on: two steps with
    loss_backend "hip" against the same two steps with "torch" within TOL; and with "hip", from the moment the model's forward has
    returned -- EMA forward, losses, backward, clipping, optimizer step, EMA update -- torch's sync debug mode stays on "error"."""
    from fresnel_amd import cvs, cvs_train
    dev = _dev()
    fx = cvs_fixture("cvs_loss_T1")
    config = dict(json.loads(str(fx["ctor"])), lambda_boundary=0.5, lambda_gradient=0.25)
    batch = {k: torch.from_numpy(fx[k]).to(dev) for k in ("input_image", "features", "R_rel", "t_rel", "target_image", "target_depth")}

    def two_steps(backend, guarded):
        cfg = cvs_train.CVSTrainConfig(use_gaussian_targets=True, loss_backend=backend,
                                       **{k: v for k, v in config.items() if k not in ("lr", "weight_decay")})
        torch.manual_seed(int(fx["model_seed"]))
        model = cvs.ConsistencyViewSynthesizer(cvs.CVSConfig(**{k: tuple(v) if isinstance(v, list) else v
                                                               for k, v in json.loads(str(fx["model_ctor"])).items()})).to(dev)
        ema = cvs.create_ema_model(model).to(dev)
        loss_fn = cvs_train.make_cvs_loss(cfg)
        optimizer = torch.optim.AdamW(model.parameters(), lr=config["lr"], weight_decay=config["weight_decay"])
        hooks = []
        torch.manual_seed(77)
        out = []
        try:
            for k in range(2):
                if guarded and k == 1:   # (the first step loads the library and builds the optimizer's state: unguarded)
                    # the model's own forward runs unguarded; everything after it must not synchronise
                    hooks = [model.register_forward_pre_hook(lambda *a: torch.cuda.set_sync_debug_mode("default")),
                             model.register_forward_hook(lambda *a: torch.cuda.set_sync_debug_mode("error"))]
                out.append(cvs_train.cvs_step(model, ema, batch, optimizer, loss_fn, cfg, epoch=40))
        finally:
            torch.cuda.set_sync_debug_mode("default")
            for h in hooks:
                h.remove()
        return out

    hip_losses = two_steps("hip", True)
    torch_losses = two_steps("torch", False)
    capsys.readouterr()
    for a, b in zip(hip_losses, torch_losses):
        assert list(a) == list(b) == ["l1_weighted", "consistency", "boundary", "gradient", "total"]
        for k in a:
            assert a[k].is_cuda and not a[k].requires_grad
            assert abs(a[k].item() - b[k].item()) <= TOL * abs(b[k].item()), k
    assert hip_losses[0]["total"].item() != hip_losses[1]["total"].item()
