"""The HIP neighbour perception and update of the NCA decoder (csrc/fgs_nca.hip; fresnel_amd.decoder.nca_perceive / nca_update,
backend "hip") on the GPU: neighbour lists, gathered rows and the backward's ordered sums bit for bit against the restatement
of tests/nca_checker.py -- random clouds at the block and vector-width seams, exact ties, coincident points, a star, NaN and Inf
rows, a hub of in-degree N - 1 -- the update against torch's own expressions, the fixtures NCA1-NCA3 through the mirror, graph
capture and one training step of --experiment 5."""
import ctypes
import functools
import json
import math

import pytest
import torch

import nca_checker as nc
from test_nca_mirror import UNDECIDED_GAP, assert_matches_fixture, build_mirror, fixture, run_mirror, SMALL

gpu = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- clouds ---------------------------------------------------------------------------------------------------------------------
def _random(Bn, N, k, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Bn, N, D, generator=g), k


def _lattice():
    """5 x 5 x 3 integer lattice, twice: every distance is an integer and most are shared by several points (exact ties)."""
    p = torch.stack(torch.meshgrid(torch.arange(5.), torch.arange(5.), torch.arange(3.), indexing="ij"), -1).reshape(75, 3)
    g = torch.Generator().manual_seed(11)
    state = torch.cat([p.expand(2, 75, 3), torch.randn(2, 75, 13, generator=g)], -1).clone()
    state[1, :, :3] = p[torch.randperm(75, generator=g)]  # the second image in another order: other tie-breaks
    return state, 6


def _coincident():
    """70 points on 9 distinct positions: distance 0 to several others, more of them than k."""
    g = torch.Generator().manual_seed(12)
    state = torch.randn(2, 70, 16, generator=g)
    state[..., :3] = torch.randn(2, 9, 3, generator=g)[:, torch.arange(70) % 9]
    return state, 5


def _star(k):
    """A centre and the 12 vertices of an icosahedron of circumradius 1 (edge 1.05): every outlier is nearer to the centre than to
    any other outlier.  With k = 1 the centre has in-degree 12 and eleven outliers in-degree 0."""
    phi = (1 + math.sqrt(5)) / 2
    v = torch.tensor([[0, s1, s2 * phi] for s1 in (-1, 1) for s2 in (-1, 1)], dtype=torch.float64)
    v = torch.cat([v, v.roll(1, 1), v.roll(2, 1)])
    pts = torch.cat([torch.zeros(1, 3, dtype=torch.float64), v / v.norm(dim=1, keepdim=True)]).float()
    g = torch.Generator().manual_seed(13)
    state = torch.cat([torch.stack([pts, pts.flip(0)]), torch.randn(2, 13, 13, generator=g)], -1)  # the centre first / last
    return state, k


def _nan_inf():
    g = torch.Generator().manual_seed(14)
    state = torch.randn(1, 90, 16, generator=g)
    state[0, 3, :3] = float("nan")
    state[0, 71, 0] = float("inf")
    state[0, 40, 5] = float("nan")  # not a position channel: copied, never compared
    return state, 6


CASES = {
    "rand_1x7_k6": lambda: _random(1, 7, 6, 16, 1),           # N = k + 1: every other point is a neighbour
    "rand_3x64_k1": lambda: _random(3, 64, 1, 16, 2),         # exactly one block
    "rand_2x65_k16": lambda: _random(2, 65, 16, 16, 3),       # one point into the second block, the largest k
    "rand_2x257_k6_d7": lambda: _random(2, 257, 6, 7, 4),     # odd D: 4-byte copies
    "rand_2x377_k6": lambda: _random(2, 377, 6, 16, 5),       # the flagship shape
    "rand_1x4096_k6": lambda: _random(1, 4096, 6, 16, 6),     # the largest N
    "rand_2x130_k3_d6": lambda: _random(2, 130, 3, 6, 7),     # even D: 8-byte copies
    "lattice": _lattice, "coincident": _coincident, "star_k1": lambda: _star(1), "star_k3": lambda: _star(3), "nan_inf": _nan_inf,
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """state, k, the checker's lists and an upstream gradient: computed once, shared by the tests, never modified."""
    state, k = CASES[name]()
    g = torch.Generator().manual_seed(99)
    up = torch.randn(state.shape[0], state.shape[1], (k + 1) * state.shape[2], generator=g)
    return state, k, nc.neighbors(state, k), up


def _hip_perceive(state, k, up, dev):
    from fresnel_amd.decoder import nca_perceive
    s = state.to(dev).requires_grad_(True)
    perception, nbr = nca_perceive(s, k, backend="hip")
    perception.backward(up.to(dev))
    torch.cuda.synchronize()
    return perception.detach().cpu(), nbr.cpu(), s.grad.cpu()


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_perceive_forward_and_backward_equal_the_checker_bit_for_bit(name):
    dev = _dev()
    state, k, want, up = _case(name)
    Bn, N, D = state.shape
    perception, nbr, g_state = _hip_perceive(state, k, up, dev)
    assert nbr.dtype == torch.int32 and nbr.shape == (Bn, N, k)
    # in range, distinct, not self: for any input
    assert int(nbr.min()) >= 0 and int(nbr.max()) < N
    assert bool((nbr != torch.arange(N).view(1, N, 1)).all())
    assert bool((nbr.sort(dim=-1).values.diff(dim=-1) != 0).all())
    assert torch.equal(nbr.long(), want), f"{name}: {int((nbr.long() != want).any(-1).sum())} of {Bn * N} lists differ"
    assert torch.equal(_bits(perception), _bits(nc.perceive(state, want))), name
    assert torch.equal(_bits(g_state), _bits(nc.perceive_backward(want, up, D))), name
    again = _hip_perceive(state, k, up, dev)
    assert torch.equal(_bits(again[2]), _bits(g_state)) and torch.equal(again[1], nbr) and torch.equal(_bits(again[0]), _bits(perception))
    if name == "star_k1":
        deg = torch.bincount(nbr[0].reshape(-1).long(), minlength=N)
        assert int(deg[0]) == N - 1 and int((deg == 0).sum()) == N - 2


@gpu
def test_backward_with_a_hub_of_in_degree_n_minus_1():
    """fgs_nca_perceive_backward on a hand-made table: point 0 is a neighbour of every other point (its bit row spans ten words
    and five blocks of sources), point 1 of all but itself, most points of nobody; out-of-range entries are ignored."""
    from fresnel_amd import _binding as B
    dev = _dev()
    Bn, N, k, D = 2, 300, 2, 16
    nbr = torch.stack([torch.zeros(N), torch.ones(N)], -1).long().repeat(Bn, 1, 1)
    nbr[:, 0] = torch.tensor([1, 2])
    nbr[:, 1] = torch.tensor([0, 2])
    g = torch.Generator().manual_seed(21)
    up = torch.randn(Bn, N, (k + 1) * D, generator=g)
    want = nc.perceive_backward(nbr, up, D)
    lib, d = B.load(), B.FgsNcaDims(Bn, N, D, k)

    def run(table):
        t, u, out = table.to(torch.int32).to(dev), up.to(dev), torch.full((Bn, N, D), float("nan"), device=dev)
        B.check(lib.fgs_nca_perceive_backward(ctypes.byref(d), ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(u.data_ptr()),
                                              ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                "fgs_nca_perceive_backward")
        torch.cuda.synchronize()
        return out.cpu()

    assert torch.equal(_bits(run(nbr)), _bits(want))
    deg = torch.bincount(nbr[0].reshape(-1), minlength=N)
    assert int(deg[0]) == N - 1 and int((deg == 0).sum()) == N - 3
    wild = nbr.clone()
    wild[:, 5, 0], wild[:, 6, 1] = -7, N  # not lists of the forward: those slots contribute to nobody, nothing is dereferenced
    keep = wild.clamp(0, N - 1)
    ref = up[..., :D].clone()  # the checker's sum in the checker's order, without the two wild slots
    for i in range(N):
        for s in range(k):
            if 0 <= int(wild[0, i, s]) < N:
                ref[torch.arange(Bn), keep[:, i, s]] = ref[torch.arange(Bn), keep[:, i, s]] + up[:, i, (s + 1) * D:(s + 2) * D]
    assert torch.equal(_bits(run(wild)), _bits(ref))


# ---- update ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", [(2, 377, 16), (3, 65, 7), (5, 4096, 64)], ids=["flagship_vec4", "odd_d_scalar", "grid_stride"])
@pytest.mark.parametrize("masked", [False, True], ids=["eval", "train"])
def test_update_equals_the_torch_expressions(shape, masked):
    """Forward and dL/ddelta: bit-equal to torch's expression and its autograd ON THE GPU.  dL/dstep_size: within 1e-6 relative of
    the float64 sum of the exact products (the kernel adds them in double and rounds once, 6e-8) and bit-equal across two calls.
    dL/dstate is the upstream gradient, the same tensor."""
    from fresnel_amd.decoder import nca_update
    dev = _dev()
    g = torch.Generator().manual_seed(31 + shape[1])
    state, delta, up = (torch.randn(*shape, generator=g).to(dev) for _ in range(3))
    uniform = torch.rand(shape[0], shape[1], 1, generator=g).to(dev) if masked else None
    step = torch.tensor(0.137, device=dev)

    def run(backend):
        s, dl, st = state.clone().requires_grad_(True), delta.clone().requires_grad_(True), step.clone().requires_grad_(True)
        new = nca_update(s, dl, st, uniform, 0.5, backend=backend)
        new.backward(up)
        torch.cuda.synchronize()
        return new.detach(), s.grad, dl.grad, st.grad

    hip, ref = run("hip"), run("torch")
    assert torch.equal(_bits(hip[0]), _bits(nc.update(state, delta, step, uniform)))
    assert torch.equal(_bits(hip[0]), _bits(ref[0]))
    assert torch.equal(_bits(hip[1]), _bits(up)) and torch.equal(_bits(hip[2]), _bits(ref[2]))
    _, want = nc.update_backward(delta.cpu(), step.cpu(), up.cpu(), None if uniform is None else uniform.cpu())
    err = abs(float(hip[3].double().cpu()) - float(want)) / abs(float(want))
    print(f"dL/dstep_size {tuple(shape)} masked={masked}: hip {float(hip[3]):.9g}, float64 {float(want):.12g}, relative {err:.2e}; torch {float(ref[3]):.9g}")
    assert err <= 1e-6
    assert torch.equal(_bits(run("hip")[3].reshape(1)), _bits(hip[3].reshape(1)))
    if masked:
        mask = (uniform < 0.5).expand(shape)
        assert 0.3 < float(mask.float().mean()) < 0.7 and not bool(hip[2][~mask].any()) and torch.equal(hip[0][~mask], state[~mask])


@gpu
def test_update_returns_the_upstream_gradient_itself():
    from fresnel_amd.decoder import nca_update
    dev = _dev()
    state = torch.randn(2, 9, 16, device=dev, requires_grad=True)
    delta, step = torch.randn(2, 9, 16, device=dev, requires_grad=True), torch.tensor(0.1, device=dev, requires_grad=True)
    up = torch.randn(2, 9, 16, device=dev)
    g_state, = torch.autograd.grad(nca_update(state, delta, step, None, 0.5, backend="hip"), state, up)
    assert g_state.data_ptr() == up.data_ptr()


# ---- the mirror -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("head_backend", ["torch", "hip"])
@pytest.mark.parametrize("name", SMALL)
def test_mirror_with_hip_nca_reproduces_the_fixtures(name, head_backend, monkeypatch):
    dev = _dev()
    fx = fixture(name)
    model, _ = build_mirror(fx, nca_backend="hip", head_backend=head_backend, device=dev)
    out, traj, grads = run_mirror(model, fx, monkeypatch, device=dev)
    assert_matches_fixture(fx, out, traj, grads, f"{name} (nca hip, head {head_backend})")


@gpu
def test_hip_lists_equal_the_reference_on_decided_rows_of_nca3():
    from fresnel_amd.decoder import nca_perceive
    dev = _dev()
    fx = fixture("NCA3_default377")
    k = json.loads(str(fx["ctor"]))["k_neighbors"]
    states, ref = torch.from_numpy(fx["states"]), torch.from_numpy(fx["nbr"]).long()
    for s in range(states.shape[0]):
        nbr = nca_perceive(states[s].to(dev), k, backend="hip")[1].cpu().long()
        is_decided = nc.relative_gaps(states[s].double(), k) >= UNDECIDED_GAP
        differs = (nbr != ref[s]).any(dim=-1)
        assert not bool((differs & is_decided).any()), f"step {int(fx['steps'][s])}: {int((differs & is_decided).sum())} decided rows differ"
        assert torch.equal(nbr, nc.neighbors(states[s], k))


@gpu
def test_perceive_captured_in_a_graph_replays_bit_equal():
    from fresnel_amd.decoder import nca_perceive
    dev = _dev()
    state, k, want, up = _case("rand_2x377_k6")
    eager = _hip_perceive(state, k, up, dev)
    s, u = state.to(dev).requires_grad_(True), up.to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture: library load, autograd's first use of the stream
        torch.autograd.grad(nca_perceive(s, k, backend="hip")[0], s, u)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        perception, nbr = nca_perceive(s, k, backend="hip")
        g_state, = torch.autograd.grad(perception, s, u)
    for _ in range(2):
        for t in (perception, nbr, g_state):
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(perception.detach().cpu()), _bits(eager[0])) and torch.equal(nbr.cpu(), eager[1])
        assert torch.equal(_bits(g_state.cpu()), _bits(eager[2]))


@gpu
def test_one_training_step_of_experiment_5_without_host_synchronisation():
    """--experiment 5 --nca_backend hip --head_backend hip at 64 x 64, B = 2, 55 points, 3 steps: the loss is finite, every parameter
    that received a gradient moved, the zero-gradient ones are those behind the zero-initialised last update layer, and torch's
    sync debug mode sees no synchronising call in the step."""
    from fresnel_amd import train
    from fresnel_amd.dist import DPContext
    from fresnel_amd.renderer import TileBasedRenderer
    dev = _dev()
    a = train.arg_parser().parse_args(["--experiment", "5", "--nca_backend", "hip", "--head_backend", "hip", "--image_size", "64",
                                       "--batch_size", "2", "--n_spiral_points", "55", "--nca_steps", "3", "--lr", "2e-3"])
    cfg = train.config_from_args(a)
    cfg.device, cfg.feature_size, cfg.feature_dim = "cuda:0", 6, 16
    torch.manual_seed(0)
    model = train.make_decoder(cfg).to(dev).train()
    renderer, camera = train.default_renderer_factory(cfg, dev, 64)
    assert isinstance(renderer, TileBasedRenderer)
    opt = train.make_optimizer(model, cfg)
    dp = DPContext(device=dev)
    data = train.SyntheticDataset(4, cfg)
    batches = [data.batch([0, 1], dev), data.batch([2, 3], dev)]
    train.train_step(model, renderer, camera, batches[0], opt, cfg, dp)  # warm-up: plan caches, camera upload, library load
    torch.cuda.synchronize()
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = train.train_step(model, renderer, camera, batches[1], opt, cfg, dp)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ld = res.to_host()
    assert ld is not None and math.isfinite(ld["total"])
    no_grad = set()
    for k, p in model.named_parameters():
        if p.grad is None or not bool(p.grad.any()):
            no_grad.add(k)
        else:
            assert not torch.equal(p.detach(), before[k]), f"{k} received a gradient and did not move"
    print("zero-gradient parameters:", sorted(no_grad))
    assert all(k.startswith(("perception.", "update_rule.0.")) for k in no_grad)
    assert {"step_size", "depth_offset", "update_rule.2.weight", "init_state_net.0.weight"}.isdisjoint(no_grad)
