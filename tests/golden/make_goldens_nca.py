"""Fixtures of the NCA decoder mirror and its neighbour perception: the reference's NCAGaussianDecoder
(scripts/models/nca_gaussian_decoder.py) run on the CPU, in float32 and again in float64.  Runs only where the reference is present
(FRESNEL_REFERENCE = its checkout); the fixtures hold data only:

    ctor            the constructor's keyword arguments, as JSON            n_steps, training, seed, min_gap
    sd.<key>        the state dict
    in.<name>       features, depth
    uniform         (steps, B, N, 1) the draws of torch.rand, step by step (training mode only)
    traj            (steps + 1, B, N, D) the state before every step and after the last
    nbr             (steps, B, N, k) int16: the reference's neighbor_idx of every step (topk of cdist, self dropped)
    out.<name>      every entry of the returned dict                         g.<name>  the upstream gradient of that entry
    grad.features, grad.sd.<parameter>     gradients of sum_name sum(out.<name> x g.<name>); zeros where autograd gave none
    f64.<...>       traj, nbr, out.*, grad.* of the same run in float64 (same weights, inputs, draws and upstream gradients)

  NCA1  eval mode,     n_points 34, k 4, 4 steps, B 2, feature_dim 8, hidden_dim 16
  NCA2  training mode, the same with 8 steps, the draws recorded
  NCA3  default sizes (feature_dim 384, hidden_dim 128), B 2, n_points 377, k 6, 16 steps, eval mode: only `states` (4, B, N, D), the
        states before steps 0, 5, 10 and 15, and `nbr` (4, B, N, k), the reference's lists there.  No seed search.

Pinned harness-side while the reference runs: the random sign it adds to b2 before normalising (GDM:208) is +1, the draw this
repository's head fixes.  The last init_state_net layer is scaled up and the last update_rule layer, zero in
a fresh model, gets random weights, so that the points spread and move.

Seed condition of NCA1 and NCA2: the first seed at which, at every step, (a) the reference's float32 lists equal the canonical
lists of tests/nca_checker.py on the same state, (b) its float64 lists equal them too, and (c) the smallest relative gap between
consecutive sorted neighbour distances (the (k+1)-th other point included, nca_checker.relative_gaps on the float64 states) is
>= 5e-4: the fixtures then say the same thing under either neighbour definition and in either precision.
"""
import contextlib
import json
import os
import sys

REF = os.environ.get("FRESNEL_REFERENCE", "")
if not os.path.isdir(os.path.join(REF, "scripts")):
    sys.exit("make_goldens_nca.py: set FRESNEL_REFERENCE to a checkout of the reference; fixtures can only be generated where it is present")
sys.path.insert(0, os.path.join(REF, "scripts"))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import models.nca_gaussian_decoder as ncm  # noqa: E402  (the reference, read-only)
import nca_checker as nc  # noqa: E402

torch.set_num_threads(8)
META = dict(torch=torch.__version__, numpy=np.__version__, device="cpu")
MIN_GAP = 5e-4


@contextlib.contextmanager
def pinned(draws=None, record=None):
    """GDM:208's sign is +1; torch.rand replays `draws` (a list, consumed front to back) or records into `record`."""
    randn_like, rand = torch.randn_like, torch.rand
    torch.randn_like = lambda t, **kw: torch.ones_like(t)

    def patched_rand(*size, **kw):
        if draws is not None:
            return draws.pop(0).clone()
        u = rand(*size, **kw)
        if record is not None:
            record.append(u.clone())
        return u

    torch.rand = patched_rand
    try:
        yield
    finally:
        torch.randn_like, torch.rand = randn_like, rand


def make_model(ctor, seed, init_gain, rule_std):
    torch.manual_seed(seed)
    model = ncm.NCAGaussianDecoder(**ctor)
    with torch.no_grad():
        model.init_state_net[-1].weight.mul_(init_gain)
        model.init_state_net[-1].bias.copy_(torch.randn_like(model.init_state_net[-1].bias) * 0.5)
        model.update_rule[-1].weight.copy_(torch.randn_like(model.update_rule[-1].weight) * rule_std)
        model.update_rule[-1].bias.copy_(torch.randn_like(model.update_rule[-1].bias) * 0.1)
    return model


def run_once(model, inputs, n_steps, training, dtype, ups=None, draws=None):
    """One forward + backward of the reference in `dtype`.  -> dict of tensors (traj, nbr, out.*, grad.*), ups, recorded draws."""
    model = model.to(dtype).train(training)
    model.zero_grad(set_to_none=True)
    kw = {k: v.detach().to(dtype) for k, v in inputs.items()}
    kw["features"].requires_grad_(True)
    lists, record = [], []
    gather = model._gather_neighbors

    def spy(state, neighbor_idx):
        lists.append(neighbor_idx.clone())
        return gather(state, neighbor_idx)

    model._gather_neighbors = spy
    try:
        with pinned(draws=None if draws is None else [u.clone() for u in draws], record=record):
            out = model(**kw, n_steps=n_steps, return_trajectory=True)
            traj = out.pop("trajectory")
            if ups is None:
                g = torch.Generator().manual_seed(977)
                ups = {k: torch.randn(v.shape, generator=g) for k, v in out.items()}
            sum((out[k] * ups[k].to(dtype)).sum() for k in out).backward()
    finally:
        del model._gather_neighbors
    rec = {"traj": torch.stack(traj), "nbr": torch.stack(lists), "grad.features": kw["features"].grad}
    for k, p in model.named_parameters():
        rec["grad.sd." + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    for k, v in out.items():
        rec["out." + k] = v.detach()
    return rec, ups, record


def decided(rec32, rec64, k):
    """(every list agrees with the canonical one in both precisions, the smallest float64 gap over all steps)."""
    steps = rec32["nbr"].shape[0]
    ok, gap = True, float("inf")
    for s in range(steps):
        canon = nc.neighbors(rec32["traj"][s], k)
        ok = ok and torch.equal(canon, rec32["nbr"][s]) and torch.equal(canon, rec64["nbr"][s])
        gap = min(gap, float(nc.relative_gaps(rec64["traj"][s], k).min()))
    return ok, gap


def plausible(model, inputs, n_steps, training, k):
    """A cheap look before the two full runs (about one seed in a few thousand meets condition (c) over 8 steps: the smallest of
    ~2700 relative gaps of a 3-D cloud is rarely above 5e-4): the float32 forward alone, its gaps against 0.8 MIN_GAP.  The
    float64 states are within 2e-6 of these, which moves a relative gap by ~1e-5: no seed that meets the condition is lost."""
    state = torch.get_rng_state()
    with torch.no_grad(), pinned():
        traj = model.train(training)(**inputs, n_steps=n_steps, return_trajectory=True)["trajectory"]
    torch.set_rng_state(state)  # the full run draws the same uniforms
    return all(float(nc.relative_gaps(t.double(), k).min()) >= 0.8 * MIN_GAP for t in traj[:n_steps])


def small_case(name, n_steps, training, seed0):
    ctor = dict(feature_dim=8, n_points=34, n_steps=n_steps, k_neighbors=4, hidden_dim=16)
    seed = seed0
    while True:
        model = make_model(ctor, seed, init_gain=6.0, rule_std=0.6)
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        g = torch.Generator().manual_seed(seed + 1)
        inputs = dict(features=torch.randn(2, 8, 5, 7, generator=g), depth=torch.rand(2, 1, 24, 24, generator=g))
        if not plausible(model, inputs, n_steps, training, ctor["k_neighbors"]):
            seed += 1
            if seed > seed0 + 100000:
                sys.exit(f"{name}: no seed in {seed0} ... {seed} meets the condition")
            continue
        rec32, ups, draws = run_once(model, inputs, n_steps, training, torch.float32)
        model.load_state_dict(sd)
        rec64, _, _ = run_once(model, inputs, n_steps, training, torch.float64, ups=ups, draws=draws if training else None)
        ok, gap = decided(rec32, rec64, ctor["k_neighbors"])
        if ok and gap >= MIN_GAP:
            break
        seed += 1
        if seed > seed0 + 100000:
            sys.exit(f"{name}: no seed in {seed0} ... {seed} meets the condition")
    rec = dict(class_name=np.array("NCAGaussianDecoder"), ctor=np.array(json.dumps(ctor)), n_steps=np.int32(n_steps),
               training=np.int32(training), seed=np.int32(seed), min_gap=np.float64(gap))
    for k, v in sd.items():
        rec["sd." + k] = v.numpy()
    for k, v in inputs.items():
        rec["in." + k] = v.numpy()
    for k, v in ups.items():
        rec["g." + k] = v.numpy()
    if training:
        rec["uniform"] = torch.stack(draws).numpy()
    for k, v in rec32.items():
        rec[k] = v.numpy().astype(np.int16) if k == "nbr" else v.float().numpy()
    for k, v in rec64.items():
        rec["f64." + k] = v.numpy().astype(np.int16) if k == "nbr" else v.numpy()
    for k, v in META.items():
        rec["meta_" + k] = np.array(v)
    move = float((rec32["traj"][-1][..., :2] - rec32["traj"][0][..., :2]).abs().max())
    return rec, f"seed {seed}, smallest fp64 gap {gap:.2e}, largest x/y move {move:.3f}"


def default_case():
    ctor = dict(n_points=377, k_neighbors=6)
    model = make_model(ctor, 1400, init_gain=4.0, rule_std=0.15).eval()
    g = torch.Generator().manual_seed(1401)
    features, depth = torch.randn(2, 384, 37, 37, generator=g), torch.rand(2, 1, 64, 64, generator=g)
    lists = []
    gather = model._gather_neighbors
    model._gather_neighbors = lambda state, idx: (lists.append(idx.clone()), gather(state, idx))[1]
    with torch.no_grad(), pinned():
        traj = model(features, depth, n_steps=16, return_trajectory=True)["trajectory"]
    at = [0, 5, 10, 15]
    rec = dict(ctor=np.array(json.dumps(ctor)), steps=np.array(at, np.int32), states=torch.stack([traj[s] for s in at]).numpy(),
               nbr=torch.stack([lists[s] for s in at]).numpy().astype(np.int16))
    for k, v in META.items():
        rec["meta_" + k] = np.array(v)
    move = float((traj[-1][..., :2] - traj[0][..., :2]).abs().max())
    return rec, f"largest x/y move {move:.3f}"


def main():
    for name, (rec, note) in (("NCA1_eval34", small_case("NCA1", 4, False, 0)), ("NCA2_train34", small_case("NCA2", 8, True, 0)),
                              ("NCA3_default377", default_case())):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **rec)
        print(f"{name}: {note}, {os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
