"""Shared inputs of the GaussianMatchingLoss tests (test_match_checker.py, test_match_mirror.py, test_hip_match.py,
test_workspace_hygiene_match.py): the reference fixtures tests/golden/match_M{1,2,3}.npz, the comparison against them under the
project's parity rule, and the seeded clouds of the GPU cases."""
import contextlib
import json
import os

import numpy as np
import torch

import match_checker as mc
from helpers import GOLDEN, rel_to_max

FIXTURES = ("match_M1", "match_M2", "match_M3")
OUT_KEYS = ("total",) + mc.KEYS
TOL = 1e-4
_CACHE = {}


def fixture(name):
    if name not in _CACHE:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
            fx = {k: z[k] for k in z.files}
        fx["ctor"] = json.loads(str(fx["ctor"]))
        fx["draws"] = [fx[f"draw_{n}"] for n in range(sum(k.startswith("draw_") for k in fx))]
        _CACHE[name] = fx
    return _CACHE[name]


def fixture_weights(fx):
    """The six weights of a fixture's constructor, as match_checker's dict (the reference's defaults where not given)."""
    return {k: fx["ctor"].get(k + "_weight", mc.WEIGHTS[k]) for k in mc.KEYS}


def fixture_masks(fx):
    """The masks that stand for a fixture's selection: the caller's own masks (the zero-padding filter is then the checker's to
    apply), or, where the reference subsampled, the rows its recorded draws kept."""
    if fx["draws"]:
        return fx["pred_keep"], fx["target_keep"]
    return fx.get("pred_mask"), fx.get("target_mask")


def out_of(ev):
    """The module's seven values from a checker (or kernel) evaluation: total, and the components of the last non-skipped image."""
    live = [b for b in range(len(ev["counts"])) if ev["counts"][b, 0] > 0 and ev["counts"][b, 1] > 0]
    last = ev["terms"][live[-1]] if live else np.zeros(8)
    out = {"total": ev["total"]}
    out.update({k: last[i] for i, k in enumerate(mc.KEYS)})
    return out


def fixture_errors(fx, out, grad, prefix):
    """{name: error relative to the tensor's max} of the seven values and the gradient against the reference's run `prefix`
    ("" = float32, "f64." = float64)."""
    err = {k: rel_to_max(np.float64(out[k]), np.float64(fx[prefix + "out." + k])) for k in OUT_KEYS}
    err["grad"] = rel_to_max(np.asarray(grad, np.float64), fx[prefix + "grad"].astype(np.float64))
    return err


def checker_on_fixture(fx, **mutation):
    """match_checker on a fixture's inputs.  -> the evaluation, and the worst error over both runs."""
    ev = mc.evaluate(fx["pred"], fx["target"], *fixture_masks(fx), fixture_weights(fx), **mutation)
    worst = max(max(fixture_errors(fx, out_of(ev), ev["grad"], p).values()) for p in ("", "f64."))
    return ev, worst


@contextlib.contextmanager
def replayed_randperm(draws):
    """torch.randperm hands out the recorded draws, front to back."""
    real, left = torch.randperm, [torch.from_numpy(np.asarray(d)) for d in draws]

    def patched(n, **kw):
        d = left.pop(0)
        assert d.numel() == n, "the mirror draws in another order than the reference"
        return d.clone()

    torch.randperm = patched
    try:
        yield left
    finally:
        torch.randperm = real


# ---- seeded clouds ----------------------------------------------------------------------------------------------------------
def cloud(rs, Bn, N, spread=1.0):
    rows = np.empty((Bn, N, 14), np.float32)
    rows[..., 0:3] = rs.uniform(-spread, spread, (Bn, N, 3))
    rows[..., 3:6] = rs.uniform(0.01, 0.3, (Bn, N, 3))
    rows[..., 6:10] = rs.standard_normal((Bn, N, 4))
    rows[..., 10:13] = rs.uniform(0, 1, (Bn, N, 3))
    rows[..., 13] = rs.uniform(0.05, 1, (Bn, N))
    return rows


def random_case(seed, Bn, Np, Nt):
    rs = np.random.RandomState(seed)
    return cloud(rs, Bn, Np), cloud(rs, Bn, Nt)


def lattice_case(seed=5):
    """A 5 x 5 x 3 integer lattice against a copy shifted by (0.5, 0.5, 0): every interior point has four nearest candidates at
    d2 = 0.5 exactly.  The second image holds the same rows in another order, so the index decides differently."""
    rs = np.random.RandomState(seed)
    grid = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    pred, target = cloud(rs, 2, 75), cloud(rs, 2, 75)
    pred[0, :, :3], target[0, :, :3] = grid, grid + np.float32([0.5, 0.5, 0.0])
    pp, tp = rs.permutation(75), rs.permutation(75)
    pred[1], target[1] = pred[0, pp], target[0, tp]
    return pred, target


def coincident_case(seed=6):
    """Coincident points: groups of targets on one spot (d2 = 0 from the prediction sitting there to several candidates)."""
    rs = np.random.RandomState(seed)
    pred, target = cloud(rs, 1, 20), cloud(rs, 1, 60)
    target[0, :, :3] = pred[0, np.arange(60) % 20, :3]  # three targets on every prediction
    target[0, 40:, :3] = pred[0, 3, :3]                 # and twenty more on prediction 3
    pred[0, 10, :3] = pred[0, 3, :3]                    # two predictions on one spot as well
    return pred, target


def hub_case(seed=7, Np=65, Nt=3000):
    """Prediction 17 is the nearest of all 3000 targets; every other prediction has in-degree 0."""
    rs = np.random.RandomState(seed)
    pred, target = cloud(rs, 1, Np), cloud(rs, 1, Nt, spread=0.2)
    pred[0, :, :3] += np.float32([5.0, 5.0, 5.0])
    pred[0, 17, :3] = 0.01
    return pred, target


def skipping_case(seed=8):
    """A batch of three: image 0 has no active prediction (all masked), image 2 no active target (zero padding throughout)."""
    pred, target = random_case(seed, 3, 70, 130)
    pk, tk = np.ones((3, 70), np.uint8), np.ones((3, 130), np.uint8)
    pk[0] = 0
    pk[1, ::7] = 0
    tk[1, 5:20] = 0
    target[2] = 0.0
    pred[1, 60:] = 0.0
    return pred, target, pk, tk


def filter_seam_case(seed=9):
    """|x| + |y| + |z| and |opacity| exactly on 1e-6f (inactive) and one ulp above (active), the other quantity at 0."""
    pred, target = random_case(seed, 1, 12, 12)
    t, up = np.float32(1e-6), np.nextafter(np.float32(1e-6), np.float32(1))
    for rows in (pred, target):
        rows[0, :4, :3], rows[0, :4, 13] = 0.0, 0.0
        rows[0, 0, 0] = t                       # inactive: the sum is exactly 1e-6f
        rows[0, 1, 0] = -up                     # active
        rows[0, 2, 13] = -t                     # inactive
        rows[0, 3, 13] = up                     # active
    return pred, target


def quaternion_case(seed=10):
    """Matched pairs (prediction i sits next to target i) with a zero quaternion, one of norm 1e-9 (both under the 1e-8 clamp), a
    pair with dot exactly 0, and a zero TARGET quaternion."""
    rs = np.random.RandomState(seed)
    pred, target = cloud(rs, 1, 8), cloud(rs, 1, 8)
    pred[0, :, :3] = np.arange(8, dtype=np.float32)[:, None] * 3
    target[0, :, :3] = pred[0, :, :3] + np.float32(0.25)
    pred[0, 0, 6:10] = 0.0
    pred[0, 1, 6:10] = (1e-9, 0, 0, 0)
    pred[0, 2, 6:10], target[0, 2, 6:10] = (1, 0, 0, 0), (0, 1, 0, 0)
    target[0, 3, 6:10] = 0.0
    return pred, target


def nan_inf_case(seed=11):
    pred, target = random_case(seed, 2, 40, 50)
    pred[0, 3, 0] = np.nan
    pred[0, 7, :3] = np.inf
    target[0, 5, 1] = -np.inf
    target[0, 9, 13] = np.nan
    target[1, 4, :3] = np.nan
    pred[1, 2, 13] = np.nan
    pred[1, 2, :3] = 0.0  # inactive: a NaN opacity compares false and the position is zero
    return pred, target
