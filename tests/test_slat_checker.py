"""tests/slat_checker.py against the reference's fixtures S1-S4 in fp32 and fp64, and six wrong rules, each of which must make the
comparison fail by at least 10 x the tolerance.

What that shows differs by rule.  `no_abs`, `div63`, `no_coord_clamp` and `clamp_first` are noticed by the REFERENCE's recorded values
of S1.  `open_gate` and `no_norm_floor` cannot be: the seed rule keeps every fixture element 1e-3 away from +-10 and every quaternion
norm above 1e-3, so no recorded value depends on them.  For those two the test moves raw onto the gate / below the floor and takes
the expected values from the checker's own right rule: it shows that the switch changes the checker where it should, not that the
fixtures hold the rule.  The closed gate and the norm floor themselves are held by the GPU seam tests
(tests/test_hip_slat.py test_raw_on_and_one_ulp_outside_the_gate, test_quaternion_norm_floor) and by the reference's source."""
import numpy as np
import pytest
import torch

import slat_checker as sc
from helpers import rel_to_max
from test_decoder_mirror import TOL
from test_slat_mirror import FIXTURES, fixture


def _head_case(fx, dtype):
    raw = torch.from_numpy(fx["raw"]).to(dtype).requires_grad_(True)
    pg = torch.from_numpy(fx["sd.gaussian_head.position_offset_scale"]).to(dtype).requires_grad_(True)
    sf = torch.from_numpy(fx["sd.gaussian_head.scale_factor"]).to(dtype).requires_grad_(True)
    return raw, torch.from_numpy(fx["in.coords"]), pg, sf


def _errors(fx, dtype, wrong=None):
    """-> {what: distance from the fixture relative to its maximum}: the output, dL/d raw and the two gain gradients."""
    raw, coords, pg, sf = _head_case(fx, dtype)
    out = sc.head(raw, coords, pg, sf, wrong=wrong)
    (out * torch.from_numpy(fx["g.gaussians"]).to(dtype)).sum().backward()
    return {"out": rel_to_max(out.detach().numpy(), fx["out.gaussians"]),
            "grad raw": rel_to_max(raw.grad.numpy(), fx["grad.raw"]),
            "grad position_offset_scale": rel_to_max(pg.grad.numpy(), fx["grad.sd.gaussian_head.position_offset_scale"]),
            "grad scale_factor": rel_to_max(sf.grad.numpy(), fx["grad.sd.gaussian_head.scale_factor"])}


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_checker_reproduces_the_reference_head(name, dtype):
    for what, e in _errors(fixture(name), dtype).items():
        assert e <= TOL, f"{name}: checker {what} is {e:.2e} of its maximum away"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_checker_reproduces_the_gated_lists(dtype):
    fx1, fx2 = fixture("slat_S1"), fixture("slat_S2")
    raw, coords, pg, sf = _head_case(fx1, dtype)   # S2 is S1's model on S1's inputs: the same raw
    keep = torch.from_numpy(fx2["out.occupancy_mask"] & fx2["in.coord_mask"])
    with torch.no_grad():
        packed, counts = sc.gated(raw, coords, pg, sf, keep)
    G = raw.shape[2]
    assert (counts * G).tolist() == fx2["out.n_gaussians"].tolist()
    for b, n in enumerate(fx2["out.n_gaussians"]):
        assert float(np.abs(packed[b, :n].numpy() - fx2[f"out.gaussians.{b}"]).max()) <= TOL
        assert not packed[b, n:].any()


# which fixture and which quantity notices a wrong rule (S1 has coordinates beyond [0, 63] and a negative scale_factor)
NOTICED_BY = {"open_gate": "grad raw", "no_abs": "out", "div63": "out", "no_coord_clamp": "out", "clamp_first": "out",
              "no_norm_floor": "out"}


@pytest.mark.parametrize("wrong", sc.WRONG)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_fixtures_notice_a_wrong_rule(wrong, dtype):
    fx = fixture("slat_S1")
    if wrong in ("open_gate", "no_norm_floor"):
        # the seed rule keeps every fixture element 1e-3 away from +-10 and every quaternion norm above 1e-3: put elements ON the
        # gate / a quaternion below the floor, and take the expected values from the right rule (held against the fixture above)
        fx = {k: fx[k] for k in fx.files}
        raw = fx["raw"].copy()
        if wrong == "open_gate":
            at = np.abs(np.abs(raw) - 10) < 2.0
            raw[at] = np.sign(raw[at]) * 10.0
        else:
            raw[:, :, 0, 6:10] = 1e-8   # norm 2e-8: the floor makes the output 0.01, without it it is 0.5
        closed, _, pg, sf = _head_case(dict(fx, raw=raw), dtype)
        want = sc.head(closed, torch.from_numpy(fx["in.coords"]), pg, sf)
        (want * torch.from_numpy(fx["g.gaussians"]).to(dtype)).sum().backward()
        fx["raw"], fx["out.gaussians"], fx["grad.raw"] = raw, want.detach().numpy(), closed.grad.numpy()
        fx["grad.sd.gaussian_head.position_offset_scale"], fx["grad.sd.gaussian_head.scale_factor"] = pg.grad.numpy(), sf.grad.numpy()
        assert all(e <= TOL for e in _errors(fx, dtype).values())
    e = _errors(fx, dtype, wrong=wrong)[NOTICED_BY[wrong]]
    assert e >= 10 * TOL, f"the fixture does not notice {wrong}: {NOTICED_BY[wrong]} is only {e:.2e} away"
