"""The seeded random parity sweeps as tests: 840 scenes in seven families (tests/fuzz_cases.py), the HIP renderers against the CPU
oracle computed in the same run in fp32 and fp64 (tests/sweep_support.py).

GPU part (`-m gpu`): one test per (family, seed), 38 in all.  Each runs all its cases -- image, depth, every gradient, the phase
gradient and dL/dlambda where the renderer has them; on the blend path also the integer stages, bit-exact, at the case's own radius
cap, principal point, tile width and cameras -- and fails at the end with every failing case listed in the line format of
profiles/random_sweeps_pytest.txt, so that a failure names a scene (family, seed, iteration) that tests/golden/make_goldens.py
--kinks-only can turn into a fixture.  A last test bounds how many cases may pass through the referee rule alone.  The run writes its
record to build/random_sweeps_pytest.txt (git-ignored), or to the file that the environment variable FGS_SWEEP_RECORD names.

CPU part (no marker): the harness judged by itself -- with the fp32 oracle in the HIP side's place every case is `ok`; with that
stand-in wrong in one of eight ways a wiring or kernel error would make it wrong, some case fails; the rule on synthetic tensors; the
generators' draws pinned to the committed records."""
import os
import types

import numpy as np
import pytest

import sweep_support as S
from helpers import REFEREE_FACTOR, ROOT

# ----------------------------------------------------------------------------------------------------------------------------
# CPU part: the harness with the fp32 oracle standing in for the HIP side
# ----------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}  # (family, seed) -> {it: (o32, o64, stage records, seconds)}: computed once, shared by the CPU tests


def _oracle_of(family, seed):
    if (family, seed) not in _ORACLE:
        _ORACLE[(family, seed)] = {c["it"]: S.oracle_both(family, c) + (0.0,) for c in S.cases(family, seed)}
    return _ORACLE[(family, seed)]


def _stages_as_hip(records, W, H, tile_w):
    """Oracle stage records laid out as hip_stages returns the HIP forward's: packed records, depth keys, order, ranges, one list."""
    from oracle import fgs_oracle as orc
    Bn, N = len(records), records[0]["N"]
    rec = np.zeros((Bn, N, 12), np.float32)
    bits = rec.view(np.uint32)
    key = np.full((Bn, N), 0xFFFFFFFF, np.uint32)
    order = np.zeros((Bn, N), np.int32)
    ranges, dup = [], []
    for b, r in enumerate(records):
        vis = r["visible"].astype(bool)
        rec[b, :, 0:2], rec[b, :, 9] = r["mean2d"], r["depth"]
        bb = r["bbox"].astype(np.uint32)
        bits[b, :, 10], bits[b, :, 11] = bb[:, 0] | (bb[:, 1] << 16), bb[:, 2] | (bb[:, 3] << 16)
        key[b, vis] = np.ascontiguousarray(r["depth"][vis]).view(np.uint32)
        order[b] = np.concatenate([r["vis_sorted"], np.flatnonzero(~vis)])
        ro, ids = orc.tile_lists(r["vis_sorted"], r["bbox"], W, H, 16, tile_w=tile_w)
        off = sum(len(d) for d in dup)
        ranges.append(np.stack([ro[:-1], ro[1:]], 1) + off)
        dup.append(ids + b * N)
    return dict(rec=rec, depth_key=key.view(np.int32), order=order, ranges=np.stack(ranges).astype(np.int32),
                dup_ids=np.concatenate(dup).astype(np.int32), layout=types.SimpleNamespace(tile_w=tile_w))


class _StandIn:
    """The fp32 oracle in the HIP side's place.  `mutate(c)` changes the case it is given (a wiring error: it renders something else
    than it was asked to), `damage(c, out)` its tensors and `damage_stages(st)` its integer stages (a kernel error)."""

    def __init__(self, mutate=None, damage=None, damage_stages=None):
        self.mutate, self.damage, self.damage_stages = mutate, damage, damage_stages

    def hip(self, family, c):
        c2 = dict(c)
        self._records = [] if family in S.INTEGER_FAMILIES else None
        if self.mutate is not None:
            self.mutate(c2)
        out = S.oracle_case(family, c2, False, self._records)
        if self.damage is not None:
            self.damage(c, out)
        return out

    def stages(self, family, c):
        W, H = (c["S"], c["S"]) if "S" in c else (c["W"], c["H"])
        st = _stages_as_hip(self._records, W, H, c.get("tile_w") or 16)
        if self.damage_stages is not None:
            self.damage_stages(st)
        return st


def _harness(family, seed, stand_in):
    table = _oracle_of(family, seed)
    return S.run_seed(family, seed, lambda c: table[c["it"]], stand_in.hip, stand_in.stages)


def _failing(results):
    return [r for r in results if r["verdict"] == "FAIL"]


RIGHT = [("blend", 0), ("blend", 1), ("batch", 0), ("phase", 0)]


@pytest.mark.parametrize("family,seed", RIGHT)
def test_harness_passes_a_right_implementation(family, seed):
    results = _harness(family, seed, _StandIn())
    assert len(results) == S.N_ITER[family]
    assert [r["verdict"] for r in results] == ["ok"] * len(results), "\n".join(r["line"] for r in results if r["verdict"] != "ok")


def _blend_with(mutate=None, damage=None, damage_stages=None, select=lambda c: True):
    """Failing-case lines of blend seeds 0-1 under one deliberate error, over the cases that `select` keeps."""
    lines = []
    for seed in (0, 1):
        keep = {c["it"] for c in S.cases("blend", seed) if select(c)}
        res = _harness("blend", seed, _StandIn(mutate, damage, damage_stages))
        lines += [r["line"] for i, r in enumerate(res) if i in keep and r["verdict"] == "FAIL"]
    return lines


def test_harness_sees_an_ignored_principal_point():
    def centre(c):
        c["cx"], c["cy"] = c["W"] / 2, c["H"] / 2
    assert _blend_with(mutate=centre)


def test_harness_sees_a_radius_cap_left_at_64():
    def cap64(c):
        c["maxr"] = 64.0
    assert _blend_with(mutate=cap64, select=lambda c: c["maxr"] in (8.0, 20.0)), "no case whose cap of 8 or 20 binds failed"


def test_harness_sees_swapped_background_channels():
    def swap(c):
        c["bg"] = (c["bg"][1], c["bg"][0], c["bg"][2])
    assert _blend_with(mutate=swap)


def test_harness_sees_a_phase_amplitude_off_by_four_per_cent():
    def amp(c):
        c["amp"] = c["amp"] * 1.04
    assert _failing(_harness("phase", 0, _StandIn(mutate=amp)))


def test_harness_sees_per_image_cameras_rotated_by_one_image():
    def rotate(c):
        c["poses"] = c["poses"][1:] + c["poses"][:1]
    res = _harness("batch", 0, _StandIn(mutate=rotate))
    bad = _failing(res)
    assert bad
    single = [r for r, c in zip(res, S.cases("batch", 0)) if c["B"] == 1]
    assert all(r["verdict"] == "ok" for r in single)  # (one image: the rotation changes nothing, and nothing is reported)


def test_harness_sees_a_gradient_scaled_by_3e_4():
    def scale(c, out):
        out["colors"] = out["colors"] * np.float32(1 + 3e-4)
    lines = _blend_with(damage=scale)
    assert lines and all("colors" in ln for ln in lines)


def test_harness_sees_one_nan_in_one_gradient():
    def nan(c, out):
        out["scales"] = out["scales"].copy()
        out["scales"].flat[out["scales"].size // 2] = np.nan
    lines = _blend_with(damage=nan)
    assert len(lines) == 80 and all("non-finite" in ln for ln in lines)  # every case, before any tolerance


def test_harness_sees_two_exchanged_entries_of_one_tile_list():
    def exchange(st):
        rg = st["ranges"][0]
        for s, e in rg:
            if e - s >= 2:
                st["dup_ids"][[s, s + 1]] = st["dup_ids"][[s + 1, s]]
                return
    lines = _blend_with(damage_stages=exchange)
    assert lines and all("integer stages, image 0: tile" in ln and "list differs" in ln for ln in lines)
    # the tensors of those cases are untouched: the integer-stage check alone fails them
    assert all("vs-fp32" not in ln for ln in lines)


def test_oracle_workers_match_the_inline_oracle_and_stay_off_the_gpu():
    """The worker processes give what the inline oracle gives (same draws from the seed, same tensors bit for bit), and
    _oracle_job itself asserts that the worker has neither initialised a device nor loaded the HIP library."""
    pool = S.OraclePool([("batch", 0)], workers=2)
    try:
        table = _oracle_of("batch", 0)
        for it in (0, 5, 15):
            o32, o64, stages, _ = pool.get("batch", 0, it)
            for k in o32:
                assert np.array_equal(o32[k], table[it][0][k]) and np.array_equal(o64[k], table[it][1][k]), (it, k)
            assert len(stages) == len(table[it][2])
    finally:
        pool.close()


# ---- the rule on synthetic tensors -----------------------------------------------------------------------------------------
def _synthetic():
    ref = np.linspace(-1.0, 1.0, 101)  # max |ref| = 1: relative and absolute errors coincide
    return ref, np.eye(1, 101, 7)[0], np.eye(1, 101, 60)[0]


def test_rule_exact_result_is_ok():
    ref, _, _ = _synthetic()
    v = S.sweep_verdict(ref.astype(np.float32), ref.astype(np.float32), ref.astype(np.float32))
    assert v["ok"] and v["via"] == "plain" and v["e32"] == 0


def test_rule_3e_4_with_no_spread_fails():
    ref, e1, _ = _synthetic()
    v = S.sweep_verdict(ref + 3e-4 * e1, ref, ref)
    assert not v["ok"] and v["via"] == "FAIL" and not v["use64"] and v["tol"] == 1e-4


def test_rule_referee_passes_inside_factor_times_spread_and_not_beyond():
    ref, e1, e2 = _synthetic()
    o64, o32 = ref, ref + 2e-4 * e1
    inside = 0.9 * REFEREE_FACTOR * 2e-4
    v = S.sweep_verdict(o64 + inside * e2, o32, o64)
    assert v["ok"] and v["via"] == "referee" and v["use64"] and v["e32"] > 1e-4 and v["e64"] > 1e-4
    assert abs(v["tol"] - REFEREE_FACTOR * 2e-4) < 1e-12
    assert not S.sweep_verdict(o64 + 1.1 * REFEREE_FACTOR * 2e-4 * e2, o32, o64)["ok"]
    # the same error where the oracle's two runs are 4e-5 apart: the rule does not apply
    v = S.sweep_verdict(o64 + inside * e2, ref + 4e-5 * e1, o64)
    assert not v["ok"] and not v["use64"]


def test_rule_either_oracle_run_at_1e_4_passes_as_plain():
    """`blend s6 it 38`: fp32 oracle and implementation exactly 0, the fp64 run not (spread 1.0) -- plain, not the referee's."""
    o64 = np.array([0.0, 3e-7, -1e-7])
    v = S.sweep_verdict(np.zeros(3, np.float32), np.zeros(3, np.float32), o64)
    assert v["ok"] and v["via"] == "plain" and v["use64"] and v["e64"] == 1.0
    ref, e1, _ = _synthetic()
    assert S.sweep_verdict(ref + 2e-4 * e1, ref + 2.5e-4 * e1, ref)["via"] == "plain"  # 5e-5 from the fp32 run, 2e-4 from the fp64 run


def test_rule_nan_fails_before_any_tolerance():
    ref, _, _ = _synthetic()
    x = ref.copy()
    x[3] = np.nan
    for form in ("rel", "abs", "wavelength"):
        v = S.sweep_verdict(x, ref, ref, form)
        assert not v["ok"] and v["via"] == "non-finite"
    x[3] = np.inf
    assert not S.sweep_verdict(x, ref, ref)["ok"]


def test_rule_wavelength_gradient_with_a_nan_reference_channel_is_judged_in_fp64():
    o64 = np.array([-3.0, 2.0, 0.5])
    o32 = np.array([-3.0, np.nan, 0.5])
    good = S.sweep_verdict(o64.copy(), o32, o64, "wavelength")
    assert good["ok"] and good["use64"]
    off = o64.copy()
    off[1] += 3e-4 * 3.0  # wrong in the very channel the fp32 reference cannot judge
    v = S.sweep_verdict(off, o32, o64, "wavelength")
    assert not v["ok"] and v["e64"] == pytest.approx(3e-4)
    # and a finite fp32 reference is a reference like any other
    assert S.sweep_verdict(o64 * (1 + 5e-5), o64.copy(), o64, "wavelength")["via"] == "plain"
    assert not S.sweep_verdict(o64 * (1 + 3e-4), o64.copy(), o64, "wavelength")["ok"]


def test_rule_absolute_form_ignores_the_scale_of_the_image():
    img = np.full((3, 4, 4), 0.01)
    assert not S.sweep_verdict(img + 2e-4, img, img, "abs")["ok"]
    assert S.sweep_verdict(img + 5e-5, img, img, "abs")["ok"]  # (relative to max this would be 5e-3)


def test_excluded_phase_gradient_must_still_be_finite():
    c = next(c for c in S.cases("asm", 0) if c["N"] == 1)
    assert "phases" not in S.compared_tensors("asm", c)
    names = S.compared_tensors("asm", c)
    o = {k: np.ones(3) for k in names}
    ok = S.judge_case("asm", 0, c, dict(o, phases=np.array([123.0])), o, o)
    assert ok["verdict"] == "ok"
    bad = S.judge_case("asm", 0, c, dict(o, phases=np.array([np.nan])), o, o)
    assert bad["verdict"] == "FAIL" and "non-finite" in bad["line"]


# ---- the draws are pinned --------------------------------------------------------------------------------------------------
def _case(family, seed, it):
    return next(c for c in S.cases(family, seed) if c["it"] == it)


def test_named_cases_are_the_scenes_of_the_committed_records():
    """The cases that became fixtures (profiles/r05_fuzz_sweeps.txt): a reordered statement in tests/fuzz_cases.py moves them."""
    c = _case("phase", 2, 12)
    assert (c["W"], c["H"], c["N"], c["amp"]) == (145, 66, 17, 0.45)
    c = _case("phase", 1, 23)
    assert (c["W"], c["H"], c["N"], c["amp"]) == (113, 54, 65, 0.45)
    c = _case("asm", 0, 4)
    assert (c["W"], c["H"], c["N"], c["P"], c["kind"], c["rgbph"]) == (96, 40, 700, 16, "asm", False) and c["phases"].shape == (700,)
    c = _case("blend", 6, 38)
    assert (c["W"], c["H"], c["N"], c["smax"], c["tile_w"]) == (13, 26, 1, 0.02, 32)
    c = _case("blend_big", 0, 3)
    assert (c["W"], c["H"], c["N"], c["smax"], c["tile_w"], c["tuning"]) == (270, 270, 4000, 0.03, 16, {"tile_w": 16})


def test_family_sizes_are_pinned():
    its = {(f, s): [c["it"] for c in S.cases(f, s)] for f, s in S.FAMILY_SEEDS}
    sizes = {f: sum(len(v) for (ff, _), v in its.items() if ff == f) for f in S.FAMILIES}
    assert sizes == dict(phase=240, blend=320, blend_big=24, batch=48, batch_wide=48, asm=112, asm_batched=48)
    assert sum(sizes.values()) == 840 and len(S.FAMILY_SEEDS) == 38
    for (f, s), v in its.items():  # the oracle jobs cover every case exactly once
        assert [it for job in S.oracle_jobs(f, s) for it in range(job[2], job[3])] == v


# ----------------------------------------------------------------------------------------------------------------------------
# the tally and the cap on the referee rule
# ----------------------------------------------------------------------------------------------------------------------------
def _new_tally():
    return dict(reported=set(), cases=0, verdicts={}, referee_only=[], oracle_needs=[], seconds={})


def check_tally(tally, narrowed):
    """The cap: over the run, the cases that pass ONLY through the referee rule (`ok-referee`) must not outnumber the cases whose
    oracle fp32 run is itself further than 1e-4 from its fp64 run in some compared tensor -- both counted in this run.  A run that was
    not narrowed must have heard from all 38 (family, seed) tests: the cap over a partial tally would pass vacuously."""
    if not narrowed:
        missing = [p for p in S.FAMILY_SEEDS if p not in tally["reported"]]
        assert not missing, f"{len(missing)} of 38 (family, seed) tests did not report: {missing}"
        assert tally["cases"] == 840, f"{tally['cases']} cases reported, not 840"
    assert len(tally["referee_only"]) <= len(tally["oracle_needs"]), (
        f"{len(tally['referee_only'])} cases pass only through the referee rule, but the oracle's own fp32 run needs it for "
        f"{len(tally['oracle_needs'])}: {tally['referee_only']}")


def test_cap_fails_on_a_partial_tally_and_on_too_many_referee_verdicts():
    t = _new_tally()
    t["reported"].update(S.FAMILY_SEEDS[:37])
    t["cases"] = 816
    check_tally(t, narrowed=True)
    with pytest.raises(AssertionError, match="did not report"):
        check_tally(t, narrowed=False)
    t["reported"].update(S.FAMILY_SEEDS)
    t["cases"] = 840
    t["oracle_needs"] = ["asm s0 it 2"]
    t["referee_only"] = ["asm s0 it 2"]
    check_tally(t, narrowed=False)
    t["referee_only"].append("phase s2 it 12")
    with pytest.raises(AssertionError, match="only through the referee rule"):
        check_tally(t, narrowed=False)


# ----------------------------------------------------------------------------------------------------------------------------
# GPU part
# ----------------------------------------------------------------------------------------------------------------------------
TALLY = _new_tally()
_DIED = []  # a sweep test whose HIP side raised: no further GPU work is started after that
RECORD = os.environ.get("FGS_SWEEP_RECORD") or os.path.join(ROOT, "build", "random_sweeps_pytest.txt")


@pytest.fixture(scope="module")
def sweep_run(request):
    """Oracle jobs of every selected (family, seed) submitted up front to CPU-only workers; the run's record file."""
    pairs = [(it.callspec.params["family"], it.callspec.params["seed"]) for it in request.session.items
             if getattr(it, "module", None) is request.module and it.name.startswith("test_sweep[")]
    S.cuda_device()
    from fresnel_amd import _binding
    os.makedirs(os.path.dirname(os.path.abspath(RECORD)), exist_ok=True)
    f = open(RECORD, "w")

    def emit(s):
        f.write(s + "\n")
        f.flush()

    emit("# randomized sweeps, HIP vs the CPU oracle computed in the same run in fp32 and fp64; tests/test_random_sweeps.py")
    emit(f"# library: {_binding.load().fgs_version().decode()}")
    emit("# per case: verdict | worst tensor by (error / tolerance) | error vs the run that referees it | tolerance | the oracle's own "
         "fp32-vs-fp64 spread | largest distance from the nearer oracle run over all tensors | seconds of the HIP side")
    emit("# verdicts: ok = every tensor finite and <= 1e-4 of max from the fp32 oracle or from its fp64 run, integer stages bit-exact (blend "
         "path); ok-referee = some tensor is > 1e-4 from both, the oracle's own runs are > 5e-5 apart there and the HIP result is inside "
         "tests/helpers.referee_tolerance(spread) of the fp64 run; FAIL = neither, a non-finite value, or an integer stage that differs")
    pool = S.OraclePool(pairs)
    try:
        yield types.SimpleNamespace(pool=pool, emit=emit)
    finally:
        pool.close()
        f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("family,seed", S.FAMILY_SEEDS, ids=[f"{f}-s{s}" for f, s in S.FAMILY_SEEDS])
def test_sweep(family, seed, sweep_run):
    """All cases of one (family, seed): every compared tensor by S.sweep_verdict, every HIP tensor finite, and on the blend path
    the integer stages bit-exact.  No case is skipped or excused; every failing case is listed."""
    import time
    if _DIED:
        pytest.fail(f"not started: the HIP side raised in {_DIED[0]}")
    sweep_run.emit(f"== {family} seed {seed}")
    t0 = time.time()
    try:
        results = S.run_seed(family, seed, lambda c: sweep_run.pool.get(family, seed, c["it"]), S.hip_case, S.hip_case_stages, sweep_run.emit)
    except RuntimeError as e:
        _DIED.append(f"{family} s{seed}")
        sweep_run.emit(f"CRASH      {e}")
        raise
    TALLY["reported"].add((family, seed))
    TALLY["cases"] += len(results)
    TALLY["seconds"][(family, seed)] = time.time() - t0
    for r, c in zip(results, S.cases(family, seed)):
        TALLY["verdicts"][r["verdict"]] = TALLY["verdicts"].get(r["verdict"], 0) + 1
        name = f"{family} s{seed} it {c['it']}"
        if r["verdict"] == "ok-referee":
            TALLY["referee_only"].append(name)
        if r["needs"]:
            TALLY["oracle_needs"].append(name)
    assert len(results) == S.N_ITER[family]
    bad = [r["line"] for r in results if r["verdict"] == "FAIL"]
    assert not bad, f"{len(bad)} of {len(results)} cases fail:\n" + "\n".join(bad)


@pytest.mark.gpu
def test_referee_rule_decides_no_more_cases_than_the_oracle_needs(request, sweep_run):
    opt = request.config.option
    narrowed = bool(opt.keyword) or bool(getattr(opt, "deselect", None)) or any("::" in a for a in request.config.args)
    t = TALLY
    sweep_run.emit("# tally: " + ", ".join(f"{k} {v}" for k, v in sorted(t["verdicts"].items())) +
                   f"; {t['cases']} cases of {len(t['reported'])} (family, seed) tests" + ("; narrowed run" if narrowed else ""))
    sweep_run.emit(f"# passing only through the referee rule: {len(t['referee_only'])} ({', '.join(t['referee_only']) or 'none'})")
    sweep_run.emit(f"# oracle's own fp32 run > 1e-4 from its fp64 run in some compared tensor: {len(t['oracle_needs'])} cases (the cap)")
    sweep_run.emit("# seconds per family (HIP side and waiting for the oracle): " + ", ".join(
        f"{f} {sum(v for (ff, _), v in t['seconds'].items() if ff == f):.0f}" for f in S.FAMILIES))
    check_tally(t, narrowed)
