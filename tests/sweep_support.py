"""Support of the randomized parity sweeps (tests/test_random_sweeps.py) and of the GPU parity tests that share its pieces:

  * the seven sweep families over the seeded case generators of tests/fuzz_cases.py;
  * the two sides of one case -- `oracle_case` (CPU oracle, fp32 or fp64) and `hip_case` (the HIP renderers through autograd) -- with the
    same cameras and renderer arguments on both sides;
  * the integer stages of a HIP forward (`hip_stages`) and their bit-exact check against the oracle (`check_integer_stages`);
  * the verdict of one tensor (`sweep_verdict`: the referee rule of tests/helpers.py plus the sweeps' "within 1e-4 of either oracle run")
    and of one case (`judge_case`), and the record lines of profiles/random_sweeps_pytest.txt;
  * the oracle side in CPU-only worker processes (`OraclePool`).

A plain module, not a conftest: nothing here changes how tests are collected or run."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fuzz_cases as FC  # noqa: E402
from helpers import referee_tolerance, rel_to_max  # noqa: E402

TOL = 1e-4
GRADS = ["positions", "scales", "rotations", "colors", "opacities"]
FAMILIES = {  # family -> (seeds, case generator); 240 / 320 / 24 / 48 / 48 / 112 / 48 = 840 cases
    "phase": (tuple(range(10)), lambda s: FC.phase_cases(s)),
    "blend": (tuple(range(8)), lambda s: FC.blend_cases(s)),
    "blend_big": (tuple(range(4)), lambda s: FC.blend_big_cases(s)),
    "batch": (tuple(range(3)), lambda s: FC.batch_cases(s, 2)),
    "batch_wide": (tuple(range(3)), lambda s: FC.batch_cases(s, 1)),
    "asm": (tuple(range(8)), lambda s: FC.asm_cases(s)),
    "asm_batched": ((4, 5), lambda s: FC.asm_batched_cases(s)),
}
FAMILY_SEEDS = [(f, s) for f in FAMILIES for s in FAMILIES[f][0]]  # the 38 GPU tests
INTEGER_FAMILIES = ("blend", "blend_big", "batch", "batch_wide")  # blend path: the integer stages are checked bit-exact
# cases per oracle job: the expensive families go case by case so that eight workers share one seed (one asm_batched seed is about a
# minute on one core) and no result is larger than one case's tensors
CASES_PER_JOB = {"phase": 8, "blend": 10, "blend_big": 1, "batch": 4, "batch_wide": 4, "asm": 2, "asm_batched": 1}
MAX_WORKERS = 8


def cases(family, seed):
    return FAMILIES[family][1](seed)


def describe(c):
    keys = [k for k in ("W", "H", "S", "B", "N", "P", "maxr", "smax", "amp", "tile_w", "tuning", "kind", "rgbph") if k in c]
    return " ".join(f"{k}{c[k]}" if not isinstance(c[k], str) else c[k] for k in keys)


def compared_tensors(family, c):
    """Names of the tensors of one case that are compared.  The one exclusion: the phase gradient of a single-Gaussian ASM / wave
    scene (a global phase: the true gradient is 0, the ratio would be noise / noise) -- it must still be finite."""
    names = ["image"] + GRADS
    if family in ("phase", "blend", "blend_big", "batch", "batch_wide") or (family == "asm" and c["kind"] == "wave"):
        names.insert(1, "depth")
    if family == "phase" or family == "asm_batched" or (family == "asm" and c["N"] > 1):
        names.append("phases")
    if family == "asm_batched" or (family == "asm" and c["kind"] == "asm"):
        names.append("wavelengths")
    return names


def tensor_form(family, name):
    """How a tensor's error is measured: ASM / wave-field images live in [0, 1] -> absolute (as tests/test_hip_asm.py does it);
    dL/dlambda -> the wavelength-gradient form; everything else relative to the reference's maximum."""
    if name == "wavelengths":
        return "wavelength"
    if family.startswith("asm") and name == "image":
        return "abs"
    return "rel"


# ----------------------------------------------------------------------------------------------------------------------------
# oracle side (CPU)
# ----------------------------------------------------------------------------------------------------------------------------
def pose_cameras(c):
    """The orbit cameras of a batch case as plain numbers: [(view 4x4, fx, fy, cx, cy)] per image."""
    from fresnel_amd.renderer import create_camera_from_pose  # (numpy / host torch only: opens no device, loads no HIP library)
    out = []
    for el, az, dist in c["poses"]:
        cc = create_camera_from_pose(el, az, c["S"], distance=dist)
        out.append((cc.view_matrix.numpy().copy(), cc.fx, cc.fy, cc.cx, cc.cy))
    return out


def _stage_record(r):
    """What the integer-stage check needs of an oracle forward (fp32 run)."""
    p = r.proj
    return dict(N=int(r.pos.shape[0]), visible=p["visible"].copy(), bbox=p["bbox"].copy(), mean2d=p["mean2d"].copy(),
                depth=p["depth"].copy(), vis_sorted=np.asarray(r.vis_sorted).copy())


class OracleStages:
    """The `r` argument of check_integer_stages rebuilt from a _stage_record (the Rendered itself stays in the worker)."""

    def __init__(self, rec):
        self.pos = np.empty((rec["N"], 3), np.float32)
        self.proj = dict(visible=rec["visible"], bbox=rec["bbox"], mean2d=rec["mean2d"], depth=rec["depth"])
        self.vis_sorted = rec["vis_sorted"]


def oracle_case(family, c, f64, stages=None):
    """Expected tensors of one case in one precision.  `stages`: a list that receives one _stage_record per image (blend path)."""
    import contextlib
    import torch
    from oracle import asm_oracle, fgs_oracle as orc
    prec = orc.fp64() if f64 else contextlib.nullcontext()
    out = {}
    if family in ("phase", "blend", "blend_big"):
        W, H = c["W"], c["H"]
        if family == "phase":
            cam = orc.make_camera(np.eye(4), 0.8 * W, 0.8 * W, W / 2, H / 2, W, H)
            kw = dict(bg=c["bg"], phases=c["phases"], phase_amp=c["amp"])
        else:
            cam = orc.make_camera(np.eye(4), c["fx"], c["fx"], c["cx"], c["cy"], W, H)
            kw = dict(bg=c["bg"], max_radius=c["maxr"])
        with prec:
            r = orc.render(*c["arrs"], cam, **kw)
            g = orc.render_backward(r, c["gI"], c["gD"])
        if stages is not None:
            stages.append(_stage_record(r))
        rs_ = c.get("row_stride", 1)  # (big frames: every row_stride-th row of the image and depth is kept)
        out["image"], out["depth"] = r.image[:, ::rs_], r.depth[::rs_]
        for k in GRADS + (["phases"] if family == "phase" else []):
            out[k] = g[k]
    elif family in ("batch", "batch_wide"):
        S = c["S"]
        res = {k: [] for k in ["image", "depth"] + GRADS}
        for b, (view, fx, fy, cx, cy) in enumerate(c.get("cams") or pose_cameras(c)):
            cam = orc.make_camera(view, fx, fy, cx, cy, S, S)
            with prec:
                r = orc.render(*[a[b] for a in c["arrs"]], cam, bg=c["bg"])
                g = orc.render_backward(r, c["gI"][b], c["gD"][b])
            if stages is not None:
                stages.append(_stage_record(r))
            res["image"].append(r.image); res["depth"].append(r.depth)
            for k in GRADS:
                res[k].append(g[k])
        out = {k: np.stack(v) for k, v in res.items()}
    elif family == "asm":
        W, H = c["W"], c["H"]
        cam = orc.make_camera(np.eye(4), 0.8 * W, 0.8 * W, W / 2, H / 2, W, H)
        dt = torch.float64 if f64 else torch.float32
        if c["kind"] == "asm":
            kw = c["kw"]
            r = asm_oracle.render(*c["arrs"], c["phases"], c["wl"], cam, bg=c["bg"], num_planes=c["P"], depth_range=(0.1, 3.2),
                                  focal_depth=kw["focal_depth"], pixel_pitch=kw["pixel_pitch"], grad_out=c["gI"], dtype=dt, project_f64=f64)
            out["wavelengths"] = r["grad_wavelengths"]
        else:
            r = asm_oracle.render_wave(*c["arrs"], c["phases"], cam, bg=c["bg"], grad_out=c["gI"], grad_depth=c["gD"], dtype=dt, project_f64=f64)
            out["depth"] = r["depth"]
        out["image"] = r["image"]
        for k in GRADS + ["phases"]:
            out[k] = r["grad_" + k]
    elif family == "asm_batched":
        W, H, kw = c["W"], c["H"], c["kw"]
        cam = orc.make_camera(np.eye(4), c["f"], c["f"], W / 2, H / 2, W, H)
        dt = torch.float64 if f64 else torch.float32
        res = {k: [] for k in ["image"] + GRADS + ["phases"]}
        gw = 0.0
        for b in range(c["B"]):
            r = asm_oracle.render(*[a[b] for a in c["arrs"]], c["phases"][b], c["wl"], cam, bg=c["bg"], num_planes=c["P"],
                                  depth_range=kw["depth_range"], focal_depth=kw["focal_depth"], pixel_pitch=kw["pixel_pitch"],
                                  grad_out=c["gI"][b], dtype=dt, project_f64=f64)
            res["image"].append(r["image"])
            for k in GRADS + ["phases"]:
                res[k].append(r["grad_" + k])
            gw = gw + r["grad_wavelengths"].astype(np.float64)
        out = {k: np.stack(v) for k, v in res.items()}
        out["wavelengths"] = gw
    else:
        raise KeyError(family)
    keep = np.float64 if f64 else np.float32
    return {k: np.asarray(v, np.float64 if k == "wavelengths" else keep) for k, v in out.items()}


def oracle_both(family, c):
    """(fp32 tensors, fp64 tensors, stage records of the fp32 run or None) of one case."""
    stages = [] if family in INTEGER_FAMILIES else None
    o32 = oracle_case(family, c, False, stages)
    return o32, oracle_case(family, c, True), stages


# ---- worker processes: CPU only --------------------------------------------------------------------------------------------
def _worker_init():
    # the workers never touch the GPU: no device is visible to them, whatever they import
    os.environ["HIP_VISIBLE_DEVICES"] = ""
    os.environ["CUDA_VISIBLE_DEVICES"] = ""
    import torch
    torch.set_num_threads(1)


def _oracle_job(job):
    """One job = cases [lo, hi) of one (family, seed), re-drawn from the seed in the worker.  -> {it: (o32, o64, stages, seconds)}."""
    family, seed, lo, hi = job
    import torch
    torch.set_num_threads(1)
    out = {}
    for c in cases(family, seed):
        if c["it"] >= hi:
            break
        if c["it"] >= lo:
            t0 = time.time()
            out[c["it"]] = oracle_both(family, c) + (time.time() - t0,)
    from fresnel_amd import _binding
    assert not torch.cuda.is_initialized() and _binding._lib is None, "an oracle worker touched the GPU side"
    return out


N_ITER = {"phase": 24, "blend": 40, "blend_big": 6, "batch": 16, "batch_wide": 16, "asm": 14, "asm_batched": 24}  # the generators' defaults


def oracle_jobs(family, seed):
    n, step = N_ITER[family], CASES_PER_JOB[family]  # (that N_ITER is what the generators yield: test_family_sizes_are_pinned)
    return [(family, seed, lo, min(lo + step, n)) for lo in range(0, n, step)]


class OraclePool:
    """All oracle jobs of the selected (family, seed) pairs, submitted up front to at most MAX_WORKERS spawned CPU-only processes and
    collected case by case, so that the CPU work overlaps the GPU work of the tests that are already running."""

    def __init__(self, pairs, workers=None):
        import concurrent.futures as cf
        import multiprocessing as mp
        n = min(MAX_WORKERS, workers or MAX_WORKERS, max(1, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1))
        self._ex = cf.ProcessPoolExecutor(max_workers=n, mp_context=mp.get_context("spawn"), initializer=_worker_init)
        self._fut = {}
        for family, seed in pairs:
            for job in oracle_jobs(family, seed):
                f = self._ex.submit(_oracle_job, job)
                for it in range(job[2], job[3]):
                    self._fut[(family, seed, it)] = f
        self._done = {}

    def get(self, family, seed, it):
        """(o32, o64, stages, oracle seconds) of one case; each case can be taken once (its tensors are dropped afterwards)."""
        key = (family, seed, it)
        f = self._fut.pop(key)
        if id(f) not in self._done:
            self._done[id(f)] = f.result()
        res = self._done[id(f)]
        val = res.pop(it)
        if not res:
            del self._done[id(f)]
        return val

    def close(self):
        self._ex.shutdown(wait=True, cancel_futures=True)


# ----------------------------------------------------------------------------------------------------------------------------
# HIP side
# ----------------------------------------------------------------------------------------------------------------------------
def cuda_device():
    import pytest
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _hip_cameras(family, c):
    import torch
    from fresnel_amd.renderer import Camera
    if family in ("batch", "batch_wide"):
        cams = []
        for view, fx, fy, cx, cy in c.get("cams") or pose_cameras(c):
            cam = Camera(fx, fy, cx, cy, c["S"], c["S"])
            cam.set_view(torch.from_numpy(np.asarray(view, np.float32)))
            cams.append(cam)
        return cams
    W, H = c["W"], c["H"]
    if family in ("blend", "blend_big"):
        return Camera(c["fx"], c["fx"], c["cx"], c["cy"], W, H)
    if family == "asm_batched":
        return Camera(c["f"], c["f"], W / 2, H / 2, W, H)
    return Camera(0.8 * W, 0.8 * W, W / 2, H / 2, W, H)


def _blend_tuning(family, c):
    return c["tuning"] if family == "blend_big" else dict(tile_w=c["tile_w"])


def hip_case(family, c):
    """The HIP renderers on one case, forward and backward through autograd.  -> dict of numpy tensors, named as oracle_case names
    them (every gradient the renderer returns, compared or not)."""
    import torch
    from fresnel_amd.renderer import ASMWaveFieldRenderer, TileBasedRenderer, WaveFieldRenderer
    dev = cuda_device()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ts = [up(a).requires_grad_(True) for a in c["arrs"]]
    cam = _hip_cameras(family, c)
    out = {}
    if family in ("phase", "blend", "blend_big", "batch", "batch_wide"):
        ph = None
        if family == "phase":
            ren = TileBasedRenderer(c["W"], c["H"], background=c["bg"], use_phase_blending=True, phase_amplitude=c["amp"])
            ph = up(c["phases"]).requires_grad_(True)
            img, dep = ren(*ts, cam, return_depth=True, phases=ph)
        elif family in ("blend", "blend_big"):
            ren = TileBasedRenderer(c["W"], c["H"], background=c["bg"], max_radius=c["maxr"])
            ren.tuning = _blend_tuning(family, c)
            img, dep = ren(*ts, cam, return_depth=True)
        else:
            img, dep = TileBasedRenderer(c["S"], c["S"], background=c["bg"])(*ts, cam, return_depth=True)
        ((img * up(c["gI"])).sum() + (dep * up(c["gD"])).sum()).backward()
        rs_ = c.get("row_stride", 1)
        out["image"], out["depth"] = img.detach().cpu().numpy()[..., ::rs_, :], dep.detach().cpu().numpy()[..., ::rs_, :]
        if ph is not None:
            out["phases"] = ph.grad.cpu().numpy()
    elif family == "asm":
        W, H = c["W"], c["H"]
        ph = up(c["phases"]).requires_grad_(True)
        if c["kind"] == "asm":
            ren = ASMWaveFieldRenderer(W, H, background=c["bg"], **c["kw"]).to(dev)
            wl = up(c["wl"]).requires_grad_(True)
            img = ren(*ts, cam, phases=ph, wavelengths_rgb=wl)
            (img * up(c["gI"])).sum().backward()
            out["wavelengths"] = wl.grad.cpu().numpy()
        else:
            ren = WaveFieldRenderer(W, H, background=c["bg"]).to(dev)
            img, dep = ren(*ts, cam, return_depth=True, phases=ph)
            ((img * up(c["gI"])).sum() + (dep * up(c["gD"])).sum()).backward()
            out["depth"] = dep.detach().cpu().numpy()
        out["image"] = img.detach().cpu().numpy()
        out["phases"] = ph.grad.cpu().numpy()
    elif family == "asm_batched":
        W, H = c["W"], c["H"]
        ph = up(c["phases"]).requires_grad_(True)
        wl = up(c["wl"]).requires_grad_(True)
        ren = ASMWaveFieldRenderer(W, H, background=c["bg"], **c["kw"]).to(dev)
        img = ren(*ts, cam, phases=ph, wavelengths_rgb=wl)
        (img * up(c["gI"])).sum().backward()
        out.update(image=img.detach().cpu().numpy(), phases=ph.grad.cpu().numpy(), wavelengths=wl.grad.cpu().numpy())
    else:
        raise KeyError(family)
    for k, t in zip(GRADS, ts):
        out[k] = t.grad.cpu().numpy()
    return out


def hip_stages(arrs, cam, W, H, bg=(0, 0, 0), tuning=None, max_radius=64):
    """Integer stages of one forward (B,N,.) via the raw C-ABI entry; numpy views."""
    import torch
    from fresnel_amd import renderer as R
    dev = cuda_device()
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]
    cfg = R._Cfg(W, H, bg, max_radius, False, 0.25, tuning=tuning)
    camt = R.pack_cameras(cam, dev)
    img, dep, saved, dims, _ = R.forward_raw(*ts, None, camt, cfg)
    torch.cuda.synchronize()
    st = R.inspect_saved(saved, dims)
    out = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in st.items()}
    out["image"], out["depth"] = img.cpu().numpy(), dep.cpu().numpy()
    return out


def hip_case_stages(family, c):
    """hip_stages of a blend-path sweep case at the case's own radius cap, principal point, tile width and per-image cameras."""
    cam = _hip_cameras(family, c)
    if family in ("batch", "batch_wide"):
        return hip_stages(c["arrs"], cam, c["S"], c["S"], c["bg"])
    return hip_stages([a[None] for a in c["arrs"]], cam, c["W"], c["H"], c["bg"], tuning=_blend_tuning(family, c), max_radius=c["maxr"])


def check_integer_stages(st, b, r, W, H):
    """HIP integer stages of image b vs oracle Rendered r: all bit-exact."""
    from oracle import fgs_oracle as orc
    N = r.pos.shape[0]
    rec = st["rec"][b]
    key = st["depth_key"][b].view(np.uint32)
    vis_h = (key != 0xFFFFFFFF)
    assert np.array_equal(vis_h, r.proj["visible"].astype(bool)), "visibility differs"
    bbx = np.ascontiguousarray(rec[:, 10]).view(np.uint32)
    bby = np.ascontiguousarray(rec[:, 11]).view(np.uint32)
    bbox_h = np.stack([bbx & 0xFFFF, bbx >> 16, bby & 0xFFFF, bby >> 16], 1).astype(np.int32)
    assert np.array_equal(bbox_h[vis_h], r.proj["bbox"][vis_h]), "bbox differs"
    # canonical depth order: visible subsequence of the HIP order == oracle's
    order_h = st["order"][b]
    nv = int(vis_h.sum())
    assert np.array_equal(order_h[:nv], r.vis_sorted), "depth order differs"
    # the projected floats feeding those decisions are bit-identical too (canonical fp32)
    assert np.array_equal(np.ascontiguousarray(rec[vis_h, 0:2]).view(np.uint32), np.ascontiguousarray(r.proj["mean2d"][vis_h]).view(np.uint32))
    assert np.array_equal(np.ascontiguousarray(rec[vis_h, 9]).view(np.uint32), np.ascontiguousarray(r.proj["depth"][vis_h]).view(np.uint32))
    # per-tile lists
    ranges_o, ids_o = orc.tile_lists(r.vis_sorted, r.proj["bbox"], W, H, 16, tile_w=int(st["layout"].tile_w))
    T = len(ranges_o) - 1
    rg = st["ranges"][b]
    dup = st["dup_ids"]
    for t in range(T):
        s, e = int(rg[t, 0]), int(rg[t, 1])
        exp = ids_o[ranges_o[t]:ranges_o[t + 1]]
        assert e - s == len(exp), f"tile {t}: list length {e - s} != {len(exp)}"
        if len(exp):
            assert np.array_equal(dup[s:e] - b * N, exp), f"tile {t}: list differs"


def case_stage_failures(family, c, st, stages):
    """check_integer_stages on every image of a blend-path case.  -> list of 'image b: what differs' (empty = bit-exact)."""
    W, H = (c["S"], c["S"]) if "S" in c else (c["W"], c["H"])
    bad = []
    if c.get("tile_w") and int(st["layout"].tile_w) != c["tile_w"]:  # (0 = automatic: whatever the library picked is what is checked)
        bad.append(f"tile width {int(st['layout'].tile_w)} in use, {c['tile_w']} asked for")
    for b, rec in enumerate(stages):
        try:
            check_integer_stages(st, b, OracleStages(rec), W, H)
        except AssertionError as e:
            bad.append(f"image {b}: {str(e).splitlines()[0] if str(e) else 'projected mean2d / depth bits differ'}")
    return bad


# ----------------------------------------------------------------------------------------------------------------------------
# verdicts
# ----------------------------------------------------------------------------------------------------------------------------
def _distance(form, x, ref, ref64):
    """Distance of x from ref in one of the three forms; `ref64` fixes the scale of the wavelength form."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    if form == "rel":
        return rel_to_max(x, ref)
    if form == "abs":
        return float(np.abs(x - ref).max()) if ref.size else 0.0
    m = float(np.abs(np.asarray(ref64, np.float64)).max()) or 1.0
    fin = np.isfinite(ref)  # torch's fp32 autograd is NaN for a frequency exactly on the evanescent boundary: compared where finite
    return float(np.abs(x - ref)[fin].max() / m) if fin.any() else float("inf")


def sweep_verdict(x, o32, o64, form="rel"):
    """Verdict of one tensor of a sweep case against the oracle's fp32 run `o32` and fp64 run `o64`.

    The rule of tests/helpers.py (referee_tolerance) with the one addition the sweeps have always had: a tensor that is within 1e-4
    of EITHER oracle run passes, also where the fp64 run referees -- agreeing with the fp32 oracle to 1e-4 is the parity statement
    itself (`blend s6 it 38`: the fp32 oracle's gradients and HIP's are exactly 0, the fp64 oracle's are not).  So a tensor passes
      * "plain":   within 1e-4 of the fp32 run or of the fp64 run, or
      * "referee": the oracle's own spread exceeds 5e-5 and the tensor is within referee_tolerance(spread) of the fp64 run.
    A non-finite value fails before any tolerance is looked at.  A wavelength gradient whose fp32 reference has a NaN channel is
    judged against the fp64 run alone.  -> dict(ok, via in {"plain", "referee", "FAIL", "non-finite"}, e32, e64, spread, tol, use64,
    err = distance from the run that referees, ratio = smallest error / tolerance of the ways to pass)."""
    x = np.asarray(x)
    o32a = np.asarray(o32)
    if not np.isfinite(x).all():
        inf = float("inf")
        return dict(ok=False, via="non-finite", e32=inf, e64=inf, spread=float("nan"), tol=TOL, use64=False, err=inf, ratio=inf)
    spread = _distance(form, o32a, o64, o64) if form != "wavelength" else _distance(form, o64, o32a, o64)
    if not np.isfinite(spread):  # no finite channel in the fp32 reference at all
        spread = 1.0
    use64, tol = referee_tolerance(spread)
    e32, e64 = _distance(form, x, o32a, o64), _distance(form, x, o64, o64)
    if not np.isfinite(o32a).all():  # the NaN channels have no fp32 reference: the fp64 run judges the whole tensor
        use64, e32 = True, float("inf")
    plain = min(e32, e64) <= TOL
    referee = use64 and e64 <= tol
    ratio = min(e32 / TOL, e64 / TOL, e64 / tol if use64 else float("inf"))
    via = "plain" if plain else "referee" if referee else "FAIL"
    return dict(ok=plain or referee, via=via, e32=e32, e64=e64, spread=spread, tol=tol, use64=use64, err=e64 if use64 else e32, ratio=ratio)


def oracle_needs_referee(family, c, o32, o64):
    """Is the oracle's own fp32 run further than 1e-4 from its fp64 run in some compared tensor?  (The yardstick of the cap on
    referee-only verdicts: a faithful fp32 implementation has no reason to need the rule more often than the fp32 oracle does.)"""
    for k in compared_tensors(family, c):
        form = tensor_form(family, k)
        s = _distance(form, o64[k], o32[k], o64[k]) if form == "wavelength" else _distance(form, o32[k], o64[k], o64[k])
        if not s <= TOL:
            return True
    return False


def judge_case(family, seed, c, hip, o32, o64, stage_failures=(), seconds=0.0):
    """Verdict of one case.  -> dict(verdict in {"ok", "ok-referee", "FAIL"}, line, needs = oracle_needs_referee).
    `line`: `verdict family sSEED it IT <shape> | worst tensor | error vs the run that referees | tol | spread | plain | seconds`, followed
    for anything but a plain ok by one line per tensor that is not within 1e-4 of the fp32 oracle, and by the integer-stage
    differences."""
    rows, fail = [], []
    names = compared_tensors(family, c)
    for k in hip:
        if k in names:
            v = sweep_verdict(hip[k], o32[k], o64[k], tensor_form(family, k))
            rows.append((v["ratio"] if v["ratio"] == v["ratio"] else float("inf"), k, v))
            if not v["ok"]:
                fail.append(k)
        elif not np.isfinite(hip[k]).all():  # not compared, but must be finite
            inf = float("inf")
            rows.append((inf, k, dict(ok=False, via="non-finite", e32=inf, e64=inf, spread=float("nan"), tol=TOL, use64=False, err=inf, ratio=inf)))
            fail.append(k)
    missing = [k for k in names if k not in hip]
    rows.sort(key=lambda r: -r[0])
    _, wk, w = rows[0]
    plain = max(min(r[2]["e32"], r[2]["e64"]) for r in rows)
    if fail or missing or stage_failures:
        verdict = "FAIL"
    else:
        verdict = "ok-referee" if any(r[2]["via"] == "referee" for r in rows) else "ok"
    line = (f"{verdict:10s} {family} s{seed} it {c['it']:2d} {describe(c)} | {wk} | {w['err']:.2e} vs {'fp64' if w['use64'] else 'fp32'} | "
            f"tol {w['tol']:.1e} | spread {w['spread']:.1e} | plain {plain:.2e} | {seconds:.1f}s")
    if verdict != "ok":
        for _, k, v in rows:
            if not v["ok"] or v["e32"] > TOL:
                line += (f"\n             {k:12s} {v['via']:10s} err {v['err']:.2e} ({'fp64' if v['use64'] else 'fp32'} referee) tol {v['tol']:.1e} "
                         f"spread {v['spread']:.1e} vs-fp32 {v['e32']:.2e} vs-fp64 {v['e64']:.2e}")
        for k in missing:
            line += f"\n             {k:12s} missing from the result"
        for s in stage_failures:
            line += f"\n             integer stages, {s}"
    return dict(verdict=verdict, line=line, needs=oracle_needs_referee(family, c, o32, o64))


def run_seed(family, seed, get_oracle, hip_fn, stages_fn, emit=None):
    """Every case of one (family, seed): the implementation's side (`hip_fn(family, c)` -> tensors, `stages_fn(family, c)` -> integer
    stages in hip_stages' layout, blend-path families only) judged against `get_oracle(c)` -> (o32, o64, stage records, seconds).
    -> the judge_case results in case order; no case is left out and nothing stops at the first failure."""
    results = []
    for c in cases(family, seed):
        o32, o64, stages, _ = get_oracle(c)
        t0 = time.time()
        try:
            hip = hip_fn(family, c)
            bad = case_stage_failures(family, c, stages_fn(family, c), stages) if family in INTEGER_FAMILIES else ()
        except Exception as e:  # noqa: BLE001 -- say which scene it was, then let the test error out
            raise RuntimeError(f"{family} s{seed} it {c['it']} {describe(c)}: {type(e).__name__}: {e}") from e
        res = judge_case(family, seed, c, hip, o32, o64, bad, time.time() - t0)
        if emit is not None:
            emit(res["line"])
        results.append(res)
    return results
