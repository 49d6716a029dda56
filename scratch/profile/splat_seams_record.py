"""Record of tests/test_splat_seams.py: per scene what its CPU checks found, the oracle's own fp32-fp64 spread per tensor and -- with a
GPU -- the HIP renderer's distance from the oracle with the tolerance that applied, dL/dlambda of the ASM scenes, whether a second run
and the replicas / single-camera calls are bitwise equal.  Nothing is asserted here beyond the placement checks; the tests do that.
A HIP error ends the run at once.

    python scratch/profile/splat_seams_record.py [out.txt] [--cpu]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import helpers  # noqa: E402
import test_splat_seams as ss  # noqa: E402


def seam_errors(say):
    """what one seam error of each kind does to the oracle (CPU): the tensors that leave the statement, (distance, tolerance)"""
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ss.test_statement_sees_a_seam_error()
    say("\n== one seam error given to the oracle (CPU): {(image, tensor): (distance, tolerance)} of the tensors that fail the statement")
    for line in buf.getvalue().splitlines():
        say("  " + line)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    gpu = "--cpu" not in sys.argv
    out = open(args[0], "w") if args else sys.stdout

    def say(*a):
        print(*a, file=out, flush=True)

    say(f"tolerance {ss.TOL:.0e} (image: absolute; depth map and gradients: of the tensor's maximum) against the fp32 oracle; the oracle's "
        f"fp32-fp64 spread must stay <= {ss.SPREAD_MAX:.0e}, else (REFEREED) helpers.referee: the fp64 run and its tolerance")
    for key in ss.KEYS:
        sc = ss.scene(key)
        t0 = time.time()
        found = ss.check_placement(key)
        say(f"\n== {key}: {sc.kind}, call of {len(sc.batch)} image(s) of {sc.images[0].arrs[0].shape[0]} Gaussians, {len(sc.cams)} camera(s), "
            f"max_radius {sc.max_radius:g}" + (f", planes {sc.asm['num_planes']} over {sc.asm['depth_range']}" if sc.kind == "asm" else ""))
        say(f"  found: {found}")
        for j, (r32, r64) in enumerate(ss.reference(key)):
            say(f"  image {j}: peak {r32['peak']:.4f} ({r32['peak_count']} element(s)), summed amplitude {float(r32['tasq'].min()):.3g} ... "
                f"{float(r32['tasq'].max()):.3g}, nearest to its clamp at 1: {float(np.abs(r32['tasq'] - 1).min()):.1e}"
                if "peak" in r32 else f"  image {j}: no visible Gaussian")
        spread = ss.spreads(key)
        got = ss.hip(key) if gpu else None
        dist = ss.distances(key, got) if gpu else {}
        for (j, name), s in spread.items():
            d = dist.get((j, name))
            ref = name in ss.REFEREED.get(key, ())
            say(f"  image {j} {name:10s} oracle spread {s:.1e}" + ("" if d is None else f"   HIP {d[0]:.1e}   tolerance {d[1]:.1e}")
                + (" (referee)" if ref else "") + ("   SPREAD ABOVE BOUND" if s > ss.SPREAD_MAX and not ref else "")
                + ("   ABOVE TOLERANCE" if d is not None and not d[0] <= d[1] else ""))
        if gpu and sc.kind == "asm":
            want = sum(np.asarray(ss.reference(key)[j][0]["grad_wavelengths"], np.float64) for j in sc.batch)
            want64 = sum(np.asarray(ss.reference(key)[j][1]["grad_wavelengths"], np.float64) for j in sc.batch)
            m = float(np.abs(want64).max())
            fin = np.isfinite(want)
            s = float(np.abs(want - want64)[fin].max() / m)
            use64, tol = helpers.referee_tolerance(s)
            err = float(np.abs(got["wavelengths"] - (want64 if use64 else want))[fin].max() / (m if use64 else np.abs(want[fin]).max()))
            say(f"  dL/dlambda         oracle spread {s:.1e}   HIP {err:.1e}   tolerance {tol:.1e}" + (" (fp64 run)" if use64 else "")
                + ("   ABOVE TOLERANCE" if not err <= tol else ""))
        if gpu:
            again = ss._hip(sc)
            say(f"  second run bitwise equal: {all(np.array_equal(got[k], again[k]) for k in got)}; every gradient finite: "
                f"{all(np.isfinite(got[k]).all() for k in got)}; culled rows exactly zero: "
                f"{all(not got[k][b, sc.images[j].culled].any() for k in ss.GRADS for b, j in enumerate(sc.batch))}")
            if key.startswith("onewave"):
                same = all(np.array_equal(got[k][b], got[k][b % 4]) for k in ["image", "depth"] + ss.GRADS for b in range(4, len(sc.batch)))
                say(f"  replicas of each of the four scenes bitwise equal: {same}")
            if key.startswith("cameras_each"):
                for b in range(3):
                    one = ss._hip(ss.Scene(sc.kind, sc.W, sc.H, [sc.images[b]], cams=[sc.cams[b]], asm=sc.asm))
                    names = ["image"] + (["depth"] if sc.kind == "wave" else []) + ss.GRADS
                    say(f"  image {b} bitwise the single-image call with camera {b}: { {k: bool(np.array_equal(got[k][b], one[k][0])) for k in names} }")
        say(f"  ({time.time() - t0:.2f} s)")
    seam_errors(say)


if __name__ == "__main__":
    main()
