"""Record of tests/test_phase_seams.py: per scene what its CPU checks found (list lengths and starts, the nt set, the branch figures of
the faint and clamp scenes), the oracle's own fp32-fp64 spread and -- with a GPU -- the HIP path's distance from the fp32 oracle per
tensor, and the largest checkpoint deviation.  Nothing is asserted here beyond the placement checks; the tests do that.

    python scratch/profile/phase_seams_record.py [out.txt] [--cpu]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_phase_seams as ps  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    gpu = "--cpu" not in sys.argv
    out = open(args[0], "w") if args else sys.stdout

    def say(*a):
        print(*a, file=out, flush=True)

    say(f"tolerance {ps.TOL:.0e} of max against the fp32 oracle; the oracle's fp32-fp64 spread must stay <= {ps.SPREAD_MAX:.0e}")
    for key in ps.KEYS:
        sc = ps.scene(key)
        t0 = time.time()
        found = ps.check_placement(key)
        say(f"\n== {key}: {len(sc.images)} image(s) of {sc.images[0].arrs[0].shape[0]} Gaussians, amplitude {sc.amp}")
        for b, L in enumerate(ps.lists(key)):
            say(f"  image {b}: list lengths {[int(n) for n in L['length']]} starts {[int(s) for s in L['start']]} "
                f"starts mod 8 {[int(s) % 8 for s in L['start']]}")
        say(f"  nt per (tile, sub-tile, scan block): {sorted(ps._nt_set(key))}")
        if key.startswith(("groups", "amp0")):
            clash = [v for v in ps._slots(key, with_tile=False).values() if len({(b, t) for b, t, _, _ in v}) > 1]
            say(f"  checkpoint slots in use {len(ps._slots(key))}, none shared; without the `+ tile` term {len(clash)} would be shared by two tiles")
        if found is not None:
            say(f"  found: {found}")
        spread = ps.spreads(key)
        dist = ps.distances(key, ps.hip(key)) if gpu else {}
        for (b, name), s in spread.items():
            d = dist.get((b, name))
            say(f"  image {b} {name:18s} oracle spread {s:.1e}" + ("" if d is None else f"   HIP vs fp32 oracle {d:.1e}")
                + ("   SPREAD ABOVE BOUND" if s > ps.SPREAD_MAX else "") + ("   ABOVE TOLERANCE" if d is not None and d > ps.TOL else ""))
        say(f"  ({time.time() - t0:.2f} s)")
    if gpu:
        worst, n = ps.read_back_checkpoints("groups-64x32")
        say(f"\ncheckpoints of groups-64x32 read back: largest deviation from the fp64 loop {worst:.1e} over {n} (slot, sub-tile) pairs")


if __name__ == "__main__":
    main()
