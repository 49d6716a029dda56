"""scratch/profile/bwd_zero_units.py [workload] [distribution] [tuning]: which walk the units of one k_composite_bwd launch take.

Needs an experiment library built with FGS_BWD_UNIT_TRACE (python -m fresnel_amd.build --define FGS_BWD_UNIT_TRACE=1 --suffix _trace),
selected through FGS_LIB.  Every launch slot records its unit and its walk: 0 general, 1 dead walk over every sub-tile, 4 dead walk
with some sub-tiles masked (their S is +-0 on every lane), 3 a zero unit (S is +-0 on every lane of every sub-tile: rows written without
a walk).  This script runs the benchmark's batch (bench.synth_batch; default config3 saag), reads the records of the last backward and
prints the share of every kind out of all units and out of all list entries -- the premise figures of
profiles/r16_ab_bwd_zero_units.txt section 1.  `tuning` as bench.py --tuning takes it, e.g. tile_w=16.
It also prints how many of the units are TAIL units (behind the closing slot of every half of their tile, saved.fwd_close), how many zero
units are among them, and the summed launch-slot time (exit - entry clock) of every kind, 5 = a tail unit that left on its tile's
verdict (k_bwd_tail_verdict) -- profiles/r17_ab_bwd_tail_verdict.txt sections 1 and 4.
For the general units it prints their sub-tile passes and the share that lies in sub-tiles zero at the unit's restart (T == +0 on every
in-frame lane, S == +-0 on every lane), counted by the trace build whether or not the walk masks them (tuning key bwd_sub) --
profiles/r18_ab_bwd_zero_subtiles.txt section 1.  `--opacity X` (anywhere on the line) sets every opacity of the batch to X."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))  # the repository root
import bench  # noqa: E402

bench._import_compute()
from fresnel_amd import _binding as B  # noqa: E402
from fresnel_amd import renderer as R  # noqa: E402

opacity = None  # --opacity X: every opacity of the batch set to X (scratch/ab/opacity_batch.py's batch)
if "--opacity" in sys.argv:
    i = sys.argv.index("--opacity")
    opacity = float(sys.argv[i + 1])
    del sys.argv[i:i + 2]
workload = sys.argv[1] if len(sys.argv) > 1 else "config3"
distribution = sys.argv[2] if len(sys.argv) > 2 else "saag"
tuning = sys.argv[3] if len(sys.argv) > 3 else ""
dev = torch.device("cuda:0")
N, S, Bn = bench.WORKLOADS[workload]
pos, scale, quat, col, opa = bench.synth_batch(Bn, N, 1000 * int(workload[-1]), dev, distribution)
if opacity is not None:
    opa.fill_(opacity)
leaves = [t.requires_grad_(True) for t in (pos, scale, quat, col, opa)]
cam = R.Camera(0.8 * S, 0.8 * S, S / 2, S / 2, S, S)
ren = R.TileBasedRenderer(S, S).to(dev)
# (bwd_zero=1: automatic turns the path on from 8192 tile halves per launch only; the premise is measured at every size)
ren.tuning = dict(bwd_zero=1, **({k: int(v) for k, v in (kv.split("=") for kv in tuning.split(","))} if tuning else {}))
g = torch.Generator().manual_seed(4242)
gI = torch.randn(Bn, 3, S, S, generator=g).to(dev)
gD = (torch.randn(Bn, S, S, generator=g) * 0.1).to(dev)

lib = B.load()
if not hasattr(lib, "fgs_bwd_unit_trace"):
    sys.exit("the library has no fgs_bwd_unit_trace: build it with --define FGS_BWD_UNIT_TRACE=1")
lib.fgs_bwd_unit_trace.restype = ctypes.c_long
lib.fgs_bwd_unit_trace.argtypes = [ctypes.c_void_p, ctypes.c_size_t]

for step in range(2):
    for t in leaves:
        t.grad = None
    img, dep = ren(*leaves, cam, return_depth=True)
    node = img.grad_fn
    st = R.inspect_saved(node.saved_tensors[-1], node.dims)
    torch.autograd.backward([img, dep], [gI, gD])
torch.cuda.synchronize()
cap = int(st["layout"].seg_capacity)
seg_len = int(st["layout"].seg_len)
buf = np.zeros((cap, 3), np.uint64)
n = lib.fgs_bwd_unit_trace(buf.ctypes.data, cap)
assert n > 0, n
U = int(st["counters"][2])
rec = buf[:U]
assert (rec[:, 2] >> np.uint64(63)).all(), "a launch slot below U left no record"
unit = (rec[:, 2] & np.uint64(0xFFFFFFFF)).astype(np.int64)
walk = ((rec[:, 2] >> np.uint64(32)) & np.uint64(7)).astype(np.int64)
assert np.array_equal(np.sort(unit), np.arange(U)), "the launch did not run every unit exactly once"
rg = st["ranges"].cpu().numpy().astype(np.int64).reshape(-1, 2)
lens = rg[:, 1] - rg[:, 0]
seg_off = st["seg_off"].cpu().numpy().astype(np.int64)
seg_tile = st["seg_tile"][:U].cpu().numpy().astype(np.int64)
ulen = np.minimum(seg_len, lens[seg_tile[unit]] - (unit - seg_off[seg_tile[unit]]) * seg_len)
E = int(ulen.sum())
print(f"{workload} {distribution} {tuning or '-'}: tile_w {int(st['layout'].tile_w)}, seg_len {seg_len}, U = {U} units, {E} list entries")
for code, name in ((0, "general walk"), (3, "(a) zero units: S == +-0 on every lane of every sub-tile"),
                   (4, "(b) dead, some but not all sub-tiles all-zero"), (1, "(c) dead, no sub-tile all-zero")):
    m = walk == code
    print(f"  {name:62s} {int(m.sum()):7d} units = {100.0 * m.sum() / U:5.1f} %   {int(ulen[m].sum()):9d} entries = {100.0 * ulen[m].sum() / E:5.1f} %")
# ZERO SUB-TILES OF GENERAL UNITS (profiles/r18_ab_bwd_zero_subtiles.txt section 1).  A general unit's record carries, behind the walk
# code: bits 3-15 its sub-tile passes with none masked (sum over its entries of the touched sub-tiles), bits 16-28 those of them that
# lie in a sub-tile that is zero at the unit's restart (T == +0 on every in-frame lane, S == +-0 on every lane), bit 29 whether it has
# such a sub-tile at all.  Counted whether or not the walk masks them (tuning key bwd_sub).
code = (rec[:, 2] >> np.uint64(32)).astype(np.int64)
gen = walk == 0
passes, zpasses, has = (code >> 3) & 0x1FFF, (code >> 16) & 0x1FFF, (code >> 29) & 1
if gen.any():
    print(f"  general units: {int(passes[gen].sum())} sub-tile passes ({passes[gen].sum() / max(int(ulen[gen].sum()), 1):.2f} per entry), "
          f"{int(zpasses[gen].sum())} = {100.0 * zpasses[gen].sum() / max(int(passes[gen].sum()), 1):.2f} % in sub-tiles zero at restart; "
          f"{int(has[gen].sum())} = {100.0 * has[gen].sum() / gen.sum():.1f} % of the general units have such a sub-tile, "
          f"{int((zpasses[gen] > 0).sum())} of them a pass in one")
dead = walk != 0
print(f"  dead units in all: {100.0 * dead.sum() / U:.1f} % of the units, {100.0 * ulen[dead].sum() / E:.1f} % of the entries; "
      f"kind (a) is {100.0 * (walk == 3).sum() / max(int(dead.sum()), 1):.1f} % of the dead units")
# TAIL units (profiles/r17_ab_bwd_tail_verdict.txt section 1): segment >= the closing slot of EVERY 16 x 16 half of the tile, every
# half having one (saved.fwd_close).  All tail units of a tile restart from the same slots: one verdict per tile covers them.
if "fwd_close" in st:
    halves = int(st["layout"].tile_w) // 16
    fc = st["fwd_close"].cpu().numpy().astype(np.int64).reshape(-1, 2)[:, :halves]
    closed = (fc >= 0).all(axis=1)
    first_tail = np.where(closed, fc.max(axis=1), np.iinfo(np.int64).max)
    seg = unit - seg_off[seg_tile[unit]]
    tail = seg >= first_tail[seg_tile[unit]]
    zero = (walk == 3) | (walk == 5)  # (5: a tail unit that took its tile's verdict -- a zero unit that did not have to find out)
    tz = tail & zero
    print(f"  tail units: {int(tail.sum())} = {100.0 * tail.sum() / U:.1f} % of the units, {int(ulen[tail].sum())} entries = "
          f"{100.0 * ulen[tail].sum() / E:.1f} %; tiles with a tail: {int(np.unique(seg_tile[unit][tail]).size)} of {len(lens)}")
    print(f"  tail zero units: {int(tz.sum())} = {100.0 * tz.sum() / max(int(zero.sum()), 1):.1f} % of the zero units, "
          f"{int(ulen[tz].sum())} entries = {100.0 * ulen[tz].sum() / max(int(ulen[zero].sum()), 1):.1f} % of the zero units' entries, "
          f"{100.0 * ulen[tz].sum() / E:.1f} % of all entries; tail units that are NOT zero units: {int((tail & ~zero).sum())}")
    # a tile's tail units all take one verdict: tiles whose tail holds both zero and non-zero units would contradict that
    tt = seg_tile[unit][tail]
    zc = np.bincount(tt, weights=zero[tail].astype(np.float64), minlength=len(lens))
    ac = np.bincount(tt, minlength=len(lens))
    print(f"  tiles whose tail units disagree about the verdict: {int(((zc > 0) & (zc < ac)).sum())}")
else:
    print("  (no saved.fwd_close: the exiting forward did not run, no unit is a tail unit)")
# slot time: exit - entry clock (100 MHz) of every launch slot, by kind
dt = (rec[:, 1].astype(np.int64) - rec[:, 0].astype(np.int64)).astype(np.float64)
span = float(rec[:, 1].max() - rec[:, 0].min())
for code, name in ((0, "general"), (1, "dead, full"), (4, "dead, masked"), (3, "zero units"), (5, "tail exits")):
    m = walk == code
    if m.any():
        print(f"  slot time {name:13s} {dt[m].sum() / 100.0:10.1f} us summed = {100.0 * dt[m].sum() / dt.sum():5.1f} % of all slots' "
              f"({100.0 * m.sum() / U:5.1f} % of the launch slots), mean {dt[m].mean() / 100.0:6.2f} us")
print(f"  all slots: {dt.sum() / 100.0:.1f} us summed over {U} slots; first entry to last exit {span / 100.0:.1f} us")
