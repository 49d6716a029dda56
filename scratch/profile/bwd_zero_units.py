"""scratch/profile/bwd_zero_units.py [workload] [distribution] [tuning]: which walk the units of one k_composite_bwd launch take.

Needs an experiment library built with FGS_BWD_UNIT_TRACE (python -m fresnel_amd.build --define FGS_BWD_UNIT_TRACE=1 --suffix _trace),
selected through FGS_LIB.  Every launch slot records its unit and its walk: 0 general, 1 dead walk over every sub-tile, 4 dead walk
with some sub-tiles masked (their S is +-0 on every lane), 3 a zero unit (S is +-0 on every lane of every sub-tile: rows written without
a walk).  This script runs the benchmark's batch (bench.synth_batch; default config3 saag), reads the records of the last backward and
prints the share of every kind out of all units and out of all list entries -- the premise figures of
profiles/r16_ab_bwd_zero_units.txt section 1.  `tuning` as bench.py --tuning takes it, e.g. tile_w=16."""
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

workload = sys.argv[1] if len(sys.argv) > 1 else "config3"
distribution = sys.argv[2] if len(sys.argv) > 2 else "saag"
tuning = sys.argv[3] if len(sys.argv) > 3 else ""
dev = torch.device("cuda:0")
N, S, Bn = bench.WORKLOADS[workload]
pos, scale, quat, col, opa = bench.synth_batch(Bn, N, 1000 * int(workload[-1]), dev, distribution)
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
dead = walk != 0
print(f"  dead units in all: {100.0 * dead.sum() / U:.1f} % of the units, {100.0 * ulen[dead].sum() / E:.1f} % of the entries; "
      f"kind (a) is {100.0 * (walk == 3).sum() / max(int(dead.sum()), 1):.1f} % of the dead units")
