"""scratch/profile/bwd_unit_drain.py [workload]: how one k_composite_bwd launch of the benchmark's batch ends.

Needs an experiment library built with FGS_BWD_UNIT_TRACE (python -m fresnel_amd.build --define FGS_BWD_UNIT_TRACE=1 --suffix _trace;
with --define FGS_BWD_TILE_ORDER=1 as well: the units in tile order, as before saved.unit_order existed), selected through FGS_LIB.
Every launch slot of the kernel records wall_clock64() (100 MHz) at entry and exit, its unit and the walk it took; this script runs
a few steps of the workload (default config3: bench.synth_batch, 8 x 32 768 at 512^2), reads the records of the last backward and
prints: the launch's length, the time from the last unit's start to the kernel's end (the drain), the number of resident units in
10 us steps over the last 200 us, and the residency of full / partial and dead / general units."""
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
dev = torch.device("cuda:0")
N, S, Bn = bench.WORKLOADS[workload]
pos, scale, quat, col, opa = bench.synth_batch(Bn, N, 3000, dev)
leaves = [t.requires_grad_(True) for t in (pos, scale, quat, col, opa)]
cam = R.Camera(0.8 * S, 0.8 * S, S / 2, S / 2, S, S)
ren = R.TileBasedRenderer(S, S).to(dev)
g = torch.Generator().manual_seed(4242)
gI = torch.randn(Bn, 3, S, S, generator=g).to(dev)
gD = (torch.randn(Bn, S, S, generator=g) * 0.1).to(dev)

lib = B.load()
if not hasattr(lib, "fgs_bwd_unit_trace"):
    sys.exit("the library has no fgs_bwd_unit_trace: build it with --define FGS_BWD_UNIT_TRACE=1")
lib.fgs_bwd_unit_trace.restype = ctypes.c_long
lib.fgs_bwd_unit_trace.argtypes = [ctypes.c_void_p, ctypes.c_size_t]

for step in range(4):
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
t0, t1 = rec[:, 0].astype(np.int64), rec[:, 1].astype(np.int64)
unit = (rec[:, 2] & np.uint64(0xFFFFFFFF)).astype(np.int64)
walk = ((rec[:, 2] >> np.uint64(32)) & np.uint64(3)).astype(np.int64)
assert np.array_equal(np.sort(unit), np.arange(U)), "the launch did not run every unit exactly once"
rg = st["ranges"].cpu().numpy().astype(np.int64).reshape(-1, 2)
lens = rg[:, 1] - rg[:, 0]
seg_off = st["seg_off"].cpu().numpy().astype(np.int64)
seg_tile = st["seg_tile"][:U].cpu().numpy().astype(np.int64)
ulen = np.minimum(seg_len, lens[seg_tile[unit]] - (unit - seg_off[seg_tile[unit]]) * seg_len)
US = 100.0  # ticks per microsecond
begin, end = t0.min(), t1.max()
dur = (t1 - t0) / US
print(f"{os.path.basename(os.environ.get('FGS_LIB', 'libfgs_hip.so'))} {B.version()} {workload}: U = {U} units ({(ulen == seg_len).sum()} full, "
      f"{(ulen != seg_len).sum()} partial of mean {ulen[ulen != seg_len].mean():.1f} entries; {(walk == 1).sum()} dead walks), seg_len {seg_len}")
print(f"launch: first entry to last exit {(end - begin) / US:.1f} us; mean residency of a unit {dur.mean():.1f} us (full {dur[ulen == seg_len].mean():.1f}, "
      f"partial {dur[ulen != seg_len].mean():.1f}; dead walk {dur[walk == 1].mean():.1f}, general walk {dur[walk == 0].mean():.1f})")
print(f"drain: last unit starts {(end - t0.max()) / US:.1f} us before the kernel's end; the last FULL unit starts {(end - t0[ulen == seg_len].max()) / US:.1f} us before it")
last = np.argsort(t1)[-8:]
print("the eight last units to end: " + ", ".join(f"{ulen[i]} entries / {dur[i]:.0f} us" + (" dead" if walk[i] == 1 else "") for i in last))
print("resident units, in 10 us steps before the kernel's end (us before the end: units, of them partial):")
line = []
for k in range(20, -1, -1):
    t = end - int(k * 10 * US)
    res = (t0 <= t) & (t1 > t)
    line.append(f"{k * 10}: {int(res.sum())}/{int((res & (ulen != seg_len)).sum())}")
print("  " + "  ".join(line))
idle = 0.0
for k in range(200):
    t = end - int((k + 0.5) * US)
    idle += 5120 - min(5120, int(((t0 <= t) & (t1 > t)).sum()))
print(f"unit slots left empty over the last 200 us (of 5120 x 200 slot-us): {idle:.0f} slot-us = {idle / 5120:.1f} us of the whole chip")
