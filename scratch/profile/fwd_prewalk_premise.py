"""scratch/profile/fwd_prewalk_premise.py [workload] [distribution] [tuning] [--opacity X]: what a pre-walk of short lists' later parts
would walk, counted from one forward's tables (saved.ranges, saved.fwd_open, saved.fwd_close through inspect_saved).

A SHORT list has 2 <= nseg <= NP segments (NP = the plan's list parts): spp == 1, the head's reach is segment 0, parts 1 .. nseg - 1
are one segment each and start from T = 1.  For the halves of such tiles the script prints how many the head closed, how many it left
open, and the entry-visits (list entries staged by one wave of one half) of parts 1.. in either kind: walked for nothing in a closed
half, moved out of the rest launch in an open one.  The same for spp <= 2 (nseg <= 2 NP).  Premise figures of
profiles/r19_ab_fwd_prewalk.txt section 1.  The counts do not depend on the tuning key fwd_prewalk: the head's marks are the same words."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))  # the repository root
import bench  # noqa: E402

bench._import_compute()
from fresnel_amd import renderer as R  # noqa: E402

opacity = None
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
cam = R.Camera(0.8 * S, 0.8 * S, S / 2, S / 2, S, S)
ren = R.TileBasedRenderer(S, S).to(dev)
ren.tuning = {k: int(v) for k, v in (kv.split("=") for kv in tuning.split(","))} if tuning and tuning != "-" else None
leaves = [t.requires_grad_(True) for t in (pos, scale, quat, col, opa)]
img, dep = ren(*leaves, cam, return_depth=True)
node = img.grad_fn
st = R.inspect_saved(node.saved_tensors[-1], node.dims)
torch.cuda.synchronize()
if "fwd_open" not in st:
    sys.exit("no saved.fwd_open: the exiting forward did not run")
L = st["layout"]
seg_len, halves = int(L.seg_len), int(L.tile_w) // 16
NP = int(st["counters"][5]) & 0x1F  # the plan's work split as the forward recorded it
rg = st["ranges"].cpu().numpy().astype(np.int64).reshape(-1, 2)
lens = rg[:, 1] - rg[:, 0]
nseg = (lens + seg_len - 1) // seg_len
op = st["fwd_open"].cpu().numpy().astype(np.int64).reshape(-1, 2)[:, :halves]
fc = st["fwd_close"].cpu().numpy().astype(np.int64).reshape(-1, 2)[:, :halves]
print(f"{workload} {distribution} {tuning or '-'} opacity {opacity}: tile_w {int(L.tile_w)}, seg_len {seg_len}, NP {NP}, {len(lens)} tiles, "
      f"{int(lens.sum())} list entries; open halves {int((op != 0).sum())} in {int((op != 0).any(axis=1).sum())} tiles")
for name, reach in (("spp == 1 (2 <= nseg <= NP)", 1), ("spp <= 2 (2 <= nseg <= 2 NP)", 2)):
    spp = (nseg + NP - 1) // NP
    m = (nseg >= 2) & (spp <= reach) & (nseg > spp)  # more than one part
    later = np.maximum(lens - spp * seg_len, 0)  # entries behind part 0
    n_open = (op[m] != 0).sum(axis=1)
    n_closed = halves - n_open
    ended = ((op[m] == 0) & (fc[m] < 0)).sum()  # not open, no closing slot: closed inside the last segment (a list of >= 2 segments cannot END in the head)
    print(f"  {name}: {int(m.sum())} tiles, {int(m.sum()) * halves} halves: {int(n_closed.sum())} the head closes "
          f"({int(ended)} of them without a closing slot), {int(n_open.sum())} it leaves open")
    print(f"    entry-visits of parts 1..: closed halves {int((later[m] * n_closed).sum())} (walked for nothing), "
          f"open halves {int((later[m] * n_open).sum())} (moved out of the rest launch); part waves moved {int(((nseg[m] - 1) // spp[m] * n_open).sum())}, "
          f"for nothing {int(((nseg[m] - 1) // spp[m] * n_closed).sum())}")
other = (op != 0).sum(axis=1)[nseg > 2 * NP]
print(f"  longer lists (nseg > 2 NP): {int((nseg > 2 * NP).sum())} tiles, {int(other.sum())} open halves; nseg <= 1: {int((nseg <= 1).sum())} tiles")
