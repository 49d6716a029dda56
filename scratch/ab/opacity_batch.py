"""scratch/ab/opacity_batch.py <opacity>: config 3's batch (bench.synth_batch, 8 x 32 768 at 512^2) with every opacity set to the value; forward +
backward step timed by events over 100 steps after 10 warm-up steps.  The library comes from FGS_LIB."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))  # the repository root
import bench  # noqa: E402

bench._import_compute()
from fresnel_amd import renderer as R  # noqa: E402

opacity = float(sys.argv[1])
dev = torch.device("cuda:0")
N, S, B = bench.WORKLOADS["config3"]
pos, scale, quat, col, opa = bench.synth_batch(B, N, 3000, dev)
opa.fill_(opacity)
leaves = [t.requires_grad_(True) for t in (pos, scale, quat, col, opa)]
cam = R.Camera(0.8 * S, 0.8 * S, S / 2, S / 2, S, S)
ren = R.TileBasedRenderer(S, S).to(dev)
g = torch.Generator().manual_seed(4242)
gI = torch.randn(B, 3, S, S, generator=g).to(dev)
gD = (torch.randn(B, S, S, generator=g) * 0.1).to(dev)


def step():
    for t in leaves:
        t.grad = None
    img, dep = ren(*leaves, cam, return_depth=True)
    torch.autograd.backward([img, dep], [gI, gD])


for _ in range(10):
    step()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(100):
    step()
e1.record()
torch.cuda.synchronize()
print("%-28s opacity %.2f step %.4f ms" % (os.path.basename(os.environ.get("FGS_LIB", "libfgs_hip.so")), opacity, e0.elapsed_time(e1) / 100))
