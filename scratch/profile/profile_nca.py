"""Workload for a kernel trace of the NCA decoder: 10 forward + backward passes of NCAGaussianDecoder at the reference's defaults,
16 images, training mode, after 3 untraced-in-spirit warm-up passes (they are in the trace too: 13 passes in all).
usage: rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scratch/profile/profile_nca.py torch|hip"""
import sys
import torch
sys.path.insert(0, '.')
from fresnel_amd.decoder import NCAGaussianDecoder

backend = sys.argv[1]
dev = torch.device("cuda:0")
torch.manual_seed(0)
model = NCAGaussianDecoder(nca_backend=backend, head_backend="hip").to(dev).train()
with torch.no_grad():
    model.update_rule[-1].weight.normal_(0.0, 0.15)
features = torch.randn(16, 384, 37, 37, device=dev, requires_grad=True)
depth = torch.rand(16, 1, 64, 64, device=dev)
for _ in range(13):
    out = model(features, depth)
    sum(v.sum() for v in out.values()).backward()
torch.cuda.synchronize()
print("done", backend)
