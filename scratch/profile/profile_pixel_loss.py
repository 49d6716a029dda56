"""Per-pixel loss profile: the fused HIP block (fresnel_amd.losses.pixel_losses -> csrc/fgs_pixel_loss.hip; density-weighted L1
+ zone-boundary term + normalised-depth L1) against the torch formulation of the same terms (the "torch" backend of
fresnel_amd.train.compute_losses, autograd) on the same GPU in the same process, ALTERNATING, at config 3's rendered batch
(8 x 3 x 512 x 512) and config 2's (16 x 3 x 256 x 256).  Forward + backward, gradients for the rendered batch and its depth.
Run plain for ms per call, or as
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python3 scratch/profile/profile_pixel_loss.py kernels`
for per-kernel times (that mode runs the HIP block alone, 20 calls at 8 x 3 x 512 x 512).  Prints one JSON line."""
import json, statistics, sys, time
import torch
sys.path.insert(0, '.')
from fresnel_amd.train import TrainingConfig, compute_losses

dev = torch.device('cuda:0')
HBM_BPS = 6.29e12  # measured float4-copy HBM rate
kernels_only = len(sys.argv) > 1 and sys.argv[1] == 'kernels'
TERMS = {'all_terms': dict(use_vlm_guidance=True, use_fresnel_zones=True, boundary_weight=0.1), 'rgb_depth': {}}


def timed(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


out = {}
for Bn, S in ((8, 512), (16, 256))[:1 if kernels_only else 2]:  # (kernel statistics: one shape, so that the averages mean something)
    g = torch.Generator().manual_seed(0)
    t = torch.rand(Bn, 3, S, S, generator=g).to(dev)
    r = (t + 0.25 * torch.randn(Bn, 3, S, S, generator=g).to(dev)).clamp(0, 1).requires_grad_(True)
    td = torch.rand(Bn, S, S, generator=g).to(dev)
    rd = (0.3 + 2.0 * td + 0.5 * torch.randn(Bn, S, S, generator=g).to(dev)).requires_grad_(True)
    den = (0.5 + torch.rand(Bn, 1, S, S, generator=g)).to(dev)
    row = {}
    for tname, tkw in TERMS.items():
        def fb(backend):
            cfg = TrainingConfig(image_size=S, device='cuda:0', ssim_weight=0.0, pixel_loss_backend=backend, **tkw)
            return lambda: torch.autograd.grad(compute_losses(r, t, rd, td, cfg, vlm_density=den)[0], (r, rd))
        if kernels_only:
            if tname == 'all_terms':
                f = fb('hip')
                for _ in range(20):
                    f()
                torch.cuda.synchronize()
            continue
        legs = {'hip': [], 'torch': []}
        for _ in range(5):  # alternating legs: both formulations see the same clocks and the same neighbours
            for backend in ('hip', 'torch'):
                legs[backend].append(timed(fb(backend)))
        gh, gt = fb('hip')(), fb('torch')()
        n = Bn * S * S
        fwd_b = (6 + 3) * 4 * n if tname == 'all_terms' else (6 + 2) * 4 * n
        row[tname] = {
            'fwd_bwd_ms': {k: {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)} for k, v in legs.items()},
            'speedup_median': round(statistics.median(legs['torch']) / statistics.median(legs['hip']), 2),
            'rendered_grad_gap_of_max': float((gh[0] - gt[0]).abs().max() / gt[0].abs().max()),
            'paper_bytes': {'stage1': fwd_b, 'stage2': 8 * n, 'stage3': 8 * n, 'backward': fwd_b + 16 * n},
            'paper_us_at_hbm_rate': {'stage1': round(fwd_b / HBM_BPS * 1e6, 1), 'stage2': round(8 * n / HBM_BPS * 1e6, 1),
                                     'stage3': round(8 * n / HBM_BPS * 1e6, 1), 'backward': round((fwd_b + 16 * n) / HBM_BPS * 1e6, 1)},
        }
    out[f'{Bn}x3x{S}x{S}'] = row
print(json.dumps({'what': 'compute_losses with pixel_loss_backend hip vs torch, fp32, forward + backward (gradients of rendered and '
                  'rendered_depth); ms per call by host clock over 50 calls with one sync, 5 alternating legs each; all_terms = '
                  'VLM-weighted L1 + boundary + depth, rgb_depth = the default terms', 'device': torch.cuda.get_device_name(0),
                  'mode': 'kernels' if kernels_only else 'timing', 'pixel_loss': out}))
