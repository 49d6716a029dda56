"""SSIM loss profile: the library's fused SSIM kernels (fresnel_amd.losses.ssim -> csrc/fgs_ssim.hip) against the torch
formulation of the same definition (pytorch_msssim's: grouped conv2d Gaussian filter, autograd) on the same GPU, at config 3's
rendered batch (8 x 3 x 512 x 512) and 16 x 3 x 256 x 256.  Run plain for ms per call, or under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python3 scratch/profile/profile_ssim.py` for per-kernel times.
Prints one JSON line: forward+backward ms (gradient for the rendered batch only, as in training), no-grad forward ms, the
algorithmic bytes and flops of the kernels, and the HBM / VALU fractions those imply at the measured call times."""
import json, sys, time
import torch
import torch.nn.functional as F
sys.path.insert(0, '.')
from fresnel_amd import losses as hip

dev = torch.device('cuda:0')
HBM_BPS, VALU_FLOPS = 6.29e12, 78.6e12  # measured float4-copy HBM rate; the plain (non-packed) fp32 vector rate


def torch_ssim(X, Y, data_range=1.0, win_size=11, win_sigma=1.5, K=(0.01, 0.03)):
    """pytorch_msssim.ssim(X, Y, data_range, size_average=True) in stock torch (fp32, grouped conv2d)."""
    C = X.shape[1]
    coords = torch.arange(win_size, dtype=torch.float32) - win_size // 2
    g = torch.exp(-(coords ** 2) / (2 * win_sigma ** 2))
    g = (g / g.sum()).to(X.device).reshape(1, 1, 1, -1).repeat(C, 1, 1, 1)

    def filt(t):
        return F.conv2d(F.conv2d(t, g.transpose(2, 3), groups=C), g, groups=C)
    c1, c2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mu1, mu2 = filt(X), filt(Y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = filt(X * X) - mu1_sq, filt(Y * Y) - mu2_sq, filt(X * Y) - mu1_mu2
    cs_map = (2 * s12 + c2) / (s1 + s2 + c2)
    ssim_map = ((2 * mu1_mu2 + c1) / (mu1_sq + mu2_sq + c1)) * cs_map
    return torch.flatten(ssim_map, 2).mean(-1).mean()


def timed(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


out = {}
for Bn, C, S in ((8, 3, 512), (16, 3, 256)):
    g = torch.Generator().manual_seed(0)
    x = torch.rand(Bn, C, S, S, generator=g).to(dev).requires_grad_(True)
    y = (x.detach() + 0.1 * torch.randn(Bn, C, S, S, generator=g).to(dev)).clamp(0, 1)

    def fb(fn):
        return lambda: torch.autograd.grad(fn(x, y, data_range=1.0), (x,))

    def nog(fn):
        def run():
            with torch.no_grad():
                fn(x, y, data_range=1.0)
        return run
    hip_fb, torch_fb = timed(fb(hip.ssim)), timed(fb(torch_ssim))
    hip_fwd, torch_fwd = timed(nog(hip.ssim)), timed(nog(torch_ssim))
    with torch.no_grad():
        diff = abs(float(hip.ssim(x, y, data_range=1.0)) - float(torch_ssim(x, y)))
    n = Bn * C * S * S
    Ho = S - 10
    rows = (42 / 32)  # horizontal pass: 32 + 10 staged rows per 32-row tile
    # algorithmic bytes: forward reads X, Y and writes 3 factor maps (valid region); backward reads X, Y, 3 maps, writes dX
    fwd_b, bwd_b, nog_b = 8 * n + 12 * Bn * C * Ho * Ho, 8 * n + 12 * Bn * C * Ho * Ho + 4 * n, 8 * n
    # flops per output pixel: horizontal 5 moments x 11 FMA + 3 products per staged row, vertical 5 x 11 FMA, S ~ 20, maps ~ 25;
    # backward per input pixel: 3 maps x 11 FMA horizontal (per staged row) + vertical, combine 8
    fwd_f = Bn * C * Ho * Ho * ((5 * 11 * 2 + 3) * rows + 5 * 11 * 2 + 20 + 25)
    bwd_f = n * (3 * 11 * 2 * rows + 3 * 11 * 2 + 8)
    floor_ms = (max((fwd_b) / HBM_BPS, fwd_f / VALU_FLOPS) + max(bwd_b / HBM_BPS, bwd_f / VALU_FLOPS)) * 1e3
    out[f'{Bn}x{C}x{S}x{S}'] = {
        'fwd_bwd_ms': {'hip': round(hip_fb, 4), 'torch': round(torch_fb, 4), 'speedup': round(torch_fb / hip_fb, 2)},
        'no_grad_fwd_ms': {'hip': round(hip_fwd, 4), 'torch': round(torch_fwd, 4), 'speedup': round(torch_fwd / hip_fwd, 2)},
        'loss_abs_diff_vs_torch_fp32': diff,
        'algorithmic': {'fwd_bytes': fwd_b, 'bwd_bytes': bwd_b, 'no_grad_fwd_bytes': nog_b, 'fwd_flops': int(fwd_f),
                        'bwd_flops': int(bwd_f)},
        'paper_floor_fwd_bwd_ms': round(floor_ms, 4),
        'hbm_fraction_fwd_bwd_call': round((fwd_b + bwd_b) / HBM_BPS * 1e3 / hip_fb, 3),
        'valu_fraction_fwd_bwd_call': round((fwd_f + bwd_f) / VALU_FLOPS * 1e3 / hip_fb, 3),
        'hbm_fraction_no_grad_call': round(nog_b / HBM_BPS * 1e3 / hip_fwd, 3),
    }
print(json.dumps({'what': 'losses.ssim (HIP) vs the torch formulation, fp32, data_range 1, 11-tap window; ms per call (host '
                  'clock over 50 calls, one sync); fractions = algorithmic bytes or flops at peak over the CALL time',
                  'device': torch.cuda.get_device_name(0), 'ssim': out}))
