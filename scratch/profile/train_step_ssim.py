"""What the SSIM term costs per training step: fresnel_amd.train.train_step at config 2 / config 3 shapes (as
train_step_bench.py) with ssim_backend "msssim" (the default: pytorch_msssim's term when that package is importable, none
otherwise -- `msssim_available` says which) and "hip" (fresnel_amd.losses.ssim), eager and replayed from one captured graph.
usage: python scratch/profile/train_step_ssim.py [steps]  -> one JSON line"""
import json, sys, time
import numpy as np, torch
sys.path.insert(0, '.')
from fresnel_amd import train as T
from fresnel_amd.dist import DPContext
from fresnel_amd.train import GraphedTrainStep, PatchGaussianDecoder, SyntheticDataset, TrainingConfig, default_renderer_factory, make_optimizer, train_step

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
dev = torch.device('cuda:0')
out = {'msssim_available': T.SSIM_AVAILABLE}
for name, K, S, Bn in (("config2_shape", 6, 256, 16), ("config3_shape", 24, 512, 8)):
    row = {}
    for backend in ("msssim", "hip"):
        cfg = TrainingConfig(batch_size=Bn, image_size=S, gaussians_per_patch=K, device='cuda:0', ssim_backend=backend)
        torch.manual_seed(0)
        model = PatchGaussianDecoder(cfg.feature_dim, K, grid=cfg.feature_size).to(dev)
        renderer, camera = default_renderer_factory(cfg, dev)
        opt = make_optimizer(model, cfg)
        dp = DPContext(device=dev)
        data = SyntheticDataset(4 * Bn, cfg)
        batches = [data.batch(list(range(i * Bn, (i + 1) * Bn)), dev) for i in range(4)]
        rng = np.random.RandomState(0)
        t_spin = time.perf_counter()
        while time.perf_counter() - t_spin < 0.5:
            for i in range(5):
                train_step(model, renderer, camera, batches[i % 4], opt, cfg, dp, pose_rng=rng)
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            res = train_step(model, renderer, camera, batches[i % 4], opt, cfg, dp, pose_rng=rng)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        cfg_g = TrainingConfig(batch_size=Bn, image_size=S, gaussians_per_patch=K, device='cuda:0', ssim_backend=backend, hip_graph=True)
        opt_g = make_optimizer(model, cfg_g)
        g = GraphedTrainStep(model, renderer, camera, opt_g, cfg_g, dp, batches[0])
        for i in range(3):
            g(batches[i % 4])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            g(batches[i % 4])
        torch.cuda.synchronize()
        gms = (time.perf_counter() - t0) / steps * 1e3
        row[backend] = dict(step_ms=round(ms, 3), step_ms_hip_graph=round(gms, 3), terms=sorted(res.to_host() or {}))
    row['hip_term_cost_ms'] = round(row['hip']['step_ms'] - row['msssim']['step_ms'], 3)
    row['hip_term_cost_ms_hip_graph'] = round(row['hip']['step_ms_hip_graph'] - row['msssim']['step_ms_hip_graph'], 3)
    out[name] = dict(gaussians=37 * 37 * K, resolution=S, images=Bn, **row)
print(json.dumps(out))
