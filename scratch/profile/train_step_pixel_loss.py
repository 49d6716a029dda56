"""What the fused per-pixel losses change per training step: fresnel_amd.train.train_step at config 2 / config 3 shapes (as
train_step_bench.py) with pixel_loss_backend "torch" and "hip" and IDENTICAL terms, eager and replayed from one captured graph.
Two term sets: the default (L1 + depth) and everything (--use_vlm_guidance --use_fresnel_zones --boundary_weight 0.1).  The
torch leg runs twice, before and after the hip leg: the difference of the two is the spread the comparison has to beat.
usage: python scratch/profile/train_step_pixel_loss.py [steps]  -> one JSON line"""
import json, sys, time
import numpy as np, torch
sys.path.insert(0, '.')
from fresnel_amd.dist import DPContext
from fresnel_amd.train import GraphedTrainStep, PatchGaussianDecoder, SyntheticDataset, TrainingConfig, default_renderer_factory, make_optimizer, train_step

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
dev = torch.device('cuda:0')
TERMS = {'rgb_depth': {}, 'all_terms': dict(use_vlm_guidance=True, use_fresnel_zones=True, boundary_weight=0.1)}
out = {}
for name, K, S, Bn in (("config2_shape", 6, 256, 16), ("config3_shape", 24, 512, 8)):
    shape_row = {}
    for tname, tkw in TERMS.items():
        row = {}
        for leg, backend in (("torch", "torch"), ("hip", "hip"), ("torch_again", "torch")):
            kw = dict(batch_size=Bn, image_size=S, gaussians_per_patch=K, device='cuda:0', pixel_loss_backend=backend, **tkw)
            cfg = TrainingConfig(**kw)
            torch.manual_seed(0)
            model = PatchGaussianDecoder(cfg.feature_dim, K, grid=cfg.feature_size, use_fresnel_zones=cfg.use_fresnel_zones,
                                         num_fresnel_zones=cfg.num_fresnel_zones).to(dev)
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
            cfg_g = TrainingConfig(hip_graph=True, **kw)
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
            row[leg] = dict(step_ms=round(ms, 3), step_ms_hip_graph=round(gms, 3), terms=sorted(res.to_host() or {}))
        for key in ("step_ms", "step_ms_hip_graph"):
            spread = abs(row["torch"][key] - row["torch_again"][key])
            best_torch = min(row["torch"][key], row["torch_again"][key])
            row["summary_" + key] = dict(torch_spread=round(spread, 3), hip_minus_best_torch=round(row["hip"][key] - best_torch, 3),
                                         hip_slower_than_spread=bool(row["hip"][key] - max(row["torch"][key], row["torch_again"][key]) > spread))
        shape_row[tname] = row
    out[name] = dict(gaussians=37 * 37 * K, resolution=S, images=Bn, **shape_row)
print(json.dumps(out))
