"""What the decoder costs per training step: fresnel_amd.train.train_step at the config-2 shape (as train_step_ssim.py: 37 x 37 x 6 =
8214 Gaussians, 256 x 256, 16 images) with the stand-in decoder (the default path, unchanged) and with --decoder direct under
--head_backend torch, hip, then torch again (the spread), eager and replayed from one captured graph.
usage: python scratch/profile/train_step_decoder_head.py [steps] [out.json]  -> one JSON line"""
import json, sys, time
import numpy as np, torch
sys.path.insert(0, '.')
from fresnel_amd.dist import DPContext
from fresnel_amd.train import GraphedTrainStep, SyntheticDataset, TrainingConfig, default_renderer_factory, make_decoder, make_optimizer, train_step

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
dev = torch.device('cuda:0')
K, S, Bn = 6, 256, 16
legs = (("standin", "standin", "torch"), ("direct_torch", "direct", "torch"), ("direct_hip", "direct", "hip"),
        ("direct_torch_again", "direct", "torch"))
row = {}
for name, decoder, backend in legs:
    kw = dict(batch_size=Bn, image_size=S, gaussians_per_patch=K, device='cuda:0', decoder=decoder, head_backend=backend)
    cfg = TrainingConfig(**kw)
    torch.manual_seed(0)
    model = make_decoder(cfg).to(dev)
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
    row[name] = dict(step_ms=round(ms, 3), step_ms_hip_graph=round(gms, 3), terms=sorted(res.to_host() or {}),
                     parameters=sum(p.numel() for p in model.parameters()))
    print(name, row[name], flush=True)
out = dict(config2_shape=dict(gaussians=37 * 37 * K, resolution=S, images=Bn, steps_per_leg=steps, **row))
out["config2_shape"]["hip_head_saves_ms"] = round(row["direct_torch"]["step_ms"] - row["direct_hip"]["step_ms"], 3)
out["config2_shape"]["hip_head_saves_ms_hip_graph"] = round(row["direct_torch"]["step_ms_hip_graph"] - row["direct_hip"]["step_ms_hip_graph"], 3)
out["config2_shape"]["torch_spread_ms"] = round(abs(row["direct_torch"]["step_ms"] - row["direct_torch_again"]["step_ms"]), 3)
print(json.dumps(out))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
