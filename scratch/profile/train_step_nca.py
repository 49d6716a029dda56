"""What the NCA decoder's backend costs per training step: fresnel_amd.train.train_step under --experiment 5 --fast_mode (64 x 64,
256 importance-sampled Gaussians of 377, 16 NCA steps, 16 images, 384-channel 37 x 37 features) with --nca_backend torch, hip,
then torch again (the spread); eager only (the HFTS hand-off is not graph-captured).
usage: python scratch/profile/train_step_nca.py [steps] [out.json]  -> one JSON line"""
import json, sys, time
import numpy as np, torch
sys.path.insert(0, '.')
from fresnel_amd import train
from fresnel_amd.dist import DPContext
from fresnel_amd.handoff import HFTSConfig

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
dev = torch.device('cuda:0')
Bn = 16
row = {}
for name, backend in (("nca_torch", "torch"), ("nca_hip", "hip"), ("nca_torch_again", "torch"), ("nca_hip_again", "hip")):
    a = train.arg_parser().parse_args(["--experiment", "5", "--fast_mode", "--nca_backend", backend, "--head_backend", "hip",
                                       "--batch_size", str(Bn)])
    cfg = train.config_from_args(a)
    cfg.device = "cuda:0"
    hfts = HFTSConfig(fast_mode=True)
    res_px = hfts.get_effective_train_resolution(cfg.image_size)
    torch.manual_seed(0)
    model = train.make_decoder(cfg).to(dev).train()
    renderer, camera = train.default_renderer_factory(cfg, dev, res_px)
    opt = train.make_optimizer(model, cfg)
    dp = DPContext(device=dev)
    data = train.SyntheticDataset(4 * Bn, cfg)
    batches = [data.batch(list(range(i * Bn, (i + 1) * Bn)), dev) for i in range(4)]
    rng, gen = np.random.RandomState(0), torch.Generator(device=dev).manual_seed(7)
    kw = dict(hfts=hfts, epoch=0, train_res=res_px, pose_rng=rng, sample_gen=gen)
    t_spin = time.perf_counter()
    while time.perf_counter() - t_spin < 0.5:
        for i in range(5):
            train.train_step(model, renderer, camera, batches[i % 4], opt, cfg, dp, **kw)
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        res = train.train_step(model, renderer, camera, batches[i % 4], opt, cfg, dp, **kw)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    row[name] = dict(step_ms=round(ms, 3), terms=sorted(res.to_host() or {}), parameters=sum(p.numel() for p in model.parameters()))
    print(name, row[name], flush=True)
out = dict(experiment5_fast_mode=dict(points=cfg.n_spiral_points, nca_steps=cfg.nca_steps, neighbors=cfg.nca_neighbors,
                                      resolution=res_px, images=Bn, head_backend="hip", steps_per_leg=steps, **row))
o = out["experiment5_fast_mode"]
o["hip_nca_saves_ms"] = round(row["nca_torch"]["step_ms"] - row["nca_hip"]["step_ms"], 3)
o["spread_ms"] = round(max(abs(row["nca_torch"]["step_ms"] - row["nca_torch_again"]["step_ms"]),
                           abs(row["nca_hip"]["step_ms"] - row["nca_hip_again"]["step_ms"])), 3)
print(json.dumps(out))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
