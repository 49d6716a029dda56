"""Fixtures of the consistency view synthesizer's losses and training step: the reference's QualityAwareCVSLoss
(scripts/models/quality_aware_losses.py), ConsistencyLoss (scripts/models/consistency_view_synthesis.py, CVS:844-941) and the body of
CVSTrainer.train_step (scripts/training/train_cvs.py:457-528) run on the CPU, once in fp32 and once in fp64 on the same numbers.  Runs
only where the reference is present (FRESNEL_REFERENCE = its checkout); the fixtures hold data only, in the layout of
tests/golden/make_goldens_cvs_unet.py (`record_runs`: the fp32 run as it is, d64.<key> / u64.<key> the fp64 run as int16 counts).

  Q1  QualityAwareCVSLoss(lambda_perceptual=0, lambda_boundary=0.7, lambda_gradient=0.3), (2, 3, 5, 7), with ema: all four terms.
      Inputs from tests/cvs_loss_checker.make_case (ties of pred with target, ema and its own neighbours; depth pairs whose difference
      EQUALS the boundary threshold).  Stored: mask (compute_quality_mask), loss.<key>, grad.pred of the total
  Q2  QualityAwareCVSLoss(lambda_perceptual=0, use_quality_weighting=False), (3, 1, 8, 8), consistency_weight_override 0.3
  C1  ConsistencyLoss() under seed 1361 on the U1 synthesizer (seed 1340, tests/golden/make_goldens_cvs_unet.py) and its EMA copy,
      B 2, timesteps (0, 999): loss.<key>, x0_pred, grad.x0_pred of the total, and what the EMA U-Net was given: x_t_prev, t_prev
  T1  two steps of train_step's body on the quality-aware path (U1, B 2, AdamW lr 1e-4 weight_decay 0.01, epoch 0 of 100: the
      progressive weight 0.1), the random draws of the forwards under torch.manual_seed(1380) -- timesteps from randint, noise from
      randn_like, which BOTH runs draw in fp32 so that the fp64 run sees the same numbers: step<k>.<loss key>, and afterwards
      param.<name> / ema.<name> of every wavelength and of a few 1-D parameters
"""
import hashlib
import json
import os
import sys

REF = os.environ.get("FRESNEL_REFERENCE", "")
if not os.path.isdir(os.path.join(REF, "scripts")):
    sys.exit("make_goldens_cvs_loss.py: set FRESNEL_REFERENCE to a checkout of the reference; fixtures can only be generated where it is present")
sys.path.insert(0, os.path.join(REF, "scripts"))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import models.consistency_view_synthesis as cvs  # noqa: E402  (the reference, read-only)
import models.quality_aware_losses as qal  # noqa: E402
from cvs_loss_checker import make_case  # noqa: E402  (the input recipe)

torch.set_num_threads(8)
META = dict(torch=torch.__version__, numpy=np.__version__, device="cpu")
CAP = os.path.getsize(os.path.join(HERE, "attn_A1.npz"))
U1_CONFIG = dict(image_size=16, base_channels=32, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(8,),
                 cross_attention_dim=384, time_embed_dim=32, pose_embed_dim=32)
U1_SEED = 1340
TRACKED = ("unet.out_conv.0.weight", "unet.out_conv.2.bias", "unet.time_embed.1.bias", "pose_encoder.ray_proj.0.bias")


def grid(t, step):
    return torch.round(t / step) * step


def to_dtype(module, dtype):
    module = module.to(dtype)
    for sub in module.modules():   # GroupNorm32 computes in float32 whatever it is given (x.float()): its parameters stay fp32
        if isinstance(sub, cvs.GroupNorm32):
            sub.float()
    return module


def record_runs(rec, run):
    """run(dtype) -> {key: tensor}: the fp32 run as it is, the fp64 run as int16 differences."""
    for dtype in (torch.float32, torch.float64):
        torch.set_default_dtype(dtype)   # (the pose encoder builds its ray origin with torch.zeros)
        try:
            res = run(dtype)
        finally:
            torch.set_default_dtype(torch.float32)
        for k, v in res.items():
            v = v.detach().numpy()
            if dtype is torch.float32:
                rec[k] = v.astype(np.float32)
            else:
                unit = float(np.abs(v).max()) * 2.0 ** -28
                counts = np.rint((v - rec[k].astype(np.float64)) / unit) if unit > 0 else np.zeros(v.shape)
                assert np.abs(counts).max() <= 32767, f"{k}: fp32 too far from fp64"
                rec["d64." + k], rec["u64." + k] = counts.astype(np.int16), np.float64(unit)


def header(kind, ctor, **more):
    rec = dict(kind=np.array(kind), ctor=np.array(json.dumps(ctor)))
    rec.update({k: np.array(v) for k, v in more.items()})
    for k, v in META.items():
        rec["meta_" + k] = np.array(v)
    return rec


def quality_fixture(ctor, shape, seed, with_ema, override):
    case = make_case(shape, seed, edge_pair=True)
    rec = header("quality", ctor, override=json.dumps(override))
    rec.update({k: case[k] for k in ("pred", "target", "depth")})
    if with_ema:
        rec["ema"] = case["ema"]

    def run(dtype):
        loss_fn = qal.QualityAwareCVSLoss(**ctor)
        pred = torch.from_numpy(case["pred"]).to(dtype).requires_grad_(True)
        target, depth = (torch.from_numpy(case[k]).to(dtype) for k in ("target", "depth"))
        ema = torch.from_numpy(case["ema"]).to(dtype) if with_ema else None
        losses = loss_fn(pred, target, depth, ema, consistency_weight_override=override)
        losses["total"].backward()
        res = {"loss." + k: v for k, v in losses.items()}
        res.update({"grad.pred": pred.grad, "mask": qal.compute_quality_mask(depth, ctor.get("quality_threshold", 0.01),
                                                                            ctor.get("quality_sharpness", 100.0))})
        return res

    record_runs(rec, run)
    return rec


def synth_inputs(g, Bn=2, S=16):
    features = grid(torch.randn(Bn, 3, 3, 384, generator=g), 0.125)
    axis = torch.nn.functional.normalize(torch.randn(Bn, 3, generator=g), dim=-1)
    angle = torch.tensor([0.4, -0.9])
    K = torch.zeros(Bn, 3, 3)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -axis[:, 2], axis[:, 1], -axis[:, 0]
    K = K - K.transpose(1, 2)
    R_rel = torch.eye(3) + torch.sin(angle)[:, None, None] * K + (1 - torch.cos(angle))[:, None, None] * (K @ K)   # Rodrigues
    t_rel = grid(torch.randn(Bn, 3, generator=g), 0.125)
    target = torch.clamp(grid(0.5 * torch.randn(Bn, 3, S, S, generator=g), 1.0 / 256), -1, 1)
    return features, R_rel, t_rel, target


def build_u1(dtype):
    torch.set_default_dtype(torch.float32)
    torch.manual_seed(U1_SEED)
    model = cvs.ConsistencyViewSynthesizer(cvs.CVSConfig(**U1_CONFIG))
    torch.set_default_dtype(dtype)
    return to_dtype(model, dtype)


def consistency_fixture(seed):
    g = torch.Generator().manual_seed(seed)
    features, R_rel, t_rel, target = synth_inputs(g)
    noisy = grid(torch.randn(2, 3, 16, 16, generator=g), 1.0 / 256)
    timestep = torch.tensor([0, U1_CONFIG.get("num_timesteps", 1000) - 1])
    ctor = dict(lambda_consistency=1.0, lambda_reconstruction=1.0, lambda_perceptual=0.5)
    torch.manual_seed(seed)
    rec = header("consistency", ctor, seed=np.int32(seed), model_seed=np.int32(U1_SEED), model_ctor=json.dumps(U1_CONFIG))
    for k, v in cvs.ConsistencyLoss(**ctor).state_dict().items():
        rec["sd0sha." + k] = np.array(hashlib.sha256(v.numpy().tobytes()).hexdigest())
    rec.update(features=features.numpy(), R_rel=R_rel.numpy(), t_rel=t_rel.numpy(), target=target.numpy(), noisy=noisy.numpy(),
               timestep=timestep.numpy())

    def run(dtype):
        model = build_u1(dtype).eval()
        ema = to_dtype(cvs.create_ema_model(model), dtype).eval()
        torch.set_default_dtype(torch.float32)
        torch.manual_seed(seed)
        loss_fn = cvs.ConsistencyLoss(**ctor).to(dtype)
        torch.set_default_dtype(dtype)
        seen = {}

        def see(mod, args):   # what the EMA U-Net is given; the loss hands it t_prev.float(), which the fp64 run casts to its dtype
            seen.update(x_t_prev=args[0].detach().clone(), t_prev=args[1].detach().clone())
            return (args[0], args[1].to(args[0].dtype), *args[2:])

        hook = ema.unet.register_forward_pre_hook(see)
        f, R, t, tg, nz = (v.to(dtype) for v in (features, R_rel, t_rel, target, noisy))
        x0_pred = model.unet(nz, timestep.to(dtype), model.image_adapter(f), model.pose_encoder(R, t))
        x0_pred.retain_grad()
        out = dict(x0_pred=x0_pred, target=tg, noisy=nz, noise=torch.zeros_like(nz), timestep=timestep)
        losses = loss_fn(out, ema_model=ema, model=model, input_features=f, R_rel=R, t_rel=t)
        hook.remove()
        losses["total"].backward()
        res = {"loss." + k: v for k, v in losses.items()}
        res.update({"x0_pred": x0_pred, "grad.x0_pred": x0_pred.grad, "x_t_prev": seen["x_t_prev"], "t_prev": seen["t_prev"].to(dtype)})
        return res

    record_runs(rec, run)
    return rec


def one_step(model, ema, loss_fn, optimizer, batch, epoch=0, epochs=100, clip=1.0, decay=0.9999):
    """CVSTrainer.train_step, quality-aware path (train_cvs.py:457-528), without the .item() at its end."""
    i, f, R, t, tg, d = batch
    model.train()
    output = model(i, f, R, t, target_image=tg)
    with torch.no_grad():
        ema_output = ema(i, f, R, t, target_image=tg)
    weight = qal.get_consistency_weight_schedule(epoch, epochs, schedule_type='progressive')
    losses = loss_fn(cvs_pred=output['x0_pred'], synthetic_target=tg, synthetic_depth=d, ema_pred=ema_output['x0_pred'],
                     consistency_weight_override=weight)
    optimizer.zero_grad()
    losses['total'].backward()
    torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
    optimizer.step()
    cvs.update_ema(model, ema, decay)
    return losses


def train_fixture(seed, steps=2):
    g = torch.Generator().manual_seed(seed)
    features, R_rel, t_rel, target = synth_inputs(g)
    input_image = torch.clamp(grid(0.5 * torch.randn(2, 3, 16, 16, generator=g), 1.0 / 256), -1, 1)
    depth = torch.from_numpy(make_case((2, 3, 16, 16), seed)["depth"])
    config = dict(epochs=100, lr=1e-4, weight_decay=0.01, gradient_clip=1.0, ema_decay=0.9999, lambda_consistency=1.0,
                  lambda_reconstruction=1.0, lambda_perceptual=0.5, quality_weighting=True, progressive_consistency=True,
                  lambda_boundary=0.0, lambda_gradient=0.0)
    rec = header("train", config, seed=np.int32(seed), model_seed=np.int32(U1_SEED), model_ctor=json.dumps(U1_CONFIG), steps=np.int32(steps))
    rec.update(input_image=input_image.numpy(), features=features.numpy(), R_rel=R_rel.numpy(), t_rel=t_rel.numpy(),
               target_image=target.numpy(), target_depth=depth.numpy())

    def run(dtype):
        model = build_u1(dtype)
        ema = to_dtype(cvs.create_ema_model(model), dtype)
        loss_fn = qal.QualityAwareCVSLoss(lambda_l1=config["lambda_reconstruction"], lambda_perceptual=config["lambda_perceptual"],
                                          lambda_consistency=config["lambda_consistency"], lambda_boundary=config["lambda_boundary"],
                                          lambda_gradient=config["lambda_gradient"], use_quality_weighting=config["quality_weighting"])
        optimizer = torch.optim.AdamW(model.parameters(), lr=config["lr"], weight_decay=config["weight_decay"])
        i, f, R, t, tg, d = (v.to(dtype) for v in (input_image, features, R_rel, t_rel, target, depth))
        torch.manual_seed(seed)
        res = {}
        real_randn_like = torch.randn_like
        torch.randn_like = lambda x: real_randn_like(x.float()).to(x.dtype)   # the fp64 run adds the fp32 run's noise
        try:
            losses_of = [one_step(model, ema, loss_fn, optimizer, (i, f, R, t, tg, d)) for _ in range(steps)]
        finally:
            torch.randn_like = real_randn_like
        for k, losses in enumerate(losses_of):
            res.update({f"step{k}.{name}": v.detach() for name, v in losses.items()})
        for prefix, module in (("param.", model), ("ema.", ema)):
            named = dict(module.named_parameters())
            for name in [n for n in named if n.endswith("wavelength")] + [n for n in TRACKED if n in named]:
                res[prefix + name] = named[name]
        return res

    record_runs(rec, run)
    return rec


def main():
    cases = [
        ("cvs_loss_Q1", lambda: quality_fixture(dict(lambda_perceptual=0.0, lambda_boundary=0.7, lambda_gradient=0.3), (2, 3, 5, 7), 1350,
                                               True, None)),
        ("cvs_loss_Q2", lambda: quality_fixture(dict(lambda_perceptual=0.0, use_quality_weighting=False), (3, 1, 8, 8), 1355, True, 0.3)),
        ("cvs_loss_C1", lambda: consistency_fixture(1361)),
        ("cvs_loss_T1", lambda: train_fixture(1380)),
    ]
    for name, make in cases:
        rec = make()
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **rec)
        size = os.path.getsize(path)
        assert size <= CAP, f"{name}: {size} bytes is larger than attn_A1.npz ({CAP})"
        worst = max((float(np.abs(rec[k]).max()) * 2.0 ** -28 for k in rec if k.startswith("d64.")), default=0.0)
        print(f"{name}: {size / 1024:.0f} KB, {sum(k.startswith('d64.') for k in rec)} tensors, fp32 vs fp64 up to {worst:.1e} of a maximum")


if __name__ == "__main__":
    main()
