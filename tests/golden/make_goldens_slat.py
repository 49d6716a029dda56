"""Fixtures of the distillation decoders and their Gaussian head: the reference's DirectSLatDecoder and MLPSLatDecoder
(scripts/models/direct_slat_decoder.py) run on the CPU in eval mode.  Runs only where the reference is present (FRESNEL_REFERENCE =
its checkout); the fixtures hold data only:

    ctor            the constructor's keyword arguments, as JSON                      class_name
    sd.<key>        the state dict
    in.<name>       features, coords and (DirectSLatDecoder) coord_mask
    raw             the output of gaussian_head.head, captured by a forward hook, as (B, N, G, 14)   (not S2: the reference runs the
                    head once per image there)
    out.<name>      every entry of the returned dict (MLPSLatDecoder's tensor as out.gaussians)      g.<name>  its upstream gradient
    grad.raw, grad.features, grad.sd.<parameter>     gradients of sum_name sum(out.<name> x g.<name>); zeros where autograd gave none

  S1 DirectSLatDecoder   feature_dim 12, hidden 20 (positional split 6 / 6 / 8), 4 heads, 2 layers, G 3; B 2, N 7, M 5; two padded voxels
                         in image 1; coordinates from [-4, 70): both coordinate clamps act; scale_factor -0.3.  Also init.<key>: the
                         state dict right after construction under torch.manual_seed(init_seed)
  S2 S1's model with apply_occupancy_mask=True: out.gaussians.<b> per image, out.n_gaussians, out.occupancy_mask, out.occupancy_logits
  S3 MLPSLatDecoder      G 8
  S4 DirectSLatDecoder   predict_occupancy=False, hidden 12, N 1030: over the 1024-query chunk of CrossAttention

The last layer of the head MLP is scaled up (`last_gain`, to a raw spread of `spread`) and its bias randomised so that raw crosses
+-10 and positions and scales meet their clamps; the occupancy head's last layer likewise, so that the mask is mixed.  A seed is
taken only if no gate is within reach of a GPU GEMM's last bits: no raw element within 1e-3 of +-10, no unclamped position within
1e-3 of +-1, no unclamped scale within 1e-3 (relative) of 1e-4 or 1, no quaternion norm below 1e-3 and (S2) no sigmoid(logit)
within 1e-3 of the threshold.  S4's 14 420 raw elements make a clean seed rare: its search walks through some 1e5 seeds (minutes).
"""
import json
import os
import sys

REF = os.environ.get("FRESNEL_REFERENCE", "")
if not os.path.isdir(os.path.join(REF, "scripts")):
    sys.exit("make_goldens_slat.py: set FRESNEL_REFERENCE to a checkout of the reference; fixtures can only be generated where it is present")
sys.path.insert(0, os.path.join(REF, "scripts"))
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import models.direct_slat_decoder as dsd  # noqa: E402  (the reference, read-only)

torch.set_num_threads(8)
META = dict(torch=torch.__version__, numpy=np.__version__, device="cpu")


def margins_ok(raw, coords, pos_gain, scale_factor):
    """The seed rule on the head's inputs; raw (B, N, G, 14)."""
    r = raw.double()
    if bool(((r.abs() - 10.0).abs() < 1e-3).any()):
        return False
    r = r.clamp(-10, 10)
    centre = coords[:, :, 1:4].double().clamp(0, 63) / 64.0 * 2 - 1
    u = centre.unsqueeze(2) + torch.tanh(r[..., :3]) * float(pos_gain)
    if bool(((u.abs() - 1.0).abs() < 1e-3).any()):
        return False
    v = F.softplus(r[..., 3:6]) * abs(float(scale_factor))
    if bool(((v / 1e-4 - 1).abs() < 1e-3).any()) or bool(((v - 1).abs() < 1e-3).any()):
        return False
    return not bool((r[..., 6:10].norm(dim=-1) < 1e-3).any())


def build(cls, ctor, seed):
    torch.manual_seed(seed)
    model = getattr(dsd, cls)(**ctor).eval()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    return model, init


def widen(model, probe, spread, scale_factor, g):
    """Scale the head's last layer to a raw spread of `spread` on the inputs `probe`, randomise its bias; mix the occupancy mask."""
    captured = {}
    h = model.gaussian_head.head.register_forward_hook(lambda _m, _i, out: captured.update(raw=out))
    with torch.no_grad():
        model(*probe)
        last = model.gaussian_head.head[-1]
        gain = spread / float(captured["raw"].std())
        last.weight.mul_(gain)
        last.bias.copy_(torch.randn(last.bias.shape, generator=g) * 2.0)
        if scale_factor is not None:
            model.gaussian_head.scale_factor.fill_(scale_factor)
        occ = getattr(model, "occupancy_head", None)
        if occ is not None:
            occ.mlp[-1].weight.mul_(40.0)
    h.remove()
    return gain


def inputs(Bn, N, M, feature_dim, padded, g):
    features = torch.randn(Bn, M, feature_dim, generator=g)
    coords = torch.randint(-4, 70, (Bn, N, 4), generator=g)
    coords[:, :, 0] = torch.arange(Bn).unsqueeze(1)
    coord_mask = torch.ones(Bn, N, dtype=torch.bool)
    if padded:
        coord_mask[1, -padded:] = False
    return features, coords, coord_mask


def run(cls, ctor, shape, seed, spread, scale_factor=None, gated=False):
    model, init = build(cls, ctor, seed)
    g = torch.Generator().manual_seed(seed + 1)
    features, coords, coord_mask = inputs(*shape, ctor["feature_dim"], 2 if cls == "DirectSLatDecoder" and shape[1] < 100 else 0, g)
    direct = cls == "DirectSLatDecoder"
    args = (features, coords, coord_mask) if direct else (features, coords)
    gain = widen(model, args, spread, scale_factor, g)
    rec = dict(class_name=np.array(cls), ctor=np.array(json.dumps(ctor)), seed=np.int32(seed), last_gain=np.float32(gain))
    rec["in.features"], rec["in.coords"] = features.numpy(), coords.numpy()
    if direct:
        rec["in.coord_mask"] = coord_mask.numpy()
    for k, v in model.state_dict().items():
        rec["sd." + k] = v.numpy()
    for k, v in META.items():
        rec["meta_" + k] = np.array(v)
    head = model.gaussian_head
    Gn = head.num_gaussians
    if gated:
        with torch.no_grad():
            out = model(features, coords, coord_mask, apply_occupancy_mask=True)
        p = torch.sigmoid(out["occupancy_logits"])
        ok = not bool(((p - model.occupancy_threshold).abs() < 1e-3).any())
        keep = out["occupancy_mask"] & coord_mask
        ok = ok and 0 < int(keep.sum()) < int(coord_mask.sum())
        for b, t in enumerate(out["gaussians"]):
            rec[f"out.gaussians.{b}"] = t.numpy()
        rec["out.n_gaussians"] = np.array(out["n_gaussians"], np.int32)
        rec["out.occupancy_mask"] = out["occupancy_mask"].numpy()
        rec["out.occupancy_logits"] = out["occupancy_logits"].numpy()
        return rec, ok, init
    features.requires_grad_(True)
    captured = {}

    def hook(_m, _i, out):
        out.retain_grad()
        captured["raw"] = out

    h = head.head.register_forward_hook(hook)
    out = model(*args)
    h.remove()
    if torch.is_tensor(out):
        out = {"gaussians": out}
    ups = {k: torch.randn(v.shape, generator=g) for k, v in out.items()}
    sum((out[k] * ups[k]).sum() for k in out).backward()
    raw = captured["raw"]
    Bn, N = coords.shape[:2]
    rec["raw"] = raw.detach().reshape(Bn, N, Gn, 14).numpy()
    rec["grad.raw"] = raw.grad.reshape(Bn, N, Gn, 14).numpy()
    rec["grad.features"] = features.grad.numpy()
    for k, p in model.named_parameters():
        rec["grad.sd." + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    for k in out:
        rec["out." + k] = out[k].detach().numpy()
        rec["g." + k] = ups[k].numpy()
    ok = margins_ok(raw.detach().reshape(Bn, N, Gn, 14), coords, head.position_offset_scale.detach(), head.scale_factor.detach())
    return rec, ok, init


def main():
    s1 = dict(feature_dim=12, hidden_dim=20, num_layers=2, num_heads=4, num_gaussians_per_voxel=3)
    cases = [
        ("slat_S1", "DirectSLatDecoder", s1, (2, 7, 5), dict(spread=8.0, scale_factor=-0.3)),
        ("slat_S2", "DirectSLatDecoder", s1, (2, 7, 5), dict(spread=8.0, scale_factor=-0.3, gated=True)),
        ("slat_S3", "MLPSLatDecoder", dict(feature_dim=12, hidden_dim=20, num_layers=2, num_gaussians_per_voxel=8), (2, 9, 5),
         dict(spread=8.0, scale_factor=0.2)),
        ("slat_S4", "DirectSLatDecoder", dict(feature_dim=8, hidden_dim=12, num_layers=1, num_heads=2, num_gaussians_per_voxel=1,
                                              predict_occupancy=False), (1, 1030, 4), dict(spread=6.0)),
    ]
    seeds = {}
    for k, (name, cls, ctor, shape, kw) in enumerate(cases):
        seed = seeds["slat_S1"] if name == "slat_S2" else 900 + 20 * k   # S2 is S1's model
        tried = 0
        while True:
            rec, ok, init = run(cls, ctor, shape, seed, **kw)
            tried += 1
            if ok and name == "slat_S1":   # S1's seed has to serve S2 as well
                ok = run(cls, ctor, shape, seed, **dict(kw, gated=True))[1]
            if ok:
                break
            assert name != "slat_S2"
            seed += 1
        seeds[name] = seed
        if name == "slat_S1":
            rec["init_seed"] = np.int32(seed)
            for key, v in init.items():
                rec["init." + key] = v.numpy()
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **rec)
        note = f"raw std {rec['raw'].std():.2f}, clamped {float((np.abs(rec['raw']) > 10).mean()):.0%}" if "raw" in rec else \
            f"kept {rec['out.n_gaussians'].tolist()}"
        print(f"{name}: seed {seed} ({tried} tried), {os.path.getsize(path) / 1024:.0f} KB, {note}")


if __name__ == "__main__":
    main()
