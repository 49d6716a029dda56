"""Fixtures of the consistency view synthesizer's U-Net: the reference's ResBlock and ConsistencyViewSynthesizer
(scripts/models/consistency_view_synthesis.py, CVS:90-134 and 477-837) run on the CPU, once in fp32 and once in fp64 on the same
numbers.  Runs only where the reference is present (FRESNEL_REFERENCE = its checkout); the fixtures hold data only, in the layout of
tests/golden/make_goldens_cvs.py:

    kind, ctor           "res" (ResBlock) | "synth" (ConsistencyViewSynthesizer); the constructor's / the CVSConfig's keyword
                         arguments, as JSON
    seed                 torch.manual_seed(seed) before the constructor gives the initial state dict
    sd0sha.<key>         SHA-256 of the bytes of every tensor of that initial state dict
    sd.<key>             (res only) the state dict the runs used: the initial one with the GroupNorm weights and biases perturbed, on
                         a binary grid.  The synthesizer's runs use the INITIAL state dict, which the digests pin down
    x, t_emb | features, R_rel, t_rel, noisy, timestep      the inputs; g the upstream gradient of the output
    out, grad.<input>, grad.sd.<parameter>                   the fp32 run: output and gradients of sum(out x g).  The synthesizer
                         stores image_cond, pose_cond and out = unet(noisy, timestep, image_cond, pose_cond), the gradients to noisy
                         and features, and the gradients of every 1-D parameter and of every wavelength
    cancelling           JSON list of the gradients NOT stored because they are mathematically zero (biases whose every consumer
                         is a GroupNorm with one channel per group): both runs hold rounding noise there
    d64.<key>, u64.<key>  the fp64 run of every <key> above as int16 counts of u64.<key> = max|fp64 value| x 2^-28 away from the
                          fp32 run.  In the fp64 run every GroupNorm32 keeps fp32 parameters: the class casts its input to float32

  R1  ResBlock(32, 64, time_embed_dim=16), B 2, 5 x 7: a skip convolution, one and two channels per group
  R2  ResBlock(96, 96, 16), B 1, 3 x 5: the identity skip, three channels per group (groups start at odd offsets)
  U1  ConsistencyViewSynthesizer(CVSConfig(image_size=16, base_channels=32, channel_mult=(1, 2), num_res_blocks=1,
      attention_resolutions=(8,), cross_attention_dim=384, time_embed_dim=32, pose_embed_dim=32)), B 2, features (2, 3, 3, 384): the
      second encoder stage runs at 8 x 8 and has an AttentionBlock besides mid_attn.  (cross_attention_dim has to be 384: the image
      adapter adds its position embeddings, out_dim wide, to the 384-wide features.)  image_cond is (2, 256, 384), larger than the
      cap on its own: the fixture stores every eighth token, image_cond[:, ::8]; all 256 enter out and grad.features
  cvs_keys.json  the ordered state-dict keys and shapes of the default-config synthesizer, built on torch.device("meta")
"""
import hashlib
import json
import os
import sys

REF = os.environ.get("FRESNEL_REFERENCE", "")
if not os.path.isdir(os.path.join(REF, "scripts")):
    sys.exit("make_goldens_cvs_unet.py: set FRESNEL_REFERENCE to a checkout of the reference; fixtures can only be generated where it is present")
sys.path.insert(0, os.path.join(REF, "scripts"))
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import models.consistency_view_synthesis as cvs  # noqa: E402  (the reference, read-only)

torch.set_num_threads(8)
META = dict(torch=torch.__version__, numpy=np.__version__, device="cpu")
CAP = os.path.getsize(os.path.join(HERE, "attn_A1.npz"))
U1_CONFIG = dict(image_size=16, base_channels=32, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(8,),
                 cross_attention_dim=384, time_embed_dim=32, pose_embed_dim=32)


def grid(t, step):
    return torch.round(t / step) * step


def build(kind, ctor):
    return cvs.ResBlock(**ctor) if kind == "res" else cvs.ConsistencyViewSynthesizer(cvs.CVSConfig(**ctor))


def to_dtype(module, dtype):
    module = module.to(dtype)
    for sub in module.modules():   # GroupNorm32 computes in float32 whatever it is given (x.float()): its parameters stay fp32
        if isinstance(sub, cvs.GroupNorm32):
            sub.float()
    return module


def record_runs(rec, run):
    """run(dtype) -> {key: tensor}: the fp32 run as it is, the fp64 run as int16 differences."""
    for dtype in (torch.float32, torch.float64):
        for k, v in run(dtype).items():
            v = v.detach().numpy()
            if dtype is torch.float32:
                rec[k] = v
            else:
                unit = float(np.abs(v).max()) * 2.0 ** -28
                counts = np.rint((v - rec[k].astype(np.float64)) / unit) if unit > 0 else np.zeros(v.shape)
                if np.abs(counts).max() > 32767:
                    # a per-channel constant whose every consumer is a GroupNorm with ONE channel per group (U1's 32-channel
                    # stages): the gradient is mathematically zero and both runs hold rounding noise.  Not stored; its name goes
                    # to `cancelling`
                    assert k.endswith(".bias") and np.abs(v).max() < 1e-4, f"{k}: fp32 too far from fp64"
                    del rec[k]
                    rec.setdefault("cancelling", []).append(k)
                    continue
                rec["d64." + k], rec["u64." + k] = counts.astype(np.int16), np.float64(unit)
    rec["cancelling"] = np.array(json.dumps(rec.get("cancelling", [])))


def header(kind, ctor, seed, module):
    rec = dict(kind=np.array(kind), ctor=np.array(json.dumps(ctor)), seed=np.int32(seed))
    for k, v in module.state_dict().items():
        rec["sd0sha." + k] = np.array(hashlib.sha256(v.numpy().tobytes()).hexdigest())
    for k, v in META.items():
        rec["meta_" + k] = np.array(v)
    return rec


def res_fixture(ctor, Bn, gh, gw, seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    module = build("res", ctor).eval()
    rec = header("res", ctor, seed, module)
    with torch.no_grad():
        for name, p in module.named_parameters():
            perturb = 0.25 * torch.randn(p.shape, generator=g) if name.startswith("norm") else 0.0
            p.copy_(grid(p + perturb, 1.0 / 128))
    x = grid(torch.randn(Bn, ctor["in_channels"], gh, gw, generator=g), 0.125)
    t_emb = grid(torch.randn(Bn, ctor["time_embed_dim"], generator=g), 0.125)
    up = grid(torch.randn(Bn, ctor["out_channels"], gh, gw, generator=g), 0.125)
    rec.update(x=x.numpy(), t_emb=t_emb.numpy(), g=up.numpy())
    for k, v in module.state_dict().items():
        rec["sd." + k] = v.numpy()

    def run(dtype):
        m = to_dtype(build("res", ctor).eval(), dtype)
        m.load_state_dict({k: v.to(m.state_dict()[k].dtype) for k, v in module.state_dict().items()})
        xi, ti = x.clone().to(dtype).requires_grad_(True), t_emb.clone().to(dtype).requires_grad_(True)
        out = m(xi, ti)
        (out * up.to(dtype)).sum().backward()
        res = {"out": out, "grad.x": xi.grad, "grad.t_emb": ti.grad}
        res.update({"grad.sd." + k: p.grad for k, p in m.named_parameters()})
        return res

    record_runs(rec, run)
    return rec


def synth_fixture(ctor, seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    module = build("synth", ctor).eval()
    rec = header("synth", ctor, seed, module)
    assert any(a is not None for a in list(module.unet.encoder_attns) + list(module.unet.decoder_attns))
    S = ctor["image_size"]
    features = grid(torch.randn(2, 3, 3, 384, generator=g), 0.125)
    axis = torch.nn.functional.normalize(torch.randn(2, 3, generator=g), dim=-1)
    angle = torch.tensor([0.4, -0.9])
    K = torch.zeros(2, 3, 3)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -axis[:, 2], axis[:, 1], -axis[:, 0]
    K = K - K.transpose(1, 2)
    R_rel = torch.eye(3) + torch.sin(angle)[:, None, None] * K + (1 - torch.cos(angle))[:, None, None] * (K @ K)   # Rodrigues
    t_rel = grid(torch.randn(2, 3, generator=g), 0.125)
    noisy = grid(torch.randn(2, 3, S, S, generator=g), 0.125)
    timestep = torch.tensor([37.0, 640.0])
    up = grid(torch.randn(2, 3, S, S, generator=g), 0.125)
    rec.update(features=features.numpy(), R_rel=R_rel.numpy(), t_rel=t_rel.numpy(), noisy=noisy.numpy(), timestep=timestep.numpy(),
               g=up.numpy())

    def run(dtype):
        m = to_dtype(build("synth", ctor).eval(), dtype)
        m.load_state_dict({k: v.to(m.state_dict()[k].dtype) for k, v in module.state_dict().items()})
        fi, ni = features.clone().to(dtype).requires_grad_(True), noisy.clone().to(dtype).requires_grad_(True)
        image_cond = m.image_adapter(fi)
        # (the pose encoder builds its ray origin with torch.zeros: the default dtype has to be the run's)
        torch.set_default_dtype(dtype)
        try:
            pose_cond = m.pose_encoder(R_rel.to(dtype), t_rel.to(dtype))
        finally:
            torch.set_default_dtype(torch.float32)
        out = m.unet(ni, timestep.to(dtype), image_cond, pose_cond)
        (out * up.to(dtype)).sum().backward()
        res = {"image_cond": image_cond[:, ::8], "pose_cond": pose_cond, "out": out, "grad.noisy": ni.grad, "grad.features": fi.grad}
        res.update({"grad.sd." + k: p.grad for k, p in m.named_parameters() if p.dim() == 1 or k.endswith("wavelength")})
        return res

    record_runs(rec, run)
    return rec


def main():
    cases = [
        ("cvs_R1", lambda: res_fixture(dict(in_channels=32, out_channels=64, time_embed_dim=16), 2, 5, 7, 1300)),
        ("cvs_R2", lambda: res_fixture(dict(in_channels=96, out_channels=96, time_embed_dim=16), 1, 3, 5, 1320)),
        ("cvs_U1", lambda: synth_fixture(U1_CONFIG, 1340)),
    ]
    for name, make in cases:
        rec = make()
        # R2's two 96 x 96 x 3 x 3 weight gradients are full-entropy fp32 and together exceed the cap: conv2's goes to a file of its
        # own, cvs_R2_convgrads.npz, which the tests read together with cvs_R2.npz
        parts = {name: rec}
        if name == "cvs_R2":
            moved = [k for k in rec if k.endswith("grad.sd.conv2.weight")]   # with its d64. and u64.
            parts = {name: {k: v for k, v in rec.items() if k not in moved}, name + "_convgrads": {k: rec[k] for k in moved}}
        for part, arrays in parts.items():
            path = os.path.join(HERE, part + ".npz")
            np.savez_compressed(path, **arrays)
            size = os.path.getsize(path)
            assert size <= CAP, f"{part}: {size} bytes is larger than attn_A1.npz ({CAP})"
            print(f"{part}: {size / 1024:.0f} KB")
        print(f"{name}: |out| max {np.abs(rec['out']).max():.3f}, fp32 vs fp64 {np.abs(rec['d64.out']).max() * 2.0 ** -28:.1e}")
    with torch.device("meta"):
        default = cvs.ConsistencyViewSynthesizer()
    keys = [[k, list(v.shape)] for k, v in default.state_dict().items()]
    with open(os.path.join(HERE, "cvs_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
        f.write("\n")
    print(f"cvs_keys.json: {len(keys)} keys")


if __name__ == "__main__":
    main()
