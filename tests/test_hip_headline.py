"""GPU parity of the BENCHMARKED code paths against the CPU oracle.

The headline bench (BASELINE config 3 per GPU: 8 images of 32 768 Gaussians @512x512) takes the 128-entry depth
segments, the 4-part depth-split forward and the backward that re-bases part-local checkpoints; config 2 runs as
one B=16 launch; the "decoder-like" distribution of SURVEY §8(d) has 3x the overdraw with thousands of Gaussians
at the 64-px radius cap.  Each of these launches is compared here -- image, depth, all five gradients <= 1e-4 of
max, integer stages bit-exact -- with the oracle (DR:527-600, DR:582-667 restated in oracle/fgs_oracle.c).
"""
import numpy as np
import pytest
import torch

from helpers import rel_to_max, synth_decoder_like, synth_saag
from sweep_support import check_integer_stages as _check_integer_stages, hip_stages as _hip_stages
from test_hip_parity import TOL, _hip_render

pytestmark = pytest.mark.gpu
KEYS = ["positions", "scales", "rotations", "colors", "opacities"]


def _run_batch_and_check(per_image, S, check, bg=(0.0, 0.0, 0.0), seed=0, expect_seg_len=None, min_segments=0):
    """per_image: list of B tuples (pos, scale, quat, color, opacity); `check`: image indices compared with the
    oracle.  One batched HIP forward + backward, integer stages of the same launch shape."""
    from oracle import fgs_oracle as orc
    from fresnel_amd.renderer import Camera
    Bn = len(per_image)
    arrs = [np.stack([p[i] for p in per_image]) for i in range(5)]
    cam = Camera(0.8 * S, 0.8 * S, S / 2, S / 2, S, S)
    ocam = orc.make_camera(np.eye(4, dtype=np.float32), 0.8 * S, 0.8 * S, S / 2, S / 2, S, S)
    rs = np.random.RandomState(seed)
    gI = rs.standard_normal((Bn, 3, S, S)).astype(np.float32)
    gD = (rs.standard_normal((Bn, S, S)) * 0.1).astype(np.float32)
    st = _hip_stages(arrs, cam, S, S, bg)
    if expect_seg_len is not None:
        assert int(st["layout"].seg_len) == expect_seg_len
    lens = st["ranges"][:, :, 1] - st["ranges"][:, :, 0]
    assert lens.max() >= min_segments * int(st["layout"].seg_len), "test must cover tiles with several depth segments"
    assert st["counters"][1] == 0  # no duplicate overflow
    out = _hip_render(arrs, cam, S, S, bg, grads=(gI, gD))
    worst = {}
    for b in check:
        r = orc.render(*[a[b] for a in arrs], ocam, bg=bg)
        _check_integer_stages(st, b, r, S, S)
        go = orc.render_backward(r, gI[b], gD[b])
        errs = dict(image=rel_to_max(out["image"][b], r.image), depth=rel_to_max(out["depth"][b], r.depth))
        for k in KEYS:
            errs[k] = rel_to_max(out["grad_" + k][b], go[k])
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= TOL, (b, k, v)
        del r, go
    return worst, st


def test_config3_headline_launch_vs_oracle():
    """BASELINE config 3 per GPU, exactly the bench's launch: B = 8 images x 32 768 Gaussians @512x512,
    create_dummy_saag (TGD:760-778).  B*N > 200 000 -> 128-entry segments, k_blend_fwd_parts<4>, re-based
    checkpoints in k_composite_bwd.  Images 0 and 7 are compared with the oracle."""
    per = [synth_saag(32768, 3000 + i) for i in range(8)]
    worst, st = _run_batch_and_check(per, 512, check=[0, 7], seed=31, expect_seg_len=128, min_segments=4)
    print("config3 worst rel-to-max errors:", worst)


def test_config3_shape_two_images_vs_oracle():
    """Same per-image shape at B = 2 (the launch a 2-image shard makes: 64-entry segments)."""
    per = [synth_saag(32768, 3100 + i) for i in range(2)]
    _run_batch_and_check(per, 512, check=[1], seed=32, min_segments=4)


def test_config2_batch16_vs_oracle():
    """BASELINE config 2: 8 192 Gaussians @256x256, one B = 16 launch; images 0, 9 and 15 vs the oracle."""
    per = [synth_saag(8192, 2000 + i) for i in range(16)]
    _run_batch_and_check(per, 256, check=[0, 9, 15], seed=33)


def test_decoder_like_distribution_vs_oracle():
    """SURVEY §8(d) second distribution at config-2 shape: 8 100 grid Gaussians @256x256, scale U(.13,.16), random
    rotations: mean radius ~33 px, ~570 pairs per pixel, 3.7x config 2's pair count.  B = 4, two images checked."""
    per = [synth_decoder_like(8192, 4000 + i) for i in range(4)]
    assert per[0][0].shape[0] == 8100
    _run_batch_and_check(per, 256, check=[0, 3], bg=(0.1, 0.2, 0.3), seed=34, min_segments=4)


def test_decoder_like_distribution_config3_shape_vs_oracle():
    """The same distribution at config 3's shape: 32 761 Gaussians @512x512, ~15 000 of them at the 64-px radius cap
    (DR:485), ~1 800 pairs per pixel (P = 4.7e8 per image).  B = 8 (the bench's --distribution decoder_like launch),
    image 5 vs the oracle."""
    per = [synth_decoder_like(32768, 5000 + i) for i in range(8)]
    assert per[0][0].shape[0] == 32761
    worst, st = _run_batch_and_check(per, 512, check=[5], seed=35, expect_seg_len=128, min_segments=8)
    print("decoder-like config3 worst rel-to-max errors:", worst)


@pytest.mark.parametrize("shape", ["small_4waves", "mid_2waves"])
def test_saturation_skip_vs_oracle(shape):
    """FgsDims.saturation_skip (off by default): 8x8 sub-tiles whose accumulated alpha reached 1.0f stop being
    composited at the next 128-entry boundary, forward and backward (dead segments write zero gradient rows).
    Compared with the ORACLE (which composites every entry, DR:582-667) on scenes that saturate most pixels with
    several segments per tile: what is dropped is < 3e-8 |colour| per pixel, so the usual 1e-4 parity bar holds."""
    from oracle import fgs_oracle as orc
    from fresnel_amd.renderer import Camera, TileBasedRenderer
    dev = torch.device("cuda:0")
    # launches of <= 6144 tiles take four waves per tile, larger ones two (row-split forward, SKIP instantiation)
    N, W, H, Bn = (4000, 64, 48, 1) if shape == "small_4waves" else (3000, 64, 64, 400)
    rs = np.random.RandomState(8)
    pos = (rs.randn(N, 3) * [0.3, 0.25, 0.3] + [0, 0, -2.0]).astype(np.float32)
    scale = (0.2 * rs.uniform(0.5, 1.5, (N, 3))).astype(np.float32)
    quat = rs.randn(N, 4).astype(np.float32)
    col = rs.rand(N, 3).astype(np.float32)
    opa = rs.uniform(0.3, 0.95, N).astype(np.float32)
    arrs = [pos, scale, quat, col, opa]
    bg = (0.3, 0.6, 0.1)
    cam = Camera(0.8 * W, 0.8 * H, W / 2, H / 2, W, H)
    ocam = orc.make_camera(np.eye(4, dtype=np.float32), 0.8 * W, 0.8 * H, W / 2, H / 2, W, H)
    gI = rs.standard_normal((3, H, W)).astype(np.float32)
    gD = (rs.standard_normal((H, W)) * 0.1).astype(np.float32)
    r = orc.render(*arrs, ocam, bg=bg)
    go = orc.render_backward(r, gI, gD)
    # the batch repeats one image: every image of the launch must give the oracle's answer
    ts = [torch.from_numpy(np.broadcast_to(a, (Bn,) + a.shape).copy()).to(dev).requires_grad_(True) for a in arrs]
    ren = TileBasedRenderer(W, H, background=bg, saturation_skip=True)
    img, dep = ren(*ts, cam, return_depth=True)
    ((img * torch.from_numpy(gI).to(dev)).sum() + (dep * torch.from_numpy(gD).to(dev)).sum()).backward()
    st = _hip_stages([a[None] for a in arrs], cam, W, H, bg)
    assert (st["ranges"][0][:, 1] - st["ranges"][0][:, 0]).max() > 3 * 128  # several segments per tile
    assert float((st["pix_state"][0, 3] == 1.0).mean()) > 0.5               # most pixels do saturate
    for b in sorted({0, Bn // 2, Bn - 1}):
        assert rel_to_max(img[b].detach().cpu().numpy(), r.image) <= TOL
        assert rel_to_max(dep[b].detach().cpu().numpy(), r.depth) <= TOL
        for k, t in zip(KEYS, ts):
            assert rel_to_max(t.grad[b].cpu().numpy(), go[k]) <= TOL, (b, k)


def test_large_frame_radix_binning_path_vs_oracle():
    """The emit + stable radix sort list builder (frames of more than 4096 tiles per image, e.g. 2400 x 1100 = 75 x 69
    tiles of 32 x 16, where the direct binning cannot be forced; here selected with bin_mode = 2 on a 1200 x 1100 frame, once
    with 16 x 16 and once with 32 x 16 tiles): image, depth, gradients and integer stages against the oracle."""
    from oracle import fgs_oracle as orc
    from fresnel_amd import _binding as B
    from fresnel_amd.renderer import Camera
    W, H, N = 1200, 1100, 3000
    with pytest.raises(B.FgsError):  # direct binning cannot be forced on a frame of more than 4096 tiles
        B.workspace_bytes(B.make_dims(1, N, 2 * W, H, tuning=dict(bin_mode=1)))
    with pytest.raises(B.FgsError):
        B.workspace_bytes(B.make_dims(1, N, W, H, tuning=dict(bin_mode=1, tile_w=16)))
    rs = np.random.RandomState(3)
    from helpers import synth_aniso
    arrs = list(synth_aniso(N, 5, smax=0.08))
    bg = (0.1, 0.2, 0.3)
    cam = Camera(0.8 * W, 0.8 * W, W / 2, H / 2, W, H)
    ocam = orc.make_camera(np.eye(4, dtype=np.float32), cam.fx, cam.fy, cam.cx, cam.cy, W, H)
    r = orc.render(*arrs, ocam, bg=bg)
    gI = rs.standard_normal((3, H, W)).astype(np.float32)
    gD = (rs.standard_normal((H, W)) * 0.1).astype(np.float32)
    go = orc.render_backward(r, gI, gD)
    for tile_w in (16, 32):
        tuning = dict(bin_mode=2, tile_w=tile_w)
        st = _hip_stages([a[None] for a in arrs], cam, W, H, bg, tuning=tuning)
        assert int(st["layout"].tile_w) == tile_w
        _check_integer_stages(st, 0, r, W, H)
        out = _hip_render(arrs, cam, W, H, bg, grads=(gI, gD), tuning=tuning)
        assert rel_to_max(out["image"], r.image) <= TOL and rel_to_max(out["depth"], r.depth) <= TOL
        for k in KEYS:
            assert rel_to_max(out["grad_" + k], go[k]) <= TOL, k


def test_more_than_65536_gaussians_per_image_vs_oracle():
    """N = 70 000 Gaussians in one image (beyond 16-bit ranks; 274 blocks of depth ranks per image): small opaque-ish
    splats over a 256 x 256 frame, long lists."""
    from helpers import synth_saag
    pos, scale, quat, col, opa = synth_saag(70000, 9)
    scale[:] = 0.02
    opa[:] = 0.05
    worst, st = _run_batch_and_check([(pos, scale, quat, col, opa)], 256, check=[0], bg=(0.2, 0.1, 0.0), seed=36,
                                     min_segments=4)
    assert st["order"].shape[1] == 70000


def test_config4_phase_launch_vs_oracle():
    """BASELINE config 4 as the bench launches it: 16 images x 8 192 Gaussians @256x256, depths snapped to 8 zone
    centres (massive depth ties -> canonical stable order), edge-aware scale factors U(.5,1), scalar phases U(0,1),
    phase blending with amplitude 0.25 -- forward, all gradients incl. dL/dphase of images 0 and 11 vs the oracle.  As the
    bench (and the training harness with --use_fresnel_zones) launches it: FgsDims.sort_mode = 1, the zone-key depth sort."""
    from oracle import fgs_oracle as orc
    from fresnel_amd.renderer import Camera
    from helpers import synth_saag
    S, N, Bn = 256, 8192, 16
    rs = np.random.RandomState(44)
    per = []
    for b in range(Bn):
        pos, scale, quat, col, opa = synth_saag(N, 4000 + b)
        pos[:, 2] = (-2.0 - 2.0 * (rs.randint(0, 8, N) + 0.5) / 8.0).astype(np.float32)
        scale = (scale * rs.uniform(0.5, 1.0, (N, 1))).astype(np.float32)
        per.append((pos, scale, quat, col, opa))
    arrs = [np.stack([p[i] for p in per]) for i in range(5)]
    phases = rs.random_sample((Bn, N)).astype(np.float32)
    cam = Camera(0.8 * S, 0.8 * S, S / 2, S / 2, S, S)
    ocam = orc.make_camera(np.eye(4, dtype=np.float32), 0.8 * S, 0.8 * S, S / 2, S / 2, S, S)
    gI = rs.standard_normal((Bn, 3, S, S)).astype(np.float32)
    gD = (rs.standard_normal((Bn, S, S)) * 0.1).astype(np.float32)
    out = _hip_render(arrs, cam, S, S, (0.0, 0.0, 0.0), phases=phases, use_phase=True, amp=0.25, grads=(gI, gD),
                      tuning=dict(sort_mode=1))
    for b in (0, 11):
        r = orc.render(*[a[b] for a in arrs], ocam, phases=phases[b], phase_amp=0.25)
        assert len(np.unique(r.proj["depth"][r.proj["visible"].astype(bool)])) <= 8
        go = orc.render_backward(r, gI[b], gD[b])
        assert rel_to_max(out["image"][b], r.image) <= TOL and rel_to_max(out["depth"][b], r.depth) <= TOL
        for k in KEYS:
            assert rel_to_max(out["grad_" + k][b], go[k]) <= TOL, (b, k)
        assert rel_to_max(out["grad_phases"][b], go["phases"]) <= TOL, b
