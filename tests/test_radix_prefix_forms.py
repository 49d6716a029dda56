"""The single-segment tile sort with a device-side length (bin_mode = 2; fgs_sort.hip, the two-launch passes) at the four forms in
which k_radix_downsweep makes its block prefix.  Which form runs depends on the blocks per segment alone, ceil(dup_capacity / 1024)
for the one segment of the tile sort:
    5  blocks: no multiple of 4                  -> the scalar batches of eight
    16 blocks: a multiple of 4, at most 16       -> four uint4 loads
    64 blocks: a multiple of 4, at most 64       -> sixteen uint4 loads
    65 blocks: above 64                          -> k_radix_scan plus the digit totals
The other tests reach this sort at whatever capacity their scene happens to have.  Here ONE scene is rendered at the four capacities
and once with the direct binning (bin_mode = 1), and everything must agree bit for bit: the scene has a few thousand duplicates, far
below every capacity, so the last block that holds keys is ragged and all blocks behind it are empty.

The scene: a 96 x 80 frame, 600 Gaussians of a few tiles each on screen, and 1800 more far off screen.  The culled ones add no
duplicate; they are there because a capacity hint only counts below the worst case batch x Gaussians x 30 tiles, which 600
Gaussians (18 000) would put under three of the four capacities."""
import numpy as np
import pytest
import torch

from sweep_support import cuda_device

pytestmark = pytest.mark.gpu
W, H, VISIBLE, CULLED = 96, 80, 600, 1800
N = VISIBLE + CULLED
CAPACITIES = [5 * 1024, 16 * 1024, 64 * 1024, 65 * 1024]
GRADS = ["positions", "scales", "rotations", "colors", "opacities"]


def _scene():
    rs = np.random.RandomState(11)
    depth = rs.uniform(1.0, 4.0, N).astype(np.float32)
    xy = np.stack([rs.uniform(-0.55, 0.55, N), rs.uniform(-0.45, 0.45, N)], 1)
    pos = np.concatenate([xy * depth[:, None], -depth[:, None]], 1).astype(np.float32)
    pos[VISIBLE:, 0] = 50.0 * depth[VISIBLE:]  # far off screen
    scale = (rs.uniform(0.02, 0.04, (N, 3)) * depth[:, None]).astype(np.float32)  # 1.5 ... 3 pixels of sigma
    quat = rs.standard_normal((N, 4)).astype(np.float32)
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    arrs = [pos, scale, quat, rs.random_sample((N, 3)).astype(np.float32), rs.uniform(0.2, 0.7, N).astype(np.float32)]
    gI = rs.standard_normal((1, 3, H, W)).astype(np.float32)
    gD = (0.1 * rs.standard_normal((1, H, W))).astype(np.float32)
    return [a[None] for a in arrs], gI, gD


def _run(arrs, gI, gD, bin_mode, dup_capacity):
    """One forward through the raw entry (integer stages) and one forward + backward through autograd, same configuration."""
    from fresnel_amd import renderer as R
    from fresnel_amd.renderer import Camera
    dev = cuda_device()
    cam = Camera(0.8 * W, 0.8 * W, W / 2, H / 2, W, H)
    tuning = dict(bin_mode=bin_mode)
    ts = [torch.from_numpy(a).to(dev) for a in arrs]
    cfg = R._Cfg(W, H, (0.1, 0.2, 0.3), 64, False, 0.25, tuning=tuning, dup_capacity=dup_capacity)
    _, _, saved, dims, _ = R.forward_raw(*ts, None, R.pack_cameras(cam, dev), cfg)
    torch.cuda.synchronize()
    st = R.inspect_saved(saved, dims)
    D = int(st["counters"][0].item())
    out = dict(capacity=int(st["layout"].dup_capacity), D=D, ranges=st["ranges"].cpu().numpy(), dup_ids=st["dup_ids"][:D].cpu().numpy())
    ts = [t.clone().requires_grad_(True) for t in ts]
    img, dep = R.render_batch(*ts, cam, W, H, background=(0.1, 0.2, 0.3), tuning=tuning, dup_capacity=dup_capacity)
    ((img * torch.from_numpy(gI).to(dev)).sum() + (dep * torch.from_numpy(gD).to(dev)).sum()).backward()
    out.update(image=img.detach().cpu().numpy(), depth=dep.detach().cpu().numpy())
    for k, t in zip(GRADS, ts):
        out[k] = t.grad.cpu().numpy()
    return out


def test_tile_sort_is_bit_equal_at_every_block_prefix_form_and_to_the_direct_binning():
    arrs, gI, gD = _scene()
    direct = _run(arrs, gI, gD, 1, 0)
    D = direct["D"]
    print(f"duplicates {D}")
    assert D > 1024 and D % 256 != 0 and D < CAPACITIES[0], D  # several blocks with keys, the last of them ragged, empty ones behind
    assert np.abs(direct["image"]).max() > 0 and all(np.abs(direct[k]).max() > 0 for k in GRADS)
    for cap in CAPACITIES:
        got = _run(arrs, gI, gD, 2, cap)
        assert got["capacity"] == cap, f"the hint {cap} did not become the capacity: {got['capacity']}"
        assert got["D"] == D, (cap, got["D"])
        for k in ["ranges", "dup_ids", "image", "depth"] + GRADS:
            a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(direct[k])
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"dup_capacity {cap}: {k} differs"
