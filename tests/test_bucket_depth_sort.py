"""Depth sort of images of more than 8192 Gaussians (fgs_sort.hip, "bucket sort"): one stable pass over memory on an 8-bit digit
that spreads the image's visible keys between their minimum and maximum over <= 255 buckets (culled keys: bucket 255), then every
bucket sorted in LDS by the low bytes the digit did not consume -- <= 2048 pairs by a 256-thread block, <= 8192 by a 1024-thread
block, above that by the block's own radix passes through global memory.  Whatever the depths look like, `order` must be the stable
argsort of the full keys, which is what every sort of this project produces: nothing downstream may change by a bit.

The scenes are 64 x 64 frames of tiny Gaussians (about one tile each), placed so that the DEPTHS are what each case needs."""
import numpy as np
import pytest
import torch

from sweep_support import cuda_device, hip_stages

pytestmark = pytest.mark.gpu
S = 64
SMALL_CAP, LARGE_CAP = 2048, 8192  # pairs a bucket may have in the 256-thread / the 1024-thread LDS sort


def _camera():
    from fresnel_amd.renderer import Camera
    return Camera(0.8 * S, 0.8 * S, S / 2, S / 2, S, S)


def _image(depth, seed, culled=None):
    """One image's five arrays with Gaussian i at depth[i] in front of the identity camera, inside the frame unless culled[i]."""
    depth = np.asarray(depth, np.float32)
    N = depth.shape[0]
    rs = np.random.RandomState(seed)
    pos = np.concatenate([rs.uniform(-0.3, 0.3, (N, 2)) * depth[:, None], -depth[:, None]], 1).astype(np.float32)
    if culled is not None:
        pos[culled, 0] = 50.0 * depth[culled]  # far off-screen
    scale = np.repeat(0.01 * depth[:, None], 3, 1).astype(np.float32)
    quat = np.zeros((N, 4), np.float32)
    quat[:, 0] = 1
    return pos, scale, quat, rs.random_sample((N, 3)).astype(np.float32), np.full(N, 0.5, np.float32)


def _stack(images):
    return [np.stack([im[i] for im in images]) for i in range(5)]


def _stages(images, sort_mode=0):
    return hip_stages(_stack(images), _camera(), S, S, tuning=dict(sort_mode=sort_mode))


def _check_order(st):
    keys = st["depth_key"].view(np.uint32)
    for b in range(keys.shape[0]):
        want = np.argsort(keys[b], kind="stable").astype(np.int32)
        assert np.array_equal(st["order"][b], want), f"image {b}: order is not the stable argsort of the keys"
    return keys


def _buckets(keys):
    """Bucket populations of one image's visible keys under the sort's digit (key - kmin) >> shift, shift the smallest that maps
    kmax - kmin to <= 254 -- a description of the SCENE, used to assert that a case reaches the path it is there for."""
    vis = keys[keys != 0xFFFFFFFF].astype(np.uint64)
    rng = int(vis.max() - vis.min())
    shift = 0
    while (rng >> shift) > 254:
        shift += 1
    return np.bincount(((vis - vis.min()) >> np.uint64(shift)).astype(np.int64), minlength=255), shift


def _band(rs, n, lo=0.04, width=1e-4):
    """n DISTINCT fp32 depths inside [lo, lo + width), in random order (fp32 has ~26 000 values there at lo = 0.04)."""
    first = np.float32(lo).view(np.uint32)
    span = int(np.float32(lo + width).view(np.uint32)) - int(first)
    assert span >= n
    return (first + rs.permutation(span)[:n].astype(np.uint32)).view(np.float32)


@pytest.mark.parametrize("N", [8193, 9001])
def test_first_sizes_above_the_single_block_sort(N):
    """The first sizes on the bucket path; 9001 is no multiple of 64 or 256.  Image 0 ordinary depths, image 1 with culled ones."""
    rs = np.random.RandomState(N)
    images = [_image(rs.uniform(0.5, 4.0, N), 1), _image(rs.uniform(1.0, 3.0, N), 2, culled=rs.rand(N) < 0.07)]
    keys = _check_order(_stages(images))
    assert (keys[0] != 0xFFFFFFFF).all() and 0 < (keys[1] == 0xFFFFFFFF).sum() < N


def _three_ranges(N=20000):
    rs = np.random.RandomState(5)
    nb = N * 9 // 10
    d1 = np.concatenate([_band(rs, nb), rs.uniform(0.5, 4.0, N - nb).astype(np.float32)])[rs.permutation(N)]
    d2 = rs.uniform(2.0, 2.001, N).astype(np.float32)
    d2[rs.permutation(N)[:6]] = [0.15, 0.15, 0.15, 40.0, 40.0, 40.0]
    return [_image(rs.uniform(0.5, 4.0, N), 11), _image(d1, 12), _image(d2, 13)]


def test_every_image_has_its_own_digit():
    """Three images of different depth ranges in one call: ordinary depths (many small buckets); 90 % of the depths distinct values in
    a band 1e-4 wide and the rest spread (one bucket of 18 000 pairs: the global passes, on bytes that really vary); a tight cluster
    with outliers at 0.15 and 40 (kmin and kmax far from nearly all keys).  A second run gives the same `order` bit for bit."""
    images = _three_ranges()
    st = _stages(images)
    keys = _check_order(st)
    pops = [_buckets(keys[b]) for b in range(3)]
    assert pops[0][0].max() <= SMALL_CAP and (pops[0][0] > 0).sum() > 64 and pops[0][1] > 8
    assert pops[1][0].max() == 18000 and pops[1][1] > 8 and np.unique(keys[1]).size > 19000
    assert pops[2][0].max() > LARGE_CAP and (pops[2][0] > 0).sum() == 3
    again = _stages(images)
    assert np.array_equal(again["order"], st["order"])


POPULATIONS = [1000, 2048, 2049, 4096, 4097, 8192, 8193]


def test_bucket_populations_at_both_edges_of_every_class():
    """One image per population P of a narrow band of distinct depths that falls into ONE bucket (the rest spread far behind it, a
    few culled): P = 2048 | 2049 is the edge between the 256-thread and the 1024-thread LDS sort, 8192 | 8193 the edge to the
    global passes; the band's low two bytes vary, so the in-bucket passes really permute."""
    N = 12000
    rs = np.random.RandomState(9)
    images = []
    for P in POPULATIONS:
        rest = rs.uniform(0.5, 4.0, N - P).astype(np.float32)
        depth = np.concatenate([_band(rs, P), rest])[rs.permutation(N)]
        images.append(_image(depth, 20 + len(images), culled=(depth > 3.9)))
    keys = _check_order(_stages(images))
    for b, P in enumerate(POPULATIONS):
        pop, shift = _buckets(keys[b])
        assert pop[0] == P and pop[1:].max() <= SMALL_CAP and shift > 16, (P, pop[0], shift)
        assert (keys[b] == 0xFFFFFFFF).any()


def test_keys_at_the_maximum_and_culled_keys():
    """Visible keys EQUAL to the image's maximum share the last visible bucket; culled ones (0xFFFFFFFF) must end behind them,
    among themselves in index order."""
    N = 10000
    rs = np.random.RandomState(3)
    depth = rs.uniform(1.0, 3.5, N).astype(np.float32)
    depth[rs.rand(N) < 0.05] = 3.5
    culled = rs.rand(N) < 0.1
    st = _stages([_image(depth, 31, culled=culled)])
    keys = _check_order(st)[0]
    vis = keys != 0xFFFFFFFF
    nv, top = int(vis.sum()), keys[vis].max()
    assert 0 < nv < N and (keys[vis] == top).sum() > 100
    order = st["order"][0]
    assert np.array_equal(order[nv:], np.nonzero(~vis)[0]) and (keys[order[nv - 100:nv]] == top).all()


def test_render_is_bit_equal_to_the_two_launch_passes():
    """N = 9000 rendered forward + backward with the automatic sort and with sort_mode = 8 (the two-launch 8-bit passes at any size):
    image, depth and all five gradients bit for bit."""
    from fresnel_amd.renderer import TileBasedRenderer
    from helpers import synth_aniso
    dev = cuda_device()
    arrs = synth_aniso(9000, 77, opacity_max=0.6, smax=0.05)
    rs = np.random.RandomState(78)
    gI = torch.from_numpy(rs.standard_normal((3, S, S)).astype(np.float32)).to(dev)
    gD = torch.from_numpy((rs.standard_normal((S, S)) * 0.1).astype(np.float32)).to(dev)
    outs = []
    for sort_mode in (0, 8):
        ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True) for a in arrs]
        ren = TileBasedRenderer(S, S, background=(0.1, 0.2, 0.3))
        ren.tuning = dict(sort_mode=sort_mode)
        img, dep = ren(*ts, _camera(), return_depth=True)
        ((img * gI).sum() + (dep * gD).sum()).backward()
        outs.append([img.detach().cpu().numpy(), dep.detach().cpu().numpy()] + [t.grad.cpu().numpy() for t in ts])
    assert np.abs(outs[0][0]).max() > 0 and all(np.abs(g).max() > 0 for g in outs[0][2:])
    for name, a, b in zip(["image", "depth", "positions", "scales", "rotations", "colors", "opacities"], *outs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
