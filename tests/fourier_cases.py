"""Scenes shared by the Fourier renderer's tests (tests/test_fourier_checker.py on the CPU, tests/test_hip_fourier.py on the
GPU): the fixture list, the 24 seeded random scenes and their checker runs, computed once per process."""
import functools

import numpy as np
import torch

import fourier_checker as fc
from helpers import load_golden, synth_aniso, upstream_grads

FIXTURES = ["F1_fourier_saag256_128", "F2_fourier_aniso300_96", "F3_fourier_fib377_64", "F4_fourier_n64_56x40",
            "F5_fourier_behind64_64", "F6_fourier_dim128_64"]
GAPPED = FIXTURES[:4]      # generated under the arg-max gap condition (>= MIN_GAP)
GRADS = ["positions", "scales", "rotations", "colors", "opacities"]
MIN_GAP = 1e-3
RANDOM_SEEDS = list(range(24))
MAX_SKIPPED = 2
_FRAMES = [(64, 64), (48, 40), (33, 17), (56, 64), (64, 37), (40, 56)]  # (W, H)


def orbit_view(el_deg, az_deg, distance=2.0):
    """World -> camera matrix of an orbit camera looking at the origin (the formula of TGD:706-744), in numpy."""
    el, az = np.deg2rad(el_deg), np.deg2rad(az_deg)
    cam = np.array([distance * np.cos(el) * np.sin(az), distance * np.sin(el), distance * np.cos(el) * np.cos(az)])
    fwd = -cam / np.linalg.norm(cam)
    right = np.cross(fwd, np.array([0.0, 1.0, 0.0]))
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    Rm = np.array([right, up, -fwd])
    V = np.eye(4, dtype=np.float32)
    V[:3, :3] = Rm.astype(np.float32)
    V[:3, 3] = (-Rm @ cam).astype(np.float32)
    return V


def intrinsics(W, H):
    return (0.8 * W, 0.8 * W, W / 2, H / 2, 0.01, 100.0)


def fixture_scene(name):
    g = load_golden(name)
    W, H = [int(v) for v in g["size"]]
    return dict(arrs=[g[k] for k in GRADS], view=g["view"], intr=[float(v) for v in g["intr"]], W=W, H=H,
                bg=[float(v) for v in g["background"]], gI=g["gI"], g=g)


def random_scene(seed):
    """Anisotropic scene around the origin, N <= 128, frame <= 64 x 64, random orbit view, random background."""
    rs = np.random.RandomState(9000 + seed)
    W, H = _FRAMES[seed % len(_FRAMES)]
    N = int(rs.randint(1, 129))
    arrs = list(synth_aniso(N, 9100 + seed, opacity_max=1.2, spread=0.4, zmean=0.0, smin=0.01, smax=0.12))
    view = orbit_view(rs.uniform(-40, 40), rs.uniform(0, 360), distance=rs.uniform(1.6, 2.4))
    bg = [0.0, 0.0, 0.0] if seed % 3 == 0 else [float(v) for v in rs.uniform(0, 0.5, 3)]
    return dict(arrs=arrs, view=view, intr=intrinsics(W, H), W=W, H=H, bg=bg, gI=upstream_grads(9200 + seed, H, W)[0])


@functools.lru_cache(maxsize=None)
def checker_run(kind, key, f64):
    """(image, raw, [five gradients]) of the checker, in fp32 or fp64, on the CPU; computed once and shared (read-only)."""
    s = fixture_scene(key) if kind == "fixture" else random_scene(key) if kind == "random" else small_scene(*key)
    return fc.render_with_grads(s["arrs"], s["view"], s["intr"], s["W"], s["H"], s["bg"], s["gI"],
                                dtype=torch.float64 if f64 else torch.float32)


def small_scene(N, W, H):
    """N around a K-chunk boundary, frames that are no multiple of a tile; frontal camera."""
    seed = 9500 + 7 * N + W
    while True:
        arrs = list(synth_aniso(N, seed, opacity_max=1.0, spread=0.35, zmean=-2.0, smin=0.02, smax=0.12))
        s = dict(arrs=arrs, view=np.eye(4, dtype=np.float32), intr=intrinsics(W, H), W=W, H=H, bg=[0.1, 0.2, 0.3],
                 gI=upstream_grads(9600 + N, H, W)[0])
        with torch.no_grad():
            raw = fc.render(*[torch.from_numpy(a) for a in arrs], s["view"], s["intr"], W, H)[1]
        if fc.argmax_gap(raw) >= MIN_GAP:
            return s
        seed += 1000


SMALL_CASES = [(n, w, h) for n in (1, 31, 65) for (w, h) in ((40, 56), (33, 17))]


@functools.lru_cache(maxsize=None)
def random_gap(seed):
    return fc.argmax_gap(torch.from_numpy(checker_run("random", seed, False)[1]))
