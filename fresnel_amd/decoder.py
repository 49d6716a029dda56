"""Patch decoders that PRODUCE renderer inputs.

`DirectPatchDecoder` and `FibonacciPatchDecoder` mirror the reference's classes of the same names
(scripts/models/gaussian_decoder_models.py, "GDM": 622-948 and 1493-1747): constructor arguments, forward signature, returned dict
and state_dict keys are the reference's, so its checkpoints load with strict=True.  Their MLP, convolutions and grid sampling
are torch modules; the Gaussian-parameter head behind the MLP is `gaussian_head`: torch expressions (head_backend "torch", runs
anywhere) or the fused HIP kernel pair of csrc/fgs_head.hip (head_backend "hip", CUDA/ROCm tensors only, no fallback).

`NCAGaussianDecoder` mirrors the reference's class of that name (scripts/models/nca_gaussian_decoder.py, "NCA"; --experiment 5) the
same way; the two parts of its step that are not GEMMs are `nca_perceive` and `nca_update`: the reference's torch expressions
(nca_backend "torch") or the HIP kernels of csrc/fgs_nca.hip (nca_backend "hip", CUDA/ROCm tensors only, no fallback).

`SAAGRefinementNet` mirrors the reference's class of that name (GDM:424-570; --experiment 1) the same way; the two stages around
its MLP are `saag_mlp_inputs` and `saag_refine_head`: the reference's torch expressions (backend "torch") or the HIP kernels of
csrc/fgs_saag.hip (backend "hip", CUDA/ROCm tensors only, no fallback).

`PhysicsDirectPatchDecoder` mirrors the reference's class of that name (GDM:955-1147; --use_wave_rendering without --use_qsr) the
same way, with `PhysicsFresnelZones` (scripts/utils/fresnel_zones.py:400-614) beside it; its head is `physics_head`: the reference's
torch expressions (backend "torch") or the HIP kernels of csrc/fgs_physics.hip (backend "hip", CUDA/ROCm tensors only, no fallback).

`PatchGaussianDecoder` is the older stand-in: own definition with the interface, shapes and ranges of the reference's DirectPatchDecoder
(scripts/models/gaussian_decoder_models.py:622-948): a 37x37 DINOv2 patch grid, K Gaussians per
patch -> dict{positions (B,N,3), scales (B,N,3) in [1e-6,2], rotations (B,N,4) unit wxyz,
colors/opacities in [0,1] [, phases (B,N) in [0,1]]}, N = 37*37*K (K=4 -> 5476).  It is the
module whose gradients the data-parallel step all-reduces (~0.63 M parameters at K=4).
"""
import math
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _binding as B
from . import _hip as hip


def rotate_positions_for_pose(positions: torch.Tensor, elevation: torch.Tensor, azimuth: torch.Tensor) -> torch.Tensor:
    """View-aware rotation of the Gaussian grid (same maths as the reference's rotate_positions_for_pose,
    scripts/models/gaussian_decoder_models.py:51-104): azimuth about Y, then elevation about X, per image.
    positions (B, ..., 3); elevation / azimuth (B,) radians."""
    shape = (positions.shape[0],) + (1,) * (positions.dim() - 2)
    ca, sa = torch.cos(azimuth).view(shape), torch.sin(azimuth).view(shape)
    ce, se = torch.cos(elevation).view(shape), torch.sin(elevation).view(shape)
    x, y, z = positions[..., 0], positions[..., 1], positions[..., 2]
    xr = x * ca + z * sa
    zr = -x * sa + z * ca
    return torch.stack([xr, y * ce - zr * se, y * se + zr * ce], dim=-1)


class DepthEdgeDetector(nn.Module):
    """Edge strength in [0,1] of a (B,1,H,W) depth grid: Sobel gradients concatenated to the depth, three 3x3
    convolutions, sigmoid -- the layout of the reference's FresnelEdgeDetector (scripts/utils/fresnel_zones.py:
    1084-1160; its weights are learned, so only the structure is mirrored)."""

    def __init__(self, hidden_channels: int = 16):
        super().__init__()
        self.conv1 = nn.Conv2d(3, hidden_channels, 3, padding=1)
        self.conv2 = nn.Conv2d(hidden_channels, hidden_channels, 3, padding=1)
        self.conv3 = nn.Conv2d(hidden_channels, 1, 3, padding=1)
        self.register_buffer("sobel_x", torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]]).view(1, 1, 3, 3))
        self.register_buffer("sobel_y", torch.tensor([[-1., -2., -1.], [0., 0., 0.], [1., 2., 1.]]).view(1, 1, 3, 3))

    def forward(self, depth: torch.Tensor) -> torch.Tensor:
        gx, gy = F.conv2d(depth, self.sobel_x, padding=1), F.conv2d(depth, self.sobel_y, padding=1)
        x = F.relu(self.conv1(torch.cat([depth, gx, gy], 1)))
        return torch.sigmoid(self.conv3(F.relu(self.conv2(x))))


class PatchGaussianDecoder(nn.Module):
    def __init__(self, feature_dim: int = 384, gaussians_per_patch: int = 4,
                 hidden_dims=(512, 512, 256, 128), grid: int = 37, use_fresnel_zones: bool = False,
                 num_fresnel_zones: int = 8, use_phase_output: bool = False, use_edge_aware: bool = False,
                 edge_scale_factor: float = 0.5, edge_opacity_boost: float = 0.2):
        super().__init__()
        # --use_edge_aware (TGD:1455-1461; decoder side gaussian_decoder_models.py:882-894): smaller, more opaque
        # Gaussians where the depth grid has edges
        self.use_edge_aware = use_edge_aware
        self.edge_scale_factor, self.edge_opacity_boost = edge_scale_factor, edge_opacity_boost
        self.edge_detector = DepthEdgeDetector() if use_edge_aware else None
        self.grid = grid
        self.gaussians_per_patch = gaussians_per_patch
        self.use_fresnel_zones = use_fresnel_zones
        self.num_fresnel_zones = num_fresnel_zones
        self.use_phase_output = use_phase_output
        self.per_gaussian = 15 + (1 if use_phase_output else 0)  # pos3 scale3 quat4 color3 opa1 (+phase)
        dims = [feature_dim + 1] + list(hidden_dims)
        layers = []
        for a, b in zip(dims[:-1], dims[1:]):
            layers += [nn.Linear(a, b), nn.GELU()]
        layers.append(nn.Linear(dims[-1], gaussians_per_patch * self.per_gaussian))
        self.mlp = nn.Sequential(*layers)
        ys, xs = torch.meshgrid(torch.linspace(-1, 1, grid), torch.linspace(-1, 1, grid), indexing="ij")
        self.register_buffer("grid_xy", torch.stack([xs, -ys], -1).reshape(grid * grid, 2))
        # identity-quaternion bias; a buffer so that the forward makes no host-to-device copy (not part of checkpoints)
        self.register_buffer("quat_bias", torch.tensor([1.0, 0.0, 0.0, 0.0]), persistent=False)

    def forward(self, features: torch.Tensor, depth: torch.Tensor, num_gaussians=None, elevation=None, azimuth=None, **_):
        """features (B,grid,grid,C) ; depth (B,1,h,w) in [0,1].
        num_gaussians: progressive growing (TGD:271-293, gaussian_decoder_models.py:770-790) -- the full capacity is
        predicted and only the first min(num_gaussians, K) Gaussians of every patch are used.
        elevation / azimuth (B,) radians: the grid is rotated to face the camera (rotate_positions_for_pose)."""
        Bn = features.shape[0]
        G, K = self.grid, self.gaussians_per_patch
        d = F.adaptive_avg_pool2d(depth, (G, G)).reshape(Bn, G * G, 1)
        x = torch.cat([features.reshape(Bn, G * G, -1), d], -1)
        o = self.mlp(x).reshape(Bn, G * G, K, self.per_gaussian)
        if num_gaussians is not None and num_gaussians < K:
            K = max(int(num_gaussians), 1)
            o = o[:, :, :K, :]
        cell = 2.0 / (G - 1)
        xy = self.grid_xy.view(1, G * G, 1, 2) + torch.tanh(o[..., 0:2]) * cell
        z = -2.0 - 2.0 * (d.unsqueeze(2) + 0.25 * torch.tanh(o[..., 2:3])).clamp(0, 1)
        if self.use_fresnel_zones:  # snap depth to zone centres (fresnel_zones.py:118-139), straight-through
            zq = -2.0 - 2.0 * ((torch.floor((-(z + 2.0) / 2.0).clamp(0, 0.999999) * self.num_fresnel_zones) + 0.5)
                               / self.num_fresnel_zones)
            z = z + (zq - z).detach()
        positions = torch.cat([xy, z.expand(-1, -1, K, -1)], -1)
        if elevation is not None and azimuth is not None:
            positions = rotate_positions_for_pose(positions, elevation, azimuth)
        scales = (0.13 + 0.03 * torch.sigmoid(o[..., 3:6])).clamp(1e-6, 2.0)
        opacities = torch.sigmoid(o[..., 13])
        if self.use_edge_aware:
            edge = self.edge_detector(d.reshape(Bn, 1, G, G)).reshape(Bn, G * G, 1)          # (B, G*G, 1) in [0,1]
            scales = scales * (1.0 - self.edge_scale_factor * edge.unsqueeze(-1))
            opacities = torch.clamp(opacities + self.edge_opacity_boost * edge, 0, 1)
        out = {
            "positions": positions.reshape(Bn, G * G * K, 3),
            "scales": scales.reshape(Bn, G * G * K, 3),
            "rotations": F.normalize(o[..., 6:10] + self.quat_bias, dim=-1
                                     ).reshape(Bn, G * G * K, 4),
            "colors": torch.sigmoid(o[..., 10:13]).reshape(Bn, G * G * K, 3),
            "opacities": opacities.reshape(Bn, G * G * K),
        }
        if self.use_phase_output:
            out["phases"] = torch.sigmoid(o[..., 15]).reshape(Bn, G * G * K)
        return out


# =================================================================================================================================
# The reference's decoders: DirectPatchDecoder (GDM:622-948), FibonacciPatchDecoder (GDM:1493-1747) and the head they share
# =================================================================================================================================
HEAD_BACKENDS = ("torch", "hip")
HEAD_OUTPUTS = ("positions", "scales", "rotations", "colors", "opacities", "phases")


def rotation_6d_to_quaternion(rot_6d: torch.Tensor) -> torch.Tensor:
    """(..., 6) -> unit quaternion (..., 4) w,x,y,z, the reference's rotation_6d_to_quaternion (GDM:186-276): Gram-Schmidt of the
    two 3-vectors with F.normalize(eps=1e-6), b3 = (0,0,1) where |b1 x b2| < 1e-6, matrix -> quaternion by the branch
    trace > 0 | R00 largest | R11 > R22 | else, normalised.  One defined deviation: where the reference adds 1e-8 times a
    RANDOM sign to b2 before normalising it (GDM:208), this adds +1e-8 -- one of the reference's own draws."""
    a1, a2 = rot_6d[..., :3], rot_6d[..., 3:6]
    b1 = F.normalize(a1, dim=-1, eps=1e-6)
    b2 = F.normalize(a2 - (b1 * a2).sum(dim=-1, keepdim=True) * b1 + 1e-8, dim=-1, eps=1e-6)
    b3 = torch.cross(b1, b2, dim=-1)
    zero = torch.zeros_like(b3[..., 0])  # (0, 0, 1) formed on the device: no host copy, so the expression can be captured in a graph
    b3 = torch.where(b3.norm(dim=-1, keepdim=True) < 1e-6, torch.stack([zero, zero, zero + 1.0], dim=-1), b3)
    b3 = F.normalize(b3, dim=-1, eps=1e-6)
    R00, R01, R02 = b1[..., 0], b2[..., 0], b3[..., 0]   # R = [b1 b2 b3], columns
    R10, R11, R12 = b1[..., 1], b2[..., 1], b3[..., 1]
    R20, R21, R22 = b1[..., 2], b2[..., 2], b3[..., 2]

    def s_of(t):
        return torch.sqrt(torch.clamp(t, min=1e-10)) * 2

    s1, s2 = s_of(R00 + R11 + R22 + 1.0), s_of(1.0 + R00 - R11 - R22)
    s3, s4 = s_of(1.0 + R11 - R00 - R22), s_of(1.0 + R22 - R00 - R11)
    cases = (
        (0.25 * s1, (R21 - R12) / s1, (R02 - R20) / s1, (R10 - R01) / s1),
        ((R21 - R12) / s2, 0.25 * s2, (R01 + R10) / s2, (R02 + R20) / s2),
        ((R02 - R20) / s3, (R01 + R10) / s3, 0.25 * s3, (R12 + R21) / s3),
        ((R10 - R01) / s4, (R02 + R20) / s4, (R12 + R21) / s4, 0.25 * s4),
    )
    c1, c2, c3 = (R00 + R11 + R22) > 0, (R00 > R11) & (R00 > R22), R11 > R22
    quat = torch.stack([torch.where(c1, cases[0][i], torch.where(c2, cases[1][i], torch.where(c3, cases[2][i], cases[3][i])))
                        for i in range(4)], dim=-1)
    return F.normalize(quat, dim=-1, eps=1e-6)


def _head_torch(raw, base_xy, base_z, pose, opacity_mod, edge, K, xy_gain, edge_scale_factor, edge_opacity_boost):
    """The head in torch ops, expression by expression as GDM:845-922: what head_backend "hip" is A/B'd against."""
    Bn, P, _, C = raw.shape
    o = raw[:, :, :K, :]
    x = base_xy[:, 0].view(1, P, 1) + o[..., 0] * xy_gain
    y = base_xy[:, 1].view(1, P, 1) + o[..., 1] * xy_gain
    z = base_z.view(Bn, P, 1).expand(Bn, P, K)
    if pose is not None:  # rotate_positions_for_pose, GDM:96-104
        ca, sa, ce, se = (pose[:, i].view(Bn, 1, 1) for i in range(4))
        xr, zr = x * ca + z * sa, -x * sa + z * ca
        x, y, z = xr, y * ce - zr * se, y * se + zr * ce
    positions = torch.stack([x, y, z], dim=-1)
    scales = torch.clamp(F.softplus(torch.clamp(o[..., 3:6], min=-10, max=20) + 1.0) * 0.15, min=1e-6, max=2.0)
    rotations = rotation_6d_to_quaternion(o[..., 6:12])
    colors = torch.sigmoid(o[..., 12:15])
    opacities = torch.sigmoid(o[..., 15])
    if edge is not None:  # GDM:882-894
        e = edge.view(Bn, P, 1)
        scales = scales * (1.0 - edge_scale_factor * e.unsqueeze(-1))
        opacities = torch.clamp(opacities + edge_opacity_boost * e, 0, 1)
    if opacity_mod is not None:  # GDM:908-912
        opacities = torch.clamp(opacities * opacity_mod.view(Bn, 1, 1), 0, 1)
    N = P * K
    out = [positions.reshape(Bn, N, 3), scales.reshape(Bn, N, 3), rotations.reshape(Bn, N, 4), colors.reshape(Bn, N, 3),
           opacities.reshape(Bn, N)]
    if C == 19:
        out.append((torch.sigmoid(o[..., 16:19]) * (2 * math.pi)).reshape(Bn, N, 3))
    return tuple(out)


_f32c = hip.f32c


class _HeadHip(torch.autograd.Function):
    """fgs_head_forward / fgs_head_backward.  Nothing but the inputs is saved: the backward recomputes from `raw`."""

    @staticmethod
    def forward(ctx, raw, base_xy, base_z, pose, opacity_mod, edge, K, xy_gain, edge_scale_factor, edge_opacity_boost):
        hip.need_cuda(raw, "gaussian_head (backend 'hip')")
        dev = raw.device
        Bn, P, KF, C = raw.shape
        d = B.FgsHeadDims(Bn, P, KF, int(K), C, float(xy_gain), float(edge_scale_factor), float(edge_opacity_boost))
        raw_, xy_, z_, pose_, mod_, edge_ = (_f32c(t) for t in (raw, base_xy, base_z, pose, opacity_mod, edge))
        N = P * int(K)
        outs = [torch.empty((Bn, N, w) if w else (Bn, N), dtype=torch.float32, device=dev) for w in (3, 3, 4, 3, 0)]
        if C == 19:
            outs.append(torch.empty((Bn, N, 3), dtype=torch.float32, device=dev))
        hip.call(dev, "fgs_head_forward", d, raw_, xy_, z_, pose_, mod_, edge_, *outs, *([None] if C != 19 else []))
        ctx.dims = d
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(raw_, pose_, mod_, edge_)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *g_outs):
        raw_, pose_, mod_, edge_ = ctx.saved_tensors
        d = ctx.dims
        need_z, need_mod, need_edge = ctx.needs_input_grad[2], ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        gs = [_f32c(g) for g in g_outs] + [None] * (6 - len(g_outs))
        dev = raw_.device
        g_raw = torch.empty_like(raw_)
        g_z = torch.empty((d.batch, d.points), dtype=torch.float32, device=dev) if need_z else None
        g_edge = torch.empty((d.batch, d.points), dtype=torch.float32, device=dev) if need_edge and edge_ is not None else None
        g_mod = scratch = None
        if need_mod and mod_ is not None:
            g_mod = torch.empty((d.batch,), dtype=torch.float32, device=dev)
            scratch = torch.empty(B.sizes("fgs_head_workspace_bytes", d), dtype=torch.uint8, device=dev)
        hip.call(dev, "fgs_head_backward", d, raw_, pose_, mod_, edge_, *gs, g_raw, g_z, g_edge, g_mod, scratch)
        return (g_raw, None, g_z, None, g_mod, g_edge, None, None, None, None)


def gaussian_head(raw: torch.Tensor, base_xy: torch.Tensor, base_z: torch.Tensor, pose: Optional[torch.Tensor] = None,
                  opacity_mod: Optional[torch.Tensor] = None, edge: Optional[torch.Tensor] = None, *,
                  num_gaussians: Optional[int] = None, xy_gain: float = 0.25, edge_scale_factor: float = 0.5,
                  edge_opacity_boost: float = 0.2, backend: str = "torch") -> Dict[str, torch.Tensor]:
    """The head shared by the reference's patch decoders (GDM:845-922): the MLP's raw (B, P, K_full, 16 | 19) output -> the
    renderers' inputs, N = P x K with K = min(num_gaussians, K_full): positions (B,N,3), scales (B,N,3), rotations (B,N,4),
    colors (B,N,3), opacities (B,N) and, with 19 channels, phases (B,N,3) in radians.

    base_xy (P,2): grid / spiral coordinates; base_z (B,P): depth_offset - 2 depth; pose (B,4): cos az, sin az, cos el, sin el
    (the positions are turned to face the camera); opacity_mod (B,): view-dependent opacity factor; edge (B,P): edge strength
    (smaller, more opaque Gaussians at depth edges).  Gradients flow to raw, base_z, opacity_mod and edge.
    backend "torch": torch expressions, any device.  backend "hip": csrc/fgs_head.hip, one launch forward and one backward,
    bitwise repeatable; CUDA/ROCm tensors only."""
    if backend not in HEAD_BACKENDS:
        raise ValueError(f"unknown head backend {backend!r}: one of {HEAD_BACKENDS}")
    if raw.dim() != 4 or raw.shape[-1] not in (16, 19):
        raise ValueError(f"raw must be (B, P, K_full, 16 | 19), got {tuple(raw.shape)}")
    Bn, P, KF, _ = raw.shape
    K = KF if num_gaussians is None else max(1, min(int(num_gaussians), KF))
    if tuple(base_xy.shape) != (P, 2) or tuple(base_z.shape) != (Bn, P):
        raise ValueError(f"base_xy must be ({P}, 2) and base_z ({Bn}, {P}), got {tuple(base_xy.shape)} and {tuple(base_z.shape)}")
    for name, t, shape in (("pose", pose, (Bn, 4)), ("opacity_mod", opacity_mod, (Bn,)), ("edge", edge, (Bn, P))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
    args = (raw, base_xy, base_z, pose, opacity_mod, edge, K, xy_gain, edge_scale_factor, edge_opacity_boost)
    outs = _HeadHip.apply(*args) if backend == "hip" else _head_torch(*args)
    return dict(zip(HEAD_OUTPUTS, outs))


class _MLP(nn.Module):
    """Linear / ReLU [/ Dropout] stack under the name `net` (GDM:279-302: the checkpoint keys are mlp.net.{0,3,6,...} with
    dropout > 0, mlp.net.{0,2,4,...} without)."""

    def __init__(self, input_dim: int, hidden_dims, output_dim: int, dropout: float = 0.0):
        super().__init__()
        layers, prev = [], input_dim
        for h in hidden_dims:
            layers += [nn.Linear(prev, h), nn.ReLU(inplace=True)]
            if dropout > 0:
                layers.append(nn.Dropout(dropout))
            prev = h
        layers.append(nn.Linear(prev, output_dim))
        self.net = nn.Sequential(*layers)

    def forward(self, x):
        return self.net(x)


class PoseEncoder(nn.Module):
    """Sinusoidal encoding of (elevation, azimuth) at frequencies 2^0 ... 2^(F-1), then a two-layer MLP (GDM:305-367)."""

    def __init__(self, embed_dim: int = 64, num_frequencies: int = 8):
        super().__init__()
        self.embed_dim, self.num_frequencies = embed_dim, num_frequencies
        self.mlp = nn.Sequential(nn.Linear(num_frequencies * 4, embed_dim), nn.ReLU(inplace=True), nn.Linear(embed_dim, embed_dim))

    def sinusoidal_encode(self, x: torch.Tensor) -> torch.Tensor:
        xf = x.unsqueeze(-1) * (2.0 ** torch.arange(self.num_frequencies, device=x.device, dtype=x.dtype))
        return torch.cat([torch.sin(xf), torch.cos(xf)], dim=-1)

    def forward(self, elevation: torch.Tensor, azimuth: torch.Tensor) -> torch.Tensor:
        return self.mlp(torch.cat([self.sinusoidal_encode(elevation), self.sinusoidal_encode(azimuth)], dim=-1))


class DepthEncoder(nn.Module):
    """Three 3x3 convolutions over the depth map, averaged down to the feature grid (GDM:577-615; the reference pools to its
    fixed 37 x 37 grid, this pools to whatever grid the features have -- the same on the reference's grid)."""

    def __init__(self, out_channels: int = 64):
        super().__init__()
        self.out_channels = out_channels
        self.encoder = nn.Sequential(nn.Conv2d(1, 32, 3, padding=1), nn.ReLU(inplace=True),
                                     nn.Conv2d(32, 64, 3, padding=1), nn.ReLU(inplace=True),
                                     nn.Conv2d(64, out_channels, 3, padding=1), nn.ReLU(inplace=True))

    def forward(self, depth: torch.Tensor, grid: Tuple[int, int] = (37, 37)) -> torch.Tensor:
        return F.adaptive_avg_pool2d(self.encoder(depth), grid)


class FresnelZoneTable(nn.Module):
    """The decoder-side part of the reference's FresnelZones (scripts/utils/fresnel_zones.py:54-139): N equal zones over the depth
    range, depths snapped to their zone's centre.  `boundary_emphasis` is the reference's learnable vector; the decoders never
    read it, it exists so that checkpoints load."""

    def __init__(self, num_zones: int = 8, depth_range: Tuple[float, float] = (0.0, 1.0)):
        super().__init__()
        self.num_zones, self.depth_range = num_zones, depth_range
        bounds = torch.linspace(depth_range[0], depth_range[1], num_zones + 1)
        self.register_buffer("zone_boundaries", bounds)
        self.register_buffer("zone_centers", (bounds[:-1] + bounds[1:]) / 2)
        self.register_buffer("zone_width", torch.tensor((depth_range[1] - depth_range[0]) / num_zones))
        self.boundary_emphasis = nn.Parameter(torch.ones(num_zones + 1))

    def get_zone_centers_for_depth(self, depth: torch.Tensor) -> torch.Tensor:
        idx = torch.bucketize(torch.clamp(depth, self.depth_range[0], self.depth_range[1]), self.zone_boundaries[1:-1])
        return self.zone_centers[idx.flatten()].view(idx.shape)


def fibonacci_spiral_positions(n_points: int, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """n points of Vogel's golden-angle spiral in the unit disc (GDM:107-140): r = sqrt(i / n), theta = i pi (3 - sqrt 5)."""
    i = torch.arange(n_points, device=device, dtype=torch.float32)
    r, theta = torch.sqrt(i / n_points), i * (math.pi * (3 - math.sqrt(5)))
    return r * torch.cos(theta), r * torch.sin(theta)


def _pose_row(elevation, azimuth):
    return torch.stack([torch.cos(azimuth), torch.sin(azimuth), torch.cos(elevation), torch.sin(elevation)], dim=-1).detach()


def _check_backend(head_backend):
    if head_backend not in HEAD_BACKENDS:
        raise ValueError(f"unknown head_backend {head_backend!r}: one of {HEAD_BACKENDS}")
    return head_backend


class DirectPatchDecoder(nn.Module):
    """The reference's DirectPatchDecoder (GDM:622-948): every cell of the (H, W) feature grid predicts `gaussians_per_patch`
    Gaussians through a per-patch MLP.  Same constructor arguments and defaults, forward signature, returned dict and
    state_dict keys.  `head_backend`: "torch" | "hip" (gaussian_head)."""

    def __init__(self, feature_dim: int = 384, gaussians_per_patch: int = 8, hidden_dims=(512, 512, 256, 128),
                 dropout: float = 0.1, use_fresnel_zones: bool = False, num_fresnel_zones: int = 8,
                 use_edge_aware: bool = False, use_phase_output: bool = False, edge_scale_factor: float = 0.5,
                 edge_opacity_boost: float = 0.2, use_pose_encoding: bool = False, pose_embed_dim: int = 64,
                 use_depth_fusion: bool = False, depth_feature_dim: int = 64, head_backend: str = "torch"):
        super().__init__()
        self.feature_dim, self.gaussians_per_patch = feature_dim, gaussians_per_patch
        self.use_fresnel_zones, self.use_edge_aware, self.use_phase_output = use_fresnel_zones, use_edge_aware, use_phase_output
        self.edge_scale_factor, self.edge_opacity_boost = edge_scale_factor, edge_opacity_boost
        self.use_pose_encoding, self.use_depth_fusion = use_pose_encoding, use_depth_fusion
        self.head_backend = _check_backend(head_backend)
        self.output_per_gaussian = 19 if use_phase_output else 16
        self.depth_encoder = DepthEncoder(depth_feature_dim) if use_depth_fusion else None
        self.mlp = _MLP(feature_dim + (depth_feature_dim if use_depth_fusion else 0), list(hidden_dims),
                        gaussians_per_patch * self.output_per_gaussian, dropout)
        self.depth_offset = nn.Parameter(torch.tensor(-2.0))
        self.fresnel_zones = FresnelZoneTable(num_fresnel_zones, (0.0, 1.0)) if use_fresnel_zones else None
        self.edge_detector = DepthEdgeDetector(16) if use_edge_aware else None
        self.pose_encoder = PoseEncoder(pose_embed_dim) if use_pose_encoding else None
        self.opacity_modulator = (nn.Sequential(nn.Linear(pose_embed_dim, 128), nn.ReLU(inplace=True), nn.Linear(128, 1),
                                                nn.Sigmoid()) if use_pose_encoding else None)
        self._grids = {}  # (H, W, device) -> (P, 2) grid coordinates

    def _grid_xy(self, H, W, device):
        key = (H, W, str(device))
        if key not in self._grids:
            ys, xs = torch.meshgrid(torch.linspace(-1, 1, H, device=device), torch.linspace(-1, 1, W, device=device), indexing="ij")
            self._grids[key] = torch.stack([xs, ys], dim=-1).reshape(H * W, 2).contiguous()
        return self._grids[key]

    def forward(self, features: torch.Tensor, depth: Optional[torch.Tensor] = None, image_size: Tuple[int, int] = (518, 518),
                num_gaussians: Optional[int] = None, elevation: Optional[torch.Tensor] = None,
                azimuth: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """features (B, C, H, W) channel-first; depth (B, 1, h, w) in [0, 1] or None; num_gaussians: progressive growing (the
        full capacity is predicted, the first min(num_gaussians, K) Gaussians of every patch are used); elevation / azimuth
        (B,) radians.  -> positions, scales, rotations, colors, opacities [, phases (B,N,3) radians] [, edge_strength (B,1,H,W)]."""
        Bn, _, H, W = features.shape
        if self.depth_encoder is not None and depth is not None:
            features = torch.cat([features, self.depth_encoder(depth, (H, W))], dim=1)
        raw = self.mlp(features.permute(0, 2, 3, 1).reshape(Bn * H * W, features.shape[1]))
        raw = raw.reshape(Bn, H * W, self.gaussians_per_patch, self.output_per_gaussian)
        edge_strength = None
        if depth is not None:
            depth_grid = F.interpolate(depth, (H, W), mode="bilinear", align_corners=False)
            if self.edge_detector is not None:
                edge_strength = self.edge_detector(depth_grid)
            if self.fresnel_zones is not None:
                depth_grid = self.fresnel_zones.get_zone_centers_for_depth(depth_grid)
            base_z = self.depth_offset + depth_grid.reshape(Bn, H * W) * (-2)
        else:  # (the reference reads the offset with .item() here: no gradient to it, and none here)
            base_z = self.depth_offset.detach().reshape(1, 1).expand(Bn, H * W).contiguous()
        posed = elevation is not None and azimuth is not None
        opacity_mod = None
        if self.pose_encoder is not None and posed:
            opacity_mod = (0.5 + self.opacity_modulator(self.pose_encoder(elevation, azimuth))).reshape(Bn)
        out = gaussian_head(raw, self._grid_xy(H, W, features.device), base_z,
                            pose=_pose_row(elevation, azimuth) if posed else None, opacity_mod=opacity_mod,
                            edge=edge_strength.reshape(Bn, H * W) if edge_strength is not None else None,
                            num_gaussians=num_gaussians, xy_gain=0.25, edge_scale_factor=self.edge_scale_factor,
                            edge_opacity_boost=self.edge_opacity_boost, backend=self.head_backend)
        if edge_strength is not None:
            out["edge_strength"] = edge_strength
        return out


class FibonacciPatchDecoder(nn.Module):
    """The reference's FibonacciPatchDecoder (GDM:1493-1747): features and depth are sampled bilinearly at `n_spiral_points`
    points of a golden-angle spiral, and a per-point MLP predicts `gaussians_per_point` Gaussians each.  Same constructor
    arguments and defaults, forward signature (num_gaussians is accepted and ignored, as there), returned dict and state_dict keys."""

    def __init__(self, feature_dim: int = 384, n_spiral_points: int = 377, gaussians_per_point: int = 1,
                 hidden_dims=(512, 256, 128), dropout: float = 0.1, use_fresnel_zones: bool = False, num_fresnel_zones: int = 8,
                 use_phase_output: bool = False, use_pose_encoding: bool = False, pose_embed_dim: int = 64,
                 head_backend: str = "torch"):
        super().__init__()
        self.feature_dim, self.n_spiral_points, self.gaussians_per_point = feature_dim, n_spiral_points, gaussians_per_point
        self.total_gaussians = n_spiral_points * gaussians_per_point
        self.use_fresnel_zones, self.use_phase_output, self.use_pose_encoding = use_fresnel_zones, use_phase_output, use_pose_encoding
        self.head_backend = _check_backend(head_backend)
        self.output_per_gaussian = 19 if use_phase_output else 16
        self.mlp = _MLP(feature_dim, list(hidden_dims), gaussians_per_point * self.output_per_gaussian, dropout)
        self.depth_offset = nn.Parameter(torch.tensor(-2.0))
        sx, sy = fibonacci_spiral_positions(n_spiral_points)
        self.register_buffer("spiral_x", sx)
        self.register_buffer("spiral_y", sy)
        self.fresnel_zones = FresnelZoneTable(num_fresnel_zones, (0.0, 1.0)) if use_fresnel_zones else None
        self.pose_encoder = PoseEncoder(pose_embed_dim) if use_pose_encoding else None
        self.opacity_modulator = (nn.Sequential(nn.Linear(pose_embed_dim, 64), nn.ReLU(inplace=True), nn.Linear(64, 1),
                                                nn.Sigmoid()) if use_pose_encoding else None)

    def forward(self, features: torch.Tensor, depth: Optional[torch.Tensor] = None, image_size: Tuple[int, int] = (518, 518),
                num_gaussians: Optional[int] = None, elevation: Optional[torch.Tensor] = None,
                azimuth: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        Bn, C = features.shape[:2]
        P = self.n_spiral_points
        xy = torch.stack([self.spiral_x, self.spiral_y], dim=-1)                      # (P, 2)
        coords = xy.view(1, 1, P, 2).expand(Bn, -1, -1, -1)
        sampled = F.grid_sample(features, coords, mode="bilinear", padding_mode="border", align_corners=True)  # (B, C, 1, P)
        raw = self.mlp(sampled.squeeze(2).permute(0, 2, 1).reshape(Bn * P, C))
        raw = raw.reshape(Bn, P, self.gaussians_per_point, self.output_per_gaussian)
        if depth is not None:
            d = F.grid_sample(depth, coords, mode="bilinear", padding_mode="border", align_corners=True).reshape(Bn, P)
            if self.fresnel_zones is not None:
                d = self.fresnel_zones.get_zone_centers_for_depth(d)
            base_z = self.depth_offset + d * (-2)
        else:
            base_z = self.depth_offset.detach().reshape(1, 1).expand(Bn, P).contiguous()
        posed = elevation is not None and azimuth is not None
        opacity_mod = None
        if self.pose_encoder is not None and posed:
            opacity_mod = (0.5 + self.opacity_modulator(self.pose_encoder(elevation, azimuth))).reshape(Bn)
        return gaussian_head(raw, xy, base_z, pose=_pose_row(elevation, azimuth) if posed else None, opacity_mod=opacity_mod,
                             xy_gain=0.15, backend=self.head_backend)


# =================================================================================================================================
# The reference's NCAGaussianDecoder (scripts/models/nca_gaussian_decoder.py, "NCA") and the two pieces of its step that are not GEMMs
# =================================================================================================================================
NCA_BACKENDS = ("torch", "hip")


def _check_nca_backend(backend):
    if backend not in NCA_BACKENDS:
        raise ValueError(f"unknown nca_backend {backend!r}: one of {NCA_BACKENDS}")
    return backend


def _nca_dims(state, k):
    Bn, N, D = state.shape
    return B.FgsNcaDims(Bn, N, D, int(k))


class _NcaPerceiveHip(torch.autograd.Function):
    """fgs_nca_perceive_forward / _backward.  Saved: the neighbour table alone."""

    @staticmethod
    def forward(ctx, state, k):
        hip.need_cuda(state, "nca_perceive (backend 'hip')")
        state_ = _f32c(state)
        d = _nca_dims(state_, k)
        dev = state_.device
        perception = torch.empty((d.batch, d.points, (d.k + 1) * d.state_dim), dtype=torch.float32, device=dev)
        neighbors = torch.empty((d.batch, d.points, d.k), dtype=torch.int32, device=dev)
        hip.call(dev, "fgs_nca_perceive_forward", d, state_, perception, neighbors)
        ctx.dims = d
        ctx.save_for_backward(neighbors)
        ctx.mark_non_differentiable(neighbors)
        return perception, neighbors

    @staticmethod
    def backward(ctx, g_perception, _g_neighbors):
        neighbors, = ctx.saved_tensors
        d = ctx.dims
        g_ = _f32c(g_perception)
        g_state = torch.empty((d.batch, d.points, d.state_dim), dtype=torch.float32, device=g_.device)
        hip.call(g_.device, "fgs_nca_perceive_backward", d, neighbors, g_, g_state)
        return g_state, None


def _nca_perceive_torch(state, k):
    """NCA:247-264 as written there: cdist, topk of k + 1 smallest with the first (self, at distance 0) dropped, gather over the
    (B, N, N, D) expanded view, cat."""
    Bn, N, D = state.shape
    positions = state[..., :3]
    dists = torch.cdist(positions, positions)
    _, neighbor_idx = dists.topk(k + 1, dim=-1, largest=False)
    neighbor_idx = neighbor_idx[..., 1:]
    idx_expanded = neighbor_idx.unsqueeze(-1).expand(-1, -1, -1, D)
    neighbors = torch.gather(state.unsqueeze(1).expand(-1, N, -1, -1), dim=2, index=idx_expanded)
    return torch.cat([state, neighbors.reshape(Bn, N, k * D)], dim=-1), neighbor_idx


def nca_perceive(state: torch.Tensor, k: int, backend: str = "torch") -> Tuple[torch.Tensor, torch.Tensor]:
    """The perception input of one NCA step (NCA:247-264): state (B, N, D), channels 0..2 the position -> (perception
    (B, N, (k+1) D): every point's own row followed by the rows of its k nearest neighbours; neighbors (B, N, k), not
    differentiable).  Gradients flow to the gathered rows only, never through the choice of neighbours.
    backend "torch": the reference's cdist + topk + gather, any device; neighbors int64, ties and near-ties in topk's order.
    backend "hip": csrc/fgs_nca.hip, one launch each way, the CANONICAL neighbours of include/fgs.h (k smallest (d2, j), d2 in
    exactly rounded fp32 differences), int32; CUDA/ROCm tensors only; 1 <= k <= 16, k + 1 <= N <= 4096, 3 <= D <= 64."""
    _check_nca_backend(backend)
    if state.dim() != 3 or state.shape[-1] < 3:
        raise ValueError(f"state must be (B, N, D >= 3), got {tuple(state.shape)}")
    if not 1 <= int(k) < state.shape[1]:
        raise ValueError(f"k must be in [1, N - 1] = [1, {state.shape[1] - 1}], got {k}")
    return _NcaPerceiveHip.apply(state, int(k)) if backend == "hip" else _nca_perceive_torch(state, int(k))


class _NcaUpdateHip(torch.autograd.Function):
    """fgs_nca_update_forward / _backward.  dL/dstate is the upstream gradient itself: the same tensor is returned, no copy."""

    @staticmethod
    def forward(ctx, state, delta, step_size, uniform, update_prob):
        hip.need_cuda(state, "nca_update (backend 'hip')")
        state_, delta_, step_, uni_ = _f32c(state), _f32c(delta), _f32c(step_size), _f32c(uniform)
        d = _nca_dims(state_, 1)
        new_state = torch.empty_like(state_)
        hip.call(state_.device, "fgs_nca_update_forward", d, state_, delta_, step_, uni_, float(update_prob), new_state)
        ctx.dims, ctx.update_prob = d, float(update_prob)
        ctx.save_for_backward(delta_, step_, uni_)
        return new_state

    @staticmethod
    def backward(ctx, g_new_state):
        delta_, step_, uni_ = ctx.saved_tensors
        d = ctx.dims
        g_ = _f32c(g_new_state)
        dev = g_.device
        g_delta = torch.empty_like(delta_)
        g_step = torch.empty((), dtype=torch.float32, device=dev)
        scratch = torch.empty(B.sizes("fgs_nca_workspace_bytes", d), dtype=torch.uint8, device=dev)
        hip.call(dev, "fgs_nca_update_backward", d, delta_, step_, uni_, ctx.update_prob, g_, g_delta, g_step, scratch)
        return g_new_state, g_delta, g_step, None, None


def nca_update(state: torch.Tensor, delta: torch.Tensor, step_size: torch.Tensor, uniform: Optional[torch.Tensor] = None,
               update_prob: float = 0.5, backend: str = "torch") -> torch.Tensor:
    """The tail of one NCA step (NCA:276-284): state + step_size x (delta x mask) with mask = (uniform < update_prob) per point.
    state, delta (B, N, D); step_size a 0-dim tensor (the learnable step); uniform (B, N) | (B, N, 1) draws of U[0, 1), or None:
    eval mode, no mask.  Gradients flow to state, delta and step_size.
    backend "torch": the reference's expressions, any device.  backend "hip": csrc/fgs_nca.hip, one launch forward (the same
    roundings: bit-equal), two backward (dL/dstep_size by a fixed-order sum in double: repeats bit for bit); CUDA/ROCm only."""
    _check_nca_backend(backend)
    if state.dim() != 3 or delta.shape != state.shape:
        raise ValueError(f"state and delta must share one (B, N, D) shape, got {tuple(state.shape)} and {tuple(delta.shape)}")
    if uniform is not None:
        if tuple(uniform.shape) not in (tuple(state.shape[:2]), tuple(state.shape[:2]) + (1,)):
            raise ValueError(f"uniform must be (B, N) or (B, N, 1), got {tuple(uniform.shape)}")
        uniform = uniform.reshape(state.shape[0], state.shape[1], 1)
    if backend == "hip":
        return _NcaUpdateHip.apply(state, delta, step_size.reshape(()), uniform, update_prob)
    if uniform is not None:
        delta = delta * (uniform < update_prob).float()
    return state + step_size * delta


def _nca_uniform(batch: int, points: int, device) -> torch.Tensor:
    """The step's draws (NCA:278): one torch.rand(B, N, 1) per step from the global generator, so the stream is the reference's."""
    return torch.rand(batch, points, 1, device=device)


class NCAGaussianDecoder(nn.Module):
    """The reference's NCAGaussianDecoder (NCA:39-365, --experiment 5): Gaussians are cells of a cellular automaton.  Features
    sampled at `n_points` spiral points give an initial (B, N, 16) state [pos 3, scale 3, rot6d 6, colour 3, opacity 1] with x, y on
    the spiral and z locked to the depth; `n_steps` times every point perceives itself and its `k_neighbors` nearest neighbours,
    two small MLPs turn that into a delta, and a random half of the points (training) take a step of the learnable `step_size`.
    Same constructor arguments and defaults, forward signature, returned dict, state_dict keys and registration order.
    `nca_backend`: neighbour perception and update, "torch" (the reference's cdist / topk / gather) | "hip" (nca_perceive,
    nca_update); `head_backend`: the final state -> Gaussian parameters, which is gaussian_head with a zero grid and gain 1."""

    def __init__(self, feature_dim: int = 384, n_points: int = 377, n_steps: int = 16, k_neighbors: int = 6, hidden_dim: int = 128,
                 update_prob: float = 0.5, state_dim: int = 16, *, nca_backend: str = "torch", head_backend: str = "torch"):
        super().__init__()
        self.feature_dim, self.n_points, self.n_steps, self.k_neighbors = feature_dim, n_points, n_steps, k_neighbors
        self.hidden_dim, self.update_prob, self.state_dim = hidden_dim, update_prob, state_dim
        self.nca_backend, self.head_backend = _check_nca_backend(nca_backend), _check_backend(head_backend)
        sx, sy = fibonacci_spiral_positions(n_points)
        self.register_buffer("spiral_x", sx)
        self.register_buffer("spiral_y", sy)
        self.depth_offset = nn.Parameter(torch.tensor(-2.0))
        self.init_state_net = nn.Sequential(nn.Linear(feature_dim, hidden_dim * 2), nn.ReLU(inplace=True),
                                            nn.Linear(hidden_dim * 2, hidden_dim), nn.ReLU(inplace=True),
                                            nn.Linear(hidden_dim, state_dim))
        self.perception = nn.Sequential(nn.Linear(state_dim * (k_neighbors + 1), hidden_dim * 2), nn.ReLU(inplace=True),
                                        nn.Linear(hidden_dim * 2, hidden_dim), nn.ReLU(inplace=True))
        self.update_rule = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.ReLU(inplace=True), nn.Linear(hidden_dim, state_dim))
        nn.init.zeros_(self.update_rule[-1].weight)  # residual learning: the automaton starts as the identity (NCA:131-132)
        nn.init.zeros_(self.update_rule[-1].bias)
        self.step_size = nn.Parameter(torch.tensor(0.1))
        # the head's grid term: the state carries absolute x, y (not part of checkpoints)
        self.register_buffer("zero_xy", torch.zeros(n_points, 2), persistent=False)

    def forward(self, features: torch.Tensor, depth: Optional[torch.Tensor] = None, image_size: Tuple[int, int] = (518, 518),
                num_gaussians: Optional[int] = None, elevation: Optional[torch.Tensor] = None,
                azimuth: Optional[torch.Tensor] = None, n_steps: Optional[int] = None,
                return_trajectory: bool = False) -> Dict[str, torch.Tensor]:
        """features (B, C, H, W); depth (B, 1, h, w) or None; num_gaussians, elevation, azimuth: accepted and ignored, as there.
        -> positions, scales, rotations, colors, opacities [, trajectory: the n_steps + 1 detached states]."""
        n_steps = n_steps if n_steps is not None else self.n_steps
        Bn, C = features.shape[:2]
        N = self.n_points
        coords = torch.stack([self.spiral_x, self.spiral_y], dim=-1).view(1, 1, N, 2).expand(Bn, -1, -1, -1)
        sampled = F.grid_sample(features, coords, mode="bilinear", padding_mode="border", align_corners=True)  # (B, C, 1, N)
        if depth is not None:
            d = F.grid_sample(depth, coords, mode="bilinear", padding_mode="border", align_corners=True).reshape(Bn, N)
        else:
            d = torch.zeros(Bn, N, device=features.device)
        init = self.init_state_net(sampled.squeeze(2).permute(0, 2, 1).reshape(Bn * N, C)).reshape(Bn, N, self.state_dim)
        # x, y: the spiral plus a small detached offset; z locked to the depth (NCA:199-210)
        x = self.spiral_x.view(1, N) + init[..., 0].detach() * 0.15
        y = self.spiral_y.view(1, N) + init[..., 1].detach() * 0.15
        z = self.depth_offset + d * (-2)
        state = torch.cat([torch.stack([x, y, z], dim=-1), init[..., 3:]], dim=-1)
        trajectory = [state.detach().clone()] if return_trajectory else None
        for _ in range(n_steps):
            state = self._nca_step(state)
            if return_trajectory:
                trajectory.append(state.detach().clone())
        result = self._parse_state(state)
        if return_trajectory:
            result["trajectory"] = trajectory
        return result

    def _nca_step(self, state: torch.Tensor) -> torch.Tensor:
        Bn, N, D = state.shape
        perception, _ = nca_perceive(state, self.k_neighbors, backend=self.nca_backend)
        delta = self.update_rule(self.perception(perception.reshape(Bn * N, -1))).reshape(Bn, N, D)
        uniform = _nca_uniform(Bn, N, state.device) if self.training else None
        return nca_update(state, delta, self.step_size, uniform, self.update_prob, backend=self.nca_backend)

    def _parse_state(self, state: torch.Tensor) -> Dict[str, torch.Tensor]:
        """NCA:324-365 through the shared head: base_xy = 0 and xy_gain = 1 leave x, y as they are, z rides as base_z."""
        return gaussian_head(state.unsqueeze(2), self.zero_xy, state[..., 2], xy_gain=1.0, backend=self.head_backend)


# =================================================================================================================================
# The reference's SAAGRefinementNet (GDM:424-570, --experiment 1) and the two stages of it that are not GEMMs
# =================================================================================================================================
SAAG_BACKENDS = ("torch", "hip")
SAAG_OUTPUTS = ("positions", "scales", "rotations", "colors", "opacities", "pos_delta", "scale_delta", "color_delta", "opacity_delta")
_SAAG_NAMES = ("positions", "scales", "rotations", "colors", "opacities")


def _check_saag_backend(backend):
    if backend not in SAAG_BACKENDS:
        raise ValueError(f"unknown saag backend {backend!r}: one of {SAAG_BACKENDS}")
    return backend


def _check_saag_cloud(positions, scales, rotations, colors, opacities):
    if positions.dim() != 3 or positions.shape[-1] != 3:
        raise ValueError(f"positions must be (B, N, 3), got {tuple(positions.shape)}")
    Bn, N = positions.shape[:2]
    for name, t, shape in (("scales", scales, (Bn, N, 3)), ("rotations", rotations, (Bn, N, 4)), ("colors", colors, (Bn, N, 3)),
                           ("opacities", opacities, (Bn, N))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
    return Bn, N


def _refuse_grad(backend_of, tensors):
    for name, t in tensors:
        if t.requires_grad:
            raise ValueError(f"{backend_of} (backend 'hip') produces no gradient for {name} (dataset data in the reference's "
                             "training); use backend 'torch' to differentiate with respect to it")


def _saag_quaternion_multiply(q1, q2):
    """q1 (x) q2, (w, x, y, z) (GDM:555-570)."""
    w1, x1, y1, z1 = q1[..., 0], q1[..., 1], q1[..., 2], q1[..., 3]
    w2, x2, y2, z2 = q2[..., 0], q2[..., 1], q2[..., 2], q2[..., 3]
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], dim=-1)


def _saag_mlp_inputs_torch(features, positions, scales, rotations, colors, opacities):
    """GDM:491-509 with FeatureInterpolator (GDM:396-417) as written there."""
    pos_2d = positions[..., :2] / positions[..., 2:3].clamp(min=0.1)
    pos_2d_norm = ((pos_2d + 2) / 4).clamp(0, 1)
    grid = (pos_2d_norm * 2 - 1).unsqueeze(2)
    sampled = F.grid_sample(features, grid, mode="bilinear", padding_mode="border", align_corners=False)  # (B, C, N, 1)
    sampled = sampled.squeeze(-1).permute(0, 2, 1)
    return torch.cat([sampled, positions, scales, rotations, colors, opacities.unsqueeze(-1)], dim=-1)


def _saag_dims(Bn, N, C=1, H=1, W=1, strides=(1, 1, 1), residual_scale=0.0):
    return B.FgsSaagDims(Bn, N, C, H, W, int(strides[0]), int(strides[1]), int(strides[2]), float(residual_scale))


def _saag_mlp_inputs_hip(features, positions, scales, rotations, colors, opacities):
    for t in (features, positions):
        hip.need_cuda(t, "saag_mlp_inputs (backend 'hip')")
    _refuse_grad("saag_mlp_inputs", (("features", features),) + tuple(zip(_SAAG_NAMES, (positions, scales, rotations, colors, opacities))))
    Bn, C, H, W = features.shape
    N = positions.shape[1]
    feats = features.detach().float()
    # the two layouts the kernel samples in place; strides come from the shape (torch leaves those of size-1 dimensions open)
    if feats.permute(0, 2, 3, 1).is_contiguous():    # the training loop's (B, h, w, C) tensor seen channel-first
        strides = (H * W * C, 1, W * C)
    else:
        feats = feats.contiguous()                   # (a no-op for a contiguous channel-first tensor)
        strides = (C * H * W, H * W, W)
    cloud = [_f32c(t) for t in (positions, scales, rotations, colors, opacities)]
    d = _saag_dims(Bn, N, C, H, W, strides)
    out = torch.empty((Bn, N, C + 14), dtype=torch.float32, device=feats.device)
    hip.call(feats.device, "fgs_saag_inputs_forward", d, feats, *cloud, out)
    return out


def saag_mlp_inputs(features: torch.Tensor, positions: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor,
                    colors: torch.Tensor, opacities: torch.Tensor, backend: str = "torch") -> torch.Tensor:
    """The input of SAAGRefinementNet's MLP (GDM:489-509): features (B, C, H, W) sampled bilinearly at every SAAG Gaussian's
    projected position, concatenated with the Gaussian's 14 parameters -> (B, N, C + 14), row = [C features | position 3 | scale 3 |
    rotation 4 | colour 3 | opacity 1].  positions (B,N,3), scales (B,N,3), rotations (B,N,4), colors (B,N,3), opacities (B,N).
    backend "torch": the reference's projection, grid_sample, permute and cat, any device, differentiable.  backend "hip":
    csrc/fgs_saag.hip, one launch that writes the result once; CUDA/ROCm tensors only; a channel-last `features` view (the
    training loop's (B, h, w, C) tensor permuted) and a contiguous channel-first tensor are sampled in place; forward only -- an
    input that requires grad is refused (every input is dataset data in the reference's training)."""
    _check_saag_backend(backend)
    if features.dim() != 4:
        raise ValueError(f"features must be (B, C, H, W), got {tuple(features.shape)}")
    Bn, _ = _check_saag_cloud(positions, scales, rotations, colors, opacities)
    if features.shape[0] != Bn:
        raise ValueError(f"features hold {features.shape[0]} images, the SAAG cloud {Bn}")
    args = (features, positions, scales, rotations, colors, opacities)
    return _saag_mlp_inputs_hip(*args) if backend == "hip" else _saag_mlp_inputs_torch(*args)


def _saag_refine_torch(raw, positions, scales, rotations, colors, opacities, gains, residual_scale):
    """GDM:515-553 as written there; gains = (pos_scale, scale_scale, color_scale, opacity_scale)."""
    pos_delta = raw[..., 0:3] * gains[0] * residual_scale
    scale_delta = raw[..., 3:6] * gains[1] * residual_scale
    color_delta = raw[..., 12:15] * gains[2] * residual_scale
    opacity_delta = raw[..., 15:16] * gains[3] * residual_scale
    rot = F.normalize(_saag_quaternion_multiply(rotation_6d_to_quaternion(raw[..., 6:12]), rotations), dim=-1)
    return (positions + pos_delta, scales * torch.exp(scale_delta), rot, torch.clamp(colors + color_delta, 0, 1),
            torch.clamp(opacities + opacity_delta.squeeze(-1), 0, 1), pos_delta, scale_delta, color_delta, opacity_delta)


class _SaagRefineHip(torch.autograd.Function):
    """fgs_saag_refine_forward / _backward.  Nothing but the inputs is saved: the backward recomputes from `raw`."""

    @staticmethod
    def forward(ctx, raw, gains, positions, scales, rotations, colors, opacities, residual_scale):
        for t in (raw, gains, positions):
            hip.need_cuda(t, "saag_refine_head (backend 'hip')")
        dev = raw.device
        Bn, N, _ = raw.shape
        raw_, gains_ = _f32c(raw), _f32c(gains)
        cloud = [_f32c(t) for t in (positions, scales, rotations, colors, opacities)]
        d = _saag_dims(Bn, N, residual_scale=residual_scale)
        outs = [torch.empty(s, dtype=torch.float32, device=dev) for s in
                ((Bn, N, 3), (Bn, N, 3), (Bn, N, 4), (Bn, N, 3), (Bn, N), (Bn, N, 3), (Bn, N, 3), (Bn, N, 3), (Bn, N, 1))]
        hip.call(dev, "fgs_saag_refine_forward", d, raw_, *cloud, gains_, *outs)
        ctx.dims = d
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(raw_, gains_, *cloud[1:])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *g_outs):
        raw_, gains_, scales_, rot_, colors_, opa_ = ctx.saved_tensors
        d = ctx.dims
        gs = [_f32c(g) for g in g_outs]
        dev = raw_.device
        g_raw = torch.empty_like(raw_)
        g_gains = torch.empty((4,), dtype=torch.float32, device=dev)
        scratch = torch.empty(B.sizes("fgs_saag_workspace_bytes", d), dtype=torch.uint8, device=dev)
        hip.call(dev, "fgs_saag_refine_backward", d, raw_, scales_, rot_, colors_, opa_, gains_, *gs, g_raw, g_gains, scratch)
        return (g_raw, g_gains, None, None, None, None, None, None)


def saag_refine_head(raw: torch.Tensor, positions: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor,
                     colors: torch.Tensor, opacities: torch.Tensor, gains: torch.Tensor, residual_scale: float = 0.1,
                     backend: str = "torch") -> Dict[str, torch.Tensor]:
    """The residual head of SAAGRefinementNet (GDM:515-553): the MLP's raw (B, N, 16) output [position 3 | scale 3 | rotation-6D 6 |
    colour 3 | opacity 1] and the SAAG cloud -> the reference's nine-entry dict: positions = saag + pos_delta, scales = saag x
    exp(scale_delta), rotations = normalize(q_delta (x) q_saag), colors / opacities = clamp(saag + delta, 0, 1), and the four
    deltas = raw x gain x residual_scale that the loss regularises (opacity_delta is (B, N, 1)).  gains: 4 floats (pos_scale,
    scale_scale, color_scale, opacity_scale) on raw's device.  Gradients flow to raw and gains.
    backend "torch": the reference's expressions, any device (and differentiable in the SAAG tensors).  backend "hip":
    csrc/fgs_saag.hip, one launch forward and two backward, bitwise repeatable, nothing read on the host; CUDA/ROCm tensors
    only; a SAAG tensor that requires grad is refused."""
    _check_saag_backend(backend)
    if raw.dim() != 3 or raw.shape[-1] != 16:
        raise ValueError(f"raw must be (B, N, 16), got {tuple(raw.shape)}")
    if tuple(_check_saag_cloud(positions, scales, rotations, colors, opacities)) != tuple(raw.shape[:2]):
        raise ValueError(f"raw is {tuple(raw.shape)}, the SAAG cloud {tuple(positions.shape[:2])}")
    if tuple(gains.shape) != (4,):
        raise ValueError(f"gains must be (4,): pos, scale, colour, opacity; got {tuple(gains.shape)}")
    cloud = (positions, scales, rotations, colors, opacities)
    if backend == "hip":
        for t in (raw, gains, positions):
            hip.need_cuda(t, "saag_refine_head (backend 'hip')")
        _refuse_grad("saag_refine_head", tuple(zip(_SAAG_NAMES, cloud)))
        outs = _SaagRefineHip.apply(raw, gains, *cloud, float(residual_scale))
    else:
        outs = _saag_refine_torch(raw, *cloud, gains, residual_scale)
    return dict(zip(SAAG_OUTPUTS, outs))


class SAAGRefinementNet(nn.Module):
    """The reference's SAAGRefinementNet (GDM:424-570, --experiment 1): features sampled at every SAAG Gaussian and the Gaussian's
    own parameters go through an MLP that predicts residuals; the output is SAAG plus the residuals, scaled by four learnable
    gains and `residual_scale`.  Same constructor arguments and defaults, forward signature (image_size and intrinsics are
    accepted and unused, as there), returned dict, state_dict keys (mlp.net.{0,3,6}.*, pos_scale, scale_scale, color_scale,
    opacity_scale) and registration order.  `backend`: "torch" | "hip" for saag_mlp_inputs and saag_refine_head."""

    def __init__(self, feature_dim: int = 384, hidden_dims=(256, 128), residual_scale: float = 0.1, dropout: float = 0.1,
                 backend: str = "torch"):
        super().__init__()
        self.feature_dim, self.residual_scale = feature_dim, residual_scale
        self.backend = _check_saag_backend(backend)
        self.mlp = _MLP(feature_dim + 14, list(hidden_dims), 16, dropout)
        self.pos_scale = nn.Parameter(torch.tensor(0.05))
        self.scale_scale = nn.Parameter(torch.tensor(0.1))
        self.color_scale = nn.Parameter(torch.tensor(0.1))
        self.opacity_scale = nn.Parameter(torch.tensor(0.1))

    def forward(self, features: torch.Tensor, saag_positions: torch.Tensor, saag_scales: torch.Tensor,
                saag_rotations: torch.Tensor, saag_colors: torch.Tensor, saag_opacities: torch.Tensor,
                image_size: Tuple[int, int] = (518, 518), intrinsics: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        cloud = (saag_positions, saag_scales, saag_rotations, saag_colors, saag_opacities)
        inputs = saag_mlp_inputs(features, *cloud, backend=self.backend)
        Bn, N, D = inputs.shape
        raw = self.mlp(inputs.reshape(Bn * N, D)).reshape(Bn, N, 16)
        # the four scalars as one device vector: the hip head reads them there, nothing goes through the host
        gains = torch.stack([self.pos_scale, self.scale_scale, self.color_scale, self.opacity_scale])
        return saag_refine_head(raw, *cloud, gains, residual_scale=self.residual_scale, backend=self.backend)


class FeatureGuidedSAAG(nn.Module):
    """The reference's FeatureGuidedSAAG (GDM:1422-1490, --experiment 3): two linear layers predict, per feature patch, six
    modifications of the SAAG generator's parameters.  Same constructor arguments and defaults, forward(features (B,C,H,W)),
    returned dict of six (B,H,W) maps (surface.MOD_KEYS, in that order) and state_dict keys (net.0.*, net.2.*).  The last layer
    starts at zero: an untrained model returns (1, 0, 1, 1, 1, 1) everywhere, the plain SAAG cloud.  The maps go into
    surface.guided_surface_gaussians, whose backward gives every one of them a gradient (the reference has no such path)."""

    def __init__(self, feature_dim: int = 384, num_params: int = 6, hidden_dim: int = 64):
        super().__init__()
        self.feature_dim, self.num_params = feature_dim, num_params
        self.net = nn.Sequential(nn.Linear(feature_dim, hidden_dim), nn.ReLU(inplace=True), nn.Linear(hidden_dim, num_params))
        nn.init.zeros_(self.net[-1].weight)
        nn.init.zeros_(self.net[-1].bias)

    def forward(self, features: torch.Tensor) -> Dict[str, torch.Tensor]:
        Bn, C, H, W = features.shape
        p = self.net(features.permute(0, 2, 3, 1).reshape(Bn * H * W, C)).reshape(Bn, H, W, self.num_params)
        return {
            "aspect_ratio_mult": 1.0 + torch.tanh(p[..., 0]) * 0.5,     # [0.5, 1.5]
            "edge_threshold_add": torch.tanh(p[..., 1]) * 0.1,          # [-0.1, 0.1]
            "edge_shrink_mult": 1.0 + torch.tanh(p[..., 2]) * 0.3,      # [0.7, 1.3]
            "normal_strength_mult": 1.0 + torch.tanh(p[..., 3]) * 0.3,  # [0.7, 1.3]
            "base_size_mult": 1.0 + torch.tanh(p[..., 4]) * 0.5,        # [0.5, 1.5]
            "opacity_mult": 1.0 + torch.tanh(p[..., 5]) * 0.3,          # [0.7, 1.3]
        }


# =================================================================================================================================
# The reference's PhysicsDirectPatchDecoder (GDM:955-1147) with PhysicsFresnelZones (scripts/utils/fresnel_zones.py, "FZ": 400-614)
# =================================================================================================================================
class PhysicsFresnelZones(nn.Module):
    """The reference's PhysicsFresnelZones (FZ:400-614): phase from the optical path difference, phi = (2 pi / lambda) |depth -
    focal_depth|, and zone boundaries r_n = sqrt(n lambda f) normalised to [0, 1].  lambda = clamp(|_wavelength_raw|,
    wavelength_min, wavelength_max); `_wavelength_raw` is a parameter (learnable_wavelength) or a buffer.  Same constructor
    arguments and defaults, methods and state-dict key."""

    def __init__(self, num_zones: int = 8, wavelength: float = 0.05, focal_depth: float = 0.5, learnable_wavelength: bool = True,
                 wavelength_min: float = 0.01, wavelength_max: float = 0.5):
        super().__init__()
        self.num_zones, self.focal_depth = num_zones, focal_depth
        self.wavelength_min, self.wavelength_max = wavelength_min, wavelength_max
        if learnable_wavelength:
            self._wavelength_raw = nn.Parameter(torch.tensor(wavelength))
        else:
            self.register_buffer("_wavelength_raw", torch.tensor(wavelength))
        self.learnable_wavelength = learnable_wavelength

    @property
    def wavelength(self) -> torch.Tensor:
        return torch.clamp(torch.abs(self._wavelength_raw), self.wavelength_min, self.wavelength_max)

    def compute_zone_boundaries(self, device=None) -> torch.Tensor:
        """(num_zones + 1,) boundaries in [0, 1]: sqrt(n lambda f) over its last value (+ 1e-8)."""
        device = self._wavelength_raw.device if device is None else device
        n = torch.arange(self.num_zones + 1, device=device, dtype=torch.float32)
        r = torch.sqrt(n * self.wavelength * self.focal_depth)
        return r / (r[-1] + 1e-8)

    def get_zone_index(self, depth: torch.Tensor) -> torch.Tensor:
        idx = torch.bucketize(depth, self.compute_zone_boundaries(depth.device)[1:-1])
        return torch.clamp(idx, 0, self.num_zones - 1)

    def get_zone_phase(self, zone_idx: torch.Tensor) -> torch.Tensor:
        """Alternating 0, pi, 0, ..."""
        return (zone_idx % 2).float() * torch.pi

    def compute_path_difference(self, depth: torch.Tensor) -> torch.Tensor:
        return torch.abs(depth - self.focal_depth)

    def depth_to_phase(self, depth: torch.Tensor) -> torch.Tensor:
        """Unwrapped phase in radians."""
        return (2 * torch.pi / self.wavelength) * self.compute_path_difference(depth)

    def forward(self, depth: torch.Tensor, return_all: bool = False):
        phase = self.depth_to_phase(depth)
        if not return_all:
            return phase
        zone_idx = self.get_zone_index(depth)
        return {"phase": phase, "zone_idx": zone_idx, "zone_phase": self.get_zone_phase(zone_idx),
                "path_difference": self.compute_path_difference(depth), "boundaries": self.compute_zone_boundaries(depth.device),
                "wavelength": self.wavelength}

    def extra_repr(self) -> str:
        return (f"num_zones={self.num_zones}, wavelength={self.wavelength.item():.4f}, focal_depth={self.focal_depth}, "
                f"learnable={self.learnable_wavelength}")


class FresnelIntegralTables(nn.Module):
    """What the reference's FresnelDiffraction (FZ:828-903) adds to a PhysicsDirectPatchDecoder: three 1000-element buffers -- the
    sample points w in [0, 5] and running sums of cos(pi t^2 / 2) dt, sin(pi t^2 / 2) dt, the Fresnel integrals C(w), S(w).  The
    decoder constructs the module and never calls it (GDM:1027-1030), so only the buffers are mirrored; they
    exist so that checkpoints load strictly."""

    def __init__(self, wavelength: float = 0.05, lut_size: int = 1000, lut_max_w: float = 5.0):
        super().__init__()
        self.wavelength, self.lut_size, self.lut_max_w = wavelength, lut_size, lut_max_w
        w = torch.linspace(0, lut_max_w, lut_size)
        dt = w[1] - w[0]
        self.register_buffer("_w_lut", w)
        self.register_buffer("_C_lut", torch.cumsum(torch.cos(torch.pi * w ** 2 / 2), dim=0) * dt)
        self.register_buffer("_S_lut", torch.cumsum(torch.sin(torch.pi * w ** 2 / 2), dim=0) * dt)


def _physics_head_torch(raw, base_xy, base_z, wavelength_raw, K, focal_depth, wavelength_min, wavelength_max, xy_gain):
    """The head in torch ops, expression by expression as GDM:1085-1126 and FZ:463-467, 553, 569-573."""
    Bn, P = raw.shape[:2]
    o = raw[:, :, :K, :]
    z = base_z.view(Bn, P, 1).expand(Bn, P, K)
    positions = torch.stack([base_xy[:, 0].view(1, P, 1) + o[..., 0] * xy_gain, base_xy[:, 1].view(1, P, 1) + o[..., 1] * xy_gain, z],
                            dim=-1)
    scales = F.softplus(o[..., 3:6] + 1.0) * 0.15
    rotations = rotation_6d_to_quaternion(o[..., 6:12])
    colors = torch.sigmoid(o[..., 12:15])
    opacities = torch.sigmoid(o[..., 15])
    z_min, z_max = z.min(), z.max()
    z_normalized = (z - z_min) / (z_max - z_min + 1e-8)
    wavelength = torch.clamp(torch.abs(wavelength_raw), wavelength_min, wavelength_max)
    phases = ((2 * torch.pi / wavelength) * torch.abs(z_normalized - focal_depth)) % (2 * torch.pi)
    N = P * K
    return (positions.reshape(Bn, N, 3), scales.reshape(Bn, N, 3), rotations.reshape(Bn, N, 4), colors.reshape(Bn, N, 3),
            opacities.reshape(Bn, N), phases.reshape(Bn, N))


class _PhysicsHeadHip(torch.autograd.Function):
    """fgs_physics_forward / fgs_physics_backward.  Saved: the inputs and the 16 bytes of the range stage; the backward recomputes
    from `raw`.  The wavelength is read on the device: nothing synchronises with the host."""

    @staticmethod
    def forward(ctx, raw, base_xy, base_z, wavelength_raw, K, focal_depth, wavelength_min, wavelength_max, xy_gain):
        for t in (raw, base_z, wavelength_raw):
            hip.need_cuda(t, "physics_head (backend 'hip')")
        dev = raw.device
        Bn, P, KF, _ = raw.shape
        d = B.FgsPhysicsDims(Bn, P, KF, int(K), float(xy_gain), float(focal_depth), float(wavelength_min), float(wavelength_max))
        raw_, xy_, z_, wl_ = (_f32c(t) for t in (raw, base_xy, base_z, wavelength_raw))
        N = P * int(K)
        ctx.dims, ctx.scratch_bytes = d, B.sizes("fgs_physics_workspace_bytes", d)
        outs = [torch.empty((Bn, N, w) if w else (Bn, N), dtype=torch.float32, device=dev) for w in (3, 3, 4, 3, 0, 0)]
        rng = torch.empty(B.FGS_PHYSICS_RANGE_BYTES, dtype=torch.uint8, device=dev)
        scratch = torch.empty(ctx.scratch_bytes, dtype=torch.uint8, device=dev)
        hip.call(dev, "fgs_physics_forward", d, raw_, xy_, z_, wl_, *outs, rng, scratch)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(raw_, z_, wl_, rng)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *g_outs):
        raw_, z_, wl_, rng = ctx.saved_tensors
        d = ctx.dims
        gs = [_f32c(g) for g in g_outs]
        dev = raw_.device
        g_raw = torch.empty_like(raw_)
        g_z = torch.empty((d.batch, d.points), dtype=torch.float32, device=dev) if ctx.needs_input_grad[2] else None
        g_wl = torch.empty((), dtype=torch.float32, device=dev) if ctx.needs_input_grad[3] else None
        scratch = torch.empty(ctx.scratch_bytes, dtype=torch.uint8, device=dev)
        hip.call(dev, "fgs_physics_backward", d, raw_, z_, wl_, rng, *gs, g_raw, g_z, g_wl, scratch)
        return (g_raw, None, g_z, g_wl, None, None, None, None, None)


def physics_head(raw: torch.Tensor, base_xy: torch.Tensor, base_z: torch.Tensor, wavelength_raw: torch.Tensor, *,
                 num_gaussians: Optional[int] = None, focal_depth: float = 0.5, wavelength_min: float = 0.01,
                 wavelength_max: float = 0.5, xy_gain: float = 0.25, backend: str = "torch") -> Dict[str, torch.Tensor]:
    """The head of the reference's PhysicsDirectPatchDecoder (GDM:1071-1147): the MLP's raw (B, P, K_full, 16) output -> the wave
    renderer's inputs, N = P x K with K = min(num_gaussians, K_full): positions (B,N,3), scales (B,N,3) = softplus(raw + 1) 0.15
    (no clamps), rotations (B,N,4), colors (B,N,3), opacities (B,N) and phases (B,N) in radians in [0, 2 pi]: (2 pi / lambda) |u -
    focal_depth| mod 2 pi with u = (z - z_min) / (z_max - z_min + 1e-8) over the WHOLE batch and lambda = clamp(|wavelength_raw|,
    wavelength_min, wavelength_max).  base_xy (P,2): grid coordinates; base_z (B,P): depth_offset - 2 depth; wavelength_raw: a
    0-dim tensor on raw's device.  Gradients flow to raw, base_z (through the position, through u, and in equal shares through the
    minimum and maximum to every element that holds them) and wavelength_raw.
    backend "torch": the reference's expressions, any device.  backend "hip": csrc/fgs_physics.hip, two launches forward and
    three backward, bitwise repeatable, nothing read on the host (capturable); CUDA/ROCm tensors only."""
    if backend not in HEAD_BACKENDS:
        raise ValueError(f"unknown head backend {backend!r}: one of {HEAD_BACKENDS}")
    if raw.dim() != 4 or raw.shape[-1] != 16:
        raise ValueError(f"raw must be (B, P, K_full, 16), got {tuple(raw.shape)}")
    Bn, P, KF, _ = raw.shape
    K = KF if num_gaussians is None else max(1, min(int(num_gaussians), KF))
    if tuple(base_xy.shape) != (P, 2) or tuple(base_z.shape) != (Bn, P):
        raise ValueError(f"base_xy must be ({P}, 2) and base_z ({Bn}, {P}), got {tuple(base_xy.shape)} and {tuple(base_z.shape)}")
    if wavelength_raw.numel() != 1:
        raise ValueError(f"wavelength_raw must hold one value, got {tuple(wavelength_raw.shape)}")
    args = (raw, base_xy, base_z, wavelength_raw.reshape(()), K, focal_depth, wavelength_min, wavelength_max, xy_gain)
    outs = _PhysicsHeadHip.apply(*args) if backend == "hip" else _physics_head_torch(*args)
    return dict(zip(HEAD_OUTPUTS, outs))


class PhysicsDirectPatchDecoder(nn.Module):
    """The reference's PhysicsDirectPatchDecoder (GDM:955-1147): DirectPatchDecoder's grid and MLP, unclamped scales, no pose / edge
    inputs, and a phase COMPUTED from the depth by the wave equation with one (learnable) wavelength.  Same constructor arguments
    and defaults, forward signature (no elevation / azimuth: DESIGN.md section 7.6), returned dict, state-dict keys (mlp.net.*,
    depth_offset, fresnel_zones._wavelength_raw [, diffraction._{w,C,S}_lut]) and registration order.  `head_backend`: "torch" |
    "hip" (physics_head)."""

    def __init__(self, feature_dim: int = 384, gaussians_per_patch: int = 8, hidden_dims=(512, 512, 256, 128), dropout: float = 0.1,
                 wavelength: float = 0.05, learnable_wavelength: bool = True, focal_depth: float = 0.5,
                 use_diffraction_placement: bool = False, head_backend: str = "torch"):
        super().__init__()
        self.feature_dim, self.gaussians_per_patch, self.wavelength = feature_dim, gaussians_per_patch, wavelength
        self.use_diffraction_placement = use_diffraction_placement
        self.head_backend = _check_backend(head_backend)
        self.output_per_gaussian = 16
        self.mlp = _MLP(feature_dim, list(hidden_dims), gaussians_per_patch * 16, dropout)
        self.depth_offset = nn.Parameter(torch.tensor(-2.0))
        self.fresnel_zones = PhysicsFresnelZones(wavelength=wavelength, focal_depth=focal_depth,
                                                 learnable_wavelength=learnable_wavelength)
        self.diffraction = FresnelIntegralTables(wavelength=wavelength) if use_diffraction_placement else None
        self._grids = {}  # (H, W, device) -> (P, 2) grid coordinates

    _grid_xy = DirectPatchDecoder._grid_xy

    def forward(self, features: torch.Tensor, depth: Optional[torch.Tensor] = None, image_size: Tuple[int, int] = (518, 518),
                num_gaussians: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """features (B, C, H, W) channel-first; depth (B, 1, h, w) in [0, 1] or None; num_gaussians: progressive growing.
        -> positions, scales, rotations, colors, opacities, phases (B, N) radians."""
        Bn, C, H, W = features.shape
        raw = self.mlp(features.permute(0, 2, 3, 1).reshape(Bn * H * W, C)).reshape(Bn, H * W, self.gaussians_per_patch, 16)
        if depth is not None:
            depth_grid = F.interpolate(depth, (H, W), mode="bilinear", align_corners=False)
            base_z = self.depth_offset + depth_grid.reshape(Bn, H * W) * (-2)
        else:  # (the reference reads the offset with .item() here: no gradient to it, and none here; no host synchronisation)
            base_z = self.depth_offset.detach().reshape(1, 1).expand(Bn, H * W).contiguous()
        fz = self.fresnel_zones
        return physics_head(raw, self._grid_xy(H, W, features.device), base_z, fz._wavelength_raw, num_gaussians=num_gaussians,
                            focal_depth=fz.focal_depth, wavelength_min=fz.wavelength_min, wavelength_max=fz.wavelength_max,
                            xy_gain=0.25, backend=self.head_backend)
