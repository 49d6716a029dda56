"""SAAG surface-aligned Gaussian clouds from depth, on HIP: the producer of the `{name}_saag.bin` caches that
`ImageDataset(load_saag=True)` reads and `--experiment 1` (SAAGRefinementNet) refines.

Mirrors what only the reference's C++ application can do (PointCloud::from_depth, center / normalize, to_surface_gaussians and
DepthMap::compute_surface_info, driven as its viewer drives them); kernels in csrc/fgs_surface.hip, contract in include/fgs.h.

    from fresnel_amd.surface import surface_gaussians, SurfaceGaussianParams
    clouds = surface_gaussians(depth, image)            # depth (B,H,W) in [0,1], image (B,3,H,W); one dict per image

    python -m fresnel_amd.surface --data_dir D [--image_size S] [--subsample K] [--batch_size B] [--overwrite] [--<parameter> V]
                                  [--guide CHECKPOINT]

`surface_gaussians` is a producer: it accepts no gradient.  `guided_surface_gaussians(depth, image, mods)` is the feature-guided
variant (the reference's experiment 3, decoder.FeatureGuidedSAAG): six of the generator's parameters are modulated per patch of
`mods`, and autograd carries dL/d rows back to `mods` through fgs_surface_guided_backward.  There is no CPU fallback.
"""
import argparse
import dataclasses
import sys
from pathlib import Path

import torch

from . import _binding as B
from . import _hip as hip

KEYS = ("positions", "scales", "rotations", "colors", "opacities")
# channels of a guide map, in the order of FeatureGuidedSAAG's dict (include/fgs.h, "Feature-guided SAAG")
MOD_KEYS = ("aspect_ratio_mult", "edge_threshold_add", "edge_shrink_mult", "normal_strength_mult", "base_size_mult", "opacity_mult")


@dataclasses.dataclass
class SurfaceGaussianParams:
    """FgsSurfaceParams (include/fgs.h): the reference's four parameter structs flattened, with its viewer's defaults."""
    fx: float = 0.0                     # <= 0: 0.8 x width (the viewer's focal length)
    fy: float = 0.0                     # <= 0: fx
    cx: float = 0.0                     # <= 0: the image centre
    cy: float = 0.0
    depth_scale: float = 2.5
    subsample: int = 1
    opacity: float = 0.9
    normalize_extent: float = 3.0       # <= 0: neither centred nor normalised
    base_size: float = 0.008
    aspect_ratio: float = 5.0
    edge_threshold: float = 0.15
    edge_shrink: float = 0.3
    min_confidence: float = 0.1
    gradient_scale: float = 50.0
    normal_strength: float = 1.0
    wrap_enabled: bool = True
    wrap_edge_threshold: float = 0.15
    wrap_layers: int = 3
    wrap_layer_spacing: float = 0.5
    wrap_opacity_falloff: float = 0.7
    wrap_max_angle: float = 75.0        # carried for completeness: the reference never reads it
    wrap_aspect: float = 2.0
    shell_enabled: bool = True
    shell_thickness: float = 0.3
    shell_back_opacity: float = 0.6
    shell_back_darken: float = 0.8
    shell_connect_walls: bool = True
    shell_wall_segments: int = 3
    shell_wall_opacity: float = 0.5
    shell_edge_threshold: float = 0.1
    density_enabled: bool = True
    density_gradient_threshold: float = 0.08
    density_extra_count: int = 4
    density_position_jitter: float = 0.6
    density_size_variance: float = 0.3
    density_opacity_scale: float = 0.7
    seed: int = 12345

    def to_c(self):
        c = B.FgsSurfaceParams()
        for f in dataclasses.fields(self):
            v = getattr(self, f.name)
            if f.type in (bool, "bool"):
                v = 1 if v else 0
            elif f.type in (int, "int"):
                if isinstance(v, bool) or int(v) != v:
                    raise B.FgsError(f"SurfaceGaussianParams.{f.name} must be an integer, got {v!r}")
                v = int(v) & 0xFFFFFFFF if f.name == "seed" else int(v)
                if not -2 ** 31 <= v < 2 ** 32:
                    raise B.FgsError(f"SurfaceGaussianParams.{f.name} = {v} is out of range")
            else:
                v = float(v)
            setattr(c, f.name, v)
        return c

    def max_rows_per_point(self):
        return 2 + self.shell_wall_segments + self.wrap_layers + self.density_extra_count


def workspace_bytes(batch, height, width, params=None):
    """fgs_surface_workspace_bytes: validates dims and params (FgsError) without touching a device."""
    dims = B.FgsSurfaceDims(int(batch), int(height), int(width))
    return B.sizes("fgs_surface_workspace_bytes", dims, (params or SurfaceGaussianParams()).to_c())


class SurfaceCount:
    """What fgs_surface_count left behind: everything `emit` needs.  `offsets` (B + 1,) int32 stays on the device;
    `offsets_host` is the one host read."""

    def __init__(self, dims, cparams, params, depth, color, scratch, offsets):
        self.dims, self.cparams, self.params = dims, cparams, params
        self.depth, self.color, self.scratch, self.offsets = depth, color, scratch, offsets
        self.offsets_host = None

    @property
    def points_per_image(self):
        s = self.params.subsample
        return ((self.dims.width + s - 1) // s) * ((self.dims.height + s - 1) // s)

    def flags(self):
        """(B, P) uint8 view of the per-point state in scratch: FGS_SURFACE_KEPT | BASE | BACK | WALLS | WRAPS | FILLS."""
        n = self.dims.batch * self.points_per_image
        return self.scratch[B.FGS_SURFACE_STATE_OFFSET:B.FGS_SURFACE_STATE_OFFSET + n].view(self.dims.batch, -1)

    def status(self):
        """First int32 of scratch after an emit: 1 when the emit refused to write (capacity below the total)."""
        return int(self.scratch[:4].view(torch.int32).item())


def count(depth, image=None, params=None):
    """Phase 1 (fgs_surface_count): depth (B,H,W) fp32 DEVICE, already curve-adjusted -> SurfaceCount.  No host read."""
    params = params or SurfaceGaussianParams()
    hip.need_cuda(depth, "surface_gaussians")
    if depth.dim() != 3 or (image is not None and (image.dim() != 4 or image.shape[1] != 3 or image.shape[0] != depth.shape[0]
                                                   or image.shape[2:] != depth.shape[1:])):
        raise B.FgsError(f"surface_gaussians: depth must be (B,H,W) and image (B,3,H,W), got {tuple(depth.shape)} and "
                         f"{None if image is None else tuple(image.shape)}")
    depth_ = depth.detach().contiguous().float()
    color_ = None if image is None else image.detach().to(depth.device).contiguous().float()
    Bn, H, W = depth_.shape
    dims, cp = B.FgsSurfaceDims(Bn, H, W), params.to_c()
    scratch = torch.empty(B.sizes("fgs_surface_workspace_bytes", dims, cp), dtype=torch.uint8, device=depth.device)
    offsets = torch.empty(Bn + 1, dtype=torch.int32, device=depth.device)
    hip.call(depth.device, "fgs_surface_count", dims, cp, depth_, scratch, offsets)
    return SurfaceCount(dims, cp, params, depth_, color_, scratch, offsets)


def emit(state, capacity=None, outputs=None):
    """Phase 2 (fgs_surface_emit) -> dict of the five concatenated tensors with `capacity` rows (default: the total).
    Reads the B + 1 offsets on the host (once per SurfaceCount) to size the outputs; a capacity below the total raises FgsError
    before anything is launched.  `outputs`: caller-allocated tensors to write into (tests)."""
    if state.offsets_host is None:
        state.offsets_host = state.offsets.cpu().tolist()   # THE host read: sizes the outputs
    total = state.offsets_host[-1]
    capacity = total if capacity is None else int(capacity)
    if capacity < total:
        raise B.FgsError(f"fgs_surface_emit: capacity {capacity} is below the {total} rows of this cloud")
    dev = state.depth.device
    if outputs is None:
        outputs = dict(positions=torch.empty(capacity, 3, dtype=torch.float32, device=dev),
                       scales=torch.empty(capacity, 3, dtype=torch.float32, device=dev),
                       rotations=torch.empty(capacity, 4, dtype=torch.float32, device=dev),
                       colors=torch.empty(capacity, 3, dtype=torch.float32, device=dev),
                       opacities=torch.empty(capacity, dtype=torch.float32, device=dev))
    emit_raw(state, outputs, capacity)
    return outputs


def emit_raw(state, outputs, capacity):
    """fgs_surface_emit as it is: no host-side comparison of `capacity` with the total (the kernel makes it: state.status())."""
    hip.call(state.depth.device, "fgs_surface_emit", state.dims, state.cparams, state.depth, state.color, state.scratch, state.offsets,
             *[outputs[k] for k in KEYS], int(capacity))


def surface_gaussians(depth, image=None, params=None, *, depth_exponent=0.7):
    """depth (B,H,W) | (B,1,H,W) | (H,W) in [0,1] on the GPU, image (B,3,H,W) | (3,H,W) or None (grey 0.7) -> one dict per
    image with positions (N,3), scales (N,3), rotations (N,4) wxyz, colors (N,3), opacities (N,): the keys of
    io.save_gaussians_to_binary and of the renderers.  The depth curve depth ** depth_exponent (the viewer's 0.7) is applied
    here, with torch.  One host read, of the B + 1 row offsets between the count and the emit, sizes the outputs."""
    if depth.requires_grad or (image is not None and image.requires_grad):
        raise B.FgsError("surface_gaussians is a producer: it accepts no gradient (detach the inputs)")
    if depth.dim() == 2:
        depth = depth.unsqueeze(0)
    elif depth.dim() == 4 and depth.shape[1] == 1:
        depth = depth[:, 0]
    if image is not None and image.dim() == 3:
        image = image.unsqueeze(0)
    state = count(depth.float().pow(float(depth_exponent)), image, params)
    out = emit(state)
    off = state.offsets_host
    return [{k: out[k][off[b]:off[b + 1]] for k in KEYS} for b in range(len(off) - 1)]


# ---- feature-guided emit ----------------------------------------------------------------------------------------------------------
def mods_tensor(mods):
    """FeatureGuidedSAAG's dict of six (B,Hp,Wp) maps, or a (B,6,Hp,Wp) tensor -> (B,6,Hp,Wp) (part of the autograd graph)."""
    if isinstance(mods, dict):
        missing = [k for k in MOD_KEYS if k not in mods]
        if missing:
            raise B.FgsError(f"guide maps: missing {missing}")
        mods = torch.stack([mods[k] for k in MOD_KEYS], dim=1)
    if mods.dim() != 4 or mods.shape[1] != len(MOD_KEYS):
        raise B.FgsError(f"guide maps must be (B,6,Hp,Wp), got {tuple(mods.shape)}")
    return mods


def _check_mods(state, mods):
    if not mods.is_cuda or mods.device != state.depth.device:
        raise B.FgsError("guide maps must live on the depth's GPU; there is no CPU fallback")
    if mods.dim() != 4 or mods.shape[0] != state.dims.batch or mods.shape[1] != len(MOD_KEYS):
        raise B.FgsError(f"guide maps must be ({state.dims.batch},6,Hp,Wp), got {tuple(mods.shape)}")
    return mods.detach().contiguous().float()


def emit_guided_raw(state, mods, outputs, point_rows, capacity):
    """fgs_surface_emit_guided as it is (mods: (B,6,Hp,Wp) fp32 contiguous)."""
    hip.call(state.depth.device, "fgs_surface_emit_guided", state.dims, state.cparams, state.depth, state.color, state.scratch,
             state.offsets, mods, int(mods.shape[2]), int(mods.shape[3]), *[outputs[k] for k in KEYS], point_rows, int(capacity))


def _emit_guided_detached(state, mods, capacity=None):
    if state.offsets_host is None:
        state.offsets_host = state.offsets.cpu().tolist()   # THE host read: sizes the outputs
    total = state.offsets_host[-1]
    capacity = total if capacity is None else int(capacity)
    if capacity < total:
        raise B.FgsError(f"fgs_surface_emit_guided: capacity {capacity} is below the {total} rows of this cloud")
    dev = state.depth.device
    outputs = dict(positions=torch.empty(capacity, 3, dtype=torch.float32, device=dev),
                   scales=torch.empty(capacity, 3, dtype=torch.float32, device=dev),
                   rotations=torch.empty(capacity, 4, dtype=torch.float32, device=dev),
                   colors=torch.empty(capacity, 3, dtype=torch.float32, device=dev),
                   opacities=torch.empty(capacity, dtype=torch.float32, device=dev))
    point_rows = torch.empty(state.dims.batch, state.points_per_image, dtype=torch.int32, device=dev)
    emit_guided_raw(state, mods, outputs, point_rows, capacity)
    return outputs, point_rows


def guided_backward(state, mods, point_rows, g_positions=None, g_scales=None, g_rotations=None, g_opacities=None):
    """fgs_surface_guided_backward: upstream gradients of the rows (None = zeros) -> dL/d mods (B,6,Hp,Wp), every element written."""
    mods = _check_mods(state, mods)
    Hp, Wp = int(mods.shape[2]), int(mods.shape[3])
    nbytes = B.sizes("fgs_surface_guided_backward_bytes", state.dims, state.cparams, Hp, Wp)
    total = state.offsets_host[-1] if state.offsets_host is not None else None
    grads = []
    for name, g, width in (("positions", g_positions, 3), ("scales", g_scales, 3), ("rotations", g_rotations, 4), ("opacities", g_opacities, 0)):
        if g is not None:
            g = g.detach().contiguous().float()
            rows = g.shape[0] if g.dim() else 0
            if not g.is_cuda or (total is not None and rows < total) or tuple(g.shape[1:]) != ((width,) if width else ()):
                raise B.FgsError(f"guided_backward: the gradient of {name} has shape {tuple(g.shape)} for a cloud of {total} rows")
        grads.append(g)
    g_mods = torch.empty(mods.shape, dtype=torch.float32, device=mods.device)
    bwd_scratch = torch.empty(nbytes, dtype=torch.uint8, device=mods.device) if nbytes else None
    hip.call(mods.device, "fgs_surface_guided_backward", state.dims, state.cparams, state.depth, state.scratch, state.offsets, mods,
             Hp, Wp, point_rows, *grads, g_mods, bwd_scratch)
    return g_mods


class _GuidedEmit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mods, state):
        m = _check_mods(state, mods)
        out, point_rows = _emit_guided_detached(state, m)
        ctx.state, ctx.in_dtype = state, mods.dtype
        ctx.save_for_backward(m, point_rows)
        ctx.mark_non_differentiable(out["colors"], point_rows)
        ctx.set_materialize_grads(False)
        return tuple(out[k] for k in KEYS) + (point_rows,)

    @staticmethod
    def backward(ctx, g_pos, g_scale, g_rot, g_col, g_op, g_rows):
        m, point_rows = ctx.saved_tensors
        return guided_backward(ctx.state, m, point_rows, g_pos, g_scale, g_rot, g_op).to(ctx.in_dtype), None


def emit_guided(state, mods):
    """Phase 2 with a guide (fgs_surface_emit_guided): `state` of `count`, `mods` FeatureGuidedSAAG's dict or (B,6,Hp,Wp) -> dict
    of the five concatenated tensors plus `point_rows` (B,P) int32, the first row of every point with a base row (-1: none).
    Differentiable with respect to `mods` (fgs_surface_guided_backward).  One host read, of the offsets, as `emit`."""
    out = _GuidedEmit.apply(mods_tensor(mods), state)
    return dict(zip(KEYS + ("point_rows",), out))


def guided_surface_gaussians(depth, image, mods, params=None, *, depth_exponent=0.7):
    """`surface_gaussians` with the generator's aspect ratio, edge threshold, edge shrink, normal strength, base size and opacity
    modulated per patch by `mods` (decoder.FeatureGuidedSAAG's dict of six (B,Hp,Wp) maps, or a (B,6,Hp,Wp) tensor on the GPU).
    One dict per image; the tensors are views of the concatenated outputs, so autograd flows back to `mods`.  `depth` and `image`
    accept no gradient.  Counts, offsets and row order are those of the plain cloud; identity maps (1, 0, 1, 1, 1, 1) give its bits."""
    if depth.requires_grad or (image is not None and image.requires_grad):
        raise B.FgsError("guided_surface_gaussians: depth and image accept no gradient (detach them)")
    if depth.dim() == 2:
        depth = depth.unsqueeze(0)
    elif depth.dim() == 4 and depth.shape[1] == 1:
        depth = depth[:, 0]
    if image is not None and image.dim() == 3:
        image = image.unsqueeze(0)
    state = count(depth.float().pow(float(depth_exponent)), image, params)
    out = emit_guided(state, mods)
    off = state.offsets_host
    return [{k: out[k][off[b]:off[b + 1]] for k in KEYS} for b in range(len(off) - 1)]


# ---- command line ---------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(
        prog="python -m fresnel_amd.surface",
        description="Write {name}_saag.bin (N x 14 float32 SAAG Gaussians) for every image of a data directory that has a "
                    "{name}_depth.bin cache, where ImageDataset(load_saag=True) looks for it.",
        epilog="Clouds of different images differ in size, and the training loader stacks the clouds of a batch only when their "
               "sizes agree: train --experiment 1 with batch size 1, or on images whose clouds have equal counts.")
    ap.add_argument("--data_dir", required=True)
    ap.add_argument("--feature_cache_dir", default=None, help="where the caches live (default: <data_dir>/features)")
    ap.add_argument("--image_size", type=int, default=256)
    ap.add_argument("--batch_size", type=int, default=8, help="images per kernel call")
    ap.add_argument("--max_images", type=int, default=None)
    ap.add_argument("--depth_exponent", type=float, default=0.7)
    ap.add_argument("--overwrite", action="store_true", help="replace existing _saag.bin files (default: refuse)")
    ap.add_argument("--guide", default=None, metavar="CHECKPOINT",
                    help="modulate the clouds with a trained --experiment 3 checkpoint (decoder.FeatureGuidedSAAG) applied to each "
                         "image's cached DINOv2 features (default: the plain generator)")
    for f in dataclasses.fields(SurfaceGaussianParams):
        if f.type in (bool, "bool"):
            ap.add_argument("--" + f.name, type=int, choices=(0, 1), default=int(f.default))
        else:
            ap.add_argument("--" + f.name, type=int if f.type in (int, "int") else float, default=f.default)
    return ap


def params_from_args(args):
    return SurfaceGaussianParams(**{f.name: (bool(getattr(args, f.name)) if f.type in (bool, "bool") else getattr(args, f.name))
                                    for f in dataclasses.fields(SurfaceGaussianParams)})


def load_guide(path, feature_dim):
    """The FeatureGuidedSAAG of an --experiment 3 checkpoint ({model_state_dict: ...} or a bare state dict), strictly loaded."""
    from .decoder import FeatureGuidedSAAG
    ck = torch.load(path, map_location="cpu", weights_only=True)
    sd = ck.get("model_state_dict", ck)
    model = FeatureGuidedSAAG(feature_dim=feature_dim, num_params=sd["net.2.weight"].shape[0], hidden_dim=sd["net.0.weight"].shape[0])
    model.load_state_dict(sd, strict=True)
    return model.eval()


def main(argv=None, generator=None, out=None):
    """`generator(depth (B,H,W), image (B,3,H,W), params, depth_exponent=) -> list of dicts`: surface_gaussians on the GPU by
    default (tests pass a stub).  With --guide it is also given `mods=` (B,6,37,37), the checkpoint's maps of the batch's cached
    features, and defaults to guided_surface_gaussians."""
    from .data import ImageDataset
    from . import io as fio
    args = build_parser().parse_args(argv)
    out = out or sys.stdout
    params = params_from_args(args)
    ds = ImageDataset(args.data_dir, image_size=args.image_size, feature_cache_dir=args.feature_cache_dir,
                      max_images=args.max_images)
    cache = Path(ds.feature_cache_dir)
    todo = []
    for idx, path in enumerate(ds.image_paths):
        name = path.stem
        if not (cache / f"{name}_depth.bin").exists():
            print(f"{name}: no {name}_depth.bin, skipped", file=out)
            continue
        todo.append((idx, name, cache / f"{name}_saag.bin"))
    existing = [str(t) for _, _, t in todo if t.exists()]
    if existing and not args.overwrite:
        print(f"refusing to overwrite {len(existing)} existing file(s), e.g. {existing[0]}: pass --overwrite", file=sys.stderr)
        return 2
    guide = load_guide(args.guide, ds.feature_dim) if args.guide else None
    if generator is None:
        def generator(depth, image, params, depth_exponent, mods=None):
            dev = torch.device("cuda")
            if mods is None:
                return surface_gaussians(depth.to(dev), image.to(dev), params, depth_exponent=depth_exponent)
            return guided_surface_gaussians(depth.to(dev), image.to(dev), mods.to(dev), params, depth_exponent=depth_exponent)
    for i in range(0, len(todo), max(1, args.batch_size)):
        chunk = todo[i:i + max(1, args.batch_size)]
        items = [ds._step_tensors(idx) for idx, _, _ in chunk]
        depth = torch.stack([it[3][0] for it in items])
        image = torch.stack([it[1] for it in items])
        extra = {}
        if guide is not None:
            with torch.no_grad():
                extra["mods"] = mods_tensor(guide(torch.stack([it[2] for it in items]).float()))
        clouds = generator(depth, image, params, depth_exponent=args.depth_exponent, **extra)
        clouds = [{k: v.detach() for k, v in c.items()} for c in clouds]
        for (_, name, target), cloud in zip(chunk, clouds):
            fio.save_gaussians_to_binary(str(target), cloud)
            print(f"{name}: {cloud['positions'].shape[0]} Gaussians -> {target}", file=out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
