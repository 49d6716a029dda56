"""Host-side mirror of the reference renderer interface, backed by hand-written HIP kernels.

Same names, argument meaning and error behaviour as the reference's
scripts/models/differentiable_renderer.py ("DR"):

    Camera                                   DR:24-95
    TileBasedRenderer(__init__ / forward)    DR:434-450, DR:489-499, DR:684-686

plus the `GaussianRenderer` torch.autograd.Function that BASELINE.json's north_star names
(the reference has no autograd.Function; its backward is whatever autograd derives from the
per-Gaussian Python loop, DR:582-667).

PyTorch is plumbing here (device memory, streams, autograd graph); all arithmetic runs in
libfgs_hip.so through the C ABI of include/fgs.h.  There is NO CPU fallback: calling the
renderer without CUDA tensors or without the built library raises.
"""
import math
from typing import Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn

from . import _binding as B
from . import _hip as hip


class Camera:
    """Simple pinhole camera model (same fields and defaults as DR:27-52)."""

    def __init__(self, fx: float, fy: float, cx: float, cy: float, width: int, height: int,
                 near: float = 0.01, far: float = 100.0):
        self.fx = fx
        self.fy = fy
        self.cx = cx
        self.cy = cy
        self.width = width
        self.height = height
        self.near = near
        self.far = far
        # identity = camera at origin looking down -Z (DR:47-48)
        self.view_matrix = torch.eye(4)
        self._packed = None  # (key, device tensor): the camera record is uploaded once, not once per call

    def set_view(self, view_matrix: torch.Tensor):
        """Set view matrix (world-to-camera transform), DR:50-52."""
        self.view_matrix = view_matrix
        self._packed = None

    def project(self, points_3d: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Project (N,3) world points to pixel coordinates + depths (DR:54-86); torch ops."""
        ones = torch.ones(points_3d.shape[0], 1, device=points_3d.device)
        homo = torch.cat([points_3d, ones], dim=1)
        view = self.view_matrix.to(points_3d.device)
        pc = (view @ homo.T).T[:, :3]
        x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
        z = torch.clamp(z.abs(), min=self.near) * torch.sign(z + 1e-8)
        u = self.fx * x / (-z) + self.cx
        v = self.fy * (-y) / (-z) + self.cy
        return torch.stack([u, v], dim=1), -z

    def get_intrinsics(self) -> torch.Tensor:
        return torch.tensor([[self.fx, 0, self.cx], [0, self.fy, self.cy], [0, 0, 1]], dtype=torch.float32)

    def packed(self) -> list:
        """The FGS_CAMERA_FLOATS-float device record of include/fgs.h."""
        v = self.view_matrix.detach().to("cpu", torch.float32).reshape(16).tolist()
        return v + [float(self.fx), float(self.fy), float(self.cx), float(self.cy),
                    float(self.near), float(self.far), 0.0, 0.0]


    def packed_tensor(self, device) -> torch.Tensor:
        """(1, FGS_CAMERA_FLOATS) device record, cached until the camera changes (fields, set_view, or an in-place
        edit of view_matrix): the reference re-uploads the view matrix on every call (DR:151); one H2D copy per
        camera is enough."""
        vm = self.view_matrix
        key = (str(device), float(self.fx), float(self.fy), float(self.cx), float(self.cy), float(self.near),
               float(self.far), _tensor_version(vm))
        # the cache entry holds the matrix OBJECT it was built from (compared with `is`: an id() alone can be reused
        # by a later tensor once this one is freed) and a copy of its 16 values (catches edits through .data, which
        # leave _version unchanged; view matrices live on the host, so this costs no device sync)
        c = self._packed
        if c is None or c[0] != key or c[2] is not vm or (not vm.is_cuda and not torch.equal(c[3], vm)):
            self._packed = (key, torch.tensor([self.packed()], dtype=torch.float32, device=device), vm,
                            vm.detach().clone() if not vm.is_cuda else None)
        return self._packed[1]


def create_camera_from_pose(elevation_rad: float, azimuth_rad: float, render_size: int,
                            focal_length_mult: float = 0.8, distance: float = 2.0) -> Camera:
    """Orbit camera looking at the origin (same formula and defaults as the reference's
    create_camera_from_pose, TGD:684-757): used for multi-pose training / novel-view evaluation.
    A list of such cameras can be passed to the batched renderer (one per image)."""
    import numpy as np
    cam = np.array([distance * np.cos(elevation_rad) * np.sin(azimuth_rad), distance * np.sin(elevation_rad),
                    distance * np.cos(elevation_rad) * np.cos(azimuth_rad)])
    fwd = -cam
    nrm = np.linalg.norm(fwd)
    fwd = np.array([0.0, 0.0, -1.0]) if nrm < 1e-6 else fwd / nrm
    right = np.cross(fwd, np.array([0.0, 1.0, 0.0]))
    rn = np.linalg.norm(right)
    right = np.array([1.0, 0.0, 0.0]) if rn < 1e-6 else right / rn
    up = np.cross(right, fwd)
    R = np.array([right, up, -fwd])
    t = -R @ cam
    view = torch.eye(4)
    view[:3, :3] = torch.from_numpy(R).float()
    view[:3, 3] = torch.from_numpy(t).float()
    camera = Camera(fx=render_size * focal_length_mult, fy=render_size * focal_length_mult,
                    cx=render_size / 2, cy=render_size / 2, width=render_size, height=render_size)
    camera.set_view(view)
    return camera


def pack_cameras(cameras: Union[Camera, Sequence[Camera]], device) -> torch.Tensor:
    if isinstance(cameras, Camera):
        return cameras.packed_tensor(device)
    return torch.tensor([c.packed() for c in cameras], dtype=torch.float32, device=device)


def _tensor_version(t):
    """Version counter of a tensor, or None for an inference tensor (created under torch.inference_mode(): it tracks no
    version -- reading `_version` raises -- and cannot be edited in place outside inference mode; callers treat None as
    "cannot tell": the cache is then keyed by object identity and value, or refreshed).  ADVICE r4."""
    try:
        return t._version
    except RuntimeError:
        return None


def _phase_channels(ph: torch.Tensor) -> int:
    """Phases are (B,N) -- one per Gaussian -- or (B,N,3) per colour channel (DR:772-776, DR:1170-1176); the kernels
    read exactly that many floats per Gaussian, so anything else is refused here (a (B,N,1) tensor is NOT three
    channels)."""
    if ph.dim() == 2:
        return 1
    if ph.dim() == 3 and ph.shape[2] in (1, 3):
        return int(ph.shape[2])
    raise ValueError(f"phases must be (N,) or (N,3) per image, got {tuple(ph.shape[1:])}")


class _Cfg:
    """Static (non-tensor) configuration of one renderer call."""

    def __init__(self, width, height, background, max_radius, use_phase, phase_amplitude, saturation_skip=False,
                 tuning=None, pair_counter=None, dup_capacity=0, workspace=None):
        self.dup_capacity = int(dup_capacity)  # FgsDims.dup_capacity of a fixed-capacity call (0 = worst case)
        self.workspace = workspace             # the renderer's _Workspace (policy + per-shape record), or None
        self.pair_counter = pair_counter  # optional device int64[1 | 3]: [0] += composited Gaussian-pixels, [1] += tile duplicates, [2] += Gaussians of every forward
        self.saturation_skip = bool(saturation_skip)
        self.tuning = dict(tuning) if tuning else None  # FgsDims.seg_len / fwd_variant / bin_mode overrides
        self.width, self.height = int(width), int(height)
        self.background = tuple(float(b) for b in background)
        self.max_radius = float(max_radius)
        self.use_phase = bool(use_phase)
        self.phase_amplitude = float(phase_amplitude)


# ---- host-side cost of one call (round 5: the per-image drop-in route, INTEGRATION.md route A, makes B small calls per step) ----
# FgsDims and the two workspace sizes are pure functions of the call's shape and configuration: built once per distinct key.
_DIMS_CACHE: dict = {}


def _shape_key(Bn, N, cfg, use_phase, num_cameras):
    """Everything but the duplicate capacity that FgsDims is made of: one CapacityTracker per such key."""
    tuning = getattr(cfg, "tuning", None)
    return (Bn, N, cfg.width, cfg.height, cfg.max_radius, cfg.background, use_phase, cfg.phase_amplitude, num_cameras,
            getattr(cfg, "saturation_skip", False), tuple(sorted(tuning.items())) if tuning else None)


def _dims_for(Bn, N, cfg, use_phase, num_cameras, dup_capacity=0):
    """-> (FgsDims, saved bytes, scratch bytes, byte offset of saved.counters) for the call shape and capacity."""
    tuning = getattr(cfg, "tuning", None)
    key = _shape_key(Bn, N, cfg, use_phase, num_cameras) + (int(dup_capacity),)
    hit = _DIMS_CACHE.get(key)
    if hit is None:
        dims = B.make_dims(Bn, N, cfg.width, cfg.height, cfg.max_radius, cfg.background, use_phase=use_phase,
                           phase_amplitude=cfg.phase_amplitude, num_cameras=num_cameras,
                           saturation_skip=getattr(cfg, "saturation_skip", False), tuning=tuning, dup_capacity=dup_capacity)
        if len(_DIMS_CACHE) > 256:
            _DIMS_CACHE.clear()
        hit = _DIMS_CACHE[key] = (dims,) + tuple(B.workspace_bytes(dims)) + (int(B.saved_layout(dims).counters),)
    return hit


# ---- right-sized workspaces (FgsDims.dup_capacity) ------------------------------------------------------------------------------
def quantise_capacity(x: int) -> int:
    """The smallest value >= x with at most four significant bits: steps of at most 12.5 %, so a demand that wanders a
    little settles on ONE capacity (one FgsDims, one block size for torch's caching allocator)."""
    x = int(x)
    if x <= 16:
        return max(x, 1)
    step = 1 << (x.bit_length() - 4)
    return (x + step - 1) // step * step


class CapacityTracker:
    """Host-only policy of the adaptive workspace mode, one per call shape: turns the duplicate demands that completed
    forwards reported (saved.counters[3]) into the capacity hint of the next forward.

        capacity = quantise_capacity(ceil(margin x max(demand of the last `window` observations))),  0 (= worst case) before
        the first observation and whenever that reaches the worst case.

    `margin` and `window` are policy defaults, not measured quantities.  An overflowed call reports its demand like any
    other, so the call after its readback has room."""
    margin = 1.25
    window = 8

    def __init__(self, worst_case: int, margin: Optional[float] = None, window: Optional[int] = None):
        self.worst_case = int(worst_case)
        if margin is not None:
            self.margin = float(margin)
        if window is not None:
            self.window = int(window)
        if not self.margin >= 1.0 or self.window < 1:
            raise ValueError("CapacityTracker: margin >= 1 and window >= 1")
        self.demands: list = []   # the last `window` demands, oldest first
        self.last_demand = None   # of the last completed observation
        self.overflows = 0        # observations whose call had overflowed

    def observe(self, demand: int, overflowed: bool = False):
        self.demands.append(int(demand))
        del self.demands[:-self.window]
        self.last_demand = int(demand)
        self.overflows += 1 if overflowed else 0

    def capacity(self) -> int:
        """FgsDims.dup_capacity for the next call (0 = worst case)."""
        if not self.demands:
            return 0
        peak = max(self.demands)
        want = quantise_capacity(max(math.ceil(self.margin * peak), peak, 1))
        return 0 if want >= self.worst_case else want


class _ShapeState:
    """Tracker + the asynchronous readback of one call shape: a small ring of pinned host slots, each with an event."""
    SLOTS = 4

    def __init__(self, worst_case):
        self.tracker = CapacityTracker(worst_case)
        self.slots = []      # [pinned int32[4], event, busy]
        self.pending = []    # busy slots, oldest first
        self.capacity = 0    # of the last call
        self.bytes = 0       # saved + scratch of the last call

    def poll(self):
        """Fold in the readbacks that have completed; never waits."""
        while self.pending and self.pending[0][1].query():
            slot = self.pending.pop(0)
            c = slot[0].tolist()
            self.tracker.observe(c[3] & 0xFFFFFFFF, overflowed=c[1] != 0)
            slot[2] = False

    def read_back(self, counters):
        """Enqueue the copy of saved.counters[0:4] to a free pinned slot (none free: this call goes unobserved)."""
        slot = next((s for s in self.slots if not s[2]), None)
        if slot is None:
            if len(self.slots) >= self.SLOTS:
                return
            slot = [torch.empty(4, dtype=torch.int32, pin_memory=True), torch.cuda.Event(), False]
            self.slots.append(slot)
        slot[0].copy_(counters, non_blocking=True)
        slot[1].record()
        slot[2] = True
        self.pending.append(slot)


class _Workspace:
    """Workspace policy of one renderer and what workspace_stats() reports: per call shape, the capacity and the bytes of the last
    call.  mode "adaptive" also learns the capacity from the previous forwards of the shape without a host synchronisation (its
    first call runs at the worst case); "worst" and "fixed" only keep the record."""

    def __init__(self, mode="worst", fixed=0):
        self.mode, self.fixed = mode, int(fixed)
        self.shapes: dict = {}

    def state(self, key, worst_case_of):
        st = self.shapes.get(key)
        if st is None:
            st = self.shapes[key] = _ShapeState(worst_case_of())
        return st

    def stats(self) -> dict:
        return {k: dict(last_demand=st.tracker.last_demand, capacity=st.capacity, bytes=st.bytes,
                        overflows=st.tracker.overflows) for k, st in self.shapes.items()}


def parse_workspace(workspace):
    """TileBasedRenderer's `workspace` argument -> ("worst" | "adaptive" | "fixed", fixed capacity)."""
    if isinstance(workspace, str):
        if workspace in ("worst", "adaptive"):
            return workspace, 0
        raise ValueError(f"workspace must be 'worst', 'adaptive' or a positive duplicate capacity, got {workspace!r}")
    if isinstance(workspace, bool) or not isinstance(workspace, int) or not 1 <= workspace <= 0xFFFFFFFF:
        raise ValueError(f"workspace must be 'worst', 'adaptive' or a positive duplicate capacity, got {workspace!r}")
    return "fixed", int(workspace)


# `scratch` lives only for the duration of one fgs_forward / fgs_backward call, and calls on one stream run in order: ONE
# buffer per (device, stream), grown to the largest request, serves them all.  (`saved` goes from a forward to its backward and
# several forwards may be pending -- the per-image loop -- so it stays a fresh tensor from torch's caching allocator.)
_SCRATCH: dict = {}


def _scratch_for(dev, nbytes, shrink=False):
    # `shrink` (calls of a renderer whose workspace is not "worst"): a cached buffer more than twice the request is replaced --
    # the first, worst-case call of an adaptive renderer would otherwise keep a worst-case scratch for the life of the process.
    # Default renderers keep the grow-only buffer.
    # under stream capture (torch.cuda.graph) the buffer must come from the graph's own memory pool and belong to that graph alone:
    # a cached buffer would be baked into the graph AND handed to later eager calls on a stream with the same handle
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    key = (dev.index, hip.stream_handle(dev))
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < nbytes or (shrink and buf.numel() > 2 * nbytes):
        buf = _SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return buf


def release_scratch():
    """Drop the cached scratch buffers (their memory goes back to torch's caching allocator; torch.cuda.empty_cache() then
    returns it to the device).  Safe at any time: the next call allocates again."""
    _SCRATCH.clear()


_f32c = hip.f32c


def forward_raw(positions, scales, rotations, colors, opacities, phases, cam_tensor, cfg):
    """fgs_forward without autograd: returns (out_rgb, out_depth, saved, dims, input tensors)."""
    if not positions.is_cuda:
        raise B.FgsError("GaussianRenderer (HIP) needs CUDA/ROCm tensors; there is no CPU fallback "
                         "(the CPU oracle lives under oracle/ and is test infrastructure only)")
    Bn, N = positions.shape[0], positions.shape[1]
    dev = positions.device
    pos, scl, rot, col, opa = _f32c(positions), _f32c(scales), _f32c(rotations), _f32c(colors), _f32c(opacities)
    ph = _f32c(phases) if (cfg.use_phase and phases is not None) else None
    cam_tensor = _f32c(cam_tensor)
    ws = getattr(cfg, "workspace", None)
    capacity = getattr(cfg, "dup_capacity", 0)
    state, adaptive = None, False
    if ws is not None:
        args = (Bn, N, cfg, ph is not None, cam_tensor.shape[0])
        state = ws.state(_shape_key(*args), lambda: int(B.saved_layout(_dims_for(*args)[0]).dup_capacity))
        capacity = ws.fixed
        # (under stream capture: no polling and no readback -- the captured graph freezes the capacity in hand)
        adaptive = ws.mode == "adaptive" and not torch.cuda.is_current_stream_capturing()
        if ws.mode == "adaptive":
            if adaptive:
                state.poll()
            capacity = state.tracker.capacity()
    dims, saved_bytes, scratch_bytes, counters_off = _dims_for(Bn, N, cfg, ph is not None, cam_tensor.shape[0], capacity)
    shrink = ws is not None and ws.mode != "worst"  # (the functional entry with a fixed dup_capacity keeps the grow-only cache)
    with hip.on_device(dev) as held:  # (also for the scratch cache's capture test and the readback's event)
        saved = torch.empty(saved_bytes, dtype=torch.uint8, device=dev)
        scratch = _scratch_for(dev, scratch_bytes, shrink)
        out_rgb = torch.empty((Bn, 3, cfg.height, cfg.width), dtype=torch.float32, device=dev)
        out_depth = torch.empty((Bn, cfg.height, cfg.width), dtype=torch.float32, device=dev)
        hip.call(held, "fgs_forward", dims, cam_tensor, pos, scl, rot, col, opa, ph, out_rgb, out_depth, saved, scratch)
        if state is not None:
            state.capacity, state.bytes = capacity, saved_bytes + scratch_bytes
            if adaptive:
                state.read_back(saved[counters_off:counters_off + 16].view(torch.int32))
    return out_rgb, out_depth, saved, dims, (pos, scl, rot, col, opa, ph)


class GaussianRenderer(torch.autograd.Function):
    """Batched differentiable rasterizer: (B,N,.) Gaussians + cameras -> (B,3,H,W), (B,H,W).

    forward  -> fgs_forward   (project, depth sort, tile binning, composite)
    backward -> fgs_backward  (composite backward, projection backward)
    """

    @staticmethod
    def forward(ctx, positions, scales, rotations, colors, opacities, phases, cam_tensor, cfg: _Cfg):
        out_rgb, out_depth, saved, dims, tensors = forward_raw(
            positions, scales, rotations, colors, opacities, phases, cam_tensor, cfg)
        pos, scl, rot, col, opa, ph = tensors
        if getattr(cfg, "pair_counter", None) is not None:
            # unit of work of SURVEY 8d, counted on the device and accumulated asynchronously (no host sync)
            n = torch.empty(1, dtype=torch.int64, device=pos.device)
            hip.call(pos.device, "fgs_count_pairs", dims, saved, n)
            cfg.pair_counter[:1] += n
            if cfg.pair_counter.numel() >= 3:  # [1]: tile duplicates D (saved.counters[0]), [2]: Gaussians -- for the algorithmic HBM bytes
                L = B.saved_layout(dims)
                cfg.pair_counter[1:2] += saved[L.counters:L.counters + 4].view(torch.int32).to(torch.int64)
                cfg.pair_counter[2:3] += int(dims.batch) * int(dims.num_gaussians)
        ctx.dims = dims
        ctx.scratch_bytes = _dims_for(pos.shape[0], pos.shape[1], cfg, ph is not None, cam_tensor.shape[0], dims.dup_capacity)[2]
        ws = getattr(cfg, "workspace", None)
        ctx.shrink_scratch = ws is not None and ws.mode != "worst"
        ctx.has_phase = ph is not None
        ctx.save_for_backward(pos, scl, rot, col, opa, ph if ph is not None else pos.new_empty(0),
                              cam_tensor, saved)
        return out_rgb, out_depth

    @staticmethod
    def backward(ctx, g_rgb, g_depth):
        pos, scl, rot, col, opa, ph, cam_tensor, saved = ctx.saved_tensors
        dims = ctx.dims
        dev = pos.device
        ph = ph if ctx.has_phase else None
        g_rgb = (g_rgb if g_rgb is not None else torch.zeros(dims.batch, 3, dims.height, dims.width, device=dev))
        g_depth = (g_depth if g_depth is not None else torch.zeros(dims.batch, dims.height, dims.width, device=dev))
        g_rgb, g_depth = _f32c(g_rgb), _f32c(g_depth)
        with hip.on_device(dev) as held:
            scratch = _scratch_for(dev, ctx.scratch_bytes, ctx.shrink_scratch)
            g_pos, g_scl, g_rot = torch.empty_like(pos), torch.empty_like(scl), torch.empty_like(rot)
            g_col, g_opa = torch.empty_like(col), torch.empty_like(opa)
            g_ph = torch.empty_like(ph) if ph is not None else None
            hip.call(held, "fgs_backward", dims, cam_tensor, pos, scl, rot, col, opa, ph, saved, scratch, g_rgb, g_depth,
                     g_pos, g_scl, g_rot, g_col, g_opa, g_ph)
        return g_pos, g_scl, g_rot, g_col, g_opa, g_ph, None, None


def render_batch(positions, scales, rotations, colors, opacities, cameras, width, height,
                 background=(0.0, 0.0, 0.0), max_radius=64, phases=None, use_phase_blending=False,
                 phase_amplitude=0.25, cam_tensor=None, saturation_skip=False, tuning=None, pair_counter=None,
                 dup_capacity=0, workspace=None):
    """Functional batched entry point: tensors are (B,N,.); cameras is one Camera (shared by
    the batch, as in the reference's training loop TGD:1209-1223) or a list of B Cameras.
    `saturation_skip` (off by default = the reference's behaviour, every list entry composited): stop
    compositing 8x8 sub-tiles whose accumulated alpha has reached 1.0f (FgsDims.saturation_skip).
    `dup_capacity` (0 = worst case): size the workspaces for that many (tile, Gaussian) duplicates (FgsDims.dup_capacity); a
    call that needs more returns NaN images and zero gradients.  `workspace`: a renderer's policy object instead."""
    if workspace is not None and dup_capacity:
        raise ValueError("render_batch: give a fixed dup_capacity or an adaptive workspace, not both")
    if cam_tensor is None:
        cam_tensor = pack_cameras(cameras, positions.device)
    cfg = _Cfg(width, height, background, max_radius, use_phase_blending and phases is not None,
               phase_amplitude, saturation_skip, tuning, pair_counter, dup_capacity, workspace)
    return GaussianRenderer.apply(positions, scales, rotations, colors, opacities, phases, cam_tensor, cfg)


class TileBasedRenderer(nn.Module):
    """Drop-in for the reference's TileBasedRenderer (DR:412-686), HIP-backed.

    forward(positions (N,3), scales (N,3), rotations (N,4), colors (N,3), opacities (N,),
            camera, return_depth=False, phases=None) -> (3,H,W) or ((3,H,W), (H,W))

    Extension: the same call with a leading batch dimension (B,N,.) renders B images in one
    launch sequence and returns (B,3,H,W) [, (B,H,W)]; `camera` may then be a list of B.
    """

    def __init__(self, image_width: int, image_height: int,
                 background: Tuple[float, float, float] = (0.0, 0.0, 0.0), max_radius: int = 64,
                 use_phase_blending: bool = False, phase_amplitude: float = 0.25,
                 saturation_skip: bool = False, workspace: Union[str, int] = "worst"):
        super().__init__()
        # workspace: "worst" (default: room for every Gaussian touching every tile its radius cap allows), "adaptive" (per call
        # shape, the capacity the previous forwards needed x a margin, learnt without a host synchronisation; a scene that
        # outgrows it gives ONE call of NaN images and zero gradients -- which a training step skips -- and the next has room)
        # or an int (fixed FgsDims.dup_capacity)
        self.workspace_mode, self.dup_capacity = parse_workspace(workspace)
        self._workspace = _Workspace(self.workspace_mode, self.dup_capacity)
        self.saturation_skip = saturation_skip  # extension, off by default (see render_batch)
        self.tuning = None  # optional FgsDims work-split overrides (tests / A-B runs); never changes results
        self.pair_counter = None  # set to a device int64[1 | 3] tensor to accumulate composited Gaussian-pixels [, tile duplicates, Gaussians] (metrics)
        self.width = image_width
        self.height = image_height
        self.background = torch.tensor(background)  # plain tensor, as in DR:447
        self.max_radius = max_radius
        self.use_phase_blending = use_phase_blending
        self.phase_amplitude = phase_amplitude

    def forward(self, positions: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor,
                colors: torch.Tensor, opacities: torch.Tensor, camera, return_depth: bool = False,
                phases: Optional[torch.Tensor] = None):
        batched = positions.dim() == 3
        if not batched:
            positions, scales, rotations = positions[None], scales[None], rotations[None]
            colors, opacities = colors[None], opacities[None]
            if phases is not None:
                phases = phases[None]
        use_phase = self.use_phase_blending and phases is not None
        if use_phase and phases.dim() != 2:
            # the reference's phase path takes a scalar phase per Gaussian in [0,1] (DR:498,
            # DR:636-637); (N,3) phases make `phase - prev_phase` fail to broadcast there
            raise RuntimeError(
                f"TileBasedRenderer phase blending expects phases of shape (N,), got {tuple(phases.shape[1:])}")
        bg = tuple(float(b) for b in self.background.tolist())  # a plain HOST tensor (DR:447): no device sync
        if positions.shape[1] == 0:
            # no Gaussians at all: the reference's zero-visible branch (DR:545-552) -- background, zero depth
            Bn, dev = positions.shape[0], positions.device
            img = torch.tensor(bg, device=dev).view(1, 3, 1, 1).expand(Bn, 3, self.height, self.width) + positions.sum() * 0.0
            depth = torch.zeros(Bn, self.height, self.width, device=dev) + positions.sum() * 0.0
            if not batched:
                img, depth = img[0], depth[0]
            return (img, depth) if return_depth else img
        img, depth = render_batch(positions, scales, rotations, colors, opacities, camera, self.width,
                                  self.height, bg, self.max_radius, phases if use_phase else None,
                                  use_phase, self.phase_amplitude, saturation_skip=self.saturation_skip,
                                  tuning=self.tuning, pair_counter=self.pair_counter, workspace=self._workspace)
        if not batched:
            img, depth = img[0], depth[0]
        if return_depth:
            return img, depth
        return img

    def workspace_stats(self) -> dict:
        """Per call shape: {shape key: dict(last_demand, capacity, bytes, overflows)} -- the capacity of the last call (0 = worst
        case) and its saved + scratch bytes; with workspace="adaptive" also the demand of the last COMPLETED readback (None
        before the first, and in the other modes) and the overflows those readbacks showed.  Host values only."""
        return self._workspace.stats()


def inspect_saved(saved: torch.Tensor, dims) -> dict:
    """Typed views of the integer stages inside a `saved` workspace (parity tests)."""
    L = B.saved_layout(dims)
    Bn, N, T = dims.batch, dims.num_gaussians, L.tiles_x * L.tiles_y

    def view(off, count, dtype):
        nbytes = count * torch.empty(0, dtype=dtype).element_size()
        return saved[off:off + nbytes].view(dtype)

    out = dict(layout=L)
    out["rec"] = view(L.rec, Bn * N * 12, torch.float32).view(Bn, N, 12)
    out["depth_key"] = view(L.depth_key, Bn * N, torch.int32).view(Bn, N)
    out["tile_count"] = view(L.tile_count, Bn * N, torch.int32).view(Bn, N)
    out["order"] = view(L.order, Bn * N, torch.int32).view(Bn, N)
    out["dup_off"] = view(L.dup_off, Bn * N, torch.int32).view(Bn, N)
    out["counters"] = view(L.counters, 16, torch.int32)
    out["ranges"] = view(L.ranges, Bn * T * 2, torch.int32).view(Bn, T, 2)
    out["tile_order"] = view(L.tile_order, Bn * T, torch.int32)
    out["dup_ids"] = view(L.dup_ids, L.dup_capacity, torch.int32)
    out["pix_state"] = view(L.pix_state, Bn * 6 * dims.height * dims.width, torch.float32).view(
        Bn, 6, dims.height, dims.width)
    if L.seg_capacity:  # depth segments = work units of the backward (non-phase path)
        out["seg_off"] = view(L.seg_off, Bn * T + 1, torch.int32)
        out["seg_tile"] = view(L.seg_tile, L.seg_capacity, torch.int32)
        if L.unit_order < L.total_bytes:  # launch order of those units (blend path only; counters[2] entries are valid)
            out["unit_order"] = view(L.unit_order, L.seg_capacity, torch.int32)
        if 0 < L.fwd_open < L.total_bytes:  # halves the exiting forward's head left to the rest kernel (tuning key fwd_exit)
            out["fwd_open"] = view(L.fwd_open, Bn * T * 2, torch.int32).view(Bn, T, 2)
        if 0 < L.fwd_close < L.total_bytes:  # closing slot of the halves the head closed, -1 (0xFFFFFFFF) elsewhere (include/fgs.h)
            out["fwd_close"] = view(L.fwd_close, Bn * T * 2, torch.int32).view(Bn, T, 2)
        if 0 < L.rank_of < L.total_bytes:  # depth rank of every Gaussian in its image (the blend backward's tail verdict, tuning key bwd_tail)
            out["rank_of"] = view(L.rank_of, Bn * N, torch.int32).view(Bn, N)
    return out


# ------------------------------------------------------------------------------------------------
# Angular-spectrum path (BASELINE config 5)
# ------------------------------------------------------------------------------------------------
class AsmRenderer(torch.autograd.Function):
    """fgs_asm_forward / fgs_asm_backward: batched ASMWaveFieldRenderer (DR:1150-1344) on hipFFT."""

    @staticmethod
    def forward(ctx, positions, scales, rotations, colors, opacities, phases, wavelengths, cam_tensor, cfg):
        hip.need_cuda(positions, "AsmRenderer (HIP)")
        Bn, N = positions.shape[0], positions.shape[1]
        dev = positions.device
        pos, scl, rot, col, opa, ph = [t.detach().contiguous().float()
                                       for t in (positions, scales, rotations, colors, opacities, phases)]
        wl = wavelengths.detach().contiguous().float().to(dev)
        cam_tensor = cam_tensor.contiguous().float()
        d = B.FgsAsmDims()
        d.batch, d.num_gaussians, d.width, d.height = Bn, N, cfg["width"], cfg["height"]
        d.max_radius = float(cfg["max_radius"])
        for i in range(3):
            d.background[i] = float(cfg["background"][i])
        d.num_planes = int(cfg["num_depth_planes"])
        d.depth_near, d.depth_far = float(cfg["depth_range"][0]), float(cfg["depth_range"][1])
        d.focal_depth, d.pixel_pitch = float(cfg["focal_depth"]), float(cfg["pixel_pitch"])
        d.phase_channels = _phase_channels(ph)
        d.num_cameras = cam_tensor.shape[0]
        d.bin_mode = int(cfg.get("bin_mode", 0))  # FgsAsmDims.bin_mode: list-building override for A/B runs and tests
        with hip.on_device(dev):  # (the query builds this device's hipFFT plans and returns their work size)
            saved_bytes, ctx.scratch_bytes = B.sizes("fgs_asm_workspace_bytes", d)
        saved = torch.empty(saved_bytes, dtype=torch.uint8, device=dev)
        scratch = torch.empty(ctx.scratch_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(Bn, 3, cfg["height"], cfg["width"], dtype=torch.float32, device=dev)
        hip.call(dev, "fgs_asm_forward", d, cam_tensor, pos, scl, rot, col, opa, ph, wl, out, saved, scratch)
        ctx.dims = d
        ctx.save_for_backward(pos, scl, rot, col, opa, ph, wl, cam_tensor, saved)
        return out

    @staticmethod
    def backward(ctx, g_out):
        pos, scl, rot, col, opa, ph, wl, cam_tensor, saved = ctx.saved_tensors
        # fgs_asm_backward turns the plane fields in `saved` into their gradients IN PLACE (fgs.h): a second backward through this
        # node (retain_graph=True, two losses sharing the graph) would read them as fields
        if getattr(ctx, "consumed", False):
            raise RuntimeError("ASMWaveFieldRenderer: backward through this node a second time -- its saved plane fields were "
                               "consumed by the first backward; render again instead of retaining the graph")
        ctx.consumed = True
        d = ctx.dims
        dev = pos.device
        g_out = g_out.contiguous().float()
        scratch = torch.empty(ctx.scratch_bytes, dtype=torch.uint8, device=dev)
        g_pos, g_scl, g_rot = torch.empty_like(pos), torch.empty_like(scl), torch.empty_like(rot)
        g_col, g_opa, g_ph = torch.empty_like(col), torch.empty_like(opa), torch.empty_like(ph)
        g_wl = torch.empty_like(wl)
        hip.call(dev, "fgs_asm_backward", d, cam_tensor, pos, scl, rot, col, opa, ph, wl, saved, scratch, g_out,
                 g_pos, g_scl, g_rot, g_col, g_opa, g_ph, g_wl)
        return g_pos, g_scl, g_rot, g_col, g_opa, g_ph, g_wl, None, None


class _AsmPropagate(torch.autograd.Function):
    """fgs_asm_propagate_forward / backward: field (C,H,W) complex64, z scalar tensor, wavelengths (C,)."""

    @staticmethod
    def forward(ctx, field, z, wavelengths, pixel_pitch, band_limit):
        hip.need_cuda(field, "AngularSpectrumPropagator (HIP)")
        dev = field.device
        f = torch.view_as_real(field.detach().to(torch.complex64).contiguous())
        C, H, W = field.shape
        zt = z.detach().reshape(1).float().contiguous().to(dev)
        wl = wavelengths.detach().reshape(C).float().contiguous().to(dev)
        with hip.on_device(dev):  # (the query builds this device's hipFFT plan and returns its work size)
            scratch_bytes = B.sizes("fgs_asm_propagate_workspace_bytes", H, W, C)
        scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty_like(f)
        spec = torch.empty_like(f)
        hip.call(dev, "fgs_asm_propagate_forward", H, W, C, float(pixel_pitch), 1 if band_limit else 0, f, zt, wl, out, spec, scratch)
        ctx.cfg = (H, W, C, float(pixel_pitch), 1 if band_limit else 0, scratch_bytes)
        ctx.shapes = (z.shape, wavelengths.shape)
        ctx.save_for_backward(spec, zt, wl)
        return torch.view_as_complex(out)

    @staticmethod
    def backward(ctx, g_out):
        spec, zt, wl = ctx.saved_tensors
        H, W, C, pitch, bl, cbytes = ctx.cfg
        dev = spec.device
        g = torch.view_as_real(g_out.detach().to(torch.complex64).contiguous())
        scratch = torch.empty(cbytes, dtype=torch.uint8, device=dev)
        g_field = torch.empty_like(g)
        g_z = torch.empty(1, dtype=torch.float32, device=dev)
        g_wl = torch.empty(C, dtype=torch.float32, device=dev)
        hip.call(dev, "fgs_asm_propagate_backward", H, W, C, pitch, bl, spec, zt, wl, g, g_field, g_z, g_wl, scratch)
        return (torch.view_as_complex(g_field), g_z.reshape(ctx.shapes[0]) if ctx.needs_input_grad[1] else None,
                g_wl.reshape(ctx.shapes[1]) if ctx.needs_input_grad[2] else None, None, None)


class AngularSpectrumPropagator(nn.Module):
    """Angular Spectrum Method propagation of a complex field (same interface as DR:929-1065):
    U(z) = ifft2(fft2(U0) * exp(i 2 pi z sqrt(max(1/lambda^2 - fx^2 - fy^2, 0)))), per channel wavelength.
    Runs in libfgs_hip.so (fgs_asm_propagate_forward / backward: batched rocFFT + fused transfer-function kernels),
    differentiable in the field, the distance and the wavelengths."""

    def __init__(self, height: int, width: int, pixel_pitch: float = 1.0 / 256.0, wavelength: float = 0.05,
                 band_limit: bool = True):
        super().__init__()
        self.height, self.width = height, width
        self.pixel_pitch, self.wavelength, self.band_limit = pixel_pitch, wavelength, band_limit
        fx = torch.fft.fftfreq(width, d=pixel_pitch)
        fy = torch.fft.fftfreq(height, d=pixel_pitch)
        FX, FY = torch.meshgrid(fx, fy, indexing="xy")
        self.register_buffer("FX", FX)  # kept for interface parity (DR:963-964); the kernels form them on the fly
        self.register_buffer("FY", FY)

    def propagate(self, field, z_distance, wavelength=None):
        """field (H,W) or (H,W,C) complex; z_distance scalar tensor; wavelength None | scalar | (C,) tensor: channel c
        uses wavelength[c] when the tensor has more than c entries, else the tensor itself (DR:1035-1040)."""
        squeeze = field.dim() == 2
        if squeeze:
            field = field.unsqueeze(-1)
        C = field.shape[-1]
        dev = field.device
        if wavelength is None:
            wl = torch.full((C,), float(self.wavelength), device=dev)
        elif not torch.is_tensor(wavelength):
            wl = torch.full((C,), float(wavelength), device=dev)
        elif wavelength.dim() == 0:
            wl = wavelength.to(dev).expand(C)
        else:
            if len(wavelength) < C and len(wavelength) != 1:
                raise RuntimeError(f"wavelength has {len(wavelength)} entries for {C} channels")
            wl = wavelength.to(dev) if len(wavelength) >= C else wavelength.to(dev).expand(C)
            wl = wl[:C]
        if not torch.is_tensor(z_distance):
            z_distance = torch.tensor(float(z_distance), device=dev)
        out = _AsmPropagate.apply(field.permute(2, 0, 1), z_distance, wl, self.pixel_pitch, self.band_limit)
        out = out.permute(1, 2, 0)
        return out.squeeze(-1) if squeeze else out

    def forward(self, field, z_distance, wavelength=None):
        return self.propagate(field, z_distance, wavelength)


class _HostBackground:
    """The wave renderers keep `background` as a registered buffer like the reference (DR:705, DR:1103), but the kernels take
    it as three host floats in the dims -- reading the buffer back would be a device sync per call.  So the module keeps a
    host copy and re-reads the buffer only when it is ANOTHER tensor object or its version counter moved (an in-place edit,
    `load_state_dict`): the reference reads the buffer on every call, and so -- observably -- does this.  Moves
    (`.to(device)`, `.cuda()`) keep the values and are absorbed in `_apply` without a read-back."""

    def _init_background(self, background):
        self.register_buffer("background", torch.tensor(background))
        self._bg = [float(b) for b in background]
        self._bg_mark()

    def _bg_mark(self):
        object.__setattr__(self, "_bg_src", (self.background, _tensor_version(self.background)))

    def _bg_fresh(self, b):
        """The host copy still describes `b`: same object, same version.  An inference tensor has no version counter
        (_tensor_version -> None): it counts as stale -- one read-back per call instead of an exception."""
        v = _tensor_version(b)
        return b is self._bg_src[0] and v is not None and v == self._bg_src[1]

    def _apply(self, fn, *a, **k):
        stale = not self._bg_fresh(self.background)
        out = super()._apply(fn, *a, **k)
        if not stale:
            self._bg_mark()
        return out

    def _background_host(self):
        b = self.background
        if not self._bg_fresh(b):
            self._bg = [float(v) for v in b.detach().cpu().tolist()]
            self._bg_mark()
        return self._bg


class ASMWaveFieldRenderer(_HostBackground, nn.Module):
    """Drop-in for the reference's ASMWaveFieldRenderer (DR:1068-1344), HIP + hipFFT backed.

    forward(positions, scales, rotations, colors, opacities, camera, return_depth=False, phases=None,
            wavelengths_rgb=None) -> (3,H,W) [, zeros (H,W)]; phases (N,) or (N,3) radians are required
    (ValueError otherwise, DR:1187-1188).  wavelengths_rgb=None falls back to the scalar `wavelength`
    for all channels (the reference raises AttributeError there).  Batched (B,N,.) inputs
    render B images per call."""

    def __init__(self, image_width: int, image_height: int, background=(0.0, 0.0, 0.0), max_radius: int = 64,
                 num_depth_planes: int = 16, depth_range=(0.1, 2.0), focal_depth: float = 0.5,
                 pixel_pitch: float = 1.0 / 256.0, wavelength: float = 0.05):
        super().__init__()
        self.width, self.height = image_width, image_height
        self.max_radius = max_radius
        self.num_depth_planes = num_depth_planes
        self.depth_range = depth_range
        self.focal_depth = focal_depth
        self.pixel_pitch = pixel_pitch
        self.wavelength = wavelength
        self._init_background(background)
        self.register_buffer("depth_planes", torch.linspace(depth_range[0], depth_range[1], num_depth_planes))
        self.propagator = AngularSpectrumPropagator(image_height, image_width, pixel_pitch, wavelength)

    def forward(self, positions, scales, rotations, colors, opacities, camera, return_depth: bool = False,
                phases: Optional[torch.Tensor] = None, wavelengths_rgb: Optional[torch.Tensor] = None):
        if phases is None:
            raise ValueError("ASMWaveFieldRenderer requires phases tensor.")
        batched = positions.dim() == 3
        if not batched:
            positions, scales, rotations = positions[None], scales[None], rotations[None]
            colors, opacities, phases = colors[None], opacities[None], phases[None]
        if wavelengths_rgb is None:
            wavelengths_rgb = torch.full((3,), float(self.wavelength), device=positions.device)
        cfg = dict(width=self.width, height=self.height, max_radius=self.max_radius,
                   background=self._background_host(),
                   num_depth_planes=self.num_depth_planes, depth_range=self.depth_range,
                   focal_depth=self.focal_depth, pixel_pitch=self.pixel_pitch,
                   bin_mode=int(getattr(self, "bin_mode", 0)))  # tests set ren.bin_mode = 2 for the radix path
        cam_tensor = pack_cameras(camera, positions.device)
        img = AsmRenderer.apply(positions, scales, rotations, colors, opacities, phases, wavelengths_rgb,
                                cam_tensor, cfg)
        if not batched:
            img = img[0]
        if return_depth:
            shape = (img.shape[0], self.height, self.width) if batched else (self.height, self.width)
            return img, torch.zeros(shape, device=img.device)  # DR:1339-1342: depth map is all zeros
        return img


# ------------------------------------------------------------------------------------------------
# WaveFieldRenderer (--use_wave_rendering / --use_qsr)
# ------------------------------------------------------------------------------------------------
class WaveRenderer(torch.autograd.Function):
    """fgs_wave_forward / fgs_wave_backward: batched WaveFieldRenderer (DR:689-926)."""

    @staticmethod
    def forward(ctx, positions, scales, rotations, colors, opacities, phases, cam_tensor, cfg):
        hip.need_cuda(positions, "WaveRenderer (HIP)")
        Bn, N = positions.shape[0], positions.shape[1]
        dev = positions.device
        pos, scl, rot, col, opa, ph = [t.detach().contiguous().float()
                                       for t in (positions, scales, rotations, colors, opacities, phases)]
        cam_tensor = cam_tensor.contiguous().float()
        d = B.FgsWaveDims()
        d.batch, d.num_gaussians, d.width, d.height = Bn, N, cfg["width"], cfg["height"]
        d.max_radius = float(cfg["max_radius"])
        for i in range(3):
            d.background[i] = float(cfg["background"][i])
        d.phase_channels = _phase_channels(ph)
        d.num_cameras = cam_tensor.shape[0]
        saved_bytes, ctx.scratch_bytes = B.sizes("fgs_wave_workspace_bytes", d)
        saved = torch.empty(saved_bytes, dtype=torch.uint8, device=dev)
        scratch = torch.empty(ctx.scratch_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(Bn, 3, cfg["height"], cfg["width"], dtype=torch.float32, device=dev)
        dep = torch.empty(Bn, cfg["height"], cfg["width"], dtype=torch.float32, device=dev)
        hip.call(dev, "fgs_wave_forward", d, cam_tensor, pos, scl, rot, col, opa, ph, out, dep, saved, scratch)
        ctx.dims = d
        ctx.save_for_backward(pos, scl, rot, col, opa, ph, cam_tensor, saved)
        return out, dep

    @staticmethod
    def backward(ctx, g_out, g_dep):
        pos, scl, rot, col, opa, ph, cam_tensor, saved = ctx.saved_tensors
        d = ctx.dims
        dev = pos.device
        g_out = (g_out if g_out is not None else torch.zeros(d.batch, 3, d.height, d.width, device=dev)).contiguous().float()
        g_dep = (g_dep if g_dep is not None else torch.zeros(d.batch, d.height, d.width, device=dev)).contiguous().float()
        scratch = torch.empty(ctx.scratch_bytes, dtype=torch.uint8, device=dev)
        g_pos, g_scl, g_rot = torch.empty_like(pos), torch.empty_like(scl), torch.empty_like(rot)
        g_col, g_opa, g_ph = torch.empty_like(col), torch.empty_like(opa), torch.empty_like(ph)
        hip.call(dev, "fgs_wave_backward", d, cam_tensor, pos, scl, rot, col, opa, ph, saved, scratch, g_out, g_dep,
                 g_pos, g_scl, g_rot, g_col, g_opa, g_ph)
        return g_pos, g_scl, g_rot, g_col, g_opa, g_ph, None, None


class WaveFieldRenderer(_HostBackground, nn.Module):
    """Drop-in for the reference's WaveFieldRenderer (DR:689-926), HIP backed: complex amplitude
    accumulation U = sum A_i exp(i phi_i), I = |U|^2.  phases (N,) or (N,3) radians are required
    (ValueError otherwise, DR:779-780).  Batched (B,N,.) inputs render B images per call."""

    def __init__(self, image_width: int, image_height: int, background=(0.0, 0.0, 0.0), max_radius: int = 64):
        super().__init__()
        self.width, self.height = image_width, image_height
        self.max_radius = max_radius
        self._init_background(background)

    def forward(self, positions, scales, rotations, colors, opacities, camera, return_depth: bool = False,
                phases: Optional[torch.Tensor] = None):
        if phases is None:
            raise ValueError("WaveFieldRenderer requires phases tensor. Use PhysicsDirectPatchDecoder to generate phases.")
        batched = positions.dim() == 3
        if not batched:
            positions, scales, rotations = positions[None], scales[None], rotations[None]
            colors, opacities, phases = colors[None], opacities[None], phases[None]
        cfg = dict(width=self.width, height=self.height, max_radius=self.max_radius, background=self._background_host())
        img, dep = WaveRenderer.apply(positions, scales, rotations, colors, opacities, phases,
                                      pack_cameras(camera, positions.device), cfg)
        if not batched:
            img, dep = img[0], dep[0]
        return (img, dep) if return_depth else img


# ------------------------------------------------------------------------------------------------
# FourierGaussianRenderer (DR:1500-1774; --experiment 4 --use_phase_blending, TGD:1877-1890)
# ------------------------------------------------------------------------------------------------
class FourierRenderer(torch.autograd.Function):
    """fgs_fourier_forward / fgs_fourier_backward: batched FourierGaussianRenderer (DR:1500-1774) as a separable fp32 matrix
    product.  `saved` goes unchanged through the backward, so a retained graph may be differentiated again."""

    @staticmethod
    def forward(ctx, positions, scales, rotations, colors, opacities, cam_tensor, cfg):
        hip.need_cuda(positions, "FourierRenderer (HIP)")
        Bn, N = positions.shape[0], positions.shape[1]
        dev = positions.device
        pos, scl, rot, col, opa = [_f32c(t) for t in (positions, scales, rotations, colors, opacities)]
        cam_tensor = cam_tensor.contiguous().float()
        d = B.FgsFourierDims()
        d.batch, d.num_gaussians, d.width, d.height = Bn, N, cfg["width"], cfg["height"]
        for i in range(3):
            d.background[i] = float(cfg["background"][i])
        d.num_cameras = cam_tensor.shape[0]
        saved_bytes, ctx.scratch_bytes = B.sizes("fgs_fourier_workspace_bytes", d)
        saved = torch.empty(saved_bytes, dtype=torch.uint8, device=dev)
        scratch = torch.empty(ctx.scratch_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(Bn, 3, cfg["height"], cfg["width"], dtype=torch.float32, device=dev)
        hip.call(dev, "fgs_fourier_forward", d, cam_tensor, pos, scl, rot, col, opa, out, saved, scratch)
        ctx.dims = d
        ctx.save_for_backward(pos, scl, rot, col, opa, cam_tensor, saved)
        return out

    @staticmethod
    def backward(ctx, g_out):
        pos, scl, rot, col, opa, cam_tensor, saved = ctx.saved_tensors
        d = ctx.dims
        dev = pos.device
        g_out = g_out.contiguous().float()
        scratch = torch.empty(ctx.scratch_bytes, dtype=torch.uint8, device=dev)
        g_pos, g_scl, g_rot = torch.empty_like(pos), torch.empty_like(scl), torch.empty_like(rot)
        g_col, g_opa = torch.empty_like(col), torch.empty_like(opa)
        hip.call(dev, "fgs_fourier_backward", d, cam_tensor, pos, scl, rot, col, opa, saved, scratch, g_out,
                 g_pos, g_scl, g_rot, g_col, g_opa)
        return g_pos, g_scl, g_rot, g_col, g_opa, None, None


class FourierGaussianRenderer(_HostBackground, nn.Module):
    """Drop-in for the reference's FourierGaussianRenderer (DR:1500-1774), HIP backed: a dense, order-independent sum of
    isotropic Gaussians (sigma^2 = half the trace of the projected covariance), normalised by the image maximum and composed
    with the background.  As in the reference, `phases` and the wavelengths do not reach the image (`wavelengths.grad` stays
    None) and the depth map of `return_depth=True` is all zeros.  Batched (B,N,.) inputs render B images per call, each
    normalised by its own maximum, with one camera or B cameras."""

    def __init__(self, image_width: int, image_height: int, background=(0.0, 0.0, 0.0), wavelength_r: float = 0.0635,
                 wavelength_g: float = 0.05, wavelength_b: float = 0.041, learnable_wavelengths: bool = True,
                 focal_depth: float = 0.5):
        super().__init__()
        self.width, self.height = image_width, image_height
        self.focal_depth = focal_depth
        self._init_background(background)
        wavelengths = torch.tensor([wavelength_r, wavelength_g, wavelength_b])
        if learnable_wavelengths:
            self.wavelengths = nn.Parameter(wavelengths)
        else:
            self.register_buffer("wavelengths", wavelengths)
        self.learnable_wavelengths = learnable_wavelengths
        self.wavelength_min, self.wavelength_max = 0.01, 0.5

    def _get_constrained_wavelengths(self) -> torch.Tensor:
        return torch.clamp(torch.abs(self.wavelengths), self.wavelength_min, self.wavelength_max)

    def forward(self, positions, scales, rotations, colors, opacities, camera, return_depth: bool = False,
                phases: Optional[torch.Tensor] = None):
        batched = positions.dim() == 3
        if not batched:
            positions, scales, rotations = positions[None], scales[None], rotations[None]
            colors, opacities = colors[None], opacities[None]
        cfg = dict(width=self.width, height=self.height, background=self._background_host())
        img = FourierRenderer.apply(positions, scales, rotations, colors, opacities,
                                    pack_cameras(camera, positions.device), cfg)
        if not batched:
            img = img[0]
        if return_depth:
            shape = (img.shape[0], self.height, self.width) if batched else (self.height, self.width)
            return img, torch.zeros(shape, device=img.device)  # DR:1758-1764: the depth map is all zeros
        return img

    def extra_repr(self) -> str:
        lam = self._get_constrained_wavelengths()
        return (f"size=({self.height}, {self.width}), λ_rgb=[{lam[0]:.4f}, {lam[1]:.4f}, {lam[2]:.4f}], "
                f"learnable={self.learnable_wavelengths}")
