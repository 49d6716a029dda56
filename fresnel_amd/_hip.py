"""Host call layer: the one way from a torch tensor to an entry point of libfgs_hip.so.

The wrapper modules (renderer, losses, decoder, surface, handoff) validate, allocate and save; what they hand to the library goes
through `call`, which takes the device, the stream, the pointers and the return code in one place.  Sizes come from
`_binding.sizes` (ctypes only).  Nothing here allocates: every `saved`, `scratch`, output and gradient buffer stays in the module
that owns it (tests/workspace_guard.py patches those modules).
"""
import ctypes

import torch

from . import _binding as B


def ptr(t):
    """Device address of a tensor as a plain int, None (NULL) for None.  Every table symbol has `argtypes`, so ctypes widens the
    int to a `void *` itself; building a c_void_p per pointer costs ~0.1 us, times twelve to nineteen pointers per launch."""
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_handle(dev=None):
    """hipStream_t of the current stream of `dev`, by default of the current device.  (torch.cuda.current_stream().cuda_stream
    builds a Stream object per call: ~7 us, twice per image on the per-image route; the raw getter is ~0.3 us.)"""
    idx = torch.cuda.current_device() if dev is None or dev.index is None else dev.index
    if _raw_stream is not None:
        return _raw_stream(idx)
    return torch.cuda.current_stream(idx).cuda_stream


class on_device:
    """`with torch.cuda.device(dev)` without its cost when `dev` is current already (the usual case: ~11 us per image saved
    on the per-image route, profiles/r05_host_profile_config1.txt)."""
    __slots__ = ("idx", "prev")

    def __init__(self, dev):
        self.idx = dev.index

    def __enter__(self):
        self.prev = torch.cuda.current_device()
        if self.idx is not None and self.idx != self.prev:
            torch.cuda.set_device(self.idx)
        else:
            self.prev = None
        return self

    def __exit__(self, *a):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)


def f32c(t):
    """float32, contiguous, detached -- without a dispatcher call when the tensor already is (the usual case).  None stays None."""
    if t is None:
        return None
    if t.dtype is torch.float32 and t.is_contiguous():
        return t.detach() if t.requires_grad else t
    return t.detach().contiguous().float()


def need_cuda(t, who):
    if not t.is_cuda:
        raise B.FgsError(f"{who} needs CUDA/ROCm tensors; there is no CPU fallback")


def _plan(params):
    """All the table says about a call: the positions of the arguments that go by reference (structures) and through `ptr` (tensors
    or None; scalars stay as they are), how many arguments the caller gives, whether the stream follows them."""
    kinds = [kind for kind, _ in params if kind != "stream"]
    return (tuple(i for i, k in enumerate(kinds) if k.endswith("*")), tuple(i for i, k in enumerate(kinds) if k == "ptr"),
            len(kinds), len(kinds) < len(params))


_PLAN = {name: _plan(params) for name, (_, params) in B.SIGNATURES.items()}  # worked out once, not per call


def call(dev, name, *args):
    """Launch entry point `name` for tensors on `dev`: with `dev` current, on its current stream, return code checked.  `dev` is
    a torch.device, or the entered `on_device` of a caller that allocates under it (the rasterizer's per-image route: one device
    enter and one stream read per call)."""
    if type(dev) is not on_device:
        with on_device(dev) as held:
            return call(held, name, *args)
    by_ref, by_ptr, count, has_stream = _PLAN[name]
    if len(args) != count:
        raise TypeError(f"{name} takes {count} arguments{' and the stream' if has_stream else ''}, got {len(args)}")
    argv = list(args)
    for i in by_ref:
        argv[i] = ctypes.byref(argv[i])
    for i in by_ptr:  # (`ptr`, written out: a frame per pointer is what this route counts)
        if argv[i] is not None:
            argv[i] = argv[i].data_ptr()
    if has_stream:
        argv.append(stream_handle())
    rc = getattr(B.load(), name)(*argv)
    if rc:
        B.check(rc, name)
