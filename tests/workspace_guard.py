"""Guard-and-poison harness for the caller-owned buffers of the HIP entry points (tests/test_workspace_hygiene.py).

The product wrappers take `saved`, `scratch`, `stats` and every output / gradient tensor from torch's caching allocator
(`torch.empty`, `torch.empty_like`, `Tensor.new_empty`) and never look at them again.  The allocator rounds sizes up and hands a
freed block back to the next call of the same size, so a kernel that writes past a buffer lands in slack, and one that forgets
an element finds the right value of the previous call still in it.  While a `WorkspaceGuard` is active, every such allocation
made by the guarded modules is instead

    [ guard | the requested bytes | guard ]      all three parts filled with the active pattern

and the caller gets a view of the middle part.  `check()` then proves that no guard byte changed; running the same call under
the three PATTERNS and comparing the results bit for bit proves that every output element was written and that nothing was
read before it was written; snapshots prove that inputs were left alone (`run_patterns` does all of it).

Nothing here needs a GPU: the harness works on tensors of any device (tests/test_workspace_guard.py runs it on CPU stand-ins).
A plain module, not a conftest: it patches only inside `with WorkspaceGuard(...)` and restores everything on exit.
"""
import sys
import traceback

import torch

GUARD_BYTES = 4096  # a multiple of 512 B: the inner pointer keeps the 512-byte alignment of torch's caching allocator

# (name, 32-bit fill word as int32, its four bytes in memory order).  Gentle before harsh: a counter that is read before it is
# written shows up as a wrong VALUE under "zero" / "one" before 0xFFFFFFFF could turn it into a far-away index.
PATTERNS = (
    ("zero", 0, (0x00, 0x00, 0x00, 0x00)),   # bytes 0x00
    ("one", 1, (0x01, 0x00, 0x00, 0x00)),    # words 0x00000001: float 1e-45, integer 1
    ("ff", -1, (0xFF, 0xFF, 0xFF, 0xFF)),    # bytes 0xFF: float NaN, key 0xFFFFFFFF
)

_real_empty = torch.empty
_real_empty_like = torch.empty_like
_real_new_empty = torch.Tensor.new_empty


class HygieneError(AssertionError):
    """A buffer-contract violation found by the harness."""


def _pattern(p):
    if isinstance(p, str):
        for q in PATTERNS:
            if q[0] == p:
                return q
        raise KeyError(p)
    return p


def _size_args(size):
    if len(size) == 1 and not isinstance(size[0], int):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


def _capturing(device):
    return device.type == "cuda" and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _site(skip):
    """The call stack of an allocation, innermost last, without the harness's own frames."""
    frames = traceback.extract_stack(sys._getframe(skip), limit=4)
    return " < ".join(f"{f.filename.rsplit('/', 1)[-1]}:{f.lineno} {f.name}" for f in reversed(frames))


class _Record:
    __slots__ = ("order", "outer", "nbytes", "shape", "dtype", "site")

    def __init__(self, order, outer, nbytes, shape, dtype, site):
        self.order, self.outer, self.nbytes, self.shape, self.dtype, self.site = order, outer, nbytes, shape, dtype, site

    def describe(self):
        return f"allocation #{self.order} ({tuple(self.shape)} {str(self.dtype).replace('torch.', '')}, {self.nbytes} bytes) made at {self.site}"


class _TorchProxy:
    """Stands in for the name `torch` in a guarded module: `empty` / `empty_like` go to the guard, everything else to torch."""

    def __init__(self, guard):
        self.__dict__["_guard"] = guard

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, dtype=None, device=None, **kw):
        g = self._guard
        dtype = dtype if dtype is not None else torch.get_default_dtype()
        device = torch.device(device) if device is not None else torch.device("cpu")
        if kw or _capturing(device):
            return _real_empty(*size, dtype=dtype, device=device, **kw)
        return g.allocate(_size_args(size), dtype, device, _site(2))

    def empty_like(self, t, **kw):
        g = self._guard
        if kw or _capturing(t.device):
            return _real_empty_like(t, **kw)
        return g.allocate(tuple(t.shape), t.dtype, t.device, _site(2))


class WorkspaceGuard:
    """Context manager: allocations of `modules` come with guards and are filled with `pattern` (a PATTERNS entry or its name).

    `modules`: module objects whose global name `torch` is replaced while active (fresnel_amd.renderer, fresnel_amd.losses, ...);
    `Tensor.new_empty` is replaced for calls made from those modules.  A module with `release_scratch()` (the renderer's
    per-stream scratch cache, which bypasses torch.empty after the first call) is asked to drop its cache on entry, so the
    buffer is allocated again under guard -- unless `keep_scratch`, the stale-scratch cases, which fill the cached buffer in
    place with `poison()` instead.  Inactive under stream capture."""

    def __init__(self, pattern, modules, guard_bytes=GUARD_BYTES, keep_scratch=False):
        assert guard_bytes >= 4096 and guard_bytes % 512 == 0, "guard: a multiple of 512 B, at least 4096 B"
        self.name, self.word, self.bytes = _pattern(pattern)
        self.modules = list(modules)
        self.guard_bytes = guard_bytes
        self.keep_scratch = keep_scratch
        self.records = []
        self.count = 0
        self._saved = None

    # ---- patching -----------------------------------------------------------------------------------------------------------
    def __enter__(self):
        assert self._saved is None, "WorkspaceGuard is not re-entrant"
        self._saved = [(m, m.__dict__["torch"]) for m in self.modules]
        proxy = _TorchProxy(self)
        names = {m.__name__ for m in self.modules}
        guard = self

        def new_empty(t, *size, dtype=None, device=None, **kw):
            dev = torch.device(device) if device is not None else t.device
            if kw or sys._getframe(1).f_globals.get("__name__") not in names or _capturing(dev):
                return _real_new_empty(t, *size, dtype=dtype, device=device, **kw)
            return guard.allocate(_size_args(size), dtype if dtype is not None else t.dtype, dev, _site(2))

        for m in self.modules:
            m.torch = proxy
            if not self.keep_scratch and hasattr(m, "release_scratch"):
                m.release_scratch()
        torch.Tensor.new_empty = new_empty
        return self

    def __exit__(self, *exc):
        torch.Tensor.new_empty = _real_new_empty
        for m, t in self._saved:
            m.torch = t
            if hasattr(m, "release_scratch"):  # a guarded scratch buffer must not serve calls outside the guard
                m.release_scratch()
        self._saved = None
        return False

    # ---- allocation ---------------------------------------------------------------------------------------------------------
    def allocate(self, shape, dtype, device, site="?"):
        numel = 1
        for s in shape:
            numel *= s
        itemsize = _real_empty(0, dtype=dtype).element_size()
        nbytes = numel * itemsize
        g = self.guard_bytes
        total = (g + nbytes + g + 3) & ~3
        outer = _real_empty(total, dtype=torch.uint8, device=device)
        outer.view(torch.int32).fill_(self.word)
        inner = outer[g:g + nbytes].view(dtype).reshape(shape)
        self.count += 1
        self.records.append(_Record(self.count, outer, nbytes, shape, dtype, site))
        return inner

    def poison(self, t):
        """Fill an existing contiguous buffer (a cached scratch) with the pattern, in place."""
        flat = t.reshape(-1).view(torch.uint8)
        n4 = flat.numel() & ~3
        flat[:n4].view(torch.int32).fill_(self.word)
        if n4 < flat.numel():
            flat[n4:] = torch.tensor(self.bytes[:flat.numel() - n4], dtype=torch.uint8, device=t.device)

    def _expected(self, start, n, device):
        pat = torch.tensor(self.bytes, dtype=torch.uint8, device=device)
        return pat[(torch.arange(start, start + n, device=device)) % 4]

    # ---- the guard check ----------------------------------------------------------------------------------------------------
    def check(self, when="", forget=False):
        """Every guard byte of every buffer allocated so far still holds the pattern (call after a synchronisation)."""
        g = self.guard_bytes
        problems = []
        for r in self.records:
            head = r.outer[:g]
            tail = r.outer[g + r.nbytes:]
            bad_h = head != self._expected(0, g, head.device)
            bad_t = tail != self._expected(g + r.nbytes, tail.numel(), tail.device)
            nh, nt = int(bad_h.sum()), int(bad_t.sum())
            if nh or nt:
                where = []
                if nt:
                    first = int(torch.nonzero(bad_t)[0])
                    where.append(f"{nt} byte(s) past the end, first at +{first}")
                if nh:
                    last = int(torch.nonzero(bad_h)[-1])
                    where.append(f"{nh} byte(s) before the start, nearest at -{g - last}")
                problems.append(f"guard bytes overwritten{' ' + when if when else ''} (pattern {self.name}): {r.describe()}: " + "; ".join(where))
        if forget:
            self.records = []
        if problems:
            raise HygieneError("\n".join(problems))


class _NoGuard:
    """The unpatched run: same interface, nothing patched."""
    name = "unpatched"

    def __init__(self, modules):
        self.modules = modules

    def __enter__(self):
        for m in self.modules:
            if hasattr(m, "release_scratch"):
                m.release_scratch()
        return self

    def __exit__(self, *exc):
        return False

    def check(self, when="", forget=False):
        pass

    def poison(self, t):
        pass


# ---- comparisons ----------------------------------------------------------------------------------------------------------------
def _bits(t):
    """(numel, itemsize) uint8 view of a tensor's elements, on the CPU."""
    t = t.detach()
    if t.is_complex():
        t = torch.view_as_real(t)
    t = t.contiguous().cpu()
    return t.reshape(-1, 1).view(torch.uint8) if t.numel() else torch.zeros(0, t.element_size(), dtype=torch.uint8)


def _first(mask_rows, shape):
    i = int(torch.nonzero(mask_rows)[0])
    idx = []
    for s in reversed(shape):
        idx.append(i % s)
        i //= s
    return tuple(reversed(idx))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def assert_inputs_untouched(inputs, snapshot, when=""):
    for k, t in inputs.items():
        if t is None:
            continue
        a, b = _bits(t), snapshot[k]
        if not torch.equal(a, b):
            rows = (a != b).any(dim=1)
            shape = tuple(torch.view_as_real(t).shape) if t.is_complex() else tuple(t.shape)
            raise HygieneError(f"input '{k}' was modified{' ' + when if when else ''}: {int(rows.sum())} element(s), first at index "
                               f"{_first(rows, shape)}")


def snapshot_inputs(inputs):
    return {k: _bits(t).clone() for k, t in inputs.items() if t is not None}


def assert_outputs_match(ref, got, ref_name, got_name, patterns=None):
    """Outputs of two runs of the same call are bitwise identical.  `patterns`: {run name: the four fill bytes} of the runs
    that were filled -- an element that holds its run's fill in both runs was never written."""
    assert set(ref) == set(got), f"runs returned different tensors: {sorted(ref)} ({ref_name}) vs {sorted(got)} ({got_name})"
    for k in ref:
        a, b = ref[k], got[k]
        if a is None and b is None:
            continue
        if a is None or b is None or a.shape != b.shape or a.dtype != b.dtype:
            raise HygieneError(f"output '{k}': {ref_name} and {got_name} differ in presence, shape or dtype")
        ba, bb = _bits(a), _bits(b)
        if torch.equal(ba, bb):
            continue
        rows = (ba != bb).any(dim=1)
        shape = tuple(torch.view_as_real(a).shape) if a.is_complex() else tuple(a.shape)
        shape = shape if shape else (1,)
        if patterns and ref_name in patterns and got_name in patterns:
            size = ba.shape[1]
            fill_a = torch.tensor((patterns[ref_name] * 2)[:size], dtype=torch.uint8)
            fill_b = torch.tensor((patterns[got_name] * 2)[:size], dtype=torch.uint8)
            unwritten = rows & (ba == fill_a).all(dim=1) & (bb == fill_b).all(dim=1)
            if bool(unwritten.any()):
                raise HygieneError(f"output '{k}': {int(unwritten.sum())} element(s) never written (they still hold the fill under "
                                   f"pattern {ref_name} and under pattern {got_name}), first at index {_first(unwritten, shape)}")
        i = int(torch.nonzero(rows)[0])
        va, vb = a.detach().cpu(), b.detach().cpu()
        if va.is_complex():
            va, vb = torch.view_as_real(va), torch.view_as_real(vb)
        raise HygieneError(f"output '{k}' depends on the initial content of a buffer (read before write, or a partly written "
                           f"element): {int(rows.sum())} element(s) differ between {ref_name} and {got_name}, first at index "
                           f"{_first(rows, shape)}: {va.reshape(-1)[i].item()!r} vs {vb.reshape(-1)[i].item()!r}")


def _sync(tensors):
    if any(t is not None and t.is_cuda for t in tensors):
        torch.cuda.synchronize()


def run_patterns(fn, inputs, modules, patterns=PATTERNS, unpatched=True, keep_scratch=False):
    """Run `fn(guard)` -> {name: tensor} under every pattern in order, then once unpatched.  After every run: guards intact,
    `inputs` ({name: tensor}) bitwise equal to their snapshot, outputs bitwise equal to the first run's.  A run starts only
    after the previous one has passed.  `fn` may call `guard.check("after forward")` between its own steps and
    `guard.poison(t)` on a cached buffer.  -> {run name: outputs}."""
    runs = {}
    fills = {_pattern(p)[0]: _pattern(p)[2] for p in patterns}
    first = None
    todo = [WorkspaceGuard(p, modules, keep_scratch=keep_scratch) for p in patterns] + ([_NoGuard(modules)] if unpatched else [])
    for guard in todo:
        snap = snapshot_inputs(inputs)
        with guard:
            out = fn(guard)
            _sync(list(inputs.values()) + list(out.values()))
            guard.check(f"at the end of the {guard.name} run")
            assert_inputs_untouched(inputs, snap, f"by the {guard.name} run")
            out = {k: (v.detach().clone() if v is not None else None) for k, v in out.items()}
        runs[guard.name] = out
        if first is None:
            first = guard.name
        else:
            assert_outputs_match(runs[first], out, first, guard.name, fills)
    return runs
