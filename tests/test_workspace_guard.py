"""Self-tests of the guard-and-poison harness (tests/workspace_guard.py) on CPU tensors: four deliberately bad stand-in
"kernels" written in plain torch must each be caught with the right message, a correct one must pass, and the harness must
leave torch exactly as it found it.  No GPU: these are the only part of the workspace-hygiene tests that runs everywhere."""
import sys

import pytest
import torch

import workspace_guard as WG

THIS = sys.modules[__name__]  # the stand-ins allocate through this module's name `torch`, which the guard replaces


# ---- stand-ins: y = 2 x + 1 over n floats with a scratch buffer, the way the product wrappers are written ----------------------
def _standin(x, mode):
    n = x.numel()
    scratch = torch.empty(n * 4, dtype=torch.uint8, device=x.device)  # like `scratch`: raw bytes
    y = torch.empty_like(x)
    tag = x.new_empty(0)
    s = scratch.view(torch.float32)
    if mode == "read_before_write":
        y.copy_(s)                 # reads scratch before anything wrote it ...
        y.mul_(0.0).add_(2 * x + 1)  # ... and keeps a trace of it (NaN * 0 = NaN, 1e-45 * 0 = 0 -> caught under "ff")
    else:
        s.copy_(2 * x)
        y.copy_(s + 1)
    if mode == "overrun":
        # one element past the end of y: as_strided reaches the memory behind the view, like a kernel with n + 1 threads
        torch.as_strided(y, (n + 1,), (1,))[n] = 7.0
    if mode == "underrun":
        torch.as_strided(scratch, (1,), (1,), scratch.storage_offset() - 1)[0] = 9
    if mode == "unwritten":
        y2 = torch.empty_like(x)
        y2[:n - 1] = y[:n - 1]     # the last element is forgotten
        y = y2
    if mode == "modifies_input":
        x[3] += 1.0
    return dict(y=y, tag=tag)


def _run(mode, n=37):
    x = torch.arange(n, dtype=torch.float32) / 8
    want = 2 * x.clone() + 1
    runs = WG.run_patterns(lambda guard: _standin(x, mode), dict(x=x), [THIS])
    return runs, want


def test_correct_standin_passes_under_every_pattern():
    runs, want = _run("ok")
    assert list(runs) == ["zero", "one", "ff", "unpatched"]
    for name, out in runs.items():
        assert torch.equal(out["y"], want), name
        assert out["tag"].numel() == 0


def test_write_past_the_end_is_caught():
    with pytest.raises(WG.HygieneError, match=r"guard bytes overwritten.*pattern zero.*\(37,\) float32, 148 bytes.*_standin.*"
                                              r"[1-4] byte\(s\) past the end, first at \+[0-3]\b"):
        _run("overrun")


def test_write_before_the_start_is_caught():
    with pytest.raises(WG.HygieneError, match=r"guard bytes overwritten.*uint8.*1 byte\(s\) before the start, nearest at -1"):
        _run("underrun")


def test_unwritten_output_element_is_caught():
    with pytest.raises(WG.HygieneError, match=r"output 'y': 1 element\(s\) never written.*first at index \(36,\)"):
        _run("unwritten")


def test_read_before_write_is_caught():
    with pytest.raises(WG.HygieneError, match=r"output 'y' depends on the initial content of a buffer.*37 element\(s\) differ "
                                              r"between zero and ff"):
        _run("read_before_write")


def test_modified_input_is_caught():
    with pytest.raises(WG.HygieneError, match=r"input 'x' was modified by the zero run: 1 element\(s\), first at index \(3,\)"):
        _run("modifies_input")


def test_patterns_and_order():
    assert [p[0] for p in WG.PATTERNS] == ["zero", "one", "ff"]
    for name, word, by in WG.PATTERNS:
        with WG.WorkspaceGuard(name, [THIS]) as g:
            t = torch.empty(5, dtype=torch.int32)
            f = torch.empty((2, 3), dtype=torch.float32)
            z = torch.empty((), dtype=torch.float32)
            d = torch.empty(3, dtype=torch.float64)
            b = torch.empty(7, dtype=torch.uint8)
            assert t.tolist() == [word] * 5 and tuple(f.shape) == (2, 3) and z.dim() == 0 and d.dtype == torch.float64
            assert b.tolist() == [by[i % 4] for i in range(7)]
            assert t.data_ptr() % 512 == g.records[0].outer.data_ptr() % 512  # the guard keeps the allocator's alignment
            assert len(g.records) == 5 and all(r.outer.numel() >= 2 * 4096 + r.nbytes for r in g.records)
            g.check()
    one = WG.PATTERNS[1]
    with WG.WorkspaceGuard(one, [THIS]):
        assert torch.empty(1, dtype=torch.float32).item() == pytest.approx(1.4e-45, rel=0.01)
    with WG.WorkspaceGuard("ff", [THIS]):
        assert torch.isnan(torch.empty(4, dtype=torch.float32)).all()


def test_a_later_pattern_runs_only_after_the_earlier_one_passed():
    seen = []

    def fn(guard):
        seen.append(guard.name)
        return _standin(x, "overrun")

    x = torch.zeros(8)
    with pytest.raises(WG.HygieneError):
        WG.run_patterns(fn, dict(x=x), [THIS])
    assert seen == ["zero"]


def test_guard_names_every_broken_buffer_and_its_order_number():
    with WG.WorkspaceGuard("one", [THIS]) as g:
        a = torch.empty(4, dtype=torch.float32)
        b = torch.empty(4, dtype=torch.float32)
        c = torch.empty(4, dtype=torch.float32)
        torch.as_strided(a, (5,), (1,))[4] = 0.0
        torch.as_strided(c, (6,), (1,))[5] = 0.0
        b.fill_(3.0)
        with pytest.raises(WG.HygieneError) as e:
            g.check("after forward")
    msg = str(e.value)
    assert "allocation #1 " in msg and "allocation #3 " in msg and "allocation #2 " not in msg
    assert "after forward" in msg and "test_workspace_guard.py" in msg


def test_poison_fills_a_cached_buffer_in_place():
    buf = torch.zeros(11, dtype=torch.uint8)
    WG.WorkspaceGuard("one", [THIS]).poison(buf)
    assert buf.tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0]
    WG.WorkspaceGuard("ff", [THIS]).poison(buf)
    assert buf.tolist() == [255] * 11


def test_patching_is_scoped_and_restored():
    real = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    assert THIS.torch is torch
    try:
        with WG.WorkspaceGuard("ff", [THIS]):
            assert THIS.torch is not WG.torch  # (inside the guard this module's own name `torch` is the proxy)
            assert WG.torch.Tensor.new_empty is not real[2]
            assert WG.torch.empty is real[0]  # other modules keep the real allocator ...
            import helpers
            assert not hasattr(helpers, "torch") or helpers.torch is WG.torch
            raise RuntimeError("leave through an exception")
    except RuntimeError:
        pass
    assert THIS.torch is torch
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == real
    assert torch.zeros(2).new_empty(3).shape == (3,)


def test_new_empty_from_other_modules_is_left_alone():
    with WG.WorkspaceGuard("ff", [THIS]) as g:
        n = len(g.records)
        torch.zeros(3).new_empty(2)        # from this (guarded) module: recorded
        assert len(g.records) == n + 1
        torch.nn.functional.pad(torch.zeros(3), (1, 1))  # torch's own Python code: not recorded, still works
        WG._real_new_empty(torch.zeros(3), 2)
        assert len(g.records) == n + 1


def test_product_modules_can_be_guarded_without_a_gpu():
    """The modules the GPU tests guard have the global `torch` the proxy replaces, and come back intact."""
    from fresnel_amd import handoff, losses, renderer
    mods = [renderer, losses, handoff]
    with WG.WorkspaceGuard("zero", mods):
        assert all(m.torch is not WG.torch for m in mods)
        assert renderer.torch.float32 is torch.float32 and renderer.torch.cuda is torch.cuda
        t = renderer.inspect_saved  # (uses torch.empty(0, dtype=...) for element sizes: must work under the guard)
        assert t is not None and renderer.torch.empty(0, dtype=torch.int32).element_size() == 4
    assert all(m.torch is torch for m in mods)
