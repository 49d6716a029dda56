"""The host side of the C ABI, checked without a GPU: the signature table of fresnel_amd/_binding.py and its ctypes structures
against include/fgs.h, name by name, and the call layer (fresnel_amd/_hip.py, _binding.sizes) against a recording stub."""
import ctypes
import os
import re

import pytest
import torch

from helpers import ROOT

from fresnel_amd import _binding as B
from fresnel_amd import _hip as hip

C_SCALARS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float,
             "double": ctypes.c_double, "size_t": ctypes.c_size_t, "int": ctypes.c_int}


# ---- include/fgs.h, parsed ------------------------------------------------------------------------------------------------------
def _header():
    txt = open(os.path.join(ROOT, "include", "fgs.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"//[^\n]*", "", txt)


def header_defines(txt):
    """{NAME: int} of the object-like macros with an integer value."""
    out = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\(?-?(?:0x[0-9a-fA-F]+|\d+)\)?)[ \t]*$", txt, flags=re.M):
        out[name] = int(value.strip("()"), 0)
    return out


_STRUCT = re.compile(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(Fgs\w+)\s*;", re.S)


def header_structs(txt):
    """{struct: [(field, C scalar type, array length as written or None), ...]} in declaration order."""
    out = {}
    for body, name in _STRUCT.findall(txt):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            ctype, names = decl.split(None, 1)
            for n in names.split(","):
                m = re.fullmatch(r"\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*", n)
                assert m, f"{name}: cannot parse {decl!r}"
                fields.append((m[1], ctype, m[2]))
        out[name] = fields
    return out


def _kind(ctype, name, last):
    words = ctype.replace("*", " * ").split()
    base = " ".join(w for w in words if w not in ("const", "*"))
    if "*" not in words:
        return base
    if base.startswith("Fgs") or base == "size_t":
        return base + "*"
    return "stream" if (base == "void" and name == "stream" and last) else "ptr"


def header_prototypes(txt):
    """{symbol: (return kind, ((kind, name), ...))} in the table's vocabulary (fresnel_amd/_binding.py)."""
    txt = _STRUCT.sub("", txt)
    txt = re.sub(r"^[ \t]*#.*$", "", txt, flags=re.M)
    txt = txt.replace('extern "C" {', "").replace("}", "")
    out = {}
    for stmt in filter(None, (s.strip() for s in txt.split(";"))):
        m = re.fullmatch(r"(.+?)\b(fgs_\w+)\s*\((.*)\)", stmt, flags=re.S)
        assert m, f"not a prototype: {stmt!r}"
        ret = {"int": "int", "size_t": "size_t", "const char *": "str"}[" ".join(m[1].split())]
        plist = [p.strip() for p in m[3].split(",")]
        params = []
        if plist != ["void"]:
            for i, p in enumerate(plist):
                pm = re.fullmatch(r"(.*?)(\w+)", p, flags=re.S)
                params.append((_kind(pm[1], pm[2], i == len(plist) - 1), pm[2]))
        out[m[2]] = (ret, tuple(params))
    return out


def table_mismatches(header, table):
    """Symbols whose return kind or (kind, name) list differs, or that one side lacks -> {symbol: (header's, table's)}."""
    return {s: (header.get(s), table.get(s)) for s in sorted(set(header) | set(table)) if header.get(s) != table.get(s)}


# ---- 1. header against table ----------------------------------------------------------------------------------------------------
def test_signature_table_matches_the_header():
    header = header_prototypes(_header())
    assert len(header) == len(B.EXPORTED_SYMBOLS) == len(B.SIGNATURES) > 60
    assert header["fgs_version"] == ("str", ()) and header["fgs_reduction_scratch_bytes"] == ("size_t", ())
    assert header["fgs_forward"][1][0] == ("FgsDims*", "dims") and header["fgs_forward"][1][-1] == ("stream", "stream")
    assert table_mismatches(header, B.SIGNATURES) == {}
    lib = B.load()
    for name, (ret, params) in header.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(params), name
        assert fn.restype is {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "str": ctypes.c_char_p}[ret], name
        for (kind, pname), at in zip(params, fn.argtypes):
            want = (ctypes.POINTER(getattr(B, kind[:-1], None) or ctypes.c_size_t) if kind.endswith("*")
                    else ctypes.c_void_p if kind in ("ptr", "stream") else C_SCALARS[kind])
            assert at is want, (name, pname, kind, at)


def test_the_comparer_reports_a_swap_and_a_dropped_parameter():
    header = header_prototypes(_header())
    doctored = dict(B.SIGNATURES)
    ret, params = doctored["fgs_backward"]
    i = [n for _, n in params].index("g_rgb")
    swapped = list(params)
    swapped[i], swapped[i + 1] = swapped[i + 1], swapped[i]   # two pointers of one kind: only the names tell
    doctored["fgs_backward"] = (ret, tuple(swapped))
    ret, params = doctored["fgs_saag_refine_backward"]
    doctored["fgs_saag_refine_backward"] = (ret, params[:7] + params[8:])
    del doctored["fgs_match_forward"]
    assert sorted(table_mismatches(header, doctored)) == ["fgs_backward", "fgs_match_forward", "fgs_saag_refine_backward"]


# ---- 2. header against structures -----------------------------------------------------------------------------------------------
def _field_shape(t):
    return (t._type_, t._length_) if issubclass(t, ctypes.Array) else (t, None)


def test_structures_match_the_header():
    txt = _header()
    defines, structs = header_defines(txt), header_structs(txt)
    python_side = {n for n in dir(B) if isinstance(getattr(B, n), type) and issubclass(getattr(B, n), ctypes.Structure)}
    assert set(structs) == python_side and len(structs) == 15
    arrays = {}
    for name, fields in structs.items():
        want = []
        for fname, ctype, length in fields:
            if length is not None and not length.isdigit():
                assert getattr(B, length) == defines[length], length   # the Python constant is the header's
                length = defines[length]
            want.append((fname, C_SCALARS[ctype], None if length is None else int(length)))
            if length is not None:
                arrays[f"{name}.{fname}"] = int(length)
        got = [(f, *_field_shape(t)) for f, t in getattr(B, name)._fields_]
        assert got == want, name
    assert arrays == {"FgsDims.background": 3, "FgsAsmDims.background": 3, "FgsWaveDims.background": 3,
                      "FgsFourierDims.background": 3, "FgsSsimDims.taps": 15, "FgsPixelLossDims.boundaries": 65}
    for macro, value in defines.items():   # every integer macro the binding restates under the header's name
        if hasattr(B, macro):
            assert getattr(B, macro) == value, macro
    assert (B.FWD_EXIT_OFF, B.FWD_EXIT_ON) == (defines["FGS_FWD_EXIT_OFF"], defines["FGS_FWD_EXIT_ON"])


# ---- 3. call layer against a recording stub -------------------------------------------------------------------------------------
STREAM = 0x5EED00


class StubLib:
    """Stands in for the CDLL: every fgs_* function records (name, args), writes `sizes` through `size_t *` arguments, returns
    `rc`."""

    def __init__(self, rc=0, sizes=(4096, 512)):
        self.rc, self.sizes, self.calls = rc, sizes, []

    def __getattr__(self, name):
        if not name.startswith("fgs_"):
            raise AttributeError(name)

        def fn(*args):
            if name == "fgs_last_error":
                return b"stub: no such luck"
            self.calls.append((name, args))
            outs = [a._obj for a in args if isinstance(getattr(a, "_obj", None), ctypes.c_size_t)]
            for o, v in zip(outs, self.sizes):
                o.value = v
            return self.rc
        return fn


@pytest.fixture
def stub(monkeypatch):
    """-> (stub library, event log): the library, the raw stream getter and torch's device calls replaced; device 0 is current."""
    lib, events, current = StubLib(), [], [0]

    def set_device(i):
        events.append(("set", i))
        current[0] = i

    def raw_stream(i):
        events.append(("stream", i))
        return STREAM + i

    monkeypatch.setattr(B, "_lib", lib)
    monkeypatch.setattr(hip, "_raw_stream", raw_stream)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: current[0])
    monkeypatch.setattr(torch.cuda, "set_device", set_device)
    return lib, events


def test_call_marshals_by_the_table(stub):
    lib, _ = stub
    d = B.FgsNcaDims(2, 100, 16, 8)
    state, delta, step, new = (torch.zeros(4) for _ in range(4))
    assert hip.call(torch.device("cuda", 0), "fgs_nca_update_forward", d, state, delta, step, None, 0.25, new) is None
    (name, args), = lib.calls
    assert name == "fgs_nca_update_forward" and len(args) == len(B.SIGNATURES[name][1]) == 8
    assert args[0]._obj is d and (args[0]._obj.batch, args[0]._obj.points, args[0]._obj.state_dim, args[0]._obj.k) == (2, 100, 16, 8)
    assert list(args[1:4]) == [t.data_ptr() for t in (state, delta, step)]   # a tensor arrives as its data_ptr()
    assert args[4] is None                                       # None arrives as NULL
    assert args[5] == 0.25 and type(args[5]) is float            # scalars as they are
    assert args[6] == new.data_ptr()
    assert args[7] == STREAM                                     # the stream handle, last
    # integer scalars between pointers, two structures
    sd, sp, t = B.FgsSurfaceDims(1, 8, 8), B.FgsSurfaceParams(), torch.zeros(4)
    hip.call(torch.device("cuda", 0), "fgs_surface_emit", sd, sp, t, None, t, t, t, t, t, t, t, 1 << 40)
    args = lib.calls[-1][1]
    assert args[0]._obj is sd and args[1]._obj is sp and args[3] is None and args[-2] == 1 << 40 and args[-1] == STREAM
    # a symbol whose table entry does not end in `stream` gets none
    L = B.FgsSavedLayout()
    hip.call(torch.device("cuda", 0), "fgs_saved_layout", B.make_dims(1, 10, 16, 16), L)
    args = lib.calls[-1][1]
    assert len(args) == 2 and args[1]._obj is L
    assert sorted(n for n, (_, p) in B.SIGNATURES.items() if not p or p[-1][0] != "stream") == sorted(
        n for n in B.SIGNATURES if n.endswith("_bytes") or n in ("fgs_saved_layout", "fgs_last_error", "fgs_version",
                                                               "fgs_stage_timing_enable", "fgs_stage_timing_read"))
    with pytest.raises(TypeError, match="fgs_saved_layout takes 2 arguments, got 3"):
        hip.call(torch.device("cuda", 0), "fgs_saved_layout", B.make_dims(1, 10, 16, 16), L, None)
    with pytest.raises(TypeError, match="fgs_count_pairs takes 3 arguments and the stream, got 4"):
        hip.call(torch.device("cuda", 0), "fgs_count_pairs", B.make_dims(1, 10, 16, 16), t, t, t)


def test_a_failing_call_raises_with_the_symbol_and_the_library_message(stub):
    lib, _ = stub
    lib.rc = -1
    with pytest.raises(B.FgsError, match=r"fgs_count_pairs failed \(rc=-1\): stub: no such luck"):
        hip.call(torch.device("cuda", 0), "fgs_count_pairs", B.make_dims(1, 10, 16, 16), torch.zeros(1), torch.zeros(1))
    with pytest.raises(B.FgsError, match=r"fgs_head_workspace_bytes failed \(rc=-1\): stub: no such luck"):
        B.sizes("fgs_head_workspace_bytes", B.FgsHeadDims())


def test_sizes_returns_what_the_table_says(stub):
    lib, _ = stub
    d = B.make_dims(1, 10, 16, 16)
    assert B.sizes("fgs_workspace_bytes", d) == (4096, 512) == B.workspace_bytes(d)
    assert lib.calls[-1][1][0]._obj is d and len(lib.calls[-1][1]) == 3
    one = B.sizes("fgs_head_workspace_bytes", B.FgsHeadDims())
    assert one == 4096 and type(one) is int
    assert B.sizes("fgs_asm_propagate_workspace_bytes", 48, 40, 3) == 4096
    assert lib.calls[-1][1][:3] == (48, 40, 3) and len(lib.calls[-1][1]) == 4
    sd, sp = B.FgsSurfaceDims(1, 8, 8), B.FgsSurfaceParams()
    assert B.sizes("fgs_surface_guided_backward_bytes", sd, sp, 5, 7) == 4096
    args = lib.calls[-1][1]
    assert args[0]._obj is sd and args[1]._obj is sp and args[2:4] == (5, 7) and len(args) == 5


def _launch(dev):
    hip.call(dev, "fgs_count_pairs", B.make_dims(1, 10, 16, 16), torch.zeros(1), torch.zeros(1))


def test_call_switches_to_the_tensors_device_and_back(stub):
    lib, events = stub
    _launch(torch.device("cuda", 1))
    assert events == [("set", 1), ("stream", 1), ("set", 0)]     # switched before the stream is read, restored after
    assert lib.calls[-1][1][-1] == STREAM + 1
    del events[:]
    lib.rc = -2
    with pytest.raises(B.FgsError):
        _launch(torch.device("cuda", 1))
    assert events == [("set", 1), ("stream", 1), ("set", 0)]     # restored also when the call fails
    del events[:]
    lib.rc = 0
    _launch(torch.device("cuda", 0))
    _launch(torch.device("cuda"))                                # no index: the current device
    assert events == [("stream", 0), ("stream", 0)]              # no set_device at all


def test_a_held_device_guard_is_entered_once(stub):
    """The rasterizer's per-image route allocates under the guard and hands the guard itself to `call`."""
    lib, events = stub
    with hip.on_device(torch.device("cuda", 1)) as held:
        assert events == [("set", 1)]
        hip.call(held, "fgs_count_pairs", B.make_dims(1, 10, 16, 16), torch.zeros(1), torch.zeros(1))
        assert events == [("set", 1), ("stream", 1)]
    assert events == [("set", 1), ("stream", 1), ("set", 0)]


def test_stream_handle_of_a_named_device_switches_nothing(stub):
    """The scratch cache's key (renderer._scratch_for): the stream of the tensors' device, whichever device is current."""
    _, events = stub
    assert hip.stream_handle(torch.device("cuda", 1)) == STREAM + 1 and hip.stream_handle(torch.device("cuda")) == STREAM
    assert hip.stream_handle() == STREAM and events == [("stream", 1), ("stream", 0), ("stream", 0)]


def test_small_helpers():
    assert hip.ptr(None) is None and hip.f32c(None) is None
    t = torch.zeros(3)
    assert hip.ptr(t) == t.data_ptr() and hip.f32c(t) is t
    from fresnel_amd import decoder, renderer
    assert renderer._f32c is hip.f32c and decoder._f32c is hip.f32c
    with pytest.raises(B.FgsError, match="^ssim needs CUDA/ROCm tensors; there is no CPU fallback$"):
        hip.need_cuda(t, "ssim")
