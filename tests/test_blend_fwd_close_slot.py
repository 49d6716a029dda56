"""The closing slot of the exiting depth-split forward (saved.fwd_close; k_blend_fwd_head and k_composite_bwd, fgs_composite.hip).

A 16 x 16 tile half that the head kernel closes after `done` list entries stores its closing state (C, A = 1, D) into ONE checkpoint
slot, k = ceil(done / seg_len) -- the first slot its walk did not reach -- and leaves k in fwd_close[tile][half]; the half's cells of
every later slot are never written.  The backward restarts every unit of that half with segment >= k from slot k, taken as an
absolute state.  The word is 0xFFFFFFFF (-1 as int32) for a half left open, a list that ended, a closing inside the last segment
(k is then no slot of the tile) and index 1 on 16 x 16 tiles.  No output bit may change, so what can go wrong is the BOOKKEEPING: a
word that names the wrong slot, a unit that reads a slot nobody wrote, a half that reads the other half's word.

Scenes, emulation and helpers are those of tests/test_blend_fwd_absorbed.py (A) and tests/test_blend_bwd_dead_units.py (D), imported.
CASES picks, per scene, the frames, tile shapes, segment lengths (64, 128) and work splits (fwd_variant 1, 2, 4) at which the
bookkeeping takes another path; fwd_exit = 1 throughout:

  mid     closing at chunk 64 with segments of 128: k = 1, slot 1 is written in the middle of segment 0
  spp     k == segments per part: the closing slot is the first slot of part 1
  last    closing inside the last segment: no later slot, the word is none
  h0 / h1 a 32 x 16 tile with half 0 closed and half 1 open, and the reverse
  ended   a list that ends inside the head's reach without closing
  behind  a half that closes behind the head's reach: left open, the rest kernel writes every slot
  edge    the frame's last tile, partial on 40 x 24

Every scene's closing pattern is asserted on the CPU from A's fp32 emulation, with its margins (A.check_scene), before the GPU runs.

GPU half: the words against ceil(closing position / seg_len) of the emulation, all kinds seen; image, depth and the five gradients
against the C oracle under the referee, bitwise equal to the same call with fwd_exit = -1, and every call under
tests/workspace_guard.py's three fills (0xFFFFFFFF, a quiet NaN, among them) and once unguarded, outputs and words identical across
the four runs -- a read of a slot that is no longer written shows there; the capacity overflow under the guard (every list empty:
every word is WRITTEN, none); a batch of an image that closes everywhere and one that never closes against the single calls.

CPU half: a model of which slots the forward writes per half and which slot each (unit, half) of the backward reads.  On every case
every slot read was written and carries the state of a full walk.  Two wrong rules are each told apart by a case -- re-basing the
closing slot (reads the unwritten first slot of a later part) and one word for both halves (a changed state, or an unwritten slot).
The third rule the design names, `seg > k` instead of `seg >= k`, CANNOT be told apart by any scene, and the model shows why
(test_cpu_seg_gt_k_is_the_same_rule): k <= segments per part, so slot k is a slot of part 0 or a part's first slot, and the unit of
segment k reads slot k, without re-basing, under either rule.
"""
import numpy as np
import pytest
import torch

import test_blend_bwd_dead_units as D
import test_blend_fwd_absorbed as A
from helpers import assert_with_referee

GRADS = D.GRADS
NONE = 0xFFFFFFFF
TUNINGS = {f"s{s}v{v}": dict(seg_len=s, fwd_variant=v) for s in (64, 128) for v in (1, 2, 4)}
# (scene, W, H, tile_w, tuning)
CASES = [
    ("dead", 64, 32, 32, "s128v2"), ("dead", 40, 24, 16, "s128v1"), ("dead", 64, 32, 16, "s64v4"), ("dead", 40, 24, 32, "s64v2"),
    ("dead", 64, 32, 32, "s128v4"),
    ("seam@127", 64, 32, 32, "s64v2"), ("seam@127", 40, 24, 16, "s64v2"), ("seam@63", 64, 32, 16, "s64v4"),
    ("seamin@128", 64, 32, 32, "s128v1"), ("seamin@128", 40, 24, 16, "s64v1"), ("seamin@128", 64, 32, 16, "s64v2"),
    ("col", 64, 32, 32, "s64v2"), ("col", 40, 24, 32, "s128v1"),
    ("sub@0", 64, 32, 32, "s64v4"), ("sub@0", 40, 24, 32, "s64v1"),
    ("zero", 64, 32, 32, "s64v2"), ("short", 64, 32, 32, "s64v2"),
    ("edge", 40, 24, 32, "s64v2"), ("edge", 40, 24, 16, "s128v2"), ("edge", 64, 32, 32, "s64v1"),
]
KINDS = {"mid", "spp", "last", "h0", "h1", "ended", "behind", "edge"}


def _id(c):
    return f"{c[0]}-{c[1]}x{c[2]}-tw{c[3]}-{c[4]}"


# ---- the model -------------------------------------------------------------------------------------------------------------------
def _geometry(n, seg_len, parts):
    """segments, segments per part, the head's reach in entries (k_blend_fwd_head)"""
    nseg = -(-n // seg_len)
    spp = -(-nseg // parts)
    hs = nseg if parts == 1 else min(spp, max(1, A.HEAD_ENTRIES // seg_len))
    return nseg, spp, min(n, hs * seg_len)


def _forward(n, pos, seg_len, parts):
    """One half of a tile with n list entries that closes at `pos` (None: never).  -> ({slot: state}, word): the slots the forward
    WRITES in that half's cells with the state they hold -- ('abs', j) the absolute state in front of segment j, ('local', j) the
    part-local one, 'closing' -- and the half's fwd_close word."""
    nseg, spp, hlen = _geometry(n, seg_len, parts)
    closed = pos is not None and pos <= hlen
    stop = pos if closed else hlen
    slots = {j: ("abs", j) for j in range(1, nseg) if j * seg_len < stop}  # part 0's slots, stored on the walk
    if closed:
        k = -(-pos // seg_len)
        if k >= nseg:
            return slots, NONE
        assert k not in slots and 1 <= k <= spp
        slots[k] = "closing"
        return slots, k
    if hlen < n:  # left open: the rest kernel walks on and writes every other slot
        for j in range(1, nseg):
            slots.setdefault(j, ("abs", j) if (j < spp or j % spp == 0) else ("local", j))
    return slots, NONE


def _compose(a, b):
    """the re-basing compose(a, b) on model states; None = an unwritten slot was read"""
    if a is None or b is None:
        return None
    if a == "closing":  # T' = 1 - 1.0f = +0 absorbs whatever follows
        return "closing"
    if a[0] == "abs" and b[0] == "local":
        return ("abs", b[1])
    return ("changed", a, b)


def _backward(seg, slots, word, spp, parts, rule="stated"):
    """the state unit `seg` (>= 1) restarts one half from: (slots read, state)"""
    behind = seg > word if rule == "gt" else seg >= word
    own = word if behind else seg
    reads, st = [own], slots.get(own)
    if parts > 1 and seg >= spp and seg % spp and (not behind or rule == "rebase"):
        first = seg // spp * spp
        reads.append(first)
        st = _compose(slots.get(first), st)
    return reads, st


def _truth(seg, word):
    """what a full walk's slots give: behind a closing the closing state, else the absolute state in front of the segment"""
    return "closing" if seg >= word else ("abs", seg)


def _walk_case(case, rule="stated", one_word=False):
    """-> (unwritten reads, changed states, kinds) of a case under a rule of the backward"""
    name, W, H, tile_w, tun = case
    seg_len, parts = TUNINGS[tun]["seg_len"], TUNINGS[tun]["fwd_variant"]
    closes = A.check_scene(name, W, H, tile_w)
    lens = A._emulate(name, W, H, tile_w)["lens"]
    unwritten, changed, kinds = [], [], set()
    halves = tile_w // 16
    last_tile = max(lens)
    for t, n in lens.items():
        nseg, spp, hlen = _geometry(n, seg_len, parts)
        fw = [_forward(n, closes.get((t, h)), seg_len, parts) for h in range(halves)]
        for h in range(halves):
            slots, word = fw[h]
            pos = closes.get((t, h))
            if word != NONE:
                kinds.add("mid" if pos % seg_len else "full")
                if word == spp and parts > 1:
                    kinds.add("spp")
                if t == last_tile and name == "edge" and (W % tile_w or H % 16):  # the frame's last tile, partial
                    kinds.add("edge")
            elif pos is not None and pos <= hlen:
                kinds.add("last")
            elif hlen == n and n >= 64:
                kinds.add("ended")
            elif pos is not None:
                kinds.add("behind")
            other = closes.get((t, 1 - h)) if halves == 2 else 0
            if halves == 2 and word != NONE and hlen < n and (other is None or other > hlen):  # this half closed, the other left open
                kinds.add("h0" if h == 0 else "h1")
            used = fw[0][1] if one_word else word
            for seg in range(1, nseg):
                reads, st = _backward(seg, slots, used, spp, parts, rule)
                if any(r not in slots for r in reads):
                    unwritten.append((t, h, seg, reads))
                elif st != _truth(seg, word):
                    changed.append((t, h, seg, st))
    return unwritten, changed, kinds


def _expected_words(case):
    """int32 [tiles, 2] of a case, from the emulation's closing positions"""
    name, W, H, tile_w, tun = case
    seg_len, parts = TUNINGS[tun]["seg_len"], TUNINGS[tun]["fwd_variant"]
    closes = A.check_scene(name, W, H, tile_w)
    lens = A._emulate(name, W, H, tile_w)["lens"]
    want = np.full((len(lens), 2), -1, np.int64)
    for t, n in lens.items():
        for h in range(tile_w // 16):
            word = _forward(n, closes.get((t, h)), seg_len, parts)[1]
            want[t, h] = -1 if word == NONE else word
    return want


# ---- CPU half --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_cpu_every_slot_read_was_written(case):
    unwritten, changed, _ = _walk_case(case)
    assert not unwritten and not changed, (unwritten[:3], changed[:3])


def test_cpu_cases_cover_every_kind():
    kinds = set()
    for case in CASES:
        kinds |= _walk_case(case)[2]
    assert kinds >= KINDS, KINDS - kinds
    assert {TUNINGS[c[4]]["fwd_variant"] for c in CASES} == {1, 2, 4} and {c[3] for c in CASES} == {16, 32}
    assert {(c[1], c[2]) for c in CASES} == {(64, 32), (40, 24)}


def test_cpu_wrong_rules_are_told_apart():
    """re-basing the closing slot reads a later part's first slot, which a closed half no longer writes; one word for both halves
    sends an open half to the other half's closing slot (a changed state) or a closed half to its own unwritten slots"""
    for rule, kw in (("rebase", dict(rule="rebase")), ("one word", dict(one_word=True))):
        caught = [c for c in CASES if any(_walk_case(c, **kw)[:2])]
        assert caught, rule
    assert any(_walk_case(("dead", 40, 24, 32, "s64v2"), rule="rebase")[0])   # k = 1 < spp = 2: segment 3 would re-base with slot 2
    assert any(_walk_case(("col", 64, 32, 32, "s64v2"), one_word=True)[1])    # half 1 is open and would restart from half 0's slot 1
    assert any(_walk_case(("sub@0", 64, 32, 32, "s64v4"), one_word=True)[0])  # half 1 is closed and would read its unwritten slots


def test_cpu_seg_gt_k_is_the_same_rule():
    """`seg > k` differs from `seg >= k` at the unit of segment k alone, and that unit reads slot k either way: k <= segments per
    part, so slot k is never re-based.  No scene can tell the two apart -- stated here instead of a scene that pretends to."""
    for case in CASES:
        assert _walk_case(case, rule="gt")[:2] == ([], [])
    for n in (65, 129, 200, 500, 2000):
        for seg_len in (64, 128):
            for parts in (1, 2, 4):
                nseg, spp, hlen = _geometry(n, seg_len, parts)
                for pos in range(64, hlen + 1, 64):
                    slots, word = _forward(n, pos, seg_len, parts)
                    if word != NONE:
                        assert word <= spp and _backward(word, slots, word, spp, parts, "gt") == _backward(word, slots, word, spp, parts)


# ---- GPU half --------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


class _Call:
    """one forward / backward on persistent device inputs, for workspace_guard.run_patterns: the seven outputs and the two tables"""

    def __init__(self, inputs, W, H, camera, bg, tuning, workspace="worst"):
        self.inputs, self.W, self.H, self.camera, self.bg, self.tuning, self.workspace = inputs, W, H, camera, bg, tuning, workspace
        self.counters = None

    def __call__(self, guard):
        import test_workspace_capacity as C
        from fresnel_amd.renderer import TileBasedRenderer, inspect_saved
        inp = self.inputs
        ts = [C._leaf(inp[k]) for k in GRADS]
        ren = TileBasedRenderer(self.W, self.H, background=self.bg, workspace=self.workspace)
        ren.tuning = dict(self.tuning)
        img, dep = ren(*ts, self.camera, return_depth=True)
        node = img.grad_fn
        C._sync_check(guard, "after the forward")
        st = inspect_saved(node.saved_tensors[-1], node.dims)
        halves = self.tuning["tile_w"] // 16
        out = dict(image=img.detach(), depth=dep.detach(), fwd_close=st["fwd_close"].clone(),
                   fwd_open=st["fwd_open"][..., :halves].clone())  # (fwd_open's index 1 is written on 32 x 16 tiles only)
        self.counters = st["counters"].clone()
        ((img * inp["gI"]).sum() + (dep * inp["gD"]).sum()).backward()
        C._sync_check(guard, "after the backward")
        for k, t in zip(GRADS, ts):
            out["grad_" + k] = t.grad
        return out


def _guarded(arrs, gI, gD, W, H, tuning):
    """the call under the three fills and once unguarded (outputs asserted identical by run_patterns) -> numpy outputs"""
    import test_workspace_capacity as C
    import workspace_guard as WG
    from fresnel_amd.renderer import Camera
    dev = D._cuda()
    single = arrs[0].ndim == 2  # one image: as a batch of one (the autograd node of the call is then the renderer's own)
    host = [a[None] if single else a for a in list(arrs) + [gI, gD]]
    inputs = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in zip(GRADS + ["gI", "gD"], host)}
    call = _Call(inputs, W, H, Camera(D.FOCAL, D.FOCAL, W / 2, H / 2, W, H), D.BG, tuning)
    runs = WG.run_patterns(call, inputs, C._mods())
    assert set(runs) == {"zero", "one", "ff", "unpatched"}
    out = {k.replace("grad_", ""): v.cpu().numpy() for k, v in runs["ff"].items()}
    if single:
        out = {k: (v if k.startswith("fwd_") else v[0]) for k, v in out.items()}
    return out


@gpu
def test_words_match_the_cpu_pattern():
    """saved.fwd_close of every case against the emulation (forward only), and every kind of word was seen on the GPU"""
    from fresnel_amd.renderer import Camera, TileBasedRenderer, inspect_saved
    dev = D._cuda()
    seen = set()
    for case in CASES:
        name, W, H, tile_w, tun = case
        want = _expected_words(case)
        kinds = _walk_case(case)[2]
        ts = [torch.from_numpy(np.ascontiguousarray(a[None])).to(dev).requires_grad_(True) for a in A._scene(name, W, H, tile_w)[0]]
        ren = TileBasedRenderer(W, H, background=D.BG)
        ren.tuning = dict(tile_w=tile_w, fwd_exit=1, **TUNINGS[tun])
        img = ren(*ts, Camera(D.FOCAL, D.FOCAL, W / 2, H / 2, W, H), return_depth=True)[0]
        st = inspect_saved(img.grad_fn.saved_tensors[-1], img.grad_fn.dims)
        got = st["fwd_close"][0].cpu().numpy().astype(np.int64)
        assert got.shape == want.shape and (got == want).all(), (_id(case), got.tolist(), want.tolist())
        marks = st["fwd_open"][0].cpu().numpy()
        assert not (marks[:, :tile_w // 16][got[:, :tile_w // 16] >= 0]).any(), _id(case)  # a half with a closing slot is not open
        seen |= kinds
    assert seen >= KINDS, KINDS - seen


@gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_case_under_the_fills_vs_oracle_and_exit_off(case):
    name, W, H, tile_w, tun = case
    A.check_scene(name, W, H, tile_w)
    arrs, gI, gD = A._scene(name, W, H, tile_w)
    tuning = dict(tile_w=tile_w, fwd_exit=1, **TUNINGS[tun])
    got = _guarded(arrs, gI, gD, W, H, tuning)
    want = _expected_words(case)
    assert (got["fwd_close"][0].astype(np.int64) == want).all(), _id(case)
    A._same_bits(got, A._hip(name, W, H, tile_w, TUNINGS[tun], fwd_exit=-1), _id(case) + " against fwd_exit=-1:")
    A._same_bits(got, A._hip(name, W, H, tile_w, TUNINGS[tun]), _id(case) + " second run:")
    r32, g32, r64, g64 = A._reference(name, W, H, tile_w)
    assert_with_referee(got["image"], r32.image, r64.image, f"{_id(case)} image")
    assert_with_referee(got["depth"], r32.depth, r64.depth, f"{_id(case)} depth")
    for k in GRADS:
        assert_with_referee(got[k], g32[k], g64[k], f"{_id(case)} grad_{k}")


@gpu
@pytest.mark.parametrize("tile_w,tun", [(32, "s64v2"), (16, "s128v2"), (32, "s128v1")])
def test_batch_of_all_closing_and_never_closing(tile_w, tun):
    """`dead` (every half closes) and `zero` (nothing closes) in ONE call: words and outputs bit-equal to the single calls"""
    W, H = 64, 32
    assert all(v == 64 for v in A.check_scene("dead", W, H, tile_w).values())
    assert all(v is None for v in A.check_scene("zero", W, H, tile_w).values())
    a, gI, gD = A._scene("dead", W, H, tile_w)
    b = A._scene("zero", W, H, tile_w)[0]
    tuning = dict(tile_w=tile_w, fwd_exit=1, **TUNINGS[tun])
    both = _guarded([np.stack([x, y]) for x, y in zip(a, b)], np.stack([gI, gI]), np.stack([gD, gD]), W, H, tuning)
    for i, name in enumerate(("dead", "zero")):
        single = A._hip(name, W, H, tile_w, TUNINGS[tun])
        for k in GRADS + ["image", "depth"]:
            assert both[k][i].tobytes() == single[k].tobytes(), (tun, name, k)
        assert (both["fwd_close"][i].astype(np.int64) == _expected_words((name, W, H, tile_w, tun))).all(), (tun, name)
    assert (both["fwd_close"][0, :, :tile_w // 16] >= 1).any() and (both["fwd_close"][1] == -1).all()


@gpu
@pytest.mark.parametrize("tuning", [dict(tile_w=32, seg_len=64, fwd_exit=1), dict(tile_w=16, seg_len=128, fwd_variant=1, fwd_exit=1)],
                         ids=["tw32-seg64", "tw16-seg128-v1"])
def test_capacity_overflow_under_the_guard_fills(tuning):
    """every list empty: the head kernel still writes EVERY word of the table (none: no half has a closing slot), whatever the fill
    was, and no output depends on a fill"""
    import test_workspace_capacity as C
    import workspace_guard as WG
    Dn = C._oracle_duplicates("aniso", tuning["tile_w"])
    inp = C._inputs()
    inputs = {k: inp[k] for k in GRADS + ["gI", "gD"]}
    call = _Call(inputs, C.W, C.H, C._camera(), C.BG, tuning, workspace=Dn // 4)
    runs = WG.run_patterns(call, inputs, C._mods())
    assert int(call.counters[1]) == 1  # overflowed
    for name, out in runs.items():
        assert bool((out["fwd_close"] == -1).all()) and not bool(out["fwd_open"].any()), name
        for k in ("image", "depth"):
            assert bool((out[k].view(torch.int32) == C.QNAN).all()), (name, k)
        for k in [g for g in out if g.startswith("grad_")]:
            assert not bool(out[k].view(torch.int32).any()), (name, k)
