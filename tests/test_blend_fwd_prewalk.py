"""The pre-walk of the exiting depth-split forward (tuning key fwd_prewalk = the FGS_FWD_PREWALK_ON / _OFF flag of
FgsDims.fwd_variant; k_blend_fwd_head and k_blend_fwd_parts<.., REST>, fgs_composite.hip).

A SHORT list has 2 <= nseg <= NP segments (NP list parts): one segment per part, the head reaches segment 0, and parts 1 .. nseg - 1
start from T = 1 and need nothing of part 0.  With the pre-walk on, extra blocks of the HEAD launch walk them -- one block per (tile,
part), one wave per 16 x 16 half -- and store the local result into the hand-over slot k_blend_fwd_parts uses (slot part + 1, slot 0
for the last part); the REST launch then only composes: its waves of parts > 0 neither walk nor store.  A pre-walk block cannot know
whether the head closes its half, so it also writes those slots behind a closing slot k = 1, where nobody reads them.  No output
bit and no word of saved.fwd_open / saved.fwd_close may change, so what can go wrong is the BOOKKEEPING: a part stored into the
wrong slot, a slot written twice or not at all, a part of a longer list (spp > 1) walked by nobody, a tile order slot or part
lost where the tile count is no multiple of 8.

Scenes: small Gaussians inside ONE 16 x 16 cell each (the first half of the four 32 x 16 tiles of a 2 x 2 grid; on 40 x 24 three of
them are partial), so that a tile's list length is the number put there plus the whole-frame / half-plane groups of 24 saturating
entries in front (the groups of tests/test_blend_bwd_dead_units.py).  Lengths are functions of (seg_len S, parts NP):

  ladderA   S - 1, S + 1, (NP - 1) S - 1, NP S + 1 entries: 1, 2, NP - 1 and NP + 1 segments (NP + 1: spp == 2, NOT pre-walked; fewer
            segments than parts: last < NP - 1).  Green is exactly 0 everywhere: nothing closes, every list ends open in every half.
  ladderB   NP S - 1, 0, NP S, 2 S + 1: NP segments with a last one of S - 1 and of S entries, an EMPTY tile between occupied ones.
  c64       a whole-frame group in front: every half with >= 64 entries closes at chunk 64 of segment 0, its later parts are
            pre-walked for nothing; one list shorter than a chunk; one of NP + 1 segments.
  c128      the open last column of tile column 0 is shut by a second group at list positions 104 .. 127: those halves close at
            128 -- inside the head's reach with S = 128 (k = 1), behind it with S = 64 (left open, composed by the rest launch).
  col       32 x 16 tiles: half 0 closes at 64, half 1 stays open through its last pixel column and its list ends open -- a closed half
            beside an open one in ONE pre-walked tile.  (16 x 16: the one half stays open.)
  nan       ladderA with a NaN colour in an entry of part 1 of the (NP - 1)-segment list.
  batch     c64 and its never-closing twin (green 0) in one call against the single calls; overflow: the capacity overflow under
            tests/workspace_guard.py's three fills.
Every scene's lengths are asserted on the oracle's lists, and its closing pattern on the fp32 emulation of
tests/test_blend_fwd_absorbed.py with its margins, on the CPU, before the GPU runs.

GPU, per case, with fwd_prewalk = 1 (automatic leaves it off), fwd_exit = 1, bwd_zero = 1 and the part count forced: image, depth and the five gradients bitwise equal to the
fwd_prewalk = -1 call, to the fwd_exit = -1 call and to a second run; fwd_open and fwd_close word for word those of the fwd_prewalk = -1
call (and of the model); the referee against the oracle; outputs and words identical under the guard's three fills and unguarded.

(The rest launch composes through LDS, part by part; the fwd_exit = -1 call composes through the checkpoint slots, as every forward did
before: the bitwise statement against it covers that hand-over too -- the A plane of a stored absolute state is ONE fma there.)

CPU half: the slot model of tests/test_blend_fwd_close_slot.py extended by WHO writes -- head blocks, pre-walk blocks, the rest
launch -- and by the rest launch's own reads.  Every slot the rest launch or a backward unit reads holds the full walk's state, that
state was written exactly once, and no slot is written by head and pre-walk blocks of the same launch (they run concurrently).  Two
wrong rules are each told apart by a scene: a pre-walk that stores part p into slot p (spp = 1: slot part * spp), and a rest launch
that still walks.  A list of two segments cannot tell the first apart (its one later part is the last and goes to slot 0 either way)
and a scene that closes everywhere cannot tell the second (the rest launch's waves of a closed half touch nothing): both stated.
"""
import functools

import numpy as np
import pytest
import torch

import test_blend_bwd_dead_units as D
import test_blend_fwd_absorbed as A
import test_blend_fwd_close_slot as S
from helpers import assert_with_referee

GRADS = D.GRADS
NONE = S.NONE
N_FRONT = 24
ORIGINS = [(0, 0), (32, 0), (0, 16), (32, 16)]  # the four 32 x 16 tiles; the crowd of each sits in its first 16 x 16 half
KINDS = ["ladderA", "ladderB", "c64", "c128", "col", "nan"]


def _name(kind, seg_len, parts, zero=False):
    return f"pw:{kind}:{seg_len}:{parts}" + (":zero" if zero else "")


def _spec(name):
    _, kind, seg_len, parts = name.split(":")[:4]
    Sg, NP = int(seg_len), int(parts)
    few = max((NP - 1) * Sg - 1, 7)  # (one part: no such list, a short one instead)
    lens = {"ladderA": [Sg - 1, Sg + 1, few, NP * Sg + 1], "nan": [Sg - 1, Sg + 1, few, NP * Sg + 1],
            "ladderB": [NP * Sg - 1, 0, NP * Sg, 2 * Sg + 1],
            "c64": [NP * Sg, 2 * Sg - 1, 40, (NP + 1) * Sg],
            "c128": [NP * Sg, max(3 * Sg - 1, 129), 2 * Sg + 1, NP * Sg + 1],
            "col": [NP * Sg - 1, (NP - 1) * Sg + 1, 2 * Sg, NP * Sg + 1]}[kind]
    return kind, Sg, NP, lens


def _groups(kind, tile_w):
    """(front groups, mid group): half-planes of the frame as in D._groups; the mid group stands at list positions 104 .. 127 of the
    tiles of column 0 (80 .. 103 elsewhere)"""
    if kind == "c64":
        return [("x", "hi", 0)], None
    if kind == "c128":
        return [("x", "lo", tile_w - 1)], ("x", "hi", tile_w - 1)
    if kind == "col":
        return [("x", "lo", tile_w - 1)], None
    return [], None


def _touches(g, X0, cw):
    """does the half-plane group reach the tile [X0, X0 + cw)"""
    return X0 < g[2] if g[1] == "lo" else X0 + cw > g[2]


def _tile_of(X0, Y0, W, tile_w):
    return (Y0 // 16) * -(-W // tile_w) + X0 // tile_w


@functools.lru_cache(maxsize=None)
def _build(name, W, H, tile_w):
    """Flat Gaussians turned about the viewing axis, item 0 frontmost (the construction of D._scene).  Array order = depth order:
    front groups | up to 80 crowd entries per tile | mid group | the rest of the crowds | anchors (frontmost in depth)."""
    kind, Sg, NP, lens = _spec(name)
    rs = np.random.RandomState(7100 + W + tile_w + Sg + NP)
    front, mid = _groups(kind, tile_w)
    u, v, r = [], [], []

    def group(g):
        gu, gv = D._group_mean(g, W, H)
        for _ in range(N_FRONT):
            u.append(gu + rs.uniform(-0.2, 0.2)); v.append(gv + rs.uniform(-0.2, 0.2)); r.append(3 * D.SIGMA)

    for g in front:
        group(g)
    crowds = []
    for (X0, Y0), n in zip(ORIGINS, lens):
        cw, ch = min(16, W - X0), min(16, H - Y0)
        tw = min(tile_w, W - X0)
        n -= N_FRONT * sum(_touches(g, X0, tw) for g in front + ([mid] if mid else []))
        n -= D.N_ANCHOR if (X0, Y0) == ORIGINS[3] else 0  # the anchors (below) are the first entries of the fourth tile's list
        assert n >= 0 and cw >= 6 and ch >= 6
        crowds.append([(X0 + rs.uniform(2.5, cw - 2.5), Y0 + rs.uniform(2.5, ch - 2.5), rs.uniform(1.0, 1.8)) for _ in range(n)])
    pre = 80 if mid else 0
    for c in crowds:
        for (cu, cv, cr) in c[:pre]:
            u.append(cu); v.append(cv); r.append(cr)
    if mid:
        group(mid)
    for c in crowds:
        for (cu, cv, cr) in c[pre:]:
            u.append(cu); v.append(cv); r.append(cr)
    n_list = len(u)
    for _ in range(D.N_ANCHOR):  # ANCHORS (D._scene): a few ordinary Gaussians in front of everything, so that every tensor has gradients
        # of ordinary size; every pixel of the frame lies in a 32 x 16 tile with a crowd, so they stand in the fourth crowd's cell
        u.append(36.0 + rs.uniform(-0.5, 0.5)); v.append(20.0 + rs.uniform(-0.5, 0.5)); r.append(rs.uniform(2.0, 2.5))
    u, v, r = np.asarray(u), np.asarray(v), np.asarray(r)
    N = len(u)
    th = rs.uniform(0.0, np.pi, N)
    minor = np.where(r > 100, 1.0, 0.6)
    color = (0.2 + 0.7 * rs.random_sample((N, 3))).astype(np.float32)
    if kind in ("ladderA", "ladderB", "nan") or name.endswith(":zero"):
        color[:, 1] = 0.0  # C_g == 0 absorbs nothing under the strict test: nothing closes
    gI = rs.standard_normal((3, H, W)).astype(np.float32)
    gD = (rs.standard_normal((H, W)) * 0.1).astype(np.float32) + 0.05
    opacity = np.full(N, 0.8, np.float32)
    z = -2.0 - 0.001 * np.arange(N)
    z[n_list:] = -1.9 - 0.004 * np.arange(D.N_ANCHOR)
    s = r / 3.0 * -z / D.FOCAL
    pos = np.stack([(u - W / 2) * -z / D.FOCAL, -(v - H / 2) * -z / D.FOCAL, z], 1).astype(np.float32)
    scale = np.stack([s, minor * s, 1e-3 * s], 1).astype(np.float32)
    quat = np.stack([np.cos(th / 2), 0 * th, 0 * th, np.sin(th / 2)], 1).astype(np.float32)
    if kind == "nan":  # list position S + 10 of the (NP - 1)-segment list: an entry of part 1 (no group stands in front in this scene)
        assert NP >= 3
        first = sum(len(c) for c in crowds[:2])
        color[first + Sg + 10, 0] = np.nan
    return [pos, scale, quat, color, opacity], gI, gD


# A's emulation and reference look their scenes up by name through A._scene: the names of this file ("pw:...") are added in front of
# it, every other name goes where it went
_a_scene = A._scene


def _scene(name, W, H, tile_w):
    return _build(name, W, H, tile_w) if name.startswith("pw:") else _a_scene(name, W, H, tile_w)


A._scene = _scene


@functools.lru_cache(maxsize=None)
def check_scene(name, W, H, tile_w):
    """the lists are what the scene says, the closing pattern holds with margin; -> ({(tile, half): closing | None}, {tile: entries})"""
    kind, Sg, NP, want = _spec(name)
    em = A._emulate(name, W, H, tile_w)
    lens = em["lens"]
    for (X0, Y0), n in zip(ORIGINS, want):
        assert lens[_tile_of(X0, Y0, W, tile_w)] == n, (name, W, H, tile_w, X0, Y0, lens, n)
    closes = {}
    for key, bl in em["bounds"].items():
        pos, cls = A._closing(bl)
        assert pos is None or cls == "closed", (name, key, pos, cls)
        closes[key] = pos
    assert not em["moved"]["stated"]
    halves = tile_w // 16
    col0 = [_tile_of(X0, Y0, W, tile_w) for (X0, Y0) in ORIGINS if X0 == 0]
    tiles_x = -(-W // tile_w)
    inframe = lambda t, h: (t % tiles_x) * tile_w + 16 * h < W  # noqa: E731  (a half with no pixel in the frame closes at once: nobody vetoes)
    assert all(p == 64 for (t, h), p in closes.items() if not inframe(t, h))
    if kind in ("ladderA", "ladderB", "nan") or name.endswith(":zero"):
        assert all(p is None for (t, h), p in closes.items() if inframe(t, h))
    elif kind == "c64":
        assert all(p == 64 for p in closes.values())
    elif kind == "c128":
        assert all(closes[(t, halves - 1)] == 128 for t in col0)
    elif kind == "col":
        assert all(closes[(t, halves - 1)] is None for t in col0) and (halves == 1 or all(closes[(t, 0)] == 64 for t in col0))
    return closes, lens


# ---- the model: who writes which slot, who reads it ------------------------------------------------------------------------------
def _half(n, pos, seg_len, parts, prewalk=True, store="stated", rest_walks=False):
    """One half of a tile: n list entries, closing at `pos` (None: never).  States: ('abs', j) the absolute state in front of segment
    j, ('end', p) the local result of part p (walked from T = 1), ('local', j) a later part's inner slot, 'resume' what the head
    leaves an open half, 'closing'.  -> (problems, final {slot: state}, word, open mark)"""
    nseg, spp, hlen = S._geometry(n, seg_len, parts)
    closed = pos is not None and pos <= hlen
    last = (nseg - 1) // spp if nseg else 0
    short = prewalk and parts > 1 and 2 <= nseg <= parts
    problems, slots, count, by = [], {}, {}, {}

    def write(who, j, st):
        if who in ("head", "prewalk") and by.get(j, who) in ("head", "prewalk") and by.get(j, who) != who:
            problems.append(("race", j, by[j], who))  # blocks of ONE launch: no order between them
        assert 0 <= j < max(nseg, 1), (who, j, nseg)
        slots[j], by[j] = st, who
        count[st] = count.get(st, 0) + 1

    def read(who, j, st):
        if slots.get(j) != st:
            problems.append(("read", who, j, st, slots.get(j)))
        elif count[st] != 1:
            problems.append(("written twice", who, j, st))

    handover = lambda p: 0 if p == last else (p + 1) * spp  # noqa: E731  (k_blend_fwd_parts)
    # the head launch: head blocks ...
    stop = pos if closed else hlen
    for j in range(1, nseg):
        if j * seg_len < stop:
            write("head", j, ("abs", j))
    word, is_open = NONE, False
    if closed:
        k = -(-pos // seg_len)
        if k < nseg:
            write("head", k, "closing")
            word = k
    elif hlen < n:
        is_open = True
        write("head", hlen // seg_len, "resume")
    # ... and pre-walk blocks, which know neither `closed` nor `is_open`
    if short:
        for p in range(1, nseg):
            write("prewalk", (p * spp if p != last else 0) if store == "part" else handover(p), ("end", p))
    # the rest launch: an open half only
    if is_open and parts > 1 and nseg > spp:
        hs = hlen // seg_len
        read("rest", hs, "resume")
        write("rest", hs, ("abs", hs))  # the A plane put right in place
        for j in range(hs + 1, spp):
            write("rest", j, ("abs", j))
        for p in range(1, last + 1):
            if not short or rest_walks:
                for j in range(p * spp + 1, min((p + 1) * spp, nseg)):
                    write("rest", j, ("local", j))
                write("rest", handover(p), ("end", p))
        write("rest", spp, ("abs", spp))
        for p in range(1, last + 1):
            read("rest", handover(p), ("end", p))
            if p != last:
                write("rest", (p + 1) * spp, ("abs", (p + 1) * spp))
    elif is_open:  # one part in fact: part 0 walks on
        for j in range(hlen // seg_len, nseg):
            slots[j] = ("abs", j)
    # the backward's units
    for seg in range(1, nseg):
        reads, st = S._backward(seg, slots, word, spp, parts)
        if any(rd not in slots for rd in reads):
            problems.append(("unwritten", seg, reads))
        elif st != S._truth(seg, word):
            problems.append(("changed", seg, st))
    return problems, slots, word, is_open


def _walk(name, W, H, tile_w, **rule):
    """-> (problems of every half, {(tile, half): (word, open mark)}, facts seen)"""
    kind, Sg, NP, _ = _spec(name)
    closes, lens = check_scene(name, W, H, tile_w)
    problems, words, seen = [], {}, set()
    for t, n in lens.items():
        nseg, spp, hlen = S._geometry(n, Sg, NP)
        marks = []
        for h in range(tile_w // 16):
            pr, slots, word, is_open = _half(n, closes.get((t, h)), Sg, NP, **rule)
            problems += [(t, h) + p for p in pr]
            words[(t, h)] = (word, is_open)
            marks.append("closed" if word != NONE else ("open" if is_open else "ended"))
            if 2 <= nseg <= NP:
                seen.add(("short", marks[-1], nseg))
                if word != NONE:
                    seen.add(("closes at", closes[(t, h)]))
            elif nseg > NP:
                seen.add(("long", marks[-1]))
        if len(marks) == 2 and 2 <= nseg <= NP and set(marks) == {"closed", "open"}:
            seen.add("closed beside open")
        if n == 0:
            seen.add("empty")
    return problems, words, seen


# (kind, W, H, tile_w, seg_len, parts): four parts is the benchmark's split; every other part count the plan takes at that size once
CASES = [
    ("ladderA", 64, 32, 32, 128, 4), ("ladderA", 40, 24, 16, 64, 4), ("ladderA", 40, 24, 32, 64, 4), ("ladderA", 64, 32, 16, 128, 4),
    ("ladderB", 64, 32, 32, 64, 4), ("ladderB", 40, 24, 16, 128, 4), ("ladderB", 40, 24, 32, 128, 4),
    ("c64", 64, 32, 32, 128, 4), ("c64", 40, 24, 16, 64, 4), ("c64", 64, 32, 16, 64, 4), ("c64", 40, 24, 32, 128, 4),
    ("c128", 64, 32, 32, 128, 4), ("c128", 40, 24, 16, 128, 4), ("c128", 64, 32, 32, 64, 4),
    ("col", 64, 32, 32, 64, 4), ("col", 40, 24, 32, 128, 4), ("col", 64, 32, 16, 128, 4),
    ("nan", 64, 32, 32, 64, 4), ("nan", 40, 24, 16, 128, 4),
    ("ladderA", 64, 32, 32, 64, 2), ("ladderA", 64, 32, 32, 64, 8), ("ladderA", 64, 32, 16, 64, 16), ("ladderA", 40, 24, 16, 64, 1),
    ("c64", 64, 32, 32, 128, 2), ("c64", 40, 24, 16, 64, 8),
]


def _id(c):
    return f"{c[0]}-{c[1]}x{c[2]}-tw{c[3]}-s{c[4]}v{c[5]}"


def _args(case):
    kind, W, H, tile_w, Sg, NP = case
    return _name(kind, Sg, NP), W, H, tile_w


# ---- CPU half --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_cpu_every_slot_read_was_written_once(case):
    problems, _, _ = _walk(*_args(case))
    assert not problems, problems[:4]
    assert not _walk(*_args(case), prewalk=False)[0]  # the parent's split, under the same model


def test_cpu_cases_cover_the_seams():
    seen = set()
    for case in CASES:
        if case[5] == 4:
            seen |= _walk(*_args(case))[2]
    want = {("short", "open", 2), ("short", "open", 3), ("short", "open", 4), ("short", "closed", 2), ("short", "closed", 4),
            ("long", "open"), ("long", "closed"), ("closes at", 64), ("closes at", 128), "closed beside open", "empty"}
    assert seen >= want, want - seen
    assert {c[5] for c in CASES} == {1, 2, 4, 8, 16} and {c[3] for c in CASES} == {16, 32} and {c[4] for c in CASES} == {64, 128}
    assert {(c[1], c[2]) for c in CASES} == {(64, 32), (40, 24)}


def test_cpu_wrong_rules_are_told_apart():
    """storing part p into slot p: the head's slot 1 is raced for and the rest launch finds slot p + 1 empty; a rest launch that
    still walks writes every hand-over state a second time"""
    open_case, closing_case = _args(("ladderA", 64, 32, 32, 128, 4)), _args(("c64", 64, 32, 32, 128, 4))
    pr = _walk(*open_case, store="part")[0]
    assert any(p[2] == "race" for p in pr) and any(p[2] == "read" for p in pr), pr[:4]
    pr = _walk(*open_case, rest_walks=True)[0]
    assert pr and all(p[2] == "written twice" for p in pr), pr[:4]
    # a closed half's pre-walk under the wrong store rule races for the closing slot itself
    assert any(p[2] == "race" for p in _walk(*closing_case, store="part")[0])
    # what CANNOT be told apart: two segments (the one later part is the last: slot 0 either way) ...
    for n in (65, 128, 129, 256):
        for seg_len in (64, 128):
            if 2 == -(-n // seg_len):
                assert _half(n, None, seg_len, 4, store="part")[:2] == _half(n, None, seg_len, 4)[:2]
    # ... and a rest launch that still walks, on a scene that closes everywhere (its waves of a closed half touch nothing)
    assert not _walk(*closing_case, rest_walks=True)[0]


def test_cpu_prewalk_never_touches_the_slots_a_closed_half_keeps():
    """k = 1 for every closing of a short list (the head's reach is one segment); the pre-walk writes slots 2 .. and slot 0"""
    for seg_len in (64, 128):
        for parts in (2, 4, 8, 16):
            for nseg in range(2, parts + 1):
                for n in ((nseg - 1) * seg_len + 1, nseg * seg_len):
                    for pos in range(64, seg_len + 1, 64):
                        problems, slots, word, is_open = _half(n, pos, seg_len, parts)
                        assert not problems and word == 1 and not is_open and slots[1] == "closing"
                        assert {j for j, st in slots.items() if st != "closing" and st[0] == "end"} == ({0} | set(range(2, nseg))) - {nseg}


def test_cpu_the_switch():
    """fwd_prewalk = 0 | 1 | -1 -> the flags of FgsDims.fwd_variant; both at once are refused; the layout does not depend on it"""
    from fresnel_amd import _binding as B
    kw = dict(batch=2, num_gaussians=100, width=64, height=32)
    assert B.make_dims(**kw, tuning=dict(fwd_prewalk=-1, fwd_variant=4, fwd_exit=1)).fwd_variant == 4 | B.FWD_EXIT_ON | B.FWD_PREWALK_OFF
    assert B.make_dims(**kw, tuning=dict(fwd_prewalk=1)).fwd_variant == B.FWD_PREWALK_ON and B.make_dims(**kw).fwd_variant == 0
    assert (B.FWD_PREWALK_OFF, B.FWD_PREWALK_ON) == (0x40000, 0x80000)  # (0x1000 and 0x20000 stay unknown bits: older tests say so)
    assert not (B.FWD_PREWALK_OFF | B.FWD_PREWALK_ON) & (B.FWD_EXIT_OFF | B.FWD_EXIT_ON | B.BWD_ZERO_OFF | B.BWD_ZERO_ON | B.BWD_TAIL_OFF | B.BWD_TAIL_ON
                                                         | B.BWD_SUB_OFF | B.BWD_SUB_ON | 0x1F)
    for bad in (dict(fwd_prewalk=2), dict(fwd_prewalk=-2), dict(fwd_prewalk=1, fwd_variant=-2)):
        with pytest.raises(B.FgsError):
            B.make_dims(**kw, tuning=bad)
    both = B.make_dims(**kw)
    both.fwd_variant = B.FWD_PREWALK_ON | B.FWD_PREWALK_OFF
    with pytest.raises(B.FgsError):
        B.workspace_bytes(both)
    # ignored where the exiting forward is off or there is one part; no section moves with it anywhere
    for tun in (dict(fwd_exit=1, fwd_variant=4), dict(fwd_exit=-1, fwd_variant=4), dict(fwd_exit=1, fwd_variant=1), dict()):
        sizes = {B.workspace_bytes(B.make_dims(**kw, tuning=dict(tun, fwd_prewalk=f))) for f in (0, 1, -1)}
        assert len(sizes) == 1, (tun, sizes)
        L = [B.saved_layout(B.make_dims(**kw, tuning=dict(tun, fwd_prewalk=f))) for f in (0, -1)]
        assert (L[0].fwd_open, L[0].fwd_close, L[0].total_bytes) == (L[1].fwd_open, L[1].fwd_close, L[1].total_bytes)
    assert B.workspace_bytes(B.make_dims(8, 32768, 512, 512)) == B.workspace_bytes(B.make_dims(8, 32768, 512, 512, tuning=dict(fwd_prewalk=-1)))


# ---- GPU half --------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def _tuning(tile_w, Sg, NP, **kw):
    return dict(dict(tile_w=tile_w, seg_len=Sg, fwd_variant=NP, fwd_exit=1, bwd_zero=1, fwd_prewalk=1), **kw)  # (automatic leaves the pre-walk off)


def _words(arrs, W, H, tuning):
    """saved.fwd_open / fwd_close of one forward (a batch of one)"""
    from fresnel_amd.renderer import Camera, TileBasedRenderer, inspect_saved
    dev = D._cuda()
    ts = [torch.from_numpy(np.ascontiguousarray(a[None])).to(dev).requires_grad_(True) for a in arrs]
    ren = TileBasedRenderer(W, H, background=D.BG)
    ren.tuning = dict(tuning)
    img = ren(*ts, Camera(D.FOCAL, D.FOCAL, W / 2, H / 2, W, H), return_depth=True)[0]
    st = inspect_saved(img.grad_fn.saved_tensors[-1], img.grad_fn.dims)
    halves = tuning["tile_w"] // 16
    return st["fwd_open"][0, :, :halves].cpu().numpy().astype(np.int64), st["fwd_close"][0].cpu().numpy().astype(np.int64)


@gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_case_same_bits_same_words_under_the_fills(case):
    kind, W, H, tile_w, Sg, NP = case
    name = _name(kind, Sg, NP)
    _, words, _ = _walk(name, W, H, tile_w)
    arrs, gI, gD = _build(name, W, H, tile_w)
    halves = tile_w // 16
    got = S._guarded(arrs, gI, gD, W, H, _tuning(tile_w, Sg, NP))  # three fills and unguarded: outputs and words identical
    off_open, off_close = _words(arrs, W, H, _tuning(tile_w, Sg, NP, fwd_prewalk=-1))
    assert (got["fwd_open"][0].astype(np.int64) == off_open).all() and (got["fwd_close"][0].astype(np.int64) == off_close).all(), _id(case)
    for (t, h), (word, is_open) in words.items():
        assert off_close[t, h] == (-1 if word == NONE else word) and off_open[t, h] == int(is_open), (_id(case), t, h, word, is_open)
    assert (off_close[:, halves:] == -1).all()
    for what, kw in (("fwd_prewalk=-1", dict(fwd_prewalk=-1)), ("fwd_exit=-1", dict(fwd_exit=-1)), ("second run", dict())):
        tun = dict(_tuning(tile_w, Sg, NP), **kw)
        A._same_bits(got, D._hip(arrs, W, H, gI, gD, tun), f"{_id(case)} against {what}:")
    if kind == "nan":  # (as in A: the image's clamp turns a NaN into 0, the gradients take NaNs of their own -- the statement is the
        return                                             # bitwise one above, NaN payloads included)
    r32, g32, r64, g64 = A._reference(name, W, H, tile_w)
    assert_with_referee(got["image"], r32.image, r64.image, f"{_id(case)} image")
    assert_with_referee(got["depth"], r32.depth, r64.depth, f"{_id(case)} depth")
    for k in GRADS:
        assert_with_referee(got[k], g32[k], g64[k], f"{_id(case)} grad_{k}")


@gpu
@pytest.mark.parametrize("tile_w,Sg", [(32, 128), (16, 64), (32, 64)])
def test_batch_of_all_closing_and_never_closing(tile_w, Sg):
    """c64 (every half closes: every pre-walk is for nothing) and its twin with green 0 (nothing closes: every pre-walk is composed)
    in ONE call -- two images, so the tile count of the launch is twice a single call's: outputs and words bit-equal to the single calls"""
    W, H, NP = 64, 32, 4
    names = (_name("c64", Sg, NP), _name("c64", Sg, NP, zero=True))
    assert all(v == 64 for v in check_scene(names[0], W, H, tile_w)[0].values())
    assert all(v is None for v in check_scene(names[1], W, H, tile_w)[0].values())
    a, gI, gD = _build(names[0], W, H, tile_w)
    b = _build(names[1], W, H, tile_w)[0]
    tuning = _tuning(tile_w, Sg, NP)
    both = S._guarded([np.stack([x, y]) for x, y in zip(a, b)], np.stack([gI, gI]), np.stack([gD, gD]), W, H, tuning)
    for i, arrs in enumerate((a, b)):
        single = D._hip(arrs, W, H, gI, gD, tuning)
        for k in GRADS + ["image", "depth"]:
            assert both[k][i].tobytes() == single[k].tobytes(), (tile_w, Sg, i, k)
        s_open, s_close = _words(arrs, W, H, tuning)
        assert (both["fwd_open"][i].astype(np.int64) == s_open).all() and (both["fwd_close"][i].astype(np.int64) == s_close).all()
    assert (both["fwd_close"][0, :, :tile_w // 16] == 1).any() and (both["fwd_close"][1] == -1).all() and both["fwd_open"][1].any()


@gpu
@pytest.mark.parametrize("tuning", [dict(tile_w=32, seg_len=64, fwd_variant=4, fwd_exit=1, bwd_zero=1, fwd_prewalk=1),
                                    dict(tile_w=16, seg_len=128, fwd_variant=4, fwd_exit=1, bwd_zero=1, fwd_prewalk=1)], ids=["tw32-seg64", "tw16-seg128"])
def test_capacity_overflow_under_the_guard_fills(tuning):
    """every list empty: the pre-walk blocks leave behind their scalar loads, every word is written, no output depends on a fill"""
    import test_workspace_capacity as C
    import workspace_guard as WG
    Dn = C._oracle_duplicates("aniso", tuning["tile_w"])
    inp = C._inputs()
    inputs = {k: inp[k] for k in GRADS + ["gI", "gD"]}
    call = S._Call(inputs, C.W, C.H, C._camera(), C.BG, tuning, workspace=Dn // 4)
    runs = WG.run_patterns(call, inputs, C._mods())
    assert int(call.counters[1]) == 1  # overflowed
    for name, out in runs.items():
        assert bool((out["fwd_close"] == -1).all()) and not bool(out["fwd_open"].any()), name
        for k in ("image", "depth"):
            assert bool((out[k].view(torch.int32) == C.QNAN).all()), (name, k)
        for k in [g for g in out if g.startswith("grad_")]:
            assert not bool(out[k].view(torch.int32).any()), (name, k)
