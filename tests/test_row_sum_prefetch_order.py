"""k_row_sum (fgs_project.hip) decides all of a lane's rows before it loads any: the ORDER of its additions is the contract.

The kernel sums a Gaussian's gradient rows with four lanes (lane `sub` takes rows sub, sub + 4, ...; moments in float64, colour and
depth sums in float32, all from +0; the lanes' totals combined pairwise) and leaves out row k of a Gaussian of depth rank r where
r >= zero_from[tile of row k] (the blend backward's tail verdict).  A Gaussian that looks rows up (rank >= the image's smallest
word) first loads the table words of ALL its lane's rows and keeps the answers as a bit mask -- at most 32 rows per lane; the host
derives the largest rectangle from k_project's radius clamp and keeps the old loop where it could be larger -- then loads and adds
the written rows in ascending k.  The sums must be the bits of the loop that decided and loaded two rows at a time, which is the
numpy model below; what can go wrong is a mask bit off by one (a lane's first or last row), a row added twice or out of order (float64
and float32 additions do not commute in their bits), and a lookup for a Gaussian that must not look anything up.

fgs_row_sum (include/fgs.h) runs the stage alone on a hand-made `saved` buffer: rectangles of 1, 3, 4, 5, 8, 9 and the maximum number
of rows (9 x 9 tiles of 16 x 16, 5 x 9 of 32 x 16 at max_radius 64: 21 / 12 rows per lane), one image per (rectangle, pattern); the
patterns leave out every lane's first row, its last, alternating rows of a lane (both phases), all rows and none.  Every image also
holds a Gaussian of a rank below the image's smallest word (it looks nothing up), one behind the designed one (more rows left
out) and one elsewhere.  The same buffers without a table give the full sums.  A frame whose rectangles can exceed 128 rows
(max_radius 200 on 12 x 12 tiles) keeps the old loop, with rectangles on both sides of the mask's width."""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
f32 = np.float32
NONE = 0xFFFFFFFF
R_OP, R_BBX, R_BBY = 5, 10, 11
RECTS = {16: [(1, 1), (3, 1), (2, 2), (5, 1), (4, 2), (3, 3), (9, 9)], 32: [(1, 1), (3, 1), (2, 2), (5, 1), (4, 2), (3, 3), (5, 9)]}
PATTERNS = ["first", "last", "alt0", "alt1", "all", "none"]
N = 4       # per image: [0] rank 0, below the smallest word; [1] the designed one, rank 1; [2] rank 2, behind it; [3] rank 3, elsewhere
RANK = 1    # depth rank of the designed Gaussian


def _left_out(pattern, k, cnt):
    lane_rows = len(range(k % 4, cnt, 4))
    i = k // 4
    return {"first": i == 0, "last": i == lane_rows - 1, "alt0": i % 2 == 0, "alt1": i % 2 == 1, "all": True, "none": False}[pattern]


def model(rows, written, opacity):
    """k_row_sum for one Gaussian: rows [cnt, 10] float32, written [cnt] bool -> the ten totals (float32)"""
    lanes = []
    for sub in range(4):
        m, c = np.zeros(6, np.float64), np.zeros(4, f32)
        for k in range(sub, len(rows), 4):
            if written[k]:
                m = m + rows[k, :6].astype(np.float64)
                c = (c + rows[k, 6:]).astype(f32)
        hp = np.float64(0.69314718055994530942)
        K = np.float64(-0.72134752044448170368)
        acc = np.array([hp * m[0], hp * m[1], K * hp * m[2], K * hp * m[3], K * hp * m[4], m[5] * (np.float64(1.0) / np.float64(opacity))]).astype(f32)
        lanes.append(np.concatenate([acc, (c * f32(0.99)).astype(f32)]))
    return ((lanes[0] + lanes[1]).astype(f32) + (lanes[2] + lanes[3]).astype(f32)).astype(f32)


def _build(tile_w, W, H, max_radius, cases):
    """cases: [(cols, rows, pattern)] -> one image each.  Returns what the call needs and what the model needs."""
    from fresnel_amd import _binding as B
    Bn = len(cases)
    dims = B.make_dims(Bn, N, W, H, max_radius=max_radius, tuning=dict(tile_w=tile_w))
    L = B.saved_layout(dims)
    tiles_x, tiles_y = int(L.tiles_x), int(L.tiles_y)
    assert int(L.tile_w) == tile_w and tiles_x == -(-W // tile_w) and tiles_y == -(-H // 16)
    T = tiles_x * tiles_y
    rs = np.random.RandomState(77 + tile_w + Bn)
    rec = np.zeros((Bn, N, 12), f32)
    order = np.zeros((Bn, N), np.int32)
    dup_off, cnts = np.zeros((Bn, N), np.uint32), np.zeros((Bn, N), np.uint32)
    table = np.full((Bn, T), NONE, np.uint64)
    rects = np.zeros((Bn, N, 4), np.int64)  # tx0, ty0, cols, rows
    ranks = [0, RANK, RANK + 1, RANK + 2]
    total = 0
    for b, (cols, rows_, pattern) in enumerate(cases):
        tx0, ty0 = (tiles_x - cols) // 2, (tiles_y - rows_) // 2
        rects[b] = [(tx0, ty0, cols, rows_),                       # rank 0: the same tiles, every row written, nothing looked up
                    (tx0, ty0, cols, rows_),                       # the designed one
                    (tx0, max(ty0 - 1, 0), min(cols + 1, tiles_x - tx0), min(rows_ + 1, tiles_y - max(ty0 - 1, 0))),  # behind it, larger
                    (0, 0, 2, 1)]                                  # elsewhere (but for the largest rectangles): looks up, every row written
        for i in range(N):
            order[b, ranks[i]] = i
            x0, y0, c_, r_ = rects[b, i]
            rec[b, i, R_OP] = 0.8
            rec[b, i, R_BBX] = np.array([x0 * tile_w | min((x0 + c_) * tile_w, W) << 16], np.uint32).view(f32)[0]
            rec[b, i, R_BBY] = np.array([y0 * 16 | min((y0 + r_) * 16, H) << 16], np.uint32).view(f32)[0]
            cnts[b, i], dup_off[b, i] = c_ * r_, total
            total += int(c_ * r_)
        cnt = cols * rows_
        for k in range(cnt):
            t = (ty0 + k // cols) * tiles_x + tx0 + k % cols
            table[b, t] = RANK if _left_out(pattern, k, cnt) else RANK + 1
    assert total <= int(L.dup_capacity)
    rows = rs.standard_normal((total, 10)).astype(f32) * (10.0 ** rs.uniform(-6, 6, (total, 1))).astype(f32)
    rows[rs.random_sample(total) < 0.1] = f32(-0.0)  # whole rows of -0 (what a zero unit may have written), and single zeros
    rows[rs.random_sample((total, 10)) < 0.05] = f32(0.0)
    return dict(dims=dims, L=L, T=T, tiles_x=tiles_x, rec=rec, order=order, dup_off=dup_off, cnts=cnts, table=table, rects=rects,
                ranks=ranks, rows=rows)


def _expected(s, with_table):
    Bn = s["rec"].shape[0]
    want = np.zeros((Bn, N, 12), f32)
    kinds = set()
    for b in range(Bn):
        smallest = int(s["table"][b].min())
        for i in range(N):
            x0, y0, c_, _ = s["rects"][b, i]
            cnt, off, rank = int(s["cnts"][b, i]), int(s["dup_off"][b, i]), s["ranks"][i]
            tiles = [(y0 + k // c_) * s["tiles_x"] + x0 + k % c_ for k in range(cnt)]
            written = np.array([not with_table or rank < s["table"][b, t] for t in tiles])
            if with_table:
                kinds.add("below" if rank < smallest else ("all" if not written.any() else ("none" if written.all() else "some")))
            want[b, i, :10] = model(s["rows"][off:off + cnt], written, f32(0.8))
    return want, kinds


def _call(s, with_table):
    from fresnel_amd import _binding as B
    from fresnel_amd import _hip as hip
    dev = torch.device("cuda:0")
    L, Bn = s["L"], s["rec"].shape[0]
    saved = torch.zeros(B.workspace_bytes(s["dims"])[0], dtype=torch.uint8, device=dev)

    def put(off, arr):
        raw = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).to(dev)
        saved[off:off + raw.numel()] = raw
    put(L.rec, s["rec"]); put(L.order, s["order"]); put(L.dup_off, s["dup_off"]); put(L.tile_count, s["cnts"])
    rows = torch.from_numpy(s["rows"]).to(dev)
    words = np.concatenate([s["table"].reshape(-1), s["table"].min(axis=1)]).astype(np.uint32)
    table = torch.from_numpy(words.view(np.int32)).to(dev) if with_table else None
    out = torch.full((Bn * N, 12), float("nan"), device=dev)
    hip.call(dev, "fgs_row_sum", s["dims"], saved, rows, table, out)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(Bn, N, 12)


@gpu
@pytest.mark.parametrize("tile_w", [16, 32])
def test_sums_are_the_model_bit_for_bit(tile_w):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    cases = [(c, r, p) for (c, r) in RECTS[tile_w] for p in PATTERNS]
    assert sorted({c * r for c, r in RECTS[tile_w]}) == [1, 3, 4, 5, 8, 9, 81 if tile_w == 16 else 45]
    s = _build(tile_w, 160, 160, 64.0, cases)
    for with_table in (True, False):
        want, kinds = _expected(s, with_table)
        got = _call(s, with_table)
        bad = [(b, i, cases[b]) for b in range(len(cases)) for i in range(N) if got[b, i].tobytes() != want[b, i].tobytes()]
        assert not bad, (tile_w, with_table, bad[:8], got[bad[0][0], bad[0][1]], want[bad[0][0], bad[0][1]])
        if with_table:
            assert kinds == {"below", "all", "none", "some"}, kinds
    # the table matters: leaving rows out changes sums
    assert _expected(s, True)[0].tobytes() != _expected(s, False)[0].tobytes()


@gpu
def test_rectangles_beyond_the_mask_keep_the_loop():
    """max_radius 200 on a 192 x 192 frame: a rectangle can hold 12 x 12 = 144 rows, 36 per lane -- more than the mask's 32 bits --
    so the launch keeps the old loop for every Gaussian; 11 x 11 = 121 rows would fit a mask and 144 would not, both are summed right"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    cases = [(12, 12, p) for p in ("alt0", "first", "last")] + [(11, 11, p) for p in ("alt1", "last")]
    s = _build(16, 192, 192, 200.0, cases)
    for with_table in (True, False):
        want, _ = _expected(s, with_table)
        got = _call(s, with_table)
        assert got.tobytes() == want.tobytes(), with_table


def test_cpu_patterns_leave_out_what_they_name():
    """first / last / alternating are statements about a LANE's rows sub, sub + 4, ...; every lane with rows is hit"""
    for cnt in (1, 3, 4, 5, 8, 9, 45, 81):
        for sub in range(min(4, cnt)):
            mine = list(range(sub, cnt, 4))
            assert [_left_out("first", k, cnt) for k in mine] == [True] + [False] * (len(mine) - 1)
            assert [_left_out("last", k, cnt) for k in mine] == [False] * (len(mine) - 1) + [True]
            assert [_left_out("alt0", k, cnt) for k in mine] == [i % 2 == 0 for i in range(len(mine))]
            assert [_left_out("alt1", k, cnt) for k in mine] == [i % 2 == 1 for i in range(len(mine))]
    assert max(len(range(sub, 81, 4)) for sub in range(4)) == 21  # the most rows a lane can have at max_radius 64


def test_cpu_model_order_matters():
    """the model tells a changed order apart: the same rows added in descending k give other bits"""
    rs = np.random.RandomState(3)
    rows = (rs.standard_normal((45, 10)) * 10.0 ** rs.uniform(-6, 6, (45, 1))).astype(f32)
    w = np.ones(45, bool)
    assert model(rows, w, f32(0.8)).tobytes() != model(rows[::-1], w, f32(0.8)).tobytes()
    z = rows.copy(); z[4] = f32(-0.0)
    w2 = w.copy(); w2[4] = False
    assert model(z, w, f32(0.8)).tobytes() == model(z, w2, f32(0.8)).tobytes()  # a -0 row left out: the same bits
