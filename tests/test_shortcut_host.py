"""No-GPU checks of the line of sight and of string pulling: the restatement (tests/shortcut_ref.py) against closed
forms, a boundary walk, fp64 sampling and the block rule of route_ref; the greedy rule on descended and hand-made
paths; the host side of gaussiangrasper_amd.transit and the two C entries' argument validation (nothing is
launched)."""
import ctypes
import itertools
import math
import types

import numpy as np
import pytest
import torch

import route_ref
import shortcut_ref as ref

FAR = route_ref.FAR
NEED, OPEN, SHUT = ref.NEED, ref.OPEN, ref.SHUT


def _set(cells):
    return {tuple(int(v) for v in c) for c in np.asarray(cells).reshape(-1, 3)}


def _pairs(rng, count, reach):
    a = rng.integers(0, reach, size=(count, 3))
    return a, a + rng.integers(-reach, reach + 1, size=(count, 3))


# ------------------------------------------------------------------------------------------------
# the cover
# ------------------------------------------------------------------------------------------------
def test_cover_of_a_move_is_the_block_of_the_block_rule():
    c = np.array([5, 6, 7])
    for m, dx, dy, dz in route_ref.MOVES:
        block = {(c[0] + ex, c[1] + ey, c[2] + ez) for ex in {0, dx} for ey in {0, dy} for ez in {0, dz}}
        assert _set(ref.cover(c, c + [dx, dy, dz])) == block and len(block) == 2 ** (abs(dx) + abs(dy) + abs(dz))
    assert _set(ref.cover(c, c)) == {tuple(c)}


def test_cover_is_symmetric_and_the_walk_agrees_with_the_slabs():
    rng = np.random.default_rng(0)
    a, b = _pairs(rng, 300, 9)                         # short segments: many ties
    a2, b2 = _pairs(rng, 100, 40)
    for p, q in zip(np.concatenate([a, a2]), np.concatenate([b, b2])):
        slab = ref.cover(p, q)
        assert np.array_equal(slab, ref.cover(q, p))
        assert np.array_equal(slab, ref.cover_walk(p, q)) and np.array_equal(slab, ref.cover_walk(q, p))


def _ties(n):
    """(crossings that two axes share, crossings that all three share) of a direction n >= 0, by enumeration in
    exact fractions: axis x crosses at (2 k + 1) / (2 n_x)"""
    from fractions import Fraction
    seen = {}
    for x in range(3):
        for k in range(n[x]):
            seen.setdefault(Fraction(2 * k + 1, 2 * n[x]), []).append(x)
    return sum(1 for v in seen.values() if len(v) == 2), sum(1 for v in seen.values() if len(v) == 3)


def test_cover_closed_forms():
    o = np.array([3, 4, 5])
    for n in (1, 2, 5, 12):
        for s in itertools.product((-1, 1), repeat=3):
            s = np.array(s)
            for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
                e = np.eye(3, dtype=np.int64)[list(perm)]
                assert len(ref.cover(o, o + n * s * e[0])) == n + 1
                assert len(ref.cover(o, o + n * s * (e[0] + e[1]))) == 3 * n + 1
            assert len(ref.cover(o, o + n * s)) == 7 * n + 1
    # No ties at all: two crossings (2 k + 1) / (2 n_a) and (2 k' + 1) / (2 n_b) are equal iff (2 k + 1) n_b ==
    # (2 k' + 1) n_a, which needs n_a and n_b to hold the same power of two.  Components with pairwise different
    # powers of two therefore cross one face at a time: 1 + n_x + n_y + n_z cells.
    for n in ((1, 2, 4), (3, 2, 4), (5, 6, 4), (7, 0, 2), (9, 4, 0), (1, 0, 0), (3, 10, 8)):
        assert _ties(n) == (0, 0)
        for perm in itertools.permutations(range(3)):
            for s in itertools.product((-1, 1), repeat=3):
                d = np.array(n)[list(perm)] * s
                assert len(ref.cover(o, o + d)) == 1 + sum(n), (n, perm, s)
    # Pairwise coprime ODD components always tie once, at t = 1/2 (k = (n_a - 1) / 2 on each axis): the corner in
    # the middle of the segment.  A tie of two axes opens 3 cells for its 2 crossings and a tie of three 7 for 3, so
    # the cover has 1 + n_x + n_y + n_z + (ties of two) + 4 (ties of three) cells.
    for n in ((3, 5, 0), (1, 3, 0), (7, 9, 0)):
        assert _ties(n) == (1, 0) and len(ref.cover(o, o + n)) == 1 + sum(n) + 1
    for n in ((3, 5, 7), (1, 3, 5), (5, 7, 9)):
        assert _ties(n) == (0, 1) and len(ref.cover(o, o + n)) == 1 + sum(n) + 4
    rng = np.random.default_rng(1)
    for n in rng.integers(0, 14, size=(60, 3)):
        two, three = _ties([int(v) for v in n])
        assert len(ref.cover(o, o - n)) == 1 + int(n.sum()) + two + 4 * three


def _box_distance(p, c):
    """fp64 distance from points p (N, 3) to the closed cube [c, c + 1]^3"""
    return np.linalg.norm(np.maximum(np.maximum(c - p, p - (c + 1.0)), 0.0), axis=1)


def test_cover_against_dense_sampling_in_fp64():
    rng = np.random.default_rng(2)
    a, b = _pairs(rng, 60, 12)
    for p, q in zip(a, b):
        cov = ref.cover(p, q)
        have = _set(cov)
        n = np.abs(q - p)
        # parameters strictly between consecutive crossings (and the two ends): no sample sits on a boundary
        cross = sorted({(2 * k + 1) / (2.0 * n[x]) for x in range(3) for k in range(n[x])})
        knots = np.array([0.0] + cross + [1.0])
        t = np.unique(np.concatenate([knots[:-1] + f * np.diff(knots) for f in (0.25, 0.5, 0.75)] + [[0.0, 1.0]]))
        pts = (p + 0.5)[None] + t[:, None] * (q - p)[None]
        assert _set(np.floor(pts)) <= have, (p, q)
        # and no cell too many: every cell of the cover is within 1e-9 cells of the segment (a float box-segment
        # distance: the smallest over the samples and the crossings themselves)
        dense = (p + 0.5)[None] + np.concatenate([t, knots])[:, None] * (q - p)[None]
        for c in cov:
            assert _box_distance(dense, c.astype(np.float64)).min() <= 1e-9, (p, q, c)
        # a cell of the box that is NOT in the cover is away from every sample
        box = ref.box_cells(np.minimum(p, q), np.maximum(p, q))
        for c in box:
            if tuple(c) not in have:
                assert _box_distance(dense, c.astype(np.float64)).min() > 0.0


def test_sight_counts_and_outside_ends():
    d = np.full((7, 6, 5), OPEN, np.int32)
    d[3, 3, 2] = d[1, 1, 1] = SHUT
    a = [(0, 0, 0), (0, 0, 0), (6, 5, 4), (2, 2, 2), (-1, 0, 0), (0, 0, 0), (3, 3, 2)]
    b = [(6, 0, 0), (2, 2, 2), (0, 0, 0), (2, 2, 2), (3, 3, 3), (0, 6, 0), (3, 3, 2)]
    cover, blocked = ref.sight(d, NEED, a, b)
    assert cover.tolist() == [7, 15, len(ref.cover(a[2], b[2])), 1, 0, 0, 1]
    assert blocked.tolist()[:2] == [0, 1] and blocked.tolist()[3:] == [0, -1, -1, 1]
    assert blocked[2] == sum(1 for c in ref.cover(a[2], b[2]) if d[tuple(c)] < NEED)
    _, _, cov, blk = ref.sight_all_pairs(d, NEED)
    one, two = ref.sight(d, NEED, *np.array([[(0, 0, 0), (6, 5, 4)], [(6, 5, 4), (1, 0, 2)]]).transpose(1, 0, 2))
    cells = ref.box_cells((0, 0, 0), (6, 5, 4))
    at = lambda c: int(np.nonzero((cells == c).all(1))[0][0])
    n = len(cells)
    assert (cov[at((0, 0, 0)) * n + at((6, 5, 4))], blk[at((0, 0, 0)) * n + at((6, 5, 4))]) == (one[0], two[0])
    assert (cov[at((6, 5, 4)) * n + at((1, 0, 2))], blk[at((6, 5, 4)) * n + at((1, 0, 2))]) == (one[1], two[1])


# ------------------------------------------------------------------------------------------------
# the greedy rule
# ------------------------------------------------------------------------------------------------
def _descended(d, goal, starts, room=128):
    cost, _ = route_ref.route(d, NEED, [goal])
    return route_ref.descend(d, NEED, cost, starts, room)


def test_greedy_on_descended_paths_of_the_wall_and_door_volume():
    d = ref.wall_and_door()
    starts = [(2, 3, 40), (5, 30, 4), (1, 17, 21), (35, 2, 2), (19, 17, 21)]
    d[38, 30, 40] = OPEN
    for s in starts:
        d[s] = OPEN
    cells, length = _descended(d, (38, 30, 40), starts)
    assert (length > 1).all() and length.max() <= 128 and length[:3].min() >= 18
    keep, count, blocked = ref.shortcut(d, NEED, cells, length, 128)
    free = ref.free_cells(d, NEED)
    assert all(np.array_equal(x, y) for x, y in zip(ref.shortcut_by_walk(d, NEED, cells, length, 128),
                                                    (keep, count, blocked)))
    for p in range(len(starts)):
        n, k = int(length[p]), int(count[p])
        rows = keep[p, :k]
        assert rows[0] == 0 and rows[-1] == n - 1 and (np.diff(rows) > 0).all() and (keep[p, k:] == n - 1).all()
        assert blocked[p] == 0
        for i, j in zip(rows[:-1], rows[1:]):              # every kept segment is clear, by the walk
            assert all(free[tuple(c)] for c in ref.cover_walk(cells[p, i], cells[p, j]))
        assert ref.kept_length(cells[p], keep[p], k) <= ref.polyline_length(cells[p, :n]) + 1e-12
        # window 1 is the path itself
        k1, c1, b1 = ref.shortcut(d, NEED, cells[p:p + 1], length[p:p + 1], 1)
        assert c1[0] == n and b1[0] == 0 and np.array_equal(k1[0, :n], np.arange(n)) and (k1[0, n:] == n - 1).all()
    # the paths through the door shrink to a few cells, and the polyline gets shorter
    assert (count[:3] <= 6).all() and (count[:3] < length[:3]).all()
    assert all(ref.kept_length(cells[p], keep[p], count[p]) < ref.polyline_length(cells[p, :length[p]]) - 1.0
               for p in range(3))
    # a smaller window keeps at least as many cells, and never steps further than the window
    keep8, count8, _ = ref.shortcut(d, NEED, cells, length, 8)
    assert (count8 >= count).all() and all(np.diff(keep8[p, :count8[p]]).max() <= 8 for p in range(len(starts)))


def test_greedy_on_the_empty_volume_keeps_the_two_ends():
    d = np.full((19, 8, 9), OPEN, np.int32)
    cells, length = _descended(d, (18, 7, 8), [(0, 0, 0), (3, 7, 0), (18, 7, 8), (18, 0, 8)], 40)
    keep, count, blocked = ref.shortcut(d, NEED, cells, length, 40)
    assert count.tolist() == [2, 2, 1, 2] and (blocked == 0).all()
    for p in range(4):
        assert keep[p, 0] == 0 and (keep[p, 1:] == length[p] - 1).all()
    keep, count, _ = ref.shortcut(d, NEED, cells, length, int(length.max()))         # window == n is enough
    assert count.tolist() == [2, 2, 1, 2]
    # paths of no cells and cut paths
    keep, count, blocked = ref.shortcut(d, NEED, cells, np.array([0, -3, 1, 77]), 40)
    assert count.tolist() == [0, 0, 1, 2] and (keep[:2] == -1).all() and (keep[2] == 0).all()
    assert keep[3, 0] == 0 and (keep[3, 1:] == 39).all() and (blocked == 0).all()


@pytest.mark.parametrize("n,clear_at", [(12, 7), (130, 100), (130, 30)])
def test_greedy_takes_the_farthest_clear_cell_beyond_nearer_blocked_ones(n, clear_at):
    d, cells = ref.comb(n, clear_at)
    _, blk = ref.sight_from(ref.free_cells(d, NEED), cells[0, 0], cells[0, 1:])
    assert (np.nonzero(blk == 0)[0] + 1).tolist() == [clear_at] and (blk[:clear_at - 1] > 0).all()
    keep, count, blocked = ref.shortcut(d, NEED, cells, [n], n)
    assert keep[0, :count[0]].tolist() == [0, clear_at, clear_at + 1, n - 1] and blocked[0] == 1
    assert all(np.array_equal(x, y) for x, y in zip(ref.shortcut_by_walk(d, NEED, cells, [n], n), (keep, count, blocked)))
    # a window that ends before the clear row sees nothing from row 0: the next row, blocked as it is
    keep, count, blocked = ref.shortcut(d, NEED, cells, [n], clear_at - 1)
    assert keep[0, :2].tolist() == [0, 1] and blocked[0] >= 1 and keep[0, count[0] - 1] == n - 1


# ------------------------------------------------------------------------------------------------
# the host side of gaussiangrasper_amd.transit
# ------------------------------------------------------------------------------------------------
def _field(lo=(0.0, 0.0, 0.0), h=0.01, dims=(40, 36, 44)):
    return types.SimpleNamespace(grid=np.array([*lo, h]), dims=np.array(dims, np.int32), h=h)


def test_euclid_and_best_on_hand_made_inputs():
    from gaussiangrasper_amd import transit
    f = _field()
    centre = lambda *c: (np.array(c) + 0.5) * f.h
    cells = np.array([[(0, 0, 0), (3, 0, 0), (3, 4, 0), (3, 4, 0)],
                      [(1, 1, 1), (1, 1, 1), (1, 1, 1), (1, 1, 1)],
                      [(-1, -1, -1)] * 4], np.int32)
    starts = np.stack([centre(0, 0, 0), centre(1, 1, 1) + [0.003, 0, 0], centre(9, 9, 9)])
    goal = centre(3, 4, 12)
    got = transit.polyline_lengths(f, starts, goal, cells, [3, 1, 0])
    assert got.dtype == np.float64 and np.isinf(got[2])
    assert got[0] == pytest.approx((3 + 4 + 12) * f.h, rel=1e-12)
    assert got[1] == pytest.approx(0.003 + np.linalg.norm(goal - centre(1, 1, 1)), rel=1e-12)
    # the same through tensors, and fewer rows of the same path: the corner is cut
    again = transit.polyline_lengths(f, starts, goal, torch.from_numpy(cells), torch.tensor([3, 1, 0]))
    assert np.array_equal(again, got)
    cut = transit.polyline_lengths(f, starts[:1], goal, cells[:1, [0, 2, 2, 2]], [2])
    assert cut[0] == pytest.approx((5 + 12) * f.h, rel=1e-12) and cut[0] < got[0]
    assert transit.polyline_lengths(f, np.zeros((0, 3)), goal, np.zeros((0, 4, 3), np.int32), []).shape == (0,)
    # best: the smallest rank among the planned and clear, the first of equals, -1 when there is none
    assert transit.best_path([True, True, True], [True, True, True], [3.0, 2.0, 2.0]) == 1
    assert transit.best_path([True, False, True], [False, True, True], [1.0, 0.5, 2.0]) == 2
    assert transit.best_path([True, True], [False, False], [1.0, 2.0]) == -1
    assert transit.best_path([], [], []) == -1
    assert transit.best_path([True, True], [True, True], [np.inf, 7.0]) == 1


def test_the_new_calls_refuse_host_tensors():
    from gaussiangrasper_amd import transit
    d = torch.zeros(4, 4, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transit.sight(d, [4, 4, 4], 4, [[0, 0, 0]], [[1, 1, 1]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transit.shortcut_cells(d, [4, 4, 4], 4, torch.zeros(1, 8, 3, dtype=torch.int32),
                               torch.ones(1, dtype=torch.int32), 8)
    f = types.SimpleNamespace(grid=np.array([0.0, 0.0, 0.0, 0.01]), dims=np.array([4, 4, 4], np.int32), h=0.01, dist2=d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transit.line_of_sight(f, [[0.005, 0.005, 0.005]], [[0.035, 0.035, 0.035]], 0.01)
    ctg = transit.CostToGo(d, 4, np.zeros((1, 3), np.int32), torch.zeros((), dtype=torch.int64), 1, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transit.shortcut(ctg, torch.zeros(1, 8, 3, dtype=torch.int32), torch.ones(1, dtype=torch.int32))
    plan = transit.TransitPlan(None, None, np.zeros(0), -1, np.zeros(0, bool), None, None, ctg)
    assert plan.keep is None and plan.count is None and plan.euclid is None          # new fields, with defaults


def test_sight_and_shortcut_argument_validation_without_a_gpu():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    n = ctypes.c_void_p(0)
    f = ctypes.c_void_p(1 << 20)        # never dereferenced: every call below fails validation first
    odd = ctypes.c_void_p((1 << 20) + 2)
    dims = lambda *d: (ctypes.c_int32 * 3)(*d)
    ok = dims(32, 32, 32)

    def sight(dims=ok, dist2=f, need=4, segments=3, a=f, b=f, cover=f, blocked=f):
        return lib.gg_field_sight(dims, dist2, need, segments, a, b, cover, blocked, n)
    cases = [
        (dict(dims=dims(0, 4, 4)), b"dims"), (dict(dims=dims(4, 1025, 4)), b"dims"), (dict(dims=None), b"dims"),
        (dict(dims=dims(1024, 1024, 129)), b"GG_FIELD_MAX_CELLS"),
        (dict(need=-1), b"need must be in 0..GG_FIELD_FAR"), (dict(need=FAR + 1), b"need must be in 0..GG_FIELD_FAR"),
        (dict(segments=-1), b"num_segments"), (dict(segments=(1 << 26) + 1), b"num_segments"),
        (dict(dist2=n), b"null pointer"), (dict(a=n), b"null pointer"), (dict(b=n), b"null pointer"),
        (dict(cover=n), b"null pointer"), (dict(blocked=n), b"null pointer"),
        (dict(a=odd), b"misaligned"), (dict(blocked=odd), b"misaligned"),
    ]
    for kw, msg in cases:
        assert sight(**kw) == -1 and msg in lib.gg_last_error() and b"gg_field_sight" in lib.gg_last_error(), kw
    assert sight(segments=0, dist2=n, a=n, b=n, cover=n, blocked=n) == 0             # S == 0: nothing to do

    def shortcut(dims=ok, dist2=f, need=4, paths=3, max_cells=8, cells=f, length=f, window=8, keep=f, count=f,
                 blocked=f):
        return lib.gg_field_shortcut(dims, dist2, need, paths, max_cells, cells, length, window, keep, count, blocked,
                                     n)
    cases = [
        (dict(dims=dims(4, 4, 0)), b"dims"), (dict(dims=None), b"dims"),
        (dict(need=-1), b"need must be in 0..GG_FIELD_FAR"), (dict(need=FAR + 1), b"need must be in 0..GG_FIELD_FAR"),
        (dict(paths=-1), b"num_paths"), (dict(max_cells=0), b"max_cells"),
        (dict(paths=1 << 14, max_cells=(1 << 12) + 1), b"GG_FIELD_MAX_POSES"),
        (dict(window=0), b"window must be >= 1"), (dict(window=-4), b"window must be >= 1"),
        (dict(dist2=n), b"null pointer"), (dict(cells=n), b"null pointer"), (dict(length=n), b"null pointer"),
        (dict(keep=n), b"null pointer"), (dict(count=n), b"null pointer"), (dict(blocked=n), b"null pointer"),
        (dict(cells=odd), b"misaligned"), (dict(count=odd), b"misaligned"),
    ]
    for kw, msg in cases:
        assert shortcut(**kw) == -1 and msg in lib.gg_last_error() and b"gg_field_shortcut" in lib.gg_last_error(), kw
    assert shortcut(paths=0, dist2=n, cells=n, length=n, keep=n, count=n, blocked=n) == 0       # P == 0
    assert shortcut(paths=0, window=0) == -1                        # but a bad argument is still refused


def test_cli_shortcut_argument_errors(tmp_path):
    from gaussiangrasper_amd import transit
    base = ["--field", "f.npz", "--from", "a.npy", "--to", "b.npy", "--gripper", "default", "--out", "o.npy",
            "--report", "r.npz"]
    for extra in (["--window", "4"], ["--shortcut", "--window", "0"], ["--shortcut", "--window", "-2"],
                  ["--shortcut", "--window", "x"]):
        with pytest.raises(SystemExit) as e:
            transit.main(base + extra)
        assert e.value.code == 2
    with pytest.raises(SystemExit, match="error"):                # accepted, and the files do not exist
        transit.main(["--field", str(tmp_path / "none.npz"), "--from", str(tmp_path / "a.npy"), "--to",
                      str(tmp_path / "b.npy"), "--gripper", "default", "--out", str(tmp_path / "o.npy"), "--report",
                      str(tmp_path / "r.npz"), "--shortcut", "--window", "16"])
    assert math.isinf(float(transit.polyline_lengths(_field(), [[0, 0, 0]], [0, 0, 1], np.zeros((1, 2, 3)), [0])[0]))
