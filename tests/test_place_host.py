"""No-GPU checks of the placement layer (gaussiangrasper_amd.place, csrc/place.hip's argument checks): the restatement
(tests/place_ref.py) against an independent statement of the max-plus and a brute-force loop, the cell and level rule on
exact boundaries, the frames, the no-penetration property of every proposed placement, propose's gates and order, and
the C calls' host-side validation."""
import ctypes
import math
import threading

import numpy as np
import pytest
import scipy.ndimage

import place_ref as ref
import plane_ref
from gaussiangrasper_amd import place

D = ctypes.c_double
EMPTY, MAXL = ref.EMPTY, ref.MAX_LEVEL
ORIGIN = -plane_ref.TRUE_OFFSET * plane_ref.TRUE_NORMAL


def _maps(rng, U, V, A, B, K, fill=0.7, lo=-500, hi=500):
    top = rng.integers(lo, hi, size=(U, V)).astype(np.int32)
    under = rng.integers(lo, hi, size=(K, A, B)).astype(np.int32)
    under[rng.random((K, A, B)) >= fill] = EMPTY
    return top, under


# ------------------------------------------------------------------------------------------------
# 1. the search restated
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,B", [(5, 4), (4, 5), (1, 1), (6, 6), (3, 8)])
def test_rest_is_a_grey_dilation_by_the_flipped_underside(A, B):
    """scipy's grey_dilation with the structure flipped is out[x] = max_a top[x + a - c] + under[a], c = (A - 1) // 2
    per axis (for 5 x 4: (2, 1)); EMPTY object cells as a large negative never win"""
    rng = np.random.default_rng(A * 10 + B)
    top, under = _maps(rng, 23, 19, A, B, 2)
    under[0, A // 2, B // 2] = 7                                  # no map without a cell
    under[1, 0, 0] = -3
    rest, _, _ = ref.search(top, under, 0)
    neg = -(1 << 40)
    for k in range(2):
        s = np.where(under[k] == EMPTY, neg, under[k].astype(np.int64))
        full = scipy.ndimage.grey_dilation(top.astype(np.int64), structure=s[::-1, ::-1], mode="constant", cval=neg)
        ca, cb = (A - 1) // 2, (B - 1) // 2
        I, J = 23 - A + 1, 19 - B + 1
        assert np.array_equal(rest[k], full[ca:ca + I, cb:cb + J])
    assert (rest != EMPTY).all()


def test_contact_and_support_against_a_triple_loop():
    rng = np.random.default_rng(3)
    top, under = _maps(rng, 11, 9, 4, 3, 3, fill=0.6, lo=-6, hi=6)
    under[2] = EMPTY                                              # a yaw with no cell
    top[0, 0], top[5, 4] = EMPTY, EMPTY
    for tol in (0, 2, MAXL):
        got, want = ref.search(top, under, tol), ref.search_brute(top, under, tol)
        for g, w in zip(got, want):
            assert g.dtype == np.int32 and np.array_equal(g, w), tol
    rest, contact, support = ref.search(top, under, 2)
    assert (rest[2] == EMPTY).all() and (contact[2] == 0).all() and (support[2] == ref.INVALID_SUPPORT).all()
    assert rest[0, 0, 0] == EMPTY or under[0, 0, 0] == EMPTY      # only object cell (0, 0) covers the corner cell
    assert ((rest == EMPTY) == (contact == 0)).all() and (contact[:2] > 0).any()
    every = ref.search(top, under, MAXL)[1]
    cells = np.broadcast_to((under[:2] != EMPTY).sum((1, 2))[:, None, None], rest[:2].shape)
    assert np.array_equal(every[:2][rest[:2] != EMPTY], cells[rest[:2] != EMPTY])


# ------------------------------------------------------------------------------------------------
# 2. the cell and level rule
# ------------------------------------------------------------------------------------------------
def test_cells_and_levels_on_exact_boundaries():
    h, hz = 2.0 ** -3, 2.0 ** -4                                  # powers of two: every product below is exact
    grid, dims = np.array([-1.0, -0.5, h, hz]), (16, 12)
    frame = np.concatenate([np.zeros(3), np.eye(3).reshape(-1)])
    dn = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))          # noqa: E731
    pts = np.array([
        [-1.0, -0.5, 0.0],                        # the grid's corner: cell (0, 0), level 0
        [-1.0 + 3 * h, -0.5 + 2 * h, 5 * hz],     # on a cell corner and a level boundary: the upper ones
        [dn(-1.0 + 3 * h), dn(-0.5 + 2 * h), dn(5 * hz)],      # just below all three
        [-1.0 + 3 * h, -0.5 + 2 * h, -5 * hz],    # a negative level boundary
        [-1.0 + 3 * h, -0.5 + 2 * h, dn(-5 * hz)],
        [1.0, 0.0, 0.0],                          # u = lo + 16 h: the upper face is outside
        [dn(1.0), dn(1.0), 0.0],                  # the last cell of both axes
        [dn(-1.0), 0.0, 0.0],                     # just below the lower face
        [0.0, 0.0, 1e30],                         # clamped levels
        [0.0, 0.0, -1e30],
        [0.0, 0.0, MAXL * hz],
        [0.0, 0.0, dn(-MAXL * hz)],
    ], np.float32)
    a, b, z, fin = ref.cells_levels(pts, frame, grid)
    assert fin.all()
    assert list(zip(a.tolist(), b.tolist(), z.tolist())) == [
        (0, 0, 0), (3, 2, 5), (2, 1, 4), (3, 2, -5), (3, 2, -6), (16, 4, 0), (15, 11, 0), (-1, 4, 0),
        (8, 4, MAXL), (8, 4, -MAXL), (8, 4, MAXL), (8, 4, -MAXL)]
    m, dropped = ref.height_map(pts, None, frame[None], grid, dims)
    assert dropped.tolist() == [2]
    assert m[0, 0, 0] == 0 and m[0, 3, 2] == 5 and m[0, 2, 1] == 4 and m[0, 15, 11] == 0 and m[0, 8, 4] == MAXL
    assert (m != EMPTY).sum() == 5
    # the underside: the same points in the frame with e2 negated hold max level(-c2)
    under, _ = ref.height_map(pts[:5], None, place.underside(frame.reshape(1, 4, 3)), grid, dims)
    assert under[0, 3, 2] == 5 and under[0, 2, 1] == -5 and under[0, 0, 0] == 0
    # weights: null takes every finite point, a threshold is strict, NaN takes no part
    w = np.array([0.5, 0.25, np.nan, 1.0, 0.2500001] + [0.0] * 7, np.float32)
    pts[3, 0] = np.inf
    _, dropped = ref.height_map(pts, w, frame[None], grid, dims, min_weight=0.25)
    assert dropped.tolist() == [10]                               # rows 0 and 4 land


# ------------------------------------------------------------------------------------------------
# 3. frames
# ------------------------------------------------------------------------------------------------
def test_frames_are_orthonormal_and_the_pivot_sits_on_the_corner():
    rng = np.random.default_rng(1)
    planes = [(plane_ref.TRUE_NORMAL, plane_ref.TRUE_OFFSET), ((0.0, 0.0, 1.0), 0.3), ((1.0, 1.0, 1.0), -2.0),
              ((0.0, -2.0, 0.0), 0.5), (rng.normal(size=3), 0.1)]
    for normal, offset in planes:
        centre = rng.normal(size=3)
        f = place.plane_frame((normal, offset), centre)
        M = np.stack([f.e0, f.e1, f.e2])
        n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
        assert np.abs(M @ M.T - np.eye(3)).max() < 1e-15 and np.linalg.det(M) > 0.0
        assert np.array_equal(f.e2, n) and abs(f.e2 @ f.o + offset / np.linalg.norm(normal)) < 1e-14
        assert np.abs(np.cross(centre - f.o, n)).max() < 1e-14             # o is centre's foot on the plane
        again = place.plane_frame((normal, offset), centre)
        assert all(np.array_equal(x, y) for x, y in zip((f.o, f.e0, f.e1), (again.o, again.e0, again.e1)))
        pivot, h, A, B = f.o + 0.2 * n + 0.01 * f.e0, 2.0 ** -7, 10, 7
        frames = place.yaw_frames(f, pivot, [0.0, 0.3, math.pi / 2], A, B, h)
        assert np.array_equal(frames[0, 1:], M)                            # at yaw 0: the plane's axes
        for fr in frames:
            assert np.abs(fr[1:] @ fr[1:].T - np.eye(3)).max() < 1e-15
            # positions: a handful of fp64 roundings on coordinates of magnitude <= 4, each <= 4.4e-16
            assert abs((fr[0] - f.o) @ n) < 1e-14                          # the origin is on the plane
            c = (pivot - fr[0]) @ fr[1:].T
            assert np.abs(c - [(A // 2) * h, (B // 2) * h, 0.2]).max() < 1e-14
        assert np.abs(frames[2, 1] - f.e1).max() < 1e-15 and np.abs(frames[2, 2] + f.e0).max() < 1e-15
    assert np.array_equal(place.yaw_angles(4), [0.0, math.pi / 4, math.pi / 2, 3 * math.pi / 4])
    with pytest.raises(ValueError):
        place.yaw_angles(0)
    with pytest.raises(ValueError):
        place.plane_frame(((0, 0, 0), 1.0), (0, 0, 0))


def test_transform_restated_and_dilation():
    f = place.plane_frame((plane_ref.TRUE_NORMAL, plane_ref.TRUE_OFFSET), (0.1, -0.2, 0.3))
    grid = np.array([-0.25, -0.125, 2.0 ** -7, 2.0 ** -10])
    frames = place.yaw_frames(f, (0.0, 0.1, 0.4), 5, 12, 12, grid[2])
    for k in range(5):
        T = place.placement_transform(f, grid, frames[k], (7, 9), -3 + k)
        assert np.abs(T - ref.placement_transform(f.o, f.e0, f.e1, f.e2, grid, frames[k], (7, 9), -3 + k)).max() < 1e-15
        assert np.abs(T[:, :3] @ T[:, :3].T - np.eye(3)).max() < 1e-15 and np.abs(T[:, :3] @ f.e2 - f.e2).max() < 1e-15
        # the frame's origin lands on the anchor's corner, lifted by (rest + 2) levels
        c = f.coords(T[:, :3] @ frames[k, 0] + T[:, 3])
        assert np.abs(c - [grid[0] + 7 * grid[2], grid[1] + 9 * grid[2], (-3 + k + 2) * grid[3]]).max() < 1e-15
    rng = np.random.default_rng(2)
    m = rng.integers(-50, 50, size=(3, 9, 11)).astype(np.int32)
    m[rng.random(m.shape) < 0.5] = EMPTY
    for d in (0, 1, 2):
        want = np.stack([scipy.ndimage.grey_dilation(x.astype(np.int64), size=(2 * d + 1,) * 2, mode="constant",
                                                     cval=EMPTY) for x in m])
        assert np.array_equal(place.dilate_maps(m, d), want)
    assert place.footprint_cells(0.05, 0.005, 1) == 24
    with pytest.raises(ValueError, match="a cell of at least 0.00806"):
        place.footprint_cells(0.5, 0.005, 1)


# ------------------------------------------------------------------------------------------------
# 4. no placement enters anything
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(dilate=0), dict(dilate=1), dict(dilate=0, max_step=None)],
                         ids=["tight", "dilated", "stacking"])
def test_no_proposed_placement_enters_the_scene(kw):
    """every moved object point is at or above (top[cell] + 1) hz, the height every scene point of that cell lies
    below; without dilation the lowest one is within 2 hz of the scene level it rests on"""
    pts, kind, _ = ref.place_scene()
    plan = ref.reference_plan(target=tuple(ORIGIN), **kw)
    p = plan.placements
    assert len(p.yaw) > 1000 and not (plan.top == EMPTY).any()
    assert plan.top.max() >= 55 and (plan.top <= 2).mean() > 0.8         # the block is in the map, the rest is table
    worst_low, worst_high, worst_skip = math.inf, -math.inf, 0.0
    for m in range(len(p.yaw)):
        gap, skipped = ref.clearance(plan, pts, kind, m)
        worst_low, worst_high, worst_skip = min(worst_low, gap), max(worst_high, gap), max(worst_skip, skipped)
    print(f"{len(p.yaw)} placements: gap {worst_low:.3f} .. {worst_high:.3f} levels, skipped share {worst_skip:.4f}")
    assert worst_skip <= 0.01
    assert worst_low >= 0.0
    if kw["dilate"] == 0:
        assert worst_high + 1.0 <= 2.0         # (top + 1) hz is one level above the scene level it rests on
    if kw.get("max_step", 0) is None:
        assert p.rest.max() >= 50 and (p.rest < 5).any()                  # on the block and on the table
    else:
        assert p.rest.max() - p.rest.min() <= place.MAX_STEP


def test_scene_top_fills_empty_cells_with_the_floor():
    """a table is never sampled densely enough: 20 000 points leave cells of a 72 x 72 map empty"""
    filled, holes = ref.reference_plan(target=tuple(ORIGIN), dilate=0), ref.reference_plan(target=tuple(ORIGIN),
                                                                                         dilate=0, floor=None)
    empty = holes.top == EMPTY
    assert 100 < empty.sum() < 0.5 * empty.size
    assert (filled.top[empty] == 0).all() and np.array_equal(filled.top[~empty], holes.top[~empty])
    assert len(holes.placements.yaw) < len(filled.placements.yaw)


# ------------------------------------------------------------------------------------------------
# 5. propose's gates and order
# ------------------------------------------------------------------------------------------------
def _constructed():
    """a 40 x 40 table at level 0 with a 10 x 10 obstacle at level 50, a drop to -100 from row 32 on (the ledge), and a
    flat 6 x 6 object"""
    top = np.zeros((40, 40), np.int32)
    top[20:30, 20:30] = 50
    top[32:, :] = -100
    under = np.zeros((1, 6, 6), np.int32)
    f = place.PlaneFrame(np.zeros(3), np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0]))
    grid = np.array([0.0, 0.0, 0.01, 0.001])
    pivot = np.array([0.5, 0.5, 0.02])
    frames = place.yaw_frames(f, pivot, [0.0], 6, 6, 0.01)
    found = place.PlaceSearch(*ref.search(top, under, 2))
    return top, under, f, grid, pivot, frames, found


def _anchors(p):
    return {(int(k), int(i), int(j)) for k, (i, j) in zip(p.yaw, p.anchor)}


def test_propose_gates_on_a_constructed_map():
    top, under, f, grid, pivot, frames, found = _constructed()
    on_table, on_block, off_ledge, over_edge = (0, 5, 5), (0, 22, 22), (0, 29, 5), (0, 17, 22)
    assert found.rest[on_block] == 50 and found.contact[on_block] == 36
    assert found.rest[off_ledge] == 0 and found.contact[off_ledge] == 18          # rows 29..31 of 29..34 are table
    assert found.support[off_ledge].tolist() == [18, 45, 0, 2, 0, 5]
    p = place.propose(found, under, f, grid, frames, pivot, max_step=0)
    got = _anchors(p)
    assert on_table in got and on_block not in got and off_ledge not in got and over_edge not in got
    assert set(p.rest.tolist()) == {0, -100} and np.array_equal(p.lift, (p.rest + 2) * 0.001)     # lower is allowed
    assert (p.contact_frac[p.rest == -100] == 1.0).all() and p.contact_frac.min() == 5 / 6
    stack = _anchors(place.propose(found, under, f, grid, frames, pivot, max_step=None))
    assert on_block in stack and on_table in stack and off_ledge not in stack
    assert over_edge not in stack                 # half on the block: the contact box ends before the pivot's cell
    loose = _anchors(place.propose(found, under, f, grid, frames, pivot, max_step=None, stability_margin=0))
    # four rows on the table: the box 0..3 holds the pivot's cell 3 only when it is not shrunk
    assert off_ledge not in loose and (0, 28, 5) in loose and (0, 28, 5) not in stack
    assert (0, 34, 5) in got                      # wholly below the ledge it rests flat again, at level -100
    # min_contact: (0, 18, 22) has 4 of its 6 rows on the block and its pivot's cell inside the shrunk box
    few = _anchors(place.propose(found, under, f, grid, frames, pivot, max_step=None, min_contact=0.7))
    assert found.contact[0, 18, 22] == 24 and (0, 18, 22) in stack and (0, 18, 22) not in few and on_block in few


def test_propose_order_by_target_and_ties():
    top, under, f, grid, pivot, frames, found = _constructed()
    p = place.propose(found, under, f, grid, frames, pivot, max_step=0)
    keys = list(zip(p.yaw.tolist(), p.anchor[:, 0].tolist(), p.anchor[:, 1].tolist()))
    assert np.array_equal(p.score, -p.contact_frac) and (np.diff(p.score) >= 0).all()       # best contact first
    assert sorted(set(p.contact_frac.tolist())) == [5 / 6, 1.0]       # 4 of 6 rows: the shrunk box misses the pivot
    for frac in (5 / 6, 1.0):                             # among ties: (k, i, j) ascending
        tie = [key for key, c in zip(keys, p.contact_frac.tolist()) if c == frac]
        assert tie == sorted(tie) and len(tie) >= 20
    target = np.array([0.1 + 0.03, 0.12 + 0.03, 0.0])            # the corner the pivot has at anchor (10, 12)
    q = place.propose(found, under, f, grid, frames, pivot, max_step=0, target=target, top_k=9)
    assert q.anchor[0].tolist() == [10, 12] and len(q.yaw) == 9
    assert abs(q.score[0] - (0.02 + 0.002)) < 1e-12             # the pivot's own height plus the lift
    ring = list(zip(q.anchor[1:5, 0].tolist(), q.anchor[1:5, 1].tolist()))
    assert sorted(ring) == [(9, 12), (10, 11), (10, 13), (11, 12)]
    assert (np.diff(q.score) >= 0).all()
    # equal distances keep (k, i, j) order wherever fp64 gives the very same score
    same = q.score[1:5]
    for a in range(4):
        for b in range(a + 1, 4):
            if same[a] == same[b]:
                assert ring[a] < ring[b]
    landed = q.transform[0, :, :3] @ pivot + q.transform[0, :, 3]
    assert np.abs(landed - [0.13, 0.15, 0.022]).max() < 1e-12


def test_release_paths_carry_the_grasp_down_onto_the_placement():
    top, under, f, grid, pivot, frames, found = _constructed()
    p = place.propose(found, under, f, grid, frames, pivot, max_step=0, top_k=3)
    row = np.zeros(17)
    row[4:13] = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]]).reshape(-1)
    row[13:16] = pivot + [0, 0, 0.05]
    paths = place.release_paths(p, row, 0.1, 5)
    assert paths.shape == (3, 5, 12) and paths.dtype == np.float32
    for m in range(3):
        T = p.transform[m]
        assert np.abs(paths[m, -1, :9].reshape(3, 3) - T[:, :3] @ row[4:13].reshape(3, 3)).max() < 1e-6
        assert np.abs(paths[m, -1, 9:] - (T[:, :3] @ row[13:16] + T[:, 3])).max() < 1e-6
        assert np.abs((paths[m, 0, 9:] - paths[m, -1, 9:]) - 0.1 * f.e2).max() < 1e-6
        assert (np.diff(paths[m, :, 11]) < 0).all() and np.array_equal(paths[m, 0, :9], paths[m, -1, :9])
    with pytest.raises(ValueError):
        place.release_paths(p, row, 0.1, 1)


# ------------------------------------------------------------------------------------------------
# 6. the C calls' argument checks
# ------------------------------------------------------------------------------------------------
def _call_on_thread(fn, cases):
    got = []

    def run():
        for kw in cases:
            got.append(fn(kw))
    t = threading.Thread(target=run)        # gg_last_error is per thread: the message does not outlive the test
    t.start()
    t.join()
    return got


def test_argument_validation_without_a_gpu():
    """dimension checks first, then everything else; refused on the host before anything is launched"""
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    assert lib.gg_abi_version() == 6
    n = ctypes.c_void_p(0)
    f = ctypes.c_void_p(1 << 20)                 # never dereferenced: every call below fails validation first
    I2 = ctypes.c_int32 * 2
    host = lambda a: ctypes.cast(a, ctypes.c_void_p)       # noqa: E731
    dims_ok, grid_ok = I2(64, 48), (D * 4)(0.0, 0.0, 0.01, 0.001)

    def hm(num_points=100, points=f, weights=n, min_weight=0.0, num_frames=4, frames=f, grid=grid_ok, dims=dims_ok,
           out=f, dropped=f):
        return lib.gg_height_map(num_points, points, weights, D(min_weight), num_frames, frames,
                                 n if grid is None else host(grid), n if dims is None else host(dims), out, dropped, n)
    cases = [
        (dict(dims=None, num_points=-1, grid=None), b"dims"),           # the dimensions come first
        (dict(dims=I2(0, 4), num_frames=0), b"dims"),
        (dict(dims=I2(4, 4097)), b"GG_PLACE_MAX_DIM"),
        (dict(num_frames=0), b"num_frames"),
        (dict(num_frames=257), b"GG_PLACE_MAX_YAWS"),
        (dict(num_points=-1), b"num_points"),
        (dict(num_points=(1 << 30) + 1), b"GG_PLACE_MAX_POINTS"),
        (dict(grid=None), b"grid"),
        (dict(grid=(D * 4)(0.0, 0.0, 0.0, 0.001)), b"grid"),
        (dict(grid=(D * 4)(0.0, 0.0, 0.01, -1.0)), b"grid"),
        (dict(grid=(D * 4)(math.nan, 0.0, 0.01, 0.001)), b"grid"),
        (dict(grid=(D * 4)(0.0, math.inf, 0.01, 0.001)), b"grid"),
        (dict(min_weight=math.nan), b"min_weight"),
        (dict(dropped=n), b"dropped"),
        (dict(dropped=ctypes.c_void_p((1 << 20) + 4)), b"dropped"),
        (dict(points=n), b"null pointer: points"),
        (dict(frames=n), b"null pointer: points / frames"),
        (dict(out=n), b"map"),
        (dict(points=ctypes.c_void_p((1 << 20) + 2)), b"misaligned"),
        (dict(weights=ctypes.c_void_p((1 << 20) + 1)), b"misaligned"),
        (dict(frames=ctypes.c_void_p((1 << 20) + 4)), b"misaligned"),
    ]
    got = _call_on_thread(lambda kw: (hm(**kw), lib.gg_last_error()), [c[0] for c in cases])
    for (st, msg), (kw, want) in zip(got, cases):
        assert st == -1 and msg.startswith(b"gg_height_map") and want in msg, (kw, msg)

    def ps(dims=dims_ok, top=f, num_yaws=3, foot=I2(8, 6), under=f, tol=2, outs=(f, f, f)):
        return lib.gg_place_search(n if dims is None else host(dims), top, num_yaws, n if foot is None else host(foot),
                                   under, tol, *outs, n)
    cases = [
        (dict(dims=None, foot=None, tol=-1), b"dims"),
        (dict(dims=I2(4097, 4), num_yaws=-1), b"dims"),
        (dict(num_yaws=-1), b"num_yaws"),
        (dict(num_yaws=257), b"GG_PLACE_MAX_YAWS"),
        (dict(foot=None), b"foot"),
        (dict(foot=I2(0, 4)), b"foot"),
        (dict(foot=I2(4, 129)), b"GG_PLACE_MAX_FOOT"),
        (dict(foot=I2(65, 4)), b"A <= U"),
        (dict(foot=I2(8, 49)), b"B <= V"),
        (dict(tol=-1), b"tol"),
        (dict(tol=MAXL + 1), b"tol"),
        (dict(top=n), b"null pointer: top"),
        (dict(under=n), b"under"),
        (dict(outs=(n, f, f)), b"rest"),
        (dict(outs=(f, n, f)), b"contact"),
        (dict(outs=(f, f, n)), b"support"),
        (dict(top=ctypes.c_void_p((1 << 20) + 2)), b"misaligned"),
        (dict(outs=(f, f, ctypes.c_void_p((1 << 20) + 1))), b"misaligned"),
    ]
    got = _call_on_thread(lambda kw: (ps(**kw), lib.gg_last_error()), [c[0] for c in cases])
    for (st, msg), (kw, want) in zip(got, cases):
        assert st == -1 and msg.startswith(b"gg_place_search") and want in msg, (kw, msg)
    # no yaw: nothing to do, null pointers accepted, nothing launched
    assert ps(num_yaws=0, top=n, under=n, outs=(n, n, n)) == 0


def test_wrappers_refuse_what_the_contract_excludes():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        place.height_map(torch.zeros(4, 3), None, np.zeros((1, 12)), [0, 0, 0.1, 0.1], (4, 4))
    with pytest.raises(ValueError):
        place.plane_grid((0, 0, 1, 1), cell=1e-4)                 # 10 000 cells per axis
    grid, dims = place.plane_grid((-0.3, -0.3, 0.3, 0.3), 0.005, 0.001)
    assert dims.tolist() == [120, 120] and grid.tolist() == [-0.3, -0.3, 0.005, 0.001]
    assert place.EMPTY == EMPTY and place.MAX_LEVEL == MAXL
    assert (place.MAX_DIM, place.MAX_FOOT, place.MAX_YAWS) == (ref.MAX_DIM, ref.MAX_FOOT, ref.MAX_YAWS)
