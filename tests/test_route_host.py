"""No-GPU checks of transit planning: the restatement (tests/route_ref.py) against forms that share nothing with it,
the host helpers of gaussiangrasper_amd.transit, and the two C entries' argument validation (nothing is launched)."""
import ctypes
import heapq
import math
import types

import numpy as np
import pytest
import torch

import route_ref as ref

FAR = ref.FAR


def _dims(*d):
    return (ctypes.c_int32 * 3)(*d)


def _volume(rng, dims, density, need=4):
    """dist2 that is below `need` on a random share `density` of the cells and above it elsewhere"""
    return np.where(rng.random(dims) < density, 0, 100).astype(np.int32)


def heap_route(dist2, need, goals):
    """Dijkstra with a heap over cells as tuples; the block rule from the definition, cell by cell"""
    d = np.asarray(dist2)
    X, Y, Z = d.shape

    def free(c):
        return 0 <= c[0] < X and 0 <= c[1] < Y and 0 <= c[2] < Z and d[c] >= need

    cost = np.full(d.shape, FAR, np.int64)
    heap = []
    for g in goals:
        g = tuple(int(v) for v in g)
        if free(g):
            cost[g] = 0
            heap.append((0, g))
    heapq.heapify(heap)
    while heap:
        k, c = heapq.heappop(heap)
        if k > cost[c]:
            continue
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    nz = (dx != 0) + (dy != 0) + (dz != 0)
                    if nz == 0:
                        continue
                    if not all(free((c[0] + ex, c[1] + ey, c[2] + ez))
                               for ex in {0, dx} for ey in {0, dy} for ez in {0, dz}):
                        continue
                    n = (c[0] + dx, c[1] + dy, c[2] + dz)
                    if k + 2 + nz < cost[n]:
                        cost[n] = k + 2 + nz
                        heapq.heappush(heap, (k + 2 + nz, n))
    return cost.astype(np.int32)


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def test_move_numbers_and_weights():
    assert len(ref.MOVES) == 26 and [m for m, *_ in ref.MOVES] == [m for m in range(27) if m != 13]
    for m, dx, dy, dz in ref.MOVES:
        assert m == (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)
        assert ref.weight(m) == {1: 3, 2: 4, 3: 5}[abs(dx) + abs(dy) + abs(dz)]


@pytest.mark.parametrize("dims,density,seed", [((7, 6, 5), 0.0, 0), ((9, 8, 7), 0.2, 1), ((6, 11, 9), 0.35, 2),
                                               ((10, 10, 10), 0.5, 3), ((1, 1, 9), 0.2, 4)])
def test_restatement_against_a_heap_dijkstra(dims, density, seed):
    rng = np.random.default_rng(seed)
    d = _volume(rng, dims, density)
    goals = np.concatenate([rng.integers(0, dims, size=(3, 3)), [[-1, 0, 0], [0, 0, dims[2]]]])
    cost, ignored = ref.route(d, 4, goals)
    assert cost.dtype == np.int32 and np.array_equal(cost, heap_route(d, 4, goals))
    blocked = sum(1 for g in goals[:3] if d[tuple(g)] < 4)
    assert ignored == 2 + blocked


def test_empty_volume_has_the_closed_form():
    dims, goal = (9, 12, 10), (2, 7, 4)
    d = np.full(dims, FAR, np.int32)
    cost, ignored = ref.route(d, 7, [goal])
    off = np.sort(np.abs(np.stack(np.meshgrid(*[np.arange(n) for n in dims], indexing="ij"), -1) - goal), -1)
    lo, mid, hi = off[..., 0], off[..., 1], off[..., 2]
    # lo moves along all three axes, mid - lo along two, hi - mid along one
    assert ignored == 0 and np.array_equal(cost, 5 * lo + 4 * (mid - lo) + 3 * (hi - mid))
    none, ignored = ref.route(d, 7, np.zeros((0, 3), np.int32))
    assert ignored == 0 and (none == FAR).all()
    shut, ignored = ref.route(np.zeros(dims, np.int32), 1, [goal])
    assert ignored == 1 and (shut == FAR).all()
    everywhere, _ = ref.route(np.zeros(dims, np.int32), 0, [goal])
    assert np.array_equal(everywhere, cost)


def test_block_rule_forbids_squeezing_between_cells_that_touch():
    d = np.full((4, 4, 1), 100, np.int32)
    d[1, 2, 0] = d[2, 1, 0] = 0                              # two blocked cells touching by an edge (a corner in 2-D)
    al = ref.allowed(d, 4)
    m_diag = (1 + 1) * 9 + (1 + 1) * 3 + 1
    assert not al[m_diag, 1, 1, 0] and al[m_diag, 2, 2, 0] and not al[m_diag, 3, 3, 0]      # the last one leaves
    d3 = np.full((4, 4, 4), 100, np.int32)
    d3[1, 1, 2] = d3[2, 2, 1] = 0                            # touching by a corner
    al = ref.allowed(d3, 4)
    assert not al[26, 1, 1, 1] and not al[0, 2, 2, 2]
    # symmetric: the move back needs the same cells
    for m, dx, dy, dz in ref.MOVES:
        back = 26 - m
        assert np.array_equal(ref._shift(al[back], dx, dy, dz) & al[m], al[m])


@pytest.mark.parametrize("seed,density", [(0, 0.0), (1, 0.1), (2, 0.2)])
def test_descended_paths_add_up_and_use_allowed_moves(seed, density):
    rng = np.random.default_rng(seed)
    dims = (10, 9, 11)
    d = _volume(rng, dims, density)
    d[0, 0, 0] = 100
    cost, _ = ref.route(d, 4, [(0, 0, 0)])
    starts = np.concatenate([rng.integers(0, dims, size=(24, 3)), [[0, 0, 0], [-1, 2, 2], [10, 0, 0]]])
    cells, length = ref.descend(d, 4, cost, starts, 64)
    al = ref.allowed(d, 4)
    seen = 0
    for p, s in enumerate(starts):
        inside = ((s >= 0) & (s < dims)).all()
        if not inside or cost[tuple(s)] >= FAR:
            assert length[p] == 0 and (cells[p] == -1).all()
            continue
        n = int(length[p])
        assert n >= 1 and tuple(cells[p, 0]) == tuple(s) and cost[tuple(cells[p, n - 1])] == 0
        total = 0
        for a, b in zip(cells[p, :n - 1], cells[p, 1:n]):
            dx, dy, dz = (int(v) for v in b - a)
            m = (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)
            assert max(abs(dx), abs(dy), abs(dz)) == 1 and al[m][tuple(a)]
            total += ref.weight(m)
        assert total == cost[tuple(s)]
        assert (cells[p, n:] == cells[p, n - 1]).all()
        seen += n > 1
    assert seen >= 5 and length[24] == 1
    # cut: the count is the whole path's, the rows are its first ones
    long = int(length.max())
    cut, n2 = ref.descend(d, 4, cost, starts, long - 1)
    assert np.array_equal(n2, length) and np.array_equal(cut, cells[:, :long - 1])


def test_ties_take_the_lowest_move_number():
    d = np.full((5, 5, 5), FAR, np.int32)
    cost, _ = ref.route(d, 0, [(0, 0, 0)])
    cells, length = ref.descend(d, 0, cost, [(2, 4, 1)], 8)
    # cost 3 + 4 + 5 + 3: of the moves that fit at the start, (-1, -1, -1) has the lowest number
    assert length[0] == 5 and tuple(cells[0, 1]) == (1, 3, 0) and tuple(cells[0, 2]) == (0, 2, 0)


# ------------------------------------------------------------------------------------------------
# the host helpers
# ------------------------------------------------------------------------------------------------
def _field(lo=(-0.25, 0.125, 0.5), h=2.0 ** -6, dims=(40, 36, 44)):
    return types.SimpleNamespace(grid=np.array([*lo, h]), dims=np.array(dims, np.int32), h=h)


def test_cells_of_on_faces_and_outside():
    from gaussiangrasper_amd import transit
    f = _field()
    lo, h = f.grid[:3], f.h
    c = np.array([[0, 0, 0], [5, 7, 9], [40, 36, 44], [-1, 3, -2], [39, 35, 43]])
    on_faces = lo + c * h                                       # exact: h is a power of two
    assert np.array_equal(transit.cells_of(f, on_faces), c)     # a face belongs to the cell above it
    # just below a face: with the corner at 0 the rule's d = p - lo is p itself
    f0 = _field(lo=(0.0, 0.0, 0.0))
    assert np.array_equal(transit.cells_of(f0, np.nextafter(c * h, -np.inf)), c - 1)
    assert np.array_equal(transit.cells_of(f, transit.cell_centres(f, c)), c)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0.0, 0.2, 0.6]])
    got = transit.cells_of(f, bad)
    assert got.dtype == np.int32 and (got[:2] == -1).all() and (got[2] >= 0).all()
    # the clamp of field_cell.h, then its correction by one: far outside every volume either way
    assert (transit.cells_of(f, [[1e300, -1e300, 0.6]])[0, :2] == [2 ** 30 + 1, -2 ** 30 - 1]).all()
    # a cell edge that is no power of two: the comparisons decide, not the division
    g = _field(lo=(0.0, 0.0, 0.0), h=0.01, dims=(100, 100, 100))
    k = np.arange(100.0)
    pts = np.stack([k * 0.01, np.nextafter(k * 0.01, -1.0), (k + 1.0) * 0.01], 1)
    got = transit.cells_of(g, pts)
    assert np.array_equal(got[:, 0], k) and np.array_equal(got[:, 1], k - 1) and np.array_equal(got[:, 2], k + 1)
    assert transit.cells_of(g, torch.tensor([[0.505, 0.005, 0.995]])).tolist() == [[50, 0, 99]]


def test_bounding_radius_and_carried_spheres_cover_their_inputs():
    from gaussiangrasper_amd import field, transit
    rng = np.random.default_rng(0)
    sp = rng.uniform(-0.1, 0.1, size=(50, 3))
    r = rng.uniform(0.0, 0.02, size=50)
    b = transit.bounding_radius(sp, r)
    assert b == (np.linalg.norm(sp, axis=1) + r).max()
    for _ in range(20):                                          # every point of every ball, at any orientation
        u = rng.normal(size=(50, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        assert (np.linalg.norm(sp + u * r[:, None], axis=1) <= b * (1 + 1e-12)).all()
    assert transit.bounding_radius(sp, 0.01) == np.linalg.norm(sp, axis=1).max() + 0.01
    with pytest.raises(ValueError):
        transit.bounding_radius(np.zeros((0, 3)), 0.01)
    pts = rng.uniform(-0.03, 0.05, size=(4000, 3))
    pts[7] = np.nan
    cs = transit.carried_spheres(pts, 0.01)
    assert cs.dtype == np.float32 and cs.ndim == 2 and 1 < len(cs) <= field.MAX_SPHERES
    ok = np.isfinite(pts).all(1)
    gap = np.linalg.norm(pts[ok, None, :] - cs[None].astype(np.float64), axis=2).min(1)
    assert gap.max() <= 0.01
    assert len(transit.carried_spheres(torch.from_numpy(pts), 0.01)) == len(cs)
    assert transit.carried_spheres(np.zeros((0, 3)), 0.01).shape == (0, 3)
    with pytest.raises(ValueError, match="more than"):
        transit.carried_spheres(rng.uniform(-1, 1, size=(5000, 3)), 0.005)
    h = 0.01
    want = (b + math.sqrt(3.0) * h) * (1 + 1e-6)
    assert transit.planning_radius(sp, r, h) == want and want > b + math.sqrt(3.0) * h


def _pose(rng, t):
    from grasp_ref import rotation
    return np.concatenate([rotation(rng, 1)[0].reshape(-1), t]).astype(np.float32)


@pytest.mark.parametrize("steps", [2, 3, 17, 200])
def test_transit_poses_ends_are_exact_and_points_stay_in_their_block(steps):
    from gaussiangrasper_amd import transit
    from gaussiangrasper_amd.field import interpolate
    rng = np.random.default_rng(steps)
    f = _field(lo=(0.0, 0.0, 0.0), h=0.01, dims=(12, 12, 12))
    d = np.full((12, 12, 12), FAR, np.int32)
    d[3:9, 5, :] = 0                                             # a wall to go round
    cost, _ = ref.route(d, 1, [(6, 9, 2)])
    cells, length = ref.descend(d, 1, cost, [(5, 1, 8)], 40)
    n = int(length[0])
    assert 8 < n <= 40
    a = _pose(rng, f.grid[:3] + (np.array([5, 1, 8]) + rng.uniform(0.02, 0.98, 3)) * f.h)
    b = _pose(rng, f.grid[:3] + (np.array([6, 9, 2]) + rng.uniform(0.02, 0.98, 3)) * f.h)
    assert transit.cells_of(f, a[None, 9:]).tolist() == [[5, 1, 8]]
    poses = transit.transit_poses(a, b, cells[0], n, f, steps)
    assert poses.dtype == np.float32 and poses.shape == (steps, 12)
    assert np.array_equal(poses[0], a) and np.array_equal(poses[-1], b)
    # the rotations are field.interpolate's at the arc fraction: orthonormal, and monotone along the arc
    R = poses[:, :9].reshape(-1, 3, 3).astype(np.float64)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6
    assert np.allclose(interpolate(a, b, 2), poses[[0, -1]])
    # every point lies in a cell of its segment's block: the cells c + e, e_a in {0, d_a}, of the move it is on (an
    # end stub stays in the end's cell)
    line = np.concatenate([a[None, 9:].astype(np.float64), transit.cell_centres(f, cells[0, :n]),
                           b[None, 9:].astype(np.float64)])
    pts, seg, frac = transit.polyline_points(line, steps)
    assert np.allclose(pts, poses[:, 9:], atol=1e-7) and frac[0] == 0.0 and frac[-1] == 1.0
    assert (np.diff(frac) > 0).all() and (np.diff(seg) >= 0).all()
    chain = np.concatenate([cells[0, :1], cells[0, :n], cells[0, n - 1:n]]).astype(np.int64)      # cells of the line's points
    for kind, at in (("fp64", pts), ("fp32", poses[:, 9:])):
        got = transit.cells_of(f, at)
        for i in range(steps):
            c0, c1 = chain[seg[i]], chain[seg[i] + 1]
            assert ((got[i] >= np.minimum(c0, c1)) & (got[i] <= np.maximum(c0, c1))).all(), (kind, i)
    # equal arc length
    step = np.linalg.norm(np.diff(pts, axis=0), axis=1)
    total = np.linalg.norm(np.diff(line, axis=0), axis=1).sum()
    assert (step <= total / (steps - 1) * (1 + 1e-9)).all()
    with pytest.raises(ValueError):
        transit.transit_poses(a, b, cells[0], 0, f, steps)
    with pytest.raises(ValueError):
        transit.transit_poses(a, b, cells[0], n, f, 1)


def test_polyline_points_with_segments_of_no_length():
    from gaussiangrasper_amd import transit
    line = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [1, 0, 0], [1, 2, 0], [1, 2, 0]], np.float64)
    pts, seg, frac = transit.polyline_points(line, 7)
    assert np.allclose(pts[:, 0], [0, 0.5, 1, 1, 1, 1, 1]) and np.allclose(pts[:, 1], [0, 0, 0, 0.5, 1, 1.5, 2])
    assert set(seg.tolist()) <= {1, 3} and np.allclose(frac, np.arange(7) / 6)
    pts, seg, frac = transit.polyline_points(np.ones((3, 3)), 4)
    assert (pts == 1).all() and (seg == 0).all() and np.allclose(frac, [0, 1 / 3, 2 / 3, 1])


# ------------------------------------------------------------------------------------------------
# the C entries without a GPU
# ------------------------------------------------------------------------------------------------
def test_route_argument_validation_without_a_gpu():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    n = ctypes.c_void_p(0)
    f = ctypes.c_void_p(1 << 20)        # never dereferenced: every call below fails validation first
    odd = ctypes.c_void_p((1 << 20) + 2)
    rounds = ctypes.c_int(-7)
    ok = _dims(32, 32, 32)
    big = lib.gg_field_route_workspace(ok)

    def route(dims=ok, dist2=f, need=4, goals_n=1, goals=f, cost=f, ignored=f, max_rounds=16, rounds_out=rounds,
              ws=ctypes.c_void_p(1 << 20), ws_bytes=big):
        out = ctypes.byref(rounds_out) if rounds_out is not None else None
        return lib.gg_field_route(dims, dist2, need, goals_n, goals, cost, ignored, max_rounds, out, ws, ws_bytes, n)
    cases = [
        (dict(dims=_dims(0, 4, 4)), b"dims"), (dict(dims=_dims(4, 1025, 4)), b"dims"),
        (dict(dims=_dims(1024, 1024, 129)), b"GG_FIELD_MAX_CELLS"), (dict(dims=None), b"dims"),
        (dict(need=-1), b"need must be in 0..GG_FIELD_FAR"), (dict(need=FAR + 1), b"need must be in 0..GG_FIELD_FAR"),
        (dict(goals_n=-1), b"num_goals"), (dict(goals_n=(1 << 24) + 1), b"num_goals"),
        (dict(max_rounds=0), b"max_rounds must be >= 1"), (dict(max_rounds=-5), b"max_rounds must be >= 1"),
        (dict(rounds_out=None), b"null pointer: rounds_out"),
        (dict(dist2=n), b"null pointer: dist2 / cost / ignored"), (dict(cost=n), b"null pointer: dist2 / cost / ignored"),
        (dict(ignored=n), b"null pointer: dist2 / cost / ignored"), (dict(goals=n), b"null pointer: goals"),
        (dict(cost=odd), b"misaligned"), (dict(goals=odd), b"misaligned"),
        (dict(ignored=ctypes.c_void_p((1 << 20) + 4)), b"misaligned"),
        (dict(ws=n), b"ws must be non-null"), (dict(ws=ctypes.c_void_p((1 << 20) + 128)), b"256-byte aligned"),
    ]
    for kw, msg in cases:
        assert route(**kw) == -1 and msg in lib.gg_last_error() and b"gg_field_route" in lib.gg_last_error(), (kw, msg)
    assert route(ws_bytes=big - 1) == -3 and b"workspace too small" in lib.gg_last_error()
    assert rounds.value == -7                                    # nothing was written before validation ended

    def descend(dims=ok, dist2=f, need=4, cost=f, paths=3, starts=f, max_cells=8, cells=f, length=f):
        return lib.gg_field_descend(dims, dist2, need, cost, paths, starts, max_cells, cells, length, n)
    cases = [
        (dict(dims=_dims(4, 4, 0)), b"dims"), (dict(dims=None), b"dims"),
        (dict(need=-1), b"need must be in 0..GG_FIELD_FAR"), (dict(need=FAR + 1), b"need must be in 0..GG_FIELD_FAR"),
        (dict(paths=-1), b"num_paths"), (dict(max_cells=0), b"max_cells"),
        (dict(paths=1 << 14, max_cells=(1 << 12) + 1), b"GG_FIELD_MAX_POSES"),
        (dict(dist2=n), b"null pointer"), (dict(cost=n), b"null pointer"), (dict(starts=n), b"null pointer"),
        (dict(cells=n), b"null pointer"), (dict(length=n), b"null pointer"),
        (dict(starts=odd), b"misaligned"), (dict(length=odd), b"misaligned"),
    ]
    for kw, msg in cases:
        assert descend(**kw) == -1 and msg in lib.gg_last_error() and b"gg_field_descend" in lib.gg_last_error(), kw
    assert descend(paths=0, dist2=n, cost=n, starts=n, cells=n, length=n) == 0      # P == 0: nothing to do


def test_route_workspace_query_is_a_pure_host_call():
    from gaussiangrasper_amd import _lib
    ws = _lib.load().gg_field_route_workspace
    for bad in ((0, 1, 1), (1, 1, 1025), (-3, 4, 4), (1024, 1024, 129)):
        assert ws(_dims(*bad)) == 0
    assert ws(None) == 0
    sizes = [ws(_dims(*d)) for d in ((1, 1, 1), (8, 8, 8), (9, 8, 8), (40, 36, 44), (128, 128, 128), (512, 512, 512))]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
    # two flag words per brick and the counters of one batch of rounds
    assert sizes[-1] >= 2 * 4 * 64 ** 3 and sizes[-1] < 3 * 4 * 64 ** 3


def test_the_calls_refuse_host_tensors_and_bad_arguments():
    from gaussiangrasper_amd import transit
    d = torch.zeros(4, 4, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transit.route(d, [4, 4, 4], 4, [[0, 0, 0]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transit.descend_cells(d, [4, 4, 4], 4, d, [[0, 0, 0]], 8)
    assert transit.MAX_GOALS == 1 << 24 and transit.STEPS == 64 and transit.MAX_ROUNDS == 4096


def test_cli_argument_errors(tmp_path, capsys):
    from gaussiangrasper_amd import transit
    base = ["--field", "f.npz", "--from", "a.npy", "--to", "b.npy", "--gripper", "default", "--out", "o.npy",
            "--report", "r.npz"]
    for extra in (["--radius", "0"], ["--margin", "-1"], ["--steps", "1"], ["--width", "nan"]):
        with pytest.raises(SystemExit) as e:
            transit.main(base + extra)
        assert e.value.code == 2
    with pytest.raises(SystemExit, match="error"):                # the files do not exist
        transit.main(["--field", str(tmp_path / "none.npz"), "--from", str(tmp_path / "a.npy"), "--to",
                      str(tmp_path / "b.npy"), "--gripper", "default", "--out", str(tmp_path / "o.npy"), "--report",
                      str(tmp_path / "r.npz")])
