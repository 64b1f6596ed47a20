"""GPU checks of the line of sight and of string pulling (gg_field_sight, gg_field_shortcut and their users in
gaussiangrasper_amd.transit) against the restatement (tests/shortcut_ref.py).  Everything is held to equality; the C
calls' arrays are carved from the sentinel arena (tests/arena.py) and compared whole."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import route_ref
import shortcut_ref as ref
from arena import Arena

gpu = pytest.mark.gpu
DEV = "cuda:0"
FAR = route_ref.FAR
NEED, OPEN, SHUT = ref.NEED, ref.OPEN, ref.SHUT


def _lib():
    from gaussiangrasper_amd import _lib as L
    return L.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def c_sight(dist2, need, a, b, seed=0):
    """gg_field_sight on a sentinel arena -> (cover, blocked)"""
    dist2 = np.asarray(dist2, np.int32)
    a, b = np.asarray(a, np.int32).reshape(-1, 3), np.asarray(b, np.int32).reshape(-1, 3)
    S = len(a)
    ar = Arena(DEV, seed)
    ar.carve("dist2", dist2, 4, "in")
    if S:
        ar.carve("a", a, 4, "in")
        ar.carve("b", b, 4, "in")
    ar.carve("cover", np.zeros(S, np.int32), 4, "out")
    ar.carve("blocked", np.zeros(S, np.int32), 4, "out")
    st = _lib().gg_field_sight((ctypes.c_int32 * 3)(*dist2.shape), ar.ptr("dist2"), int(need), S,
                               ar.ptr("a") if S else None, ar.ptr("b") if S else None, ar.ptr("cover"),
                               ar.ptr("blocked"), _stream())
    assert st == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    if S == 0:
        assert ar.untouched()
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    out = ar.check()
    return out["cover"], out["blocked"]


def c_shortcut(dist2, need, cells, length, window, seed=0):
    """gg_field_shortcut on a sentinel arena -> (keep, count, blocked)"""
    dist2, cells = np.asarray(dist2, np.int32), np.asarray(cells, np.int32)
    length = np.asarray(length, np.int32).reshape(-1)
    P, max_cells = cells.shape[:2]
    ar = Arena(DEV, seed)
    ar.carve("dist2", dist2, 4, "in")
    if P:
        ar.carve("cells", cells, 4, "in")
        ar.carve("length", length, 4, "in")
    ar.carve("keep", np.zeros((P, max_cells), np.int32), 4, "out")
    ar.carve("count", np.zeros(P, np.int32), 4, "out")
    ar.carve("blocked", np.zeros(P, np.int32), 4, "out")
    st = _lib().gg_field_shortcut((ctypes.c_int32 * 3)(*dist2.shape), ar.ptr("dist2"), int(need), P, max_cells,
                                  ar.ptr("cells") if P else None, ar.ptr("length") if P else None, int(window),
                                  ar.ptr("keep"), ar.ptr("count"), ar.ptr("blocked"), _stream())
    assert st == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    if P == 0:
        assert ar.untouched()
        return np.zeros((0, max_cells), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    out = ar.check()
    return out["keep"], out["count"], out["blocked"]


def check_sight(dist2, need, a, b, seed=0, want=None):
    cover, blocked = ref.sight(dist2, need, a, b) if want is None else want
    got = c_sight(dist2, need, a, b, seed)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], cover), \
        f"cover: {int((got[0] != cover).sum())} segments differ, the first {np.nonzero(got[0] != cover)[0][:1].tolist()}"
    assert np.array_equal(got[1], blocked), \
        f"blocked: {int((got[1] != blocked).sum())} segments differ, the first {np.nonzero(got[1] != blocked)[0][:1].tolist()}"
    return cover, blocked


def check_shortcut(dist2, need, cells, length, window, seed=0):
    want = ref.shortcut(dist2, need, cells, length, window)
    got = c_shortcut(dist2, need, cells, length, window, seed)
    for name, g, w in zip(("keep", "count", "blocked"), got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w), \
            f"{name}: paths {np.nonzero((g != w).reshape(len(g), -1).any(1))[0][:8].tolist()} differ (window {window})"
    return want


def random_volume(dims, density, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(dims) < density, SHUT, OPEN).astype(np.int32)


def descended(d, goal, starts, room):
    cost, _ = route_ref.route(d, NEED, [goal])
    return route_ref.descend(d, NEED, cost, starts, room)


# ------------------------------------------------------------------------------------------------
# sight
# ------------------------------------------------------------------------------------------------
@gpu
def test_sight_all_ordered_pairs_of_a_small_volume():
    """every direction and sign, every tie through an edge and a corner that fits in 7 x 6 x 5"""
    d = random_volume((7, 6, 5), 0.2, 1)
    a, b, cover, blocked = ref.sight_all_pairs(d, NEED)
    assert len(a) == 44100 and (blocked > 0).sum() > 10000 and (blocked == 0).sum() > 3000
    check_sight(d, NEED, a, b, seed=1, want=(cover, blocked))
    # symmetric in a and b
    back = c_sight(d, NEED, b, a, seed=2)
    assert np.array_equal(back[0], cover) and np.array_equal(back[1], blocked)


@gpu
def test_sight_random_segments():
    dims = (40, 36, 44)
    d = random_volume(dims, 0.05, 2)
    rng = np.random.default_rng(3)
    a = rng.integers(0, dims, size=(4096, 3))
    b = np.clip(a + rng.integers(-14, 15, size=(4096, 3)), 0, np.array(dims) - 1)
    b[:512] = rng.integers(0, dims, size=(512, 3))              # and long ones, across the whole volume
    cover, blocked = check_sight(d, NEED, a, b, seed=3)
    assert (blocked == 0).sum() > 400 and (blocked > 0).sum() > 400 and cover.max() > 60


@gpu
@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 1, 37), (19, 8, 9), (17, 23, 5)])
def test_sight_shapes(dims):
    d = random_volume(dims, 0.15 if max(dims) > 1 else 0.0, sum(dims))
    rng = np.random.default_rng(sum(dims))
    a, b = rng.integers(0, dims, size=(300, 3)), rng.integers(0, dims, size=(300, 3))
    a[:4] = b[:4]                                               # a == b: the cell itself
    cover, blocked = check_sight(d, NEED, a, b, seed=dims[2])
    assert (cover[:4] == 1).all() and np.array_equal(blocked[:4], (d[tuple(a[:4].T)] < NEED).astype(np.int32))


@gpu
def test_sight_at_the_largest_dimension_stays_in_int32():
    d = np.full((1024, 3, 2), OPEN, np.int32)
    d[500, 1, 0] = d[511, 1, 0] = d[512, 1, 1] = d[1000, 0, 0] = SHUT
    a = [(0, 0, 0), (1023, 2, 1), (0, 0, 0), (0, 2, 1)]
    b = [(1023, 2, 1), (0, 0, 0), (1023, 0, 0), (1023, 0, 0)]
    cover, blocked = check_sight(d, NEED, a, b, seed=1)
    # 1023, 2, 1: y crosses at t = 1/4 and 3/4, z at 1/2, and so does x (k = 511 of its 1023 crossings, at
    # 1023 / 2046): one tie of two axes, 1 + 1026 + 1 cells; the products there are 1023 * 1 against 1 * 1023
    assert cover.tolist() == [1028, 1028, 1024, 1028] and blocked[2] == 1 and blocked[0] == blocked[1]


@gpu
def test_sight_ends_outside_the_volume_and_no_segments():
    dims = (19, 8, 9)
    d = random_volume(dims, 0.1, 4)
    a = [(-1, 0, 0), (0, 0, 0), (0, 8, 0), (3, 3, 3), (19, 0, 0), (2 ** 31 - 1, 0, 0), (-2 ** 31, -2 ** 31, -2 ** 31),
         (3, 3, 3), (0, 0, -1)]
    b = [(3, 3, 3), (0, 0, 9), (1, 1, 1), (3, 3, 3), (18, 7, 8), (0, 0, 0), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1),
         (18, 7, 8), (0, 0, -1)]
    cover, blocked = check_sight(d, NEED, a, b, seed=1)
    assert cover.tolist()[:3] == [0, 0, 0] and blocked.tolist()[:3] == [-1, -1, -1] and cover[3] == 1
    assert (cover[[4, 5, 6, 8]] == 0).all() and (blocked[[4, 5, 6, 8]] == -1).all() and cover[7] > 15
    c_sight(d, NEED, np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32), seed=2)      # S == 0: nothing is written


@gpu
def test_sight_need_zero_and_a_need_no_cell_meets():
    dims = (17, 23, 5)
    d = random_volume(dims, 0.3, 6)
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, dims, size=(200, 3)), rng.integers(0, dims, size=(200, 3))
    cover, blocked = check_sight(d, 0, a, b, seed=1)                       # every cell is free
    assert (blocked == 0).all()
    shut = check_sight(d, OPEN + 1, a, b, seed=2)                          # no cell is
    assert np.array_equal(shut[0], cover) and np.array_equal(shut[1], cover)
    d[:] = FAR
    assert (check_sight(d, FAR, a, b, seed=3)[1] == 0).all()               # need at its upper end


# ------------------------------------------------------------------------------------------------
# shortcut: structure
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def door_paths():
    d = ref.wall_and_door()
    starts = [(2, 3, 40), (5, 30, 4), (1, 17, 21), (35, 2, 2), (19, 17, 21), (38, 30, 40), (20, 0, 0), (-1, 5, 5)]
    d[38, 30, 40] = OPEN
    for s in starts[:6]:
        d[s] = OPEN
    cells, length = descended(d, (38, 30, 40), starts, 96)
    assert length[:5].min() > 1 and length[5] == 1 and (length[6:] == 0).all() and length.max() <= 96
    for v in (d, cells, length):
        v.setflags(write=False)
    return d, cells, length


@gpu
@pytest.mark.parametrize("window", [1, 5, 96, 1 << 26])
def test_shortcut_wall_and_door_volume(window):
    d, cells, length = door_paths()
    keep, count, blocked = check_shortcut(d, NEED, cells, length, window, seed=window % 7)
    assert (blocked == 0).all() and count[5] == 1 and (count[6:] == 0).all() and (keep[6:] == -1).all()
    if window == 1:                                             # the path itself
        for p in range(6):
            assert count[p] == length[p] and np.array_equal(keep[p, :length[p]], np.arange(length[p]))
    if window >= 96:
        assert (count[:3] <= 6).all() and (count[:5] < length[:5]).all()
        for p in range(5):
            assert ref.kept_length(cells[p], keep[p], count[p]) <= ref.polyline_length(cells[p, :length[p]]) + 1e-12


@gpu
def test_shortcut_on_the_empty_volume_keeps_the_two_ends():
    d = np.full((19, 8, 9), OPEN, np.int32)
    cells, length = descended(d, (18, 7, 8), [(0, 0, 0), (3, 7, 0), (18, 7, 8), (18, 0, 8), (9, 4, 4)], 24)
    keep, count, blocked = check_shortcut(d, NEED, cells, length, 24, seed=1)
    assert count.tolist() == [2, 2, 1, 2, 2] and (blocked == 0).all()
    assert (keep[:, 0] == 0).all() and np.array_equal(keep[:, 1], length - 1)


@functools.lru_cache(maxsize=None)
def serpentine_paths():
    """Paths of exactly 2, 64, 65, 66, 128, 129 cells (either side of a wave of 64 candidates) and 255, 256, 257, 258
    cells (either side of the kernel's chunk of 256) through a serpentine: walls y == 3, 6, ... open at alternating
    ends of x.  The last n cells of a descended path are the descended path of their first cell."""
    dims = (12, 82, 1)
    d = np.full(dims, OPEN, np.int32)
    for i, y in enumerate(range(3, 82, 3)):
        d[:, y] = SHUT
        if i % 2 == 0:
            d[10:, y] = OPEN
        else:
            d[:2, y] = OPEN
    whole, n = descended(d, (0, 0, 0), [(0, 80, 0)], 600)
    n = int(n[0])
    assert 258 < n <= 600
    sizes = (2, 64, 65, 66, 128, 129, 255, 256, 257, 258)
    cells, length = descended(d, (0, 0, 0), [whole[0, n - k] for k in sizes], 258)
    assert length.tolist() == list(sizes)
    for v in (d, cells, length):
        v.setflags(write=False)
    return d, cells, length


@gpu
@pytest.mark.parametrize("window", [1, 63, 64, 65, 129, 255, 256, 257, 258])
def test_shortcut_path_lengths_and_windows_either_side_of_a_wave_and_of_a_chunk(window):
    d, cells, length = serpentine_paths()
    keep, count, blocked = check_shortcut(d, NEED, cells, length, window, seed=window)
    assert (blocked == 0).all() and count[0] == 2
    if window == 1:
        assert np.array_equal(count, length)
    else:
        assert (count[1:] < length[1:]).all() and (count[1:] > 4).all()      # the lanes' turns stay
    # the shorter paths with the window their own length, one path per call: other grids, other padding
    for p in range(6):
        n = int(length[p])
        check_shortcut(d, NEED, cells[p:p + 1, :n], length[p:p + 1], n, seed=p)


@gpu
@pytest.mark.parametrize("n,clear_at,window", [(520, 400, 520), (520, 100, 520), (520, 264, 519), (520, 263, 519),
                                                (520, 327, 519), (520, 328, 519), (520, 3, 519), (700, 5, 699),
                                                (300, 2, 257), (300, 1, 257),
                                                (130, 100, 130), (130, 30, 130), (130, 66, 129), (130, 65, 129),
                                                (200, 3, 199), (70, 2, 65), (70, 1, 65)])
def test_shortcut_takes_the_farthest_clear_cell_beyond_nearer_blocked_ones(n, clear_at, window):
    """Sight from row 0 is not monotone: only row clear_at is in sight, nearer and farther rows are not.  The kernel
    scans the candidates in chunks of 256 (four waves of 64) from the far end of the window.  With 520 rows and
    window 519 the chunks from row 0 are rows 264..519, 8..263 and 1..7: the clear row falls into the first chunk
    (400), into the second (100), on either side of the boundary between them (264, 263), on either side of the
    boundary between the first chunk's first two waves (327, 328), into the third chunk (3) and, with 700 rows, into
    the third as well (5); with 300 rows and window 257 on the lowest lane of the first chunk (rows 2..257) and on
    the only live lane of a second one (row 1 alone).  The cases around 64 stay: they fall on the waves' edges."""
    d, cells = ref.comb(n, clear_at)
    keep, count, blocked = check_shortcut(d, NEED, cells, [n], window, seed=clear_at)
    assert keep[0, :3].tolist() == [0, clear_at, clear_at + 1] and blocked[0] == 1


@gpu
@pytest.mark.parametrize("first,second", [(400, 300), (400, 280), (327, 328), (263, 264), (100, 400), (10, 5)])
def test_shortcut_two_cells_in_sight_in_different_waves_or_chunks(first, second):
    """two rows in sight from row 0, in different waves of a chunk or in different chunks: the larger is kept"""
    d, cells = ref.comb(520, first)
    cells[0, second] = (second, 0, 0)
    keep, count, blocked = check_shortcut(d, NEED, cells, [520], 519, seed=first)
    assert keep[0, 1] == max(first, second)


# ------------------------------------------------------------------------------------------------
# shortcut: random fields
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("density", [0.15, 0.3])
def test_shortcut_random_obstacle_fields(density):
    dims = (40, 36, 44)
    d = random_volume(dims, density, int(density * 100))
    d[20, 18, 22] = OPEN
    cost, _ = route_ref.route(d, NEED, [(20, 18, 22)])
    rng = np.random.default_rng(5)
    reach = np.argwhere(cost < FAR)
    starts = reach[rng.choice(len(reach), 64, replace=False)]
    cells, length = route_ref.descend(d, NEED, cost, starts, 96)
    assert length.min() >= 1 and length.max() <= 96 and (length > 12).sum() > 20
    for window in (96, 6):
        keep, count, blocked = check_shortcut(d, NEED, cells, length, window, seed=window)
        assert (blocked == 0).all() and (count <= length).all()
    assert (count < length).sum() > 30


# ------------------------------------------------------------------------------------------------
# shortcut: path handling
# ------------------------------------------------------------------------------------------------
@gpu
def test_shortcut_cut_paths_empty_paths_and_padding_rows():
    d, cells, length = door_paths()
    longest = int(length.max())
    # room for less than the longest path: n = max_cells, the last kept row is max_cells - 1
    for room in (longest - 1, 17, 1):
        cut = np.ascontiguousarray(cells[:, :room])
        keep, count, blocked = check_shortcut(d, NEED, cut, length, 96, seed=room)
        full = length >= room
        assert (keep[full, -1] == room - 1).all() and (count[full] >= 1).all() and (blocked == 0).all()
    # lengths of 0, below 0 and 1, whatever the rows hold
    n = np.array([0, -5, 1, 1, 0, 1, 0, 0], np.int32)
    keep, count, blocked = check_shortcut(d, NEED, cells, n, 96, seed=3)
    assert count.tolist() == [0, 0, 1, 1, 0, 1, 0, 0] and (keep[n <= 0] == -1).all() and (keep[n == 1] == 0).all()
    # padding rows repeat n - 1
    keep, count, _ = check_shortcut(d, NEED, cells, length, 96, seed=4)
    for p in range(5):
        assert (keep[p, count[p]:] == length[p] - 1).all() and keep[p, count[p] - 1] == length[p] - 1
    # P == 0: nothing is written
    got = c_shortcut(d, NEED, np.zeros((0, 8, 3), np.int32), np.zeros(0, np.int32), 8, seed=5)
    assert got[0].shape == (0, 8)


@gpu
def test_shortcut_counts_kept_segments_that_are_not_clear():
    d = np.full((12, 10, 6), OPEN, np.int32)
    d[5, :, :] = SHUT                                                      # a wall with no door
    path = [(1, 1, 1), (2, 1, 1), (3, 2, 1), (4, 2, 1), (6, 2, 1), (7, 2, 2), (8, 2, 2), (8, 20, 2), (8, 3, 2),
            (9, 3, 2)]                                                     # jumps the wall, then leaves the volume
    rows = lambda *c: list(c) + [c[-1]] * (12 - len(c))
    cells = np.array([rows(*path), rows((1, 1, 1)), rows((5, 5, 5), (5, 6, 5)), rows((1, 1, 1), (1, 50, 1)),
                      rows((1, -1, 1), (1, 1, 1), (2, 1, 1))], np.int32)
    length = np.array([len(path), 4, 2, 2, 3], np.int32)
    keep, count, blocked = check_shortcut(d, NEED, cells, length, 12, seed=1)
    assert blocked[0] == 1 and keep[0, :count[0]].tolist() == [0, 3, 4, 9] and (keep[0, count[0]:] == 9).all()
    assert keep[1, :2].tolist() == [0, 3] and count[1] == 2 and blocked[1] == 0     # a path that stands still
    assert count[2] == 2 and blocked[2] == 1                               # both cells shut
    assert keep[3, :2].tolist() == [0, 1] and blocked[3] == 1              # ends outside the volume
    assert keep[4, :count[4]].tolist() == [0, 1, 2] and blocked[4] == 1    # starts outside: nothing is in sight


@gpu
def test_shortcut_twice_gives_the_same_bytes():
    d, cells, length = door_paths()
    a = c_shortcut(d, NEED, cells, length, 96, seed=1)
    b = c_shortcut(d, NEED, cells, length, 96, seed=2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    s = [np.array(v, np.int32) for v in ([(0, 0, 0), (39, 35, 43)], [(39, 0, 43), (0, 35, 0)])]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(c_sight(d, NEED, *s, seed=1), c_sight(d, NEED, *s, seed=2)))


# ------------------------------------------------------------------------------------------------
# through the Python API
# ------------------------------------------------------------------------------------------------
H = 0.01
BOX = ((0.0, 0.0, 0.0), (0.64, 0.48, 0.40))


def _blob(lo, hi, dev, step=0.005):
    """Gaussians of sigma 4 mm on a lattice that fills the box lo..hi: (means, rot, scales, weights)"""
    ax = [torch.arange(lo[a], hi[a] + 1e-9, step, dtype=torch.float64) for a in range(3)]
    m = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3).float().to(dev)
    n = m.shape[0]
    rot = torch.eye(3, device=dev).reshape(1, 9).repeat(n, 1).contiguous()
    return m.contiguous(), rot, torch.full((n, 3), 0.004, device=dev), torch.full((n,), 0.9, device=dev)


def _pose(yaw, t):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([c, -s, 0, s, c, 0, 0, 0, 1, *t], np.float32)


@gpu
def test_plan_transit_with_shortcut_goes_round_the_wall_in_a_few_straight_pieces():
    from gaussiangrasper_amd import field, transit
    from gaussiangrasper_amd.grasp import default_gripper
    dev = torch.device(DEV)
    f = field.DistanceField(*BOX, voxel=H, device=dev)
    f.add(_blob((0.0, 0.0, 0.0), (0.64, 0.48, 0.02), dev))             # the table
    f.add(_blob((0.30, 0.0, 0.02), (0.33, 0.30, 0.40), dev))           # the wall, open beyond y = 0.30
    f.update()
    radius = 0.01
    spheres = field.gripper_spheres(default_gripper(), 0.06, 0.02, 0.02, radius)
    carried = transit.carried_spheres(np.random.default_rng(0).uniform(-0.015, 0.015, (500, 3)) + [0.03, 0, 0], radius)
    spheres = np.concatenate([spheres, carried])
    goal = _pose(0.3, (0.52, 0.12, 0.22))
    starts = np.stack([_pose(0.0, (0.12, 0.12, 0.22)), _pose(1.2, (0.10, 0.20, 0.25))])
    straight = np.linalg.norm(starts[:, 9:].astype(np.float64) - goal[9:].astype(np.float64), axis=1)
    plans = {}
    for steps in (9, 64, 997):
        plan = transit.plan_transit(f, starts, goal, spheres, radius, steps=steps, shortcut=True)
        assert plan.poses.shape == (2, steps, 12) and plan.planned.all()
        # the dense resampling is the check that the path is safe between the kept cells too
        assert bool(plan.clearance.clear.all()) and int(plan.clearance.slack.min()) >= 0, plan.clearance.first_hit
        count, length = plan.count.cpu().numpy(), plan.length.cpu().numpy()
        assert (count < length).all() and (count >= 2).all()
        assert (plan.euclid < plan.cost).all() and (plan.euclid >= straight).all()
        p = plan.poses.cpu().numpy()
        assert np.array_equal(p[:, 0], starts) and np.array_equal(p[:, -1], np.stack([goal, goal]))
        assert plan.best == int(np.argmin(plan.euclid))
        plans[steps] = plan
    # keep and count against the restatement on the plan's own cells
    plan = plans[64]
    d = f.dist2.cpu().numpy()
    cells, length = plan.cells.cpu().numpy(), plan.length.cpu().numpy()
    keep, count, blocked = ref.shortcut(d, plan.cost_to_go.need, cells, length, cells.shape[1])
    assert np.array_equal(plan.keep.cpu().numpy(), keep) and np.array_equal(plan.count.cpu().numpy(), count)
    assert (blocked == 0).all() and (count <= 8).all(), count
    # euclid is the length of the line the poses follow
    for i in range(2):
        line = np.concatenate([starts[i:i + 1, 9:], transit.cell_centres(f, cells[i][keep[i, :count[i]]]), goal[None, 9:]])
        assert plan.euclid[i] == pytest.approx(ref.polyline_length(line), rel=1e-12)
    # a window: more cells kept, still clear; the pieces through the Python layer
    near = transit.plan_transit(f, starts, goal, spheres, radius, steps=64, shortcut=True, window=4)
    assert (near.count.cpu().numpy() > count).all() and bool(near.clearance.clear.all())
    assert np.array_equal(near.keep.cpu().numpy(), ref.shortcut(d, plan.cost_to_go.need, cells, length, 4)[0])
    pulled = transit.shortcut(plan.cost_to_go, plan.cells, plan.length)
    assert np.array_equal(pulled.keep.cpu().numpy(), keep) and int(pulled.blocked.sum()) == 0
    kept = pulled.cells.cpu().numpy()
    for i in range(2):
        assert np.array_equal(kept[i, :count[i]], cells[i][keep[i, :count[i]]])
        assert (kept[i, count[i]:] == cells[i, length[i] - 1]).all()
    # line_of_sight for scene points: across the wall no, along its side yes, outside the volume no
    a = np.array([[0.12, 0.12, 0.22], [0.12, 0.12, 0.22], [0.12, 0.12, 0.22]])
    b = np.array([[0.52, 0.12, 0.22], [0.12, 0.40, 0.30], [0.12, 0.12, 0.50]])
    r = transit.planning_radius(spheres, radius, f.h)
    seen = transit.line_of_sight(f, a, b, r)
    assert seen.dtype == torch.bool and seen.cpu().tolist() == [False, True, False]
    cov, blk = transit.sight(f.dist2, f.dims, plan.cost_to_go.need, transit.cells_of(f, a), transit.cells_of(f, b))
    want = ref.sight(d, plan.cost_to_go.need, transit.cells_of(f, a), transit.cells_of(f, b))
    assert np.array_equal(cov.cpu().numpy(), want[0]) and np.array_equal(blk.cpu().numpy(), want[1])
    # shortcut=False is what it was: the poses through every cell, best by the chamfer cost, no keep
    plain = transit.plan_transit(f, starts, goal, spheres, radius, steps=64)
    every = np.stack([transit.transit_poses(starts[i], goal, cells[i], length[i], f, 64) for i in range(2)])
    assert np.array_equal(plain.poses.cpu().numpy(), every) and plain.keep is None and plain.count is None
    assert plain.best == int(np.argmin(plain.cost)) and np.array_equal(plain.cost, plan.cost)
    assert np.array_equal(plain.cells.cpu().numpy(), cells) and (plain.euclid > plan.euclid).all()
    assert not np.array_equal(plain.poses.cpu().numpy(), plan.poses.cpu().numpy())
    # no path: nothing to pull
    none = transit.plan_transit(f, starts, _pose(0.0, (0.315, 0.15, 0.2)), spheres, radius, steps=16, shortcut=True)
    assert none.best == -1 and not none.planned.any() and np.isinf(none.euclid).all()
    assert (none.count.cpu().numpy() == 0).all() and (none.keep.cpu().numpy() == -1).all()


@gpu
def test_command_line_with_shortcut_from_a_saved_field(tmp_path, capsys):
    from gaussiangrasper_amd import field, transit
    dev = torch.device(DEV)
    f = field.DistanceField(*BOX, voxel=H, device=dev)
    f.mass[:, :, :2] = field.VOTE_ONE                                  # the table
    f.mass[30:33, :30, 2:] = field.VOTE_ONE                            # the wall, open beyond y = 0.30
    f.update()
    f.save(str(tmp_path / "field.npz"))
    starts = np.stack([_pose(0.0, (0.12, 0.12, 0.22)), _pose(1.2, (0.10, 0.20, 0.25))])
    np.save(tmp_path / "from.npy", starts)
    np.save(tmp_path / "to.npy", _pose(0.3, (0.52, 0.12, 0.22)))
    base = ["--field", str(tmp_path / "field.npz"), "--from", str(tmp_path / "from.npy"), "--to",
            str(tmp_path / "to.npy"), "--gripper", "default", "--width", "0.06", "--radius", "0.01", "--steps", "32"]
    rc = transit.main(base + ["--shortcut", "--out", str(tmp_path / "paths.npy"), "--report", str(tmp_path / "r.npz")])
    out = capsys.readouterr().out
    assert rc == 0 and "2 of 2 starts have a path, 2 clear" in out and "kept cells" in out
    rc = transit.main(base + ["--shortcut", "--window", "5", "--out", str(tmp_path / "near.npy"), "--report",
                              str(tmp_path / "near.npz")])
    assert rc == 0
    paths = np.load(tmp_path / "paths.npy")
    assert paths.dtype == np.float32 and paths.shape == (2, 32, 12) and np.array_equal(paths[:, 0], starts)
    with np.load(tmp_path / "r.npz") as z, np.load(tmp_path / "near.npz") as w:
        assert {"keep", "count", "euclid", "cost", "length", "clear", "best"} <= set(z.files)
        assert z["clear"].all() and z["planned"].all() and (z["slack"] >= 0).all()
        assert z["keep"].shape[0] == 2 and (z["count"] < z["length"]).all() and (z["euclid"] < z["cost"]).all()
        assert int(z["best"]) == int(np.argmin(z["euclid"]))
        assert (w["count"] > z["count"]).all() and w["clear"].all() and np.isfinite(w["euclid"]).all()
