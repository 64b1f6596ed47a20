"""GPU checks of transit planning (gg_field_route, gg_field_descend and gaussiangrasper_amd.transit) against the
restatement (tests/route_ref.py).  Everything is held to equality; the C calls' arrays are carved from the sentinel
arena (tests/arena.py) and compared whole."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import route_ref as ref
from arena import Arena

gpu = pytest.mark.gpu
DEV = "cuda:0"
FAR = ref.FAR
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEED = 4
OPEN, SHUT = 100, 0                                # dist2 of a cell that is free / not free at NEED
NOT_CONVERGED = -5                                 # GG_ERR_NOT_CONVERGED
SHAPES = [(1, 1, 1), (1, 1, 37), (19, 8, 9), (17, 23, 5), (40, 36, 44)]


def _define(name):
    src = open(os.path.join(ROOT, "gaussiangrasper_amd", "csrc", "field.hip")).read()
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, src, flags=re.M)
    assert m, f"#define {name} not found in field.hip"
    return int(m.group(1))


FR_BATCH, FR_BRICK = _define("FR_BATCH"), _define("FR_BRICK")


def _lib():
    from gaussiangrasper_amd import _lib as L
    return L.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def c_route(dist2, need, goals, max_rounds=4096, seed=0, expect=0):
    """gg_field_route on a sentinel arena -> (cost, ignored, rounds)"""
    dist2 = np.asarray(dist2, np.int32)
    goals = np.asarray(goals, np.int32).reshape(-1, 3)
    dims = dist2.shape
    d = (ctypes.c_int32 * 3)(*dims)
    need_ws = _lib().gg_field_route_workspace(d)
    assert need_ws > 0 and need_ws % 256 == 0
    a = Arena(DEV, seed)
    a.carve("dist2", dist2, 4, "in")
    if len(goals):
        a.carve("goals", goals, 4, "in")
    a.carve("cost", np.zeros(dims, np.int32), 4, "out")
    a.carve("ignored", np.zeros(1, np.int64), 8, "out")
    a.carve("ws", int(need_ws), 256, "ws")
    rounds = ctypes.c_int(-1)
    st = _lib().gg_field_route(d, a.ptr("dist2"), int(need), len(goals), a.ptr("goals") if len(goals) else None,
                               a.ptr("cost"), a.ptr("ignored"), int(max_rounds), ctypes.byref(rounds), a.ptr("ws"),
                               ctypes.c_size_t(need_ws), _stream())
    assert st == expect, (st, _lib().gg_last_error())
    torch.cuda.synchronize()
    out = a.check()
    return out["cost"], int(out["ignored"][0]), int(rounds.value)


def c_descend(dist2, need, cost, starts, max_cells, seed=0):
    dist2, cost = np.asarray(dist2, np.int32), np.asarray(cost, np.int32)
    starts = np.asarray(starts, np.int32).reshape(-1, 3)
    P = len(starts)
    a = Arena(DEV, seed)
    a.carve("dist2", dist2, 4, "in")
    a.carve("cost", cost, 4, "in")
    if P:
        a.carve("starts", starts, 4, "in")
    a.carve("cells", np.zeros((P, max_cells, 3), np.int32), 4, "out")
    a.carve("length", np.zeros(P, np.int32), 4, "out")
    st = _lib().gg_field_descend((ctypes.c_int32 * 3)(*dist2.shape), a.ptr("dist2"), int(need), a.ptr("cost"), P,
                                 a.ptr("starts") if P else None, int(max_cells), a.ptr("cells"), a.ptr("length"),
                                 _stream())
    assert st == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    if P == 0:
        assert a.untouched()
        return np.zeros((0, max_cells, 3), np.int32), np.zeros(0, np.int32)
    out = a.check()
    return out["cells"], out["length"]


def check_route(dist2, need, goals, seed=0, **kw):
    want, ignored = ref.route(dist2, need, goals)
    got, got_ignored, rounds = c_route(dist2, need, goals, seed=seed, **kw)
    assert got.dtype == np.int32 and np.array_equal(got, want), \
        f"{int((got != want).sum())} cells differ, the first at {np.argwhere(got != want)[:1].tolist()}"
    assert got_ignored == ignored
    return want, ignored, rounds


def random_volume(dims, density, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(dims) < density, SHUT, OPEN).astype(np.int32)


# ------------------------------------------------------------------------------------------------
# route: shapes and goals
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dims", SHAPES)
@pytest.mark.parametrize("goals", ["corner", "several"])
def test_route_shapes_against_the_restatement(dims, goals):
    """one cell, one line, partial bricks on every axis, and several bricks per axis"""
    assert FR_BRICK == 8, "the shapes were chosen around bricks of 8 cells"
    d = random_volume(dims, 0.12 if max(dims) > 1 else 0.0, sum(dims))
    last = tuple(n - 1 for n in dims)
    d[0, 0, 0] = d[last] = OPEN
    g = [(0, 0, 0)] if goals == "corner" else [last, (dims[0] // 2, dims[1] // 2, dims[2] // 2), (0, 0, 0), last]
    want, ignored, rounds = check_route(d, NEED, g, seed=len(g))
    assert want[0, 0, 0] == 0 and rounds >= 1
    assert ignored == sum(1 for c in g if d[tuple(c)] < NEED)


@gpu
def test_route_goals_that_take_no_part_are_counted():
    dims = (19, 8, 9)
    d = random_volume(dims, 0.1, 5)
    d[3, 3, 3], d[4, 4, 4], d[18, 7, 8] = OPEN, SHUT, OPEN
    g = [(3, 3, 3), (4, 4, 4), (-1, 0, 0), (0, 8, 0), (0, 0, 9), (19, 0, 0), (3, 3, 3), (18, 7, 8), (2 ** 30, 0, 0),
         (-2 ** 31, -2 ** 31, -2 ** 31)]
    want, ignored, _ = check_route(d, NEED, g, seed=1)
    assert ignored == 7 and want[3, 3, 3] == 0 and want[18, 7, 8] == 0 and want[4, 4, 4] == FAR
    # every goal ignored, and no goal at all: FAR everywhere
    want, ignored, _ = check_route(d, NEED, [(4, 4, 4), (0, 0, -1)], seed=2)
    assert ignored == 2 and (want == FAR).all()
    want, ignored, rounds = check_route(d, NEED, np.zeros((0, 3), np.int32), seed=3)
    assert ignored == 0 and (want == FAR).all() and rounds == 0


@gpu
def test_route_need_zero_and_a_need_no_cell_meets():
    dims = (17, 23, 5)
    d = random_volume(dims, 0.3, 6)
    want, ignored, _ = check_route(d, 0, [(16, 22, 4)], seed=1)             # every cell is free
    assert ignored == 0 and (want < FAR).all()
    want, ignored, _ = check_route(d, OPEN + 1, [(16, 22, 4), (0, 0, 0)], seed=2)
    assert ignored == 2 and (want == FAR).all()
    d[:] = FAR
    want, _, _ = check_route(d, FAR, [(0, 0, 0)], seed=3)                   # need at its upper end
    assert want.max() == 5 * 4 + 4 * 12 + 3 * 6


# ------------------------------------------------------------------------------------------------
# route: walls and the block rule
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("wall,door", [(12, (7, 3)), (12, (7, 8)), (8, (7, 16)), (7, (8, 15)), (12, (3, 3))],
                         ids=["face", "edge", "corner", "corner-low", "inside"])
def test_route_through_a_one_cell_door(wall, door):
    """the only way through the wall x == wall is one cell, on a brick face, edge or corner (or inside a brick)"""
    dims = (24, 20, 20)
    d = np.full(dims, OPEN, np.int32)
    d[wall] = SHUT
    d[(wall,) + door] = OPEN
    want, _, rounds = check_route(d, NEED, [(1, 2, 3)], seed=wall)
    far_side = want[wall + 1:]
    assert (far_side < FAR).all() and want[(wall,) + door] < far_side.min() and rounds >= 3
    # through the door only straight: the cells next to it on either side differ by 3
    assert want[(wall + 1,) + door] - want[(wall - 1,) + door] == 6
    d[(wall,) + door] = SHUT
    want, _, _ = check_route(d, NEED, [(1, 2, 3)], seed=wall + 1)
    assert (want[wall:] == FAR).all()


@gpu
@pytest.mark.parametrize("at", [3, 7, 15], ids=["inside", "across", "across-second"])
def test_route_does_not_squeeze_between_cells_that_touch_by_an_edge(at):
    """x == at blocked for y <= at, x == at + 1 blocked for y > at: the two walls touch along the edges (at, at, z) /
    (at + 1, at + 1, z) only, and the diagonal between them is the one way through that the block rule shuts"""
    dims = (24, 24, 10)
    d = np.full(dims, OPEN, np.int32)
    d[at, :at + 1] = SHUT
    d[at + 1, at + 1:] = SHUT
    want, _, _ = check_route(d, NEED, [(0, 0, 0)], seed=at)
    assert want[at, at + 1, 4] < FAR and want[at + 1, at, 4] == FAR and (want[at + 2:] == FAR).all()
    d[at, at, 5] = OPEN                                     # one cell of the edge opened: a way through
    want, _, _ = check_route(d, NEED, [(0, 0, 0)], seed=at + 1)
    assert (want[at + 2:] < FAR).all()


@gpu
@pytest.mark.parametrize("p", [3, 7], ids=["inside", "across"])
def test_route_does_not_squeeze_between_cells_that_touch_by_a_corner(p):
    dims = (16, 16, 16)
    d = np.full(dims, OPEN, np.int32)
    d[p, p, p] = d[p + 1, p + 1, p + 1] = SHUT
    want, _, _ = check_route(d, NEED, [(p + 1, p + 1, p)], seed=p)
    assert want[p, p, p + 1] == 9                           # 5 if the diagonal past both corners were allowed
    d[p, p, p] = OPEN
    want, _, _ = check_route(d, NEED, [(p + 1, p + 1, p)], seed=p + 1)
    assert want[p, p, p + 1] == 7                           # one blocked cell of the eight is enough: 4 + 3
    d[p + 1, p + 1, p + 1] = OPEN
    want, _, _ = check_route(d, NEED, [(p + 1, p + 1, p)], seed=p + 2)
    assert want[p, p, p + 1] == 5


@gpu
def test_route_leaves_a_sealed_pocket_at_far():
    dims = (24, 20, 20)
    d = np.full(dims, OPEN, np.int32)
    d[5:13, 5:13, 5:13] = SHUT
    d[6:12, 6:12, 6:12] = OPEN                              # the pocket: across the brick boundary at 8
    want, _, _ = check_route(d, NEED, [(0, 0, 0)], seed=1)
    assert (want[6:12, 6:12, 6:12] == FAR).all() and (want[d == OPEN] < FAR).sum() == (d == OPEN).sum() - 6 ** 3
    want, _, _ = check_route(d, NEED, [(7, 7, 7)], seed=2)  # and from inside: nothing outside is reached
    assert (want < FAR).sum() == 6 ** 3
    cells, length = c_descend(d, NEED, want, [(0, 0, 0), (8, 8, 8)], 16)
    assert length.tolist() == [0, 2] and (cells[0] == -1).all()


# ------------------------------------------------------------------------------------------------
# route: many rounds
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def serpentine():
    """5 x 5 x 2 bricks; walls y == 4, 8, ..., 36 open at alternating ends of x: ten lanes of four bricks' faces"""
    dims = (40, 40, 16)
    d = np.full(dims, OPEN, np.int32)
    for i, y in enumerate(range(4, 40, 4)):
        d[:, y] = SHUT
        if i % 2 == 0:
            d[37:, y] = OPEN
        else:
            d[:3, y] = OPEN
    want, _ = ref.route(d, NEED, [(0, 0, 0)])
    d.setflags(write=False)
    want.setflags(write=False)
    return d, want


@gpu
def test_route_serpentine_takes_more_than_one_batch_of_rounds():
    d, want = serpentine()
    path, n = ref.descend(d, NEED, want, [(39, 39, 15)], 1024)
    crossings = int((np.diff(path[0, :n[0]] // FR_BRICK, axis=0) != 0).any(1).sum())
    assert crossings > 2 * FR_BATCH, crossings                           # on the CPU side: the case is what it says
    got, ignored, rounds = c_route(d, NEED, [(0, 0, 0)], seed=1)
    assert np.array_equal(got, want) and ignored == 0
    assert rounds > FR_BATCH, rounds                                      # the batch loop read back more than once
    assert rounds <= 4096


@gpu
def test_route_says_so_when_max_rounds_run_out():
    d, want = serpentine()
    got, _, rounds = c_route(d, NEED, [(0, 0, 0)], max_rounds=FR_BATCH + 1, seed=2, expect=NOT_CONVERGED)
    msg = _lib().gg_last_error()
    assert b"gg_field_route" in msg and b"max_rounds" in msg and b"upper bounds" in msg
    assert rounds == FR_BATCH + 1
    # valid upper bounds: nothing below the true cost, the goal's side done, the far end not reached yet
    assert (got >= want).all() and got[0, 0, 0] == 0 and np.array_equal(got[:, :4], want[:, :4])
    assert got[39, 39, 15] == FAR
    for limit in (1, FR_BATCH):
        c_route(d, NEED, [(0, 0, 0)], max_rounds=limit, seed=3, expect=NOT_CONVERGED)


# ------------------------------------------------------------------------------------------------
# route: random obstacle fields, repeatability
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("density", [0.15, 0.3, 0.45])
def test_route_random_obstacle_fields(density):
    dims = (40, 36, 44)
    d = random_volume(dims, density, int(density * 100))
    rng = np.random.default_rng(1)
    free = np.argwhere(d >= NEED)
    g = free[rng.choice(len(free), 6, replace=False)]
    want, _, _ = check_route(d, NEED, g, seed=1)
    reach = want < FAR
    assert reach.sum() > 100 and ((d >= NEED) & ~reach).sum() > 0, "the case must have both kinds of free cells"


@gpu
def test_route_twice_gives_the_same_bytes():
    d = random_volume((40, 36, 44), 0.25, 11)
    d[0, 0, 0] = d[39, 35, 43] = OPEN
    a = c_route(d, NEED, [(0, 0, 0), (39, 35, 43)], seed=1)
    b = c_route(d, NEED, [(0, 0, 0), (39, 35, 43)], seed=2)            # another workspace content
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]


# ------------------------------------------------------------------------------------------------
# descent
# ------------------------------------------------------------------------------------------------
@gpu
def test_descend_ties_on_the_empty_volume():
    """in an empty volume most cells have several moves that fit: the lowest move number is taken"""
    dims = (19, 8, 9)
    d = np.full(dims, FAR, np.int32)
    want, _, _ = check_route(d, NEED, [(9, 4, 4)], seed=1)
    starts = np.stack(np.meshgrid(*[np.arange(-1, n + 1, 2) for n in dims], indexing="ij"), -1).reshape(-1, 3)
    cells, length = ref.descend(d, NEED, want, starts, 24)
    got = c_descend(d, NEED, want, starts, 24, seed=2)
    assert np.array_equal(got[0], cells) and np.array_equal(got[1], length)
    assert (length == 0).sum() > 10 and (length > 5).sum() > 50 and length.max() <= 24
    assert len(starts) % 4 != 0 or len(starts) > 256       # several workgroups of four paths


@gpu
def test_descend_starts_that_have_no_path_and_padding_rows():
    dims = (24, 20, 20)
    d = np.full(dims, OPEN, np.int32)
    d[5:13, 5:13, 5:13] = SHUT
    d[6:12, 6:12, 6:12] = OPEN
    goal = (20, 3, 17)
    want, _ = ref.route(d, NEED, [goal])
    starts = [goal, (5, 5, 5), (8, 8, 8), (-1, 0, 0), (0, 20, 0), (0, 0, 0), (24, 19, 19), (23, 19, 0)]
    cells, length = ref.descend(d, NEED, want, starts, 40)
    assert length[0] == 1 and (length[[1, 2, 3, 4, 6]] == 0).all() and length[5] > 10 and length[7] > 10
    got = c_descend(d, NEED, want, starts, 40, seed=1)
    assert np.array_equal(got[0], cells) and np.array_equal(got[1], length)
    assert (got[0][0] == goal).all()                                  # start == goal: every row is the goal
    assert (got[0][1] == -1).all() and (got[0][5, length[5]:] == goal).all()
    # one short of the longest path, and room for one cell only: the count is still the whole path's
    long = int(length.max())
    for room in (long, long - 1, 1):
        cells, n = ref.descend(d, NEED, want, starts, room)
        got = c_descend(d, NEED, want, starts, room, seed=room)
        assert np.array_equal(got[0], cells) and np.array_equal(got[1], length) and np.array_equal(n, length)
    assert (got[0][5, 0] == (0, 0, 0)).all()
    # P == 0: nothing is written
    cells, n = c_descend(d, NEED, want, np.zeros((0, 3), np.int32), 8, seed=9)
    assert cells.shape == (0, 8, 3) and n.shape == (0,)


@gpu
def test_descend_random_field_many_starts():
    dims = (40, 36, 44)
    d = random_volume(dims, 0.25, 3)
    d[20, 18, 22] = OPEN
    want, _, _ = check_route(d, NEED, [(20, 18, 22)], seed=1)
    rng = np.random.default_rng(2)
    starts = rng.integers(-1, np.array(dims) + 1, size=(203, 3))
    cells, length = ref.descend(d, NEED, want, starts, 96)
    got = c_descend(d, NEED, want, starts, 96, seed=2)
    assert np.array_equal(got[0], cells) and np.array_equal(got[1], length)
    assert (length > 0).sum() > 80 and (length == 0).sum() > 20 and length.max() <= 96


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
def test_plan_transit_goes_round_a_wall_the_straight_path_hits():
    from gaussiangrasper_amd import field, transit
    from gaussiangrasper_amd.grasp import default_gripper
    dev = torch.device(DEV)
    f = field.DistanceField(*BOX, voxel=H, device=dev)
    table = _blob((0.0, 0.0, 0.0), (0.64, 0.48, 0.02), dev)
    wall = _blob((0.30, 0.0, 0.02), (0.33, 0.30, 0.40), dev)          # from the table to the top, open beyond y = 0.30
    f.add(table)
    f.add(wall)
    f.update()
    assert int((f.dist2 == 0).sum()) > 5000
    radius = 0.01
    spheres = field.gripper_spheres(default_gripper(), 0.06, 0.02, 0.02, radius)
    carried = transit.carried_spheres(np.random.default_rng(0).uniform(-0.015, 0.015, (500, 3)) + [0.03, 0, 0], radius)
    spheres = np.concatenate([spheres, carried])
    goal = _pose(0.3, (0.52, 0.12, 0.22))
    starts = np.stack([_pose(0.0, (0.12, 0.12, 0.22)), _pose(1.2, (0.10, 0.20, 0.25))])
    for s in starts:                                                   # the fixture can see the feature
        straight = field.path_clear(f, field.interpolate(s, goal, 64)[None], spheres, radius)
        assert not bool(straight.clear[0]) and 0 < int(straight.first_hit[0]) < 64
    plans = {}
    for steps in (9, 64, 257):
        plan = transit.plan_transit(f, starts, goal, spheres, radius, steps=steps)
        assert plan.poses.shape == (2, steps, 12) and plan.planned.all() and plan.cost_to_go.rounds >= 2
        assert bool(plan.clearance.clear.all()) and int(plan.clearance.slack.min()) >= 0, plan.clearance.first_hit
        p = plan.poses.cpu().numpy()
        assert np.array_equal(p[:, 0], starts) and np.array_equal(p[:, -1], np.stack([goal, goal]))
        assert plan.best == int(np.argmin(plan.cost)) and np.isfinite(plan.cost).all()
        # longer than the straight line, and past the wall's open end
        assert (plan.cost > np.linalg.norm(starts[:, 9:] - goal[9:], axis=1)).all()
        if steps > 9:
            assert (p[:, :, 10].max(1) > 0.30).all()
        plans[steps] = plan
    # the cost field and the cells against the restatement, through the Python layer
    ctg = plans[64].cost_to_go
    d = f.dist2.cpu().numpy()
    want, ignored = ref.route(d, ctg.need, ctg.goals)
    assert np.array_equal(ctg.cost.cpu().numpy(), want) and int(ctg.ignored) == ignored == 0
    cells, length = ref.descend(d, ctg.need, want, transit.cells_of(f, starts[:, 9:]), plans[64].cells.shape[1])
    assert np.array_equal(plans[64].cells.cpu().numpy(), cells) and np.array_equal(plans[64].length.cpu().numpy(), length)
    # descend with too little room calls again
    got = transit.descend(ctg, starts[:, 9:], max_cells=3)
    assert got[0].shape[1] == int(length.max()) and np.array_equal(got[1].cpu().numpy(), length)
    assert np.array_equal(got[2].cpu().numpy(), want[tuple(transit.cells_of(f, starts[:, 9:]).T)])
    # the obstacle moves: remove + add + update, and the new plan differs and is clear again
    moved = _blob((0.30, 0.18, 0.02), (0.33, 0.48, 0.40), dev)        # now open below y = 0.18
    f.remove(wall)
    f.add(moved)
    f.update()
    again = transit.plan_transit(f, starts, goal, spheres, radius, steps=64)
    assert again.planned.all() and bool(again.clearance.clear.all())
    assert not torch.equal(again.poses, plans[64].poses)
    assert (again.poses[:, :, 10].cpu().numpy().min(1) < 0.18).all()
    # a goal inside the wall: nothing is planned, and the answer says so
    none = transit.plan_transit(f, starts, _pose(0.0, (0.315, 0.30, 0.2)), spheres, radius, steps=16)
    assert none.best == -1 and not none.planned.any() and np.isinf(none.cost).all() and int(none.cost_to_go.ignored) == 1


@gpu
def test_command_line_plans_from_a_saved_field(tmp_path, capsys):
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
    np.save(tmp_path / "carried.npy", np.random.default_rng(0).uniform(-0.015, 0.015, (200, 3)) + [0.03, 0, 0])
    rc = transit.main(["--field", str(tmp_path / "field.npz"), "--from", str(tmp_path / "from.npy"), "--to",
                       str(tmp_path / "to.npy"), "--gripper", "default", "--width", "0.06", "--radius", "0.01",
                       "--steps", "32", "--carried", str(tmp_path / "carried.npy"), "--out", str(tmp_path / "paths.npy"),
                       "--report", str(tmp_path / "report.npz")])
    assert rc == 0 and "2 of 2 starts have a path, 2 clear" in capsys.readouterr().out
    paths = np.load(tmp_path / "paths.npy")
    assert paths.dtype == np.float32 and paths.shape == (2, 32, 12) and np.array_equal(paths[:, 0], starts)
    with np.load(tmp_path / "report.npz") as z:
        assert z["clear"].all() and z["planned"].all() and int(z["best"]) in (0, 1) and (z["slack"] >= 0).all()
        again = field.path_clear(field.DistanceField.load(str(tmp_path / "field.npz")), paths, z["spheres"], 0.01)
        assert np.array_equal(again.slack.cpu().numpy(), z["slack"])
        assert np.isfinite(z["cost"]).all() and (z["length"] > 30).all() and int(z["rounds"]) >= 2
