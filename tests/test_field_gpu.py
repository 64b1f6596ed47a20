"""GPU checks of the distance field (gg_field_splat, gg_field_distance, gg_field_paths and gaussiangrasper_amd.field)
against the restatement (tests/field_ref.py).  Everything is held to equality; the C calls' arrays are carved from the
sentinel arena (tests/arena.py) and compared whole."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import field_ref as ref
from arena import Arena
from grasp_ref import rotation

gpu = pytest.mark.gpu
DEV = "cuda:0"
D = ctypes.c_double
FAR = ref.FAR
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 2.0 ** -6                                   # a power of two: lo + c h is exact in fp32 and fp64
LO = (-0.25, 0.125, 0.5)
DIMS = (40, 36, 44)
GRID = np.array([*LO, H])


def _define(name):
    src = open(os.path.join(ROOT, "gaussiangrasper_amd", "csrc", "field.hip")).read()
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, src, flags=re.M)
    assert m, f"#define {name} not found in field.hip"
    return int(m.group(1))


FS_THREADS, FS_THREAD_REACH = _define("FS_THREADS"), _define("FS_THREAD_REACH")
FD_THREADS, FD_TILE = _define("FD_THREADS"), _define("FD_TILE")


def _lib():
    from gaussiangrasper_amd import _lib as L
    return L.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def c_splat(dims, grid, means, rot, scales, weights, mass=None, extent=1.0, max_reach=8, min_weight=0.0, sign=1,
            seed=0, calls=1):
    """gg_field_splat `calls` times on the same arena -> (mass, skipped, truncated) after the last one"""
    n = len(means)
    a = Arena(DEV, seed)
    a.carve("means", np.asarray(means, np.float32).reshape(n, 3), 4, "in")
    a.carve("rot", np.asarray(rot, np.float32).reshape(n, 9), 4, "in")
    a.carve("scales", np.asarray(scales, np.float32).reshape(n, 3), 4, "in")
    a.carve("weights", np.asarray(weights, np.float32).reshape(n), 4, "in")
    a.carve("mass", np.zeros(dims, np.int64) if mass is None else np.asarray(mass, np.int64), 8, "inout")
    a.carve("skipped", np.zeros(1, np.int64), 8, "out")
    a.carve("truncated", np.zeros(1, np.int64), 8, "out")
    d, g = (ctypes.c_int32 * 3)(*dims), (D * 4)(*grid)
    signs = sign if isinstance(sign, (tuple, list)) else (sign,) * calls
    for s in signs:
        st = _lib().gg_field_splat(d, g, n, a.ptr("means"), a.ptr("rot"), a.ptr("scales"), a.ptr("weights"), D(extent),
                                   max_reach, D(min_weight), s, a.ptr("mass"), a.ptr("skipped"), a.ptr("truncated"),
                                   _stream())
        assert st == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    out = a.check()
    return out["mass"], int(out["skipped"][0]), int(out["truncated"][0])


def c_distance(mass, threshold, seed=0):
    dims = mass.shape
    a = Arena(DEV, seed)
    d = (ctypes.c_int32 * 3)(*dims)
    need = _lib().gg_field_distance_workspace(d)
    assert need > 0 and need % 256 == 0
    a.carve("mass", np.asarray(mass, np.int64), 8, "in")
    a.carve("dist2", np.zeros(dims, np.int32), 4, "out")
    a.carve("ws", int(need), 256, "ws")
    st = _lib().gg_field_distance(d, a.ptr("mass"), int(threshold), a.ptr("dist2"), a.ptr("ws"),
                                  ctypes.c_size_t(need), _stream())
    assert st == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    return a.check()["dist2"]


def c_paths(dims, grid, dist2, poses, spheres, need2, outside, seed=0):
    P, W = poses.shape[:2]
    S = len(spheres)
    a = Arena(DEV, seed)
    a.carve("dist2", np.asarray(dist2, np.int32).reshape(dims), 4, "in")
    a.carve("poses", np.asarray(poses, np.float32), 4, "in")
    a.carve("spheres", np.asarray(spheres, np.float32).reshape(S, 3), 4, "in")
    a.carve("need2", np.asarray(need2, np.int32).reshape(S), 4, "in")
    a.carve("slack", np.zeros((P, W), np.int32), 4, "out")
    a.carve("first_hit", np.zeros(P, np.int32), 4, "out")
    st = _lib().gg_field_paths((ctypes.c_int32 * 3)(*dims), (D * 4)(*grid), a.ptr("dist2"), P, W, a.ptr("poses"), S,
                               a.ptr("spheres"), a.ptr("need2"), int(outside), a.ptr("slack"), a.ptr("first_hit"),
                               _stream())
    assert st == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    out = a.check()
    return out["slack"], out["first_hit"]


def rows(rng, n, dims=DIMS, smax=1.4, wide=0.02):
    """n rows in and around the volume: scales up to smax cells, a share `wide` of them up to 4 cells (the wave's
    path of field_splat_kernel, mixed into waves of rows that walk their own box)"""
    lo, dim = np.array(LO), np.array(dims)
    means = (lo + rng.uniform(-3.0, dim + 3.0, size=(n, 3)) * H).astype(np.float32)
    s = rng.uniform(0.3, smax, size=(n, 3))
    big = rng.random(n) < wide
    s[big] = rng.uniform(1.5, 4.0, size=(int(big.sum()), 3))
    return means, rotation(rng, n).astype(np.float32), (s * H).astype(np.float32), \
        rng.uniform(0.01, 1.0, n).astype(np.float32)


def check_splat(dims, grid, r, **kw):
    want = ref.splat(dims, grid, *r, **{k: v for k, v in kw.items() if k != "seed"})
    got = c_splat(dims, grid, *r, **kw)
    assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0])
    assert got[1:] == (want[1], want[2]), (got[1:], want[1:])
    return want


# ------------------------------------------------------------------------------------------------
# splat
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 100_003])
def test_splat_sizes_against_the_restatement(n):
    """around a wave, past FS_THREADS, and many workgroups (100 003 rows at max_reach 1: every row is cut)"""
    assert (FS_THREADS, FS_THREAD_REACH) == (256, 2), "sizes and reaches below were chosen around these"
    rng = np.random.default_rng(n)
    big = n > 5000
    r = rows(rng, n, smax=0.9 if big else 1.4, wide=0.0 if big else 0.05)
    if n == 1:
        r[0][0] = np.float32(LO) + np.float32([20.3, 18.6, 22.1]) * np.float32(H)      # the one row: inside
    mass, skipped, cut = check_splat(DIMS, GRID, r, max_reach=1 if big else 8, seed=n)
    assert skipped == 0 and cut == (n if big else 0)
    assert (mass != 0).sum() >= min(n, 20)


@gpu
def test_splat_rows_that_take_no_part_are_counted():
    rng = np.random.default_rng(7)
    n = 300
    m, R, s, w = rows(rng, n)
    m[3, 1], m[4, 0], m[5, 2] = np.nan, np.inf, -np.inf
    s[10, 0], s[11, 2], s[12, 1], s[13, 0] = 0.0, -H, np.nan, np.inf
    w[20], w[21], w[22], w[23], w[24], w[25] = 0.25, 0.2499, 32768.0, 40000.0, np.nan, np.inf
    w[26], w[27] = np.nextafter(np.float32(0.25), np.float32(1)), np.nextafter(np.float32(32768), np.float32(0))
    R[30, 1, 1], R[31, 2, 2] = np.nan, np.inf
    mass, skipped, _ = check_splat(DIMS, GRID, (m, R, s, w), min_weight=0.25, seed=1)
    assert skipped == int((~ref.row_takes_part(m, R, s, w, 0.25)).sum()) and skipped > 50      # w <= 0.25: a quarter
    assert ref.row_takes_part(m, R, s, w, 0.25)[[26, 27]].all()
    assert not ref.row_takes_part(m, R, s, w, 0.25)[[3, 4, 5, 10, 11, 12, 13, 20, 21, 22, 23, 24, 25, 30, 31]].any()
    _, none, _ = check_splat(DIMS, GRID, (m, R, s, w), min_weight=-np.inf, seed=2)
    assert none == 13


@gpu
def test_splat_means_outside_on_faces_and_far_away():
    lo, dim = np.array(LO), np.array(DIMS)
    # outside the volume by two cells on each side, the ellipsoid reaching in
    out = np.array([[-2, 10, 10], [dim[0] + 1, 10, 10], [10, -2, 10], [10, dim[1] + 1, 10], [10, 10, -2],
                    [10, 10, dim[2] + 1], [-2, -2, -2]], np.float64)
    m = (lo + (out + 0.5) * H).astype(np.float32)
    n = len(m)
    r = (m, np.repeat(np.eye(3, dtype=np.float32)[None], n, 0), np.full((n, 3), 3.5 * H, np.float32),
         np.full(n, 0.5, np.float32))
    mass, _, _ = check_splat(DIMS, GRID, r, seed=3)
    assert (mass != 0).sum() > 6 * 20
    # means exactly on cell faces, edges and corners, the volume's own faces among them (the upper ones are outside)
    c = np.array([[0, 0, 0], [5, 7, 9], [dim[0], 3, 3], [3, dim[1], dim[2]], [12, 0, 44], [1, 1, 1], [39, 35, 43]])
    m = (lo + c * H).astype(np.float32)
    assert np.array_equal(m.astype(np.float64), lo + c * H)
    r = (m, np.repeat(np.eye(3, dtype=np.float32)[None], len(m), 0), np.full((len(m), 3), 0.25 * H, np.float32),
         np.full(len(m), 1.0, np.float32))
    mass, _, _ = check_splat(DIMS, GRID, r, extent=0.0, seed=4)
    inside = (c < dim).all(1)
    assert (mass != 0).sum() == inside.sum() and all(mass[tuple(k)] == 65536 for k in c[inside])
    # far away: cells beyond every reach, and beyond the clamp of the cell index
    far = np.float32([[1e6, 0, 0], [-3e38, 3e38, 0], [0, 0, 1e12]])
    r = (far, np.repeat(np.eye(3, dtype=np.float32)[None], 3, 0), np.full((3, 3), 2 * H, np.float32),
         np.full(3, 1.0, np.float32))
    mass, skipped, _ = check_splat(DIMS, GRID, r, seed=5)
    assert not mass.any() and skipped == 0


@gpu
def test_splat_boundary_lattice_and_extent_zero():
    dims, grid = (24, 24, 24), np.array([0.0, 0.0, 0.0, 0.125])
    eye = np.eye(3, dtype=np.float32)[None]
    r = (np.float32([[12.5 * 0.125] * 3]), eye, np.float32([[5 * 0.125] * 3]), np.float32([1.0]))
    mass, _, cut = check_splat(dims, grid, r, seed=6)
    ii = np.stack(np.meshgrid(*[np.arange(24)] * 3, indexing="ij"), -1) - 12
    assert cut == 0 and np.array_equal(mass != 0, (ii ** 2).sum(-1) <= 25)      # (3, 4, 0) h is on the boundary
    rng = np.random.default_rng(9)
    r = rows(rng, 200)
    mass, _, _ = check_splat(DIMS, GRID, r, extent=0.0, seed=7)
    own = np.stack([ref.cell_index(r[0][:, a].astype(np.float64) - LO[a], H) for a in range(3)], 1)
    inside = ((own >= 0) & (own < np.array(DIMS))).all(1)
    assert mass.sum() == np.trunc(r[3][inside].astype(np.float64) * 65536).sum()


@gpu
@pytest.mark.parametrize("max_reach", [0, 1, FS_THREAD_REACH, FS_THREAD_REACH + 1, 8])
def test_splat_max_reach_cuts_rows(max_reach):
    rng = np.random.default_rng(20 + max_reach)
    r = rows(rng, 700, smax=1.6, wide=0.1)
    reach, cut = ref.row_reach(r[2], 1.0, H, max_reach)
    _, _, truncated = check_splat(DIMS, GRID, r, max_reach=max_reach, seed=max_reach)
    assert truncated == int(cut.sum())
    if max_reach <= 1:
        assert truncated == 700                   # n >= 1 for every scale > 0: reach 2 at least
    elif max_reach <= FS_THREAD_REACH + 1:
        assert 0 < truncated < 700
    else:
        assert truncated == 0
    if max_reach > FS_THREAD_REACH:
        assert (reach > FS_THREAD_REACH).sum() > 50 and (reach <= FS_THREAD_REACH).sum() > 50    # both paths


@gpu
def test_splat_one_row_of_reach_64():
    """the wave's path at its largest: 129^3 cells for one row, in a volume that holds them all"""
    dims, h = (130, 130, 130), 2.0 ** -7
    grid = np.array([0.0, 0.0, 0.0, h])
    rng = np.random.default_rng(3)
    r = (np.float32([[65.3 * h, 64.9 * h, 65.5 * h]]), rotation(rng, 1).astype(np.float32),
         np.float32([[63 * h, 40 * h, 20 * h]]), np.float32([0.75]))
    assert ref.row_reach(r[2], 1.0, h, 64)[0].tolist() == [64]
    mass, _, cut = check_splat(dims, grid, r, max_reach=64, seed=8)
    assert cut == 0 and (mass != 0).sum() > 150_000 and set(np.unique(mass)) == {0, 49152}
    r = (r[0], r[1], np.float32([[70 * h, 40 * h, 20 * h]]), r[3])
    assert check_splat(dims, grid, r, max_reach=64, seed=9)[2] == 1


@gpu
def test_splat_accumulates_and_a_minus_call_restores_the_zeros():
    rng = np.random.default_rng(31)
    a, b = rows(rng, 500), rows(rng, 300)
    first = ref.splat(DIMS, GRID, *a)[0]
    both = ref.splat(DIMS, GRID, *b, mass=first)[0]
    assert np.array_equal(c_splat(DIMS, GRID, *b, mass=first, seed=1)[0], both)
    assert np.array_equal(c_splat(DIMS, GRID, *a, calls=2, seed=2)[0], 2 * first)
    again = [c_splat(DIMS, GRID, *a, seed=s)[0] for s in (3, 4)]                 # run to run
    assert np.array_equal(again[0], first) and np.array_equal(again[1], first)
    back, _, _ = c_splat(DIMS, GRID, *a, sign=(1, -1), seed=5)
    assert not back.any()
    assert np.array_equal(c_splat(DIMS, GRID, *b, mass=both, sign=-1, seed=6)[0], first)


@gpu
def test_move_and_rebuild_equals_a_fresh_build():
    from gaussiangrasper_amd.field import DistanceField
    rng = np.random.default_rng(41)
    m, R, s, w = rows(rng, 3000)
    sel = rng.random(3000) < 0.3
    Q = rotation(rng, 1)[0]
    m2, R2 = m.copy(), R.copy()
    m2[sel] = ((m[sel].astype(np.float64) - np.array(LO) - 0.3) @ Q.T + np.array(LO) + 0.32).astype(np.float32)
    R2[sel] = (Q @ R[sel].astype(np.float64)).astype(np.float32)
    t = lambda *arrs: tuple(torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in arrs)      # noqa: E731
    hi = np.array(LO) + np.array(DIMS) * H
    f = DistanceField(LO, hi, H, device=DEV)
    assert tuple(f.dims) == DIMS and np.array_equal(f.grid, GRID)
    c = f.add(t(m, R, s, w))
    f.remove(t(m, R, s, w), mask=torch.from_numpy(sel).to(DEV))
    f.add(t(m2, R2, s, w), mask=torch.from_numpy(sel).to(DEV))
    fresh = DistanceField(LO, hi, H, device=DEV)
    fresh.add(t(m2, R2, s, w))
    torch.cuda.synchronize()
    assert int(c.skipped) == 0 and int(c.truncated) == 0
    assert torch.equal(f.mass, fresh.mass)
    assert np.array_equal(f.mass.cpu().numpy(), ref.splat(DIMS, GRID, m2, R2, s, w)[0])
    thr = 30000
    want = ref.distance(fresh.mass.cpu().numpy(), thr)
    assert np.array_equal(f.update(thr).dist2.cpu().numpy(), want)
    d = f.distance().cpu().numpy()
    assert d.dtype == np.float32 and np.array_equal(d, (np.sqrt(want.astype(np.float64)) * H).astype(np.float32))


# ------------------------------------------------------------------------------------------------
# distance transform
# ------------------------------------------------------------------------------------------------
def _tile_dims():
    """line counts one below, at and one above FD_TILE in each pass (z: X Y lines, y: X Z, x: Y Z), and lines whose
    FD_TILE-line tile is one below, at and one above FD_THREADS cells"""
    t, per = FD_TILE, FD_THREADS // FD_TILE
    out = []
    for n in (t - 1, t, t + 1):
        out += [(n, 1, 3), (1, n, 3), (n, 3, 1), (3, 1, n), (1, 3, n), (3, n, 1), (n, n, n)]
    for L in (per - 1, per, per + 1):
        out += [(L, 3, 5), (3, L, 5), (3, 5, L)]
    return out


EDT_DIMS = [(1, 1, 1), (1, 1, 17), (17, 1, 1), (3, 5, 7), (33, 17, 65), (64, 64, 64), (1024, 2, 2), (65, 33, 129)]


def _patterns(dims, rng, corners=True):
    X, Y, Z = dims
    yield "empty", np.zeros(dims, np.int64), 1
    yield "full", np.full(dims, 5, np.int64), 5
    for k in range(8 if corners else 0):
        m = np.zeros(dims, np.int64)
        m[(X - 1) * (k >> 2 & 1), (Y - 1) * (k >> 1 & 1), (Z - 1) * (k & 1)] = 1
        yield f"corner {k}", m, 1
    m = np.zeros(dims, np.int64)
    m[:, Y // 2, :] = 9
    yield "plane", m, 9
    for density in (0.002, 0.5):
        yield f"density {density}", (rng.random(dims) < density).astype(np.int64) * 40000, 32768
    m = rng.integers(-3, 4, size=dims) + 1000                     # cells at, just below and just above the threshold
    m.flat[0], m.flat[-1] = 1000, (999 if m.size > 1 else 1000)
    yield "threshold", m, 1000


def _check_edt(dims, corners=True):
    assert (FD_THREADS, FD_TILE) == (256, 8), "_tile_dims was written around these"
    rng = np.random.default_rng(sum(dims))
    for name, mass, thr in _patterns(dims, rng, corners):
        want = ref.distance(mass, thr)
        got = c_distance(mass, thr, seed=len(name))
        assert got.dtype == np.int32 and np.array_equal(got, want), (dims, name)
        if name == "empty":
            assert (got == FAR).all()
        if name == "threshold":
            assert np.array_equal(got == 0, mass >= 1000) and 0 < (mass == 1000).sum()


@gpu
@pytest.mark.parametrize("dims", EDT_DIMS)
def test_edt_against_the_restatement(dims):
    _check_edt(dims)


@gpu
def test_edt_around_the_line_tile_and_the_workgroup_span():
    for dims in _tile_dims():
        _check_edt(dims, corners=False)


@gpu
def test_edt_far_corner():
    m = np.zeros((1024, 2, 2), np.int64)
    m[0, 0, 0] = 2
    d = c_distance(m, 2)
    assert d[1023, 1, 1] == 1023 ** 2 + 2 and d[0, 0, 0] == 0


# ------------------------------------------------------------------------------------------------
# paths
# ------------------------------------------------------------------------------------------------
def _poses(rng, P, W, spread=4.0):
    """random rotations; translations in and around the volume"""
    lo, dim = np.array(LO), np.array(DIMS)
    t = lo + rng.uniform(-spread, dim + spread, size=(P * W, 3)) * H
    return np.concatenate([rotation(rng, P * W).reshape(-1, 9), t], 1).reshape(P, W, 12).astype(np.float32)


@gpu
@pytest.mark.parametrize("P,W,S", [(1, 1, 1), (3, 5, 7), (257, 9, 33), (1, 1, 1024), (4, 6, 0)])
def test_paths_against_the_restatement(P, W, S):
    rng = np.random.default_rng(P * 1000 + W * 10 + S)
    dist2 = rng.integers(0, 400, size=DIMS).astype(np.int32)
    dist2[rng.random(DIMS) < 0.05] = FAR
    dist2[rng.random(DIMS) < 0.05] = 0
    poses = _poses(rng, P, W)
    if P * W > 4:
        poses[P // 2, W // 2, 5] = np.nan                 # a pose that is not finite inside a path
        poses[0, W - 1, 10] = np.inf
    spheres = rng.uniform(-6 * H, 6 * H, size=(S, 3)).astype(np.float32)
    need2 = rng.integers(0, 300, size=S).astype(np.int32)
    if S >= 7:
        need2[0], need2[1] = 0, FAR
    for outside in (FAR, 0, 77):
        want = ref.paths(DIMS, GRID, dist2, poses, spheres, need2, outside)
        got = c_paths(DIMS, GRID, dist2, poses, spheres, need2, outside, seed=outside % 251)
        assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]), outside
        assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), outside
        if S == 0:
            fin = np.isfinite(poses).all(-1)
            assert (got[0][fin] == FAR).all() and (got[0][~fin] == ref.INT32_MIN).all()
    if S >= 7 and P > 100:
        w_free, w_blocked = (ref.paths(DIMS, GRID, dist2, poses, spheres, need2, o)[0] for o in (FAR, 0))
        assert (w_free != w_blocked).sum() > 50           # centres outside the volume decided those
        assert (w_free == ref.INT32_MIN).sum() == 2


@gpu
def test_paths_faces_need2_limits_and_first_hit():
    lo = np.array(LO)
    eye = np.eye(3).reshape(-1)
    dist2 = np.full(DIMS, 50, np.int32)
    dist2[10, 11, 12] = 0
    dist2[11, 11, 12] = 49
    pose = lambda c: np.concatenate([eye, lo + np.asarray(c, np.float64) * H])        # noqa: E731
    origin = np.zeros((1, 3), np.float32)
    # a centre exactly on a cell face belongs to the upper cell; on the volume's upper face it is outside
    P = np.array([[pose([10, 11, 12]), pose([11, 11, 12]), pose([10.999, 11, 12]), pose([DIMS[0], 5, 5]),
                   pose([0, 0, 0]), pose([-1e-3, 0, 0])]], np.float32)
    for outside in (FAR, 0):
        s, f = c_paths(DIMS, GRID, dist2, P, origin, [0], outside)
        assert s.tolist() == [[0, 49, 0, outside, 50, outside]] and f.tolist() == [6]
        want = ref.paths(DIMS, GRID, dist2, P, origin, [0], outside)
        assert np.array_equal(s, want[0]) and np.array_equal(f, want[1])
    # need2 of 0 never hits, need2 of FAR hits everywhere but where dist2 is FAR
    dist2[20:, :, :] = FAR
    Q = np.array([[pose([10, 11, 12]), pose([5, 5, 5]), pose([25, 5, 5])]], np.float32)
    assert c_paths(DIMS, GRID, dist2, Q, origin, [0], FAR)[0].tolist() == [[0, 50, FAR]]
    s, f = c_paths(DIMS, GRID, dist2, Q, origin, [FAR], FAR)
    assert s.tolist() == [[-FAR, 50 - FAR, 0]] and f.tolist() == [0]
    # first_hit at 0, at W - 1, absent, and behind a pose that is not finite
    W = 7
    free, hit = pose([5.5, 5.5, 5.5]), pose([10.5, 11.5, 12.5])
    paths = np.array([[free] * W] * 4, np.float32)
    paths[0, 0], paths[1, W - 1], paths[3, 4], paths[3, 2, 3] = hit, hit, hit, np.nan
    s, f = c_paths(DIMS, GRID, dist2, paths, origin, [1], FAR)
    assert f.tolist() == [0, W - 1, W, 2] and s[3, 2] == ref.INT32_MIN and s[0, 0] == -1 and s[2].tolist() == [49] * W
    want = ref.paths(DIMS, GRID, dist2, paths, origin, [1], FAR)
    assert np.array_equal(s, want[0]) and np.array_equal(f, want[1])


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
@gpu
def test_table_and_box_end_to_end(tmp_path):
    from gaussiangrasper_amd import field
    from gaussiangrasper_amd.grasp import default_gripper
    g = np.arange(-0.245, 0.25, 0.01)                      # cell centres: 50 x 50 of the table, 10^3 of the box on it
    table = np.stack(np.meshgrid(g, g, [0.005], indexing="ij"), -1).reshape(-1, 3)
    b = np.arange(-0.045, 0.05, 0.01)
    box = np.stack(np.meshgrid(b, b, np.arange(0.015, 0.11, 0.01), indexing="ij"), -1).reshape(-1, 3)
    means = np.concatenate([table, box]).astype(np.float32)
    n = len(means)
    rng = np.random.default_rng(2)
    q = rng.normal(size=(n, 4)).astype(np.float32)
    scene = types.SimpleNamespace(
        means=torch.from_numpy(means).to(DEV), quats=torch.from_numpy(q).to(DEV),
        scales=torch.full((n, 3), float(np.log(0.006)), device=DEV),
        opacities=torch.full((n, 1), 2.0, device=DEV))
    f = field.DistanceField([-0.3, -0.3, -0.05], [0.3, 0.3, 0.35], 0.01, device=DEV)
    counts = f.add(scene)
    f.update()
    ins = [t.cpu().numpy() for t in field.model_gaussians(scene)]
    mass, skipped, cut = ref.splat(f.dims, f.grid, *ins)
    assert (int(counts.skipped), int(counts.truncated)) == (skipped, cut) == (0, 0)
    assert np.array_equal(f.mass.cpu().numpy(), mass)
    dist2 = ref.distance(mass, field.THRESHOLD)
    assert np.array_equal(f.dist2.cpu().numpy(), dist2) and (dist2 == 0).sum() > 3000
    spheres = field.gripper_spheres(default_gripper(), 0.08, 0.02, 0.02, 0.008)
    down = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])               # the approach axis points down
    a, b_, c = ([*down.reshape(-1), -0.2, 0.0, z] for z in (0.3, 0.3, 0.06))
    over = field.interpolate(a, [*down.reshape(-1), 0.2, 0.0, 0.3], 16)
    through = field.interpolate(c, [*down.reshape(-1), 0.2, 0.0, 0.06], 16)
    poses = np.stack([over, through])
    res = field.path_clear(f, poses, spheres, 0.008, margin=0.005)
    need = field.need2(np.full(len(spheres), 0.008), 0.005, 0.01)
    slack, first = ref.paths(f.dims, f.grid, dist2, poses, spheres, need, FAR)
    assert np.array_equal(res.slack.cpu().numpy(), slack) and np.array_equal(res.first_hit.cpu().numpy(), first)
    assert res.clear.tolist() == [True, False] and 0 < int(res.first_hit[1]) < 15 and int(res.first_hit[0]) == 16
    blocked = field.path_clear(f, poses, spheres, 0.008, margin=0.005, outside="blocked")
    assert np.array_equal(blocked.slack.cpu().numpy(), ref.paths(f.dims, f.grid, dist2, poses, spheres, need, 0)[0])
    f.save(str(tmp_path / "f.npz"))
    back = field.DistanceField.load(str(tmp_path / "f.npz"), device=DEV)
    assert torch.equal(back.mass, f.mass) and torch.equal(back.dist2, f.dist2) and back.threshold == f.threshold
    assert np.array_equal(back.grid, f.grid) and np.array_equal(back.dims, f.dims)
