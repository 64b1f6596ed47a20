"""GPU checks of the placement layer (gg_height_map, gg_place_search and gaussiangrasper_amd.place) against the
restatement (tests/place_ref.py).  Everything is held to equality; the C calls' arrays are carved from the sentinel
arena (tests/arena.py) and compared whole."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import place_ref as ref
import plane_ref
from arena import Arena

gpu = pytest.mark.gpu
DEV = "cuda:0"
D = ctypes.c_double
I2 = ctypes.c_int32 * 2
EMPTY, MAXL = ref.EMPTY, ref.MAX_LEVEL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLS = (0, 2, MAXL)


def _define(name):
    src = open(os.path.join(ROOT, "gaussiangrasper_amd", "csrc", "place.hip")).read()
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, src, flags=re.M)
    assert m, f"#define {name} not found in place.hip"
    return int(m.group(1))


T = _define("PS_TILE")
PH_THREADS = _define("PH_THREADS")


def _lib():
    from gaussiangrasper_amd import _lib as L
    return L.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


# ------------------------------------------------------------------------------------------------
# gg_place_search
# ------------------------------------------------------------------------------------------------
def c_search(top, under, tol, seed=0):
    (U, V), (K, A, B) = top.shape, under.shape
    I, J = U - A + 1, V - B + 1
    a = Arena(DEV, seed)
    a.carve("top", np.asarray(top, np.int32), 4, "in")
    a.carve("under", np.asarray(under, np.int32), 4, "in")
    a.carve("rest", np.zeros((K, I, J), np.int32), 4, "out")
    a.carve("contact", np.zeros((K, I, J), np.int32), 4, "out")
    a.carve("support", np.zeros((K, I, J, 6), np.int32), 4, "out")
    st = _lib().gg_place_search(I2(U, V), a.ptr("top"), K, I2(A, B), a.ptr("under"), int(tol), a.ptr("rest"),
                                a.ptr("contact"), a.ptr("support"), _stream())
    assert st == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    if K == 0:
        assert a.untouched()
        return None
    out = a.check()
    return out["rest"], out["contact"], out["support"]


SHAPES = [(1, 1, 1, 1, 1), (17, 33, 1, 1, 2), (40, 37, 5, 4, 3), (T + 4, T + 4, 5, 5, 1), (T + 5, T + 5, 5, 5, 1),
          (T + 4, 2 * T + 5, 5, 5, 1), (130, 130, 128, 128, 2), (128, 128, 128, 128, 1), (150, 131, 37, 29, 5)]
CONTENTS = ("30 % full", "full, extremes, corner holes", "single cell, empty yaw, seam holes", "constant")


def _contents(kind, shape, rng):
    U, V, A, B, K = shape
    top = rng.integers(-1000, 1000, size=(U, V)).astype(np.int32)
    under = rng.integers(-1000, 1000, size=(K, A, B)).astype(np.int32)
    if kind == CONTENTS[0]:                       # random levels, negatives among them; no empty scene cell
        under[rng.random((K, A, B)) >= 0.3] = EMPTY
        under[:, rng.integers(A), rng.integers(B)] = 5            # no map without a cell
    elif kind == CONTENTS[1]:                     # every object cell; levels at +-MAX_LEVEL; holes at two corners
        top[rng.random((U, V)) < 0.05] = MAXL
        top[rng.random((U, V)) < 0.05] = -MAXL
        under[rng.random((K, A, B)) < 0.05] = MAXL
        under[rng.random((K, A, B)) < 0.05] = -MAXL
        if U * V > 1:
            top[0, 0] = top[U - 1, V - 1] = EMPTY
    elif kind == CONTENTS[2]:                     # one cell; an empty yaw beside a full one; holes on the tile seams
        under[0] = EMPTY
        under[0, A - 1, B // 2] = -7
        if K > 1:
            under[1] = EMPTY
        for s in range(T - 1, max(U, V), T):      # anchors T - 1 and T read these through different tiles
            if s + 1 < U:
                top[s:s + 2, (s * 7) % V] = EMPTY
            if s + 1 < V:
                top[(s * 5) % U, s:s + 2] = EMPTY
    else:                                         # every cell a contact, every sum at its maximum
        top[:], under[:] = MAXL, MAXL
    return top, under


@gpu
@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_search_against_the_restatement(shape, kind):
    assert T == 32, "the shapes were laid around this tile: one tile, one past it, uneven tiles, 3 x 3 anchors at 128"
    rng = np.random.default_rng(sum(shape) + CONTENTS.index(kind))
    top, under = _contents(kind, shape, rng)
    U, V, A, B, K = shape
    for tol, want in zip(TOLS, ref.search_many(top, under, TOLS)):
        got = c_search(top, under, tol, seed=tol % 251)
        for name, g, w in zip(("rest", "contact", "support"), got, want):
            assert g.dtype == np.int32 and np.array_equal(g, w), (name, tol)
    rest, contact, support = want                                   # tol = MAX_LEVEL: every cell of a valid anchor
    if kind != CONTENTS[1]:                                         # (there the levels lie further apart than that)
        cells = (under != EMPTY).sum((1, 2))
        assert ((contact == 0) | (contact == cells[:, None, None])).all()
    if kind == CONTENTS[0]:
        assert (rest != EMPTY).all()
    if kind == CONTENTS[1] and U * V > 1:
        assert rest[0, 0, 0] == EMPTY and rest[K - 1, -1, -1] == EMPTY
        assert support[0, 0, 0].tolist() == [0, 0, -1, -1, -1, -1]
    if kind == CONTENTS[2]:
        assert (contact[0][rest[0] != EMPTY] == 1).all()
        if K > 1:
            assert (rest[1] == EMPTY).all() and (contact[1] == 0).all()
        if K > 2:
            assert (rest[2] != EMPTY).any()
        if max(U - A, V - B) >= T:
            assert (rest[0] == EMPTY).any() and (rest[0] != EMPTY).any()
    if kind == CONTENTS[3]:
        assert (rest == 2 * MAXL).all() and (contact == A * B).all()
        assert (support == [A * B * (A - 1) // 2, A * B * (B - 1) // 2, 0, A - 1, 0, B - 1]).all()


@gpu
def test_search_without_a_yaw_writes_nothing():
    rng = np.random.default_rng(0)
    top = rng.integers(-9, 9, size=(12, 10)).astype(np.int32)
    assert c_search(top, np.zeros((0, 3, 4), np.int32), 2) is None


@gpu
def test_search_wrapper_and_its_level_check():
    from gaussiangrasper_amd import place
    rng = np.random.default_rng(4)
    top, under = _contents(CONTENTS[0], (50, 41, 9, 6, 4), rng)
    want = ref.search(top, under, 2)
    got = place.search(top, under, 2, device=DEV)
    again = place.search(torch.from_numpy(top).to(DEV), torch.from_numpy(under).to(DEV), 2)
    for g, h, w in zip((got.rest, got.contact, got.support), (again.rest, again.contact, again.support), want):
        assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w) and torch.equal(g, h)
    top[3, 3] = MAXL + 1
    with pytest.raises(ValueError, match="top holds a level"):
        place.search(top, under, 2, device=DEV)
    with pytest.raises(ValueError):
        place.search(top[:5], under, 2, device=DEV)             # the object does not fit


# ------------------------------------------------------------------------------------------------
# gg_height_map
# ------------------------------------------------------------------------------------------------
H, HZ = 2.0 ** -6, 2.0 ** -8
GRID = np.array([-0.5, -0.375, H, HZ])
DIMS = (70, 50)


def c_height(points, weights, frames, grid=GRID, dims=DIMS, min_weight=0.0, start=None, seed=0, calls=1):
    """gg_height_map `calls` times on the same arena -> (map, dropped) after the last one"""
    n, F = len(points), len(frames)
    a = Arena(DEV, seed)
    a.carve("points", np.asarray(points, np.float32).reshape(n, 3), 4, "in")
    if weights is not None:
        a.carve("weights", np.asarray(weights, np.float32).reshape(n), 4, "in")
    a.carve("frames", np.asarray(frames, np.float64).reshape(F, 12), 8, "in")
    a.carve("map", np.full((F, *dims), EMPTY, np.int32) if start is None else np.asarray(start, np.int32), 4, "inout")
    a.carve("dropped", np.zeros(F, np.int64), 8, "out")
    for _ in range(calls):
        st = _lib().gg_height_map(n, a.ptr("points"), a.ptr("weights") if weights is not None else ctypes.c_void_p(0),
                                  D(min_weight), F, a.ptr("frames"), (D * 4)(*grid), I2(*dims), a.ptr("map"),
                                  a.ptr("dropped"), _stream())
        assert st == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    out = a.check()
    return out["map"], out["dropped"]


def tilted_frames(F, seed):
    """F frames over plane_ref's tilted plane: yaws about the normal, origins moved about; the underside for odd f"""
    from gaussiangrasper_amd import place
    rng = np.random.default_rng(seed)
    base = place.plane_frame((plane_ref.TRUE_NORMAL, plane_ref.TRUE_OFFSET), (0.0, 0.0, 0.0))
    fr = place.yaw_frames(base, base.o + rng.uniform(-0.05, 0.05, 3), rng.uniform(0, np.pi, F), 0, 0, H)
    fr[:, 0] += rng.uniform(-0.03, 0.03, (F, 3))
    fr[1::2, 3] *= -1.0
    return fr.reshape(F, 12)


def cloud(n, seed):
    """n points around the tilted plane's origin: most over the grid, some beside it, a few not finite"""
    rng = np.random.default_rng(seed)
    o = -plane_ref.TRUE_OFFSET * plane_ref.TRUE_NORMAL
    p = (o + rng.uniform(-0.65, 0.65, (n, 3)) * [1.0, 1.0, 0.2]).astype(np.float32)
    if n >= 255:
        p[3, 1], p[10, 0], p[77, 2] = np.nan, np.inf, -np.inf
    return p


def check_height(points, weights, frames, **kw):
    ref_kw = {k: v for k, v in kw.items() if k in ("min_weight",)}
    want = ref.height_map(points, weights, frames, kw.get("grid", GRID), kw.get("dims", DIMS), out=kw.get("start"),
                          **ref_kw)
    got = c_height(points, weights, frames, **kw)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0])
    assert got[1].dtype == np.int64 and np.array_equal(got[1], want[1]), (got[1], want[1])
    return want


@gpu
@pytest.mark.parametrize("F", [1, 3, 16])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 100_003])
def test_height_map_sizes_against_the_restatement(n, F):
    """around a workgroup and many of them, null and thresholded weights, tilted frames"""
    assert PH_THREADS == 256, "the sizes were chosen around this"
    rng = np.random.default_rng(n + F)
    p, fr = cloud(n, n + F), tilted_frames(F, F)
    m, dropped = check_height(p, None, fr, seed=F)
    if n == 0:
        assert (m == EMPTY).all() and dropped.tolist() == [0] * F
    if n >= 255:
        assert (dropped >= 3).all() and (dropped < n).all() and (m != EMPTY).sum() >= min(n // 4, 2000) * F // 2
    w = rng.uniform(0.0, 1.0, n).astype(np.float32)
    if n >= 255:
        w[20], w[21], w[22] = np.nan, 0.5, np.nextafter(np.float32(0.5), np.float32(1))
    _, thr = check_height(p, w, fr, min_weight=0.5, seed=F + 1)
    if n >= 255:
        assert (thr > dropped).all() and ref.takes_part(p, w, 0.5)[[20, 21, 22]].tolist() == [False, False, True]


@gpu
def test_height_map_boundaries_outside_and_the_atomic_path():
    eye = np.concatenate([np.zeros(3), np.eye(3).reshape(-1)])[None]
    lo = GRID[:2]
    c = np.array([[0, 0, 0], [5, 7, 9], [DIMS[0], 3, 3], [3, DIMS[1], -4], [69, 49, -9], [-1, 0, 2], [12, 0, 44]])
    p = np.column_stack([lo[0] + c[:, 0] * H, lo[1] + c[:, 1] * H, c[:, 2] * HZ]).astype(np.float32)
    assert np.array_equal(p[:, 2].astype(np.float64), c[:, 2] * HZ)          # exact: on faces and level boundaries
    below = np.nextafter(p, np.float32(-np.inf))
    far = np.float32([[1e6, 0, 0], [0, -3e38, 3e38], [0, 0, 1e30], [0, 0, -1e30], [3e38, 3e38, 3e38]])
    pts = np.concatenate([p, below, far])
    m, dropped = check_height(pts, None, eye, seed=1)
    assert m[0, 5, 7] == 9 and m[0, 4, 6] == 8 and m[0, 0, 0] == 0 and m[0, 69, 49] == -9 and m[0, 68, 48] == -10
    assert m[0, 32, 24] == MAXL and dropped[0] == 3 + 3 + 3         # upper faces, below the lower ones, far away
    m, _ = check_height(far[2:4], None, place_under(eye), seed=2)
    assert m[0, 32, 24] == MAXL
    # 40 000 points in three cells: the maximum is the same whatever the order of the atomics
    rng = np.random.default_rng(8)
    cell = rng.integers(0, 3, 40_000)
    q = np.column_stack([lo[0] + (10 + cell + rng.random(40_000) * 0.99) * H,
                         lo[1] + (20 + rng.random(40_000) * 0.99) * H, rng.uniform(-1.0, 1.0, 40_000)])
    q = q.astype(np.float32)
    again = [check_height(q, None, eye, seed=s)[0] for s in (3, 4)]
    assert np.array_equal(again[0], again[1]) and (again[0] != EMPTY).sum() == 3


def place_under(frames):
    from gaussiangrasper_amd import place
    return place.underside(np.asarray(frames).reshape(-1, 4, 3))


@gpu
def test_height_map_accumulates_over_calls():
    fr = tilted_frames(3, 9)
    a, b = cloud(3000, 1), cloud(2000, 2)
    first, _ = ref.height_map(a, None, fr, GRID, DIMS)
    both, dropped = check_height(b, None, fr, start=first, seed=1)
    assert (both >= first).all() and (both > first).any() and dropped.min() > 0
    whole, _ = ref.height_map(np.concatenate([a, b]), None, fr, GRID, DIMS)
    assert np.array_equal(both, whole)                               # two calls are one call on all the points
    twice, d2 = c_height(a, None, fr, calls=2, seed=2)       # the second call changes nothing; dropped is written
    assert np.array_equal(twice, first) and np.array_equal(d2, ref.height_map(a, None, fr, GRID, DIMS)[1])


# ------------------------------------------------------------------------------------------------
# the wrappers, end to end
# ------------------------------------------------------------------------------------------------
_ENDS = {}


def _end_to_end(dilate):
    """(device plan, the same through the restatements, points, kind) on place_ref.place_scene(), once per dilate"""
    if dilate not in _ENDS:
        from gaussiangrasper_amd import place
        from gaussiangrasper_amd.grasp import model_points
        pts, kind, plane = ref.place_scene()
        n = len(pts)
        q = np.random.default_rng(2).normal(size=(n, 4)).astype(np.float32)
        scene = types.SimpleNamespace(means=torch.from_numpy(pts).to(DEV), quats=torch.from_numpy(q).to(DEV),
                                      scales=torch.full((n, 3), float(np.log(0.004)), device=DEV),
                                      opacities=torch.full((n, 1), 2.0, device=DEV))
        mask = torch.from_numpy(kind == ref.OBJECT).to(DEV)
        kw = dict(target=tuple(-plane_ref.TRUE_OFFSET * plane_ref.TRUE_NORMAL), cell=ref.CELL, level=ref.LEVEL, yaws=5,
                  region=0.28, dilate=dilate)
        plans = [place.place_object(scene, mask, plane, **kw) for _ in range(2)]
        w = model_points(scene, None)[2].cpu().numpy()
        host = place.place_points(pts, np.where(kind == ref.OBJECT, 0, w).astype(np.float32),
                                  np.where(kind == ref.OBJECT, w, 0).astype(np.float32), plane, maps=ref.height_map,
                                  searcher=ref.searcher, **kw)
        r = kw["region"]
        top = place.scene_top(scene, plane, (-r, -r, r, r), ref.CELL, ref.LEVEL, exclude=mask, centre=kw["target"])
        under = place.object_under(scene, mask, plane, 5, ref.CELL, ref.LEVEL, dilate, centre=kw["target"])
        _ENDS[dilate] = (plans, host, pts, kind, top, under)
    return _ENDS[dilate]


@gpu
@pytest.mark.parametrize("dilate", [0, 1])
def test_scene_top_and_object_under_are_the_plans_maps(dilate):
    (plan, _), host, _, _, (top, frame, grid, dims), (under, frames, pivot) = _end_to_end(dilate)
    assert top.dtype == np.int32 and np.array_equal(top, host.top) and np.array_equal(under, host.under)
    assert np.array_equal(grid, plan.grid) and np.array_equal(dims, plan.dims) and np.array_equal(frame.o, plan.frame.o)
    assert np.array_equal(pivot, host.pivot) and np.array_equal(frames, host.obj_frames)


@gpu
@pytest.mark.parametrize("dilate", [0, 1])
def test_place_object_equals_the_numpy_chain(dilate):
    (plan, again), host = _end_to_end(dilate)[:2]
    assert np.array_equal(plan.top, host.top) and np.array_equal(plan.under, host.under)
    for name in ("rest", "contact", "support"):
        g, w = getattr(plan.found, name), getattr(host.found, name)
        assert np.array_equal(g.cpu().numpy(), w), name
        assert torch.equal(g, getattr(again.found, name)), name
    p, q, r = plan.placements, host.placements, again.placements
    assert len(p.yaw) > 1000
    for name in ("yaw", "anchor", "rest"):
        assert np.array_equal(getattr(p, name), getattr(q, name)), name
    assert np.abs(p.transform - q.transform).max() <= 1e-12
    for name in ("transform", "yaw", "anchor", "rest", "lift", "contact_frac", "score"):
        assert getattr(p, name).tobytes() == getattr(r, name).tobytes(), name     # two calls: identical bytes
    assert np.array_equal(plan.top, again.top) and np.array_equal(plan.under, again.under)


@gpu
@pytest.mark.parametrize("dilate", [0, 1])
def test_no_placement_of_the_device_result_enters_the_scene(dilate):
    (plan, _), _, pts, kind = _end_to_end(dilate)[:4]
    low, high, skip = np.inf, -np.inf, 0.0
    for m in range(len(plan.placements.yaw)):
        gap, skipped = ref.clearance(plan, pts, kind, m)
        low, high, skip = min(low, gap), max(high, gap), max(skip, skipped)
    print(f"{len(plan.placements.yaw)} placements: gap {low:.3f} .. {high:.3f} levels, skipped share {skip:.4f}")
    assert skip <= 0.01 and low >= 0.0
    if dilate == 0:
        assert high + 1.0 <= 2.0
