"""GPU checks of gripper clearance (gaussiangrasper_amd.grasp.clearance on gg_grasp_clearance) against the fp64
restatement (tests/grasp_clear_ref.py): all six outputs equal on scenes whose sums are exact, at sizes around every
stage, chunk and grasp-tile boundary; points exactly on every face; limits at equality and one ulp below; rows, parts
and points that are data, not errors; the cull under scaled and sheared frames; real weights to fp32 rounding and run
to run; the finger parts against gg_grasp_contacts' collision weight; memory around every output; and a box on a
table end to end."""
import ctypes
import math

import numpy as np
import pytest
import torch

from grasp_clear_ref import part_bounds, restate, slab_gripper
from grasp_propose_ref import box_faces
from grasp_ref import grasp_rows, rotation

gpu = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("body_count", "body_weight", "sweep_count", "sweep_weight", "valid", "clear")


def run(points, weights, grasps, parts, **kw):
    from gaussiangrasper_amd.grasp import clearance
    t = [torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(DEV) for a in (points, weights, grasps)]
    r = clearance(*t, parts, **kw)
    torch.cuda.synchronize()
    return {k: getattr(r, k).cpu().numpy() for k in KEYS}


def check_equal(got, ref, p):
    """every output equal to the restatement's, the weights after its fp64 sums are rounded to fp32"""
    m = len(ref["valid"])
    for k in KEYS:
        assert got[k].shape == ((m, p) if k.endswith(("count", "weight")) else (m,)), k
    for k in ("body_count", "sweep_count"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), k
    for k in ("body_weight", "sweep_weight"):
        assert got[k].dtype == np.float32 and np.array_equal(got[k], ref[k].astype(np.float32)), k
    for k in ("valid", "clear"):
        assert got[k].dtype == np.bool_ and np.array_equal(got[k], ref[k]), k


def dyadic_weights(rng, n):
    """multiples of 2^-10 in (0, 4]: every fp64 sum of them is exact, whatever the order"""
    return (rng.integers(1, 4097, size=n) / 1024.0).astype(np.float32)


def cloud(rng, n, half=0.025):
    return rng.uniform(-half, half, size=(n, 3)).astype(np.float32)


def candidates(rng, m, spread=0.008):
    """m grasps centred inside the cloud, random rotations and sizes"""
    return grasp_rows(rotation(rng, m), rng.uniform(-spread, spread, size=(m, 3)), rng.uniform(0.02, 0.05, m),
                      rng.uniform(0.015, 0.035, m), rng.uniform(0.005, 0.03, m), score=rng.random(m))


def plant(p, g):
    """Overwrites the first points of the cloud, three for each of the first grasps, so that whatever the density
    these grasps see something with every gripper of grippers(): one point in the middle of the left finger, one
    between the fingers (inside a slab part), one 4.9 cm behind the centre (in the palm's and in a slab's sweep of
    5 cm).  The rotations are orthonormal: p = t + R u."""
    G = g.astype(np.float64)
    for k in range(min(len(g), len(p) // 3)):
        R, t = G[k, 4:13].reshape(3, 3), G[k, 13:16]
        for j, u in enumerate(([0.0, -0.5 * G[k, 1] - 0.002, 0.0], [0.0, 0.001, 0.0], [-0.049, 0.001, 0.0])):
            p[3 * k + j] = t + R @ np.array(u)
    return p


def grippers():
    from gaussiangrasper_amd.grasp import default_gripper
    return {1: slab_gripper(1), 4: default_gripper(), 8: slab_gripper(8)}


# ------------------------------------------------------------------------------------------------
# exact grid
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("m", [0, 1, 7, 256, 257, 600])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513, 5000])
def test_exact_against_the_restatement(n, m):
    """N = 5000 with M = 600 crosses both a chunk and a grasp-tile boundary (512-point chunks at least, 256 grasps
    per workgroup); 255 / 256 / 257 / 513 sit around the 256-point stage"""
    rng = np.random.default_rng(1000 * n + m)
    p, w, g = cloud(rng, n), dyadic_weights(rng, n), candidates(rng, m)
    if n == 1:
        p[0] = 0.0
    plant(p, g)
    for P, parts in grippers().items():
        for approach in (0.0, 0.05):
            # the limits are the median totals: exact sums, so half the grasps sit at or under them, one of them on it
            ref = restate(p, w, g, parts, approach=approach)
            mb, ms = (float(np.median(ref[k])) if m else 1.0 for k in ("body_total", "sweep_total"))
            ref["clear"] = ref["valid"] & (ref["body_total"] <= mb) & (ref["sweep_total"] <= ms)
            check_equal(run(p, w, g, parts, approach=approach, max_body=mb, max_sweep=ms), ref, P)
            if approach == 0.0:
                assert not ref["sweep_count"].any()
            elif n >= 255 and m > 0:          # the case has substance
                assert (ref["body_count"].sum(1) > 0).sum() > m / 2
                assert (ref["sweep_count"].sum(1) > 0).sum() > m / 2
                if m >= 256:
                    assert ref["clear"].any() and not ref["clear"].all()


# ------------------------------------------------------------------------------------------------
# faces
# ------------------------------------------------------------------------------------------------
def _perm_rotations():
    out = []
    for perm in ([0, 1, 2], [1, 2, 0], [2, 0, 1], [1, 0, 2], [0, 2, 1], [2, 1, 0]):
        for signs in ([1, 1, 1], [-1, 1, -1], [1, -1, -1], [-1, -1, 1]):
            R = np.zeros((3, 3))
            R[np.arange(3), perm] = signs
            out.append(R)
    return out


@gpu
def test_points_on_every_face():
    """dyadic sizes, centres and offsets with axis-permutation rotations: u is exact, so every closed face of the
    body, the open face x_lo of the sweep and its closed far face x_lo - approach decide as the contract states"""
    from gaussiangrasper_amd.grasp import default_gripper
    parts = default_gripper(depth_base=2.0 ** -6, finger_width=2.0 ** -8, tail_length=2.0 ** -5)
    approach, e = 2.0 ** -4, 2.0 ** -13
    width, height, depth = 2.0 ** -4, 2.0 ** -5, 2.0 ** -6
    row = grasp_rows(np.eye(3)[None], [[0, 0, 0]], width, height, depth)
    B = part_bounds(parts, row)[0]                                    # (4, 6), every bound dyadic
    U = []
    for b in B:
        xs = [b[0] - approach - e, b[0] - approach, b[0] - e, b[0], b[1], b[1] + e]
        ys = [b[2] - e, b[2], b[3], b[3] + e]
        zs = [b[4] - e, b[4], b[5], b[5] + e]
        U.append(np.array(np.meshgrid(xs, ys, zs, indexing="ij")).reshape(3, -1).T)
    U = np.unique(np.concatenate(U), axis=0)
    # what the contract says of these exact local coordinates
    yz = ((U[:, None, 1] >= B[None, :, 2]) & (U[:, None, 1] <= B[None, :, 3]) & (U[:, None, 2] >= B[None, :, 4]) &
          (U[:, None, 2] <= B[None, :, 5]))
    body = yz & (U[:, None, 0] >= B[None, :, 0]) & (U[:, None, 0] <= B[None, :, 1])
    sweep = yz & (U[:, None, 0] >= B[None, :, 0] - approach) & (U[:, None, 0] < B[None, :, 0])
    assert not (body & sweep).any() and body.sum(0).min() >= 8 and sweep.sum(0).min() >= 8
    pts, grasps = [], []
    for k, R in enumerate(_perm_rotations()):
        t = np.array([k * 0.5, -0.25 + k * 0.25, 0.5])
        pts.append(t + U @ R.T)          # p = t + R u, exact in fp32
        grasps.append(grasp_rows(R[None], [t], width, height, depth))
    p = np.concatenate(pts).astype(np.float32)
    assert np.array_equal(p.astype(np.float64), np.concatenate(pts))
    g = np.concatenate(grasps)
    w = dyadic_weights(np.random.default_rng(5), len(p))
    got = run(p, w, g, parts, approach=approach)
    check_equal(got, restate(p, w, g, parts, approach=approach), 4)
    # the grasps stand 0.55 apart and the gripper reaches 0.13: each sees its own points only
    assert (got["body_count"] == body.sum(0)).all() and (got["sweep_count"] == sweep.sum(0)).all()


# ------------------------------------------------------------------------------------------------
# limits
# ------------------------------------------------------------------------------------------------
@gpu
def test_limits_at_equality_and_one_ulp_below():
    rng = np.random.default_rng(9)
    p, w, g = cloud(rng, 3000), dyadic_weights(rng, 3000), candidates(rng, 40)
    parts = grippers()[4]
    ref = restate(p, w, g, parts, approach=0.05)
    several = ((ref["body_count"] > 0).sum(1) >= 2) & ((ref["sweep_count"] > 0).sum(1) >= 2)     # totals over parts
    assert several.any()
    k = int(np.argmax(several))
    tb, ts = float(ref["body_total"][k]), float(ref["sweep_total"][k])
    below = lambda x: float(np.nextafter(x, 0.0))
    for mb, ms, want in ((tb, ts, True), (below(tb), ts, False), (tb, below(ts), False), (math.inf, ts, True),
                         (tb, None, True)):
        kw = dict(approach=0.05, max_body=mb, max_sweep=ms)
        got = run(p, w, g, parts, **kw)
        assert bool(got["clear"][k]) is want, (mb, ms)
        check_equal(got, restate(p, w, g, parts, approach=0.05, max_body=mb,
                                 max_sweep=math.inf if ms is None else ms), 4)


# ------------------------------------------------------------------------------------------------
# rows, parts and points that are data
# ------------------------------------------------------------------------------------------------
@gpu
def test_bad_rows_empty_parts_and_points_that_take_no_part():
    from gaussiangrasper_amd.grasp import box_part, default_gripper
    rng = np.random.default_rng(13)
    n, m = 4000, 64
    p, w, g = cloud(rng, n), dyadic_weights(rng, n), candidates(rng, m)
    bad = {0: (0, np.nan), 1: (1, np.inf), 2: (2, np.nan), 3: (3, -np.inf), 4: (8, np.nan), 5: (14, np.inf),
           6: (16, np.nan), 7: (1, 0.0), 8: (1, -0.05), 9: (2, 0.0), 10: (2, -0.02)}
    for r, (col, v) in bad.items():
        g[r, col] = v
    g[11, 3] = -0.05                       # depth may have either sign: the fingers are then empty, the row valid
    p[100, 1] = np.nan                     # non-finite points between finite ones
    p[101, 0] = np.inf
    p[2000, 2] = -np.inf
    w[200:260] = 0.25                      # w <= min_weight
    w[300] = np.nan
    w[301] = -np.inf
    # a fifth part that is empty for the narrow rows only: y from 0.0175 to width / 2
    narrow = np.zeros((6, 4))
    narrow[:, 0] = [-0.01, 0.02, 0.0175, 0.0, -0.01, 0.01]
    narrow[3, 1] = 0.5
    parts = np.concatenate([default_gripper(), narrow[None], box_part((0.2, 0.1), (-1, 1), (-1, 1))[None]])
    kw = dict(approach=0.05, min_weight=0.25, max_body=6.0, max_sweep=12.0)
    got, ref = run(p, w, g, parts, **kw), restate(p, w, g, parts, **kw)
    check_equal(got, ref, 6)
    rows = sorted(bad)
    assert not got["valid"][rows].any() and not got["clear"][rows].any()
    for k in KEYS[:4]:
        assert not got[k][rows].any(), k
    assert got["valid"][11:].all() and got["body_count"][11, :2].sum() == 0
    B = part_bounds(parts, g)
    empty = B[11:, 4, 2] > B[11:, 4, 3]
    assert empty.any() and not empty.all()
    assert not got["body_count"][11:, 4][empty].any() and not got["sweep_count"][11:, 4][empty].any()
    assert got["body_count"][11:, 4][~empty].any() and got["sweep_count"][11:, 4][~empty].any()
    assert not got["body_count"][:, 5].any() and not got["sweep_count"][:, 5].any()      # x_lo > x_hi for every row
    # the points that take no part change nothing: the same call without them
    keep = np.isfinite(p).all(1) & (w.astype(np.float64) > 0.25)
    assert keep.sum() < n - 60
    check_equal(run(p[keep], w[keep], g, parts, **kw), ref, 6)
    # no points: zeros, and clear = valid; no grasps: empty outputs
    got = run(np.zeros((0, 3)), np.zeros(0), g, parts, **kw)
    assert np.array_equal(got["clear"], ref["valid"]) and np.array_equal(got["valid"], ref["valid"])
    assert not any(got[k].any() for k in KEYS[:4])
    got = run(p, w, np.zeros((0, 17)), parts, **kw)
    assert got["clear"].shape == (0,) and got["body_weight"].shape == (0, 6)


# ------------------------------------------------------------------------------------------------
# the cull
# ------------------------------------------------------------------------------------------------
def _points_around(rng, g, parts, approach, per_grasp):
    """per_grasp points for every row, spread over 1.3 times the box that holds the row's body and sweep volumes,
    mapped to the world through the inverse of u = R^T (p - t)"""
    G = g.astype(np.float64)
    B = part_bounds(parts, g)
    lo = np.stack([B[:, :, 0].min(1) - approach, B[:, :, 2].min(1), B[:, :, 4].min(1)], 1)
    hi = np.stack([B[:, :, 1].max(1), B[:, :, 3].max(1), B[:, :, 5].max(1)], 1)
    out = []
    for k in range(len(G)):
        c, h = 0.5 * (lo[k] + hi[k]), 0.65 * (hi[k] - lo[k])
        u = c + rng.uniform(-1, 1, size=(per_grasp, 3)) * h
        Q = np.linalg.inv(G[k, 4:13].reshape(3, 3)).T
        out.append(G[k, 13:16] + u @ Q.T)
    return np.concatenate(out).astype(np.float32)


@gpu
@pytest.mark.parametrize("frame", ["small", "large", "sheared"])
def test_scaled_and_sheared_frames(frame):
    """R scaled by 1e-3 and 1e3 keeps max|R| max|R^-T| near 1 and is culled with a box of the right size; R sheared
    past GC_MAX_COND = 1e3 is not culled at all.  Either way the counts are the restatement's."""
    rng = np.random.default_rng({"small": 21, "large": 22, "sheared": 23}[frame])
    m = 48
    R = rotation(rng, m)
    if frame == "sheared":
        S = np.eye(3)
        S[0, 1] = 2000.0
        R = R @ S
    else:
        R = R * (1e-3 if frame == "small" else 1e3)
    t = rng.uniform(-0.5, 0.5, size=(m, 3))
    g = grasp_rows(R, t, rng.uniform(0.03, 0.08, m), rng.uniform(0.015, 0.035, m), rng.uniform(0.005, 0.03, m))
    parts = grippers()[4]
    p = _points_around(rng, g, parts, 0.05, 400)
    w = dyadic_weights(rng, len(p))
    ref = restate(p, w, g, parts, approach=0.05)
    check_equal(run(p, w, g, parts, approach=0.05), ref, 4)
    assert (ref["body_count"].sum(1) > 0).sum() > m // 2 and (ref["sweep_count"].sum(1) > 0).sum() > m // 2


@gpu
def test_far_grasps_and_points_beside_the_faces_of_the_cull_box():
    """grasps far from every point count nothing; points within a few fp32 steps (a relative 1e-7) inside and outside
    every face of the box that holds all body and sweep volumes are inside the cull's margin, and the fp64 test
    decides them"""
    rng = np.random.default_rng(27)
    parts = grippers()[4]
    approach = 0.05
    m = 24
    Rs = _perm_rotations()
    t = rng.uniform(-0.5, 0.5, size=(m, 3))
    t[:12] = 0.0                           # at the origin the fp32 point keeps the relative 1e-7
    g = grasp_rows(np.array(Rs[:m]), t, rng.uniform(0.03, 0.08, m), rng.uniform(0.015, 0.035, m),
                   rng.uniform(0.005, 0.03, m))
    G = g.astype(np.float64)
    B = part_bounds(parts, g)
    lo = np.stack([B[:, :, 0].min(1) - approach, B[:, :, 2].min(1), B[:, :, 4].min(1)], 1)
    hi = np.stack([B[:, :, 1].max(1), B[:, :, 3].max(1), B[:, :, 5].max(1)], 1)
    pts = []
    for k in range(m):
        Rk, tk = G[k, 4:13].reshape(3, 3), G[k, 13:16]
        for ax in range(3):
            for face in (lo[k, ax], hi[k, ax]):
                # a point of that face that lies on a part: the middle of the left finger, moved onto the face (x_hi,
                # y_lo and both z faces are its own, y_hi the right finger's); the tail's sweep reaches farthest back
                u = np.array([0.5 * (B[k, 0, 0] + B[k, 0, 1]), 0.5 * (B[k, 0, 2] + B[k, 0, 3]), 0.0])
                if ax == 0 and face == lo[k, 0]:
                    u[1] = 0.0
                for rel in (-2e-7, -1e-7, 0.0, 1e-7, 2e-7):
                    v = u.copy()
                    v[ax] = face * (1.0 + rel)
                    pts.append(tk + Rk @ v)
    p = np.array(pts, np.float32)
    far = grasp_rows(rotation(rng, 8), rng.uniform(-0.5, 0.5, size=(8, 3)) + 100.0, 0.05, 0.02, 0.02)
    g = np.concatenate([g, far])
    w = dyadic_weights(rng, len(p))
    got, ref = run(p, w, g, parts, approach=approach), restate(p, w, g, parts, approach=approach)
    check_equal(got, ref, 4)
    assert not got["body_count"][m:].any() and not got["sweep_count"][m:].any() and got["clear"][m:].all()
    own = 30 * 12                                        # the points of the 12 grasps that stand alone
    hits = ref["body_count"][12:m].sum() + ref["sweep_count"][12:m].sum()
    assert 0.2 * own < hits < 0.8 * own                 # points on both sides of the faces
    assert ref["body_count"][:12].sum() + ref["sweep_count"][:12].sum() > own // 2


# ------------------------------------------------------------------------------------------------
# real weights
# ------------------------------------------------------------------------------------------------
@gpu
def test_real_weights_to_fp32_rounding_and_run_to_run():
    """the kernel's fp64 sum and the restatement's differ by reordering only, N 2^-52 relative; the fp32 rounding of
    a positive sum adds 2^-24: 2^-23 of the sum bounds both"""
    rng = np.random.default_rng(31)
    n, m = 20_000, 300
    p, g = cloud(rng, n), candidates(rng, m)
    w = (1.0 / (1.0 + np.exp(-rng.normal(size=n) * 2.0))).astype(np.float32)
    parts = grippers()[4]
    free = restate(p, w, g, parts, approach=0.05)
    mb, ms = float(np.median(free["body_total"])), float(np.median(free["sweep_total"]))
    kw = dict(approach=0.05, max_body=mb, max_sweep=ms)
    a, b = run(p, w, g, parts, **kw), run(p, w, g, parts, **kw)
    ref = restate(p, w, g, parts, **kw)
    for k in ("body_count", "sweep_count", "valid"):
        assert np.array_equal(a[k], ref[k]), k
    for k in ("body_weight", "sweep_weight"):
        assert (np.abs(a[k].astype(np.float64) - ref[k]) <= 2.0 ** -23 * ref[k]).all(), k
    assert (ref["body_weight"] > 0).sum() > m and (ref["sweep_weight"] > 0).sum() > m
    near = (np.abs(ref["body_total"] - mb) < 1e-9 * mb) | (np.abs(ref["sweep_total"] - ms) < 1e-9 * ms)
    assert near.sum() <= 2                 # a total on its limit may round either way: not compared
    assert np.array_equal(a["clear"][~near], ref["clear"][~near]) and ref["clear"].any() and not ref["clear"].all()
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------------------------------------
# the finger parts against gg_grasp_contacts
# ------------------------------------------------------------------------------------------------
@gpu
def test_finger_parts_give_the_collision_weight_of_contacts():
    """the two finger parts alone with approach 0 are gg_grasp_contacts' finger boxes but for the inner faces, which
    no random point sits on: the same points, summed in another order (N 2^-52) and rounded to fp32 per finger here
    and over both there, 2^-24 of the sum each: 2^-22 of the sum bounds the difference"""
    from gaussiangrasper_amd.grasp import contacts, default_gripper
    rng = np.random.default_rng(37)
    n, m = 20_000, 300
    p, g = cloud(rng, n), candidates(rng, m)
    w = rng.uniform(0.05, 1.0, size=n).astype(np.float32)
    nr = rng.normal(size=(n, 3)).astype(np.float32)
    t = [torch.as_tensor(a).to(DEV) for a in (p, nr, w, g)]
    want = contacts(*t).collision_weight.cpu().numpy().astype(np.float64)
    got = run(p, w, g, default_gripper()[:2])
    assert got["valid"].all() and not got["sweep_count"].any()
    both = got["body_weight"].astype(np.float64).sum(1)
    assert (np.abs(both - want) <= 2.0 ** -22 * want).all()
    assert (want > 0).sum() > m // 2


# ------------------------------------------------------------------------------------------------
# memory
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,m", [(5000, 600), (513, 257), (0, 7)])
def test_nothing_is_written_outside_the_outputs_and_the_workspace(n, m):
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(41 + n)
    P, parts = 4, np.ascontiguousarray(grippers()[4])
    p, w, g = cloud(rng, n), dyadic_weights(rng, n), candidates(rng, m)
    dp, dw, dg = (torch.as_tensor(a).to(DEV) for a in (p, w, g))
    need = lib.gg_grasp_clearance_workspace(n, m, P)
    assert need > 0
    sizes = [m * P * 4] * 4 + [m, m, need]                 # the six outputs, then the workspace
    offs, off = [], 256
    for s in sizes:
        offs.append(off)
        off = (off + s + 255) // 256 * 256 + 256            # a guard of 256 bytes at least after each
    buf = torch.full((off,), 0xA5, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    ptrs = [ctypes.c_void_p(buf.data_ptr() + o) for o in offs]
    st = lib.gg_grasp_clearance(n, ctypes.c_void_p(dp.data_ptr()), ctypes.c_void_p(dw.data_ptr()), m,
                                ctypes.c_void_p(dg.data_ptr()), P, parts.ctypes.data_as(ctypes.c_void_p), 0.05, 0.0,
                                8.0, 16.0, *ptrs[:6], ptrs[6], ctypes.c_size_t(need),
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0, lib.gg_last_error()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    guard = np.ones(off, bool)
    for o, s in zip(offs, sizes):
        guard[o:o + s] = False
    assert (host[guard] == 0xA5).all()
    ref = restate(p, w, g, parts, approach=0.05, max_body=8.0, max_sweep=16.0)
    view = lambda i, dt: host[offs[i]:offs[i] + sizes[i]].view(dt)
    got = dict(body_count=view(0, np.int32).reshape(m, P), body_weight=view(1, np.float32).reshape(m, P),
               sweep_count=view(2, np.int32).reshape(m, P), sweep_weight=view(3, np.float32).reshape(m, P),
               valid=view(4, np.uint8).astype(bool), clear=view(5, np.uint8).astype(bool))
    assert set(view(4, np.uint8).tolist()) <= {0, 1} and set(view(5, np.uint8).tolist()) <= {0, 1}
    check_equal(got, ref, P)


# ------------------------------------------------------------------------------------------------
# a scene of Gaussians, end to end
# ------------------------------------------------------------------------------------------------
H = 2.0 ** -8


def _flat_box_scene():
    """A flat box (16 x 12 x 4 H, about 6 x 5 x 1.6 cm) standing on a table at z = -H / 2, as flat discs whose
    smallest axis is the face normal.  Returns (Scene, object mask (N,) bool)."""
    from gaussiangrasper_amd.scene import make_scene
    pa, na = box_faces([16 * H, 12 * H, 4 * H], H, (0.0, 0.0, 2 * H))
    k = (np.arange(-40, 41)) * H
    tx, ty = (a.ravel() for a in np.meshgrid(k, k, indexing="ij"))
    pt = np.stack([tx, ty, np.full_like(tx, -0.5 * H)], 1)
    nt = np.tile([0.0, 0.0, 1.0], (len(pt), 1))
    p, n = np.concatenate([pa, pt]), np.concatenate([na, nt])
    sc = make_scene(len(p), feature_dim=32)
    r = math.sqrt(0.5)
    quat = np.zeros((len(p), 4))
    ax = np.abs(n).argmax(1)
    quat[ax == 2] = (1.0, 0.0, 0.0, 0.0)                                      # local z stays z
    quat[ax == 0] = (r, 0.0, r, 0.0)                                          # about y: z -> x
    quat[ax == 1] = (r, -r, 0.0, 0.0)                                         # about x: z -> y
    sc.means = torch.from_numpy(p.astype(np.float32))
    sc.quats = torch.from_numpy(quat.astype(np.float32))
    sc.scales = torch.log(torch.tensor([0.002, 0.002, 0.0002])).expand(len(p), 3).contiguous()
    sc.opacities = torch.full((len(p), 1), 4.0)
    mask = np.zeros(len(p), bool)
    mask[:len(pa)] = True
    return sc, mask


@gpu
def test_grasp_object_keeps_only_approaches_from_above():
    """Fingers 4 cm tall (height) cannot come at a 1.6 cm box sideways without scraping the table, a closing axis
    along z puts the palm through the table, and every approach from below starts under it: with the default
    gripper, a 5 cm approach and less than one disc's opacity (0.98) allowed, what is left comes down from above.
    Without a gripper the friction cone alone decides, and approaches from under the table are kept."""
    from gaussiangrasper_amd.grasp import default_gripper
    from gaussiangrasper_amd.grasp_propose import grasp_object
    sc, mask = _flat_box_scene()
    sc = sc.to(DEV)
    m = torch.from_numpy(mask).to(DEV)
    rows, res, keep = grasp_object(sc, m, num_approach=8, height=0.04, gripper=default_gripper(), approach=0.05,
                                   max_body=0.5, max_sweep=0.5)
    rows_np, keep_np = rows.cpu().numpy(), keep.cpu().numpy()
    c = res.clearance
    assert c is not None and c.body_weight.shape == (len(rows_np), 4) and c.valid.all()
    assert len(keep_np) >= 1
    a_up = rows_np[:, 10].astype(np.float64)                                   # a . up = R[2][0], up = +z
    assert (a_up[keep_np] < 0).all()
    clear = c.clear.cpu().numpy()
    assert clear[keep_np].all() and np.array_equal(res.feasible.cpu().numpy()[keep_np], clear[keep_np])
    tot = c.body_weight.double().sum(1).cpu().numpy(), c.sweep_weight.double().sum(1).cpu().numpy()
    assert (tot[0][keep_np] <= 0.5).all() and (tot[1][keep_np] <= 0.5).all()
    rows0, res0, keep0 = grasp_object(sc, m, num_approach=8, height=0.04)
    assert torch.equal(rows0, rows) and res0.clearance is None
    k0 = keep0.cpu().numpy()
    below = a_up[k0] > 0
    assert below.any() and set(keep_np.tolist()) < set(k0.tolist())
    start_z = rows_np[k0, 15] - 0.05 * a_up[k0]                                # t - approach a, its height
    assert (start_z[below] < -0.5 * H).any()                                   # it sets out from under the table
    assert not clear[k0[below]].any()


@gpu
def test_cli_report_gains_the_clearance_arrays_only_with_a_gripper(tmp_path):
    from gaussiangrasper_amd import grasp, interop
    sc, _ = _flat_box_scene()
    interop.save_checkpoint(tmp_path / "step-000029999.ckpt", sc, {
        "layers.0.weight": torch.randn(128, 32) * 0.2, "layers.0.bias": torch.randn(128) * 0.1,
        "layers.2.weight": torch.randn(512, 128) * 0.1, "layers.2.bias": torch.randn(512) * 0.1}, 29999)
    rng = np.random.default_rng(43)
    g = grasp_rows(rotation(rng, 50), rng.uniform(-0.03, 0.03, size=(50, 3)) + [0, 0, 0.02], 0.07, 0.02, 0.02)
    np.save(tmp_path / "grasps.npy", g)
    common = ["--ckpt", str(tmp_path / "step-000029999.ckpt"), "--grasps", str(tmp_path / "grasps.npy"),
              "--out", str(tmp_path / "kept.npy"), "--report", str(tmp_path / "report.npz")]
    base = {"grasps_scene", "contact_idx", "normals", "angles", "region_count", "region_weight", "collision_weight",
            "feasible"}
    assert grasp.main(common) == 0
    assert set(np.load(tmp_path / "report.npz").files) == base
    assert grasp.main(common + ["--gripper", "default", "--approach", "0.05", "--max-sweep-collision", "0.5"]) == 0
    r = np.load(tmp_path / "report.npz")
    assert set(r.files) == base | {"body_weight", "sweep_weight", "body_count", "sweep_count", "clear"}
    pts, _, w = grasp.model_points(sc.to(DEV))
    want = grasp.clearance(pts, w, torch.from_numpy(g).to(DEV), grasp.default_gripper(), approach=0.05,
                           max_sweep=0.5)
    assert np.array_equal(r["clear"], want.clear.cpu().numpy()) and r["body_count"].shape == (50, 4)
    assert np.array_equal(r["sweep_weight"], want.sweep_weight.cpu().numpy())
    assert not (r["feasible"] & ~r["clear"]).any() and len(np.load(tmp_path / "kept.npy")) == r["feasible"].sum()
