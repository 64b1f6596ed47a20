"""GPU checks of the support plane (gg_plane_consensus, gg_plane_classify, gaussiangrasper_amd.support, grasp.plane_clear)
against the fp64 restatement (tests/plane_ref.py).  count, valid, best, side and height are compared for equality; every
output is carved out of a sentinel-filled buffer that is compared whole; the workspace holds garbage before every call.
Sizes around the wave, the 256-point pass, the 256-record hypothesis chunk and the 1024-point classify block; lattice
scenes on which every product is exact and many points lie exactly on the limit; hypotheses that are data, not errors;
run-to-run identity; fit_plane, plane_clear and grasp_object end to end."""
import ctypes
import math

import numpy as np
import pytest
import torch

import plane_ref as PR

gpu = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64
S8, S32, SF, SD = 0xA5, -77, -12345.5, -98765.25
P = ctypes.c_void_p
D = ctypes.c_double
FIT = dict(dist=0.004, up=(0.0, 0.0, 1.0), max_tilt=math.radians(20.0))


def _garbage(nbytes, seed):
    gen = torch.Generator(device=DEV).manual_seed(4321 + seed)
    return torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=DEV, generator=gen)


def _wrap(a, dtype, s):
    return np.concatenate([np.full(PAD, s, dtype), np.asarray(a, dtype).reshape(-1), np.full(PAD, s, dtype)])


def call_consensus(points, weights, min_weight, hyp, dist, min_sin2, up=None, cos2=0.0, garbage=0):
    """One gg_plane_consensus call; returns the three output buffers WHOLE (PAD sentinels either side) as numpy."""
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    hyp = np.ascontiguousarray(hyp, np.int32).reshape(-1, 3)
    n, h = len(pts), len(hyp)
    pd = torch.from_numpy(pts).to(DEV)
    wd = None if weights is None else torch.from_numpy(np.ascontiguousarray(weights, np.float32)).to(DEV)
    hd = torch.from_numpy(hyp).to(DEV)
    count = torch.full((h + 2 * PAD,), S32, dtype=torch.int32, device=DEV)
    valid = torch.full((h + 2 * PAD,), S8, dtype=torch.uint8, device=DEV)
    best = torch.full((2 + 2 * PAD,), S32, dtype=torch.int32, device=DEV)
    need = lib.gg_plane_consensus_workspace(n, h)
    assert need > 0 and need % 256 == 0
    ws = _garbage(need, garbage)
    upp = None if up is None else ctypes.cast((D * 3)(*up), P)
    st = lib.gg_plane_consensus(n, P(pd.data_ptr()), P(0 if wd is None else wd.data_ptr()), float(min_weight), h,
                                P(hd.data_ptr()), float(dist), float(min_sin2), upp, float(cos2),
                                P(count.data_ptr() + 4 * PAD), P(valid.data_ptr() + PAD), P(best.data_ptr() + 4 * PAD),
                                P(ws.data_ptr()), need, P(torch.cuda.current_stream().cuda_stream))
    assert st == 0, lib.gg_last_error()
    torch.cuda.synchronize()
    return dict(count=count.cpu().numpy(), valid=valid.cpu().numpy(), best=best.cpu().numpy())


def check_consensus(points, weights, min_weight, hyp, dist, min_sin2, up=None, cos2=0.0):
    """the call equals the restatement, sentinels included; returns the restatement"""
    ref = PR.consensus(points, weights, min_weight, hyp, dist, min_sin2, up, cos2)
    got = call_consensus(points, weights, min_weight, hyp, dist, min_sin2, up, cos2)
    want = dict(count=_wrap(ref["count"], np.int32, S32), valid=_wrap(ref["valid"], np.uint8, S8),
                best=_wrap(ref["best"] if len(np.asarray(hyp).reshape(-1, 3)) else [S32, S32], np.int32, S32))
    for k in ("count", "valid", "best"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    return ref


def call_classify(points, weights, min_weight, plane, origin, dist, garbage=0):
    """One gg_plane_classify call; returns height, side and sums WHOLE (PAD sentinels either side) as numpy."""
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = len(pts)
    pd = torch.from_numpy(pts).to(DEV)
    wd = None if weights is None else torch.from_numpy(np.ascontiguousarray(weights, np.float32)).to(DEV)
    height = torch.full((n + 2 * PAD,), SF, dtype=torch.float32, device=DEV)
    side = torch.full((n + 2 * PAD,), S8, dtype=torch.uint8, device=DEV)
    sums = torch.full((16 + 2 * PAD,), SD, dtype=torch.float64, device=DEV)
    need = lib.gg_plane_classify_workspace(n)
    assert need > 0 and need % 256 == 0
    ws = _garbage(need, garbage)
    st = lib.gg_plane_classify(n, P(pd.data_ptr()), P(0 if wd is None else wd.data_ptr()), float(min_weight),
                               ctypes.cast((D * 4)(*plane), P), ctypes.cast((D * 3)(*origin), P), float(dist),
                               P(height.data_ptr() + 4 * PAD), P(side.data_ptr() + PAD), P(sums.data_ptr() + 8 * PAD),
                               P(ws.data_ptr()), need, P(torch.cuda.current_stream().cuda_stream))
    assert st == 0, lib.gg_last_error()
    torch.cuda.synchronize()
    return dict(height=height.cpu().numpy(), side=side.cpu().numpy(), sums=sums.cpu().numpy())


def check_classify(points, weights, min_weight, plane, origin, dist, exact_sums=False):
    """side and height bit-equal to the restatement, the counts exact, every sum within M 2^-52 sum|terms| (PARITY.md:
    the bound of a reordered fp64 sum of M terms), the sentinels untouched, and two calls the same bits."""
    ref = PR.classify(points, weights, min_weight, plane, origin, dist)
    got = call_classify(points, weights, min_weight, plane, origin, dist)
    assert np.array_equal(got["side"], _wrap(ref["side"], np.uint8, S8))
    assert np.array_equal(got["height"].view(np.uint32), _wrap(ref["height"], np.float32, SF).view(np.uint32))
    s = got["sums"]
    assert (s[:PAD] == SD).all() and (s[-PAD:] == SD).all()
    s = s[PAD:-PAD]
    assert np.array_equal(s[:3], ref["sums"][:3])
    bound = ref["terms"] * 2.0 ** -52 * ref["abs_sums"]
    assert (np.abs(s - ref["sums"]) <= bound).all(), (s - ref["sums"], bound)
    assert (s[ref["abs_sums"] == 0.0] == 0.0).all()                       # a sum over nothing is 0, not garbage
    if exact_sums:
        assert np.array_equal(s, ref["sums"])
    again = call_classify(points, weights, min_weight, plane, origin, dist, garbage=1)
    for k in ("height", "side", "sums"):
        assert again[k].tobytes() == got[k].tobytes(), k
    return ref, s


# ------------------------------------------------------------------------------------------------
# 1. the lattice scene: every product exact, many pairs exactly on the limit
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 257, 1025, 4099])
@pytest.mark.parametrize("h", [1, 63, 64, 65, 300])
def test_consensus_is_exact_on_the_lattice(n, h):
    pts, w = PR.lattice_scene(n, seed=n)
    hyp = PR.lattice_hypotheses(pts, h, seed=1000 * n + h)
    hyp[0] = (0, min(1, n - 1), min(2, n - 1))
    ref = check_consensus(pts, w, 0.25, hyp, 2.0 ** -5, 1e-6)
    if n >= 257 and h >= 63:
        assert ref["valid"].sum() > h // 8 and ref["best"][1] > n // 8
        assert ref["on_limit"] > 100                       # pairs with s s == (dist dist) nn: the limit is inclusive
    # without weights every finite point takes part; with up, the tilted triples drop out
    check_consensus(pts, None, 0.0, hyp, 2.0 ** -5, 1e-6, (0.0, 0.0, 1.0), 0.75)


# ------------------------------------------------------------------------------------------------
# 2. hypotheses that are data, not errors
# ------------------------------------------------------------------------------------------------
@gpu
def test_invalid_hypotheses_count_nothing_and_leave_the_others_alone():
    pts, w = PR.lattice_scene(600, seed=5)
    pts[:8] = [[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [0.25, 0.5, 0], [-0.5, -0.5, 0], [0.5, 0.5, 0],
               [0, 0, 0.5], [0.5, 0, 0.25]]
    w[:8] = 1.0
    pts[8] = (np.nan, 0.0, 0.0)
    pts[9], w[9] = (0.25, -0.25, 0.0), 0.25                      # w <= min_weight: takes no part
    good = [(0, 1, 2), (1, 2, 3), (2, 0, 4)]
    bad = [(0, 0, 1),                # a repeated index
           (1, 2, 2), (3, 1, 3),
           (-1, 1, 2), (0, 600, 2),  # index -1 and index N
           (0, 1, 2 ** 31 - 1), (-2 ** 31, 1, 2),
           (4, 0, 5),                # collinear: (-.5,-.5,0), (0,0,0), (.5,.5,0)
           (0, 1, 8),                # through a NaN point
           (0, 1, 9),                # through a point with w <= min_weight
           (0, 1, 6), (0, 6, 7)]     # the planes y = 0 and x ~ z: tilted beyond max_tilt against up = z
    hyp = np.array(good + bad + good, np.int32)
    up, cos2 = (0.0, 0.0, 1.0), math.cos(math.radians(20.0)) ** 2
    ref = check_consensus(pts, w, 0.25, hyp, 2.0 ** -5, 1e-6, up, cos2)
    assert ref["valid"].tolist() == [1, 1, 1] + [0] * len(bad) + [1, 1, 1]
    assert (ref["count"][3:3 + len(bad)] == 0).all() and (ref["count"][:3] > 200).all()
    assert np.array_equal(ref["count"][:3], ref["count"][-3:])
    # the others unchanged: the same good hypotheses alone give the same counts
    alone = check_consensus(pts, w, 0.25, np.array(good, np.int32), 2.0 ** -5, 1e-6, up, cos2)
    assert np.array_equal(alone["count"], ref["count"][:3])
    # duplicated hypotheses tie to the smaller index: all six good ones are the plane z = 0
    assert ref["count"][0] == ref["count"][1] == ref["count"][2] and ref["best"].tolist() == [0, ref["count"][0]]
    assert check_consensus(pts, w, 0.25, hyp[::-1].copy(), 2.0 ** -5, 1e-6, up, cos2)["best"][0] == 0
    # without up the tilted triples are valid; with min_sin2 = 0 only the exactly collinear one drops out
    free = check_consensus(pts, w, 0.25, hyp, 2.0 ** -5, 1e-6)
    assert free["valid"][-5:-3].tolist() == [1, 1] and free["valid"][10] == 0
    assert check_consensus(pts, w, 0.25, hyp, 2.0 ** -5, 0.0)["valid"][10] == 0
    # all invalid: best = (-1, 0)
    none = check_consensus(pts, w, 0.25, np.array(bad, np.int32), 2.0 ** -5, 1e-6, up, cos2)
    assert none["best"].tolist() == [-1, 0] and not none["valid"].any()
    # N == 0: every hypothesis invalid; H == 0: nothing is written
    assert check_consensus(np.zeros((0, 3), np.float32), None, 0.0, np.array(good, np.int32), 0.1, 1e-6)["best"][0] == -1
    check_consensus(pts, w, 0.25, np.zeros((0, 3), np.int32), 2.0 ** -5, 1e-6)
    # dist == 0: only points exactly on the plane
    zero = check_consensus(pts, w, 0.25, np.array(good, np.int32), 0.0, 1e-6)
    assert 100 < zero["count"][0] < ref["count"][0]


@gpu
def test_consensus_across_point_chunks_and_hypothesis_chunks():
    """20000 points make 20 point chunks; 600 hypotheses make 3 hypothesis chunks, the last one ragged."""
    pts, w = PR.lattice_scene(20000, seed=9)
    hyp = PR.lattice_hypotheses(pts, 600, seed=10)
    ref = check_consensus(pts, w, 0.25, hyp, 2.0 ** -5, 1e-6)
    assert ref["best"][1] > 5000 and ref["on_limit"] > 100
    a = call_consensus(pts, w, 0.25, hyp, 2.0 ** -5, 1e-6, garbage=1)
    b = call_consensus(pts, w, 0.25, hyp, 2.0 ** -5, 1e-6, garbage=2)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)


# ------------------------------------------------------------------------------------------------
# 3. classify
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 4099, 16384, 16385, 32769])
def test_classify_is_exact_on_the_lattice(n):
    """plane z = 0, dist 2^-5: a quarter of the points lie exactly at +-dist, and they are "on".  Every term is a
    multiple of 2^-14 below 2: the sums are exact in any order.  16384, 16385 and 32769 points are 16, 17 and 33 slab
    rows: sp_finish_kernel's 16 chains take one, two and three rows."""
    pts, w = PR.lattice_scene(n, seed=100 + n)
    if n > 10:
        pts[3], pts[7, 1] = (np.inf, 0.0, 0.0), np.nan
    ref, _ = check_classify(pts, w, 0.25, (0.0, 0.0, 1.0, 0.0), (2.0 ** -7, 0.0, -2.0 ** -7), 2.0 ** -5,
                            exact_sums=True)
    if n >= 1023:
        z = pts[:, 2].astype(np.float64)
        at = np.isfinite(pts).all(1) & (w > 0.25) & (np.abs(z) == 2.0 ** -5)
        assert at.sum() > 50 and (ref["side"][at] == 1).all()
        assert set(ref["side"].tolist()) == {0, 1, 2, 3} and np.isnan(ref["height"][[3, 7]]).all()
    check_classify(pts, None, 0.0, (0.0, 0.0, -1.0, 2.0 ** -6), (0.0, 0.0, 0.0), 0.0, exact_sums=True)


@gpu
def test_classify_on_the_table_scene():
    pts = PR.table_scene()[0]
    rng = np.random.default_rng(3)
    w = rng.uniform(0.05, 1.0, len(pts)).astype(np.float32)
    plane = (*PR.TRUE_NORMAL, PR.TRUE_OFFSET)
    ref, s = check_classify(pts, w, 0.1, plane, pts[0].astype(np.float64), 0.004)
    assert ref["sums"][0] > 2500 and ref["sums"][1] > ref["sums"][2] > 0
    assert np.abs(np.abs(ref["h"]) - 0.004).min() > 1e-9              # no label is a matter of rounding
    # nothing on the plane: the moments are sums over nothing
    far, s = check_classify(pts, w, 0.1, (0.0, 0.0, 1.0, 5.0), (0.0, 0.0, 0.0), 0.004)
    assert far["sums"][0] == 0 and far["sums"][2] == 0 and (s[3:14] == 0.0).all()


# ------------------------------------------------------------------------------------------------
# 4. fit_plane
# ------------------------------------------------------------------------------------------------
@gpu
def test_fit_plane_on_the_table_scene():
    from gaussiangrasper_amd import support
    pts = PR.table_scene()[0]
    ref = PR.fit_plane(pts, num_hypotheses=256, **FIT)
    diff = PR.order_difference(pts, num_hypotheses=256, **FIT)
    got = support.fit_plane(torch.from_numpy(pts).to(DEV), None, num_hypotheses=256, **FIT)
    dn, do = float(np.abs(got.normal - ref["normal"]).max()), abs(got.offset - ref["offset"])
    print(f"fit_plane against the restatement: normal {dn:.3e}, offset {do:.3e}; the order of the sums alone: "
          f"{diff:.3e}")
    assert got.best == ref["best"] and got.hypothesis_count == ref["hypothesis_count"] and got.status == "ok"
    assert (got.count_on, got.count_above, got.count_below) == ref["counts"]
    assert got.side.dtype == torch.uint8 and np.array_equal(got.side.cpu().numpy(), ref["side"])
    assert diff > 0.0 and dn <= 4 * diff and do <= 4 * diff
    assert abs(got.rmse - ref["rmse"]) <= 1e-12 * ref["rmse"] and got.dist == 0.004
    assert np.abs(got.height.cpu().numpy().astype(np.float64) - ref["height"]).max() <= 2.0 ** -24
    # without up: the same plane, pointing to the heavier side (the box, the wall and most of the clutter)
    free = support.fit_plane(torch.from_numpy(pts).to(DEV), None, dist=0.004, num_hypotheses=256)
    fref = PR.fit_plane(pts, dist=0.004, num_hypotheses=256)
    assert free.best == fref["best"] and np.array_equal(free.side.cpu().numpy(), fref["side"])
    assert free.normal @ PR.TRUE_NORMAL > 0.999 and free.count_above > free.count_below
    # weights: with the table's points switched off the wall is the plane
    w = torch.ones(len(pts), device=DEV)
    w[:3000] = 0.0
    wall = support.fit_plane(torch.from_numpy(pts).to(DEV), w, dist=0.004, num_hypotheses=1024)
    wref = PR.fit_plane(pts, w.cpu().numpy(), dist=0.004, num_hypotheses=1024)
    assert wall.best == wref["best"] and np.array_equal(wall.side.cpu().numpy(), wref["side"])
    assert wall.normal[0] < -0.999 and wall.count_on >= 800 and int((wall.side == 3).sum()) == 3000
    with pytest.raises(ValueError, match="valid"):
        support.fit_plane(torch.from_numpy(pts).to(DEV), torch.zeros(len(pts), device=DEV), num_hypotheses=16)


# ------------------------------------------------------------------------------------------------
# 5. the grasp layer
# ------------------------------------------------------------------------------------------------
@gpu
def test_plane_clear_on_the_device_equals_the_restatement():
    from gaussiangrasper_amd import support
    from gaussiangrasper_amd.grasp import default_gripper, plane_clear
    rows = PR.clear_rows(512, seed=11)
    plane = support.SupportPlane(normal=PR.TRUE_NORMAL, offset=PR.TRUE_OFFSET, dist=0.004)
    rc, rl = PR.plane_clear(rows, default_gripper(), plane.normal, plane.offset, 0.05, 0.0)
    assert np.abs(rl).min() > 1e-9 and 100 < rc.sum() < 412            # no row within 1e-9 of the margin
    c, lo = plane_clear(torch.from_numpy(rows).to(DEV), default_gripper(), plane, approach=0.05)
    assert c.device.type == "cuda" and lo.dtype == torch.float64
    assert np.array_equal(c.cpu().numpy(), rc) and (np.abs(lo.cpu().numpy() - rl) <= 1e-12 * (1 + np.abs(rl))).all()


def _table_model():
    """The table scene's table and box as flat discs whose smallest axis is the outward normal.  Returns (Scene,
    object mask (N,) bool)."""
    from gaussiangrasper_amd.scene import make_scene
    pts, nrm, kind = PR.table_scene()
    keep = kind <= 1
    p, n = pts[keep], nrm[keep]
    sc = make_scene(len(p), feature_dim=32)
    # the rotation that takes z to n, as (w, x, y, z): (1 + n_z, z x n) normalised
    q = np.column_stack([1.0 + n[:, 2], -n[:, 1], n[:, 0], np.zeros(len(n))])
    flip = q[:, 0] < 1e-9                                              # n = -z: half a turn about x
    q[flip] = (0.0, 1.0, 0.0, 0.0)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    sc.means = torch.from_numpy(p.astype(np.float32))
    sc.quats = torch.from_numpy(q.astype(np.float32))
    sc.scales = torch.log(torch.tensor([0.004, 0.004, 0.0004])).expand(len(p), 3).contiguous()
    sc.opacities = torch.full((len(p), 1), 4.0)
    return sc, kind[keep] == 1


@gpu
def test_grasp_object_with_a_support_plane_keeps_the_gripper_above_it():
    from gaussiangrasper_amd import support
    from gaussiangrasper_amd.grasp import default_gripper
    from gaussiangrasper_amd.grasp_propose import grasp_object
    sc, mask = _table_model()
    sc = sc.to(DEV)
    m = torch.from_numpy(mask).to(DEV)
    plane = support.support_plane(sc, m, dist=0.004, num_hypotheses=256, up=(0.0, 0.0, 1.0))
    assert plane.normal @ PR.TRUE_NORMAL > 0.9999 and plane.side.shape == (len(mask),)
    lifted = support.above(m, plane)
    assert 0 < int(lifted.sum()) < int(m.sum()) and not bool((lifted & ~m).any())      # the bottom face goes
    kw = dict(num_approach=8, up=plane.normal, max_seeds=256)
    rows0, res0, keep0 = grasp_object(sc, m, **kw)
    rows1, res1, keep1 = grasp_object(sc, m, gripper=default_gripper(), approach=0.05, **kw)
    margin = 0.002
    rows, res, keep = grasp_object(sc, m, gripper=default_gripper(), approach=0.05, support=plane,
                                   support_margin=margin, **kw)
    assert torch.equal(rows, rows0) and torch.equal(rows, rows1)
    assert res.support_clear is not None and res.support_lowest.dtype == torch.float64
    low, k = res.support_lowest.cpu().numpy(), keep.cpu().numpy()
    assert len(k) >= 1 and (low[k] >= margin).all()
    rc, rl = PR.plane_clear(rows.cpu().numpy(), default_gripper(), plane.normal, plane.offset, 0.05, margin)
    assert np.abs(rl - margin).min() > 1e-9 and np.array_equal(res.support_clear.cpu().numpy(), rc)
    assert np.array_equal(res.feasible.cpu().numpy(), res1.feasible.cpu().numpy() & rc)
    assert set(k.tolist()) <= set(keep1.cpu().numpy().tolist())
    # the plane takes out approaches the opacity test let through or not: some row is under the plane
    assert (~rc).any() and (low[keep0.cpu().numpy()] < margin).any()
    # with a tilt limit the kept rows come down within it
    _, res_t, keep_t = grasp_object(sc, m, gripper=default_gripper(), approach=0.05, support=plane,
                                    support_margin=margin, max_approach_tilt=math.radians(45.0), **kw)
    a = rows.cpu().numpy()[:, [4, 7, 10]].astype(np.float64)
    kt = keep_t.cpu().numpy()
    assert (-(a[kt] @ plane.normal) >= math.cos(math.radians(45.0))).all() and set(kt.tolist()) <= set(k.tolist())
    # without support: exactly what it returned before, and no new field set
    rows2, res2, keep2 = grasp_object(sc, m, gripper=default_gripper(), approach=0.05, **kw)
    assert torch.equal(rows2, rows1) and torch.equal(keep2, keep1) and torch.equal(res2.feasible, res1.feasible)
    assert res1.support_clear is None and res1.support_lowest is None and res0.support_clear is None
