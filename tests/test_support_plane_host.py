"""No-GPU checks of the support plane: the fp64 restatement (tests/plane_ref.py) on the table scene against the truth,
against a brute-force count and against an SVD fit; how far the order of a sum moves the fitted plane (printed; the GPU
test's bound is 4 x that); the C entries' argument checks and workspace queries; grasp.plane_clear on hand-built rows;
the plane file; and the command lines' cross-checks."""
import ctypes
import json
import math
import threading

import numpy as np
import pytest
import torch

import plane_ref as PR

D = ctypes.c_double
FIT = dict(dist=0.004, up=(0.0, 0.0, 1.0), max_tilt=math.radians(20.0))


def _angle_deg(n):
    c = abs(float(n @ PR.TRUE_NORMAL)) / math.sqrt(float(n @ n))
    return math.degrees(math.acos(min(1.0, c)))


@pytest.fixture(scope="module")
def scene():
    return PR.table_scene()


@pytest.fixture(scope="module")
def fits(scene):
    return {h: PR.fit_plane(scene[0], num_hypotheses=h, **FIT) for h in (64, 256)}


# ------------------------------------------------------------------------------------------------
# the restatement on the table scene
# ------------------------------------------------------------------------------------------------
def test_the_scene_is_a_pure_function_rounded_to_fp32(scene):
    pts, nrm, kind = scene
    again = PR.table_scene()[0]
    assert pts.dtype == np.float32 and pts.shape == (5500, 3) and np.array_equal(pts, again)
    assert np.bincount(kind).tolist() == [3000, 1200, 800, 500]
    h = pts[kind == 0].astype(np.float64) @ PR.TRUE_NORMAL + PR.TRUE_OFFSET
    assert 0.0008 < h.std() < 0.0012                                     # the 1 mm noise
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0)


@pytest.mark.parametrize("h", [64, 256])
def test_consensus_finds_the_table(scene, fits, h):
    con = fits[h]["consensus"]
    best, count = int(con["best"][0]), int(con["best"][1])
    hyp = np.random.default_rng(0).integers(0, 5500, size=(h, 3), dtype=np.int32)
    n, d = PR.plane_from_triple(*scene[0][hyp[best]].astype(np.float64))
    print(f"H = {h}: best {best} with {count} inliers, {_angle_deg(n):.3f} degrees from the truth, "
          f"{int(con['valid'].sum())} valid, gap {con['gap']:.3g}, on the limit {con['on_limit']}")
    assert count >= 2700 and _angle_deg(n) < 1.0                          # 1 mm noise in a 4 mm slab: most of 3000
    assert con["count"][con["valid"] == 0].sum() == 0
    # brute force, another formula: |P.n + d| / |n| <= dist, for every valid hypothesis
    p = scene[0].astype(np.float64)
    for k in np.nonzero(con["valid"])[0]:
        a, b, c = p[hyp[k]]
        nk = np.cross(b - a, c - a)
        brute = int((np.abs(p @ nk - nk @ a) / np.linalg.norm(nk) <= FIT["dist"]).sum())
        assert brute == con["count"][k], k
    # no (hypothesis, point) pair near enough to the limit for the two formulas, or any rounding, to disagree
    # gap is in squared distance: |h^2 - dist^2| = |h - dist| (h + dist) ~ 2 dist |h - dist|
    print(f"H = {h}: the nearest point is {con['gap'] / (2 * FIT['dist']):.3g} from the limit")
    assert con["gap"] / (2 * FIT["dist"]) > 1e-9


def test_refit_reaches_the_truth(scene, fits):
    for h, fit in fits.items():
        on, above, below = fit["counts"]
        ang = _angle_deg(fit["normal"])
        n = fit["normal"] if fit["normal"] @ PR.TRUE_NORMAL > 0 else -fit["normal"]
        # distance between the planes at the middle of the table
        mid = -PR.TRUE_OFFSET * PR.TRUE_NORMAL
        off = abs(float(n @ mid) + math.copysign(fit["offset"], fit["offset"] * float(n @ fit["normal"])))
        print(f"H = {h}: after two refits {ang:.5f} degrees and {off * 1e3:.4f} mm from the truth, "
              f"{on} on, {above} above, {below} below, rmse {fit['rmse'] * 1e3:.3f} mm, status {fit['status']}")
        assert fit["status"] == "ok" and fit["normal"] @ np.array(FIT["up"]) > 0
        assert ang <= 0.1 and off <= 0.0005
        assert on + above + below == 5500 and on >= 3000 and above > below > 0
        assert abs(float(fit["normal"] @ fit["normal"]) - 1.0) < 1e-14
        # no point within 1e-9 of +-dist of any plane a classify ran against: the labels are not a matter of rounding
        p = scene[0].astype(np.float64)
        for pn, po in fit["planes"]:
            hh = p @ pn + po
            assert np.abs(np.abs(hh) - FIT["dist"]).min() > 1e-9
        assert np.array_equal(fit["side"], np.where(np.abs(p @ fit["normal"] + fit["offset"]) <= FIT["dist"], 1,
                                                    np.where(p @ fit["normal"] + fit["offset"] > 0, 2, 0)))


def test_moments_equal_an_svd_fit(scene, fits):
    fit = fits[256]
    p = scene[0].astype(np.float64)
    pn, po = fit["planes"][-2]                                            # the plane the last refit started from
    inl = p[np.abs(p @ pn + po) <= FIT["dist"]]
    origin = inl[0]
    cl = PR.classify(scene[0], None, 0.0, [*pn, po], origin, FIT["dist"])
    assert int(cl["sums"][0]) == len(inl)
    n, d, status = PR.plane_from_moments(cl["sums"], origin, pn, po)
    c = inl.mean(axis=0)
    v = np.linalg.svd(inl - c)[2][2]
    v = v if v @ pn > 0 else -v
    assert status == "ok" and np.abs(n - v).max() < 1e-12 and abs(d + float(v @ c)) < 1e-12
    from gaussiangrasper_amd import support
    n2, d2, s2 = support.plane_from_moments(cl["sums"], origin, pn, po)
    assert s2 == "ok" and np.array_equal(n2, n) and d2 == d
    # fewer than three points, and points on a line: the previous plane stands
    n0, d0, s0 = support.plane_from_moments(np.zeros(16), origin, pn, po)
    assert np.array_equal(n0, pn) and d0 == po and s0 == "degenerate"
    line = np.outer(np.linspace(-1, 1, 9), [1.0, 2.0, 0.5]).astype(np.float32)
    cl = PR.classify(line, None, 0.0, [0.0, 0.0, 1.0, 0.0], np.zeros(3), 10.0)
    assert support.plane_from_moments(cl["sums"], np.zeros(3), [0.0, 0.0, 1.0], 0.0)[2] == "degenerate"
    assert PR.plane_from_moments(cl["sums"], np.zeros(3), [0.0, 0.0, 1.0], 0.0)[2] == "degenerate"


def test_order_of_the_sums_moves_the_plane_this_much(scene):
    """The figure the GPU test's bound is 4 x of (PARITY.md "Support plane")."""
    diff = PR.order_difference(scene[0], num_hypotheses=256, **FIT)
    print(f"pairwise against sequential moments: the fitted plane moves by {diff:.3e}")
    assert 0.0 < diff < 1e-12


def test_hypotheses_and_triples_are_pure_functions():
    from gaussiangrasper_amd import support
    a, b = support.draw_hypotheses(5500, 256, 0), support.draw_hypotheses(5500, 256, 0)
    assert a.dtype == np.int32 and a.shape == (256, 3) and np.array_equal(a, b)
    assert np.array_equal(a, np.random.default_rng(0).integers(0, 5500, size=(256, 3), dtype=np.int32))
    assert not np.array_equal(a, support.draw_hypotheses(5500, 256, 1))
    assert a.min() >= 0 and a.max() < 5500 and support.draw_hypotheses(3, 0, 0).shape == (0, 3)
    for bad in ((0, 4, 0), (10, -1, 0), (10, 65537, 0)):
        with pytest.raises(ValueError):
            support.draw_hypotheses(*bad)
    n, d = support.plane_from_triple([0, 0, 1], [0, 1, 1], [1, 0, 1])
    assert np.array_equal(n, [0.0, 0.0, 1.0]) and d == -1.0               # the largest component is positive
    rng = np.random.default_rng(2)
    for _ in range(20):
        t = rng.normal(size=(3, 3))
        n, d = support.plane_from_triple(*t)
        rn, rd = PR.plane_from_triple(*t)
        assert np.array_equal(n, rn) and d == rd and np.abs(t @ n + d).max() < 1e-14
    with pytest.raises(ValueError, match="span no plane"):
        support.plane_from_triple([0, 0, 0], [1, 1, 1], [2, 2, 2])
    assert support.check_up(None, None) == (None, 0.0)
    u, c2 = support.check_up((0, 0, 2), math.radians(60.0))
    assert u.tolist() == [0.0, 0.0, 2.0] and abs(c2 - 0.25) < 1e-15
    for up, tilt in (((0, 0, 0), None), (None, 0.1), ((0, 0, 1), -0.1), ((0, 0, 1), 2.0), ((0, math.nan, 1), None)):
        with pytest.raises(ValueError):
            support.check_up(up, tilt)


# ------------------------------------------------------------------------------------------------
# the C entries
# ------------------------------------------------------------------------------------------------
def _call_on_thread(fn, cases):
    got = []

    def run():
        for args in cases:
            got.append(fn(args))
    t = threading.Thread(target=run)        # gg_last_error is per thread: the message does not outlive the test
    t.start()
    t.join()
    return got


def test_workspace_queries_are_pure_host_calls():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    con, cla = lib.gg_plane_consensus_workspace, lib.gg_plane_classify_workspace
    assert con(-1, 4) == 0 and con(4, -1) == 0 and con((1 << 30) + 1, 4) == 0 and con(4, 65537) == 0
    assert con(0, 0) > 0 and con(1 << 30, 65536) == 65536 * 64
    for h in (1, 63, 64, 65, 300, 1024, 4096):
        assert con(1000, h) % 256 == 0 and con(1000, h) >= 56 * h and con(1000, h) == con(5, h)
    assert cla(-1) == 0 and cla((1 << 30) + 1) == 0 and cla(0) > 0
    for n in (1, 1024, 1025, 5_000_000):
        assert cla(n) % 256 == 0 and cla(n) >= (n + 1023) // 1024 * 128
    assert cla(1 << 30) == (1 << 20) * 128


def test_argument_validation_without_a_gpu():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    n = ctypes.c_void_p(0)
    f = ctypes.c_void_p(1 << 20)        # never dereferenced: every call below fails validation first
    up_ok, up_zero, up_nan = (D * 3)(0, 0, 1), (D * 3)(0, 0, 0), (D * 3)(0, math.nan, 1)

    def con(num_points=100, points=f, weights=f, min_weight=0.0, num_hyp=8, hyp=f, dist=0.01, min_sin2=1e-6,
            up=None, cos2=0.5, outs=(f, f, f), ws=f, ws_bytes=1 << 30):
        upp = None if up is None else ctypes.cast(up, ctypes.c_void_p)
        return (num_points, points, weights, D(min_weight), num_hyp, hyp, D(dist), D(min_sin2), upp, D(cos2), *outs,
                ws, ctypes.c_size_t(ws_bytes), n)
    cases = [
        (con(num_points=-1), b"num_points"),
        (con(num_points=(1 << 30) + 1), b"GG_GRASP_MAX_POINTS"),
        (con(num_hyp=-1), b"num_hypotheses"),
        (con(num_hyp=65537), b"GG_PLANE_MAX_HYPOTHESES"),
        (con(min_weight=math.nan), b"min_weight"),
        (con(dist=-1e-9), b"dist"),
        (con(dist=math.nan), b"dist"),
        (con(dist=math.inf), b"dist"),
        (con(min_sin2=1.0000001), b"min_sin2"),
        (con(min_sin2=-0.1), b"min_sin2"),
        (con(up=up_zero), b"up must not be zero"),
        (con(up=up_nan), b"up must be finite"),
        (con(up=up_ok, cos2=1.5), b"cos2_tilt"),
        (con(up=up_ok, cos2=math.nan), b"cos2_tilt"),
        (con(points=n), b"null pointer"),
        (con(hyp=n), b"null pointer"),
        (con(outs=(n, f, f)), b"null pointer"),
        (con(outs=(f, n, f)), b"null pointer"),
        (con(outs=(f, f, n)), b"null pointer"),
        (con(hyp=ctypes.c_void_p((1 << 20) + 2)), b"misaligned"),
        (con(ws=n), b"ws"),
        (con(ws=ctypes.c_void_p((1 << 20) + 16)), b"ws"),
    ]
    got = _call_on_thread(lambda a: (lib.gg_plane_consensus(*a), lib.gg_last_error()), [c[0] for c in cases])
    for (st, msg), (_, want) in zip(got, cases):
        assert st == -1 and msg.startswith(b"gg_plane_consensus") and want in msg, msg
    for st, msg in _call_on_thread(lambda a: (lib.gg_plane_consensus(*a), lib.gg_last_error()),
                                   [con(ws_bytes=lib.gg_plane_consensus_workspace(100, 8) - 1), con(ws_bytes=0)]):
        assert st == -3 and b"workspace" in msg
    # no hypothesis: nothing to do, null pointers accepted (weights may always be null)
    assert lib.gg_plane_consensus(*con(num_hyp=0, points=n, weights=n, hyp=n, outs=(n, n, n), ws=n, ws_bytes=0)) == 0

    plane_ok, plane_zero, plane_nan = (D * 4)(0, 0, 1, -0.2), (D * 4)(0, 0, 0, 1), (D * 4)(0, 0, 1, math.inf)
    org_ok, org_nan = (D * 3)(0, 0, 0), (D * 3)(math.nan, 0, 0)

    def cla(num_points=100, points=f, weights=f, min_weight=0.0, plane=plane_ok, origin=org_ok, dist=0.01,
            outs=(f, f, f), ws=f, ws_bytes=1 << 30):
        c = lambda a: None if a is None else ctypes.cast(a, ctypes.c_void_p)        # noqa: E731
        return (num_points, points, weights, D(min_weight), c(plane), c(origin), D(dist), *outs, ws,
                ctypes.c_size_t(ws_bytes), n)
    cases = [
        (cla(num_points=-1), b"num_points"),
        (cla(num_points=(1 << 30) + 1), b"GG_GRASP_MAX_POINTS"),
        (cla(min_weight=math.nan), b"min_weight"),
        (cla(dist=-1.0), b"dist"),
        (cla(dist=math.nan), b"dist"),
        (cla(plane=None), b"null pointer"),
        (cla(origin=None), b"null pointer"),
        (cla(plane=plane_zero), b"normal must not be zero"),
        (cla(plane=plane_nan), b"offset"),
        (cla(origin=org_nan), b"finite"),
        (cla(points=n), b"null pointer"),
        (cla(outs=(n, f, f)), b"null pointer"),
        (cla(outs=(f, n, f)), b"null pointer"),
        (cla(outs=(f, f, n)), b"null pointer"),
        (cla(outs=(f, f, ctypes.c_void_p((1 << 20) + 4))), b"misaligned"),
        (cla(ws=n), b"ws"),
    ]
    got = _call_on_thread(lambda a: (lib.gg_plane_classify(*a), lib.gg_last_error()), [c[0] for c in cases])
    for (st, msg), (_, want) in zip(got, cases):
        assert st == -1 and msg.startswith(b"gg_plane_classify") and want in msg, msg
    (st, msg), = _call_on_thread(lambda a: (lib.gg_plane_classify(*a), lib.gg_last_error()), [cla(ws_bytes=0)])
    assert st == -3 and b"workspace" in msg
    assert lib.gg_prof_name(52) == b"gg_support_plane(all launches)"
    assert lib.gg_prof_name(53) == b""
    assert lib.gg_abi_version() == 6


def test_the_calls_refuse_host_tensors_and_bad_arguments():
    from gaussiangrasper_amd import support
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        support.fit_plane(torch.zeros(10, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        support.classify(torch.zeros(10, 3), None, [0, 0, 1], 0.0, [0, 0, 0], 0.01)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        support.consensus(torch.zeros(10, 3), None, torch.zeros(4, 3, dtype=torch.int32), 0.01)


# ------------------------------------------------------------------------------------------------
# grasp.plane_clear, the plane file, the command lines
# ------------------------------------------------------------------------------------------------
def _row(R, t, width=0.06, height=0.02, depth=0.03):
    g = np.zeros(17, np.float32)
    g[0], g[1], g[2], g[3] = 0.5, width, height, depth
    g[4:13], g[13:16] = np.asarray(R, np.float64).reshape(9), t
    return g


def test_plane_clear_on_three_hand_built_rows():
    from gaussiangrasper_amd import support
    from gaussiangrasper_amd.grasp import default_gripper, plane_clear
    plane = support.SupportPlane(normal=np.array([0.0, 0.0, 1.0]), offset=0.0, dist=0.004)
    # row-major R, columns (a, b, c)
    down = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [-1.0, 0.0, 0.0]])        # a = (0, 0, -1): coming down
    up = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])            # a = (0, 0, 1): from under the plane
    assert abs(np.linalg.det(down) - 1) < 1e-15 and abs(np.linalg.det(up) - 1) < 1e-15
    rows = np.stack([
        _row(down, (0.0, 0.0, 0.10)),                # finger tips at 0.10 - 0.03 = 0.07: well above
        _row(down, (0.1, 0.0, 0.025)),               # finger tips at 0.025 - 0.03: 5 mm below the plane
        _row(up, (0.0, 0.1, 0.10)),                  # final pose above, but it sets out from 0.10 - 0.20 and below
    ])
    g = default_gripper()
    clear, lowest = plane_clear(torch.from_numpy(rows), g, plane, approach=0.2)
    assert clear.dtype == torch.bool and lowest.dtype == torch.float64 and clear.tolist() == [True, False, False]
    assert abs(float(lowest[0]) - 0.07) < 1e-8 and abs(float(lowest[1]) + 0.005) < 1e-8
    # the third row's lowest corner: the tail's far end at the approach start, 0.10 - 0.2 - (0.02 + 0.004 + 0.04)
    assert abs(float(lowest[2]) - (0.10 - 0.2 - 0.064)) < 1e-8
    rc, rl = PR.plane_clear(rows, g, plane.normal, plane.offset, 0.2)
    assert rc.tolist() == [True, False, False] and np.abs(rl - lowest.numpy()).max() < 1e-12
    # without the approach the third row is clear; a margin above its lowest corner takes the first row out
    assert plane_clear(torch.from_numpy(rows), g, plane, approach=0.0)[0].tolist() == [True, False, True]
    assert plane_clear(torch.from_numpy(rows), g, plane, 0.2, margin=0.08)[0].tolist() == [False, False, False]
    # scale: scene units per metre; the rows are scaled by the caller, the gripper, approach and margin here
    big = rows.copy()
    big[:, 1:4] *= 10.0
    big[:, 13:16] *= 10.0
    c10, l10 = plane_clear(torch.from_numpy(big), g, plane, approach=0.2, scale=10.0)
    assert c10.tolist() == [True, False, False] and np.abs(l10.numpy() - 10.0 * lowest.numpy()).max() < 1e-6
    # a row that is not finite is not clear; a gripper whose parts are all empty holds nothing under the plane
    bad = rows.copy()
    bad[0, 14] = np.nan
    assert plane_clear(torch.from_numpy(bad), g, plane)[0].tolist() == [False, False, True]
    empty = np.zeros((1, 6, 4))
    empty[0, 0, 0], empty[0, 1, 0] = 1.0, -1.0
    c, lo = plane_clear(torch.from_numpy(rows), empty, plane)
    assert c.all() and torch.isinf(lo).all()
    assert plane_clear(torch.zeros(0, 17), g, plane)[0].shape == (0,)
    with pytest.raises(ValueError):
        plane_clear(torch.zeros(3, 16), g, plane)


def test_plane_clear_equals_the_restatement_on_512_poses():
    from gaussiangrasper_amd import support
    from gaussiangrasper_amd.grasp import default_gripper, plane_clear
    rows = PR.clear_rows(512, seed=11)
    plane = support.SupportPlane(normal=PR.TRUE_NORMAL, offset=PR.TRUE_OFFSET, dist=0.004)
    rc, rl = PR.plane_clear(rows, default_gripper(), plane.normal, plane.offset, 0.05, 0.0)
    assert np.abs(rl).min() > 1e-9 and 100 < rc.sum() < 412           # no row on the margin; both outcomes common
    c, lo = plane_clear(torch.from_numpy(rows), default_gripper(), plane, approach=0.05)
    assert np.array_equal(c.numpy(), rc) and (np.abs(lo.numpy() - rl) <= 1e-12 * (1 + np.abs(rl))).all()


def test_score_grasps_and_grasp_object_want_a_gripper_with_a_plane():
    from gaussiangrasper_amd import support
    from gaussiangrasper_amd.grasp import GraspContacts, apply_support, score_grasps
    from gaussiangrasper_amd.grasp_propose import grasp_object
    plane = support.SupportPlane(normal=np.array([0.0, 0.0, 1.0]), offset=0.0, dist=0.01)
    with pytest.raises(ValueError, match="support needs gripper"):
        score_grasps(None, np.zeros((1, 17), np.float32), support=plane)
    with pytest.raises(ValueError, match="support needs gripper"):
        grasp_object(None, support=plane)
    f = GraspContacts.__dataclass_fields__
    assert f["support_clear"].default is None and f["support_lowest"].default is None
    res = GraspContacts(*([None] * 6), feasible=torch.ones(2, dtype=torch.bool))
    assert apply_support(res, None, None, None, 1.0, 0.0, 0.0, None) is res and res.support_clear is None
    with pytest.raises(ValueError, match="need support"):
        apply_support(res, None, None, None, 1.0, 0.0, 0.0, 0.3)
    # the tilt limit: a.(-n) >= cos(tilt)
    from gaussiangrasper_amd.grasp import default_gripper
    down = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [-1.0, 0.0, 0.0]])
    c, s = math.cos(math.radians(40.0)), math.sin(math.radians(40.0))
    tilted = np.array([[s, c, 0.0], [0.0, 0.0, -1.0], [-c, s, 0.0]])           # a = (s, 0, -c): 40 degrees off
    rows = torch.from_numpy(np.stack([_row(down, (0, 0, 0.2)), _row(tilted, (0, 0, 0.2))]))
    for tilt, want in ((math.radians(30.0), [True, False]), (math.radians(45.0), [True, True]), (None, [True, True])):
        res = GraspContacts(*([None] * 6), feasible=torch.ones(2, dtype=torch.bool))
        apply_support(res, rows, default_gripper(), plane, 1.0, 0.0, 0.0, tilt)
        assert res.feasible.tolist() == want and res.support_clear.tolist() == [True, True]


def test_plane_file_round_trip(tmp_path):
    from gaussiangrasper_amd import support
    n = np.array([0.05, -0.03, 1.0])
    p = support.SupportPlane(normal=n / np.linalg.norm(n), offset=-0.2000000000000123, dist=0.004, count_on=7)
    path = str(tmp_path / "plane.json")
    support.save_plane(path, p)
    assert sorted(json.load(open(path))) == ["dist", "normal", "offset"]
    q = support.load_plane(path)
    assert np.array_equal(q.normal, p.normal) and q.offset == p.offset and q.dist == p.dist
    assert q.side is None and q.height is None
    with pytest.raises(ValueError, match="no labels"):
        support.above(torch.ones(4, dtype=torch.bool), q)
    json.dump({"normal": [0, 0, 2.0], "offset": -1.0, "dist": 0.01}, open(path, "w"))
    q = support.load_plane(path)
    assert q.normal.tolist() == [0.0, 0.0, 1.0] and q.offset == -0.5                 # brought to unit length
    for bad in ({"normal": [0, 0, 0], "offset": 0, "dist": 0.01}, {"normal": [0, 0, 1], "offset": 0},
                {"normal": [0, 0, 1], "offset": 0, "dist": -1}, {"normal": [0, 1], "offset": 0, "dist": 0}):
        json.dump(bad, open(path, "w"))
        with pytest.raises(ValueError):
            support.load_plane(path)
    open(path, "w").write("not json")
    with pytest.raises(ValueError, match="not JSON"):
        support.load_plane(path)
    # above: mask & side == 2 & height > margin
    q.side = torch.tensor([2, 2, 1, 0, 3, 2], dtype=torch.uint8)
    q.height = torch.tensor([0.5, 0.02, 0.0, -0.3, 0.4, 0.3])
    m = torch.tensor([True, True, True, True, True, False])
    assert support.above(m, q).tolist() == [True, True, False, False, False, False]
    assert support.above(m, q, margin=0.1).tolist() == [True, False, False, False, False, False]


def test_command_lines_reject_incomplete_option_sets(capsys):
    from gaussiangrasper_amd import cluster, grasp, grasp_propose, support
    sel = ["--positives", "p.npy", "--negatives", "n.npy", "--threshold", "0.5"]
    base = ["--ckpt", "x.ckpt", "--out", "o.npy"]
    cases = [
        (grasp.main, base + ["--grasps", "g.npy", "--support-margin", "0.01"], "--support-margin needs --support-plane"),
        (grasp.main, base + ["--grasps", "g.npy", "--max-approach-tilt", "30"],
         "--max-approach-tilt needs --support-plane"),
        (grasp.main, base + ["--grasps", "g.npy", "--support-dist", "0.01"], "--support-dist needs --support-plane"),
        (grasp.main, base + ["--grasps", "g.npy", "--remove-support"] + sel, "--remove-support needs --support-plane"),
        (grasp.main, base + ["--grasps", "g.npy", "--support-plane", "fit"], "--support-plane needs --gripper"),
        (grasp.main, base + ["--grasps", "g.npy", "--support-plane", "fit", "--gripper", "default",
                             "--remove-support"], "--remove-support needs a selection"),
        (grasp.main, base + ["--grasps", "g.npy", "--support-plane", "fit", "--gripper", "default",
                             "--max-approach-tilt", "181"], "--max-approach-tilt must be in 0..180"),
        (grasp.main, base + ["--grasps", "g.npy", "--support-plane", "p.json", "--gripper", "default",
                             "--support-dist", "0.01"], "--support-dist goes with --support-plane fit"),
        (grasp_propose.main, base + sel + ["--support-plane", "fit"], "--support-plane needs --gripper"),
        (grasp_propose.main, base + sel + ["--remove-support"], "--remove-support needs --support-plane"),
        (grasp_propose.main, base + sel + ["--support-plane", "fit", "--gripper", "default", "--support-dist", "-1"],
         "--support-dist must be finite and >= 0"),
        (cluster.main, base + sel + ["--remove-support"], "--remove-support needs --support-plane"),
        (cluster.main, base + sel + ["--support-margin", "0.1"], "unrecognized arguments"),
        (support.main, ["--ckpt", "x.ckpt", "--out", "p.json", "--max-tilt", "20"], "--max-tilt needs --up"),
        (support.main, ["--ckpt", "x.ckpt", "--out", "p.json", "--up", "0", "0", "1", "--max-tilt", "91"],
         "--max-tilt must be in 0..90"),
        (support.main, ["--ckpt", "x.ckpt", "--out", "p.json", "--hypotheses", "0"], "--hypotheses must be in"),
        (support.main, ["--ckpt", "x.ckpt", "--out", "p.json", "--dist", "-0.01"], "--dist must be finite"),
    ]
    for main, argv, want in cases:
        with pytest.raises(SystemExit) as exc:
            main(argv)
        assert exc.value.code == 2 and want in capsys.readouterr().err, (argv, want)


def test_report_arrays_gain_the_support_arrays_only_when_present():
    from gaussiangrasper_amd._cli import REPORT_KEYS, report_arrays
    from gaussiangrasper_amd.grasp import GraspContacts
    res = GraspContacts(*[torch.zeros(2) for _ in REPORT_KEYS])
    assert sorted(report_arrays(res)) == sorted(REPORT_KEYS)
    res.support_clear, res.support_lowest = torch.tensor([True, False]), torch.tensor([0.1, -0.2], dtype=torch.float64)
    out = report_arrays(res)
    assert sorted(out) == sorted(REPORT_KEYS + ("support_clear", "support_lowest"))
    assert out["support_clear"].tolist() == [True, False] and out["support_lowest"].dtype == np.float64
