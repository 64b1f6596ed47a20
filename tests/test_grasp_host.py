"""No-GPU checks of grasp filtering (gaussiangrasper_amd.grasp, gg_grasp_contacts): the C entry's argument validation
and workspace query, the candidate loader and frame change against closed forms, the score ordering of
filter_grasps, the command-line tool's argument errors, and the fp64 restatement (tests/grasp_ref.py) against
hand-worked cases."""
import ctypes
import json
import math
import threading

import numpy as np
import pytest
import torch

from grasp_ref import grasp_rows, restate

D = ctypes.c_double


def _call_on_thread(fn, cases):
    got = []

    def run():
        for args in cases:
            got.append(fn(args))
    t = threading.Thread(target=run)        # gg_last_error is per thread: the message does not outlive the test
    t.start()
    t.join()
    return got


def test_grasp_argument_validation_without_a_gpu():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    n = ctypes.c_void_p(0)
    f = ctypes.c_void_p(1 << 20)        # never dereferenced: every call below fails validation first
    ok = (0.02, 0.004, 0.003, 0.5, 0.0, math.inf)

    def args(num_points=10, pts=f, nrm=f, w=f, num_grasps=4, grasps=f, params=ok, outs=(f,) * 7, ws=f, ws_bytes=1 << 30):
        return (num_points, pts, nrm, w, num_grasps, grasps, *map(D, params), *outs, ws, ctypes.c_size_t(ws_bytes), n)

    def p(**kw):
        d = dict(zip(("depth_base", "finger_width", "band", "mu", "min_weight", "max_collision"), ok))
        d.update(kw)
        return tuple(d.values())
    cases = [
        (args(num_points=-1), b"num_points"),
        (args(num_grasps=-3), b"num_grasps"),
        (args(num_grasps=(1 << 20) + 1), b"GG_GRASP_MAX"),
        (args(params=p(band=-1e-3)), b"band"),
        (args(params=p(band=math.nan)), b"band"),
        (args(params=p(band=math.inf)), b"band"),
        (args(params=p(mu=-0.1)), b"mu"),
        (args(params=p(mu=math.inf)), b"mu"),
        (args(params=p(depth_base=-0.02)), b"depth_base"),
        (args(params=p(depth_base=math.nan)), b"depth_base"),
        (args(params=p(finger_width=-1.0)), b"finger_width"),
        (args(params=p(min_weight=math.nan)), b"min_weight"),
        (args(params=p(max_collision=math.nan)), b"max_collision"),
        (args(grasps=n), b"null pointer"),
        (args(outs=(f, f, n, f, f, f, f)), b"null pointer"),
        (args(outs=(f,) * 6 + (n,)), b"null pointer"),
        (args(pts=n), b"null pointer"),
        (args(nrm=n), b"null pointer"),
        (args(w=n), b"null pointer"),
        (args(pts=ctypes.c_void_p((1 << 20) + 2)), b"misaligned"),
        (args(ws=n), b"ws"),
        (args(ws=ctypes.c_void_p((1 << 20) + 16)), b"ws"),
    ]
    got = _call_on_thread(lambda a: (lib.gg_grasp_contacts(*a), lib.gg_last_error()), [c[0] for c in cases])
    for (st, msg), (_, want) in zip(got, cases):
        assert st == -1 and msg.startswith(b"gg_grasp_contacts") and want in msg, msg
    # a workspace one byte short is refused before any launch
    need = lib.gg_grasp_contacts_workspace(10, 4)
    (st, msg), = _call_on_thread(lambda a: (lib.gg_grasp_contacts(*a), lib.gg_last_error()),
                                 [args(ws_bytes=need - 1)])
    assert st == -3 and b"workspace" in msg
    # no grasps: nothing to do, null outputs accepted; no points with null point arrays passes validation too
    assert lib.gg_grasp_contacts(*args(num_grasps=0, grasps=n, outs=(n,) * 7, ws=n, ws_bytes=0)) == 0


def test_workspace_query():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    ws = lib.gg_grasp_contacts_workspace
    assert ws(-1, 5) == 0 and ws(10, -1) == 0 and ws(10, 0) == 0 and ws(10, (1 << 20) + 1) == 0
    assert ws((1 << 30) + 1, 5) == 0
    assert ws(0, 5) > 0                              # per-grasp state, no chunks
    assert ws(1, 5) > ws(0, 5)
    assert ws(300_000, 1000) >= ws(50_000, 1000) >= ws(1, 1000)
    # bounded: the chunk count falls as the grasp tiles rise (about 2048 workgroups per pass)
    assert ws(5_000_000, 65536) < 200 << 20 and ws(5_000_000, 1024) < 200 << 20


def test_contacts_refuses_host_tensors():
    from gaussiangrasper_amd.grasp import contacts
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        contacts(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4), torch.zeros(2, 17))


# ------------------------------------------------------------------------------------------------
# candidates and frames
# ------------------------------------------------------------------------------------------------
def test_load_grasps_checks_the_shape(tmp_path):
    from gaussiangrasper_amd.grasp import load_grasps
    g = np.random.default_rng(0).normal(size=(5, 17))
    np.save(tmp_path / "g.npy", g)
    got = load_grasps(str(tmp_path / "g.npy"))
    assert got.dtype == np.float32 and got.shape == (5, 17) and np.array_equal(got, g.astype(np.float32))
    for bad in (np.zeros((5, 16)), np.zeros(17), np.zeros((2, 3, 17))):
        np.save(tmp_path / "b.npy", bad)
        with pytest.raises(ValueError, match="17"):
            load_grasps(str(tmp_path / "b.npy"))


def _rz(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def test_grasps_to_scene_closed_forms():
    from gaussiangrasper_amd.grasp import grasps_to_scene
    R = np.stack([np.eye(3), _rz(30.0)])
    g = grasp_rows(R, [[0.1, 0.2, 0.3], [-0.5, 0.25, 1.0]], [0.04, 0.08], 0.02, [0.01, 0.03], object_id=7)
    # identity
    assert np.array_equal(grasps_to_scene(g), g)
    # a 90 degree turn about z: (x, y, z) -> (-y, x, z), rotations composed on the left
    C = np.eye(4)
    C[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    C[:3, 3] = [1.0, 2.0, 3.0]
    got = grasps_to_scene(g, cam_to_world=C)
    assert np.allclose(got[:, 13:16], [[1.0 - 0.2, 2.0 + 0.1, 3.3], [1.0 - 0.25, 2.0 - 0.5, 4.0]], atol=1e-6)
    assert np.allclose(got[1, 4:13].reshape(3, 3), _rz(120.0), atol=1e-6)
    assert np.array_equal(got[:, [0, 1, 2, 3, 16]], g[:, [0, 1, 2, 3, 16]])
    # scale 2 with the scene matrix: t' = 2 (M3 (C3 t + C_t) + M_t); sizes doubled, R' = M3 C3 R
    M = np.eye(4)
    M[:3, :3] = _rz(-90.0)
    M[:3, 3] = [0.5, 0.0, -0.5]
    got = grasps_to_scene(g, C, M, 2.0)
    t_world = np.array([[0.8, 2.1, 3.3], [0.75, 1.5, 4.0]])
    assert np.allclose(got[:, 13:16], 2.0 * (t_world @ _rz(-90.0).T + [0.5, 0.0, -0.5]), atol=1e-6)
    assert np.allclose(got[:, 1:4], 2.0 * g[:, 1:4].astype(np.float64), rtol=1e-7)
    assert np.allclose(got[0, 4:13].reshape(3, 3), np.eye(3), atol=1e-6)      # -90 after +90
    assert got[0, 0] == g[0, 0] and got[1, 16] == 7


def test_grasps_to_scene_rejects_non_orthonormal_rotations():
    from gaussiangrasper_amd.grasp import grasps_to_scene
    g = grasp_rows(np.eye(3)[None], [[0, 0, 0]], 0.04, 0.02, 0.01)
    bad = g.copy()
    bad[0, 4] = 1.001                                    # R[0][0] scaled by 1.001
    with pytest.raises(ValueError, match="grasp rotation"):
        grasps_to_scene(bad)
    almost = g.copy()
    almost[0, 4] = 1.00001                               # within 1e-4
    grasps_to_scene(almost)
    C = np.eye(4)
    C[0, 1] = 0.01
    with pytest.raises(ValueError, match="cam_to_world"):
        grasps_to_scene(g, cam_to_world=C)
    with pytest.raises(ValueError, match="matrix"):
        grasps_to_scene(g, matrix=2.0 * np.eye(4))
    with pytest.raises(ValueError, match="scale"):
        grasps_to_scene(g, scale=0.0)
    nan_row = np.concatenate([g, np.full((1, 17), np.nan, np.float32)])     # not valid, not an error
    assert np.isnan(grasps_to_scene(nan_row)[1]).all()


def test_filter_grasps_sorts_by_score_stably():
    from gaussiangrasper_amd.grasp import filter_grasps
    g = np.zeros((8, 17), np.float32)
    g[:, 0] = [0.5, 0.9, 0.5, 0.1, 0.9, 0.7, 0.5, 0.95]
    feas = torch.tensor([1, 1, 1, 1, 1, 0, 1, 0], dtype=torch.bool)
    got = filter_grasps(g, feas)
    assert got.tolist() == [1, 4, 0, 2, 6, 3]
    assert filter_grasps(g, torch.zeros(8, dtype=torch.bool)).tolist() == []
    with pytest.raises(ValueError, match="match"):
        filter_grasps(g, torch.ones(7, dtype=torch.bool))


# ------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------
def test_cli_argument_errors(tmp_path):
    from gaussiangrasper_amd import grasp
    g = tmp_path / "g.npy"
    np.save(g, grasp_rows(np.eye(3)[None], [[0, 0, 0]], 0.04, 0.02, 0.01))
    out = str(tmp_path / "kept.npy")
    base = ["--ckpt", str(tmp_path / "none.ckpt"), "--grasps", str(g), "--out", out]
    with pytest.raises(SystemExit):                                   # --grasps is required
        grasp.main(["--ckpt", "x.ckpt", "--out", out])
    with pytest.raises(SystemExit):                                   # alternatives
        grasp.main(base + ["--object-points", "o.npy", "--positives", "p.npy", "--negatives", "n.npy",
                           "--threshold", "0.5"])
    with pytest.raises(SystemExit):
        grasp.main(base + ["--positives", "p.npy", "--negatives", "n.npy"])       # no threshold
    with pytest.raises(SystemExit):
        grasp.main(base + ["--threshold", "0.5"])                                  # no positives
    for opt, v in (("--mu", "-1"), ("--band", "nan"), ("--min-opacity", "-0.5"), ("--max-collision", "nan")):
        with pytest.raises(SystemExit):
            grasp.main(base + [opt, v])
    np.save(tmp_path / "bad.npy", np.zeros((3, 16), np.float32))
    with pytest.raises(SystemExit, match="17"):
        grasp.main(["--ckpt", "x.ckpt", "--grasps", str(tmp_path / "bad.npy"), "--out", out])
    np.save(tmp_path / "pose.npy", np.eye(3))
    with pytest.raises(SystemExit, match="camera pose"):
        grasp.main(base + ["--camera-pose", str(tmp_path / "pose.npy")])
    (tmp_path / "tj.json").write_text(json.dumps({"scale": 1.0}))
    with pytest.raises(SystemExit, match="transform_matrix"):
        grasp.main(base + ["--transform-json", str(tmp_path / "tj.json")])
    with pytest.raises(SystemExit, match="error"):                    # no such checkpoint
        grasp.main(base)
    assert not (tmp_path / "kept.npy").exists()


# ------------------------------------------------------------------------------------------------
# the restatement against hand-worked cases
# ------------------------------------------------------------------------------------------------
def _one(points, normals, weights, R=np.eye(3), t=(0.0, 0.0, 0.0), width=0.04, height=0.02, depth=0.01, **kw):
    g = grasp_rows(np.asarray(R)[None], [t], width, height, depth)
    r = restate(np.asarray(points, np.float32), np.asarray(normals, np.float32), np.asarray(weights, np.float32),
                g, **kw)
    return {k: v[0] for k, v in r.items()}


def test_restatement_two_contacts_with_opposed_normals():
    # identity frame: u = p - t; a = x (approach), b = y (closing), c = z; width 0.04 -> |u1| <= 0.02
    P = [[0.0, -0.015, 0.0], [0.0, 0.0125, 0.001], [0.005, 0.0, 0.0]]
    N = [[0.0, 1.0, 0.0], [0.0, 2.0, 0.0], [1.0, 0.0, 0.0]]        # any sign, any length
    r = _one(P, N, [0.5, 0.25, 1.0])
    assert r["region_count"] == 3 and list(r["contact_idx"]) == [0, 1]
    assert r["region_weight"] == 1.75 and r["collision_weight"] == 0.0
    # left patch u1 <= -0.012: point 0 only, oriented toward -y; right patch u1 >= 0.0095: point 1, toward +y
    assert np.allclose(r["normals"], [[0, -1, 0], [0, 1, 0]])
    assert np.allclose(r["angles"], 0.0) and r["valid"] and r["feasible"]


def test_restatement_friction_cone_edge():
    # the right normal tilted 30 deg from b: beyond atan(0.5) = 26.57 deg, inside atan(0.6) = 30.96 deg
    s, c = math.sin(math.radians(30)), math.cos(math.radians(30))
    P = [[0.0, -0.015, 0.0], [0.0, 0.015, 0.0]]
    N = [[0.0, -1.0, 0.0], [s, c, 0.0]]
    r = _one(P, N, [1.0, 1.0])
    assert r["valid"] and not r["feasible"]
    assert abs(r["angles"][0]) < 1e-12 and abs(r["angles"][1] - math.radians(30)) < 1e-6    # fp32 normal
    assert _one(P, N, [1.0, 1.0], mu=0.6)["feasible"]


def test_restatement_boxes_and_participation():
    # dyadic sizes so that every edge is exact: w/2 = 2^-6, fw = 2^-8, h/2 = depth = 2^-7, depth_base = 2^-6
    hw, fw, hh, db = 2.0 ** -6, 2.0 ** -8, 2.0 ** -7, 2.0 ** -6
    e = 2.0 ** -12
    P = [[0.0, -hw, 0.0],           # region edge |u1| = w/2: region
         [0.0, hw + e, 0.0],        # right finger box
         [0.0, -hw - fw, 0.0],      # left finger box edge -w/2 - fw: in
         [0.0, hw + fw + e, 0.0],   # beyond the finger: nowhere
         [-db, 0.0, 0.0],           # u0 = -depth_base: region
         [hh + e, 0.0, 0.0],        # u0 > depth: nowhere
         [0.0, 0.0, -hh - e],       # |u2| > h/2: nowhere
         [0.0, e, 0.0],             # NaN normal: takes no part
         [0.0, 2 * e, 0.0]]         # weight 0 (not > min_weight 0): takes no part
    N = [[0, 1, 0]] * 7 + [[np.nan, 0, 0], [0, 1, 0]]
    W = [1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, 0.0]
    kw = dict(width=2 * hw, height=2 * hh, depth=hh, finger_width=fw, depth_base=db)
    r = _one(P, N, W, **kw)
    assert r["region_count"] == 2 and r["region_weight"] == 17.0 and r["collision_weight"] == 6.0
    assert list(r["contact_idx"]) == [0, 4]
    assert not _one(P, N, W, max_collision=5.0, **kw)["feasible"]
    assert _one(P, N, W, max_collision=6.0, **kw)["feasible"]


def test_restatement_ties_empty_single_and_bad_rows():
    P = [[0.0, 0.01, 0.0], [0.0, -0.01, 0.0], [0.001, -0.01, 0.0], [0.0, 0.01, 0.001]]
    N = [[0, 1, 0]] * 4
    r = _one(P, N, [1.0] * 4)
    assert list(r["contact_idx"]) == [1, 0]                            # ties: the smallest index
    r = _one([[0.0, 0.001, 0.0]], [[0, 1, 0]], [1.0])                 # one point: y_L == y_R, not valid
    assert r["region_count"] == 1 and list(r["contact_idx"]) == [0, 0] and not r["valid"]
    assert np.isnan(r["angles"]).all() and not r["feasible"]
    r = _one([[1.0, 1.0, 1.0]], [[0, 1, 0]], [1.0])                   # empty region
    assert r["region_count"] == 0 and list(r["contact_idx"]) == [-1, -1] and not r["valid"]
    for w, h, d in ((0.0, 0.02, 0.01), (0.04, -0.02, 0.01), (0.04, 0.02, -0.03)):
        r = _one(P, N, [1.0] * 4, width=w, height=h, depth=d)
        assert r["region_count"] == 0 and not r["valid"]
