"""CPU checks of the scene-update masks (gaussiangrasper_amd.edit_masks): the host restatement (tests/objmask_ref.py)
against the reference's literal projection, scipy's ConvexHull, a brute-force point-in-polygon fill and
scipy.ndimage's dilation with cv2's anchor; degenerate hulls; the command line's argument errors, the output names
and per-frame intrinsics; and the C ABI of gg_object_masks without a GPU."""
import ctypes
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import objmask_ref as R


def _view(rng):
    c2w = R.ring(1, seed=int(rng.integers(1 << 30)))[0]
    return np.array([500.0 + rng.random(), 480.0 + rng.random(), 320.5, 239.25]), np.linalg.inv(c2w)


def test_projection_truncates_like_the_reference_expression():
    rng = np.random.default_rng(1)
    checked = 0
    for _ in range(5):
        K, E = _view(rng)
        p = rng.normal(scale=0.1, size=(5000, 3))
        ix, iy, kept = R.project(p, K, E[:3])
        assert kept.all()
        uv, lit = R.project_literal(p, K, E)
        far = (np.abs(uv - np.round(uv)) > 1e-9).all(axis=1)
        assert far.mean() > 0.99
        assert np.array_equal(ix[far], lit[far, 0]) and np.array_equal(iy[far], lit[far, 1])
        checked += int(far.sum())
    assert checked > 20000


def test_projection_drop_rule():
    K = np.array([100.0, 100.0, 10.0, 10.0])
    E = np.hstack([np.eye(3), np.zeros((3, 1))])
    p = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [np.nan, 0.0, 1.0], [np.inf, 0.0, 1.0],
                  [0.0, 0.0, np.inf], [2.0 ** 30 / 100, 0.0, 1.0], [-2.0 ** 30 / 100 + 1e-3, 0.0, 1.0],
                  [0.05, -0.07, 1.0]])
    ix, iy, kept = R.project(p, K, E)
    assert kept.tolist() == [True, False, False, False, False, False, False, True, True]
    # toward zero: u = -1073741813.9... -> -1073741813, v = 100 * -0.07 + 10 = 2.9999999999999991 -> 2
    assert ix.tolist() == [10, -1073741813, 15] and iy.tolist() == [10, 10, 2]


def test_hull_vertex_set_equals_scipy():
    from scipy.spatial import ConvexHull
    rng = np.random.default_rng(2)
    for trial in range(200):
        n = int(rng.integers(3, 60))
        span = int(rng.choice([5, 50, 10 ** 6, 2 ** 29]))
        xy = rng.integers(-span, span, size=(n, 2))
        if np.linalg.matrix_rank(xy[1:] - xy[0]) < 2:
            continue
        hull = R.convex_hull(xy)
        ref = {tuple(int(c) for c in xy[i]) for i in ConvexHull(xy.astype(np.float64)).vertices}
        assert set(hull) == ref, trial
        assert len(hull) == len(set(hull))
        for i in range(len(hull)):     # counter-clockwise, strictly convex
            assert R._cross(hull[i], hull[(i + 1) % len(hull)], hull[(i + 2) % len(hull)]) > 0


def _inside_brute(poly, x, y):
    """closed polygon membership, exact: on an edge, or ray casting with rationals"""
    n = len(poly)
    for i in range(n):
        (ax, ay), (bx, by) = poly[i], poly[(i + 1) % n]
        if (bx - ax) * (y - ay) - (by - ay) * (x - ax) == 0 and min(ax, bx) <= x <= max(ax, bx) \
                and min(ay, by) <= y <= max(ay, by):
            return True
    inside = False
    for i in range(n):
        (ax, ay), (bx, by) = poly[i], poly[(i + 1) % n]
        if (ay > y) != (by > y):
            xc = ax + Fraction((bx - ax) * (y - ay), by - ay)
            if x < xc:
                inside = not inside
    return inside


def test_fill_equals_brute_force_point_in_polygon():
    rng = np.random.default_rng(3)
    h, w = 23, 31
    for trial in range(25):
        n = int(rng.integers(3, 12))
        xy = np.stack([rng.integers(-8, w + 8, n), rng.integers(-8, h + 8, n)], 1)
        hull = R.convex_hull(xy)
        m = R.fill(hull, h, w)
        if len(hull) < 3:
            continue
        ref = np.array([[_inside_brute(hull, x, y) for x in range(w)] for y in range(h)])
        assert np.array_equal(m, ref), trial


def test_dilation_equals_scipy_with_the_cv2_anchor():
    from scipy import ndimage
    rng = np.random.default_rng(4)
    for k in range(0, 10):
        for shape in ((13, 17), (1, 1), (5, 2), (40, 9)):
            m = rng.random(shape) < 0.06
            m[0, 0] = True
            ref = m if k <= 1 else ndimage.binary_dilation(m, np.ones((k, k), bool), origin=-1 if k % 2 == 0 else 0)
            assert np.array_equal(R.dilate(m, k), ref), (k, shape)


def test_degenerate_hulls():
    h, w = 12, 15
    assert R.convex_hull([]) == [] and not R.fill([], h, w).any()
    assert R.convex_hull([(4, 5)] * 7) == [(4, 5)]
    m = R.fill(R.convex_hull([(4, 5)] * 7), h, w)
    assert m.sum() == 1 and m[5, 4]
    seg = R.convex_hull([(1, 1), (3, 2), (5, 3), (7, 4), (9, 5)])         # collinear: the end points
    assert seg == [(1, 1), (9, 5)]
    m = R.fill(seg, h, w)
    assert sorted(zip(*np.nonzero(m))) == [(1, 1), (2, 3), (3, 5), (4, 7), (5, 9)]
    m = R.fill(R.convex_hull([(2, 3), (2, 9), (2, 6)]), h, w)               # vertical
    assert m[:, 2].sum() == 7 and m.sum() == 7
    m = R.fill(R.convex_hull([(-5, 4), (40, 4)]), h, w)                     # horizontal, clipped
    assert m[4].all() and m.sum() == w
    assert R.box(np.zeros((3, 4), bool))[0].tolist() == [-1] * 4 and np.isnan(R.box(np.zeros((3, 4), bool))[1]).all()


def test_mask_stem_replaces_any_extension():
    from gaussiangrasper_amd.edit_masks import mask_stem
    assert mask_stem("images/frame_0001.png") == "frame_0001.npy"
    assert mask_stem("rgb/x.jpg") == "x.npy"
    assert mask_stem("a/b/c.d.jpeg") == "c.d.npy"
    assert mask_stem("noext") == "noext.npy"


def test_scan_cameras_follow_per_frame_intrinsics(tmp_path):
    from gaussiangrasper_amd.edit_masks import motion, scan_cameras
    from gaussiangrasper_amd.edit import pose_to_matrix
    c2w = R.ring(3, seed=5)
    meta = R.write_transforms(str(tmp_path / "t.json"), c2w, 30, 40, 50.0, 51.0, 20.0, 15.0,
                              overrides={1: {"fl_x": 77.0, "cy": 14.5}})
    intr, w2c, h, w = scan_cameras(meta)
    assert (h, w) == (30, 40)
    assert intr.tolist() == [[50.0, 51.0, 20.0, 15.0], [77.0, 51.0, 20.0, 14.5], [50.0, 51.0, 20.0, 15.0]]
    assert np.array_equal(w2c, np.array([np.linalg.inv(T) for T in c2w]))
    a, b = [0.1, 0.2, 0.0, 0.1, 0.0, 0.3], [0.0, 0.1, 0.2, 0.0, 0.2, 0.0]
    assert np.array_equal(motion(a, b), pose_to_matrix(b) @ np.linalg.inv(pose_to_matrix(a)))
    with pytest.raises(ValueError):
        scan_cameras({"w": 4, "h": 3, "frames": []})
    with pytest.raises(ValueError):
        scan_cameras({"h": 3, "frames": meta["frames"]})


def test_motion_matches_scipy_get_transform():
    from scipy.spatial.transform import Rotation
    from gaussiangrasper_amd.edit_masks import motion
    a, b = np.array([0.1, 0.2, 0.05, 0.3, -0.2, 0.1]), np.array([-0.1, 0.25, 0.1, 0.0, 0.4, -0.2])
    T1, T2 = np.eye(4), np.eye(4)
    T1[:3, :3], T1[:3, 3] = Rotation.from_rotvec(a[3:]).as_matrix(), a[:3]
    T2[:3, :3], T2[:3, 3] = Rotation.from_rotvec(b[3:]).as_matrix(), b[:3]
    assert np.abs(motion(a, b) - T2 @ np.linalg.inv(T1)).max() < 1e-14


def test_cli_argument_errors(tmp_path, capsys):
    from gaussiangrasper_amd.edit_masks import main
    base = ["--transforms", str(tmp_path / "t.json"), "--object-points", str(tmp_path / "o.txt"),
            "--pose-from", "0", "0", "0", "0", "0", "0", "--pose-to", "0", "0", "0", "0", "0", "0",
            "--out", str(tmp_path / "out")]
    with pytest.raises(SystemExit) as e:
        main(base[:4])                                             # required arguments missing
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        main(base + ["--dilate", "-1"])
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        main(base[:7] + ["0", "0"] + base[13:])                    # --pose-from with too few numbers
    assert main(base) == 2                                        # missing files: an error line, no traceback
    assert "error:" in capsys.readouterr().err
    np.savetxt(tmp_path / "o.txt", np.zeros((4, 2)))
    (tmp_path / "t.json").write_text(json.dumps({"w": 4, "h": 3, "frames": []}))
    assert main(base) == 2
    assert "error:" in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "out")


def test_abi_symbols_and_host_workspace_query():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "gg_object_masks") and hasattr(raw, "gg_object_masks_workspace")
    small, big = lib.gg_object_masks_workspace(1, 16384), lib.gg_object_masks_workspace(200, 16384)
    assert 2 * 16384 * 12 <= small < big and big >= 400 * 16384 * 12
    assert lib.gg_object_masks_workspace(0, 16) > 0
    assert lib.gg_object_masks_workspace(-1, 16) == 0 and lib.gg_object_masks_workspace(1, 0) == 0
    assert lib.gg_object_masks_workspace(1, 65537) == 0 and lib.gg_object_masks_workspace(16385, 16) == 0
    n = ctypes.c_void_p(0)
    T = (ctypes.c_double * 12)(*np.eye(3, 4).ravel())
    ws = ctypes.create_string_buffer(1024)
    assert lib.gg_object_masks(-1, n, T, 0, n, n, 4, 4, 0, 16, n, n, n, n, n, n, ws, 1024, n) == _lib.C.c_int(-1).value
    assert b"num_points" in lib.gg_last_error()
    assert lib.gg_object_masks(0, n, T, 0, n, n, 4, 4, -1, 16, n, n, n, n, n, n, ws, 1024, n) == -1
    assert b"dilate" in lib.gg_last_error()
    assert lib.gg_object_masks(0, n, T, 0, n, n, 0, 4, 0, 16, n, n, n, n, n, n, ws, 1024, n) == -1
    assert lib.gg_object_masks(0, n, None, 0, n, n, 4, 4, 0, 16, n, n, n, n, n, n, ws, 1024, n) == -1
    assert lib.gg_object_masks(0, n, T, 1, n, n, 4, 4, 0, 16, n, n, n, n, n, n, ws, 1024, n) == -1   # null outputs
    assert lib.gg_prof_name(39) == b"gg_object_masks(all launches)"
