"""GPU checks of the scene-update masks (gaussiangrasper_amd.edit_masks on gg_object_masks): bit-exact against the host
restatement of tests/objmask_ref.py — masks, boxes, centres and drop counts — for objects in view, partly and
entirely out of frame, points behind the camera, on its plane and not finite, hull vertices exactly on pixel centres,
degenerate hulls, odd and tiny image sizes, every dilation size of the contract and 300 views; the capacity error
with nothing written; a time guard; and the command-line tool end to end, twice, byte for byte."""
import ctypes
import json
import os
import time

import numpy as np
import pytest
import torch

import objmask_ref as R

gpu = pytest.mark.gpu


def _blob(rng, m, centre=(0.0, 0.0, 0.0), scale=0.05):
    return np.asarray(centre) + rng.normal(scale=scale, size=(m, 3)) * np.array([1.0, 0.6, 1.4])


def _motion(a=(0.02, -0.01, 0.03, 0.1, -0.2, 0.3), b=(0.1, 0.05, 0.0, -0.1, 0.1, 0.0)):
    from gaussiangrasper_amd.edit_masks import motion
    return motion(a, b)


def _cams(n, h, w, seed, target=(0.0, 0.0, 0.0), f=0.9):
    c2w = R.ring(n, seed=seed, target=target)
    rng = np.random.default_rng(seed)
    intr = np.array([[f * w + rng.random(), f * w + rng.random(), w / 2 + 0.3 * rng.normal(), h / 2 + 0.3 * rng.normal()]
                     for _ in range(n)])
    return intr, np.array([np.linalg.inv(T)[:3] for T in c2w])


def _aside(n, seed):
    """camera-to-world matrices on the ring that look 65-75 degrees past the origin: the object is in front of them
    and out of frame, with projections of a few hundred pixels"""
    rng = np.random.default_rng(seed)
    out = []
    for T in R.ring(n, seed=seed):
        eye = T[:3, 3]
        a = np.deg2rad(rng.uniform(65, 75)) * rng.choice([-1.0, 1.0])
        d = R.rodrigues([0.0, 0.0, a]) @ (-eye)
        out.append(R.look_at_c2w(eye, eye + d))
    return np.array(out)


def _check(points, T, intr, w2c, h, w, k, expect_empty=None, expect_drops=None):
    from gaussiangrasper_amd.edit_masks import object_masks
    got = object_masks(points, T, intr, w2c, h, w, dilate=k)
    torch.cuda.synchronize()
    ref = R.object_masks(points, T, intr, w2c, h, w, k)
    for name in ("before", "after", "union"):
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == bool and g.shape == ref[name].shape
        bad = np.nonzero((g != ref[name]).any(axis=(1, 2)))[0]
        assert bad.size == 0, f"{name}: views {bad[:10]} differ (k={k})"
    assert np.array_equal(got.boxes.cpu().numpy(), ref["boxes"])
    c = got.centres.cpu().numpy()
    assert np.array_equal(np.isnan(c), np.isnan(ref["centres"])) and np.array_equal(np.nan_to_num(c, nan=-7.0),
                                                                                      np.nan_to_num(ref["centres"],
                                                                                                    nan=-7.0))
    assert np.array_equal(got.dropped.cpu().numpy(), ref["dropped"])
    if expect_empty is not None:
        assert (ref["boxes"][:, 2, 0] < 0).sum() == expect_empty
    if expect_drops is not None:
        assert ref["dropped"].sum() == expect_drops
    return ref


@gpu
@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 7])
def test_random_objects_in_and_out_of_frame(k):
    rng = np.random.default_rng(10 + k)
    h, w = 37, 53
    pts = _blob(rng, 400)
    intr, w2c = _cams(12, h, w, seed=k)
    ref = _check(pts, _motion(), intr, w2c, h, w, k)
    assert ref["union"].sum() > 0 and (ref["boxes"][:, 2, 0] >= 0).all()
    # partly out of frame: the cameras look past the object
    intr, w2c = _cams(12, h, w, seed=k + 20, target=(0.12, 0.0, 0.05))
    ref = _check(pts, _motion(), intr, w2c, h, w, k)
    part = ref["union"].any(axis=(1, 2))
    assert part.any()
    # entirely out of frame in some views: the object in front of the camera, 65-75 degrees off its axis
    intr, w2c = _cams(6, h, w, seed=k + 40)
    w2c = np.concatenate([w2c, np.linalg.inv(_aside(6, k + 40))[:, :3]])
    intr = np.concatenate([intr, intr])
    ref = _check(pts, _motion(), intr, w2c, h, w, k)
    assert (ref["boxes"][6:, 2, 0] < 0).all() and (ref["boxes"][:6, 2, 0] >= 0).all()


@gpu
def test_points_behind_on_the_camera_plane_and_not_finite():
    h, w = 40, 50
    intr = np.array([[40.0, 40.0, 25.0, 20.0], [35.5, 41.0, 24.5, 19.5]])
    w2c = np.array([np.hstack([np.eye(3), np.zeros((3, 1))]), np.hstack([R.rodrigues([0.1, -0.2, 0.05]),
                                                                        [[0.01], [-0.02], [0.1]]])])
    rng = np.random.default_rng(3)
    pts = np.concatenate([_blob(rng, 50, (0.0, 0.0, 1.0), 0.2),
                          [[0.1, 0.1, 0.0], [0.0, 0.0, 0.0], [0.3, -0.2, -0.5], [0.1, 0.1, -1e-300],
                           [np.nan, 0.0, 1.0], [0.0, np.inf, 1.0], [0.0, 0.0, -np.inf], [1e300, 1e300, 1.0],
                           [1e-3, 0.0, 1e-12]]])
    ref = _check(pts, np.eye(4), intr, w2c, h, w, 0)
    assert ref["dropped"][0, 0] >= 9
    _check(pts, _motion(), intr, w2c, h, w, 3)


@gpu
def test_hull_vertices_on_pixel_centres_and_degenerate_hulls():
    # fx = fy = 1, cx = cy = 0, E = [I | 0], z = 1: u = x, v = y exactly, so every vertex lies on a pixel centre
    h, w = 37, 53
    intr = np.array([[1.0, 1.0, 0.0, 0.0]])
    E = np.array([np.hstack([np.eye(3), np.zeros((3, 1))])])
    shift = np.eye(4)
    shift[:3, 3] = [3.0, -2.0, 0.0]
    cases = {
        "triangle": [[2, 3], [40, 10], [15, 33]],
        "thin diagonal": [[0, 0], [52, 5]],
        "steep": [[5, 0], [7, 36]],
        "collinear": [[1, 1], [3, 2], [5, 3], [9, 5], [7, 4]],
        "vertical": [[10, 4], [10, 30], [10, 12]],
        "horizontal": [[-10, 8], [70, 8]],
        "single": [[20, 20]],
        "identical": [[11, 12]] * 9,
        "square on the border": [[0, 0], [52, 0], [52, 36], [0, 36]],
        "outside corners": [[-30, -30], [80, -5], [60, 70], [-5, 50]],
    }
    for name, xy in cases.items():
        pts = np.hstack([np.asarray(xy, np.float64), np.ones((len(xy), 1))])
        for k in (0, 2, 3):
            ref = _check(pts, shift, intr, E, h, w, k)
            assert ref["before"].any(), name
    # M = 1 and M = 3 with a motion that leaves the frame
    away = np.eye(4)
    away[:3, 3] = [500.0, 0.0, 0.0]
    _check(np.array([[4.0, 5.0, 1.0]]), away, intr, E, h, w, 0, expect_empty=0)
    _check(np.array([[4.0, 5.0, 1.0], [9.0, 5.0, 1.0], [4.0, 20.0, 1.0]]), away, intr, E, h, w, 4)
    _check(np.zeros((0, 3)), away, intr, E, h, w, 0, expect_empty=1)


@gpu
def test_tiny_and_non_square_images():
    rng = np.random.default_rng(5)
    pts = _blob(rng, 300)
    for h, w in ((1, 1), (1, 7), (9, 1), (37, 53), (53, 37), (2, 3)):
        intr, w2c = _cams(5, h, w, seed=h * 100 + w, f=1.5)
        for k in (0, 1, 2, 7):
            _check(pts, _motion(), intr, w2c, h, w, k)


@gpu
def test_many_points_and_300_views():
    rng = np.random.default_rng(6)
    pts = _blob(rng, 100_000)
    intr, w2c = _cams(8, 48, 64, seed=7)
    _check(pts, _motion(), intr, w2c, 48, 64, 3)
    pts = _blob(rng, 2000)
    intr, w2c = _cams(300, 24, 32, seed=8, target=(0.05, 0.0, 0.0))
    _check(pts, _motion(), intr, w2c, 24, 32, 2)


@gpu
def test_row_capacity_error_names_the_view_and_writes_nothing():
    from gaussiangrasper_amd import _lib
    from gaussiangrasper_amd.edit_masks import object_masks
    from gaussiangrasper_amd.ops import _ptr, _stream
    h, w = 30, 40
    intr = np.array([[1.0, 1.0, 0.0, 0.0]] * 5)
    E = np.array([np.hstack([np.eye(3), np.zeros((3, 1))])] * 5)
    E[3, 1, 1] = 50.0                 # view 3: rows 0 .. 500 — beyond max_rows = 64
    E[4, 1, 1] = 80.0                 # view 4 too; the first is named
    pts = np.array([[1.0, 0.0, 1.0], [2.0, 10.0, 1.0], [5.0, 6.0, 1.0]])
    with pytest.raises(_lib.GGError, match="view 3"):
        object_masks(pts, np.eye(4), intr, E, h, w, max_rows=64)
    dev = torch.device("cuda")
    lib = _lib.load()
    P, K, Ed = (torch.as_tensor(a, device=dev).contiguous() for a in (pts, intr, E[:, :3]))
    outs = [torch.full((5, h, w), 7, dtype=torch.uint8, device=dev) for _ in range(3)]
    boxes = torch.full((5, 3, 4), 7, dtype=torch.int32, device=dev)
    centres = torch.full((5, 3, 2), 7.0, dtype=torch.float64, device=dev)
    dropped = torch.full((5, 2), 7, dtype=torch.int32, device=dev)
    need = lib.gg_object_masks_workspace(5, 64)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    T = np.ascontiguousarray(np.eye(3, 4))
    st = lib.gg_object_masks(3, _ptr(P), T.ctypes.data_as(ctypes.c_void_p), 5, _ptr(K), _ptr(Ed), h, w, 0, 64,
                             _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(boxes), _ptr(centres), _ptr(dropped),
                             _ptr(ws), need, _stream(dev))
    assert st == -4 and b"view 3" in lib.gg_last_error()
    for t in outs + [boxes, dropped]:
        assert (t == 7).all()
    assert (centres == 7.0).all()
    # the same call with room enough succeeds and matches the restatement
    _check(pts, np.eye(4), intr, E[:, :3], h, w, 0)


@gpu
def test_time_guard_200_views_200k_points():
    from gaussiangrasper_amd.edit_masks import object_masks
    rng = np.random.default_rng(9)
    pts = torch.as_tensor(_blob(rng, 200_000), device="cuda")
    intr, w2c = _cams(200, 480, 640, seed=9)
    object_masks(pts[:1000], _motion(), intr, w2c, 480, 640, dilate=5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = object_masks(pts, _motion(), intr, w2c, 480, 640, dilate=5)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert dt < 1.0, dt
    assert (m.boxes[:, 2, 0] >= 0).all()


@gpu
def test_cli_end_to_end_twice_byte_identical(tmp_path):
    from gaussiangrasper_amd.edit_masks import main
    rng = np.random.default_rng(11)
    h, w = 30, 41
    c2w = R.ring(6, seed=12)
    c2w = np.concatenate([c2w, _aside(1, 13)])                                         # one frame without it
    meta = R.write_transforms(str(tmp_path / "scan" / "transforms.json"), c2w, h, w, 35.0, 36.0, 20.1, 14.7,
                              ext=".jpg", overrides={2: {"fl_x": 40.0, "cx": 19.0}})
    pts = _blob(rng, 700)
    np.savetxt(tmp_path / "obj.txt", np.hstack([pts, rng.random((700, 3))]))
    a, b = ["0.01", "0.0", "0.02", "0.1", "0.0", "0.2"], ["0.05", "-0.02", "0.0", "0.0", "0.3", "0.0"]
    outs = []
    for run in ("a", "b"):
        out = tmp_path / run
        assert main(["--transforms", str(tmp_path / "scan" / "transforms.json"), "--object-points",
                     str(tmp_path / "obj.txt"), "--pose-from", *a, "--pose-to", *b, "--out", str(out), "--dilate", "3",
                     "--all"]) == 0
        outs.append(out)
    files = sorted(os.path.relpath(os.path.join(d, f), outs[0]) for d, _, fs in os.walk(outs[0]) for f in fs)
    assert len(files) == 1 + 3 * 7 and "union/frame_0000.npy" in files
    for f in files:
        assert (outs[0] / f).read_bytes() == (outs[1] / f).read_bytes(), f
    from gaussiangrasper_amd.edit_masks import motion
    intr = np.array([[35.0, 36.0, 20.1, 14.7]] * 7)
    intr[2, 0], intr[2, 2] = 40.0, 19.0
    ref = R.object_masks(pts, motion([float(x) for x in a], [float(x) for x in b]), intr,
                         np.array([np.linalg.inv(T)[:3] for T in c2w]), h, w, 3)
    prompts = json.loads((outs[0] / "prompts.json").read_text())["frames"]
    for i in range(7):
        for m, name in enumerate(("before", "after", "union")):
            x = np.load(outs[0] / name / f"frame_{i:04d}.npy")
            assert x.dtype == np.float64 and x.shape == (h, w) and set(np.unique(x)) <= {0.0, 1.0}
            assert np.array_equal(x, ref[name][i].astype(np.float64)), (i, name)
            assert prompts[i]["boxes"][name] == ref["boxes"][i, m].tolist()
        assert prompts[i]["mask"] == f"frame_{i:04d}.npy"
    assert prompts[6]["boxes"]["union"] == [-1] * 4 and prompts[6]["centres"]["union"] == [None, None]
    # union only without --all; every frame empty -> non-zero
    out = tmp_path / "c"
    assert main(["--transforms", str(tmp_path / "scan" / "transforms.json"), "--object-points", str(tmp_path / "obj.txt"),
                 "--pose-from", *a, "--pose-to", *b, "--out", str(out)]) == 0
    assert sorted(os.listdir(out)) == ["prompts.json", "union"]
    meta["frames"] = meta["frames"][6:]
    (tmp_path / "away.json").write_text(json.dumps(meta))
    assert main(["--transforms", str(tmp_path / "away.json"), "--object-points", str(tmp_path / "obj.txt"),
                 "--pose-from", *a, "--pose-to", *b, "--out", str(tmp_path / "d")]) == 1
    assert main(["--transforms", str(tmp_path / "scan" / "transforms.json"), "--object-points",
                 str(tmp_path / "obj.txt"), "--pose-from", *a, "--pose-to", *b, "--out", str(tmp_path / "e"),
                 "--max-rows", "2"]) == 2
