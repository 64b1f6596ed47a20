"""No-GPU checks of the scene update (gaussiangrasper_amd.edit, gg_hull_edit): the host-side pieces — outlier filter,
hull half-spaces, the gripper transform — against direct numpy statements, the C entry's argument validation, and the
command-line tool's refusal of a checkpoint that is not a splatting model."""
import ctypes
import json

import numpy as np
import pytest
import torch


def test_outlier_filter_is_the_stated_rule():
    from gaussiangrasper_amd.edit import filter_object_points
    rng = np.random.default_rng(0)
    p = rng.normal(size=(2000, 3))
    p[:5] += 40.0                       # far above Q3 + IQR: dropped
    for f in (1.0, 0.25, 3.0):
        got = filter_object_points(p, f)
        q1, q3 = np.min(p, axis=0), np.percentile(p, 80, axis=0)
        iqr = q3 - q1
        keep = np.all((p >= q1 - f * iqr) & (p <= q3 + f * iqr), axis=1)
        assert np.array_equal(got, p[keep])
    got = filter_object_points(p, 1.0)
    assert len(got) < len(p) and not np.isin(p[:5, 0], got[:, 0]).any()
    # far below everything: Q1 is the minimum, so the low side never filters
    low = rng.normal(size=(2000, 3))
    low[:5] -= 40.0
    for f in (0.0, 1.0):
        got = filter_object_points(low, f)
        assert np.isin(low[:5, 0], got[:, 0]).all()


def test_rotvec_to_matrix_is_rodrigues():
    from gaussiangrasper_amd.edit import rotvec_to_matrix
    rng = np.random.default_rng(1)
    for v in list(rng.normal(size=(20, 3))) + [np.array([np.pi, 0.0, 0.0]), np.zeros(3)]:
        th = np.linalg.norm(v)
        if th == 0.0:
            ref = np.eye(3)
        else:
            x, y, z = v / th
            c, s, C = np.cos(th), np.sin(th), 1.0 - np.cos(th)
            ref = np.array([[c + x * x * C, x * y * C - z * s, x * z * C + y * s],
                            [y * x * C + z * s, c + y * y * C, y * z * C - x * s],
                            [z * x * C - y * s, z * y * C + x * s, c + z * z * C]])
        got = rotvec_to_matrix(v)
        assert np.abs(got - ref).max() < 1e-14
        assert np.abs(got @ got.T - np.eye(3)).max() < 1e-14


def test_compose_transform_is_the_matrix_product():
    from gaussiangrasper_amd.edit import compose_transform, object_points_to_scene, rotvec_to_matrix
    rng = np.random.default_rng(2)
    M = np.eye(4)
    M[:3, :3] = rotvec_to_matrix(rng.normal(size=3))
    M[:3, 3] = rng.normal(size=3)
    scale = 0.37
    a, b = rng.normal(size=6), rng.normal(size=6)

    def hom(p):
        T = np.eye(4)
        T[:3, :3] = rotvec_to_matrix(p[3:])
        T[:3, 3] = p[:3]
        return T
    T = M @ hom(b) @ np.linalg.inv(hom(a)) @ np.linalg.inv(M)
    T[:3, 3] *= scale
    got = compose_transform(M, scale, a, b)
    assert got.dtype == np.float32 and got.shape == (3, 4)
    assert np.array_equal(got, T[:3, :].astype(np.float32))
    pts = rng.normal(size=(50, 3))
    ref = (pts @ M[:3, :3].T + M[:3, 3]) * scale
    assert np.abs(object_points_to_scene(pts, M, scale) - ref).max() < 1e-13


def test_hull_planes_agree_with_delaunay_away_from_the_boundary():
    pytest.importorskip("scipy")
    from scipy.spatial import Delaunay
    from gaussiangrasper_amd.edit import hull_planes
    rng = np.random.default_rng(3)
    for m in (8, 60, 2000):
        obj = rng.normal(size=(m, 3)) * np.array([1.0, 0.5, 0.3])
        planes = hull_planes(obj)
        assert planes.dtype == np.float64 and planes.shape[1] == 4 and planes.shape[0] >= 4
        assert np.allclose(np.linalg.norm(planes[:, :3], axis=1), 1.0)
        x = rng.normal(size=(20000, 3)) * 1.2
        v = x @ planes[:, :3].T + planes[:, 3]
        clear = np.abs(v).min(axis=1) >= 1e-9
        inside = (v <= 0.0).all(axis=1)
        ref = Delaunay(obj).find_simplex(x) >= 0
        assert np.array_equal(inside[clear], ref[clear])
        assert inside.any() and (~inside).any()


def test_hull_planes_without_scipy_names_the_way_out(monkeypatch):
    import builtins
    from gaussiangrasper_amd import edit
    real = builtins.__import__

    def no_scipy(name, *a, **k):
        if name.startswith("scipy"):
            raise ImportError("No module named 'scipy'")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_scipy)
    with pytest.raises(ImportError, match="planes="):
        edit.hull_planes(np.eye(4, 3))


def test_hull_edit_argument_validation_without_a_gpu():
    """invalid arguments are rejected on the host before anything is launched (checked on a thread of its own:
    gg_last_error is per thread, so the message does not outlive the test)"""
    import threading
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    n = ctypes.c_void_p(0)
    fake = ctypes.c_void_p(1 << 20)     # never dereferenced: every call below fails validation first
    rt = (ctypes.c_float * 12)()
    cases = [
        ((-1, fake, fake, 6, fake, 0.0, n, fake, fake, n), b"num_points"),
        ((10, fake, fake, 3, fake, 0.0, n, fake, fake, n), b"num_planes"),
        ((10, fake, fake, 6, fake, 0.0, n, fake, n, n), b"count_out"),
        ((10, n, fake, 6, fake, 0.0, n, fake, fake, n), b"null pointer"),
        ((10, fake, fake, 6, n, 0.0, n, fake, fake, n), b"null pointer"),
        ((10, fake, fake, 6, fake, 0.0, n, n, fake, n), b"null pointer"),
        ((10, fake, n, 6, fake, 0.0, ctypes.cast(rt, ctypes.c_void_p), fake, fake, n), b"quats"),
    ]
    got = []

    def run():
        for args, _ in cases:
            got.append((lib.gg_hull_edit(*args), lib.gg_last_error()))
    t = threading.Thread(target=run)
    t.start()
    t.join()
    assert len(got) == len(cases)
    for (st, msg), (_, want) in zip(got, cases):
        assert st == -1 and msg.startswith(b"gg_hull_edit") and want in msg, msg


def test_select_and_move_refuses_host_tensors():
    from gaussiangrasper_amd.edit import select_and_move
    planes = np.array([[1.0, 0, 0, -1], [-1.0, 0, 0, -1], [0, 1.0, 0, -1], [0, -1.0, 0, -1]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        select_and_move(torch.zeros(4, 3), torch.zeros(4, 4), planes)


def test_cli_refuses_a_checkpoint_without_means(tmp_path):
    from gaussiangrasper_amd import edit
    ck = tmp_path / "step-000001000.ckpt"
    torch.save({"step": 1000, "pipeline": {"_model.quats": torch.zeros(3, 4)}, "optimizers": {}}, ck)
    np.save(tmp_path / "obj.npy", np.random.default_rng(0).normal(size=(50, 3)))
    (tmp_path / "transform.json").write_text(json.dumps({"transform_matrix": np.eye(4).tolist(), "scale": 1.0}))
    out = tmp_path / "out.ckpt"
    with pytest.raises(SystemExit, match="_model.means"):
        edit.main(["--ckpt", str(ck), "--object-points", str(tmp_path / "obj.npy"),
                   "--transform-json", str(tmp_path / "transform.json"), "--pose-from", *["0"] * 6,
                   "--pose-to", *["0"] * 6, "--out", str(out)])
    assert not out.exists()
