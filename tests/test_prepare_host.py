"""CPU checks of scene preparation (gaussiangrasper_amd.prepare): the host restatements (tests/prepare_ref.py) against
the reference's literal formulas and sklearn, the subsample law, the COLMAP text writers read back by restated
colmap_utils readers, byte identity of points3D.txt with np.savetxt, the scan-directory validation of the CLI and
the plugin's device-kNN switch.  No GPU."""
import json
import os

import numpy as np
import pytest

import prepare_ref as R


def _frames(rng, f=3, h=20, w=28):
    depth = 0.5 + 0.05 * rng.normal(size=(f, h, w))
    depth[rng.random((f, h, w)) < 0.05] = 0.0
    depth[0, 2, 3], depth[1, 4, 5], depth[2, 6, 7] = np.nan, np.inf, -np.inf
    mask = (rng.random((f, h, w)) > 0.1).astype(np.uint8)
    rgb = rng.integers(0, 256, (f, h, w, 3), dtype=np.uint8)
    intr = np.array([[0.9 * w, 0.85 * w, w / 2 - 0.3, h / 2 + 0.2]] * f)
    T = np.array([np.eye(4)] * f)
    for i in range(f):
        T[i, :3, :3] = R.rodrigues(rng.normal(size=3) * 0.1) @ np.diag([1.0, -1.0, -1.0])
        T[i, :3, 3] = [0.01 * i, -0.02, 0.3]
    return depth, mask, rgb, intr, T


def test_backproject_restatement_matches_the_reference_formulas():
    rng = np.random.default_rng(1)
    depth, mask, rgb, intr, T = _frames(rng)
    p, c = R.backproject(depth, mask, rgb, intr, T)
    assert 0 < p.shape[0] < depth.size
    lp, lc = [], []
    for f in range(depth.shape[0]):
        with np.errstate(invalid="ignore"):
            a, b = R.backproject_literal(depth[f], mask[f], rgb[f], *intr[f], T[f])
        lp.append(a)
        lc.append(b)
    lp, lc = np.concatenate(lp), np.concatenate(lc)
    assert p.shape == lp.shape and np.array_equal(c, lc)
    assert np.abs(p - lp).max() <= 1e-12


def test_normals_restatement_matches_the_reference_formulas():
    rng = np.random.default_rng(2)
    for h, w in ((480, 640), (7, 5), (2, 2), (3, 11)):
        d = 0.4 + 0.1 * rng.random((1, h, w))
        d[0, 0, 0] = 0.005          # clamped
        if h > 2:
            d[0, 1, 1] = np.nan
            d[0, -1, -1] = np.inf
        T = R.random_pose(rng)[None]
        intr = np.array([[385.86, 385.38, w / 2, h / 2]])
        a = R.normals(d, intr, T)[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            b = R.normals_literal(d[0], 385.86, 385.38, T[0])
        assert np.isfinite(a).all() and np.isfinite(b).all()
        assert np.abs(a - b).max() <= 1e-12


def test_knn_restatement_is_bit_equal_to_sklearn():
    neighbors = pytest.importorskip("sklearn.neighbors")
    g = np.arange(28, dtype=np.float32) * 0.25
    x = np.stack(np.meshgrid(g, g, g[:26]), -1).reshape(-1, 3)[:20000]
    x = np.concatenate([x, x[::400][:50]])            # 50 duplicated rows
    ref = neighbors.NearestNeighbors(n_neighbors=4).fit(x).kneighbors(x)[0][:, 1:].astype(np.float32)
    got, _ = R.knn(x, 3)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    rng = np.random.default_rng(3)
    y = rng.normal(size=(3000, 3)).astype(np.float32)
    ref = neighbors.NearestNeighbors(n_neighbors=4).fit(y).kneighbors(y)[0][:, 1:].astype(np.float32)
    assert np.array_equal(R.knn(y, 3)[0].view(np.uint32), ref.view(np.uint32))


def test_subsample_law():
    from gaussiangrasper_amd.prepare import subsample_indices, splitmix64_keys
    for num, keep in ((0, 8), (7, 8), (8, 8), (12345, 8), (1000, 1), (1000, 3)):
        i = subsample_indices(num, keep, seed=5)
        assert i.dtype == np.int64 and i.shape == (num // keep,)
        assert np.all(np.diff(i) > 0) and (i.size == 0 or (i[0] >= 0 and i[-1] < num))
    assert np.array_equal(subsample_indices(50000, 8, 7), subsample_indices(50000, 8, 7))
    assert not np.array_equal(subsample_indices(50000, 8, 7), subsample_indices(50000, 8, 8))
    assert len(np.unique(splitmix64_keys(3, 100000))) == 100000
    # roughly uniform: how often each of 20 strata is hit, over 40 seeds (loose chi-square, 19 dof)
    num, keep, bins = 4000, 8, 20
    hits = np.zeros(bins)
    for s in range(40):
        hits += np.bincount(subsample_indices(num, keep, s) * bins // num, minlength=bins)
    e = hits.sum() / bins
    assert ((hits - e) ** 2 / e).sum() < 60.0


def test_colmap_writers_round_trip(tmp_path):
    from gaussiangrasper_amd.prepare import write_cameras_txt, write_images_txt, write_points3d_txt
    rng = np.random.default_rng(4)
    cam = {"fl_x": 385.86016845703125, "fl_y": 385.3817443847656, "cx": 325.68145751953125, "cy": 243.561767578125,
           "w": 640, "h": 480, "k1": -0.055006977170705795, "k2": 0.06818309426307678, "p1": -0.0007415282307192683,
           "p2": 0.0006959497695788741}
    write_cameras_txt(str(tmp_path / "cameras.txt"), cam)
    cams = R.read_cameras_text(str(tmp_path / "cameras.txt"))
    model, w, h, params = cams[1]
    assert (model, w, h) == ("OPENCV", 640, 480)
    assert params.tolist() == [cam[k] for k in ("fl_x", "fl_y", "cx", "cy", "k1", "k2", "p1", "p2")]
    poses = [R.random_pose(rng) for _ in range(6)]
    poses[1][:3, :3] = np.diag([1.0, -1.0, -1.0])         # half turns: Shepperd's other branches
    poses[2][:3, :3] = np.diag([-1.0, 1.0, -1.0])
    poses[3][:3, :3] = np.diag([-1.0, -1.0, 1.0])
    names = [f"frame_{i:04d}.png" for i in range(6)]
    write_images_txt(str(tmp_path / "images.txt"), poses, names)
    ims = R.read_images_text(str(tmp_path / "images.txt"))
    assert sorted(ims) == list(range(1, 7))
    for i, T in enumerate(poses):
        q, t, cid, name, xys = ims[i + 1]
        assert cid == 1 and name == names[i] and xys.shape == (1, 2)
        assert np.abs(R.qvec2rotmat(q) - T[:3, :3]).max() <= 1e-12 and np.abs(t - T[:3, 3]).max() <= 1e-12
    pts = rng.normal(size=(500, 3)) * 0.3
    pts[0] = [-0.0000004, 1e-7, -0.2999995]
    cols = rng.integers(0, 256, (500, 3), dtype=np.uint8)
    write_points3d_txt(str(tmp_path / "points3D.txt"), pts, cols)
    # save_points3D :360-367 as written
    merged = np.concatenate((pts, cols.astype(np.uint8)), axis=1)
    ids = np.arange(1, merged.shape[0] + 1).reshape(-1, 1)
    np.savetxt(str(tmp_path / "ref.txt"), np.concatenate((ids, merged), axis=1), fmt="%d " + "%.6f " * 3 + "%d %d %d")
    assert (tmp_path / "points3D.txt").read_bytes() == (tmp_path / "ref.txt").read_bytes()
    back = R.read_points3D_text(str(tmp_path / "points3D.txt"))
    assert len(back) == 500 and np.array_equal(back[500][1], cols[499].astype(int))


def _cli(argv):
    from gaussiangrasper_amd.prepare import main
    return main(argv)


def test_cli_names_a_missing_file(tmp_path, capsys):
    R.write_scan(str(tmp_path), n_frames=2)
    os.remove(tmp_path / "depths" / "frame_0001.npy")
    assert _cli(["--scan", str(tmp_path)]) == 2
    assert os.path.join("depths", "frame_0001.npy") in capsys.readouterr().err


def test_cli_rejects_mismatched_sizes(tmp_path, capsys):
    R.write_scan(str(tmp_path), n_frames=2, h=24, w=32)
    np.save(tmp_path / "depths" / "frame_0000.npy", np.ones((24, 31)))
    assert _cli(["--scan", str(tmp_path)]) == 2
    err = capsys.readouterr().err
    assert "frame_0000.npy" in err and "24 x 32" in err


def test_cli_pairs_frames_by_stem_not_by_listing_order(tmp_path, capsys):
    meta = R.write_scan(str(tmp_path), n_frames=2)
    meta["frames"][0]["file_path"] = "images/other.png"       # no such stem
    (tmp_path / "transforms.json").write_text(json.dumps(meta))
    assert _cli(["--scan", str(tmp_path)]) == 2
    assert os.path.join("images", "other.png") in capsys.readouterr().err


def test_cli_refuses_to_overwrite(tmp_path, capsys):
    R.write_scan(str(tmp_path), n_frames=2)
    out = tmp_path / "colmap" / "sparse" / "0"
    out.mkdir(parents=True)
    (out / "points3D.txt").write_text("keep me\n")
    assert _cli(["--scan", str(tmp_path)]) == 2
    assert "--force" in capsys.readouterr().err
    assert (out / "points3D.txt").read_text() == "keep me\n"


def test_knn_distances_rejects_what_sklearn_rejects():
    from gaussiangrasper_amd.prepare import knn_distances
    with pytest.raises(ValueError):
        knn_distances(np.zeros((3, 3), np.float32), 3)
    x = np.random.default_rng(0).normal(size=(10, 3)).astype(np.float32)
    x[4, 1] = np.nan
    with pytest.raises(ValueError):
        knn_distances(x, 3)
    x[4, 1] = np.inf
    with pytest.raises(ValueError):
        knn_distances(x, 3)


def test_device_knn_is_opt_in(monkeypatch):
    from gaussiangrasper_amd.plugin import make_fused_model_class
    from gaussiangrasper_amd.stub import StubGaussianSplattingModel
    monkeypatch.delenv("GG_DEVICE_KNN", raising=False)
    assert not hasattr(make_fused_model_class(StubGaussianSplattingModel), "k_nearest_sklearn")
    assert hasattr(make_fused_model_class(StubGaussianSplattingModel, device_knn=True), "k_nearest_sklearn")
    monkeypatch.setenv("GG_DEVICE_KNN", "1")
    assert hasattr(make_fused_model_class(StubGaussianSplattingModel), "k_nearest_sklearn")


def test_knn_grid_fits_the_bulk():
    import torch
    from gaussiangrasper_amd.prepare import knn_grid
    rng = np.random.default_rng(5)
    x = rng.random((100000, 3)).astype(np.float32)
    x[:10] = 1e4                                            # far outliers do not stretch the grid
    grid, dims = knn_grid(torch.from_numpy(x))
    assert grid[3] < 0.1 and 1 <= dims.min() and np.prod(dims.astype(np.int64)) <= 2 * 100000
    grid, dims = knn_grid(torch.zeros((1000, 3)))
    assert dims.tolist() == [1, 1, 1] and grid[3] > 0
    p = rng.random((10000, 3)).astype(np.float32)
    p[:, 2] = 0.5                                           # planar
    grid, dims = knn_grid(torch.from_numpy(p))
    assert dims[2] == 1 and dims[0] > 50


def test_cameras_follow_per_frame_intrinsics(tmp_path):
    from gaussiangrasper_amd.prepare import camera_ids, write_cameras_txt, write_images_txt
    meta = {"fl_x": 300.0, "fl_y": 301.0, "cx": 160.0, "cy": 120.0, "w": 320, "h": 240, "k1": 0.01}
    frames = [{}, {"fl_x": 310.0}, {}, {"fl_x": 310.0, "k2": 0.5}]
    cams, ids = camera_ids(meta, frames)
    assert ids == [1, 2, 1, 3] and len(cams) == 3
    assert cams[0] == (300.0, 301.0, 160.0, 120.0, 0.01, 0.0, 0.0, 0.0) and cams[2][5] == 0.5
    write_cameras_txt(str(tmp_path / "cameras.txt"), meta, cams)
    back = R.read_cameras_text(str(tmp_path / "cameras.txt"))
    assert sorted(back) == [1, 2, 3] and all(back[i][:3] == ("OPENCV", 320, 240) for i in back)
    assert back[2][3].tolist() == list(cams[1])
    write_images_txt(str(tmp_path / "images.txt"), [np.eye(4)] * 4, [f"{i}.png" for i in range(4)], ids)
    assert [v[2] for _, v in sorted(R.read_images_text(str(tmp_path / "images.txt")).items())] == ids


def test_single_channel_3d_npy_mask(tmp_path):
    from gaussiangrasper_amd.prepare import _read_mask
    m = np.zeros((5, 7, 1), np.uint8)
    m[2, 3, 0] = 9
    np.save(tmp_path / "m.npy", m)
    got = _read_mask(str(tmp_path / "m.npy"))
    assert got.shape == (5, 7) and got.sum() == 1 and got[2, 3]
    rgb = np.zeros((5, 7, 3), np.uint8)
    rgb[1, 1] = [0, 200, 0]
    np.save(tmp_path / "c.npy", rgb)
    got = _read_mask(str(tmp_path / "c.npy"))
    assert got.shape == (5, 7) and got.sum() == 1 and got[1, 1]
