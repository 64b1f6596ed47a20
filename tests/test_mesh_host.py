"""Mesh export without a GPU: the numpy restatement (tests/tsdf_ref.py) on an analytic sphere, the batch-split
invariance of the fusion rule, the PLY round trip, the frame helpers against direct matrix arithmetic, and the C
entries' host-side checks."""
import ctypes

import numpy as np
import pytest

import tsdf_ref as R

# Achieved on this scene: 0.73 voxels (|distance to the sphere| of the farthest vertex).
SPHERE_BOUND_VOXELS = 1.0


def sphere_scene(n=48, views=24, H=96, W=128, radius=0.5):
    vs = np.float32(1.6 / n)
    grid = np.array([-0.8, -0.8, -0.8, vs, vs, vs], np.float32)
    K = np.array([100.0, 100.0, 64.0, 48.0])
    E = R.sphere_cameras(views, 2.0)
    depth = np.stack([R.raycast_spheres(e, K, H, W, [((0.0, 0.0, 0.0), radius)]) for e in E])
    return (n, n, n), grid, np.float32(5 * vs), depth, np.tile(K, (views, 1)), E


def test_table_is_the_kuhn_decomposition():
    corner, ntri, edge = R.TABLE
    for t in range(6):
        assert corner[t, 0] == 0 and corner[t, 3] == 7
        for cs in range(16):
            ins = bin(cs).count("1")
            assert ntri[t, cs] == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[ins]
            for s in range(ntri[t, cs]):
                for code in edge[t, cs, s]:
                    lo = code >> 3
                    hi = lo + int(R.DIRS[code & 7] @ np.array([4, 2, 1]))
                    ids = list(corner[t])
                    assert lo in ids and hi in ids, "an edge of the tetrahedron"
                    assert ((cs >> ids.index(lo)) & 1) != ((cs >> ids.index(hi)) & 1), "a sign-changing edge"


def test_restatement_sphere_is_a_closed_oriented_manifold():
    dims, grid, trunc, depth, K, E = sphere_scene()
    vol = R.integrate(R.new_volume(dims), dims, grid, trunc, depth, K, E)
    v, nrm, col, f = R.extract(dims, grid, vol["tsdf"], vol["weight"])
    assert col is None and len(f) > 1000
    assert R.check_closed_manifold(f, len(v)) == 2
    fn = R.face_normals(v, f)
    cen = v[f].mean(axis=1)
    assert ((fn * cen).sum(axis=1) > 0).all(), "face normals point outwards (towards increasing TSDF)"
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    assert np.abs(r - 0.5).max() <= SPHERE_BOUND_VOXELS * grid[3]
    assert ((nrm * (v / r[:, None])).sum(axis=1) > 0.8).all(), "vertex normals follow the sphere's"


def test_restatement_batch_split_invariance():
    dims, grid, trunc, depth, K, E = sphere_scene(n=24, views=6, H=48, W=64)
    rgb = np.random.default_rng(0).random(depth.shape + (3,)).astype(np.float32)
    one = R.integrate(R.new_volume(dims, True), dims, grid, trunc, depth, K, E, rgb)
    split = R.new_volume(dims, True)
    for v in range(len(depth)):
        R.integrate(split, dims, grid, trunc, depth[v:v + 1], K[v:v + 1], E[v:v + 1], rgb[v:v + 1])
    for key in one:
        assert np.array_equal(one[key].view(np.uint32), split[key].view(np.uint32)), key


def test_restatement_skips_no_observation_and_carves_free_space():
    dims, grid, trunc = (8, 8, 8), np.array([-1, -1, 1, 0.25, 0.25, 0.25], np.float32), np.float32(0.5)
    E = np.array([[[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]]])
    K = np.array([[8.0, 8.0, 8.0, 8.0]])
    for value, weight, tsdf in ((0.0, 0.0, 1.0), (np.nan, 0.0, 1.0), (-1.0, 0.0, 1.0), (np.inf, 1.0, 1.0)):
        vol = R.integrate(R.new_volume(dims), dims, grid, trunc, np.full((1, 16, 16), value, np.float32), K, E)
        assert (vol["weight"] == weight).all() and (vol["tsdf"] == tsdf).all(), value


def test_ply_round_trip(tmp_path):
    from gaussiangrasper_amd.mesh import Mesh, read_ply_mesh, write_ply_mesh
    rng = np.random.default_rng(1)
    v = rng.standard_normal((50, 3)).astype(np.float32)
    n = rng.standard_normal((50, 3)).astype(np.float32)
    c = (rng.integers(0, 256, (50, 3)) / 255.0).astype(np.float32)
    f = rng.integers(0, 50, (70, 3)).astype(np.int32)
    p = str(tmp_path / "m.ply")
    write_ply_mesh(p, Mesh(v, f, n, c))
    m = read_ply_mesh(p)
    for a, b in ((m.vertices, v), (m.normals, n), (m.faces, f)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(np.rint(m.colors * 255), np.rint(c * 255))
    head = open(p, "rb").read(400).decode("latin-1")
    assert "format binary_little_endian 1.0" in head and "property list uchar int vertex_indices" in head
    write_ply_mesh(p, Mesh(v, f, n, None))
    assert (read_ply_mesh(p).colors == 0).all()


def test_opencv_w2c_matches_direct_arithmetic():
    from gaussiangrasper_amd.camera import ring_cameras
    from gaussiangrasper_amd.mesh import opencv_to_opengl_c2w, opencv_w2c
    rng = np.random.default_rng(2)
    for _ in range(5):
        q = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        c2w = np.eye(4)
        c2w[:3, :3], c2w[:3, 3] = q, rng.standard_normal(3)
        w2c = opencv_w2c(c2w)[0]
        flip = np.diag([1.0, -1.0, -1.0])
        assert np.allclose(w2c[:, :3], (q @ flip).T) and np.allclose(w2c[:, 3], -(q @ flip).T @ c2w[:3, 3])
        x = rng.standard_normal(3)
        xc = w2c[:, :3] @ x + w2c[:, 3]                  # OpenCV camera coordinates
        xgl = np.linalg.inv(c2w) @ np.append(x, 1.0)      # OpenGL camera coordinates
        assert np.allclose(xc, xgl[:3] * [1, -1, -1])
        assert np.allclose(opencv_to_opengl_c2w(np.linalg.inv(np.vstack([w2c, [0, 0, 0, 1]]))), c2w)
    # the renderer's own conversion (camera.view_from_c2w) gives the same world-to-camera
    view = ring_cameras(3, 48, 64)[1]
    c2w = np.linalg.inv(view.viewmat.double().numpy()) @ np.diag([1.0, -1.0, -1.0, 1.0])
    assert np.allclose(opencv_w2c(c2w)[0], view.viewmat.double().numpy()[:3], atol=1e-6)


def test_dataparser_frame_helpers_match_object_points_to_scene():
    from gaussiangrasper_amd.edit import object_points_to_scene, rotvec_to_matrix
    from gaussiangrasper_amd.mesh import c2w_to_scene, directions_from_scene, points_from_scene
    rng = np.random.default_rng(3)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = rotvec_to_matrix([0.3, -0.5, 0.2]), [0.1, -0.4, 0.25]
    s = 0.37
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = rotvec_to_matrix([1.0, 0.2, -0.7]), [0.5, 1.5, -0.2]
    cs = c2w_to_scene(c2w, M, s)
    pts_cam = rng.standard_normal((10, 3))
    raw = pts_cam @ c2w[:3, :3].T + c2w[:3, 3]
    scene = object_points_to_scene(raw, M, s)
    # the scene camera sees the scene points at the raw camera coordinates times the scale
    assert np.allclose((scene - cs[:3, 3]) @ cs[:3, :3], pts_cam * s)
    assert np.allclose(points_from_scene(scene, M, s), raw)
    d = rng.standard_normal((10, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    assert np.allclose(directions_from_scene(d @ M[:3, :3].T, M), d)


def test_workspace_queries_and_argument_validation_without_a_gpu():
    """(on a thread of its own: the library's error message is per thread, and the other tests' stays empty)"""
    import threading
    failure = []

    def run():
        try:
            _validation()
        except BaseException as exc:  # noqa: BLE001 - re-raised on the test's thread
            failure.append(exc)
    th = threading.Thread(target=run)
    th.start()
    th.join()
    if failure:
        raise failure[0]


def _validation():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    dims = lambda *d: (ctypes.c_int32 * 3)(*d)  # noqa: E731
    small, big = lib.gg_tsdf_mesh_workspace(dims(16, 16, 16)), lib.gg_tsdf_mesh_workspace(dims(256, 256, 256))
    assert 0 < small < big < 12 * 256 ** 3
    for bad in ((0, 4, 4), (4097, 2, 2), (512, 512, 513), (-1, 4, 4)):
        assert lib.gg_tsdf_mesh_workspace(dims(*bad)) == 0, bad
    assert lib.gg_tsdf_mesh_workspace(None) == 0
    n = ctypes.c_void_p(0)
    g = (ctypes.c_float * 6)(0, 0, 0, 0.1, 0.1, 0.1)
    st = lib.gg_tsdf_integrate(dims(512, 512, 513), g, 0.5, 1, 4, 4, n, n, n, n, n, n, n, n, n)
    assert st == -1 and b"GG_TSDF_MAX_POINTS" in lib.gg_last_error()
    st = lib.gg_tsdf_integrate(dims(4, 4, 4), (ctypes.c_float * 6)(0, 0, 0, 0.1, 0.0, 0.1), 0.5, 1, 4, 4,
                               n, n, n, n, n, n, n, n, n)
    assert st == -1 and b"voxel sizes" in lib.gg_last_error()
    st = lib.gg_tsdf_integrate(dims(4, 4, 4), g, float("nan"), 1, 4, 4, n, n, n, n, n, n, n, n, n)
    assert st == -1 and b"trunc" in lib.gg_last_error()
    st = lib.gg_tsdf_integrate(dims(4, 4, 4), g, 0.5, 1, 4, 4, n, n, n, n, n, n, n, n, n)
    assert st == -1 and b"null pointer" in lib.gg_last_error()
    c = ctypes.c_void_p(256)
    st = lib.gg_tsdf_mesh_count(dims(4, 4, 4), c, c, c, c, 0, n)
    assert st == -3 and b"workspace too small" in lib.gg_last_error()
    st = lib.gg_tsdf_mesh_emit(dims(4, 4, 0), g, c, n, 0, 0, n, n, n, n, c, 1 << 20, n)
    assert st == -1 and b"GG_TSDF_MAX_DIM" in lib.gg_last_error()


def test_volume_rejects_out_of_range_sizes_before_any_device_work():
    from gaussiangrasper_amd.mesh import TSDFVolume
    with pytest.raises(ValueError, match="2\\^27"):
        TSDFVolume((-1, -1, -1), (1, 1, 1), (600, 600, 600), device="cpu")
    with pytest.raises(ValueError, match="bbox"):
        TSDFVolume((0, 0, 0), (1, 0, 1), 8, device="cpu")
