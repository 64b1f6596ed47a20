"""GPU checks of known free space (gg_depth_min_pyramid, gg_field_observe, gg_field_distance_known and the Python layer
on top) against the restatement (tests/observe_ref.py).  Everything is held to equality, no case exempt: fp64 add,
multiply, divide and floor are correctly rounded on both sides.  The C calls' arrays are carved from the sentinel arena
(tests/arena.py) and compared whole."""
import ctypes
import math

import numpy as np
import pytest
import torch

import field_ref
import observe_ref as ref
from arena import Arena

gpu = pytest.mark.gpu
DEV = "cuda:0"
D = ctypes.c_double
WIDE_LO, WIDE_DIMS = (-0.8, -0.8, -0.1), (52, 50, 21)      # the frames cover a part of it: the cull's edge is inside
WIDE_GRID = np.array([*WIDE_LO, ref.CELL])


def _lib():
    from gaussiangrasper_amd import _lib as L
    return L.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def c_pyramid(depth, seed=0):
    V, H, W = depth.shape
    S = int(_lib().gg_depth_min_pyramid_size(H, W))
    assert S == ref.level_offsets(H, W)[1]
    a = Arena(DEV, seed)
    a.carve("depth", np.asarray(depth, np.float32), 4, "in")
    a.carve("pyr", np.zeros((V, S), np.float32), 4, "out")
    st = _lib().gg_depth_min_pyramid(V, H, W, a.ptr("depth"), a.ptr("pyr"), _stream())
    assert st == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    if V == 0:
        return a.untouched()
    return a.check()["pyr"]


def c_observe(dims, grid, pyr, H, W, K, E, radius=ref.RADIUS, margin=ref.MARGIN, near=ref.NEAR, seen=None, looked=None,
              no_looked=False, seed=0, calls=((0, None),)):
    """gg_field_observe on one arena, once per (first view, end view) of `calls` -> (seen, looked or None)"""
    V, S = len(K), ref.level_offsets(H, W)[1]
    a = Arena(DEV, seed)
    a.carve("pyr", np.asarray(pyr, np.float32).reshape(V, S), 4, "in")
    a.carve("K", np.asarray(K, np.float64).reshape(V, 4), 8, "in")
    a.carve("E", np.asarray(E, np.float64).reshape(V, 3, 4), 8, "in")
    z = np.zeros(dims, np.uint16)
    a.carve("seen", z if seen is None else np.asarray(seen, np.uint16), 2, "inout")
    if not no_looked:
        a.carve("looked", z if looked is None else np.asarray(looked, np.uint16), 2, "inout")
    for v0, v1 in calls:
        v1 = V if v1 is None else v1
        st = _lib().gg_field_observe((ctypes.c_int32 * 3)(*dims), (D * 4)(*grid), v1 - v0, H, W,
                                     ctypes.c_void_p(a.address("pyr") + 4 * S * v0),
                                     ctypes.c_void_p(a.address("K") + 32 * v0), ctypes.c_void_p(a.address("E") + 96 * v0),
                                     D(radius), D(margin), D(near), a.ptr("seen"),
                                     None if no_looked else a.ptr("looked"), _stream())
        assert st == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    if V == 0:
        a.untouched()
        return a.before("seen"), None if no_looked else a.before("looked")
    out = a.check()
    return out["seen"], out.get("looked")


def c_distance(mass, threshold, seen=None, min_views=1, seed=0):
    dims = mass.shape
    a = Arena(DEV, seed)
    d = (ctypes.c_int32 * 3)(*dims)
    need = _lib().gg_field_distance_workspace(d)
    a.carve("mass", np.asarray(mass, np.int64), 8, "in")
    if seen is not None:
        a.carve("seen", np.asarray(seen, np.uint16), 2, "in")
    a.carve("dist2", np.zeros(dims, np.int32), 4, "out")
    a.carve("ws", int(need), 256, "ws")
    if seen is None:
        st = _lib().gg_field_distance(d, a.ptr("mass"), int(threshold), a.ptr("dist2"), a.ptr("ws"),
                                      ctypes.c_size_t(need), _stream())
    else:
        st = _lib().gg_field_distance_known(d, a.ptr("mass"), int(threshold), a.ptr("seen"), int(min_views),
                                            a.ptr("dist2"), a.ptr("ws"), ctypes.c_size_t(need), _stream())
    assert st == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    return a.check()["dist2"]


@pytest.fixture(scope="module")
def scene():
    fx = ref.fixture()
    fx["pyr"] = ref.pyramid(fx["depth"])            # computed once, shared, left unchanged
    fx["pyr"].setflags(write=False)
    return fx


def check_observe(scene, dims, grid, views=slice(None), **kw):
    K, E, pyr = scene["K"][views], scene["E"][views], scene["pyr"][views]
    ref_kw = {k: v for k, v in kw.items() if k in ("radius", "margin", "near", "seen", "looked")}
    want_seen, want_looked = ref.observe(dims, grid, pyr, ref.FH, ref.FW, K, E, **{
        "radius": ref.RADIUS, "margin": ref.MARGIN, "near": ref.NEAR, **ref_kw})
    seen, looked = c_observe(dims, grid, pyr, ref.FH, ref.FW, K, E, **kw)
    assert np.array_equal(seen, want_seen)
    if looked is not None:
        assert np.array_equal(looked, want_looked)
    return want_seen, want_looked


# ------------------------------------------------------------------------------------------------
# pyramid
# ------------------------------------------------------------------------------------------------
@gpu
def test_pyramid_of_the_fixture(scene):
    assert np.array_equal(c_pyramid(scene["depth"]).view(np.uint32), scene["pyr"].view(np.uint32))


@gpu
@pytest.mark.parametrize("V,H,W", [(1, 1, 1), (3, 1, 9), (2, 7, 1), (2, 2, 2), (2, 33, 17), (1, 64, 64), (3, 129, 255),
                                   (0, 5, 5)])
def test_pyramid_sizes_and_special_values(V, H, W):
    """odd sizes, one row, one column, powers of two, more than one workgroup; +inf, 0, negative and NaN inputs"""
    rng = np.random.default_rng(V * 1000 + H * 10 + W)
    d = rng.uniform(0.5, 4.0, size=(V, H, W)).astype(np.float32)
    special = np.array([np.inf, 0.0, -1.0, np.nan, -np.inf, -0.0], np.float32)
    where = rng.random((V, H, W)) < 0.3
    d[where] = special[rng.integers(0, len(special), int(where.sum()))]
    got = c_pyramid(d)
    if V:
        assert np.array_equal(got.view(np.uint32), ref.pyramid(d).view(np.uint32))


# ------------------------------------------------------------------------------------------------
# observe
# ------------------------------------------------------------------------------------------------
@gpu
def test_fixture_whole(scene):
    seen, looked = check_observe(scene, ref.DIMS, ref.GRID)
    solid = ref.solid(ref.centres())
    assert (seen[~solid] > 0).mean() >= 0.85 and not seen[solid].any() and looked.max() == 5


@gpu
@pytest.mark.parametrize("dims", [(12, 8, 16), (1, 1, 1), (4, 8, 8), (5, 9, 9)])
def test_brick_multiples_and_one_cell(scene, dims):
    """exact multiples of the 4 x 8 x 8 brick, one brick, one cell over in every direction, one cell in all"""
    check_observe(scene, dims, ref.GRID)


@gpu
@pytest.mark.parametrize("views", [slice(0, 0), slice(2, 3), slice(0, 5)])
def test_view_counts(scene, views):
    pre = np.random.default_rng(1).integers(0, 9, ref.DIMS).astype(np.uint16)
    check_observe(scene, ref.DIMS, ref.GRID, views, seen=pre, looked=pre[::-1].copy())


@gpu
def test_calls_add_up(scene):
    one = c_observe(ref.DIMS, ref.GRID, scene["pyr"], ref.FH, ref.FW, scene["K"], scene["E"])
    two = c_observe(ref.DIMS, ref.GRID, scene["pyr"], ref.FH, ref.FW, scene["K"], scene["E"], calls=((0, 2), (2, 5)))
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])


@gpu
def test_a_view_behind_the_volume(scene):
    """the camera looks away from the volume: every brick skips it, nothing is counted"""
    behind = dict(scene)
    behind["E"] = np.stack([ref.look_at((0.9, 0.2, 0.8), (1.8, 0.4, 1.5)), scene["E"][1]])
    behind["K"], behind["pyr"] = scene["K"][:2], scene["pyr"][:2]
    seen, looked = check_observe(behind, ref.DIMS, ref.GRID)
    alone, alone_looked = ref.observe(ref.DIMS, ref.GRID, scene["pyr"][1:2], ref.FH, ref.FW, scene["K"][1:2],
                                      scene["E"][1:2], ref.RADIUS, ref.MARGIN, ref.NEAR)
    assert np.array_equal(seen, alone) and np.array_equal(looked, alone_looked)


@gpu
def test_views_that_cover_a_part_of_the_volume(scene):
    """the frames' frustums end inside the wider volume: bricks outside skip the view, bricks on the edge do not"""
    seen, looked = check_observe(scene, WIDE_DIMS, WIDE_GRID)
    assert (looked == 0).any() and (looked == 5).any() and (seen > 0).any()
    assert looked[0, 0, 20] == 0 and looked[-1, -1, -1] == 0         # whole bricks no view has in its image


@gpu
def test_a_view_so_close_that_footprints_need_the_coarsest_level(scene):
    """From inside the volume some cells' footprints span the image: they are read from the 2 x 2 level 5, the coarsest
    a 37 x 53 frame's footprint can need (tests/test_observe_host.py: the level below the top always qualifies); in
    a 1 x 1 frame the top level is level 0."""
    E = ref.look_at((-0.2, -0.3, 0.35), (-0.2, -0.25, 0.1))[None]
    levels = []
    ref.observe_views(ref.DIMS, ref.GRID, scene["pyr"][:1], ref.FH, ref.FW, scene["K"][:1], E, ref.RADIUS, ref.MARGIN,
                      ref.NEAR, levels)
    assert levels[0].max() == len(ref.level_shapes(ref.FH, ref.FW)) - 2 and set(np.unique(levels[0])) >= {-1, 2, 3, 4, 5}
    close = {"K": scene["K"][:1], "E": E, "pyr": scene["pyr"][:1]}
    _, looked = check_observe(close, ref.DIMS, ref.GRID)
    assert 0 < looked.sum() < looked.size
    # one pixel: a far camera whose only pixel holds every cell's footprint
    K1, E1 = np.array([[0.05, 0.05, 0.5, 0.5]]), ref.look_at((0.0, 0.0, 40.0), (-0.2, -0.25, 0.2), up=(0, 1, 0))[None]
    for d in (50.0, 39.0, 0.0):
        pyr1 = np.array([[d]], np.float32)
        want = ref.observe(ref.DIMS, ref.GRID, pyr1, 1, 1, K1, E1, ref.RADIUS, ref.MARGIN, ref.NEAR)
        got = c_observe(ref.DIMS, ref.GRID, pyr1, 1, 1, K1, E1)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert (want[1] == 1).all() and (want[0] == (1 if d == 50.0 else 0)).all()


@gpu
def test_counters_saturate(scene):
    pre = np.full(ref.DIMS, 65534, np.uint16)
    seen, looked = check_observe(scene, ref.DIMS, ref.GRID, seen=pre, looked=pre)
    assert set(np.unique(seen)) == {65534, 65535} and set(np.unique(looked)) == {65535}


@gpu
def test_looked_may_be_null(scene):
    check_observe(scene, ref.DIMS, ref.GRID, no_looked=True)


@gpu
def test_other_radius_margin_and_near(scene):
    check_observe(scene, ref.DIMS, ref.GRID, radius=0.01, margin=0.0, near=0.3)
    check_observe(scene, ref.DIMS, ref.GRID, radius=0.09, margin=0.05, near=0.7)


# ------------------------------------------------------------------------------------------------
# distance with unknown space blocked
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def counts(scene):
    return ref.observe(ref.DIMS, ref.GRID, scene["pyr"], ref.FH, ref.FW, scene["K"], scene["E"], ref.RADIUS,
                       ref.MARGIN, ref.NEAR)


def _mass():
    mass = np.zeros(ref.DIMS, np.int64)
    mass[3:5, 4, 10:13] = 40000
    mass[9, 2, 17] = 32767                                            # one vote short of the threshold
    return mass


@gpu
@pytest.mark.parametrize("min_views", [1, 3])
def test_distance_known_against_the_restatement(counts, min_views):
    got = c_distance(_mass(), 32768, counts[0], min_views)
    assert np.array_equal(got, ref.distance_known(_mass(), 32768, counts[0], min_views))
    assert (got == 0).sum() > 6


@gpu
def test_distance_known_with_everything_seen_is_distance():
    mass = _mass()
    full = np.full(ref.DIMS, 65535, np.uint16)
    plain = c_distance(mass, 32768)
    assert np.array_equal(c_distance(mass, 32768, full, 65535), plain)
    assert np.array_equal(plain, field_ref.distance(mass, 32768))
    assert (c_distance(mass, 32768, np.zeros(ref.DIMS, np.uint16), 1) == 0).all()


# ------------------------------------------------------------------------------------------------
# through DistanceField
# ------------------------------------------------------------------------------------------------
def _wide_field():
    from gaussiangrasper_amd import field as F
    hi = np.array(WIDE_LO) + (np.array(WIDE_DIMS) - 0.2) * ref.CELL
    f = F.DistanceField(WIDE_LO, hi, ref.CELL, device=DEV)
    assert tuple(f.dims) == WIDE_DIMS
    return F, f


@pytest.fixture(scope="module")
def wide(scene):
    """the field over the wide volume after two observe calls (OpenCV w2c, then OpenGL c2w), and what it must hold"""
    from gaussiangrasper_amd.mesh import opencv_to_opengl_c2w, opencv_w2c
    F, f = _wide_field()
    f.mass[20:23, 30, 5:9] = 40000
    K, E, depth = scene["K"], scene["E"], scene["depth"]
    bottom = np.broadcast_to(np.array([0.0, 0.0, 0.0, 1.0]), (3, 1, 4))
    c2w_gl = opencv_to_opengl_c2w(np.linalg.inv(np.concatenate([E[2:], bottom], 1)))
    f.observe(torch.from_numpy(depth[:2]), K[:2], w2c=E[:2], margin=ref.MARGIN, near=ref.NEAR, batch=1)
    assert f.seen.dtype == torch.uint16 and f.looked.shape == f.mass.shape
    f.observe(depth[2:], K[2:], c2w=c2w_gl, margin=ref.MARGIN, near=ref.NEAR, batch=2)
    args = (WIDE_DIMS, WIDE_GRID)
    cam = (F.cell_ball(f.h), ref.MARGIN, ref.NEAR)
    seen, looked = ref.observe(*args, scene["pyr"][:2], ref.FH, ref.FW, K[:2], E[:2], *cam)
    seen, looked = ref.observe(*args, scene["pyr"][2:], ref.FH, ref.FW, K[2:], opencv_w2c(c2w_gl), *cam, seen=seen,
                               looked=looked)
    return F, f, seen, looked


@gpu
def test_distance_field_observe_update_and_knowledge(wide, tmp_path):
    F, f, seen, looked = wide
    assert np.array_equal(f.seen.cpu().numpy(), seen) and np.array_equal(f.looked.cpu().numpy(), looked)
    mass = f.mass.cpu().numpy()
    f.update()
    assert np.array_equal(f.dist2.cpu().numpy(), field_ref.distance(mass, f.threshold))      # the old dist2, byte for byte
    f.update(unknown="blocked", min_views=2)
    blocked = ref.distance_known(mass, f.threshold, seen, 2)
    assert np.array_equal(f.dist2.cpu().numpy(), blocked)
    occ = mass >= f.threshold
    free = ~occ & (seen >= 2)
    occl = ~occ & ~free & (looked > 0)
    assert f.knowledge(2) == {"occupied": int(occ.sum()), "free": int(free.sum()), "occluded": int(occl.sum()),
                              "unseen": int((~occ & ~free & ~occl).sum())}
    assert all(type(v) is int and v > 0 for v in f.knowledge(2).values())
    f.save(str(tmp_path / "f.npz"))
    back = F.DistanceField.load(str(tmp_path / "f.npz"), device=DEV)
    assert torch.equal(back.seen.view(torch.int16), f.seen.view(torch.int16)) and back.knowledge(2) == f.knowledge(2)
    back.update(unknown="blocked", min_views=2)
    assert torch.equal(back.dist2, f.dist2)
    # the robot's envelope: a box taken as known opens exactly its cells
    corner = np.array(WIDE_LO)
    f.assume_free(corner, corner + 4 * ref.CELL)
    f.update(unknown="blocked", min_views=2)
    seen2 = seen.copy()
    seen2[:4, :4, :4] = 65535
    assert np.array_equal(f.dist2.cpu().numpy(), ref.distance_known(mass, f.threshold, seen2, 2))
    f.seen = torch.from_numpy(seen).to(DEV)


@gpu
def test_a_path_through_a_never_looked_at_corner_flips_to_blocked(wide):
    F, f, seen, looked = wide
    f.seen = torch.from_numpy(seen).to(DEV)
    assert looked[0, 0, 20] == 0                                      # the corner no view has in its image
    blocked = ref.distance_known(f.mass.cpu().numpy(), f.threshold, seen, 2)
    start = np.unravel_index(int(np.argmax(blocked)), blocked.shape)  # the cell deepest inside known free space
    centre = lambda c: WIDE_GRID[:3] + (np.asarray(c, np.float64) + 0.5) * ref.CELL
    W = 24
    t = centre(start)[None] + np.linspace(0.0, 1.0, W)[:, None] * (centre((0, 0, 20)) - centre(start))[None]
    poses = np.zeros((1, W, 12), np.float32)
    poses[0, :, [0, 4, 8]] = 1.0
    poses[0, :, 9:] = t
    spheres = np.zeros((1, 3), np.float32)
    f.update()
    res = F.path_clear(f, poses, spheres, 0.005)
    assert bool(res.clear[0]) and int(res.first_hit[0]) == W          # no Gaussian is near: "clear", seen or not
    f.update(unknown="blocked", min_views=2)
    res = F.path_clear(f, poses, spheres, 0.005)
    assert not bool(res.clear[0]) and 1 <= int(res.first_hit[0]) < W
    assert int(res.slack[0, 0]) >= 0 and int(res.slack[0, -1]) < 0
    with pytest.raises(ValueError, match="blocked"):
        _wide_field()[1].update(unknown="blocked")


@gpu
def test_python_calls_check_their_tensors(scene):
    from gaussiangrasper_amd import field as F
    pyr = F.depth_pyramid(torch.from_numpy(scene["depth"]).to(DEV))
    assert np.array_equal(pyr.cpu().numpy().view(np.uint32), scene["pyr"].view(np.uint32))
    seen = torch.zeros(ref.DIMS, dtype=torch.uint16, device=DEV)
    F.observe(seen, None, ref.GRID, ref.DIMS, pyr, scene["K"], scene["E"], ref.FH, ref.FW, ref.RADIUS, ref.MARGIN, ref.NEAR)
    want = ref.observe(ref.DIMS, ref.GRID, scene["pyr"], ref.FH, ref.FW, scene["K"], scene["E"], ref.RADIUS,
                       ref.MARGIN, ref.NEAR)[0]
    assert np.array_equal(seen.cpu().numpy(), want)
    ok = (seen, None, ref.GRID, ref.DIMS, pyr, scene["K"], scene["E"], ref.FH, ref.FW, ref.RADIUS)
    swap = lambda i, v: ok[:i] + (v,) + ok[i + 1:]
    for bad in (swap(0, seen.to(torch.int32)), swap(0, seen[:, :, :20]), swap(1, seen[:12]), swap(4, pyr[:, :-1]),
                swap(4, pyr.double()), swap(5, scene["K"][:4]), swap(7, ref.FH + 1), swap(9, 0.0), swap(9, math.inf),
                ok + (-0.001,), ok + (0.0, 0.0), swap(5, -scene["K"])):
        with pytest.raises(ValueError):
            F.observe(*bad)
    assert np.array_equal(seen.cpu().numpy(), want)                   # a refused call changes nothing
    with pytest.raises(ValueError):
        F.depth_pyramid(torch.zeros(4, 5, device=DEV))
    with pytest.raises(ValueError):
        F.depth_pyramid(torch.zeros(1, 4, 5, dtype=torch.float64, device=DEV))
    mass = torch.zeros(ref.DIMS, dtype=torch.int64, device=DEV)
    for kw in ({"min_views": 0}, {"min_views": 65536}, {"threshold": 0}):
        with pytest.raises(ValueError):
            F.distance_known(mass, seen, ref.DIMS, **kw)


# ------------------------------------------------------------------------------------------------
# the sources of frames: a scan directory, the model's own depth, and the command line's routes to both
# ------------------------------------------------------------------------------------------------
DP_SCALE = 0.5                                   # the dataparser's map raw -> model frame: x -> scale (M [x, 1])
DP_M = np.array([[math.cos(0.3), -math.sin(0.3), 0.0, 0.11], [math.sin(0.3), math.cos(0.3), 0.0, -0.07],
                 [0.0, 0.0, 1.0, 0.05]])


def _raw_c2w_cv(E):
    """OpenCV camera-to-world in the scan's RAW frame of the fixture's cameras (E: world-to-camera, model frame)"""
    c2w = np.linalg.inv(np.concatenate([E, np.broadcast_to([0.0, 0, 0, 1], (len(E), 1, 4))], 1))
    raw = c2w.copy()
    raw[:, :3, :3] = DP_M[:, :3].T @ c2w[:, :3, :3]
    raw[:, :3, 3] = (c2w[:, :3, 3] / DP_SCALE - DP_M[:, 3]) @ DP_M[:, :3]
    return raw


def _write_scan(root, scene):
    """a scan directory of the fixture in its raw frame (depth in raw units, a few pixels masked out) and the
    dataparser's file -> (transforms.json, dataparser json, boundary masks)"""
    import json
    from PIL import Image
    for d in ("images", "depths", "boundary_mask"):
        (root / d).mkdir(parents=True)
    raw = _raw_c2w_cv(scene["E"])
    K = scene["K"][0]
    meta = {"fl_x": K[0], "fl_y": K[1], "cx": K[2], "cy": K[3], "w": ref.FW, "h": ref.FH, "frames": []}
    masks = np.ones((5, ref.FH, ref.FW), bool)
    masks[:, 3:6, 40:44] = False
    for i in range(5):
        stem = f"frame_{i:04d}"
        meta["frames"].append({"file_path": f"images/{stem}.png", "transform_matrix": raw[i].tolist()})
        np.save(root / "depths" / f"{stem}.npy", scene["depth"][i].astype(np.float64) / DP_SCALE)
        np.save(root / "boundary_mask" / f"{stem}.npy", masks[i].astype(np.uint8) * 255)
        Image.fromarray(np.zeros((ref.FH, ref.FW, 3), np.uint8)).save(root / "images" / f"{stem}.png")
    (root / "transforms.json").write_text(json.dumps(meta))
    (root / "dataparser_transforms.json").write_text(json.dumps({"transform_matrix": DP_M.tolist(), "scale": DP_SCALE}))
    return str(root / "transforms.json"), str(root / "dataparser_transforms.json"), masks


def _fixture_field():
    from gaussiangrasper_amd import field as F
    f = F.DistanceField(ref.LO, (0.0, -0.12, 0.55), ref.CELL, device=DEV)
    assert tuple(f.dims) == ref.DIMS
    return F, f


def _counts(f):
    return f.seen.cpu().numpy(), f.looked.cpu().numpy()


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def _model_frame_poses(scene):
    """the fixture's cameras as the routes under test must deliver them: the raw OpenCV poses through the library's
    own raw -> model map (frames.c2w_to_scene) reproduce the fixture's world-to-camera matrices"""
    from gaussiangrasper_amd.frames import c2w_to_scene
    c2w_cv = c2w_to_scene(_raw_c2w_cv(scene["E"]), DP_M, DP_SCALE)
    assert np.allclose(np.linalg.inv(c2w_cv)[:, :3, :], scene["E"], atol=1e-12, rtol=0)
    return c2w_cv


@pytest.fixture
def rendered(scene, monkeypatch):
    """mesh.render_depth replaced by the fixture's exact ray cast FROM THE POSE IT IS GIVEN, taken as the OpenGL
    camera-to-world its docstring names; the poses it received are recorded"""
    from gaussiangrasper_amd import mesh
    got = []

    def render_depth(model, c2w, intrinsics, height, width, mask=None, alpha_min=0.0, depth_mode="expected"):
        got.append((np.array(c2w, np.float64), depth_mode))
        E = mesh.opencv_w2c(c2w)[0]
        d = ref.ray_depth(E, np.asarray(intrinsics, np.float64), int(height), int(width))
        return torch.from_numpy(d).to(DEV), None, None

    monkeypatch.setattr(mesh, "render_depth", render_depth)
    return got


@gpu
def test_observe_scan_equals_observe_on_the_frames_it_reads(scene, tmp_path):
    """the scan's raw frame IS the volume's (no transform): depth as mesh.scan_frames hands it on (masked pixels,
    +inf and NaN become 0: no reading), poses inverted from the file's OpenCV camera-to-world"""
    import json
    F, f = _fixture_field()
    (tmp_path / "s").mkdir()
    tj, _, masks = _write_scan(tmp_path / "s" / "scan", scene)
    meta = json.loads(open(tj).read())
    c2w = np.linalg.inv(np.concatenate([scene["E"], np.broadcast_to([0.0, 0, 0, 1], (5, 1, 4))], 1))
    for fr, T in zip(meta["frames"], c2w):
        fr["transform_matrix"] = T.tolist()
    open(tj, "w").write(json.dumps(meta))
    f.observe_scan(str(tmp_path / "s" / "scan"), depth_units_per_metre=1.0 / DP_SCALE, margin=ref.MARGIN,
                   near=ref.NEAR, batch=2)
    raw = scene["depth"].astype(np.float64) / DP_SCALE / (1.0 / DP_SCALE)
    with np.errstate(invalid="ignore"):
        depth = np.where(masks & np.isfinite(raw) & (raw > 0), raw, 0.0).astype(np.float32)
    _, g = _fixture_field()
    g.observe(depth, scene["K"], w2c=np.linalg.inv(c2w)[:, :3, :], margin=ref.MARGIN, near=ref.NEAR)
    assert _same(_counts(f), _counts(g)) and int(g.seen.to(torch.int32).sum()) > 1000
    want = ref.observe(ref.DIMS, ref.GRID, ref.pyramid(depth), ref.FH, ref.FW, scene["K"], np.linalg.inv(c2w)[:, :3, :],
                       F.cell_ball(f.h), ref.MARGIN, ref.NEAR)
    assert _same(_counts(f), want)
    # +inf was free space to infinity in the ray cast and is "no reading" from a sensor: fewer cells are seen
    assert (want[0] <= ref.observe(ref.DIMS, ref.GRID, scene["pyr"], ref.FH, ref.FW, scene["K"], scene["E"],
                                   F.cell_ball(f.h), ref.MARGIN, ref.NEAR)[0] + 1).all()


@gpu
def test_observe_model_renders_at_the_poses_it_is_given_and_equals_observe(scene, rendered):
    from gaussiangrasper_amd.mesh import opencv_to_opengl_c2w, opencv_w2c
    F, f = _fixture_field()
    c2w_gl = opencv_to_opengl_c2w(_model_frame_poses(scene))
    cams = [(c2w_gl[i], scene["K"][i], ref.FH, ref.FW) for i in range(5)]
    f.observe_model(object(), cams, downscale=1.0, margin=ref.MARGIN, near=ref.NEAR, batch=2)
    assert len(rendered) == 5 and all(mode == "median" for _, mode in rendered)
    assert all(np.array_equal(p, c) for (p, _), c in zip(rendered, c2w_gl))
    w2c = opencv_w2c(c2w_gl)
    depth = np.stack([ref.ray_depth(w2c[i], scene["K"][i], ref.FH, ref.FW) for i in range(5)])
    _, g = _fixture_field()
    g.observe(depth, scene["K"], c2w=c2w_gl, margin=ref.MARGIN, near=ref.NEAR)
    assert _same(_counts(f), _counts(g))
    want = ref.observe(ref.DIMS, ref.GRID, ref.pyramid(depth), ref.FH, ref.FW, scene["K"], w2c, F.cell_ball(f.h),
                       ref.MARGIN, ref.NEAR)
    assert _same(_counts(f), want)
    solid = ref.solid(ref.centres())
    assert (want[0][~solid] > 0).mean() >= 0.85 and not want[0][solid].any()     # the cameras look AT the scene


def _cli_scene():
    import types
    means = np.array([[-0.2, -0.3, 0.3], [-0.3, -0.2, 0.4]], np.float32)
    return types.SimpleNamespace(
        means=torch.from_numpy(means).to(DEV), quats=torch.tensor([[1.0, 0, 0, 0]] * 2, device=DEV),
        scales=torch.full((2, 3), float(np.log(0.02)), device=DEV), opacities=torch.full((2, 1), 3.0, device=DEV))


@gpu
def test_command_line_brings_the_scans_cameras_into_the_models_frame(scene, rendered, tmp_path, monkeypatch, capsys):
    """--observe-transforms takes the scan's transforms.json (OpenCV camera-to-world, raw frame) through
    --transform-json and the axis flip before observe_model sees it: the stub renderer receives OpenGL poses that
    reproduce the fixture's cameras, and the saved counts are those of DistanceField.observe on the same frames"""
    from gaussiangrasper_amd import _cli, field as F
    from gaussiangrasper_amd.mesh import opencv_to_opengl_c2w, opencv_w2c
    monkeypatch.setattr(_cli, "load_scene", lambda ckpt: (_cli_scene(), None))
    tj, dp, _ = _write_scan(tmp_path / "scan", scene)
    base = ["--ckpt", "x.ckpt", "--bbox", *map(str, ref.LO), "0.0", "-0.12", "0.55", "--voxel", str(ref.CELL),
            "--transform-json", dp, "--observe-margin", str(ref.MARGIN), "--observe-near", str(ref.NEAR)]
    out = str(tmp_path / "model.npz")
    box = ["-0.4", "-0.4", "0.3", "-0.3", "-0.3", "0.5"]
    assert F.main(base + ["--out", out, "--observe-transforms", tj, "--unknown", "blocked", "--min-views", "2",
                          "--assume-free", *box]) == 0
    line = capsys.readouterr().out
    assert "known free" in line and "unknown counts as blocked" in line
    c2w_gl = opencv_to_opengl_c2w(_model_frame_poses(scene))
    assert len(rendered) == 5
    for (p, _), c in zip(rendered, c2w_gl):
        assert np.allclose(opencv_w2c(p)[0], opencv_w2c(c)[0], atol=1e-12, rtol=0)       # the fixture's cameras
    poses = np.stack([p for p, _ in rendered])
    w2c = opencv_w2c(poses)
    depth = np.stack([ref.ray_depth(w2c[i], scene["K"][i], ref.FH, ref.FW) for i in range(5)])
    _, g = _fixture_field()
    g.observe(depth, scene["K"], c2w=poses, margin=ref.MARGIN, near=ref.NEAR)
    got = F.DistanceField.load(out, device=DEV)
    assert np.array_equal(got.looked.cpu().numpy(), g.looked.cpu().numpy())
    g.assume_free([float(v) for v in box[:3]], [float(v) for v in box[3:]])
    assert np.array_equal(got.seen.cpu().numpy(), g.seen.cpu().numpy())
    solid = ref.solid(ref.centres())
    seen = g.seen.cpu().numpy()
    assert (seen[~solid] > 0).mean() >= 0.85 and not seen[solid].any()
    mass = got.mass.cpu().numpy()
    assert (mass >= got.threshold).sum() > 0
    assert np.array_equal(got.dist2.cpu().numpy(), ref.distance_known(mass, got.threshold, seen, 2))
    # the sensor's route: the same map for the poses, the depth times the scale
    rendered.clear()
    out2 = str(tmp_path / "scan.npz")
    assert F.main(base + ["--out", out2, "--observe-scan", str(tmp_path / "scan")]) == 0
    assert not rendered and "unknown counts as free" in capsys.readouterr().out
    masks = np.ones((5, ref.FH, ref.FW), bool)                        # _write_scan's
    masks[:, 3:6, 40:44] = False
    raw = scene["depth"].astype(np.float64) / DP_SCALE
    with np.errstate(invalid="ignore"):
        d = np.where(masks & np.isfinite(raw) & (raw > 0), raw, 0.0).astype(np.float32) * np.float32(DP_SCALE)
    _, g2 = _fixture_field()
    g2.observe(d, scene["K"], w2c=np.linalg.inv(_model_frame_poses(scene))[:, :3, :], margin=ref.MARGIN, near=ref.NEAR)
    got2 = F.DistanceField.load(out2, device=DEV)
    assert _same(_counts(got2), _counts(g2)) and int(g2.seen.to(torch.int32).sum()) > 1000
    assert np.array_equal(got2.dist2.cpu().numpy(), field_ref.distance(mass, got2.threshold))   # --unknown free
