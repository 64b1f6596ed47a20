"""No-GPU checks of known free space (PARITY.md "Known free space"): the rule of gg_field_observe, as tests/observe_ref.py
restates it, is sound by brute force and useful on the shared fixture; the pyramid, the level choice and the counters at
their edges; the Python layer's host paths and every argument check of it; the C entries' refusals (made on the host,
before any launch)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import observe_ref as ref

D = ctypes.c_double


@pytest.fixture(scope="module")
def scene():
    fx = ref.fixture()
    fx["pyr"] = ref.pyramid(fx["depth"])
    fx["looked"], fx["seen"] = ref.observe_views(ref.DIMS, ref.GRID, fx["pyr"], ref.FH, ref.FW, fx["K"], fx["E"],
                                                 ref.RADIUS, ref.MARGIN, ref.NEAR)
    return fx


# ------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------
def test_fixture_has_every_kind_of_reading(scene):
    d = scene["depth"]
    assert d.shape == (5, ref.FH, ref.FW) and d.dtype == np.float32
    assert np.isinf(d).any() and (d == 0).sum() == 40 and np.isnan(d).sum() == 1 and (d[np.isfinite(d)] >= 0).all()


def test_seen_cells_are_free_through_all_of_their_volume(scene):
    """Soundness by brute force: 40 uniform points in the cube of every (cell, view) counted as seen; each lands on
    an in-image pixel whose RAW depth exceeds the point's camera z by more than the margin.  No violation allowed."""
    rng = np.random.default_rng(7)
    c = ref.centres()
    tested = bad = 0
    for v in range(5):
        cells = c[scene["seen"][v]]
        q = cells[:, None, :] + rng.uniform(-0.5, 0.5, size=(len(cells), 40, 3)) * ref.CELL
        E, K = scene["E"][v], scene["K"][v]
        p = q @ E[:, :3].T + E[:, 3]
        u, w = K[0] * p[..., 0] / p[..., 2] + K[2], K[1] * p[..., 1] / p[..., 2] + K[3]
        inside = (p[..., 2] > 0) & (u >= 0) & (u < ref.FW) & (w >= 0) & (w < ref.FH)
        px, py = np.clip(np.floor(u), 0, ref.FW - 1).astype(int), np.clip(np.floor(w), 0, ref.FH - 1).astype(int)
        raw = scene["depth"][v][py, px].astype(np.float64)
        with np.errstate(invalid="ignore"):
            ok = inside & (raw > p[..., 2] + ref.MARGIN)
        tested += ok.size
        bad += int((~ok).sum())
    assert tested > 250_000 and bad == 0


def test_no_solid_cell_is_seen_and_most_free_cells_are(scene):
    solid = ref.solid(ref.centres())
    any_seen = scene["seen"].any(0)
    assert solid.sum() > 300 and not any_seen[solid].any()
    # usefulness: a rule that marks nothing must not pass.  The restatement reaches 92 % here.
    assert any_seen[~solid].mean() >= 0.85
    assert (scene["seen"] <= scene["looked"]).all() and scene["looked"].any(0).mean() > any_seen.mean()


def test_a_missing_reading_makes_the_view_abstain(scene):
    """Cells whose footprint touches the punched block or the NaN are looked at and not seen, whatever lies behind."""
    pyr = ref.pyramid(np.full((5, ref.FH, ref.FW), 1e9, np.float32))
    lk, sn = ref.observe_views(ref.DIMS, ref.GRID, pyr, ref.FH, ref.FW, scene["K"], scene["E"], ref.RADIUS, 0.0,
                               ref.NEAR)
    assert (lk == sn).all()                          # everything looked at is seen when depth is far everywhere
    holes = np.full((5, ref.FH, ref.FW), 1e9, np.float32)
    holes[1, 12:16, 20:30] = 0.0
    E3, K3 = scene["E"][3], scene["K"][3]
    q = E3[:, :3] @ ref.centres()[6, 4, 10] + E3[:, 3]              # a NaN under a cell that view 3 looks at
    assert lk[3, 6, 4, 10]
    holes[3, int(K3[1] * q[1] / q[2] + K3[3]), int(K3[0] * q[0] / q[2] + K3[2])] = np.nan
    lk2, sn2 = ref.observe_views(ref.DIMS, ref.GRID, ref.pyramid(holes), ref.FH, ref.FW, scene["K"], scene["E"],
                                 ref.RADIUS, 0.0, ref.NEAR)
    assert (lk2 == lk).all() and (sn2 <= sn).all()
    assert (sn[1] & ~sn2[1]).sum() > 0 and sn[3, 6, 4, 10] and not sn2[3, 6, 4, 10]
    assert (sn2[[0, 2, 4]] == sn[[0, 2, 4]]).all()


# ------------------------------------------------------------------------------------------------
# pyramid, levels, counters
# ------------------------------------------------------------------------------------------------
def _pyramid_by_definition(depth):
    """every texel as the minimum over the pixels it covers"""
    d = np.asarray(depth, np.float32)
    with np.errstate(invalid="ignore"):
        clean = np.where(d > 0, d, np.float32(0))
    V, H, W = d.shape
    out = []
    for l, (h, w) in enumerate(ref.level_shapes(H, W)):
        s = 1 << l
        lev = np.empty((V, h, w), np.float32)
        for y in range(h):
            for x in range(w):
                lev[:, y, x] = clean[:, y * s:(y + 1) * s, x * s:(x + 1) * s].reshape(V, -1).min(1)
        out.append(lev.reshape(V, -1))
    return np.concatenate(out, 1)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (5, 1), (2, 2), (3, 5), (37, 53), (16, 16), (17, 33)])
def test_pyramid_levels_offsets_and_special_values(H, W):
    rng = np.random.default_rng(H * 100 + W)
    d = rng.uniform(0.5, 4.0, size=(2, H, W)).astype(np.float32)
    special = np.array([np.inf, 0.0, -1.0, np.nan, -np.inf, -0.0], np.float32)
    where = rng.random((2, H, W)) < 0.3
    d[where] = special[rng.integers(0, len(special), int(where.sum()))]
    pyr = ref.pyramid(d)
    off, S = ref.level_offsets(H, W)
    shapes = ref.level_shapes(H, W)
    assert pyr.shape == (2, S) and shapes[0] == (H, W) and shapes[-1] == (1, 1)
    assert all(s != (1, 1) for s in shapes[:-1]) and list(off) == list(np.cumsum([0] + [h * w for h, w in shapes])[:-1])
    assert np.array_equal(pyr.view(np.uint32), _pyramid_by_definition(d).view(np.uint32))
    lvl0 = pyr[:, :H * W].reshape(2, H, W)
    assert not np.isnan(pyr).any() and (pyr >= 0).all() and not np.signbit(pyr).any()
    assert (lvl0[np.isposinf(d)] == np.inf).all() and (lvl0[~(d > 0)] == 0).all()
    from gaussiangrasper_amd import field as F
    assert F.pyramid_size(H, W) == S


def test_level_choice_from_one_pixel_to_the_whole_image():
    one = lambda au, bu, av, bv, n=6: int(ref.choose_level(np.int64(au), np.int64(bu), np.int64(av), np.int64(bv), n))
    assert one(5, 5, 9, 9) == 0 and one(5, 6, 9, 10) == 0            # one pixel, two by two
    assert one(5, 7, 9, 9) == 1 and one(4, 6, 9, 9) == 1             # three wide: (2, 3), (2, 3)
    assert one(3, 4, 0, 0) == 0 and one(3, 5, 0, 0) == 1 and one(3, 6, 0, 0) == 2    # 3..6 >> 1 = 1..3: one more
    assert one(0, 31, 0, 0) == 4 and one(0, 31, 0, 31) == 4 and one(15, 16, 0, 0) == 0 and one(15, 17, 0, 0) == 1
    # The whole 37 x 53 image: its 2 x 2 level 5.  With sides up to 2^k every index >> (k - 1) is 0 or 1, so the level
    # below the top always qualifies: the 1 x 1 top is chosen only where it is level 0, in a 1 x 1 image.
    assert one(0, 52, 0, 36, 7) == 5 and one(0, 63, 0, 0, 7) == 5 and one(0, 0, 0, 0, 1) == 0
    # the property itself, on random footprints: l qualifies, l - 1 does not
    rng = np.random.default_rng(3)
    a = rng.integers(0, 1000, size=(4, 500))
    Au, Bu, Av, Bv = np.minimum(a[0], a[1]), np.maximum(a[0], a[1]), np.minimum(a[2], a[3]), np.maximum(a[2], a[3])
    l = ref.choose_level(Au, Bu, Av, Bv, 11)
    fits = lambda k: (((Bu >> k) - (Au >> k)) <= 1) & (((Bv >> k) - (Av >> k)) <= 1)
    assert fits(l).all() and (~fits(np.maximum(l - 1, 0)) | (l == 0)).all()


def test_counters_saturate_and_calls_add_up(scene):
    args = (ref.DIMS, ref.GRID)
    cam = (ref.RADIUS, ref.MARGIN, ref.NEAR)
    seen5, looked5 = ref.observe(*args, scene["pyr"], ref.FH, ref.FW, scene["K"], scene["E"], *cam)
    assert seen5.dtype == np.uint16 and seen5.max() <= 5 and looked5.max() == 5
    s2, l2 = ref.observe(*args, scene["pyr"][:2], ref.FH, ref.FW, scene["K"][:2], scene["E"][:2], *cam)
    s2, l2 = ref.observe(*args, scene["pyr"][2:], ref.FH, ref.FW, scene["K"][2:], scene["E"][2:], *cam, seen=s2,
                         looked=l2)
    assert np.array_equal(s2, seen5) and np.array_equal(l2, looked5)
    pre = np.full(ref.DIMS, 65534, np.uint16)
    s, l = ref.observe(*args, scene["pyr"], ref.FH, ref.FW, scene["K"], scene["E"], *cam, seen=pre, looked=pre)
    assert np.array_equal(s, np.where(seen5 >= 1, 65535, 65534)) and np.array_equal(l, np.where(looked5 >= 1, 65535, 65534))


def test_distance_known_blocks_what_was_not_seen(scene):
    import field_ref
    seen5, _ = ref.observe(ref.DIMS, ref.GRID, scene["pyr"], ref.FH, ref.FW, scene["K"], scene["E"], ref.RADIUS,
                           ref.MARGIN, ref.NEAR)
    mass = np.zeros(ref.DIMS, np.int64)
    mass[3, 4, 10] = 40000
    d1, d3 = ref.distance_known(mass, 32768, seen5, 1), ref.distance_known(mass, 32768, seen5, 3)
    assert ((d1 == 0) == ((seen5 < 1) | (mass >= 32768))).all() and ((d3 == 0) == ((seen5 < 3) | (mass >= 32768))).all()
    assert (d3 <= d1).all() and (d1 <= field_ref.distance(mass, 32768)).all()
    full = np.full(ref.DIMS, 65535, np.uint16)
    assert np.array_equal(ref.distance_known(mass, 32768, full, 65535), field_ref.distance(mass, 32768))


# ------------------------------------------------------------------------------------------------
# the Python layer on the host
# ------------------------------------------------------------------------------------------------
def _field():
    from gaussiangrasper_amd import field as F
    f = F.DistanceField((-0.4, -0.4, -0.1), (0.0, -0.12, 0.55), ref.CELL, device="cpu")
    assert tuple(f.dims) == ref.DIMS
    return F, f


def test_cell_ball_and_defaults():
    from gaussiangrasper_amd import field as F
    assert F.cell_ball(ref.CELL) == 0.5 * math.sqrt(3.0) * ref.CELL * (1.0 + 2.0 ** -40) == ref.RADIUS
    assert F.cell_ball(1.0) > math.sqrt(3.0) / 2
    assert (F.OBSERVE_MARGIN, F.OBSERVE_NEAR, F.OBSERVE_MIN_VIEWS) == (0.005, 0.05, 2)
    with pytest.raises(ValueError):
        F.cell_ball(0.0)


def test_assume_free_knowledge_save_load_round_trip(tmp_path):
    F, f = _field()
    assert f.seen is None and f.looked is None
    assert f.knowledge() == {"occupied": 0, "free": 0, "occluded": 0, "unseen": 13 * 9 * 21}
    p0 = str(tmp_path / "plain.npz")
    f.save(p0)
    with np.load(p0) as z:
        assert "seen" not in z.files and "looked" not in z.files      # files without them load as before
    g = F.DistanceField.load(p0, device="cpu")
    assert g.seen is None and g.looked is None
    f.mass[2, 2, 5] = F.THRESHOLD
    f.assume_free((-0.4, -0.4, 0.0), (-0.3, -0.2, 0.1))
    c = ref.centres()
    want = ((c >= (-0.4, -0.4, 0.0)) & (c <= (-0.3, -0.2, 0.1))).all(-1)
    assert f.seen.dtype == torch.uint16 and np.array_equal(f.seen.numpy(), np.where(want, 65535, 0))
    assert want[2, 2, 5] and not f.looked.numpy().any()
    f.looked.view(torch.int16)[10, 1, :3] = 1
    k = f.knowledge()
    assert k == {"occupied": 1, "free": int(want.sum()) - 1, "occluded": 3, "unseen": 13 * 9 * 21 - int(want.sum()) - 3}
    p1 = str(tmp_path / "known.npz")
    f.save(p1)
    g = F.DistanceField.load(p1, device="cpu")
    assert g.seen.dtype == torch.uint16 and np.array_equal(g.seen.numpy(), f.seen.numpy())
    assert np.array_equal(g.looked.numpy(), f.looked.numpy()) and g.knowledge() == k
    f.assume_free((-1, -1, -1), (1, 1, 1))
    assert (f.seen.numpy() == 65535).all() and f.knowledge()["unseen"] == 0
    for bad in (((0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, math.nan)), ((0, 0, 1), (1, 1, 0))):
        with pytest.raises(ValueError):
            f.assume_free(*bad)


def test_python_argument_checks():
    F, f = _field()
    K, E = np.array([[40.0, 41.0, 26.3, 18.1]]), ref.look_at((0.9, 0.2, 0.8), ref.TARGET)[None]
    depth = np.ones((1, 4, 5), np.float32)
    with pytest.raises(ValueError, match="blocked"):
        f.update(unknown="blocked")                                   # nothing was observed
    with pytest.raises(ValueError, match="unknown"):
        f.update(unknown="maybe")
    with pytest.raises(ValueError, match="exactly one"):
        f.observe(depth, K)
    with pytest.raises(ValueError, match="exactly one"):
        f.observe(depth, K, c2w=np.eye(4)[None], w2c=E)
    with pytest.raises(ValueError, match="batch"):
        f.observe(depth, K, w2c=E, batch=0)
    with pytest.raises(ValueError, match="depth"):
        f.observe(np.ones((1, 1, 4, 5), np.float32), K, w2c=E)
    with pytest.raises(ValueError, match="same V"):
        f.observe(depth, np.tile(K, (2, 1)), w2c=E)
    for bad in (np.array([[0.0, 41.0, 1, 1]]), np.array([[40.0, -1.0, 1, 1]])):
        with pytest.raises(ValueError, match="fx and fy"):
            f.observe(depth, bad, w2c=E)
    with pytest.raises(ValueError, match="finite"):
        f.observe(depth, np.array([[40.0, 41.0, math.nan, 1]]), w2c=E)
    with pytest.raises(ValueError, match="finite"):
        f.observe(depth, K, w2c=np.full_like(E, math.inf))
    for kw in ({"margin": -1.0}, {"margin": math.nan}, {"near": 0.0}, {"near": math.inf}):
        with pytest.raises(ValueError, match="margin|near"):
            f.observe(depth, K, w2c=E, **kw)
    assert f.seen is None                                             # a refused call allocates nothing
    with pytest.raises(RuntimeError, match="HIP"):                    # a field on the CPU: refused before the counters
        f.observe(depth, K, w2c=E)
    assert f.seen is None and f.looked is None
    with pytest.raises(ValueError, match="blocked"):
        f.update(unknown="blocked")
    with pytest.raises(ValueError):
        F.pyramid_size(0, 4)
    with pytest.raises(ValueError):
        F.pyramid_size(4, F.MAX_SIDE + 1)
    with pytest.raises(ValueError, match="same V"):
        F.camera_arrays(K, np.zeros((1, 2, 4)))
    k, e = F.camera_arrays(K[0], np.concatenate([E[0], [[0, 0, 0, 1]]]))       # one camera, (4, 4)
    assert k.shape == (1, 4) and e.shape == (1, 3, 4) and k.dtype == e.dtype == np.float64
    # the device calls themselves have no CPU path
    t = torch.zeros(ref.DIMS, dtype=torch.uint16)
    with pytest.raises(RuntimeError, match="HIP"):
        F.observe(t, None, f.grid, f.dims, torch.zeros(1, 27), K, E, 4, 5, 0.03)
    with pytest.raises(RuntimeError, match="HIP"):
        F.depth_pyramid(torch.zeros(1, 4, 5))
    with pytest.raises(RuntimeError, match="HIP"):
        F.distance_known(f.mass, t, f.dims)


def test_command_line_refuses_before_loading_anything(capsys):
    from gaussiangrasper_amd import field as F
    base = ["--ckpt", "none.ckpt", "--bbox", "0", "0", "0", "1", "1", "1", "--out", "o.npz"]
    for extra, word in ((["--unknown", "blocked"], "--unknown blocked needs"), (["--min-views", "0"], "--min-views"),
                        (["--observe-margin", "-1"], "--observe_margin"), (["--observe-near", "0"], "--observe_near"),
                        (["--observe-scan", "a", "--observe-transforms", "b"], "not allowed with")):
        with pytest.raises(SystemExit):
            F.main(base + extra)
        assert word in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------
# the C entries' refusals: on the host, before any launch
# ------------------------------------------------------------------------------------------------
def test_c_entries_refuse_bad_arguments():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    n, a8, a2, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4098), ctypes.c_void_p(4097)
    dims, grid = (ctypes.c_int32 * 3)(*ref.DIMS), (D * 4)(*ref.GRID)
    assert lib.gg_depth_min_pyramid_size(ref.FH, ref.FW) == ref.level_offsets(ref.FH, ref.FW)[1]
    assert lib.gg_depth_min_pyramid_size(1, 1) == 1 and lib.gg_depth_min_pyramid_size(32768, 32768) == (4 ** 16 - 1) // 3
    assert lib.gg_depth_min_pyramid_size(0, 5) == 0 and lib.gg_depth_min_pyramid_size(5, 32769) == 0

    def refused(st, word):
        assert st == -1 and word in lib.gg_last_error(), (st, lib.gg_last_error())

    refused(lib.gg_depth_min_pyramid(-1, 4, 4, a8, a8, n), b"num_views")
    refused(lib.gg_depth_min_pyramid((1 << 20) + 1, 4, 4, a8, a8, n), b"num_views")
    refused(lib.gg_depth_min_pyramid(1, 0, 4, a8, a8, n), b"height")
    refused(lib.gg_depth_min_pyramid(1, 4, 32769, a8, a8, n), b"width")
    refused(lib.gg_depth_min_pyramid(1, 4, 4, n, a8, n), b"null")
    refused(lib.gg_depth_min_pyramid(1, 4, 4, a8, a2, n), b"misaligned")
    assert lib.gg_depth_min_pyramid(0, 4, 4, n, n, n) == 0           # V == 0 writes nothing

    def observe(V=1, H=4, W=4, pyr=a8, K=a8, E=a8, radius=0.03, margin=0.0, near=0.05, seen=a2, looked=n, d=dims, g=grid):
        return lib.gg_field_observe(d, g, V, H, W, pyr, K, E, D(radius), D(margin), D(near), seen, looked, n)

    for bad in (0.0, -1.0, math.inf, math.nan):
        refused(observe(radius=bad), b"radius")
        refused(observe(near=bad), b"near")
    for bad in (-1e-9, math.inf, math.nan):
        refused(observe(margin=bad), b"margin")
    refused(observe(V=-1), b"num_views")
    refused(observe(V=(1 << 20) + 1), b"num_views")
    refused(observe(H=32769), b"height")
    refused(observe(W=0), b"width")
    refused(observe(d=(ctypes.c_int32 * 3)(1025, 1, 1)), b"dims")
    refused(observe(g=(D * 4)(0, 0, 0, 0)), b"grid")
    refused(observe(seen=n), b"seen")
    refused(observe(pyr=n), b"null")
    refused(observe(pyr=a2), b"misaligned")
    refused(observe(K=ctypes.c_void_p(4100)), b"misaligned")
    refused(observe(E=ctypes.c_void_p(4100)), b"misaligned")
    refused(observe(seen=odd), b"misaligned")
    refused(observe(looked=odd), b"misaligned")
    assert observe(V=0, pyr=n, K=n, E=n, seen=n) == 0                # V == 0 leaves both arrays untouched

    ws = ctypes.c_void_p(8192)
    need = lib.gg_field_distance_workspace(dims)

    def known(mass=a8, thr=1, seen=a2, mv=1, out=a8, w=ws, nbytes=None):
        return lib.gg_field_distance_known(dims, mass, thr, seen, mv, out, w, ctypes.c_size_t(need if nbytes is None else nbytes), n)

    refused(known(mv=0), b"min_views")
    refused(known(mv=65536), b"min_views")
    refused(known(thr=0), b"threshold")
    refused(known(seen=n), b"null")
    refused(known(seen=odd), b"misaligned")
    refused(known(mass=ctypes.c_void_p(4100)), b"misaligned")
    refused(known(w=a2), b"ws")
    assert known(nbytes=need - 1) == -3 and b"workspace" in lib.gg_last_error()
    assert lib.gg_abi_version() == 6
