"""Surface hits on the host: the reference (tests/hits_ref.py) holds the properties the contract states, the
constructed cases (tests/hits_cases.py) contain what they were built for, the Python layer refuses bad arguments
without a GPU, and the plate-over-wall fixture separates the expected depth from the median depth."""
import numpy as np
import pytest
import torch

import hits_cases as HC
import hits_ref as HR
import lift_ref as R

SCENES = tuple(R.SCENES)


# ------------------------------------------------------------------------------------------------
# the reference on lift_ref's scenes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_reference_properties(oracle, name):
    c, ref = HR.scene_ref(oracle, name)
    # the last prefix is the whole list: its final_T is the full render's, bit for bit
    assert ref.last_prefix_T.tobytes() == np.ascontiguousarray(c.final_T).tobytes()
    assert ref.ties == 0
    n_hits = []
    for t in HR.THRESHOLDS:
        hit, pos = ref.hit[t], ref.pos[t]
        # a pixel has a hit iff the forward's final_T is <= t_hit (fp32 comparison)
        assert np.array_equal(hit >= 0, c.final_T <= np.float32(t)), (name, t)
        assert np.array_equal(hit >= 0, pos > 0)
        # every hit is a blended entry of that pixel
        yy, xx = np.nonzero(hit >= 0)
        assert (c.W[yy, xx, hit[yy, xx]] > 0).all()
        n_hits.append(int((hit >= 0).sum()))
    print(f"{name}: hits at t = 0.1 / 0.5 / 0.9: {n_hits} of {c.h * c.w} pixels")
    # monotone in t_hit: a hit at t is at or before the hit at t' < t, and exists whenever that one does
    for hi, lo in ((0.9, 0.5), (0.5, 0.1)):
        both = ref.pos[lo] > 0
        assert (ref.pos[hi][both] > 0).all() and (ref.pos[hi][both] <= ref.pos[lo][both]).all()
    if name != "S1":
        assert n_hits[0] < n_hits[1] < n_hits[2]
    # count, and the largest vis
    assert np.array_equal(ref.count, (c.W > 0).sum(axis=-1))
    assert np.array_equal(ref.top_vis, c.W.max(axis=-1))
    assert np.array_equal(ref.top_idx >= 0, ref.count > 0)
    yy, xx = np.nonzero(ref.top_idx >= 0)
    assert np.array_equal(c.W[yy, xx, ref.top_idx[yy, xx]], ref.top_vis[yy, xx])


# ------------------------------------------------------------------------------------------------
# the constructed cases
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HC.NAMES)
def test_constructed_case_contains_what_it_was_built_for(oracle, name):
    case = HC.cases()[name]
    ref = HR.case_ref(oracle, case)
    u, v = case.probe
    pos, hit = ref.pos[case.t_hit], ref.hit[case.t_hit]
    assert int(pos[v, u]) == case.expect_pos, (name, int(pos[v, u]))
    assert sorted(case.ids.tolist()) == list(range(case.n))
    if case.expect_pos:
        tile = (v // 16) * case.tiles_x + u // 16
        assert int(hit[v, u]) == int(case.ids[case.tile_bins[tile, 0] + case.expect_pos - 1]) != case.expect_pos - 1
    assert np.array_equal(hit >= 0, ref.final_T <= np.float32(case.t_hit))
    if name.startswith("hit_at_"):
        # alpha = opacity exactly at the centre: T there is the fp32 product chain
        a, T = np.float32(case.opacity[0, 0]), np.float32(1.0)
        assert a >= HC.ALPHA_MIN
        for k in range(case.expect_pos):
            before, T = T, T * (np.float32(1.0) - a)
        assert before > np.float32(0.5) >= T
        assert case.expect_pos < int(ref.count[v, u]) <= case.n    # the full walk goes on past the hit
    if name == "stops_before_hit":
        assert int(hit[v, u]) == -1 and int(ref.count[v, u]) == 2 and np.float32(1e-4) < ref.final_T[v, u]
        assert ref.final_T[v, u] > np.float32(case.t_hit)
    if name == "near_one":
        assert int(ref.count[v, u]) == 2 and (hit >= 0).sum() >= 1
    if name == "skipped_ahead":
        assert int(ref.count[v, u]) == 4                           # six entries, two of them never blended
        W, _ = HR.weights(oracle, case.ids, case.tile_bins, case.xys, case.conics, case.opacity, case.h, case.w)
        assert not W[..., case.ids[0]].any() and not W[v, u, case.ids[1]]
    if name == "four_quadrants":
        chunks = set()
        for (cu, cv) in ((3, 3), (12, 3), (3, 12), (12, 12)):
            assert pos[cv, cu] > 0
            chunks.add((int(pos[cv, cu]) - 1) // 64)
        assert chunks == {0, 1, 2, 3}
    if name == "empty_between":
        lens = case.tile_bins[:, 1] - case.tile_bins[:, 0]
        assert lens.tolist() == [2, 0, 0, 0, 4, 0, 0, 0, 1]
        empty = np.isin(HR.pixel_tiles(case.h, case.w), np.nonzero(lens == 0)[0])
        assert (hit[empty] == -1).all() and (ref.count[empty] == 0).all() and (ref.top_idx[empty] == -1).all()
        assert (hit >= 0).any()


# ------------------------------------------------------------------------------------------------
# validation without a GPU
# ------------------------------------------------------------------------------------------------
def _proj(n=5):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)   # noqa: E731
    return z(n, 2), z(n), z(n, dt=torch.int32), z(n, 3), z(n, dt=torch.int32), z(n, 1)


def test_blend_hits_refuses_bad_arguments_without_a_gpu():
    from gaussiangrasper_amd import ops
    for t in (0.0, 1e-4, 1.0, 1.5, -0.5, float("nan")):
        with pytest.raises(ValueError, match="t_hit"):
            ops.blend_hits(*_proj(), 8, 8, t_hit=t)
    with pytest.raises(ValueError, match="xys"):
        ops.blend_hits(torch.zeros(5, 3), *_proj()[1:], 8, 8)
    with pytest.raises(ValueError, match="image"):
        ops.blend_hits(*_proj(), 0, 8)
    with pytest.raises(ValueError, match="opacity"):
        ops.blend_hits(*_proj()[:5], torch.zeros(4, 1), 8, 8)
    with pytest.raises(ValueError, match="conics"):
        ops.blend_hits(*_proj()[:3], torch.zeros(5, 2), *_proj()[4:], 8, 8)
    # valid arguments on host tensors: there is no CPU path
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.blend_hits(*_proj(), 8, 8)
    assert ops.check_t_hit(0.5) == 0.5


def test_surface_refuses_bad_arguments_without_a_gpu():
    from gaussiangrasper_amd import surface
    sc, cam, _ = HC.two_layer_scene()
    c2w, K, h, w = cam
    with pytest.raises(ValueError, match="t_hit"):
        surface.view_hits(sc, c2w, K, h, w, t_hit=1.0)
    with pytest.raises(ValueError, match="image"):
        surface.view_hits(sc, c2w, K, 0, w)
    with pytest.raises(ValueError, match="intrinsics"):
        surface.view_hits(sc, c2w, (1.0, 2.0, 3.0), h, w)
    with pytest.raises(ValueError, match="camera matrices"):
        surface.view_hits(sc, np.eye(3), K, h, w)
    with pytest.raises(ValueError, match="mask"):
        surface.view_hits(sc, c2w, K, h, w, mask=torch.ones(3, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="HIP device"):
        surface.view_hits(sc, c2w, K, h, w)
    for bad in ([[w, 0]], [[0, h]], [[-1, 0]], [[0, -1]]):
        with pytest.raises(ValueError, match="outside"):
            surface.pick(sc, cam, bad)
    with pytest.raises(ValueError, match="pixels"):
        surface.pick(sc, cam, [1, 2, 3])
    with pytest.raises(ValueError, match="whole numbers"):
        surface.pick(sc, cam, [[0.5, 1.0]])
    with pytest.raises(ValueError, match="camera"):
        surface.pick(sc, (c2w, K), [[0, 0]])
    with pytest.raises(ValueError, match="stride"):
        surface.point_cloud(sc, [cam], stride=0)
    from gaussiangrasper_amd import mesh
    with pytest.raises(ValueError, match="depth_mode"):
        mesh.render_depth(sc, c2w, K, h, w, depth_mode="mode")
    with pytest.raises(ValueError, match="depth_mode"):
        mesh.mesh_model(sc, [cam], depth_mode="mean")


def test_hit_depth_and_back_projection_on_the_host():
    from gaussiangrasper_amd import surface
    depths = torch.tensor([1.5, 2.5, 0.75])
    hit = torch.tensor([[2, -1], [0, 1]], dtype=torch.int32)
    d = surface.hit_depth(depths, hit)
    assert d.tolist() == [[0.75, float("inf")], [1.5, 2.5]]
    K = (2.0, 4.0, 0.5, 0.25)
    c2w = np.eye(4)
    c2w[:3, 3] = (10.0, 20.0, 30.0)
    p = surface.back_project(d, c2w, K).numpy()
    assert np.isnan(p[0, 1]).all()
    # OpenGL camera: x right, y up, looking down -z; pixel (u, v) = (0, 1) at depth 1.5
    want = np.array([10.0 + (0 - 0.5) * 1.5 / 2.0, 20.0 - (1 - 0.25) * 1.5 / 4.0, 30.0 - 1.5])
    assert np.array_equal(p[1, 0], want.astype(np.float32))


def test_command_line_refuses_before_it_loads_anything(tmp_path, capsys):
    from gaussiangrasper_amd import mesh, surface
    base = ["--ckpt", str(tmp_path / "none.ckpt"), "--transforms", str(tmp_path / "none.json")]
    for extra in ([], ["--out", "c.ply", "--stride", "0"], ["--out", "c.ply", "--t-hit", "1.0"],
                  ["--out", "c.ply", "--t-hit", "0.0001"], ["--pick", "0", "1", "--out-pick", "p.json"],
                  ["--pick", "0", "1", "2"], ["--out", "c.ply", "--out-pick", "p.json"]):
        with pytest.raises(SystemExit) as e:
            surface.main(base + extra)
        assert e.value.code == 2, extra
    with pytest.raises(SystemExit) as e:
        surface.main(["--out", "c.ply"])
    assert e.value.code == 2
    # a missing transforms.json: an error message and exit status 2, nothing loaded
    assert surface.main(base + ["--out", str(tmp_path / "c.ply")]) == 2
    assert "error:" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        mesh.main(base + ["--out", "m.ply", "--depth-mode", "mode"])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        mesh.main(["--scan", str(tmp_path), "--out", "m.ply", "--depth-mode", "median"])
    assert e.value.code == 2


# ------------------------------------------------------------------------------------------------
# the plate over the wall
# ------------------------------------------------------------------------------------------------
def test_the_two_layer_fixture_separates_expected_from_median(oracle):
    sc, cam, is_plate = HC.two_layer_scene()
    p = R.project(oracle, R.activated(sc), R.view_of(cam))
    W, final_T, bins = R.pixel_weights(oracle, p)
    z = p["depths"].astype(np.float64)
    assert np.allclose(z[is_plate], HC.PLATE_Z, atol=1e-6) and np.allclose(z[~is_plate], HC.WALL_Z, atol=1e-6)
    W64 = W.astype(np.float64)
    A = W64.sum(axis=-1)
    expected = np.where(A >= 0.5, (W64 * z).sum(axis=-1) / np.where(A > 0, A, 1.0), np.inf)
    between = (expected > 1.1) & (expected < 1.9)
    print(f"expected depth in (1.1, 1.9) at {int(between.sum())} pixels, columns "
          f"{np.nonzero(between.any(axis=0))[0].tolist()}")
    assert between.sum() >= 1
    ref = HR.Ref(oracle, bins["gaussian_ids_sorted"], bins["tile_bins"], p["xys"], p["conics"], p["opacity"],
                 HC.LAYER_H, HC.LAYER_W, (0.5,), W=W, final_T=final_T)
    hit = ref.hit[0.5]
    assert (hit[between] >= 0).all()                     # the median has an answer where the mean lies between
    median = np.where(hit >= 0, p["depths"][np.clip(hit, 0, None)], np.inf)
    finite = np.isfinite(median)
    assert finite.mean() > 0.9
    assert np.isin(median[finite], p["depths"]).all()
    assert ((np.abs(median[finite] - HC.PLATE_Z) < 1e-6) | (np.abs(median[finite] - HC.WALL_Z) < 1e-6)).all()
    # both layers are seen
    assert (np.abs(median[finite] - HC.PLATE_Z) < 1e-6).any() and (np.abs(median[finite] - HC.WALL_Z) < 1e-6).any()
