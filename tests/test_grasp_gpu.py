"""GPU checks of grasp filtering (gaussiangrasper_amd.grasp on gg_grasp_contacts): contacts, region counts and
feasibility exactly against the fp64 restatement (tests/grasp_ref.py), normals, angles and weights to 1e-6, for
random scenes at sizes that are no multiple of any tile, points on every box boundary, points at the far corners of
the boxes (the cull's worst case), duplicate extremes, non-finite points, weights and grasp rows; closed forms
(parallel plates at a known tilt, a sphere); determinism; the model path; and the command-line tool."""
import json
import math

import numpy as np
import pytest
import torch

from grasp_ref import grasp_rows, restate, rotation

gpu = pytest.mark.gpu
DEV = "cuda:0"
EXACT = ("contact_idx", "region_count", "feasible")


def run(points, normals, weights, grasps, **kw):
    from gaussiangrasper_amd.grasp import contacts
    t = [torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(DEV) for a in (points, normals, weights, grasps)]
    r = contacts(*t, **kw)
    torch.cuda.synchronize()
    return {k: getattr(r, k).cpu().numpy() for k in ("contact_idx", "normals", "angles", "region_count",
                                                     "region_weight", "collision_weight", "feasible")}


def check(got, ref):
    for k in EXACT:
        assert np.array_equal(got[k].astype(np.int64), ref[k].astype(np.int64)), k
    v = ref["valid"]
    assert np.array_equal(~np.isnan(got["angles"]).any(1), v)
    assert np.array_equal(np.isnan(got["normals"]).all((1, 2)), ~v)
    assert np.allclose(got["normals"][v], ref["normals"][v], rtol=0, atol=1e-6)
    assert np.allclose(got["angles"][v], ref["angles"][v], rtol=0, atol=1e-6)
    for k in ("region_weight", "collision_weight"):
        assert np.allclose(got[k], ref[k], rtol=1e-6, atol=0), k


def scene(rng, n, half=0.05):
    """points in a box of half-size `half` (a tabletop object at metre scale), random normals and weights, with
    NaN / inf points, normals and weights and zero weights sprinkled in"""
    p = rng.uniform(-half, half, size=(n, 3))
    nr = rng.normal(size=(n, 3)) * rng.uniform(0.5, 2.0, size=(n, 1))
    w = rng.uniform(0.0, 1.0, size=n)
    if n >= 100:
        k = rng.choice(n, size=max(5, n // 200), replace=False)
        q = np.array_split(k, 5)
        p[q[0], rng.integers(0, 3, len(q[0]))] = np.nan
        p[q[1], 0] = np.inf
        nr[q[2], 1] = -np.inf
        w[q[3]] = np.where(rng.random(len(q[3])) < 0.5, np.nan, -np.inf)
        w[q[4]] = 0.0
    return p.astype(np.float32), nr.astype(np.float32), w.astype(np.float32)


def candidates(rng, m, points, spread=0.01):
    """m grasps centred near random points, random rotations and sizes; a few rows not valid"""
    fin = np.nonzero(np.isfinite(points).all(1))[0]
    c = points[rng.choice(fin, size=m)] + rng.normal(size=(m, 3)) * spread
    g = grasp_rows(rotation(rng, m), c, rng.uniform(0.01, 0.08, m), rng.uniform(0.005, 0.03, m),
                   rng.uniform(-0.01, 0.04, m), score=rng.random(m))
    if m >= 7:
        g[1, 5] = np.nan                 # non-finite R
        g[3, 16] = np.inf                # non-finite object id
        g[4, 1] = 0.0                    # width 0
        g[5, 3] = -0.05                  # depth < -depth_base
    return g


@gpu
@pytest.mark.parametrize("n", [1, 100, 50_000, 300_000])
@pytest.mark.parametrize("m", [1, 7, 1000])
def test_exact_against_the_restatement(n, m):
    rng = np.random.default_rng(1000 * n + m)
    p, nr, w = scene(rng, n)
    if n == 1:
        p[0] = 0.0
    g = candidates(rng, m, p)
    kw = dict(mu=0.7, max_collision=2.0 if m == 7 else None)
    got = run(p, nr, w, g, **kw)
    ref = restate(p, nr, w, g, **{k: v for k, v in kw.items() if v is not None})
    check(got, ref)
    if n >= 50_000 and m == 1000:      # the case has substance: contacts, valid and feasible grasps all occur
        assert (ref["region_count"] > 0).sum() > 500 and ref["valid"].sum() > 100 and ref["feasible"].sum() > 10


def _perm_rotations():
    out = []
    for perm in ([0, 1, 2], [1, 2, 0], [2, 0, 1], [1, 0, 2], [0, 2, 1], [2, 1, 0]):
        for signs in ([1, 1, 1], [-1, 1, -1], [1, -1, -1], [-1, -1, 1]):
            R = np.zeros((3, 3))
            R[np.arange(3), perm] = signs
            out.append(R)
    return out


@gpu
def test_points_on_the_box_boundaries():
    """dyadic sizes, centres and offsets with axis-permutation rotations: u is exact, so every closed / open edge
    of the region and the finger boxes decides as the contract states"""
    hw, fw, hh, depth, db = 2.0 ** -6, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6
    e = 2.0 ** -13
    u0s = [-db - e, -db, 0.0, depth, depth + e]
    u1s = [-hw - fw - e, -hw - fw, -hw - e, -hw, -e, 0.0, hw, hw + e, hw + fw, hw + fw + e]
    u2s = [-hh - e, -hh, 0.0, hh, hh + e]
    U = np.array(np.meshgrid(u0s, u1s, u2s, indexing="ij")).reshape(3, -1).T
    Rs = _perm_rotations()
    pts, grasps = [], []
    for k, R in enumerate(Rs):
        t = np.array([k * 0.125, -0.25 + k * 0.0625, 0.5])
        pts.append(t + U @ R.T)          # p = t + R u, exact in fp32
        grasps.append(grasp_rows(R[None], [t], 2 * hw, 2 * hh, depth))
    p = np.concatenate(pts).astype(np.float32)
    assert np.array_equal(p.astype(np.float64), np.concatenate(pts))
    g = np.concatenate(grasps)
    rng = np.random.default_rng(5)
    nr = rng.normal(size=p.shape).astype(np.float32)
    w = rng.uniform(0.1, 1.0, size=len(p)).astype(np.float32)
    kw = dict(finger_width=fw, depth_base=db)
    got = run(p, nr, w, g, **kw)
    ref = restate(p, nr, w, g, **kw)
    check(got, ref)
    inside = (U[:, 0] >= -db) & (U[:, 0] <= depth) & (np.abs(U[:, 2]) <= hh) & (np.abs(U[:, 1]) <= hw)
    assert (got["region_count"] == inside.sum()).all()


@gpu
def test_far_corners_survive_the_cull():
    """points at the far corners of the region and of the finger boxes, and one fp32 step either side of them,
    under random rotations and far from the origin: the cull keeps everything the fp64 test keeps"""
    rng = np.random.default_rng(7)
    m = 200
    R = rotation(rng, m)
    t = rng.uniform(-3.0, 3.0, size=(m, 3)) + np.array([10.0, -20.0, 5.0])
    width, height, depth = rng.uniform(0.01, 0.08, m), rng.uniform(0.005, 0.03, m), rng.uniform(-0.01, 0.04, m)
    g = grasp_rows(R, t, width, height, depth)
    G = g.astype(np.float64)
    db, fw = 0.02, 0.004
    pts = []
    for i in range(m):
        hw, hh, dp = 0.5 * G[i, 1], 0.5 * G[i, 2], G[i, 3]
        Ri, ti = G[i, 4:13].reshape(3, 3), G[i, 13:16]
        for u0 in (-db, dp):
            for u1 in (-hw - fw, -hw, hw, hw + fw):
                for u2 in (-hh, hh):
                    x = (ti + Ri @ np.array([u0, u1, u2])).astype(np.float32)
                    for s in (-1, 0, 1):
                        pts.append(np.nextafter(x, np.float32(s * np.inf)) if s else x)
    p = np.array(pts, np.float32)
    rng.shuffle(p)
    nr = rng.normal(size=p.shape).astype(np.float32)
    w = np.ones(len(p), np.float32)
    got = run(p, nr, w, g)
    ref = restate(p, nr, w, g)
    check(got, ref)
    assert ref["region_count"].sum() > m and (ref["collision_weight"] > 0).sum() > m // 2


@gpu
def test_duplicate_extremes_take_the_smallest_index():
    n = 50_000
    rng = np.random.default_rng(11)
    p = rng.uniform(-0.004, 0.004, size=(n, 3)).astype(np.float32)
    # identity frame, width 0.02: the extremes u1 = -0.009 and 0.009 each occur at three indices in three chunks
    for i in (40_000, 3, 17_777):
        p[i] = (0.0, -0.009, 0.0)
    for i in (49_999, 12_345, 777):
        p[i] = (0.001, 0.009, 0.0)
    nr = np.tile(np.float32([0, 1, 0]), (n, 1))
    w = np.ones(n, np.float32)
    g = grasp_rows(np.stack([np.eye(3)] * 3), [[0, 0, 0]] * 3, 0.02, 0.02, 0.01)
    got = run(p, nr, w, g)
    assert (got["contact_idx"] == [3, 777]).all()
    check(got, restate(p, nr, w, g))


@gpu
def test_empty_single_and_no_points():
    g = grasp_rows(np.stack([np.eye(3)] * 3), [[0, 0, 0], [5, 5, 5], [0, 0, 0]], 0.04, 0.02, 0.01)
    g[2, 6] = np.nan
    p = np.float32([[0.0, 0.005, 0.0]])
    nr = np.float32([[0, 1, 0]])
    got = run(p, nr, np.float32([1.0]), g)
    assert got["region_count"].tolist() == [1, 0, 0]
    assert got["contact_idx"].tolist() == [[0, 0], [-1, -1], [-1, -1]]
    assert np.isnan(got["angles"]).all() and not got["feasible"].any()
    got = run(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), g)
    assert got["region_count"].tolist() == [0, 0, 0] and (got["contact_idx"] == -1).all()
    assert np.isnan(got["normals"]).all() and not got["feasible"].any() and (got["region_weight"] == 0).all()
    got = run(p, nr, np.float32([1.0]), np.zeros((0, 17)))
    assert got["feasible"].shape == (0,)


# ------------------------------------------------------------------------------------------------
# closed forms
# ------------------------------------------------------------------------------------------------
def plates(half_gap=0.02, k=41):
    x, z = np.meshgrid(np.linspace(-0.01, 0.01, k), np.linspace(-0.005, 0.005, k // 2))
    x, z = x.ravel(), z.ravel()
    left = np.stack([x, np.full_like(x, -half_gap), z], 1)
    right = np.stack([x, np.full_like(x, half_gap), z], 1)
    p = np.concatenate([left, right])
    nr = np.concatenate([np.tile([0.0, -1.0, 0.0], (len(x), 1)), np.tile([0.0, 1.0, 0.0], (len(x), 1))])
    nr[::3] *= -1.0                                       # normals of either sign
    return p.astype(np.float32), nr.astype(np.float32), np.ones(len(p), np.float32)


def tilted(phis):
    """approach a = z, closing b = (sin phi, cos phi, 0), height c = a x b"""
    R = []
    for phi in phis:
        b = np.array([math.sin(phi), math.cos(phi), 0.0])
        a = np.array([0.0, 0.0, 1.0])
        R.append(np.stack([a, b, np.cross(a, b)], 1))
    return np.array(R)


@gpu
def test_parallel_plates_give_the_tilt_and_the_friction_cone_edge():
    p, nr, w = plates()
    deg = [0.0, 5.0, 10.0, 20.0, 25.0, 26.0, 27.0, 30.0, 40.0]
    phis = np.radians(deg)
    g = grasp_rows(tilted(phis), np.zeros((len(deg), 3)), 0.07, 0.1, 0.01)
    got = run(p, nr, w, g, mu=0.5)
    b = g[:, [5, 8, 11]].astype(np.float64)
    phi32 = np.arccos(np.clip(b[:, 1] / np.linalg.norm(b, axis=1), -1, 1))     # the tilt of the fp32 row
    assert np.allclose(got["angles"], phi32[:, None], atol=1e-6)
    assert np.allclose(got["normals"][:, 0], [0, -1, 0], atol=1e-6)
    assert np.allclose(got["normals"][:, 1], [0, 1, 0], atol=1e-6)
    lim = math.degrees(math.atan(0.5))                                        # 26.57 deg
    assert got["feasible"].tolist() == [d <= lim for d in deg]
    check(got, restate(p, nr, w, g, mu=0.5))


@gpu
def test_points_on_a_sphere_give_near_zero_angles():
    k = 20_000
    i = np.arange(k) + 0.5
    th, ph = np.arccos(1 - 2 * i / k), np.pi * (1 + 5 ** 0.5) * i
    d = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], 1)
    p = (0.02 * d).astype(np.float32)
    nr = (d * np.where(np.arange(k) % 2, 1.0, -1.0)[:, None]).astype(np.float32)
    rng = np.random.default_rng(3)
    g = grasp_rows(rotation(rng, 16), np.zeros((16, 3)), 0.05, 0.05, 0.03)
    got = run(p, nr, np.ones(k, np.float32), g)
    assert got["feasible"].all() and np.nanmax(got["angles"]) < 0.02
    check(got, restate(p, nr, np.ones(k, np.float32), g))


@gpu
def test_two_calls_are_bit_identical():
    rng = np.random.default_rng(21)
    p, nr, w = scene(rng, 300_000)
    g = candidates(rng, 1000, p)
    a, b = run(p, nr, w, g), run(p, nr, w, g)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------------------------------------
# the model path and the command-line tool
# ------------------------------------------------------------------------------------------------
def _model_grasps(rng, means, m=300):
    c = means[rng.choice(len(means), size=m)] + rng.normal(size=(m, 3)) * 0.02
    return grasp_rows(rotation(rng, m), c, rng.uniform(0.05, 0.3, m), rng.uniform(0.02, 0.2, m),
                      rng.uniform(0.0, 0.1, m), score=rng.random(m))


@gpu
def test_score_grasps_on_the_stub_model():
    from gaussiangrasper_amd import edit, grasp, ops, query
    from gaussiangrasper_amd.scene import make_scene
    from gaussiangrasper_amd.stub import StubGaussianSplattingModel
    model = StubGaussianSplattingModel(make_scene(40_000, feature_dim=32)).to(DEV)
    means = model.means.detach()
    rng = np.random.default_rng(31)
    g = _model_grasps(rng, means.cpu().numpy())
    # hand-built oriented points: R(q) column of the smallest scale, sigmoid(opacity)
    R = ops.quat_to_rotmat(model.quats.detach())
    col = model.scales.detach().argmin(dim=1)
    normals = R[torch.arange(len(col), device=DEV), :, col].contiguous()
    w0 = torch.sigmoid(model.opacities.detach()).reshape(-1)
    planes = edit.hull_planes(rng.normal(size=(200, 3)) * 0.3)
    hull, _ = edit.select_and_move(means.contiguous(), None, planes)
    fea_up = [torch.randn(128, 32, device=DEV) * 0.2, torch.randn(128, device=DEV) * 0.1,
              torch.randn(512, 128, device=DEV) * 0.1, torch.randn(512, device=DEV) * 0.1]
    qmask = query.select_gaussians(model, fea_up, rng.normal(size=(1, 512)), rng.normal(size=(2, 512)), 0.5)
    assert 0 < int(hull.sum()) < len(col) and 0 < int(qmask.sum()) < len(col)
    M = np.eye(4)
    M[:3, :3] = rotation(rng, 1)[0]
    M[:3, 3] = [0.1, -0.2, 0.05]
    C = np.eye(4)
    C[:3, :3] = rotation(rng, 1)[0]
    for mask in (None, hull, qmask):
        w = w0 if mask is None else w0 * mask.float()
        for frame in (dict(), dict(cam_to_world=C, matrix=M, scale=0.5)):
            got = grasp.score_grasps(model, g, mask, **frame)
            s = frame.get("scale", 1.0)
            gs = torch.from_numpy(grasp.grasps_to_scene(g, frame.get("cam_to_world"), frame.get("matrix"), s))
            want = grasp.contacts(means, normals, w, gs.to(DEV), depth_base=0.02 * s, finger_width=0.004 * s,
                                  band=0.003 * s)
            for k in ("contact_idx", "normals", "angles", "region_count", "region_weight", "collision_weight",
                      "feasible"):
                a, b = getattr(got, k), getattr(want, k)
                assert torch.equal(a.nan_to_num(-7.0) if a.is_floating_point() else a,
                                   b.nan_to_num(-7.0) if b.is_floating_point() else b), k
            assert int((got.region_count > 0).sum()) > 0


@gpu
def test_cli_on_a_synthetic_checkpoint(tmp_path):
    pytest.importorskip("scipy")
    from gaussiangrasper_amd import grasp, interop
    from gaussiangrasper_amd.scene import make_scene
    sc = make_scene(30_000, feature_dim=32)
    interop.save_checkpoint(tmp_path / "step-000029999.ckpt", sc, {
        "layers.0.weight": torch.randn(128, 32) * 0.2, "layers.0.bias": torch.randn(128) * 0.1,
        "layers.2.weight": torch.randn(512, 128) * 0.1, "layers.2.bias": torch.randn(512) * 0.1}, 29999)
    rng = np.random.default_rng(41)
    C = np.eye(4)
    C[:3, :3] = rotation(rng, 1)[0]
    C[:3, 3] = [0.3, 0.1, -0.2]
    M = np.eye(4)
    M[:3, :3] = rotation(rng, 1)[0]
    scale = 2.0
    # candidates in the grasp frame, placed on Gaussians: world = inv(M) (x / scale), grasp = inv(C) world
    means = sc.means.numpy().astype(np.float64)
    g_scene = _model_grasps(rng, means, 400)
    Gs = g_scene.astype(np.float64)
    A = np.linalg.inv(M[:3, :3] @ C[:3, :3])
    g = Gs.copy()
    g[:, 4:13] = (A @ Gs[:, 4:13].reshape(-1, 3, 3)).reshape(-1, 9)
    world = (Gs[:, 13:16] / scale - M[:3, 3]) @ np.linalg.inv(M[:3, :3]).T
    g[:, 13:16] = (world - C[:3, 3]) @ C[:3, :3]
    g[:, 1:4] /= scale
    g = g.astype(np.float32)
    np.save(tmp_path / "grasps.npy", g)
    np.save(tmp_path / "pose.npy", C)
    (tmp_path / "tj.json").write_text(json.dumps({"transform_matrix": M.tolist(), "scale": scale}))
    obj = tmp_path / "obj.npy"
    np.save(obj, (rng.normal(size=(500, 3)) * 0.4 / scale) @ np.linalg.inv(M[:3, :3]).T)
    common = ["--ckpt", str(tmp_path / "step-000029999.ckpt"), "--grasps", str(tmp_path / "grasps.npy"),
              "--camera-pose", str(tmp_path / "pose.npy"), "--transform-json", str(tmp_path / "tj.json"),
              "--mu", "0.8"]
    for extra in ([], ["--object-points", str(obj)]):
        out, rep = tmp_path / "kept.npy", tmp_path / "report.npz"
        assert grasp.main(common + extra + ["--out", str(out), "--report", str(rep)]) == 0
        kept = np.load(out)
        r = np.load(rep)
        assert set(r.files) == {"grasps_scene", "contact_idx", "normals", "angles", "region_count",
                                "region_weight", "collision_weight", "feasible"}
        assert r["contact_idx"].shape == (400, 2) and r["normals"].shape == (400, 2, 3)
        f = r["feasible"].astype(bool)
        assert 0 < f.sum() == len(kept)
        order = np.argsort(-g[f, 0].astype(np.float64), kind="stable")
        assert np.array_equal(kept, g[f][order])                   # input frame and units, by score
        assert (np.diff(kept[:, 0]) <= 0).all()
        scene_t = torch.from_numpy(r["grasps_scene"]).to(DEV)
        if not extra:      # the whole scene: the report equals a direct call
            from gaussiangrasper_amd.grasp import contacts, model_points
            want = contacts(*model_points(sc.to(DEV)), scene_t, depth_base=0.02 * scale,
                            finger_width=0.004 * scale, band=0.003 * scale, mu=0.8)
            assert np.array_equal(want.feasible.cpu().numpy(), f)
            assert np.array_equal(want.contact_idx.cpu().numpy(), r["contact_idx"])
