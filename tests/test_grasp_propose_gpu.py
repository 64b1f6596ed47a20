"""GPU checks of grasp proposals (gaussiangrasper_amd.grasp_propose on gg_grasp_propose) against the fp64 restatement
(tests/grasp_propose_ref.py): contacts, tube counts and validity exactly, spans to 1e-6 relative, rows to 1e-6, the NaN
pattern exactly, at sizes that are no multiple of any tile or wave, on every closed edge of the contract, with tied
and duplicate extremes, non-finite inputs, zero-length normals and seeds that are out of range or repeated;
determinism and independence of the seed split; a synthetic scene of Gaussians end to end through the friction-cone
filter; and the command-line tool."""
import json
import math

import numpy as np
import pytest
import torch

import grasp_ref
from grasp_propose_ref import box_faces, restate

gpu = pytest.mark.gpu
DEV = "cuda:0"
H = 2.0 ** -8


def run(points, normals, weights, seeds, **kw):
    from gaussiangrasper_amd.grasp_propose import antipodal
    t = [torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(DEV) for a in (points, normals, weights)]
    s = torch.as_tensor(np.ascontiguousarray(seeds, np.int32)).to(DEV)
    r = antipodal(*t, s, **kw)
    torch.cuda.synchronize()
    return {k: getattr(r, k).cpu().numpy() for k in ("pair_idx", "tube_count", "span", "valid", "rows")}


def check(got, ref):
    for k in ("pair_idx", "tube_count", "valid"):
        assert got[k].shape == ref[k].shape and np.array_equal(got[k].astype(np.int64), ref[k].astype(np.int64)), k
    usable = ref["pair_idx"][:, 0] >= 0
    assert np.array_equal(~np.isnan(got["span"]), usable)
    err = np.abs(got["span"][usable].astype(np.float64) - ref["span"][usable])
    assert (err <= 1e-6 * np.abs(ref["span"][usable])).all()
    v = ref["valid"]
    assert got["rows"].shape == ref["rows"].shape
    assert np.isnan(got["rows"][~v]).all() and not np.isnan(got["rows"][v]).any()
    assert np.abs(got["rows"][v].astype(np.float64) - ref["rows"][v]).max(initial=0.0) <= 1e-6


def scene(rng, n, half=0.05):
    """points in a box of half-size `half`, random normals of any length and weights, with NaN / inf points,
    normals and weights, zero weights and zero-length normals sprinkled in"""
    p = rng.uniform(-half, half, size=(n, 3))
    nr = rng.normal(size=(n, 3)) * rng.uniform(0.5, 2.0, size=(n, 1))
    w = rng.uniform(0.0, 1.0, size=n)
    if n >= 100:
        q = np.array_split(rng.choice(n, size=max(6, n // 150), replace=False), 6)
        p[q[0], rng.integers(0, 3, len(q[0]))] = np.nan
        p[q[1], 0] = np.inf
        nr[q[2], 1] = -np.inf
        w[q[3]] = np.where(rng.random(len(q[3])) < 0.5, np.nan, -np.inf)
        w[q[4]] = 0.0
        nr[q[5]] = 0.0
    return p.astype(np.float32), nr.astype(np.float32), w.astype(np.float32)


def some_seeds(rng, s, n):
    """s seed indices: mostly in range, some repeated, a few out of range"""
    k = rng.integers(0, n, size=s)
    if s >= 7:
        k[1] = k[0]
        k[2], k[3], k[4] = -1, n, n + 5
        k[s - 1] = k[s // 2]
    return k.astype(np.int32)


@gpu
@pytest.mark.parametrize("k_app", [1, 8, 64])
@pytest.mark.parametrize("s", [1, 65, 4097])
@pytest.mark.parametrize("n", [1, 63, 1000, 100_003])
def test_exact_against_the_restatement(n, s, k_app):
    rng = np.random.default_rng(100 * n + 10 * s + k_app)
    p, nr, w = scene(rng, n)
    seeds = some_seeds(rng, s, n)
    # a sparse cloud gets a wide tube, so that tubes hold more than their seed at every size
    kw = dict(num_approach=k_app, tube_radius=0.003 if n > 1000 else 0.02, up=(0.1, -0.2, 1.0), min_align=0.3)
    got = run(p, nr, w, seeds, **kw)
    ref = restate(p, nr, w, seeds, **kw)
    check(got, ref)
    if n >= 1000 and s == 4097:        # the case has substance: valid and not valid seeds, full tubes
        assert ref["valid"].sum() > 200 and (~ref["valid"] & (ref["pair_idx"][:, 0] >= 0)).sum() > 200
        assert ref["tube_count"].max() > 20


def _axis_frames():
    out = []
    for perm in ([0, 1, 2], [1, 2, 0], [2, 0, 1]):
        for sign in (1.0, -1.0):
            R = np.zeros((3, 3))
            R[perm, np.arange(3)] = (sign, 1.0, sign)
            out.append(R)
    return out


@gpu
def test_points_on_every_closed_edge():
    """small integers times powers of two: every product of the contract is exact, so a point exactly on the tube
    radius, at s s == W W nn, at min_width and at W - 2c decides as written, under every axis permutation"""
    r_, W, w0, c, e = 2.0 ** -8, 2.0 ** -3, 2.0 ** -6, 2.0 ** -6, 2.0 ** -14
    kw = dict(tube_radius=r_, max_width=W, min_width=w0, clearance=c, num_approach=3)
    clusters = [                       # local points (seed first, line along local x), expected count, pair, valid
        ([[0, 0, 0], [2.0 ** -5, r_, 0], [2.0 ** -4, r_ + e, 0], [2.0 ** -4, 0, -r_ - e]], 2, (0, 1), True),
        ([[0, 0, 0], [W, 0, 0], [W + e, 0, 0], [-W - e, 0, 0]], 2, (0, 1), False),
        ([[0, 0, 0], [W - 2 * c, 0, 0]], 2, (0, 1), True),
        ([[0, 0, 0], [W - 2 * c + e, 0, 0]], 2, (0, 1), False),
        ([[0, 0, 0], [-w0, 0, 0]], 2, (1, 0), True),
        ([[0, 0, 0], [-w0 + e, 0, 0]], 2, (1, 0), False),
        ([[0, 0, 0], [2.0 ** -5, 0, e], [2.0 ** -5, e, 0], [-(2.0 ** -5), 0, 0], [-(2.0 ** -5), 0, 0]], 5, (3, 1), True),
    ]
    pts, nrm, seeds, want = [], [], [], []
    for f, R in enumerate(_axis_frames()):
        for k, (loc, cnt, pair, valid) in enumerate(clusters):
            origin = np.array([0.5 * k, 0.5 * f, 0.25 * (k + f)])
            base = sum(len(a) for a in pts)
            pts.append(origin + np.asarray(loc, np.float64) @ R.T)
            nrm.append(np.tile(R[:, 0] * (2.0 if k % 2 else -4.0), (len(loc), 1)))
            seeds.append(base)
            # a normal of the other sign walks the line the other way: lo and hi swap
            pair = pair if k % 2 else pair[::-1]
            want.append((cnt, (base + pair[0], base + pair[1]), valid))
    p, nr = np.concatenate(pts), np.concatenate(nrm)
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    w = np.ones(len(p))
    got = run(p, nr, w, seeds, **kw)
    assert got["tube_count"].tolist() == [x[0] for x in want]
    assert got["pair_idx"].tolist() == [list(x[1]) for x in want]
    assert got["valid"].tolist() == [x[2] for x in want]
    check(got, restate(p, nr, w, seeds, **kw))


@gpu
def test_tied_and_duplicate_extremes_take_the_smallest_index():
    n = 50_000
    rng = np.random.default_rng(11)
    p = rng.uniform(-0.002, 0.002, size=(n, 3)).astype(np.float32)
    for i in (40_000, 3, 17_777):                  # s_lo three times, in three chunks
        p[i] = (-0.03125, 0.0, 0.0)
    for i in (49_999, 12_345, 777):                # s_hi likewise, one of them off the line but at the same s
        p[i] = (0.03125, 0.0, 0.0)
    p[777, 1] = 0.001
    p[5] = 0.0
    nr = np.tile(np.float32([3.0, 0, 0]), (n, 1))
    w = np.ones(n, np.float32)
    seeds = [5, 3, 777, 5]
    got = run(p, nr, w, seeds)
    assert got["pair_idx"][0].tolist() == [3, 777] and got["pair_idx"][3].tolist() == [3, 777]
    assert got["pair_idx"][1].tolist() == [3, 777] and got["valid"][[0, 1, 3]].all()
    assert got["tube_count"][0] > 1000
    check(got, restate(p, nr, w, seeds))


@gpu
def test_unusable_seeds_empty_calls_and_no_points():
    p = np.float32([[0, 0, 0], [0.03, 0, 0], [0.01, np.nan, 0], [0.02, 0, 0], [0.02, 0, 0], [0.02, 0, 0], [0.025, 0, 0]])
    nr = np.float32([[1, 0, 0], [0, 0, 0], [1, 0, 0], [np.inf, 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0]])
    w = np.float32([1, 1, 1, 1, 0, np.nan, 1])
    seeds = [0, 1, 2, 3, 4, 5, 6, 7, -1, 0, 2 ** 31 - 1, -2 ** 31]
    got = run(p, nr, w, seeds, num_approach=2)
    # seed 0: tube {0, 1, 6}; the far contact 1 has a zero-length normal: found, not valid.  Seed 1: n.n == 0;
    # seeds 2..5 take no part; seed 6 is alone in its tube; 7, -1 and the int32 extremes are out of range
    assert got["pair_idx"][0].tolist() == [0, 1] and got["tube_count"][0] == 3 and not got["valid"][0]
    assert abs(got["span"][0] - 0.03) < 1e-7
    assert (got["pair_idx"][1:6] == -1).all() and (got["tube_count"][1:6] == 0).all()
    assert got["pair_idx"][6].tolist() == [6, 6] and got["tube_count"][6] == 1 and got["span"][6] == 0.0
    assert (got["pair_idx"][7:9] == -1).all() and (got["tube_count"][7:9] == 0).all()
    assert got["pair_idx"][9].tolist() == [0, 1] and (got["pair_idx"][10:] == -1).all()
    assert not got["valid"].any() and np.isnan(got["rows"]).all()
    check(got, restate(p, nr, w, seeds, num_approach=2))
    # a contact normal perpendicular to the line fails any min_align > 0 and passes 0
    q, qn = np.float32([[0, 0, 0], [0.025, 0, 0]]), np.float32([[1, 0, 0], [0, 2, 0]])
    assert run(q, qn, np.ones(2), [0], min_align=0.0)["valid"][0]
    assert not run(q, qn, np.ones(2), [0], min_align=1e-3)["valid"][0]
    # S == 0
    got = run(p, nr, w, np.zeros(0, np.int32), num_approach=5)
    assert got["rows"].shape == (0, 5, 17) and got["valid"].shape == (0,) and got["pair_idx"].shape == (0, 2)
    # no point takes part; no points at all
    for pts, nrm, wts in ((p, nr, np.zeros(len(p), np.float32)), (np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0))):
        got = run(pts, nrm, wts, [0, 1, 5])
        assert (got["pair_idx"] == -1).all() and (got["tube_count"] == 0).all() and np.isnan(got["span"]).all()
        assert not got["valid"].any() and np.isnan(got["rows"]).all()
        check(got, restate(pts, nrm, wts, [0, 1, 5]))
    # min_weight moves the line between taking part and not
    assert run(p, nr, np.full(len(p), 0.5, np.float32), [0], min_weight=0.5)["tube_count"][0] == 0
    assert run(p[:1], nr[:1], np.float32([0.5]), [0], min_weight=0.25)["tube_count"][0] == 1


@gpu
def test_far_from_the_origin_the_cull_keeps_the_tube():
    """the object 30 m from the origin, long and short normals: the fp32 cull box holds every point of the tube"""
    rng = np.random.default_rng(13)
    p, nr, w = scene(rng, 20_000, half=0.04)
    p = (p.astype(np.float64) + [30.0, -20.0, 10.0]).astype(np.float32)
    nr = (nr * 10.0 ** rng.uniform(-12, 12, size=(len(nr), 1))).astype(np.float32)
    seeds = some_seeds(rng, 500, len(p))
    kw = dict(tube_radius=0.004, max_width=0.12)
    ref = restate(p, nr, w, seeds, **kw)
    check(run(p, nr, w, seeds, **kw), ref)
    assert ref["valid"].sum() > 50 and ref["tube_count"].max() > 20


@gpu
def test_deterministic_and_independent_of_the_seed_split():
    rng = np.random.default_rng(21)
    p, nr, w = scene(rng, 200_000)
    seeds = some_seeds(rng, 4097, len(p))
    a, b = run(p, nr, w, seeds), run(p, nr, w, seeds)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    perm = rng.permutation(len(seeds))[:700]           # other seed tiles, another chunk count over the points
    c = run(p, nr, w, seeds[perm])
    for k in a:
        assert a[k][perm].tobytes() == c[k].tobytes(), k
    assert a["valid"].sum() > 100


# ------------------------------------------------------------------------------------------------
# a scene of Gaussians, end to end
# ------------------------------------------------------------------------------------------------
SIZE_A = np.array([16 * H, 12 * H, 14 * H])


def _disc_scene(unit=1.0):
    """Box A on a table with box B beside it, as flat discs whose smallest axis is the face normal; lengths times
    `unit`.  Returns (Scene, object mask of A (N,) bool, points, normals, weights as numpy)."""
    from gaussiangrasper_amd.scene import make_scene
    pa, na = box_faces(SIZE_A, H, (0.0, 0.0, 7 * H))                          # stands on z = 0
    pb, nb = box_faces([12 * H, 12 * H, 6 * H], H, (15.5 * H, 0.0, 3 * H))    # 1.5 h beside A's +x face, lower
    g = (np.arange(-40, 41)) * H
    tx, ty = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    pt = np.stack([tx, ty, np.full_like(tx, -0.5 * H)], 1)                    # the table, just under both
    nt = np.tile([0.0, 0.0, 1.0], (len(pt), 1))
    p, n = np.concatenate([pa, pb, pt]) * unit, np.concatenate([na, nb, nt])
    sc = make_scene(len(p), feature_dim=32)
    r = math.sqrt(0.5)
    quat = np.zeros((len(p), 4))
    ax = np.abs(n).argmax(1)
    quat[ax == 2] = (1.0, 0.0, 0.0, 0.0)                                      # local z stays z
    quat[ax == 0] = (r, 0.0, r, 0.0)                                          # about y: z -> x
    quat[ax == 1] = (r, -r, 0.0, 0.0)                                         # about x: z -> y
    sc.means = torch.from_numpy(p.astype(np.float32))
    sc.quats = torch.from_numpy(quat.astype(np.float32))
    sc.scales = torch.log(torch.tensor([0.002, 0.002, 0.0002]) * unit).expand(len(p), 3).contiguous()
    sc.opacities = torch.full((len(p), 1), 4.0)
    mask = np.zeros(len(p), bool)
    mask[:len(pa)] = True
    w = torch.sigmoid(torch.full((len(p),), 4.0)).numpy()
    return sc, mask, p.astype(np.float32), n.astype(np.float32), w


def _check_box_grasps(rows, unit=1.0, clearance=0.005):
    b = rows[:, [5, 8, 11]].astype(np.float64)
    ax = np.abs(b).argmax(1)
    face = np.zeros_like(b)
    face[np.arange(len(b)), ax] = np.sign(b[np.arange(len(b)), ax])
    assert np.abs(b - face).max() <= 1e-6                                     # the closing axis is a face normal
    assert np.abs(rows[:, 1] - unit * (SIZE_A[ax] + 2 * clearance)).max() <= 1e-6 * max(unit, 1.0)
    return ax


@gpu
def test_grasp_object_on_a_box_on_a_table():
    from gaussiangrasper_amd.grasp_propose import grasp_object, propose_grasps
    sc, mask, p, n, w = _disc_scene()
    sc = sc.to(DEV)
    m = torch.from_numpy(mask).to(DEV)
    rows, res, keep = grasp_object(sc, m, num_approach=8)
    assert torch.equal(rows, propose_grasps(sc, m, num_approach=8))
    rows_np, keep_np = rows.cpu().numpy(), keep.cpu().numpy()
    assert rows_np.shape[1] == 17 and len(rows_np) == 8 * int(mask.sum()) and np.isfinite(rows_np).all()
    assert len(keep_np) > 0 and res.feasible.cpu().numpy()[keep_np].all()
    assert (np.diff(rows_np[keep_np, 0].astype(np.float64)) <= 0).all()
    ax = _check_box_grasps(rows_np[keep_np])
    assert {0, 1} <= set(ax.tolist())                                         # both horizontal closings occur
    # contacts on the object only: every contact index is one of A's Gaussians
    ci = res.contact_idx.cpu().numpy()[keep_np]
    assert (ci >= 0).all() and mask[ci].all()
    # the collision term sees the whole scene: equal to the filter's restatement on the scene's points
    others = ~mask
    coll = grasp_ref.restate(p[others], n[others], w[others], rows_np)["collision_weight"]
    got_c = res.collision_weight.cpu().numpy().astype(np.float64)
    assert np.allclose(got_c, coll, rtol=1e-5, atol=1e-6)                     # A's own discs never sit in a finger box
    assert (coll[keep_np] > 0.5).any()                                        # some feasible grasps do hit something
    # with a limit, no kept grasp has table or neighbour opacity inside its finger boxes above it
    rows2, res2, keep2 = grasp_object(sc, m, num_approach=8, max_collision=0.5)
    assert torch.equal(rows2, rows)
    k2 = keep2.cpu().numpy()
    assert 0 < len(k2) < len(keep_np) and (coll[k2] <= 0.5).all()
    assert set(k2.tolist()) == set(keep_np[coll[keep_np] <= 0.5].tolist())
    _check_box_grasps(rows_np[k2])
    # B stands beside A's +x face, lower than A: closing along x is still possible above it
    assert (np.abs(rows_np[k2][:, 5]) > 0.5).any()


@gpu
def test_choose_seeds_and_scale():
    from gaussiangrasper_amd.grasp_propose import choose_seeds, propose_grasps
    from gaussiangrasper_amd.prepare import subsample_indices
    w = torch.tensor([0.5, 0.0, 0.2, float("nan"), -1.0, 0.9, 0.1] * 1000, device=DEV)
    part = np.nonzero(np.tile([True, False, True, False, False, True, True], 1000))[0]
    assert np.array_equal(choose_seeds(w, 4096).cpu().numpy(), part) and choose_seeds(w, 4096).dtype == torch.int32
    got = choose_seeds(w, 1500, seed=7).cpu().numpy()
    assert np.array_equal(got, part[subsample_indices(4000, 3, 7)]) and len(got) == 1333
    assert np.array_equal(choose_seeds(w, 1500, seed=7).cpu().numpy(), got)
    assert not np.array_equal(choose_seeds(w, 1500, seed=8).cpu().numpy(), got)
    assert len(choose_seeds(w, 4096, min_weight=0.4)) == 2000
    with pytest.raises(ValueError, match="max_seeds"):
        choose_seeds(w, 0)
    # the same scene in units of 1/2 m: rows scale with it
    sc, mask, *_ = _disc_scene()
    sc2, *_ = _disc_scene(unit=2.0)
    m = torch.from_numpy(mask).to(DEV)
    a = propose_grasps(sc.to(DEV), m, max_seeds=300).cpu().numpy().astype(np.float64)
    b = propose_grasps(sc2.to(DEV), m, max_seeds=300, scale=2.0).cpu().numpy().astype(np.float64)
    assert len(a) == len(b) > 0
    a[:, 1:4] *= 2.0
    a[:, 13:16] *= 2.0
    assert np.abs(a - b).max() < 1e-6


@gpu
def test_cli_on_a_synthetic_checkpoint(tmp_path):
    pytest.importorskip("scipy")
    from gaussiangrasper_amd import grasp_propose, interop
    from gaussiangrasper_amd.grasp import grasps_to_scene
    scale = 2.0
    sc, mask, p, n, w = _disc_scene(unit=scale)             # the checkpoint holds the scene frame: 2 units a metre
    interop.save_checkpoint(tmp_path / "step-000029999.ckpt", sc, None, 29999)
    M = np.eye(4)
    M[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]          # world -> scene: a quarter turn about z, then a shift
    M[:3, 3] = [0.125, -0.25, 0.0625]
    (tmp_path / "tj.json").write_text(json.dumps({"transform_matrix": M.tolist(), "scale": scale}))
    # the object's cloud in the world frame: the corners of A, 0.2 h outside its faces
    lo, hi = -0.5 * SIZE_A - 0.2 * H, 0.5 * SIZE_A + 0.2 * H
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    corners[:, 2] += 7 * H
    np.save(tmp_path / "obj.npy", (corners - M[:3, 3]) @ M[:3, :3])          # x_world = M3^T (x_scene / scale - M_t)
    out, rep = tmp_path / "grasps.npy", tmp_path / "report.npz"
    assert grasp_propose.main(["--ckpt", str(tmp_path / "step-000029999.ckpt"), "--object-points",
                               str(tmp_path / "obj.npy"), "--transform-json", str(tmp_path / "tj.json"),
                               "--max-seeds", "600", "--num-approach", "4", "--max-collision", "0.5",
                               "--out", str(out), "--report", str(rep)]) == 0
    kept, r = np.load(out), np.load(rep)
    assert set(r.files) == {"grasps_scene", "contact_idx", "normals", "angles", "region_count", "region_weight",
                            "collision_weight", "feasible"}
    f = r["feasible"].astype(bool)
    gs = r["grasps_scene"]
    assert kept.dtype == np.float32 and kept.shape == (f.sum(), 17) and 0 < f.sum() < len(gs)
    assert gs.shape[1] == 17 and len(gs) % 4 == 0 and (r["collision_weight"][f] <= 0.5).all()
    assert (np.diff(kept[:, 0].astype(np.float64)) <= 0).all()
    # the output is in the world frame, in metres: back in the scene frame it is the report's feasible rows by score
    order = np.argsort(-gs[f, 0].astype(np.float64), kind="stable")
    assert np.abs(grasps_to_scene(kept, None, M, scale).astype(np.float64) - gs[f][order]).max() < 1e-5
    # world-frame closing axes are A's face normals turned back by M3^T; widths are A's sides plus 2c, in metres
    b_scene = (M[:3, :3] @ kept[:, [5, 8, 11]].astype(np.float64).T).T
    ax = np.abs(b_scene).argmax(1)
    assert np.abs(np.abs(b_scene[np.arange(len(ax)), ax]) - 1.0).max() < 1e-6
    assert np.abs(kept[:, 1] - (SIZE_A[ax] + 0.01)).max() < 1e-6
    _check_box_grasps(gs[f], unit=scale)
    # every contact is one of A's Gaussians: the hull selected the object
    assert mask[r["contact_idx"][f]].all()
