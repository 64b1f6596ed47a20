"""GPU checks of object instances (gaussiangrasper_amd.cluster on gg_cluster_dbscan / gg_cluster_stats) against the
fp64 restatement (tests/cluster_ref.py): labels, core flags, neighbour counts and the number of clusters EQUAL on
blobs, the tie lattice, duplicates, both extremes of min_points, masks, non-finite rows, points far outside the grid,
long chains and a million points; determinism; the statistics (counts and boxes equal, fp64 sums within the
summation bound M 2^-52 sum|terms|); and two mugs on a table end to end through grasp proposals and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cluster_ref as R

gpu = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(p, eps, mp, active=None, grid=None):
    from gaussiangrasper_amd.cluster import dbscan
    pts = torch.as_tensor(np.ascontiguousarray(p, np.float32)).to(DEV)
    m = None if active is None else torch.as_tensor(np.ascontiguousarray(active)).to(DEV)
    c = dbscan(pts, eps, mp, m, grid)
    torch.cuda.synchronize()
    return dict(labels=c.labels.cpu().numpy(), core=c.core.cpu().numpy(),
                neighbor_count=c.neighbor_count.cpu().numpy(), num_clusters=c.num_clusters)


def check(got, ref):
    assert got["labels"].dtype == np.int32 and got["neighbor_count"].dtype == np.int32 and got["core"].dtype == bool
    assert np.array_equal(got["neighbor_count"], ref["neighbor_count"])
    assert np.array_equal(got["core"], ref["core"])
    assert got["num_clusters"] == ref["num_clusters"]
    assert np.array_equal(got["labels"], ref["labels"])


def border(ref):
    return int(((ref["labels"] >= 0) & ~ref["core"]).sum())


# ------------------------------------------------------------------------------------------------
# the kernel against the restatement
# ------------------------------------------------------------------------------------------------
@gpu
def test_blobs_plus_noise_50k():
    p = R.blobs(11, 50_000)
    ref = R.restate(p, 0.012, 6)
    check(run(p, 0.012, 6), ref)
    assert ref["num_clusters"] > 1 and border(ref) > 100 and (ref["labels"] < 0).sum() > 100


@gpu
@pytest.mark.parametrize("mp", [1, 4, 7])
def test_the_tie_lattice(mp):
    p = R.lattice()
    ref = R.restate(p, 0.25, mp)
    assert ref["near"] > 1000
    check(run(p, 0.25, mp), ref)


@gpu
def test_duplicates():
    p = R.with_duplicates(5, 30_000)
    ref = R.restate(p, 0.012, 6)
    check(run(p, 0.012, 6), ref)
    assert ref["num_clusters"] > 1 and border(ref) > 0


@gpu
def test_both_extremes_of_min_points():
    p = R.blobs(12, 20_000)
    ref = R.restate(p, 0.012, 1)
    got = run(p, 0.012, 1)
    check(got, ref)
    assert got["core"].all() and (got["labels"] >= 0).all()          # every point is core, none is noise
    top = int(ref["neighbor_count"].max())
    got = run(p, 0.012, top + 1)
    check(got, R.restate(p, 0.012, top + 1))
    assert got["num_clusters"] == 0 and (got["labels"] == -1).all() and not got["core"].any()
    assert run(p, 0.012, top)["num_clusters"] >= 1


@gpu
def test_an_active_mask_selecting_a_third():
    p = R.blobs(13, 60_000)
    act = np.random.default_rng(13).random(len(p)) < 1.0 / 3.0
    ref = R.restate(p, 0.02, 5, act)
    for a in (act, act.astype(np.uint8) * 7):
        got = run(p, 0.02, 5, a)
        check(got, ref)
        assert (got["labels"][~act] == -1).all() and (got["neighbor_count"][~act] == 0).all()
    assert ref["num_clusters"] > 1 and border(ref) > 0
    # the same as clustering the selected rows alone
    sub = run(p[act], 0.02, 5)
    assert np.array_equal(sub["labels"], ref["labels"][act]) and sub["num_clusters"] == ref["num_clusters"]


@gpu
def test_non_finite_rows_are_inactive_and_change_nothing_else():
    p = R.blobs(14, 30_000)
    clean = run(p, 0.012, 6)
    rng = np.random.default_rng(14)
    bad = rng.choice(len(p), 300, replace=False)
    q = p.copy()
    q[bad[:100], rng.integers(0, 3, 100)] = np.nan
    q[bad[100:200], rng.integers(0, 3, 100)] = np.inf
    q[bad[200:], rng.integers(0, 3, 100)] = -np.inf
    ref = R.restate(q, 0.012, 6)
    got = run(q, 0.012, 6)
    check(got, ref)
    assert (got["labels"][bad] == -1).all() and (got["neighbor_count"][bad] == 0).all() and not got["core"][bad].any()
    # against the same cloud with those rows masked out instead
    act = np.ones(len(p), bool)
    act[bad] = False
    check(run(p, 0.012, 6, act), ref)
    assert clean["num_clusters"] >= 1


@gpu
@pytest.mark.parametrize("sides", [1, 2])
def test_points_far_outside_the_fitted_grid(sides):
    """a tenth of the cloud 1e3 .. 1e6 box sizes away on one side, then on two: the fitted grid ignores them, they
    sit in its border cells, and the result does not change"""
    p = R.blobs(15, 40_000)
    rng = np.random.default_rng(15)
    far = rng.choice(len(p), 4000, replace=False)
    p[far[:2000]] += np.float32([1e3, 0, 0]) if sides == 1 else np.float32([1e3, -1e6, 0])
    if sides == 2:
        p[far[2000:]] += np.float32([-1e4, 0, 3e5])
    else:
        p[far[2000:]] = p[far[2000:]] * np.float32(0.5) + np.float32([2e5, 0.1, 0.2])    # a second, denser lump
    ref = R.restate(p, 0.012, 5)
    check(run(p, 0.012, 5), ref)
    assert (ref["labels"][far] >= 0).sum() > 0 and ref["num_clusters"] > 1
    # any grid gives the same result: one cell, and a grid that misses the cloud altogether
    one = (np.array([0.0, 0.0, 0.0, 1.0]), np.ones(3, np.int32))
    off = (np.array([50.0, 50.0, 50.0, 0.001]), np.array([40, 30, 20], np.int32))
    small = R.blobs(16, 3000)
    ref = R.restate(small, 0.03, 5)
    for g in (one, off, None):
        check(run(small, 0.03, 5, grid=g), ref)


@gpu
@pytest.mark.parametrize("shuffled", [False, True])
def test_one_chain_of_200k_points_is_one_cluster(shuffled):
    """label propagation's worst case: every point sees its two chain neighbours only"""
    n, eps = 200_000, 1.0
    p = R.helix(n, 0.9 * eps)
    if shuffled:
        p = p[np.random.default_rng(17).permutation(n)]
    got = run(p, eps, 3)
    assert got["num_clusters"] == 1 and (got["labels"] == 0).all()
    assert got["core"].sum() == n - 2 and sorted(got["neighbor_count"].tolist())[:3] == [2, 2, 3]
    check(got, R.restate(p, eps, 3))


@gpu
def test_two_interleaved_chains_are_two_clusters():
    n, eps = 100_000, 1.0
    a, b = R.helix(n, 0.9 * eps), R.helix(n, 0.9 * eps, z0=np.pi)     # half a turn's rise apart: pi > eps
    p = np.concatenate([a, b])
    perm = np.random.default_rng(18).permutation(2 * n)
    p = p[perm]
    got = run(p, eps, 2)
    check(got, R.restate(p, eps, 2))
    assert got["num_clusters"] == 2
    first = (perm < n)
    assert len(set(got["labels"][first])) == 1 and len(set(got["labels"][~first])) == 1
    assert got["labels"][first][0] != got["labels"][~first][0]


@gpu
def test_a_million_points_at_about_16_neighbours():
    p = R.blobs(19, 1_000_000, num_blobs=40, sigma=0.035, noise=0.1)
    eps = 0.006
    ref = R.restate(p, eps, 8)
    med = float(np.median(ref["neighbor_count"]))
    print(f"1M: median neighbour count {med}, {ref['num_clusters']} clusters, {border(ref)} border points")
    assert 8 <= med <= 32 and ref["num_clusters"] > 1 and border(ref) > 1000
    check(run(p, eps, 8), ref)


@gpu
def test_two_runs_are_bit_equal_warm_and_fresh_workspace():
    from gaussiangrasper_amd import cluster
    p = R.with_duplicates(20, 200_000)
    pts = torch.as_tensor(p).to(DEV)
    runs = []
    for k in range(4):
        if k == 2:                                  # fresh workspace: drop the allocator's cached blocks
            torch.cuda.empty_cache()
        if k == 3:                                  # a workspace full of another call's leftovers
            junk = torch.randint(0, 255, (64 << 20,), dtype=torch.uint8, device=DEV)
            del junk
        c = cluster.dbscan(pts, 0.01, 6)
        st = cluster.cluster_stats(pts, torch.ones(len(p), device=DEV), c)
        runs.append((c.labels.cpu().numpy().tobytes(), c.core.cpu().numpy().tobytes(),
                     c.neighbor_count.cpu().numpy().tobytes(), c.num_clusters, st.count.cpu().numpy().tobytes(),
                     st.bbox.cpu().numpy().tobytes()))
    assert all(r == runs[0] for r in runs[1:]) and runs[0][3] > 1


# ------------------------------------------------------------------------------------------------
# statistics
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [1000, 300_000])
def test_statistics_against_the_restatement(n):
    from gaussiangrasper_amd.cluster import cluster_stats
    rng = np.random.default_rng(n)
    p = (R.blobs(21, n, noise=0.05) - np.float32([0.5, 0.4, -3.0])).astype(np.float32)     # both signs, an offset
    ref = R.restate(p, 0.03 if n == 1000 else 0.008, 5)
    k = ref["num_clusters"]
    assert k > 1
    w = rng.uniform(0.01, 1.0, n).astype(np.float32)
    st = cluster_stats(torch.as_tensor(p).to(DEV), torch.as_tensor(w).to(DEV),
                       (torch.as_tensor(ref["labels"]).to(DEV), k))
    torch.cuda.synchronize()
    rs = R.restate_stats(p, w, ref["labels"], k)
    assert st.count.dtype == torch.int64 and np.array_equal(st.count.cpu().numpy(), rs["count"])
    assert st.bbox.dtype == torch.float32 and np.array_equal(st.bbox.cpu().numpy(), rs["bbox"])
    ew = np.abs(st.weight.cpu().numpy() - rs["weight"])
    ec = np.abs(st.centroid.cpu().numpy() - rs["centroid"])
    print(f"n {n}: worst weight error / bound {(ew / rs['weight_bound']).max():.3g}, centroid "
          f"{(ec / rs['centroid_bound']).max():.3g}")
    assert (ew <= rs["weight_bound"]).all() and (ec <= rs["centroid_bound"]).all()
    # labels out of range are skipped, an empty cluster has count 0 and NaN box
    lab = ref["labels"].copy()
    lab[lab == 0] = k + 5
    st2 = cluster_stats(torch.as_tensor(p).to(DEV), torch.as_tensor(w).to(DEV), (torch.as_tensor(lab).to(DEV), k))
    assert st2.count[0].item() == 0 and torch.isnan(st2.bbox[0]).all() and st2.weight[0].item() == 0.0
    assert np.array_equal(st2.count.cpu().numpy()[1:], rs["count"][1:])


# ------------------------------------------------------------------------------------------------
# two mugs on a table, end to end
# ------------------------------------------------------------------------------------------------
def _shell(rng, n, centre, radii=(0.04, 0.04, 0.05)):
    """n oriented points on an ellipsoid: (points, outward unit normals)"""
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = np.asarray(radii)
    nrm = u / r
    return np.asarray(centre) + u * r, nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def _quats_z_to(nrm):
    """unit quaternions (w, x, y, z) turning local z onto each normal"""
    z = np.array([0.0, 0.0, 1.0])
    ax = np.cross(np.tile(z, (len(nrm), 1)), nrm)
    w = 1.0 + nrm @ z
    q = np.concatenate([w[:, None], ax], 1)
    flip = w < 1e-9                                    # the normal is -z: half a turn about x
    q[flip] = (0.0, 1.0, 0.0, 0.0)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _two_mugs():
    """Two ellipsoid-shell mugs 0.3 m apart (the heavier one first), a table plane under them and speckle all over
    the room (0.5 % of the Gaussians); the mask a query would give: both mugs and the speckle.
    Returns (Scene, mask, membership (N,) int: 0 / 1 the mugs, 2 the table, 3 speckle)."""
    from gaussiangrasper_amd.scene import make_scene
    rng = np.random.default_rng(30)
    pa, na = _shell(rng, 6000, (0.0, 0.0, 0.05))
    pb, nb = _shell(rng, 4000, (0.3, 0.0, 0.05))
    g = np.arange(-60, 101) * 0.005
    tx, ty = (a.ravel() for a in np.meshgrid(g, np.arange(-60, 61) * 0.005, indexing="ij"))
    pt = np.stack([tx, ty, np.full_like(tx, -0.01)], 1)
    nt = np.tile([0.0, 0.0, 1.0], (len(pt), 1))
    total = len(pa) + len(pb) + len(pt)
    ns = int(round(0.005 * total / 0.995))
    ps = rng.uniform([-1.0, -1.0, 0.3], [1.0, 1.0, 1.5], size=(ns, 3))          # in the air, far from everything
    nsn = rng.normal(size=(ns, 3))
    nsn /= np.linalg.norm(nsn, axis=1, keepdims=True)
    # mug 0 has a Gaussian at either pole, and one speckle Gaussian sits on its axis 3 cm above the top: in the tube
    # of the pole seeds, within the gripper's reach, so on the raw mask it is their far "contact"
    pa[:2], na[:2] = [[0.0, 0.0, 0.10], [0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]]
    ps[0], nsn[0] = [0.0, 0.0, 0.13], [0.0, 0.0, 1.0]
    p = np.concatenate([pa, pb, pt, ps])
    n = np.concatenate([na, nb, nt, nsn])
    member = np.concatenate([np.zeros(len(pa), int), np.ones(len(pb), int), np.full(len(pt), 2), np.full(ns, 3)])
    perm = rng.permutation(len(p))
    p, n, member = p[perm], n[perm], member[perm]
    sc = make_scene(len(p), feature_dim=32)
    sc.means = torch.from_numpy(p.astype(np.float32))
    sc.quats = torch.from_numpy(_quats_z_to(n).astype(np.float32))
    sc.scales = torch.log(torch.tensor([0.002, 0.002, 0.0002])).expand(len(p), 3).contiguous()
    sc.opacities = torch.full((len(p), 1), 4.0)
    mask = (member == 0) | (member == 1) | (member == 3)
    return sc, mask, member


@gpu
def test_two_mugs_are_two_instances_and_grasps_stay_on_one():
    from gaussiangrasper_amd.cluster import instance_mask, object_instances
    from gaussiangrasper_amd.grasp_propose import antipodal, choose_seeds, grasp_object
    from gaussiangrasper_amd.grasp import model_points
    sc, mask, member = _two_mugs()
    assert abs((member == 3).mean() - 0.005) < 2e-4
    sc = sc.to(DEV)
    m = torch.from_numpy(mask).to(DEV)
    inst = object_instances(sc, m)                                   # eps derived from the selection itself
    assert len(inst) == 2
    ids = inst.ids.cpu().numpy()
    assert np.array_equal(ids == 0, member == 0) and np.array_equal(ids == 1, member == 1)
    assert (ids[member >= 2] == -1).all()
    assert inst.stats.count.tolist() == [6000, 4000]
    assert np.abs(inst.stats.centroid.cpu().numpy() - [[0, 0, 0.05], [0.3, 0, 0.05]]).max() < 5e-3
    assert torch.equal(instance_mask(inst, 0), torch.from_numpy(member == 0).to(DEV))
    assert torch.equal(instance_mask(inst, [0.28, 0.02, 0.0]), torch.from_numpy(member == 1).to(DEV))
    # a given eps, in the means' units, gives the same split
    again = object_instances(sc, m, eps=0.01)
    assert torch.equal(again.ids, inst.ids)
    # grasps on instance 0 touch instance 0 only; on the raw mask a seed's tube reaches the speckle behind the mug
    kw = dict(max_width=0.16, tube_radius=0.003)

    def pairs(msk):
        pts, nrm, w = model_points(sc, msk)
        res = antipodal(pts, nrm, w, choose_seeds(w, 1 << 20), **kw)       # what propose_grasps runs
        return res.pair_idx[res.valid].cpu().numpy()

    one = instance_mask(inst, 0)
    assert (member[pairs(one)] == 0).all()
    assert (member[pairs(m)] == 3).any()                             # the construction: the feature matters
    rows, res, keep = grasp_object(sc, one, **kw)
    ci = res.contact_idx.cpu().numpy()[keep.cpu().numpy()]
    assert len(ci) > 0 and (member[ci] == 0).all()


@gpu
def test_grasp_propose_cli_with_instance_largest(tmp_path):
    """--object-points around both mugs selects both (and the speckle between); --instance largest proposes on one"""
    from gaussiangrasper_amd import interop
    sc, mask, member = _two_mugs()
    interop.save_checkpoint(tmp_path / "step-000029999.ckpt", sc, None, 29999)
    lo, hi = np.array([-0.06, -0.06, -0.005]), np.array([0.36, 0.06, 0.4])
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    np.save(tmp_path / "obj.npy", corners)
    base = [sys.executable, "-m", "gaussiangrasper_amd.grasp_propose", "--ckpt", str(tmp_path / "step-000029999.ckpt"),
            "--object-points", str(tmp_path / "obj.npy"), "--max-width", "0.16", "--num-approach", "2"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    outs = {}
    for name, extra in (("all", []), ("largest", ["--instance", "largest", "--cluster-eps", "0.01"]),
                        ("second", ["--instance", "1", "--cluster-min-points", "6"])):
        rep = tmp_path / f"{name}.npz"
        r = subprocess.run(base + extra + ["--out", str(tmp_path / f"{name}.npy"), "--report", str(rep)], env=env,
                           cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        z = np.load(rep)
        outs[name] = member[z["contact_idx"][z["feasible"].astype(bool)]]
    assert len(outs["largest"]) > 0 and (outs["largest"] == 0).all()
    assert len(outs["second"]) > 0 and (outs["second"] == 1).all()
    assert {0, 1} <= set(outs["all"].ravel().tolist())
    r = subprocess.run(base + ["--instance", "7", "--out", str(tmp_path / "x.npy")], env=env, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "instances" in r.stderr
    # the cluster tool itself: instance numbers per Gaussian and a report
    r = subprocess.run([sys.executable, "-m", "gaussiangrasper_amd.cluster", "--ckpt",
                        str(tmp_path / "step-000029999.ckpt"), "--object-points", str(tmp_path / "obj.npy"),
                        "--out", str(tmp_path / "labels.npy"), "--report", str(tmp_path / "stats.json")], env=env,
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lab = np.load(tmp_path / "labels.npy")
    assert lab.dtype == np.int32 and np.array_equal(lab == 0, member == 0) and np.array_equal(lab == 1, member == 1)
    rep = json.loads((tmp_path / "stats.json").read_text())
    assert rep["num_instances"] == 2 and rep["count"] == [6000, 4000]
