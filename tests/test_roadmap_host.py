"""No-GPU checks of the arm roadmap: the restatement (tests/roadmap_ref.py) against independent forms (a k-d tree, a
plain Bellman-Ford), the quantisation law at its edges, the graph assembly, the string-pulling rule, save / load, the
command line's argument errors, the metric's bound on the sweep, and the claims of the end-to-end fixture the GPU tests
rest on."""
import numpy as np
import pytest

import arm_motion_ref as mref
import arm_ref
import roadmap_ref as rr


# ------------------------------------------------------------------------------------------------
# the restatement against independent forms
# ------------------------------------------------------------------------------------------------
def test_neighbours_restatement_against_a_kd_tree():
    """scipy's cKDTree on the metric-scaled nodes orders by the rounded Euclidean distance, so it is an independent
    form wherever no two candidate distances of a query lie within 1e-9 relative of each other; the fixture is chosen
    so that no query is excluded"""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(11)
    N, M, J, k = 700, 90, 7, 16
    nodes, queries = rng.uniform(-2, 2, size=(N, J)), rng.uniform(-2, 2, size=(M, J))
    metric = np.array([1.3, 1.1, 0.9, 0.8, 0.4, 0.3, 0.1])
    idx, d2 = rr.neighbours(nodes, queries, metric, k)
    d = np.sort(rr.d2_matrix(nodes, queries, metric), axis=1)[:, :k + 1]
    close = (np.diff(d, axis=1) <= 1e-9 * d[:, 1:]).any(1)
    print(f"{int(close.sum())} of {M} queries excluded for near ties")
    assert close.sum() == 0
    dist, want = cKDTree(nodes * metric).query(queries * metric, k=k)
    assert np.array_equal(idx, want)
    assert np.abs(np.sqrt(d2) - dist).max() <= 1e-12
    # the tie rule on a lattice, where the tree's order is not defined: the lowest index among equals, by hand
    lat = np.array([[x, y] for x in range(-2, 3) for y in range(-2, 3)], np.float64)
    idx, d2 = rr.neighbours(lat, np.zeros((1, 2)), np.ones(2), 9)
    assert idx[0].tolist() == [12, 7, 11, 13, 17, 6, 8, 16, 18] and d2[0].tolist() == [0, 1, 1, 1, 1, 2, 2, 2, 2]


def test_route_restatement_against_bellman_ford():
    off, tg, w = rr.knn_graph(300, 5, 3)
    tg, w = tg.copy(), w.copy()
    tg[7], tg[8], w[9], w[10] = -1, 300, 0, 1001                    # ignored edges
    goals = np.array([5, 5, 299, -4, 300, 17], np.int32)
    go = np.array([0, 3, 3, 6], np.int32)                           # query 1 has no goal; query 2 has one in range
    cost, ignored = rr.route(300, off, tg, w, 1000, go, goals)
    assert ignored == 4
    for q in range(3):
        assert np.array_equal(cost[q], rr.bellman_ford(300, off, tg, w, 1000, goals[go[q]:go[q + 1]]))
    assert (cost[1] == rr.FAR).all() and cost[0, 5] == 0 and cost[0, 299] == 0 and cost[2, 17] == 0
    assert (cost[0] < rr.FAR).any() and rr.is_upper_bound_of_walks(300, off, tg, w, 1000, go, goals, cost)
    # descend on it ends on a goal and adds up
    starts = np.arange(0, 300, 7, dtype=np.int32)
    path, n = rr.descend(300, off, tg, w, 1000, cost, np.zeros(len(starts), np.int32), starts, 300)
    for p, s in enumerate(starts):
        if cost[0, s] >= rr.FAR:
            assert n[p] == 0 and (path[p] == -1).all()
            continue
        walk = path[p, :n[p]]
        assert walk[0] == s and walk[-1] in (5, 299) and (path[p, n[p]:] == walk[-1]).all()
        assert len(set(walk.tolist())) == len(walk)


# ------------------------------------------------------------------------------------------------
# the host functions of roadmap.py
# ------------------------------------------------------------------------------------------------
def test_edge_weights_at_multiples_of_the_unit_and_one_ulp_either_side():
    from gaussiangrasper_amd import roadmap as R
    # sqrt(fl(x x)) == x for every double x (barring over- and underflow), and a division by a power of two is exact:
    # with such a unit the quotient is n at L = n unit, and one ulp of L either side of it one ulp either side of n
    for unit in (2.0 ** -10, 0.25, 4.0):
        for n in (1, 2, 3, 7, 100, 16383):
            L = n * unit
            up, down = np.nextafter(L, np.inf), np.nextafter(L, 0.0)
            assert np.sqrt(L * L) == L and np.sqrt(up * up) == up and np.sqrt(down * down) == down
            assert R.edge_weights(L * L, unit) == n
            assert R.edge_weights(up * up, unit) == n + 1
            assert R.edge_weights(down * down, unit) == n
    # with the default unit the quotient is rounded: the law is the literal one, whatever it gives at the multiple
    for n in (1, 2, 3, 7, 100, 16383):
        L = n * 1e-3
        for x in (np.nextafter(L, 0.0), L, np.nextafter(L, np.inf)):
            want = max(1, int(np.ceil(np.sqrt(x * x) / 1e-3)))
            assert R.edge_weights(x * x) == want and n <= want + 1 and want <= n + 1
    assert R.edge_weights(0.0) == 1 and R.edge_weights(1e-30) == 1          # at least 1
    w = R.edge_weights(np.array([np.inf, np.nan, 4e-6, 1.0]), 1e-3)
    assert w[0] == w[1] == np.iinfo(np.int64).max and w[2] == 2 and w[3] == 1000
    # the literal law, element by element
    d2 = np.random.default_rng(2).uniform(0, 30, 1000)
    assert np.array_equal(R.edge_weights(d2, 1e-3), [max(1, int(np.ceil(np.sqrt(x) / 1e-3))) for x in d2])
    with pytest.raises(ValueError, match="unit"):
        R.edge_weights(1.0, 0.0)


def test_assemble_is_symmetric_sorted_free_of_duplicates_and_keeps_indices():
    from gaussiangrasper_amd import roadmap as R
    rng = np.random.default_rng(4)
    N = 50
    a, b = rng.integers(0, N, 400), rng.integers(0, N, 400)
    a[:40], b[:40] = b[40:80].copy(), a[40:80].copy()               # pairs given in both orders
    ok = rng.uniform(size=400) < 0.7
    pair = np.minimum(a, b) * N + np.maximum(a, b)
    w = 1 + pair % 97                                               # a function of the pair: duplicates agree
    first = {}
    for e in range(400):
        first.setdefault(int(pair[e]), e)
    off, tg, wt = R.assemble(N, a, b, ok, w)
    assert off.dtype == tg.dtype == wt.dtype == np.int32 and off[0] == 0 and off[-1] == len(tg) == len(wt)
    dense = np.zeros((N, N), np.int64)
    for i in range(N):
        row = tg[off[i]:off[i + 1]]
        assert (np.diff(row) > 0).all()                             # sorted by target, no parallel edges
        assert (row != i).all()
        dense[i, row] = wt[off[i]:off[i + 1]]
    assert np.array_equal(dense, dense.T)
    want = np.zeros((N, N), np.int64)
    for key, e in first.items():
        lo, hi = divmod(key, N)
        if ok[e] and lo != hi:
            want[lo, hi] = want[hi, lo] = w[e]
    assert np.array_equal(dense, want)
    # a node without an edge keeps its (empty) row, and more nodes only add empty rows
    off2, tg2, wt2 = R.assemble(N + 3, a, b, ok, w)
    assert np.array_equal(off2[:N + 1], off) and (off2[N:] == off[-1]).all() and np.array_equal(tg2, tg)
    e0 = R.assemble(4, [], [], [], [])
    assert e0[0].tolist() == [0] * 5 and len(e0[1]) == 0
    with pytest.raises(ValueError, match="outside"):
        R.assemble(3, [0], [3], [True], [1])
    # candidate_pairs: the union of both lists, each pair once as a < b
    idx = np.array([[1, 2], [0, -1], [3, 0], [-1, -1]])
    pa, pb = R.candidate_pairs(np.arange(4), idx, 4)
    assert list(zip(pa.tolist(), pb.tolist())) == [(0, 1), (0, 2), (2, 3)]


def test_shortcut_select_against_the_brute_force_rule():
    from gaussiangrasper_amd import roadmap as R
    rng = np.random.default_rng(9)
    for window in (1, 2, 3, 8):
        lengths = [0, 1, 2, 3, 9, 17]
        p, i, j = R.shortcut_pairs(lengths, window)
        assert ((j > i) & (j <= i + window)).all() and (j < np.asarray(lengths)[p]).all()
        assert len(p) == sum(min(window, n - 1 - a) for n in lengths for a in range(n))
        assert (np.diff(p * 10000 + i * 100 + j) > 0).all()
        for density in (0.0, 0.3, 1.0):
            ok = rng.uniform(size=len(p)) < density
            table = {(int(a), int(b), int(c)): bool(o) for a, b, c, o in zip(p, i, j, ok)}
            got = R.shortcut_select(lengths, window, ok)
            for path, n in enumerate(lengths):
                want = rr.shortcut_keep(n, window, lambda a, b, path=path: table[(path, a, b)])
                assert got[path].tolist() == want
                if n:
                    assert got[path][0] == 0 and got[path][-1] == n - 1
            if density == 1.0 and window >= 16:
                assert got[5].tolist() == [0, 16]
    assert R.shortcut_select([5], 4, [True] * 10)[0].tolist() == [0, 4]
    assert R.shortcut_select([5], 4, [False] * 10)[0].tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match="window"):
        R.shortcut_pairs([3], 0)
    with pytest.raises(ValueError, match="one entry per pair"):
        R.shortcut_select([3], 2, [True])


def _host_roadmap():
    """the restated fixture as a Roadmap whose Motion sits on the host"""
    import torch
    from gaussiangrasper_amd import roadmap as R
    from gaussiangrasper_amd.arm import Motion
    f = rr.plan_fixture()
    e = f["edges"]
    motion = Motion(*(torch.from_numpy(np.ascontiguousarray(e[k])) for k in ("samples", "slack", "slack_at", "worst", "gap",
                                                                           "gap_at", "pair")),
                    torch.from_numpy(f["ok"]), rr.H, 0.0)
    params = dict(res=rr.H, margin=0.0, self_margin=0.0, spheres=None, radius=0.005, pairs=None, outside="free",
                  max_samples=4096)
    return R.Roadmap(f["nodes"], f["valid"], f["offsets"], f["targets"], f["weights"], f["metric"], R.UNIT, R.MAX_WEIGHT,
                     f["k"], f["a"], f["b"], f["d2"], f["w"], motion, params), f


def test_save_and_load_round_trip(tmp_path):
    from gaussiangrasper_amd import roadmap as R
    rm, _ = _host_roadmap()
    path = str(tmp_path / "roadmap.npz")
    rm.save(path)
    back = R.Roadmap.load(path)
    for name in ("nodes", "valid", "offsets", "targets", "weights", "metric", "edge_a", "edge_b", "edge_d2", "edge_w"):
        a, b = getattr(rm, name), getattr(back, name)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    assert (back.unit, back.max_weight, back.k, back.dropped) == (rm.unit, rm.max_weight, rm.k, rm.dropped)
    for k in R.MOTION_KEYS:
        assert getattr(back.motion, k).numpy().tobytes() == getattr(rm.motion, k).numpy().tobytes(), k
    assert back.motion.res == rm.motion.res and back.motion.self_margin == rm.motion.self_margin
    assert back.params["spheres"] is None and back.params["pairs"] is None and back.params["outside"] == "free"
    assert {k: back.params[k] for k in ("res", "margin", "self_margin", "max_samples", "radius")} == \
        {k: rm.params[k] for k in ("res", "margin", "self_margin", "max_samples", "radius")}
    assert back.arm is None and back.field is None
    with pytest.raises(ValueError, match="attach"):
        back.add(np.zeros((1, 7)))
    # the optional parameters that are arrays, and pairs=False
    rm.params.update(spheres=np.array([[0.0, 0.01, 0.02]], np.float32), pairs=False, radius=np.array([0.01]))
    rm.save(path)
    back = R.Roadmap.load(path)
    assert np.array_equal(back.params["spheres"], rm.params["spheres"]) and back.params["pairs"] is False
    assert np.array_equal(back.params["radius"], [0.01])
    rm.params.update(pairs=np.eye(9, dtype=np.uint8))
    rm.save(path)
    assert np.array_equal(R.Roadmap.load(path).params["pairs"], np.eye(9))
    np.savez(path, nodes=np.zeros((1, 7)))
    with pytest.raises(ValueError, match="not a roadmap"):
        R.Roadmap.load(path)


def test_command_line_argument_errors(tmp_path, capsys):
    from gaussiangrasper_amd import arm as A, roadmap as R
    out = str(tmp_path / "r.npz")
    base = ["build", "--arm", "default", "--out", out]
    for extra, word in ((["--motion-res", "0.02", "--nodes", "0"], "--nodes"),
                        (["--motion-res", "0.02", "--k", "33"], "--k"),
                        (["--motion-res", "0.02", "--unit", "0"], "--unit"),
                        (["--motion-res", "nan"], "--motion-res"),
                        (["--motion-res", "0.02", "--margin", "-1"], "--margin"),
                        (["--motion-res", "0.02", "--max-samples", "0"], "--max-samples"),
                        ([], "--field or --motion-res"),
                        (["--motion-res", "0.02", "--spheres", "s.npy"], "--spheres needs --field")):
        with pytest.raises(SystemExit) as exc:
            R.main(base + extra)
        assert exc.value.code == 2 and word in capsys.readouterr().err
    with pytest.raises(SystemExit) as exc:
        R.main(["plan", "--arm", "default", "--motion-res", "0.02", "--from", "a.npy", "--to", "b.npy", "--out", out,
                "--shortcut", "-1"])
    assert exc.value.code == 2 and "--shortcut" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        R.main(["fly"])
    capsys.readouterr()
    # files that are missing or of the wrong shape: SystemExit with the message, as elsewhere
    with pytest.raises(SystemExit, match="error"):
        R.main(["build", "--arm", str(tmp_path / "none.json"), "--motion-res", "0.02", "--out", out])
    np.save(tmp_path / "bad.npy", np.zeros((2, 5)))
    with pytest.raises(SystemExit, match="expected"):
        R.main(["plan", "--arm", "default", "--motion-res", "0.02", "--from", str(tmp_path / "bad.npy"), "--to",
                str(tmp_path / "bad.npy"), "--out", out])
    # arm's command line: the new option's own errors
    arm_base = ["--arm", "default", "--poses", "p.npy", "--motion-res", "0.02", "--out", out, "--report", out]
    for extra, word in ((["--connect-roadmap", "100"], "goes with --connect-from"),
                        (["--connect-from", "q.npy", "--connect-roadmap", "0"], "--connect-roadmap"),
                        (["--connect-from", "q.npy", "--connect-roadmap", "many"], "--connect-roadmap")):
        with pytest.raises(SystemExit) as exc:
            A.main(arm_base + extra)
        assert exc.value.code == 2 and word in capsys.readouterr().err


@pytest.mark.parametrize("which", ["default", "eight"])
def test_default_metric_bounds_the_sweep(which):
    """B <= sqrt(J) sqrt(d2) on 256 random edges: b_s = sum_j |dq_j| reach[j][s] <= sum_j |dq_j| metric[j] =
    |e|_1 <= sqrt(J) |e|_2.  The slack allowed is the rounding of the J-term sums: J ulps of the value."""
    from gaussiangrasper_amd import arm as A, roadmap as R
    rng = np.random.default_rng(23)
    if which == "default":
        model = A.default_arm()
        extra = np.array([[0.0, 0.0, 0.0], [-0.03, 0.04, 0.0]], np.float32)
        metric = R.default_metric(model, extra, 0.01)
        c, f, _ = A._self_set(model, extra, 0.01)
        assert np.array_equal(R.default_metric(model), model.reach_table().max(1))
    else:
        chain, J = arm_ref.random_chain(8, 5, prismatic=(2, 5))
        base, fixed, axis, lo, hi, kind = arm_ref.unpack(chain, J)
        sph = np.concatenate([rng.integers(0, J + 2, size=(23, 1)).astype(np.float64), rng.uniform(-0.1, 0.1, (23, 3)),
                              rng.uniform(0.02, 0.06, (23, 1))], 1)
        model = A.Arm(base, fixed, axis, lo, hi, kind, sph)
        metric = R.default_metric(model)
        c, f, _ = model.link_spheres()
    J = model.num_joints
    reach = A.reach_table(model, c, f)
    assert metric.shape == (J,) and np.array_equal(metric, reach.max(1)) and (metric > 0).any()
    qa = rng.uniform(model.lo, model.hi, size=(256, J))
    qb = rng.uniform(model.lo, model.hi, size=(256, J))
    L = np.sqrt(R.metric_d2(qa, qb, metric))
    B = np.array([mref.sweep_bound(qa[e], qb[e], reach) for e in range(256)])
    assert (B <= np.sqrt(J) * L * (1 + 4 * J * np.finfo(np.float64).eps)).all(), float((B / (np.sqrt(J) * L)).max())
    assert (B > 0.2 * L).all()                                      # and the bound is not idle
    # metric_d2 is the restatement's d2, to the bit
    assert np.array_equal(R.metric_d2(qa, qb, metric), np.diag(rr.d2_matrix(qb, qa, metric)))
    assert np.array_equal(R.metric_d2(qa, qb, metric), R.metric_d2(qb, qa, metric))     # either direction, to the bit


# ------------------------------------------------------------------------------------------------
# the end-to-end fixture's claims
# ------------------------------------------------------------------------------------------------
def test_plan_fixture_claims():
    """what the GPU tests take for granted: the conditions tests/test_arm_motion_host.py uses for equality of the
    device's verdicts with the restatement's, on every node and every candidate edge, none excluded"""
    from gaussiangrasper_amd import roadmap as R
    f = rr.plan_fixture()
    N = len(f["nodes"])
    assert N == f["num_nodes"] + 2 and np.array_equal(f["nodes"][0], f["model"].home())
    assert np.array_equal(f["nodes"][N - 2], rr.Q_LEFT) and np.array_equal(f["nodes"][N - 1], rr.Q_RIGHT)
    assert f["valid"][N - 2] and f["valid"][N - 1] and 0 < (f["valid"] == 0).sum() < N
    assert not f["ok"][f["direct"]]                                 # the direct move is not ok
    cost, ignored = rr.route(N, f["offsets"], f["targets"], f["weights"], R.MAX_WEIGHT, [0, 1], [N - 1])
    assert ignored == 0 and 0 < cost[0, N - 2] < rr.FAR             # and a route exists in the restated roadmap
    path, n = rr.descend(N, f["offsets"], f["targets"], f["weights"], R.MAX_WEIGHT, cost, [0], [N - 2], N)
    assert n[0] >= 3 and path[0, 0] == N - 2 and path[0, n[0] - 1] == N - 1
    print(f"{int(f['valid'].sum())} of {N} nodes valid, {int(f['ok'].sum())} of {len(f['a'])} edges ok, route of "
          f"{int(n[0])} nodes at cost {int(cost[0, N - 2])}")
    # no edge touches a node that is not valid, every pair once as a < b
    assert (f["a"] < f["b"]).all() and f["valid"][f["a"]].all() and f["valid"][f["b"]].all()
    assert len(np.unique(f["a"] * N + f["b"])) == len(f["a"])
    assert (f["w"] <= R.MAX_WEIGHT).all()
    # every sampled centre stays 1e-9 from a cell face
    assert f["own"]["face"].min() > 1e-9 and f["edges"]["face"].min() > 1e-9
    # every sweep bound is 1e-9 relative from a multiple of res (a node against itself has B = 0 and n = 1 exactly)
    assert (f["own"]["B"] == 0).all() and (f["own"]["samples"] == 1).all()
    ratio = f["edges"]["B"] / rr.H
    assert (np.abs(ratio - np.round(ratio)) > 1e-9 * np.maximum(ratio, 1.0)).all()
    assert (f["edges"]["samples"] > 0).all()
    # the smallest gap clears its threshold by more than the restatement's rounding
    assert (np.abs(f["edges"]["gap"] - rr.H) > 1e-9).all() and (np.abs(f["own"]["gap"] - rr.H) > 1e-9).all()
    # the metric bounds every edge's cost: samples <= ceil(sqrt(J) L / res)
    L = np.sqrt(f["d2"])
    assert (f["edges"]["samples"] <= np.ceil(np.sqrt(7) * L / rr.H * (1 + 1e-12))).all()
