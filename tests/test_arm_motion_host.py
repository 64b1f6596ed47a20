"""No-GPU checks of the arm's motion test: the sweep bound's table against finite differences, the theorem the
outputs of gg_arm_motion are read by (by brute force on the restatement, tests/arm_motion_ref.py), the default table
of tested frame pairs, the claims of the fixtures the GPU tests rest on, connect's selection rule, and the Arm
record's JSON with and without `pairs`."""
import json

import numpy as np
import pytest

import arm_motion_ref as mref
import arm_ref as ref


def _speeds(arm, J, q, spheres, frame, eps=1e-6):
    """(N, J, S) central-difference |d c_s / d q_j|"""
    out = np.empty((len(q), J, len(spheres)))
    for j in range(J):
        d = np.zeros(J)
        d[j] = eps
        hi = ref.sphere_centres(arm, J, q + d, spheres, frame)
        lo = ref.sphere_centres(arm, J, q - d, spheres, frame)
        out[:, j] = np.linalg.norm(hi - lo, axis=2) / (2 * eps)
    return out


@pytest.mark.parametrize("which", ["default", "prismatic"])
def test_reach_table_bounds_the_speed_of_every_centre(which):
    """on 256 configurations within the limits; the difference quotient is good to about eps^2 |c'''| + ulp / eps,
    1e-9 here, and the table may be attained (a centre at its full distance from an axis), hence the 1e-8"""
    from gaussiangrasper_amd import arm as A
    rng = np.random.default_rng(17)
    if which == "default":
        arm, J = ref.default_chain()
        model = A.default_arm()
        c, frame, _ = model.link_spheres()
        spheres = c.astype(np.float64)
        table = model.reach_table()
        assert np.array_equal(table, A.reach_table(model, c, frame))
    else:
        arm, J = ref.random_chain(8, 5, prismatic=(2, 5))
        base, fixed, axis, lo, hi, kind = ref.unpack(arm, J)
        spheres = rng.uniform(-0.1, 0.1, size=(30, 3))
        frame = rng.integers(0, J + 2, size=30)
        model = A.Arm(base, fixed, axis, lo, hi, kind)
        table = A.reach_table(model, spheres, frame)
    assert table.shape == (J, len(spheres))
    assert np.abs(table - mref.reach_table(arm, J, spheres, frame)).max() <= 1e-15
    assert (table[np.arange(J)[:, None] >= np.asarray(frame)[None, :]] == 0).all()
    q = ref.in_limits(arm, J, 256, rng, inset=0.0)
    speed = _speeds(arm, J, q, spheres, frame)
    assert (speed <= table[None] + 1e-8).all(), float((speed - table[None]).max())
    kind = ref.unpack(arm, J)[5]
    moved = np.arange(J)[:, None] < np.asarray(frame)[None, :]
    for j in range(J):
        if kind[j] == 1.0:                                          # a sliding joint moves what rides on it at speed 1
            assert np.abs(speed[:, j, moved[j]] - 1.0).max() <= 1e-8 and (table[j, moved[j]] == 1.0).all()


def test_sample_count_is_decided_by_the_comparisons():
    res = 0.1
    for k in (1, 3, 7, 4096):
        B = float(k) * res
        assert mref.sample_count(B, res, 4096) == k                 # n res >= B holds with equality
        assert mref.sample_count(np.nextafter(B, np.inf), res, 4096) == (k + 1 if k < 4096 else 0)
    assert mref.sample_count(0.0, res, 4096) == 1
    assert mref.sample_count(np.inf, res, 4096) == 0


@pytest.mark.parametrize("which", ["default", "prismatic"])
def test_edge_fixture_claims(which):
    """what the GPU tests take for granted, on all 257 edges, none excluded"""
    f = mref.edge_fixture(which)
    w = f["want"]
    n = w["samples"]
    assert np.array_equal(n, np.array(mref.TARGETS)[np.arange(257) % len(mref.TARGETS)])
    assert w["face"].min() > 1e-9, float(w["face"].min())          # no sampled centre near a cell face
    ratio = w["B"] / f["res"]
    assert (np.abs(ratio - np.round(ratio)) > 1e-9 * np.maximum(ratio, 1.0)).all()      # B not near a multiple of res
    assert w["runner_up"].min() > 1e-9, float(w["runner_up"].min())  # the smallest gap stands alone
    assert (w["slack"] < 0).any() and (w["slack"] >= 0).any()
    assert (w["slack_at"] > 0).any() and (w["gap_at"] > 0).any() and (w["gap_at"] == 0).any()
    assert np.isfinite(w["gap"]).all() and len(np.unique(w["pair"], axis=0)) >= 4
    if f["lo"] is not None:                                         # the sliding joints stay within their limits
        kind = ref.unpack(f["arm"], f["J"])[5] == 1.0
        for q in (f["q_a"], f["q_b"]):
            assert ((q >= f["lo"]) & (q <= f["hi"]))[:, kind].all()


def test_the_verdict_holds_between_the_samples():
    """the theorem of include/gg_raster.h by brute force: every edge of the fixture that the restatement calls ok is
    sampled 64 times finer, and there every ball of radius + margin stays out of the occupied cubes (exact distance
    to the blocks) and every tested pair keeps self_margin"""
    f = mref.edge_fixture("default")
    from gaussiangrasper_amd.field import need2
    arm, J, res = f["arm"], f["J"], f["res"]
    margin, self_margin = 0.01, 0.005
    need = need2(f["radius"] + 0.5 * res, margin, res)
    sel = np.arange(0, 257, 2)
    got = mref.motion(arm, J, (f["dims"], f["grid"], f["dist2"]), f["q_a"][sel], f["q_b"][sel], f["spheres"], f["frame"],
                      need, ref.FAR, f["radius"], f["pairs"], f["reach"], res)
    ok = (got["samples"] > 0) & (got["slack"] >= 0) & (got["gap"] >= self_margin + res)
    assert ok.sum() >= 10 and (got["samples"][ok] >= 63).any(), (int(ok.sum()), got["samples"][ok].max())
    clearance, distance = np.inf, np.inf
    for e in np.nonzero(ok)[0]:
        q = mref.samples_of(f["q_a"][sel][e], f["q_b"][sel][e], 64 * int(got["samples"][e]))
        cen = ref.sphere_centres(arm, J, q, f["spheres"].astype(np.float64), f["frame"])
        d = mref.distance_to_occupied(cen.reshape(-1, 3)).reshape(cen.shape[:2]) - f["radius"][None, :]
        clearance = min(clearance, float(d.min()))
        distance = min(distance, float(mref.pair_gaps(cen, f["frame"], f["radius"], f["pairs"], J)[0].min()))
    print(f"{int(ok.sum())} ok edges of {len(sel)}: true clearance {clearance:.4f} >= {margin}, "
          f"true pair distance {distance:.4f} >= {self_margin}")
    assert clearance >= margin and distance >= self_margin


def test_default_self_pairs_of_the_default_arm():
    from gaussiangrasper_amd import arm as A
    model = A.default_arm()
    t = A.default_self_pairs(model)
    assert t.shape == (9, 9) and t.dtype == np.uint8 and np.array_equal(t, t.T)
    off = {(a, b) for a in range(9) for b in range(a + 1, 9) if not t[a, b]}
    assert off == {(a, a + 1) for a in range(8)} | {(4, 6), (5, 7)}
    assert (np.diag(t) == 0).all()
    # at home the smallest tested gap is 0.051 m
    c, frame, r = model.link_spheres()
    gap, pair = mref.self_gap(model.to_array(), 7, model.home()[None], c, frame, r, t)
    assert abs(gap[0] - 0.051) < 5e-4 and pair[0].tolist() == [4, 7]
    # the sampled share of self-colliding configurations: frames 4 and 7 lead
    q = np.random.default_rng(7).uniform(model.lo, model.hi, (1024, 7))
    q[0] = model.home()
    only = np.zeros((9, 9), np.uint8)
    only[4, 7] = only[7, 4] = 1
    hit = mref.self_gap(model.to_array(), 7, q, c, frame, r, only)[0] < 0
    assert abs(hit.mean() - 0.099) < 0.002
    # min_gap 1 tests neighbours that do not always overlap; every pair that always overlaps stays off
    assert A.default_self_pairs(model, min_gap=1).sum() >= t.sum()


def test_connect_select_on_hand_made_tables():
    from gaussiangrasper_amd.arm import connect_select
    T, F = True, False
    d_ok = np.array([[T, F, F, T]])
    d_cost = np.array([[1.0, 1.0, 1.0, 1.0]])
    l1_ok = np.array([[T, T, F]])
    l1_cost = np.array([[0.5, 0.2, 0.1]])
    l2_ok = np.array([[T, T, F, T], [T, T, F, T], [T, T, T, T]])
    l2_cost = np.array([[0.7, 0.3, 0.1, 0.5], [1.0, 0.6, 0.1, 0.7], [0.1, 0.1, 0.1, 0.1]])
    via, cost = connect_select(d_ok, d_cost, l1_ok, l1_cost, l2_ok, l2_cost)
    # b = 0: the direct move (1.0) beats the vias (1.2, 1.2); b = 1: no direct move, the vias tie at 0.8: the lowest;
    # b = 2: only via 2 reaches it, and nothing reaches via 2: none; b = 3: via 1 (0.9) beats the direct move (1.0)
    assert via.tolist() == [[-1, 0, -2, 1]]
    assert np.allclose(cost, [[1.0, 0.8, np.inf, 0.9]])
    # a via route of the direct move's cost: the direct move
    via, cost = connect_select([[T]], [[1.0]], [[T]], [[0.5]], [[T]], [[0.5]])
    assert via.tolist() == [[-1]] and cost.tolist() == [[1.0]]
    # no vias at all
    via, cost = connect_select([[T, F]], [[1.0, 1.0]], np.zeros((1, 0), bool), np.zeros((1, 0)), np.zeros((0, 2), bool),
                               np.zeros((0, 2)))
    assert via.tolist() == [[-1, -2]] and cost.tolist() == [[1.0, np.inf]]


def test_json_round_trip_with_and_without_pairs(tmp_path):
    from gaussiangrasper_amd import arm as A
    model = A.default_arm()
    assert model.pairs is None and model.pair_table() is None
    plain = str(tmp_path / "plain.json")
    model.to_json(plain)
    with open(plain) as fh:
        assert "pairs" not in json.load(fh)                         # written only when set: old files stay as they are
    back = A.Arm.from_json(plain)
    assert back.pairs is None and np.array_equal(back.to_array(), model.to_array())
    table = A.default_self_pairs(model)
    table[0, 8] = table[8, 0] = 0
    import dataclasses
    with_pairs = dataclasses.replace(model, pairs=table)
    path = str(tmp_path / "pairs.json")
    with_pairs.to_json(path)
    again = A.Arm.from_json(path)
    assert np.array_equal(again.pair_table(), table) and np.array_equal(again.to_array(), model.to_array())
    assert np.array_equal(again.spheres, model.spheres)
    # a table that is not symmetric, of the wrong size or not 0 / 1 is refused, naming the file
    for bad in (np.triu(table), table[:8, :8], table * 2):
        with open(path) as fh:
            d = json.load(fh)
        d["pairs"] = np.asarray(bad).tolist()
        with open(path, "w") as fh:
            json.dump(d, fh)
        with pytest.raises(ValueError, match="pairs"):
            A.Arm.from_json(path)
