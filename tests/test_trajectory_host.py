"""The numpy restatement of the arm-trajectory contract (tests/trajectory_ref.py) against independent forms, on the CPU:
the per-step closed form against scipy's linear programme, both limits inside every interval, a straight move against
the analytic trapezoid, exact scaling, reversal, the blend theorem by brute force, and what every constructed GPU case
(tests/trajectory_cases.py) was built to contain."""
import numpy as np
import pytest

import trajectory_cases as tc
import trajectory_ref as tr


def lp_xbar(qp0, qp1, qpp, delta, nxt, v, a):
    """max x subject to the interval's rows, by scipy: the independent form of step_back"""
    from scipy.optimize import linprog
    two = 2.0 * delta
    A_ub, b_ub = [], []
    for j in range(len(qp0)):
        for B in (qp0[j], two * qpp[j] + qp1[j]):
            A_ub += [[qpp[j], B], [-qpp[j], -B]]
            b_ub += [a[j], a[j]]
    mx = np.maximum(np.abs(qp0), np.abs(qp1))
    cap = min([(v[j] / mx[j]) ** 2 for j in range(len(qp0)) if mx[j] > 0] + [np.inf])
    nxt = min(nxt, cap)
    A_ub += [[1.0, two], [-1.0, -two]]
    b_ub += [nxt, 0.0]
    res = linprog([-1.0, 0.0], A_ub=A_ub, b_ub=b_ub, bounds=[(0.0, None if np.isinf(cap) else cap), (None, None)],
                  method="highs")
    assert res.status == 0, res.message
    return res.x[0]


def interval_draws():
    """(kind, qp0, qp1, qpp, delta, next, v, a) of random intervals of every kind the issue names"""
    rng = np.random.default_rng(3)
    out = []
    for trial in range(120):
        J = int(rng.integers(1, 9))
        v, a = rng.uniform(0.5, 3.0, J), rng.uniform(2.0, 20.0, J)
        delta = float(rng.uniform(0.01, 0.3))
        qp0 = rng.uniform(-2.0, 2.0, J)
        kind = ("line", "blend", "zero", "stop")[trial % 4]
        qpp = np.zeros(J) if kind == "line" else rng.uniform(-8.0, 8.0, J)
        nxt = 0.0 if kind == "stop" else float(rng.uniform(0.0, 6.0))
        if kind == "zero":
            qp0[0] = 0.0                                            # a row whose u coefficient is exactly 0
        qp1 = qp0 + delta * qpp
        out.append((kind, qp0, qp1, qpp, delta, nxt, v, a))
    return out


def test_the_closed_form_of_a_step_is_the_linear_programmes_optimum():
    seen = set()
    for kind, qp0, qp1, qpp, delta, nxt, v, a in interval_draws():
        got = tr.step_back(qp0[None], qp1[None], qpp[None], np.array([delta]), np.array([nxt]), v, a)[0]
        want = lp_xbar(qp0, qp1, qpp, delta, nxt, v, a)
        assert abs(got - want) <= 1e-9 * max(abs(want), 1.0), (kind, got, want)
        seen.add(kind)
        if kind == "zero":
            assert qpp[0] != 0.0 and got <= a[0] / abs(qpp[0]) * (1 + 1e-12)
    assert seen == {"line", "blend", "zero", "stop"}


def test_the_feasible_x_of_a_step_form_an_interval_from_zero():
    # (x, u) = (0, 0) meets every row and the rows are linear: every x in [0, xbar] has a u, none above xbar has
    from scipy.optimize import linprog
    for kind, qp0, qp1, qpp, delta, nxt, v, a in interval_draws()[:40]:
        xbar = tr.step_back(qp0[None], qp1[None], qpp[None], np.array([delta]), np.array([nxt]), v, a)[0]
        two = 2.0 * delta
        vc = tr.vcap(qp0[None], qp1[None], v)[0]
        cu, cl, d, cap = (r[0] for r in tr.rows(qp0[None], qp1[None], qpp[None], np.array([two]),
                                                np.array([min(nxt, vc)]), a))
        for x in (0.0, 0.3 * xbar, xbar * (1 - 1e-9)):
            assert (cl + d * x).max() <= (cu + d * x).min() + 1e-9 and x <= min(cap.min(), vc)
        x = xbar * (1 + 1e-6) + 1e-9
        assert (cl + d * x).max() > (cu + d * x).min() or x > min(cap.min(), vc)


@pytest.mark.parametrize("name", sorted(tc.cases()))
def test_both_limits_hold_inside_every_interval(name):
    c, law = tc.cases()[name], tc.law(name)
    worst_v = worst_a = 0.0
    for p in np.nonzero((law["status"] == tr.OK) & (law["count"] > 0))[0]:
        g = tr.Grid(c["way"][p], c["length"][p], c["blend"][p], c["m"])
        row = {k: law[k][p] for k in ("x", "u")}
        qd, qdd = tr.inside(g, row, 64)
        worst_v = max(worst_v, (np.abs(qd) / c["v"]).max())
        worst_a = max(worst_a, (np.abs(qdd) / c["a"]).max())
        assert law["infeasible"][p] <= 1e-9 * np.abs(law["u"][p, :g.G]).max()
        assert (np.diff(law["t"][p, :g.G + 1]) > 0).all() and (law["x"][p, :g.G + 1] <= law["xbar"][p, :g.G + 1]).all()
    assert worst_v <= 1 + 1e-9 and worst_a <= 1 + 1e-9, (worst_v, worst_a)


def trapezoid(d, v, a):
    """the quickest time of the straight move d under v and a: the analytic trapezoid or triangle"""
    nz = d != 0
    V, A = (v[nz] / np.abs(d[nz])).min(), (a[nz] / np.abs(d[nz])).min()
    return 2.0 * np.sqrt(1.0 / A) if V * V / A >= 1.0 else 1.0 / V + V / A


def test_a_straight_move_against_the_analytic_profile():
    rng = np.random.default_rng(11)
    excess = {}
    for m in (4, 16, 64):
        ratios = []
        for trial in range(8):
            J = 7
            way = rng.uniform(-2, 2, size=(1, 2, J))
            v, a = rng.uniform(0.5, 3.0, J), rng.uniform(2.0, 20.0, J)
            if trial % 2:
                v = v * 100.0                                       # the triangle: the speed limit is never met
            law = tr.time_law(way, [2], np.zeros((1, 2)), v, a, m)
            best = trapezoid(way[0, 1] - way[0, 0], v, a)
            ratios.append(law["duration"][0] / best)
            assert law["duration"][0] >= best * (1 - 1e-12)
        excess[m] = max(ratios)
    print("largest duration / analytic optimum per m:", excess)
    assert excess[64] <= excess[16] <= excess[4]                    # the excess shrinks as the grid is refined


def test_scaling_the_limits_by_powers_of_two_scales_the_law_to_the_bit():
    for name in ("joints7", "fractions", "reversal"):
        c, law = tc.cases()[name], tc.law(name)
        slow = tr.time_law(c["way"], c["length"], c["blend"], c["v"] / 2, c["a"] / 4, c["m"])
        for key, scale in (("x", 0.25), ("xbar", 0.25), ("u", 0.25), ("t", 2.0), ("duration", 2.0)):
            assert np.array_equal(slow[key], law[key] * scale, equal_nan=True), (name, key)


def greedy_is_largest(g):
    """True when no upper line of any interval of the grid falls faster than -1 / (2 Delta): x -> x + 2 Delta u_max(x)
    then does not decrease, the forward sweep's x is the pointwise largest profile that meets the rows, and that
    profile does not know the direction of travel.  Decided from the geometry alone."""
    two = 2.0 * g.delta[:, None]
    ok = True
    for B in (g.qp0, two * g.qpp + g.qp1, -g.qp1, two * g.qpp - g.qp0):         # both ends, both directions of travel
        with np.errstate(divide="ignore", invalid="ignore"):
            ok = ok and bool((np.where(B != 0.0, two * (g.qpp / B), 0.0) <= 1.0).all())
    return ok


def test_reversing_a_path_reverses_x():
    """Where the forward sweep is the largest profile (greedy_is_largest).  Where it is not, the sweep is still within
    the limits but may sit below the largest profile, and the two directions differ: path 9 of case joints7 (m = 3, a
    blend where a joint nearly reverses) differs by 2.5e-6 absolute in x inside that blend."""
    held = blends = 0
    # paths without a reversing joint, |d| in 0.3..1: |q''| 2 Delta = |e| / m <= 0.7 / 16 < 0.3 <= |q'| on every blend
    rng = np.random.default_rng(17)
    mono = np.cumsum(rng.uniform(0.3, 1.0, size=(12, 5, 7)) * np.where(rng.uniform(size=(12, 1, 7)) < 0.5, -1.0, 1.0), 1)
    mono = tc._case(mono, [5] * 12, tc.MENU[rng.integers(1, 4, size=(12, 5))], rng.uniform(0.5, 3.0, 7),
                    rng.uniform(2.0, 20.0, 7), 16)
    todo = [(mono, tr.time_law(mono["way"], mono["length"], mono["blend"], mono["v"], mono["a"], 16))]
    todo += [(tc.cases()[n], tc.law(n)) for n in ("joints2", "joints7", "fractions", "still", "steps16", "limits1e3")]
    for c, law in todo:
        name = c["way"].shape
        P, W, J = c["way"].shape
        way, blend = c["way"].copy(), c["blend"].copy()
        for p in range(P):
            n = c["length"][p]
            way[p, :n], blend[p, :n] = c["way"][p, :n][::-1], c["blend"][p, :n][::-1]
        back = tr.time_law(way, c["length"], blend, c["v"], c["a"], c["m"])
        for p in range(P):
            G = law["count"][p]
            assert back["count"][p] == G
            g = tr.Grid(c["way"][p], c["length"][p], c["blend"][p], c["m"])
            if G == 0 or not greedy_is_largest(g):
                continue
            held += 1
            blends += sum(kind for kind, _, _, _ in g.pieces)
            a, b = law["x"][p, :G + 1], back["x"][p, :G + 1][::-1]
            assert np.abs(a - b).max() <= 1e-9 * np.abs(a).max(), (name, p)
            assert abs(law["duration"][p] - back["duration"][p]) <= 1e-9 * law["duration"][p]
    assert held >= 20 and blends >= 20, (held, blends)


def test_blended_paths_are_quicker_than_stopping_at_every_waypoint():
    gains = {}
    for n in (3, 5, 9):
        way = np.stack([tc.zigzag(n, 7, 100 + n + i) for i in range(4)])
        v, a = np.full(7, 2.0), np.full(7, 10.0)
        stop = tr.time_law(way, [n] * 4, np.zeros((4, n)), v, a, 16)
        half = tr.time_law(way, [n] * 4, np.full((4, n), 0.5), v, a, 16)
        assert (half["duration"] < stop["duration"]).all()
        gains[n] = float(1.0 - (half["duration"] / stop["duration"]).mean())
    print("shorter at f = 1/2 than with stops, by waypoints:", gains)
    c = tc.cases()["fractions"]
    stop = tr.time_law(c["way"], c["length"], np.zeros_like(c["blend"]), c["v"], c["a"], c["m"])
    assert (tc.law("fractions")["duration"] < stop["duration"]).all()


def test_the_blend_theorem_by_brute_force():
    from gaussiangrasper_amd import arm as A
    from gaussiangrasper_amd.trajectory import blend_fractions, sweep_bounds
    arm = A.default_arm()
    c, f, _ = arm.link_spheres()
    rng = np.random.default_rng(21)
    lo, hi = np.asarray(arm.lo), np.asarray(arm.hi)
    kept, worst = 0, 0.0
    for delta in (0.005, 0.05):
        way = rng.uniform(lo, hi, size=(6, 7))
        way[3] = way[2] + 0.02 * (way[3] - way[2])                  # a short segment: its corners may blend by 1/2
        fr = blend_fractions(arm, way, delta)
        B = sweep_bounds(arm, way)
        assert fr[0] == 0 and fr[-1] == 0 and (fr[1:-1] > 0).all() and (fr <= 0.5).all()
        for k in range(1, 5):
            assert fr[k] == min(0.5, 2 * delta / B[k - 1], 2 * delta / B[k])
        g = tr.Grid(way, 6, fr, 4)
        pts = tr.curve(g, 64)                                        # (G, 65, J)
        for i in range(g.G):
            kind, k, fk, L = g.pieces[g.piece[i]]
            if kind == 0:
                continue
            kept += 1
            # the two configurations of the polyline the proof names: X on the incoming segment, Y on the outgoing one
            tau = ((i % 4 + np.arange(65) / 64) / 4)[:, None]
            X = way[k] - ((1.0 - tau) * fk) * (way[k] - way[k - 1])
            Y = way[k] + (tau * fk) * (way[k + 1] - way[k])
            centres = []
            for cfg in (pts[i], X, Y):
                R, t = A._fk_host(arm, cfg)
                centres.append(np.einsum("nsab,sb->nsa", R[:, f], c.astype(np.float64)) + t[:, f])      # (65, S, 3)
            # ONE configuration of the polyline within delta for all spheres at once: what the self test needs
            dx = np.linalg.norm(centres[0] - centres[1], axis=-1).max(axis=1)
            dy = np.linalg.norm(centres[0] - centres[2], axis=-1).max(axis=1)
            worst = max(worst, float(np.minimum(dx, dy).max() / delta))
            assert np.minimum(dx, dy).max() <= delta + 1e-12, (delta, k, np.minimum(dx, dy).max())
    print("largest distance from the polyline's sweep, in units of delta:", worst)
    assert kept >= 16 and worst > 0.0


def test_every_constructed_case_contains_what_it_was_built_for():
    cs = tc.cases()
    for J in (1, 2, 7, 8):
        c = cs[f"joints{J}"]
        assert c["way"].shape[2] == J and set(c["length"]) == {1, 2, 3, 4, 6}
    assert set(cs["longest"]["length"]) == {1, 2, 3, 4, tr.MAX_WAYPOINTS}
    assert tc.law("longest")["count"].max() > 64 * 2
    assert [cs[f"steps{m}"]["m"] for m in (2, 3, 16, 64)] == [2, 3, 16, tr.MAX_STEPS]
    assert [len(cs[f"paths{P}"]["length"]) for P in (1, 63, 64, 65, 1025)] == [1, 63, 64, 65, 1025]
    # fractions: stops, two stops in a row, a tiny blend, a skipped line
    c = cs["fractions"]
    for p in range(2):
        f = tr.fractions(c["blend"][p], 12)
        assert ((f[1:-2] == 0) & (f[2:-1] == 0)).any() and (f == 1e-6).any() and (f == 0.25).any()
        skipped = [(1.0 - f[k]) - f[k + 1] <= 0 for k in range(11)]
        assert any(skipped)
        g = tr.Grid(c["way"][p], 12, c["blend"][p], c["m"])
        assert len(g.pieces) < 2 * 12 - 3 and g.stop[1:-1].sum() >= 2
    # a joint at rest on a segment, and one at rest everywhere
    c = cs["still"]
    d = np.diff(c["way"][0], axis=0)
    assert (d[:, 2] == 0).all() and d[1, 1] == 0 and d[1, 0] != 0
    # the reversal: a row with u coefficient exactly 0 and q'' != 0 at a blend's middle grid point
    c = cs["reversal"]
    for p in range(2):
        g = tr.Grid(c["way"][p], 3, c["blend"][p], c["m"])
        hit = (g.qp0[:, 0] == 0.0) & (g.qpp[:, 0] != 0.0)
        assert hit.sum() == 1 and not g.stop[np.nonzero(hit)[0][0]]
    assert cs["limits1e3"]["v"].max() / cs["limits1e3"]["v"].min() == 1e3
    law = tc.law("bad")
    for p, st in tc.bad_rows().items():
        assert law["status"][p] == st and law["count"][p] == 0 and np.isnan(law["x"][p]).all()
    good = [p for p in range(7) if p not in tc.bad_rows()]
    assert (law["status"][good] == tr.OK).all() and np.isfinite(law["duration"][good]).all()
    law = tc.law("pow2")
    assert law["x"][0].tolist() == [0.0, 4.0, 0.0] and law["t"][0].tolist() == [0.0, 0.5, 1.0]
    assert law["count"][1] == 0 and law["duration"][1] == 0.0


def test_the_sampler_starts_and_ends_at_the_waypoints_and_counts_its_rows():
    c, law = tc.cases()["pow2"], tc.law("pow2")
    q, qd, qdd, num = tr.sample(c["way"], c["length"], c["blend"], c["m"], law, 0.25, 8)
    assert num.tolist() == [5, 1]
    assert q[0, :5, 0].tolist() == [0.0, 0.125, 0.5, 0.875, 1.0] and np.isnan(q[0, 5:]).all()
    assert qd[0, :5, 0].tolist() == [0.0, 1.0, 2.0, 1.0, 0.0] and qdd[0, :5, 0].tolist() == [4.0, 4.0, -4.0, -4.0, -4.0]
    assert q[1, 0, 0] == 3.0 and qd[1, 0, 0] == 0.0 and np.isnan(q[1, 1:]).all()
    q, _, _, num = tr.sample(c["way"], c["length"], c["blend"], c["m"], law, 4.0, 2)      # dt above the duration
    assert num.tolist() == [2, 1] and q[0, :, 0].tolist() == [0.0, 1.0]
    for name in ("joints7", "fractions"):
        c, law = tc.cases()[name], tc.law(name)
        dt = float(np.nanmax(law["duration"])) / 50
        q, qd, qdd, num = tr.sample(c["way"], c["length"], c["blend"], c["m"], law, dt, 64)
        for p in range(len(num)):
            n = c["length"][p]
            assert np.array_equal(q[p, 0], c["way"][p, 0])
            assert np.abs(q[p, num[p] - 1] - c["way"][p, n - 1]).max() <= 1e-9
            assert (np.abs(qd[p, :num[p]]) <= c["v"] * (1 + 1e-9)).all()
            assert (np.abs(qdd[p, :num[p]]) <= c["a"] * (1 + 1e-9)).all()


def test_limits_and_fractions_of_the_task_layer(tmp_path):
    from gaussiangrasper_amd import arm as A
    from gaussiangrasper_amd import trajectory as T
    lim = T.default_limits()
    assert lim.v_max.tolist() == [2.175] * 4 + [2.61] * 3 and lim.a_max.tolist() == [15, 7.5, 10, 12.5, 15, 20, 20]
    half = lim.scaled(0.5, 0.25)
    assert np.array_equal(half.v_max, lim.v_max * 0.5) and np.array_equal(half.a_max, lim.a_max * 0.25)
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            lim.scaled(bad, 1.0)
    path = tmp_path / "limits.json"
    half.to_json(str(path))
    back = T.Limits.from_json(str(path))
    assert np.array_equal(back.v_max, half.v_max) and np.array_equal(back.a_max, half.a_max)
    path.write_text('{"v_max": [1, 2]}')
    with pytest.raises(ValueError, match="a_max"):
        T.Limits.from_json(str(path))
    with pytest.raises(ValueError):
        T.Limits([1.0, -1.0], [1.0, 1.0])
    # the limits do not live in the arm: its saved form is what it was
    arm = A.default_arm()
    arm.to_json(str(tmp_path / "arm.json"))
    import json
    assert sorted(json.loads((tmp_path / "arm.json").read_text())) == ["base", "fixed", "joints", "spheres"]
    # duplicates and NaN padding leave, as the report of `roadmap plan` pads its routes
    w = np.array([[0.0, 0], [0, 0], [1, 1], [1, 1], [2, 0], [np.nan, np.nan]])
    assert T.dedupe(w).tolist() == [[0, 0], [1, 1], [2, 0]]
    way, length = T.pack_routes([w, w[:1]], 2)
    assert way.shape == (2, 3, 2) and length.tolist() == [3, 1]
    assert T.grid_max(1, 16) == 0 and T.grid_max(2, 16) == 16 and T.grid_max(5, 3) == 21 == tr.grid_max(5, 3)
