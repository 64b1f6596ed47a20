"""Arm trajectories on the GPU: gg_traj_time and gg_traj_sample held to the numpy restatement (tests/trajectory_ref.py)
to the bit through the C entries, every array in a sentinel arena (tests/arena.py), on the constructed cases whose
claims tests/test_trajectory_host.py establishes; then the task layer of gaussiangrasper_amd/trajectory.py on the block
scene of tests/roadmap_ref.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import roadmap_ref as rr
import trajectory_cases as tc
import trajectory_ref as tr
from arena import Arena

gpu = pytest.mark.gpu
DEV = "cuda"
TIME_OUT = ("count", "xbar", "x", "u", "t", "q_grid", "duration", "infeasible", "status")


def _lib():
    from gaussiangrasper_amd import _lib as L
    return L.load()


def _host(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    return a, a.ctypes.data_as(C.c_void_p)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def same(got, want, what=""):
    """to the bit: the same operations in the same order, no contraction; NaN where the restatement has NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what
        bad = np.nonzero(got[~nan].view(np.uint64) != want[~nan].view(np.uint64))[0]
        assert len(bad) == 0, (what, len(bad), got[~nan][bad[:4]], want[~nan][bad[:4]])
    else:
        assert np.array_equal(got, want), what


def time_arena(c, seed=1, q_grid=True):
    P, W, J = c["way"].shape
    g = tr.grid_max(W, c["m"])
    ar = Arena(DEV, seed)
    ar.carve("way", c["way"], 8, "in").carve("length", c["length"], 4, "in").carve("blend", c["blend"], 8, "in")
    ar.carve("count", np.zeros(P, np.int32), 4, "out").carve("status", np.zeros(P, np.int32), 4, "out")
    for name in ("xbar", "x", "t"):
        ar.carve(name, np.zeros((P, g + 1)), 8, "out")
    ar.carve("u", np.zeros((P, g)), 8, "out")
    if q_grid:
        ar.carve("q_grid", np.zeros((P, g + 1, J)), 8, "out")
    ar.carve("duration", np.zeros(P), 8, "out").carve("infeasible", np.zeros(P), 8, "out")
    return ar


def time_call(ar, c, with_grid=True, **o):
    P, W, J = c["way"].shape
    keep = (_host(c["v"], np.float64), _host(c["a"], np.float64))
    a = dict(J=J, P=P, W=W, way=ar.ptr("way"), length=ar.ptr("length"), blend=ar.ptr("blend"), v=keep[0][1],
             a=keep[1][1], m=c["m"], count=ar.ptr("count"), xbar=ar.ptr("xbar"), x=ar.ptr("x"), u=ar.ptr("u"),
             t=ar.ptr("t"), q_grid=ar.ptr("q_grid") if with_grid else None, duration=ar.ptr("duration"),
             infeasible=ar.ptr("infeasible"), status=ar.ptr("status"))
    a.update(o)
    return _lib().gg_traj_time(a["J"], a["P"], a["W"], a["way"], a["length"], a["blend"], a["v"], a["a"], a["m"],
                               a["count"], a["xbar"], a["x"], a["u"], a["t"], a["q_grid"], a["duration"],
                               a["infeasible"], a["status"], _stream())


def run_time(c, q_grid=True, seed=1):
    ar = time_arena(c, seed, q_grid)
    assert time_call(ar, c, q_grid) == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    return ar.check()


def check_time(out, want, q_grid=True):
    for key in TIME_OUT:
        if key == "q_grid" and not q_grid:
            continue
        same(out[key], want[key], key)


def sample_call(c, law, dt, K, seed=2):
    """(q, qd, qdd, num) of gg_traj_sample fed `law`, a dict of arrays under time_law's names"""
    P, W, J = c["way"].shape
    ar = Arena(DEV, seed)
    ar.carve("way", c["way"], 8, "in").carve("length", c["length"], 4, "in").carve("blend", c["blend"], 8, "in")
    for name, dt_ in (("count", np.int32), ("x", np.float64), ("u", np.float64), ("t", np.float64),
                      ("duration", np.float64), ("status", np.int32)):
        ar.carve(name, np.ascontiguousarray(law[name], dt_), 8 if dt_ == np.float64 else 4, "in")
    for name in ("q", "qd", "qdd"):
        ar.carve(name, np.zeros((P, K, J)), 8, "out")
    ar.carve("num", np.zeros(P, np.int32), 4, "out")
    st = _lib().gg_traj_sample(J, P, W, ar.ptr("way"), ar.ptr("length"), ar.ptr("blend"), c["m"], ar.ptr("count"),
                               ar.ptr("x"), ar.ptr("u"), ar.ptr("t"), ar.ptr("duration"), ar.ptr("status"), float(dt), K,
                               ar.ptr("q"), ar.ptr("qd"), ar.ptr("qdd"), ar.ptr("num"), _stream())
    assert st == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    out = ar.check()
    return out["q"], out["qd"], out["qdd"], out["num"]


def check_sample(c, law, dt, K):
    got = sample_call(c, law, dt, K)
    want = tr.sample(c["way"], c["length"], c["blend"], c["m"], law, dt, K)
    for g, w, name in zip(got, want, ("q", "qd", "qdd", "num")):
        same(g, w, name)
    return got


# ------------------------------------------------------------------------------------------------
# the time law
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", sorted(tc.cases()))
def test_time_law_equals_the_restatement_to_the_bit(name):
    c, want = tc.cases()[name], tc.law(name)
    out = run_time(c)
    check_time(out, want)
    ok = out["status"] == tr.OK
    moving = ok & (out["count"] > 0)
    if moving.any():
        biggest = np.nanmax(np.abs(out["u"][moving]), axis=1)
        assert (out["infeasible"][moving] <= 1e-9 * biggest).all()


@gpu
def test_bad_paths_come_back_nan_and_their_neighbours_as_if_alone():
    c = tc.cases()["bad"]
    out = run_time(c)
    for p, st in tc.bad_rows().items():
        assert out["status"][p] == st and out["count"][p] == 0
        for key in ("xbar", "x", "u", "t", "q_grid"):
            assert np.isnan(out[key][p]).all(), key
        assert np.isnan(out["duration"][p]) and np.isnan(out["infeasible"][p])
    for p in range(len(c["length"])):
        if p in tc.bad_rows():
            continue
        alone = dict(c, way=c["way"][p:p + 1], length=c["length"][p:p + 1], blend=c["blend"][p:p + 1])
        one = run_time(alone, seed=7)
        for key in TIME_OUT:
            same(one[key][0], out[key][p], key)


@gpu
def test_null_q_grid_and_twice_the_same_bytes():
    for name in ("joints7", "fractions", "paths65"):
        c, want = tc.cases()[name], tc.law(name)
        out = run_time(c, q_grid=False)
        check_time(out, want, q_grid=False)
        full, again = run_time(c, seed=3), run_time(c, seed=4)
        for key in TIME_OUT:
            assert full[key].tobytes() == again[key].tobytes(), key
            if key != "q_grid":
                assert full[key].tobytes() == out[key].tobytes(), key


@gpu
def test_time_law_refuses_bad_arguments_before_any_launch():
    lib = _lib()
    c = tc.cases()["joints7"]
    ar = time_arena(c)
    J = c["way"].shape[2]

    def refused(status, *words):
        assert status == -1
        msg = lib.gg_last_error()
        for word in words:
            assert word in msg, (word, msg)

    def off_by(name, n):
        return C.c_void_p(ar.address(name) + n)
    refused(time_call(ar, c, m=1), b"steps")
    refused(time_call(ar, c, m=tr.MAX_STEPS + 1), b"steps")
    refused(time_call(ar, c, J=0), b"num_joints")
    refused(time_call(ar, c, J=9), b"num_joints")
    refused(time_call(ar, c, W=0), b"num_waypoints")
    refused(time_call(ar, c, W=tr.MAX_WAYPOINTS + 1), b"num_waypoints")
    refused(time_call(ar, c, P=-1), b"num_paths")
    refused(time_call(ar, c, P=1 << 26), b"num_paths")
    for bad in (0.0, -1.0, np.nan, np.inf):
        lim = np.full(J, 1.0)
        lim[J - 1] = bad
        keep, bp = _host(lim, np.float64)
        refused(time_call(ar, c, v=bp), b"v_max")
        refused(time_call(ar, c, a=bp), b"a_max")
    refused(time_call(ar, c, v=None), b"null pointer", b"v_max")
    for name in ("way", "length", "blend", "count", "xbar", "x", "u", "t", "duration", "infeasible", "status"):
        refused(time_call(ar, c, **{name: None}), b"null pointer", name.encode())
    for name in ("way", "blend", "xbar", "x", "u", "t", "q_grid", "duration", "infeasible"):
        refused(time_call(ar, c, **{name: off_by(name, 4)}), b"misaligned", name.encode())
    for name in ("length", "count", "status"):
        refused(time_call(ar, c, **{name: off_by(name, 2)}), b"misaligned", name.encode())
    assert time_call(ar, c, P=0) == 0
    torch.cuda.synchronize()
    assert ar.untouched()


# ------------------------------------------------------------------------------------------------
# the sampler
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("K", [1, 2, 64, 65])
def test_samples_equal_the_restatement_fed_its_law_and_fed_the_kernels(K):
    for name in ("joints1", "joints2", "joints7", "joints8", "fractions", "still", "reversal", "limits1e3", "bad",
                 "paths65", "steps64"):
        c, law = tc.cases()[name], tc.law(name)
        longest = float(np.nanmax(law["duration"]))
        for dt in (longest / 40.0, longest / 3.0, longest * 2.0):   # past K, within K, larger than every duration
            check_sample(c, law, dt, K)
        kernel = run_time(c, seed=9)
        got = check_sample(c, kernel, longest / 50.0, K)
        want = tr.sample(c["way"], c["length"], c["blend"], c["m"], law, longest / 50.0, K)
        for g, w, what in zip(got, want, ("q", "qd", "qdd", "num")):
            same(g, w, what)


@gpu
def test_samples_on_grid_times_past_the_end_and_with_one_waypoint():
    c, law = tc.cases()["pow2"], tc.law("pow2")
    q, qd, qdd, num = check_sample(c, law, 0.25, 8)                 # t = 0.5 and 1.0 are grid times
    assert num.tolist() == [5, 1] and q[0, :5, 0].tolist() == [0.0, 0.125, 0.5, 0.875, 1.0]
    assert qd[0, :5, 0].tolist() == [0.0, 1.0, 2.0, 1.0, 0.0] and np.isnan(q[0, 5:]).all() and q[1, 0, 0] == 3.0
    q, _, _, num = check_sample(c, law, 4.0, 2)                     # dt above the duration: the start and the end
    assert num.tolist() == [2, 1] and q[0, :, 0].tolist() == [0.0, 1.0]
    check_sample(c, law, 0.5, 1)
    check_sample(c, law, 1.0 / 1024, 65)
    for name in ("longest", "paths1025"):
        c, law = tc.cases()[name], tc.law(name)
        check_sample(c, law, float(np.nanmax(law["duration"])) / 60.0, 64)


@gpu
def test_sampler_refuses_bad_arguments_and_survives_a_foreign_count():
    lib = _lib()
    c, law = tc.cases()["joints7"], tc.law("joints7")
    P, W, J = c["way"].shape
    t = {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in
         dict(way=c["way"], length=c["length"], blend=c["blend"], count=law["count"], x=law["x"], u=law["u"], t=law["t"],
              duration=law["duration"], status=law["status"]).items()}
    K = 4
    q, qd, qdd = (torch.zeros(P, K, J, dtype=torch.float64, device=DEV) for _ in range(3))
    num = torch.zeros(P, dtype=torch.int32, device=DEV)

    def call(**o):
        a = dict(J=J, P=P, W=W, m=c["m"], dt=0.1, K=K, q=q.data_ptr(), num=num.data_ptr(), count=t["count"].data_ptr())
        a.update(o)
        return lib.gg_traj_sample(a["J"], a["P"], a["W"], t["way"].data_ptr(), t["length"].data_ptr(),
                                  t["blend"].data_ptr(), a["m"], a["count"], t["x"].data_ptr(), t["u"].data_ptr(),
                                  t["t"].data_ptr(), t["duration"].data_ptr(), t["status"].data_ptr(), a["dt"], a["K"],
                                  a["q"], qd.data_ptr(), qdd.data_ptr(), a["num"], _stream())
    for bad, word in ((dict(dt=0.0), b"dt"), (dict(dt=float("nan")), b"dt"), (dict(K=0), b"num_samples"),
                      (dict(m=1), b"steps"), (dict(q=None), b"null pointer"), (dict(num=None), b"null pointer"),
                      (dict(q=q.data_ptr() + 4), b"misaligned"), (dict(num=num.data_ptr() + 2), b"misaligned")):
        assert call(**bad) == -1 and word in lib.gg_last_error(), bad
    # a count that is not the path's own: NaN rows, no read outside the arrays
    wrong = torch.full((P,), tr.grid_max(W, c["m"]), dtype=torch.int32, device=DEV)
    assert call(count=wrong.data_ptr()) == 0
    torch.cuda.synchronize()
    assert call() == 0
    torch.cuda.synchronize()
    want = tr.sample(c["way"], c["length"], c["blend"], c["m"], law, 0.1, K)
    same(q.cpu().numpy(), want[0], "q")


# ------------------------------------------------------------------------------------------------
# the task layer, on the block scene of tests/roadmap_ref.py
# ------------------------------------------------------------------------------------------------
DELTA = 0.005


def _scene():
    from gaussiangrasper_amd import field
    f = field.DistanceField(*rr.BOX, voxel=rr.H, device=torch.device(DEV))
    (x0, x1), (y0, y1), (z0, z1) = rr.BLOCK
    f.mass[x0:x1, y0:y1, z0:z1] = field.VOTE_ONE
    f.update()
    return f


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV)


def _round_the_block(model, f):
    """the route from Q_LEFT to Q_RIGHT round the block, its edges proven with margin DELTA and self margin 2 DELTA"""
    from gaussiangrasper_amd import roadmap as R
    plan = R.plan(model, rr.Q_LEFT[None], rr.Q_RIGHT[None], f, num_nodes=200, k=8, margin=DELTA, self_margin=2 * DELTA)
    assert plan.routes[0][0] is not None and len(plan.routes[0][0]) >= 3
    return plan.routes[0][0]


@gpu
def test_proven_blends_keep_every_sample_clear():
    from gaussiangrasper_amd import arm as A, trajectory as T
    model, f = A.default_arm(), _scene()
    way = _round_the_block(model, f)
    lim = T.default_limits()
    tr_ = T.plan_trajectories(model, [way, way[::-1]], lim, f, delta=DELTA, dt=0.01)
    assert (tr_.status.cpu().numpy() == T.OK).all() and (tr_.fractions[:, 1:len(way) - 1] > 0).all()
    assert not tr_.verified.any()
    stops = T.plan_trajectories(model, [way, way[::-1]], lim, f, dt=0.01)
    assert (tr_.duration < stops.duration).all() and (stops.fractions == 0).all()
    num = tr_.num.cpu().numpy()
    c, fr, need = A._sphere_set(model, None, A.SPHERE_RADIUS, 0.0, f.h)
    for p in range(2):
        q = tr_.q[p, :num[p]].contiguous()
        assert q[0].cpu().numpy().tobytes() == (way if p == 0 else way[::-1])[0].tobytes()
        assert np.abs(q[-1].cpu().numpy() - (way if p == 0 else way[::-1])[-1]).max() <= 1e-9
        slack, _ = A.clear(model, f.dist2, f.grid, f.dims, q, _t(c).float().reshape(-1, 3),
                           torch.from_numpy(fr).to(DEV), torch.from_numpy(need).to(DEV))
        assert (slack >= 0).all()                                   # the unraised margin
        gap, _ = A.self_gap(model, q)
        assert (gap >= 2 * DELTA - 2 * DELTA).all()                 # self_margin less 2 delta
        assert (tr_.qd[p, :num[p]].abs().cpu().numpy() <= lim.v_max * (1 + 1e-9)).all()
        assert (tr_.qdd[p, :num[p]].abs().cpu().numpy() <= lim.a_max * (1 + 1e-9)).all()


@gpu
def test_large_blends_are_verified_and_fall_back_where_a_chord_is_not_clear():
    from gaussiangrasper_amd import arm as A, trajectory as T
    model, f = A.default_arm(), _scene()
    L, R_ = rr.Q_LEFT, rr.Q_RIGHT
    assert not bool(A.motion(model, _t([L]), _t([R_]), f).ok[0])   # straight through the block
    over = _round_the_block(model, f)
    assert len(over) == 3
    # a corner as tight about the block as a clear polyline allows: between the middle of the straight move and the
    # roadmap's via, the first V whose two moves are ok while the point the blend of 1/2 passes at its middle grid
    # point, c(1/2) = mid + 3/4 (V - mid), is not clear
    mid = 0.5 * (L + R_)
    lam = (np.arange(1, 33) / 32.0)[:, None]
    V, cut = mid + lam * (over[1] - mid), mid + (0.75 * lam) * (over[1] - mid)
    ends = np.broadcast_to(L, V.shape), np.broadcast_to(R_, V.shape)
    legs = (A.motion(model, _t(ends[0]), _t(V), f).ok & A.motion(model, _t(V), _t(ends[1]), f).ok).cpu().numpy()
    blocked = ~A.motion(model, _t(cut), _t(cut), f).ok.cpu().numpy()
    print("moves ok:", legs.astype(int), "cut blocked:", blocked.astype(int))
    assert (legs & blocked).any()
    tight = np.stack([L, V[np.nonzero(legs & blocked)[0][0]], R_])
    # a small zigzag about Q_LEFT, far from the block: every blend of 1/2 is clear
    free = L + 0.05 * np.array([[0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 1, 0, 0], [1, 0, 0, 0, 0, 1, 1],
                                [0, 0, 0, 0, 1, 0, 1]], np.float64)
    assert bool(A.motion(model, _t(free[:-1]), _t(free[1:]), f).ok.all())
    routes = [over, free, tight]
    with pytest.raises(ValueError, match="verify"):
        T.plan_trajectories(model, routes, T.default_limits(), f, blend=0.5)
    tr_ = T.plan_trajectories(model, routes, T.default_limits(), f, blend=0.5, verify=True, dt=0.01)
    inner = np.zeros_like(tr_.verified)
    for p, r in enumerate(routes):
        inner[p, 1:len(r) - 1] = True
    kept, fell = tr_.verified & inner, ~tr_.verified & inner
    print("blends kept:", int(kept.sum()), "fallen back:", int(fell.sum()))
    assert kept[1, 1:3].all() and not tr_.verified[2].any() and kept.sum() >= 2 and fell.sum() >= 1
    assert (tr_.fractions[kept] == 0.5).all() and (tr_.fractions[fell] == 0.0).all() and not tr_.verified[~inner].any()
    assert (tr_.status.cpu().numpy() == T.OK).all()
    # the fallen blend is a stop: the arm is at rest at the corner
    num = tr_.num.cpu().numpy()
    at_rest = tr_.qd[2, :num[2]].abs().amax(dim=1).cpu().numpy()
    assert at_rest[1:-1].min() <= 0.05 * at_rest.max()
    # with delta too, a blend that falls back keeps its proven fraction
    both = T.plan_trajectories(model, routes, T.default_limits(), f, blend=0.5, delta=DELTA, verify=True, dt=0.01)
    assert np.array_equal(both.verified, tr_.verified)
    proven = T.blend_fractions(model, tight, DELTA)
    assert proven[1] > 0 and np.array_equal(both.fractions[2, :3], proven)


@gpu
def test_time_plan_ranks_by_duration_not_by_metric_length():
    from gaussiangrasper_amd import arm as A, roadmap as R, trajectory as T
    model, f = A.default_arm(), _scene()
    base_turn, wrist_turn = rr.Q_LEFT.copy(), rr.Q_LEFT.copy()
    base_turn[0] -= 0.5                                             # long in the metric: the whole arm swings
    wrist_turn[6] += 1.0                                            # short in the metric: the last joint turns
    plan = R.plan(model, rr.Q_LEFT[None], np.stack([base_turn, wrist_turn]), f, num_nodes=200, k=8)
    assert plan.hops.tolist() == [[1, 1]] and plan.length[0, 1] < plan.length[0, 0]
    before = (plan.length.copy(), plan.cost.copy(), [r.copy() for r in plan.routes[0]])
    lim = T.default_limits()
    slow_wrist = T.Limits(lim.v_max * np.array([1, 1, 1, 1, 1, 1, 0.02]), lim.a_max)
    timed = T.time_plan(plan, slow_wrist)
    assert timed.duration.shape == (1, 2) and timed.duration[0, 0] < timed.duration[0, 1] and timed.best.tolist() == [0]
    assert timed.duration[0, 1] >= 1.0 / slow_wrist.v_max[6]
    fair = T.time_plan(plan, lim)
    assert np.isfinite(fair.duration).all()
    assert np.array_equal(plan.length, before[0]) and np.array_equal(plan.cost, before[1])
    assert all(np.array_equal(a, b) for a, b in zip(plan.routes[0], before[2]))


@gpu
def test_time_reach_times_every_seed_that_follows_its_path():
    from gaussiangrasper_amd import arm as A, trajectory as T
    model = A.default_arm()
    q = np.stack([rr.Q_LEFT, rr.Q_LEFT + 0.1, rr.Q_LEFT + 0.2])
    poses = A.fk(model, _t(q))[:, -1].float().cpu().numpy()[None]   # (1, 3, 12)
    res = A.reach(model, poses, num_seeds=4)
    seed_before = res.seed.clone()
    timed = T.time_reach(res, T.default_limits(), model)
    whole = (res.follow.first_fail == 3).cpu().numpy()
    assert timed.duration.shape == (1, 4) and np.array_equal(np.isfinite(timed.duration), whole)
    assert whole.any() and timed.best[0] == np.argmin(timed.duration[0]) and torch.equal(res.seed, seed_before)


@gpu
def test_command_lines(tmp_path, capsys):
    from gaussiangrasper_amd import roadmap as R, trajectory as T
    f = _scene()
    f.save(str(tmp_path / "field.npz"))
    np.save(tmp_path / "from.npy", rr.Q_LEFT)
    np.save(tmp_path / "to.npy", np.stack([rr.Q_RIGHT]))
    way = str(tmp_path / "way.npz")
    base = ["plan", "--arm", "default", "--field", str(tmp_path / "field.npz"), "--from", str(tmp_path / "from.npy"),
            "--to", str(tmp_path / "to.npy"), "--nodes", "150", "--k", "8", "--out", way]
    assert R.main(base) == 0
    with np.load(way) as z:
        assert set(z.files) == {"cost", "length", "hops", "waypoints"}      # without the flag: the report as it was
        plain = {k: z[k].copy() for k in z.files}
    assert R.main(base + ["--time-limits", "default"]) == 0
    with np.load(way) as z:
        assert set(z.files) == {"cost", "length", "hops", "waypoints", "duration"}
        for k, v in plain.items():
            assert np.array_equal(z[k], v, equal_nan=True)
        assert z["duration"].shape == (1, 1) and 0.0 < z["duration"][0, 0] < 60.0
        duration = float(z["duration"][0, 0])
    capsys.readouterr()
    out = str(tmp_path / "traj.npz")
    assert T.main(["--arm", "default", "--waypoints", way, "--limits", "default", "--dt", "0.01", "--steps", "16",
                   "--out", out]) == 0
    assert "1 of 1 routes timed" in capsys.readouterr().out
    with np.load(out) as z:
        assert set(z.files) == {"t", "q", "qd", "qdd", "num", "duration", "fractions", "verified", "status"}
        assert z["duration"][0] == duration and z["num"][0] == int(np.ceil(duration / 0.01)) + 1
        assert np.array_equal(z["q"][0, 0], rr.Q_LEFT) and np.abs(z["q"][0, z["num"][0] - 1] - rr.Q_RIGHT).max() <= 1e-9
    T.default_limits().scaled(0.5, 0.5).to_json(str(tmp_path / "limits.json"))
    assert T.main(["--arm", "default", "--waypoints", way, "--limits", str(tmp_path / "limits.json"), "--delta", "0.005",
                   "--vel-scale", "0.5", "--out", out]) == 0
    with np.load(out) as z:
        assert z["duration"][0] > duration and (z["fractions"][0, 1:int(plain["hops"][0, 0])] > 0).all()
