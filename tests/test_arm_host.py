"""No-GPU checks of arm reachability: the restatement (tests/arm_ref.py) against independent forms, the claims of the
fixtures the GPU tests rest on, the selection rule, the Arm record and its JSON, the host helpers of
gaussiangrasper_amd.arm and the three C entries' argument validation (nothing is launched)."""
import ctypes
import json
import threading

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import arm_ref as ref

LAW = ref.LAW


def _chains():
    return {"default": ref.default_chain(), "prismatic": ref.random_chain(5, 3, prismatic=(1, 3)),
            "one": ref.random_chain(1, 4), "eight": ref.random_chain(8, 5, prismatic=(6,))}


# ------------------------------------------------------------------------------------------------
# the restatement against independent forms
# ------------------------------------------------------------------------------------------------
def _fk_matrices(arm, J, q):
    """frames (J + 2, 4, 4) of one configuration as products of homogeneous matrices, the rotations from scipy"""
    base, fixed, axis, _, _, kind = ref.unpack(arm, J)
    T = ref.matrix(base)
    out = [T]
    for j in range(J):
        M = np.eye(4)
        if kind[j] == 0.0:
            M[:3, :3] = Rotation.from_rotvec(axis[j] * q[j]).as_matrix()
        else:
            M[:3, 3] = axis[j] * q[j]
        T = T @ ref.matrix(fixed[j]) @ M
        out.append(T)
    out.append(T @ ref.matrix(fixed[J]))
    return np.stack(out)


@pytest.mark.parametrize("name", ["default", "prismatic", "one", "eight"])
def test_fk_equals_homogeneous_matrix_products(name):
    arm, J = _chains()[name]
    q = ref.in_limits(arm, J, 33, np.random.default_rng(J), inset=0.0)
    got = ref.fk(arm, J, q)
    worst = 0.0
    for i in range(len(q)):
        want = _fk_matrices(arm, J, q[i])
        for f in range(J + 2):
            worst = max(worst, np.abs(ref.matrix(got[i, f]) - want[f]).max())
    assert worst <= 1e-13, worst
    # a row that is not finite is NaN, whole; the others are untouched by it
    q[7, J - 1] = np.inf
    again = ref.fk(arm, J, q)
    assert np.isnan(again[7]).all() and np.array_equal(np.delete(again, 7, 0), np.delete(got, 7, 0))


def test_default_arm_geometry():
    """what the recalled table implies, by hand: at q = 0 with joint 4 at -pi/2 and joint 6 at +pi/2 the gripper
    points straight down: the forearm lies level, a_4 + d_5 + a_7 out along x, and the elbow's second offset (a_5, across
    the forearm) adds to the height d_1 + d_3 from which the flange and the hand hang"""
    arm, J = ref.default_chain()
    q = np.zeros((1, 7))
    q[0, 3], q[0, 5] = -np.pi / 2, np.pi / 2
    T = ref.fk(arm, J, q)[0, J + 1]
    R, t = T[:9].reshape(3, 3), T[9:]
    assert np.allclose(R[:, 0], [0, 0, -1], atol=1e-12)                 # the approach axis
    assert np.allclose(t, [0.0825 + 0.384 + 0.088, 0.0, 0.333 + 0.316 + 0.0825 - 0.107 - 0.1034], atol=1e-12), t
    assert abs(np.linalg.det(R) - 1.0) <= 1e-12
    fixed = ref.unpack(arm, J)[1]
    assert {0.0825, 0.088} <= set(np.abs(fixed[:, 9]).round(6))         # the a column


@pytest.mark.parametrize("name", ["default", "prismatic", "one", "eight"])
def test_jacobian_equals_central_differences(name):
    arm, J = _chains()[name]
    q = ref.in_limits(arm, J, 9, np.random.default_rng(10 + J), inset=0.1)
    jac = ref.jacobian(arm, J, q, L=1.0)
    eps = 1e-6
    T0 = ref.fk(arm, J, q)[:, J + 1]
    for j in range(J):
        d = np.zeros(J)
        d[j] = eps
        Tp, Tm = ref.fk(arm, J, q + d)[:, J + 1], ref.fk(arm, J, q - d)[:, J + 1]
        lin = (Tp[:, 9:] - Tm[:, 9:]) / (2 * eps)
        # the angular velocity: skew part of dR R^T
        dR = ((Tp[:, :9] - Tm[:, :9]) / (2 * eps)).reshape(-1, 3, 3)
        W = dR @ np.swapaxes(T0[:, :9].reshape(-1, 3, 3), 1, 2)
        ang = np.stack([W[:, 2, 1] - W[:, 1, 2], W[:, 0, 2] - W[:, 2, 0], W[:, 1, 0] - W[:, 0, 1]], 1) / 2
        assert np.abs(jac[:, :3, j] - lin).max() <= 1e-7, (name, j)
        assert np.abs(jac[:, 3:, j] - ang).max() <= 1e-7, (name, j)


def test_rotation_vector_equals_scipy():
    rng = np.random.default_rng(5)
    axes = rng.normal(size=(400, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    axes[:3], axes[3:6] = np.eye(3), -np.eye(3)
    angles = np.concatenate([[0.0, 1e-9, 1e-9, 1e-7, 1e-4, np.pi - 1e-6, np.pi - 1e-6, np.pi / 2, 3.0, 2.5],
                             rng.uniform(0, np.pi - 1e-6, 390)])
    angles[:6] = [1e-9, np.pi - 1e-6, 1e-9, np.pi - 1e-6, 1e-9, np.pi - 1e-6]          # and about the coordinate axes
    rv = axes * angles[:, None]
    R = Rotation.from_rotvec(rv).as_matrix()
    got = ref.rotvec(R.reshape(-1, 9))
    want = Rotation.from_matrix(R).as_rotvec()
    assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()
    assert np.abs(got - rv).max() <= 1e-9           # and the angle that went in (pi - 1e-6 loses digits in R itself)
    assert np.array_equal(ref.rotvec(np.eye(3).reshape(1, 9)), np.zeros((1, 3)))


def test_step_law_against_numpy_linear_algebra():
    """one update of the restatement equals J^T (J J^T + lambda2 I)^-1 e by numpy's solver"""
    arm, J = ref.default_chain()
    rng = np.random.default_rng(8)
    q = ref.in_limits(arm, J, 12, rng)
    target = ref.fk(arm, J, q + rng.uniform(-0.02, 0.02, q.shape))[:, J + 1]
    out = ref.follow(arm, J, target.astype(np.float32)[:, None], q[:, None], **{**LAW, "max_iter": 1})
    # max_iter 1 lets one update happen; redo it here
    tgt = target.astype(np.float32).astype(np.float64)
    _, _, e_p, e_r = ref.pose_error(arm, J, q, tgt)
    jac = ref.jacobian(arm, J, q, LAW["L"])
    lo, hi = ref.unpack(arm, J)[3:5]
    for i in range(len(q)):
        e = np.concatenate([e_p[i], LAW["L"] * e_r[i]])
        lam2 = LAW["k"] * (e @ e) + LAW["lambda_min"] ** 2
        dq = jac[i].T @ np.linalg.solve(jac[i] @ jac[i].T + lam2 * np.eye(6), e)
        if np.abs(dq).max() > LAW["max_step"]:
            dq *= LAW["max_step"] / np.abs(dq).max()
        want = np.clip(q[i] + dq, lo, hi)
        if out[1][i, 0, 0] == 1:                    # converged after the one update: q_out is the updated q
            assert np.abs(out[0][i, 0, 0] - want).max() <= 1e-9
    assert (out[1][:, 0, 0] == 1).sum() >= 6


# ------------------------------------------------------------------------------------------------
# the fixtures' claims
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cut", "default"])
def test_near_fixture_converges_away_from_the_tolerances(which):
    f = ref.near_fixture(which)
    arm, J = f["arm"], f["J"]
    assert f["truth"].shape == (65, J) and f["J"] == (6 if which == "cut" else 7)
    lo, hi = ref.unpack(arm, J)[3:5]
    assert ((f["truth"] >= lo) & (f["truth"] <= hi)).all()
    sig = np.linalg.svd(ref.jacobian(arm, J, f["truth"], LAW["L"]), compute_uv=False)[:, -1]
    assert sig.min() >= ref.NEAR_SIGMA
    assert np.abs(f["seeds"][:, 0] - f["truth"]).max() <= 0.2
    q, iters, resid, first = f["out"]
    assert (first == 1).all() and (iters >= 0).all() and iters.max() <= 8, iters.max()
    assert ref.near_tolerance(f["decisions"], LAW["tol_p"], LAW["tol_r"]) == 0
    assert sum(len(d[0]) for d in f["decisions"]) == int((iters + 1).sum())
    if which == "cut":          # isolated solutions: it comes back to the one the seed was drawn about
        assert np.abs(q[:, 0, 0] - f["truth"]).max() <= 2 * (LAW["tol_p"] + LAW["L"] * LAW["tol_r"]) / ref.NEAR_SIGMA


def test_random_seed_fixture_targets_are_reached_by_four_seeds():
    f = ref.random_seed_fixture()
    assert f["poses"].shape == (16, 1, 12) and f["seeds"].shape == (16, 16, 7)
    it = f["out"][1][:, :, 0]
    assert (((it >= 0) & (it <= LAW["max_iter"] // 2)).sum(1) >= 4).all()
    assert np.array_equal(f["seeds"][:, 0], np.broadcast_to(f["seeds"][0, 0], (16, 7)))     # seed 0 is home


def test_unreachable_fixture_is_out_of_range():
    f = ref.unreachable_fixture()
    arm, J = f["arm"], f["J"]
    assert (np.linalg.norm(f["poses"][:, 0, 9:], axis=1) > f["span"] + 0.1).all()
    # no configuration gets there: the gripper never leaves the ball of the summed link lengths
    q = ref.in_limits(arm, J, 2000, np.random.default_rng(1), inset=0.0)
    assert np.linalg.norm(ref.fk(arm, J, q)[:, J + 1, 9:], axis=1).max() <= f["span"]
    q_out, iters, resid, first = ref.follow(arm, J, f["poses"], f["seeds"], **LAW)
    assert (first == 0).all() and (iters == -1).all() and np.isnan(q_out).all() and np.isnan(resid).all()


def test_field_fixture_keeps_off_the_cell_faces():
    f = ref.field_fixture()
    assert tuple(f["dims"]) == (40, 36, 44) and np.log2(f["grid"][3]) == round(np.log2(f["grid"][3]))
    assert f["q"].shape == (257, 7) and (f["dist2"] == 0).sum() > 100
    assert f["face"] == 0
    assert f["keep32"].sum() >= 250
    slack, worst = ref.clear(f["arm"], f["J"], f["dims"], f["grid"], f["dist2"], f["q"], f["spheres"], f["frame"],
                             f["need"], ref.FAR)
    assert (slack < 0).sum() >= 40 and (slack >= 0).sum() >= 40 and len(np.unique(worst)) >= 8
    # the restatement's clear by brute force on a few rows
    cen = ref.sphere_centres(f["arm"], f["J"], f["q"][:5], f["spheres"].astype(np.float64), f["frame"])
    for m in range(5):
        cell = np.floor((cen[m] - f["grid"][:3]) / f["grid"][3]).astype(int)
        vals = []
        for s, c in enumerate(cell):
            inside = ((c >= 0) & (c < f["dims"])).all()
            vals.append((f["dist2"][tuple(c)] if inside else ref.FAR) - f["need"][s])
        assert slack[m] == min(vals) and worst[m] == int(np.argmin(vals))


# ------------------------------------------------------------------------------------------------
# the selection rule
# ------------------------------------------------------------------------------------------------
def test_selection_rule_on_a_hand_made_table():
    from gaussiangrasper_amd.arm import select
    W = 3
    first = [[3, 3, 3, 1],       # three follow; the middle one is not clear; of the others the smaller jump wins
             [3, 3, 3, 3],       # a tie of the smallest jump: the lower index
             [0, 2, 1, 0],       # none follows
             [3, 3, 0, 3],       # all that follow hit something: reachable, not clear, the smallest jump still
             [2, 3, 2, 2],       # only one follows, with the largest jump
             [3, 3, 3, 3]]       # the smallest jump belongs to a seed that is not clear
    clear = [[1, 0, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1], [0, 0, 1, 0], [1, 1, 1, 1], [0, 1, 1, 1]]
    jump = [[0.5, 0.1, 0.4, 0.0], [0.7, 0.2, 0.2, 0.9], [np.nan] * 4, [0.9, 0.3, np.nan, 0.3], [np.nan, 2.5, np.nan, np.nan],
            [0.1, 0.6, 0.5, 0.5]]
    seed, reachable, ok = select(first, W, np.array(clear, bool), jump)
    assert seed.tolist() == [2, 1, -1, 1, 1, 2]
    assert reachable.tolist() == [True, True, False, True, True, True]
    assert ok.tolist() == [True, True, False, False, True, True]
    none = select(np.zeros((2, 0), np.int32), W, np.zeros((2, 0), bool), np.zeros((2, 0)))
    assert none[0].tolist() == [-1, -1] and not none[1].any() and not none[2].any()


# ------------------------------------------------------------------------------------------------
# the Arm record
# ------------------------------------------------------------------------------------------------
def test_arm_json_round_trip_and_helpers(tmp_path):
    from gaussiangrasper_amd import arm as A
    a = A.default_arm()
    arr = a.to_array()
    assert arr.shape == (A.arm_doubles(7),) == (150,) and arr.dtype == np.float64
    path = str(tmp_path / "arm.json")
    a.to_json(path)
    b = A.Arm.from_json(path)
    assert np.array_equal(b.to_array(), arr) and np.array_equal(b.spheres, a.spheres)
    text = json.load(open(path))
    assert sorted(text) == ["base", "fixed", "joints", "spheres"] and len(text["joints"]) == 7
    c, f, r = a.link_spheres()
    assert c.dtype == np.float32 and f.dtype == np.int32 and len(c) == len(f) == len(r) >= 14
    assert f.min() == 0 and f.max() <= 8 and all((f == k).sum() >= 2 for k in range(8)) and (r > 0).all()
    # with_base: a copy, the base given as 12 numbers, (3, 4) or (4, 4)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rotation.from_euler("z", 0.3).as_matrix(), [0.1, -0.2, 0.05]
    moved = a.with_base(T)
    assert np.array_equal(moved.to_array()[:12], ref.twelve(T)) and np.array_equal(a.to_array(), arr)
    assert np.array_equal(a.with_base(T[:3]).base, moved.base) and np.array_equal(a.with_base(ref.twelve(T)).base, moved.base)
    got = ref.fk(moved.to_array(), 7, a.home()[None])[0, 8]
    want = T @ ref.matrix(ref.fk(arr, 7, a.home()[None])[0, 8])
    assert np.abs(ref.matrix(got) - want).max() <= 1e-13
    # seeds: home first, the others inside the limits, the same from the same seed
    s = A.seeds(a, 5, 9, seed=3)
    assert s.shape == (5, 9, 7) and np.array_equal(s[:, 0], np.broadcast_to(a.home(), (5, 7)))
    assert ((s >= a.lo) & (s <= a.hi)).all() and np.array_equal(s, A.seeds(a, 5, 9, seed=3))
    assert not np.array_equal(s[:, 1:], A.seeds(a, 5, 9, seed=4)[:, 1:])
    assert np.array_equal(A.seeds(a, 2, 3, home=a.lo)[:, 0], np.broadcast_to(a.lo, (2, 7)))
    with pytest.raises(ValueError):
        A.seeds(a, 2, 0)


def _broken(a, what):
    from dataclasses import replace
    fixed, axis = a.fixed.copy(), a.axis.copy()
    lo, hi, kind, base = a.lo.copy(), a.hi.copy(), a.kind.copy(), a.base.copy()
    if what == "nan base":
        base[10] = np.nan
    elif what == "inf fixed":
        fixed[3, 11] = np.inf
    elif what == "skew base":
        base[0] += 1e-8
    elif what == "skew fixed":
        fixed[7, 4] += 1e-8
    elif what == "long axis":
        axis[2, 2] += 1e-8
    elif what == "nan axis":
        axis[5, 0] = np.nan
    elif what == "lo > hi":
        lo[4], hi[4] = 1.0, 0.5
    elif what == "inf limit":
        hi[1] = np.inf
    elif what == "kind":
        kind[6] = 2.0
    return replace(a, base=base, fixed=fixed, axis=axis, lo=lo, hi=hi, kind=kind)


MALFORMED = [("nan base", "base"), ("inf fixed", "fixed[3]"), ("skew base", "base"), ("skew fixed", "fixed[7]"),
             ("long axis", "axis[2]"), ("nan axis", "axis[5]"), ("lo > hi", "lo[4]"), ("inf limit", "hi[1]"),
             ("kind", "kind[6]")]


@pytest.mark.parametrize("what,names", MALFORMED)
def test_malformed_arms_are_refused_by_to_array(what, names, tmp_path):
    from gaussiangrasper_amd import arm as A
    bad = _broken(A.default_arm(), what)
    with pytest.raises(ValueError) as e:
        bad.to_array()
    assert names in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        bad.to_json(str(tmp_path / "bad.json"))


def test_arm_shapes_and_files_are_refused(tmp_path):
    from dataclasses import replace
    from gaussiangrasper_amd import arm as A
    a = A.default_arm()
    for bad, names in ((replace(a, fixed=a.fixed[:7]), "fixed"), (replace(a, lo=a.lo[:6]), "lo"),
                       (replace(a, base=a.base[:9]), "base"), (replace(a, axis=np.zeros((9, 3))), "axis"),
                       (replace(a, axis=np.zeros((0, 3))), "axis")):
        with pytest.raises(ValueError) as e:
            bad.to_array()
        assert names in str(e.value)
    with pytest.raises(ValueError) as e:
        replace(a, spheres=np.array([[9, 0, 0, 0, 0.1]])).link_spheres()
    assert "frame" in str(e.value)
    for name, text in (("a.json", "{ not json"), ("b.json", "[1, 2]"), ("c.json", '{"base": [1]}'),
                       ("d.json", json.dumps({"base": a.base.tolist(), "fixed": a.fixed.tolist(),
                                              "joints": [[0, 0, 2, -1, 1, 0]] * 7}))):
        p = tmp_path / name
        p.write_text(text)
        with pytest.raises(ValueError) as e:
            A.Arm.from_json(str(p))
        assert name in str(e.value)
    with pytest.raises(OSError):
        A.Arm.from_json(str(tmp_path / "missing.json"))


def test_wrappers_have_no_cpu_path():
    import torch
    from gaussiangrasper_amd import arm as A
    a = A.default_arm()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.fk(a, torch.zeros(2, 7, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.follow(a, torch.zeros(1, 1, 12), torch.zeros(1, 1, 7, dtype=torch.float64))
    z = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.clear(a, torch.zeros(2, 2, 2, dtype=torch.int32), [0, 0, 0, 1.0], [2, 2, 2],
                torch.zeros(1, 7, dtype=torch.float64), torch.zeros(1, 3), z, z)


# ------------------------------------------------------------------------------------------------
# the C entries' argument validation (before any launch: no GPU needed)
# ------------------------------------------------------------------------------------------------
def _call_on_thread(fn, cases):
    """gg_last_error is per thread: run the calls on one fresh thread and return (status, message) of each"""
    out = []

    def run():
        for c in cases:
            out.append(fn(c))
    t = threading.Thread(target=run)
    t.start()
    t.join()
    return out


def _host(a):
    a = np.ascontiguousarray(a, np.float64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_c_entries_refuse_bad_arguments_before_any_launch():
    from gaussiangrasper_amd import _lib
    from gaussiangrasper_amd import arm as A
    lib = _lib.load()
    model = A.default_arm()
    keep = []

    def arm_ptr(arr):
        a, p = _host(arr)
        keep.append(a)
        return p
    good = arm_ptr(model.to_array())
    n, f = ctypes.c_void_p(0), ctypes.c_void_p(1 << 20)
    odd4, odd2 = ctypes.c_void_p((1 << 20) + 4), ctypes.c_void_p((1 << 20) + 2)
    D = ctypes.c_double
    law = [D(1e-4), D(1e-3), D(0.1), D(1.0), D(1e-4), D(0.2), 100]

    def fk(J=7, arm=good, M=3, q=f, frames=f):
        return (J, arm, M, q, frames, n)
    bad_arms = []
    for what, _ in MALFORMED:
        b = _broken(model, what)
        joints = np.concatenate([b.axis, b.lo[:, None], b.hi[:, None], b.kind[:, None]], 1)
        bad_arms.append(arm_ptr(np.concatenate([b.base, b.fixed.reshape(-1), joints.reshape(-1)])))
    wants = [b"not finite", b"not finite", b"base", b"fixed[7]", b"axis[2]", b"not finite", b"joint 4: lo > hi",
             b"not finite", b"kind[6]"]
    cases = [(fk(arm=p), w) for p, w in zip(bad_arms, wants)]
    cases += [(fk(J=0), b"num_joints"), (fk(J=9), b"num_joints"), (fk(arm=n), b"null pointer: arm"),
              (fk(M=-1), b"num_rows"), (fk(M=(1 << 26) + 1), b"num_rows"), (fk(q=n), b"null pointer"),
              (fk(frames=n), b"null pointer"), (fk(q=odd4), b"misaligned"), (fk(frames=odd4), b"misaligned")]
    got = _call_on_thread(lambda a: (lib.gg_arm_fk(*a), lib.gg_last_error()), [c[0] for c in cases])
    for (st, msg), (_, want) in zip(got, cases):
        assert st == -1 and msg.startswith(b"gg_arm_fk") and want in msg, (msg, want)
    assert lib.gg_arm_fk(*fk(M=0, q=n, frames=n)) == 0

    def follow(J=7, arm=good, P=2, W=3, poses=f, S=4, seeds=f, law=law, outs=(f, f, f, f)):
        return (J, arm, P, W, poses, S, seeds, *law, *outs, n)

    def with_law(i, v):
        out = list(law)
        out[i] = D(v) if i < 6 else v
        return out
    cases = [(follow(arm=bad_arms[2]), b"base"), (follow(P=-1), b"num_paths"),
             (follow(P=1 << 14, S=1 << 13), b"GG_FIELD_MAX_POSES"), (follow(P=1 << 10, S=1 << 10, W=1 << 7), b"GG_FIELD_MAX_POSES"),
             (follow(law=with_law(0, -1.0)), b"tol_p"), (follow(law=with_law(1, float("nan"))), b"tol_r"),
             (follow(law=with_law(2, 0.0)), b"rot_length"), (follow(law=with_law(3, -0.5)), b"gain"),
             (follow(law=with_law(4, 0.0)), b"lambda_min"), (follow(law=with_law(5, float("inf"))), b"max_step"),
             (follow(law=with_law(6, 1025)), b"max_iter"), (follow(law=with_law(6, -1)), b"max_iter"),
             (follow(poses=n), b"null pointer"), (follow(seeds=n), b"null pointer"),
             (follow(outs=(n, f, f, f)), b"null pointer"), (follow(outs=(f, f, f, n)), b"null pointer"),
             (follow(seeds=odd4), b"misaligned"), (follow(outs=(odd4, f, f, f)), b"misaligned"),
             (follow(outs=(f, f, odd4, f)), b"misaligned"), (follow(poses=odd2), b"misaligned"),
             (follow(outs=(f, odd2, f, f)), b"misaligned")]
    got = _call_on_thread(lambda a: (lib.gg_arm_follow(*a), lib.gg_last_error()), [c[0] for c in cases])
    for (st, msg), (_, want) in zip(got, cases):
        assert st == -1 and msg.startswith(b"gg_arm_follow") and want in msg, (msg, want)
    assert lib.gg_arm_follow(*follow(P=0, poses=n, seeds=n, outs=(n,) * 4)) == 0
    assert lib.gg_arm_follow(*follow(S=0, poses=n, seeds=n, outs=(n,) * 4)) == 0

    dims, grid = (ctypes.c_int32 * 3)(8, 8, 8), (D * 4)(0, 0, 0, 0.1)

    def p(a):
        return ctypes.cast(a, ctypes.c_void_p)

    def clear(J=7, arm=good, dims=p(dims), grid=p(grid), dist2=f, M=3, q=f, S=5, spheres=f, frame=f, need=f,
              outside=ref.FAR, outs=(f, f)):
        return (J, arm, dims, grid, dist2, M, q, S, spheres, frame, need, outside, *outs, n)
    cases = [(clear(arm=bad_arms[4]), b"axis[2]"), (clear(dims=p((ctypes.c_int32 * 3)(8, 0, 8))), b"dims"),
             (clear(dims=p((ctypes.c_int32 * 3)(1024, 1024, 129))), b"GG_FIELD_MAX_CELLS"), (clear(dims=n), b"dims"),
             (clear(grid=n), b"grid"), (clear(grid=p((D * 4)(0, 0, 0, 0.0))), b"h finite and > 0"),
             (clear(M=-1), b"num_rows"), (clear(S=1025), b"num_spheres"), (clear(S=-1), b"num_spheres"),
             (clear(outside=-1), b"outside"), (clear(outside=ref.FAR + 1), b"outside"),
             (clear(dist2=n), b"null pointer"), (clear(q=n), b"null pointer"), (clear(outs=(n, f)), b"null pointer"),
             (clear(outs=(f, n)), b"null pointer"), (clear(spheres=n), b"null pointer"),
             (clear(frame=n), b"null pointer"), (clear(need=n), b"null pointer"), (clear(q=odd4), b"misaligned"),
             (clear(frame=odd2), b"misaligned"), (clear(outs=(f, odd2)), b"misaligned")]
    got = _call_on_thread(lambda a: (lib.gg_arm_clear(*a), lib.gg_last_error()), [c[0] for c in cases])
    for (st, msg), (_, want) in zip(got, cases):
        assert st == -1 and msg.startswith(b"gg_arm_clear") and want in msg, (msg, want)
    assert lib.gg_arm_clear(*clear(M=0, dist2=n, q=n, spheres=n, frame=n, need=n, outs=(n, n))) == 0


def test_command_line_errors(tmp_path):
    from gaussiangrasper_amd import arm as A
    bad = tmp_path / "bad_arm.json"
    bad.write_text('{"base": [1, 0, 0]}')
    poses = tmp_path / "poses.npy"
    np.save(poses, np.zeros((2, 3, 12), np.float32))
    with pytest.raises(SystemExit) as e:
        A.main(["--arm", str(bad), "--poses", str(poses), "--out", str(tmp_path / "q.npy"),
                "--report", str(tmp_path / "r.npz")])
    assert str(e.value).startswith("error: ") and "bad_arm.json" in str(e.value)
    with pytest.raises(SystemExit) as e:
        A.main(["--arm", "default", "--poses", str(tmp_path / "nothing.npy"), "--out", str(tmp_path / "q.npy"),
                "--report", str(tmp_path / "r.npz")])
    assert str(e.value).startswith("error: ")
    np.save(tmp_path / "flat.npy", np.zeros((4, 12), np.float32))
    with pytest.raises(SystemExit) as e:
        A.main(["--arm", "default", "--poses", str(tmp_path / "flat.npy"), "--out", str(tmp_path / "q.npy"),
                "--report", str(tmp_path / "r.npz")])
    assert str(e.value).startswith("error: ") and "(P, W, 12)" in str(e.value)
    for argv in (["--arm", "default", "--out", "q", "--report", "r"],
                 ["--arm", "default", "--poses", "p", "--grasps", "g", "--out", "q", "--report", "r"],
                 ["--arm", "default", "--grasps", "g", "--out", "q", "--report", "r"],
                 ["--arm", "default", "--poses", "p", "--steps", "3", "--out", "q", "--report", "r"]):
        with pytest.raises(SystemExit) as e:
            A.main(argv)
        assert e.value.code == 2
