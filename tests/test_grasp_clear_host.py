"""No-GPU checks of gripper clearance (gaussiangrasper_amd.grasp.clearance, gg_grasp_clearance): the fp64 restatement
(tests/grasp_clear_ref.py) against an independent world-frame formulation, the default gripper model against hand
computation, the C entry's argument validation and workspace query, the command-line tools' argument errors, and
that grasp_object without a gripper makes no clearance call."""
import ctypes
import json
import math
import threading

import numpy as np
import pytest
import torch

from grasp_clear_ref import part_bounds, restate, row_valid, slab_gripper
from grasp_ref import grasp_rows, rotation

D = ctypes.c_double


# ------------------------------------------------------------------------------------------------
# the restatement against half-spaces of the world frame
# ------------------------------------------------------------------------------------------------
def _world_planes(points, grasps, parts, approach):
    """Counts per (grasp, part) from the six face planes of every part mapped into the world frame: with n_j the
    j-th column of R, u_j >= lo is n_j . p >= n_j . t + lo.  Also the smallest distance of any point to any face
    plane (body faces and the sweep's far face)."""
    p = np.asarray(points, np.float64)
    G = np.asarray(grasps, np.float64)
    B = part_bounds(parts, grasps)
    m, P = B.shape[:2]
    body, sweep, closest = np.zeros((m, P), np.int64), np.zeros((m, P), np.int64), math.inf
    for g in range(m):
        R, t = G[g, 4:13].reshape(3, 3), G[g, 13:16]
        s = [p @ R[:, j] for j in range(3)]              # n_j . p
        o = [R[:, j] @ t for j in range(3)]              # n_j . t
        for k in range(P):
            b = B[g, k]
            inside = []
            for j in range(3):
                lo, hi = s[j] - (o[j] + b[2 * j]), (o[j] + b[2 * j + 1]) - s[j]
                closest = min(closest, np.abs(lo).min(), np.abs(hi).min())
                inside.append((lo >= 0) & (hi >= 0))
            far = s[0] - (o[0] + (b[0] - approach))
            closest = min(closest, np.abs(far).min())
            body[g, k] = (inside[0] & inside[1] & inside[2]).sum()
            sweep[g, k] = ((far >= 0) & (s[0] - (o[0] + b[0]) < 0) & inside[1] & inside[2]).sum()
    return body, sweep, closest


def test_restatement_against_world_frame_half_spaces():
    from gaussiangrasper_amd.grasp import default_gripper
    rng = np.random.default_rng(2)
    n, m = 1500, 40
    p = rng.uniform(-0.06, 0.06, size=(n, 3)).astype(np.float32)
    w = np.ones(n, np.float32)
    g = grasp_rows(rotation(rng, m), rng.uniform(-0.02, 0.02, size=(m, 3)), rng.uniform(0.03, 0.09, m),
                   rng.uniform(0.02, 0.04, m), rng.uniform(0.0, 0.03, m))
    for parts in (default_gripper(), slab_gripper(8)):
        body, sweep, closest = _world_planes(p, g, parts, 0.05)
        assert closest > 1e-9                   # no point within 1e-9 of a face: none had to be excluded
        r = restate(p, w, g, parts, approach=0.05)
        assert np.array_equal(r["body_count"], body) and np.array_equal(r["sweep_count"], sweep)
        assert (body.sum(1) > 0).sum() > m // 2 and (sweep.sum(1) > 0).sum() > m // 2
        assert np.array_equal(r["body_weight"], body.astype(np.float64))
    r0 = restate(p, w, g, default_gripper(), approach=0.0)
    assert r0["sweep_count"].sum() == 0
    assert np.array_equal(r0["body_count"], _world_planes(p, g, default_gripper(), 0.0)[0])


def test_restatement_limits_and_bad_rows():
    parts = slab_gripper(2)
    g = grasp_rows(np.stack([np.eye(3)] * 4), np.zeros((4, 3)), 0.5, 0.5, 0.25)
    g[1, 1] = 0.0                               # width 0
    g[2, 9] = np.nan
    g[3, 2] = -0.5                              # height < 0
    p = np.float32([[0.0, -0.125, 0.0], [0.125, 0.125, 0.0], [-0.125, 0.0625, 0.0], [0.0, 0.0, 0.5]])
    w = np.float32([0.5, 0.25, 2.0, 8.0])
    r = restate(p, w, g, parts, approach=0.25)
    assert r["valid"].tolist() == [True, False, False, False] and np.array_equal(row_valid(g), r["valid"])
    assert r["body_count"][0].tolist() == [1, 1] and r["body_weight"][0].tolist() == [0.5, 0.25]
    assert r["sweep_count"][0].tolist() == [0, 1] and r["sweep_weight"][0].tolist() == [0.0, 2.0]
    assert not r["body_count"][1:].any() and not r["clear"][1:].any() and r["clear"][0]
    assert restate(p, w, g, parts, approach=0.25, max_body=0.75, max_sweep=2.0)["clear"][0]
    assert not restate(p, w, g, parts, approach=0.25, max_body=np.nextafter(0.75, 0), max_sweep=2.0)["clear"][0]
    assert not restate(p, w, g, parts, approach=0.25, max_body=0.75, max_sweep=np.nextafter(2.0, 0))["clear"][0]
    assert restate(p, w, g, parts, approach=0.25, min_weight=0.25)["body_count"][0].tolist() == [1, 0]


# ------------------------------------------------------------------------------------------------
# the gripper model
# ------------------------------------------------------------------------------------------------
def test_default_gripper_bounds_for_a_hand_computed_row():
    from gaussiangrasper_amd.grasp import default_gripper
    parts = default_gripper()
    assert parts.shape == (4, 6, 4) and parts.dtype == np.float64
    g = grasp_rows(np.eye(3)[None], [[0, 0, 0]], 0.08, 0.02, 0.03)
    W, H, Dp = (float(g[0, k]) for k in (1, 2, 3))        # the fp32 sizes the kernel reads
    b = part_bounds(parts, g)[0]
    want = [[-0.02, Dp, -W / 2 - 0.004, -W / 2, -H / 2, H / 2],
            [-0.02, Dp, W / 2, W / 2 + 0.004, -H / 2, H / 2],
            [-0.024, -0.02, -W / 2 - 0.004, W / 2 + 0.004, -H / 2, H / 2],
            [-0.064, -0.024, -0.002, 0.002, -0.002, 0.002]]
    assert np.allclose(b, want, rtol=0, atol=1e-15)
    b = part_bounds(default_gripper(depth_base=0.03, finger_width=0.01, tail_length=0.1, tail_width=0.05,
                                    tail_height=0.02), g)[0]
    assert np.allclose(b[3], [-0.14, -0.04, -0.025, 0.025, -0.01, 0.01], rtol=0, atol=1e-15)
    assert np.allclose(b[2, :2], [-0.04, -0.03], rtol=0, atol=1e-15)
    for bad in (dict(depth_base=-1.0), dict(finger_width=math.nan), dict(tail_length=math.inf), dict(scale=0.0)):
        with pytest.raises(ValueError):
            default_gripper(**bad)


def test_default_gripper_parts_are_disjoint_up_to_faces():
    from gaussiangrasper_amd.grasp import default_gripper
    rng = np.random.default_rng(4)
    g = grasp_rows(rotation(rng, 50), np.zeros((50, 3)), rng.uniform(0.001, 0.1, 50), rng.uniform(0.001, 0.05, 50),
                   rng.uniform(0.0, 0.05, 50))
    B = part_bounds(default_gripper(), g)
    assert (B[:, :, 0::2] <= B[:, :, 1::2]).all()          # no part is empty
    for i in range(4):
        for j in range(i + 1, 4):
            lo = np.maximum(B[:, i, 0::2], B[:, j, 0::2])
            hi = np.minimum(B[:, i, 1::2], B[:, j, 1::2])
            assert ((hi - lo).min(axis=1) <= 0).all(), (i, j)      # the overlap has no volume


def test_scale_multiplies_the_constant_terms_only():
    from gaussiangrasper_amd.grasp import default_gripper, scale_gripper
    a, b = default_gripper(), default_gripper(scale=2.5)
    assert np.array_equal(b[:, :, 0], 2.5 * a[:, :, 0]) and np.array_equal(b[:, :, 1:], a[:, :, 1:])
    assert np.array_equal(scale_gripper(a, 2.5), b)
    assert (a[:, :, 0] != 0).sum() >= 10 and (a[:, :, 1:] != 0).sum() >= 10


def test_box_part_check_gripper_and_json_round_trip(tmp_path):
    from gaussiangrasper_amd.grasp import box_part, check_gripper, default_gripper, load_gripper
    wrist = box_part((-0.2, -0.064), (-0.04, 0.04), (-0.03, 0.05))
    assert wrist.shape == (6, 4) and wrist[:, 0].tolist() == [-0.2, -0.064, -0.04, 0.04, -0.03, 0.05]
    assert not wrist[:, 1:].any()
    parts = np.concatenate([default_gripper(), wrist[None]])
    assert check_gripper(parts).shape == (5, 6, 4)
    path = tmp_path / "gripper.json"
    path.write_text(json.dumps(parts.tolist()))
    assert np.array_equal(load_gripper(str(path)), parts)
    for bad in (np.zeros((0, 6, 4)), np.zeros((9, 6, 4)), np.zeros((2, 6, 3)), np.zeros((6, 4)),
                np.full((1, 6, 4), np.nan), [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            check_gripper(bad)
    for bad in ((0.0, 1.0, 2.0), (0.0, math.inf)):
        with pytest.raises(ValueError):
            box_part(bad, (0.0, 1.0), (0.0, 1.0))
    for text in ("{not json", json.dumps([[1, 2, 3]]), json.dumps({"parts": []})):
        path.write_text(text)
        with pytest.raises(ValueError, match="gripper.json"):
            load_gripper(str(path))


# ------------------------------------------------------------------------------------------------
# the C entry
# ------------------------------------------------------------------------------------------------
def _call_on_thread(fn, cases):
    got = []

    def run():
        for args in cases:
            got.append(fn(args))
    t = threading.Thread(target=run)        # gg_last_error is per thread: the message does not outlive the test
    t.start()
    t.join()
    return got


def test_clearance_argument_validation_without_a_gpu():
    from gaussiangrasper_amd import _lib
    from gaussiangrasper_amd.grasp import default_gripper
    lib = _lib.load()
    n = ctypes.c_void_p(0)
    f = ctypes.c_void_p(1 << 20)        # never dereferenced: every call below fails validation first
    good = (D * 96)(*default_gripper().ravel())
    nan_parts = (D * 96)(*default_gripper().ravel())
    nan_parts[37] = math.nan
    inf_parts = (D * 96)(*default_gripper().ravel())
    inf_parts[95] = math.inf
    ok = dict(approach=0.05, min_weight=0.0, max_body=math.inf, max_sweep=0.5)

    def args(num_points=10, pts=f, w=f, num_grasps=4, grasps=f, num_parts=4, parts=good, outs=(f,) * 6, ws=f,
             ws_bytes=1 << 30, **kw):
        d = dict(ok)
        d.update(kw)
        return (num_points, pts, w, num_grasps, grasps, num_parts, ctypes.cast(parts, ctypes.c_void_p),
                *map(D, d.values()), *outs, ws, ctypes.c_size_t(ws_bytes), n)
    cases = [
        (args(num_points=-1), b"num_points"),
        (args(num_grasps=-3), b"num_grasps"),
        (args(num_grasps=(1 << 20) + 1), b"GG_GRASP_MAX"),
        (args(num_points=(1 << 30) + 1), b"GG_GRASP_MAX_POINTS"),
        (args(num_parts=0), b"num_parts"),
        (args(num_parts=9), b"num_parts"),
        (args(num_parts=-1), b"num_parts"),
        (args(parts=n), b"parts"),
        (args(parts=nan_parts), b"coefficient"),
        (args(parts=inf_parts), b"coefficient"),
        (args(approach=-1e-3), b"approach"),
        (args(approach=math.nan), b"approach"),
        (args(approach=math.inf), b"approach"),
        (args(min_weight=math.nan), b"min_weight"),
        (args(max_body=math.nan), b"max_body"),
        (args(max_sweep=math.nan), b"max_sweep"),
        (args(grasps=n), b"null pointer"),
        (args(outs=(f, f, n, f, f, f)), b"null pointer"),
        (args(outs=(f,) * 5 + (n,)), b"null pointer"),
        (args(pts=n), b"null pointer"),
        (args(w=n), b"null pointer"),
        (args(pts=ctypes.c_void_p((1 << 20) + 2)), b"misaligned"),
        (args(ws=n), b"ws"),
        (args(ws=ctypes.c_void_p((1 << 20) + 16)), b"ws"),
    ]
    got = _call_on_thread(lambda a: (lib.gg_grasp_clearance(*a), lib.gg_last_error()), [c[0] for c in cases])
    for (st, msg), (_, want) in zip(got, cases):
        assert st == -1 and msg.startswith(b"gg_grasp_clearance") and want in msg, msg
    # the NaN sits in part 1: a model of the first part alone is accepted as far as the workspace check
    need = lib.gg_grasp_clearance_workspace(10, 4, 4)
    short = [args(ws_bytes=need - 1), args(num_parts=1, parts=nan_parts, ws_bytes=0)]
    for st, msg in _call_on_thread(lambda a: (lib.gg_grasp_clearance(*a), lib.gg_last_error()), short):
        assert st == -3 and b"workspace" in msg
    # no grasps: nothing to do, null outputs accepted
    assert lib.gg_grasp_clearance(*args(num_grasps=0, grasps=n, outs=(n,) * 6, ws=n, ws_bytes=0)) == 0
    assert lib.gg_prof_name(50) == b"gg_grasp_clearance(all launches)"


def test_clearance_workspace_query():
    from gaussiangrasper_amd import _lib
    ws = _lib.load().gg_grasp_clearance_workspace
    assert ws(-1, 5, 4) == 0 and ws(10, -1, 4) == 0 and ws(10, 0, 4) == 0 and ws(10, (1 << 20) + 1, 4) == 0
    assert ws((1 << 30) + 1, 5, 4) == 0 and ws(10, 5, 0) == 0 and ws(10, 5, 9) == 0
    assert ws(0, 5, 4) > 0 and ws(0, 5, 4) % 256 == 0                # no chunks: still not "out of range"
    assert ws(1, 5, 4) >= ws(0, 5, 4) and ws(1, 5, 4) % 256 == 0
    assert ws(300_000, 1000, 4) >= ws(50_000, 1000, 4) >= ws(1, 1000, 4)
    assert ws(50_000, 1000, 8) > ws(50_000, 1000, 4) > ws(50_000, 1000, 1)
    # bounded: the chunk count falls as the grasp tiles rise (about 2048 workgroups)
    assert ws(5_000_000, 65536, 8) < 200 << 20 and ws(5_000_000, 1024, 8) < 200 << 20


def test_clearance_refuses_host_tensors_and_bad_arguments():
    from gaussiangrasper_amd.grasp import clearance, default_gripper
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clearance(torch.zeros(4, 3), torch.zeros(4), torch.zeros(2, 17), default_gripper())


# ------------------------------------------------------------------------------------------------
# command lines, and grasp_object without a gripper
# ------------------------------------------------------------------------------------------------
def _cli_errors(main, base, tmp_path):
    for extra in (["--approach", "0.05"], ["--max-body-collision", "0.5"], ["--max-sweep-collision", "0.5"]):
        with pytest.raises(SystemExit) as e:              # they need --gripper
            main(base + extra)
        assert e.value.code == 2
    for extra in (["--approach", "-0.01"], ["--approach", "nan"], ["--approach", "inf"],
                  ["--max-body-collision", "nan"], ["--max-sweep-collision", "nan"], ["--approach"]):
        with pytest.raises(SystemExit) as e:
            main(base + ["--gripper", "default"] + extra)
        assert e.value.code == 2
    with pytest.raises(SystemExit, match="error"):        # no such gripper file
        main(base + ["--gripper", str(tmp_path / "none.json")])
    (tmp_path / "bad.json").write_text(json.dumps([[[0.0] * 4] * 5]))
    with pytest.raises(SystemExit, match="bad.json"):
        main(base + ["--gripper", str(tmp_path / "bad.json")])
    with pytest.raises(SystemExit, match="error"):        # valid options: on to the checkpoint, which is not there
        main(base + ["--gripper", "default", "--approach", "0.05", "--max-body-collision", "0.5",
                     "--max-sweep-collision", "inf"])


def test_cli_argument_errors(tmp_path):
    from gaussiangrasper_amd import grasp, grasp_propose
    g = tmp_path / "g.npy"
    np.save(g, grasp_rows(np.eye(3)[None], [[0, 0, 0]], 0.04, 0.02, 0.01))
    np.save(tmp_path / "obj.npy", np.zeros((8, 3)))
    ckpt = str(tmp_path / "none.ckpt")
    _cli_errors(grasp.main, ["--ckpt", ckpt, "--grasps", str(g), "--out", str(tmp_path / "kept.npy")], tmp_path)
    _cli_errors(grasp_propose.main, ["--ckpt", ckpt, "--object-points", str(tmp_path / "obj.npy"), "--out",
                                     str(tmp_path / "kept.npy")], tmp_path)
    assert not (tmp_path / "kept.npy").exists()


def test_grasp_object_without_a_gripper_makes_no_clearance_call(monkeypatch):
    from gaussiangrasper_amd import grasp, grasp_propose

    class Called(Exception):
        pass

    def refuse(*a, **k):
        raise Called()
    rows = torch.zeros(3, 17)
    res = grasp.GraspContacts(*(torch.zeros(3) for _ in range(6)), feasible=torch.tensor([True, False, True]))
    monkeypatch.setattr(grasp_propose, "propose_grasps", lambda *a, **k: rows)
    monkeypatch.setattr(grasp_propose, "model_points", lambda *a, **k: (torch.zeros(1, 3),) * 2 + (torch.zeros(1),))
    monkeypatch.setattr(grasp_propose, "contacts", lambda *a, **k: res)
    monkeypatch.setattr(grasp, "apply_clearance", refuse)
    monkeypatch.setattr(grasp, "clearance", refuse)
    got_rows, got, keep = grasp_propose.grasp_object(object(), None)
    assert got_rows is rows and got.clearance is None and keep.tolist() == [0, 2]
    with pytest.raises(Called):
        grasp_propose.grasp_object(object(), None, gripper=grasp.default_gripper())
