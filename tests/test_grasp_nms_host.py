"""No-GPU checks of grasp NMS (gaussiangrasper_amd.grasp.nms, gg_grasp_nms): the fp64 restatement
(tests/grasp_nms_ref.py) against the properties of a greedy suppression checked by brute force, its rotation test
against the angle itself, the half-turn symmetry, the C entry's argument validation and workspace query, the order and
support that the Python layer builds, the command-line tools' argument errors, and that score_grasps and grasp_object
without nms_translation make no NMS call."""
import ctypes
import math
import threading

import numpy as np
import pytest
import torch

from grasp_nms_ref import all_pairs, clustered_rows, restate
from grasp_ref import grasp_rows, rotation

D = ctypes.c_double
MAX_ORDER = 65536


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def test_restatement_is_a_greedy_suppression():
    rng = np.random.default_rng(7)
    m = 300
    g = clustered_rows(rng, m, 40, spread_t=0.012, spread_r=0.3)
    order = np.argsort(-g[:, 0], kind="stable")
    tr_, cr = 0.014, math.cos(0.3)
    r = restate(g, order, tr_, cr, True)
    near = all_pairs(g, tr_, cr, True)["near"]
    assert np.array_equal(near, near.T) and near.diagonal().all()
    pos = np.empty(m, np.int64)
    pos[order] = np.arange(m)
    keep, sup = r["keep"], r["suppressor"]
    kept = np.nonzero(keep)[0]
    assert r["num_kept"] == len(kept) and np.array_equal(r["kept"][:len(kept)], order[keep[order]])
    assert (r["kept"][len(kept):] == -1).all() and (sup[keep] == -1).all() and (sup[~keep] >= 0).all()
    off = near & ~np.eye(m, dtype=bool)
    assert not off[np.ix_(kept, kept)].any()                  # no two kept rows are near
    for j in np.nonzero(~keep)[0]:
        s = sup[j]
        assert near[j, s] and keep[s] and pos[s] < pos[j]     # near its suppressor, which is kept and earlier
        earlier = kept[pos[kept] < pos[s]]
        assert not near[j, earlier].any()                     # and no earlier kept row is near it
    # the scene is not trivial
    assert m / 4 <= (~keep).sum() <= 3 * m / 4
    better_near = np.array([(near[j] & (pos < pos[j])).any() for j in range(m)])      # "anything better is near"
    chain = keep & better_near
    assert chain.sum() >= 1                                   # kept, though near a better (suppressed) row
    assert not np.array_equal(keep, ~better_near)             # the non-greedy rule gives another answer
    # the walk depends on the order: reversed, other rows survive
    assert not np.array_equal(restate(g, order[::-1], tr_, cr, True)["keep"], keep)


def test_rotation_test_against_the_angle():
    rng = np.random.default_rng(8)
    g = clustered_rows(rng, 200, 6, spread_r=0.6, twins=False)
    g[:, 13:16] = 0.0
    for rot in (0.05, 0.3, math.pi / 6, 1.0, 2.5):
        p = all_pairs(g, 1.0, math.cos(rot), False)
        angle = np.arccos(np.clip((p["tr"] - 1.0) / 2.0, -1.0, 1.0))
        clear = np.abs(angle - rot) > 1e-9
        assert clear.sum() > 0.99 * clear.size
        assert np.array_equal(p["near"][clear], (angle <= rot)[clear])
        off = ~np.eye(200, dtype=bool)
        assert p["near"][off].any() and not p["near"][off].all()


def test_half_turn_twin_is_near_only_with_symmetry():
    rng = np.random.default_rng(9)
    R = rotation(rng, 20)
    t = rng.uniform(-0.1, 0.1, size=(20, 3))
    g = np.concatenate([grasp_rows(R, t, 0.05, 0.02, 0.02), grasp_rows(R * np.array([1.0, -1.0, -1.0]), t, 0.05,
                                                                      0.02, 0.02)])
    pair = (np.arange(20), np.arange(20) + 20)
    for rot in (0.0, 0.1, math.pi / 6, 3.0):
        # float32 rotations are orthonormal to 1e-7: cos(0) as the limit needs a little room
        c = math.cos(rot) - (1e-6 if rot == 0.0 else 0.0)
        assert all_pairs(g, 0.0, c, True)["near"][pair].all()
        assert not all_pairs(g, 0.0, c, False)["near"][pair].any()
    order = np.arange(40)
    assert restate(g, order, 0.0, math.cos(0.1), True)["num_kept"] == 20
    assert restate(g, order, 0.0, math.cos(0.1), False)["num_kept"] == 40
    r = restate(g, order[::-1], 0.0, math.cos(0.1), True)
    assert r["keep"][20:].all() and np.array_equal(r["suppressor"][:20], np.arange(20) + 20)


def test_restatement_skips_rows_that_take_no_part():
    g = grasp_rows(np.stack([np.eye(3)] * 6), np.zeros((6, 3)), 0.05, 0.02, 0.02)
    g[1, 7] = np.nan
    g[2, 14] = np.inf
    g[3, 0] = np.nan                    # the score is not read
    r = restate(g, [9, 1, -1, 2, 3, 0, 5], 0.01, 0.5, True)
    assert r["keep"].tolist() == [False, False, False, True, False, False]
    assert r["suppressor"].tolist() == [3, -2, -2, -1, -2, 3]
    assert r["kept"].tolist() == [3, -1, -1, -1, -1, -1, -1] and r["num_kept"] == 1


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


def test_nms_argument_validation_without_a_gpu():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    n = ctypes.c_void_p(0)
    f = ctypes.c_void_p(1 << 20)        # never dereferenced: every call below fails validation first

    def args(num_grasps=8, grasps=f, num_order=5, order=f, translation=0.03, cos_rotation=0.5, symmetric=1,
             outs=(f,) * 4, ws=f, ws_bytes=1 << 30):
        return (num_grasps, grasps, num_order, order, D(translation), D(cos_rotation), symmetric, *outs, ws,
                ctypes.c_size_t(ws_bytes), n)
    cases = [
        (args(num_grasps=-1), b"num_grasps"),
        (args(num_grasps=(1 << 20) + 1), b"GG_GRASP_MAX"),
        (args(num_order=-1), b"num_order"),
        (args(num_order=MAX_ORDER + 1), b"GG_NMS_MAX_ORDER"),
        (args(translation=-1e-9), b"translation"),
        (args(translation=math.nan), b"translation"),
        (args(translation=math.inf), b"translation"),
        (args(cos_rotation=1.0000001), b"cos_rotation"),
        (args(cos_rotation=-1.5), b"cos_rotation"),
        (args(cos_rotation=math.nan), b"cos_rotation"),
        (args(grasps=n), b"null pointer"),
        (args(order=n), b"null pointer"),
        (args(outs=(n, f, f, f)), b"null pointer"),
        (args(outs=(f, n, f, f)), b"null pointer"),
        (args(outs=(f, f, n, f)), b"null pointer"),
        (args(outs=(f, f, f, n)), b"null pointer"),
        (args(num_order=0, outs=(f, f, n, n)), b"null pointer"),          # rows to write, nowhere for num_kept
        (args(order=ctypes.c_void_p((1 << 20) + 2)), b"misaligned"),
        (args(ws=n), b"ws"),
        (args(ws=ctypes.c_void_p((1 << 20) + 16)), b"ws"),
    ]
    got = _call_on_thread(lambda a: (lib.gg_grasp_nms(*a), lib.gg_last_error()), [c[0] for c in cases])
    for (st, msg), (_, want) in zip(got, cases):
        assert st == -1 and msg.startswith(b"gg_grasp_nms") and want in msg, msg
    need = lib.gg_grasp_nms_workspace(5)
    for st, msg in _call_on_thread(lambda a: (lib.gg_grasp_nms(*a), lib.gg_last_error()),
                                   [args(ws_bytes=need - 1), args(ws_bytes=0)]):
        assert st == -3 and b"workspace" in msg
    # nothing to walk and nothing to write: null pointers accepted
    assert lib.gg_grasp_nms(*args(num_grasps=0, grasps=n, num_order=0, order=n, outs=(n,) * 4, ws=n,
                                  ws_bytes=0)) == 0
    assert lib.gg_prof_name(51) == b"gg_grasp_nms(all launches)"
    assert lib.gg_prof_name(52) != lib.gg_prof_name(51)


def test_nms_workspace_query():
    from gaussiangrasper_amd import _lib
    ws = _lib.load().gg_grasp_nms_workspace
    assert ws(-1) == 0 and ws(MAX_ORDER + 1) == 0
    assert ws(0) > 0 and ws(0) % 256 == 0
    for a in (1, 63, 64, 65, 1000, 4097, 16384, 32768, MAX_ORDER):
        assert ws(a) % 256 == 0 and ws(a - 1) <= ws(a)
        assert a * ((a + 63) // 64) * 8 <= ws(a) <= a * a // 8 + 64 * a + 1024       # the bit matrix, plus O(A)
    assert ws(16384) <= 33 << 20 and ws(MAX_ORDER) <= 516 << 20


def test_nms_refuses_host_tensors_and_bad_arguments():
    from gaussiangrasper_amd.grasp import nms
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nms(torch.zeros(4, 17))


# ------------------------------------------------------------------------------------------------
# Python: the order, the support, and the calls that are not made
# ------------------------------------------------------------------------------------------------
def test_order_is_stable_drops_nan_scores_and_is_cut():
    from gaussiangrasper_amd.grasp import nms_order
    g = torch.zeros(10, 17)
    g[:, 0] = torch.tensor([0.5, 0.9, math.nan, 0.5, 0.9, -math.inf, math.inf, 0.5, 0.1, 0.9])
    assert nms_order(g).tolist() == [6, 1, 4, 9, 0, 3, 7, 8, 5] and nms_order(g).dtype == torch.int32
    active = torch.tensor([1, 0, 1, 1, 1, 1, 0, 1, 1, 1], dtype=torch.bool)
    assert nms_order(g, active).tolist() == [4, 9, 0, 3, 7, 8, 5]
    assert nms_order(g, active, max_candidates=3).tolist() == [4, 9, 0]
    assert nms_order(g, torch.zeros(10, dtype=torch.bool)).tolist() == []
    # the sort is on the fp32 score: two scores that differ only in fp64 are equal and go by index
    rng = np.random.default_rng(3)
    s = rng.integers(0, 50, size=2000).astype(np.float32) / 8
    g = torch.zeros(2000, 17)
    g[:, 0] = torch.from_numpy(s)
    assert np.array_equal(nms_order(g, max_candidates=65536).numpy(), np.argsort(-s, kind="stable"))
    for bad in (0, -1, 65537, 2.5):
        with pytest.raises(ValueError, match="max_candidates"):
            nms_order(g, None, bad)
    with pytest.raises(ValueError, match="active"):
        nms_order(g, torch.ones(5, dtype=torch.bool))


def test_support_counts_the_rows_a_kept_row_suppressed():
    from gaussiangrasper_amd.grasp import nms_support
    keep = torch.tensor([True, False, False, True, False, False, True])
    sup = torch.tensor([-1, 0, 0, -1, 3, -2, -1], dtype=torch.int32)
    got = nms_support(keep, sup)
    assert got.dtype == torch.int32 and got.tolist() == [3, 0, 0, 2, 0, 0, 1]
    assert nms_support(torch.zeros(0, dtype=torch.bool), torch.zeros(0, dtype=torch.int32)).tolist() == []
    rng = np.random.default_rng(5)
    g = clustered_rows(rng, 120, 10)
    r = restate(g, np.argsort(-g[:, 0], kind="stable"), 0.03, math.cos(math.pi / 6), True)
    got = nms_support(torch.from_numpy(r["keep"]), torch.from_numpy(r["suppressor"])).numpy()
    assert got.sum() == 120 and (got[r["keep"]] >= 1).all() and not got[~r["keep"]].any() and got.max() > 3


class _Called(Exception):
    pass


def _refuse(*a, **k):
    raise _Called()


def _spy(monkeypatch):
    """every way to an NMS call raises _Called"""
    from gaussiangrasper_amd import _lib, grasp
    monkeypatch.setattr(_lib.load(), "gg_grasp_nms", _refuse)
    monkeypatch.setattr(grasp, "nms", _refuse)
    monkeypatch.setattr(grasp, "apply_nms", _refuse)


def _contacts():
    from gaussiangrasper_amd import grasp
    return grasp.GraspContacts(*(torch.zeros(3) for _ in range(6)), feasible=torch.tensor([True, False, True]))


def test_grasp_object_without_nms_translation_makes_no_nms_call(monkeypatch):
    from gaussiangrasper_amd import grasp_propose
    rows = torch.zeros(3, 17)
    rows[:, 0] = torch.tensor([0.1, 0.9, 0.5])
    res = _contacts()
    monkeypatch.setattr(grasp_propose, "propose_grasps", lambda *a, **k: rows)
    monkeypatch.setattr(grasp_propose, "model_points", lambda *a, **k: (torch.zeros(1, 3),) * 2 + (torch.zeros(1),))
    monkeypatch.setattr(grasp_propose, "contacts", lambda *a, **k: res)
    _spy(monkeypatch)
    got_rows, got, keep = grasp_propose.grasp_object(object(), None)
    assert got_rows is rows and got.nms is None and got.clearance is None and keep.tolist() == [2, 0]
    with pytest.raises(_Called):
        grasp_propose.grasp_object(object(), None, nms_translation=0.03)
    with pytest.raises(_Called):
        grasp_propose.grasp_object(object(), None, nms_translation=0.0, top_k=2)
    for bad in (dict(top_k=5), dict(top_k=1, nms_rotation=0.1), dict(nms_translation=0.03, top_k=0),
                dict(nms_translation=0.03, top_k=1.5)):
        with pytest.raises(ValueError, match="top_k"):
            grasp_propose.grasp_object(object(), None, **bad)


def test_score_grasps_without_nms_translation_makes_no_nms_call(monkeypatch):
    from gaussiangrasper_amd import grasp
    res = _contacts()
    monkeypatch.setattr(grasp, "model_points", lambda *a, **k: (torch.zeros(1, 3),) * 2 + (torch.zeros(1),))
    monkeypatch.setattr(grasp, "contacts", lambda *a, **k: res)
    _spy(monkeypatch)
    g = grasp_rows(np.stack([np.eye(3)] * 3), np.zeros((3, 3)), 0.05, 0.02, 0.02)
    got = grasp.score_grasps(object(), g)
    assert got is res and got.nms is None
    with pytest.raises(_Called):
        grasp.score_grasps(object(), g, nms_translation=0.03)
    with pytest.raises(ValueError, match="top_k"):
        grasp.score_grasps(object(), g, top_k=5)


def test_report_arrays_gain_the_nms_record():
    from gaussiangrasper_amd import _cli, grasp
    res = _contacts()
    assert not any(k.startswith("nms_") for k in _cli.report_arrays(res))
    res.nms = grasp.GraspNMS(keep=torch.tensor([True, False, True]), suppressor=torch.tensor([-1, -2, -1]),
                             order=torch.tensor([2, 0]), support=torch.tensor([1, 0, 1]))
    out = _cli.report_arrays(res)
    assert out["nms_keep"].tolist() == [True, False, True] and out["nms_suppressor"].tolist() == [-1, -2, -1]
    assert out["nms_support"].tolist() == [1, 0, 1]
    assert grasp.nms_summary(2, 3, res, 2, "grasps") == "2 of 3 grasps feasible, 2 distinct after NMS, 2 written"
    res.nms = None
    assert grasp.nms_summary(2, 3, res, 2, "grasps") == "2 of 3 grasps feasible"


# ------------------------------------------------------------------------------------------------
# command lines
# ------------------------------------------------------------------------------------------------
def _cli_errors(main, base):
    for extra in (["--nms-rotation", "30"], ["--nms-no-symmetry"], ["--top-k", "5"]):
        with pytest.raises(SystemExit) as e:              # they need --nms-translation
            main(base + extra)
        assert e.value.code == 2
    for extra in (["--nms-translation", "nan"], ["--nms-translation", "-0.01"], ["--nms-translation", "inf"],
                  ["--nms-translation"], ["--nms-translation", "0.03", "--nms-rotation", "nan"],
                  ["--nms-translation", "0.03", "--nms-rotation", "-1"],
                  ["--nms-translation", "0.03", "--nms-rotation", "181"],
                  ["--nms-translation", "0.03", "--top-k", "0"], ["--nms-translation", "0.03", "--top-k", "-2"],
                  ["--nms-translation", "0.03", "--top-k", "2.5"]):
        with pytest.raises(SystemExit) as e:
            main(base + extra)
        assert e.value.code == 2
    with pytest.raises(SystemExit, match="error"):        # valid options: on to the checkpoint, which is not there
        main(base + ["--nms-translation", "0.03", "--nms-rotation", "20", "--nms-no-symmetry", "--top-k", "10"])
    with pytest.raises(SystemExit, match="error"):
        main(base + ["--nms-translation", "0"])


def test_cli_argument_errors(tmp_path):
    from gaussiangrasper_amd import grasp, grasp_propose
    g = tmp_path / "g.npy"
    np.save(g, grasp_rows(np.eye(3)[None], [[0, 0, 0]], 0.04, 0.02, 0.01))
    np.save(tmp_path / "obj.npy", np.zeros((8, 3)))
    ckpt = str(tmp_path / "none.ckpt")
    _cli_errors(grasp.main, ["--ckpt", ckpt, "--grasps", str(g), "--out", str(tmp_path / "kept.npy")])
    _cli_errors(grasp_propose.main, ["--ckpt", ckpt, "--object-points", str(tmp_path / "obj.npy"), "--out",
                                     str(tmp_path / "kept.npy")])
    assert not (tmp_path / "kept.npy").exists()
