"""No-GPU checks of the one gate path behind grasp.score_grasps and grasp_propose.grasp_object (grasp.GraspGates,
grasp.apply_gates) and of the command-line options the two tools share (_cli.add_grasp_options, check_grasp_options,
grasp_gate_kwargs).  contacts, clearance, nms and model_points are recording fakes; plane_clear runs as it is, on the
CPU, behind a recorder."""
import argparse
import math
import types

import numpy as np
import pytest
import torch

from grasp_ref import grasp_rows

M, SCALE = 4, 2.0
PLANE = types.SimpleNamespace(normal=np.array([0.0, 0.0, 1.0]), offset=0.0)
GATES = dict(approach=0.05, max_body=0.5, max_sweep=0.25, nms_translation=0.03, nms_rotation=0.4,
             nms_symmetric=False, top_k=2, support=PLANE, support_margin=0.01, max_approach_tilt=2.0)


def _grasps():
    g = grasp_rows(np.stack([np.eye(3)] * M), np.array([[0.1 * k, 0.0, 1.0] for k in range(M)]), 0.05, 0.02, 0.02)
    g[:, 0] = [0.2, 0.9, 0.4, 0.7]
    return g


@pytest.fixture
def fakes(monkeypatch):
    """Both modules' contacts / model_points and grasp's clearance / nms / plane_clear record into one log."""
    from gaussiangrasper_amd import grasp, grasp_propose
    log = []
    real_plane_clear = grasp.plane_clear

    def model_points(model, mask=None):
        log.append(("model_points", mask))
        return torch.zeros(5, 3), torch.zeros(5, 3), torch.full((5,), 0.0 if mask is None else 1.0)

    def contacts(points, normals, weights, rows, *args):
        log.append(("contacts", points, weights, rows, args))
        return grasp.GraspContacts(*(torch.zeros(M) for _ in range(6)), feasible=torch.ones(M, dtype=torch.bool))

    def clearance(points, weights, rows, gripper, approach, min_weight, max_body, max_sweep):
        log.append(("clearance", points, weights, rows, gripper, approach, min_weight, max_body, max_sweep))
        clear = torch.tensor([True, True, False, True])
        return grasp.GraspClearance(*(torch.zeros(M, 4) for _ in range(4)), valid=torch.ones(M, dtype=torch.bool),
                                    clear=clear)

    def plane_clear(rows, gripper, plane, approach=0.0, margin=0.0, scale=1.0):
        log.append(("plane_clear", rows, gripper, plane, approach, margin, scale))
        return real_plane_clear(rows, gripper, plane, approach, margin, scale)

    def nms(rows, active, translation, rotation, symmetric, scale):
        log.append(("nms", rows, active.feasible.clone(), translation, rotation, symmetric, scale))
        keep = active.feasible.clone()
        return grasp.GraspNMS(keep=keep, suppressor=torch.full((M,), -1, dtype=torch.int32),
                              order=torch.nonzero(keep).reshape(-1), support=keep.to(torch.int32))

    for mod in (grasp, grasp_propose):
        monkeypatch.setattr(mod, "model_points", model_points)
        monkeypatch.setattr(mod, "contacts", contacts)
    monkeypatch.setattr(grasp, "clearance", clearance)
    monkeypatch.setattr(grasp, "plane_clear", plane_clear)
    monkeypatch.setattr(grasp, "nms", nms)
    return log


def _run_both(monkeypatch):
    """(grasp-frame candidates, their scene-frame rows, score_grasps, grasp_object with those rows as its proposals)"""
    from gaussiangrasper_amd import grasp, grasp_propose
    g = _grasps()
    rows = torch.from_numpy(grasp.grasps_to_scene(g, None, None, SCALE))
    monkeypatch.setattr(grasp_propose, "propose_grasps", lambda *a, **k: rows)
    return g, rows, grasp.score_grasps, grasp_propose.grasp_object


def _gate_calls(log):
    return [c for c in log if c[0] in ("clearance", "plane_clear", "nms")]


def test_both_pipelines_run_the_gates_in_one_order_with_the_same_scaled_arguments(fakes, monkeypatch):
    from gaussiangrasper_amd import grasp
    g, rows, score_grasps, grasp_object = _run_both(monkeypatch)
    gripper = grasp.default_gripper()
    mask = torch.ones(5, dtype=torch.bool)
    res_s = score_grasps(object(), g, mask, scale=SCALE, min_weight=0.1, gripper=gripper, **GATES)
    calls_s, whole_s = _gate_calls(fakes), [c for c in fakes if c[0] == "model_points" and c[1] is None]
    del fakes[:]
    got_rows, res_o, keep = grasp_object(object(), mask, scale=SCALE, min_weight=0.1, gripper=gripper, **GATES)
    calls_o, whole_o = _gate_calls(fakes), [c for c in fakes if c[0] == "model_points" and c[1] is None]
    assert got_rows is rows and len(whole_s) == 1 and len(whole_o) == 1      # whole-scene points: formed once
    for calls in (calls_s, calls_o):
        assert [c[0] for c in calls] == ["clearance", "plane_clear", "nms"]
        _, pts, w, r, parts, approach, min_weight, max_body, max_sweep = calls[0]
        assert torch.equal(r, rows) and pts.shape == (5, 3) and not w.any()   # the whole scene's weights
        assert np.array_equal(parts, grasp.scale_gripper(gripper, SCALE)) and np.array_equal(
            parts[:, :, 0], gripper[:, :, 0] * SCALE) and np.array_equal(parts[:, :, 1:], gripper[:, :, 1:])
        assert (approach, min_weight, max_body, max_sweep) == (0.05 * SCALE, 0.1, 0.5, 0.25)
        _, r, parts, plane, approach, margin, scale = calls[1]                # plane_clear scales by itself
        assert torch.equal(r, rows) and parts is gripper and plane is PLANE
        assert (approach, margin, scale) == (0.05, 0.01, SCALE)
        _, r, active, translation, rotation, symmetric, scale = calls[2]      # as does nms
        assert torch.equal(r, rows) and (translation, rotation, symmetric, scale) == (0.03, 0.4, False, SCALE)
        assert active.tolist() == [True, True, False, True]                   # the NMS sees what the gates left
    for res in (res_s, res_o):
        assert res.clearance is not None and res.support_clear.all() and res.nms is not None
        assert res.feasible.tolist() == [True, True, False, True]
    assert res_s.nms.order.tolist() == [0, 1] and keep.tolist() == [0, 1]      # order[:top_k]
    assert res_o.nms.order.tolist() == [0, 1, 3]                               # grasp_object returns keep beside it


def test_without_options_no_gate_runs_and_keep_is_filter_grasps(fakes, monkeypatch):
    g, rows, score_grasps, grasp_object = _run_both(monkeypatch)
    res = score_grasps(object(), g, scale=SCALE)
    assert res.nms is None and res.clearance is None and res.support_clear is None
    got_rows, res, keep = grasp_object(object(), None, scale=SCALE)
    assert keep.tolist() == [1, 3, 2, 0] and res.nms is None                   # by score, descending
    assert not _gate_calls(fakes)
    # grasp_object without a mask: the object's points are the whole scene's, formed once for both uses
    del fakes[:]
    from gaussiangrasper_amd import grasp
    grasp_object(object(), None, scale=SCALE, gripper=grasp.default_gripper())
    assert [c[0] for c in fakes] == ["model_points", "contacts", "clearance"]


@pytest.mark.parametrize("bad, text", [(dict(top_k=2), "top_k needs nms_translation"),
                                       (dict(support=PLANE), "support needs gripper")])
def test_configuration_errors_come_before_any_call(fakes, monkeypatch, bad, text):
    g, rows, score_grasps, grasp_object = _run_both(monkeypatch)
    proposed = []
    from gaussiangrasper_amd import grasp_propose
    monkeypatch.setattr(grasp_propose, "propose_grasps", lambda *a, **k: proposed.append(1))
    with pytest.raises(ValueError, match=text):
        score_grasps(object(), g, **bad)
    with pytest.raises(ValueError, match=text):
        grasp_object(object(), None, **bad)
    assert not fakes and not proposed


def test_gates_record_checks_like_check_top_k():
    from gaussiangrasper_amd.grasp import NMS_ROTATION, GraspGates
    d = GraspGates()
    assert (d.gripper, d.approach, d.max_body, d.max_sweep, d.nms_translation, d.nms_rotation, d.nms_symmetric,
            d.top_k, d.support, d.support_margin, d.max_approach_tilt) == (None, 0.0, None, None, None, NMS_ROTATION,
                                                                           True, None, None, 0.0, None)
    assert d.check() is d
    k = GraspGates(nms_translation=0.0, top_k=np.int64(3)).check().top_k
    assert k == 3 and type(k) is int
    for top_k in (0, 1.5):
        with pytest.raises(ValueError, match="top_k must be an integer >= 1"):
            GraspGates(nms_translation=0.03, top_k=top_k).check()


# ------------------------------------------------------------------------------------------------
# command lines
# ------------------------------------------------------------------------------------------------
class _Parsed(Exception):
    pass


def _parser_of(main, monkeypatch):
    """the ArgumentParser `main` builds, caught at its parse_args"""
    def caught(self, *a, **k):
        raise _Parsed(self)
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", caught)
    with pytest.raises(_Parsed) as e:
        main([])
    monkeypatch.undo()
    return e.value.args[0]


def _options(ap):
    return {s: (tuple(act.option_strings), type(act), act.default, act.type, act.nargs, act.metavar, act.help)
            for act in ap._actions for s in act.option_strings}


def test_the_two_parsers_expose_identical_gate_options(monkeypatch):
    from gaussiangrasper_amd import _cli, grasp, grasp_propose
    ap = argparse.ArgumentParser(add_help=False)
    _cli.add_grasp_options(ap)
    shared = _options(ap)
    assert sorted(shared) == sorted(
        ["--mu", "--min-opacity", "--max-collision", "--gripper", "--approach", "--max-body-collision",
         "--max-sweep-collision", "--nms-translation", "--nms-rotation", "--nms-no-symmetry", "--top-k",
         "--support-plane", "--support-dist", "--remove-support", "--support-margin", "--max-approach-tilt"])
    assert shared["--mu"][2] == grasp.MU and shared["--min-opacity"][2] == grasp.MIN_WEIGHT
    opts = [_options(_parser_of(m, monkeypatch)) for m in (grasp.main, grasp_propose.main)]
    for name, spec in shared.items():
        assert opts[0][name] == spec and opts[1][name] == spec, name
    assert "--band" in opts[0] and "--band" not in opts[1] and "--band" not in shared


def test_grasp_gate_kwargs_maps_the_checked_options():
    import inspect
    from gaussiangrasper_amd import _cli, grasp, grasp_propose
    ap = argparse.ArgumentParser()
    _cli.add_grasp_options(ap)
    a = ap.parse_args(["--mu", "0.4", "--min-opacity", "0.1", "--max-collision", "2", "--gripper", "default",
                       "--approach", "0.05", "--max-body-collision", "0.5", "--nms-translation", "0.02",
                       "--nms-rotation", "45", "--nms-no-symmetry", "--top-k", "3", "--support-plane", "fit",
                       "--max-approach-tilt", "60"])
    _cli.check_grasp_options(ap, a)
    assert _cli.grasp_gate_kwargs(a, PLANE) == dict(
        mu=0.4, min_weight=0.1, max_collision=2.0, approach=0.05, max_body=0.5, max_sweep=None, nms_translation=0.02,
        nms_rotation=math.radians(45.0), nms_symmetric=False, top_k=3, support=PLANE, support_margin=0.0,
        max_approach_tilt=math.radians(60.0))
    a = ap.parse_args([])
    _cli.check_grasp_options(ap, a)
    assert _cli.grasp_gate_kwargs(a, None) == dict(
        mu=grasp.MU, min_weight=grasp.MIN_WEIGHT, max_collision=None, approach=0.0, max_body=None, max_sweep=None,
        nms_translation=None, nms_rotation=math.radians(_cli.NMS_ROTATION_DEGREES), nms_symmetric=True, top_k=None,
        support=None, support_margin=0.0, max_approach_tilt=None)
    # every key is a keyword of both functions
    for fn in (grasp.score_grasps, grasp_propose.grasp_object):
        assert set(_cli.grasp_gate_kwargs(a, None)) < set(inspect.signature(fn).parameters)
