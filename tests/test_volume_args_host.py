"""No-GPU checks of the argument helpers every caller of the distance-field volume shares (field.volume_args,
volume_tensor, cell_count, pose_paths, sphere_table; _call.host_array, check_finite_options), and of the wrappers that
use them: each names the argument it refuses."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

from gaussiangrasper_amd import _call, arm, field, transit


def test_volume_args_takes_any_three_integers_and_an_optional_grid():
    for dims in ([3, 5, 7], (3, 5, 7), np.array([3, 5, 7], np.int32), np.array([3, 5, 7], np.int64),
                 np.array([[3, 5, 7]]), torch.tensor([3, 5, 7], dtype=torch.int32)):
        d, g, shape = field.volume_args(dims)
        assert isinstance(d, ctypes.c_int32 * 3) and list(d) == [3, 5, 7]
        assert g is None and shape == (3, 5, 7) and all(type(v) is int for v in shape)
    d, g, shape = field.volume_args(np.array([4, 4, 2], np.int32), np.array([0.5, -1.0, 2.0, 0.01]))
    assert isinstance(g, ctypes.c_double * 4) and list(g) == [0.5, -1.0, 2.0, 0.01] and shape == (4, 4, 2)
    assert list(field.volume_args([1, 2, 3], [0, 0, 0, 1])[1]) == [0.0, 0.0, 0.0, 1.0]
    for bad in ([3, 5], [3, 5, 7, 9], [], np.zeros((2, 3), np.int32)):
        with pytest.raises(ValueError, match="dims"):
            field.volume_args(bad)
    for bad in ([0, 0, 0], [0, 0, 0, 1, 1], []):
        with pytest.raises(ValueError, match="grid"):
            field.volume_args([3, 5, 7], bad)


def test_volume_tensor_names_the_tensor_it_refuses():
    good = torch.zeros(3, 5, 7, dtype=torch.int32)
    assert field.volume_tensor(good, "dist2", torch.int32, (3, 5, 7)) is good
    assert field.volume_tensor(good, "dist2", torch.int32, (3, 5, 7), torch.device("cpu")) is good
    mass = torch.zeros(3, 5, 7, dtype=torch.int64)
    assert field.volume_tensor(mass, "mass", torch.int64, (3, 5, 7)) is mass
    cases = [(good.long(), torch.int32, (3, 5, 7), None), (good.float(), torch.int32, (3, 5, 7), None),
             (good, torch.int64, (3, 5, 7), None),                                          # dtype
             (good, torch.int32, (3, 5, 8), None), (good.reshape(-1), torch.int32, (3, 5, 7), None),   # shape
             (torch.zeros(3, 7, 5, dtype=torch.int32).transpose(1, 2), torch.int32, (3, 5, 7), None),  # not contiguous
             (good, torch.int32, (3, 5, 7), torch.device("meta"))]                          # device
    for t, dtype, shape, dev in cases:
        with pytest.raises(ValueError, match="cost_xyz"):
            field.volume_tensor(t, "cost_xyz", dtype, shape, dev)


def test_cell_count_is_zero_to_far():
    assert field.cell_count("need", 0) == 0 and field.cell_count("need", field.FAR) == field.FAR
    assert field.cell_count("outside", np.int32(7)) == 7 and type(field.cell_count("outside", np.int32(7))) is int
    for name, bad in (("need", -1), ("outside", field.FAR + 1)):
        with pytest.raises(ValueError, match=name):
            field.cell_count(name, bad)


def test_pose_paths_and_sphere_table_name_what_they_refuse():
    poses = torch.zeros(2, 3, 12)
    assert field.pose_paths(poses) is poses and field.pose_paths(poses.transpose(0, 1)).is_contiguous()
    for bad in (poses.double(), poses[0], torch.zeros(2, 3, 11)):
        with pytest.raises(ValueError, match="poses"):
            field.pose_paths(bad)
    sp, need, frame = torch.zeros(5, 3), torch.zeros(5, dtype=torch.int32), torch.ones(5, dtype=torch.int32)
    out = field.sphere_table(sp, frame=frame, need=need)
    assert len(out) == 3 and out[0] is sp and out[1] is frame and out[2] is need
    alone = field.sphere_table(sp)
    assert len(alone) == 1 and alone[0] is sp
    assert field.sphere_table(torch.zeros(0, 3), need=need[:0])[0].shape == (0, 3)
    for bad in (sp.double(), torch.zeros(5, 4), torch.zeros(5)):
        with pytest.raises(ValueError, match="spheres"):
            field.sphere_table(bad, need=need)
    with pytest.raises(ValueError, match="spheres"):
        field.sphere_table(torch.zeros(field.MAX_SPHERES + 1, 3))
    for column in (need[:4], need.long(), need.reshape(5, 1)):        # length, dtype, shape
        with pytest.raises(ValueError, match="need"):
            field.sphere_table(sp, frame=frame, need=column)
        with pytest.raises(ValueError, match="frame"):
            field.sphere_table(sp, frame=column, need=need)


def test_host_array_detaches():
    t = torch.arange(6, dtype=torch.float32).reshape(2, 3).requires_grad_()
    a = _call.host_array(t, np.float64)
    assert isinstance(a, np.ndarray) and a.dtype == np.float64 and np.array_equal(a, np.arange(6.0).reshape(2, 3))
    assert _call.host_array(t).dtype == np.float32
    assert _call.host_array([[1, 2], [3, 4]], np.int64).shape == (2, 2)
    b = np.arange(3)
    assert _call.host_array(b) is b
    # the callers that took a tensor without detaching it now take one that requires grad
    rows = torch.zeros(2, 17, requires_grad=True)
    assert field.grasp_poses(rows).shape == (2, 1, 12)


def test_check_finite_options_keeps_the_messages(capsys):
    ap = argparse.ArgumentParser(prog="x")
    ok = argparse.Namespace(radius=0.1, margin=0.0)
    _call.check_finite_options(ap, ok, positive=("radius",), nonneg=("margin",))
    for a, text in ((argparse.Namespace(radius=0.0, margin=0.0), "--radius must be finite and > 0, got 0.0"),
                    (argparse.Namespace(radius=float("nan"), margin=0.0), "--radius must be finite and > 0, got nan"),
                    (argparse.Namespace(radius=0.1, margin=-1.0), "--margin must be finite and >= 0, got -1.0"),
                    (argparse.Namespace(radius=0.1, margin=float("inf")), "--margin must be finite and >= 0, got inf")):
        with pytest.raises(SystemExit) as e:
            _call.check_finite_options(ap, a, positive=("radius",), nonneg=("margin",))
        assert e.value.code == 2 and text in capsys.readouterr().err


def _volume_calls():
    """(name of the refused argument, call(dist2-like tensor)) for every wrapper that takes a volume.  The other
    arguments are valid, so the volume is what is refused."""
    ok = torch.zeros(4, 4, 4, dtype=torch.int32)
    dims, grid = [4, 4, 4], [0, 0, 0, 0.01]
    z = torch.zeros(1, dtype=torch.int32)
    cells, length = torch.zeros(1, 8, 3, dtype=torch.int32), torch.ones(1, dtype=torch.int32)
    model = arm.default_arm()
    return [
        ("dist2", lambda t: field.paths(t, grid, dims, torch.zeros(1, 1, 12), torch.zeros(1, 3), z)),
        ("dist2", lambda t: arm.clear(model, t, grid, dims, torch.zeros(1, 7, dtype=torch.float64), torch.zeros(1, 3),
                                      z, z)),
        ("dist2", lambda t: transit.route(t, dims, 4, [[0, 0, 0]])),
        ("out", lambda t: transit.route(ok, dims, 4, [[0, 0, 0]], out=t)),
        ("dist2", lambda t: transit.descend_cells(t, dims, 4, ok, [[0, 0, 0]], 8)),
        ("cost", lambda t: transit.descend_cells(ok, dims, 4, t, [[0, 0, 0]], 8)),
        ("dist2", lambda t: transit.sight(t, dims, 4, [[0, 0, 0]], [[1, 1, 1]])),
        ("dist2", lambda t: transit.shortcut_cells(t, dims, 4, cells, length, 8)),
    ]


@pytest.mark.parametrize("case", range(8))
@pytest.mark.parametrize("what", ["dtype", "shape"])
def test_every_volume_call_names_the_volume_it_refuses(case, what, monkeypatch):
    # the wrappers look at the device first; here that check lets the host tensors through, and every call below is
    # refused before it reaches the library
    for mod in (field, transit, arm):
        monkeypatch.setattr(mod, "_require_hip", lambda *tensors: tensors[0].device)
    name, call = _volume_calls()[case]
    bad = torch.zeros(4, 4, 4, dtype=torch.int64) if what == "dtype" else torch.zeros(4, 4, 5, dtype=torch.int32)
    with pytest.raises(ValueError, match=f"^{name} must be a contiguous torch.int32 \\(4, 4, 4\\) tensor"):
        call(bad)
