"""No-GPU checks of grasp proposals (gaussiangrasper_amd.grasp_propose, gg_grasp_propose): the fp64 restatement
(tests/grasp_propose_ref.py) against closed forms it did not come from (a box, a sphere, the frame's orthonormality
and orientation), its rows fed to the grasp filter's restatement (tests/grasp_ref.py: the row layout and frame are the
ones the filter reads), the C entry's argument validation and workspace query, and the Python layer without a
device."""
import ctypes
import json
import math
import threading

import numpy as np
import pytest
import torch

import grasp_ref
from grasp_propose_ref import box_faces, frame, restate

D = ctypes.c_double
H = 2.0 ** -8


# ------------------------------------------------------------------------------------------------
# the restatement against closed forms
# ------------------------------------------------------------------------------------------------
def _check_frames(rows):
    R = rows[..., 4:13].reshape(-1, 3, 3)
    assert np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() < 1e-12
    assert np.abs(np.linalg.det(R) - 1.0).max() < 1e-12
    return R


def test_restatement_on_a_box():
    size, centre = np.array([16 * H, 12 * H, 14 * H]), np.array([0.25, -0.125, 0.5])
    p, n = box_faces(size, H, centre)
    n[::3] *= -2.5                                          # any sign, any length
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    K, up = 8, (0.0, 0.0, 1.0)
    r = restate(p, n, np.ones(len(p)), np.arange(len(p)), num_approach=K, up=up)
    assert r["valid"].all() and (r["tube_count"] >= 2).all()
    ax = np.abs(n).argmax(1)
    assert np.abs(r["span"] - size[ax]).max() < 1e-12
    assert np.abs(r["rows"][:, :, 1] - (size[ax] + 0.01)[:, None]).max() < 1e-12
    assert np.abs(r["mid"][np.arange(len(p)), ax] - centre[ax]).max() < 1e-12            # on the mid-plane
    off = np.ones_like(p, bool)
    off[np.arange(len(p)), ax] = False
    assert np.abs(r["mid"] - p)[off].max() < 1e-12                                       # straight across
    assert np.abs(np.abs(r["axis"]) - np.abs(np.sign(n))).max() < 1e-12                  # b = the face normal
    assert np.array_equal(r["rows"][:, :, 0], np.ones((len(p), K)))                      # score == 1
    # contacts: the seed and its antipode
    pr = r["pair_idx"]
    assert ((pr[:, 0] == np.arange(len(p))) | (pr[:, 1] == np.arange(len(p)))).all()
    assert np.abs(np.abs(p[pr[:, 1]] - p[pr[:, 0]]).sum(1) - size[ax]).max() < 1e-12
    R = _check_frames(r["rows"]).reshape(len(p), K, 3, 3)
    assert np.abs(R[:, :, :, 1] - r["axis"][:, None]).max() < 1e-15                      # column 1 = closing axis
    # approach 0 comes from above unless the closing axis is vertical; the fallback is taken exactly then
    a0 = R[:, 0, :, 0]
    assert np.array_equal(r["fallback"], ax == 2)
    assert (a0[ax != 2] @ np.array(up) < -0.999999).all()
    assert np.abs(a0[ax == 2] - [1.0, 0.0, 0.0]).max() < 1e-12                           # smallest |b_k|, smallest k
    # t sits half a finger depth back along the approach
    assert np.abs(r["rows"][:, :, 13:16] - (r["mid"][:, None] - 0.01 * R[:, :, :, 0])).max() < 1e-15
    assert (r["rows"][:, :, 2:4] == 0.02).all() and (r["rows"][:, :, 16] == 0).all()


def test_restatement_on_a_sphere():
    k = 1500
    i = np.arange(k) + 0.5
    th, ph = np.arccos(1 - 2 * i / k), np.pi * (1 + 5 ** 0.5) * i
    d = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], 1)
    half = (0.04 * d).astype(np.float32).astype(np.float64)
    p = np.concatenate([half, -half])                       # exact antipodes
    n = p * np.where(np.arange(2 * k) % 3 == 0, -16.0, 16.0)[:, None]        # exactly radial, any sign and length
    up = (0.3, -0.2, 1.0)
    r = restate(p, n, np.ones(2 * k), np.arange(2 * k), num_approach=4, up=up)
    assert r["valid"].all()
    assert np.abs(r["mid"]).max() < 1e-12                   # the centre
    assert np.abs(r["span"] - 2.0 * np.linalg.norm(p, axis=1)).max() < 1e-12 and np.abs(r["span"] - 0.08).max() < 1e-8
    assert np.array_equal(np.sort(r["pair_idx"], 1),
                          np.sort(np.stack([np.arange(2 * k), (np.arange(2 * k) + k) % (2 * k)], 1), 1))
    R = _check_frames(r["rows"]).reshape(2 * k, 4, 3, 3)
    assert not r["fallback"].any() and (R[:, 0, :, 0] @ np.array(up) < 0).all()
    assert np.abs(r["rows"][:, :, 0] - 1.0).max() < 1e-12


def test_frame_fallback_only_when_the_axis_is_parallel_to_up():
    up = np.array([1.0, 2.0, -2.0])
    for b, want in ((up / 3.0, True), (-up / 3.0, True), (np.array([0.0, 1.0, 0.0]), False),
                    (np.array([2.0, -1.0, 0.0]) / math.sqrt(5.0), False)):
        a0, c0, fb = frame(b, up)
        assert fb == want
        assert abs(a0 @ b) < 1e-15 and abs(a0 @ a0 - 1) < 1e-15 and np.abs(np.cross(a0, b) - c0).max() < 1e-15
        if not fb:
            assert a0 @ up < 0
        else:
            e = np.eye(3)[0] - b * b[0]
            assert np.abs(a0 - e / np.linalg.norm(e)).max() < 1e-15


def test_restatement_decisions_ties_and_participation():
    """dyadic coordinates: every product is exact, so the closed edges decide as the contract states"""
    r_, W, w0, c = 2.0 ** -8, 2.0 ** -3, 2.0 ** -6, 2.0 ** -6
    e = 2.0 ** -14
    kw = dict(tube_radius=r_, max_width=W, min_width=w0, clearance=c, num_approach=1)
    x = np.array([1.0, 0.0, 0.0])

    def one(pts, nrm=None, w=None, seeds=(0,), **k2):
        pts = np.asarray(pts, np.float64)
        nrm = np.tile(2.0 * x, (len(pts), 1)) if nrm is None else np.asarray(nrm, np.float64)
        w = np.ones(len(pts)) if w is None else w
        out = restate(pts, nrm, w, np.asarray(seeds), **dict(kw, **k2))
        return {k: v[0] for k, v in out.items()}
    # on the tube radius: in; one step outside: out
    o = one([[0, 0, 0], [2.0 ** -5, r_, 0], [2.0 ** -4, r_ + e, 0]])
    assert o["tube_count"] == 2 and list(o["pair_idx"]) == [0, 1] and o["valid"]
    # exactly at s = W: in the tube, but wider than W - 2c: not valid; at W - 2c: valid; at min_width: valid, below: not
    o = one([[0, 0, 0], [W, 0, 0], [W + e, 0, 0]])
    assert o["tube_count"] == 2 and list(o["pair_idx"]) == [0, 1] and not o["valid"] and o["span"] == W
    assert np.isnan(o["rows"]).all()
    assert one([[0, 0, 0], [W - 2 * c, 0, 0]])["valid"] and not one([[0, 0, 0], [W - 2 * c + e, 0, 0]])["valid"]
    assert one([[0, 0, 0], [-w0, 0, 0]])["valid"] and not one([[0, 0, 0], [-w0 + e, 0, 0]])["valid"]
    # ties: the smallest index; duplicates; both directions along the line
    o = one([[0, 0, 0], [2.0 ** -5, 0, e], [2.0 ** -5, e, 0], [-(2.0 ** -5), 0, 0], [-(2.0 ** -5), 0, 0]])
    assert list(o["pair_idx"]) == [3, 1] and o["tube_count"] == 5 and o["span"] == 2.0 ** -4
    # no part: NaN point, inf normal, weight 0 / NaN; a seed among them or out of range is not usable
    far = [2.0 ** -4, 0, 0]
    pts = [[0, 0, 0], [2.0 ** -5, 0, 0], [2.0 ** -4, np.nan, 0], far, far, far]
    nrm = [2.0 * x] * 3 + [[np.inf, 0, 0]] + [2.0 * x] * 2
    w = np.array([1.0, 1.0, 1.0, 1.0, 0.0, np.nan])
    out = restate(pts, nrm, w, np.array([0, 1, 2, 3, 4, 5, 6, -1]), **kw)
    assert out["tube_count"].tolist() == [2, 2, 0, 0, 0, 0, 0, 0]
    assert out["pair_idx"].tolist() == [[0, 1], [0, 1]] + [[-1, -1]] * 6
    assert out["valid"].tolist() == [True, True] + [False] * 6 and np.isnan(out["span"][2:]).all()
    # zero-length normal on the seed: not usable; on a contact: not valid, though the contact is found
    out = restate([[0, 0, 0], [2.0 ** -5, 0, 0]], [[0, 0, 0], 2.0 * x], np.ones(2), np.array([0, 1]), **kw)
    assert out["pair_idx"].tolist() == [[-1, -1], [0, 1]] and out["valid"].tolist() == [False, False]
    assert out["tube_count"].tolist() == [0, 2] and out["span"][1] == 2.0 ** -5
    # min_align: a contact normal 60 degrees off the line passes its own cosine (closed) and fails just above it
    t = [[0, 0, 0], [2.0 ** -5, 0, 0]]
    nn_ = [2.0 * x, [1.0, 0.0, math.sqrt(3.0)]]
    g = np.float64(np.float32(math.sqrt(3.0)))
    edge = 1.0 / math.sqrt(1.0 + g * g)
    assert one(t, nn_, min_align=edge * (1 - 1e-9))["valid"] and not one(t, nn_, min_align=edge * (1 + 1e-9))["valid"]
    s = one(t, nn_, min_align=0.0)["rows"][0, 0]
    assert abs(s - edge) < 1e-12                            # score = |cos| at the tilted contact x 1 at the seed


# ------------------------------------------------------------------------------------------------
# closing the loop on the CPU: proposed rows through the filter's restatement
# ------------------------------------------------------------------------------------------------
def test_proposed_rows_through_the_filter_restatement():
    """two parallel plates (normals along y); one seed per tilt whose own normal is tilted by phi in the x-y plane
    and whose weight is negligible.  The proposal closes along the tilted line; the filter then measures the plates'
    normals against it: angle = phi on both sides, feasible exactly when phi <= atan(mu)."""
    hg, mu, tube = 0.01, 0.5, 0.003
    x, z = (a.ravel() for a in np.meshgrid(np.linspace(-0.03, 0.03, 61), np.linspace(-0.005, 0.005, 11)))
    left = np.stack([x, np.full_like(x, -hg), z], 1)
    right = np.stack([x, np.full_like(x, hg), z], 1)
    nl, nr_ = np.tile([0.0, -1.0, 0.0], (len(x), 1)), np.tile([0.0, 1.0, 0.0], (len(x), 1))
    nl[::3] *= -1.0
    deg = [0.0, 5.0, 10.0, 20.0, 25.0, 26.0, 27.0, 30.0, 40.0]
    rad = np.radians(deg)
    sp = np.array([[0.0, -hg, 0.0]] * len(deg))
    sn = np.stack([np.sin(rad), np.cos(rad), np.zeros(len(deg))], 1)
    p = np.concatenate([left, right, sp]).astype(np.float32)
    n = np.concatenate([nl, nr_, sn]).astype(np.float32)
    w = np.concatenate([np.ones(2 * len(x)), np.full(len(deg), 1e-6)]).astype(np.float32)
    seeds = 2 * len(x) + np.arange(len(deg))
    K = 2
    prop = restate(p, n, w, seeds, num_approach=K, tube_radius=tube)
    assert prop["valid"].all()
    assert (prop["pair_idx"][:, 1] >= len(x)).all() and (prop["pair_idx"][:, 1] < 2 * len(x)).all()   # the far plate
    extra = prop["span"] - 2 * hg / np.cos(rad)             # the tube's width lets the extremes sit off the line
    assert (extra >= -1e-7).all() and (extra <= 2 * tube * np.tan(rad) + 1e-7).all()
    rows = prop["rows"].reshape(-1, 17).astype(np.float32)
    got = grasp_ref.restate(p, n, w, rows, mu=mu)
    assert got["valid"].all()
    ci = got["contact_idx"].reshape(len(deg), K, 2)
    assert (ci[..., 0] < len(x)).all() and (ci[..., 1] >= len(x)).all() and (ci[..., 1] < 2 * len(x)).all()
    ang = got["angles"].reshape(len(deg), K, 2)
    assert np.allclose(ang, rad[:, None, None], atol=1e-5)
    lim = math.degrees(math.atan(mu))                       # 26.57 deg
    assert got["feasible"].reshape(len(deg), K).tolist() == [[d <= lim] * K for d in deg]


# ------------------------------------------------------------------------------------------------
# the C entry without a GPU
# ------------------------------------------------------------------------------------------------
def _call_on_thread(fn, cases):
    got = []

    def run():
        for args in cases:
            got.append(fn(args))
    t = threading.Thread(target=run)        # gg_last_error is per thread
    t.start()
    t.join()
    return got


NAMES = ("tube_radius", "max_width", "min_width", "clearance", "depth", "height", "min_weight", "min_align")
OK = (0.003, 0.10, 0.005, 0.005, 0.02, 0.02, 0.0, 0.0)


def test_propose_argument_validation_without_a_gpu():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    n = ctypes.c_void_p(0)
    f = ctypes.c_void_p(1 << 20)        # never dereferenced: every call below fails validation first
    up_ok = (D * 3)(0.0, 0.0, 1.0)
    keep = [up_ok]

    def args(num_points=10, pts=f, nrm=f, w=f, num_seeds=4, seeds=f, params=OK, up=up_ok, k=8, outs=(f,) * 5, ws=f,
             ws_bytes=1 << 30):
        if isinstance(up, tuple):
            up = (D * 3)(*up)
            keep.append(up)
        return (num_points, pts, nrm, w, num_seeds, seeds, *map(D, params), ctypes.cast(up, ctypes.c_void_p), k,
                *outs, ws, ctypes.c_size_t(ws_bytes), n)

    def p(**kw):
        d = dict(zip(NAMES, OK))
        d.update(kw)
        return tuple(d.values())
    cases = [
        (args(num_points=-1), b"num_points"),
        (args(num_seeds=-3), b"num_seeds"),
        (args(num_seeds=(1 << 20) + 1), b"GG_PROPOSE_MAX_SEEDS"),
        (args(params=p(tube_radius=-1e-3)), b"tube_radius"),
        (args(params=p(tube_radius=math.nan)), b"tube_radius"),
        (args(params=p(max_width=0.0)), b"max_width"),
        (args(params=p(max_width=math.inf)), b"max_width"),
        (args(params=p(min_width=-1.0)), b"min_width"),
        (args(params=p(clearance=-0.1)), b"clearance"),
        (args(params=p(clearance=0.051)), b"clearance"),
        (args(params=p(depth=-0.02)), b"depth"),
        (args(params=p(height=0.0)), b"height"),
        (args(params=p(min_weight=math.nan)), b"min_weight"),
        (args(params=p(min_align=-0.1)), b"min_align"),
        (args(params=p(min_align=1.1)), b"min_align"),
        (args(params=p(min_align=math.nan)), b"min_align"),
        (args(up=n), b"up"),
        (args(up=(0.0, 0.0, 0.0)), b"up"),
        (args(up=(0.0, math.nan, 1.0)), b"up"),
        (args(k=0), b"num_approach"),
        (args(k=65), b"num_approach"),
        (args(seeds=n), b"null pointer"),
        (args(outs=(f, f, n, f, f)), b"null pointer"),
        (args(outs=(f,) * 4 + (n,)), b"null pointer"),
        (args(pts=n), b"null pointer"),
        (args(w=n), b"null pointer"),
        (args(nrm=ctypes.c_void_p((1 << 20) + 2)), b"misaligned"),
        (args(ws=n), b"ws"),
        (args(ws=ctypes.c_void_p((1 << 20) + 16)), b"ws"),
    ]
    got = _call_on_thread(lambda a: (lib.gg_grasp_propose(*a), lib.gg_last_error()), [c[0] for c in cases])
    for (st, msg), (_, want) in zip(got, cases):
        assert st == -1 and msg.startswith(b"gg_grasp_propose") and want in msg, msg
    need = lib.gg_grasp_propose_workspace(10, 4)
    (st, msg), = _call_on_thread(lambda a: (lib.gg_grasp_propose(*a), lib.gg_last_error()), [args(ws_bytes=need - 1)])
    assert st == -3 and b"workspace" in msg
    # no seeds: nothing to do, null outputs accepted; 2 clearance == max_width is allowed
    assert lib.gg_grasp_propose(*args(num_seeds=0, seeds=n, outs=(n,) * 5, ws=n, ws_bytes=0,
                                      params=p(clearance=0.05))) == 0


def test_propose_workspace_query():
    from gaussiangrasper_amd import _lib
    ws = _lib.load().gg_grasp_propose_workspace
    assert ws(-1, 5) == 0 and ws(10, -1) == 0 and ws(10, 0) == 0 and ws(10, (1 << 20) + 1) == 0
    assert ws((1 << 30) + 1, 5) == 0
    assert ws(0, 5) > 0 and ws(1, 5) > ws(0, 5)
    assert ws(1_000_000, 16384) >= ws(100_000, 16384) >= ws(1, 16384)
    assert ws(5_000_000, 1 << 20) < 400 << 20 and ws(5_000_000, 4096) < 100 << 20


# ------------------------------------------------------------------------------------------------
# the Python layer without a device
# ------------------------------------------------------------------------------------------------
def test_antipodal_refuses_host_tensors_and_bad_parameters():
    from gaussiangrasper_amd.grasp_propose import antipodal, choose_seeds
    t = (torch.zeros(4, 3), torch.zeros(4, 3), torch.ones(4), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        antipodal(*t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        choose_seeds(torch.ones(4))
    bad = [dict(tube_radius=-1.0), dict(tube_radius=math.nan), dict(max_width=0.0), dict(max_width=math.inf),
           dict(min_width=-0.01), dict(clearance=-0.001), dict(clearance=0.06), dict(depth=-0.01), dict(depth=math.inf),
           dict(height=0.0), dict(height=math.nan), dict(min_weight=math.nan), dict(min_align=-0.5),
           dict(min_align=1.5), dict(min_align=math.nan), dict(up=(0.0, 0.0, 0.0)), dict(up=(0.0, 1.0)),
           dict(up=(math.inf, 0.0, 1.0)), dict(num_approach=0), dict(num_approach=65), dict(num_approach=2.5)]
    for kw in bad:
        with pytest.raises(ValueError, match=next(iter(kw))):
            antipodal(*t, **kw)


def _rot(rng):
    return grasp_ref.rotation(rng, 1)[0]


def test_grasps_from_scene_inverts_grasps_to_scene():
    from gaussiangrasper_amd.grasp import grasps_to_scene
    from gaussiangrasper_amd.grasp_propose import grasps_from_scene
    rng = np.random.default_rng(3)
    m = 50
    g = grasp_ref.grasp_rows(grasp_ref.rotation(rng, m), rng.uniform(-1, 1, (m, 3)), rng.uniform(0.01, 0.1, m),
                             rng.uniform(0.01, 0.05, m), rng.uniform(0.0, 0.04, m), score=rng.random(m), object_id=3)
    C, M = np.eye(4), np.eye(4)
    C[:3, :3], C[:3, 3] = _rot(rng), [0.3, 0.1, -0.2]
    M[:3, :3], M[:3, 3] = _rot(rng), [0.1, -0.2, 0.05]
    for cam, mat, s in ((None, None, 1.0), (C, None, 1.0), (None, M[:3], 2.5), (C, M, 0.4)):
        there = grasps_to_scene(g, cam, mat, s)
        assert np.abs(grasps_from_scene(there, cam, mat, s).astype(np.float64) - g).max() < 1e-6
        back = grasps_from_scene(g, cam, mat, s)
        assert np.abs(grasps_to_scene(back, cam, mat, s).astype(np.float64) - g).max() < 1e-6
    assert np.array_equal(grasps_from_scene(g), g)
    with pytest.raises(ValueError, match="scale"):
        grasps_from_scene(g, scale=0.0)
    with pytest.raises(ValueError, match="matrix"):
        grasps_from_scene(g, matrix=2.0 * np.eye(4))
    with pytest.raises(ValueError, match="17"):
        grasps_from_scene(np.zeros((3, 16)))
    nan_row = np.concatenate([g[:1], np.full((1, 17), np.nan, np.float32)])      # not valid, not an error
    assert np.isnan(grasps_from_scene(nan_row, C, M, 2.0)[1]).all()


def test_cli_argument_errors(tmp_path):
    from gaussiangrasper_amd import grasp_propose
    out = str(tmp_path / "grasps.npy")
    obj = tmp_path / "obj.npy"
    np.save(obj, np.random.default_rng(0).normal(size=(20, 3)))
    base = ["--ckpt", str(tmp_path / "none.ckpt"), "--out", out]
    sel = ["--object-points", str(obj)]
    with pytest.raises(SystemExit):                                   # --out is required
        grasp_propose.main(["--ckpt", "x.ckpt"] + sel)
    with pytest.raises(SystemExit):                                   # a selection is required
        grasp_propose.main(base)
    with pytest.raises(SystemExit):                                   # alternatives
        grasp_propose.main(base + sel + ["--positives", "p.npy", "--negatives", "n.npy", "--threshold", "0.5"])
    with pytest.raises(SystemExit):
        grasp_propose.main(base + ["--positives", "p.npy", "--negatives", "n.npy"])       # no threshold
    with pytest.raises(SystemExit):
        grasp_propose.main(base + sel + ["--threshold", "0.5"])                            # no positives
    for opt, v in (("--mu", "-1"), ("--min-opacity", "nan"), ("--max-collision", "nan"), ("--max-seeds", "0"),
                   ("--num-approach", "0"), ("--num-approach", "65"), ("--max-width", "0"), ("--max-width", "0.009")):
        with pytest.raises(SystemExit):
            grasp_propose.main(base + sel + [opt, v])
    with pytest.raises(SystemExit):
        grasp_propose.main(base + sel + ["--up", "0", "0", "0"])
    (tmp_path / "tj.json").write_text(json.dumps({"scale": 1.0}))
    with pytest.raises(SystemExit, match="transform_matrix"):
        grasp_propose.main(base + sel + ["--transform-json", str(tmp_path / "tj.json")])
    with pytest.raises(SystemExit, match="error"):                    # no such checkpoint
        grasp_propose.main(base + sel)
    assert not (tmp_path / "grasps.npy").exists()
