"""gg_blend_hits on the GPU: all four arrays equal the oracle-built reference (tests/hits_ref.py) on lift_ref's scenes
and on the constructed cases (tests/hits_cases.py); the hit-only build, the packed-workspace route, the memory contract
of the entry; and the layer on top: surface.view_hits / pick / point_cloud / locate and mesh's median depth."""
import ctypes

import numpy as np
import pytest
import torch

import hits_cases as HC
import hits_ref as HR
import lift_ref as R
from arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = ctypes.c_void_p
F = ctypes.c_float


def _lib():
    from gaussiangrasper_amd import _lib
    return _lib.load()


def _stream():
    return P(torch.cuda.current_stream().cuda_stream)


def _err():
    return _lib().gg_last_error().decode("utf-8", "replace")


def _dev(p):
    t = {k: torch.from_numpy(np.ascontiguousarray(p[k])).to(DEV) for k in ("xys", "depths", "radii", "conics", "nth",
                                                                          "opacity")}
    return t["xys"], t["depths"], t["radii"], t["conics"], t["nth"], t["opacity"]


def _same(got, ref, t, full=True):
    hit, top, vis, cnt = (None if a is None else a.cpu().numpy() for a in got)
    assert hit.dtype == np.int32 and np.array_equal(hit, ref.hit[t]), int((hit != ref.hit[t]).sum())
    if full:
        assert top.dtype == np.int32 and vis.dtype == np.float32 and cnt.dtype == np.int32
        assert np.array_equal(top, ref.top_idx), int((top != ref.top_idx).sum())
        assert vis.tobytes() == np.ascontiguousarray(ref.top_vis).tobytes()
        assert np.array_equal(cnt, ref.count), int((cnt != ref.count).sum())
    else:
        assert top is None and vis is None and cnt is None


# ------------------------------------------------------------------------------------------------
# the scenes, through ops.blend_hits
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", HR.THRESHOLDS)
@pytest.mark.parametrize("name", tuple(R.SCENES))
def test_hits_equal_the_reference(oracle, name, t):
    from gaussiangrasper_amd import ops
    c, ref = HR.scene_ref(oracle, name)
    dev = _dev(c.proj)
    _same(ops.blend_hits(*dev, c.h, c.w, t), ref, t)
    _same(ops.blend_hits(*dev, c.h, c.w, t, full=False), ref, t, full=False)


def test_nothing_visible_gives_the_defaults():
    from gaussiangrasper_amd import ops
    h, w = 20, 24
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)   # noqa: E731
    for n in (5, 0):
        hit, top, vis, cnt = ops.blend_hits(z(n, 2), z(n), z(n, dt=torch.int32), z(n, 3), z(n, dt=torch.int32),
                                            z(n, 1) + 0.5, h, w)
        assert hit.shape == (h, w) and bool((hit == -1).all()) and bool((top == -1).all())
        assert bool((vis == 0).all()) and bool((cnt == 0).all())
        hit, top, vis, cnt = ops.blend_hits(z(n, 2), z(n), z(n, dt=torch.int32), z(n, 3), z(n, dt=torch.int32),
                                            z(n, 1) + 0.5, h, w, full=False)
        assert bool((hit == -1).all()) and top is None and vis is None and cnt is None


# ------------------------------------------------------------------------------------------------
# the C entry on hand-made lists, in the sentinel arena
# ------------------------------------------------------------------------------------------------
OUTS = ("hit_idx", "top_idx", "top_vis", "count")


def _arena_call(case, seed, full=True, n=None, t_hit=None, null=(), shift=None, h=None, w=None, ws=None, packed=0):
    """One gg_blend_hits call with every array carved from a sentinel arena: inputs at 4-byte alignment, outputs at
    exactly 4-byte alignment with guards, the workspace seeded garbage (or the bytes `ws` of an earlier call)."""
    lib = _lib()
    n = case.n if n is None else n
    need = lib.gg_blend_workspace(max(case.n, 0))
    ar = Arena(DEV, seed)
    for name, a in (("ids", case.ids), ("tile_bins", case.tile_bins), ("xys", case.xys), ("conics", case.conics),
                    ("opacity", case.opacity)):
        ar.carve(name, np.ascontiguousarray(a), 4, "in")
    ar.carve("hit_idx", np.zeros((case.h, case.w), np.int32), 4, "out")
    ar.carve("top_idx", np.zeros((case.h, case.w), np.int32), 4, "out")
    ar.carve("top_vis", np.zeros((case.h, case.w), np.float32), 4, "out")
    ar.carve("count", np.zeros((case.h, case.w), np.int32), 4, "out")
    if ws is None:
        ar.carve("ws", need, 256, "ws")
    else:
        ar.carve("ws", ws, 256, "inout")
    for o in OUTS:
        assert ar.address(o) % 8 == 4

    def q(name):
        if name in null or (not full and name in OUTS[1:]):
            return P(None)
        return P(ar.address(name) + (shift or {}).get(name, 0))
    st = lib.gg_blend_hits(n, case.h if h is None else h, case.w if w is None else w, q("ids"), q("tile_bins"), q("xys"),
                           q("conics"), q("opacity"), F(case.t_hit if t_hit is None else t_hit), q("hit_idx"),
                           q("top_idx"), q("top_vis"), q("count"), q("ws"), need, packed, _stream())
    return ar, st


def _check_outputs(ar, out, ref, t, full):
    assert np.array_equal(out["hit_idx"], ref.hit[t]), int((out["hit_idx"] != ref.hit[t]).sum())
    if full:
        assert np.array_equal(out["top_idx"], ref.top_idx)
        assert out["top_vis"].tobytes() == np.ascontiguousarray(ref.top_vis).tobytes()
        assert np.array_equal(out["count"], ref.count)
    else:
        for o in OUTS[1:]:
            assert out[o].tobytes() == ar.sentinel_like(o).tobytes()


@pytest.mark.parametrize("name", HC.NAMES)
def test_constructed_cases(oracle, name):
    case = HC.cases()[name]
    ref = HR.case_ref(oracle, case)
    for full in (True, False):
        ar, st = _arena_call(case, 7, full)
        assert st == 0, _err()
        _check_outputs(ar, ar.check(), ref, case.t_hit, full)


def test_memory_contract(oracle):
    case = HC.cases()["empty_between"]
    ref = HR.case_ref(oracle, case)
    for full in (True, False):
        runs = []
        for seed in (1, 2):          # the workspace is garbage on entry, and different garbage each time
            ar, st = _arena_call(case, seed, full)
            assert st == 0, _err()
            out = ar.check()         # inputs and guards unchanged
            _check_outputs(ar, out, ref, case.t_hit, full)
            runs.append(b"".join(out[o].tobytes() for o in OUTS))
        assert runs[0] == runs[1]
    # num_points == 0 writes the defaults; the lists are not read (here they name Gaussians that do not exist)
    ar, st = _arena_call(case, 3, n=0)
    assert st == 0, _err()
    out = ar.check()
    assert (out["hit_idx"] == -1).all() and (out["top_idx"] == -1).all()
    assert (out["top_vis"] == 0).all() and (out["count"] == 0).all()
    assert out["ws"].tobytes() == ar.before("ws").tobytes()
    # refused before any launch, the message naming the argument: nothing is written
    for kw, word in ((dict(t_hit=1.0), "t_hit"), (dict(t_hit=1e-4), "t_hit"), (dict(t_hit=0.0), "t_hit"),
                     (dict(t_hit=float("nan")), "t_hit"), (dict(null=("hit_idx",)), "hit_idx"),
                     (dict(null=("top_vis",)), "top_idx, top_vis and count"),
                     (dict(null=("top_idx", "count")), "top_idx, top_vis and count"),
                     (dict(shift={"hit_idx": 2}), "hit_idx"), (dict(shift={"top_idx": 1}), "top_idx"),
                     (dict(shift={"top_vis": 2}), "top_vis"), (dict(shift={"count": 3}), "count"),
                     (dict(null=("tile_bins",)), "tile_bins"), (dict(null=("ids",)), "gaussian_ids_sorted"),
                     (dict(null=("xys",)), "xys"), (dict(n=-1), "num_points"), (dict(h=0), "img_height"),
                     (dict(w=-3), "img_width")):
        ar, st = _arena_call(case, 5, **kw)
        assert st == -1 and word in _err(), (kw, st, _err())
        ar.untouched()


def test_a_forward_s_workspace_serves_as_packed_records(oracle):
    """ws_packed = 1 on the workspace a gg_blend_fwd over the same Gaussians left: xys, conics and opacity are not
    read, the outputs are the same bytes."""
    lib = _lib()
    case = HC.cases()["four_quadrants"]
    ref = HR.case_ref(oracle, case)
    n, h, w = case.n, case.h, case.w
    need = lib.gg_blend_workspace(n)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    ids, bins, xys, conics, op = t(case.ids), t(case.tile_bins), t(case.xys), t(case.conics), t(case.opacity)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=DEV)
    cols, bg = torch.zeros(n, 1, device=DEV), torch.zeros(1, device=DEV)
    img, ft = torch.empty(h, w, 1, device=DEV), torch.empty(h, w, device=DEV)
    fi = torch.empty(h, w, dtype=torch.int32, device=DEV)
    q = lambda x: P(x.data_ptr())   # noqa: E731
    assert lib.gg_blend_fwd(1, n, h, w, q(ids), q(bins), q(xys), q(conics), q(cols), q(op), q(bg), q(img), q(ft), q(fi),
                            q(ws), need, _stream()) == 0, _err()
    assert ft.cpu().numpy().tobytes() == np.ascontiguousarray(ref.final_T).tobytes()
    torch.cuda.synchronize()
    ar, st = _arena_call(case, 9, null=("xys", "conics", "opacity"), ws=ws.cpu().numpy(), packed=1)
    assert st == 0, _err()
    packed = ar.check()
    ar2, st = _arena_call(case, 10)
    assert st == 0, _err()
    fresh = ar2.check()
    _check_outputs(ar, packed, ref, case.t_hit, True)
    for o in OUTS:
        assert packed[o].tobytes() == fresh[o].tobytes()
    assert packed["ws"].tobytes() == ws.cpu().numpy().tobytes()       # the records are read, not rewritten


def test_a_one_pixel_image(oracle):
    c = HC.Case("one_pixel", 1, 1, 0.5, (0, 0), 2)
    c.stack(0, 0, 0, HC.WIDE, [0.4, 0.4, 0.4]).finish()
    ref = HR.Ref(oracle, c.ids, c.tile_bins, c.xys, c.conics, c.opacity, 1, 1, (0.5,))
    assert int(ref.pos[0.5][0, 0]) == 2 and int(ref.count[0, 0]) == 3
    for full in (True, False):
        ar, st = _arena_call(c, 11, full)
        assert st == 0, _err()
        _check_outputs(ar, ar.check(), ref, 0.5, full)


# ------------------------------------------------------------------------------------------------
# surface
# ------------------------------------------------------------------------------------------------
def _d1():
    n, h, w, _, grow, ob = R.SCENES["D1"]
    return R.build_scene(n, grow, ob).to(DEV), R.ring(3, h, w), h, w


def _restate_points(depth, c2w, K):
    """numpy fp64 back-projection of the pixel centres (mesh / prepare convention), NaN without a hit"""
    fx, fy, cx, cy = K
    h, w = depth.shape
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    z = depth.astype(np.float64)
    with np.errstate(invalid="ignore"):                  # 0 * inf where there is no hit: overwritten below
        cam = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z, np.ones_like(z)], axis=-1)
        world = cam @ (np.asarray(c2w, np.float64) @ np.diag([1.0, -1.0, -1.0, 1.0])).T
    world = world[..., :3]
    world[~np.isfinite(z)] = np.nan
    return world


def test_view_hits_depth_points_and_normals():
    from gaussiangrasper_amd import lift, ops, surface
    sc, cams, h, w = _d1()
    c2w, K, _, _ = cams[1]
    hits = surface.view_hits(sc, c2w, K, h, w)
    proj = lift.project_view(sc, c2w, K, h, w)
    raw = ops.blend_hits(*proj, h, w, 0.5)
    for a, b in zip((hits.hit_idx, hits.top_idx, hits.top_vis, hits.count), raw):
        assert torch.equal(a, b)
    hit = hits.hit_idx.cpu().numpy()
    ok = hit >= 0
    assert 0 < ok.sum() < h * w
    depths = proj[1].cpu().numpy()
    depth = hits.depth.cpu().numpy()
    want = np.where(ok, depths[np.clip(hit, 0, None)], np.float32(np.inf)).astype(np.float32)
    assert depth.dtype == np.float32 and depth.tobytes() == want.tobytes()
    pts = hits.points.cpu().numpy()
    ref = _restate_points(depth, c2w, K)
    assert pts.dtype == np.float32 and np.array_equal(np.isnan(pts), np.isnan(ref))
    ulp = np.spacing(np.abs(ref[ok]).astype(np.float32)).astype(np.float64)
    err = np.abs(pts[ok].astype(np.float64) - ref[ok])
    print(f"points: max error {np.max(err / ulp):.3f} ulp over {int(ok.sum())} hit pixels")
    assert (err <= ulp).all()
    nrm = hits.normals.cpu().numpy()
    assert np.isnan(nrm[~ok]).all() and np.isfinite(nrm[ok]).all()
    assert np.allclose(np.linalg.norm(nrm[ok].astype(np.float64), axis=-1), 1.0, atol=1e-5)
    to_cam = np.asarray(c2w, np.float64)[:3, 3] - pts[ok].astype(np.float64)
    dot = (nrm[ok].astype(np.float64) * to_cam).sum(axis=-1)
    # the flip is decided on the fp64 dot product of these fp32 values; its rounding error is below 4 * 2^-53 |d|
    assert (dot >= -1e-15 * np.linalg.norm(to_cam, axis=-1)).all()
    # full=False: the same hits, nothing else
    lean = surface.view_hits(sc, c2w, K, h, w, full=False)
    assert torch.equal(lean.hit_idx, hits.hit_idx) and lean.top_idx is None and lean.count is None
    assert lean.depth.cpu().numpy().tobytes() == depth.tobytes()
    # a mask walks the selected Gaussians only; ids index the whole model
    from gaussiangrasper_amd.scene import Scene
    mask = torch.arange(sc.means.shape[0], device=DEV) % 3 != 0
    sub = Scene(*(t[mask] for t in (sc.means, sc.scales, sc.quats, sc.opacities, sc.colors_all, sc.feature)))
    index = torch.nonzero(mask).reshape(-1).to(torch.int32)
    sub_hits = surface.view_hits(sub, c2w, K, h, w)
    masked = surface.view_hits(sc, c2w, K, h, w, mask=mask)
    for a, b in ((masked.hit_idx, sub_hits.hit_idx), (masked.top_idx, sub_hits.top_idx)):
        assert torch.equal(a, torch.where(b >= 0, index[b.clamp_min(0).long()], b))
    assert bool((sub_hits.hit_idx >= 0).any()) and torch.equal(masked.count, sub_hits.count)
    assert masked.depth.cpu().numpy().tobytes() == sub_hits.depth.cpu().numpy().tobytes()


def test_pick_returns_the_view_s_hits(oracle):
    from gaussiangrasper_amd import cluster, surface
    sc, cams, h, w = _d1()
    hits = surface.view_hits(sc, *cams[1])
    hit = hits.hit_idx.cpu().numpy()
    yy, xx = np.nonzero(hit >= 0)
    my, mx = np.nonzero(hit < 0)
    px = np.array([[xx[0], yy[0]], [mx[0], my[0]], [xx[-1], yy[-1]], [0, 0], [w - 1, h - 1]])
    ids, pts = surface.pick(sc, cams[1], px)
    assert ids.dtype == torch.int32 and ids.cpu().tolist() == [int(hit[v, u]) for u, v in px]
    want = hits.points.cpu().numpy()[px[:, 1], px[:, 0]]
    assert pts.cpu().numpy().tobytes() == want.tobytes()
    assert int(ids[1]) == -1 and np.isnan(pts[1].cpu().numpy()).all()
    # the clicked instance: two instances by hand, the rest noise
    n = sc.means.shape[0]
    g = int(ids[0])
    inst = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    inst[: n // 2] = 1
    inst[g] = 0
    cent = torch.stack([pts[0].double() + 5.0, pts[0].double()]).to(DEV)
    stats = cluster.ClusterStats(torch.tensor([1, n // 2], device=DEV), torch.ones(2, dtype=torch.float64, device=DEV),
                                 cent, torch.zeros(2, 6, device=DEV))
    instances = cluster.Instances(inst, torch.arange(2, device=DEV), stats)
    m = surface.pick_instance(sc, cams[1], px[0], instances)
    assert m.dtype == torch.bool and int(m.sum()) == 1 and bool(m[g])
    inst[g] = -1          # noise: the instance whose centroid is nearest to the hit point
    m = surface.pick_instance(sc, cams[1], px[0], cluster.Instances(inst, torch.arange(2, device=DEV), stats))
    assert torch.equal(m, inst == 1)
    with pytest.raises(ValueError, match="nothing is under"):
        surface.pick_instance(sc, cams[1], px[1], instances)


def test_point_cloud_over_three_views():
    from gaussiangrasper_amd import mesh, surface
    sc, cams, h, w = _d1()
    per_view = [surface.view_hits(sc, *c, full=False) for c in cams]
    counts = [int((v.hit_idx >= 0).sum()) for v in per_view]
    pts, nrm, col, ids = surface.point_cloud(sc, cams)
    assert pts.shape == (sum(counts), 3) and nrm.shape == pts.shape and col.shape == pts.shape
    assert ids.shape == (sum(counts),) and ids.dtype == torch.int32 and min(counts) > 0
    assert bool(torch.isfinite(pts).all()) and bool(torch.isfinite(nrm).all())
    assert bool((col >= 0).all()) and bool((col <= 1).all())
    # view-major, then row-major
    k0 = per_view[0].hit_idx >= 0
    assert torch.equal(ids[:counts[0]], per_view[0].hit_idx[k0]) and torch.equal(pts[:counts[0]], per_view[0].points[k0])
    k2 = per_view[2].hit_idx >= 0
    assert torch.equal(ids[-counts[2]:], per_view[2].hit_idx[k2])
    rgb = mesh.render_depth(sc, *cams[0])[1]
    assert torch.equal(col[:counts[0]], rgb[k0])
    s_pts, _, _, s_ids = surface.point_cloud(sc, cams[:1], stride=3)
    assert torch.equal(s_ids, per_view[0].hit_idx[::3, ::3][k0[::3, ::3]]) and s_pts.shape[0] == s_ids.shape[0]


def test_median_depth_has_no_skirt_between_two_layers():
    from gaussiangrasper_amd import lift, mesh
    sc, cam, is_plate = HC.two_layer_scene()
    sc = sc.to(DEV)
    c2w, K, h, w = cam
    plain = mesh.render_depth(sc, c2w, K, h, w)
    expected = mesh.render_depth(sc, c2w, K, h, w, depth_mode="expected")
    for a, b in zip(plain, expected):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    e = expected[0].cpu().numpy()
    between = (e > 1.1) & (e < 1.9)
    print(f"expected depth in (1.1, 1.9) at {int(between.sum())} pixels")
    assert between.sum() >= 1                                   # the fixture can see the feature
    median = mesh.render_depth(sc, c2w, K, h, w, depth_mode="median")
    m = median[0].cpu().numpy()
    depths = lift.project_view(sc, c2w, K, h, w)[1].cpu().numpy()
    finite = np.isfinite(m)
    assert finite.mean() > 0.9 and np.isin(m[finite], depths).all()
    near_plate, near_wall = np.abs(m - HC.PLATE_Z) < 1e-5, np.abs(m - HC.WALL_Z) < 1e-5
    assert (near_plate | near_wall)[finite].all() and near_plate.any() and near_wall.any()
    assert np.isin(m[near_plate], depths[is_plate]).all() and np.isin(m[near_wall], depths[~is_plate]).all()
    assert (m[~finite] == np.inf).all()
    for a, b in zip(median[1:], expected[1:]):                   # colour and alpha do not depend on the mode
        assert torch.equal(a, b)
    # through mesh_model: the median volume builds, and the default is the expected depth
    bbox = ((-0.8, -0.6, -2.3), (0.8, 0.6, -0.7))
    a = mesh.mesh_model(sc, [cam], bbox, 32, downscale=1, color=False, depth_mode="median")
    assert len(a.faces) > 0


def test_locate_finds_the_queried_ball():
    """lift_ref's two balls on a table, with features that say where on its ball a Gaussian sits:
    feature = e_object + (mean - centre) / radius . (e_x, e_y, e_z), nine orthonormal directions apart, and a fea_up that
    is an isometry (relu(x) - relu(-x) = x, then 512 orthonormal columns), so the similarity of a pixel to a query is
    the cosine of their features.  The query names the spot of the ball that faces camera 0: e_ball + d0 . (e_x, e_y,
    e_z), d0 the unit vector from the ball's centre to that camera.  The best pixel is then the one whose ray runs
    through the ball's centre in view 0, and a point of that ray at the depth of a Gaussian of the ball is within one
    radius of the centre.  Temperature 1 keeps the relevancy off the sigmoid's plateau.

    (With one constant feature per object the relevancy is the same number, bit for bit, over most of the ball; the
    pixel taken from that plateau is arbitrary, and the hit points of 60 % of the ball's pixels in view 0 lie beyond one
    radius from the centre — up to 0.22 — because a hit point has the depth of its Gaussian's centre but the pixel's
    own ray: such a query landed 0.168 from the centre.)"""
    from gaussiangrasper_amd import surface
    sc, member = R.two_object_scene()
    rng = np.random.default_rng(11)
    E = np.linalg.qr(rng.normal(size=(32, 6)))[0].T.astype(np.float32)      # table, ball 1, ball 2, e_x, e_y, e_z
    Pm = torch.from_numpy(np.linalg.qr(rng.normal(size=(512, 32)))[0].astype(np.float32))
    radius, centres = 0.15, {1: np.array([-0.35, 0.0, 0.0]), 2: np.array([0.35, 0.0, 0.0])}
    means = sc.means.numpy()
    feat = E[member].copy()
    for k, c in centres.items():
        feat[member == k] += ((means[member == k] - c) / radius).astype(np.float32) @ E[3:6]
    sc.feature = torch.from_numpy(feat).contiguous()
    eye = torch.eye(32)
    w1 = torch.cat([eye, -eye, torch.zeros(64, 32)])
    w2 = torch.cat([Pm, -Pm, torch.zeros(512, 64)], dim=1)
    fea_up = tuple(t.contiguous().to(DEV) for t in (w1, torch.zeros(128), w2, torch.zeros(512)))
    cams = R.ring(R.TWO_VIEWS, R.TWO_H, R.TWO_W)
    dev_scene = sc.to(DEV)
    for ball, centre in centres.items():
        d0 = cams[0][0][:3, 3] - centre
        d0 /= np.linalg.norm(d0)
        pos = ((E[ball] + d0.astype(np.float32) @ E[3:6]) @ Pm.numpy().T)[None]
        neg = np.stack([E[0], E[3 - ball]]) @ Pm.numpy().T
        point, view, (u, v), rel = surface.locate(dev_scene, cams, pos, neg, fea_up, temperature=1.0)
        p = point.double().cpu().numpy()
        d, spot = float(np.linalg.norm(p - centre)), float(np.linalg.norm(p - (centre + radius * d0)))
        print(f"ball {ball}: view {view}, pixel ({u}, {v}), relevancy {rel:.6f}, {d:.4f} from the centre, {spot:.4f} "
              f"from the spot")
        assert 0 <= view < len(cams) and 0 <= u < R.TWO_W and 0 <= v < R.TWO_H and 0.5 < rel <= 1.0
        assert point.dtype == torch.float32 and point.shape == (3,)
        assert d <= radius                                     # one ball radius


# ------------------------------------------------------------------------------------------------
# the command line, end to end
# ------------------------------------------------------------------------------------------------
def test_command_line_writes_the_cloud_and_the_picks(tmp_path, capsys):
    import json
    import objmask_ref
    from gaussiangrasper_amd import interop, mesh, surface
    sc, _ = R.two_object_scene()
    cams = R.ring(3, R.TWO_H, R.TWO_W)
    t = str(tmp_path / "transforms.json")
    objmask_ref.write_transforms(t, [c[0] @ mesh.GL_TO_CV for c in cams], R.TWO_H, R.TWO_W, *cams[0][1])
    ckpt = tmp_path / "step-000029999.ckpt"
    interop.save_checkpoint(str(ckpt), sc, None, 29999)
    dev_scene = sc.to(DEV)
    pts, nrm, col, ids = surface.point_cloud(dev_scene, cams, stride=2)
    hit = surface.view_hits(dev_scene, *cams[1], full=False).hit_idx.cpu().numpy()
    (v1, u1), (v0, u0) = np.argwhere(hit >= 0)[0], np.argwhere(hit < 0)[0]
    out, picks = str(tmp_path / "cloud.ply"), str(tmp_path / "picks.json")
    assert surface.main(["--ckpt", str(ckpt), "--transforms", t, "--out", out, "--stride", "2", "--pick", "1", str(u1),
                         str(v1), "1", str(u0), str(v0), "--out-pick", picks]) == 0
    said = capsys.readouterr().out
    assert f"{pts.shape[0]} points of 3 views" in said and "1 of 2 picks hit" in said
    m = mesh.read_ply_mesh(out)
    assert len(m.faces) == 0 and m.vertices.tobytes() == pts.cpu().numpy().tobytes()
    assert m.normals.tobytes() == nrm.cpu().numpy().tobytes()
    assert np.abs(m.colors - col.cpu().numpy()).max() <= 0.5 / 255 + 1e-6
    with open(picks) as f:
        rows = json.load(f)
    want_ids, want_pts = surface.pick(dev_scene, cams[1], [[u1, v1]])
    assert rows[0] == {"view": 1, "pixel": [int(u1), int(v1)], "gaussian": int(want_ids[0]),
                       "point": [float(x) for x in want_pts[0].double().cpu().numpy()]}
    assert rows[1] == {"view": 1, "pixel": [int(u0), int(v0)], "gaussian": -1, "point": None}
    # a pick outside the image is refused before the checkpoint is read
    assert surface.main(["--ckpt", str(tmp_path / "none.ckpt"), "--transforms", t, "--pick", "0", str(R.TWO_W), "0",
                         "--out-pick", picks]) == 2
    assert "outside" in capsys.readouterr().err
