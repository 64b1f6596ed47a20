"""gg_blend_votes on the GPU: the votes equal the oracle-built reference (tests/lift_ref.py) bit for bit, they
accumulate, they do not depend on the run or on who packed the records; the memory contract of the entry; lift_labels
over several views; and the float-atomic route the entry replaces, to that route's own tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import lift_ref as R
from arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = ctypes.c_void_p
PATTERNS = ("one", "ignored", "checker", "split", "random", "wide", "beyond", "many")


def _lib():
    from gaussiangrasper_amd import _lib
    return _lib.load()


def _stream():
    return P(torch.cuda.current_stream().cuda_stream)


def _err():
    return _lib().gg_last_error().decode("utf-8", "replace")


def _dev(p):
    """the oracle's projection on the device, in the order ops.blend_votes takes it"""
    t = {k: torch.from_numpy(np.ascontiguousarray(p[k])).to(DEV) for k in ("xys", "depths", "radii", "conics", "nth",
                                                                          "opacity")}
    return t["xys"], t["depths"], t["radii"], t["conics"], t["nth"], t["opacity"]


def _votes(p, labels, L, prefill=None, dev=None):
    from gaussiangrasper_amd import ops
    dev = dev or _dev(p)
    n = p["xys"].shape[0]
    votes = torch.zeros(n, L, dtype=torch.int64, device=DEV) if prefill is None else prefill.clone()
    seen = ops.blend_votes(*dev, p["h"], p["w"], torch.from_numpy(labels).to(DEV), votes)
    return seen, votes.cpu().numpy()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", tuple(R.SCENES))
def test_votes_equal_the_reference_bit_for_bit(oracle, name, pattern):
    c = R.case(oracle, name)
    labels, L = R.label_patterns(c.h, c.w, 11)[pattern]
    ref = c.votes(labels, L)
    prefill = None
    if pattern == "ignored":
        prefill = (torch.arange(c.n * L, dtype=torch.int64, device=DEV).reshape(c.n, L) * 7 + 3)
        assert not ref.any()
    seen, got = _votes(c.proj, labels, L, prefill)
    assert seen
    want = ref if prefill is None else ref + prefill.cpu().numpy()
    assert np.array_equal(got, want), (name, pattern, int((got != want).sum()))
    if pattern != "ignored" and name != "S1":
        assert ref.any()


def test_votes_accumulate_over_views(oracle):
    c = R.case(oracle, "D1")
    other = R.project(oracle, R.activated(c.scene), R.ring_cameras(3, c.h, c.w)[2])
    W2, _, _ = R.pixel_weights(oracle, other)
    labels, L = R.label_patterns(c.h, c.w, 5)["random"]
    labels2, _ = R.label_patterns(c.h, c.w, 6)["random"]
    ref1, ref2 = c.votes(labels, L), R.votes_from_q(R.quantise(W2), labels2, L)
    assert ref1.any() and ref2.any() and not np.array_equal(ref1, ref2)
    prefill = 2 ** 40 + torch.arange(c.n * L, dtype=torch.int64, device=DEV).reshape(c.n, L)
    from gaussiangrasper_amd import ops
    votes = prefill.clone()
    assert ops.blend_votes(*_dev(c.proj), c.h, c.w, torch.from_numpy(labels).to(DEV), votes)
    assert ops.blend_votes(*_dev(other), c.h, c.w, torch.from_numpy(labels2).to(DEV), votes)
    assert np.array_equal(votes.cpu().numpy(), prefill.cpu().numpy() + ref1 + ref2)


def test_two_runs_give_the_same_bits(oracle):
    c = R.case(oracle, "D3")
    labels, L = R.label_patterns(c.h, c.w, 11)["random"]
    dev = _dev(c.proj)
    a = _votes(c.proj, labels, L, dev=dev)[1]
    b = _votes(c.proj, labels, L, dev=dev)[1]
    assert a.tobytes() == b.tobytes()


def _lists(p, dev):
    from gaussiangrasper_amd import ops
    bins = ops.bin_and_sort_gaussians(dev[0], dev[1], dev[2], dev[4], p["h"], p["w"], use_cache=False)
    return bins.gaussian_ids_sorted.contiguous(), bins.tile_bins.contiguous(), bins.num_intersects


def test_a_forward_s_workspace_serves_as_packed_records(oracle):
    lib = _lib()
    c = R.case(oracle, "D2")
    labels, L = R.label_patterns(c.h, c.w, 11)["checker"]
    xys, depths, radii, conics, nth, op = dev = _dev(c.proj)
    ids, tile_bins, _ = _lists(c.proj, dev)
    n, h, w = c.n, c.h, c.w
    lab = torch.from_numpy(labels).to(DEV)
    need = lib.gg_blend_workspace(n)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=DEV)
    cols, bg = torch.zeros(n, 1, device=DEV), torch.zeros(1, device=DEV)
    img, ft = torch.empty(h, w, 1, device=DEV), torch.empty(h, w, device=DEV)
    fi = torch.empty(h, w, dtype=torch.int32, device=DEV)
    q = lambda t: P(t.data_ptr())
    assert lib.gg_blend_fwd(1, n, h, w, q(ids), q(tile_bins), q(xys), q(conics), q(cols), q(op), q(bg), q(img), q(ft), q(fi),
                            q(ws), need, _stream()) == 0, _err()
    packed = torch.zeros(n, L, dtype=torch.int64, device=DEV)
    # ws_packed: xys, conics and opacity are not read
    assert lib.gg_blend_votes(L, n, h, w, q(ids), q(tile_bins), None, None, None, q(lab), q(packed), q(ws), need, 1,
                              _stream()) == 0, _err()
    fresh = torch.zeros(n, L, dtype=torch.int64, device=DEV)
    ws2 = torch.full((need,), 0xC3, dtype=torch.uint8, device=DEV)
    assert lib.gg_blend_votes(L, n, h, w, q(ids), q(tile_bins), q(xys), q(conics), q(op), q(lab), q(fresh), q(ws2), need, 0,
                              _stream()) == 0, _err()
    ref = c.votes(labels, L)
    assert np.array_equal(packed.cpu().numpy(), ref) and np.array_equal(fresh.cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------------
# lift_labels
# ------------------------------------------------------------------------------------------------
def test_lift_labels_over_three_views_is_the_sum_of_the_views(oracle):
    """The reference is built from the ORACLE's projection of the same activated parameters (the projection is pinned
    bit-exact), one view at a time; from the second view on the lists are built speculatively."""
    from gaussiangrasper_amd import lift
    n, h, w, _, grow, ob = R.SCENES["D1"]
    sc = R.build_scene(n, grow, ob)
    cams = R.ring(3, h, w)
    act = R.activated(sc, DEV)
    L = 8
    labs, ref, counts = [], np.zeros((n, L), np.int64), np.zeros(L, np.int64)
    for k, cam in enumerate(cams):
        lab = R.label_patterns(h, w, 20 + k)["random"][0]
        W, _, _ = R.pixel_weights(oracle, R.project(oracle, act, R.view_of(cam)))
        ref += R.votes_from_q(R.quantise(W), lab, L)
        counts += np.bincount(lab.reshape(-1), minlength=256)[:L]
        labs.append(lab)
    res = lift.lift_labels(sc.to(DEV), cams, labs, L)
    assert res.views == 3 and np.array_equal(res.pixel_counts, counts)
    assert res.votes.dtype == torch.int64 and res.votes.device.type == "cuda"
    assert np.array_equal(res.votes.cpu().numpy(), ref)
    # torch tensors on the device as label images, and accumulate_view on its own
    votes = torch.zeros(n, L, dtype=torch.int64, device=DEV)
    for cam, lab in zip(cams, labs):
        assert lift.accumulate_view(votes, sc.to(DEV), cam[0], cam[1], h, w, torch.from_numpy(lab).to(DEV))
    assert torch.equal(votes, res.votes)


def test_two_objects_are_selected_as_on_the_host(oracle):
    from gaussiangrasper_amd import lift
    two = R.two_objects(oracle)
    res = lift.lift_labels(two.scene.to(DEV), two.cameras, two.labels, 3)
    for k in (1, 2):
        sel = lift.select(res.votes, k, min_ratio=0.35).cpu().numpy()
        host = lift.select(torch.from_numpy(two.votes), k, min_ratio=0.35).numpy()
        assert np.array_equal(sel, two.member == k) and np.array_equal(sel, host)


def test_nothing_visible_returns_false_and_touches_nothing():
    from gaussiangrasper_amd import ops
    n, h, w = 5, 20, 24
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    votes = torch.arange(n * 2, dtype=torch.int64, device=DEV).reshape(n, 2) + 9
    before = votes.clone()
    seen = ops.blend_votes(z(n, 2), z(n), z(n, dt=torch.int32), z(n, 3), z(n, dt=torch.int32), z(n, 1) + 0.5, h, w,
                           z(h, w, dt=torch.uint8), votes)
    assert seen is False and torch.equal(votes, before)
    assert ops.blend_votes(z(0, 2), z(0), z(0, dt=torch.int32), z(0, 3), z(0, dt=torch.int32), z(0, 1), h, w,
                           z(h, w, dt=torch.uint8), torch.zeros(0, 2, dtype=torch.int64, device=DEV)) is False
    with pytest.raises(ValueError):
        ops.blend_votes(z(n, 2), z(n), z(n, dt=torch.int32), z(n, 3), z(n, dt=torch.int32), z(n, 1), h, w,
                        z(w, h, dt=torch.uint8), votes)
    with pytest.raises(ValueError):
        ops.blend_votes(z(n, 2), z(n), z(n, dt=torch.int32), z(n, 3), z(n, dt=torch.int32), z(n, 1), h, w,
                        z(h, w, dt=torch.uint8), votes.int())


# ------------------------------------------------------------------------------------------------
# memory contract
# ------------------------------------------------------------------------------------------------
def _arena_call(c, ids, tile_bins, labels, L, seed, prefill, n=None, shift=None, null=(), num_labels=None):
    lib = _lib()
    p = c.proj
    n = c.n if n is None else n
    need = lib.gg_blend_workspace(c.n)
    ar = Arena(DEV, seed)
    for name, a in (("ids", ids), ("tile_bins", tile_bins), ("xys", p["xys"]), ("conics", p["conics"]),
                    ("opacity", p["opacity"])):
        ar.carve(name, np.ascontiguousarray(a), 4, "in")
    ar.carve("labels", labels, 1, "in")
    ar.carve("votes", prefill, 8, "inout")
    ar.carve("ws", need, 256, "ws")
    assert ar.address("labels") % 2 == 1 and ar.address("votes") % 16 == 8 and ar.nbytes("votes") == c.n * L * 8

    def q(name):
        if name in null:
            return P(None)
        return P(ar.address(name) + (shift or {}).get(name, 0))
    st = lib.gg_blend_votes(L if num_labels is None else num_labels, n, c.h, c.w, q("ids"), q("tile_bins"), q("xys"),
                            q("conics"), q("opacity"), q("labels"), q("votes"), q("ws"), need, 0, _stream())
    return ar, st


def test_memory_contract(oracle):
    c = R.case(oracle, "D2")
    labels, L = R.label_patterns(c.h, c.w, 11)["random"]
    dev = _dev(c.proj)
    ids, tile_bins, count = _lists(c.proj, dev)
    ids, tile_bins = ids.cpu().numpy()[:count], tile_bins.cpu().numpy()
    prefill = (np.arange(c.n * L, dtype=np.int64).reshape(c.n, L) << 20) + 1
    ref = c.votes(labels, L) + prefill
    runs = []
    for seed in (1, 2):
        ar, st = _arena_call(c, ids, tile_bins, labels, L, seed, prefill)
        assert st == 0, _err()
        out = ar.check()
        assert np.array_equal(out["votes"], ref)
        runs.append(out["votes"].tobytes())
    assert runs[0] == runs[1]
    # num_points == 0: GG_OK, nothing written
    ar, st = _arena_call(c, ids, tile_bins, labels, L, 3, prefill, n=0)
    assert st == 0, _err()
    ar.untouched()
    # empty lists: GG_OK, nothing written but the workspace (the packed records)
    ar, st = _arena_call(c, ids, np.zeros_like(tile_bins), labels, L, 4, prefill)
    assert st == 0, _err()
    assert np.array_equal(ar.check()["votes"], prefill)
    # refused before any launch, the message naming the argument
    for kw, word in ((dict(num_labels=0), "num_labels"), (dict(num_labels=256), "num_labels"),
                     (dict(null=("labels",)), "labels"), (dict(null=("votes",)), "votes"),
                     (dict(shift={"votes": 4}), "votes"), (dict(null=("tile_bins",)), "tile_bins"),
                     (dict(null=("ids",)), "gaussian_ids_sorted"), (dict(null=("xys",)), "xys"),
                     (dict(n=-1), "num_points")):
        ar, st = _arena_call(c, ids, tile_bins, labels, L, 5, prefill, **kw)
        assert st == -1 and word in _err(), (kw, st, _err())
        ar.untouched()


# ------------------------------------------------------------------------------------------------
# the route it replaces: the float-atomic backward under a one-hot cotangent
# ------------------------------------------------------------------------------------------------
def test_votes_match_the_backward_s_colour_gradient():
    """v_colors of NDRasterizeGaussians under v_out = one-hot(labels) against weights(votes): 5e-5 |v| + 1e-6 max |v|
    (the bar of the float-atomic backward against the oracle) plus num_tiles_hit 256 2^-24 (the truncation of at most
    one unit per pixel of the Gaussian's tile box)."""
    from gaussiangrasper_amd import lift, ops
    from gaussiangrasper_amd.scene import make_scene
    n, h, w, L = 20000, 150, 200, 3
    sc = make_scene(n, config_index=1).to(DEV)
    cam = R.ring(3, h, w)[0]
    proj = lift.project_view(sc, cam[0], cam[1], h, w)
    labels = torch.from_numpy(np.random.default_rng(3).integers(0, L, (h, w)).astype(np.uint8)).to(DEV)
    votes = torch.zeros(n, L, dtype=torch.int64, device=DEV)
    assert ops.blend_votes(*proj, h, w, labels, votes)
    xys, depths, radii, conics, nth, op = proj
    colors = torch.rand(n, L, device=DEV, requires_grad=True)
    img = ops.NDRasterizeGaussians.apply(xys, depths, radii, conics, nth, colors, op, h, w, torch.zeros(L, device=DEV))
    img.backward(torch.nn.functional.one_hot(labels.long(), L).float())
    v = colors.grad.double().cpu().numpy()
    got = lift.weights(votes).cpu().numpy()
    tol = 5e-5 * np.abs(v) + 1e-6 * np.abs(v).max() + nth.cpu().numpy()[:, None] * 256 * 2.0 ** -24
    err = np.abs(got - v)
    print(f"max |weights - v_colors| {err.max():.3e}, max of error / allowed {(err / tol).max():.3f}, max |v| {np.abs(v).max():.3f}")
    assert np.abs(v).max() > 1.0
    assert (err <= tol).all()


# ------------------------------------------------------------------------------------------------
# the command line and the text-query route, end to end
# ------------------------------------------------------------------------------------------------
def _write_scan(tmp_path, cameras, h, w):
    """transforms.json with the cameras as OpenCV c2w (the file's convention); the reader flips them back exactly"""
    import objmask_ref
    from gaussiangrasper_amd.mesh import GL_TO_CV
    K = cameras[0][1]
    t = str(tmp_path / "transforms.json")
    objmask_ref.write_transforms(t, [c[0] @ GL_TO_CV for c in cameras], h, w, *K)
    return t


def test_command_line_selects_the_ball_from_mask_files(oracle, tmp_path, capsys):
    from gaussiangrasper_amd import interop, lift
    two = R.two_objects(oracle)
    t = _write_scan(tmp_path, two.cameras, R.TWO_H, R.TWO_W)
    masks = tmp_path / "masks"
    masks.mkdir()
    for stem, lab in zip(lift.frame_stems(t), two.labels):
        np.save(masks / f"{stem}.npy", lab.astype(np.int64))
    ckpt = tmp_path / "step-000029999.ckpt"
    interop.save_checkpoint(str(ckpt), two.scene, None, 29999)
    out = {k: str(tmp_path / f"{k}.npy") for k in ("sel", "votes", "pts")}
    assert lift.main(["--ckpt", str(ckpt), "--transforms", t, "--masks", str(masks), "--label", "2", "--min-ratio", "0.35",
                      "--out", out["sel"], "--out-votes", out["votes"], "--out-points", out["pts"]]) == 0
    assert "150 of 600 Gaussians carry label 2 over 6 views" in capsys.readouterr().out
    sel, votes, pts = (np.load(out[k]) for k in ("sel", "votes", "pts"))
    assert sel.dtype == np.bool_ and np.array_equal(sel, two.member == 2)
    assert votes.dtype == np.int64 and votes.shape == (600, 3)
    assert np.array_equal(sel, lift.select(torch.from_numpy(votes), 2, 0.35).numpy())
    assert pts.dtype == np.float64 and np.array_equal(pts, two.scene.means.numpy()[sel].astype(np.float64))
    # bool masks select label 1: ball 1 alone
    for stem, lab in zip(lift.frame_stems(t), two.labels):
        np.save(masks / f"{stem}.npy", lab == 1)
    assert lift.main(["--ckpt", str(ckpt), "--transforms", t, "--masks", str(masks), "--min-ratio", "0.35",
                      "--out", out["sel"]]) == 0
    assert np.array_equal(np.load(out["sel"]), two.member == 1)


def test_a_text_query_is_decided_in_the_views_and_lifted():
    """query.lift_relevancy = render the features, threshold the relevancy where the alpha sum reaches ALPHA_MIN, lift:
    the same votes as lift_labels on label images made by hand from the same calls."""
    from gaussiangrasper_amd import lift, mesh, ops, query
    n, h, w, _, grow, ob = R.SCENES["D1"]
    sc = R.build_scene(n, grow, ob).to(DEV)
    cams = R.ring(3, h, w)
    g = torch.Generator().manual_seed(5)
    fea_up = tuple(t.to(DEV) for t in (torch.randn(128, 32, generator=g) * 0.2, torch.randn(128, generator=g) * 0.1,
                                       torch.randn(512, 128, generator=g) * 0.1, torch.randn(512, generator=g) * 0.1))
    pos, neg = torch.randn(2, 512, generator=g).numpy(), torch.randn(3, 512, generator=g).numpy()
    thr = 0.5
    labs = []
    for c2w, K, _, _ in cams:
        proj = lift.project_view(sc, c2w, K, h, w)
        img, alpha = ops.rasterize_segments(*proj, h, w, [(sc.feature.contiguous(), torch.zeros(32, device=DEV)),
                                                           (torch.ones(n, 1, device=DEV), torch.zeros(1, device=DEV))])
        rel = query.relevancy(img, fea_up, pos, neg)
        labs.append(((rel > thr).any(dim=-1) & (alpha[..., 0] >= mesh.ALPHA_MIN)).to(torch.uint8))
    ones = sum(int(l.sum()) for l in labs)
    assert 0 < ones < 3 * h * w
    want = lift.lift_labels(sc, cams, labs, 2)
    got = query.lift_relevancy(sc, fea_up, cams, pos, neg, thr)
    assert torch.equal(got.votes, want.votes) and got.views == 3
    assert np.array_equal(got.pixel_counts, want.pixel_counts) and got.pixel_counts[1] == ones
    sel = query.select_gaussians_in_views(sc, fea_up, cams, pos, neg, thr, min_ratio=0.4)
    assert torch.equal(sel, lift.select(want.votes, 1, 0.4)) and 0 < int(sel.sum()) < n
