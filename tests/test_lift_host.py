"""Mask lifting on the host: the reference votes (tests/lift_ref.py) against two independent statements of the same
sums, the pure functions of a vote array, the argument checks and the command lines.  No GPU."""
import os

import numpy as np
import pytest
import torch

import lift_ref as R
from gaussiangrasper_amd import _cli, lift

NAMES = tuple(R.SCENES)


# ------------------------------------------------------------------------------------------------
# the reference against the forward's own transmittance, and against the oracle's backward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_votes_conserve_the_blended_weight(oracle, name):
    """sum of the votes of a pixel = 1 - final_T of that pixel, up to the truncation of every pair (< 2^-24 each) and
    the fp32 rounding of the T product (<= 2^-24 per list entry walked, T <= 1)."""
    c = R.case(oracle, name)
    labels, L = R.label_patterns(c.h, c.w, 11)["random"]
    counted = labels < L
    votes = c.votes(labels, L)
    lens = (c.bins["tile_bins"][:, 1] - c.bins["tile_bins"][:, 0]).astype(np.int64)
    tiles_x = (c.w + 15) // 16
    yy, xx = np.mgrid[0:c.h, 0:c.w]
    list_len = lens[(yy // 16) * tiles_x + xx // 16]
    pairs = int((c.W[counted] > 0).sum())
    lhs = votes.sum() / 2.0 ** 24
    rhs = (1.0 - c.final_T.astype(np.float64))[counted].sum()
    bound = (pairs + int(list_len[counted].sum())) * 2.0 ** -24
    print(f"{name}: sum votes {lhs:.9f}  sum (1 - T) {rhs:.9f}  |diff| {abs(lhs - rhs):.3e}  bound {bound:.3e}")
    assert pairs > 0
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("name", NAMES)
def test_votes_are_the_backward_s_colour_gradient_of_a_one_hot_cotangent(oracle, name):
    """v_colors[g, l] of the oracle's fp64 backward under v_out = one-hot(labels) is sum over the pixels of label l of
    vis(p, g): the votes without the truncation (< 2^-24 for each of the m_g pixels that blend g) and with fp64
    instead of fp32 rounding of alpha T (1e-6 relative)."""
    O = oracle
    c = R.case(O, name)
    labels, L = R.label_patterns(c.h, c.w, 11)["random"]
    p = c.proj
    b = c.bins
    cols, bg = np.zeros((c.n, L)), np.zeros(L)
    _, ft, fi = O.blend_fwd(b["gaussian_ids_sorted"], b["tile_bins"], p["xys"], p["conics"], cols, p["opacity"], c.h, c.w,
                            bg, dtype=np.float64)
    v_out = np.zeros((c.h, c.w, L))
    for l in range(L):
        v_out[..., l] = labels == l
    v_colors = O.blend_bwd(b["gaussian_ids_sorted"], b["tile_bins"], p["xys"], p["conics"], cols, p["opacity"], c.h, c.w,
                           bg, ft, fi, v_out, dtype=np.float64)[2]
    w = c.votes(labels, L) / 2.0 ** 24
    m = (c.W > 0).reshape(-1, c.n).sum(axis=0)
    tol = m[:, None] * 2.0 ** -24 + 1e-6 * np.abs(v_colors)
    err = np.abs(w - v_colors)
    print(f"{name}: max |votes / 2^24 - v_colors| {err.max():.3e}, max of error / allowed {(err / np.maximum(tol, 1e-300)).max():.3f}")
    assert (err <= tol).all()


# ------------------------------------------------------------------------------------------------
# select / assign
# ------------------------------------------------------------------------------------------------
U = 2 ** 24


def test_weights_are_exact_below_2_53():
    v = torch.tensor([[0, 1, U, 2 ** 53 - 1]], dtype=torch.int64)
    w = lift.weights(v)
    assert w.dtype == torch.float64
    assert w[0].tolist() == [0.0, 2.0 ** -24, 1.0, (2 ** 53 - 1) / 2.0 ** 24]
    assert lift.weights(v.numpy()).equal(w)


def test_select_limits_are_inclusive_and_exact():
    v = torch.tensor([[3 * U, 1 * U],          # ratio 0.25 exactly
                      [1 * U, 1 * U],          # 0.5
                      [0, 0],                  # nothing saw it
                      [0, 5],                  # all of a tiny weight
                      [U, U - 1],              # one unit below half
                      [7, 0]], dtype=torch.int64)
    assert lift.select(v, 1, 0.25).tolist() == [True, True, False, True, True, False]
    assert lift.select(v, 1, 0.5).tolist() == [False, True, False, True, False, False]
    assert lift.select(v, 1, 0.5, min_weight=1.0).tolist() == [False, True, False, False, False, False]
    assert lift.select(v, 1, 0.25, min_weight=1.0).tolist() == [True, True, False, False, False, False]
    assert lift.select(v, 1, 0.0, min_weight=5 * 2.0 ** -24).tolist() == [True, True, False, True, True, False]
    assert lift.select(v, 0, 1.0).tolist() == [False, False, False, False, False, True]
    assert lift.select(v, 1, 0.0).tolist() == [True, True, False, True, True, True]     # 0 >= 0 * total, total > 0
    assert lift.select(v.numpy(), 1, 0.5).tolist() == lift.select(v, 1, 0.5).tolist()
    assert lift.select(lift.Votes(v, 1, np.zeros(2, np.int64))).tolist() == lift.select(v, 1, 0.5).tolist()
    for bad in (dict(label=2), dict(label=-1), dict(min_ratio=1.5), dict(min_ratio=float("nan")), dict(min_weight=-1.0)):
        with pytest.raises(ValueError):
            lift.select(v, **bad)
    with pytest.raises(ValueError):
        lift.select(v.float())


def test_assign_takes_the_largest_label_and_breaks_ties_downwards():
    v = torch.tensor([[2 * U, 2 * U, 0],       # tie of 0 and 1 -> 0 (ratio 0.5 each)
                      [0, 0, 0],               # none
                      [1 * U, 3 * U, 0],       # 1 at 0.75
                      [U, U, U],               # three-way tie at 1/3
                      [0, 3, 3],               # tie of 1 and 2
                      [2 * U, U, U]], dtype=torch.int64)
    a = lift.assign(v, 0.5)
    assert a.dtype == torch.int32 and a.tolist() == [0, -1, 1, -1, 1, 0]
    assert lift.assign(v, 1.0 / 3.0).tolist()[3] in (0, -1)          # 1/3 in float64 times 3 U: whichever way it rounds
    assert lift.assign(v, 0.25).tolist() == [0, -1, 1, 0, 1, 0]
    assert lift.assign(v, 0.5, min_weight=2.5).tolist() == [-1, -1, 1, -1, -1, -1]
    assert lift.assign(v, 0.5, min_weight=2.0).tolist() == [0, -1, 1, -1, -1, 0]
    assert lift.assign(torch.zeros(0, 3, dtype=torch.int64)).shape == (0,)
    # assign agrees with select label by label
    for l in range(3):
        sel = lift.select(v, l, 0.5)
        assert ((a == l) <= sel).all()


# ------------------------------------------------------------------------------------------------
# two objects on a table
# ------------------------------------------------------------------------------------------------
def test_two_objects_are_recovered_exactly(oracle):
    """Lifting the per-view labels of two balls on a table recovers both balls exactly at min_ratio 0.35.  The vote
    ratios of this scene: members at least 0.5264 / 0.5383, everything else at most 0.1512 / 0.1614."""
    two = R.two_objects(oracle)
    v = torch.from_numpy(two.votes)
    w = lift.weights(v).numpy()
    total = w.sum(axis=1)
    assert (total[two.member > 0] > 0).all()
    for k, lo, hi in ((1, 0.526, 0.152), (2, 0.538, 0.162)):
        member = two.member == k
        sel = lift.select(v, k, min_ratio=0.35).numpy()
        tp = int((sel & member).sum())
        precision, recall = tp / max(int(sel.sum()), 1), tp / int(member.sum())
        ratio = w[:, k] / np.where(total > 0, total, 1.0)
        print(f"ball {k}: precision {precision} recall {recall}  member ratios >= {ratio[member].min():.4f}  "
              f"others <= {ratio[~member].max():.4f}")
        assert precision == 1.0 and recall == 1.0
        assert ratio[member].min() >= lo
        assert ratio[~member].max() <= hi
    a = lift.assign(v, 0.35).numpy()
    assert ((a == 1) == (two.member == 1)).all() and ((a == 2) == (two.member == 2)).all()


# ------------------------------------------------------------------------------------------------
# argument checks and command lines
# ------------------------------------------------------------------------------------------------
class _Src:
    means = torch.zeros(4, 3)


CAM = (np.eye(4), (20.0, 20.0, 8.0, 6.0), 12, 16)


def test_lift_labels_refuses_bad_label_images_before_anything_runs():
    ok = np.zeros((12, 16), np.uint8)
    with pytest.raises(ValueError, match=r"expected \(12, 16\)"):
        lift.lift_labels(_Src(), [CAM], [np.zeros((16, 12), np.uint8)], 2)
    bad = ok.copy()
    bad[3, 4] = 2
    with pytest.raises(ValueError, match="label 2 is neither below num_labels = 2"):
        lift.lift_labels(_Src(), [CAM], [bad], 2)
    bad[3, 4] = 254
    with pytest.raises(ValueError, match="label 254"):
        lift.lift_labels(_Src(), [CAM, CAM], [ok, bad], 254)
    with pytest.raises(ValueError, match="integers or bool"):
        lift.lift_labels(_Src(), [CAM], [ok.astype(np.float32)], 2)
    with pytest.raises(ValueError, match=r"\[0, 255\]"):
        lift.lift_labels(_Src(), [CAM], [ok.astype(np.int32) - 1], 2)
    with pytest.raises(ValueError, match="1 cameras but 2"):
        lift.lift_labels(_Src(), [CAM], [ok, ok], 2)
    for L in (0, 256):
        with pytest.raises(ValueError, match="num_labels"):
            lift.lift_labels(_Src(), [CAM], [ok], L)
    # a good call gets as far as asking for a HIP device: there is no CPU fallback
    ign = ok.copy()
    ign[0, 0] = 255
    with pytest.raises(RuntimeError, match="HIP device"):
        lift.lift_labels(_Src(), [CAM], [ign], 2)


def _scan(tmp_path, frames=2):
    import objmask_ref
    t = str(tmp_path / "transforms.json")
    objmask_ref.write_transforms(t, objmask_ref.ring(frames), 12, 16, 20.0, 20.0, 8.0, 6.0)
    masks = tmp_path / "masks"
    masks.mkdir()
    return t, str(masks)


def test_mask_files(tmp_path):
    from PIL import Image
    t, masks = _scan(tmp_path)
    assert lift.frame_stems(t) == ["frame_0000", "frame_0001"]
    ids = np.arange(12 * 16).reshape(12, 16) % 3
    ids[0, 0] = 255
    np.save(os.path.join(masks, "frame_0000.npy"), ids)
    img = np.zeros((12, 16), np.uint8)
    img[2:5, 3:9] = 200
    Image.fromarray(img).save(os.path.join(masks, "frame_0001.png"))
    a = lift.read_label_image(lift.find_mask(masks, "frame_0000"))
    assert a.dtype == np.uint8 and np.array_equal(a, ids)
    b = lift.read_label_image(lift.find_mask(masks, "frame_0001"))
    assert b.dtype == np.uint8 and np.array_equal(b, (img != 0).astype(np.uint8))
    np.save(os.path.join(masks, "bools.npy"), img != 0)
    assert np.array_equal(lift.read_label_image(os.path.join(masks, "bools.npy")), b)
    np.save(os.path.join(masks, "big.npy"), ids + 300)
    with pytest.raises(ValueError, match=r"\[0, 255\]"):
        lift.read_label_image(os.path.join(masks, "big.npy"))
    with pytest.raises(ValueError, match="no mask for frame 'frame_0007'"):
        lift.find_mask(masks, "frame_0007")


def test_command_line_refuses_before_it_loads_anything(tmp_path, capsys):
    t, masks = _scan(tmp_path)
    base = ["--ckpt", str(tmp_path / "none.ckpt"), "--transforms", t, "--out", str(tmp_path / "sel.npy")]
    emb = str(tmp_path / "e.npy")
    groups = ([],                                                     # neither source
              ["--masks", masks, "--positives", emb],                 # both
              ["--masks", masks, "--threshold", "0.5"],
              ["--positives", emb],                                   # incomplete query
              ["--positives", emb, "--negatives", emb],
              ["--masks", masks, "--label", "255"],
              ["--masks", masks, "--min-ratio", "1.5"],
              ["--masks", masks, "--min-weight", "-1"])
    for extra in groups:
        with pytest.raises(SystemExit) as exc:
            lift.main(base + extra)
        assert exc.value.code == 2, extra
    capsys.readouterr()
    # a frame without its mask: an error message and status 2, before the checkpoint is looked at
    np.save(os.path.join(masks, "frame_0000.npy"), np.zeros((12, 16), np.int64))
    assert lift.main(base + ["--masks", masks]) == 2
    assert "no mask for frame 'frame_0001'" in capsys.readouterr().err
    assert not os.path.exists(str(tmp_path / "sel.npy"))


def _object_parser(hull=True):
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt")
    ap.add_argument("--transform-json", default=None)
    _cli.add_object_options(ap, "selects", "selects" if hull else None)
    return ap


def test_shared_object_options_default_to_off(monkeypatch):
    ap = _object_parser()
    a = ap.parse_args(["--positives", "p.npy", "--negatives", "n.npy", "--threshold", "0.6"])
    assert a.views is None and a.object_masks is None
    for hull in ("optional", "required", "none"):
        _cli.check_object_options(ap, a, hull)
    calls = []
    from gaussiangrasper_amd import interop, query
    monkeypatch.setattr(interop, "fea_up_weights", lambda *x: "weights")
    monkeypatch.setattr(query, "load_embeddings", lambda path, name: path)
    monkeypatch.setattr(query, "select_gaussians", lambda *x: calls.append(("own", x[1:])) or "own")
    monkeypatch.setattr(query, "select_gaussians_in_views", lambda *x: calls.append(("views", x[1:])) or "views")

    class S:
        means = torch.zeros(1, 3)
    assert _cli.selection_mask(a, S(), None) == "own"
    assert calls == [("own", ("weights", "p.npy", "n.npy", 0.6))]
    none = ap.parse_args([])
    _cli.check_object_options(ap, none, "optional")
    assert _cli.selection_mask(none, S(), None) is None
    pts = ap.parse_args(["--object-points", "o.npy"])
    _cli.check_object_options(ap, pts, "required")


def test_shared_object_options_views_and_masks(monkeypatch, tmp_path):
    ap = _object_parser()
    t, masks = _scan(tmp_path)
    q = ["--positives", "p.npy", "--negatives", "n.npy", "--threshold", "0.6"]
    for bad in (["--object-masks", masks], ["--views", t], ["--views", t, "--object-masks", masks] + q,
                ["--views", t, "--object-masks", masks, "--object-points", "o.npy"]):
        with pytest.raises(SystemExit):
            _cli.check_object_options(ap, ap.parse_args(bad), "optional")
    a = ap.parse_args(["--views", t] + q)
    _cli.check_object_options(ap, a, "required")
    calls = []
    from gaussiangrasper_amd import interop, query
    monkeypatch.setattr(interop, "fea_up_weights", lambda *x: "weights")
    monkeypatch.setattr(query, "load_embeddings", lambda path, name: path)
    monkeypatch.setattr(query, "select_gaussians_in_views", lambda *x: calls.append(x[1:]) or "views")

    class S:
        means = torch.zeros(1, 3)
    assert _cli.selection_mask(a, S(), None) == "views"
    (w, cams, pos, neg, thr), = calls
    assert (w, pos, neg, thr) == ("weights", "p.npy", "n.npy", 0.6) and len(cams) == 2 and cams[0][2:] == (12, 16)
    m = ap.parse_args(["--views", t, "--object-masks", masks, "--instance", "largest"])
    _cli.check_object_options(ap, m, "required")
    with pytest.raises(ValueError, match="no mask for frame 'frame_0000'"):
        _cli.selection_mask(m, S(), None)
