"""Lift 2-D label images onto the Gaussians: exact blend-weight votes.

A segmenter's masks, or a thresholded relevancy image, say which PIXELS belong to an object.  The transpose of the
blend takes that to the Gaussians: for every Gaussian, the weight alpha T with which the forward walk blended it into
the pixels of each label, summed over many views (Gaussian Grouping, SAGA, FlashSplat use the same operator).  A
hidden Gaussian has no blend weight, so occlusion is handled by construction.  One HIP kernel per view
(`gg_blend_votes`, csrc/votes.hip) walks the tile lists exactly as the forward does and adds trunc(alpha T 2^24) as
integers: the sums do not depend on any order, so the votes are defined to the bit (include/gg_raster.h).

    accumulate_view(votes, model_or_scene, c2w, intrinsics, h, w, labels)   one view into a vote array
    lift_labels(model_or_scene, cameras, label_images, num_labels)          -> Votes (votes (N, L) int64, ...)
    weights(votes)                                                          votes / 2^24 as float64
    select(votes, label, min_ratio, min_weight)                             (N,) bool
    assign(votes, min_ratio, min_weight)                                    (N,) int32 label, -1: none
    python -m gaussiangrasper_amd.lift --ckpt ... --transforms T.json --masks DIR --out selection.npy

Labels are bytes: 0 .. num_labels - 1 vote, 255 means "ignore this pixel"; num_labels <= 255.  A vote is an exact
float64 while it stays below 2^53 units of 2^-24, i.e. about 5e8 fully opaque pixel hits of one Gaussian and label.
Inference only: nothing here carries autograd history."""
from __future__ import annotations

import argparse
import json
import os
import sys
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._call import ArrayLike, require_hip as _require_hip
from .frames import homogeneous

UNIT = float(2 ** 24)        # votes per unit of blend weight (GG votes are trunc(alpha T 2^24))
IGNORE = 255                 # the label that votes for nobody
MAX_LABELS = 255
MIN_RATIO = 0.5              # select's default share of a Gaussian's weight (unverified on a real checkpoint: PARITY.md)
MASK_EXTS = (".npy", ".png", ".jpg", ".jpeg")


@dataclass
class Votes:
    """What lift_labels returns: votes (N, L) int64 on the device in units of 2^-24 of blend weight, the number of
    views that were added, and how many pixels carried each label over all views ((L,) int64, host)."""
    votes: Tensor
    views: int
    pixel_counts: np.ndarray


# ------------------------------------------------------------------------------------------------
# pure functions of a vote array
# ------------------------------------------------------------------------------------------------
def _votes(votes) -> Tensor:
    v = votes.votes if isinstance(votes, Votes) else votes
    v = v if isinstance(v, Tensor) else torch.as_tensor(np.asarray(v))
    if v.ndim != 2 or v.dtype != torch.int64:
        raise ValueError(f"votes must be an int64 (N, L) array, got {v.dtype} {tuple(v.shape)}")
    return v


def _limits(min_ratio: float, min_weight: float) -> Tuple[float, float]:
    r, w = float(min_ratio), float(min_weight)
    if not 0.0 <= r <= 1.0:                       # NaN fails
        raise ValueError(f"min_ratio must be in [0, 1], got {min_ratio}")
    if not w >= 0.0:
        raise ValueError(f"min_weight must be >= 0, got {min_weight}")
    return r, w


def weights(votes) -> Tensor:
    """The blend weight behind every vote, float64 (N, L): votes / 2^24.  Exact while a vote is below 2^53 (about
    5e8 fully opaque pixel hits)."""
    return _votes(votes).double() / UNIT


def _passes(w: Tensor, total: Tensor, min_ratio: float, min_weight: float) -> Tensor:
    return (total > 0) & (w >= min_weight) & (w >= min_ratio * total)


def select(votes, label: int = 1, min_ratio: float = MIN_RATIO, min_weight: float = 0.0) -> Tensor:
    """(N,) bool: Gaussian g is selected iff total_g > 0, w >= min_weight and w >= min_ratio * total_g, where
    w = weights[g, label] and total_g is the weight over all labels (the integer sum, then one division).  Both limits
    are inclusive; each comparison is one float64 product and one comparison."""
    v = _votes(votes)
    if not 0 <= int(label) < v.shape[1]:
        raise ValueError(f"label must be in [0, {v.shape[1]}), got {label}")
    r, mw = _limits(min_ratio, min_weight)
    return _passes(v[:, int(label)].double() / UNIT, v.sum(dim=1).double() / UNIT, r, mw)


def assign(votes, min_ratio: float = MIN_RATIO, min_weight: float = 0.0) -> Tensor:
    """(N,) int32: the label with the most votes if it passes select's tests, -1 otherwise (ties: the smallest
    label)."""
    v = _votes(votes)
    r, mw = _limits(min_ratio, min_weight)
    n, L = v.shape
    if L == 0 or n == 0:
        return torch.full((n,), -1, dtype=torch.int32, device=v.device)
    top = v.max(dim=1, keepdim=True).values
    idx = torch.arange(L, device=v.device).expand(n, L)
    best = torch.where(v == top, idx, torch.full_like(idx, L)).min(dim=1).values
    ok = _passes(top[:, 0].double() / UNIT, v.sum(dim=1).double() / UNIT, r, mw)
    return torch.where(ok, best, torch.full_like(best, -1)).to(torch.int32)


# ------------------------------------------------------------------------------------------------
# views
# ------------------------------------------------------------------------------------------------
def _label_image(labels: ArrayLike, h: int, w: int, num_labels: int, what: str = "label image") -> Tensor:
    """A label image as a uint8 (h, w) tensor (on whatever device it is on), after the size and value checks."""
    t = labels if isinstance(labels, Tensor) else torch.as_tensor(np.asarray(labels))
    if tuple(t.shape) != (h, w):
        raise ValueError(f"{what}: expected ({h}, {w}) labels, got {tuple(t.shape)}")
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    if t.dtype.is_floating_point or t.dtype.is_complex:
        raise ValueError(f"{what}: labels must be integers or bool, got {t.dtype}")
    if t.numel():
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi > IGNORE:
            raise ValueError(f"{what}: labels must be in [0, {IGNORE}], got {lo} .. {hi}")
        bad = (t >= num_labels) & (t != IGNORE)
        if bool(bad.any()):
            raise ValueError(f"{what}: label {int(t[bad].min())} is neither below num_labels = {num_labels} nor "
                             f"{IGNORE} (ignore)")
    return t.to(torch.uint8).contiguous()


def _check_num_labels(num_labels: int) -> int:
    L = int(num_labels)
    if not 1 <= L <= MAX_LABELS:
        raise ValueError(f"num_labels must be in 1..{MAX_LABELS}, got {num_labels}")
    return L


@torch.no_grad()
def project_view(model_or_scene, c2w: ArrayLike, intrinsics: ArrayLike, height: int, width: int):
    """The projection of one view exactly as mesh.render_depth runs it (eval semantics, nerfstudio / OpenGL c2w,
    intrinsics fx, fy, cx, cy): (xys, depths, radii, conics, num_tiles_hit, opacity (N, 1)) for the rasterize
    operators and ops.blend_votes; one binning serves every call on these tensors."""
    from . import ops
    from .camera import view_from_c2w
    src = model_or_scene
    means, scales, quats, opac = src.means.detach(), src.scales.detach(), src.quats.detach(), src.opacities.detach()
    dev = _require_hip(means, scales, quats, opac)
    h, w = int(height), int(width)
    fx, fy, cx, cy = (float(x) for x in np.asarray(intrinsics, dtype=np.float64).reshape(4))
    view = view_from_c2w(torch.as_tensor(homogeneous(c2w)), fx, fy, cx, cy, h, w, dev)
    means = means.float().contiguous()
    xys, depths, radii, conics, num_tiles_hit, _ = ops.ProjectGaussians.apply(
        means, torch.exp(scales.float()), 1, (quats / quats.norm(dim=-1, keepdim=True)).float(),
        view.viewmat[:3, :], view.projmat, fx, fy, cx, cy, h, w, view.tile_bounds)
    op = torch.sigmoid(opac.float()).reshape(-1, 1).contiguous()
    return xys, depths, radii, conics, num_tiles_hit, op


@torch.no_grad()
def accumulate_view(votes: Tensor, model_or_scene, c2w: ArrayLike, intrinsics: ArrayLike, height: int, width: int,
                    labels: ArrayLike) -> bool:
    """Add one view's votes to `votes` (N, L) int64 on the device: project_view, then ops.blend_votes with the
    (height, width) label image.  False: nothing is visible from this camera, votes is unchanged."""
    from . import ops
    n = model_or_scene.means.shape[0]
    dev = _require_hip(model_or_scene.means, votes)
    h, w = int(height), int(width)
    if votes.ndim != 2 or votes.shape[0] != n:
        raise ValueError(f"votes must be ({n}, L), got {tuple(votes.shape)}")
    lab = _label_image(labels, h, w, votes.shape[1]).to(dev)
    if n == 0:
        return False
    return ops.blend_votes(*project_view(model_or_scene, c2w, intrinsics, h, w), h, w, lab, votes)


def lift_labels(model_or_scene, cameras: Sequence[Tuple[ArrayLike, ArrayLike, int, int]],
                label_images: Sequence[ArrayLike], num_labels: int) -> Votes:
    """Votes of every Gaussian for every label over `cameras` ((c2w OpenGL (3|4, 4), intrinsics fx, fy, cx, cy,
    height, width), as mesh.mesh_model takes them), one (height, width) label image per camera.  ValueError on an image
    of the wrong size or with a label in [num_labels, 255), before anything runs."""
    L = _check_num_labels(num_labels)
    cameras, label_images = list(cameras), list(label_images)
    if len(cameras) != len(label_images):
        raise ValueError(f"{len(cameras)} cameras but {len(label_images)} label images")
    labs = [_label_image(img, int(h), int(w), L, f"label image {k}")
            for k, (img, (_, _, h, w)) in enumerate(zip(label_images, cameras))]
    means = model_or_scene.means
    dev = _require_hip(means)
    votes = torch.zeros(means.shape[0], L, dtype=torch.int64, device=dev)
    counts = np.zeros(L, np.int64)
    views = 0
    for lab, (c2w, K, h, w) in zip(labs, cameras):
        counts += torch.bincount(lab.reshape(-1).long(), minlength=IGNORE + 1)[:L].cpu().numpy()
        views += 1
        accumulate_view(votes, model_or_scene, c2w, K, int(h), int(w), lab)
    return Votes(votes, views, counts)


# ------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------
def read_label_image(path: str) -> np.ndarray:
    """A mask file as labels: an integer .npy array gives label ids directly; a bool .npy array or an image gives
    non-zero -> 1 (read as prepare reads a boundary mask)."""
    if path.endswith(".npy"):
        m = np.load(path)
        if m.ndim == 2 and m.dtype != np.bool_ and np.issubdtype(m.dtype, np.integer):
            if m.size and (m.min() < 0 or m.max() > IGNORE):
                raise ValueError(f"{path}: labels must be in [0, {IGNORE}], got {m.min()} .. {m.max()}")
            return m.astype(np.uint8)
    from .prepare import _read_mask
    return _read_mask(path).astype(np.uint8)


def frame_stems(transforms_json: str) -> list:
    """The file stem of every frame of a transforms.json, in the order mesh.transforms_cameras lists the frames."""
    with open(transforms_json) as f:
        meta = json.load(f)
    return [os.path.splitext(os.path.basename(str(fr.get("file_path", k))))[0]
            for k, fr in enumerate(meta.get("frames") or [])]


def find_mask(masks_dir: str, stem: str) -> str:
    for ext in MASK_EXTS:
        p = os.path.join(masks_dir, stem + ext)
        if os.path.exists(p):
            return p
    raise ValueError(f"no mask for frame '{stem}' in {masks_dir} (looked for {', '.join(stem + e for e in MASK_EXTS)})")


def scene_cameras(transforms_json: str, transform_json: Optional[str] = None):
    """(cameras as lift_labels takes them, the dataparser's (matrix, scale) or None) of a scan's transforms.json."""
    from .frames import c2w_to_scene
    from .mesh import dataparser_transform, opencv_to_opengl_c2w, transforms_cameras
    tf = dataparser_transform(transform_json) if transform_json else None
    cams = []
    for c2w_cv, K, h, w in transforms_cameras(transforms_json):
        if tf is not None:
            c2w_cv = c2w_to_scene(c2w_cv, *tf)
        cams.append((opencv_to_opengl_c2w(c2w_cv), K, h, w))
    return cams, tf


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.lift",
                                 description="Select the Gaussians of an object from per-frame 2-D masks, or from the "
                                             "relevancy of rendered feature images: exact blend-weight votes.")
    ap.add_argument("--ckpt", required=True, help="step-*.ckpt of a splatting model")
    ap.add_argument("--transforms", required=True, help="the scan's transforms.json (OpenCV c2w, raw frame): the "
                                                        "cameras the masks belong to")
    ap.add_argument("--transform-json", default=None, help="dataparser_transforms.json (transform_matrix, scale) from "
                                                           "the scan's frame to the checkpoint's")
    ap.add_argument("--masks", default=None, metavar="DIR",
                    help="one mask per frame, named by the frame's file stem: an integer .npy gives label ids (255: "
                         "ignore), a bool .npy or an image gives non-zero -> 1")
    ap.add_argument("--positives", default=None, help=".npy text embeddings: label the pixels whose rendered feature's "
                                                      "relevancy exceeds --threshold")
    ap.add_argument("--negatives", default=None, help=".npy canonical negatives (LERF relevancy)")
    ap.add_argument("--threshold", type=float, default=None, help="relevancy threshold for --positives")
    ap.add_argument("--label", type=int, default=1, metavar="K", help="the label to select (default 1)")
    ap.add_argument("--min-ratio", type=float, default=MIN_RATIO,
                    help="the label's share of a Gaussian's blend weight, at least (default %(default)s)")
    ap.add_argument("--min-weight", type=float, default=0.0, help="the label's blend weight, at least")
    ap.add_argument("--out", required=True, help="output .npy, (N,) bool selection")
    ap.add_argument("--out-votes", default=None, help="also write the votes, (N, L) int64 in units of 2^-24")
    ap.add_argument("--out-points", default=None, help="also write the selected means in the scan's frame, (M, 3) "
                                                       "float64 (edit --object-points)")
    return ap


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = _parser()
    a = ap.parse_args(argv)
    query = a.positives or a.negatives or a.threshold is not None
    if bool(a.masks) == bool(query):
        ap.error("one of --masks and --positives / --negatives / --threshold is needed (they are alternatives)")
    if query and not (a.positives and a.negatives and a.threshold is not None):
        ap.error("--positives needs --negatives and --threshold (LERF relevancy)")
    if a.label < 0 or a.label >= MAX_LABELS:
        ap.error(f"--label must be in [0, {MAX_LABELS}), got {a.label}")
    try:
        _limits(a.min_ratio, a.min_weight)
    except ValueError as exc:
        ap.error(str(exc))
    try:
        cams, tf = scene_cameras(a.transforms, a.transform_json)
        if a.masks:
            labs = [read_label_image(find_mask(a.masks, s)) for s in frame_stems(a.transforms)]
            top = max(int(m[m != IGNORE].max(initial=0)) for m in labs)
            num_labels = max(top, a.label, 1) + 1
        from ._cli import load_scene
        scene, mlp_state = load_scene(a.ckpt)
        if a.masks:
            res = lift_labels(scene, cams, labs, num_labels)
        else:
            from . import query as Q
            from .interop import fea_up_weights
            if a.label != 1:
                raise ValueError("--positives labels the matching pixels 1: --label must be 1")
            w = fea_up_weights(mlp_state, scene.means.device, a.ckpt, "for --positives")
            res = Q.lift_relevancy(scene, w, cams, Q.load_embeddings(a.positives, "positives"),
                                   Q.load_embeddings(a.negatives, "negatives"), a.threshold)
        sel = select(res.votes, a.label, a.min_ratio, a.min_weight)
    except (KeyError, ValueError, OSError, _lib.GGError) as exc:
        print(f"error: {exc}", file=sys.stderr)
        return 2
    np.save(a.out, sel.cpu().numpy())
    if a.out_votes:
        np.save(a.out_votes, res.votes.cpu().numpy())
    if a.out_points:
        pts = scene.means.detach()[sel].double().cpu().numpy()
        if tf is not None:
            from .frames import points_from_scene
            pts = points_from_scene(pts, *tf)
        np.save(a.out_points, np.asarray(pts, dtype=np.float64))
    print(f"{int(sel.sum())} of {sel.shape[0]} Gaussians carry label {a.label} over {res.views} views "
          f"({int(res.pixel_counts[a.label]) if a.label < len(res.pixel_counts) else 0} labelled pixels) -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
