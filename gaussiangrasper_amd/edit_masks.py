"""Per-view masks of the moved object for the fine-tune after a scene update: where the object was and where it is
now, in every frame of a scan — the reference's scripts/project_hull.py (:83-121), which makes them one frame at a
time in numpy and cv2 — on one HIP call (`gg_object_masks`, csrc/objmask.hip).  The contract is in
include/gg_raster.h and PARITY.md "Scene update", the design in DESIGN.md §3.14.

    project_hull.py                                   here
    get_transform :8-19                               edit.pose_to_matrix(to) @ inv(edit.pose_to_matrix(from))
    inv(transform_matrix) :86-87, intrinsic_matrix    scan_masks (transforms.json, per-frame overrides)
    project_points_3d_to_2d + astype(int32) :21-34    object_masks (gg_object_masks: project, truncate)
    get_convex_hull_mask :36-46                       exact closed convex hull (no LINE_AA rim, PARITY)
    get_dialated_mask :48-53 (not called there)       dilate=k
    finetune_mask1 / 2 / 3, center1 :93-121           ObjectMasks.before / after / union, centres
    python -m gaussiangrasper_amd.edit_masks --transforms T.json --object-points obj.txt --pose-from ... \\
        --pose-to ... --out DIR [--dilate K] [--all]

The overlay PNGs (:95-99, :110-114) are not made.  No GPU work falls back to the host: a missing device is an
error."""
from __future__ import annotations

import argparse
import json
import os
import sys
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._call import ArrayLike, default_device, host_ptr, ptr as _ptr, stream as _stream, to_device, workspace as _ws
from .edit import load_object_points, pose_to_matrix
from .frames import rigid_rows
from .prepare import camera_params

MAX_ROWS = 16384                 # default row-table capacity per (view, pose)
MASK_NAMES = ("before", "after", "union")


@dataclass
class ObjectMasks:
    """Device tensors of one gg_object_masks call: masks (V, H, W) bool; boxes (V, 3, 4) int32 rmin, rmax, cmin, cmax
    of before / after / union (-1 when empty); centres (V, 3, 2) float64 (row, col), NaN when empty; dropped (V, 2)
    int32 points dropped before / after (behind the camera or not finite)."""
    before: Tensor
    after: Tensor
    union: Tensor
    boxes: Tensor
    centres: Tensor
    dropped: Tensor


def object_masks(points: ArrayLike, transform: ArrayLike, intrinsics: ArrayLike, w2c: ArrayLike, height: int,
                 width: int, dilate: int = 0, max_rows: int = MAX_ROWS) -> ObjectMasks:
    """Masks of the object's points P (M, 3) before and after the motion T ([R | t] (3, 4) or (4, 4)) in V views:
    intrinsics (V, 4) fx, fy, cx, cy and w2c (V, 3, 4) or (V, 4, 4) world-to-camera (OpenCV axes), all fp64.  One
    launch sequence and one status read-back; raises _lib.GGError when a view's projection spans more than max_rows
    pixel rows (nothing is returned then)."""
    dev = points.device if isinstance(points, Tensor) and points.device.type == "cuda" else \
        default_device("edit_masks")
    P = to_device(points, torch.float64, dev)
    if P.ndim != 2 or P.shape[1] != 3:
        raise ValueError(f"points must be (M, 3), got {tuple(P.shape)}")
    T = rigid_rows(transform, np.float64)
    K = to_device(intrinsics, torch.float64, dev)
    E = to_device(w2c, torch.float64, dev)
    if K.ndim != 2 or K.shape[1] != 4:
        raise ValueError(f"intrinsics must be (V, 4) fx, fy, cx, cy, got {tuple(K.shape)}")
    if E.ndim != 3 or E.shape[0] != K.shape[0] or E.shape[1:] not in ((3, 4), (4, 4)):
        raise ValueError(f"w2c must be ({K.shape[0]}, 3, 4) or ({K.shape[0]}, 4, 4), got {tuple(E.shape)}")
    E = E[:, :3, :].contiguous()
    V, h, w = K.shape[0], int(height), int(width)
    if h < 1 or w < 1:
        raise ValueError(f"image size must be positive, got {h} x {w}")
    if int(dilate) < 0:
        raise ValueError(f"dilate must be >= 0, got {dilate}")
    lib = _lib.load()
    need = lib.gg_object_masks_workspace(V, int(max_rows))
    if need == 0:
        raise ValueError(f"unsupported sizes: {V} views, max_rows {max_rows}")
    ws = _ws(need, dev)
    m = torch.empty((3, V, h, w), dtype=torch.uint8, device=dev)
    boxes = torch.empty((V, 3, 4), dtype=torch.int32, device=dev)
    centres = torch.empty((V, 3, 2), dtype=torch.float64, device=dev)
    dropped = torch.empty((V, 2), dtype=torch.int32, device=dev)
    _lib.check(lib.gg_object_masks(P.shape[0], _ptr(P), host_ptr(T), V, _ptr(K), _ptr(E), h, w,
                                   int(dilate), int(max_rows), _ptr(m[0]), _ptr(m[1]), _ptr(m[2]), _ptr(boxes),
                                   _ptr(centres), _ptr(dropped), _ptr(ws), ws.numel(), _stream(dev)),
               "gg_object_masks")
    mb = m.view(torch.bool)
    return ObjectMasks(mb[0], mb[1], mb[2], boxes, centres, dropped)


# ------------------------------------------------------------------------------------------------
# a scan's transforms.json
# ------------------------------------------------------------------------------------------------
def mask_stem(file_path: str) -> str:
    """Output name of a frame: the basename of file_path with its extension replaced by .npy (the reference's
    `.replace('.png', '.npy')` would make x.jpg.npy of x.jpg; PARITY)."""
    return os.path.splitext(os.path.basename(file_path))[0] + ".npy"


def scan_cameras(meta: dict) -> Tuple[np.ndarray, np.ndarray, int, int]:
    """intrinsics (V, 4) fx, fy, cx, cy (per-frame overrides), w2c (V, 4, 4) = inv(transform_matrix) in fp64 (no axis
    flip), height, width of a transforms.json."""
    frames = meta.get("frames") or []
    if not frames:
        raise ValueError("transforms.json has no frames")
    for key in ("w", "h"):
        if key not in meta:
            raise ValueError(f"transforms.json has no '{key}'")
    intr = np.array([camera_params(meta, fr)[:4] for fr in frames], dtype=np.float64)
    w2c = np.array([np.linalg.inv(np.asarray(fr["transform_matrix"], dtype=np.float64)) for fr in frames])
    return intr, w2c, int(meta["h"]), int(meta["w"])


def motion(pose_from: ArrayLike, pose_to: ArrayLike) -> np.ndarray:
    """get_transform (:8-19): T = T(to) @ inv(T(from)), 4 x 4 fp64."""
    return pose_to_matrix(pose_to) @ np.linalg.inv(pose_to_matrix(pose_from))


def scan_masks(transforms_json_path: str, points: ArrayLike, pose_from: ArrayLike, pose_to: ArrayLike,
               dilate: int = 0, max_rows: int = MAX_ROWS) -> Tuple[ObjectMasks, List[str]]:
    """Masks of every frame of a nerfstudio transforms.json (object points in the scan's raw frame) and the frames'
    output names (mask_stem)."""
    with open(transforms_json_path) as f:
        meta = json.load(f)
    intr, w2c, h, w = scan_cameras(meta)
    masks = object_masks(points, motion(pose_from, pose_to), intr, w2c, h, w, dilate, max_rows)
    return masks, [mask_stem(fr["file_path"]) for fr in meta["frames"]]


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.edit_masks",
                                 description="Per-frame masks of a moved object (where it was | where it is now) for "
                                             "the fine-tune after a scene update: DIR/union/<stem>.npy, float64 0/1.")
    ap.add_argument("--transforms", required=True, help="the scan's transforms.json")
    ap.add_argument("--object-points", required=True, help="object point cloud, .npy or text, first 3 columns")
    ap.add_argument("--pose-from", type=float, nargs=6, required=True, metavar=("X", "Y", "Z", "RX", "RY", "RZ"))
    ap.add_argument("--pose-to", type=float, nargs=6, required=True, metavar=("X", "Y", "Z", "RX", "RY", "RZ"))
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--dilate", type=int, default=0, help="k x k dilation of each mask (0 or 1: none)")
    ap.add_argument("--max-rows", type=int, default=MAX_ROWS, help="row-table capacity per view and pose")
    ap.add_argument("--all", action="store_true", help="also write before/ and after/")
    a = ap.parse_args(argv)
    if a.dilate < 0:
        ap.error("--dilate must be >= 0")
    try:
        pts = load_object_points(a.object_points)
        masks, stems = scan_masks(a.transforms, pts, a.pose_from, a.pose_to, a.dilate, a.max_rows)
    except (OSError, KeyError, ValueError, _lib.GGError) as exc:
        print(f"error: {exc}", file=sys.stderr)
        return 2
    names = MASK_NAMES if a.all else ("union",)
    host = {n: getattr(masks, n).cpu().numpy() for n in names}
    boxes, centres = masks.boxes.cpu().numpy(), masks.centres.cpu().numpy()
    dropped = masks.dropped.cpu().numpy()
    for n in names:
        os.makedirs(os.path.join(a.out, n), exist_ok=True)
    prompts = []
    for i, stem in enumerate(stems):
        for n in names:
            np.save(os.path.join(a.out, n, stem), host[n][i].astype(np.float64))
        prompts.append({"mask": stem,
                        "boxes": {n: boxes[i, m].tolist() for m, n in enumerate(MASK_NAMES)},
                        "centres": {n: [None if np.isnan(c) else float(c) for c in centres[i, m]]
                                    for m, n in enumerate(MASK_NAMES)},
                        "dropped": {"before": int(dropped[i, 0]), "after": int(dropped[i, 1])}})
    with open(os.path.join(a.out, "prompts.json"), "w") as f:
        json.dump({"frames": prompts}, f, indent=1)
    empty = int((boxes[:, 2, 0] < 0).sum())
    print(f"{len(stems)} frames {host['union'].shape[2]}x{host['union'].shape[1]}: {len(stems) - empty} with the "
          f"object, {empty} empty; {int(dropped.sum())} projections dropped -> {a.out}")
    if empty == len(stems):
        print("error: the object is in no frame", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
