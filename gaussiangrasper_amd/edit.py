"""Scene update after a grasp: the first half of the reference's `update.sh` (nerfstudio/scripts/update.py, SURVEY.md
§3.3) — select the Gaussians inside the convex hull of an object's point cloud and move them rigidly with the
gripper's pose change — on one HIP kernel (`gg_hull_edit`, csrc/edit.hip) instead of a host round trip.

    update.py                                  here
    points_inside_convex_hull :293-328         filter_object_points -> hull_planes -> select_and_move (mask)
    prepare_transform :342-355, main :141-158  rotvec_to_matrix, compose_transform, object_points_to_scene
    transformed_gs :217-240                    select_and_move (in place) / edit_model
    (not in the reference)                     sh= / rotate_sh= / --rotate-sh: the moved Gaussians' SH lobes turn too
    (not in the reference)                     refine= / --refine-transforms: the pose change is first corrected against
                                               frames captured after the object was put down (pose.refine_object)
    save_checkpoint :257-286                   python -m gaussiangrasper_amd.edit ... --out step-000000000.ckpt

The fine-tune that follows is the existing training path.  Two deliberate differences from the reference
(PARITY.md): the inside test is the hull's half-spaces with a tolerance instead of `Delaunay.find_simplex`, and the
moved quaternions come from Shepperd's method, which takes the reference's formula where the trace is the largest
diagonal term and never produces NaN.  scipy (Qhull) is needed only to build the hull from points; callers that
have the planes pass them directly."""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib, sh_rotation
from ._call import ArrayLike, host_ptr, ptr as _ptr, require_hip as _require_hip, stream as _stream
from .frames import load_transform_json, points_to_scene as object_points_to_scene, rigid_rows
from .interop import MODEL_PREFIX


# ------------------------------------------------------------------------------------------------
# host side: the object's hull and the rigid transform (numpy, fp64)
# ------------------------------------------------------------------------------------------------
def filter_object_points(points: ArrayLike, outlier_factor: float = 1.0) -> np.ndarray:
    """The reference's outlier filter (update.py:313-319): per axis Q1 = 0th and Q3 = 80th percentile, IQR = Q3 - Q1;
    a row is dropped when any coordinate lies outside [Q1 - f IQR, Q3 + f IQR].  Q1 is the minimum, so the low side
    never drops anything — kept as the reference has it."""
    p = np.asarray(points, dtype=np.float64)
    lo = np.percentile(p, 0, axis=0)
    hi = np.percentile(p, 80, axis=0)
    iqr = hi - lo
    out = (p < lo - outlier_factor * iqr) | (p > hi + outlier_factor * iqr)
    return p[~out.any(axis=1)]


def hull_planes(points: ArrayLike) -> np.ndarray:
    """(F, 4) float64 outward half-spaces (n0, n1, n2, d) of the convex hull of `points`, inside where n.x + d <= 0:
    Qhull's `equations` through scipy.spatial.ConvexHull."""
    try:
        from scipy.spatial import ConvexHull
    except ImportError as exc:
        raise ImportError("hull_planes needs scipy (scipy.spatial.ConvexHull); without it, build the hull elsewhere "
                          "and pass its (F, 4) half-spaces as planes= directly") from exc
    eq = ConvexHull(np.asarray(points, dtype=np.float64)).equations
    return np.ascontiguousarray(eq, dtype=np.float64)


def rotvec_to_matrix(rotvec: ArrayLike) -> np.ndarray:
    """3x3 rotation of an axis-angle vector (Rodrigues; what scipy's Rotation.from_rotvec(v).as_matrix() gives)."""
    v = np.asarray(rotvec, dtype=np.float64).reshape(3)
    theta = float(np.linalg.norm(v))
    if theta == 0.0:
        return np.eye(3)
    k = v / theta
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


def pose_to_matrix(pose: ArrayLike) -> np.ndarray:
    """4x4 homogeneous matrix of a gripper pose x, y, z, rx, ry, rz (translation, rotation vector)."""
    p = np.asarray(pose, dtype=np.float64).reshape(6)
    T = np.eye(4)
    T[:3, :3] = rotvec_to_matrix(p[3:])
    T[:3, 3] = p[:3]
    return T


def compose_transform(matrix: ArrayLike, scale: float, pose_from: ArrayLike, pose_to: ArrayLike) -> np.ndarray:
    """The scene-frame rigid motion of the grasped object (update.py main :151-155 with prepare_transform :342-355):
    T = matrix @ T_to @ inv(T_from) @ inv(matrix) in fp64, its translation times `scale`.  Returns [R | t], (3, 4)
    float32 — what select_and_move takes."""
    M = np.asarray(matrix, dtype=np.float64)
    T = M @ (pose_to_matrix(pose_to) @ np.linalg.inv(pose_to_matrix(pose_from))) @ np.linalg.inv(M)
    T[:3, 3] *= float(scale)
    return T[:3, :].astype(np.float32)


# ------------------------------------------------------------------------------------------------
# device side: one launch of gg_hull_edit
# ------------------------------------------------------------------------------------------------
def select_and_move(means: Tensor, quats: Optional[Tensor], planes: ArrayLike,
                    transform: Optional[ArrayLike] = None, tol: float = 0.0,
                    sh: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """Select the Gaussians whose mean is inside the hull (every plane n.x + d <= tol) and, with a transform, move
    them in place: means' = R x + t, quats' = quaternion of R quat_to_rotmat(q) (Shepperd, w >= 0).  Rows not
    selected are not written.  One launch; nothing waits on the host.

    means (N, 3) and quats (N, 4): fp32, contiguous, on the HIP device (no CPU path); quats may be None without a
    transform.  planes: (F >= 4, 4) half-spaces (hull_planes).  Returns (mask (N,) uint8, count () int64), both on
    the device.

    sh: the SH colour coefficients (N, K, 3), fp32, contiguous, same device.  With it the selected rows' lobes are
    turned by R as well (gg_sh_rotate, a second launch on the same stream that reads the mask the first one wrote; no
    read-back).  R is the float32 [R | t] actually applied to the means, widened to fp64 (sh_rotation.rotation_bands);
    when it is exactly the identity, a translation only, the second launch is skipped.  Needs a transform."""
    dev = _require_hip(*[t for t in (means, quats, sh) if t is not None])
    for name, t, w in (("means", means, 3), ("quats", quats, 4)):
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_contiguous() or t.ndim != 2 or t.shape[1] != w:
            raise ValueError(f"{name} must be a contiguous float32 (N, {w}) tensor, got {t.dtype} "
                             f"{tuple(t.shape)}{'' if t.is_contiguous() else ' (not contiguous)'}")
    n = means.shape[0]
    if quats is not None and quats.shape[0] != n:
        raise ValueError(f"means has {n} rows, quats {quats.shape[0]}")
    rt = None if transform is None else rigid_rows(transform, np.float32)
    if rt is not None and quats is None:
        raise ValueError("a transform moves means and quats: pass quats")
    packed = None
    if sh is not None:
        if rt is None:
            raise ValueError("sh is rotated with the moved Gaussians: pass a transform")
        k = sh_rotation.check_coefficients(sh)
        if sh.shape[0] != n:
            raise ValueError(f"means has {n} rows, sh {sh.shape[0]}")
        R = rt.reshape(3, 4)[:, :3].astype(np.float64)
        if k > 1 and not np.array_equal(R, np.eye(3)):      # built before anything is moved: a bad R moves nothing
            packed = sh_rotation.pack_bands(sh_rotation.rotation_bands(R, sh_rotation.NUM_BASES.index(k)), k)
    pl = torch.as_tensor(planes.detach() if isinstance(planes, Tensor) else np.asarray(planes))
    pl = pl.to(device=dev, dtype=torch.float64).contiguous()
    if pl.ndim != 2 or pl.shape[1] != 4 or pl.shape[0] < 4:
        raise ValueError(f"planes must be (F >= 4, 4) half-spaces (n0, n1, n2, d), got {tuple(pl.shape)}")
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    count = torch.empty((), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().gg_hull_edit(n, _ptr(means), _ptr(quats), pl.shape[0], _ptr(pl), float(tol), host_ptr(rt),
                                        _ptr(mask), _ptr(count), _stream(dev)), "gg_hull_edit")
    if packed is not None:
        sh_rotation.launch(sh, mask, packed, dev)
    return mask, count


def refine_transform(model, planes: ArrayLike, transform: Optional[ArrayLike], refine: dict, tol: float = 0.0
                     ) -> np.ndarray:
    """The object's motion re-localised against observed frames before it is applied (pose.refine_object): select
    the hull's Gaussians (nothing is moved), fit the six-number correction on the left of `transform` with every
    Gaussian frozen, and return the composed [R | t], (3, 4) float32 — what select_and_move takes.
    refine: pose.refine_object's keywords — cameras, rgbs, and optionally depths, valids, steps, depth_weight, mode."""
    from . import pose
    mask, count = select_and_move(model.means.detach(), None, planes, None, tol)
    if int(count.item()) == 0:
        raise ValueError("no Gaussian lies inside the object's hull")
    base = None
    if transform is not None:
        base = torch.eye(4, dtype=torch.float64)
        base[:3, :] = torch.from_numpy(rigid_rows(transform, np.float64).reshape(3, 4))
    T, _ = pose.refine_object(model, mask, base=base, **refine)
    return T[:3, :].detach().cpu().numpy().astype(np.float32)


def edit_model(model, planes: ArrayLike, transform: Optional[ArrayLike], tol: float = 0.0,
               rotate_sh: bool = False, refine: Optional[dict] = None) -> int:
    """update.py transformed_gs (:217-240) on a model holding `means` / `quats` Parameters (the plugin's fused model,
    stub.StubGaussianSplattingModel): the same Parameter objects are edited in place, so an optimizer keeps
    referencing them and its Adam moments stay as they are (the reference keeps them too: it saves the original
    checkpoint's `optimizers`).  The version counters are bumped after the raw-pointer write, so nothing keyed on
    (data_ptr, _version) serves the unedited scene.  Returns the number of Gaussians selected; raises if none are
    (the reference asserts the same).

    rotate_sh: also turn the selected rows of `model.colors_all` (select_and_move's sh=), in place on the same
    Parameter.  Its Adam moments are left as they are, like those of means and quats: they are not rotated.

    refine: None, or refine_transform's dictionary (cameras, rgbs, depths, valids, steps, ...): the transform is
    first corrected against the observed frames with the Gaussians frozen, then applied by the same exact path
    (Shepperd's quaternion rule, rotate_sh as given)."""
    if refine is not None:
        with torch.enable_grad():
            transform = refine_transform(model, planes, transform, refine, tol)
    with torch.no_grad():
        return _edit_model(model, planes, transform, tol, rotate_sh)


def _edit_model(model, planes, transform, tol, rotate_sh) -> int:
    means, quats = model.means, model.quats
    colors = model.colors_all if rotate_sh else None
    mask, count = select_and_move(means.detach(), quats.detach(), planes, transform, tol,
                                  sh=None if colors is None else colors.detach())
    torch.autograd.graph.increment_version(means)
    torch.autograd.graph.increment_version(quats)
    if colors is not None:
        torch.autograd.graph.increment_version(colors)
    selected = int(count.item())
    if selected == 0:
        raise ValueError("no Gaussian lies inside the object's hull")
    return selected


# ------------------------------------------------------------------------------------------------
# command line: update.sh steps 1-3 on a checkpoint
# ------------------------------------------------------------------------------------------------
def load_object_points(path: str) -> np.ndarray:
    """(M, 3) object points from .npy or text (update.py:144-147: the first three columns)."""
    pts = np.load(path) if path.endswith(".npy") else np.loadtxt(path)
    pts = np.asarray(pts, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] < 3:
        raise ValueError(f"{path}: expected (M, >=3) points, got {pts.shape}")
    return pts[:, :3]


def read_refine_frames(transforms_json: str, transform_json: Optional[str], scale: float,
                       depth_dir: Optional[str] = None):
    """The observed frames pose.refine_object fits against, from a scan's transforms.json (OpenCV c2w, raw frame):
    (cameras as lift.scene_cameras gives them, in the checkpoint's frame; rgbs (H, W, 3) float32 in [0, 1], read with
    PIL from images/<stem>.png next to the json, as prepare reads them; depths (H, W) float32 or None, <stem>.npy of
    depth_dir in the scan's metres times `scale`; valids (H, W) bool, depth > 0, or None)."""
    from PIL import Image
    from .lift import frame_stems, scene_cameras
    cams, _ = scene_cameras(transforms_json, transform_json)
    root = os.path.dirname(os.path.abspath(transforms_json))
    rgbs, depths, valids = [], [], []
    for stem, (_, _, h, w) in zip(frame_stems(transforms_json), cams):
        path = os.path.join(root, "images", stem + ".png")
        if not os.path.exists(path):
            raise ValueError(f"missing file: {path}")
        rgb = np.asarray(Image.open(path).convert("RGB"))
        if rgb.shape[:2] != (h, w):
            raise ValueError(f"{path} is {rgb.shape[0]} x {rgb.shape[1]}, transforms.json gives h x w = {h} x {w}")
        rgbs.append(torch.from_numpy(rgb.astype(np.float32) / 255.0))
        if depth_dir:
            dpath = os.path.join(depth_dir, stem + ".npy")
            if not os.path.exists(dpath):
                raise ValueError(f"missing file: {dpath}")
            d = np.load(dpath).astype(np.float64).reshape(h, w) * float(scale)
            depths.append(torch.from_numpy(d.astype(np.float32)))
            valids.append(torch.from_numpy(np.isfinite(d) & (d > 0)))
    return cams, rgbs, (depths or None), (valids or None)


def refine_scene_transform(scene, mask: Tensor, rt: np.ndarray, cams, rgbs, depths=None, valids=None,
                           steps: int = 100) -> np.ndarray:
    """pose.refine_object on a Scene (a checkpoint's tensors) through the differentiable operator sequence
    (pipeline.render_view), cameras as lift.scene_cameras gives them: the corrected [R | t], (3, 4) float32."""
    from . import ops, pose
    from .camera import view_from_c2w
    from .constants import deg_from_sh
    from .frames import homogeneous
    from .pipeline import render_view
    from .scene import Scene
    dev = scene.means.device
    views = [view_from_c2w(torch.as_tensor(homogeneous(c2w)), *[float(v) for v in K], int(h), int(w), dev)
             for c2w, K, h, w in cams]
    deg = deg_from_sh(scene.colors_all.shape[1])
    fixed = [t.detach() for t in (scene.scales, scene.opacities, scene.colors_all, scene.feature)]

    def render(means, quats, k):
        ops.clear_bin_cache()
        s = Scene(means, fixed[0], quats, fixed[1], fixed[2], fixed[3])
        return render_view(s, views[k], ops, sh_degree_to_use=deg, channels=("rgb", "depth"))
    base = torch.eye(4, dtype=torch.float64)
    base[:3, :] = torch.from_numpy(np.asarray(rt, np.float64).reshape(3, 4))
    T, _ = pose.refine_object(render, mask, [None] * len(views), rgbs, depths=depths, valids=valids, base=base,
                              steps=steps, means=scene.means.float(), quats=scene.quats.float())
    return T[:3, :].detach().cpu().numpy().astype(np.float32)


def edit_checkpoint(ckpt: str, object_points: np.ndarray, matrix: ArrayLike, scale: float, pose_from: ArrayLike,
                    pose_to: ArrayLike, out: str, tol: float = 0.0, outlier_factor: float = 1.0,
                    device: str = "cuda", rotate_sh: bool = False, refine: Optional[dict] = None) -> int:
    """Load `ckpt`, move the Gaussians inside the object's hull, write `out` with `step` 0.  Only
    `pipeline["_model.means"]` and `pipeline["_model.quats"]` change — with rotate_sh also
    `pipeline["_model.colors_all"]`, the moved Gaussians' SH coefficients turned with them and written back in their
    stored dtype; every other entry, `optimizers` included (Adam moments are not rotated), is saved as loaded
    (update.py save_checkpoint :257-286).  Returns the selected count."""
    blob = torch.load(ckpt, map_location="cpu", weights_only=True)
    pipe = blob.get("pipeline") if isinstance(blob, dict) else None
    keys = (MODEL_PREFIX + "means", MODEL_PREFIX + "quats") + ((MODEL_PREFIX + "colors_all",) if rotate_sh else ())
    if not isinstance(pipe, dict) or any(k not in pipe for k in keys):
        raise KeyError(f"{ckpt}: not a splatting checkpoint (no pipeline entries {', '.join(keys)})")
    pts = filter_object_points(object_points_to_scene(object_points, matrix, scale), outlier_factor)
    planes = hull_planes(pts)
    rt = compose_transform(matrix, scale, pose_from, pose_to)
    m0, q0 = pipe[keys[0]], pipe[keys[1]]
    means = m0.detach().to(device=device, dtype=torch.float32).contiguous()
    quats = q0.detach().to(device=device, dtype=torch.float32).contiguous()
    sh = pipe[keys[2]].detach().to(device=device, dtype=torch.float32).contiguous() if rotate_sh else None
    if refine is not None:
        # re-localise the object against the observed frames first (pose.refine_object); the move itself stays the
        # exact path below.  refine: transforms (the frames' transforms.json), transform_json (the dataparser's file,
        # for the cameras), depth_dir, steps
        from ._cli import load_scene
        sel, n_sel = select_and_move(means, None, planes, None, tol)
        if int(n_sel.item()) == 0:
            raise ValueError("no Gaussian lies inside the object's hull")
        cams, rgbs, depths, valids = read_refine_frames(refine["transforms"], refine.get("transform_json"), scale,
                                                        refine.get("depth_dir"))
        rt = refine_scene_transform(load_scene(ckpt)[0], sel, rt, cams, rgbs, depths, valids,
                                    steps=int(refine.get("steps") or 100))
    _, count = select_and_move(means, quats, planes, rt, tol, sh=sh)
    selected = int(count.item())
    if selected == 0:
        raise ValueError("no Gaussian lies inside the object's hull")
    new_pipe = dict(pipe)
    new_pipe[keys[0]] = means.cpu().to(m0.dtype)
    new_pipe[keys[1]] = quats.cpu().to(q0.dtype)
    if rotate_sh:
        new_pipe[keys[2]] = sh.cpu().to(pipe[keys[2]].dtype)
    new_blob = dict(blob)
    new_blob["pipeline"] = new_pipe
    new_blob["step"] = 0
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    torch.save(new_blob, out)
    return selected


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.edit",
                                 description="Move the Gaussians inside an object's convex hull with the gripper's "
                                             "pose change (update.sh steps 1-3) and write a checkpoint to fine-tune.")
    ap.add_argument("--ckpt", required=True, help="input step-*.ckpt")
    ap.add_argument("--object-points", required=True, help="object point cloud, .npy or text, first 3 columns")
    ap.add_argument("--transform-json", required=True, help="JSON with transform_matrix (4x4) and scale")
    ap.add_argument("--pose-from", type=float, nargs=6, required=True, metavar=("X", "Y", "Z", "RX", "RY", "RZ"))
    ap.add_argument("--pose-to", type=float, nargs=6, required=True, metavar=("X", "Y", "Z", "RX", "RY", "RZ"))
    ap.add_argument("--out", required=True, help="output checkpoint, e.g. .../step-000000000.ckpt")
    ap.add_argument("--tol", type=float, default=0.0, help="a mean is inside when every n.x + d <= tol")
    ap.add_argument("--outlier-factor", type=float, default=1.0)
    ap.add_argument("--rotate-sh", action="store_true",
                    help="also rotate the moved Gaussians' SH colour coefficients (_model.colors_all)")
    ap.add_argument("--refine-transforms", default=None, metavar="T.json",
                    help="re-localise the object first: a transforms.json (OpenCV c2w, raw frame) of frames captured "
                         "after the object was put down, images in images/<stem>.png next to it; the pose change is "
                         "corrected by fitting the render to them with the Gaussians frozen (pose.refine_object)")
    ap.add_argument("--refine-depth", default=None, metavar="DIR",
                    help="with --refine-transforms: <stem>.npy depth maps of those frames, metres")
    ap.add_argument("--refine-steps", type=int, default=None, metavar="K",
                    help="with --refine-transforms: at most K evaluations of the loss (default 100)")
    a = ap.parse_args(argv)
    if not a.refine_transforms and (a.refine_depth or a.refine_steps is not None):
        ap.error("--refine-depth / --refine-steps need --refine-transforms")
    if a.refine_steps is not None and a.refine_steps < 1:
        ap.error(f"--refine-steps must be >= 1, got {a.refine_steps}")
    with open(a.transform_json) as f:
        tj = json.load(f)
    refine = None
    if a.refine_transforms:
        refine = {"transforms": a.refine_transforms, "transform_json": a.transform_json, "depth_dir": a.refine_depth,
                  "steps": a.refine_steps}
    try:
        n = edit_checkpoint(a.ckpt, load_object_points(a.object_points), *load_transform_json(tj), a.pose_from,
                            a.pose_to, a.out, a.tol, a.outlier_factor, rotate_sh=a.rotate_sh, refine=refine)
    except (KeyError, ValueError) as exc:
        raise SystemExit(f"error: {exc}") from exc
    print(f"selected {n} Gaussians; wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
