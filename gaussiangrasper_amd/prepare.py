"""Scene preparation from RGB-D frames (the paper's step (a)): from a scan directory to the layout the trainer's
COLMAP parser and dataset loader read — seed cloud, cameras, poses and per-view normal maps — and the exact k nearest
neighbours whose distances set the first Gaussian scales.  The hot paths are HIP (csrc/prepare.hip, csrc/knn.hip);
the contracts are in include/gg_raster.h and PARITY.md "Scene preparation", the design in DESIGN.md §3.13.

    reference (scripts/generate_data.py, gaussian_splatting.py)     here
    depth_image_to_point_cloud + merge_point_clouds :14-45            backproject_frames (gg_backproject)
    gen_pointcloud :296-337                                           prepare_scene (frames paired by file stem)
    save_points3D :340-370 (np.random.choice(num, num // 8))          subsample_indices / subsample (gg_subsample)
                                                                      + write_points3d_txt (np.savetxt, same fmt)
    cal_normal :204-229                                               depth_normals (gg_depth_normals)
    gen_image_info :163-181 (c2w, not w2c)                            write_images_txt
    gen_camera_info :185-201                                          write_cameras_txt (values of transforms.json)
    k_nearest_sklearn :315-331                                        knn_distances (gg_knn)
    coloricp :47-83 (defined, never called)                           --refine-poses (register.refine_scan_poses)
    python -m gaussiangrasper_amd.prepare --scan DIR [--out DIR] [...]

No GPU work falls back to the host: a missing device is an error."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._call import (ArrayLike, default_device, grid_args, ptr as _ptr, require_hip as _require_hip, stream as _stream,
                    to_device, workspace as _ws)
from .grid import knn_grid

DEPTH_RANGE = (0.001, 1.2)       # depth_image_to_point_cloud :22
Z_RANGE = (-0.3, -0.1)           # merge_point_clouds :39
KEEP = 8                         # save_points3D :346
READERS = 16                     # reader threads at most
POINTS3D_FMT = "%d %.6f %.6f %.6f %d %d %d"   # save_points3D :365-367
COLMAP_DIR = os.path.join("colmap", "sparse", "0")

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)


# ------------------------------------------------------------------------------------------------
# subsample law (host statement; gg_subsample computes the same set on the device)
# ------------------------------------------------------------------------------------------------
def splitmix64_keys(seed: int, num: int) -> np.ndarray:
    """uint64 keys of rows 0..num-1: the SplitMix64 output function of seed + (i + 1) * 0x9E3779B97F4A7C15."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + (np.arange(1, num + 1, dtype=np.uint64) * _GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def subsample_indices(num: int, keep: int = KEEP, seed: int = 0) -> np.ndarray:
    """The rows save_points3D keeps, as a law: exactly num // keep distinct indices, a uniform subset, ascending, a
    pure function of (seed, num) — the num // keep rows with the smallest keys (splitmix64_keys; all distinct)."""
    if num < 0 or keep < 1:
        raise ValueError(f"need num >= 0 and keep >= 1, got {num}, {keep}")
    m = num // keep
    if m == 0:
        return np.zeros(0, dtype=np.int64)
    keys = splitmix64_keys(seed, num)
    return np.sort(np.argpartition(keys, m - 1)[:m]).astype(np.int64)


# ------------------------------------------------------------------------------------------------
# device calls
# ------------------------------------------------------------------------------------------------
def _frames_args(depth, intrinsics, c2w, dev):
    d = to_device(depth, torch.float64, dev)
    if d.ndim == 2:
        d = d[None]
    if d.ndim != 3:
        raise ValueError(f"depth must be (F, H, W) or (H, W), got {tuple(d.shape)}")
    f = d.shape[0]
    k = to_device(intrinsics, torch.float64, dev).reshape(-1, 4)
    if k.shape[0] == 1 and f > 1:
        k = k.expand(f, 4).contiguous()
    t = to_device(c2w, torch.float64, dev).reshape(-1, 4, 4)
    if t.shape[0] == 1 and f > 1:
        t = t.expand(f, 4, 4).contiguous()
    if k.shape[0] != f or t.shape[0] != f:
        raise ValueError(f"{f} depth frames, {k.shape[0]} intrinsics rows (fx, fy, cx, cy), {t.shape[0]} c2w matrices")
    return d, k, t


def backproject_frames(depth: ArrayLike, mask: ArrayLike, rgb: ArrayLike, intrinsics: ArrayLike, c2w: ArrayLike,
                       depth_range: Tuple[float, float] = DEPTH_RANGE,
                       z_range: Tuple[float, float] = Z_RANGE) -> Tuple[Tensor, Tensor]:
    """Frames to base-frame points (gg_backproject): depth (F, H, W) metres, mask (F, H, W) (!= 0 keeps), rgb
    (F, H, W, 3) uint8, intrinsics (F, 4) or (4,) fx, fy, cx, cy, c2w (F, 4, 4) or (4, 4).  A pixel is kept when
    mask != 0 and d_lo < d < d_hi and its base-frame z is inside z_lo < z < z_hi.  Returns points (M, 3) float64 and
    colors (M, 3) uint8 on the device, frame-major then row-major, in tensors of their own (the F*H*W-row output
    buffers are released)."""
    dev = default_device("prepare")
    d, k, t = _frames_args(depth, intrinsics, c2w, dev)
    f, h, w = d.shape
    m = mask if isinstance(mask, Tensor) else torch.as_tensor(np.asarray(mask))
    m = (m != 0).to(device=dev, dtype=torch.uint8).reshape(-1, h, w).contiguous()
    c = to_device(rgb, torch.uint8, dev)
    if m.shape[0] != f or tuple(c.shape) != (f, h, w, 3):
        raise ValueError(f"depth {tuple(d.shape)}, mask {tuple(m.shape)}, rgb {tuple(c.shape)}: need (F, H, W) and "
                         f"(F, H, W, 3)")
    lib = _lib.load()
    n = f * h * w
    if n > (1 << 30):
        raise ValueError(f"{n} pixels in one call: split the frames (frames_per_batch)")
    pts = torch.empty((n, 3), dtype=torch.float64, device=dev)
    cols = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    count = torch.zeros((), dtype=torch.int64, device=dev)
    ws = _ws(lib.gg_backproject_workspace(f, h, w), dev)
    _lib.check(lib.gg_backproject(f, h, w, _ptr(d), _ptr(m), _ptr(c), _ptr(k), _ptr(t), float(depth_range[0]),
                                  float(depth_range[1]), float(z_range[0]), float(z_range[1]), _ptr(pts), _ptr(cols),
                                  _ptr(count), _ptr(ws), ws.numel(), _stream(dev)), "gg_backproject")
    kept = int(count.item())
    return pts[:kept].clone(), cols[:kept].clone()


def _subsample_call(num: int, keep: int, seed: int, points, colors, out_p, out_c, out_i, dev) -> None:
    if num > (1 << 30):
        raise ValueError(f"{num} rows to subsample: gg_subsample takes at most 2^30 (GG_PREP_MAX_ROWS)")
    lib = _lib.load()
    ws = _ws(lib.gg_subsample_workspace(num), dev)
    _lib.check(lib.gg_subsample(num, keep, seed & 0xFFFFFFFFFFFFFFFF, _ptr(points), _ptr(colors), _ptr(out_p),
                                _ptr(out_c), _ptr(out_i), _ptr(ws), ws.numel(), _stream(dev)), "gg_subsample")


def subsample_device_indices(num: int, keep: int = KEEP, seed: int = 0) -> Tensor:
    """subsample_indices(num, keep, seed) computed on the device (gg_subsample without a gather): int64 (num // keep,),
    for rows that are not on the device (prepare_scene stages each batch's rows on the host)."""
    if num < 0 or keep < 1:
        raise ValueError(f"need num >= 0 and keep >= 1, got {num}, {keep}")
    dev = default_device("prepare")
    out_i = torch.empty(num // keep, dtype=torch.int64, device=dev)
    if num // keep:
        _subsample_call(num, keep, seed, None, None, None, None, out_i, dev)
    return out_i


def subsample(points: Tensor, colors: Tensor, keep: int = KEEP, seed: int = 0) -> Tuple[Tensor, Tensor, Tensor]:
    """The rows of subsample_indices(len(points), keep, seed), gathered on the device (gg_subsample): points
    (num // keep, 3) float64, colors (num // keep, 3) uint8 and their indices int64."""
    dev = _require_hip(points, colors)
    if points.dtype != torch.float64 or colors.dtype != torch.uint8 or points.ndim != 2 or points.shape[1] != 3 \
            or tuple(colors.shape) != tuple(points.shape):
        raise ValueError(f"points must be (N, 3) float64 and colors (N, 3) uint8, got {points.dtype} "
                         f"{tuple(points.shape)} / {colors.dtype} {tuple(colors.shape)}")
    if keep < 1:
        raise ValueError(f"keep must be >= 1, got {keep}")
    points, colors = points.contiguous(), colors.contiguous()
    num = points.shape[0]
    m = num // keep
    out_p = torch.empty((m, 3), dtype=torch.float64, device=dev)
    out_c = torch.empty((m, 3), dtype=torch.uint8, device=dev)
    out_i = torch.empty(m, dtype=torch.int64, device=dev)
    if m == 0:
        return out_p, out_c, out_i
    _subsample_call(num, keep, seed, points, colors, out_p, out_c, out_i, dev)
    return out_p, out_c, out_i


def depth_normals(depth: ArrayLike, intrinsics: ArrayLike, c2w: ArrayLike) -> Tensor:
    """cal_normal on the device (gg_depth_normals): world-frame unit normals (F, H, W, 3) float64 of depth frames
    (F, H, W) or (H, W) in metres; intrinsics (F, 4) / (4,) fx, fy, cx, cy; c2w (F, 4, 4) / (4, 4).  H, W >= 2."""
    dev = default_device("prepare")
    d, k, t = _frames_args(depth, intrinsics, c2w, dev)
    f, h, w = d.shape
    if h < 2 or w < 2:
        raise ValueError(f"normal maps need H, W >= 2 (np.gradient), got {h} x {w}")
    out = torch.empty((f, h, w, 3), dtype=torch.float64, device=dev)
    _lib.check(_lib.load().gg_depth_normals(f, h, w, _ptr(d), _ptr(k), _ptr(t), _ptr(out), _stream(dev)),
               "gg_depth_normals")
    return out


def knn_distances(points: ArrayLike, k: int = 3) -> Tuple[Tensor, Tensor]:
    """k_nearest_sklearn without the KD-tree: for every point the k smallest distances to the other points (exact:
    fp64 from the fp32 coordinates, rounded to fp32) and a neighbour set attaining them.  Returns (dist (N, k)
    float32, idx (N, k) int64) on the device.  Raises ValueError, as sklearn does, for N <= k and for non-finite
    coordinates."""
    if not 1 <= k <= 8:
        raise ValueError(f"k must be in 1..8, got {k}")
    x = points.detach() if isinstance(points, Tensor) else torch.as_tensor(np.asarray(points))
    x = x.to(torch.float32)
    if x.ndim != 2 or x.shape[1] != 3:
        raise ValueError(f"points must be (N, 3), got {tuple(x.shape)}")
    n = x.shape[0]
    if n <= k:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k + 1}, n_samples_fit = {n}")
    if n > (1 << 30):
        raise ValueError(f"{n} points: at most 2^30")
    if not bool(torch.isfinite(x).all()):
        raise ValueError("Input X contains NaN or infinity")
    x = (x if x.device.type == "cuda" else x.to(default_device("prepare"))).contiguous()
    dev = x.device
    grid_c, dims_c = grid_args(knn_grid(x))
    lib = _lib.load()
    ws = _ws(lib.gg_knn_workspace(n, dims_c), dev)
    dist = torch.empty((n, k), dtype=torch.float32, device=dev)
    idx = torch.empty((n, k), dtype=torch.int64, device=dev)
    _lib.check(lib.gg_knn(n, _ptr(x), k, grid_c, dims_c, _ptr(dist), _ptr(idx), _ptr(ws), ws.numel(), _stream(dev)),
               "gg_knn")
    return dist, idx


# ------------------------------------------------------------------------------------------------
# COLMAP text writers (what colmap_dataparser reads) and the quaternion of a pose
# ------------------------------------------------------------------------------------------------
def rotmat_to_qvec(R: ArrayLike) -> np.ndarray:
    """(w, x, y, z) unit quaternion of a rotation matrix (Shepperd's method, w >= 0), the inverse of COLMAP's
    qvec2rotmat."""
    R = np.asarray(R, dtype=np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    i = int(np.argmax([tr, R[0, 0], R[1, 1], R[2, 2]]))
    if i == 0:
        s = 2.0 * np.sqrt(1.0 + tr)
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif i == 1:
        s = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif i == 2:
        s = 2.0 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = 2.0 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.array(q)
    q /= np.linalg.norm(q)
    return -q if q[0] < 0 else q


CAMERA_KEYS = ("fl_x", "fl_y", "cx", "cy", "k1", "k2", "p1", "p2")


def camera_params(meta: Dict, frame: Optional[Dict] = None) -> Tuple[float, ...]:
    """(fx, fy, cx, cy, k1, k2, p1, p2) of a frame of transforms.json: its own values where it has them, else the
    top-level ones (distortion 0 when neither has it)."""
    frame = frame or {}
    return tuple(float(frame.get(key, meta.get(key, 0.0))) for key in CAMERA_KEYS)


def camera_ids(meta: Dict, frames: Sequence[Dict]) -> Tuple[List[Tuple[float, ...]], List[int]]:
    """The distinct camera parameter sets of the frames in order of first use, and each frame's 1-based camera id."""
    cams, ids = [], []
    for fr in frames:
        c = camera_params(meta, fr)
        if c not in cams:
            cams.append(c)
        ids.append(cams.index(c) + 1)
    return cams, ids


def write_cameras_txt(path: str, cam: Dict, params: Optional[Sequence[Sequence[float]]] = None) -> None:
    """`id OPENCV w h fx fy cx cy k1 k2 p1 p2` per camera (gen_camera_info's layout, the values of transforms.json).
    params: the parameter sets of camera_ids (default: the top-level one, as camera 1)."""
    params = params or [camera_params(cam)]
    with open(path, "w") as f:
        for i, p in enumerate(params):
            vals = [int(cam["w"]), int(cam["h"])] + [float(v) for v in p]
            f.write(f"{i + 1} OPENCV " + " ".join(str(v) for v in vals) + "\n")


def write_images_txt(path: str, c2w_list: Sequence[np.ndarray], names: Sequence[str],
                     cam_ids: Optional[Sequence[int]] = None) -> None:
    """gen_image_info: `id qw qx qy qz tx ty tz camera_id name` then `0 0 0`, holding the camera-to-base pose (this
    fork's parser reads c2w directly, colmap_dataparser.py:134-143).  cam_ids default to 1."""
    cam_ids = cam_ids or [1] * len(names)
    with open(path, "w") as f:
        for i, (T, name, cid) in enumerate(zip(c2w_list, names, cam_ids)):
            T = np.asarray(T, dtype=np.float64)
            q = rotmat_to_qvec(T[:3, :3])
            f.write(" ".join([str(i + 1)] + [str(float(v)) for v in q] + [str(float(v)) for v in T[:3, 3]]
                             + [str(int(cid)), name]) + "\n0 0 0\n")


def write_points3d_txt(path: str, points: np.ndarray, colors: np.ndarray) -> None:
    """save_points3D's file: ids from 1, np.savetxt with fmt '%d %.6f %.6f %.6f %d %d %d'."""
    m = points.shape[0]
    rows = np.concatenate((np.arange(1, m + 1, dtype=np.float64)[:, None], np.asarray(points, dtype=np.float64),
                           np.asarray(colors).astype(np.float64)), axis=1)
    np.savetxt(path, rows, fmt=POINTS3D_FMT)


# ------------------------------------------------------------------------------------------------
# scan directory -> trainer layout
# ------------------------------------------------------------------------------------------------
class ScanError(ValueError):
    pass


def read_transforms(scan_dir: str) -> Tuple[str, Dict, List[Dict]]:
    """(path, contents, frames) of a scan's transforms.json; ScanError when it is missing or lists no frames."""
    tpath = os.path.join(scan_dir, "transforms.json")
    if not os.path.exists(tpath):
        raise ScanError(f"missing file: {tpath}")
    with open(tpath) as f:
        meta = json.load(f)
    frames = meta.get("frames") or []
    if not frames:
        raise ScanError(f"{tpath} lists no frames")
    return tpath, meta, frames


def frame_files(scan: str, frame: Dict) -> Tuple[str, str, str, str]:
    """(stem, image, depth, mask) paths of a frame of transforms.json; ScanError when one is missing."""
    stem = os.path.splitext(os.path.basename(frame["file_path"]))[0]
    image = os.path.join(scan, "images", stem + ".png")
    depth = os.path.join(scan, "depths", stem + ".npy")
    mask = os.path.join(scan, "boundary_mask", stem + ".npy")
    if not os.path.exists(mask):
        mask = os.path.join(scan, "boundary_mask", stem + ".png")
    for p in (image, depth, mask):
        if not os.path.exists(p):
            raise ScanError(f"missing file for frame '{frame['file_path']}': {p}")
    return stem, image, depth, mask


def _read_mask(path: str) -> np.ndarray:
    from PIL import Image
    if path.endswith(".npy"):
        m = np.load(path)
        if m.ndim == 3 and m.shape[2] == 1:
            m = m[..., 0]
        if m.ndim == 3:
            m = np.asarray(Image.fromarray(np.ascontiguousarray(m[..., :3]).astype(np.uint8)).convert("L"))
    else:
        m = np.asarray(Image.open(path).convert("L"))
    return m != 0


def _check_sizes(files, hw: Tuple[int, int]) -> None:
    """Every frame's depth, image and mask are h x w (headers only)."""
    from PIL import Image
    _, image, depth, mask = files
    with Image.open(image) as im:
        shapes = [("image", image, (im.size[1], im.size[0]))]
    shapes.append(("depth", depth, np.load(depth, mmap_mode="r").shape))
    if mask.endswith(".npy"):
        shapes.append(("mask", mask, np.load(mask, mmap_mode="r").shape[:2]))
    else:
        with Image.open(mask) as im:
            shapes.append(("mask", mask, (im.size[1], im.size[0])))
    for what, path, shape in shapes:
        if tuple(shape) != hw:
            raise ScanError(f"{what} {path} has shape {tuple(shape)}, transforms.json gives h x w = {hw[0]} x {hw[1]}")


def read_frame(files, units: float):
    """(depth (H, W) fp64 metres, mask (H, W) bool, rgb (H, W, 3) uint8) of a frame's frame_files."""
    from PIL import Image
    _, image, depth, mask = files
    rgb = np.asarray(Image.open(image).convert("RGB"))
    d = np.load(depth).astype(np.float64) / units
    return d, _read_mask(mask), rgb


def prepare_scene(scan_dir: str, out_dir: Optional[str] = None, keep: int = KEEP, seed: int = 0,
                  depth_units_per_metre: float = 1.0, depth_range: Tuple[float, float] = DEPTH_RANGE,
                  z_range: Tuple[float, float] = Z_RANGE, frames_per_batch: int = 16, normal_vis: bool = False,
                  force: bool = False, refine_poses: bool = False, refine_options: Optional[Dict] = None) -> Dict:
    """Scan directory (transforms.json, images/, depths/, boundary_mask/) -> colmap/sparse/0/{cameras, images,
    points3D}.txt and normals/<stem>.npy (+ normal_vis/<stem>.png) under out_dir (default: the scan directory).
    Frames are paired by the stem of each frame's file_path; depth in metres is raw / depth_units_per_metre.
    refine_poses (off by default): the frames' poses are first refined by frame-to-model coloured ICP
    (register.refine_scan_poses, keyword arguments in refine_options); the refined camera-to-base matrices go into
    images.txt, the seed cloud and the normal maps, and transforms_refined.json and refine_report.json are written
    next to them.  Returns counts and the timing breakdown (seconds: read, gpu, write)."""
    out_dir = out_dir or scan_dir
    if keep < 1 or frames_per_batch < 1 or not depth_units_per_metre > 0:
        raise ScanError("keep and frames_per_batch must be >= 1, depth_units_per_metre > 0")
    tpath, meta, frames = read_transforms(scan_dir)
    for key in ("fl_x", "fl_y", "cx", "cy", "w", "h"):
        if key not in meta and not (key in ("fl_x", "fl_y", "cx", "cy") and all(key in fr for fr in frames)):
            raise ScanError(f"{tpath} has no top-level '{key}'")
    hw = (int(meta["h"]), int(meta["w"]))
    files = [frame_files(scan_dir, fr) for fr in frames]
    for fl in files:
        _check_sizes(fl, hw)
    stems = [f[0] for f in files]
    if len(set(stems)) != len(stems):
        raise ScanError("two frames share a file stem")
    colmap = os.path.join(out_dir, COLMAP_DIR)
    outputs = [os.path.join(colmap, n) for n in ("cameras.txt", "images.txt", "points3D.txt")]
    outputs += [os.path.join(out_dir, "normals", s + ".npy") for s in stems]
    if normal_vis:
        outputs += [os.path.join(out_dir, "normal_vis", s + ".png") for s in stems]
    if refine_poses:
        outputs += [os.path.join(out_dir, n) for n in ("transforms_refined.json", "refine_report.json")]
    existing = [p for p in outputs if os.path.exists(p)]
    if existing and not force:
        raise ScanError(f"{len(existing)} output file(s) exist, e.g. {existing[0]}: pass force=True (--force)")
    os.makedirs(colmap, exist_ok=True)
    os.makedirs(os.path.join(out_dir, "normals"), exist_ok=True)
    if normal_vis:
        os.makedirs(os.path.join(out_dir, "normal_vis"), exist_ok=True)
    c2w = np.array([np.asarray(fr["transform_matrix"], dtype=np.float64) for fr in frames])
    cams, cam_ids = camera_ids(meta, frames)
    intr = np.array([cams[i - 1][:4] for i in cam_ids], dtype=np.float64)
    dev = default_device("prepare")
    t_read = t_gpu = t_write = 0.0
    refined = None
    if refine_poses:
        t0 = time.perf_counter()
        c2w, refined = _refine_poses(files, float(depth_units_per_metre), intr, c2w, depth_range, z_range,
                                     refine_options or {})
        t_gpu += time.perf_counter() - t0
    clouds, colours, pending = [], [], []
    with ThreadPoolExecutor(max_workers=max(1, min(READERS, os.cpu_count() or 1))) as pool:
        for b0 in range(0, len(frames), frames_per_batch):
            b1 = min(len(frames), b0 + frames_per_batch)
            t0 = time.perf_counter()
            got = list(pool.map(lambda fl: read_frame(fl, float(depth_units_per_metre)), files[b0:b1]))
            depth = torch.from_numpy(np.stack([g[0] for g in got]))
            mask = torch.from_numpy(np.stack([g[1] for g in got]).astype(np.uint8))
            rgb = torch.from_numpy(np.stack([g[2] for g in got]))
            t1 = time.perf_counter()
            depth = depth.to(dev)
            pts, cols = backproject_frames(depth, mask, rgb, intr[b0:b1], c2w[b0:b1], depth_range, z_range)
            nrm = depth_normals(depth, intr[b0:b1], c2w[b0:b1]).cpu().numpy()
            clouds.append(pts.cpu().numpy())       # staged on the host: device memory stays per batch
            colours.append(cols.cpu().numpy())
            del pts, cols, depth
            t2 = time.perf_counter()
            for s_, n_ in zip(stems[b0:b1], nrm):
                pending.append(pool.submit(_write_normal, out_dir, s_, n_, normal_vis))
            for p in pending:
                p.result()
            pending = []
            t3 = time.perf_counter()
            t_read += t1 - t0
            t_gpu += t2 - t1
            t_write += t3 - t2
    t0 = time.perf_counter()
    num = sum(c.shape[0] for c in clouds)
    if num > (1 << 30):
        raise ScanError(f"{num} points pass the depth and workspace windows, more than the 2^30 one subsample takes: "
                        f"narrow --depth-range / --z-range or prepare the frames in parts")
    allp = np.concatenate(clouds) if len(clouds) > 1 else clouds[0]
    allc = np.concatenate(colours) if len(colours) > 1 else colours[0]
    sel = subsample_device_indices(num, keep, seed).cpu().numpy()
    sp, sc = allp[sel], allc[sel]
    t1 = time.perf_counter()
    write_cameras_txt(outputs[0], meta, cams)
    write_images_txt(outputs[1], list(c2w), [os.path.basename(fr["file_path"]) for fr in frames], cam_ids)
    write_points3d_txt(outputs[2], sp, sc)
    if refined is not None:
        out_meta = dict(meta)
        out_meta["frames"] = [dict(fr, transform_matrix=T.tolist()) for fr, T in zip(frames, c2w)]
        with open(os.path.join(out_dir, "transforms_refined.json"), "w") as f:
            json.dump(out_meta, f, indent=1)
        with open(os.path.join(out_dir, "refine_report.json"), "w") as f:
            json.dump([dict(row, name=os.path.basename(fr["file_path"])) for row, fr in zip(refined.report, frames)],
                      f, indent=1)
    t2 = time.perf_counter()
    t_gpu += t1 - t0
    t_write += t2 - t1
    return {"frames": len(frames), "height": hw[0], "width": hw[1], "points": int(allp.shape[0]),
            "seed_points": int(sp.shape[0]), "read_s": t_read, "gpu_s": t_gpu, "write_s": t_write,
            "out_dir": out_dir, **({"refined_frames": int(sum(refined.accepted)) - 1} if refined is not None else {})}


def _refine_poses(files, units: float, intr: np.ndarray, c2w: np.ndarray, depth_range, z_range, options: Dict):
    """(refined c2w (F, 4, 4), the ScanRefinement): every frame back-projected on its own at its given pose,
    voxel-downsampled at the finest voxel size, then register.refine_scan_poses."""
    from .register import VOXEL_RADIUS, refine_scan_poses, voxel_downsample
    finest = min(options.get("voxel_radius", VOXEL_RADIUS)) * float(options.get("scale", 1.0))
    clouds = []
    for k, fl in enumerate(files):
        d, m, rgb = read_frame(fl, units)
        pts, cols = backproject_frames(d[None], m[None], rgb[None], intr[k:k + 1], c2w[k:k + 1], depth_range, z_range)
        clouds.append(voxel_downsample(pts, cols.double() / 255.0, finest))
    ref = refine_scan_poses(clouds, **options)
    return np.array([ref.corrections[k] @ c2w[k] for k in range(len(files))]), ref


def _write_normal(out_dir: str, stem: str, n: np.ndarray, vis: bool) -> None:
    np.save(os.path.join(out_dir, "normals", stem + ".npy"), n)
    if vis:
        from PIL import Image
        Image.fromarray(np.uint8((n + 1) / 2 * 255)).save(os.path.join(out_dir, "normal_vis", stem + ".png"))


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.prepare",
                                 description="RGB-D scan directory -> COLMAP text files and normal maps for training")
    ap.add_argument("--scan", required=True, help="directory with transforms.json, images/, depths/, boundary_mask/")
    ap.add_argument("--out", default=None, help="output root (default: the scan directory)")
    ap.add_argument("--keep", type=int, default=KEEP, help="keep num // KEEP seed points (default 8)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--depth-units-per-metre", type=float, default=1.0, help="1000 for millimetre depth files")
    ap.add_argument("--depth-range", type=float, nargs=2, default=DEPTH_RANGE, metavar=("LO", "HI"))
    ap.add_argument("--z-range", type=float, nargs=2, default=Z_RANGE, metavar=("LO", "HI"))
    ap.add_argument("--frames-per-batch", type=int, default=16)
    ap.add_argument("--normal-vis", action="store_true", help="also write normal_vis/<stem>.png")
    ap.add_argument("--force", action="store_true", help="overwrite existing outputs")
    ap.add_argument("--refine-poses", action="store_true",
                    help="refine the frames' poses by frame-to-model coloured ICP first; also writes "
                         "transforms_refined.json and refine_report.json")
    a = ap.parse_args(argv)
    try:
        r = prepare_scene(a.scan, a.out, keep=a.keep, seed=a.seed, depth_units_per_metre=a.depth_units_per_metre,
                          depth_range=tuple(a.depth_range), z_range=tuple(a.z_range),
                          frames_per_batch=a.frames_per_batch, normal_vis=a.normal_vis, force=a.force,
                          refine_poses=a.refine_poses)
    except ScanError as exc:
        print(f"error: {exc}", file=sys.stderr)
        return 2
    print(f"{r['frames']} frames {r['width']}x{r['height']}: {r['points']} points, {r['seed_points']} seed points "
          f"-> {r['out_dir']}")
    print(f"time: read/decode {r['read_s']:.3f} s, gpu {r['gpu_s']:.3f} s, write {r['write_s']:.3f} s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
