"""Mesh export: a triangle mesh of the trained field, of one queried object, or of a raw RGB-D scan — what the
reference advertises through nerfstudio's `ns-export tsdf` (scripts/exporter.py, exporter/tsdf_utils.py), which
cannot run on the splatting model (its `render_trajectory` gets `{}` back from `get_outputs` for a ray bundle) and
needs skimage, pymeshlab and open3d.  Depth frames are fused into a TSDF volume and its zero level set extracted by
marching tetrahedra on two HIP calls (`gg_tsdf_integrate`, `gg_tsdf_mesh_count` / `gg_tsdf_mesh_emit`,
csrc/tsdf.hip).  The contract is in include/gg_raster.h, the deliberate differences from the reference in PARITY.md
"Mesh export", the design in DESIGN.md §3.16.

    reference (nerfstudio)                           here
    TSDF.from_aabb (tsdf_utils.py)                   TSDFVolume(bbox_min, bbox_max, resolution)
    TSDF.integrate_tsdf                              TSDFVolume.integrate (projective z, plain running mean)
    render_trajectory (exporter_utils.py)            render_depth (the library's own operators, depth = D / A, or
                                                     depth_mode="median": the median Gaussian's, surface.py)
    TSDF.get_mesh (skimage marching cubes)           TSDFVolume.extract (marching tetrahedra, observed cells)
    export_tsdf_mesh + pymeshlab save                mesh_model / mesh_scan + write_ply_mesh
    ns-export tsdf --resolution 128 --downscale 2    python -m gaussiangrasper_amd.mesh --ckpt ... | --scan ...

No GPU work falls back to the host: a missing device is an error."""
from __future__ import annotations

import argparse
import json
import os
import sys
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._call import (ArrayLike, default_device, host_ptr, ptr as _ptr, require_hip as _require_hip, stream as _stream,
                    workspace as _ws)
from ._cli import (add_object_options, add_support_options, check_object_options, check_support_options,
                   object_mask)
from .frames import c2w_to_scene, directions_from_scene, homogeneous, load_transform_json, points_from_scene

RESOLUTION = 128                 # the reference exporter's defaults
DOWNSCALE = 2
BBOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
TRUNCATION_VOXELS = 5.0          # TSDF.from_aabb's truncation margin, in voxels of x
ALPHA_MIN = 0.5
GL_TO_CV = np.diag([1.0, -1.0, -1.0, 1.0])   # nerfstudio / OpenGL camera axes <-> OpenCV camera axes


@dataclass
class Mesh:
    """vertices (Nv, 3) fp32, faces (Nf, 3) int32, normals (Nv, 3) fp32 (unit or zero), colors (Nv, 3) fp32 in
    [0, 1] or None.  Device tensors from TSDFVolume.extract; numpy arrays from read_ply_mesh."""
    vertices: Union[Tensor, np.ndarray]
    faces: Union[Tensor, np.ndarray]
    normals: Union[Tensor, np.ndarray]
    colors: Optional[Union[Tensor, np.ndarray]] = None

    def numpy(self) -> "Mesh":
        f = lambda t: t.detach().cpu().numpy() if isinstance(t, Tensor) else t  # noqa: E731
        return Mesh(f(self.vertices), f(self.faces), f(self.normals), f(self.colors))


# ------------------------------------------------------------------------------------------------
# frames: the one place camera axes are converted
# ------------------------------------------------------------------------------------------------
def opencv_w2c(c2w_gl: ArrayLike) -> np.ndarray:
    """(V, 3, 4) fp64 world-to-camera with OpenCV axes (x right, y down, z forward) of nerfstudio / OpenGL
    camera-to-world matrices (V, 3|4, 4) or one (3|4, 4): inv(c2w diag(1, -1, -1, 1))."""
    a = homogeneous(c2w_gl)
    one = a.ndim == 2
    a = a[None] if one else a
    w2c = np.linalg.inv(a @ GL_TO_CV)[:, :3, :]
    return w2c


def opencv_to_opengl_c2w(c2w_cv: ArrayLike) -> np.ndarray:
    """OpenCV camera-to-world (.., 3|4, 4) -> nerfstudio / OpenGL camera-to-world (.., 4, 4) (flip y and z)."""
    return homogeneous(c2w_cv) @ GL_TO_CV


def dataparser_transform(path_or_dict) -> Tuple[np.ndarray, float]:
    """(transform_matrix (4, 4) fp64, scale) of a nerfstudio dataparser_transforms.json (or its dict)."""
    M, scale = load_transform_json(path_or_dict)
    return homogeneous(M), scale


# ------------------------------------------------------------------------------------------------
# the volume
# ------------------------------------------------------------------------------------------------
def _triple(v, name: str, kind=float) -> Tuple:
    t = tuple(kind(x) for x in (np.broadcast_to(np.asarray(v), (3,)) if np.ndim(v) <= 1 else np.asarray(v).ravel()))
    if len(t) != 3:
        raise ValueError(f"{name} must be a scalar or 3 values, got {v}")
    return t


class TSDFVolume:
    """Dense TSDF volume over the box [bbox_min, bbox_max): resolution lattice points per axis (one int or three),
    point (i, j, k) at bbox_min + (i, j, k) * voxel_size with voxel_size = (bbox_max - bbox_min) / resolution (the
    reference's TSDF.from_aabb grid), C-ordered [X][Y][Z].  truncation defaults to 5 voxels of x.  Starts with
    tsdf 1, weight 0; colour only once a frame with rgb is integrated."""

    def __init__(self, bbox_min: ArrayLike = BBOX[0], bbox_max: ArrayLike = BBOX[1], resolution=RESOLUTION,
                 truncation: Optional[float] = None, device=None):
        lo = np.asarray(_triple(bbox_min, "bbox_min"), dtype=np.float64)
        hi = np.asarray(_triple(bbox_max, "bbox_max"), dtype=np.float64)
        self.dims = np.asarray(_triple(resolution, "resolution", int), dtype=np.int32)
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
            raise ValueError(f"need finite bbox_min < bbox_max, got {lo.tolist()} / {hi.tolist()}")
        self.voxel_size = ((hi - lo) / self.dims).astype(np.float32)
        self.origin = lo.astype(np.float32)
        self.grid = np.concatenate([self.origin, self.voxel_size]).astype(np.float32)
        self.truncation = float(np.float32(TRUNCATION_VOXELS * float(self.voxel_size[0]) if truncation is None
                                           else truncation))
        if not (np.isfinite(self.truncation) and self.truncation > 0):
            raise ValueError(f"truncation must be finite and > 0, got {truncation}")
        lib = _lib.load()
        if lib.gg_tsdf_mesh_workspace(host_ptr(self.dims)) == 0:
            raise ValueError(f"volume {self.dims.tolist()}: each side must be 1..4096 and the product at most 2^27 "
                             f"points (gg_raster.h GG_TSDF_MAX_*)")
        self.device = torch.device(device) if device is not None else default_device("mesh")
        shape = tuple(int(d) for d in self.dims)
        self.tsdf = torch.ones(shape, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.color: Optional[Tensor] = None
        self.color_weight: Optional[Tensor] = None

    def integrate_w2c(self, depth: Tensor, intrinsics: ArrayLike, w2c: ArrayLike, rgb: Optional[Tensor] = None):
        """depth (V, H, W) or (H, W) (> 0 observed, +inf free space, 0 / NaN nothing), intrinsics (V, 4) fx, fy,
        cx, cy, w2c (V, 3, 4) OpenCV world-to-camera, rgb (V, H, W, 3) in [0, 1] or None: one gg_tsdf_integrate."""
        dev = self.device
        d = depth.detach().to(device=dev, dtype=torch.float32)
        d = (d[None] if d.ndim == 2 else d).contiguous()
        if d.ndim != 3:
            raise ValueError(f"depth must be (V, H, W) or (H, W), got {tuple(depth.shape)}")
        V, H, W = d.shape
        K = torch.as_tensor(np.asarray(intrinsics, dtype=np.float32).reshape(-1, 4), device=dev).contiguous()
        E = torch.as_tensor(np.asarray(w2c, dtype=np.float32).reshape(-1, 3, 4), device=dev).contiguous()
        if K.shape[0] != V or E.shape[0] != V:
            raise ValueError(f"{V} depth frames, {K.shape[0]} intrinsics, {E.shape[0]} poses")
        c = None
        if rgb is not None:
            c = rgb.detach().to(device=dev, dtype=torch.float32)
            c = (c[None] if c.ndim == 3 else c).contiguous()
            if tuple(c.shape) != (V, H, W, 3):
                raise ValueError(f"rgb must be ({V}, {H}, {W}, 3), got {tuple(rgb.shape)}")
            if self.color is None:
                self.color = torch.zeros(tuple(int(x) for x in self.dims) + (3,), dtype=torch.float32, device=dev)
                self.color_weight = torch.zeros_like(self.weight)
        _lib.check(_lib.load().gg_tsdf_integrate(
            host_ptr(self.dims), host_ptr(self.grid), self.truncation, V, H, W, _ptr(d), _ptr(c), _ptr(K), _ptr(E),
            _ptr(self.tsdf), _ptr(self.weight), _ptr(self.color if c is not None else None),
            _ptr(self.color_weight if c is not None else None), _stream(dev)), "gg_tsdf_integrate")
        return self

    def integrate(self, depth: Tensor, intrinsics: ArrayLike, c2w: ArrayLike, rgb: Optional[Tensor] = None):
        """Like integrate_w2c with nerfstudio / OpenGL camera-to-world poses (V, 3|4, 4), as camera.view_from_c2w
        takes them."""
        return self.integrate_w2c(depth, intrinsics, opencv_w2c(c2w), rgb)

    def extract(self) -> Mesh:
        """The zero level set of the observed cells (gg_tsdf_mesh_count, one read-back of the two counts,
        gg_tsdf_mesh_emit).  Colours when a frame with rgb was integrated."""
        dev, lib = self.device, _lib.load()
        ws = _ws(lib.gg_tsdf_mesh_workspace(host_ptr(self.dims)), dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(lib.gg_tsdf_mesh_count(host_ptr(self.dims), _ptr(self.tsdf), _ptr(self.weight), _ptr(counts),
                                          _ptr(ws), ws.numel(), _stream(dev)), "gg_tsdf_mesh_count")
        nv, nf = (int(x) for x in counts.cpu().tolist())
        if nv < 0 or nf < 0:
            raise _lib.GGError("gg_tsdf_mesh_count: the prefix scan gave up")
        verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        nrms = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        cols = torch.empty((nv, 3), dtype=torch.float32, device=dev) if self.color is not None else None
        faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        _lib.check(lib.gg_tsdf_mesh_emit(host_ptr(self.dims), host_ptr(self.grid), _ptr(self.tsdf), _ptr(self.color),
                                         nv, nf, _ptr(verts), _ptr(nrms), _ptr(cols), _ptr(faces), _ptr(ws), ws.numel(),
                                         _stream(dev)), "gg_tsdf_mesh_emit")
        return Mesh(verts, faces, nrms, cols)


# ------------------------------------------------------------------------------------------------
# depth of the Gaussian field
# ------------------------------------------------------------------------------------------------
DEPTH_MODES = ("expected", "median")


def check_depth_mode(depth_mode: str) -> str:
    if depth_mode not in DEPTH_MODES:
        raise ValueError(f"depth_mode must be one of {', '.join(DEPTH_MODES)}, got {depth_mode!r}")
    return depth_mode


@torch.no_grad()
def render_depth(model_or_scene, c2w: ArrayLike, intrinsics: ArrayLike, height: int, width: int,
                 mask: Optional[Tensor] = None, alpha_min: float = ALPHA_MIN,
                 depth_mode: str = "expected") -> Tuple[Tensor, Tensor, Tensor]:
    """(depth (H, W), rgb (H, W, 3), alpha (H, W)) of a model or Scene from one nerfstudio / OpenGL c2w, through the
    library's operators with eval semantics (the full SH degree).  One extra segment of colour (z, 1) over a (0, 0)
    background gives D = sum w z and A = sum w; depth = D / A where A >= alpha_min, +inf (free space) elsewhere;
    rgb = the rendered colour / A.  mask (N,) bool renders only the selected Gaussians.
    depth_mode "median": depth is the depth of the Gaussian at which the transmittance falls to <= 0.5
    (ops.blend_hits on the same tile lists), +inf where it never does — always the depth of a real Gaussian, where D / A
    lies between two surfaces that share a pixel; t_hit = 0.5 plays the role of alpha_min, which is then not used."""
    from . import ops
    from .camera import view_from_c2w
    from .constants import deg_from_sh
    check_depth_mode(depth_mode)
    src = model_or_scene
    means, scales, quats = src.means.detach(), src.scales.detach(), src.quats.detach()
    opac, sh = src.opacities.detach(), src.colors_all.detach()
    dev = _require_hip(means, scales, quats, opac, sh)
    if mask is not None:
        mask = mask.reshape(-1).to(device=dev, dtype=torch.bool)
        if mask.shape[0] != means.shape[0]:
            raise ValueError(f"mask has {mask.shape[0]} entries for {means.shape[0]} Gaussians")
        means, scales, quats, opac, sh = means[mask], scales[mask], quats[mask], opac[mask], sh[mask]
    fx, fy, cx, cy = (float(x) for x in np.asarray(intrinsics, dtype=np.float64).reshape(4))
    h, w = int(height), int(width)
    view = view_from_c2w(torch.as_tensor(homogeneous(c2w)), fx, fy, cx, cy, h, w, dev)
    if means.shape[0] == 0:
        return (torch.full((h, w), float("inf"), device=dev), torch.zeros((h, w, 3), device=dev),
                torch.zeros((h, w), device=dev))
    means = means.float().contiguous()
    xys, depths, radii, conics, num_tiles_hit, _ = ops.ProjectGaussians.apply(
        means, torch.exp(scales.float()), 1, (quats / quats.norm(dim=-1, keepdim=True)).float(),
        view.viewmat[:3, :], view.projmat, fx, fy, cx, cy, h, w, view.tile_bounds)
    config = getattr(src, "config", None)
    degree = int(config.sh_degree) if config is not None else deg_from_sh(sh.shape[1])
    if degree > 0:
        viewdirs = means - view.cam_pos.to(dev)
        viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
        rgbs = torch.clamp(ops.SphericalHarmonics.apply(degree, viewdirs, sh.float().contiguous()) + 0.5, 0.0, 1.0)
    else:
        rgbs = torch.sigmoid(sh[:, 0, :].float())
    zw = torch.stack([depths, torch.ones_like(depths)], dim=1).contiguous()
    op = torch.sigmoid(opac.float()).reshape(-1, 1).contiguous()
    rgb, za = ops.rasterize_segments(xys, depths, radii, conics, num_tiles_hit, op, h, w,
                                     [(rgbs.contiguous(), torch.zeros(3, device=dev)),
                                      (zw, torch.zeros(2, device=dev))])
    D, A = za[..., 0], za[..., 1]
    hit = A >= float(alpha_min)
    depth = torch.where(hit, D / A, torch.full_like(D, float("inf")))
    if depth_mode == "median":       # what surface.view_hits(full=False).depth holds, on this call's projection
        from .surface import hit_depth
        depth = hit_depth(depths, ops.blend_hits(xys, depths, radii, conics, num_tiles_hit, op, h, w, full=False)[0])
    rgb = torch.where(A[..., None] > 0, rgb / A[..., None].clamp_min(1e-12), torch.zeros_like(rgb)).clamp(0.0, 1.0)
    return depth, rgb, A


def _scaled_intrinsics(K: np.ndarray, h: int, w: int, downscale: float) -> Tuple[np.ndarray, int, int]:
    s = 1.0 / float(downscale)
    return K * s, int(h * s), int(w * s)


def mesh_model(model_or_scene, cameras: Sequence[Tuple[ArrayLike, ArrayLike, int, int]], bbox=BBOX,
               resolution=RESOLUTION, downscale: float = DOWNSCALE, mask: Optional[Tensor] = None,
               truncation: Optional[float] = None, alpha_min: float = ALPHA_MIN, batch: int = 16,
               color: bool = True, depth_mode: str = "expected") -> Mesh:
    """Mesh of a model or Scene (of the Gaussians `mask` selects): every camera (c2w OpenGL (3|4, 4), intrinsics
    fx, fy, cx, cy, height, width) rendered at 1 / downscale of its size, fused in batches of `batch` frames.
    depth_mode: render_depth's ("median": no skirt where a front object and the background share a pixel)."""
    check_depth_mode(depth_mode)
    if downscale <= 0:
        raise ValueError(f"downscale must be > 0, got {downscale}")
    vol = TSDFVolume(bbox[0], bbox[1], resolution, truncation, device=model_or_scene.means.device)
    frames = []
    for c2w, K, h, w in cameras:
        Ks, hs, ws = _scaled_intrinsics(np.asarray(K, dtype=np.float64).reshape(4), int(h), int(w), downscale)
        frames.append((c2w, Ks, hs, ws))
    by_size = {}
    for fr in frames:
        by_size.setdefault((fr[2], fr[3]), []).append(fr)
    for (hs, ws), group in by_size.items():
        for b0 in range(0, len(group), batch):
            part = group[b0:b0 + batch]
            rendered = [render_depth(model_or_scene, c2w, K, hs, ws, mask, alpha_min, depth_mode) for c2w, K, _, _ in part]
            depth = torch.stack([r[0] for r in rendered])
            rgb = torch.stack([r[1] for r in rendered]) if color else None
            vol.integrate(depth, np.stack([p[1] for p in part]), np.stack([homogeneous(p[0]) for p in part]), rgb)
    return vol.extract()


def scan_frames(scan_dir: str, depth_units_per_metre: float = 1.0):
    """Frames of a scan directory as prepare reads them: yields (depth (H, W) fp32 metres, rgb (H, W, 3) fp32 in
    [0, 1], intrinsics (4,), c2w OpenCV (4, 4) in the scan's raw frame).  Pixels outside the boundary mask and sensor
    zeros are 0 (no observation)."""
    from .prepare import camera_params, frame_files, read_frame, read_transforms
    _, meta, frames = read_transforms(scan_dir)
    for fr in frames:
        d, m, rgb = read_frame(frame_files(scan_dir, fr), float(depth_units_per_metre))
        d = np.where(m & np.isfinite(d) & (d > 0), d, 0.0).astype(np.float32)
        yield (d, rgb.astype(np.float32) / 255.0, np.asarray(camera_params(meta, fr)[:4], dtype=np.float64),
               homogeneous(np.asarray(fr["transform_matrix"], dtype=np.float64)))


def mesh_scan(scan_dir: str, bbox=BBOX, resolution=RESOLUTION, truncation: Optional[float] = None,
              depth_units_per_metre: float = 1.0, batch: int = 16, color: bool = True, device=None) -> Mesh:
    """Mesh of the raw RGB-D frames of a scan directory (transforms.json, images/, depths/, boundary_mask/), in the
    scan's raw frame."""
    vol = TSDFVolume(bbox[0], bbox[1], resolution, truncation, device=device)
    buf = []

    def flush():
        if not buf:
            return
        depth = torch.from_numpy(np.stack([b[0] for b in buf]))
        rgb = torch.from_numpy(np.stack([b[1] for b in buf])) if color else None
        w2c = np.linalg.inv(np.stack([b[3] for b in buf]))[:, :3, :]
        vol.integrate_w2c(depth, np.stack([b[2] for b in buf]), w2c, rgb)
        buf.clear()

    shape = None
    for fr in scan_frames(scan_dir, depth_units_per_metre):
        if shape is not None and fr[0].shape != shape:
            flush()
        shape = fr[0].shape
        buf.append(fr)
        if len(buf) == batch:
            flush()
    flush()
    return vol.extract()


# ------------------------------------------------------------------------------------------------
# PLY, binary little endian (no pymeshlab)
# ------------------------------------------------------------------------------------------------
_VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                          ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def write_ply_mesh(path: str, mesh: Mesh) -> None:
    """Vertices x, y, z, nx, ny, nz (float), red, green, blue (uchar, round(255 c), 0 without colours); faces as
    `vertex_indices` (uchar count, int triples)."""
    m = mesh.numpy()
    v = np.asarray(m.vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(m.faces, dtype=np.int32).reshape(-1, 3)
    rows = np.zeros(v.shape[0], _VERTEX_DTYPE)
    rows["x"], rows["y"], rows["z"] = v[:, 0], v[:, 1], v[:, 2]
    n = np.asarray(m.normals, dtype=np.float32).reshape(-1, 3)
    rows["nx"], rows["ny"], rows["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if m.colors is not None:
        c = np.clip(np.rint(np.asarray(m.colors, dtype=np.float64).reshape(-1, 3) * 255.0), 0, 255).astype(np.uint8)
        rows["red"], rows["green"], rows["blue"] = c[:, 0], c[:, 1], c[:, 2]
    fr = np.zeros(f.shape[0], _FACE_DTYPE)
    fr["n"] = 3
    fr["v"] = f
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {v.shape[0]}\n"
              "property float x\nproperty float y\nproperty float z\n"
              "property float nx\nproperty float ny\nproperty float nz\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              f"element face {f.shape[0]}\n"
              "property list uchar int vertex_indices\nend_header\n")
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(rows.tobytes())
        fh.write(fr.tobytes())


def read_ply_mesh(path: str) -> Mesh:
    """What write_ply_mesh writes: numpy vertices, faces, normals and colours (uchar / 255)."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = data[:end].decode("ascii").splitlines()
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError(f"{path}: only binary_little_endian PLY is read")
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("element ")}
    props = [ln.split()[-1] for ln in lines if ln.startswith("property ") and "list" not in ln]
    if props != list(_VERTEX_DTYPE.names):
        raise ValueError(f"{path}: unexpected vertex properties {props}")
    off = end + len(b"end_header\n")
    nv, nf = counts.get("vertex", 0), counts.get("face", 0)
    rows = np.frombuffer(data, _VERTEX_DTYPE, nv, off)
    fr = np.frombuffer(data, _FACE_DTYPE, nf, off + nv * _VERTEX_DTYPE.itemsize)
    if nf and (fr["n"] != 3).any():
        raise ValueError(f"{path}: only triangles are read")
    v = np.stack([rows["x"], rows["y"], rows["z"]], axis=1).astype(np.float32)
    n = np.stack([rows["nx"], rows["ny"], rows["nz"]], axis=1).astype(np.float32)
    c = np.stack([rows["red"], rows["green"], rows["blue"]], axis=1).astype(np.float32) / 255.0
    return Mesh(v, np.ascontiguousarray(fr["v"], dtype=np.int32).reshape(-1, 3), n, c)


# ------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------
def transforms_cameras(transforms_json: str) -> list:
    """(c2w OpenCV (4, 4), intrinsics (4,), h, w) of every frame of a scan's transforms.json (per-frame overrides)."""
    from .prepare import camera_params
    with open(transforms_json) as f:
        meta = json.load(f)
    frames = meta.get("frames") or []
    if not frames:
        raise ValueError(f"{transforms_json} lists no frames")
    return [(homogeneous(np.asarray(fr["transform_matrix"], dtype=np.float64)),
             np.asarray(camera_params(meta, fr)[:4], dtype=np.float64), int(fr.get("h", meta["h"])),
             int(fr.get("w", meta["w"]))) for fr in frames]


def _checkpoint_mesh(a, bbox) -> Tuple[Mesh, Optional[Tuple[np.ndarray, float]]]:
    from .interop import load_checkpoint
    scene, mlp_state, _ = load_checkpoint(a.ckpt)
    dev = default_device("mesh")
    scene = scene.to(dev)
    tf = dataparser_transform(a.transform_json) if a.transform_json else None
    cams = []
    for c2w_cv, K, h, w in transforms_cameras(a.transforms):
        if tf is not None:
            c2w_cv = c2w_to_scene(c2w_cv, *tf)
        cams.append((opencv_to_opengl_c2w(c2w_cv), K, h, w))
    mask = object_mask(a, scene, mlp_state)
    if mask is not None and not bool(mask.any()):
        raise ValueError("the query selects no Gaussian")
    mesh = mesh_model(scene, cams, bbox, a.resolution, a.downscale, mask, depth_mode=a.depth_mode)
    return mesh, tf


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.mesh",
                                 description="Triangle mesh (PLY) of a checkpoint's Gaussians, of one queried object, "
                                             "or of a raw RGB-D scan: TSDF fusion and marching tetrahedra.")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--ckpt", help="step-*.ckpt of a splatting model (needs --transforms)")
    src.add_argument("--scan", help="scan directory (transforms.json, images/, depths/, boundary_mask/)")
    ap.add_argument("--transforms", help="with --ckpt: the scan's transforms.json (OpenCV c2w, raw frame) whose "
                                         "cameras are rendered")
    ap.add_argument("--transform-json", help="with --ckpt: dataparser_transforms.json (transform_matrix, scale) "
                                             "from the scan's frame to the checkpoint's; outputs go back to the scan's")
    ap.add_argument("--out", required=True, help="output .ply")
    ap.add_argument("--bbox", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                    help="volume box (checkpoint frame for --ckpt, default [-1, 1]^3)")
    ap.add_argument("--resolution", type=int, default=RESOLUTION, help="lattice points per axis")
    ap.add_argument("--downscale", type=float, default=DOWNSCALE, help="render at 1 / K of each camera's size")
    ap.add_argument("--depth-mode", choices=DEPTH_MODES, default="expected",
                    help="with --ckpt: the depth fused per pixel: the expected depth D / A, or the depth of the median "
                         "Gaussian (transmittance 0.5)")
    ap.add_argument("--depth-units", type=float, default=1.0, help="with --scan: raw depth units per metre")
    add_object_options(ap, "mesh only the Gaussians the query selects")
    add_support_options(ap, grasp=False)
    ap.add_argument("--out-points", help="also write the mesh vertices as an (N, 3) float64 .npy (object points)")
    a = ap.parse_args(argv)
    if a.ckpt and not a.transforms:
        ap.error("--ckpt needs --transforms")
    if a.scan and (a.transforms or a.transform_json or a.positives):
        ap.error("--transforms, --transform-json and --positives go with --ckpt")
    if a.scan and a.depth_mode != "expected":
        ap.error("--depth-mode goes with --ckpt")
    check_object_options(ap, a, "none")
    check_support_options(ap, a, grasp=False)
    if a.resolution < 2 or a.downscale <= 0:
        ap.error("--resolution must be >= 2 and --downscale > 0")
    bbox = BBOX if a.bbox is None else (tuple(a.bbox[:3]), tuple(a.bbox[3:]))
    try:
        if a.ckpt:
            mesh, tf = _checkpoint_mesh(a, bbox)
        else:
            mesh, tf = mesh_scan(a.scan, bbox, a.resolution, depth_units_per_metre=a.depth_units), None
    except (KeyError, ValueError, OSError, _lib.GGError) as exc:
        print(f"error: {exc}", file=sys.stderr)
        return 2
    m = mesh.numpy()
    if tf is not None:
        m = Mesh(points_from_scene(m.vertices, *tf).astype(np.float32), m.faces,
                 directions_from_scene(m.normals, tf[0]).astype(np.float32), m.colors)
    write_ply_mesh(a.out, m)
    if a.out_points:
        np.save(a.out_points, np.asarray(m.vertices, dtype=np.float64))
    print(f"{len(m.vertices)} vertices, {len(m.faces)} faces -> {a.out}")
    if len(m.faces) == 0:
        print("error: the mesh is empty (nothing observed inside the box?)", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
