"""float64 torch restatement of the per-Gaussian chain of one view (csrc/project.hip: gg_view_fwd, gg_shade_tail_fwd,
gg_view_bwd and the three kernels those replace, gg_sh_bwd_multi): the activations as the reference model's
`get_outputs` states them (PARITY.md, "caller-side ops"), the projection of tests/pose_grad_ref.py with its discrete
part added, the SH colours from the closed-form real basis, the clamp and the rgb | depth | normal tail.  One
differentiable function (`forward`) and autograd of a 13-column gradient record through it (`grads`): an independent,
high-precision statement of what the kernels write, Gaussian by Gaussian.  Nothing here shares code with the kernels or
with oracle/gg_oracle.c; tests/test_view_chain_cases_host.py ties the SH constants to the oracle's to 1e-12."""
import math
from collections import namedtuple

import numpy as np
import torch

import pose_grad_ref as pref
from gaussiangrasper_amd import constants as K

EIG_FLOOR, RADIUS_SIGMA = float(np.float32(K.EIG_FLOOR)), float(np.float32(K.RADIUS_SIGMA))
QUAT_NORM_EPS = 1e-12            # F.normalize's default eps (quat_to_rotmat)

# cam_pos (3,), viewmat (3, 4), full_proj (4, 4): float32 numpy; tile_bounds (tiles_x, tiles_y, 1)
View = namedtuple("View", "cam_pos viewmat full_proj fx fy cx cy h w tile_bounds clip")

_PI = math.pi
SH_C0 = 0.5 * math.sqrt(1.0 / _PI)
SH_C1 = math.sqrt(3.0 / (4.0 * _PI))
SH_C2 = (0.5 * math.sqrt(15.0 / _PI), -0.5 * math.sqrt(15.0 / _PI), 0.25 * math.sqrt(5.0 / _PI),
         -0.5 * math.sqrt(15.0 / _PI), 0.25 * math.sqrt(15.0 / _PI))
SH_C3 = (-0.25 * math.sqrt(35.0 / (2.0 * _PI)), 0.5 * math.sqrt(105.0 / _PI), -0.25 * math.sqrt(21.0 / (2.0 * _PI)),
         0.25 * math.sqrt(7.0 / _PI), -0.25 * math.sqrt(21.0 / (2.0 * _PI)), 0.25 * math.sqrt(105.0 / _PI),
         -0.25 * math.sqrt(35.0 / (2.0 * _PI)))
SH_C4 = (0.75 * math.sqrt(35.0 / _PI), -0.75 * math.sqrt(35.0 / (2.0 * _PI)), 0.75 * math.sqrt(5.0 / _PI),
         -0.75 * math.sqrt(5.0 / (2.0 * _PI)), 3.0 / 16.0 * math.sqrt(1.0 / _PI), -0.75 * math.sqrt(5.0 / (2.0 * _PI)),
         3.0 / 8.0 * math.sqrt(5.0 / _PI), -0.75 * math.sqrt(35.0 / (2.0 * _PI)), 3.0 / 16.0 * math.sqrt(35.0 / _PI))
# ... held as the kernels and the oracle (in both precisions) hold them: rounded to float32
_f32 = lambda c: float(np.float32(c))
SH_C0, SH_C1 = _f32(SH_C0), _f32(SH_C1)
SH_C2, SH_C3, SH_C4 = (tuple(_f32(c) for c in cs) for cs in (SH_C2, SH_C3, SH_C4))


def f64(t):
    return torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t).detach().to("cpu", torch.float64)


def sh_basis(deg, dirs):
    """real spherical harmonics to degree `deg` (<= 4) of the unit vectors dirs (N, 3) -> (N, num_sh_bases(deg))"""
    x, y, z = dirs.unbind(-1)
    Y = [torch.full_like(x, SH_C0)]
    if deg >= 1:
        Y += [-SH_C1 * y, SH_C1 * z, -SH_C1 * x]
    if deg >= 2:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        Y += [SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy)]
    if deg >= 3:
        Y += [SH_C3[0] * y * (3 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4 * zz - xx - yy),
              SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy), SH_C3[4] * x * (4 * zz - xx - yy), SH_C3[5] * z * (xx - yy),
              SH_C3[6] * x * (xx - 3 * yy)]
    if deg >= 4:
        Y += [SH_C4[0] * xy * (xx - yy), SH_C4[1] * yz * (3 * xx - yy), SH_C4[2] * xy * (7 * zz - 1),
              SH_C4[3] * yz * (7 * zz - 3), SH_C4[4] * (zz * (35 * zz - 30) + 3), SH_C4[5] * xz * (7 * zz - 3),
              SH_C4[6] * (xx - yy) * (7 * zz - 1), SH_C4[7] * xz * (xx - 3 * yy),
              SH_C4[8] * (xx * (xx - 3 * yy) - yy * (3 * xx - yy))]
    return torch.stack(Y, -1)


def rotmat(q):
    """quat_to_rotmat: R(F.normalize(q)), wxyz, (N, 3, 3)"""
    w, x, y, z = torch.nn.functional.normalize(q, dim=-1, eps=QUAT_NORM_EPS).unbind(-1)
    return torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), -1).reshape(-1, 3, 3)


def forward(means, log_scales, quats, opacities, colors_all, view, degrees_to_use, viewmat=None, full_proj=None,
            viewdirs=None, axis=None):
    """float64 leaves (N, 3), (N, 3), (N, 4), (N, 1), (N, K, 3) -> dict of everything the forward kernels write, plus
    `margins`: the quantities compared with a threshold, before the comparison (not differentiable).  viewmat /
    full_proj: the view's own when None; (N, 3, 4) / (N, 4, 4) leaves for the camera's gradient.  viewdirs: held at
    these values instead of following the means (the reference model detaches them: a finite difference in the means
    has to hold them still to see what autograd sees); axis: likewise the normal's column, which a finite difference
    in tied log-scales would otherwise switch."""
    n = means.shape[0]
    V = f64(view.viewmat) if viewmat is None else viewmat
    Pm = f64(view.full_proj) if full_proj is None else full_proj
    cam = f64(view.cam_pos)
    # ---- activations (reference get_outputs :701, :703, :742, :727-728, :605-619)
    scales = torch.exp(log_scales)
    quats_n = quats / quats.norm(dim=-1, keepdim=True)
    opac = torch.sigmoid(opacities)
    if viewdirs is None:
        viewdirs = means.detach() - cam
        viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
    if axis is None:
        axis = torch.argmin(scales.detach(), dim=-1)              # the first minimum
        first = torch.stack([(scales.detach()[:, k:k + 1] <= scales.detach()).all(-1) for k in range(3)], -1)
        assert torch.equal(axis, first.to(torch.int64).argmax(-1))
    normals = rotmat(quats)[torch.arange(n), :, axis]
    # ---- projection
    xys, tz, conics = pref.project(means, scales, 1.0, quats_n, V, Pm, view.fx, view.fy, view.cx, view.cy, view.h, view.w)
    with torch.no_grad():
        # cov2d back from the conic (its inverse), then the radius and the tile box
        ca, cb, cc = conics.unbind(-1)
        det = 1.0 / (ca * cc - cb * cb)
        a, c = cc * det, ca * det
        bm = 0.5 * (a + c)
        gap = bm * bm - det
        lam = bm + torch.sqrt(torch.clamp(gap, min=EIG_FLOOR))
        radius_f = RADIUS_SIGMA * torch.sqrt(lam)
        radius = torch.ceil(radius_f)
        tiles_x, tiles_y = int(view.tile_bounds[0]), int(view.tile_bounds[1])
        tcx, tcy, tr = xys[:, 0] / K.BLOCK, xys[:, 1] / K.BLOCK, radius / K.BLOCK
        corners = torch.stack((tcx - tr, tcx + tr + 1.0, tcy - tr, tcy + tr + 1.0), -1)
        bounds = torch.tensor([tiles_x, tiles_x, tiles_y, tiles_y], dtype=torch.float64)
        box = torch.floor(torch.minimum(torch.clamp(corners, min=0.0), bounds)).to(torch.int64)
        area = (box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2])
        vis = (tz > view.clip) & (det != 0) & (area > 0)
        radii = (radius.to(torch.int64) * vis).to(torch.int32)
        num_tiles_hit = (area * vis).to(torch.int32)
        Vn = V if V.dim() == 2 else V[0]
        t = means @ Vn[:, :3].T + Vn[:, 3]
        lim_x, lim_y = pref.FOV_LIM * (0.5 * view.w) / view.fx, pref.FOV_LIM * (0.5 * view.h) / view.fy
        margins = {"tz": tz.clone(), "rx": t[:, 0] / t[:, 2], "ry": t[:, 1] / t[:, 2], "lim_x": lim_x, "lim_y": lim_y,
                   "radius": radius_f, "corners": corners, "bounds": bounds, "eig_gap": gap, "area": area, "vis": vis}
        # the forward kernel stores the conic before the tile cull (as gsplat's does): what the array holds afterwards
        conics_written = conics * ((tz > view.clip) & (det != 0)).to(torch.float64)[:, None]
    m = vis.to(torch.float64)
    xys, depths, conics = xys * m[:, None], tz * m, conics * m[:, None]
    # ---- SH, clamp, tail
    nb = K.num_sh_bases(degrees_to_use)
    assert colors_all.shape[1] >= nb
    Y = sh_basis(degrees_to_use, viewdirs)
    raw = (Y[:, :, None] * colors_all[:, :nb, :]).sum(1) + 0.5
    rgb = torch.clamp(raw, 0.0, 1.0)
    with torch.no_grad():
        open_ = (raw >= 0.0) & (raw <= 1.0)
        mask = (open_.to(torch.int64) * torch.tensor([1, 2, 4])).sum(-1).to(torch.uint8)
        margins["rgb_raw"] = raw.clone()
    tail = torch.cat((rgb, depths[:, None], normals), -1)
    return {"scales": scales, "quats_n": quats_n, "opac": opac, "viewdirs": viewdirs, "normals": normals, "axis": axis,
            "xys": xys, "depths": depths, "radii": radii, "conics": conics, "num_tiles_hit": num_tiles_hit, "tail": tail,
            "mask": mask, "vis": vis, "margins": margins, "conics_written": conics_written}


def case_leaves(case, n=None):
    """the case's float32 leaves as float64 tensors, truncated to the first n Gaussians"""
    n = case.means.shape[0] if n is None else n
    return tuple(f64(a[:n]) for a in (case.means, case.log_scales, case.quats, case.opacities, case.colors_all))


def record_loss(out, record):
    """the scalar whose gradient is the chain's backward of the record's 13 columns
    [v_xy 0..1 | v_conic 2..4 | v_opacity 5 | v_rgb 6..8 | v_depth 9 | v_normal 10..12]"""
    r = f64(record)[:, :13]
    return pref.cotangent_loss(out["xys"], out["depths"], out["conics"], r[:, 0:2], r[:, 9], r[:, 2:5]) + \
        (r[:, 5:6] * out["opac"]).sum() + (r[:, 6:9] * out["tail"][:, 0:3]).sum() + \
        (r[:, 10:13] * out["normals"]).sum()


def grads(case, record, n=None, degrees_to_use=None, colors_all=None, view=None):
    """autograd of the record (rows of >= 13 floats) through `forward` -> dict: means, log_scales, quats, opacities,
    colors_all (the five parameter gradients), v_rgb (the clamp-masked colour cotangent), v_viewmat (3, 4), v_projmat
    (4, 4) and their per-entry absolute sums over the Gaussians (abs_viewmat, abs_projmat), as pose_grad_ref.pose_grads
    returns them."""
    leaves = [t.clone().requires_grad_(True) for t in case_leaves(case, n)]
    if colors_all is not None:
        leaves[4] = f64(colors_all).clone().requires_grad_(True)
    nn = leaves[0].shape[0]
    view = case.view if view is None else view
    V = f64(view.viewmat).expand(nn, 3, 4).clone().requires_grad_(True)
    Pm = f64(view.full_proj).expand(nn, 4, 4).clone().requires_grad_(True)
    deg = case.degree if degrees_to_use is None else degrees_to_use
    out = forward(*leaves, view, deg, V, Pm)
    record_loss(out, f64(record)[:nn]).backward()
    r = f64(record)[:nn]
    open_ = torch.stack([(out["mask"].to(torch.int64) >> c) & 1 for c in range(3)], -1).to(torch.float64)
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return {"means": zero(leaves[0]), "log_scales": zero(leaves[1]), "quats": zero(leaves[2]),
            "opacities": zero(leaves[3]), "colors_all": zero(leaves[4]), "v_rgb": r[:, 6:9] * open_,
            "v_viewmat": V.grad.sum(0), "v_projmat": Pm.grad.sum(0), "abs_viewmat": V.grad.abs().sum(0),
            "abs_projmat": Pm.grad.abs().sum(0), "out": out}


PARAMS = ("means", "log_scales", "quats", "opacities")


def opacity_floor(record, n=None):
    """(N,) the absolute precision of the opacity gradient: the reference model forms sigmoid' from the activated
    opacity s as s (1 - s), and a float32 s carries half an ulp of 1 (2^-24), so the product does too, times |v_opacity|.
    At logit +30 the float64 derivative is 9.4e-14 and the float32 one exactly 0 (s rounds to 1): both are right to
    that precision, and the row's scale in `row_errors` is not taken below it."""
    r = f64(record)
    return 2.0 ** -24 * r[:r.shape[0] if n is None else n, 5].abs()


def row_errors(got, ref, floor=None):
    """the error measure of the chain's tests: per Gaussian and parameter row |got - ref| / max|ref row| -> (N,), with
    rows whose reference is exactly zero required to be exactly zero (reported as inf when they are not).  floor (N,):
    a lower bound of the row's scale where the reference is not zero (opacity_floor)"""
    got, ref = f64(got).reshape(ref.shape[0], -1), f64(ref).reshape(ref.shape[0], -1)
    scale = ref.abs().max(-1).values
    diff = (got - ref).abs().max(-1).values
    if floor is not None:
        scale = torch.where(scale > 0, torch.maximum(scale, floor), scale)
    err = torch.where(scale > 0, diff / torch.where(scale > 0, scale, torch.ones_like(scale)),
                      torch.where(diff == 0, torch.zeros_like(diff), torch.full_like(diff, float("inf"))))
    return err
