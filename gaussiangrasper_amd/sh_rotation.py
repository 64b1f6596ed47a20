"""Rotation of spherical-harmonic colour coefficients, for the scene update (gaussiangrasper_amd.edit): a Gaussian moved
by a rotation R keeps its appearance only if its SH lobes, which are expressed in world axes (`viewdirs = means -
cam_pos`), turn with it.  Host side in numpy fp64; the device side is one HIP kernel (`gg_sh_rotate`,
csrc/sh_rotate.hip).

The band matrices D_l are FITTED to the basis the renderer evaluates — `sh_basis` of csrc/project.hip, with the
header's constants as the header has them (`f` literals: the fp32 rounding of the printed number) — instead of taken
from the Ivanic-Ruedenberg recursion for ideal real harmonics.  Band l of that basis spans a rotation-invariant space
of dimension 2l+1 whatever its constants are, so a least-squares fit on enough directions recovers the exact change of
coefficients: colours evaluated by this library are invariant to ~4e-15 in fp64.  The price: the fp32-rounded
constants make the basis orthonormal only to ~1e-7, so D D^T - I is ~8e-8 instead of 1e-16.  That is the right
matrix for this basis, not a defect (PARITY.md "Scene update")."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._call import ArrayLike, host_ptr, ptr as _ptr, require_hip as _require_hip, stream as _stream

MAX_DEGREE = 4
NUM_BASES = (1, 4, 9, 16, 25)
ORTHO_TOL = 1e-4
FIT_DIRECTIONS = 96

_f = lambda s: float(np.float32(s))  # noqa: E731 - an `f` literal of include/gg_constants.h, widened exactly

# GG_SH_C* of include/gg_constants.h, restated (tests/test_sh_rotate_host.py compares the two)
SH_CONSTANTS = {
    "GG_SH_C0": _f("0.28209479177387814"),
    "GG_SH_C1": _f("0.4886025119029199"),
    "GG_SH_C2_0": _f("1.0925484305920792"),
    "GG_SH_C2_1": _f("-1.0925484305920792"),
    "GG_SH_C2_2": _f("0.31539156525252005"),
    "GG_SH_C2_3": _f("-1.0925484305920792"),
    "GG_SH_C2_4": _f("0.5462742152960396"),
    "GG_SH_C3_0": _f("-0.5900435899266435"),
    "GG_SH_C3_1": _f("2.890611442640554"),
    "GG_SH_C3_2": _f("-0.4570457994644658"),
    "GG_SH_C3_3": _f("0.3731763325901154"),
    "GG_SH_C3_4": _f("-0.4570457994644658"),
    "GG_SH_C3_5": _f("1.445305721320277"),
    "GG_SH_C3_6": _f("-0.5900435899266435"),
    "GG_SH_C4_0": _f("2.5033429417967046"),
    "GG_SH_C4_1": _f("-1.7701307697799304"),
    "GG_SH_C4_2": _f("0.9461746957575601"),
    "GG_SH_C4_3": _f("-0.6690465435572892"),
    "GG_SH_C4_4": _f("0.10578554691520431"),
    "GG_SH_C4_5": _f("-0.6690465435572892"),
    "GG_SH_C4_6": _f("0.47308734787878004"),
    "GG_SH_C4_7": _f("-1.7701307697799304"),
    "GG_SH_C4_8": _f("0.6258357354491761"),
}


def sh_basis(dirs: ArrayLike, degree: int) -> np.ndarray:
    """(M, (degree + 1)^2) fp64: the library's SH basis (csrc/project.hip `sh_basis`, the same expressions in the same
    order) on the normalised rows of `dirs` (M, 3)."""
    if not 0 <= int(degree) <= MAX_DEGREE:
        raise ValueError(f"degree must be 0..{MAX_DEGREE}, got {degree}")
    degree = int(degree)
    d = np.asarray(dirs, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] != 3:
        raise ValueError(f"dirs must be (M, 3), got {d.shape}")
    C = SH_CONSTANTS
    Y = np.empty((d.shape[0], (degree + 1) ** 2), np.float64)
    Y[:, 0] = C["GG_SH_C0"]
    if degree < 1:
        return Y
    norm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    x, y, z = d[:, 0] / norm, d[:, 1] / norm, d[:, 2] / norm
    Y[:, 1] = C["GG_SH_C1"] * (-y)
    Y[:, 2] = C["GG_SH_C1"] * z
    Y[:, 3] = C["GG_SH_C1"] * (-x)
    if degree < 2:
        return Y
    xx, xy, xz, yy, yz, zz = x * x, x * y, x * z, y * y, y * z, z * z
    Y[:, 4] = C["GG_SH_C2_0"] * xy
    Y[:, 5] = C["GG_SH_C2_1"] * yz
    Y[:, 6] = C["GG_SH_C2_2"] * ((2.0 * zz - xx) - yy)
    Y[:, 7] = C["GG_SH_C2_3"] * xz
    Y[:, 8] = C["GG_SH_C2_4"] * (xx - yy)
    if degree < 3:
        return Y
    Y[:, 9] = (C["GG_SH_C3_0"] * y) * (3.0 * xx - yy)
    Y[:, 10] = (C["GG_SH_C3_1"] * xy) * z
    Y[:, 11] = (C["GG_SH_C3_2"] * y) * ((4.0 * zz - xx) - yy)
    Y[:, 12] = (C["GG_SH_C3_3"] * z) * ((2.0 * zz - 3.0 * xx) - 3.0 * yy)
    Y[:, 13] = (C["GG_SH_C3_4"] * x) * ((4.0 * zz - xx) - yy)
    Y[:, 14] = (C["GG_SH_C3_5"] * z) * (xx - yy)
    Y[:, 15] = (C["GG_SH_C3_6"] * x) * (xx - 3.0 * yy)
    if degree < 4:
        return Y
    Y[:, 16] = (C["GG_SH_C4_0"] * xy) * (xx - yy)
    Y[:, 17] = (C["GG_SH_C4_1"] * yz) * (3.0 * xx - yy)
    Y[:, 18] = (C["GG_SH_C4_2"] * xy) * (7.0 * zz - 1.0)
    Y[:, 19] = (C["GG_SH_C4_3"] * yz) * (7.0 * zz - 3.0)
    Y[:, 20] = C["GG_SH_C4_4"] * (zz * (35.0 * zz - 30.0) + 3.0)
    Y[:, 21] = (C["GG_SH_C4_5"] * xz) * (7.0 * zz - 3.0)
    Y[:, 22] = (C["GG_SH_C4_6"] * (xx - yy)) * (7.0 * zz - 1.0)
    Y[:, 23] = (C["GG_SH_C4_7"] * xz) * (xx - 3.0 * yy)
    Y[:, 24] = C["GG_SH_C4_8"] * (xx * (xx - 3.0 * yy) - yy * (3.0 * xx - yy))
    return Y


def fit_directions() -> np.ndarray:
    """The (96, 3) Fibonacci-sphere directions the band matrices are fitted on: four times the 25 unknown rows of the
    widest band, spread evenly enough that the fit's condition number stays below 1.02."""
    i = np.arange(FIT_DIRECTIONS, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / FIT_DIRECTIONS
    r = np.sqrt(1.0 - z * z)
    phi = math.pi * (1.0 + math.sqrt(5.0)) * i
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def nearest_rotation(R: ArrayLike) -> np.ndarray:
    """`R` (3, 3) projected to the nearest rotation (SVD, fp64).  ValueError when it is not one to begin with:
    max |R^T R - I| > 1e-4 (a scale or shear inside R is out of scope) or det R <= 0 (a reflection)."""
    R = np.asarray(R, dtype=np.float64)
    if R.shape != (3, 3):
        raise ValueError(f"R must be a (3, 3) rotation matrix, got {R.shape}")
    if not np.isfinite(R).all():
        raise ValueError("R is not finite")
    err = np.abs(R.T @ R - np.eye(3)).max()
    if err > ORTHO_TOL:
        raise ValueError(f"R is not orthonormal (max |R^T R - I| = {err:.3g} > {ORTHO_TOL:g})")
    if np.linalg.det(R) <= 0.0:
        raise ValueError("R is a reflection (det R <= 0), not a rotation")
    U, _, Vt = np.linalg.svd(R)
    return U @ Vt


def rotation_bands(R: ArrayLike, degree: int = MAX_DEGREE) -> List[np.ndarray]:
    """[D_1, ..., D_degree], D_l (2l+1, 2l+1) fp64, such that for every direction d and coefficient vector c
    sum_k (D c)_k Y_k(R d) = sum_k c_k Y_k(d): the coefficients of a lobe turned by R.  D is block-diagonal over the
    bands and band 0 is 1.  Each D_l is the least-squares solution of Y_l(X) D_l = Y_l(X R) on fit_directions()."""
    if not 0 <= int(degree) <= MAX_DEGREE:
        raise ValueError(f"degree must be 0..{MAX_DEGREE}, got {degree}")
    degree = int(degree)
    R = nearest_rotation(R)
    X = fit_directions()
    Y0, Y1 = sh_basis(X, degree), sh_basis(X @ R, degree)
    out = []
    for l in range(1, degree + 1):
        lo, hi = l * l, (l + 1) * (l + 1)
        out.append(np.linalg.lstsq(Y0[:, lo:hi], Y1[:, lo:hi], rcond=None)[0])
    return out


def pack_bands(bands: Sequence[np.ndarray], num_bases: int) -> np.ndarray:
    """The fp32 array gg_sh_rotate takes: D_1, D_2, ... of the bands `num_bases` has, each row-major, concatenated
    (9 + 25 + 49 + 81 = 164 floats for 25 bases; empty for 1)."""
    if num_bases not in NUM_BASES:
        raise ValueError(f"num_bases must be one of {NUM_BASES}, got {num_bases}")
    deg = NUM_BASES.index(num_bases)
    if len(bands) < deg:
        raise ValueError(f"{num_bases} bases need D_1..D_{deg}, got {len(bands)} bands")
    parts = []
    for l in range(1, deg + 1):
        D = np.asarray(bands[l - 1], dtype=np.float64)
        if D.shape != (2 * l + 1, 2 * l + 1):
            raise ValueError(f"D_{l} must be ({2 * l + 1}, {2 * l + 1}), got {D.shape}")
        parts.append(D.reshape(-1))
    return np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0), dtype=np.float32)


def check_coefficients(coeffs: Tensor, mask: Optional[Tensor] = None) -> int:
    """The layout gg_sh_rotate edits in place; returns K."""
    if (coeffs.dtype != torch.float32 or coeffs.ndim != 3 or coeffs.shape[2] != 3 or not coeffs.is_contiguous()
            or coeffs.shape[1] not in NUM_BASES):
        raise ValueError(f"SH coefficients must be a contiguous float32 (N, K, 3) tensor with K in {NUM_BASES}, got "
                         f"{coeffs.dtype} {tuple(coeffs.shape)}{'' if coeffs.is_contiguous() else ' (not contiguous)'}")
    if mask is not None and (mask.dtype != torch.uint8 or mask.ndim != 1 or mask.shape[0] != coeffs.shape[0]
                             or not mask.is_contiguous()):
        raise ValueError(f"mask must be a contiguous uint8 ({coeffs.shape[0]},) tensor, got {mask.dtype} "
                         f"{tuple(mask.shape)}")
    return coeffs.shape[1]


def launch(coeffs: Tensor, mask: Optional[Tensor], packed: np.ndarray, dev: torch.device) -> None:
    """One gg_sh_rotate on the current stream of `dev`; arguments already checked."""
    _lib.check(_lib.load().gg_sh_rotate(coeffs.shape[0], coeffs.shape[1], _ptr(coeffs), _ptr(mask), host_ptr(packed),
                                        _stream(dev)), "gg_sh_rotate")


def rotate_coefficients(coeffs: Tensor, R: ArrayLike, mask: Optional[Tensor] = None) -> Tensor:
    """Turn the SH coefficients of the selected rows by the rotation R, in place, and return `coeffs`.

    coeffs: contiguous float32 (N, K, 3) on the HIP device (no CPU path), K in {1, 4, 9, 16, 25}.  mask: uint8 (N,) on
    the same device, non-zero = selected, or None for every row.  The bands are built from the fp64 value of R; the
    device arithmetic is fp32 in a fixed order (include/gg_raster.h).  One launch; nothing waits on the host."""
    dev = _require_hip(coeffs) if mask is None else _require_hip(coeffs, mask)
    k = check_coefficients(coeffs, mask)
    R = R.detach().cpu().numpy() if isinstance(R, Tensor) else np.asarray(R)
    packed = pack_bands(rotation_bands(R.astype(np.float64), NUM_BASES.index(k)), k)
    launch(coeffs, mask, packed, dev)
    return coeffs
