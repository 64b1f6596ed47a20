"""Device-call plumbing shared by every module that calls libgg_raster.so: which device, tensors and host arrays
as the pointers the C ABI takes, the stream, workspaces, grids, and the argument checks several callers make alike.
Imports nothing from the package."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

ArrayLike = Union[np.ndarray, Tensor, Sequence]


def require_hip(*tensors: Tensor) -> torch.device:
    dev = None
    for t in tensors:
        if not isinstance(t, Tensor):
            raise TypeError(f"expected a torch.Tensor, got {type(t)}")
        if t.device.type != "cuda":
            raise RuntimeError(
                "gaussiangrasper_amd operators run only on a HIP device (PyTorch-ROCm 'cuda'); "
                f"got a tensor on '{t.device}'. There is no CPU fallback.")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"tensors on different devices: {dev} vs {t.device}")
    return dev


def default_device(who: str) -> torch.device:
    """The current HIP device, for module `who`'s inputs that are not on one yet."""
    if not torch.cuda.is_available():
        raise RuntimeError(f"gaussiangrasper_amd.{who} runs on a HIP device (PyTorch-ROCm 'cuda'); none is available. "
                           "There is no CPU fallback.")
    return torch.device("cuda", torch.cuda.current_device())


def to_device(x: ArrayLike, dtype: torch.dtype, dev: torch.device) -> Tensor:
    """A tensor, array or sequence as a detached contiguous `dtype` tensor on `dev`."""
    t = x.detach() if isinstance(x, Tensor) else torch.as_tensor(np.asarray(x))
    return t.to(device=dev, dtype=dtype).contiguous()


def host_array(x: ArrayLike, dtype=None) -> np.ndarray:
    """A tensor (detached, brought to the host), array or sequence as a numpy array of `dtype` (None: as it is)."""
    return np.asarray(x.detach().cpu().numpy() if isinstance(x, Tensor) else x, dtype)


def f32(t: Tensor) -> Tensor:
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


def i32(t: Tensor) -> Tensor:
    return t.contiguous() if t.dtype == torch.int32 else t.int().contiguous()


def ptr(t: Optional[Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


def host_ptr(a):
    """A contiguous host numpy array or a ctypes array as c_void_p (None: NULL); the caller keeps `a` alive."""
    if a is None:
        return None
    return a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else C.cast(a, C.c_void_p)


def stream(dev: torch.device):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def workspace(nbytes: int, dev: torch.device) -> Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def sized_workspace(nbytes: int, what: str, dev: torch.device) -> Tensor:
    """The workspace a gg_*_workspace query sized.  0 bytes is the query's "out of range": ValueError(what)."""
    if nbytes == 0:
        raise ValueError(what)
    return workspace(nbytes, dev)


def grid_args(grid):
    """(grid, dims) as grid.knn_grid and grid.cluster_grid return them -> (c_double[4], c_int32[3]) for the C ABI."""
    g, dims = grid
    return ((C.c_double * 4)(*np.asarray(g, dtype=np.float64).tolist()),
            (C.c_int32 * 3)(*np.asarray(dims, dtype=np.int32).tolist()))


def f32_rows(t: Tensor, name: str, width: Optional[int]) -> Tensor:
    """`t` contiguous, after checking that it is float32 (N, width), or (N,) with width None."""
    shape_ok = t.ndim == 2 and t.shape[1] == width if width else t.ndim == 1
    if t.dtype != torch.float32 or not shape_ok:
        want = f"(N, {width})" if width else "(N,)"
        raise ValueError(f"{name} must be a float32 {want} tensor, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def nonneg(name: str, v: float) -> float:
    v = float(v)
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"{name} must be finite and >= 0, got {v}")
    return v


def positive(name: str, v: float) -> float:
    v = float(v)
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"{name} must be finite and > 0, got {v}")
    return v


def check_finite_options(ap, a, positive=(), nonneg=()) -> None:
    """ap.error unless the parsed options named in `positive` are finite and > 0, those in `nonneg` finite and >= 0."""
    for n in positive:
        if not (math.isfinite(getattr(a, n)) and getattr(a, n) > 0.0):
            ap.error(f"--{n} must be finite and > 0, got {getattr(a, n)}")
    for n in nonneg:
        if not (math.isfinite(getattr(a, n)) and getattr(a, n) >= 0.0):
            ap.error(f"--{n} must be finite and >= 0, got {getattr(a, n)}")
