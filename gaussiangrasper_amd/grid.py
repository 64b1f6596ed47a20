"""The uniform grids the grid-sorted calls take (csrc/grid_sort.h): gg_knn sorts into knn_grid, and gg_cluster_dbscan,
gg_cloud_frames and gg_icp_step into cluster_grid.  A grid sets the speed of a call, never its result.  Host numpy on a
sample of the points read back; `prepare.knn_grid` and `cluster.cluster_grid` are these functions."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from ._call import positive


def knn_grid(points: Tensor, target_cells_per_point: float = 2.0, sample: int = 65536):
    """The grid gg_knn sorts into: fitted to the bulk of the cloud (per axis the 0.1 %-99.9 % quantiles of a strided
    sample of at most `sample` rows, within the quartiles -/+ 3 IQR) so that far outliers, up to a quarter of the
    points on one side, do not stretch it; about `target_cells_per_point` cells per point.  Points outside it go to its border cells: the grid only sets the speed, never the result.
    Returns (grid float64 [lo x, y, z, cell], dims int32 [3])."""
    n = points.shape[0]
    step = max(1, n // sample)
    s = points[::step].detach().to("cpu", torch.float64).numpy()
    # per axis: the 0.1 %-99.9 % quantiles, narrowed to Tukey's far fences (quartiles -/+ 3 IQR) so that a few per
    # cent of far points cannot stretch the grid over the dense part
    q = np.quantile(s, [0.001, 0.25, 0.75, 0.999], axis=0)
    iqr = q[2] - q[1]
    lo = np.maximum(q[0], q[1] - 3.0 * iqr)
    hi = np.minimum(q[3], q[2] + 3.0 * iqr)
    ext = hi - lo
    emax = float(ext.max())
    cap = 1 << 26
    target = int(min(max(1.0, target_cells_per_point * n), cap // 2))
    if not emax > 0.0:
        return np.array([lo[0], lo[1], lo[2], 1.0]), np.ones(3, dtype=np.int32)

    def cells(cell):
        return np.maximum(1, np.ceil(ext / cell)).astype(np.int64)

    a, b = emax / target, emax    # cells(a) >= target, cells(b) == 1 per axis
    for _ in range(60):
        mid = (a * b) ** 0.5
        if np.prod(cells(mid)) > target:
            a = mid
        else:
            b = mid
    dims = cells(b)
    return np.array([lo[0], lo[1], lo[2], b], dtype=np.float64), dims.astype(np.int32)


def active(points: Tensor, mask: Optional[Tensor]) -> Tensor:
    a = torch.isfinite(points).all(dim=1)
    return a if mask is None else a & (mask != 0)


def cluster_grid(points: Tensor, eps: float, mask: Optional[Tensor] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The grid gg_cluster_dbscan sorts into: knn_grid fitted to the active points, with the cell edge raised
    to at least eps (fewer cells over the same box).  Points outside it go to its border cells: the grid sets the
    speed, never the result.  Returns (grid float64 [lo x, y, z, cell], dims int32 [3])."""
    eps = positive("eps", eps)
    pts = points[active(points, mask)]
    if pts.shape[0] == 0:
        return np.array([0.0, 0.0, 0.0, eps]), np.ones(3, dtype=np.int32)
    grid, dims = knn_grid(pts)
    if grid[3] < eps:
        ext = dims.astype(np.float64) * grid[3]
        dims = np.maximum(1, np.ceil(ext / eps)).astype(np.int32)
        grid = np.array([grid[0], grid[1], grid[2], eps], dtype=np.float64)
    return grid, dims
