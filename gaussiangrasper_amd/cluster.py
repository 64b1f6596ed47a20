"""Object instances: DBSCAN clustering of the Gaussians a query selects, so that "the mug" is one compact object and
not every mug in the room plus speckle.  Two HIP calls (`gg_cluster_dbscan` and `gg_cluster_stats`,
csrc/cluster.hip); the contract is in include/gg_raster.h and PARITY.md "Object instances".  Labels are a pure
function of the inputs and equal sklearn.cluster.DBSCAN's wherever no pair sits within rounding of eps.

    cluster_grid       the grid gg_cluster_dbscan sorts into (grid.py): knn_grid with cells of at least eps
    dbscan             labels, core flags, neighbour counts and the number of clusters of a point set (Clusters)
    cluster_stats      per cluster: count, weight, weighted centroid, bounding box (ClusterStats)
    rank_instances     clusters above min_count / min_weight by descending weight (Instances); any device
    derive_eps         eps_scale times the median 3rd-nearest-neighbour distance of the selected means
    object_instances   all of the above on a model or scene and an object mask
    instance_mask      (N,) bool mask of one instance, by rank or by the centroid nearest to a point
    python -m gaussiangrasper_amd.cluster --ckpt IN (--positives ... | --object-points ...) --out labels.npy
"""
from __future__ import annotations

import argparse
import json
import sys
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._call import (f32_rows, grid_args, host_ptr, nonneg, positive, ptr as _ptr, require_hip as _require_hip,
                    sized_workspace, stream as _stream)
from .grid import active as _active, cluster_grid

# This project's choices (PARITY.md "Object instances"); nobody has measured good values on a real checkpoint
EPS_SCALE = 3.0              # eps = EPS_SCALE x the median 3rd-nearest-neighbour distance of the selection
EPS_K = 3
MIN_POINTS = 8               # neighbours within eps, the point itself included, that make a core point
MIN_COUNT = 32               # an instance has at least this many Gaussians ...
MIN_WEIGHT = 0.0             # ... and at least this much summed opacity
MAX_POINTS = 1 << 30         # GG_CLUSTER_MAX_POINTS


@dataclass
class Clusters:
    """Outputs of one gg_cluster_dbscan call; N = number of points."""
    labels: Tensor             # (N,) int32: cluster number, -1 for noise and inactive points
    core: Tensor               # (N,) bool
    neighbor_count: Tensor     # (N,) int32: points within eps, the point itself included; 0 for inactive points
    num_clusters: int


@dataclass
class ClusterStats:
    """Outputs of one gg_cluster_stats call; K = number of clusters."""
    count: Tensor              # (K,) int64
    weight: Tensor             # (K,) float64: sum of the members' weights
    centroid: Tensor           # (K, 3) float64: weighted mean of the members
    bbox: Tensor               # (K, 6) float32: min x, y, z, max x, y, z

    def take(self, idx: Tensor) -> "ClusterStats":
        return ClusterStats(self.count[idx], self.weight[idx], self.centroid[idx], self.bbox[idx])


@dataclass
class Instances:
    """The clusters kept as object instances, instance 0 the heaviest; K' of them."""
    ids: Tensor                # (N,) int32: instance number of every point, -1 for none
    cluster: Tensor            # (K',) int64: the cluster number each instance had
    stats: ClusterStats        # of the kept clusters, in instance order

    def __len__(self) -> int:
        return int(self.cluster.shape[0])

    def masks(self) -> Tensor:
        """(K', N) bool: one mask per instance."""
        k = torch.arange(len(self), device=self.ids.device, dtype=self.ids.dtype)
        return self.ids[None, :] == k[:, None]


# ------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------
def dbscan(points: Tensor, eps: float, min_points: int = MIN_POINTS, mask: Optional[Tensor] = None,
           grid: Optional[Tuple[np.ndarray, np.ndarray]] = None) -> Clusters:
    """DBSCAN of `points` (N, 3) float32 on the HIP device (no CPU path) with radius eps and sklearn's min_samples
    convention for min_points; `mask` (N,) bool or uint8 restricts it to the points it selects, and points with a
    non-finite coordinate never take part (include/gg_raster.h gg_cluster_dbscan).  Clusters are numbered in
    ascending order of their smallest core index; a border point takes the smallest number among its core
    neighbours; everything else is -1.  `grid`: (grid, dims) as cluster_grid returns (None: fitted here, which reads
    a sample of the points back).  The kernels run on the current stream; num_clusters is read back once."""
    eps = positive("eps", eps)
    k = int(min_points)
    if k != min_points or k < 1:
        raise ValueError(f"min_points must be an integer >= 1, got {min_points}")
    dev = _require_hip(points) if mask is None else _require_hip(points, mask)
    points = f32_rows(points, "points", 3)
    n = points.shape[0]
    if n > MAX_POINTS:
        raise ValueError(f"{n} points: at most 2^30")
    act = None
    if mask is not None:
        if mask.ndim != 1 or mask.shape[0] != n or mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"mask must be a bool or uint8 ({n},) tensor, got {mask.dtype} {tuple(mask.shape)}")
        act = mask.to(torch.uint8).contiguous()
    res = Clusters(labels=torch.empty(n, dtype=torch.int32, device=dev),
                   core=torch.empty(n, dtype=torch.uint8, device=dev),
                   neighbor_count=torch.empty(n, dtype=torch.int32, device=dev), num_clusters=0)
    if n > 0:
        grid_c, dims_c = grid_args(cluster_grid(points, eps, mask) if grid is None else grid)
        lib = _lib.load()
        ws = sized_workspace(lib.gg_cluster_workspace(n, dims_c), f"{n} points on a grid of {list(dims_c)} cells is "
                             f"beyond gg_cluster_dbscan's limits", dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(lib.gg_cluster_dbscan(n, _ptr(points), _ptr(act), eps, k, host_ptr(grid_c), host_ptr(dims_c),
                                         _ptr(res.labels), _ptr(res.core), _ptr(res.neighbor_count), _ptr(count),
                                         _ptr(ws), ws.numel(), _stream(dev)), "gg_cluster_dbscan")
        res.num_clusters = int(count.item())
    res.core = res.core.bool()
    return res


def cluster_stats(points: Tensor, weights: Tensor, clusters: Union[Clusters, Tuple[Tensor, int]]) -> ClusterStats:
    """Per cluster: member count, summed weight, weighted centroid and bounding box of `points` (N, 3) under
    `weights` (N,), float32 on the HIP device (include/gg_raster.h gg_cluster_stats).  `clusters`: a Clusters, or
    (labels (N,) int32, num_clusters).  Counts and boxes are exact; the fp64 sums are atomic, so their last bits may
    differ from call to call."""
    labels, k = (clusters.labels, clusters.num_clusters) if isinstance(clusters, Clusters) else clusters
    dev = _require_hip(points, weights, labels)
    points = f32_rows(points, "points", 3)
    weights = f32_rows(weights, "weights", None)
    n, k = points.shape[0], int(k)
    if labels.dtype != torch.int32 or labels.ndim != 1 or labels.shape[0] != n or weights.shape[0] != n:
        raise ValueError(f"points has {n} rows, weights {tuple(weights.shape)}, labels {labels.dtype} "
                         f"{tuple(labels.shape)} (int32 (N,) wanted)")
    if not 0 <= k <= n:
        raise ValueError(f"num_clusters must be in 0..{n}, got {k}")
    res = ClusterStats(count=torch.empty(k, dtype=torch.int64, device=dev),
                       weight=torch.empty(k, dtype=torch.float64, device=dev),
                       centroid=torch.empty(k, 3, dtype=torch.float64, device=dev),
                       bbox=torch.empty(k, 6, dtype=torch.float32, device=dev))
    if k > 0:
        _lib.check(_lib.load().gg_cluster_stats(n, _ptr(points), _ptr(weights), _ptr(labels.contiguous()), k,
                                                _ptr(res.count), _ptr(res.weight), _ptr(res.centroid),
                                                _ptr(res.bbox), _stream(dev)), "gg_cluster_stats")
    return res


# ------------------------------------------------------------------------------------------------
# instances: which clusters are objects, and in which order (torch only; any device)
# ------------------------------------------------------------------------------------------------
def rank_instances(labels: Tensor, stats: ClusterStats, min_count: int = MIN_COUNT,
                   min_weight: float = MIN_WEIGHT) -> Instances:
    """The clusters with count >= min_count and weight >= min_weight as instances, ordered by descending weight,
    equal weights by ascending cluster number: instance 0 is "the object".  Points of dropped clusters and of no
    cluster get id -1.  Works on the tensors' own device."""
    mw = float(min_weight)
    if mw != mw:
        raise ValueError("min_weight must not be NaN")
    mc = int(min_count)
    if mc != min_count or mc < 0:
        raise ValueError(f"min_count must be an integer >= 0, got {min_count}")
    k = stats.count.shape[0]
    keep = torch.nonzero((stats.count >= mc) & (stats.weight >= mw)).reshape(-1)
    order = keep[torch.sort(stats.weight[keep], descending=True, stable=True).indices]
    rank = torch.full((k + 1,), -1, dtype=torch.int32, device=labels.device)        # slot k: label -1
    rank[order] = torch.arange(order.shape[0], dtype=torch.int32, device=labels.device)
    lab = labels.long()
    ids = rank[torch.where((lab >= 0) & (lab < k), lab, torch.full_like(lab, k))]
    return Instances(ids=ids, cluster=order, stats=stats.take(order))


def derive_eps(points: Tensor, mask: Optional[Tensor] = None, eps_scale: float = EPS_SCALE) -> float:
    """eps_scale times the median distance to the EPS_K-th (3rd) nearest neighbour among the selected finite points
    (prepare.knn_distances): a radius that follows the selection's own density.  One read-back."""
    from .prepare import knn_distances
    s = positive("eps_scale", eps_scale)
    pts = points[_active(points, mask)]
    if pts.shape[0] <= EPS_K:
        raise ValueError(f"{pts.shape[0]} selected points: deriving eps needs more than {EPS_K}")
    d = knn_distances(pts, EPS_K)[0][:, EPS_K - 1]
    eps = s * float(d.double().median().item())
    if not eps > 0.0:
        raise ValueError("the selection's median neighbour distance is 0: give eps")
    return eps


def object_instances(model_or_scene, mask: Optional[Tensor] = None, eps: Optional[float] = None,
                     min_points: int = MIN_POINTS, min_weight: float = MIN_WEIGHT, min_count: int = MIN_COUNT,
                     eps_scale: float = EPS_SCALE) -> Instances:
    """The object instances among the Gaussians `mask` selects (None: all): dbscan of the means, cluster_stats
    under sigmoid(opacity) (the weights grasp.model_points uses), rank_instances.  eps None: derive_eps(means, mask,
    eps_scale); otherwise a length in the means' units."""
    means = model_or_scene.means.detach()
    opac = model_or_scene.opacities.detach()
    dev = _require_hip(means, opac)
    means = means.float().contiguous()
    if mask is not None:
        mask = mask.reshape(-1).to(dev)
        if mask.shape[0] != means.shape[0]:
            raise ValueError(f"mask has {mask.shape[0]} entries for {means.shape[0]} Gaussians")
        mask = mask != 0
    if eps is None:
        eps = derive_eps(means, mask, eps_scale)
    cl = dbscan(means, eps, min_points, mask)
    weights = torch.sigmoid(opac.float()).reshape(-1).contiguous()
    return rank_instances(cl.labels, cluster_stats(means, weights, cl), min_count, min_weight)


def instance_mask(instances: Instances, which=0) -> Tensor:
    """(N,) bool mask of one instance.  `which`: an int rank (0 the heaviest), or a 3-vector: the instance whose
    centroid is nearest to that point (the smallest rank on a tie)."""
    k = len(instances)
    if k == 0:
        raise ValueError("there are no instances")
    if isinstance(which, (int, np.integer)) and not isinstance(which, bool):
        if not 0 <= which < k:
            raise ValueError(f"instance {which} of {k}")
        r = int(which)
    else:
        p = torch.as_tensor(np.asarray(which, dtype=np.float64).reshape(-1))
        if p.shape[0] != 3 or not bool(torch.isfinite(p).all()):
            raise ValueError(f"which must be an int rank or 3 finite numbers, got {which}")
        d = ((instances.stats.centroid.double().cpu() - p) ** 2).sum(dim=1)
        r = int(torch.argmin(d).item())
    return instances.ids == r


def report(instances: Instances) -> dict:
    s = instances.stats
    return {"num_instances": len(instances), "cluster": instances.cluster.cpu().tolist(),
            "count": s.count.cpu().tolist(), "weight": s.weight.cpu().tolist(),
            "centroid": s.centroid.cpu().tolist(), "bbox": s.bbox.cpu().tolist()}


# ------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------
def main(argv: Optional[Sequence[str]] = None) -> int:
    from ._cli import (add_object_options, add_support_options, check_object_options, check_support_options,
                       load_scene, object_mask)
    from .frames import check_rotation, load_transform_json
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.cluster",
                                 description="Split the Gaussians a query selects into object instances (DBSCAN) and "
                                             "write every Gaussian's instance number.")
    ap.add_argument("--ckpt", required=True, help="step-*.ckpt of a splatting model")
    ap.add_argument("--transform-json", default=None, help="JSON with transform_matrix and scale (world -> scene)")
    add_object_options(ap, "the query selects the Gaussians", "selects the Gaussians", instances=False)
    add_support_options(ap, grasp=False)
    ap.add_argument("--eps", type=float, default=None, help="neighbour radius, world units (default: --eps-scale "
                                                            "times the selection's median 3rd-neighbour distance)")
    ap.add_argument("--eps-scale", type=float, default=EPS_SCALE, help="see --eps")
    ap.add_argument("--min-points", type=int, default=MIN_POINTS, help="neighbours within eps that make a core point")
    ap.add_argument("--min-count", type=int, default=MIN_COUNT, help="Gaussians an instance has at least")
    ap.add_argument("--min-weight", type=float, default=MIN_WEIGHT, help="summed opacity an instance has at least")
    ap.add_argument("--out", required=True, help="output .npy: (N,) int32 instance number per Gaussian, -1 for none; "
                                                 "instance 0 is the heaviest")
    ap.add_argument("--report", default=None, help="output .json: per instance count, weight, centroid and bbox "
                                                   "(scene frame)")
    a = ap.parse_args(argv)
    check_object_options(ap, a, "required")
    check_support_options(ap, a, grasp=False)
    if a.eps is not None and not (np.isfinite(a.eps) and a.eps > 0.0):
        ap.error(f"--eps must be finite and > 0, got {a.eps}")
    if not (np.isfinite(a.eps_scale) and a.eps_scale > 0.0):
        ap.error(f"--eps-scale must be finite and > 0, got {a.eps_scale}")
    if a.min_points < 1 or a.min_count < 0 or a.min_weight != a.min_weight:
        ap.error("--min-points must be >= 1, --min-count >= 0 and --min-weight a number")
    try:
        matrix, scale = None, 1.0
        if a.transform_json:
            matrix, scale = load_transform_json(a.transform_json)
            if matrix.shape not in ((3, 4), (4, 4)):
                raise ValueError(f"transform_matrix must be 3x4 or 4x4, got {matrix.shape}")
            check_rotation(matrix[:3, :3], "matrix rotation")
        scene, mlp_state = load_scene(a.ckpt)
        mask = object_mask(a, scene, mlp_state, matrix, scale)
        inst = object_instances(scene, mask, None if a.eps is None else a.eps * nonneg("scale", scale),
                                a.min_points, a.min_weight, a.min_count, a.eps_scale)
    except (KeyError, ValueError, OSError) as exc:
        raise SystemExit(f"error: {exc}") from exc
    np.save(a.out, inst.ids.cpu().numpy())
    if a.report:
        with open(a.report, "w") as f:
            json.dump(report(inst), f, indent=1)
    print(f"{len(inst)} instances among {int(mask.sum())} selected Gaussians; wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
