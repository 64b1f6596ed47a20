"""What the command lines of grasp, grasp_propose and mesh share: the options that say which Gaussians are the
object (the convex hull of --object-points, or the LERF relevancy of --positives against --negatives above
--threshold), their cross-checks, the mask they select, and the per-grasp arrays of a --report file."""
from __future__ import annotations

import numpy as np

REPORT_KEYS = ("contact_idx", "normals", "angles", "region_count", "region_weight", "collision_weight", "feasible")


def add_object_options(ap, query_does: str, hull_does: str = None) -> None:
    """--object-points (only with `hull_does`), --positives, --negatives, --threshold; the two arguments end the
    help strings of --positives and --object-points."""
    if hull_does:
        ap.add_argument("--object-points", default=None, help="object point cloud (world frame): its convex hull "
                                                              + hull_does)
    ap.add_argument("--positives", default=None, help=".npy text embeddings: " + query_does)
    ap.add_argument("--negatives", default=None, help=".npy canonical negatives (LERF relevancy)")
    ap.add_argument("--threshold", type=float, default=None, help="relevancy threshold for --positives")


def check_object_options(ap, a, hull: str) -> None:
    """ap.error unless the selection is complete.  hull "optional": --object-points or --positives or neither;
    "required": exactly one of them; "none": the parser has no --object-points, and stray --negatives / --threshold
    pass."""
    if hull == "required" and bool(a.object_points) == bool(a.positives):
        ap.error("one of --object-points and --positives is needed (they are alternatives)")
    if hull == "optional" and a.object_points and a.positives:
        ap.error("--object-points and --positives are alternatives")
    if a.positives and (a.threshold is None or not a.negatives):
        ap.error("--positives needs --negatives and --threshold (LERF relevancy, query.select_gaussians)")
    if hull != "none" and (a.negatives or a.threshold is not None) and not a.positives:
        ap.error("--negatives / --threshold need --positives")


def object_mask(a, scene, mlp_state, matrix=None, scale: float = 1.0):
    """(N,) mask on the scene's device of the Gaussians the parsed options select, None without a selection.
    matrix, scale: the world -> scene map of the object points (None: identity)."""
    if getattr(a, "object_points", None):
        from . import edit
        pts = edit.filter_object_points(edit.object_points_to_scene(
            edit.load_object_points(a.object_points), np.eye(4) if matrix is None else matrix, scale))
        return edit.select_and_move(scene.means.contiguous(), None, edit.hull_planes(pts))[0]
    if a.positives:
        from . import query
        from .interop import fea_up_weights
        w = fea_up_weights(mlp_state, scene.means.device, a.ckpt, "for --positives")
        return query.select_gaussians(scene, w, query.load_embeddings(a.positives, "positives"),
                                      query.load_embeddings(a.negatives, "negatives"), a.threshold)
    return None
