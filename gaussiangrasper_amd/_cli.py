"""What the command lines of grasp, grasp_propose, mesh and cluster share: the options that say which Gaussians are
the object (the convex hull of --object-points, or the LERF relevancy of --positives against --negatives above
--threshold — per Gaussian, or with --views in rendered views and lifted — or the 2-D masks of --object-masks lifted
over --views; of that selection, with --instance, one DBSCAN instance), their cross-checks, the mask they select, and
the per-grasp arrays of a --report file; and the options of the support plane (--support-plane fits or loads the
table's plane, --remove-support takes the Gaussians that are not above it out of the selection, and the grasp command
lines also hold the gripper above it)."""
from __future__ import annotations

import argparse
import math

import numpy as np

REPORT_KEYS = ("contact_idx", "normals", "angles", "region_count", "region_weight", "collision_weight", "feasible")
CLEAR_KEYS = ("body_weight", "sweep_weight", "body_count", "sweep_count", "clear")     # only with --gripper
NMS_KEYS = ("keep", "suppressor", "support")             # only with --nms-translation, as nms_keep, ...
NMS_ROTATION_DEGREES = 30.0                              # grasp.NMS_ROTATION


def load_scene(ckpt: str):
    """(scene, mlp_state) of a checkpoint, the scene on the device."""
    from .interop import load_checkpoint
    scene, mlp_state, _ = load_checkpoint(ckpt)
    return scene.to("cuda"), mlp_state


def add_gripper_sphere_options(ap, prefix: str = "") -> None:
    """--gripper, --width, --depth, --height, --radius, --margin: a gripper model covered by spheres
    (field.gripper_spheres).  `prefix` starts every help string; without one --gripper is required."""
    ap.add_argument("--gripper", default=None, required=not prefix, metavar="{default,FILE.json}",
                    help=prefix + "the gripper model")
    ap.add_argument("--width", type=float, default=0.08, help=prefix + "the gripper's opening, scene units")
    ap.add_argument("--depth", type=float, default=0.02, help=prefix + "the fingers' depth")
    ap.add_argument("--height", type=float, default=0.02, help=prefix + "the fingers' height")
    ap.add_argument("--radius", type=float, default=0.005, help=prefix + "radius of the covering spheres")
    ap.add_argument("--margin", type=float, default=0.0, help=prefix + "clearance kept beyond the spheres")


def add_grasp_options(ap) -> None:
    """What the grasp and grasp_propose command lines share: --mu, --min-opacity, --max-collision (grasp.contacts);
    --gripper, --approach, --max-body-collision, --max-sweep-collision (grasp.clearance); --nms-translation,
    --nms-rotation, --nms-no-symmetry, --top-k (grasp.nms); and add_support_options."""
    from .grasp import MIN_WEIGHT, MU
    ap.add_argument("--mu", type=float, default=MU, help="friction coefficient")
    ap.add_argument("--min-opacity", type=float, default=MIN_WEIGHT, help="a Gaussian takes part above it")
    ap.add_argument("--max-collision", type=float, default=None, help="limit on the opacity inside the fingers")
    ap.add_argument("--gripper", default=None, metavar="{default,FILE.json}",
                    help="also test the whole gripper against the whole scene: graspnetAPI's drawing (default) or a "
                         "JSON list of parts (grasp.load_gripper)")
    ap.add_argument("--approach", type=float, default=None, metavar="METRES",
                    help="with --gripper: length of the straight approach that is swept, grasp units (default 0)")
    ap.add_argument("--max-body-collision", type=float, default=None,
                    help="with --gripper: limit on the opacity inside the gripper at the final pose")
    ap.add_argument("--max-sweep-collision", type=float, default=None,
                    help="with --gripper: limit on the opacity the gripper passes through on its approach")
    ap.add_argument("--nms-translation", type=float, default=None, metavar="METRES",
                    help="keep distinct grasps only: of the feasible rows, best first, drop one that is within this "
                         "distance (grasp units) and --nms-rotation of a kept one")
    ap.add_argument("--nms-rotation", type=float, default=None, metavar="DEGREES",
                    help=f"with --nms-translation: the rotation that still counts as near (default "
                         f"{NMS_ROTATION_DEGREES:g})")
    ap.add_argument("--nms-no-symmetry", action="store_true",
                    help="with --nms-translation: a pose and its half turn about the approach axis are two grasps")
    ap.add_argument("--top-k", type=int, default=None, metavar="K",
                    help="with --nms-translation: write the best K distinct grasps only")
    add_support_options(ap)


def check_grasp_options(ap, a, lengths=()) -> None:
    """ap.error unless the options of add_grasp_options (and the caller's own `lengths`, checked like --mu) are complete
    and in range; a.approach None becomes 0, a.nms_rotation None the default, a.support_margin None 0."""
    for name in ("mu", *lengths, "min_opacity"):
        v = getattr(a, name)
        if not (math.isfinite(v) and v >= 0.0):
            ap.error(f"--{name.replace('_', '-')} must be finite and >= 0, got {v}")
    if a.max_collision is not None and math.isnan(a.max_collision):
        ap.error("--max-collision must not be NaN")
    for n in ("approach", "max_body_collision", "max_sweep_collision"):
        v = getattr(a, n)
        if v is None:
            continue
        opt = "--" + n.replace("_", "-")
        if not a.gripper:
            ap.error(f"{opt} needs --gripper")
        if math.isnan(v):
            ap.error(f"{opt} must not be NaN")
    if a.approach is not None and not (math.isfinite(a.approach) and a.approach >= 0.0):
        ap.error(f"--approach must be finite and >= 0, got {a.approach}")
    if a.approach is None:
        a.approach = 0.0
    if a.nms_translation is None:
        for n, given in (("nms_rotation", a.nms_rotation is not None), ("nms_no_symmetry", a.nms_no_symmetry),
                         ("top_k", a.top_k is not None)):
            if given:
                ap.error("--" + n.replace("_", "-") + " needs --nms-translation")
    elif not (math.isfinite(a.nms_translation) and a.nms_translation >= 0.0):
        ap.error(f"--nms-translation must be finite and >= 0, got {a.nms_translation}")
    if a.nms_rotation is not None and not 0.0 <= a.nms_rotation <= 180.0:        # NaN fails
        ap.error(f"--nms-rotation must be in 0..180 degrees, got {a.nms_rotation}")
    if a.top_k is not None and a.top_k < 1:
        ap.error(f"--top-k must be >= 1, got {a.top_k}")
    if a.nms_rotation is None:
        a.nms_rotation = NMS_ROTATION_DEGREES
    check_support_options(ap, a)


def grasp_gate_kwargs(a, plane) -> dict:
    """The keywords grasp.score_grasps and grasp_propose.grasp_object take from the checked options of add_grasp_options
    (the gripper apart, which the command lines load first), degrees as radians; `plane`: support_option_plane's."""
    return dict(mu=a.mu, min_weight=a.min_opacity, max_collision=a.max_collision, approach=a.approach,
                max_body=a.max_body_collision, max_sweep=a.max_sweep_collision, nms_translation=a.nms_translation,
                nms_rotation=math.radians(a.nms_rotation), nms_symmetric=not a.nms_no_symmetry, top_k=a.top_k,
                support=plane, support_margin=a.support_margin,
                max_approach_tilt=None if a.max_approach_tilt is None else math.radians(a.max_approach_tilt))


def add_support_options(ap, grasp: bool = True) -> None:
    """--support-plane, --support-dist and --remove-support (support.support_plane, support.above); with `grasp` also
    --support-margin and --max-approach-tilt (grasp.plane_clear)."""
    ap.add_argument("--support-plane", default=None, metavar="{fit,FILE.json}",
                    help="the table's plane, scene frame: fitted to the Gaussians around the selection (fit; around "
                         "all of them without a selection) or read from a file support.save_plane wrote"
                         + ("; the whole gripper and its approach must stay above it (needs --gripper)" if grasp
                            else ""))
    ap.add_argument("--support-dist", type=float, default=None, metavar="METRES",
                    help="with --support-plane fit: half thickness of the plane's slab (default 0.01)")
    ap.add_argument("--remove-support", action="store_true",
                    help="with --support-plane: keep only the selected Gaussians above the plane's slab")
    if grasp:
        ap.add_argument("--support-margin", type=float, default=None, metavar="METRES",
                        help="with --support-plane: the gripper stays this far above the plane (default 0)")
        ap.add_argument("--max-approach-tilt", type=float, default=None, metavar="DEGREES",
                        help="with --support-plane: the approach axis is within this of the plane's inward normal")


def check_support_options(ap, a, grasp: bool = True) -> None:
    """ap.error unless the support options are complete and in range; a.support_margin None becomes 0."""
    given = [("support_dist", a.support_dist is not None), ("remove_support", a.remove_support)]
    if grasp:
        given += [("support_margin", a.support_margin is not None),
                  ("max_approach_tilt", a.max_approach_tilt is not None)]
    if not a.support_plane:
        for n, g in given:
            if g:
                ap.error("--" + n.replace("_", "-") + " needs --support-plane")
    elif grasp and not a.gripper:
        ap.error("--support-plane needs --gripper: the plane test has to know which boxes must stay above the plane")
    if a.support_dist is not None:
        if a.support_plane != "fit":
            ap.error("--support-dist goes with --support-plane fit (a plane file holds its own)")
        if not (math.isfinite(a.support_dist) and a.support_dist >= 0.0):
            ap.error(f"--support-dist must be finite and >= 0, got {a.support_dist}")
    if a.remove_support and not (getattr(a, "object_points", None) or a.positives or getattr(a, "object_masks", None)):
        ap.error("--remove-support needs a selection to remove the support from")
    if grasp:
        if a.support_margin is not None and not math.isfinite(a.support_margin):
            ap.error(f"--support-margin must be finite, got {a.support_margin}")
        if a.max_approach_tilt is not None and not 0.0 <= a.max_approach_tilt <= 180.0:        # NaN fails
            ap.error(f"--max-approach-tilt must be in 0..180 degrees, got {a.max_approach_tilt}")
        if a.support_margin is None:
            a.support_margin = 0.0


def support_option_plane(a, scene, mask, scale: float = 1.0, up=None):
    """The support.SupportPlane the parsed --support-plane asks for, None without the option: fitted around `mask`
    (support.support_plane; --support-dist metres, times scale; `up` orients the normal) or loaded and labelled
    against the scene's Gaussians.  Made once per parsed `a` and kept on it, so that --remove-support and the grasp
    layer see the same plane."""
    if not getattr(a, "support_plane", None):
        return None
    if getattr(a, "_support_fitted", None) is None:
        from . import support
        if a.support_plane == "fit":
            kw = {} if a.support_dist is None else {"dist": a.support_dist}
            a._support_fitted = support.support_plane(scene, mask, scale=scale, up=up, **kw)
        else:
            a._support_fitted = support.label_model(scene, support.load_plane(a.support_plane))
    return a._support_fitted


def report_arrays(res) -> dict:
    """The per-grasp arrays of a --report file: REPORT_KEYS of a GraspContacts, CLEAR_KEYS of its .clearance when it
    has one, NMS_KEYS of its .nms, as nms_keep, nms_suppressor and nms_support, when it has one, and support_clear
    and support_lowest when a support plane was applied."""
    out = {k: getattr(res, k).cpu().numpy() for k in REPORT_KEYS}
    if res.clearance is not None:
        out.update({k: getattr(res.clearance, k).cpu().numpy() for k in CLEAR_KEYS})
    if getattr(res, "nms", None) is not None:
        out.update({"nms_" + k: getattr(res.nms, k).cpu().numpy() for k in NMS_KEYS})
    for k in ("support_clear", "support_lowest"):
        if getattr(res, k, None) is not None:
            out[k] = getattr(res, k).cpu().numpy()
    return out


def instance_choice(text: str):
    """--instance: "all", "largest" (rank 0) or a rank K >= 0."""
    if text in ("all", "largest"):
        return text
    try:
        k = int(text)
    except ValueError:
        k = -1
    if k < 0:
        raise argparse.ArgumentTypeError(f"expected all, largest or a rank >= 0, got {text!r}")
    return k


def add_object_options(ap, query_does: str, hull_does: str = None, instances: bool = True) -> None:
    """--object-points (only with `hull_does`), --positives, --negatives, --threshold; the two arguments end the
    help strings of --positives and --object-points.  With `instances`, also --instance and the --cluster-* options
    that go with it."""
    if hull_does:
        ap.add_argument("--object-points", default=None, help="object point cloud (world frame): its convex hull "
                                                              + hull_does)
    ap.add_argument("--positives", default=None, help=".npy text embeddings: " + query_does)
    ap.add_argument("--negatives", default=None, help=".npy canonical negatives (LERF relevancy)")
    ap.add_argument("--threshold", type=float, default=None, help="relevancy threshold for --positives")
    ap.add_argument("--views", default=None, metavar="T.json",
                    help="a scan's transforms.json (OpenCV c2w, raw frame; --transform-json maps it): with --positives "
                         "the relevancy is thresholded in these rendered views and lifted onto the Gaussians "
                         "(query.select_gaussians_in_views) instead of being taken per Gaussian")
    ap.add_argument("--object-masks", default=None, metavar="DIR",
                    help="with --views: one 2-D mask per frame, named by the frame's file stem; the Gaussians that "
                         "carry label 1 are the object (lift.lift_labels)")
    if instances:
        ap.add_argument("--instance", type=instance_choice, default="all", metavar="{all,largest,K}",
                        help="of the selection, keep one DBSCAN instance (cluster.object_instances): the heaviest, or "
                             "the one of rank K; all: the selection as it is")
        ap.add_argument("--cluster-eps", type=float, default=None,
                        help="with --instance: neighbour radius, world units (default: derived from the selection)")
        ap.add_argument("--cluster-eps-scale", type=float, default=None,
                        help="with --instance: eps = this times the selection's median 3rd-neighbour distance")
        ap.add_argument("--cluster-min-points", type=int, default=None,
                        help="with --instance: neighbours within eps that make a core point")


def check_object_options(ap, a, hull: str) -> None:
    """ap.error unless the selection is complete.  hull "optional": --object-points or --positives or neither;
    "required": exactly one of them; "none": the parser has no --object-points, and stray --negatives / --threshold
    pass."""
    views, masks = getattr(a, "views", None), getattr(a, "object_masks", None)
    if masks and not views:
        ap.error("--object-masks needs --views (the cameras the masks belong to)")
    if masks and (a.positives or getattr(a, "object_points", None)):
        ap.error("--object-masks is an alternative to --positives" + ("" if hull == "none" else " and --object-points"))
    if views and not (masks or a.positives):
        ap.error("--views needs --positives or --object-masks")
    if hull == "required" and bool(a.object_points) == bool(a.positives) and not masks:
        ap.error("one of --object-points and --positives is needed (they are alternatives)")
    if hull == "optional" and a.object_points and a.positives:
        ap.error("--object-points and --positives are alternatives")
    if a.positives and (a.threshold is None or not a.negatives):
        ap.error("--positives needs --negatives and --threshold (LERF relevancy, query.select_gaussians)")
    if hull != "none" and (a.negatives or a.threshold is not None) and not a.positives:
        ap.error("--negatives / --threshold need --positives")
    inst = getattr(a, "instance", "all")
    given = [n for n in ("cluster_eps", "cluster_eps_scale", "cluster_min_points") if getattr(a, n, None) is not None]
    if given and inst == "all":
        ap.error("--" + given[0].replace("_", "-") + " needs --instance largest or --instance K")
    if inst != "all" and not (getattr(a, "object_points", None) or a.positives or masks):
        ap.error("--instance needs a selection (--positives" + (")" if hull == "none" else " or --object-points)"))
    for n in ("cluster_eps", "cluster_eps_scale"):
        v = getattr(a, n, None)
        if v is not None and not (math.isfinite(v) and v > 0.0):
            ap.error(f"--{n.replace('_', '-')} must be finite and > 0, got {v}")
    if getattr(a, "cluster_eps", None) is not None and getattr(a, "cluster_eps_scale", None) is not None:
        ap.error("--cluster-eps and --cluster-eps-scale are alternatives")
    if getattr(a, "cluster_min_points", None) is not None and a.cluster_min_points < 1:
        ap.error(f"--cluster-min-points must be >= 1, got {a.cluster_min_points}")


def object_mask(a, scene, mlp_state, matrix=None, scale: float = 1.0):
    """(N,) mask on the scene's device of the Gaussians the parsed options select, None without a selection.
    matrix, scale: the world -> scene map of the object points (None: identity).  With --instance largest or K,
    that selection's instance of that rank (cluster.object_instances; --cluster-eps times scale).  With
    --remove-support, the selection is first cut to support.above(selection, plane), the plane of
    support_option_plane around the selection."""
    mask = selection_mask(a, scene, mlp_state, matrix, scale)
    if mask is not None and getattr(a, "remove_support", False):
        from . import support
        mask = support.above(mask, support_option_plane(a, scene, mask, scale, getattr(a, "support_up", None)))
    inst = getattr(a, "instance", "all")
    if inst == "all" or mask is None:
        return mask
    from . import cluster
    kw = {}
    if a.cluster_eps_scale is not None:
        kw["eps_scale"] = a.cluster_eps_scale
    if a.cluster_min_points is not None:
        kw["min_points"] = a.cluster_min_points
    found = cluster.object_instances(scene, mask, None if a.cluster_eps is None else a.cluster_eps * float(scale),
                                     **kw)
    rank = 0 if inst == "largest" else inst
    if rank >= len(found):
        raise ValueError(f"--instance {inst}: the selection has {len(found)} instances")
    return cluster.instance_mask(found, rank)


def selection_mask(a, scene, mlp_state, matrix=None, scale: float = 1.0):
    """object_mask before --instance: the hull's or the query's Gaussians, None without a selection."""
    if getattr(a, "object_points", None):
        from . import edit
        pts = edit.filter_object_points(edit.object_points_to_scene(
            edit.load_object_points(a.object_points), np.eye(4) if matrix is None else matrix, scale))
        return edit.select_and_move(scene.means.contiguous(), None, edit.hull_planes(pts))[0]
    if getattr(a, "object_masks", None):
        from . import lift
        cams, _ = lift.scene_cameras(a.views, getattr(a, "transform_json", None))
        labs = [lift.read_label_image(lift.find_mask(a.object_masks, st)) for st in lift.frame_stems(a.views)]
        top = max(int(m[m != lift.IGNORE].max(initial=0)) for m in labs)
        return lift.select(lift.lift_labels(scene, cams, labs, max(top, 1) + 1).votes, 1)
    if a.positives:
        from . import query
        from .interop import fea_up_weights
        w = fea_up_weights(mlp_state, scene.means.device, a.ckpt, "for --positives")
        if getattr(a, "views", None):
            from . import lift
            cams, _ = lift.scene_cameras(a.views, getattr(a, "transform_json", None))
            return query.select_gaussians_in_views(scene, w, cams, query.load_embeddings(a.positives, "positives"),
                                                   query.load_embeddings(a.negatives, "negatives"), a.threshold)
        return query.select_gaussians(scene, w, query.load_embeddings(a.positives, "positives"),
                                      query.load_embeddings(a.negatives, "negatives"), a.threshold)
    return None
