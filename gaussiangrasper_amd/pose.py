"""Camera pose refinement against the Gaussian field.

The projection's backward carries the image cotangents to the camera (csrc/project.hip: the pose VJP of
gg_view_bwd_pose / gg_project_pose_bwd, reached through ops.ViewGeometry when `viewmat` or `full_proj` requires grad).
This module holds the pieces on top of it:

  exp_map_so3xr3 / exp_map_se3   the two tangent parametrisations of the reference's camera optimizer
                                 (CameraOptimizerConfig.mode "SO3xR3" / "SE3": a (k, 6) tangent -> (k, 3, 4) [R | t],
                                 translation first, rotation second), written from the closed forms
  refine_camera                  relocalise one camera against an observed RGB(-D) frame with the Gaussians frozen:
                                 the correction `c2w @ adj` (the reference's apply_to_camera convention) is fitted by
                                 L-BFGS through the plugin model's own get_outputs
  object_transform               the rigid motion of an object as ops.RigidMove takes it, (rt, qt), from a tangent: the
                                 rotation about a centre, composed on the left of a known motion
  refine_object                  re-localise a rigid object (a masked subset of the Gaussians) against observed RGB(-D)
                                 frames with every Gaussian frozen and the rest of the scene occluding: the twin of
                                 refine_camera, through the plugin model's object_pose hook or any render callable
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch


def _skew(w: torch.Tensor) -> torch.Tensor:
    """(k, 3) -> (k, 3, 3) cross-product matrices"""
    z = torch.zeros_like(w[:, 0])
    return torch.stack((torch.stack((z, -w[:, 2], w[:, 1]), -1),
                        torch.stack((w[:, 2], z, -w[:, 0]), -1),
                        torch.stack((-w[:, 1], w[:, 0], z), -1)), -2)


def _rodrigues_coeffs(theta2: torch.Tensor):
    """sin(t)/t, (1 - cos t)/t^2, (t - sin t)/t^3 of t = sqrt(theta2); Taylor series below t = 1e-2 (no 0/0, and a
    gradient at exactly zero)"""
    small = theta2 < 1e-4
    t2 = torch.where(small, torch.ones_like(theta2), theta2)
    t = t2.sqrt()
    a = torch.where(small, 1.0 - theta2 / 6.0 + theta2 * theta2 / 120.0, t.sin() / t)
    b = torch.where(small, 0.5 - theta2 / 24.0 + theta2 * theta2 / 720.0, (1.0 - t.cos()) / t2)
    c = torch.where(small, 1.0 / 6.0 - theta2 / 120.0 + theta2 * theta2 / 5040.0, (t - t.sin()) / (t2 * t))
    return a, b, c


def exp_map_so3xr3(tangent: torch.Tensor) -> torch.Tensor:
    """(k, 6) = [translation | rotation vector] -> (k, 3, 4) [exp(rotation) | translation]"""
    w = tangent[:, 3:]
    a, b, _ = _rodrigues_coeffs((w * w).sum(-1))
    K = _skew(w)
    eye = torch.eye(3, dtype=tangent.dtype, device=tangent.device)[None]
    R = eye + a[:, None, None] * K + b[:, None, None] * (K @ K)
    return torch.cat((R, tangent[:, :3, None]), dim=-1)


def exp_map_se3(tangent: torch.Tensor) -> torch.Tensor:
    """(k, 6) = [rho | rotation vector] in se(3) -> (k, 3, 4) [R | V rho], V the left Jacobian of SO(3)"""
    w = tangent[:, 3:]
    a, b, c = _rodrigues_coeffs((w * w).sum(-1))
    K = _skew(w)
    KK = K @ K
    eye = torch.eye(3, dtype=tangent.dtype, device=tangent.device)[None]
    R = eye + a[:, None, None] * K + b[:, None, None] * KK
    V = eye + b[:, None, None] * K + c[:, None, None] * KK
    return torch.cat((R, V @ tangent[:, :3, None]), dim=-1)


def exp_map(tangent: torch.Tensor, mode: str = "SO3xR3") -> torch.Tensor:
    if mode == "SO3xR3":
        return exp_map_so3xr3(tangent)
    if mode == "SE3":
        return exp_map_se3(tangent)
    raise ValueError(f"unknown camera optimizer mode {mode!r} (SO3xR3 or SE3)")


def homogeneous(adj: torch.Tensor) -> torch.Tensor:
    """(k, 3, 4) -> (k, 4, 4) with the row [0, 0, 0, 1]"""
    last = torch.zeros(adj.shape[0], 1, 4, dtype=adj.dtype, device=adj.device)
    last[:, 0, 3] = 1.0
    return torch.cat((adj, last), dim=1)


def _half_angle_coeffs(theta2: torch.Tensor):
    """cos(t / 2), sin(t / 2) / t of t = sqrt(theta2), with _rodrigues_coeffs' guard: Taylor series below t = 1e-2"""
    small = theta2 < 1e-4
    t2 = torch.where(small, torch.ones_like(theta2), theta2)
    t = t2.sqrt()
    c = torch.where(small, 1.0 - theta2 / 8.0 + theta2 * theta2 / 384.0, (0.5 * t).cos())
    s = torch.where(small, 0.5 - theta2 / 48.0 + theta2 * theta2 / 3840.0, (0.5 * t).sin() / t)
    return c, s


def _quat_mul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack((w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2), -1)


def rotmat_to_quat(R: torch.Tensor) -> torch.Tensor:
    """(3, 3) rotation -> (4,) wxyz unit quaternion with w >= 0 (Shepperd: the branch of the largest of the trace
    and the diagonal, so no division by a small number).  A constant of the fit (`base`): computed on the host."""
    m = R.detach().double().cpu()
    tr = float(m[0, 0] + m[1, 1] + m[2, 2])
    cand = [tr, float(m[0, 0]), float(m[1, 1]), float(m[2, 2])]
    k = max(range(4), key=lambda i: cand[i])
    if k == 0:
        s = 2.0 * (1.0 + tr) ** 0.5
        q = [0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s]
    else:
        i = k - 1
        j, l = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * float(1.0 + m[i, i] - m[j, j] - m[l, l]) ** 0.5
        q = [0.0] * 4
        q[0] = (m[l, j] - m[j, l]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (m[j, i] + m[i, j]) / s
        q[1 + l] = (m[l, i] + m[i, l]) / s
    q = torch.tensor([float(v) for v in q], dtype=torch.float64)
    q = q / q.norm()
    return -q if q[0] < 0 else q


def object_transform(delta: torch.Tensor, base: Optional[torch.Tensor] = None, centre: Optional[torch.Tensor] = None,
                     mode: str = "SO3xR3") -> Tuple[torch.Tensor, torch.Tensor]:
    """The rigid motion of an object as ops.RigidMove takes it: (rt (3, 4) = [R | t], qt (4,) wxyz, the quaternion
    of R), in torch, differentiable in `delta`.

    delta: exp_map's tangent, (6,) or (1, 6) = [translation | rotation vector].  Its rotation turns the object about
    `centre` (3,) — the selection's centroid; None: the origin — and its translation follows:
    D x = exp(w) (x - c) + c + t.  D is composed on the LEFT of `base` (4, 4) or (3, 4), the motion already known
    (the arm's report; None: identity): T = D base.  qt = (cos(th / 2), sin(th / 2) w / th) (x) quat(base), with the
    series of _rodrigues_coeffs' guard below th = 1e-2, so the gradient at delta = 0 is finite."""
    d = delta.reshape(1, 6)
    adj = exp_map(d, mode)[0]
    R, t = adj[:, :3], adj[:, 3]
    w = d[0, 3:]
    c, s = _half_angle_coeffs((w * w).sum())
    q = torch.cat((c.reshape(1), s * w))
    if centre is not None:
        cen = centre.detach().to(device=d.device, dtype=d.dtype).reshape(3)
        t = t + cen - R @ cen
    if base is not None:
        b = base.detach().to(device=d.device, dtype=d.dtype)
        Rb, tb = b[:3, :3], b[:3, 3]
        t = R @ tb + t
        R = R @ Rb
        q = _quat_mul(q, rotmat_to_quat(Rb).to(device=d.device, dtype=d.dtype))
    return torch.cat((R, t[:, None]), dim=1), q


def refine_object(model_or_render, mask: torch.Tensor, cameras, rgbs, depths=None, valids=None,
                  base: Optional[torch.Tensor] = None, steps: int = 100, depth_weight: float = 1.0, lr: float = 1.0,
                  mode: str = "SO3xR3", means: Optional[torch.Tensor] = None, quats: Optional[torch.Tensor] = None,
                  centre: Optional[torch.Tensor] = None, rigid_move=None, restart_every: int = 10
                  ) -> Tuple[torch.Tensor, List[float]]:
    """Re-localise a rigid object against observed RGB(-D) frames with every Gaussian frozen: the six numbers `delta`
    of object_transform(delta, base, centre) are fitted so that the scene with the rows `mask` selects moved by that
    transform renders like the frames.  refine_camera's loss (mean squared rgb error + depth_weight * mean squared
    depth error over the valid pixels) summed over the views, and its L-BFGS settings; at most `steps` evaluations
    (one evaluation renders every view).  The rest of the scene stays where it is and occludes, which is what makes
    this no camera motion.

    model_or_render: a plugin model on the GPU — each view is `model.get_outputs(cameras[k])` with
    `model.object_pose = (mask, rt, qt)` set (the hook moves `means` / `quats` through ops.RigidMove) — or a
    callable `render(means, quats, k) -> {"rgb": (H, W, 3), "depth": (H, W, 1) or (H, W)}` for view k, e.g.
    `lambda m, q, k: pipeline.render_view(Scene(m, ...), views[k], ops)` with any operator namespace; then `means`
    (N, 3) and `quats` (N, 4) are the scene's and the move is `rigid_move` (default ops.RigidMove), once per
    evaluation.  mask (N,) uint8 / bool.  cameras: one per frame (unused by a callable beyond their number: None is
    fine).  rgbs / depths / valids: per view (H, W, 3), (H, W) or (H, W, 1), (H, W) bool (e.g. edit_masks' union);
    depths and valids optional.  base (4, 4): the motion the arm reports (None: identity).  centre: the pivot of the
    rotation (default: the centroid of the selected means, where `base` puts it).  SH coefficients are not rotated inside the loop.

    Two things are this function's own on top of refine_camera's optimiser: the rotation unknowns are scaled by the
    object's radius (the loss is ~r^2 flatter in a radian than in a scene unit, and L-BFGS spends its budget learning
    that), and the optimiser is started afresh from the best point every `restart_every` evaluations (see below).

    Returns (T (4, 4) = [exp(delta) about centre] base for the delta of the lowest loss seen, the loss of every
    evaluation: never more than `steps` of them).  The model's parameters, train / eval mode and object_pose are left
    as they were."""
    from . import ops as _ops
    is_model = not callable(model_or_render) or hasattr(model_or_render, "get_outputs")
    if is_model:
        model = model_or_render
        means, quats = model.means.detach(), model.quats.detach()
    elif means is None or quats is None:
        raise ValueError("refine_object with a render callable needs means= and quats=")
    else:
        means, quats = means.detach(), quats.detach()
    move = rigid_move or _ops.RigidMove
    dev, dtype = means.device, torch.float32
    n_views = len(rgbs)
    if n_views == 0:
        raise ValueError("refine_object needs at least one frame")
    sel = mask.to(dev) != 0
    if mask.shape != (means.shape[0],):
        raise ValueError(f"mask must be (N,) = ({means.shape[0]},), got {tuple(mask.shape)}")
    mask_u8 = sel.to(torch.uint8)
    if centre is None:
        if not bool(sel.any()):
            raise ValueError("refine_object: the mask selects no Gaussian")
        centre = means[sel].double().mean(dim=0)
        if base is not None:            # where `base` puts the centroid: the correction turns the object about itself
            b64 = torch.as_tensor(base).detach().to(device=dev, dtype=torch.float64)
            centre = b64[:3, :3] @ centre + b64[:3, 3]
    centre = centre.detach().to(device=dev, dtype=dtype)
    base_t = None if base is None else torch.as_tensor(base).detach().to(device=dev, dtype=dtype)
    targets = [t.to(device=dev, dtype=dtype) for t in rgbs]
    target_d = None if depths is None else [d.to(device=dev, dtype=dtype).reshape(t.shape[:2])
                                            for d, t in zip(depths, targets)]
    weights = None if valids is None else [v.to(device=dev).reshape(t.shape[:2]).to(dtype)
                                           for v, t in zip(valids, targets)]
    # The optimiser's variable is u with delta = u * unit: translations in scene units, rotations in units of
    # 1 / radius radians (radius: the selected means' RMS distance from their centroid), so that a unit of either moves
    # the object's Gaussians about as far and the two curvatures of the loss are of one order
    radius = 1.0
    if bool(sel.any()):
        own = means[sel].double()
        radius = float((own - own.mean(dim=0)).square().sum(dim=1).mean().sqrt())
    unit = torch.tensor([1.0] * 3 + [1.0 / max(radius, 1e-6)] * 3, device=dev, dtype=dtype)
    u = torch.zeros(6, device=dev, dtype=dtype, requires_grad=True)
    losses = []
    best = [float("inf"), u.detach().clone()]

    class _BudgetSpent(Exception):
        pass

    def masked_mean(err, k):
        if weights is None:
            return err.mean()
        return (err * weights[k]).sum() / weights[k].sum().clamp_min(1.0)

    def closure():
        if len(losses) >= steps:        # torch's L-BFGS checks max_eval between iterations only: a line search may
            raise _BudgetSpent()        # run past it.  `steps` evaluations is a promise, so it is held here
        u.grad = None
        rt, qt = object_transform(u * unit, base_t, centre, mode)
        if not is_model:
            moved = move(means, quats, mask_u8, rt, qt)
        loss = 0.0
        for k in range(n_views):
            if is_model:
                model.object_pose = (mask_u8, rt, qt)
                out = model.get_outputs(cameras[k])
            else:
                out = model_or_render(moved[0], moved[1], k)
            if "depth" not in out:
                raise RuntimeError(f"refine_object: nothing of the field is visible in view {k}")
            loss = loss + masked_mean(((out["rgb"] - targets[k]) ** 2).sum(-1), k)
            if target_d is not None:
                loss = loss + depth_weight * masked_mean((out["depth"].reshape(target_d[k].shape) - target_d[k]) ** 2, k)
        loss.backward()
        losses.append(loss.detach())
        value = float(loss.detach())    # (L-BFGS reads it back anyway)
        if value < best[0]:             # a line search that is cut short leaves `u` at a trial point
            best[0], best[1] = value, u.detach().clone()
        return loss

    if is_model:
        params = [(p, p.requires_grad) for p in model.parameters()]
        was_training, saved_pose = model.training, model.object_pose
    try:
        if is_model:
            for p, _ in params:
                p.requires_grad_(False)     # frozen Gaussians: RigidMove's pose-only backward
            model.eval()
        # Rounds of `restart_every` evaluations, each a fresh L-BFGS from the best point so far.  The rendered loss has
        # small jumps (two Gaussians swapping depth order, an alpha crossing 1 / 255); a line search that lands on one
        # leaves a curvature pair that shrinks every later step to nothing while the gradient is still far from zero.
        # A fresh start forgets it and takes a gradient step of sensible length (min(1, 1 / |g|_1) lr).
        try:
            while len(losses) < steps:
                before = best[0]
                with torch.no_grad():
                    u.copy_(best[1])
                opt = torch.optim.LBFGS([u], lr=lr, max_iter=restart_every, max_eval=restart_every,
                                        history_size=20, line_search_fn="strong_wolfe", tolerance_grad=1e-12,
                                        tolerance_change=1e-14)
                opt.step(closure)
                if not best[0] < before:
                    break                   # a whole round without a lower loss: converged, or nothing to gain
        except _BudgetSpent:
            pass
    finally:
        if is_model:
            for p, req in params:
                p.requires_grad_(req)
            model.train(was_training)
            model.object_pose = saved_pose
    with torch.no_grad():
        rt, _ = object_transform(best[1] * unit, base_t, centre, mode)
        T = torch.cat((rt, torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=dev, dtype=dtype)), dim=0)
    return T, [float(v) for v in torch.stack(losses).cpu()] if losses else []


def refine_camera(model, camera, rgb: torch.Tensor, depth: Optional[torch.Tensor] = None,
                  valid: Optional[torch.Tensor] = None, steps: int = 100, lr: float = 1.0,
                  depth_weight: float = 1.0, mode: str = "SO3xR3") -> Tuple[torch.Tensor, List[float]]:
    """Estimate the pose correction of `camera` (one camera, `Cameras` or stub.StubCameras) that makes the model's
    render match an observed frame, with the Gaussians frozen.

    model: a plugin model (plugin.make_fused_model_class(...) instance) on the GPU.  rgb (H, W, 3) in [0, 1];
    depth (H, W) or (H, W, 1) in world units, optional; valid (H, W) bool, optional: the pixels the loss reads
    (observed depth holes, the robot's own arm ...).  Loss: mean squared rgb error + depth_weight * mean squared depth
    error over the valid pixels.  The correction is `camera_to_worlds @ [exp(delta) ; 0 0 0 1]` (the reference's
    apply_to_camera), delta (1, 6) fitted by L-BFGS with a strong-Wolfe line search (step length `lr`), at most
    `steps` renders.  Not Adam: a lateral translation and a rotation move the image almost alike (they differ by the
    parallax only), and Adam's per-coordinate steps crawl along that valley; L-BFGS's curvature estimate does not.

    Returns (corrected camera_to_worlds (1, 3, 4), the loss of every render).  The model's parameters, train / eval mode
    and the camera are left as they were."""
    base = camera.camera_to_worlds.detach().clone()
    if base.shape[0] != 1:
        raise ValueError("refine_camera takes one camera")
    dev = base.device
    target = rgb.to(device=dev, dtype=torch.float32)
    target_d = None if depth is None else depth.to(device=dev, dtype=torch.float32).reshape(target.shape[:2])
    mask = None if valid is None else valid.to(device=dev).reshape(target.shape[:2]).to(torch.float32)
    delta = torch.zeros(1, 6, device=dev, dtype=base.dtype, requires_grad=True)
    opt = torch.optim.LBFGS([delta], lr=lr, max_iter=steps, max_eval=steps, history_size=20,
                            line_search_fn="strong_wolfe", tolerance_grad=1e-12, tolerance_change=1e-14)
    params = [(p, p.requires_grad) for p in model.parameters()]
    was_training, saved = model.training, camera.camera_to_worlds
    losses = []

    def masked_mean(err):
        if mask is None:
            return err.mean()
        return (err * mask).sum() / mask.sum().clamp_min(1.0)

    def closure():
        opt.zero_grad(set_to_none=True)
        camera.camera_to_worlds = torch.bmm(base, homogeneous(exp_map(delta, mode)))
        out = model.get_outputs(camera)
        if "depth" not in out:
            raise RuntimeError("refine_camera: nothing of the field is visible from this camera")
        loss = masked_mean(((out["rgb"] - target) ** 2).sum(-1))
        if target_d is not None:
            loss = loss + depth_weight * masked_mean((out["depth"].reshape(target_d.shape) - target_d) ** 2)
        loss.backward()
        losses.append(loss.detach())
        return loss

    try:
        for p, _ in params:
            p.requires_grad_(False)         # frozen Gaussians: the projection's pose-only backward
        model.eval()
        if steps > 0:
            opt.step(closure)
    finally:
        for p, req in params:
            p.requires_grad_(req)
        model.train(was_training)
        camera.camera_to_worlds = saved
    with torch.no_grad():
        c2w = torch.bmm(base, homogeneous(exp_map(delta.detach(), mode)))
    return c2w, [float(v) for v in torch.stack(losses).cpu()] if losses else []
