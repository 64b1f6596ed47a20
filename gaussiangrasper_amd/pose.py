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
