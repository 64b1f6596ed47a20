"""Language query of the feature field: where in a view, or which Gaussians, match a text embedding.

The field's 32- or 128-channel features go through `fea_up` (32/128 -> 128 -> 512) into CLIP space, and a query
needs only a few numbers per row of that 512-dim output: the cosine similarity to each text embedding,
s_k = F.normalize(y) @ q_k, or LERF's relevancy against canonical negatives (Kerr et al. 2023),
r_p = min_j softmax(tau [s_p, s_nj])[0] = 1 / (1 + exp(tau (max_j s_nj - s_p))), tau = 10 by default.
One HIP kernel (`gg_clip_query`, csrc/query.hip) computes both without writing the 512-dim output to memory.

    clip_similarity(features, fea_up, queries)                 (..., Q) cosine similarities
    relevancy(features, fea_up, positives, negatives)          (..., P) relevancy
    relevancy_view(model, camera, positives, negatives)        {"relevancy": (H, W, P)[, "similarity": (H, W, Q)]}
    relevancy_gaussians(model_or_scene, fea_up, pos, neg)      (N, P) over the Gaussians' own features
    select_gaussians(model_or_scene, fea_up, pos, neg, t)      (N,) bool: semantic selection
    select_gaussians_in_views(model_or_scene, fea_up, cameras, pos, neg, t)
                                                               (N,) bool: the selection made in rendered views and
                                                               lifted onto the Gaussians (lift.py)
    python -m gaussiangrasper_amd.query --ckpt ... --positives pos.npy [--negatives neg.npy] --out scores.npy

`fea_up` is any module with Linear `layers[0]` / `layers[2]` (mlp.MLP, stub.MLP, the reference's MLP) or a tuple
(w1, b1, w2, b2).  Text embeddings come from outside the project (no CLIP model here); they are normalised on the
host in fp32.  Inference only: inputs are used detached, outputs carry no autograd history.

Shapes the kernel does not take — feature widths other than 32, 64 and 128, a CLIP width that is not a multiple of
16 or too wide for the LDS beside the query rows — go through `mlp.mlp_forward` and torch (F.normalize, a matrix
product, the closed-form relevancy) instead, with the 512-dim output materialised."""
from __future__ import annotations

import argparse
import math
import sys
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor

from . import _lib
from ._call import ArrayLike, ptr as _ptr, require_hip as _require_hip, stream as _stream
from .mlp import FAST_MAX_OUT, HIDDEN, mlp_forward

MAX_QUERIES = 8            # GG_QUERY_MAX: query rows per kernel launch (positives + negatives)
KERNEL_IN = (32, 64, 128)
DEFAULT_TEMPERATURE = 10.0


def _max_queries(out_dim: int) -> int:
    """Query rows one launch takes at this CLIP width: the LDS beside the two weight slices holds
    2 out_dim + 129 nq + 256 floats of 8192 (csrc/query.hip).  0: the kernel does not take the width."""
    if out_dim <= 0 or out_dim % 16 or out_dim > FAST_MAX_OUT:
        return 0
    return max(0, min(MAX_QUERIES, (8192 - 256 - 2 * out_dim) // (HIDDEN + 1)))


def _weights(fea_up) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    if isinstance(fea_up, (tuple, list)):
        if len(fea_up) != 4:
            raise ValueError("fea_up as a tuple must be (w1, b1, w2, b2)")
        w = tuple(fea_up)
    else:
        layers = getattr(fea_up, "layers", None)
        if layers is None or len(layers) != 3:
            raise ValueError("fea_up must have layers = (Linear, ReLU, Linear) (the reference's MLP with one hidden layer)")
        w = (layers[0].weight, layers[0].bias, layers[2].weight, layers[2].bias)
    w1, b1, w2, b2 = (torch.as_tensor(t).detach().float() for t in w)
    if w1.ndim != 2 or w1.shape[0] != HIDDEN or tuple(b1.shape) != (HIDDEN,) or w2.ndim != 2 or \
            w2.shape[1] != HIDDEN or tuple(b2.shape) != (w2.shape[0],):
        raise ValueError(f"expected w1 (128, D), b1 (128,), w2 (C, 128), b2 (C,), got {tuple(w1.shape)}, "
                         f"{tuple(b1.shape)}, {tuple(w2.shape)}, {tuple(b2.shape)}")
    return w1, b1, w2, b2


def _unit_rows(e: Optional[ArrayLike], out_dim: int, name: str) -> Tensor:
    """(K, out_dim) float32 unit rows on the host (a single embedding may be 1-D; None or empty: K = 0)."""
    if e is None:
        return torch.zeros(0, out_dim)
    t = e.detach().cpu().float() if isinstance(e, Tensor) else torch.as_tensor(np.asarray(e, dtype=np.float32))
    if t.ndim == 1 and t.numel() > 0:
        t = t[None]
    if t.numel() == 0:
        return torch.zeros(0, out_dim)
    if t.ndim != 2 or t.shape[1] != out_dim:
        raise ValueError(f"{name} must be (K, {out_dim}) embeddings (fea_up's output width), got {tuple(t.shape)}")
    if not torch.isfinite(t).all():
        raise ValueError(f"{name} contains non-finite values")
    n = torch.linalg.vector_norm(t, dim=1, keepdim=True)
    if (n == 0).any():
        raise ValueError(f"{name}: an embedding of zero norm has no direction")
    return (t / n).contiguous()


def _check_temperature(temperature: float) -> float:
    t = float(temperature)
    if not math.isfinite(t) or t <= 0.0:
        raise ValueError(f"temperature must be finite and > 0, got {temperature}")
    return t


def _features(features: Tensor, in_dim: int) -> Tensor:
    if not isinstance(features, Tensor):
        raise TypeError(f"features must be a torch.Tensor, got {type(features)}")
    if features.ndim < 1 or features.shape[-1] != in_dim:
        raise ValueError(f"features must be (..., {in_dim}) (fea_up's input width), got {tuple(features.shape)}")
    return features.detach()


def _launch(x2: Tensor, w, q: Tensor, num_pos: int, tau: float, want_sims: bool, want_rel: bool):
    """One gg_clip_query over rows x2 (R, D) with the unit rows q (Q, C) on the device, the first num_pos positive."""
    w1, b1, w2, b2 = w
    rows, dev = x2.shape[0], x2.device
    lib = _lib.load()
    nq, out_dim = q.shape
    sims = torch.empty(rows, nq, dtype=torch.float32, device=dev) if want_sims else None
    rel = torch.empty(rows, num_pos, dtype=torch.float32, device=dev) if want_rel else None
    ws = torch.empty(lib.gg_clip_query_workspace(x2.shape[1], HIDDEN, out_dim, nq), dtype=torch.uint8, device=dev)
    _lib.check(lib.gg_clip_query(rows, x2.shape[1], HIDDEN, out_dim, _ptr(x2), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2),
                                 nq, num_pos, _ptr(q), tau, _ptr(sims), _ptr(rel), _ptr(ws), ws.numel(), _stream(dev)),
               "gg_clip_query")
    return sims, rel


def _query(features: Tensor, fea_up, positives, negatives, temperature: float, want_sims: bool, want_rel: bool):
    """(similarities (..., P + N) or None, relevancy (..., P) or None); positives first, then negatives."""
    w = _weights(fea_up)
    in_dim, out_dim = w[0].shape[1], w[2].shape[0]
    x = _features(features, in_dim)
    pos = _unit_rows(positives, out_dim, "positives")
    neg = _unit_rows(negatives, out_dim, "negatives")
    tau = _check_temperature(temperature)
    if pos.shape[0] == 0:
        raise ValueError("no query embedding given")
    if want_rel and neg.shape[0] == 0:
        raise ValueError("relevancy needs at least one negative (canonical phrases such as 'object', 'things', "
                         "'stuff', 'texture'); use clip_similarity for plain cosine similarities")
    if neg.shape[0] > MAX_QUERIES - 1:
        raise ValueError(f"at most {MAX_QUERIES - 1} negatives (GG_QUERY_MAX = {MAX_QUERIES} query rows per launch, "
                         f"one of them a positive), got {neg.shape[0]}")
    dev = _require_hip(x)
    lead = x.shape[:-1]
    x2 = x.reshape(-1, in_dim)
    if x2.dtype != torch.float32:
        x2 = x2.float()
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.contiguous() if not x2.is_contiguous() else x2.clone()
    w = tuple(t.to(dev).contiguous() for t in w)
    pos, neg = pos.to(dev), neg.to(dev)
    limit = _max_queries(out_dim) if in_dim in KERNEL_IN else 0
    with torch.no_grad():
        if limit <= neg.shape[0]:            # the documented fallback: fea_up materialised, then torch
            y = F.normalize(mlp_forward(x2, *w), dim=-1)
            s = y @ torch.cat((pos, neg)).T
            P = pos.shape[0]
            r = None
            if want_rel:
                m = s[:, P:].max(dim=1, keepdim=True).values
                r = 1.0 / (1.0 + torch.exp(tau * (m - s[:, :P])))
            sims = s if want_sims else None
        else:
            step = limit - neg.shape[0]
            s_parts, r_parts, s_neg = [], [], None
            for p0 in range(0, pos.shape[0], step):
                pc = pos[p0:p0 + step]
                q = torch.cat((pc, neg)).contiguous()
                s, r = _launch(x2, w, q, pc.shape[0], tau, want_sims, want_rel and neg.shape[0] > 0)
                if want_sims:
                    s_parts.append(s[:, :pc.shape[0]])
                    if s_neg is None:
                        s_neg = s[:, pc.shape[0]:]
                if r is not None:
                    r_parts.append(r)
            sims = torch.cat(s_parts + [s_neg], dim=1) if want_sims else None
            r = (r_parts[0] if len(r_parts) == 1 else torch.cat(r_parts, dim=1)) if want_rel else None
    sims = None if sims is None else sims.reshape(lead + (sims.shape[1],))
    r = None if r is None else r.reshape(lead + (r.shape[1],))
    return sims, r


def clip_similarity(features: Tensor, fea_up, queries: ArrayLike) -> Tensor:
    """F.normalize(fea_up(features), dim=-1) @ unit(queries).T without materialising fea_up's output:
    features (..., D) on the HIP device, queries (Q, C) -> (..., Q) float32."""
    return _query(features, fea_up, queries, None, DEFAULT_TEMPERATURE, True, False)[0]


def relevancy(features: Tensor, fea_up, positives: ArrayLike, negatives: ArrayLike,
              temperature: float = DEFAULT_TEMPERATURE) -> Tensor:
    """LERF relevancy of every row against each positive: min over the negatives of softmax(tau [s_p, s_n])[0].
    features (..., D), positives (P, C), negatives (N >= 1, C) -> (..., P) float32."""
    return _query(features, fea_up, positives, negatives, temperature, False, True)[1]


def relevancy_view(model, camera, positives: ArrayLike, negatives: ArrayLike,
                   temperature: float = DEFAULT_TEMPERATURE, similarity: bool = False) -> dict:
    """Render `camera` through the model's own get_outputs (the plugin's fused model) under no_grad in eval mode,
    restore model.training, and query the feature image: {"relevancy": (H, W, P)} and, with similarity=True,
    {"similarity": (H, W, P + N)} (positives first)."""
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            out = model.get_outputs(camera)
    finally:
        model.train(was)
    if "feature" not in out:
        raise ValueError("the model rendered nothing (no 'feature' output) for this camera")
    sims, rel = _query(out["feature"], model.fea_up, positives, negatives, temperature, similarity, True)
    res = {"relevancy": rel}
    if similarity:
        res["similarity"] = sims
    return res


def _gaussian_features(model_or_scene) -> Tensor:
    feat = getattr(model_or_scene, "feature", None)
    if not isinstance(feat, Tensor) or feat.ndim != 2:
        raise ValueError("expected a model or scene with a (N, D) `feature` tensor")
    return feat.detach()


def relevancy_gaussians(model_or_scene, fea_up, positives: ArrayLike, negatives: ArrayLike,
                        temperature: float = DEFAULT_TEMPERATURE) -> Tensor:
    """(N, P) relevancy of every Gaussian's own feature (fea_up None: the model's)."""
    fea_up = getattr(model_or_scene, "fea_up", None) if fea_up is None else fea_up
    return relevancy(_gaussian_features(model_or_scene), fea_up, positives, negatives, temperature)


def select_gaussians(model_or_scene, fea_up, positives: ArrayLike, negatives: ArrayLike, threshold: float,
                     temperature: float = DEFAULT_TEMPERATURE) -> Tensor:
    """Semantic selection: (N,) bool, True where the relevancy to any positive exceeds `threshold`."""
    return (relevancy_gaussians(model_or_scene, fea_up, positives, negatives, temperature) > float(threshold)).any(dim=-1)


@torch.no_grad()
def lift_relevancy(model_or_scene, fea_up, cameras, positives: ArrayLike, negatives: ArrayLike, threshold: float,
                   temperature: float = DEFAULT_TEMPERATURE):
    """lift.Votes with two labels over `cameras` (as mesh.mesh_model takes them): per camera the feature image is
    rendered (lift.project_view, ops.rasterize_segments with a second segment of ones for the alpha sum), a pixel is
    labelled 1 where any positive's relevancy exceeds `threshold` and the alpha sum is >= mesh.ALPHA_MIN, 0
    otherwise, and the labels are lifted through the same view's tile lists (ops.blend_votes)."""
    from . import lift, ops
    from .mesh import ALPHA_MIN
    fea_up = getattr(model_or_scene, "fea_up", None) if fea_up is None else fea_up
    feat = _gaussian_features(model_or_scene)
    dev = _require_hip(feat)
    feat = feat.float().contiguous()
    n = feat.shape[0]
    votes = torch.zeros(n, 2, dtype=torch.int64, device=dev)
    counts = np.zeros(2, np.int64)
    ones = torch.ones(n, 1, device=dev)
    views = 0
    for c2w, K, h, w in cameras:
        h, w = int(h), int(w)
        views += 1
        if n == 0:
            continue
        proj = lift.project_view(model_or_scene, c2w, K, h, w)
        img, alpha = ops.rasterize_segments(*proj, h, w, [(feat, torch.zeros(feat.shape[1], device=dev)),
                                                           (ones, torch.zeros(1, device=dev))])
        rel = relevancy(img, fea_up, positives, negatives, temperature)
        lab = ((rel > float(threshold)).any(dim=-1) & (alpha[..., 0] >= ALPHA_MIN)).to(torch.uint8)
        ones_px = int(lab.sum())
        counts += np.asarray([h * w - ones_px, ones_px], np.int64)
        ops.blend_votes(*proj, h, w, lab, votes)
    return lift.Votes(votes, views, counts)


def select_gaussians_in_views(model_or_scene, fea_up, cameras, positives: ArrayLike, negatives: ArrayLike,
                              threshold: float, min_ratio: float = 0.5,
                              temperature: float = DEFAULT_TEMPERATURE) -> Tensor:
    """Semantic selection made where the features were supervised — in rendered pixels — and lifted onto the
    Gaussians: (N,) bool, True where label 1 of lift_relevancy holds at least `min_ratio` of the Gaussian's blend
    weight over `cameras`.  select_gaussians thresholds each Gaussian's own feature instead."""
    from . import lift
    res = lift_relevancy(model_or_scene, fea_up, cameras, positives, negatives, threshold, temperature)
    return lift.select(res.votes, 1, min_ratio)


# ------------------------------------------------------------------------------------------------
# command line: score every Gaussian of a checkpoint
# ------------------------------------------------------------------------------------------------
def score_checkpoint(ckpt: str, positives: np.ndarray, negatives: Optional[np.ndarray],
                     temperature: float = DEFAULT_TEMPERATURE, device: str = "cuda") -> np.ndarray:
    """(N, P) float32: relevancy with negatives, cosine similarity without, of every Gaussian's feature through the
    checkpoint's fea_up."""
    from .interop import fea_up_weights, load_checkpoint
    scene, mlp_state, _ = load_checkpoint(ckpt)
    w = fea_up_weights(mlp_state, device, ckpt, "(_model.fea_up.layers.{0,2}.{weight,bias})")
    feat = scene.feature.to(device)
    if negatives is None or len(negatives) == 0:
        out = clip_similarity(feat, w, positives)
    else:
        out = relevancy(feat, w, positives, negatives, temperature)
    return out.cpu().numpy().astype(np.float32)


def load_embeddings(path: str, name: str) -> np.ndarray:
    """(K, C) float32 text embeddings of a .npy file (one embedding may be 1-D)."""
    e = np.asarray(np.load(path), dtype=np.float32)
    if e.ndim == 1:
        e = e[None]
    if e.ndim != 2 or e.shape[0] == 0:
        raise ValueError(f"{name} {path}: expected (K, C) embeddings, got {e.shape}")
    return e


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.query",
                                 description="Score every Gaussian of a checkpoint against text embeddings: LERF "
                                             "relevancy with --negatives, cosine similarity without.")
    ap.add_argument("--ckpt", required=True, help="step-*.ckpt with _model.feature and _model.fea_up")
    ap.add_argument("--positives", required=True, help=".npy (P, C) or (C,) text embeddings")
    ap.add_argument("--negatives", default=None, help=".npy (N, C) canonical negatives")
    ap.add_argument("--temperature", type=float, default=DEFAULT_TEMPERATURE)
    ap.add_argument("--threshold", type=float, default=None, help="print how many Gaussians score above it")
    ap.add_argument("--out", required=True, help="output .npy, (N, P) float32")
    a = ap.parse_args(argv)
    try:
        _check_temperature(a.temperature)
        if a.threshold is not None and not math.isfinite(a.threshold):
            raise ValueError(f"threshold must be finite, got {a.threshold}")
        pos = load_embeddings(a.positives, "positives")
        neg = load_embeddings(a.negatives, "negatives") if a.negatives else None
        scores = score_checkpoint(a.ckpt, pos, neg, a.temperature)
    except (KeyError, ValueError, OSError) as exc:
        raise SystemExit(f"error: {exc}") from exc
    np.save(a.out, scores)
    msg = f"scored {scores.shape[0]} Gaussians against {scores.shape[1]} positive(s); wrote {a.out}"
    if a.threshold is not None:
        msg += f"; {int((scores > a.threshold).any(axis=1).sum())} above {a.threshold:g}"
    print(msg)
    return 0


if __name__ == "__main__":
    sys.exit(main())
