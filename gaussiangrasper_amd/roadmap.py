"""Arm roadmap: a probabilistic roadmap (Kavraki et al. 1996) between joint configurations over the Gaussian field.
Who is near whom in a weighted joint metric (`gg_roadmap_neighbours`), exact cost-to-go over the checked graph for many
goal sets at once (`gg_roadmap_route`) and the walk down it (`gg_roadmap_descend`), csrc/roadmap.hip; the edges are
tested by `arm.motion`, whose verdict covers every point of the move.  The contract is in include/gg_raster.h and
PARITY.md "Arm roadmap"; the design in DESIGN.md §3.34.

    neighbours         the k nearest nodes of every query, ties by the lowest index (no CPU path)
    default_metric     metres of sphere travel per unit of each joint: the row maxima of arm.reach_table
    metric_d2          the squared metric distance on the host, in the header's operation order
    edge_weights       the one quantisation law: max(1, ceil(sqrt(d2) / unit))
    candidate_pairs    every unordered pair of the neighbour lists once, as a < b
    assemble           the symmetric CSR of the checked edges, rows sorted by target
    build              sample, drop nodes that are not clear, find neighbours, test every candidate edge once -> Roadmap
    Roadmap            nodes, valid, the CSR, the tested edges with their Motion, the parameters; add / save / load
    route / descend    cost-to-go (Q, N) for Q goal sets; node paths down it (no CPU path)
    shortcut_pairs / shortcut_select / shortcut   greedy string pulling in joint space, gg_field_shortcut's rule
    plan               from every q_from to every q_to through the roadmap -> Plan
    python -m gaussiangrasper_amd.roadmap build --arm {default,FILE.json} --field field.npz --out roadmap.npz ...
    python -m gaussiangrasper_amd.roadmap plan  --arm ... --field ... --from A.npy --to B.npy --out way.npz ...
                                                [--time-limits {default,FILE.json}]

When the arm is where along a route, inside joint velocity and acceleration limits, is trajectory.py's.  Out of scope:
lazy edge evaluation, roadmap repair after the scene changes, torque limits and jerk."""
from __future__ import annotations

import argparse
import copy
import ctypes as C
import math
import sys
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._call import (ArrayLike, check_finite_options, default_device, host_array, host_ptr, positive, ptr as _ptr,
                    require_hip as _require_hip, sized_workspace, stream as _stream, to_device)
from . import arm as _arm
from .arm import MAX_JOINTS, MAX_SAMPLES, SPHERE_RADIUS, Arm, Motion
from .field import FAR, MAX_POSES

MAX_K = 32                     # GG_ROADMAP_MAX_K
MAX_NODES = 65536              # GG_ROADMAP_MAX_NODES
TILE = 256                     # GG_ROADMAP_TILE
MAX_EDGES = 1 << 27
# This project's choices (PARITY.md "Arm roadmap"); none has been measured on a robot
NUM_NODES = 4096
K = 16
UNIT = 1e-3                    # metres of the metric per unit of weight
MAX_WEIGHT = ((1 << 30) - 1) // MAX_NODES      # N max_weight < 2^30 for every N the entries take: 16.383 m at UNIT
MOTION_KEYS = ("samples", "slack", "slack_at", "worst", "gap", "gap_at", "pair", "ok")


# ------------------------------------------------------------------------------------------------
# the calls as they are
# ------------------------------------------------------------------------------------------------
def _metric(metric: ArrayLike, J: int) -> np.ndarray:
    m = np.ascontiguousarray(host_array(metric, np.float64).reshape(-1))
    if m.shape != (J,) or not (np.isfinite(m).all() and (m >= 0).all()):
        raise ValueError(f"metric must be ({J},) finite numbers >= 0, got {m.shape}")
    return m


def neighbours(nodes: ArrayLike, k: int, metric: ArrayLike, queries: Optional[ArrayLike] = None,
               skip: Optional[ArrayLike] = None, valid: Optional[ArrayLike] = None) -> Tuple[Tensor, Tensor]:
    """(idx (M, k) int32, d2 (M, k) float64) of one gg_roadmap_neighbours call, on the HIP device (no CPU path).
    nodes (N, J) and queries (M, J) float64; queries None: the nodes against themselves, each skipping itself.  skip
    (M,) a node index the query must not return, or -1; valid (N,) 0 / 1."""
    dev = nodes.device if isinstance(nodes, Tensor) and nodes.device.type == "cuda" else default_device("roadmap")
    n = to_device(nodes, torch.float64, dev)
    if n.ndim != 2 or not 1 <= n.shape[1] <= MAX_JOINTS:
        raise ValueError(f"nodes must be (N, J) with J in 1..{MAX_JOINTS}, got {tuple(n.shape)}")
    N, J = n.shape
    if N > MAX_NODES:
        raise ValueError(f"{N} nodes are more than {MAX_NODES}")
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must be in 1..{MAX_K}, got {k}")
    m = _metric(metric, J)
    if queries is None:
        q = n
        if skip is None:
            skip = torch.arange(N, dtype=torch.int32, device=dev)
    else:
        q = to_device(queries, torch.float64, dev)
        if q.ndim != 2 or q.shape[1] != J:
            raise ValueError(f"queries must be (M, {J}), got {tuple(q.shape)}")
    M = q.shape[0]
    if M > MAX_POSES:
        raise ValueError(f"{M} queries are more than {MAX_POSES}")
    s = None if skip is None else to_device(skip, torch.int32, dev).reshape(-1)
    if s is not None and s.shape[0] != M:
        raise ValueError(f"skip must be ({M},), got {tuple(s.shape)}")
    v = None if valid is None else to_device(valid, torch.uint8, dev).reshape(-1)
    if v is not None and v.shape[0] != N:
        raise ValueError(f"valid must be ({N},), got {tuple(v.shape)}")
    idx = torch.empty(M, int(k), dtype=torch.int32, device=dev)
    d2 = torch.empty(M, int(k), dtype=torch.float64, device=dev)
    _lib.check(_lib.load().gg_roadmap_neighbours(J, N, _ptr(n), M, _ptr(q), host_ptr(m), _ptr(s), _ptr(v), int(k),
                                                 _ptr(idx), _ptr(d2), _stream(dev)), "gg_roadmap_neighbours")
    return idx, d2


def _csr(offsets, targets, weights, dev):
    o = to_device(offsets, torch.int32, dev).reshape(-1)
    t = to_device(targets, torch.int32, dev).reshape(-1)
    w = to_device(weights, torch.int32, dev).reshape(-1)
    if o.shape[0] < 1 or t.shape[0] != w.shape[0] or t.shape[0] > MAX_EDGES:
        raise ValueError(f"a CSR graph is offsets (N + 1,), targets (E,) and weights (E,) with E <= {MAX_EDGES}")
    return o, t, w


def route_csr(offsets: ArrayLike, targets: ArrayLike, weights: ArrayLike, max_weight: int, goals: Sequence,
              max_rounds: Optional[int] = None, device=None) -> Tuple[Tensor, int, int]:
    """(cost (Q, N) int32 on the device, ignored, rounds) of one gg_roadmap_route call (no CPU path).  goals: a
    sequence of Q sequences of node indices.  max_rounds None: N + 1, which always suffices (a shortest walk has at
    most N - 1 edges).  GGError when the rounds run out.  The call synchronises the stream."""
    dev = default_device("roadmap") if device is None else torch.device(device)
    o, t, w = _csr(offsets, targets, weights, dev)
    N = o.shape[0] - 1
    sets = [np.asarray(g, np.int64).reshape(-1) for g in goals]
    Q = len(sets)
    go = np.zeros(Q + 1, np.int32)
    go[1:] = np.cumsum([len(g) for g in sets])
    flat = np.concatenate(sets).astype(np.int32) if Q else np.zeros(0, np.int32)
    gt = to_device(flat, torch.int32, dev)
    lib = _lib.load()
    ws = sized_workspace(lib.gg_roadmap_route_workspace(N, Q), f"{N} nodes x {Q} queries are out of range", dev)
    cost = torch.empty(Q, N, dtype=torch.int32, device=dev)
    ignored = torch.zeros(1, dtype=torch.int64, device=dev)
    rounds = C.c_int(0)
    _lib.check(lib.gg_roadmap_route(N, t.shape[0], _ptr(o), _ptr(t), _ptr(w), int(max_weight), Q, host_ptr(go),
                                    _ptr(gt), _ptr(cost), _ptr(ignored), int(N + 1 if max_rounds is None else max_rounds),
                                    C.byref(rounds), _ptr(ws), ws.numel(), _stream(dev)), "gg_roadmap_route")
    return cost, int(ignored.item()), rounds.value


def descend_csr(offsets: ArrayLike, targets: ArrayLike, weights: ArrayLike, max_weight: int, cost: Tensor,
                query: ArrayLike, starts: ArrayLike, max_nodes: int) -> Tuple[Tensor, Tensor]:
    """(path (P, max_nodes) int32, length (P,) int32) of one gg_roadmap_descend call (no CPU path)."""
    dev = _require_hip(cost)
    o, t, w = _csr(offsets, targets, weights, dev)
    N = o.shape[0] - 1
    if cost.dtype != torch.int32 or cost.ndim != 2 or cost.shape[1] != N:
        raise ValueError(f"cost must be an int32 (Q, {N}) tensor, got {cost.dtype} {tuple(cost.shape)}")
    cost = cost.contiguous()
    qt = to_device(query, torch.int32, dev).reshape(-1)
    st = to_device(starts, torch.int32, dev).reshape(-1)
    P = qt.shape[0]
    if st.shape[0] != P:
        raise ValueError(f"query and starts must have as many entries, got {P} and {st.shape[0]}")
    if int(max_nodes) < 1 or P * int(max_nodes) > MAX_POSES:
        raise ValueError(f"need max_nodes >= 1 and P max_nodes <= {MAX_POSES}, got {P} x {max_nodes}")
    path = torch.empty(P, int(max_nodes), dtype=torch.int32, device=dev)
    length = torch.empty(P, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().gg_roadmap_descend(N, t.shape[0], _ptr(o), _ptr(t), _ptr(w), int(max_weight), cost.shape[0],
                                              _ptr(cost), P, _ptr(qt), _ptr(st), int(max_nodes), _ptr(path),
                                              _ptr(length), _stream(dev)), "gg_roadmap_descend")
    return path, length


# ------------------------------------------------------------------------------------------------
# host side: the metric, the quantisation law, the graph
# ------------------------------------------------------------------------------------------------
def default_metric(arm: Arm, spheres: Optional[ArrayLike] = None,
                   radius: Union[float, ArrayLike] = SPHERE_RADIUS) -> np.ndarray:
    """(J,) float64: metric[j] = max_s reach_table[j][s] over the spheres arm.motion would test (the link spheres, then
    the gripper-frame `spheres`): metres of sphere travel per unit of joint j at most.  With it an edge of metric
    length L = sqrt(d2) has gg_arm_motion's sweep bound B <= sqrt(J) L, so at most
    ceil(sqrt(J) L / res) samples."""
    c, f, _ = _arm._self_set(arm, spheres, radius)
    table = _arm.reach_table(arm, c, f)
    return table.max(1) if table.shape[1] else np.zeros(arm.num_joints)


def metric_d2(qa: ArrayLike, qb: ArrayLike, metric: ArrayLike) -> np.ndarray:
    """d2 of the rows of qa against the rows of qb as the header states it: fp64, every operation rounded, j
    ascending.  numpy keeps the order, so this is the device's value to the bit."""
    a, b = np.asarray(qa, np.float64), np.asarray(qb, np.float64)
    m = np.asarray(metric, np.float64)
    e = m[0] * (a[..., 0] - b[..., 0])
    d = e * e
    for j in range(1, a.shape[-1]):
        e = m[j] * (a[..., j] - b[..., j])
        d = d + e * e
    return d


def edge_weights(d2: ArrayLike, unit: float = UNIT) -> np.ndarray:
    """int64 w = max(1, ceil(sqrt(d2) / unit)) in fp64: IEEE sqrt, then the division, then ceil.  The one quantisation
    law.  A d2 that is not finite gives the largest int64 (never a usable weight)."""
    unit = positive("unit", unit)
    d = np.asarray(d2, np.float64)
    with np.errstate(invalid="ignore"):
        x = np.ceil(np.sqrt(d) / unit)
    fits = np.isfinite(x) & (x < 2.0 ** 62)
    w = np.maximum(np.where(fits, x, 1.0), 1.0).astype(np.int64)
    return np.where(fits, w, np.iinfo(np.int64).max)


def candidate_pairs(sources: ArrayLike, idx: ArrayLike, num_nodes: int) -> Tuple[np.ndarray, np.ndarray]:
    """(a, b) int64 with a < b: every unordered pair {sources[m], idx[m][r]} with idx >= 0 once, ascending in (a, b).
    The union of both nodes' neighbour lists: a pair that either end lists is there."""
    idx = np.asarray(idx, np.int64)
    src = np.broadcast_to(np.asarray(sources, np.int64).reshape(-1, 1), idx.shape)
    keep = (idx >= 0) & (idx != src)
    lo, hi = np.minimum(src[keep], idx[keep]), np.maximum(src[keep], idx[keep])
    key = np.unique(lo * int(num_nodes) + hi)
    return key // int(num_nodes), key % int(num_nodes)


def assemble(num_nodes: int, a: ArrayLike, b: ArrayLike, ok: ArrayLike, w: ArrayLike):
    """(offsets (N + 1,), targets (E,), weights (E,)) int32: the symmetric CSR of the undirected edges {a, b} with ok,
    both directions stored, rows sorted by target.  A pair given twice (in either order) is taken once, its first
    occurrence; a == b is dropped."""
    N = int(num_nodes)
    a, b = np.asarray(a, np.int64).reshape(-1), np.asarray(b, np.int64).reshape(-1)
    ok, w = np.asarray(ok, bool).reshape(-1), np.asarray(w, np.int64).reshape(-1)
    if len(a) and (min(a.min(), b.min()) < 0 or max(a.max(), b.max()) >= N):
        raise ValueError("an edge names a node outside 0..num_nodes - 1")
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    _, first = np.unique(lo * N + hi, return_index=True)
    first = first[ok[first] & (lo[first] != hi[first])]
    lo, hi, w = lo[first], hi[first], w[first]
    if len(w) and (w.min() < 1 or w.max() > np.iinfo(np.int32).max):
        raise ValueError("a kept edge has a weight outside 1..2^31 - 1")
    src, dst, ww = np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([w, w])
    order = np.lexsort((dst, src))
    offsets = np.zeros(N + 1, np.int64)
    np.add.at(offsets, src + 1, 1)
    return (np.cumsum(offsets).astype(np.int32), dst[order].astype(np.int32), ww[order].astype(np.int32))


# ------------------------------------------------------------------------------------------------
# the roadmap
# ------------------------------------------------------------------------------------------------
@dataclass
class Roadmap:
    nodes: np.ndarray          # (N, J) float64
    valid: np.ndarray          # (N,) uint8: the configuration is clear itself; a row that is not stays, without edges
    offsets: np.ndarray        # (N + 1,) int32   the symmetric CSR of the edges that are ok and within max_weight
    targets: np.ndarray        # (E,) int32
    weights: np.ndarray        # (E,) int32
    metric: np.ndarray         # (J,) float64
    unit: float
    max_weight: int
    k: int
    edge_a: np.ndarray         # (T,) int64  the tested edges, each once, as the move from the lower index ...
    edge_b: np.ndarray         # (T,) int64  ... to the higher
    edge_d2: np.ndarray        # (T,) float64
    edge_w: np.ndarray         # (T,) int64  edge_weights(edge_d2, unit)
    motion: Motion             # of the tested edges, (T,)
    params: dict               # what the verdicts depend on: res, margin, self_margin, spheres, radius, pairs, outside,
                               # max_samples
    dropped: int = 0           # tested edges that are ok and heavier than max_weight
    arm: Optional[Arm] = None          # not saved: build and attach set them, add and plan use them
    field: object = None

    @property
    def num_nodes(self) -> int:
        return len(self.nodes)

    def attach(self, arm: Arm, field) -> "Roadmap":
        self.arm, self.field = arm, field
        return self

    def copy(self) -> "Roadmap":
        """own arrays, the same arm and field"""
        out = copy.copy(self)
        for name in ("nodes", "valid", "offsets", "targets", "weights", "metric", "edge_a", "edge_b", "edge_d2", "edge_w"):
            setattr(out, name, getattr(self, name).copy())
        out.params = dict(self.params)
        return out

    def motion_kw(self) -> dict:
        p = self.params
        return dict(spheres=p["spheres"], radius=p["radius"], margin=p["margin"], self_margin=p["self_margin"],
                    res=p["res"], max_samples=p["max_samples"], pairs=p["pairs"], outside=p["outside"])

    def _rebuild(self) -> None:
        ok = self.motion.ok.cpu().numpy() & (self.edge_w <= self.max_weight)
        self.dropped = int((self.motion.ok.cpu().numpy() & (self.edge_w > self.max_weight)).sum())
        self.offsets, self.targets, self.weights = assemble(len(self.nodes), self.edge_a, self.edge_b, ok, self.edge_w)

    def add(self, q: ArrayLike, force: Optional[Tuple[ArrayLike, ArrayLike]] = None, arm: Optional[Arm] = None,
            field=None) -> np.ndarray:
        """Adds the configurations q (R, J) and returns their indices N .. N + R - 1.  Each is tested itself (a
        zero-length motion), then offered its k nearest old nodes (one neighbours call, the queries apart from the
        nodes) and its nearest new ones; `force` = (a, b) further pairs of node indices, old or new, to test.  The new
        edges are tested in one motion call and appended; the edges among the old nodes stay as they are."""
        arm = self.arm if arm is None else arm
        field = self.field if field is None else field
        if arm is None:
            raise ValueError("the roadmap has no arm: attach(arm, field) after load")
        J = self.nodes.shape[1]
        q = host_array(q, np.float64).reshape(-1, J)
        N, R = len(self.nodes), len(q)
        if N + R > MAX_NODES:
            raise ValueError(f"{N + R} nodes are more than {MAX_NODES}")
        new = np.arange(N, N + R)
        if R == 0:
            return new
        dev = default_device("roadmap") if field is None else field.dist2.device
        kw = self.motion_kw()
        qt = to_device(q, torch.float64, dev)
        v_new = _arm.motion(arm, qt, qt, field, **kw).ok.cpu().numpy().astype(np.uint8)
        parts = []
        if N:
            idx, _ = neighbours(to_device(self.nodes, torch.float64, dev), min(self.k, MAX_K), self.metric, queries=qt,
                                valid=self.valid)
            idx = idx.cpu().numpy()
            idx[v_new == 0] = -1
            parts.append(candidate_pairs(new, idx, N + R))
        if R > 1:
            idx, _ = neighbours(qt, min(self.k, MAX_K), self.metric, valid=v_new)
            idx = idx.cpu().numpy().astype(np.int64)
            idx = np.where(idx >= 0, idx + N, -1)
            idx[v_new == 0] = -1
            parts.append(candidate_pairs(new, idx, N + R))
        nodes = np.concatenate([self.nodes, q])
        valid = np.concatenate([self.valid, v_new])
        if force is not None:
            fa, fb = (np.asarray(x, np.int64).reshape(-1) for x in force)
            keep = (valid[fa] != 0) & (valid[fb] != 0) & (fa != fb)
            parts.append((np.minimum(fa, fb)[keep], np.maximum(fa, fb)[keep]))
        a = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, np.int64)
        b = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, np.int64)
        key = np.setdiff1d(np.unique(a * (N + R) + b), self.edge_a * (N + R) + self.edge_b)
        a, b = key // (N + R), key % (N + R)
        m = _arm.motion(arm, to_device(nodes[a], torch.float64, dev), to_device(nodes[b], torch.float64, dev), field, **kw)
        d2 = metric_d2(nodes[a], nodes[b], self.metric)
        self.nodes, self.valid = nodes, valid
        self.edge_a, self.edge_b = np.concatenate([self.edge_a, a]), np.concatenate([self.edge_b, b])
        self.edge_d2 = np.concatenate([self.edge_d2, d2])
        self.edge_w = np.concatenate([self.edge_w, edge_weights(d2, self.unit)])
        self.motion = _cat_motion(self.motion, m)
        self._rebuild()
        return new

    def save(self, path: str) -> None:
        p = self.params
        np.savez_compressed(
            path, nodes=self.nodes, valid=self.valid, offsets=self.offsets, targets=self.targets, weights=self.weights,
            metric=self.metric, unit=np.float64(self.unit), max_weight=np.int64(self.max_weight), k=np.int64(self.k),
            edge_a=self.edge_a, edge_b=self.edge_b, edge_d2=self.edge_d2, edge_w=self.edge_w,
            dropped=np.int64(self.dropped), res=np.float64(p["res"]), margin=np.float64(p["margin"]),
            self_margin=np.float64(p["self_margin"]), max_samples=np.int64(p["max_samples"]),
            spheres=np.zeros((0, 3), np.float32) if p["spheres"] is None else np.asarray(p["spheres"], np.float32),
            has_spheres=np.bool_(p["spheres"] is not None), radius=np.asarray(p["radius"], np.float64),
            pairs=np.zeros((0, 0), np.uint8) if p["pairs"] is None or p["pairs"] is False else np.asarray(p["pairs"], np.uint8),
            pairs_kind=np.int64(0 if p["pairs"] is None else 1 if p["pairs"] is False else 2),
            outside=np.str_(p["outside"]),
            **{f"motion_{k}": getattr(self.motion, k).cpu().numpy() for k in MOTION_KEYS})

    @classmethod
    def load(cls, path: str) -> "Roadmap":
        """The roadmap of `save`; its Motion sits on the host.  ValueError naming the file when a field is missing."""
        try:
            with np.load(path) as z:
                kind = int(z["pairs_kind"])
                params = dict(res=float(z["res"]), margin=float(z["margin"]), self_margin=float(z["self_margin"]),
                              max_samples=int(z["max_samples"]), spheres=z["spheres"] if bool(z["has_spheres"]) else None,
                              radius=float(z["radius"]) if z["radius"].ndim == 0 else z["radius"],
                              pairs=None if kind == 0 else False if kind == 1 else z["pairs"], outside=str(z["outside"]))
                motion = Motion(**{k: torch.from_numpy(z[f"motion_{k}"]) for k in MOTION_KEYS}, res=params["res"],
                                self_margin=params["self_margin"])
                return cls(z["nodes"], z["valid"], z["offsets"], z["targets"], z["weights"], z["metric"], float(z["unit"]),
                           int(z["max_weight"]), int(z["k"]), z["edge_a"], z["edge_b"], z["edge_d2"], z["edge_w"], motion,
                           params, int(z["dropped"]))
        except KeyError as exc:
            raise ValueError(f"{path}: not a roadmap: {exc.args[0]}") from exc


def _cat_motion(a: Motion, b: Motion) -> Motion:
    return Motion(**{k: torch.cat([getattr(a, k).to(getattr(b, k).device), getattr(b, k)]) for k in MOTION_KEYS},
                  res=b.res, self_margin=b.self_margin)


def sample_nodes(arm: Arm, num_nodes: int, seed: int = 0) -> np.ndarray:
    """(num_nodes, J): the home configuration, then uniform within the limits from np.random.default_rng(seed): the
    rule of arm.connect's via configurations."""
    n, J = max(int(num_nodes), 0), arm.num_joints
    v = np.empty((n, J))
    if n:
        v[0] = arm.home()
        v[1:] = np.random.default_rng(seed).uniform(np.asarray(arm.lo, np.float64), np.asarray(arm.hi, np.float64),
                                                    size=(n - 1, J))
    return v


def build(arm: Arm, field=None, num_nodes: int = NUM_NODES, k: int = K, seed: int = 0, nodes: Optional[ArrayLike] = None,
          terminals: Optional[ArrayLike] = None, metric: Optional[ArrayLike] = None, unit: float = UNIT,
          max_weight: int = MAX_WEIGHT, force: Optional[Tuple[ArrayLike, ArrayLike]] = None,
          spheres: Optional[ArrayLike] = None, radius: Union[float, ArrayLike] = SPHERE_RADIUS, margin: float = 0.0,
          self_margin: float = 0.0, res: Optional[float] = None, max_samples: int = MAX_SAMPLES, pairs=None,
          outside: str = "free") -> Roadmap:
    """A roadmap of the arm over `field` (a field.DistanceField after update(); None: self-collision only, give res).
    nodes None: sample_nodes(arm, num_nodes, seed); `terminals` are appended after them.  One zero-length motion call
    marks the nodes that are clear themselves (the others stay as rows with valid = 0), one neighbours call finds each
    valid node's k nearest valid nodes, one motion call tests every candidate edge once (from the lower index to the
    higher: the verdict covers every point of the segment, so it holds both ways), `assemble` builds the graph.
    force = (a, b): further pairs of node indices to test.  spheres .. outside: arm.motion's."""
    J = arm.num_joints
    v = sample_nodes(arm, num_nodes, seed) if nodes is None else host_array(nodes, np.float64).reshape(-1, J)
    if terminals is not None:
        v = np.concatenate([v, host_array(terminals, np.float64).reshape(-1, J)])
    N = len(v)
    if N > MAX_NODES:
        raise ValueError(f"{N} nodes are more than {MAX_NODES}")
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must be in 1..{MAX_K}, got {k}")
    if not 1 <= int(max_weight) or N * int(max_weight) >= 1 << 30:
        raise ValueError(f"need max_weight >= 1 and num_nodes max_weight < 2^30, got {N} x {max_weight}")
    unit = positive("unit", unit)
    dev = default_device("roadmap") if field is None else field.dist2.device
    if res is None:
        if field is None:
            raise ValueError("without a field, give res")
        res = field.h
    m = default_metric(arm, spheres, radius) if metric is None else _metric(metric, J)
    sp = None if spheres is None else host_array(spheres, np.float32).reshape(-1, 3).copy()
    params = dict(res=float(res), margin=float(margin), self_margin=float(self_margin), spheres=sp, radius=radius,
                  pairs=pairs if pairs is None or pairs is False else np.asarray(pairs, np.uint8), outside=outside,
                  max_samples=int(max_samples))
    empty = Motion(*(torch.zeros(0, dtype=t, device=dev) for t in (torch.int32,) * 4), torch.zeros(0, dtype=torch.float64, device=dev),
                   torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, 2, dtype=torch.int32, device=dev),
                   torch.zeros(0, dtype=torch.bool, device=dev), float(res), float(self_margin))
    zero = np.zeros(0, np.int64)
    rm = Roadmap(v[:0].copy(), np.zeros(0, np.uint8), np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32),
                 m, unit, int(max_weight), int(k), zero, zero.copy(), np.zeros(0), zero.copy(), empty, params, 0, arm, field)
    # a roadmap is its nodes added to an empty one: the new nodes try each other
    rm.add(v, force=force)
    return rm


def route(roadmap: Roadmap, goals: Sequence, max_rounds: Optional[int] = None) -> Tensor:
    """cost (Q, N) int32 on the device: the cost-to-go of every node to the goal set of each query, in units of
    roadmap.unit; FAR where there is no route.  goals: Q node indices, or Q sequences of them."""
    sets = [np.atleast_1d(np.asarray(g, np.int64)) for g in goals]
    dev = default_device("roadmap") if roadmap.field is None else roadmap.field.dist2.device
    return route_csr(roadmap.offsets, roadmap.targets, roadmap.weights, roadmap.max_weight, sets, max_rounds, dev)[0]


def descend(roadmap: Roadmap, cost: Tensor, query: ArrayLike, starts: ArrayLike,
            max_nodes: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """(path (P, max_nodes) int32 node indices, length (P,) int32) down `cost` from starts[p] for query[p].  max_nodes
    None: as many as fit, the number of nodes at most."""
    P = int(np.asarray(host_array(query)).size)
    if max_nodes is None:
        max_nodes = max(1, min(roadmap.num_nodes, MAX_POSES // max(P, 1)))
    return descend_csr(roadmap.offsets, roadmap.targets, roadmap.weights, roadmap.max_weight, cost, query, starts,
                       max_nodes)


# ------------------------------------------------------------------------------------------------
# string pulling in joint space
# ------------------------------------------------------------------------------------------------
def shortcut_pairs(lengths: ArrayLike, window: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(p, i, j) int64: every pair i < j <= i + window of every path p of lengths[p] waypoints, ascending in (p, i, j):
    the moves `shortcut` tests and `shortcut_select` reads, in this order."""
    if int(window) < 1:
        raise ValueError(f"window must be >= 1, got {window}")
    ps, is_, js = [], [], []
    for p, n in enumerate(np.asarray(lengths, np.int64).reshape(-1)):
        i = np.repeat(np.arange(n), int(window))
        j = i + np.tile(np.arange(1, int(window) + 1), n)
        keep = j < n
        ps.append(np.full(int(keep.sum()), p)), is_.append(i[keep]), js.append(j[keep])
    cat = (lambda x: np.concatenate(x).astype(np.int64)) if ps else (lambda x: np.zeros(0, np.int64))
    return cat(ps), cat(is_), cat(js)


def shortcut_select(lengths: ArrayLike, window: int, ok: ArrayLike) -> List[np.ndarray]:
    """The waypoints each path keeps, numpy: from the anchor i (0 first) the next anchor is the largest j in i + 1 ..
    min(i + window, n - 1) whose move i -> j is ok; i + 1 when there is none (the path's own move, taken as it is).
    ok: one verdict per row of shortcut_pairs(lengths, window)."""
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    p, i, j = shortcut_pairs(lengths, window)
    ok = np.asarray(ok, bool).reshape(-1)
    if ok.shape != p.shape:
        raise ValueError(f"ok must have one entry per pair: {p.shape[0]}, got {ok.shape[0]}")
    table = {(int(a), int(b), int(c)): bool(o) for a, b, c, o in zip(p, i, j, ok)}
    out = []
    for path, n in enumerate(lengths):
        keep, at = ([0] if n else []), 0
        while at < n - 1:
            nxt = at + 1
            for cand in range(min(at + int(window), n - 1), at + 1, -1):
                if table[(path, at, cand)]:
                    nxt = cand
                    break
            keep.append(nxt)
            at = nxt
        out.append(np.asarray(keep, np.int64))
    return out


def shortcut(roadmap_or_arm: Union[Roadmap, Arm], paths: Sequence[ArrayLike], window: int, field=None,
             **kw) -> List[np.ndarray]:
    """Greedy string pulling of joint-space paths ((n, J) waypoints each) by gg_field_shortcut's rule: every pair
    within the window of every path goes into ONE arm.motion call, `shortcut_select` chooses.  Given a Roadmap, its
    arm, field and motion parameters are used (a `field` given here replaces the roadmap's); given an Arm, **kw are
    arm.motion's."""
    if isinstance(roadmap_or_arm, Roadmap):
        arm, kw = roadmap_or_arm.arm, {**roadmap_or_arm.motion_kw(), **kw}
        field = roadmap_or_arm.field if field is None else field
        if arm is None:
            raise ValueError("the roadmap has no arm: attach(arm, field) after load")
    else:
        arm = roadmap_or_arm
    J = arm.num_joints
    ways = [host_array(w, np.float64).reshape(-1, J) for w in paths]
    p, i, j = shortcut_pairs([len(w) for w in ways], window)
    if len(p) == 0:
        return [w.copy() for w in ways]
    dev = default_device("roadmap") if field is None else field.dist2.device
    qa = np.stack([ways[a][b] for a, b in zip(p, i)])
    qb = np.stack([ways[a][b] for a, b in zip(p, j)])
    ok = _arm.motion(arm, to_device(qa, torch.float64, dev), to_device(qb, torch.float64, dev), field, **kw).ok
    keep = shortcut_select([len(w) for w in ways], window, ok.cpu().numpy())
    return [w[k] for w, k in zip(ways, keep)]


# ------------------------------------------------------------------------------------------------
# planning
# ------------------------------------------------------------------------------------------------
@dataclass
class Plan:
    routes: list               # [A][B]: None, or the (n, J) float64 numpy waypoints from q_from[a] to q_to[b]
    cost: np.ndarray           # (A, B) int64 the graph route's sum of weights, in units of roadmap.unit; -1 without one
    length: np.ndarray         # (A, B) float64 the returned waypoints' summed sqrt(d2) in the metric; inf without one
    hops: np.ndarray           # (A, B) int64 the returned waypoints' moves; -1 without a route
    nodes: list                # [A][B]: None, or the (n,) node indices of the graph route (before shortcutting)
    roadmap: Roadmap           # with the A + B terminals added: from a is node start + a, to b is node start + A + b
    start: int                 # the index of the first terminal


def path_length(way: np.ndarray, metric: ArrayLike) -> float:
    """the summed sqrt(d2) of a path's moves, added in order onto 0.0"""
    total = 0.0
    for d in np.sqrt(metric_d2(way[:-1], way[1:], metric)) if len(way) > 1 else ():
        total = total + float(d)
    return total


def plan(arm: Arm, q_from: ArrayLike, q_to: ArrayLike, field=None, roadmap: Optional[Roadmap] = None,
         shortcut_window: int = 0, **kw) -> Plan:
    """A clear joint-space route from every q_from (A, J) to every q_to ((B, J), or (J,) for B = 1) through a roadmap.
    The A + B terminals are added to a copy of `roadmap` (its arm, field and parameters hold; **kw must be empty), or a
    fresh one is built with them (**kw: build's).  Every (from, to) pair is forced into the candidate edges, so the
    direct move is an edge like any other.  One route call with the B goals as B queries, one descend from the A
    starts; shortcut_window > 0 then string-pulls the routes (`cost` stays the graph route's)."""
    J = arm.num_joints
    qa = host_array(q_from, np.float64).reshape(-1, J)
    qb = host_array(q_to, np.float64).reshape(-1, J)
    A, B = len(qa), len(qb)
    term = np.concatenate([qa, qb])
    if roadmap is None:
        if kw.get("terminals") is not None or kw.get("force") is not None:
            raise ValueError("plan appends its own terminals and forces its own pairs")
        base = kw.pop("nodes", None)
        base = sample_nodes(arm, kw.pop("num_nodes", NUM_NODES), kw.get("seed", 0)) if base is None else \
            host_array(base, np.float64).reshape(-1, J)
        n0 = len(base)
        fa = n0 + np.repeat(np.arange(A), B)
        fb = n0 + A + np.tile(np.arange(B), A)
        rm = build(arm, field, nodes=base, terminals=term, force=(fa, fb), **kw)
    else:
        if kw:
            raise ValueError(f"with a roadmap its own parameters hold; got {sorted(kw)}")
        rm = roadmap.copy()
        if rm.arm is None or field is not None:
            rm.attach(arm, roadmap.field if field is None else field)
        n0 = rm.num_nodes
        fa = n0 + np.repeat(np.arange(A), B)
        fb = n0 + A + np.tile(np.arange(B), A)
        rm.add(term, force=(fa, fb))
    routes = [[None] * B for _ in range(A)]
    ids = [[None] * B for _ in range(A)]
    cost = np.full((A, B), -1, np.int64)
    length = np.full((A, B), np.inf)
    hops = np.full((A, B), -1, np.int64)
    if A and B:
        c = route(rm, [[n0 + A + b] for b in range(B)])
        path, n = descend(rm, c, np.tile(np.arange(B), A), n0 + np.repeat(np.arange(A), B))
        path, n, ch = path.cpu().numpy(), n.cpu().numpy(), c.cpu().numpy()
        if (n > path.shape[1]).any():
            raise ValueError(f"a route has more than {path.shape[1]} nodes: plan fewer pairs at once")
        for a in range(A):
            for b in range(B):
                r = a * B + b
                if n[r] > 0:
                    ids[a][b] = path[r, :n[r]].astype(np.int64)
                    routes[a][b] = rm.nodes[ids[a][b]]
                    cost[a, b] = ch[b, n0 + a]
        found = [(a, b) for a in range(A) for b in range(B) if routes[a][b] is not None]
        if int(shortcut_window) > 0 and found:
            pulled = shortcut(rm, [routes[a][b] for a, b in found], shortcut_window)
            for (a, b), w in zip(found, pulled):
                routes[a][b] = w
        for a, b in found:
            length[a, b] = path_length(routes[a][b], rm.metric)
            hops[a, b] = len(routes[a][b]) - 1
    return Plan(routes, cost, length, hops, ids, rm, n0)


# ------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------
def _motion_options(ap) -> None:
    ap.add_argument("--arm", required=True, metavar="{default,FILE.json}", help="the arm model")
    ap.add_argument("--base", default=None, help=".npy (12,), (3, 4) or (4, 4): scene from arm base")
    ap.add_argument("--field", default=None, help=".npz of python -m gaussiangrasper_amd.field (--out)")
    ap.add_argument("--margin", type=float, default=0.0, help="clearance kept beyond the spheres")
    ap.add_argument("--self-margin", type=float, default=0.0, help="gap kept between the arm's own spheres")
    ap.add_argument("--motion-res", type=float, default=None,
                    help="no sphere centre moves further than this between two samples of a move (default: the "
                         "field's cell edge)")
    ap.add_argument("--max-samples", type=int, default=MAX_SAMPLES, help="samples per move at most")
    ap.add_argument("--spheres", default=None, help=".npy (S, 3) further sphere centres, gripper frame")
    ap.add_argument("--radius", type=float, default=SPHERE_RADIUS, help="radius of gripper-frame spheres (--spheres)")


def _build_options(ap) -> None:
    ap.add_argument("--nodes", type=int, default=NUM_NODES, help="sampled configurations, the home configuration first")
    ap.add_argument("--k", type=int, default=K, help="neighbours offered to every node")
    ap.add_argument("--seed", type=int, default=0, help="of the sampled configurations")
    ap.add_argument("--unit", type=float, default=UNIT, help="metres of the metric per unit of edge weight")


def _check_options(ap, a) -> None:
    check_finite_options(ap, a, positive=("radius",) + (("unit",) if hasattr(a, "unit") else ()),
                         nonneg=("margin", "self_margin"))
    if a.motion_res is not None and not (math.isfinite(a.motion_res) and a.motion_res > 0.0):
        ap.error(f"--motion-res must be finite and > 0, got {a.motion_res}")
    if a.motion_res is None and not a.field:
        ap.error("give --field or --motion-res")
    if a.spheres and not a.field:
        ap.error("--spheres needs --field")
    if not 1 <= a.max_samples <= MAX_SAMPLES:
        ap.error(f"--max-samples must be in 1..{MAX_SAMPLES}, got {a.max_samples}")
    if hasattr(a, "nodes"):
        if not 1 <= a.nodes <= MAX_NODES:
            ap.error(f"--nodes must be in 1..{MAX_NODES}, got {a.nodes}")
        if not 1 <= a.k <= MAX_K:
            ap.error(f"--k must be in 1..{MAX_K}, got {a.k}")


def _scene(a):
    from .field import DistanceField
    arm = _arm.load_arm_option(a.arm)
    if a.base:
        arm = arm.with_base(np.load(a.base))
        arm.to_array()
    field = DistanceField.load(a.field) if a.field else None
    spheres = np.asarray(np.load(a.spheres), np.float32).reshape(-1, 3) if a.spheres else None
    kw = dict(spheres=spheres, radius=a.radius, margin=a.margin, self_margin=a.self_margin, res=a.motion_res,
              max_samples=a.max_samples)
    return arm, field, kw


def plan_report(p: Plan) -> dict:
    """Plan as arrays: cost, length, hops (A, B) and waypoints (A, B, W, J), NaN beyond a route's end."""
    A, B = p.cost.shape
    J = p.roadmap.nodes.shape[1]
    W = max([len(r) for row in p.routes for r in row if r is not None] + [1])
    way = np.full((A, B, W, J), np.nan)
    for a in range(A):
        for b in range(B):
            if p.routes[a][b] is not None:
                way[a, b, :len(p.routes[a][b])] = p.routes[a][b]
    return dict(cost=p.cost, length=p.length, hops=p.hops, waypoints=way)


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.roadmap",
                                 description="A roadmap between joint configurations of an arm over a saved distance "
                                             "field, and routes through it.")
    sub = ap.add_subparsers(dest="command", required=True)
    bp = sub.add_parser("build", help="sample, test and save a roadmap")
    _motion_options(bp)
    _build_options(bp)
    bp.add_argument("--out", required=True, help="output .npz roadmap")
    pp = sub.add_parser("plan", help="routes from every --from configuration to every --to configuration")
    _motion_options(pp)
    _build_options(pp)
    pp.add_argument("--roadmap", default=None, help=".npz of the build command (its parameters hold); default: a fresh one")
    pp.add_argument("--from", dest="q_from", required=True, help=".npy (A, J) or (J,) start configurations")
    pp.add_argument("--to", dest="q_to", required=True, help=".npy (B, J) or (J,) goal configurations")
    pp.add_argument("--shortcut", type=int, default=0, help="string-pull the routes over this window (0: not)")
    pp.add_argument("--out", required=True, help="output .npz cost, length, hops, waypoints (A, B, W, J; NaN padded)")
    pp.add_argument("--time-limits", default=None, metavar="{default,FILE.json}",
                    help="joint velocity and acceleration limits: adds duration (A, B), seconds, to the report "
                         "(python -m gaussiangrasper_amd.trajectory)")
    a = ap.parse_args(argv)
    sp = bp if a.command == "build" else pp
    _check_options(sp, a)
    if a.command == "plan" and a.shortcut < 0:
        sp.error(f"--shortcut must be >= 0, got {a.shortcut}")
    try:
        arm, field, kw = _scene(a)
        if a.command == "build":
            rm = build(arm, field, num_nodes=a.nodes, k=a.k, seed=a.seed, unit=a.unit, **kw)
            rm.save(a.out)
            print(f"{int(rm.valid.sum())} of {rm.num_nodes} nodes clear, {int(rm.motion.ok.sum())} of {len(rm.edge_a)} "
                  f"tested edges clear, {rm.dropped} dropped as too long; wrote {a.out}")
            return 0
        J = arm.num_joints
        ends = []
        for name in (a.q_from, a.q_to):
            q = np.asarray(np.load(name), np.float64)
            if q.ndim not in (1, 2) or q.shape[-1] != J:
                raise ValueError(f"{name}: expected ({J},) or (A, {J}) configurations, got {q.shape}")
            ends.append(q.reshape(-1, J))
        if a.roadmap:
            p = plan(arm, ends[0], ends[1], field, roadmap=Roadmap.load(a.roadmap).attach(arm, field),
                     shortcut_window=a.shortcut)
        else:
            p = plan(arm, ends[0], ends[1], field, shortcut_window=a.shortcut, num_nodes=a.nodes, k=a.k, seed=a.seed,
                     unit=a.unit, **kw)
        report = plan_report(p)
        if a.time_limits:
            from . import trajectory as _traj
            report["duration"] = _traj.time_plan(p, _traj.load_limits_option(a.time_limits), arm=arm).duration
        np.savez(a.out, **report)
    except (KeyError, ValueError, OSError, _lib.GGError) as exc:
        raise SystemExit(f"error: {exc}") from exc
    print(f"{int((p.hops >= 0).sum())} of {p.hops.size} routes found; wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
