"""Restatement of the blend votes (include/gg_raster.h gg_blend_votes) on the CPU oracle, and the scenes the lift tests
share.

The per-pixel weights come from the oracle's own forward: with colours = the identity matrix over a zero background,
channel g of pixel p is an fma chain of ONE product vis(p, g) * 1 and zeros, i.e. exactly the value by which the
walk multiplies Gaussian g's colour there.  q = trunc(vis 2^24) and the sums over the pixels of each label follow in
integers."""
import math

import numpy as np
import torch

from gaussiangrasper_amd.camera import ring_cameras
from gaussiangrasper_amd.scene import Scene, make_scene

UNIT = np.float32(2 ** 24)
IGNORE = 255

#        name: (n, h, w, view, grow, opacity shift)
SCENES = {
    "S1": (1, 16, 16, 0, None, None),
    "S2": (7, 45, 70, 0, None, None),
    "D1": (400, 32, 32, 1, 12.0, 3.0),
    "D2": (1500, 45, 70, 1, 10.0, 3.0),
    "D3": (3000, 83, 101, 1, 8.0, 2.0),
}


def build_scene(n, grow=None, ob=None):
    sc = make_scene(n, config_index=1)
    if grow is not None:
        sc.scales += math.log(grow)
        sc.opacities += ob
    return sc


def activated(sc, device="cpu"):
    """(means, scales, quats, opacity (N, 1)) as lift.project_view hands them to the projection, numpy fp32; the
    activations are torch's on `device` (exp and sigmoid may differ in the last bit between devices)."""
    sc = sc.to(device)
    return tuple(t.cpu().numpy() for t in (
        sc.means.float(), torch.exp(sc.scales.float()), (sc.quats / sc.quats.norm(dim=-1, keepdim=True)).float(),
        torch.sigmoid(sc.opacities.float()).reshape(-1, 1)))


def ring(num_views, h, w):
    """camera.ring_cameras as (c2w (4, 4), intrinsics, h, w) tuples, the form mesh.mesh_model and lift.lift_labels
    take: the c2w is read back from the view matrix (exact: transposes and sign flips)."""
    cams = []
    for v in ring_cameras(num_views, h, w):
        c2w = np.eye(4)
        c2w[:3, :3] = v.viewmat[:3, :3].numpy().T.astype(np.float64) * np.array([1.0, -1.0, -1.0])
        c2w[:3, 3] = v.cam_pos.numpy()
        cams.append((c2w, (v.fx, v.fy, v.cx, v.cy), h, w))
    return cams


def view_of(camera):
    """The ViewParams lift.project_view derives from one camera tuple."""
    from gaussiangrasper_amd.camera import view_from_c2w
    c2w, K, h, w = camera
    return view_from_c2w(torch.as_tensor(c2w), *K, h, w)


def project(O, act, v):
    """The oracle's projection of activated parameters for a camera.ViewParams: dict of numpy arrays."""
    means, scales, quats, op = act
    xys, depths, radii, conics, nth, _ = O.project_fwd(means, scales, 1.0, quats, v.viewmat[:3].cpu().numpy(),
                                                       v.projmat.cpu().numpy(), v.fx, v.fy, v.cx, v.cy, v.height,
                                                       v.width, v.tile_bounds)
    return dict(xys=xys, depths=depths, radii=radii, conics=conics, nth=nth, opacity=op, h=v.height, w=v.width)


def pixel_weights(O, p):
    """W (H, W, N) float32 with W[p, g] = vis(p, g), the forward's final_T (H, W) and the oracle's lists; None, None,
    bins when nothing is visible."""
    n = p["xys"].shape[0]
    W, saved = O.rasterize_fwd(p["xys"], p["depths"], p["radii"], p["conics"], p["nth"], np.eye(n, dtype=np.float32),
                               p["opacity"], p["h"], p["w"], np.zeros(n, np.float32))
    if saved["final_Ts"] is None:
        return None, None, saved["bins"]
    return W, saved["final_Ts"], saved["bins"]


def quantise(W):
    """q (H, W, N) int64 = trunc(vis 2^24); the product is exact in fp32"""
    return (W * UNIT).astype(np.int64)


def votes_from_q(q, labels, num_labels):
    n = q.shape[-1]
    out = np.zeros((n, num_labels), np.int64)
    if q.size == 0:
        return out
    for l in range(num_labels):
        out[:, l] = q[labels == l].sum(axis=0)
    return out


class Case:
    """One scene and view: the oracle's projection, W, q and the lists (computed once, shared, never modified)."""

    def __init__(self, O, name):
        n, h, w, view, grow, ob = SCENES[name]
        self.name, self.n, self.h, self.w = name, n, h, w
        self.scene = build_scene(n, grow, ob)
        self.view = ring_cameras(3, h, w)[view]
        self.proj = project(O, activated(self.scene), self.view)
        W, final_T, bins = pixel_weights(O, self.proj)
        self.W, self.final_T, self.bins = W, final_T, bins
        self.q = quantise(W) if W is not None else np.zeros((h, w, n), np.int64)
        for a in (self.W, self.final_T, self.q):
            if a is not None:
                a.setflags(write=False)

    def votes(self, labels, num_labels):
        return votes_from_q(self.q, np.asarray(labels), num_labels)


_cases = {}


def case(O, name):
    if name not in _cases:
        _cases[name] = Case(O, name)
    return _cases[name]


# ------------------------------------------------------------------------------------------------
# label patterns (every one a (h, w) uint8 image and its number of labels)
# ------------------------------------------------------------------------------------------------
def label_patterns(h, w, seed):
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(seed)
    rnd = rng.integers(0, 8, (h, w)).astype(np.uint8)
    rnd[rng.random((h, w)) < 0.1] = IGNORE
    return {
        "one": (np.zeros((h, w), np.uint8), 1),
        "ignored": (np.full((h, w), IGNORE, np.uint8), 2),
        "checker": (((xx + yy) % 3).astype(np.uint8), 3),
        "split": (((xx % 8 >= 3).astype(np.uint8) + 2 * (yy % 8 >= 5).astype(np.uint8)).astype(np.uint8), 4),
        "random": (rnd, 8),
        "wide": (np.where((xx // 3 + yy // 5) % 2 == 0, 0, 254).astype(np.uint8), 255),
        "beyond": ((rnd % 6).astype(np.uint8), 4),        # labels 4 and 5 are >= L: ignored by the kernel
        "many": (((xx * 7 + yy * 13) % 40).astype(np.uint8), 40),   # up to 40 labels in a quadrant
    }


# ------------------------------------------------------------------------------------------------
# the two-object scene
# ------------------------------------------------------------------------------------------------
def two_object_scene():
    """Two balls of 150 Gaussians on a table of 300; member[g] = 1 / 2 for the balls, 0 for the table."""
    rng = np.random.default_rng(7)

    def ball(c):
        d = rng.normal(size=(150, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return np.asarray(c) + d * 0.15 * rng.random(150)[:, None] ** (1.0 / 3.0)

    b1, b2 = ball((-0.35, 0.0, 0.0)), ball((0.35, 0.0, 0.0))
    table = np.concatenate([rng.uniform(-0.9, 0.9, (300, 2)), np.full((300, 1), -0.2)], axis=1)
    means = np.concatenate([b1, b2, table]).astype(np.float32)
    scales = np.concatenate([np.full((300, 3), 0.03), np.tile([0.08, 0.08, 0.01], (300, 1))]).astype(np.float32)
    n = len(means)
    quats = np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (n, 1))
    member = np.concatenate([np.full(150, 1), np.full(150, 2), np.zeros(300, int)])
    sc = Scene(torch.from_numpy(means), torch.log(torch.from_numpy(scales)), torch.from_numpy(quats),
               torch.full((n, 1), 3.0), torch.zeros(n, 1, 3), torch.zeros(n, 1))
    return sc, member


TWO_H, TWO_W, TWO_VIEWS = 96, 128, 6


class TwoObjects:
    """The two-object scene through the oracle: per view the projection, the label image (k where ball k holds at
    least half of the pixel's summed weight and that sum is >= 0.5, 0 elsewhere) and the reference votes."""

    def __init__(self, O):
        self.scene, self.member = two_object_scene()
        self.cameras = ring(TWO_VIEWS, TWO_H, TWO_W)
        self.views = [view_of(c) for c in self.cameras]
        act = activated(self.scene)
        self.labels, self.per_view = [], []
        n = len(self.member)
        self.votes = np.zeros((n, 3), np.int64)
        for v in self.views:
            p = project(O, act, v)
            W, _, _ = pixel_weights(O, p)
            W64 = W.astype(np.float64)
            total = W64.sum(axis=-1)
            lab = np.zeros((TWO_H, TWO_W), np.uint8)
            for k in (1, 2):
                wk = W64[..., self.member == k].sum(axis=-1)
                lab[(wk >= 0.5 * total) & (total >= 0.5)] = k
            ref = votes_from_q(quantise(W), lab, 3)
            self.labels.append(lab)
            self.per_view.append(ref)
            self.votes += ref


_two = []


def two_objects(O):
    if not _two:
        _two.append(TwoObjects(O))
    return _two[0]
