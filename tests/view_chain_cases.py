"""Constructed Gaussians for the per-Gaussian chain of one view (csrc/project.hip: gg_view_fwd, gg_shade_tail_fwd,
gg_view_bwd / gg_view_bwd_pose, their three-kernel fallback and the SH expansion).  CPU only (numpy, and the float64
restatement to place the radii): what the constructions claim is established on the CPU by
tests/test_view_chain_cases_host.py, the kernels are run on them by tests/test_view_chain_gpu.py.

Every Gaussian is placed in the camera frame — a depth tz and multiples (a, b) of lim_x tz and lim_y tz along the
camera's right / down axes, lim = 1.3 tan(fov / 2) being the EWA clamp — and mapped to the world through the view's own
matrices; its size is given in pixels at its depth (sigma_px = f s / tz).  The leaves are float32 (what the kernels
read); the float64 restatement (tests/view_chain_ref.py) reads the same float32 values.  Each case holds, on each of
three views, Gaussians on both sides of every branch the device code takes:

  near plane      tz = clip (1 +- DELTA); deep ones at 30 ... 1000
  FOV clamp       t.x / t.z and t.y / t.z at +-lim (1 +- DELTA): each axis alone, both, mixed signs; 1.5 and 3 times the
                  limit, large enough to stay visible
  eigenvalue      isotropic splats (bm^2 - det far under the floor), anisotropic ones far above it
  radius          3 sqrt(lambda) at an integer +- 0.02
  tile box        centres outside each side and corner of the tile grid by the radius -+ 0.04 pixels (area 0 / area >= 1);
                  one splat covering every tile
  activations     log-scales -12 ... +4; ties of the smallest scale in every position; opacity logits 0, +-8, +-30;
                  |q| = 1e-3 ... 1e3, single-component quaternions of both signs, |q| = 1e-13 (the branch under
                  F.normalize's eps).  The zero quaternion is NaN in the reference model too (q / |q|) and is left out.
  SH tail         colour rows solved so that every clamp-mask value occurs at every degree; rows 1e-3 either side of
                  both clamp bounds; view directions on the coordinate axes (the two poles among them)
  records         16-float rows with NaN in columns 13 ... 15 (never read), all-zero rows, invisible rows with
                  cotangents

DELTA and the distances above are conditions on the float64 restatement; the radius of every Gaussian not built for
the radius edge is moved to an integer + 0.5 (all three log-scales shifted together), so that ceil() is decided the same
way in both precisions whatever the size.  Representatives of the edges sit on lanes 0, 63, 64, 255, 256 and the
last index, so the truncations N = 1, 64, 255, 256, 257 end on them."""
from collections import namedtuple

import numpy as np
import torch

import view_chain_ref as ref
from gaussiangrasper_amd.camera import ring_cameras
from gaussiangrasper_amd.constants import CLIP_THRESH_DEFAULT, num_sh_bases

DELTA = 1e-3
MARGIN = 1e-4              # the least relative distance of any compared quantity from its threshold
SIZES = ((16, 16), (17, 33), (48, 64))      # (h, w): one tile, ragged both ways, 3 x 4 tiles
TRUNCATIONS = (1, 64, 255, 256, 257)
KEY_LANES = (0, 63, 64, 255, 256, -1)
NUM = 560

# The fp32 oracle chain against the float64 restatement on these cases, worst row-relative error per parameter over
# the three cases (tests/test_view_chain_cases_host.py measures them and holds them under these; PARITY.md lists the
# measured values).  The kernels are allowed twice as much (ocml expf in the activations is not numpy's; operation order), and no more.
# colors_all_two_views: the SH gradient of two views added in float32, whose terms cancel in part.
ORACLE_WORST = {"means": 2e-6, "log_scales": 8e-6, "quats": 2e-5, "opacities": 5e-5, "colors_all": 1e-6,
                "colors_all_two_views": 3.5e-6}
FWD_WORST = 1e-5           # the same for the forward's float outputs (the pixel centre of a Gaussian at the near plane)

# leaves float32: means (N, 3), log_scales (N, 3), quats (N, 4), opacities (N, 1), colors_all (N, 25, 3); view: ref.View;
# degree: degrees_to_use; labels: the edge every Gaussian was built for; edges {label: indices}; record (N, 16) float32
Case = namedtuple("Case", "name means log_scales quats opacities colors_all view degree labels edges record")


def make_view(h, w, which=1):
    """which = 1: the view the Gaussians are built for; 2: another camera of the ring, for the SH gradient of two views
    (the clamp mask keeps its margins from any direction, see _colors; nothing else of that view is compared)"""
    # a camera close to the origin: world coordinates of the Gaussians at the near plane stay small, so that the fp32
    # rounding of t.z = V p + T there stays some 1e-6 of clip
    v = ring_cameras(3, h, w, radius=0.25)[which]
    f32 = lambda x: float(np.float32(x))
    return ref.View(v.cam_pos.numpy().astype(np.float32).reshape(3), v.viewmat[:3].numpy().astype(np.float32),
                    v.projmat.numpy().astype(np.float32), f32(v.fx), f32(v.fy), f32(v.cx), f32(v.cy), h, w,
                    tuple(int(t) for t in v.tile_bounds), CLIP_THRESH_DEFAULT)


class _Builder:
    def __init__(self, view, seed):
        self.view, self.rng, self.rows = view, np.random.default_rng(seed), []
        self.lim_x = ref.pref.FOV_LIM * 0.5 * view.w / view.fx
        self.lim_y = ref.pref.FOV_LIM * 0.5 * view.h / view.fy

    def quat(self, norm=None):
        q = self.rng.normal(size=4)
        q /= np.linalg.norm(q)
        return q * (np.exp(self.rng.uniform(-0.5, 0.5)) if norm is None else norm)

    def add(self, label, a=None, b=None, tz=None, sigma_px=None, log_scales=None, quat=None, logit=None, pixel=None,
            world=None, snap=True):
        """a, b: t.x / t.z and t.y / t.z as multiples of the clamp limits (or `pixel`: the centre's pixel position);
        sigma_px: the three sizes in pixels at depth tz (or `log_scales`); world: the mean itself"""
        v, rng = self.view, self.rng
        tz = float(np.exp(rng.uniform(np.log(0.5), np.log(6.0)))) if tz is None else tz
        if pixel is not None:
            rx, ry = (pixel[0] + 0.5 - v.cx) / v.fx, (pixel[1] + 0.5 - v.cy) / v.fy
        else:
            rx = (rng.uniform(-0.8, 0.8) if a is None else a) * self.lim_x
            ry = (rng.uniform(-0.8, 0.8) if b is None else b) * self.lim_y
        t = np.array([rx * tz, ry * tz, tz])
        R, T = v.viewmat[:, :3].astype(np.float64), v.viewmat[:, 3].astype(np.float64)
        mean = R.T @ (t - T) if world is None else np.asarray(world, np.float64)
        if log_scales is None:
            sigma_px = np.exp(rng.uniform(np.log(0.4), np.log(4.0), 3)) if sigma_px is None else np.asarray(sigma_px, float)
            log_scales = np.log(sigma_px * tz / v.fx)
        self.rows.append({"label": label, "mean": mean, "log_scales": np.broadcast_to(np.asarray(log_scales, float), 3),
                          "quat": self.quat() if quat is None else np.asarray(quat, float),
                          "logit": rng.uniform(-2.0, 2.0) if logit is None else logit, "snap": snap})


def _colors(n, rng, edge_rows):
    """(N, 25, 3): row i is solved for clamp-mask value i % 8 at EVERY degree — the sum of the bases past the first stays
    under 0.35 and rgb + 0.5 without it is -0.5 (below), 0.5 (open) or 1.5 (above) — and the `edge_rows` hold only the
    first coefficient, with rgb + 0.5 at 0 -+ 1e-3 and 1 -+ 1e-3 (closed, open, open, closed), one channel each way"""
    col = rng.uniform(-0.04, 0.04, (n, 25, 3))
    want = np.zeros((n, 3))
    for i in range(n):
        for c in range(3):
            open_ = (i % 8) >> c & 1
            want[i, c] = 0.5 if open_ else (-0.5 if (i // 8 + c) % 2 else 1.5)
    col[:, 0, :] = (want - 0.5) / ref.SH_C0
    near = (-1e-3, 1e-3, 1.0 - 1e-3, 1.0 + 1e-3)
    for k, i in enumerate(edge_rows):
        col[i, 1:, :] = 0.0
        col[i, 0, :] = (np.array([near[k % 4], near[(k + 1) % 4], near[(k + 2) % 4]]) - 0.5) / ref.SH_C0
    return col


def _snap_radii(means, log_scales, quats, opac, col, view, keep):
    """shift the three log-scales of every Gaussian outside `keep` together until 3 sqrt(lambda) is an integer + 0.5"""
    ls = log_scales.copy()
    for _ in range(20):
        out = ref.forward(*(ref.f64(a) for a in (means, ls, quats, opac, col)), view, 0)
        r = out["margins"]["radius"].numpy()
        off = np.abs(r - (np.floor(r) + 0.5))
        todo = (~keep) & (off > 0.2)
        if not todo.any():
            break
        # (the radius grows like the scale where the blur does not dominate it, more slowly where it does)
        target = np.floor(r) + 0.5
        target = np.where(target < 2.0, 2.5, target)
        ls[todo] = (ls[todo].astype(np.float64) + np.log(target / r)[todo, None]).astype(np.float32)
    return ls


def margins(out, view):
    """{quantity: (N,) relative distance from its threshold} of a float64 forward (ref.forward's output): tz from clip,
    |t.x / t.z| and |t.y / t.z| from the clamp limits, bm^2 - det from the eigenvalue floor, the radius from the integers
    ceil() steps at, the tile-box corners from the integers 1 ... bound their truncation steps at (below 1 the clamp at 0
    gives the same tile either way), the activated scales from each other unless equal, and rgb + 0.5 from 0 and 1.  The
    quantities the projection only forms in front of the near plane are held to it there alone."""
    m = out["margins"]
    front = (m["tz"] > view.clip).numpy()
    inf = np.full(front.shape, np.inf)
    res = {"tz": ((m["tz"] - view.clip).abs() / view.clip).numpy()}
    res["rx"] = np.where(front, ((m["rx"].abs() - m["lim_x"]).abs() / m["lim_x"]).numpy(), inf)
    res["ry"] = np.where(front, ((m["ry"].abs() - m["lim_y"]).abs() / m["lim_y"]).numpy(), inf)
    gap = m["eig_gap"].numpy()
    res["eig_gap"] = np.where(front, np.abs(gap - ref.EIG_FLOOR) / np.maximum(np.abs(gap), ref.EIG_FLOOR), inf)
    r = m["radius"].numpy()
    res["radius"] = np.where(front, np.abs(r - np.round(r)) / r, inf)
    c, bound = m["corners"].numpy(), m["bounds"].numpy()
    step = np.clip(np.round(c), 1.0, bound)                 # the nearest integer at which the truncated corner changes
    res["corners"] = np.where(front, (np.abs(c - step) / np.maximum(np.abs(c), 1.0)).min(-1), inf)
    s = out["scales"].detach().numpy()
    d = np.stack([np.abs(s[:, i] - s[:, j]) / np.maximum(s[:, i], s[:, j]) for i, j in ((0, 1), (0, 2), (1, 2))], -1)
    res["scale_ties"] = np.where(d == 0, np.inf, d).min(-1)
    raw = m["rgb_raw"].numpy()
    res["rgb"] = np.minimum(np.abs(raw), np.abs(raw - 1.0)).min(-1)
    return res


def build_case(h, w, seed=0):
    view = make_view(h, w)
    b = _Builder(view, seed + 1000 * h + w)
    rng = b.rng
    big = 0.1 * max(h, w) + 2.0                     # pixels: reaches the image from the clamp limit
    clip = view.clip
    # ---- near plane, deep
    for k in range(4):
        b.add("near_in", tz=clip * (1 + DELTA), a=rng.uniform(-0.5, 0.5), b=rng.uniform(-0.5, 0.5))
        b.add("near_out", tz=clip * (1 - DELTA), a=rng.uniform(-0.5, 0.5), b=rng.uniform(-0.5, 0.5))
    for tz in (30.0, 100.0, 300.0, 1000.0):
        b.add("deep", tz=tz)
    # ---- FOV clamp: every sign combination, just inside and just outside; far outside
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            if sx == 0 and sy == 0:
                continue
            for side, f in (("out", 1 + DELTA), ("in", 1 - DELTA)):
                for _ in range(2):
                    b.add(f"clamp_{side}[{sx:+d},{sy:+d}]", a=sx * f if sx else None, b=sy * f if sy else None,
                          sigma_px=big * np.exp(rng.uniform(-0.2, 0.2, 3)))
    for mult, size in ((1.5, 0.35), (3.0, 1.1)):
        s = (size * max(h, w) + 3.0) * np.array([1.0, 1.2, 0.9])
        b.add(f"clamp_far[{mult}]", a=mult, b=0.2, sigma_px=s)
        b.add(f"clamp_far[{mult}]", a=-mult, b=-0.3, sigma_px=s)
        b.add(f"clamp_far[{mult}]", a=0.1, b=mult, sigma_px=s)
        b.add(f"clamp_far[{mult}]", a=-0.2, b=-mult, sigma_px=s)
        b.add(f"clamp_far[{mult}]", a=mult, b=-mult, sigma_px=s)
    # ---- eigenvalue floor: isotropic (far under it), strongly anisotropic (far above)
    for _ in range(8):
        b.add("eig_floor", sigma_px=np.full(3, rng.uniform(0.3, 1.5)), a=rng.uniform(-0.3, 0.3), b=rng.uniform(-0.3, 0.3))
    # ---- radius either side of an integer: isotropic at the image centre, cov2d = (sigma^2 + 0.3) I
    for k in (4, 5, 6):
        for d in (-0.02, 0.02):
            sig = np.sqrt(((k + d) / 3.0) ** 2 - 0.3 - np.sqrt(0.1))
            b.add(f"radius[{k}{d:+.2f}]", pixel=(view.cx - 0.5, view.cy - 0.5), sigma_px=np.full(3, sig), snap=False)
    # ---- tile box: tiny splats (radius 3) either side of every edge and corner of the tile grid
    gx, gy = 16.0 * view.tile_bounds[0], 16.0 * view.tile_bounds[1]
    for side, e in (("out", 0.04), ("in", -0.04)):
        xs = {"l": -3.0 - e, "m": 0.37 * w, "r": gx + 3.0 + e}
        ys = {"t": -3.0 - e, "m": 0.41 * h, "b": gy + 3.0 + e}
        for kx in "lmr":
            for ky in "tmb":
                if kx == "m" and ky == "m":
                    continue
                b.add(f"box_{side}[{kx}{ky}]", pixel=(xs[kx], ys[ky]), log_scales=np.full(3, -11.0), tz=1.5, snap=False)
    b.add("cover_all", a=0.0, b=0.0, sigma_px=np.full(3, 2.0 * max(h, w)) * np.array([1.0, 0.8, 1.1]))
    # ---- activations
    for v in (-12.0, -10.0, -8.0, -6.0, -4.0):
        b.add("scale_range", log_scales=np.array([v, v + 0.5, v + 1.0]), tz=2.0)
    for v in (0.0, 2.0, 3.0, 4.0):
        b.add("scale_range", log_scales=np.array([v - 1.0, v, v - 0.5]), tz=1000.0, a=0.1, b=-0.1)
    lo, hi = 1.0, 2.5
    for pattern in ((lo, lo, hi), (lo, hi, lo), (hi, lo, lo), (lo, lo, lo), (lo, hi, 2 * hi), (hi, lo, 2 * hi),
                    (2 * hi, hi, lo)):
        for _ in range(2):
            b.add("tie" + str(tuple(int(p == lo) for p in pattern)), sigma_px=np.array(pattern))
    for logit in (0.0, 8.0, -8.0, 30.0, -30.0):
        for _ in range(2):
            b.add(f"logit[{logit:+.0f}]", logit=logit)
    for e in (-3, -2, -1, 0, 1, 2, 3):
        for _ in range(2):
            b.add(f"qnorm[1e{e:+d}]", quat=b.quat(10.0 ** e))
    for k in range(4):
        for s in (1.0, -1.0):
            q = np.zeros(4)
            q[k] = s * rng.uniform(0.5, 2.0)
            b.add("q_single", quat=q)
    for _ in range(4):
        b.add("q_tiny", quat=b.quat(1e-13))
    # ---- view directions on the coordinate axes
    for k in range(3):
        for s in (2.0, -2.0):
            e = np.zeros(3)
            e[k] = s
            b.add("dir_axis", world=view.cam_pos.astype(np.float64) + e, log_scales=np.array([-3.0, -2.5, -2.0]))
    while len(b.rows) < NUM:
        b.add("plain")
    rows = b.rows
    assert len(rows) == NUM
    # ---- lanes: one representative of six edges on lanes 0, 63, 64, 255, 256 and the last index
    first = lambda lab: next(i for i, r in enumerate(rows) if r["label"].startswith(lab))
    keys = [first("clamp_out[+1,+1]"), first("near_in"), first("q_tiny"), first("clamp_out[-1,+1]"), first("near_out"),
            first("tie(1, 1, 1)")]
    order = list(range(NUM))
    for lane, k in zip(KEY_LANES, keys):
        lane = lane % NUM
        i, j = order.index(k), lane
        order[i], order[j] = order[j], order[i]
    rows = [rows[i] for i in order]
    means = np.stack([r["mean"] for r in rows]).astype(np.float32)
    log_scales = np.stack([r["log_scales"] for r in rows]).astype(np.float32)
    quats = np.stack([r["quat"] for r in rows]).astype(np.float32)
    opac = np.array([[r["logit"]] for r in rows], np.float32)
    labels = np.array([r["label"] for r in rows])
    sh_edge = np.flatnonzero(labels == "plain")[:8]
    col = _colors(NUM, rng, sh_edge).astype(np.float32)
    keep = np.array([not r["snap"] for r in rows])
    log_scales = _snap_radii(means, log_scales, quats, opac, col, view, keep)
    # a filler Gaussian that happens to land near a threshold (a tile-box corner near an integer, mostly) is drawn again
    for _ in range(8):
        out = ref.forward(*(ref.f64(a) for a in (means, log_scales, quats, opac, col)), view, 0)
        worst = np.min(np.stack([m for k, m in margins(out, view).items() if k != "rgb"]), axis=0)
        bad = np.flatnonzero((worst < 3 * MARGIN) & (labels == "plain"))
        if bad.size == 0:
            break
        for i in bad:
            b.add("plain")
            r = b.rows.pop()
            means[i], quats[i] = r["mean"].astype(np.float32), r["quat"].astype(np.float32)
            log_scales[i] = r["log_scales"].astype(np.float32)
        log_scales = _snap_radii(means, log_scales, quats, opac, col, view, keep)
    labels[sh_edge] = "sh_edge"
    # ---- the gradient record: random cotangents, NaN in the columns nothing reads, some all-zero rows
    g = torch.Generator(device="cpu").manual_seed(seed + 7)
    record = torch.randn(NUM, 16, generator=g).numpy().astype(np.float32)
    record[:, 13:] = np.nan
    zero_rows = np.concatenate([np.flatnonzero(labels == "plain")[-6:], np.flatnonzero(labels == "near_out")[-1:],
                                np.flatnonzero(labels == "clamp_out[+1,-1]")[-1:]])
    record[zero_rows, :13] = 0.0
    edges = {lab: np.flatnonzero(labels == lab) for lab in sorted(set(labels))}
    edges["zero_rows"] = np.sort(zero_rows)
    return Case(f"{h}x{w}", means, log_scales, quats, opac, col, view, 4, labels, edges, record)


_CASES = {}


def cases():
    """the three cases, built once"""
    if not _CASES:
        for h, w in SIZES:
            _CASES[f"{h}x{w}"] = build_case(h, w)
    return _CASES


def second_record(seed=11):
    """the second view's gradient record (the SH gradient of two views): another draw of cotangents"""
    rec = torch.randn(NUM, 16, generator=torch.Generator().manual_seed(seed)).numpy().astype(np.float32)
    rec[:, 13:] = np.nan
    return rec


def colors_for(case, deg, full):
    """the SH coefficients the tests hand over for `deg`: all 25 rows (`full`) or the first num_sh_bases(deg)"""
    return case.colors_all if full else np.ascontiguousarray(case.colors_all[:, :num_sh_bases(deg)])
