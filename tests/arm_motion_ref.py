"""numpy fp64 restatement of gg_arm_self and gg_arm_motion (include/gg_raster.h), built on arm_ref's fk, sphere_centres
and clear, in the operation order the header gives; the sweep bound's table restated from its definition; and the
builders of the fixtures the motion tests share.  Test infrastructure: plain."""
import functools

import numpy as np

import arm_ref as ref

FAR = ref.FAR
INT32_MIN = ref.INT32_MIN
MAX_SAMPLES = 4096


# ------------------------------------------------------------------------------------------------
# the table of the sweep bound
# ------------------------------------------------------------------------------------------------
def reach_table(arm, J, spheres, frame):
    """(J, S): 0 for j >= frame[s]; 1 for a prismatic joint j; for a revolute one |offset| plus, for k = j + 1 ..
    frame - 1, |t(A_k)| and, where joint k exists and slides, max(|lo_k|, |hi_k|)"""
    _, fixed, _, lo, hi, kind = ref.unpack(arm, J)
    sp = np.asarray(spheres, np.float64).reshape(-1, 3)
    frame = np.asarray(frame, np.int64).reshape(-1)
    out = np.zeros((J, len(sp)))
    for s in range(len(sp)):
        for j in range(min(int(frame[s]), J)):
            if kind[j] == 1.0:
                out[j, s] = 1.0
                continue
            total = float(np.sqrt((sp[s] ** 2).sum()))
            for k in range(j + 1, int(frame[s])):
                total += float(np.sqrt((fixed[k, 9:] ** 2).sum()))
                if k < J and kind[k] == 1.0:
                    total += max(abs(lo[k]), abs(hi[k]))
            out[j, s] = total
    return out


def all_pairs(J):
    return np.ones((J + 2, J + 2), np.uint8)


# ------------------------------------------------------------------------------------------------
# self
# ------------------------------------------------------------------------------------------------
def pair_gaps(centres, frame, radius, pairs, J):
    """(gaps (N, K), s (K,), t (K,)) of the K tested pairs s < t in lexicographic order, for centres (N, S, 3)"""
    S = centres.shape[1]
    frame = np.clip(np.asarray(frame, np.int64).reshape(-1), 0, J + 1)
    radius = np.asarray(radius, np.float64).reshape(-1)
    s, t = np.triu_indices(S, 1)
    on = np.asarray(pairs).reshape(J + 2, J + 2)[frame[s], frame[t]] != 0
    s, t = s[on], t[on]
    d = centres[:, s] - centres[:, t]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return np.sqrt(d2) - (radius[s] + radius[t]), s, t


def self_gap(arm, J, q, spheres, frame, radius, pairs):
    """(gap (M,), pair (M, 2) int32)"""
    q = np.asarray(q, np.float64).reshape(-1, J)
    sp = np.asarray(spheres, np.float32).reshape(-1, 3).astype(np.float64)
    M = len(q)
    fin = np.isfinite(q).all(1)
    gap = np.full(M, np.inf)
    pair = np.full((M, 2), -1, np.int32)
    if len(sp) >= 2:
        cen = ref.sphere_centres(arm, J, np.where(fin[:, None], q, 0.0), sp, np.clip(frame, 0, J + 1))
        g, s, t = pair_gaps(cen, frame, radius, pairs, J)
        if g.shape[1]:
            k = np.argmin(g, axis=1)                                # the first of equals: the lowest (s, t)
            gap = g[np.arange(M), k]
            pair = np.stack([s[k], t[k]], 1).astype(np.int32)
    gap[~fin] = np.nan
    pair[~fin] = -1
    return gap, pair


# ------------------------------------------------------------------------------------------------
# motion
# ------------------------------------------------------------------------------------------------
def sweep_bound(qa, qb, reach):
    """B of one edge: b_s added for j ascending onto 0.0, then the maximum; 0 without spheres"""
    dq = np.asarray(qb, np.float64) - np.asarray(qa, np.float64)
    reach = np.asarray(reach, np.float64).reshape(len(dq), -1)
    b = np.zeros(reach.shape[1])
    for j in range(len(dq)):
        b = b + abs(dq[j]) * reach[j]
    return float(b.max()) if len(b) else 0.0


def sample_count(B, res, max_samples):
    """the smallest n >= 1 with (double)n res >= B, by the comparisons themselves; 0: not resolved"""
    if B > float(max_samples) * res:
        return 0
    n = np.arange(1, max_samples + 1)
    return int(n[np.argmax(n.astype(np.float64) * res >= B)])


def samples_of(qa, qb, n):
    i = np.arange(n + 1)
    q = qa[None, :] + (i.astype(np.float64) / float(n))[:, None] * (qb - qa)[None, :]
    q[n] = qb
    return q


def motion(arm, J, field, q_a, q_b, spheres, frame, need2, outside, radius, pairs, reach, res, max_samples=MAX_SAMPLES,
           detail=False):
    """dict of samples, slack, slack_at, worst, gap, gap_at, pair as the header states them.  field: None or (dims,
    grid, dist2); pairs: None or the table.  detail=True adds per edge B, face (the smallest distance of a sampled centre
    to a cell face, in metres) and runner_up (the second smallest (sample, pair) gap minus the smallest)."""
    q_a = np.asarray(q_a, np.float64).reshape(-1, J)
    q_b = np.asarray(q_b, np.float64).reshape(-1, J)
    sp = np.asarray(spheres, np.float32).reshape(-1, 3)
    E, S = len(q_a), len(sp)
    out = dict(samples=np.zeros(E, np.int32), slack=np.full(E, INT32_MIN, np.int32), slack_at=np.full(E, -1, np.int32),
               worst=np.full(E, -1, np.int32), gap=np.full(E, np.nan), gap_at=np.full(E, -1, np.int32),
               pair=np.full((E, 2), -1, np.int32))
    if detail:
        out.update(B=np.full(E, np.nan), face=np.full(E, np.inf), runner_up=np.full(E, np.inf))
    for e in range(E):
        if not (np.isfinite(q_a[e]).all() and np.isfinite(q_b[e]).all()):
            continue
        B = sweep_bound(q_a[e], q_b[e], reach) if S else 0.0
        if detail:
            out["B"][e] = B
        n = sample_count(B, res, max_samples)
        if n == 0:
            continue
        q = samples_of(q_a[e], q_b[e], n)
        out["samples"][e] = n
        out["slack"][e], out["slack_at"][e], out["worst"][e] = FAR, -1, -1
        if field is not None:
            dims, grid, dist2 = field
            sl, wo = ref.clear(arm, J, dims, grid, dist2, q, sp, frame, need2, outside)
            at = int(np.argmin(sl))                                 # the first of equals
            out["slack"][e], out["slack_at"][e], out["worst"][e] = sl[at], at, wo[at]
        out["gap"][e], out["gap_at"][e] = np.inf, -1
        cen = None
        if S and (detail or pairs is not None):
            cen = ref.sphere_centres(arm, J, q, sp.astype(np.float64), np.clip(frame, 0, J + 1))
        if pairs is not None:
            out["gap_at"][e] = 0
            if S >= 2:
                g, s, t = pair_gaps(cen, frame, radius, pairs, J)
                if g.shape[1]:
                    k = int(np.argmin(g))                           # row-major: the lowest sample, then the lowest pair
                    i, p = divmod(k, g.shape[1])
                    out["gap"][e], out["gap_at"][e], out["pair"][e] = g[i, p], i, (s[p], t[p])
                    if detail and g.size > 1:
                        two = np.partition(g.reshape(-1), 1)[:2]
                        out["runner_up"][e] = two[1] - two[0]
        if detail and field is not None and S:
            grid = np.asarray(field[1], np.float64)
            u = (cen - grid[:3]) / grid[3]
            out["face"][e] = float(np.abs(u - np.round(u)).min() * grid[3])
    return out


# ------------------------------------------------------------------------------------------------
# fixtures (built once per process)
# ------------------------------------------------------------------------------------------------
TARGETS = (1, 2, 3, 63, 64, 65, 200)
EDGE_SEED = {"default": 3, "prismatic": 5}


def scaled_edges(arm, J, q0, reach, res, targets, rng, lo=None, hi=None, weight=None):
    """edges from the rows of q0 in random directions (times `weight` per joint), scaled so that B = (target - 1/2) res:
    n is the target.  With limits, the direction of a joint that would leave them is turned round."""
    E = len(q0)
    d = rng.normal(size=(E, J)) * (1.0 if weight is None else weight)
    q1 = np.empty_like(q0)
    for e in range(E):
        B = sweep_bound(np.zeros(J), d[e], reach)
        step = d[e] * ((targets[e % len(targets)] - 0.5) * res / B)
        if lo is not None:
            out = (q0[e] + step < lo) | (q0[e] + step > hi)
            step = np.where(out, -step, step)
        q1[e] = q0[e] + step
    return q1


@functools.lru_cache(maxsize=None)
def edge_fixture(which="default"):
    """257 edges over arm_ref.field_fixture's volume with res = h, the sample counts cycling through TARGETS, and the
    restatement's outputs with their detail.  "default": the default arm, its link spheres and four gripper-frame
    ones (each moved off its joint axis a little), default_self_pairs; "prismatic": random_chain(8, 5, prismatic=(2, 5)) with 23 random spheres, every frame pair
    two apart tested, the edges within the limits."""
    from gaussiangrasper_amd import arm as A
    from gaussiangrasper_amd.field import need2
    f = ref.field_fixture()
    dims, grid, dist2 = f["dims"], f["grid"], f["dist2"]
    res = float(grid[3])
    rng = np.random.default_rng(EDGE_SEED[which])
    if which == "default":
        arm, J = f["arm"], f["J"]
        # the link spheres' centres sit on joint axes and origins, where the distance of a pair can be the same at every
        # sample (shoulder to elbow); moved off them by up to 2 cm, no smallest gap is shared by two samples
        spheres = (f["spheres"] + rng.uniform(-0.02, 0.02, size=f["spheres"].shape)).astype(np.float32)
        frame = f["frame"]
        radius = np.concatenate([A.default_arm().link_spheres()[2], np.full(len(f["gripper"]), 0.01)])
        pairs = A.default_self_pairs(A.default_arm())
        q0, lo, hi, weight = f["q"], None, None, None
    else:
        arm, J = ref.random_chain(8, 5, prismatic=(2, 5))
        arm = arm.copy()
        arm[9:12] = (0.0, -0.1, 0.3)                                 # the base in a free part of the volume
        lo, hi = ref.unpack(arm, J)[3:5]
        spheres = rng.uniform(-0.1, 0.1, size=(23, 3)).astype(np.float32)
        frame = rng.integers(0, J + 2, size=23).astype(np.int32)
        radius = rng.uniform(0.02, 0.06, size=23)
        pairs = np.zeros((J + 2, J + 2), np.uint8)
        for a in range(J + 2):
            for b in range(J + 2):
                pairs[a, b] = abs(a - b) >= 2
        q0 = ref.in_limits(arm, J, 257, rng, inset=0.02)
        weight = np.where(ref.unpack(arm, J)[5] == 1.0, 0.01, 1.0)    # the sliding joints have half a metre in all
    reach = reach_table(arm, J, spheres, frame)
    need = need2(radius + 0.5 * res, 0.0, res)
    q1 = scaled_edges(arm, J, q0, reach, res, TARGETS, rng, lo, hi, weight)
    want = motion(arm, J, (dims, grid, dist2), q0, q1, spheres, frame, need, FAR, radius, pairs, reach, res,
                  detail=True)
    return dict(arm=arm, J=J, dims=dims, grid=grid, dist2=dist2, q_a=q0, q_b=q1, spheres=spheres, frame=frame,
                need=need, radius=radius, pairs=pairs, reach=reach, res=res, want=want, lo=lo, hi=hi)


FIELD_BOXES = (((4, 9), (20, 30), (10, 16)), ((28, 36), (5, 12), (0, 6)), ((18, 22), (16, 20), (30, 40)),
               ((10, 30), (28, 33), (18, 21)))                      # arm_ref.field_fixture's occupied blocks, in cells


def distance_to_occupied(points):
    """the exact distance of (N, 3) world points to the union of the field fixture's occupied cubes"""
    lo = np.array(ref.FIELD_LO)
    best = np.full(len(points), np.inf)
    for box in FIELD_BOXES:
        a = lo + np.array([b[0] for b in box]) * ref.FIELD_H
        b = lo + np.array([b[1] for b in box]) * ref.FIELD_H
        d = np.maximum(np.maximum(a - points, points - b), 0.0)
        best = np.minimum(best, np.sqrt((d * d).sum(1)))
    return best
