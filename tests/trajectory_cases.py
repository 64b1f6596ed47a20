"""The constructed cases of the arm-trajectory tests: every one is a dict of way (P, W, J), length (P,), blend (P, W),
v, a (J,) and m.  tests/test_trajectory_host.py counts from the restatement that each case holds what it was built
for; tests/test_trajectory_gpu.py runs the kernels on them.  Built once per process."""
import functools

import numpy as np

import trajectory_ref as tr

MENU = np.array([0.0, 1e-6, 0.25, 0.5])


def _case(way, length, blend, v, a, m):
    way = np.ascontiguousarray(way, np.float64)
    P, W, J = way.shape
    return dict(way=way, length=np.asarray(length, np.int32).reshape(P), blend=np.ascontiguousarray(blend, np.float64),
                v=np.asarray(v, np.float64).reshape(J), a=np.asarray(a, np.float64).reshape(J), m=int(m))


def random_case(seed, P, W, J, m, lengths=None, limits=None):
    """P random paths; the lengths cycle through `lengths` (default 1, 2, 3, 4, W), the fractions come from MENU"""
    rng = np.random.default_rng(seed)
    way = rng.uniform(-2.0, 2.0, size=(P, W, J))
    lengths = [n for n in (lengths or (1, 2, 3, 4, W)) if n <= W]
    length = np.array([lengths[p % len(lengths)] for p in range(P)])
    blend = MENU[rng.integers(0, len(MENU), size=(P, W))]
    v, a = limits if limits else (rng.uniform(0.5, 3.0, J), rng.uniform(2.0, 20.0, J))
    return _case(way, length, blend, v, a, m)


def zigzag(n, J, seed):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.uniform(0.2, 1.0, size=(n, J)) * np.where(np.arange(n)[:, None] % 2 == 0, 1.0, -1.0), axis=0)


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for J in (1, 2, 7, 8):
        out[f"joints{J}"] = random_case(10 + J, 10, 6, J, 3)
    out["longest"] = random_case(20, 5, tr.MAX_WAYPOINTS, 7, 2)
    for m in (2, 3, 16, tr.MAX_STEPS):
        out[f"steps{m}"] = random_case(30 + m, 4, 4, 2, m, lengths=(2, 3, 4, 4))
    for P in (1, 63, 64, 65, 1025):
        out[f"paths{P}"] = random_case(40 + P, P, 4, 3, 2)
    # every fraction next to every other: stops, two stops in a row, 1e-6, 1/4, 1/2 next to 1/2 (the skipped line)
    w = zigzag(12, 2, 50)
    f = np.array([0.5, 0.0, 0.0, 1e-6, 0.25, 0.5, 0.5, 0.5, 0.0, 0.25, 1e-6, 0.5])
    out["fractions"] = _case(np.stack([w, w[::-1]]), [12, 12], np.stack([f, np.roll(f, 3)]), [1.0, 2.0], [4.0, 3.0], 4)
    # joint 1 does not move on segment 1, joint 2 never moves
    w = np.array([[0.0, 0.0, 0.3], [1.0, 0.5, 0.3], [2.0, 0.5, 0.3], [2.5, 1.5, 0.3]])
    out["still"] = _case(np.stack([w, w]), [4, 4], [[0, 0.25, 0.5, 0], [0, 0.0, 0.0, 0]], [1, 1, 1], [2, 2, 2], 4)
    # joint 0 reverses exactly across the blend, m even: q'_0 = 0 at the blend's middle grid point
    w = np.array([[0.0, 0.0], [1.0, 1.0], [0.0, 2.0]])
    out["reversal"] = _case(np.stack([w, w]), [3, 3], [[0, 0.5, 0], [0, 0.25, 0]], [1.5, 1.0], [3.0, 5.0], 4)
    # limits that differ by 1e3 between the joints
    out["limits1e3"] = random_case(60, 6, 5, 2, 3, limits=(np.array([1.0, 1e3]), np.array([1e3, 1.0])))
    # a NaN waypoint and a segment of length zero inside a batch
    c = random_case(70, 7, 5, 3, 3, lengths=(5, 4, 5, 3, 5, 2, 5))
    c["way"][1, 2, 1] = np.nan
    c["way"][3, 2] = c["way"][3, 1]
    c["way"][5, 0, 0] = np.inf
    c["way"][0, 4] = np.nan                                         # past the end of a path of 4 waypoints: not read
    c["length"][0] = 4
    out["bad"] = c
    # a straight move whose grid times are powers of two: x = (0, 4, 0), t = (0, 1/2, 1)
    out["pow2"] = _case([[[0.0], [1.0]], [[3.0], [3.0]]], [2, 1], np.zeros((2, 2)), [1024.0], [4.0], 2)
    return out


def bad_rows():
    """the rows of case `bad` and the status each was built for"""
    return {1: tr.NOT_FINITE, 3: tr.ZERO_SEGMENT, 5: tr.NOT_FINITE}


@functools.lru_cache(maxsize=None)
def law(name):
    """the restatement's time law of a case: computed once, shared, not to be changed"""
    c = cases()[name]
    out = tr.time_law(c["way"], c["length"], c["blend"], c["v"], c["a"], c["m"])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
