"""GPU checks of the arm's self-collision and motion tests (gg_arm_self, gg_arm_motion and the task layer of
gaussiangrasper_amd.arm built on them) against the restatement (tests/arm_motion_ref.py).  The C calls' arrays are
carved from the sentinel arena (tests/arena.py) and compared whole.  The fixtures' own claims (no centre near a cell
face, no sweep bound near a multiple of res, no smallest gap with a close runner-up) are established on the CPU in
tests/test_arm_motion_host.py."""
import ctypes

import numpy as np
import pytest
import torch

import arm_motion_ref as mref
import arm_ref as ref
from arena import Arena

gpu = pytest.mark.gpu
DEV = "cuda:0"
D = ctypes.c_double
FAR = ref.FAR
INT32_MIN = ref.INT32_MIN
OUTS = (("samples", np.int32, ()), ("slack", np.int32, ()), ("slack_at", np.int32, ()), ("worst", np.int32, ()),
        ("gap", np.float64, ()), ("gap_at", np.int32, ()), ("pair", np.int32, (2,)))


def _lib():
    from gaussiangrasper_amd import _lib as L
    return L.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _host(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def c_self(arm, J, q, spheres, frame, radius, pairs, seed=0, sentinel=0xA5):
    q = np.asarray(q, np.float64).reshape(-1, J)
    spheres = np.asarray(spheres, np.float32).reshape(-1, 3)
    M, S = len(q), len(spheres)
    keep, ap = _host(arm, np.float64)
    keep2, pp = _host(pairs, np.uint8)
    ar = Arena(DEV, seed, sentinel)
    ar.carve("q", q, 8, "in")
    if S:
        ar.carve("spheres", spheres, 4, "in")
        ar.carve("frame", np.asarray(frame, np.int32).reshape(S), 4, "in")
        ar.carve("radius", np.asarray(radius, np.float64).reshape(S), 8, "in")
    ar.carve("gap", np.zeros(M), 8, "out")
    ar.carve("pair", np.zeros((M, 2), np.int32), 4, "out")
    n = None
    st = _lib().gg_arm_self(J, ap, M, ar.ptr("q"), S, ar.ptr("spheres") if S else n, ar.ptr("frame") if S else n,
                            ar.ptr("radius") if S else n, pp, ar.ptr("gap"), ar.ptr("pair"), _stream())
    assert st == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    out = ar.check()
    return out["gap"], out["pair"]


def c_motion(arm, J, field, q_a, q_b, spheres, frame, need, outside, radius, pairs, reach, res, max_samples=4096, seed=0,
             sentinel=0xA5):
    """field: None or (dims, grid, dist2); pairs: None or the table"""
    q_a = np.asarray(q_a, np.float64).reshape(-1, J)
    q_b = np.asarray(q_b, np.float64).reshape(-1, J)
    spheres = np.asarray(spheres, np.float32).reshape(-1, 3)
    E, S = len(q_a), len(spheres)
    keep, ap = _host(arm, np.float64)
    keep2, pp = (None, None) if pairs is None else _host(pairs, np.uint8)
    ar = Arena(DEV, seed, sentinel)
    if field is not None:
        ar.carve("dist2", np.asarray(field[2], np.int32).reshape(tuple(field[0])), 4, "in")
    ar.carve("q_a", q_a, 8, "in")
    ar.carve("q_b", q_b, 8, "in")
    if S:
        ar.carve("spheres", spheres, 4, "in")
        ar.carve("frame", np.asarray(frame, np.int32).reshape(S), 4, "in")
        ar.carve("reach", np.asarray(reach, np.float64).reshape(J, S), 8, "in")
        if field is not None:
            ar.carve("need", np.asarray(need, np.int32).reshape(S), 4, "in")
        if pairs is not None:
            ar.carve("radius", np.asarray(radius, np.float64).reshape(S), 8, "in")
    for name, dtype, tail in OUTS:
        ar.carve(name, np.zeros((E,) + tail, dtype), 8 if dtype == np.float64 else 4, "out")
    n = None
    dims = None if field is None else (ctypes.c_int32 * 3)(*[int(d) for d in field[0]])
    grid = None if field is None else (D * 4)(*field[1])
    st = _lib().gg_arm_motion(J, ap, dims, grid, ar.ptr("dist2") if field is not None else n, E, ar.ptr("q_a"),
                              ar.ptr("q_b"), S, ar.ptr("spheres") if S else n, ar.ptr("frame") if S else n,
                              ar.ptr("need") if S and field is not None else n, int(outside),
                              ar.ptr("radius") if S and pairs is not None else n, pp, ar.ptr("reach") if S else n,
                              D(res), int(max_samples), *[ar.ptr(name) for name, _, _ in OUTS], _stream())
    assert st == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    return ar.check()


def c_clear(arm, J, dims, grid, dist2, q, spheres, frame, need, outside, seed=0):
    q = np.asarray(q, np.float64).reshape(-1, J)
    M, S = len(q), len(spheres)
    keep, ap = _host(arm, np.float64)
    ar = Arena(DEV, seed)
    ar.carve("dist2", np.asarray(dist2, np.int32).reshape(tuple(dims)), 4, "in")
    ar.carve("q", q, 8, "in")
    ar.carve("spheres", np.asarray(spheres, np.float32), 4, "in")
    ar.carve("frame", np.asarray(frame, np.int32), 4, "in")
    ar.carve("need", np.asarray(need, np.int32), 4, "in")
    ar.carve("slack", np.zeros(M, np.int32), 4, "out")
    ar.carve("worst", np.zeros(M, np.int32), 4, "out")
    st = _lib().gg_arm_clear(J, ap, (ctypes.c_int32 * 3)(*[int(d) for d in dims]), (D * 4)(*grid), ar.ptr("dist2"), M,
                             ar.ptr("q"), S, ar.ptr("spheres"), ar.ptr("frame"), ar.ptr("need"), int(outside),
                             ar.ptr("slack"), ar.ptr("worst"), _stream())
    assert st == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    out = ar.check()
    return out["slack"], out["worst"]


def check_motion(got, want, rows=slice(None)):
    for name in ("samples", "slack", "slack_at", "worst", "gap_at", "pair"):
        g, w = got[name], want[name][rows]
        assert g.dtype == np.int32 and np.array_equal(g, w), (name, np.nonzero((g != w).reshape(len(g), -1).any(1))[0][:8])
    g, w = got["gap"], want["gap"][rows]
    assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isinf(g), np.isinf(w))
    fin = np.isfinite(w)
    assert np.array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)])
    dev = float(np.abs(g[fin] - w[fin]).max()) if fin.any() else 0.0
    assert dev <= 1e-12, dev
    return dev


# ------------------------------------------------------------------------------------------------
# self
# ------------------------------------------------------------------------------------------------
CHAINS = {1: lambda: ref.random_chain(1, 4), 2: lambda: ref.random_chain(2, 6, prismatic=(1,)), 7: ref.default_chain,
          8: lambda: ref.random_chain(8, 5, prismatic=(2, 6))}


def _tables(J):
    a = np.arange(J + 2)
    return {"zero": np.zeros((J + 2, J + 2), np.uint8), "one": np.ones((J + 2, J + 2), np.uint8),
            "apart": (np.abs(a[:, None] - a[None, :]) >= 2).astype(np.uint8)}


@gpu
@pytest.mark.parametrize("S", [0, 1, 2, 63, 64, 65, 256])
@pytest.mark.parametrize("J", [1, 2, 7, 8])
def test_self_matches_the_restatement(J, S):
    """gap within 1e-12 (centres of at most 9 composed transforms below a metre, one square root), pair equal: with
    random spheres the runner-up of a smallest gap is some 1e-5 away"""
    arm, _ = CHAINS[J]()
    rng = np.random.default_rng(100 * J + S)
    spheres = rng.uniform(-0.2, 0.2, size=(S, 3)).astype(np.float32)
    frame = rng.integers(0, J + 2, size=S).astype(np.int32)
    radius = rng.uniform(0.0, 0.08, size=S)
    worst = 0.0
    for name, table in _tables(J).items():
        for M in (1, 65, 257):
            q = ref.in_limits(arm, J, M, rng, inset=0.0)
            if M > 1:
                q[M // 2, J - 1] = np.nan            # a row that is not finite: NaN and (-1, -1), the neighbours untouched
            want = mref.self_gap(arm, J, q, spheres, frame, radius, table)
            gap, pair = c_self(arm, J, q, spheres, frame, radius, table, seed=M)
            assert gap.shape == (M,) and pair.shape == (M, 2) and pair.dtype == np.int32
            assert np.array_equal(pair, want[1]), (name, M, np.nonzero((pair != want[1]).any(1))[0][:8])
            assert np.array_equal(np.isnan(gap), np.isnan(want[0])) and np.array_equal(np.isinf(gap), np.isinf(want[0]))
            fin = np.isfinite(want[0])
            if fin.any():
                worst = max(worst, np.abs(gap[fin] - want[0][fin]).max())
            if M > 1:
                assert np.isnan(gap[M // 2]) and pair[M // 2].tolist() == [-1, -1]
            none = name == "zero" or S < 2 or (name == "apart" and not table[frame[:, None], frame[None, :]].any())
            if none:                                 # no tested pair: +inf and (-1, -1)
                rows = np.isfinite(q).all(1)
                assert np.isposinf(gap[rows]).all() and (pair[rows] == -1).all()
    print(f"gg_arm_self J={J} S={S}: max |device - restatement| = {worst:.3e}")
    assert worst <= 1e-12


@gpu
def test_self_lowest_pair_wins_a_tie():
    arm, J = ref.default_chain()
    rng = np.random.default_rng(5)
    S = 70
    spheres = rng.uniform(-0.1, 0.1, size=(S, 3)).astype(np.float32)
    frame = rng.integers(0, J + 2, size=S).astype(np.int32)
    radius = rng.uniform(0.0, 0.03, size=S)
    # two identical spheres, so large that every smallest gap is theirs; their own frame's pairs are not tested, so
    # (9, t) and (66, t) tie for every t, and with t* the partner: (9, t*) when t* > 9, else (t*, 9)
    spheres[[9, 66]] = spheres[9]
    frame[[9, 66]] = 3
    radius[[9, 66]] = 5.0
    table = np.ones((J + 2, J + 2), np.uint8) - np.eye(J + 2, dtype=np.uint8)
    q = ref.in_limits(arm, J, 65, rng)
    gap, pair = c_self(arm, J, q, spheres, frame, radius, table, seed=1)
    want = mref.self_gap(arm, J, q, spheres, frame, radius, table)
    assert np.array_equal(pair, want[1]) and np.abs(gap - want[0]).max() <= 1e-12
    assert ((pair == 9).sum(1) == 1).all() and not (pair == 66).any() and (gap < -4.0).all()
    # three of them, their frame tested against itself: (9, 30), (9, 66), (30, 66) tie exactly, at -2 r
    spheres[30], frame[30], radius[30] = spheres[9], 3, 5.0
    gap, pair = c_self(arm, J, q, spheres, frame, radius, np.ones((J + 2, J + 2), np.uint8), seed=2)
    assert (pair == [9, 30]).all() and (gap == -10.0).all()


# ------------------------------------------------------------------------------------------------
# motion
# ------------------------------------------------------------------------------------------------
def _run_fixture(f, rows, field=True, pairs=True, seed=0, sentinel=0xA5):
    return c_motion(f["arm"], f["J"], (f["dims"], f["grid"], f["dist2"]) if field else None, f["q_a"][rows],
                    f["q_b"][rows], f["spheres"], f["frame"], f["need"], FAR, f["radius"],
                    f["pairs"] if pairs else None, f["reach"], f["res"], seed=seed, sentinel=sentinel)


@gpu
@pytest.mark.parametrize("E", [1, 63, 65, 257])
@pytest.mark.parametrize("which", ["default", "prismatic"])
def test_motion_edge_fixture(which, E):
    """the first E edges of the fixture: n cycles through 1, 2, 3, 63, 64, 65, 200"""
    f = mref.edge_fixture(which)
    rows = slice(0, E)
    got = _run_fixture(f, rows, seed=E)
    dev = check_motion(got, f["want"], rows)
    print(f"gg_arm_motion {which} E={E}: max |gap_device - gap_restatement| = {dev:.3e}")


@gpu
def test_motion_without_field_or_pairs_or_spheres():
    f = mref.edge_fixture("default")
    rows = slice(0, 65)
    want = f["want"]
    n = want["samples"][rows]
    # dist2 null: no field test; the gap outputs are what they were
    got = _run_fixture(f, rows, field=False, seed=1)
    assert np.array_equal(got["samples"], n) and (got["slack"] == FAR).all()
    assert (got["slack_at"] == -1).all() and (got["worst"] == -1).all()
    assert np.array_equal(got["gap_at"], want["gap_at"][rows]) and np.array_equal(got["pair"], want["pair"][rows])
    assert np.abs(got["gap"] - want["gap"][rows]).max() <= 1e-12
    # pairs null: no self test; the field outputs are what they were
    got = _run_fixture(f, rows, pairs=False, seed=2)
    assert np.array_equal(got["samples"], n) and np.isposinf(got["gap"]).all()
    assert (got["gap_at"] == -1).all() and (got["pair"] == -1).all()
    for name in ("slack", "slack_at", "worst"):
        assert np.array_equal(got[name], want[name][rows])
    # neither
    got = _run_fixture(f, rows, field=False, pairs=False, seed=3)
    assert np.array_equal(got["samples"], n) and (got["slack"] == FAR).all() and np.isposinf(got["gap"]).all()
    # a table that tests nothing: +inf at every sample, so the first one, and no pair
    got = c_motion(f["arm"], f["J"], None, f["q_a"][rows], f["q_b"][rows], f["spheres"], f["frame"], None, FAR,
                   f["radius"], np.zeros_like(f["pairs"]), f["reach"], f["res"], seed=4)
    assert np.isposinf(got["gap"]).all() and (got["gap_at"] == 0).all() and (got["pair"] == -1).all()
    # no spheres: B = 0, n = 1, nothing to hit
    none = np.zeros((0, 3), np.float32)
    got = c_motion(f["arm"], f["J"], (f["dims"], f["grid"], f["dist2"]), f["q_a"][rows], f["q_b"][rows], none,
                   np.zeros(0, np.int32), np.zeros(0, np.int32), FAR, np.zeros(0), f["pairs"], np.zeros((f["J"], 0)),
                   f["res"], seed=5)
    assert (got["samples"] == 1).all() and (got["slack"] == FAR).all() and (got["slack_at"] == 0).all()
    assert (got["worst"] == -1).all() and np.isposinf(got["gap"]).all() and (got["gap_at"] == 0).all()
    assert (got["pair"] == -1).all()


@gpu
def test_motion_edge_cases():
    f = mref.edge_fixture("default")
    arm, J, res = f["arm"], f["J"], f["res"]
    field = (f["dims"], f["grid"], f["dist2"])
    q_a, q_b = f["q_a"][:12].copy(), f["q_b"][:12].copy()
    q_b[0] = q_a[0]                                  # a zero-length edge: n = 1, the two samples alike, both _at 0
    q_a[3, 2] = np.nan                               # ends that are not finite
    q_b[4, 6] = np.inf
    # an edge scaled to just above max_samples res (unresolved) and one to just below it (n = max_samples)
    max_samples = 8
    d = q_b[5] - q_a[5]
    unit = mref.sweep_bound(np.zeros(J), d, f["reach"])
    q_b[5] = q_a[5] + d * (max_samples * res * (1 + 1e-9) / unit)
    q_b[6] = q_a[5] + d * (max_samples * res * (1 - 1e-9) / unit)
    q_a[6] = q_a[5]
    above, below = (mref.sweep_bound(q_a[k], q_b[k], f["reach"]) for k in (5, 6))
    assert above > max_samples * res >= below > (max_samples - 1) * res
    for k in (7, 8, 9, 10, 11):                      # the others short enough for 8 samples: n = 1 .. 5
        q_b[k] = q_a[k] + (q_b[k] - q_a[k]) * ((k - 6.5) * res / mref.sweep_bound(q_a[k], q_b[k], f["reach"]))
    for k in (1, 2):
        q_b[k] = q_a[k] + (q_b[k] - q_a[k]) * (3.5 * res / mref.sweep_bound(q_a[k], q_b[k], f["reach"]))
    want = mref.motion(arm, J, field, q_a, q_b, f["spheres"], f["frame"], f["need"], FAR, f["radius"], f["pairs"],
                       f["reach"], res, max_samples, detail=True)
    assert want["samples"].tolist() == [1, 4, 4, 0, 0, 0, 8, 1, 2, 3, 4, 5]
    assert want["runner_up"][[1, 2, 6, 7, 8, 9, 10, 11]].min() > 1e-9 and want["face"].min() > 1e-9
    got = c_motion(arm, J, field, q_a, q_b, f["spheres"], f["frame"], f["need"], FAR, f["radius"], f["pairs"],
                   f["reach"], res, max_samples, seed=7)
    check_motion(got, want)
    assert got["slack_at"][0] == 0 and got["gap_at"][0] == 0
    for k in (3, 4, 5):
        assert got["samples"][k] == 0 and got["slack"][k] == INT32_MIN and np.isnan(got["gap"][k])
        assert got["slack_at"][k] == got["worst"][k] == got["gap_at"][k] == -1 and got["pair"][k].tolist() == [-1, -1]


@gpu
def test_motion_of_two_samples_is_clear_and_self_at_the_ends():
    """n = 1: the samples are q_a and q_b themselves, and what gg_arm_motion reports is what gg_arm_clear and
    gg_arm_self report there, to the bit"""
    f = mref.edge_fixture("default")
    arm, J = f["arm"], f["J"]
    rows = np.nonzero(f["want"]["samples"] == 1)[0]
    assert len(rows) >= 30
    got = _run_fixture(f, rows, seed=8)
    assert (got["samples"] == 1).all()
    sl, wo, gp, pr = [], [], [], []
    for k, q in enumerate((f["q_a"][rows], f["q_b"][rows])):
        s, w = c_clear(arm, J, f["dims"], f["grid"], f["dist2"], q, f["spheres"], f["frame"], f["need"], FAR, seed=9 + k)
        g, p = c_self(arm, J, q, f["spheres"], f["frame"], f["radius"], f["pairs"], seed=11 + k)
        sl.append(s), wo.append(w), gp.append(g), pr.append(p)
    at = (sl[1] < sl[0]).astype(np.int32)
    assert np.array_equal(got["slack_at"], at) and np.array_equal(got["slack"], np.where(at == 1, sl[1], sl[0]))
    assert np.array_equal(got["worst"], np.where(at == 1, wo[1], wo[0]))
    at = (gp[1] < gp[0]).astype(np.int32)
    assert np.array_equal(got["gap_at"], at)
    assert got["gap"].tobytes() == np.where(at == 1, gp[1], gp[0]).tobytes()
    assert np.array_equal(got["pair"], np.where(at[:, None] == 1, pr[1], pr[0]))


@gpu
def test_motion_gives_the_same_bytes_on_different_garbage():
    f = mref.edge_fixture("prismatic")
    rows = slice(100, 165)
    a = _run_fixture(f, rows, seed=21, sentinel=0xA5)
    b = _run_fixture(f, rows, seed=22, sentinel=0x3C)
    for name, _, _ in OUTS:
        assert a[name].tobytes() == b[name].tobytes(), name


@gpu
def test_refused_and_empty_calls_write_nothing():
    f = mref.edge_fixture("default")
    arm, J, res = f["arm"], f["J"], f["res"]
    S, E = len(f["spheres"]), 5
    keep, ap = _host(arm, np.float64)
    keep2, pp = _host(f["pairs"], np.uint8)
    lib = _lib()
    ar = Arena(DEV, 40)
    ar.carve("dist2", f["dist2"], 4, "in")
    ar.carve("q_a", f["q_a"][:E + 1], 8, "in")
    ar.carve("q_b", f["q_b"][:E + 1], 8, "in")
    ar.carve("spheres", f["spheres"], 4, "in")
    ar.carve("frame", f["frame"], 4, "in")
    ar.carve("need", f["need"], 4, "in")
    ar.carve("radius", f["radius"], 8, "in")
    ar.carve("reach", f["reach"], 8, "in")
    for name, dtype, tail in OUTS:
        ar.carve(name, np.zeros((E,) + tail, dtype), 8 if dtype == np.float64 else 4, "out")
    ar.carve("gap1", np.zeros(E), 8, "out")                         # gg_arm_self's own outputs
    ar.carve("pair1", np.zeros((E, 2), np.int32), 4, "out")
    dims, grid = (ctypes.c_int32 * 3)(*[int(d) for d in f["dims"]]), (D * 4)(*f["grid"])

    def motion(**kw):
        a = dict(dims=dims, grid=grid, dist2=ar.ptr("dist2"), E=E, q_a=ar.ptr("q_a"), q_b=ar.ptr("q_b"), S=S,
                 spheres=ar.ptr("spheres"), frame=ar.ptr("frame"), need=ar.ptr("need"), outside=FAR,
                 radius=ar.ptr("radius"), pairs=pp, reach=ar.ptr("reach"), res=res, max_samples=4096,
                 **{name: ar.ptr(name) for name, _, _ in OUTS})
        a.update(kw)
        return lib.gg_arm_motion(J, ap, a["dims"], a["grid"], a["dist2"], a["E"], a["q_a"], a["q_b"], a["S"],
                                 a["spheres"], a["frame"], a["need"], a["outside"], a["radius"], a["pairs"], a["reach"],
                                 D(a["res"]), a["max_samples"], *[a[name] for name, _, _ in OUTS], _stream())

    def self_(**kw):
        a = dict(M=E, q=ar.ptr("q_a"), S=S, spheres=ar.ptr("spheres"), frame=ar.ptr("frame"), radius=ar.ptr("radius"),
                 pairs=pp, gap=ar.ptr("gap1"), pair=ar.ptr("pair1"))
        a.update(kw)
        return lib.gg_arm_self(J, ap, a["M"], a["q"], a["S"], a["spheres"], a["frame"], a["radius"], a["pairs"],
                               a["gap"], a["pair"], _stream())

    def refused(status, *words):
        msg = lib.gg_last_error()
        assert status == -1 and all(w in msg for w in words), msg

    def odd(name, by):
        return ctypes.c_void_p(ar.address(name) + by)
    refused(motion(q_a=odd("q_a", 4)), b"gg_arm_motion", b"q_a", b"misaligned")
    refused(motion(gap=odd("gap", 4)), b"gap", b"misaligned")
    refused(motion(reach=odd("reach", 4)), b"reach", b"misaligned")
    refused(motion(slack=odd("slack", 2)), b"slack", b"misaligned")
    refused(motion(q_b=None), b"null pointer", b"q_b")
    refused(motion(samples=None), b"null pointer", b"samples")
    refused(motion(reach=None), b"null pointer", b"reach")
    refused(motion(need=None), b"null pointer", b"need2")
    refused(motion(radius=None), b"null pointer", b"radius")
    refused(motion(grid=None), b"null pointer", b"grid")
    refused(motion(res=0.0), b"res")
    refused(motion(res=float("nan")), b"res")
    refused(motion(max_samples=0), b"max_samples")
    refused(motion(max_samples=4097), b"max_samples")
    refused(motion(S=257), b"num_spheres")
    refused(motion(E=-1), b"num_edges")
    refused(motion(outside=-1), b"outside")
    refused(self_(q=odd("q_a", 4)), b"gg_arm_self", b"q", b"misaligned")
    refused(self_(pairs=None), b"null pointer", b"pairs")
    refused(self_(radius=None), b"null pointer", b"radius")
    refused(self_(S=257), b"num_spheres")
    refused(self_(M=-1), b"num_rows")
    bad = arm.copy()
    bad[3] = 0.5
    keep3, bp = _host(bad, np.float64)
    assert lib.gg_arm_self(J, bp, E, ar.ptr("q_a"), S, ar.ptr("spheres"), ar.ptr("frame"), ar.ptr("radius"), pp,
                           ar.ptr("gap1"), ar.ptr("pair1"), _stream()) == -1 and b"base" in lib.gg_last_error()
    # the empty calls
    assert motion(E=0) == 0 and self_(M=0) == 0
    torch.cuda.synchronize()
    assert ar.untouched()
    # and the same arena serves the two calls as they are meant: guards and inputs untouched
    assert motion() == 0 and self_() == 0
    torch.cuda.synchronize()
    out = ar.check()
    check_motion({k: out[k] for k, _, _ in OUTS}, f["want"], slice(0, E))
    want = mref.self_gap(arm, J, f["q_a"][:E], f["spheres"], f["frame"], f["radius"], f["pairs"])
    assert np.abs(out["gap1"] - want[0]).max() <= 1e-12 and np.array_equal(out["pair1"], want[1])


# ------------------------------------------------------------------------------------------------
# the task layer
# ------------------------------------------------------------------------------------------------
H = 0.02
BOX = ((0.1, -0.5, -0.1), (1.0, 0.5, 0.7))
Q_LEFT = np.array([-0.7, 0.5, 0.0, -1.8, 0.0, 2.3, 0.785])
Q_RIGHT = np.array([0.7, 0.5, 0.0, -1.8, 0.0, 2.3, 0.785])


def _block_scene():
    """the default arm at the origin reaching forward, and a block of 7 x 4 x 9 cells where its hand passes when joint 0
    swings from -0.7 to 0.7: either end is clear, the move between them is not"""
    from gaussiangrasper_amd import field
    f = field.DistanceField(*BOX, voxel=H, device=torch.device(DEV))
    f.mass[24:31, 23:27, 13:22] = field.VOTE_ONE
    f.update()
    return f


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV)


@gpu
def test_motion_finds_the_block_between_two_clear_configurations_and_connect_goes_round():
    from gaussiangrasper_amd import arm as A
    model = A.default_arm()
    f = _block_scene()
    ends = A.motion(model, _t([Q_LEFT, Q_RIGHT]), _t([Q_LEFT, Q_RIGHT]), f)
    assert ends.ok.all() and (ends.samples == 1).all()                # each end is clear, inflated by res / 2
    m = A.motion(model, _t([Q_LEFT]), _t([Q_RIGHT]), f)
    n = int(m.samples[0])
    assert not bool(m.ok[0]) and int(m.slack[0]) < 0 and 0 < int(m.slack_at[0]) < n
    assert int(m.worst[0]) >= 13 and float(m.gap[0]) > m.res        # the wrist and hand hit it; the arm misses itself
    # the restatement on the field the device computed
    c, fr, r = model.link_spheres()
    from gaussiangrasper_amd.field import need2
    want = mref.motion(model.to_array(), 7, (f.dims, f.grid, f.dist2.cpu().numpy()), Q_LEFT[None], Q_RIGHT[None], c, fr,
                       need2(r + 0.5 * H, 0.0, H), FAR, r, A.default_self_pairs(model), model.reach_table(), H)
    assert n == want["samples"][0] and int(m.slack[0]) == want["slack"][0] and int(m.slack_at[0]) == want["slack_at"][0]
    # connect: the direct move is refused, a via configuration leads round the block
    con = A.connect(model, Q_LEFT, Q_RIGHT, f)
    route = con.routes[0][0]
    assert con.via[0, 0] >= 0 and route.shape == (3, 7)
    assert np.array_equal(route[0], Q_LEFT) and np.array_equal(route[2], Q_RIGHT)
    assert np.array_equal(route[1], con.vias[con.via[0, 0]])
    legs = A.motion(model, _t(route[:2]), _t(route[1:]), f)
    assert legs.ok.all()
    assert con.cost[0, 0] == np.abs(route[1] - route[0]).max() + np.abs(route[2] - route[1]).max()
    assert not bool(con.motion.ok[0])                                 # edge 0 of the one call is the direct move
    # no cheaper via was clear
    V = len(con.vias)
    ok = con.motion.ok.cpu().numpy()
    cost = np.abs(con.vias - Q_LEFT).max(1) + np.abs(Q_RIGHT - con.vias).max(1)
    both = ok[1:1 + V] & ok[1 + V:]
    assert both[con.via[0, 0]] and cost[both].min() == con.cost[0, 0]
    # between two configurations with nothing in the way: the direct move
    near = Q_LEFT.copy()
    near[0] = -0.5
    con = A.connect(model, Q_LEFT, near, f, num_vias=4)
    assert con.via[0, 0] == -1 and con.routes[0][0].shape == (2, 7) and con.cost[0, 0] == np.abs(near - Q_LEFT).max()


@gpu
def test_an_edge_through_a_self_collision_is_rejected_by_the_gap():
    from gaussiangrasper_amd import arm as A
    model = A.default_arm()
    c, fr, r = model.link_spheres()
    # the wrist folded back onto the forearm: frames 4 and 7, at the end of the edge (their gap depends on joint 5 alone)
    folded = model.home()
    folded[5] = 0.1
    # and a move of joint 4 alone between two clear configurations that swings the hand through the shoulder
    a = np.array([1.02, 1.728, 1.726, -2.864, -1.03, 0.866, -2.304])
    b = a.copy()
    b[4] = 0.67
    m = A.motion(model, _t([model.home(), a]), _t([folded, b]), res=0.02)
    assert not m.ok.any() and (m.slack == FAR).all() and (m.gap < 0).all()
    pair = m.pair.cpu().numpy()
    assert fr[pair[0]].tolist() == [4, 7] and int(m.gap_at[0]) == int(m.samples[0])
    assert fr[pair[1]].tolist() == [1, 7] and 0 < int(m.gap_at[1]) < int(m.samples[1])
    gap, at = A.self_gap(model, _t([model.home(), folded, a, b]))
    assert (gap[[0, 2, 3]] >= 0.02).all() and float(gap[1]) == float(m.gap[0]) and at[1].tolist() == pair[0].tolist()
    want = mref.motion(model.to_array(), 7, None, np.stack([model.home(), a]), np.stack([folded, b]), c, fr, None, FAR, r,
                       A.default_self_pairs(model), model.reach_table(), 0.02)
    assert np.array_equal(m.samples.cpu().numpy(), want["samples"]) and np.array_equal(pair, want["pair"])
    assert np.abs(m.gap.cpu().numpy() - want["gap"]).max() <= 1e-12
    # with the pairs off there is nothing to reject
    assert A.motion(model, _t([a]), _t([b]), res=0.02, pairs=False).ok.all()


def _table_scene():
    """tests/test_arm_gpu.py's table: a slab from x = 0.3 on with its top at z = 0.2, and grasps from above"""
    from gaussiangrasper_amd import field
    f = field.DistanceField(*BOX, voxel=H, device=torch.device(DEV))
    f.mass[10:, :, :15] = field.VOTE_ONE
    f.update()
    down = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float64)
    rows = [np.concatenate([[0.9 - 0.1 * i, 0.06, 0.02, 0.02], down.reshape(-1), [x, y, 0.3], [0.0]])
            for i, (x, y) in enumerate(((0.45, -0.2), (0.5, 0.0), (0.55, 0.15), (0.45, 0.25)))]
    rows.append(np.concatenate([[1.0, 0.06, 0.02, 0.02], down.reshape(-1), [1.5, 0.0, 0.3], [0.0]]))   # out of range
    return f, np.array(rows)


@gpu
def test_reach_without_the_flag_is_what_it_was_and_with_it_drops_seeds():
    from gaussiangrasper_amd import arm as A, field
    model = A.default_arm()
    f, rows = _table_scene()
    poses = torch.from_numpy(field.approach_paths(rows, 0.1, 3)).to(DEV)
    P, W, S, J = 5, 3, A.NUM_SEEDS, 7
    res = A.reach(model, poses, f)
    assert res.motion_ok is None and res.motion_all is None and res.motion is None and res.gap_all is None
    # byte for byte what follow, clear and select give, as reach composed them before there was a motion test
    sd = torch.from_numpy(A.seeds(model, P, S, 0)).to(DEV)
    fol = A.follow(model, poses, sd)
    c, fr, r = model.link_spheres()
    dev = torch.device(DEV)
    sl, wo = A.clear(model, f.dist2, f.grid, f.dims, fol.q.reshape(-1, J), torch.from_numpy(c).to(dev),
                     torch.from_numpy(fr).to(dev), torch.from_numpy(field.need2(r, 0.0, f.h)).to(dev))
    sl, wo = sl.reshape(P, S, W), wo.reshape(P, S, W)
    prev = torch.cat([_t(model.home()).expand(P, S, 1, J), fol.q[:, :, :-1]], 2)
    jump = (fol.q - prev).abs().amax(-1).amax(-1)
    plain_ok = (sl >= 0).all(-1)
    pick, reachable, ok = A.select(fol.first_fail.cpu().numpy(), W, plain_ok.cpu().numpy(), jump.cpu().numpy())
    at = np.maximum(pick, 0)
    ar = np.arange(P)

    def same(t, a):
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()
    same(res.follow.q, fol.q.cpu().numpy()), same(res.follow.first_fail, fol.first_fail.cpu().numpy())
    same(res.slack_all, sl.cpu().numpy()), same(res.worst_all, wo.cpu().numpy())
    same(res.seed, pick), same(res.reachable, reachable), same(res.clear, ok)
    same(res.slack, sl.cpu().numpy()[ar, at]), same(res.worst, wo.cpu().numpy()[ar, at])
    q = fol.q.cpu().numpy()[ar, at]
    q[pick < 0] = np.nan
    same(res.q, q)
    same(res.jump, np.where(pick < 0, np.inf, jump.cpu().numpy()[ar, at]))
    assert reachable.tolist() == [True] * 4 + [False] and ok.tolist() == [True] * 4 + [False]
    # with the flag: the moves between the waypoints and the arm against itself count too
    self_margin = 0.0
    rm = A.reach(model, poses, f, motion=True, self_margin=self_margin)
    same(rm.follow.q, fol.q.cpu().numpy()), same(rm.slack_all, sl.cpu().numpy())
    follows = (fol.first_fail == W)
    kept = plain_ok & follows
    edges_ok, gaps = rm.motion.ok.all(-1), rm.gap_all
    assert rm.motion.ok.shape == (P, S, W - 1) and gaps.shape == (P, S, W)
    assert torch.equal(rm.motion_all, edges_ok & (gaps >= self_margin).all(-1) & follows)
    dropped = kept & ~rm.motion_all
    print(f"reach: {int(kept.sum())} (path, seed) pairs clear at their waypoints, {int(dropped.sum())} of them dropped "
          f"by the motion test, {int(rm.clear.sum())} of {int(res.clear.sum())} paths stay clear")
    assert dropped.any()                                              # a seed that reach keeps and motion drops
    assert ((rm.motion.slack < 0) & (rm.motion.slack_at > 0) & dropped[..., None]).any()    # for what lies between
    pick2, _, ok2 = A.select(fol.first_fail.cpu().numpy(), W, (plain_ok & rm.motion_all).cpu().numpy(),
                             jump.cpu().numpy())
    same(rm.seed, pick2), same(rm.clear, ok2)
    assert not (rm.clear & ~res.clear).any()
    same(rm.motion_ok, rm.motion_all.cpu().numpy()[ar, np.maximum(pick2, 0)] & (pick2 >= 0))
    assert not bool(rm.motion_ok[4])
    # a seed that fails its path has NaN rows: samples 0, not ok
    fails = ~follows
    if fails.any():
        assert not rm.motion_all[fails].any()
    # the edges are gg_arm_motion's of those configurations
    one = A.motion(model, fol.q[0, 0, :-1], fol.q[0, 0, 1:], f, self_margin=self_margin)
    assert torch.equal(one.ok, rm.motion.ok[0, 0]) and torch.equal(one.samples, rm.motion.samples[0, 0])


@gpu
def test_command_line_writes_the_motion_report(tmp_path, capsys):
    from gaussiangrasper_amd import arm as A
    f, rows = _table_scene()
    f.save(str(tmp_path / "field.npz"))
    np.save(tmp_path / "grasps.npy", rows.astype(np.float32))
    np.save(tmp_path / "from.npy", A.default_arm().home())
    out, rep = str(tmp_path / "q.npy"), str(tmp_path / "r.npz")
    rc = A.main(["--arm", "default", "--grasps", str(tmp_path / "grasps.npy"), "--standoff", "0.1", "--steps", "3",
                 "--field", str(tmp_path / "field.npz"), "--check-motion", "--self-margin", "0.005", "--max-samples",
                 "512", "--connect-from", str(tmp_path / "from.npy"), "--out", out, "--report", rep])
    text = capsys.readouterr().out
    assert rc == 0 and "4 of 5 paths reachable" in text and "every move between waypoints clear" in text
    assert "connections found" in text
    q = np.load(out)
    with np.load(rep) as z:
        assert {"reachable", "clear", "seed", "slack", "worst", "jump", "first_fail", "iters", "motion_ok", "samples",
                "gap", "pair", "slack_at", "connect_via", "connect_cost", "connect_waypoints"} <= set(z.files)
        assert z["motion_ok"].shape == (5,) and z["samples"].shape == (5, 2) and z["gap"].shape == (5, 2)
        assert z["pair"].shape == (5, 2, 2) and z["slack_at"].shape == (5, 2)
        assert not z["motion_ok"][4] and (z["samples"][4] == 0).all()
        assert np.array_equal(z["motion_ok"] & z["clear"], z["clear"])        # clear now implies the moves are
        ok = z["motion_ok"]
        assert (z["samples"][ok] >= 1).all() and (z["gap"][ok] >= 0.005 + H).all()
        via, way = z["connect_via"], z["connect_waypoints"]
        assert via.shape == (1, 5) and way.shape == (1, 5, 3, 7) and via[0, 4] == -2
        for p in range(4):
            if via[0, p] != -2:
                assert np.array_equal(way[0, p, 0], A.default_arm().home())
                last = 1 if via[0, p] == -1 else 2
                assert np.array_equal(way[0, p, last], q[p, 0])
    # without --check-motion the report has the keys it had
    rc = A.main(["--arm", "default", "--grasps", str(tmp_path / "grasps.npy"), "--standoff", "0.1", "--steps", "3",
                 "--field", str(tmp_path / "field.npz"), "--out", out, "--report", rep])
    capsys.readouterr()
    with np.load(rep) as z:
        assert set(z.files) == {"reachable", "clear", "seed", "slack", "worst", "jump", "first_fail", "iters"}
    with pytest.raises(SystemExit):
        A.main(["--arm", "default", "--grasps", str(tmp_path / "grasps.npy"), "--standoff", "0.1", "--steps", "3",
                "--check-motion", "--out", out, "--report", rep])
