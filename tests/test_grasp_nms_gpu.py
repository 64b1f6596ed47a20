"""GPU checks of grasp NMS (gg_grasp_nms, gaussiangrasper_amd.grasp.nms) against the fp64 restatement
(tests/grasp_nms_ref.py).  Every comparison of keep, suppressor, kept and num_kept is equality, and the four outputs
are carved out of sentinel-filled buffers that are compared whole; the workspace holds garbage before every call.
Sizes around every 64-position word and the 256-row tile of the pair kernel; chains of suppression across words and
blocks; translations and rotations exactly on their limits; the half-turn symmetry; rows and order entries that are
data, not errors; the degenerate limits; run-to-run identity; and grasp.nms and grasp_object end to end."""
import ctypes
import math

import numpy as np
import pytest
import torch

from grasp_nms_ref import all_pairs, clustered_rows, restate
from grasp_propose_ref import box_faces
from grasp_ref import grasp_rows, rotation

gpu = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64
S8, S32 = 0xA5, -77
COS30 = math.cos(math.pi / 6)


def call(g, order, translation, cos_rotation, symmetric, garbage=0):
    """One gg_grasp_nms call; returns the four output buffers WHOLE (PAD sentinels either side) as numpy."""
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    g = np.ascontiguousarray(g, np.float32).reshape(-1, 17)
    order = np.ascontiguousarray(order, np.int32).reshape(-1)
    m, a = len(g), len(order)
    gd, od = torch.from_numpy(g).to(DEV), torch.from_numpy(order).to(DEV)
    keep = torch.full((m + 2 * PAD,), S8, dtype=torch.uint8, device=DEV)
    sup = torch.full((m + 2 * PAD,), S32, dtype=torch.int32, device=DEV)
    kept = torch.full((a + 2 * PAD,), S32, dtype=torch.int32, device=DEV)
    num = torch.full((1 + 2 * PAD,), S32, dtype=torch.int32, device=DEV)
    need = lib.gg_grasp_nms_workspace(a)
    assert need > 0 and need % 256 == 0
    gen = torch.Generator(device=DEV).manual_seed(1234 + garbage)
    ws = torch.randint(0, 256, (need,), dtype=torch.uint8, device=DEV, generator=gen)
    p = ctypes.c_void_p
    st = lib.gg_grasp_nms(m, p(gd.data_ptr()), a, p(od.data_ptr()), float(translation), float(cos_rotation),
                          int(symmetric), p(keep.data_ptr() + PAD), p(sup.data_ptr() + 4 * PAD),
                          p(kept.data_ptr() + 4 * PAD), p(num.data_ptr() + 4 * PAD), p(ws.data_ptr()), need,
                          p(torch.cuda.current_stream().cuda_stream))
    assert st == 0, lib.gg_last_error()
    torch.cuda.synchronize()
    return dict(keep=keep.cpu().numpy(), suppressor=sup.cpu().numpy(), kept=kept.cpu().numpy(),
                num_kept=num.cpu().numpy())


def padded(ref):
    """the restatement's outputs inside the same sentinels"""
    def wrap(a, dtype, s):
        return np.concatenate([np.full(PAD, s, dtype), np.asarray(a, dtype).reshape(-1), np.full(PAD, s, dtype)])
    return dict(keep=wrap(ref["keep"], np.uint8, S8), suppressor=wrap(ref["suppressor"], np.int32, S32),
                kept=wrap(ref["kept"], np.int32, S32), num_kept=wrap([ref["num_kept"]], np.int32, S32))


def check(g, order, translation, cos_rotation, symmetric=True):
    """the call equals the restatement, sentinels included; returns the restatement"""
    ref = restate(g, order, translation, cos_rotation, symmetric)
    got, want = call(g, order, translation, cos_rotation, symmetric), padded(ref)
    for k in ("keep", "suppressor", "kept", "num_kept"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    return ref


# ------------------------------------------------------------------------------------------------
# sizes
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("a", [0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 4097])
def test_exact_against_the_restatement(a):
    """M > num_order, the order a random permutation (not by score); 4097 crosses the 256-row tiles, the 4-word
    groups of the pair kernel and the 64 words of the walk's first wave"""
    rng = np.random.default_rng(100 + a)
    m = a + 37
    g = clustered_rows(rng, m, max(2, m // 8), spread_t=0.012, spread_r=0.3)
    order = rng.permutation(m)[:a]
    for sym in ((True, False) if a <= 1000 else (True,)):
        ref = check(g, order, 0.014, math.cos(0.3), sym)
        outside = np.setdiff1d(np.arange(m), order)
        assert (ref["suppressor"][outside] == -2).all() and not ref["keep"][outside].any()
        if a >= 63:                              # the case has substance
            assert a / 5 <= ref["num_kept"] <= 4 * a / 5


# ------------------------------------------------------------------------------------------------
# chains
# ------------------------------------------------------------------------------------------------
@gpu
def test_chains_across_words_and_blocks():
    a = 4100
    t = np.zeros((a, 3))
    t[:, 2] = 1024.0 + 16.0 * np.arange(a)                    # everyone far from everyone
    t[0] = (0.0, 0.0, 0.0)
    t[64] = (0.875, 0.0, 0.0)                                 # near position 0: suppressed
    t[65] = (0.5, 0.0, 0.0)
    t[4096] = (0.625, 0.0, 0.0)
    t[130] = (1.75, 0.0, 0.0)                                 # near position 64 only, which is suppressed: kept
    t[1] = (0.0, 128.0, 0.0)
    t[70] = (1.5, 128.0, 0.0)                                 # far from position 1: kept
    t[129] = (0.75, 128.0, 0.0)                               # near both: position 1 comes first
    rng = np.random.default_rng(11)
    m = a + 5
    row_of = rng.permutation(m)[:a]                           # position -> row
    g = grasp_rows(np.stack([np.eye(3)] * m), np.full((m, 3), -5000.0), 0.05, 0.02, 0.02)
    g[row_of, 13:16] = t
    ref = check(g, row_of, 1.0, 0.5)
    sup, keep = ref["suppressor"], ref["keep"]
    for p in (64, 65, 4096):
        assert sup[row_of[p]] == row_of[0] and not keep[row_of[p]]
    assert keep[row_of[130]] and keep[row_of[1]] and keep[row_of[70]] and keep[row_of[0]]
    assert sup[row_of[129]] == row_of[1] and ref["num_kept"] == a - 4


@gpu
def test_all_identical_and_all_far():
    rng = np.random.default_rng(12)
    R = rotation(rng, 1)
    g = grasp_rows(np.concatenate([R] * 200), np.tile([[0.1, -0.2, 0.3]], (200, 1)), 0.05, 0.02, 0.02)
    order = rng.permutation(200)
    ref = check(g, order, 0.03, COS30)
    assert ref["num_kept"] == 1 and ref["keep"][order[0]]
    assert (np.delete(ref["suppressor"], order[0]) == order[0]).all()
    g = grasp_rows(rotation(rng, 300), np.arange(900).reshape(300, 3), 0.05, 0.02, 0.02)
    order = rng.permutation(300)
    ref = check(g, order, 0.03, COS30)
    assert ref["num_kept"] == 300 and np.array_equal(ref["kept"], order) and (ref["suppressor"] == -1).all()


# ------------------------------------------------------------------------------------------------
# exact boundaries
# ------------------------------------------------------------------------------------------------
def _proper_axis_rotations():
    out = []
    for perm in ([0, 1, 2], [1, 2, 0], [2, 0, 1], [1, 0, 2], [0, 2, 1], [2, 1, 0]):
        for s in range(8):
            R = np.zeros((3, 3))
            R[np.arange(3), perm] = [1 - 2 * ((s >> k) & 1) for k in range(3)]
            if np.linalg.det(R) > 0:
                out.append(R)
    assert len(out) == 24
    return np.stack(out)


@gpu
def test_pairs_exactly_on_both_limits_are_near():
    """translations on a lattice of multiples of 2^-7 with translation = 2^-5: dd == translation^2 is hit exactly
    (offsets (4, 0, 0)); quarter turns about the coordinate axes with cos_rotation = 0: tr == 1 is hit exactly"""
    rng = np.random.default_rng(13)
    m = 400
    Rs = _proper_axis_rotations()
    g = grasp_rows(Rs[rng.integers(0, 24, m)], rng.integers(0, 7, size=(m, 3)) * 2.0 ** -7, 0.05, 0.02, 0.02)
    tt = (2.0 ** -5) ** 2
    for sym in (False, True):
        p = all_pairs(g, 2.0 ** -5, 0.0, sym)
        iu = np.triu_indices(m, 1)
        on_t = (p["dd"] == tt)[iu]
        rot_ok = ((p["tr"] >= 1.0) | ((p["trs"] >= 1.0) & sym))[iu]
        on_r = ((p["tr"] == 1.0) & ((p["trs"] < 1.0) | (not sym)))[iu]          # near by tr == bound alone
        assert (on_t & rot_ok).sum() > 100 and (on_r & (p["dd"] <= tt)[iu]).sum() > 100
        assert (on_t & on_r).sum() > 10                                          # on both at once
        assert p["near"][iu][on_t & rot_ok].all() and p["near"][iu][on_r & (p["dd"] <= tt)[iu]].all()
        ref = check(g, rng.permutation(m), 2.0 ** -5, 0.0, sym)
        assert 10 < ref["num_kept"] < m - 10
    # one ulp under either limit, the pairs on it are no longer near
    fewer = all_pairs(g, np.nextafter(2.0 ** -5, 0), 0.0, True)["near"].sum()
    assert fewer < all_pairs(g, 2.0 ** -5, 0.0, True)["near"].sum()
    check(g, np.arange(m), np.nextafter(2.0 ** -5, 0), 0.0, True)
    check(g, np.arange(m), 2.0 ** -5, 2.0 ** -53, True)          # bound = 1 + 2^-52


# ------------------------------------------------------------------------------------------------
# symmetry, and rows that are data
# ------------------------------------------------------------------------------------------------
@gpu
def test_half_turn_twins_with_and_without_symmetry():
    rng = np.random.default_rng(14)
    R = rotation(rng, 150)
    t = rng.uniform(-0.2, 0.2, size=(150, 3))
    g = np.concatenate([grasp_rows(R, t, 0.05, 0.02, 0.02), grasp_rows(R * np.array([1.0, -1.0, -1.0]), t, 0.05,
                                                                      0.02, 0.02)])
    order = rng.permutation(300)
    with_sym, without = check(g, order, 0.001, math.cos(0.1), True), check(g, order, 0.001, math.cos(0.1), False)
    assert with_sym["num_kept"] == 150 and without["num_kept"] == 300
    twin = (np.arange(300) + 150) % 300
    s = ~with_sym["keep"]
    assert np.array_equal(with_sym["suppressor"][s], twin[s])
    g = clustered_rows(rng, 500, 30, spread_t=0.012, spread_r=0.3, twins=True)
    order = rng.permutation(500)
    assert check(g, order, 0.014, math.cos(0.3), True)["num_kept"] < check(g, order, 0.014, math.cos(0.3),
                                                                         False)["num_kept"]


@gpu
def test_rows_and_entries_that_take_no_part():
    rng = np.random.default_rng(15)
    m = 400
    g = clustered_rows(rng, m, 30, spread_t=0.012, spread_r=0.3)
    bad = rng.permutation(m)[:40]
    for k, r in enumerate(bad):
        g[r, 4 + k % 12] = (np.nan, np.inf, -np.inf)[k % 3]
    g[rng.permutation(m)[:20], 0] = np.nan                    # the score, width, ... are not read
    g[rng.permutation(m)[:20], 1:4] = np.inf
    order = rng.permutation(m)[:330].astype(np.int64)
    clean = order.copy()
    junk = [-1, m, m + 100, -2 ** 31, 2 ** 31 - 1, -7]
    where = np.sort(rng.permutation(330)[:len(junk)])
    order = np.insert(order, where, junk)
    assert np.isin(bad, order).sum() > 20
    ref = check(g, order, 0.014, math.cos(0.3))
    assert (ref["suppressor"][bad] == -2).all() and not ref["keep"][bad].any()
    # the neighbours are unaffected: the same rows without the junk entries and without the bad rows
    ref2 = check(g, clean[~np.isin(clean, bad)], 0.014, math.cos(0.3))
    assert np.array_equal(ref["keep"], ref2["keep"]) and np.array_equal(ref["suppressor"], ref2["suppressor"])
    assert 50 < ref["num_kept"] < 250
    # nobody takes part
    g[:, 13] = np.nan
    assert check(g, order, 0.014, math.cos(0.3))["num_kept"] == 0
    # no grasps at all, entries all out of range
    assert check(np.zeros((0, 17), np.float32), [0, 1, -1], 0.014, 0.5)["num_kept"] == 0


@gpu
def test_degenerate_limits():
    rng = np.random.default_rng(16)
    base = clustered_rows(rng, 150, 12, spread_t=0.012, spread_r=0.3)
    g = np.concatenate([base, base[:100]])                    # 100 exact duplicates
    order = rng.permutation(250)
    r0 = check(g, order, 0.0, math.cos(0.3))
    assert r0["num_kept"] == 150                              # translation 0: only the duplicates go
    check(g, order, 0.0, math.cos(0.3), False)
    everything = check(g, order, 0.014, -1.0, False)          # every rotation is near: translation alone decides
    assert everything["num_kept"] < check(g, order, 0.014, math.cos(0.3), False)["num_kept"]
    far = check(g, order, 1e6, -1.0, False)
    assert far["num_kept"] == 1
    check(g, order, 0.014, 1.0, True)                         # cos_rotation 1: tr >= 3
    check(g, order, 1e6, 1.0, False)


@gpu
def test_two_calls_give_identical_bytes_whatever_the_workspace_held():
    rng = np.random.default_rng(17)
    g = clustered_rows(rng, 1500, 100, spread_t=0.012, spread_r=0.3)
    order = rng.permutation(1500)[:1300]
    a = call(g, order, 0.014, math.cos(0.3), True, garbage=1)
    b = call(g, order, 0.014, math.cos(0.3), True, garbage=2)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------------------------------------
# through Python
# ------------------------------------------------------------------------------------------------
H = 2.0 ** -7


def _two_box_scene():
    """Box A on a table with box B beside it, as flat discs whose smallest axis is the face normal: a few hundred
    Gaussians on a grid of pitch 2^-7.  Returns (Scene, object mask of A (N,) bool)."""
    from gaussiangrasper_amd.scene import make_scene
    pa, na = box_faces([8 * H, 6 * H, 7 * H], H, (0.0, 0.0, 3.5 * H))
    pb, nb = box_faces([6 * H, 6 * H, 3 * H], H, (8 * H, 0.0, 1.5 * H))
    gx = np.arange(-12, 13) * H
    tx, ty = (a.ravel() for a in np.meshgrid(gx, gx, indexing="ij"))
    pt = np.stack([tx, ty, np.full_like(tx, -0.25 * H)], 1)
    nt = np.tile([0.0, 0.0, 1.0], (len(pt), 1))
    p, n = np.concatenate([pa, pb, pt]), np.concatenate([na, nb, nt])
    sc = make_scene(len(p), feature_dim=32)
    r = math.sqrt(0.5)
    quat = np.zeros((len(p), 4))
    ax = np.abs(n).argmax(1)
    quat[ax == 2] = (1.0, 0.0, 0.0, 0.0)
    quat[ax == 0] = (r, 0.0, r, 0.0)
    quat[ax == 1] = (r, -r, 0.0, 0.0)
    sc.means = torch.from_numpy(p.astype(np.float32))
    sc.quats = torch.from_numpy(quat.astype(np.float32))
    sc.scales = torch.log(torch.tensor([0.004, 0.004, 0.0004])).expand(len(p), 3).contiguous()
    sc.opacities = torch.full((len(p), 1), 4.0)
    mask = np.zeros(len(p), bool)
    mask[:len(pa)] = True
    return sc.to(DEV), torch.from_numpy(mask).to(DEV)


def _expected_order(rows, active):
    s = rows[:, 0]
    idx = np.nonzero(active & ~np.isnan(s))[0]
    return idx[np.argsort(-s[idx], kind="stable")]


@gpu
def test_nms_on_proposer_output_equals_the_restatement():
    from gaussiangrasper_amd import grasp
    from gaussiangrasper_amd.grasp_propose import propose_grasps
    sc, mask = _two_box_scene()
    rows = propose_grasps(sc, mask, num_approach=8)
    rows_np = rows.cpu().numpy()
    m = len(rows_np)
    assert 500 < m < 5000
    rng = np.random.default_rng(18)
    active = rng.random(m) < 0.7
    for act, kw in ((None, {}), (active, {}), (active, dict(symmetric=False, rotation=0.2, translation=0.01)),
                    (active, dict(max_candidates=300)), (active, dict(scale=0.5))):
        rec = grasp.nms(rows, None if act is None else torch.from_numpy(act).to(DEV), **kw)
        order = _expected_order(rows_np, np.ones(m, bool) if act is None else act)[:kw.get("max_candidates", 16384)]
        ref = restate(rows_np, order, kw.get("translation", 0.03) * kw.get("scale", 1.0),
                      math.cos(kw.get("rotation", math.pi / 6)), kw.get("symmetric", True))
        assert rec.keep.dtype == torch.bool and rec.suppressor.dtype == torch.int32
        assert rec.order.dtype == torch.int64 and rec.support.dtype == torch.int32
        assert np.array_equal(rec.keep.cpu().numpy(), ref["keep"])
        assert np.array_equal(rec.suppressor.cpu().numpy(), ref["suppressor"])
        assert np.array_equal(rec.order.cpu().numpy(), ref["kept"][:ref["num_kept"]])
        sup = ref["suppressor"]
        support = np.where(ref["keep"], 1 + np.bincount(sup[sup >= 0], minlength=m), 0)
        assert np.array_equal(rec.support.cpu().numpy(), support) and support.sum() == len(order)
        print(kw, len(order), ref["num_kept"])
        if not kw:
            assert 1 < ref["num_kept"] < len(order) / 4      # the proposer's rows are many copies of few grasps
    # with every row's half-turn twin appended (b -> -b, c -> -c: columns 1 and 2 of R), symmetry keeps the same rows:
    # tr and tr_s change places exactly, so a twin is near whatever its original is near, and comes after it
    twins = rows.clone()
    twins[:, [5, 8, 11, 6, 9, 12]] *= -1.0
    assert torch.equal(grasp.nms(torch.cat([rows, twins])).order, grasp.nms(rows).order)
    # a GraspContacts as `active`: its .feasible
    res = grasp.GraspContacts(*(torch.zeros(m, device=DEV) for _ in range(6)),
                              feasible=torch.from_numpy(active).to(DEV))
    assert torch.equal(grasp.nms(rows, res).keep, grasp.nms(rows, res.feasible).keep)
    empty = grasp.nms(rows[:0])
    assert empty.keep.shape == (0,) and empty.order.shape == (0,) and empty.support.shape == (0,)
    none = grasp.nms(rows, torch.zeros(m, dtype=torch.bool, device=DEV))
    assert not none.keep.any() and (none.suppressor == -2).all() and none.order.numel() == 0


@gpu
def test_grasp_object_with_nms_and_top_k():
    from gaussiangrasper_amd.grasp_propose import grasp_object
    sc, mask = _two_box_scene()
    rows0, res0, keep0 = grasp_object(sc, mask, num_approach=8)
    rows1, res1, keep1 = grasp_object(sc, mask, num_approach=8)
    assert res0.nms is None and torch.equal(rows0, rows1) and torch.equal(keep0, keep1)
    assert torch.equal(res0.feasible, res1.feasible) and torch.equal(res0.contact_idx, res1.contact_idx)
    assert keep0.numel() > 20
    rows, res, keep = grasp_object(sc, mask, num_approach=8, nms_translation=0.03, top_k=5)
    assert torch.equal(rows, rows0) and torch.equal(res.feasible, res0.feasible) and res.nms is not None
    k, k0 = keep.cpu().numpy(), keep0.cpu().numpy()
    assert 1 <= len(k) <= 5 and keep.dtype == torch.int64
    it = iter(k0.tolist())
    assert all(any(x == y for y in it) for x in k.tolist())                 # a subsequence of keep0
    near = all_pairs(rows.cpu().numpy()[k], 0.03, COS30, True)["near"]
    assert not (near & ~np.eye(len(k), dtype=bool)).any()                   # pairwise not near
    assert np.array_equal(res.nms.order.cpu().numpy()[:5], k) and k[0] == k0[0]
    assert res.nms.keep.sum().item() == len(res.nms.order) and res.nms.support.sum().item() == len(k0)
    ref = restate(rows.cpu().numpy(), k0, 0.03, COS30, True)
    assert np.array_equal(res.nms.keep.cpu().numpy(), ref["keep"])
    assert np.array_equal(res.nms.suppressor.cpu().numpy(), ref["suppressor"])
    _, _, keep_all = grasp_object(sc, mask, num_approach=8, nms_translation=0.03)
    assert torch.equal(keep_all, res.nms.order)
