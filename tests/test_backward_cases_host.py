"""What the constructed backward cases (tests/backward_cases.py) claim about themselves, established with numpy and the
CPU oracle: the survivors a quadrant queues, the distance of every blend decision from its threshold, that no blended
Gaussian has a vanishing reference gradient, and that the reference alone (fp32 against fp64 oracle) stays inside the
criterion the kernels are held to in tests/test_backward_batches.py."""
import numpy as np
import pytest

import backward_cases as B

RTOL, ATOL_FRAC = 5e-5, 1e-6          # the criterion of the blend backward (tests/test_gpu_parity.py test_blend_bwd)


@pytest.fixture(scope="module")
def forwards(oracle):
    return {name: B.forward32(oracle, case) for name, case in B.CASES.items()}


@pytest.mark.parametrize("name", list(B.CASES))
def test_designed_survivor_counts(name, forwards):
    """per (tile, quadrant): designed count == Gaussians centred in the quadrant (the broad ones of the per-pixel fin
    case count for all four quadrants of their tile) == Gaussians with fp64 alpha >= 1/255 on a pixel centre of it"""
    case = B.CASES[name]
    assert (B.quadrant_of(case)[~case.broad] == case.order[~case.broad]).all()
    tiles_x = (case.w + 15) // 16
    centre_tile = (case.xys[:, 0] // 16 + tiles_x * (case.xys[:, 1] // 16)).astype(np.int64)
    assert (centre_tile == case.tile).all()
    reaches = B.alpha64(case) >= B.ALPHA_MIN
    for t, k, r in B.quadrant_views(case, reaches):
        centred = int((((B.quadrant_of(case) == k) | case.broad) & (case.tile == t)).sum())
        reached = int(r.any(axis=(1, 2)).sum())
        assert case.counts[t][k] == centred == reached, (name, t, k, case.counts[t][k], centred, reached)
    assert sum(sum(c) for c in case.counts.values()) == len(case.order) + 3 * int(case.broad.sum())
    assert int(case.tile_bins[-1, 1]) == len(case.order) <= 300


def test_the_cases_are_the_listed_ones():
    one = lambda name: B.CASES[name].counts[0]
    for c in B.EDGES_16 + B.EDGES_32:
        assert one("edges_%d_%d_%d_%d" % c) == c
    for c in B.NARROW_COUNTS:
        assert one("narrow_%d_%d_%d_%d" % c) == c and len(B.CASES["narrow_%d_%d_%d_%d" % c].order) == 64
    for left in (15, 27):
        case = B.CASES["fullest_%d" % left]
        assert (case.order[:64] == 0).all() and case.order[127] == 0 and len(case.order) == 128
        assert int((case.order[64:] == 0).sum()) == left
    case = B.CASES["left_over_260"]
    assert case.counts[0] == (87, 87, 86, 0) and float(case.opacity.max()) <= np.float32(0.08)
    for k in B.CHUNK_LENGTHS:
        assert one("chunk_%d" % k) == (0, k, 0, 0)
    for k in B.TWO_TILE_LENGTHS:
        case = B.CASES["two_tiles_%d" % k]
        assert case.tile_bins.tolist() == [[0, 37], [37, 37 + k]] and (case.h, case.w) == (16, 32)
    case = B.CASES["fin_inside_a_batch"]
    assert case.counts[0] == (60, 8, 8, 8)
    small = np.setdiff1d(np.arange(60), B.FIN_NARROW + B.FIN_BROAD)
    assert float(case.opacity[small].max()) <= np.float32(0.05)


@pytest.mark.parametrize("name", list(B.CASES))
def test_walks_start_where_designed(name, forwards):
    """no pixel saturates outside the per-pixel fin case: the largest final_idx of a quadrant is the position behind its
    last own entry (0 for a quadrant without one: it walks nothing)"""
    case = B.CASES[name]
    _, fi = forwards[name]
    if name == "fin_inside_a_batch":
        assert fi[2, 2] == 26 and (np.delete(fi.ravel(), 2 * 16 + 2) == B.FIN_LAST).all()
        return
    for t, k, f in B.quadrant_views(case, fi[None]):
        own = np.flatnonzero((case.order == k) & (case.tile == t))
        assert f.max() == (own.max() + 1 if own.size else 0), (name, t, k)
    if name.startswith("fullest") or name.startswith("chunk") or name.startswith("two_tiles"):
        assert fi.max() == len(case.order)           # hi = the list's end for the quadrant under test


@pytest.mark.parametrize("name", list(B.CASES))
def test_decisions_keep_their_distance_from_the_thresholds(name):
    """no (pixel, Gaussian) pair within 1e-5 of alpha = 1/255: the fp32 kernels, the fp32 and the fp64 oracle decide every
    pair alike (a condition on the seeds of backward_cases)"""
    d = np.abs(255.0 * B.alpha64(B.CASES[name]) - 1.0).min()
    print(f"{name}: min |255 alpha - 1| = {d:.2e}")
    assert d >= 1e-5, d


def _blends(case, fi):
    """(n,) does the Gaussian blend on some pixel: alpha >= 1/255 at a pixel whose walk reaches its list position"""
    pos = np.arange(len(case.order))[:, None, None]
    tiles_x = (case.w + 15) // 16
    ys, xs = np.mgrid[0:case.h, 0:case.w]
    pixel_tile = (xs // 16 + tiles_x * (ys // 16))[None]
    return ((B.alpha64(case) >= B.ALPHA_MIN) & (pos < fi[None]) & (pixel_tile == case.tile[:, None, None])).any(axis=(1, 2))


@pytest.mark.parametrize("channels", B.CHANNELS)
@pytest.mark.parametrize("name", list(B.CASES))
def test_reference_rows_are_not_small_and_the_reference_alone_meets_the_criterion(oracle, forwards, name, channels):
    """at every channel count the GPU file runs.  The fp32 oracle (final_T / final_idx from its own forward) against the
    fp64 one under the kernels' criterion, and inside HALF of it: the kernels do the fp32 oracle's arithmetic per pixel
    with a reciprocal and an exp of 1..2 ulp instead of correctly rounded ones and fp32 instead of double sums, so a case
    on which the reference alone used up the criterion would fail them for its conditioning, not for a fault of theirs.
    A condition on the seeds (backward_cases.OPERAND_SEED)."""
    case = B.CASES[name]
    ft, fi = forwards[name]
    colors, bg, v_out = B.operands(case, channels)
    ref64 = B.reference(oracle, case, colors, bg, v_out, ft, fi, np.float64)
    ref32 = B.reference(oracle, case, colors, bg, v_out, ft, fi, np.float32)
    # a dropped or doubled slot changes a colour-gradient row by the row itself: orders of magnitude above 1e-6 of scale
    rows = np.abs(ref64[2]).max(axis=1)
    blends = _blends(case, fi)
    assert (rows[~blends] == 0).all()
    smallest = rows[blends].min() / rows.max()
    print(f"{name} C={channels}: smallest blended colour-gradient row {smallest:.2e} of the largest; final_T >= {ft.min():.1e}")
    assert smallest >= 1e-3, smallest
    for what, a, b in zip(("v_xy", "v_conic", "v_colors", "v_opacity"), ref32, ref64):
        worst, ok = B.excess(a, b, RTOL, ATOL_FRAC)
        print(f"{name} C={channels} {what}: fp32 oracle exceeds rtol |ref| by {worst:.2e} of scale (allowed {ATOL_FRAC:g})")
        assert ok.all(), (what, worst)
        b64 = np.asarray(b, np.float64)
        used = (np.abs(a - b64) / (ATOL_FRAC * np.abs(b64).max() + RTOL * np.abs(b64) + 1e-300)).max()
        print(f"{name} C={channels} {what}: fp32 oracle uses {used:.2f} of the criterion")
        assert used <= 0.5, (what, used)
