"""Constructed tile lists for the blend backward kernels (csrc/blend2.hip blend2_bwd_wide_kernel and
blend2_bwd_narrow_kernel), and the arithmetic shared with tests/test_fast_forward_batches.py.  numpy only: what the
constructions claim is established on the CPU by tests/test_backward_cases_host.py, the kernels are run on them by
tests/test_backward_batches.py.

A wave of the wide backward takes its 8x8 quadrant's list in 64-entry chunks from `hi` (the wave maximum of final_idx)
downwards, culls each chunk against the quadrant's rectangle, queues the survivors, runs batches of 16 (the 16-slot
builds) or 28..32 slots while another chunk remains, moves the left-over (<= 15 / <= 27) to the front of the queue and
ends with one tail batch padded with null records.  Which survivor counts, left-overs and chunk edges a quadrant meets
decides which of these paths run: the cases below fix them.

A Gaussian with conic (a, 0, a) and opacity o reaches alpha >= 1/255 within r = sqrt(2 ln(255 o) / a) of its centre.
With a = 1.5625 (sigma 0.8 pixels), centres 2..5 pixels inside their quadrant and r < 2.9, the nearest pixel centre of
a neighbouring quadrant is >= 3 pixels away: sigma there is >= 7.03 against a cut-off (record margin included) of
<= 6.59.  So a quadrant's queue holds exactly the Gaussians centred in it, and every one of them reaches a pixel
centre of its own quadrant (the nearest is <= 0.71 pixels away, r >= 1.44 at opacity 0.02).

List order is index order: entry k of a tile's list is Gaussian `start + k`.  Every Gaussian is listed in one tile."""
from collections import namedtuple

import numpy as np

CONIC = 1.5625        # sigma = 0.8 pixels
QUADS = ((0, 0), (8, 0), (0, 8), (8, 8))      # (x0, y0) of the four quadrants of tile 0
ALPHA_MIN = 1.0 / 255.0


def _np_inputs(xys, conics, radii, opac, col, bg, h, w):
    """the oracle's argument tuple; list order = index order, tile counts from the radius box as the projection does"""
    n = len(xys)
    xys, conics = np.ascontiguousarray(xys, np.float32), np.ascontiguousarray(conics, np.float32)
    radii = np.ascontiguousarray(radii, np.int32)
    depths = np.linspace(1.0, 2.0, n).astype(np.float32)
    tiles_x, tiles_y = (w + 15) // 16, (h + 15) // 16
    x0 = np.clip(np.floor((xys[:, 0] - radii) / 16.0), 0, tiles_x)
    x1 = np.clip(np.floor((xys[:, 0] + radii) / 16.0) + 1, 0, tiles_x)
    y0 = np.clip(np.floor((xys[:, 1] - radii) / 16.0), 0, tiles_y)
    y1 = np.clip(np.floor((xys[:, 1] + radii) / 16.0) + 1, 0, tiles_y)
    nth = ((x1 - x0) * (y1 - y0)).astype(np.int32)
    opac = np.ascontiguousarray(opac, np.float32).reshape(n, 1)
    return xys, depths, radii, conics, nth, np.ascontiguousarray(col, np.float32), opac, np.ascontiguousarray(bg, np.float32)


def _reach(opac, conic=CONIC):
    return np.sqrt(2.0 * np.log(255.0 * np.asarray(opac, np.float64)) / conic)


def _quadrant_lists(order, rng):
    """small Gaussians, one per entry of `order` (quadrant numbers in list order), centred inside their quadrant"""
    n = len(order)
    opac = rng.uniform(0.02, 0.3, n)
    assert _reach(opac).max() < 2.9           # centres keep 3 pixels from the neighbouring quadrants' pixel centres
    q = np.asarray(order)
    x0 = np.array([QUADS[k][0] for k in q], np.float64)
    y0 = np.array([QUADS[k][1] for k in q], np.float64)
    xys = np.stack([x0 + rng.uniform(2.0, 5.0, n), y0 + rng.uniform(2.0, 5.0, n)], axis=1)
    conics = np.tile(np.float32([CONIC, 0.0, CONIC]), (n, 1))
    return xys, conics, np.full(n, 3, np.int32), opac


# ------------------------------------------------------------------------------------------------
# the backward cases
# ------------------------------------------------------------------------------------------------
# xys (n, 2) f32, conics (n, 3) f32, radii (n,) i32, opacity (n, 1) f32; order (n,): the quadrant a small Gaussian is
# centred in; tile (n,): the tile whose list holds it; broad (n,) bool: covers its whole tile (queued by all four
# quadrants); counts {tile: designed survivors per quadrant}; tile_bins (tiles, 2) i32; h, w: the image
Case = namedtuple("Case", "name xys conics radii opacity order tile broad counts tile_bins h w")


def _case(name, order, rng, max_opac=None, tile=None, h=16, w=16, edit=None):
    order = np.asarray(order, np.int64)
    n = len(order)
    tile = np.zeros(n, np.int64) if tile is None else np.asarray(tile, np.int64)
    assert (np.diff(tile) >= 0).all()          # the lists follow each other in tile order
    xys, conics, radii, opac = _quadrant_lists(order, rng)
    if max_opac is not None:
        opac = np.minimum(opac, max_opac)
    tiles_x, tiles_y = (w + 15) // 16, (h + 15) // 16
    xys[:, 0] += 16.0 * (tile % tiles_x)
    xys[:, 1] += 16.0 * (tile // tiles_x)
    broad = np.zeros(n, bool)
    if edit is not None:
        edit(xys, conics, radii, opac, broad)
    ntiles = tiles_x * tiles_y
    ends = np.cumsum(np.bincount(tile, minlength=ntiles))
    bins = np.stack([ends - np.bincount(tile, minlength=ntiles), ends], axis=1).astype(np.int32)
    counts = {t: tuple(int(((order == k) & (tile == t) & ~broad).sum() + (broad & (tile == t)).sum()) for k in range(4))
              for t in range(ntiles)}
    return Case(name, np.ascontiguousarray(xys, np.float32), np.ascontiguousarray(conics, np.float32),
                np.ascontiguousarray(radii, np.int32), np.ascontiguousarray(opac, np.float32).reshape(n, 1), order, tile,
                broad, counts, bins, h, w)


def ids_of(case):
    """gaussian_ids_sorted of the case: list order is index order"""
    return np.arange(len(case.order), dtype=np.int32)


# survivors per quadrant around the batch sizes: 16 slots / 28..32 slots
EDGES_16 = ((0, 1, 3, 4), (5, 15, 16, 17), (31, 32, 33, 48))
EDGES_32 = ((27, 28, 29, 31), (32, 33, 55, 56), (59, 60, 61, 64))
CHUNK_LENGTHS = (1, 63, 64, 65, 128, 129)
TWO_TILE_LENGTHS = (64, 65, 129)
NARROW_COUNTS = ((0, 1, 63, 0), (3, 4, 5, 52), (64, 0, 0, 0))     # survivors of ONE 64-entry chunk
FIN_NARROW, FIN_BROAD, FIN_LAST = (4, 5, 6), tuple(range(24, 32)), 29


def batch_edges(counts):
    """one tile; the four quadrants queue `counts` survivors, shuffled through the list.  No pixel saturates, so a
    quadrant's walk starts at its own last entry (hi = that position + 1; the list length for the quadrant that holds
    the last entry)"""
    rng = np.random.default_rng(100 + sum(counts))
    order = rng.permutation(np.repeat(np.arange(4), counts))
    return _case("edges_%d_%d_%d_%d" % counts, order, rng, max_opac=0.15)


def fullest_queue(left):
    """positions 0..63: quadrant 0; positions 64..127: `left` (15 / 27) entries of quadrant 0, position 127 among them,
    the rest in the other quadrants.  Quadrant 0 walks from hi = 128: the first chunk queues `left` and runs no batch,
    the second brings the queue to left + 64 (79; 91 of BQ_CAP 92), then batches, a left-over of `left` and the tail"""
    rng = np.random.default_rng(200 + left)
    second = np.concatenate([np.zeros(left - 1, np.int64), 1 + np.arange(64 - left) % 3])
    order = np.concatenate([np.zeros(64, np.int64), rng.permutation(second), [0]])
    return _case("fullest_%d" % left, order, rng, max_opac=0.08)


def left_over_moves():
    """260 entries, a third to each of three quadrants: five chunks of about 21 survivors, the left-over moves to the
    front several times; the fourth quadrant walks nothing"""
    return _case("left_over_260", np.arange(260) % 3, np.random.default_rng(6), max_opac=0.08)


def chunk_edges(length):
    """every entry in quadrant 1: chunks of 64 from hi = length; the other quadrants blend nothing"""
    return _case("chunk_%d" % length, np.ones(length, np.int64), np.random.default_rng(300 + length), max_opac=0.08)


def two_tiles(length):
    """a 16 x 32 image: tile 0 lists 37 entries, tile 1 `length`, so tile 1's range starts at 37 (no multiple of 4 or
    64); every Gaussian stays inside its own tile"""
    rng = np.random.default_rng(400 + length)
    order = rng.integers(0, 4, 37 + length)
    order[-1] = 3
    tile = np.concatenate([np.zeros(37, np.int64), np.ones(length, np.int64)])
    return _case("two_tiles_%d" % length, order, rng, max_opac=0.08, tile=tile, h=16, w=32)


def fin_inside_a_batch():
    """60 entries in quadrant 0.  Positions 4..6: narrow Gaussians of opacity 0.8 on pixel (2, 2), which then stops after
    two of the broad ones; positions 24..31: broad Gaussians of opacity 0.8 over the whole tile, of which every other
    pixel blends five (T falls below 1e-4 at the sixth).  final_idx is 26 on (2, 2) and 29 elsewhere: pos < fin differs
    between the pixels of one batch, entries behind position 28 are walked by no pixel, and the three other quadrants
    queue only the broad entries"""
    def edit(xys, conics, radii, opac, broad):
        np.minimum(opac, 0.05, out=opac)
        for k in FIN_NARROW:
            xys[k], opac[k], conics[k] = (2.0, 2.0), 0.8, (8.0, 0.0, 8.0)
        for k in FIN_BROAD:
            xys[k], opac[k], radii[k], conics[k], broad[k] = (4.0, 4.0), 0.8, 40, (1e-5, 0.0, 1e-5), True
    return _case("fin_inside_a_batch", np.zeros(60, np.int64), np.random.default_rng(8), edit=edit)


def narrow_chunk(counts):
    """one chunk of 64 list entries of which the quadrants keep `counts`"""
    rng = np.random.default_rng(500 + counts[0])
    order = rng.permutation(np.repeat(np.arange(4), counts))
    return _case("narrow_%d_%d_%d_%d" % counts, order, rng, max_opac=0.08)


def _all(*groups):
    return {c.name: c for g in groups for c in g}


SHARED = _all([fullest_queue(15), fullest_queue(27), left_over_moves(), fin_inside_a_batch()],
              [chunk_edges(k) for k in CHUNK_LENGTHS], [two_tiles(k) for k in TWO_TILE_LENGTHS])
WIDE_16 = _all([batch_edges(c) for c in EDGES_16])
WIDE_32 = _all([batch_edges(c) for c in EDGES_32])
NARROW = _all([narrow_chunk(c) for c in NARROW_COUNTS])
CASES = {**WIDE_16, **WIDE_32, **SHARED, **NARROW}
# what a build runs: both batch-edge sets on every wide build (a 32-slot count is one more left-over for 16 slots)
WIDE_CASES = list({**WIDE_16, **WIDE_32, **SHARED})
NARROW_CASES = list({**NARROW, **SHARED})


# ------------------------------------------------------------------------------------------------
# fp64 arithmetic of the constructions
# ------------------------------------------------------------------------------------------------
def alpha64(case):
    """(n, h, w) opacity * exp(-sigma) in fp64 on the case's fp32 inputs, at the pixel centres (integer coordinates)"""
    x, y = case.xys[:, 0].astype(np.float64), case.xys[:, 1].astype(np.float64)
    c = case.conics.astype(np.float64)
    dx = x[:, None, None] - np.arange(case.w, dtype=np.float64)[None, None, :]
    dy = y[:, None, None] - np.arange(case.h, dtype=np.float64)[None, :, None]
    sigma = 0.5 * (c[:, 0, None, None] * dx * dx + c[:, 2, None, None] * dy * dy) + c[:, 1, None, None] * dx * dy
    return case.opacity.astype(np.float64).reshape(-1, 1, 1) * np.exp(-sigma)


def quadrant_views(case, a):
    """[(tile, quadrant, a[:, its 8 x 8 pixels])]"""
    tiles_x = (case.w + 15) // 16
    out = []
    for t in range(len(case.tile_bins)):
        for k, (x0, y0) in enumerate(QUADS):
            xs, ys = 16 * (t % tiles_x) + x0, 16 * (t // tiles_x) + y0
            out.append((t, k, a[:, ys:ys + 8, xs:xs + 8]))
    return out


def quadrant_of(case):
    """(n,) tile-local quadrant a Gaussian's centre lies in"""
    lx, ly = case.xys[:, 0] % 16.0, case.xys[:, 1] % 16.0
    return (lx >= 8).astype(np.int64) + 2 * (ly >= 8).astype(np.int64)


def excess(a, b, rtol, atol_frac):
    """the criterion of test_gpu_parity.assert_close, |a - b| <= atol_frac max|b| + rtol |b|, as numbers: the largest
    |a - b| - rtol |b| as a fraction of max|b| (the criterion holds when it is <= atol_frac), and per element whether it
    is met"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.abs(b).max() if b.size else 0.0
    err = np.abs(a - b) - rtol * np.abs(b)
    ok = err <= atol_frac * scale + 1e-30
    return (float(err.max() / scale) if b.size and scale > 0 else 0.0), ok


# ------------------------------------------------------------------------------------------------
# operands and references (the oracle module is handed in: nothing here imports it)
# ------------------------------------------------------------------------------------------------
# channel counts the GPU file runs (a pair of 32 + c2 channels is one array of that many to the reference)
CHANNELS = (1, 3, 5, 8, 12, 17, 32, 33, 35, 39, 40)
# The per-pixel fin case is badly conditioned for v_opacity: T is rebuilt from final_T ~ 2e-4 through five factors
# 1 / (1 - alpha) with 1 - alpha = 0.2, which carries the fp32 rounding of alpha fourfold each, and the first broad
# entry's gradient is a sum of 256 such terms of either sign.  Where that sum happens to be small the fp32 ORACLE misses
# the criterion against the fp64 one (seed 0, 17 channels: 3.2 times the allowed error).  A case's operands use the first
# seed that meets the conditions tests/test_backward_cases_host.py holds every case to at every channel count above: the
# fp32 oracle inside half the criterion, and no blended Gaussian with a colour-gradient row below 1e-3 of the largest
# (with a single channel a row is one sum of either sign: seed 0 leaves one of 4.6e-5 in two_tiles_64).
OPERAND_SEED = {"fin_inside_a_batch": 7, "two_tiles_64": 1}


def operands(case, channels, seed=None):
    """(colours (n, channels) in [-1, 1), background in [0, 1), standard-normal cotangent (h, w, channels)), fp32"""
    seed = OPERAND_SEED.get(case.name, 0) if seed is None else seed
    rng = np.random.default_rng(1000 * seed + channels)
    n = len(case.order)
    return (rng.uniform(-1, 1, (n, channels)).astype(np.float32), rng.uniform(0, 1, channels).astype(np.float32),
            rng.standard_normal((case.h, case.w, channels)).astype(np.float32))


def forward32(oracle, case, ids=None, tile_bins=None):
    """final_T, final_idx of the fp32 oracle's forward over the case's lists (they do not depend on the colours)"""
    ids = ids_of(case) if ids is None else ids
    bins = case.tile_bins if tile_bins is None else tile_bins
    n = len(case.order)
    _, ft, fi = oracle.blend_fwd(ids, bins, case.xys, case.conics, np.zeros((n, 1), np.float32), case.opacity, case.h,
                                 case.w, np.zeros(1, np.float32))
    return ft, fi


def reference(oracle, case, colors, bg, v_out, final_T, final_idx, dtype=np.float64, ids=None, tile_bins=None):
    """the oracle's blend_bwd -> (v_xy, v_conic, v_colors, v_opacity (n, 1))"""
    ids = ids_of(case) if ids is None else ids
    bins = case.tile_bins if tile_bins is None else tile_bins
    return oracle.blend_bwd(ids, bins, case.xys, case.conics, colors, case.opacity, case.h, case.w, bg, final_T,
                            final_idx, v_out, dtype=dtype)
