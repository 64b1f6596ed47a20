"""Inputs built to land on the size classes and pass counts of csrc/binning.hip, in numpy only (no GPU, no library).

The bucket depth sort orders a bucket's run in one of three ways by its length (<= 256 by rank counting in 1..4 slots of
64, 257..512 by LSD byte passes in LDS, longer ones by a compare-exchange network in global memory), the tile sort
splits the tile id's bits over ceil(bits / 8) passes, the tile box travels packed in 10-bit fields, and the radix kernels
switch from 4 to 16 keys per thread at 4096 * 1024 entries.  Random scenes reach few of these; the builders here aim at
each one, and `bucket_runs` / `tile_boxes` let a test assert that the aim was true before it compares anything.

Expected values never come from this file's restatement of the bucket law: every comparison is with the oracle's 64-bit
sort (oracle.bin_and_sort); `lexsort_lists` is a second, independent statement of that order, used on the CPU to keep
the builders and the oracle honest with each other.
"""
import functools
from collections import namedtuple

import numpy as np

TILE = 16
ONE_BITS = 0x3F800000                       # bits of 1.0f
SENTINEL_LO, SENTINEL_HI = 0xFFFFFFFF, 0    # range part of a block without a visible Gaussian (include/gg_raster.h)
RS_SWITCH = 4096 * 1024                     # entries from which the radix kernels take 16 keys per thread

Case = namedtuple("Case", "xys depths radii nth tiles_x tiles_y")


# ---------------------------------------------------------------------------------------------------------------------
# tile boxes, bucket runs, expected lists
# ---------------------------------------------------------------------------------------------------------------------
def tile_boxes(xys, radii, tiles_x, tiles_y):
    """The tile box of every Gaussian in the projection's fp32 arithmetic -> x0, y0, x1, y1, num_tiles_hit (int32).
    A radius <= 0 gives a count of 0; so does a box that the clip to the grid leaves empty (the radius stays)."""
    f = np.float32
    xys = np.asarray(xys, np.float32)
    cx, cy, r = xys[:, 0] / f(TILE), xys[:, 1] / f(TILE), np.asarray(radii).astype(np.float32) / f(TILE)
    x0 = np.clip(cx - r, 0, tiles_x).astype(np.int32)
    x1 = np.clip((cx + r) + f(1), 0, tiles_x).astype(np.int32)
    y0 = np.clip(cy - r, 0, tiles_y).astype(np.int32)
    y1 = np.clip((cy + r) + f(1), 0, tiles_y).astype(np.int32)
    nth = ((x1 - x0) * (y1 - y0)).astype(np.int32)
    nth[np.asarray(radii) <= 0] = 0
    return x0, y0, x1, y1, nth


def num_buckets(n):
    nb = 256
    while nb < 32768 and nb * 64 < n:
        nb <<= 1
    return nb


def bucket_runs(depths, radii):
    """-> (number of buckets, run length of every bucket over the visible Gaussians): a numpy restatement of the
    PRESENT bucket law of binning.hip (db_buckets / db_range_of / db_bucket: bucket = floor((bits - min) * floor(NB 2^32 /
    (max - min + 1)) / 2^32), NB from the number of Gaussians, the range over radius > 0 only).

    For PRECONDITIONS only — "this input really contains a run of 257" — never for expected values.  If a later change
    alters the bucket law, the precondition fails: its author re-aims the inputs (and this function) so that every size
    class is reached again.  The comparison with the oracle that the precondition guards is not what gets deleted."""
    depths = np.ascontiguousarray(depths, np.float32)
    nb = num_buckets(len(depths))
    k = depths.view(np.uint32)[np.asarray(radii) > 0].astype(np.uint64)
    if k.size == 0:
        return nb, np.zeros(nb, np.int64)
    lo, hi = int(k.min()), int(k.max())
    mul = (nb << 32) // (hi - lo + 1)
    d = k - np.uint64(lo)                                                  # < 2^32; mul < 2^47: the two partial
    mh, ml = np.uint64(mul >> 32), np.uint64(mul & 0xFFFFFFFF)             # products below stay inside 64 bits
    b = np.minimum(d * mh + ((d * ml) >> np.uint64(32)), np.uint64(nb - 1)).astype(np.int64)
    return nb, np.bincount(b, minlength=nb)


def lexsort_lists(xys, depths, radii, tiles_x, tiles_y):
    """-> (gaussian_ids_sorted int32 (I,), tile_bins int32 (T, 2)): every Gaussian's box emitted row-major, the entries
    ordered by np.lexsort over (tile id, depth bits, Gaussian id); an empty tile's range is (0, 0)."""
    x0, y0, x1, y1, nth = tile_boxes(xys, radii, tiles_x, tiles_y)
    n, total = len(nth), int(nth.sum(dtype=np.int64))
    g = np.repeat(np.arange(n, dtype=np.int64), nth)
    first = np.cumsum(nth, dtype=np.int64) - nth
    k = np.arange(total, dtype=np.int64) - first[g]
    bw = np.maximum((x1 - x0).astype(np.int64), 1)[g]
    tile = (y0[g] + k // bw) * tiles_x + x0[g] + k % bw
    bits = np.ascontiguousarray(depths, np.float32).view(np.uint32)[g]
    order = np.lexsort((g, bits, tile))
    ids, tile = g[order].astype(np.int32), tile[order]
    t = np.arange(tiles_x * tiles_y)
    bins = np.stack([np.searchsorted(tile, t, "left"), np.searchsorted(tile, t, "right")], axis=1).astype(np.int32)
    bins[bins[:, 0] == bins[:, 1]] = 0
    return ids, bins


def range_parts(depths, radii, block, parts=None):
    """The partial minima / maxima of the visible depth bits per `block` consecutive Gaussians, as gg_view_fwd leaves
    them for gg_bin_sort_dev_ex (block 256); a block without a visible Gaussian — or beyond the end, when `parts` asks
    for more pairs than blocks — holds (0xFFFFFFFF, 0).  -> (lo, hi) uint32 arrays."""
    bits = np.ascontiguousarray(depths, np.float32).view(np.uint32)
    vis = np.asarray(radii) > 0
    n = len(bits)
    blocks = -(-n // block)
    parts = blocks if parts is None else parts
    assert parts >= blocks
    lo = np.full(parts, SENTINEL_LO, np.uint32)
    hi = np.full(parts, SENTINEL_HI, np.uint32)
    for p in range(blocks):
        v = bits[p * block:(p + 1) * block][vis[p * block:(p + 1) * block]]
        if v.size:
            lo[p], hi[p] = v.min(), v.max()
    return lo, hi


def tile_digit_split(tiles_x, tiles_y):
    """bits per radix pass of the tile sort: tile_bits over ceil(tile_bits / 8) passes of equal width"""
    bits = 1
    while (1 << bits) < tiles_x * tiles_y:
        bits += 1
    passes = (bits + 7) // 8
    per = (bits + passes - 1) // passes
    return [min(per, bits - per * p) for p in range(passes)]


def _case(xys, depths, radii, tiles_x, tiles_y, zero_radius_of_empty_boxes=False):
    radii = np.ascontiguousarray(radii, np.int32)
    nth = tile_boxes(xys, radii, tiles_x, tiles_y)[4]
    if zero_radius_of_empty_boxes:
        radii[nth == 0] = 0
    return Case(np.ascontiguousarray(xys, np.float32), np.ascontiguousarray(depths, np.float32), radii, nth,
                tiles_x, tiles_y)


# ---------------------------------------------------------------------------------------------------------------------
# A. bucket runs of exact length
# ---------------------------------------------------------------------------------------------------------------------
GROUP_SIZES = (1, 2, 63, 64, 65, 96, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 320, 383, 384, 385, 448, 449,
               511, 512, 513, 514, 700, 1023, 1024, 1025)
GROUP_VISIBLE = sum(GROUP_SIZES)                                   # 10 468
GROUP_EDGES = (128, 129, 192, 193, 256, 257, 512, 513, 1024, 1025)   # lengths either side of every class boundary
GROUP_LAWS = ("identical", "distinct", "ties", "random")
GROUP_N = (10_468, 40_468, 130_468)                                # 256, 1 024, 2 048 buckets


def group_case(law, n, seed=3):
    """30 groups of visible Gaussians, group g of GROUP_SIZES[g] members with depth bits bits(1.0f) + (g << 23) + offset
    — 2^g (1 + offset ulps) — so that with 30 groups over 29 octaves every group is one bucket's run and no two share a
    bucket (asserted by the callers with bucket_runs; offsets stay below 4 096 and the first element's is 0).  n -
    10 468 culled Gaussians (radius 0, depths up to 1e9 that must not enter the range) are mixed in and the index order
    is shuffled, so a group's members are spread over the walking workgroups.  64 x 64 image, radii 1..11, centres from
    -10 to 74: some visible Gaussians have an empty box; they keep their radius (they are part of their run) and emit
    nothing.  Offset laws:
      identical  all 0: in the 257..512 class every depth digit is constant, the id round decides alone;
      distinct   a permutation of 0 .. size-1, times 3: no ties, id order unrelated to depth order;
      ties       five values k * 257: two depth bytes vary, hundreds of ties per run;
      random     uniform below 2 048."""
    assert law in GROUP_LAWS and n >= GROUP_VISIBLE
    rng = np.random.default_rng(seed)
    sizes = np.array(GROUP_SIZES)
    group = np.repeat(np.arange(len(sizes)), sizes)
    if law == "identical":
        off = np.zeros(GROUP_VISIBLE, np.int64)
    elif law == "distinct":
        off = np.concatenate([rng.permutation(s) for s in sizes]) * 3
    elif law == "ties":
        off = rng.integers(0, 5, GROUP_VISIBLE) * 257
    else:
        off = rng.integers(0, 2048, GROUP_VISIBLE)
    off[0] = 0
    assert off.max() < 4096                 # (from 2^14 on a group would lie across a bucket boundary)
    bits = (ONE_BITS + (group << 23) + off).astype(np.uint32)
    culled = n - GROUP_VISIBLE
    depths = np.concatenate([bits.view(np.float32), rng.uniform(0.5, 1e9, culled).astype(np.float32)])
    radii = np.concatenate([rng.integers(1, 12, GROUP_VISIBLE), np.zeros(culled, np.int64)]).astype(np.int32)
    xys = rng.uniform(-10.0, 74.0, (n, 2)).astype(np.float32)
    perm = rng.permutation(n)
    return _case(xys[perm], depths[perm], radii[perm], 4, 4)


def group_preconditions(c):
    nb, runs = bucket_runs(c.depths, c.radii)
    assert nb == num_buckets(len(c.depths))
    got = sorted(runs[runs > 0].tolist())
    for length in GROUP_EDGES:
        assert length in got, f"no bucket run of exactly {length} entries"
    assert got == sorted(GROUP_SIZES), "a group shares a bucket or lies across a bucket boundary"
    assert int(((c.radii > 0) & (c.nth == 0)).sum()) > 0, "no visible Gaussian with an empty box"
    assert int((c.radii > 0).sum()) == GROUP_VISIBLE


def reordered_culled_ends(c, blocks=20, block=256):
    """the same Gaussians in an order whose first and last `blocks` blocks of `block` hold culled ones only"""
    rng = np.random.default_rng(11)
    culled = np.flatnonzero(c.radii <= 0)
    need = blocks * block
    assert len(culled) >= 2 * need
    middle = rng.permutation(np.setdiff1d(np.arange(len(c.radii)), culled[:2 * need]))
    order = np.concatenate([culled[:need], middle, culled[need:2 * need]])
    return _case(c.xys[order], c.depths[order], c.radii[order], c.tiles_x, c.tiles_y)


def nothing_visible(c):
    return _case(c.xys, c.depths, np.zeros_like(c.radii), c.tiles_x, c.tiles_y)


# ---------------------------------------------------------------------------------------------------------------------
# B. tile grids and pass counts
# ---------------------------------------------------------------------------------------------------------------------
GRIDS = {(1, 1): [1], (2, 1): [1], (16, 16): [8], (257, 1): [5, 4], (1, 257): [5, 4], (256, 256): [8, 8],
         (1023, 65): [6, 6, 5], (1023, 1023): [7, 7, 6]}           # grid -> bits per pass of the tile sort


def grid_case(tiles_x, tiles_y, seed=5):
    """3 000 Gaussians with centres uniform over the grid's pixels, radii 1..39, depths uniform in 0.5..30, plus seven
    placed ones: radius 3 in each corner tile, one covering the whole grid, one reaching over the full width from the
    bottom row and one over the full height from the right column."""
    rng = np.random.default_rng(seed)
    n = 3000
    w, h = float(TILE * tiles_x), float(TILE * tiles_y)
    xys = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], axis=1)
    radii = rng.integers(1, 40, n)
    depths = rng.uniform(0.5, 30.0, n + 7)
    placed = [((8.0, 8.0), 3), ((w - 8.0, 8.0), 3), ((8.0, h - 8.0), 3), ((w - 8.0, h - 8.0), 3),
              ((w / 2, h / 2), int(max(w, h))), ((w / 2, h - 8.0), int(w)), ((w - 8.0, h / 2), int(h))]
    xys = np.concatenate([xys, np.array([p for p, _ in placed])])
    radii = np.concatenate([radii, np.array([r for _, r in placed])])
    perm = rng.permutation(n + 7)
    return _case(xys[perm], depths[perm], radii[perm], tiles_x, tiles_y)


def grid_preconditions(c):
    tx, ty = c.tiles_x, c.tiles_y
    assert tile_digit_split(tx, ty) == GRIDS[(tx, ty)]
    x0, y0, x1, y1, nth = tile_boxes(c.xys, c.radii, tx, ty)
    hit = nth > 0
    assert int((x1 - x0)[hit].max()) == tx, "no box as wide as the grid"
    assert int(x0[hit].max()) == tx - 1 and int(y0[hit].max()) == ty - 1, "no box starting in the last column / row"
    assert bool((hit & (x1 == tx) & (y1 == ty)).any()), "the last tile's list is empty"


# ---------------------------------------------------------------------------------------------------------------------
# C. the 16-keys-per-thread switch
# ---------------------------------------------------------------------------------------------------------------------
SWITCH_CASES = {(262_143, 15): 4_194_303, (262_144, 0): 4_194_304, (262_144, 1): 4_194_305, (262_500, 77): 4_200_077}
TIE_DEPTHS = (1.0, 1.5, 2.0, 2.0000002)


def switch_case(n1, extra, seed=2):
    """4 x 4 grid: n1 Gaussians of radius 200 at (32, 32), 16 tiles each, `extra` of radius 1 at (8, 8), one tile each;
    depths from four values, two of them one ulp apart."""
    rng = np.random.default_rng(seed)
    n = n1 + extra
    xys = np.full((n, 2), 32.0, np.float32)
    radii = np.full(n, 200, np.int32)
    xys[n1:] = 8.0
    radii[n1:] = 1
    depths = rng.choice(np.array(TIE_DEPTHS, np.float32), n)
    return _case(xys, depths, radii, 4, 4)


def switch_preconditions(c, n1, extra):
    total = int(c.nth.sum(dtype=np.int64))
    assert total == SWITCH_CASES[(n1, extra)] == 16 * n1 + extra
    assert (total >= RS_SWITCH) == ((n1, extra) != (262_143, 15))
    assert bucket_runs(c.depths, c.radii)[1].max() > 60_000        # runs through the global compare-exchange network


# ---------------------------------------------------------------------------------------------------------------------
# F. bucket counts beyond 64 KB of LDS histogram
# ---------------------------------------------------------------------------------------------------------------------
MANY_BUCKETS = {600_000: 16_384, 1_100_000: 32_768}


def many_buckets_case(n, seed=21):
    """97 % culled, the rest log-uniform depths over six decades, centres up to 20 pixels outside a 100 x 140 image,
    radii below 12 (the random-shapes test's second depth law)."""
    rng = np.random.default_rng(seed)
    h, w = 100, 140
    depths = (10.0 ** rng.uniform(-1.5, 4.5, n)).astype(np.float32) + np.float32(0.011)
    xys = np.stack([rng.uniform(-20, w + 20, n), rng.uniform(-20, h + 20, n)], axis=1)
    radii = rng.integers(0, 12, n)
    radii[rng.random(n) < 0.97] = 0
    return _case(xys, depths, radii, (w + 15) // 16, (h + 15) // 16, zero_radius_of_empty_boxes=True)


def many_buckets_preconditions(c):
    n = len(c.depths)
    assert num_buckets(n) == MANY_BUCKETS[n]
    assert 0.02 * n < int((c.radii > 0).sum()) < 0.04 * n


# ---------------------------------------------------------------------------------------------------------------------
# the cases by name (built once per process, never modified: the arrays are read-only)
# ---------------------------------------------------------------------------------------------------------------------
GROUP_CASES = [("identical", GROUP_N[0]), ("distinct", GROUP_N[0])] + \
              [(law, n) for law in ("ties", "random") for n in GROUP_N]
PARTS_BASE = "groups-random-40468"          # E: the input whose range parts are handed over
CASE_NAMES = [f"groups-{law}-{n}" for law, n in GROUP_CASES] + \
             [f"grid-{tx}x{ty}" for tx, ty in GRIDS] + \
             [f"switch-{n1}+{extra}" for n1, extra in SWITCH_CASES] + \
             [f"buckets-{n}" for n in MANY_BUCKETS] + \
             ["parts-culled-ends", "parts-nothing-visible"]
LEXSORT_SKIPPED = [f"switch-{n1}+{extra}" for n1, extra in SWITCH_CASES] + ["grid-1023x1023"]   # I > 1 M


@functools.lru_cache(maxsize=None)
def case(name):
    kind, _, rest = name.partition("-")
    if kind == "groups":
        law, n = rest.split("-")
        c = group_case(law, int(n))
    elif kind == "grid":
        c = grid_case(*map(int, rest.split("x")))
    elif kind == "switch":
        c = switch_case(*map(int, rest.split("+")))
    elif kind == "buckets":
        c = many_buckets_case(int(rest))
    elif name == "parts-culled-ends":
        c = reordered_culled_ends(case(PARTS_BASE))
    elif name == "parts-nothing-visible":
        c = nothing_visible(case(PARTS_BASE))
    else:
        raise KeyError(name)
    for a in c[:4]:
        a.setflags(write=False)
    return c


def check_preconditions(name):
    c = case(name)
    kind, _, rest = name.partition("-")
    assert np.array_equal(c.nth, tile_boxes(c.xys, c.radii, c.tiles_x, c.tiles_y)[4])
    if kind == "groups":
        group_preconditions(c)
    elif kind == "grid":
        grid_preconditions(c)
    elif kind == "switch":
        switch_preconditions(c, *map(int, rest.split("+")))
    elif kind == "buckets":
        many_buckets_preconditions(c)
    elif name == "parts-culled-ends":
        group_preconditions(c)
        lo, hi = range_parts(c.depths, c.radii, 256)
        for ends in (slice(0, 20), slice(-20, None)):
            assert np.all(lo[ends] == SENTINEL_LO) and np.all(hi[ends] == SENTINEL_HI)
        assert np.any(lo != SENTINEL_LO)
    elif name == "parts-nothing-visible":
        lo, hi = range_parts(c.depths, c.radii, 256)
        assert np.all(lo == SENTINEL_LO) and np.all(hi == SENTINEL_HI) and int(c.nth.sum()) == 0
    else:
        raise KeyError(name)
