"""csrc/binning.hip on inputs built to hit each of its size classes and pass counts (tests/binning_cases.py), through the
C ABI, bit for bit against the oracle's 64-bit sort:

  A  bucket runs of exact length: 1 .. 1 025 entries, either side of every boundary between the rank-counting slots
     (64 / 128 / 192 / 256), the LDS byte passes (257 .. 512) and the global compare-exchange network (513 ..), under
     four laws for the depths inside a run and three bucket counts;
  B  tile grids from 1 x 1 to 1023 x 1023: one, two and three radix passes of the tile sort (8 + 8 and 7 + 7 + 6 bits
     among them) and every field of the packed tile box at its largest value;
  C  list lengths one below, at and above the switch from 4 to 16 keys per thread, and a ragged last block;
  D  gg_bin_sort_dev with the count on the device below, at and one below the capacity;
  E  gg_bin_sort_dev_ex with handed-over range parts: 1, 65, ceil(N / 256) and 300 of them, blocks of culled Gaussians
     at both ends, nothing visible at all;
  F  16 384 and 32 768 depth buckets (more than 64 KB of LDS histogram in the walking kernels).

Every call writes into arrays pre-filled with -7 that carry a guard tail of 4 096 entries, which must come back
untouched; the sorted tile ids are requested and compared with the tile ranges' own statement of them.  Each case first
asserts, on the CPU, that it contains what it was built for (binning_cases.check_preconditions); the oracle's result for
a case is computed once and shared."""
import numpy as np
import pytest
import torch

import binning_cases as BC
from gaussiangrasper_amd import _lib
from gaussiangrasper_amd import ops as P
from test_gpu_parity import assert_bitexact

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096
FILL = -7
_REF = {}


def _reference(oracle, name):
    """the oracle's lists for a named case, computed once: (case, count, gaussian_ids_sorted, tile_bins)"""
    if name not in _REF:
        BC.check_preconditions(name)
        c = BC.case(name)
        ref = oracle.bin_and_sort(c.xys, c.depths, c.radii, c.nth, (c.tiles_x, c.tiles_y, 1))
        assert ref["num_intersects"] == int(c.nth.sum(dtype=np.int64))
        ids, bins = ref["gaussian_ids_sorted"], ref["tile_bins"]
        ids.setflags(write=False)
        bins.setflags(write=False)
        _REF[name] = (c, int(ref["num_intersects"]), ids, bins)
    return _REF[name]


def _dev(a):
    a = np.array(a, order="C")          # (a copy: the cases' arrays are read-only)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(DEV)


def _call(c, count, entry="gg_bin_sort", capacity=None, parts=None):
    """One call of `entry` on case c -> (ids, tiles, bins) as numpy, ids / tiles [:capacity] (the guard tails are
    asserted here).  gg_bin_sort takes the count itself; the _dev entries take `capacity` and find the count on the
    device; parts = (lo, hi) uint32 arrays for gg_bin_sort_dev_ex."""
    lib = _lib.load()
    n, ntiles = len(c.depths), c.tiles_x * c.tiles_y
    cap = count if capacity is None else capacity
    xt, dt, rt, nt = _dev(c.xys), _dev(c.depths), _dev(c.radii), _dev(c.nth)
    ids = torch.full((cap + GUARD,), FILL, dtype=torch.int32, device=DEV)
    tiles = torch.full((cap + GUARD,), FILL, dtype=torch.int32, device=DEV)
    bins = torch.full((ntiles + GUARD, 2), FILL, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(lib.gg_bin_sort_workspace(n, cap), 256), dtype=torch.uint8, device=DEV)
    geometry = (P._ptr(xt), P._ptr(dt), P._ptr(rt), P._ptr(nt), c.tiles_x, c.tiles_y, P._ptr(ids), P._ptr(bins),
                P._ptr(tiles), P._ptr(ws), ws.numel())
    stream = P._stream(xt.device)
    if entry == "gg_bin_sort":
        assert capacity is None and parts is None
        status = lib.gg_bin_sort(n, count, *geometry, stream)
    else:
        total = torch.tensor([count], dtype=torch.int64, device=DEV)
        if entry == "gg_bin_sort_dev":
            assert parts is None
            status = lib.gg_bin_sort_dev(n, cap, P._ptr(total), *geometry, stream)
        else:
            lo, hi = (_dev(parts[0]), _dev(parts[1])) if parts else (None, None)
            status = lib.gg_bin_sort_dev_ex(n, cap, P._ptr(total), *geometry, P._ptr(lo) if parts else None,
                                            P._ptr(hi) if parts else None, len(parts[0]) if parts else 0, stream)
    _lib.check(status, entry)
    torch.cuda.synchronize()
    ids, tiles, bins = ids.cpu().numpy(), tiles.cpu().numpy(), bins.cpu().numpy()
    assert np.all(ids[cap:] == FILL), f"{entry}: gaussian_ids_sorted written past its {cap} entries"
    assert np.all(tiles[cap:] == FILL), f"{entry}: isect_tile_sorted written past its {cap} entries"
    assert np.all(bins[ntiles:] == FILL), f"{entry}: tile_bins written past its {ntiles} ranges"
    return ids[:cap], tiles[:cap], bins[:ntiles]


def _assert_equals_oracle(got, count, ref_ids, ref_bins, what):
    ids, tiles, bins = got
    assert_bitexact(bins, ref_bins, f"{what}: tile_bins")
    assert_bitexact(ids[:count], ref_ids, f"{what}: gaussian_ids_sorted")
    lens = np.diff(np.asarray(ref_bins).reshape(-1, 2), axis=1).ravel()
    assert_bitexact(tiles[:count], np.repeat(np.arange(len(lens), dtype=np.int32), lens), f"{what}: isect_tile_sorted")


def _check(oracle, name, entry="gg_bin_sort", capacity=None, parts=None):
    c, count, ref_ids, ref_bins = _reference(oracle, name)
    got = _call(c, count, entry, capacity, parts)
    _assert_equals_oracle(got, count, ref_ids, ref_bins, f"{name} {entry}")
    return got


# ---- A ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law,n", BC.GROUP_CASES)
def test_bucket_runs_of_exact_length(oracle, law, n):
    """one run of each of 1, 2, 63, 64, 65, 96, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 320, 383, 384, 385,
    448, 449, 511, 512, 513, 514, 700, 1 023, 1 024 and 1 025 entries (asserted), among culled Gaussians and visible
    ones with an empty tile box"""
    _check(oracle, f"groups-{law}-{n}")


# ---- B ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles_x,tiles_y", list(BC.GRIDS))
def test_tile_grids_and_pass_counts(oracle, tiles_x, tiles_y):
    """digit splits [1], [1], [8], [5, 4], [5, 4], [8, 8], [6, 6, 5], [7, 7, 6]; a box as wide as the grid, boxes
    starting in the last column and the last row, the last tile's list not empty (asserted)"""
    _check(oracle, f"grid-{tiles_x}x{tiles_y}")


# ---- C ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,extra", list(BC.SWITCH_CASES))
def test_switch_to_16_keys_per_thread(oracle, n1, extra):
    """4 194 303, 4 194 304, 4 194 305 and 4 200 077 entries; four depth values, so runs of ~65 000 Gaussians go
    through the global compare-exchange network"""
    _check(oracle, f"switch-{n1}+{extra}")


# ---- D ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["groups-random-10468", "switch-262144+1"])
def test_device_count_below_a_capacity_of_whole_mi_entries(oracle, name):
    """what ops.bin_and_sort_gaussians does in production: launches sized for 5 Mi entries (16 keys per thread), the
    real count on the device; entries [:count] and every range equal the oracle's"""
    _check(oracle, name, "gg_bin_sort_dev", capacity=5 << 20)


@pytest.mark.parametrize("slack", [0, 1])
def test_device_count_at_and_one_below_the_capacity(oracle, slack):
    name = "groups-random-10468"
    _check(oracle, name, "gg_bin_sort_dev", capacity=_reference(oracle, name)[1] + slack)


# ---- E ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [None, 1, 65, 300])
def test_handed_over_range_parts(oracle, parts):
    """gg_bin_sort_dev_ex with the range parts computed as include/gg_raster.h describes them: ceil(N / 256) pairs over
    blocks of 256 (None), and 1, 65 and 300 pairs over correspondingly larger or smaller blocks (the reduction strides
    by 64).  Equal to the oracle's lists and to gg_bin_sort's."""
    c, count, _, _ = _reference(oracle, BC.PARTS_BASE)
    n = len(c.depths)
    lo, hi = BC.range_parts(c.depths, c.radii, 256) if parts is None else \
        BC.range_parts(c.depths, c.radii, -(-n // parts), parts)
    assert len(lo) == (parts or -(-n // 256))
    got = _check(oracle, BC.PARTS_BASE, "gg_bin_sort_dev_ex", capacity=count, parts=(lo, hi))
    plain = _check(oracle, BC.PARTS_BASE)
    for a, b, what in zip(got, plain, ("gaussian_ids_sorted", "isect_tile_sorted", "tile_bins")):
        assert_bitexact(a, b, f"gg_bin_sort_dev_ex vs gg_bin_sort: {what}")


def test_range_parts_with_culled_blocks_at_both_ends(oracle):
    """the first and the last 20 blocks of 256 hold culled Gaussians only: their parts are (0xFFFFFFFF, 0)"""
    name = "parts-culled-ends"
    c, count, _, _ = _reference(oracle, name)
    parts = BC.range_parts(c.depths, c.radii, 256)
    got = _check(oracle, name, "gg_bin_sort_dev_ex", capacity=count, parts=parts)
    plain = _check(oracle, name)
    for a, b, what in zip(got, plain, ("gaussian_ids_sorted", "isect_tile_sorted", "tile_bins")):
        assert_bitexact(a, b, f"gg_bin_sort_dev_ex vs gg_bin_sort: {what}")


def test_range_parts_with_nothing_visible(oracle):
    """every part is (0xFFFFFFFF, 0) and the count on the device is 0: status OK, every range (0, 0), nothing written
    past the outputs"""
    name = "parts-nothing-visible"
    c, count, ref_ids, ref_bins = _reference(oracle, name)
    assert count == 0 and len(ref_ids) == 0 and not np.asarray(ref_bins).any()
    parts = BC.range_parts(c.depths, c.radii, 256)
    for capacity in (1, 1000):
        ids, tiles, bins = _call(c, 0, "gg_bin_sort_dev_ex", capacity=capacity, parts=parts)
        assert_bitexact(bins, ref_bins, "tile_bins")
    ids, tiles, bins = _call(c, 0)                      # gg_bin_sort with a count of 0
    assert_bitexact(bins, ref_bins, "gg_bin_sort: tile_bins")


# ---- F ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(BC.MANY_BUCKETS))
def test_bucket_counts_beyond_64_kb_of_histogram(oracle, n):
    """600 000 Gaussians: 16 384 buckets; 1 100 000: 32 768 — the walking kernels' LDS histogram is 64 KB + 12 bytes and
    128 KB + 12 bytes; 97 % of the Gaussians are culled"""
    _check(oracle, f"buckets-{n}")
