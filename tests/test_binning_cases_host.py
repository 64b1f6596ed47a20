"""The constructed binning inputs (tests/binning_cases.py) on the CPU: every case really contains what it was built to
contain — the bucket runs, box fields, pass counts and entry counts that tests/test_binning_constructed.py relies on —
and the oracle's lists for it equal an independent np.lexsort statement of the order.  The second half also checks the
oracle itself on tile grids and entry counts no scene gives it.

The lexsort comparison is skipped where the case has more than 1 M list entries (binning_cases.LEXSORT_SKIPPED: the four
16-keys-per-thread cases and the 1023 x 1023 grid); their preconditions are still asserted."""
import numpy as np
import pytest

import binning_cases as BC
from test_gpu_parity import assert_bitexact


@pytest.mark.parametrize("name", BC.CASE_NAMES)
def test_case_meets_its_preconditions(name):
    BC.check_preconditions(name)


@pytest.mark.parametrize("name", [n for n in BC.CASE_NAMES if n not in BC.LEXSORT_SKIPPED])
def test_oracle_lists_equal_the_lexsort_statement(oracle, name):
    c = BC.case(name)
    assert int(c.nth.sum(dtype=np.int64)) <= 1 << 20
    ref = oracle.bin_and_sort(c.xys, c.depths, c.radii, c.nth, (c.tiles_x, c.tiles_y, 1))
    ids, bins = BC.lexsort_lists(c.xys, c.depths, c.radii, c.tiles_x, c.tiles_y)
    assert ref["num_intersects"] == len(ids) == int(c.nth.sum(dtype=np.int64))
    assert_bitexact(ref["tile_bins"], bins, "tile_bins")
    assert_bitexact(ref["gaussian_ids_sorted"], ids, "gaussian_ids_sorted")


def test_skipped_cases_are_the_large_ones():
    for name in BC.CASE_NAMES:
        big = int(BC.case(name).nth.sum(dtype=np.int64)) > 1 << 20
        assert big == (name in BC.LEXSORT_SKIPPED), name


def test_bucket_runs_on_hand_made_inputs():
    """the precondition helper itself: two depths at the ends of the range fall into the first and the last bucket, a
    culled Gaussian's depth does not widen the range, equal depths share a run"""
    depths = np.array([1.0, 1.0, 4.0, 1e9, 2.0], np.float32)
    radii = np.array([3, 1, 2, 0, 0], np.int32)
    nb, runs = BC.bucket_runs(depths, radii)
    assert nb == 256 and runs.sum() == 3 and runs[0] == 2 and runs[255] == 1
    assert BC.bucket_runs(depths, np.zeros(5, np.int32))[1].sum() == 0
    assert [BC.num_buckets(n) for n in (1, 16_384, 16_385, 131_072, 131_073, 1_048_577, 5_000_000)] == \
        [256, 256, 512, 2048, 4096, 32_768, 32_768]


def test_range_parts_blocks_and_sentinels():
    depths = np.arange(1, 11, dtype=np.float32)
    radii = np.array([1, 1, 0, 0, 0, 0, 1, 0, 1, 1], np.int32)
    lo, hi = BC.range_parts(depths, radii, 2, parts=7)
    bits = depths.view(np.uint32)
    assert lo.tolist() == [bits[0], BC.SENTINEL_LO, BC.SENTINEL_LO, bits[6], bits[8], BC.SENTINEL_LO, BC.SENTINEL_LO]
    assert hi.tolist() == [bits[1], 0, 0, bits[6], bits[9], 0, 0]
