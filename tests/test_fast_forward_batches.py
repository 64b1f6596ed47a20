"""The batched pair forward on constructed lists (csrc/blend2.hip blend2_fwd_batch_kernel, 16-slot batches): what the
random scenes of tests/test_fast_forward.py cross only by chance.  Same method and the same tolerances as that file:
images within 1e-6 (1 + |oracle|) of the oracle, final_T / final_idx equal to the oracle's and the exact-order kernel's
bits, the fast kernel selected through gg_blend_fwd_pair_fast.

  * batch boundaries: one 16x16 tile whose four quadrants queue 1 / 15 / 16 / 17 and 31 / 32 / 33 / 80 survivors, and a
    list of 260 entries of which a third survives each of three quadrants (the queue's left-over moves to the front four
    times, the fourth quadrant walks nothing);
  * ragged images: pixels outside the image in every quadrant position, second arrays of 7 / 3 / 1 channels;
  * a colour 10^6 times its predecessors' in the middle of a walk (the scale shrinks, the accumulators are rescaled);
  * the walk stops inside a batch: for some pixels at slot 5 of the first, for the whole quadrant at slot 9 of the second.

A Gaussian with conic (a, 0, a) and opacity o reaches alpha >= 1/255 within r = sqrt(2 ln(255 o) / a) of its centre; the
constructions keep r below the distance to the neighbouring quadrants' nearest pixel centres, so a quadrant's queue holds
exactly the Gaussians centred inside it (the cull never rejects one whose centre lies inside the rectangle)."""
import numpy as np
import pytest
import torch

from backward_cases import CONIC, QUADS, _np_inputs, _quadrant_lists, _reach      # noqa: F401 (shared constructions)
from test_fast_forward import DEV, Pair, _close, _np, _t

pytestmark = pytest.mark.gpu


class Built(Pair):
    """Pair on given arrays instead of a projected scene"""

    def __init__(self, xys, conics, radii, opac, col, bg, h, w, c=32):
        from gaussiangrasper_amd import _lib, ops as P
        self.lib, self.P, self._lib = _lib.load(), P, _lib
        self.np_in = _np_inputs(xys, conics, radii, opac, col, bg, h, w)
        xys, depths, radii, conics, nth, col, opac, bg = self.np_in
        self.n, self.h, self.w, self.c, self.c2 = len(xys), h, w, c, col.shape[1] - c
        self.xys, self.conics, self.opac = _t(xys), _t(conics), _t(opac)
        self.col, self.col2 = _t(col[:, :c]), _t(col[:, c:])
        self.bg, self.bg2 = _t(bg[:c]), _t(bg[c:])
        P.clear_bin_cache()
        b = P.bin_and_sort_gaussians(self.xys, _t(depths), _t(radii), _t(nth), h, w)
        self.ids, self.tile_bins = b.gaussian_ids_sorted, b.tile_bins
        self.ws = torch.empty(self.lib.gg_blend_workspace(self.n), dtype=torch.uint8, device=DEV)


def _check(pc, oracle, tol_images=True):
    e_img, e_img2, e_T, e_i = pc.run(False)
    f_img, f_img2, f_T, f_i = pc.run(True)
    assert torch.equal(e_T, f_T) and torch.equal(e_i, f_i), "final_T / final_idx must keep their bits"
    (o1, s1), (o2, _) = pc.oracle_images(oracle)
    assert np.array_equal(_np(f_T).view(np.uint32), s1["final_Ts"].view(np.uint32))
    assert np.array_equal(_np(f_i), s1["final_idx"])
    if tol_images:
        _close(_np(f_img), o1, "first array vs oracle")
        _close(_np(f_img2), o2, "second array vs oracle")
        _close(_np(f_img), _np(e_img), "first array vs exact kernel")
    return (f_img, f_img2), (o1, o2), s1


@pytest.mark.parametrize("counts", [(1, 15, 16, 17), (31, 32, 33, 80)])
def test_survivor_counts_around_the_batch_size(oracle, counts):
    rng = np.random.default_rng(5)
    order = rng.permutation(np.repeat(np.arange(4), counts))
    xys, conics, radii, opac = _quadrant_lists(order, rng)
    col = rng.uniform(-1, 1, (len(order), 39))
    pc = Built(xys, conics, radii, opac, col, rng.uniform(0, 1, 39), 16, 16)
    _, _, saved = _check(pc, oracle)
    fi = saved["final_idx"].reshape(16, 16)
    for k, (x0, y0) in enumerate(QUADS):       # every quadrant blended its own last Gaussian somewhere, and no later one
        assert fi[y0:y0 + 8, x0:x0 + 8].max() == np.flatnonzero(order == k).max() + 1


def test_queue_left_over_moves_to_the_front_several_times(oracle):
    rng = np.random.default_rng(6)
    order = np.arange(260) % 3                 # five chunks of 64 list entries; about 21 survivors per chunk and quadrant
    xys, conics, radii, opac = _quadrant_lists(order, rng)
    opac = np.minimum(opac, 0.08)              # 87 survivors per quadrant must not saturate it
    col = rng.uniform(-1, 1, (260, 39))
    pc = Built(xys, conics, radii, opac, col, rng.uniform(0, 1, 39), 16, 16)
    (f_img, _), _, saved = _check(pc, oracle)
    fi = saved["final_idx"].reshape(16, 16)
    assert fi[:8, :8].max() > 250 and (fi[8:, 8:] == 0).all()
    assert torch.equal(f_img[8:, 8:], pc.bg.expand(8, 8, 32))       # the empty quadrant is the background


@pytest.mark.parametrize("h,w", [(45, 70), (17, 33)])
@pytest.mark.parametrize("c2", [7, 3, 1])
def test_ragged_images_and_second_array_widths(oracle, h, w, c2):
    pc = Pair(oracle, 600, h, w, 32, c2, seed=41)
    _check(pc, oracle)


def test_colour_scale_shrinks_in_the_middle_of_a_walk(oracle):
    """40 survivors of colour ~1e-3, one of 1e3 in one channel of each array, small colours again: the tolerance is the
    wide-range one of test_fast_pair_forward_over_a_wide_dynamic_range, 2^-20 of the channel's largest |colour|"""
    rng = np.random.default_rng(7)
    n = 70
    xys, conics, radii, opac = _quadrant_lists(np.zeros(n, int), rng)
    opac = np.minimum(opac, 0.08)
    col = rng.uniform(-1e-3, 1e-3, (n, 39))
    col[40, 5], col[40, 32 + 2] = 1e3, -1e3
    bg = rng.uniform(0, 1, 39)
    pc = Built(xys, conics, radii, opac, col, bg, 16, 16)
    (f_img, f_img2), (o1, o2), _ = _check(pc, oracle, tol_images=False)
    col, bg = pc.np_in[5], pc.np_in[7]
    for img, ref, cc, bb in ((_np(f_img), o1, col[:, :32], bg[:32]), (_np(f_img2), o2, col[:, 32:], bg[32:])):
        cmax = np.maximum(np.abs(cc).max(axis=0), np.abs(bb)).astype(np.float64)       # per channel
        err = np.abs(img.astype(np.float64) - ref).reshape(-1, img.shape[-1]).max(axis=0)
        assert (err <= 2.0 ** -20 * cmax + 1e-37).all(), (err / cmax).max()
    assert np.abs(o1[..., 5]).max() > 1.0 and np.abs(o2[..., 2]).max() > 1.0       # the large colour was blended


def test_walk_stops_inside_a_batch(oracle):
    """list positions 4, 5: opaque points on pixel (2, 2) — that pixel stops at slot 5 of the first batch; positions 24, 25:
    opaque Gaussians over the whole tile — every other pixel stops at slot 9 of the second batch (alpha is capped at 0.999:
    the second opaque Gaussian takes T below 1e-4 and is not blended).  Strong colours follow and must not show."""
    rng = np.random.default_rng(8)
    n = 40
    xys, conics, radii, opac = _quadrant_lists(np.zeros(n, int), rng)
    opac = np.minimum(opac, 0.05)
    for k in (4, 5):
        xys[k], opac[k] = (2.0, 2.0), 1.0
        conics[k] = (8.0, 0.0, 8.0)            # alpha 0.018 one pixel away: only (2, 2) saturates
    for k in (24, 25):
        xys[k], opac[k], radii[k] = (4.0, 4.0), 1.0, 40
        conics[k] = (1e-5, 0.0, 1e-5)
    col = rng.uniform(-1, 1, (n, 39))
    col[26:] = 50.0
    pc = Built(xys, conics, radii, opac, col, rng.uniform(0, 1, 39), 16, 16)
    (f_img, f_img2), _, saved = _check(pc, oracle)
    fi = saved["final_idx"].reshape(16, 16)
    assert fi[2, 2] == 5                        # last blended: list position 4
    assert (np.delete(fi.ravel(), 2 * 16 + 2) == 25).all()      # every other pixel of the tile: list position 24
    assert float(f_img.abs().max()) < 2.0 and float(f_img2.abs().max()) < 2.0
