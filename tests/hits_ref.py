"""Reference for the surface hits (include/gg_raster.h gg_blend_hits), built from the CPU oracle as a black box.

O.blend_fwd takes explicit tile lists.  With every tile's list cut to its first k entries its final_T is T_after of
list position k for every pixel (T is unchanged by an entry that is not blended), so the hit for a threshold t is the
first k with final_T_k <= t and its id is ids[start + k - 1]; k runs to the longest list.  top_idx, top_vis and count
come from W[p, g] = vis(p, g) (identity colours over a zero background, as in lift_ref): the argmax is taken in list
order, the earliest on equal values."""
import numpy as np

import lift_ref

THRESHOLDS = (0.1, 0.5, 0.9)


def pixel_tiles(h, w):
    """(h, w) tile number of every pixel"""
    tiles_x = (w + 15) // 16
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy // 16) * tiles_x + xx // 16


def weights(O, ids, tile_bins, xys, conics, opacity, h, w):
    """W (h, w, N) float32 = vis, and the forward's final_T, on explicit lists"""
    n = xys.shape[0]
    W, ft, _ = O.blend_fwd(ids, tile_bins, xys, conics, np.eye(n, dtype=np.float32), opacity, h, w,
                           np.zeros(n, np.float32))
    return W, ft


class Ref:
    """hit[t] (h, w) int32 ids, pos[t] (h, w) 1-based list position of the hit (0: none), top_idx, top_vis, count,
    final_T — of one set of lists, for the thresholds given (float32 comparisons)."""

    def __init__(self, O, ids, tile_bins, xys, conics, opacity, h, w, thresholds=THRESHOLDS, W=None, final_T=None):
        ids = np.ascontiguousarray(ids, np.int32)
        tile_bins = np.ascontiguousarray(tile_bins, np.int32).reshape(-1, 2)
        n = xys.shape[0]
        self.h, self.w = h, w
        if W is None:
            W, final_T = weights(O, ids, tile_bins, xys, conics, opacity, h, w)
        self.final_T = final_T
        tile = pixel_tiles(h, w)
        start, end = tile_bins[:, 0], tile_bins[:, 1]
        longest = int((end - start).max(initial=0))
        ts = [np.float32(t) for t in thresholds]
        self.pos = {float(t): np.zeros((h, w), np.int32) for t in thresholds}
        one = np.zeros((n, 1), np.float32)
        last = np.ones((h, w), np.float32)
        for k in range(1, longest + 1):
            cut = np.stack([start, np.minimum(end, start + k)], axis=1).astype(np.int32)
            _, last, _ = O.blend_fwd(ids, cut, xys, conics, one, opacity, h, w, np.zeros(1, np.float32))
            for t, key in zip(ts, self.pos):
                p = self.pos[key]
                p[(p == 0) & (last <= t)] = k
        self.last_prefix_T = last
        self.hit = {}
        for key, p in self.pos.items():
            e = np.clip(start[tile] + p - 1, 0, max(len(ids) - 1, 0))
            self.hit[key] = np.where(p > 0, ids[e] if len(ids) else -1, -1).astype(np.int32)
        # the largest vis in list order, and the number of blended entries
        self.top_idx = np.full((h, w), -1, np.int32)
        self.top_vis = np.zeros((h, w), np.float32)
        self.count = (W > 0).sum(axis=-1).astype(np.int32)
        self.ties = 0
        for t in range(len(tile_bins)):
            lst = ids[start[t]:end[t]]
            sel = tile == t
            if len(lst) == 0 or not sel.any():
                continue
            Wt = W[sel][:, lst]                                   # (pixels, list order)
            k = Wt.argmax(axis=1)                                 # the first of equal values
            v = Wt[np.arange(len(k)), k]
            self.ties += int(((Wt == v[:, None]).sum(axis=1) > 1)[v > 0].sum())
            self.top_idx[sel] = np.where(v > 0, lst[k], -1)
            self.top_vis[sel] = v
        for a in (self.top_idx, self.top_vis, self.count, self.final_T, *self.hit.values(), *self.pos.values()):
            a.setflags(write=False)


_refs = {}


def scene_ref(O, name):
    """(lift_ref.Case, Ref) of one of lift_ref's scenes, computed once per session and never modified"""
    if name not in _refs:
        c = lift_ref.case(O, name)
        p, b = c.proj, c.bins
        _refs[name] = (c, Ref(O, b["gaussian_ids_sorted"], b["tile_bins"], p["xys"], p["conics"], p["opacity"], c.h,
                              c.w, W=c.W, final_T=c.final_T))
    return _refs[name]


def case_ref(O, case):
    """Ref of a constructed case (hits_cases.Case) at its own threshold, cached"""
    key = ("case", case.name)
    if key not in _refs:
        _refs[key] = Ref(O, case.ids, case.tile_bins, case.xys, case.conics, case.opacity, case.h, case.w,
                         (case.t_hit,))
    return _refs[key]
