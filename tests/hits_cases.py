"""Constructed inputs for gg_blend_hits: hand-made xys / conics / opacity / ids / tile_bins, as the C ABI takes them.

A stack is a run of equal Gaussians centred on an integer pixel: there sigma = 0, gg_exp(0) = 1 and alpha = opacity
exactly, so T after k entries of opacity a is the fp32 product chain (1 - a)^k and the list position of the hit at the
centre pixel can be chosen.  Gaussian ids are a permutation of the list positions, so an id is never its position."""
import numpy as np

ALPHA_MIN = np.float32(1.0) / np.float32(255.0)
HIT_POSITIONS = (1, 4, 5, 63, 64, 65, 127, 128, 129)     # group-of-four and 64-entry chunk boundaries


class Case:
    def __init__(self, name, h, w, t_hit, probe, expect_pos):
        self.name, self.h, self.w, self.t_hit = name, h, w, float(t_hit)
        self.probe, self.expect_pos = probe, expect_pos   # pixel (u, v) and the hit's 1-based list position there (0: none)
        self.tiles_x, self.tiles_y = (w + 15) // 16, (h + 15) // 16
        self._g = []                                      # (tile, x, y, conic (3,), opacity)

    def add(self, tile, x, y, conic, opacity):
        self._g.append((tile, float(x), float(y), tuple(conic), float(opacity)))
        return self

    def stack(self, tile, x, y, conic, opacities):
        for a in opacities:
            self.add(tile, x, y, conic, a)
        return self

    def finish(self):
        n = len(self._g)
        step = next(s for s in (7, 11, 13, 17, 19, 23) if n % s != 0)
        perm = (np.arange(n) * step + 3) % n              # list position -> Gaussian id (a bijection)
        if n > 1:
            assert len(set(perm.tolist())) == n
        ntiles = self.tiles_x * self.tiles_y
        order = sorted(range(n), key=lambda k: self._g[k][0])          # stable: list order inside a tile
        self.n = n
        self.xys = np.zeros((n, 2), np.float32)
        self.conics = np.zeros((n, 3), np.float32)
        self.opacity = np.zeros((n, 1), np.float32)
        self.ids = np.zeros(n, np.int32)
        self.tile_bins = np.zeros((ntiles, 2), np.int32)
        counts = np.zeros(ntiles, np.int64)
        for e, k in enumerate(order):
            tile, x, y, conic, a = self._g[k]
            g = int(perm[e])
            self.ids[e] = g
            self.xys[g], self.conics[g], self.opacity[g, 0] = (x, y), conic, a
            counts[tile] += 1
        ends = np.cumsum(counts)
        self.tile_bins[:, 1] = ends
        self.tile_bins[:, 0] = ends - counts
        return self


def uniform_opacity(position):
    """The opacity a with (1 - a)^(position - 1) > 0.5 > (1 - a)^position, well inside: the hit at t_hit = 0.5 lands
    at list position `position` of a stack (>= 1/255 up to position 129; the host test asserts the landing)."""
    return float(np.float32(1.0 - 0.5 ** (1.0 / (position - 0.5))))


WIDE = (0.05, 0.0, 0.05)      # reaches every quadrant of the tile for a strong Gaussian, few for a weak one
NARROW = (2.0, 0.0, 2.0)      # about 1.5 pixels: stays inside its quadrant


def hit_at(position):
    c = Case(f"hit_at_{position}", 16, 16, 0.5, (5, 6), position)
    return c.stack(0, 5, 6, WIDE, [uniform_opacity(position)] * (position + 6)).finish()


def stops_before_hit():
    """0.9, 0.9 take T to about 0.01 > t_hit = 0.001; the third (0.999) would take it to 1e-5 <= 1e-4: not blended, the
    walk ends; what follows is never reached."""
    c = Case("stops_before_hit", 16, 16, 0.001, (9, 3), 0)
    return c.stack(0, 9, 3, WIDE, [0.9, 0.9, 0.999, 0.9, 0.9]).finish()


def near_one():
    """t_hit = 0.999.  A blended entry has alpha >= 1/255, so T_after <= 0.9961 <= 0.999: the FIRST BLENDED entry
    always hits at this threshold, whatever its opacity (a first blended entry that does not hit cannot be built).
    What can differ is its list position: two entries that are not blended come first."""
    c = Case("near_one", 16, 16, 0.999, (4, 11), 3)
    below = float(np.nextafter(ALPHA_MIN, np.float32(0)))
    return c.stack(0, 4, 11, WIDE, [below, below, float(ALPHA_MIN), 0.5]).finish()


def skipped_ahead():
    """sigma < 0 (a negative-definite conic off the pixel centres: never culled, never blended) and alpha one ulp
    below 1/255, ahead of the entries that hit."""
    c = Case("skipped_ahead", 16, 16, 0.5, (10, 9), 5)
    below = float(np.nextafter(ALPHA_MIN, np.float32(0)))
    c.add(0, 10.5, 9.5, (-0.1, 0.0, -0.1), 0.9)
    c.add(0, 10, 9, WIDE, below)
    return c.stack(0, 10, 9, WIDE, [0.3, 0.2, 0.4, 0.6]).finish()     # T: 0.7, 0.56, 0.336 -> position 2 + 3


def four_quadrants():
    """One 16x16 tile: four narrow stacks, one per quadrant, share the tile's list.  Their hits lie in chunks 0, 1, 2
    and 3 of that list, so a wave that has its hit (and, in the hit-only build, leaves) must not end another's walk."""
    c = Case("four_quadrants", 16, 16, 0.5, (12, 12), 5 + 70 + 70 + 69)
    c.stack(0, 3, 3, NARROW, [0.4] * 5)                  # hit at 2, chunk 0
    c.stack(0, 12, 3, NARROW, [uniform_opacity(69)] * 70)       # hit at 5 + 69 = 74, chunk 1
    c.stack(0, 3, 12, NARROW, [uniform_opacity(69)] * 70)       # 75 + 69 = 144, chunk 2
    c.stack(0, 12, 12, NARROW, [uniform_opacity(69)] * 70)      # 145 + 69 = 214, chunk 3
    return c.finish()


def empty_between():
    """40 x 37: a ragged 3 x 3 tile grid, lists on tiles 0, 4 and 8 only"""
    c = Case("empty_between", 37, 40, 0.5, (20, 20), 3)
    c.stack(0, 2, 2, WIDE, [0.8, 0.8])
    c.stack(4, 20, 20, WIDE, [0.2, 0.2, 0.3, 0.9])       # T: 0.8, 0.64, 0.448
    c.stack(8, 38, 35, WIDE, [0.6])
    return c.finish()


def all_cases():
    return [hit_at(p) for p in HIT_POSITIONS] + [stops_before_hit(), near_one(), skipped_ahead(), four_quadrants(),
                                                 empty_between()]


_cases = {}


def cases():
    if not _cases:
        for c in all_cases():
            _cases[c.name] = c
    return _cases


NAMES = tuple(f"hit_at_{p}" for p in HIT_POSITIONS) + ("stops_before_hit", "near_one", "skipped_ahead",
                                                       "four_quadrants", "empty_between")


# ------------------------------------------------------------------------------------------------
# the two-layer fixture: a plate in front of a wall
# ------------------------------------------------------------------------------------------------
LAYER_H, LAYER_W = 48, 64
LAYER_K = (50.0, 50.0, 31.5, 23.5)
PLATE_Z, WALL_Z = 1.0, 2.0
PLATE_EDGE = 0.0            # the plate covers x <= PLATE_EDGE: the left half of the image


def two_layer_scene():
    """A fronto-parallel plate of opaque Gaussians at depth 1 over the left half of the view, in front of a wall at
    depth 2, seen by a camera at the origin looking down -z (OpenGL c2w = identity).  Returns (Scene, camera tuple,
    is_plate (N,) bool).  At the plate's edge a pixel blends both layers: the expected depth D / A lies between them
    (tests/test_hits_host.py holds that on the oracle), the median depth is one of the two."""
    import torch
    from gaussiangrasper_amd.scene import Scene

    def layer(x0, x1, y0, y1, step, z, sxy):
        xs, ys = np.arange(x0, x1 + 1e-9, step), np.arange(y0, y1 + 1e-9, step)
        gx, gy = np.meshgrid(xs, ys)
        m = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, -z)], axis=1)
        return m, np.tile([sxy, sxy, 0.003], (len(m), 1))

    pm, ps = layer(-0.72, PLATE_EDGE, -0.56, 0.56, 0.04, PLATE_Z, 0.03)
    wm, ws = layer(-1.44, 1.44, -1.12, 1.12, 0.08, WALL_Z, 0.06)
    means = np.concatenate([pm, wm]).astype(np.float32)
    scales = np.concatenate([ps, ws]).astype(np.float32)
    n = len(means)
    quats = np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (n, 1))
    sc = Scene(torch.from_numpy(means), torch.log(torch.from_numpy(scales)), torch.from_numpy(quats),
               torch.full((n, 1), 4.0), torch.zeros(n, 1, 3), torch.zeros(n, 1))
    is_plate = np.arange(n) < len(pm)
    return sc, (np.eye(4), LAYER_K, LAYER_H, LAYER_W), is_plate
