"""A numpy restatement of gg_field_sight and gg_field_shortcut (include/gg_raster.h "Line of sight") that does NOT
walk: the cover of a segment is found by testing every cell of the bounding box of its ends against the segment with
the slab method in integers.  In doubled coordinates the centres are A = 2 a + 1 and B = 2 b + 1, the closed cube of
cell c is [2 c, 2 c + 2]^3, and the parameters at which the segment enters and leaves a slab are fractions over
D_a = B_a - A_a; scaled by M = the product of the |D_a| that are not 0 they are integers (below 2^44 for dims up to
1024), and the closed comparison max(enter) <= min(exit) decides.  `sight` and the greedy `shortcut` sit on top of it.

`cover_walk` is a second implementation, written as the boundary walk the header describes; test_shortcut_host.py
holds the two to equality."""
import numpy as np


def free_cells(dist2, need):
    return np.asarray(dist2, np.int64) >= int(need)


def meets(a, b, cells):
    """(S, N) bool: the closed cube of cells[n] meets the closed segment between the centres of a[s] and b[s].
    a, b (S, 3), cells (N, 3), integers."""
    A = 2 * np.asarray(a, np.int64).reshape(-1, 1, 3) + 1
    B = 2 * np.asarray(b, np.int64).reshape(-1, 1, 3) + 1
    lo = 2 * np.asarray(cells, np.int64).reshape(1, -1, 3)
    D = B - A
    M = np.where(D != 0, np.abs(D), 1).prod(axis=2, keepdims=True)           # (S, 1, 1)
    q = np.where(D != 0, np.sign(D) * (M // np.where(D != 0, np.abs(D), 1)), 0)      # M / D_a, exact
    t0, t1 = (lo - A) * q, (lo + 2 - A) * q                                  # M t at the slab's two faces
    inside = (lo <= A) & (A <= lo + 2)                                        # an axis the segment does not move along
    enter = np.where(D != 0, np.minimum(t0, t1), 0)
    leave = np.where(D != 0, np.maximum(t0, t1), np.where(inside, M, -1))
    return np.maximum(enter.max(axis=2), 0) <= np.minimum(leave.min(axis=2), M[:, :, 0])


def box_cells(lo, hi):
    """(N, 3) int64: every cell c with lo <= c <= hi"""
    ax = [np.arange(int(lo[k]), int(hi[k]) + 1) for k in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def cover(a, b):
    """(K, 3) int64, sorted: the cells of cover(a, b)"""
    a, b = np.asarray(a, np.int64).reshape(3), np.asarray(b, np.int64).reshape(3)
    box = box_cells(np.minimum(a, b), np.maximum(a, b))
    return box[meets(a, b, box)[0]]


def cover_walk(a, b):
    """the same set by the boundary walk: crossings ordered by cross-multiplication, a tie opens every cell it
    touches"""
    a, b = [int(v) for v in np.asarray(a).reshape(3)], [int(v) for v in np.asarray(b).reshape(3)]
    n = [abs(b[k] - a[k]) for k in range(3)]
    s = [1 if b[k] > a[k] else -1 for k in range(3)]
    c, k = list(a), [0, 0, 0]
    out = [tuple(c)]
    while sum(k) < sum(n):
        live = [x for x in range(3) if k[x] < n[x]]
        # t_x = (2 k_x + 1) / (2 n_x): x is first iff t_x <= t_y for every live y
        first = [x for x in live if all((2 * k[x] + 1) * n[y] <= (2 * k[y] + 1) * n[x] for y in live)]
        for e in range(1, 1 << len(first)):
            cell = list(c)
            for bit, x in enumerate(first):
                if e >> bit & 1:
                    cell[x] += s[x]
            out.append(tuple(cell))
        for x in first:
            c[x] += s[x]
            k[x] += 1
    return np.array(sorted(out), np.int64).reshape(-1, 3)


def _inside(cells, dims):
    c = np.asarray(cells, np.int64).reshape(-1, 3)
    return ((c >= 0) & (c < np.asarray(dims, np.int64))).all(1)


def sight_from(free, a, targets):
    """(cover, blocked) int32 (K,) of the segments a -> targets[k], all tested against ONE box of cells"""
    free = np.asarray(free, bool)
    a = np.asarray(a, np.int64).reshape(3)
    t = np.asarray(targets, np.int64).reshape(-1, 3)
    cov, blk = np.zeros(len(t), np.int32), np.full(len(t), -1, np.int32)
    ok = _inside(t, free.shape) & bool(_inside(a, free.shape)[0])
    if ok.any():
        ends = np.concatenate([a[None], t[ok]])
        box = box_cells(ends.min(0), ends.max(0))
        hit = meets(np.broadcast_to(a, (int(ok.sum()), 3)), t[ok], box)
        cov[ok] = hit.sum(1)
        blk[ok] = (hit & ~free[tuple(box.T)][None]).sum(1)
    return cov, blk


def sight(dist2, need, a, b):
    """(cover int32 [S], blocked int32 [S]): the contract of gg_field_sight"""
    free = free_cells(dist2, need)
    a, b = np.asarray(a, np.int64).reshape(-1, 3), np.asarray(b, np.int64).reshape(-1, 3)
    cov, blk = np.zeros(len(a), np.int32), np.full(len(a), -1, np.int32)
    for s in range(len(a)):
        c, k = sight_from(free, a[s], b[s:s + 1])
        cov[s], blk[s] = c[0], k[0]
    return cov, blk


def sight_all_pairs(dist2, need, chunk=2048):
    """(a, b, cover, blocked) of every ordered pair of cells of a small volume, every pair against every cell"""
    free = free_cells(dist2, need)
    cells = box_cells((0, 0, 0), np.array(free.shape) - 1)
    ia, ib = np.meshgrid(np.arange(len(cells)), np.arange(len(cells)), indexing="ij")
    a, b = cells[ia.reshape(-1)], cells[ib.reshape(-1)]
    shut = ~free.reshape(-1)
    cov, blk = np.zeros(len(a), np.int32), np.zeros(len(a), np.int32)
    for at in range(0, len(a), chunk):
        hit = meets(a[at:at + chunk], b[at:at + chunk], cells)
        cov[at:at + chunk] = hit.sum(1)
        blk[at:at + chunk] = (hit & shut[None]).sum(1)
    return a, b, cov, blk


def shortcut(dist2, need, cells, length, window):
    """(keep int32 [P][max_cells], count int32 [P], blocked int32 [P]): the contract of gg_field_shortcut"""
    free = free_cells(dist2, need)
    cells = np.asarray(cells, np.int64)
    P, max_cells = cells.shape[:2]
    keep = np.full((P, max_cells), -1, np.int32)
    count, blocked = np.zeros(P, np.int32), np.zeros(P, np.int32)
    for p in range(P):
        n = min(int(length[p]), max_cells)
        if n <= 0:
            continue
        anchors, i = [0], 0
        while i < n - 1:
            far = min(i + int(window), n - 1)
            _, blk = sight_from(free, cells[p, i], cells[p, i + 1:far + 1])
            clear = np.nonzero(blk == 0)[0]
            if len(clear):
                i = i + 1 + int(clear[-1])                  # the largest clear j, whatever lies before it
            else:
                i, blocked[p] = i + 1, blocked[p] + 1
            anchors.append(i)
        count[p] = len(anchors)
        keep[p, :len(anchors)] = anchors
        keep[p, len(anchors):] = n - 1
    return keep, count, blocked


def clear_walk(free, a, b):
    """is the segment clear, by the boundary walk (both ends inside the volume)"""
    return all(free[tuple(c)] for c in cover_walk(a, b))


def shortcut_by_walk(dist2, need, cells, length, window):
    """the same contract the way a host program would do it: candidates from the far end, one walk each"""
    free = free_cells(dist2, need)
    cells = np.asarray(cells, np.int64)
    P, max_cells = cells.shape[:2]
    keep = np.full((P, max_cells), -1, np.int32)
    count, blocked = np.zeros(P, np.int32), np.zeros(P, np.int32)
    inside = _inside(cells.reshape(-1, 3), free.shape).reshape(P, max_cells)
    for p in range(P):
        n = min(int(length[p]), max_cells)
        if n <= 0:
            continue
        anchors, i = [0], 0
        while i < n - 1:
            for j in range(min(i + int(window), n - 1), i, -1):
                if inside[p, i] and inside[p, j] and clear_walk(free, cells[p, i], cells[p, j]):
                    break
            else:
                j, blocked[p] = i + 1, blocked[p] + 1
            anchors.append(j)
            i = j
        count[p] = len(anchors)
        keep[p, :len(anchors)] = anchors
        keep[p, len(anchors):] = n - 1
    return keep, count, blocked


def kept_length(cells, keep, count):
    """the length, in cells, of the polyline through the centres of the kept rows of one path"""
    return polyline_length(np.asarray(cells)[np.asarray(keep)[:int(count)]])


# ------------------------------------------------------------------------------------------------
# fixtures the host and the GPU tests share
# ------------------------------------------------------------------------------------------------
NEED = 4
OPEN, SHUT = 100, 0                                # dist2 of a cell that is free / not free at NEED


def wall_and_door(seed=0, clutter=0.02):
    """(40, 36, 44): a wall one cell thick at x == 20 with a 3 x 3 door, and random clutter on either side"""
    rng = np.random.default_rng(seed)
    d = np.where(rng.random((40, 36, 44)) < clutter, SHUT, OPEN).astype(np.int32)
    d[20] = SHUT
    d[20, 16:19, 20:23] = OPEN
    return d


def comb(n, clear_at):
    """A volume and a hand-made path of n rows on which sight from row 0 is NOT monotone: row y == 1 is shut from
    x == 1 on, so from (0, 0, 0) every cell (x, 0, 0) is in sight along the open row y == 0 and no cell (x, 3, 0),
    x >= 3, is (its segment is in the row y == 1 for t in [1/6, 1/2], at x >= 1).  The path's rows 1.. are such cells
    (x, 3, 0), except row clear_at, which is (clear_at, 0, 0)."""
    d = np.full((n + 3, 4, 1), OPEN, np.int32)
    d[1:, 1] = SHUT
    cells = np.array([[0, 0, 0]] + [[j + 2, 3, 0] for j in range(1, n)], np.int32)
    cells[clear_at] = (clear_at, 0, 0)
    return d, cells[None]


def polyline_length(points):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    return float(np.linalg.norm(np.diff(p, axis=0), axis=1).sum())
