"""A numpy / scipy restatement of gg_field_route and gg_field_descend (include/gg_raster.h "Transit planning"): the
allowed-move graph of a dist2 volume, scipy's Dijkstra from the goals (integer weights 3, 4, 5: exact in float64), and
the descent as a Python loop with the move-number tie rule."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import dijkstra

FAR = 1 << 30
MOVES = [(m, m // 9 - 1, (m // 3) % 3 - 1, m % 3 - 1) for m in range(27) if m != 13]


def weight(m):
    return 2 + sum(1 for d in (m // 9 - 1, (m // 3) % 3 - 1, m % 3 - 1) if d != 0)


def free_cells(dist2, need):
    return np.asarray(dist2, np.int64) >= int(need)


def _shift(a, dx, dy, dz):
    """out[c] = a[c + d], False where c + d is outside"""
    X, Y, Z = a.shape
    out = np.zeros_like(a)
    sx, tx = (slice(max(0, -dx), X - max(0, dx)), slice(max(0, dx), X - max(0, -dx)))
    sy, ty = (slice(max(0, -dy), Y - max(0, dy)), slice(max(0, dy), Y - max(0, -dy)))
    sz, tz = (slice(max(0, -dz), Z - max(0, dz)), slice(max(0, dz), Z - max(0, -dz)))
    out[sx, sy, sz] = a[tx, ty, tz]
    return out


def allowed(dist2, need):
    """(27, X, Y, Z) bool: move m from cell c is allowed iff every c + e, e_a in {0, d_a}, is free"""
    free = free_cells(dist2, need)
    out = np.zeros((27,) + free.shape, bool)
    for m, dx, dy, dz in MOVES:
        ok = np.ones(free.shape, bool)
        for ex in {0, dx}:
            for ey in {0, dy}:
                for ez in {0, dz}:
                    ok &= _shift(free, ex, ey, ez)
        out[m] = ok
    return out


def graph(dist2, need):
    """csr matrix of the allowed moves, entry [c, c + d] = the move's weight (flat C-order cell indices)"""
    al = allowed(dist2, need)
    X, Y, Z = al.shape[1:]
    idx = np.arange(X * Y * Z).reshape(X, Y, Z)
    rows, cols, vals = [], [], []
    for m, dx, dy, dz in MOVES:
        src = idx[al[m]]
        rows.append(src)
        cols.append(src + (dx * Y + dy) * Z + dz)
        vals.append(np.full(len(src), weight(m), np.float64))
    n = X * Y * Z
    return coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()


def goals_taking_part(dist2, need, goals):
    """(flat indices of the goals that take part, the number ignored)"""
    free = free_cells(dist2, need)
    g = np.asarray(goals, np.int64).reshape(-1, 3)
    dims = np.array(free.shape)
    inside = ((g >= 0) & (g < dims)).all(1)
    part = inside.copy()
    part[inside] = free[tuple(g[inside].T)]
    flat = (g[part] * [dims[1] * dims[2], dims[2], 1]).sum(1)
    return flat, int((~part).sum())


def route(dist2, need, goals):
    """(cost int32 [X][Y][Z], ignored): the contract of gg_field_route"""
    d = np.asarray(dist2)
    flat, ignored = goals_taking_part(d, need, goals)
    cost = np.full(d.shape, FAR, np.int32)
    if len(flat) == 0:
        return cost, ignored
    # the moves are symmetric (d from c and -d from c + d need the same cells), so to-goal equals from-goal
    dist = dijkstra(graph(d, need), directed=True, indices=np.unique(flat), min_only=True)
    fin = np.isfinite(dist)
    assert (dist[fin] == np.rint(dist[fin])).all() and (dist[fin] < FAR).all()
    cost.reshape(-1)[fin] = dist[fin].astype(np.int32)
    assert (cost[~free_cells(d, need)] == FAR).all()
    return cost, ignored


def descend(dist2, need, cost, starts, max_cells):
    """(cells int32 [P][max_cells][3], length int32 [P]): the contract of gg_field_descend"""
    d, cost = np.asarray(dist2), np.asarray(cost)
    free = free_cells(d, need)
    dims = free.shape
    starts = np.asarray(starts, np.int64).reshape(-1, 3)
    cells = np.full((len(starts), max_cells, 3), -1, np.int32)
    length = np.zeros(len(starts), np.int32)

    def is_free(c):
        return all(0 <= c[a] < dims[a] for a in range(3)) and bool(free[tuple(c)])

    for p, s in enumerate(starts):
        c = tuple(int(v) for v in s)
        if not is_free(c) or cost[c] >= FAR:
            continue
        path = [c]
        while cost[c] > 0:
            for m, dx, dy, dz in MOVES:                          # in move-number order: the tie rule
                block = [(c[0] + ex, c[1] + ey, c[2] + ez) for ex in {0, dx} for ey in {0, dy} for ez in {0, dz}]
                n = (c[0] + dx, c[1] + dy, c[2] + dz)
                if all(is_free(b) for b in block) and int(cost[n]) + weight(m) == int(cost[c]):
                    c = n
                    break
            else:
                raise AssertionError(f"no move fits at {c}: cost is no fixed point")
            path.append(c)
        length[p] = len(path)
        k = min(len(path), max_cells)
        cells[p, :k] = path[:k]
        cells[p, k:] = path[-1]
    return cells, length
