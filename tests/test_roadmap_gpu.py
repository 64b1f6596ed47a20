"""The arm roadmap on the GPU: gg_roadmap_neighbours, gg_roadmap_route and gg_roadmap_descend held to equality with the
numpy restatement (tests/roadmap_ref.py) through the C entries, their memory contract in a sentinel arena
(tests/arena.py), and the task layer of gaussiangrasper_amd/roadmap.py on the fixture whose claims
tests/test_roadmap_host.py establishes."""
import ctypes as C

import numpy as np
import pytest
import torch

import roadmap_ref as rr
from arena import Arena

gpu = pytest.mark.gpu
DEV = "cuda"
FAR = rr.FAR
TILE = 256
NOT_CONVERGED = -5


def _lib():
    from gaussiangrasper_amd import _lib as L
    return L.load()


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _host(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    return a, a.ctypes.data_as(C.c_void_p)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def nb(nodes, queries, metric, k, skip=None, valid=None):
    nodes, queries = np.asarray(nodes, np.float64), np.asarray(queries, np.float64)
    J = queries.shape[1]
    N, M = len(nodes), len(queries)
    n, q = _dev(nodes.reshape(N, J), np.float64), _dev(queries, np.float64)
    keep, mp = _host(metric, np.float64)
    s = None if skip is None else _dev(skip, np.int32)
    v = None if valid is None else _dev(valid, np.uint8)
    idx = torch.full((M, k), -77, dtype=torch.int32, device=DEV)
    d2 = torch.full((M, k), -77.0, dtype=torch.float64, device=DEV)
    st = _lib().gg_roadmap_neighbours(J, N, _p(n), M, _p(q), mp, _p(s), _p(v), k, _p(idx), _p(d2), _stream())
    assert st == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d2.cpu().numpy()


def same_neighbours(got, want):
    assert np.array_equal(got[0], want[0])
    nan = np.isnan(want[1])
    assert np.array_equal(np.isnan(got[1]), nan)
    assert got[1][~nan].tobytes() == want[1][~nan].tobytes()        # to the bit: the same operations, no contraction


def check_nb(nodes, queries, metric, k, skip=None, valid=None):
    got = nb(nodes, queries, metric, k, skip, valid)
    J = np.asarray(queries).shape[1]
    same_neighbours(got, rr.neighbours(np.asarray(nodes, np.float64).reshape(len(nodes), J), queries, metric, k, skip,
                                       valid))
    return got


# ------------------------------------------------------------------------------------------------
# neighbours
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("J", [1, 2, 7, 8])
def test_neighbours_over_joint_counts_list_lengths_and_node_counts(J):
    rng = np.random.default_rng(100 + J)
    metric = rng.uniform(0.1, 1.5, J)
    for k in (1, 2, 16, 32):
        for N in (0, 1, 2, k, k + 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 1025, 4099):
            nodes = rng.uniform(-3, 3, size=(N, J))
            queries = rng.uniform(-3, 3, size=(5, J))
            check_nb(nodes, queries, metric, k)


@gpu
@pytest.mark.parametrize("M", [1, 64, 65, 1025])
def test_neighbours_over_query_counts(M):
    rng = np.random.default_rng(M)
    nodes, queries = rng.uniform(-3, 3, size=(777, 7)), rng.uniform(-3, 3, size=(M, 7))
    skip = rng.integers(-1, 777, M)
    valid = rng.uniform(size=777) < 0.8
    check_nb(nodes, queries, rng.uniform(0.1, 1.5, 7), 16, skip, valid)


@gpu
def test_neighbours_ties_go_to_the_lowest_index():
    # an integer lattice of 33 x 33 nodes: exact ties everywhere, tiles end inside rings of equal distance
    side = 33
    lat = np.array([[x, y] for x in range(side) for y in range(side)], np.float64)
    assert len(lat) > 4 * TILE
    rng = np.random.default_rng(5)
    queries = np.concatenate([lat[rng.integers(0, len(lat), 40)], lat[rng.integers(0, len(lat), 20)] + 0.5])
    idx, d2 = check_nb(lat, queries, np.ones(2), 16)
    ties = (np.diff(d2, axis=1) == 0)
    assert ties.sum() > 300 and (np.diff(idx, axis=1)[ties] > 0).all()
    # a tie across a tile boundary: nodes TILE - 1 and TILE at the same distance
    nodes = np.arange(600, dtype=np.float64)[:, None]
    q = np.array([[TILE - 0.5]])
    idx, d2 = check_nb(nodes, q, np.ones(1), 4)
    assert idx[0].tolist() == [TILE - 1, TILE, TILE - 2, TILE + 1] and d2[0].tolist() == [0.25, 0.25, 2.25, 2.25]
    # shuffled so that the lower index of a tie comes from the later tile's side of the sort: still the lowest index
    perm = rng.permutation(len(lat))
    check_nb(lat[perm], queries, np.ones(2), 32)
    # 200 identical nodes
    same = np.tile(rng.uniform(-1, 1, size=(1, 7)), (200, 1))
    idx, d2 = check_nb(same, same[:3], np.ones(7), 32, skip=np.array([-1, 3, 199]))
    assert idx[0].tolist() == list(range(32)) and idx[1].tolist() == [0, 1, 2] + list(range(4, 33)) and (d2 == 0).all()


@gpu
def test_neighbours_when_every_candidate_inserts_and_when_none_does():
    N = 1500
    far_first = np.arange(N, 0, -1, dtype=np.float64)[:, None]      # descending distance from 0: every node inserts
    near_first = far_first[::-1].copy()                             # ascending: none inserts after the first k
    q = np.zeros((3, 1))
    for k in (1, 16, 32):
        idx, _ = check_nb(far_first, q, np.ones(1), k)
        assert idx[0].tolist() == list(range(N - 1, N - 1 - k, -1))
        idx, _ = check_nb(near_first, q, np.ones(1), k)
        assert idx[0].tolist() == list(range(k))


@gpu
def test_neighbours_masks_skips_and_values_that_are_not_finite():
    rng = np.random.default_rng(8)
    N, M, J, k = 700, 40, 7, 16
    nodes, queries = rng.uniform(-3, 3, size=(N, J)), rng.uniform(-3, 3, size=(M, J))
    metric = rng.uniform(0.1, 1.5, J)
    metric[2] = 0.0                                                 # a joint that does not count
    idx, _ = check_nb(nodes, queries, metric, k)
    moved = nodes.copy()
    moved[:, 2] += rng.uniform(-5, 5, N)
    assert np.array_equal(nb(moved, queries, metric, k)[0], idx)
    check_nb(nodes, queries, np.zeros(J), k)                        # all zero: every node at distance 0, the lowest k
    for valid in (np.zeros(N, bool), np.arange(N) % 2 == 0, np.arange(N) == N - 1, rng.uniform(size=N) < 0.5,
                  np.arange(N) < 5, (np.arange(N) % 3).astype(np.uint8) * 100):
        got = check_nb(nodes, queries, metric, k, valid=valid)
        assert (np.asarray(valid)[got[0][got[0] >= 0]] != 0).all()
    few = check_nb(nodes, queries, metric, k, valid=np.arange(N) < 5)
    assert (few[0][:, 5:] == -1).all() and np.isinf(few[1][:, 5:]).all() and (few[0][:, :5] >= 0).all()
    plain = check_nb(nodes, queries, metric, k, skip=np.full(M, -1))
    same_neighbours(plain, nb(nodes, queries, metric, k, skip=None))
    named = check_nb(nodes, queries, metric, k, skip=plain[0][:, 0])
    assert np.array_equal(named[0][:, :k - 1], plain[0][:, 1:])     # without its nearest, the list moves up by one
    # a NaN and an inf inside one node each, a node at 1e200 whose d2 overflows: none is a neighbour
    odd = nodes.copy()
    first = plain[0][:, 0]
    odd[first[0], 3] = np.nan
    odd[first[1], 0] = np.inf
    odd[first[2], 6] = -np.inf
    odd[first[3]] = 1e200
    odd[first[4], 2] = np.nan                                       # under the zero metric entry: still not finite
    got = check_nb(odd, queries, metric, k)
    assert not np.isin(first[:5], got[0]).any() and np.isfinite(got[1]).all()
    # a query that is not finite: -1 and NaN, its neighbours in the batch as they were
    qq = queries.copy()
    qq[1, 4], qq[7, 0], qq[9, 2] = np.nan, np.inf, np.nan
    got = check_nb(nodes, qq, metric, k)
    assert (got[0][[1, 7, 9]] == -1).all() and np.isnan(got[1][[1, 7, 9]]).all()
    assert np.array_equal(np.delete(got[0], [1, 7, 9], 0), np.delete(plain[0], [1, 7, 9], 0))


@gpu
def test_neighbours_of_the_nodes_themselves_and_twice_the_same_bytes():
    rng = np.random.default_rng(12)
    nodes = rng.uniform(-3, 3, size=(1000, 7))
    nodes[500] = nodes[20]                                          # a node equal to another under another index
    metric = rng.uniform(0.1, 1.5, 7)
    with_self = check_nb(nodes, nodes, metric, 8)
    assert (with_self[1][:, 0] == 0).all()
    assert with_self[0][20, :2].tolist() == [20, 500] and with_self[0][500, :2].tolist() == [20, 500]
    without = check_nb(nodes, nodes, metric, 8, skip=np.arange(1000))
    assert (without[0] != np.arange(1000)[:, None]).all()
    assert without[0][20, 0] == 500 and without[1][20, 0] == 0 and without[0][500, 0] == 20
    again = nb(nodes, nodes, metric, 8, skip=np.arange(1000))
    assert again[0].tobytes() == without[0].tobytes() and again[1].tobytes() == without[1].tobytes()
    # the task layer's call: queries None is the nodes against themselves, each skipping itself
    from gaussiangrasper_amd import roadmap as R
    idx, d2 = R.neighbours(nodes, 8, metric)
    assert idx.cpu().numpy().tobytes() == without[0].tobytes() and d2.cpu().numpy().tobytes() == without[1].tobytes()


# ------------------------------------------------------------------------------------------------
# route and descend
# ------------------------------------------------------------------------------------------------
def route_call(N, off, tg, w, max_weight, go, goals, max_rounds=None):
    lib = _lib()
    Q = len(go) - 1
    o, t, ww = _dev(off, np.int32), _dev(tg, np.int32), _dev(w, np.int32)
    keep, gp = _host(go, np.int32)
    g = _dev(goals, np.int32)
    cost = torch.full((Q, N), -77, dtype=torch.int32, device=DEV)
    ignored = torch.full((1,), -77, dtype=torch.int64, device=DEV)
    nbytes = lib.gg_roadmap_route_workspace(N, Q)
    assert nbytes > 0
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    ws = ws[-ws.data_ptr() % 256:][:nbytes]
    rounds = C.c_int(-1)
    st = lib.gg_roadmap_route(N, len(tg), _p(o), _p(t), _p(ww), max_weight, Q, gp, _p(g), _p(cost), _p(ignored),
                              N + 1 if max_rounds is None else max_rounds, C.byref(rounds), _p(ws), nbytes, _stream())
    torch.cuda.synchronize()
    return st, cost.cpu().numpy(), int(ignored.item()), rounds.value


def check_route(N, off, tg, w, max_weight, go, goals):
    st, cost, ignored, rounds = route_call(N, off, tg, w, max_weight, go, goals)
    assert st == 0, _lib().gg_last_error()
    want, want_ignored = rr.route(N, off, tg, w, max_weight, go, goals)
    assert np.array_equal(cost, want) and ignored == want_ignored
    assert 1 <= rounds <= N + 1
    return cost


def path_graph(N, weight=3):
    rows = [[(j, weight) for j in (i - 1, i + 1) if 0 <= j < N] for i in range(N)]
    return rr.csr_from_lists(rows)


@gpu
def test_route_on_a_path_graph_and_when_the_rounds_run_out():
    N = 1025
    off, tg, w = path_graph(N)
    cost = check_route(N, off, tg, w, 3, [0, 1, 3], [0, 0, N - 1])
    assert cost[0].tolist() == [3 * i for i in range(N)]
    assert cost[1].tolist() == [3 * min(i, N - 1 - i) for i in range(N)]
    # one round: not converged, and every value below FAR is the weight of a real walk
    go, goals = [0, 1, 3], [0, 0, N - 1]
    st, part, _, rounds = route_call(N, off, tg, w, 3, go, goals, max_rounds=1)
    assert st == NOT_CONVERGED and rounds == 1 and b"max_rounds" in _lib().gg_last_error()
    assert (part >= cost).all() and (part < FAR).any() and (part == FAR).any()
    assert (part[part < FAR] % 3 == 0).all()
    assert rr.is_upper_bound_of_walks(N, off, tg, w, 3, go, goals, part)
    # twice: the same bytes, although the rounds may differ
    a = route_call(N, off, tg, w, 3, go, goals)
    b = route_call(N, off, tg, w, 3, go, goals)
    assert a[0] == b[0] == 0 and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] == 0


@gpu
def test_route_rows_of_every_length_ignored_edges_and_goal_sets():
    rng = np.random.default_rng(31)
    N, max_w = 400, 50
    degrees = [0, 1, 63, 64, 65, 300]
    rows = []
    for i in range(N):
        deg = degrees[i] if i < len(degrees) else int(rng.integers(0, 6))
        rows.append([(int(rng.integers(0, N)), int(rng.integers(1, max_w + 1))) for _ in range(deg)])
    rows[10] = [(10, 1), (11, 7), (11, 2), (11, 9), (12, 50)]      # a self loop, parallel edges of different weights
    rows[11] = [(12, 0), (12, max_w + 1), (-1, 3), (N, 3), (13, 4)] # ignored: weight 0, too heavy, target -1, target N
    rows[5][100] = (-1, 1)
    rows[5][299] = (N, max_w)
    # a component nothing leads out of towards the rest: its nodes are exactly FAR for goals outside it
    for i in range(380, 400):
        rows[i] = [(380 + int(rng.integers(0, 20)), 1)]
    off, tg, w = rr.csr_from_lists(rows)
    goals = np.array([13, 13, 13, -1, N, 2 ** 30, 200, 385, 7, 7], np.int32)     # duplicates, out of range
    for Q in (1, 3, 64, 65):
        go = np.zeros(Q + 1, np.int32)
        cuts = np.sort(rng.integers(0, len(goals) + 1, Q - 1)) if Q > 1 else np.zeros(0, np.int64)
        go[1:Q], go[Q] = cuts, len(goals)
        if Q >= 3:
            go[2] = go[1]                                           # a query with no goal
        cost = check_route(N, off, tg, w, max_w, go, goals)
        if Q >= 3:
            assert (cost[1] == FAR).all()
    cost = check_route(N, off, tg, w, max_w, [0, 1, 4, 6], [13, 3, 4, 5, -1, N])
    assert cost[0, 10] == 2 + 4 and cost[0, 11] == 4 and (cost[0, 380:] == FAR).all() and (cost[2] == FAR).all()
    _, _, ignored, _ = route_call(N, off, tg, w, max_w, [0, 1], [13])
    assert ignored == 6
    # no nodes, no queries
    st, cost, ignored, _ = route_call(0, [0], [], [], 1, [0, 1], [0])
    assert st == 0 and cost.shape == (1, 0) and ignored == 0
    st, cost, ignored, _ = route_call(N, off, tg, w, max_w, [0], [])
    assert st == 0 and ignored == 6


@gpu
def test_route_on_a_random_neighbour_graph():
    N = 4096
    off, tg, w = rr.knn_graph(N, 8, 77)
    goals = np.array([0, 4095, 17, 2000, 2001], np.int32)
    cost = check_route(N, off, tg, w, 1000, [0, 1, 2, 5], goals)
    assert (cost < FAR).mean() > 0.5


def descend_call(N, off, tg, w, max_weight, cost, query, starts, max_nodes):
    o, t, ww = _dev(off, np.int32), _dev(tg, np.int32), _dev(w, np.int32)
    c, q, s = _dev(cost, np.int32), _dev(query, np.int32), _dev(starts, np.int32)
    P = len(query)
    path = torch.full((P, max_nodes), -77, dtype=torch.int32, device=DEV)
    length = torch.full((P,), -77, dtype=torch.int32, device=DEV)
    st = _lib().gg_roadmap_descend(N, len(tg), _p(o), _p(t), _p(ww), max_weight, cost.shape[0], _p(c), P, _p(q), _p(s),
                                   max_nodes, _p(path), _p(length), _stream())
    assert st == 0, _lib().gg_last_error()
    torch.cuda.synchronize()
    return path.cpu().numpy(), length.cpu().numpy()


def check_descend(N, off, tg, w, max_weight, cost, query, starts, max_nodes):
    got = descend_call(N, off, tg, w, max_weight, cost, query, starts, max_nodes)
    want = rr.descend(N, off, tg, w, max_weight, cost, query, starts, max_nodes)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return got


@gpu
def test_descend_takes_the_lowest_row_position_and_cuts_and_repeats():
    # a diamond with equal-cost branches: 0 -> {3, 1, 2} -> 4; row 0 lists 3 first
    rows = [[(3, 2), (1, 2), (2, 2), (4, 9)], [(4, 2)], [(4, 2)], [(4, 2)], [], [(0, 1)], []]
    N = len(rows)
    off, tg, w = rr.csr_from_lists(rows)
    cost, _ = rr.route(N, off, tg, w, 10, [0, 1, 2], [4, 6])
    assert cost[0].tolist() == [4, 2, 2, 2, 0, 5, FAR] and cost[1].tolist() == [FAR] * 6 + [0]
    for max_nodes in (1, 2, 3, 4, 7):                              # below, at and above the lengths
        for P in (1, 65):
            query = np.zeros(P, np.int32)
            starts = (np.arange(P) % 6).astype(np.int32)
            path, n = check_descend(N, off, tg, w, 10, cost, query, starts, max_nodes)
            assert n[0] == 3 and path[0, :3].tolist() == [0, 3, 4][:max_nodes] + [4] * max(0, min(3, max_nodes) - 3)
            if P > 5:
                assert n[4] == 1 and (path[4] == 4).all()           # length 1 on a goal
                assert n[5] == 4 and path[5, :min(max_nodes, 4)].tolist() == [5, 0, 3, 4][:max_nodes]
            if max_nodes == 7:
                assert path[0].tolist() == [0, 3, 4, 4, 4, 4, 4]
    # length 0: a start at FAR, a start out of range, a query out of range, a tampered cost
    query = np.array([0, 0, 0, 2, -1, 1, 1, 0], np.int32)
    starts = np.array([6, -1, N, 0, 0, 0, 6, 5], np.int32)
    path, n = check_descend(N, off, tg, w, 10, cost, query, starts, 5)
    assert n.tolist() == [0, 0, 0, 0, 0, 0, 1, 4] and (path[:6] == -1).all()
    bad = cost.copy()
    bad[0, 3] = 1                                                   # no edge of 0 fits any more except through 1
    path, n = check_descend(N, off, tg, w, 10, bad, [0, 0], [0, 5], 5)
    assert n[0] == 3 and path[0, :3].tolist() == [0, 1, 4]
    bad[0, 1] = bad[0, 2] = 1
    path, n = check_descend(N, off, tg, w, 10, bad, [0, 0], [0, 5], 5)
    assert n.tolist() == [0, 0] and (path == -1).all()
    bad = cost.copy()
    bad[0, 0] = -3                                                  # a negative cost: no edge fits
    check_descend(N, off, tg, w, 10, bad, [0], [0], 5)
    # rows longer than a wave: the fitting edge at position 0, 63, 64, 299 of a row of 300
    for at in (0, 63, 64, 299):
        row = [(1, 5)] * 300
        row[at] = (2, 4)
        if at + 1 < 300:
            row[at + 1] = (3, 4)                                    # the same cost one position later: not taken
        g = rr.csr_from_lists([row, [(4, 9)], [(4, 1)], [(4, 1)], []])
        c, _ = rr.route(5, *g, 10, [0, 1], [4])
        path, n = check_descend(5, *g, 10, c, [0], [0], 4)
        assert c[0, 0] == 5 and path[0].tolist() == [0, 2, 4, 4]
    # on the routed random graph, from every node
    N = 4096
    off, tg, w = rr.knn_graph(N, 8, 77)
    c, _ = rr.route(N, off, tg, w, 1000, [0, 1], [17])
    starts = np.arange(0, N, 13, dtype=np.int32)
    check_descend(N, off, tg, w, 1000, c, np.zeros(len(starts), np.int32), starts, 40)


# ------------------------------------------------------------------------------------------------
# the memory contract
# ------------------------------------------------------------------------------------------------
@gpu
def test_memory_contract_of_the_three_entries():
    lib = _lib()
    rng = np.random.default_rng(3)
    N, M, J, k = 300, 70, 7, 16
    nodes, queries = rng.uniform(-3, 3, (N, J)), rng.uniform(-3, 3, (M, J))
    skip = rng.integers(-1, N, M).astype(np.int32)
    valid = (rng.uniform(size=N) < 0.8).astype(np.uint8)
    off, tg, w = rr.knn_graph(N, 5, 9)
    go, goals = np.array([0, 2, 3], np.int32), np.array([4, 250, 7], np.int32)
    Q, P, max_nodes = 2, 9, 6
    want_cost, _ = rr.route(N, off, tg, w, 1000, go, goals)
    query, starts = (np.arange(P) % 2).astype(np.int32), rng.integers(0, N, P).astype(np.int32)
    ws_bytes = lib.gg_roadmap_route_workspace(N, Q)
    ar = Arena(DEV, 5)
    ar.carve("nodes", nodes, 8, "in").carve("queries", queries, 8, "in").carve("skip", skip, 4, "in")
    ar.carve("valid", valid, 1, "in")
    ar.carve("idx", np.zeros((M, k), np.int32), 4, "out").carve("d2", np.zeros((M, k), np.float64), 8, "out")
    ar.carve("offsets", off, 4, "in").carve("targets", tg, 4, "in").carve("weights", w, 4, "in")
    ar.carve("goals", goals, 4, "in").carve("cost", np.zeros((Q, N), np.int32), 4, "out")
    ar.carve("ignored", np.zeros(1, np.int64), 8, "out").carve("ws", ws_bytes, 256, "ws")
    ar.carve("cost_in", want_cost, 4, "in").carve("query", query, 4, "in").carve("starts", starts, 4, "in")
    ar.carve("path", np.zeros((P, max_nodes), np.int32), 4, "out").carve("length", np.zeros(P, np.int32), 4, "out")
    for name in ("nodes", "queries", "d2"):
        assert ar.address(name) % 16 == 8                           # fp64 arrays at 8-byte, not 16-byte, offsets
    keep, mp = _host(rng.uniform(0.1, 1.5, J), np.float64)
    keep2, gp = _host(go, np.int32)
    rounds = C.c_int(-1)

    def neigh(**o):
        a = dict(J=J, N=N, nodes=ar.ptr("nodes"), M=M, queries=ar.ptr("queries"), metric=mp, skip=ar.ptr("skip"),
                 valid=ar.ptr("valid"), k=k, idx=ar.ptr("idx"), d2=ar.ptr("d2"))
        a.update(o)
        return lib.gg_roadmap_neighbours(a["J"], a["N"], a["nodes"], a["M"], a["queries"], a["metric"], a["skip"],
                                         a["valid"], a["k"], a["idx"], a["d2"], _stream())

    def route(**o):
        a = dict(N=N, E=len(tg), offsets=ar.ptr("offsets"), targets=ar.ptr("targets"), weights=ar.ptr("weights"),
                 max_weight=1000, Q=Q, go=gp, goals=ar.ptr("goals"), cost=ar.ptr("cost"), ignored=ar.ptr("ignored"),
                 max_rounds=N + 1, rounds=C.byref(rounds), ws=ar.ptr("ws"), ws_bytes=ws_bytes)
        a.update(o)
        return lib.gg_roadmap_route(a["N"], a["E"], a["offsets"], a["targets"], a["weights"], a["max_weight"], a["Q"],
                                    a["go"], a["goals"], a["cost"], a["ignored"], a["max_rounds"], a["rounds"], a["ws"],
                                    a["ws_bytes"], _stream())

    def desc(**o):
        a = dict(N=N, E=len(tg), offsets=ar.ptr("offsets"), targets=ar.ptr("targets"), weights=ar.ptr("weights"),
                 max_weight=1000, Q=Q, cost=ar.ptr("cost_in"), P=P, query=ar.ptr("query"), starts=ar.ptr("starts"),
                 max_nodes=max_nodes, path=ar.ptr("path"), length=ar.ptr("length"))
        a.update(o)
        return lib.gg_roadmap_descend(a["N"], a["E"], a["offsets"], a["targets"], a["weights"], a["max_weight"], a["Q"],
                                      a["cost"], a["P"], a["query"], a["starts"], a["max_nodes"], a["path"], a["length"],
                                      _stream())

    def refused(status, *words):
        assert status == -1
        msg = lib.gg_last_error()
        for word in words:
            assert word in msg, (word, msg)

    def off_by(name, n):
        return C.c_void_p(ar.address(name) + n)
    # every refusal names its argument and comes before any launch
    refused(neigh(k=0), b"k must be")
    refused(neigh(k=33), b"k must be")
    refused(neigh(J=0), b"num_joints")
    refused(neigh(J=9), b"num_joints")
    refused(neigh(N=65537), b"num_nodes")
    refused(neigh(metric=None), b"null pointer", b"metric")
    refused(neigh(nodes=None), b"null pointer", b"nodes")
    refused(neigh(queries=None), b"null pointer", b"queries")
    refused(neigh(idx=None), b"null pointer", b"idx")
    refused(neigh(d2=None), b"null pointer", b"d2")
    refused(neigh(nodes=off_by("nodes", 4)), b"misaligned", b"nodes")
    refused(neigh(d2=off_by("d2", 4)), b"misaligned", b"d2")
    refused(neigh(idx=off_by("idx", 2)), b"misaligned", b"idx")
    refused(neigh(skip=off_by("skip", 2)), b"misaligned", b"skip")
    for bad in (-1.0, np.nan, np.inf):
        m = np.full(J, 1.0)
        m[3] = bad
        keep3, bp = _host(m, np.float64)
        refused(neigh(metric=bp), b"metric")
    refused(route(max_weight=(1 << 30) // N + 1), b"max_weight")    # N max_weight >= 2^30
    refused(route(max_weight=0), b"max_weight")
    refused(route(max_rounds=0), b"max_rounds")
    refused(route(rounds=None), b"null pointer", b"rounds_out")
    refused(route(go=None), b"null pointer", b"goal_offsets")
    refused(route(cost=None), b"null pointer", b"cost")
    refused(route(ignored=None), b"null pointer", b"ignored")
    refused(route(offsets=None), b"null pointer", b"offsets")
    refused(route(targets=None), b"null pointer", b"targets")
    refused(route(goals=None), b"null pointer", b"goals")
    refused(route(cost=off_by("cost", 2)), b"misaligned", b"cost")
    refused(route(ignored=off_by("ignored", 4)), b"misaligned", b"ignored")
    refused(route(E=(1 << 27) + 1), b"num_edges")
    keep4, badgo = _host([0, 2, 1], np.int32)
    refused(route(go=badgo), b"goal_offsets")
    assert route(ws_bytes=ws_bytes - 1) == -3 and route(ws=off_by("ws", 64)) == -1
    refused(desc(max_nodes=0), b"max_nodes")
    refused(desc(P=1 << 26, max_nodes=2), b"max_nodes")
    refused(desc(max_weight=(1 << 30) // N + 1), b"max_weight")
    refused(desc(path=None), b"null pointer", b"path")
    refused(desc(cost=None), b"null pointer", b"cost")
    refused(desc(length=off_by("length", 2)), b"misaligned", b"length")
    # the empty calls
    assert neigh(M=0) == 0 and desc(P=0) == 0
    torch.cuda.synchronize()
    assert ar.untouched()
    # the calls as they are meant: guards and inputs untouched, the outputs exactly as long as the result
    assert neigh() == 0 and route() == 0 and desc() == 0
    torch.cuda.synchronize()
    out = ar.check()
    metric = keep
    same_neighbours((out["idx"], out["d2"]), rr.neighbours(nodes, queries, metric, k, skip, valid))
    assert np.array_equal(out["cost"], want_cost) and out["ignored"][0] == 0 and 1 <= rounds.value <= N + 1
    want = rr.descend(N, off, tg, w, 1000, want_cost, query, starts, max_nodes)
    assert np.array_equal(out["path"], want[0]) and np.array_equal(out["length"], want[1])
    # N == 0 writes the empty rows and reads no node
    ar.rebase()
    assert neigh(N=0, nodes=None, valid=None) == 0
    torch.cuda.synchronize()
    out = ar.check()
    assert (out["idx"] == -1).all() and np.isinf(out["d2"]).all()


# ------------------------------------------------------------------------------------------------
# the task layer, on the block scene of tests/roadmap_ref.py
# ------------------------------------------------------------------------------------------------
def _scene():
    from gaussiangrasper_amd import field
    f = field.DistanceField(*rr.BOX, voxel=rr.H, device=torch.device(DEV))
    (x0, x1), (y0, y1), (z0, z1) = rr.BLOCK
    f.mass[x0:x1, y0:y1, z0:z1] = field.VOTE_ONE
    f.update()
    return f


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV)


@gpu
def test_build_equals_the_restated_roadmap_of_the_host_fixture():
    from gaussiangrasper_amd import arm as A, roadmap as R
    fx = rr.plan_fixture()
    f = _scene()
    assert np.array_equal(f.dist2.cpu().numpy(), rr.block_field()[2])
    N = len(fx["nodes"])
    rm = R.build(fx["model"], f, num_nodes=fx["num_nodes"], k=fx["k"], seed=fx["seed"],
                 terminals=np.stack([rr.Q_LEFT, rr.Q_RIGHT]), force=([N - 2], [N - 1]))
    assert rm.nodes.tobytes() == fx["nodes"].tobytes() and np.array_equal(rm.valid, fx["valid"])
    assert np.array_equal(rm.metric, fx["metric"])
    assert np.array_equal(rm.edge_a, fx["a"]) and np.array_equal(rm.edge_b, fx["b"])
    assert rm.edge_d2.tobytes() == fx["d2"].tobytes() and np.array_equal(rm.edge_w, fx["w"])
    assert np.array_equal(rm.motion.ok.cpu().numpy(), fx["ok"])
    assert np.array_equal(rm.motion.samples.cpu().numpy(), fx["edges"]["samples"])
    assert np.array_equal(rm.motion.slack.cpu().numpy(), fx["edges"]["slack"])
    for name in ("offsets", "targets", "weights"):
        assert np.array_equal(getattr(rm, name), fx[name]) and getattr(rm, name).dtype == np.int32
    assert rm.dropped == 0 and rm.params["res"] == rr.H and rm.k == fx["k"]


@gpu
def test_build_route_and_add_on_a_few_hundred_nodes():
    from gaussiangrasper_amd import arm as A, roadmap as R
    model = A.default_arm()
    f = _scene()
    rm = R.build(model, f, num_nodes=300, k=8, seed=2)
    N = rm.num_nodes
    assert N == 300 and 0 < rm.valid.sum() < N
    # valid: arm.motion's own verdict of the zero-length move
    own = A.motion(model, _t(rm.nodes), _t(rm.nodes), f)
    assert np.array_equal(rm.valid, own.ok.cpu().numpy().astype(np.uint8))
    # the candidates: the restatement's neighbours; the verdicts: arm.motion's own
    idx, _ = rr.neighbours(rm.nodes, rm.nodes, rm.metric, 8, skip=np.arange(N), valid=rm.valid)
    idx[rm.valid == 0] = -1
    a, b = R.candidate_pairs(np.arange(N), idx, N)
    assert np.array_equal(rm.edge_a, a) and np.array_equal(rm.edge_b, b)
    m = A.motion(model, _t(rm.nodes[a]), _t(rm.nodes[b]), f)
    ok = m.ok.cpu().numpy()
    assert np.array_equal(rm.motion.ok.cpu().numpy(), ok) and 0 < ok.sum() < len(ok)
    d2 = R.metric_d2(rm.nodes[a], rm.nodes[b], rm.metric)
    w = R.edge_weights(d2, rm.unit)
    want = R.assemble(N, a, b, ok & (w <= rm.max_weight), w)
    for got, exp in zip((rm.offsets, rm.targets, rm.weights), want):
        assert np.array_equal(got, exp)
    # the sample count of every edge is bounded through the metric
    assert (rm.motion.samples.cpu().numpy() <= np.ceil(np.sqrt(7) * np.sqrt(d2) / rr.H * (1 + 1e-12))).all()
    # route equals Dijkstra on that CSR
    goals = [[0], [5, 17, 250], [N - 1]]
    cost = R.route(rm, goals).cpu().numpy()
    want_cost, _ = rr.route(N, rm.offsets, rm.targets, rm.weights, rm.max_weight, [0, 1, 4, 5], [0, 5, 17, 250, N - 1])
    assert np.array_equal(cost, want_cost) and (cost < FAR).any()
    path, n = R.descend(rm, R.route(rm, goals), [0, 1, 2], [7, 9, 11])
    wp, wn = rr.descend(N, rm.offsets, rm.targets, rm.weights, rm.max_weight, want_cost, [0, 1, 2], [7, 9, 11],
                        path.shape[1])
    assert np.array_equal(path.cpu().numpy(), wp) and np.array_equal(n.cpu().numpy(), wn)
    # add: the old rows' edges among old nodes stay as they are
    before = rm.copy()
    new = rm.add(np.stack([rr.Q_LEFT, rr.Q_RIGHT, rm.nodes[3]]))
    assert new.tolist() == [N, N + 1, N + 2] and rm.num_nodes == N + 3 and before.num_nodes == N
    assert rm.nodes[:N].tobytes() == before.nodes.tobytes() and np.array_equal(rm.valid[:N], before.valid)
    T = len(before.edge_a)
    assert np.array_equal(rm.edge_a[:T], before.edge_a) and np.array_equal(rm.edge_b[:T], before.edge_b)
    assert (rm.edge_b[T:] >= N).all() and len(rm.edge_a) > T
    for i in range(N):
        row = rm.targets[rm.offsets[i]:rm.offsets[i + 1]]
        wrow = rm.weights[rm.offsets[i]:rm.offsets[i + 1]]
        old = before.targets[before.offsets[i]:before.offsets[i + 1]]
        assert np.array_equal(row[row < N], old)
        assert np.array_equal(wrow[row < N], before.weights[before.offsets[i]:before.offsets[i + 1]])
    assert rm.offsets[N + 1] > rm.offsets[N]                        # the new nodes found neighbours
    # a copy of a valid node is a neighbour of it at distance 0: weight 1
    if rm.valid[3]:
        row = rm.targets[rm.offsets[N + 2]:rm.offsets[N + 3]]
        assert 3 in row and rm.weights[rm.offsets[N + 2]:rm.offsets[N + 3]][row == 3][0] == 1


def _check_plan(model, f, plan, qa, qb, R, A):
    rm = plan.roadmap
    for a in range(len(qa)):
        for b in range(len(qb)):
            way = plan.routes[a][b]
            if way is None:
                assert plan.cost[a, b] == -1 and plan.hops[a, b] == -1 and np.isinf(plan.length[a, b])
                continue
            # the ends to the bit, every move ok when it is run on its own
            assert way[0].tobytes() == qa[a].tobytes() and way[-1].tobytes() == qb[b].tobytes()
            legs = A.motion(model, _t(way[:-1]), _t(way[1:]), f)
            assert legs.ok.all()
            ids = plan.nodes[a][b]
            assert ids[0] == plan.start + a and ids[-1] == plan.start + len(qa) + b
            # cost: the sum of the graph route's edge weights
            total = 0
            for u, v in zip(ids[:-1], ids[1:]):
                row = rm.targets[rm.offsets[u]:rm.offsets[u + 1]]
                total += int(rm.weights[rm.offsets[u]:rm.offsets[u + 1]][row == v][0])
            assert plan.cost[a, b] == total
            want = sum(float(np.sqrt(R.metric_d2(way[i], way[i + 1], rm.metric))) for i in range(len(way) - 1))
            assert abs(plan.length[a, b] - want) <= 1e-12 * want and plan.hops[a, b] == len(way) - 1


@gpu
def test_plan_goes_round_the_block_and_twice_the_same_bytes():
    from gaussiangrasper_amd import arm as A, roadmap as R
    model = A.default_arm()
    f = _scene()
    assert not bool(A.motion(model, _t([rr.Q_LEFT]), _t([rr.Q_RIGHT]), f).ok[0])        # the direct move is not ok
    near = rr.Q_LEFT.copy()
    near[0] = -0.5
    qa, qb = np.stack([rr.Q_LEFT, near]), np.stack([rr.Q_RIGHT, near])
    plan = R.plan(model, qa, qb, f, num_nodes=200, k=8)
    assert plan.routes[0][0] is not None and len(plan.routes[0][0]) >= 3 and plan.hops[0, 0] >= 2
    assert plan.routes[0][1].shape == (2, 7) and plan.hops[0, 1] == 1                   # the direct move is an edge
    assert plan.routes[1][1].shape == (2, 7) and plan.cost[1, 1] == 1                   # from a node to its copy
    _check_plan(model, f, plan, qa, qb, R, A)
    unpulled = plan.length.copy()
    assert np.array_equal(plan.nodes[0][0], np.asarray(plan.nodes[0][0]))
    # cost and length are consistent: each edge's weight is its length in units, rounded up
    way = plan.routes[0][0]
    assert plan.cost[0, 0] >= plan.length[0, 0] / R.UNIT and plan.cost[0, 0] <= plan.length[0, 0] / R.UNIT + len(way)
    # twice: the same bytes
    again = R.plan(model, qa, qb, f, num_nodes=200, k=8)
    for a in range(2):
        for b in range(2):
            assert again.routes[a][b].tobytes() == plan.routes[a][b].tobytes()
    assert again.cost.tobytes() == plan.cost.tobytes() and again.length.tobytes() == plan.length.tobytes()
    assert again.roadmap.targets.tobytes() == plan.roadmap.targets.tobytes()
    # through a roadmap built before, saved and loaded: the same routes as through the fresh one with these terminals
    base = R.build(model, f, num_nodes=200, k=8)
    kept = base.copy()
    through = R.plan(model, qa, qb, f, roadmap=base)
    assert base.num_nodes == 200 and base.targets.tobytes() == kept.targets.tobytes()   # planned on a copy
    _check_plan(model, f, through, qa, qb, R, A)
    assert through.routes[0][0] is not None and through.start == 200
    # shortcut: only moves that are ok, the ends kept, never longer (the triangle inequality of the metric)
    pulled = R.plan(model, qa, qb, f, num_nodes=200, k=8, shortcut_window=4)
    _check_plan(model, f, pulled, qa, qb, R, A)
    assert (pulled.length <= unpulled * (1 + 1e-12)).all() and np.array_equal(pulled.cost, plan.cost)
    assert (pulled.hops <= plan.hops).all()
    ways = R.shortcut(plan.roadmap, [plan.routes[0][0]], 4)
    assert ways[0].tobytes() == pulled.routes[0][0].tobytes()
    # the selection is shortcut_select of arm.motion's verdicts on shortcut_pairs
    way = plan.routes[0][0]
    p, i, j = R.shortcut_pairs([len(way)], 4)
    ok = A.motion(model, _t(way[i]), _t(way[j]), f).ok.cpu().numpy()
    assert np.array_equal(ways[0], way[R.shortcut_select([len(way)], 4, ok)[0]])
    with pytest.raises(ValueError, match="own parameters"):
        R.plan(model, qa, qb, f, roadmap=base, k=4)


@gpu
def test_plan_finds_a_route_wherever_connect_does_through_the_same_vias():
    from gaussiangrasper_amd import arm as A, roadmap as R
    model = A.default_arm()
    f = _scene()
    near = rr.Q_LEFT.copy()
    near[0] = -0.5
    qa, qb = np.stack([rr.Q_LEFT, near, model.home()]), np.stack([rr.Q_RIGHT, near])
    con = A.connect(model, qa, qb, f, num_vias=28)
    assert len(con.vias) + 5 <= 33 and (con.via == -1).any()        # k = 32 covers every other node
    print(f"connect through {len(con.vias)} vias: via = {con.via.tolist()}")
    plan = R.plan(model, qa, qb, f, nodes=con.vias, k=32)
    for a in range(3):
        for b in range(2):
            if con.via[a, b] != -2:
                assert plan.routes[a][b] is not None, (a, b)
                # and no longer in the metric than connect's, since connect's moves are edges of this graph
                assert plan.cost[a, b] <= sum(R.edge_weights(R.metric_d2(u, v, plan.roadmap.metric))
                                              for u, v in zip(con.routes[a][b][:-1], con.routes[a][b][1:]))
    _check_plan(model, f, plan, qa, qb, R, A)


@gpu
def test_command_lines(tmp_path, capsys):
    from gaussiangrasper_amd import arm as A, roadmap as R
    f = _scene()
    f.save(str(tmp_path / "field.npz"))
    np.save(tmp_path / "from.npy", rr.Q_LEFT)
    np.save(tmp_path / "to.npy", np.stack([rr.Q_RIGHT]))
    out, way = str(tmp_path / "roadmap.npz"), str(tmp_path / "way.npz")
    assert R.main(["build", "--arm", "default", "--field", str(tmp_path / "field.npz"), "--nodes", "150", "--k", "8",
                   "--out", out]) == 0
    assert "nodes clear" in capsys.readouterr().out
    rm = R.Roadmap.load(out)
    fresh = R.build(A.default_arm(), f, num_nodes=150, k=8)
    assert rm.targets.tobytes() == fresh.targets.tobytes() and rm.weights.tobytes() == fresh.weights.tobytes()
    for extra in (["--roadmap", out], ["--nodes", "150", "--k", "8"]):
        assert R.main(["plan", "--arm", "default", "--field", str(tmp_path / "field.npz"), "--from",
                       str(tmp_path / "from.npy"), "--to", str(tmp_path / "to.npy"), "--out", way] + extra) == 0
        assert "1 of 1 routes found" in capsys.readouterr().out
        with np.load(way) as z:
            assert set(z.files) == {"cost", "length", "hops", "waypoints"} and z["hops"][0, 0] >= 2
            n = int(z["hops"][0, 0]) + 1
            assert np.array_equal(z["waypoints"][0, 0, 0], rr.Q_LEFT) and np.array_equal(z["waypoints"][0, 0, n - 1], rr.Q_RIGHT)
            assert np.isnan(z["waypoints"][0, 0, n:]).all()
    # arm's command line: without --connect-roadmap the report has exactly the keys it has today; with it, the
    # roadmap's in place of the one-via search's
    poses = A.fk(A.default_arm(), _t([rr.Q_RIGHT]))[:, -1].float().cpu().numpy()[:, None, :]
    np.save(tmp_path / "poses.npy", poses)
    q, rep = str(tmp_path / "q.npy"), str(tmp_path / "r.npz")
    base = ["--arm", "default", "--poses", str(tmp_path / "poses.npy"), "--field", str(tmp_path / "field.npz"),
            "--connect-from", str(tmp_path / "from.npy"), "--out", q, "--report", rep]
    plain = {"reachable", "clear", "seed", "slack", "worst", "jump", "first_fail", "iters"}
    assert A.main(base) == 0
    capsys.readouterr()
    with np.load(rep) as z:
        assert set(z.files) == plain | {"connect_via", "connect_cost", "connect_waypoints"}
    assert A.main(base + ["--connect-roadmap", "150"]) == 0
    assert "through the roadmap" in capsys.readouterr().out
    reached = np.load(q)
    with np.load(rep) as z:
        assert set(z.files) == plain | {"roadmap_cost", "roadmap_hops", "roadmap_waypoints"}
        assert z["roadmap_cost"].shape == (1, 1) and z["roadmap_waypoints"].shape[:2] == (1, 1)
        if np.isfinite(reached[0, 0]).all() and z["roadmap_hops"][0, 0] >= 0:
            n = int(z["roadmap_hops"][0, 0]) + 1
            assert np.array_equal(z["roadmap_waypoints"][0, 0, 0], rr.Q_LEFT)
            assert np.array_equal(z["roadmap_waypoints"][0, 0, n - 1], reached[0, 0])
    assert A.main(base + ["--connect-roadmap", out]) == 0
    capsys.readouterr()
    with np.load(rep) as z:
        assert set(z.files) == plain | {"roadmap_cost", "roadmap_hops", "roadmap_waypoints"}
