"""No-GPU checks of object instances: the restatement (tests/cluster_ref.py) against sklearn.cluster.DBSCAN with no
point excluded; gg_cluster_dbscan / gg_cluster_stats refusing bad arguments on the host before any launch; the
Python layer's instance ordering, dropping and selection on CPU tensors; and every new command-line cross-check."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import cluster_ref as R


# ------------------------------------------------------------------------------------------------
# the restatement against sklearn
# ------------------------------------------------------------------------------------------------
def _against_sklearn(p, eps, mp, ref=None):
    from sklearn.cluster import DBSCAN
    ref = ref or R.restate(p, eps, mp)
    sk = DBSCAN(eps=eps, min_samples=mp).fit(p.astype(np.float64))
    core = np.zeros(len(p), bool)
    core[sk.core_sample_indices_] = True
    assert np.array_equal(ref["core"], core)
    assert np.array_equal(ref["labels"], sk.labels_)
    assert ref["num_clusters"] == sk.labels_.max() + 1
    return ref


@pytest.mark.parametrize("seed,n,eps,mp", [(1, 6000, 0.02, 6), (2, 20_000, 0.012, 5), (3, 20_000, 0.03, 40),
                                           (4, 41_000, 0.01, 4)])
def test_restatement_equals_sklearn_on_blobs_plus_noise(seed, n, eps, mp):
    p, ref = R.blobs_without_ties(seed, n, eps, mp)
    assert ref["near"] == 0                                  # so no point needs excluding
    _against_sklearn(p, eps, mp, ref)
    border = (ref["labels"] >= 0) & ~ref["core"]
    assert ref["num_clusters"] > 1 and border.sum() > 0 and (ref["labels"] < 0).sum() > 0
    print(f"seed {seed}: {ref['num_clusters']} clusters, {border.sum()} border points, {ref['core'].sum()} core")


@pytest.mark.parametrize("mp", [1, 3, 5, 7])
def test_restatement_equals_sklearn_on_the_tie_lattice(mp):
    p = R.lattice()
    ref = _against_sklearn(p, 0.25, mp)
    assert ref["near"] > 1000                                # axis neighbours sit exactly on the boundary
    assert ref["neighbor_count"].max() == 7 and ref["num_clusters"] >= 1


def test_restatement_equals_sklearn_with_duplicates():
    p = R.with_duplicates(5, 6000)
    ref = _against_sklearn(p, 0.015, 6)
    assert ref["num_clusters"] > 1 and ((ref["labels"] >= 0) & ~ref["core"]).sum() > 0
    assert len(np.unique(p, axis=0)) < len(p)


def test_restatement_numbering_border_and_inactive_rows():
    # two groups of core points, one with a border point; noise points, a NaN row, a masked row
    p = np.float32([[10, 0, 0], [0, 0, 0], [0.5, 0, 0], [5, 0, 0], [4.5, 0, 0], [np.nan, 0, 0], [0.25, 0, 0],
                    [4.0, 0.5, 0], [0, 0.5, 0], [5, 0.5, 0], [2.25, 0, 0]])
    act = np.ones(len(p), np.uint8)
    act[6] = 0
    ref = R.restate(p, 0.75, 3, act)
    #   cluster 0: smallest core index 1 -> {1, 2, 8}; cluster 1: core {3, 4, 9} and the border point 7 (it sees 4 only)
    assert ref["labels"].tolist() == [-1, 0, 0, 1, 1, -1, -1, 1, 0, 1, -1]
    assert ref["neighbor_count"].tolist() == [1, 3, 3, 3, 4, 0, 0, 2, 3, 3, 1]
    assert ref["core"].tolist() == [False, True, True, True, True, False, False, False, True, True, False]
    assert ref["num_clusters"] == 2
    # a border point between two clusters takes the smaller number
    q = np.float32([[3, 0, 0], [3.5, 0, 0], [3.25, 0.25, 0], [3.25, -0.25, 0],
                    [0, 0, 0], [0.5, 0, 0], [0.25, 0.25, 0], [0.25, -0.25, 0], [1.75, 0, 0]])
    ref = R.restate(q, 1.3, 4)
    assert ref["core"].tolist() == [True] * 8 + [False]
    assert ref["labels"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 0] and ref["neighbor_count"][8] == 3


# ------------------------------------------------------------------------------------------------
# the C ABI without a GPU
# ------------------------------------------------------------------------------------------------
def _buffers(n=8):
    """host arrays standing in for device pointers: validation never dereferences them"""
    b = dict(points=np.zeros((n, 3), np.float32), labels=np.zeros(n, np.int32), core=np.zeros(n, np.uint8),
             count=np.zeros(n, np.int32), num=np.zeros(1, np.int32), ws=np.zeros(1 << 16, np.uint8))
    base = b["ws"].ctypes.data
    b["ws_ptr"] = ctypes.c_void_p((base + 255) // 256 * 256)
    return b


def _call(lib, b, n=8, eps=0.5, mp=3, grid=(0.0, 0.0, 0.0, 1.0), dims=(2, 2, 2), ws_bytes=None, null=()):
    grid_c = (ctypes.c_double * 4)(*grid)
    dims_c = (ctypes.c_int32 * 3)(*dims)
    P = lambda k: ctypes.c_void_p(0) if k in null else ctypes.c_void_p(b[k].ctypes.data)  # noqa: E731
    need = lib.gg_cluster_workspace(n, dims_c)
    return lib.gg_cluster_dbscan(n, P("points"), None, eps, mp, ctypes.cast(grid_c, ctypes.c_void_p),
                                 ctypes.cast(dims_c, ctypes.c_void_p), P("labels"), P("core"), P("count"), P("num"),
                                 ctypes.c_void_p(0) if "ws" in null else b["ws_ptr"],
                                 need if ws_bytes is None else ws_bytes, None)


def test_dbscan_arguments_are_checked_on_the_host():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    b = _buffers()
    cases = [(dict(eps=0.0), b"eps"), (dict(eps=-1.0), b"eps"), (dict(eps=float("nan")), b"eps"),
             (dict(eps=float("inf")), b"eps"), (dict(mp=0), b"min_points"), (dict(mp=-3), b"min_points"),
             (dict(null=("labels",)), b"null"), (dict(null=("core",)), b"null"), (dict(null=("count",)), b"null"),
             (dict(null=("num",)), b"null"), (dict(null=("points",)), b"null"), (dict(null=("ws",)), b"ws"),
             (dict(ws_bytes=256), b"workspace too small"), (dict(ws_bytes=0), b"workspace too small"),
             (dict(n=-1), b"num_points"), (dict(grid=(0.0, 0.0, 0.0, 0.0)), b"grid"),
             (dict(grid=(float("nan"), 0.0, 0.0, 1.0)), b"grid"), (dict(dims=(0, 1, 1)), b"dims"),
             (dict(dims=(1 << 14, 1 << 14, 1)), b"dims")]
    for kw, word in cases:
        assert _call(lib, b, **kw) == -1, kw
        msg = lib.gg_last_error()
        assert msg.startswith(b"gg_cluster_dbscan:") and word in msg, (kw, msg)
    with pytest.raises(_lib.GGError, match="gg_cluster_dbscan"):
        _lib.check(_call(lib, b, eps=0.0), "gg_cluster_dbscan")
    # N == 0: nothing to do, nothing launched, no pointer looked at
    assert _call(lib, b, n=0, null=("points", "labels", "core", "count", "num", "ws"), ws_bytes=0) == 0


def test_stats_arguments_are_checked_on_the_host():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    n0 = ctypes.c_void_p(0)
    a = np.zeros(64, np.float64)
    p = ctypes.c_void_p(a.ctypes.data)
    assert lib.gg_cluster_stats(-1, p, p, p, 1, p, p, p, p, None) == -1 and b"num_points" in lib.gg_last_error()
    assert lib.gg_cluster_stats(4, p, p, p, -1, p, p, p, p, None) == -1 and b"num_clusters" in lib.gg_last_error()
    assert lib.gg_cluster_stats(4, p, p, p, 5, p, p, p, p, None) == -1 and b"num_clusters" in lib.gg_last_error()
    for k in range(7):
        args = [p] * 7
        args[k] = n0
        assert lib.gg_cluster_stats(4, *args[:3], 2, *args[3:], None) == -1
        assert lib.gg_last_error().startswith(b"gg_cluster_stats:") and b"null" in lib.gg_last_error()
    assert lib.gg_cluster_stats(4, n0, n0, n0, 0, n0, n0, n0, n0, None) == 0     # no clusters: nothing to do


def test_workspace_query_is_a_pure_host_call():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    dims = lambda *d: (ctypes.c_int32 * 3)(*d)  # noqa: E731
    small, big = lib.gg_cluster_workspace(1000, dims(8, 8, 8)), lib.gg_cluster_workspace(1_000_000, dims(64, 64, 64))
    assert 0 < small < big < 64 * 2 ** 20 and small % 256 == 0 and big % 256 == 0
    assert big >= 1_000_000 * (16 + 4 + 4 + 4 + 1)          # sorted rows, parent, flags, rank, core flags
    assert lib.gg_cluster_workspace(0, dims(1, 1, 1)) > 0
    assert lib.gg_cluster_workspace(-1, dims(1, 1, 1)) == 0
    assert lib.gg_cluster_workspace((1 << 30) + 1, dims(1, 1, 1)) == 0
    assert lib.gg_cluster_workspace(10, dims(0, 1, 1)) == 0 and lib.gg_cluster_workspace(10, dims(1 << 14, 1 << 14, 1)) == 0
    assert lib.gg_cluster_workspace(10, None) == 0
    assert lib.gg_prof_name(46) == b"gg_cluster_dbscan(all launches)"
    assert lib.gg_prof_name(47) == b"gg_cluster_stats(all launches)"


def test_no_cpu_fallback():
    from gaussiangrasper_amd import cluster
    with pytest.raises(RuntimeError, match="HIP device"):
        cluster.dbscan(torch.zeros(10, 3), 0.1)
    with pytest.raises(RuntimeError, match="HIP device"):
        cluster.cluster_stats(torch.zeros(10, 3), torch.zeros(10), (torch.zeros(10, dtype=torch.int32), 1))
    with pytest.raises(ValueError, match="eps"):
        cluster.dbscan(torch.zeros(10, 3), 0.0)
    with pytest.raises(ValueError, match="min_points"):
        cluster.dbscan(torch.zeros(10, 3), 0.1, min_points=0)


# ------------------------------------------------------------------------------------------------
# the Python layer on CPU tensors
# ------------------------------------------------------------------------------------------------
def _hand_made():
    from gaussiangrasper_amd.cluster import ClusterStats
    labels = torch.tensor([0, 0, 1, 1, 1, -1, 2, 3, 3, 3, 3, 4, 4, 4, -1, 0], dtype=torch.int32)
    stats = ClusterStats(count=torch.tensor([3, 3, 1, 4, 3]),
                         weight=torch.tensor([2.0, 2.5, 9.0, 2.5, 0.5], dtype=torch.float64),
                         centroid=torch.tensor([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [1, 0.1, 0]],
                                               dtype=torch.float64),
                         bbox=torch.zeros(5, 6))
    return labels, stats


def test_instances_are_ordered_by_weight_then_cluster_number():
    from gaussiangrasper_amd.cluster import instance_mask, rank_instances
    labels, stats = _hand_made()
    inst = rank_instances(labels, stats, min_count=2, min_weight=1.0)
    # cluster 2 has one member (dropped by min_count), cluster 4 weighs 0.5 (dropped by min_weight); 1 and 3 tie at
    # 2.5 and keep their cluster order; 0 is the lightest of the kept
    assert inst.cluster.tolist() == [1, 3, 0] and len(inst) == 3
    assert inst.ids.tolist() == [2, 2, 0, 0, 0, -1, -1, 1, 1, 1, 1, -1, -1, -1, -1, 2]
    assert inst.ids.dtype == torch.int32
    assert inst.stats.count.tolist() == [3, 4, 3] and inst.stats.weight.tolist() == [2.5, 2.5, 2.0]
    assert inst.stats.centroid[:, 0].tolist() == [1.0, 3.0, 0.0]
    assert inst.masks().shape == (3, 16) and torch.equal(inst.masks()[1], inst.ids == 1)
    # nothing dropped: the single heavy point leads
    every = rank_instances(labels, stats, min_count=0, min_weight=0.0)
    assert every.cluster.tolist() == [2, 1, 3, 0, 4]
    assert rank_instances(labels, stats, min_count=100).cluster.tolist() == []
    assert (rank_instances(labels, stats, min_count=100).ids == -1).all()
    # by rank, and by the nearest centroid (the smallest rank on a tie)
    assert torch.equal(instance_mask(inst, 0), labels == 1)
    assert torch.equal(instance_mask(inst, 2), labels == 0)
    assert torch.equal(instance_mask(inst, [2.9, 0.0, 0.0]), labels == 3)
    assert torch.equal(instance_mask(inst, np.array([0.4, 0.0, 0.0])), labels == 0)
    assert torch.equal(instance_mask(inst, (2.0, 0.0, 0.0)), labels == 1)       # 1 and 3 are both 1 away
    assert torch.equal(instance_mask(every, (1.0, 0.1, 0.0)), labels == 4)
    for bad in (3, -1, [0.0, 1.0], [0.0, float("nan"), 0.0]):
        with pytest.raises(ValueError):
            instance_mask(inst, bad)
    with pytest.raises(ValueError, match="no instances"):
        instance_mask(rank_instances(labels, stats, min_count=100), 0)
    with pytest.raises(ValueError, match="min_weight"):
        rank_instances(labels, stats, min_weight=float("nan"))
    with pytest.raises(ValueError, match="min_count"):
        rank_instances(labels, stats, min_count=-1)


# ------------------------------------------------------------------------------------------------
# command lines
# ------------------------------------------------------------------------------------------------
QUERY = ["--positives", "p.npy", "--negatives", "n.npy", "--threshold", "0.5"]


def _mains():
    from gaussiangrasper_amd import grasp, grasp_propose, mesh
    return [(grasp_propose.main, ["--ckpt", "x.ckpt", "--out", "o.npy"]),
            (grasp.main, ["--ckpt", "x.ckpt", "--grasps", "g.npy", "--out", "o.npy"]),
            (mesh.main, ["--ckpt", "x.ckpt", "--transforms", "t.json", "--out", "o.ply"])]


@pytest.mark.parametrize("extra,message", [
    (QUERY + ["--cluster-eps", "0.1"], "--cluster-eps needs --instance"),
    (QUERY + ["--cluster-eps-scale", "2"], "--cluster-eps-scale needs --instance"),
    (QUERY + ["--cluster-min-points", "4"], "--cluster-min-points needs --instance"),
    (QUERY + ["--instance", "all", "--cluster-eps", "0.1"], "--cluster-eps needs --instance"),
    (QUERY + ["--instance", "largest", "--cluster-eps", "0"], "--cluster-eps must be finite and > 0"),
    (QUERY + ["--instance", "largest", "--cluster-eps", "nan"], "--cluster-eps must be finite and > 0"),
    (QUERY + ["--instance", "1", "--cluster-eps-scale", "-2"], "--cluster-eps-scale must be finite and > 0"),
    (QUERY + ["--instance", "1", "--cluster-eps", "0.1", "--cluster-eps-scale", "2"], "are alternatives"),
    (QUERY + ["--instance", "largest", "--cluster-min-points", "0"], "--cluster-min-points must be >= 1"),
    (QUERY + ["--instance", "biggest"], "expected all, largest or a rank"),
    (QUERY + ["--instance", "-1"], "expected all, largest or a rank"),
])
def test_cli_cross_checks_of_the_instance_options(extra, message, capsys):
    for main, base in _mains():
        with pytest.raises(SystemExit) as exc:
            main(base + extra)
        assert exc.value.code == 2
        assert message in capsys.readouterr().err, main.__module__


def test_cli_instance_needs_a_selection(capsys):
    from gaussiangrasper_amd import grasp, mesh
    for main, base in ((grasp.main, ["--ckpt", "x.ckpt", "--grasps", "g.npy", "--out", "o.npy"]),
                       (mesh.main, ["--ckpt", "x.ckpt", "--transforms", "t.json", "--out", "o.ply"])):
        with pytest.raises(SystemExit) as exc:
            main(base + ["--instance", "largest"])
        assert exc.value.code == 2 and "--instance needs a selection" in capsys.readouterr().err


@pytest.mark.parametrize("extra,message", [
    (QUERY + ["--eps", "0"], "--eps must be finite and > 0"),
    (QUERY + ["--eps-scale", "inf"], "--eps-scale must be finite and > 0"),
    (QUERY + ["--min-points", "0"], "--min-points must be >= 1"),
    (QUERY + ["--min-count", "-1"], "--min-count"),
    ([], "one of --object-points and --positives is needed"),
    (["--positives", "p.npy"], "--positives needs --negatives and --threshold"),
    (QUERY + ["--instance", "largest"], "unrecognized arguments"),
])
def test_cluster_cli_cross_checks(extra, message, capsys):
    from gaussiangrasper_amd import cluster
    with pytest.raises(SystemExit) as exc:
        cluster.main(["--ckpt", "x.ckpt", "--out", "labels.npy"] + extra)
    assert exc.value.code == 2 and message in capsys.readouterr().err


def test_instance_choice_values():
    from gaussiangrasper_amd._cli import add_object_options, instance_choice
    assert instance_choice("all") == "all" and instance_choice("largest") == "largest" and instance_choice("3") == 3
    ap = argparse.ArgumentParser()
    add_object_options(ap, "q", "h")
    a = ap.parse_args([])
    assert a.instance == "all" and a.cluster_eps is None and a.cluster_eps_scale is None
    assert a.cluster_min_points is None
    assert ap.parse_args(["--instance", "2"]).instance == 2
    plain = argparse.ArgumentParser()
    add_object_options(plain, "q", "h", instances=False)
    assert not hasattr(plain.parse_args([]), "instance")


def test_object_mask_is_the_selection_unless_an_instance_is_asked_for(monkeypatch):
    """--instance all, or a parser without the option, hands on the very mask object the selection made; largest or
    K goes through cluster.object_instances on that mask"""
    from gaussiangrasper_amd import _cli, cluster
    labels, stats = _hand_made()
    selected = labels >= 0
    seen = {}

    def fake_selection(a, scene, mlp_state, matrix=None, scale=1.0):
        return selected

    def fake_instances(scene, mask, eps=None, **kw):
        seen.update(mask=mask, eps=eps, **kw)
        return cluster.rank_instances(labels, stats, min_count=2, min_weight=1.0)

    monkeypatch.setattr(_cli, "selection_mask", fake_selection)
    monkeypatch.setattr(cluster, "object_instances", fake_instances)
    old_style = argparse.Namespace(object_points=None, positives="p.npy", negatives="n.npy", threshold=0.5)
    assert _cli.object_mask(old_style, None, None) is selected and not seen
    ns = lambda **kw: argparse.Namespace(**{**vars(old_style), "instance": "all", "cluster_eps": None,  # noqa: E731
                                            "cluster_eps_scale": None, "cluster_min_points": None, **kw})
    assert _cli.object_mask(ns(), None, None) is selected and not seen
    got = _cli.object_mask(ns(instance="largest"), None, None)
    assert torch.equal(got, labels == 1) and seen == dict(mask=selected, eps=None)
    got = _cli.object_mask(ns(instance=2, cluster_eps=0.25, cluster_min_points=5), None, None, None, 2.0)
    assert torch.equal(got, labels == 0) and seen == dict(mask=selected, eps=0.5, min_points=5)
    _cli.object_mask(ns(instance=1, cluster_eps_scale=4.0), None, None)
    assert seen["eps"] is None and seen["eps_scale"] == 4.0
    with pytest.raises(ValueError, match="has 3 instances"):
        _cli.object_mask(ns(instance=3), None, None)
    # without a selection there is nothing to split
    monkeypatch.setattr(_cli, "selection_mask", lambda *a, **k: None)
    assert _cli.object_mask(ns(instance="largest"), None, None) is None


def test_without_a_selection_object_mask_is_none():
    from gaussiangrasper_amd import _cli
    a = argparse.Namespace(object_points=None, positives=None, negatives=None, threshold=None)
    assert _cli.object_mask(a, None, None) is None
