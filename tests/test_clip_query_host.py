"""No-GPU checks of the language query (gaussiangrasper_amd.query, gg_clip_query): the workspace query, the C entry's
argument validation, the closed-form relevancy against LERF's softmax-then-min form in fp64, the Python-side
validation (refused before any device work) and the command line's refusals."""
import ctypes
import os
import re
import threading

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_query_max_matches_the_header():
    from gaussiangrasper_amd import query
    src = open(os.path.join(ROOT, "include", "gg_raster.h")).read()
    assert int(re.search(r"#define\s+GG_QUERY_MAX\s+(\d+)", src).group(1)) == query.MAX_QUERIES
    assert query.MAX_QUERIES >= 4


def test_workspace_is_a_pure_host_call_and_zero_for_unsupported_shapes():
    from gaussiangrasper_amd import _lib, query
    lib = _lib.load()
    Q = query.MAX_QUERIES
    for d in (32, 64, 128):
        assert lib.gg_clip_query_workspace(d, 128, 512, 1) >= lib.gg_mlp_fwd_fast_workspace(d, 128, 512)
        assert lib.gg_clip_query_workspace(d, 128, 512, Q) > lib.gg_clip_query_workspace(d, 128, 512, 1)
    for args in ((16, 128, 512, 1), (48, 128, 512, 1), (32, 64, 512, 1), (32, 128, 520, 1), (32, 128, 0, 1),
                 (32, 128, 3984, 1), (32, 128, 512, 0), (32, 128, 512, Q + 1), (32, 128, 512, -1),
                 (32, 128, 3968, Q)):      # the last: the query rows no longer fit the LDS beside the slices
        assert lib.gg_clip_query_workspace(*args) == 0, args
    assert query._max_queries(512) == Q and query._max_queries(520) == 0 and query._max_queries(3968) < Q


def test_clip_query_argument_validation_without_a_gpu():
    """every invalid argument is refused on the host with a message before anything is launched (on a thread of its
    own: gg_last_error is per thread)"""
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    n = ctypes.c_void_p(0)
    f = ctypes.c_void_p(1 << 20)            # 16-byte aligned, never dereferenced: validation fails first
    odd = ctypes.c_void_p((1 << 20) + 4)
    ws_ok = lib.gg_clip_query_workspace(32, 128, 512, 4)

    def call(rows=100, d=32, hid=128, c=512, x=f, w1=f, b1=f, w2=f, b2=f, nq=4, npos=1, q=f, tau=10.0, sims=f,
             rel=f, ws=f, wsb=ws_ok):
        return lib.gg_clip_query(rows, d, hid, c, x, w1, b1, w2, b2, nq, npos, q, tau, sims, rel, ws, wsb, n)
    cases = [
        (dict(rows=-1), -1, b"num_rows"),
        (dict(d=16), -1, b"in_dim"),
        (dict(hid=64), -1, b"hidden_dim"),
        (dict(c=520), -1, b"out_dim"),
        (dict(c=4096), -1, b"out_dim"),
        (dict(nq=0), -1, b"num_queries"),
        (dict(nq=9), -1, b"num_queries"),
        (dict(c=3968, nq=8, npos=1), -1, b"LDS"),
        (dict(npos=5), -1, b"num_positives"),
        (dict(npos=4), -1, b"negative"),          # relevancy with no negatives
        (dict(npos=0), -1, b"negative"),          # relevancy with no positives
        (dict(sims=n, rel=n), -1, b"NULL"),
        (dict(tau=0.0), -1, b"temperature"),
        (dict(tau=-1.0), -1, b"temperature"),
        (dict(tau=float("inf")), -1, b"temperature"),
        (dict(tau=float("nan")), -1, b"temperature"),
        (dict(x=n), -1, b"null pointer"),
        (dict(w2=n), -1, b"null pointer"),
        (dict(q=n), -1, b"null pointer"),
        (dict(x=odd), -1, b"aligned"),
        (dict(sims=ctypes.c_void_p((1 << 20) + 2)), -1, b"aligned"),
        (dict(ws=n), -3, b"workspace"),
        (dict(wsb=ws_ok - 16), -3, b"workspace"),
        (dict(ws=odd), -3, b"workspace"),
    ]
    got = []

    def run():
        for kw, _, _ in cases:
            got.append((call(**kw), lib.gg_last_error()))
        got.append((call(rows=0, x=n, w1=n, b1=n, w2=n, b2=n, q=n, ws=n, wsb=0), lib.gg_last_error()))
    t = threading.Thread(target=run)
    t.start()
    t.join()
    assert len(got) == len(cases) + 1
    for (st, msg), (kw, want_st, want) in zip(got, cases):
        assert st == want_st and msg.startswith(b"gg_clip_query") and want in msg, (kw, st, msg)
    assert got[-1][0] == 0       # rows = 0: a no-op once the shapes are valid


def lerf_softmax_min(s, n_pos, tau):
    """LERF's form, fp64: for each positive p, min over the negatives j of softmax(tau [s_p, s_nj])[0]"""
    out = np.empty(s.shape[:-1] + (n_pos,))
    for p in range(n_pos):
        best = np.full(s.shape[:-1], np.inf)
        for j in range(n_pos, s.shape[-1]):
            z = tau * np.stack([s[..., p], s[..., j]], -1)
            z = z - z.max(-1, keepdims=True)
            e = np.exp(z)
            best = np.minimum(best, e[..., 0] / e.sum(-1))
        out[..., p] = best
    return out


def closed_form(s, n_pos, tau):
    m = s[..., n_pos:].max(-1, keepdims=True)
    return 1.0 / (1.0 + np.exp(tau * (m - s[..., :n_pos])))


@pytest.mark.parametrize("n_pos,n_neg", [(1, 1), (1, 3), (3, 5), (7, 1)])
def test_closed_form_relevancy_is_lerf_softmax_min(n_pos, n_neg):
    rng = np.random.default_rng(n_pos * 10 + n_neg)
    s = rng.uniform(-1, 1, size=(4000, n_pos + n_neg))
    s[:200, n_pos:] = s[:200, :1]                   # ties between a positive and every negative
    s[200:400, n_pos:] = s[200:400, n_pos:n_pos + 1]  # ties among the negatives
    for tau in (10.0, 1.0, 100.0):
        a, b = closed_form(s, n_pos, tau), lerf_softmax_min(s, n_pos, tau)
        assert np.abs(a - b).max() <= 1e-14
    assert np.all(closed_form(s[:200], n_pos, 10.0)[:, 0] == 0.5)


def _mlp(d=32, c=512):
    from gaussiangrasper_amd.stub import MLP
    return MLP(d, c, hidden_list=[128])


def test_python_validation_before_any_device_work():
    """all of these are refused on CPU tensors with ValueError, i.e. before the HIP-device check"""
    from gaussiangrasper_amd import query
    m = _mlp()
    x = torch.randn(10, 32)
    pos, neg = torch.randn(2, 512), torch.randn(3, 512)
    with pytest.raises(ValueError, match="features"):
        query.relevancy(torch.randn(10, 16), m, pos, neg)
    with pytest.raises(ValueError, match="positives"):
        query.relevancy(x, m, torch.randn(2, 500), neg)
    with pytest.raises(ValueError, match="negatives"):
        query.relevancy(x, m, pos, torch.randn(3, 511))
    with pytest.raises(ValueError, match="zero norm"):
        query.relevancy(x, m, torch.cat([pos, torch.zeros(1, 512)]), neg)
    with pytest.raises(ValueError, match="zero norm"):
        query.clip_similarity(x, m, torch.zeros(512))
    with pytest.raises(ValueError, match="non-finite"):
        query.clip_similarity(x, m, torch.full((1, 512), float("nan")))
    with pytest.raises(ValueError, match="at most"):
        query.relevancy(x, m, pos, torch.randn(query.MAX_QUERIES, 512))
    with pytest.raises(ValueError, match="at least one negative"):
        query.relevancy(x, m, pos, None)
    for tau in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            query.relevancy(x, m, pos, neg, temperature=tau)
    with pytest.raises(ValueError, match="w1"):
        query.relevancy(x, (torch.randn(64, 32), torch.randn(64), torch.randn(512, 64), torch.randn(512)), pos, neg)
    # a valid call on host tensors reaches the device check: there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        query.relevancy(x, m, pos, neg)


def test_cli_rejects_bad_arguments(tmp_path):
    from gaussiangrasper_amd import query
    np.save(tmp_path / "pos.npy", np.ones((1, 512), np.float32))
    np.save(tmp_path / "empty.npy", np.zeros((0, 512), np.float32))
    ck = tmp_path / "step-000000100.ckpt"
    torch.save({"step": 100, "pipeline": {"_model.quats": torch.zeros(3, 4)}}, ck)
    out = tmp_path / "scores.npy"
    base = ["--ckpt", str(ck), "--out", str(out)]
    with pytest.raises(SystemExit):                          # --positives is required
        query.main(base)
    with pytest.raises(SystemExit, match="temperature"):
        query.main(base + ["--positives", str(tmp_path / "pos.npy"), "--temperature", "0"])
    with pytest.raises(SystemExit, match="positives"):
        query.main(base + ["--positives", str(tmp_path / "empty.npy")])
    with pytest.raises(SystemExit, match="missing"):         # not a splatting checkpoint
        query.main(base + ["--positives", str(tmp_path / "pos.npy")])
    with pytest.raises(SystemExit, match="error"):
        query.main(base + ["--positives", str(tmp_path / "nope.npy")])
    assert not out.exists()
