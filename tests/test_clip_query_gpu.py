"""GPU checks of the language query (gaussiangrasper_amd.query on gg_clip_query): similarities and relevancy against an
fp64 numpy restatement (fp64 MLP -> normalise -> dot -> closed-form / softmax-min), against the unfused torch chain,
run-to-run identity, the edge cases of the contract, relevancy_view on the plugin's model, the memory the fused query
saves, semantic selection of Gaussians and the command-line tool on a synthetic checkpoint."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
DEV = "cuda:0"


def make_mlp(d, c, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    w1 = torch.randn(128, d, generator=g) / d ** 0.5 * scale
    b1 = torch.randn(128, generator=g) * 0.1 * scale
    w2 = torch.randn(c, 128, generator=g) / 128 ** 0.5 * scale
    b2 = torch.randn(c, generator=g) * 0.1 * scale
    return w1, b1, w2, b2


def ref_sims(x, w, q):
    """fp64: y = W2 relu(W1 x + b1) + b2, s = y / max(|y|, 1e-12) . q / |q|"""
    w1, b1, w2, b2 = (t.double().numpy() for t in w)
    xd = x.reshape(-1, x.shape[-1]).double().numpy()
    y = np.maximum(xd @ w1.T + b1, 0.0) @ w2.T + b2
    y = y / np.maximum(np.linalg.norm(y, axis=1, keepdims=True), 1e-12)
    qd = q.double().numpy()
    qd = qd / np.linalg.norm(qd, axis=1, keepdims=True)
    return y @ qd.T


def ref_rel(s, n_pos, tau=10.0):
    m = s[:, n_pos:].max(axis=1, keepdims=True)
    return 1.0 / (1.0 + np.exp(tau * (m - s[:, :n_pos])))


def to_dev(w):
    return tuple(t.to(DEV) for t in w)


@gpu
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("c", [96, 512])
def test_similarities_against_fp64(d, c):
    from gaussiangrasper_amd import query
    w = make_mlp(d, c, seed=d + c)
    wd = to_dev(w)
    g = torch.Generator().manual_seed(7)
    worst = 0.0
    for rows in (1, 15, 16, 17, 511, 512, 513, 300_000 if (d, c) == (32, 512) else 4097):
        x = torch.randn(rows, d, generator=g)
        for nq in sorted({1, 2, 4, query.MAX_QUERIES}):
            q = torch.randn(nq, c, generator=g)
            got = query.clip_similarity(x.to(DEV), wd, q).cpu().double().numpy()
            assert got.shape == (rows, nq)
            err = np.abs(got - ref_sims(x, w, q)).max()
            worst = max(worst, err)
            assert err <= 2e-5, (rows, nq, err)
    print(f"d={d} c={c}: max |ds| {worst:.2e}")


@gpu
def test_more_positives_than_a_launch_takes_are_chunked():
    from gaussiangrasper_amd import query
    w = make_mlp(32, 512, seed=3)
    x = torch.randn(3000, 32)
    q = torch.randn(2 * query.MAX_QUERIES + 3, 512)
    got = query.clip_similarity(x.to(DEV), to_dev(w), q).cpu().double().numpy()
    assert np.abs(got - ref_sims(x, w, q)).max() <= 2e-5
    pos, neg = torch.randn(11, 512), torch.randn(3, 512)
    r = query.relevancy(x.to(DEV), to_dev(w), pos, neg).cpu().double().numpy()
    assert r.shape == (3000, 11)
    assert np.abs(r - ref_rel(ref_sims(x, w, torch.cat([pos, neg])), 11)).max() <= 1e-4


@gpu
@pytest.mark.parametrize("n_pos,n_neg", [(1, 3), (2, 1), (1, 7), (5, 3)])
def test_relevancy_against_fp64_and_the_unfused_chain(n_pos, n_neg):
    from gaussiangrasper_amd import query
    from gaussiangrasper_amd.mlp import mlp_forward
    w = make_mlp(32, 512, seed=11)
    wd = to_dev(w)
    x = torch.randn(20_000, 32, generator=torch.Generator().manual_seed(12))
    pos, neg = torch.randn(n_pos, 512), torch.randn(n_neg, 512)
    for tau in (10.0, 3.0):
        r = query.relevancy(x.to(DEV), wd, pos, neg, temperature=tau)
        assert r.shape == (20_000, n_pos) and r.grad_fn is None
        ref = ref_rel(ref_sims(x, w, torch.cat([pos, neg])), n_pos, tau)
        assert np.abs(r.cpu().double().numpy() - ref).max() <= 1e-4
        # the chain it replaces: fea_up, F.normalize, @ q^T, softmax then min over the negatives
        qn = F.normalize(torch.cat([pos, neg]).to(DEV), dim=-1)
        s = F.normalize(mlp_forward(x.to(DEV), *wd), dim=-1) @ qn.T
        pair = torch.stack([s[:, :n_pos, None].expand(-1, -1, n_neg), s[:, None, n_pos:].expand(-1, n_pos, -1)], -1)
        chain = torch.softmax(tau * pair, dim=-1)[..., 0].min(dim=-1).values
        assert (r - chain).abs().max().item() <= 1e-4


@gpu
def test_two_calls_are_bit_identical():
    from gaussiangrasper_amd import query
    wd = to_dev(make_mlp(128, 512, seed=5))
    x = torch.randn(100_003, 128, device=DEV)
    pos, neg = torch.randn(2, 512), torch.randn(3, 512)
    a = query._query(x, wd, pos, neg, 10.0, True, True)
    b = query._query(x, wd, pos, neg, 10.0, True, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@gpu
def test_edge_cases():
    from gaussiangrasper_amd import query
    pos, neg = torch.randn(1, 512), torch.randn(3, 512)
    # zero weights: y = 0 -> s = 0 -> r = 1/2
    z = tuple(torch.zeros_like(t).to(DEV) for t in make_mlp(32, 512, 0))
    s, r = query._query(torch.randn(1000, 32, device=DEV), z, pos, neg, 10.0, True, True)
    assert torch.all(s == 0) and torch.all(r == 0.5)
    # one NaN row: only that row is NaN
    w = make_mlp(32, 512, seed=21)
    x = torch.randn(1000, 32)
    x[517, 5] = float("nan")
    s, r = query._query(x.to(DEV), to_dev(w), pos, neg, 10.0, True, True)
    bad = torch.isnan(s).any(1).cpu()
    assert bad[517] and bad.sum() == 1 and torch.isnan(s[517]).all() and torch.isnan(r[517]).all()
    assert not torch.isnan(r[torch.arange(1000) != 517]).any()
    keep = np.arange(1000) != 517
    assert np.abs(s.cpu().double().numpy()[keep] - ref_sims(x[keep], w, torch.cat([pos, neg]))).max() <= 2e-5
    # rows = 0
    s, r = query._query(torch.zeros(0, 32, device=DEV), to_dev(w), pos, neg, 10.0, True, True)
    assert s.shape == (0, 4) and r.shape == (0, 1)
    # scales
    for fs, ws in ((1e-4, 1.0), (1e4, 1.0), (1.0, 1e-4), (1.0, 1e4), (1e2, 1e2), (1e-2, 1e-2)):
        w = make_mlp(32, 512, seed=31, scale=ws)
        x = torch.randn(5000, 32) * fs
        s = query.clip_similarity(x.to(DEV), to_dev(w), torch.cat([pos, neg])).cpu().double().numpy()
        assert np.abs(s - ref_sims(x, w, torch.cat([pos, neg]))).max() <= 2e-5, (fs, ws)
    # an (H, W, D) non-contiguous view
    w = make_mlp(32, 512, seed=41)
    big = torch.randn(64, 96, 40, device=DEV)
    img = big[:, :, 4:36].transpose(0, 1)
    s = query.clip_similarity(img, to_dev(w), torch.cat([pos, neg]))
    assert s.shape == (96, 64, 4)
    ref = ref_sims(img.contiguous().cpu(), w, torch.cat([pos, neg])).reshape(96, 64, 4)
    assert np.abs(s.cpu().double().numpy() - ref).max() <= 2e-5


@gpu
def test_relevancy_view_on_the_plugin_model():
    from gaussiangrasper_amd import query
    from gaussiangrasper_amd.camera import ring_cameras
    from gaussiangrasper_amd.plugin import make_fused_model_class
    from gaussiangrasper_amd.scene import make_scene
    from gaussiangrasper_amd.stub import StubCameras, StubGaussianSplattingModel
    model = make_fused_model_class(StubGaussianSplattingModel)(make_scene(20_000, feature_dim=32)).to(DEV)
    model.train()
    cam = StubCameras.from_view(ring_cameras(2, 120, 160)[0], device=DEV)
    pos, neg = torch.randn(2, 512), torch.randn(3, 512)
    out = query.relevancy_view(model, cam, pos, neg, similarity=True)
    assert model.training
    assert out["relevancy"].shape == (120, 160, 2) and out["similarity"].shape == (120, 160, 5)
    assert out["relevancy"].grad_fn is None and out["similarity"].grad_fn is None
    model.eval()
    with torch.no_grad():
        feat = model.get_outputs(cam)["feature"]
    assert torch.equal(out["relevancy"], query.relevancy(feat, model.fea_up, pos, neg))
    assert torch.equal(out["similarity"], query.clip_similarity(feat, model.fea_up, torch.cat([pos, neg])))
    model.train()
    out2 = query.relevancy_view(model, cam, pos, neg)
    assert set(out2) == {"relevancy"} and torch.equal(out2["relevancy"], out["relevancy"])


@gpu
def test_no_full_size_intermediate():
    from gaussiangrasper_amd import query
    wd = to_dev(make_mlp(32, 512, seed=51))
    x = torch.randn(1200, 1600, 32, device=DEV)
    pos, neg = torch.randn(1, 512), torch.randn(3, 512)
    query.relevancy(x[:8], wd, pos, neg)                # warm the library and the allocator
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = query.relevancy(x, wd, pos, neg)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base - r.numel() * 4
    assert grown < 64 * 2 ** 20, grown / 2 ** 20      # the 3.9 GB fea_up output would not fit


@gpu
def test_select_gaussians_plants_a_cluster():
    from gaussiangrasper_amd import query
    from gaussiangrasper_amd.scene import make_scene
    w = make_mlp(32, 512, seed=61)
    sc = make_scene(50_000, feature_dim=32)
    g = torch.Generator().manual_seed(62)
    target = torch.randn(32, generator=g)
    feat = torch.randn(50_000, 32, generator=g)
    feat[:2000] = target + 0.05 * torch.randn(2000, 32, generator=g)     # the planted cluster
    sc.feature = feat
    w1, b1, w2, b2 = w
    y = torch.relu(feat @ w1.T + b1) @ w2.T + b2
    pos = (torch.relu(target @ w1.T + b1) @ w2.T + b2)[None]             # the cluster's own direction in CLIP space
    # canonical negatives: what every Gaussian looks like (the background's mean direction) and two random phrases
    neg = torch.cat([y[2000:].mean(0)[None], torch.randn(2, 512, generator=g)])
    scd = sc.to(DEV)
    thr = 0.9
    mask = query.select_gaussians(scd, to_dev(w), pos, neg, thr).cpu().numpy()
    r = ref_rel(ref_sims(feat, w, torch.cat([pos, neg])), 1)[:, 0]
    clear = np.abs(r - thr) > 1e-4
    assert np.array_equal(mask[clear], (r > thr)[clear])
    assert mask[:2000].all() and mask[2000:].mean() < 0.01


@gpu
def test_cli_on_a_synthetic_checkpoint(tmp_path):
    from gaussiangrasper_amd import interop, query
    from gaussiangrasper_amd.scene import make_scene
    w = make_mlp(32, 512, seed=71)
    sc = make_scene(30_000, feature_dim=32)
    state = dict(zip(("layers.0.weight", "layers.0.bias", "layers.2.weight", "layers.2.bias"), w))
    ck = tmp_path / "step-000030000.ckpt"
    interop.save_checkpoint(ck, sc, state, step=30000)
    rng = np.random.default_rng(72)
    pos, neg = rng.normal(size=(2, 512)).astype(np.float32), rng.normal(size=(3, 512)).astype(np.float32)
    np.save(tmp_path / "pos.npy", pos)
    np.save(tmp_path / "neg.npy", neg)
    out = tmp_path / "scores.npy"
    assert query.main(["--ckpt", str(ck), "--positives", str(tmp_path / "pos.npy"), "--negatives",
                       str(tmp_path / "neg.npy"), "--threshold", "0.5", "--out", str(out)]) == 0
    got = np.load(out)
    assert got.dtype == np.float32 and got.shape == (30_000, 2)
    want = query.relevancy_gaussians(sc.to(DEV), to_dev(w), pos, neg).cpu().numpy()
    assert np.array_equal(got, want)
    assert query.main(["--ckpt", str(ck), "--positives", str(tmp_path / "pos.npy"), "--out", str(out)]) == 0
    assert np.abs(np.load(out) - ref_sims(sc.feature, w, torch.from_numpy(pos))).max() <= 2e-5
