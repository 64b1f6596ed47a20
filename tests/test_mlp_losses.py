"""SURVEY 8f-2, second half: backward of the fea_up MLP and the cosine-similarity loss.  Both are
pinnable: the reference code is plain torch (nerfstudio/models/gaussian_splatting.py:113-118,198-213),
restated here in two lines each and differentiated by torch autograd."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mlp_ref


def ref_cosine_similarity_loss(e1, e2):          # gaussian_splatting.py:113-118
    e1, e2 = F.normalize(e1, dim=0), F.normalize(e2, dim=0)
    return 1 - torch.sum(e1 * e2, dim=0).mean()


def ref_mlp(x, w1, b1, w2, b2):                  # MLP.forward :198-213 (Linear, ReLU, Linear)
    return F.linear(F.relu(F.linear(x, w1, b1)), w2, b2)


def _mlp_case(p, in_dim, out_dim, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=dtype)
    return r(p, in_dim), r(128, in_dim) * 0.2, r(128) * 0.1, r(out_dim, 128) * 0.1, r(out_dim) * 0.1, r(p, out_dim)


@pytest.mark.parametrize("p,in_dim,out_dim", [(1, 8, 32), (37, 32, 512), (100, 128, 64)])
def test_oracle_mlp_backward_matches_torch_autograd(oracle, p, in_dim, out_dim):
    x, w1, b1, w2, b2, g = _mlp_case(p, in_dim, out_dim, seed=p)
    leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    ref_mlp(*leaves).backward(g)
    got = oracle.mlp_bwd(x.numpy(), w1.numpy(), b1.numpy(), w2.numpy(), g.numpy(), dtype=np.float64)
    for name, a, t in zip(("v_x", "v_w1", "v_b1", "v_w2", "v_b2"), got, leaves):
        assert np.allclose(a, t.grad.numpy(), rtol=1e-10, atol=1e-12), name
    got32 = oracle.mlp_bwd(*(t.float().numpy() for t in (x, w1, b1, w2, g)))
    for name, a, t in zip(("v_x", "v_w1", "v_b1", "v_w2", "v_b2"), got32, leaves):
        ref = t.grad.numpy()
        assert np.abs(a - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max()), name


@pytest.mark.parametrize("m,c", [(1, 3), (800, 32), (1000, 512)])
def test_oracle_cosine_loss_matches_torch_autograd(oracle, m, c):
    g = torch.Generator().manual_seed(m + c)
    a = torch.randn(m, c, generator=g, dtype=torch.float64)
    b = torch.randn(m, c, generator=g, dtype=torch.float64)
    if m > 2:
        a[1] = 0.0                      # F.normalize's eps clamp: zero vector, zero gradient through the norm
    ta, tb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    loss = ref_cosine_similarity_loss(ta.permute(1, 0), tb.permute(1, 0))
    (loss * 1.7).backward()
    l, sim, na, nb = oracle.cosine_loss_fwd(a.numpy(), b.numpy(), dtype=np.float64)
    assert abs(l - loss.item()) < 1e-12
    va, vb = oracle.cosine_loss_bwd(a.numpy(), b.numpy(), sim, na, nb, 1.7, dtype=np.float64)
    assert np.allclose(va, ta.grad.numpy(), rtol=1e-7, atol=1e-14)      # the zero row: gradients ~ b / eps = 1e9
    assert np.allclose(vb, tb.grad.numpy(), rtol=1e-7, atol=1e-14)
    l32, *_ = oracle.cosine_loss_fwd(a.float().numpy(), b.float().numpy())
    assert abs(l32 - loss.item()) < 2e-6


def test_product_modules_refuse_cpu_tensors():
    from gaussiangrasper_amd.losses import cosine_similarity_loss
    from gaussiangrasper_amd.mlp import MLP
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cosine_similarity_loss(torch.randn(8, 5), torch.randn(8, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MLP(32, 512, [128])(torch.randn(4, 32))
    with pytest.raises(NotImplementedError):
        MLP(32, 512, [64])
    MLP(128, 512, [128])     # BASELINE config 5's first layer: accepted (library GEMMs on the device)


DEV = "cuda:0"
gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("p,in_dim,out_dim", [(1, 32, 512), (1000, 32, 512), (777, 8, 96), (4099, 64, 512),
                                              (300, 128, 512),
                                              # output widths that clip the eight output groups (ob, o_hi): 1 and 7
                                              # leave most groups empty, 37 is no multiple of 8 or 32; 1024 outputs
                                              # with 128 inputs are the largest LDS request, 94 208 bytes
                                              (300, 16, 1), (300, 32, 7), (300, 32, 37), (64, 64, 1024),
                                              (64, 128, 1024)])
def test_gpu_mlp_backward_vs_oracle_and_autograd(oracle, p, in_dim, out_dim):
    from gaussiangrasper_amd.mlp import mlp_forward
    x, w1, b1, w2, b2, g = (t.float() for t in _mlp_case(p, in_dim, out_dim, seed=3 * p))
    dl = [t.clone().to(DEV).requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y = mlp_forward(*dl)
    y.backward(g.to(DEV))
    rl = [t.clone().double().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    ref_mlp(*rl).backward(g.double())
    want = oracle.mlp_bwd(x.numpy(), w1.numpy(), b1.numpy(), w2.numpy(), g.numpy())
    for name, t, r, o in zip(("v_x", "v_w1", "v_b1", "v_w2", "v_b2"), dl, rl, want):
        got, ref = t.grad.cpu().numpy().astype(np.float64), r.grad.numpy()
        scale = max(1.0, np.abs(ref).max())
        assert np.abs(got - ref).max() <= 3e-5 * scale, name          # fp32 sums vs fp64 autograd
        assert np.abs(got - o).max() <= 3e-5 * scale, name            # and vs the oracle


# The lattice cases (tests/mlp_ref.py): fp32 is exact on them, so gg_mlp_bwd must give the reference's bits whatever
# the order of its tiles and atomics.  32769 rows are 2049 tiles of 16 on a grid capped at 2048 workgroups: workgroup 0
# takes a second tile that holds one row.  65536 rows: every workgroup takes exactly two tiles (and in_dim 16, and 96
# outputs in eighths of 12).  15 / 16 / 17 rows: a ragged tile, a full one, one row into a second workgroup.
LATTICE_SHAPES = [(32769, 32, 512), (65536, 16, 96), (15, 8, 32), (16, 8, 32), (17, 8, 32)]


@functools.lru_cache(maxsize=None)
def _lattice_autograd(shape):
    """The five gradients of the lattice case of `shape` by fp64 torch autograd, as read-only numpy arrays with +0
    for every zero; computed once per process."""
    (x, w1, b1, w2, b2, g), _ = mlp_ref.lattice_reference(*shape)
    leaves = [torch.from_numpy(a.copy()).requires_grad_(True) for a in (x, w1, b1, w2, b2)]
    ref_mlp(*leaves).backward(torch.from_numpy(g.copy()))
    out = tuple(t.grad.numpy() + 0.0 for t in leaves)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("shape", LATTICE_SHAPES, ids=str)
def test_mlp_backward_lattice_case_is_exact_in_fp32(shape):
    """The condition under which the GPU test below may ask for bits: every term of every gradient element is a
    multiple of a unit u, the absolute values of an element's terms sum to less than 2^24 u, and an fp32 evaluation
    gives the same bits in two row orders, those of fp64 autograd."""
    (x, w1, b1, w2, b2, g), grads = mlp_ref.lattice_reference(*shape)
    cond, h = mlp_ref.condition(x, w1, b1, w2, g)
    for name, (unit, abs_sum) in cond.items():
        print(f"lattice {shape} {name}: unit {unit}, largest sum of |terms| {abs_sum / unit:.0f} units (2^24 = "
              f"16777216)")
        assert abs_sum < 2.0 ** 24 * unit, name
    for name, a in zip(("v_x", "v_w1", "v_b1", "v_w2", "v_b2"), grads):
        assert mlp_ref.is_multiple(a, cond[name][0]) and np.abs(a).max() <= cond[name][1], name
        assert a.any(), name
    # pre-activations exactly at 0, with a cotangent arriving there: relu'(0) = 0 (hp > 0) decides those gradients
    at_zero = h == 0.0
    arriving = (g @ w2)[at_zero]
    print(f"lattice {shape}: {int(at_zero.sum())} of {h.size} pre-activations are 0, {int((arriving != 0).sum())} "
          f"of them with a non-zero dL/dh")
    assert at_zero.sum() >= h.size // 100 and (arriving != 0).sum() >= at_zero.sum() // 10
    auto = _lattice_autograd(shape)
    perm = np.random.default_rng(1).permutation(shape[0])
    fwd = mlp_ref.backward(x, w1, b1, w2, g, dtype=np.float32)
    rev = mlp_ref.backward(x[perm], w1, b1, w2, g[perm], dtype=np.float32)
    rev = (rev[0][np.argsort(perm)],) + rev[1:]
    for name, a, b, c, d in zip(("v_x", "v_w1", "v_b1", "v_w2", "v_b2"), fwd, rev, grads, auto):
        assert a.dtype == np.float32 and a.tobytes() == b.tobytes(), name
        assert a.tobytes() == c.astype(np.float32).tobytes() == d.astype(np.float32).tobytes(), name
        assert np.array_equal(c, d), name


@gpu
@pytest.mark.parametrize("shape", LATTICE_SHAPES, ids=str)
def test_gpu_mlp_backward_is_exact_on_the_lattice(monkeypatch, shape):
    from gaussiangrasper_amd import _lib, mlp as M
    (x, w1, b1, w2, b2, g), _ = mlp_ref.lattice_reference(*shape)
    want = _lattice_autograd(shape)
    lib, calls = _lib.load(), []
    native = lib.gg_mlp_bwd

    def spy(rows, *args):
        calls.append(rows)
        return native(rows, *args)
    monkeypatch.setattr(lib, "gg_mlp_bwd", spy)
    assert shape[0] <= M.NATIVE_BWD_MAX_ROWS
    leaves = [torch.tensor(a, dtype=torch.float32, device=DEV).requires_grad_(True) for a in (x, w1, b1, w2, b2)]
    M.mlp_forward(*leaves).backward(torch.tensor(g, dtype=torch.float32, device=DEV))
    assert calls == [shape[0]]                                  # the native kernel ran, once
    for name, t, r in zip(("v_x", "v_w1", "v_b1", "v_w2", "v_b2"), leaves, want):
        got, ref = t.grad.cpu().numpy(), r.astype(np.float32)
        wrong = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
        print(f"mlp_bwd lattice {shape} {name}: {wrong} of {ref.size} elements differ from fp64 autograd")
        assert got.dtype == np.float32 and got.shape == ref.shape and wrong == 0, name


@gpu
def test_gpu_mlp_backward_large_row_count_uses_the_library_and_agrees():
    from gaussiangrasper_amd import mlp as M
    x, w1, b1, w2, b2, g = (t.float().to(DEV) for t in _mlp_case(3000, 32, 512, seed=5))
    res = []
    for cap in (1 << 16, 16):        # native kernel, then the GEMM path
        M.NATIVE_BWD_MAX_ROWS = cap
        leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
        M.mlp_forward(*leaves).backward(g)
        res.append([t.grad.clone() for t in leaves])
    M.NATIVE_BWD_MAX_ROWS = 1 << 16
    for a, b in zip(*res):
        assert torch.allclose(a, b, rtol=1e-4, atol=2e-5 * float(b.abs().max()))


@gpu
@pytest.mark.parametrize("m,c", [(1, 3), (800, 32), (1000, 512), (5000, 7), (70000, 17), (1_500_000, 3)])
def test_gpu_cosine_loss_vs_oracle_and_autograd(oracle, m, c):
    # (1.5 M x 3: the reference's normal loss runs it on every masked pixel of the normal image, :879)
    from gaussiangrasper_amd.losses import cosine_similarity_loss
    g = torch.Generator().manual_seed(m * c)
    a, b = torch.randn(m, c, generator=g), torch.randn(m, c, generator=g)
    if m > 2:
        a[1] = 0.0
    da, db = a.clone().to(DEV).requires_grad_(True), b.clone().to(DEV).requires_grad_(True)
    loss = cosine_similarity_loss(da.permute(1, 0), db.permute(1, 0))       # the reference's (C, M) call shape
    (loss * 1.7).backward()
    ta, tb = a.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = ref_cosine_similarity_loss(ta.permute(1, 0), tb.permute(1, 0))
    (ref * 1.7).backward()
    assert abs(loss.item() - ref.item()) < 3e-6
    l, sim, na, nb = oracle.cosine_loss_fwd(a.numpy(), b.numpy())
    assert abs(loss.item() - l) < (3e-6 if m < 100000 else 3e-5)     # fp32 sum of m terms on both sides
    va, vb = oracle.cosine_loss_bwd(a.numpy(), b.numpy(), sim, na, nb, 1.7)
    for got, r, o in ((da.grad, ta.grad, va), (db.grad, tb.grad, vb)):
        gg = got.cpu().numpy()
        assert np.allclose(gg, r.numpy(), rtol=2e-5, atol=1e-9)
        assert np.allclose(gg, o, rtol=2e-5, atol=1e-9)


def test_gather_pixels_equals_the_references_advanced_indexing():
    """losses.gather_pixels: values and gradients of the reference's per-set gathers (:912-917), through one
    index_select (pure torch; runs on the CPU)"""
    from gaussiangrasper_amd.losses import gather_pixels
    g = torch.Generator().manual_seed(0)
    img = torch.randn(20, 30, 5, generator=g).requires_grad_(True)
    sets = [torch.stack([torch.randint(0, 20, (m,), generator=g), torch.randint(0, 30, (m,), generator=g)], 1)
            for m in (7, 4, 9)]
    rows = gather_pixels(img, *sets)
    ref = [img[s[:, 0], s[:, 1]] for s in sets]
    for a, b in zip(rows, ref):
        assert torch.equal(a, b)
    w = [2.0, 1.0, -0.5]
    sum(wi * r.sum() for wi, r in zip(w, rows)).backward()
    got, img.grad = img.grad.clone(), None
    sum(wi * r.sum() for wi, r in zip(w, ref)).backward()
    assert torch.allclose(got, img.grad)
