"""The memory contract of the training path's C entry points, one test per family, every call through ctypes on a
sentinel arena (tests/arena.py) under the rules of tests/test_memory_contract_gpu.py:

  view chain            gg_view_fwd (+ gg_blend_fwd_pair_packed on its `records`), gg_shade_tail_fwd[_ex], gg_view_bwd,
                        gg_view_bwd_pose, gg_sh_bwd_multi
  projection fallback   gg_project_fwd, gg_project_fwd_count, gg_project_bwd, gg_project_bwd_ex
  binning               gg_bin_sort_dev_ex
  blend forward         gg_blend_fwd, gg_blend_fwd_pair, gg_blend_fwd_pair_fast, gg_blend_fwd_pair_packed
  blend backward        gg_blend_bwd, gg_blend_bwd_pair, gg_blend_bwd_deterministic
  MLP, cosine loss      gg_mlp_fwd, gg_mlp_fwd_fast, gg_mlp_bwd, gg_cosine_loss_fwd / _bwd

  * every device array at exactly the smallest alignment include/gg_raster.h and the entry's own checks allow (byte arrays
    at odd addresses, int64 at 8, quaternion rows, blend / binning / pose workspaces and packed records at 16), followed
    by a guard; a second layout where a coarser alignment selects another kernel build (16-byte aligned out_img,
    background, colors and v_out_img; a 16-float gradient record on a 64-byte boundary).  Which build a layout selects is
    tests/test_blend_dispatch.py's business: here both layouts hold the contract;
  * every workspace exactly the queried number of bytes, inside the arena, full of seeded garbage; every call made twice
    with different garbage: outputs the header and PARITY.md call deterministic are byte-equal, the float-atomic
    backwards within their bound both times;
  * outputs under the criterion of the family's present GPU test, imported where it is importable (no new tolerance);
  * accumulating outputs are inout regions preloaded with known values and come back as preload plus reference;
  * Arena.check() after every accepted call, Arena.untouched() after every refused or empty call, rebase() between the
    calls of a chain;
  * a pointer one step below its alignment is refused before any launch with the argument named in gg_last_error(),
    for every alignment rule an entry checks.  No call hands a kernel a pointer the header forbids."""
import ctypes

import numpy as np
import pytest
import torch

from arena import Arena
from test_memory_contract_gpu import _carve, _is_sentinel, _ptrs, _refused, _same_bytes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = ctypes.c_void_p
F32, F64, I32, I64, U8, U32 = np.float32, np.float64, np.int32, np.int64, np.uint8, np.uint32


def _lib():
    from gaussiangrasper_amd import _lib
    return _lib.load()


def _stream():
    return P(torch.cuda.current_stream().cuda_stream)


def _err():
    return _lib().gg_last_error().decode("utf-8", "replace")


def _bits(a):
    return np.ascontiguousarray(a).view(U32)


def _at(ar, align, *names):
    """the regions sit at exactly `align`: a multiple of it, not of twice it"""
    for k in names:
        assert ar.address(k) % (2 * align) == align, (k, align)


def _host_ptrs(ar, names, shift=None):
    """a host array of device pointers (v_out_img2_parts, viewdirs / v_colors of gg_sh_bwd_multi)"""
    q = _ptrs(ar, shift)
    return (ctypes.c_void_p * len(names))(*[q(k).value for k in names])


def _preload(shape, seed):
    """known values for an accumulating output: multiples of 2^-10 in +-0.25"""
    return (np.random.default_rng(seed).integers(-256, 257, shape) / 1024.0).astype(F32)


# ------------------------------------------------------------------------------------------------
# cosine loss
# ------------------------------------------------------------------------------------------------
def cosine_arena(a, b, seed):
    m, c = a.shape
    ar = Arena(DEV, seed)
    _carve(ar, "in", 4, a=a, b=b, v_loss=np.array([1.7], F32))
    _carve(ar, "out", 4, sim=np.empty(m, F32), norm_a=np.empty(m, F32), norm_b=np.empty(m, F32),
           sim_sum=np.empty(1, F32), v_a=np.empty((m, c), F32), v_b=np.empty((m, c), F32))
    return ar


def cosine_fwd(ar, m, c):
    q = _ptrs(ar)
    return _lib().gg_cosine_loss_fwd(m, c, q("a"), q("b"), q("sim"), q("norm_a"), q("norm_b"), q("sim_sum"), _stream())


def cosine_bwd(ar, m, c):
    q = _ptrs(ar)
    return _lib().gg_cosine_loss_bwd(m, c, q("a"), q("b"), q("sim"), q("norm_a"), q("norm_b"), q("v_loss"), q("v_a"),
                                     q("v_b"), _stream())


@pytest.mark.parametrize("m,c", [(1, 3), (5000, 7)])
def test_cosine_loss(oracle, m, c):
    """criterion: tests/test_mlp_losses.py test_gpu_cosine_loss_vs_oracle_and_autograd (loss within 3e-6, gradients
    rtol 2e-5, atol 1e-9, against the oracle and against fp64 autograd)"""
    from test_mlp_losses import ref_cosine_similarity_loss
    g = torch.Generator().manual_seed(m * c)
    a, b = torch.randn(m, c, generator=g), torch.randn(m, c, generator=g)
    if m > 2:
        a[1] = 0.0
    ta, tb = a.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = ref_cosine_similarity_loss(ta.permute(1, 0), tb.permute(1, 0))
    (ref * 1.7).backward()
    a, b = a.numpy(), b.numpy()
    l, sim, na, nb = oracle.cosine_loss_fwd(a, b)
    va, vb = oracle.cosine_loss_bwd(a, b, sim, na, nb, 1.7)
    for seed in (1, 2):
        ar = cosine_arena(a, b, seed)
        _at(ar, 4, "a", "b", "sim", "norm_a", "norm_b", "sim_sum", "v_a", "v_b")
        assert cosine_fwd(ar, m, c) == 0, _err()
        out = ar.check()
        loss = 1.0 - float(out["sim_sum"][0]) / m
        assert abs(loss - ref.item()) < 3e-6 and abs(loss - l) < 3e-6
        assert _is_sentinel(ar, "v_a", out["v_a"]) and _is_sentinel(ar, "v_b", out["v_b"])
        kept = {k: out[k].copy() for k in ("sim", "norm_a", "norm_b", "sim_sum")}
        ar.rebase()
        assert cosine_bwd(ar, m, c) == 0, _err()
        out = ar.check()
        _same_bytes(out, kept, kept)                            # the backward only reads what the forward kept
        for got, r, o in ((out["v_a"], ta.grad, va), (out["v_b"], tb.grad, vb)):
            assert np.allclose(got, r.numpy(), rtol=2e-5, atol=1e-9)
            assert np.allclose(got, o, rtol=2e-5, atol=1e-9)
    # num_points == 0: the forward zeroes sim_sum and writes nothing else, the backward writes nothing
    ar = cosine_arena(a, b, 3)
    assert cosine_fwd(ar, 0, c) == 0, _err()
    out = ar.check()
    assert out["sim_sum"][0] == 0.0
    assert all(_is_sentinel(ar, k, out[k]) for k in ("sim", "norm_a", "norm_b", "v_a", "v_b"))
    ar.rebase()
    assert cosine_bwd(ar, 0, c) == 0, _err()
    ar.untouched()


# ------------------------------------------------------------------------------------------------
# gg_mlp_fwd, gg_mlp_fwd_fast, gg_mlp_bwd
# ------------------------------------------------------------------------------------------------
def _mlp_weights(rows, in_dim, out_dim, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, in_dim, generator=g)
    w1, b1 = torch.randn(128, in_dim, generator=g) * 0.3, torch.randn(128, generator=g)
    w2, b2 = torch.randn(out_dim, 128, generator=g) * 0.2, torch.randn(out_dim, generator=g)
    return [t.numpy() for t in (x, w1, b1, w2, b2)]


def mlp_fwd_call(fast, x, w1, b1, w2, b2, seed, shift=None, rows=None):
    lib = _lib()
    n, in_dim = x.shape
    out_dim = len(b2)
    ar = Arena(DEV, seed)
    ar.carve("x", x, 16, "in")
    _carve(ar, "in", 4 if fast else 16, w1=w1, w2=w2)         # gg_mlp_fwd stages the weights four floats per load
    _carve(ar, "in", 4, b1=b1, b2=b2)
    ar.carve("y", np.empty((n, out_dim), F32), 16, "out")
    q = _ptrs(ar, shift)
    rows = n if rows is None else rows
    if not fast:
        return ar, lib.gg_mlp_fwd(rows, in_dim, 128, out_dim, q("x"), q("w1"), q("b1"), q("w2"), q("b2"), q("y"),
                                  _stream()), 0
    need = lib.gg_mlp_fwd_fast_workspace(in_dim, 128, out_dim)
    ar.carve("ws", need, 16, "ws")
    return ar, lib.gg_mlp_fwd_fast(rows, in_dim, 128, out_dim, q("x"), q("w1"), q("b1"), q("w2"), q("b2"), q("y"),
                                   q("ws"), need, _stream()), need


MLP_FWD = [("exact", 300, 32, 64), ("exact", 17, 128, 32), ("fast", 300, 32, 48), ("fast", 17, 128, 512)]


@pytest.mark.parametrize("kind,rows,in_dim,out_dim", MLP_FWD)
def test_mlp_forward(oracle, kind, rows, in_dim, out_dim):
    """gg_mlp_fwd: the oracle's bits (tests/test_gpu_parity.py test_mlp_fwd_bitexact_vs_oracle).  gg_mlp_fwd_fast: the
    bound of test_mlp_fwd_fast_is_fp32_grade: max |err| <= 1e-6 of the largest fp64 output and, where gg_mlp_fwd takes the
    shape, <= 1.5 times the exact kernel's error + 1e-8 (the exact kernel's outputs are the oracle's bits)"""
    from test_gpu_parity import _mlp_ref64, assert_bitexact
    fast = kind == "fast"
    w = _mlp_weights(rows, in_dim, out_dim, 3 * rows + in_dim + out_dim)
    ref64 = _mlp_ref64(*w)
    scale = np.abs(ref64).max()
    exact = oracle.mlp_fwd(*w) if out_dim % 32 == 0 else None
    runs = []
    for seed in (1, 2):
        ar, st, need = mlp_fwd_call(fast, *w, seed)
        assert st == 0, _err()
        _at(ar, 16, "x", "y", *(("ws",) if fast else ()))
        _at(ar, 4 if fast else 16, "w1", "w2")
        _at(ar, 4, "b1", "b2")
        out = ar.check()
        if fast:
            assert need > 0 and ar.nbytes("ws") == need
            err_fast = np.abs(out["y"] - ref64).max() / scale
            assert err_fast <= 1e-6, err_fast
            if exact is not None:
                err_exact = np.abs(exact - ref64).max() / scale
                assert err_fast <= 1.5 * err_exact + 1e-8, (err_fast, err_exact)
        else:
            assert_bitexact(out["y"], exact, "gg_mlp_fwd")
        runs.append(out)
    _same_bytes(runs[0], runs[1], ("y",))
    ar, st, _ = mlp_fwd_call(fast, *w, 3, rows=0)                       # num_rows == 0 does nothing
    assert st == 0, _err()
    ar.untouched()
    for name in ("x", "y") if fast else ("x", "y", "w1", "w2"):         # one check, one message per argument
        ar, st, _ = mlp_fwd_call(fast, *w, 4, shift={name: 4})
        _refused(ar, st, name)
    if fast:
        ar, st, _ = mlp_fwd_call(fast, *w, 4, shift={"ws": 4})
        _refused(ar, st, "workspace")


MLP_GRADS = ("v_x", "v_w1", "v_b1", "v_w2", "v_b2")


def mlp_bwd_call(x, w1, b1, w2, g, seed, rows=None):
    n, in_dim = x.shape
    out_dim = w2.shape[0]
    ar = Arena(DEV, seed)
    _carve(ar, "in", 4, x=x, w1=w1, b1=b1, w2=w2, g=g)
    _carve(ar, "out", 4, v_x=np.empty_like(x), v_w1=np.empty_like(w1), v_b1=np.empty_like(b1), v_w2=np.empty_like(w2),
           v_b2=np.empty(out_dim, F32))
    q = _ptrs(ar)
    st = _lib().gg_mlp_bwd(n if rows is None else rows, in_dim, 128, out_dim, q("x"), q("w1"), q("b1"), q("w2"), q("g"),
                           *[q(k) for k in MLP_GRADS], _stream())
    return ar, st


@pytest.mark.parametrize("rows,in_dim,out_dim", [(300, 32, 37), (17, 8, 32)])
def test_mlp_backward(oracle, rows, in_dim, out_dim):
    """criterion: tests/test_mlp_losses.py test_gpu_mlp_backward_vs_oracle_and_autograd: 3e-5 max(1, max|ref|) against
    fp64 autograd and against the oracle (float atomics: a bound, both times)"""
    import test_mlp_losses as M
    x, w1, b1, w2, b2, g = (t.float() for t in M._mlp_case(rows, in_dim, out_dim, seed=3 * rows))
    leaves = [t.clone().double().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    M.ref_mlp(*leaves).backward(g.double())
    args = [t.numpy() for t in (x, w1, b1, w2, g)]
    want = oracle.mlp_bwd(*args)
    for seed in (1, 2):
        ar, st = mlp_bwd_call(*args, seed)
        assert st == 0, _err()
        _at(ar, 4, "x", "w1", "b1", "w2", "g", *MLP_GRADS)
        out = ar.check()
        for name, t, o in zip(MLP_GRADS, leaves, want):
            ref = t.grad.numpy()
            scale = max(1.0, np.abs(ref).max())
            assert np.abs(out[name] - ref).max() <= 3e-5 * scale, name
            assert np.abs(out[name].astype(F64) - o).max() <= 3e-5 * scale, name
    # num_rows == 0: "all fully written" — the weight gradients are zeros, v_x has no rows
    ar, st = mlp_bwd_call(*args, 3, rows=0)
    assert st == 0, _err()
    out = ar.check()
    assert all(not out[k].any() for k in MLP_GRADS[1:]) and _is_sentinel(ar, "v_x", out["v_x"])


# ------------------------------------------------------------------------------------------------
# blend: the scenes both families run on
# ------------------------------------------------------------------------------------------------
_SCENES = {}


def _blend_scene(oracle, name):
    """name -> dict(n, h, w, ids, bins, xys, conics, opacity): a constructed case of tests/backward_cases.py, or the
    ragged 17 x 33 scene of 600 Gaussians of tests/test_fast_forward_batches.py (lists by the oracle's sort)"""
    if name not in _SCENES:
        import backward_cases as B
        if name == "ragged_600":
            from test_gpu_parity import _blend_inputs
            xys, depths, radii, conics, nth, _, opac, _ = _blend_inputs(oracle, 600, 17, 33, 1, seed=41)
            s = oracle.bin_and_sort(xys, depths, radii, nth, (3, 2, 1))
            sc = dict(n=600, h=17, w=33, ids=s["gaussian_ids_sorted"], bins=s["tile_bins"], xys=xys, conics=conics,
                      opacity=np.asarray(opac, F32).reshape(-1, 1))
            assert s["num_intersects"] > 600
        else:
            c = B.CASES[name]
            sc = dict(n=len(c.order), h=c.h, w=c.w, ids=B.ids_of(c), bins=c.tile_bins, xys=c.xys, conics=c.conics,
                      opacity=c.opacity)
        _SCENES[name] = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    return _SCENES[name]


def _carve_lists(ar, sc, ws_role="ws", ws_data=None):
    """ids, tile_bins, xys, conics, opacity at 4 bytes, the blend workspace at 16: exactly gg_blend_workspace bytes"""
    need = _lib().gg_blend_workspace(sc["n"])
    _carve(ar, "in", 4, ids=sc["ids"].astype(I32), tile_bins=sc["bins"].astype(I32), xys=sc["xys"], conics=sc["conics"],
           opacity=sc["opacity"])
    if ws_data is None:
        ar.carve("ws", need, 16, ws_role)
    else:
        assert ws_data.nbytes == need
        ar.carve("ws", ws_data, 16, ws_role)
    return need


# ------------------------------------------------------------------------------------------------
# blend forward
# ------------------------------------------------------------------------------------------------
# (entry, scene, channels of the second array): the single-array entries once per scene
FWD_RUNS = [(e, s, 0) for e in ("fwd_c3", "fwd_c35") for s in ("two_tiles_64", "ragged_600")] + \
           [(e, s, c2) for e in ("pair", "pair_fast", "packed", "packed_fast")
            for s, c2 in (("two_tiles_64", 7), ("ragged_600", 7), ("ragged_600", 1))]
_FWD_REF = {}


def _fwd_data(oracle, scene, c, c2):
    """colours, backgrounds and the oracle's images / final_Ts / final_idx of (scene, c + c2 channels), computed once"""
    key = (scene, c, c2)
    if key not in _FWD_REF:
        sc = _blend_scene(oracle, scene)
        rng = np.random.default_rng(100 * c + c2)
        col = rng.uniform(-1, 1, (sc["n"], c + c2)).astype(F32)
        bg = rng.uniform(0, 1, c + c2).astype(F32)
        img, ft, fi = oracle.blend_fwd(sc["ids"], sc["bins"], sc["xys"], sc["conics"], col, sc["opacity"], sc["h"],
                                       sc["w"], bg)
        empty = oracle.blend_fwd(sc["ids"], np.zeros_like(sc["bins"]), sc["xys"], sc["conics"], col, sc["opacity"],
                                 sc["h"], sc["w"], bg)
        _FWD_REF[key] = (col, bg, img, ft, fi, empty)
    return _FWD_REF[key]


def blend_fwd_call(sc, entry, col, bg, c, c2, wide, seed, shift=None, records=None, empty_lists=False):
    """one forward call; wide: out_img, background, colors on 16-byte boundaries (the batched forward's layout)"""
    lib = _lib()
    n, h, w = sc["n"], sc["h"], sc["w"]
    ar = Arena(DEV, seed)
    sc = dict(sc, bins=np.zeros_like(sc["bins"])) if empty_lists else sc
    packed = entry.startswith("packed")
    need = _carve_lists(ar, sc, "in" if packed else "ws", records)
    a = 16 if wide else 4
    ar.carve("colors", np.ascontiguousarray(col[:, :c]), a, "in")
    ar.carve("background", np.ascontiguousarray(bg[:c]), a, "in")
    ar.carve("out_img", np.empty((h, w, c), F32), a, "out")
    if c2:
        _carve(ar, "in", 4, colors2=np.ascontiguousarray(col[:, c:]), background2=np.ascontiguousarray(bg[c:]))
        ar.carve("out_img2", np.empty((h, w, c2), F32), 4, "out")
    _carve(ar, "out", 4, final_Ts=np.empty((h, w), F32), final_idx=np.empty((h, w), I32))
    q = _ptrs(ar, shift)
    lists = (n, h, w, q("ids"), q("tile_bins"))
    outs = (q("final_Ts"), q("final_idx"), q("ws"), need)
    if not c2:
        st = lib.gg_blend_fwd(c, *lists, q("xys"), q("conics"), q("colors"), q("opacity"), q("background"), q("out_img"),
                              *outs, _stream())
    elif packed:
        st = lib.gg_blend_fwd_pair_packed(c, c2, *lists, q("colors"), q("colors2"), q("background"), q("background2"),
                                          q("out_img"), q("out_img2"), *outs, int(entry == "packed_fast"), _stream())
    else:
        fn = lib.gg_blend_fwd_pair_fast if entry == "pair_fast" else lib.gg_blend_fwd_pair
        st = fn(c, c2, *lists, q("xys"), q("conics"), q("colors"), q("colors2"), q("opacity"), q("background"),
                q("background2"), q("out_img"), q("out_img2"), *outs, _stream())
    _at(ar, 16, "ws")
    _at(ar, a, "colors", "background", "out_img")
    _at(ar, 4, "ids", "tile_bins", "xys", "conics", "opacity", "final_Ts", "final_idx")
    return ar, st


def _fwd_hold(entry, out, img, ft, fi, c):
    """final_Ts / final_idx: the oracle's bits, always.  Images: the oracle's bits for the exact entries; for the batched
    ones tests/test_fast_forward.py's _close, 1e-6 (1 + |oracle|), which bit equality also meets"""
    from test_fast_forward import _close
    from test_gpu_parity import assert_bitexact
    assert_bitexact(out["final_Ts"], ft, entry + " final_Ts")
    assert_bitexact(out["final_idx"], fi, entry + " final_idx")
    pairs = [("out_img", img[..., :c])] + ([("out_img2", img[..., c:])] if "out_img2" in out else [])
    for k, r in pairs:
        if entry.endswith("fast"):
            _close(out[k], r, f"{entry} {k}")
        else:
            assert_bitexact(out[k], np.ascontiguousarray(r), f"{entry} {k}")


@pytest.mark.parametrize("entry,scene,c2", FWD_RUNS, ids=["%s-%s-c2_%d" % r for r in FWD_RUNS])
def test_blend_forward(oracle, entry, scene, c2):
    sc = _blend_scene(oracle, scene)
    c = {"fwd_c3": 3, "fwd_c35": 35}.get(entry, 32)
    col, bg, img, ft, fi, empty = _fwd_data(oracle, scene, c, c2)
    records = None
    if entry.startswith("packed"):
        # the workspace of an earlier forward over the same xys / conics / opacity, handed over as an INPUT: the packed
        # call reads it and check() holds it unchanged
        ar, st = blend_fwd_call(sc, "pair", col, bg, c, c2, False, 9)
        assert st == 0, _err()
        records = ar.check()["ws"]
    exact = ("out_img", "out_img2", "final_Ts", "final_idx") if not entry.endswith("fast") else ("final_Ts", "final_idx")
    for wide in (False, True) if c % 4 == 0 else (False,):      # 16-byte rows need channels % 4 == 0 to matter
        runs = []
        for seed in (1, 2):
            ar, st = blend_fwd_call(sc, entry, col, bg, c, c2, wide, seed, records=records)
            assert st == 0, _err()
            out = ar.check()
            _fwd_hold(entry, out, img, ft, fi, c)
            runs.append(out)
        _same_bytes(runs[0], runs[1], [k for k in exact if k in runs[0]])
        if records is None:                                     # the packing pass does not depend on the garbage either
            assert runs[0]["ws"][:32 * sc["n"]].tobytes() == runs[1]["ws"][:32 * sc["n"]].tobytes()
    # empty tile lists: every pixel is the background, final_T 1, final_idx 0 (the oracle's statement of it)
    ar, st = blend_fwd_call(sc, entry, col, bg, c, c2, False, 3, records=records, empty_lists=True)
    assert st == 0, _err()
    _fwd_hold(entry, ar.check(), *empty, c)
    assert (empty[1] == 1.0).all() and not empty[2].any()
    # blend_begin: ws on a 16-byte boundary
    ar, st = blend_fwd_call(sc, entry, col, bg, c, c2, False, 4, shift={"ws": 4}, records=records)
    _refused(ar, st, "ws")


# ------------------------------------------------------------------------------------------------
# blend backward
# ------------------------------------------------------------------------------------------------
BWD_CASES = ("two_tiles_64", "fin_inside_a_batch")
GG_BWD_WS_FROM_FORWARD, GG_BWD_ACCUMULATE_COLORS, GG_BWD_ACCUMULATE_GEOM = 1, 2, 4
# (entry, channels, layout of the gradient arrays, wide: colors and v_out_img on 16-byte boundaries)
BWD_SINGLE = [("gg_blend_bwd", 3, "dense", False), ("gg_blend_bwd", 3, "record", False),
              ("gg_blend_bwd", 3, "strided", False), ("gg_blend_bwd", 35, "dense", False),
              ("gg_blend_bwd", 35, "record", False), ("gg_blend_bwd", 35, "strided", False),
              ("gg_blend_bwd", 32, "dense", True), ("gg_blend_bwd", 32, "record", True),
              ("gg_blend_bwd", 32, "accumulate", False),
              ("gg_blend_bwd_deterministic", 3, "dense", False), ("gg_blend_bwd_deterministic", 32, "dense", True),
              ("gg_blend_bwd_deterministic", 17, "strided", False)]


def _bwd_inputs(ar, sc, data, c, c2, wide):
    ids, ft, fi, colors, bg, v_out, _ = data
    a = 16 if wide else 4
    ar.carve("colors", np.ascontiguousarray(colors[:, :c]), a, "in")
    ar.carve("v_out_img", np.ascontiguousarray(v_out[..., :c]), a, "in")
    _carve(ar, "in", 4, background=np.ascontiguousarray(bg[:c]), final_Ts=ft, final_idx=fi)
    if c2:
        _carve(ar, "in", 4, colors2=np.ascontiguousarray(colors[:, c:]), background2=np.ascontiguousarray(bg[c:]))


def _bwd_hold(what, got, ref):
    """tests/test_backward_batches.py's criterion against the fp64 oracle"""
    from test_backward_batches import ATOL_FRAC, RTOL
    from test_gpu_parity import assert_close
    for k, r in ref.items():
        assert_close(got[k].reshape(r.shape), r, f"memory_contract.{what}.{k}", rtol=RTOL, atol_frac=ATOL_FRAC)


def blend_bwd_call(sc, data, entry, c, layout, wide, seed, shift=None, n=None, empty_lists=False):
    """gg_blend_bwd / gg_blend_bwd_deterministic -> arena, status, the gradients as dense arrays (None if refused)"""
    lib = _lib()
    N, h, w = sc["n"], sc["h"], sc["w"]
    ar = Arena(DEV, seed)
    need = _carve_lists(ar, dict(sc, bins=np.zeros_like(sc["bins"])) if empty_lists else sc)
    _bwd_inputs(ar, sc, data, c, 0, wide)
    flags, gs, cs, pre = 0, 0, 0, {}
    if layout == "record":                       # one interleaved record of 6 + C floats per Gaussian
        gs = cs = 6 + c
        ar.carve("rec", np.empty((N, gs), F32), 4, "out")
    else:
        role = "inout" if layout == "accumulate" else "out"
        if layout == "accumulate":
            flags = GG_BWD_ACCUMULATE_COLORS | GG_BWD_ACCUMULATE_GEOM
            pre = {k: _preload(s, 7 + i) for i, (k, s) in enumerate((("v_xy", (N, 2)), ("v_conic", (N, 3)),
                                                                      ("v_opacity", (N, 1)), ("v_colors", (N, c))))}
        for k, cols in (("v_xy", 2), ("v_conic", 3), ("v_opacity", 1)):
            ar.carve(k, pre.get(k, np.empty((N, cols), F32)), 4, role)
        cs = c + 3 if layout == "strided" else 0                       # exactly N * color_stride floats
        ar.carve("v_colors", pre.get("v_colors", np.empty((N, cs or c), F32)), 4, role)
    det = entry.endswith("deterministic")
    count = len(sc["ids"])
    if det:
        det_need = lib.gg_blend_bwd_deterministic_workspace(N, c, count)
        ar.carve("det_ws", det_need, 4, "ws")
    q = _ptrs(ar, shift)
    if layout == "record":
        grads = (q("rec"), q("rec", 8), q("rec", 24), q("rec", 20))
    else:
        grads = (q("v_xy"), q("v_conic"), q("v_colors"), q("v_opacity"))
    args = (c, N if n is None else n, h, w, q("ids"), q("tile_bins"), q("xys"), q("conics"), q("colors"), q("opacity"),
            q("background"), q("final_Ts"), q("final_idx"), q("v_out_img"), *grads, gs, cs, q("ws"), need, flags)
    if det:
        st = lib.gg_blend_bwd_deterministic(*args, count, q("det_ws"), det_need, _stream())
    else:
        st = lib.gg_blend_bwd(*args, _stream())
    _at(ar, 16, "ws")
    _at(ar, 16 if wide else 4, "colors", "v_out_img")
    return ar, st, pre


def _single_grads(out, c, layout):
    if layout == "record":
        r = out["rec"]
        return {"v_xy": r[:, 0:2], "v_conic": r[:, 2:5], "v_opacity": r[:, 5:6], "v_colors": r[:, 6:]}
    g = {k: out[k] for k in ("v_xy", "v_conic", "v_opacity")}
    g["v_colors"] = out["v_colors"][:, :c]
    if layout == "strided":
        assert not out["v_colors"][:, c:].any(), "the call owns and clears the rows' padding"
    return g


@pytest.mark.parametrize("entry,c,layout,wide", BWD_SINGLE,
                         ids=["%s-c%d-%s%s" % (e[3:], c, l, "-wide" if w else "") for e, c, l, w in BWD_SINGLE])
@pytest.mark.parametrize("case", BWD_CASES)
def test_blend_backward(oracle, case, entry, c, layout, wide):
    """operands, final_T / final_idx and the fp64 reference: tests/test_backward_batches.py _case_data (the seeds of
    backward_cases.OPERAND_SEED); criterion: assert_close(rtol 5e-5, atol_frac 1e-6)"""
    from test_backward_batches import _case_data
    sc = _blend_scene(oracle, case)
    data = _case_data(oracle, case, c, 0)
    ref = data[6]
    det = entry.endswith("deterministic")
    runs = []
    for seed in (1, 2):
        ar, st, pre = blend_bwd_call(sc, data, entry, c, layout, wide, seed)
        assert st == 0, _err()
        out = ar.check()
        got = _single_grads(out, c, layout)
        _bwd_hold(f"{entry}.{layout}", got, {k: r + pre[k].astype(F64).reshape(r.shape) for k, r in ref.items()} if pre
                  else ref)
        runs.append(got)
    if det:
        _same_bytes(runs[0], runs[1], runs[0])
    # num_points == 0: GG_OK, nothing written; empty tile lists: the cleared arrays are the answer
    ar, st, _ = blend_bwd_call(sc, data, entry, c, layout, wide, 3, n=0)
    assert st == 0, _err()
    ar.untouched()
    if layout != "accumulate":
        ar, st, _ = blend_bwd_call(sc, data, entry, c, layout, wide, 3, empty_lists=True)
        assert st == 0, _err()
        out = ar.check()
        assert all(not out[k].any() for k in out if k not in ("ws", "det_ws"))
    ar, st, _ = blend_bwd_call(sc, data, entry, c, layout, wide, 4, shift={"ws": 4})
    _refused(ar, st, "ws")


BWD_PAIR = [("rec", (7,), False), ("rec", (3, 1, 3), False), ("rec16", (7,), True), ("rec16", (3, 1, 3), True),
            ("rec16", (7,), False)]


def blend_pair_call(sc, data, layout, parts, wide, seed, chain, shift=None, n=None):
    """gg_blend_bwd_pair, 32 + 7 channels, the geometry and the second array's gradients in one record per Gaussian (6 + c2
    floats, or 16 floats: on a 64-byte boundary when `wide`), v_colors dense.  chain: the matching gg_blend_fwd_pair runs
    first in the same arena, the backward takes its workspace (GG_BWD_WS_FROM_FORWARD) and adds to a preloaded v_colors
    (GG_BWD_ACCUMULATE_COLORS)."""
    lib = _lib()
    c, c2 = 32, 7
    N, h, w = sc["n"], sc["h"], sc["w"]
    v_out = data[5]
    ar = Arena(DEV, seed)
    need = _carve_lists(ar, sc)
    _bwd_inputs(ar, sc, data, c, c2, wide)
    at = np.cumsum((0,) + parts)
    names = []
    for k, (lo, hi) in enumerate(zip(at[:-1], at[1:])):
        names.append(f"v_out_img2_{k}")
        ar.carve(names[-1], np.ascontiguousarray(v_out[..., c + lo:c + hi]), 4, "in")
    stride = 16 if layout == "rec16" else 6 + c2
    ar.carve("rec", np.empty((N, stride), F32), 64 if (wide and stride == 16) else 4, "out")
    pre = _preload((N, c), 5) if chain else np.zeros((N, c), F32)
    ar.carve("v_colors", pre, 4, "inout" if chain else "out")
    if chain:
        _carve(ar, "out", 4, out_img=np.empty((h, w, c), F32), out_img2=np.empty((h, w, c2), F32),
               fwd_Ts=np.empty((h, w), F32), fwd_idx=np.empty((h, w), I32))
    q = _ptrs(ar, shift)
    head = (c, c2, N if n is None else n, h, w, q("ids"), q("tile_bins"), q("xys"), q("conics"), q("colors"), q("colors2"),
            q("opacity"), q("background"), q("background2"))
    fwd = None
    if chain:
        st = lib.gg_blend_fwd_pair(*head, q("out_img"), q("out_img2"), q("fwd_Ts"), q("fwd_idx"), q("ws"), need, _stream())
        assert st == 0, _err()
        fwd = ar.check()
        ar.rebase()
    chans = (ctypes.c_int * len(parts))(*parts)
    st = lib.gg_blend_bwd_pair(*head, q("final_Ts"), q("final_idx"), q("v_out_img"), _host_ptrs(ar, names, shift), chans,
                               len(parts), q("rec"), q("rec", 8), q("v_colors"), q("rec", 24), q("rec", 20), stride, 0,
                               stride, q("ws"), need,
                               (GG_BWD_ACCUMULATE_COLORS | GG_BWD_WS_FROM_FORWARD) if chain else 0, _stream())
    _at(ar, 16, "ws")
    _at(ar, 64 if (wide and stride == 16) else 4, "rec")
    return ar, st, pre, fwd


@pytest.mark.parametrize("layout,parts,wide", BWD_PAIR,
                         ids=["%s-%dparts%s" % (l, len(p), "-wide" if w else "") for l, p, w in BWD_PAIR])
@pytest.mark.parametrize("case", BWD_CASES)
def test_blend_backward_pair(oracle, case, layout, parts, wide):
    from test_backward_batches import _case_data
    from test_gpu_parity import assert_bitexact
    sc = _blend_scene(oracle, case)
    data = _case_data(oracle, case, 32, 7)
    ref = data[6]
    for chain in (False, True):
        for seed in (1, 2):
            ar, st, pre, fwd = blend_pair_call(sc, data, layout, parts, wide, seed, chain)
            assert st == 0, _err()
            out = ar.check()
            r = out["rec"]
            assert not r[:, 13:].any(), "the record's padding is cleared and stays clear"
            got = {"v_xy": r[:, 0:2], "v_conic": r[:, 2:5], "v_opacity": r[:, 5:6], "v_colors2": r[:, 6:13],
                   "v_colors": out["v_colors"]}
            _bwd_hold(f"gg_blend_bwd_pair.{layout}", got, dict(ref, v_colors=ref["v_colors"] + pre.astype(F64)))
            if chain:                            # the forward's own outputs, and the workspace the backward only reads
                assert_bitexact(fwd["fwd_Ts"], data[1], "final_Ts")
                assert_bitexact(fwd["fwd_idx"], data[2], "final_idx")
                _same_bytes(out, fwd, ("ws", "out_img", "out_img2", "fwd_Ts", "fwd_idx"))
    ar, st, _, _ = blend_pair_call(sc, data, layout, parts, wide, 3, False, n=0)       # num_points == 0
    assert st == 0, _err()
    ar.untouched()
    ar, st, _, _ = blend_pair_call(sc, data, layout, parts, wide, 4, False, shift={"ws": 4})
    _refused(ar, st, "ws")


# ------------------------------------------------------------------------------------------------
# binning: gg_bin_sort_dev_ex
# ------------------------------------------------------------------------------------------------
# None of tests/binning_cases.py's constructions puts ONE run across a bucket boundary: a run is by definition what one
# bucket holds, and group_case asserts that no group lies across a boundary.  What stands in for it is grid-16x16: its
# 3 007 depths, uniform in 0.5 .. 30, are cut by the boundaries wherever they fall, so consecutive depths land in
# neighbouring buckets (_neighbouring_runs asserts that on the CPU).  groups-ties-10468 (runs of 1 .. 1 025 with hundreds
# of ties) runs with the count equal to the capacity, the grid with 37 entries to spare.
BIN_CASES = [("grid-16x16", 37), ("groups-ties-10468", 0)]


def _neighbouring_runs(c):
    """the precondition of the grid case: most buckets are occupied, long stretches of neighbouring buckets all hold a
    run, and runs of several lengths occur (binning_cases.bucket_runs: for preconditions only)"""
    import binning_cases as BC
    nb, runs = BC.bucket_runs(c.depths, c.radii)
    full = runs > 0
    stretch = best = 0
    for f in full:
        stretch = stretch + 1 if f else 0
        best = max(best, stretch)
    assert full.sum() >= nb // 2 and best >= 16, (int(full.sum()), nb, best)
    assert len(set(runs[full].tolist())) >= 8 and runs.max() >= 16


def bin_call(c, count, capacity, parts, seed, shift=None, num=None):
    lib = _lib()
    n, ntiles = len(c.depths), c.tiles_x * c.tiles_y
    need = lib.gg_bin_sort_workspace(n, capacity)
    ar = Arena(DEV, seed)
    ar.carve("count", np.array([count], I64), 8, "in")
    _carve(ar, "in", 4, xys=c.xys, depths=c.depths, radii=c.radii, nth=c.nth)
    if parts is not None:
        _carve(ar, "in", 4, lo=parts[0].view(I32), hi=parts[1].view(I32))
    _carve(ar, "out", 4, ids=np.empty(capacity, I32), tile_bins=np.empty((ntiles, 2), I32), tiles=np.empty(capacity, I32))
    ar.carve("ws", need, 16, "ws")
    q = _ptrs(ar, shift)
    st = lib.gg_bin_sort_dev_ex(n if num is None else num, capacity, q("count"), q("xys"), q("depths"), q("radii"), q("nth"), c.tiles_x, c.tiles_y,
                                q("ids"), q("tile_bins"), q("tiles"), q("ws"), need, q("lo" if parts else None),
                                q("hi" if parts else None), len(parts[0]) if parts else 0, _stream())
    _at(ar, 16, "ws")
    _at(ar, 8, "count")
    _at(ar, 4, "xys", "depths", "radii", "nth", "ids", "tile_bins", "tiles")
    return ar, st, need


@pytest.mark.parametrize("with_parts", [False, True], ids=["own_range", "range_parts"])
@pytest.mark.parametrize("name,spare", BIN_CASES)
def test_bin_sort(oracle, name, spare, with_parts):
    """criterion: tests/test_binning_constructed.py's equality with the oracle's 64-bit sort"""
    import binning_cases as BC
    from test_binning_constructed import _assert_equals_oracle, _reference
    c, count, ref_ids, ref_bins = _reference(oracle, name)
    if name.startswith("grid"):
        _neighbouring_runs(c)
    parts = BC.range_parts(c.depths, c.radii, 256) if with_parts else None
    capacity = count + spare
    runs = []
    for seed in (1, 2):
        ar, st, need = bin_call(c, count, capacity, parts, seed)
        assert st == 0 and need > 0 and ar.nbytes("ws") == need, _err()
        out = ar.check()
        _assert_equals_oracle((out["ids"], out["tiles"], out["tile_bins"]), count, ref_ids, ref_bins, name)
        runs.append({"ids": out["ids"][:count], "tiles": out["tiles"][:count], "tile_bins": out["tile_bins"]})
    _same_bytes(runs[0], runs[1], ("ids", "tiles", "tile_bins"))
    # num_points == 0: every range (0, 0), nothing else is written
    ar, st, _ = bin_call(c, count, capacity, parts, 3, num=0)
    assert st == 0, _err()
    out = ar.check()
    assert not out["tile_bins"].any() and _is_sentinel(ar, "ids", out["ids"]) and _is_sentinel(ar, "tiles", out["tiles"])
    assert out["ws"].tobytes() == ar.before("ws").tobytes()
    ar, st, _ = bin_call(c, count, capacity, parts, 4, shift={"ws": 4})
    _refused(ar, st, "ws")


# ------------------------------------------------------------------------------------------------
# the view chain (tests/view_chain_cases.py at 17 x 33: ragged both ways)
# ------------------------------------------------------------------------------------------------
VIEW = "17x33"
VIEW_N = (257, 1)          # two workgroups, the second holding one Gaussian; one Gaussian
FWD_FLOATS = ("scales", "quats_n", "opac", "viewdirs", "normals", "xys", "depths", "conics")
FWD_INTS = ("axis", "radii", "num_tiles_hit")


def _view_case(n):
    import view_chain_cases as vc
    c = vc.cases()[VIEW]
    return c, c.view


def view_fwd_call(n, seed, shift=None, num=None, lists=None):
    """gg_view_fwd; lists = (ids, tile_bins, colours, backgrounds): also carved, for the packed forward that follows"""
    lib = _lib()
    c, v = _view_case(n)
    blocks = (n + 255) // 256
    need, rneed = lib.gg_view_fwd_workspace(n), lib.gg_blend_workspace(n)
    assert need == 12 * blocks
    ar = Arena(DEV, seed)
    _carve(ar, "in", 4, means=c.means[:n], log_scales=c.log_scales[:n], opacities=c.opacities[:n],
           cam_pos=np.asarray(v.cam_pos, F32).reshape(-1)[:3], viewmat=np.asarray(v.viewmat, F32)[:3],
           projmat=np.asarray(v.full_proj, F32))
    ar.carve("quats", c.quats[:n], 16, "in")
    _carve(ar, "out", 4, scales=np.empty((n, 3), F32), opac=np.empty((n, 1), F32), viewdirs=np.empty((n, 3), F32),
           normals=np.empty((n, 3), F32), axis=np.empty(n, I32), xys=np.empty((n, 2), F32), depths=np.empty(n, F32),
           radii=np.empty(n, I32), conics=np.empty((n, 3), F32), num_tiles_hit=np.empty(n, I32))
    ar.carve("quats_n", np.empty((n, 4), F32), 16, "out")
    ar.carve("total", np.empty(1, I64), 8, "out")
    ar.carve("parts", np.empty(3 * blocks, U32), 4, "ws")
    ar.carve("records", rneed, 16, "ws")
    if lists is not None:
        ids, bins, col, bg = lists
        _carve(ar, "in", 4, ids=ids, tile_bins=bins, colors=np.ascontiguousarray(col[:, :32]),
               colors2=np.ascontiguousarray(col[:, 32:]), background=np.ascontiguousarray(bg[:32]),
               background2=np.ascontiguousarray(bg[32:]))
        _carve(ar, "out", 4, out_img=np.empty((v.h, v.w, 32), F32), out_img2=np.empty((v.h, v.w, 7), F32),
               final_Ts=np.empty((v.h, v.w), F32), final_idx=np.empty((v.h, v.w), I32))
    q = _ptrs(ar, shift)
    tb = v.tile_bounds
    st = lib.gg_view_fwd(n if num is None else num, q("means"), q("log_scales"), q("quats"), q("opacities"), q("cam_pos"),
                         q("viewmat"), q("projmat"), v.fx, v.fy, v.cx, v.cy, v.h, v.w, int(tb[0]), int(tb[1]), float(v.clip),
                         q("scales"), q("quats_n"), q("opac"), q("viewdirs"), q("normals"), q("axis"), q("xys"), q("depths"),
                         q("radii"), q("conics"), q("num_tiles_hit"), q("total"), q("parts"), need, q("records"), rneed,
                         _stream())
    _at(ar, 16, "quats", "quats_n", "records")
    _at(ar, 8, "total")
    _at(ar, 4, "means", "parts", "xys", "conics")
    return ar, st


def _view_fwd_hold(out, n):
    """tests/test_view_chain_gpu.py test_view_forward_against_the_restatement's statements"""
    import view_chain_cases as vc
    from test_view_chain_gpu import MARGIN_X, _hold, _ref_forward
    want = _ref_forward(VIEW, n)
    for k in FWD_INTS:
        assert np.array_equal(out[k].astype(I64), want[k].numpy().astype(I64)), k
    assert int(out["total"][0]) == int(want["num_tiles_hit"].sum())
    bound = MARGIN_X * vc.FWD_WORST
    for k in FWD_FLOATS:
        assert not np.isnan(out[k]).any(), k
        _hold(f"memory contract view fwd {k}[n={n}]", torch.from_numpy(out[k]),
              want["conics_written" if k == "conics" else k].detach(), bound)
    blocks = (n + 255) // 256
    parts = out["parts"].reshape(3, blocks)
    vis, nth, bits = want["vis"].numpy(), want["num_tiles_hit"].numpy(), _bits(out["depths"])
    for b in range(blocks):
        sl = slice(256 * b, min(256 * (b + 1), n))
        assert parts[0, b] == nth[sl].sum(), b
        if vis[sl].any():
            assert parts[1, b] == bits[sl][vis[sl]].min() and parts[2, b] == bits[sl][vis[sl]].max(), b
        else:
            assert parts[1, b] == 0xFFFFFFFF and parts[2, b] == 0, b


@pytest.mark.parametrize("n", VIEW_N)
def test_view_forward(oracle, n):
    """gg_view_fwd twice, the second time followed in the same arena by gg_blend_fwd_pair_packed on its `records` (lists by
    the oracle's sort of the first run's outputs; images, final_Ts, final_idx: the oracle's bits on those outputs)"""
    from test_gpu_parity import assert_bitexact
    c, v = _view_case(n)
    ar, st = view_fwd_call(n, 1)
    assert st == 0, _err()
    first = ar.check()
    _view_fwd_hold(first, n)
    s = oracle.bin_and_sort(first["xys"], first["depths"], first["radii"], first["num_tiles_hit"], v.tile_bounds)
    rng = np.random.default_rng(n)
    col, bg = rng.uniform(-1, 1, (n, 39)).astype(F32), rng.uniform(0, 1, 39).astype(F32)
    ids = s["gaussian_ids_sorted"] if s["num_intersects"] else np.zeros(1, I32)
    ar, st = view_fwd_call(n, 2, lists=(ids, s["tile_bins"], col, bg))
    assert st == 0, _err()
    second = ar.check()
    _view_fwd_hold(second, n)
    keys = FWD_FLOATS + FWD_INTS + ("total", "parts")
    _same_bytes(first, second, keys)
    assert first["records"][:32 * n].tobytes() == second["records"][:32 * n].tobytes()
    assert all(_is_sentinel(ar, k, second[k]) for k in ("out_img", "out_img2", "final_Ts", "final_idx"))
    ar.rebase()
    q = _ptrs(ar)
    rneed = ar.nbytes("records")
    for fast in (0, 1):
        st = _lib().gg_blend_fwd_pair_packed(32, 7, n, v.h, v.w, q("ids"), q("tile_bins"), q("colors"), q("colors2"),
                                             q("background"), q("background2"), q("out_img"), q("out_img2"), q("final_Ts"),
                                             q("final_idx"), q("records"), rneed, fast, _stream())
        assert st == 0, _err()
        out = ar.check()
        _same_bytes(out, second, keys + ("records",))            # the packed forward only reads the chain's outputs
        img, ft, fi = oracle.blend_fwd(ids, s["tile_bins"], first["xys"], first["conics"], col, first["opac"], v.h, v.w, bg)
        _fwd_hold("packed_fast" if fast else "packed", out, img, ft, fi, 32)
        ar.rebase()
    # num_points == 0: the count is written, 0, and nothing else
    ar, st = view_fwd_call(n, 3, num=0)
    assert st == 0, _err()
    out = ar.check()
    assert out["total"][0] == 0
    assert all(_is_sentinel(ar, k, out[k]) for k in FWD_FLOATS + FWD_INTS)
    assert out["parts"].tobytes() == ar.before("parts").tobytes() and out["records"].tobytes() == ar.before("records").tobytes()
    if n == 257:
        for name in ("quats", "quats_n", "records"):
            ar, st = view_fwd_call(n, 4, shift={name: 4})
            _refused(ar, st, name)


def _chain(n, deg=4, full=True, which=1):
    """inputs for the calls behind the forward: the kernels' own forward outputs of the case (torch tensors -> numpy)"""
    from test_view_chain_gpu import _chain_forward
    sc, view, v, geo, mask = _chain_forward(_lib(), VIEW, n, deg, full, which)
    g = {k: t.cpu().numpy() for k, t in geo.items() if k not in ("total", "parts", "records")}
    return sc, view, v, g, mask.cpu().numpy()


def tail_call(n, k, deg, coeffs, geo, variant, seed, num=None):
    lib = _lib()
    ar = Arena(DEV, seed)
    _carve(ar, "in", 4, viewdirs=geo["viewdirs"], coeffs=coeffs, depths=geo["depths"], normals=geo["normals"])
    ar.carve("tail", np.empty((n, 7), F32), 4, "out")
    ar.carve("clamp_mask", np.empty(n, U8), 1, "out")
    q = _ptrs(ar)
    args = (n if num is None else num, k, deg, q("viewdirs"), q("coeffs"), q("depths"), q("normals"), q("tail"),
            q("clamp_mask"))
    st = lib.gg_shade_tail_fwd(*args, _stream()) if variant is None else lib.gg_shade_tail_fwd_ex(*args, variant, _stream())
    _at(ar, 1, "clamp_mask")
    _at(ar, 4, "viewdirs", "coeffs", "depths", "normals", "tail")
    return ar, st


@pytest.mark.parametrize("n", VIEW_N)
def test_shade_tail_forward(n):
    """tests/test_view_chain_gpu.py test_shade_tail_forward_against_the_restatement's statements, degree 4, 25 bases:
    gg_shade_tail_fwd and gg_shade_tail_fwd_ex with one_wave 0 / 1, the same bytes from all three"""
    import view_chain_cases as vc
    from test_view_chain_gpu import MARGIN_X, _ref_forward
    sc, view, v, geo, _ = _chain(n)
    coeffs = sc.colors_all.cpu().numpy()
    want = _ref_forward(VIEW, n)
    runs = []
    for variant in (None, 0, 1):
        for seed in (1, 2):
            ar, st = tail_call(n, 25, 4, coeffs, geo, variant, seed)
            assert st == 0, _err()
            out = ar.check()
            assert np.array_equal(out["clamp_mask"], want["mask"].numpy())
            err = np.abs(out["tail"][:, :3].astype(F64) - want["tail"][:, :3].detach().numpy()).max()
            assert err <= MARGIN_X * vc.FWD_WORST, (variant, err)
            assert out["tail"][:, 3].tobytes() == geo["depths"].tobytes()
            assert np.ascontiguousarray(out["tail"][:, 4:7]).tobytes() == geo["normals"].tobytes()
            runs.append(out)
    for r in runs[1:]:
        _same_bytes(runs[0], r, ("tail", "clamp_mask"))
    for variant in (None, 1):                                           # num_points == 0 does nothing
        ar, st = tail_call(n, 25, 4, coeffs, geo, variant, 3, num=0)
        assert st == 0, _err()
        ar.untouched()


SINKS = ("v_means", "v_log_scales", "v_quats", "v_opacities")


def view_bwd_call(n, pose, stride, sc, v, geo, mask, rec, start, seed, shift=None, num=None):
    lib = _lib()
    ar = Arena(DEV, seed)
    ar.carve("rec", np.ascontiguousarray(rec[:, :stride]), 16 if stride % 4 == 0 else 4, "in")
    ar.carve("clamp_mask", mask, 1, "in")
    _carve(ar, "in", 4, means=sc.means.cpu().numpy(), scales=geo["scales"], opac=geo["opac"], axis=geo["axis"],
           viewmat=np.asarray(v.viewmat, F32)[:3], projmat=np.asarray(v.full_proj, F32), radii=geo["radii"],
           conics=geo["conics"])
    _carve(ar, "in", 16, quats_raw=sc.quats.cpu().numpy(), quats_n=geo["quats_n"])
    ar.carve("v_rgb", np.empty((n, 3), F32), 4, "out")
    for k, a in zip(SINKS, start):
        ar.carve(k, a, 16 if k == "v_quats" else 4, "inout")
    if pose:
        need = lib.gg_pose_grad_workspace(n)
        _carve(ar, "out", 4, v_viewmat=np.empty(12, F32), v_projmat=np.empty(16, F32))
        ar.carve("ws", need, 16, "ws")
    q = _ptrs(ar, shift)
    args = (n if num is None else num, q("rec"), stride, q("clamp_mask"), q("means"), q("scales"), 1.0, q("quats_raw"),
            q("quats_n"), q("opac"), q("axis"), q("viewmat"), q("projmat"), v.fx, v.fy, v.h, v.w, q("radii"), q("conics"),
            q("v_rgb"), *[q(k) for k in SINKS])
    if pose:
        st = lib.gg_view_bwd_pose(*args, q("v_viewmat"), q("v_projmat"), q("ws"), need, _stream())
        _at(ar, 16, "ws")
    else:
        st = lib.gg_view_bwd(*args, _stream())
    _at(ar, 16, "quats_raw", "quats_n", "v_quats")
    _at(ar, 16 if stride % 4 == 0 else 4, "rec")
    _at(ar, 1, "clamp_mask")
    return ar, st


@pytest.mark.parametrize("n", VIEW_N)
def test_view_backward(n):
    """gg_view_bwd and gg_view_bwd_pose, records of 13 floats (4-byte aligned) and of 16 (16-byte aligned, columns 13 .. 15
    NaN), as tests/test_view_chain_gpu.py test_view_backward_against_the_restatement holds them: from zeroed sinks the
    gradients against the restatement per Gaussian; from preloaded sinks fl(preload + that gradient), bit for bit; the
    pose sums within 1e-5 of their absolute sums and the same bytes on every call"""
    import view_chain_cases as vc
    import view_chain_ref as ref
    from test_view_chain_gpu import MARGIN_X, _hold, _ref_grads, _starts
    c, _ = _view_case(n)
    sc, view, v, geo, mask = _chain(n)
    want = _ref_grads(VIEW, n)
    rec = c.record[:n]
    assert np.isnan(rec[:, 13:]).all()
    open_ = np.stack([(mask >> ch) & 1 for ch in range(3)], -1).astype(bool)
    rgb_want = np.where(open_, rec[:, 6:9], F32(0))
    zero = [t.cpu().numpy() for t in _starts(n, zero=True)]
    start = [t.cpu().numpy() for t in _starts(n, zero=False)]
    ar, st = view_bwd_call(n, False, 16, sc, v, geo, mask, rec, zero, 1)
    assert st == 0, _err()
    base = ar.check()
    assert base["v_rgb"].tobytes() == rgb_want.tobytes()
    for p, k in zip(ref.PARAMS, SINKS):
        floor = ref.opacity_floor(c.record, n) if p == "opacities" else None
        _hold(f"memory contract gg_view_bwd {p}[n={n}]", torch.from_numpy(base[k]), want[p], MARGIN_X * vc.ORACLE_WORST[p],
              floor)
    expect = {k: (s + base[k]).astype(F32) for k, s in zip(SINKS, start)}        # one fp32 addition per element
    poses = []
    for stride in (13, 16):
        for pose in (False, True):
            for seed in (1, 2):
                ar, st = view_bwd_call(n, pose, stride, sc, v, geo, mask, rec, start, seed)
                assert st == 0, _err()
                out = ar.check()
                assert out["v_rgb"].tobytes() == rgb_want.tobytes(), (stride, pose)
                for k in SINKS:
                    assert out[k].tobytes() == expect[k].tobytes(), (k, stride, pose)
                if pose:
                    for key, shape in (("viewmat", (3, 4)), ("projmat", (4, 4))):
                        err = np.abs(out["v_" + key].reshape(shape).astype(F64) - ref.f64(want["v_" + key]).numpy())
                        assert (err <= 1e-5 * ref.f64(want["abs_" + key]).numpy() + 1e-30).all(), (key, stride)
                    assert not out["v_projmat"].reshape(4, 4)[2].any()
                    poses.append(out)
    for p in poses[1:]:
        _same_bytes(poses[0], p, ("v_viewmat", "v_projmat"))
    # num_points == 0: gg_view_bwd writes nothing; gg_view_bwd_pose zeros to the 28 pose floats and nothing else
    ar, st = view_bwd_call(n, False, 13, sc, v, geo, mask, rec, start, 3, num=0)
    assert st == 0, _err()
    ar.untouched()
    ar, st = view_bwd_call(n, True, 13, sc, v, geo, mask, rec, start, 3, num=0)
    assert st == 0, _err()
    out = ar.check()
    assert not out["v_viewmat"].any() and not out["v_projmat"].any() and _is_sentinel(ar, "v_rgb", out["v_rgb"])
    assert out["ws"].tobytes() == ar.before("ws").tobytes()
    for k, s in zip(SINKS, start):
        assert out[k].tobytes() == s.tobytes(), k
    if n == 257:
        for pose in (False, True):
            for name in ("quats_raw", "quats_n", "v_quats"):
                ar, st = view_bwd_call(n, pose, 13, sc, v, geo, mask, rec, start, 4, shift={name: 4})
                _refused(ar, st, name)
            ar, st = view_bwd_call(n, pose, 16, sc, v, geo, mask, rec, start, 4, shift={"rec": 4})
            _refused(ar, st, "rec")
        ar, st = view_bwd_call(n, True, 13, sc, v, geo, mask, rec, start, 4, shift={"ws": 4})
        _refused(ar, st, "workspace")


def sh_multi_call(n, k, deg, dirs, cots, v_coeffs, accumulate, seed, num=None):
    ar = Arena(DEV, seed)
    names_d, names_c = [], []
    for i, (d, g) in enumerate(zip(dirs, cots)):
        names_d.append(f"viewdirs_{i}")
        names_c.append(f"v_colors_{i}")
        _carve(ar, "in", 4, **{names_d[-1]: d, names_c[-1]: g})
    ar.carve("v_coeffs", v_coeffs, 4, "inout" if accumulate else "out")
    st = _lib().gg_sh_bwd_multi(n if num is None else num, k, deg, len(dirs), _host_ptrs(ar, names_d),
                                _host_ptrs(ar, names_c), ar.ptr("v_coeffs"), int(accumulate), _stream())
    _at(ar, 4, "v_coeffs", *names_d, *names_c)
    return ar, st


@pytest.mark.parametrize("deg", [0, 4])
@pytest.mark.parametrize("n", VIEW_N)
def test_sh_bwd_multi(n, deg):
    """two kept views, 25 stored bases, degrees 0 and 4: the sum against the restatement's colors_all gradient of both
    views under tests/test_view_chain_gpu.py's bound; under `accumulate` the header's statement, "the bits of adding
    view after view" to the buffer's value: preload plus that gradient under the same bound, the same bytes both times"""
    import view_chain_cases as vc
    from test_view_chain_gpu import MARGIN_X, _hold, _record, _ref_grads
    dirs, cots = [], []
    for which, seed in ((1, None), (2, 11)):
        sc, view, v, geo, mask = _chain(n, deg, True, which)
        rec = _record(VIEW, seed)[:n]
        open_ = np.stack([(mask >> ch) & 1 for ch in range(3)], -1).astype(bool)
        dirs.append(geo["viewdirs"])
        cots.append(np.where(open_, rec[:, 6:9], F32(0)).astype(F32))
    want = _ref_grads(VIEW, n, deg, True)["colors_all"] + _ref_grads(VIEW, n, deg, True, 2, 11)["colors_all"]
    nb = (deg + 1) ** 2
    blank = np.empty((n, 25, 3), F32)
    runs = []
    for seed in (1, 2):
        ar, st = sh_multi_call(n, 25, deg, dirs, cots, blank, False, seed)
        assert st == 0, _err()
        out = ar.check()
        _hold(f"memory contract gg_sh_bwd_multi[n={n} deg={deg}]", torch.from_numpy(out["v_coeffs"]), want,
              MARGIN_X * vc.ORACLE_WORST["colors_all_two_views"])
        assert not out["v_coeffs"][:, nb:].any() and (n == 1 or np.abs(out["v_coeffs"][:, :nb]).sum() > 0)
        runs.append(out)
    _same_bytes(runs[0], runs[1], ("v_coeffs",))
    pre = _preload((n, 25, 3), 13)
    pre[:, nb:] = 0.0
    acc = []
    for seed in (1, 2):
        ar, st = sh_multi_call(n, 25, deg, dirs, cots, pre, True, seed)
        assert st == 0, _err()
        acc.append(ar.check())
        _hold(f"memory contract gg_sh_bwd_multi accumulate[n={n} deg={deg}]", torch.from_numpy(acc[-1]["v_coeffs"]),
              want + torch.from_numpy(pre).double(), MARGIN_X * vc.ORACLE_WORST["colors_all_two_views"])
        assert not acc[-1]["v_coeffs"][:, nb:].any()
    _same_bytes(acc[0], acc[1], ("v_coeffs",))
    ar, st = sh_multi_call(n, 25, deg, dirs, cots, pre, True, 3, num=0)            # num_points == 0 does nothing
    assert st == 0, _err()
    ar.untouched()


# ------------------------------------------------------------------------------------------------
# the projection fallback: gg_project_fwd[_count], gg_project_bwd[_ex]
# ------------------------------------------------------------------------------------------------
PROJ_OUTS = ("xys", "depths", "radii", "conics", "num_tiles_hit", "cov3d")


def _proj_inputs(n):
    c, v = _view_case(n)
    scales = np.exp(c.log_scales[:n].astype(F64)).astype(F32)
    return c.means[:n], scales, c.quats[:n], v


def project_fwd_call(n, count, seed, shift=None, num=None):
    lib = _lib()
    means, scales, quats, v = _proj_inputs(n)
    ar = Arena(DEV, seed)
    _carve(ar, "in", 4, means=means, scales=scales, viewmat=np.asarray(v.viewmat, F32)[:3],
           projmat=np.asarray(v.full_proj, F32))
    ar.carve("quats", quats, 16, "in")
    _carve(ar, "out", 4, cov3d=np.empty((n, 6), F32), xys=np.empty((n, 2), F32), depths=np.empty(n, F32),
           radii=np.empty(n, I32), conics=np.empty((n, 3), F32), num_tiles_hit=np.empty(n, I32))
    if count:
        need = lib.gg_project_count_workspace(n)
        ar.carve("total", np.empty(1, I64), 8, "out")
        ar.carve("count_ws", need, 4, "ws")
    q = _ptrs(ar, shift)
    tb = v.tile_bounds
    args = (n if num is None else num, q("means"), q("scales"), 1.0, q("quats"), q("viewmat"), q("projmat"), v.fx, v.fy,
            v.cx, v.cy, v.h, v.w, int(tb[0]), int(tb[1]), float(v.clip), q("cov3d"), q("xys"), q("depths"), q("radii"),
            q("conics"), q("num_tiles_hit"))
    if count:
        st = lib.gg_project_fwd_count(*args, q("total"), q("count_ws"), need, _stream())
        _at(ar, 8, "total")
        _at(ar, 4, "count_ws")
    else:
        st = lib.gg_project_fwd(*args, _stream())
    _at(ar, 16, "quats")
    _at(ar, 4, "means", "scales", *PROJ_OUTS)
    return ar, st


@pytest.mark.parametrize("count", [False, True], ids=["gg_project_fwd", "gg_project_fwd_count"])
@pytest.mark.parametrize("n", VIEW_N)
def test_project_forward(oracle, n, count):
    """criterion: tests/test_gpu_parity.py test_project_fwd_bitexact — all six outputs the oracle's bits"""
    from test_gpu_parity import assert_bitexact
    means, scales, quats, v = _proj_inputs(n)
    ref = oracle.project_fwd(means, scales, 1.0, quats, np.asarray(v.viewmat, F32)[:3], np.asarray(v.full_proj, F32),
                             v.fx, v.fy, v.cx, v.cy, v.h, v.w, v.tile_bounds, clip_thresh=float(v.clip))
    assert n == 1 or ((ref[2] > 0).any() and (ref[2] == 0).any())
    runs = []
    for seed in (1, 2):
        ar, st = project_fwd_call(n, count, seed)
        assert st == 0, _err()
        out = ar.check()
        for k, r in zip(PROJ_OUTS, ref):
            assert_bitexact(out[k], r.reshape(out[k].shape), f"project_fwd.{k}")
        if count:
            assert int(out["total"][0]) == int(ref[4].sum(dtype=I64))
        runs.append(out)
    _same_bytes(runs[0], runs[1], PROJ_OUTS + (("total",) if count else ()))
    ar, st = project_fwd_call(n, count, 3, num=0)          # num_points == 0: nothing, but for the count, 0
    assert st == 0, _err()
    if count:
        out = ar.check()
        assert out["total"][0] == 0 and all(_is_sentinel(ar, k, out[k]) for k in PROJ_OUTS)
        assert out["count_ws"].tobytes() == ar.before("count_ws").tobytes()
    else:
        ar.untouched()
    if n == 257:
        ar, st = project_fwd_call(n, count, 4, shift={"quats": 4})
        _refused(ar, st, "quats")


PROJ_GRADS = ("v_mean3d", "v_scale", "v_quat")


def project_bwd_call(n, ex, fwd, cot, pre, seed, shift=None, num=None):
    """gg_project_bwd on dense cotangents; gg_project_bwd_ex with v_xy / v_conic as columns 0..1 / 2..4 of a 13-float
    record and v_mean3d added to (an inout region holding `pre`)"""
    lib = _lib()
    means, scales, quats, v = _proj_inputs(n)
    v_xy, v_depth, v_conic = cot
    ar = Arena(DEV, seed)
    _carve(ar, "in", 4, means=means, scales=scales, viewmat=np.asarray(v.viewmat, F32)[:3],
           projmat=np.asarray(v.full_proj, F32), radii=fwd[2], conics=fwd[3], v_depth=v_depth)
    ar.carve("quats", quats, 16, "in")
    if ex:
        rec = np.full((n, 13), np.nan, F32)
        rec[:, 0:2], rec[:, 2:5] = v_xy, v_conic
        ar.carve("rec", rec, 4, "in")
        ar.carve("v_mean3d", pre, 4, "inout")
    else:
        _carve(ar, "in", 4, v_xy=v_xy, v_conic=v_conic)
        ar.carve("v_mean3d", np.empty((n, 3), F32), 4, "out")
    ar.carve("v_scale", np.empty((n, 3), F32), 4, "out")
    ar.carve("v_quat", np.empty((n, 4), F32), 16, "out")
    q = _ptrs(ar, shift)
    head = (n if num is None else num, q("means"), q("scales"), 1.0, q("quats"), q("viewmat"), q("projmat"), v.fx, v.fy,
            v.cx, v.cy, v.h, v.w, q("radii"), q("conics"))
    if ex:
        st = lib.gg_project_bwd_ex(*head, q("rec"), 13, q("v_depth"), q("rec", 8), 13, q("v_mean3d"), 1, q("v_scale"),
                                   q("v_quat"), _stream())
    else:
        st = lib.gg_project_bwd(*head, q("v_xy"), q("v_depth"), q("v_conic"), q("v_mean3d"), q("v_scale"), q("v_quat"),
                                _stream())
    _at(ar, 16, "quats", "v_quat")
    _at(ar, 4, "means", "v_mean3d", "v_scale")
    return ar, st


@pytest.mark.parametrize("ex", [False, True], ids=["gg_project_bwd", "gg_project_bwd_ex"])
@pytest.mark.parametrize("n", VIEW_N)
def test_project_backward(oracle, n, ex):
    """criterion: tests/test_gpu_parity.py test_project_bwd — assert_close(rtol 1e-6, atol_frac 1e-7) against the oracle;
    one Gaussian per lane and no reduction, so the same bytes on every call"""
    from test_gpu_parity import assert_close
    means, scales, quats, v = _proj_inputs(n)
    vm, pm = np.asarray(v.viewmat, F32)[:3], np.asarray(v.full_proj, F32)
    fwd = oracle.project_fwd(means, scales, 1.0, quats, vm, pm, v.fx, v.fy, v.cx, v.cy, v.h, v.w, v.tile_bounds,
                             clip_thresh=float(v.clip))
    rng = np.random.default_rng(2 + n)
    cot = (rng.standard_normal((n, 2)).astype(F32), rng.standard_normal(n).astype(F32),
           rng.standard_normal((n, 3)).astype(F32))
    ref = oracle.project_bwd(means, scales, 1.0, quats, vm, pm, v.fx, v.fy, v.cx, v.cy, v.h, v.w, fwd[2], fwd[3], *cot)
    pre = _preload((n, 3), 17)
    runs = []
    for seed in (1, 2):
        ar, st = project_bwd_call(n, ex, fwd, cot, pre, seed)
        assert st == 0, _err()
        out = ar.check()
        for k, r in zip(PROJ_GRADS, ref):
            r = r + pre.astype(F64) if (ex and k == "v_mean3d") else r
            assert_close(out[k], r, f"memory_contract.project_bwd.{k}", rtol=1e-6, atol_frac=1e-7)
        runs.append(out)
    _same_bytes(runs[0], runs[1], PROJ_GRADS)
    ar, st = project_bwd_call(n, ex, fwd, cot, pre, 3, num=0)           # num_points == 0 does nothing
    assert st == 0, _err()
    ar.untouched()
    if n == 257:
        for name in ("quats", "v_quat"):
            ar, st = project_bwd_call(n, ex, fwd, cot, pre, 4, shift={name: 4})
            _refused(ar, st, name)
