"""The per-Gaussian chain of one view on the MI355X (csrc/project.hip) against the float64 restatement
(tests/view_chain_ref.py), Gaussian by Gaussian, on the constructed cases of tests/view_chain_cases.py: gg_view_fwd and
gg_shade_tail_fwd[_ex] on everything they write; gg_view_bwd / gg_view_bwd_pose through the C ABI with both record
strides, preloaded sinks and every truncation; the three-kernel fallback bit for bit; ops.ViewGeometry through both
branches of its backward, and the SH expansion of two kept views (gg_sh_bwd_multi) at every degree.

Measure and bounds (tests/test_view_chain_cases_host.py): per Gaussian and parameter row |got - ref| / max|ref row|,
at most twice what the fp32 oracle chain reaches on the same cases (view_chain_cases.ORACLE_WORST, FWD_WORST); rows
whose reference is exactly zero are exactly zero; discrete outputs are equal.  No Gaussian is left out."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import view_chain_cases as vc
import view_chain_ref as ref
from gaussiangrasper_amd import _lib, ops as P
from gaussiangrasper_amd._call import ptr as _ptr, stream as _stream, workspace as _workspace
from gaussiangrasper_amd.constants import num_sh_bases
from test_forward_chain_shapes import _view_fwd
from test_gpu_parity import ERROR_STATS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [f"{h}x{w}" for h, w in vc.SIZES]
SIZES_N = (vc.NUM,) + vc.TRUNCATIONS
MARGIN_X = 2.0             # the kernels' allowance over the oracle's measured error: ocml expf, operation order


def _off(t, floats):
    return C.c_void_p(t.data_ptr() + 4 * floats)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs(name, n, deg=4, full=True, which=1):
    """the case's leaves on the GPU (the first n Gaussians) as the scene / view objects _view_fwd takes"""
    c = vc.cases()[name]
    v = c.view if which == 1 else vc.make_view(c.view.h, c.view.w, which)
    col = vc.colors_for(c, deg, full)
    sc = types.SimpleNamespace(means=_dev(c.means[:n]), scales=_dev(c.log_scales[:n]), quats=_dev(c.quats[:n]),
                               opacities=_dev(c.opacities[:n]), colors_all=_dev(col[:n]))
    vm4 = torch.eye(4)
    vm4[:3] = torch.from_numpy(v.viewmat)
    view = types.SimpleNamespace(viewmat=vm4.to(DEV), projmat=_dev(v.full_proj), cam_pos=_dev(v.cam_pos), fx=v.fx, fy=v.fy,
                                 cx=v.cx, cy=v.cy, height=v.h, width=v.w, tile_bounds=v.tile_bounds)
    return sc, view, v


@functools.lru_cache(maxsize=None)
def _ref_forward(name, n, deg=4, full=True):
    c = vc.cases()[name]
    leaves = ref.case_leaves(c, n)
    return ref.forward(*leaves[:4], ref.f64(vc.colors_for(c, deg, full)[:n]), c.view, deg)


@functools.lru_cache(maxsize=None)
def _ref_grads(name, n, deg=4, full=True, which=1, seed=None):
    c = vc.cases()[name]
    v = c.view if which == 1 else vc.make_view(c.view.h, c.view.w, which)
    return ref.grads(c, _record(name, seed), n, deg, vc.colors_for(c, deg, full)[:n], view=v)


def _record(name, seed=None):
    """the case's own record, or another draw of cotangents (the second view's)"""
    return vc.cases()[name].record if seed is None else vc.second_record(seed)


def _stat(what, err, bound):
    err = ref.f64(err).numpy()
    ERROR_STATS.append({"what": what, "n": int(err.size), "max_abs_over_scale": float(err.max()),
                        "rel_p999": float(np.quantile(err, 0.999)), "rel_max": float(err.max()), "rtol": 0.0,
                        "atol_frac": bound})


def _hold(what, got, want, bound, floor=None):
    """the row measure, recorded and asserted"""
    err = ref.row_errors(got, want, floor)
    _stat(what, err, bound)
    worst = int(err.argmax())
    print(f"{what}: worst row error {float(err.max()):.3e} (Gaussian {worst}), allowed {bound:.1e}")
    assert float(err.max()) <= bound, (what, float(err.max()), worst, bound)


def _tail_fwd(lib, sc, geo, n, k, deg, variant):
    tail = torch.full((n, 7), float("nan"), dtype=torch.float32, device=DEV)
    mask = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
    args = (n, k, deg, _ptr(geo["viewdirs"]), _ptr(sc.colors_all), _ptr(geo["depths"]), _ptr(geo["normals"]), _ptr(tail),
            _ptr(mask))
    if variant is None:
        _lib.check(lib.gg_shade_tail_fwd(*args, _stream(DEV)), "gg_shade_tail_fwd")
    else:
        _lib.check(lib.gg_shade_tail_fwd_ex(*args, variant, _stream(DEV)), "gg_shade_tail_fwd_ex")
    torch.cuda.synchronize()
    return tail, mask


# ----------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES_N)
@pytest.mark.parametrize("name", CASES)
def test_view_forward_against_the_restatement(name, n):
    """gg_view_fwd on poisoned outputs: discrete outputs equal, float outputs within twice the oracle's error, the three
    partial results of every workgroup (a workgroup without a visible Gaussian among them at N = 257), the packed
    records equal to blend_prep's packing of the same outputs"""
    lib = _lib.load()
    sc, view, v = _inputs(name, n)
    want = _ref_forward(name, n)
    geo = _view_fwd(sc, view, v.h, v.w)
    for k in ("radii", "num_tiles_hit", "axis"):
        assert torch.equal(geo[k].cpu().to(torch.int64), want[k].to(torch.int64)), k
    assert int(geo["total"]) == int(want["num_tiles_hit"].sum())
    bound = MARGIN_X * vc.FWD_WORST
    for k in ("scales", "quats_n", "opac", "viewdirs", "normals", "xys", "depths"):
        assert not torch.isnan(geo[k]).any(), k
        _hold(f"view chain fwd {k}[{name} n={n}]", geo[k].cpu(), want[k].detach(), bound)
    _hold(f"view chain fwd conics[{name} n={n}]", geo["conics"].cpu(), want["conics_written"], bound)
    # the workgroups' partial results
    blocks = (n + 255) // 256
    parts = geo["parts"].cpu().numpy().view(np.uint32).reshape(3, blocks)
    vis, nth = want["vis"].numpy(), want["num_tiles_hit"].numpy()
    bits = geo["depths"].cpu().numpy().view(np.uint32)
    empty = 0
    for b in range(blocks):
        sl = slice(256 * b, min(256 * (b + 1), n))
        assert parts[0, b] == nth[sl].sum(), b
        if vis[sl].any():
            assert parts[1, b] == bits[sl][vis[sl]].min() and parts[2, b] == bits[sl][vis[sl]].max(), b
        else:
            empty += 1
            assert parts[1, b] == 0xFFFFFFFF and parts[2, b] == 0, b
    assert empty == (1 if n == 257 else 0)
    # the packed records: what blend_prep_kernel packs from the same arrays (a blend forward over empty tile lists)
    tiles = v.tile_bounds[0] * v.tile_bounds[1]
    ws = _workspace(lib.gg_blend_workspace(n), DEV)
    ws.zero_()
    col, bg = torch.zeros(n, 1, device=DEV), torch.zeros(1, device=DEV)
    img, ft = torch.empty(v.h, v.w, 1, device=DEV), torch.empty(v.h, v.w, device=DEV)
    fi = torch.empty(v.h, v.w, dtype=torch.int32, device=DEV)
    ids, bins = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(tiles, 2, dtype=torch.int32, device=DEV)
    _lib.check(lib.gg_blend_fwd(1, n, v.h, v.w, _ptr(ids), _ptr(bins), _ptr(geo["xys"]), _ptr(geo["conics"]), _ptr(col),
                                _ptr(geo["opac"]), _ptr(bg), _ptr(img), _ptr(ft), _ptr(fi), _ptr(ws), ws.numel(),
                                _stream(DEV)), "gg_blend_fwd")
    torch.cuda.synchronize()
    assert torch.equal(geo["records"][:32 * n], ws[:32 * n]), "packed records"


@pytest.mark.parametrize("deg", range(5))
@pytest.mark.parametrize("name", CASES)
def test_shade_tail_forward_against_the_restatement(name, deg):
    """gg_shade_tail_fwd and gg_shade_tail_fwd_ex(one_wave = 0 / 1), 25 stored bases and num_sh_bases(deg): the clamp
    mask equal (all eight values, both bounds from both sides), colours within twice the oracle's error of the clamp's
    range, depth and normal columns the forward's own values"""
    lib = _lib.load()
    n = vc.NUM
    for full in (True, False):
        sc, view, v = _inputs(name, n, deg, full)
        want = _ref_forward(name, n, deg, full)
        geo = _view_fwd(sc, view, v.h, v.w)
        k = sc.colors_all.shape[1]
        assert k == (25 if full else num_sh_bases(deg))
        for variant in (None, 0, 1):
            tail, mask = _tail_fwd(lib, sc, geo, n, k, deg, variant)
            assert torch.equal(mask.cpu(), want["mask"]), (full, variant)
            assert np.bincount(mask.cpu().numpy(), minlength=8).min() >= 8
            err = (tail[:, :3].cpu().double() - want["tail"][:, :3].detach()).abs().max(-1).values
            _stat(f"view chain tail rgb[{name} deg={deg}]", err, MARGIN_X * vc.FWD_WORST)
            assert float(err.max()) <= MARGIN_X * vc.FWD_WORST, (full, variant, float(err.max()))
            assert torch.equal(tail[:, 3], geo["depths"]) and torch.equal(tail[:, 4:7], geo["normals"])
    if deg == 4:
        for m in vc.TRUNCATIONS:
            sc, view, v = _inputs(name, m)
            geo = _view_fwd(sc, view, v.h, v.w)
            for variant in (None, 1):
                tail, mask = _tail_fwd(lib, sc, geo, m, 25, 4, variant)
                assert torch.equal(mask.cpu(), _ref_forward(name, m)["mask"]), (m, variant)
                assert not torch.isnan(tail).any()


# ----------------------------------------------------------------------------------------------------------------------
# backward, C ABI
# ----------------------------------------------------------------------------------------------------------------------
def _chain_forward(lib, name, n, deg=4, full=True, which=1):
    sc, view, v = _inputs(name, n, deg, full, which)
    geo = _view_fwd(sc, view, v.h, v.w)
    _, mask = _tail_fwd(lib, sc, geo, n, sc.colors_all.shape[1], deg, None)
    return sc, view, v, geo, mask


def _starts(n, zero):
    g = torch.Generator(device="cpu").manual_seed(99)
    shapes = (3, 3, 4, 1)
    return [torch.zeros(n, k, device=DEV) if zero else torch.randn(n, k, generator=g).to(DEV) for k in shapes]


def _view_bwd(lib, pose, n, sc, view, v, geo, mask, rec, stride, sinks):
    """gg_view_bwd / gg_view_bwd_pose adding into `sinks` -> v_rgb[, v_viewmat, v_projmat]"""
    v_rgb = torch.full((n, 3), float("nan"), device=DEV)
    vm, pm = view.viewmat[:3, :].contiguous(), view.projmat.contiguous()
    args = [n, _ptr(rec), stride, _ptr(mask), _ptr(sc.means), _ptr(geo["scales"]), 1.0, _ptr(sc.quats), _ptr(geo["quats_n"]),
            _ptr(geo["opac"]), _ptr(geo["axis"]), _ptr(vm), _ptr(pm), v.fx, v.fy, v.h, v.w, _ptr(geo["radii"]),
            _ptr(geo["conics"]), _ptr(v_rgb)] + [_ptr(s) for s in sinks]
    if not pose:
        _lib.check(lib.gg_view_bwd(*args, _stream(DEV)), "gg_view_bwd")
        torch.cuda.synchronize()
        return v_rgb, None, None
    out_v, out_p = torch.full((12,), float("nan"), device=DEV), torch.full((16,), float("nan"), device=DEV)
    ws = torch.empty(max(lib.gg_pose_grad_workspace(n), 256), dtype=torch.uint8, device=DEV)
    _lib.check(lib.gg_view_bwd_pose(*args, _ptr(out_v), _ptr(out_p), _ptr(ws), ws.numel(), _stream(DEV)), "gg_view_bwd_pose")
    torch.cuda.synchronize()
    return v_rgb, out_v, out_p


def _three_kernels(lib, n, sc, view, v, geo, mask, rec, stride, sinks):
    """gg_shade_tail_bwd_split, gg_project_bwd_ex, gg_activate_bwd_ex over the record in place, adding into `sinks`"""
    v_rgb = torch.full((n, 3), float("nan"), device=DEV)
    v_depths, v_normals = torch.empty(n, device=DEV), torch.empty(n, 3, device=DEV)
    v_scale, v_quat = torch.empty(n, 3, device=DEV), torch.empty(n, 4, device=DEV)
    vm, pm = view.viewmat[:3, :].contiguous(), view.projmat.contiguous()
    _lib.check(lib.gg_shade_tail_bwd_split(n, _off(rec, 6), stride, _ptr(mask), _ptr(v_rgb), _ptr(v_depths), _ptr(v_normals),
                                           _stream(DEV)), "gg_shade_tail_bwd_split")
    _lib.check(lib.gg_project_bwd_ex(n, _ptr(sc.means), _ptr(geo["scales"]), 1.0, _ptr(geo["quats_n"]), _ptr(vm), _ptr(pm),
                                     v.fx, v.fy, v.cx, v.cy, v.h, v.w, _ptr(geo["radii"]), _ptr(geo["conics"]), _ptr(rec),
                                     stride, _ptr(v_depths), _off(rec, 2), stride, _ptr(sinks[0]), 1, _ptr(v_scale),
                                     _ptr(v_quat), _stream(DEV)), "gg_project_bwd_ex")
    _lib.check(lib.gg_activate_bwd_ex(n, _ptr(sc.quats), _ptr(geo["scales"]), _ptr(geo["opac"]), _ptr(geo["axis"]),
                                      _ptr(v_scale), _ptr(v_quat), _off(rec, 5), stride, _ptr(v_normals), _ptr(sinks[1]),
                                      _ptr(sinks[2]), _ptr(sinks[3]), 1, _stream(DEV)), "gg_activate_bwd_ex")
    torch.cuda.synchronize()
    return v_rgb


@pytest.mark.parametrize("n", SIZES_N)
@pytest.mark.parametrize("name", CASES)
def test_view_backward_against_the_restatement(name, n):
    """gg_view_bwd and gg_view_bwd_pose, records of 13 and of 16 floats (columns 13 ... 15 NaN): from zeroed sinks the
    four parameter gradients against autograd through the restatement, per Gaussian; from sinks holding known values
    the result is fl(start + that gradient), bit for bit, in every build; v_rgb is the masked record columns; the pose
    sums within 1e-5 of their absolute sums; the three-kernel fallback equals gg_view_bwd bit for bit."""
    lib = _lib.load()
    c = vc.cases()[name]
    sc, view, v, geo, mask = _chain_forward(lib, name, n)
    want = _ref_grads(name, n)
    rec16 = _dev(c.record[:n])
    recs = {16: rec16, 13: rec16[:, :13].contiguous()}
    assert torch.isnan(rec16[:, 13:]).all()
    open_ = torch.stack([(mask >> ch) & 1 for ch in range(3)], -1).bool()
    rgb_want = torch.where(open_, rec16[:, 6:9], torch.zeros((), device=DEV))
    vis = want["out"]["vis"]
    # the gradient itself: zeroed sinks, one build
    base = _starts(n, zero=True)
    v_rgb, _, _ = _view_bwd(lib, False, n, sc, view, v, geo, mask, recs[16], 16, base)
    assert torch.equal(v_rgb, rgb_want)
    for p, got in zip(ref.PARAMS, base):
        floor = ref.opacity_floor(c.record, n) if p == "opacities" else None
        _hold(f"view chain gg_view_bwd {p}[{name} n={n}]", got.cpu(), want[p], MARGIN_X * vc.ORACLE_WORST[p], floor)
        assert not got.cpu().reshape(n, -1)[(want[p].reshape(n, -1).abs().max(-1).values == 0)].any(), p
    assert not base[0].cpu()[~vis].any() and not base[1].cpu()[~vis].any()      # invisible: no projection part ...
    live = torch.from_numpy(c.record[:n, :13].any(-1))
    if bool((~vis & live).any()):                                                # ... but the activations' part
        assert base[2].cpu()[~vis & live].abs().sum(-1).min() > 0 and base[3].cpu()[~vis & live].abs().min() > 0
    # every build and stride from known non-zero values: start + gradient
    start = _starts(n, zero=False)
    expect = [s + g for s, g in zip(start, base)]
    for stride in (13, 16):
        for pose in (False, True):
            sinks = [s.clone() for s in start]
            v_rgb, got_v, got_p = _view_bwd(lib, pose, n, sc, view, v, geo, mask, recs[stride], stride, sinks)
            assert torch.equal(v_rgb, rgb_want), (stride, pose)
            for p, got, exp in zip(ref.PARAMS, sinks, expect):
                assert torch.equal(got, exp), (p, stride, pose)
            if pose:
                for got, key in ((got_v.reshape(3, 4), "viewmat"), (got_p.reshape(4, 4), "projmat")):
                    err = (got.cpu().double() - want["v_" + key]).abs()
                    bound = 1e-5 * want["abs_" + key] + 1e-30
                    assert (err <= bound).all(), (key, stride, err.max().item(), (err / bound).max().item())
                assert (got_p.reshape(4, 4)[2] == 0).all()
        sinks = [s.clone() for s in start]
        v_rgb = _three_kernels(lib, n, sc, view, v, geo, mask, recs[stride], stride, sinks)
        assert torch.equal(v_rgb, rgb_want), stride
        for p, got, exp in zip(ref.PARAMS, sinks, expect):
            assert torch.equal(got, exp), ("three kernels", p, stride)


# ----------------------------------------------------------------------------------------------------------------------
# backward, operator level
# ----------------------------------------------------------------------------------------------------------------------
def _counted(lib, names, monkeypatch):
    calls = []
    for k in names:
        f = getattr(lib, k)
        monkeypatch.setattr(lib, k, (lambda f_, k_: (lambda *a: (calls.append((k_, a)), f_(*a))[1]))(f, k), raising=False)
    return calls


def _leaves(sc):
    return [t.detach().clone().requires_grad_(True) for t in (sc.means, sc.scales, sc.quats, sc.opacities, sc.colors_all)]


def _apply(leaves, view, v, deg):
    return P.ViewGeometry.apply(*leaves, view.cam_pos, view.viewmat[:3, :], view.projmat, v.fx, v.fy, v.cx, v.cy, v.h, v.w,
                                v.tile_bounds, deg)


OPERATOR_CASES = [(name, 4, True) for name in CASES] + [("17x33", d, d % 2 == 0) for d in range(4)]


@pytest.mark.parametrize("name,deg,full", OPERATOR_CASES)
def test_view_geometry_backward_against_the_restatement(name, deg, full, monkeypatch):
    """ops.ViewGeometry through both branches of its backward.  With sinks and the cotangents as the columns of one
    record: one gg_view_bwd call per view; two views are kept and their SH gradient expanded once (gg_sh_bwd_multi, two
    views), compared with the restatement's colors_all gradient summed over the views; the entries past
    num_sh_bases(deg) are exactly zero.  Without sinks, dense cotangents: the three operators' backwards."""
    lib = _lib.load()
    n = vc.NUM
    c = vc.cases()[name]
    calls = _counted(lib, ("gg_view_bwd", "gg_view_bwd_pose", "gg_sh_bwd_multi", "gg_shade_tail_bwd", "gg_project_bwd_ex",
                           "gg_activate_bwd_ex"), monkeypatch)
    nb = num_sh_bases(deg)
    want1 = _ref_grads(name, n, deg, full)
    want2 = _ref_grads(name, n, deg, full, 2, 11)
    sc, view, v = _inputs(name, n, deg, full)
    _, view2, v2 = _inputs(name, n, deg, full, 2)
    recs = [_dev(c.record), _dev(_record(name, 11))]
    # ---- sinks, record views
    leaves = _leaves(sc)
    bufs = [torch.zeros_like(t) for t in leaves]
    more = {"views": True}
    try:
        for t, b in zip(leaves, bufs):
            P.register_grad_sink(t, b, defer=(lambda: more["views"]) if t is leaves[4] else None)
        snapshot = None
        for k, (vw, vv, rec) in enumerate(((view, v, recs[0]), (view2, v2, recs[1]))):
            more["views"] = k == 0
            P.clear_bin_cache()
            xys, depths, radii, conics, nth, opac, tail, normals, packed = _apply(leaves, vw, vv, deg)
            torch.autograd.backward([xys, conics, opac, tail], [rec[:, 0:2], rec[:, 2:5], rec[:, 5:6], rec[:, 6:13]])
            torch.cuda.synchronize()
            if k == 0:
                snapshot = [b.clone() for b in bufs]
        names = [k for k, _ in calls]
        assert names == ["gg_view_bwd", "gg_view_bwd", "gg_sh_bwd_multi"], names
        assert calls[2][1][3] == 2 and calls[2][1][1] == leaves[4].shape[1] and calls[2][1][2] == deg
        assert all(t.grad is None for t in leaves)
    finally:
        P.clear_grad_sinks()
        P.clear_bin_cache()
    for p, got in zip(ref.PARAMS, snapshot):           # the first view alone: the case's own view
        floor = ref.opacity_floor(c.record) if p == "opacities" else None
        _hold(f"view chain ViewGeometry sinks {p}[{name} deg={deg}]", got.cpu(), want1[p], MARGIN_X * vc.ORACLE_WORST[p], floor)
    assert not snapshot[4].any()                        # kept, not yet expanded
    _hold(f"view chain gg_sh_bwd_multi colors_all[{name} deg={deg}]", bufs[4].cpu(), want1["colors_all"] + want2["colors_all"],
          MARGIN_X * vc.ORACLE_WORST["colors_all_two_views"])
    assert not bufs[4][:, nb:].any() and bufs[4][:, :nb].abs().sum() > 0
    # ---- no sinks, dense cotangents
    calls.clear()
    leaves = _leaves(sc)
    P.clear_bin_cache()
    xys, depths, radii, conics, nth, opac, tail, normals, packed = _apply(leaves, view, v, deg)
    rec = recs[0]
    torch.autograd.backward([xys, conics, opac, tail], [rec[:, 0:2].contiguous(), rec[:, 2:5].contiguous(),
                                                        rec[:, 5:6].contiguous(), rec[:, 6:13].contiguous()])
    torch.cuda.synchronize()
    P.clear_bin_cache()
    names = [k for k, _ in calls]
    assert names == ["gg_shade_tail_bwd", "gg_project_bwd_ex", "gg_activate_bwd_ex"], names
    for p, t in zip(ref.PARAMS + ("colors_all",), leaves):
        floor = ref.opacity_floor(c.record) if p == "opacities" else None
        _hold(f"view chain ViewGeometry dense {p}[{name} deg={deg}]", t.grad.cpu(), want1[p], MARGIN_X * vc.ORACLE_WORST[p], floor)
    assert not leaves[4].grad[:, nb:].any()
