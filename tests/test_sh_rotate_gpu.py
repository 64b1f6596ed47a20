"""GPU checks of the SH rotation of moved Gaussians (gg_sh_rotate, gaussiangrasper_amd.sh_rotation, edit's sh= /
rotate_sh=): the kernel bit for bit against the fp32 restatement of its contract (tests/sh_rotate_ref.py) with every
byte around the selected rows watched, the colour a Gaussian shows through the library's own SH evaluation before and
after a turn, the edit path with a partial selection, the transforms that must leave the coefficients alone, the
rendered image of a scene moved together with its cameras, edit_model and the checkpoint tool."""
import os
import re

import numpy as np
import pytest
import torch

from sh_rotate_ref import sh_rotate_ref

gpu = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.678
ROTVEC, SHIFT = (0.9, -1.3, 0.6), (0.11, -0.07, 0.05)


def kernel_rows():
    """rows per workgroup of sh_rotate_kernel, read from the source; the kernel has no grid cap and no loop over
    tiles (one workgroup per SR_ROWS rows), so no size gives a workgroup a second trip"""
    src = open(os.path.join(ROOT, "gaussiangrasper_amd", "csrc", "sh_rotate.hip")).read()
    rows = int(re.search(r"^#define\s+SR_ROWS\s+(\d+)\b", src, flags=re.M).group(1))
    assert "(long long)blockIdx.x * SR_ROWS" in src and "+ SR_ROWS - 1) / SR_ROWS" in src
    assert "gridDim" not in src
    return rows


def box_planes(lo, hi):
    rows = []
    for a in range(3):
        n = np.zeros(3)
        n[a] = 1.0
        rows.append([*n, -float(hi[a])])
        rows.append([*(-n), float(lo[a])])
    return np.array(rows)


def rigid(rotvec=ROTVEC, shift=SHIFT):
    from gaussiangrasper_amd.edit import rotvec_to_matrix
    rt = np.zeros((3, 4))
    rt[:, :3] = rotvec_to_matrix(rotvec)
    rt[:, 3] = shift
    return rt.astype(np.float32)


def packed_for(R, k):
    from gaussiangrasper_amd import sh_rotation
    return sh_rotation.pack_bands(sh_rotation.rotation_bands(np.asarray(R, np.float64), (1, 4, 9, 16, 25).index(k)), k)


def assert_same_bits(got, want, what=""):
    """every value that is not a NaN equal as int32 bits (infinities included), NaN positions equal"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    ng, nw = np.isnan(got), np.isnan(want)
    assert np.array_equal(ng, nw), f"{what}: NaN positions differ"
    bad = (got.view(np.int32) != want.view(np.int32)) & ~ng
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ, first at flat index {int(np.flatnonzero(bad)[0])}"


def masks_for(n, rows, rng):
    idx = np.arange(n)
    out = {"null": None, "zeros": np.zeros(n, np.uint8), "ones": np.ones(n, np.uint8)}
    last = np.zeros(n, np.uint8)
    last[-1] = 1
    out["last"] = last
    out["alternating"] = (idx % 2).astype(np.uint8)
    out["one_per_64"] = (idx % 64 == min(5, n - 1)).astype(np.uint8)
    runs = np.zeros(n, np.uint8)
    for b in range(64, n, 64):              # every wave boundary, the workgroup boundaries (multiples of rows) among them
        runs[max(b - 3, 0):b + 3] = 1
    assert rows % 64 == 0
    out["boundary_runs"] = runs
    out["bytes_1_2_255"] = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=n)
    return out


# ------------------------------------------------------------------------------------------------
# the kernel against its contract
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [1, 4, 9, 16, 25])
def test_bit_equal_to_the_restatement_and_nothing_else_written(k):
    from gaussiangrasper_amd import sh_rotation
    rows = kernel_rows()
    rng = np.random.default_rng(100 + k)
    R = rigid()[:, :3]
    packed = packed_for(R, k)
    for n in (1, 63, 64, 65, 257, 1025):
        c = rng.normal(size=(n, k, 3)).astype(np.float32)
        if k >= 9 and n >= 63:                   # one row with an inf and a NaN in band 2
            c[n // 2, 4, 0] = np.inf
            c[n // 2, 6, 1] = np.nan
        for name, m in masks_for(n, rows, rng).items():
            # the coefficients sit at an odd float offset of a sentinel-filled buffer: 4-byte, not 16-byte aligned
            buf = torch.full((3 + c.size + 301,), SENTINEL, dtype=torch.float32)
            buf[3:3 + c.size] = torch.from_numpy(c.reshape(-1))
            want = buf.numpy().copy()
            want[3:3 + c.size] = sh_rotate_ref(c, packed, m).reshape(-1)
            d_buf = buf.to(DEV)
            assert d_buf.data_ptr() % 16 == 0
            view = d_buf[3:3 + c.size].view(n, k, 3)
            assert view.data_ptr() % 16 == 12 and view.is_contiguous()
            d_m = None if m is None else torch.from_numpy(m).to(DEV)
            out = sh_rotation.rotate_coefficients(view, R, d_m)
            assert out is view
            got = d_buf.cpu().numpy()
            assert_same_bits(got, want, f"K={k} N={n} mask={name}")
            if k >= 9 and n >= 63 and name in ("null", "ones"):
                r = got[3:3 + c.size].reshape(n, k, 3)[n // 2]
                assert np.isnan(r[4:9, 1]).all() and not np.isfinite(r[4:9, 0]).any()
                assert np.isfinite(r[:4]).all() and np.isfinite(r[9:]).all() and np.isfinite(r[4:9, 2]).all()


@gpu
def test_bit_equal_on_many_workgroups():
    """100 003 rows (782 workgroups), a random tenth selected, and the same rows through mask=None"""
    from gaussiangrasper_amd import sh_rotation
    rng = np.random.default_rng(7)
    n, k = 100_003, 25
    R = rigid((0.2, 2.9, -0.4))[:, :3]
    c = rng.normal(size=(n, k, 3)).astype(np.float32)
    m = (rng.random(n) < 0.1).astype(np.uint8)
    packed = packed_for(R, k)
    for mask in (m, None):
        d_c = torch.from_numpy(c).to(DEV)
        sh_rotation.rotate_coefficients(d_c, R, None if mask is None else torch.from_numpy(mask).to(DEV))
        assert_same_bits(d_c.cpu().numpy(), sh_rotate_ref(c, packed, mask))


@gpu
def test_colour_of_a_gaussian_is_invariant():
    """ops.SphericalHarmonics of (R d, rotated coefficients) against (d, coefficients): within 2e-7 sum_k |c_k|"""
    from gaussiangrasper_amd import ops, sh_rotation
    rng = np.random.default_rng(11)
    R = rigid()[:, :3].astype(np.float64)
    d = rng.normal(size=(2000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d0 = torch.from_numpy(d.astype(np.float32)).to(DEV)
    d1 = torch.from_numpy((d @ R.T).astype(np.float32)).to(DEV)
    for deg in (1, 2, 3, 4):
        c = torch.from_numpy(rng.normal(size=(2000, (deg + 1) ** 2, 3)).astype(np.float32)).to(DEV)
        before = ops.SphericalHarmonics.apply(deg, d0, c).double()
        turned = sh_rotation.rotate_coefficients(c.clone(), R)
        after = ops.SphericalHarmonics.apply(deg, d1, turned).double()
        total = c.double().abs().sum(dim=1)
        worst = float(((after - before).abs() / total).max())
        print(f"colour invariance, degree {deg}: worst |diff| / sum|c| = {worst:.3g} (bound 2e-7)")
        assert bool(((after - before).abs() <= 2e-7 * total).all())


# ------------------------------------------------------------------------------------------------
# through the edit path
# ------------------------------------------------------------------------------------------------
@gpu
def test_edit_path_with_a_partial_selection():
    from gaussiangrasper_amd.edit import select_and_move
    from gaussiangrasper_amd.scene import make_scene
    sc = make_scene(4096, feature_dim=8)
    planes = box_planes([-2, -2, -2], [0, 2, 2])            # x <= 0: about half
    rt = rigid()
    m0, q0 = sc.means.to(DEV), sc.quats.to(DEV)
    mask0, count0 = select_and_move(m0, q0, planes, rt)
    m1, q1, sh = sc.means.to(DEV), sc.quats.to(DEV), sc.colors_all.to(DEV)
    mask, count = select_and_move(m1, q1, planes, rt, sh=sh)
    sel = mask.cpu().numpy()
    assert 1000 < int(count.item()) == int(sel.sum()) < 3096
    assert torch.equal(mask, mask0) and torch.equal(count, count0)
    assert torch.equal(m1.view(torch.int32), m0.view(torch.int32))
    assert torch.equal(q1.view(torch.int32), q0.view(torch.int32))
    c = sc.colors_all.numpy()
    want = sh_rotate_ref(c, packed_for(rt[:, :3], 25), sel)
    got = sh.cpu().numpy()
    assert_same_bits(got, want)
    assert np.array_equal(got[sel == 0].view(np.int32), c[sel == 0].view(np.int32))
    assert not np.array_equal(got[sel != 0], c[sel != 0])
    with pytest.raises(ValueError, match="transform"):
        select_and_move(m1, q1, planes, None, sh=sh)
    with pytest.raises(ValueError, match="rows"):
        select_and_move(m1, q1, planes, rt, sh=sh[:100])
    with pytest.raises(ValueError, match="SH coefficients"):
        select_and_move(m1, q1, planes, rt, sh=sh.double())
    bad = rt.copy()
    bad[:, :3] *= 1.01
    before = m1.clone()
    with pytest.raises(ValueError, match="orthonormal"):
        select_and_move(m1, q1, planes, bad, sh=sh)
    assert torch.equal(m1, before)                           # refused before anything moved


@gpu
def test_identity_and_translation_leave_the_coefficients_alone():
    from gaussiangrasper_amd.edit import select_and_move
    from gaussiangrasper_amd.scene import make_scene
    sc = make_scene(4096, feature_dim=8)
    planes = box_planes([-2, -2, -2], [2, 2, 2])
    for rt in (np.eye(3, 4, dtype=np.float32), rigid((0.0, 0.0, 0.0), (0.3, -0.2, 0.1))):
        m, q, sh = sc.means.to(DEV), sc.quats.to(DEV), sc.colors_all.to(DEV)
        _, count = select_and_move(m, q, planes, rt, sh=sh)
        assert int(count.item()) == 4096
        assert torch.equal(sh.cpu().view(torch.int32), sc.colors_all.view(torch.int32))


def fixture_a(deg):
    from gaussiangrasper_amd.scene import make_scene
    sc = make_scene(400, 8, deg)
    sc.scales += float(np.log(8.0))
    sc.colors_all[:, 1:, :] *= 6.0
    return sc


def moved_view(view, rt):
    """the camera of `view` moved by [R | t]: view_from_c2w(T @ c2w)"""
    from gaussiangrasper_amd.camera import view_from_c2w
    c2w = torch.eye(4)
    c2w[:3, :3] = view.viewmat[:3, :3].T @ torch.diag(torch.tensor([1.0, -1.0, -1.0]))
    c2w[:3, 3] = view.cam_pos
    T = torch.eye(4)
    T[:3, :] = torch.from_numpy(rt).reshape(3, 4)
    return view_from_c2w(T @ c2w, view.fx, view.fy, view.cx, view.cy, view.height, view.width)


@gpu
@pytest.mark.parametrize("deg", [3, 4])
def test_rendered_image_is_invariant_when_scene_and_cameras_move_together(deg):
    """Fixture A.  Set aside: at most 0.5 % of the pixels, those that differ by more than 1e-4 (tile or alpha
    decisions flipped by the fp32 rounding of the moved projection); every other pixel within 2e-5.  The same move
    without sh= differs by more than 0.02 at the median pixel: the fixture can see the feature."""
    from gaussiangrasper_amd import ops
    from gaussiangrasper_amd.camera import ring_cameras
    from gaussiangrasper_amd.edit import select_and_move
    from gaussiangrasper_amd.pipeline import render_view
    from gaussiangrasper_amd.scene import Scene
    rt = rigid()
    planes = box_planes([-3, -3, -3], [3, 3, 3])
    views = ring_cameras(3, 48, 64)
    base = fixture_a(deg).to(DEV)

    def render(sc, view):
        with torch.no_grad():
            return render_view(sc, view, ops, sh_degree_to_use=deg, channels=("rgb",))["rgb"].detach().cpu().double()

    def moved(with_sh):
        sc = Scene(*[t.clone() for t in base.params()])
        _, count = select_and_move(sc.means, sc.quats, planes, rt, sh=sc.colors_all if with_sh else None)
        assert int(count.item()) == 400
        return sc

    turned, stale = moved(True), moved(False)
    assert torch.equal(turned.means, stale.means) and not torch.equal(turned.colors_all, stale.colors_all)
    for v, view in enumerate(views):
        ref = render(base, view)
        assert ref.shape == (48, 64, 3)
        mv = moved_view(view, rt)
        diff = (render(turned, mv) - ref).abs().amax(dim=-1)
        aside = diff > 1e-4
        rest = float(diff[~aside].max())
        gap = float((render(stale, mv) - ref).abs().amax(dim=-1).median())
        print(f"fixture A, degree {deg}, view {v}: set aside {int(aside.sum())} of {aside.numel()} pixels, "
              f"others within {rest:.3g} (bound 2e-5); without sh= the median pixel differs by {gap:.3g}")
        assert float(aside.double().mean()) <= 0.005
        assert rest <= 2e-5
        assert gap > 0.02


# ------------------------------------------------------------------------------------------------
# edit_model and the checkpoint tool
# ------------------------------------------------------------------------------------------------
@gpu
def test_edit_model_rotate_sh_on_the_stub_model():
    from gaussiangrasper_amd.edit import edit_model
    from gaussiangrasper_amd.scene import make_scene
    from gaussiangrasper_amd.stub import StubGaussianSplattingModel
    model = StubGaussianSplattingModel(make_scene(6000, feature_dim=8)).to(DEV)
    opt = torch.optim.Adam(model.get_gaussian_param_groups()["color"], lr=1e-3)
    model.colors_all.grad = torch.randn_like(model.colors_all)
    opt.step()
    moments = {k: v.clone() for k, v in opt.state[model.colors_all].items()}
    param, c0 = model.colors_all, model.colors_all.detach().clone()
    planes, rt = box_planes([-0.4, -0.4, -0.3], [0.4, 0.4, 0.3]), rigid()
    ver = param._version
    n0 = edit_model(model, planes, np.eye(3, 4, dtype=np.float32))          # default: colours untouched
    assert param._version == ver and torch.equal(param.detach(), c0)
    means_before = model.means.detach().clone()
    n1 = edit_model(model, planes, rt, rotate_sh=True)
    assert n1 == n0 > 0
    assert param._version > ver
    assert model.colors_all is param and opt.param_groups[0]["params"][0] is param
    for k, v in moments.items():
        assert torch.equal(opt.state[param][k], v)              # Adam moments are left as they are
    x = means_before.cpu().numpy().astype(np.float64)
    sel = ((np.abs(x) <= np.array([0.4, 0.4, 0.3])).all(axis=1)).astype(np.uint8)
    assert int(sel.sum()) == n1
    assert_same_bits(param.detach().cpu().numpy(), sh_rotate_ref(c0.cpu().numpy(), packed_for(rt[:, :3], 25), sel))


@gpu
@pytest.mark.parametrize("stored", [torch.float32, torch.float64])
def test_checkpoint_round_trip(tmp_path, monkeypatch, stored):
    from gaussiangrasper_amd import edit, interop
    from gaussiangrasper_amd.scene import make_scene
    sc = make_scene(5000, feature_dim=8)
    pipe = interop.state_dict_from_scene(sc, {})
    pipe["_model.colors_all"] = pipe["_model.colors_all"].to(stored)
    ck = tmp_path / "step-000029999.ckpt"
    torch.save({"step": 29999, "pipeline": pipe, "optimizers": {}}, ck)
    planes = box_planes([-0.5, -0.5, -0.4], [0.5, 0.5, 0.4])
    monkeypatch.setattr(edit, "hull_planes", lambda pts: planes)         # the hull itself is not under test (no Qhull)
    obj = np.random.default_rng(0).normal(size=(100, 3))
    pose_from, pose_to = [0.1, 0.0, 0.2, 0.0, 0.1, 0.0], [0.3, -0.1, 0.2, 0.2, 0.1, -0.4]
    outs = {}
    for flag in (False, True):
        out = tmp_path / f"out{int(flag)}.ckpt"
        n = edit.edit_checkpoint(str(ck), obj, np.eye(4), 1.0, pose_from, pose_to, str(out), rotate_sh=flag)
        assert n > 0
        outs[flag] = torch.load(out, weights_only=True)["pipeline"]
    src = torch.load(ck, weights_only=True)["pipeline"]
    key = "_model.colors_all"
    assert outs[False][key].dtype == stored and torch.equal(outs[False][key], src[key])
    assert outs[False][key].numpy().tobytes() == src[key].numpy().tobytes()
    for k in src:
        assert torch.equal(outs[True][k], outs[False][k]) == (k != key), k
    rt = edit.compose_transform(np.eye(4), 1.0, pose_from, pose_to)
    m, q = src["_model.means"].to(DEV), src["_model.quats"].to(DEV)
    mask, _ = edit.select_and_move(m, q, planes, rt)
    c32 = src[key].float().numpy()
    want = torch.from_numpy(sh_rotate_ref(c32, packed_for(rt[:, :3], c32.shape[1]), mask.cpu().numpy())).to(stored)
    assert outs[True][key].dtype == stored
    assert outs[True][key].numpy().tobytes() == want.numpy().tobytes()
