"""GPU checks of the registration kernels (gg_cloud_frames, gg_icp_step) and of register.colored_icp /
refine_scan_poses against the fp64 numpy restatement (tests/register_ref.py).  The bounds are the issue's; the
measured values are printed before they are asserted and recorded in PARITY.md "Registration"."""
import numpy as np
import pytest
import torch

import register_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev32(a):
    return torch.tensor(np.asarray(a, dtype=np.float32), device=DEV)


@pytest.fixture(scope="module")
def scene():
    """The scene and the restatement's frames of its target, computed once and never changed."""
    P, I, S, Is = R.scene()
    nrm, grad, count, valid, gap = R.cloud_frames(P, I, 0.02)
    s = dict(P=P, I=I, S=S, Is=Is, nrm=nrm, grad=grad, count=count, valid=valid, gap=gap,
             nrm32=R.f32(nrm), grad32=R.f32(grad))
    for v in s.values():
        v.setflags(write=False)
    return s


def gpu_frames(P, I, radius, grid=None):
    from gaussiangrasper_amd.register import cloud_frames
    t = cloud_frames(dev32(P), dev32(I), radius, grid=grid)
    torch.cuda.synchronize()
    return (t.normals.double().cpu().numpy(), t.gradients.double().cpu().numpy(), t.count.cpu().numpy(),
            t.valid.cpu().numpy().astype(bool))


def check_frames(P, I, radius, ref=None, what="", max_excluded=0.0, grid=None):
    P, I = R.f32(P), R.f32(I)
    nrm, grad, count, valid = gpu_frames(P, I, radius, grid)
    rn, rg, rc, rv, gap = ref if ref is not None else R.cloud_frames(P, I, radius)
    assert np.array_equal(count, rc) and np.array_equal(valid, rv)
    assert np.isnan(nrm[~rv]).all() and (grad[~rv] == 0).all()
    assert np.allclose(np.linalg.norm(nrm[rv], axis=1), 1.0, rtol=0, atol=1e-6)
    lead = np.take_along_axis(nrm[rv], np.argmax(np.abs(nrm[rv]), axis=1)[:, None], axis=1)
    assert (lead > 0).all()
    clear = rv & (gap >= 1e-2)
    excluded = int((rv & ~clear).sum())
    dn = np.abs(nrm[clear] - rn[clear]).max(initial=0.0)
    size = np.linalg.norm(rg, axis=1)
    dg = np.abs(grad - rg).max(axis=1)
    bound = 1e-5 * size + 1e-6 * size.max(initial=0.0)
    worst = (dg[clear] / np.where(bound[clear] > 0, bound[clear], 1.0)).max(initial=0.0)
    print(f"frames {what}: N {len(P)}, excluded by the eigen-gap {excluded}, max normal deviation {dn:.3e} (1e-6), "
          f"max gradient deviation {dg[clear].max(initial=0.0):.3e}, {worst:.3f} of its bound")
    assert excluded <= max_excluded * len(P)
    assert dn <= 1e-6
    assert (dg[clear] <= bound[clear]).all()
    return nrm, grad, count, valid


@pytest.mark.parametrize("n", [1, 2, 3, 4, 257])
def test_cloud_frames_small(n):
    rng = np.random.default_rng(100 + n)
    P = rng.uniform(0.0, 0.02, (n, 3)) * [1.0, 1.0, 0.2]
    I = rng.uniform(0.0, 1.0, n)
    check_frames(P, I, 0.015, what=f"random {n}", max_excluded=0.01 if n >= 100 else 0.0)


def test_cloud_frames_scene(scene):
    ref = (scene["nrm"], scene["grad"], scene["count"], scene["valid"], scene["gap"])
    check_frames(scene["P"], scene["I"], 0.02, ref=ref, what="scene")


def test_cloud_frames_special_cases():
    # a pile of identical points: a frame exists (count >= 3), the gradient system is singular
    P = np.tile([[0.25, -0.5, 0.125]], (6, 1))
    nrm, grad, count, valid = gpu_frames(P, np.linspace(0, 1, 6), 0.1)
    assert (count == 6).all() and valid.all() and (grad == 0).all()
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, rtol=0, atol=1e-6)
    # a NaN point is invalid and nobody's neighbour
    rng = np.random.default_rng(5)
    P = rng.uniform(0, 0.01, (9, 3))
    P[4, 1] = np.nan
    P[7, 0] = np.inf
    nrm, grad, count, valid = check_frames(P, rng.uniform(0, 1, 9), 0.05, what="NaN point")
    assert count[4] == 0 and count[7] == 0 and (count[[0, 1, 2, 3, 5, 6, 8]] == 7).all()
    # exactly collinear points: the normal is perpendicular to the line, the gradient system is singular
    P = np.zeros((5, 3))
    P[:, 0] = [0.0, 0.125, 0.25, 0.375, 0.5]
    nrm, grad, count, valid = gpu_frames(P, P[:, 0], 1.0)
    assert (count == 5).all() and valid.all() and (nrm[:, 0] == 0).all() and (grad == 0).all()
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, rtol=0, atol=1e-6)
    # exactly coplanar points with a linear intensity: the plane's normal, the tangential part of the slope
    xy = rng.integers(-64, 64, (40, 2)) / 1024.0
    P = np.c_[xy, np.full(40, 0.5)]
    a = np.array([1.5, -2.0, 0.75])
    nrm, grad, count, valid = check_frames(P, P @ a, 1.0, what="coplanar")
    assert np.abs(nrm - [0, 0, 1]).max() <= 1e-6
    assert np.abs(grad - [1.5, -2.0, 0.0]).max() <= 1e-5 * 2.5 + 1e-6 * 2.5
    # a pair exactly at the radius is a pair of neighbours; one ulp less of radius and it is not
    P = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0]])
    assert (gpu_frames(P, [0.0, 1.0], 0.25)[2] == 2).all()
    assert (gpu_frames(P, [0.0, 1.0], np.nextafter(0.25, 0.0))[2] == 1).all()


# ------------------------------------------------------------------------------------------------
# gg_icp_step
# ------------------------------------------------------------------------------------------------
def make_target(P, I, nrm, grad, valid):
    from gaussiangrasper_amd.register import IcpTarget
    n = len(P)
    return IcpTarget(points=dev32(P), intensity=dev32(I), normals=dev32(nrm), gradients=dev32(grad),
                     count=torch.zeros(n, dtype=torch.int32, device=DEV),
                     valid=torch.tensor(np.asarray(valid, dtype=np.uint8), device=DEV), radius=0.0)


def gpu_step(S, Is, target, T, max_dist, lam, **kw):
    from gaussiangrasper_amd.register import icp_step
    r = icp_step(dev32(S), dev32(Is), target, T, max_dist, lam, corr=True, abs_sums=True, **kw)
    return r.sums, r.abs_sums, r.corr.cpu().numpy()


def check_step(S, Is, P, I, nrm, grad, valid, T, max_dist, lam, what=""):
    S, Is, P, I, nrm, grad = (R.f32(x) for x in (S, Is, P, I, nrm, grad))
    target = make_target(P, I, nrm, grad, valid)
    sums, asum, corr = gpu_step(S, Is, target, T, max_dist, lam)
    rs, ra, rc = R.icp_sums(S, Is, P, I, nrm, grad, valid, T, max_dist, lam)
    assert np.array_equal(corr, rc) and sums[27] == rs[27] == (rc >= 0).sum()
    bound = len(S) * 2.0 ** -52 * asum
    worst = (np.abs(sums - rs) / np.where(bound > 0, bound, 1.0)).max()
    print(f"icp_step {what}: M {len(S)}, N {len(P)}, inliers {int(sums[27])}, worst sum deviation {worst:.3e} of "
          f"M 2^-52 abs_sums")
    assert (np.abs(sums - rs) <= bound).all() and sums[31] == 0
    assert (np.abs(asum - ra) <= bound).all()
    sums2, asum2, corr2 = gpu_step(S, Is, target, T, max_dist, lam)
    assert sums.tobytes() == sums2.tobytes() and asum.tobytes() == asum2.tobytes() and np.array_equal(corr, corr2)
    return sums, corr, target


START = R.rigid([0.004, -0.003, 0.006], [0.0012, -0.0008, 0.0006])


@pytest.mark.parametrize("m", [1, 63, 64, 65, 256, 257, 3000])
def test_icp_step_against_the_scene(scene, m):
    S, Is = scene["S"][:m], scene["Is"][:m]
    T = R.TRUE_MOTION @ START                        # near the answer, so that most points have a correspondent
    check_step(S, Is, scene["P"], scene["I"], scene["nrm32"], scene["grad32"], scene["valid"], T, 0.01, 0.968,
               what="scene")


@pytest.mark.parametrize("m", [1, 63, 64, 65, 256, 257, 3000])
def test_icp_step_against_one_point(m):
    rng = np.random.default_rng(m)
    S = rng.normal(0.0, 0.02, (m, 3))
    n = np.array([0.6, 0.0, 0.8])
    check_step(S, rng.uniform(0, 1, m), [[0.001, -0.002, 0.003]], [0.4], [n], [[0.3, -0.2, 0.1]], [1],
               R.rigid([0.01, 0.02, -0.01], [0.001, 0.0, -0.001]), 0.03, 0.5, what="one target")


@pytest.fixture(scope="module")
def long_source():
    """8449 source points (34 slab rows of 256) of the scene's surface, seen from the frame moved by the inverse of
    TRUE_MOTION as R.scene()'s are; prefixes of it are the shorter sources."""
    S0, Is = R.surface(8449, 3)
    Gi = np.linalg.inv(R.TRUE_MOTION)
    S = R.f32(S0 @ Gi[:3, :3].T + Gi[:3, 3])
    S.setflags(write=False), Is.setflags(write=False)
    return S, Is


@pytest.mark.parametrize("m", [4096, 4097, 8449])
def test_icp_step_past_one_row_per_chain(scene, long_source, m):
    # rg_finish_kernel sums the slab's rows by 16 chains: 16, 17 and 34 rows give chain 0 one, two and three rows
    S, Is = long_source[0][:m], long_source[1][:m]
    sums, _, _ = check_step(S, Is, scene["P"], scene["I"], scene["nrm32"], scene["grad32"], scene["valid"],
                            R.TRUE_MOTION @ START, 0.01, 0.968, what="scene, long source")
    assert sums[27] > 0.9 * m                        # the rows past the first pass hold inliers


@pytest.mark.parametrize("m", [1, 257, 3000, 8449])
def test_icp_step_without_corr_and_abs_sums(scene, long_source, m):
    # rg_step_kernel<false> / rg_finish_kernel<false> with corr == NULL is what colored_icp runs: the same terms
    # summed in the same order, so the same bits
    from gaussiangrasper_amd.register import icp_step
    S, Is = dev32(long_source[0][:m]), dev32(long_source[1][:m])
    target = make_target(scene["P"], scene["I"], scene["nrm32"], scene["grad32"], scene["valid"])
    T = R.TRUE_MOTION @ START
    full = icp_step(S, Is, target, T, 0.01, 0.968, corr=True, abs_sums=True)
    lean = icp_step(S, Is, target, T, 0.01, 0.968, corr=False, abs_sums=False)
    assert lean.corr is None and lean.abs_sums is None
    assert full.sums[27] == (full.corr.cpu().numpy() >= 0).sum() > 0.9 * m
    assert lean.sums.tobytes() == full.sums.tobytes()


def test_icp_step_workspace_across_source_sizes(scene, long_source):
    # one StepWorkspace, one target and max_dist: a shorter source reuses the sort, a longer one grows the workspace
    # and sorts again; every step equals a fresh call's
    from gaussiangrasper_amd.register import StepWorkspace
    target = make_target(scene["P"], scene["I"], scene["nrm32"], scene["grad32"], scene["valid"])
    T = R.TRUE_MOTION @ START
    st = StepWorkspace()
    sizes = []
    for m in (3000, 257, 8449, 3000):
        S, Is = long_source[0][:m], long_source[1][:m]
        kept = gpu_step(S, Is, target, T, 0.01, 0.968, state=st)
        fresh = gpu_step(S, Is, target, T, 0.01, 0.968)
        assert fresh[0][27] > 0.9 * m
        assert kept[0].tobytes() == fresh[0].tobytes() and kept[1].tobytes() == fresh[1].tobytes()
        assert np.array_equal(kept[2], fresh[2])
        sizes.append(st.ws.numel())
    assert sizes[0] == sizes[1] < sizes[2] == sizes[3]           # kept, kept, grown, kept


# "any grid gives the same result" (include/gg_raster.h): one cell, and a grid that misses the cloud, which clamps
# every point into one corner cell; (lower corner and cell edge, cells per axis) as cluster.cluster_grid returns them
HOSTILE_GRIDS = {"one cell": (np.array([0.0, 0.0, 0.0, 1.0]), np.array([1, 1, 1], np.int32)),
                 "misses the cloud": (np.array([50.0, 50.0, 50.0, 0.001]), np.array([40, 30, 20], np.int32))}


@pytest.fixture(scope="module")
def small_target():
    """A 3000-point target and the restatement's frames of it, computed once and never changed."""
    P, I = R.surface(3000, 4)
    ref = R.cloud_frames(P, I, 0.02)
    for v in (P, I) + ref:
        v.setflags(write=False)
    return P, I, ref


@pytest.mark.parametrize("grid", list(HOSTILE_GRIDS))
def test_cloud_frames_on_any_grid(small_target, grid):
    # count and valid equal the restatement's; the fp64 sums follow slot order, so normals and gradients keep
    # check_frames' bounds rather than bits
    P, I, ref = small_target
    check_frames(P, I, 0.02, ref=ref, what=f"3000 points, {grid}", grid=HOSTILE_GRIDS[grid])
    assert ref[3].all() and ref[2].min() >= 4


@pytest.mark.parametrize("grid", list(HOSTILE_GRIDS))
def test_icp_step_on_any_grid(small_target, long_source, grid):
    # the correspondent is the smallest (distance, index) pair and the sums have a fixed order: nothing depends on
    # the slot order, so a caller's grid gives the fitted grid's correspondences and bytes
    P, I, (nrm, grad, _, valid, _) = small_target
    target = make_target(P, I, R.f32(nrm), R.f32(grad), valid)
    S, Is, T = long_source[0][:257], long_source[1][:257], R.TRUE_MOTION @ START
    fit = gpu_step(S, Is, target, T, 0.01, 0.968)
    got = gpu_step(S, Is, target, T, 0.01, 0.968, grid=HOSTILE_GRIDS[grid])
    print(f"icp_step {grid}: {int(fit[0][27])} of 257 source points have a correspondent")
    assert fit[0][27] > 128
    assert np.array_equal(got[2], fit[2])
    assert got[0].tobytes() == fit[0].tobytes() and got[1].tobytes() == fit[1].tobytes()


def test_icp_step_is_independent_of_the_target_order(scene):
    S, Is, T = scene["S"], scene["Is"], R.TRUE_MOTION @ START
    sums, corr, _ = check_step(S, Is, scene["P"], scene["I"], scene["nrm32"], scene["grad32"], scene["valid"], T,
                               0.01, 0.968, what="in order")
    perm = np.random.default_rng(9).permutation(len(scene["P"]))
    t2 = make_target(scene["P"][perm], scene["I"][perm], scene["nrm32"][perm], scene["grad32"][perm],
                     scene["valid"][perm])
    sums2, _, corr2 = gpu_step(S, Is, t2, T, 0.01, 0.968)
    assert np.array_equal(np.where(corr2 >= 0, perm[np.maximum(corr2, 0)], -1), corr)
    assert sums.tobytes() == sums2.tobytes()
    # a kept workspace (the target sorted once) changes nothing either
    from gaussiangrasper_amd.register import StepWorkspace
    st = StepWorkspace()
    a = gpu_step(S, Is, t2, T, 0.01, 0.968, state=st)
    b = gpu_step(S, Is, t2, T, 0.01, 0.968, state=st)
    assert a[0].tobytes() == b[0].tobytes() == sums.tobytes() and np.array_equal(a[2], b[2])


def test_icp_step_special_cases():
    I4 = np.eye(4)
    z, up = [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]
    one = dict(P=[z], I=[0.5], nrm=[up], grad=[[0.5, 0.25, 0.0]], valid=[1])
    # exactly max_dist away: in; one ulp (of the fp32 coordinate) beyond: out
    sums, corr, _ = check_step([[0.25, 0.0, 0.0]], [0.5], T=I4, max_dist=0.25, lam=0.968, what="at max_dist", **one)
    assert corr[0] == 0 and sums[27] == 1 and sums[28] == 0.0625
    beyond = np.nextafter(np.float32(0.25), np.float32(1.0))
    sums, corr, _ = check_step([[beyond, 0.0, 0.0]], [0.5], T=I4, max_dist=0.25, lam=0.968, what="one ulp beyond",
                               **one)
    assert corr[0] == -1 and not sums.any()
    # two targets equidistant: the smaller index, whichever side it is on
    for first in (-0.125, 0.125):
        two = dict(P=[[first, 0, 0], [-first, 0, 0]], I=[0.5, 0.25], nrm=[up, up], grad=[z, z], valid=[1, 1])
        _, corr, _ = check_step([z], [0.5], T=I4, max_dist=0.5, lam=0.968, what="equidistant", **two)
        assert corr[0] == 0
    # an invalid nearest target is skipped
    inv = dict(P=[[0.01, 0, 0], [0.05, 0, 0]], I=[0.5, 0.25], nrm=[up, up], grad=[z, z], valid=[0, 1])
    _, corr, _ = check_step([z], [0.5], T=I4, max_dist=0.5, lam=0.968, what="invalid nearest", **inv)
    assert corr[0] == 1
    # a NaN source point has no correspondent; the others keep theirs
    sums, corr, _ = check_step([[np.nan, 0, 0], [0.01, 0, 0], [0, np.inf, 0]], [0.5, 0.5, 0.5], T=I4, max_dist=0.5,
                               lam=0.968, what="NaN source", **one)
    assert corr.tolist() == [-1, 0, -1] and sums[27] == 1
    # no inliers at all: every sum is zero
    S = np.random.default_rng(2).uniform(5.0, 6.0, (300, 3))
    sums, corr, _ = check_step(S, np.zeros(300), T=I4, max_dist=0.5, lam=0.968, what="no inliers", **one)
    assert (corr == -1).all() and not sums.any()


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
def test_colored_icp_end_to_end(scene):
    from gaussiangrasper_amd.register import colored_icp
    col = lambda i: np.repeat(i[:, None], 3, axis=1)
    for lam, colours in ((0.968, True), (1.0, False)):
        sc, pc = (col(scene["Is"]), col(scene["I"])) if colours else (None, None)
        Tr, fit_r, rmse_r, it_r = R.colored_icp(scene["S"], sc, scene["P"], pc, lam=lam)
        rot_r, tr_r = R.motion_error(Tr)
        r = colored_icp(scene["S"], sc, scene["P"], pc, lambda_geometric=lam)
        rot, tr = R.motion_error(r.transformation)
        print(f"colored_icp lambda {lam}: rotation error {rot:.3e} (restatement {rot_r:.3e}), translation error "
              f"{tr:.3e} m ({tr_r:.3e}), fitness {r.fitness:.5f} ({fit_r:.5f}), rmse {r.inlier_rmse:.4e} "
              f"({rmse_r:.4e}), iterations {r.iterations} ({it_r}), {r.status}")
        assert rot <= 1.5 * rot_r + 1e-6 and tr <= 1.5 * tr_r + 1e-6
        assert abs(r.fitness - fit_r) <= 1e-3
        assert len(r.iterations) == 3 and np.isfinite(r.transformation).all()
    rot0, tr0 = R.motion_error(np.eye(4))
    assert rot < 0.1 * rot0 and tr < 0.1 * tr0                 # lambda = 1 without colours converges too


def synthetic_frame(c2w, h=48, w=64, f=120.0):
    """Depth (h, w) fp64 and rgb (h, w, 3) uint8 of the test surface seen by a pinhole camera at c2w (OpenCV axes)."""
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    ray = np.stack([(u - w / 2) / f, (v - h / 2) / f, np.ones_like(u)], axis=-1) @ c2w[:3, :3].T
    d = np.full((h, w), c2w[2, 3])
    for _ in range(40):                                        # |dz/dd| < 1: the fixed point of the ray-surface hit
        p = c2w[:3, 3] + d[..., None] * ray
        d = (R.surface_height(p[..., 0], p[..., 1]) - c2w[2, 3]) / ray[..., 2]
    p = c2w[:3, 3] + d[..., None] * ray
    g = np.uint8(np.clip(R.surface_intensity(p[..., 0], p[..., 1]), 0, 1) * 255 + 0.5)
    return d, np.repeat(g[..., None], 3, axis=2)


def test_refine_scan_poses():
    from gaussiangrasper_amd.prepare import backproject_frames
    from gaussiangrasper_amd.register import refine_scan_poses
    down = np.diag([1.0, -1.0, -1.0])                          # camera looking down the base frame's -z
    centres = [(-0.02, 0.0), (0.01, 0.01), (0.03, -0.01), (1.5, 1.5)]
    errors = [np.eye(4), R.rigid([0.006, -0.004, 0.008], [0.002, -0.0015, 0.001]),
              R.rigid([-0.005, 0.007, -0.006], [-0.0015, 0.002, -0.001]), np.eye(4)]
    true, given, clouds, cams = [], [], [], []
    for (cx, cy), E in zip(centres, errors):
        T = np.eye(4)
        T[:3, :3] = down @ R.rodrigues([0.05 * cx, 0.03, 0.0])
        T[:3, 3] = [cx, cy, 0.4]
        depth, rgb = synthetic_frame(T)
        G = E @ T
        k = [120.0, 120.0, 32.0, 24.0]
        pts, cols = backproject_frames(depth[None], np.ones((1, 48, 64), np.uint8), rgb[None], k, G[None],
                                       (0.001, 1.2), (-1.0, 1.0))
        cam, _ = backproject_frames(depth[None], np.ones((1, 48, 64), np.uint8), rgb[None], k, np.eye(4)[None],
                                    (0.001, 1.2), (-10.0, 10.0))
        assert pts.shape[0] == 48 * 64
        true.append(T), given.append(G), clouds.append((pts, cols.double() / 255.0)), cams.append(cam.cpu().numpy())
    ref = refine_scan_poses(clouds)
    assert ref.accepted == [True, True, True, False] and ref.report[3]["reason"]
    assert np.array_equal(ref.corrections[0], np.eye(4)) and np.array_equal(ref.corrections[3], np.eye(4))

    def rms(A, B, X):
        return float(np.sqrt((((X @ A[:3, :3].T + A[:3, 3]) - (X @ B[:3, :3].T + B[:3, 3])) ** 2).sum(axis=1).mean()))

    for k in (1, 2):
        before, after = rms(given[k], true[k], cams[k]), rms(ref.corrections[k] @ given[k], true[k], cams[k])
        print(f"refine_scan_poses frame {k}: rms point error {before:.3e} m given, {after:.3e} m refined; "
              f"{ref.report[k]}")
        assert after < before
