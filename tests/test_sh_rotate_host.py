"""No-GPU checks of the SH rotation (gaussiangrasper_amd.sh_rotation, gg_sh_rotate): the restated basis against the
header and the fp64 oracle, the fitted band matrices against the invariance that defines them (on the oracle's own SH
evaluation), their group properties, the inputs they refuse, the fp32 restatement of the kernel's arithmetic
(tests/sh_rotate_ref.py) against the same invariance, the C entry's argument validation and the command line's
plumbing of --rotate-sh."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from sh_rotate_ref import BAND_OFFSETS, sh_rotate_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rotations():
    """a generic turn, a half turn about an axis, a 1e-4 rad turn"""
    from gaussiangrasper_amd.edit import rotvec_to_matrix
    axis = np.array([0.3, -0.5, 0.81])
    axis /= np.linalg.norm(axis)
    return [rotvec_to_matrix([0.9, -1.3, 0.6]), rotvec_to_matrix(np.pi * axis),
            rotvec_to_matrix(1e-4 * np.array([0.6, 0.0, -0.8]))]


def unit_dirs(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def apply_bands(bands, c):
    """D c per channel in fp64: c (N, K, 3)"""
    out = c.copy()
    for l, D in enumerate(bands, start=1):
        lo, hi = l * l, (l + 1) * (l + 1)
        if hi <= c.shape[1]:
            out[:, lo:hi, :] = np.einsum("ab,nbc->nac", D, c[:, lo:hi, :])
    return out


def test_constants_are_the_headers_literals():
    from gaussiangrasper_amd import sh_rotation
    src = open(os.path.join(ROOT, "include", "gg_constants.h")).read()
    defs = dict(re.findall(r"^#define\s+(GG_SH_C[0-9_]+)\s+(-?[0-9.]+)f\b", src, flags=re.M))
    assert len(defs) == 23
    assert set(defs) == set(sh_rotation.SH_CONSTANTS)
    for name, text in defs.items():
        assert sh_rotation.SH_CONSTANTS[name] == float(np.float32(float(text))), name


def test_basis_is_the_oracles(oracle):
    from gaussiangrasper_amd.sh_rotation import sh_basis
    d = np.random.default_rng(0).normal(size=(1000, 3)) * 3.0        # not normalised: the basis normalises
    ones = np.ones((1000, 3))
    for deg in (1, 2, 3, 4):
        k = (deg + 1) ** 2
        ref = oracle.sh_bwd(deg, k, d, ones, dtype=np.float64)[:, :, 0]
        got = sh_basis(d, deg)
        assert got.shape == (1000, k) and got.dtype == np.float64
        assert np.abs(got - ref).max() <= 1e-14
    ref = oracle.sh_bwd(4, 25, d, ones, dtype=np.float64)[:, :, 0]
    assert np.abs(sh_basis(d, 4) - ref).max() <= 1e-14


def test_fit_is_well_conditioned():
    from gaussiangrasper_amd.sh_rotation import fit_directions, sh_basis
    X = fit_directions()
    assert X.shape == (96, 3) and np.abs(np.linalg.norm(X, axis=1) - 1.0).max() < 1e-15
    Y = sh_basis(X, 4)
    for l in (1, 2, 3, 4):
        assert np.linalg.cond(Y[:, l * l:(l + 1) ** 2]) < 1.05


def test_invariance_on_the_fp64_oracle(oracle):
    from gaussiangrasper_amd.sh_rotation import rotation_bands
    rng = np.random.default_rng(1)
    d = unit_dirs(1000, 2)
    worst = 0.0
    for R in rotations():
        bands = rotation_bands(R)
        assert [b.shape for b in bands] == [(3, 3), (5, 5), (7, 7), (9, 9)] and all(b.dtype == np.float64 for b in bands)
        for deg in (1, 2, 3, 4):
            c = rng.normal(size=(1000, (deg + 1) ** 2, 3))
            before = oracle.sh_fwd(deg, d, c, dtype=np.float64)
            after = oracle.sh_fwd(deg, d @ R.T, apply_bands(bands, c), dtype=np.float64)
            ratio = np.abs(after - before) / np.abs(c).sum(axis=1)
            worst = max(worst, ratio.max())
            assert (np.abs(after - before) <= 1e-12 * np.abs(c).sum(axis=1)).all()
    print(f"fp64 invariance: worst |diff| / sum|c| = {worst:.3g} (bound 1e-12)")


def test_composition_identity_orthogonality():
    from gaussiangrasper_amd.sh_rotation import rotation_bands
    R1, R2, R3 = rotations()
    for A, B in ((R1, R2), (R2, R3), (R3, R1)):
        for DAB, DA, DB in zip(rotation_bands(A @ B), rotation_bands(A), rotation_bands(B)):
            assert np.abs(DAB - DA @ DB).max() <= 1e-12
    for l, D in enumerate(rotation_bands(np.eye(3)), start=1):
        assert np.abs(D - np.eye(2 * l + 1)).max() <= 1e-14
    worst = 0.0
    for R in rotations():
        for l, D in enumerate(rotation_bands(R), start=1):
            worst = max(worst, np.abs(D @ D.T - np.eye(2 * l + 1)).max())
    assert worst <= 2.5e-7
    assert len(rotation_bands(R1, degree=2)) == 2 and rotation_bands(R1, degree=0) == []


def test_input_is_projected_to_the_nearest_rotation():
    from gaussiangrasper_amd.sh_rotation import nearest_rotation, rotation_bands
    R = rotations()[0]
    R32 = R.astype(np.float32).astype(np.float64)           # what edit passes: off orthonormal by ~1e-7
    P = nearest_rotation(R32)
    assert np.abs(P.T @ P - np.eye(3)).max() < 1e-15 and np.abs(P - R).max() < 1e-7
    for D, Dp in zip(rotation_bands(R32), rotation_bands(P)):
        assert np.abs(D - Dp).max() <= 1e-14         # (projecting twice moves the last bits)


def test_rejected_inputs():
    from gaussiangrasper_amd.sh_rotation import pack_bands, rotation_bands, sh_basis
    R = rotations()[0]
    with pytest.raises(ValueError, match="reflection"):
        rotation_bands(R @ np.diag([1.0, 1.0, -1.0]))
    off = R.copy()
    off[0, 0] += 1e-3
    with pytest.raises(ValueError, match="orthonormal"):
        rotation_bands(off)
    with pytest.raises(ValueError, match="orthonormal"):
        rotation_bands(R * 1.001)                            # a similarity: out of scope
    for bad in (np.eye(4), np.zeros((3, 4)), np.zeros(9)):
        with pytest.raises(ValueError, match=r"\(3, 3\)"):
            rotation_bands(bad)
    with pytest.raises(ValueError, match="finite"):
        rotation_bands(np.full((3, 3), np.nan))
    with pytest.raises(ValueError, match="degree"):
        rotation_bands(R, degree=5)
    with pytest.raises(ValueError, match=r"\(M, 3\)"):
        sh_basis(np.zeros((4, 2)), 2)
    bands = rotation_bands(R)
    with pytest.raises(ValueError, match="num_bases"):
        pack_bands(bands, 5)
    with pytest.raises(ValueError, match="bands"):
        pack_bands(bands[:2], 25)
    with pytest.raises(ValueError, match="D_2"):
        pack_bands([bands[0], bands[0]], 9)


def test_pack_bands_layout():
    from gaussiangrasper_amd.sh_rotation import pack_bands, rotation_bands
    bands = rotation_bands(rotations()[0])
    for deg, k in enumerate((1, 4, 9, 16, 25)):
        p = pack_bands(bands, k)
        assert p.dtype == np.float32 and p.shape == (BAND_OFFSETS[deg],) and p.flags.c_contiguous
        for l in range(1, deg + 1):
            w = 2 * l + 1
            assert np.array_equal(p[BAND_OFFSETS[l - 1]:BAND_OFFSETS[l]].reshape(w, w), bands[l - 1].astype(np.float32))
    assert BAND_OFFSETS == (0, 9, 34, 83, 164)


def test_fp32_restatement_meets_the_invariance_on_the_fp32_oracle(oracle):
    from gaussiangrasper_amd.sh_rotation import pack_bands, rotation_bands
    rng = np.random.default_rng(3)
    d = unit_dirs(1000, 4)
    worst = 0.0
    for R in rotations():
        bands = rotation_bands(R)
        for deg in (1, 2, 3, 4):
            k = (deg + 1) ** 2
            c = rng.normal(size=(1000, k, 3)).astype(np.float32)
            turned = sh_rotate_ref(c, pack_bands(bands, k))
            assert turned.dtype == np.float32 and np.array_equal(turned[:, 0], c[:, 0])
            before = oracle.sh_fwd(deg, d, c, dtype=np.float32).astype(np.float64)
            after = oracle.sh_fwd(deg, d @ R.T, turned, dtype=np.float32).astype(np.float64)
            total = np.abs(c.astype(np.float64)).sum(axis=1)
            worst = max(worst, (np.abs(after - before) / total).max())
            assert (np.abs(after - before) <= 2e-7 * total).all()
    print(f"fp32 restatement: worst |diff| / sum|c| = {worst:.3g} (bound 2e-7)")


def test_restatement_leaves_unselected_rows_and_band_0():
    from gaussiangrasper_amd.sh_rotation import pack_bands, rotation_bands
    c = np.random.default_rng(5).normal(size=(10, 9, 3)).astype(np.float32)
    mask = np.array([0, 1, 0, 2, 0, 255, 0, 0, 1, 0], np.uint8)
    out = sh_rotate_ref(c, pack_bands(rotation_bands(rotations()[0]), 9), mask)
    assert np.array_equal(out[mask == 0], c[mask == 0]) and np.array_equal(out[:, 0], c[:, 0])
    assert not np.array_equal(out[mask != 0, 1:], c[mask != 0, 1:])
    assert np.array_equal(sh_rotate_ref(c[:, :1].copy(), np.zeros(0, np.float32)), c[:, :1])


def test_sh_rotate_argument_validation_without_a_gpu():
    """invalid arguments are rejected on the host before anything is launched; K = 1 and N = 0 return without a launch
    (checked on a thread of its own: gg_last_error is per thread)"""
    import threading
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    n = ctypes.c_void_p(0)
    fake = ctypes.c_void_p(1 << 20)     # never dereferenced: every call below returns before a launch
    bands = (ctypes.c_float * 164)()
    host = ctypes.cast(bands, ctypes.c_void_p)
    bad = [((-1, 25, fake, n, host, n), b"num_points"),
           ((10, 5, fake, n, host, n), b"num_bases"),
           ((10, 0, fake, n, host, n), b"num_bases"),
           ((10, 36, fake, n, host, n), b"num_bases"),
           ((10, 25, n, n, host, n), b"null pointer"),
           ((10, 25, fake, n, n, n), b"null pointer"),
           ((10, 25, ctypes.c_void_p((1 << 20) + 2), n, host, n), b"misaligned")]
    ok = [(10, 1, fake, fake, n, n), (0, 25, n, n, n, n), (0, 1, n, n, n, n)]
    got = []

    def run():
        for args, _ in bad:
            got.append((lib.gg_sh_rotate(*args), lib.gg_last_error()))
        for args in ok:
            got.append((lib.gg_sh_rotate(*args), b""))
    t = threading.Thread(target=run)
    t.start()
    t.join()
    assert len(got) == len(bad) + len(ok)
    for (st, msg), (_, want) in zip(got, bad):
        assert st == -1 and msg.startswith(b"gg_sh_rotate") and want in msg, msg
    assert [st for st, _ in got[len(bad):]] == [0, 0, 0]


def test_python_surface_refuses_host_tensors_and_bad_layouts():
    from gaussiangrasper_amd import sh_rotation
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sh_rotation.rotate_coefficients(torch.zeros(4, 9, 3), np.eye(3))
    for bad in (torch.zeros(4, 9, 3, dtype=torch.float64), torch.zeros(4, 10, 3), torch.zeros(4, 9, 4),
                torch.zeros(4, 27), torch.zeros(4, 3, 9).transpose(1, 2)):
        with pytest.raises(ValueError, match="SH coefficients"):
            sh_rotation.check_coefficients(bad)
    good = torch.zeros(4, 16, 3)
    assert sh_rotation.check_coefficients(good) == 16
    for bad in (torch.zeros(4, dtype=torch.bool), torch.zeros(5, dtype=torch.uint8), torch.zeros(4, 1, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="mask"):
            sh_rotation.check_coefficients(good, bad)


def test_command_line_passes_rotate_sh_through(tmp_path, monkeypatch):
    """The tool's device path needs the GPU (tests/test_sh_rotate_gpu.py holds the bytes); here: the flag reaches
    edit_checkpoint, is off by default, and a checkpoint without colors_all is refused before any device work."""
    from gaussiangrasper_amd import edit
    np.save(tmp_path / "obj.npy", np.random.default_rng(0).normal(size=(50, 3)))
    (tmp_path / "transform.json").write_text(json.dumps({"transform_matrix": np.eye(4).tolist(), "scale": 1.0}))
    seen = []

    def fake(*args, **kwargs):
        seen.append(kwargs.get("rotate_sh"))
        return 7
    monkeypatch.setattr(edit, "edit_checkpoint", fake)
    base = ["--ckpt", "x.ckpt", "--object-points", str(tmp_path / "obj.npy"), "--transform-json",
            str(tmp_path / "transform.json"), "--pose-from", *["0"] * 6, "--pose-to", *["0"] * 6, "--out", "y.ckpt"]
    assert edit.main(base) == 0 and edit.main(base + ["--rotate-sh"]) == 0
    assert seen == [False, True]
    monkeypatch.undo()

    ck =tmp_path / "step-000001000.ckpt"
    torch.save({"step": 1000, "pipeline": {"_model.means": torch.zeros(3, 3), "_model.quats": torch.zeros(3, 4)},
                "optimizers": {}}, ck)
    out = tmp_path / "out.ckpt"
    with pytest.raises(SystemExit, match="_model.colors_all"):
        edit.main(["--ckpt", str(ck), "--object-points", str(tmp_path / "obj.npy"), "--transform-json",
                   str(tmp_path / "transform.json"), "--pose-from", *["0"] * 6, "--pose-to", *["0"] * 6,
                   "--out", str(out), "--rotate-sh"])
    assert not out.exists()
