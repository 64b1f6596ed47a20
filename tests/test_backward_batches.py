"""Every build of the blend backward (csrc/blend2.hip blend2_bwd_wide_kernel, blend2_bwd_narrow_kernel) on the
constructed tile lists of tests/backward_cases.py: survivor counts around the batch sizes, the fullest queue, a
left-over that moves several times, list lengths around the 64-entry chunk, a tile range that starts at 37, and a
batch inside which final_idx differs from pixel to pixel.  tests/test_backward_cases_host.py establishes on the CPU
what the constructions claim.

Calls go through the C ABI.  ids / tile_bins are built directly (list order = index order) and the same arrays go to
the oracle and to the device; final_T / final_idx are the fp32 oracle's forward, the cotangents standard normal, the
reference the fp64 oracle's blend_bwd, the criterion the project's own for these kernels: assert_close(rtol = 5e-5,
atol_frac = 1e-6).  A failure names the build, the case, and the Gaussians (id = list position, quadrant) whose rows
miss.  The operands' seeds are fixed by conditions on the reference alone (backward_cases.OPERAND_SEED: the fp32 oracle
inside half the criterion at every channel count used here), never by what a kernel returned.

Which kernel a call runs is decided by gg_launch_blend2_bwd / gg_launch_blend2_bwd_pair (csrc/blend2.hip) and the
chunk plan of csrc/blend.hip (<= 3 remaining channels: the narrow kernel of that width; 4..8: narrow<8>; more: chunks
of 32 on the wide kernel); the rule is written beside each build below."""
import ctypes as C

import numpy as np
import pytest
import torch

import backward_cases as B

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL, ATOL_FRAC = 5e-5, 1e-6

# name -> (entry, channels, second array's channels, its cotangent parts, layout)
#   layout "off1": v_out one float off a 16-byte boundary; "rec": record of 6 + c2 floats; "rec16": merged-flush record
WIDE_BUILDS = {
    # chunk of 32 at offset 0, C % 4 == 0, colours and v_out 16-byte aligned -> <true, 0, 32, false, false, true> (S16)
    "single16_c32": ("single", 32, 0, (), ""),
    # v_out off alignment -> rows_aligned16 fails -> blend2_bwd_wide_kernel<true> (32 slots, full)
    "full32_c32_unaligned": ("single", 32, 0, (), "off1"),
    # C % 4 != 0 -> first chunk on blend2_bwd_wide_kernel<true>, the 3 remaining channels on narrow<3>
    "full32_c35": ("single", 35, 0, (), ""),
    # one chunk of width 32 with n = 12 <= 16 live channels -> <false, 0, 16>
    "partial16_c12": ("single", 12, 0, (), ""),
    # n = 17 > 16 -> <false, 0, 32>
    "partial32_c17": ("single", 17, 0, (), ""),
    # slab given, n == 32 -> <true, 0, 32, true>; n = 17 -> <false, 0, 32, true>
    "det_c32": ("det", 32, 0, (), ""),
    "det_c17": ("det", 17, 0, (), ""),
    # aligned rows, record of 6 + c2 floats (geom_stride != 16: not merged) -> <true, 0, 32, false, true, true>
    "pair16_c2_7": ("pair", 32, 7, (7,), "rec"),
    "pair16_c2_1": ("pair", 32, 1, (1,), "rec"),
    # 16-float record on a 64-byte boundary, v_conic = v_xy + 2, v_opacity = v_xy + 5, v_colors2 = v_xy + 6, both strides 16
    # -> the merged flush <true, 0, 32, false, true, true, true>
    "merged16_c2_7": ("pair", 32, 7, (7,), "rec16"),
    "merged16_c2_7_parts": ("pair", 32, 7, (3, 1, 3), "rec16"),
    "merged16_c2_3": ("pair", 32, 3, (3,), "rec16"),
    # first array's v_out off alignment -> <true, 0, 32, false, true> (pair, 32 slots)
    "pair32_unaligned": ("pair", 32, 7, (7,), "rec off1"),
}
NARROW_BUILDS = {
    "narrow_c1": ("single", 1, 0, (), ""),          # narrow<1>
    "narrow_c3": ("single", 3, 0, (), ""),          # narrow<3>
    # 4..8 channels go to narrow<8>, n live channels (the wide <false, 0, 8> build is never chosen: a chunk of width 32
    # has more than 8 channels left)
    "narrow8_c5": ("single", 5, 0, (), ""),
    "narrow8_c8": ("single", 8, 0, (), ""),
    "single16_c40_tail8": ("single", 40, 0, (), ""),     # aligned: S16 on channels 0..31, narrow<8> on 32..39
    "det_c3": ("det", 3, 0, (), ""),                # narrow<3, 0, true>
}
RUNS = [(b, c) for b in WIDE_BUILDS for c in B.WIDE_CASES] + [(b, c) for b in NARROW_BUILDS for c in B.NARROW_CASES]
BUILDS = {**WIDE_BUILDS, **NARROW_BUILDS}


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)       # (a copy: the shared arrays are read-only)


def _np(t):
    return t.detach().cpu().numpy()


def _off_by_one_float(a):
    """the array on the device, one float behind a 16-byte boundary"""
    buf = torch.empty(a.size + 8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[1:1 + a.size].view(a.shape)
    t.copy_(torch.from_numpy(np.array(a, order="C")))
    assert t.data_ptr() % 16 == 4
    return t


_SHARED = {}


def _case_data(oracle, name, channels, c2):
    """per (case, channel counts), computed once: operands, the fp32 forward's final_T / final_idx, the fp64 reference
    (two arrays: geometry gradients summed, as autograd would over two calls)"""
    key = (name, channels, c2)
    if key not in _SHARED:
        case = B.CASES[name]
        ids = B.ids_of(case)
        ft, fi = B.forward32(oracle, case, ids, case.tile_bins)
        colors, bg, v_out = B.operands(case, channels + c2)
        g = B.reference(oracle, case, colors[:, :channels], bg[:channels], v_out[..., :channels], ft, fi, ids=ids,
                        tile_bins=case.tile_bins)
        ref = {"v_xy": g[0], "v_conic": g[1], "v_colors": g[2], "v_opacity": g[3]}
        if c2:
            g2 = B.reference(oracle, case, colors[:, channels:], bg[channels:], v_out[..., channels:], ft, fi, ids=ids,
                             tile_bins=case.tile_bins)
            ref = {"v_xy": g[0] + g2[0], "v_conic": g[1] + g2[1], "v_colors": g[2], "v_opacity": g[3] + g2[3],
                   "v_colors2": g2[2]}
        for a in (ids, ft, fi, colors, bg, v_out, *ref.values()):
            a.setflags(write=False)
        _SHARED[key] = (ids, ft, fi, colors, bg, v_out, ref)
    return _SHARED[key]


class Call:
    def __init__(self, oracle, build, name):
        from gaussiangrasper_amd import _lib, ops as P
        self.entry, self.c, self.c2, self.parts, self.layout = BUILDS[build]
        self.lib, self._lib, self.p = _lib.load(), _lib, P._ptr
        self.case = case = B.CASES[name]
        self.n, self.h, self.w = len(case.order), case.h, case.w
        ids, ft, fi, colors, bg, v_out, self.ref = _case_data(oracle, name, self.c, self.c2)
        c = self.c
        self.ids, self.bins = _t(ids), _t(case.tile_bins)
        # the device call and the oracle walk the same lists
        assert np.array_equal(_np(self.ids), ids) and np.array_equal(_np(self.bins), case.tile_bins)
        assert self.ids.dtype == torch.int32 and self.bins.dtype == torch.int32 and int(self.bins[-1, 1]) == self.n
        self.xys, self.conics, self.opac = _t(case.xys), _t(case.conics), _t(case.opacity)
        self.col, self.bg = _t(colors[:, :c]), _t(bg[:c])
        self.fT, self.fi = _t(ft), _t(fi)
        first = np.ascontiguousarray(v_out[..., :c])
        self.v1 = _off_by_one_float(first) if "off1" in self.layout else _t(first)
        if "off1" not in self.layout:
            assert self.v1.data_ptr() % 16 == 0
        assert self.col.data_ptr() % 16 == 0
        if self.c2:
            self.col2, self.bg2 = _t(colors[:, c:]), _t(bg[c:])
            second, at = v_out[..., c:], np.cumsum((0,) + self.parts)
            assert at[-1] == self.c2
            self.v2 = [_t(second[..., a:b]) for a, b in zip(at[:-1], at[1:])]
        self.ws = torch.empty(self.lib.gg_blend_workspace(self.n), dtype=torch.uint8, device=DEV)
        self.stream = P._stream(self.xys.device)

    def head(self, *channels):
        p = self.p
        return (*channels, self.n, self.h, self.w, p(self.ids), p(self.bins), p(self.xys), p(self.conics))

    def single(self, garbage=0xA5):
        """gg_blend_bwd / gg_blend_bwd_deterministic on dense, separate gradient arrays pre-filled with NaN"""
        p, n = self.p, self.n
        out = {"v_xy": torch.full((n, 2), np.nan, device=DEV), "v_conic": torch.full((n, 3), np.nan, device=DEV),
               "v_colors": torch.full((n, self.c), np.nan, device=DEV), "v_opacity": torch.full((n, 1), np.nan, device=DEV)}
        self.ws.fill_(garbage)
        args = (*self.head(self.c), p(self.col), p(self.opac), p(self.bg), p(self.fT), p(self.fi), p(self.v1),
                p(out["v_xy"]), p(out["v_conic"]), p(out["v_colors"]), p(out["v_opacity"]), 0, 0, p(self.ws),
                self.ws.numel(), 0)
        if self.entry == "det":
            det = torch.full((self.lib.gg_blend_bwd_deterministic_workspace(n, self.c, n),), garbage, dtype=torch.uint8,
                             device=DEV)
            st = self.lib.gg_blend_bwd_deterministic(*args, n, p(det), det.numel(), self.stream)
        else:
            st = self.lib.gg_blend_bwd(*args, self.stream)
        self._lib.check(st, self.entry)
        torch.cuda.synchronize()
        return {k: _np(v) for k, v in out.items()}

    def pair(self):
        """gg_blend_bwd_pair: the geometry and the second array's gradients in one record per Gaussian"""
        p, n, c2 = self.p, self.n, self.c2
        stride = 16 if "rec16" in self.layout else 6 + c2
        rec = torch.full((n, stride), np.nan, device=DEV)
        vcol = torch.full((n, 32), np.nan, device=DEV)
        if "rec16" in self.layout:
            assert rec.data_ptr() % 64 == 0
        self.ws.fill_(0xA5)
        parts = (C.c_void_p * len(self.v2))(*[t.data_ptr() for t in self.v2])
        chs = (C.c_int * len(self.v2))(*self.parts)
        st = self.lib.gg_blend_bwd_pair(*self.head(32, c2), p(self.col), p(self.col2), p(self.opac), p(self.bg),
                                        p(self.bg2), p(self.fT), p(self.fi), p(self.v1), parts, chs, len(self.v2),
                                        p(rec[:, 0:2]), p(rec[:, 2:5]), p(vcol), p(rec[:, 6:]), p(rec[:, 5:6]), stride, 0,
                                        stride, p(self.ws), self.ws.numel(), 0, self.stream)
        self._lib.check(st, "gg_blend_bwd_pair")
        torch.cuda.synchronize()
        r = _np(rec)
        assert not r[:, 6 + c2:].any(), "the record's padding is cleared and stays clear"
        return {"v_xy": r[:, 0:2], "v_conic": r[:, 2:5], "v_opacity": r[:, 5:6], "v_colors2": r[:, 6:6 + c2],
                "v_colors": _np(vcol)}

    def run(self):
        return self.pair() if self.entry == "pair" else self.single()


def _compare(build, case, got, ref):
    from test_gpu_parity import assert_close
    for what, r in ref.items():
        a = got[what].reshape(r.shape)
        try:
            assert_close(a, r, f"backward_batches.{build}.{what}", rtol=RTOL, atol_frac=ATOL_FRAC)
        except AssertionError as e:
            worst, ok = B.excess(a, r, RTOL, ATOL_FRAC)
            rows = np.flatnonzero(~ok.all(axis=1))
            rows = [(int(k), "tile %d quadrant %s" % (case.tile[k], "all" if case.broad[k] else case.order[k]))
                    for k in rows[:12]]
            raise AssertionError(f"{build} on {case.name}: {e}; {int((~ok.all(axis=1)).sum())} rows miss, the first "
                                 f"(id = list position, where): {rows}; designed survivors {case.counts}") from None


@pytest.mark.parametrize("build,name", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_backward_build_on_a_constructed_list(oracle, build, name):
    call = Call(oracle, build, name)
    got = call.run()
    _compare(build, call.case, got, call.ref)
    if name == "fin_inside_a_batch":
        # behind every pixel's final_idx nothing is walked: exact zeros, not small numbers
        for what, a in got.items():
            assert not a[B.FIN_LAST:].any(), f"{build}: {what} of entries behind every final_idx must be exactly 0"
        assert all(np.abs(call.ref[w][B.FIN_LAST - 1]).max() > 0 for w in got)        # ... and position 28 is blended
    if call.entry == "det":
        again = call.single(garbage=0x3C)
        for what, a in got.items():
            assert a.tobytes() == again[what].tobytes(), f"{build}: {what} differs between two calls"
