"""The host side of the blend entries (csrc/blend.hip), pinned through the C ABI: which regions of the gradient
arrays a backward call clears, which layouts it rejects, and which kernels every entry launches for a channel count.

Everything runs on 5 Gaussians whose tile lists are EMPTY (every tile range is [0, 0)), so the blend kernels walk
nothing and add nothing: what a backward call leaves in memory is exactly its zeroing.  The gradient arrays are carved
out of one device buffer pre-filled with a signalling-NaN bit pattern (the style of tests/test_adam_rows_layouts.py)
and the WHOLE buffer is compared, as uint32, with a literal map of zeroed / untouched words.

The launch counts are literals derived from the chunking rule in csrc/blend.hip: <= 3 remaining channels go to the
narrow kernel of that width, 4..8 to the 8-wide narrow kernel, anything wider is walked in chunks of 32 (a last
partial chunk included); a forward whose image rows are 16-byte aligned (C % 4 == 0 and an aligned out_img) takes up
to `chunk_blocks` (default 3) full 32-channel blocks per walk, and the exact pair walk 1, 2 or 4 blocks of the first
array (`pair_blocks`, default 1; the batched pair kernel always one)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x7FA5A5A5
WORDS = 1536
N = 5
WS_FROM_FORWARD, ACC_COLORS, ACC_GEOM = 1, 2, 4
INVALID_ARG = -1
# gg_prof ids (include/gg_raster.h): blend_prep 5; forward 10 + width index, backward 20 + width index, with widths
# {1, 3, 4, 8, 16, 32} -> 0..5; the pair walks 16 / 17
PREP, FWD1, FWD3, FWD8, FWD32, FWD_PAIR, BWD_PAIR, BWD1, BWD3, BWD8, BWD32 = 5, 10, 11, 13, 15, 16, 17, 20, 21, 23, 25
BLEND_IDS = (5, 10, 11, 12, 13, 14, 15, 16, 17, 20, 21, 22, 23, 24, 25)


def _p(t, words=0):
    return C.c_void_p(t.data_ptr() + 4 * words)


class Scene:
    """5 Gaussians over an h x w image whose tile lists are all empty"""

    def __init__(self, h=16, w=16):
        from gaussiangrasper_amd import _lib
        from gaussiangrasper_amd._call import stream
        self.lib, self.h, self.w = _lib.load(), h, w
        g = torch.Generator().manual_seed(7)
        self.xys = (torch.rand(N, 2, generator=g) * 16).to(DEV)
        self.conics = torch.tensor([[0.5, 0.0, 0.5]] * N, device=DEV)
        self.opacity = torch.full((N,), 0.5, device=DEV)
        self.ids = torch.zeros(8, dtype=torch.int32, device=DEV)
        ntiles = ((h + 15) // 16) * ((w + 15) // 16)
        self.bins = torch.zeros(ntiles, 2, dtype=torch.int32, device=DEV)
        self.ws = torch.empty(max(int(self.lib.gg_blend_workspace(N)), 256), dtype=torch.uint8, device=DEV)
        self.final_Ts = torch.ones(h, w, device=DEV)
        self.final_idx = torch.zeros(h, w, dtype=torch.int32, device=DEV)
        self.stream = stream(torch.device(DEV))
        self._colors = {}

    def colors(self, c):
        """(colours, background, cotangent) of a c-channel array"""
        if c not in self._colors:
            g = torch.Generator().manual_seed(c)
            self._colors[c] = (torch.rand(N, c, generator=g).to(DEV), torch.rand(c, generator=g).to(DEV),
                               torch.zeros(self.h, self.w, c, device=DEV))
        return self._colors[c]

    def head(self, *channels):
        return (*channels, N, self.h, self.w, _p(self.ids), _p(self.bins))

    def workspace(self):
        return (_p(self.ws), self.ws.numel())


@pytest.fixture(scope="module")
def scene():
    return Scene()


class SentinelBuffer:
    def __init__(self):
        self.t = torch.full((WORDS,), SENTINEL, dtype=torch.int32, device=DEV)
        assert self.t.data_ptr() % 64 == 0

    def at(self, word):
        return _p(self.t, word)

    def check(self, zeroed, what):
        """the whole buffer: 0 in the `zeroed` ranges [(first word, words)], the sentinel everywhere else"""
        want = np.full(WORDS, SENTINEL, np.uint32)
        for first, words in zeroed:
            assert want[first:first + words].size == words
            want[first:first + words] = 0
        torch.cuda.synchronize()
        got = self.t.cpu().numpy().view(np.uint32)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "%s: %d words differ, first at word %d: got %#010x want %#010x" % (
            what, bad.size, bad[0], got[bad[0]], want[bad[0]])


# ------------------------------------------------------------------------------------------------
# (a) zeroing: gg_blend_bwd / gg_blend_bwd_deterministic
# ------------------------------------------------------------------------------------------------
# name -> f(C) = (word offsets of v_xy, v_conic, v_colors, v_opacity; geom_stride, color_stride;
#                 the words the call clears for the geometry; the words it clears for the colours)
# Without flags both sets are cleared, GG_BWD_ACCUMULATE_COLORS keeps the colour set, GG_BWD_ACCUMULATE_GEOM the
# geometry set (colours inside the record belong to it).
SINGLE_LAYOUTS = {
    "dense_separate": lambda c: ((64, 96, 160, 128), 0, 0, [(64, 10), (96, 15), (128, 5)], [(160, 5 * c)]),
    "dense_back_to_back": lambda c: ((64, 74, 94, 89), 0, 0, [(64, 30)], [(94, 5 * c)]),
    # rows of C + 5 floats: the padding is cleared with the rows, the last row's included
    "dense_padded_rows": lambda c: ((64, 96, 160, 128), 0, c + 5, [(64, 10), (96, 15), (128, 5)], [(160, 5 * c + 25)]),
    "record_6": lambda c: ((64, 66, 512, 69), 6, 0, [(64, 30)], [(512, 5 * c)]),
    "record_8": lambda c: ((64, 66, 512, 69), 8, 0, [(64, 40)], [(512, 5 * c)]),
    "record_16": lambda c: ((64, 66, 512, 69), 16, 0, [(64, 80)], [(512, 5 * c)]),
    # colours at floats 6.. of a record of 16 (C = 3) / 48 (C = 35) floats
    "colors_in_record": lambda c: ((64, 66, 70, 69), 16 if c == 3 else 48, 16 if c == 3 else 48,
                                   [(64, 80 if c == 3 else 240)], []),
}
FLAG_SETS = {"none": 0, "acc_colors": ACC_COLORS, "acc_geom": ACC_GEOM, "both": ACC_COLORS | ACC_GEOM}


def _bwd(scene, buf, entry, c, offsets, gstride, cstride, flags):
    lib = scene.lib
    col, bg, v_out = scene.colors(c)
    xy, conic, colors, opac = offsets
    args = (*scene.head(c), _p(scene.xys), _p(scene.conics), _p(col), _p(scene.opacity), _p(bg), _p(scene.final_Ts),
            _p(scene.final_idx), _p(v_out), buf.at(xy), buf.at(conic), buf.at(colors), buf.at(opac), gstride, cstride,
            *scene.workspace(), flags)
    if entry == "bwd":
        return lib.gg_blend_bwd(*args, scene.stream)
    return lib.gg_blend_bwd_deterministic(*args, 0, None, 0, scene.stream)


@pytest.mark.parametrize("c", [3, 35])
@pytest.mark.parametrize("entry", ["bwd", "deterministic"])
@pytest.mark.parametrize("layout", list(SINGLE_LAYOUTS))
def test_backward_clears_exactly_these_words(scene, layout, entry, c):
    offsets, gstride, cstride, geom, colors = SINGLE_LAYOUTS[layout](c)
    for name, flags in FLAG_SETS.items():
        buf = SentinelBuffer()
        st = _bwd(scene, buf, entry, c, offsets, gstride, cstride, flags)
        what = f"{layout}, {entry}, C = {c}, flags {name}"
        if layout == "colors_in_record" and flags & ACC_COLORS:
            assert st == INVALID_ARG, what
            assert b"GG_BWD_ACCUMULATE_COLORS needs v_colors outside" in scene.lib.gg_last_error()
            buf.check([], what)
            continue
        assert st == 0, (what, scene.lib.gg_last_error())
        buf.check((geom if not flags & ACC_GEOM else []) + (colors if not flags & ACC_COLORS else []), what)


# (offsets of v_xy, v_conic, v_colors, v_opacity; geom_stride; color_stride as a function of C; text of the message)
SINGLE_REJECTED = {
    "conic_misplaced": ((64, 67, 512, 69), 8, lambda c: 0, b"v_conic = v_xy + 2 and v_opacity = v_xy + 5 expected"),
    "opacity_misplaced": ((64, 66, 512, 70), 8, lambda c: 0, b"v_conic = v_xy + 2 and v_opacity = v_xy + 5 expected"),
    "geom_stride_5": ((64, 66, 512, 69), 5, lambda c: 0, b"geom_stride must be 0 (dense) or >= 6"),
    "geom_stride_negative": ((64, 96, 160, 128), -1, lambda c: 0, b"geom_stride must be 0 (dense) or >= 6"),
    "color_stride_short": ((64, 96, 160, 128), 0, lambda c: c - 1, b"color_stride must be 0 (dense) or >= channels"),
}


@pytest.mark.parametrize("c", [3, 35])
@pytest.mark.parametrize("entry", ["bwd", "deterministic"])
@pytest.mark.parametrize("case", list(SINGLE_REJECTED))
def test_backward_rejects_these_layouts_and_writes_nothing(scene, case, entry, c):
    offsets, gstride, cstride, text = SINGLE_REJECTED[case]
    for name, flags in FLAG_SETS.items():
        buf = SentinelBuffer()
        assert _bwd(scene, buf, entry, c, offsets, gstride, cstride(c), flags) == INVALID_ARG, (case, name)
        assert text in scene.lib.gg_last_error(), (case, name, scene.lib.gg_last_error())
        buf.check([], f"{case}, {entry}, C = {c}, flags {name}")


def test_backward_status_of_a_short_workspace_and_a_null_pointer(scene):
    lib = scene.lib
    col, bg, v_out = scene.colors(3)
    buf = SentinelBuffer()
    args = [*scene.head(3), _p(scene.xys), _p(scene.conics), _p(col), _p(scene.opacity), _p(bg), _p(scene.final_Ts),
            _p(scene.final_idx), _p(v_out), buf.at(64), buf.at(96), buf.at(160), buf.at(128), 0, 0, _p(scene.ws), 16, 0]
    assert lib.gg_blend_bwd(*args, scene.stream) == -3 and b"workspace too small" in lib.gg_last_error()
    args[-2] = scene.ws.numel()
    args[10] = None                                   # background
    assert lib.gg_blend_bwd(*args, scene.stream) == INVALID_ARG and b"null pointer" in lib.gg_last_error()
    buf.check([], "rejected calls")


# ------------------------------------------------------------------------------------------------
# (a) zeroing: gg_blend_bwd_pair, C = 32, C2 = 7; the first array's gradient rows sit at word 768
# ------------------------------------------------------------------------------------------------
# name -> (offsets of v_xy, v_conic, v_colors2, v_opacity; geom_stride, color_stride, color_stride2;
#          words cleared whatever the flags; words cleared unless GG_BWD_ACCUMULATE_COLORS)
PAIR_LAYOUTS = {
    "dense_second_outside": ((64, 96, 160, 128), 0, 0, 0, [(64, 10), (96, 15), (128, 5), (160, 35)], [(768, 160)]),
    "dense_second_padded_rows": ((64, 96, 160, 128), 0, 40, 8, [(64, 10), (96, 15), (128, 5), (160, 40)], [(768, 200)]),
    "record_16_second_inside": ((64, 66, 70, 69), 16, 0, 16, [(64, 80)], [(768, 160)]),
    "record_13_second_inside": ((64, 66, 70, 69), 13, 0, 13, [(64, 65)], [(768, 160)]),
    "record_8_second_outside": ((64, 66, 160, 69), 8, 0, 0, [(64, 40), (160, 35)], [(768, 160)]),
    "record_16_second_outside_rows_of_16": ((64, 66, 160, 69), 16, 0, 16, [(64, 80), (160, 80)], [(768, 160)]),
}


def _bwd_pair(scene, buf, offsets, gstride, cstride, cstride2, flags, channels=(7,), c=32, c2=7):
    col, bg, v_out = scene.colors(c)
    col2, bg2, _ = scene.colors(c2)
    cots = [torch.zeros(scene.h, scene.w, k, device=DEV) for k in channels]
    parts = (C.c_void_p * len(cots))(*[t.data_ptr() for t in cots])
    chs = (C.c_int * len(cots))(*channels)
    xy, conic, colors2, opac = offsets
    st = scene.lib.gg_blend_bwd_pair(*scene.head(c, c2), _p(scene.xys), _p(scene.conics), _p(col), _p(col2),
                                     _p(scene.opacity), _p(bg), _p(bg2), _p(scene.final_Ts), _p(scene.final_idx),
                                     _p(v_out), parts, chs, len(cots), buf.at(xy), buf.at(conic), buf.at(768),
                                     buf.at(colors2), buf.at(opac), gstride, cstride, cstride2, *scene.workspace(),
                                     flags, scene.stream)
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("layout", list(PAIR_LAYOUTS))
def test_pair_backward_clears_exactly_these_words(scene, layout):
    offsets, gstride, cstride, cstride2, always, colors = PAIR_LAYOUTS[layout]
    for name, flags in FLAG_SETS.items():
        for parts in ((7,), (3, 1, 3)):
            buf = SentinelBuffer()
            st = _bwd_pair(scene, buf, offsets, gstride, cstride, cstride2, flags, parts)
            what = f"{layout}, flags {name}, parts {parts}"
            if flags & ACC_GEOM:
                assert st == INVALID_ARG and b"writes the geometry gradients itself" in scene.lib.gg_last_error(), what
                buf.check([], what)
            else:
                assert st == 0, (what, scene.lib.gg_last_error())
                buf.check(always + (colors if not flags & ACC_COLORS else []), what)


# (offsets; geom_stride, color_stride, color_stride2; channels of the cotangent parts; text of the message)
PAIR_REJECTED = {
    "record_too_short": ((64, 66, 70, 69), 12, 0, 12, (7,), b"the record is too short for the second array's gradients"),
    "conic_misplaced": ((64, 67, 160, 69), 16, 0, 0, (7,), b"v_conic = v_xy + 2 and v_opacity = v_xy + 5 expected"),
    "opacity_misplaced": ((64, 66, 160, 68), 16, 0, 0, (7,), b"v_conic = v_xy + 2 and v_opacity = v_xy + 5 expected"),
    "geom_stride_5": ((64, 66, 160, 69), 5, 0, 0, (7,), b"geom_stride must be 0 (dense) or >= 6"),
    "color_stride_short": ((64, 96, 160, 128), 0, 31, 0, (7,), b"color_stride must be 0 (dense) or >= channels"),
    "color_stride2_short": ((64, 96, 160, 128), 0, 0, 6, (7,), b"color_stride2 must be 0 (dense) or >= channels2"),
    "parts_add_up_to_6": ((64, 96, 160, 128), 0, 0, 0, (3, 3), b"must add up to channels2"),
    "parts_add_up_to_8": ((64, 96, 160, 128), 0, 0, 0, (3, 1, 4), b"must add up to channels2"),
}


@pytest.mark.parametrize("case", list(PAIR_REJECTED))
def test_pair_backward_rejects_these_calls_and_writes_nothing(scene, case):
    offsets, gstride, cstride, cstride2, parts, text = PAIR_REJECTED[case]
    for name, flags in (("none", 0), ("acc_colors", ACC_COLORS)):
        buf = SentinelBuffer()
        assert _bwd_pair(scene, buf, offsets, gstride, cstride, cstride2, flags, parts) == INVALID_ARG, (case, name)
        assert text in scene.lib.gg_last_error(), (case, name, scene.lib.gg_last_error())
        buf.check([], f"{case}, flags {name}")


# ------------------------------------------------------------------------------------------------
# (b) which kernels run
# ------------------------------------------------------------------------------------------------
def _launches(lib, call):
    """{gg_prof id: launches} of the blend kernels that `call` starts (ids without a launch left out)"""
    lib.gg_prof_reset()
    lib.gg_prof_enable(1)
    try:
        st = call()
    finally:
        lib.gg_prof_enable(0)
    assert st == 0, lib.gg_last_error()
    torch.cuda.synchronize()
    out = {}
    for k in BLEND_IDS:
        n = C.c_int(0)
        assert lib.gg_prof_get(k, C.byref(n), None) == 0
        if n.value:
            out[k] = n.value
    lib.gg_prof_reset()
    return out


def _fwd(scene, c, misalign=0):
    col, bg, _ = scene.colors(c)
    img = torch.empty(scene.h * scene.w * c + 4, device=DEV)
    assert img.data_ptr() % 16 == 0
    return scene.lib.gg_blend_fwd(*scene.head(c), _p(scene.xys), _p(scene.conics), _p(col), _p(scene.opacity), _p(bg),
                                  _p(img, misalign), _p(scene.final_Ts), _p(scene.final_idx), *scene.workspace(),
                                  scene.stream), img


# C -> launches of gg_blend_fwd with 16-byte aligned rows (chunk_blocks 3) / with out_img one float off (one block
# per walk); where C % 4 != 0 the rows are never aligned and the two agree
FWD_LAUNCHES = {
    1: ({PREP: 1, FWD1: 1},) * 2,
    2: ({PREP: 1, FWD3: 1},) * 2,
    3: ({PREP: 1, FWD3: 1},) * 2,
    4: ({PREP: 1, FWD8: 1},) * 2,
    8: ({PREP: 1, FWD8: 1},) * 2,
    9: ({PREP: 1, FWD32: 1},) * 2,
    32: ({PREP: 1, FWD32: 1},) * 2,
    33: ({PREP: 1, FWD32: 1, FWD1: 1},) * 2,
    35: ({PREP: 1, FWD32: 1, FWD3: 1},) * 2,
    40: ({PREP: 1, FWD32: 1, FWD8: 1},) * 2,
    64: ({PREP: 1, FWD32: 1}, {PREP: 1, FWD32: 2}),             # one walk of 2 blocks / 2 walks
    96: ({PREP: 1, FWD32: 1}, {PREP: 1, FWD32: 3}),             # one walk of 3 blocks / 3 walks
    128: ({PREP: 1, FWD32: 2}, {PREP: 1, FWD32: 4}),            # 3 blocks + 1 block / 4 walks
    135: ({PREP: 1, FWD32: 4, FWD8: 1},) * 2,
    160: ({PREP: 1, FWD32: 2}, {PREP: 1, FWD32: 5}),            # 3 blocks + 2 blocks / 5 walks
}


@pytest.mark.parametrize("c", list(FWD_LAUNCHES))
def test_forward_launches_per_channel_count(scene, c):
    aligned, misaligned = FWD_LAUNCHES[c]
    assert _launches(scene.lib, lambda: _fwd(scene, c)[0]) == aligned
    assert _launches(scene.lib, lambda: _fwd(scene, c, misalign=1)[0]) == misaligned


def _fwd_pair(scene, entry, c, c2=7):
    lib = scene.lib
    col, bg, _ = scene.colors(c)
    col2, bg2, _ = scene.colors(c2)
    img, img2 = torch.empty(scene.h, scene.w, c, device=DEV), torch.empty(scene.h, scene.w, c2, device=DEV)
    assert img.data_ptr() % 16 == 0 and bg.data_ptr() % 16 == 0
    outs = (_p(img), _p(img2), _p(scene.final_Ts), _p(scene.final_idx), *scene.workspace())
    if entry.startswith("packed"):
        st = lib.gg_blend_fwd_pair_packed(*scene.head(c, c2), _p(col), _p(col2), _p(bg), _p(bg2), *outs,
                                          int(entry == "packed_fast"), scene.stream)
    else:
        fn = lib.gg_blend_fwd_pair_fast if entry == "fast" else lib.gg_blend_fwd_pair
        st = fn(*scene.head(c, c2), _p(scene.xys), _p(scene.conics), _p(col), _p(col2), _p(scene.opacity), _p(bg),
                _p(bg2), *outs, scene.stream)
    return st, img, img2


# (pair_blocks, chunk_blocks) -> C -> launches behind the pair walk of the exact kernel / of the batched kernel (which
# always takes one block; C % 4 != 0 falls back to the exact kernel, whose rows are then unaligned as well)
PAIR_FWD_LAUNCHES = {
    (1, 3): {32: ({},) * 2, 33: ({FWD1: 1},) * 2, 64: ({FWD32: 1},) * 2, 128: ({FWD32: 1},) * 2,     # 1 | 3 blocks
             135: ({FWD32: 3, FWD8: 1},) * 2},
    (2, 2): {32: ({},) * 2, 33: ({FWD1: 1},) * 2, 64: ({}, {FWD32: 1}),           # pair walk of 2 | 1 + 1
             128: ({FWD32: 1}, {FWD32: 2}),                                      # 2 + 2 | 1 + 2 + 1
             135: ({FWD32: 3, FWD8: 1},) * 2},
    (4, 4): {32: ({},) * 2, 33: ({FWD1: 1},) * 2, 64: ({}, {FWD32: 1}),           # pair walk of 2 | 1 + 1
             128: ({}, {FWD32: 1}),                                              # pair walk of 4 | 1 + 3
             135: ({FWD32: 3, FWD8: 1},) * 2},
}


@pytest.mark.parametrize("c", [32, 33, 64, 128, 135])
@pytest.mark.parametrize("policy", list(PAIR_FWD_LAUNCHES), ids=lambda p: "blocks%d_%d" % p)
def test_pair_forward_launches_per_channel_count_and_block_policy(scene, policy, c):
    lib = scene.lib
    exact, batched = PAIR_FWD_LAUNCHES[policy][c]
    try:
        lib.gg_debug_set_fwd_blocks(*policy)
        for entry, prep, behind in (("exact", 1, exact), ("fast", 1, batched), ("packed_exact", 0, exact),
                                    ("packed_fast", 0, batched)):
            want = {FWD_PAIR: 1, **behind, **({PREP: 1} if prep else {})}
            assert _launches(lib, lambda: _fwd_pair(scene, entry, c)[0]) == want, entry
    finally:
        lib.gg_debug_set_fwd_blocks(1, 3)      # the library's defaults (csrc/blend.hip)


# C -> launches of the backward walks of gg_blend_bwd: one chunk each, whatever the alignment
BWD_LAUNCHES = {1: {BWD1: 1}, 2: {BWD3: 1}, 3: {BWD3: 1}, 4: {BWD8: 1}, 8: {BWD8: 1}, 9: {BWD32: 1}, 32: {BWD32: 1},
                33: {BWD32: 1, BWD1: 1}, 35: {BWD32: 1, BWD3: 1}, 40: {BWD32: 1, BWD8: 1}, 64: {BWD32: 2},
                96: {BWD32: 3}, 128: {BWD32: 4}, 135: {BWD32: 4, BWD8: 1}, 160: {BWD32: 5}}
# C -> launches behind the pair walk of gg_blend_bwd_pair (channels [32, C) of the first array)
PAIR_BWD_LAUNCHES = {32: {}, 33: {BWD1: 1}, 64: {BWD32: 1}, 128: {BWD32: 3}, 135: {BWD32: 3, BWD8: 1}}


@pytest.mark.parametrize("c", list(BWD_LAUNCHES))
def test_backward_launches_per_channel_count(scene, c):
    grads = torch.empty(N * (6 + c), device=DEV)
    offsets = (0, 2 * N, 6 * N, 5 * N)

    class Plain:
        at = staticmethod(lambda word: _p(grads, word))
    for flags, prep in ((0, {PREP: 1}), (WS_FROM_FORWARD, {})):
        got = _launches(scene.lib, lambda: _bwd(scene, Plain, "bwd", c, offsets, 0, 0, flags))
        assert got == {**BWD_LAUNCHES[c], **prep}, flags
        assert not grads.any()


@pytest.mark.parametrize("c", list(PAIR_BWD_LAUNCHES))
def test_pair_backward_launches_per_channel_count(scene, c):
    for flags, prep in ((0, {PREP: 1}), (WS_FROM_FORWARD, {})):
        buf = SentinelBuffer()      # first array's rows: 5 * c <= 675 words from word 768
        got = _launches(scene.lib, lambda: _bwd_pair(scene, buf, (64, 66, 70, 69), 16, 0, 16, flags, (3, 1, 3), c=c))
        assert got == {BWD_PAIR: 1, **PAIR_BWD_LAUNCHES[c], **prep}, flags
        buf.check([(64, 80), (768, 5 * c)], f"C = {c}")


def test_ragged_image_of_two_by_three_tiles():
    """17 x 33 pixels = 2 x 3 tiles, the last row and column of tiles ragged: every pixel of every tile is written (the
    background, final_T = 1, final_idx = 0) by the single-array and by the exact pair forward, with the launches of the
    one-tile image; the backward over the same grid clears its arrays and adds nothing."""
    scene = Scene(17, 33)
    lib = scene.lib
    scene.final_Ts.fill_(-1.0)
    scene.final_idx.fill_(-1)
    assert _launches(lib, lambda: _fwd(scene, 35)[0]) == FWD_LAUNCHES[35][0]
    st, img = _fwd(scene, 35)
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(img[:17 * 33 * 35].view(17, 33, 35), scene.colors(35)[1].expand(17, 33, 35))
    assert (scene.final_Ts == 1).all() and (scene.final_idx == 0).all()
    scene.final_Ts.fill_(-1.0)
    scene.final_idx.fill_(-1)
    st, img, img2 = _fwd_pair(scene, "exact", 33)
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(img, scene.colors(33)[1].expand(17, 33, 33))
    assert torch.equal(img2, scene.colors(7)[1].expand(17, 33, 7))
    assert (scene.final_Ts == 1).all() and (scene.final_idx == 0).all()
    buf = SentinelBuffer()
    got = _launches(lib, lambda: _bwd_pair(scene, buf, (64, 66, 70, 69), 16, 0, 16, 0, (7,), c=33))
    assert got == {PREP: 1, BWD_PAIR: 1, BWD1: 1}
    buf.check([(64, 80), (768, 165)], "17 x 33")
