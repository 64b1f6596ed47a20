"""SURVEY 8f-3, second file: fused Adam and the row kernels on the layouts tests/test_densify_adam.py does not
reach — several groups in one launch with ragged quads and a zero-length group, arrays that are 4-byte but not
16-byte aligned (the scalar branch of adam_kernel), the second pass of the grid-stride loop, value edges of the
Adam element, more than 8 Adam entries / more than 24 row arrays through the Python wrappers, and destinations
that are exactly as long as the result.

Everything the C ABI reads or writes sits in ONE flat device buffer (`GuardBuffer`) that is filled with a
signalling-NaN sentinel; after the call the WHOLE buffer is compared, as uint32, with a host image: the expected
contents where arrays sit (inputs that must not change included), the sentinel everywhere else.  A float written
one past the end of an array therefore fails, whoever owns the allocation's slack.

References: the CPU oracle for the GPU tests (bit for bit, NaNs as NaN-ness); torch.optim.Adam and numpy indexing
for the oracle (CPU tests below).  Never the kernel's own output."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from test_densify_adam import _params, _ulp_diff, torch_dup_in_optim, torch_split_dup

DEV = "cuda:0"
gpu = pytest.mark.gpu

# A SIGNALLING NaN with a recognisable payload: arithmetic quiets it (bit 22 set), so a kernel that loads a guard word,
# pushes it through the Adam element and stores it back changes the word and is caught; a quiet NaN would come back
# bit-identical from such a read-modify-write.
SENTINEL = 0x7FA5A5A5
GUARD = 8                   # sentinel floats before and after every array, at least


# ------------------------------------------------------------------------------------------------
# the guard-band buffer (host-side bookkeeping is tested on the CPU below)
# ------------------------------------------------------------------------------------------------
class Region:
    def __init__(self, name, start, nbytes):
        self.name, self.start, self.nbytes = name, start, nbytes     # start in 4-byte words, from a 16-byte boundary

    @property
    def words(self):
        return -(-self.nbytes // 4)


class GuardBuffer:
    """Layout of arrays inside one flat fp32 buffer whose base is 16-byte aligned.  `place(name, data, offset)` puts
    the bytes of `data` at a word index that is `offset` (0..3) floats past a 16-byte boundary, at least GUARD
    sentinel words after the previous array; `finish()` adds the trailing guard.  `image` is the host copy (uint32)."""

    def __init__(self):
        self.regions, self._data, self._cursor, self.image, self.dev = [], [], 0, None, None

    def place(self, name, data, offset=0):
        assert self.image is None and 0 <= offset < 4
        raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        start = self._cursor + GUARD
        start += (offset - start) % 4
        r = Region(name, start, raw.size)
        self.regions.append(r)
        self._data.append(raw.copy())
        self._cursor = start + r.words
        return r

    def reserve(self, name, nwords, offset=0):
        """an output-only array: it starts as sentinels, so an element the kernel skips shows as well"""
        return self.place(name, np.full(nwords, SENTINEL, np.uint32), offset)

    def finish(self):
        total = self._cursor + GUARD
        total += (-total) % 4
        self.image = np.full(total, SENTINEL, np.uint32)
        for r, raw in zip(self.regions, self._data):
            self.image.view(np.uint8)[4 * r.start:4 * r.start + r.nbytes] = raw
        return self.image

    # -- host image access ----------------------------------------------------------------------
    @staticmethod
    def put(image, region, data):
        raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        assert raw.size == region.nbytes, (region.name, raw.size, region.nbytes)
        image.view(np.uint8)[4 * region.start:4 * region.start + region.nbytes] = raw

    @staticmethod
    def get(image, region, dtype=np.float32):
        return image.view(np.uint8)[4 * region.start:4 * region.start + region.nbytes].view(dtype).copy()

    def where(self, word):
        for r in self.regions:
            if r.start <= word < r.start + r.words:
                return f"{r.name}[{word - r.start}]"
        near = min(self.regions, key=lambda r: min(abs(word - r.start), abs(word - (r.start + r.words - 1))))
        d = word - near.start if word < near.start else word - (near.start + near.words - 1)
        return f"guard band, {d:+d} from {near.name}"

    def compare(self, got, want, nan_words=None, loose_words=None):
        """got == want word for word; `nan_words` (bool image): the reference holds a NaN there and any NaN will do;
        `loose_words`: compared by the caller with a tolerance of its own, skipped here."""
        assert got.shape == want.shape == self.image.shape
        bad = got != want
        if nan_words is not None:
            bad &= ~(nan_words & np.isnan(got.view(np.float32)))
        if loose_words is not None:
            bad &= ~loose_words
        idx = np.nonzero(bad)[0]
        assert idx.size == 0, "%d words differ: %s" % (idx.size, "; ".join(
            f"{self.where(int(i))} got {int(got[i]):#010x} want {int(want[i]):#010x}" for i in idx[:6]))

    # -- device side ----------------------------------------------------------------------------
    def upload(self, dev=DEV):
        if self.image is None:
            self.finish()
        self.dev = torch.empty(self.image.size, dtype=torch.float32, device=dev)
        assert self.dev.data_ptr() % 16 == 0
        self.dev.view(torch.int32).copy_(torch.from_numpy(self.image.view(np.int32)))
        return self

    def ptr(self, region):
        return self.dev.data_ptr() + 4 * region.start

    def download(self):
        torch.cuda.synchronize()
        return self.dev.view(torch.int32).cpu().numpy().view(np.uint32)


def test_guard_buffer_bookkeeping():
    gb = GuardBuffer()
    rng = np.random.default_rng(0)
    specs = [("a", rng.standard_normal(5).astype(np.float32), 0), ("b", rng.standard_normal(4).astype(np.float32), 1),
             ("empty", np.zeros(0, np.float32), 3), ("mask", np.arange(1, 6, dtype=np.uint8), 2),
             ("cnt", np.array([7], np.int64), 2), ("c", rng.standard_normal(1).astype(np.float32), 3)]
    regs = [gb.place(n, d, o) for n, d, o in specs]
    out = gb.reserve("out", 3, 1)
    img = gb.finish()
    assert img.dtype == np.uint32 and img.size % 4 == 0
    covered = np.zeros(img.size, bool)
    prev_end = 0
    for r, (n, d, o) in zip(regs + [out], specs + [("out", np.full(3, SENTINEL, np.uint32), 1)]):
        assert r.start % 4 == o and r.start - prev_end >= GUARD, n
        assert not covered[r.start:r.start + r.words].any()
        covered[r.start:r.start + r.words] = True
        assert np.array_equal(GuardBuffer.get(img, r, d.dtype), d.reshape(-1)), n
        prev_end = r.start + r.words
    assert img.size - prev_end >= GUARD
    # the bytes of the mask's last word that the mask does not own are sentinel bytes, like every uncovered word
    assert img[regs[3].start + 1] == ((SENTINEL & 0xFFFFFF00) | 5)
    hole = covered.copy()
    hole[regs[3].start + 1] = True
    assert (img[~hole] == SENTINEL).all()
    assert GuardBuffer.get(img, regs[4], np.int64)[0] == 7
    assert np.isnan(np.array([SENTINEL], np.uint32).view(np.float32))[0] and not SENTINEL & 0x00400000
    # compare: equal images pass; one word past an array, one word inside an array and a NaN with another payload
    # fail, each named by where it is; nan_words lets any NaN through and nothing else
    gb.compare(img.copy(), img)
    for word, where in ((regs[0].start + 5, "guard band, +1 from a"), (regs[1].start - 1, "guard band, -1 from b"),
                        (regs[1].start + 2, "b[2]")):
        got = img.copy()
        got[word] = 0
        with pytest.raises(AssertionError, match=re.escape(where)):
            gb.compare(got, img)
    want = img.copy()
    GuardBuffer.put(want, regs[0], np.array([1, np.nan, 3, 4, 5], np.float32))
    got = want.copy()
    got[regs[0].start + 1] = 0xFFC00001
    nan_words = np.zeros(img.size, bool)
    with pytest.raises(AssertionError, match=r"a\[1\]"):
        gb.compare(got, want)
    nan_words[regs[0].start + 1] = True
    gb.compare(got, want, nan_words=nan_words)
    got[regs[0].start + 1] = np.array([2.0], np.float32).view(np.uint32)[0]
    with pytest.raises(AssertionError, match=r"a\[1\]"):
        gb.compare(got, want, nan_words=nan_words)


# ------------------------------------------------------------------------------------------------
# Adam: data, special values, the oracle against torch.optim.Adam on them (CPU)
# ------------------------------------------------------------------------------------------------
def _adam_data(numel, seed):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(numel).astype(np.float32)
    g = (rng.standard_normal(numel) * 1e-2).astype(np.float32)
    m = (rng.standard_normal(numel) * 1e-3).astype(np.float32)
    v = (rng.random(numel) * 1e-5).astype(np.float32)
    return p, g, m, v


# (name, p, g, m, v); None keeps the plain random value of that element
_INF, _NAN = float("inf"), float("nan")
EDGE_CASES = [
    ("g0_v0_m", None, 0.0, 1.25e-3, 0.0),
    ("g0_v0_negm", None, 0.0, -3e-4, 0.0),
    ("g0_v0_m0", None, 0.0, 0.0, 0.0),
    ("g0_v0_m0_negzero", None, -0.0, -0.0, 0.0),
    ("denormal_g", None, 1e-40, None, None),
    ("denormal_negg_zero_state", None, -3e-41, 0.0, 0.0),
    ("smallest_denormal_g_zero_state", None, 1.4e-45, 0.0, 0.0),
    ("denormal_m_v", None, 1e-3, 2e-39, 5e-42),
    ("g_1e25", None, 1e25, None, None),
    ("g_neg1e25", None, -1e25, None, None),
    ("g_inf", None, _INF, None, None),
    ("g_neginf", None, -_INF, None, None),
    ("g_nan", None, _NAN, None, None),
    ("p_denormal", 7e-41, None, None, None),
    ("p_denormal_g0", -2e-39, 0.0, 0.0, 0.0),
]
EDGE_NUMEL = 4 * 3 * len(EDGE_CASES) + 4 + 3          # ragged: the last quad has three elements


def _edge_index(j):
    """case j sits in lane j % 4 of a quad whose other three lanes, and both neighbouring quads, are plain"""
    return 4 * (3 * j + 1) + j % 4


def _edge_data(seed):
    p, g, m, v = _adam_data(EDGE_NUMEL, seed)
    for j, (_, cp, cg, cm, cv) in enumerate(EDGE_CASES):
        i = _edge_index(j)
        for arr, val in ((p, cp), (g, cg), (m, cm), (v, cv)):
            if val is not None:
                arr[i] = np.float32(val)
    special = np.zeros(EDGE_NUMEL, bool)
    special[[_edge_index(j) for j in range(len(EDGE_CASES))]] = True
    return (p, g, m, v), special


# two hyper-parameter sets for the edges: the reference's eps without weight decay (g = 0 stays 0), and weight decay on
EDGE_HYPER = [dict(lr=1.6e-4, beta1=0.9, beta2=0.999, eps=1e-15, weight_decay=0.0, step=3),
              dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=3)]


def _classes(a):
    """0 finite, +1 / -1 the infinities, 2 NaN"""
    a = np.asarray(a, np.float32)
    c = np.zeros(a.shape, np.int8)
    c[np.isnan(a)], c[a == np.inf], c[a == -np.inf] = 2, 1, -1
    return c


def test_edge_data_places_each_case_in_its_own_quad():
    (p, g, m, v), special = _edge_data(0)
    assert int(special.sum()) == len(EDGE_CASES) and EDGE_NUMEL % 4 == 3
    quads = np.nonzero(special)[0] // 4
    assert len(set(quads)) == len(quads) and np.diff(np.sort(quads)).min() >= 2
    assert set(np.nonzero(special)[0] % 4) == {0, 1, 2, 3}
    for a in (p, m, v):
        assert np.isfinite(a).all()
    assert np.isfinite(g[~special]).all() and (np.abs(g[~special]) > 1e-30).all()
    # denormal inputs really are denormal in fp32, and no magnitude sits in the 1e18..1e20 band
    tiny = np.finfo(np.float32).tiny
    for name, cp, cg, cm, cv in EDGE_CASES:
        for val in (cp, cg, cm, cv):
            if val is not None and np.isfinite(val):
                assert not 1e18 <= abs(val) <= 1e20
        if "denormal" in name:
            assert any(val is not None and 0 < abs(np.float32(val)) < tiny for val in (cp, cg, cm, cv)), name


@pytest.mark.parametrize("hyper", EDGE_HYPER, ids=["eps1e-15", "weight_decay"])
def test_oracle_adam_matches_torch_optim_adam_on_the_value_edges(oracle, hyper):
    """oracle.adam_step against torch.optim.Adam(foreach=False) on the special values the GPU test uses: the same
    finite / +inf / -inf / NaN class per element of the parameter and both moments, and the finite results within
    the tolerances of test_oracle_adam_matches_torch_optim_adam (2 ulp on the moments, 4e-7 max(1, |p|) step on the
    parameter, here per element).  No value class is dropped."""
    (p, g, m, v), special = _edge_data(5)
    step = hyper["step"]
    ref = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([ref], lr=hyper["lr"], betas=(hyper["beta1"], hyper["beta2"]), eps=hyper["eps"],
                           weight_decay=hyper["weight_decay"], foreach=False)
    opt.state[ref] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m.copy()),
                      "exp_avg_sq": torch.from_numpy(v.copy())}
    ref.grad = torch.from_numpy(g.copy())
    opt.step()
    st = opt.state[ref]
    assert float(st["step"]) == step
    pn, mn, vn = oracle.adam_step(p, g, m, v, **hyper)
    tp, tm, tv = ref.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
    for name, a, b in (("param", pn, tp), ("exp_avg", mn, tm), ("exp_avg_sq", vn, tv)):
        ca, cb = _classes(a), _classes(b)
        wrong = np.nonzero(ca != cb)[0]
        assert wrong.size == 0, (name, [(int(i), float(a[i]), float(b[i])) for i in wrong[:5]])
    # every non-finite class occurs, so the classification above is not vacuous
    assert np.isnan(pn).any() and np.isinf(mn).any() and np.isinf(vn).any() and (np.isinf(vn) & ~np.isnan(pn)).any()
    fin = np.isfinite(mn) & np.isfinite(tm)
    assert _ulp_diff(mn[fin], tm[fin]).max() <= 2
    fin = np.isfinite(vn) & np.isfinite(tv)
    assert _ulp_diff(vn[fin], tv[fin]).max() <= 2
    fin = np.isfinite(pn) & np.isfinite(tp)
    err = np.abs(pn[fin].astype(np.float64) - tp[fin])
    assert (err <= 4e-7 * np.maximum(1.0, np.abs(pn[fin])) * step).all(), float(err.max())
    assert special[~fin].all()          # only special lanes may leave the finite set


# ------------------------------------------------------------------------------------------------
# GPU: gg_adam_step through the C ABI inside a guard buffer
# ------------------------------------------------------------------------------------------------
# floats past a 16-byte boundary of (param, grad, exp_avg, exp_avg_sq)
ALIGN_OFFSETS = [(0, 0, 0, 0), (0, 1, 0, 0), (0, 0, 0, 3), (1, 2, 3, 1), (2, 2, 2, 2)]


def _place_group(gb, tag, data, offsets):
    return [gb.place(f"{tag}.{n}", a, o) for n, a, o in zip(("param", "grad", "exp_avg", "exp_avg_sq"), data, offsets)]


def _adam_launch(gb, groups, zero_grad):
    """groups: [(regions or None, numel, hyper)]; None = a zero-length group with null pointers"""
    from gaussiangrasper_amd import _lib
    from gaussiangrasper_amd._call import stream
    lib = _lib.load()
    arr = (_lib.AdamGroup * len(groups))()
    for k, (regs, numel, h) in enumerate(groups):
        ptrs = [None] * 4 if regs is None else [gb.ptr(r) for r in regs]
        arr[k] = _lib.AdamGroup(*ptrs, numel, h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"], h["step"])
    _lib.check(lib.gg_adam_step(len(groups), arr, int(zero_grad), stream(gb.dev.device)), "gg_adam_step")


def _adam_expect(oracle, want, nan_words, regs, data, hyper, zero_grad):
    """writes the oracle's step of one group into the image `want`; marks where the oracle has a NaN"""
    p, g, m, v = data
    pn, mn, vn = oracle.adam_step(p, g, m, v, **hyper)
    for r, a in zip((regs[0], regs[2], regs[3]), (pn, mn, vn)):
        GuardBuffer.put(want, r, a)
        nan_words[r.start:r.start + r.words] = np.isnan(a)
    if zero_grad:
        GuardBuffer.put(want, regs[1], np.zeros(len(g), np.float32))      # +0.0, exactly numel of them


# eight hyper-parameter sets, all different in every field; step 1, and a step at which both bias corrections are 1
HYPER8 = [dict(lr=1.6e-4, beta1=0.9, beta2=0.999, eps=1e-15, weight_decay=0.0, step=1),
          dict(lr=5e-4, beta1=0.8, beta2=0.99, eps=1e-8, weight_decay=0.01, step=2),
          dict(lr=0.05, beta1=0.5, beta2=0.9, eps=1e-6, weight_decay=0.0, step=100_000),
          dict(lr=0.005, beta1=0.95, beta2=0.9995, eps=1e-10, weight_decay=0.1, step=7),
          dict(lr=0.001, beta1=0.0, beta2=0.95, eps=1e-12, weight_decay=0.0, step=33),
          dict(lr=0.02, beta1=0.85, beta2=0.98, eps=1e-7, weight_decay=0.003, step=4),
          dict(lr=3e-3, beta1=0.99, beta2=0.999, eps=1e-15, weight_decay=0.05, step=100_000),
          dict(lr=7e-5, beta1=0.7, beta2=0.97, eps=1e-9, weight_decay=0.0, step=12)]
NUMEL8 = (1, 2, 3, 4, 5, 0, 1027, 4099)


def test_hyper8_has_the_steps_the_group_test_needs():
    assert len({tuple(sorted(h.items())) for h in HYPER8}) == 8
    for key in ("lr", "beta1", "beta2", "eps", "step"):
        assert len({h[key] for h in HYPER8}) >= 7, key
    assert {h["weight_decay"] == 0.0 for h in HYPER8} == {True, False}
    assert any(h["step"] == 1 for h in HYPER8)
    big = [h for h in HYPER8 if np.float32(1.0 - h["beta1"] ** h["step"]) == 1 and
           np.float32(np.sqrt(1.0 - h["beta2"] ** h["step"])) == 1]
    assert len(big) == 2 and all(h["beta1"] > 0 for h in big)


@gpu
@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("order", ["zero_inside", "zero_first", "zero_last"])
def test_gpu_adam_eight_ragged_groups_in_one_launch(oracle, order, zero_grad):
    """numel (1, 2, 3, 4, 5, 0, 1027, 4099) in ONE gg_adam_step: every group but the last ends on a ragged quad that
    the next group follows, a zero-length group with null pointers sits inside / first / last, and every group has
    its own lr, betas, eps, weight_decay and step, so each result equals only the oracle run with ITS hyper-parameters.
    Alignments cycle through the matrix of the alignment test, so vector and scalar groups alternate.

    Mutation check (adam_kernel): `k = 0;` before `const AdamDev &grp = G.g[k];` (always pick group 0) — every
    group but the first keeps its input, so param / exp_avg / exp_avg_sq of the later groups differ from the oracle
    here: this test fails on "g1.param[0]"."""
    pairs = list(zip(NUMEL8, HYPER8))           # a group keeps its hyper-parameters wherever it stands
    if order != "zero_inside":
        empty = pairs.pop(NUMEL8.index(0))
        pairs.insert(0 if order == "zero_first" else len(pairs), empty)
    gb, groups, datas = GuardBuffer(), [], []
    for k, (numel, h) in enumerate(pairs):
        if numel == 0:
            groups.append((None, 0, h))
            datas.append(None)
            continue
        data = _adam_data(numel, 100 + k)
        groups.append((_place_group(gb, f"g{k}", data, ALIGN_OFFSETS[k % len(ALIGN_OFFSETS)]), numel, h))
        datas.append(data)
    gb.upload()
    _adam_launch(gb, groups, zero_grad)
    want, nan_words = gb.image.copy(), np.zeros(gb.image.size, bool)
    for (regs, numel, h), data in zip(groups, datas):
        if numel:
            _adam_expect(oracle, want, nan_words, regs, data, h, zero_grad)
    assert not nan_words.any()
    gb.compare(gb.download(), want)


ALIGN_NUMELS = (16, 17, 19, 3, 1)       # 4k, 4k + 1, 4k + 3 for k = 4; 3; 1


@gpu
@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("offsets", ALIGN_OFFSETS, ids=lambda o: "off%d%d%d%d" % o)
def test_gpu_adam_alignment_matrix(oracle, offsets, zero_grad):
    """One group per launch, the four arrays `offsets` floats past a 16-byte boundary: (0,0,0,0) takes the float4
    branch for whole quads and the scalar branch for the ragged tail, every other row of the matrix makes
    `grp.vec == 0` and takes the scalar branch throughout.  With zero_grad exactly numel gradient floats become +0.0,
    without it the gradient is bit-unchanged; both are part of the whole-buffer image.

    Mutation check (adam_kernel): `if (grp.vec && e0 + 4 <= grp.numel + 1)` — with offsets (0,0,0,0) and numel 19
    (and 3) the last quad is then loaded and stored as a float4: the sentinel after param / exp_avg / exp_avg_sq
    (and after grad with zero_grad) is overwritten, and this test fails on "guard band, +1 from n19.param"."""
    gb, launches = GuardBuffer(), []
    hyper = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=3)
    for numel in ALIGN_NUMELS:
        data = _adam_data(numel, 7 * numel + sum(offsets))
        launches.append((_place_group(gb, f"n{numel}", data, offsets), numel, data))
    gb.upload()
    want, nan_words = gb.image.copy(), np.zeros(gb.image.size, bool)
    for regs, numel, data in launches:
        assert all((gb.ptr(r) % 16) // 4 == o for r, o in zip(regs, offsets))
        _adam_launch(gb, [(regs, numel, hyper)], zero_grad)
        _adam_expect(oracle, want, nan_words, regs, data, hyper, zero_grad)
    gb.compare(gb.download(), want)


@gpu
@pytest.mark.parametrize("zero_grad", [0, 1])
def test_gpu_adam_aligned_and_misaligned_group_in_one_launch(oracle, zero_grad):
    """`vec` is per group: an all-aligned group (float4 branch) and misaligned ones (scalar branch) in one launch,
    in both orders"""
    gb, groups, datas = GuardBuffer(), [], []
    for k, (numel, offsets) in enumerate([(19, (0, 0, 0, 0)), (17, (1, 2, 3, 1)), (1031, (0, 0, 0, 0)),
                                          (1029, (0, 0, 0, 3)), (16, (0, 0, 0, 0))]):
        data = _adam_data(numel, 40 + k)
        groups.append((_place_group(gb, f"g{k}", data, offsets), numel, HYPER8[k + 1]))
        datas.append(data)
    gb.upload()
    _adam_launch(gb, groups, zero_grad)
    want, nan_words = gb.image.copy(), np.zeros(gb.image.size, bool)
    for (regs, numel, h), data in zip(groups, datas):
        _adam_expect(oracle, want, nan_words, regs, data, h, zero_grad)
    gb.compare(gb.download(), want)


GRID_NUMEL = 4 * 1_048_576 + 4 * 256 * 3 + 1


@gpu
@pytest.mark.parametrize("offsets", [(0, 0, 0, 0), (1, 2, 3, 1)], ids=["vector", "scalar"])
def test_gpu_adam_grid_stride_second_pass(oracle, offsets):
    """The grid is capped at 256 * 16 workgroups of 256 threads = 1 048 576 quads per pass.  One group of
    4 * 1 048 576 + 4 * 256 * 3 + 1 elements followed by a 5-element group: three workgroups' worth of whole quads,
    a ragged quad, the group boundary and a second ragged quad all fall in the second pass of the loop.

    Mutation check (adam_kernel): drop `q += (long long)gridDim.x * blockDim.x` (break after the first pass) —
    elements 4 194 304.. of the first group and the whole second group keep their input; this test fails on
    "big.param[4194304]"."""
    assert (GRID_NUMEL + 3) // 4 > 256 * 16 * 256
    gb = GuardBuffer()
    hyper = [dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-15, weight_decay=0.0, step=5),
             dict(lr=0.05, beta1=0.8, beta2=0.99, eps=1e-8, weight_decay=0.01, step=2)]
    datas = [_adam_data(GRID_NUMEL, 77), _adam_data(5, 78)]
    groups = [(_place_group(gb, "big", datas[0], offsets), GRID_NUMEL, hyper[0]),
              (_place_group(gb, "tail", datas[1], offsets), 5, hyper[1])]
    gb.upload()
    _adam_launch(gb, groups, 1)
    want, nan_words = gb.image.copy(), np.zeros(gb.image.size, bool)
    for (regs, numel, h), data in zip(groups, datas):
        _adam_expect(oracle, want, nan_words, regs, data, h, 1)
    gb.compare(gb.download(), want)


@gpu
@pytest.mark.parametrize("offsets", [(0, 0, 0, 0), (0, 1, 0, 0)], ids=["vector", "scalar"])
def test_gpu_adam_value_edges(oracle, offsets):
    """EDGE_CASES at known lanes of a float4 (plain values in the other three lanes and in both neighbouring quads),
    once with the reference's eps = 1e-15 and no weight decay, once with weight decay: zero gradient on zero second
    moment (the update is m / eps), denormal gradients, moments and parameters, gradients whose square overflows,
    +-inf and NaN gradients.  Bit-exact against the oracle wherever the oracle is not NaN, NaN exactly where it is
    NaN — so a NaN or inf lane leaves its three neighbours clean."""
    gb, groups, datas = GuardBuffer(), [], []
    for k, h in enumerate(EDGE_HYPER):
        data, special = _edge_data(5 + k)
        groups.append((_place_group(gb, f"edge{k}", data, offsets), EDGE_NUMEL, h))
        datas.append(data)
    gb.upload()
    _adam_launch(gb, groups, 0)
    want, nan_words = gb.image.copy(), np.zeros(gb.image.size, bool)
    for (regs, numel, h), data in zip(groups, datas):
        _adam_expect(oracle, want, nan_words, regs, data, h, 0)
        # the oracle's NaNs are where the cases put them: parameter of the +-inf cases, everything of the NaN case
        p_nan = np.isnan(GuardBuffer.get(want, regs[0]))
        assert p_nan.sum() == 3 and special[p_nan].all()
    gb.compare(gb.download(), want, nan_words=nan_words)


# ------------------------------------------------------------------------------------------------
# GPU: the Python optimizer layer
# ------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().cpu().contiguous().numpy().reshape(-1).view(np.uint32)


def _eleven_parameters():
    base = _params(1001, d=32, seed=51)
    g = torch.Generator().manual_seed(52)
    for i, n in enumerate((1, 3, 7, 1025, 4099)):
        base[f"vec{i}"] = torch.randn(n, generator=g)
    assert len(base) == 11
    # (parameter names, hyper-parameters) per param_group; optimizers: 2 + 1 + 1 + 2 groups
    layout = [[(["means"], dict(lr=1.6e-4, eps=1e-15)), (["scales", "quats"], dict(lr=0.005, eps=1e-15))],
              [(["opacities", "vec0", "vec3"], dict(lr=0.05, eps=1e-15, betas=(0.8, 0.99)))],
              [(["colors_all", "feature"], dict(lr=5e-4, eps=1e-15))],
              [(["vec1", "vec2"], dict(lr=1e-3, eps=1e-8, weight_decay=0.01)), (["vec4"], dict(lr=2e-3, eps=1e-10))]]
    return base, layout


def _build_optimizers(cls, params, layout):
    return [cls([dict(params=[params[n] for n in names], **hp) for names, hp in groups]) for groups in layout]


@gpu
def test_gpu_fused_step_over_eleven_ragged_parameters(oracle):
    """11 parameters (rows = 1001 with the six Gaussian shapes, five 1-D ones of odd length) in four FusedAdam
    instances with six param_groups, three steps of fused_step: 11 entries cross the 8-entry split of optim._launch.
    Every parameter and both moments bit for bit the oracle's per-parameter run, every state["step"] == 3, and
    torch.optim.Adam on the device within the tolerances of
    test_gpu_fused_adam_tracks_torch_adam_over_the_reference_groups."""
    from gaussiangrasper_amd.optim import FusedAdam, fused_step
    base, layout = _eleven_parameters()
    mine = {k: torch.nn.Parameter(v.clone().to(DEV)) for k, v in base.items()}
    ref = {k: torch.nn.Parameter(v.clone().to(DEV)) for k, v in base.items()}
    o_mine = _build_optimizers(FusedAdam, mine, layout)
    o_ref = _build_optimizers(torch.optim.Adam, ref, layout)
    hyper = {n: hp for groups in layout for names, hp in groups for n in names}
    host = {k: (v.numpy().reshape(-1).copy(), np.zeros(v.numel(), np.float32), np.zeros(v.numel(), np.float32))
            for k, v in base.items()}
    g = torch.Generator().manual_seed(53)
    for step in range(1, 4):
        for k in base:
            grad = torch.randn(base[k].shape, generator=g) * 1e-3
            mine[k].grad, ref[k].grad = grad.clone().to(DEV), grad.clone().to(DEV)
            hp = hyper[k]
            b1, b2 = hp.get("betas", (0.9, 0.999))
            host[k] = oracle.adam_step(*host[k][:1], grad.numpy().reshape(-1), *host[k][1:], lr=hp["lr"], beta1=b1,
                                       beta2=b2, eps=hp["eps"], weight_decay=hp.get("weight_decay", 0.0), step=step)
        fused_step(o_mine)
        for o in o_ref:
            o.step()
    state = {k: next(o.state[mine[k]] for o in o_mine if mine[k] in o.state) for k in base}
    state_ref = {k: next(o.state[ref[k]] for o in o_ref if ref[k] in o.state) for k in base}
    for k in base:
        sm, sr, lr = state[k], state_ref[k], hyper[k]["lr"]
        assert float(sm["step"]) == 3 == float(sr["step"]), k
        for name, t, want in (("param", mine[k], host[k][0]), ("exp_avg", sm["exp_avg"], host[k][1]),
                              ("exp_avg_sq", sm["exp_avg_sq"], host[k][2])):
            assert np.array_equal(_bits(t), want.view(np.uint32)), (k, name)
        assert torch.allclose(sm["exp_avg"], sr["exp_avg"], rtol=2e-6, atol=1e-12), k
        assert torch.allclose(sm["exp_avg_sq"], sr["exp_avg_sq"], rtol=2e-6, atol=1e-18), k
        assert torch.allclose(mine[k], ref[k], rtol=0, atol=5e-6 * lr / 1e-4 + 2e-6), k


@gpu
def test_gpu_fused_adam_leaves_a_parameter_without_gradient_alone(oracle):
    from gaussiangrasper_amd.optim import FusedAdam, fused_step
    g = torch.Generator().manual_seed(61)
    shapes = {"a": (1001, 3), "b": (7,), "c": (1025,), "never": (5,)}
    ps = {k: torch.nn.Parameter(torch.randn(*s, generator=g).to(DEV)) for k, s in shapes.items()}
    opts = [FusedAdam([ps["a"], ps["b"]], lr=1e-2), FusedAdam([ps["c"], ps["never"]], lr=1e-3, weight_decay=0.1)]
    for k in ("a", "b", "c"):
        ps[k].grad = (torch.randn(*shapes[k], generator=g) * 1e-2).to(DEV)
    fused_step(opts)
    assert len(opts[1].state[ps["never"]]) == 0                 # no gradient yet: no state, as torch.optim.Adam
    owner = {"a": opts[0], "b": opts[0], "c": opts[1]}
    before = {k: (_bits(ps[k]).copy(), _bits(o.state[ps[k]]["exp_avg"]).copy(),
                  _bits(o.state[ps[k]]["exp_avg_sq"]).copy()) for k, o in owner.items()}
    ps["b"].grad = None
    fused_step(opts)
    for k in ("a", "b", "c"):
        st = owner[k].state[ps[k]]
        now = (_bits(ps[k]), _bits(st["exp_avg"]), _bits(st["exp_avg_sq"]))
        if k == "b":
            assert float(st["step"]) == 1 and all(np.array_equal(x, y) for x, y in zip(now, before[k]))
        else:
            assert float(st["step"]) == 2 and not any(np.array_equal(x, y) for x, y in zip(now, before[k]))
    assert len(opts[1].state[ps["never"]]) == 0 and ps["never"].grad is None


@gpu
@pytest.mark.parametrize("n,shape", [(19, (19,)), (3003, (1001, 3))])
def test_gpu_fused_adam_on_a_gradient_view_at_a_misaligned_offset(oracle, n, shape):
    """p.grad = flat[1:1+n].view_as(p): 4-byte but not 16-byte aligned, the branch GradBucket's 64-float padding keeps
    the training loop out of.  Two steps, the second zeroing the gradient in the same pass: results bit for bit the
    oracle's, exactly n floats of `flat` zeroed, the floats of `flat` around the view unchanged."""
    from gaussiangrasper_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(*shape, generator=g)
    p = torch.nn.Parameter(p0.clone().to(DEV))
    opt = FusedAdam([p], lr=0.02, eps=1e-15, weight_decay=0.01)
    flat = torch.empty(n + 2 * GUARD, dtype=torch.float32, device=DEV)
    flat.view(torch.int32).fill_(SENTINEL)
    lo = GUARD + 1
    assert flat.data_ptr() % 16 == 0 and (flat[lo:].data_ptr() % 16) == 4
    p.grad = flat[lo:lo + n].view_as(p)
    hp, hm, hv = p0.numpy().reshape(-1).copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for step, zero in ((1, False), (2, True)):
        grad = torch.randn(n, generator=g) * 1e-2
        flat[lo:lo + n].copy_(grad)
        opt.step(zero_grad=zero)
        hp, hm, hv = oracle.adam_step(hp, grad.numpy(), hm, hv, lr=0.02, eps=1e-15, weight_decay=0.01, step=step)
        st = opt.state[p]
        assert np.array_equal(_bits(p), hp.view(np.uint32)), step
        assert np.array_equal(_bits(st["exp_avg"]), hm.view(np.uint32)), step
        assert np.array_equal(_bits(st["exp_avg_sq"]), hv.view(np.uint32)), step
        want = np.full(n + 2 * GUARD, SENTINEL, np.uint32)
        want[lo:lo + n] = 0 if zero else grad.numpy().view(np.uint32)
        assert np.array_equal(_bits(flat), want), step


@gpu
def test_gpu_adam_pieces_at_odd_offsets_and_more_than_eight_pieces(oracle):
    """optim.adam_pieces (dist.ShardedAdamStep's call) with 9 pieces — two launches — cut out of flat buffers at odd
    float offsets: parameter pieces at 3, 1, 2, 0, ..., gradient pieces one float further.  Bit for bit the oracle's,
    and every float of the flat buffers outside the pieces keeps its sentinel."""
    from gaussiangrasper_amd.optim import adam_pieces
    sizes = (5, 19, 1, 1027, 3, 16, 7, 4099, 2)
    gb, regs, datas = GuardBuffer(), [], []
    for k, n in enumerate(sizes):
        data = _adam_data(n, 200 + k)
        offs = ((3 - k) % 4, (4 - k) % 4, 0, (k % 2) * 2)
        regs.append(_place_group(gb, f"piece{k}", data, offs))
        datas.append(data)
    gb.upload()
    view = lambda r: gb.dev[r.start:r.start + r.words]
    entries, want, nan_words = [], gb.image.copy(), np.zeros(gb.image.size, bool)
    for k, (r, data) in enumerate(zip(regs, datas)):
        h = HYPER8[k % 8]
        entries.append((view(r[0]), view(r[1]), view(r[2]), view(r[3]), h["lr"], (h["beta1"], h["beta2"]), h["eps"],
                        h["weight_decay"], h["step"] + k // 8))
        _adam_expect(oracle, want, nan_words, r, data, dict(h, step=h["step"] + k // 8), 0)
    assert entries[0][0].data_ptr() % 16 == 12 and entries[0][1].data_ptr() % 16 == 0
    adam_pieces(entries)
    gb.compare(gb.download(), want)


# ------------------------------------------------------------------------------------------------
# GPU: row kernels through the C ABI, destinations exactly as long as the result
# ------------------------------------------------------------------------------------------------
COMPACT_WIDTHS = (1, 3, 4, 7, 32, 75, 128)


def _deleted_mask(name, n):
    """uint8 deleted-mask; a row is KEPT where the byte is 0"""
    if name == "none_deleted":
        return np.zeros(n, np.uint8)
    if name == "all_deleted":
        return np.full(n, 1, np.uint8)
    if name == "alternating":
        return (np.arange(n) % 2).astype(np.uint8)
    m = np.full(n, 1, np.uint8)
    if name == "only_last_kept":
        m[n - 1] = 0
    elif name == "rows_1023_1024_kept":
        m[1023:1025] = 0
    elif name == "run_1000_1100_kept":
        m[1000:1101] = 0
    elif name == "random_1_2_255":
        rng = np.random.default_rng(n)
        m = rng.choice(np.array([0, 0, 0, 1, 2, 255], np.uint8), size=n)
    else:
        raise KeyError(name)
    return m


_MASK_MIN_ROWS = {"none_deleted": 1, "all_deleted": 1, "alternating": 1, "only_last_kept": 1,
                  "rows_1023_1024_kept": 1025, "run_1000_1100_kept": 1101, "random_1_2_255": 1}
COMPACT_CASES = [(n, name) for n in (1, 1023, 1024, 1025, 2049) for name, lo in _MASK_MIN_ROWS.items() if n >= lo]


def test_row_mask_cases_are_what_their_names_say():
    assert len(COMPACT_CASES) == 5 * 5 + 2 + 1
    for n, name in COMPACT_CASES:
        m = _deleted_mask(name, n)
        assert m.dtype == np.uint8 and m.shape == (n,)
    assert np.array_equal(np.nonzero(_deleted_mask("rows_1023_1024_kept", 1025) == 0)[0], [1023, 1024])
    assert np.array_equal(np.nonzero(_deleted_mask("run_1000_1100_kept", 2049) == 0)[0], np.arange(1000, 1101))
    assert np.array_equal(np.nonzero(_deleted_mask("only_last_kept", 2049) == 0)[0], [2048])
    assert set(_deleted_mask("random_1_2_255", 1025)) == {0, 1, 2, 255}


def _workspace(lib, n):
    return torch.empty(max(int(lib.gg_rows_workspace(n)), 256), dtype=torch.uint8, device=DEV)


@gpu
@pytest.mark.parametrize("n,mask_name", COMPACT_CASES)
def test_gpu_compact_rows_exact_length_destinations(oracle, n, mask_name):
    """gg_compact_rows, seven widths in one launch, every destination exactly kept * w floats at an odd 4-byte offset
    between sentinels (zero floats when everything is deleted): a[mask == 0] from numpy (and the oracle),
    num_kept_out, sentinels intact, mask and sources unchanged."""
    from gaussiangrasper_amd import _lib
    from gaussiangrasper_amd._call import stream
    lib = _lib.load()
    mask = _deleted_mask(mask_name, n)
    kept = int((mask == 0).sum())
    rng = np.random.default_rng(n + 1)
    gb = GuardBuffer()
    r_mask = gb.place("mask", mask, 1)
    r_kept = gb.reserve("num_kept_out", 2, 2)
    srcs, r_src, r_dst = [], [], []
    for k, w in enumerate(COMPACT_WIDTHS):
        a = rng.standard_normal((n, w)).astype(np.float32)
        srcs.append(a)
        r_src.append(gb.place(f"src_w{w}", a, (0, 3, 1, 2)[k % 4]))
        r_dst.append(gb.reserve(f"dst_w{w}", kept * w, (1, 3)[k % 2]))
    gb.upload()
    desc = (_lib.RowArray * len(srcs))()
    for k, w in enumerate(COMPACT_WIDTHS):
        desc[k] = _lib.RowArray(gb.ptr(r_src[k]), gb.ptr(r_dst[k]), w, 0)
    ws = _workspace(lib, n)
    _lib.check(lib.gg_compact_rows(n, C.c_void_p(gb.ptr(r_mask)), len(srcs), desc, C.c_void_p(gb.ptr(r_kept)),
                                   C.c_void_p(ws.data_ptr()), ws.numel(), stream(gb.dev.device)), "gg_compact_rows")
    want = gb.image.copy()
    GuardBuffer.put(want, r_kept, np.array([kept], np.int64))
    for a, r in zip(srcs, r_dst):
        out = a[mask == 0]
        assert np.array_equal(oracle.compact_rows(mask, a), out)
        GuardBuffer.put(want, r, out)
    gb.compare(gb.download(), want)


@gpu
@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_gpu_mask_scan_counts_every_nonzero_byte(oracle, n, invert):
    """gg_mask_scan on masks whose set bytes are 1, 2 and 255 mixed (and on the block-boundary masks): a byte counts
    as set by != 0.  ranks is exactly N int32 between sentinels; ranks, the total and the sentinel after
    ranks[N-1] come from numpy's cumsum (and the oracle)."""
    from gaussiangrasper_amd import _lib
    from gaussiangrasper_amd._call import stream
    lib = _lib.load()
    names = [name for name, lo in _MASK_MIN_ROWS.items() if n >= lo]
    gb, cases = GuardBuffer(), []
    for k, name in enumerate(names):
        mask = _deleted_mask(name, n)
        cases.append((mask, gb.place(f"{name}.mask", mask, k % 4), gb.reserve(f"{name}.ranks", n, (k + 1) % 4),
                      gb.reserve(f"{name}.total", 2, 2 * (k % 2))))
    gb.upload()
    ws = _workspace(lib, n)
    want = gb.image.copy()
    for mask, r_mask, r_ranks, r_total in cases:
        _lib.check(lib.gg_mask_scan(n, C.c_void_p(gb.ptr(r_mask)), invert, C.c_void_p(gb.ptr(r_ranks)),
                                    C.c_void_p(gb.ptr(r_total)), C.c_void_p(ws.data_ptr()), ws.numel(),
                                    stream(gb.dev.device)), "gg_mask_scan")
        sel = ((mask != 0) != bool(invert)).astype(np.int64)
        ranks = (np.cumsum(sel) - sel).astype(np.int32)
        o_ranks, o_total = oracle.mask_scan(mask, invert=bool(invert))
        assert np.array_equal(o_ranks, ranks) and o_total == int(sel.sum())
        GuardBuffer.put(want, r_ranks, ranks)
        GuardBuffer.put(want, r_total, np.array([sel.sum()], np.int64))
    gb.compare(gb.download(), want)


DENSIFY_CASES = ("dups_only", "splits_only", "neither", "all_split_and_dup", "last_row_split")


def _densify_masks(case, n):
    rng = np.random.default_rng(n + len(case))
    some = lambda frac: (rng.random(n) < frac) if n > 1 else np.ones(n, bool)
    split, dup = np.zeros(n, bool), np.zeros(n, bool)
    if case == "dups_only":
        dup = some(0.3)
    elif case == "splits_only":
        split = some(0.2)
    elif case == "all_split_and_dup":
        split[:], dup[:] = True, True
    elif case == "last_row_split":
        split[n - 1] = True
        dup = some(0.3)
        dup[n - 1] = True
    return split, dup


@gpu
@pytest.mark.parametrize("case", DENSIFY_CASES)
@pytest.mark.parametrize("nsamps", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 1025, 2049])
def test_gpu_densify_rows_exact_length_destinations(oracle, n, nsamps, case):
    """gg_densify_rows with all four kinds in one launch and every destination exactly N + nsamps * n_split + n_dup
    rows between sentinels.  A side with no selected row passes NULL mask and ranks, as the ABI allows (with
    n_split == 0 the kernel's split_mask is null, with n_dup == 0 its dup_mask).  Set mask bytes are 1 and 255.
    COPY / ZERO_NEW bit for bit the oracle's; MEANS / SCALES within rtol = atol = 2e-6 of the oracle where expf / logf
    enter (new split rows of the means; split rows, their samples and their duplicates of the scales) and bit for
    bit everywhere else; sentinels intact; masks, ranks, samples and sources unchanged."""
    from gaussiangrasper_amd import _lib
    from gaussiangrasper_amd._call import stream
    lib = _lib.load()
    split, dup = _densify_masks(case, n)
    ns, nd = int(split.sum()), int(dup.sum())
    assert {"dups_only": ns == 0 < nd, "splits_only": nd == 0 < ns, "neither": ns == nd == 0,
            "all_split_and_dup": ns == nd == n, "last_row_split": ns == 1 and split[-1]}[case]
    total = n + nsamps * ns + nd
    p = {k: v.numpy() for k, v in _params(n, d=7, seed=n + nsamps).items()}
    rng = np.random.default_rng(n * 7 + nsamps)
    z = rng.standard_normal((nsamps * ns, 3)).astype(np.float32)
    moment = rng.standard_normal((n, 5)).astype(np.float32)
    arrays = [("means", p["means"], _lib.ROWS_MEANS), ("scales", p["scales"], _lib.ROWS_SCALES),
              ("quats", p["quats"], _lib.ROWS_COPY), ("opacities", p["opacities"], _lib.ROWS_COPY),
              ("feature", p["feature"], _lib.ROWS_COPY), ("moment", moment, _lib.ROWS_ZERO_NEW),
              ("scales_moment", rng.standard_normal((n, 3)).astype(np.float32), _lib.ROWS_ZERO_NEW)]
    as_bytes = lambda m: np.where(m, np.where(np.arange(n) % 3 == 0, 255, 1), 0).astype(np.uint8)
    ranks = lambda m: (np.cumsum(m) - m).astype(np.int32)
    gb = GuardBuffer()
    r_sm, r_dm = gb.place("split_mask", as_bytes(split), 3), gb.place("dup_mask", as_bytes(dup), 1)
    r_sr, r_dr = gb.place("split_ranks", ranks(split), 1), gb.place("dup_ranks", ranks(dup), 2)
    r_z = gb.place("samples", z, 3)
    r_src, r_dst = {}, {}
    for k, (name, a, kind) in enumerate(arrays):
        r_src[name] = gb.place(f"src.{name}", a, (1, 0, 2, 3)[k % 4])
        r_dst[name] = gb.reserve(f"dst.{name}", total * a.shape[1], (3, 1, 0, 2)[k % 4])
    gb.upload()
    desc = (_lib.RowArray * len(arrays))()
    for k, (name, a, kind) in enumerate(arrays):
        desc[k] = _lib.RowArray(gb.ptr(r_src[name]), gb.ptr(r_dst[name]), a.shape[1], kind)
    vp = lambda r, on=True: C.c_void_p(gb.ptr(r)) if on else None
    _lib.check(lib.gg_densify_rows(n, vp(r_sm, ns), vp(r_dm, nd), vp(r_sr, ns), vp(r_dr, nd), ns, nd, nsamps,
                                   vp(r_z, ns), 1.6, vp(r_src["means"]), vp(r_src["scales"]), vp(r_src["quats"]),
                                   len(arrays), desc, stream(gb.dev.device)), "gg_densify_rows")
    got = gb.download()
    want, loose = gb.image.copy(), np.zeros(gb.image.size, bool)
    for name, a, kind in arrays:
        o = oracle.densify_rows(a, kind, split, dup, nsamps, z, 1.6, p["means"], p["scales"], p["quats"])
        assert o.shape == (total, a.shape[1])
        r = r_dst[name]
        GuardBuffer.put(want, r, o)
        rows = np.zeros(total, bool)        # rows of this destination that hold an expf / logf result
        if kind == _lib.ROWS_MEANS:
            rows[n:n + nsamps * ns] = True
        elif kind == _lib.ROWS_SCALES:
            rows[:n] = split
            rows[n:n + nsamps * ns] = True
            rows[n + nsamps * ns:] = split[dup]
        if rows.any():
            loose[r.start:r.start + r.words] = np.repeat(rows, a.shape[1])
            g = GuardBuffer.get(got, r).reshape(o.shape)
            assert np.allclose(g[rows], o[rows], rtol=2e-6, atol=2e-6), name
        if case == "neither":
            assert np.array_equal(o, a) and not rows.any()
    gb.compare(got, want, loose_words=loose)


# ------------------------------------------------------------------------------------------------
# GPU: densify.compact / densify.append_rows across their 24-array chunks
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("count", [24, 25, 49])
def test_gpu_compact_wrapper_across_chunks(count):
    """densify.compact with 24, 25 and 49 arrays = one, two and three gg_compact_rows launches that share one
    workspace and one `kept` cell: every output is a[~mask], so the count read after the last chunk is right"""
    from gaussiangrasper_amd.densify import compact
    n = 1500
    g = torch.Generator().manual_seed(count)
    mask = torch.rand(n, generator=g) < 0.35
    arrays = [torch.randn(n, (1, 3, 4, 7)[k % 4], generator=g) for k in range(count)]
    arrays[-1] = torch.randn(n, 5, 3, generator=g)
    outs = compact([a.to(DEV) for a in arrays], mask.to(DEV))
    assert len(outs) == count
    for k, (a, o) in enumerate(zip(arrays, outs)):
        assert o.shape[0] == int((~mask).sum()) and torch.equal(o.cpu(), a[~mask]), k


@gpu
@pytest.mark.parametrize("count", [24, 25, 49])
def test_gpu_append_rows_wrapper_across_chunks(oracle, count):
    """densify.append_rows with 24, 25 and 49 arrays (one, two, three gg_densify_rows launches): the MEANS / SCALES
    arrays sit in the first and in the LAST chunk; COPY / ZERO_NEW arrays equal the torch.cat restatement bit for
    bit, MEANS / SCALES the oracle and the restatement within rtol = atol = 2e-6"""
    import oracle_ops
    from gaussiangrasper_amd import _lib
    from gaussiangrasper_amd.densify import append_rows
    n, samps = 1500, 2
    p = _params(n, d=8, seed=count)
    g = torch.Generator().manual_seed(count + 1)
    split = torch.rand(n, generator=g) < 0.15
    dup = torch.rand(n, generator=g) < 0.25
    z = torch.randn(samps * int(split.sum()), 3, generator=g)
    arrays = [(p["means"], _lib.ROWS_MEANS), (p["scales"], _lib.ROWS_SCALES)]
    for k in range(count - 4):
        arrays.append((torch.randn(n, (1, 3, 4, 7)[k % 4], generator=g), (_lib.ROWS_COPY, _lib.ROWS_ZERO_NEW)[k % 2]))
    arrays += [(p["scales"], _lib.ROWS_SCALES), (p["means"], _lib.ROWS_MEANS)]
    assert len(arrays) == count
    dev = lambda t: t.to(DEV)
    outs, ns, nd, used = append_rows([(dev(a), kind) for a, kind in arrays], dev(split), dev(dup), samps, dev(z),
                                     dev(p["means"]), dev(p["scales"]), dev(p["quats"]))
    assert (ns, nd, len(outs)) == (int(split.sum()), int(dup.sum()), count) and torch.equal(used.cpu(), z)
    want_t = torch_split_dup(p, split, dup, samps, z, oracle_ops.quat_to_rotmat)
    rep = lambda t: t[split].repeat(samps, *([1] * (t.dim() - 1)))
    for k, ((a, kind), o) in enumerate(zip(arrays, outs)):
        o = o.cpu()
        assert o.shape[0] == n + samps * ns + nd, k
        if kind == _lib.ROWS_COPY:
            assert torch.equal(o, torch.cat([a, rep(a), a[dup]])), k
        elif kind == _lib.ROWS_ZERO_NEW:
            assert torch.equal(o, torch_dup_in_optim(a, split, dup, samps)), k
        else:
            name = "means" if kind == _lib.ROWS_MEANS else "scales"
            want_o = oracle.densify_rows(a.numpy(), kind, split.numpy(), dup.numpy(), samps, z.numpy(), 1.6,
                                         p["means"].numpy(), p["scales"].numpy(), p["quats"].numpy())
            assert np.allclose(o.numpy(), want_o, rtol=2e-6, atol=2e-6), k
            assert np.allclose(o.numpy(), want_t[name].numpy(), rtol=2e-6, atol=2e-6), k
            assert np.array_equal(o.numpy()[:n][~split.numpy()], a.numpy()[~split.numpy()]), k
