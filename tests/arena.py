"""A sentinel arena for the memory contract of the C entry points (tests/test_memory_contract_gpu.py).

Every device array of one call is carved out of ONE uint8 tensor filled with a sentinel byte: inputs get the caller's
bytes, workspaces seeded random bytes, outputs stay sentinel.  Each region sits at exactly the alignment asked for (a
multiple of `align`, not of 2 * align) and is followed by a guard of at least GUARD bytes; a guard also precedes the
first region.  After the call check() compares every byte outside the out / inout / ws regions with the image taken
before the call and names the region and byte offset of the first difference.  Works on any torch device."""
import ctypes

import numpy as np
import torch

GUARD = 256
SENTINEL = 0xA5
ROLES = ("in", "out", "inout", "ws")


class ArenaError(AssertionError):
    pass


class _Region:
    __slots__ = ("name", "nbytes", "align", "role", "data", "dtype", "shape", "off")

    def __init__(self, name, nbytes, align, role, data, dtype, shape):
        self.name, self.nbytes, self.align, self.role = name, nbytes, align, role
        self.data, self.dtype, self.shape, self.off = data, dtype, shape, -1


class Arena:
    """carve(...) every array, then ptr(name) for the call (the first ptr() lays the buffer out and fills it), then
    check() or untouched()."""

    def __init__(self, device, seed, sentinel=SENTINEL):
        self.device = torch.device(device)
        self.seed = int(seed)
        self.sentinel = int(sentinel)
        self.regions = {}
        self.buf = None
        self.image = None

    # ------------------------------------------------------------------------------------------------
    def carve(self, name, nbytes_or_array, align, role):
        """A region of `nbytes` bytes, or of the bytes of an array (which also gives the dtype and shape of the view
        check() returns; for role `out` and `ws` only its size, dtype and shape are used).  `align` a power of two."""
        assert self.buf is None, "carve() after the arena was laid out"
        assert role in ROLES, role
        assert name not in self.regions, name
        align = int(align)
        assert align >= 1 and align & (align - 1) == 0, align
        if isinstance(nbytes_or_array, (int, np.integer)):
            nbytes, data, dtype, shape = int(nbytes_or_array), None, np.dtype(np.uint8), (int(nbytes_or_array),)
            assert role in ("out", "ws"), "an in / inout region needs its bytes"
        else:
            a = np.ascontiguousarray(nbytes_or_array)
            nbytes, dtype, shape = a.nbytes, a.dtype, a.shape
            data = a.reshape(-1).view(np.uint8).copy() if role in ("in", "inout") else None
        assert nbytes >= 0
        self.regions[name] = _Region(name, nbytes, align, role, data, dtype, shape)
        return self

    def _build(self):
        regs = list(self.regions.values())
        total = 2 * GUARD + 512 + sum(r.nbytes + GUARD + 2 * r.align for r in regs)
        self._raw = torch.empty(total + 256, dtype=torch.uint8, device=self.device)
        skip = -self._raw.data_ptr() % 256           # the host allocator promises 64 bytes only
        self.buf = self._raw[skip:skip + total]
        base = self.buf.data_ptr()
        assert base % 256 == 0, f"arena base {base:#x} is not 256-byte aligned"
        self.base = base
        cur = base + GUARD
        for r in regs:
            a = r.align
            addr = (cur + a - 1) // a * a
            if addr % (2 * a) == 0:
                addr += a
            r.off = addr - base
            cur = addr + r.nbytes + GUARD
        assert cur - base <= total
        img = np.full(total, self.sentinel, np.uint8)
        rng = np.random.default_rng(self.seed)
        for r in regs:
            if r.role in ("in", "inout"):
                img[r.off:r.off + r.nbytes] = r.data
            elif r.role == "ws":
                img[r.off:r.off + r.nbytes] = rng.integers(0, 256, r.nbytes, dtype=np.uint8)
        self.image = img
        self.buf.copy_(torch.from_numpy(img))
        self._sync()

    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    # ------------------------------------------------------------------------------------------------
    def address(self, name):
        if self.buf is None:
            self._build()
        return self.base + self.regions[name].off

    def ptr(self, name):
        return ctypes.c_void_p(self.address(name))

    def nbytes(self, name):
        return self.regions[name].nbytes

    def _host(self):
        if self.buf is None:
            self._build()
        self._sync()
        return self.buf.cpu().numpy()

    def _where(self, off):
        """the region or guard that holds byte `off` of the buffer"""
        prev = None
        for r in self.regions.values():
            if off < r.off:
                break
            if off < r.off + r.nbytes:
                return f"{r.role} region '{r.name}', byte {off - r.off}"
            prev = r
        if prev is None:
            return f"guard before the first region, byte {off}"
        return f"guard after '{prev.name}', byte {off - prev.off - prev.nbytes}"

    def _view(self, host, r):
        return host[r.off:r.off + r.nbytes].copy().view(r.dtype).reshape(r.shape)

    def check(self):
        """Guards and `in` regions unchanged, or ArenaError naming the first changed byte.  Returns host copies of
        the out, inout and ws regions by name."""
        host = self._host()
        fixed = np.ones(len(host), bool)
        for r in self.regions.values():
            if r.role != "in":
                fixed[r.off:r.off + r.nbytes] = False
        bad = np.nonzero(fixed & (host != self.image))[0]
        if len(bad):
            o = int(bad[0])
            raise ArenaError(f"{len(bad)} byte(s) changed outside the outputs; the first: {self._where(o)} "
                             f"(was {self.image[o]:#04x}, is {host[o]:#04x})")
        return {r.name: self._view(host, r) for r in self.regions.values() if r.role != "in"}

    def untouched(self):
        """The whole buffer equals its image before the call (refused and empty calls)."""
        host = self._host()
        bad = np.nonzero(host != self.image)[0]
        if len(bad):
            o = int(bad[0])
            raise ArenaError(f"{len(bad)} byte(s) changed; the first: {self._where(o)} "
                             f"(was {self.image[o]:#04x}, is {host[o]:#04x})")
        return True

    def rebase(self):
        """Take the buffer as it is now for the image: the next check() / untouched() is about the next call alone
        (a backward after its forward, an emit after its count)."""
        self.image = self._host().copy()
        return self

    def before(self, name):
        """a region's bytes before the call, typed"""
        if self.buf is None:
            self._build()
        r = self.regions[name]
        return self.image[r.off:r.off + r.nbytes].copy().view(r.dtype).reshape(r.shape)

    def sentinel_like(self, name):
        """what an out region holds where nothing was written"""
        r = self.regions[name]
        return np.full(r.nbytes, self.sentinel, np.uint8).view(r.dtype).reshape(r.shape)
