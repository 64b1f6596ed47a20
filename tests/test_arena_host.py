"""The sentinel arena (tests/arena.py) on the CPU: check() finds a byte planted one past an output, one before it, in
an input and in the last guard, passes on an untouched arena, and every carved address has exactly the alignment asked
for."""
import ctypes

import numpy as np
import pytest

from arena import GUARD, SENTINEL, Arena, ArenaError


def make(seed=1):
    a = Arena("cpu", seed)
    a.carve("x", np.arange(13, dtype=np.float32), 4, "in")
    a.carve("bytes", np.arange(7, dtype=np.uint8), 1, "in")
    a.carve("d", np.arange(6, dtype=np.float64).reshape(2, 3), 8, "inout")
    a.carve("out", np.empty((5, 3), np.float32), 16, "out")
    a.carve("mask", 11, 1, "out")
    a.carve("ws", 768, 256, "ws")
    a.carve("empty", np.empty((0, 3), np.float32), 4, "out")
    a.carve("last", np.empty(3, np.int32), 4, "out")
    return a


def plant(a, name, delta, value=0x11):
    """one byte written at region `name`'s address + delta, through the pointer the kernel would get"""
    p = ctypes.cast(a.ptr(name).value + delta, ctypes.POINTER(ctypes.c_uint8))
    assert p[0] != value
    p[0] = value


def test_addresses_have_exactly_the_requested_alignment():
    a = make()
    for name, align in (("x", 4), ("bytes", 1), ("d", 8), ("out", 16), ("mask", 1), ("ws", 256), ("empty", 4),
                        ("last", 4)):
        addr = a.ptr(name).value
        assert isinstance(a.ptr(name), ctypes.c_void_p)
        assert addr % align == 0 and addr % (2 * align) == align, (name, hex(addr))
    assert a.base % 256 == 0
    # regions in carve order, each followed by at least GUARD bytes, the first preceded by as many
    regs = list(a.regions.values())
    assert regs[0].off >= GUARD
    for r, nxt in zip(regs, regs[1:]):
        assert nxt.off - (r.off + r.nbytes) >= GUARD
    assert len(a.image) - (regs[-1].off + regs[-1].nbytes) >= GUARD


def test_fill_inputs_workspace_and_sentinel():
    a, b, c = make(1), make(1), make(2)
    out = a.check()
    assert set(out) == {"d", "out", "mask", "ws", "empty", "last"}
    assert out["d"].dtype == np.float64 and np.array_equal(out["d"], np.arange(6.0).reshape(2, 3))
    assert out["out"].shape == (5, 3) and (out["out"].view(np.uint8) == SENTINEL).all()
    assert out["empty"].shape == (0, 3) and (out["mask"] == SENTINEL).all()
    assert np.array_equal(a.before("x"), np.arange(13, dtype=np.float32))
    assert np.array_equal(out["ws"], b.check()["ws"]) and not np.array_equal(out["ws"], c.check()["ws"])
    assert len(np.unique(out["ws"])) > 100                         # garbage, not a fill
    assert np.array_equal(a.sentinel_like("out").view(np.uint8), out["out"].view(np.uint8))
    # everything that is not a region is sentinel
    free = np.ones(len(a.image), bool)
    for r in a.regions.values():
        free[r.off:r.off + r.nbytes] = False
    assert (a.image[free] == SENTINEL).all()


def test_an_untouched_arena_passes():
    a = make()
    a.ptr("out")
    a.check()
    assert a.untouched()


def test_writes_inside_outputs_pass_check_but_not_untouched():
    a = make()
    plant(a, "out", 0)
    plant(a, "out", a.nbytes("out") - 1)
    plant(a, "d", 5)
    plant(a, "ws", 767)
    out = a.check()
    assert out["out"].view(np.uint8).reshape(-1)[0] == 0x11 and out["ws"][767] == 0x11
    with pytest.raises(ArenaError, match=r"4 byte\(s\) changed; the first: inout region 'd', byte 5"):
        a.untouched()


@pytest.mark.parametrize("name,delta,where", [
    ("out", 60, r"guard after 'out', byte 0"),                     # one past an output
    ("out", -1, r"guard after 'd', byte \d+"),                     # one before an output
    ("mask", 11, r"guard after 'mask', byte 0"),
    ("mask", -1, r"guard after 'out', byte \d+"),
    ("x", -1, r"guard before the first region, byte \d+"),
    ("x", 17, r"in region 'x', byte 17"),                          # in an input
    ("bytes", 6, r"in region 'bytes', byte 6"),
    ("ws", 768, r"guard after 'ws', byte 0"),
    ("ws", -1, r"guard after 'mask', byte \d+"),
    ("empty", 0, r"guard after 'empty', byte 0"),
    ("last", 12, r"guard after 'last', byte 0"),
])
def test_check_names_a_planted_byte(name, delta, where):
    a = make()
    plant(a, name, delta)
    with pytest.raises(ArenaError, match=where):
        a.check()
    with pytest.raises(ArenaError):
        a.untouched()


def test_the_last_byte_of_the_last_guard():
    a = make()
    a.ptr("x")
    end = a.base + len(a.image) - 1
    ctypes.cast(end, ctypes.POINTER(ctypes.c_uint8))[0] = 0
    with pytest.raises(ArenaError, match=r"guard after 'last', byte \d+"):
        a.check()


def test_rebase_makes_the_next_check_about_the_next_call():
    a = make()
    plant(a, "out", 3)                                             # a first call writes its output
    first = a.check()["out"]
    a.rebase()
    assert a.untouched()                                           # a second call that writes nothing
    plant(a, "out", 3, 0x22)
    with pytest.raises(ArenaError, match=r"out region 'out', byte 3 \(was 0x11, is 0x22\)"):
        a.untouched()
    assert a.check()["out"].tobytes() != first.tobytes()
    plant(a, "out", 60)                                            # and one that strays
    with pytest.raises(ArenaError, match=r"guard after 'out', byte 0"):
        a.check()


def test_carve_refuses_misuse():
    a = Arena("cpu", 0)
    with pytest.raises(AssertionError):
        a.carve("a", 16, 3, "out")                                 # not a power of two
    with pytest.raises(AssertionError):
        a.carve("a", 16, 4, "in")                                  # an input needs bytes
    with pytest.raises(AssertionError):
        a.carve("a", 16, 4, "scratch")
    a.carve("a", 16, 4, "out")
    with pytest.raises(AssertionError):
        a.carve("a", 16, 4, "out")                                 # the same name twice
    a.ptr("a")
    with pytest.raises(AssertionError):
        a.carve("b", 16, 4, "out")                                 # after the layout
