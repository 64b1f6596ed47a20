"""A lattice case of the fea_up MLP's backward (gg_mlp_bwd) on which fp32 is exact, and a plain numpy restatement of
that backward.  Test infrastructure only; imports nothing from the package.

Every input is a small multiple of a power of two, so every product of the backward is exactly representable, and so
is every partial sum as long as the absolute values of a gradient element's terms add up to less than 2^24 units: the
five gradients then do not depend on the order of the sums (tiles, atomics, GEMM blocking) at all.  `condition` checks
that in fp64, term by term: a gradient element's terms are the fully expanded products (for v_x: g w2 w1 over every
output and hidden unit), so any partial sum that any association can form is a sum of some of them."""
import functools

import numpy as np

HIDDEN = 128
G_DENSITY = 1.0 / 16.0


def lattice_case(rows, in_dim, out_dim, seed):
    """(x, w1, b1, w2, b2, g) fp64: x in multiples of 1/2 within +-2, w1 and w2 in {-1/2, 0, 1/2}, b1 in multiples of
    1/4 within +-1, g in {-1, 0, 1} and non-zero with probability 1/16, b2 zero (it has no part in the backward)."""
    r = np.random.default_rng(seed)
    x = r.integers(-4, 5, (rows, in_dim)) / 2.0
    w1 = r.integers(-1, 2, (HIDDEN, in_dim)) / 2.0
    b1 = r.integers(-4, 5, HIDDEN) / 4.0
    w2 = r.integers(-1, 2, (out_dim, HIDDEN)) / 2.0
    g = r.integers(-1, 2, (rows, out_dim)) * (r.random((rows, out_dim)) < G_DENSITY)
    return x, w1, b1, w2, np.zeros(out_dim), g.astype(np.float64)


def backward(x, w1, b1, w2, g, dtype=np.float64):
    """(v_x, v_w1, v_b1, v_w2, v_b2) of relu(x w1^T + b1) w2^T + b2 against the cotangent g, evaluated in `dtype`;
    relu'(0) = 0, torch's convention.  Zeros are +0."""
    x, w1, b1, w2, g = (np.asarray(a, dtype=dtype) for a in (x, w1, b1, w2, g))
    h = x @ w1.T + b1
    gh = np.where(h > 0, g @ w2, dtype(0))
    out = (gh @ w1, gh.T @ x, gh.sum(axis=0), g.T @ np.maximum(h, dtype(0)), g.sum(axis=0))
    return tuple((a + dtype(0)).astype(dtype) for a in out)


def is_multiple(a, unit):
    q = np.asarray(a, dtype=np.float64) / unit
    return bool((q == np.rint(q)).all())


def condition(x, w1, b1, w2, g):
    """Per gradient (unit, largest sum over an element's terms of their absolute values), and the pre-activations h.
    Asserts the factors' units, from which every term's unit follows."""
    assert is_multiple(x, 0.5) and is_multiple(w1, 0.5) and is_multiple(b1, 0.25) and is_multiple(w2, 0.5)
    assert is_multiple(g, 1.0)
    ax, aw1, aw2, ag = np.abs(x), np.abs(w1), np.abs(w2), np.abs(g)
    h = x @ w1.T + b1                                   # fp64: exact, |h| < 2^53 units by far
    ah = ax @ aw1.T + np.abs(b1)                        # the absolute values of h's terms (units of 1/4)
    on = h > 0
    agh = np.where(on, ag @ aw2, 0.0)                   # dL/dh: terms g w2, units of 1/2
    return {
        "h": (0.25, float(ah.max())),
        "gh": (0.5, float((ag @ aw2).max())),           # formed before the relu mask is applied
        "v_x": (0.25, float((agh @ aw1).max())),        # terms g w2 w1
        "v_w1": (0.25, float((agh.T @ ax).max())),      # terms g w2 x
        "v_b1": (0.5, float(agh.sum(axis=0).max())),    # terms g w2
        "v_w2": (0.25, float((ag.T @ np.where(on, ah, 0.0)).max())),   # terms g (w1 x), g b1
        "v_b2": (1.0, float(ag.sum(axis=0).max())),     # terms g
    }, h


@functools.lru_cache(maxsize=None)
def lattice_reference(rows, in_dim, out_dim):
    """The case of a shape and its fp64 backward, computed once per process and read-only."""
    case = lattice_case(rows, in_dim, out_dim, seed=rows + in_dim + out_dim)
    x, w1, b1, w2, b2, g = case
    grads = backward(x, w1, b1, w2, g)
    for a in case + grads:
        a.setflags(write=False)
    return case, grads
