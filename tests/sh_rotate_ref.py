"""gg_sh_rotate's arithmetic contract (include/gg_raster.h) restated in numpy fp32: for a selected row, band l >= 1,
output a and channel ch,

    out[a][ch] = ((D[a][lo] c[lo][ch] + D[a][lo+1] c[lo+1][ch]) + ...) + D[a][hi-1] c[hi-1][ch]

with a loop over b on fp32 arrays, so every product and every sum is rounded to fp32 once, as the kernel's are (numpy
does not contract).  Band 0 and rows not selected are copied."""
import numpy as np

BAND_OFFSETS = (0, 9, 34, 83, 164)      # pack_bands: D_l starts at BAND_OFFSETS[l - 1]


def sh_rotate_ref(coeffs, packed, mask=None):
    """coeffs (N, K, 3) fp32, packed: the fp32 pack_bands array, mask (N,) of anything (non-zero = selected) or None.
    Returns a new (N, K, 3) fp32 array."""
    c = np.asarray(coeffs)
    assert c.dtype == np.float32 and c.ndim == 3 and c.shape[2] == 3
    packed = np.asarray(packed)
    assert packed.dtype == np.float32
    n, k, _ = c.shape
    deg = {1: 0, 4: 1, 9: 2, 16: 3, 25: 4}[k]
    assert packed.size == BAND_OFFSETS[deg]
    sel = np.ones(n, bool) if mask is None else np.asarray(mask) != 0
    out = c.copy()
    src = c[sel]
    new = src.copy()
    with np.errstate(all="ignore"):         # inf / NaN rows: the same IEEE results as the device's
        for l in range(1, deg + 1):
            lo, hi, w = l * l, (l + 1) * (l + 1), 2 * l + 1
            D = packed[BAND_OFFSETS[l - 1]:BAND_OFFSETS[l]].reshape(w, w)
            for a in range(w):
                acc = D[a, 0] * src[:, lo, :]
                for b in range(1, w):
                    acc = acc + D[a, b] * src[:, lo + b, :]
                assert acc.dtype == np.float32
                new[:, lo + a, :] = acc
    out[sel] = new
    return out
