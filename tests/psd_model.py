"""The Welch power spectrum of include/galsynth.h (gal_synth_iq_psd) stated in numpy: an INTEGER radix-2 transform, so that the
library's uint64 sums are held with np.array_equal.  Vectorised over the segments; the stage loop is log2 N <= 12 iterations.

    values(buf, fmt)                          the interleaved values v[j] of a buffer, as the correlator bank defines them
    psd(v, fmt, log2_n, hop, window)          -> (uint64[N] sums in natural bin order, n_seg)
    transform(xw_r, xw_i)                     the transform of windowed segments [n_seg, N] (int64 arrays holding int32 values)
"""
import numpy as np

ISHORT, IBYTE, IBIT = 0, 1, 2
SCALE = {ISHORT: 0, IBYTE: 8, IBIT: 14}  # g: v 2^g is the value on the int16 grid

_K = np.arange(4096)
C = np.rint(2.0 ** 30 * np.cos(2.0 * np.pi * _K / 4096.0)).astype(np.int64)
S = np.rint(2.0 ** 30 * np.sin(2.0 * np.pi * _K / 4096.0)).astype(np.int64)

_I32 = (-(1 << 31), (1 << 31) - 1)


def values(buf, fmt):
    """int64 v[j] of the bytes / int16 / int8 array `buf` in format fmt"""
    if fmt == ISHORT:
        return np.asarray(buf).view(np.int16).astype(np.int64)
    if fmt == IBYTE:
        return np.asarray(buf).view(np.int8).astype(np.int64)
    bits = np.unpackbits(np.asarray(buf).view(np.uint8))  # MSB first
    return bits.astype(np.int64) * 2 - 1


def segments(log2_n, hop, n_samples):
    """n_seg of gal_synth_psd_segments: 0 where the call is refused"""
    if not (3 <= log2_n <= 12):
        return 0
    n = 1 << log2_n
    if not (1 <= hop <= n) or n_samples < n:
        return 0
    n_seg = (n_samples - n) // hop + 1
    return n_seg if n_seg * n * n <= 1 << 32 else 0


def window(log2_n, kind):
    n = 1 << log2_n
    if kind == 0:
        return np.full(n, 32768, np.int64)
    return ((1 << 30) - C[np.arange(n) * (4096 // n)]) >> 16


def _check32(a, seen):
    lo, hi = int(a.min()), int(a.max())
    assert _I32[0] <= lo and hi <= _I32[1], "a value left int32: %d .. %d" % (lo, hi)
    if seen is not None:
        seen[0] = max(seen[0], -lo, hi)


def transform(xr, xi, seen=None):
    """radix-2 decimation in time of [n_seg, N] int64 arrays; every intermediate value is checked to fit an int32 (seen: a
    one-element list that receives the largest magnitude met)"""
    n = xr.shape[1]
    bits = n.bit_length() - 1
    rev = np.zeros(n, np.int64)
    for b in range(bits):
        rev |= ((np.arange(n) >> b) & 1) << (bits - 1 - b)
    xr, xi = xr[:, rev].copy(), xi[:, rev].copy()  # position rev[n] <- sample n is the same permutation: rev is an involution
    p_all = np.arange(n)
    h = 1
    while h < n:
        p = p_all[(p_all % (2 * h)) < h]
        j = (p % h) * (4096 // (2 * h))
        wr, wi = C[j], -S[j]
        ur, ui, vr, vi = xr[:, p], xi[:, p], xr[:, p + h], xi[:, p + h]
        tr = (vr * wr - vi * wi + (1 << 29)) >> 30
        ti = (vr * wi + vi * wr + (1 << 29)) >> 30
        xr[:, p], xi[:, p], xr[:, p + h], xi[:, p + h] = ur + tr, ui + ti, ur - tr, ui - ti
        _check32(xr, seen)
        _check32(xi, seen)
        h *= 2
    return xr, xi


def windowed(v, fmt, log2_n, hop, kind):
    """the windowed segments (xw_r, xw_i), [n_seg, N] int64, of the interleaved values v"""
    n = 1 << log2_n
    n_seg = segments(log2_n, hop, len(v) // 2)
    assert n_seg > 0, "refused"
    v = np.asarray(v, np.int64)
    win = window(log2_n, kind)
    g = SCALE[fmt]
    out = []
    for rail in (v[0::2], v[1::2]):
        seg = np.lib.stride_tricks.sliding_window_view(rail, n)[::hop][:n_seg]
        out.append(((seg << g) * win + (1 << 14)) >> 15)
    return out[0], out[1]


def psd(v, fmt, log2_n, hop, kind, chunk=4096):
    """(uint64[N], n_seg): the sums of |X[k]|^2 over the segments, natural bin order (bin k = k fs / N; k >= N / 2 negative)"""
    n = 1 << log2_n
    xr, xi = windowed(v, fmt, log2_n, hop, kind)
    acc = np.zeros(n, np.uint64)
    for s0 in range(0, xr.shape[0], chunk):
        yr, yi = transform(xr[s0:s0 + chunk], xi[s0:s0 + chunk])
        acc += (yr * yr + yi * yi).astype(np.uint64).sum(axis=0, dtype=np.uint64)
    return acc, xr.shape[0]
