"""A numpy statement of the ionospheric scintillation of include/galsynth.h (gal_synth_iq_scint): the Philox /
Gauss draws, the 32-tap shaping sum, the nodes, the linear interpolation between them and the complex product.  It knows nothing of
tiles, launches or the GPU: z at a sample is a function of (row, N) alone.  Also gal_synth_scint_make in python numbers."""
import math

import numpy as np

import noise_model
import osc_model

# iq_scint.hip's kTile and kMaxBlocks: the GPU tests place their lengths at these edges.  Change them here too, or the edge sizes go
# stale without a failure.
TILE = 1024
MAX_BLOCKS = 2048
MIN_NODE, MAX_NODE = 64, 1 << 24
FIELDS = ("seed", "stream", "node_len", "a_q12", "b_q12")


def row(**kw):
    unknown = set(kw) - set(FIELDS)
    if unknown:
        raise ValueError("unknown fields %s" % sorted(unknown))
    r = {"seed": 1, "stream": 0, "node_len": MIN_NODE, "a_q12": 4096, "b_q12": 0}
    r.update({k: int(v) for k, v in kw.items()})
    return r


def table():
    """h[0..31] by the formula: round(32768 c exp(-(t - 15.5)^2 / 32)) with c = sqrt(2^30 / sum (32768 exp(..))^2), int64."""
    e = [math.exp(-(t - 15.5) ** 2 / 32.0) for t in range(32)]
    c = math.sqrt(2.0 ** 30 / sum((32768.0 * x) ** 2 for x in e))
    return np.array([int(math.floor(32768.0 * c * x + 0.5)) for x in e], dtype=np.int64)


_H = table()


def draws(seed, stream, i_first, n):
    """(gI, gQ) of the draws i_first .. i_first + n - 1 (int64 arrays): words 0 and 1 of Philox with counter word 3 = 2."""
    i = np.uint64(int(i_first)) + np.arange(int(n), dtype=np.uint64)
    w = noise_model.philox4x32_10(i & noise_model.MASK, i >> np.uint64(32), int(stream), 2, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    return noise_model.gauss_q12(w[0]), noise_model.gauss_q12(w[1])


def shaped(r, j_first, n):
    """(XI, XQ) of the nodes j_first .. j_first + n - 1 (int64)."""
    gI, gQ = draws(r["seed"], r["stream"], j_first, n + 31)
    SI = np.convolve(gI, _H[::-1], mode="valid")  # sum_t h[t] g(j + t); exact in int64
    SQ = np.convolve(gQ, _H[::-1], mode="valid")
    return (SI + (1 << 14)) >> 15, (SQ + (1 << 14)) >> 15


def nodes(r, j_first, n):
    """(ZI, ZQ) of the nodes j_first .. j_first + n - 1 (int64)."""
    XI, XQ = shaped(r, j_first, n)
    A, B = r["a_q12"], r["b_q12"]
    return np.clip(A + ((B * XI + 2048) >> 12), -32767, 32767), np.clip((B * XQ + 2048) >> 12, -32767, 32767)


def factor(r, first_sample, n):
    """(zI, zQ) at the samples N = first_sample .. first_sample + n - 1 (int64)."""
    L = r["node_len"]
    first_sample, n = int(first_sample), int(n)
    j_first, j_last = first_sample // L, (first_sample + n - 1) // L
    ZI, ZQ = nodes(r, j_first, j_last - j_first + 2)
    N = first_sample - j_first * L + np.arange(n, dtype=np.int64)  # relative to node j_first
    j, m = N // L, N % L
    R = (1 << 32) // L
    fr = (m * R) >> 20
    return ZI[j] + (((ZI[j + 1] - ZI[j]) * fr + 2048) >> 12), ZQ[j] + (((ZQ[j + 1] - ZQ[j]) * fr + 2048) >> 12)


def apply(x, r, first_sample):
    """The interleaved int16 stream x whose first complex sample has the global index first_sample -> (y as int16, complex samples a
    clamp changed)."""
    x = np.asarray(x, dtype=np.int16).astype(np.int64)
    n = x.size // 2
    if n == 0:
        return np.zeros(0, dtype=np.int16), 0
    zI, zQ = factor(r, first_sample, n)
    xI, xQ = x[0::2], x[1::2]
    vI, vQ = (xI * zI - xQ * zQ + 2048) >> 12, (xI * zQ + xQ * zI + 2048) >> 12
    assert np.abs(xI * zI - xQ * zQ).max() + 2048 < 1 << 31 and np.abs(xI * zQ + xQ * zI).max() + 2048 < 1 << 31
    yI, yQ = np.clip(vI, -32768, 32767), np.clip(vQ, -32768, 32767)
    y = np.empty(2 * n, dtype=np.int16)
    y[0::2], y[1::2] = yI, yQ
    return y, int(np.count_nonzero((yI != vI) | (yQ != vQ)))


def x_variance():
    """The variance of XI / 4096 as gal_synth_scint_make takes it: (H2 / 2^30) x (M2 / 2^55)."""
    h2 = int(np.sum(_H * _H))
    return (float(h2) / 2.0 ** 30) * (float(osc_model.gauss_m2()) / 2.0 ** 55)


def _llround(v):
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def make(s4, tau0_s, sample_rate=2.6e6):
    """gal_synth_scint_make, operation for operation in double; ValueError where it refuses."""
    if not all(math.isfinite(v) for v in (s4, tau0_s, sample_rate)) or not 0.0 <= s4 <= 1.0 or not sample_rate > 0:
        raise ValueError("argument")
    lv = tau0_s * sample_rate / 8.0
    if not 0.0 <= lv < 2.0 ** 32:
        raise ValueError("node_len")
    L = _llround(lv)
    if not MIN_NODE <= L <= MAX_NODE:
        raise ValueError("node_len")
    v = x_variance()
    if s4 == 0.0:
        A, B = 4096, 0
    elif s4 == 1.0:
        A, B = 0, _llround(4096.0 * math.sqrt(1.0 / (2.0 * v)))
    else:
        m = 1.0 / (s4 * s4)
        q = math.sqrt(m * m - m)
        K = q / (m - q)
        A, B = _llround(4096.0 * math.sqrt(K / (K + 1.0))), _llround(4096.0 * math.sqrt(1.0 / (2.0 * (K + 1.0) * v)))
    return row(node_len=L, a_q12=A, b_q12=B)
