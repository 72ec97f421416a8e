"""A numpy statement of the receiver oscillator of include/galsynth.h (gal_synth_osc_set, gal_synth_iq_osc): the
phase Phi(N) = P0 + N F + T(N) D + S Z(N) modulo 2^64, the Philox / Gauss increments z, the table look-up with its first-order
correction and the rotation.  It knows nothing of tiles, launches or the GPU: a sample's phase is a function of (parameters, N0, N)
alone.  Also gal_synth_osc_make and gal_synth_osc_lo_step in python numbers."""
import math

import numpy as np

import interf_model
import noise_model

# iq_osc.hip's kTile and kMaxBlocks: the GPU tests place their lengths at these edges.  Change them here too, or the edge sizes go
# stale without a failure.
TILE = 1024
MAX_BLOCKS = 2048
MAX_S = 1 << 48
FIELDS = ("seed", "stream", "p0", "f", "d", "s")
M64 = (1 << 64) - 1

_C = interf_model.cos_table()


def osc(**kw):
    unknown = set(kw) - set(FIELDS)
    if unknown:
        raise ValueError("unknown fields %s" % sorted(unknown))
    o = {"seed": 1, "stream": 0, "p0": 0, "f": 0, "d": 0, "s": 0}
    o.update({k: int(v) for k, v in kw.items()})
    return o


def tri(N):
    """T(N) = N (N - 1) / 2 mod 2^64 for a uint64 array: the even factor is halved first, then the product wraps."""
    N = np.asarray(N, dtype=np.uint64)
    one = np.uint64(1)
    with np.errstate(over="ignore"):
        return np.where(N & one, N * ((N - one) >> one), (N >> one) * (N - one))


def z(seed, stream, j_first, n):
    """z(j) for j = j_first .. j_first + n - 1 (int64): noise_model's Gaussian of Philox words with counter word 3 = 1."""
    j_first, n = int(j_first), int(n)
    b_first, b_last = j_first >> 2, (j_first + n - 1) >> 2
    blocks = np.arange(b_first, b_last + 1, dtype=np.uint64)
    words = noise_model.philox4x32_10(blocks & noise_model.MASK, blocks >> np.uint64(32), int(stream), 1, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    u = np.stack(words, axis=1).ravel()
    lo = j_first - 4 * b_first
    return noise_model.gauss_q12(u[lo:lo + n])


def phase(o, n0, first_sample, n, z_before=0):
    """(Phi(N) for N = first_sample .. first_sample + n - 1 as uint64, Z at the last of them).  z_before = Z(first_sample - 1), the sum
    an earlier piece of the stream returned (0 where first_sample == n0: z(n0) itself is not part of Z)."""
    N = np.uint64(first_sample) + np.arange(n, dtype=np.uint64)
    u = lambda v: np.uint64(int(v) & M64)  # noqa: E731
    with np.errstate(over="ignore"):
        phi = u(o["p0"]) + N * u(o["f"]) + tri(N) * u(o["d"])
        zz = int(z_before)
        if o["s"]:
            inc = z(o["seed"], o["stream"], first_sample, n)
            if int(first_sample) == int(n0):
                inc[0] = 0
            Z = np.cumsum(inc) + np.int64(z_before)
            zz = int(Z[-1])
            phi = phi + Z.astype(np.uint64) * u(o["s"])  # (a negative int64 -> its two's complement: the product wraps as it must)
    return phi, zz


def cos_sin(theta):
    """theta (uint32 values in any integer array) -> (c, s) in Q12 with the first-order correction, int64."""
    t = (np.asarray(theta).astype(np.int64) + (1 << 21)) & 0xFFFFFFFF
    i = t >> 22
    e = ((t >> 10) & 4095) - 2048
    c0, s0 = _C[i], _C[(i - 256) & 1023]
    return c0 - ((s0 * e * 101 + (1 << 25)) >> 26), s0 + ((c0 * e * 101 + (1 << 25)) >> 26)


def rotate(x, o, n0, first_sample, z_before=0):
    """The interleaved int16 stream x whose first complex sample has the global index first_sample -> (y as int16, complex samples a
    clamp changed, Z at the last sample)."""
    x = np.asarray(x, dtype=np.int16).astype(np.int64)
    n = x.size // 2
    if n == 0:
        return np.zeros(0, dtype=np.int16), 0, int(z_before)
    phi, zz = phase(o, n0, first_sample, n, z_before)
    c, s = cos_sin(phi >> np.uint64(32))
    xI, xQ = x[0::2], x[1::2]
    vI, vQ = (xI * c - xQ * s + 2048) >> 12, (xI * s + xQ * c + 2048) >> 12
    yI, yQ = np.clip(vI, -32768, 32767), np.clip(vQ, -32768, 32767)
    y = np.empty(2 * n, dtype=np.int16)
    y[0::2], y[1::2] = yI, yQ
    return y, int(np.count_nonzero((yI != vI) | (yQ != vQ))), zz


def gauss_m2():
    """The exact integer sum of mag(w)^2 over the 2^31 words w of the Gauss table's input (noise_model.z_moments, in integers)."""
    t = noise_model.gauss_table()
    m2 = 0
    for o in range(31):
        low = 30 - o
        step = 1 if low >= 13 else 1 << (13 - low)
        sf = np.arange(0, 8192, step)
        a, b = t[o, sf >> 8, 0], t[o, sf >> 8, 1]
        mag = a - (((a - b) * (sf & 255) + 128) >> 8)
        acc = int(np.sum(mag * mag))
        m2 += acc << (low - 13) if low >= 13 else acc
    return m2 + int(t[31, 0, 0]) ** 2


def z_variance():
    """The variance of z in units of 4096^2, as gal_synth_osc_make takes it: one correctly rounded division of the exact sum."""
    return float(gauss_m2()) / 2.0 ** 55


def _llround(v):
    if abs(v) >= 2.0 ** 52:
        return int(v)
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def make(f_hz=0.0, drift_hz_s=0.0, h0=0.0, sample_rate=2.6e6, carrier_hz=1575.42e6):
    """gal_synth_osc_make, operation for operation in double; ValueError where it refuses."""
    args = (f_hz, drift_hz_s, h0, sample_rate, carrier_hz)
    if not all(math.isfinite(v) for v in args) or not sample_rate > 0 or carrier_hz < 0 or h0 < 0:
        raise ValueError("argument")
    fv = f_hz / sample_rate * 2.0 ** 64
    dv = drift_hz_s / sample_rate / sample_rate * 2.0 ** 64
    if not abs(f_hz) < sample_rate / 2 or not abs(fv) < 2.0 ** 63 or not abs(dv) < 2.0 ** 63:
        raise ValueError("range")
    sigma_cycles = carrier_hz * math.sqrt(h0 / (2.0 * sample_rate))
    sv = sigma_cycles / math.sqrt(z_variance()) * 2.0 ** 52
    if not sv <= float(MAX_S):
        raise ValueError("s")
    return osc(f=_llround(fv), d=_llround(dv), s=_llround(sv))


def lo_step(o, N):
    """gal_synth_osc_lo_step: (F + N D) mod 2^64 >> 32 as an int32."""
    v = (((o["f"] + int(N) * o["d"]) & M64) >> 32)
    return v - (1 << 32) if v >= 1 << 31 else v


def sigma_cycles(o):
    """The per-sample phase-noise sigma in cycles: S 2^-64 x the standard deviation of z."""
    return o["s"] * 2.0 ** -64 * 4096.0 * math.sqrt(z_variance())
