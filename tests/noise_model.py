"""A numpy statement of the noise floor of include/galsynth.h (gal_synth_iq_convert_noise): Philox4x32-10
uniform words, the octave-segment inverse CDF in Q12, the integer mix, and the three output formats behind it.  It knows nothing
of batches, vectors or the GPU: a value's noise is a function of (seed, stream, global value index J) alone."""
from statistics import NormalDist

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counter words (arrays or scalars) and key words (scalars) -> the four output words, uint64 arrays holding 32-bit values."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK for v in (c0, c1, c2, c3)]
    n = max(v.size for v in c)
    c = [np.broadcast_to(v, (n,)).copy() for v in c]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = c[0] * np.uint64(M0)  # 32 x 32 bits: fits 64
        p1 = c[2] * np.uint64(M1)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def gauss_table():
    """T[32][32][2] from q(v) = -Phi^-1(v / 2^32), int64."""
    nd = NormalDist()

    def q12(v):
        return int(round(-4096.0 * nd.inv_cdf(v / 4294967296.0)))

    t = np.zeros((32, 32, 2), dtype=np.int64)
    for o in range(31):
        base = 2.0 ** (30 - o)
        for s in range(32):
            t[o, s] = (q12(base * (1 + s / 32.0)), q12(base * (1 + (s + 1) / 32.0)))
    t[31] = q12(0.5)
    return t


_T = None


def _table():
    global _T
    if _T is None:
        _T = gauss_table()
    return _T


def gauss_q12(u):
    """32-bit uniform words -> z in Q12 (int64)."""
    u = np.asarray(u, dtype=np.uint64) & MASK
    neg = (u >> np.uint64(31)).astype(bool)
    w = (u & np.uint64(0x7FFFFFFF)).astype(np.int64)
    # leading zeros of w as a 31-bit number: 31 - bit_length(w)
    bl = np.zeros(w.shape, dtype=np.int64)
    nz = w > 0
    bl[nz] = np.floor(np.log2(w[nz].astype(np.float64))).astype(np.int64) + 1  # exact: w < 2^31 is exact in float64
    o = 31 - bl
    wn = np.where(nz, w << np.minimum(o, 30), 0)
    s = (wn >> 25) & 31
    f = (wn >> 17) & 255
    t = _table()
    a, b = t[o, s, 0], t[o, s, 1]
    mag = a - (((a - b) * f + 128) >> 8)
    return np.where(neg, -mag, mag)


def noise_z(seed, stream, j_first, n_val):
    """z for the global value indices J = j_first .. j_first + n_val - 1 (int64 array)."""
    j_first, n_val = int(j_first), int(n_val)
    b_first, b_last = j_first >> 2, (j_first + n_val - 1) >> 2
    blocks = np.arange(b_first, b_last + 1, dtype=np.uint64)
    words = philox4x32_10(blocks & MASK, blocks >> np.uint64(32), int(stream), 0, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    u = np.stack(words, axis=1).ravel()  # word J & 3 of block J >> 2, in J order
    lo = j_first - 4 * b_first
    return gauss_q12(u[lo:lo + n_val])


def mix(x, seed, stream, gain_q16, sigma_q4, first_sample=0, piece=1 << 22):
    """y[j] = clamp16((x[j] G + z S + 32768) >> 16) for the interleaved int16 stream x whose first complex sample has the index
    first_sample in the whole output; returns (y as int16, number of values the clamp changed as a boolean array)."""
    x = np.asarray(x, dtype=np.int16)
    y = np.empty(x.size, dtype=np.int16)
    clipped = np.empty(x.size, dtype=bool)
    for a in range(0, x.size, piece):
        xs = x[a:a + piece].astype(np.int64)
        z = noise_z(seed, stream, 2 * int(first_sample) + a, xs.size)
        v = (xs * int(gain_q16) + z * int(sigma_q4) + 32768) >> 16
        clipped[a:a + piece] = (v < -32768) | (v > 32767)
        y[a:a + piece] = np.clip(v, -32768, 32767).astype(np.int16)
    return y, clipped


def convert(x, fmt, shift, noise, first_sample=0):
    """The whole definition: noise = (seed, stream, gain_q16, sigma_q4); returns (output bytes as uint8, saturated count).
    A value counts once if either clamp (to int16 in the mix, to +-127 in ibyte) changed it."""
    y, clipped = mix(x, noise[0], noise[1], noise[2], noise[3], first_sample)
    if fmt == "ishort":
        return y.astype("<i2").view(np.uint8), int(np.count_nonzero(clipped))
    if fmt == "ibyte":
        r = (1 << (shift - 1)) if shift else 0
        v = (y.astype(np.int32) + r) >> shift
        sat = clipped | (v < -127) | (v > 127)
        return np.clip(v, -127, 127).astype(np.int8).view(np.uint8), int(np.count_nonzero(sat))
    return np.packbits(y > 0), int(np.count_nonzero(clipped))


def noise_from_cn0(cn0_dbhz, sample_rate, gain=1.0):
    """(gain_q16, sigma_q4) of gal_synth_noise_from_cn0: sigma = 250 gain sqrt(sample_rate / 10^(cn0 / 10)) int16 LSB."""
    return int(round(gain * 65536.0)), int(round(16.0 * 250.0 * gain * (sample_rate / 10.0 ** (cn0_dbhz / 10.0)) ** 0.5))


def z_moments():
    """Exact variance (unit 1 = 4096^2) and kurtosis of z over all 2^32 words, by enumeration of the (octave, segment, fraction)
    cells: for octave o a 31-bit word has 30 - o bits below its leading one, of which 13 select (s, f); the others do not change z."""
    t = _table().astype(np.float64)
    m2 = m4 = 0.0
    total = 0.0
    f_all = np.arange(256)
    for o in range(31):
        low = 30 - o  # bits below the leading one
        if low >= 13:
            f, weight = f_all, 2.0 ** (low - 13)
        else:  # the shift fills the low bits of (s, f) with zeros: only every 2^(13 - low)-th cell occurs, once
            step = 1 << (13 - low)
            sf = np.arange(0, 8192, step)
            weight = 1.0
            for s in np.unique(sf >> 8):
                ff = sf[(sf >> 8) == s] & 255
                a, b = t[o, s]
                mag = a - np.floor(((a - b) * ff + 128) / 256)
                m2 += weight * np.sum(mag ** 2)
                m4 += weight * np.sum(mag ** 4)
                total += weight * ff.size
            continue
        for s in range(32):
            a, b = t[o, s]
            mag = a - np.floor(((a - b) * f + 128) / 256)
            m2 += weight * np.sum(mag ** 2)
            m4 += weight * np.sum(mag ** 4)
            total += weight * f.size
    mag0 = t[31, 0, 0]  # w = 0
    m2 += mag0 ** 2
    m4 += mag0 ** 4
    total += 1
    assert total == 2.0 ** 31
    m2 /= total
    m4 /= total
    return m2 / 4096.0 ** 2, m4 / m2 ** 2
