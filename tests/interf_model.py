"""A numpy statement of the interference sources of include/galsynth.h (gal_synth_iq_convert_interf): the
closed-form phase of a CW tone or a restarting linear chirp, the Q12 cosine table, the pulse gate, and the integer mix with the noise
floor of noise_model in front of the three output formats.  It knows nothing of batches, vectors or the GPU: a source's term is a
function of (its parameters, global complex-sample index N) alone.

A source is a dict with the fields of gal_iq_interf_t (amp_q4, ph0, f0, df, sweep_len, pulse_period, pulse_on; missing ones are 0)."""
import math

import numpy as np

import noise_model

FIELDS = ("amp_q4", "ph0", "f0", "df", "sweep_len", "pulse_period", "pulse_on")
M32 = np.uint64(0xFFFFFFFF)


def cos_table():
    """C[k] = round(4096 cos(2 pi k / 1024)), int64."""
    return np.array([int(math.floor(4096.0 * math.cos(2.0 * math.pi * k / 1024.0) + 0.5)) for k in range(1024)], dtype=np.int64)


_C = cos_table()


def source(**kw):
    unknown = set(kw) - set(FIELDS)
    if unknown:
        raise ValueError("unknown fields %s" % sorted(unknown))
    return {k: int(kw.get(k, 0)) for k in FIELDS}


def phase(src, n_first, n):
    """phi(N) mod 2^32 for N = n_first .. n_first + n - 1 (uint64 array holding 32-bit values), by the closed form.  uint64
    arithmetic wraps modulo 2^64, of which 2^32 is a divisor: every product below may overflow except m (m - 1), which must be
    halved exactly and is below 2^64."""
    N = np.uint64(n_first) + np.arange(n, dtype=np.uint64)
    f0, df, ph0 = np.uint64(src["f0"] & 0xFFFFFFFF), np.uint64(src["df"] & 0xFFFFFFFF), np.uint64(src["ph0"] & 0xFFFFFFFF)
    L = src["sweep_len"]
    with np.errstate(over="ignore"):
        if L == 0:
            return (ph0 + (N & M32) * f0) & M32
        s, m = N // np.uint64(L), N % np.uint64(L)
        W = (L * (src["f0"] & 0xFFFFFFFF) + (src["df"] & 0xFFFFFFFF) * (L * (L - 1) // 2)) & 0xFFFFFFFF  # python integers: exact
        tri = (m * (m - np.uint64(1))) >> np.uint64(1)  # m (m - 1) / 2 (m = 0: 0 x (2^64 - 1) = 0)
        return (ph0 + (s & M32) * np.uint64(W) + m * f0 + df * (tri & M32)) & M32


def phase_recurrence(src, n_first, n, phi_first):
    """The same by phi(N + 1) = phi(N) + f0 + (N mod sweep_len) df, from phi(n_first) = phi_first, in python integers."""
    out = np.empty(n, dtype=np.uint64)
    phi, L = int(phi_first), src["sweep_len"]
    for k in range(n):
        out[k] = phi
        N = int(n_first) + k
        phi = (phi + src["f0"] + ((N % L) if L else 0) * src["df"]) & 0xFFFFFFFF
    return out


def gate(src, n_first, n):
    if src["pulse_period"] == 0:
        return np.ones(n, dtype=np.int64)
    N = np.uint64(n_first) + np.arange(n, dtype=np.uint64)
    return ((N % np.uint64(src["pulse_period"])) < np.uint64(src["pulse_on"])).astype(np.int64)


def terms(sources, n_first, n):
    """The sum over the sources of gate A C[..] for the 2 n interleaved values of the complex samples n_first .. n_first + n - 1 (int64)."""
    t = np.zeros(2 * n, dtype=np.int64)
    for src in sources:
        i = (phase(src, n_first, n) >> np.uint64(22)).astype(np.int64)
        a = gate(src, n_first, n) * src["amp_q4"]
        t[0::2] += a * _C[i]
        t[1::2] += a * _C[(i - 256) & 1023]
    return t


def mix(x, noise, sources, first_sample=0, piece=1 << 21):
    """y[j] = clamp16((x[j] G + z S + sum of the source terms + 32768) >> 16); noise = (seed, stream, gain_q16, sigma_q4) or None
    (G = 65536, S = 0).  Returns (y as int16, a boolean array: the clamp changed the value)."""
    x = np.asarray(x, dtype=np.int16)
    assert x.size % 2 == 0
    y = np.empty(x.size, dtype=np.int16)
    clipped = np.empty(x.size, dtype=bool)
    for a in range(0, x.size, 2 * piece):
        xs = x[a:a + 2 * piece].astype(np.int64)
        if noise is None:
            v = xs * 65536
        else:
            v = xs * int(noise[2]) + noise_model.noise_z(noise[0], noise[1], 2 * int(first_sample) + a, xs.size) * int(noise[3])
        v = (v + terms(sources, int(first_sample) + a // 2, xs.size // 2) + 32768) >> 16
        clipped[a:a + 2 * piece] = (v < -32768) | (v > 32767)
        y[a:a + 2 * piece] = np.clip(v, -32768, 32767).astype(np.int16)
    return y, clipped


def formatted(y, clipped, fmt, shift):
    """y and the clamp flags of mix() in a format: (output bytes as uint8, saturated count)."""
    if fmt == "ishort":
        return y.astype("<i2").view(np.uint8), int(np.count_nonzero(clipped))
    if fmt == "ibyte":
        r = (1 << (shift - 1)) if shift else 0
        v = (y.astype(np.int32) + r) >> shift
        sat = clipped | (v < -127) | (v > 127)
        return np.clip(v, -127, 127).astype(np.int8).view(np.uint8), int(np.count_nonzero(sat))
    return np.packbits(y > 0), int(np.count_nonzero(clipped))


def convert(x, fmt, shift, noise, sources, first_sample=0):
    """The whole definition; returns (output bytes as uint8, saturated count).  A value counts once if either clamp changed it."""
    y, clipped = mix(x, noise, sources, first_sample)
    return formatted(y, clipped, fmt, shift)


def _llround(v):
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def interf_make(js_db, gain, sample_rate, f_lo_hz, f_hi_hz=0.0, sweep_s=0.0, pulse_period_s=0.0, pulse_on_s=0.0):
    """The formula of gal_synth_interf_make (no range checks)."""
    src = source(amp_q4=_llround(16.0 * 250.0 * math.sqrt(2.0) * gain * 10.0 ** (js_db / 20.0)), f0=_llround(f_lo_hz / sample_rate * 4294967296.0))
    if sweep_s != 0.0:
        src["sweep_len"] = _llround(sweep_s * sample_rate)
        src["df"] = _llround((f_hi_hz - f_lo_hz) / sample_rate * 4294967296.0 / src["sweep_len"])
    src["pulse_period"] = _llround(pulse_period_s * sample_rate)
    src["pulse_on"] = _llround(pulse_on_s * sample_rate)
    return src
