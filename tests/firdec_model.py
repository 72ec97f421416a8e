"""The decimating front-end filter as include/galsynth.h defines it (gal_synth_firdec_check, gal_synth_firdec_lowpass,
gal_synth_firdec_out_samples, gal_synth_iq_firdec), in numpy -- TEST INFRASTRUCTURE: the product never imports this."""
import numpy as np

GAL_FIRDEC_MAX_TAPS = 512
GAL_FIRDEC_MAX_DECIM = 16
GAL_FIR_UNITY = 16384
TILE_INPUTS = 4096  # csrc/iq_firdec.hip: kTileIn


def tile_inputs(M):
    """The input samples one block of k_iq_firdec filters: (4096 / M) & ~3 outputs, M inputs each."""
    return ((TILE_INPUTS // M) & ~3) * M


def check(taps, decim):
    """True where gal_synth_firdec_check admits taps and decimation."""
    h = np.asarray(taps, dtype=np.int64)
    return (h.ndim == 1 and 1 <= h.size <= GAL_FIRDEC_MAX_TAPS and 2 <= int(decim) <= GAL_FIRDEC_MAX_DECIM
            and int(np.abs(h).sum()) <= 65535)


def out_samples(first_sample, n_in, decim):
    """The number of m with first_sample <= decim * m < first_sample + n_in (Python integers)."""
    P, n, M = int(first_sample), int(n_in), int(decim)
    return -((-(P + n)) // M) - -((-P) // M)


def firdec(x, taps, decim, first_sample=0, history=None):
    """x: interleaved int16 (I0, Q0, I1, Q1, ...) of the next input samples of a stream, the first of them with the global index
    first_sample; taps: int16 Q14; history: the interleaved input samples in front of x (None: zeros; only its last T - 1 samples
    matter).  Returns (y int16 interleaved, values the clamp changed): per rail a[m] = sum_k h[k] x[M m - k], y[m] = clamp16((a[m] +
    8192) >> 14) for the m with first_sample <= M m < first_sample + n.  Only the kept outputs are computed and counted."""
    x = np.asarray(x, dtype=np.int16)
    h = np.asarray(taps, dtype=np.int64)
    M, P = int(decim), int(first_sample)
    assert x.ndim == 1 and x.size % 2 == 0 and check(h, M) and P >= 0
    n, T = x.size // 2, h.size
    past = np.zeros(2 * (T - 1), dtype=np.int64)
    if history is not None and T > 1:
        hist = np.asarray(history, dtype=np.int64)
        assert hist.ndim == 1 and hist.size % 2 == 0
        m = min(hist.size, past.size)
        if m:
            past[past.size - m:] = hist[hist.size - m:]
    s = np.concatenate([past, x.astype(np.int64)]).reshape(-1, 2)  # s[T - 1 + i] = the input with the local index i
    i0 = (-P) % M
    idx = np.arange(i0, n, M, dtype=np.int64)  # the local indices of the kept outputs
    assert idx.size == out_samples(P, n, M)
    a = np.zeros((idx.size, 2), dtype=np.int64)
    for k in range(T):
        a += h[k] * s[idx + (T - 1 - k)]
    v = (a + 8192) >> 14
    y = np.clip(v, -32768, 32767)
    return y.astype(np.int16).reshape(-1), int(np.count_nonzero(y != v))


def lowpass(cutoff_hz, sample_rate_in, n_taps):
    """gal_synth_firdec_lowpass in double, operation for operation as the header states gal_synth_fir_lowpass: a Hamming-windowed
    sinc, rounded to Q14, the centre tap adjusted so that the taps sum to 16384."""
    assert n_taps % 2 == 1 and 3 <= n_taps <= GAL_FIRDEC_MAX_TAPS - 1 and 0.0 < cutoff_hz < sample_rate_in / 2
    pi = np.float64(3.14159265358979323846)
    fc = np.float64(cutoff_hz) / np.float64(sample_rate_in)
    M = n_taps - 1
    ws = np.zeros(n_taps, dtype=np.float64)
    S = np.float64(0.0)
    for k in range(n_taps):
        t = np.float64(k - M // 2)
        s = np.float64(2.0) * fc if k == M // 2 else np.sin(np.float64(2.0) * pi * fc * t) / (pi * t)
        w = np.float64(0.54) - np.float64(0.46) * np.cos(np.float64(2.0) * pi * np.float64(k) / np.float64(M))
        ws[k] = w * s
        S = S + ws[k]
    q = np.zeros(n_taps, dtype=np.int64)
    for k in range(n_taps):
        v = np.float64(16384.0) * ws[k] / S
        q[k] = int(np.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)  # llround: ties away from zero
    q[M // 2] += GAL_FIR_UNITY - int(q.sum())
    return q.astype(np.int16)


def default_taps(decim, rate_out=2.6e6):
    """The CLI's default decimator: a low-pass at 0.45 x the output rate with 32 M + 1 taps, a delay of 16 output samples."""
    return lowpass(0.45 * rate_out, decim * rate_out, 32 * decim + 1)


def random_taps(rng, T):
    """fir_model.random_taps for 1 <= T <= 512: T random int16 taps with sum |h| = 65535 exactly (T = 1 cannot reach it: -32768, the
    largest single tap) and |h[0]| >= 20000, so that a full-scale sample of h[0]'s sign is clamped: 20000 x 32767 > 16384 x 32768."""
    if T == 1:
        return np.array([-32768], dtype=np.int16)
    if T == 2:
        return np.array([32767, -32768], dtype=np.int16)
    m = np.zeros(T, dtype=np.int64)
    m[0] = int(rng.integers(20000, 30001))
    rest = 65535 - int(m[0])
    w = rng.integers(1, 20001, size=T - 1).astype(np.float64)
    m[1:] = np.minimum(np.floor(w * (rest / w.sum())).astype(np.int64), 32767)
    rem = 65535 - int(m.sum())
    for k in range(1, T):
        add = min(rem, 32767 - int(m[k]))
        m[k] += add
        rem -= add
    assert rem == 0 and int(m.sum()) == 65535
    h = m * rng.choice([-1, 1], size=T)
    return h.astype(np.int16)


def worst_taps(T):
    """T taps <= 0 at the admitted bound: -32768 first, the rest sharing 32767 (sum |h| = 65535)."""
    m = np.zeros(T, dtype=np.int64)
    m[0] = 32768
    m[1:] = 32767 // (T - 1)
    m[1: 1 + 32767 - int(m[1:].sum())] += 1
    assert int(m.sum()) == 65535
    return (-m).astype(np.int16)
