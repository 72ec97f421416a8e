"""The antenna array as include/galsynth.h defines it (gal_synth_steer_make, gal_synth_array_phase, gal_synth_iq_array,
gal_synth_run_array), in numpy -- TEST INFRASTRUCTURE: the product never imports this."""
import numpy as np

GAL_ARRAY_MAX_ELEM = 8
GAL_STEER_GAIN_MAX = 1023
LAMBDA_E1 = 299792458.0 / 1575420000.0


def steer_index(phase):
    """The table index of a phase in 2^-32 cycles: rounded, not truncated."""
    return (((np.asarray(phase, dtype=np.int64) & 0xffffffff) + (1 << 21)) >> 22) & 1023


def steer_make(gain_q7, phase, cos1024):
    """(w_re, w_im) = ((g C[i] + 64) >> 7, (g C[(i - 256) & 1023] + 64) >> 7), i = steer_index(phase); arrays broadcast."""
    g = np.asarray(gain_q7, dtype=np.int64)
    assert g.min() >= 0 and g.max() <= GAL_STEER_GAIN_MAX
    C = np.asarray(cos1024, dtype=np.int64)
    i = steer_index(phase)
    return (g * C[i] + 64) >> 7, (g * C[(i - 256) & 1023] + 64) >> 7


def array_phase(enu_m, az_rad, el_rad):
    """llround((cyc - floor(cyc)) 2^32) mod 2^32, cyc = (enu . u) / lambda, u = (sin az cos el, cos az cos el, sin el); in double."""
    e = np.asarray(enu_m, dtype=np.float64)
    az, el = np.float64(az_rad), np.float64(el_rad)
    ce = np.cos(el)
    u = (np.sin(az) * ce, np.cos(az) * ce, np.sin(el))
    cyc = (e[0] * u[0] + e[1] * u[1] + e[2] * u[2]) / np.float64(LAMBDA_E1)
    v = (cyc - np.floor(cyc)) * 4294967296.0
    return int(np.floor(v + 0.5)) & 0xffffffff  # (v >= 0: round half away from zero is round half up)


def needs_int64(weights):
    """weights: [n_epochs, n_elem, n_parts, 2].  True where some (epoch, element) has sum_k (|w_re| + |w_im|) > 65535."""
    w = np.abs(np.asarray(weights, dtype=np.int64))
    return bool((w.sum(axis=(2, 3)) > 65535).any())


def array(parts, weights, samples_per_epoch):
    """parts: [n_parts, n_epochs * samples_per_epoch * 2] int16 (interleaved I, Q); weights: [n_epochs, n_elem, n_parts, 2] (w_re, w_im),
    -32767 .. 32767.  Returns (y int16 [n_elem, n_val], values the clamp changed):
    AI = sum_k (xI w_re - xQ w_im), AQ = sum_k (xI w_im + xQ w_re), y = clamp((A + 2048) >> 12), int64 arithmetic."""
    x = np.asarray(parts, dtype=np.int16)
    w = np.asarray(weights, dtype=np.int64)
    n_parts, n_val = x.shape
    n_epochs, n_elem = w.shape[0], w.shape[1]
    assert w.shape == (n_epochs, n_elem, n_parts, 2) and n_val == n_epochs * samples_per_epoch * 2
    assert 1 <= n_elem <= GAL_ARRAY_MAX_ELEM and w.min() >= -32767 and w.max() <= 32767
    xI = x[:, 0::2].astype(np.int64).reshape(n_parts, n_epochs, samples_per_epoch)
    xQ = x[:, 1::2].astype(np.int64).reshape(n_parts, n_epochs, samples_per_epoch)
    y = np.zeros((n_elem, n_val), dtype=np.int16)
    sat = 0
    for a in range(n_elem):
        AI = np.zeros((n_epochs, samples_per_epoch), dtype=np.int64)
        AQ = np.zeros((n_epochs, samples_per_epoch), dtype=np.int64)
        for k in range(n_parts):
            re, im = w[:, a, k, 0][:, None], w[:, a, k, 1][:, None]
            AI += xI[k] * re - xQ[k] * im
            AQ += xI[k] * im + xQ[k] * re
        for rail, A in ((0, AI), (1, AQ)):
            v = (A.reshape(-1) + 2048) >> 12
            c = np.clip(v, -32768, 32767)
            sat += int(np.count_nonzero(c != v))
            y[a, rail::2] = c.astype(np.int16)
    return y, sat
