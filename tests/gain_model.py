"""Per-satellite signal power as include/galsynth.h defines it (gal_synth_gain_q7, gal_synth_iq_wsum, gal_synth_run_gains), in numpy --
TEST INFRASTRUCTURE: the product never imports this."""
import numpy as np

GAL_GAIN_UNITY = 128
GAL_GAIN_MAX = 32767
REF_DISTANCE_M = 23222000.0  # Galileo's nominal altitude
R2D = 57.2957795131  # the reference's constant (include/constants.h:178)


def boresight_index(elev_rad):
    off = (90.0 - np.float64(elev_rad) * R2D) / 5.0
    return 0 if off <= 0.0 else 36 if off >= 36.0 else int(off)


def gain_q7(d_m, elev_rad, pattern_db=None, offset_db=0.0):
    """min(32767, (int)(128 (23222000 / d) 10^(-pattern_db[ibs] / 20) 10^(offset_db / 20))), in double, left to right."""
    ant = np.float64(1.0) if pattern_db is None else np.float64(10.0) ** (-np.float64(pattern_db[boresight_index(elev_rad)]) / 20.0)
    v = np.float64(128.0) * (np.float64(REF_DISTANCE_M) / np.float64(d_m)) * ant * np.float64(10.0) ** (np.float64(offset_db) / 20.0)
    return GAL_GAIN_MAX if v >= 32767.0 else int(v)


def wsum(parts, gains, samples_per_epoch):
    """parts: [n_parts, n_epochs * samples_per_epoch * 2] int16 (interleaved I, Q); gains: [n_epochs, n_parts], 0 .. 32767.
    Returns (y int16, values the clamp changed): y[j] = clamp((sum_k g[e(j), k] parts[k, j] + 64) >> 7), e(j) = (j / 2) / N."""
    x = np.asarray(parts, dtype=np.int16)
    g = np.asarray(gains, dtype=np.int64)
    n_parts, n_val = x.shape
    n_epochs = g.shape[0]
    assert g.shape == (n_epochs, n_parts) and n_val == n_epochs * samples_per_epoch * 2
    assert g.min() >= 0 and g.max() <= GAL_GAIN_MAX
    w = np.zeros(n_val, dtype=np.int64)
    per_value = np.repeat(g, 2 * samples_per_epoch, axis=0)  # [n_val, n_parts]
    for k in range(n_parts):
        w += per_value[:, k] * x[k].astype(np.int64)
    v = (w + 64) >> 7
    y = np.clip(v, -32768, 32767)
    return y.astype(np.int16), int(np.count_nonzero(y != v))


def slot_alone(params, slot):
    """The batch with only the records of `slot` active (x_s of the definition)."""
    p = params.copy()
    keep = p["prn"][:, slot].copy()
    p["prn"][:, :] = 0
    p["prn"][:, slot] = keep
    return p
