"""Per-satellite multipath as include/galsynth.h defines it (gal_synth_iq_mpath, gal_synth_run_mpath, gal_synth_mpath_make, _row), in
numpy -- TEST INFRASTRUCTURE: the product never imports this."""
import math

import numpy as np

GAL_GAIN_MAX = 32767
GAL_ECHO_MAX = 32
GAL_ECHO_MAX_DELAY = 1024
GAL_ECHO_LINES = 64
ECHO_DTYPE = np.dtype([("gain_q7", "<u2"), ("delay", "<u2"), ("ph0", "<u4"), ("dph", "<i4"), ("reserved", "<u4")])
H = GAL_ECHO_MAX_DELAY


def rows(n_epochs, n_echo, gain_q7=0, delay=0, ph0=0, dph=0):
    """An echo table [n_epochs, n_echo]; every argument broadcasts over it."""
    r = np.zeros((n_epochs, n_echo), dtype=ECHO_DTYPE)
    r["gain_q7"], r["delay"], r["ph0"], r["dph"] = gain_q7, delay, ph0, dph
    return r


def echo_terms(x, hist, row, samples_per_epoch, cos1024):
    """The int64 terms A r (I and Q, one per sample) of one echo: x the part's interleaved int16 values of the call, hist the 2 x 1024
    values in front of it, row the echo's column of the table [n_epochs]."""
    N = samples_per_epoch
    n_epochs = row.shape[0]
    ext = np.concatenate([np.asarray(hist, dtype=np.int16), np.asarray(x, dtype=np.int16)]).astype(np.int64)
    n = np.arange(n_epochs * N, dtype=np.int64)
    m = n % N
    per = lambda f: np.repeat(row[f].astype(np.int64), N)  # noqa: E731
    j = n - per("delay") + H
    assert j.min() >= 0
    uI, uQ = ext[2 * j], ext[2 * j + 1]
    i = ((per("ph0") + m * per("dph")) % (1 << 32)) >> 22
    C = np.asarray(cos1024, dtype=np.int64)
    c, s = C[i], C[(i - 256) & 1023]
    rI = (uI * c - uQ * s + 2048) >> 12
    rQ = (uI * s + uQ * c + 2048) >> 12
    assert max(np.abs(rI).max(), np.abs(rQ).max()) <= 65536
    A = per("gain_q7")
    return A * rI, A * rQ


def mpath(parts, gains, samples_per_epoch, part_of_echo, echo_rows, cos1024, hist=None):
    """parts [n_parts, n_epochs * N * 2] int16; gains [n_epochs, n_parts]; echo_rows [n_epochs, n_echo] ECHO_DTYPE; hist [n_parts,
    2048] int16 = the 1024 samples in front of the call (None: zeros).  Returns (y int16, values the clamp changed, the new hist)."""
    x = np.asarray(parts, dtype=np.int16)
    g = np.asarray(gains, dtype=np.int64)
    n_parts, n_val = x.shape
    n_epochs = g.shape[0]
    N = samples_per_epoch
    assert g.shape == (n_epochs, n_parts) and n_val == n_epochs * N * 2
    assert g.min() >= 0 and g.max() <= GAL_GAIN_MAX
    r = np.asarray(echo_rows, dtype=ECHO_DTYPE).reshape(n_epochs, -1)
    n_echo = r.shape[1]
    assert n_echo <= GAL_ECHO_MAX and len(part_of_echo) == n_echo
    if n_echo:
        assert r["gain_q7"].max() <= GAL_GAIN_MAX and r["delay"].max() <= H and not r["reserved"].any()
    if hist is None:
        hist = np.zeros((n_parts, 2 * H), dtype=np.int16)
    w = np.zeros(n_val, dtype=np.int64)
    per_value = np.repeat(g, 2 * N, axis=0)
    for k in range(n_parts):
        w += per_value[:, k] * x[k].astype(np.int64)
    for e in range(n_echo):
        p = int(part_of_echo[e])
        assert 0 <= p < n_parts
        tI, tQ = echo_terms(x[p], hist[p], r[:, e], N, cos1024)
        w[0::2] += tI
        w[1::2] += tQ
    v = (w + 64) >> 7
    y = np.clip(v, -32768, 32767)
    new_hist = np.concatenate([np.asarray(hist, dtype=np.int16), x], axis=1)[:, -2 * H:]
    return y.astype(np.int16), int(np.count_nonzero(y != v)), new_hist


class Lines:
    """The handle's 64 history lines: call() is gal_synth_iq_mpath with hist_id, reset() gal_synth_mpath_reset."""

    def __init__(self, cos1024):
        self.cos = cos1024
        self.reset()

    def reset(self):
        self.lines = np.zeros((GAL_ECHO_LINES, 2 * H), dtype=np.int16)

    def call(self, parts, gains, samples_per_epoch, part_of_echo, echo_rows, hist_id=None):
        n_parts = len(parts)
        ids = list(range(n_parts)) if hist_id is None else [int(i) for i in hist_id]
        named = [i for i in ids if i >= 0]
        assert len(set(named)) == len(named) and all(ids[int(p)] >= 0 for p in part_of_echo)
        hist = np.stack([self.lines[i] if i >= 0 else np.zeros(2 * H, np.int16) for i in ids])
        y, sat, new = mpath(parts, gains, samples_per_epoch, part_of_echo, echo_rows, self.cos, hist)
        for k, i in enumerate(ids):
            if i >= 0:
                self.lines[i] = new[k]
        return y, sat


def needs_int64(gains, echo_rows):
    """True where some epoch has sum g + 2 sum A > 65535: the int32 accumulator could wrap."""
    g = np.asarray(gains, dtype=np.int64).sum(axis=1)
    r = np.asarray(echo_rows, dtype=ECHO_DTYPE).reshape(g.shape[0], -1)
    return bool((g + 2 * r["gain_q7"].astype(np.int64).sum(axis=1)).max() > 65535)


def _llround(x):
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def make(delay_s, rel_db, phase_deg, fade_hz, sample_rate):
    """gal_synth_mpath_make, operation for operation."""
    turns = phase_deg / 360.0
    return {"delay": _llround(delay_s * sample_rate), "alpha_q12": _llround(4096.0 * 10.0 ** (rel_db / 20.0)),
            "ph0": _llround((turns - math.floor(turns)) * 4294967296.0) % (1 << 32), "dph": _llround(fade_hz / sample_rate * 4294967296.0)}


def row(echo, slot_gain_q7, epoch, samples_per_epoch):
    """gal_synth_mpath_row: (gain_q7, delay, ph0, dph, 0)."""
    A = min(GAL_GAIN_MAX, (int(slot_gain_q7) * echo["alpha_q12"] + 2048) >> 12)
    return (A, echo["delay"], (echo["ph0"] + epoch * samples_per_epoch * echo["dph"]) % (1 << 32), echo["dph"], 0)


def column(echo, slot_gains, first_epoch, samples_per_epoch):
    out = np.zeros(len(slot_gains), dtype=ECHO_DTYPE)
    for e, g in enumerate(slot_gains):
        out[e] = row(echo, g, first_epoch + e, samples_per_epoch)
    return out
