"""Geometric reflectors as include/galsynth.h defines them (gal_synth_iq_refl, gal_synth_run_refl, gal_synth_refl_geom, _row), in numpy
-- TEST INFRASTRUCTURE: the product never imports this.  The echo pass of mpath_model with a delay of D + F / 4096 samples."""
import math

import numpy as np

import mpath_model
from mpath_model import GAL_ECHO_LINES, GAL_ECHO_MAX, GAL_ECHO_MAX_DELAY, GAL_GAIN_MAX, H, _llround

REFL_DTYPE = np.dtype([("gain_q7", "<u2"), ("delay", "<u2"), ("ph0", "<u4"), ("dph", "<i4"), ("frac_q12", "<u2"), ("reserved", "<u2")])
GROUND, WALL = 0, 1
C_LIGHT = 299792458.0
LAMBDA = 299792458.0 / 1575420000.0


def rows(n_epochs, n_echo, gain_q7=0, delay=0, ph0=0, dph=0, frac_q12=0):
    """A reflector table [n_epochs, n_echo]; every argument broadcasts over it."""
    r = np.zeros((n_epochs, n_echo), dtype=REFL_DTYPE)
    r["gain_q7"], r["delay"], r["ph0"], r["dph"], r["frac_q12"] = gain_q7, delay, ph0, dph, frac_q12
    return r


def from_echo(echo_rows):
    """gal_iq_echo_t rows as gal_iq_refl_t rows with F = 0: the same bytes."""
    e = np.ascontiguousarray(echo_rows, dtype=mpath_model.ECHO_DTYPE)
    assert not e["reserved"].any()
    return e.view(REFL_DTYPE).reshape(e.shape)


def interpolate(x, hist, row, samples_per_epoch):
    """u (I, Q as int64, one per sample) of one echo: x the part's interleaved int16 values of the call, hist the 2 x 1024 values in
    front of it, row the echo's column of the table [n_epochs].  Also returns a and b (for the tests of the bound)."""
    N = samples_per_epoch
    ext = np.concatenate([np.asarray(hist, dtype=np.int16), np.asarray(x, dtype=np.int16)]).astype(np.int64)
    n = np.arange(row.shape[0] * N, dtype=np.int64)
    per = lambda f: np.repeat(row[f].astype(np.int64), N)  # noqa: E731
    F = per("frac_q12")
    ja = n - per("delay") + H
    jb = np.where(F > 0, ja - 1, ja)  # (F = 0: b is not read)
    assert jb.min() >= 0
    a = np.stack([ext[2 * ja], ext[2 * ja + 1]])
    b = np.stack([ext[2 * jb], ext[2 * jb + 1]])
    assert np.abs(F * (b - a)).max(initial=0) < 1 << 28
    u = a + ((F * (b - a) + 2048) >> 12)
    return u, a, b


def echo_terms(x, hist, row, samples_per_epoch, cos1024):
    """The int64 terms A r (I and Q, one per sample) of one echo."""
    N = samples_per_epoch
    (uI, uQ), _, _ = interpolate(x, hist, row, N)
    m = np.arange(row.shape[0] * N, dtype=np.int64) % N
    per = lambda f: np.repeat(row[f].astype(np.int64), N)  # noqa: E731
    i = ((per("ph0") + m * per("dph")) % (1 << 32)) >> 22
    C = np.asarray(cos1024, dtype=np.int64)
    c, s = C[i], C[(i - 256) & 1023]
    rI = (uI * c - uQ * s + 2048) >> 12
    rQ = (uI * s + uQ * c + 2048) >> 12
    assert max(np.abs(rI).max(initial=0), np.abs(rQ).max(initial=0)) <= 65536
    A = per("gain_q7")
    return A * rI, A * rQ


def check(refl_rows):
    r = np.asarray(refl_rows, dtype=REFL_DTYPE)
    if r.size:
        assert r["gain_q7"].max() <= GAL_GAIN_MAX and r["frac_q12"].max() <= 4095 and not r["reserved"].any()
        assert (r["delay"].astype(np.int64) + (r["frac_q12"] > 0)).max() <= H


def refl(parts, gains, samples_per_epoch, part_of_echo, refl_rows, cos1024, hist=None, acc=np.int64):
    """parts [n_parts, n_epochs * N * 2] int16; gains [n_epochs, n_parts]; refl_rows [n_epochs, n_echo] REFL_DTYPE; hist [n_parts,
    2048] int16 = the 1024 samples in front of the call (None: zeros).  acc = np.int32 forms w as the narrow kernel instance does
    (wrapping).  Returns (y int16, values the clamp changed, the new hist)."""
    x = np.asarray(parts, dtype=np.int16)
    g = np.asarray(gains, dtype=np.int64)
    n_parts, n_val = x.shape
    n_epochs = g.shape[0]
    N = samples_per_epoch
    assert g.shape == (n_epochs, n_parts) and n_val == n_epochs * N * 2
    assert g.min() >= 0 and g.max() <= GAL_GAIN_MAX
    r = np.asarray(refl_rows, dtype=REFL_DTYPE).reshape(n_epochs, -1)
    n_echo = r.shape[1]
    assert n_echo <= GAL_ECHO_MAX and len(part_of_echo) == n_echo
    check(r)
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
    w = (w + 64).astype(acc).astype(np.int64)
    v = w >> 7
    y = np.clip(v, -32768, 32767)
    new_hist = np.concatenate([np.asarray(hist, dtype=np.int16), x], axis=1)[:, -2 * H:]
    return y.astype(np.int16), int(np.count_nonzero(y != v)), new_hist


class Lines(mpath_model.Lines):
    """The handle's 64 history lines, shared by both passes: call() is gal_synth_iq_mpath, call_refl() gal_synth_iq_refl."""

    def call_refl(self, parts, gains, samples_per_epoch, part_of_echo, refl_rows, hist_id=None):
        n_parts = len(parts)
        ids = list(range(n_parts)) if hist_id is None else [int(i) for i in hist_id]
        named = [i for i in ids if i >= 0]
        assert len(set(named)) == len(named) and all(ids[int(p)] >= 0 for p in part_of_echo)
        hist = np.stack([self.lines[i] if i >= 0 else np.zeros(2 * H, np.int16) for i in ids])
        y, sat, new = refl(parts, gains, samples_per_epoch, part_of_echo, refl_rows, self.cos, hist)
        for k, i in enumerate(ids):
            if i >= 0:
                self.lines[i] = new[k]
        return y, sat


def needs_int64(gains, refl_rows):
    """True where some epoch has sum g + 2 sum A > 65535: the int32 accumulator could wrap."""
    g = np.asarray(gains, dtype=np.int64).sum(axis=1)
    r = np.asarray(refl_rows, dtype=REFL_DTYPE).reshape(g.shape[0], -1)
    return bool((g + 2 * r["gain_q7"].astype(np.int64).sum(axis=1)).max() > 65535)


def geom(kind, p, az, el):
    """gal_synth_refl_geom, operation for operation: the excess path in metres, -1.0 where there is no echo."""
    if kind == GROUND:
        return 2.0 * p[0] * math.sin(el) if el > 0.0 else -1.0
    x = -2.0 * p[0] * math.cos(el) * math.cos(az - p[1])
    return x if x > 0.0 else -1.0


def phase(excess_m, refl_phase_deg):
    cyc = -excess_m / LAMBDA + refl_phase_deg / 360.0
    return _llround((cyc - math.floor(cyc)) * 4294967296.0) % (1 << 32)


def row(excess_now_m, excess_next_m, rel_db, refl_phase_deg, sample_rate, samples_per_epoch, slot_gain_q7):
    """gal_synth_refl_row, operation for operation: (gain_q7, delay, ph0, dph, frac_q12, 0)."""
    if excess_now_m < 0.0:
        return (0, 0, 0, 0, 0, 0)
    t = excess_now_m / C_LIGHT * sample_rate
    D = int(math.floor(t))
    F = _llround((t - D) * 4096.0)
    if F == 4096:
        D, F = D + 1, 0
    assert D + (F > 0) <= GAL_ECHO_MAX_DELAY
    A = min(GAL_GAIN_MAX, (int(slot_gain_q7) * _llround(4096.0 * 10.0 ** (rel_db / 20.0)) + 2048) >> 12)
    ph0 = phase(excess_now_m, refl_phase_deg)
    dph = 0
    if excess_next_m >= 0.0:
        d = (phase(excess_next_m, refl_phase_deg) - ph0) % (1 << 32)
        d -= (d >> 31) << 32  # the wrapped signed difference
        dph = _llround(d / float(samples_per_epoch))
    return (A, D, ph0, dph, F, 0)


assert GAL_ECHO_LINES == 64
