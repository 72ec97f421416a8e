"""A numpy statement of the correlator bank of include/galsynth.h (gal_synth_correlate): integers only, so the
kernel's int64 sums must come out exactly.  Also the host helpers gal_corr_from_epoch and gal_corr_cn0 restated."""
import math

import numpy as np

HALF_CHIPS = 8184
L = HALF_CHIPS << 32
FIELDS = ("prn", "max_periods", "code_ph0", "code_dph", "carr_ph0", "carr_dph", "delay0", "delay_step", "n_delay", "dopp0", "dopp_step",
          "n_dopp")
DEFAULTS = {"max_periods": 1, "carr_ph0": 0, "carr_dph": 0, "delay0": 0, "delay_step": 1, "n_delay": 1, "dopp0": 0, "dopp_step": 0, "n_dopp": 1}


def full(req):
    d = dict(DEFAULTS)
    d.update(req)
    return d


def values(buf, fmt, n_samples):
    """The interleaved I/Q values v[j], j < 2 n_samples, of a buffer (uint8 array of its bytes) in format "ishort" | "ibyte" | "ibit"."""
    b = np.ascontiguousarray(buf).view(np.uint8).ravel()
    if fmt in ("ishort", 0):
        return b[: 4 * n_samples].view("<i2").astype(np.int64)
    if fmt in ("ibyte", 1):
        return b[: 2 * n_samples].view(np.int8).astype(np.int64)
    bits = np.unpackbits(b[: (n_samples + 3) // 4])[: 2 * n_samples]  # MSB first
    return bits.astype(np.int64) * 2 - 1


def replicas(tables, prn):
    """(b, c): the E1B / E1C primary code of `prn` times the BOC(1,1) sub-carrier, +-1 per half chip: a set table bit is -1, an even
    half chip carries -1 (sboc: each chip x becomes [-x, +x])."""
    h = np.arange(HALF_CHIPS)
    chip = h >> 1
    sub = np.where(h & 1, 1, -1)
    out = []
    for name in ("e1b", "e1c"):
        bit = (tables[name][prn - 1][chip >> 5] >> (chip & 31).astype(np.uint32)) & 1
        out.append((np.where(bit, -1, 1) * sub).astype(np.int64))
    return out


def correlate(v, req, tables):
    """out[m, d, k, 4] int64 of one request over the samples (v[2n], v[2n+1])."""
    q = full(req)
    v = np.asarray(v, dtype=np.int64)
    n_samples = v.size // 2
    I, Q = v[0::2], v[1::2]
    M, D, K = q["max_periods"], q["n_dopp"], q["n_delay"]
    assert q["code_ph0"] + (n_samples - 1) * q["code_dph"] < 1 << 64
    n = np.arange(n_samples, dtype=np.uint64)
    P = np.uint64(q["code_ph0"]) + n * np.uint64(q["code_dph"])
    hi = (P >> np.uint64(32)).astype(np.int64)
    m = hi // HALF_CHIPS
    h = hi - m * HALF_CHIPS
    keep = int(np.searchsorted(m, M, side="left"))  # m is non-decreasing: the samples of the periods < M
    I, Q, m, h, n = I[:keep], Q[:keep], m[:keep], h[:keep], n[:keep].astype(np.int64)
    out = np.zeros((M, D, K, 4), dtype=np.int64)
    if keep == 0:
        return out
    b, c = replicas(tables, q["prn"])
    cos, sin = tables["cos512"].astype(np.int64), tables["sin512"].astype(np.int64)
    periods = np.unique(m)
    starts = np.searchsorted(m, periods, side="left")
    delays = (q["delay0"] + np.arange(K, dtype=np.int64) * q["delay_step"]) % HALF_CHIPS
    for d in range(D):
        step = (q["carr_dph"] + q["dopp0"] + d * q["dopp_step"]) % (1 << 32)
        phi = (q["carr_ph0"] + n * step) % (1 << 32)  # n step < 2^32 2^32: exact in int64 for n < 2^31
        i = phi >> 23
        re = I * cos[i] + Q * sin[i]
        im = Q * cos[i] - I * sin[i]
        for k0 in range(0, K, 128):
            hk = (h[None, :] - delays[k0:k0 + 128, None]) % HALF_CHIPS
            for col, (rep, x) in enumerate(((b, re), (b, im), (c, re), (c, im))):
                prod = rep[hk] * x[None, :]
                out[periods, d, k0:k0 + 128, col] = np.add.reduceat(prod, starts, axis=1).T
    return out


def from_epoch(rec, sample_rate, sample_offset=0):
    """gal_corr_from_epoch: round to nearest, ties away from zero (C's llround)."""
    def llround(x):
        return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)

    two32 = 4294967296.0
    dph = llround(2.0 * float(rec["f_code"]) / sample_rate * two32)
    cdph = llround(float(rec["f_carr"]) / sample_rate * two32)
    q = {"prn": int(rec["prn"]), "code_dph": dph, "carr_dph": cdph, "carr_ph0": 0,
         "code_ph0": (llround(2.0 * float(rec["code_phase0"]) * two32) + sample_offset * dph) % L}
    if int(rec["flags"]) & 1:
        fr = float(rec["carr_phase0"]) - math.floor(float(rec["carr_phase0"]))
        q["carr_ph0"] = (llround(fr * two32) + sample_offset * cdph) % (1 << 32)
    return q


def cn0(out, req, k_prompt, k_noise, d, sample_rate):
    """gal_corr_cn0: (cn0_dbhz, Pp / Pn) over the whole periods 1 .. max_periods - 2, or None where Pp <= Pn."""
    q = full(req)
    a = np.asarray(out, dtype=np.float64)[1:q["max_periods"] - 1, d]
    pp = float(np.mean(np.sum(a[:, k_prompt] ** 2, axis=1)))
    pn = float(np.mean(np.sum(a[:, k_noise] ** 2, axis=1)))
    if not pp > pn or not pn > 0:
        return None
    T = L / q["code_dph"] / sample_rate
    return 10.0 * math.log10((pp - pn) / (pn * T / 2.0)), pp / pn
