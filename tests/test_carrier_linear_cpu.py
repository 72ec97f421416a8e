"""k_synth_g's linear carrier start (synth_group.hip, SG_LIN_CYCLES), modelled with exact arithmetic: the loader lane's
T_c = fma(511, pm, 2^20 + 512 + 2^-26), a group's t = fma(16 g, 511 |d|, T_c) and the 15 additions of 511 |d| behind it, each a
correctly rounded double made from fractions.Fraction.  Every sample the kernel decides itself (fraction word of t >= 128) must read
the table entry the reference reads from its sequentially stepped phase, `(int)(511 p) & 511`, and no sample's index may leave the
2048-entry table -- for carriers up to the host gate's limit (1024 + 16) |d| <= 2 and both signs of the step.  The gate itself is
checked on both sides of that limit through the hooks build's host-only plan."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

LUT_N = 2048                                  # SG_LUT_LIN_N
BIAS = 1049088.0 + 2.0 ** -26                 # SG_BIAS
AMB = 128                                     # SG_AMB: a smaller fraction word leaves the sample to k_repair_g
LIMIT = 2.0                                   # SG_LIN_CYCLES
CHUNK = 1024


def _largest_admitted_step():
    """The largest |d| the host gate admits: it compares the ROUNDED product fl(1040 |d|) with 2."""
    d = LIMIT / (CHUNK + 16)
    while float(CHUNK + 16) * d > LIMIT:
        d = float(np.nextafter(d, 0.0))
    while float(CHUNK + 16) * float(np.nextafter(d, 1.0)) <= LIMIT:
        d = float(np.nextafter(d, 1.0))
    return d


D_MAX = _largest_admitted_step()


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _entry_k(i):
    """The table builder's rule: entry i holds LUT[k], conjugate table LUT[-k]; i < 512: the mirrored phase is still negative."""
    assert 0 <= i < LUT_N
    return i - 511 if i < 512 else (i - 512) % 511


def _reference_indices(p0, d, n):
    """(int)(511 p) & 511 before every one of n samples, the phase stepped as the reference does (p += d; p -= (long)p)."""
    out = []
    p = p0
    for _ in range(n):
        out.append(int(511.0 * p) & 511)
        p = p + d
        p = p - float(int(p))
    return out


def _kernel_indices(p0, d, n):
    """Per sample: (LUT index read, fraction word, table entry) by the kernel's arithmetic from the chunk's checkpoint p0."""
    neg = math.copysign(1.0, d) < 0.0
    pm = -p0 if neg else p0                   # the mirrored phase
    dabs = abs(d)
    if dabs == 0.0:                           # a carrier that stands still: the middle of the entry of its phase
        k = int(511.0 * pm)
        pm = (float(k if k >= 0 else k - 1) + 0.5) * (1.0 / 511.0)
    c511 = 511.0 * dabs
    tc = _fma(511.0, pm, BIAS)
    out = []
    for g in range((n + 15) // 16):
        t = _fma(float(16 * g), c511, tc)
        for _ in range(16):
            assert 2.0 ** 20 <= t < 2.0 ** 21
            hi = int(math.floor(t))
            i = hi - 2 ** 20
            fw = int((Fraction(t) - hi) * 2 ** 32)
            assert Fraction(fw, 2 ** 32) == Fraction(t) - hi  # 32 fraction bits exactly
            assert 0 <= i < LUT_N, (p0, d, g, i)
            k = _entry_k(i)
            out.append(((-k if neg else k) & 511, fw, i))
            t = t + c511
    return out[:((n + 15) // 16) * 16]


def _check(p0, d, n=CHUNK):
    ref = _reference_indices(p0, d, n)
    ker = _kernel_indices(p0, d, n)
    decided = 0
    top = 0
    for u in range(n):
        k, fw, i = ker[u]
        top = max(top, i)
        if fw >= AMB:
            decided += 1
            assert k == ref[u], (p0, d, u, k, ref[u], fw)
    return decided, top


def _cases():
    rng = np.random.default_rng(20251020)
    below1 = [1.0 - 2.0 ** -53, 1.0 - 2.0 ** -52, 1.0 - 3 * 2.0 ** -53, 1.0 - 2.0 ** -30]
    below0 = [-2.0 ** -1074, -2.0 ** -60, -2.0 ** -30, -1.0 / 511.0 + 2.0 ** -40]
    edges = below1 + below0 + [0.0, 2.0 ** -60, -(1.0 - 2.0 ** -53), 0.5, -0.5]
    steps = [D_MAX, -D_MAX, 0.0, -0.0, D_MAX / 2, -D_MAX / 2, 3500.0 / 2.6e6, -3500.0 / 2.6e6, 2.0 ** -40, -2.0 ** -40, 0.5 / 511.0,
             1.0 / (16 * 511.0)]  # (0.5 / 511, 1 / (16 x 511): half an entry per sample, an entry per group -- phases that start ON an
                                  # index boundary come back to one again and again)
    cases = [(p, d) for p in edges for d in steps]
    for _ in range(40):
        cases.append((float(rng.uniform(-1.0, 1.0)), float(rng.uniform(-D_MAX, D_MAX))))
    # adversarial: 511 p of sample n lands eps beside an integer, on either side of the undecided band and inside it
    for eps in (2.0 ** -25, -2.0 ** -25, 2.0 ** -26 + 2.0 ** -29, -2.0 ** -26 - 2.0 ** -29, 2.0 ** -27, -2.0 ** -27, 2.0 ** -33, 0.0):
        for d in (D_MAX, -D_MAX, 1234.5 / 2.6e6, -0.3 * D_MAX):
            n = int(rng.integers(1, CHUNK))
            K = int(rng.integers(1, 511))
            pm = float((Fraction(K) + Fraction(eps)) / 511 - n * Fraction(abs(d)))
            pm = pm - math.floor(pm)          # a mirrored phase in [0, 1)
            cases.append((math.copysign(pm, d), d))
    return cases


def test_decided_samples_read_the_reference_entry_and_stay_inside_the_table():
    assert float(CHUNK + 16) * D_MAX <= LIMIT < float(CHUNK + 16) * float(np.nextafter(D_MAX, 1.0))
    tops = []
    undecided = 0
    cases = _cases()
    for p0, d in cases:
        assert -1.0 < p0 < 1.0
        # a phase carries the sign of the steps that made it, or the other one right behind a Doppler sign change: both
        dec, top = _check(p0, d)
        undecided += CHUNK - dec
        tops.append(top)
    print("%d cases, %d of %d samples undecided, highest entry %d of %d" % (len(cases), undecided, len(cases) * CHUNK, max(tops), LUT_N))
    # the table's last cycle is reached, and 512 + 3 x 511 bounds the index
    assert 512 + 2 * 511 <= max(tops) < 512 + 3 * 511


def test_ragged_tail_computes_whole_groups():
    """An epoch's last chunk ends inside a group: the lane still runs its 16 samples, stores the first ones -- no index leaves the table."""
    for n in (100, 1, 1009):
        _check(1.0 - 2.0 ** -53, D_MAX, n)
        _kernel_indices(-(1.0 - 2.0 ** -53), -D_MAX, n)


def _hooks(pkg):
    lib = pkg.synth.load_library(hooks=True)
    lib.gal_hooks_plan_host_ms.restype = ctypes.c_double
    lib.gal_hooks_plan_host_ms.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32]
    lib.gal_hooks_plan_host_array.restype = ctypes.c_void_p
    lib.gal_hooks_plan_host_array.argtypes = [ctypes.c_char_p]
    return lib


def host_verdict(pkg, p, n_samp, rate=2.6e6, flags=0):
    """(kernel family, bisection instances, linear carrier start) the plan's gates give these records."""
    lib = _hooks(pkg)
    cfg = pkg.synth._Cfg(float(rate), int(n_samp), int(p.shape[1]), 0, 0, 0, int(flags))
    p = np.ascontiguousarray(p)
    assert lib.gal_hooks_plan_host_ms(ctypes.byref(cfg), p.ctypes.data, p.shape[0], None, 1) >= 0.0
    return tuple(int(lib.gal_hooks_plan_host_array(k) or 0) - 1 for k in (b"family", b"search", b"linear"))


def f_carr_at_limit(rate, above=False):
    """The largest Doppler the gate admits at this rate, by its own arithmetic -- (1024 + 16) x |fl(f x fl(1 / rate))| <= 2 --
    or the next double above it."""
    delt = 1.0 / rate
    f = LIMIT / (CHUNK + 16) * rate
    while float(CHUNK + 16) * abs(f * delt) > LIMIT:
        f = float(np.nextafter(f, 0.0))
    while float(CHUNK + 16) * abs(float(np.nextafter(f, np.inf)) * delt) <= LIMIT:
        f = float(np.nextafter(f, np.inf))
    return float(np.nextafter(f, np.inf)) if above else f


@pytest.mark.parametrize("rate", [2.6e6, 4.0e6, 10.0e6, 16.0e6])
def test_host_gate_on_both_sides_of_the_limit(pkg, rate, monkeypatch):
    monkeypatch.delenv("GAL_G_LINEAR", raising=False)
    n = 2 * 1024 + 100
    p = pkg.workloads.make_synthetic(n_epochs=3, n_chan=12, n_slots=16, samples_per_epoch=n, sample_rate=rate, seed=77)
    assert host_verdict(pkg, p, n, rate) == (1, 0, 1)       # +-3.5 kHz: inside at every rate
    f_in, f_out = f_carr_at_limit(rate), f_carr_at_limit(rate, above=True)
    assert abs(f_in / rate - 2.0 / 1040.0) < 1e-12 and f_out > f_in
    for sign in (1.0, -1.0):
        q = p.copy()
        q["f_carr"][1, 5] = sign * f_in
        assert host_verdict(pkg, q, n, rate) == (1, 0, 1), (rate, sign)
        q["f_carr"][1, 5] = sign * f_out                    # ONE record beyond the limit: the whole batch takes the legacy start
        assert host_verdict(pkg, q, n, rate) == (1, 0, 0), (rate, sign)
    q = p.copy()
    q["f_carr"][:, 0] = 0.0                                 # a standing carrier is inside
    assert host_verdict(pkg, q, n, rate) == (1, 0, 1)
    monkeypatch.setenv("GAL_G_LINEAR", "0")                 # the hooks build's switch: the legacy start for every batch
    assert host_verdict(pkg, p, n, rate) == (1, 0, 0)
    monkeypatch.setenv("GAL_G_LINEAR", "1")                 # ... which never forces the linear one beyond its table
    q["f_carr"][1, 5] = f_out
    assert host_verdict(pkg, q, n, rate) == (1, 0, 0)


def test_bisection_and_cboc_batches_keep_the_legacy_start(pkg, monkeypatch):
    monkeypatch.delenv("GAL_G_LINEAR", raising=False)
    n = 2 * 1024 + 100
    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=6, n_slots=8, samples_per_epoch=n, sample_rate=2.5e6, seed=78)
    assert host_verdict(pkg, p, n, 2.5e6) == (1, 1, 0)      # crowded thresholds: the bisection instances
    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=6, n_slots=8, samples_per_epoch=n, seed=79)
    assert host_verdict(pkg, p, n, flags=pkg.synth.GAL_CFG_CBOC)[2] == 0
