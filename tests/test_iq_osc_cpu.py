"""The receiver oscillator without a GPU: the numpy model (tests/osc_model.py) against python integers, the int32 bounds of the
definition, the host helpers gal_synth_osc_check / _make / _lo_step against their formulas, and the physics of the model -- a tone
lands in its bin, a drift is a parabola in phase, the phase noise is a random walk of the stated variance."""
import math

import numpy as np
import pytest

import osc_model

FS = 2.6e6
FC = 1575.42e6
GAL_E_INVAL = -1


def _tone(n, amp=8000):
    x = np.zeros(2 * n, dtype=np.int16)
    x[0::2] = amp
    return x


def _cplx(y):
    return y[0::2].astype(np.float64) + 1j * y[1::2].astype(np.float64)


def test_the_zero_oscillator_is_the_identity():
    rng = np.random.default_rng(1)
    x = rng.integers(-32768, 32768, 2 * 5000, dtype=np.int16)
    x[:4] = (-32768, -32768, 32767, 32767)
    for first in (0, 7, 2 ** 40 + 3):
        y, sat, zz = osc_model.rotate(x, osc_model.osc(), first, first)
        assert np.array_equal(y, x) and sat == 0 and zz == 0
    c, s = osc_model.cos_sin(np.zeros(1, dtype=np.int64))
    assert (int(c[0]), int(s[0])) == (4096, 0)


@pytest.mark.parametrize("base", [0, 2 ** 40, 2 ** 61, 2 ** 64 - 40])
def test_the_triangular_number_is_exact(base):
    N = [(base + k) & osc_model.M64 for k in range(-3 if base else 0, 37)]
    got = osc_model.tri(np.array(N, dtype=np.uint64))
    want = [(v * (v - 1) // 2) & osc_model.M64 for v in N]
    assert [int(v) for v in got] == want


def test_the_phase_is_the_closed_form_in_python_integers():
    o = osc_model.osc(p0=0x123456789ABCDEF0, f=-(2 ** 62) + 12345, d=2 ** 45 + 7, s=0)
    for first in (0, 2 ** 40 + 3):
        phi, _ = osc_model.phase(o, 0, first, 50)
        for k in (0, 1, 17, 49):
            N = first + k
            assert int(phi[k]) == (o["p0"] + N * o["f"] + (N * (N - 1) // 2) * o["d"]) & osc_model.M64


def test_the_noise_sum_excludes_the_first_sample_and_carries_over():
    o = osc_model.osc(s=12345678901, seed=9, stream=2)
    n0 = 2 ** 40 + 3
    zs = osc_model.z(9, 2, n0, 100)
    phi, zz = osc_model.phase(o, n0, n0, 100)
    Z = np.cumsum(np.concatenate(([0], zs[1:])))
    assert zz == int(Z[-1])
    assert [int(v) for v in phi] == [(int(v) * o["s"]) & osc_model.M64 for v in Z]
    # in two pieces
    _, z1 = osc_model.phase(o, n0, n0, 37)
    phi2, z2 = osc_model.phase(o, n0, n0 + 37, 63, z1)
    assert z2 == zz and np.array_equal(phi2, phi[37:])
    # counter word 3 = 1: not the noise floor's words
    import noise_model

    assert not np.array_equal(zs, noise_model.noise_z(9, 2, n0, 100))


def test_the_bounds_hold_at_the_int16_corners_for_every_phase():
    """All 2^22 (i, e) pairs: |c|, |s| <= 4096 + 13, and every product and sum of the definition fits an int32 at x = (-32768, -32768)
    and x = (32767, 32767) (computed in int64, compared with the int32 range)."""
    C = osc_model._C
    lim = 1 << 31
    worst_c = worst_v = worst_t = 0
    for i0 in range(0, 1024, 64):
        i = np.repeat(np.arange(i0, i0 + 64, dtype=np.int64), 4096)
        e = np.tile(np.arange(-2048, 2048, dtype=np.int64), 64)
        theta = (((i << 22) | ((e + 2048) << 10)) - (1 << 21)) & 0xFFFFFFFF
        c, s = osc_model.cos_sin(theta)
        c0, s0 = C[i], C[(i - 256) & 1023]
        for t in (s0 * e, s0 * e * 101, s0 * e * 101 + (1 << 25), c0 * e, c0 * e * 101, c0 * e * 101 + (1 << 25)):
            worst_t = max(worst_t, int(np.abs(t).max()))
        worst_c = max(worst_c, int(np.abs(c).max()), int(np.abs(s).max()))
        for x in (-32768, 32767):
            for t in (x * c, x * s, x * c - x * s, x * c - x * s + 2048, x * s + x * c, x * s + x * c + 2048):
                worst_v = max(worst_v, int(np.abs(t).max()))
    assert worst_c <= 4096 + 13, worst_c
    assert worst_t < lim and worst_v < lim, (worst_t, worst_v)


def test_make_agrees_with_its_formulas(pkg):
    m2 = osc_model.gauss_m2()
    assert abs(osc_model.z_variance() - 1.0) < 1e-3 and osc_model.z_variance() != 1.0
    import noise_model

    assert abs(osc_model.z_variance() - noise_model.z_moments()[0]) < 1e-12
    assert m2 < 2 ** 61
    cases = [(0.0, 0.0, 0.0, FS, FC), (1234.5, 0.0, 0.0, FS, FC), (-1500.0, 2.0, 1e-21, FS, FC), (3000.0, -0.5, 1e-19, 2 * FS, FC),
             (FS / 2 - 1.0, 1e9, 1e-23, FS, FC), (-(FS / 2 - 1.0), -3.3e12, 3e-18, FS, FC), (10.0, 0.0, 1e-20, 4.092e6, 1.0e9)]
    for c in cases:
        got = pkg.osc_make(*c)
        want = osc_model.make(*c)
        assert got == want, (c, got, want)
        pkg.osc_check(got)
    o = pkg.osc_make(1234.5, 0.0, 0.0, FS, FC)
    assert o["f"] == round(1234.5 / FS * 2 ** 64) or abs(o["f"] - 1234.5 / FS * 2 ** 64) <= 2048  # (a double carries 53 bits)
    assert o["seed"] == 1 and o["stream"] == 0 and o["p0"] == 0 and o["s"] == 0
    # the sigma of a sample: carrier sqrt(h0 / (2 fs)) cycles, through the table's own variance
    o = pkg.osc_make(0.0, 0.0, 1e-21, FS, FC)
    assert abs(osc_model.sigma_cycles(o) / (FC * math.sqrt(1e-21 / (2 * FS))) - 1.0) < 1e-9


def test_make_and_check_refuse(pkg):
    nan, inf = float("nan"), float("inf")
    big_d = 0.5 * FS * FS
    for c in [(nan, 0, 0, FS, FC), (0, inf, 0, FS, FC), (0, 0, nan, FS, FC), (0, 0, 0, inf, FC), (0, 0, 0, FS, nan), (0, 0, 0, 0.0, FC),
              (0, 0, 0, -FS, FC), (FS / 2, 0, 0, FS, FC), (-FS / 2, 0, 0, FS, FC), (FS, 0, 0, FS, FC), (0, 0, -1e-21, FS, FC),
              (0, 0, 1e-10, FS, FC), (0, big_d, 0, FS, FC), (0, -big_d, 0, FS, FC), (0, 0, 0, FS, -1.0)]:
        with pytest.raises(pkg.GalSynthError) as ei:
            pkg.osc_make(*c)
        assert ei.value.code == GAL_E_INVAL, c
        with pytest.raises(ValueError):
            osc_model.make(*c)
    # the largest drift that fits is admitted
    d_max = math.nextafter(big_d, 0.0)
    assert pkg.osc_make(0.0, d_max, 0.0, FS, FC) == osc_model.make(0.0, d_max, 0.0, FS, FC)
    pkg.osc_check({"s": 1 << 48})
    with pytest.raises(pkg.GalSynthError) as ei:
        pkg.osc_check({"s": (1 << 48) + 1})
    assert ei.value.code == GAL_E_INVAL
    o = pkg.synth._osc_struct({"s": 5})
    o.reserved = 1
    with pytest.raises(pkg.GalSynthError) as ei:
        pkg.osc_check(o)
    assert ei.value.code == GAL_E_INVAL
    lib = pkg.load_library()
    assert lib.gal_synth_osc_check(None) == GAL_E_INVAL
    assert lib.gal_synth_osc_make(0.0, 0.0, 0.0, FS, FC, None) == GAL_E_INVAL
    assert lib.gal_synth_osc_lo_step(None, 0, None) == GAL_E_INVAL


def test_lo_step(pkg):
    o = osc_model.make(2000.0, 2.0, 0.0, FS, FC)
    assert pkg.osc_lo_step(o, 0) == o["f"] >> 32 == osc_model.lo_step(o, 0)
    # in the correlator's units: the offset over the sample rate x 2^32, rounded down
    assert abs(pkg.osc_lo_step(o, 0) - 2000.0 / FS * 2 ** 32) <= 1
    for o in (o, osc_model.osc(f=-(2 ** 63), d=2 ** 63 - 1), osc_model.osc(f=2 ** 63 - 1, d=-(2 ** 63)), osc_model.osc(f=-1, d=-1)):
        for N in (0, 1, 260000, 2 ** 40 + 3, 2 ** 62 - 1):
            want = (((o["f"] + N * o["d"]) % 2 ** 64) >> 32)
            want -= (want >> 31) << 32
            assert pkg.osc_lo_step(o, N) == want == osc_model.lo_step(o, N), (o, N)
    # after one second of 2 Hz/s the step is that of 2002 Hz
    o = osc_model.make(2000.0, 2.0, 0.0, FS, FC)
    assert abs(pkg.osc_lo_step(o, 2600000) - 2002.0 / FS * 2 ** 32) <= 1


# ---- physics, on the model ---------------------------------------------------------------------------------------------------------
def _bh4(n):
    k = 2.0 * np.pi * np.arange(n) / n
    return 0.35875 - 0.48829 * np.cos(k) + 0.14128 * np.cos(2 * k) - 0.01168 * np.cos(3 * k)


def tone_spectrum(f_hz=1234.5, n=1 << 18):
    """(peak bin, strongest spur in dBc) of the constant (8000, 0) through the offset f_hz: 4-term Blackman-Harris window (side lobes
    below -92 dB), the spur searched outside +-8 bins of the peak."""
    y, sat, _ = osc_model.rotate(_tone(n), osc_model.make(f_hz, 0.0, 0.0, FS, FC), 0, 0)
    assert sat == 0
    p = np.abs(np.fft.fft(_cplx(y) * _bh4(n))) ** 2
    k = int(np.argmax(p))
    q = p.copy()
    q[np.arange(k - 8, k + 9) % n] = 0.0
    return k, 10.0 * math.log10(q.max() / p[k])


# measured on the model (tone_spectrum() above): -94.25 dBc, at the level of the window's own side lobes; DESIGN.md section 19
SPUR_MODEL_DBC = -94.25


def test_a_tone_lands_in_its_bin():
    n = 1 << 18
    k, spur = tone_spectrum(1234.5, n)
    print("peak bin %d, strongest spur %.2f dBc" % (k, spur))
    assert k == round(1234.5 / FS * n)
    assert spur <= SPUR_MODEL_DBC + 6.0, spur
    k, _ = tone_spectrum(-1234.5, n)
    assert k == n - round(1234.5 / FS * n)


def test_a_drift_is_a_parabola_in_phase():
    """The phase of the tone against P0 + F n + D n (n - 1) / 2 in floating point cycles: within the table's resolution, 2^-10 cycles."""
    n = 200000
    o = osc_model.make(1234.5, 5.0e4, 0.0, FS, FC)
    o["p0"] = 0x4000000000000000 + 12345
    for first in (0, 2 ** 40 + 3):
        y, sat, _ = osc_model.rotate(_tone(n), o, first, first)
        assert sat == 0
        got = np.angle(_cplx(y)) / (2.0 * np.pi)
        N = [first + k for k in range(0, n, 97)]
        want = np.array([((o["p0"] + v * o["f"] + (v * (v - 1) // 2) * o["d"]) % 2 ** 64) / 2.0 ** 64 for v in N])
        err = got[::97] - want
        err -= np.round(err)
        print("first %d: worst phase error %.3e cycles" % (first, np.abs(err).max()))
        assert np.abs(err).max() < 2.0 ** -10
    # the drift is there: the frequency at the end is that of F + n D
    f_end = (o["f"] + (n - 1) * o["d"]) / 2.0 ** 64 * FS
    assert abs(f_end - (1234.5 + 5.0e4 * (n - 1) / FS)) < 1e-3


@pytest.mark.parametrize("lag", [1, 16, 256])
def test_the_phase_noise_is_a_random_walk_of_the_stated_variance(lag):
    """Increments of the tone's phase over non-overlapping spans of `lag` samples have the variance lag x sigma^2, sigma from S and the
    table's own variance; the estimator's scatter over 2^16 / lag increments is sqrt(2 lag / 2^16) relative, five of them allowed."""
    n = 1 << 16
    o = osc_model.osc(s=int(1e-3 * 2 ** 52), seed=4242, stream=3)
    y, sat, _ = osc_model.rotate(_tone(n + 256), o, 1000, 1000)
    assert sat == 0
    w = _cplx(y)
    a, b = w[0:n:lag], w[lag:n + lag:lag]
    inc = np.angle(b * np.conj(a)) / (2.0 * np.pi)
    assert inc.size == n // lag
    got = float(np.mean(inc ** 2))
    want = lag * osc_model.sigma_cycles(o) ** 2
    tol = 5.0 * math.sqrt(2.0 * lag / n)
    print("lag %d: variance %.6e cycles^2, expected %.6e (ratio %.4f, tolerance %.4f)" % (lag, got, want, got / want, tol))
    assert abs(got / want - 1.0) <= tol
