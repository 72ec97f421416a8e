"""The interference sources on the MI355X (gal_synth_iq_convert_interf): the kernels bit for bit against the numpy statement of the
definition (tests/interf_model.py), in every format, with and without the noise floor, at vector tails, at odd and large
first_sample, across the grid-stride jump, cut into calls, in place; and the C/N0 a receiver reads under a wideband chirp."""
import ctypes
import math

import numpy as np
import pytest

import interf_model
import noise_model
from test_iq_noise_gpu import _input

pytestmark = pytest.mark.gpu

GAL_E_INVAL = -1
FS = 2.6e6
SIGMA_45 = noise_model.noise_from_cn0(45.0, FS)[1]
FIRST_SAMPLES = (0, 1, 2, 3, (1 << 33) + 10, (1 << 33) + 11)
SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 1023, 4099, 100003)
FORMATS = (("ishort", 0), ("ibyte", 7), ("ibyte", 0), ("ibit", 0))
# four at once: a CW tone; a chirp whose restarts fall inside a 16-byte vector; a chirp of one-sample sweeps (from a first_sample above
# 2^33 its sweep number needs more than 32 bits); a pulsed tone, two samples of five
FOUR = [
    interf_model.source(amp_q4=3000 * 16, ph0=0x12345678, f0=165191050),
    interf_model.source(amp_q4=2000 * 16 + 5, ph0=0xF0000000, f0=-1234567891, df=300000007, sweep_len=7),
    interf_model.source(amp_q4=1500 * 16 + 3, ph0=77, f0=987654321, df=-55555, sweep_len=1),
    interf_model.source(amp_q4=2500 * 16 + 9, ph0=1 << 31, f0=-40000001, pulse_period=5, pulse_on=2),
]
# long sweeps and periods: restarts are rare, a lane's jump is shorter than a sweep
LONG = [
    interf_model.source(amp_q4=4000 * 16, ph0=5, f0=-(1 << 31), df=65535, sweep_len=65537),
    interf_model.source(amp_q4=3000 * 16, ph0=9, f0=123456789, df=-4251, sweep_len=1000003, pulse_period=1000, pulse_on=300),
    interf_model.source(amp_q4=1000 * 16, f0=1 << 30, pulse_period=4000037, pulse_on=4000000),
]


def _convert(eng, x_dev, n, fmt, s, noise, interf, first_sample=0, guard=64, n_offset=0):
    """As test_iq_noise_gpu._convert, with sources: (output bytes, the guard bytes behind them, saturated count)."""
    import torch

    from galileo_sdr_sim_amd import iq_bytes

    out = torch.full((iq_bytes(fmt, n) + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.iq_saturated(reset=True)
    eng.iq_convert(x_dev.data_ptr() + 4 * n_offset, n, fmt, s, out.data_ptr(), noise=noise, first_sample=first_sample, interf=interf)
    sat = eng.iq_saturated()
    o = out.cpu().numpy()
    return o[: o.size - guard], o[o.size - guard:], sat


@pytest.fixture(scope="module")
def eng(pkg):
    with pkg.SynthEngine(device=0) as e:
        yield e


@pytest.fixture(scope="module")
def data():
    """One input for the whole module, on the host and on the device."""
    import torch

    x = _input(SIZES[-1], 17)
    return x, torch.from_numpy(x).cuda()


@pytest.mark.parametrize("with_noise", (True, False))
@pytest.mark.parametrize("first_sample", FIRST_SAMPLES)
def test_formats_sizes_and_first_sample(eng, data, first_sample, with_noise):
    """Sizes that end inside a 16-byte vector, inside ibyte's 16 values and inside ibit's 64; with the noise at gain 1.5 and without
    any (G = 65536, S = 0).  A value's output does not depend on the call's length: the model is evaluated once at the largest size."""
    x, xd = data
    noise = (0x123456789ABCDEF0, 3, 98304, SIGMA_45) if with_noise else None
    y, clipped = interf_model.mix(x, noise, FOUR, first_sample)
    clamps16 = clamps8 = 0
    for n in SIZES:
        for fmt, s in FORMATS:
            got, guard, sat = _convert(eng, xd, n, fmt, s, noise, FOUR, first_sample)
            want, want_sat = interf_model.formatted(y[: 2 * n], clipped[: 2 * n], fmt, s)
            assert got.size == want.size and np.array_equal(got, want), (fmt, s, n, first_sample)
            assert sat == want_sat, (fmt, s, n, sat, want_sat)
            assert (guard == 0xA5).all(), (fmt, s, n)
            if n == SIZES[-1] and fmt == "ishort":
                clamps16 = want_sat
            if n == SIZES[-1] and fmt == "ibyte" and s == 7:
                clamps8 = want_sat
    assert 0 < clamps16 < clamps8 < 2 * SIZES[-1]
    # the sources are in it: the same call without them differs on most values
    plain = noise_model.convert(x, "ishort", 0, noise)[0] if with_noise else x.view(np.uint8)
    assert np.count_nonzero(y != plain.view(np.int16)) > 0.9 * y.size


@pytest.mark.parametrize("fmt,s,n,with_noise,cases", [
    ("ishort", 0, 2_200_003, True, ((FOUR, (1 << 33) + 2), (LONG, 999_999))),
    ("ibyte", 6, 4_300_005, False, ((FOUR, (1 << 33) + 3), (LONG, 999_998))),
    ("ibit", 0, 16_900_007, False, (([FOUR[1], LONG[1], FOUR[3]], (1 << 33) + 999_999),)),
    ("ishort", 0, 2_200_003, True, (([], (1 << 33) + 4), ([], (1 << 33) + 7))),  # noise only, even and odd
    ("ishort", 0, 2_200_003, False, ((FOUR, (1 << 33) + 6),)),  # sources without noise
])
def test_beyond_one_trip_of_the_grid(eng, fmt, s, n, with_noise, cases):
    """More vectors than the 2048 x 256 lanes of the grid (4, 8, 32 complex samples per vector): the lanes of the first blocks take a
    second trip, and (s, m) and the pulse position jump by the constant stride -- with sweeps and periods shorter than a vector
    (FOUR) and longer than the jump (LONG).  The instances without sources and the one without noise share that loop and its tail:
    an empty source list is the noise floor alone (interf_model.convert is then noise_model.convert)."""
    import torch

    x = _input(n, 41)
    xd = torch.from_numpy(x).cuda()
    noise = (5, 0, 65536, SIGMA_45) if with_noise else None
    for src, first in cases:
        got, guard, sat = _convert(eng, xd, n, fmt, s, noise, src, first)
        want, want_sat = interf_model.convert(x, fmt, s, noise, src, first)
        assert np.array_equal(got, want) and sat == want_sat and (guard == 0xA5).all(), (fmt, first)


def test_three_unequal_calls_equal_one(eng):
    """One buffer in three calls with the running first_sample = one call (the pieces start at multiples of 4 samples)."""
    import torch

    noise = (99, 1, 65536, SIGMA_45)
    n = 100003
    x = _input(n, 23)
    xd = torch.from_numpy(x).cuda()
    cuts = (0, 40004, 40008, n)
    for base, src in ((0, LONG), (7, FOUR), ((1 << 34) + 5, LONG + FOUR[3:])):
        for fmt, s in (("ishort", 0), ("ibyte", 6), ("ibit", 0)):
            whole, _, sat = _convert(eng, xd, n, fmt, s, noise, src, base)
            parts, sats = [], 0
            for a, b in zip(cuts[:-1], cuts[1:]):
                got, guard, st = _convert(eng, xd, b - a, fmt, s, noise, src, base + a, n_offset=a)
                assert (guard == 0xA5).all()
                parts.append(got)
                sats += st
            assert np.array_equal(np.concatenate(parts), whole), (fmt, base)
            assert sats == sat
            assert np.array_equal(whole, interf_model.convert(x, fmt, s, noise, src, base)[0])


def test_ishort_in_place(eng):
    import torch

    for n, first, noise in ((100003, 0, (11, 0, 65536, SIGMA_45)), (100003, 9, None), (5, 1, None)):
        x = _input(n, 31)
        xd = torch.from_numpy(x).cuda()
        want, _, want_sat = _convert(eng, xd, n, "ishort", 0, noise, FOUR, first)
        assert np.array_equal(want, interf_model.convert(x, "ishort", 0, noise, FOUR, first)[0])
        buf = torch.full((2 * n + 32,), 0x5A5A, dtype=torch.int16, device="cuda")
        buf[: 2 * n] = xd
        torch.cuda.synchronize()
        eng.iq_saturated(reset=True)
        eng.iq_convert(buf.data_ptr(), n, "ishort", 0, buf.data_ptr(), noise=noise, first_sample=first, interf=FOUR)
        sat = eng.iq_saturated()
        got = buf.cpu().numpy()
        assert np.array_equal(got[: 2 * n].view(np.uint8), want) and sat == want_sat
        assert (got[2 * n:] == 0x5A5A).all()


def test_no_source_is_the_noise_floor(eng, data):
    """n_interf = 0, and sources of amplitude 0, give the bytes and counts of gal_synth_iq_convert_noise (of gal_synth_iq_convert
    without noise)."""
    x, xd = data
    n = SIZES[-1]
    silent = [dict(c, amp_q4=0) for c in FOUR]
    for noise in ((7, 2, 98304, SIGMA_45), None):
        for fmt, s in FORMATS:
            for first in (0, 5):
                want, _, want_sat = _convert(eng, xd, n, fmt, s, noise, None, first)
                for src in ([], silent):
                    got, guard, sat = _convert(eng, xd, n, fmt, s, noise, src, first)
                    assert np.array_equal(got, want) and sat == want_sat and (guard == 0xA5).all(), (fmt, s, first, len(src))


def test_bad_arguments(eng, pkg):
    import torch

    lib = pkg.load_library()
    x = torch.zeros(64, dtype=torch.int16, device="cuda")
    out = torch.zeros(256, dtype=torch.uint8, device="cuda")
    h, p, o = eng._h, x.data_ptr(), out.data_ptr()
    Noise, Interf = pkg.synth._Noise, pkg.synth._Interf

    def call(src, fmt, shift, noise=None, src_ptr=p, dst=o, first=0, n=8, count=None):
        arr = (Interf * max(1, len(src)))(*src)
        return lib.gal_synth_iq_convert_interf(h, src_ptr, n, first, ctypes.byref(noise) if noise is not None else None,
                                               arr if src is not None else None, len(src) if count is None else count, fmt, shift, dst)

    ok = Interf(16000, 0, 1000, 10, 7, 5, 2, 0)
    nz = Noise(1, 0, 65536, 160, 0)
    assert call([Interf((1 << 20) + 1, 0, 0, 0, 0, 0, 0, 0)], 1, 5) == GAL_E_INVAL  # amp_q4 above 2^20
    assert call([Interf(16, 0, 1000, 1, 0, 0, 0, 0)], 1, 5) == GAL_E_INVAL  # df without a sweep
    assert call([Interf(16, 0, 0, 0, 0, 5, 6, 0)], 1, 5) == GAL_E_INVAL  # pulse_on > pulse_period
    assert call([Interf(16, 0, 0, 0, 0, 0, 1, 0)], 1, 5) == GAL_E_INVAL
    assert call([Interf(16, 0, 0, 0, 0, 0, 0, 1)], 1, 5) == GAL_E_INVAL  # reserved
    assert call([ok, ok, Interf(16, 0, 0, 0, 0, 0, 0, 1)], 1, 5) == GAL_E_INVAL  # the third of three
    assert b"source 2" in lib.gal_synth_last_error()
    assert call([ok] * 5, 1, 5) == GAL_E_INVAL and call([ok], 1, 5, count=-1) == GAL_E_INVAL  # n_interf outside 0..4
    assert lib.gal_synth_iq_convert_interf(h, p, 8, 0, None, None, 1, 1, 5, o) == GAL_E_INVAL  # null interf
    assert call([ok], 3, 0) == GAL_E_INVAL  # unknown format
    assert call([ok], 1, 16) == GAL_E_INVAL and call([ok], 1, -1) == GAL_E_INVAL and call([ok], 2, 3) == GAL_E_INVAL and call([ok], 0, 1) == GAL_E_INVAL
    assert call([ok], 1, 5, src_ptr=p + 2) == GAL_E_INVAL and call([ok], 1, 5, dst=o + 4) == GAL_E_INVAL  # misaligned
    assert call([ok], 1, 5, src_ptr=None) == GAL_E_INVAL and call([ok], 1, 5, dst=None) == GAL_E_INVAL
    assert call([ok], 1, 5, dst=p) == GAL_E_INVAL and call([ok], 2, 0, dst=p) == GAL_E_INVAL  # in place is for ishort only
    assert call([ok], 0, 0, dst=p + 16) == GAL_E_INVAL  # ishort: exactly in place or not at all
    assert b"overlap" in lib.gal_synth_last_error()
    assert call([ok], 0, 0, first=1 << 62) == GAL_E_INVAL
    assert call([ok], 1, 5, noise=Noise(1, 0, (1 << 20) + 1, 160, 0)) == GAL_E_INVAL
    assert call([ok], 1, 5, noise=Noise(1, 0, 65536, 160, 1)) == GAL_E_INVAL
    assert call([Interf(1 << 20, 0xFFFFFFFF, -(1 << 31), (1 << 31) - 1, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0)] * 4, 1, 5, noise=nz) == 0  # the bounds
    assert call([ok], 0, 0, dst=p) == 0 and call([ok], 0, 0, noise=nz, dst=p) == 0 and call([ok], 2, 0) == 0
    assert call([ok], 0, 0, first=(1 << 62) - 1) == 0
    assert call([], 1, 5, dst=p) == GAL_E_INVAL and call([], 1, 5) == 0  # n_interf = 0: the rules of the noise call
    eng.iq_saturated()
    with pytest.raises(pkg.GalSynthError) as ei:
        eng.iq_convert(p, 8, "ibyte", 5, o, interf=[{"amp_q4": 1 << 21}])
    assert ei.value.code == GAL_E_INVAL


def test_convert_interf_of_the_batch_in_flight_is_refused(pkg):
    import torch

    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=4, n_slots=16, samples_per_epoch=26000, seed=12)
    with pkg.SynthEngine(samples_per_epoch=26000, n_slots=16, device=0) as e:
        e.plan(p)
        iq = torch.empty(e.output_bytes() // 2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        e.execute(iq.data_ptr())
        with pytest.raises(pkg.GalSynthError) as ei:
            e.iq_convert(iq.data_ptr(), 52000, "ishort", 0, iq.data_ptr(), interf=FOUR)
        assert ei.value.code == -4  # GAL_E_STATE
        e.finish()
        x = iq.cpu().numpy()
        e.iq_convert(iq.data_ptr(), 52000, "ishort", 0, iq.data_ptr(), interf=FOUR)
        e.iq_saturated()
        assert np.array_equal(iq.cpu().numpy(), interf_model.mix(x, None, FOUR)[0])


def _tolerance_db(cn0_dbhz, M):
    """Three standard errors of gal_corr_cn0 in dB at the level cn0_dbhz, as tests/test_iq_corr_gpu.py derives them: per whole period
    the prompt holds signal + noise with the power ratio SNR = (C/N0) T / 2 (T = 4 ms), the far tap noise alone; over M periods the
    mean noise power has the relative standard error 1 / sqrt(M), the signal part sqrt((2 SNR + 1) / M) / SNR; in quadrature, as dB."""
    snr = 10 ** (cn0_dbhz / 10) * 0.004 / 2
    se = math.sqrt(1.0 / M + (2 * snr + 1) / (M * snr * snr))
    return 3 * 10 / math.log(10) * se


CHIRP_LEN = 1009  # not commensurate with the 10 400 samples of a code period


def chirp_cn0(pkg, eng, xd, n, q, js_db, seed):
    """C/N0 that gal_corr_cn0 reads from one second of one satellite under the 45 dB-Hz floor and a chirp over the whole band."""
    import torch

    noise = pkg.noise_from_cn0(45.0, FS, 1.0)  # the CLI's gain rule gives 1: 5 x 2267 + 4100 + 11 180 <= 32 767
    noise["seed"] = seed
    src = []
    if js_db is not None:
        src = [dict(pkg.interf_make(js_db, 1.0, FS, 0.0), f0=-(1 << 31), df=int(round(2.0 ** 32 / CHIRP_LEN)), sweep_len=CHIRP_LEN)]
    out = torch.zeros(2 * n, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    eng.iq_saturated(reset=True)
    eng.iq_convert(xd.data_ptr(), n, "ishort", 0, out.data_ptr(), noise=noise, first_sample=0, interf=src)
    sat = eng.iq_saturated()
    sums = eng.correlate(out.data_ptr(), "ishort", n, q)
    return pkg.corr_cn0(sums, q, 0, 1, 0, FS)[0], sat


def test_cn0_under_a_wideband_chirp(pkg, eng):
    """One satellite, ten epochs = 1 s, the noise floor at 45 dB-Hz and a chirp from -fs/2 to +fs/2 every 1009 samples at J/S 20 and
    30 dB.  Over many sweeps the chirp's spectrum is flat, J / fs per Hz, so a receiver should read
    C / (N0 + J / fs) = 1 / (1 / cn0 + (J/S) / fs): 41.54 dB-Hz at 20 dB, 33.81 dB-Hz at 30 dB.  The readings must fall strictly with
    J/S, and agree with the prediction within three standard errors of the estimator at the predicted level (_tolerance_db, M = 248
    whole periods: 0.86 dB at 41.5 dB-Hz, 1.00 dB at 33.8 dB-Hz).  Measured figures: DESIGN.md section 13."""
    import torch

    p = pkg.workloads.make_synthetic(n_epochs=10, n_chan=1, n_slots=16, prns=[11], seed=77)
    x, _, _ = eng.run_host(p)
    n = x.size // 2
    xd = torch.from_numpy(x).cuda()
    q = pkg.corr_from_epoch(p[0, 0], FS, 0, max_periods=250, delay0=0, delay_step=2046, n_delay=2)
    got = {}
    for js in (None, 20.0, 30.0):
        got[js], sat = chirp_cn0(pkg, eng, xd, n, q, js, 20241008)
        want = 45.0 if js is None else -10 * math.log10(10 ** -4.5 + 10 ** (js / 10) / FS)
        tol = _tolerance_db(want, 248)
        print("J/S %s dB: C/N0 %.3f dB-Hz, predicted %.3f, tolerance %.3f dB, saturated %d" % (js, got[js], want, tol, sat))
        assert sat == 0
        assert abs(got[js] - want) <= tol, (js, got[js], want, tol)
    assert got[None] > got[20.0] > got[30.0]
