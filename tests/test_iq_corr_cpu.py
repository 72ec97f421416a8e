"""The correlator bank's host side (include/galsynth.h: gal_synth_corr_out_bytes, gal_corr_from_epoch, gal_corr_cn0, the refusals that
need no device) and the definition itself, stated in tests/corr_model.py, on a stream the oracle synthesised.  No GPU."""
import ctypes
import math

import numpy as np
import pytest

import corr_model
from oracle_binding import oracle_run

GAL_E_INVAL = -1
FS = 2.6e6
BIN_250HZ = round(250.0 / FS * 2 ** 32)


def test_out_bytes(pkg):
    assert pkg.corr_out_bytes({"prn": 1, "code_ph0": 0, "code_dph": 1}) == 32
    assert pkg.corr_out_bytes({"prn": 1, "code_ph0": 0, "code_dph": 1, "max_periods": 25, "n_dopp": 3, "n_delay": 4}) == 25 * 3 * 4 * 32
    assert pkg.corr_out_bytes({"prn": 1, "code_ph0": 0, "code_dph": 1, "max_periods": 1024, "n_dopp": 64, "n_delay": 8184}) == 1024 * 64 * 8184 * 32
    for bad in ({"n_delay": 0}, {"n_delay": 8185}, {"n_dopp": 0}, {"n_dopp": 65}, {"max_periods": 0}, {"max_periods": 1025}):
        q = {"prn": 1, "code_ph0": 0, "code_dph": 1}
        q.update(bad)
        assert pkg.corr_out_bytes(q) == 0, bad
    assert pkg.load_library().gal_synth_corr_out_bytes(None) == 0
    assert ctypes.sizeof(pkg.synth._CorrReq) == 56


def test_from_epoch_rounds_as_the_model(pkg):
    p = pkg.workloads.make_synthetic(n_epochs=4, n_chan=12, n_slots=16, seed=3)
    for e in range(4):
        for s in range(12):
            for off in (0, 32, 123457):
                got = pkg.corr_from_epoch(p[e, s], FS, off)
                want = corr_model.from_epoch(p[e, s], FS, off)
                assert got == want, (e, s, off, got, want)
                assert 0 <= got["code_ph0"] < corr_model.L
                if e > 0:
                    assert got["carr_ph0"] == 0  # a continuing channel: the phase is the engine's state
    # ties and signs: f_carr / fs x 2^32 = -1.5 rounds away from zero
    rec = p[0, 0].copy()
    rec["f_carr"] = -1.5 * FS / 2 ** 32
    assert pkg.corr_from_epoch(rec, FS)["carr_dph"] == -2 == corr_model.from_epoch(rec, FS)["carr_dph"]
    # the drift bound of the header: the replica's step differs from twice the engine's double step by at most 2^-33 half chips
    q = pkg.corr_from_epoch(p[0, 0], FS)
    assert abs(q["code_dph"] / 2 ** 32 - 2.0 * float(p[0, 0]["f_code"]) / FS) <= 2.0 ** -33
    assert pkg.corr_from_epoch(p[0, 0], FS, 0, n_delay=3, delay0=-1)["n_delay"] == 3  # the grid is the caller's


def test_from_epoch_refusals(pkg):
    lib = pkg.load_library()
    p = pkg.workloads.make_synthetic(n_epochs=1, n_chan=1, n_slots=16, seed=3)
    q = pkg.synth._CorrReq()

    def call(rec, fs=FS, off=0, out=q):
        r = np.ascontiguousarray(rec).reshape(1)
        return lib.gal_corr_from_epoch(r.ctypes.data, fs, off, ctypes.byref(out) if out is not None else None)

    assert call(p[0, 0]) == 0
    assert lib.gal_corr_from_epoch(None, FS, 0, ctypes.byref(q)) == GAL_E_INVAL and call(p[0, 0], out=None) == GAL_E_INVAL
    assert call(p[0, 1]) == GAL_E_INVAL  # idle slot: prn 0
    assert call(p[0, 0], off=-1) == GAL_E_INVAL
    assert call(p[0, 0], fs=0.0) == GAL_E_INVAL and call(p[0, 0], fs=float("nan")) == GAL_E_INVAL
    rec = p[0, 0].copy()
    rec["f_carr"] = FS  # the step does not fit an int32
    assert call(rec) == GAL_E_INVAL
    rec = p[0, 0].copy()
    rec["f_code"] = 0.6 * FS  # more than a half chip per sample
    assert call(rec) == GAL_E_INVAL
    with pytest.raises(pkg.GalSynthError):
        pkg.corr_from_epoch(p[0, 1], FS)


def test_correlate_refusals_without_a_device(pkg):
    """A null handle is refused before anything touches a device."""
    lib = pkg.load_library()
    q = pkg.synth._CorrReq(1, 1, 0, 1 << 31, 0, 0, 0, 1, 1, 0, 0, 1)
    assert lib.gal_synth_correlate(None, 16, 0, 100, ctypes.byref(q), 1, 32) == GAL_E_INVAL


def _model_sums(M=12, seed=1, amp=1000.0, noise=300.0):
    rng = np.random.default_rng(seed)
    out = np.rint(rng.normal(0.0, noise, (M, 2, 3, 4))).astype(np.int64)
    out[:, 1, 1, 0] += int(amp)
    out[:, 1, 1, 2] -= int(amp)
    return out


def test_cn0_on_model_sums(pkg):
    q = {"prn": 3, "code_ph0": 5, "code_dph": 3379813460, "max_periods": 12, "n_dopp": 2, "n_delay": 3}
    out = _model_sums()
    got = pkg.corr_cn0(out, q, 1, 2, 1, FS)
    want = corr_model.cn0(out, q, 1, 2, 1, FS)
    assert want is not None and abs(got[0] - want[0]) < 1e-9 and abs(got[1] / want[1] - 1) < 1e-12
    # by hand: the whole periods 1 .. 10 only
    a = out[1:11, 1].astype(np.float64)
    pp, pn = np.mean(np.sum(a[:, 1] ** 2, axis=1)), np.mean(np.sum(a[:, 2] ** 2, axis=1))
    T = 8184 * 2 ** 32 / 3379813460 / FS
    assert abs(got[0] - 10 * math.log10(2 * (pp - pn) / (pn * T))) < 1e-9 and abs(got[1] - pp / pn) < 1e-9
    # m = 0 and the last period do not count
    spoiled = out.copy()
    spoiled[0] = 10 ** 9
    spoiled[11] = -10 ** 9
    assert pkg.corr_cn0(spoiled, q, 1, 2, 1, FS) == got
    # no peak: GAL_E_INVAL
    with pytest.raises(pkg.GalSynthError) as ei:
        pkg.corr_cn0(out, q, 2, 1, 1, FS)
    assert ei.value.code == GAL_E_INVAL
    for bad in ((3, 2, 1), (1, -1, 1), (1, 2, 2)):
        with pytest.raises(pkg.GalSynthError):
            pkg.corr_cn0(out, q, *bad, FS)
    q2 = dict(q, max_periods=2)
    with pytest.raises(pkg.GalSynthError):
        pkg.corr_cn0(out[:2], q2, 1, 2, 1, FS)


def test_cn0_recovers_a_stated_ratio(pkg):
    """Sums built to DESIGN.md section 12's powers: per component an amplitude A N and noise of variance N s^2 A^2 ... in the sums' own
    terms: S_B = S_C = a + noise of variance v per part.  Then (Pp - Pn) / Pn = 2 a^2 / (4 v), and the function must say
    C/N0 = 2 (Pp - Pn) / (Pn T) within the estimator's error at M = 1000 periods."""
    M, a, v = 1002, 4000.0, 1000.0 ** 2
    rng = np.random.default_rng(7)
    out = rng.normal(0.0, math.sqrt(v), (M, 1, 2, 4))
    out[:, 0, 0, 0] += a
    out[:, 0, 0, 2] += a
    q = {"prn": 1, "code_ph0": 0, "code_dph": 3379813460, "max_periods": M, "n_delay": 2}
    T = 8184 * 2 ** 32 / 3379813460 / FS
    want = 10 * math.log10(2 * (2 * a * a) / (4 * v) / T)
    got, ratio = pkg.corr_cn0(np.rint(out).astype(np.int64), q, 0, 1, 0, FS)
    snr = 2 * a * a / (4 * v)
    se = math.sqrt(1 / 1000 + (2 * snr + 1) / 1000 / snr ** 2)  # relative: Pn, and Pp - Pn (the docstring of the GPU test)
    assert abs(got - want) <= 3 * 10 / math.log(10) * se, (got, want)
    assert abs(ratio - (1 + snr)) < 0.1 * (1 + snr)


@pytest.fixture(scope="module")
def one_satellite(pkg):
    """Three epochs of one satellite (PRN 7), noise-free, from the oracle."""
    p = pkg.workloads.make_synthetic(n_epochs=3, n_chan=1, n_slots=16, prns=[7], seed=5)
    iq, _ = oracle_run(p, 260000, FS)
    return p, iq


def test_end_to_end_model_peak(pkg, one_satellite):
    """The model's replica, made from the planned record alone, despreads the oracle's stream: at zero offset |S_B| of a whole period
    is the period's N samples x 250^2 (the carrier table squared) less the E1B-E1C cross term of this PRN, sum b c over the samples,
    which the signal (B d - C s) w carries into both components (with the sign of the period's symbols d s), and less the phase error of the engine's (int)(511 phase) index
    against the replica's 512 phase.  Expected from the model: 250^2 (N - |sum_n b[h(n)] c[h(n)]|) -- for PRN 7 here 0.9703 N 250^2
    in period 1 -- and the bound is that less 2 %."""
    p, iq = one_satellite
    T = pkg.tables()
    q = pkg.corr_from_epoch(p[0, 0], FS, 0, max_periods=6, delay0=-4, n_delay=9, dopp0=-2 * BIN_250HZ, dopp_step=BIN_250HZ, n_dopp=5)
    n_samples = 70000
    out = corr_model.correlate(iq[: 2 * n_samples], q, T)
    n = np.arange(n_samples, dtype=np.uint64)
    hi = ((np.uint64(q["code_ph0"]) + n * np.uint64(q["code_dph"])) >> np.uint64(32)).astype(np.int64)
    m, h = hi // 8184, hi % 8184
    b, c = corr_model.replicas(T, 7)
    power = out[..., 0].astype(np.float64) ** 2 + out[..., 1].astype(np.float64) ** 2 + out[..., 2].astype(np.float64) ** 2 + out[..., 3].astype(np.float64) ** 2
    for period in range(1, 6):
        N = int(np.count_nonzero(m == period))
        assert 10399 <= N <= 10401
        cross = abs(int(np.sum(b[h[m == period]] * c[h[m == period]])))
        expected = 250 ** 2 * (N - cross)
        mag = math.hypot(*out[period, 2, 4, 0:2].astype(np.float64))
        print("period %d: N %d, cross term %d, |S_B| = %.4f N 250^2 = %.4f expected" % (period, N, cross, mag / (N * 250 ** 2), mag / expected))
        assert mag >= 0.9 * N * 250 ** 2
        # (above: the table entries are rounded to integers, |w| <= 250 + 0.71, so |w|^2 may pass 250^2 by up to 0.6 %)
        # and the data symbol x secondary code of the period decides the sign of the cross term: N - cross or N + cross
        assert 0.98 * expected <= mag <= 1.006 * expected or 0.98 * 250 ** 2 * (N + cross) <= mag <= 1.006 * 250 ** 2 * (N + cross)
        # single satellite, no noise: the samples are non-zero only where B d = -C s, so S_C = -+S_B exactly
        assert abs(int(out[period, 2, 4, 2])) == abs(int(out[period, 2, 4, 0]))
        assert np.unravel_index(int(np.argmax(power[period])), power[period].shape) == (2, 4)  # offset (0 bins, 0 half chips)
    assert np.unravel_index(int(np.argmax(power[1:6].sum(axis=0))), power[0].shape) == (2, 4)


def test_model_cn0_of_a_noisy_stream(pkg, one_satellite):
    """The definition end to end on the CPU: the oracle's satellite + the noise floor of tests/noise_model.py at 45 dB-Hz, despread by
    the model over 0.3 s (M = 72 whole periods): gal_corr_cn0 gives the requested composite C/N0 within three standard errors
    (the formula of tests/test_iq_corr_gpu.py: 1.56 dB at M = 72, per-period SNR 63)."""
    import noise_model

    p, iq = one_satellite
    T = pkg.tables()
    G, S = noise_model.noise_from_cn0(45.0, FS)
    y = noise_model.mix(iq, 11, 0, G, S)[0]
    q = pkg.corr_from_epoch(p[0, 0], FS, 0, max_periods=74, delay0=0, delay_step=2046, n_delay=2)
    out = corr_model.correlate(y, q, T)
    cn0, ratio = pkg.corr_cn0(out, q, 0, 1, 0, FS)
    snr = 10 ** 4.5 * 0.004 / 2
    se = math.sqrt(1 / 72 + (2 * snr + 1) / 72 / snr ** 2)
    tol = 3 * 10 / math.log(10) * se
    print("C/N0 %.3f dB-Hz (asked 45), Pp / Pn %.2f, 3 standard errors %.2f dB" % (cn0, ratio, tol))
    assert abs(cn0 - 45.0) <= tol


def test_model_fills_an_int32_within_128_samples(pkg):
    """The standing request of tests/test_iq_corr_gpu.py::test_full_scale_input reaches what it claims.  The carrier table's loudest
    entry with cos and sin of one sign has |cos| + |sin| = 354 (250 sqrt 2, rounded per entry), so the sample (-32768, -32768) is
    wiped to |Re| = 32768 x 354 = 11.6 M -- 0.71 of the 2 x 32768 x 250 that iq_corr.hip's kSub = 128 is sized for -- and, the code
    and the carrier standing, every sample adds it with one sign: 128 consecutive samples sum to 1.48 x 10^9, above 2^30 and below
    2^31.  An int32 accumulator over 256 samples would wrap (kSub is tight within a factor of 2), and the whole buffer's sum needs
    the int64 it is handed to."""
    T = pkg.tables()
    c, s = T["cos512"].astype(np.int64), T["sin512"].astype(np.int64)
    i = int(np.argmax(np.abs(c + s)))
    amp = int(abs(c[i] + s[i]))
    assert amp == (np.abs(c) + np.abs(s)).max() and 350 <= amp <= 2 * 251
    n = 8190
    q = {"prn": 50, "code_ph0": (8183 << 32) + 17, "code_dph": 0, "carr_ph0": i << 23, "carr_dph": 0, "dopp0": 0, "max_periods": 1, "n_delay": 2,
         "delay0": 8183}
    v = np.full(2 * n, -32768, dtype=np.int64)
    # the model's per-sample wiped values: (I + iQ) conj(w) with w = (cos, sin)[carr_ph0 >> 23] for every sample
    re = v[0::2] * c[i] + v[1::2] * s[i]
    im = v[1::2] * c[i] - v[0::2] * s[i]
    assert (np.abs(re) == 32768 * amp).all() and np.abs(im).max() <= 32768 * 2
    window = np.abs(np.convolve(re, np.ones(128, dtype=np.int64), mode="valid"))  # every sum of 128 consecutive samples
    assert 2 ** 30 < int(window.max()) == 128 * 32768 * amp < 2 ** 31
    assert 256 * 32768 * amp > 2 ** 31 and n * 32768 * amp > 2 ** 36
    out = corr_model.correlate(v, q, T)
    b, _ = corr_model.replicas(T, 50)
    # delay 8183 of half chip 8183 reads b[0]; the next delay (8184 = 0) reads b[8183]
    assert out.shape == (1, 1, 2, 4) and out[0, 0, 0, 0] == b[0] * re.sum() and out[0, 0, 1, 0] == b[8183] * re.sum()
    assert abs(int(out[0, 0, 0, 0])) == n * 32768 * amp
    # the sign trick of the kernel's walk, (x ^ s) - s with s = 0 or -1, is x or -x for every value the wipe-off can give: |x| is at
    # most 32768 x 2 x 251 < 2^31, so -x never meets INT32_MIN, the one value it would leave unchanged
    x = np.array([32768 * amp, -32768 * amp, 32768 * 502, -32768 * 502, 0, 1, -1], dtype=np.int32)
    for sgn in (0, -1):
        assert np.array_equal((x ^ np.int32(sgn)) - np.int32(sgn), x if sgn == 0 else -x)
