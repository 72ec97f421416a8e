"""Per-satellite multipath without a GPU: the numpy model's own invariants (tests/mpath_model.py), the int32 bound as arithmetic, the
host-only entry points gal_synth_mpath_check / _make / _row, the ctypes layout, and the physics of one echo on the CPU: the correlator
model over a one-satellite oracle stream with an echo against the superposition of the echo-free correlations."""
import ctypes
import math

import numpy as np
import pytest

import corr_model
import gain_model
import mpath_model
from oracle_binding import oracle_run

GAL_E_INVAL = -1


@pytest.fixture(scope="module")
def cos1024(pkg):
    return pkg.tables()["cos1024"]


def _parts(rng, n_parts, n_epochs, spe, lim=32768):
    return rng.integers(-lim, lim, size=(n_parts, n_epochs * spe * 2), dtype=np.int16)


def _rows(pkg, part_of_echo, n_parts, *args):
    """An echo table of the product's row type that the product's own admission (gal_synth_mpath_check) takes for these parts."""
    r = mpath_model.rows(*args).astype(pkg.ECHO_DTYPE)
    pkg.mpath_check(r, part_of_echo, n_parts)
    return r


# ---- the model's own invariants ------------------------------------------------------------------------------------------------------
def test_no_echo_is_the_weighted_sum(pkg, cos1024):
    rng = np.random.default_rng(1)
    spe = 37
    x = _parts(rng, 3, 4, spe)
    g = rng.integers(0, 32768, size=(4, 3))
    want, want_sat = gain_model.wsum(x, g, spe)
    got, sat, hist = mpath_model.mpath(x, g, spe, [], _rows(pkg, [], 3, 4, 0), cos1024)
    assert np.array_equal(got, want) and sat == want_sat and want_sat > 0
    # an echo of gain 0 adds nothing either, whatever its delay and phase
    got, sat, _ = mpath_model.mpath(x, g, spe, [2], _rows(pkg, [2], 3, 4, 1, 0, 9, 12345, -7), cos1024)
    assert np.array_equal(got, want) and sat == want_sat
    # the history that comes back: the last 1024 samples, zeros in front of a call shorter than that
    assert hist.shape == (3, 2048) and np.array_equal(hist[:, -x.shape[1]:], x) and not hist[:, :-x.shape[1]].any()


def test_an_echo_at_delay_0_phase_0_and_the_parts_gain_doubles_the_part(pkg, cos1024):
    """C[0] = 4096 and C[-256] = 0: r = u exactly, so the echo at A = g makes w = 2 g x: the weighted sum at twice the gain."""
    assert cos1024[0] == 4096 and cos1024[(0 - 256) & 1023] == 0
    rng = np.random.default_rng(2)
    spe = 50
    x = _parts(rng, 2, 3, spe, 3000)
    g = np.array([[100, 7], [128, 0], [1, 300]])
    got, sat, _ = mpath_model.mpath(x, g, spe, [0], _rows(pkg, [0], 2, 3, 1, g[:, :1], 0, 0, 0), cos1024)
    g2 = g.copy()
    g2[:, 0] *= 2
    want, want_sat = gain_model.wsum(x, g2, spe)
    assert np.array_equal(got, want) and sat == want_sat


def test_delay_reaches_back_over_epochs_and_calls(pkg, cos1024):
    """A pure delay at phase 0 (one part, gain 0, echo at A = 128): y[n] = x[n - D], over epochs shorter than the delay, and any cut
    of the stream into calls that hands the history on gives the bytes of one call."""
    rng = np.random.default_rng(3)
    spe, n_epochs, D = 7, 300, 1023
    x = _parts(rng, 1, n_epochs, spe)
    g = np.zeros((n_epochs, 1), dtype=np.int64)
    r = _rows(pkg, [0], 1, n_epochs, 1, 128, D)
    y, sat, _ = mpath_model.mpath(x, g, spe, [0], r, cos1024)
    assert sat == 0 and not y[:2 * D].any() and np.array_equal(y[2 * D:], x[0, :-2 * D])
    L = mpath_model.Lines(cos1024)
    got, e0 = [], 0
    for ne in (1, 100, 3, 146, 50):  # 7, 700, 21, ... samples: the history rolls several times inside one delay
        got.append(L.call(x[:, 2 * spe * e0:2 * spe * (e0 + ne)], g[e0:e0 + ne], spe, [0], r[e0:e0 + ne])[0])
        e0 += ne
    assert e0 == n_epochs and np.array_equal(np.concatenate(got), y)


def test_phase_rotates_as_e_to_the_plus_j_theta(pkg, cos1024):
    """ph0 = 2^30 is +90 degrees: (I, Q) -> (-Q, I); dph walks the table: after N samples of dph = 2^32 / N the phase is back."""
    spe = 64
    x = np.zeros((1, 2 * spe), dtype=np.int16)
    x[0, 0::2], x[0, 1::2] = 1000, 200
    g = np.zeros((1, 1), dtype=np.int64)
    y, _, _ = mpath_model.mpath(x, g, spe, [0], _rows(pkg, [0], 1, 1, 1, 128, 0, 1 << 30, 0), cos1024)
    assert (y[0::2] == -200).all() and (y[1::2] == 1000).all()
    y, _, _ = mpath_model.mpath(x, g, spe, [0], _rows(pkg, [0], 1, 1, 1, 128, 0, 0, (1 << 32) // spe), cos1024)
    z = (y[0::2] + 1j * y[1::2]) / (1000 + 200j)
    want = np.exp(2j * np.pi * np.arange(spe) / spe)
    assert np.abs(z - want).max() < 2e-3  # Q12 table entries and the rounding of r on |u| = 1020
    y2, _, _ = mpath_model.mpath(x, g, spe, [0], _rows(pkg, [0], 1, 1, 1, 128, 0, 0, -((1 << 32) // spe)), cos1024)
    assert np.array_equal(y2[0::2][1:], y[0::2][:0:-1]) and np.array_equal(y2[1::2][1:], y[1::2][:0:-1])  # a negative step runs backwards


# ---- the int32 bound ---------------------------------------------------------------------------------------------------------------
def test_the_int32_bound_is_sum_g_plus_twice_sum_a(pkg, cos1024):
    """|x| <= 32768 and |r| <= 2 x 32768 x 4096 / 4096 = 65536 give |w| <= 32768 (sum g + 2 sum A): at 65535 |w| + 64 fits an int32,
    at 65536 it is 2^31."""
    assert 65535 * 32768 + 64 < 2 ** 31 <= 65536 * 32768
    assert 32767 * 65536 < 2 ** 31  # one echo's product A r by itself
    # the bound on r from the table: |uI c - uQ s| <= 32768 (|c| + |s|), and no entry pair sums to more than 2 x 4096
    C = cos1024.astype(np.int64)
    assert (np.abs(C) + np.abs(np.roll(C, 256))).max() <= 2 * 4096
    # rows at the bound and one beyond it, on full-scale input: the exact w of the model against the int32 range
    for extra, wide in ((0, False), (1, True)):
        gains = np.array([[32767, 32168 + extra]])
        r = _rows(pkg, [0, 1], 2, 1, 2, [[100, 200]])
        assert int(gains.sum()) + 2 * int(r["gain_q7"].astype(np.int64).sum()) == 65535 + extra
        assert mpath_model.needs_int64(gains, r) == wide
        worst = 32768 * int(gains.sum()) + 65536 * int(r["gain_q7"].astype(np.int64).sum())  # every x at -32768, every r at its bound
        assert (worst + 64 < 2 ** 31) == (not wide)
    # and the largest |r| that the table lets full-scale input reach stays inside the bound the admission uses
    u = np.array([-32768, 32767], dtype=np.int64)
    big = max(abs(int((a * c - b * s + 2048) >> 12)) for a in u for b in u for c, s in zip(C, np.roll(C, 256)))
    assert 46000 < big <= 65536


# ---- host-only entry points --------------------------------------------------------------------------------------------------------
def test_echo_row_layout(pkg):
    from galileo_sdr_sim_amd import synth

    assert ctypes.sizeof(synth._Echo) == 16 and synth.ECHO_DTYPE.itemsize == 16 and pkg.ECHO_DTYPE == mpath_model.ECHO_DTYPE
    assert [synth.ECHO_DTYPE.fields[k][1] for k in ("gain_q7", "delay", "ph0", "dph", "reserved")] == [0, 2, 4, 8, 12]
    assert [getattr(synth._Echo, k).offset for k in ("gain_q7", "delay", "ph0", "dph", "reserved")] == [0, 2, 4, 8, 12]
    assert ctypes.sizeof(synth._MpathEcho) == 16
    assert (synth.GAL_ECHO_MAX, synth.GAL_ECHO_MAX_DELAY, synth.GAL_ECHO_LINES) == (32, 1024, 64)


def _refused(fn, *args, **kw):
    from galileo_sdr_sim_amd import synth

    with pytest.raises(synth.GalSynthError) as e:
        fn(*args, **kw)
    assert e.value.code == GAL_E_INVAL
    return str(e.value)


def test_mpath_check(pkg):
    ok = mpath_model.rows(3, 2, 32767, 1024, 0xffffffff, -(1 << 31))
    pkg.mpath_check(ok, [0, 63], 64)
    pkg.mpath_check(mpath_model.rows(3, 0), [], 1)
    pkg.mpath_check(mpath_model.rows(1, 32), [0] * 32, 1)
    assert "33 echoes" in _refused(pkg.mpath_check, mpath_model.rows(1, 33), [0] * 33, 1)
    assert "part 2" in _refused(pkg.mpath_check, ok, [0, 2], 2)
    assert "part -1" in _refused(pkg.mpath_check, ok, [-1, 0], 2)
    assert "n_parts 65" in _refused(pkg.mpath_check, ok, [0, 0], 65)
    assert "n_parts 0" in _refused(pkg.mpath_check, ok, [0, 0], 0)
    for field, value, text in (("gain_q7", 32768, "gain 32768 of epoch 1, echo 1"), ("delay", 1025, "delay 1025 of epoch 1, echo 1"),
                               ("reserved", 1, "reserved = 1 in epoch 1, echo 1")):
        bad = ok.copy()
        bad[field][1, 1] = value
        assert text in _refused(pkg.mpath_check, bad, [0, 1], 2)
    lib = pkg.load_library()
    pof = np.zeros(2, dtype=np.int32)
    assert lib.gal_synth_mpath_check(ok.ctypes.data, 2, 0, pof.ctypes.data, 2) == GAL_E_INVAL  # no epochs
    assert lib.gal_synth_mpath_check(None, 2, 3, pof.ctypes.data, 2) == GAL_E_INVAL
    assert lib.gal_synth_mpath_check(ok.ctypes.data, 2, 3, None, 2) == GAL_E_INVAL
    assert lib.gal_synth_mpath_check(None, 0, 3, None, 2) == 0  # no echoes: the pointers are not looked at
    assert lib.gal_synth_mpath_check(ok.ctypes.data, -1, 3, pof.ctypes.data, 2) == GAL_E_INVAL


def test_mpath_make_and_row(pkg):
    fs = 10.4e6
    for args in ((30.0 / 299792458.0, -6.0, 90.0, 0.0), (0.0, 0.0, 0.0, 0.0), (1024 / fs, 6.0, -45.0, 2.5), (3.3e-6, -20.0, 725.0, -0.75),
                 (1e-6, -3.0, 359.99999999, 5e6)):
        got = pkg.mpath_make(*args, sample_rate=fs)
        assert got == mpath_model.make(*args, fs), args
    e = pkg.mpath_make(100.0 / 299792458.0, -6.0, 90.0, 0.0, sample_rate=2.6e6)
    assert e == {"delay": 1, "alpha_q12": 2053, "ph0": 1 << 30, "dph": 0}
    assert pkg.mpath_make(0, 6.0205999, 0, 0)["alpha_q12"] == 8192
    assert "more than 1024" in _refused(pkg.mpath_make, 1025 / fs, 0, 0, 0, sample_rate=fs)
    assert "more than 2" in _refused(pkg.mpath_make, 0, 6.03, 0, 0, sample_rate=fs)
    assert "sample_rate / 2" in _refused(pkg.mpath_make, 0, 0, 0, fs / 2, sample_rate=fs)
    assert "sample_rate / 2" in _refused(pkg.mpath_make, 0, 0, 0, -fs, sample_rate=fs)
    for bad in ((-1e-9, 0, 0, 0, fs), (float("nan"), 0, 0, 0, fs), (0, float("inf"), 0, 0, fs), (0, 0, float("nan"), 0, fs),
                (0, 0, 0, float("inf"), fs), (0, 0, 0, 0, 0.0), (0, 0, 0, 0, float("nan"))):
        assert "must be finite" in _refused(pkg.mpath_make, *bad[:4], sample_rate=bad[4])
    assert pkg.load_library().gal_synth_mpath_make(0.0, 0.0, 0.0, 0.0, fs, None) == GAL_E_INVAL
    # the per-epoch rule: A[e] = (g alpha + 2048) >> 12 capped, ph0[e + 1] = ph0[e] + N dph modulo 2^32
    echo = pkg.mpath_make(2e-6, -4.0, 33.0, 1234.5, sample_rate=fs)
    gains = [0, 1, 128, 129, 20000, 32767]
    N = 1040001
    col = pkg.mpath_rows(echo, gains, 4100, N)
    assert np.array_equal(col, mpath_model.column(echo, gains, 4100, N))
    assert [int(a) for a in col["gain_q7"]] == [(g * echo["alpha_q12"] + 2048) >> 12 for g in gains]
    assert ((col["ph0"][1:].astype(np.int64) - col["ph0"][:-1]) % (1 << 32) == (N * echo["dph"]) % (1 << 32)).all()
    assert (col["delay"] == echo["delay"]).all() and (col["dph"] == echo["dph"]).all() and not col["reserved"].any()
    loud = dict(echo, alpha_q12=8192)
    assert [int(a) for a in pkg.mpath_rows(loud, [16383, 16384, 32767], 0, N)["gain_q7"]] == [32766, 32767, 32767]  # the cap
    _refused(pkg.mpath_rows, dict(echo, alpha_q12=8193), [128], 0, N)
    _refused(pkg.mpath_rows, dict(echo, delay=1025), [128], 0, N)
    _refused(pkg.mpath_rows, echo, [32768], 0, N)
    _refused(pkg.mpath_rows, echo, [128], 0, 0)


def test_compute_entry_points_need_a_gpu_or_refuse(pkg):
    """Null handles are refused before any device work."""
    lib = pkg.load_library()
    assert lib.gal_synth_mpath_reset(None) == GAL_E_INVAL
    assert lib.gal_synth_iq_mpath(None, None, 1, None, None, 1, None, None, 0, None) == GAL_E_INVAL
    assert lib.gal_synth_run_mpath(None, None, 1, None, None, None, None, 0, None, None) == GAL_E_INVAL
    assert lib.gal_synth_run_mpath(None, None, 1, None, None, None, None, 1, None, None) == GAL_E_INVAL


# ---- one echo, despread ------------------------------------------------------------------------------------------------------------
# Measured on the CPU model (this test prints it): the largest |S_with_echo - superposition| over the whole periods and delays 0 .. 4
# half chips, relative to the direct prompt |S|.  It comes from the D = 4 samples at each period edge that the delayed stream carries
# over from the neighbouring period (4 of 16 368 samples, times alpha, with either sign), the Q12 / Q7 roundings of r and y, and
# the replica's 512-entry carrier table, whose index can step between sample n - D and sample n.  DESIGN.md section 18 quotes it.
ECHO_RESIDUAL_MEASURED = 5.1e-4  # 5.065e-4 as printed


def test_one_echo_is_the_superposition_of_two_correlations(pkg, cos1024):
    """One satellite from the oracle at 4.092 MS/s (two samples per half chip) plus one echo, D = 4 samples = 2 half chips, alpha = 0.5,
    phase 90 degrees.  Despread by the correlator model at the delays 0 .. 4 half chips: S(k) = S_direct(k) + alpha e^{j (theta - 2 pi
    f_carr D / fs)} S_direct(k - 2), S_direct the correlations of the echo-free stream."""
    fs, N, n_epochs, D = 4.092e6, 40920, 2, 4
    p = pkg.workloads.make_synthetic(n_epochs=n_epochs, n_chan=1, n_slots=16, samples_per_epoch=N, sample_rate=fs, prns=[11], seed=18)
    x, _ = oracle_run(p, N, fs)
    echo = pkg.mpath_make(D / fs, 20 * math.log10(0.5), 90.0, 0.0, sample_rate=fs)
    assert echo == {"delay": 4, "alpha_q12": 2048, "ph0": 1 << 30, "dph": 0}
    g = np.full((n_epochs, 1), 128)
    rows = pkg.mpath_rows(echo, g[:, 0], 0, N).reshape(n_epochs, 1)
    assert (rows["gain_q7"] == 64).all()
    y, sat, _ = mpath_model.mpath(x[None, :], g, N, [0], rows, cos1024)
    assert sat == 0
    T = pkg.tables()
    q = pkg.corr_from_epoch(p[0, 0], fs, 0, max_periods=5, delay0=-2, n_delay=7)
    Sx = corr_model.correlate(x, q, T)[1:4].astype(np.float64)  # whole periods only; delays -2 .. 4
    Sy = corr_model.correlate(y, dict(q, delay0=0, n_delay=5), T)[1:4].astype(np.float64)  # delays 0 .. 4
    cx = np.stack([Sx[..., 0] + 1j * Sx[..., 1], Sx[..., 2] + 1j * Sx[..., 3]], axis=-1)  # [m, d, k, (B, C)]
    cy = np.stack([Sy[..., 0] + 1j * Sy[..., 1], Sy[..., 2] + 1j * Sy[..., 3]], axis=-1)
    f_carr = float(p["f_carr"][0, 0])
    rot = 0.5 * np.exp(1j * (math.pi / 2 - 2 * math.pi * f_carr * D / fs))
    want = cx[:, :, 2:7] + rot * cx[:, :, 0:5]
    prompt = np.abs(cx[:, 0, 2, 0]).min()
    assert prompt > 0.9 * 16368 * 250 ** 2 * 0.95
    residual = np.abs(cy - want).max() / prompt
    effect = np.abs(cy - cx[:, :, 2:7]).max() / prompt
    print("echo residual %.3e of the prompt correlation; the echo itself moves the sums by %.3f of it" % (residual, effect))
    assert effect > 0.45  # at delay 2 the echo's own peak, alpha = 0.5 of the prompt
    assert residual <= 3 * ECHO_RESIDUAL_MEASURED
