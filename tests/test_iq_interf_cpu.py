"""The interference sources without a GPU: the model's closed-form phase against the sample-by-sample recurrence, the library's
cosine table against the definition, the physics of the model (where a tone lands, what power it has, how a chirp's frequency
moves, the duty of a pulse), gal_synth_interf_make, the argument checks that come before any device work, and the CLI's option checks."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import interf_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
GAL_E_INVAL = -1
FS = 2.6e6


@pytest.mark.parametrize("sweep_len", (0, 1, 2, 3, 7, 1000, 65537))
def test_closed_form_is_the_recurrence(sweep_len):
    src = interf_model.source(ph0=0xDEADBEEF, f0=-1234567891, df=300000007 if sweep_len else 0, sweep_len=sweep_len)
    n = max(3000, 2 * sweep_len + 10)  # two restarts at least
    assert np.array_equal(interf_model.phase(src, 0, n), interf_model.phase_recurrence(src, 0, n, src["ph0"]))
    for first in ((1 << 33) + 5, (1 << 61) + 12345):
        got = interf_model.phase(src, first, n)
        assert np.array_equal(got, interf_model.phase_recurrence(src, first, n, got[0]))
        # and the window's first phase is itself on the chain from sample 0: a window cut anywhere is the same values
        assert np.array_equal(interf_model.phase(src, first + 17, 50), got[17:67])
    if sweep_len == 0:
        assert int(interf_model.phase(src, (1 << 61) + 12345, 1)[0]) == (src["ph0"] + ((1 << 61) + 12345) * src["f0"]) % (1 << 32)
    else:
        N = (1 << 61) + 12345
        s, m = divmod(N, sweep_len)
        W = sweep_len * src["f0"] + src["df"] * (sweep_len * (sweep_len - 1) // 2)
        assert int(interf_model.phase(src, N, 1)[0]) == (src["ph0"] + s * W + m * src["f0"] + src["df"] * (m * (m - 1) // 2)) % (1 << 32)


def test_library_table_is_the_definition(pkg):
    t = pkg.tables()["cos1024"]
    assert t.shape == (1024,) and t.dtype == np.int16
    want = interf_model.cos_table()
    assert np.array_equal(t, want)
    assert t[0] == 4096 and t[256] == 0 and t[512] == -4096 and t[768] == 0
    exact = 4096.0 * np.cos(2.0 * np.pi * np.arange(1024) / 1024.0)
    assert np.abs(np.abs(exact - np.floor(exact)) - 0.5).min() > 0.006  # no entry near a rounding tie: any libm gives this table
    assert np.abs(want - exact).max() <= 0.5


def test_cw_tone_lands_on_its_bin_with_its_power():
    """x = 0, one CW source of A = 1000 LSB at bin 1237 of 65536: the FFT of y peaks there, not at the mirror bin (the sine has the
    sign of a positive frequency), and mean |y|^2 = A^2 within the quantisation of a 1024-entry Q12 table and of the int16 output
    (phase quantised to 2 pi / 1024: a loss of (2 pi / 1024)^2 / 12 = 3e-6; rounding C to Q12 and y to 1 LSB: +-1e-3 at most)."""
    n, k = 65536, 1237
    src = interf_model.source(amp_q4=16000, ph0=12345, f0=k << 16)
    y, clipped = interf_model.mix(np.zeros(2 * n, dtype=np.int16), None, [src])
    assert not clipped.any()
    z = y[0::2].astype(np.float64) + 1j * y[1::2].astype(np.float64)
    spec = np.abs(np.fft.fft(z)) ** 2
    assert int(np.argmax(spec)) == k
    assert spec[k] > 1e4 * np.delete(spec, k).max()
    power = float(np.mean(np.abs(z) ** 2)) / 1000.0 ** 2
    print("mean |y|^2 / A^2 = %.5f" % power)
    assert abs(power - 1.0) <= 2e-3
    neg = interf_model.source(amp_q4=16000, f0=-(k << 16))
    y, _ = interf_model.mix(np.zeros(2 * n, dtype=np.int16), None, [neg])
    assert int(np.argmax(np.abs(np.fft.fft(y[0::2] + 1j * y[1::2])))) == n - k


def test_chirp_phase_increments():
    """The measured phase increment of sample N is f0 + (N mod sweep_len) df: exactly in the phase, and to the table's resolution
    (2 pi / 1024 per look-up) in the angle of y."""
    src = interf_model.source(amp_q4=16 * 8000, ph0=999, f0=-(1 << 29), df=(1 << 30) // 500, sweep_len=500)
    n = 2000
    phi = interf_model.phase(src, 123, n + 1).astype(np.int64)
    m = (123 + np.arange(n)) % 500
    assert np.array_equal((phi[1:] - phi[:-1]) % (1 << 32), (src["f0"] + m * src["df"]) % (1 << 32))
    y, _ = interf_model.mix(np.zeros(2 * (n + 1), dtype=np.int16), None, [src], first_sample=123)
    ang = np.angle(y[0::2] + 1j * y[1::2].astype(np.float64))
    step = np.angle(np.exp(1j * (ang[1:] - ang[:-1])))
    want = np.angle(np.exp(2j * np.pi * ((src["f0"] + m * src["df"]) / 2.0 ** 32)))
    assert np.abs(np.angle(np.exp(1j * (step - want)))).max() <= 2 * (2 * np.pi / 1024) + 2e-3


def test_pulse_duty_is_exact():
    for period, on, first in ((5, 2, 0), (5, 2, (1 << 33) + 3), (1000, 1, 7), (7, 7, 1), (7, 0, 1)):
        src = interf_model.source(amp_q4=16000, pulse_period=period, pulse_on=on)
        g = interf_model.gate(src, first, 40 * period)
        assert int(g.sum()) == 40 * on
        y, _ = interf_model.mix(np.zeros(80 * period, dtype=np.int16), None, [src], first_sample=first)
        assert np.array_equal(y[0::2] != 0, g.astype(bool))  # f0 = 0, ph0 = 0: I = A while on
    assert interf_model.gate(interf_model.source(amp_q4=1), 5, 100).all()  # period 0: always on


def test_interf_make(pkg):
    lib = pkg.load_library()
    keys = interf_model.FIELDS
    for js in (-10.0, 0.0, 20.0, 33.3, 40.0):
        for gain in (1.0, 0.5, 0.25, 0.7):
            for args in ((1e5,), (-1.2e6,), (0.0,), (-1e6, 1e6, 100e-6), (1.29e6, -1.29e6, 1e-3, 1e-2, 2e-3), (2e5, 3e5, 3.9e-7, 1.0, 1.0),
                         (5e4, 0.0, 0.0, 2e-3, 5e-4)):
                want = interf_model.interf_make(js, gain, FS, *args)
                got = pkg.interf_make(js, gain, FS, *args)
                assert set(got) == set(keys) and got["ph0"] == 0
                assert abs(got["amp_q4"] - want["amp_q4"]) <= 1 and abs(got["f0"] - want["f0"]) <= 1 and abs(got["df"] - want["df"]) <= 1, (js, gain, args)
                assert [got[k] for k in ("sweep_len", "pulse_period", "pulse_on")] == [want[k] for k in ("sweep_len", "pulse_period", "pulse_on")]
    d = pkg.interf_make(20.0, 1.0, FS, 1e5)
    assert d == {"amp_q4": 56569, "ph0": 0, "f0": 165191050, "df": 0, "sweep_len": 0, "pulse_period": 0, "pulse_on": 0}  # A = 3535.5 LSB
    # J/S against the composite signal: A^2 = (J/S) 2 (250 g)^2
    assert abs((d["amp_q4"] / 16.0) ** 2 / (2 * 250.0 ** 2) - 100.0) < 0.01
    assert pkg.interf_make(20.0, 1.0, FS, 1e5, 5e5, 0.0)["df"] == 0  # CW: f_hi is not looked at ...
    assert pkg.interf_make(20.0, 1.0, FS, 1e5, float("nan"), 0.0)["sweep_len"] == 0  # ... at all
    c = pkg.interf_make(20.0, 1.0, FS, -1e6, 1e6, 1e-3)
    assert c["sweep_len"] == 2600 and c["df"] == round(2e6 / FS * 2 ** 32 / 2600)


def test_interf_make_errors(pkg):
    lib = pkg.load_library()
    nan, inf = float("nan"), float("inf")
    good = [20.0, 1.0, FS, 1e5, 2e5, 1e-3, 1e-2, 1e-3]
    pkg.interf_make(*good)
    bad = []
    for k in range(8):
        for v in (nan, inf, -inf):
            bad.append(good[:k] + [v] + good[k + 1:])
    bad += [
        [20.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [20.0, 1.0, -FS, 0.0, 0.0, 0.0, 0.0, 0.0],  # sample rate
        [20.0, -1.0, FS, 1e5, 0.0, 0.0, 0.0, 0.0],  # gain
        [20.0, 1.0, FS, 1.3e6, 0.0, 0.0, 0.0, 0.0], [20.0, 1.0, FS, -1.3e6, 0.0, 0.0, 0.0, 0.0], [20.0, 1.0, FS, 2e6, 0.0, 0.0, 0.0, 0.0],  # |f| >= fs / 2
        [20.0, 1.0, FS, 1e5, 1.3e6, 1e-3, 0.0, 0.0], [20.0, 1.0, FS, 1e5, -1.4e6, 1e-3, 0.0, 0.0],
        [20.0, 1.0, FS, 1.3e6 * (1 - 2.0 ** -40), 0.0, 0.0, 0.0, 0.0],  # rounds to fs / 2 itself: beyond an int32 step
        [50.0, 1.0, FS, 1e5, 0.0, 0.0, 0.0, 0.0],  # 250 sqrt(2) x 316 = 111 803 LSB: beyond amp_q4
        [20.0, 400.0, FS, 1e5, 0.0, 0.0, 0.0, 0.0],
        [20.0, 1.0, FS, 1e5, 2e5, 1e-7, 0.0, 0.0],  # a sweep of 0.26 samples
        [20.0, 1.0, FS, 1e5, 2e5, -1e-3, 0.0, 0.0],
        [20.0, 1.0, FS, 1e5, 2e5, 1700.0, 0.0, 0.0], [20.0, 1.0, FS, 1e5, 0.0, 0.0, 1700.0, 1.0], [20.0, 1.0, FS, 1e5, 0.0, 0.0, 1700.0, 1700.0],  # 4.4e9 samples
        [20.0, 1.0, FS, 1e5, 0.0, 0.0, 1e-3, 2e-3], [20.0, 1.0, FS, 1e5, 0.0, 0.0, 0.0, 1e-3],  # pulse_on > pulse_period
        [20.0, 1.0, FS, 1e5, 0.0, 0.0, -1e-3, 0.0], [20.0, 1.0, FS, 1e5, 0.0, 0.0, 1e-3, -1e-3],
    ]
    for args in bad:
        out = pkg.synth._Interf(1, 2, 3, 4, 5, 6, 7, 8)
        rc = lib.gal_synth_interf_make(*args, ctypes.byref(out))
        assert rc == GAL_E_INVAL, args
        assert b"gal_synth_interf_make" in lib.gal_synth_last_error()
        assert (out.amp_q4, out.reserved) == (1, 8)  # untouched
    assert lib.gal_synth_interf_make(*good, None) == GAL_E_INVAL
    with pytest.raises(pkg.GalSynthError):
        pkg.interf_make(20.0, 1.0, FS, 2e6)


def test_convert_interf_checks_before_device_work(pkg):
    lib = pkg.load_library()
    buf = ctypes.create_string_buffer(96)
    addr = (ctypes.addressof(buf) + 15) & ~15
    Interf = pkg.synth._Interf
    one = (Interf * 1)(Interf(16000, 0, 1000, 0, 0, 0, 0, 0))
    noise = pkg.synth._Noise(1, 0, 65536, 16, 0)
    assert lib.gal_synth_iq_convert_interf(None, addr, 4, 0, ctypes.byref(noise), one, 1, 1, 5, addr + 32) == GAL_E_INVAL
    assert b"null" in lib.gal_synth_last_error()
    assert lib.gal_synth_iq_convert_interf(None, addr, 4, 0, None, one, 0, 1, 5, addr + 32) == GAL_E_INVAL  # n_interf = 0: the noise call's answer
    assert lib.gal_synth_iq_convert_interf(None, addr, 4, 0, None, one, 5, 1, 5, addr + 32) == GAL_E_INVAL
    assert b"n_interf 5" in lib.gal_synth_last_error()
    assert lib.gal_synth_iq_convert_interf(None, addr, 4, 0, None, one, -1, 1, 5, addr + 32) == GAL_E_INVAL
    assert b"n_interf -1" in lib.gal_synth_last_error()


def test_symbols_and_python_surface(pkg):
    lib = ctypes.CDLL(pkg.synth.LIB_PATH)
    for name in ("gal_synth_iq_convert_interf", "gal_synth_interf_make", "gal_tables_cos1024"):
        assert name in pkg.synth.EXPORTED_SYMBOLS and hasattr(lib, name)
    hooks = ctypes.CDLL(pkg.synth.HOOKS_LIB_PATH)
    assert hasattr(hooks, "gal_synth_iq_convert_interf")
    assert ctypes.sizeof(pkg.synth._Interf) == 32 and pkg.synth.GAL_INTERF_MAX == 4
    assert callable(pkg.interf_make)
    c = pkg.synth._interf_struct({"amp_q4": 5, "f0": -7, "sweep_len": 9, "df": -1})
    assert (c.amp_q4, c.ph0, c.f0, c.df, c.sweep_len, c.pulse_period, c.pulse_on, c.reserved) == (5, 0, -7, -1, 9, 0, 0, 0)
    with pytest.raises(ValueError):
        pkg.synth._interf_struct({"amp_q4": 1, "amplitude": 2})
    with pytest.raises(ValueError):
        pkg.synth._interf_struct({"f0": 2})
    import inspect

    assert "interf" in inspect.signature(pkg.SynthEngine.iq_convert).parameters


def _cli(*args):
    return subprocess.run([CLI, "-e", NAV, "-l", "-6,51,100", "-t", "2022/02/20,12:00:00", "-d", "1", "-P", "0"] + list(args),
                          capture_output=True, text=True, timeout=120)


def test_cli_jam_option_errors(pkg, tmp_path):
    out = str(tmp_path / "x.bin")
    for spec in ("20", "20,", ",1e5", "20,1e5,3e5", "20,1e5,3e5,100,50", "20,1e5,3e5,100,50,10,1", "loud,1e5", "20,1e5x", "20,1e5,3e5,0",
                 "20 ,1e5", ""):
        r = _cli("--jam", spec, "-o", out)
        assert r.returncode == 1 and "is not js_db,f_hz" in r.stderr, (spec, r.stderr)
    for spec in ("20,1.3e6", "20,-2e6", "20,1e5,1.3e6,100", "20,1e5,0,0.1", "20,1e5,2e5,100,10,20", "inf,1e5", "20,nan"):
        r = _cli("--jam", spec, "-o", out)
        assert r.returncode == 1 and "gal_synth_interf_make" in r.stderr, (spec, r.stderr)
    r = _cli("--jam", "60,1e5", "--signal-gain", "1", "-o", out)  # 353 553 LSB
    assert r.returncode == 1 and "amp_q4" in r.stderr
    five = []
    for k in range(5):
        five += ["--jam", "10,%d" % (1000 * k)]
    r = _cli(*five, "-o", out)
    assert r.returncode == 1 and "4 times at most" in r.stderr
    r = _cli("--jam", "20,1e5", "--noise-seed", "3", "-o", out)
    assert r.returncode == 1 and "need --cn0" in r.stderr
    r = _cli("--jam", "20,1e5", "--signal-gain", "0", "-o", out)
    assert r.returncode == 1 and "0 < g <= 16" in r.stderr
    assert not os.path.exists(out)
    assert "--jam" in subprocess.run([CLI], capture_output=True, text=True).stdout


def test_cli_prints_the_sources_gain_and_shift(pkg, tmp_path):
    """The choices are made, and printed, before any device work: they show on a machine without a GPU too (where the run then stops)."""
    out = str(tmp_path / "x.bin")
    r = _cli("--jam", "20,1e5", "-o", out)  # A = 3535.5: 4100 + 3536 <= 32767
    assert "Interference without a noise floor: signal gain 1 (chosen)\n" in r.stderr
    assert "Interference 1: J/S 20 dB -> A 3535.6 LSB, 100000.0 Hz .. 100000.0 Hz, sweep 0 samples, pulse 0 of 0 samples" in r.stderr
    assert "Noise floor" not in r.stderr
    r = _cli("--jam", "45,0", "--jam", "45,10", "--iq-format", "ibyte", "-o", out)  # 2 x 62 872 at gain 1 -> gain 0.25: 1025 + 31 436
    assert "signal gain 0.25 (chosen), --iq-shift 8 (chosen)" in r.stderr  # 127 x 256 = 32 512 >= 32 461
    assert "Interference 2: J/S 45 dB -> A 15717.9 LSB" in r.stderr
    r = _cli("--jam", "40,1e5", "--signal-gain", "0.5", "--iq-format", "ibyte", "--iq-shift", "6", "-o", out)
    assert "signal gain 0.5, --iq-shift 6\n" in r.stderr and "chosen" not in r.stderr
    # with --cn0: 5 x 2267 + 4100 + 11 180 <= 32 767 at gain 1; 127 x 2^s >= 4 x 2267 + 11 180 = 20 248: s = 8
    r = _cli("--cn0", "45", "--jam", "30,-1e6,1e6,100,1000,200", "--iq-format", "ibyte", "-o", out)
    line = [ln for ln in r.stderr.splitlines() if ln.startswith("Noise floor")]
    assert len(line) == 1 and "signal gain 1 (chosen)" in line[0] and "--iq-shift 8 (chosen)" in line[0]
    assert "Interference 1: J/S 30 dB -> A 11180.3 LSB, -1000000.0 Hz .. 1000000.0 Hz, sweep 260 samples, pulse 520 of 2600 samples" in r.stderr
    assert "Interference without" not in r.stderr
    # 35 dB-Hz alone takes gain 0.5 (5 x 7169 + 4100 = 39 945); with 30 dB of J/S 51 125 -> still 0.5: 25 563
    r = _cli("--cn0", "35", "--jam", "30,1e5", "-o", out)
    assert "signal gain 0.5 (chosen)" in r.stderr and "A 5590.2 LSB" in r.stderr
    # without --jam: the messages of before
    r = _cli("--cn0", "45", "--iq-format", "ibyte", "-o", out)
    assert "Interference" not in r.stderr and "--iq-shift 7 (chosen)" in r.stderr
