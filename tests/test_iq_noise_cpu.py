"""The noise floor without a GPU: the numpy model's Philox against published known answers, the library's table against the
definition, the exact moments of the Gaussian word, gal_synth_noise_from_cn0, the argument checks that come before any device work,
and the CLI's option checks."""
import ctypes
import math
import os
import subprocess
from statistics import NormalDist

import numpy as np
import pytest

import noise_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
GAL_E_INVAL = -1


def test_model_philox_known_answers():
    """Philox4x32-10 of Random123 (kat_vectors: zeros, all ones, digits of pi)."""
    kat = [
        ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
    ]
    for ctr, key, want in kat:
        got = " ".join("%08x" % int(w[0]) for w in noise_model.philox4x32_10(*ctr, *key))
        assert got == want
    # vectorised over counters = one at a time
    many = noise_model.philox4x32_10(np.arange(5), 7, 3, 0, 11, 13)
    for i in range(5):
        one = noise_model.philox4x32_10(i, 7, 3, 0, 11, 13)
        assert [int(w[i]) for w in many] == [int(w[0]) for w in one]


def test_model_value_index():
    """The noise of a value depends on (seed, stream, J) only: any window of the stream, cut anywhere, is the same values."""
    z = noise_model.noise_z(5, 2, 0, 1000)
    for a, n in ((0, 1), (1, 7), (2, 9), (3, 100), (6, 994), (997, 3)):
        assert np.array_equal(noise_model.noise_z(5, 2, a, n), z[a:a + n])
    hi = (1 << 35) + 2
    assert np.array_equal(noise_model.noise_z(5, 2, hi + 1, 50), noise_model.noise_z(5, 2, hi, 51)[1:])
    assert not np.array_equal(noise_model.noise_z(5, 2, hi, 50), noise_model.noise_z(5, 2, hi - (1 << 34), 50))  # counter word 1
    assert not np.array_equal(noise_model.noise_z(5, 3, 0, 1000), z) and not np.array_equal(noise_model.noise_z(6, 2, 0, 1000), z)
    assert not np.array_equal(noise_model.noise_z(5 + (1 << 32), 2, 0, 1000), z)  # key word 1


def test_library_table_is_the_definition(pkg):
    t = pkg.tables()["gauss"]
    assert t.shape == (32, 32, 2) and t.dtype == np.int32
    nd = NormalDist()

    def q12(v):
        return int(round(-4096.0 * nd.inv_cdf(v / 4294967296.0)))

    for o in range(31):
        for s in range(32):
            want = (q12(2.0 ** (30 - o) * (1 + s / 32.0)), q12(2.0 ** (30 - o) * (1 + (s + 1) / 32.0)))
            assert (int(t[o, s, 0]), int(t[o, s, 1])) == want, (o, s)
    assert q12(0.5) == 25960 and (t[31] == 25960).all()
    assert np.array_equal(t, noise_model.gauss_table())
    # one 32-bit word per cell in the kernel's LDS copy: a and a - b both fit 16 bits
    assert (t[..., 0] >= t[..., 1]).all() and t.min() >= 0 and t.max() < 65536


def test_exact_moments_of_z():
    var, kurt = noise_model.z_moments()
    print("variance %.6f kurtosis %.6f" % (var, kurt))
    assert abs(var - 1.0) <= 2e-4
    assert abs(kurt - 3.0) <= 1e-3
    z = noise_model.gauss_q12(np.array([0, 0x80000000, 0x7FFFFFFF, 0xFFFFFFFF, 1, 0x40000000], dtype=np.uint64))
    assert list(z) == [25960, -25960, 0, 0, int(noise_model.gauss_table()[30, 0, 0]), int(noise_model.gauss_table()[0, 0, 0])]
    assert np.abs(noise_model.noise_z(1, 0, 0, 1 << 16)).max() <= 25960  # 6.338 sigma


def _from_cn0(lib, cn0, rate, gain):
    n = (ctypes.c_uint32 * 6)(*([0xDEADBEEF] * 6))  # gal_iq_noise_t: u64 seed, u32 stream, gain_q16, sigma_q4, reserved
    lib.gal_synth_noise_from_cn0.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    rc = lib.gal_synth_noise_from_cn0(cn0, rate, gain, ctypes.cast(n, ctypes.c_void_p))
    return rc, list(n)


def test_noise_from_cn0(pkg):
    lib = pkg.load_library()
    for cn0 in (25.0, 35.0, 40.0, 45.0, 50.5, 60.0):
        for rate in (2.6e6, 5.2e6, 16.368e6):
            for gain in (1.0, 0.5, 0.25, 0.7, 2.0):
                rc, n = _from_cn0(lib, cn0, rate, gain)
                want_g = int(round(gain * 65536.0))
                want_s = int(round(16.0 * 250.0 * gain * math.sqrt(rate / 10.0 ** (cn0 / 10.0))))
                if want_s > 1 << 20:
                    assert rc == GAL_E_INVAL, (cn0, rate, gain)
                    continue
                assert rc == 0, (cn0, rate, gain)
                assert n[0] == 0 and n[1] == 0 and n[2] == 0 and n[5] == 0  # seed, stream, reserved
                assert n[3] == want_g and abs(n[4] - want_s) <= 1, (cn0, rate, gain, n)
                assert (want_g, want_s) == noise_model.noise_from_cn0(cn0, rate, gain)
    rc, n = _from_cn0(lib, 45.0, 2.6e6, 1.0)
    assert rc == 0 and abs(n[4] / 16.0 - 2267.0) < 1.0  # sigma ~ 2267 LSB
    d = pkg.noise_from_cn0(45.0, 2.6e6)
    assert d == {"seed": 0, "stream": 0, "gain_q16": 65536, "sigma_q4": n[4]}
    assert pkg.noise_from_cn0(45.0, 2.6e6, gain=0.5)["gain_q16"] == 32768


def test_noise_from_cn0_errors(pkg):
    lib = pkg.load_library()
    nan, inf = float("nan"), float("inf")
    for cn0, rate, gain in ((nan, 2.6e6, 1.0), (inf, 2.6e6, 1.0), (-inf, 2.6e6, 1.0), (45.0, nan, 1.0), (45.0, inf, 1.0), (45.0, 0.0, 1.0),
                            (45.0, -2.6e6, 1.0), (45.0, 2.6e6, nan), (45.0, 2.6e6, -0.5), (45.0, 2.6e6, 16.5), (45.0, 2.6e6, inf),
                            (-20.0, 2.6e6, 1.0)):  # -20 dB-Hz: sigma 4 M LSB, beyond sigma_q4
        rc, _ = _from_cn0(lib, cn0, rate, gain)
        assert rc == GAL_E_INVAL, (cn0, rate, gain)
        assert b"gal_synth_noise_from_cn0" in lib.gal_synth_last_error()
    lib.gal_synth_noise_from_cn0.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    assert lib.gal_synth_noise_from_cn0(45.0, 2.6e6, 1.0, None) == GAL_E_INVAL
    with pytest.raises(pkg.GalSynthError):
        pkg.noise_from_cn0(nan, 2.6e6)


def test_convert_noise_rejects_a_null_handle(pkg):
    lib = pkg.load_library()
    buf = ctypes.create_string_buffer(96)
    addr = (ctypes.addressof(buf) + 15) & ~15
    noise = pkg.synth._Noise(1, 0, 65536, 16, 0)
    assert lib.gal_synth_iq_convert_noise(None, addr, 4, 0, ctypes.byref(noise), 1, 5, addr + 32) == GAL_E_INVAL
    assert b"null" in lib.gal_synth_last_error()
    assert lib.gal_synth_iq_convert_noise(None, addr, 4, 0, None, 1, 5, addr + 32) == GAL_E_INVAL  # noise == NULL: gal_synth_iq_convert
    assert lib.gal_synth_iq_convert_noise(None, addr, 4, 0, ctypes.byref(noise), 0, 0, addr) == GAL_E_INVAL


def test_symbols_and_python_surface(pkg):
    lib = ctypes.CDLL(pkg.synth.LIB_PATH)
    for name in ("gal_synth_iq_convert_noise", "gal_synth_noise_from_cn0", "gal_tables_gauss"):
        assert name in pkg.synth.EXPORTED_SYMBOLS and hasattr(lib, name)
    hooks = ctypes.CDLL(pkg.synth.HOOKS_LIB_PATH)
    assert hasattr(hooks, "gal_synth_iq_convert_noise")
    assert ctypes.sizeof(pkg.synth._Noise) == 24
    n = pkg.synth._noise_struct({"seed": 2**63 + 5, "gain_q16": 65536, "sigma_q4": 3})
    assert (n.seed, n.stream, n.gain_q16, n.sigma_q4, n.reserved) == (2**63 + 5, 0, 65536, 3, 0)
    n = pkg.synth._noise_struct((1, 2, 3, 4))
    assert (n.seed, n.stream, n.gain_q16, n.sigma_q4) == (1, 2, 3, 4)
    with pytest.raises(ValueError):
        pkg.synth._noise_struct({"seed": 1, "gain": 1.0, "sigma_q4": 3})


def _cli(*args):
    return subprocess.run([CLI, "-e", NAV, "-l", "-6,51,100", "-t", "2022/02/20,12:00:00", "-d", "1", "-P", "0"] + list(args),
                          capture_output=True, text=True, timeout=120)


def test_cli_noise_option_errors(pkg, tmp_path):
    out = str(tmp_path / "x.bin")
    r = _cli("--noise-seed", "3", "-o", out)
    assert r.returncode == 1 and "need --cn0" in r.stderr
    r = _cli("--signal-gain", "0.5", "-o", out)
    assert r.returncode == 1 and "need --cn0" in r.stderr
    r = _cli("--cn0", "loud", "-o", out)
    assert r.returncode == 1 and "not a number" in r.stderr
    r = _cli("--cn0", "-30", "-o", out)  # sigma beyond what sigma_q4 holds
    assert r.returncode == 1 and "--cn0" in r.stderr
    r = _cli("--cn0", "45", "--signal-gain", "0", "-o", out)
    assert r.returncode == 1 and "0 < g <= 16" in r.stderr
    r = _cli("--cn0", "45", "--signal-gain", "17", "-o", out)
    assert r.returncode == 1 and "0 < g <= 16" in r.stderr
    r = _cli("--cn0", "45", "--noise-seed", "-1", "-o", out)
    assert r.returncode == 1 and "unsigned 64-bit" in r.stderr
    r = _cli("--cn0", "45", "--noise-seed", "18446744073709551616", "-o", out)
    assert r.returncode == 1 and "unsigned 64-bit" in r.stderr
    r = _cli("--cn0", "45", "--noise-stream", "4294967296", "-o", out)
    assert r.returncode == 1 and "unsigned 32-bit" in r.stderr
    assert not os.path.exists(out)
    u = subprocess.run([CLI], capture_output=True, text=True)
    for opt in ("--cn0", "--noise-seed", "--noise-stream", "--signal-gain"):
        assert opt in u.stdout


def test_cli_prints_the_chosen_gain_and_shift(pkg, tmp_path):
    """The choices are made, and printed, before any device work: they show on a machine without a GPU too (where the run then stops)."""
    out = str(tmp_path / "x.bin")
    want = {"45": ("signal gain 1 (chosen)", "--iq-shift 7 (chosen)"),  # sigma 2267: 5 sigma + 4100 = 15 435; 127 x 128 >= 9068
            "35": ("signal gain 0.5 (chosen)", "--iq-shift 7 (chosen)"),  # sigma(1) 7169 -> g 0.5: sigma 3584.6, 4 sigma = 14 338
            "30": ("signal gain 0.25 (chosen)", "--iq-shift 7 (chosen)")}  # sigma(1) 12 748 -> g 0.25: sigma 3187
    for cn0, (gain, shift) in want.items():
        r = _cli("--cn0", cn0, "--iq-format", "ibyte", "-o", out)
        line = [ln for ln in r.stderr.splitlines() if ln.startswith("Noise floor")]
        assert len(line) == 1 and gain in line[0] and shift in line[0] and "seed 1, stream 0" in line[0], r.stderr
    r = _cli("--cn0", "45", "--iq-format", "ibyte", "--iq-shift", "6", "--signal-gain", "0.5", "--noise-seed", "0x10", "-o", out)
    line = [ln for ln in r.stderr.splitlines() if ln.startswith("Noise floor")][0]
    assert "signal gain 0.5," in line and "--iq-shift 6" in line and "chosen" not in line and "seed 16" in line
