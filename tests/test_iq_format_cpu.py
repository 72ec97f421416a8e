"""The 8-bit and 1-bit IQ output formats without a GPU: the byte counts of gal_synth_iq_bytes, the argument checks of the two
device entry points on a null handle, and the CLI's option checks, which all come before any device work."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
GAL_E_INVAL = -1


def test_iq_bytes(pkg):
    lib = pkg.load_library()
    for n in (0, 1, 2, 3, 4, 5, 7, 8, 1023, 260000, 260001, 311740000, 15 * 10**9 + 3):
        assert lib.gal_synth_iq_bytes(0, n) == 4 * n
        assert lib.gal_synth_iq_bytes(1, n) == 2 * n
        assert lib.gal_synth_iq_bytes(2, n) == (n + 3) // 4
        for bad in (-1, 3, 100):
            assert lib.gal_synth_iq_bytes(bad, n) == 0
    assert pkg.iq_bytes("ishort", 10) == 40 and pkg.iq_bytes("ibyte", 10) == 20 and pkg.iq_bytes("ibit", 10) == 3
    assert pkg.IQ_FORMATS == {"ishort": 0, "ibyte": 1, "ibit": 2}
    with pytest.raises(ValueError):
        pkg.iq_bytes("icomplex", 4)


def test_iq_entry_points_reject_a_null_handle(pkg):
    lib = pkg.load_library()
    buf = ctypes.create_string_buffer(64)
    addr = (ctypes.addressof(buf) + 15) & ~15
    assert lib.gal_synth_iq_convert(None, addr, 4, 1, 5, addr) == GAL_E_INVAL
    assert lib.gal_synth_iq_convert(None, addr, 4, 0, 0, addr) == GAL_E_INVAL
    n = ctypes.c_uint64(7)
    assert lib.gal_synth_iq_saturated(None, ctypes.byref(n), 0) == GAL_E_INVAL
    assert b"null" in lib.gal_synth_last_error()


def _cli(*args):
    return subprocess.run([CLI, "-e", NAV, "-l", "-6,51,100", "-t", "2022/02/20,12:00:00", "-d", "1", "-P", "0"] + list(args),
                          capture_output=True, text=True, timeout=120)


def test_cli_iq_option_errors(pkg, tmp_path):
    out = str(tmp_path / "x.bin")
    r = _cli("--iq-format", "bogus", "-o", out)
    assert r.returncode == 1 and "ishort, ibyte, ibit" in r.stderr and "bogus" in r.stderr
    r = _cli("--iq-format", "ibyte", "--iq-shift", "16", "-o", out)
    assert r.returncode == 1 and "0..15" in r.stderr
    r = _cli("--iq-format", "ibyte", "--iq-shift", "-1", "-o", out)
    assert r.returncode == 1 and "0..15" in r.stderr
    r = _cli("--iq-format", "ibit", "--iq-shift", "3", "-o", out)
    assert r.returncode == 1 and "ibyte only" in r.stderr
    r = _cli("--iq-shift", "5", "-o", out)  # (ishort, the default format)
    assert r.returncode == 1 and "ibyte only" in r.stderr
    for r in (_cli("--iq-format", "bogus", "-o", out), _cli("--iq-format", "ibit", "--iq-shift", "1", "-o", out)):
        assert "Start =" not in r.stderr  # rejected before the scenario is opened
    assert not os.path.exists(out)
    u = subprocess.run([CLI], capture_output=True, text=True)
    assert "--iq-format" in u.stdout and "--iq-shift" in u.stdout
