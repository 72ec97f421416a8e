"""galileo-sdr-sim --lo-offset / --phase-noise on the MI355X: the file does not depend on the batch length; a zero offset is the run
without the option; the file is the numpy model (tests/osc_model.py) over the same command's file without the oscillator; --oversample
keeps the file's size; --monitor follows the oscillator (no Doppler-bin offset, the C/N0 of the run without it); the refusals."""
import hashlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import osc_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
START = "2022/02/20,12:00:00"
SCEN = ["-e", NAV, "-l", "-6,51,100", "-t", START, "-d", "2", "-U", "1", "-b", "1", "-I", "1", "-P", "0", "--cn0", "45"]  # G1's sky, 19 epochs
EPOCHS = 19
SAMPLES = EPOCHS * 260000
FS = 2.6e6
FC = 1575.42e6
OSC = ["--lo-offset", "1500,2", "--phase-noise", "1e-21"]


def _run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=600)


def _ok(args):
    r = _run(SCEN + args)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _md5(path):
    return hashlib.md5(open(str(path), "rb").read()).hexdigest()


def _monitor(path):
    lines = open(str(path)).read().strip().split("\n")
    assert lines[0] == "time_s,prn,doppler_hz,cn0_dbhz,peak_ratio,best_delay_halfchips,best_doppler_bins"
    rows = [ln.split(",") for ln in lines[1:]]
    return {(round(float(r[0]), 1), int(r[1])): (float(r[2]), float(r[3]), int(r[5]), int(r[6])) for r in rows}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """The command's ishort file and monitor CSV without the oscillator, written once."""
    d = tmp_path_factory.mktemp("osc")
    _ok(["-o", str(d / "plain.ishort"), "--monitor", str(d / "plain.csv")])
    assert os.path.getsize(str(d / "plain.ishort")) == 4 * SAMPLES
    return d / "plain.ishort", d / "plain.csv"


def test_the_file_does_not_depend_on_the_batch_length_and_is_the_model(pkg, plain, tmp_path):
    a, b = tmp_path / "a.ishort", tmp_path / "b.ishort"
    r = _ok(OSC + ["-o", str(a)])
    _ok(OSC + ["-B", "3", "-o", str(b)])
    assert _md5(a) == _md5(b) and _md5(a) != _md5(plain[0])
    assert os.path.getsize(str(a)) == 4 * SAMPLES
    line = [ln for ln in r.stderr.split("\n") if ln.startswith("Oscillator: ")]
    assert len(line) == 1 and "offset 1500.0" in line[0] and "drift 2 Hz/s" in line[0] and "rms phase" in line[0] and "linewidth" in line[0], r.stderr[-2000:]
    # the file is the model over the command's own stream without the oscillator: seed 1, stream 0, from sample 0
    o = pkg.osc_make(1500.0, 2.0, 1e-21, FS, FC)
    assert o == osc_model.make(1500.0, 2.0, 1e-21, FS, FC) and o["s"] > 0
    assert int(re.search(r"S = (\d+)", line[0]).group(1)) == o["s"]
    x = np.fromfile(str(plain[0]), dtype="<i2")
    want, _, _ = osc_model.rotate(x, o, 0, 0)
    assert np.array_equal(np.fromfile(str(a), dtype="<i2"), want)
    # another stream, another file
    c = tmp_path / "c.ishort"
    _ok(OSC + ["--osc-stream", "1", "-o", str(c)])
    assert _md5(c) != _md5(a)


@pytest.mark.parametrize("fmt", ["ishort", "ibyte"])
def test_a_zero_offset_is_the_run_without_the_option(tmp_path, fmt):
    a, b = tmp_path / ("a." + fmt), tmp_path / ("b." + fmt)
    _ok(["--iq-format", fmt, "-o", str(a)])
    _ok(["--iq-format", fmt, "--lo-offset", "0", "-o", str(b)])
    assert _md5(a) == _md5(b)


def test_oversampled_run_keeps_the_files_size(tmp_path):
    a, b = tmp_path / "a.ishort", tmp_path / "b.ishort"
    r = _ok(OSC + ["--oversample", "2", "-o", str(a)])
    _ok(OSC + ["--oversample", "2", "-B", "3", "-o", str(b)])
    assert os.path.getsize(str(a)) == 4 * SAMPLES and _md5(a) == _md5(b)
    assert "at 5.2 MS/s" in r.stderr  # the oscillator runs at the high rate


def test_the_monitor_follows_the_oscillator(plain, tmp_path):
    """Every PRN's measured Doppler-bin offset stays 0 and its C/N0 within 1 dB of the same run without --lo-offset (the two CSVs are
    compared); dopp(planned) stays the satellite's own."""
    for extra in ([], ["--oversample", "2"]):
        base = plain[1]
        if extra:
            base = tmp_path / "base.csv"
            _ok(extra + ["-o", str(tmp_path / "base.ishort"), "--monitor", str(base)])
        mon = tmp_path / "m.csv"
        _ok(OSC + extra + ["-o", str(tmp_path / "m.ishort"), "--monitor", str(mon)])
        got, want = _monitor(mon), _monitor(base)
        assert len(want) >= 10 and set(got) == set(want)
        assert sum(not math.isnan(v[1]) for v in want.values()) >= 10
        for k in want:
            assert got[k][0] == want[k][0], k  # the planned Doppler: the satellite's own
            assert got[k][3] == 0 and want[k][3] == 0, (k, got[k])
            assert got[k][2] == want[k][2], (k, got[k], want[k])
            if math.isnan(want[k][1]):  # the run without the oscillator has no figure for this line either: nothing to compare with
                assert math.isnan(got[k][1]), (k, got[k], want[k])
            else:
                assert abs(got[k][1] - want[k][1]) <= 1.0, (k, got[k], want[k])


def test_refusals(tmp_path):
    out = tmp_path / "x.ishort"
    for args, word in ((["--lo-offset", "abc"], "--lo-offset"), (["--lo-offset", "1500,"], "--lo-offset"), (["--lo-offset", "1.3e6"], "--lo-offset"),
                       (["--phase-noise", "-1e-21"], "--phase-noise"), (["--phase-noise", "x"], "--phase-noise"), (["--phase-noise", "1e-9"], "--phase-noise"),
                       (["--osc-seed", "5"], "--osc-seed"), (["--lo-offset", "10", "--osc-seed", "-3"], "--osc-seed"),
                       (["--lo-offset", "10", "--osc-stream", "4294967296"], "--osc-stream")):
        r = _run(SCEN + args + ["-o", str(out)])
        assert r.returncode == 1 and word in r.stderr, (args, r.stderr[-500:])
        assert not out.exists()
