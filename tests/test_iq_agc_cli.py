"""galileo-sdr-sim --agc / --iq-format i2bit on the MI355X: the written file and --agc-log against the numpy model (tests/agc_model.py)
applied to the same command's plain ishort file without --agc, whatever the batch length, with and without --oversample; a pulsed
jammer in the logged gain; --monitor beside the AGC; and the refusals."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import agc_model
import noise_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
START = "2022/02/20,12:00:00"
SCEN = ["-e", NAV, "-l", "-6,51,100", "-t", START, "-d", "3", "-U", "1", "-b", "1", "-I", "1", "-P", "0", "--cn0", "45"]  # 29 epochs
EPOCHS = 29
SAMPLES = EPOCHS * 260000
FS = 2.6e6
B = 2600
FORMATS = {"ishort": 0, "ibyte": None, "i2bit": 1024}  # the parameter; ibyte's shift is the one the CLI chooses and prints


def _run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=600)


def _ok(args):
    r = _run(SCEN + args)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _md5(path):
    return hashlib.md5(open(str(path), "rb").read()).hexdigest()


def _sigma(stderr):
    """The noise sigma per rail in int16 LSB, exactly as the CLI has it: sigma_q4 / 16 at the printed signal gain."""
    gain = float(re.search(r"signal gain ([0-9.e+-]+)", stderr).group(1))
    rate = FS * (int(re.search(r"Oversampling: (\d+) x", stderr).group(1)) if "Oversampling:" in stderr else 1)
    return noise_model.noise_from_cn0(45.0, rate, gain)[1] / 16.0


def _agc_line(stderr):
    line = [ln for ln in stderr.split("\n") if ln.startswith("AGC: ")]
    assert len(line) == 1, stderr[-2000:]
    return line[0]


def _read_log(path):
    lines = open(str(path)).read().strip().split("\n")
    assert lines[0] == "time_s,gain_q12,gain_db"
    rows = [ln.split(",") for ln in lines[1:]]
    return (np.array([float(r[0]) for r in rows]), np.array([int(r[1]) for r in rows], dtype=np.uint32), np.array([float(r[2]) for r in rows]))


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """The command's plain ishort file without --agc, written once and left unchanged."""
    path = tmp_path_factory.mktemp("agc") / "plain.ishort"
    r = _ok(["-o", str(path)])
    x = np.fromfile(str(path), dtype="<i2")
    assert x.size == 2 * SAMPLES
    x.setflags(write=False)
    return x, _sigma(r.stderr)


@pytest.mark.parametrize("fmt", ("i2bit", "ibyte", "ishort"))
def test_file_and_log_equal_the_model(pkg, plain, tmp_path, fmt):
    x, sigma = plain
    out, log = tmp_path / ("a." + fmt), tmp_path / "gains.csv"
    r = _ok(["--agc", "--iq-format", fmt, "-o", str(out), "--agc-log", str(log)])
    line = _agc_line(r.stderr)
    param = FORMATS[fmt]
    if fmt == "ibyte":  # the smallest shift with 127 x 2^s >= 4 sigma
        param = int(re.search(r"--iq-shift (\d+) \(chosen\)", line).group(1))
        assert 127 * (1 << param) >= 4 * sigma > 127 * (1 << (param - 1))
    target = {"ishort": 2048, "ibyte": 32 << (param or 0), "i2bit": 1024}[fmt]
    assert "target rms %d LSB, blocks of 2600 samples, window 8 blocks" % target in line
    p = agc_model.from_rms(target, sigma, B, 8)
    assert pkg.synth.agc_from_rms(target, sigma, B, 8) == p
    want, want_g, _ = agc_model.agc(x, p, 0, fmt, param)
    got = np.fromfile(str(out), dtype=np.uint8)
    assert got.size == agc_model.out_bytes(fmt, SAMPLES) == want.size
    assert np.array_equal(got, want)
    t, g, db = _read_log(log)
    assert np.array_equal(g, want_g) and g.size == SAMPLES // B
    assert np.allclose(t, np.arange(g.size) * (B / FS), atol=1e-9) and np.allclose(db, 20 * np.log10(g / 4096.0), atol=1e-4)
    # the log does not change the file
    if fmt == "i2bit":
        again = tmp_path / "b.i2bit"
        _ok(["--agc", "--iq-format", fmt, "-o", str(again)])
        assert _md5(again) == _md5(out)


@pytest.mark.parametrize("fmt", ("i2bit", "ibyte"))
def test_the_file_does_not_depend_on_the_batch_length(tmp_path, fmt):
    a, b, c = (tmp_path / ("%s.%s" % (k, fmt)) for k in "abc")
    _ok(["--agc", "--iq-format", fmt, "-o", str(a)])
    _ok(["--agc", "--iq-format", fmt, "-B", "3", "-o", str(b)])
    _ok(["--agc", "--iq-format", fmt, "-B", "7", "-o", str(c)])
    assert _md5(a) == _md5(b) == _md5(c)
    assert os.path.getsize(str(a)) == agc_model.out_bytes(fmt, SAMPLES)


def test_oversampled_file_is_the_model_over_the_commands_own_stream(pkg, tmp_path):
    """--oversample 2: the AGC runs behind the decimator, at the output rate: the file keeps its size, and it is the model over the
    same command's un-AGC'd ishort file, with the sigma behind the filter as the initial rms."""
    un, out, b3 = tmp_path / "un.ishort", tmp_path / "a.i2bit", tmp_path / "b.i2bit"
    r0 = _ok(["--oversample", "2", "-o", str(un)])
    r = _ok(["--oversample", "2", "--iq-format", "i2bit", "-o", str(out)])
    _ok(["--oversample", "2", "--iq-format", "i2bit", "-B", "3", "-o", str(b3)])
    assert _md5(out) == _md5(b3)
    x = np.fromfile(str(un), dtype="<i2")
    assert x.size == 2 * SAMPLES and os.path.getsize(str(out)) == SAMPLES // 2
    taps = [ln for ln in r.stderr.split("\n") if ln.startswith("Front-end filter:")]
    h = np.array([int(v) for v in taps[0].split(":")[-1].split()], dtype=np.float64)
    sigma_out = _sigma(r.stderr) * np.sqrt(float((h ** 2).sum())) / 16384.0
    assert _sigma(r0.stderr) == _sigma(r.stderr)
    p = agc_model.from_rms(1024, sigma_out, B, 8)
    want, _, _ = agc_model.agc(x, p, 0, "i2bit", 1024)
    assert np.array_equal(np.fromfile(str(out), dtype=np.uint8), want)


def test_a_pulsed_jammer_shows_in_the_gain(pkg, tmp_path):
    """--jam 40,1e5,0,0,50000,10000: a tone 40 dB over one satellite, on for 10 ms of every 50 ms, blocks of 1 ms, a window of 4.  The
    jammer's power is 2 x 250^2 x 10^4 = 1.25e9, the noise 2 sigma^2 = 1.03e7 at 45 dB-Hz: a ratio of 121, a gain step of 20.9 dB; 15 dB
    leaves room for the signals and the window edges.  The settled part of a phase: the blocks whose whole window lies inside it."""
    out, log, mon = tmp_path / "j.ibyte", tmp_path / "gains.csv", tmp_path / "monitor.csv"
    _ok(["--jam", "40,1e5,0,0,50000,10000", "--agc", "--agc-block", "2600", "--agc-window", "4", "--iq-format", "ibyte", "-o", str(out),
         "--agc-log", str(log), "--monitor", str(mon)])
    t, g, db = _read_log(log)
    assert g.size == SAMPLES // B
    r = np.rint(t * FS / B).astype(np.int64) % 50  # the block's place in the pulse period: on for r = 0 .. 9
    later = np.arange(g.size) >= 50                # (the first period starts from the initial rms)
    on = later & (r >= 4) & (r <= 10)              # the window r - 4 .. r - 1 lies in 0 .. 9
    off = later & ((r >= 14) | (r == 0))           # ... in 10 .. 49
    assert on.sum() > 100 and off.sum() > 500
    assert db[on].max() <= db[off].min() - 15.0, (db[on].max(), db[off].min())
    # --monitor on this run still reports every planned PRN, at every monitored epoch
    rows = pkg.Scenario(NAV, llh=(-6, 51, 100), start=START, duration_s=3, iono_enable=False).all()
    assert rows.shape[0] == EPOCHS
    lines = mon.read_text().strip().split("\n")[1:]
    seen = {(round(float(ln.split(",")[0]), 1), int(ln.split(",")[1])) for ln in lines}
    planned = {(round(0.1 * e, 1), int(prn)) for e in (0, 10, 20) for prn in rows["prn"][e] if prn > 0}
    assert len(planned) >= 15 and seen == planned


def test_refusals_and_the_implied_agc(tmp_path):
    r = _run(SCEN + ["--iq-format", "i2bit", "--monitor", str(tmp_path / "m.csv"), "-o", str(tmp_path / "x.i2bit")])
    assert r.returncode == 1 and "--monitor" in r.stderr and "i2bit" in r.stderr
    assert not (tmp_path / "x.i2bit").exists() and not (tmp_path / "m.csv").exists()
    r = _run(SCEN + ["--agc", "--iq-format", "ibit", "-o", str(tmp_path / "x.ibit")])
    assert r.returncode == 1 and "--agc" in r.stderr and not (tmp_path / "x.ibit").exists()
    # --iq-format i2bit alone turns the AGC on, and the default name takes the extension
    short = [a if a != "3" else "1" for a in SCEN]
    r = subprocess.run([CLI] + short + ["--iq-format", "i2bit"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "target rms 1024 LSB" in _agc_line(r.stderr) and "--i2bit-threshold 1024" in _agc_line(r.stderr)
    assert os.path.getsize(str(tmp_path / "galileosim.i2bit")) == 9 * 260000 // 2
