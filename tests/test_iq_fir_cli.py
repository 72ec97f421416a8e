"""galileo-sdr-sim --fir / --fir-lowpass: the argument checks (no GPU: they fail before any device work) and, on the MI355X, the
filtered file against the numpy model (tests/fir_model.py) over the same command's unfiltered file -- whatever the batch length --,
the chain noise -> filter -> ibyte against the models, and --monitor following the filter's delay."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import fir_model
import noise_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
G1 = ["-l", "-6,51,100", "-t", "2022/02/20,12:00:00", "-d", "3", "-U", "1", "-b", "1", "-I", "1", "-P", "0"]  # the golden scenario G1's sky
EPOCHS = 29
G45, S45 = noise_model.noise_from_cn0(45.0, 2.6e6, 1.0)  # the CLI chooses gain 1 at 45 dB-Hz (test_iq_noise_cli.py)


def _run(args, **kw):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=600, **kw)


def _ok(args):
    r = _run(["-e", NAV] + G1 + args)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _tap_file(path, taps):
    path.write_text("".join("%d\n" % int(t) for t in taps))
    return str(path)


def _delta(T, D):
    h = np.zeros(T, dtype=np.int16)
    h[D] = 16384
    return h


def test_fir_argument_checks(pkg, tmp_path):
    """Each of these ends with exit code 1 and its own message before the scenario is opened or a device is touched (the navigation
    file named does not even exist)."""
    nav = str(tmp_path / "does_not_exist.rnx")
    good = _tap_file(tmp_path / "good.txt", [100, 16184, 100])
    r = _run(["-e", nav, "--fir", str(tmp_path / "no_such_taps.txt")])
    assert r.returncode == 1 and "cannot read the tap file" in r.stderr
    r = _run(["-e", nav, "--fir", _tap_file(tmp_path / "t129.txt", [16384] + [0] * 128)])
    assert r.returncode == 1 and "more than 128 taps" in r.stderr
    r = _run(["-e", nav, "--fir", _tap_file(tmp_path / "t128.txt", [16384] + [0] * 127)])
    assert r.returncode == 1 and "--fir" not in r.stderr  # 128 taps are accepted: the run fails at the navigation file
    for k, bad in enumerate(("1.5\n", "abc\n", "16384 12\n", "40000\n", "0x10\n")):
        p = tmp_path / ("bad%d.txt" % k)
        p.write_text("100\n" + bad + "100\n")
        r = _run(["-e", nav, "--fir", str(p)])
        assert r.returncode == 1 and "line 2" in r.stderr and "not an integer tap" in r.stderr, bad
    empty = tmp_path / "empty.txt"
    empty.write_text("\n\n")
    r = _run(["-e", nav, "--fir", str(empty)])
    assert r.returncode == 1 and "holds no tap" in r.stderr
    r = _run(["-e", nav, "--fir", _tap_file(tmp_path / "big.txt", [32767, -32768, 1])])
    assert r.returncode == 1 and "65535" in r.stderr
    r = _run(["-e", nav, "--fir", _tap_file(tmp_path / "edge.txt", [32767, -32768])])
    assert r.returncode == 1 and "--fir" not in r.stderr  # sum |h| = 65535 is accepted
    r = _run(["-e", nav, "--fir", good, "--fir-lowpass", "1e6"])
    assert r.returncode == 1 and "exclude each other" in r.stderr
    for bad in ("", "abc", "1e6,", "1e6,x", "1e6,63,5", "1e6,62", "1e6,129", "1.3e6", "0", "-5"):
        r = _run(["-e", nav, "--fir-lowpass", bad])
        assert r.returncode == 1 and "--fir-lowpass" in r.stderr, bad
    r = _run(["-e", nav, "--fir"])
    assert r.returncode == 1
    # accepted: the taps are printed, then the run fails at the navigation file, not at the option
    r = _run(["-e", nav, "--fir-lowpass", "1e6,25"])
    assert r.returncode == 1 and "ERROR: --fir" not in r.stderr
    line = [ln for ln in r.stderr.split("\n") if ln.startswith("Front-end filter:")]
    assert len(line) == 1 and "25 taps" in line[0]
    printed = np.array([int(v) for v in line[0].split(":")[-1].split()])
    assert np.array_equal(printed, pkg.synth.fir_lowpass(1.0e6, 2.6e6, 25))
    r = _run(["-e", nav, "--fir-lowpass", "1e6"])
    assert r.returncode == 1 and "63 taps" in r.stderr
    r = _run(["-e", nav, "--fir", good])
    assert r.returncode == 1 and "--fir" not in r.stderr
    h = _run(["-e"])
    assert "--fir <file>" in h.stdout and "--fir-lowpass <cutoff_hz>[,n_taps]" in h.stdout


def _md5(path):
    return hashlib.md5(open(str(path), "rb").read()).hexdigest()


@pytest.fixture(scope="module")
def clean(tmp_path_factory):
    """The unfiltered ishort file of the scenario, read once and left unchanged."""
    path = tmp_path_factory.mktemp("fir_cli") / "clean.ishort"
    r = _ok(["-o", str(path)])
    assert "Front-end filter" not in r.stderr
    x = np.fromfile(str(path), dtype="<i2")
    assert x.size == EPOCHS * 520000
    x.setflags(write=False)
    return x


@pytest.mark.gpu
def test_unity_tap_is_the_unfiltered_file(clean, tmp_path):
    out = tmp_path / "unity.ishort"
    r = _ok(["--fir", _tap_file(tmp_path / "unity.txt", [16384]), "-o", str(out)])
    assert out.read_bytes() == clean.tobytes()
    assert "saturated" not in r.stderr


@pytest.mark.gpu
def test_filtered_file_is_the_model_whatever_the_batch(pkg, clean, tmp_path):
    taps = pkg.synth.fir_lowpass(1.0e6, 2.6e6, 25)
    tf = _tap_file(tmp_path / "lp25.txt", taps)
    a, b = tmp_path / "a.ishort", tmp_path / "b.ishort"
    _ok(["--fir", tf, "-o", str(a)])
    _ok(["--fir", tf, "-B", "7", "-o", str(b)])
    assert _md5(a) == _md5(b)
    want, sat = fir_model.fir(clean, taps)
    assert sat == 0 and np.count_nonzero(want != clean) > 0.5 * clean.size
    assert a.read_bytes() == want.astype("<i2").tobytes()
    # --fir-lowpass makes the same taps, hence the same file
    c = tmp_path / "c.ishort"
    _ok(["--fir-lowpass", "1e6,25", "-B", "11", "-o", str(c)])
    assert _md5(c) == _md5(a)


@pytest.mark.gpu
def test_noise_then_filter_then_ibyte(pkg, clean, tmp_path):
    taps = pkg.synth.fir_lowpass(1.0e6, 2.6e6, 25)
    tf = _tap_file(tmp_path / "lp25.txt", taps)
    args = ["--fir", tf, "--cn0", "45", "--noise-seed", "7", "--iq-format", "ibyte", "--iq-shift", "7"]
    a, b = tmp_path / "a.ibyte", tmp_path / "b.ibyte"
    _ok(args + ["-o", str(a)])
    _ok(args + ["-B", "7", "-o", str(b)])
    assert _md5(a) == _md5(b)
    noisy, sat_n = noise_model.convert(clean, "ishort", 0, (7, 0, G45, S45))
    filtered, sat_f = fir_model.fir(noisy.view("<i2"), taps)
    want, _ = noise_model.convert(filtered, "ibyte", 7, (0, 0, 65536, 0))
    assert sat_n == 0 and sat_f == 0
    assert a.read_bytes() == want.tobytes()


@pytest.mark.gpu
def test_monitor_follows_the_filter_delay(tmp_path):
    """A pure delay of 12 samples = 9.4 half chips: without the delay handling no line would name the planned delay."""
    tf = _tap_file(tmp_path / "delay12.txt", _delta(25, 12))
    args = ["--fir", tf, "--cn0", "45"]
    with_mon, without = tmp_path / "a.ishort", tmp_path / "b.ishort"
    mon = tmp_path / "monitor.csv"
    _ok(args + ["-o", str(with_mon), "--monitor", str(mon), "--monitor-every", "10"])
    _ok(args + ["-o", str(without)])
    assert _md5(with_mon) == _md5(without)
    lines = mon.read_text().strip().split("\n")
    assert lines[0] == "time_s,prn,doppler_hz,cn0_dbhz,peak_ratio,best_delay_halfchips,best_doppler_bins"
    rows = [ln.split(",") for ln in lines[1:]]
    assert sorted({float(x[0]) for x in rows}) == [0.0, 1.0, 2.0] and len(rows) >= 12
    for x in rows:
        assert (x[5], x[6]) == ("0", "0"), x  # the planned delay and Doppler bin are the strongest
