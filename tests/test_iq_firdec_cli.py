"""galileo-sdr-sim --oversample: the argument checks (they fail before any device work) and, on the MI355X, the file against the Python
mirror of the chain -- engine at 10.4 MS/s, noise and interference models at that rate, the decimator's model (tests/firdec_model.py),
the format --, whatever the batch length; --monitor following the decimator's delay; and the bytes of a run without the option."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import firdec_model
import interf_model
import noise_model
from oracle_binding import oracle_run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "firdec_parent.json")))
START = "2022/02/20,12:00:00"
G1 = ["-l", "-6,51,100", "-t", START, "-d", "1", "-U", "1", "-b", "1", "-I", "1", "-P", "0"]  # the golden scenario G1's sky, 9 epochs
EPOCHS = 9
FS = 2.6e6
M = 4


def _run(args, **kw):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=600, **kw)


def _ok(args):
    r = _run(["-e", NAV] + G1 + args)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _tap_file(path, taps):
    path.write_text("".join("%d\n" % int(t) for t in taps))
    return str(path)


def _md5(path):
    return hashlib.md5(open(str(path), "rb").read()).hexdigest()


def _printed_taps(stderr):
    line = [ln for ln in stderr.split("\n") if ln.startswith("Front-end filter:")]
    assert len(line) == 1, stderr[-2000:]
    return np.array([int(v) for v in line[0].split(":")[-1].split()], dtype=np.int16)


@pytest.fixture(scope="module")
def wide(pkg):
    """The engine's stream of the scenario at 10.4 MS/s, computed once and left unchanged.  It is the oracle's, int16 by int16: the
    mirror chain below rests on the oracle, not on the engine."""
    rows = pkg.Scenario(NAV, llh=(-6, 51, 100), start=START, duration_s=1, iono_enable=False).all()
    assert rows.shape[0] == EPOCHS
    with pkg.SynthEngine(sample_rate=M * FS, samples_per_epoch=M * 260000, n_slots=rows.shape[1], device=0) as eng:
        iq, _, _ = eng.run_host(rows)
    assert iq.size == EPOCHS * M * 520000
    ref, _ = oracle_run(rows, M * 260000, M * FS)
    assert np.array_equal(iq, ref)
    iq.setflags(write=False)
    return iq


@pytest.mark.parametrize("fmt", ("ishort", "ibyte"))
def test_oversampled_file_is_the_mirror_chain_whatever_the_batch(pkg, wide, tmp_path, fmt):
    """--cn0 45 and a tone at 3.0 MHz, which lies outside +-1.3 MHz and can only be asked for with the option."""
    args = ["--oversample", str(M), "--cn0", "45", "--noise-seed", "7", "--jam", "30,3.0e6", "--iq-format", fmt]
    a, b, c, plain = (tmp_path / ("%s.%s" % (k, fmt)) for k in "abcp")
    r = _ok(args + ["-o", str(a)])
    _ok(args + ["-B", "1", "-o", str(b)])
    _ok(args + ["-B", "7", "-o", str(c)])
    assert _md5(a) == _md5(b) == _md5(c)
    _ok(["--iq-format", fmt, "-o", str(plain)])
    assert os.path.getsize(str(a)) == os.path.getsize(str(plain)) == EPOCHS * 260000 * (4 if fmt == "ishort" else 2)
    taps = _printed_taps(r.stderr)
    assert np.array_equal(taps, pkg.synth.firdec_lowpass(0.45 * FS, M * FS, 32 * M + 1))
    gain = float(re.search(r"signal gain ([0-9.e+-]+)", r.stderr).group(1))
    g, s = noise_model.noise_from_cn0(45.0, M * FS, gain)
    src = [interf_model.interf_make(30.0, gain, M * FS, 3.0e6)]
    # the automatic gain: the int16 stream in front of the filter holds 5 sigma + the signals + the tone at the high rate
    unit = noise_model.noise_from_cn0(45.0, M * FS, 1.0)[1] / 16.0
    need = 5 * unit + 4100 + 250 * np.sqrt(2.0) * 10 ** 1.5
    assert need * gain <= 32767 < need * gain * 2 and gain < 1.0
    noisy, sat_n = interf_model.convert(wide, "ishort", 0, (7, 0, g, s), src)
    kept, sat_f = firdec_model.firdec(noisy.view("<i2"), taps, M)
    shift = 0
    if fmt == "ibyte":
        shift = int(re.search(r"Decimator: .*--iq-shift (\d+) \(chosen\)", r.stderr).group(1))
        sigma_out = s / 16.0 * np.sqrt(float((taps.astype(np.float64) ** 2).sum())) / 16384.0
        need = 4 * sigma_out + src[0]["amp_q4"] / 16.0
        assert 127 * (1 << shift) >= need > 127 * (1 << (shift - 1))
    want, _ = noise_model.convert(kept, fmt, shift, (0, 0, 65536, 0))
    assert sat_n == 0 and sat_f == 0
    assert a.read_bytes() == want.tobytes()
    # the tone the front-end rejects: |H(3.0 MHz)| of these taps is below -40 dB
    H = abs(np.sum(taps / 16384.0 * np.exp(-2j * np.pi * 3.0e6 * np.arange(taps.size) / (M * FS))))
    assert H < 0.01


def test_monitor_follows_the_decimators_delay(tmp_path):
    """16384 at index 4 x 12: a pure delay of 12 output samples = 9.4 half chips; without the delay handling no line would name the
    planned delay."""
    delta = np.zeros(2 * M * 12 + 1, dtype=np.int16)
    delta[M * 12] = 16384
    tf = _tap_file(tmp_path / "delay12.txt", delta)
    args = ["--oversample", str(M), "--fir", tf, "--cn0", "45"]
    with_mon, without = tmp_path / "a.ishort", tmp_path / "b.ishort"
    mon = tmp_path / "monitor.csv"
    _ok(args + ["-o", str(with_mon), "--monitor", str(mon), "--monitor-every", "4"])
    _ok(args + ["-o", str(without)])
    assert _md5(with_mon) == _md5(without)
    lines = mon.read_text().strip().split("\n")
    assert lines[0] == "time_s,prn,doppler_hz,cn0_dbhz,peak_ratio,best_delay_halfchips,best_doppler_bins"
    rows = [ln.split(",") for ln in lines[1:]]
    assert sorted({float(x[0]) for x in rows}) == [0.0, 0.4, 0.8] and len(rows) >= 12
    for x in rows:
        assert (x[5], x[6]) == ("0", "0"), x  # the planned delay and Doppler bin are the strongest


def test_refusals_before_any_device_work(tmp_path):
    nav = str(tmp_path / "does_not_exist.rnx")
    for bad in ("1", "16", "0", "abc", "4x", ""):
        r = _run(["-e", nav, "--oversample", bad])
        assert r.returncode == 1 and "--oversample" in r.stderr, bad
    r = _run(["-e", nav, "--oversample", "15"])
    assert r.returncode == 1 and "ERROR: --oversample" not in r.stderr and "481 taps" in r.stderr  # accepted: the default taps are printed
    # --monitor wants a delay of whole output samples
    r = _run(["-e", nav, "--oversample", "4", "--fir-lowpass", "1e6,63", "--monitor", str(tmp_path / "m.csv")])
    assert r.returncode == 1 and "multiple of 8" in r.stderr and "--monitor" in r.stderr
    r = _run(["-e", nav, "--oversample", "4", "--fir-lowpass", "1e6,65", "--monitor", str(tmp_path / "m.csv")])
    assert r.returncode == 1 and "multiple of" not in r.stderr
    # the decimator's taps: up to 512, designed up to 511
    r = _run(["-e", nav, "--oversample", "4", "--fir", _tap_file(tmp_path / "t513.txt", [16384] + [0] * 512)])
    assert r.returncode == 1 and "more than 512 taps" in r.stderr
    r = _run(["-e", nav, "--oversample", "4", "--fir", _tap_file(tmp_path / "t512.txt", [16384] + [0] * 511)])
    assert r.returncode == 1 and "--fir" not in r.stderr
    r = _run(["-e", nav, "--fir", _tap_file(tmp_path / "t129.txt", [16384] + [0] * 128)])
    assert r.returncode == 1 and "more than 128 taps" in r.stderr  # without the option: as before
    r = _run(["-e", nav, "--oversample", "4", "--fir-lowpass", "1e6,511"])
    assert r.returncode == 1 and "ERROR: --fir" not in r.stderr and "511 taps" in r.stderr
    r = _run(["-e", nav, "--fir-lowpass", "1e6,129"])
    assert r.returncode == 1 and "--fir-lowpass" in r.stderr
    # a tone at 1.4 MHz: refused without the option, as before; admitted with it
    r = _run(["-e", nav, "--jam", "20,1.4e6"])
    assert r.returncode == 1 and "--jam" in r.stderr
    r = _run(["-e", nav, "--oversample", "2", "--jam", "20,1.4e6"])
    assert r.returncode == 1 and "--jam" not in r.stderr
    h = _run(["-e"])
    assert "--oversample <M>" in h.stdout


def test_without_oversample_the_parents_bytes(tmp_path):
    """test_iq_fir_cli.py's `--fir-lowpass 1e6,25 -B 11` over 29 epochs: the md5 the parent commit's binary wrote."""
    out = tmp_path / "c.ishort"
    args = list(G1)
    args[args.index("-d") + 1] = "3"
    r = _run(["-e", NAV] + args + ["--fir-lowpass", "1e6,25", "-B", "11", "-o", str(out)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Oversampling" not in r.stderr and "Decimator" not in r.stderr
    assert _md5(out) == GOLD["fir_lowpass_1e6_25_B11_d3_ishort_md5"]
