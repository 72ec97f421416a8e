"""The CLI's --jam on the MI355X: the written file against the numpy model (tests/interf_model.py) applied to the same command's plain
ishort file with the gain the CLI printed -- with and without --cn0, in ibyte, and for two batch lengths --, the option checks
that stop a run before any device work, and the bytes of a run without --jam."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import interf_model
import noise_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "iq_format_md5.json")))
G1 = ["-l", "-6,51,100", "-t", "2022/02/20,12:00:00", "-d", "10", "-U", "1", "-b", "1", "-I", "1", "-P", "0"]
FS = 2.6e6
# a CW tone at J/S 28 dB, a chirp over 2 MHz every 100 us at 25 dB, pulsed 200 us of every 1000
JAM = ["--jam", "28,1e5", "--jam", "25,-1e6,1e6,100,1000,200"]
JAM_ARGS = ((28.0, 1e5), (25.0, -1e6, 1e6, 100e-6, 1000e-6, 200e-6))


def _run(args, ok=True):
    r = subprocess.run([CLI, "-e", NAV] + args, capture_output=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr.decode(errors="replace")[-2000:]
    return r


def _with_duration(d):
    a = list(G1)
    a[a.index("-d") + 1] = str(d)
    return a


def _printed_gain(stderr):
    m = re.search(rb"signal gain ([0-9.e+-]+)", stderr)
    assert m, stderr[-2000:]
    return float(m.group(1))


@pytest.fixture(scope="module")
def clean(tmp_path_factory):
    """The plain run, 29 epochs: shared by the tests below and left unchanged."""
    out = tmp_path_factory.mktemp("jam") / "clean.ishort"
    _run(_with_duration(3) + ["-o", str(out)])
    x = np.fromfile(str(out), dtype="<i2")
    assert x.size == 29 * 520000
    x.setflags(write=False)
    return x


def test_jam_alone_and_two_batch_lengths(tmp_path, clean):
    a, b = tmp_path / "a.ishort", tmp_path / "b.ishort"
    r = _run(_with_duration(3) + JAM + ["-o", str(a)])
    gain = _printed_gain(r.stderr)
    assert gain == 1.0 and b"Noise floor" not in r.stderr  # 4100 + 8881 + 6287 <= 32 767
    assert b"Interference 1: J/S 28 dB" in r.stderr and b"Interference 2: J/S 25 dB" in r.stderr
    src = [interf_model.interf_make(js, gain, FS, *rest) for js, *rest in JAM_ARGS]
    want, sat = interf_model.convert(clean, "ishort", 0, None, src)
    assert sat == 0 and a.read_bytes() == want.tobytes()
    assert np.count_nonzero(want.view(np.int16) != clean) > 0.9 * clean.size
    _run(_with_duration(3) + JAM + ["-B", "7", "-o", str(b)])
    assert b.read_bytes() == a.read_bytes()


def test_jam_at_a_given_gain(tmp_path, clean):
    """--signal-gain without --cn0: the signals are scaled in the same pass, nothing random is added."""
    out = tmp_path / "half.ishort"
    r = _run(_with_duration(3) + JAM + ["--signal-gain", "0.5", "-B", "11", "-o", str(out)])
    assert _printed_gain(r.stderr) == 0.5
    src = [interf_model.interf_make(js, 0.5, FS, *rest) for js, *rest in JAM_ARGS]
    want, _ = interf_model.convert(clean, "ishort", 0, (0, 0, 32768, 0), src)
    assert out.read_bytes() == want.tobytes()


@pytest.mark.parametrize("fmt", ("ishort", "ibyte"))
def test_jam_with_cn0(tmp_path, clean, fmt):
    out = tmp_path / ("noisy." + fmt)
    r = _run(_with_duration(3) + JAM + ["--cn0", "45", "--noise-seed", "7", "--iq-format", fmt, "-B", "7", "-o", str(out)])
    gain = _printed_gain(r.stderr)
    assert gain == 1.0  # 5 x 2267 + 4100 + 8881 + 6287 = 30 603 <= 32 767
    g, s = noise_model.noise_from_cn0(45.0, FS, gain)
    src = [interf_model.interf_make(js, gain, FS, *rest) for js, *rest in JAM_ARGS]
    shift = 0
    if fmt == "ibyte":
        m = re.search(rb"--iq-shift (\d+) \(chosen\)", r.stderr)
        shift = int(m.group(1))
        need = 4 * s / 16.0 + sum(c["amp_q4"] for c in src) / 16.0
        assert 127 * (1 << shift) >= need > 127 * (1 << (shift - 1))
    want, sat = interf_model.convert(clean, fmt, shift, (7, 0, g, s), src)
    assert out.read_bytes() == want.tobytes()
    if sat > 0:
        assert (b"WARNING: %d of" % sat) in r.stderr
    else:
        assert b"saturated" not in r.stderr


def test_bad_jam_stops_before_device_work(tmp_path):
    out = tmp_path / "x.ishort"
    for extra in (["--jam", "20"], ["--jam", "20,2e6"], ["--jam", "20,1e5,2e5"], ["--jam", "1,1"] * 5):
        r = _run(_with_duration(1) + extra + ["-o", str(out)], ok=False)
        assert r.returncode == 1 and b"--jam" in r.stderr
        assert not out.exists()


def test_without_jam_the_pinned_bytes(tmp_path):
    out = tmp_path / "g1.ishort"
    r = _run(G1 + ["-o", str(out)])
    assert hashlib.md5(out.read_bytes()).hexdigest() == GOLD["G1"]["ishort"]["md5"]
    assert b"Interference" not in r.stderr
