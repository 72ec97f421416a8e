"""The CLI's --cn0 on the MI355X: every format against the numpy model (tests/noise_model.py) applied to the same command's
noiseless ishort file -- the model knows nothing of batches, so a run longer than one batch shows that the file does not depend on
the batch cut --, --sites with one noise stream per site, and the bytes of a run without --cn0."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import noise_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "iq_format_md5.json")))
G1 = ["-l", "-6,51,100", "-t", "2022/02/20,12:00:00", "-d", "10", "-U", "1", "-b", "1", "-I", "1", "-P", "0"]
NOISE = ["--cn0", "45", "--noise-seed", "7"]
G45, S45 = noise_model.noise_from_cn0(45.0, 2.6e6, 1.0)  # the CLI chooses gain 1 at 45 dB-Hz: 5 x 2267 + 4100 <= 32767


def _run(args):
    r = subprocess.run([CLI, "-e", NAV] + args, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r


def _with_duration(d):
    a = list(G1)
    a[a.index("-d") + 1] = str(d)
    return a


def test_without_cn0_the_pinned_bytes(tmp_path):
    out = tmp_path / "g1.ishort"
    r = _run(G1 + ["-o", str(out)])
    assert hashlib.md5(out.read_bytes()).hexdigest() == GOLD["G1"]["ishort"]["md5"]
    assert b"Noise floor" not in r.stderr


def test_ishort_longer_than_one_batch(tmp_path):
    """139 epochs: the CLI's batches are 128 epochs, the second one starts at sample 128 x 260 000."""
    base = _with_duration(14)
    clean, noisy = tmp_path / "clean.ishort", tmp_path / "noisy.ishort"
    _run(base + ["-o", str(clean)])
    r = _run(base + NOISE + ["-o", str(noisy)])
    assert b"signal gain 1 (chosen)" in r.stderr and b"seed 7, stream 0" in r.stderr
    x = np.fromfile(str(clean), dtype="<i2")
    assert x.size == 139 * 520000
    want, sat = noise_model.convert(x, "ishort", 0, (7, 0, G45, S45))
    assert sat == 0 and (b"saturated" not in r.stderr)
    got = np.fromfile(str(noisy), dtype=np.uint8)
    assert got.size == want.size and np.array_equal(got, want)
    # other batch lengths, the same file: the first 30 epochs in batches of 7
    short = tmp_path / "short.ishort"
    _run(_with_duration(3.1) + NOISE + ["-B", "7", "-o", str(short)])
    assert short.read_bytes() == want[: 30 * 1040000].tobytes()


@pytest.mark.parametrize("fmt,extra,shift", [("ibyte", [], 7), ("ibyte", ["--iq-shift", "5"], 5), ("ibit", [], 0)])
def test_ibyte_and_ibit(tmp_path, fmt, extra, shift):
    base = _with_duration(3)
    clean, noisy = tmp_path / "clean.ishort", tmp_path / ("noisy." + fmt)
    _run(base + ["-o", str(clean)])
    r = _run(base + NOISE + ["--iq-format", fmt, "-B", "7", "-o", str(noisy)] + extra)
    x = np.fromfile(str(clean), dtype="<i2")
    assert x.size == 29 * 520000
    want, sat = noise_model.convert(x, fmt, shift, (7, 0, G45, S45))
    assert noisy.read_bytes() == want.tobytes()
    if fmt == "ibyte":
        assert (b"--iq-shift %d" % shift) in r.stderr
        assert ((b"%d of" % sat) in r.stderr) == (sat > 0)
    if shift == 5:
        assert sat > 0  # 127 x 32 = 1.8 sigma


def test_sites_take_one_noise_stream_each(tmp_path):
    lst = tmp_path / "sites.txt"
    lst.write_text("-6,51,100\n-6,51,100\n")
    common = ["-t", "2022/02/20,12:00:00", "-d", "2", "-I", "1"]
    sites = ["--sites", str(lst), "--gpus", "1", "--per-gpu", "2"]
    _run(common + ["-l", "-6,51,100", "-P", "0", "-o", str(tmp_path / "clean.ishort")])
    _run(common + sites + NOISE + ["-o", str(tmp_path / "a.ishort")])
    x = np.fromfile(str(tmp_path / "clean.ishort"), dtype="<i2")
    assert x.size == 19 * 520000
    files = [(tmp_path / ("a.site%d.ishort" % k)).read_bytes() for k in range(2)]
    assert files[0] != files[1]
    for k in range(2):
        assert files[k] == noise_model.convert(x, "ishort", 0, (7, k, G45, S45))[0].tobytes(), k
