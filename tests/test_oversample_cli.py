"""galileo-sdr-sim --oversample M with a decimator of the single tap 16384 -- an exact pick of every M-th sample
(tests/test_iq_firdec_cpu.py) -- and nothing else in the chain: the file is the oracle's stream at M x 2.6 MS/s picked at that phase,
byte for byte, at the default batch length and with a plan per epoch (the channel state carried from batch to batch)."""
import os
import subprocess

import numpy as np
import pytest

from oracle_binding import oracle_run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
START = "2022/02/20,12:00:00"
G1 = ["-l", "-6,51,100", "-t", START, "-d", "0.3", "-U", "1", "-b", "1", "-I", "1", "-P", "0"]  # the golden scenario G1's sky
FS, N = 2.6e6, 260000


@pytest.fixture(scope="module")
def sky(pkg):
    rows = pkg.Scenario(NAV, llh=(-6, 51, 100), start=START, duration_s=0.3, iono_enable=False).all()
    assert rows.shape[0] >= 2 and int((rows["prn"][0] > 0).sum()) >= 8  # more than one epoch: -B 1 carries the state
    rows.setflags(write=False)
    return rows


@pytest.mark.parametrize("M", [2, 6, 15])
def test_oversampled_file_is_the_oracles_stream_picked(pkg, sky, tmp_path, M):
    tap = tmp_path / "one_tap.txt"
    tap.write_text("16384\n")
    files = []
    for name, batch in (("default", []), ("b1", ["-B", "1"])):
        out = tmp_path / (name + ".ishort")
        r = subprocess.run([CLI, "-e", NAV] + G1 + ["--oversample", str(M), "--fir", str(tap), "-o", str(out)] + batch,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        files.append(np.fromfile(str(out), dtype="<i2"))
    ref, _ = oracle_run(sky, M * N, M * FS)
    want = ref.reshape(-1, 2)[::M].reshape(-1)  # the stream starts at sample 0: the kept phase is 0
    assert want.size == sky.shape[0] * N * 2
    for got, name in zip(files, ("default -B", "-B 1")):
        assert got.size == want.size, (name, got.size, want.size)
        nbad = int(np.count_nonzero(got != want))
        assert nbad == 0, "%s: %d of %d int16 values differ (first at %d)" % (name, nbad, got.size, int(np.flatnonzero(got != want)[0]))
    assert np.array_equal(files[0], files[1])
