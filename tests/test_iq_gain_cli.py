"""The CLI's --power-model / --antenna / --prn-power on the MI355X: the written file against the same scenario composed through the
Python mirror -- the front-end's gains through SynthEngine.run_gains --, and the bytes of the command line without the options."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
REF = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_md5.json")))
G1 = ["-l", "-6,51,100", "-t", "2022/02/20,12:00:00", "-d", "10", "-U", "1", "-b", "1", "-I", "1", "-P", "0"]
# a pattern of the test's own: 0.4 dB more per 5 degrees off the zenith
PATTERN = [0.4 * k for k in range(37)]
# G1's sky is PRN 5, 9, 10, 11, 12, 14, 24, 31, 36: some up, some down, some left alone
OFFSETS = {5: -6.0, 9: 3.5, 10: -12.25, 12: 1.0, 24: 7.0, 36: -0.5}


def _run(args):
    r = subprocess.run([CLI, "-e", NAV] + args, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r


def _two_seconds():
    a = list(G1)
    a[a.index("-d") + 1] = "2"
    return a


def test_power_options_against_the_python_mirror(pkg, tmp_path):
    import torch

    ant = tmp_path / "antenna.txt"
    ant.write_text("\n".join("%.1f" % v for v in PATTERN) + "\n")
    out = tmp_path / "power.ishort"
    spec = ",".join("%d:%g" % kv for kv in OFFSETS.items())
    r = _run(_two_seconds() + ["--power-model", "--antenna", str(ant), "--prn-power", spec, "-B", "7", "-o", str(out)])
    assert b"Signal power per PRN" in r.stderr and b"PRN  5: gain" in r.stderr

    sc = pkg.Scenario(NAV, llh=(-6.0, 51.0, 100.0), start="2022/02/20,12:00:00", duration_s=2.0, iono_enable=False)
    sc.set_power(PATTERN, OFFSETS, path_loss=True)
    rows, gains = sc.next_gains(sc.total_epochs)
    assert rows.shape[0] == 19
    active = rows["prn"] > 0
    assert len(np.unique(gains[active])) > 6 and gains[active].max() > 128 > gains[active].min() > 0
    with pkg.SynthEngine(samples_per_epoch=260000, n_slots=16, device=0) as eng:
        dev = torch.zeros(19 * 520000, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        eng.run_gains(rows, gains, dev.data_ptr())
        sat = eng.iq_saturated()
        want = dev.cpu().numpy()
        plain, _, _ = eng.run_host(rows)
    assert sat == 0 and b"saturated" not in r.stderr
    got = np.fromfile(str(out), dtype="<i2")
    assert got.size == want.size
    assert hashlib.md5(got.tobytes()).hexdigest() == hashlib.md5(want.tobytes()).hexdigest()
    assert np.count_nonzero(want != plain) > 0.5 * want.size

    # without the three options: the plain bytes, and those of the reference
    short, long_ = tmp_path / "plain2.ishort", tmp_path / "g1.ishort"
    r = _run(_two_seconds() + ["-B", "7", "-o", str(short)])
    assert b"Signal power" not in r.stderr
    assert short.read_bytes() == plain.tobytes()
    _run(G1 + ["-o", str(long_)])
    data = long_.read_bytes()
    assert hashlib.md5(data).hexdigest() == REF["G1"]["md5"]
    assert data[:plain.nbytes] == plain.tobytes()
