"""galileo-sdr-sim --multipath: the refused files with their messages (they fail before any device work) and, on the MI355X, the file
against a Python mirror of the chain built from the wrappers -- run_mpath with the rows of mpath_rows, then with --oversample 4 --cn0 45
the noise floor and the decimator --, whatever the batch length."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
START = "2022/02/20,12:00:00"
G1 = ["-l", "-6,51,100", "-t", START, "-d", "2", "-U", "1", "-b", "1", "-I", "1", "-P", "0"]  # the golden scenario G1's sky, 19 epochs
EPOCHS = 19
FS = 2.6e6
C_LIGHT = 299792458.0


def _run(args, **kw):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=600, **kw)


def _ok(args):
    r = _run(["-e", NAV] + G1 + args)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _md5(path):
    return hashlib.md5(open(str(path), "rb").read()).hexdigest()


@pytest.fixture(scope="module")
def sky(pkg):
    rows = pkg.Scenario(NAV, llh=(-6, 51, 100), start=START, duration_s=2, iono_enable=False).all()
    assert rows.shape[0] == EPOCHS
    rows.setflags(write=False)
    return rows


def _echo_file(path, sky):
    """Three echoes of the first PRN in view (one of them fading), one of the second, one of a PRN that is not in view."""
    in_view = [int(p) for p in sky["prn"][0] if p > 0]
    absent = next(p for p in range(1, 51) if not (sky["prn"] == p).any())
    spec = [(in_view[0], 250.0, -6.0, 90.0, 0.0), (in_view[0], 1000.0, -10.0, 200.0, 3.5), (in_view[0], 20000.0, -3.0, 0.0, -1.25),
            (in_view[1], 120.0, 0.0, 45.0, 0.0), (absent, 300.0, -3.0, 10.0, 0.0)]
    path.write_text("# prn,delay_m,rel_db,phase_deg[,fade_hz]\n\n" + "".join(
        "%d,%g,%g,%g%s\n" % (s[0], s[1], s[2], s[3], ",%g" % s[4] if s[4] else "") for s in spec))
    return spec


def _mirror_rows(pkg, sky, spec, fs, spe):
    """The CLI's rule: an echo goes to the slot that carries its PRN, with the rows of gal_synth_mpath_row at unity gain."""
    slot_of, cols = [], []
    for prn, delay_m, rel_db, phase, fade in spec:
        where = np.argwhere(sky["prn"] == prn)
        if where.size == 0:
            continue
        slot = int(where[0][1])
        echo = pkg.mpath_make(delay_m / C_LIGHT, rel_db, phase, fade, sample_rate=fs)
        slot_of.append(slot)
        cols.append(pkg.mpath_rows(echo, np.where(sky["prn"][:, slot] == prn, 128, 0), 0, spe))
    return slot_of, np.stack(cols, axis=1)


@pytest.mark.gpu
def test_multipath_file_is_the_mirror_chain_whatever_the_batch(pkg, sky, tmp_path):
    import torch

    spec = _echo_file(tmp_path / "echoes.txt", sky)
    args = ["--multipath", str(tmp_path / "echoes.txt")]
    a, b, plain = (tmp_path / ("%s.ishort" % k) for k in "abp")
    r = _ok(args + ["-o", str(a)])
    _ok(args + ["-B", "7", "-o", str(b)])
    _ok(["-o", str(plain)])
    assert _md5(a) == _md5(b) != _md5(plain)
    lines = [ln for ln in r.stderr.split("\n") if ln.startswith("Multipath ")]
    assert len(lines) == 5 and "delay 2 samples = 230.61 m (asked 250.00 m)" in lines[0] and "delay 173 samples" in lines[2]
    slot_of, rows = _mirror_rows(pkg, sky, spec, FS, 260000)
    assert len(slot_of) == 4 and rows["delay"][0].tolist() == [2, 9, 173, 1]
    with pkg.SynthEngine(sample_rate=FS, samples_per_epoch=260000, n_slots=sky.shape[1], device=0) as eng:
        out = torch.zeros(EPOCHS * 520000, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        eng.run_mpath(sky, np.full(sky.shape, 128), out.data_ptr(), slot_of, rows)
        assert eng.iq_saturated() == 0
        want = out.cpu().numpy()
    assert a.read_bytes() == want.tobytes()


@pytest.mark.gpu
def test_multipath_oversampled_with_noise(pkg, sky, tmp_path):
    """--oversample 4 --cn0 45: the echo pass at 10.4 MS/s (the delays in samples of that rate), in front of the noise floor and the
    decimator; the automatic signal gain leaves room for 1 + the largest per-PRN sum of amplitudes."""
    import torch

    import noise_model

    M = 4
    spec = _echo_file(tmp_path / "echoes.txt", sky)
    args = ["--multipath", str(tmp_path / "echoes.txt"), "--oversample", str(M), "--cn0", "45"]
    a, b = tmp_path / "a.ishort", tmp_path / "b.ishort"
    r = _ok(args + ["-o", str(a)])
    _ok(args + ["-B", "5", "-o", str(b)])
    assert _md5(a) == _md5(b)
    gain = float(re.search(r"signal gain ([0-9.e+-]+) \(chosen\)", r.stderr).group(1))
    unit = noise_model.noise_from_cn0(45.0, M * FS, 1.0)[1] / 16.0
    peak = 1 + 10 ** (-6 / 20) + 10 ** (-10 / 20) + 10 ** (-3 / 20)
    need = 5 * unit + 4100 * peak
    assert need * gain <= 32767 < need * gain * 2
    spe = M * 260000
    slot_of, rows = _mirror_rows(pkg, sky, spec, M * FS, spe)
    assert rows["delay"][0].tolist() == [9, 35, 694, 4]
    taps = pkg.synth.firdec_lowpass(0.45 * FS, M * FS, 32 * M + 1)
    noise = dict(pkg.noise_from_cn0(45.0, M * FS, gain), seed=1)
    with pkg.SynthEngine(sample_rate=M * FS, samples_per_epoch=spe, n_slots=sky.shape[1], device=0) as eng:
        wide = torch.zeros(EPOCHS * spe * 2, dtype=torch.int16, device="cuda")
        kept = torch.zeros(EPOCHS * 520000, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        eng.run_mpath(sky, np.full(sky.shape, 128), wide.data_ptr(), slot_of, rows)
        eng.iq_convert(wide.data_ptr(), EPOCHS * spe, "ishort", out_ptr=wide.data_ptr(), noise=noise, first_sample=0)
        eng.firdec_set(taps, M, 0)
        assert eng.iq_firdec(wide.data_ptr(), EPOCHS * spe, kept.data_ptr()) == EPOCHS * 260000
        eng.iq_saturated()
        want = kept.cpu().numpy()
    assert a.read_bytes() == want.tobytes()


REFUSED = (
    ("7,100,-6\n", "line 1 is not prn,delay_m,rel_db,phase_deg[,fade_hz]"),
    ("# a comment\n\n7,100,-6,90,1,2\n", "line 3 is not prn,delay_m"),
    ("7,100,-6,x\n", "line 1 is not prn,delay_m"),
    ("0,100,-6,90\n", "line 1: PRN outside 1..50"),
    ("51,100,-6,90\n", "line 1: PRN outside 1..50"),
    ("7.5,100,-6,90\n", "line 1: PRN outside 1..50"),
    ("".join("%d,100,-6,90\n" % (1 + k % 50) for k in range(33)), "more than 32 echoes"),
    ("7,100,-6,90\n" * 5, "line 5: more than 4 echoes of PRN 7"),
    ("# nothing\n\n", "it holds no echo"),
    ("7,118500,-6,90\n", "more than 1024"),  # 1027.7 samples at 2.6 MS/s
    ("7,-1,-6,90\n", "must be finite"),
    ("7,100,6.1,90\n", "more than 2 (+6.02 dB)"),
    ("7,100,-6,90,1.3e6\n", "sample_rate / 2"),
)


def test_refused_files_before_any_device_work(tmp_path):
    nav = str(tmp_path / "does_not_exist.rnx")
    f = tmp_path / "echoes.txt"
    r = _run(["-e", nav, "--multipath", str(tmp_path / "missing.txt")])
    assert r.returncode == 1 and "ERROR: --multipath" in r.stderr and "cannot read it" in r.stderr
    for text, message in REFUSED:
        f.write_text(text)
        r = _run(["-e", nav, "--multipath", str(f)])
        assert r.returncode == 1 and "ERROR: --multipath" in r.stderr and message in r.stderr, (text[:40], r.stderr[-500:])
    # admitted: the echoes are printed with their rounded delays, and the run stops at the navigation file
    f.write_text("7,29000,-6,90\n  # indented comment\n11,0,6,725,-2.5\n")
    r = _run(["-e", nav, "--multipath", str(f)])
    assert r.returncode == 1 and "ERROR: --multipath" not in r.stderr
    assert "Multipath 1: PRN 7, delay 252 samples = 29056.81 m (asked 29000.00 m)" in r.stderr
    assert "Multipath 2: PRN 11, delay 0 samples = 0.00 m" in r.stderr and "phase 5.00 deg, fading -2.500 Hz" in r.stderr
    assert "up to 2.995 times" in r.stderr
    # the same delay is 1006 samples at 10.4 MS/s, and 30 km are 1041: the limit is in samples of the rate the pass runs at
    r = _run(["-e", nav, "--multipath", str(f), "--oversample", "4"])
    assert r.returncode == 1 and "delay 1006 samples" in r.stderr and "ERROR: --multipath" not in r.stderr
    f.write_text("7,30000,-6,90\n")
    assert "delay 260 samples" in _run(["-e", nav, "--multipath", str(f)]).stderr
    r = _run(["-e", nav, "--multipath", str(f), "--oversample", "4"])
    assert r.returncode == 1 and "ERROR: --multipath" in r.stderr and "more than 1024" in r.stderr
    assert "--multipath <f>" in _run(["-e"]).stdout
