"""galileo-sdr-sim --reflector on a 2 s sky: the refusals with their messages (before any device work), and, on the MI355X, the file
against the wrappers fed with the rows of --reflector-log, whatever the batch length; a ground plane without excess path; the
oversampled chain; the stop at more than 32 echoes; and --monitor's strongest delay against the echo the log describes."""
import hashlib
import math
import os
import subprocess

import numpy as np
import pytest

import refl_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
START = "2022/02/20,12:00:00"
G1 = ["-l", "-6,51,100", "-t", START, "-d", "2", "-U", "1", "-b", "1", "-I", "1", "-P", "0"]  # the golden scenario G1's sky, 19 epochs
EPOCHS = 19
FS = 2.6e6
HALF_CHIP_M = 299792458.0 / (2 * 1.023e6)


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
    active = rows["prn"] > 0
    assert (active == active[0]).all() and (rows["prn"] == rows["prn"][0]).all()  # one set of satellites, each in its slot throughout
    rows.setflags(write=False)
    return rows


def _log(path):
    """The lines of --reflector-log: time_s, prn, reflector, excess_m, D, F, ph0, gain_q7, dph."""
    out = []
    for ln in open(str(path)).read().strip().split("\n"):
        x = ln.split(",")
        assert len(x) == 9, ln
        out.append((float(x[0]), int(x[1]), int(x[2]), float(x[3])) + tuple(int(v) for v in x[4:]))
    return out


def _mirror(pkg, sky, log, n_refl, spe):
    """The CLI's rule: a column per (slot with a satellite, reflector), its rows those of the log."""
    slots = [s for s in range(sky.shape[1]) if sky["prn"][0, s] > 0]
    slot_of = [s for s in slots for _ in range(n_refl)]
    rows = refl_model.rows(EPOCHS, len(slot_of))
    seen = 0
    for t, prn, k, _, D, F, ph0, gain, dph in log:
        e = int(round(t * 10))
        j = slots.index(int(np.flatnonzero(sky["prn"][e] == prn)[0])) * n_refl + k
        rows[e, j] = (gain, D, ph0, dph, F, 0)
        seen += 1
    assert seen == EPOCHS * len(slot_of)
    return slot_of, rows


def _synth(pkg, sky, slot_of, rows, rate, spe):
    import torch

    with pkg.SynthEngine(sample_rate=rate, samples_per_epoch=spe, n_slots=sky.shape[1], device=0) as eng:
        out = torch.zeros(EPOCHS * spe * 2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        eng.run_refl(sky, np.full(sky.shape, 128), out.data_ptr(), slot_of, rows)
        assert eng.iq_saturated() == 0
        return out.cpu().numpy()


@pytest.mark.gpu
def test_ground_plane_without_excess_path(pkg, sky, tmp_path):
    """--reflector ground,0,-6: no excess path, so D = F = 0 and the echo is the satellite's own sample at half the amplitude, turned by
    the reflection's 180 degrees: the file differs from the plain run exactly as gal_synth_run_refl with those rows says."""
    a, plain, log = tmp_path / "a.ishort", tmp_path / "p.ishort", tmp_path / "r.csv"
    r = _ok(["--reflector", "ground,0,-6", "--reflector-log", str(log), "-o", str(a)])
    assert "Reflector 0: ground, antenna height 0.000 m, amplitude 0.5012 (-6.00 dB), reflection phase 180.00 deg" in r.stderr
    _ok(["-o", str(plain)])
    assert _md5(a) != _md5(plain)
    lines = _log(log)
    n_sat = int((sky["prn"][0] > 0).sum())
    assert len(lines) == EPOCHS * n_sat
    assert all(x[2:] == (0, 0.0, 0, 0, 1 << 31, 64, 0) for x in lines)
    slot_of, rows = _mirror(pkg, sky, lines, 1, 260000)
    want = _synth(pkg, sky, slot_of, rows, FS, 260000)
    assert a.read_bytes() == want.tobytes()
    # and as arithmetic on the plain file: w = 128 x + 64 (-x) per satellite, so y is (64 sum + 64) >> 7 of the satellites' streams;
    # the plain file is their sum itself, and halving it can differ from that only by the rounding of the single echoes' r
    x = np.frombuffer(plain.read_bytes(), dtype="<i2").astype(np.int64)
    assert np.abs(want.astype(np.int64) - ((64 * x + 64) >> 7)).max() <= 1


@pytest.mark.gpu
def test_file_is_the_wrappers_fed_with_the_log_whatever_the_batch(pkg, sky, tmp_path):
    """A ground bounce under a 2 m mast and a wall at 100 m towards the east: the file of three batch lengths is one file, the log is
    one log, and the file is gal_synth_run_refl over the front-end's rows with the rows the log states.  The log's rows are those of
    the geometry: gal_synth_refl_row of consecutive excess paths."""
    args = ["--reflector", "ground,2,-6", "--reflector", "wall,100,90,-3,170"]
    files = [tmp_path / ("%s.ishort" % k) for k in "abc"]
    logs = [tmp_path / ("%s.csv" % k) for k in "abc"]
    for f, lg, batch in zip(files, logs, ([], ["-B", "7"], ["-B", "1"])):
        _ok(args + batch + ["-o", str(f), "--reflector-log", str(lg)])
    assert _md5(files[0]) == _md5(files[1]) == _md5(files[2])
    assert logs[0].read_bytes() == logs[1].read_bytes() == logs[2].read_bytes()
    lines = _log(logs[0])
    slot_of, rows = _mirror(pkg, sky, lines, 2, 260000)
    assert a_wall_echo_and_a_shadow(lines)
    want = _synth(pkg, sky, slot_of, rows, FS, 260000)
    assert files[0].read_bytes() == want.tobytes()
    # the rows are gal_synth_refl_row of the logged excess paths: this epoch's and the next one's (the last epoch: none behind it)
    by_key = {(x[0], x[1], x[2]): x for x in lines}
    spec = {0: (-6.0, 180.0), 1: (-3.0, 170.0)}
    for (t, prn, k), x in by_key.items():
        nxt = by_key.get((round(t + 0.1, 1), prn, k))
        A, D, ph0, dph, F, _ = refl_model.row(x[3], nxt[3] if nxt else -1.0, spec[k][0], spec[k][1], FS, 260000, 128)
        assert (x[7], x[4], x[5]) == (A, D, F), (t, prn, k)
        if x[7]:
            # the log prints the excess path to 1e-9 m: half a unit of that is 11.3 units of 2^-32 cycle, plus the rounding of ph0
            tol = 0.5e-9 / refl_model.LAMBDA * 4294967296.0 + 1
            assert abs((x[6] - ph0 + (1 << 31)) % (1 << 32) - (1 << 31)) <= tol and abs(x[8] - dph) <= 1, (t, prn, k, x, ph0, dph)
    assert any(x[8] != 0 for x in lines)  # the phase turns as the satellites move


def a_wall_echo_and_a_shadow(lines):
    """The wall is at 100 m: satellites in the west see an echo up to 200 m late, those in the east none (excess -1, gain 0)."""
    wall = [x for x in lines if x[2] == 1]
    lit, dark = [x for x in wall if x[3] > 0], [x for x in wall if x[3] < 0]
    return lit and dark and all(x[7] == 0 for x in dark) and all(0 < x[3] <= 200.0 and x[7] == 91 for x in lit)


@pytest.mark.gpu
def test_oversampled_with_noise_and_the_headroom(pkg, sky, tmp_path):
    """--oversample 4 --cn0 45: the pass runs at 10.4 MS/s (the log's delays are in samples of that rate), in front of the noise floor
    and the decimator, as --multipath does; the file does not depend on -B; the automatic signal gain leaves room for 1 + the sum
    of the reflectors' amplitudes."""
    import re

    import noise_model

    M = 4
    args = ["--reflector", "ground,2,-6", "--reflector", "wall,100,90,-3", "--oversample", str(M), "--cn0", "45"]
    a, b, log = tmp_path / "a.ishort", tmp_path / "b.ishort", tmp_path / "r.csv"
    r = _ok(args + ["-o", str(a), "--reflector-log", str(log)])
    _ok(args + ["-B", "5", "-o", str(b)])
    assert _md5(a) == _md5(b)
    gain = float(re.search(r"signal gain ([0-9.e+-]+) \(chosen\)", r.stderr).group(1))
    unit = noise_model.noise_from_cn0(45.0, M * FS, 1.0)[1] / 16.0
    need = 5 * unit + 4100 * (1 + 10 ** (-6 / 20) + 10 ** (-3 / 20))
    assert need * gain <= 32767 < need * gain * 2
    for x in _log(log):
        if x[3] >= 0:
            t = x[3] / 299792458.0 * M * FS
            assert abs(x[4] + x[5] / 4096.0 - t) <= 0.5 / 4096 + 1e-9


@pytest.mark.gpu
def test_more_than_32_echoes_stop_the_run_and_a_prn_list_admits_it(pkg, sky, tmp_path):
    n_sat = int((sky["prn"][0] > 0).sum())
    assert 4 * n_sat > 32
    four = [v for k in range(4) for v in ("--reflector", "ground,%d,-12" % (k + 1))]
    r = _run(["-e", NAV] + G1 + four + ["-o", str(tmp_path / "x.ishort")])
    assert r.returncode != 0
    assert "--reflector: 4 reflectors x %d satellites = %d echoes in epoch 0 (0.0 s), more than 32" % (n_sat, 4 * n_sat) in r.stderr
    prns = [int(p) for p in sky["prn"][0] if p > 0][:3]
    log = tmp_path / "r.csv"
    _ok(four + ["--reflector-prn", ",".join(str(p) for p in prns), "--reflector-log", str(log), "-o", str(tmp_path / "y.ishort")])
    assert sorted({x[1] for x in _log(log)}) == sorted(prns)


def _boc_r(lag):
    """The autocorrelation of a BOC(1,1) code over the lag in half chips: 1 at 0, -1/2 at +-1, 0 from +-2 on, linear between."""
    lag = abs(lag)
    return 1.0 - 1.5 * lag if lag <= 1 else (-0.5 + 0.5 * (lag - 1) if lag <= 2 else 0.0)


@pytest.mark.gpu
def test_monitor_strongest_delay_follows_the_echo(pkg, sky, tmp_path):
    """A wall at 100 m, -3 dB, no noise.  For every monitored (epoch, satellite) the log gives the echo's delay, amplitude and phase;
    the power at the monitor's delays k = -1, 0, +1 half chips is then |R(k) + a e^{j theta} R(k - delay)|^2 with R the BOC(1,1)
    autocorrelation.  Wherever that prediction is clear (the best beats the second by 20 %), the monitor's strongest-delay column
    names it -- also where the echo moves it off the planned delay; satellites in the wall's shadow keep the plain run's strongest cell.  (At -3 dB and at most 1.4 half chips
    of delay the direct peak stays the strongest whatever the phase -- 1.35 against 1.21 at worst --, which is what the prediction
    says and the column shows: the test prints how many predictions were clear and how many moved.)"""
    a, mon, log, mon0 = tmp_path / "a.ishort", tmp_path / "m.csv", tmp_path / "r.csv", tmp_path / "m0.csv"
    _ok(["--reflector", "wall,100,90,-3,0", "--reflector-log", str(log), "--monitor", str(mon), "--monitor-every", "1", "-o", str(a)])
    _ok(["--monitor", str(mon0), "--monitor-every", "1", "-o", str(tmp_path / "p.ishort")])
    rows = {(round(float(x[0]), 1), int(x[1])): x for x in (ln.split(",") for ln in open(str(mon)).read().strip().split("\n")[1:])}
    plain = {(round(float(x[0]), 1), int(x[1])): x for x in (ln.split(",") for ln in open(str(mon0)).read().strip().split("\n")[1:])}
    clear = moved = shadow = 0
    for t, prn, _, excess, D, F, ph0, gain, _ in _log(log):
        got = rows[(t, prn)]
        if gain == 0:
            assert got[5:] == plain[(t, prn)][5:]  # (its C/N0 feels the others' echoes as multiple-access noise)
            shadow += 1
            continue
        assert got[3:5] != plain[(t, prn)][3:5]  # C/N0 and peak ratio see the echo
        z = gain / 128.0 * np.exp(2j * math.pi * ph0 / 4294967296.0)
        lag = (D + F / 4096.0) / FS * 299792458.0 / HALF_CHIP_M
        power = [abs(_boc_r(k) + z * _boc_r(k - lag)) ** 2 for k in (-1, 0, 1)]
        order = np.argsort(power)
        if power[order[2]] < 1.2 * power[order[1]]:
            continue
        clear += 1
        assert int(got[5]) == int(order[2]) - 1, (t, prn, power, got)
        moved += int(got[5]) != 0
    assert shadow > 0 and clear > 0.5 * (len(rows) - shadow)
    print("monitor: %d clear predictions, %d of them off the planned delay, %d lines in the wall's shadow" % (clear, moved, shadow))


REFUSED = (
    (["--reflector", "ground,2,-6", "--multipath", "echoes.txt"], "--reflector does not go with --multipath"),
    (["--reflector", "ground,2,-6", "--scint", "scint.txt"], "--reflector does not go with --scint"),
    (["--reflector", "ground,2,-6", "--array", "array.txt"], "--reflector does not go with --array"),
    (["--reflector", "ground,2"], "is not ground,h_m,rel_db[,phase_deg]"),
    (["--reflector", "ground,2,-6,180,1"], "is not ground,h_m,rel_db[,phase_deg]"),
    (["--reflector", "wall,20,90"], "is not wall,dist_m,az_deg,rel_db[,phase_deg]"),
    (["--reflector", "wall,20,x,-6"], "is not wall,dist_m,az_deg,rel_db[,phase_deg]"),
    (["--reflector", "roof,2,-6"], "is neither ground,h_m,rel_db[,phase_deg] nor wall,dist_m,az_deg,rel_db[,phase_deg]"),
    (["--reflector", "ground,-1,-6"], "height or distance -1 m >= 0"),
    (["--reflector", "wall,nan,90,-6"], "must be finite"),
    (["--reflector", "ground,2,6.1"], "more than 2 (+6.02 dB)"),
    (["--reflector", "ground,2,-6"] * 5, "--reflector may be given 4 times at most"),
    (["--reflector-prn", "3"], "--reflector-prn and --reflector-log need --reflector"),
    (["--reflector-log", "r.csv"], "--reflector-prn and --reflector-log need --reflector"),
    (["--reflector", "ground,2,-6", "--reflector-prn", "0"], "is not prn[,prn...] (PRN 1..50)"),
    (["--reflector", "ground,2,-6", "--reflector-prn", "3,51"], "is not prn[,prn...] (PRN 1..50)"),
    (["--reflector", "ground,2,-6", "--reflector-prn", "3;4"], "is not prn[,prn...] (PRN 1..50)"),
    (["--reflector", "ground,2,-6", "--reflector-log", "-"], "--reflector-log needs a file name"),
)


def test_refusals_before_any_file_is_opened(tmp_path):
    """Every refusal with its message.  The files the other options name do not exist, and neither does the navigation file: the
    message is the reflector's, so nothing was opened before it."""
    nav = str(tmp_path / "does_not_exist.rnx")
    for args, message in REFUSED:
        r = _run(["-e", nav] + args, cwd=str(tmp_path))
        assert r.returncode == 1 and "ERROR: --reflector" in r.stderr and message in r.stderr, (args, r.stderr[-500:])
        assert "cannot read" not in r.stderr and not os.listdir(str(tmp_path))
    # admitted: the reflectors are printed, and the run stops at the navigation file
    r = _run(["-e", nav, "--reflector", "ground,2,-6", "--reflector", "wall,20,135,-3,170", "--reflector-prn", "3,11"], cwd=str(tmp_path))
    assert r.returncode == 1 and "ERROR: --reflector" not in r.stderr
    assert "Reflector 1: wall at 20.000 m towards azimuth 135.00 deg, amplitude 0.7079 (-3.00 dB), reflection phase 170.00 deg" in r.stderr
    assert "Reflectors: 2; a satellite reaches up to 2.209 times its own amplitude" in r.stderr
