"""galileo-sdr-sim --array: the refused combinations and files with their messages (before any device work) and, on the MI355X, the
element files -- the plain run's bytes for elements at the reference point, one satellite's rotation against the model with the
indices of --array-log and against the geometry, the full sky with --power-model and --scint against the composed model of every
element, independent noise per element, the same bytes for two batch lengths, and a jammer's direction of arrival."""
import hashlib
import math
import os
import subprocess

import numpy as np
import pytest

import array_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
START = "2022/02/20,12:00:00"
G1 = ["-l", "-6,51,100", "-t", START, "-d", "2", "-U", "1", "-b", "1", "-I", "1", "-P", "0"]  # the golden scenario G1's sky, 19 epochs
EPOCHS, N = 19, 260000
FS = 2.6e6
EAST = 0.095  # metres: half a wavelength, all but 0.2 mm
TWO = "0,0,0\n%g,0,0   # east of the reference point\n" % EAST


def _run(args, **kw):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=600, **kw)


def _ok(args):
    r = _run(["-e", NAV] + G1 + args)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _md5(path):
    return hashlib.md5(open(str(path), "rb").read()).hexdigest()


def _iq(path):
    return np.fromfile(str(path), dtype=np.int16)


@pytest.fixture(scope="module")
def sky(pkg):
    rows = pkg.Scenario(NAV, llh=(-6, 51, 100), start=START, duration_s=2, iono_enable=False).all()
    assert rows.shape[0] == EPOCHS
    rows.setflags(write=False)
    return rows


def _only(sky, keep):
    """--prn-power that leaves `keep` (None: nobody) at unity and takes every other PRN that is ever in view to -60 dB: Q7 gain 0."""
    prns = sorted({int(p) for p in sky["prn"].ravel() if p > 0 and p != keep})
    return ["--prn-power", ",".join("%d:-60" % p for p in prns)]


def test_refused_combinations_and_files_before_any_device_work(tmp_path):
    arr = tmp_path / "a.txt"
    arr.write_text(TWO)
    other = tmp_path / "other.txt"
    other.write_text("5,100,-6,0\n")
    out = tmp_path / "x.ishort"
    base = ["-e", NAV] + G1 + ["-o", str(out), "--array", str(arr)]
    for extra, want in ((["--multipath", str(other)], "--array does not go with --multipath"),
                        (["--lo-offset", "100"], "--array does not go with --lo-offset / --phase-noise"),
                        (["--phase-noise", "1e-20"], "--array does not go with --lo-offset / --phase-noise"),
                        (["--fir", str(other)], "--array does not go with --fir / --fir-lowpass"),
                        (["--fir-lowpass", "1e6"], "--array does not go with --fir / --fir-lowpass"),
                        (["--oversample", "2"], "--array does not go with --oversample"),
                        (["--agc"], "--array does not go with --agc"),
                        (["--iq-format", "i2bit"], "--array does not go with --iq-format i2bit"),
                        (["--monitor", str(tmp_path / "m.csv")], "--array does not go with --monitor"),
                        (["--sites", str(other)], "--array does not go with --sites"),
                        (["--jam-dir", "90,0"], "--jam-dir may be given once per --jam"),
                        (["--jam", "30,1e5", "--jam-dir", "90"], "is not az_deg,el_deg"),
                        (["--jam", "30,1e5", "--jam-dir", "90,91"], "is not az_deg,el_deg"),
                        (["--array-log", "-"], "--array-log needs a file name")):
        r = _run(base + extra)
        assert r.returncode == 1 and want in r.stderr and "ERROR: " in r.stderr, (extra, r.stderr[-500:])
    r = _run(["-e", NAV] + G1 + ["-o", "-", "--array", str(arr)])
    assert r.returncode == 1 and "one file per element" in r.stderr
    for extra, want in ((["--array-log", str(tmp_path / "l.csv")], "--array-log needs --array"), (["--jam", "30,1e5", "--jam-dir", "90,0"], "--jam-dir needs --array")):
        r = _run(["-e", NAV] + G1 + ["-o", str(out)] + extra)
        assert r.returncode == 1 and want in r.stderr, r.stderr[-500:]
    bad = tmp_path / "bad.txt"
    for text, want in (("0,0\n", "line 1 is not east_m,north_m,up_m"), ("0,0,0,0\n", "line 1 is not"), ("0,0,0\nx,0,0\n", "line 2 is not"),
                       ("# nothing\n\n", "it must hold 1 to 8 elements"), ("0,0,0\n" * 9, "it must hold 1 to 8 elements"), ("0,nan,0\n", "line 1 is not")):
        bad.write_text(text)
        r = _run(["-e", NAV] + G1 + ["-o", str(out), "--array", str(bad)])
        assert r.returncode == 1 and "ERROR: --array" in r.stderr and want in r.stderr, (text, r.stderr[-500:])
    r = _run(["-e", NAV] + G1 + ["-o", str(out), "--array", str(tmp_path / "missing.txt")])
    assert r.returncode == 1 and "cannot be opened" in r.stderr
    left = sorted(p.name for p in tmp_path.iterdir())
    assert left == ["a.txt", "bad.txt", "other.txt"], left  # no output file, no log, no monitor file


@pytest.mark.gpu
def test_elements_at_the_reference_point_are_the_plain_run(tmp_path):
    arr = tmp_path / "a.txt"
    arr.write_text("0,0,0\n0,0,0\n# the third\n0,0,0\n 0 , 0 , 0\n")
    plain = tmp_path / "plain.ishort"
    _ok(["-o", str(plain)])
    assert os.path.getsize(str(plain)) == 4 * EPOCHS * N
    r = _ok(["-o", str(tmp_path / "el.ishort"), "--array", str(arr), "-B", "7"])
    assert "Antenna array: 4 elements" in r.stderr
    for k in range(4):
        assert _md5(tmp_path / ("el.a%d.ishort" % k)) == _md5(plain), k
    assert not (tmp_path / "el.ishort").exists()
    # one element keeps the suffix; a name without an extension gets it at the end; ibyte and ibit go the same way
    arr.write_text("0,0,0\n")
    _ok(["-o", str(tmp_path / "one"), "--array", str(arr)])
    assert _md5(tmp_path / "one.a0") == _md5(plain)
    arr.write_text("0,0,0\n0,0,0\n")
    for fmt in ("ibyte", "ibit"):
        _ok(["-o", str(tmp_path / ("p." + fmt)), "--iq-format", fmt])
        _ok(["-o", str(tmp_path / ("e." + fmt)), "--iq-format", fmt, "--array", str(arr), "-B", "5"])
        for k in range(2):
            assert _md5(tmp_path / ("e.a%d.%s" % (k, fmt))) == _md5(tmp_path / ("p." + fmt)), (fmt, k)


def _log(path):
    """--array-log: {(epoch, prn): (az_deg, el_deg, [index per element])}"""
    out = {}
    for line in open(str(path)):
        f = line.strip().split(",")
        out[(int(round(float(f[0]) * 10)), int(f[1]))] = (float(f[2]), float(f[3]), [int(v) for v in f[4:]])
    return out


@pytest.mark.gpu
def test_one_satellite_is_turned_by_its_direction_of_arrival(pkg, sky, tmp_path):
    """Two elements, the second 0.095 m east; one satellite at unity, every other at Q7 gain 0, the path loss off.  Element 0 is the
    plain run; element 1 is the model applied to element 0 with the table indices of --array-log, byte for byte; and the angle between
    the two over the first epoch is the geometric 2 pi east sin az cos el / lambda of the logged direction to 0.2 degrees: half a table
    step (0.176) plus the weight's rounding (0.007); the output rounding averages out over 260 000 samples."""
    prn = int(sky["prn"][0][sky["prn"][0] > 0][0])
    assert (sky["prn"] == prn).any(axis=1).all()  # in view throughout
    arr = tmp_path / "a.txt"
    arr.write_text(TWO)
    power = _only(sky, prn)
    plain = tmp_path / "plain.ishort"
    _ok(["-o", str(plain)] + power)
    log = tmp_path / "log.csv"
    _ok(["-o", str(tmp_path / "el.ishort"), "--array", str(arr), "--array-log", str(log)] + power)
    assert _md5(tmp_path / "el.a0.ishort") == _md5(plain)
    x0, x1 = _iq(tmp_path / "el.a0.ishort"), _iq(tmp_path / "el.a1.ishort")
    rows = _log(log)
    assert len(rows) == int((sky["prn"] > 0).sum())
    C = pkg.tables()["cos1024"]
    w = np.zeros((EPOCHS, 1, 1, 2), dtype=np.int64)
    for e in range(EPOCHS):
        az, el, idx = rows[(e, prn)]
        assert len(idx) == 2 and idx[0] == 0
        want = array_model.steer_index(array_model.array_phase((EAST, 0.0, 0.0), math.radians(az), math.radians(el)))
        assert (idx[1] - int(want)) % 1024 in (0, 1, 1023)  # (the log's four decimals of a degree against the front-end's doubles)
        w[e, 0, 0] = array_model.steer_make(128, idx[1] << 22, C)
    y, sat = array_model.array(x0[None, :], w, N)
    assert sat == 0 and y[0].tobytes() == x1.tobytes()
    a = x0[:2 * N].astype(np.float64).view(np.complex128)
    b = x1[:2 * N].astype(np.float64).view(np.complex128)
    got = math.degrees(np.angle(np.sum(b * np.conj(a))))
    az, el, _ = rows[(0, prn)]
    geo = 360.0 * EAST * math.sin(math.radians(az)) * math.cos(math.radians(el)) / array_model.LAMBDA_E1
    print("PRN %d from az %.2f el %.2f: measured %.4f deg, geometric %.4f deg" % (prn, az, el, got, geo))
    assert abs((got - geo + 180.0) % 360.0 - 180.0) <= 0.2


@pytest.mark.gpu
def test_full_sky_with_power_model_and_scint_is_the_model_of_every_element(pkg, sky, tmp_path):
    """Three elements, every satellite in view at its path-loss gain, two of them fading: every element file is
    compose_model.array_model_run over the engine's own runs of every slot alone, with the front-end's gains, the phases index << 22 of
    --array-log and the scintillation table the test builds from the file's lines -- a weight per satellite, epoch and element.  The
    same bytes for -B 4 and -B 7; the log holds one line per epoch and PRN in view."""
    import compose_model
    import gain_model

    K = 3
    arr = tmp_path / "a.txt"
    arr.write_text("0,0,0\n%g,0,0\n0,0.12,0.05\n" % EAST)
    in_view = [int(p) for p in sky["prn"][0] if p > 0]
    spec = [(in_view[1], 0.8, 0.02), (in_view[4], 0.5, 0.05)]
    sc_file = tmp_path / "s.txt"
    sc_file.write_text("".join("%d,%g,%g\n" % s for s in spec))
    log = tmp_path / "log.csv"
    opts = ["--array", str(arr), "--power-model", "--scint", str(sc_file), "--scint-seed", "4"]
    _ok(["-o", str(tmp_path / "el.ishort"), "-B", "4", "--array-log", str(log)] + opts)
    _ok(["-o", str(tmp_path / "e7.ishort"), "-B", "7"] + opts)
    lines = [ln for ln in open(str(log)) if ln.strip()]
    entries = _log(log)
    assert len(lines) == len(entries) == int((sky["prn"] > 0).sum())
    assert set(entries) == {(e, int(p)) for e in range(EPOCHS) for p in sky["prn"][e] if p > 0}
    sc = pkg.Scenario(NAV, llh=(-6, 51, 100), start=START, duration_s=2, iono_enable=False)
    sc.set_power(None, None, path_loss=True)
    rows, gains = sc.next_gains(sc.total_epochs)
    assert np.array_equal(rows["prn"], sky["prn"]) and len(np.unique(gains[rows["prn"] > 0])) > 6 and gains.max() <= 1023
    n = 1 + max(int(s) for s in np.argwhere(rows["prn"] > 0)[:, 1])
    phase = np.zeros((EPOCHS, K, rows.shape[1]), dtype=np.int64)
    for e in range(EPOCHS):
        for s in range(n):
            if rows["prn"][e, s] > 0:
                idx = entries[(e, int(rows["prn"][e, s]))][2]
                assert len(idx) == K and idx[0] == 0
                phase[e, :, s] = np.asarray(idx, dtype=np.int64) << 22
    assert len(np.unique(phase[:, 1:, :n])) > len(in_view)  # (two seconds move no satellite far: about one index per satellite and element)
    table = compose_model.cli_scint_rows(pkg, rows, spec, 4, 0, FS)
    with pkg.SynthEngine(sample_rate=FS, samples_per_epoch=N, n_slots=rows.shape[1], device=0) as eng:
        alone = np.stack([np.ascontiguousarray(eng.run_host(gain_model.slot_alone(rows, s))[0]).view(np.int16).ravel() for s in range(n)])
    want, _ = compose_model.array_model_run(alone, rows, gains, phase, table, 0, N, pkg.tables()["cos1024"])
    for k in range(K):
        got = _iq(tmp_path / ("el.a%d.ishort" % k))
        bad = np.flatnonzero(got != want[k])
        assert got.size == want[k].size and bad.size == 0, "element %d: %d values differ, the first at %d (epoch %d)" % (
            k, bad.size, bad[0], bad[0] // (2 * N))
        assert _md5(tmp_path / ("e7.a%d.ishort" % k)) == _md5(tmp_path / ("el.a%d.ishort" % k)), k
    assert _md5(tmp_path / "el.a0.ishort") != _md5(tmp_path / "el.a1.ishort") != _md5(tmp_path / "el.a2.ishort")


@pytest.mark.gpu
def test_noise_is_independent_per_element_and_the_bytes_do_not_depend_on_the_batch(pkg, sky, tmp_path):
    arr = tmp_path / "a.txt"
    arr.write_text(TWO)
    _ok(["-o", str(tmp_path / "q.ishort"), "--array", str(arr)])  # no noise: what --signal-gain 1 adds the noise to
    opts = ["--array", str(arr), "--cn0", "45", "--signal-gain", "1", "--noise-seed", "9"]
    r = _ok(["-o", str(tmp_path / "n.ishort"), "-B", "1"] + opts)
    assert "noise stream 8 x --noise-stream + 1" in r.stderr
    _ok(["-o", str(tmp_path / "m.ishort"), "-B", "7"] + opts)
    _ok(["-o", str(tmp_path / "r.ishort"), "-B", "7"] + opts)
    for k in range(2):
        assert _md5(tmp_path / ("n.a%d.ishort" % k)) == _md5(tmp_path / ("m.a%d.ishort" % k)) == _md5(tmp_path / ("r.a%d.ishort" % k))
    assert _md5(tmp_path / "n.a0.ishort") != _md5(tmp_path / "n.a1.ishort")
    # the noise of an element = its file minus its noise-free file (the first epoch; the few clamped values aside)
    nz = [_iq(tmp_path / ("n.a%d.ishort" % k))[:2 * N].astype(np.float64) - _iq(tmp_path / ("q.a%d.ishort" % k))[:2 * N] for k in range(2)]
    sigma = pkg.noise_from_cn0(45, FS, 1.0)["sigma_q4"] / 16.0
    rho = float(np.corrcoef(nz[0], nz[1])[0, 1])
    print("sigma %.1f: element noise std %.1f, %.1f, correlation %.4f" % (sigma, nz[0].std(), nz[1].std(), rho))
    for k in range(2):
        assert abs(nz[k].std() / sigma - 1.0) < 0.02
    assert abs(rho) < 0.01  # (520 000 values: one sigma of the estimate is 0.0014) -- the difference is not the signal's rotation alone
    # another --noise-stream: other noise on both
    _ok(["-o", str(tmp_path / "s.ishort"), "--noise-stream", "1"] + opts)
    assert _md5(tmp_path / "s.a0.ishort") not in (_md5(tmp_path / "n.a0.ishort"), _md5(tmp_path / "n.a1.ishort"))


def _tone(path, f_hz):
    x = _iq(path)[:2 * N].astype(np.float64).view(np.complex128)
    return np.sum(x * np.exp(-2j * np.pi * f_hz / FS * np.arange(N)))


@pytest.mark.gpu
def test_a_jammer_arrives_from_its_direction(pkg, sky, tmp_path):
    """All satellites muted, one CW source at 100 kHz.  From the east on the horizon the second element's tone leads by
    gal_synth_array_phase's value, to the table step of cos1024 (0.35 degrees); without --jam-dir it arrives from the zenith, both
    elements lie at up = 0, and the angle is 0."""
    arr = tmp_path / "a.txt"
    arr.write_text(TWO)
    mute = _only(sky, None)
    r = _ok(["-o", str(tmp_path / "j.ishort"), "--array", str(arr), "--jam", "30,100000", "--jam-dir", "90,0"] + mute)
    assert "azimuth 90.00 deg, elevation 0.00 deg" in r.stderr and "sqrt(2) larger" in r.stderr
    t0, t1 = _tone(tmp_path / "j.a0.ishort", 1e5), _tone(tmp_path / "j.a1.ishort", 1e5)
    assert abs(t0) > 1000.0 * N
    got = math.degrees(np.angle(t1 * np.conj(t0)))
    want = pkg.array_phase((EAST, 0.0, 0.0), math.radians(90.0), 0.0) / 2.0 ** 32 * 360.0
    print("jammer: measured %.4f deg, array_phase %.4f deg" % (got, want))
    assert abs((got - want + 180.0) % 360.0 - 180.0) <= 360.0 / 1024
    r = _ok(["-o", str(tmp_path / "z.ishort"), "--array", str(arr), "--jam", "30,100000"] + mute)
    assert "the zenith" in r.stderr
    assert _md5(tmp_path / "z.a0.ishort") == _md5(tmp_path / "z.a1.ishort")
    z0, z1 = _tone(tmp_path / "z.a0.ishort", 1e5), _tone(tmp_path / "z.a1.ishort", 1e5)
    assert abs(math.degrees(np.angle(z1 * np.conj(z0)))) < 1e-9
