"""galileo-sdr-sim --scint: the refused files and options with their messages and the printed rows (before any device work) and, on the
MI355X, the file -- the same bytes for two batch lengths, the plain run's file at s4 = 0 and for a PRN that is not in view, another
file for another --scint-seed; and the file against the models: one fading satellite against scint_model alone; the full sky with
--multipath and --power-model, and --oversample 3 with the decimator, against a mirror through SynthEngine.run_scint with a table the
test builds; two identical --sites against the single runs with --scint-site; the headroom of the chosen --signal-gain."""
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
LINE = re.compile(r"Scintillation: PRN (\d+), S4 (\S+), tau0 (\S+) s -> A (\d+), B (\d+), L (\d+) \(tau0 (\S+) s at (\S+) MS/s\), seed (\d+), stream (\d+)")


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


def _in_view(sky):
    return [int(p) for p in sky["prn"][0] if p > 0], next(p for p in range(1, 51) if not (sky["prn"] == p).any())


def test_refused_files_and_options_before_any_device_work(tmp_path):
    f = tmp_path / "s.txt"
    cases = [("5,0.8\n", "line 1 is not prn,s4,tau0_s"), ("5,0.8,0.5,1\n", "line 1 is not prn,s4,tau0_s"), ("5,abc,0.5\n", "line 1 is not"),
             ("# only a comment\n\n", "it holds no satellite"), ("0,0.5,0.5\n", "PRN outside 1..50"), ("51,0.5,0.5\n", "PRN outside 1..50"),
             ("5.5,0.5,0.5\n", "PRN outside 1..50"), ("5,0.5,0.5\n# again\n5,0.2,0.5\n", "line 3: a second line for PRN 5"),
             ("5,1.5,0.5\n", "line 1: s4 outside 0..1"), ("5,-0.1,0.5\n", "line 1: s4 outside 0..1"),
             ("5,0.5,0.0001\n", "node_len"), ("5,0.5,100\n", "node_len"), ("5,0.5,-1\n", "node_len")]
    for text, want in cases:
        f.write_text(text)
        r = _run(["-e", NAV] + G1 + ["-o", str(tmp_path / "x.ishort"), "--scint", str(f)])
        assert r.returncode == 1 and "ERROR: --scint" in r.stderr and want in r.stderr, (text, r.stderr[-500:])
    r = _run(["-e", NAV] + G1 + ["-o", str(tmp_path / "x.ishort"), "--scint", str(tmp_path / "missing.txt")])
    assert r.returncode == 1 and "cannot read it" in r.stderr
    f.write_text("5,0.5,0.5\n")
    for extra, want in ((["--scint-seed", "-1"], "--scint-seed '-1' is not an unsigned 64-bit integer"),
                        (["--scint-seed", "x"], "--scint-seed 'x'"), (["--scint-site", str(1 << 24)], "--scint-site")):
        r = _run(["-e", NAV] + G1 + ["-o", str(tmp_path / "x.ishort"), "--scint", str(f)] + extra)
        assert r.returncode == 1 and want in r.stderr, r.stderr[-500:]
    for extra in (["--scint-seed", "3"], ["--scint-site", "3"]):
        r = _run(["-e", NAV] + G1 + ["-o", str(tmp_path / "x.ishort")] + extra)
        assert r.returncode == 1 and "need --scint <file>" in r.stderr
    assert not (tmp_path / "x.ishort").exists()


@pytest.mark.parametrize("osr", [1, 3])
def test_the_printed_rows_are_those_of_scint_make(pkg, tmp_path, osr):
    """The lines come out of the option stage, in front of any device work: they are there with or without a GPU.  A comment behind
    the values, blanks around them; the rate is the one the synthesis runs at; stream = site << 8 | prn."""
    f = tmp_path / "s.txt"
    spec = [(5, 0.8, 0.5), (12, 0.3, 1.0), (31, 1.0, 0.02), (7, 0.0, 2.0)]
    f.write_text("# prn,s4,tau0_s\n\n5,0.8,0.5\n 12 , 0.3 , 1.0   # mild\n31,1,0.02\n7,0,2\n")
    args = ["--scint", str(f), "--scint-seed", "77", "--scint-site", "3"] + (["--oversample", str(osr)] if osr > 1 else [])
    r = _run(["-e", NAV] + G1 + ["-o", str(tmp_path / "x.ishort")] + args)
    got = {int(m.group(1)): m for m in LINE.finditer(r.stdout + r.stderr)}
    assert sorted(got) == [5, 7, 12, 31], (r.stdout + r.stderr)[-2000:]
    for prn, s4, tau0 in spec:
        want = pkg.scint_make(s4, tau0, osr * FS)
        m = got[prn]
        assert (int(m.group(4)), int(m.group(5)), int(m.group(6))) == (want["a_q12"], want["b_q12"], want["node_len"]), prn
        assert abs(float(m.group(7)) - 8.0 * want["node_len"] / (osr * FS)) < 1e-6 * tau0 + 1e-9
        assert abs(float(m.group(8)) - osr * 2.6) < 1e-9 and int(m.group(9)) == 77 and int(m.group(10)) == (3 << 8) | prn
    # the headroom: the largest (A + 4 B) / 4096, here the Rayleigh row's
    ray = pkg.scint_make(1.0, 0.02, osr * FS)
    m = re.search(r"a satellite is taken at up to (\S+) times its own amplitude", r.stdout + r.stderr)
    assert m and abs(float(m.group(1)) - 4.0 * ray["b_q12"] / 4096.0) < 1e-3


@pytest.mark.gpu
def test_the_file_for_two_batch_lengths_seeds_and_the_identity(pkg, sky, tmp_path):
    in_view, absent = _in_view(sky)
    f = tmp_path / "s.txt"
    f.write_text("%d,0.8,0.02\n%d,0.4,0.05\n%d,0.9,0.02\n" % (in_view[0], in_view[2], absent))
    plain = tmp_path / "plain.ishort"
    _ok(["-o", str(plain)])
    assert os.path.getsize(str(plain)) == 4 * EPOCHS * 260000
    a, b, c = tmp_path / "a.ishort", tmp_path / "b.ishort", tmp_path / "c.ishort"
    _ok(["-o", str(a), "--scint", str(f), "-B", "4"])
    _ok(["-o", str(b), "--scint", str(f), "-B", "7"])
    assert os.path.getsize(str(a)) == os.path.getsize(str(plain))
    assert _md5(a) == _md5(b) != _md5(plain)
    _ok(["-o", str(c), "--scint", str(f), "-B", "7", "--scint-seed", "2"])
    assert _md5(c) not in (_md5(a), _md5(plain))
    _ok(["-o", str(c), "--scint", str(f), "-B", "7", "--scint-seed", "1", "--scint-site", "0"])  # the defaults, spelled out
    assert _md5(c) == _md5(a)
    _ok(["-o", str(c), "--scint", str(f), "-B", "7", "--scint-site", "1"])
    assert _md5(c) not in (_md5(a), _md5(plain))
    # s4 = 0 for every PRN, and a PRN that is not in view: the file of the run without the option
    f.write_text("".join("%d,0,0.5\n" % p for p in range(1, 51)))
    _ok(["-o", str(c), "--scint", str(f)])
    assert _md5(c) == _md5(plain)
    f.write_text("%d,0.9,0.02\n" % absent)
    _ok(["-o", str(c), "--scint", str(f), "-B", "5"])
    assert _md5(c) == _md5(plain)


# ---- the file against the models ------------------------------------------------------------------------------------------------------
C_LIGHT = 299792458.0
N = 260000


def _iq(path):
    return np.fromfile(str(path), dtype=np.int16)


def _only(sky, keep):
    """--prn-power that leaves `keep` at unity and takes every other PRN that is ever in view to -60 dB: Q7 gain 0."""
    prns = sorted({int(p) for p in sky["prn"].ravel() if p > 0 and p != keep})
    return ["--prn-power", ",".join("%d:-60" % p for p in prns)]


def _scint_file(path, spec):
    path.write_text("# prn,s4,tau0_s\n" + "".join("%d,%g,%g\n" % s for s in spec))
    return ["--scint", str(path)]


def _differ(got, want):
    bad = np.flatnonzero(got != want)
    return "%d of %d values differ (first at %d)" % (bad.size, got.size, bad[0] if bad.size else -1)


@pytest.mark.gpu
def test_one_fading_satellite_is_the_numpy_model_of_the_plain_file(pkg, sky, tmp_path):
    """One satellite at unity, every other at Q7 gain 0: the file is scint_model.apply of the file without --scint, with the row of
    scint_make, seed = --scint-seed, stream = --scint-site << 8 | PRN and the sample count from 0 -- no library call in the
    expectation.  A wrong seed, stream, rate or sample count in the command gives other bytes."""
    import scint_model

    prn = _in_view(sky)[0][0]
    assert (sky["prn"] == prn).any(axis=1).all()  # in view throughout
    power = _only(sky, prn)
    plain = tmp_path / "plain.ishort"
    _ok(["-o", str(plain)] + power)
    row = dict(pkg.scint_make(0.8, 0.02, FS), seed=77, stream=(3 << 8) | prn)
    want, _ = scint_model.apply(_iq(plain), scint_model.row(**row), 0)
    assert want.size == 2 * EPOCHS * N and np.count_nonzero(want != _iq(plain)) > 0.4 * want.size  # (one satellite alone: many values are 0)
    opts = _scint_file(tmp_path / "s.txt", [(prn, 0.8, 0.02)]) + ["--scint-seed", "77", "--scint-site", "3"] + power
    for batch in ("4", "7"):
        out = tmp_path / ("b%s.ishort" % batch)
        _ok(["-o", str(out), "-B", batch] + opts)
        got = _iq(out)
        assert got.size == want.size and np.array_equal(got, want), "-B %s: %s" % (batch, _differ(got, want))


def _echo_rows(pkg, sky, gains, spec, fs, spe):
    """As _mirror_rows of tests/test_iq_mpath_cli.py, with the gains of --power-model: an echo goes to the slot that carries its PRN,
    with the rows of gal_synth_mpath_row at the slot's gain where it carries that PRN and at 0 elsewhere."""
    slot_of, cols = [], []
    for prn, delay_m, rel_db, phase, fade in spec:
        where = np.argwhere(sky["prn"] == prn)
        if where.size == 0:
            continue
        slot = int(where[0][1])
        echo = pkg.mpath_make(delay_m / C_LIGHT, rel_db, phase, fade, sample_rate=fs)
        slot_of.append(slot)
        cols.append(pkg.mpath_rows(echo, np.where(sky["prn"][:, slot] == prn, gains[:, slot], 0), 0, spe))
    return slot_of, np.stack(cols, axis=1)


@pytest.mark.gpu
def test_full_sky_with_multipath_and_power_model_is_the_mirror(pkg, sky, tmp_path):
    """--scint on two satellites, one of them with echoes, another satellite with an echo and no fading, the path-loss gains on all:
    the file for -B 1 and -B 7 is SynthEngine.run_scint over the whole sky in one call, with the table this test builds line by line
    (tests/test_run_compose_gpu.py holds that call against the numpy models)."""
    import torch

    import compose_model

    in_view, absent = _in_view(sky)
    echoes = [(in_view[0], 250.0, -6.0, 90.0, 0.0), (in_view[0], 20000.0, -3.0, 0.0, -1.25), (in_view[1], 120.0, 0.0, 45.0, 0.0), (absent, 300.0, -3.0, 10.0, 0.0)]
    (tmp_path / "echoes.txt").write_text("".join("%d,%g,%g,%g,%g\n" % e for e in echoes))
    spec = [(in_view[0], 0.8, 0.02), (in_view[2], 0.4, 0.05), (absent, 0.9, 0.02)]
    opts = _scint_file(tmp_path / "s.txt", spec) + ["--scint-seed", "5", "--multipath", str(tmp_path / "echoes.txt"), "--power-model"]
    a, b = tmp_path / "a.ishort", tmp_path / "b.ishort"
    _ok(["-o", str(a), "-B", "1"] + opts)
    _ok(["-o", str(b), "-B", "7"] + opts)
    assert _md5(a) == _md5(b)
    sc = pkg.Scenario(NAV, llh=(-6, 51, 100), start=START, duration_s=2, iono_enable=False)
    sc.set_power(None, None, path_loss=True)
    rows, gains = sc.next_gains(sc.total_epochs)
    assert np.array_equal(rows["prn"], sky["prn"]) and len(np.unique(gains[rows["prn"] > 0])) > 6
    slot_of, echo_rows = _echo_rows(pkg, rows, gains, echoes, FS, N)
    table = compose_model.cli_scint_rows(pkg, rows, spec, 5, 0, FS)
    assert len(slot_of) == 3 and sum(1 for s in range(rows.shape[1]) if compose_model.spans(table, s)) == 2
    with pkg.SynthEngine(sample_rate=FS, samples_per_epoch=N, n_slots=rows.shape[1], device=0) as eng:
        out = torch.zeros(EPOCHS * N * 2, dtype=torch.int16, device="cuda")
        plain = torch.zeros(EPOCHS * N * 2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        eng.run_scint(rows, gains, out.data_ptr(), table, 0, slot_of, echo_rows)
        eng.iq_saturated()
        want = out.cpu().numpy()
        eng.mpath_reset()
        eng.run_scint(rows, gains, plain.data_ptr(), None, 0, slot_of, echo_rows)
        eng.iq_saturated()
        assert np.count_nonzero(plain.cpu().numpy() != want) > 0.5 * want.size
    got = _iq(a)
    assert got.size == want.size and np.array_equal(got, want), _differ(got, want)


@pytest.mark.gpu
def test_oversampled_rows_and_sample_count_run_at_the_high_rate(pkg, sky, tmp_path):
    """--oversample 3: the rows are those of scint_make at 7.8 MS/s and first_sample counts samples of that rate.  The mirror is
    run_scint over the 19 epochs of 780 000 samples in one call and the decimator with the default taps; the command runs in batches of
    2 and of 5 epochs, so that all batches but the first depend on the count."""
    import torch

    import compose_model

    M = 3
    in_view, _ = _in_view(sky)
    spec = [(in_view[0], 0.8, 0.02), (in_view[3], 1.0, 0.01)]
    opts = _scint_file(tmp_path / "s.txt", spec) + ["--oversample", str(M)]
    a, b = tmp_path / "a.ishort", tmp_path / "b.ishort"
    _ok(["-o", str(a), "-B", "2"] + opts)
    _ok(["-o", str(b), "-B", "5"] + opts)
    assert _md5(a) == _md5(b)
    spe = M * N
    table = compose_model.cli_scint_rows(pkg, sky, spec, 1, 0, M * FS)
    assert table["node_len"].max() == pkg.scint_make(0.8, 0.02, M * FS)["node_len"] == 3 * pkg.scint_make(0.8, 0.02, FS)["node_len"]
    taps = pkg.synth.firdec_lowpass(0.45 * FS, M * FS, 32 * M + 1)
    with pkg.SynthEngine(sample_rate=M * FS, samples_per_epoch=spe, n_slots=sky.shape[1], device=0) as eng:
        wide = torch.zeros(EPOCHS * spe * 2, dtype=torch.int16, device="cuda")
        kept = torch.zeros(EPOCHS * N * 2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        eng.run_scint(sky, np.full(sky.shape, 128), wide.data_ptr(), table, 0)
        eng.firdec_set(taps, M, 0)
        assert eng.iq_firdec(wide.data_ptr(), EPOCHS * spe, kept.data_ptr()) == EPOCHS * N
        eng.iq_saturated()
        want = kept.cpu().numpy()
    got = _iq(a)
    assert got.size == want.size and np.array_equal(got, want), _differ(got, want)


@pytest.mark.gpu
def test_two_identical_sites_fade_apart(sky, tmp_path):
    """--sites with the same position twice: site k's file is the single run with --scint-site k, and the two differ."""
    in_view, _ = _in_view(sky)
    opts = _scint_file(tmp_path / "s.txt", [(in_view[0], 0.8, 0.02), (in_view[2], 0.4, 0.05)]) + ["--scint-seed", "9"]
    lst = tmp_path / "sites.txt"
    lst.write_text("-6,51,100\n-6,51,100\n")
    scen = [w for w in G1 if w not in ("-l", "-6,51,100")]
    r = _run(["-e", NAV] + scen + ["--sites", str(lst), "-o", str(tmp_path / "run.ishort"), "--gpus", "1", "--per-gpu", "2"] + opts)
    assert r.returncode == 0 and "Sites = 2  failed = 0" in r.stderr, r.stderr[-2000:]
    md5 = []
    for k in range(2):
        single = tmp_path / ("single%d.ishort" % k)
        _ok(["-o", str(single), "--scint-site", str(k)] + opts)
        md5.append(_md5(single))
        assert _md5(tmp_path / ("run.site%d.ishort" % k)) == md5[k], k
    assert md5[0] != md5[1]


def _gain_for(need):
    """cli_options.cpp's gain_for: the largest power of two <= 1 that keeps `need` inside int16."""
    g = 1.0
    while need * g > 32767.0:
        g *= 0.5
    return g


# echoes of 0 dB and -6 dB on the satellite with the largest row, and a weak one on a satellite that does not fade
LOUD_ECHOES = "12,250,0,90\n12,1000,-6,200,3.5\n9,120,-12,45\n"


@pytest.mark.parametrize("cn0,echoes,want_gain", [(45, None, 1.0), (45, LOUD_ECHOES, 0.5), (39, None, 0.5)],
                         ids=["45", "45-echoes", "39"])
def test_the_chosen_signal_gain_leaves_room_for_the_largest_row(pkg, tmp_path, cn0, echoes, want_gain):
    """--scint --cn0: need x gain <= 32767 < 2 x need x gain with need = 5 sigma + 4100 x (A + 4 B) / 4096 of the largest row, times
    1 + the amplitudes of that satellite's echoes with --multipath (README; 4100: cli_options.cpp's sig_peak).  At 45 dB-Hz the rows
    alone leave the gain at 1 (need 22 930); with the echoes the rule decides: 40 336 asks for 0.5, where a rule without the row's
    factor (21 589) or without the echoes' (22 930) would keep 1.  At 39 dB-Hz the row's factor alone decides (34 210 against 26 715).
    The gain is asserted as a number.  The line comes out of the option stage, with or without a GPU."""
    import noise_model

    spec = [(5, 0.8, 0.5), (12, 1.0, 0.02), (31, 0.2, 1.0)]
    args = _scint_file(tmp_path / "s.txt", spec) + ["--cn0", str(cn0)]
    row_peak = max((r["a_q12"] + 4.0 * r["b_q12"]) / 4096.0 for r in (pkg.scint_make(s4, tau0, FS) for _, s4, tau0 in spec))
    ray = pkg.scint_make(1.0, 0.02, FS)
    assert row_peak == 4.0 * ray["b_q12"] / 4096.0 > 2.5
    echo_peak = 1.0
    if echoes:
        (tmp_path / "e.txt").write_text(echoes)
        args += ["--multipath", str(tmp_path / "e.txt")]
        echo_peak = 1 + 10 ** (0 / 20) + 10 ** (-6 / 20)
    peak = row_peak * echo_peak
    r = _run(["-e", NAV] + G1 + ["-o", str(tmp_path / "x.ishort")] + args)
    text = r.stdout + r.stderr
    m = re.search(r"a satellite is taken at up to (\S+) times its own amplitude", text)
    assert m and abs(float(m.group(1)) - peak) < 1e-3, text[-2000:]
    gain = float(re.search(r"signal gain ([0-9.e+-]+) \(chosen\)", text).group(1))
    unit = noise_model.noise_from_cn0(float(cn0), FS, 1.0)[1] / 16.0
    need = 5 * unit + 4100 * peak
    wrong = {"no row factor": 5 * unit + 4100 * echo_peak, "no echo factor": 5 * unit + 4100 * row_peak, "neither": 5 * unit + 4100}
    print("sigma %.1f, peak %.4f, need %.1f, gain %g; %s" % (unit, peak, need, gain, {k: round(v, 1) for k, v in wrong.items()}))
    assert need * gain <= 32767 < 2 * need * gain
    assert gain == want_gain == _gain_for(need)
    if want_gain < 1.0:  # the case decides: every rule that leaves a factor out chooses another gain
        assert all(_gain_for(v) == 1.0 for k, v in wrong.items() if v != need), wrong
