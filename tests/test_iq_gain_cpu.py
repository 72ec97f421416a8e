"""Per-satellite signal power without a GPU: gal_synth_gain_q7 against the numpy statement of its formula (tests/gain_model.py), the
gains the scenario front-end computes beside its rows (gal_scen_next_gains), and the CLI's refusal of malformed --prn-power / --antenna
input, which happens before any device work."""
import math
import os
import subprocess

import numpy as np
import pytest

import gain_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
GAL_E_INVAL = -1
D0 = gain_model.REF_DISTANCE_M
# a pattern of the tests' own: 0 dB over the first 10 degrees, then 0.25 dB more per 5 degrees, 3 dB extra below the horizon
PATTERN = [0.0, 0.0] + [0.25 * k for k in range(1, 17)] + [7.0 + 0.5 * k for k in range(19)]
assert len(PATTERN) == 37


def test_exported_and_constants(pkg):
    lib = pkg.load_library()
    for name in ("gal_synth_gain_q7", "gal_synth_iq_wsum", "gal_synth_run_gains"):
        assert hasattr(lib, name), name
    scen = pkg.scenario.load_library()
    for name in ("gal_scen_set_power", "gal_scen_set_path_loss", "gal_scen_next_gains"):
        assert hasattr(scen, name), name
    assert pkg.GAL_GAIN_UNITY == gain_model.GAL_GAIN_UNITY == 128 and pkg.GAL_GAIN_MAX == gain_model.GAL_GAIN_MAX == 32767


def test_gain_q7_hand_picked(pkg):
    z = math.pi / 2
    assert pkg.gain_q7(D0, z) == 128  # the zenith at the reference distance: unity
    assert pkg.gain_q7(2 * D0, z) == 64 and pkg.gain_q7(D0 / 2, z) == 256
    assert pkg.gain_q7(D0, z, offset_db=6.0206) == 256  # 10^0.30103 = 2.0000000199: doubles
    assert pkg.gain_q7(D0, z, offset_db=-6.0206) == 63  # 0.49999999...: truncated like the reference's (int)
    # the pattern steps every 5 degrees off the zenith: 10 degrees off is index 2 (0.25 dB), 9.99 degrees still index 1 (0 dB)
    assert pkg.gain_q7(D0, math.radians(80.01), PATTERN) == 128
    assert pkg.gain_q7(D0, math.radians(79.99), PATTERN) == gain_model.gain_q7(D0, math.radians(79.99), PATTERN) == 124
    assert int(128 * 10.0 ** (-0.25 / 20.0)) == 124
    # elevations 90, 0 and below: indices 0, 18, up to 36 (and no further)
    assert gain_model.boresight_index(z) == 0 and gain_model.boresight_index(0.0) == 18
    assert gain_model.boresight_index(-z) == 36 and gain_model.boresight_index(-3.0) == 36 and gain_model.boresight_index(2.0) == 0
    for elev in (z, 0.0, -0.3, -z, -3.0, 2.0):
        assert pkg.gain_q7(25.0e6, elev, PATTERN, 1.5) == gain_model.gain_q7(25.0e6, elev, PATTERN, 1.5), elev
    assert pkg.gain_q7(D0, 0.0, PATTERN) == int(128 * 10.0 ** (-PATTERN[18] / 20.0))
    # the clamp
    assert pkg.gain_q7(D0, z, offset_db=48.0) == 32152 and pkg.gain_q7(D0, z, offset_db=48.2) == 32767
    assert pkg.gain_q7(D0 / 1000.0, z, offset_db=60.0) == 32767
    assert pkg.gain_q7(1e12, z) == 0


def test_gain_q7_bad_arguments(pkg):
    for args in ((0.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0), (D0, float("inf")), (D0, 1.0, None, float("nan")),
                 (D0, 1.0, [0.0] * 36 + [float("inf")], 0.0)):
        with pytest.raises(pkg.GalSynthError) as e:
            pkg.gain_q7(*args)
        assert e.value.code == GAL_E_INVAL
    with pytest.raises(ValueError):
        pkg.gain_q7(D0, 1.0, [0.0] * 36)
    assert pkg.load_library().gal_synth_gain_q7(D0, 1.0, None, 0.0, None) == GAL_E_INVAL


def test_gain_q7_random_inputs(pkg):
    """libm's pow and numpy's may differ in the last bit, which shows only where the product lies on a truncation boundary: never by
    more than 1, and on fewer than 1 % of the inputs."""
    rng = np.random.default_rng(20220220)
    n, differ = 1000, 0
    for _ in range(n):
        d = rng.uniform(20.0e6, 30.0e6)
        elev = rng.uniform(-0.2, math.pi / 2)
        pat = PATTERN if rng.integers(0, 2) else None
        off = rng.uniform(-20.0, 20.0)
        got, want = pkg.gain_q7(d, elev, pat, off), gain_model.gain_q7(d, elev, pat, off)
        assert abs(got - want) <= 1, (d, elev, off, got, want)
        differ += got != want
    assert differ < n // 100, differ


def _scenario(pkg, **kw):
    return pkg.Scenario(NAV, llh=(-6.0, 51.0, 100.0), start="2022/02/20,12:00:00", duration_s=3.0, iono_enable=False, **kw)


def test_scenario_gains(pkg):
    plain = _scenario(pkg).all()
    sc = _scenario(pkg)
    rows, gains = sc.next_gains(sc.total_epochs)
    assert rows.shape == plain.shape == gains.shape == (29, 16) and gains.dtype == np.uint16
    assert rows.tobytes() == plain.tobytes()
    active = rows["prn"] > 0
    assert active.any() and not active.all()
    assert np.array_equal(gains == 0, ~active)
    # no pattern, no offsets: the path loss alone, for distances between 23.2e6 and 29.5e6 m
    lo, hi = int(128.0 * (D0 / 29.5e6)), int(128.0 * (D0 / 23.2e6))
    assert (lo, hi) == (100, 128)
    assert gains[active].min() >= lo and gains[active].max() <= hi
    assert len(np.unique(gains[active])) > 1  # the satellites do not all stand at one distance
    # in two pieces: the same rows and gains
    sc = _scenario(pkg)
    r1, g1 = sc.next_gains(10)
    r2, g2 = sc.next_gains(100)
    assert np.array_equal(np.concatenate([g1, g2]), gains) and np.concatenate([r1, r2]).tobytes() == rows.tobytes()


def test_scenario_pattern_offsets_and_path_loss_switch(pkg):
    base_sc = _scenario(pkg)
    _, base = base_sc.next_gains(base_sc.total_epochs)
    sc = _scenario(pkg)
    sc.set_power(None, None, path_loss=False)
    rows, unit = sc.next_gains(sc.total_epochs)
    active = rows["prn"] > 0
    assert np.array_equal(unit[active], np.full(active.sum(), 128)) and not unit[~active].any()
    prn = int(rows["prn"][active][0])
    sc = _scenario(pkg)
    sc.set_power(None, {prn: 6.0206}, path_loss=False)
    rows, up = sc.next_gains(sc.total_epochs)
    assert np.array_equal(up[rows["prn"] == prn], np.full((rows["prn"] == prn).sum(), 256))
    other = (rows["prn"] > 0) & (rows["prn"] != prn)
    assert np.array_equal(up[other], np.full(other.sum(), 128))
    # an attenuating pattern never raises a gain, and lowers some (no satellite of this sky stands within 10 degrees of the zenith)
    sc = _scenario(pkg)
    sc.set_power(PATTERN, None)
    _, pat = sc.next_gains(sc.total_epochs)
    assert (pat <= base).all() and (pat[active] < base[active]).any() and not pat[~active].any()
    with pytest.raises(ValueError):
        sc.set_power([0.0] * 5)
    with pytest.raises(ValueError):
        sc.set_power(None, {51: 1.0})
    with pytest.raises(pkg.GalScenError):
        sc.set_power([float("nan")] * 37)


def _cli(*args):
    return subprocess.run([CLI, "-e", NAV, "-l", "-6,51,100", "-t", "2022/02/20,12:00:00", "-d", "1", "-P", "0"] + list(args),
                          capture_output=True, text=True, timeout=120)


def test_cli_refuses_malformed_power_options(pkg, tmp_path):
    out = tmp_path / "x.ishort"
    for spec in ("5", "5:", ":3", "0:3", "51:3", "5:abc", "5:3,", "5:3;6:1", "5:nan", "5:inf", "5:61", "5:3,x:1", " 5:3", "-5:3", ""):
        r = _cli("--prn-power", spec, "-o", str(out))
        assert r.returncode != 0 and "--prn-power" in r.stderr and "is not prn:dB" in r.stderr, (spec, r.stderr)
        assert not out.exists()
    r = _cli("--antenna", str(tmp_path / "missing.txt"), "-o", str(out))
    assert r.returncode != 0 and "--antenna" in r.stderr and "cannot read" in r.stderr
    cases = {"short": " ".join(["1.0"] * 36), "long": "\n".join(["1.0"] * 38), "word": " ".join(["1.0"] * 36 + ["loud"]),
             "nan": " ".join(["1.0"] * 36 + ["nan"]), "huge": " ".join(["1.0"] * 36 + ["1e3"]), "empty": ""}
    for name, text in cases.items():
        f = tmp_path / (name + ".txt")
        f.write_text(text)
        r = _cli("--antenna", str(f), "-o", str(out))
        assert r.returncode != 0 and "--antenna" in r.stderr, (name, r.stderr)
        assert ("values, not 37" in r.stderr) or ("is not a number of dB" in r.stderr), (name, r.stderr)
        assert not out.exists()
    assert "--power-model" in subprocess.run([CLI], capture_output=True, text=True).stdout


def test_cli_prints_the_power_choices(pkg, tmp_path):
    """Well-formed options are taken, and the headroom of --cn0 is sized for the largest gain they can produce, before any device
    work: visible on a machine without a GPU too (where the run then stops)."""
    f = tmp_path / "ant.txt"
    f.write_text("# dB per 5 degrees off the zenith\n" + ", ".join("%.2f" % v for v in PATTERN) + "\n")
    r = _cli("--power-model", "--antenna", str(f), "--prn-power", "5:-6,12:3", "--prn-power", "9:1.5", "-o", str(tmp_path / "x.ishort"))
    assert "Signal power: path loss on, antenna %s, 2 PRN offset lists; largest gain 1.432 (3.12 dB)" % f in r.stderr, r.stderr
    # 5 sigma + 4100 g: at 45 dB-Hz sigma = 2267, 11 335 + 4100 fits; with +16 dB on one PRN 4100 x 6.31 = 25 869 does not: gain 0.5
    assert "signal gain 1 (chosen)" in _cli("--cn0", "45", "-o", str(tmp_path / "x.ishort")).stderr
    r = _cli("--cn0", "45", "--prn-power", "5:16", "-o", str(tmp_path / "x.ishort"))
    assert "signal gain 0.5 (chosen)" in r.stderr, r.stderr


def test_model_at_the_int32_bound_of_the_narrow_sum():
    """The inputs of tests/test_iq_gain_gpu.py::test_wsum_at_the_int32_bound reach what they claim: with all three parts at -32768 the
    row [32767, 32767, 1] (sum 65535, the largest the int32 instance of k_iq_wsum takes) gives w = -65535 x 32768, which an int32
    holds with the rounding 64 added; the rows that sum to 65536 and 65537 give -2^31 exactly and -2^31 - 32768, and 65537 x -32768
    does not fit an int32: those calls need the int64 instance.  At +32767 all three fit, the sign decides."""
    spe, n_epochs = 4, 2
    rows = ([32767, 32767, 1], [32767, 32767, 2], [32767, 32767, 3])
    lo, hi = -2 ** 31, 2 ** 31 - 1
    for level in (-32768, 32767):
        parts = np.full((3, n_epochs * spe * 2), level, dtype=np.int16)
        for row in rows:
            g = np.tile(row, (n_epochs, 1))
            w = (g.astype(np.int64)[0][:, None] * parts[:, : 2 * spe].astype(np.int64)).sum(axis=0)  # the model's w of epoch 0
            assert (w == sum(row) * level).all()
            y, sat = gain_model.wsum(parts, g, spe)
            assert (y == level).all() and sat == parts.shape[1]  # |(w + 64) >> 7| = 16.7 M: every value clamps, to the parts' own level
            if level < 0:
                assert (lo <= int(w[0]) and int(w[0]) + 64 <= hi) == (sum(row) <= 65536)
            else:
                assert lo <= int(w[0]) and int(w[0]) + 64 <= hi
    assert -65535 * 32768 == -2147450880 and lo <= -65535 * 32768 and -65535 * 32768 + 64 <= hi
    assert 65535 * 32767 + 64 <= hi
    assert 65536 * -32768 == lo and 65537 * -32768 < lo  # the host sends any row above 65535 to the int64 instance
