"""The antenna array without a GPU: gal_synth_steer_make and gal_synth_array_phase against the numpy model (tests/array_model.py), the
refusals of gal_synth_steer_check, the model's own identity with the weighted sum, the layouts through ctypes and through a C99
translation unit, and the directions of arrival the front-end hands out beside its rows (gal_scen_next_azel)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import array_model
import gain_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
GAL_E_INVAL = -1
LAM = array_model.LAMBDA_E1


def test_symbols_and_constants(pkg):
    lib = pkg.load_library()
    for name in ("gal_synth_steer_check", "gal_synth_steer_make", "gal_synth_array_phase", "gal_synth_iq_array", "gal_synth_run_array"):
        assert name in pkg.synth.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "gal_scen_next_azel" in pkg.scenario.EXPORTED_SYMBOLS and hasattr(pkg.scenario.load_library(), "gal_scen_next_azel")
    assert pkg.synth.GAL_ARRAY_MAX_ELEM == array_model.GAL_ARRAY_MAX_ELEM == 8
    assert pkg.synth.GAL_STEER_GAIN_MAX == array_model.GAL_STEER_GAIN_MAX == 1023


def test_steer_make_over_the_whole_table(pkg):
    C = pkg.tables()["cos1024"]
    for g in (0, 1, 127, 128, 1023):
        phases = np.arange(1024, dtype=np.int64) << 22
        re, im = array_model.steer_make(g, phases, C)
        for i in range(1024):
            assert pkg.steer_make(g, int(phases[i])) == (int(re[i]), int(im[i])), (g, i)
        assert max(abs(int(re.max())), abs(int(re.min())), abs(int(im.max())), abs(int(im.min()))) <= 32767
    assert pkg.steer_make(128, 0) == (4096, 0)
    assert pkg.steer_make(128, 1 << 30) == (0, 4096)  # a quarter of a cycle forward: +j
    assert pkg.steer_make(128, 1 << 31) == (-4096, 0)
    assert pkg.steer_make(1023, 0) == (32736, 0)
    # Q7 gain g, unrotated: 32 g, the weighted sum's gain in Q12
    for g in (0, 1, 127, 128, 1023):
        assert pkg.steer_make(g, 0) == (32 * g, 0)


def test_the_phase_is_rounded_to_the_table(pkg):
    C = pkg.tables()["cos1024"]
    g = 1000
    for i in (0, 1, 255, 256, 511, 512, 1022, 1023):
        at = lambda k: tuple(int(v) for v in array_model.steer_make(g, (k & 1023) << 22, C))  # noqa: E731
        mid = i << 22
        assert pkg.steer_make(g, (mid + (1 << 21)) & 0xffffffff) == at(i + 1)       # the tie goes up
        assert pkg.steer_make(g, (mid - (1 << 21)) & 0xffffffff) == at(i)           # ... so the lower tie belongs to i
        assert pkg.steer_make(g, (mid + (1 << 21) - 1) & 0xffffffff) == at(i)
        assert pkg.steer_make(g, (mid - (1 << 21) + 1) & 0xffffffff) == at(i)
        assert pkg.steer_make(g, (mid - (1 << 21) - 1) & 0xffffffff) == at(i - 1)
        for ph in (mid + (1 << 21), mid - (1 << 21), mid + (1 << 21) - 1, mid - (1 << 21) + 1):
            assert pkg.steer_make(g, ph & 0xffffffff) == tuple(int(v) for v in array_model.steer_make(g, ph & 0xffffffff, C))


def test_steer_make_refuses(pkg):
    lib = pkg.load_library()
    with pytest.raises(pkg.GalSynthError) as ei:
        pkg.steer_make(1024, 0)
    assert ei.value.code == GAL_E_INVAL and "1024" in str(ei.value)
    with pytest.raises(pkg.GalSynthError):
        pkg.steer_make(65535, 0)
    assert lib.gal_synth_steer_make(128, 0, None) == GAL_E_INVAL


def _moddiff(a, b):
    d = (a - b) & 0xffffffff
    return min(d, (1 << 32) - d)


def test_array_phase_against_the_formula(pkg):
    rng = np.random.default_rng(5)
    worst = 0
    for _ in range(2000):
        enu = rng.uniform(-2.0, 2.0, 3)
        az, el = rng.uniform(0.0, 2 * math.pi), rng.uniform(0.0, math.pi / 2)
        worst = max(worst, _moddiff(pkg.array_phase(enu, az, el), array_model.array_phase(enu, az, el)))
    print("largest modular difference to numpy: %d units of 2^-32 cycles" % worst)
    assert worst <= 1  # libm's last place in sin / cos
    for az, el in ((0.0, 0.0), (1.0, 0.5), (4.0, 1.5)):
        assert pkg.array_phase((0.0, 0.0, 0.0), az, el) == 0
        u = np.array([math.sin(az) * math.cos(el), math.cos(az) * math.cos(el), math.sin(el)])
        assert _moddiff(pkg.array_phase(u * LAM / 2, az, el), 1 << 31) <= 1   # half a wavelength towards the source: half a cycle on
        assert _moddiff(pkg.array_phase(u * LAM / 4, az, el), 1 << 30) <= 1   # ... a quarter: the phase ADVANCES
        assert _moddiff(pkg.array_phase(-u * LAM / 4, az, el), 3 << 30) <= 1
        perp = np.cross(u, [0.3, -0.2, 0.9])
        assert _moddiff(pkg.array_phase(perp, az, el), 0) <= 64                # perpendicular: 0 (|perp . u| <= 1e-16 m of rounding)
    # exact cases: a source in the east on the horizon, an element on the north axis; the zenith and an element in the plane
    assert pkg.array_phase((0.0, 0.7, 0.0), math.pi / 2, 0.0) in (0, 1, 0xffffffff)
    assert pkg.array_phase((0.0, 0.0, LAM / 2), 0.3, math.pi / 2) == 1 << 31
    assert pkg.array_phase((LAM / 2, 0.0, 0.0), math.pi / 2, 0.0) == 1 << 31


def test_array_phase_refuses(pkg):
    lib = pkg.load_library()
    inf, nan = float("inf"), float("nan")
    for enu, az, el in (((nan, 0, 0), 0.0, 0.0), ((0, inf, 0), 0.0, 0.0), ((0, 0, -inf), 0.0, 0.0), ((0, 0, 0), nan, 0.0), ((0, 0, 0), 0.0, inf),
                        (None, 0.0, 0.0)):
        with pytest.raises(pkg.GalSynthError) as ei:
            pkg.array_phase(enu, az, el)
        assert ei.value.code == GAL_E_INVAL
    v = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    assert lib.gal_synth_array_phase(v, 0.0, 0.0, None) == GAL_E_INVAL


def test_steer_check_refuses(pkg):
    ok = np.zeros((2, 8, 64, 2), dtype=np.int64)
    ok[..., 0], ok[..., 1] = 32767, -32767
    pkg.steer_check(ok)
    pkg.steer_check(ok[:1, :1, :1])
    for where in ((1, 7, 63, 0), (0, 0, 0, 1)):
        bad = ok.copy()
        bad[where] = -32768
        with pytest.raises(pkg.GalSynthError) as ei:
            pkg.steer_check(bad)
        assert ei.value.code == GAL_E_INVAL and "epoch %d, element %d, part %d" % where[:3] in str(ei.value)
    lib = pkg.load_library()
    rows = np.zeros(2 * 9 * 65, dtype=pkg.STEER_DTYPE)
    for E, K, P in ((1, 0, 1), (1, 9, 1), (1, 1, 0), (1, 1, 65), (0, 1, 1), (1, -1, 1)):
        assert lib.gal_synth_steer_check(rows.ctypes.data, E, K, P) == GAL_E_INVAL, (E, K, P)
    assert lib.gal_synth_steer_check(rows.ctypes.data, 2, 8, 64) == 0
    with pytest.raises(pkg.GalSynthError) as ei:
        pkg.steer_check(None, 1, 1, 1)
    assert ei.value.code == GAL_E_INVAL


def test_the_model_with_unrotated_weights_is_the_weighted_sum():
    """w = (32 g, 0): floor((32 S + 2048) / 4096) = floor((S + 64) / 128), clamps and counts included."""
    rng = np.random.default_rng(9)
    spe, n_epochs, n_parts = 37, 4, 5
    x = rng.integers(-32768, 32768, size=(n_parts, n_epochs * spe * 2), dtype=np.int16)
    for hi in (25, 1023):  # (5 parts x 25 x 32768 / 128 = 32000: no clamp)
        g = rng.integers(0, hi + 1, size=(n_epochs, n_parts))
        w = np.zeros((n_epochs, 1, n_parts, 2), dtype=np.int64)
        w[:, 0, :, 0] = 32 * g
        y, sat = array_model.array(x, w, spe)
        want, want_sat = gain_model.wsum(x, g, spe)
        assert np.array_equal(y[0], want) and sat == want_sat
        assert (sat > 0) == (hi == 1023)
    # a single value in python integers, both rails, a weight that turns
    w = np.array([[[[1234, -777]]]])
    y, _ = array_model.array(np.array([[100, -200]], dtype=np.int16), w, 1)
    assert int(y[0, 0]) == (100 * 1234 - (-200) * (-777) + 2048) >> 12 and int(y[0, 1]) == (100 * (-777) + (-200) * 1234 + 2048) >> 12
    assert not array_model.needs_int64(np.full((1, 1, 1, 2), 32767)) and array_model.needs_int64(np.full((1, 1, 2, 2), 16384))
    assert 32768 * 65535 + 2048 < 1 << 31


def test_struct_layouts(pkg, tmp_path):
    st = pkg.synth._Steer
    assert ctypes.sizeof(st) == 4 and st.w_re.offset == 0 and st.w_im.offset == 2
    f = pkg.STEER_DTYPE.fields
    assert pkg.STEER_DTYPE.itemsize == 4 and f["w_re"][1] == 0 and f["w_im"][1] == 2
    exe = tmp_path / "array_check"
    pkg_dir = os.path.join(ROOT, "galileo-sdr-sim_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "abi_c", "array_check.c"), "-o", str(exe), "-L", pkg_dir, "-lgalsynth", "-lgalscen",
                        "-Wl,-rpath," + pkg_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "array ok" in r.stdout, r.stdout + r.stderr


def _scenario(pkg, **kw):
    return pkg.Scenario(NAV, llh=(-6.0, 51.0, 100.0), start="2022/02/20,12:00:00", duration_s=3.0, iono_enable=False, **kw)


def test_scenario_directions(pkg, capfd):
    sc = _scenario(pkg)
    rows0, gains0 = sc.next_gains(sc.total_epochs)
    capfd.readouterr()
    sc = _scenario(pkg, verbose=True)
    table = capfd.readouterr().err
    rows, gains, azel = sc.next_azel(sc.total_epochs)
    assert rows.tobytes() == rows0.tobytes() and np.array_equal(gains, gains0)
    assert azel.shape == (29, 16, 2) and azel.dtype == np.float64
    active = rows["prn"] > 0
    assert active.any() and not active.all()
    assert not azel[~active].any()
    el, az = azel[..., 1][active], azel[..., 0][active]
    assert el.min() > 0.0 and el.max() <= math.pi / 2
    assert az.min() >= 0.0 and az.max() < 2 * math.pi
    assert len(np.unique(np.round(az, 3))) > 1
    # the table the front-end prints at allocation: PRN, azimuth, elevation in degrees
    printed = {int(m.group(1)): (float(m.group(2)), float(m.group(3))) for m in re.finditer(r"^(\d\d) +(-?[\d.]+) +(-?[\d.]+) +[\d.]+ +[\d.]+$", table, re.M)}
    assert len(printed) == int(active[0].sum()) > 0, table
    for s in np.flatnonzero(active[0]):
        a, e = printed[int(rows["prn"][0, s])]
        assert abs(math.degrees(azel[0, s, 1]) - e) <= 0.1
        assert abs((math.degrees(azel[0, s, 0]) - a + 180.0) % 360.0 - 180.0) <= 0.1
    # without gains: the rows of next(); in two pieces: the same
    sc = _scenario(pkg)
    r1, g1, a1 = sc.next_azel(10, gains=False)
    r2, g2, a2 = sc.next_azel(100, gains=False)
    assert g1 is None and g2 is None
    assert np.concatenate([r1, r2]).tobytes() == rows.tobytes() and np.array_equal(np.concatenate([a1, a2]), azel)
    lib = pkg.scenario.load_library()
    assert lib.gal_scen_next_azel(sc._h, 1, rows.ctypes.data, None, None) == GAL_E_INVAL
