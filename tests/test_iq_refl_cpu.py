"""Geometric reflectors without a GPU: the numpy model's own invariants (tests/refl_model.py), the interpolation's bound and the int32
rule as arithmetic, the host-only entry points gal_synth_refl_check / _geom / _row, the ctypes layout, and the physics of one echo with
a fractional delay on the CPU: the correlator model over a one-satellite oracle stream against the superposition of the echo-free
correlations."""
import ctypes
import math

import numpy as np
import pytest

import corr_model
import mpath_model
import refl_model
from oracle_binding import oracle_run

GAL_E_INVAL = -1


@pytest.fixture(scope="module")
def cos1024(pkg):
    return pkg.tables()["cos1024"]


def _parts(rng, n_parts, n_epochs, spe, lim=32768):
    return rng.integers(-lim, lim, size=(n_parts, n_epochs * spe * 2), dtype=np.int16)


def _random_rows(rng, n_epochs, n_echo, frac=True):
    r = refl_model.rows(n_epochs, n_echo)
    r["gain_q7"] = rng.integers(0, 400, size=r.shape)
    r["delay"] = rng.choice((0, 1, 3, 4, 5, 255, 1023), size=r.shape)
    r["ph0"] = rng.integers(0, 1 << 32, size=r.shape, dtype=np.uint64)
    r["dph"] = rng.integers(-(1 << 20), 1 << 20, size=r.shape)
    if frac:
        r["frac_q12"] = rng.choice((0, 1, 2047, 2048, 4095), size=r.shape)
    return r


# ---- the model's own invariants ------------------------------------------------------------------------------------------------------
def test_frac_0_is_the_echo_pass(pkg, cos1024):
    """Rows with F = 0 are gal_iq_echo_t rows byte for byte, and the model gives mpath_model's bytes, count and history -- the delay of
    1024 included, which only F = 0 may have."""
    rng = np.random.default_rng(1)
    spe, n_epochs = 37, 40
    x = _parts(rng, 3, n_epochs, spe)
    g = rng.integers(0, 2000, size=(n_epochs, 3))
    r = _random_rows(rng, n_epochs, 4, frac=False)
    r["delay"][:, 3] = 1024
    e = mpath_model.rows(n_epochs, 4, r["gain_q7"], r["delay"], r["ph0"], r["dph"])
    assert e.tobytes() == r.tobytes() and np.array_equal(refl_model.from_echo(e), r)
    pkg.refl_check(r.astype(pkg.REFL_DTYPE), [0, 1, 2, 2], 3)
    hist = _parts(rng, 3, 1, 1024)
    want = mpath_model.mpath(x, g, spe, [0, 1, 2, 2], e, cos1024, hist)
    got = refl_model.refl(x, g, spe, [0, 1, 2, 2], r, cos1024, hist)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] > 0 and np.array_equal(got[2], want[2])
    # no echo at all: the weighted sum (mpath_model's own test ties that to gain_model)
    got = refl_model.refl(x, g, spe, [], refl_model.rows(n_epochs, 0), cos1024, hist)
    want = mpath_model.mpath(x, g, spe, [], mpath_model.rows(n_epochs, 0), cos1024, hist)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]


def test_u_lies_between_a_and_b():
    """For every F, on random full-range pairs and on the four corners: min(a, b) <= u <= max(a, b) per rail, so |u| <= 32768, and
    |F (b - a)| < 2^28.  F = 2048 between neighbours is the mean rounded up; F = 4095 falls one short of b only where |b - a| > 2048."""
    rng = np.random.default_rng(2)
    spe = 4096
    x = _parts(rng, 1, 2, spe)
    x[0, :8] = [-32768, 32767, 32767, -32768, -32768, -32768, 32767, 32767]
    for F in (1, 2, 2047, 2048, 2049, 4094, 4095):
        r = refl_model.rows(2, 1, 128, 0, 0, 0, F)
        u, a, b = refl_model.interpolate(x[0], np.zeros(2048, np.int16), r[:, 0], spe)
        assert (u >= np.minimum(a, b)).all() and (u <= np.maximum(a, b)).all() and np.abs(u).max() <= 32768
        assert np.array_equal(u, a + ((F * (b - a) + 2048) >> 12))
    assert 4095 * 65535 < 1 << 28
    # the exhaustive statement of the bound: every difference d = b - a of two int16 and every F
    d = np.arange(-65535, 65536, dtype=np.int64)[None, :]
    t = (np.arange(4096, dtype=np.int64)[:, None] * d + 2048) >> 12
    assert (np.sign(t) * np.sign(d) >= 0).all() and (np.abs(t) <= np.abs(d)).all()
    # a pure fractional delay at phase 0: y[n] = mean of x[n - 1] and x[n - 2], rounded as the definition says
    r = refl_model.rows(2, 1, 128, 1, 0, 0, 2048)
    y, sat, _ = refl_model.refl(x, np.zeros((2, 1), np.int64), spe, [0], r, np.asarray(_unit_table()))
    xa = np.concatenate([np.zeros(4, np.int64), x[0].astype(np.int64)])
    a, b = xa[2:-2], xa[:-4]
    assert sat == 0 and np.array_equal(y, a + ((2048 * (b - a) + 2048) >> 12))


def _unit_table():
    """A table with C[0] = 4096 and C[-256] = 0 is all the phase 0 needs: r = u exactly."""
    t = np.zeros(1024, dtype=np.int64)
    t[0] = 4096
    return t


def test_both_accumulator_widths_agree_at_the_bound(pkg, cos1024):
    """Rows with sum g + 2 sum A = 65535 (the last the int32 accumulator takes) and 65536, on parts at -32768 and at +32767 and F > 0:
    u stays at the level, so the worst case of the echo pass is reached and the rule carries over -- w formed in an int32 gives the
    int64 bytes at 65535, and |w| + 64 reaches 2^31 one row further."""
    spe, n_epochs = 50, 3
    r = refl_model.rows(n_epochs, 2, [[100, 200]], [[0, 3]], [[5 << 29, 7 << 29], [1 << 29, 3 << 29], [0, 1 << 31]], 0, [[4095, 1]])
    for level in (-32768, 32767):
        x = np.full((2, n_epochs * spe * 2), level, dtype=np.int16)
        hist = np.full((2, 2048), level, dtype=np.int16)
        for extra in (0, 1):
            g = np.tile([32767, 32168 + extra], (n_epochs, 1))
            assert refl_model.needs_int64(g, r) == bool(extra)
            wide = refl_model.refl(x, g, spe, [0, 1], r, cos1024, hist)
            assert wide[1] == x.shape[1]  # every value clamps
            if not extra:
                narrow = refl_model.refl(x, g, spe, [0, 1], r, cos1024, hist, acc=np.int32)
                assert np.array_equal(narrow[0], wide[0]) and narrow[1] == wide[1]
    assert 65535 * 32768 + 64 < 2 ** 31 <= 65536 * 32768


# ---- host-only entry points --------------------------------------------------------------------------------------------------------
def test_refl_row_layout(pkg):
    from galileo_sdr_sim_amd import synth

    names = ("gain_q7", "delay", "ph0", "dph", "frac_q12", "reserved")
    assert ctypes.sizeof(synth._Refl) == 16 and synth.REFL_DTYPE.itemsize == 16 and pkg.REFL_DTYPE == refl_model.REFL_DTYPE
    assert [synth.REFL_DTYPE.fields[k][1] for k in names] == [0, 2, 4, 8, 12, 14]
    assert [getattr(synth._Refl, k).offset for k in names] == [0, 2, 4, 8, 12, 14]
    assert (synth.GAL_REFL_GROUND, synth.GAL_REFL_WALL) == (refl_model.GROUND, refl_model.WALL) == (0, 1)


def _refused(fn, *args, **kw):
    from galileo_sdr_sim_amd import synth

    with pytest.raises(synth.GalSynthError) as e:
        fn(*args, **kw)
    assert e.value.code == GAL_E_INVAL
    return str(e.value)


def test_refl_check(pkg):
    ok = refl_model.rows(3, 2, 32767, [[1023, 1024]], 0xffffffff, -(1 << 31), [[4095, 0]])
    pkg.refl_check(ok, [0, 63], 64)
    pkg.refl_check(refl_model.rows(3, 0), [], 1)
    pkg.refl_check(refl_model.rows(1, 32), [0] * 32, 1)
    assert "33 echoes" in _refused(pkg.refl_check, refl_model.rows(1, 33), [0] * 33, 1)
    assert "part 2" in _refused(pkg.refl_check, ok, [0, 2], 2)
    assert "n_parts 65" in _refused(pkg.refl_check, ok, [0, 0], 65)
    for fields, text in (({"frac_q12": 4096}, "frac_q12 4096 of epoch 1, echo 0"), ({"delay": 1024, "frac_q12": 1}, "delay 1024 + 1/4096 of epoch 1, echo 0"),
                         ({"reserved": 1}, "reserved = 1 in epoch 1, echo 0"), ({"gain_q7": 32768}, "gain 32768 of epoch 1, echo 0"),
                         ({"delay": 1025, "frac_q12": 0}, "delay 1025 + 0/4096")):
        bad = ok.copy()
        for k, v in fields.items():
            bad[k][1, 0] = v
        assert text in _refused(pkg.refl_check, bad, [0, 1], 2)
    lib = pkg.load_library()
    pof = np.zeros(2, dtype=np.int32)
    assert lib.gal_synth_refl_check(ok.ctypes.data, 2, 0, pof.ctypes.data, 2) == GAL_E_INVAL
    assert lib.gal_synth_refl_check(None, 2, 3, pof.ctypes.data, 2) == GAL_E_INVAL
    assert lib.gal_synth_refl_check(None, 0, 3, None, 2) == 0


def test_refl_geom(pkg):
    rad = math.radians
    G, W = refl_model.GROUND, refl_model.WALL
    assert pkg.refl_geom(G, [2.0], rad(123.0), rad(30.0)) == pytest.approx(2.0, abs=1e-12)  # 2 h sin(el)
    assert pkg.refl_geom(G, [2.0], 0.0, rad(90.0)) == 4.0
    assert pkg.refl_geom(G, [0.0], 0.0, rad(45.0)) == 0.0  # an antenna on the ground: an echo with no excess path
    assert pkg.refl_geom(G, [2.0], 0.0, 0.0) == -1.0 and pkg.refl_geom(G, [2.0], 0.0, rad(-5.0)) == -1.0
    # a wall 20 m to the north: a satellite in the south at the horizon sees the full 40 m, one in the north none
    assert pkg.refl_geom(W, [20.0, 0.0], rad(180.0), 0.0) == pytest.approx(40.0, abs=1e-12)
    assert pkg.refl_geom(W, [20.0, 0.0], rad(180.0), rad(60.0)) == pytest.approx(20.0, abs=1e-12)
    assert pkg.refl_geom(W, [20.0, 0.0], rad(10.0), rad(20.0)) == -1.0
    assert pkg.refl_geom(W, [20.0, 0.0], rad(90.0), rad(20.0)) == -1.0  # along the wall (cos = 6e-17: not > 0 after the sign)
    assert pkg.refl_geom(W, [20.0, rad(90.0)], rad(300.0), rad(20.0)) == pytest.approx(-40.0 * math.cos(rad(20.0)) * math.cos(rad(210.0)), abs=1e-12)
    rng = np.random.default_rng(5)
    for _ in range(200):
        kind = int(rng.integers(0, 2))
        p = [float(rng.uniform(0, 60)), float(rng.uniform(-7, 7))]
        az, el = float(rng.uniform(-7, 7)), float(rng.uniform(-0.2, 1.6))
        assert pkg.refl_geom(kind, p, az, el) == refl_model.geom(kind, p, az, el)
    assert "kind 2" in _refused(pkg.refl_geom, 2, [1.0], 0.0, 0.5)
    for bad in (([-1.0], 0.0, 0.5), ([float("nan")], 0.0, 0.5), ([1.0], float("inf"), 0.5), ([1.0], 0.0, float("nan"))):
        assert "must be finite" in _refused(pkg.refl_geom, refl_model.GROUND, *bad)
    assert "must be finite" in _refused(pkg.refl_geom, W, [1.0, float("nan")], 0.0, 0.5)
    lib = pkg.load_library()
    assert lib.gal_synth_refl_geom(0, None, 0.0, 0.5, ctypes.byref(ctypes.c_double())) == GAL_E_INVAL


def test_refl_row(pkg):
    fs, N, c = 10.4e6, 10400, 299792458.0
    rng = np.random.default_rng(6)
    for _ in range(300):
        now, nxt = float(rng.uniform(0, 200)), float(rng.uniform(0, 200))
        args = (now, nxt, float(rng.uniform(-30, 6)), float(rng.uniform(-400, 400)), fs, N, int(rng.integers(0, 32768)))
        assert tuple(pkg.refl_row(*args).tolist()) == refl_model.row(*args), args
    # D and F: 3.5 samples; the carry at F = 4096 (t = D + 4095.6 / 4096 rounds up into D + 1, F = 0)
    r = pkg.refl_row(3.5 * c / fs, 3.5 * c / fs, -6.0, 180.0, fs, N, 128)
    assert (int(r["delay"]), int(r["frac_q12"]), int(r["gain_q7"]), int(r["dph"]), int(r["reserved"])) == (3, 2048, 64, 0, 0)
    t = 7 + 4095.6 / 4096
    r = pkg.refl_row(t * c / fs, 0.0, 0.0, 0.0, fs, N, 128)
    assert (int(r["delay"]), int(r["frac_q12"])) == (8, 0) and refl_model.row(t * c / fs, 0.0, 0.0, 0.0, fs, N, 128)[1::3] == (8, 0)
    r = pkg.refl_row((7 + 4095.4 / 4096) * c / fs, 0.0, 0.0, 0.0, fs, N, 128)
    assert (int(r["delay"]), int(r["frac_q12"])) == (7, 4095)
    # no excess path: D = F = 0, and the phase is the reflection's own
    r = pkg.refl_row(0.0, 0.0, -6.0, 180.0, fs, N, 128)
    assert (int(r["delay"]), int(r["frac_q12"]), int(r["ph0"]), int(r["dph"])) == (0, 0, 1 << 31, 0)
    # one wavelength more path: the same phase; a quarter more: -90 degrees
    lam = refl_model.LAMBDA
    assert abs(int(pkg.refl_row(5 * lam, 0.0, 0.0, 0.0, fs, N, 128)["ph0"]) - (1 << 32)) % (1 << 32) < 64
    assert abs(int(pkg.refl_row(5.25 * lam, 0.0, 0.0, 0.0, fs, N, 128)["ph0"]) - (3 << 30)) < 64
    # the range: 1024 samples exactly is the last delay, anything beyond it needs sample n - 1025
    assert (int(pkg.refl_row(1024 * c / fs, 0.0, 0.0, 0.0, fs, N, 128)["delay"])) == 1024
    assert "more than 1024" in _refused(pkg.refl_row, 1024.01 * c / fs, 0.0, 0.0, 0.0, fs, N, 128)
    assert "more than 1024" in _refused(pkg.refl_row, 1e9, 0.0, 0.0, 0.0, fs, N, 128)
    assert "more than 2" in _refused(pkg.refl_row, 1.0, 1.0, 6.03, 0.0, fs, N, 128)
    for bad in ((float("nan"), 0, 0, 0, fs, N, 128), (0, float("inf"), 0, 0, fs, N, 128), (0, 0, 0, 0, 0.0, N, 128), (0, 0, 0, 0, fs, 0, 128),
                (0, 0, 0, 0, fs, N, 32768)):
        assert "must be finite" in _refused(pkg.refl_row, *bad)
    # no echo now: the zero row whatever else; none in the next epoch: the phase stands still
    assert not any(pkg.refl_row(-1.0, 5.0, -6.0, 180.0, fs, N, 128).tolist())
    assert int(pkg.refl_row(5.0, -1.0, -6.0, 180.0, fs, N, 128)["dph"]) == 0


def test_refl_row_phase_runs_from_epoch_to_epoch(pkg):
    """A ground bounce under a 2 m mast while the satellite climbs 0.005 degrees per 4 ms epoch (far faster than any does): the excess
    path changes by fractions of a wavelength per epoch, and ph0[e] + N dph[e] meets ph0[e + 1] to within N / 2 units of 2^-32 cycle
    (the rounding of dph) -- the phase is continuous without a free fade parameter.  A step of more than half a cycle would alias:
    the wrapped difference is the shortest way round."""
    fs, N = 2.6e6, 10400
    el = math.radians(20.0) + math.radians(0.005) * np.arange(40)
    x = [pkg.refl_geom(refl_model.GROUND, [2.0], 1.0, float(e)) for e in el]
    rows = [pkg.refl_row(x[e], x[e + 1], -6.0, 180.0, fs, N, 128) for e in range(39)]
    ph0 = np.array([int(r["ph0"]) for r in rows], dtype=np.int64)
    dph = np.array([int(r["dph"]) for r in rows], dtype=np.int64)
    assert np.abs(dph).min() > 0
    err = (ph0[:-1] + N * dph[:-1] - ph0[1:]) % (1 << 32)
    err = np.where(err >= 1 << 31, err - (1 << 32), err)
    assert np.abs(err).max() <= N // 2
    # against the geometry itself: the phase falls by (x[e + 1] - x[e]) / lambda cycles per epoch
    want = -(np.diff(x) / refl_model.LAMBDA) * 4294967296.0 / N
    assert np.abs(dph - want).max() <= 1.0 and np.abs(want).max() * N < 0.5 * 4294967296.0


def test_compute_entry_points_refuse_a_null_handle(pkg):
    lib = pkg.load_library()
    assert lib.gal_synth_iq_refl(None, None, 1, None, None, 1, None, None, 0, None) == GAL_E_INVAL
    assert lib.gal_synth_run_refl(None, None, 1, None, None, None, None, 0, None, None) == GAL_E_INVAL
    assert lib.gal_synth_run_refl(None, None, 1, None, None, None, None, 1, None, None) == GAL_E_INVAL


# ---- one echo with a fractional delay, despread ----------------------------------------------------------------------------------------
# Measured on the CPU model (this test prints it): the largest |S_with_echo - superposition| over the whole periods and the delays
# 0 .. 4 half chips, relative to the direct prompt |S|.  As in test_iq_mpath_cpu it comes from the few samples at each period edge that
# the delayed stream carries over from the neighbouring period, the roundings of u, r and y, and the replica's 512-entry carrier table.
# DESIGN.md section 23 quotes it next to section 18's 5.07e-4.
REFL_RESIDUAL_MEASURED = 3.2e-4  # 3.198e-4 as printed


def test_one_fractional_echo_is_the_superposition_of_the_neighbouring_correlations(pkg, cos1024):
    """One satellite from the oracle at 4.092 MS/s (two samples per half chip) plus one echo at D = 3, F = 2048 -- 3.5 samples --,
    alpha = 0.5, phase 90 degrees, despread by the correlator model over three whole periods at the delays 0 .. 4 half chips.

    The echo is u[n] = (x[n - 3] + x[n - 4]) / 2.  x[n - 4] lags by two half chips: S_direct(k - 2).  x[n - 3] lags by one and a half:
    on every second sample its half chip is that of lag 1, on the others that of lag 2, so it correlates as (S_direct(k - 1) +
    S_direct(k - 2)) / 2 -- the correlation of a sample-held stream is piecewise linear between the lags.  Each tap carries the
    carrier rotation of its own delay.  Hence
        S(k) = S_direct(k) + alpha e^{j theta} (1/4 r3 S_direct(k - 1) + (1/4 r3 + 1/2 r4) S_direct(k - 2)),  rD = e^{-j 2 pi f_carr D / fs}:
    the correlation function of the echo sits at 1.75 half chips = 3.5 samples, moved by exactly the fraction.  (Equal weights on
    S_direct(k - 1) and S_direct(k - 2) would be an echo at 3 samples; against that sum this stream differs by 0.2 of the prompt,
    which the test prints and asserts to be large: the fraction is visible.)"""
    fs, N, n_epochs, D, F = 4.092e6, 40920, 2, 3, 2048
    p = pkg.workloads.make_synthetic(n_epochs=n_epochs, n_chan=1, n_slots=16, samples_per_epoch=N, sample_rate=fs, prns=[11], seed=18)
    x, _ = oracle_run(p, N, fs)
    row = pkg.refl_row(3.5 * 299792458.0 / fs, 3.5 * 299792458.0 / fs, 20 * math.log10(0.5), 90.0 + 360.0 * 3.5 * 1575.42e6 / fs, fs, N, 128)
    assert (int(row["delay"]), int(row["frac_q12"]), int(row["gain_q7"]), int(row["dph"])) == (D, F, 64, 0)
    rows = refl_model.rows(n_epochs, 1, 64, D, 1 << 30, 0, F)  # theta = 90 degrees exactly
    assert abs(int(row["ph0"]) - (1 << 30)) < 1 << 12  # (the geometry's phase, with the path's own turn taken out again, is that theta)
    g = np.full((n_epochs, 1), 128)
    y, sat, _ = refl_model.refl(x[None, :], g, N, [0], rows, cos1024)
    assert sat == 0
    T = pkg.tables()
    q = pkg.corr_from_epoch(p[0, 0], fs, 0, max_periods=5, delay0=-2, n_delay=7)
    Sx = corr_model.correlate(x, q, T)[1:4].astype(np.float64)  # whole periods only; delays -2 .. 4
    Sy = corr_model.correlate(y, dict(q, delay0=0, n_delay=5), T)[1:4].astype(np.float64)  # delays 0 .. 4
    cx = np.stack([Sx[..., 0] + 1j * Sx[..., 1], Sx[..., 2] + 1j * Sx[..., 3]], axis=-1)  # [m, d, k, (B, C)]
    cy = np.stack([Sy[..., 0] + 1j * Sy[..., 1], Sy[..., 2] + 1j * Sy[..., 3]], axis=-1)
    f_carr = float(p["f_carr"][0, 0])
    rot = lambda d: 0.5 * np.exp(1j * (math.pi / 2 - 2 * math.pi * f_carr * d / fs))  # noqa: E731
    k1, k2 = cx[:, :, 1:6], cx[:, :, 0:5]  # S_direct(k - 1), S_direct(k - 2)
    want = cx[:, :, 2:7] + 0.25 * rot(3) * k1 + (0.25 * rot(3) + 0.5 * rot(4)) * k2
    prompt = np.abs(cx[:, 0, 2, 0]).min()
    assert prompt > 0.9 * 16368 * 250 ** 2 * 0.95
    residual = np.abs(cy - want).max() / prompt
    effect = np.abs(cy - cx[:, :, 2:7]).max() / prompt
    whole = np.abs(cy - (cx[:, :, 2:7] + rot(3) * 0.5 * (k1 + k2))).max() / prompt
    print("reflector residual %.3e of the prompt correlation; the echo itself moves the sums by %.3f of it; against an echo at 3 samples "
          "(equal weights on the two neighbours) %.3f" % (residual, effect, whole))
    assert effect > 0.3
    assert whole > 0.1  # half a sample of delay is no rounding effect
    assert residual <= 3 * REFL_RESIDUAL_MEASURED
