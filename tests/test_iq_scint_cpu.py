"""The ionospheric scintillation without a GPU: the committed shaping table against its formula, the numpy model (tests/scint_model.py)
against python integers and its int32 bounds, the host helpers gal_synth_scint_check / _make against their formulas, and the
statistics of the model's node sequence -- S4, mean power and the autocorrelation of the scattered field."""
import ctypes
import math

import numpy as np
import pytest

import noise_model
import scint_model

FS = 2.6e6
GAL_E_INVAL = -1
S4S = (0.2, 0.5, 0.8, 1.0)


def test_the_table_is_symmetric_and_equals_the_formula(pkg):
    h = pkg.tables()["scint"].astype(np.int64)
    assert h.shape == (32,)
    assert np.array_equal(h, h[::-1])
    assert np.array_equal(h, scint_model.table())
    assert [int(v) for v in h[:16]] == [7, 17, 41, 93, 197, 393, 733, 1287, 2122, 3286, 4782, 6536, 8392, 10123, 11471, 12211]
    assert int(h.sum()) == 123382
    h2 = int(np.sum(h * h))
    print("H2 / 2^30 = %.7f" % (h2 / 2.0 ** 30))
    assert abs(h2 / 2.0 ** 30 - 1.0) < 1e-4
    # the autocorrelation of the table is exp(-k^2 / 64): 1/e at a lag of 8 nodes
    for k in (8, 16):
        assert abs(float(np.sum(h[k:] * h[:-k])) / h2 - math.exp(-k * k / 64.0)) < 2e-3
    # the symbol is exported and the generator writes the committed file
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_tables", os.path.join(root, "tools", "gen_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.scint_table() == [int(v) for v in h]


def test_the_draws_are_philox_words_0_and_1_with_counter_word_3_equal_2():
    seed, stream = 0x1234567890ABCDEF, 7
    for first in (0, 2 ** 40 + 5, 2 ** 58):
        gI, gQ = scint_model.draws(seed, stream, first, 9)
        for k in (0, 8):
            i = first + k
            w = noise_model.philox4x32_10(i & 0xFFFFFFFF, i >> 32, stream, 2, seed & 0xFFFFFFFF, seed >> 32)
            assert int(gI[k]) == int(noise_model.gauss_q12(w[0])[0]) and int(gQ[k]) == int(noise_model.gauss_q12(w[1])[0])
    # not the words of the noise floor (0) or of the oscillator (1)
    for c3 in (0, 1):
        w = noise_model.philox4x32_10(np.arange(9), 0, stream, c3, seed & 0xFFFFFFFF, seed >> 32)
        assert not np.array_equal(noise_model.gauss_q12(w[0]), scint_model.draws(seed, stream, 0, 9)[0])
    assert np.abs(np.concatenate(scint_model.draws(3, 1, 0, 1 << 16))).max() <= 25960


def test_a_node_and_a_sample_in_python_integers():
    r = scint_model.row(seed=99, stream=3, node_len=67, a_q12=2500, b_q12=3000)
    h = [int(v) for v in scint_model.table()]
    first = 2 ** 40 + 5
    j0 = first // 67
    gI, gQ = scint_model.draws(99, 3, j0, 40)
    Z = []
    for j in range(3):
        SI = sum(h[t] * int(gI[j + t]) for t in range(32))
        SQ = sum(h[t] * int(gQ[j + t]) for t in range(32))
        XI, XQ = (SI + 16384) >> 15, (SQ + 16384) >> 15
        Z.append((max(-32767, min(32767, 2500 + ((3000 * XI + 2048) >> 12))), max(-32767, min(32767, (3000 * XQ + 2048) >> 12))))
    zI, zQ = scint_model.factor(r, first, 100)
    R = (1 << 32) // 67
    for k in (0, 1, 50, 66, 67, 99):
        N = first + k
        j, m = N // 67 - j0, N % 67
        fr = (m * R) >> 20
        assert 0 <= fr <= 4095
        assert int(zI[k]) == Z[j][0] + (((Z[j + 1][0] - Z[j][0]) * fr + 2048) >> 12)
        assert int(zQ[k]) == Z[j][1] + (((Z[j + 1][1] - Z[j][1]) * fr + 2048) >> 12)
    # a stream in pieces is the stream
    a = scint_model.factor(r, first, 37)
    b = scint_model.factor(r, first + 37, 63)
    assert np.array_equal(np.concatenate((a[0], b[0])), zI) and np.array_equal(np.concatenate((a[1], b[1])), zQ)


def test_the_identity_row_and_the_int32_bounds():
    rng = np.random.default_rng(1)
    x = rng.integers(-32768, 32768, 2 * 5000, dtype=np.int16)
    x[:4] = (-32768, -32768, 32767, 32767)
    for first in (0, 7, 2 ** 40 + 3):
        y, sat = scint_model.apply(x, scint_model.row(node_len=65), first)
        assert np.array_equal(y, x) and sat == 0
    # |X| < 2^17 at the largest draws; the node clamp bounds every product of the sample step
    hsum = int(scint_model.table().sum())
    assert ((hsum * 25960 + (1 << 14)) >> 15) < 1 << 17
    assert 4096 * (1 << 17) < 1 << 31
    assert 2 * 32768 * 32767 + 2048 < 1 << 31
    assert 2 * 32767 * 4095 + 2048 < 1 << 31
    for L in (64, 65, 1000, 1 << 24):
        assert (L - 1) * ((1 << 32) // L) < 1 << 32 and ((L - 1) * ((1 << 32) // L)) >> 20 <= 4095
    # full scale through a strong Rayleigh row: clamps, counts, never wraps (apply asserts the int32 bound itself)
    r = scint_model.row(node_len=64, a_q12=0, b_q12=4096, seed=5)
    x = np.tile(np.array([-32768, -32768, 32767, 32767, -32768, 32767], dtype=np.int16), 4000)
    y, sat = scint_model.apply(x, r, 0)
    assert 0 < sat < x.size // 2


def test_make_agrees_with_the_model(pkg):
    v = scint_model.x_variance()
    assert abs(v - 1.0) < 1e-3
    for s4 in (0.0, 0.2, 0.5, 0.8, 1.0):
        for tau0, fs in ((0.02, FS), (0.5, FS), (1.0, 4 * FS), (64 * 8 / FS, FS)):
            got = pkg.scint_make(s4, tau0, fs)
            want = scint_model.make(s4, tau0, fs)
            assert got == want, (s4, tau0, fs, got, want)
            assert got["seed"] == 1 and got["stream"] == 0
    assert pkg.scint_make(0.0, 0.5, FS)["a_q12"] == 4096 and pkg.scint_make(0.0, 0.5, FS)["b_q12"] == 0
    ray = pkg.scint_make(1.0, 0.5, FS)
    assert ray["a_q12"] == 0 and ray["b_q12"] == int(math.floor(4096.0 * math.sqrt(1.0 / (2.0 * v)) + 0.5))
    assert pkg.scint_make(0.5, 0.5, FS)["node_len"] == 162500
    # the mean of |z|^2 is 4096^2: A^2 + 2 B^2 v
    for s4 in (0.2, 0.5, 0.8, 1.0):
        r = pkg.scint_make(s4, 0.02, FS)
        assert abs((r["a_q12"] ** 2 + 2 * r["b_q12"] ** 2 * v) / 4096.0 ** 2 - 1.0) < 1e-3


def test_make_and_check_refuse(pkg):
    lib = pkg.load_library()
    inf, nan = float("inf"), float("nan")
    for c in ((nan, 0.5, FS), (0.5, inf, FS), (0.5, 0.5, nan), (-0.01, 0.5, FS), (1.01, 0.5, FS), (0.5, 0.5, 0.0), (0.5, 0.5, -FS),
              (0.5, 63.4 * 8 / FS, FS), (0.5, ((1 << 24) + 1) * 8 / FS, FS), (0.5, -0.5, FS), (0.5, 1e30, FS)):
        with pytest.raises(pkg.GalSynthError) as ei:
            pkg.scint_make(*c)
        assert ei.value.code == GAL_E_INVAL, c
        with pytest.raises(ValueError):
            scint_model.make(*c)
    assert pkg.scint_make(0.5, 64 * 8 / FS, FS)["node_len"] == 64 and pkg.scint_make(0.5, (1 << 24) * 8 / FS, FS)["node_len"] == 1 << 24
    assert lib.gal_synth_scint_make(0.5, 0.5, FS, None) == GAL_E_INVAL
    pkg.scint_check({"node_len": 64, "a_q12": 4096, "b_q12": 4096})
    pkg.scint_check({"node_len": 1 << 24})
    for bad in ({"node_len": 63}, {"node_len": (1 << 24) + 1}, {"a_q12": 4097}, {"b_q12": 4097}):
        with pytest.raises(pkg.GalSynthError) as ei:
            pkg.scint_check(bad)
        assert ei.value.code == GAL_E_INVAL, bad
    r = pkg.synth._scint_struct({})
    r.reserved = 1
    assert lib.gal_synth_scint_check(ctypes.byref(r)) == GAL_E_INVAL
    assert lib.gal_synth_scint_check(None) == GAL_E_INVAL


@pytest.mark.parametrize("s4", S4S)
def test_the_statistics_of_the_node_sequence(s4):
    """2^17 nodes of the integer model with Philox draws, |z|^2 as the power.  A float stand-in of the process over four seeds gave S4
    within 1 % of the request, mean power within 1.6 % of 1, lag-8 autocorrelation 0.365 .. 0.373 (1/e = 0.368) and lag-16 0.019 ..
    0.025 (e^-4 = 0.018); the margins are about three times that spread.  The autocorrelation is that of the scattered field, z minus
    its mean."""
    r = dict(scint_model.make(s4, 0.02, FS), seed=1, stream=0)
    ZI, ZQ = scint_model.nodes(r, 0, 1 << 17)
    z = (ZI.astype(np.float64) + 1j * ZQ.astype(np.float64)) / 4096.0
    p = np.abs(z) ** 2
    got_s4 = float(np.sqrt(p.var()) / p.mean())
    w = z - z.mean()
    den = float(np.sum(np.abs(w) ** 2))
    rho8 = float(np.real(np.sum(w[8:] * np.conj(w[:-8])))) / den
    rho16 = float(np.real(np.sum(w[16:] * np.conj(w[:-16])))) / den
    print("s4 %.1f: S4 %.4f (%+.2f %%), mean power %.4f, rho(8) %.4f, rho(16) %.4f" % (s4, got_s4, 100 * (got_s4 / s4 - 1), p.mean(), rho8, rho16))
    assert abs(got_s4 / s4 - 1.0) < 0.03
    assert abs(p.mean() - 1.0) < 0.03
    assert abs(rho8 - math.exp(-1.0)) < 0.03
    assert rho16 < 0.06
