"""The front-end FIR filter without a GPU: the numpy model (tests/fir_model.py) against a naive per-sample loop and its two identities,
gal_synth_fir_check at its bounds, gal_synth_fir_lowpass against the model's double arithmetic."""
import ctypes

import numpy as np
import pytest

import fir_model

GAL_E_INVAL = -1


def _naive(x, taps):
    """y[n] = clamp16((sum_k h[k] x[n - k] + 8192) >> 14) per rail, one sample at a time in Python integers."""
    n = len(x) // 2
    y, sat = [], 0
    for i in range(n):
        for rail in (0, 1):
            a = 0
            for k, h in enumerate(taps):
                if i - k >= 0:
                    a += int(h) * int(x[2 * (i - k) + rail])
            v = (a + 8192) >> 14
            c = min(max(v, -32768), 32767)
            sat += c != v
            y.append(c)
    return np.array(y, dtype=np.int16), sat


@pytest.mark.parametrize("T", [1, 2, 5])
def test_model_against_a_naive_loop(T):
    rng = np.random.default_rng(40 + T)
    x = rng.integers(-32768, 32768, size=2 * 200, dtype=np.int16)
    taps = fir_model.random_taps(rng, T)
    assert fir_model.check(taps) and (T == 1 or np.abs(taps.astype(np.int64)).sum() == 65535)
    x[:16] = 32767 if taps[0] >= 0 else -32768  # eight full-scale samples of the first tap's sign: the clamp fires
    want, want_sat = _naive(x, taps)
    got, sat = fir_model.fir(x, taps)
    assert np.array_equal(got, want) and sat == want_sat and sat > 0
    # any cut with the history handed on gives the same
    cut = 2 * 3
    a, sa = fir_model.fir(x[:cut], taps)
    b, sb = fir_model.fir(x[cut:], taps, history=x[:cut])
    assert np.array_equal(np.concatenate([a, b]), want) and sa + sb == want_sat


def test_model_identities():
    rng = np.random.default_rng(7)
    x = rng.integers(-32768, 32768, size=2 * 300, dtype=np.int16)
    y, sat = fir_model.fir(x, [16384])
    assert np.array_equal(y, x) and sat == 0
    D = 12
    delta = np.zeros(25, dtype=np.int16)
    delta[D] = 16384
    y, sat = fir_model.fir(x, delta)
    assert sat == 0 and not y[: 2 * D].any() and np.array_equal(y[2 * D:], x[: -2 * D])


def _check(lib, taps, n=None):
    t = np.ascontiguousarray(taps, dtype=np.int16)
    return lib.gal_synth_fir_check(t.ctypes.data, len(t) if n is None else n)


def test_fir_check_bounds(pkg):
    lib = pkg.synth.load_library()
    assert _check(lib, [32767, -32768]) == 0  # 65535
    assert _check(lib, [32767, -32768, 0, 0]) == 0
    assert _check(lib, [32767, -32768, 1]) == GAL_E_INVAL  # 65536
    assert b"65535" in lib.gal_synth_last_error()
    assert _check(lib, [16384] + [0] * 127) == 0  # 128 taps
    assert _check(lib, [16384] + [0] * 128) == GAL_E_INVAL  # 129
    assert _check(lib, [16384], n=0) == GAL_E_INVAL
    assert _check(lib, [16384], n=-1) == GAL_E_INVAL
    assert lib.gal_synth_fir_check(None, 1) == GAL_E_INVAL
    # the Python wrapper raises
    pkg.synth.fir_check([16384])
    with pytest.raises(pkg.synth.GalSynthError):
        pkg.synth.fir_check([32767, 32767, 2])
    with pytest.raises(pkg.synth.GalSynthError):
        pkg.synth.fir_check([])


@pytest.mark.parametrize("cutoff,n_taps", [(1.0e6, 63), (1.2e6, 25), (0.5e6, 127), (1.29e6, 3), (2.0e5, 63), (1.023e6, 41)])
def test_fir_lowpass_against_the_model(pkg, cutoff, n_taps):
    fs = 2.6e6
    h = pkg.synth.fir_lowpass(cutoff, fs, n_taps)
    assert h.dtype == np.int16 and h.shape == (n_taps,)
    assert np.array_equal(h, h[::-1])
    assert int(h.astype(np.int64).sum()) == 16384
    pkg.synth.fir_check(h)
    assert fir_model.check(h)
    want = fir_model.lowpass(cutoff, fs, n_taps)
    # libm's and numpy's sin / cos may differ in the last place: a double within an ulp of a rounding tie may round the other way
    assert np.abs(h.astype(np.int64) - want.astype(np.int64)).max() <= 1
    assert int(want.astype(np.int64).sum()) == 16384
    # a low-pass: unity at DC (exact), nearly nothing at the Nyquist frequency for a cutoff well below it
    if cutoff <= 1.0e6 and n_taps >= 25:
        nyq = abs(int((h.astype(np.int64) * (-1) ** np.arange(n_taps)).sum()))
        assert nyq < 16384 // 50


def test_fir_lowpass_refusals(pkg):
    lib = pkg.synth.load_library()
    out = np.zeros(128, dtype=np.int16)
    fs = 2.6e6
    for cutoff, n in ((1.0e6, 62), (1.0e6, 1), (1.0e6, 129), (1.3e6, 63), (2.0e6, 63), (0.0, 63), (-1.0, 63), (float("nan"), 63)):
        assert lib.gal_synth_fir_lowpass(ctypes.c_double(cutoff), ctypes.c_double(fs), n, out.ctypes.data) == GAL_E_INVAL, (cutoff, n)
    assert lib.gal_synth_fir_lowpass(ctypes.c_double(1.0e6), ctypes.c_double(0.0), 63, out.ctypes.data) == GAL_E_INVAL
    assert lib.gal_synth_fir_lowpass(ctypes.c_double(1.0e6), ctypes.c_double(fs), 63, None) == GAL_E_INVAL
    assert not out.any()  # a refused call writes nothing
    with pytest.raises(pkg.synth.GalSynthError):
        pkg.synth.fir_lowpass(1.0e6, fs, 64)


def worst_taps(T, sign):
    """T taps of one sign at the admitted bound: sign -1 gives -32768 first and the rest sharing 32767 (sum |h| = 65535); +1 gives
    32767 first and the rest sharing 32768 (65535 for T >= 3; two non-negative int16 taps reach 65534 only)."""
    first = 32768 if sign < 0 else 32767
    m = np.zeros(T, dtype=np.int64)
    m[0] = first
    rest = min(65535 - first, 32767 * (T - 1))
    m[1:] = rest // (T - 1)
    m[1: 1 + rest - int(m[1:].sum())] += 1
    assert int(m.sum()) == (65535 if T > 2 or sign < 0 else 65534) and m.max() <= first
    return (sign * m).astype(np.int16)


@pytest.mark.parametrize("T", [2, 5, 128])
def test_model_reaches_the_int32_bound_of_the_accumulator(T):
    """The inputs of tests/test_iq_fir_gpu.py::test_aligned_worst_case reach what they claim: every tap negative with the first at
    -32768, every sample -32768 on both rails -- from sample T - 1 on a[n] = 65535 x 32768, and a + 8192 = 2 147 459 072, the bound
    DESIGN.md section 15 states, 24 576 below 2^31.  Every output clamps."""
    n = 1025
    taps = worst_taps(T, -1)
    assert taps[0] == -32768 and (T != 2 or taps[1] == -32767) and (taps <= 0).all() and fir_model.check(taps)
    x = np.full(2 * n, -32768, dtype=np.int16)
    a = np.convolve(x[0::2].astype(np.int64), taps.astype(np.int64))[:n]  # a[n] = sum_k h[k] x[n - k] in int64, zeros in front
    assert int((a + 8192).max()) == 65535 * 32768 + 8192 == 2147459072 < 2 ** 31
    assert (a[T - 1:] == 65535 * 32768).all() and (np.diff(a[:T]) >= 0).all()  # the partial sums only grow towards it
    assert int(taps[0]) * -32768 + int(taps[1]) * -32768 <= 65535 * 32768  # the largest pair of products, one dot product's worth
    y, sat = fir_model.fir(x, taps)
    assert sat == 2 * n and (y == 32767).all()
    # the other sign: all taps >= 0 against +32767, just inside the bound
    pos = worst_taps(T, +1)
    assert (pos >= 0).all() and fir_model.check(pos)
    y, sat = fir_model.fir(np.full(2 * n, 32767, dtype=np.int16), pos)
    assert sat == 2 * n and (y == 32767).all()
