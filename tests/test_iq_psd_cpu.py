"""The Welch power spectrum (include/galsynth.h: gal_synth_iq_psd) without a GPU: the numpy model of the integer transform
(tests/psd_model.py) against a float64 FFT of the same windowed integers, the library's table, gal_synth_psd_segments and the layout of
gal_iq_psd_t."""
import ctypes
import math

import numpy as np
import pytest

import psd_model


def _inputs(n):
    """[3, n] complex int16 segments as (re, im): random full-range, full-scale DC, a full-scale tone at 45 degrees of phase"""
    rng = np.random.default_rng(n)
    k = np.arange(n)
    ph = 2.0 * np.pi * (n // 8 + 1) * k / n + np.pi / 4
    re = np.stack([rng.integers(-32768, 32768, n), np.full(n, -32768), np.rint(32767 * np.cos(ph)).astype(np.int64)])
    im = np.stack([rng.integers(-32768, 32768, n), np.full(n, -32768), np.rint(32767 * np.sin(ph)).astype(np.int64)])
    return re.astype(np.int64), im.astype(np.int64)


@pytest.mark.parametrize("kind", (0, 1))
@pytest.mark.parametrize("log2_n", (3, 6, 10, 12))
def test_model_against_a_float_fft(log2_n, kind):
    """max |dX| <= sqrt(N) log2 N (8.5, 48, 320, 768): log2 N stages, each rounding every value once by at most 0.5 + the table's 2^-31
    relative error, the errors of a stage adding in power over the N / 2 butterflies that feed a bin.  Found on these inputs: 0.67, 3.3, 18, 40 (on other draws up to 0.7, 3.7, 35, 140).  No
    intermediate value leaves int32 (transform() asserts it at every stage); the largest met stays below 2^27.5."""
    n = 1 << log2_n
    re, im = _inputs(n)
    win = psd_model.window(log2_n, kind)
    xr, xi = (re * win + (1 << 14)) >> 15, (im * win + (1 << 14)) >> 15
    seen = [0]
    yr, yi = psd_model.transform(xr, xi, seen)
    ref = np.fft.fft(xr.astype(np.float64) + 1j * xi.astype(np.float64), axis=1)
    err = float(np.abs(ref - (yr + 1j * yi)).max())
    print("N = %d window %d: max |dX| = %.3f, largest value 2^%.2f" % (n, kind, err, math.log2(seen[0])))
    assert err <= math.sqrt(n) * log2_n
    assert seen[0] <= 2 ** 27.5 * 1.0001
    if kind == 0:  # full-scale DC: X[0] = -N 32768 on both rails, exactly, and nothing else
        assert yr[1, 0] == -n * 32768 and yi[1, 0] == -n * 32768 and not yr[1, 1:].any() and not yi[1, 1:].any()


def test_table_and_window(pkg):
    t = pkg.tables()["psd"]
    k = np.arange(4096)
    assert t.shape == (2, 4096) and t.dtype == np.int32
    assert np.array_equal(t[0], np.rint(2.0 ** 30 * np.cos(2 * np.pi * k / 4096)).astype(np.int64))
    assert np.array_equal(t[1], np.rint(2.0 ** 30 * np.sin(2 * np.pi * k / 4096)).astype(np.int64))
    assert np.array_equal(t[0], psd_model.C) and np.array_equal(t[1], psd_model.S)
    for log2_n in range(3, 13):
        n = 1 << log2_n
        w = ((1 << 30) - t[0].astype(np.int64)[np.arange(n) * (4096 // n)]) >> 16
        assert w[0] == 0 and w[n // 2] == 32768 and w.min() == 0 and w.max() == 32768
        assert np.array_equal(w, psd_model.window(log2_n, 1))
        assert np.array_equal(w[1:], w[1:][::-1])  # periodic Hann: symmetric about N / 2


def test_psd_segments(pkg):
    seg = pkg.psd_segments
    for log2_n, hop, n in ((3, 1, 100), (3, 8, 100), (10, 512, 260000), (10, 1024, 260000), (12, 2048, 260000), (6, 17, 5000)):
        N = 1 << log2_n
        assert seg(log2_n, hop, 1, n) == (n - N) // hop + 1 == psd_model.segments(log2_n, hop, n)
    for log2_n, hop in ((3, 3), (10, 512), (12, 4096)):
        N = 1 << log2_n
        assert seg(log2_n, hop, 0, N - 1) == 0
        assert seg(log2_n, hop, 0, N) == 1
        assert seg(log2_n, hop, 0, N + hop - 1) == 1
        assert seg(log2_n, hop, 0, N + hop) == 2
        # the bound: n_seg N^2 = 2^32 exactly is accepted, one segment more is not
        most = (1 << 32) >> (2 * log2_n)
        assert seg(log2_n, hop, 0, N + (most - 1) * hop) == most
        assert seg(log2_n, hop, 0, N + most * hop - 1) == most
        assert seg(log2_n, hop, 0, N + most * hop) == 0
    assert seg(12, 4096, 0, 4096 * 256) == 256 and seg(12, 4096, 0, 4096 * 257) == 0
    # every field out of range
    assert seg(10, 512, 1, 260000) == 506
    for bad in ((2, 4, 0, 0), (13, 4, 0, 0), (-1, 4, 0, 0), (10, 0, 0, 0), (10, -1, 0, 0), (10, 1025, 0, 0), (10, 512, 2, 0), (10, 512, -1, 0),
                (10, 512, 1, 1), (10, 512, 1, -1)):
        assert seg(bad[0], bad[1], bad[2], 260000, reserved=bad[3]) == 0, bad
    assert pkg.load_library().gal_synth_psd_segments(None, 260000) == 0


def test_struct_layout(pkg):
    P = pkg.synth._Psd
    assert ctypes.sizeof(P) == 16
    assert [getattr(P, f).offset for f in ("log2_n", "hop", "window", "reserved")] == [0, 4, 8, 12]
    assert all(getattr(P, f).size == 4 for f in ("log2_n", "hop", "window", "reserved"))
