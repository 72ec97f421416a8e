"""The decimating front-end filter without a GPU: the numpy model (tests/firdec_model.py) against the merged filter's model sampled
every M-th output, gal_synth_firdec_out_samples / _check / _lowpass at their bounds, the int32 bound, the model's physics, and a replay
of k_iq_firdec's index arithmetic (staging into polyphase planes, the host's tap table, the word walk, the history, the output count)
lane by lane in integers against the model."""
import ctypes

import numpy as np
import pytest

import fir_model
import firdec_model

GAL_E_INVAL = -1
# gal_synth_fir_lowpass(1.0e6, 2.6e6, 9) and (1.2e6, 2.6e6, 25) as the library returned them before the decimator existed
PARENT_LOWPASS_9 = [-25, 308, -1400, 2997, 12624, 2997, -1400, 308, -25]
PARENT_LOWPASS_25 = [-8, 21, -49, 102, -189, 311, -466, 643, -826, 998, -1137, 1229, 15126, 1229, -1137, 998, -826, 643, -466, 311, -189, 102, -49,
                     21, -8]
DECIMS = tuple(range(2, 17))


def _fir_any(x, taps):
    """fir_model.fir without its bound of 128 taps (the same arithmetic: used where T > 128)."""
    x = np.asarray(x, dtype=np.int64).reshape(-1, 2)
    h = np.asarray(taps, dtype=np.int64)
    T, n = h.size, x.shape[0]
    s = np.concatenate([np.zeros((T - 1, 2), dtype=np.int64), x])
    a = np.zeros((n, 2), dtype=np.int64)
    for k in range(T):
        a += h[k] * s[T - 1 - k: T - 1 - k + n]
    v = (a + 8192) >> 14
    y = np.clip(v, -32768, 32767)
    return y.astype(np.int16), (y != v)


@pytest.mark.parametrize("M,T", [(2, 1), (2, 3), (3, 128), (4, 127), (5, 7), (8, 64), (16, 15), (16, 17)])
def test_model_is_every_mth_sample_of_the_merged_filter(M, T):
    rng = np.random.default_rng(100 * M + T)
    n = 700
    taps = firdec_model.random_taps(rng, T)
    x = rng.integers(-32768, 32768, size=2 * n, dtype=np.int16)
    x[:32] = 32767 if taps[0] >= 0 else -32768
    full, _ = fir_model.fir(x, taps)
    full = full.reshape(-1, 2)
    v, changed = _fir_any(x, taps)
    assert np.array_equal(v, full)
    for P in (0, 1, M - 1, M, 2 ** 40 + 3):
        i0 = (-P) % M
        got, sat = firdec_model.firdec(x, taps, M, first_sample=P)
        assert np.array_equal(got.reshape(-1, 2), full[i0::M]), (M, T, P)
        assert sat == int(np.count_nonzero(changed[i0::M]))  # the kept outputs' count, nothing else
        if P == 0:
            assert sat > 0
        # any cut with the history handed on gives the same
        for cut in (1, M - 1, M + 1, 333):
            a, sa = firdec_model.firdec(x[: 2 * cut], taps, M, first_sample=P)
            b, sb = firdec_model.firdec(x[2 * cut:], taps, M, first_sample=P + cut, history=x[: 2 * cut])
            assert np.array_equal(np.concatenate([a, b]), got) and sa + sb == sat


@pytest.mark.parametrize("M", DECIMS)
def test_one_unity_tap_is_an_exact_pick_of_every_mth_sample(M):
    """A decimator of the single tap 16384: (16384 x + 8192) >> 14 = x for every int16, so the output is the input at the kept phase --
    the samples whose GLOBAL index is a multiple of M: x[0::M] for a stream that starts at 0 -- and nothing saturates, -32768 and
    32767 included.  The CLI's `--oversample M --fir one_tap.txt` rests on this (tests/test_oversample_cli.py)."""
    rng = np.random.default_rng(40 + M)
    n = 50 * M + 7
    x = rng.integers(-32768, 32768, size=2 * n, dtype=np.int16)
    x[:4] = [-32768, 32767, 32767, -32768]
    x[2 * M: 2 * M + 2] = [32767, -32768]
    xs = x.reshape(-1, 2)
    for P in (0, 1, M - 1, M, 260000, 2 ** 40 + 3):
        got, sat = firdec_model.firdec(x, [16384], M, first_sample=P)
        assert np.array_equal(got.reshape(-1, 2), xs[(-P) % M::M]) and sat == 0, (M, P)
    # a stream from 0 cut anywhere keeps x[0::M]
    a, sa = firdec_model.firdec(x[: 2 * (M + 1)], [16384], M)
    b, sb = firdec_model.firdec(x[2 * (M + 1):], [16384], M, first_sample=M + 1)
    assert np.array_equal(np.concatenate([a, b]).reshape(-1, 2), xs[::M]) and sa + sb == 0


def test_out_samples_against_a_brute_force_count(pkg):
    for M in DECIMS:
        for P in (0, 1, M - 1, M, 2 ** 40 + 3):
            for n in range(0, 3 * M + 1):
                brute = sum(1 for g in range(P, P + n) if g % M == 0)
                assert firdec_model.out_samples(P, n, M) == brute
                assert pkg.synth.firdec_out_samples(P, n, M) == brute, (M, P, n)
    assert pkg.synth.firdec_out_samples(0, 10, 1) == 0 and pkg.synth.firdec_out_samples(0, 10, 17) == 0
    assert pkg.synth.firdec_out_samples(2 ** 64 - 1, 1, 2) == 0  # the sum wraps
    assert pkg.synth.firdec_out_samples(3, 2 ** 41, 16) == 2 ** 37


def _check(lib, taps, M, n=None):
    t = np.ascontiguousarray(taps, dtype=np.int16)
    return lib.gal_synth_firdec_check(t.ctypes.data, len(t) if n is None else n, M)


def test_firdec_check_bounds(pkg):
    lib = pkg.synth.load_library()
    assert _check(lib, [32767, -32768], 2) == 0  # 65535
    assert _check(lib, [32767, -32768, 1], 2) == GAL_E_INVAL  # 65536
    assert b"65535" in lib.gal_synth_last_error()
    assert _check(lib, [16384] + [0] * 511, 16) == 0  # 512 taps
    assert _check(lib, [16384] + [0] * 512, 16) == GAL_E_INVAL  # 513
    assert _check(lib, [16384], 2, n=0) == GAL_E_INVAL
    assert _check(lib, [16384], 1) == GAL_E_INVAL
    assert _check(lib, [16384], 17) == GAL_E_INVAL
    assert _check(lib, [16384], 2) == 0 and _check(lib, [16384], 16) == 0
    assert lib.gal_synth_firdec_check(None, 1, 2) == GAL_E_INVAL
    pkg.synth.firdec_check([16384], 4)
    with pytest.raises(pkg.synth.GalSynthError):
        pkg.synth.firdec_check([32767, 32767, 2], 4)
    with pytest.raises(pkg.synth.GalSynthError):
        pkg.synth.firdec_check([], 4)
    # the merged filter's bound has not moved
    assert pkg.synth.GAL_FIR_MAX_TAPS == 128 and pkg.synth.GAL_FIRDEC_MAX_TAPS == 512 and pkg.synth.GAL_FIRDEC_MAX_DECIM == 16
    with pytest.raises(pkg.synth.GalSynthError):
        pkg.synth.fir_check([16384] + [0] * 128)


@pytest.mark.parametrize("cutoff,rate,n_taps", [(1.17e6, 10.4e6, 3), (1.17e6, 10.4e6, 129), (1.17e6, 39.0e6, 511), (1.0e6, 5.2e6, 63)]
                         + [(1.17e6, M * 2.6e6, 32 * M + 1) for M in range(2, 16)])
def test_firdec_lowpass_against_the_model(pkg, cutoff, rate, n_taps):
    h = pkg.synth.firdec_lowpass(cutoff, rate, n_taps)
    assert h.dtype == np.int16 and h.shape == (n_taps,)
    assert np.array_equal(h, h[::-1])
    assert int(h.astype(np.int64).sum()) == 16384
    pkg.synth.firdec_check(h, 2)
    want = firdec_model.lowpass(cutoff, rate, n_taps)
    # libm's and numpy's sin / cos may differ in the last place: a double within an ulp of a rounding tie may round the other way
    assert np.abs(h.astype(np.int64) - want.astype(np.int64)).max() <= 1
    assert int(want.astype(np.int64).sum()) == 16384


def test_lowpass_refusals_and_the_merged_designer_unchanged(pkg):
    lib = pkg.synth.load_library()
    out = np.zeros(512, dtype=np.int16)
    fs = 10.4e6
    for cutoff, n in ((1.0e6, 62), (1.0e6, 1), (1.0e6, 513), (5.2e6, 63), (6.0e6, 63), (0.0, 63), (-1.0, 63), (float("nan"), 63)):
        assert lib.gal_synth_firdec_lowpass(ctypes.c_double(cutoff), ctypes.c_double(fs), n, out.ctypes.data) == GAL_E_INVAL, (cutoff, n)
    assert lib.gal_synth_firdec_lowpass(ctypes.c_double(1.0e6), ctypes.c_double(0.0), 63, out.ctypes.data) == GAL_E_INVAL
    assert lib.gal_synth_firdec_lowpass(ctypes.c_double(1.0e6), ctypes.c_double(fs), 63, None) == GAL_E_INVAL
    assert not out.any()
    # gal_synth_fir_lowpass: the same taps as the decimator's designer for n <= 127, the model's within its bound, 129 still refused
    for cutoff, n in ((1.0e6, 63), (1.2e6, 25), (0.5e6, 127), (1.29e6, 3)):
        a = pkg.synth.fir_lowpass(cutoff, 2.6e6, n)
        assert np.array_equal(a, pkg.synth.firdec_lowpass(cutoff, 2.6e6, n))
        assert np.abs(a.astype(np.int64) - fir_model.lowpass(cutoff, 2.6e6, n).astype(np.int64)).max() <= 1
    with pytest.raises(pkg.synth.GalSynthError):
        pkg.synth.fir_lowpass(1.0e6, 2.6e6, 129)
    # recorded from the parent commit's library: the merged designer's taps are bit for bit what they were
    assert pkg.synth.fir_lowpass(1.0e6, 2.6e6, 9).tolist() == PARENT_LOWPASS_9
    assert pkg.synth.fir_lowpass(1.2e6, 2.6e6, 25).tolist() == PARENT_LOWPASS_25


def test_model_reaches_the_int32_bound_of_the_accumulator():
    """T = 512, every tap <= 0 with the first at -32768 and sum |h| = 65535, every sample -32768: from input T - 1 on a = 65535 x
    32768 and a + 8192 = 2 147 459 072, 24 576 below 2^31 (tests/test_iq_fir_cpu.py's test of the same name, at the decimator's T)."""
    T, n = 512, 2100
    taps = firdec_model.worst_taps(T)
    assert taps[0] == -32768 and (taps <= 0).all() and firdec_model.check(taps, 4)
    x = np.full(2 * n, -32768, dtype=np.int16)
    a = np.convolve(x[0::2].astype(np.int64), taps.astype(np.int64))[:n]
    assert int((a + 8192).max()) == 65535 * 32768 + 8192 == 2147459072 < 2 ** 31
    assert (a[T - 1:] == 65535 * 32768).all() and (np.diff(a[:T]) >= 0).all()
    for M in (2, 4, 15, 16):
        y, sat = firdec_model.firdec(x, taps, M)
        assert y.size == 2 * firdec_model.out_samples(0, n, M) and (y == 32767).all() and sat == y.size


def test_model_physics_an_out_of_band_tone_comes_out_with_the_filters_gain():
    """M = 4, the default taps (1.17 MHz, 129 taps at 10.4 MS/s).  A complex tone A exp(2 pi i f n / fs) at f outside +-1.3 MHz,
    rounded to int16, filtered and decimated.  With H(f) = sum_k h[k] exp(-2 pi i f k / fs) / 16384 from the QUANTISED taps the ideal
    output is H(f) x the tone at the kept samples (which aliases to f mod 2.6 MHz: a tone of the amplitude |H(f)| A).  The bound per
    rail: the input tone is rounded to integers, an error of at most 0.5 per sample and rail, which the filter can amplify by at most
    sum |h| / 16384; the output is rounded once more, at most 0.5 (round to nearest).  Nothing clamps."""
    M, fs, A = 4, 10.4e6, 20000.0
    h = firdec_model.default_taps(M)
    assert h.size == 32 * M + 1
    hq = h.astype(np.float64) / 16384.0
    bound = 0.5 * float(np.abs(h.astype(np.int64)).sum()) / 16384.0 + 0.5
    assert bound < 1.5
    n = 6000
    k = np.arange(n, dtype=np.float64)
    for f in (1.6e6, 2.0e6, -3.0e6, 4.5e6):
        assert abs(f) > 1.3e6
        z = A * np.exp(2j * np.pi * f * k / fs)
        x = np.empty(2 * n, dtype=np.int16)
        x[0::2] = np.rint(z.real)
        x[1::2] = np.rint(z.imag)
        y, sat = firdec_model.firdec(x, h, M)
        assert sat == 0
        H = np.sum(hq * np.exp(-2j * np.pi * f * np.arange(h.size) / fs))
        m = np.arange(y.size // 2)
        keep = M * m >= h.size - 1  # behind the filter's start-up
        ideal = H * z[M * m]
        err = np.maximum(np.abs(y[0::2] - ideal.real), np.abs(y[1::2] - ideal.imag))[keep]
        assert err.max() <= bound + 1e-6, (f, err.max(), bound)
        amp = np.abs(y[0::2] + 1j * y[1::2])[keep]
        assert abs(amp.mean() - abs(H) * A) <= np.sqrt(2.0) * bound
    # and the filter does what it is for: the 3.0 MHz tone is far down, a tone in band is not
    assert abs(np.sum(hq * np.exp(-2j * np.pi * 3.0e6 * np.arange(h.size) / fs))) < 10 ** (-40 / 20)
    assert abs(np.sum(hq * np.exp(-2j * np.pi * 0.5e6 * np.arange(h.size) / fs))) > 0.99


# ---- k_iq_firdec replayed in integers -----------------------------------------------------------------------------------------------
K_THREADS, K_TILE_IN, K_HIST, K_STAGE = 256, 4096, 512, 4096 + 640


def _table(lib, taps, M):
    """galk_firdec_table of the library (host code): (rows [nb][trips][4] uint32, trips)."""
    t = np.ascontiguousarray(taps, dtype=np.int16)
    tab = np.zeros(640, dtype=np.uint32)
    trips = ctypes.c_int(0)
    words = lib.galk_firdec_table(ctypes.c_void_p(t.ctypes.data), int(t.size), int(M), ctypes.c_void_p(tab.ctypes.data), ctypes.byref(trips))
    nb = min(M, t.size)
    assert words == 4 * nb * trips.value and 0 < words <= 640
    return tab[:words].reshape(nb, trips.value, 4), trips.value


def _s16(w):
    w = np.asarray(w, dtype=np.int64) & 0xffff
    return np.where(w >= 32768, w - 65536, w)


def _dot2(w, g, acc):
    """v_dot2_i32_i16 on packed 32-bit words (int64 arrays / scalars holding uint32)."""
    return acc + _s16(w) * _s16(g) + _s16(np.asarray(w, dtype=np.int64) >> 16) * _s16(int(g) >> 16)


def _replay_call(x32, n, hist_in, i0, tab, trips, T, M):
    """One launch of k_iq_firdec as the file states it: x32 = the call's input as packed uint32 (I low, Q high), hist_in [512] uint32.
    Every LDS and global index is asserted in range.  Returns (out uint32 [n_out], saturated, hist_out)."""
    OB = (K_TILE_IN // M) & ~3
    U = (T - 1) // M
    nb = min(M, T)
    PL = OB + 4 * trips
    inv = (1 << 32) // M + 1
    assert M * PL <= K_STAGE and PL % 4 == 0
    n_out = (n - i0 + M - 1) // M if n > i0 else 0
    blocks = max(1, -(-n_out // OB))
    out = np.zeros(n_out, dtype=np.uint32)
    sat = 0
    for b in range(blocks):
        obase = b * OB
        sI = np.full(K_STAGE, 1 << 40, dtype=np.int64)  # poison: an element read but never staged shows
        sQ = np.full(K_STAGE, 1 << 40, dtype=np.int64)
        lo = i0 + obase * M - (M * U + M - 1)
        lo4 = lo & ~3
        skip, total = lo - lo4, M * PL
        nv = (total + skip + 3) // 4
        for v in range(nv):
            s = lo4 + 4 * v
            a = [0, 0, 0, 0]
            if s < 0:
                if s >= -K_HIST:
                    q = (s + K_HIST) >> 2
                    assert 0 <= q < K_HIST // 4
                    a = [int(c) for c in hist_in[4 * q: 4 * q + 4]]
            elif s + 4 <= n:
                a = [int(c) for c in x32[s: s + 4]]
            else:
                a = [int(x32[s + m]) if s + m < n else 0 for m in range(4)]
            for m in range(4):
                d = 4 * v + m - skip
                if 0 <= d < total:
                    e = (d * inv) >> 32
                    assert e == d // M
                    r = M - 1 - (d - e * M)
                    assert 0 <= r < M and 0 <= e < PL and sI[r * PL + e] == 1 << 40  # written exactly once
                    sI[r * PL + e] = a[m] & 0xffff
                    sQ[r * PL + e] = a[m] >> 16
        assert (sI[:total] != 1 << 40).all()
        groups = np.arange(OB // 4)
        groups = groups[obase + 4 * groups < n_out]
        if groups.size == 0:
            continue
        aI = np.full((4, groups.size), 8192, dtype=np.int64)
        aQ = np.full((4, groups.size), 8192, dtype=np.int64)

        def word(plane, r, u2):  # the uint2 at index g + u2 of plane r: two words of two elements each
            e = r * PL + 4 * (groups + u2)
            assert e.max() + 3 < (r + 1) * PL
            return plane[e] | (plane[e + 1] << 16), plane[e + 2] | (plane[e + 3] << 16)

        for r in range(nb):
            cI, cQ = word(sI, r, 0), word(sQ, r, 0)
            for i in range(trips):
                g = [int(c) for c in tab[r, i]]
                nI, nQ = word(sI, r, i + 1), word(sQ, r, i + 1)
                for acc, c, nx in ((aI, cI, nI), (aQ, cQ, nQ)):
                    acc[0] = _dot2(c[0], g[0], acc[0])
                    acc[1] = _dot2(c[0], g[1], acc[1])
                    acc[2] = _dot2(c[1], g[0], acc[2])
                    acc[3] = _dot2(c[1], g[1], acc[3])
                    acc[0] = _dot2(c[1], g[2], acc[0])
                    acc[1] = _dot2(c[1], g[3], acc[1])
                    acc[2] = _dot2(nx[0], g[2], acc[2])
                    acc[3] = _dot2(nx[0], g[3], acc[3])
                cI, cQ = nI, nQ
        assert np.abs(aI).max() < 2 ** 31 and np.abs(aQ).max() < 2 ** 31
        for m in range(4):
            o = obase + 4 * groups + m
            ok = o < n_out
            vI, vQ = aI[m] >> 14, aQ[m] >> 14
            yI, yQ = np.clip(vI, -32768, 32767), np.clip(vQ, -32768, 32767)
            sat += int(np.count_nonzero((yI != vI)[ok])) + int(np.count_nonzero((yQ != vQ)[ok]))
            out[o[ok]] = ((yI & 0xffff) | ((yQ & 0xffff) << 16))[ok].astype(np.uint32)
    hist_out = np.zeros(K_HIST, dtype=np.uint32)
    for k in range(K_HIST):
        p = n + k
        hist_out[k] = x32[p - K_HIST] if p >= K_HIST else hist_in[p]
    return out, sat, hist_out


REPLAY = [(2, 1), (2, 2), (2, 3), (3, 128), (4, 129), (4, 512), (5, 7), (8, 257), (15, 481), (16, 15), (16, 16), (16, 17), (16, 512), (2, 512)]


@pytest.mark.parametrize("M,T", REPLAY)
def test_kernel_index_arithmetic_replayed_against_the_model(pkg, M, T):
    lib = pkg.synth.load_library()
    rng = np.random.default_rng(7000 + 100 * M + T)
    taps = firdec_model.random_taps(rng, T)
    tab, trips = _table(lib, taps, M)
    tile = firdec_model.tile_inputs(M)
    assert tile == lib.galk_firdec_tile_inputs(M)
    n_all = tile + 700
    x = rng.integers(-32768, 32768, size=2 * n_all, dtype=np.int16)
    x[:32] = 32767 if taps[0] >= 0 else -32768
    x32 = x.view(np.uint32) if x.dtype.byteorder != ">" else None
    for P, cuts in ((0, (n_all,)), (1, (1, M - 1, M, M + 1, 3, 509, tile + 1, None)), (M - 1, (tile - 1, 4 * M + 1, None)),
                    (2 ** 40 + 3, (tile, 511, None))):
        want, want_sat = firdec_model.firdec(x, taps, M, first_sample=P)
        hist = np.zeros(K_HIST, dtype=np.uint32)
        at, phase, outs, sat = 0, P % M, [], 0
        for c in cuts:
            c = n_all - at if c is None else c
            if c == 0:
                continue
            i0 = (M - phase) % M
            o, s, hist = _replay_call(x32[at: at + c], c, hist, i0, tab, trips, T, M)
            assert o.size == firdec_model.out_samples(P + at, c, M)
            outs.append(o)
            sat += s
            at += c
            phase = (phase + c) % M
        assert at == n_all
        got = np.concatenate(outs).view(np.int16)
        assert np.array_equal(got, want), (M, T, P)
        assert sat == want_sat and (P != 0 or sat > 0)
