"""The host paths the stages of the output chain share (csrc/iq_api.cpp), on the MI355X: set / unset / set again, the scratch and the
tables growing while the call before is still on the device, and gal_synth_destroy with every stage's kernels just enqueued.  Expected
bytes and saturation counts are the numpy models' (osc_model, agc_model, fir_model, firdec_model, gain_model, mpath_model)."""
import ctypes

import numpy as np
import pytest

import agc_model
import fir_model
import firdec_model
import gain_model
import mpath_model
import osc_model

pytestmark = pytest.mark.gpu

N = 40  # samples per epoch of the handles here (the weighted sums' epochs)
GAL_E_STATE = -4
T = osc_model.TILE
OSC = dict(p0=0x3333333344444444, f=round(1234.5 / 2.6e6 * 2 ** 64), d=round(5.0e4 / 2.6e6 / 2.6e6 * 2 ** 64), s=int(1e-4 * 2 ** 52),
           seed=0x1234567890ABCDEF, stream=7)
OSC_FIRST = 2 ** 40 + 3
AGC = agc_model.params(agc_model.GAL_AGC_MIN_BLOCK, 2, 9000 * 256, p_init=2 * agc_model.GAL_AGC_MIN_BLOCK * 3000 ** 2)
DECIM = 3
SEEDS = {"fir": 22, "firdec": 23, "agc": 24, "osc": 25}


def _dev(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _empty(n_bytes):
    return _dev(np.zeros(n_bytes + 16, dtype=np.uint8))


def _input(seed, n, amp=32767):
    return np.random.default_rng(seed).integers(-amp, amp + 1, 2 * n, dtype=np.int16)


def _bytes(t, n_bytes):
    return t.cpu().numpy().view(np.uint8)[:n_bytes]


def _i16(a):
    return np.ascontiguousarray(a).view(np.uint8)


class _Stage:
    """One stage as case (a) sees it: set(), unset(), call(device input, samples, device output), the model of a whole stream."""

    def __init__(self, name, n, who, message):
        self.name, self.n, self.who, self.message = name, n, who, message
        self.x = _input(SEEDS[name], n)

    def out_bytes(self, n_done, n):
        """bytes a call of n samples writes, n_done samples of the stream behind it"""
        if self.name == "firdec":
            return 4 * firdec_model.out_samples(n_done, n, DECIM)
        return 4 * n


def _stage(name):
    rng = np.random.default_rng(21)
    if name == "fir":
        s = _Stage(name, T + 5, "gal_synth_iq_fir", "no filter set (call gal_synth_fir_set first)")
        taps = fir_model.random_taps(rng, 33)
        s.set = lambda eng: eng.fir_set(taps)
        s.unset = lambda eng: eng.fir_set(None)
        s.call = lambda eng, i, n, o: eng.iq_fir(i, n, o)
        y, sat = fir_model.fir(s.x, taps)
    elif name == "firdec":
        s = _Stage(name, firdec_model.tile_inputs(DECIM) + 5, "gal_synth_iq_firdec", "no decimator set (call gal_synth_firdec_set first)")
        taps = firdec_model.random_taps(rng, 40)
        s.set = lambda eng: eng.firdec_set(taps, DECIM, 0)
        s.unset = lambda eng: eng.firdec_set(None)
        s.call = lambda eng, i, n, o: eng.iq_firdec(i, n, o)
        y, sat = firdec_model.firdec(s.x, taps, DECIM)
    elif name == "agc":
        s = _Stage(name, T + 5, "gal_synth_iq_agc", "no AGC set (call gal_synth_agc_set first)")
        s.set = lambda eng: eng.agc_set(AGC, 0)
        s.unset = lambda eng: eng.agc_set(None)
        s.call = lambda eng, i, n, o: eng.iq_agc(i, n, "ishort", 0, o)
        y, _, sat = agc_model.agc(s.x, AGC, 0, "ishort", 0)
    else:
        s = _Stage(name, T + 5, "gal_synth_iq_osc", "no oscillator set (call gal_synth_osc_set first)")
        o = osc_model.osc(**OSC)
        s.set = lambda eng: eng.osc_set(o, OSC_FIRST)
        s.unset = lambda eng: eng.osc_set(None)
        s.call = lambda eng, i, n, o_: eng.iq_osc(i, n, o_)
        y, sat, _ = osc_model.rotate(s.x, o, OSC_FIRST, OSC_FIRST)
    s.want, s.want_sat = _i16(y), int(sat)
    return s


def _run_cuts(eng, s, cuts):
    """The stage's stream in calls of the lengths `cuts`: (bytes, saturated)."""
    before = eng.iq_saturated()
    got, at = [], 0
    for c in cuts:
        d_in = _dev(s.x[2 * at: 2 * (at + c)])
        nb = s.out_bytes(at, c)
        d_out = _empty(nb)
        s.call(eng, d_in.data_ptr(), c, d_out.data_ptr())
        eng.iq_saturated()
        got.append(_bytes(d_out, nb))
        at += c
    return np.concatenate(got), eng.iq_saturated() - before


@pytest.mark.parametrize("name", ["fir", "firdec", "agc", "osc"])
def test_set_unset_set_again(pkg, name):
    """(a) A stage that was unset refuses its pass with GAL_E_STATE and its message; set again, it starts a new stream, and that stream
    in two calls -- a tile, then the five samples behind it -- is the model bit for bit."""
    s = _stage(name)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        s.set(eng)
        got, sat = _run_cuts(eng, s, [s.n])
        assert np.array_equal(got, s.want) and sat == s.want_sat
        s.unset(eng)
        d_in, d_out = _dev(s.x), _empty(4 * s.n)
        with pytest.raises(pkg.GalSynthError) as err:
            s.call(eng, d_in.data_ptr(), s.n, d_out.data_ptr())
        assert err.value.code == GAL_E_STATE
        assert str(err.value).endswith("%s: %s" % (s.who, s.message)), str(err.value)
        s.unset(eng)  # (unsetting twice is fine)
        s.set(eng)
        got, sat = _run_cuts(eng, s, [s.n - 5, 5])
        bad = np.flatnonzero(got != s.want)
        assert bad.size == 0, "%s: %d bytes differ, first at %d" % (name, bad.size, bad[0])
        assert sat == s.want_sat


def _two_calls_no_sync(eng, call, x, n1, out_bytes1, out_bytes2):
    """Two calls back to back: every buffer is on the device before the first, nothing waits between them."""
    n = x.size // 2
    d1, d2 = _dev(x[: 2 * n1]), _dev(x[2 * n1:])
    o1, o2 = _empty(out_bytes1), _empty(out_bytes2)
    before = eng.iq_saturated()
    call(d1.data_ptr(), n1, o1.data_ptr())
    call(d2.data_ptr(), n - n1, o2.data_ptr())
    sat = eng.iq_saturated() - before
    return np.concatenate((_bytes(o1, out_bytes1), _bytes(o2, out_bytes2))), sat


def test_osc_scratch_grows_under_the_call_before(pkg):
    """(b) Phase noise: a call of one tile (scratch 12 bytes, capacity 12 + 3 + 256), then at once one of 40 tiles and 3 samples, whose
    492 bytes do not fit: the host must wait for the first call's kernels before it frees their scratch."""
    n1, n2 = T, 40 * T + 3
    assert 12 * ((n2 + T - 1) // T) > 12 + 12 // 4 + 256
    x = _input(31, n1 + n2)
    o = osc_model.osc(**OSC)
    want, want_sat, _ = osc_model.rotate(x, o, OSC_FIRST, OSC_FIRST)
    assert want_sat > 0
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        eng.osc_set(o, OSC_FIRST)
        got, sat = _two_calls_no_sync(eng, eng.iq_osc, x, n1, 4 * n1, 4 * n2)
    assert np.array_equal(got, _i16(want)) and sat == want_sat


def test_agc_scratch_grows_under_the_call_before(pkg):
    """(b) The smallest block length, 16: a call of one block (scratch 12 + 4 bytes, capacity 16 + 4 + 256), then at once one that
    touches 24 blocks (292 bytes)."""
    B = AGC["block_len"]
    n1, n2 = B, 23 * B + 3
    assert 12 * ((n2 - 1) // B + 1) + 4 > 16 + 16 // 4 + 256
    x = _input(32, n1 + n2)
    want, _, want_sat = agc_model.agc(x, AGC, 0, "ishort", 0)
    assert want_sat > 0
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        eng.agc_set(AGC, 0)
        got, sat = _two_calls_no_sync(eng, lambda i, n, o: eng.iq_agc(i, n, "ishort", 0, o), x, n1, 4 * n1, 4 * n2)
    assert np.array_equal(got, want) and sat == want_sat


# (c) 1 epoch of 1 part, then at once 3 epochs of 3 parts (and 2 echoes): the sizes of the issue, which the first table's headroom of a
# quarter still holds; then 200 epochs, which it does not -- the host waits for the kernel that reads the old table, frees it and makes a
# larger one
SHAPES = ((1, 1, 0), (3, 3, 2), (200, 3, 2))


def test_wsum_table_grows_under_the_call_before(pkg):
    rng = np.random.default_rng(33)
    calls = []
    for n_epochs, n_parts, _ in SHAPES:
        parts = rng.integers(-32768, 32768, size=(n_parts, n_epochs * N * 2), dtype=np.int16)
        gains = rng.integers(0, 200, size=(n_epochs, n_parts))
        calls.append((parts, gains) + gain_model.wsum(parts, gains, N))
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        devs = [([_dev(p) for p in parts], _empty(want.size * 2)) for parts, _, want, _ in calls]
        before = eng.iq_saturated()
        for (parts, gains, _, _), (d_parts, d_out) in zip(calls, devs):
            eng.iq_wsum([d.data_ptr() for d in d_parts], gains, d_out.data_ptr())
        sat = eng.iq_saturated() - before
        for (_, _, want, _), (_, d_out) in zip(calls, devs):
            assert np.array_equal(_bytes(d_out, want.size * 2), _i16(want))
    assert sat == sum(int(c[3]) for c in calls) > 0


def test_mpath_table_grows_under_the_call_before(pkg):
    rng = np.random.default_rng(34)
    lines = mpath_model.Lines(pkg.tables()["cos1024"])
    calls = []
    for n_epochs, n_parts, n_echo in SHAPES:
        parts = rng.integers(-32768, 32768, size=(n_parts, n_epochs * N * 2), dtype=np.int16)
        gains = rng.integers(0, 200, size=(n_epochs, n_parts))
        pof = [k % n_parts for k in range(n_echo)]
        rows = mpath_model.rows(n_epochs, n_echo, gain_q7=rng.integers(1, 100, size=(n_epochs, n_echo)), delay=rng.integers(0, 1025, size=(n_epochs, n_echo)),
                                ph0=rng.integers(0, 2 ** 32, size=(n_epochs, n_echo)), dph=rng.integers(-2 ** 20, 2 ** 20, size=(n_epochs, n_echo)))
        want, want_sat = lines.call(parts, gains, N, pof, rows)[:2]
        calls.append((parts, gains, pof, rows, want, want_sat))
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        devs = [([_dev(p) for p in c[0]], _empty(c[4].size * 2)) for c in calls]
        before = eng.iq_saturated()
        for (parts, gains, pof, rows, _, _), (d_parts, d_out) in zip(calls, devs):
            eng.iq_mpath([d.data_ptr() for d in d_parts], gains, d_out.data_ptr(), pof, rows)
        sat = eng.iq_saturated() - before
        for c, (_, d_out) in zip(calls, devs):
            assert np.array_equal(_bytes(d_out, c[4].size * 2), _i16(c[4]))
    assert sat == sum(int(c[5]) for c in calls) > 0


def test_destroy_with_every_stage_enqueued(pkg):
    """(d) Every stage set and a kernel of each just enqueued: gal_synth_destroy returns GAL_OK, and a fresh handle gives case (a)'s
    oscillator bytes."""
    stages = [_stage(name) for name in ("fir", "firdec", "agc", "osc")]
    parts = np.stack([_input(41, 2 * N), _input(42, 2 * N)])
    gains = np.full((2, 2), 100)
    rows = mpath_model.rows(2, 1, gain_q7=50, delay=7, ph0=12345, dph=678)
    eng = pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0)
    bufs = [(_dev(s.x), _empty(4 * s.n)) for s in stages]
    d_parts, d_sum, d_echo = [_dev(p) for p in parts], _empty(8 * N), _empty(8 * N)
    for s in stages:
        s.set(eng)
    for s, (d_in, d_out) in zip(stages, bufs):
        s.call(eng, d_in.data_ptr(), s.n, d_out.data_ptr())
    eng.iq_wsum([d.data_ptr() for d in d_parts], gains, d_sum.data_ptr())
    eng.iq_mpath([d.data_ptr() for d in d_parts], gains, d_echo.data_ptr(), [1], rows)
    rc = eng._lib.gal_synth_destroy(eng._h)
    eng._h = ctypes.c_void_p()
    assert rc == 0
    osc = stages[3]
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as fresh:
        osc.set(fresh)
        got, sat = _run_cuts(fresh, osc, [osc.n])
    assert np.array_equal(got, osc.want) and sat == osc.want_sat
