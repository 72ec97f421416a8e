"""The front-end FIR filter on the MI355X: k_iq_fir against the numpy model (tests/fir_model.py) on random full-range int16 at the
vector, wave and tile edges of its 1024-sample tile, the history across calls (any cut of a stream gives the bytes of one call), the
refusals, and the engine's own output filtered against the model over the oracle's stream."""
import numpy as np
import pytest

import fir_model
from oracle_binding import oracle_run

pytestmark = pytest.mark.gpu

N = 26000
FS = 2.6e6
GAL_E_INVAL, GAL_E_STATE = -1, -4
TAPS = (1, 2, 3, 4, 5, 63, 128)
SIZES = (1, 2, 3, 4, 5, 127, 128, 129, 1023, 1024, 1025, 2049, 4097)  # the kernel's tile is 1024 samples: 1023, 1024, 1025 are its edges
CUTS = (1, 3, 126, 127, 128, 4, 1021, 1024)  # then the rest of the 5000 samples


def _dev(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _empty(n_val):
    import torch

    t = torch.zeros(n_val, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    return t


def _fir_call(eng, x):
    """One gal_synth_iq_fir call over the interleaved int16 x in a buffer of its own (16-byte aligned); (output, saturated values).
    The output buffer is longer than the call and must come back untouched behind it."""
    d_in, d_out = _dev(x), _empty(x.size + 16)
    before = eng.iq_saturated()
    eng.iq_fir(d_in.data_ptr(), x.size // 2, d_out.data_ptr())
    sat = eng.iq_saturated() - before
    got = d_out.cpu().numpy()
    assert not got[x.size:].any(), "the kernel wrote behind the call's last sample"
    return got[: x.size], sat


def _stream_in_cuts(eng, x, cuts):
    out, sat, at = [], 0, 0
    for c in list(cuts) + [x.size // 2 - sum(cuts)]:
        y, s = _fir_call(eng, x[2 * at: 2 * (at + c)])
        out.append(y)
        sat += s
        at += c
    assert at == x.size // 2
    return np.concatenate(out), sat


def _differ(got, want):
    bad = np.flatnonzero(got != want)
    return "%d of %d values differ (first at value %d)" % (bad.size, got.size, bad[0] if bad.size else -1)


@pytest.mark.parametrize("T", TAPS)
def test_kernel_against_the_model(pkg, T):
    rng = np.random.default_rng(9000 + T)
    taps = fir_model.random_taps(rng, T)
    full = rng.integers(-32768, 32768, size=2 * max(SIZES), dtype=np.int16)
    full[:32] = 32767 if taps[0] >= 0 else -32768  # the first 16 samples at full scale, of the first tap's sign: the clamp fires
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        for n in SIZES:
            x = full[: 2 * n]
            want, want_sat = fir_model.fir(x, taps)
            assert want_sat > 0
            eng.fir_set(taps)  # a new stream for every size
            got, sat = _fir_call(eng, x)
            assert np.array_equal(got, want), "T %d, n %d: %s" % (T, n, _differ(got, want))
            assert sat == want_sat, (T, n)
        if T == 1:  # the unity tap: the stream itself, nothing clamped
            eng.fir_set([16384])
            for n in SIZES:
                got, sat = _fir_call(eng, full[: 2 * n])
                assert np.array_equal(got, full[: 2 * n]) and sat == 0, n


@pytest.fixture(scope="module")
def stream():
    """5000 samples of random full-range int16, T = 128 random taps at the admitted bound, and the model's output of ONE call."""
    rng = np.random.default_rng(128)
    taps = fir_model.random_taps(rng, 128)
    x = rng.integers(-32768, 32768, size=2 * 5000, dtype=np.int16)
    x[:32] = 32767 if taps[0] >= 0 else -32768
    want, want_sat = fir_model.fir(x, taps)
    for a in (taps, x, want):
        a.setflags(write=False)
    return taps, x, want, want_sat


def test_any_cut_of_a_stream_gives_the_bytes_of_one_call(pkg, stream):
    taps, x, want, want_sat = stream
    assert want_sat > 0
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        eng.fir_set(taps)
        one, sat_one = _fir_call(eng, x)
        assert np.array_equal(one, want), _differ(one, want)
        assert sat_one == want_sat
        # fir_set again restarts from zero history (without it the call above would be the history of the next)
        eng.fir_set(taps)
        cut, sat_cut = _stream_in_cuts(eng, x, CUTS)
        assert np.array_equal(cut, want), _differ(cut, want)
        assert sat_cut == want_sat
        # not reset: the stream goes on, the history is the end of x
        more, _ = _fir_call(eng, x[: 2 * 300])
        want_more, _ = fir_model.fir(x[: 2 * 300], taps, history=x)
        assert np.array_equal(more, want_more)
        assert not np.array_equal(more, want[: 2 * 300])
        # n_taps = 0 frees the filter
        eng.fir_set(None)
        with pytest.raises(pkg.GalSynthError) as e:
            _fir_call(eng, x[:8])
        assert e.value.code == GAL_E_STATE


def test_pure_delay_across_the_cuts(pkg, stream):
    _, x, _, _ = stream
    D = 12
    delta = np.zeros(25, dtype=np.int16)
    delta[D] = 16384
    want = np.concatenate([np.zeros(2 * D, dtype=np.int16), x[: -2 * D]])
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        eng.fir_set(delta)
        got, sat = _stream_in_cuts(eng, x, CUTS)
    assert np.array_equal(got, want), _differ(got, want)
    assert sat == 0


def test_refusals(pkg, stream):
    taps, x, want, _ = stream
    p = pkg.workloads.make_synthetic(n_epochs=1, n_chan=2, n_slots=16, samples_per_epoch=N, seed=79)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        a, b = _dev(x[: 2 * 1000]), _empty(2 * 1000 + 16)

        def code(fn, *args):
            with pytest.raises(pkg.GalSynthError) as e:
                fn(*args)
            return e.value.code

        assert code(eng.iq_fir, a.data_ptr(), 1000, b.data_ptr()) == GAL_E_STATE  # no filter set
        eng.fir_set(taps)
        assert code(eng.iq_fir, a.data_ptr() + 4, 900, b.data_ptr()) == GAL_E_INVAL  # misaligned input
        assert code(eng.iq_fir, a.data_ptr(), 900, b.data_ptr() + 8) == GAL_E_INVAL  # misaligned output
        assert code(eng.iq_fir, 0, 900, b.data_ptr()) == GAL_E_INVAL
        assert code(eng.iq_fir, a.data_ptr(), 900, 0) == GAL_E_INVAL
        assert code(eng.iq_fir, a.data_ptr(), 1000, a.data_ptr()) == GAL_E_INVAL  # in place
        assert code(eng.iq_fir, a.data_ptr(), 500, a.data_ptr() + 4 * 496) == GAL_E_INVAL  # the output begins inside the input
        assert code(eng.iq_fir, a.data_ptr() + 4 * 496, 500, a.data_ptr()) == GAL_E_INVAL  # the input begins inside the output
        eng.iq_fir(a.data_ptr(), 500, a.data_ptr() + 4 * 500)  # side by side in one buffer is no overlap
        eng.iq_saturated()
        # bad taps leave the filter in force, and its history, as they are
        eng.fir_set(taps)
        first, _ = _fir_call(eng, x[: 2 * 700])
        for bad in ([32767, 32767, 2], [16384] * 129):
            assert code(eng.fir_set, bad) == GAL_E_INVAL
        assert eng._lib.gal_synth_fir_set(eng._h, None, 5) == GAL_E_INVAL
        rest, _ = _fir_call(eng, x[2 * 700: 2 * 1500])
        assert np.array_equal(np.concatenate([first, rest]), want[: 2 * 1500])
        # a buffer of the batch in flight, as input and as output
        iq = _empty(N * 2)
        eng.plan(p)
        eng.execute(iq.data_ptr())
        assert code(eng.iq_fir, iq.data_ptr(), 1000, b.data_ptr()) == GAL_E_STATE
        assert code(eng.iq_fir, a.data_ptr(), 1000, iq.data_ptr() + 4 * 1000) == GAL_E_STATE
        eng.finish()
        eng.iq_fir(iq.data_ptr(), 1000, b.data_ptr())
        eng.iq_saturated()


def test_engine_output_filtered_and_parity_kept(pkg):
    """3 epochs x 26000 samples of the engine, filtered with a 63-tap low-pass: the model over the oracle's stream; the unfiltered
    output of the same handle afterwards is still the oracle's."""
    p = pkg.workloads.make_synthetic(n_epochs=3, n_chan=4, n_slots=16, samples_per_epoch=N, seed=77)
    ref, _ = oracle_run(p, N, FS)
    taps = pkg.synth.fir_lowpass(1.0e6, FS, 63)
    want, want_sat = fir_model.fir(ref, taps)
    assert want_sat == 0 and np.count_nonzero(want != ref) > 0.5 * ref.size
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        iq, out = _empty(3 * N * 2), _empty(3 * N * 2)
        eng.fir_set(taps)
        eng.plan(p)
        eng.execute(iq.data_ptr())
        eng.finish()
        before = eng.iq_saturated()
        # the batch in two calls, cut at an epoch boundary, as a caller with batches of one and two epochs would
        eng.iq_fir(iq.data_ptr(), N, out.data_ptr())
        eng.iq_fir(iq.data_ptr() + 4 * N, 2 * N, out.data_ptr() + 4 * N)
        assert eng.iq_saturated() - before == want_sat
        got = out.cpu().numpy()
        assert np.array_equal(iq.cpu().numpy(), ref)  # the input is only read
        assert np.array_equal(got, want), _differ(got, want)
        plain, _, _ = eng.run_host(p)
        assert np.array_equal(plain, ref)


# ---- the int32 accumulator at its bound, and the tap table at every shape ----------------------------------------------------------
def _worst_taps(T, sign):
    """T taps of one sign at the admitted bound (tests/test_iq_fir_cpu.py: worst_taps, and the witness that they reach it): sign -1
    gives -32768 first and the rest sharing 32767 (sum |h| = 65535); +1 gives 32767 first and the rest sharing 32768 (65535 for
    T >= 3; two non-negative int16 taps reach 65534 only)."""
    first = 32768 if sign < 0 else 32767
    m = np.zeros(T, dtype=np.int64)
    m[0] = first
    rest = min(65535 - first, 32767 * (T - 1))
    m[1:] = rest // (T - 1)
    m[1: 1 + rest - int(m[1:].sum())] += 1
    assert int(m.sum()) == (65535 if T > 2 or sign < 0 else 65534) and m.max() <= first
    return (sign * m).astype(np.int16)


def _one_call_and_cuts(eng, taps, x, cuts):
    want, want_sat = fir_model.fir(x, taps)
    eng.fir_set(taps)
    got, sat = _fir_call(eng, x)
    assert np.array_equal(got, want), "one call: " + _differ(got, want)
    assert sat == want_sat
    eng.fir_set(taps)
    got, sat = _stream_in_cuts(eng, x, cuts)
    assert np.array_equal(got, want), "in cuts: " + _differ(got, want)
    assert sat == want_sat
    return want_sat


@pytest.mark.parametrize("T", [2, 5, 128])
def test_aligned_worst_case(pkg, T):
    """Every product of one sign at full scale: the int32 accumulator (and a single v_dot2_i32_i16, whose two products are the first
    two taps') at a + 8192 = 65535 x 32768 + 8192, 24 576 below 2^31.  Every output clamps and is counted.  1025 samples are one
    tile and one sample; they are cut as the calls of CUTS that fit into them, then the rest."""
    n = 1025
    cuts = CUTS[:6]
    assert sum(cuts) < n < sum(CUTS[:7])
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        neg = _worst_taps(T, -1)
        assert neg[0] == -32768 and (T != 2 or neg[1] == -32767) and (neg <= 0).all()
        assert _one_call_and_cuts(eng, neg, np.full(2 * n, -32768, dtype=np.int16), cuts) == 2 * n
        pos = _worst_taps(T, +1)
        assert (pos >= 0).all()
        assert _one_call_and_cuts(eng, pos, np.full(2 * n, 32767, dtype=np.int16), cuts) == 2 * n


@pytest.mark.parametrize("T", [2, 5, 128])
def test_sign_matched_worst_case(pkg, T):
    """Taps of mixed signs at sum |h| = 65535, the first at -32768, and an input matched to them in sign around a few samples n0:
    on the I rail x[n0 - k] = -32768 sign(h[k]) (as far as an int16 goes: +32767), every product negative; on the Q rail the opposite
    sign, every product positive.  The n0 are the first and the last sample of a tile, the last of a wave and the first of the next
    (samples 255 and 256 of a tile), and sample T - 1, whose window is the stream's first T samples; random full-range int16 elsewhere."""
    n = 3073
    rng = np.random.default_rng(500 + T)
    taps = (_worst_taps(T, -1).astype(np.int64) * np.concatenate([[1], rng.choice([-1, 1], size=T - 1)])).astype(np.int16)
    assert taps[0] == -32768 and int(np.abs(taps.astype(np.int64)).sum()) == 65535 and (T == 2 or ((taps > 0).any() and (taps[1:] < 0).any()))
    x = rng.integers(-32768, 32768, size=(n, 2), dtype=np.int16)
    sgn = np.sign(taps.astype(np.int64))
    centres = (T - 1, 1024, 1024 + 255, 2048 + 256, 2048 + 1023)
    for n0 in centres:
        assert n0 - (T - 1) >= 0
        k = np.arange(T)
        x[n0 - k, 0] = np.clip(-32768 * sgn, -32768, 32767)
        x[n0 - k, 1] = np.clip(32768 * sgn, -32768, 32767)
    assert all(b - (T - 1) > a for a, b in zip(centres, centres[1:]))  # the windows do not overlap
    x = x.reshape(-1)
    want, _ = fir_model.fir(x, taps)
    for n0 in centres:  # far beyond the clamp on both rails, in opposite directions
        assert want[2 * n0] == -32768 and want[2 * n0 + 1] == 32767
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        assert _one_call_and_cuts(eng, taps, x, CUTS) > 0


TABLE_TAPS = (6, 7, 8, 9, 10, 14, 17, 64, 65, 66, 125, 127)
TABLE_SIZES = SIZES


def _table_shape(T):
    """galk_fir_table (csrc/iq_fir.hip), restated: the halo is T - 1 rounded up to a multiple of 4 samples, a trip of the kernel's
    loop takes two tap pairs of the Hs / 2 + 1 there are."""
    Hs = (T - 1 + 3) & ~3
    return Hs, (Hs // 2 + 1 + 1) // 2


@pytest.mark.parametrize("T", TABLE_TAPS)
def test_kernel_against_the_model_at_every_table_shape(pkg, T):
    """test_kernel_against_the_model at the tap counts between its own: T = 2, 3, 0, 1 (mod 4) at halos of 8, 12, 16, 64, 68, 124 and
    128 samples, where the table's zero padding in front of the first tap and behind the last has every length it can have."""
    shapes = [_table_shape(t) for t in TABLE_TAPS]
    assert {hs % 8 for hs, _ in shapes} == {0, 4} and {hs for hs, _ in shapes} == {8, 12, 16, 64, 68, 124, 128}
    assert {trips for _, trips in shapes} == {3, 4, 5, 17, 18, 32, 33}
    assert {t % 4 for t in TABLE_TAPS} == {0, 1, 2, 3}
    assert [_table_shape(t) for t in TAPS] == [(0, 1), (4, 2), (4, 2), (4, 2), (4, 2), (64, 17), (128, 33)]  # what the first test reaches
    rng = np.random.default_rng(9000 + T)
    taps = fir_model.random_taps(rng, T)
    full = rng.integers(-32768, 32768, size=2 * max(TABLE_SIZES), dtype=np.int16)
    full[:32] = 32767 if taps[0] >= 0 else -32768  # the first 16 samples at full scale, of the first tap's sign: the clamp fires
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        for n in TABLE_SIZES:
            x = full[: 2 * n]
            want, want_sat = fir_model.fir(x, taps)
            assert want_sat > 0
            eng.fir_set(taps)  # a new stream for every size
            got, sat = _fir_call(eng, x)
            assert np.array_equal(got, want), "T %d, n %d: %s" % (T, n, _differ(got, want))
            assert sat == want_sat, (T, n)
