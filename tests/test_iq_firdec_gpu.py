"""The decimating front-end filter on the MI355X: k_iq_firdec against the numpy model (tests/firdec_model.py) on random full-range
int16 at the edges of its tile, at every alignment of the stream to the decimation; against the merged kernel's output [::M]; the
history across calls (any cut of the input stream gives the bytes of one call); the int32 bound; the refusals; and the engine's own
oversampled output decimated against the model over the oracle's stream."""
import numpy as np
import pytest

import firdec_model
from oracle_binding import oracle_run

pytestmark = pytest.mark.gpu

N = 26000
FS = 2.6e6
GAL_E_INVAL, GAL_E_STATE = -1, -4
SHAPES = [(2, 1), (2, 2), (2, 3), (3, 128), (4, 129), (4, 512), (5, 7), (8, 257), (15, 481), (16, 15), (16, 16), (16, 17), (16, 512)]
SENTINEL = 0x5a5a


def TILE_INPUTS(M):
    """The input samples one block of k_iq_firdec filters (csrc/iq_firdec.hip: (kTileIn / M) & ~3 outputs of M inputs each)."""
    return firdec_model.tile_inputs(M)


def _sizes(M):
    t = TILE_INPUTS(M)
    return sorted({1, M - 1, M, M + 1, 4 * M - 1, 4 * M, 4 * M + 1, t - 1, t, t + 1, 2 * t + 1})


def _firsts(M):
    return (0, 1, M - 1, 2 ** 40 + 3)


def _dev(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _empty(n_val, fill=SENTINEL):
    import torch

    t = torch.full((n_val,), fill, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    return t


def _call(eng, x, expect_out):
    """One gal_synth_iq_firdec call over the interleaved int16 x in a buffer of its own; (output, saturated values).  The output
    buffer is 16 values longer than the outputs and must come back untouched behind them."""
    d_in, d_out = _dev(x), _empty(2 * expect_out + 16)
    before = eng.iq_saturated()
    n_out = eng.iq_firdec(d_in.data_ptr(), x.size // 2, d_out.data_ptr())
    sat = eng.iq_saturated() - before
    assert n_out == expect_out
    got = d_out.cpu().numpy()
    assert (got[2 * n_out:] == SENTINEL).all(), "the kernel wrote behind the call's last output"
    return got[: 2 * n_out], sat


def _stream_in_cuts(eng, x, cuts, M, P):
    out, sat, at = [], 0, 0
    for c in list(cuts) + [x.size // 2 - sum(cuts)]:
        y, s = _call(eng, x[2 * at: 2 * (at + c)], firdec_model.out_samples(P + at, c, M))
        out.append(y)
        sat += s
        at += c
    assert at == x.size // 2
    return np.concatenate(out), sat


def _differ(got, want):
    bad = np.flatnonzero(got != want)
    return "%d of %d values differ (first at value %d)" % (bad.size, got.size, bad[0] if bad.size else -1)


@pytest.mark.parametrize("M,T", SHAPES)
def test_kernel_against_the_model(pkg, M, T):
    rng = np.random.default_rng(9000 + 100 * M + T)
    taps = firdec_model.random_taps(rng, T)
    sizes = _sizes(M)
    full = rng.integers(-32768, 32768, size=2 * max(sizes), dtype=np.int16)
    full[: 2 * (2 * M + 2)] = 32767 if taps[0] >= 0 else -32768  # the first samples at full scale, of the first tap's sign: the clamp fires
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        for P in _firsts(M):
            for n in sizes:
                x = full[: 2 * n]
                want, want_sat = firdec_model.firdec(x, taps, M, first_sample=P)
                assert want_sat > 0 or P != 0  # at the stream's start the first output is h[0] x a full-scale sample: it clamps
                eng.firdec_set(taps, M, P)  # a new stream for every size
                got, sat = _call(eng, x, want.size // 2)
                assert np.array_equal(got, want), "M %d, T %d, P %d, n %d: %s" % (M, T, P, n, _differ(got, want))
                assert sat == want_sat, (M, T, P, n)


@pytest.mark.parametrize("M", [2, 3, 4])
def test_cross_check_with_the_merged_kernel(pkg, M):
    """The decimator's output is gal_synth_iq_fir's output [::M] on the same device input."""
    n = 2 * TILE_INPUTS(M) + 1
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        for T in (3, 63, 128):
            rng = np.random.default_rng(300 + 10 * M + T)
            taps = firdec_model.random_taps(rng, T)
            x = rng.integers(-32768, 32768, size=2 * n, dtype=np.int16)
            d_in, d_full, d_dec = _dev(x), _empty(2 * n), _empty(2 * n)
            eng.fir_set(taps)
            eng.firdec_set(taps, M)
            eng.iq_fir(d_in.data_ptr(), n, d_full.data_ptr())
            n_out = eng.iq_firdec(d_in.data_ptr(), n, d_dec.data_ptr())
            eng.iq_saturated()
            assert n_out == (n + M - 1) // M
            full = d_full.cpu().numpy().reshape(-1, 2)
            dec = d_dec.cpu().numpy()[: 2 * n_out].reshape(-1, 2)
            assert np.array_equal(dec, full[::M]), (M, T)


@pytest.fixture(scope="module")
def streams():
    """Per (M, T): 20 000 samples of random full-range int16, random taps at the admitted bound, the model's output of ONE call."""
    out = {}
    for M, T in ((4, 512), (15, 481)):
        rng = np.random.default_rng(1000 * M + T)
        taps = firdec_model.random_taps(rng, T)
        x = rng.integers(-32768, 32768, size=2 * 20000, dtype=np.int16)
        x[:64] = 32767 if taps[0] >= 0 else -32768
        want, want_sat = firdec_model.firdec(x, taps, M)
        for a in (taps, x, want):
            a.setflags(write=False)
        out[(M, T)] = (taps, x, want, want_sat)
    return out


@pytest.mark.parametrize("M,T", [(4, 512), (15, 481)])
def test_any_cut_of_a_stream_gives_the_bytes_of_one_call(pkg, streams, M, T):
    taps, x, want, want_sat = streams[(M, T)]
    cuts = (1, 3, M - 1, M, M + 1, 510, 511, 512, 4, 1021, 4096)
    assert want_sat > 0
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        eng.firdec_set(taps, M)
        one, sat_one = _call(eng, x, want.size // 2)
        assert np.array_equal(one, want), _differ(one, want)
        assert sat_one == want_sat
        # firdec_set again restarts the stream
        eng.firdec_set(taps, M)
        cut, sat_cut = _stream_in_cuts(eng, x, cuts, M, 0)
        assert cut.size == want.size  # the per-call n_out sum to the single call's
        assert np.array_equal(cut, want), _differ(cut, want)
        assert sat_cut == want_sat
        # not reset: the stream goes on, the history is the end of x and the position 20 000
        more, _ = _call(eng, x[: 2 * 300], firdec_model.out_samples(20000, 300, M))
        want_more, _ = firdec_model.firdec(x[: 2 * 300], taps, M, first_sample=20000, history=x)
        assert np.array_equal(more, want_more)
        # n_taps = 0 frees the decimator
        eng.firdec_set(None)
        with pytest.raises(pkg.GalSynthError) as e:
            eng.iq_firdec(_dev(x[:8]).data_ptr(), 4, _empty(16).data_ptr())
        assert e.value.code == GAL_E_STATE


@pytest.mark.parametrize("M", [2, 4, 15, 16])
def test_aligned_worst_case_of_the_int32_bound(pkg, M):
    """T = 512, every tap <= 0 with the first at -32768, sum |h| = 65535, every sample -32768: a + 8192 = 65535 x 32768 + 8192, 24 576
    below 2^31 (tests/test_iq_firdec_cpu.py shows the model reaches it).  Every output clamps and is counted, in one call and in cuts."""
    T = 512
    taps = firdec_model.worst_taps(T)
    n = TILE_INPUTS(M) + 600
    x = np.full(2 * n, -32768, dtype=np.int16)
    want, want_sat = firdec_model.firdec(x, taps, M)
    assert want_sat == want.size and (want == 32767).all()
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        eng.firdec_set(taps, M)
        got, sat = _call(eng, x, want.size // 2)
        assert np.array_equal(got, want) and sat == want_sat
        eng.firdec_set(taps, M)
        got, sat = _stream_in_cuts(eng, x, (1, 3, 511, 512, 1021), M, 0)
        assert np.array_equal(got, want) and sat == want_sat


def test_unity_tap_and_pure_delay(pkg, streams):
    _, x, _, _ = streams[(4, 512)]
    xs = x.reshape(-1, 2)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        for M in (2, 3, 4, 16):
            for P in (0, 1):
                i0 = (-P) % M
                eng.firdec_set([16384], M, P)
                got, sat = _call(eng, x, firdec_model.out_samples(P, 20000, M))
                assert np.array_equal(got.reshape(-1, 2), xs[i0::M]) and sat == 0, (M, P)
            D = 4 * M + 3
            delta = np.zeros(D + 5, dtype=np.int16)
            delta[D] = 16384
            delayed = np.concatenate([np.zeros((D, 2), dtype=np.int16), xs[:-D]])
            eng.firdec_set(delta, M)
            got, sat = _stream_in_cuts(eng, x, (1, 3, 511, 4096), M, 0)
            assert np.array_equal(got.reshape(-1, 2), delayed[::M]) and sat == 0, M


def test_refusals(pkg, streams):
    taps, x, want, _ = streams[(4, 512)]
    M = 4
    p = pkg.workloads.make_synthetic(n_epochs=1, n_chan=2, n_slots=16, samples_per_epoch=N, seed=79)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        a, b = _dev(x[: 2 * 1000]), _empty(2 * 1000 + 16)
        lib, h = eng._lib, eng._h
        import ctypes

        def code(fn, *args):
            with pytest.raises(pkg.GalSynthError) as e:
                fn(*args)
            return e.value.code

        n_out = ctypes.c_size_t(0)
        assert code(eng.iq_firdec, a.data_ptr(), 1000, b.data_ptr()) == GAL_E_STATE  # no decimator set
        eng.firdec_set(taps, M)
        assert lib.gal_synth_iq_firdec(None, ctypes.c_void_p(a.data_ptr()), 900, ctypes.c_void_p(b.data_ptr()), ctypes.byref(n_out)) == GAL_E_INVAL
        assert lib.gal_synth_iq_firdec(h, ctypes.c_void_p(a.data_ptr()), 900, ctypes.c_void_p(b.data_ptr()), None) == GAL_E_INVAL  # null n_out
        assert lib.gal_synth_firdec_set(None, ctypes.c_void_p(taps.ctypes.data), 512, M, 0) == GAL_E_INVAL
        assert code(eng.iq_firdec, a.data_ptr() + 4, 900, b.data_ptr()) == GAL_E_INVAL  # misaligned input
        assert code(eng.iq_firdec, a.data_ptr(), 900, b.data_ptr() + 8) == GAL_E_INVAL  # misaligned output
        assert code(eng.iq_firdec, 0, 900, b.data_ptr()) == GAL_E_INVAL
        assert code(eng.iq_firdec, a.data_ptr(), 900, 0) == GAL_E_INVAL
        assert code(eng.iq_firdec, a.data_ptr(), 1000, a.data_ptr()) == GAL_E_INVAL  # in place
        assert code(eng.iq_firdec, a.data_ptr(), 500, a.data_ptr() + 4 * 496) == GAL_E_INVAL  # the output begins inside the input
        assert code(eng.iq_firdec, a.data_ptr() + 4 * 100, 500, a.data_ptr()) == GAL_E_INVAL  # 125 outputs from a: they reach the input
        assert code(eng.iq_firdec, a.data_ptr(), 2 ** 41, b.data_ptr()) == GAL_E_INVAL
        assert eng.iq_firdec(a.data_ptr(), 500, a.data_ptr() + 4 * 500) == 125  # side by side in one buffer is no overlap
        eng.iq_saturated()
        # bad taps and decimations leave the decimator in force, its history and its position as they are
        eng.firdec_set(taps, M)
        first, _ = _call(eng, x[: 2 * 701], firdec_model.out_samples(0, 701, M))
        for bad, m in (([32767, 32767, 2], M), ([16384] * 513, M), (taps, 1), (taps, 17)):
            assert code(eng.firdec_set, bad, m) == GAL_E_INVAL
        assert lib.gal_synth_firdec_set(h, None, 5, M, 0) == GAL_E_INVAL
        rest, _ = _call(eng, x[2 * 701: 2 * 1500], firdec_model.out_samples(701, 799, M))
        assert np.array_equal(np.concatenate([first, rest]), want[: 2 * 375])
        # the merged filter's slot is independent: setting and freeing it leaves the decimator's stream alone
        eng.fir_set([16384])
        eng.fir_set(None)
        more, _ = _call(eng, x[2 * 1500: 2 * 2300], 200)
        assert np.array_equal(more, want[2 * 375: 2 * 575])
        # a buffer of the batch in flight, as input and as output
        iq = _empty(N * 2, fill=0)
        eng.plan(p)
        eng.execute(iq.data_ptr())
        assert code(eng.iq_firdec, iq.data_ptr(), 1000, b.data_ptr()) == GAL_E_STATE
        assert code(eng.iq_firdec, a.data_ptr(), 1000, iq.data_ptr() + 4 * 1000) == GAL_E_STATE
        eng.finish()
        eng.iq_firdec(iq.data_ptr(), 1000, b.data_ptr())
        eng.iq_saturated()


@pytest.mark.parametrize("M", [3, 4])
def test_engine_output_decimated_and_parity_kept(pkg, M):
    """3 epochs x M x 26000 samples of the engine at M x 2.6 MS/s, decimated with the default taps: the model over the oracle's stream
    at that rate; the plain output of the same handle afterwards is still the oracle's."""
    n = M * N
    p = pkg.workloads.make_synthetic(n_epochs=3, n_chan=4, n_slots=16, samples_per_epoch=n, sample_rate=M * FS, seed=77)
    ref, _ = oracle_run(p, n, M * FS)
    taps = pkg.synth.firdec_lowpass(0.45 * FS, M * FS, 32 * M + 1)
    assert np.abs(taps.astype(np.int64) - firdec_model.default_taps(M).astype(np.int64)).max() <= 1
    want, want_sat = firdec_model.firdec(ref, taps, M)
    assert want_sat == 0 and want.size == 2 * 3 * N
    with pkg.SynthEngine(samples_per_epoch=n, n_slots=16, device=0, sample_rate=M * FS) as eng:
        iq, out = _empty(3 * n * 2, fill=0), _empty(3 * N * 2)
        eng.firdec_set(taps, M)
        eng.plan(p)
        eng.execute(iq.data_ptr())
        eng.finish()
        before = eng.iq_saturated()
        # the batch in two calls, cut at an epoch boundary, as a caller with batches of one and two epochs would
        assert eng.iq_firdec(iq.data_ptr(), n, out.data_ptr()) == N
        assert eng.iq_firdec(iq.data_ptr() + 4 * n, 2 * n, out.data_ptr() + 4 * N) == 2 * N
        assert eng.iq_saturated() - before == want_sat
        got = out.cpu().numpy()
        assert np.array_equal(iq.cpu().numpy(), ref)  # the input is only read
        assert np.array_equal(got, want), _differ(got, want)
        plain, _, _ = eng.run_host(p)
        assert np.array_equal(plain, ref)
