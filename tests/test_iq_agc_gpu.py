"""The block AGC and the 2-bit quantiser on the MI355X: k_agc_power, k_agc_gains and k_iq_agc against the numpy model
(tests/agc_model.py) -- bytes, gains and saturation count all equal -- on input in segments of very different amplitude, at the edges of
the blocks, of the lane runs, of a workgroup and of the grid, at every alignment of the stream to the blocks; the stream in cuts; the
window bound; gal_synth_agc_set; the refusals; and the engine's own output with a noise floor against the model over the oracle's
stream."""
import ctypes

import numpy as np
import pytest

import agc_model
import noise_model
from oracle_binding import oracle_run

pytestmark = pytest.mark.gpu

N = 26000
FS = 2.6e6
GAL_E_INVAL, GAL_E_STATE = -1, -4
SHAPES = [(16, 1), (17, 3), (64, 64), (2600, 8), (4099, 15), (65536, 1)]
FORMATS = [("ishort", 0), ("ibyte", 5), ("i2bit", 1024)]
SENTINEL = 0x5A
GAIN_SENTINEL = 0xA5A5A5A5


def _params(B, W):
    """gain_min 1.5: the full-scale segment saturates the int16 clamp; a p_init of rms 300: a gain of 13981 on the first blocks."""
    return agc_model.params(B, W, 1024 * 256, gain_min_q12=6144, p_init=2 * B * 300 * 300)


def _sizes(B, fmt):
    run, wg = agc_model.RUN[fmt], agc_model.RUN[fmt] * agc_model.THREADS
    c = agc_model.POWER_CHUNK
    return sorted({1, B - 1, B, B + 1, 4 * B + 3, run - 1, run, run + 1, wg - 1, wg, wg + 1, c - 1, c, c + 1})


def _firsts(B):
    return (0, 1, B - 1, 2 ** 40 + 3)


def _dev(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _full(n, value, dtype):
    import torch

    t = torch.full((n,), value, dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    return t


def _call(eng, x, fmt, param, expect_gains):
    """One gal_synth_iq_agc call over the interleaved int16 x in buffers of its own: (bytes, gains, saturated values).  The output is 32
    bytes and the gain array 8 words longer than the call needs, and both must come back untouched behind what the call wrote."""
    import torch

    n = x.size // 2
    nb = agc_model.out_bytes(fmt, n)
    d_in, d_out = _dev(x), _full(nb + 32, SENTINEL, torch.uint8)
    d_g = _full(expect_gains + 8, GAIN_SENTINEL - (1 << 32), torch.int32)
    before = eng.iq_saturated()
    ng = eng.iq_agc(d_in.data_ptr(), n, fmt, param, d_out.data_ptr(), d_g.data_ptr())
    sat = eng.iq_saturated() - before
    assert ng == expect_gains
    out = d_out.cpu().numpy()
    g = d_g.cpu().numpy().view(np.uint32)
    assert (out[nb:] == SENTINEL).all(), "the kernel wrote behind the call's last byte"
    assert (g[ng:] == GAIN_SENTINEL).all(), "the kernel wrote behind the call's last gain"
    return out[:nb], g[:ng], sat


def _stream_in_cuts(eng, x, cuts, B, P, fmt, param):
    outs, gains, sat, at = [], [], 0, 0
    for c in list(cuts) + [x.size // 2 - sum(cuts)]:
        o, g, s = _call(eng, x[2 * at: 2 * (at + c)], fmt, param, agc_model.blocks(P + at, c, B))
        outs.append(o)
        gains.append(g)
        sat += s
        at += c
    assert at == x.size // 2
    return np.concatenate(outs), np.concatenate(gains), sat


def _differ(got, want):
    if got.size != want.size:
        return "%d values, not %d" % (got.size, want.size)
    bad = np.flatnonzero(got != want)
    return "%d of %d differ (first at %d)" % (bad.size, got.size, bad[0] if bad.size else -1)


@pytest.mark.parametrize("fmt,param", FORMATS)
@pytest.mark.parametrize("B,W", SHAPES)
def test_kernels_against_the_model(pkg, B, W, fmt, param):
    p = _params(B, W)
    rng = np.random.default_rng(100 * B + W)
    sizes = _sizes(B, fmt)
    full = agc_model.make_input(rng, max(max(sizes), 3 * agc_model.segment(p)), p)
    # the input does what it is for: over its first three segments both gain clamps fire and the int16 clamp saturates
    _, g_all, sat_all = agc_model.agc(full[: 2 * 3 * agc_model.segment(p)], p, 0, fmt, param)
    assert sat_all > 0 and int(g_all.max()) == 1 << 24 and int(g_all.min()) == 6144
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        for P in _firsts(B):
            for n in sizes + ([3 * agc_model.segment(p)] if P == 1 else []):
                x = full[: 2 * n]
                want, want_g, want_sat = agc_model.agc(x, p, P, fmt, param)
                assert want_sat > 0  # the first block already saturates
                eng.agc_set(p, P)  # a new stream for every size
                got, g, sat = _call(eng, x, fmt, param, want_g.size)
                assert np.array_equal(got, want), "B %d, W %d, P %d, n %d: bytes: %s" % (B, W, P, n, _differ(got, want))
                assert np.array_equal(g, want_g), "B %d, W %d, P %d, n %d: gains: %s" % (B, W, P, n, _differ(g, want_g))
                assert sat == want_sat, (B, W, P, n)


@pytest.mark.parametrize("fmt,param", FORMATS)
def test_the_grid_stride_loop_runs_twice(pkg, fmt, param):
    """One size just over what the full grid of k_iq_agc covers in one trip (2048 workgroups x 256 lanes x the format's run), from
    inside a block, with a tail."""
    B, W = 2600, 8
    p = _params(B, W)
    n = agc_model.MAX_BLOCKS * agc_model.THREADS * agc_model.RUN[fmt] + 2 * agc_model.RUN[fmt] + 3
    x = agc_model.make_input(np.random.default_rng(5), n, p)
    want, want_g, want_sat = agc_model.agc(x, p, 1, fmt, param)
    assert want_sat > 0
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        eng.agc_set(p, 1)
        got, g, sat = _call(eng, x, fmt, param, want_g.size)
        assert np.array_equal(got, want), _differ(got, want)
        assert np.array_equal(g, want_g), _differ(g, want_g)
        assert sat == want_sat


@pytest.fixture(scope="module")
def streams():
    """Per shape: a stream of three segments and 4700 samples, and the model's output of ONE call per format."""
    out = {}
    for B, W in ((17, 3), (2600, 8)):
        p = _params(B, W)
        x = agc_model.make_input(np.random.default_rng(B), 3 * agc_model.segment(p) + 4700, p)
        x.setflags(write=False)
        out[(B, W)] = (p, x, {fmt: agc_model.agc(x, p, 0, fmt, param) for fmt, param in FORMATS})
    return out


@pytest.mark.parametrize("fmt,param", FORMATS)
@pytest.mark.parametrize("B,W", [(17, 3), (2600, 8)])
def test_any_cut_of_a_stream_gives_the_bytes_and_gains_of_one_call(pkg, streams, B, W, fmt, param):
    p, x, want = streams[(B, W)]
    want_out, want_g, want_sat = want[fmt]
    cuts = [1, 3, B - 1, B, B + 1, 2, 510, 4096]
    if fmt == "i2bit":  # the packed format: cuts at even sample counts, so that every call begins at a byte
        cuts = [c + (c & 1) for c in cuts]
    assert want_sat > 0 and sum(cuts) < x.size // 2
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        eng.agc_set(p)
        one, g, sat = _call(eng, x, fmt, param, want_g.size)
        assert np.array_equal(one, want_out) and np.array_equal(g, want_g) and sat == want_sat
        # agc_set again restarts the stream: the history is p_init again
        eng.agc_set(p)
        cut, g, sat = _stream_in_cuts(eng, x, cuts, B, 0, fmt, param)
        assert np.array_equal(cut, want_out), _differ(cut, want_out)
        assert np.array_equal(g, want_g), _differ(g, want_g)
        assert sat == want_sat
        # not reset: the stream goes on from the end of x
        n = x.size // 2
        more, g_more, _ = _call(eng, x[: 2 * 600], fmt, param, agc_model.blocks(n, 600, B))
        s = agc_model.Stream(p)
        s.call(x, fmt, param)
        want_more, want_g_more, _ = s.call(x[: 2 * 600], fmt, param)
        assert np.array_equal(more, want_more) and np.array_equal(g_more, want_g_more)
        # a refused agc_set leaves the AGC in force, its state and its position as they are
        for bad in (dict(p, block_len=15), dict(p, window=65), dict(p, block_len=65536, window=2), dict(p, target_q8=0),
                    dict(p, gain_min_q12=0), dict(p, p_init=(B << 31) + 1)):
            with pytest.raises(pkg.GalSynthError) as e:
                eng.agc_set(bad)
            assert e.value.code == GAL_E_INVAL
        with pytest.raises(pkg.GalSynthError) as e:
            eng.agc_set(p, 2 ** 62)
        assert e.value.code == GAL_E_INVAL
        again, g_again, _ = _call(eng, x[2 * 600: 2 * 1300], fmt, param, agc_model.blocks(n + 600, 700, B))
        want_again, want_g_again, _ = s.call(x[2 * 600: 2 * 1300], fmt, param)
        assert np.array_equal(again, want_again) and np.array_equal(g_again, want_g_again)
        # NULL frees it
        eng.agc_set(None)
        with pytest.raises(pkg.GalSynthError) as e:
            _call(eng, x[:64], fmt, param, 0)
        assert e.value.code == GAL_E_STATE


@pytest.mark.parametrize("B,W", [(65536, 1), (1024, 64)])
def test_the_window_bound(pkg, B, W):
    """All values -32768 at B x W = 65536 with p_init at its bound: Q = 2^47 exactly for every block, Q << 16 = 2^63, rms_q8 = 2^23
    (tests/test_iq_agc_cpu.py shows the model reaches it); in one call and in cuts."""
    p = agc_model.params(B, W, 32767 * 256, p_init=B << 31)
    n = (W + 2) * B + 3
    x = np.full(2 * n, -32768, dtype=np.int16)
    want, want_g, want_sat = agc_model.agc(x, p)
    assert (want_g == 4095).all() and want_sat == 0 and (want.view("<i2") == -32760).all()
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        eng.agc_set(p)
        got, g, sat = _call(eng, x, "ishort", 0, want_g.size)
        assert np.array_equal(got, want) and np.array_equal(g, want_g) and sat == 0
        eng.agc_set(p)
        got, g, sat = _stream_in_cuts(eng, x, (1, B - 1, B + 1, 3), B, 0, "ishort", 0)
        assert np.array_equal(got, want) and np.array_equal(g, want_g) and sat == 0


def test_refusals(pkg, streams):
    import torch

    p, x, _ = streams[(2600, 8)]
    w = pkg.workloads.make_synthetic(n_epochs=1, n_chan=2, n_slots=16, samples_per_epoch=N, seed=79)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        a, b = _dev(x[: 2 * 6000]), _full(4 * 6000 + 64, 0, torch.uint8)
        gbuf = _full(64, 0, torch.int32)
        lib, h = eng._lib, eng._h

        def code(*args):
            with pytest.raises(pkg.GalSynthError) as e:
                eng.iq_agc(*args)
            return e.value.code

        assert code(a.data_ptr(), 1000, "ishort", 0, b.data_ptr()) == GAL_E_STATE  # no AGC set
        eng.agc_set(p)
        ng = ctypes.c_size_t(7)
        assert lib.gal_synth_iq_agc(None, ctypes.c_void_p(a.data_ptr()), 900, 0, 0, ctypes.c_void_p(b.data_ptr()), None, ctypes.byref(ng)) == GAL_E_INVAL
        assert code(a.data_ptr(), 1000, 2, 0, b.data_ptr()) == GAL_E_INVAL  # ibit: a sign needs no gain control
        assert code(a.data_ptr(), 1000, 4, 0, b.data_ptr()) == GAL_E_INVAL  # unknown formats
        assert code(a.data_ptr(), 1000, -1, 0, b.data_ptr()) == GAL_E_INVAL
        with pytest.raises(ValueError):
            eng.iq_agc(a.data_ptr(), 1000, "ibit", 0, b.data_ptr())
        for fmt, bad in (("ishort", 1), ("ishort", -1), ("ibyte", -1), ("ibyte", 16), ("i2bit", 0), ("i2bit", 32768), ("i2bit", -5)):
            assert code(a.data_ptr(), 1000, fmt, bad, b.data_ptr()) == GAL_E_INVAL, (fmt, bad)
        assert code(a.data_ptr() + 4, 900, "ishort", 0, b.data_ptr()) == GAL_E_INVAL  # misaligned input
        assert code(a.data_ptr(), 900, "ishort", 0, b.data_ptr() + 8) == GAL_E_INVAL  # misaligned output
        assert code(a.data_ptr(), 900, "ishort", 0, b.data_ptr(), gbuf.data_ptr() + 2) == GAL_E_INVAL  # misaligned gains
        assert code(0, 900, "ishort", 0, b.data_ptr()) == GAL_E_INVAL
        assert code(a.data_ptr(), 900, "ishort", 0, 0) == GAL_E_INVAL
        assert code(a.data_ptr(), 1000, "ishort", 0, a.data_ptr()) == GAL_E_INVAL  # in place
        assert code(a.data_ptr(), 1000, "i2bit", 1024, a.data_ptr() + 4 * 992) == GAL_E_INVAL  # the output begins inside the input
        assert code(a.data_ptr() + 4 * 100, 1000, "i2bit", 1024, a.data_ptr()) == GAL_E_INVAL  # 500 bytes from a: they reach the input
        assert code(a.data_ptr(), 3000, "ishort", 0, b.data_ptr(), a.data_ptr() + 4 * 2996) == GAL_E_INVAL  # the gains inside the input
        assert code(a.data_ptr(), 3000, "ishort", 0, b.data_ptr(), b.data_ptr() + 4 * 2999) == GAL_E_INVAL  # ... inside the output
        assert code(a.data_ptr(), 2 ** 41, "ishort", 0, b.data_ptr()) == GAL_E_INVAL
        # nothing of this moved the stream: side by side in one buffer is no overlap, and the bytes are those of the stream's start
        assert eng.iq_agc(a.data_ptr(), 1000, "i2bit", 1024, a.data_ptr() + 4 * 1000, a.data_ptr() + 4 * 1000 + 512) == 1
        eng.iq_saturated()
        want, want_g, _ = agc_model.agc(x[: 2 * 1000], p, 0, "i2bit", 1024)
        got = a.cpu().numpy().view(np.uint8)
        assert np.array_equal(got[4 * 1000: 4 * 1000 + 500], want)
        assert np.array_equal(got[4 * 1000 + 512: 4 * 1000 + 516].view(np.uint32), want_g)
        assert eng.iq_agc(a.data_ptr(), 0, "ishort", 0, b.data_ptr()) == 0  # nothing happens
        # the filters' slots are independent of the AGC's
        eng.fir_set([16384])
        eng.fir_set(None)
        # a buffer of the batch in flight, as input and as output
        iq = _full(N * 2, 0, torch.int16)
        eng.plan(w)
        eng.execute(iq.data_ptr())
        assert code(iq.data_ptr(), 1000, "ishort", 0, b.data_ptr()) == GAL_E_STATE
        assert code(a.data_ptr(), 1000, "ishort", 0, iq.data_ptr() + 4 * 1000) == GAL_E_STATE
        assert code(a.data_ptr(), 3000, "ishort", 0, b.data_ptr(), iq.data_ptr() + 4 * 2000) == GAL_E_STATE
        eng.finish()
        eng.iq_agc(iq.data_ptr(), 1000, "ishort", 0, b.data_ptr())
        eng.iq_saturated()


@pytest.mark.parametrize("fmt,param", FORMATS)
def test_engine_output_with_a_noise_floor(pkg, fmt, param):
    """3 epochs x 26000 samples of the engine, the noise floor of gal_synth_iq_convert_noise at 45 dB-Hz in place, then the AGC: the
    models over the oracle's stream; the plain output of the same handle afterwards is still the oracle's."""
    import torch

    w = pkg.workloads.make_synthetic(n_epochs=3, n_chan=4, n_slots=16, samples_per_epoch=N, seed=77)
    ref, _ = oracle_run(w, N, FS)
    gq, sq = noise_model.noise_from_cn0(45.0, FS, 1.0)
    noise = {"seed": 11, "stream": 2, "gain_q16": gq, "sigma_q4": sq}
    noisy, clipped = noise_model.mix(ref, 11, 2, gq, sq)
    assert int(np.count_nonzero(clipped)) == 0
    p = pkg.synth.agc_from_rms(1024.0, sq / 16.0, 2600, 8)
    assert p == agc_model.from_rms(1024.0, sq / 16.0, 2600, 8)
    want, want_g, want_sat = agc_model.agc(noisy, p, 0, fmt, param)
    assert want_g.size == 30
    # the gain settles near 1024 / sigma: the four satellites add at most 4 x 2 x 250^2 = 5e5 to sigma^2 = 5.1e6 per rail, 5 % in rms,
    # on top of the 2 % of the convergence test (tests/test_iq_agc_cpu.py)
    assert abs(want_g[-1] / 4096.0 * (sq / 16.0) / 1024.0 - 1.0) < 0.07
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        iq = _full(3 * N * 2, 0, torch.int16)
        out = _full(agc_model.out_bytes(fmt, 3 * N) + 32, SENTINEL, torch.uint8)
        gains = _full(30 + 8, 0, torch.int32)
        eng.agc_set(p)
        eng.plan(w)
        eng.execute(iq.data_ptr())
        eng.finish()
        before = eng.iq_saturated()
        eng.iq_convert(iq.data_ptr(), 3 * N, "ishort", out_ptr=iq.data_ptr(), noise=noise, first_sample=0)
        # the batch in two calls, cut inside a block where the bytes of every format end on the 16-byte grid
        n1 = 25600
        nb1 = agc_model.out_bytes(fmt, n1)
        assert eng.iq_agc(iq.data_ptr(), n1, fmt, param, out.data_ptr(), gains.data_ptr()) == 10
        assert eng.iq_agc(iq.data_ptr() + 4 * n1, 3 * N - n1, fmt, param, out.data_ptr() + nb1, gains.data_ptr() + 40) == 20
        assert eng.iq_saturated() - before == want_sat
        got = out.cpu().numpy()
        assert np.array_equal(iq.cpu().numpy(), noisy)  # the AGC only reads its input
        assert np.array_equal(got[: want.size], want), _differ(got[: want.size], want)
        assert (got[want.size:] == SENTINEL).all()
        assert np.array_equal(gains.cpu().numpy().view(np.uint32)[:30], want_g)
        plain, _, _ = eng.run_host(w)
        assert np.array_equal(plain, ref)
