"""The receiver oscillator on the MI355X: k_osc_tilesum, k_osc_scan and k_iq_osc against the numpy model (tests/osc_model.py) -- bytes
and saturation count equal -- at the edges of a vector, a wave, a tile and the grid, in place and out of place, with and without phase
noise; three trips of the grid-stride loop, the scan with every lane full and the stream behind such a call; the stream in cuts; the wrap arithmetic at the largest parameters; full-scale input; gal_synth_osc_set; the refusals; and one
satellite of the oracle's stream through a +2 kHz oscillator and the correlator bank."""
import ctypes

import numpy as np
import pytest

import corr_model
import osc_model
from oracle_binding import oracle_run
from tile_launch_model import OSC_GEOMETRIES

pytestmark = pytest.mark.gpu

N = 26000
FS = 2.6e6
FC = 1575.42e6
GAL_E_INVAL, GAL_E_STATE = -1, -4
SENTINEL = 0x5A5A
T = osc_model.TILE
LENGTHS = sorted({1, 3, 4, 5, 255, 256, 257} | {k * T + d for k in (1, 2, 65) for d in (-1, 0, 1)})
FIRSTS = (0, 2 ** 40 + 3)
# an offset, a drift and a start phase that make every term of Phi matter; S: 1e-4 cycles per sample
DET = dict(p0=0x3333333344444444, f=round(1234.5 / FS * 2 ** 64), d=round(5.0e4 / FS / FS * 2 ** 64))
NOISY = dict(DET, s=int(1e-4 * 2 ** 52), seed=0x1234567890ABCDEF, stream=7)


def _dev(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _input(rng, n, amp=12000):
    return rng.integers(-amp, amp + 1, 2 * n, dtype=np.int16)


def _call(eng, x, in_place):
    """One gal_synth_iq_osc call over the interleaved int16 x: (output, saturated samples).  The buffers are 16 values longer than the
    call needs and must come back untouched behind the call's last sample; out of place the input must come back as it was."""
    import torch

    n = x.size // 2
    d_in = _dev(np.concatenate((x, np.full(16, SENTINEL, dtype=np.int16))))
    d_out = d_in if in_place else _dev(np.full(2 * n + 16, SENTINEL, dtype=np.int16))
    before = eng.iq_saturated()
    eng.iq_osc(d_in.data_ptr(), n, d_out.data_ptr())
    sat = eng.iq_saturated() - before
    out = d_out.cpu().numpy()
    assert (out[2 * n:] == SENTINEL).all(), "the kernel wrote behind the call's last sample"
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy()[: 2 * n], x), "the input changed"
    del d_in, d_out
    torch.cuda.synchronize()
    return out[: 2 * n], sat


def _differ(got, want):
    bad = np.flatnonzero(got != want)
    return "%d of %d differ (first at %d)" % (bad.size, got.size, bad[0] if bad.size else -1)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("o", [DET, NOISY], ids=["S0", "S>0"])
def test_lengths_against_the_model(pkg, o, in_place):
    rng = np.random.default_rng(5)
    full = _input(rng, max(LENGTHS))
    o = osc_model.osc(**o)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        for first in FIRSTS:
            want_all, _, _ = osc_model.rotate(full, o, first, first)
            assert not np.array_equal(want_all, full)
            for n in LENGTHS:
                want, want_sat, _ = osc_model.rotate(full[: 2 * n], o, first, first)
                assert np.array_equal(want, want_all[: 2 * n])  # (a prefix of the stream: the model has no look-ahead)
                eng.osc_set(o, first)  # a new stream for every length
                got, sat = _call(eng, full[: 2 * n], in_place)
                assert np.array_equal(got, want), "first %d, n %d: %s" % (first, n, _differ(got, want))
                assert sat == want_sat == 0, (first, n)


@pytest.mark.parametrize("o", [DET, NOISY], ids=["S0", "S>0"])
def test_the_grid_stride_loop_runs_twice(pkg, o):
    """More tiles than the grid has blocks, and an odd global start: every block takes a second tile, the last of them a partial one."""
    n = (osc_model.MAX_BLOCKS + 3) * T + 2
    rng = np.random.default_rng(6)
    x = _input(rng, n)
    o = osc_model.osc(**o)
    want, want_sat, _ = osc_model.rotate(x, o, 2 ** 40 + 1, 2 ** 40 + 1)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        eng.osc_set(o, 2 ** 40 + 1)
        got, sat = _call(eng, x, True)
    assert np.array_equal(got, want), _differ(got, want)
    assert sat == want_sat


@pytest.fixture(scope="module")
def long_input():
    """Input for the longest geometry of tile_launch_model.OSC_GEOMETRIES and the two short calls behind it."""
    n = max(n for n, _ in OSC_GEOMETRIES.values()) + SHORT_BEHIND[0] + SHORT_BEHIND[1]
    x = _input(np.random.default_rng(11), n)
    x.setflags(write=False)
    return x


SHORT_BEHIND = (5, T + 1)  # the calls directly behind a long one: less than a vector more than one, and a tile and a sample
LONG_CASES = [("third_trip", DET), ("third_trip", NOISY), ("full_scan", NOISY)]


@pytest.mark.parametrize("name,o", LONG_CASES, ids=["third_trip-S0", "third_trip-S>0", "full_scan-S>0"])
def test_three_trips_and_the_stream_behind_them(pkg, long_input, name, o):
    """The geometries of tests/tile_launch_model.py (tests/test_iq_launch_geometry_cpu.py asserts what each is for): a block's third
    trip writes the LDS set its first trip read (k_osc_tilesum, k_iq_osc<true>); the scan with five tiles per lane and empty lanes
    behind, and with six in every lane so that the last lane forms the state word from its own tiles.  In place, bit for bit, count
    and guard.  Directly behind the long call, with no osc_set in between, two short calls go on with the stream: they start from the
    state word that the long scan wrote.  With S = 0 (one launch, no LDS in the loop) the per-tile A and W at tiles beyond 2^22
    samples."""
    n, first = OSC_GEOMETRIES[name]
    o = osc_model.osc(**o)
    x = long_input[:2 * n]
    want, want_sat, zz = osc_model.rotate(x, o, first, first)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        eng.osc_set(o, first)
        got, sat = _call(eng, x, True)
        assert np.array_equal(got, want), "%s: %s" % (name, _differ(got, want))
        assert sat == want_sat
        at = n
        for m in SHORT_BEHIND:
            xs = long_input[2 * at:2 * (at + m)]
            want, want_sat, zz = osc_model.rotate(xs, o, first, first + at, zz)
            got, sat = _call(eng, xs, False)
            assert np.array_equal(got, want), "%s, %d samples behind sample %d: %s" % (name, m, at, _differ(got, want))
            assert sat == want_sat
            at += m
    assert (zz != 0) == (o["s"] != 0)


@pytest.mark.parametrize("first", FIRSTS)
def test_any_cut_into_calls_is_the_single_call(pkg, first):
    n = 3 * 26001
    rng = np.random.default_rng(7 + (first & 7))
    x = _input(rng, n)
    o = osc_model.osc(**NOISY)
    want, want_sat, _ = osc_model.rotate(x, o, first, first)
    cuts = []
    while sum(cuts) < n:
        cuts.append(min(int(rng.integers(1, 4901)), n - sum(cuts)))
    assert len(cuts) > 20 and any(c % 4 for c in cuts)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        eng.osc_set(o, first)
        single, sat1 = _call(eng, x, False)
        assert np.array_equal(single, want), _differ(single, want)
        eng.osc_set(o, first)
        outs, sat, at = [], 0, 0
        for k, c in enumerate(cuts):
            got, s = _call(eng, x[2 * at: 2 * (at + c)], bool(k & 1))
            outs.append(got)
            sat += s
            at += c
        pieces = np.concatenate(outs)
        assert np.array_equal(pieces, want), _differ(pieces, want)
        assert sat == sat1 == want_sat


@pytest.mark.parametrize("sign", [1, -1])
def test_the_largest_parameters_wrap_as_the_model(pkg, sign):
    """F at +-(fs / 2 - 1 Hz), the largest drift gal_synth_osc_make admits and S = 2^48: every product wraps many times."""
    import math

    o = pkg.osc_make(sign * (FS / 2 - 1.0), sign * math.nextafter(0.5 * FS * FS, 0.0), 0.0, FS, FC)
    assert abs(o["f"]) > 2 ** 62 and abs(o["d"]) > 2 ** 62
    o = osc_model.osc(**dict(o, s=1 << 48, p0=2 ** 64 - 1, seed=2 ** 64 - 1, stream=2 ** 32 - 1))
    n = 2 * T + 77
    x = _input(np.random.default_rng(8), n)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        for first in (0, 2 ** 40 + 3, 2 ** 62 - 2 * T - 78):
            want, want_sat, _ = osc_model.rotate(x, o, first, first)
            eng.osc_set(o, first)
            got, sat = _call(eng, x, False)
            assert np.array_equal(got, want), "first %d: %s" % (first, _differ(got, want))
            assert sat == want_sat


@pytest.mark.parametrize("o", [DET, NOISY], ids=["S0", "S>0"])
def test_full_scale_input_clamps_and_counts(pkg, o):
    n = 3 * T + 3
    rng = np.random.default_rng(9)
    # both rails at +-full scale clamp at every phase (|x| = 46341: the larger rail of the turned sample is at least 32768); both at
    # +-26000 (|x| = 36770) clamp only where the turned sample comes near an axis: the counter must tell the two apart
    x = rng.choice(np.array([-32768, 32767, -26000, 26000], dtype=np.int16), 2 * n)
    x[0:8] = (-32768, -32768, 32767, 32767, -32768, 32767, 32767, -32768)
    o = osc_model.osc(**o)
    want, want_sat, _ = osc_model.rotate(x, o, 11, 11)
    assert 0 < want_sat < n and (want == 32767).any() and (want == -32768).any()
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        eng.osc_set(o, 11)
        got, sat = _call(eng, x, False)
        assert np.array_equal(got, want), _differ(got, want)
        assert sat == want_sat
        # the zero oscillator passes full scale through untouched
        eng.osc_set({}, 0)
        got, sat = _call(eng, x, True)
        assert np.array_equal(got, x) and sat == 0


def test_osc_set_restarts_the_sum_and_null_switches_off(pkg):
    import torch

    n = 2 * T + 5
    x = _input(np.random.default_rng(10), n)
    o = osc_model.osc(**NOISY)
    want, _, _ = osc_model.rotate(x, o, 100, 100)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        buf = _dev(x)
        with pytest.raises(pkg.GalSynthError) as ei:  # nothing set yet
            eng.iq_osc(buf.data_ptr(), n, buf.data_ptr())
        assert ei.value.code == GAL_E_STATE
        eng.osc_set(o, 100)
        first, _ = _call(eng, x, False)
        cont, _ = _call(eng, x, False)  # the stream goes on: another phase, another sum
        assert np.array_equal(first, want) and not np.array_equal(cont, want)
        want2, _, _ = osc_model.rotate(np.concatenate((x, x)), o, 100, 100)
        assert np.array_equal(cont, want2[2 * n:])
        eng.osc_set(o, 100)  # Z starts again
        again, _ = _call(eng, x, False)
        assert np.array_equal(again, want)
        eng.osc_set(None)
        with pytest.raises(pkg.GalSynthError) as ei:
            eng.iq_osc(buf.data_ptr(), n, buf.data_ptr())
        assert ei.value.code == GAL_E_STATE
        torch.cuda.synchronize()


def test_bad_arguments_and_overlap_are_refused(pkg):
    import torch

    lib = pkg.load_library()
    n = 4096
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        buf = torch.zeros(4 * n + 64, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        a = buf.data_ptr()
        o = pkg.synth._osc_struct({"s": (1 << 48) + 1})
        assert lib.gal_synth_osc_set(eng._h, ctypes.byref(o), 0) == GAL_E_INVAL
        o = pkg.synth._osc_struct({"f": 5})
        o.reserved = 3
        assert lib.gal_synth_osc_set(eng._h, ctypes.byref(o), 0) == GAL_E_INVAL
        o.reserved = 0
        assert lib.gal_synth_osc_set(eng._h, ctypes.byref(o), 1 << 62) == GAL_E_INVAL
        assert lib.gal_synth_osc_set(None, ctypes.byref(o), 0) == GAL_E_INVAL
        assert lib.gal_synth_iq_osc(eng._h, a, n, a + 4 * n) == GAL_E_STATE  # the refused sets left no oscillator
        eng.osc_set({"f": 5, "s": 9}, 0)

        def call(src, count, dst):
            return lib.gal_synth_iq_osc(eng._h, src, count, dst)

        assert call(None, n, a) == GAL_E_INVAL and call(a, n, None) == GAL_E_INVAL
        assert lib.gal_synth_iq_osc(None, a, n, a) == GAL_E_INVAL
        assert call(a + 4, n, a + 4 * n) == GAL_E_INVAL and call(a, n, a + 4 * n + 8) == GAL_E_INVAL  # alignment
        assert call(a, 1 << 41, a) == GAL_E_INVAL
        assert call(a, n, a + 16) == GAL_E_INVAL and call(a + 16, n, a) == GAL_E_INVAL  # partial overlap
        assert call(a, n, a + 4 * n - 16) == GAL_E_INVAL
        assert call(a, 0, a) == 0
        assert call(a, n, a) == 0 and call(a, n, a + 4 * n) == 0  # exactly in place, and disjoint
        eng.iq_saturated()


def test_buffer_of_the_batch_in_flight_is_refused(pkg):
    import torch

    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=4, n_slots=16, samples_per_epoch=N, seed=12)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as e:
        iq = torch.zeros(2 * N * 2, dtype=torch.int16, device="cuda")
        other = torch.zeros(2 * N * 2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        e.osc_set({"f": 1 << 50}, 0)
        e.plan(p)
        e.execute(iq.data_ptr())
        for src, dst in ((iq, other), (other, iq), (iq, iq)):
            with pytest.raises(pkg.GalSynthError) as ei:
                e.iq_osc(src.data_ptr(), 2 * N, dst.data_ptr())
            assert ei.value.code == GAL_E_STATE
        e.finish()
        e.iq_osc(iq.data_ptr(), 2 * N, iq.data_ptr())
        e.iq_saturated()


def test_a_satellite_through_the_oscillator_and_the_correlator(pkg):
    """One satellite of the oracle at 4.092 MS/s, six code periods; +2 kHz of oscillator; the correlator at carr_dph + lo_step finds
    the prompt sums of the unrotated stream at the request's own carr_dph.  The two differ by the tables' phase steps (the
    correlator's 512-entry carrier table sees other phases): the figure is measured on the numpy model -- the worst
    |S_rot - S_plain| / |S_plain| over the whole periods and both components -- and three times that is allowed (DESIGN.md section 19:
    the model's figure is 1.1e-4)."""
    import torch

    fs, spe = 4.092e6, 6 * 16368
    p = pkg.workloads.make_synthetic(n_epochs=1, n_chan=1, n_slots=16, samples_per_epoch=spe, sample_rate=fs, prns=[11], seed=77)
    iq, _ = oracle_run(p, spe, fs)
    iq = np.ascontiguousarray(iq).view(np.int16).ravel()
    o = pkg.osc_make(2000.0, 0.0, 0.0, fs, FC)
    step = pkg.osc_lo_step(o, 0)
    assert step == osc_model.lo_step(o, 0) and abs(step - 2000.0 / fs * 2 ** 32) <= 1
    q = pkg.corr_from_epoch(p[0, 0], fs, 0, max_periods=6)
    q_lo = dict(q, carr_dph=q["carr_dph"] + step)
    tables = pkg.tables()

    def prompt(s):  # complex S_B, S_C of the whole periods 1 .. 4
        s = np.asarray(s, dtype=np.float64)[1:5, 0, 0]
        return np.stack((s[:, 0] + 1j * s[:, 1], s[:, 2] + 1j * s[:, 3]), axis=1)

    def figure(rot, plain):
        return float(np.max(np.abs(prompt(rot) - prompt(plain)) / np.abs(prompt(plain))))

    y_model, sat_model, _ = osc_model.rotate(iq, o, 0, 0)
    plain_model = corr_model.correlate(iq.astype(np.int64), q, tables)
    fig_model = figure(corr_model.correlate(y_model.astype(np.int64), q_lo, tables), plain_model)
    # without following the oscillator the peak is gone: 2 kHz turns eight times in a period
    lost = corr_model.correlate(y_model.astype(np.int64), q, tables)
    assert np.abs(prompt(lost)).max() < 0.1 * np.abs(prompt(plain_model)).min()
    with pkg.SynthEngine(sample_rate=fs, samples_per_epoch=spe, n_slots=16, device=0) as eng:
        d = _dev(iq)
        plain = eng.correlate(d.data_ptr(), "ishort", spe, q)
        eng.osc_set(o, 0)
        before = eng.iq_saturated()
        eng.iq_osc(d.data_ptr(), spe, d.data_ptr())
        assert eng.iq_saturated() - before == sat_model == 0
        assert np.array_equal(d.cpu().numpy(), y_model)
        rot = eng.correlate(d.data_ptr(), "ishort", spe, q_lo)
        torch.cuda.synchronize()
    assert np.array_equal(plain, plain_model)
    fig = figure(rot, plain)
    print("prompt sums: model figure %.3e, device %.3e" % (fig_model, fig))
    assert 0 < fig_model < 1e-2
    assert fig <= 3.0 * fig_model
