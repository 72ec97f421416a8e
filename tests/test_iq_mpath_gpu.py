"""Per-satellite multipath on the MI355X: k_iq_echo bit for bit against the numpy model (tests/mpath_model.py) -- part and echo counts,
epochs that end inside a vector, every kind of delay, history across calls, phase steps that wrap, both accumulator widths, the launch
geometry -- and gal_synth_run_mpath against the model over the oracle's output of every slot on its own."""
import numpy as np
import pytest

import gain_model
import launch_model
import mpath_model
from oracle_binding import oracle_run

pytestmark = pytest.mark.gpu

N = 26000
FS = 2.6e6
GAL_E_INVAL, GAL_E_STATE = -1, -4
DELAYS = (0, 1, 3, 4, 5, 255, 1023, 1024)
GUARD = 16  # int16 values behind the output that the kernel must leave alone


@pytest.fixture(scope="module")
def cos1024(pkg):
    return pkg.tables()["cos1024"]


def _dev(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _call(eng, parts, gains, pof, rows, hist_id=None):
    """One gal_synth_iq_mpath call: (bytes, saturation count); the GUARD values behind the output must come back untouched."""
    import torch

    devs = [_dev(p) for p in parts]
    out = torch.full((parts.shape[1] + GUARD,), 0x5a5a, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    before = eng.iq_saturated()
    eng.iq_mpath([d.data_ptr() for d in devs], gains, out.data_ptr(), pof, rows, hist_id)
    sat = eng.iq_saturated() - before
    got = out.cpu().numpy()
    assert (got[parts.shape[1]:] == 0x5a5a).all(), "the kernel wrote behind the last epoch"
    return got[:parts.shape[1]], sat


def _same(got, want, spe):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d of %d values differ, the first at value %d = epoch %d, value %d of it (got %d, want %d)" % (
        bad.size, got.size, bad[0], bad[0] // (2 * spe), bad[0] % (2 * spe), got[bad[0]], want[bad[0]])


def _check(eng, lines, spe, parts, gains, pof, rows, hist_id=None):
    """The call on the handle and on the model's lines, which both carry their history on: bytes and saturation count."""
    got, sat = _call(eng, parts, gains, pof, rows, hist_id)
    want, want_sat = lines.call(parts, gains, spe, pof, rows, hist_id)
    _same(got, want, spe)
    assert sat == want_sat
    return want_sat


def _parts(rng, n_parts, n_epochs, spe, lim=3000):
    return rng.integers(-lim, lim, size=(n_parts, n_epochs * spe * 2), dtype=np.int16)


def _edge_parts(rng, n_parts, n_epochs, spe):
    """Random full-range int16; the first 8 values of every epoch +32767 on all parts at once, the next 8 -32768."""
    x = rng.integers(-32768, 32768, size=(n_parts, n_epochs, 2 * spe), dtype=np.int16)
    x[:, :, :8] = 32767
    x[:, :, 8:16] = -32768
    return x.reshape(n_parts, -1)


def _random_rows(rng, n_epochs, n_echo, gain_hi=400):
    r = mpath_model.rows(n_epochs, n_echo)
    r["gain_q7"] = rng.integers(1, gain_hi, size=r.shape)
    r["delay"] = rng.choice(DELAYS, size=r.shape)
    r["ph0"] = rng.integers(0, 1 << 32, size=r.shape, dtype=np.uint64)
    r["dph"] = rng.integers(-(1 << 20), 1 << 20, size=r.shape)
    return r


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n_parts", [1, 2, 3, 4, 5, 6, 63, 64])
def test_part_counts(pkg, cos1024, n_parts, wide):
    """The part loop takes four parts per trip and the rest one by one; echoes on the first and on the LAST part, two of them on one
    part.  Full-range parts: values clamp, and the count must be the model's.  wide: rows beyond 65535, the int64 instance."""
    spe, n_epochs = 1030, 3
    rng = np.random.default_rng(100 + n_parts)
    parts = _edge_parts(rng, n_parts, n_epochs, spe)
    gains = rng.integers(0, (30000 if wide else min(32767, 40000 // n_parts)) + 1, size=(n_epochs, n_parts))
    pof = [0, n_parts - 1, n_parts - 1]
    rows = _random_rows(rng, n_epochs, 3, 4000)
    rows["delay"][:, 0], rows["delay"][:, 1], rows["delay"][:, 2] = (1, 1024, 5), (4, 3, 1023), (255, 0, 2)
    if wide:
        rows["gain_q7"][1] = 32767
    assert mpath_model.needs_int64(gains, rows) == wide
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        lines = mpath_model.Lines(cos1024)
        sat = _check(eng, lines, spe, parts, gains, pof, rows)
        assert sat > 0 or not wide
        _check(eng, lines, spe, parts[::-1], gains, pof, rows)  # a second call: the delays read the first call's samples


@pytest.mark.parametrize("n_echo", [1, 2, 32])
@pytest.mark.parametrize("spe,n_epochs", [(26000, 3), (26001, 3), (26002, 3), (7, 300)])
def test_echo_counts_epoch_alignments_and_delays(pkg, cos1024, spe, n_epochs, n_echo):
    """Epochs that begin at every offset inside a 16-byte vector (the head and tail lanes), and every delay of DELAYS against them:
    multiples of 4 (one aligned load), the three other residues (two loads and a pick), 0 and the longest; with 7-sample epochs a
    delay reaches back over 146 epochs.  One call per delay for one echo; pairs; 32 echoes with a delay of their own per epoch."""
    rng = np.random.default_rng(spe + n_echo)
    n_parts = 3
    parts = _parts(rng, n_parts, n_epochs, spe)
    gains = rng.integers(0, 300, size=(n_epochs, n_parts))
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        lines = mpath_model.Lines(cos1024)
        if n_echo == 1:
            for D in DELAYS:
                rows = _random_rows(rng, n_epochs, 1)
                rows["delay"] = D
                _check(eng, lines, spe, parts, gains, [int(rng.integers(0, n_parts))], rows)
        elif n_echo == 2:
            for D0, D1 in zip(DELAYS, DELAYS[::-1]):
                rows = _random_rows(rng, n_epochs, 2)
                rows["delay"][:, 0], rows["delay"][:, 1] = D0, D1
                _check(eng, lines, spe, parts, gains, [2, 2], rows)
        else:
            rows = _random_rows(rng, n_epochs, 32, 60)
            rows["delay"][0] = np.resize(DELAYS, 32)
            pof = rng.integers(0, n_parts, size=32)
            pof[-1] = n_parts - 1
            for _ in range(2):
                _check(eng, lines, spe, parts, gains, pof, rows)


CUTS = (1, 5, 2, 30, 3, 9, 1, 49)  # epochs per call, of 100 samples: 100, 500, 200, 3000, 300, 900, 100 and 4900 samples


def test_any_cut_into_calls_is_the_single_call(pkg, cos1024):
    """Calls shorter than a history line roll it: the delay of 1024 samples reaches over three calls at the start.  In front of the
    stream are zeros, and again after gal_synth_mpath_reset."""
    spe, n_epochs = 100, sum(CUTS)
    rng = np.random.default_rng(11)
    parts = _parts(rng, 2, n_epochs, spe)
    gains = rng.integers(0, 300, size=(n_epochs, 2))
    rows = _random_rows(rng, n_epochs, 4)
    rows["delay"][:, 0], rows["delay"][:, 1] = 1024, 1023
    pof = [0, 1, 1, 0]
    want, want_sat, _ = mpath_model.mpath(parts, gains, spe, pof, rows, cos1024)
    assert want[:2 * spe].any()
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        for attempt in range(2):
            got, sat, e0 = [], 0, 0
            for ne in CUTS:
                y, s = _call(eng, parts[:, 2 * spe * e0:2 * spe * (e0 + ne)], gains[e0:e0 + ne], pof, rows[e0:e0 + ne])
                got.append(y)
                sat += s
                e0 += ne
            _same(np.concatenate(got), want, spe)
            assert sat == want_sat
            if attempt == 0:  # without a reset the stream goes on: other bytes at the start
                y, _ = _call(eng, parts[:, :2 * spe * 12], gains[:12], pof, rows[:12])
                assert not np.array_equal(y, want[:2 * spe * 12])
                eng.mpath_reset()
        eng.mpath_reset()
        y, s = _call(eng, parts, gains, pof, rows)  # and the whole stream in one call
        _same(y, want, spe)
        assert s == want_sat


def test_hist_id_names_the_line(pkg, cos1024):
    """Lines are named per call: permuted between calls, left out (-1) and taken up again, the last line (63)."""
    spe, n_epochs = 333, 2
    rng = np.random.default_rng(12)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        lines = mpath_model.Lines(cos1024)
        for ids, pof in (([5, 9, -1], [0, 1, 1]), ([9, 5, 63], [0, 1, 2]), ([-1, 63, 5], [2, 1, 1]), (None, [0, 1, 2]), ([2, 1, 0], [0, 1, 2])):
            rows = _random_rows(rng, n_epochs, 3)
            rows["delay"] = rng.choice((1024, 1023, 700, 4), size=rows.shape)
            _check(eng, lines, spe, _parts(rng, 3, n_epochs, spe), rng.integers(0, 300, size=(n_epochs, 3)), pof, rows, ids)


def test_phase_steps(pkg, cos1024):
    """Negative steps, and steps next to +-2^31 with 26001-sample epochs: m dph wraps thousands of times inside an epoch."""
    spe, n_epochs = 26001, 2
    rng = np.random.default_rng(13)
    parts = _parts(rng, 2, n_epochs, spe)
    gains = rng.integers(0, 300, size=(n_epochs, 2))
    steps = (-1, -12345, (1 << 31) - 1, -(1 << 31), -(1 << 31) + 1, (1 << 31) - 2, 1 << 22, -(1 << 22) - 1)
    rows = _random_rows(rng, n_epochs, len(steps))
    rows["dph"][0], rows["dph"][1] = steps, steps[::-1]
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        _check(eng, mpath_model.Lines(cos1024), spe, parts, gains, [0, 1] * 4, rows)


def test_both_instances_at_the_int32_bound(pkg, cos1024):
    """Rows with sum g + 2 sum A = 65535 (the last the int32 instance takes) and 65536 on parts at -32768 and at +32767, with echo
    phases at the eight octants (|c| + |s| at its largest between the axes): every value clamps, the count is the model's."""
    spe, n_epochs = 1030, 3
    rows = mpath_model.rows(n_epochs, 2, [[100, 200]], [[0, 3]], [[5 << 29, 7 << 29], [1 << 29, 3 << 29], [0, 1 << 31]])
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        lines = mpath_model.Lines(cos1024)
        for level in (-32768, 32767):
            parts = np.full((2, n_epochs * spe * 2), level, dtype=np.int16)
            for extra in (0, 1):
                gains = np.tile([32767, 32168 + extra], (n_epochs, 1))
                assert mpath_model.needs_int64(gains, rows) == bool(extra)
                assert _check(eng, lines, spe, parts, gains, [0, 1], rows) == parts.shape[1]
            # the 65535 row between two small ones (the int32 instance), the 65536 row among them (the int64 one)
            for extra in (0, 1):
                _check(eng, lines, spe, parts, np.array([[1, 0], [32767, 32168 + extra], [0, 129]]), [0, 1], rows)


def test_more_epochs_than_grid_rows(pkg, cos1024):
    """2051 epochs of 40 samples on a grid of 2048 rows: three blocks take a second epoch; every delay beyond 40 crosses epochs."""
    spe, n_epochs = 40, 2051
    rng = np.random.default_rng(14)
    parts = _parts(rng, 3, n_epochs, spe)
    gains = rng.integers(0, 300, size=(n_epochs, 3))
    rows = _random_rows(rng, n_epochs, 5)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        _check(eng, mpath_model.Lines(cos1024), spe, parts, gains, [0, 1, 2, 2, 0], rows)


def stride_case(name):
    """The inputs of test_stride_loops (tests/test_iq_launch_geometry_cpu.py asserts what they must be): 3 full-range parts, 8 echoes on
    the first and the last part whose delays every epoch draws from DELAYS and whose phase steps span the int32 range; gains small
    enough that most values stay inside the clamp (a clamped value hides its arithmetic) and some do not.  `wide_gains` are the
    gains with ONE row beyond 65535 (epoch `e_wide`): the int64 instance for the whole call.  `second` is a short call behind the long
    one whose echoes read the lines that the long call left."""
    spe, n_epochs = launch_model.GEOMETRIES[name]
    rng = np.random.default_rng(spe + n_epochs)
    parts = _edge_parts(rng, 3, n_epochs, spe)
    gains = rng.integers(0, 121, size=(n_epochs, 3))
    rows = _random_rows(rng, n_epochs, 8, 60)
    rows["dph"] = rng.integers(-(1 << 31), 1 << 31, size=rows.shape)
    e_wide = n_epochs // 2
    wide_gains = gains.copy()
    wide_gains[e_wide] = (32767, 32767, 2)
    rows2 = _random_rows(rng, 3, 8, 60)
    rows2["delay"][0] = (1024, 1023, 255, 5, 4, 3, 1, 0)
    second = (_edge_parts(rng, 3, 3, spe), rng.integers(0, 121, size=(3, 3)), rows2)
    return {"spe": spe, "n_epochs": n_epochs, "parts": parts, "gains": gains, "wide_gains": wide_gains, "e_wide": e_wide, "rows": rows,
            "pof": [0, 2, 2, 0, 2, 0, 0, 2], "second": second}


@pytest.mark.parametrize("name", list(launch_model.GEOMETRIES))
def test_stride_loops(pkg, cos1024, name):
    """Lanes that take a second vector (i += stride, where cap < need) and blocks that take a second epoch (e += gridDim.y): the phase
    m0 = 4 i - a and the delayed vector q of the second trip, against the model, in both instances.  Every long call is followed by a
    short one on the same handle that reads the lines the long call left."""
    case = stride_case(name)
    spe, parts = case["spe"], case["parts"]
    narrow, wide = launch_model.long_call_model(mpath_model.mpath, case, cos1024)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        for gains, (want, want_sat) in ((case["gains"], narrow), (case["wide_gains"], wide)):
            assert mpath_model.needs_int64(gains, case["rows"]) == (gains is case["wide_gains"])
            eng.mpath_reset()
            got, sat = _call(eng, parts, gains, case["pof"], case["rows"])
            _same(got, want, spe)
            assert sat == want_sat and 0 < sat < parts.shape[1]
            lines = mpath_model.Lines(cos1024)
            lines.lines[:3] = parts[:, -2 * mpath_model.H:]  # what a call of more than 1024 samples leaves
            p2, g2, r2 = case["second"]
            _check(eng, lines, spe, p2, g2, case["pof"], r2)


def test_table_regrows_between_calls(pkg, cos1024):
    """One handle, 3 epochs, then 4100 (the device table of the first call is too small), then 3 again."""
    spe = 7
    rng = np.random.default_rng(15)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        lines = mpath_model.Lines(cos1024)
        for n_epochs in (3, 4100, 3):
            _check(eng, lines, spe, _parts(rng, 3, n_epochs, spe), rng.integers(0, 300, size=(n_epochs, 3)), [0, 2, 2, 1],
                   _random_rows(rng, n_epochs, 4))


def test_no_echo_is_iq_wsum(pkg, cos1024):
    spe, n_epochs = 1030, 3
    rng = np.random.default_rng(16)
    parts = _edge_parts(rng, 5, n_epochs, spe)
    gains = rng.integers(0, 32768, size=(n_epochs, 5))
    want, want_sat = gain_model.wsum(parts, gains, spe)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        got, sat = _call(eng, parts, gains, [], None, [-1] * 5)
        _same(got, want, spe)
        assert sat == want_sat > 0
        import torch

        devs = [_dev(p) for p in parts]
        out = torch.zeros(parts.shape[1], dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        eng.iq_wsum([d.data_ptr() for d in devs], gains, out.data_ptr())
        eng.iq_saturated()
        assert np.array_equal(out.cpu().numpy(), got)


# ---- gal_synth_run_mpath ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch(pkg):
    """3 epochs, 4 channels; slot 3 comes up in epoch 1 only (GAL_CH_RESTART).  Shared, left unchanged: the records, the oracle's
    output and end state of the full run, and the oracle's output of every slot alone."""
    p = pkg.workloads.make_synthetic(n_epochs=3, n_chan=4, n_slots=16, samples_per_epoch=N, seed=79)
    p["prn"][0, 3] = 0
    p["flags"][0, 3] = 0
    p["flags"][1, 3] = pkg.GAL_CH_RESTART
    p["carr_phase0"][1, 3] = 0.37
    p["page_init"][1, 3] = p["page_init"][0, 3]
    full, full_st = oracle_run(p, N, FS)
    alone = np.stack([oracle_run(gain_model.slot_alone(p, s), N, FS)[0] for s in range(4)])
    for a in (p, full, full_st, alone):
        a.setflags(write=False)
    return p, full, full_st, alone


def _states_equal(st, ref_st):
    act = ref_st["prn"] > 0
    assert np.array_equal(st["prn"], ref_st["prn"])
    assert np.array_equal(st["carr_phase"][act].view(np.uint64), ref_st["carr_phase"][act].view(np.uint64))
    assert np.array_equal(st["page"][act], ref_st["page"][act])


def _run(eng, p, gains, sof, rows, state_in=None):
    import torch

    out = torch.zeros(p.shape[0] * N * 2, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    before = eng.iq_saturated()
    st = eng.run_mpath(p, gains, out.data_ptr(), sof, rows, state_in)
    sat = eng.iq_saturated() - before
    return out.cpu().numpy(), st, sat


def test_run_mpath_over_two_batches(pkg, cos1024, batch):
    """Echoes on slot 0 (two) and on slot 3, which is idle in the first epoch; slots 1 and 2 at one gain share a run.  Two batches with
    the state carried over: the bytes of the model over the oracle's per-slot streams in ONE call (the history follows the slot), the
    end states of the full run, three runs per batch."""
    p, full, full_st, alone = batch
    rng = np.random.default_rng(17)
    g = rng.integers(1, 700, size=p.shape)
    g[:, 2] = g[:, 1]
    echoes = [pkg.mpath_make(30.0 / 299792458.0 * 100, -6.0, 90.0, 3.0, FS), pkg.mpath_make(1024 / FS, -1.0, 200.0, -40.0, FS),
              pkg.mpath_make(5 / FS, 3.0, 10.0, 0.0, FS)]
    sof = [0, 0, 3]
    rows = np.stack([pkg.mpath_rows(e, g[:, s], 0, N) for e, s in zip(echoes, sof)], axis=1)
    assert rows.shape == (3, 3) and rows["delay"][0].tolist() == [26, 1024, 5]
    want, want_sat, _ = mpath_model.mpath(alone, g[:, :4], N, sof, rows, cos1024)
    plain, _ = gain_model.wsum(alone, g[:, :4], N)
    assert np.count_nonzero(want != plain) > 0.5 * want.size
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        a, st_a, sat_a = _run(eng, p[:2], g[:2], sof, rows[:2])
        assert eng.gain_runs() == 3
        b, st_b, sat_b = _run(eng, p[2:], g[2:], sof, rows[2:], st_a)
        assert eng.gain_runs() == 3
        _same(np.concatenate([a, b]), want, N)
        assert sat_a + sat_b == want_sat
        _states_equal(st_b, full_st)
        # no echoes: gal_synth_run_gains, the single-run unity case included
        got, st, sat = _run(eng, p, np.full(p.shape, 128), [], None)
        assert eng.gain_runs() == 1 and np.array_equal(got, full) and sat == 0
        _states_equal(st, full_st)
        got, _, _ = _run(eng, p, g, [], None)
        assert eng.gain_runs() == 3 and np.array_equal(got, plain)
        # after a reset the stream starts again
        eng.mpath_reset()
        a2, _, _ = _run(eng, p[:2], g[:2], sof, rows[:2])
        assert np.array_equal(a2, a)


def test_bad_arguments_and_call_order(pkg, batch):
    import torch

    p, _, _, _ = batch
    spe = N
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        out, a, b = (torch.zeros(3 * spe * 2 + 8, dtype=torch.int16, device="cuda") for _ in range(3))
        torch.cuda.synchronize()

        def refused(fn, *args):
            with pytest.raises(pkg.GalSynthError) as e:
                fn(*args)
            return e.value.code, str(e.value)

        g2 = np.full((3, 2), 128)
        rows = mpath_model.rows(3, 1, 64, 4)
        ptrs = [a.data_ptr(), b.data_ptr()]
        assert refused(eng.iq_mpath, ptrs, g2, out.data_ptr(), [1], rows, [0, -1])[0] == GAL_E_INVAL
        assert "no history line" in refused(eng.iq_mpath, ptrs, g2, out.data_ptr(), [1], rows, [0, -1])[1]
        assert "named by two parts" in refused(eng.iq_mpath, ptrs, g2, out.data_ptr(), [1], rows, [7, 7])[1]
        assert "hist_id 64" in refused(eng.iq_mpath, ptrs, g2, out.data_ptr(), [1], rows, [0, 64])[1]
        assert "hist_id -2" in refused(eng.iq_mpath, ptrs, g2, out.data_ptr(), [1], rows, [-2, 1])[1]
        assert "echo 0 on part 2" in refused(eng.iq_mpath, ptrs, g2, out.data_ptr(), [2], rows)[1]
        bad = rows.copy()
        bad["delay"][2, 0] = 1025
        assert "delay 1025" in refused(eng.iq_mpath, ptrs, g2, out.data_ptr(), [1], bad)[1]
        g_bad = g2.copy()
        g_bad[1, 1] = 32768
        assert refused(eng.iq_mpath, ptrs, g_bad, out.data_ptr(), [1], rows)[0] == GAL_E_INVAL
        assert refused(eng.iq_mpath, [a.data_ptr(), b.data_ptr() + 4], g2, out.data_ptr(), [1], rows)[0] == GAL_E_INVAL  # misaligned part
        assert refused(eng.iq_mpath, ptrs, g2, out.data_ptr() + 8, [1], rows)[0] == GAL_E_INVAL  # misaligned output
        assert "overlap" in refused(eng.iq_mpath, [a.data_ptr(), out.data_ptr() + 16], g2, out.data_ptr(), [1], rows)[1]
        assert refused(eng.iq_mpath, [a.data_ptr(), 0], g2, out.data_ptr(), [1], rows)[0] == GAL_E_INVAL
        assert refused(eng.iq_mpath, [], np.zeros((3, 0)), out.data_ptr(), [], None)[0] == GAL_E_INVAL
        assert refused(eng.iq_mpath, [a.data_ptr()] * 65, np.full((3, 65), 1), out.data_ptr(), [], None)[0] == GAL_E_INVAL
        eng.iq_mpath([a.data_ptr(), a.data_ptr()], g2, out.data_ptr(), [1], rows)  # parts may be one buffer
        eng.iq_saturated()
        # run_mpath: a slot outside the handle's, the refusals of run_gains
        g = np.full(p.shape, 128)
        assert "part 16" in refused(eng.run_mpath, p, g, out.data_ptr(), [16], rows)[1]
        assert refused(eng.run_mpath, p, g, out.data_ptr() + 2, [0], rows)[0] == GAL_E_INVAL
        with pytest.raises(ValueError):
            eng.run_mpath(p, g, out.data_ptr(), [0, 1], rows)
        # a batch in flight
        eng.plan(p)
        eng.execute(a.data_ptr())
        assert refused(eng.run_mpath, p, g, out.data_ptr(), [0], rows)[0] == GAL_E_STATE
        assert refused(eng.iq_mpath, ptrs, g2, out.data_ptr(), [1], rows)[0] == GAL_E_STATE
        eng.finish()
        eng.run_mpath(p, g, out.data_ptr(), [0], rows)
        eng.iq_mpath(ptrs, g2, out.data_ptr(), [1], rows)
        eng.iq_saturated()
