"""gal_synth_run_scint and gal_synth_run_array on the MI355X against the composed model (tests/compose_model.py) over the oracle's
per-slot streams -- bytes, saturation count, runs and end states, exact: echoes of the scintillated stream over a batch boundary; rows
that come and go inside a batch, on an idle slot and with a PRN change; 64, 65 and 70 scintillation jobs in one batch (the job table
is used twice); a row change at an epoch that begins inside a 16-byte vector, refused, and its accepted neighbour; the array with
scintillation.  Every case says on the CPU whether anything clamps before the GPU is asked."""
import numpy as np
import pytest

import compose_model
import gain_model
import mpath_model
from compose_model import N, FS
from oracle_binding import oracle_run

pytestmark = pytest.mark.gpu

GAL_E_INVAL = -1
SENTINEL = 0x5A5A


@pytest.fixture(scope="module")
def cos1024(pkg):
    return pkg.tables()["cos1024"]


def _alone(p, cuts, n, spe=N):
    """The oracle's stream of every slot 0 .. n - 1 on its own, batch by batch with the state chained: ([batch][n, n_val], [batch][n]
    end states of the slots' own runs)."""
    streams, states = [[] for _ in cuts], [[] for _ in cuts]
    for s in range(n):
        st = None
        for k, (a, b) in enumerate(cuts):
            iq, st = oracle_run(gain_model.slot_alone(p[a:b], s), spe, FS, state_in=st)
            streams[k].append(iq)
            states[k].append(st[s].copy())
    return [np.stack(x) for x in streams], states


def _same(got, want, spe=N):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d of %d values differ, the first at %d = epoch %d, sample %d" % (bad.size, got.size, bad[0], bad[0] // (2 * spe),
                                                                                             bad[0] % (2 * spe) // 2)


def _state_is(st, ref):
    assert st["prn"] == ref["prn"] and st["carr_phase"].tobytes() == ref["carr_phase"].tobytes() and np.array_equal(st["page"], ref["page"])


def _out(n_val, n=1):
    import torch

    outs = [torch.full((n_val + 16,), SENTINEL, dtype=torch.int16, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    return outs


def _fetch(outs, n_val):
    got = np.stack([o.cpu().numpy() for o in outs])
    assert (got[:, n_val:] == SENTINEL).all(), "written behind the batch"
    return got[:, :n_val]


def _run_scint(eng, p, g, rows, first, sof=(), echo_rows=None, state_in=None, spe=N):
    out = _out(p.shape[0] * spe * 2)
    before = eng.iq_saturated()
    st = eng.run_scint(p, g, out[0].data_ptr(), rows, first, sof, echo_rows, state_in)
    sat = eng.iq_saturated() - before
    return _fetch(out, p.shape[0] * spe * 2)[0], st, sat


def _run_array(eng, p, g, phase, rows, first, state_in=None, spe=N):
    outs = _out(p.shape[0] * spe * 2, phase.shape[1])
    before = eng.iq_saturated()
    st = eng.run_array(p, g, phase, [o.data_ptr() for o in outs], rows, first, state_in)
    sat = eng.iq_saturated() - before
    return _fetch(outs, p.shape[0] * spe * 2), st, sat


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
def test_echoes_of_the_scintillated_stream_over_a_batch_boundary(pkg, cos1024):
    """compose_model.echo_fade_case in two chained batches of three epochs, first_sample = 2^33 + 10 N: slot 1's echoes (delay 1;
    delay 1024 with dph != 0) are echoes of its faded stream, and in the first 1024 samples of the second batch they come from the
    history line, which holds the first batch's faded samples.  tests/test_compose_model_cpu.py shows that the model's bytes differ
    for either pass order and for a stale line.  Then the six epochs as one batch: the same bytes."""
    c = compose_model.echo_fade_case(pkg)
    p, g, rows, sof, er, first = (c[k] for k in ("params", "gains", "scint_rows", "slot_of_echo", "echo_rows", "first_sample"))
    cuts = [(0, 3), (3, 6)]
    alone, states = _alone(p, cuts, 4)
    lines, want = mpath_model.Lines(cos1024), []
    for k, (a, b) in enumerate(cuts):
        y, sat = compose_model.run_model(alone[k], p[a:b], g[a:b], rows[a:b], first + a * N, N, lines, sof, er[a:b], cos1024)
        assert sat == 0
        want.append(y)
    fresh, _ = compose_model.run_model(alone[1], p[3:], g[3:], rows[3:], first + 3 * N, N, None, sof, er[3:], cos1024)
    assert np.flatnonzero(fresh != want[1]).size > 1000  # the second batch does depend on the line
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        st = None
        for k, (a, b) in enumerate(cuts):
            got, st, sat = _run_scint(eng, p[a:b], g[a:b], rows[a:b], first + a * N, sof, er[a:b], st)
            assert eng.gain_runs() == 4  # slot 0, and one each for the slots that fade or carry an echo
            _same(got, want[k])
            assert sat == 0
            for s in range(4):
                _state_is(st[s], states[k][s])
        eng.mpath_reset()
        got, st, sat = _run_scint(eng, p, g, rows, first, sof, er)
        _same(got, np.concatenate(want))
        assert sat == 0
        for s in range(4):
            _state_is(st[s], states[1][s])


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------
def test_rows_that_come_and_go_inside_a_batch(pkg, cos1024):
    """Four epochs.  Slot 1: the identity, a Rice row in epochs 1-2, the identity -- one job of two epochs at first_sample + N.  Slot 2
    keeps a Rayleigh row through epoch 1, in which it is idle: zeros stay zeros, its weight there is 0.  Slot 3 changes its PRN at epoch
    2 (GAL_CH_RESTART) and its row with it: two jobs.  Through run_scint, with a gain of 32767 in one epoch so that the sum clamps and
    the count is the model's, and through run_array with two elements."""
    E, first = 4, 2 ** 35 + 3 * 4 * N
    p = pkg.workloads.make_synthetic(n_epochs=E, n_chan=4, n_slots=16, samples_per_epoch=N, seed=92)
    p["prn"][1, 2] = 0
    p["flags"][2, 2] = pkg.GAL_CH_RESTART
    p["carr_phase0"][2, 2] = 0.21
    p["page_init"][2, 2] = p["page_init"][0, 2]
    p["prn"][2:, 3] = 30
    p["flags"][2, 3] = pkg.GAL_CH_RESTART
    p["carr_phase0"][2, 3] = 0.37
    p["page_init"][2, 3] = p["page_init"][0, 3]
    rice, ray = dict(pkg.scint_make(0.7, 0.02, FS), node_len=1000, seed=8), dict(pkg.scint_make(1.0, 0.01, FS), node_len=900, seed=8)
    rows = pkg.scint_rows({2: dict(ray, stream=int(p["prn"][0, 2]))}, E, 16)
    r1 = pkg.scint_rows({1: dict(rice, stream=int(p["prn"][0, 1]))}, E, 16)
    rows[1:3, 1] = r1[1:3, 1]
    rows[:2, 3] = pkg.scint_rows({3: dict(rice, stream=int(p["prn"][0, 3]))}, E, 16)[:2, 3]
    rows[2:, 3] = pkg.scint_rows({3: dict(rice, stream=30)}, E, 16)[2:, 3]
    assert [(a, b) for a, b, _ in compose_model.spans(rows, 1)] == [(1, 3)]
    assert [(a, b) for a, b, _ in compose_model.spans(rows, 2)] == [(0, 4)]
    assert [(a, b) for a, b, _ in compose_model.spans(rows, 3)] == [(0, 2), (2, 4)]
    rng = np.random.default_rng(93)
    g = rng.integers(1, 700, size=p.shape)
    g[3, 0] = 32767
    alone, states = _alone(p, [(0, E)], 4)
    alone, states = alone[0], states[0]
    assert not alone[2, 2 * N:4 * N].any()
    want, want_sat = compose_model.run_model(alone, p, g, rows, first, N)
    assert want_sat > 0
    ga = np.minimum(g, 1023)
    phase = rng.integers(0, 1 << 32, size=(E, 2, 16), dtype=np.uint64)
    want_a, want_a_sat = compose_model.array_model_run(alone, p, ga, phase, rows, first, N, cos1024)
    assert want_a_sat == 0
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        got, st, sat = _run_scint(eng, p, g, rows, first)
        assert eng.gain_runs() == 4
        _same(got, want)
        assert sat == want_sat
        for s in range(4):
            _state_is(st[s], states[s])
        got, st, sat = _run_array(eng, p, ga, phase, rows, first)
        assert eng.gain_runs() == 4
        for a in range(2):
            _same(got[a], want_a[a])
        assert sat == 0
        for s in range(4):
            _state_is(st[s], states[s])


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_alt,n_const,E,n_jobs", [(5, 0, 14, 70), (4, 0, 16, 64), (4, 1, 16, 65)])
def test_more_jobs_than_one_call_takes(pkg, n_alt, n_const, E, n_jobs):
    """n_alt slots whose seed alternates from epoch to epoch -- a job per slot and epoch -- and n_const slots with one row: 64 jobs are
    one gal_synth_iq_scint call, 65 and 70 are two on the one job table, and the second waits for the first.  Gains of 1 to 2.3: the
    model says that nothing clamps."""
    n, first = n_alt + n_const, 2 ** 34 + 7
    p = pkg.workloads.make_synthetic(n_epochs=E, n_chan=n, n_slots=16, samples_per_epoch=N, seed=94)
    base = dict(pkg.scint_make(0.6, 0.02, FS), node_len=1000)
    rows = pkg.scint_rows({s: dict(base, seed=20, stream=int(p["prn"][0, s])) for s in range(n)}, E, 16)
    rows["seed"][1::2, :n_alt] = 21
    assert sum(len(compose_model.spans(rows, s)) for s in range(16)) == n_jobs
    g = np.full(p.shape, 128)
    g[:, :n] = 128 + 40 * np.arange(n)
    alone, states = _alone(p, [(0, E)], n)
    want, want_sat = compose_model.run_model(alone[0], p, g, rows, first, N)
    assert want_sat == 0
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        got, st, sat = _run_scint(eng, p, g, rows, first)
        assert eng.gain_runs() == n
        _same(got, want)
        assert sat == 0
        for s in range(n):
            _state_is(st[s], states[0][s])


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
def test_a_row_change_inside_a_vector_is_refused_and_its_neighbour_is_not(pkg):
    """26001 samples per epoch, six epochs.  A row that begins at epoch 1 would begin at sample 26001, inside a 16-byte vector: refused
    with the slot and the epoch in the text, nothing written, the handle as good as before.  The same rows beginning at epoch 4 --
    4 x 26001 is a multiple of 4 -- equal the model; the job starts at first_sample + 104004.  (Six epochs of 26001 samples are no
    multiple of 16 bytes either: the parts of the batch lie on 16-byte addresses all the same.)"""
    spe, E, first = 26001, 6, 2 ** 33 + 11
    p = pkg.workloads.make_synthetic(n_epochs=E, n_chan=3, n_slots=16, samples_per_epoch=spe, seed=95)
    rice = dict(pkg.scint_make(0.7, 0.02, FS), node_len=1000, seed=9)
    whole = pkg.scint_rows({1: dict(rice, stream=int(p["prn"][0, 1])), 2: dict(rice, stream=int(p["prn"][0, 2]))}, E, 16)
    ident = pkg.scint_rows({}, E, 16)
    at1, at4 = whole.copy(), whole.copy()
    at1[:1, 1] = ident[:1, 1]
    at4[:4, 1] = ident[:4, 1]
    assert [(a, b) for a, b, _ in compose_model.spans(at4, 1)] == [(4, 6)] and (4 * spe) % 4 == 0 and spe % 4 == 1
    g = np.full(p.shape, 128)
    g[:, :3] = (200, 333, 150)
    alone, states = _alone(p, [(0, E)], 3, spe)
    want, want_sat = compose_model.run_model(alone[0], p, g, at4, first, spe)
    plain, _ = gain_model.wsum(alone[0], g[:, :3], spe)
    assert want_sat == 0 and not np.array_equal(want, plain)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        out = _out(E * spe * 2)
        with pytest.raises(pkg.GalSynthError) as ei:
            eng.run_scint(p, g, out[0].data_ptr(), at1, first)
        assert ei.value.code == GAL_E_INVAL
        assert "slot 1" in str(ei.value) and "epoch 1" in str(ei.value) and "a multiple of 4 only" in str(ei.value), str(ei.value)
        eng.iq_saturated()
        assert (out[0].cpu().numpy() == SENTINEL).all()
        got, st, sat = _run_scint(eng, p, g, at4, first, spe=spe)
        assert eng.gain_runs() == 3
        _same(got, want, spe)
        assert sat == 0
        for s in range(3):
            _state_is(st[s], states[0][s])
        # a row that is there from the first epoch on, and none at all: the weighted sum at this epoch length
        got, _, _ = _run_scint(eng, p, g, ident, first, spe=spe)
        assert eng.gain_runs() == 3
        _same(got, plain, spe)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------
def test_run_array_with_scintillation_over_two_batches(pkg, cos1024):
    """Two chained batches of three epochs, four satellites, three elements, random gains up to 1023 and random phases; slots 1 and 3
    fade.  All three elements, the count and the states are array_model_run's.  One element with every phase 0 is run_scint's bytes of
    the same call."""
    E, K, first = 3, 3, 2 ** 33 + 4 * N
    full = pkg.workloads.make_synthetic(n_epochs=2 * E, n_chan=4, n_slots=16, samples_per_epoch=N, seed=96)
    rng = np.random.default_rng(97)
    g = rng.integers(0, 1024, size=full.shape)
    g[1, 2] = 1023
    phase = rng.integers(0, 1 << 32, size=(2 * E, K, 16), dtype=np.uint64)
    rows = pkg.scint_rows({1: dict(pkg.scint_make(0.8, 0.02, FS), node_len=1000, seed=12, stream=int(full["prn"][0, 1])),
                           3: dict(pkg.scint_make(0.5, 0.05, FS), node_len=650, seed=12, stream=int(full["prn"][0, 3]))}, 2 * E, 16)
    cuts = [(0, E), (E, 2 * E)]
    alone, states = _alone(full, cuts, 4)
    want = [compose_model.array_model_run(alone[k], full[a:b], g[a:b], phase[a:b], rows[a:b], first + a * N, N, cos1024) for k, (a, b) in enumerate(cuts)]
    assert all(w[1] == 0 for w in want)  # gains up to 8 on satellites of a few hundred LSB: nothing clamps
    unfaded, _ = compose_model.array_model_run(alone[0], full[:E], g[:E], phase[:E], None, first, N, cos1024)
    assert np.count_nonzero(unfaded != want[0][0]) > 0.3 * unfaded.size
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        st = st_one = st_ref = None
        for k, (a, b) in enumerate(cuts):
            got, st, sat = _run_array(eng, full[a:b], g[a:b], phase[a:b], rows[a:b], first + a * N, st)
            assert eng.gain_runs() == 4
            for el in range(K):
                _same(got[el], want[k][0][el])
            assert sat == want[k][1]
            for s in range(4):
                _state_is(st[s], states[k][s])
            one, st_one, sat_one = _run_array(eng, full[a:b], g[a:b], np.zeros((E, 1, 16)), rows[a:b], first + a * N, st_one)
            ref, st_ref, sat_ref = _run_scint(eng, full[a:b], g[a:b], rows[a:b], first + a * N, state_in=st_ref)
            assert one[0].tobytes() == ref.tobytes() and sat_one == sat_ref
            assert st_one.tobytes() == st_ref.tobytes() == st.tobytes()
