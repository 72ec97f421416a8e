"""Per-satellite ionospheric scintillation on the MI355X: k_iq_scint against the numpy model (tests/scint_model.py) -- bytes and
saturation count equal -- at the edges of a vector, a node interval, a tile and the grid, in place and out of place, many jobs in one
launch; three and four trips of the grid-stride loop at node lengths up to 2^24 and at the CLI's split; the stream in cuts; full-scale
input; the identity; the refusals; gal_synth_run_scint against the model over the oracle's per-slot streams; and one fading satellite
through the correlator bank."""
import ctypes

import numpy as np
import pytest

import gain_model
import scint_model
from oracle_binding import oracle_run
from tile_launch_model import SCINT_GEOMETRIES

pytestmark = pytest.mark.gpu

N = 26000
FS = 2.6e6
GAL_E_INVAL, GAL_E_STATE = -1, -4
SENTINEL = 0x5A5A
GUARD = 16  # int16 values behind every job's buffer that the kernel must leave alone
T = scint_model.TILE
LENGTHS = (1, 3, 4, 5, 63, 64, 65, 1023, 1025, 4099)
NODE_LENS = (64, 65, 67, 1000)
RICE = dict(a_q12=2500, b_q12=3000, seed=0x1234567890ABCDEF, stream=7)
RAYLEIGH = dict(a_q12=0, b_q12=2896, seed=3, stream=0x40B)


def _dev(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _input(rng, n, amp=12000):
    return rng.integers(-amp, amp + 1, 2 * n, dtype=np.int16)


def _differ(got, want):
    bad = np.flatnonzero(got != want)
    return "%d of %d differ (first at %d)" % (bad.size, got.size, bad[0] if bad.size else -1)


def _call(eng, specs):
    """One gal_synth_iq_scint call: specs = [(x, first_sample, row, in_place)].  Every job's buffers lie in one device array each for
    inputs and outputs, 16-byte aligned, GUARD sentinels behind each; returns ([output per job], saturated samples of the call)."""
    import torch

    offs, at = [], 0
    for x, _, _, _ in specs:
        offs.append(at)
        at += (x.size + GUARD + 7) // 8 * 8
    host = np.full(at, SENTINEL, dtype=np.int16)
    for o, (x, _, _, _) in zip(offs, specs):
        host[o:o + x.size] = x
    d_in = _dev(host)
    d_out = _dev(np.full(at, SENTINEL, dtype=np.int16))
    jobs = []
    for o, (x, first, row, in_place) in zip(offs, specs):
        src = d_in.data_ptr() + 2 * o
        jobs.append((src, src if in_place else d_out.data_ptr() + 2 * o, x.size // 2, first, row))
    before = eng.iq_saturated()
    eng.iq_scint(jobs)
    sat = eng.iq_saturated() - before
    got_in, got_out = d_in.cpu().numpy(), d_out.cpu().numpy()
    outs = []
    for o, (x, _, _, in_place) in zip(offs, specs):
        res, other = (got_in, got_out) if in_place else (got_out, got_in)
        outs.append(res[o:o + x.size].copy())
        assert (res[o + x.size:o + x.size + GUARD] == SENTINEL).all(), "the kernel wrote behind a job's last sample"
        if in_place:
            assert (other[o:o + x.size + GUARD] == SENTINEL).all(), "an in-place job wrote somewhere else"
        else:
            assert np.array_equal(other[o:o + x.size], x), "the input changed"
    del d_in, d_out
    torch.cuda.synchronize()
    return outs, sat


def _check(eng, specs):
    outs, sat = _call(eng, specs)
    want_sat = 0
    for k, (got, (x, first, row, _)) in enumerate(zip(outs, specs)):
        want, s = scint_model.apply(x, scint_model.row(**row), first)
        assert np.array_equal(got, want), "job %d (n %d, first %d, L %d): %s" % (k, x.size // 2, first, row["node_len"], _differ(got, want))
        want_sat += s
    assert sat == want_sat
    return want_sat


@pytest.fixture(scope="module")
def stream():
    x = _input(np.random.default_rng(5), 40 * T)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("L", NODE_LENS)
def test_lengths_and_first_samples_against_the_model(pkg, stream, L, in_place):
    """Every length at every first sample, 60 jobs in ONE launch: node boundaries inside a vector (L = 65, 67), n < L (L = 1000), a job
    over 64 nodes (n = 4099 at L = 64), a first sample that is no multiple of four, one far beyond 2^32."""
    row = dict(RICE, node_len=L)
    specs = [(stream[:2 * n], first, row, in_place) for first in (0, 1, 2, 3, L - 1, 2 ** 40 + 5) for n in LENGTHS]
    assert len(specs) == 60 and 4099 // 64 > 40
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        assert _check(eng, specs) == 0
    want, _ = scint_model.apply(stream[:2 * 4099], scint_model.row(**row), 0)
    assert not np.array_equal(want, stream[:2 * 4099])


def test_the_grid_stride_loop_runs_twice(pkg, stream):
    """64 jobs share the grid's MAX_BLOCKS blocks, 32 each: a job of 35 tiles and two samples takes a second trip in three blocks, the
    last of them a partial tile, with (j0, m0) stepped across the trips at an L that divides nothing."""
    per_job = scint_model.MAX_BLOCKS // 64
    n = (per_job + 3) * T + 2
    specs = [(stream[:8], k, dict(RICE, node_len=64), False) for k in range(63)]
    specs.append((stream[:2 * n], 2 ** 40 + 1, dict(RICE, node_len=67), True))
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        _check(eng, specs)
        # one job alone gets a block per tile.  (Three and four trips, at node lengths from 67 to 2^24 and at the CLI's 170 blocks per
        # job, are test_many_trips_* below.  What stays untested is n_jobs = 1 with more than MAX_BLOCKS tiles: a second trip at
        # bx = MAX_BLOCKS, a stride of 2^21 samples, needs more than 2.1 M samples in one job.)
        _check(eng, [(stream[:2 * (3 * T + 1)], 5, dict(RICE, node_len=1000), True)])


@pytest.fixture(scope="module")
def long_stream():
    """Input for the longest job of tile_launch_model.SCINT_GEOMETRIES; job k of a call reads it from its value 8 k on."""
    n = max(n for _, jobs in SCINT_GEOMETRIES.values() for n, _, _ in jobs)
    x = _input(np.random.default_rng(6), n + 4 * 64)
    x.setflags(write=False)
    return x


def _specs(name, long_stream, rows, in_place):
    """The named geometry's jobs as _check takes them: rows[L] (rows[L][k] where there are several jobs of one L) is the row without
    its node_len, in_place the set of job indices that run in place.  Every job has an input of its own."""
    n_jobs, jobs = SCINT_GEOMETRIES[name]
    specs = []
    for k, (n, first, L) in enumerate(jobs):
        r = rows[L][k] if isinstance(rows[L], list) else rows[L]
        specs.append((long_stream[8 * k:8 * k + 2 * n], first, dict(r, node_len=L), k in in_place))
    return specs


def test_many_trips_at_many_node_lengths(pkg, long_stream):
    """64 jobs, 32 blocks each: five jobs of 98 tiles take three and four trips at L = 1025 (a whole tile between two nodes), 40 000
    (above the stride: sj = 0, three nodes inside vectors), 162 500 (--scint at tau0 = 0.5 s: m0 grows for two steps before the correction
    fires), 2^24 (the largest: one node, five samples into the job) and 67.  tests/test_iq_launch_geometry_cpu.py asserts that the
    geometry has all of that, and on which steps the correction of (j0, m0) fires."""
    rows = {64: RICE, 1025: RICE, 40000: RAYLEIGH, 162500: dict(RICE, seed=77, stream=0x10B),
            1 << 24: dict(a_q12=0, b_q12=4096, seed=12, stream=0x40B), 67: RICE}
    specs = _specs("node_lens_at_four_trips", long_stream, rows, in_place={60, 62})
    assert [s[2]["node_len"] for s in specs[59:]] == [1025, 40000, 162500, 1 << 24, 67] and [s[3] for s in specs[59:]].count(True) == 2
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        _check(eng, specs)
    # the factor moves inside every long job; at L = 2^24 a sample's step is 1 / 4096 of the nodes' difference at best, so there the three
    # nodes themselves must differ (seed 12 was chosen for that): a tile that took its neighbour's pair of nodes would show
    for x, first, row, _ in specs[59:]:
        r, L = scint_model.row(**row), row["node_len"]
        if L < 1 << 24:
            zI, zQ = scint_model.factor(r, first, x.size // 2)
            assert np.ptp(zI) > 8 and np.ptp(zQ) > 8, L
        else:
            ZI, ZQ = scint_model.nodes(r, first // L, 3)
            assert min(np.abs(np.diff(ZI)).min(), np.abs(np.diff(ZQ)).min()) > 600


def test_many_trips_at_the_default_batchs_split(pkg, long_stream):
    """Twelve jobs -- the scintillating satellites of the default batch -- get 170 blocks each; at L = 162 500 the stride is (1, 11580)
    nodes and samples.  345 tiles and three samples per job: three trips.  Rician and Rayleigh rows in turn, every job with its own
    seed, stream, input and first sample."""
    rows = {162500: [dict(RAYLEIGH if k & 1 else RICE, seed=1000 + k, stream=(k << 8) | 11) for k in range(12)]}
    specs = _specs("cli_split", long_stream, rows, in_place={1, 2, 5, 8, 11})
    assert len(specs) == 12 and len({(s[2]["seed"], s[2]["stream"], s[1]) for s in specs}) == 12
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        _check(eng, specs)


def test_b0_at_four_trips(pkg, long_stream):
    """B = 0 (z = A: no draws, no sums, one barrier fewer per trip) over 98 tiles on 32 blocks, beside 63 jobs that draw; A = 3000 is
    not the identity."""
    rows = {64: RICE, 67: dict(a_q12=3000, b_q12=0, seed=9, stream=1)}
    specs = _specs("b0_at_four_trips", long_stream, rows, in_place={63})
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        _check(eng, specs)
    x, first, row, _ = specs[63]
    assert not np.array_equal(scint_model.apply(x[:64], scint_model.row(**row), first)[0], x[:64])


def test_three_jobs_of_different_lengths_rows_and_seeds_in_one_call(pkg, stream):
    specs = [(stream[:2 * 4099], 17, dict(RICE, node_len=64), True),
             (stream[100:100 + 2 * 1025], 2 ** 40 + 5, dict(a_q12=4000, b_q12=700, seed=9, stream=2, node_len=1000), False),
             (stream[300:300 + 2 * 65], 3, dict(RAYLEIGH, node_len=67), False)]
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        outs, _ = _call(eng, specs)
        _check(eng, specs)
        # another seed, another stream, another row: other bytes
        for change in (dict(seed=RICE["seed"] + 1), dict(stream=8), dict(b_q12=2999)):
            other, _ = _call(eng, [(specs[0][0], 17, dict(specs[0][2], **change), False)])
            assert not np.array_equal(other[0], outs[0])


@pytest.mark.parametrize("first", [0, 2 ** 40 + 5])
def test_any_cut_into_calls_is_the_single_call(pkg, stream, first):
    n = 4099
    x = stream[:2 * n]
    row = dict(RICE, node_len=65)
    want, want_sat = scint_model.apply(x, scint_model.row(**row), first)
    rng = np.random.default_rng(7)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        for pieces in (2, 3, 2, 3, 3):
            cuts = [0] + sorted(int(c) for c in rng.choice(np.arange(1, n), pieces - 1, replace=False)) + [n]
            outs, sat = [], 0
            for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                got, s = _call(eng, [(x[2 * a:2 * b].copy(), first + a, row, bool(k & 1))])
                outs.append(got[0])
                sat += s
            got = np.concatenate(outs)
            assert np.array_equal(got, want), "cuts %s: %s" % (cuts, _differ(got, want))
            assert sat == want_sat


def test_full_scale_input_clamps_and_counts(pkg):
    n = 3 * T + 3
    rng = np.random.default_rng(9)
    x = rng.choice(np.array([-32768, 32767, -26000, 26000], dtype=np.int16), 2 * n)
    x[0:8] = (-32768, -32768, 32767, 32767, -32768, 32767, 32767, -32768)
    # the Rayleigh row of gal_synth_scint_make and the largest row there is: |z| reaches the node clamp
    rows = [dict(pkg.scint_make(1.0, 64 * 8 / FS, FS), seed=11, stream=5), dict(a_q12=4096, b_q12=4096, seed=12, stream=6, node_len=64)]
    assert rows[0]["a_q12"] == 0 and rows[0]["b_q12"] > 2800
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        for row in rows:
            want, want_sat = scint_model.apply(x, scint_model.row(**row), 11)
            assert 0 < want_sat < n and (want == 32767).any() and (want == -32768).any()
            assert _check(eng, [(x, 11, row, False)]) == want_sat
    ZI, ZQ = scint_model.nodes(scint_model.row(**rows[1]), 0, 3 * T // 64 + 2)
    assert max(np.abs(ZI).max(), np.abs(ZQ).max()) > 2 * 4096


def test_the_identity_row_is_a_bit_exact_copy(pkg):
    rng = np.random.default_rng(10)
    x = rng.integers(-32768, 32768, 2 * (2 * T + 3), dtype=np.int16)
    x[:4] = (-32768, -32768, 32767, 32767)
    ident = dict(node_len=777)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        outs, sat = _call(eng, [(x, 5, ident, False), (x, 2 ** 40, ident, True), (x[:6], 1, ident, False)])
        assert all(np.array_equal(o, x[:o.size]) for o in outs) and sat == 0


def test_bad_arguments_and_overlap_are_refused(pkg):
    import torch

    lib = pkg.load_library()
    Job, Row = pkg.synth._ScintJob, pkg.synth._Scint
    n = 4096
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        buf = torch.zeros(8 * n + 64, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        a = buf.data_ptr()

        def row(**kw):
            r = pkg.synth._scint_struct(dict(RICE, node_len=64))
            for k, v in kw.items():
                setattr(r, k, v)
            return r

        def call(*jobs):
            arr = (Job * max(1, len(jobs)))(*jobs)
            return lib.gal_synth_iq_scint(eng._h, arr, len(jobs))

        good = Job(a, a + 4 * n, n, 0, row())
        assert call(good) == 0
        assert lib.gal_synth_iq_scint(None, (Job * 1)(good), 1) == GAL_E_INVAL
        assert lib.gal_synth_iq_scint(eng._h, None, 1) == GAL_E_INVAL
        assert call() == GAL_E_INVAL  # n_jobs = 0
        many = [Job(a + 64 * k, a + 64 * k, 16, 0, row()) for k in range(65)]
        assert call(*many) == GAL_E_INVAL and call(*many[:64]) == 0
        assert call(Job(None, a, n, 0, row())) == GAL_E_INVAL and call(Job(a, None, n, 0, row())) == GAL_E_INVAL
        assert call(Job(a + 4, a + 4 * n, n, 0, row())) == GAL_E_INVAL and call(Job(a, a + 4 * n + 8, n, 0, row())) == GAL_E_INVAL  # alignment
        assert call(Job(a, a + 16, n, 0, row())) == GAL_E_INVAL and call(Job(a + 16, a, n, 0, row())) == GAL_E_INVAL  # partial overlap
        assert call(Job(a, a + 4 * n - 16, n, 0, row())) == GAL_E_INVAL
        assert call(Job(a, a, n, 0, row())) == 0  # exactly in place
        # between jobs: an output that meets another job's input or output
        assert call(Job(a, a, n, 0, row()), Job(a + 8 * n, a + 16, n, 0, row())) == GAL_E_INVAL
        assert call(Job(a, a + 4 * n, n, 0, row()), Job(a + 12 * n, a + 4 * n + 16, n, 0, row())) == GAL_E_INVAL
        assert call(Job(a, a, n, 0, row()), Job(a, a + 4 * n, n, 0, row())) == GAL_E_INVAL
        assert call(Job(a, a + 4 * n, n, 0, row()), Job(a, a + 8 * n, n, 0, row())) == 0  # two jobs may read one input
        assert call(Job(a, a, n, 0, row(reserved=1))) == GAL_E_INVAL
        assert call(Job(a, a, n, 0, row(node_len=63))) == GAL_E_INVAL
        assert call(Job(a, a, n, 0, row(node_len=(1 << 24) + 1))) == GAL_E_INVAL
        assert call(Job(a, a, n, 0, row(a_q12=4097))) == GAL_E_INVAL and call(Job(a, a, n, 0, row(b_q12=4097))) == GAL_E_INVAL
        assert call(Job(a, a, 1 << 41, 0, row())) == GAL_E_INVAL
        assert call(Job(a, a, n, 1 << 62, row())) == GAL_E_INVAL
        assert call(good, Job(a + 8 * n, a + 8 * n, n, 0, row(node_len=63))) == GAL_E_INVAL  # any job of the call
        assert call(Job(a, a, 0, 0, row())) == 0
        eng.iq_saturated()
        assert not buf.cpu().numpy().any()  # zeros stay zeros: no refused call wrote


def test_buffer_of_the_batch_in_flight_is_refused(pkg):
    import torch

    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=4, n_slots=16, samples_per_epoch=N, seed=12)
    row = dict(RICE, node_len=64)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as e:
        iq = torch.zeros(2 * N * 2, dtype=torch.int16, device="cuda")
        other = torch.zeros(2 * N * 2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        e.plan(p)
        e.execute(iq.data_ptr())
        for src, dst in ((iq, other), (other, iq), (iq, iq)):
            with pytest.raises(pkg.GalSynthError) as ei:
                e.iq_scint([(src.data_ptr(), dst.data_ptr(), 2 * N, 0, row)])
            assert ei.value.code == GAL_E_STATE
        e.finish()
        e.iq_scint([(iq.data_ptr(), iq.data_ptr(), 2 * N, 0, row)])
        e.iq_saturated()


# ---- gal_synth_run_scint ---------------------------------------------------------------------------------------------------------
def _run(eng, p, gains, rows, first):
    import torch

    out = torch.zeros(p.shape[0] * N * 2, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    before = eng.iq_saturated()
    st = eng.run_scint(p, gains, out.data_ptr(), rows, first)
    sat = eng.iq_saturated() - before
    return out.cpu().numpy(), st, sat


def test_run_scint_against_the_model_over_the_slots_own_streams(pkg):
    """Two epochs of 26000 samples, three satellites; slot 1 scintillates.  NULL rows: gal_synth_run_mpath.  With a row: the model
    applied to slot 1's own stream (the oracle's, alone), summed with the others by the weighted sum's model; slots 0 and 2 at one gain
    share a run.  A row that changes between the epochs makes two jobs."""
    first = 5 * 2 * N + 2 ** 33
    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=3, n_slots=16, samples_per_epoch=N, seed=81)
    alone = np.stack([oracle_run(gain_model.slot_alone(p, s), N, FS)[0].view(np.int16).ravel() for s in range(3)])
    g = np.full(p.shape, 128)
    g[:, :3] = (300, 128, 300)
    row = dict(pkg.scint_make(0.8, 0.02, FS), node_len=1000, seed=4, stream=(0 << 8) | int(p["prn"][0, 1]))
    rows = pkg.scint_rows({1: row}, 2, 16)
    faded, fsat = scint_model.apply(alone[1], scint_model.row(**row), first)
    assert fsat == 0 and not np.array_equal(faded, alone[1])
    want, want_sat = gain_model.wsum(np.stack([alone[0], faded, alone[2]]), g[:, :3], N)
    plain, _ = gain_model.wsum(alone, g[:, :3], N)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        import torch

        ref = torch.zeros(2 * N * 2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        st_ref = eng.run_mpath(p, g, ref.data_ptr())
        eng.iq_saturated()
        runs_ref = eng.gain_runs()
        got, st, sat = _run(eng, p, g, None, first)
        assert np.array_equal(got, ref.cpu().numpy()) and np.array_equal(got, plain) and eng.gain_runs() == runs_ref == 2
        assert st.tobytes() == st_ref.tobytes()
        # identity rows for every slot: the same bytes, no extra run
        got, _, _ = _run(eng, p, g, pkg.scint_rows({}, 2, 16), first)
        assert np.array_equal(got, plain) and eng.gain_runs() == 2
        got, st, sat = _run(eng, p, g, rows, first)
        assert eng.gain_runs() == 2  # slot 1 was a run of its own already: its gain differs
        assert np.array_equal(got, want), _differ(got, want)
        assert sat == want_sat and st.tobytes() == st_ref.tobytes()
        # at the others' gain slot 1 would share their run: the row makes it a run of its own
        g1 = np.full(p.shape, 300)
        want1, _ = gain_model.wsum(np.stack([alone[0], faded, alone[2]]), g1[:, :3], N)
        got, _, _ = _run(eng, p, g1, None, first)
        assert eng.gain_runs() == 1
        got, _, _ = _run(eng, p, g1, rows, first)
        assert eng.gain_runs() == 2 and np.array_equal(got, want1), _differ(got, want1)
        # another row in the second epoch: two jobs, each with its own first sample
        rows2 = rows.copy()
        rows2["seed"][1, 1] = 5
        f0, _ = scint_model.apply(alone[1][:2 * N], scint_model.row(**row), first)
        f1, _ = scint_model.apply(alone[1][2 * N:], scint_model.row(**dict(row, seed=5)), first + N)
        want2, _ = gain_model.wsum(np.stack([alone[0], np.concatenate((f0, f1)), alone[2]]), g[:, :3], N)
        got, _, _ = _run(eng, p, g, rows2, first)
        assert np.array_equal(got, want2), _differ(got, want2)
        # refusals: a row the check refuses, a first sample beyond 2^62
        bad = rows.copy()
        bad["node_len"][1, 5] = 63
        for r, f in ((bad, first), (rows, 1 << 62)):
            with pytest.raises(pkg.GalSynthError) as ei:
                eng.run_scint(p, g, ref.data_ptr(), r, f)
            assert ei.value.code == GAL_E_INVAL


def test_a_fading_satellite_through_the_correlator(pkg):
    """One satellite of the oracle at 4.092 MS/s, 34 code periods; s4 = 0.8 made with tau0 = 20 ms and L overridden to 1000 so that the
    run stays short (tau0 = 8000 samples = half a code period: deep fades within the run).  The correlator's unit of time is the code
    period of 4 ms: the prompt power |S_B|^2 + |S_C|^2 of every whole period follows |the mean of z over the period's samples|^2 of the
    model -- what a coherent sum over a period sees of z.  Noise-free, so only quantisation stands against it: the correlation
    coefficient exceeds 0.99."""
    import torch

    fs, periods = 4.092e6, 34
    spe = periods * 16368
    p = pkg.workloads.make_synthetic(n_epochs=1, n_chan=1, n_slots=16, samples_per_epoch=spe, sample_rate=fs, prns=[11], seed=77)
    iq, _ = oracle_run(p, spe, fs)
    iq = np.ascontiguousarray(iq).view(np.int16).ravel()
    row = dict(pkg.scint_make(0.8, 0.02, fs), node_len=1000, seed=21, stream=11)
    first = 12345
    q = pkg.corr_from_epoch(p[0, 0], fs, 0, max_periods=periods)
    zI, zQ = scint_model.factor(scint_model.row(**row), first, spe)
    z = (zI + 1j * zQ) / 4096.0
    code = (q["code_ph0"] + np.arange(spe, dtype=np.uint64) * np.uint64(q["code_dph"])) >> np.uint64(32)
    m = (code // np.uint64(2 * 4092)).astype(np.int64)
    whole = np.arange(1, m.max())  # period 0 and the last one are cut by the run
    model = np.array([np.abs(z[m == k].mean()) ** 2 for k in whole])
    y_model, sat_model = scint_model.apply(iq, scint_model.row(**row), first)
    with pkg.SynthEngine(sample_rate=fs, samples_per_epoch=spe, n_slots=16, device=0) as eng:
        d = _dev(iq)
        before = eng.iq_saturated()
        eng.iq_scint([(d.data_ptr(), d.data_ptr(), spe, first, row)])
        assert eng.iq_saturated() - before == sat_model == 0
        assert np.array_equal(d.cpu().numpy(), y_model)
        s = np.asarray(eng.correlate(d.data_ptr(), "ishort", spe, q), dtype=np.float64)[:, 0, 0]
        torch.cuda.synchronize()
    power = (s[:, 0] ** 2 + s[:, 1] ** 2 + s[:, 2] ** 2 + s[:, 3] ** 2)[whole]
    rho = float(np.corrcoef(power, model)[0, 1])
    print("%d periods: power max / min %.1f, model max / min %.1f, correlation %.5f" % (whole.size, power.max() / power.min(),
                                                                                      model.max() / model.min(), rho))
    assert whole.size >= 30 and model.max() / model.min() > 10
    assert rho > 0.99
