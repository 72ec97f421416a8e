"""Per-satellite signal power on the MI355X: k_iq_wsum against the numpy model (tests/gain_model.py) on random int16 streams, and
gal_synth_run_gains against the model over the oracle's output of every slot on its own -- bytes, saturation count and channel state."""
import numpy as np
import pytest

import gain_model
from oracle_binding import oracle_run

pytestmark = pytest.mark.gpu

N = 26000
FS = 2.6e6
GAL_E_INVAL, GAL_E_STATE = -1, -4
EDGE_GAINS = (0, 1, 128, 129, 32767)


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


def _wsum_case(eng, spe, parts, gains):
    devs = [_dev(p) for p in parts]
    out = _empty(parts.shape[1])
    before = eng.iq_saturated()
    eng.iq_wsum([d.data_ptr() for d in devs], gains, out.data_ptr())
    sat = eng.iq_saturated() - before
    want, want_sat = gain_model.wsum(parts, gains, spe)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), "%d of %d values differ (first at %d)" % (np.count_nonzero(got != want), got.size, np.flatnonzero(got != want)[0])
    assert sat == want_sat
    return want_sat


# "mixed": every row's gains sum to less than 65536 (the int32 instance); "max": rows of 32767s (the int64 instance)
@pytest.mark.parametrize("n_parts,kind", [(1, "mixed"), (3, "mixed"), (3, "max"), (16, "mixed16")])
def test_wsum_against_the_model(pkg, n_parts, kind):
    rng = np.random.default_rng(1000 + n_parts)
    parts = rng.integers(-32768, 32768, size=(n_parts, 3 * N * 2), dtype=np.int16)
    parts[:, :8] = 32767  # full scale on every part at once, both signs
    parts[:, 8:16] = -32768
    if kind == "mixed" and n_parts == 1:
        cases = [np.array([[0], [1], [128]]), np.array([[129], [32767], [128]])]
    elif kind == "mixed":
        cases = [np.array([[0, 1, 128], [129, 32767, 128], [128, 128, 128]])]
    elif kind == "max":
        cases = [np.array([[32767, 32767, 32767], [32767, 0, 32767], [1, 129, 128]])]
    else:  # 16 parts: every edge gain several times in every epoch, sums far beyond an int32 at full scale
        cases = [rng.choice(EDGE_GAINS, size=(3, n_parts))]
        cases[0][:, :5] = EDGE_GAINS
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        sat = [_wsum_case(eng, N, parts, g) for g in cases]
        if kind != "mixed" or n_parts == 3:
            assert max(sat) > 0
        if n_parts == 1:  # unity: the stream itself, nothing clamped
            assert _wsum_case(eng, N, parts, np.full((3, 1), 128)) == 0


@pytest.mark.parametrize("spe", [26001, 26002, 7])
def test_wsum_epochs_that_end_inside_a_vector(pkg, spe):
    """samples_per_epoch not a multiple of 4: epoch boundaries fall inside 16-byte vectors, the gain changes there."""
    rng = np.random.default_rng(spe)
    parts = rng.integers(-3000, 3000, size=(3, 3 * spe * 2), dtype=np.int16)
    gains = np.array([[0, 1, 128], [129, 300, 128], [32767, 128, 5]])
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        _wsum_case(eng, spe, parts, gains)
        _wsum_case(eng, spe, parts[:, :2 * spe * 2], gains[:2])


@pytest.fixture(scope="module")
def batch(pkg):
    """3 epochs, 4 channels; slot 3 comes up in epoch 1 only (GAL_CH_RESTART).  Shared, left unchanged: the records, the oracle's
    output and end state of the full run, and the oracle's output of every slot alone."""
    p = pkg.workloads.make_synthetic(n_epochs=3, n_chan=4, n_slots=16, samples_per_epoch=N, seed=77)
    p["prn"][0, 3] = 0
    p["flags"][0, 3] = 0
    p["flags"][1, 3] = pkg.GAL_CH_RESTART
    p["carr_phase0"][1, 3] = 0.37
    p["page_init"][1, 3] = p["page_init"][0, 3]
    full, full_st = oracle_run(p, N, FS)
    alone = np.stack([oracle_run(gain_model.slot_alone(p, s), N, FS)[0] for s in range(4)])
    assert np.array_equal(alone.astype(np.int32).sum(axis=0), full.astype(np.int32))  # the plain output is the sum of the x_s
    for a in (p, full, full_st, alone):
        a.setflags(write=False)
    return p, full, full_st, alone


def _states_equal(st, ref_st):
    act = ref_st["prn"] > 0
    assert np.array_equal(st["prn"], ref_st["prn"])
    assert np.array_equal(st["carr_phase"][act].view(np.uint64), ref_st["carr_phase"][act].view(np.uint64))
    assert np.array_equal(st["page"][act], ref_st["page"][act])


def _run_gains(eng, p, gains, state_in=None):
    out = _empty(p.shape[0] * N * 2)
    before = eng.iq_saturated()
    st = eng.run_gains(p, gains, out.data_ptr(), state_in)
    sat = eng.iq_saturated() - before
    return out.cpu().numpy(), st, sat


def test_unity_gains_are_the_plain_bytes(pkg, batch):
    p, full, full_st, _ = batch
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        plain, _, _ = eng.run_host(p)
        assert eng.gain_runs() == 0
        got, st, sat = _run_gains(eng, p, np.full(p.shape, 128))
        assert eng.gain_runs() == 1  # the unity case costs one run (and no sum)
    assert np.array_equal(plain, full) and np.array_equal(got, full) and sat == 0
    _states_equal(st, full_st)


def _random_gains(p, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(1, 700, size=p.shape)
    g[:, 1] = 0  # slot 1 is switched off throughout: its state still advances
    g[0, 0], g[2, 2] = 129, 32767
    return g


def test_random_gains_against_the_model_over_the_oracle(pkg, batch):
    p, full, full_st, alone = batch
    g = _random_gains(p, 5)
    want, want_sat = gain_model.wsum(alone, g[:, :4], N)
    assert np.count_nonzero(want != full) > 0.9 * full.size
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        got, st, sat = _run_gains(eng, p, g)
        assert eng.gain_runs() == 4  # four active slots, four gain columns
    assert np.array_equal(got, want), "%d values differ" % np.count_nonzero(got != want)
    assert sat == want_sat
    _states_equal(st, full_st)


def test_slots_with_equal_gains_share_a_run(pkg, batch):
    """Slots 0 and 2 at one gain column, slot 3 at the same gains where it is active: the same bits as the definition asks for."""
    p, _, full_st, alone = batch
    g = _random_gains(p, 6)
    g[:, 2] = g[:, 0]
    g[1:, 3] = g[1:, 0]
    g[0, 3] = 0
    want, want_sat = gain_model.wsum(alone, g[:, :4], N)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        got, st, sat = _run_gains(eng, p, g)
        assert eng.gain_runs() == 2  # slots 0, 2 and 3 in one run, slot 1 (gain 0) in another
    assert np.array_equal(got, want) and sat == want_sat
    _states_equal(st, full_st)


def test_two_chained_calls_are_the_single_call(pkg, batch):
    p, _, full_st, alone = batch
    g = _random_gains(p, 7)
    want, _ = gain_model.wsum(alone, g[:, :4], N)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        a, st_a, _ = _run_gains(eng, p[:2], g[:2])
        b, st_b, _ = _run_gains(eng, p[2:], g[2:], st_a)
    assert np.array_equal(np.concatenate([a, b]), want)
    _states_equal(st_b, full_st)


def test_twice_the_gain_doubles_the_correlator_sums(pkg):
    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=1, n_slots=16, samples_per_epoch=N, seed=78)
    ref, _ = oracle_run(p, N, FS)
    q = pkg.corr_from_epoch(p[0, 0], FS, 0, max_periods=2, n_delay=3, delay0=-1)
    sums = []
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        for gain in (128, 256):
            out = _empty(2 * N * 2)
            before = eng.iq_saturated()
            eng.run_gains(p, np.full(p.shape, gain), out.data_ptr())
            assert eng.iq_saturated() == before
            if gain == 128:
                assert np.array_equal(out.cpu().numpy(), ref)
            sums.append(eng.correlate(out.data_ptr(), "ishort", N, q))
        # the handle goes back and forth between the plain path and the gains
        plain, _, _ = eng.run_host(p)
        again, _, sat = _run_gains(eng, p, np.full(p.shape, 128))
    assert np.abs(sums[0]).max() > 100000 and np.array_equal(sums[1], 2 * sums[0])
    assert np.array_equal(plain, ref) and np.array_equal(again, ref) and sat == 0


def test_bad_arguments_and_call_order(pkg, batch):
    p, _, _, _ = batch
    g = np.full(p.shape, 128)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        out, a, b = _empty(3 * N * 2 + 8), _empty(3 * N * 2), _empty(3 * N * 2)

        def code(fn, *args):
            with pytest.raises(pkg.GalSynthError) as e:
                fn(*args)
            return e.value.code

        big = g.copy()
        big[1, 2] = 32768
        assert code(eng.run_gains, p, big, out.data_ptr()) == GAL_E_INVAL
        assert code(eng.run_gains, p, g, out.data_ptr() + 2) == GAL_E_INVAL
        assert code(eng.run_gains, p, g, 0) == GAL_E_INVAL
        with pytest.raises(ValueError):
            eng.run_gains(p, g[:2], out.data_ptr())
        lib, h = eng._lib, eng._h
        assert lib.gal_synth_run_gains(h, p.ctypes.data, 0, None, np.zeros(16, np.uint16).ctypes.data, out.data_ptr(), None) == GAL_E_INVAL
        assert lib.gal_synth_run_gains(h, None, 3, None, np.zeros(48, np.uint16).ctypes.data, out.data_ptr(), None) == GAL_E_INVAL
        assert lib.gal_synth_run_gains(h, p.ctypes.data, 3, None, None, out.data_ptr(), None) == GAL_E_INVAL
        g2 = np.full((3, 2), 128)
        g_bad = g2.copy()
        g_bad[1, 1] = 32768
        assert code(eng.iq_wsum, [a.data_ptr(), b.data_ptr()], g_bad, out.data_ptr()) == GAL_E_INVAL
        assert code(eng.iq_wsum, [a.data_ptr(), b.data_ptr() + 4], g2, out.data_ptr()) == GAL_E_INVAL  # misaligned part
        assert code(eng.iq_wsum, [a.data_ptr(), b.data_ptr()], g2, out.data_ptr() + 8) == GAL_E_INVAL  # misaligned output
        assert code(eng.iq_wsum, [a.data_ptr(), out.data_ptr() + 16], g2, out.data_ptr()) == GAL_E_INVAL  # output overlaps a part
        assert code(eng.iq_wsum, [a.data_ptr(), 0], g2, out.data_ptr()) == GAL_E_INVAL
        assert code(eng.iq_wsum, [], np.zeros((3, 0)), out.data_ptr()) == GAL_E_INVAL
        assert code(eng.iq_wsum, [a.data_ptr()] * 65, np.full((3, 65), 1), out.data_ptr()) == GAL_E_INVAL
        eng.iq_wsum([a.data_ptr(), a.data_ptr()], g2, out.data_ptr())  # parts may be one buffer
        eng.iq_saturated()
        # a batch in flight
        eng.plan(p)
        eng.execute(a.data_ptr())
        assert code(eng.run_gains, p, g, out.data_ptr()) == GAL_E_STATE
        assert code(eng.iq_wsum, [a.data_ptr(), b.data_ptr()], g2, out.data_ptr()) == GAL_E_STATE
        eng.plan(p, wait=False)  # staged under the batch in flight: it waits for its execute
        eng.finish()
        assert code(eng.run_gains, p, g, out.data_ptr()) == GAL_E_STATE
        eng.execute(a.data_ptr())
        eng.finish()
        eng.run_gains(p, g, out.data_ptr())
        eng.iq_wsum([a.data_ptr(), b.data_ptr()], g2, out.data_ptr())
        eng.iq_saturated()


# ---- k_iq_wsum's launch geometry, part counts and int32 edge ----------------------------------------------------------------------
# galk_launch_iq_wsum (csrc/iq_gain.hip), restated: a grid of (bx, by) blocks of 256 lanes, at most 2048 blocks in all.
#   by   = min(n_epochs, 2048)                block y takes the epochs y, y + by, y + 2 by, ...
#   need = ceil((spe / 4) / 256)              blocks that give every 16-byte vector (4 complex samples) of an epoch a lane of its own
#   cap  = 2048 / by
#   bx   = min(need, cap), at least 1         lane t of block x takes the epoch's whole vectors x 256 + t, + bx 256, + 2 bx 256, ...
# The up to three samples in front of an epoch's first whole vector and behind its last are taken by block x = 0, one per lane.
from launch_model import launch as _launch  # noqa: E402  (the restatement above, shared with the echo, reflector and array tests)


def _edge_parts(rng, n_parts, n_epochs, spe):
    """Random full-range int16; the first 8 values of every epoch +32767 on all parts at once, the next 8 -32768."""
    x = rng.integers(-32768, 32768, size=(n_parts, n_epochs, 2 * spe), dtype=np.int16)
    x[:, :, :8] = 32767
    x[:, :, 8:16] = -32768
    return x.reshape(n_parts, -1)


def _edge_gains(rng, n_epochs, n_parts, wide):
    """Per row one of EDGE_GAINS in a random column, a small one of them in another, random fill small enough that the row sums to at
    most 65535 (the int32 instance).  wide: every third row all 32767 -- a sum above 65535, the int64 instance for the call."""
    lim = (65535 - 32767 - 129) // max(1, n_parts - 2)
    g = rng.integers(0, lim + 1, size=(n_epochs, n_parts))
    rows = np.arange(n_epochs)
    col = rng.integers(0, n_parts, size=n_epochs)
    g[rows, (col + 1) % n_parts] = rng.choice(EDGE_GAINS[:4], size=n_epochs)
    edge = rng.choice(EDGE_GAINS, size=n_epochs)
    edge[:len(EDGE_GAINS)] = EDGE_GAINS[:n_epochs]  # every one of them at least once where there are five epochs
    g[rows, col] = edge
    assert g.sum(axis=1).max() <= 65535
    if wide:
        g[1::3] = 32767
        assert g.sum(axis=1).max() > 65535
    return g


GUARD = 16  # int16 values behind the output that the kernel must leave alone


def _wsum_guarded(eng, spe, parts, gains, epochs_per_model_call=None):
    """One gal_synth_iq_wsum call against gain_model.wsum (in pieces of whole epochs where asked: the sum is separable per epoch), bytes
    and saturation count; the output buffer is GUARD values longer than the call and must come back untouched there."""
    import torch

    devs = [_dev(p) for p in parts]
    out = torch.full((parts.shape[1] + GUARD,), 0x5a5a, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    before = eng.iq_saturated()
    eng.iq_wsum([d.data_ptr() for d in devs], gains, out.data_ptr())
    sat = eng.iq_saturated() - before
    got = out.cpu().numpy()
    assert (got[parts.shape[1]:] == 0x5a5a).all(), "the kernel wrote behind the last epoch"
    got = got[:parts.shape[1]]
    n_epochs = gains.shape[0]
    step = epochs_per_model_call or n_epochs
    want_sat = 0
    for e0 in range(0, n_epochs, step):
        lo, hi = e0 * spe * 2, min(n_epochs, e0 + step) * spe * 2
        want, s = gain_model.wsum(parts[:, lo:hi], gains[e0:e0 + step], spe)
        want_sat += s
        bad = np.flatnonzero(got[lo:hi] != want)
        assert bad.size == 0, "%d values differ, the first at value %d = epoch %d, value %d of it" % (
            bad.size, lo + bad[0], (lo + bad[0]) // (2 * spe), (lo + bad[0]) % (2 * spe))
    assert sat == want_sat
    return want_sat


# (spe, n_epochs, n_parts) and what _launch must say about it
GEOMETRIES = {
    "epochs_beyond_the_grid": (1030, 2051, 3),
    "uneven_x_stride": (4101, 600, 5),
    "seven_sample_epochs": (7, 4100, 2),
    "cli_batch": (260000, 128, 2),
}


def _geometry_holds(name, spe, n_epochs, n_parts):
    L = _launch(spe, n_epochs)
    if spe == 1030:
        # by = 2048 < 2051: blocks y = 0, 1, 2 take a second epoch; cap = 1 < need = 2: the one x block walks 257 vectors in two trips,
        # the second with one lane; the epochs begin at value offsets 0 and 2 of a vector in turn
        assert (L["by"], L["y_trips"], n_epochs - L["by"]) == (2048, 2, 3)
        assert (L["cap"], L["need"], L["bx"]) == (1, 2, 1) and (L["vec"] == 257).all() and (L["x_trips"] == 2).all()
        assert spe % 4 == 2 and set((np.arange(n_epochs) * spe) % 4) == {0, 2}
    elif spe == 4101:
        # cap = 3 < need = 5: three x blocks, stride 768, over 1024 or 1025 vectors: a second trip that 256 or 257 of 768 lanes take
        assert (L["by"], L["y_trips"]) == (600, 1) and (L["cap"], L["need"], L["bx"], L["x_stride"]) == (3, 5, 3, 768)
        assert set(L["vec"]) == {1024, 1025} and (L["x_trips"] == 2).all() and set(L["vec"] - 768) == {256, 257}
        assert spe % 2 == 1 and set((np.arange(n_epochs) * spe) % 4) == {0, 1, 2, 3} and (n_parts // 4, n_parts % 4) == (1, 1)
    elif spe == 7:
        # 4100 = 2 x 2048 + 4: two whole rounds of the y grid, four blocks go a third time; one whole vector per epoch, three samples
        # for the head / tail lanes, at every alignment
        assert (L["by"], L["y_trips"], n_epochs - 2 * L["by"]) == (2048, 3, 4) and L["bx"] == 1
        assert (L["vec"] == 1).all() and set((np.arange(n_epochs) * spe) % 4) == {0, 1, 2, 3}
    else:
        # 128-epoch batches of 260 000 samples: cap = 16 < need = 254, every lane makes 15 or 16 trips over 65 000 vectors
        assert (spe, n_epochs) == (260000, 128)
        assert (L["by"], L["cap"], L["need"], L["bx"], L["x_stride"]) == (128, 16, 254, 16, 4096)
        assert (L["vec"] == 65000).all() and (L["x_trips"] == 16).all() and 65000 % 4096 != 0


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_wsum_stride_loops(pkg, name):
    """Shapes at which blocks take a second epoch (e += gridDim.y) and lanes a second vector (i += stride), with epochs that begin and
    end inside a 16-byte vector; both instances where three or more parts can sum beyond 65535."""
    spe, n_epochs, n_parts = GEOMETRIES[name]
    _geometry_holds(name, spe, n_epochs, n_parts)
    rng = np.random.default_rng(spe + n_epochs)
    parts = _edge_parts(rng, n_parts, n_epochs, spe)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        for wide in (False, True)[: 2 if n_parts >= 3 else 1]:
            sat = _wsum_guarded(eng, spe, parts, _edge_gains(rng, n_epochs, n_parts, wide), epochs_per_model_call=max(1, 2 ** 21 // spe))
            assert sat > 0


@pytest.mark.parametrize("n_parts,wide", [(k, False) for k in (2, 4, 5, 7, 8, 9, 63, 64)] + [(k, True) for k in (4, 5, 7, 8, 9, 63, 64)])
def test_wsum_part_counts(pkg, n_parts, wide):
    """The part loop takes four parts per trip and the rest one by one: 0, 1, 2 and 15, 16 whole trips with every remainder, up to
    GAL_ENGINE_MAX_CHAN = 64 parts; in int32 (rows that sum to at most 65535) and in int64 (rows of 32767s)."""
    spe, n_epochs = 1030, 3
    assert {k // 4 for k in (2, 4, 5, 7, 8, 9, 63, 64)} == {0, 1, 2, 15, 16} and {k % 4 for k in (2, 4, 5, 7, 8, 9, 63, 64)} == {0, 1, 2, 3}
    rng = np.random.default_rng(7000 + n_parts)
    parts = _edge_parts(rng, n_parts, n_epochs, spe)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        sat = _wsum_guarded(eng, spe, parts, _edge_gains(rng, n_epochs, n_parts, wide))
        assert sat > 0 or not wide


INT32_EDGE_ROWS = ([32767, 32767, 1], [32767, 32767, 2], [32767, 32767, 3])  # sums 65535 (the last the int32 instance takes), 65536, 65537


def test_wsum_at_the_int32_bound(pkg):
    """Full scale on every part against rows that sum to 65535, 65536 and 65537: w = -65535 x 32768 = -2 147 450 880 still fits the
    int32 instance, the other two rows must go to the int64 one (65537 x -32768 < -2^31; tests/test_iq_gain_cpu.py has the
    arithmetic).  Every value clamps; the count must be the model's."""
    spe, n_epochs = 1030, 3
    assert [sum(r) for r in INT32_EDGE_ROWS] == [65535, 65536, 65537]
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        for level in (-32768, 32767):
            parts = np.full((3, n_epochs * spe * 2), level, dtype=np.int16)
            for row in INT32_EDGE_ROWS:
                assert _wsum_guarded(eng, spe, parts, np.tile(row, (n_epochs, 1))) == parts.shape[1]
            # the three rows in one call (the int64 instance), and the 65535 row between two small ones (the int32 instance)
            assert _wsum_guarded(eng, spe, parts, np.array(INT32_EDGE_ROWS)) == parts.shape[1]
            _wsum_guarded(eng, spe, parts, np.array([[1, 0, 128], INT32_EDGE_ROWS[0], [0, 129, 1]]))


def test_wsum_gain_table_regrows_between_calls(pkg):
    """One handle, 3 epochs, then 4100 (the device table of the first call is too small: freed and made anew behind the first call's
    kernel), then 3 again (the larger table is kept)."""
    spe, n_parts = 7, 3
    rng = np.random.default_rng(4100)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        for n_epochs in (3, 4100, 3):
            parts = _edge_parts(rng, n_parts, n_epochs, spe)
            _wsum_guarded(eng, spe, parts, _edge_gains(rng, n_epochs, n_parts, n_epochs == 4100))
