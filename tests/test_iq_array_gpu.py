"""The antenna array on the MI355X: k_iq_array bit for bit against the numpy model (tests/array_model.py), outputs and saturation count
-- part and element counts with both accumulator widths, epochs that begin at every offset inside a 16-byte vector, the launch
geometry, the identity with gal_synth_iq_wsum, the table's regrowth, calls back to back, the refusals -- and gal_synth_run_array against
the model over the engine's own single-slot runs."""
import ctypes

import numpy as np
import pytest

import array_model
import gain_model
import launch_model

pytestmark = pytest.mark.gpu

FS = 2.6e6
GAL_E_INVAL, GAL_E_STATE = -1, -4
GUARD = 16  # int16 values behind every output that the kernel must leave alone


def _dev(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _outs(n_elem, n_val):
    import torch

    outs = [torch.full((n_val + GUARD,), 0x5a5a, dtype=torch.int16, device="cuda") for _ in range(n_elem)]
    torch.cuda.synchronize()
    return outs


def _fetch(outs, n_val):
    got = np.stack([o.cpu().numpy() for o in outs])
    assert (got[:, n_val:] == 0x5a5a).all(), "the kernel wrote behind the last epoch"
    return got[:, :n_val]


def _call(eng, parts, weights):
    """One gal_synth_iq_array call: ([n_elem, n_val] int16, saturation count)."""
    devs = [_dev(p) for p in parts]
    outs = _outs(weights.shape[1], parts.shape[1])
    before = eng.iq_saturated()
    eng.iq_array([d.data_ptr() for d in devs], weights, [o.data_ptr() for o in outs])
    sat = eng.iq_saturated() - before
    return _fetch(outs, parts.shape[1]), sat


def _same(got, want, spe):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d of %d values differ, the first in element %d at value %d = epoch %d, value %d of it (got %d, want %d)" % (
        len(bad), got.size, bad[0][0], bad[0][1], bad[0][1] // (2 * spe), bad[0][1] % (2 * spe), got[tuple(bad[0])], want[tuple(bad[0])])


def _check(eng, parts, weights, spe):
    got, sat = _call(eng, parts, weights)
    want, want_sat = array_model.array(parts, weights, spe)
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


def _weights(rng, n_epochs, n_elem, n_parts, row_sum):
    """Random weights of either sign whose |w_re| + |w_im| sum to at most row_sum over the parts of every (epoch, element)."""
    hi = min(32767, row_sum // (2 * n_parts))
    return rng.integers(-hi, hi + 1, size=(n_epochs, n_elem, n_parts, 2))


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n_elem", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("n_parts", [1, 2, 3, 4, 5, 63, 64])
def test_part_and_element_counts(pkg, n_parts, n_elem, wide):
    """The part loop takes two parts per trip and the last one alone; every element count is an instance of its own.  Inside the int32
    bound: rows that sum to exactly 65535 in one (epoch, element), on parts of +-3000.  wide: rows beyond 65535 -- the int64 instance
    -- on full-range parts with the rails pinned at the start of every epoch: values clamp, and the count must be the model's."""
    spe, n_epochs = 1030, 3
    rng = np.random.default_rng(1000 * n_elem + n_parts)
    if wide:
        parts = _edge_parts(rng, n_parts, n_epochs, spe)
        w = rng.integers(-32767, 32768, size=(n_epochs, n_elem, n_parts, 2))
        w[0, 0, :, :] = 32767  # all parts in phase on the pinned values: the largest sum there is
        w[1, n_elem - 1, :, :] = -32767
    else:
        parts = _parts(rng, n_parts, n_epochs, spe)
        w = _weights(rng, n_epochs, n_elem, n_parts, 65535)
        w[1, n_elem - 1] = 0
        w[1, n_elem - 1, 0] = (32767, -32767)  # |w_re| + |w_im| = 65534 ...
        if n_parts > 1:
            w[1, n_elem - 1, n_parts - 1] = (0, 1)  # ... and 65535: the bound itself
    # (a single part cannot pass the bound: 2 x 32767 = 65534.  Its "wide" case is the int32 instance at the largest weights)
    assert array_model.needs_int64(w) == (wide and n_parts > 1)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        sat = _check(eng, parts, w, spe)
        assert sat > 0 or not wide


@pytest.mark.parametrize("spe,n_epochs", [(26000, 3), (26001, 3), (26002, 3), (26003, 3), (7, 300), (4, 1000), (5, 1000), (6, 1000)])
def test_epoch_alignments(pkg, spe, n_epochs):
    """Epochs that begin at every offset inside a 16-byte vector (the head and tail lanes); with 7 samples an epoch has at most one
    whole vector, with 5 or 6 most have none at all (head and tail lanes only), with 4 every epoch is one vector.  Every epoch has
    weights of its own.  (One sample per epoch cannot be had: gal_synth_create admits no handle below four samples per epoch; DESIGN.md
    section 22.)"""
    rng = np.random.default_rng(spe)
    parts = _parts(rng, 3, n_epochs, spe)
    w = _weights(rng, n_epochs, 3, 3, 65535)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        _check(eng, parts, w, spe)
        # the int64 instance over the same heads and tails: full-range parts, weights of the whole range
        full = rng.integers(-32768, 32768, size=parts.shape, dtype=np.int16)
        ww = rng.integers(-32767, 32768, size=w.shape)
        assert array_model.needs_int64(ww)
        assert _check(eng, full, ww, spe) > 0


@pytest.mark.parametrize("spe,n_epochs", [(4 * 256 * 3 + 4 * 100 + 2, 2), (5, 2100)])
def test_launch_geometry(pkg, spe, n_epochs):
    """A total that is no multiple of the block's tile of 256 vectors (three full tiles, 100 vectors and two samples per epoch), and more
    epochs than the grid has rows (2048): the rows stride."""
    rng = np.random.default_rng(n_epochs)
    parts = _parts(rng, 2, n_epochs, spe)
    w = _weights(rng, n_epochs, 2, 2, 65535)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        _check(eng, parts, w, spe)


# (geometry of tests/launch_model.py, parts, elements, the int64 instance): 5 parts are two whole two-part trips and the single one
STRIDE_CASES = (("rows_and_lanes_stride", 3, 3, False), ("rows_and_lanes_stride", 3, 3, True), ("uneven_x_stride", 5, 8, False),
                ("uneven_x_stride", 5, 4, True))


def stride_case(name, n_parts, n_elem, wide):
    """The inputs of test_stride_loops (tests/test_iq_launch_geometry_cpu.py asserts what they must be): every (epoch, element) has
    weights of its own.  Inside the int32 bound one (epoch, element) sums to 65535 itself, on parts of +-3000.  wide: full-range parts
    with the rails pinned at the start of every epoch under weights of a few hundred, so that most values stay inside the clamp, and
    whole-range weights in one element of every 97th epoch, all parts in phase in two of them: those clamp."""
    spe, n_epochs = launch_model.GEOMETRIES[name]
    rng = np.random.default_rng(spe + n_elem + wide)
    if wide:
        parts = _edge_parts(rng, n_parts, n_epochs, spe)
        w = rng.integers(-400, 401, size=(n_epochs, n_elem, n_parts, 2))
        for e in range(0, n_epochs, 97):
            w[e, e % n_elem] = rng.integers(-32767, 32768, size=(n_parts, 2))
        w[0, 0, :, :] = 32767
        w[97, 97 % n_elem, :, :] = -32767
    else:
        parts = _parts(rng, n_parts, n_epochs, spe)
        w = _weights(rng, n_epochs, n_elem, n_parts, 65535)
        e = n_epochs - 2  # (in rows_and_lanes_stride an epoch of the blocks' second y trip)
        w[e, n_elem - 1] = 0
        w[e, n_elem - 1, 0] = (32767, -32767)
        w[e, n_elem - 1, n_parts - 1] = (0, 1)
    return spe, parts, w


@pytest.mark.parametrize("name,n_parts,n_elem,wide", STRIDE_CASES)
def test_stride_loops(pkg, name, n_parts, n_elem, wide):
    """Lanes that take a second vector (i += stride, where cap < need) and blocks that take a second epoch (e += gridDim.y), with K
    output streams behind one index, in both widths."""
    spe, parts, w = stride_case(name, n_parts, n_elem, wide)
    assert array_model.needs_int64(w) == wide
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        sat = _check(eng, parts, w, spe)
        assert not wide or 0 < sat < n_elem * parts.shape[1]


@pytest.mark.parametrize("n_parts", [1, 3, 12])
def test_unrotated_weights_are_the_weighted_sum(pkg, n_parts):
    """K = 1, w = (32 g, 0), g <= 1023: gal_synth_iq_wsum on the same handle, byte for byte, saturation count included."""
    import torch

    spe, n_epochs = 2601, 3
    rng = np.random.default_rng(n_parts)
    parts = _edge_parts(rng, n_parts, n_epochs, spe)
    g = rng.integers(0, 1024, size=(n_epochs, n_parts))
    g[0, 0] = 1023
    w = np.zeros((n_epochs, 1, n_parts, 2), dtype=np.int64)
    w[:, 0, :, 0] = 32 * g
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        devs = [_dev(p) for p in parts]
        ref = torch.zeros(parts.shape[1], dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        before = eng.iq_saturated()
        eng.iq_wsum([d.data_ptr() for d in devs], g, ref.data_ptr())
        ref_sat = eng.iq_saturated() - before
        got, sat = _call(eng, parts, w)
        assert got[0].tobytes() == ref.cpu().numpy().tobytes() and sat == ref_sat
        assert sat > 0 or n_parts == 1


def test_the_table_grows_and_calls_follow_each_other_without_a_fence(pkg):
    """A small call, then one whose table is 400 times as large (the handle frees and allocates); then two calls back to back on
    different outputs with no fence between them: the second waits for the first one's kernel before it rewrites the one table."""
    spe = 64
    rng = np.random.default_rng(3)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        _check(eng, _parts(rng, 1, 1, spe), _weights(rng, 1, 1, 1, 65535), spe)
        _check(eng, _parts(rng, 10, 40, spe), _weights(rng, 40, 8, 10, 65535), spe)
        _check(eng, _parts(rng, 2, 2, spe), _weights(rng, 2, 2, 2, 65535), spe)
        pa, pb = _parts(rng, 10, 40, spe), _parts(rng, 3, 40, spe)
        wa, wb = _weights(rng, 40, 8, 10, 65535), _weights(rng, 40, 2, 3, 200000)
        da, db = [_dev(p) for p in pa], [_dev(p) for p in pb]
        oa, ob = _outs(8, pa.shape[1]), _outs(2, pb.shape[1])
        before = eng.iq_saturated()
        eng.iq_array([d.data_ptr() for d in da], wa, [o.data_ptr() for o in oa])
        eng.iq_array([d.data_ptr() for d in db], wb, [o.data_ptr() for o in ob])
        sat = eng.iq_saturated() - before
        want_a, sat_a = array_model.array(pa, wa, spe)
        want_b, sat_b = array_model.array(pb, wb, spe)
        _same(_fetch(oa, pa.shape[1]), want_a, spe)
        _same(_fetch(ob, pb.shape[1]), want_b, spe)
        assert sat == sat_a + sat_b


def test_refusals_leave_the_handle_working(pkg):
    import torch

    spe, n_epochs = 100, 2
    n = n_epochs * spe  # complex samples = 4 n bytes per stream
    rng = np.random.default_rng(8)
    parts = _parts(rng, 2, n_epochs, spe)
    w = _weights(rng, n_epochs, 2, 2, 65535)
    want, _ = array_model.array(parts, w, spe)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        buf = torch.zeros(8 * n * 2, dtype=torch.int16, device="cuda")  # eight streams' worth, zeros
        buf[:2 * n * 2] = torch.from_numpy(parts.reshape(-1)).cuda()
        torch.cuda.synchronize()
        a = buf.data_ptr()
        pp = [a, a + 4 * n]
        free = [a + 4 * n * k for k in range(2, 8)]

        def works():
            eng.iq_array(pp, w, free[:2])
            eng.iq_saturated()
            got = buf.cpu().numpy()
            _same(np.stack([got[4 * n:6 * n], got[6 * n:8 * n]]), want, spe)
            assert not got[8 * n:].any()  # no refused call wrote into the streams behind

        def refused(code, part_ptrs, rows, out_ptrs):
            with pytest.raises(pkg.GalSynthError) as ei:
                eng.iq_array(part_ptrs, rows, out_ptrs)
            assert ei.value.code == code, str(ei.value)
            works()

        works()
        refused(GAL_E_INVAL, pp, w, [free[2], pp[1]])                        # an output that is a part
        refused(GAL_E_INVAL, pp, w, [free[2], pp[1] + 4 * n - 16])           # ... that meets a part's last vector
        refused(GAL_E_INVAL, pp, w, [free[2], free[2]])                      # two outputs that are one
        refused(GAL_E_INVAL, pp, w, [free[2], free[2] + 16])                 # ... that meet
        refused(GAL_E_INVAL, pp, w, [free[2], free[3] + 4])                  # a misaligned output
        refused(GAL_E_INVAL, [pp[0], pp[1] + 8], w, free[2:4])               # a misaligned part
        refused(GAL_E_INVAL, pp, w, [free[2], 0])                            # a null output
        bad = w.copy()
        bad[1, 1, 0, 1] = -32768
        refused(GAL_E_INVAL, pp, bad, free[2:4])
        lib, h = pkg.load_library(), eng._h
        rows9 = np.zeros((n_epochs, 9, 2), dtype=pkg.STEER_DTYPE)
        ptrs = (ctypes.c_void_p * 2)(*pp)
        outs9 = (ctypes.c_void_p * 9)(*[free[2]] * 9)
        assert lib.gal_synth_iq_array(h, ptrs, 2, rows9.ctypes.data, n_epochs, 9, outs9) == GAL_E_INVAL  # K = 9
        assert lib.gal_synth_iq_array(h, ptrs, 2, rows9.ctypes.data, n_epochs, 0, outs9) == GAL_E_INVAL
        assert lib.gal_synth_iq_array(h, ptrs, 2, None, n_epochs, 2, outs9) == GAL_E_INVAL
        assert lib.gal_synth_iq_array(h, None, 2, rows9.ctypes.data, n_epochs, 2, outs9) == GAL_E_INVAL
        assert lib.gal_synth_iq_array(h, ptrs, 2, rows9.ctypes.data, n_epochs, 2, None) == GAL_E_INVAL
        assert lib.gal_synth_iq_array(h, ptrs, 65, rows9.ctypes.data, n_epochs, 1, outs9) == GAL_E_INVAL
        works()
        # parts may overlap each other
        eng.iq_array([pp[0], pp[0]], w, free[2:4])
        eng.iq_saturated()


def test_buffer_of_the_batch_in_flight_is_refused(pkg):
    import torch

    N = 26000
    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=4, n_slots=16, samples_per_epoch=N, seed=12)
    w = np.zeros((2, 1, 1, 2), dtype=np.int64)
    w[..., 0] = 4096
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as e:
        iq = torch.zeros(2 * N * 2, dtype=torch.int16, device="cuda")
        other = torch.zeros(2 * N * 2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        e.plan(p)
        e.execute(iq.data_ptr())
        for src, dst in ((iq, other), (other, iq)):
            with pytest.raises(pkg.GalSynthError) as ei:
                e.iq_array([src.data_ptr()], w, [dst.data_ptr()])
            assert ei.value.code == GAL_E_STATE
        with pytest.raises(pkg.GalSynthError) as ei:
            e.run_array(p, np.full(p.shape, 128), np.zeros((2, 1, 16)), [other.data_ptr()])
        assert ei.value.code == GAL_E_STATE
        e.finish()
        e.iq_array([iq.data_ptr()], w, [other.data_ptr()])
        e.iq_saturated()
        assert np.array_equal(other.cpu().numpy(), iq.cpu().numpy())  # (4096, 0): the part itself


# ---- gal_synth_run_array ---------------------------------------------------------------------------------------------------------
def test_run_array_over_two_batches_against_the_model(pkg):
    """Two batches of three epochs, four satellites, three elements, the states chained.  The model's parts are the engine's own runs
    of every slot alone (gal_synth_run_host: x_s of the header), its weights steer_make of the random gains and phases.  Four runs per
    batch.  Then one element with all phases 0: gal_synth_run_gains' bytes."""
    import torch

    N, E, K = 26000, 3, 3
    full = pkg.workloads.make_synthetic(n_epochs=2 * E, n_chan=4, n_slots=16, samples_per_epoch=N, seed=33)
    C = pkg.tables()["cos1024"]
    rng = np.random.default_rng(44)
    gains = rng.integers(0, 1024, size=(2 * E, 16))
    gains[1, 2] = 1023
    phase = rng.integers(0, 1 << 32, size=(2 * E, K, 16), dtype=np.uint64)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        outs = _outs(K, E * N * 2)
        one = torch.zeros(E * N * 2, dtype=torch.int16, device="cuda")
        ref = torch.zeros(E * N * 2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        st = st_ref = st_one = None
        alone_st = [None] * 4
        for b in range(2):
            p, g, ph = full[b * E:(b + 1) * E], gains[b * E:(b + 1) * E], phase[b * E:(b + 1) * E]
            alone = []
            for s in range(4):
                iq, alone_st[s], _ = eng.run_host(gain_model.slot_alone(p, s), alone_st[s])
                alone.append(np.ascontiguousarray(iq).view(np.int16).ravel())
            alone = np.stack(alone)
            w = np.zeros((E, K, 4, 2), dtype=np.int64)
            for a in range(K):
                w[:, a, :, 0], w[:, a, :, 1] = array_model.steer_make(g[:, :4], ph[:, a, :4], C)
            want, want_sat = array_model.array(alone, w, N)
            before = eng.iq_saturated()
            st = eng.run_array(p, g, ph, [o.data_ptr() for o in outs], state_in=st)
            sat = eng.iq_saturated() - before
            assert eng.gain_runs() == 4
            _same(_fetch(outs, E * N * 2), want, N)
            assert sat == want_sat
            for s in range(4):  # the end state of a slot is that of its own run
                assert st[s].tobytes() == alone_st[s][s].tobytes()
            # one element, every phase 0: the weighted sum of run_gains, which groups the slots by gain
            st_ref = eng.run_gains(p, g, ref.data_ptr(), state_in=st_ref)
            eng.iq_saturated()
            st_one = eng.run_array(p, g, np.zeros((E, 1, 16)), [one.data_ptr()], state_in=st_one)
            eng.iq_saturated()
            assert eng.gain_runs() == 4
            assert one.cpu().numpy().tobytes() == ref.cpu().numpy().tobytes()
            assert st_one.tobytes() == st_ref.tobytes() == st.tobytes()
        # a gain of 1024; nine elements; outputs that meet; a misaligned output -- and the handle still works
        p, g, ph = full[:E], gains[:E].copy(), phase[:E]
        ptrs = [o.data_ptr() for o in outs]
        g[2, 5] = 1024
        with pytest.raises(pkg.GalSynthError) as ei:
            eng.run_array(p, g, ph, ptrs)
        assert ei.value.code == GAL_E_INVAL and "slot 5" in str(ei.value) and "epoch 2" in str(ei.value)
        g[2, 5] = 0
        for bad in ([ptrs[0], ptrs[1], ptrs[1] + 16], [ptrs[0], ptrs[1], ptrs[2] + 8], [ptrs[0], ptrs[0], ptrs[2]]):
            with pytest.raises(pkg.GalSynthError) as ei:
                eng.run_array(p, g, ph, bad)
            assert ei.value.code == GAL_E_INVAL
        with pytest.raises(pkg.GalSynthError) as ei:
            eng.run_array(p, g, np.zeros((E, 9, 16)), [ptrs[0]] * 9)
        assert ei.value.code == GAL_E_INVAL
        eng.run_array(p, g, ph, ptrs)
        eng.iq_saturated()
        assert eng.gain_runs() == 4
