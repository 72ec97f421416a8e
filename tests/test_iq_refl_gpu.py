"""Geometric reflectors on the MI355X: k_iq_refl bit for bit against the numpy model (tests/refl_model.py) at the smallest shapes that
can go wrong -- epochs of 4, 5, 6 and 260 samples, 1 to 3 parts, every residue of the delay with and without a fraction, the ends of
the range, history across calls and shared with the echo pass, both accumulator widths -- and gal_synth_run_refl against the model
over the oracle's output of every slot on its own."""
import numpy as np
import pytest

import gain_model
import launch_model
import mpath_model
import refl_model
from oracle_binding import oracle_run

pytestmark = pytest.mark.gpu

GAL_E_INVAL = -1
GUARD = 16  # int16 values behind the output that the kernel must leave alone
# (D, F): D = 0 with F > 0 reads sample n - 1 (the history at n = 0); every residue of D mod 4 with F > 0, where the five delayed
# samples take their two aligned vectors differently; F = 0 beside them (the echo kernel's reads); both ends of the range
DELAYS = ((0, 1), (0, 2048), (1, 4095), (2, 1), (3, 2048), (4, 4095), (5, 7), (6, 2047), (7, 2049), (255, 1000), (256, 3000), (1020, 1),
          (1021, 4095), (1022, 2048), (1023, 4095), (1024, 0), (0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (1023, 0))


@pytest.fixture(scope="module")
def cos1024(pkg):
    return pkg.tables()["cos1024"]


def _dev(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _call(eng, parts, gains, pof, rows, hist_id=None, echo=False):
    """One gal_synth_iq_refl (echo: gal_synth_iq_mpath) call: (bytes, saturation count); the GUARD values behind the output must come
    back untouched."""
    import torch

    devs = [_dev(p) for p in parts]
    out = torch.full((parts.shape[1] + GUARD,), 0x5a5a, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    before = eng.iq_saturated()
    (eng.iq_mpath if echo else eng.iq_refl)([d.data_ptr() for d in devs], gains, out.data_ptr(), pof, rows, hist_id)
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
    want, want_sat = lines.call_refl(parts, gains, spe, pof, rows, hist_id)
    _same(got, want, spe)
    assert sat == want_sat
    return want_sat


def _parts(rng, n_parts, n_epochs, spe, lim=3000):
    return rng.integers(-lim, lim, size=(n_parts, n_epochs * spe * 2), dtype=np.int16)


def _random_rows(rng, n_epochs, n_echo, gain_hi=400):
    r = refl_model.rows(n_epochs, n_echo)
    r["gain_q7"] = rng.integers(1, gain_hi, size=r.shape)
    pick = rng.integers(0, len(DELAYS), size=r.shape)
    r["delay"], r["frac_q12"] = np.asarray(DELAYS)[pick, 0], np.asarray(DELAYS)[pick, 1]
    r["ph0"] = rng.integers(0, 1 << 32, size=r.shape, dtype=np.uint64)
    r["dph"] = rng.integers(-(1 << 24), 1 << 24, size=r.shape)
    return r


@pytest.mark.parametrize("spe,n_epochs", [(4, 300), (5, 300), (6, 300), (260, 7)])
@pytest.mark.parametrize("n_parts", [1, 2, 3])
def test_every_delay_at_small_epochs(pkg, cos1024, spe, n_epochs, n_parts):
    """Epochs of one vector and of one vector with a head or a tail (the first block's single lanes take up to all samples), and 260
    samples (65 vectors, more than one wave); 300 epochs of 4 are more than a history line, so the long delays read the call, the
    first of them the line.  One call per (D, F) with one echo, every call handing its history to the next; then all of DELAYS as 22
    echoes at once, twice."""
    rng = np.random.default_rng(1000 * spe + n_parts)
    parts = _parts(rng, n_parts, n_epochs, spe)
    gains = rng.integers(0, 300, size=(n_epochs, n_parts))
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        lines = refl_model.Lines(cos1024)
        for D, F in DELAYS:
            rows = _random_rows(rng, n_epochs, 1)
            rows["delay"], rows["frac_q12"] = D, F
            _check(eng, lines, spe, parts, gains, [int(rng.integers(0, n_parts))], rows)
        rows = _random_rows(rng, n_epochs, len(DELAYS), 60)
        rows["delay"][::2], rows["frac_q12"][::2] = np.asarray(DELAYS)[:, 0], np.asarray(DELAYS)[:, 1]  # odd epochs: a random pick each
        pof = rng.integers(0, n_parts, size=len(DELAYS))
        for _ in range(2):
            _check(eng, lines, spe, parts, gains, pof, rows)


def test_both_instances_at_the_int32_bound_and_the_saturation_count(pkg, cos1024):
    """Rows with sum g + 2 sum A = 65535 (the last the int32 instance takes) and 65536 on parts at -32768 and at +32767 with F > 0: u
    stays at the level, every value clamps, the count is the model's; then full-range random parts, where only some values clamp."""
    spe, n_epochs = 262, 3
    rows = refl_model.rows(n_epochs, 2, [[100, 200]], [[0, 3]], [[5 << 29, 7 << 29], [1 << 29, 3 << 29], [0, 1 << 31]], 0, [[4095, 1]])
    rng = np.random.default_rng(21)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        lines = refl_model.Lines(cos1024)
        for level in (-32768, 32767):
            parts = np.full((2, n_epochs * spe * 2), level, dtype=np.int16)
            for extra in (0, 1):
                gains = np.tile([32767, 32168 + extra], (n_epochs, 1))
                assert refl_model.needs_int64(gains, rows) == bool(extra)
                sat = _check(eng, lines, spe, parts, gains, [0, 1], rows)
                assert sat >= parts.shape[1] - 16  # (all but the few values whose echo reads the zeros in front of the first call)
            for extra in (0, 1):  # the 65535 row between two small ones (the int32 instance), the 65536 row among them (the int64 one)
                _check(eng, lines, spe, parts, np.array([[1, 0], [32767, 32168 + extra], [0, 129]]), [0, 1], rows)
        parts = rng.integers(-32768, 32768, size=(2, n_epochs * spe * 2), dtype=np.int16)
        for wide in (False, True):
            gains = rng.integers(30000 if wide else 0, 32768 if wide else 20000, size=(n_epochs, 2))
            r = _random_rows(rng, n_epochs, 3, 4000)
            r["gain_q7"][:, 0] = 3999
            assert refl_model.needs_int64(gains, r) == wide
            sat = _check(eng, lines, spe, parts, gains, [0, 1, 1], r)
            assert 0 < sat < parts.shape[1]


def test_frac_0_is_iq_mpath_on_the_same_handle_and_the_passes_share_a_line(pkg, cos1024):
    """F = 0 in every row: the bytes of gal_synth_iq_mpath, called on the same handle after a reset.  Then calls of the two passes
    alternate on one stream: each reads the line the other wrote, and the bytes are those of the one call of the model."""
    spe, n_epochs = 261, 8
    rng = np.random.default_rng(22)
    parts = _parts(rng, 3, n_epochs, spe)
    gains = rng.integers(0, 300, size=(n_epochs, 3))
    rows = _random_rows(rng, n_epochs, 4)
    rows["frac_q12"] = 0
    erows = mpath_model.rows(n_epochs, 4, rows["gain_q7"], rows["delay"], rows["ph0"], rows["dph"])
    pof = [0, 2, 2, 1]
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        a, sat_a = _call(eng, parts, gains, pof, rows)
        a2, _ = _call(eng, parts[::-1], gains, pof, rows)  # a second call: long delays read the first one's samples
        eng.mpath_reset()
        b, sat_b = _call(eng, parts, gains, pof, erows, echo=True)
        b2, _ = _call(eng, parts[::-1], gains, pof, erows, echo=True)
        assert np.array_equal(a, b) and sat_a == sat_b and np.array_equal(a2, b2)
        _same(a, mpath_model.mpath(parts, gains, spe, pof, erows, cos1024)[0], spe)
        # mixed calls: echo rows are reflector rows with F = 0, so ONE call of the model states the whole stream
        eng.mpath_reset()
        mixed = _random_rows(rng, n_epochs, 4)
        mixed["delay"][:, 0], mixed["frac_q12"][:, 0] = 1023, 4095
        cuts = ((0, 1, True), (1, 3, False), (3, 4, True), (4, 7, False), (7, 8, True))  # (first epoch, end, by the echo pass)
        for e0, e1, echo in cuts:
            if echo:
                mixed["frac_q12"][e0:e1] = 0
        want, want_sat, _ = refl_model.refl(parts, gains, spe, pof, mixed, cos1024)
        got, sat = [], 0
        for e0, e1, echo in cuts:
            r = mixed[e0:e1]
            if echo:
                r = mpath_model.rows(e1 - e0, 4, r["gain_q7"], r["delay"], r["ph0"], r["dph"])
            y, s = _call(eng, parts[:, 2 * spe * e0:2 * spe * e1], gains[e0:e1], pof, r, echo=echo)
            got.append(y)
            sat += s
        _same(np.concatenate(got), want, spe)
        assert sat == want_sat


def _edge_parts(rng, n_parts, n_epochs, spe):
    """Random full-range int16; the first 8 values of every epoch +32767 on all parts at once, the next 8 -32768."""
    x = rng.integers(-32768, 32768, size=(n_parts, n_epochs, 2 * spe), dtype=np.int16)
    x[:, :, :8] = 32767
    x[:, :, 8:16] = -32768
    return x.reshape(n_parts, -1)


def stride_case(name):
    """The inputs of test_stride_loops (tests/test_iq_launch_geometry_cpu.py asserts what they must be): those of the echo file's
    stride_case with reflector rows -- 8 echoes per epoch drawn from DELAYS, F > 0 and F = 0 side by side -- and both ends of the
    range, D = 1023 with F = 4095 and D = 1024 with F = 0, forced into epoch 10 and into the last epoch (in rows_and_lanes_stride one
    that a block takes on its second y trip, and that begins on a vector: the one lane of its second x trip reads the epoch's first
    samples)."""
    spe, n_epochs = launch_model.GEOMETRIES[name]
    rng = np.random.default_rng(spe + n_epochs + 1)
    parts = _edge_parts(rng, 3, n_epochs, spe)
    gains = rng.integers(0, 121, size=(n_epochs, 3))
    rows = _random_rows(rng, n_epochs, 8, 60)
    rows["dph"] = rng.integers(-(1 << 31), 1 << 31, size=rows.shape)
    for e in (10, n_epochs - 1):
        rows["delay"][e, :2], rows["frac_q12"][e, :2] = (1023, 1024), (4095, 0)
    e_wide = n_epochs // 2
    wide_gains = gains.copy()
    wide_gains[e_wide] = (32767, 32767, 2)
    rows2 = _random_rows(rng, 3, 8, 60)
    rows2["delay"][0], rows2["frac_q12"][0] = (1024, 1023, 1023, 255, 4, 3, 1, 0), (0, 4095, 0, 1000, 2048, 1, 4095, 7)
    second = (_edge_parts(rng, 3, 3, spe), rng.integers(0, 121, size=(3, 3)), rows2)
    return {"spe": spe, "n_epochs": n_epochs, "parts": parts, "gains": gains, "wide_gains": wide_gains, "e_wide": e_wide, "rows": rows,
            "pof": [0, 2, 2, 0, 2, 0, 0, 2], "second": second}


@pytest.mark.parametrize("name", list(launch_model.GEOMETRIES))
def test_stride_loops(pkg, cos1024, name):
    """Lanes that take a second vector (i += stride, where cap < need) and blocks that take a second epoch (e += gridDim.y): the phase
    m0 = 4 i - a and the delayed vectors q, q + 1 of the second trip, against the model, in both instances.  Every long call is
    followed by a short one on the same handle that reads the lines the long call left."""
    case = stride_case(name)
    spe, parts = case["spe"], case["parts"]
    narrow, wide = launch_model.long_call_model(refl_model.refl, case, cos1024)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        for gains, (want, want_sat) in ((case["gains"], narrow), (case["wide_gains"], wide)):
            assert refl_model.needs_int64(gains, case["rows"]) == (gains is case["wide_gains"])
            eng.mpath_reset()
            got, sat = _call(eng, parts, gains, case["pof"], case["rows"])
            _same(got, want, spe)
            assert sat == want_sat and 0 < sat < parts.shape[1]
            lines = refl_model.Lines(cos1024)
            lines.lines[:3] = parts[:, -2 * refl_model.H:]  # what a call of more than 1024 samples leaves
            p2, g2, r2 = case["second"]
            _check(eng, lines, spe, p2, g2, case["pof"], r2)


PART_COUNTS = (4, 5, 6, 7, 8, 63, 64)


def part_counts_case(n_parts, wide):
    """The inputs of test_part_counts: three echoes on the first and on the LAST part (two on one part) at (D, F) = (1, 4095), (1023, 1)
    and (4, 2048), permuted from epoch to epoch; full-range parts under gains small enough that most values stay inside the clamp, so
    that a part taken with its neighbour's gain shows in the bytes.  wide: epoch 1 beyond 65535, the int64 instance for the call."""
    spe, n_epochs = 1030, 3
    rng = np.random.default_rng(2300 + n_parts)
    parts = _edge_parts(rng, n_parts, n_epochs, spe)
    gains = rng.integers(1, max(3, int(200 / n_parts ** 0.5)) + 1, size=(n_epochs, n_parts))
    rows = _random_rows(rng, n_epochs, 3, 60)
    df = ((1, 4095), (1023, 1), (4, 2048))
    for e in range(n_epochs):
        for r in range(3):
            rows["delay"][e, r], rows["frac_q12"][e, r] = df[(r + e) % 3]
    if wide:
        gains[1] = rng.integers(20000, 32768, size=n_parts)
        rows["gain_q7"][1] = 32767
    return spe, parts, gains, [0, n_parts - 1, n_parts - 1], rows


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n_parts", PART_COUNTS)
def test_part_counts(pkg, cos1024, n_parts, wide):
    """The part loop takes four parts per trip and the rest one by one: 1, 2, 15 and 16 whole trips with every remainder.  Some values
    clamp, and the count must be the model's.  A second call on the reversed parts: the delays read the first call's samples."""
    assert {k // 4 for k in PART_COUNTS} == {1, 2, 15, 16} and {k % 4 for k in PART_COUNTS} == {0, 1, 2, 3}
    spe, parts, gains, pof, rows = part_counts_case(n_parts, wide)
    assert refl_model.needs_int64(gains, rows) == wide
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        lines = refl_model.Lines(cos1024)
        sat = _check(eng, lines, spe, parts, gains, pof, rows)
        assert 0 < sat < parts.shape[1]
        _check(eng, lines, spe, parts[::-1], gains, pof, rows)


def echoes32_case(wide):
    """The inputs of test_32_echoes: GAL_ECHO_MAX = 32 echoes on 3 parts, all of DELAYS in every second epoch and a random pick in the
    others, at gains inside the int32 bound (3 x 300 + 2 x 32 x 59 < 65535) or, wide, beyond it."""
    spe, n_epochs = 261, 8
    rng = np.random.default_rng(2400 + wide)
    parts = _parts(rng, 3, n_epochs, spe)
    gains = rng.integers(0, 300, size=(n_epochs, 3))
    if wide:
        parts //= 10  # (most values stay inside the clamp under the larger gains too)
    rows = _random_rows(rng, n_epochs, 32, 2100 if wide else 60)
    d = np.asarray(DELAYS + DELAYS[:10])
    rows["delay"][::2], rows["frac_q12"][::2] = d[:, 0], d[:, 1]
    pof = rng.integers(0, 3, size=32)
    pof[-1] = 2
    return spe, parts, gains, pof, rows


def test_32_echoes(pkg, cos1024):
    """The largest echo count there is, twice on one handle (the second call reads the first one's lines), then again with gains that
    need the int64 instance."""
    with pkg.SynthEngine(samples_per_epoch=261, n_slots=16, device=0) as eng:
        lines = refl_model.Lines(cos1024)
        for wide in (False, True):
            spe, parts, gains, pof, rows = echoes32_case(wide)
            assert rows.shape[1] == refl_model.GAL_ECHO_MAX and refl_model.needs_int64(gains, rows) == wide
            assert {(int(D), int(F)) for D, F in zip(rows["delay"].ravel(), rows["frac_q12"].ravel())} == set(DELAYS)
            for _ in range(2):
                _check(eng, lines, spe, parts, gains, pof, rows)


PHASE_STEPS = (-(1 << 31), -(1 << 31) + 1, -1, 1, (1 << 31) - 1)  # and a random one


def test_phase_steps(pkg, cos1024):
    """Steps next to +-2^31 and +-1 with 26001-sample epochs: m dph wraps thousands of times inside an epoch, and the kernel's
    m0 * dph (uint32) must be the model's product mod 2^32.  F > 0 on four of the six echoes."""
    spe, n_epochs = 26001, 3
    rng = np.random.default_rng(25)
    parts = _parts(rng, 2, n_epochs, spe)
    gains = rng.integers(0, 300, size=(n_epochs, 2))
    rows = _random_rows(rng, n_epochs, 6)
    steps = np.asarray(PHASE_STEPS + (int(rng.integers(-(1 << 31), 1 << 31)),))
    for e in range(n_epochs):
        rows["dph"][e] = np.roll(steps, e)
    rows["frac_q12"][:, :4] = rng.integers(1, 4096, size=(n_epochs, 4))
    rows["delay"][:, :4] = np.minimum(rows["delay"][:, :4], 1023)
    rows["frac_q12"][:, 4:] = 0
    assert (spe - 1) * ((1 << 31) - 1) >> 32 > 10000
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        _check(eng, refl_model.Lines(cos1024), spe, parts, gains, [0, 1, 1, 0, 1, 0], rows)


def test_hist_id_names_the_line(pkg, cos1024):
    """Lines are named per call: permuted between calls, left out (-1) and taken up again, the last line (63).  Reflector rows with
    F > 0; in the middle one call of gal_synth_iq_mpath, whose part 0 reads line 63, which the reflector pass wrote as its part 2."""
    spe, n_epochs = 333, 2
    rng = np.random.default_rng(26)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        lines = refl_model.Lines(cos1024)
        for ids, pof, echo in (([5, 9, -1], [0, 1, 1], False), ([9, 5, 63], [0, 1, 2], False), ([63, -1, 9], [0, 2, 0], True),
                               ([-1, 63, 5], [2, 1, 1], False), (None, [0, 1, 2], False), ([2, 1, 0], [0, 1, 2], False)):
            rows = _random_rows(rng, n_epochs, 3)
            rows["delay"] = rng.choice((1023, 1022, 700, 4), size=rows.shape)
            rows["frac_q12"] = 0 if echo else rng.integers(1, 4096, size=rows.shape)
            parts, gains = _parts(rng, 3, n_epochs, spe), rng.integers(0, 300, size=(n_epochs, 3))
            if not echo:
                _check(eng, lines, spe, parts, gains, pof, rows, ids)
                continue
            erows = mpath_model.rows(n_epochs, 3, rows["gain_q7"], rows["delay"] + 1, rows["ph0"], rows["dph"])  # 1024 among them
            got, sat = _call(eng, parts, gains, pof, erows, ids, echo=True)
            want, want_sat = lines.call(parts, gains, spe, pof, erows, ids)
            _same(got, want, spe)
            assert sat == want_sat


CUTS = (1, 5, 2, 8, 3, 9, 1, 21)  # epochs per call, of 100 samples: 5000 samples in all


def test_any_cut_of_5000_samples_into_calls_is_the_single_call(pkg, cos1024):
    """Calls shorter than a history line roll it: D = 1023 with F > 0 reads 1024 samples back, over three calls at the start."""
    spe, n_epochs = 100, sum(CUTS)
    assert spe * n_epochs == 5000
    rng = np.random.default_rng(23)
    parts = _parts(rng, 2, n_epochs, spe)
    gains = rng.integers(0, 300, size=(n_epochs, 2))
    rows = _random_rows(rng, n_epochs, 4)
    rows["delay"][:, :2], rows["frac_q12"][:, 0], rows["frac_q12"][:, 1] = 1023, 4095, 1
    pof = [0, 1, 1, 0]
    want, want_sat, _ = refl_model.refl(parts, gains, spe, pof, rows, cos1024)
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        got, sat, e0 = [], 0, 0
        for ne in CUTS:
            y, s = _call(eng, parts[:, 2 * spe * e0:2 * spe * (e0 + ne)], gains[e0:e0 + ne], pof, rows[e0:e0 + ne])
            got.append(y)
            sat += s
            e0 += ne
        _same(np.concatenate(got), want, spe)
        assert sat == want_sat
        eng.mpath_reset()
        y, s = _call(eng, parts, gains, pof, rows)  # and the whole stream in one call
        _same(y, want, spe)
        assert s == want_sat


def test_refusals(pkg):
    import torch

    spe = 260
    with pkg.SynthEngine(samples_per_epoch=spe, n_slots=16, device=0) as eng:
        out, a, b = (torch.zeros(3 * spe * 2 + 8, dtype=torch.int16, device="cuda") for _ in range(3))
        torch.cuda.synchronize()

        def refused(fn, *args):
            with pytest.raises(pkg.GalSynthError) as e:
                fn(*args)
            assert e.value.code == GAL_E_INVAL
            return str(e.value)

        g2 = np.full((3, 2), 128)
        rows = refl_model.rows(3, 1, 64, 4, 0, 0, 100)
        ptrs = [a.data_ptr(), b.data_ptr()]
        assert "no history line" in refused(eng.iq_refl, ptrs, g2, out.data_ptr(), [1], rows, [0, -1])
        assert "gal_synth_iq_refl" in refused(eng.iq_refl, ptrs, g2, out.data_ptr(), [1], rows, [7, 7])
        for fields, text in (({"delay": 1024, "frac_q12": 1}, "delay 1024 + 1/4096"), ({"frac_q12": 4096}, "frac_q12 4096"), ({"reserved": 1}, "reserved = 1")):
            bad = rows.copy()
            for k, v in fields.items():
                bad[k][2, 0] = v
            assert text in refused(eng.iq_refl, ptrs, g2, out.data_ptr(), [1], bad)
        assert refused(eng.iq_refl, ptrs, g2, out.data_ptr() + 8, [1], rows)
        eng.iq_refl(ptrs, g2, out.data_ptr(), [1], rows)
        eng.iq_saturated()


# ---- gal_synth_run_refl ------------------------------------------------------------------------------------------------------------
N = 2600
FS = 2.6e6


@pytest.fixture(scope="module")
def batch(pkg):
    """3 epochs of 2600 samples, 3 satellites.  Shared, left unchanged: the records, the oracle's output and end state of the full
    run, and the oracle's output of every slot alone."""
    p = pkg.workloads.make_synthetic(n_epochs=3, n_chan=3, n_slots=16, samples_per_epoch=N, seed=81)
    full, full_st = oracle_run(p, N, FS)
    alone = np.stack([oracle_run(gain_model.slot_alone(p, s), N, FS)[0] for s in range(3)])
    for a in (p, full, full_st, alone):
        a.setflags(write=False)
    return p, full, full_st, alone


def _run(eng, p, gains, sof, rows, state_in=None):
    import torch

    out = torch.zeros(p.shape[0] * N * 2, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    before = eng.iq_saturated()
    st = eng.run_refl(p, gains, out.data_ptr(), sof, rows, state_in)
    sat = eng.iq_saturated() - before
    return out.cpu().numpy(), st, sat


def test_run_refl_over_two_batches(pkg, cos1024, batch):
    """A ground bounce and a wall echo on slot 0 and a ground bounce on slot 2, rows from gal_synth_refl_geom / _row; slot 1 has none.
    Two batches with the state carried over: the bytes of the model over the oracle's per-slot streams in ONE call (the history line
    follows the slot), the end states of the full run, three runs per batch."""
    p, full, full_st, alone = batch
    rng = np.random.default_rng(24)
    g = rng.integers(1, 700, size=p.shape)
    sof = [0, 0, 2]
    el = np.radians(35.0) + 1e-5 * np.arange(4)  # per epoch and the one behind the batch
    spec = ((refl_model.GROUND, [2.0], -6.0, 180.0), (refl_model.WALL, [100.0, 0.3], -3.0, 170.0), (refl_model.GROUND, [40.0], 2.0, 10.0))
    rows = refl_model.rows(3, 3)
    for k, (kind, geo, rel_db, ph) in enumerate(spec):
        x = [pkg.refl_geom(kind, geo, 3.3, float(e)) for e in el]
        for e in range(3):
            rows[e, k] = pkg.refl_row(x[e], x[e + 1], rel_db, ph, FS, N, int(g[e, sof[k]]))
            assert tuple(rows[e, k].tolist()) == refl_model.row(x[e], x[e + 1], rel_db, ph, FS, N, int(g[e, sof[k]]))
    assert rows["delay"][0].tolist() == [0, 1, 0] and (rows["frac_q12"] > 0).all() and (rows["dph"][:, 1] != 0).all()
    want, want_sat, _ = refl_model.refl(alone, g[:, :3], N, sof, rows, cos1024)
    plain, _ = gain_model.wsum(alone, g[:, :3], N)
    assert np.count_nonzero(want != plain) > 0.5 * want.size
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        a, st_a, sat_a = _run(eng, p[:2], g[:2], sof, rows[:2])
        assert eng.gain_runs() == 3
        b, st_b, sat_b = _run(eng, p[2:], g[2:], sof, rows[2:], st_a)
        assert eng.gain_runs() == 3
        _same(np.concatenate([a, b]), want, N)
        assert sat_a + sat_b == want_sat
        act = full_st["prn"] > 0
        assert np.array_equal(st_b["prn"], full_st["prn"])
        assert np.array_equal(st_b["carr_phase"][act].view(np.uint64), full_st["carr_phase"][act].view(np.uint64))
        # no echoes: gal_synth_run_gains, the single-run unity case included
        import torch

        got, _, sat = _run(eng, p, np.full(p.shape, 128), [], None)
        assert eng.gain_runs() == 1 and np.array_equal(got, full) and sat == 0
        got, _, _ = _run(eng, p, g, [], None)
        out = torch.zeros(p.shape[0] * N * 2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        eng.run_gains(p, g, out.data_ptr())
        eng.iq_saturated()
        assert np.array_equal(got, plain) and np.array_equal(out.cpu().numpy(), got)
        # a slot outside the handle's, a row outside the range
        with pytest.raises(pkg.GalSynthError) as e:
            eng.run_refl(p, g, out.data_ptr(), [16, 0, 2], rows)
        assert "part 16" in str(e.value)
        bad = rows.copy()
        bad["delay"][1, 1] = 1024
        with pytest.raises(pkg.GalSynthError) as e:
            eng.run_refl(p, g, out.data_ptr(), sof, bad)
        assert "delay 1024 +" in str(e.value)


@pytest.fixture(scope="module")
def batch6(pkg):
    """3 epochs of 2600 samples, 6 satellites: more slot groups than the four-parts-per-trip body of k_iq_refl takes in one trip.
    Shared, left unchanged: the records, the oracle's end state of the full run, and the oracle's output of every slot alone."""
    p = pkg.workloads.make_synthetic(n_epochs=3, n_chan=6, n_slots=16, samples_per_epoch=N, seed=82)
    _, full_st = oracle_run(p, N, FS)
    alone = np.stack([oracle_run(gain_model.slot_alone(p, s), N, FS)[0] for s in range(6)])
    for a in (p, full_st, alone):
        a.setflags(write=False)
    return p, full_st, alone


def test_run_refl_with_six_groups(pkg, cos1024, batch6):
    """Echoes on five of six slots, two of them on slot 1; slot 4 has none.  Every slot with an echo is a run of its own and slot 4 is
    the one run of the rest: six runs per batch, six parts for k_iq_refl -- one trip of four and two single
    ones.  Two batches with the state carried over: the bytes and the count of the model over the oracle's per-slot streams in ONE
    call, the end states of the full run."""
    p, full_st, alone = batch6
    assert (p["prn"][:, :6] > 0).all() and not (p["prn"][:, 6:] > 0).any()
    rng = np.random.default_rng(27)
    g = rng.integers(1, 700, size=p.shape)
    sof = [0, 1, 1, 2, 3, 5]
    rows = _random_rows(rng, 3, len(sof), 300)
    rows["delay"][0], rows["frac_q12"][0] = (1023, 1024, 0, 3, 4, 255), (4095, 0, 1, 2048, 4095, 1000)  # the first batch reads zeros
    want, want_sat, _ = refl_model.refl(alone, g[:, :6], N, sof, rows, cos1024)
    plain, _ = gain_model.wsum(alone, g[:, :6], N)
    assert np.count_nonzero(want != plain) > 0.5 * want.size
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=16, device=0) as eng:
        a, st_a, sat_a = _run(eng, p[:2], g[:2], sof, rows[:2])
        assert eng.gain_runs() == 5 + 1
        b, st_b, sat_b = _run(eng, p[2:], g[2:], sof, rows[2:], st_a)
        assert eng.gain_runs() == 5 + 1
        _same(np.concatenate([a, b]), want, N)
        assert sat_a + sat_b == want_sat
        act = full_st["prn"] > 0
        assert np.array_equal(st_b["prn"], full_st["prn"])
        assert np.array_equal(st_b["carr_phase"][act].view(np.uint64), full_st["carr_phase"][act].view(np.uint64))
