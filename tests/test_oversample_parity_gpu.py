"""The rates of galileo-sdr-sim --oversample M (M x 2.6 MS/s, M = 2 .. 15) through the library against the oracle, int16 by int16 and
the end state as uint64: every M on epochs of 1.25 code periods and an odd length, in one batch and in two with the state carried;
M = 6 and 15 on epochs of the product's length (M x 260 000 samples); and batches whose records take TWO window forms -- 7.8 and
15.6 MS/s lie 1.4 % inside their form (gal_synth_plan's rw_mode_of switches at a code step of 0.266 and 0.133 half chips per sample) --,
which is what the majority choice, the accumulating exact-replay launch for the minority and the switch back to k_synth are for.

What the plan should choose is derived here from the gate as csrc/synth_api.cpp states it, never from what the engine reports."""
import numpy as np
import pytest

from oracle_binding import oracle_run

pytestmark = pytest.mark.gpu

FS = 2.6e6
CARR_TO_CODE = 0.0006493506493506494  # 1 / 1540: the front end's f_code = 1.023e6 + f_carr / 1540
MIN_GAP, MIN_GAP_CBOC = 1.0 / 128.0 + 4e-6, 1.0 / 64.0 + 4e-6  # kRwMinGap, kRwMinGapCboc
GROUP_SYMS = 64  # kGroupSyms


def _form(cs2):
    """rw_mode_of for the steps of these rates (below 0.74 half chips per sample): 4 above 0.266, 3 above 0.133, 2 from 0.0083."""
    assert 0.0083 <= cs2 < 0.74
    return 4 if cs2 > 0.266 else 3 if cs2 > 0.133 else 2


def _bins_ok(cs2, cboc):
    """rw_threshold_gap and rw_threshold_edge: the 15 pattern thresholds 1 - frac(u s) lie more than a bin from each other and from 0
    and 1 (CBOC: those of the BOC(6,1) half periods, step 6 s, too, in bins twice as wide)."""
    need = MIN_GAP_CBOC if cboc else MIN_GAP
    for s in (cs2, 6.0 * cs2) if cboc else (cs2,):
        t = np.sort(1.0 - np.mod(np.arange(1, 16) * s, 1.0))
        if not (np.diff(t).min() > need and min(t.min(), 1.0 - t.max()) > need):
            return False
    return True


def _plan_of_the_gate(p, n, rate, cboc=False):
    """gal_synth_plan's choice for a batch on automatic chunking, as the gate is written: every record's form; k_synth_g takes the
    form most records have (on a tie the lower number) if no more than half of the epochs hold a record of another form, and the
    others go to the exact-replay launch behind it.  Returns (k_synth_g?, form, records of the exact launch, bisection instances?)."""
    E = p.shape[0]
    on = p["prn"] > 0
    cs2 = 2.0 * (p["f_code"] * (1.0 / rate))
    ad = np.abs(p["f_carr"] * (1.0 / rate))
    assert ((ad[on] >= 2.0 ** -40) & (511.0 * ad[on] * 16.0 <= 120.0)).all()  # the carrier gate admits every record of these tests
    form = np.zeros(p.shape, dtype=int)
    bins = np.zeros(p.shape, dtype=bool)
    for e, s in zip(*np.nonzero(on)):
        form[e, s] = _form(cs2[e, s])
        bins[e, s] = _bins_ok(cs2[e, s], cboc)
    fit = on & (bins | (not cboc))  # (the CBOC mode has bin tables only)
    count = [int((fit & (form == m)).sum()) for m in range(5)]
    g_mode = 1
    for m in (2, 3, 4):
        if count[m] > count[g_mode]:
            g_mode = m
    mine = fit & (form == g_mode)
    n_exact_epochs = int((on & ~mine).any(axis=1).sum())
    fam_g = (count[g_mode] > 0 and 2 * n_exact_epochs <= E and n * cs2[on].max() / (2.0 * 4092.0) + 4.0 < GROUP_SYMS)
    return fam_g, g_mode, int((on & ~mine).sum()), bool((mine & ~bins).any())


def _run(pkg, p, n, rate):
    with pkg.SynthEngine(sample_rate=rate, samples_per_epoch=n, n_slots=p.shape[1], device=0) as eng:
        return eng.run_host(p)


def _same(iq, st, stats, ref_iq, ref_st, what):
    """test_parity_gpu.py's _compare: the samples int16 by int16, the end state bitwise."""
    assert stats["chain_mismatch"] == 0, what
    nbad = int(np.count_nonzero(iq != ref_iq))
    assert nbad == 0, "%s: %d of %d int16 values differ (first at %d)" % (what, nbad, iq.size, int(np.flatnonzero(iq != ref_iq)[0]))
    act = ref_st["prn"] > 0
    assert np.array_equal(st["prn"], ref_st["prn"]), what
    assert np.array_equal(st["carr_phase"][act].view(np.uint64), ref_st["carr_phase"][act].view(np.uint64)), what
    assert np.array_equal(st["page"][act], ref_st["page"][act]), what


def _every_rate(pkg, M, cboc):
    rate = M * FS
    n = M * 13000 + 1  # 1.25 code periods, odd: the wrap moves through the chunks from epoch to epoch
    p = pkg.workloads.make_synthetic(n_epochs=3, n_chan=6, n_slots=8, samples_per_epoch=n, sample_rate=rate, seed=2600 + M)
    p["f_code"][:, :6] = 1.023e6 + p["f_carr"][:, :6] * CARR_TO_CODE
    flags = pkg.synth.GAL_CFG_CBOC if cboc else 0
    ref_iq, ref_st = oracle_run(p, n, rate, cboc=cboc)
    fam_g, form, n_exact, search = _plan_of_the_gate(p, n, rate, cboc)
    assert form == _form(2 * 1.023 / (M * 2.6)) and n_exact == 0
    # the gate as written admits k_synth_g at every one of these rates, in both modes: the steps of M = 3, 6 and 15 keep their
    # thresholds a CBOC bin apart; M = 11 (a step of 1 / 13.98) crowds them and runs BOC(1,1) on the bisection instances
    assert fam_g and search == (M == 11)
    with pkg.SynthEngine(sample_rate=rate, samples_per_epoch=n, n_slots=8, device=0, flags=flags) as eng:
        iq, st, stats = eng.run_host(p)
        print("M %2d %s: kernel_family %d window_mode %d exact_records %d" % (M, "CBOC" if cboc else "BOC ", stats["kernel_family"],
                                                                             stats["window_mode"], stats["exact_records"]))
        _same(iq, st, stats, ref_iq, ref_st, "one batch")
        assert stats["window_mode"] & 15 == form and (stats["window_mode"] >= 16) == search, stats
        assert stats["kernel_family"] == 1 and stats["exact_records"] == 0, stats
        # 1 + 2 epochs with the state carried
        iq_a, st_a, stats_a = eng.run_host(p[:1])
        iq_b, st_b, stats_b = eng.run_host(p[1:], st_a)
        _same(np.concatenate([iq_a, iq_b]), st_b, stats_b, ref_iq, ref_st, "two batches")
        assert stats_a["chain_mismatch"] == 0 and stats_a["kernel_family"] == stats_b["kernel_family"] == 1


@pytest.mark.parametrize("M", range(2, 16))
def test_every_oversampled_rate(pkg, M):
    _every_rate(pkg, M, False)


@pytest.mark.parametrize("M", [3, 6, 15])
def test_every_oversampled_rate_cboc(pkg, M):
    _every_rate(pkg, M, True)


@pytest.mark.parametrize("M", [6, 15])
def test_full_length_epochs(pkg, M):
    """The product's epochs: 0.1 s = M x 260 000 samples, 25 symbols each, sample indices up to 3.9 M per epoch; one slot is
    re-allocated to another PRN in epoch 1."""
    from galileo_sdr_sim_amd import GAL_CH_RESTART

    rate, n = M * FS, M * 260000
    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=3, n_slots=4, samples_per_epoch=n, sample_rate=rate, seed=2700 + M)
    q = pkg.workloads.make_synthetic(n_epochs=2, n_chan=1, n_slots=4, samples_per_epoch=n, sample_rate=rate, seed=2800 + M, prns=[33])
    p[1, 1] = q[1, 0]
    p["flags"][1, 1] = GAL_CH_RESTART
    p["carr_phase0"][1, 1] = 0.625
    p["page_init"][1, 1] = q["page_next"][0, 0]
    p["f_code"][:, :3] = 1.023e6 + p["f_carr"][:, :3] * CARR_TO_CODE
    ref_iq, ref_st = oracle_run(p, n, rate)
    fam_g, form, n_exact, search = _plan_of_the_gate(p, n, rate)
    assert fam_g and form == 2 and n_exact == 0 and not search
    iq, st, stats = _run(pkg, p, n, rate)
    _same(iq, st, stats, ref_iq, ref_st, "M %d" % M)
    assert stats["kernel_family"] == 1 and stats["window_mode"] == 2 and stats["exact_records"] == 0, stats


# records of the other form, [epoch, channel] of 4 epochs x 6 channels
def _minority(*cells):
    m = np.zeros((4, 6), dtype=bool)
    for e, j in cells:
        m[e, j] = True
    return m


TWO_FORMS = {
    "one_record": _minority((2, 4)),                                      # k_synth_g + one record on the accumulating launch
    "one_epoch_of_four": _minority((1, 0), (1, 3), (1, 5)),               # fewer than half of the epochs
    "two_epochs_of_four": _minority((0, 2), (3, 2)),                      # exactly half: 2 x 2 <= 4 still splits
    "three_epochs_of_four": _minority((0, 1), (1, 1), (3, 1)),            # more than half: the batch leaves k_synth_g
    "equal_split_by_epochs": _minority(*[(e, j) for e in (0, 1) for j in range(6)]),   # 12 : 12, half of the epochs: the tie decides
    "equal_split_by_channels": _minority(*[(e, j) for e in range(4) for j in (0, 2, 4)]),  # 12 : 12 in every epoch
}


@pytest.mark.parametrize("case", sorted(TWO_FORMS))
@pytest.mark.parametrize("M", [3, 6])
def test_two_window_forms_in_one_batch(pkg, M, case):
    """7.8 MS/s: nominal records take form 3 (step 0.2623), the others a code rate of 1 040 520 Hz, a step of 0.2668: form 4.  15.6
    MS/s: 0.1312 is form 2, the same code rate's 0.1334 form 3.  (The API admits any f_code with f_code / fs in [2^-20, 0.5].)"""
    rate, n, E = M * FS, 4 * 1024 + 17, 4
    other = TWO_FORMS[case]
    p = pkg.workloads.make_synthetic(n_epochs=E, n_chan=6, n_slots=8, samples_per_epoch=n, sample_rate=rate, seed=2900 + M)
    f_code = 1.023e6 + p["f_carr"][:, :6] * CARR_TO_CODE
    f_code[other] += 1040520.0 - 1.023e6
    p["f_code"][:, :6] = f_code
    nominal = _form(2 * 1.023 / (M * 2.6))
    assert nominal == {3: 3, 6: 2}[M] and _form(2 * 1040520.0 / rate) == nominal + 1
    fam_g, form, n_exact, search = _plan_of_the_gate(p, n, rate)
    n_other = int(other.sum())
    want = {"one_record": (True, nominal, 1), "one_epoch_of_four": (True, nominal, 3), "two_epochs_of_four": (True, nominal, 2),
            "three_epochs_of_four": (False, nominal, 3), "equal_split_by_epochs": (True, nominal, 12),
            "equal_split_by_channels": (False, nominal, 12)}[case]
    assert (fam_g, form, n_exact) == want and n_exact == n_other and not search
    ref_iq, ref_st = oracle_run(p, n, rate)
    iq, st, stats = _run(pkg, p, n, rate)
    print("M %d %s: kernel_family %d window_mode %d exact_records %d" % (M, case, stats["kernel_family"], stats["window_mode"],
                                                                         stats["exact_records"]))
    _same(iq, st, stats, ref_iq, ref_st, case)
    if fam_g:
        assert stats["kernel_family"] == 1 and stats["window_mode"] == form and stats["exact_records"] == n_exact, stats
    else:
        # k_synth's resampled windows need ONE form on every record: classic windows
        assert stats["kernel_family"] != 1 and stats["window_mode"] == 0 and stats["exact_records"] == 0, stats
