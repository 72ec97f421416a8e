"""k_synth_g's group start in fixed point (synth_group.hip, SG_FIX): the BOC(1,1) bin-table instances keep the chip phase of a
group as ONE biased double -- high word = half-chip index, low word = fraction in units of 2^-32 -- and compare the fraction word
with integer thresholds.  Output must stay the oracle's, int16 by int16; which groups are listed for k_repair_g is checked against
a CPU model of the listing rule where the carriers stand still (no group is listed for a carrier index then)."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle_binding import oracle_run
from test_parity_gpu import _compare

pytestmark = pytest.mark.gpu

N = 52000
RATE = 2.6e6
BINS = 128
EDGE = np.float32(2.0 ** -20)   # RW_EDGE
DELTA = 2.0 ** -22              # RW_DELTA: the undecided band on either side of a threshold
# the kernel's fraction word against the exact rational phase of a group start computed from the chunk's checkpoint: the loader's
# and the fma's rounding, 2^-33 each, and the word's own grid 2^-32
SLACK = 2.0 ** -31


def _s_of(f_code, rate=RATE):
    """The code step in half chips per sample as the plan computes it: 2 x fl(f_code x fl(1 / rate)) (the doubling is exact)."""
    return 2.0 * float(np.float64(f_code) * (np.float64(1.0) / np.float64(rate)))


def _thresholds(s):
    """The kernel's 15 pattern thresholds T_u = 1 - frac(u s) of a channel, rounded to float as it keeps them, sorted."""
    t = []
    for u in range(1, 16):
        us = float(u) * s
        t.append(np.float32(1.0 - (us - math.floor(us))))
    return sorted(t)


def _bin_rule(thr):
    """Per bin: (undecidable, threshold or None) by build_bins' rules -- the thresholds registered in a bin are those in
    [b / 128 - 2^-20, (b + 1) / 128 + 2^-20), float compares; two of them, or one beside 0 (bin 0) or 1 (the last bin), leave the bin
    undecidable; bin 0 compares with 0 and the last bin with 1 otherwise."""
    rule = []
    for b in range(BINS):
        lo = np.float32(b) * np.float32(1.0 / BINS) - EDGE
        hi = np.float32(b + 1) * np.float32(1.0 / BINS) + EDGE
        inside = [t for t in thr if not (t < lo) and t < hi]
        edge = b in (0, BINS - 1)
        if len(inside) >= 2 or (edge and inside):
            rule.append((True, None))
        elif edge:
            rule.append((False, 0.0 if b == 0 else 1.0))
        else:
            rule.append((False, float(inside[0]) if inside else None))
    return rule


def _group_fracs(x0, cstep, n_samp):
    """Fraction of the half-chip phase at every group start of one epoch, from the chunk checkpoints of the SEQUENTIAL chain
    (x += cstep, rounded; the wrap at 4092 chips is taken before a sample is used and is an integer of half chips)."""
    x = float(x0)
    fr = []
    s = 2.0 * cstep
    for n in range(0, n_samp, 1024):
        if n:
            for _ in range(1024):
                if x >= 4092.0:
                    x -= 4092.0
                x = x + cstep
        groups = (min(1024, n_samp - n) + 15) // 16
        yc = Fraction(x) * 2
        for g in range(groups):
            y = yc + Fraction(s) * (16 * g)
            fr.append(float(y - math.floor(y)))
    return np.array(fr)


def _dist(f, t):
    """Distance of a fraction from a bin's threshold on the circle (0 and 1 are the same point: a fraction just below 1 is looked up in
    the last bin, whose threshold is 1); no threshold: far."""
    if t is None:
        return 1.0
    d = abs(f - t)
    return min(d, 1.0 - d)


def _listed_bounds(fr, thr):
    """(certainly listed, possibly listed) masks over the groups of one channel by the fixed-point rule: listed iff the bin is
    undecidable or |fraction - threshold| <= 2^-22; SLACK on the fraction on either side, at the band's ends and at the bins' edges."""
    rule = _bin_rule(thr)
    sure = np.zeros(len(fr), bool)
    maybe = np.zeros(len(fr), bool)
    for off, into in ((0.0, None), (-SLACK, maybe), (SLACK, maybe)):
        b = np.floor(((fr + off) % 1.0) * BINS).astype(int).clip(0, BINS - 1)
        for k in range(len(fr)):
            und, t = rule[b[k]]
            d = _dist(fr[k], t)
            if into is None:
                sure[k] = (und or d <= DELTA - SLACK)
                maybe[k] |= (und or d <= DELTA + SLACK)
            else:
                into[k] |= (und or d <= DELTA + SLACK)
    # a fraction within SLACK of a bin edge may be looked up in either bin: certain only if both agree
    b_lo = np.floor(((fr - SLACK) % 1.0) * BINS).astype(int).clip(0, BINS - 1)
    b_hi = np.floor(((fr + SLACK) % 1.0) * BINS).astype(int).clip(0, BINS - 1)
    for k in np.flatnonzero(b_lo != b_hi):
        ok = True
        for bb in (b_lo[k], b_hi[k]):
            und, t = rule[bb]
            ok &= und or _dist(fr[k], t) <= DELTA - SLACK
        sure[k] = ok
    return sure, maybe


def _one_still_channel(pkg, seed, f_code=None):
    """Two epochs of one channel whose carrier stands still (step exactly 0: no sample is ever undecided for its table index)."""
    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=1, n_slots=4, samples_per_epoch=N, seed=seed)
    p["f_carr"][:, 0] = 0.0
    if f_code is not None:
        p["f_code"][:, 0] = f_code
    return p


def _place(p, s, target, g):
    """Start code phase of epoch 0 (chips, a double) that puts the fraction of group g of the first chunk at `target` (mod 1), and
    the fraction it really gets, both in exact rational arithmetic."""
    want = (Fraction(target) - Fraction(s) * (16 * g)) % 1
    x0 = float((want + 200) / 2)  # a phase of about 100 chips: its grid is 2^-46
    y = Fraction(x0) * 2 + Fraction(s) * (16 * g)
    return x0, y - math.floor(y)


OFFSETS = [-2.0 ** -20, -2.0 ** -22 - 2.0 ** -30, -2.0 ** -23, 0.0, 2.0 ** -23, 2.0 ** -22 + 2.0 ** -30]


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("kind", ["mid_bin", "bin_edge", "zero", "one"])
def test_thresholds_at_their_edges(pkg, kind, off):
    """A chosen group's start fraction at -2^-20 .. +(2^-22 + 2^-30) of a pattern threshold in the middle of its bin, of one within
    2^-20 of a bin edge (step 101/128 - 2^-21: every T_u sits u x 2^-21 above an edge), of 0 and of 1: equal to the oracle, the group
    counted among the repaired ones inside +-2^-22, and the whole count inside the CPU model's bounds."""
    if kind == "bin_edge":
        p = _one_still_channel(pkg, 41, f_code=(101.0 / 128.0 - 2.0 ** -21) * RATE / 2.0)
    else:
        p = _one_still_channel(pkg, 42)
    cstep = float(np.float64(p["f_code"][0, 0]) * (np.float64(1.0) / np.float64(RATE)))
    s = 2.0 * cstep
    assert s == _s_of(p["f_code"][0, 0])
    thr = _thresholds(s)
    if kind == "mid_bin":
        T = next(float(t) for t in thr if 0.3 < (float(t) * BINS) % 1.0 < 0.7)
    elif kind == "bin_edge":
        T = next(float(t) for t in thr if (float(t) * BINS) % 1.0 < 2.0 ** -20 * BINS)
    else:
        T = 0.0 if kind == "zero" else 1.0
    g = 37
    x0, got = _place(p, s, (Fraction(T) + Fraction(off)) % 1, g)
    assert abs(float((got - Fraction(T) - Fraction(off) + Fraction(1, 2)) % 1 - Fraction(1, 2))) < 2.0 ** -40
    p["code_phase0"][0, 0] = x0
    _, _, stats = _compare(pkg, p, N)
    assert stats["kernel_family"] == 1 and stats["window_mode"] == 1 and stats["chain_mismatch"] == 0, stats
    sure = maybe = 0
    for e in range(2):
        fr = _group_fracs(p["code_phase0"][e, 0], cstep, N)
        a, b = _listed_bounds(fr, thr)
        if e == 0 and abs(off) < DELTA:
            assert a[g], "the model does not list the placed group"
        if e == 0 and abs(off) > DELTA:
            assert not b[g], "the model lists the placed group"
        sure += int(a.sum())
        maybe += int(b.sum())
    print("kind %s off %+.3e: repaired %d, model %d .. %d" % (kind, off, stats["repaired_groups"], sure, maybe))
    assert sure <= stats["repaired_groups"] <= maybe, (stats["repaired_groups"], sure, maybe)
    if abs(off) < DELTA:
        assert stats["repaired_groups"] >= 1


@pytest.mark.parametrize("n_chan", [12, 24])
@pytest.mark.parametrize("rate", [2.6e6, 4.0e6, 10.0e6, 16.0e6])
def test_each_window_form_and_both_widths(pkg, rate, n_chan, monkeypatch):
    """Every form of the resampled window (2.6: holds, 4.0: any pattern, 10.0: <= 4 advances, 16.0: <= 2) on the instances for up to
    12 positions and on the wide ones (24 positions in one launch: the hooks build's GAL_G_WIDE, the plan picks them for long batches)."""
    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=n_chan, n_slots=24, samples_per_epoch=N, sample_rate=rate, seed=int(rate / 1e5) + n_chan)
    p["ibit0"][0, :2] = [499, 0]
    p["code_phase0"][0, :2] = [4091.9, 4085.0]
    p["carr_phase0"][0, 3:5] = 0.0  # listed groups for certain
    if n_chan > 12:
        monkeypatch.setenv("GAL_G_WIDE", "1")
    _, _, stats = _compare(pkg, p, N, rate=rate, test_hooks=n_chan > 12)
    assert stats["kernel_family"] == 1 and stats["chain_mismatch"] == 0 and stats["chunk_samples"] == 1024, stats
    # the form itself, without the bisection flag (+ 16): such a batch would run neither the fixed-point path nor the wide instances
    print("rate %.1f MS/s, %d channels: window_mode %d" % (rate / 1e6, n_chan, stats["window_mode"]))
    assert stats["window_mode"] == {2.6e6: 1, 4.0e6: 4, 10.0e6: 3, 16.0e6: 2}[rate], stats
    assert stats["repaired_groups"] >= 1 and stats["exact_records"] == 0, stats


def test_more_than_24_channels_runs_an_accumulating_launch(pkg):
    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=29, n_slots=32, samples_per_epoch=N, seed=529)
    p["carr_phase0"][0, 20:26] = 0.0
    _, _, stats = _compare(pkg, p, N)
    assert stats["kernel_family"] == 1 and stats["chain_mismatch"] == 0 and stats["n_active_max"] == 29 and stats["window_mode"] == 1, stats
    assert stats["repaired_groups"] >= 1


@pytest.mark.parametrize("where", [0, 1, 15, 16])
def test_code_wrap_inside_the_window_at_group_positions(pkg, where):
    """The code wrap after 2000 + `where` samples of epoch 0 (2000 = 125 groups): at the first, second and last sample of a group and
    at the first of the next one, with the symbol's sign changing across it."""
    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=4, n_slots=4, samples_per_epoch=N, seed=950 + where)
    step = p["f_code"][0, :4] / RATE
    p["code_phase0"][0, :4] = 4092.0 - (2000 + where) * step + np.array([0.0, 1e-9, -1e-9, 0.3]) * step
    p["ibit0"][0, :4] = [10, 499, 24, 498]
    _, _, stats = _compare(pkg, p, N)
    assert stats["kernel_family"] == 1 and stats["chain_mismatch"] == 0 and stats["window_mode"] == 1, stats


def test_integer_part_at_its_limits(pkg):
    """A wrap that is pending at a chunk's first sample (the phase reaches 4092 chips with sample 1024 / 2048 exactly), a chunk that
    starts just below the wrap (its last group has the largest half-chip index the window row holds: 8184 + 1008), and an idle
    position: a channel that leaves after the first epoch, so the instance for 5 positions runs with 4 active."""
    p = pkg.workloads.make_synthetic(n_epochs=3, n_chan=5, n_slots=8, samples_per_epoch=N, seed=960)
    step = p["f_code"][0, :5] / RATE
    p["code_phase0"][0, 0] = 4092.0 - 1024 * step[0] + 1e-7            # pending at the first sample of chunk 1
    p["code_phase0"][0, 1] = 4092.0 - 2048 * step[1] + 0.5 * step[1]   # ... of chunk 2, by half a sample
    p["code_phase0"][0, 2] = 4092.0 - 1024 * step[2] - 1e-7            # chunk 1 starts just below the wrap
    p["code_phase0"][0, 3] = 4092.0 - 3072 * step[3] - 0.5 * step[3]   # ... chunk 3, by half a sample
    p["code_phase0"][1, 0] = 4091.9999999                              # the epoch itself starts just below it
    p["code_phase0"][2, 1] = 6137.9                                    # a pending wrap that lands mid-period
    p["ibit0"][0, :4] = [499, 498, 0, 250]
    p[1:, 4] = np.zeros((), dtype=p.dtype)
    _, _, stats = _compare(pkg, p, N)
    assert stats["kernel_family"] == 1 and stats["chain_mismatch"] == 0 and stats["n_active_max"] == 5 and stats["window_mode"] == 1, stats


def test_float_path_still_in_use_on_the_bisection_instances(pkg):
    n = 49104  # 12 ms at 4.092 MS/s: two samples per half chip, all 15 thresholds on top of each other
    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=6, n_slots=8, samples_per_epoch=n, sample_rate=4.092e6, seed=4092)
    p["carr_phase0"][0, :2] = 0.0
    _, _, stats = _compare(pkg, p, n, rate=4.092e6)
    assert stats["kernel_family"] == 1 and stats["window_mode"] == 4 + 16 and stats["chain_mismatch"] == 0, stats


def test_float_path_still_in_use_in_the_cboc_mode(pkg):
    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=7, n_slots=8, samples_per_epoch=N, seed=611)
    p["ibit0"][0, 0] = 499
    p["code_phase0"][0, 0] = 4091.9
    p["carr_phase0"][0, :3] = 0.0
    ref_iq, _ = oracle_run(p, N, RATE, cboc=True)
    with pkg.SynthEngine(samples_per_epoch=N, n_slots=8, device=0, flags=pkg.synth.GAL_CFG_CBOC) as eng:
        iq, _, stats = eng.run_host(p)
    assert stats["chain_mismatch"] == 0 and stats["kernel_family"] == 1, stats
    assert np.array_equal(iq, ref_iq)


# repaired_groups of this batch with the float group start (the commit before the fixed-point one), measured on an MI355X:
# profiles/r09_group_start_listed.log
LISTED_BEFORE = 88


def test_listing_does_not_grow(pkg):
    """12 channels x 64 epochs x 260000 samples: the finer fraction should list no more groups than the float one did; 10 % on top
    for the groups that move across the band's edge."""
    import torch

    from oracle_binding import oracle_matches_device

    p = pkg.workloads.make_synthetic(n_epochs=64, n_chan=12, n_slots=16, samples_per_epoch=260000, seed=20250919)
    with pkg.SynthEngine(samples_per_epoch=260000, n_slots=16, device=0) as eng:
        eng.plan(p)
        out = torch.empty(eng.output_bytes() // 2, dtype=torch.int16, device="cuda")
        eng.execute(out.data_ptr())
        _, stats = eng.finish()
    print("repaired_groups %d (before: %s)" % (stats["repaired_groups"], LISTED_BEFORE))
    assert stats["chain_mismatch"] == 0 and stats["kernel_family"] == 1, stats
    bad, _ = oracle_matches_device(out, p, 260000, RATE)
    assert bad == 0, "%d int16 values differ from the oracle" % bad
    assert stats["repaired_groups"] <= LISTED_BEFORE * 1.10, (stats["repaired_groups"], LISTED_BEFORE)
