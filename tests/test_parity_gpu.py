"""GPU parity: the HIP path (through the C-ABI) against the oracle, bit for bit, on seeded inputs.
int16 IQ is integer work: the bar is exact equality, pre-quantisation tolerance is 0."""
import os

import numpy as np
import pytest

from oracle_binding import oracle_matches_device, oracle_run

pytestmark = pytest.mark.gpu


def _compare(pkg, params, n_samp, rate=2.6e6, state_in=None, **eng_kw):
    n_slots = params.shape[1]
    with pkg.SynthEngine(sample_rate=rate, samples_per_epoch=n_samp, n_slots=n_slots, device=0, **eng_kw) as eng:
        return _compare_on(eng, params, n_samp, rate, state_in)


def _compare_on(eng, params, n_samp, rate=2.6e6, state_in=None, cboc=False):
    """_compare's run and checks on an engine the caller keeps (many batches through one handle); cboc: against the oracle's CBOC loop."""
    iq, st, stats = eng.run_host(params, state_in)
    ref_iq, ref_st = oracle_run(params, n_samp, rate, state_in, cboc=cboc)
    assert stats["chain_mismatch"] == 0
    nbad = int(np.count_nonzero(iq != ref_iq))
    assert nbad == 0, "%d of %d int16 values differ (first at %d)" % (nbad, iq.size, int(np.flatnonzero(iq != ref_iq)[0]))
    act = ref_st["prn"] > 0
    assert np.array_equal(st["prn"], ref_st["prn"])
    assert np.array_equal(st["carr_phase"][act].view(np.uint64), ref_st["carr_phase"][act].view(np.uint64))
    assert np.array_equal(st["page"][act], ref_st["page"][act])
    return iq, st, stats


@pytest.mark.parametrize("n_chan", [1, 4, 9, 12])
def test_small_batches_bit_exact(pkg, n_chan):
    p = pkg.workloads.make_synthetic(n_epochs=4, n_chan=n_chan, n_slots=16, samples_per_epoch=26000, seed=100 + n_chan)
    _compare(pkg, p, 26000)


def test_full_epoch_size_bit_exact(pkg):
    """Reference geometry: 260000 samples per epoch, 12 channels, several epochs."""
    p = pkg.workloads.make_synthetic(n_epochs=6, n_chan=12, n_slots=16, samples_per_epoch=260000, seed=5)
    iq, st, stats = _compare(pkg, p, 260000)  # the default kernel of this geometry: 16-sample groups out of 1024-sample chunks
    assert stats["kernel_family"] == 1 and stats["chunk_samples"] == 1024 and stats["chunks_per_epoch"] == 254
    iq, st, stats = _compare(pkg, p, 260000, flags=4)  # GAL_CFG_EXACT_REPLAY: one chunk per lane
    # a batch this small gets short chunks (one block per CU would need 65536 of them) that still divide the code period
    assert stats["chunk_samples"] == 416 and stats["chunks_per_epoch"] == 625 and 10400 % stats["chunk_samples"] == 0
    iq, st, stats = _compare(pkg, p, 260000, chunk_samples=1040)
    assert stats["chunk_samples"] == 1040 and stats["chunks_per_epoch"] == 250


def test_chunk_length_follows_the_batch_size(pkg):
    """The exact-replay kernel (GAL_CFG_EXACT_REPLAY; the default kernel of this geometry always takes 1024-sample chunks):
    gal_synth_plan picks the chunk length from the batch size: ~1024 samples (1040 = a tenth of the code period at
    2.6 MS/s) from 263 epochs on, shorter for batches that would otherwise leave CUs without a block; same bits either way
    (the full-size tests cover 1040 against 1024 / 520)."""
    for n_ep, want in ((1, 416), (64, 416), (128, 416), (300, 1040)):
        p = pkg.workloads.make_synthetic(n_epochs=n_ep, n_chan=3, n_slots=4, samples_per_epoch=260000, seed=40 + n_ep)
        with pkg.SynthEngine(samples_per_epoch=260000, n_slots=4, device=0, flags=4) as eng:
            eng.plan(p)
            assert eng.output_bytes() == n_ep * 260000 * 4
            import torch

            out = torch.empty(eng.output_bytes() // 2, dtype=torch.int16, device="cuda")
            eng.execute(out.data_ptr())
            _, stats = eng.finish()
        assert stats["chunk_samples"] == want and stats["chain_mismatch"] == 0, (n_ep, stats)
        if n_ep <= 64:
            ref_iq, _ = oracle_run(p[:2], 260000, 2.6e6)
            assert np.array_equal(out[: ref_iq.size].cpu().numpy(), ref_iq)


def test_page_flip_mid_epoch(pkg):
    """ibit0 near 499 forces the symbol counter to wrap (page_next installed) inside the first epochs."""
    p = pkg.workloads.make_synthetic(n_epochs=3, n_chan=6, n_slots=16, samples_per_epoch=260000, seed=9)
    p["ibit0"][0, :6] = [499, 498, 480, 476, 0, 250]
    # keep later epochs consistent with the forced start (as geometry would)
    for e in range(1, 3):
        p["ibit0"][e, :6] = (p["ibit0"][0, :6] + 25 * e) % 500
    _compare(pkg, p, 260000)


def test_negative_and_tiny_doppler(pkg):
    p = pkg.workloads.make_synthetic(n_epochs=5, n_chan=8, n_slots=16, samples_per_epoch=52000, seed=11)
    f = np.array([-3400.0, -1000.0, -3.0, -0.02, 0.03, 2.5, 700.0, 3499.0])
    for e in range(5):
        p["f_carr"][e, :8] = f + 0.01 * e * np.sign(f)
        p["f_code"][e, :8] = 1.023e6 + p["f_carr"][e, :8] * 0.0006493506493506494
    _compare(pkg, p, 52000)


def test_doppler_sign_change_between_epochs(pkg):
    p = pkg.workloads.make_synthetic(n_epochs=8, n_chan=3, n_slots=16, samples_per_epoch=52000, seed=12)
    for j in range(3):
        f = np.linspace(40.0, -40.0, 8) * (j + 1)
        p["f_carr"][:, j] = f
        p["f_code"][:, j] = 1.023e6 + f * 0.0006493506493506494
    _compare(pkg, p, 52000)


def test_ragged_sizes(pkg):
    """samples_per_epoch not a multiple of the chunk, tiny epochs, odd chunk sizes."""
    for n_samp, chunk in [(1000, 0), (2604, 0), (26000, 100), (26000, 252), (4096, 4)]:
        p = pkg.workloads.make_synthetic(n_epochs=3, n_chan=5, n_slots=8, samples_per_epoch=n_samp, seed=n_samp)
        _compare(pkg, p, n_samp, chunk_samples=chunk)


@pytest.mark.parametrize("rate", [2.047e6, 2.2e6, 4.092e6, 10e6])
def test_sample_rates_window_limits(pkg, rate):
    """The 16-half-chip window of k_synth is full at f_code/fs = 0.5 (2.047 MS/s: 15.99 half chips per 16
    samples); high rates give groups that stay inside one chip.  The reference fixes 2.6 MS/s
    (include/constants.h:96); the loop itself is rate-agnostic and so is the oracle."""
    n_samp = int(rate / 100)  # 10 ms epochs: 2.5 code periods each
    p = pkg.workloads.make_synthetic(n_epochs=5, n_chan=6, n_slots=8, samples_per_epoch=n_samp, sample_rate=rate,
                                     seed=int(rate) % 1000)
    _compare(pkg, p, n_samp, rate=rate)
    _compare(pkg, p, n_samp, rate=rate, chunk_samples=64)


@pytest.mark.parametrize("rate,mode", [(2.1e6, 1), (2.2e6, 1), (2.4e6, 1), (2.6e6, 1), (2.76e6, 1),
                                       (2.0462e6, 0), (2.5e6, 17), (2.728e6, 17), (2.77e6, 4), (3.0e6, 4),
                                       (5e6, 4), (7.6e6, 4), (7.8e6, 3), (10e6, 3), (12.5e6, 3), (15.3e6, 3),
                                       (15.5e6, 2), (16e6, 2), (25e6, 2), (40e6, 2), (200e6, 2)])
def test_resampled_window_rates(pkg, rate, mode):
    """k_synth's resampled-window fast body (one chip look-up pattern per 16-sample group, code NCO advanced once per
    group) serves batches with 0.74 <= 2 f_code / fs < 0.9999 whose 15 pattern thresholds are more than a bin apart
    (synth_api.cpp: rw_threshold_gap): the first five rates qualify (2.76 MS/s: four holds per group, the maximum);
    2.0462 MS/s (a code step of 0.9999 half chips: beyond the hold form, classic body), 2.5 MS/s (step ~ 9/11) and 2.728 MS/s
    (step = 3/4) have clustered thresholds: k_synth runs its classic body there (the chunk_samples=208 run below), and the default
    kernel of round 6 finds the patterns of the latter two by bisection (k_synth_g's bisection instances: window_mode 1 + 16;
    rounds 2-5: the whole batch on k_synth's classic body).  From
    15.4 MS/s (code step <= 2/15 half chips) the body's second form takes over: the window ADVANCES at <= 2 samples of
    a group instead of holding at <= 4 (config 4's 25 MS/s); the third form does the same with <= 4 advances (7.7 to
    15.4 MS/s); 2.77, 3, 5 and 7.6 MS/s lie between the forms -- k_synth_g's general form 4 since round 5 (k_synth itself
    runs its classic body there: the chunk_samples=208 run below).
    Epochs of 6.2 code periods so that every lane passes the small binades of the code phase (where the group advance
    has to add sample by sample) and the channel's tie binade."""
    n_samp = int(rate * (0.025 if rate < 5e6 else 0.009 if rate < 100e6 else 0.0045))
    p = pkg.workloads.make_synthetic(n_epochs=4 if rate < 100e6 else 2, n_chan=12, n_slots=12, samples_per_epoch=n_samp,
                                     sample_rate=rate, seed=int(rate) % 997)
    _, _, stats = _compare(pkg, p, n_samp, rate=rate)
    # (+ 16: the patterns found by bisection -- thresholds that crowd; 15.3 MS/s sits at the edge of its form and may go either way)
    assert stats["window_mode"] & 15 == mode & 15 and (stats["window_mode"] >= 16) == (mode >= 16 or rate == 15.3e6 and stats["window_mode"] >= 16)
    _compare(pkg, p, n_samp, rate=rate, chunk_samples=208)


def test_resampled_window_tie_binades(pkg):
    """Code steps whose significand ends in k zero bits put the tie binade of the group advance at 2^k half chips:
    steps built with 1 .. 13 trailing zeros make every binade of the code phase a tie binade for some channel."""
    n_samp = 65000
    p = pkg.workloads.make_synthetic(n_epochs=3, n_chan=12, n_slots=12, samples_per_epoch=n_samp, seed=4242)
    for j in range(12):
        step = float(p["f_code"][0, j]) / 2.6e6  # code step per sample; the kernel doubles it (exact)
        m = np.frombuffer(np.float64(step).tobytes(), dtype=np.uint64)[0]
        k = j + 2
        m = (int(m) >> k << k) | (1 << k)  # significand ends in 1 followed by k zeros
        step2 = np.frombuffer(np.uint64(m).tobytes(), dtype=np.float64)[0]
        p["f_code"][:, j] = step2 * 2.6e6
        # f_code * (1 / fs) must reproduce the crafted step: search the neighbourhood
        f = float(p["f_code"][0, j])
        for _ in range(64):
            if f * (1.0 / 2.6e6) == step2:
                break
            f = np.nextafter(f, f + (1 if f * (1.0 / 2.6e6) < step2 else -1))
        p["f_code"][:, j] = f
    _compare(pkg, p, n_samp)


def test_classic_window_body_at_the_reference_rate(pkg, monkeypatch):
    """The classic fast body (per-sample window index) still serves other sample rates; the GAL_TEST_HOOKS build can be
    told to use it at 2.6 MS/s too, so that both bodies are compared with the oracle on the same batch."""
    monkeypatch.setenv("GAL_SYNTH_RW", "0")
    p = pkg.workloads.make_synthetic(n_epochs=4, n_chan=12, n_slots=16, samples_per_epoch=52000, seed=99)
    _, _, stats = _compare(pkg, p, 52000, test_hooks=True)
    assert stats["window_mode"] == 0
    monkeypatch.delenv("GAL_SYNTH_RW")
    _, _, stats = _compare(pkg, p, 52000, test_hooks=True)
    assert stats["window_mode"] == 1
    # ... and the same at 25 MS/s, 24 channels (two launches, the second accumulating): advance form against classic
    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=24, n_slots=24, samples_per_epoch=250000, sample_rate=25e6, seed=98)
    _, _, stats = _compare(pkg, p, 250000, rate=25e6, test_hooks=True)
    assert stats["window_mode"] == 2
    monkeypatch.setenv("GAL_SYNTH_RW", "0")
    _, _, stats = _compare(pkg, p, 250000, rate=25e6, test_hooks=True)
    assert stats["window_mode"] == 0


@pytest.mark.parametrize("rate,force", [(3.0e6, 11), (2.5e6, 11), (2.0462e6, 11), (10e6, 12), (4.0e6, 12), (2.6e6, 12),
                                        (4.0e6, 13), (2.6e6, 13), (25e6, 13)])
def test_resampled_window_safety_nets(pkg, monkeypatch, rate, force):
    """The host's gate keeps the resampled-window bodies away from rates they do not serve.  Forced onto such rates
    (GAL_TEST_HOOKS build) the kernel's own nets must hold: more holds / advances per group than the pattern masks carry
    (3 MS/s in form 1; 2.6, 4 and 10 MS/s in form 2; 2.6 and 4 MS/s in form 3) turn the block over to the slow body;
    clustered thresholds (2.5 and 2.0462 MS/s in form 1) leave bins undecidable, whose lanes do the same group by group;
    25 MS/s in form 3 is simply the wider form on a rate the narrower one serves."""
    monkeypatch.setenv("GAL_SYNTH_RW", str(force))
    n_samp = int(rate * 0.012)
    p = pkg.workloads.make_synthetic(n_epochs=3, n_chan=8, n_slots=8, samples_per_epoch=n_samp, sample_rate=rate,
                                     seed=int(rate) % 991 + force)
    _, _, stats = _compare(pkg, p, n_samp, rate=rate, test_hooks=True)
    assert stats["window_mode"] == force - 10


def test_code_wrap_at_every_group_position(pkg):
    """Code phases chosen so that the wrap (x >= 4092) falls on each of the 16 positions of a sample group,
    including the first sample (wrap pending from the previous group) and the first sample of a chunk."""
    n_samp, n_slots = 4160, 16  # 4 chunks of 1040 when chunk_samples=1040
    p = pkg.workloads.make_synthetic(n_epochs=3, n_chan=16, n_slots=n_slots, samples_per_epoch=n_samp, seed=77)
    step = p["f_code"][0] / 2.6e6
    for j in range(n_slots):
        # wrap just before sample 1040 + j of the first epoch
        p["code_phase0"][0, j] = 4092.0 - (1040 + j) * step[j] + 0.25 * step[j]
    for chunk in (1040, 0, 16):
        with pkg.SynthEngine(samples_per_epoch=n_samp, n_slots=n_slots, device=0, chunk_samples=chunk) as eng:
            iq, st, stats = eng.run_host(p[:1])
        ref_iq, _ = oracle_run(p[:1], n_samp, 2.6e6)
        assert np.array_equal(iq, ref_iq), chunk


def test_channel_comes_and_goes_and_state_carry(pkg):
    """Slots freed / re-allocated between epochs (src/channel.cpp:112-119) and a run split in two calls."""
    from galileo_sdr_sim_amd import GAL_CH_RESTART

    n_samp = 26000
    p = pkg.workloads.make_synthetic(n_epochs=10, n_chan=6, n_slots=16, samples_per_epoch=n_samp, seed=21)
    # slot 2 disappears at epoch 4; slot 7 appears at epoch 5 with a fresh carrier / page; slot 1 is
    # re-allocated to another PRN at epoch 6
    p[4:, 2] = np.zeros((), dtype=p.dtype)
    q = pkg.workloads.make_synthetic(n_epochs=10, n_chan=1, n_slots=16, samples_per_epoch=n_samp, seed=22, prns=[33])
    p[5:, 7] = q[5:, 0]
    p["flags"][5, 7] = GAL_CH_RESTART
    p["carr_phase0"][5, 7] = 0.625
    p["page_init"][5, 7] = q["page_next"][0, 0]
    r = pkg.workloads.make_synthetic(n_epochs=10, n_chan=1, n_slots=16, samples_per_epoch=n_samp, seed=23, prns=[41])
    p[6:, 1] = r[6:, 0]
    p["flags"][6, 1] = GAL_CH_RESTART
    p["carr_phase0"][6, 1] = 0.125
    p["page_init"][6, 1] = r["page_next"][1, 0]
    iq_all, st_all, _ = _compare(pkg, p, n_samp)
    # same run as two calls carrying gal_chan_state_t across the boundary
    with pkg.SynthEngine(sample_rate=2.6e6, samples_per_epoch=n_samp, n_slots=16, device=0) as eng:
        iq_a, st_a, _ = eng.run_host(p[:7])
        iq_b, st_b, _ = eng.run_host(p[7:], st_a)
    assert np.array_equal(np.concatenate([iq_a, iq_b]), iq_all)
    assert np.array_equal(st_b["carr_phase"].view(np.uint64), st_all["carr_phase"].view(np.uint64))


def test_more_channels_than_one_launch(pkg):
    """> 12 active channels: channel groups, later groups accumulate onto the first."""
    p = pkg.workloads.make_synthetic(n_epochs=3, n_chan=16, n_slots=16, samples_per_epoch=26000, seed=31)
    _compare(pkg, p, 26000)
    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=24, n_slots=24, samples_per_epoch=25000, sample_rate=25e6,
                                     seed=32)
    _compare(pkg, p, 25000, rate=25e6)


def test_invalid_batches_are_rejected(pkg):
    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=2, n_slots=4, samples_per_epoch=1000, seed=1)
    with pkg.SynthEngine(samples_per_epoch=1000, n_slots=4, device=0) as eng:
        bad = p.copy()
        bad["flags"][0, 0] = 0  # continues without state
        with pytest.raises(pkg.GalSynthError):
            eng.run_host(bad)
        bad = p.copy()
        bad["prn"][1, 1] = 51
        with pytest.raises(pkg.GalSynthError):
            eng.run_host(bad)
        bad = p.copy()
        bad["ibit0"][0, 0] = 500
        with pytest.raises(pkg.GalSynthError):
            eng.run_host(bad)
        bad = p.copy()
        bad["f_code"][1, 0] = 1.31e6  # more than half a chip per sample: outside the half-chip window
        with pytest.raises(pkg.GalSynthError):
            eng.run_host(bad)
        bad = p.copy()
        bad["code_phase0"][1, 1] = 8183.9  # a pending wrap followed by a second one within a few samples
        with pytest.raises(pkg.GalSynthError):
            eng.run_host(bad)


def _hard_batch(pkg, monkeypatch):
    """A batch whose carrier chain is NOT complete after one walk + stitch (some legs have to be walked again).  Since round 6's first
    guesses follow the phase through Doppler sign changes no random small batch is (tools/find_multi_pass_batch.py: 0 of 3000; rounds
    1-5 took case 35 of the fuzz generator's seed 5, a sign-flipping one), so the fault-injection build spoils ONE guess
    (GAL_GUESS_SPOIL: the first pass anchors leg 5 of slot 0 one sample late): the stitch re-anchors it at the true event and a second
    pass walks it again.  Engines must be made with test_hooks=True."""
    from fuzz_cases import random_case

    hard, n_samp, rate, chunk = random_case(pkg, np.random.default_rng([5, 35]), False)
    assert (rate, n_samp, chunk, hard.shape) == (2.6e6, 260000, 1360, (3, 8))
    monkeypatch.setenv("GAL_GUESS_SPOIL", "1")
    return hard, n_samp, rate, chunk


def test_unconverged_speculation_is_repaired(pkg, monkeypatch):
    """With a single enqueued walker pass a batch that needs two is not verified in time: gal_synth_finish() must
    iterate from the host and redo the synthesis -- the result is still bit-exact.  (An ordinary batch is complete after
    ONE pass: the stitch translates re-anchored legs on the spot.)"""
    hard, n_samp, rate, chunk = _hard_batch(pkg, monkeypatch)
    monkeypatch.setenv("GAL_WALK_PASSES", "1")  # honoured by the GAL_TEST_HOOKS build only
    iq, st, stats = _compare(pkg, hard, n_samp, rate=rate, chunk_samples=chunk, test_hooks=True)
    assert stats["walk_passes"] >= 2 and stats["synth_runs"] == 2
    iq, st, stats = _compare(pkg, hard, n_samp, rate=rate, test_hooks=True)  # ... and on the default kernel of this geometry
    assert stats["walk_passes"] >= 2 and stats["synth_runs"] == 2 and stats["kernel_family"] == 1
    monkeypatch.delenv("GAL_WALK_PASSES")
    iq, st, stats = _compare(pkg, hard, n_samp, rate=rate, chunk_samples=chunk, test_hooks=True)
    assert stats["walk_passes"] >= 2 and stats["synth_runs"] == 1
    monkeypatch.delenv("GAL_GUESS_SPOIL")
    iq, st, stats = _compare(pkg, hard, n_samp, rate=rate, chunk_samples=chunk, test_hooks=True)
    assert stats["walk_passes"] == 1 and stats["synth_runs"] == 1  # the batch as it is: one pass (rounds 1-5: two)
    p = pkg.workloads.make_synthetic(n_epochs=5, n_chan=7, n_slots=16, samples_per_epoch=52000, seed=77)
    monkeypatch.setenv("GAL_WALK_PASSES", "1")
    iq, st, stats = _compare(pkg, p, 52000, test_hooks=True)
    assert stats["walk_passes"] == 1 and stats["synth_runs"] == 1


def test_enqueued_carrier_passes_belong_to_the_plan(pkg, monkeypatch):
    """A NEW plan of more than 32 epochs gets three carrier passes enqueued up front (a batch that needs more than were enqueued pays a
    second synthesis: a scenario in which a satellite's Doppler passes through zero, one in eight of the random M-SYN12 seeds, needs
    two); a plan that is EXECUTED AGAIN enqueues what its last execute needed.  Rounds 3-5 kept the count per handle ("one after a
    batch that got by with one"): right for a bench that re-executes one resident plan, wrong for a caller with new parameters every
    batch -- a hard batch behind an easy one was repaired by a second synthesis (synth_runs == 2).  Now it never is.  Plans of a few
    epochs (one-epoch calls: all latency, every spare pass is two launches in front of the synthesis) keep the per-handle count."""
    import torch

    n = 52000
    big = pkg.workloads.make_synthetic(n_epochs=40, n_chan=6, n_slots=8, samples_per_epoch=n, seed=12)
    ref_big, _ = oracle_run(big, n, 2.6e6)
    with pkg.SynthEngine(samples_per_epoch=n, n_slots=8, device=0, test_hooks=True) as eng:
        for spoil in (True, False, True, True, False):  # (GAL_GUESS_SPOIL, read when the batch is planned: one leg walked again in pass two)
            if spoil:
                monkeypatch.setenv("GAL_GUESS_SPOIL", "1")
            else:
                monkeypatch.delenv("GAL_GUESS_SPOIL", raising=False)
            iq, _, stats = eng.run_host(big)
            assert np.array_equal(iq, ref_big) and stats["synth_runs"] == 1, (spoil, stats)
            assert (stats["walk_passes"] >= 2) if spoil else (stats["walk_passes"] == 1)
        # the same plan executed again and again: same passes, one synthesis each
        monkeypatch.setenv("GAL_GUESS_SPOIL", "1")
        eng.plan(big)
        out = torch.empty(ref_big.size, dtype=torch.int16, device="cuda")
        for _ in range(3):
            eng.execute(out.data_ptr())
            _, stats = eng.finish()
            assert stats["walk_passes"] >= 2 and stats["synth_runs"] == 1
            assert np.array_equal(out.cpu().numpy(), ref_big)
    # small plans: the handle's first enqueues two, then what its last small batch needed
    hard, n_samp, rate, chunk = _hard_batch(pkg, monkeypatch)
    ref_hard, _ = oracle_run(hard, n_samp, rate)
    with pkg.SynthEngine(sample_rate=rate, samples_per_epoch=n_samp, n_slots=8, device=0, chunk_samples=chunk, test_hooks=True) as eng:
        runs = []
        for spoil in (True, False, True, True):
            if spoil:
                monkeypatch.setenv("GAL_GUESS_SPOIL", "1")
            else:
                monkeypatch.delenv("GAL_GUESS_SPOIL", raising=False)
            iq, _, stats = eng.run_host(hard)
            assert np.array_equal(iq, ref_hard)
            runs.append((stats["walk_passes"] >= 2, stats["synth_runs"]))
        assert runs == [(True, 1), (False, 1), (True, 2), (True, 1)]  # (one enqueued behind the easy batch: repaired, then two again)


def test_translated_legs_on_moving_receiver(pkg):
    """M-DYN-like Doppler (changes every epoch): most second-pass legs are accepted by translation, a few
    are walked again, and the replay check never has to force the all-walked fallback."""
    p = pkg.workloads.make_synthetic(n_epochs=40, n_chan=12, n_slots=16, samples_per_epoch=260000, seed=4242,
                                     dyn_track=True)
    # sprinkle tie-prone steps (multiples of 2^-52 / 2^-53 cycles per sample): never translated
    for e, j, k in [(5, 0, 52), (9, 3, 53), (17, 7, 52), (30, 11, 50)]:
        d = p["f_carr"][e, j] / 2.6e6
        p["f_carr"][e, j] = np.round(d * 2.0 ** k) / 2.0 ** k * 2.6e6
        p["f_code"][e, j] = 1.023e6 + p["f_carr"][e, j] * 0.0006493506493506494
    with pkg.SynthEngine(samples_per_epoch=260000, n_slots=16, device=0) as eng:
        iq, st, stats = eng.run_host(p)
        walked, translated, fallbacks = eng.walk_counts()
    ref_iq, ref_st = oracle_run(p, 260000, 2.6e6)
    assert np.array_equal(iq, ref_iq)
    assert stats["chain_mismatch"] == 0 and fallbacks == 0
    legs = 40 * 32 * 12  # (a batch of up to 256 epochs: 32 carrier legs per epoch)
    assert translated > legs // 2 and walked < legs + legs // 4, (walked, translated)


def test_full_size_properties(pkg):
    """BASELINE configs[1] size (M-SYN12: 1199 epochs x 260000 samples x 12 SVs = 1.247 GB of IQ):
      * EVERY epoch equals the oracle, int16 by int16, and so does the end state (8 s of CPU on the GPU box's host);
      * chunking / leg layout must not matter: automatic chunking, 1024 and 520 give the same bytes;
      * a run split in two calls with the carried state equals the single run (gal_chan_state_t contract);
      * the chain self-check is clean; no leg is walked twice."""
    import torch

    n, rate = 260000, 2.6e6
    p = pkg.workloads.m_syn12()
    E = p.shape[0]
    outs = []
    for chunk in (0, 1024, 520):
        with pkg.SynthEngine(samples_per_epoch=n, n_slots=16, device=0, chunk_samples=chunk) as eng:
            eng.plan(p)
            out = torch.empty(eng.output_bytes() // 2, dtype=torch.int16, device="cuda")
            eng.execute(out.data_ptr())
            st, stats = eng.finish()
            assert stats["chain_mismatch"] == 0
            if chunk == 0:
                walked, translated, fallbacks = eng.walk_counts()
                assert fallbacks == 0 and walked <= E * 8 * 12 + 64, (walked, translated)
                state_full = st
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    bad, ref_end = oracle_matches_device(outs[0], p, n, rate)
    assert bad == 0, "%d int16 values of the full-size output differ from the oracle" % bad
    act0 = state_full["prn"] > 0
    assert np.array_equal(ref_end["carr_phase"][act0].view(np.uint64), state_full["carr_phase"][act0].view(np.uint64))
    del outs[1:]
    # split run: 700 + 499 epochs
    with pkg.SynthEngine(samples_per_epoch=n, n_slots=16, device=0) as eng:
        eng.plan(p[:700])
        a = torch.empty(eng.output_bytes() // 2, dtype=torch.int16, device="cuda")
        eng.execute(a.data_ptr())
        st_a, _ = eng.finish()
        q = p[700:].copy()
        q["flags"][0, :12] = 0  # continues from the carried state
        eng.plan(q, st_a)
        b = torch.empty(eng.output_bytes() // 2, dtype=torch.int16, device="cuda")
        eng.execute(b.data_ptr())
        st_b, _ = eng.finish()
        # state at epoch 1195 from a third plan, so that the oracle can replay the LAST 4 epochs on its own
        eng.plan(q[:495], st_a)
        c = torch.empty(eng.output_bytes() // 2, dtype=torch.int16, device="cuda")
        eng.execute(c.data_ptr())
        st_c, _ = eng.finish()
    assert torch.equal(outs[0][: a.numel()], a) and torch.equal(outs[0][a.numel():], b)
    act = state_full["prn"] > 0
    assert np.array_equal(st_b["carr_phase"][act].view(np.uint64), state_full["carr_phase"][act].view(np.uint64))
    assert np.array_equal(st_b["page"][act], state_full["page"][act])
    tail = p[1195:].copy()
    tail["flags"][0, :12] = 0
    ref_tail, ref_st = oracle_run(tail, n, rate, st_c)
    assert np.array_equal(outs[0][1195 * n * 2:].cpu().numpy(), ref_tail)
    assert np.array_equal(ref_st["carr_phase"][act].view(np.uint64), state_full["carr_phase"][act].view(np.uint64))


def _dev_equal(a, b, piece=1 << 30):
    """torch.equal in pieces (the comparison mask of a 60 GB pair would be another 30 GB)."""
    import torch

    if a.numel() != b.numel():
        return False
    return all(torch.equal(a[o:o + piece], b[o:o + piece]) for o in range(0, a.numel(), piece))


def test_m_syn24_full_size_properties(pkg):
    """BASELINE config 4 at FULL size (M-SYN24: 5999 epochs x 2 500 000 samples x 24 SVs @25 MS/s = 15.0 G samples,
    60 GB of IQ per run, sample indices beyond 2^32 bytes and 2^32 int16 elements):
      * EVERY epoch equals the oracle (round 6: 64 slices on the host's cores, states chained by induction -- see
        _every_epoch_against_the_oracle_in_slices); the first 2 and the LAST 2 epochs once more on their own;
      * chunk 0 (default) and 2048 give the same 60 GB;
      * a run split 3000 + 2999 with the carried state equals the single run, end state included;
      * the chain self-check is clean, the all-walked fallback is never needed, the synthesis ran once per batch."""
    import torch

    n, rate, S = 2500000, 25e6, 24
    free, _total = torch.cuda.mem_get_info()
    if free < 200e9:
        pytest.skip("needs 200 GB of free HBM (two 60 GB outputs plus the split runs)")
    p = pkg.workloads.m_syn24()
    E = p.shape[0]
    assert E == 5999
    outs = []
    for chunk in (0, 2048):
        with pkg.SynthEngine(sample_rate=rate, samples_per_epoch=n, n_slots=S, device=0, chunk_samples=chunk) as eng:
            eng.plan(p)
            assert eng.output_bytes() == E * n * 4 > 2 ** 35
            out = torch.empty(eng.output_bytes() // 2, dtype=torch.int16, device="cuda")
            eng.execute(out.data_ptr())
            st, stats = eng.finish()
            assert stats["chain_mismatch"] == 0 and stats["n_active_max"] == 24 and stats["synth_runs"] == 1
            assert eng.walk_counts()[2] == 0
            if chunk == 0:
                state_full = st
        outs.append(out)
    assert _dev_equal(outs[0], outs[1])
    del outs[1:], out
    torch.cuda.empty_cache()
    full = outs[0]
    ref_iq, _ = oracle_run(p[:2], n, rate)
    assert np.array_equal(full[: 2 * n * 2].cpu().numpy(), ref_iq)
    with pkg.SynthEngine(sample_rate=rate, samples_per_epoch=n, n_slots=S, device=0) as eng:
        eng.plan(p[:3000])
        a = torch.empty(eng.output_bytes() // 2, dtype=torch.int16, device="cuda")
        eng.execute(a.data_ptr())
        st_a, stats_a = eng.finish()
        assert stats_a["chain_mismatch"] == 0
        assert _dev_equal(full[: a.numel()], a)
        q = p[3000:].copy()
        q["flags"][0, :] = 0  # continues from the carried state
        eng.plan(q, st_a)
        eng.execute(a.data_ptr())  # 2999 epochs into the 3000-epoch buffer
        st_b, stats_b = eng.finish()
        assert stats_b["chain_mismatch"] == 0
        assert _dev_equal(full[3000 * n * 2:], a[: 2999 * n * 2])
        # state at epoch 5997 from a third plan, so that the oracle can replay the last 2 epochs on its own
        eng.plan(q[:2997], st_a)
        eng.execute(a.data_ptr())
        st_c, _ = eng.finish()
    act = state_full["prn"] > 0
    assert act.sum() == 24
    assert np.array_equal(st_b["carr_phase"][act].view(np.uint64), state_full["carr_phase"][act].view(np.uint64))
    assert np.array_equal(st_b["page"][act], state_full["page"][act])
    tail = p[5997:].copy()
    tail["flags"][0, :] = 0
    ref_tail, ref_st = oracle_run(tail, n, rate, st_c)
    assert np.array_equal(full[5997 * n * 2:].cpu().numpy(), ref_tail)
    assert np.array_equal(ref_st["carr_phase"][act].view(np.uint64), state_full["carr_phase"][act].view(np.uint64))
    del a
    torch.cuda.empty_cache()
    _every_epoch_against_the_oracle_in_slices(pkg, p, full, n, rate, S, state_full)


def _every_epoch_against_the_oracle_in_slices(pkg, p, full, n, rate, S, state_full, n_slices=64):
    """EVERY epoch of config 4 (15 G samples x 24 channels, ~11 CPU-minutes of the oracle) against the oracle, on the
    host's cores: the 5999 epochs are cut into 64 slices; slice k's start state is the END state gal_synth_execute_range returns for
    slice k - 1 (the engine walks the prefix silently); every slice runs through oracle_run on its own thread (ctypes releases the
    GIL), in pieces of 4 epochs with the oracle's own state carried, and must give (a) the samples of the single 60 GB run, int16 by
    int16, and (b) an end state BITWISE equal to the start state the next slice was given.  (b) closes the induction: slice 0 starts
    from the records' own restart, so every state the slices start from is the oracle's own -- the 64 threads together ARE the
    sequential oracle run over all 5999 epochs (src/galileo-sdr.cpp:481-539)."""
    import os
    from concurrent.futures import ThreadPoolExecutor

    import torch

    E = p.shape[0]
    per = n * 2
    bounds = [round(k * E / n_slices) for k in range(n_slices + 1)]
    starts = [None]  # start state of every slice, from the engine
    with pkg.SynthEngine(sample_rate=rate, samples_per_epoch=n, n_slots=S, device=0) as eng:
        eng.plan(p)
        scratch = torch.empty(max(b - a for a, b in zip(bounds[:-1], bounds[1:])) * per, dtype=torch.int16, device="cuda")
        for k in range(n_slices):
            a, b = bounds[k], bounds[k + 1]
            eng.execute(scratch.data_ptr(), a, b - a)
            st, stats = eng.finish()
            assert stats["chain_mismatch"] == 0 and eng.walk_counts()[2] == 0
            assert _dev_equal(full[a * per:b * per], scratch[: (b - a) * per]), k  # the range alone = its part of the single run
            starts.append(st)
        del scratch
    act = state_full["prn"] > 0
    assert np.array_equal(starts[-1]["carr_phase"][act].view(np.uint64), state_full["carr_phase"][act].view(np.uint64))

    def run_slice(k):
        a, b = bounds[k], bounds[k + 1]
        st, bad = starts[k], 0
        for c in range(a, b, 4):
            d = min(c + 4, b)
            ref, st = oracle_run(p[c:d], n, rate, state_in=st)
            bad += int(np.count_nonzero(full[c * per:d * per].cpu().numpy() != ref))
        nxt = starts[k + 1]
        on = nxt["prn"] > 0
        state_ok = (np.array_equal(st["carr_phase"][on].view(np.uint64), nxt["carr_phase"][on].view(np.uint64))
                    and np.array_equal(st["page"][on], nxt["page"][on]) and np.array_equal(st["prn"], nxt["prn"]))
        return bad, state_ok

    with ThreadPoolExecutor(min(os.cpu_count() or 1, n_slices)) as ex:
        res = list(ex.map(run_slice, range(n_slices)))
    assert sum(r[0] for r in res) == 0, [k for k, r in enumerate(res) if r[0]]
    assert all(r[1] for r in res), [k for k, r in enumerate(res) if not r[1]]


def test_replay_check_catches_a_wrong_translation(pkg, monkeypatch):
    """Safety net of the translated acceptance, BOTH chains: a leg shifted by the wrong amount (test hooks: GAL_WALK_TRANSLATE=2 a
    carrier leg, =3 a code leg) must be caught IN THE BATCH IT HAPPENS IN -- by k_verify_carr / k_verify_code on the default kernel
    (every leg of both chains in every batch: the default since round 6), by k_synth's replay check with GAL_CFG_EXACT_REPLAY;
    gal_synth_finish then redoes both chains with every leg walked and repeats the synthesis -- the caller still gets bit-exact IQ,
    and the fallback is counted.  GAL_CFG_VERIFY_SAMPLED (opt-in): the leg's turn in the rotation comes within eight batches."""
    p = pkg.workloads.make_synthetic(n_epochs=6, n_chan=4, n_slots=8, samples_per_epoch=260000, seed=99)
    ref_iq, ref_st = oracle_run(p, 260000, 2.6e6)
    act = ref_st["prn"] > 0
    for hook in ("2", "3"):
        monkeypatch.setenv("GAL_WALK_TRANSLATE", hook)  # honoured by the GAL_TEST_HOOKS build only
        for flags in (0, pkg.synth.GAL_CFG_VERIFY_ALL, pkg.synth.GAL_CFG_EXACT_REPLAY):
            with pkg.SynthEngine(samples_per_epoch=260000, n_slots=8, device=0, test_hooks=True, flags=flags) as eng:
                assert b"testhooks" in eng._lib.gal_synth_version()
                iq, st, stats = eng.run_host(p)
                walked, translated, fallbacks = eng.walk_counts()
            assert fallbacks == 1 and stats["chain_mismatch"] == 0, (hook, flags)
            assert np.array_equal(iq, ref_iq), (hook, flags)
            assert np.array_equal(st["carr_phase"][act].view(np.uint64), ref_st["carr_phase"][act].view(np.uint64))
        # the sampled mode: an eighth of the leg positions per batch, rotating -- the bad leg is caught when its turn comes, the
        # output of the batches before that is wrong in the leg's chunks (what the rotation trades for ~4 % of a step)
        with pkg.SynthEngine(samples_per_epoch=260000, n_slots=8, device=0, test_hooks=True,
                             flags=pkg.synth.GAL_CFG_VERIFY_SAMPLED) as eng:
            n_caught = 0
            for _ in range(8):
                before = eng.walk_counts()[2]
                iq, st, stats = eng.run_host(p)
                assert stats["chain_mismatch"] == 0
                if eng.walk_counts()[2] > before:  # this batch's rotation looked at the leg: repaired, exact
                    n_caught += 1
                    assert np.array_equal(iq, ref_iq)
                    assert np.array_equal(st["carr_phase"][act].view(np.uint64), ref_st["carr_phase"][act].view(np.uint64))
            # (the leg's own turn, and its predecessor's, whose hand-over lands on its first checkpoint; k_repair_g's chunk walks may
            # add a catch of their own)
            assert 1 <= n_caught <= 3, (hook, n_caught)
    monkeypatch.setenv("GAL_WALK_TRANSLATE", "0")  # and the all-walked mode on its own
    _compare(pkg, p, 260000, test_hooks=True)
    # the product library has no such hook: the same environment leaves it on the normal path
    # (GAL_SYNTH_LIB: an A/B run that loads another build in the product's place -- the NaN-poisoned run of the suite loads the hooks build)
    for hook in ("2", "3") if not os.environ.get("GAL_SYNTH_LIB") else ():
        monkeypatch.setenv("GAL_WALK_TRANSLATE", hook)
        with pkg.SynthEngine(samples_per_epoch=260000, n_slots=8, device=0) as eng:
            assert b"testhooks" not in eng._lib.gal_synth_version()
            iq2, _, _ = eng.run_host(p)
            assert eng.walk_counts()[2] == 0
        assert np.array_equal(iq2, ref_iq)


def test_plan_async_with_fresh_parameters_every_batch(pkg):
    """gal_synth_plan_async (round 6): the plan returns with its upload enqueued, the next execute's walkers wait for it on the device.
    Two handles, a NEW scenario for every batch (other seed, other channel count, a state carried into some), planned on the handle
    that has just been finished while the other one's batch runs: every batch bit-exact, end states included; the staging buffer is
    reused only after its upload has left it (plans back to back on one handle)."""
    import torch

    n = 52000
    sets = [pkg.workloads.make_synthetic(n_epochs=6 + (k % 5) * 7, n_chan=3 + (k * 5) % 12, n_slots=16, samples_per_epoch=n, seed=900 + k)
            for k in range(9)]
    refs = [oracle_run(q, n, 2.6e6) for q in sets]
    engines = [pkg.SynthEngine(samples_per_epoch=n, n_slots=16, device=0) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = [torch.empty(max(q.shape[0] for q in sets) * n * 2, dtype=torch.int16, device="cuda") for _ in range(2)]
    for e, st in zip(engines, streams):
        e.set_stream(st.cuda_stream)
    pending = [None, None]

    def reap(j):
        k = pending[j]
        st, stats = engines[j].finish()
        ref_iq, ref_st = refs[k]
        assert stats["chain_mismatch"] == 0 and stats["ms_plan"] > 0 and stats["ms_h2d"] > 0
        assert np.array_equal(outs[j][: ref_iq.size].cpu().numpy(), ref_iq), k
        act = ref_st["prn"] > 0
        assert np.array_equal(st["carr_phase"][act].view(np.uint64), ref_st["carr_phase"][act].view(np.uint64))
        pending[j] = None

    for rep in range(3):
        for k in range(len(sets)):
            j = k % 2
            if pending[j] is not None:
                reap(j)
            if k == 4:  # two plans back to back on one handle: the second must wait for the first upload to leave the staging buffer
                engines[j].plan(sets[0], wait=False)
            engines[j].plan(sets[k], wait=False)
            engines[j].execute(outs[j].data_ptr())
            pending[j] = k
    for j in range(2):
        if pending[j] is not None:
            reap(j)
    # a carried state through the asynchronous plan: a scenario split in two, the second half planned without waiting
    q = sets[4]
    half = q.shape[0] // 2
    engines[0].plan(q[:half], wait=False)
    engines[0].execute(outs[0].data_ptr())
    st_a, _ = engines[0].finish()
    a = outs[0][: half * n * 2].cpu().numpy()
    engines[0].plan(q[half:], st_a, wait=False)
    engines[0].execute(outs[0].data_ptr())
    st_b, _ = engines[0].finish()
    b = outs[0][: (q.shape[0] - half) * n * 2].cpu().numpy()
    assert np.array_equal(np.concatenate([a, b]), refs[4][0])
    for e in engines:
        e.close()


def test_plan_async_while_the_batch_before_is_in_flight(pkg):
    """plan(k+1) under execute(k) on ONE handle (round 6): gal_synth_plan_async with a batch in flight stages the next plan on the host
    only -- the arena, the device plan and everything gal_synth_finish reports still belong to the batch in flight --; the next
    gal_synth_execute (behind that batch's finish) commits it: upload enqueued, walkers behind it.  Two handles, one thread, a new
    scenario every step (other sizes, other channel counts, a bigger one that makes the arena grow at the commit): every batch
    bit-exact, the statistics those of the batch that ran.  The synchronous gal_synth_plan with a batch in flight stays an error, and
    so does an execute in front of the finish."""
    import torch

    n = 52000
    sets = [pkg.workloads.make_synthetic(n_epochs=5 + (k * 7) % 23, n_chan=2 + (k * 5) % 13, n_slots=16, samples_per_epoch=n, seed=1500 + k)
            for k in range(11)]
    refs = [oracle_run(q, n, 2.6e6) for q in sets]
    engines = [pkg.SynthEngine(samples_per_epoch=n, n_slots=16, device=0) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = [torch.empty(max(q.shape[0] for q in sets) * n * 2, dtype=torch.int16, device="cuda") for _ in range(2)]
    for e, st in zip(engines, streams):
        e.set_stream(st.cuda_stream)
    running, staged = [None, None], [None, None]

    def reap(j):
        k = running[j]
        st, stats = engines[j].finish()
        ref_iq, ref_st = refs[k]
        assert stats["chain_mismatch"] == 0 and stats["n_epochs"] == sets[k].shape[0], k  # (of the batch that ran, not of the staged plan)
        assert stats["n_active_max"] == int((sets[k]["prn"] > 0).sum(axis=1).max())
        assert np.array_equal(outs[j][: ref_iq.size].cpu().numpy(), ref_iq), k
        act = ref_st["prn"] > 0
        assert np.array_equal(st["carr_phase"][act].view(np.uint64), ref_st["carr_phase"][act].view(np.uint64))
        running[j] = None

    order = list(range(len(sets))) * 2
    for step, k in enumerate(order):
        j = step % 2
        if running[j] is not None:
            with pytest.raises(pkg.GalSynthError):  # a batch in flight and a plan staged: execute must wait for the finish
                engines[j].execute(outs[j].data_ptr())
            reap(j)
        if staged[j] is None:
            engines[j].plan(sets[k], wait=False)
            staged[j] = k
        assert engines[j].output_bytes() == sets[staged[j]].shape[0] * n * 4
        engines[j].execute(outs[j].data_ptr())  # commits the staged plan
        running[j], staged[j] = staged[j], None
        if step + 2 < len(order):
            nxt = order[step + 2]
            with pytest.raises(pkg.GalSynthError):
                engines[j].plan(sets[nxt])  # the synchronous plan needs the handle idle
            engines[j].plan(sets[nxt], wait=False)  # ... the asynchronous one stages beside the batch in flight
            staged[j] = nxt
            assert engines[j].output_bytes() == sets[nxt].shape[0] * n * 4
    for j in range(2):
        if running[j] is not None:
            reap(j)
    # a staged plan that is replaced before it ever ran, and one that is dropped by a synchronous plan after the finish
    engines[0].plan(sets[0], wait=False)
    engines[0].execute(outs[0].data_ptr())
    engines[0].plan(sets[1], wait=False)
    engines[0].plan(sets[2], wait=False)  # replaces the staged plan of set 1
    running[0] = 0
    reap(0)
    engines[0].execute(outs[0].data_ptr())
    running[0] = 2
    engines[0].plan(sets[3], wait=False)
    reap(0)
    engines[0].plan(sets[4])  # synchronous: takes the place of the staged plan of set 3
    engines[0].execute(outs[0].data_ptr())
    running[0] = 4
    reap(0)
    for e in engines:
        e.close()


def test_ranges_of_one_plan_keep_the_stitch_records_apart(pkg, monkeypatch):
    """the stitch's look-back records (k_scanm) were laid out from the RANGE-CUT leg count, so executing ranges of
    different lengths on one plan moved the status words over former payload words (claim kinds 0..2, fold flags 0..7) that
    nobody clears and that can equal a young handle's small tags.  Now they are laid out from the plan: any sequence of ranges,
    on young handles (tags 1, 2, 3 ...), with many blocks per slot, must stay bit-exact and never need the fallback; and the
    32-bit tag's wrap (hook: a handle that starts just below it) clears the status words and goes on."""
    import torch

    n = 26000
    p = pkg.workloads.make_synthetic(n_epochs=40, n_chan=9, n_slots=16, samples_per_epoch=n, seed=606)
    ref_iq, _ = oracle_run(p, n, 2.6e6)
    seqs = [((0, 40), (0, 20), (0, 40), (0, 8), (0, 33), (0, 40)), ((0, 20), (0, 40), (0, 12), (0, 40)),
            ((5, 35), (0, 9), (10, 30), (0, 40))]
    for lpb, tag0 in ((None, None), ("8", None), ("3", None), (None, "0xFFF00000"), ("8", "0xFFEFFFFD")):
        if lpb:
            monkeypatch.setenv("GAL_SCAN_BLOCK_LEGS", lpb)
        else:
            monkeypatch.delenv("GAL_SCAN_BLOCK_LEGS", raising=False)
        if tag0:
            monkeypatch.setenv("GAL_SCAN_TAG0", tag0)
        else:
            monkeypatch.delenv("GAL_SCAN_TAG0", raising=False)
        for seq in seqs:
            with pkg.SynthEngine(samples_per_epoch=n, n_slots=16, device=0, test_hooks=bool(lpb or tag0)) as eng:
                eng.plan(p)
                for e0, ne in seq:
                    out = torch.empty(ne * n * 2, dtype=torch.int16, device="cuda")
                    eng.execute(out.data_ptr(), e0, ne)
                    st, stats = eng.finish()
                    assert stats["chain_mismatch"] == 0 and eng.walk_counts()[2] == 0, (lpb, tag0, seq, e0, ne)
                    assert np.array_equal(out.cpu().numpy(), ref_iq[e0 * n * 2:(e0 + ne) * n * 2]), (lpb, tag0, seq, e0, ne)


def test_range_execute_never_rests_on_an_unreplayed_translation(pkg, monkeypatch):
    """gal_synth_execute_range replays (and therefore checks) only its own epochs, so a translated leg in front of
    the range could not be caught by k_synth's self-check: such legs must be walked, never translated.  The test
    hook would corrupt the translation of (slot 0, epoch 0, leg 5); a range that starts after epoch 0 must come
    out bit-exact WITHOUT needing the fallback, and the state at the end of the range must be exact too."""
    import torch

    n = 260000
    p = pkg.workloads.make_synthetic(n_epochs=6, n_chan=4, n_slots=8, samples_per_epoch=n, seed=99)
    ref_iq, ref_st = oracle_run(p, n, 2.6e6)
    monkeypatch.setenv("GAL_WALK_TRANSLATE", "2")
    with pkg.SynthEngine(samples_per_epoch=n, n_slots=8, device=0, test_hooks=True) as eng:  # (default: every leg verified)
        eng.plan(p)
        for e0, ne in ((2, 3), (1, 5), (5, 1)):
            out = torch.empty(ne * n * 2, dtype=torch.int16, device="cuda")
            eng.execute(out.data_ptr(), e0, ne)
            st, stats = eng.finish()
            assert stats["chain_mismatch"] == 0 and eng.walk_counts()[2] == 0
            assert np.array_equal(out.cpu().numpy(), ref_iq[e0 * n * 2:(e0 + ne) * n * 2]), (e0, ne)
            _, end_st = oracle_run(p[: e0 + ne], n, 2.6e6)  # finish() returns the state at the end of the RANGE
            act = end_st["prn"] > 0
            assert np.array_equal(st["carr_phase"][act].view(np.uint64), end_st["carr_phase"][act].view(np.uint64))
            assert np.array_equal(st["page"][act], end_st["page"][act])
        # a range that contains the bad leg is replayed, caught and repaired
        out = torch.empty(2 * n * 2, dtype=torch.int16, device="cuda")
        eng.execute(out.data_ptr(), 0, 2)
        eng.finish()
        assert eng.walk_counts()[2] == 1
        assert np.array_equal(out.cpu().numpy(), ref_iq[: 2 * n * 2])


def test_randomised_soak(pkg):
    """A slice of the randomised soak (tests/fuzz_cases.py, driven at length by tools/fuzz_parity.py: random shapes,
    rates, chunkings, Doppler patterns, channels coming and going): every case bit-exact, the all-walked fallback never needed.  The tool itself was run over 6000
    small and 360 reference-geometry cases at the end of round 1."""
    from fuzz_cases import random_case

    rng = np.random.default_rng(2024)
    for c in range(80):
        p, n_samp, rate, chunk = random_case(pkg, rng, big=(c % 20 == 19))
        with pkg.SynthEngine(sample_rate=rate, samples_per_epoch=n_samp, n_slots=p.shape[1], device=0,
                             chunk_samples=chunk) as eng:
            iq, st, stats = eng.run_host(p)
            assert eng.walk_counts()[2] == 0
        ref_iq, ref_st = oracle_run(p, n_samp, rate)
        assert np.array_equal(iq, ref_iq) and stats["chain_mismatch"] == 0, (c, rate, p.shape, n_samp, chunk)
        act = ref_st["prn"] > 0
        assert np.array_equal(st["carr_phase"][act].view(np.uint64), ref_st["carr_phase"][act].view(np.uint64))
        assert np.array_equal(st["page"][act], ref_st["page"][act])


def test_batch_without_any_channel(pkg):
    """All slots idle for a whole batch (found by tools/fuzz_parity.py with split runs): zeros, as the reference's
    loop stores when no channel has a PRN (src/galileo-sdr.cpp:489,536-537); also as the tail of a split run."""
    p = pkg.workloads.make_synthetic(n_epochs=4, n_chan=2, n_slots=8, samples_per_epoch=20000, seed=17)
    p[2:] = np.zeros((), dtype=p.dtype)
    iq, st, stats = _compare(pkg, p, 20000)
    assert not iq[2 * 20000 * 2:].any()
    with pkg.SynthEngine(samples_per_epoch=20000, n_slots=8, device=0) as eng:
        iq1, st1, _ = eng.run_host(p[:2])
        iq2, st2, _ = eng.run_host(p[2:], st1)
    assert not iq2.any() and not (st2["prn"] > 0).any()
    assert np.array_equal(np.concatenate([iq1, iq2]), iq)


def test_epoch_ranges_of_one_plan(pkg):
    """gal_synth_execute_range: one scenario cut into contiguous epoch ranges (how it shards over GPUs, bench.py
    --shard scenario): each range synthesised on its own equals the corresponding slice of the full output; the
    walker covers the epochs up to the end of the range (those in front of it silently), so a range that starts mid-run
    gets the exact carrier state, and finish() returns the state at the end of the range: the next range, planned on its
    own from that state, continues bit-exactly."""
    import torch

    n = 52000
    p = pkg.workloads.make_synthetic(n_epochs=11, n_chan=14, n_slots=16, samples_per_epoch=n, seed=4321)  # 2 groups
    ref_iq, _ = oracle_run(p, n, 2.6e6)
    with pkg.SynthEngine(samples_per_epoch=n, n_slots=16, device=0) as eng:
        eng.plan(p)
        for world in (1, 2, 3, 4):
            parts = []
            for r in range(world):
                e0, ne = pkg.shard.epoch_range(r, world, p.shape[0])
                out = torch.empty(ne * n * 2, dtype=torch.int16, device="cuda")
                eng.execute(out.data_ptr(), e0, ne)
                st, stats = eng.finish()
                assert stats["chain_mismatch"] == 0
                parts.append(out.cpu().numpy())
                walked = eng.walk_counts()[0]
                # legs of the prefix, not of the plan (legs in front of the range are never translated: those whose anchor moved
                # are walked a second time)
                legs = 32 if p.shape[0] <= 256 else 16 if p.shape[0] <= 512 else 8  # gal_synth_plan: shorter legs for batches that do not fill the chip
                assert walked <= 2 * (e0 + ne) * legs * 14 + 64, (walked, e0, ne)
            assert np.array_equal(np.concatenate(parts), ref_iq), world
        # the state finish() returns is the one at the end of the range: a fresh plan of the remaining epochs continues from it
        out = torch.empty(4 * n * 2, dtype=torch.int16, device="cuda")
        eng.execute(out.data_ptr(), 3, 4)
        st_mid, _ = eng.finish()
        q = p[7:].copy()
        q["flags"][0, :] = 0
        rest, _, _ = eng.run_host(q, st_mid)
        assert np.array_equal(rest, ref_iq[7 * n * 2:])
        eng.plan(p)
        with pytest.raises(pkg.GalSynthError):
            eng.execute(out.data_ptr(), 10, 2)


def test_call_sequence_is_checked(pkg):
    """plan / execute while a batch is in flight would race with the kernels still reading the plan: GAL_E_STATE."""
    import torch

    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=3, n_slots=8, samples_per_epoch=20000, seed=5)
    with pkg.SynthEngine(samples_per_epoch=20000, n_slots=8, device=0) as eng:
        with pytest.raises(pkg.GalSynthError):
            eng.finish()
        eng.plan(p)
        out = torch.empty(eng.output_bytes() // 2, dtype=torch.int16, device="cuda")
        eng.execute(out.data_ptr())
        with pytest.raises(pkg.GalSynthError):
            eng.execute(out.data_ptr())
        with pytest.raises(pkg.GalSynthError):
            eng.plan(p)
        st, stats = eng.finish()
        eng.execute(out.data_ptr())  # the same plan again
        eng.finish()
        ref_iq, _ = oracle_run(p, 20000, 2.6e6)
        assert np.array_equal(out.cpu().numpy(), ref_iq)


def test_completion_record_belongs_to_the_batch(pkg):
    """gal_synth_finish polls the record the device writes into pinned host memory behind k_synth (counters, end state,
    sequence number).  Different plans one after the other on ONE handle: every finish must return the state and the
    statistics of ITS batch (a stale record would hand out the previous batch's), also when the caller has queued work of
    its own behind execute() on the same stream -- finish waits for the batch, not for the stream -- and when execute is
    repeated for an unchanged plan."""
    import torch

    n = 26000
    st = torch.cuda.Stream()
    filler = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
    with pkg.SynthEngine(samples_per_epoch=n, n_slots=8, device=0) as eng:
        eng.set_stream(st.cuda_stream)
        for k in range(6):
            n_ep = 2 + (k % 3)
            p = pkg.workloads.make_synthetic(n_epochs=n_ep, n_chan=2 + k, n_slots=8, samples_per_epoch=n, seed=900 + k)
            eng.plan(p)
            out = torch.empty(eng.output_bytes() // 2, dtype=torch.int16, device="cuda")
            ref_iq, ref_st = oracle_run(p, n, 2.6e6)
            act = ref_st["prn"] > 0
            for rep in range(2):
                eng.execute(out.data_ptr())
                with torch.cuda.stream(st):  # the caller's own work behind the batch, same stream
                    for _ in range(4):
                        filler.mul_(1.0001)
                state, stats = eng.finish()
                assert stats["n_epochs"] == n_ep and stats["chain_mismatch"] == 0 and stats["n_active_max"] == 2 + k
                assert np.array_equal(state["prn"], ref_st["prn"])
                assert np.array_equal(state["carr_phase"][act].view(np.uint64), ref_st["carr_phase"][act].view(np.uint64))
                assert np.array_equal(state["page"][act], ref_st["page"][act])
                assert np.array_equal(out.cpu().numpy(), ref_iq)
            torch.cuda.synchronize()


def test_single_stream_mode(pkg):
    """GAL_CFG_SINGLE_STREAM: walkers and synthesis on the caller's stream (no internal high-priority stream)."""
    p = pkg.workloads.make_synthetic(n_epochs=4, n_chan=7, n_slots=16, samples_per_epoch=52000, seed=606)
    _compare(pkg, p, 52000, flags=pkg.synth.GAL_CFG_SINGLE_STREAM)


def test_two_handles_in_flight(pkg):
    """Software pipeline as bench.py runs it: two handles on two streams, executes interleaved."""
    import torch

    n = 52000
    pa = pkg.workloads.make_synthetic(n_epochs=4, n_chan=6, n_slots=16, samples_per_epoch=n, seed=81)
    pb = pkg.workloads.make_synthetic(n_epochs=4, n_chan=9, n_slots=16, samples_per_epoch=n, seed=82)
    ea = pkg.SynthEngine(samples_per_epoch=n, device=0)
    eb = pkg.SynthEngine(samples_per_epoch=n, device=0)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    ea.set_stream(sa.cuda_stream)
    eb.set_stream(sb.cuda_stream)
    ea.plan(pa)
    eb.plan(pb)
    oa = torch.empty(ea.output_bytes() // 2, dtype=torch.int16, device="cuda")
    ob = torch.empty(eb.output_bytes() // 2, dtype=torch.int16, device="cuda")
    for _ in range(3):
        ea.execute(oa.data_ptr())
        eb.execute(ob.data_ptr())
        ea.finish()
        eb.finish()
    ra, _ = oracle_run(pa, n, 2.6e6)
    rb, _ = oracle_run(pb, n, 2.6e6)
    assert np.array_equal(oa.cpu().numpy(), ra) and np.array_equal(ob.cpu().numpy(), rb)
    ea.close()
    eb.close()


def test_m_syn24_real_geometry(pkg):
    """BASELINE config 4 at its real geometry (24 SVs in two 12-channel launches, 25 MS/s, 2 500 000 samples per
    epoch), 4 epochs = 10 M samples: every sample against the oracle; chunking must not matter; a run split in two
    calls with the carried state equals the single run."""
    import torch

    n, rate = 2500000, 25e6
    p = pkg.workloads.m_syn24(n_epochs=4)
    ref_iq, ref_st = oracle_run(p, n, rate)
    outs = []
    for chunk in (0, 2048):
        with pkg.SynthEngine(sample_rate=rate, samples_per_epoch=n, n_slots=24, device=0, chunk_samples=chunk) as eng:
            eng.plan(p)
            out = torch.empty(eng.output_bytes() // 2, dtype=torch.int16, device="cuda")
            eng.execute(out.data_ptr())
            st, stats = eng.finish()
            assert stats["chain_mismatch"] == 0 and stats["n_active_max"] == 24 and eng.walk_counts()[2] == 0
            outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], ref_iq)
    assert np.array_equal(outs[1], ref_iq)
    act = ref_st["prn"] > 0
    assert np.array_equal(st["carr_phase"][act].view(np.uint64), ref_st["carr_phase"][act].view(np.uint64))
    with pkg.SynthEngine(sample_rate=rate, samples_per_epoch=n, n_slots=24, device=0) as eng:
        a, st_a, _ = eng.run_host(p[:3])
        q = p[3:].copy()
        q["flags"][0, :] = 0
        b, st_b, _ = eng.run_host(q, st_a)
    assert np.array_equal(np.concatenate([a, b]), ref_iq)
    assert np.array_equal(st_b["carr_phase"][act].view(np.uint64), ref_st["carr_phase"][act].view(np.uint64))


def test_m_dyn_full_size_properties(pkg):
    """BASELINE config 3 at full size (M-DYN: 2999 epochs x 260000 samples x 12 SVs, Doppler changing every epoch with
    a 10 Hz circular track):
      * EVERY epoch equals the oracle, int16 by int16, end state included (20 s of CPU on the GPU box's host); the last 4
        epochs once more from the oracle restarted on the carried state of a split run;
      * automatic chunking and chunk 1024 give the same bytes;
      * a run split 1500 + 1499 with the carried state equals the single run, end state included;
      * the chain self-check is clean and the all-walked fallback is never needed."""
    import torch

    n, rate = 260000, 2.6e6
    p = pkg.workloads.m_dyn()
    E = p.shape[0]
    assert E == 2999
    outs = []
    for chunk in (0, 1024):
        with pkg.SynthEngine(samples_per_epoch=n, n_slots=16, device=0, chunk_samples=chunk) as eng:
            eng.plan(p)
            out = torch.empty(eng.output_bytes() // 2, dtype=torch.int16, device="cuda")
            eng.execute(out.data_ptr())
            st, stats = eng.finish()
            assert stats["chain_mismatch"] == 0 and eng.walk_counts()[2] == 0
            if chunk == 0:
                state_full = st
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    del outs[1:]
    bad, ref_end = oracle_matches_device(outs[0], p, n, rate)
    assert bad == 0, "%d int16 values of the full-size output differ from the oracle" % bad
    act0 = state_full["prn"] > 0
    assert np.array_equal(ref_end["carr_phase"][act0].view(np.uint64), state_full["carr_phase"][act0].view(np.uint64))
    with pkg.SynthEngine(samples_per_epoch=n, n_slots=16, device=0) as eng:
        eng.plan(p[:1500])
        a = torch.empty(eng.output_bytes() // 2, dtype=torch.int16, device="cuda")
        eng.execute(a.data_ptr())
        st_a, _ = eng.finish()
        q = p[1500:].copy()
        q["flags"][0, :12] = 0
        eng.plan(q, st_a)
        b = torch.empty(eng.output_bytes() // 2, dtype=torch.int16, device="cuda")
        eng.execute(b.data_ptr())
        st_b, _ = eng.finish()
        # state at epoch 2995 from a third plan, so that the oracle can replay the last 4 epochs on its own
        eng.plan(q[:1495], st_a)
        c = torch.empty(eng.output_bytes() // 2, dtype=torch.int16, device="cuda")
        eng.execute(c.data_ptr())
        st_c, _ = eng.finish()
    assert torch.equal(outs[0][: a.numel()], a) and torch.equal(outs[0][a.numel():], b)
    act = state_full["prn"] > 0
    assert np.array_equal(st_b["carr_phase"][act].view(np.uint64), state_full["carr_phase"][act].view(np.uint64))
    assert np.array_equal(st_b["page"][act], state_full["page"][act])
    tail = p[2995:].copy()
    tail["flags"][0, :12] = 0
    ref_tail, ref_st = oracle_run(tail, n, rate, st_c)
    assert np.array_equal(outs[0][2995 * n * 2:].cpu().numpy(), ref_tail)
    assert np.array_equal(ref_st["carr_phase"][act].view(np.uint64), state_full["carr_phase"][act].view(np.uint64))


@pytest.mark.parametrize("block_legs", [8, 3])
def test_long_batch_stitcher_on_small_batches(pkg, monkeypatch, block_legs):
    """A batch with more than 256 carrier legs per slot (32 epochs) is stitched by several blocks per slot that exchange
    their aggregates inside the launch (k_scanm: tickets, look-back).  The full-size tests cover it at 1199 / 2999 epochs;
    here the fault-injection build gives a block 8 (3) legs instead of 256, so that small random batches (channels coming
    and going, idle epochs, sign changes, tie-prone steps) hit every corner of the exchange quickly -- with 3 legs a block
    ends inside an epoch and the "big" cases need more than one round of 256 records in the look-back."""
    monkeypatch.setenv("GAL_SCAN_BLOCK_LEGS", str(block_legs))  # honoured by the GAL_TEST_HOOKS build only
    from fuzz_cases import random_case

    rng = np.random.default_rng(77)
    for c in range(60 if block_legs == 8 else 30):
        p, n_samp, rate, chunk = random_case(pkg, rng, big=(c % 15 == 14))
        with pkg.SynthEngine(sample_rate=rate, samples_per_epoch=n_samp, n_slots=p.shape[1], device=0, chunk_samples=chunk,
                             test_hooks=True) as eng:
            iq, st, stats = eng.run_host(p)
            fallbacks = eng.walk_counts()[2]
        ref_iq, ref_st = oracle_run(p, n_samp, rate)
        assert stats["chain_mismatch"] == 0 and fallbacks == 0, c
        assert np.array_equal(iq, ref_iq), c
        act = ref_st["prn"] > 0
        assert np.array_equal(st["carr_phase"][act].view(np.uint64), ref_st["carr_phase"][act].view(np.uint64)), c
