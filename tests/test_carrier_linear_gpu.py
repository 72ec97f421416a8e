"""k_synth_g's linear carrier start and its biased sign-mask address (synth_group.hip: SG_LIN_CYCLES, SgRecLin) on the device: every
case bit for bit against the oracle, 12 channels, epochs of 2 x 1024 + 100 samples -- two full chunks and a ragged tail.  Which start
a batch runs is the plan's verdict (test_carrier_linear_cpu.host_verdict, the same gates on the same records); the hooks build's
GAL_G_LINEAR=0 sends a batch the linear start would take through the legacy instances, and both outputs must be the same.
Listed groups observed on an MI355X, linear / legacy start: 25 / 25 at the limit (each of the four rates), 0 / 0 with the sign changes
and with the standing carriers, 3 / 3 with the phases just below 1, 4 / 4 with the code wraps (each of the four positions)."""
import numpy as np
import pytest

from test_carrier_linear_cpu import f_carr_at_limit, host_verdict
from test_parity_gpu import _compare

pytestmark = pytest.mark.gpu

N = 2 * 1024 + 100
K_CODE = 0.0006493506493506494
# Groups the linear start may list beyond the legacy one's on the same inputs.  The two DDA words of a sample differ by their rounding
# histories, a few units of the 2^-32 fraction word (file header of synth_group.hip), so a sample is listed by one start and not by the
# other only if its word lies that close to the band's edge at 128: about 2^-29 of the samples.  A handful covers it.
HANDFUL = 4


def _batch(pkg, rate=2.6e6, n_epochs=3, seed=1):
    return pkg.workloads.make_synthetic(n_epochs=n_epochs, n_chan=12, n_slots=16, samples_per_epoch=N, sample_rate=rate, seed=seed)


def _set_doppler(p, e, j, f):
    p["f_carr"][e, j] = f
    p["f_code"][e, j] = 1.023e6 + f * K_CODE


def _both_starts(pkg, p, rate, monkeypatch, linear=1):
    """The batch through the start the plan picks (`linear`: which one that must be) and, if that is the linear one, through the
    legacy instances too: each equal to the oracle (_compare), and to each other.  Returns the listed-group counts (picked, legacy)."""
    monkeypatch.delenv("GAL_G_LINEAR", raising=False)
    assert host_verdict(pkg, p, N, rate) == (1, 0, linear)
    iq, _, stats = _compare(pkg, p, N, rate=rate, test_hooks=True)
    assert stats["kernel_family"] == 1 and stats["chain_mismatch"] == 0 and stats["exact_records"] == 0 and stats["window_mode"] < 16, stats
    if not linear:
        return stats["repaired_groups"], stats["repaired_groups"]
    monkeypatch.setenv("GAL_G_LINEAR", "0")
    assert host_verdict(pkg, p, N, rate) == (1, 0, 0)
    iq2, _, stats2 = _compare(pkg, p, N, rate=rate, test_hooks=True)
    monkeypatch.delenv("GAL_G_LINEAR")
    assert stats2["kernel_family"] == 1 and stats2["chain_mismatch"] == 0 and stats2["window_mode"] == stats["window_mode"], stats2
    assert np.array_equal(iq, iq2)
    print("listed groups: linear start %d, legacy start %d" % (stats["repaired_groups"], stats2["repaired_groups"]))
    assert stats["repaired_groups"] <= stats2["repaired_groups"] + HANDFUL, (stats["repaired_groups"], stats2["repaired_groups"])
    return stats["repaired_groups"], stats2["repaired_groups"]


@pytest.mark.parametrize("rate", [2.6e6, 4.0e6, 10.0e6, 16.0e6])
def test_doppler_beside_the_limit_in_every_window_form(pkg, rate, monkeypatch):
    """One rate per window form (2.6: holds, 4: any pattern, 10: <= 4 advances, 16: <= 2).  The largest Doppler the gate admits, both
    signs, from phases just below 1 (the table's last cycle) and elsewhere: the linear start.  The next double above it on ONE record:
    the legacy start for the batch."""
    p = _batch(pkg, rate, seed=int(rate / 1e5))
    f_in, f_out = f_carr_at_limit(rate), f_carr_at_limit(rate, above=True)
    for e in range(3):
        for j, f in ((0, f_in), (1, -f_in), (2, f_in), (3, -f_in)):
            _set_doppler(p, e, j, f)
    p["carr_phase0"][0, :4] = [1.0 - 2.0 ** -53, -(1.0 - 2.0 ** -53), 0.25, 0.0]
    _both_starts(pkg, p, rate, monkeypatch, linear=1)
    _set_doppler(p, 1, 2, f_out)
    _both_starts(pkg, p, rate, monkeypatch, linear=0)
    _set_doppler(p, 1, 2, -f_out)
    _both_starts(pkg, p, rate, monkeypatch, linear=0)


def test_doppler_sign_change_between_epochs(pkg, monkeypatch):
    """The phase an epoch ends with keeps its sign into the next one: with the step's sign flipped the mirrored phase starts negative
    (the table's first 512 entries) and climbs through zero without a wrap."""
    p = _batch(pkg, seed=2)
    for j in range(12):
        f = (250.0 + 400.0 * j) * (1.0 if j % 2 else -1.0)
        for e in range(3):
            _set_doppler(p, e, j, f if e != 1 else -f)
    _set_doppler(p, 2, 0, -40.0)   # ... and slowly: negative for the whole epoch
    _set_doppler(p, 1, 1, 0.7)
    _both_starts(pkg, p, 2.6e6, monkeypatch)


def test_standing_carrier(pkg, monkeypatch):
    """Steps of +0 and -0: the loader lane puts the phase in the middle of its entry, the groups add zero -- also with the phase ON an
    index boundary, where a moving carrier's sample would be undecided."""
    p = _batch(pkg, seed=3)
    p["f_carr"][:, 0:6] = [0.0, -0.0, 0.0, -0.0, 0.0, -0.0]
    p["f_code"][:, 0:6] = 1.023e6
    p["carr_phase0"][0, 0:6] = [0.0, 0.0, 100.0 / 511.0, -100.0 / 511.0, 1.0 - 2.0 ** -53, 0.3]
    p["f_carr"][2, 6] = 0.0        # a carrier that stops: its phase is wherever the chain left it
    _both_starts(pkg, p, 2.6e6, monkeypatch)


def test_start_phase_a_few_ulp_below_one(pkg, monkeypatch):
    """The chunk at an epoch's start takes the record's phase as it is: 1 - 1, 2, 3 ulp (and their negatives under a negative step)
    with ordinary Dopplers -- the first sample sits in the last entry of a cycle, the next ones behind the wrap."""
    p = _batch(pkg, seed=4)
    ulp = 2.0 ** -53
    p["carr_phase0"][0, 0:6] = [1.0 - ulp, 1.0 - 2 * ulp, 1.0 - 3 * ulp, -(1.0 - ulp), -(1.0 - 2 * ulp), -(1.0 - 3 * ulp)]
    for e in range(3):
        for j, f in enumerate((3499.0, 0.01, 1000.0, -3499.0, -0.01, -1000.0)):
            _set_doppler(p, e, j, f)
    _both_starts(pkg, p, 2.6e6, monkeypatch)


@pytest.mark.parametrize("where", [0, 1, 15, 16])
def test_code_wrap_at_group_positions(pkg, where, monkeypatch):
    """The code wrap after 1040 + `where` samples of epoch 0 (1040 = 65 groups, in the second chunk): at the first, second and last
    sample of a group and at the first of the next one, and at the same places of the first chunk; symbols of either sign on both
    sides.  The mask's address is the clamp of the half-chip word itself here."""
    p = _batch(pkg, seed=950 + where)
    step = p["f_code"][0, :12] / 2.6e6
    at = np.array([1040, 1040, 1040, 1040, 16, 16, 16, 16, 2032, 2032, 2128, 2128]) + where
    p["code_phase0"][0, :12] = 4092.0 - at * step + np.tile([0.0, 1e-9, -1e-9, 0.3], 3) * step
    p["ibit0"][0, :12] = [10, 499, 24, 498, 0, 11, 12, 13, 499, 250, 251, 252]
    _both_starts(pkg, p, 2.6e6, monkeypatch)
