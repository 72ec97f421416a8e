"""k_synth_g's per-position constants in scalar registers (synth_group.hip: SG_SCAL -- the DDA's step 511 |d| and the carrier table's
base, fetched once per block and wave instead of read from LDS by every part of every group) on the device.  Every case bit for bit
against the oracle, through the start the plan picks (linear) and, in the hooks build, through the legacy start (GAL_G_LINEAR=0) on the
same records; epochs of 2 x 1024 + 100 samples -- two full chunks and a ragged tail -- and 3 of them unless a case says otherwise.

The arithmetic of a group is what it was, so the number of listed groups is too: the counts below were observed on an MI355X with the
kernel that read the constants from LDS, linear / legacy start, and each case asserts them without a margin.
    part shapes, 1 / 2 / 3 / 4 / 5 / 8 / 9 / 12 active channels           1 / 1 with 4 channels, 0 / 0 with the others   (PART_COUNTS)
    every epoch its own Dopplers and signs, a slot that goes and comes back with another PRN       0 / 0   (PER_BLOCK_COUNTS)
    one epoch of 2148 samples in two blocks (GAL_G_BPE=2)                  0 / 0
    one epoch of 40 x 1024 + 100 samples (sg_grid: two blocks)             1 / 1
    standing carriers and the gate's largest Doppler, both signs           0 / 0   (EDGE_COUNTS)
    4 / 10 / 16 MS/s                                                       0 / 0 each   (FORM_COUNTS)"""
import numpy as np
import pytest

from test_carrier_linear_cpu import f_carr_at_limit, host_verdict
from test_parity_gpu import _compare

pytestmark = pytest.mark.gpu

N = 2 * 1024 + 100
K_CODE = 0.0006493506493506494

PART_COUNTS = {1: (0, 0), 2: (0, 0), 3: (0, 0), 4: (1, 1), 5: (0, 0), 8: (0, 0), 9: (0, 0), 12: (0, 0)}
PER_BLOCK_COUNTS = {"three_epochs": (0, 0), "one_epoch_two_blocks": (0, 0), "one_long_epoch": (1, 1)}
EDGE_COUNTS = (0, 0)
FORM_COUNTS = {4.0e6: (0, 0), 10.0e6: (0, 0), 16.0e6: (0, 0)}


def _batch(pkg, n_chan=12, rate=2.6e6, n_epochs=3, seed=1, n=N):
    return pkg.workloads.make_synthetic(n_epochs=n_epochs, n_chan=n_chan, n_slots=16, samples_per_epoch=n, sample_rate=rate, seed=seed)


def _set_doppler(p, e, j, f):
    p["f_carr"][e, j] = f
    p["f_code"][e, j] = 1.023e6 + f * K_CODE


def _own_dopplers(p, n_chan, per_epoch=False):
    """Every channel its own Doppler, 270 Hz apart, signs alternating: a constant read from a neighbour's register changes the output.
    per_epoch: every epoch another magnitude, and the opposite sign of the epoch before."""
    for e in range(p.shape[0]):
        for j in range(n_chan):
            sign = -1.0 if (j + (e if per_epoch else 0)) % 2 else 1.0
            _set_doppler(p, e, j, sign * (300.0 + 270.0 * j + (37.0 * e if per_epoch else 0.0)))


def _both_starts(pkg, p, rate, monkeypatch, mode, n=N):
    """The batch through the linear start (the plan's choice) and through the legacy instances: each equal to the oracle (_compare), equal
    to each other, the same number of listed groups.  Returns that number for (linear, legacy)."""
    monkeypatch.delenv("GAL_G_LINEAR", raising=False)
    assert host_verdict(pkg, p, n, rate) == (1, 0, 1)
    iq, _, stats = _compare(pkg, p, n, rate=rate, test_hooks=True)
    assert stats["kernel_family"] == 1 and stats["chain_mismatch"] == 0 and stats["exact_records"] == 0, stats
    assert stats["window_mode"] == mode, stats
    monkeypatch.setenv("GAL_G_LINEAR", "0")
    assert host_verdict(pkg, p, n, rate) == (1, 0, 0)
    iq2, _, stats2 = _compare(pkg, p, n, rate=rate, test_hooks=True)
    monkeypatch.delenv("GAL_G_LINEAR")
    assert stats2["kernel_family"] == 1 and stats2["chain_mismatch"] == 0 and stats2["exact_records"] == 0, stats2
    assert stats2["window_mode"] == mode, stats2
    assert np.array_equal(iq, iq2)
    print("listed groups: linear start %d, legacy start %d" % (stats["repaired_groups"], stats2["repaired_groups"]))
    assert stats["repaired_groups"] == stats2["repaired_groups"], (stats["repaired_groups"], stats2["repaired_groups"])
    return stats["repaired_groups"], stats2["repaired_groups"]


@pytest.mark.parametrize("n_chan", [1, 2, 3, 4, 5, 8, 9, 12])
def test_every_part_shape(pkg, n_chan, monkeypatch):
    """Parts of 1, 2, 3, 4, 3+2, 4+4, 3+3+3 and 4+4+4 positions: every CNT at every J0 the instances for up to 12 channels have."""
    p = _batch(pkg, n_chan, seed=1200 + n_chan)
    _own_dopplers(p, n_chan)
    assert _both_starts(pkg, p, 2.6e6, monkeypatch, mode=1) == PART_COUNTS[n_chan]


def _coming_and_going(pkg, p, seed):
    """Slot 2: idle in epoch 1 (eleven positions there, the ones behind it move up), back in epoch 2 with PRN 33 and a Doppler of its own."""
    q = pkg.workloads.make_synthetic(n_epochs=3, n_chan=1, n_slots=16, samples_per_epoch=N, seed=seed, prns=[33])
    p[1, 2] = np.zeros((), dtype=p.dtype)
    p[2, 2] = q[2, 0]
    p["flags"][2, 2] = pkg.GAL_CH_RESTART
    p["carr_phase0"][2, 2] = 0.625
    p["page_init"][2, 2] = q["page_next"][0, 0]
    _set_doppler(p, 2, 2, -1111.0)


def test_constants_are_fetched_again_by_every_block(pkg, monkeypatch):
    """One block per epoch: every epoch has its own Dopplers, of the opposite sign of the epoch before (the other table's base), and one
    slot goes idle and comes back as another satellite."""
    p = _batch(pkg, 12, seed=1301)
    _own_dopplers(p, 12, per_epoch=True)
    _coming_and_going(pkg, p, 1302)
    assert _both_starts(pkg, p, 2.6e6, monkeypatch, mode=1) == PER_BLOCK_COUNTS["three_epochs"]


def test_one_epoch_in_several_blocks(pkg, monkeypatch):
    """Blocks that share an epoch: the three chunks of one short epoch as two blocks (the hooks build's GAL_G_BPE), and an epoch of 41
    chunks, which sg_grid cuts in two by itself."""
    p = _batch(pkg, 12, n_epochs=1, seed=1303)
    _own_dopplers(p, 12)
    monkeypatch.setenv("GAL_G_BPE", "2")
    assert _both_starts(pkg, p, 2.6e6, monkeypatch, mode=1) == PER_BLOCK_COUNTS["one_epoch_two_blocks"]
    monkeypatch.delenv("GAL_G_BPE")
    n = 40 * 1024 + 100
    p = _batch(pkg, 12, n_epochs=1, seed=1304, n=n)
    _own_dopplers(p, 12)
    assert _both_starts(pkg, p, 2.6e6, monkeypatch, mode=1, n=n) == PER_BLOCK_COUNTS["one_long_epoch"]


def test_standing_carrier_and_the_largest_doppler(pkg, monkeypatch):
    """Steps of +0 and -0 (a step of 0.0 in the register, the plain and the conjugate table) and the largest Doppler the linear gate
    admits, both signs: the sign half of the table base comes out of the scalar."""
    p = _batch(pkg, 12, seed=1305)
    _own_dopplers(p, 12)
    f_in = f_carr_at_limit(2.6e6)
    for e in range(3):
        for j, f in ((0, 0.0), (1, -0.0), (2, f_in), (3, -f_in), (6, -0.0), (7, 0.0), (10, -f_in), (11, f_in)):
            _set_doppler(p, e, j, f)
    p["carr_phase0"][0, [0, 1, 6, 7]] = [100.0 / 511.0, -100.0 / 511.0, 0.3, 1.0 - 2.0 ** -53]
    assert _both_starts(pkg, p, 2.6e6, monkeypatch, mode=1) == EDGE_COUNTS


@pytest.mark.parametrize("rate,mode", [(4.0e6, 4), (10.0e6, 3), (16.0e6, 2)])
def test_the_other_window_forms(pkg, rate, mode, monkeypatch):
    """Any pattern of holds (4 MS/s), at most four advances (10), at most two (16): the other three MODEs of the same instances."""
    p = _batch(pkg, 12, rate=rate, seed=1400 + int(rate / 1e6))
    _own_dopplers(p, 12)
    assert _both_starts(pkg, p, rate, monkeypatch, mode=mode) == FORM_COUNTS[rate]
