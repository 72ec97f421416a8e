"""Every k_synth_g instance a plan can launch (tests/group_instance_model.py: 400 of the 480 compiled), run once and compared with the
oracle bit for bit: per (family, window form) one test that takes its batches through one engine per slot count.  A batch of 2 k
channels launches <k, false> and <k, true>; 6 and 13 (7 + 6) bring the two instances of six positions; the wide family runs 13 .. 24
in one launch and 26, 28 .. 48 in two.  tests/test_group_instances_cpu.py holds the batches against the model and the model against the
plan, and counts: the union of these batches' instances IS the reachable set.

Every batch: 3 epochs of 2 x 1024 + 100 samples (a chunk hand-over, a vector tail, a second block); every channel its own Doppler,
signs alternating, all inside the linear gate at the batch's rate; the first code wrap of position j near sample 200 + 150 j of the
batch, so in another group and lane for every position (a third of a sample off the sample grid: at the commensurate rates a wrap ON
the grid puts the groups around it on the pattern thresholds, and k_repair_g would replay just those); carr_phase0 = 0 on the first
half of the channels (group 0 is listed); from three channels on, slot 2 is idle in epoch 1 and back in epoch 2 as another PRN.

k_repair_g overwrites a listed group with the exact replay, so a batch may list at most 5 % of its 3 x 135 groups, and every (family,
form) must list some group somewhere.  kernel_family, exact_records, synth_runs, window_mode and n_active_max are asserted after
every run: the handle's hold-off or the list-overflow fall-back would put the exact replay in the kernel's place."""
import time

import numpy as np
import pytest

import group_instance_model as gim
from test_carrier_linear_cpu import _hooks, f_carr_at_limit
from test_group_scalar_consts_gpu import N, _coming_and_going, _set_doppler
from test_parity_gpu import _compare_on

pytestmark = pytest.mark.gpu

E = 3
GROUPS = E * ((N + 15) // 16)                 # 3 x 135
LISTED_CAP = GROUPS // 20                     # 5 %
ORDINARY = {1: 2.6e6, 2: 16.0e6, 3: 10.0e6, 4: 4.0e6}
RATES = {"linear": ORDINARY, "legacy": ORDINARY, "wide": ORDINARY,
         "search": {1: 2.728e6, 2: 16.368e6, 3: 8.184e6, 4: 4.092e6},    # 3, 8, 4, 2 samples per half chip and a half
         "cboc": {1: 2.6e6, 2: 16.0e6, 3: 8.0e6, 4: 4.0e6}}
NARROW_CHANNELS = (1, 2, 3, 4, 5, 6, 12, 13, 14, 16, 18, 20, 22, 24)
WIDE_CHANNELS = tuple(range(13, 25)) + tuple(range(26, 49, 2))
# Batches that take another seed and Doppler set than the rule's (variant 1: base 307 Hz).  As variant 0 these three need a second pass
# of the speculative carrier walk (stats.walk_passes == 2, measured on an MI355X; the other 317 need one), and a handle whose batch
# before needed one pass enqueues one: gal_synth_finish then walks on and synthesises again -- synth_runs == 2, through the same instance
VARIANTS = {("search", 4, 22): 1, ("search", 4, 24): 1, ("wide", 1, 23): 1}
CASES = [(fam, form) for fam in gim.FAMILIES for form in gim.MODES]


def channels_of(family):
    return WIDE_CHANNELS if family == "wide" else NARROW_CHANNELS


def slots_of(n_chan):
    return 48 if n_chan > 24 else 24


def build_batch(pkg, family, form, n_chan, variant=None):
    """(records, rate, engine flags) of one batch of the matrix.  variant: another seed and other Dopplers (VARIANTS names a batch's)."""
    rate = RATES[family][form]
    n_slots = slots_of(n_chan)
    variant = VARIANTS.get((family, form, n_chan), 0) if variant is None else variant
    seed = 7000 + 1000 * gim.FAMILIES.index(family) + 100 * form + n_chan + 100000 * variant
    p = pkg.workloads.make_synthetic(n_epochs=E, n_chan=n_chan, n_slots=n_slots, samples_per_epoch=N, sample_rate=rate, seed=seed)
    f_in = f_carr_at_limit(rate)
    base = 300.0 + 7.0 * variant
    step = min(270.0, (0.9 * f_in - base) / max(n_chan - 1, 1))
    for j in range(n_chan):
        f = (-1.0 if j % 2 else 1.0) * (base + step * j)
        if family == "legacy" and j == 0:
            f = f_carr_at_limit(rate, above=True)      # ONE record beyond the linear gate: the batch takes the legacy start
        for e in range(E):
            _set_doppler(p, e, j, f)
        # the first wrap near sample 200 + 150 j of the batch (42 positions fit its 6444 samples), the phase carried over the epochs
        w = 200.0 + 150.0 * (j % 42) + 75.0 * (j // 42) + 0.37 + 0.01 * j
        cstep = p["f_code"][0, j] / rate
        ib0 = 499 - j if j < 2 else int(p["ibit0"][0, j])   # positions 0 and 1: the wrap ends a page, and the symbol before that
        tot = 4092.0 - w * cstep + np.arange(E) * (N * cstep)
        wraps = np.floor(tot / 4092.0)
        p["code_phase0"][:, j] = np.clip(tot - wraps * 4092.0, 0.0, np.nextafter(4092.0, 0.0))
        p["ibit0"][:, j] = (ib0 + wraps.astype(np.int64)) % 500
    p["carr_phase0"][0, :max(1, n_chan // 2)] = 0.0
    if n_chan >= 3:
        _coming_and_going(pkg, p, seed + 50000)
    return p, rate, (pkg.synth.GAL_CFG_CBOC if family == "cboc" else 0)


def active_counts(p):
    return [int(np.count_nonzero(p["prn"][e] > 0)) for e in range(p.shape[0])]


def expected_launches(family, form, p):
    """What the model says this batch launches, given what its family is reached by."""
    return gim.launches(active_counts(p), form, N, cboc=family == "cboc", search=family == "search", linear=family != "legacy",
                        hooks=("GAL_G_WIDE",) if family == "wide" else ())


def plan_report(pkg, p, rate, flags):
    """The host-only plan of the hooks build on these records: kernel family, bisection instances, linear start, window form, launches
    per execute, and the size of every launch (the largest of its per-epoch position counts)."""
    import ctypes

    lib = _hooks(pkg)
    cfg = pkg.synth._Cfg(float(rate), N, int(p.shape[1]), 0, 0, 0, int(flags))
    p = np.ascontiguousarray(p)
    assert lib.gal_hooks_plan_host_ms(ctypes.byref(cfg), p.ctypes.data, p.shape[0], None, 1) >= 0.0
    out = {k: int(lib.gal_hooks_plan_host_array(k.encode()) or 0) - 1 for k in ("family", "search", "linear", "form", "groups")}
    nact = np.ctypeslib.as_array(ctypes.cast(lib.gal_hooks_plan_host_array(b"nact"), ctypes.POINTER(ctypes.c_int32)),
                                 shape=(out["groups"], p.shape[0]))
    out["sizes"] = [int(v) for v in nact.max(axis=1)]
    return out


def check_plan(pkg, family, form, p, rate, flags):
    """The plan's verdict on the batch is the family and the launches the model names."""
    want = expected_launches(family, form, p)
    got = plan_report(pkg, p, rate, flags)
    assert got["family"] == 1 and got["form"] == form, (family, form, got)
    assert got["search"] == (1 if family == "search" else 0), (family, form, got)
    assert got["groups"] == len(want) and got["sizes"] == [nch for _, nch, _, _ in want], (family, form, got, want)
    fams = {gim.family_of(nch, cboc=family == "cboc", search=got["search"] == 1, linear=got["linear"] == 1) for nch in got["sizes"]}
    assert fams == {fam for fam, _, _, _ in want}, (family, form, got, want)
    return want


@pytest.mark.parametrize("family,form", CASES, ids=["%s-form%d" % c for c in CASES])
def test_every_reachable_instance(pkg, family, form, monkeypatch):
    for name in ("GAL_G_WIDE", "GAL_G_NARROW", "GAL_G_LINEAR", "GAL_G_SEARCH"):
        monkeypatch.delenv(name, raising=False)
    if family == "wide":
        monkeypatch.setenv("GAL_G_WIDE", "1")     # (the plan takes the wide instances on its own for 2048+ epochs of 1024+ chunks only)
    t0 = time.perf_counter()
    mode = form + (16 if family == "search" else 0)
    listed = {}
    rate = RATES[family][form]
    flags = pkg.synth.GAL_CFG_CBOC if family == "cboc" else 0
    for n_slots in sorted({slots_of(n) for n in channels_of(family)}):
        with pkg.SynthEngine(sample_rate=rate, samples_per_epoch=N, n_slots=n_slots, device=0, flags=flags, test_hooks=family == "wide") as eng:
            for n_chan in (n for n in channels_of(family) if slots_of(n) == n_slots):
                p, _, _ = build_batch(pkg, family, form, n_chan)
                check_plan(pkg, family, form, p, rate, flags)
                _, _, stats = _compare_on(eng, p, N, rate, cboc=family == "cboc")
                assert stats["kernel_family"] == 1 and stats["exact_records"] == 0 and stats["synth_runs"] == 1, (n_chan, stats)
                assert stats["window_mode"] == mode and stats["n_active_max"] == n_chan and stats["chain_mismatch"] == 0, (n_chan, stats)
                listed[n_chan] = stats["repaired_groups"]
    print("%s form %d: listed groups of %d per batch %s; %.2f s" % (family, form, GROUPS, listed, time.perf_counter() - t0))
    assert max(listed.values()) <= LISTED_CAP, listed
    assert max(listed.values()) >= 1, listed
