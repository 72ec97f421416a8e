"""The launch geometries that the echo, reflector and array kernels are held at, without a GPU: what tests/launch_model.py says about each
shape, and that the inputs which the GPU tests build at them (the same builders, the same seeds) are what those tests are for -- some
values clamp and most do not, the instance is the one named, the second x trip reads where it should.  A change of kMaxBlocks or
kThreads that empties a case fails here.  Below that, the same for the tile launches of the oscillator and the scintillation pass
(tests/tile_launch_model.py): the trip counts, the scan's fill and the stepping of (j0, m0) that each named geometry is for."""
import os
import re

import numpy as np
import pytest

import array_model
import launch_model
import mpath_model
import osc_model
import refl_model
import scint_model
import test_iq_array_gpu as array_gpu
import test_iq_mpath_gpu as echo_gpu
import test_iq_refl_gpu as refl_gpu
import tile_launch_model as tlm
from launch_model import GEOMETRIES, launch, second_trip_windows
from tile_launch_model import OSC_GEOMETRIES, SCINT_GEOMETRIES, osc_launch, scint_geometry, scint_launch, scint_trips

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "galileo-sdr-sim_amd", "csrc")


@pytest.fixture(scope="module")
def cos1024(pkg):
    return pkg.tables()["cos1024"]


def test_the_model_has_the_kernels_constants():
    """launch_model restates kMaxBlocks of the four launchers and kThreads of iq_dev.h: a change there must be followed here, and then the
    geometries below show whether they still reach what they are for."""
    def const(path, name):
        with open(os.path.join(CSRC, path)) as f:
            return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))

    for src in ("iq_gain.hip", "iq_echo.hip", "iq_refl.hip", "iq_array.hip"):
        assert const(src, "kMaxBlocks") == launch_model.K_BLOCKS, src
    assert const("iq_dev.h", "kThreads") == launch_model.K_LANES
    assert mpath_model.H == launch_model.H == 4 * launch_model.K_LANES  # a line is exactly one block's trip: see test_second_trip_*


def test_rows_and_lanes_stride():
    spe, n_epochs = GEOMETRIES["rows_and_lanes_stride"]
    assert (spe, n_epochs) == (1030, 2051)
    L = launch(spe, n_epochs)
    # by = 2048 < 2051: blocks y = 0, 1, 2 take a second epoch; cap = 1 < need = 2: the one x block walks 257 vectors in two trips, the
    # second with one lane; the epochs begin at value offsets 0 and 2 of a vector in turn
    assert (L["by"], L["y_trips"], n_epochs - L["by"]) == (2048, 2, 3)
    assert (L["cap"], L["need"], L["bx"]) == (1, 2, 1) and L["cap"] < L["need"]
    assert (L["vec"] == 257).all() and (L["x_trips"] == 2).all() and (L["vec"] - L["x_stride"] == 1).all()
    assert set((np.arange(n_epochs) * spe) % 4) == {0, 2}


def test_uneven_x_stride():
    spe, n_epochs = GEOMETRIES["uneven_x_stride"]
    assert (spe, n_epochs) == (4101, 600)
    L = launch(spe, n_epochs)
    # cap = 3 < need = 5: three x blocks, stride 768, over 1024 or 1025 vectors: a second trip that 256 or 257 of 768 lanes take
    assert (L["by"], L["y_trips"]) == (600, 1) and (L["cap"], L["need"], L["bx"], L["x_stride"]) == (3, 5, 3, 768)
    assert L["cap"] < L["need"] and set(L["vec"]) == {1024, 1025} and (L["x_trips"] == 2).all() and set(L["vec"] - 768) == {256, 257}
    assert set((np.arange(n_epochs) * spe) % 4) == {0, 1, 2, 3}


def test_a_second_x_trip_needs_two_million_samples():
    """A second trip needs spe / 4 > 256 bx with bx = cap = 2048 / by: more than by x cap x 1024 samples per call, which is 2.1 M where
    by divides 2048 and never below 1.05 M.  The cases stay below 2.5 M."""
    for spe, n_epochs in GEOMETRIES.values():
        L = launch(spe, n_epochs)
        floor = L["by"] * L["cap"] * 4 * launch_model.K_LANES
        assert launch_model.K_BLOCKS * 2 * launch_model.K_LANES < floor < spe * n_epochs < 2500000


def _windows(name, rows):
    spe, n_epochs = GEOMETRIES[name]
    tot = {}
    for r in range(rows.shape[1]):
        frac = rows["frac_q12"][:, r] if "frac_q12" in rows.dtype.names else np.zeros(n_epochs, np.int64)
        for k, v in second_trip_windows(spe, n_epochs, rows["delay"][:, r], frac, rows["gain_q7"][:, r]).items():
            tot[k] = tot.get(k, 0) + v
    return tot


def _second_trip_reads(name, rows):
    """What the delayed reads of the second x trip can reach, and that the case's rows reach it.

    A window in ANOTHER EPOCH than the lane's own vector cannot be had on a second trip, at these or any shapes: the trip begins at
    least 4 x 256 x bx >= 1024 samples into the epoch, and the oldest sample a lane reads is D' = D + (F > 0) <= 1024 samples old.
    (Windows in front of the epoch are the first trip's: every epoch of every case here has them, and the blocks' second y trip
    too.)  What the second trip does have, and must have here: windows that begin in front of the trip, in vectors that other lanes
    wrote on their first; and where bx = 1, a window that goes back exactly to the epoch's first samples."""
    spe, n_epochs = GEOMETRIES[name]
    L = launch(spe, n_epochs)
    assert 4 * L["x_stride"] >= launch_model.H
    w = _windows(name, rows)
    assert w["lanes"] > 0 and w["other_epoch"] == 0 and w["first_trip"] > 0
    if L["bx"] == 1:
        assert w["epoch_start"] > 0
    # the blocks' second y trip (rows_and_lanes_stride): its first lanes read the epoch in front, which another block wrote
    if L["y_trips"] > 1:
        assert ((rows["delay"][L["by"]:] > 0) & (rows["gain_q7"][L["by"]:] > 0)).any()


def _clamps_in_part(model, case, cos1024):
    """Both instances' model counts of the long call: some values clamp, most do not (a clamped value hides its arithmetic)."""
    n_val = case["parts"].shape[1]
    for gains, (_, sat) in zip((case["gains"], case["wide_gains"]), launch_model.long_call_model(model, case, cos1024)):
        assert 0 < sat < n_val // 4


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_echo_stride_inputs(cos1024, name):
    case = echo_gpu.stride_case(name)
    rows = case["rows"]
    assert (case["spe"], case["n_epochs"]) == GEOMETRIES[name] and case["parts"].shape == (3, 2 * case["spe"] * case["n_epochs"])
    assert rows.shape[1] == 8 and set(rows["delay"].ravel()) == set(echo_gpu.DELAYS) and set(case["pof"]) == {0, 2}
    assert rows["dph"].min() < -(3 << 29) and rows["dph"].max() > 3 << 29
    assert not mpath_model.needs_int64(case["gains"], rows) and mpath_model.needs_int64(case["wide_gains"], rows)
    beyond = [e for e in range(case["n_epochs"]) if mpath_model.needs_int64(case["wide_gains"][e:e + 1], rows[e:e + 1])]
    assert beyond == [case["e_wide"]]  # one row beyond 65535
    assert case["parts"].min() == -32768 and case["parts"].max() == 32767
    _second_trip_reads(name, rows)
    _clamps_in_part(mpath_model.mpath, case, cos1024)
    assert 1024 in case["second"][2]["delay"][0]  # the short call behind reads the whole line


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_refl_stride_inputs(cos1024, name):
    case = refl_gpu.stride_case(name)
    rows = case["rows"]
    assert (case["spe"], case["n_epochs"]) == GEOMETRIES[name] and rows.shape[1] == 8 and set(case["pof"]) == {0, 2}
    pairs = {(int(D), int(F)) for D, F in zip(rows["delay"].ravel(), rows["frac_q12"].ravel())}
    assert pairs == set(refl_gpu.DELAYS)
    mixed = ((rows["frac_q12"] > 0).any(axis=1) & (rows["frac_q12"] == 0).any(axis=1))
    assert mixed.mean() > 0.9  # F > 0 and F = 0 within an epoch
    for D, F in ((1023, 4095), (1024, 0)):
        at = np.flatnonzero(((rows["delay"] == D) & (rows["frac_q12"] == F)).any(axis=1))
        assert {10, case["n_epochs"] - 1} <= set(at)
    assert rows["dph"].min() < -(3 << 29) and rows["dph"].max() > 3 << 29
    assert not refl_model.needs_int64(case["gains"], rows) and refl_model.needs_int64(case["wide_gains"], rows)
    beyond = [e for e in range(case["n_epochs"]) if refl_model.needs_int64(case["wide_gains"][e:e + 1], rows[e:e + 1])]
    assert beyond == [case["e_wide"]]
    _second_trip_reads(name, rows)
    _clamps_in_part(refl_model.refl, case, cos1024)
    r2 = case["second"][2]
    assert (1024, 0) in zip(r2["delay"][0], r2["frac_q12"][0]) and (1023, 4095) in zip(r2["delay"][0], r2["frac_q12"][0])


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n_parts", refl_gpu.PART_COUNTS)
def test_refl_part_counts_inputs(cos1024, n_parts, wide):
    spe, parts, gains, pof, rows = refl_gpu.part_counts_case(n_parts, wide)
    assert refl_model.needs_int64(gains, rows) == wide and pof == [0, n_parts - 1, n_parts - 1]
    assert {(int(D), int(F)) for D, F in zip(rows["delay"][0], rows["frac_q12"][0])} == {(1, 4095), (1023, 1), (4, 2048)}
    assert all(sorted(zip(rows["delay"][e], rows["frac_q12"][e])) == sorted(zip(rows["delay"][0], rows["frac_q12"][0])) for e in (1, 2))
    assert len({tuple(rows["delay"][e]) for e in range(3)}) == 3  # permuted from epoch to epoch
    # neighbouring gains of the four-part body differ in nearly every row: a part taken with its neighbour's gain shows
    assert (gains[:, 3::4] != gains[:, 2::4][:, :gains[:, 3::4].shape[1]]).any()
    _, sat, _ = refl_model.refl(parts, gains, spe, pof, rows, cos1024)
    assert 0 < sat < parts.shape[1]
    unclamped_epochs = 2 if wide else 3
    assert sat < parts.shape[1] * (3 - unclamped_epochs) // 3 + parts.shape[1] // 5


def test_refl_32_echoes_inputs(cos1024):
    for wide in (False, True):
        spe, parts, gains, pof, rows = refl_gpu.echoes32_case(wide)
        assert rows.shape == (8, 32) and refl_model.needs_int64(gains, rows) == wide and set(pof) == {0, 1, 2}
        _, sat, _ = refl_model.refl(parts, gains, spe, pof, rows, cos1024)
        assert sat < parts.shape[1] // 4


@pytest.mark.parametrize("name,n_parts,n_elem,wide", array_gpu.STRIDE_CASES)
def test_array_stride_inputs(name, n_parts, n_elem, wide):
    spe, parts, w = array_gpu.stride_case(name, n_parts, n_elem, wide)
    n_epochs = GEOMETRIES[name][1]
    assert w.shape == (n_epochs, n_elem, n_parts, 2) and parts.shape == (n_parts, 2 * spe * n_epochs)
    assert array_model.needs_int64(w) == wide
    sums = np.abs(w).sum(axis=(2, 3))
    flat = w.reshape(n_epochs * n_elem, -1)
    assert len(np.unique(flat, axis=0)) == len(flat)  # every (epoch, element) has weights of its own
    if wide:
        assert parts.min() == -32768 and parts.max() == 32767
        _, sat = array_model.array(parts, w, spe)
        assert 0 < sat < n_elem * parts.shape[1] // 4
    else:
        assert np.count_nonzero(sums == 65535) == 1 and sums.max() == 65535
        e = int(np.argwhere(sums == 65535)[0][0])
        assert launch(spe, n_epochs)["y_trips"] == 1 or e >= launch(spe, n_epochs)["by"]


def test_every_array_instance_is_launched():
    """K = 1 .. 8 in both widths: the parametrisation of test_part_and_element_counts, read from the test itself."""
    marks = {m.args[0]: m.args[1] for m in array_gpu.test_part_and_element_counts.pytestmark}
    assert list(marks["n_elem"]) == list(range(1, array_model.GAL_ARRAY_MAX_ELEM + 1)) and list(marks["wide"]) == [False, True]
    assert {k // 2 for k in marks["n_parts"]} >= {0, 1, 2, 31, 32} and {k % 2 for k in marks["n_parts"]} == {0, 1}


# ---- the tile launches of the oscillator and the scintillation pass (tests/tile_launch_model.py) ----------------------------------
def test_the_tile_model_has_the_kernels_constants():
    def const(path, name):
        with open(os.path.join(CSRC, path)) as f:
            return re.search(r"constexpr int %s = ([^;]+);" % name, f.read()).group(1)

    for src in ("iq_osc.hip", "iq_scint.hip"):
        assert int(const(src, "kMaxBlocks")) == tlm.MAX_BLOCKS, src
        assert const(src, "kTile") == "4 * kThreads" and 4 * int(const("iq_dev.h", "kThreads")) == tlm.TILE, src
    assert int(const("iq_osc.hip", "kScanThreads")) == tlm.SCAN_LANES and int(const("iq_scint.hip", "kMaxNodes")) == tlm.MAX_NODES
    assert (osc_model.TILE, osc_model.MAX_BLOCKS) == (scint_model.TILE, scint_model.MAX_BLOCKS) == (tlm.TILE, tlm.MAX_BLOCKS)
    assert (scint_model.MIN_NODE, scint_model.MAX_NODE) == (64, 1 << 24)


def test_osc_third_trip():
    n, first = OSC_GEOMETRIES["third_trip"]
    assert n == (2 * tlm.MAX_BLOCKS + 3) * tlm.TILE + 2 == 4197378
    assert first % 4 == 1 and first > 2 ** 33  # two Philox blocks per lane
    la = osc_launch(n)
    # a third trip exists, in four blocks, and the last tile is partial
    assert (la["nt"], la["grid"], la["trips"], la["min_trips"], la["blocks_at_trips"]) == (4100, 2048, 3, 2, 4) and n % tlm.TILE == 2
    # nothing shorter has one: a tile less and no block takes a third trip
    assert osc_launch(n - 2 - 3 * tlm.TILE)["trips"] == 2 and osc_launch(n - 2 - 3 * tlm.TILE + 1)["trips"] == 3
    # the scan: several tiles per lane, the trailing lanes empty -- the state word is everything in front of the last lane
    assert (la["c"], la["scan_lanes"], la["last_lane_tiles"]) == (5, 820, 0) and not la["last_lane_full"]
    # the per-tile A and W are formed at tile indices beyond 2^22 samples
    assert (la["nt"] - 1) * tlm.TILE > 1 << 22


def test_osc_full_scan():
    n, first = OSC_GEOMETRIES["full_scan"]
    assert n == 3 * tlm.MAX_BLOCKS * tlm.TILE and first % 4 == 0 and first > 2 ** 33
    la = osc_launch(n)
    # every block takes exactly three trips; every lane of the scan is full and the last writes the state word from its own tiles
    assert (la["grid"], la["trips"], la["min_trips"], la["blocks_at_trips"]) == (2048, 3, 3, 2048)
    assert la["c"] == 6 and la["scan_lanes"] == tlm.SCAN_LANES and la["last_lane_full"] and la["last_lane_tiles"] == 6
    assert la["nt"] % tlm.SCAN_LANES == 0 and la["c"] > 1


def test_what_the_suite_had_reached_no_third_trip():
    """The cases from before: a second trip in four blocks, and c = 3 with empty trailing lanes."""
    la = osc_launch((tlm.MAX_BLOCKS + 3) * tlm.TILE + 2)
    assert (la["trips"], la["blocks_at_trips"], la["c"], la["last_lane_full"]) == (2, 4, 3, False) and la["scan_lanes"] < tlm.SCAN_LANES
    tr = scint_trips((32 + 3) * tlm.TILE + 2, 2 ** 40 + 1, 67, scint_launch((32 + 3) * tlm.TILE + 2, 64)["bx"])
    assert tr["trips"] == 2


def _recurrence_is_direct(tr, L):
    live = tr["live"]
    assert live[0].all() or tr["trips"] == 1
    assert np.array_equal(tr["j0"][live], tr["dj"][live]) and np.array_equal(tr["m0"][live], tr["dm"][live])
    assert 2 <= tr["nn"][live].min() and tr["nn"][live].max() <= tlm.MAX_NODES
    assert (tr["nn"][live] == (tr["dm"][live] + tlm.TILE - 1) // L + 2).all()
    assert (L - 1) * ((1 << 32) // L) < 1 << 32  # r R stays a uint32
    assert tr["sm"] < L and tr["m0"][live].max() < L


SWEEP_L = (64, 67, 1000, 1024, 1025, 40000, 162500, 1 << 24)
SWEEP_BX = (1, 32, 170, 2048)
SWEEP_FIRST = (0, 3, 2 ** 24 - 5, 2 ** 40 + 1, (2 ** 16 + 3) * 2 ** 24 - 5, 2 ** 62 - 10 * 2048 * 1024)


@pytest.mark.parametrize("L", SWEEP_L)
def test_the_scint_recurrence_is_the_direct_division(L):
    """Five trips (the last of five blocks at most, with a ragged end) at every block count: (j0, m0) stepped by (sj, sm) with the one
    correction are divmod(first + 1024 t, L) on every trip of every block."""
    for bx in SWEEP_BX:
        for first in SWEEP_FIRST:
            n = (4 * bx + min(bx, 5)) * tlm.TILE - 1021
            tr = scint_trips(n, first, L, bx)
            assert tr["trips"] == 5 and first + n < 1 << 62
            _recurrence_is_direct(tr, L)
    assert scint_launch(10 ** 9, 1)["bx"] == 2048 and scint_launch(10 ** 9, 12)["bx"] == 170 and scint_launch(10 ** 9, 64)["bx"] == 32
    assert scint_launch(5, 64)["bx"] == 1 and scint_launch(3 * tlm.TILE + 1, 1)["bx"] == 4


@pytest.mark.parametrize("name", list(SCINT_GEOMETRIES))
def test_the_named_scint_geometries_step_as_the_direct_division(name):
    la, trips = scint_geometry(name)
    for tr, (n, first, L) in zip(trips, SCINT_GEOMETRIES[name][1]):
        _recurrence_is_direct(tr, L)


def _crossings(n, first, L):
    """The job's samples that lie ON a node (N mod L = 0), the job's first excepted."""
    k = np.arange(1, n, dtype=np.int64)
    return k[(first + k) % L == 0]


def test_scint_node_lens_at_four_trips():
    la, trips = scint_geometry("node_lens_at_four_trips")
    n_jobs, jobs = SCINT_GEOMETRIES["node_lens_at_four_trips"]
    assert (n_jobs, la["bx"], la["nt"]) == (64, 32, 98) and jobs[:59] == [(4, k, 64) for k in range(59)]
    long = dict((L, (n, first, tr)) for (n, first, L), tr in zip(jobs[59:], trips[59:]))
    assert sorted(long) == [67, 1025, 40000, 162500, 1 << 24]
    stride = la["bx"] * tlm.TILE
    for L, (n, first, tr) in long.items():
        assert n >= (3 * 32 + 1) * tlm.TILE + 1 and n % tlm.TILE and n % 4  # a ragged end that is no whole vector either
        assert tr["trips"] == 4 and tr["live"][2].all() and tr["live"][3].sum() == 2  # a third trip in every block, a fourth in two
        assert (tr["sj"] == 0) == (L > stride)
    assert len({n for n, _, _ in long.values()}) == 5
    # L = 1025: just above a tile -- a whole tile between two nodes (nn = 2) and a node inside a tile (nn = 3); both branches of the step
    n, first, tr = long[1025]
    live = tr["live"]
    assert set(tr["nn"][live]) == {2, 3} and (tr["sj"], tr["sm"]) == (31, 993)
    assert (tr["fired"][1:] & live[1:]).any() and (~tr["fired"][1:] & live[1:]).any()
    # L = 40000 > the stride: sj = 0; three nodes inside the job, each inside a 16-byte vector; both branches
    n, first, tr = long[40000]
    assert tr["sj"] == 0 and first > 2 ** 33
    assert list(_crossings(n, first, 40000)) == [1001, 41001, 81001] and all(c % 4 == 1 for c in _crossings(n, first, 40000))
    assert (tr["fired"][1:] & tr["live"][1:]).any() and (~tr["fired"][1:] & tr["live"][1:]).any()
    # L = 162500 > 4 strides: block 0 goes 112499, 145267, then fires; blocks 0 .. 16 fire on the second step alone, the others on the
    # first alone
    n, first, tr = long[162500]
    assert tr["sj"] == 0 and first % 4 == 3 and first > 2 ** 33 and list(_crossings(n, first, 162500)) == [50001]
    assert list(tr["m0"][:3, 0]) == [112499, 145267, 178035 - 162500] and list(tr["fired"][:, 0]) == [False, False, True, False]
    assert 162500 > 4 * stride and list(tr["fired"][1]) == [x >= 17 for x in range(32)] and list(tr["fired"][2]) == [x < 17 for x in range(32)]
    assert not tr["fired"][3].any() and (tr["m0"][1, :17] - tr["m0"][0, :17] == stride).all()
    assert set(tr["nn"][tr["live"]]) == {2, 3}
    # L = 2^24, the largest admitted: first = k 2^24 - 5 beyond 2^40; the one node lies in block 0's second vector; r R near 2^32
    n, first, tr = long[1 << 24]
    assert first > 2 ** 40 and (first + 5) % (1 << 24) == 0 and list(_crossings(n, first, 1 << 24)) == [5]
    assert tr["fired"].sum() == 1 and tr["fired"][1, 0] and tr["m0"][0, 0] == (1 << 24) - 5
    assert ((1 << 24) - 1) * ((1 << 32) >> 24) == (1 << 32) - 256
    # L = 67: nodes everywhere, the most a tile can need but one
    n, first, tr = long[67]
    assert set(tr["nn"][tr["live"]]) == {17, 18} and tr["sj"] == 32768 // 67
    assert (tr["fired"][1:] & tr["live"][1:]).any() and (~tr["fired"][1:] & tr["live"][1:]).any()


def test_scint_cli_split():
    la, trips = scint_geometry("cli_split")
    n_jobs, jobs = SCINT_GEOMETRIES["cli_split"]
    # what the default batch gets: twelve scintillating satellites, 170 blocks each -- there over 2032 tiles in 12 trips, here over 346
    assert (n_jobs, la["bx"]) == (12, 170) and -(-2080000 // tlm.TILE) == 2032 and -(-2032 // 170) == 12
    assert {first % 4 for _, first, _ in jobs} == {0, 1, 2, 3} and len({first for _, first, _ in jobs}) == 12
    fired = not_fired = 0
    for tr, (n, first, L) in zip(trips, jobs):
        assert L == 162500 and n == (2 * 170 + 5) * tlm.TILE + 3 and (tr["sj"], tr["sm"]) == (1, 174080 - 162500)
        assert tr["trips"] == 3 and tr["live"][1].all() and tr["live"][2].sum() == 6  # a third trip in six blocks, the last partial
        fired += int((tr["fired"][1:] & tr["live"][1:]).sum())
        not_fired += int((~tr["fired"][1:] & tr["live"][1:]).sum())
        assert len(_crossings(n, first, L)) >= 2
    assert fired >= 12 and not_fired >= 12
    assert (trips[0]["fired"][2] & trips[0]["live"][2]).sum() == 6 and not trips[0]["fired"][1, :6].any()  # ... also into a third trip


def test_scint_b0_at_four_trips():
    la, trips = scint_geometry("b0_at_four_trips")
    n_jobs, jobs = SCINT_GEOMETRIES["b0_at_four_trips"]
    assert (n_jobs, la["bx"]) == (64, 32) and jobs[:63] == [(4, k, 64) for k in range(63)]
    tr = trips[63]
    assert tr["trips"] == 4 and tr["live"][2].all() and tr["live"][3].sum() == 2
