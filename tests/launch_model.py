"""The launch that k_iq_wsum, k_iq_echo, k_iq_refl and k_iq_array share (galk_launch_iq_wsum in csrc/iq_gain.hip, copied by the three
others), restated -- TEST INFRASTRUCTURE: the product never imports this.  A grid of (bx, by) blocks of 256 lanes, at most 2048 blocks:
  by   = min(n_epochs, 2048)                block y takes the epochs y, y + by, y + 2 by, ...
  need = ceil((spe / 4) / 256)              blocks that give every 16-byte vector (4 complex samples) of an epoch a lane of its own
  cap  = 2048 / by
  bx   = min(need, cap), at least 1         lane t of block x takes the epoch's whole vectors x 256 + t, + bx 256, + 2 bx 256, ...
The up to three samples in front of an epoch's first whole vector and behind its last are taken by block x = 0, one per lane."""
import numpy as np

K_BLOCKS, K_LANES = 2048, 256  # kMaxBlocks of the four .hip files, kThreads of csrc/iq_dev.h


def launch(spe, n_epochs):
    by = min(n_epochs, K_BLOCKS)
    need, cap = (spe // 4 + K_LANES - 1) // K_LANES, K_BLOCKS // by
    bx = max(1, min(need, cap))
    a = np.arange(n_epochs, dtype=np.int64) * spe
    vec = (a + spe) // 4 - (a + 3) // 4  # whole vectors of every epoch
    return {"by": by, "bx": bx, "need": need, "cap": cap, "y_trips": -(-n_epochs // by), "vec": vec, "x_stride": bx * K_LANES,
            "x_trips": -(-vec // (bx * K_LANES))}


# name: (spe, n_epochs) -- the smallest totals at which a lane takes a second vector (cap < need): by x cap x 1024 samples, about 2.1 M
# however they are split.  tests/test_iq_launch_geometry_cpu.py asserts what each is for.
GEOMETRIES = {
    "rows_and_lanes_stride": (1030, 2051),  # by = 2048 < 2051 epochs AND cap = 1 < need = 2: both loops stride
    "uneven_x_stride": (4101, 600),         # cap = 3 < need = 5: a second trip that 256 or 257 of 768 lanes take; every start offset
}


def second_trip_samples(spe, n_epochs):
    """(first, end): per epoch the complex samples [first, end) of the call that lanes write on their SECOND x trip (end = first where
    the epoch has none): the whole vectors from v0 + x_stride on."""
    L = launch(spe, n_epochs)
    a = np.arange(n_epochs, dtype=np.int64) * spe
    v0, v1 = (a + 3) // 4, (a + spe) // 4
    lo = np.minimum(v0 + L["x_stride"], v1)
    hi = np.minimum(v0 + 2 * L["x_stride"], v1)
    return 4 * lo, 4 * hi


def second_trip_windows(spe, n_epochs, delay, frac_q12, gain_q7):
    """Where the delayed windows of the second x trip begin, for ONE echo given as per-epoch columns (gain 0: no echo in that epoch).
    The lane that writes the samples n .. n + 3 reads n - D' .. n - D + 3, D' = D + (F > 0).  Counts of second-trip lanes over the call:
      lanes        that have the echo at all
      other_epoch  whose window begins in front of the lane's own epoch
      first_trip   whose window begins in front of the trip: in a vector that ANOTHER lane wrote on its first trip
      epoch_start  whose window begins in the epoch's first four samples (the head samples and the first vector's start)"""
    first, end = second_trip_samples(spe, n_epochs)
    a = np.arange(n_epochs, dtype=np.int64) * spe
    Dp = np.asarray(delay, dtype=np.int64) + (np.asarray(frac_q12) > 0)
    on = np.asarray(gain_q7) > 0
    lanes = (end - first) // 4
    # lane j of the trip begins at first + 4 j, its oldest sample is first + 4 j - D': in front of `lim` for j < (lim + D' - first) / 4
    below = lambda lim: np.clip(-(-(lim + Dp - first) // 4), 0, lanes)  # noqa: E731
    count = lambda c: int(np.where(on, c, 0).sum())  # noqa: E731
    return {"lanes": count(lanes), "other_epoch": count(below(a)), "first_trip": count(below(first)), "epoch_start": count(below(a + 4) - below(a))}


# ---- the model of one long call, for the tests that run an echo kernel at GEOMETRIES ---------------------------------------------------
# case: a dict with spe, parts, gains, wide_gains, e_wide, rows, pof (tests/test_iq_mpath_gpu.py and tests/test_iq_refl_gpu.py build
# them); model: mpath_model.mpath or refl_model.refl.
H = 1024  # GAL_ECHO_MAX_DELAY: the samples of a history line


def epoch_alone(model, case, gains, e, cos1024):
    """(bytes, saturation count) of epoch e of the case's long call under `gains`, from the model over that epoch alone: an epoch's
    output depends on its own gains and rows and on the parts, whose 1024 samples in front of the epoch stand in for the line."""
    spe, lo = case["spe"], case["spe"] * e
    assert lo >= H
    y, sat, _ = model(case["parts"][:, 2 * lo:2 * (lo + spe)], gains[e:e + 1], spe, case["pof"], case["rows"][e:e + 1], cos1024,
                      case["parts"][:, 2 * (lo - H):2 * lo])
    return y, sat


def long_call_model(model, case, cos1024):
    """The model's (bytes, count) of the long call on zero lines, under `gains` and under `wide_gains`.  The model runs ONCE over the
    call; the wide call differs in epoch e_wide alone, which is computed on its own (and, under `gains`, must give the long run's
    bytes: the cut is checked)."""
    spe, e = case["spe"], case["e_wide"]
    want, want_sat, _ = model(case["parts"], case["gains"], spe, case["pof"], case["rows"], cos1024)
    y, sat = epoch_alone(model, case, case["gains"], e, cos1024)
    assert np.array_equal(y, want[2 * spe * e:2 * spe * (e + 1)])
    y_wide, sat_wide = epoch_alone(model, case, case["wide_gains"], e, cos1024)
    wide = want.copy()
    wide[2 * spe * e:2 * spe * (e + 1)] = y_wide
    return (want, want_sat), (wide, want_sat - sat + sat_wide)
