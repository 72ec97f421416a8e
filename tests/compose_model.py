"""What gal_synth_run_scint and gal_synth_run_array promise for a whole batch (include/galsynth.h), composed from the numpy models of the
single passes -- TEST INFRASTRUCTURE: the product never imports this.  Every slot's own stream (x_s of the header: the oracle's run, or
the engine's, of the batch with only that slot active) goes through scint_model.apply wherever its row is not the identity; then one
part per slot goes through mpath_model.Lines.call (echoes), gain_model.wsum (none) or array_model.array.  One part per slot is
legitimate because the engine's group part is the exact sum of its slots' streams as long as that sum stays inside int16, which
slots_fit_int16 asserts.  Nothing here knows of groups, jobs, tables or launches."""
import numpy as np

import array_model
import gain_model
import mpath_model
import scint_model

SCINT_FIELDS = scint_model.FIELDS


def is_identity(row):
    return int(row["a_q12"]) == 4096 and int(row["b_q12"]) == 0


def _row(rec):
    return scint_model.row(**{k: int(rec[k]) for k in SCINT_FIELDS})


def spans(scint_rows, slot):
    """[(e0, e1, row)]: the maximal runs of epochs e0 .. e1 - 1 in which the slot's row is one and the same, the identity's left out."""
    col = scint_rows[:, slot]
    out, e0 = [], 0
    while e0 < col.shape[0]:
        e1 = e0 + 1
        while e1 < col.shape[0] and col[e1] == col[e0]:
            e1 += 1
        if not is_identity(col[e0]):
            out.append((e0, e1, _row(col[e0])))
        e0 = e1
    return out


def fade(alone, scint_rows, first_sample, spe):
    """alone [n, n_epochs * spe * 2] int16 -> (the faded copy, complex samples the scintillation's clamp changed)."""
    parts = np.array(alone, dtype=np.int16, copy=True)
    sat = 0
    if scint_rows is None:
        return parts, sat
    assert parts.shape[1] == scint_rows.shape[0] * spe * 2
    for s in range(parts.shape[0]):
        for e0, e1, row in spans(scint_rows, s):
            y, n = scint_model.apply(parts[s, 2 * e0 * spe:2 * e1 * spe], row, int(first_sample) + e0 * spe)
            parts[s, 2 * e0 * spe:2 * e1 * spe] = y
            sat += n
    return parts, sat


def fading_slots(scint_rows, n):
    if scint_rows is None:
        return set()
    return {s for s in range(n) if spans(scint_rows, s)}


def slots_fit_int16(alone, own_part):
    """The slots that are no part of their own share groups by their gains; whichever way, a group's stream is a sum over some of them."""
    shared = [s for s in range(len(alone)) if s not in own_part]
    if shared:
        assert np.abs(np.asarray(alone, dtype=np.int64)[shared]).sum(axis=0).max() <= 32767, "a group's sum could leave int16"


def _active_gains(params, gains, n):
    assert not (params["prn"][:, n:] > 0).any(), "a slot beyond the streams given is active"
    return np.where(params["prn"][:, :n] > 0, np.asarray(gains, dtype=np.int64)[:, :n], 0)


def run_model(alone, params, gains, scint_rows, first_sample, spe, lines=None, slot_of_echo=(), echo_rows=None, cos1024=None):
    """gal_synth_run_scint: (bytes as int16, saturation count).  lines: the mpath_model.Lines that carries the echo history from batch to
    batch (None: a stream that starts here)."""
    n = len(alone)
    slot_of_echo = [int(s) for s in slot_of_echo]
    slots_fit_int16(alone, fading_slots(scint_rows, n) | set(slot_of_echo))
    parts, fsat = fade(alone, scint_rows, first_sample, spe)
    g = _active_gains(params, gains, n)
    if slot_of_echo:
        if lines is None:
            lines = mpath_model.Lines(cos1024)
        hist_id = [s if s in slot_of_echo else -1 for s in range(n)]
        y, sat = lines.call(parts, g, spe, slot_of_echo, echo_rows, hist_id)
    else:
        y, sat = gain_model.wsum(parts, g, spe)
    return y, sat + fsat


def steer_weights(params, gains, phase, n, cos1024):
    """[n_epochs, n_elem, n, 2]: steer_make of the slot's gain and phase; the gain 0 of an idle slot makes (0, 0) at any phase."""
    E, K = phase.shape[0], phase.shape[1]
    g = _active_gains(params, gains, n)
    w = np.zeros((E, K, n, 2), dtype=np.int64)
    for a in range(K):
        w[:, a, :, 0], w[:, a, :, 1] = array_model.steer_make(g, np.asarray(phase)[:, a, :n], cos1024)
    assert not w[np.broadcast_to(params["prn"][:, None, :n] <= 0, (E, K, n))].any()
    return w


def array_model_run(alone, params, gains, phase, scint_rows, first_sample, spe, cos1024):
    """gal_synth_run_array: (bytes as int16 [n_elem, n_val], saturation count).  Every slot is a part of its own there.  The array pass
    is a function of the epoch's samples and weights alone: it is taken epoch by epoch, which keeps the int64 copies small."""
    n = len(alone)
    parts, sat = fade(alone, scint_rows, first_sample, spe)
    w = steer_weights(params, gains, phase, n, cos1024)
    y = np.zeros((w.shape[1], parts.shape[1]), dtype=np.int16)
    for e in range(w.shape[0]):
        y[:, 2 * e * spe:2 * (e + 1) * spe], s = array_model.array(parts[:, 2 * e * spe:2 * (e + 1) * spe], w[e:e + 1], spe)
        sat += s
    return y, sat


def cli_scint_rows(pkg, sky, spec, seed, site, rate):
    """The table galileo-sdr-sim --scint makes of its file: spec = [(prn, s4, tau0_s)], one line each; the row of a line -- scint_make at
    the rate the synthesis runs at, seed = --scint-seed, stream = site << 8 | prn -- wherever a slot carries that PRN, the identity
    everywhere else."""
    rows = pkg.scint_rows({}, sky.shape[0], sky.shape[1])
    for prn, s4, tau0 in spec:
        r = dict(pkg.scint_make(s4, tau0, rate), seed=int(seed), stream=(int(site) << 8) | int(prn))
        rows[sky["prn"] == prn] = (r["seed"], r["stream"], r["node_len"], r["a_q12"], r["b_q12"], 0)
    return rows


# ---- the inputs of "echoes of the scintillated stream" (tests/test_run_compose_gpu.py, test 1): shared with the CPU test that shows that
# the model tells the orders of the two passes apart
N = 26000
FS = 2.6e6
ECHO_FADE_FIRST = 2 ** 33 + 5 * 2 * N


def echo_fade_case(pkg):
    """Six epochs (two batches of three), four satellites at distinct gains: slot 0 plain, slot 1 fades and has two echoes (delay 1;
    delay 1024 with dph != 0), slot 2 fades, slot 3 has an echo.  Returns a dict; the echo rows are those of the whole stream."""
    p = pkg.workloads.make_synthetic(n_epochs=6, n_chan=4, n_slots=16, samples_per_epoch=N, seed=91)
    g = np.full(p.shape, 128)
    g[:, :4] = (150, 420, 260, 333)
    g[3:, :4] = (170, 380, 300, 290)
    rows = pkg.scint_rows({1: dict(pkg.scint_make(0.8, 0.02, FS), node_len=1000, seed=6, stream=int(p["prn"][0, 1])),
                           2: dict(pkg.scint_make(1.0, 0.01, FS), node_len=777, seed=6, stream=int(p["prn"][0, 2]))}, 6, 16)
    echoes = [pkg.mpath_make(1 / FS, -2.0, 30.0, 0.0, FS), pkg.mpath_make(1024 / FS, -1.0, 200.0, -40.0, FS), pkg.mpath_make(5 / FS, -3.0, 10.0, 7.0, FS)]
    sof = [1, 1, 3]
    echo_rows = np.stack([pkg.mpath_rows(e, g[:, s], 0, N) for e, s in zip(echoes, sof)], axis=1)
    assert echo_rows["delay"][0].tolist() == [1, 1024, 5] and echo_rows["dph"][0, 1] != 0
    return dict(params=p, gains=g, scint_rows=rows, slot_of_echo=sof, echo_rows=echo_rows, first_sample=ECHO_FADE_FIRST)
