"""tests/compose_model.py against the models it composes, without a GPU: identity rows are the weighted sum, unity without fading and
echoes is the sum of the parts, a batch cut in two with the history lines carried is the single call -- and the composed expectation of
"echoes of the scintillated stream" (tests/test_run_compose_gpu.py) differs from every wrong order of the two passes, so that the GPU
test can tell them apart."""
import numpy as np
import pytest

import compose_model
import gain_model
import mpath_model
from compose_model import N, FS
from oracle_binding import oracle_run


@pytest.fixture(scope="module")
def case(pkg):
    """The inputs of the GPU test, the oracle's stream of every slot alone over the six epochs, and the cosine table."""
    c = compose_model.echo_fade_case(pkg)
    alone = np.stack([oracle_run(gain_model.slot_alone(c["params"], s), N, FS)[0] for s in range(4)])
    alone.setflags(write=False)
    return c, alone, pkg.tables()["cos1024"]


def _model(c, alone, cos, a, b, lines=None, **change):
    k = dict(c, **change)
    rows = k["scint_rows"]
    return compose_model.run_model(alone[:, 2 * a * N:2 * b * N], k["params"][a:b], k["gains"][a:b], None if rows is None else rows[a:b],
                                   k["first_sample"] + a * N, N, lines, k["slot_of_echo"], k["echo_rows"][a:b], cos)


def test_identity_rows_are_the_weighted_sum(pkg, case):
    c, alone, cos = case
    ident = pkg.scint_rows({}, 6, 16)
    want, want_sat = gain_model.wsum(alone, c["gains"][:, :4], N)
    for rows in (ident, None):
        got, sat = _model(c, alone, cos, 0, 6, scint_rows=rows, slot_of_echo=[], echo_rows=c["echo_rows"][:, :0])
        assert np.array_equal(got, want) and sat == want_sat == 0
    # an idle epoch counts with the gain 0, whatever the gain table says
    p = c["params"].copy()
    p["prn"][2, 0] = 0
    g = c["gains"].copy()
    g[2, 0] = 0
    want, _ = gain_model.wsum(alone, g[:, :4], N)
    got, _ = _model(c, alone, cos, 0, 6, params=p, scint_rows=ident, slot_of_echo=[], echo_rows=c["echo_rows"][:, :0])
    assert np.array_equal(got, want)


def test_unity_without_fading_and_echoes_is_the_sum_of_the_parts(pkg, case):
    c, alone, cos = case
    got, sat = _model(c, alone, cos, 0, 6, gains=np.full(c["gains"].shape, 128), scint_rows=None, slot_of_echo=[], echo_rows=c["echo_rows"][:, :0])
    assert sat == 0 and np.array_equal(got.astype(np.int64), alone.astype(np.int64).sum(axis=0))
    # ... and a group's sum that could leave int16 is refused
    with pytest.raises(AssertionError):
        compose_model.slots_fit_int16(np.full((3, 8), 11000, dtype=np.int16), set())
    compose_model.slots_fit_int16(np.full((3, 8), 11000, dtype=np.int16), {2})


def test_a_batch_cut_in_two_with_the_lines_carried_is_the_single_call(case):
    c, alone, cos = case
    whole, whole_sat = _model(c, alone, cos, 0, 6)
    lines = mpath_model.Lines(cos)
    a, sat_a = _model(c, alone, cos, 0, 3, lines)
    b, sat_b = _model(c, alone, cos, 3, 6, lines)
    assert np.array_equal(np.concatenate([a, b]), whole) and sat_a + sat_b == whole_sat == 0
    # without the lines the second half starts a stream: the echo of delay 1024 has nothing to delay in its first 1024 samples
    b0, _ = _model(c, alone, cos, 3, 6)
    bad = np.flatnonzero(b0 != b)
    assert bad.size > 1000 and bad.max() < 2 * 1024


def test_the_model_tells_the_order_of_scintillation_and_echoes_apart(pkg, case):
    """Three ways of having the two passes in the wrong order, each with other bytes than the model's: the scintillation behind the
    echo pass (it turns the parts once the sum has read them: no fading in the output at all); the echoes of the un-faded stream beside
    the faded direct signal; and a history line that keeps the un-faded samples, which shows in the first 1024 samples of the second
    batch alone."""
    c, alone, cos = case
    lines = mpath_model.Lines(cos)
    a, _ = _model(c, alone, cos, 0, 3, lines)
    b, _ = _model(c, alone, cos, 3, 6, lines)
    # 1. no fading
    plain, _ = _model(c, alone, cos, 0, 6, scint_rows=None)
    assert np.count_nonzero(plain != np.concatenate([a, b])) > 0.5 * plain.size
    # 2. the direct signals faded, the echoes those of the un-faded streams: extra parts at gain 0 carry them
    faded, _ = compose_model.fade(alone, c["scint_rows"], c["first_sample"], N)
    g = np.concatenate([c["gains"][:, :4], np.zeros((6, 2), dtype=np.int64)], axis=1)
    wrong, _, _ = mpath_model.mpath(np.concatenate([faded, alone[[1, 3]]]), g, N, [4, 4, 5], c["echo_rows"], cos)
    right, _, _ = mpath_model.mpath(faded, g[:, :4], N, c["slot_of_echo"], c["echo_rows"], cos)
    assert np.array_equal(right, np.concatenate([a, b]))
    assert np.count_nonzero(wrong != right) > 0.5 * right.size
    # 3. the line of slot 1 holds what the synthesis wrote, not what the scintillation made of it
    stale = mpath_model.Lines(cos)
    _model(c, alone, cos, 0, 3, stale)
    assert np.array_equal(stale.lines[1], faded[1, 2 * 3 * N - 2048:2 * 3 * N]) and not np.array_equal(stale.lines[1], alone[1, 2 * 3 * N - 2048:2 * 3 * N])
    stale.lines[1] = alone[1, 2 * 3 * N - 2048:2 * 3 * N]
    b_stale, _ = _model(c, alone, cos, 3, 6, stale)
    bad = np.flatnonzero(b_stale != b)
    assert bad.size > 1000 and bad.max() < 2 * 1024
