"""The correlator bank on the MI355X (gal_synth_correlate): the kernel's int64 sums against the numpy statement of the definition
(tests/corr_model.py), exactly, in the three formats, on batches the engine synthesised; the refusals that need a handle; and the
physical check -- a single satellite under the noise floor of gal_synth_noise_from_cn0 comes out of gal_corr_cn0 at the C/N0 asked
for, and 1-bit and 8-bit quantisation cost what the textbook says."""
import ctypes
import math

import numpy as np
import pytest

import corr_model

pytestmark = pytest.mark.gpu

GAL_E_INVAL, GAL_E_STATE = -1, -4
FS = 2.6e6
BIN_250HZ = round(250.0 / FS * 2 ** 32)
FORMATS = (("ishort", 0), ("ibyte", 5), ("ibit", 0))


@pytest.fixture(scope="module")
def eng(pkg):
    with pkg.SynthEngine(device=0) as e:
        yield e


@pytest.fixture(scope="module")
def batch12(pkg, eng):
    """Two epochs of the 12-channel synthetic record set, synthesised by the engine, in the three formats: device tensors + host bytes."""
    import torch

    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=12, n_slots=16, seed=41)
    x, _, _ = eng.run_host(p)
    n = x.size // 2
    xd = torch.from_numpy(x).cuda()
    bufs = {}
    for fmt, s in FORMATS:
        out = torch.zeros(pkg.iq_bytes(fmt, n) + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        eng.iq_convert(xd.data_ptr(), n, fmt, s, out.data_ptr())
        eng.iq_saturated()
        bufs[fmt] = (out, out.cpu().numpy())
    return p, n, bufs


def _check(pkg, eng, bufs, fmt, n_samples, reqs, tables, byte_offset=0, sample_offset=0):
    dev, host = bufs[fmt]
    got = eng.correlate(dev.data_ptr() + byte_offset, fmt, n_samples, reqs)
    v = corr_model.values(host[byte_offset:], fmt, n_samples)
    for r, (q, g) in enumerate(zip(reqs, got)):
        want = corr_model.correlate(v, q, tables)
        assert g.shape == want.shape and g.dtype == np.int64
        assert np.array_equal(g, want), (fmt, r, q, int(np.count_nonzero(g != want)))
    return got


@pytest.mark.parametrize("fmt", [f for f, _ in FORMATS])
def test_grids_on_a_12_channel_batch(pkg, eng, batch12, fmt):
    """1 x 1, 3 x 3 with a negative delay0, a wide step, max_periods smaller than the periods present (100 003 samples hold 10), and
    an n_samples that is no multiple of the 2048-sample tile -- per channel of the plan, all 12 in one call."""
    p, n, bufs = batch12
    T = pkg.tables()
    reqs = []
    for s in range(12):
        base = pkg.corr_from_epoch(p[0, s], FS, 0)
        shape = ({"max_periods": 4}, {"max_periods": 3, "delay0": -1, "n_delay": 3, "dopp0": -BIN_250HZ, "dopp_step": BIN_250HZ, "n_dopp": 3},
                 {"max_periods": 12, "delay0": -5000, "delay_step": 2046, "n_delay": 5, "dopp0": 7, "dopp_step": -3, "n_dopp": 2})[s % 3]
        reqs.append(dict(base, **shape))
    got = _check(pkg, eng, bufs, fmt, 100003, reqs, T)
    assert not got[2][10:].any() and got[2][9].any()  # periods the buffer does not reach stay 0
    if fmt == "ishort":  # the planned satellite is there: in the 3 x 3 grid of channel 1 the prompt cell is the strongest, period 1
        g = (got[1][1].astype(np.float64) ** 2).sum(axis=2)
        assert np.unravel_index(int(np.argmax(g)), g.shape) == (1, 1)


@pytest.mark.parametrize("fmt", [f for f, _ in FORMATS])
def test_full_code_search(pkg, eng, batch12, fmt):
    """8184 delays x 1 bin: every half chip of the code, two periods; the peak is the planned delay."""
    p, n, bufs = batch12
    T = pkg.tables()
    q = pkg.corr_from_epoch(p[0, 3], FS, 0, max_periods=2, n_delay=8184)
    got = _check(pkg, eng, bufs, fmt, 12001, [q], T)[0]
    power = (got[1, 0].astype(np.float64) ** 2).sum(axis=1)
    assert int(np.argmax(power)) == 0


@pytest.mark.parametrize("fmt", [f for f, _ in FORMATS])
def test_period_boundary_at_a_tile_edge(pkg, eng, batch12, fmt):
    """code_dph = 3/4 half chip per sample and code_ph0 chosen so that period 1 starts at sample 2047, 2048 (the first of the second
    tile) and 2049; and a buffer that starts 16 bytes into the allocation."""
    p, n, bufs = batch12
    T = pkg.tables()
    dph = 3 << 30
    reqs = []
    for first in (2047, 2048, 2049, 4096):
        reqs.append({"prn": 5, "code_ph0": corr_model.L - first * dph, "code_dph": dph, "carr_ph0": 12345, "carr_dph": -BIN_250HZ * 7, "max_periods": 2,
                     "delay0": -2, "n_delay": 5, "dopp0": -9, "dopp_step": 9, "n_dopp": 3})
    _check(pkg, eng, bufs, fmt, 8190, reqs, T)
    _check(pkg, eng, bufs, fmt, 4097, reqs, T, byte_offset=16)
    # a standing code (code_dph 0: every sample in period 0) and a single sample
    still = {"prn": 50, "code_ph0": (8183 << 32) + 17, "code_dph": 0, "max_periods": 1, "n_delay": 2, "delay0": 8183}
    _check(pkg, eng, bufs, fmt, 5000, [still], T)
    _check(pkg, eng, bufs, fmt, 1, [still], T)


def test_64_requests_in_one_call(pkg, eng, batch12):
    p, n, bufs = batch12
    T = pkg.tables()
    reqs = []
    for r in range(64):
        base = pkg.corr_from_epoch(p[0, r % 12], FS, 0)
        reqs.append(dict(base, max_periods=1 + r % 3, delay0=-(r % 4), n_delay=1 + r % 5, dopp0=-(r % 2) * BIN_250HZ, dopp_step=BIN_250HZ, n_dopp=1 + r % 3))
    for fmt, _ in FORMATS:
        _check(pkg, eng, bufs, fmt, 30011, reqs, T)


def test_refusals(pkg, eng, batch12):
    import torch

    lib = pkg.load_library()
    p, n, bufs = batch12
    Req = pkg.synth._CorrReq
    buf = bufs["ishort"][0].data_ptr()
    out = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
    o = out.data_ptr()
    torch.cuda.synchronize()
    ok = dict(prn=1, max_periods=2, code_ph0=0, code_dph=1 << 31, carr_ph0=0, carr_dph=0, delay0=0, delay_step=1, n_delay=4, dopp0=0, dopp_step=1, n_dopp=2)

    def call(q=None, src=buf, dst=o, fmt=0, n_samples=10000, n_req=1, reqs=None):
        arr = reqs if reqs is not None else (Req * 1)(Req(**(q or ok)))
        return lib.gal_synth_correlate(eng._h, src, fmt, n_samples, arr, n_req, dst)

    assert call() == 0
    assert call(src=buf + 4) == GAL_E_INVAL and call(dst=o + 8) == GAL_E_INVAL  # 16-byte alignment
    assert call(src=None) == GAL_E_INVAL and call(dst=None) == GAL_E_INVAL
    assert lib.gal_synth_correlate(eng._h, buf, 0, 10000, None, 1, o) == GAL_E_INVAL
    assert call(fmt=3) == GAL_E_INVAL and call(fmt=-1) == GAL_E_INVAL
    assert call(n_samples=0) == GAL_E_INVAL
    assert call(n_req=0) == GAL_E_INVAL
    many = (Req * 65)(*[Req(**ok) for _ in range(65)])
    assert call(reqs=many, n_req=65) == GAL_E_INVAL and call(reqs=many, n_req=64) == 0
    for bad in (dict(n_delay=8185), dict(n_delay=0), dict(n_dopp=65), dict(n_dopp=0), dict(max_periods=1025), dict(max_periods=0), dict(prn=0),
                dict(prn=51), dict(delay_step=0), dict(code_ph0=corr_model.L), dict(code_dph=(1 << 32) + 1)):
        assert call(dict(ok, **bad)) == GAL_E_INVAL, bad
    assert call(dict(ok, max_periods=1024, n_dopp=64, n_delay=8184)) == GAL_E_INVAL  # 17 GB of sums
    assert b"bytes of output" in lib.gal_synth_last_error()
    # output inside the buffer, and the buffer's tail inside the output
    assert call(dst=buf + 1024) == GAL_E_INVAL
    assert b"overlap" in lib.gal_synth_last_error()
    assert call(src=o + 256, dst=o, n_samples=64) == GAL_E_INVAL
    eng.iq_saturated()
    with pytest.raises(pkg.GalSynthError) as ei:
        eng.correlate(buf, "ishort", 1000, [dict(ok, n_delay=9000)])
    assert ei.value.code == GAL_E_INVAL


def test_buffer_of_the_batch_in_flight_is_refused(pkg):
    import torch

    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=4, n_slots=16, samples_per_epoch=26000, seed=12)
    q = pkg.corr_from_epoch(p[0, 0], FS, 0, max_periods=2, n_delay=3, delay0=-1)
    with pkg.SynthEngine(samples_per_epoch=26000, n_slots=16, device=0) as e:
        e.plan(p)
        iq = torch.empty(e.output_bytes() // 2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        e.execute(iq.data_ptr())
        with pytest.raises(pkg.GalSynthError) as ei:
            e.correlate(iq.data_ptr(), "ishort", 26000, [q])
        assert ei.value.code == GAL_E_STATE
        e.finish()
        got = e.correlate(iq.data_ptr(), "ishort", 26000, q)  # (a single dict: a single array)
        want = corr_model.correlate(corr_model.values(iq.cpu().numpy(), "ishort", 26000), q, pkg.tables())
        assert np.array_equal(got, want)


def _tolerance_db(cn0_dbhz, M):
    """Three standard errors of gal_corr_cn0 in dB.  Per whole period the prompt holds signal + noise with the per-period power ratio
    SNR = (Pp - Pn) / Pn = (C/N0) T / 2 (T = 4 ms), the far tap noise alone.  Over M periods the mean Pn has the
    relative standard error 1 / sqrt(M) (an exponential-like power: standard deviation = mean), the signal part Pp - Pn has
    sqrt((2 SNR + 1) / M) / SNR (cross term 2 SNR, noise 1, in units of Pn^2).  In quadrature, as dB: (10 / ln 10) x that."""
    snr = 10 ** (cn0_dbhz / 10) * 0.004 / 2
    se = math.sqrt(1.0 / M + (2 * snr + 1) / (M * snr * snr))
    return 3 * 10 / math.log(10) * se


def test_cn0_of_a_single_satellite_and_quantisation_loss(pkg, eng):
    """One satellite (no other raises the floor), ten epochs = 1 s in one batch, the noise floor of gal_synth_noise_from_cn0 at 45 and
    35 dB-Hz, despread with the replica of the first record over max_periods = 250: M = 248 whole periods.

    ishort: gal_corr_cn0 must give the C/N0 asked for within three standard errors of the estimator (_tolerance_db): relative standard
    error sqrt(1 / M + (2 SNR + 1) / (M SNR^2)), SNR = (C/N0) x 4 ms / 2 = 63.2 and 6.32 -> 3 x 0.280 = 0.84 dB at 45 dB-Hz,
    3 x 0.319 = 0.96 dB at 35 dB-Hz.

    ibit: below the ishort figure, by at most the textbook 1.96 dB (2 / pi: a hard limiter at low SNR per sample, here -19 and -29 dB)
    plus the same three standard errors.  ibyte at the CLI's own shift (the smallest with 127 x 2^s >= 4 sigma) loses
    10 log10(1 + 2^2s / (12 sigma^2)) = 0.001 dB, three orders below the instrument's standard error: its sign cannot be observed, so
    that figure is printed and bounded only, and the assertion of the sign is made at the first shift whose step reaches sigma
    (2^s >= sigma: s = 12 at both levels, textbook loss 1.04 dB and 0.45 dB), where the loss is 20 times the error of the DIFFERENCE
    (both estimates see the same noise).  Measured figures: DESIGN.md section 12."""
    import torch

    p = pkg.workloads.make_synthetic(n_epochs=10, n_chan=1, n_slots=16, prns=[11], seed=77)
    x, _, _ = eng.run_host(p)
    n = x.size // 2
    xd = torch.from_numpy(x).cuda()
    q = pkg.corr_from_epoch(p[0, 0], FS, 0, max_periods=250, delay0=0, delay_step=2046, n_delay=2)
    M = 248
    for cn0 in (45.0, 35.0):
        unit = pkg.noise_from_cn0(cn0, FS)
        gain = 1.0
        while (5.0 * unit["sigma_q4"] / 16.0 + 4100.0) * gain > 32767.0:  # the CLI's rule: 5 sigma + the largest signal inside int16
            gain *= 0.5
        noise = pkg.noise_from_cn0(cn0, FS, gain)
        noise["seed"] = 20241008
        sigma = noise["sigma_q4"] / 16.0
        s_cli = 0
        while 127.0 * (1 << s_cli) < 4.0 * sigma:
            s_cli += 1
        s_coarse = 0
        while (1 << s_coarse) < sigma:
            s_coarse += 1
        est = {}
        for name, fmt, s in (("ishort", "ishort", 0), ("ibyte", "ibyte", s_cli), ("ibyte_coarse", "ibyte", s_coarse), ("ibit", "ibit", 0)):
            out = torch.zeros(pkg.iq_bytes(fmt, n), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            eng.iq_saturated(reset=True)
            eng.iq_convert(xd.data_ptr(), n, fmt, s, out.data_ptr(), noise=noise, first_sample=0)
            sat = eng.iq_saturated()
            sums = eng.correlate(out.data_ptr(), fmt, n, q)
            assert sums[249].any() and sums[1].any()
            est[name] = pkg.corr_cn0(sums, q, 0, 1, 0, FS) + (s, sat)
        tol = _tolerance_db(cn0, M)
        loss = {k: est["ishort"][0] - est[k][0] for k in est}
        book = {"ibit": 10 * math.log10(math.pi / 2), "ibyte": 10 * math.log10(1 + 4.0 ** s_cli / (12 * sigma ** 2)),
                "ibyte_coarse": 10 * math.log10(1 + 4.0 ** s_coarse / (12 * sigma ** 2))}
        print("asked %.0f dB-Hz, gain %g, sigma %.1f LSB, tolerance %.3f dB" % (cn0, gain, sigma, tol))
        for k in est:
            print("  %-12s shift %2d: C/N0 %.3f dB-Hz, Pp / Pn %.3f, loss %.4f dB (textbook %.4f), saturated %d" %
                  (k, est[k][2], est[k][0], est[k][1], loss[k], book.get(k, 0.0), est[k][3]))
        assert abs(est["ishort"][0] - cn0) <= tol, (cn0, est["ishort"], tol)
        assert 0.0 < loss["ibit"] <= book["ibit"] + tol
        assert 0.0 < loss["ibyte_coarse"] <= book["ibyte_coarse"] + tol
        assert abs(loss["ibyte"]) <= book["ibyte"] + tol


# ---- full-scale input, every lane split of the delays, the largest code rate -------------------------------------------------------
N_OWN = 8190  # samples of the buffers below: four tiles of 2048 less 2
OUT_GUARD = 16  # int64 behind the sums that the kernel must leave alone


def _own(host_bytes):
    """A device buffer of the tests' own with 64 spare bytes behind it: (device tensor, host bytes), as batch12's."""
    import torch

    host = np.concatenate([np.ascontiguousarray(host_bytes).view(np.uint8).ravel(), np.zeros(64, dtype=np.uint8)])
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return dev, host


@pytest.fixture(scope="module")
def own():
    """Buffers no synthesis would write: ishort all (-32768, -32768), random full-range, and (-32768, 32767), (32767, -32768) in turn;
    ibyte of -128, -127 and 127 only, its first 300 samples all -128; ibit of random bytes."""
    rng = np.random.default_rng(812)
    j = np.arange(2 * N_OWN)
    byte = rng.choice(np.array([-128, -127, 127], dtype=np.int8), size=2 * N_OWN)
    byte[:600] = -128
    return {
        "ishort_min": ("ishort", _own(np.full(2 * N_OWN, -32768, dtype=np.int16))),
        "ishort_random": ("ishort", _own(rng.integers(-32768, 32768, size=2 * N_OWN, dtype=np.int16))),
        "ishort_alternating": ("ishort", _own(np.where((j // 2 + j) % 2 == 0, -32768, 32767).astype(np.int16))),
        "ibyte_edges": ("ibyte", _own(byte)),
        "ibit_random": ("ibit", _own(rng.integers(0, 256, size=(N_OWN + 3) // 4, dtype=np.uint8))),
    }


def _check_guarded(pkg, eng, own, name, n_samples, reqs, tables):
    """As _check, with the sums written to a device buffer of the test's own that is OUT_GUARD int64 longer than they are."""
    import torch

    fmt, (dev, host) = own[name]
    sizes = [pkg.corr_out_bytes(q) // 8 for q in reqs]
    out = torch.full((sum(sizes) + OUT_GUARD,), 0x5a5a5a5a5a5a, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert eng.correlate(dev.data_ptr(), fmt, n_samples, reqs, out_ptr=out.data_ptr()) is None
    eng.iq_saturated()  # the fence
    got = out.cpu().numpy()
    assert (got[sum(sizes):] == 0x5a5a5a5a5a5a).all(), "the kernel wrote behind the sums"
    v = corr_model.values(host, fmt, n_samples)
    off, res = 0, []
    for r, (q, size) in enumerate(zip(reqs, sizes)):
        want = corr_model.correlate(v, q, tables)
        g = got[off:off + size].reshape(want.shape)
        assert np.array_equal(g, want), (name, r, q, int(np.count_nonzero(g != want)))
        res.append(g)
        off += size
    return res


def _loudest_carrier_phase(tables):
    """carr_ph0 of the carrier table's entry with the largest |cos| + |sin| among those where the two have one sign: there the
    (-32768, -32768) sample gives the largest |Re| of x conj(w) there is, 32768 (|cos| + |sin|)."""
    c, s = tables["cos512"].astype(np.int64), tables["sin512"].astype(np.int64)
    i = int(np.argmax(np.abs(c + s)))
    assert abs(c[i] + s[i]) == (np.abs(c) + np.abs(s)).max()
    return i << 23, int(abs(c[i] + s[i]))


def _moving(first, dph=3 << 30, **grid):
    """The request of test_period_boundary_at_a_tile_edge: period 1 starts at sample `first`."""
    q = {"prn": 5, "code_ph0": corr_model.L - first * dph, "code_dph": dph, "carr_ph0": 12345, "carr_dph": -BIN_250HZ * 7, "max_periods": 2,
         "delay0": -2, "n_delay": 5, "dopp0": -9, "dopp_step": 9, "n_dopp": 3}
    q.update(grid)
    return q


@pytest.mark.parametrize("name", ["ishort_min", "ishort_random", "ishort_alternating", "ibyte_edges"])
def test_full_scale_input(pkg, eng, own, name):
    """int16 at its ends (and int8 at -128, which the ibyte writer never makes): a standing code and a standing carrier at the table's
    loudest phase, so that every sample adds 32768 x (|cos| + |sin|) = 11.6 M with one sign and 128 samples fill an int32
    accumulator to more than 2^30 (tests/test_iq_corr_cpu.py has the arithmetic); and the ordinary moving request.  A lane walks
    128 consecutive samples only where its segment of the tile is that long: with 2 delays the 256 lanes split the tile into 128
    segments of 16 samples, so the standing request is also made with 17 delays (8 segments of 256 samples: two int32 accumulations
    each) and with 129 (one delay per lane, the whole tile of 2048 samples: sixteen)."""
    T = pkg.tables()
    ph, amp = _loudest_carrier_phase(T)
    assert 2 ** 30 < 128 * 32768 * amp < 2 ** 31
    standing = {"prn": 50, "code_ph0": (8183 << 32) + 17, "code_dph": 0, "carr_ph0": ph, "carr_dph": 0, "dopp0": 0, "max_periods": 1, "n_delay": 2,
                "delay0": 8183}
    reqs = [standing, _moving(3000), dict(standing, carr_ph0=ph ^ (1 << 31), prn=1, delay0=0), dict(standing, n_delay=17),
            dict(standing, n_delay=129, delay_step=63)]
    assert [(2048 * kd // 256) for kd, _, _ in map(_lanes_per_segment, (2, 17, 129))] == [16, 256, 2048]  # samples per segment
    got = _check_guarded(pkg, eng, own, name, N_OWN, reqs, T)
    _check_guarded(pkg, eng, own, name, 4097, reqs, T)
    if name == "ishort_min":  # the sums are what the bound speaks of: every sample at full weight, one sign
        assert abs(int(got[0][0, 0, 0, 0])) == N_OWN * 32768 * amp > 2 ** 36


DELAY_COUNTS = (9, 16, 17, 33, 64, 100, 128, 129, 256, 257, 300)


def _lanes_per_segment(n_delay):
    """galk_launch_corr (csrc/iq_corr.hip), restated: kd = the power of two >= n_delay, at most the block's 256 lanes; the block's
    lanes are 256 / kd segments of the tile per delay, and it takes ceil(n_delay / kd) trips over the delays."""
    kd = 1
    while kd < n_delay and kd < 256:
        kd <<= 1
    return kd, 256 // kd, -(-n_delay // kd)


@pytest.mark.parametrize("n_delay", DELAY_COUNTS)
def test_every_split_of_the_lanes(pkg, eng, own, n_delay):
    """16, 8, 4 and 2 segments of the tile per delay (summed through LDS, the lanes beyond kd idle behind it), full and partly
    filled, one delay per lane at the switch (129), and a second trip over the delays that only some lanes take (257, 300) -- with a
    period boundary inside the second tile (sample 3000), where max_periods = 2 goes on into period 1 and max_periods = 1 ends the
    tile there."""
    shapes = [_lanes_per_segment(k) for k in DELAY_COUNTS]
    assert {kd for kd, _, _ in shapes} == {16, 32, 64, 128, 256} and {nseg for _, nseg, _ in shapes} == {16, 8, 4, 2, 1}
    assert [s for s in shapes if s[2] > 1] == [(256, 1, 2), (256, 1, 2)] and 257 % 256 and 300 % 256  # a partial second trip
    assert _lanes_per_segment(128) == (128, 2, 1) and _lanes_per_segment(129) == (256, 1, 1) and _lanes_per_segment(256) == (256, 1, 1)
    assert {_lanes_per_segment(k)[0] for k in (1, 3, 5, 8184)} == {1, 4, 8, 256}  # what the tests above reach
    assert 2048 < 3000 < 4096
    T = pkg.tables()
    reqs = [_moving(3000, n_delay=n_delay, n_dopp=2, max_periods=2), _moving(3000, n_delay=n_delay, n_dopp=2, max_periods=1)]
    got = _check_guarded(pkg, eng, own, "ishort_random", N_OWN, reqs, T)
    assert got[0][1].any() and np.array_equal(got[0][0], got[1][0])


@pytest.mark.parametrize("name", ["ishort_random", "ibyte_edges", "ibit_random"])
def test_one_half_chip_per_sample(pkg, eng, own, name):
    """code_dph = 2^32, the largest admitted: a tile of 2048 samples spans exactly 2048 half chips.  Period 1 starts at sample 2047,
    2048 (the first of the second tile) and 2049; and at sample 1, so that period 2 starts at 8185, inside the last tile."""
    T = pkg.tables()
    dph = 1 << 32
    reqs = [_moving(first, dph=dph, n_delay=5) for first in (2047, 2048, 2049)] + [_moving(1, dph=dph, n_delay=5, max_periods=3)]
    assert all(q["code_dph"] == 1 << 32 and 0 <= q["code_ph0"] < corr_model.L for q in reqs)
    got = _check_guarded(pkg, eng, own, name, N_OWN, reqs, T)
    assert got[3][2].any()  # five samples of period 2
    _check_guarded(pkg, eng, own, name, 2049, reqs[:3], T)
