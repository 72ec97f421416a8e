"""The seeded noise floor on the MI355X (gal_synth_iq_convert_noise): the fused kernels bit for bit against the numpy statement of
the definition (tests/noise_model.py), in every format, at vector tails, at odd and large first_sample, cut into calls, in place,
and on a synthesised batch."""
import ctypes

import numpy as np
import pytest

import noise_model

pytestmark = pytest.mark.gpu

GAL_E_INVAL = -1
SIGMA_45 = noise_model.noise_from_cn0(45.0, 2.6e6)[1]  # sigma_q4 at 45 dB-Hz: 2267 LSB
FIRST_SAMPLES = (0, 1, 2, 3, (1 << 33) + 10, (1 << 33) + 11)  # even / odd; beyond 2^33 the counter's high word B >> 32 is not 0


def _convert(eng, x_dev, n, fmt, s, noise, first_sample=0, guard=64, n_offset=0):
    """Convert n complex samples of the device tensor x_dev from complex sample n_offset on; returns (output bytes, the guard bytes
    behind them, saturated count)."""
    import torch

    from galileo_sdr_sim_amd import iq_bytes

    out = torch.full((iq_bytes(fmt, n) + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.iq_saturated(reset=True)
    eng.iq_convert(x_dev.data_ptr() + 4 * n_offset, n, fmt, s, out.data_ptr(), noise=noise, first_sample=first_sample)
    sat = eng.iq_saturated()
    o = out.cpu().numpy()
    return o[: o.size - guard], o[o.size - guard:], sat


def _input(n, seed):
    """2 n int16 values: the spread of a synthesised batch, a tenth of them anywhere in int16, and the corners themselves."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-4100, 4101, 2 * n).astype(np.int16)
    wild = rng.random(2 * n) < 0.1
    x[wild] = rng.integers(-32768, 32768, int(wild.sum())).astype(np.int16)
    corners = np.array([32767, -32768, 32766, -32767, 0, 1, -1], dtype=np.int16)
    x[: min(corners.size, x.size)] = corners[: x.size]
    return x


@pytest.fixture(scope="module")
def eng(pkg):
    with pkg.SynthEngine(device=0) as e:
        yield e


@pytest.mark.parametrize("first_sample", FIRST_SAMPLES)
def test_formats_sizes_and_first_sample(eng, first_sample):
    """Sizes that end inside a 16-byte vector, inside ibyte's 16 values and inside ibit's 64; gain 1.5, so that both clamps fire."""
    import torch

    noise = (0x123456789ABCDEF0, 3, 98304, SIGMA_45)
    n_max = 100003
    x = _input(n_max, 17)
    xd = torch.from_numpy(x).cuda()
    clamps16 = clamps8 = 0
    for n in (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 1023, 4099, n_max):
        for fmt, s in (("ishort", 0), ("ibyte", 7), ("ibyte", 0), ("ibit", 0)):
            got, guard, sat = _convert(eng, xd, n, fmt, s, noise, first_sample)
            want, want_sat = noise_model.convert(x[: 2 * n], fmt, s, noise, first_sample)
            assert got.size == want.size and np.array_equal(got, want), (fmt, s, n, first_sample)
            assert sat == want_sat, (fmt, s, n, sat, want_sat)
            assert (guard == 0xA5).all(), (fmt, s, n)
            if n == n_max and fmt == "ishort":
                clamps16 = want_sat
            if n == n_max and fmt == "ibyte" and s == 7:
                clamps8 = want_sat
    assert 0 < clamps16 < clamps8 < 2 * n_max  # the int16 clamp fired, the +-127 clamp fired on more, and not on everything


def test_three_unequal_calls_equal_one(eng):
    """One buffer in three calls with the running first_sample = one call: from an even and from an odd start.  (The pieces start
    at multiples of 4 samples: 16-byte alignment of the input.)"""
    import torch

    noise = {"seed": 99, "stream": 1, "gain_q16": 65536, "sigma_q4": SIGMA_45}
    n = 100003
    x = _input(n, 23)
    xd = torch.from_numpy(x).cuda()
    cuts = (0, 40004, 40008, n)
    for base in (0, 7, (1 << 34) + 5):
        for fmt, s in (("ishort", 0), ("ibyte", 6), ("ibit", 0)):
            whole, _, sat = _convert(eng, xd, n, fmt, s, noise, base)
            parts, sats = [], 0
            for a, b in zip(cuts[:-1], cuts[1:]):
                got, guard, st = _convert(eng, xd, b - a, fmt, s, noise, base + a, n_offset=a)
                assert (guard == 0xA5).all()
                parts.append(got)
                sats += st
            assert np.array_equal(np.concatenate(parts), whole), (fmt, base)  # (ibit: every piece is a multiple of 4 samples = whole bytes)
            assert sats == sat
            assert np.array_equal(whole, noise_model.convert(x, fmt, s, (99, 1, 65536, SIGMA_45), base)[0])


def test_seeds_and_streams_differ(eng):
    import torch

    n = 4096
    x = _input(n, 5)
    xd = torch.from_numpy(x).cuda()
    a, _, _ = _convert(eng, xd, n, "ishort", 0, (1, 0, 65536, SIGMA_45))
    again, _, _ = _convert(eng, xd, n, "ishort", 0, (1, 0, 65536, SIGMA_45))
    other_seed, _, _ = _convert(eng, xd, n, "ishort", 0, (2, 0, 65536, SIGMA_45))
    high_seed, _, _ = _convert(eng, xd, n, "ishort", 0, (1 + (1 << 32), 0, 65536, SIGMA_45))
    other_stream, _, _ = _convert(eng, xd, n, "ishort", 0, (1, 1, 65536, SIGMA_45))
    assert np.array_equal(a, again)
    for b in (other_seed, high_seed, other_stream):
        assert np.count_nonzero(a.view(np.int16) != b.view(np.int16)) > 0.99 * 2 * n
    assert np.array_equal(high_seed, noise_model.convert(x, "ishort", 0, (1 + (1 << 32), 0, 65536, SIGMA_45))[0])


def test_unit_gain_without_noise_is_the_plain_conversion(eng):
    import torch

    n = 100003
    x = _input(n, 29)
    xd = torch.from_numpy(x).cuda()
    for fmt, s in (("ishort", 0), ("ibyte", 5), ("ibyte", 0), ("ibit", 0)):
        for first in (0, 5):
            got, guard, sat = _convert(eng, xd, n, fmt, s, (7, 0, 65536, 0), first)
            plain, _, plain_sat = _convert(eng, xd, n, fmt, s, None)
            assert np.array_equal(got, plain) and sat == plain_sat and (guard == 0xA5).all(), (fmt, s, first)
    # and a gain alone: y = round(x / 2), nothing random
    got, _, sat = _convert(eng, xd, n, "ishort", 0, (7, 0, 32768, 0))
    assert np.array_equal(got.view(np.int16), ((x.astype(np.int32) + 1) >> 1).astype(np.int16)) and sat == 0


def test_ishort_in_place(eng):
    import torch

    noise = (11, 0, 65536, SIGMA_45)
    for n, first in ((100003, 0), (100003, 9), (5, 1)):
        x = _input(n, 31)
        xd = torch.from_numpy(x).cuda()
        want, _, want_sat = _convert(eng, xd, n, "ishort", 0, noise, first)
        buf = torch.full((2 * n + 32,), 0x5A5A, dtype=torch.int16, device="cuda")
        buf[: 2 * n] = xd
        torch.cuda.synchronize()
        eng.iq_saturated(reset=True)
        eng.iq_convert(buf.data_ptr(), n, "ishort", 0, buf.data_ptr(), noise=noise, first_sample=first)
        sat = eng.iq_saturated()
        got = buf.cpu().numpy()
        assert np.array_equal(got[: 2 * n].view(np.uint8), want) and sat == want_sat
        assert (got[2 * n:] == 0x5A5A).all()


def test_bad_arguments(eng, pkg):
    import torch

    lib = pkg.load_library()
    x = torch.zeros(64, dtype=torch.int16, device="cuda")
    out = torch.zeros(256, dtype=torch.uint8, device="cuda")
    h, p, o = eng._h, x.data_ptr(), out.data_ptr()
    Noise = pkg.synth._Noise

    def call(noise, fmt, shift, src=p, dst=o, first=0, n=8):
        return lib.gal_synth_iq_convert_noise(h, src, n, first, ctypes.byref(noise) if noise is not None else None, fmt, shift, dst)

    ok = Noise(1, 0, 65536, 160, 0)
    assert call(Noise(1, 0, (1 << 20) + 1, 160, 0), 1, 5) == GAL_E_INVAL  # gain_q16 above 2^20
    assert call(Noise(1, 0, 65536, (1 << 20) + 1, 0), 1, 5) == GAL_E_INVAL  # sigma_q4 above 2^20
    assert call(Noise(1, 0, 65536, 160, 1), 1, 5) == GAL_E_INVAL  # reserved
    assert call(ok, 3, 0) == GAL_E_INVAL  # unknown format
    assert call(ok, 1, 16) == GAL_E_INVAL and call(ok, 1, -1) == GAL_E_INVAL and call(ok, 2, 3) == GAL_E_INVAL and call(ok, 0, 1) == GAL_E_INVAL
    assert call(ok, 1, 5, src=p + 2) == GAL_E_INVAL and call(ok, 1, 5, dst=o + 4) == GAL_E_INVAL  # misaligned
    assert call(ok, 1, 5, src=None) == GAL_E_INVAL and call(ok, 1, 5, dst=None) == GAL_E_INVAL
    assert call(ok, 1, 5, dst=p) == GAL_E_INVAL  # in place is for ishort only
    assert call(ok, 2, 0, dst=p) == GAL_E_INVAL
    assert call(ok, 0, 0, dst=p + 16) == GAL_E_INVAL  # ishort: exactly in place or not at all
    assert b"overlap" in lib.gal_synth_last_error()
    assert call(ok, 0, 0, first=1 << 62) == GAL_E_INVAL
    assert call(None, 1, 5, dst=p) == GAL_E_INVAL  # noise == NULL: the rules of gal_synth_iq_convert
    assert call(None, 0, 0, dst=p) == GAL_E_INVAL
    assert call(Noise(1, 0, 1 << 20, 1 << 20, 0), 1, 5) == 0  # both at their upper bound
    assert call(ok, 0, 0, dst=p) == 0 and call(ok, 0, 0, dst=o) == 0 and call(None, 1, 5) == 0
    assert call(ok, 0, 0, first=(1 << 62) - 1) == 0
    eng.iq_saturated()
    with pytest.raises(pkg.GalSynthError) as ei:
        eng.iq_convert(p, 8, "ibyte", 5, o, noise={"gain_q16": 1 << 21, "sigma_q4": 0})
    assert ei.value.code == GAL_E_INVAL


def test_convert_noise_of_the_batch_in_flight_is_refused(pkg):
    import torch

    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=4, n_slots=16, samples_per_epoch=26000, seed=12)
    with pkg.SynthEngine(samples_per_epoch=26000, n_slots=16, device=0) as e:
        e.plan(p)
        iq = torch.empty(e.output_bytes() // 2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        e.execute(iq.data_ptr())
        with pytest.raises(pkg.GalSynthError) as ei:
            e.iq_convert(iq.data_ptr(), 52000, "ishort", 0, iq.data_ptr(), noise=(1, 0, 65536, SIGMA_45))
        assert ei.value.code == -4  # GAL_E_STATE
        e.finish()
        x = iq.cpu().numpy()
        e.iq_convert(iq.data_ptr(), 52000, "ishort", 0, iq.data_ptr(), noise=(1, 0, 65536, SIGMA_45))
        e.iq_saturated()
        assert np.array_equal(iq.cpu().numpy(), noise_model.mix(x, 1, 0, 65536, SIGMA_45)[0])


def test_synthesised_batch_difference_is_the_noise(pkg):
    """Ten epochs of M-SYN12 (5.2 M values) at unit gain: nothing clips, so y - x is the model's (z S + 32768) >> 16, and its
    variance is sigma^2 within 1 % (the estimator's relative standard deviation at N >= 5 M is sqrt(2 / N) <= 6.4e-4)."""
    import torch

    params = pkg.workloads.m_syn12()[:10]
    noise = pkg.noise_from_cn0(45.0, 2.6e6)
    noise["seed"] = 2024
    first = 1199 * 260000
    with pkg.SynthEngine(device=0) as e:
        x, _, _ = e.run_host(params)
        n = x.size // 2
        assert x.size >= 5_000_000
        xd = torch.from_numpy(x).cuda()
        torch.cuda.synchronize()
        e.iq_convert(xd.data_ptr(), n, "ishort", 0, xd.data_ptr(), noise=noise, first_sample=first)
        sat = e.iq_saturated()
        y = xd.cpu().numpy()
    S = noise["sigma_q4"]
    z = np.concatenate([noise_model.noise_z(2024, 0, 2 * first + a, min(1 << 22, x.size - a)) for a in range(0, x.size, 1 << 22)])
    want = (z * S + 32768) >> 16
    peak = int(np.abs(x.astype(np.int32)).max()) + int(np.abs(want).max())
    assert peak <= 32767 and sat == 0, (peak, sat)
    d = y.astype(np.int64) - x.astype(np.int64)
    assert np.array_equal(d, want)
    sigma = S / 16.0
    var = float(np.mean(d.astype(np.float64) ** 2) - np.mean(d.astype(np.float64)) ** 2)
    print("sigma %.2f LSB, variance of y - x %.1f = %.5f sigma^2, mean %.3f" % (sigma, var, var / sigma ** 2, float(d.mean())))
    assert abs(var / sigma ** 2 - 1.0) <= 0.01
