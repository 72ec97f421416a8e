"""The block AGC and the 2-bit quantiser without a GPU: the host functions against the numpy model (tests/agc_model.py), every refusal
of gal_synth_agc_check, the null-handle refusals of the device entry points, the byte and block counts at their edges, the model's
independence of how the stream is cut, its convergence on Gaussian input, its bounds, and the CLI's option refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import agc_model

GAL_E_INVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")


def _struct(pkg, p, reserved=0):
    a = pkg.synth._agc_struct(p)
    a.reserved = reserved
    return a


def test_symbols_and_tables(pkg):
    lib = pkg.synth.load_library()
    for name in ("gal_synth_agc_check", "gal_synth_agc_out_bytes", "gal_synth_agc_blocks", "gal_synth_agc_from_rms", "gal_synth_agc_set",
                 "gal_synth_iq_agc"):
        assert name in pkg.synth.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert pkg.synth.AGC_FORMATS == {"ishort": 0, "ibyte": 1, "i2bit": 3} and pkg.synth.GAL_IQ_I2BIT == 3
    # the plain formats do not know the 2-bit code
    assert pkg.synth.IQ_FORMATS == {"ishort": 0, "ibyte": 1, "ibit": 2}
    assert pkg.iq_bytes(3, 1000) == 0
    assert ctypes.sizeof(pkg.synth._Agc) == 32 and pkg.synth._Agc.p_init.offset == 24


def test_every_refusal_of_agc_check(pkg):
    lib = pkg.synth.load_library()
    good = agc_model.params(2600, 8, 1024 * 256, p_init=2 * 2600 * 750 * 750)
    assert lib.gal_synth_agc_check(ctypes.byref(_struct(pkg, good))) == 0
    assert lib.gal_synth_agc_check(None) == GAL_E_INVAL
    assert lib.gal_synth_agc_check(ctypes.byref(_struct(pkg, good, reserved=1))) == GAL_E_INVAL
    cases = [
        (dict(block_len=15), False), (dict(block_len=16), True), (dict(block_len=65536, window=1), True), (dict(block_len=65537, window=1), False),
        (dict(window=0), False), (dict(window=1), True), (dict(block_len=16, window=64), True), (dict(block_len=16, window=65), False),
        (dict(block_len=1024, window=64), True), (dict(block_len=1025, window=64), False), (dict(block_len=65536, window=2), False),
        (dict(block_len=4099, window=15), True), (dict(block_len=4099, window=16), False),
        (dict(target_q8=0), False), (dict(target_q8=1), True), (dict(target_q8=32767 * 256), True), (dict(target_q8=32767 * 256 + 1), False),
        (dict(gain_min_q12=0), False), (dict(gain_min_q12=5000, gain_max_q12=4999), False), (dict(gain_min_q12=5000, gain_max_q12=5000), True),
        (dict(gain_max_q12=1 << 24), True), (dict(gain_max_q12=(1 << 24) + 1), False),
        (dict(p_init=2600 << 31), True), (dict(p_init=(2600 << 31) + 1), False), (dict(p_init=0), True),
    ]
    for change, ok in cases:
        p = dict(good)
        p.update(change)
        assert agc_model.check(p) == ok, change
        rc = lib.gal_synth_agc_check(ctypes.byref(_struct(pkg, p)))
        assert rc == (0 if ok else GAL_E_INVAL), change
        if ok:
            pkg.synth.agc_check(p)
        else:
            with pytest.raises(pkg.GalSynthError):
                pkg.synth.agc_check(p)


def test_null_handle_refusals(pkg):
    lib = pkg.synth.load_library()
    a = _struct(pkg, agc_model.params(2600, 8, 1024 * 256))
    n = ctypes.c_size_t(7)
    assert lib.gal_synth_agc_set(None, ctypes.byref(a), 0) == GAL_E_INVAL
    assert lib.gal_synth_agc_set(None, None, 0) == GAL_E_INVAL
    assert lib.gal_synth_iq_agc(None, ctypes.c_void_p(4096), 100, 0, 0, ctypes.c_void_p(65536), None, ctypes.byref(n)) == GAL_E_INVAL
    assert n.value == 7


def test_out_bytes_and_blocks_over_edge_values(pkg):
    ob = pkg.synth.agc_out_bytes
    for n in (0, 1, 2, 3, 4, 5, 2599, 2600, 260000, 2 ** 41 - 1):
        assert ob("ishort", n) == 4 * n and ob("ibyte", n) == 2 * n and ob("i2bit", n) == (n + 1) // 2
        for f in agc_model.FORMATS:
            assert ob(f, n) == agc_model.out_bytes(f, n)
        assert ob(2, n) == 0 and ob(4, n) == 0 and ob(-1, n) == 0  # ibit and unknown formats
    bl = pkg.synth.agc_blocks
    for B in (16, 17, 2600, 65536):
        for P in (0, 1, B - 1, B, B + 1, 2 ** 40 + 3):
            for n in (0, 1, 2, B - 1, B, B + 1, 3 * B + 1):
                want = agc_model.blocks(P, n, B)
                if B <= 17:
                    assert want == sum(1 for g in range(P, P + n) if g % B == 0)
                assert bl(P, n, B) == want, (B, P, n)
    assert bl(0, 100, 15) == 0 and bl(0, 100, 65537) == 0 and bl(0, 100, 0) == 0 and bl(0, 100, -16) == 0
    assert bl(2 ** 64 - 1, 1, 16) == 0  # the sum wraps
    assert bl(3, 2 ** 41, 16) == 2 ** 37


def test_from_rms_rounding(pkg):
    fr = pkg.synth.agc_from_rms
    for target, init, B, W in ((1024.0, 750.0, 2600, 8), (4096.0, 2267.3, 2600, 4), (0.00390625, 0.0, 16, 1), (32767.0, 32768.0, 65536, 1),
                               (1023.998046875, 0.70710678118, 17, 3), (100.001953125, 1234.56789, 4099, 15), (2048.0, 8000.4999, 64, 64)):
        got = fr(target, init, B, W)
        assert got == agc_model.from_rms(target, init, B, W), (target, init, B, W)
        assert got["gain_min_q12"] == 1 and got["gain_max_q12"] == 1 << 24
    assert fr(1.5, 3.0, 16, 1)["target_q8"] == 384 and fr(1.5, 3.0, 16, 1)["p_init"] == 2 * 16 * 9
    # llround: ties away from zero, in the product and in the square
    assert fr(0.501953125, 0.0, 16, 1)["target_q8"] == 129  # 128.5
    assert fr(1.0, np.sqrt(2.5), 16, 1)["p_init"] == 2 * 16 * _llround_sq(np.sqrt(2.5))
    assert fr(1.0, 32768.0, 16, 1)["p_init"] == 16 << 31  # the largest p_init there is
    for bad in ((0.0, 1.0, 16, 1), (32767.5, 1.0, 16, 1), (1.0, -1.0, 16, 1), (1.0, 32768.5, 16, 1), (float("nan"), 1.0, 16, 1),
                (1.0, float("inf"), 16, 1), (1.0, 1.0, 15, 1), (1.0, 1.0, 16, 0), (1.0, 1.0, 2600, 64), (1.0, 1.0, -16, 1)):
        with pytest.raises(pkg.GalSynthError) as e:
            fr(*bad)
        assert e.value.code == GAL_E_INVAL, bad
    lib = pkg.synth.load_library()
    assert lib.gal_synth_agc_from_rms(1.0, 1.0, 16, 1, None) == GAL_E_INVAL


def _llround_sq(r):
    return agc_model._llround(np.float64(r) * np.float64(r))


def test_isqrt_and_gain_arithmetic():
    v = np.array([0, 1, 2, 3, 4, 8, 9, 15, 16, 2 ** 46, 2 ** 46 - 1, (2 ** 23 - 1) ** 2, (2 ** 23 - 1) ** 2 - 1, 10 ** 13 + 7], dtype=np.uint64)
    r = agc_model.isqrt(v)
    import math

    assert [int(k) for k in r] == [math.isqrt(int(k)) for k in v]
    p = agc_model.params(2600, 8, 1024 * 256)
    # sigma 1000 per rail: Q = 2 B W sigma^2 -> rms_q8 = 256000 -> g = 1024 x 256 x 4096 / 256000
    Q = 2 * 2600 * 8 * 1000 * 1000
    assert int(agc_model.gain_of(np.array([Q], dtype=np.uint64), p)[0]) == (1024 * 256 << 12) // 256000
    assert int(agc_model.gain_of(np.array([0], dtype=np.uint64), p)[0]) == 1 << 24  # rms 0 counts as 1: gain_max fires
    p2 = agc_model.params(2600, 8, 1024 * 256, gain_min_q12=4096, gain_max_q12=8192)
    assert [int(g) for g in agc_model.gain_of(np.array([0, Q, 400 * Q], dtype=np.uint64), p2)] == [8192, 4194, 4096]


@pytest.mark.parametrize("B,W", [(16, 1), (17, 3), (64, 64), (2600, 8)])
def test_the_model_is_cut_independent(B, W):
    rng = np.random.default_rng(7 * B + W)
    p = agc_model.params(B, W, 1024 * 256, gain_min_q12=6144, p_init=2 * B * 300 * 300)
    n = 3 * agc_model.segment(p) + 5  # full scale, zero, random full range, and five samples more
    x = agc_model.make_input(rng, n, p)
    for P in (0, 1, B - 1, 2 ** 40 + 3):
        for fmt, param in (("ishort", 0), ("ibyte", 5), ("i2bit", 1024)):
            one, gains, sat = agc_model.agc(x, p, P, fmt, param)
            assert sat > 0 and gains.size == agc_model.blocks(P, n, B)
            assert int(gains.max()) == 1 << 24 and int(gains.min()) == 6144  # both clamps fire
            even = fmt == "i2bit"
            cuts = [c + (c & 1) if even else c for c in (1, 3, B - 1, B, B + 1, 2, 510)]
            cuts = [c for c in cuts if sum(cuts) <= n]
            while sum(cuts) > n:
                cuts.pop()
            got, g2, s2 = agc_model.agc_in_cuts(x, p, cuts, P, fmt, param)
            assert np.array_equal(got, one) and np.array_equal(g2, gains) and s2 == sat, (P, fmt)
    # the gain of a block depends on the W blocks before it only: the values are those of a brute-force loop
    one, gains, _ = agc_model.agc(x, p, 0, "ishort", 0)
    xs = x.astype(np.int64).reshape(-1, 2)
    Pb = [p["p_init"]] * W + [int((xs[b * B: (b + 1) * B] ** 2).sum()) for b in range(n // B + 1)]
    for b in range(gains.size):
        ms = (sum(Pb[b: b + W]) << 16) // (2 * B * W)
        import math

        want = min(max((p["target_q8"] << 12) // max(math.isqrt(ms), 1), 6144), 1 << 24)
        assert int(gains[b]) == want, b


@pytest.mark.parametrize("sigma", [100, 1000, 8000])
def test_convergence_on_gaussian_input(sigma):
    """B = 2600, W = 16: from block W on the output rms per rail lies within 2 % of the target.  The estimator's own standard deviation
    is 1 / sqrt(2 x 2 B W) = 0.25 %, so 2 % is eight of them; the Q8 rms step adds at most 1 / (256 x 100).  The 2 % is held by the rms of
    the whole output from block W on and by every block's gain x sigma; a single block's own measured rms scatters by another 1 % (5200
    values) and is held to 2 % + 4 x 1 % on top of those two, not instead of them."""
    B, W, target = 2600, 16, 2048
    rng = np.random.default_rng(sigma)
    n = (W + 24) * B
    x = np.clip(np.rint(rng.normal(0.0, sigma, size=2 * n)), -32768, 32767).astype(np.int16)
    p = agc_model.from_rms(target, 750.0, B, W)
    out, gains, sat = agc_model.agc(x, p)
    z = out.view("<i2").astype(np.float64).reshape(-1, 2)
    assert gains.size == W + 24
    # the output from block W on, as a whole: within 2 %
    tail = z[W * B:]
    assert abs(np.sqrt((tail ** 2).mean()) / target - 1.0) < 0.02
    for b in range(W, W + 24):
        # every block: what its gain makes of the true sigma lies within the same 2 % ...
        assert abs(gains[b] / 4096.0 * sigma / target - 1.0) < 0.02, (b, gains[b])
        # ... and its own measured rms, which scatters by another 1 / sqrt(2 x 2 B) = 1 % (5200 values), within 2 % + 4 x 1 %
        rms = np.sqrt((z[b * B: (b + 1) * B] ** 2).mean())
        assert abs(rms / target - 1.0) < 0.06, (b, rms)


def test_model_bounds_at_the_largest_window():
    """All values -32768 at B x W = 65536: every block's power is 2^31 B, Q = 2^47 exactly, Q << 16 = 2^63, ms_q16 = 2^46, rms_q8 = 2^23;
    p_init at its bound gives the same in front of the stream.  Nothing wraps in uint64."""
    for B, W in ((65536, 1), (1024, 64), (16, 64)):
        p = agc_model.params(B, W, 32767 * 256, p_init=B << 31)
        n = (W + 2) * B + 3
        x = np.full(2 * n, -32768, dtype=np.int16)
        out, gains, sat = agc_model.agc(x, p)
        if B * W == 65536:
            assert W * (B << 31) == 1 << 47
        want = (32767 * 256 << 12) // (1 << 23) if B * W == 65536 else None
        if want is not None:
            assert (gains == want).all() and want == 4095
            z = out.view("<i2")
            assert (z == ((-32768 * want + 2048) >> 12)).all() and sat == 0
        got, g2, s2 = agc_model.agc_in_cuts(x, p, (1, B - 1, B + 1), 0)
        assert np.array_equal(got, out) and np.array_equal(g2, gains)
    # the largest gain on the largest value: |y g| = 2^39, and the clamp counts it
    p = agc_model.params(16, 1, 32767 * 256, p_init=0)
    x = np.full(2 * 16, -32768, dtype=np.int16)
    out, gains, sat = agc_model.agc(x, p)
    assert int(gains[0]) == 1 << 24 and sat == 32 and (out.view("<i2") == -32768).all()


def _run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120)


def test_cli_option_refusals(pkg, tmp_path):
    """All before any device work: the navigation file does not exist, so an accepted command line stops there, with another message."""
    nav = str(tmp_path / "does_not_exist.rnx")
    r = _run(["-e", nav, "--agc", "--iq-format", "ibit"])
    assert r.returncode == 1 and "--agc" in r.stderr and "ibit" in r.stderr
    r = _run(["-e", nav, "--iq-format", "i2bit", "--monitor", str(tmp_path / "m.csv")])
    assert r.returncode == 1 and "--monitor" in r.stderr and "i2bit" in r.stderr
    assert not (tmp_path / "m.csv").exists()
    for bad in (["--agc-block", "15"], ["--agc-block", "65537"], ["--agc-block", "x"], ["--agc-window", "0"], ["--agc-window", "65"],
                ["--agc-block", "2600", "--agc-window", "26"], ["--agc-block", "65536", "--agc-window", "2"]):
        r = _run(["-e", nav, "--agc"] + bad)
        assert r.returncode == 1 and "ERROR: --agc-" in r.stderr, bad
    for bad in (["--agc", "0"], ["--agc", "40000"], ["--agc=abc"], ["--agc", "--agc-init-rms", "-1"], ["--agc", "--agc-init-rms", "40000"],
                ["--agc", "--agc-log", "-"]):
        r = _run(["-e", nav] + bad)
        assert r.returncode == 1 and "ERROR: --agc" in r.stderr, bad
    for bad in (["--agc-block", "2600"], ["--agc-window", "8"], ["--agc-init-rms", "700"], ["--agc-log", str(tmp_path / "g.csv")]):
        r = _run(["-e", nav] + bad)
        assert r.returncode == 1 and "need --agc" in r.stderr, bad
    r = _run(["-e", nav, "--i2bit-threshold", "1024"])
    assert r.returncode == 1 and "--i2bit-threshold" in r.stderr
    for bad in ("0", "32768", "x"):
        r = _run(["-e", nav, "--iq-format", "i2bit", "--i2bit-threshold", bad])
        assert r.returncode == 1 and "--i2bit-threshold" in r.stderr, bad
    # accepted: the AGC's parameters are printed, and the run stops at the navigation file
    for ok, words in ((["--agc"], "target rms 2048 LSB, blocks of 2600 samples, window 8 blocks, initial rms 750 LSB"),
                      (["--agc", "3000", "--agc-block", "1024", "--agc-window", "64"], "target rms 3000 LSB, blocks of 1024 samples, window 64 blocks"),
                      (["--agc=1500.5"], "target rms 1500.5 LSB"),
                      (["--iq-format", "i2bit"], "target rms 1024 LSB"),
                      (["--iq-format", "i2bit", "--i2bit-threshold", "700"], "target rms 700 LSB"),
                      (["--iq-format", "ibyte", "--agc"], "target rms 1024 LSB"),
                      (["--iq-format", "ibyte", "--iq-shift", "3", "--agc"], "target rms 256 LSB"),
                      (["--agc", "--monitor", str(tmp_path / "m2.csv")], "target rms 2048 LSB")):
        r = _run(["-e", nav] + ok)
        assert r.returncode == 1 and "ERROR: --" not in r.stderr and words in r.stderr, (ok, r.stderr[-500:])
    # --cn0 45 with a 40 dB jammer: the automatic shift holds 4 sigma and leaves the jammer to the AGC
    r = _run(["-e", nav, "--iq-format", "ibyte", "--cn0", "45", "--jam", "40,1e5", "--agc"])
    a = _run(["-e", nav, "--iq-format", "ibyte", "--cn0", "45", "--jam", "40,1e5"])
    s_agc = int(r.stderr.split("--iq-shift ")[1].split()[0])
    s_plain = int(a.stderr.split("--iq-shift ")[1].split()[0])
    sigma = float(r.stderr.split("sigma ")[1].split()[0])
    assert 127 * (1 << s_agc) >= 4 * sigma > 127 * (1 << (s_agc - 1)) and s_plain > s_agc
    assert "target rms %d LSB" % (32 << s_agc) in r.stderr
    assert abs(float(r.stderr.split("initial rms ")[1].split()[0]) - sigma) <= 0.05  # (the noise line prints one decimal)
    # behind --fir the default initial rms is the sigma behind the filter, sigma x sqrt(sum h^2) / 16384
    r = _run(["-e", nav, "--cn0", "45", "--fir-lowpass", "1e6,25", "--agc"])
    taps = [ln for ln in r.stderr.split("\n") if ln.startswith("Front-end filter:")][0]
    h2 = sum(int(v) ** 2 for v in taps.split(":")[-1].split())
    sigma = float(r.stderr.split("sigma ")[1].split()[0])
    init = float(r.stderr.split("initial rms ")[1].split()[0])
    assert abs(init - sigma * h2 ** 0.5 / 16384.0) <= 0.05 * h2 ** 0.5 / 16384.0 + 0.01 and init < 0.95 * sigma
    h = _run(["-e"])
    for word in ("--agc [rms]", "--agc-block <n>", "--agc-window <n>", "--agc-init-rms <r>", "--agc-log <file>", "--i2bit-threshold <n>", "i2bit"):
        assert word in h.stdout, word



def test_jam_with_six_numbers_and_no_sweep_is_a_pulsed_tone(tmp_path):
    """--jam a,f,0,0,period_us,on_us: accepted as a pulsed CW tone (printed: sweep 0 samples, the pulse in samples); what is still
    refused: a sweep time of 0 with an f_hi, with four numbers, and a pulse longer than its period."""
    nav = str(tmp_path / "does_not_exist.rnx")
    r = _run(["-e", nav, "--jam", "40,1e5,0,0,50000,10000"])
    assert r.returncode == 1 and "ERROR: --jam" not in r.stderr
    assert "J/S 40 dB" in r.stderr and "sweep 0 samples, pulse 26000 of 130000 samples" in r.stderr
    same = _run(["-e", nav, "--jam", "40,1e5"])
    assert r.stderr.split("Hz .. ")[0] == same.stderr.split("Hz .. ")[0]  # the same tone: amplitude and frequency
    for bad in ("40,1e5,2e5,0,50000,10000", "40,1e5,0,0", "40,1e5,2e5,0", "40,1e5,0,0,50000", "40,1e5,0,0,10000,50000", "40,1e5,0,-1,50000,10000"):
        r = _run(["-e", nav, "--jam", bad])
        assert r.returncode == 1 and "ERROR: --jam" in r.stderr, bad
    r = _run(["-e", nav, "--jam", "25,-1e6,1e6,100,1000,200"])  # a pulsed chirp: as before
    assert r.returncode == 1 and "ERROR: --jam" not in r.stderr and "sweep 260 samples, pulse 520 of 2600 samples" in r.stderr
