"""The 8-bit and 1-bit IQ output formats on the MI355X: the conversion kernels against a numpy statement of their definitions
(include/galsynth.h GAL_IQ_*), the library's batches converted behind gal_synth_finish against the oracle, and the CLI's
--iq-format files against the reference program's output (tests/golden/iq_format_md5.json)."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from oracle_binding import oracle_run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "iq_format_md5.json")))
G1 = ["-l", "-6,51,100", "-t", "2022/02/20,12:00:00", "-d", "10", "-U", "1", "-b", "1", "-I", "1", "-P", "0"]
GAL_E_INVAL = -1


# ---- the definitions, in numpy ----------------------------------------------------------------------------------------------
def np_ibyte(x, s):
    """(int8) clamp((x + r) >> s, -127, 127), r = s ? 1 << (s - 1) : 0, in int32; (bytes as uint8, saturated count)."""
    r = (1 << (s - 1)) if s else 0
    v = (np.asarray(x).astype(np.int32) + r) >> s
    return np.clip(v, -127, 127).astype(np.int8).view(np.uint8), int(np.count_nonzero((v < -127) | (v > 127)))


def np_ibit(x):
    return np.packbits(np.asarray(x) > 0)


def np_format(x, fmt, s=0):
    if fmt == "ishort":
        return np.asarray(x, dtype="<i2").view(np.uint8), 0
    if fmt == "ibyte":
        return np_ibyte(x, s)
    return np_ibit(x), 0


def _convert(eng, x_dev, n, fmt, s, guard=64):
    """Convert n complex samples of the device tensor x_dev; returns (output bytes, guard bytes behind them, saturated)."""
    import torch

    from galileo_sdr_sim_amd import iq_bytes

    out = torch.full((iq_bytes(fmt, n) + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.iq_saturated(reset=True)
    eng.iq_convert(x_dev.data_ptr(), n, fmt, s, out.data_ptr())
    sat = eng.iq_saturated()  # the fence: waits for the conversion on the handle's stream, whatever its format
    o = out.cpu().numpy()
    return o[: o.size - guard], o[o.size - guard:], sat


@pytest.fixture(scope="module")
def eng(pkg):
    with pkg.SynthEngine(device=0) as e:
        yield e


# ---- kernel ---------------------------------------------------------------------------------------------------------------------
def test_every_int16_value_at_every_shift(eng):
    import torch

    x = np.random.default_rng(1).permutation(np.arange(-32768, 32768, dtype=np.int32)).astype(np.int16)
    xd = torch.from_numpy(x).cuda()
    n = x.size // 2
    for s in range(16):
        got, guard, sat = _convert(eng, xd, n, "ibyte", s)
        want, want_sat = np_ibyte(x, s)
        assert np.array_equal(got, want), s
        assert sat == want_sat, (s, sat, want_sat)
        assert (guard == 0xA5).all()
    assert np_ibyte(x, 8)[1] == 256  # (the numpy statement itself: x + 128 >= 128 * 256 or < -127 * 256, 128 values each)
    got, guard, sat = _convert(eng, xd, n, "ibit", 0)
    assert np.array_equal(got, np.packbits(x > 0)) and sat == 0 and (guard == 0xA5).all()
    got, guard, _ = _convert(eng, xd, n, "ishort", 0)
    assert np.array_equal(got, x.view(np.uint8)) and (guard == 0xA5).all()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 1023, 260000, 260001])
def test_sizes_and_tails(eng, n):
    import torch

    x = np.random.default_rng(n).integers(-9000, 9000, 2 * n).astype(np.int16)
    x[::7] = 0  # x > 0 is strict
    xd = torch.from_numpy(x).cuda()
    for fmt, s in (("ibyte", 5), ("ibyte", 0), ("ibit", 0), ("ishort", 0)):
        got, guard, sat = _convert(eng, xd, n, fmt, s)
        want, want_sat = np_format(x, fmt, s)
        assert got.size == want.size and np.array_equal(got, want), (fmt, s, n)
        assert sat == want_sat and (guard == 0xA5).all(), (fmt, s, n)


def test_bad_arguments(eng, pkg):
    import torch

    lib = pkg.load_library()
    x = torch.zeros(64, dtype=torch.int16, device="cuda")
    out = torch.zeros(256, dtype=torch.uint8, device="cuda")
    h, p, o = eng._h, x.data_ptr(), out.data_ptr()
    assert p % 16 == 0 and o % 16 == 0
    assert lib.gal_synth_iq_convert(h, p + 2, 8, 1, 5, o) == GAL_E_INVAL  # misaligned input
    assert lib.gal_synth_iq_convert(h, p + 8, 8, 2, 0, o) == GAL_E_INVAL
    assert lib.gal_synth_iq_convert(h, p, 8, 1, 5, o + 4) == GAL_E_INVAL  # misaligned output
    assert lib.gal_synth_iq_convert(h, p, 8, 3, 0, o) == GAL_E_INVAL  # unknown format
    assert lib.gal_synth_iq_convert(h, p, 8, 1, 16, o) == GAL_E_INVAL  # shift out of range
    assert lib.gal_synth_iq_convert(h, p, 8, 1, -1, o) == GAL_E_INVAL
    assert lib.gal_synth_iq_convert(h, p, 8, 2, 3, o) == GAL_E_INVAL  # a shift for ibit
    assert lib.gal_synth_iq_convert(h, None, 8, 1, 5, o) == GAL_E_INVAL
    assert lib.gal_synth_iq_convert(h, p, 8, 1, 5, p) == GAL_E_INVAL  # in place
    assert lib.gal_synth_iq_convert(h, p, 8, 2, 0, p + 16) == GAL_E_INVAL  # output inside the input
    assert lib.gal_synth_iq_convert(h, p + 16, 16, 1, 5, p) == GAL_E_INVAL  # 32 output bytes at p reach into the input at p + 16
    assert b"overlap" in lib.gal_synth_last_error()
    assert lib.gal_synth_iq_convert(h, p, 8, 2, 0, p + 32) == 0  # 32 input bytes, then 4 output bytes: adjacent, not overlapping
    assert lib.gal_synth_iq_convert(h, p, 8, 1, 5, o) == 0
    eng.iq_saturated()


def test_ibit_only_on_a_fresh_engine(pkg):
    """gal_synth_iq_saturated is the fence for every format, also on a handle that never made an ibyte conversion (whose counter
    does not exist yet); the default shift of SynthEngine.iq_convert for "ibyte" is IQ_SHIFT_DEFAULT."""
    import torch

    x = np.random.default_rng(5).integers(-5000, 5000, 2 * 1_000_003).astype(np.int16)
    xd = torch.from_numpy(x).cuda()
    n = x.size // 2
    with pkg.SynthEngine(device=0) as e:
        got, guard, sat = _convert(e, xd, n, "ibit", 0)
        assert np.array_equal(got, np_ibit(x)) and sat == 0 and (guard == 0xA5).all()
    with pkg.SynthEngine(device=0) as e:
        out = torch.zeros(pkg.iq_bytes("ibyte", n), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        e.iq_convert(xd.data_ptr(), n, "ibyte", out_ptr=out.data_ptr())
        sat = e.iq_saturated()
        want, want_sat = np_ibyte(x, pkg.synth.IQ_SHIFT_DEFAULT)
        assert np.array_equal(out.cpu().numpy(), want) and sat == want_sat


def test_convert_of_the_batch_in_flight_is_refused(pkg):
    """Between execute and finish the int16 buffer is not final (finish may synthesise it again): a conversion that reads it is
    GAL_E_STATE; behind finish the same call is accepted."""
    import torch

    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=4, n_slots=16, samples_per_epoch=26000, seed=12)
    ref, _ = oracle_run(p, 26000, 2.6e6)
    n = ref.size // 2
    with pkg.SynthEngine(samples_per_epoch=26000, n_slots=16, device=0) as e:
        e.plan(p)
        iq = torch.empty(e.output_bytes() // 2, dtype=torch.int16, device="cuda")
        out = torch.empty(pkg.iq_bytes("ibit", n), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        e.execute(iq.data_ptr())
        with pytest.raises(pkg.GalSynthError) as ei:
            e.iq_convert(iq.data_ptr(), n, "ibit", 0, out.data_ptr())
        assert ei.value.code == -4  # GAL_E_STATE
        with pytest.raises(pkg.GalSynthError) as ei:  # any part of it
            e.iq_convert(iq.data_ptr() + 4 * 26000, 16, "ibit", 0, out.data_ptr())
        assert ei.value.code == -4
        e.finish()
        e.iq_convert(iq.data_ptr(), n, "ibit", 0, out.data_ptr())
        e.iq_saturated()
        assert np.array_equal(out.cpu().numpy(), np_ibit(ref))


def test_large_conversion_past_2_31_bytes(eng):
    """600 M samples: 2.4 GB of int16 in, so byte offsets pass 2^31 (and value offsets 2^30).  Every output byte is compared with
    the definition evaluated by torch in pieces; windows at the start, across the 2^31-byte boundary and at the end with numpy."""
    import torch

    n = 600_000_000
    nv = 2 * n
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    x = torch.randint(-32768, 32768, (nv,), dtype=torch.int16, device="cuda", generator=g)
    s = 4
    piece = 1 << 27
    from galileo_sdr_sim_amd import iq_bytes

    out = torch.empty(iq_bytes("ibyte", n), dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    eng.iq_saturated(reset=True)
    eng.iq_convert(x.data_ptr(), n, "ibyte", s, out.data_ptr())
    sat = eng.iq_saturated()
    want_sat, bad = 0, 0
    for a in range(0, nv, piece):
        v = (x[a:a + piece].to(torch.int32) + (1 << (s - 1))) >> s
        want_sat += int(((v < -127) | (v > 127)).sum())
        bad += int((v.clamp(-127, 127).to(torch.int8) != out[a:a + piece]).sum())
    assert bad == 0 and sat == want_sat
    # ibit of the same input
    bits = torch.empty(iq_bytes("ibit", n), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.iq_convert(x.data_ptr(), n, "ibit", 0, bits.data_ptr())
    eng.iq_saturated()
    w = torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], dtype=torch.int32, device="cuda")
    bad = 0
    for a in range(0, nv, piece):
        b = ((x[a:a + piece] > 0).to(torch.int32).view(-1, 8) * w).sum(1).to(torch.uint8)
        bad += int((b != bits[a // 8:(a + piece) // 8]).sum())
    assert bad == 0
    for lo in (0, (1 << 30) - 4096, nv - 8192):  # value offsets: start, the 2^31-byte boundary of the input, the end
        xs = x[lo:lo + 8192].cpu().numpy()
        assert np.array_equal(out[lo:lo + 8192].cpu().numpy().view(np.uint8), np_ibyte(xs, s)[0]), lo
        assert np.array_equal(bits[lo // 8:(lo + 8192) // 8].cpu().numpy(), np_ibit(xs)), lo
    del x, out, bits
    torch.cuda.empty_cache()


# ---- library end to end ---------------------------------------------------------------------------------------------------------
def _batch_then_convert(pkg, params, n_samp, rate, n_slots, **kw):
    """plan, execute, finish, then convert on the handle's own (non-default) stream with no host sync between finish and convert;
    each format against the definition applied to the oracle's int16 of the same rows."""
    import torch

    ref, _ = oracle_run(params, n_samp, rate)
    n = ref.size // 2
    with pkg.SynthEngine(sample_rate=rate, samples_per_epoch=n_samp, n_slots=n_slots, device=0, **kw) as e:
        e.plan(params)
        iq = torch.empty(e.output_bytes() // 2, dtype=torch.int16, device="cuda")
        fmts = {"ishort": "ishort", "ibit": "ibit", "ibyte4": "ibyte", "ibyte5": "ibyte"}
        outs = {k: torch.empty(pkg.iq_bytes(f, n), dtype=torch.uint8, device="cuda") for k, f in fmts.items()}
        torch.cuda.synchronize()
        e.execute(iq.data_ptr())
        _, stats = e.finish()
        e.iq_convert(iq.data_ptr(), n, "ibyte", 5, outs["ibyte5"].data_ptr())
        e.iq_convert(iq.data_ptr(), n, "ibyte", 4, outs["ibyte4"].data_ptr())
        e.iq_convert(iq.data_ptr(), n, "ibit", 0, outs["ibit"].data_ptr())
        e.iq_convert(iq.data_ptr(), n, "ishort", 0, outs["ishort"].data_ptr())
        sat = e.iq_saturated()
        got = {k: v.cpu().numpy() for k, v in outs.items()}
    assert stats["chain_mismatch"] == 0
    assert np.array_equal(got["ishort"], ref.view(np.uint8))
    w5, s5 = np_ibyte(ref, 5)
    w4, s4 = np_ibyte(ref, 4)
    assert np.array_equal(got["ibyte5"], w5) and np.array_equal(got["ibyte4"], w4)
    assert sat == s4 + s5
    assert np.array_equal(got["ibit"], np_ibit(ref))
    return stats


def test_library_m_syn12_slice_with_repaired_groups(pkg):
    p = pkg.workloads.m_syn12()[:12]
    stats = _batch_then_convert(pkg, p, 260000, 2.6e6, 16)
    assert stats["kernel_family"] == 1 and stats["repaired_groups"] > 0, stats


def test_library_batch_synthesised_twice(pkg, monkeypatch):
    """A batch whose speculative chain is not verified in time: gal_synth_finish synthesises it again, the conversion behind it
    sees the second result (fault-injection build: one walker pass, one spoiled first guess)."""
    from fuzz_cases import random_case

    hard, n_samp, rate, chunk = random_case(pkg, np.random.default_rng([5, 35]), False)
    monkeypatch.setenv("GAL_GUESS_SPOIL", "1")
    monkeypatch.setenv("GAL_WALK_PASSES", "1")
    stats = _batch_then_convert(pkg, hard, n_samp, rate, hard.shape[1], test_hooks=True)
    assert stats["synth_runs"] == 2


def test_library_more_than_24_channels(pkg):
    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=30, n_slots=32, samples_per_epoch=26000, seed=61)
    _batch_then_convert(pkg, p, 26000, 2.6e6, 32)


# ---- CLI ------------------------------------------------------------------------------------------------------------------------
def _run(args, **kw):
    r = subprocess.run([CLI, "-e", NAV] + args, capture_output=True, timeout=600, **kw)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r


@pytest.fixture(scope="module")
def g1_ishort(tmp_path_factory):
    out = tmp_path_factory.mktemp("g1") / "g1.ishort"
    _run(G1 + ["-o", str(out)])
    x = np.fromfile(str(out), dtype="<i2")
    assert hashlib.md5(x.tobytes()).hexdigest() == GOLD["G1"]["ishort"]["md5"]
    return x


@pytest.mark.parametrize("fmt,shift,key", [("ibyte", "4", "ibyte_shift4"), ("ibyte", "5", "ibyte_shift5"), ("ibyte", None, "ibyte_shift5"),
                                           ("ibit", None, "ibit")])
def test_cli_g1_matches_the_reference_in_every_format(tmp_path, fmt, shift, key):
    out = tmp_path / ("g1." + fmt)
    r = _run(G1 + ["-o", str(out), "--iq-format", fmt] + (["--iq-shift", shift] if shift else []) + ["-v"])
    data = out.read_bytes()
    assert len(data) == GOLD["G1"][key]["bytes"] and hashlib.md5(data).hexdigest() == GOLD["G1"][key]["md5"]
    if fmt == "ibyte":
        sat = GOLD["G1"][key]["saturated"]
        assert (b"saturated" in r.stderr) and ((b"WARNING" in r.stderr) == (sat > 0))
        if sat:
            assert (b"%d of" % sat) in r.stderr


def test_cli_ibyte_sinks_agree_with_ishort(tmp_path, g1_ishort):
    want = np_ibyte(g1_ishort, 5)[0].tobytes()
    r = _run(G1 + ["-o", "-", "--iq-format", "ibyte"])
    assert r.stdout == want
    out = tmp_path / "w.ibyte"
    _run(G1 + ["-o", str(out), "--iq-format", "ibyte", "--writers", "2"])
    assert out.read_bytes() == want
    out = tmp_path / "b.ibit"
    _run(G1 + ["-o", str(out), "--iq-format", "ibit", "-B", "3"])  # batches of 3 epochs: the per-batch split in whole bytes
    assert out.read_bytes() == np_ibit(g1_ishort).tobytes()


def test_cli_sites_in_ibyte(tmp_path):
    lst = tmp_path / "sites.txt"
    lst.write_text("-6,51,100\n45,10,100\n")
    common = ["--sites", str(lst), "-t", "2022/02/20,12:00:00", "-d", "3", "-I", "1", "--gpus", "1", "--per-gpu", "2"]
    _run(common + ["-o", str(tmp_path / "a.ishort")])
    _run(common + ["-o", str(tmp_path / "a.ibyte"), "--iq-format", "ibyte", "--iq-shift", "6"])
    for k in range(2):
        x = np.fromfile(str(tmp_path / ("a.site%d.ishort" % k)), dtype="<i2")
        assert x.size == 29 * 520000
        assert (tmp_path / ("a.site%d.ibyte" % k)).read_bytes() == np_ibyte(x, 6)[0].tobytes(), k


def test_cli_shift_0_reports_saturation_on_stderr_only(g1_ishort):
    r = _run(G1 + ["-o", "-", "--iq-format", "ibyte", "--iq-shift", "0"])
    want, sat = np_ibyte(g1_ishort, 0)
    assert sat > 0 and r.stdout == want.tobytes()
    line = [ln for ln in r.stderr.decode().splitlines() if "saturated" in ln]
    assert len(line) == 1 and ("%d of %d" % (sat, g1_ishort.size)) in line[0] and "--iq-shift" in line[0]
