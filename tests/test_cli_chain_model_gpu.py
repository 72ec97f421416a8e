"""galileo-sdr-sim's output chain on the MI355X against computed bytes: for every recorded case of tools/cli_golden.py whose chain has
more than one stage (or one stage that no model-based CLI test runs at that format), and for the reflector case, the IQ file at -B 1
and at -B 3 is tests/chain_model.py over the command's own front stream -- the same command with its synthesis options only, as ishort
at the synthesis rate --, every byte; so are the gains of --agc-log and the saturated count the command prints.  The synthesis-path CLI
tests hold the front streams against models and wrappers; this one is about what run_chain does behind them: the order of the stages,
the fused mix, first_sample from batch to batch, the buffer each stage reads, the state carried across batches and output slots.

The parameters come from the option values through the library's own helpers (noise_from_cn0, interf_make, osc_make, fir_lowpass,
agc_from_rms), as in the per-stage CLI tests, and from the decisions the command prints: the signal gain, the shift, the seeds and
streams, the decimator's taps, the AGC line.

--oversample 2: the command writes nothing at the high rate, so the front stream is put together from two runs whose decimator is a
single tap 16384, an exact pick (tests/test_oversample_cli.py): taps "16384" keep x[2m], taps "0 16384" keep x[2m - 1].  The last
sample x[2N - 1] appears in neither and is taken as 0: no kept output reads it (output m reads x[2m - k], k >= 0)."""
import os
import re
import sys
import time

import numpy as np
import pytest

import chain_model
from test_iq_agc_cli import _agc_line, _read_log
from test_iq_firdec_cli import _printed_taps

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import cli_golden  # noqa: E402  (the scenario, the cases and the runner)

FS = 2.6e6
FC = 1575.42e6
EPOCHS, N = 4, 260000  # CHAIN_SCEN: 0.5 s
PICKS = {"pick0.txt": "16384\n", "pick1.txt": "0\n16384\n"}
# case -> the command's synthesis options: what makes the front stream
FRONT = {
    "cn0_ibyte_fused": [],
    "osc_ishort": [],
    "cn0_jam_osc_ibyte": [],
    "cn0_agc_log_ishort": [],
    "jam_osc_i2bit": [],
    "cn0_osc_fir_agc_monitor_ibyte": [],
    "osr_cn0_osc_mpath_power_ibyte": ["--oversample", "2", "--multipath", "mp.txt", "--power-model"],
    "array_scint_cn0_ibyte": ["--array", "arr.txt", "--scint", "sc.txt"],
    "refl_cn0_osc_ibyte": ["--reflector", "ground,2,-6", "--reflector", "wall,100,90,-3"],
}
# The case whose count cannot be 0: the AGC holds the rms at 32 x 2^shift and ibyte clamps at 127 x 2^shift, 3.97 sigma of a Gaussian
# stream: 7e-5 of 2.08 M values, about 150.  (Without an AGC the chosen shift puts the clamp at 4 to 8 sigma of the noise, here 7.2.)
SATURATES = {"cn0_osc_fir_agc_monitor_ibyte"}
CASES = {c["name"]: c for c in cli_golden.CHAIN_CASES}


def _opts(argv, name):
    return [argv[k + 1] for k, a in enumerate(argv) if a == name]


def _numbers(text, n):
    v = [float(t) for t in text.split(",")]
    return v + [0.0] * (n - len(v))


def _printed_saturated(stderr):
    m = re.search(r"WARNING: (\d+) of \d+ IQ values", stderr)
    return int(m.group(1)) if m else 0


def _front(case):
    """The front stream(s) of a case, one per element, and the count its synthesis passes report."""
    argv, elements = FRONT[case["name"]], case.get("elements")
    run = lambda extra, files: cli_golden.run_chain_files(  # noqa: E731
        cli_golden.CLI, {"name": case["name"] + "_front", "fmt": "ishort", "argv": argv + extra, "elements": elements}, 3, files)
    if "--oversample" not in argv:
        w = run([], cli_golden.CHAIN_FILES)
        return [np.frombuffer(b, dtype="<i2") for b in w["iq"]], _printed_saturated(w["stderr"])
    files = dict(cli_golden.CHAIN_FILES, **PICKS)
    even, odd = run(["--fir", "pick0.txt"], files), run(["--fir", "pick1.txt"], files)
    a, b = (np.frombuffer(w["iq"][0], dtype="<i2").reshape(-1, 2) for w in (even, odd))
    assert a.shape == b.shape == (EPOCHS * N, 2) and not b[0].any()  # (x[-1]: the start of the stream)
    x = np.zeros((2 * EPOCHS * N, 2), dtype=np.int16)
    x[0::2] = a
    x[1:-1:2] = b[1:]
    assert _printed_saturated(even["stderr"]) == _printed_saturated(odd["stderr"])
    return [x.reshape(-1)], _printed_saturated(even["stderr"])


def _chain_args(pkg, case, stderr):
    """chain_model.Chain's arguments for the case's options, with the decisions the command printed."""
    argv, fmt = case["argv"], case["fmt"]
    M = int((_opts(argv, "--oversample") or ["1"])[0])
    rate = M * FS
    kw = {"fmt": fmt, "param": 0, "decim": M}
    cn0, jams = _opts(argv, "--cn0"), _opts(argv, "--jam")
    sigma = None
    if cn0 or jams:
        gain = float(re.search(r"signal gain ([0-9.e+-]+) \(chosen\)", stderr).group(1))
        kw["noise"] = (0, 0, int(round(gain * 65536.0)), 0)
        if cn0:
            n = pkg.noise_from_cn0(float(cn0[0]), rate, gain)
            m = re.search(r"Noise floor: .*, seed (\d+), stream (\d+)", stderr)
            kw["noise"] = (int(m.group(1)), int(m.group(2)), n["gain_q16"], n["sigma_q4"])
            sigma = n["sigma_q4"] / 16.0
        kw["interf"] = []
        for text in jams:
            js, f_lo, f_hi, sweep_us, period_us, on_us = _numbers(text, 6)
            kw["interf"].append(pkg.interf_make(js, gain, rate, f_lo, f_hi, sweep_us * 1e-6, period_us * 1e-6, on_us * 1e-6))
    if _opts(argv, "--lo-offset") or _opts(argv, "--phase-noise"):
        f_hz, drift = _numbers((_opts(argv, "--lo-offset") or ["0"])[0], 2)
        o = pkg.osc_make(f_hz, drift, float((_opts(argv, "--phase-noise") or ["0"])[0]), rate, FC)
        m = re.search(r"Oscillator: .*; seed (\d+), stream (\d+)", stderr)
        kw["osc"] = dict(o, seed=int(m.group(1)), stream=int(m.group(2)))
        assert ("S = %d)" % o["s"]) in stderr and ("F = %d, D = %d at" % (o["f"], o["d"])) in stderr
    if M > 1:
        kw["taps"] = _printed_taps(stderr)
        assert np.array_equal(kw["taps"], pkg.synth.firdec_lowpass(0.45 * FS, rate, 32 * M + 1))
    elif _opts(argv, "--fir-lowpass"):
        fc, nt = _numbers(_opts(argv, "--fir-lowpass")[0], 2)
        kw["taps"] = pkg.synth.fir_lowpass(fc, FS, int(nt))
        assert np.array_equal(kw["taps"], _printed_taps(stderr))
    if fmt == "ibyte":
        kw["param"] = int(re.search(r"--iq-shift (\d+) \(chosen\)", stderr).group(1))
    if "--agc" in argv or fmt == "i2bit":
        line = _agc_line(stderr)
        m = re.search(r"target rms (\S+) LSB, blocks of (\d+) samples, window (\d+) blocks, initial rms (\S+) LSB", line)
        init = 750.0 if sigma is None else sigma  # the sigma where the AGC sits: behind the filter where there is one
        if sigma is not None and "taps" in kw:
            init *= np.sqrt(float((kw["taps"].astype(np.float64) ** 2).sum())) / 16384.0
        assert "%g" % init == m.group(4), (init, line)
        kw["agc"] = pkg.synth.agc_from_rms(float(m.group(1)), init, int(m.group(2)), int(m.group(3)))
        if fmt == "i2bit":
            kw["param"] = int(re.search(r"--i2bit-threshold (\d+)", line).group(1))
    return kw


def _element(kw, k):
    """--array: element k's chain is the one fused pass with the noise stream 8 x --noise-stream + k (tests/test_iq_array_cli.py)."""
    seed, stream, g, s = kw["noise"]
    return dict(kw, noise=(seed, 8 * stream + k, g, s))


@pytest.mark.parametrize("name", list(FRONT))
def test_both_batch_lengths_write_the_chain_model_over_the_front_stream(pkg, tmp_path, name):
    case = CASES[name]
    t0 = time.time()
    fronts, front_sat = _front(case)
    assert all(x.size == 2 * EPOCHS * N * (2 if "--oversample" in case["argv"] else 1) for x in fronts) and len(fronts) == case.get("elements", 1)
    wrote = {b: cli_golden.run_chain_files(cli_golden.CLI, case, b, cli_golden.CHAIN_FILES) for b in cli_golden.CHAIN_BATCHES}
    t1 = time.time()
    kw = _chain_args(pkg, case, wrote[1]["stderr"])
    chains = [chain_model.Chain(**(_element(kw, k) if case.get("elements") else kw)) for k in range(len(fronts))]
    model = [c.run(x) for c, x in zip(chains, fronts)]  # once per case
    t2 = time.time()
    sats = [m[2] for m in model]
    print("%s: stages %s, %.1f s in the command's %d runs, %.1f s in the model; saturated: front %d, chain %s" % (
        name, "+".join(chains[0].stages), t1 - t0, len(wrote) + (2 if "--oversample" in case["argv"] else 1), t2 - t1, front_sat, sats))
    # the input does what it is for: the stages change most values of the stream
    plain = {k: v for k, v in kw.items() if k in ("fmt", "param") or (k == "agc" and case["fmt"] == "i2bit")}
    for (out, _, _), x in zip(model, fronts):
        kept = x.reshape(-1, 2)[::kw["decim"]].reshape(-1)
        base = chain_model.Chain(**plain).run(kept)[0]
        assert base.size == out.size and np.count_nonzero(base != out) > 0.5 * out.size, name
    if name in SATURATES:
        assert all(s > 0 for s in sats), sats
    for b in cli_golden.CHAIN_BATCHES:
        assert len(wrote[b]["iq"]) == len(model)
        for k, ((out, gains, _), got) in enumerate(zip(model, wrote[b]["iq"])):
            got = np.frombuffer(got, dtype=np.uint8)
            assert got.size == out.size, (name, b, k, got.size, out.size)
            bad = np.flatnonzero(got != out)
            assert bad.size == 0, "%s -B %d, element %d: %d of %d bytes differ, the first at %d" % (name, b, k, bad.size, got.size, bad[0])
        total = front_sat + sum(sats)
        assert _printed_saturated(wrote[b]["stderr"]) == total, (name, b, front_sat, sats)
        assert ("saturated" in wrote[b]["stderr"]) == (total > 0)
        if case.get("agc_log"):
            log = tmp_path / ("agc_B%d.csv" % b)
            log.write_bytes(wrote[b]["agc_log"])
            _, g, _ = _read_log(log)
            assert np.array_equal(g, model[0][1]) and g.size == EPOCHS * N // kw["agc"]["block_len"]
