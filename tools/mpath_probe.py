#!/usr/bin/env python3
"""Probe of the multipath pass (gal_synth_iq_mpath, k_iq_echo of csrc/iq_echo.hip) on the MI355X, on the CLI's batch: 12 parts of
128 epochs x 260 000 complex samples.  Each call is timed between two HIP events on the engine's stream.  Measured, alternating in one
process: gal_synth_iq_wsum on the 12 parts (the yardstick, never the code under test); gal_synth_iq_mpath with 0, 12 and 32 echoes
whose delays have every residue modulo 4; 12 echoes whose delays are all multiples of 4 (one aligned load per echo instead of two);
and the 0-echo call in a second interleaved series, whose median's distance from the first is the run-to-run scatter to judge the rest
by.  Then gal_synth_run_mpath (three slots with an echo) against gal_synth_run_gains on one 12-satellite batch with twelve distinct
gain columns, timed on the host around the call and its fence.  Median and range per line, the ratio to the weighted sum, the bytes
per second that parts and output alone account for, and the kernel source's SHA-256.  With --out the lines are also written to that
file (profiles/).  Run it under a time limit of its own:
    timeout -k 10 500 python tools/mpath_probe.py --out profiles/mpath_probe.log"""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 260000
PARTS = 12
WARM = 3


def main():
    import numpy as np
    import torch

    from __graft_entry__ import load_pkg

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=128)
    ap.add_argument("--run-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    pkg = load_pkg()
    torch.cuda.init()
    E = a.epochs
    rng = np.random.default_rng(18)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(18)
    # one satellite's stream each: a few hundred LSB, so that the clamp stays as quiet as in a real run
    parts = [torch.randint(-500, 501, (2 * E * N,), dtype=torch.int16, device="cuda", generator=gen) for _ in range(PARTS)]
    out = torch.zeros(2 * E * N, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ptrs = [p.data_ptr() for p in parts]
    gains = rng.integers(60, 300, size=(E, PARTS))

    def table(n_echo, aligned):
        r = np.zeros((E, n_echo), dtype=pkg.ECHO_DTYPE)
        r["gain_q7"] = rng.integers(20, 120, size=r.shape)
        d = rng.integers(1, 256, size=n_echo) * 4 if aligned else rng.integers(1, 1025, size=n_echo)
        if not aligned and n_echo >= 4:
            d[:4] = (1021, 1022, 1023, 1024)
        r["delay"] = d[None, :]
        r["ph0"] = rng.integers(0, 1 << 32, size=r.shape, dtype=np.uint64)
        r["dph"] = rng.integers(-4000, 4000, size=n_echo)[None, :]  # fading of a few Hz
        return np.arange(n_echo) % PARTS, r

    cases = {"iq_mpath  0 echoes": table(0, False), "iq_mpath 12 echoes": table(12, False), "iq_mpath 32 echoes": table(32, False),
             "iq_mpath 12 echoes, delays multiples of 4": table(12, True)}
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {}

    def timed(name, fn, rep):
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        if rep >= WARM:
            res.setdefault(name, []).append(t0.elapsed_time(t1))

    lines = []
    with pkg.SynthEngine(device=0) as eng:
        stream = torch.cuda.Stream()
        eng.set_stream(stream.cuda_stream)
        for rep in range(a.reps + WARM):
            timed("iq_wsum  (12 parts)", lambda: eng.iq_wsum(ptrs, gains, out.data_ptr()), rep)
            for name, (pof, rows) in cases.items():
                timed(name, lambda: eng.iq_mpath(ptrs, gains, out.data_ptr(), pof, rows), rep)
            pof, rows = cases["iq_mpath  0 echoes"]
            timed("iq_mpath  0 echoes, second series", lambda: eng.iq_mpath(ptrs, gains, out.data_ptr(), pof, rows), rep)
        sat = eng.iq_saturated()
        eng.set_stream(None)
        del parts
        # run_mpath against run_gains: 12 satellites, 12 distinct gain columns (12 synthesis runs either way), echoes on three slots
        p = pkg.workloads.make_synthetic(n_epochs=E, n_chan=12, n_slots=16, seed=18)
        g = np.tile(rng.permutation(np.arange(100, 116))[None, :], (E, 1))
        echoes = [pkg.mpath_make(d, db, ph, f) for d, db, ph, f in ((1e-6, -6, 90, 2.0), (3.3e-6, -3, 10, 0.0), (2e-4, -10, 200, -1.0),
                                                                    (5e-5, -8, 300, 0.5))]
        sof = [0, 0, 5, 11]
        erows = np.stack([pkg.mpath_rows(e, g[:, s], 0, N) for e, s in zip(echoes, sof)], axis=1)
        runs = {}
        for rep in range(a.run_reps + 1):
            for name, fn in (("run_gains", lambda: eng.run_gains(p, g, out.data_ptr())),
                             ("run_mpath", lambda: eng.run_mpath(p, g, out.data_ptr(), sof, erows))):
                eng.iq_saturated()
                w0 = time.perf_counter()
                fn()
                eng.iq_saturated()
                if rep >= 1:
                    runs.setdefault(name, []).append((time.perf_counter() - w0) * 1e3)
                runs[name + " runs"] = eng.gain_runs()
    src = os.path.join(ROOT, "galileo-sdr-sim_amd", "csrc", "iq_echo.hip")
    lines += ["%d parts x %d epochs x %d complex samples, %d repetitions after %d warm-up rounds (ms: median, min .. max); %d values clamped"
              % (PARTS, E, N, a.reps, WARM, sat),
              "csrc/iq_echo.hip sha256 %s" % hashlib.sha256(open(src, "rb").read()).hexdigest(), "device: %s" % torch.cuda.get_device_name(0)]
    base = float(np.median(res["iq_wsum  (12 parts)"]))
    stream_bytes = 4.0 * (PARTS + 1) * E * N  # every part read once, the output written once
    for name, ts in res.items():
        t = np.array(ts)
        lines.append("  %-44s %8.3f  %8.3f .. %8.3f   %.2f x iq_wsum   %.3g bytes/s of parts and output" % (
            name, np.median(t), t.min(), t.max(), np.median(t) / base, stream_bytes / np.median(t) * 1e3))
    s1, s2 = np.median(res["iq_mpath  0 echoes"]), np.median(res["iq_mpath  0 echoes, second series"])
    lines.append("  scatter: two interleaved series of one call differ by %.3f ms in the median (%.2f %%)" % (abs(s1 - s2), 100.0 * abs(s1 - s2) / s1))
    for name in ("run_gains", "run_mpath"):
        t = np.array(runs[name])
        lines.append("  %-44s %8.1f  %8.1f .. %8.1f   %d synthesis runs, %d repetitions (host clock, call + fence)" % (
            name, np.median(t), t.min(), t.max(), runs[name + " runs"], t.size))
    lines.append("  run_mpath / run_gains = %.3f" % (np.median(runs["run_mpath"]) / np.median(runs["run_gains"])))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
