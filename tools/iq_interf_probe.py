#!/usr/bin/env python3
"""Probe of the interference pass (gal_synth_iq_convert_interf) on the MI355X: at the CLI's batch -- 128 epochs = 33.28 M complex
samples -- and in each output format, the time of one call with the noise floor alone (n_interf = 0: the instances k_iq_pass<Fmt, 1, false> of csrc/iq_pass.hip),
with 1 and with 4 sources on top of it, and with 1 source and no noise.  The variants alternate inside every repetition, each call
between two events on the engine's stream; the noise-only call is timed twice per repetition, so that the difference of its two
series is the run-to-run scatter against which the others are read.  Kernel times proper:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/iq_interf_probe.py --child ishort
Without --child the three formats run as child processes, each under its own timeout, and none is started after one that fails."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS = 2.6e6


def child(fmt, reps, epochs):
    import numpy as np
    import torch

    from __graft_entry__ import load_pkg

    pkg = load_pkg()
    torch.cuda.init()
    n = epochs * 260000
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randint(-4100, 4101, (2 * n,), generator=gen, device="cuda", dtype=torch.int16)
    out = torch.zeros(pkg.iq_bytes(fmt, n), dtype=torch.uint8, device="cuda")
    noise = pkg.noise_from_cn0(45.0, FS)
    noise["seed"] = 1
    cw = pkg.interf_make(20.0, 1.0, FS, 1e5)
    four = [cw, pkg.interf_make(20.0, 1.0, FS, -1.2e6, 1.2e6, 100e-6), pkg.interf_make(15.0, 1.0, FS, 3e5, 0.0, 0.0, 1e-3, 2e-4),
            pkg.interf_make(10.0, 1.0, FS, -5e5, 5e5, 1e-3, 5e-3, 1e-3)]
    shift = 8 if fmt == "ibyte" else 0
    variants = [("noise only (a)", noise, None), ("noise + 1 source", noise, [cw]), ("noise + 4 sources", noise, four),
                ("1 source, no noise", None, [cw]), ("noise only (b)", noise, None)]
    with pkg.SynthEngine(device=0) as eng:
        stream = torch.cuda.Stream()
        eng.set_stream(stream.cuda_stream)
        times = {name: [] for name, _, _ in variants}
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for rep in range(reps + 2):  # two warm-up rounds: code objects, the counter
            for name, nz, src in variants:
                t0.record(stream)
                eng.iq_convert(x.data_ptr(), n, fmt, shift, out.data_ptr(), noise=nz, first_sample=rep * n, interf=src)
                t1.record(stream)
                t1.synchronize()
                if rep >= 2:
                    times[name].append(t0.elapsed_time(t1))
        eng.iq_saturated()
        eng.set_stream(None)
    print("%s, %d epochs = %.2f M samples, %d calls each (ms: median, min .. max; samples per second at the median)" % (fmt, epochs, n / 1e6, reps))
    for name, _, _ in variants:
        t = np.array(times[name])
        print("  %-20s %8.3f  %8.3f .. %8.3f   %.3g" % (name, np.median(t), t.min(), t.max(), n / np.median(t) * 1e3))
    a, b = np.median(times["noise only (a)"]), np.median(times["noise only (b)"])
    print("  scatter of the same call: medians %.3f and %.3f ms (%.2f %%)" % (a, b, 100.0 * abs(a - b) / min(a, b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("ishort", "ibyte", "ibit"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=128)
    ap.add_argument("--timeout", type=int, default=180)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.epochs)
        return 0
    for fmt in ("ishort", "ibyte", "ibit"):
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", fmt, "--reps", str(a.reps),
                            "--epochs", str(a.epochs)])
        if r.returncode != 0:
            print("format %s ended with status %d: stopping" % (fmt, r.returncode))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
