#!/usr/bin/env python3
"""Probe of the decimating front-end filter (gal_synth_iq_firdec, k_iq_firdec of csrc/iq_firdec.hip) on the MI355X.  Per decimation M
the input is 120 epochs x M x 260 000 complex samples; each call is timed between two HIP events on the engine's stream.  Measured:
the decimator at (M, T) = (4, 129), (4, 511), (8, 257), (15, 481); and, as yardsticks that are never the code under test, a
device-to-device copy of as many bytes as the decimator reads, and the merged gal_synth_iq_fir at T = 127 over the same input beside
the decimator at T = 127 for M = 2, 4 and 8 -- the one condition: the decimator, with 1 / M of the arithmetic and of the bytes written,
is not slower than the full-rate filter.  One call (the decimator at M = 4, T = 127) is timed in two interleaved series, whose
medians' difference is the run-to-run scatter to judge the rest by.  Warm-up rounds first, then --reps repetitions (at least 20) in
which all calls of one input size alternate; median and range per line, and the kernel source's SHA-256.  With --out the lines are
also written to that file (profiles/).  Run it under a time limit of its own:
    timeout -k 10 500 python tools/firdec_probe.py --out profiles/firdec_probe.log"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS = 2.6e6
N = 260000
SHAPES = ((4, 129), (4, 511), (8, 257), (15, 481))
VERSUS = (2, 4, 8)  # the merged filter against the decimator, both at T = 127
WARM = 3


def main():
    import numpy as np
    import torch

    from __graft_entry__ import load_pkg

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=120)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    pkg = load_pkg()
    torch.cuda.init()
    rng = np.random.default_rng(16)
    decims = sorted({m for m, _ in SHAPES} | set(VERSUS))
    n_max = a.epochs * N * max(decims)
    # a signal of the engine's size (a dozen satellites: a few thousand LSB), so that the clamp stays as quiet as in a real run
    x = torch.from_numpy(rng.integers(-3000, 3001, size=2 * n_max, dtype=np.int16)).cuda()
    y = torch.zeros(2 * a.epochs * N * max(VERSUS), dtype=torch.int16, device="cuda")
    c = torch.zeros(2 * n_max, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {}  # name -> (list of ms, input samples, taps or 0)
    lp127 = pkg.synth.fir_lowpass(1.0e6, FS, 127)

    def timed(name, n_in, T, fn, rep):
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        if rep >= WARM:
            res.setdefault(name, ([], n_in, T))[0].append(t0.elapsed_time(t1))

    with pkg.SynthEngine(device=0) as eng:
        stream = torch.cuda.Stream()
        eng.set_stream(stream.cuda_stream)
        for M in decims:
            n_in = a.epochs * N * M
            shapes = [T for m, T in SHAPES if m == M]
            for rep in range(a.reps + WARM):
                for T in shapes:
                    eng.firdec_set(pkg.synth.firdec_lowpass(0.45 * FS, M * FS, T), M)
                    eng.iq_saturated()  # the table's upload is not part of the interval
                    timed("k_iq_firdec M = %2d, T = %3d" % (M, T), n_in, T, lambda: eng.iq_firdec(x.data_ptr(), n_in, y.data_ptr()), rep)
                if M in VERSUS:
                    eng.firdec_set(lp127, M)
                    eng.fir_set(lp127)
                    eng.iq_saturated()
                    timed("k_iq_firdec M = %2d, T = 127" % M, n_in, 127, lambda: eng.iq_firdec(x.data_ptr(), n_in, y.data_ptr()), rep)
                    timed("k_iq_fir    same input, T = 127 (M = %d)" % M, n_in, -127, lambda: eng.iq_fir(x.data_ptr(), n_in, c.data_ptr()), rep)
                    if M == 4:  # the second series of one call: the scatter
                        timed("k_iq_firdec M =  4, T = 127, second series", n_in, 127, lambda: eng.iq_firdec(x.data_ptr(), n_in, y.data_ptr()), rep)

                def copy():
                    with torch.cuda.stream(stream):
                        c[: 2 * n_in].copy_(x[: 2 * n_in])

                timed("copy of the bytes read (M = %d)" % M, n_in, 0, copy, rep)
        sat = eng.iq_saturated()
        eng.set_stream(None)
    src = os.path.join(ROOT, "galileo-sdr-sim_amd", "csrc", "iq_firdec.hip")
    lines = ["%d epochs x M x %d complex input samples, %d repetitions after %d warm-up rounds (ms: median, min .. max); %d values clamped"
             % (a.epochs, N, a.reps, WARM, sat),
             "csrc/iq_firdec.hip sha256 %s" % hashlib.sha256(open(src, "rb").read()).hexdigest(),
             "device: %s" % torch.cuda.get_device_name(0)]
    med = {k: float(np.median(v[0])) for k, v in res.items()}
    for name, (ts, n_in, T) in res.items():
        t = np.array(ts)
        line = "  %-46s %8.3f  %8.3f .. %8.3f" % (name, np.median(t), t.min(), t.max())
        M = int(name.split("M =")[1].split(",")[0].split(")")[0])
        if T > 0:  # the decimator: T multiply-adds per rail and output, n_in / M outputs
            line += "   %.3g multiply-adds/s   %.2f x the copy" % (2.0 * T * (n_in / M) / np.median(t) * 1e3, np.median(t) / med["copy of the bytes read (M = %d)" % M])
        elif T < 0:
            line += "   %.3g multiply-adds/s   the decimator takes %.2f x this" % (2.0 * -T * n_in / np.median(t) * 1e3, med["k_iq_firdec M = %2d, T = 127" % M] / np.median(t))
        else:
            line += "   %.3g bytes/s read" % (4.0 * n_in / np.median(t) * 1e3)
        lines.append(line)
    s1, s2 = med["k_iq_firdec M =  4, T = 127"], med["k_iq_firdec M =  4, T = 127, second series"]
    lines.append("  scatter: two interleaved series of one call differ by %.3f ms in the median (%.2f %%)" % (abs(s1 - s2), 100.0 * abs(s1 - s2) / s1))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
