#!/usr/bin/env python3
"""Probe of the receiver oscillator (gal_synth_iq_osc, csrc/iq_osc.hip) on the MI355X, on the CLI's batch: 128 epochs x 260 000
complex samples, in place.  Each call is timed between two HIP events on the engine's stream.  Measured, alternating in one process:
gal_synth_iq_osc with S = 0 (one launch, no Philox work); gal_synth_iq_osc with S > 0 (all three launches: tile sums, scan, rotation);
and the two yardsticks, never the code under test -- gal_synth_iq_convert_noise in place (ishort), which draws twice the Gaussians
per sample, and gal_synth_iq_fir with one tap, the plain read-and-write pass; the S = 0 call in a second interleaved series, whose
median's distance from the first is the run-to-run scatter to judge the rest by.  Median and range per line, the bytes per second that
input and output alone account for, and the kernel source's SHA-256.  With --out the lines are also written to that file
(profiles/).  Run it under a time limit of its own:
    timeout -k 10 300 python tools/osc_probe.py --out profiles/osc_probe.log"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 260000
WARM = 3


def main():
    import numpy as np
    import torch

    from __graft_entry__ import load_pkg

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    pkg = load_pkg()
    torch.cuda.init()
    n = a.epochs * N
    gen = torch.Generator(device="cuda")
    gen.manual_seed(19)
    # a sum of satellites and noise: about a thousand LSB, so that the clamp stays as quiet as in a real run
    buf = torch.randint(-3000, 3001, (2 * n,), dtype=torch.int16, device="cuda", generator=gen)
    out = torch.zeros(2 * n, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    det = pkg.osc_make(1500.0, 2.0, 0.0)
    noisy = pkg.osc_make(1500.0, 2.0, 1e-21)
    noise = pkg.noise_from_cn0(60.0, 2.6e6, 1.0)  # a small sigma: the buffer takes the noise of every repetition
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {}

    def timed(name, fn, rep):
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        if rep >= WARM:
            res.setdefault(name, []).append(t0.elapsed_time(t1))

    with pkg.SynthEngine(device=0) as eng, pkg.SynthEngine(device=0) as eng2:
        stream = torch.cuda.Stream()
        eng.set_stream(stream.cuda_stream)   # S = 0
        eng2.set_stream(stream.cuda_stream)  # S > 0: a handle of its own, so that each stream runs on
        eng.osc_set(det, 0)
        eng2.osc_set(noisy, 0)
        eng.fir_set([16384])
        for rep in range(a.reps + WARM):
            timed("iq_osc S = 0 (1 launch)", lambda: eng.iq_osc(buf.data_ptr(), n, buf.data_ptr()), rep)
            timed("iq_osc S > 0 (3 launches)", lambda: eng2.iq_osc(buf.data_ptr(), n, buf.data_ptr()), rep)
            timed("iq_convert_noise ishort, in place", lambda: eng.iq_convert(buf.data_ptr(), n, "ishort", out_ptr=buf.data_ptr(), noise=noise,
                                                                               first_sample=rep * n), rep)
            timed("iq_fir 1 tap", lambda: eng.iq_fir(buf.data_ptr(), n, out.data_ptr()), rep)
            timed("iq_osc S = 0, second series", lambda: eng.iq_osc(buf.data_ptr(), n, buf.data_ptr()), rep)
        sat = eng.iq_saturated() + eng2.iq_saturated()
        eng.set_stream(None)
        eng2.set_stream(None)
    src = os.path.join(ROOT, "galileo-sdr-sim_amd", "csrc", "iq_osc.hip")
    lines = ["%d epochs x %d complex samples in place, %d repetitions after %d warm-up rounds (ms: median, min .. max); %d values clamped"
             % (a.epochs, N, a.reps, WARM, sat),
             "csrc/iq_osc.hip sha256 %s" % hashlib.sha256(open(src, "rb").read()).hexdigest(), "device: %s" % torch.cuda.get_device_name(0)]
    base = float(np.median(res["iq_fir 1 tap"]))
    stream_bytes = 8.0 * n  # every sample read once and written once
    for name, ts in res.items():
        t = np.array(ts)
        lines.append("  %-36s %8.3f  %8.3f .. %8.3f   %.2f x iq_fir 1 tap   %.3g bytes/s of input and output" % (
            name, np.median(t), t.min(), t.max(), np.median(t) / base, stream_bytes / np.median(t) * 1e3))
    s1, s2 = np.median(res["iq_osc S = 0 (1 launch)"]), np.median(res["iq_osc S = 0, second series"])
    lines.append("  scatter: two interleaved series of one call differ by %.3f ms in the median (%.2f %%)" % (abs(s1 - s2), 100.0 * abs(s1 - s2) / s1))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
