#!/usr/bin/env python3
"""Probe of the front-end FIR pass (gal_synth_iq_fir, k_iq_fir of csrc/iq_fir.hip) on the MI355X: 120 epochs x 260 000 complex samples
(31.2 M samples, 125 MB in and 125 MB out) filtered with T = 1, 25, 63 and 128 taps, each call timed between two HIP events on the
engine's stream, beside a device-to-device copy of the same number of bytes (read 125 MB, write 125 MB) in the same process and on
the same stream -- the yardstick: a filter that tracks the copy is bound by memory, one that falls behind it by the 2 T integer
multiply-adds per complex sample.  Warm-up calls first, then --reps repetitions (at least 20) in which the four filters and the copy
alternate; median and range per line, and the kernel source's SHA-256, so that a figure can be tied to the code it was taken from.
With --out the lines are also written to that file (profiles/).  Run it under a time limit of its own:
    timeout -k 10 300 python tools/fir_probe.py --out profiles/fir_probe.log"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS = 2.6e6
N = 260000
TAPS = (1, 25, 63, 128)


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
    n = a.epochs * N
    rng = np.random.default_rng(15)
    # a signal of the engine's size (a dozen satellites: a few thousand LSB), so that the clamp stays as quiet as in a real run
    x = torch.from_numpy(rng.integers(-3000, 3001, size=2 * n, dtype=np.int16)).cuda()
    y = torch.zeros(2 * n, dtype=torch.int16, device="cuda")
    filters = {}
    for T in TAPS:
        if T == 1:
            filters[T] = np.array([16384], dtype=np.int16)
        elif T % 2:
            filters[T] = pkg.synth.fir_lowpass(1.0e6, FS, T)
        else:  # an even length: the 127-tap low-pass behind one zero tap -- as many multiply-adds as any 128 taps
            filters[T] = np.concatenate([pkg.synth.fir_lowpass(1.0e6, FS, T - 1), np.zeros(1, dtype=np.int16)])
    torch.cuda.synchronize()
    t_fir = {T: [] for T in TAPS}
    t_copy = []
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with pkg.SynthEngine(device=0) as eng:
        stream = torch.cuda.Stream()
        eng.set_stream(stream.cuda_stream)
        for rep in range(a.reps + 3):  # three warm-up rounds: code object, the filter table, the counter
            for T in TAPS:
                eng.fir_set(filters[T])
                eng.iq_saturated()  # the table's upload is not part of the interval
                t0.record(stream)
                eng.iq_fir(x.data_ptr(), n, y.data_ptr())
                t1.record(stream)
                t1.synchronize()
                if rep >= 3:
                    t_fir[T].append(t0.elapsed_time(t1))
            with torch.cuda.stream(stream):
                t0.record(stream)
                y.copy_(x)
                t1.record(stream)
            t1.synchronize()
            if rep >= 3:
                t_copy.append(t0.elapsed_time(t1))
        sat = eng.iq_saturated()
        eng.set_stream(None)
    nbytes = 8 * n  # 4 bytes read and 4 written per complex sample
    src = os.path.join(ROOT, "galileo-sdr-sim_amd", "csrc", "iq_fir.hip")
    lines = ["%d epochs x %d = %.2f M complex samples, %d repetitions after 3 warm-up rounds (ms: median, min .. max); %d values clamped"
             % (a.epochs, N, n / 1e6, a.reps, sat),
             "csrc/iq_fir.hip sha256 %s" % hashlib.sha256(open(src, "rb").read()).hexdigest(),
             "device: %s" % torch.cuda.get_device_name(0)]
    tc = np.array(t_copy)
    for T in TAPS:
        t = np.array(t_fir[T])
        lines.append("  k_iq_fir, T = %3d:        %8.3f  %8.3f .. %8.3f   %.3g bytes/s   %.2f x the copy   %.3g multiply-adds/s"
                     % (T, np.median(t), t.min(), t.max(), nbytes / np.median(t) * 1e3, np.median(t) / np.median(tc), 2.0 * T * n / np.median(t) * 1e3))
    lines.append("  copy of as many bytes:    %8.3f  %8.3f .. %8.3f   %.3g bytes/s" % (np.median(tc), tc.min(), tc.max(), nbytes / np.median(tc) * 1e3))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
