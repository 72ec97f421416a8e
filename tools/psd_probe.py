#!/usr/bin/env python3
"""Probe of the Welch power spectrum (gal_synth_iq_psd) on the MI355X: one epoch -- 260 000 samples of ishort -- under the Hann window at
N = 1024 (hop 512, 506 segments) and at N = 4096 (hop 2048, 125 segments), each timed with events over `--reps` calls, beside the two
floors the time is held against: the buffer's bytes over the HBM read rate, and the butterfly count n_seg (N / 2) log2 N.  Kernel
times proper:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/psd_probe.py --child 1024     (or: --child 4096)
Without --child the two steps run as child processes, each under its own timeout, and the second is not started if the first fails."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8.0e12  # the MI355X's nominal HBM3E read rate


def child(size, reps):
    import numpy as np
    import torch

    from __graft_entry__ import load_pkg

    pkg = load_pkg()
    torch.cuda.init()
    log2_n = size.bit_length() - 1
    p = pkg.workloads.m_syn12(n_epochs=1)
    with pkg.SynthEngine(device=0) as eng:
        x, _, _ = eng.run_host(p)
        n = x.size // 2
        xd = torch.from_numpy(x).cuda()
        out = torch.zeros(size, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        _, n_seg = eng.iq_psd(xd.data_ptr(), "ishort", n, log2_n, size // 2, "hann", out_ptr=out.data_ptr())  # warm-up (code objects)
        eng.iq_saturated()
        stream = torch.cuda.Stream()
        eng.set_stream(stream.cuda_stream)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(reps):
            t0.record(stream)
            eng.iq_psd(xd.data_ptr(), "ishort", n, log2_n, size // 2, "hann", out_ptr=out.data_ptr())
            t1.record(stream)
            t1.synchronize()
            times.append(t0.elapsed_time(t1))
        eng.set_stream(None)
        sums = out.cpu().numpy().view(np.uint64).astype(np.float64)
        us = float(np.median(times)) * 1e3
        bfly = n_seg * (size // 2) * log2_n
        k = int(np.argmax(sums))
        print("N = %d Hann: %d samples, %d segments; strongest bin %+d (%.0f Hz), %.1f dB over the median"
              % (size, n, n_seg, k - size if k >= size // 2 else k, (k - size if k >= size // 2 else k) * 2.6e6 / size, 10 * np.log10(sums.max() / np.median(sums))))
        print("N = %d Hann: %d calls, median %.1f us (min %.1f, max %.1f) from memset to kernel end; floors: %d bytes / %.0f TB/s = %.2f us; "
              "%d butterflies -> %.1f butterflies/ns" % (size, reps, us, min(times) * 1e3, max(times) * 1e3, 4 * n, HBM_BYTES_PER_S / 1e12,
                                                       4 * n / HBM_BYTES_PER_S * 1e6, bfly, bfly / us / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("1024", "4096"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=120)
    a = ap.parse_args()
    if a.child:
        child(int(a.child), a.reps)
        return 0
    for step in ("1024", "4096"):
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", step, "--reps", str(a.reps)])
        if r.returncode != 0:
            print("step %s ended with status %d: stopping" % (step, r.returncode))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
