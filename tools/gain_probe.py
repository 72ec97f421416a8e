#!/usr/bin/env python3
"""Probe of the per-satellite power path (gal_synth_run_gains, k_iq_wsum of csrc/iq_gain.hip) on the MI355X, 12 satellites x 120 epochs
at 2.6 MS/s (31.2 M complex samples): the wall time of run_gains with 12 different gain columns (12 single-slot runs + the weighted
sum, fence included) against plain plan + execute + finish of the same records and against run_gains at unity (one run), the three
alternating inside every repetition; and the time of k_iq_wsum alone on 12 parts between two events on the engine's stream, as bytes
per second ((12 + 1) x 4 bytes per sample), beside a device-to-device copy of the same number of bytes moved on the same card
(read + write, as torch's copy_ does it).  The interval around iq_wsum holds what the call enqueues -- the copy of the gain table
(6 KB) to the device in front of the kernel -- and starts only after the call's wait, on the host, for the kernel of the call before.
tools/wrcal.hip's coalesced 1 GiB fill is the write-only streaming figure of the same card: it prints no time of its own,
    rocprofv3 --kernel-trace --stats -d <dir> -- tools/wrcal
gives it.  The plain call is timed twice per repetition: the difference of its two series is the
run-to-run scatter.  Run it under a time limit of its own:  timeout -k 10 300 python tools/gain_probe.py"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS = 2.6e6
N = 260000


def main():
    import numpy as np
    import torch

    from __graft_entry__ import load_pkg

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=120)
    ap.add_argument("--chan", type=int, default=12)
    a = ap.parse_args()
    pkg = load_pkg()
    torch.cuda.init()
    E, C = a.epochs, a.chan
    p = pkg.workloads.make_synthetic(n_epochs=E, n_chan=C, n_slots=16, samples_per_epoch=N, seed=11)
    rng = np.random.default_rng(3)
    g_diff = np.zeros(p.shape, dtype=np.uint16)
    g_diff[:, :C] = 80 + 4 * rng.permutation(C)  # one column per slot, all different: a base value plus a permutation
    assert len({tuple(g_diff[:, s]) for s in range(C)}) == C
    g_unity = np.full(p.shape, 128, dtype=np.uint16)
    n_val = E * N * 2
    out = torch.zeros(n_val, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    walls = {"plain (a)": [], "run_gains, %d columns" % C: [], "run_gains, unity": [], "plain (b)": []}
    with pkg.SynthEngine(device=0) as eng:
        stream = torch.cuda.Stream()
        eng.set_stream(stream.cuda_stream)

        def plain():
            eng.plan(p)
            eng.execute(out.data_ptr())
            eng.finish()

        def gains(g):
            eng.run_gains(p, g, out.data_ptr())
            eng.iq_saturated()

        calls = [plain, lambda: gains(g_diff), lambda: gains(g_unity), plain]
        gains(g_diff)
        assert eng.gain_runs() == C, eng.gain_runs()  # what the line below calls "C columns" is C runs and a C-part sum
        gains(g_unity)
        assert eng.gain_runs() == 1
        for rep in range(a.reps + 2):  # two warm-up rounds: code objects, scratch buffers, the counter
            for name, fn in zip(walls, calls):
                t = time.perf_counter()
                fn()
                if rep >= 2:
                    walls[name].append((time.perf_counter() - t) * 1e3)
        # the sum alone
        parts = [torch.randint(-500, 501, (n_val,), device="cuda", dtype=torch.int16) for _ in range(C)]
        gk = np.ascontiguousarray(g_diff[:, :C])
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t_sum, t_copy = [], []
        nbytes = (C + 1) * 2 * n_val
        a_buf = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda")
        b_buf = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda")
        for rep in range(a.reps + 2):
            t0.record(stream)
            eng.iq_wsum([x.data_ptr() for x in parts], gk, out.data_ptr())
            t1.record(stream)
            t1.synchronize()
            if rep >= 2:
                t_sum.append(t0.elapsed_time(t1))
            with torch.cuda.stream(stream):
                t0.record(stream)
                b_buf.copy_(a_buf)
                t1.record(stream)
            t1.synchronize()
            if rep >= 2:
                t_copy.append(t0.elapsed_time(t1))
        eng.iq_saturated()
        eng.set_stream(None)
    print("%d satellites x %d epochs = %.2f M samples, %d repetitions (ms: median, min .. max)" % (C, E, E * N / 1e6, a.reps))
    for name, t in walls.items():
        t = np.array(t)
        print("  %-24s %9.3f  %9.3f .. %9.3f" % (name, np.median(t), t.min(), t.max()))
    pa, pb = np.median(walls["plain (a)"]), np.median(walls["plain (b)"])
    print("  scatter of the plain call: medians %.3f and %.3f ms (%.2f %%)" % (pa, pb, 100.0 * abs(pa - pb) / min(pa, pb)))
    print("  run_gains / plain: %.2f (%d columns), %.2f (unity)" % (np.median(walls["run_gains, %d columns" % C]) / min(pa, pb), C,
                                                                   np.median(walls["run_gains, unity"]) / min(pa, pb)))
    ts, tc = np.array(t_sum), np.array(t_copy)
    print("  k_iq_wsum, %d parts:      %9.3f  %9.3f .. %9.3f   %.3g bytes/s over %.3g bytes" % (C, np.median(ts), ts.min(), ts.max(),
                                                                                              nbytes / np.median(ts) * 1e3, nbytes))
    print("  copy of as many bytes:   %9.3f  %9.3f .. %9.3f   %.3g bytes/s" % (np.median(tc), tc.min(), tc.max(), nbytes / np.median(tc) * 1e3))
    return 0


if __name__ == "__main__":
    sys.exit(main())
