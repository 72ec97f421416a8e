#!/usr/bin/env python3
"""Probe of the correlator bank (gal_synth_correlate) on the MI355X: one full-code acquisition of a PRN -- 8184 delays x 41 Doppler
bins x 1 code period of ishort -- and the tracking-shaped call the CLI's --monitor makes -- 12 channels x (3 + 1) delays x 3 bins x
25 periods --, each timed with events over `--reps` calls, the peak printed.  Kernel times proper:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/iq_corr_probe.py --child acq     (or: --child track)
Without --child the two steps run as child processes, each under its own timeout, and the second is not started if the first fails."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS = 2.6e6
BIN = round(250.0 / FS * 2 ** 32)


def child(step, reps):
    import numpy as np
    import torch

    from __graft_entry__ import load_pkg

    pkg = load_pkg()
    torch.cuda.init()
    p = pkg.workloads.m_syn12(n_epochs=1)
    with pkg.SynthEngine(device=0) as eng:
        x, _, _ = eng.run_host(p)
        n = x.size // 2
        xd = torch.from_numpy(x).cuda()
        if step == "acq":
            # one whole period: period 1 of the buffer (max_periods 2), 41 bins of 250 Hz around the plan
            reqs = [pkg.corr_from_epoch(p[0, 0], FS, 0, max_periods=2, n_delay=8184, dopp0=-20 * BIN, dopp_step=BIN, n_dopp=41)]
            ops = 8184 * 41 * 10400 * 4
        else:
            reqs = []
            for s in range(12):
                base = pkg.corr_from_epoch(p[0, s], FS, 0, max_periods=25, dopp0=-BIN, dopp_step=BIN, n_dopp=3)
                reqs += [dict(base, delay0=-1, n_delay=3), dict(base, delay0=2046, n_delay=1)]
            ops = 12 * 4 * 3 * 260000 * 4
        out = torch.zeros(sum(pkg.corr_out_bytes(q) for q in reqs) // 8, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        eng.correlate(xd.data_ptr(), "ishort", n, reqs, out_ptr=out.data_ptr())  # warm-up (tables, code objects)
        eng.iq_saturated()
        stream = torch.cuda.Stream()
        eng.set_stream(stream.cuda_stream)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(reps):
            t0.record(stream)
            eng.correlate(xd.data_ptr(), "ishort", n, reqs, out_ptr=out.data_ptr())
            t1.record(stream)
            t1.synchronize()
            times.append(t0.elapsed_time(t1))
        eng.set_stream(None)
        sums = out.cpu().numpy()
        ms = float(np.median(times))
        if step == "acq":
            a = sums.reshape(2, 41, 8184, 4)[1].astype(np.float64)
            power = (a ** 2).sum(axis=2)
            d, k = np.unravel_index(int(np.argmax(power)), power.shape)
            print("acquisition PRN %d: peak at Doppler bin %+d, delay %d half chips, peak / mean %.1f" % (reqs[0]["prn"], d - 20, k, power.max() / power.mean()))
        else:
            a = sums.reshape(12, 1200, 4)
            for s in range(12):
                cn0, ratio = pkg.corr_cn0(np.concatenate([a[s, :900].reshape(25, 3, 3, 4), a[s, 900:].reshape(25, 3, 1, 4)], axis=2),
                                          dict(reqs[2 * s], n_delay=4), 1, 3, 1, FS)
                print("track PRN %2d: Pp / Pn %.1f (no noise floor: the other 11 satellites are the floor; C/N0 figure %.1f dB-Hz)" % (reqs[2 * s]["prn"], ratio, cn0))
        print("%s: %d calls, median %.3f ms (min %.3f, max %.3f) from memset to last kernel; %.3g useful add/subtracts -> %.2f Tops/s"
              % (step, reps, ms, min(times), max(times), ops, ops / ms / 1e9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("acq", "track"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps)
        return 0
    for step in ("acq", "track"):
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", step, "--reps", str(a.reps)])
        if r.returncode != 0:
            print("step %s ended with status %d: stopping" % (step, r.returncode))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
