#!/usr/bin/env python3
"""Probe of the scintillation pass (gal_synth_iq_scint, k_iq_scint of csrc/iq_scint.hip) on the MI355X: 1, 4 and 12 jobs of 2 080 000
complex samples each -- the CLI's default batch of 8 epochs at 2.6 MS/s --, in place, every call ONE launch, timed between two HIP
events on the engine's stream.  The yardstick, alternating with them in the same process and never the code under test: a
device-to-device copy of the same bytes (4 in + 4 out per complex sample, the traffic of the pass).  tools/wrcal.hip's coalesced fill
is the write-only figure of the same card; it prints no time of its own (rocprofv3 --kernel-trace --stats -- tools/wrcal gives it).
Rows: L = 64 (18 nodes and 49 draws per tile: the most node work there is), L = 162 500 (tau0 = 0.5 s: what the CLI runs) and B = 0
(no draws).  Median and range per line, GB/s, the ratio to the copy, and the kernel source's SHA-256.  With --out the lines are also
written to that file (profiles/).  Run it under a time limit of its own:
    timeout -k 10 300 python tools/scint_probe.py --out profiles/scint_probe.log"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 2080000
WARM = 3


def main():
    import numpy as np
    import torch

    from __graft_entry__ import load_pkg

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    pkg = load_pkg()
    torch.cuda.init()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20)
    bufs = [torch.randint(-500, 501, (2 * N,), dtype=torch.int16, device="cuda", generator=gen) for _ in range(12)]
    dst = [torch.zeros(2 * N, dtype=torch.int16, device="cuda") for _ in range(12)]
    torch.cuda.synchronize()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    src = os.path.join(ROOT, "galileo-sdr-sim_amd", "csrc", "iq_scint.hip")
    say("scint_probe: %s, iq_scint.hip sha256 %s" % (torch.cuda.get_device_name(0), hashlib.sha256(open(src, "rb").read()).hexdigest()[:16]))
    rows = {"L=64": dict(pkg.scint_make(0.8, 64 * 8 / 2.6e6), seed=3), "L=162500": dict(pkg.scint_make(0.8, 0.5), seed=3),
            "B=0": dict(node_len=162500, a_q12=3000, b_q12=0)}
    with pkg.SynthEngine(samples_per_epoch=260000, n_slots=16, device=0) as eng:
        stream = torch.cuda.Stream()
        eng.set_stream(stream.cuda_stream)

        def timed(fn):
            ms = []
            for _ in range(WARM + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                with torch.cuda.stream(stream):
                    e0.record()
                    fn()
                    e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            return np.array(ms[WARM:])

        say("timing: HIP events on the engine's stream; %d warm-up + %d timed calls per line" % (WARM, a.reps))
        for n_jobs in (1, 4, 12):
            gb = 8.0 * N * n_jobs / 1e9

            def copy():
                for k in range(n_jobs):
                    dst[k].copy_(bufs[k], non_blocking=True)

            t_copy = timed(copy)
            med_c = float(np.median(t_copy))
            say("%2d jobs  copy      : median %.4f ms (%.4f .. %.4f)  %.1f GB/s" % (n_jobs, med_c, t_copy.min(), t_copy.max(), gb / med_c * 1e3))
            for name, row in rows.items():
                jobs = [(bufs[k].data_ptr(), bufs[k].data_ptr(), N, 0, dict(row, stream=k)) for k in range(n_jobs)]
                t = timed(lambda: eng.iq_scint(jobs))
                med = float(np.median(t))
                say("%2d jobs  %-10s: median %.4f ms (%.4f .. %.4f)  %.1f GB/s  %.2f x the copy's time" % (
                    n_jobs, name, med, t.min(), t.max(), gb / med * 1e3, med / med_c))
        eng.iq_saturated()
        eng.set_stream(None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
