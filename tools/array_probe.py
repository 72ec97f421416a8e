#!/usr/bin/env python3
"""Probe of the array pass (gal_synth_iq_array, k_iq_array of csrc/iq_array.hip) on the MI355X at the CLI's own shape: 12 parts of 128
epochs x 260 000 complex samples, K = 1, 4 and 8 elements with weights that turn (inside the int32 bound), every call ONE launch, timed
between two HIP events on the engine's stream.  Beside it, alternating in the same process: K calls of gal_synth_iq_wsum on the same
parts -- the nearest thing there was before the pass -- and a device-to-device copy as the yardstick of the card (whole streams: where P + K is odd it moves half a stream less than the pass, so
the pass is compared with the copy's time scaled to the pass's bytes).
Per complex sample the pass moves 4 (P + K) bytes and K weighted sums 4 K (P + 1).  Median and range per line, the bytes moved, GB/s,
the share of the 8 TB/s HBM peak, and the kernel source's SHA-256.  With --out the lines are also written to that file (profiles/).
Run it under a time limit of its own:
    timeout -k 10 300 python tools/array_probe.py --out profiles/array_probe.log"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SPE, E, P = 260000, 128, 12
WARM = 3
HBM_PEAK = 8.0e12  # bytes per second


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
    gen.manual_seed(22)
    n = SPE * E
    parts = [torch.randint(-500, 501, (2 * n,), dtype=torch.int16, device="cuda", generator=gen) for _ in range(P)]
    outs = [torch.zeros(2 * n, dtype=torch.int16, device="cuda") for _ in range(8)]
    torch.cuda.synchronize()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    src = os.path.join(ROOT, "galileo-sdr-sim_amd", "csrc", "iq_array.hip")
    say("array_probe: %s, iq_array.hip sha256 %s" % (torch.cuda.get_device_name(0), hashlib.sha256(open(src, "rb").read()).hexdigest()[:16]))
    say("shape: %d parts, %d epochs x %d samples = %.1f MB per stream" % (P, E, SPE, 4.0 * n / 1e6))
    rng = np.random.default_rng(1)
    gains = rng.integers(64, 257, size=(E, P))
    pp = [t.data_ptr() for t in parts]
    with pkg.SynthEngine(samples_per_epoch=SPE, n_slots=16, device=0) as eng:
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

        def line(name, t, nbytes):
            med = float(np.median(t))
            rate = nbytes / med * 1e3
            say("%-22s: median %8.4f ms (%8.4f .. %8.4f)  %7.1f MB moved  %7.1f GB/s  %4.1f %% of the HBM peak" % (
                name, med, t.min(), t.max(), nbytes / 1e6, rate / 1e9, 100.0 * rate / HBM_PEAK))
            return med

        say("timing: HIP events on the engine's stream; %d warm-up + %d timed calls per line" % (WARM, a.reps))
        for K in (1, 4, 8):
            phase = rng.integers(0, 1 << 32, size=(E, K, P), dtype=np.uint64)
            w = np.zeros((E, K, P, 2), dtype=np.int64)
            for e in range(E):
                for k in range(K):
                    for s in range(P):
                        w[e, k, s] = pkg.steer_make(int(gains[e, s]), int(phase[e, k, s]))
            oo = [t.data_ptr() for t in outs[:K]]
            b_pass, b_sums = 4.0 * n * (P + K), 4.0 * n * K * (P + 1)

            def copy():  # the pass's bytes: (P + K) / 2 streams read and written
                for j in range((P + K) // 2):
                    outs[j % 8].copy_(parts[j % P], non_blocking=True)

            def sums():
                for k in range(K):
                    eng.iq_wsum(pp, gains, oo[k])

            b_copy = 8.0 * n * ((P + K) // 2)
            t_c = line("K=%d  copy of %d streams" % (K, (P + K) // 2), timed(copy), b_copy) * b_pass / b_copy  # at the pass's bytes
            t_s = line("K=%d  %d x iq_wsum" % (K, K), timed(sums), b_sums)
            t_a = line("K=%d  iq_array" % K, timed(lambda: eng.iq_array(pp, w, oo)), b_pass)
            say("K=%d  iq_array takes %.2f x the time of %d weighted sums and moves %.2f x their bytes; %.2f x the copy's time at equal bytes" % (
                K, t_a / t_s, K, b_pass / b_sums, t_a / t_c))
        eng.iq_saturated()
        eng.set_stream(None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
