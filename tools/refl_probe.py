#!/usr/bin/env python3
"""Probe of the reflector pass (gal_synth_iq_refl, k_iq_refl of csrc/iq_refl.hip) on the MI355X against the echo pass
(gal_synth_iq_mpath, k_iq_echo) at an equal echo count, on the CLI's batch: the same 12 parts of 128 epochs x 260 000 complex samples
and the same 12 echoes for both.  Each call is timed between two HIP events on the engine's stream, 3 warm-up rounds and then --reps
(at least 20) timed ones, the cases alternating in one process.  Measured: gal_synth_iq_mpath with 12 echoes (the yardstick);
gal_synth_iq_refl with the same rows (F = 0: the same bytes); gal_synth_iq_refl with a fraction on every echo (F > 0); a device copy
of the pass's bytes (12 parts in, one stream out: 13 buffers' worth moved by hipMemcpyAsync, the rate a pass that only streams could
reach); and the yardstick in a second interleaved series, whose median's distance from the first is the run-to-run scatter to judge
the rest by.  Median and range per line, the ratio to the echo pass, and the kernel source's SHA-256.  With --out the lines are also
written to that file (profiles/).  Run it under a time limit of its own:
    timeout -k 10 500 python tools/refl_probe.py --out profiles/refl_probe.log"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 260000
PARTS = 12
ECHOES = 12
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
    E = a.epochs
    rng = np.random.default_rng(23)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(23)
    parts = [torch.randint(-500, 501, (2 * E * N,), dtype=torch.int16, device="cuda", generator=gen) for _ in range(PARTS)]
    out = torch.zeros(2 * E * N, dtype=torch.int16, device="cuda")
    sink = torch.zeros(2 * E * N, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ptrs = [p.data_ptr() for p in parts]
    gains = rng.integers(60, 300, size=(E, PARTS))
    # what --reflector makes: delays of a few samples with every residue modulo 4, phases that turn slowly
    refl = np.zeros((E, ECHOES), dtype=pkg.REFL_DTYPE)
    refl["gain_q7"] = rng.integers(20, 120, size=refl.shape)
    refl["delay"] = (np.arange(ECHOES) % 8)[None, :]
    refl["ph0"] = rng.integers(0, 1 << 32, size=refl.shape, dtype=np.uint64)
    refl["dph"] = rng.integers(-4000, 4000, size=ECHOES)[None, :]
    echo = np.zeros((E, ECHOES), dtype=pkg.ECHO_DTYPE)
    for k in ("gain_q7", "delay", "ph0", "dph"):
        echo[k] = refl[k]
    frac = refl.copy()
    frac["frac_q12"] = rng.integers(1, 4096, size=frac.shape)
    pof = np.arange(ECHOES) % PARTS
    n_bytes = 4 * E * N
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {}

    def timed(name, fn, rep):
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        if rep >= WARM:
            res.setdefault(name, []).append(t0.elapsed_time(t1))

    def copies():
        with torch.cuda.stream(stream):
            for _ in range(6):  # 6 copies read and write a buffer each: 12 buffers' worth, and a half one more for the 13th
                sink.copy_(parts[0], non_blocking=True)
            sink[:E * N].copy_(parts[1][:E * N], non_blocking=True)

    with pkg.SynthEngine(device=0) as eng:
        stream = torch.cuda.Stream()
        eng.set_stream(stream.cuda_stream)
        for rep in range(a.reps + WARM):
            timed("iq_mpath 12 echoes (the yardstick)", lambda: eng.iq_mpath(ptrs, gains, out.data_ptr(), pof, echo), rep)
            timed("iq_refl  12 echoes, F = 0", lambda: eng.iq_refl(ptrs, gains, out.data_ptr(), pof, refl), rep)
            timed("iq_refl  12 echoes, F > 0", lambda: eng.iq_refl(ptrs, gains, out.data_ptr(), pof, frac), rep)
            timed("device copy of 13 buffers' bytes", copies, rep)
            timed("iq_mpath 12 echoes, second series", lambda: eng.iq_mpath(ptrs, gains, out.data_ptr(), pof, echo), rep)
        sat = eng.iq_saturated()
        eng.set_stream(None)
    src = os.path.join(ROOT, "galileo-sdr-sim_amd", "csrc", "iq_refl.hip")
    lines = ["%d parts x %d epochs x %d complex samples, %d echoes, %d repetitions after %d warm-up rounds (ms: median, min .. max); %d values clamped"
             % (PARTS, E, N, ECHOES, a.reps, WARM, sat),
             "csrc/iq_refl.hip sha256 %s" % hashlib.sha256(open(src, "rb").read()).hexdigest(), "device: %s" % torch.cuda.get_device_name(0)]
    base = float(np.median(res["iq_mpath 12 echoes (the yardstick)"]))
    for name, ts in res.items():
        t = np.array(ts)
        lines.append("  %-40s %8.3f  %8.3f .. %8.3f   %.3f x iq_mpath   %.3g bytes/s of parts and output" % (
            name, np.median(t), t.min(), t.max(), np.median(t) / base, (PARTS + 1.0) * n_bytes / np.median(t) * 1e3))
    s2 = float(np.median(res["iq_mpath 12 echoes, second series"]))
    lines.append("  scatter: two interleaved series of the yardstick differ by %.3f ms in the median (%.2f %%)" % (abs(base - s2), 100.0 * abs(base - s2) / base))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
