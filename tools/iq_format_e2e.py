#!/usr/bin/env python3
"""Measurements of the IQ output formats (--iq-format ishort | ibyte | ibit) on the MI355X.  One JSON line per measurement.

    python tools/iq_format_e2e.py kernel [--reps R]
        One conversion of BASELINE config 1's batch (1199 epochs x 260 000 = 311.74 M complex samples) into ibyte and ibit, and the
        CLI's per-batch conversion (128 epochs), timed with device events on the handle's stream.  Bytes moved: int16 in + format
        out; the share is of 6.29 TB/s, the measured float4-copy rate of the chip's HBM.  Run it under `rocprofv3 --kernel-trace --stats` for the
        kernel times of the profiler (k_iq_pass<FmtByte, 0, false>, k_iq_pass<FmtBit, 0, false> of csrc/iq_pass.hip).  Then the same with
        the noise floor at 45 dB-Hz mixed in (ishort in place, ibyte at shift 7, ibit; k_iq_pass<Fmt, 1, false>), beside the plain legs in
        the same process.
    python tools/iq_format_e2e.py cli [--reps R] [--dir D]
        The CLI on config 1 (-l -6,51,100 -t 2022/02/20,12:00:00 -d 120) in each format, into /dev/null and into a file under D
        (default /dev/shm, a tmpfs), alternating formats; the rate is the CLI's own "Process time" figure (samples / s).
    python tools/iq_format_e2e.py cli-noise [--reps R] [--cli OTHER]
        The CLI on config 1 into /dev/null, ishort without and with --cn0 45, alternating; --cli names a second executable (another
        build of the CLI) whose plain ishort run goes into the same alternation.
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
HBM_TBS = 6.29
CONFIG1 = ["-l", "-6,51,100", "-t", "2022/02/20,12:00:00", "-d", "120", "-U", "1", "-b", "1", "-P", "0"]


def kernel(reps):
    import torch

    from __graft_entry__ import load_pkg

    pkg = load_pkg()
    n_full = 1199 * 260000
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    # int16 IQ with the spread of the reference geometry (sigma ~750 LSB)
    x = (torch.randn(2 * n_full, device="cuda", generator=g) * 750).round().clamp(-32768, 32767).to(torch.int16)
    out = torch.empty(2 * n_full, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with pkg.SynthEngine(device=0) as eng, torch.cuda.stream(stream):
        eng.set_stream(stream.cuda_stream)
        for n, what in ((n_full, "config1_batch"), (128 * 260000, "cli_batch_128_epochs")):
            noise = dict(pkg.noise_from_cn0(45.0, 2.6e6), seed=1)
            legs = [("ibyte", None), ("ibit", None), ("ishort", noise), ("ibyte", noise), ("ibit", noise)]
            for fmt, nz in legs + legs:
                s = (7 if nz else 5) if fmt == "ibyte" else 0
                # ishort with noise: in place, as the CLI runs it (the buffer is noise on noise after the first pass: the same work)
                dst = x.data_ptr() if fmt == "ishort" else out.data_ptr()
                for _ in range(3):
                    eng.iq_convert(x.data_ptr(), n, fmt, s, dst, noise=nz)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                for _ in range(reps):
                    eng.iq_convert(x.data_ptr(), n, fmt, s, dst, noise=nz)
                b.record(stream)
                b.synchronize()
                ms = a.elapsed_time(b) / reps
                nbytes = 4 * n + pkg.iq_bytes(fmt, n)
                print(json.dumps({"leg": "kernel", "what": what, "format": fmt, "noise": bool(nz), "samples": n, "bytes": nbytes,
                                  "ms": round(ms, 4), "TB_s": round(nbytes / ms / 1e9, 3),
                                  "share_of_6.29TB_s": round(nbytes / ms / 1e9 / HBM_TBS, 3)}), flush=True)
        eng.iq_saturated(reset=True)


def cli(reps, d):
    path = os.path.join(d, "iq_format_e2e_%d.out" % os.getpid())
    try:
        for rep in range(reps):
            for sink in ("/dev/null", path):
                for fmt in ("ishort", "ibyte", "ibit"):
                    r = subprocess.run([CLI, "-e", NAV] + CONFIG1 + ["-o", sink, "--iq-format", fmt], capture_output=True, text=True,
                                       timeout=600)
                    m = re.search(r"Process time = ([0-9.]+) \[sec\]\s+\(([0-9.]+) Msamples/s", r.stderr)
                    size = os.path.getsize(sink) if sink == path and os.path.exists(sink) else None
                    print(json.dumps({"leg": "cli", "rep": rep, "sink": "devnull" if sink == "/dev/null" else "tmpfs_file", "format": fmt,
                                      "rc": r.returncode, "s": float(m.group(1)) if m else None,
                                      "Gsamples_s": round(float(m.group(2)) / 1e3, 3) if m else None, "file_bytes": size}), flush=True)
                    if r.returncode != 0:
                        sys.stderr.write(r.stderr[-2000:])
                        return 1
                    if sink == path:
                        os.unlink(path)
    finally:
        if os.path.exists(path):
            os.unlink(path)
    return 0


def cli_noise(reps, other):
    runs = [("ishort", CLI, []), ("ishort_cn0_45", CLI, ["--cn0", "45"])]
    if other:
        runs.append(("ishort_other_cli", other, []))
    for rep in range(reps):
        for name, exe, extra in runs:
            r = subprocess.run([exe, "-e", NAV] + CONFIG1 + ["-o", "/dev/null"] + extra, capture_output=True, text=True, timeout=600)
            m = re.search(r"Process time = ([0-9.]+) \[sec\]\s+\(([0-9.]+) Msamples/s", r.stderr)
            print(json.dumps({"leg": "cli-noise", "rep": rep, "run": name, "rc": r.returncode, "s": float(m.group(1)) if m else None,
                              "Gsamples_s": round(float(m.group(2)) / 1e3, 3) if m else None}), flush=True)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:])
                return 1
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=("kernel", "cli", "cli-noise"))
    ap.add_argument("--reps", type=int, default=0)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--cli", default=None)
    a = ap.parse_args()
    if a.leg == "kernel":
        kernel(a.reps or 20)
        return 0
    if a.leg == "cli-noise":
        return cli_noise(a.reps or 3, a.cli)
    return cli(a.reps or 2, a.dir)


if __name__ == "__main__":
    sys.exit(main())
