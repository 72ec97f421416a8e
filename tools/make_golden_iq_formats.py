#!/usr/bin/env python3
"""Writes tests/golden/iq_format_md5.json: the 8-bit and 1-bit IQ formats (include/galsynth.h GAL_IQ_IBYTE / GAL_IQ_IBIT) of the
reference program's own output for G1 and G2, so that the CLI's --iq-format files are tied to the reference's bytes.

    python tools/make_golden_iq_formats.py        (CPU only; needs oracle/_ref/ref_task, which build() makes where the reference lies)

For each scenario: oracle/_ref/ref_task (the reference's file-sink program) writes its int16 file, whose md5 must equal
tests/golden/reference_md5.json; the definitions of the formats are then applied in numpy (ibyte at shifts 4, 5 and 6, ibit) and
each result's md5, byte count and saturated count recorded, with the command lines.  Prints the saturated fraction per shift.
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ref_task_goldens import ARGS, REF, run_ref_task  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "iq_format_md5.json")
SHIFTS = (4, 5, 6)


def ibyte(x, s):
    """(int8) clamp((x + r) >> s, -127, 127), r = s ? 1 << (s - 1) : 0, in int32; returns (bytes, saturated count)."""
    r = (1 << (s - 1)) if s else 0
    v = (x.astype(np.int32) + r) >> s
    return np.clip(v, -127, 127).astype(np.int8).tobytes(), int(np.count_nonzero((v < -127) | (v > 127)))


def ibit(x):
    """numpy.packbits(x > 0): byte k = x[8k] .. x[8k+7], x[8k] in bit 7."""
    return np.packbits(x > 0).tobytes()


def main():
    binary = os.path.join(ROOT, "oracle", "_ref", "ref_task")
    if not os.path.exists(binary):
        sys.exit("oracle/_ref/ref_task is not built (make -C oracle ref, with the reference tree present)")
    doc = {
        "source": "tools/make_golden_iq_formats.py: the reference program's int16 file (oracle/_ref/ref_task, md5 checked against "
                  "reference_md5.json) converted by the definitions of include/galsynth.h GAL_IQ_IBYTE / GAL_IQ_IBIT in numpy",
        "ref_task_command": "ref_task -e 20feb2022.rnx <args> -U 1 -b 1 -o <file>",
        "cli_command": "galileo-sdr-sim -e 20feb2022.rnx <args> --iq-format ibyte --iq-shift <s> | --iq-format ibit -o <file>",
    }
    with tempfile.TemporaryDirectory() as d:
        for name in ("G1", "G2"):
            path = os.path.join(d, name + ".ishort")
            md5, n, _, _ = run_ref_task(binary, ARGS[name], path)
            if md5 != REF[name]["md5"] or n != REF[name]["bytes"]:
                sys.exit("%s: ref_task wrote %s (%d B), reference_md5.json has %s" % (name, md5, n, REF[name]["md5"]))
            x = np.fromfile(path, dtype="<i2")
            entry = {"args": ARGS[name], "ishort": {"md5": md5, "bytes": n}, "values": int(x.size)}
            for s in SHIFTS:
                b, sat = ibyte(x, s)
                entry["ibyte_shift%d" % s] = {"md5": hashlib.md5(b).hexdigest(), "bytes": len(b), "saturated": sat}
                print("%s ibyte shift %d: %d of %d values saturated (%.3g)" % (name, s, sat, x.size, sat / x.size), flush=True)
            b = ibit(x)
            entry["ibit"] = {"md5": hashlib.md5(b).hexdigest(), "bytes": len(b), "saturated": 0}
            print("%s rms %.1f LSB, max |x| %d" % (name, float(np.sqrt(np.mean(x.astype(np.float64) ** 2))), int(np.abs(x.astype(np.int32)).max())))
            doc[name] = entry
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
