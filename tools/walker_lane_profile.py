#!/usr/bin/env python3
"""Where do the lanes of k_walk_carr / k_verify_carr go?  

Runs the product's own carrier walker (csrc/nco_walk.h compiled for the host, libgalwalk_host.so: galwalk_lane_profile) over
M-SYN12's own parameters -- shard.rank_workload(0, 1199), 8 legs per epoch -- with the kernels' thread -> (slot, leg) mapping, groups
the legs into the 64-lane waves the kernels form, and reports per kernel
  (a) trip-count imbalance: a wave runs each loop as often as its slowest lane (max against mean closed-form iterations), and
  (b) divergence inside an iteration: in how many of the wave's iterations a branch of the loop body is taken by SOME lane (the
      wave then executes it) against how many lanes take it.

    python tools/walker_lane_profile.py [epochs] [legs_per_epoch] > profiles/<tag>_walker_lanes.log        CPU only, ~10 s
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_pkg  # noqa: E402

pkg = load_pkg()
W = ctypes.CDLL(os.path.join(ROOT, "galileo-sdr-sim_amd", "libgalwalk_host.so"))
COLS = 18
N, R, RATE = 260000, 1024, 2.6e6
E = int(sys.argv[1]) if len(sys.argv) > 1 else 1199
LEGS_PER_EPOCH = int(sys.argv[2]) if len(sys.argv) > 2 else 8
nchunks = (N + R - 1) // R
Lc = (nchunks + LEGS_PER_EPOCH - 1) // LEGS_PER_EPOCH
Wl = (nchunks + Lc - 1) // Lc
p = pkg.shard.rank_workload(0, E)
S = 12  # the active slots (idle slots are whole waves that leave at once)
dstep = np.ascontiguousarray(p["f_carr"][:, :S].astype(np.float64) * (1.0 / RATE))  # the plan's d = f_carr * delt, one rounding
root = np.ascontiguousarray(p["carr_phase0"][0, :S].astype(np.float64))
nw_max = (E * Wl * S + 63) // 64
W.galwalk_lane_profile.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]

print("M-SYN12: %d epochs x %d slots, %d samples per epoch, checkpoints every %d, %d legs per epoch of %d chunks: %d legs, %d waves of 64"
      % (E, S, N, R, Wl, Lc, E * Wl * S, nw_max))
print("|d| per slot (first epoch): " + " ".join("%.2e" % abs(x) for x in dstep[0]))
for mode, name in ((0, "k_walk_carr (first pass: anchor -> leg start, then the leg)"), (1, "k_verify_carr (every leg from its first checkpoint)")):
    out = np.zeros((nw_max, COLS))
    nw = W.galwalk_lane_profile(E, S, Wl, Lc, N, R, dstep.ctypes.data, root.ctypes.data, mode, out.ctypes.data, nw_max)
    assert nw == nw_max, nw
    out = out[out[:, 0] > 0]
    lanes, wave_it, lane_it, longest = out[:, 0], out[:, 1], out[:, 2], out[:, 3]
    t = out.sum(axis=0)
    print("\n== %s" % name)
    print("waves with work %d, lanes with work %d (%.1f per wave)" % (len(out), t[0], t[0] / len(out)))
    print("closed-form iterations: %.0f lane iterations = %.1f per leg = %.0f per (slot, epoch) record" % (t[2], t[2] / t[0], t[2] / t[0] * Wl))
    print("(a) trip counts:  wave iterations %.0f (sum over waves of what the slowest lane of every loop needs)" % t[1])
    print("    lane utilisation  lane iterations / (64 x wave iterations)            = %.4f" % (t[2] / (64 * t[1])))
    print("    ... counting only the lanes that have a leg (a partial last wave)      = %.4f" % (t[2] / (lanes * wave_it).sum()))
    print("    ... if every lane's loops were one loop (longest lane instead)         = %.4f" % (t[2] / (64 * longest.sum())))
    r = lane_it / (lanes * wave_it)
    print("    per wave: utilisation min %.3f  5%% %.3f  median %.3f  max %.3f" % (r.min(), np.percentile(r, 5), np.median(r), r.max()))
    print("    per wave: iterations of the slowest lane min %.0f median %.0f max %.0f; mean lane min %.1f median %.1f max %.1f"
          % (wave_it.min(), np.median(wave_it), wave_it.max(), (lane_it / lanes).min(), np.median(lane_it / lanes), (lane_it / lanes).max()))
    print("(b) branches of the loop body: wave iterations in which SOME lane takes it / lanes that take it, per wave iteration")
    for k, label in ((4, "genuine step wraps"), (6, "genuine step crosses a binade"), (8, "checkpoint at the iteration start"),
                     (12, "no closed-form batch (n == 0)"), (14, "tie bookkeeping"), (16, "general loop (phase against the step)")):
        print("    %-40s wave %8.0f (%.4f of wave iterations)   lanes %10.0f (%.2f of 64 when taken)"
              % (label, t[k], t[k] / t[1], t[k + 1], t[k + 1] / max(t[k], 1)))
    print("    %-40s wave %8.0f trips (%.4f per wave iteration)   lanes %10.0f (%.4f per lane iteration)"
          % ("checkpoint loop inside the batch", t[10], t[10] / t[1], t[11], t[11] / t[2]))
    print("    by slot (waves are cut every 64 threads, so a few straddle two slots):")
    per = len(out) / S
    for s in range(S):
        o = out[int(round(s * per)):int(round((s + 1) * per))]
        if len(o) == 0:
            continue
        ts = o.sum(axis=0)
        print("      slot %2d |d| %.2e: %6.1f iterations per leg, utilisation %.4f, wrap-step waves %.3f, checkpoint trips per wave iteration %.3f (lanes %.3f)"
              % (s, abs(dstep[0, s]), ts[2] / ts[0], ts[2] / (o[:, 0] * o[:, 1]).sum(), ts[4] / ts[1], ts[10] / ts[1], ts[11] / ts[2]))
