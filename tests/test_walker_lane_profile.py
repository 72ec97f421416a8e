"""galwalk_lane_profile (walk_host.cpp), the counting behind tools/walker_lane_profile.py and DESIGN.md section 5.3: its lane iterations
are the single-leg iteration counts of the walker itself, its wave iterations the slowest lane's, and it walks the true chain."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = 18


def test_lane_profile_counts_what_single_legs_cost(pkg):
    W = ctypes.CDLL(os.path.join(ROOT, "galileo-sdr-sim_amd", "libgalwalk_host.so"))
    d_, i_, vp = ctypes.c_double, ctypes.c_int, ctypes.c_void_p
    W.galwalk_lane_profile.argtypes = [i_] * 6 + [vp, vp, i_, vp, i_]
    W.galwalk_carr_iters.restype = ctypes.c_long
    W.galwalk_carr_iters.argtypes = [d_, d_, i_]
    W.galwalk_carr.restype = d_
    W.galwalk_carr.argtypes = [d_, d_, i_, i_, vp, vp]
    E, S, N, R, legs = 6, 3, 40000, 1024, 8
    nchunks = (N + R - 1) // R
    Lc = (nchunks + legs - 1) // legs
    Wl = (nchunks + Lc - 1) // Lc
    L = Lc * R
    rng = np.random.default_rng(5)
    dstep = np.ascontiguousarray(rng.uniform(2e-4, 1.3e-3, (E, S)) * np.array([1.0, -1.0, 1.0]))
    root = np.ascontiguousarray(np.array([0.25, -0.6, 0.0]))
    nw = (E * Wl * S + 63) // 64
    out = np.zeros((nw, COLS))
    assert W.galwalk_lane_profile(E, S, Wl, Lc, N, R, dstep.ctypes.data, root.ctypes.data, 1, out.ctypes.data, nw) == nw
    # verify mode: every leg from its own first checkpoint = the true phase there, taken from an independent walk of the chain
    lane_iters, n_legs = 0, 0
    for s in range(S):
        p = float(root[s])
        for e in range(E):
            cp = np.zeros(nchunks)
            d = float(dstep[e, s])
            p_end = W.galwalk_carr(p, d, N, R, cp.ctypes.data, None)
            for w in range(Wl):
                n = min(L, N - w * L)
                lane_iters += W.galwalk_carr_iters(float(cp[w * Lc]), d, n)
                n_legs += 1
            p = p_end
    assert out[:, 0].sum() == n_legs == E * Wl * S
    # (galwalk_carr_iters counts iterations of the general batch routine; the lean loop of the product's walk batches the same binades)
    assert out[:, 2].sum() == lane_iters
    assert np.all(out[:, 1] * out[:, 0] >= out[:, 2]) and np.all(out[:, 3] <= out[:, 1]) and np.all(out[:, 1] <= out[:, 2])
    # walk mode: the same legs plus the stretch from each leg's anchor, at most one carrier cycle in front of it
    out0 = np.zeros((nw, COLS))
    assert W.galwalk_lane_profile(E, S, Wl, Lc, N, R, dstep.ctypes.data, root.ctypes.data, 0, out0.ctypes.data, nw) == nw
    assert out0[:, 0].sum() == n_legs
    extra = out0[:, 2].sum() - out[:, 2].sum()
    assert 0 <= extra <= n_legs * 16
