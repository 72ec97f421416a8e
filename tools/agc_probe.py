"""Device-event timings of gal_synth_iq_agc (three launches) beside the plain ibyte conversion on the same buffers."""
import sys, os, statistics
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_pkg
pkg = load_pkg()
torch.cuda.init()
def timed(fn, reps=15, warm=3):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)
st = torch.cuda.Stream()
torch.cuda.set_stream(st)
assert st.cuda_stream != 0
with pkg.SynthEngine(samples_per_epoch=26000, n_slots=16, device=0) as eng:
    eng.set_stream(st.cuda_stream)
    p = pkg.synth.agc_from_rms(1024.0, 750.0, 2600, 8)
    eng.agc_set(p)
    for n in (128 * 260000, 311740000):
        x = (torch.randn(2 * n, device="cuda") * 750).to(torch.int16)
        out = torch.empty(4 * n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        print("n = %d samples" % n)
        for name, fn in (("plain ibyte convert", lambda: eng.iq_convert(x.data_ptr(), n, "ibyte", 5, out.data_ptr())),
                         ("agc ishort", lambda: eng.iq_agc(x.data_ptr(), n, "ishort", 0, out.data_ptr())),
                         ("agc ibyte", lambda: eng.iq_agc(x.data_ptr(), n, "ibyte", 5, out.data_ptr())),
                         ("agc i2bit", lambda: eng.iq_agc(x.data_ptr(), n, "i2bit", 1024, out.data_ptr())),
                         ("plain ibit convert", lambda: eng.iq_convert(x.data_ptr(), n, "ibit", 0, out.data_ptr())),
                         ("d2d copy of the input", lambda: out[: 4 * n].copy_(x.view(torch.uint8)))):
            med, lo, hi = timed(fn)
            print("  %-24s %8.3f ms (%.3f .. %.3f)  %.1f Gsamples/s" % (name, med, lo, hi, n / med / 1e6))
        eng.iq_saturated()
        del x, out
