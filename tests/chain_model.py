"""The output chain behind the synthesis as galileo-sdr-sim's run_chain strings it together (csrc/cli_main.cpp), in
numpy -- TEST INFRASTRUCTURE: the product never imports this.  No arithmetic is stated here: every stage is the model its kernel is
held against (interf_model / noise_model, osc_model, fir_model, firdec_model, agc_model).  What this module states is what lies
between them:

  the order     1. noise floor and interference, as ishort       2. the oscillator
                3. the FIR filter, or with decim > 1 the decimator    4. the AGC with the format, or the format alone
  the absences  a stage that is not asked for is not there; a chain without any stage is the format of the stream as it is
  the fusing    where the mix is the last stage, ONE pass mixes and formats: a value that both clamps change counts once
  the state     the stream comes in pieces, as the command's batches do: every stage counts the samples it has seen (the mix's and the
                oscillator's first_sample, the decimator's position modulo M, the AGC's position in its block) and keeps what the next
                piece needs (the oscillator's random-walk sum, the last T - 1 inputs of the filter, the AGC's window and open block)

Chain(...).push(x) takes the next piece of the front stream and returns (bytes, AGC gains, saturated count over the stages); run() is
push() over a list of cuts.  `order` is run_chain's; the tests hand in another one only to show that their input tells the orders
apart."""
import numpy as np

import agc_model
import fir_model
import firdec_model
import interf_model
import osc_model

ORDER = ("mix", "osc", "fir", "agc")


class Chain:
    """fmt: "ishort", "ibyte" (param: the shift), "ibit", or with an AGC "i2bit" (param: the threshold).
    noise: (seed, stream, gain_q16, sigma_q4) or None; interf: interf_model sources -- either switches the mix on.
    osc: an osc_model dict.  taps with decim == 1: the FIR filter; with decim > 1: the decimator.  agc: agc_model parameters."""

    def __init__(self, fmt="ishort", param=0, noise=None, interf=(), osc=None, taps=None, decim=1, agc=None, order=ORDER):
        assert sorted(order) == sorted(ORDER) and (decim == 1 or taps is not None) and (fmt != "i2bit" or agc is not None)
        self.fmt, self.param, self.noise, self.interf, self.osc, self.decim, self.agc = fmt, int(param), noise, list(interf), osc, int(decim), agc
        self.taps = None if taps is None else np.asarray(taps, dtype=np.int16)
        on = {"mix": noise is not None or len(self.interf) > 0, "osc": osc is not None, "fir": taps is not None, "agc": agc is not None}
        self.stages = [s for s in order if on[s]]
        self.seen = dict.fromkeys(ORDER, 0)  # complex samples each stage has taken so far
        self.osc_z = 0
        self.hist = np.zeros(0, dtype=np.int16)
        self.agc_stream = agc_model.Stream(agc) if agc is not None else None

    def _stage(self, name, x, last):
        """One stage over the next piece x of ITS input; returns (int16 stream or, from a last stage that formats, bytes; the clamp
        flags that the format behind a last mix still has to count, or None; gains; saturated)."""
        first = self.seen[name]
        self.seen[name] += x.size // 2
        none = np.zeros(0, dtype=np.uint32)
        if name == "mix":
            y, clipped = interf_model.mix(x, self.noise, self.interf, first)
            return (y, clipped, none, 0) if last else (y, None, none, int(np.count_nonzero(clipped)))
        if name == "osc":
            y, sat, self.osc_z = osc_model.rotate(x, self.osc, 0, first, self.osc_z)
            return y, None, none, sat
        if name == "fir":
            if self.decim > 1:
                y, sat = firdec_model.firdec(x, self.taps, self.decim, first, self.hist)
            else:
                y, sat = fir_model.fir(x, self.taps, self.hist)
            self.hist = np.concatenate([self.hist, x])[-2 * (self.taps.size - 1):] if self.taps.size > 1 else self.hist
            return y, None, none, sat
        out, gains, sat = self.agc_stream.call(x, self.fmt, self.param) if last else self.agc_stream.call(x, "ishort", 0)
        return (out if last else out.view("<i2").astype(np.int16)), None, gains, sat

    def push(self, x):
        x = np.asarray(x, dtype=np.int16)
        assert x.ndim == 1 and x.size % 2 == 0
        clipped, gains, total = None, np.zeros(0, dtype=np.uint32), 0
        for k, name in enumerate(self.stages):
            x, clipped, g, sat = self._stage(name, x, k == len(self.stages) - 1)
            gains = np.concatenate([gains, g])
            total += sat
        if self.stages and self.stages[-1] == "agc":
            return x, gains, total
        out, sat = interf_model.formatted(x, np.zeros(x.size, dtype=bool) if clipped is None else clipped, self.fmt, self.param)
        return np.ascontiguousarray(out, dtype=np.uint8), gains, total + sat

    def run(self, x, cuts=()):
        """push() over pieces of the lengths `cuts` (complex samples), then the rest: (bytes, gains, saturated) of the whole stream."""
        x = np.asarray(x, dtype=np.int16)
        outs, gains, total, at = [], [], 0, 0
        for c in list(cuts) + [x.size // 2 - sum(cuts)]:
            o, g, s = self.push(x[2 * at: 2 * (at + c)])
            outs.append(o)
            gains.append(g)
            total += s
            at += c
        assert at == x.size // 2
        return np.concatenate(outs), np.concatenate(gains), total
