"""tests/chain_model.py on its own (no GPU): over a random full-range stream, with parameters at which every stage clamps some values
and leaves most alone, the chain without a stage is the stream, the chain with one stage is that stage's model, any cut into pieces
gives the bytes, gains and count of one piece, and the input tells run_chain's order from its neighbours -- without that
tests/test_cli_chain_model_gpu.py could pass with the stages in another order."""
import numpy as np
import pytest

import agc_model
import chain_model
import fir_model
import firdec_model
import interf_model
import noise_model
import osc_model

N = 5000  # complex samples
BLOCK = 64  # the AGC's block
NOISE = (7, 3, 65536, 16 * 1500)
INTERF = [interf_model.source(amp_q4=16 * 3000, ph0=12345, f0=0x06000000),
          interf_model.source(amp_q4=16 * 2000, f0=0xF0000000, df=70000, sweep_len=300, pulse_period=700, pulse_on=250)]
OSC = osc_model.osc(seed=5, stream=2, p0=1 << 61, f=0x0123456789ABCDEF, d=1 << 40, s=1 << 44)
TAPS = fir_model.lowpass(1.0e6, 2.6e6, 25)
DEC_TAPS = firdec_model.default_taps(2)
AGC = agc_model.from_rms(20000, 15000, BLOCK, 4)
FULL = dict(noise=NOISE, interf=INTERF, osc=OSC, taps=TAPS, agc=AGC)
# complex samples per piece: 1, 3, a block - 1 and + 1, pieces that are no multiple of 4; the second list keeps ibit (4 samples a byte)
# and, behind a decimator by 2, i2bit (2 kept samples a byte) on byte boundaries
CUTS = ([1, 3, BLOCK - 1, BLOCK + 1, 1001, 2, 1498], [N - 1], [1] * 9 + [BLOCK] * 3)
CUTS_BYTES = ([4, 12, BLOCK - 4, BLOCK + 4, 1004, 8, 1496], [N - 4], [4] * 5 + [BLOCK] * 3)


@pytest.fixture(scope="module")
def x():
    v = np.random.default_rng(20220220).integers(-32768, 32768, size=2 * N).astype(np.int16)
    v.setflags(write=False)
    return v


def _some(sat, values):
    """Some values clamp, most do not."""
    assert 0 < sat < 0.25 * values, (sat, values)


def test_no_stage_is_the_stream(x):
    out, gains, sat = chain_model.Chain().run(x)
    assert out.tobytes() == x.astype("<i2").tobytes() and gains.size == 0 and sat == 0
    for fmt, shift in (("ibyte", 8), ("ibit", 0)):
        out, gains, sat = chain_model.Chain(fmt, shift).run(x, [4, 1000])
        want, want_sat = noise_model.convert(x, fmt, shift, (0, 0, 65536, 0))
        assert out.tobytes() == want.tobytes() and sat == want_sat and gains.size == 0
    _some(chain_model.Chain("ibyte", 8).run(x)[2], 2 * N)


@pytest.mark.parametrize("fmt,shift", [("ishort", 0), ("ibyte", 8), ("ibit", 0)])
def test_the_mix_alone_is_the_fused_pass(x, fmt, shift):
    """One pass mixes and formats: a value both clamps change counts once."""
    out, _, sat = chain_model.Chain(fmt, shift, noise=NOISE, interf=INTERF).run(x)
    want, want_sat = interf_model.convert(x, fmt, shift, NOISE, INTERF)
    assert out.tobytes() == want.tobytes() and sat == want_sat
    _some(sat, 2 * N)
    out, _, sat = chain_model.Chain(fmt, shift, noise=NOISE).run(x)
    want, want_sat = noise_model.convert(x, fmt, shift, NOISE)
    assert out.tobytes() == want.tobytes() and sat == want_sat
    out, _, sat = chain_model.Chain(fmt, shift, interf=INTERF).run(x)
    want, want_sat = interf_model.convert(x, fmt, shift, None, INTERF)
    assert out.tobytes() == want.tobytes() and sat == want_sat


def test_the_oscillator_alone(x):
    out, _, sat = chain_model.Chain(osc=OSC).run(x)
    want, want_sat, _ = osc_model.rotate(x, OSC, 0, 0)
    assert out.tobytes() == want.astype("<i2").tobytes() and sat == want_sat
    _some(sat, N)


def test_the_filter_and_the_decimator_alone(x):
    out, _, sat = chain_model.Chain(taps=TAPS).run(x)
    want, want_sat = fir_model.fir(x, TAPS)
    assert out.tobytes() == want.astype("<i2").tobytes() and sat == want_sat
    _some(sat, 2 * N)
    out, _, sat = chain_model.Chain(taps=DEC_TAPS, decim=2).run(x)
    want, want_sat = firdec_model.firdec(x, DEC_TAPS, 2)
    assert out.tobytes() == want.astype("<i2").tobytes() and sat == want_sat and want.size == N
    _some(sat, N)


@pytest.mark.parametrize("fmt,param", [("ishort", 0), ("ibyte", 8), ("i2bit", 9000)])
def test_the_agc_alone(x, fmt, param):
    out, gains, sat = chain_model.Chain(fmt, param, agc=AGC).run(x)
    want, want_gains, want_sat = agc_model.agc(x, AGC, 0, fmt, param)
    assert out.tobytes() == want.tobytes() and np.array_equal(gains, want_gains) and sat == want_sat
    assert gains.size == -(-N // BLOCK) and len(np.unique(gains)) > 10
    _some(sat, 2 * N)


CHAINS = {
    "mix_osc_fir_agc_ibyte": (dict(FULL, fmt="ibyte", param=8), CUTS),
    "mix_osc_fir_agc_ishort": (dict(FULL, fmt="ishort"), CUTS),
    "mix_osc_dec_agc_i2bit": (dict(FULL, taps=DEC_TAPS, decim=2, fmt="i2bit", param=9000), CUTS_BYTES),
    "mix_osc_dec_ibyte": (dict(noise=NOISE, osc=OSC, taps=DEC_TAPS, decim=2, fmt="ibyte", param=8), CUTS),
    "mix_osc_ibyte": (dict(noise=NOISE, interf=INTERF, osc=OSC, fmt="ibyte", param=8), CUTS),
    "jam_osc_agc_i2bit": (dict(interf=INTERF, osc=OSC, agc=AGC, fmt="i2bit", param=9000), CUTS_BYTES),
    "mix_fir_ibit": (dict(noise=NOISE, taps=TAPS, fmt="ibit"), CUTS_BYTES),
    "mix_ibyte_fused": (dict(noise=NOISE, interf=INTERF, fmt="ibyte", param=8), CUTS),
}


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_any_cut_gives_the_bytes_gains_and_count_of_one_piece(x, name):
    kw, cut_lists = CHAINS[name]
    out, gains, sat = chain_model.Chain(**kw).run(x)
    assert sat > 0 and np.count_nonzero(out) > 0.5 * out.size
    for cuts in cut_lists:
        o, g, s = chain_model.Chain(**kw).run(x, cuts)
        assert o.tobytes() == out.tobytes() and np.array_equal(g, gains) and s == sat, (name, cuts)


def test_the_stages_compose_in_run_chains_order(x):
    """The whole chain by hand, one model behind the other, with the counts summed."""
    a, clipped = interf_model.mix(x, NOISE, INTERF)
    b, sat_o, _ = osc_model.rotate(a, OSC, 0, 0)
    c, sat_f = fir_model.fir(b, TAPS)
    want, want_gains, sat_a = agc_model.agc(c, AGC, 0, "ibyte", 8)
    out, gains, sat = chain_model.Chain("ibyte", 8, **FULL).run(x)
    assert out.tobytes() == want.tobytes() and np.array_equal(gains, want_gains)
    assert sat == int(np.count_nonzero(clipped)) + sat_o + sat_f + sat_a and min(int(np.count_nonzero(clipped)), sat_o, sat_f, sat_a) > 0


@pytest.mark.parametrize("swap", [("osc", "mix", "fir", "agc"), ("mix", "fir", "osc", "agc"), ("mix", "osc", "agc", "fir")],
                         ids=["osc_mix", "fir_osc", "agc_fir"])
def test_this_input_tells_the_order_from_its_neighbours(x, swap):
    for kw in (dict(FULL, fmt="ibyte", param=8), dict(FULL, fmt="ishort"), dict(FULL, taps=DEC_TAPS, decim=2, fmt="ibyte", param=8)):
        out, gains, _ = chain_model.Chain(**kw).run(x)
        other, other_gains, _ = chain_model.Chain(order=swap, **kw).run(x)
        assert other.size == out.size and np.count_nonzero(other != out) > 0.5 * out.size, swap
        assert not np.array_equal(other_gains, gains)
