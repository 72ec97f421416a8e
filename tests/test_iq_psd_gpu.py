"""The Welch power spectrum on the MI355X (gal_synth_iq_psd): the kernel's uint64 sums against the numpy statement of the definition
(tests/psd_model.py), exactly (np.array_equal), in the three formats, at every size class of the kernel -- N = 8 (odd stage count, 128
segments side by side in a block), 16, 64, 1024 (one segment per slab) and 4096 (the LDS maximum, four butterflies of four per lane) --,
both windows, on a batch the engine synthesised and on random full-range int16; the edge shapes; the full-scale range; the refusals
that need a handle; repeatability."""
import numpy as np
import pytest

import psd_model

pytestmark = pytest.mark.gpu

GAL_E_INVAL, GAL_E_STATE = -1, -4
FORMATS = (("ishort", 0), ("ibyte", 5), ("ibit", 0))
FMT_CODE = {"ishort": 0, "ibyte": 1, "ibit": 2}
SIZES = (3, 4, 6, 10, 12)


@pytest.fixture(scope="module")
def eng(pkg):
    with pkg.SynthEngine(device=0) as e:
        yield e


def _three_formats(pkg, eng, x):
    """the int16 stream x (interleaved) in the three formats: {fmt: (device tensor, host bytes)}; 64 spare bytes behind each"""
    import torch

    n = x.size // 2
    xd = torch.from_numpy(x).cuda()
    bufs = {}
    for fmt, s in FORMATS:
        out = torch.zeros(pkg.iq_bytes(fmt, n) + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        eng.iq_convert(xd.data_ptr(), n, fmt, s, out.data_ptr())
        eng.iq_saturated()
        bufs[fmt] = (out, out.cpu().numpy())
    return n, bufs


@pytest.fixture(scope="module")
def batch12(pkg, eng):
    """Two epochs of the 12-channel synthetic record set, synthesised by the engine, as tests/test_iq_corr_gpu.py makes it."""
    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=12, n_slots=16, seed=41)
    x, _, _ = eng.run_host(p)
    return _three_formats(pkg, eng, x)


@pytest.fixture(scope="module")
def random16(pkg, eng):
    """40 000 samples of full-range int16, -32768 and 32767 among them"""
    x = np.random.default_rng(77).integers(-32768, 32768, 2 * 40000).astype(np.int16)
    x[:4] = (-32768, 32767, 32767, -32768)
    return _three_formats(pkg, eng, x)


_want = {}


def _model(key, host, fmt, n_samples, log2_n, hop, win):
    """the model's sums, computed once per (buffer, shape)"""
    k = (key, fmt, n_samples, log2_n, hop, win)
    if k not in _want:
        nb = {"ishort": 4 * n_samples, "ibyte": 2 * n_samples, "ibit": (n_samples + 3) // 4}[fmt]
        v = psd_model.values(host[:nb], FMT_CODE[fmt])[: 2 * n_samples]
        _want[k] = psd_model.psd(v, FMT_CODE[fmt], log2_n, hop, win)
    return _want[k]


def _check(eng, key, bufs, fmt, n_samples, log2_n, hop, win, byte_offset=0):
    dev, host = bufs[fmt]
    got, n_seg = eng.iq_psd(dev.data_ptr() + byte_offset, fmt, n_samples, log2_n, hop, win)
    want, want_seg = _model((key, byte_offset), host[byte_offset:], fmt, n_samples, log2_n, hop, win)
    assert n_seg == want_seg
    assert got.dtype == np.uint64 and got.shape == (1 << log2_n,)
    assert np.array_equal(got, want), (fmt, log2_n, hop, win, int(np.count_nonzero(got != want)))
    return got


@pytest.mark.parametrize("fmt", [f for f, _ in FORMATS])
@pytest.mark.parametrize("win", (0, 1))
@pytest.mark.parametrize("log2_n", SIZES)
def test_synthesised_batch(eng, batch12, log2_n, win, fmt):
    """520 000 samples, hop N / 2 under the Hann window and N under the rectangular one: 130 000 segments at N = 8 (a run of 254 slabs per
    block, the last one short), 253 at N = 4096"""
    n, bufs = batch12
    got = _check(eng, "b12", bufs, fmt, n, log2_n, (1 << log2_n) >> win, win)
    assert got.any()


@pytest.mark.parametrize("fmt", [f for f, _ in FORMATS])
@pytest.mark.parametrize("win", (0, 1))
@pytest.mark.parametrize("log2_n", SIZES)
def test_random_full_range(eng, random16, log2_n, win, fmt):
    n, bufs = random16
    _check(eng, "rnd", bufs, fmt, n, log2_n, (1 << log2_n) >> win, win)


@pytest.mark.parametrize("fmt", [f for f, _ in FORMATS])
def test_shapes(eng, random16, fmt):
    n, bufs = random16
    for log2_n in (3, 6, 10, 12):
        N = 1 << log2_n
        _check(eng, "rnd", bufs, fmt, N, log2_n, N // 2, 1)                 # one segment
        _check(eng, "rnd", bufs, fmt, N + N // 2, log2_n, N // 2, 1)        # two
        _check(eng, "rnd", bufs, fmt, N + N // 2 + 1, log2_n, N // 2, 0)    # two and a tail of one sample
        _check(eng, "rnd", bufs, fmt, 3 * N - 1, log2_n, N, 0)              # hop = N, a tail of N - 1
    _check(eng, "rnd", bufs, fmt, 8 + 36 * 3, 3, 3, 1)                      # 37 segments, an odd hop
    _check(eng, "rnd", bufs, fmt, 1024 + 36 * 100 + 99, 10, 100, 1)         # 37 segments of 1024 and a tail
    _check(eng, "rnd", bufs, fmt, 100, 3, 1, 1)                             # hop = 1: 93 segments
    _check(eng, "rnd", bufs, fmt, 100, 3, 1, 0)
    # a buffer that starts 16 bytes into the allocation
    _check(eng, "rnd", bufs, fmt, 5000, 6, 17, 1, byte_offset=16)
    _check(eng, "rnd", bufs, fmt, 9000, 12, 2048, 1, byte_offset=16)


def test_full_scale_range(pkg, eng):
    """N = 4096, rectangular, 256 segments -- n_seg N^2 = 2^32 exactly -- of the sample (-32768, -32768): X[0] = -2^27 on both rails,
    out[0] = 256 x 2 x 2^54 = 2^63 exactly, every other bin 0.  The same shape with the full-scale Nyquist alternation
    (-32768, -32768), (32767, 32767), ...: against the model (bin N / 2 carries nearly all of it)."""
    import torch

    n = 4096 * 256
    x = np.full(2 * n, -32768, np.int16)
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    got, n_seg = eng.iq_psd(xd.data_ptr(), "ishort", n, 12, 4096, 0)
    assert n_seg == 256
    assert int(got[0]) == 1 << 63 and not got[1:].any()
    x[2::4] = 32767
    x[3::4] = 32767
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    got, n_seg = eng.iq_psd(xd.data_ptr(), "ishort", n, 12, 4096, 0)
    # every segment is the same: the model on one, times 256
    one, _ = psd_model.psd(x[: 2 * 4096].astype(np.int64), 0, 12, 4096, 0)
    assert n_seg == 256 and np.array_equal(got, one * np.uint64(256))
    assert int(np.argmax(got)) == 2048 and int(got[2048]) > (1 << 63) - (1 << 49)


def test_refusals_that_need_a_handle(pkg, eng, random16):
    import torch

    n, bufs = random16
    dev = bufs["ishort"][0]
    out = torch.zeros(4096 + 8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def refused(buf_ptr, fmt, n_samples, log2_n, hop, win, out_ptr, code=GAL_E_INVAL, **kw):
        with pytest.raises(pkg.GalSynthError) as ei:
            eng.iq_psd(buf_ptr, fmt, n_samples, log2_n, hop, win, out_ptr=out_ptr, **kw)
        assert ei.value.code == code

    ok = (dev.data_ptr(), "ishort", 4096, 10, 512, 1, out.data_ptr())
    assert eng.iq_psd(*ok) == (None, 7)
    refused(dev.data_ptr(), 3, 4096, 10, 512, 1, out.data_ptr())            # i2bit
    refused(dev.data_ptr(), 4, 4096, 10, 512, 1, out.data_ptr())            # unknown
    refused(dev.data_ptr(), "ishort", 4096, 10, 512, 1, out.data_ptr() + 8)  # misaligned out_dev
    refused(dev.data_ptr() + 4, "ishort", 4096, 10, 512, 1, out.data_ptr())  # misaligned buffer
    refused(0, "ishort", 4096, 10, 512, 1, out.data_ptr())
    refused(dev.data_ptr(), "ishort", 4096, 10, 512, 1, dev.data_ptr() + 4096 * 4 - 16)  # the last 16 bytes of the buffer
    refused(dev.data_ptr() + 8 * 1024 - 16, "ishort", 4096, 10, 512, 1, dev.data_ptr())  # ... of the output
    for bad in ((2, 4, 1), (13, 4, 1), (10, 0, 1), (10, 1025, 1), (10, 512, 2), (10, 512, -1)):
        refused(dev.data_ptr(), "ishort", 4096, bad[0], bad[1], bad[2], out.data_ptr())
    refused(dev.data_ptr(), "ishort", 4096, 10, 512, 1, out.data_ptr(), reserved=1)
    refused(dev.data_ptr(), "ishort", 1023, 10, 512, 1, out.data_ptr())     # no segment
    # over the bound: N = 64 allows 2^20 segments; hop 1 on 2^20 + 64 samples is one more (the buffer is never touched: refused first)
    big = torch.zeros(4 * ((1 << 20) + 64), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert pkg.psd_segments(6, 1, 0, (1 << 20) + 63) == 1 << 20
    refused(big.data_ptr(), "ishort", (1 << 20) + 64, 6, 1, 0, out.data_ptr())


def test_buffer_of_the_batch_in_flight_is_refused(pkg):
    import torch

    p = pkg.workloads.make_synthetic(n_epochs=2, n_chan=4, n_slots=16, samples_per_epoch=26000, seed=12)
    with pkg.SynthEngine(samples_per_epoch=26000, n_slots=16, device=0) as e:
        e.plan(p)
        iq = torch.empty(e.output_bytes() // 2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        e.execute(iq.data_ptr())
        with pytest.raises(pkg.GalSynthError) as ei:
            e.iq_psd(iq.data_ptr(), "ishort", 26000, 8, 128, 1)
        assert ei.value.code == GAL_E_STATE
        e.finish()
        got, n_seg = e.iq_psd(iq.data_ptr(), "ishort", 26000, 8, 128, 1)
        want, want_seg = psd_model.psd(psd_model.values(iq.cpu().numpy(), 0)[: 2 * 26000], 0, 8, 128, 1)
        assert n_seg == want_seg and np.array_equal(got, want)


def test_two_calls_give_the_same_sums(eng, batch12):
    """out_dev is zeroed by the call and the atomics are order-free: a second call into the SAME output buffer gives the same array"""
    import torch

    n, bufs = batch12
    dev = bufs["ishort"][0]
    out = torch.full((1024,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    res = []
    for _ in range(2):
        eng.iq_psd(dev.data_ptr(), "ishort", n, 10, 512, 1, out_ptr=out.data_ptr())
        eng.iq_saturated()
        res.append(out.cpu().numpy().view(np.uint64).copy())
    assert np.array_equal(res[0], res[1])
    want, _ = _model(("b12", 0), bufs["ishort"][1], "ishort", n, 10, 512, 1)
    assert np.array_equal(res[0], want)
