"""The block AGC and the 2-bit quantiser as include/galsynth.h defines them (gal_synth_agc_check, gal_synth_agc_from_rms,
gal_synth_agc_out_bytes, gal_synth_agc_blocks, gal_synth_iq_agc), in numpy -- TEST INFRASTRUCTURE: the product
never imports this.

agc() states the function over a whole stream at once; Stream carries the state the handle keeps (the powers of the last W complete
blocks, the open block's partial sum, the position) from call to call, written on its own, so that "any cut gives the bytes of one
call" is a property of the definition before it is one of the kernels."""
import numpy as np

GAL_AGC_MIN_BLOCK = 16
GAL_AGC_MAX_BLOCK = 65536
GAL_AGC_MAX_WINDOW = 64
GAL_AGC_MAX_SPAN = 65536
GAL_AGC_GAIN_MAX = 1 << 24
TARGET_Q8_MAX = 32767 * 256
FORMATS = ("ishort", "ibyte", "i2bit")
# csrc/iq_agc.hip: complex samples per lane and trip of k_iq_agc (4 x kVec), threads per workgroup, the grid cap, and the samples one
# workgroup of k_agc_power owns
RUN = {"ishort": 4, "ibyte": 8, "i2bit": 16}
THREADS = 256
MAX_BLOCKS = 2048
POWER_CHUNK = 16384


def params(block_len, window, target_q8, gain_min_q12=1, gain_max_q12=GAL_AGC_GAIN_MAX, p_init=0):
    return {"block_len": int(block_len), "window": int(window), "target_q8": int(target_q8), "gain_min_q12": int(gain_min_q12),
            "gain_max_q12": int(gain_max_q12), "p_init": int(p_init)}


def check(p):
    """True where gal_synth_agc_check admits the parameters."""
    B, W = p["block_len"], p["window"]
    return (GAL_AGC_MIN_BLOCK <= B <= GAL_AGC_MAX_BLOCK and 1 <= W <= GAL_AGC_MAX_WINDOW and B * W <= GAL_AGC_MAX_SPAN
            and 1 <= p["target_q8"] <= TARGET_Q8_MAX and 1 <= p["gain_min_q12"] <= p["gain_max_q12"] <= GAL_AGC_GAIN_MAX
            and 0 <= p["p_init"] <= (B << 31))


def _llround(v):
    """C's llround of a double: ties away from zero."""
    v = float(v)
    return int(np.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def from_rms(target_rms, init_rms, block_len, window):
    """gal_synth_agc_from_rms in double, operation for operation as the header states it."""
    t = np.float64(target_rms) * np.float64(256.0)
    sq = np.float64(init_rms) * np.float64(init_rms)
    p = params(block_len, window, _llround(t), p_init=2 * int(block_len) * _llround(sq))
    assert check(p)
    return p


def out_bytes(fmt, n):
    return {"ishort": 4 * n, "ibyte": 2 * n, "i2bit": (n + 1) // 2}[fmt]


def blocks(first_sample, n, block_len):
    """The number of b with first_sample <= b B < first_sample + n (Python integers)."""
    P, n, B = int(first_sample), int(n), int(block_len)
    return -((-(P + n)) // B) - -((-P) // B)


def isqrt(v):
    """floor(sqrt(v)) of a uint64 array, v <= 2^46: the float result fixed up in integers."""
    v = np.asarray(v, dtype=np.uint64)
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.uint64)
    for _ in range(4):
        r = np.where(r * r > v, r - np.uint64(1), r)
        r = np.where((r + np.uint64(1)) * (r + np.uint64(1)) <= v, r + np.uint64(1), r)
    assert (r * r <= v).all() and ((r + np.uint64(1)) * (r + np.uint64(1)) > v).all()
    return r


def gain_of(Q, p):
    """g of the window sums Q (uint64 array)."""
    Q = np.asarray(Q, dtype=np.uint64)
    assert Q.size == 0 or int(Q.max()) <= 1 << 47
    ms = (Q << np.uint64(16)) // np.uint64(2 * p["block_len"] * p["window"])
    rms = np.maximum(isqrt(ms), np.uint64(1))
    g = np.uint64(p["target_q8"] << 12) // rms
    return np.clip(g, np.uint64(p["gain_min_q12"]), np.uint64(p["gain_max_q12"])).astype(np.uint32)


def quantise(z, fmt, param):
    """z: int64 values BEFORE the clamp to int16, interleaved.  Returns (bytes as a uint8 array, values a counted clamp changed)."""
    y = np.clip(z, -32768, 32767)
    sat = y != z
    if fmt == "ishort":
        assert param == 0
        out = y.astype("<i2").view(np.uint8)
    elif fmt == "ibyte":
        assert 0 <= param <= 15
        r = (1 << (param - 1)) if param else 0
        q = (y + r) >> param
        sat = sat | (q < -127) | (q > 127)
        out = np.clip(q, -127, 127).astype(np.int8).view(np.uint8)
    elif fmt == "i2bit":
        assert 1 <= param <= 32767 and z.size % 2 == 0
        q = (y > param).astype(np.int64) + (y > 0) + (y > -param) - 2
        code = (q & 3).astype(np.uint8)
        code = np.concatenate([code, np.zeros((-code.size) % 4, dtype=np.uint8)]).reshape(-1, 4)
        out = (code[:, 0] << 6) | (code[:, 1] << 4) | (code[:, 2] << 2) | code[:, 3]
    else:
        raise ValueError(fmt)
    return np.ascontiguousarray(out, dtype=np.uint8), int(np.count_nonzero(sat))


def _apply(x, g_of_sample, fmt, param):
    g2 = np.repeat(g_of_sample.astype(np.int64), 2)
    z = (x.astype(np.int64) * g2 + 2048) >> 12
    return quantise(z, fmt, param)


def agc(x, p, first_sample=0, fmt="ishort", param=0):
    """x: interleaved int16 of a WHOLE stream whose first sample has the global index first_sample (every block in front of
    first_sample div B has the power p_init; the samples in front of first_sample in its own block count as 0).  Returns (bytes as a
    uint8 array, the uint32 gains of the blocks that start in the stream, values a counted clamp changed)."""
    x = np.asarray(x, dtype=np.int16)
    assert x.ndim == 1 and x.size % 2 == 0 and check(p) and first_sample >= 0
    n, B, W = x.size // 2, p["block_len"], p["window"]
    off0 = int(first_sample) % B
    nt = (off0 + n - 1) // B + 1 if n else 0  # blocks touched, counted from first_sample div B
    pw = np.zeros(nt * B, dtype=np.uint64)
    xs = x.astype(np.int64).reshape(-1, 2)
    pw[off0: off0 + n] = (xs[:, 0] * xs[:, 0] + xs[:, 1] * xs[:, 1]).astype(np.uint64)
    P = np.concatenate([np.full(W, p["p_init"], dtype=np.uint64), pw.reshape(nt, B).sum(axis=1, dtype=np.uint64)])  # P[W + j]: block j
    Q = np.zeros(nt, dtype=np.uint64)
    for i in range(1, W + 1):
        Q += P[W - i: W - i + nt]
    g = gain_of(Q, p)
    blk = (off0 + np.arange(n, dtype=np.int64)) // B
    out, sat = _apply(x, g[blk] if n else g[:0], fmt, param)
    assert out.size == out_bytes(fmt, n)
    gains = g[(1 if off0 else 0):]
    assert gains.size == blocks(first_sample, n, B)
    return out, gains, sat


class Stream:
    """The stream in calls, with the state gal_synth_agc_set / gal_synth_iq_agc keep."""

    def __init__(self, p, first_sample=0):
        assert check(p) and first_sample >= 0
        self.p = p
        self.hist = [p["p_init"]] * p["window"]  # the powers of the last W complete blocks, oldest first
        self.part = 0                            # the open block's sum so far
        self.pos = int(first_sample)

    def call(self, x, fmt="ishort", param=0):
        """The next samples x of the stream: (bytes, gains of the blocks that start in the call, saturated)."""
        x = np.asarray(x, dtype=np.int16)
        n, B = x.size // 2, self.p["block_len"]
        xs = x.astype(np.int64).reshape(-1, 2)
        pw = xs[:, 0] * xs[:, 0] + xs[:, 1] * xs[:, 1]
        g_of_sample = np.zeros(n, dtype=np.uint32)
        gains, at = [], 0
        while at < n:
            rem = self.pos % B
            g = int(gain_of(np.array([sum(self.hist)], dtype=np.uint64), self.p)[0])
            if rem == 0:
                gains.append(g)
            take = min(B - rem, n - at)
            g_of_sample[at: at + take] = g
            self.part += int(pw[at: at + take].sum())
            self.pos += take
            at += take
            if self.pos % B == 0:
                self.hist = self.hist[1:] + [self.part]
                self.part = 0
        out, sat = _apply(x, g_of_sample, fmt, param)
        return out, np.array(gains, dtype=np.uint32), sat


def agc_in_cuts(x, p, cuts, first_sample=0, fmt="ishort", param=0):
    """agc() through Stream: calls of the lengths `cuts`, then the rest.  For "i2bit" the cuts must be even."""
    x = np.asarray(x, dtype=np.int16)
    s = Stream(p, first_sample)
    outs, gains, sat, at = [], [], 0, 0
    for c in list(cuts) + [x.size // 2 - sum(cuts)]:
        o, g, k = s.call(x[2 * at: 2 * (at + c)], fmt, param)
        outs.append(o)
        gains.append(g)
        sat += k
        at += c
    assert at == x.size // 2
    return np.concatenate(outs), np.concatenate(gains), sat


def segment(p):
    """The length of one segment of make_input: longer than the window, so that the window comes to lie inside every segment."""
    return (p["window"] + 2) * p["block_len"] + 3


def make_input(rng, n, p):
    """n complex samples in segments of very different amplitude, each segment(p) long: first one at full scale, +-32767 / -32768 (a gain
    above about 1.0 saturates the int16 clamp: with a gain_min above that it fires at the end of the segment, and a small p_init
    saturates from the first sample on), then one all zero (gain_max fires), then random full-range int16, small and tiny values."""
    x = np.zeros(2 * n, dtype=np.int16)
    seg = segment(p)
    kinds = ["scale", "zero", "full", "small", "tiny", "full"]
    at, k = 0, 0
    while at < n:
        m = min(seg, n - at)
        kind = kinds[k % len(kinds)]
        if kind == "full":
            v = rng.integers(-32768, 32768, size=2 * m)
        elif kind == "small":
            v = rng.integers(-300, 301, size=2 * m)
        elif kind == "tiny":
            v = rng.integers(-3, 4, size=2 * m)
        elif kind == "scale":
            v = rng.choice(np.array([-32768, 32767]), size=2 * m)
        else:
            v = np.zeros(2 * m, dtype=np.int64)
        x[2 * at: 2 * (at + m)] = v
        at += m
        k += 1
    return x
