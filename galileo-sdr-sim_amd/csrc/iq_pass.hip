// iq_pass.hip -- every pass over the FINAL interleaved int16 stream x[j] = I0, Q0, I1, Q1, ... (src/galileo-sdr.cpp:536-537) that ends
// in an output format of include/galsynth.h: the plain formats (gal_synth_iq_convert), the seeded AWGN noise floor
// (gal_synth_iq_convert_noise) and the seeded CW / chirp / pulsed interference sources (gal_synth_iq_convert_interf).  One kernel,
// k_iq_pass<Fmt, kMode, kSrc>, in 17 instances.  Per value, with J = 2 first_sample + j the index of the value in the whole output
// stream and N = J >> 1 its complex sample (both 64-bit):
//
//   u       word J & 3 of Philox4x32-10(counter = (B lo, B hi, stream, 0), key = (seed lo, seed hi)), B = J >> 2
//   z       the octave-segment inverse normal CDF of u in Q12 (table T of csrc/gauss_table.inc; unit variance at 4096)
//   per source:
//   (s, m)  = (N div sweep_len, N mod sweep_len)                     (a CW source is run as sweep_len 1, df 0: the same phase)
//   phi     = ph0 + s W + m f0 + df m (m - 1) / 2  (mod 2^32),  W = sweep_len f0 + df sweep_len (sweep_len - 1) / 2
//   i       = phi >> 22;  I takes A C[i], Q takes A C[(i - 256) & 1023] while (N mod pulse_period) < pulse_on
//   y       = clamp16((int64(x) G + int64(z) S + sum of the source terms + 32768) >> 16)
//   out     y in the format: ishort y; ibyte (y + r) >> s clamped to +-127, r = s ? 1 << (s - 1) : 0 (int32 arithmetic shift: round
//           to nearest, ties up); ibit y > 0, byte k = the values 8k .. 8k+7 with 8k in bit 7 (numpy.packbits), unused low bits 0
//
// A value counts once as saturated if either clamp changed it.  Everything is integer arithmetic: the output is a fixed function of
// (parameters, J, x) on any machine (tests/noise_model.py and tests/interf_model.py state it in numpy).
//
//   Fmt    the output format: how many 16-byte vectors a lane takes per trip, the pack of eight mixed values, the store, the tail
//   kMode  0 nothing random (S = 0: no Philox work, no Gauss table); 1 noise at even first_sample: a vector of 8 values is two Philox
//          blocks; 2 noise at odd first_sample: the vector starts at word 2 of a block and takes three (correct, a block per vector
//          wasted; the CLI's batches are even)
//   kSrc   sources present: the lane state, the cosine table and the InterfArgs argument exist only then
//
// <Fmt, 0, false> is the plain conversion: y = x, no table, no 64-bit multiply, and ibit counts nothing.  (Plain ishort is a copy and
// has no instance.)  The plain instances are memory-bound streams: every input byte is read once, nothing is reused, and ibit issues
// all eight loads of a trip before it uses any.  Input loads are plain: non-temporal ones (__builtin_nontemporal_load) were measured
// slower for ibit at every size (2.1x at 311.74 M samples) and for ibyte on the CLI's 128-epoch batch, which the synthesis has just
// written.  The mixed instances are bound by the 40 32-bit multiplies of a Philox block and the per-sample
// source steps, not by HBM (DESIGN.md sections 11, 13); ibit runs its eight vectors two at a time there to stay in its registers.
//
// Shape: 16-byte loads, 64-bit indices (a batch of the library may hold well over 2^31 bytes), a grid-stride loop, the complex
// samples behind the last whole trip in one lane.  Saturated values are counted per lane in a register, summed per wave (shuffles)
// and per block (LDS), and one lane per block adds the block's sum to the handle's 64-bit counter with one ordinary global atomicAdd
// -- and only if it is not 0.  The Gauss table sits in LDS as one 32-bit word per cell, a | (a - b) << 16, 4 KB: half of all look-ups
// fall into the 32 cells of octave 0, which lie in 32 different banks; the 2 KB cosine table sits beside it.
//
// Sources: nothing is divided per sample.  A lane handles a RUN of consecutive samples per trip (4 ishort, 8 ibyte, 32 ibit) and its
// next run lies a constant number of samples further on.  The host divides first_sample once per source; a lane finds its first
// (s, m) and pulse position with one 32-bit division per source, steps them sample by sample inside a run -- the phase by the
// recurrence phi += f0 + m df, which the closed form equals -- and takes the constant jump to its next run with the host's
// (jump div len, jump mod len) and one conditional correction, where the phase is formed anew from the closed form (four 32-bit
// multiplies).  The source parameters arrive by value.
//
// This is a separate launch behind gal_synth_finish, never fused into the synthesis kernels: k_repair_g and the accumulating
// exact-replay launches rewrite int16 output after k_synth_g has run, and gal_synth_finish may synthesise the batch again.
#include <string.h>

#include <type_traits>

#include "../../include/galsynth.h"

#define GAL_GAUSS_DEVICE_TABLE
#define GAL_INTERF_DEVICE_TABLE
#include "iq_dev.h"

namespace {

constexpr int kMaxBlocks = 2048;  // 8 blocks of 4 waves per CU, the rest by the grid-stride loop

struct NoiseArgs {
    uint64_t j0;      // 2 first_sample: the global index of the call's first value
    uint32_t k0, k1;  // seed, low and high word
    uint32_t stream;
    int g, s;         // gain_q16, sigma_q4 (both <= 2^20)
};

struct InterfSrc {
    int amp;                  // A = amp_q4, 0 .. 2^20
    uint32_t ph0, f0, df, w;  // w = W, the phase advance of one whole sweep (mod 2^32)
    uint32_t len, period, on; // len >= 1 (CW: 1); period >= 1 (always on: 1 / 1)
    uint32_t s0, m0, p0;      // at the call's first sample: sweep number (low word), position in the sweep, position in the pulse period
    uint32_t ts, tm, tp;      // the same at the tail's first sample
    uint32_t jq, jr, jp;      // from the end of a run to the lane's next: jump div len, jump mod len, jump mod period
};

struct InterfArgs {
    int n;  // sources in use, 0 .. 4
    InterfSrc src[GAL_INTERF_MAX];
};

struct NoSrcArgs {};  // the kernel argument of the instances without sources

struct Lane {  // one source as one lane sees it, at the sample the lane handles next
    uint32_t s, m, pp, ph, step;
};

// ---- noise ---------------------------------------------------------------------------------------------------------------------
// ---- sources -------------------------------------------------------------------------------------------------------------------
// m (m - 1) / 2 mod 2^32 (the product is even and below 2^64: halve the even factor first)
__device__ __forceinline__ uint32_t tri(uint32_t m) { return (m & 1u) ? m * ((m - 1u) >> 1) : (m >> 1) * (m - 1u); }

// phase and phase step of the closed form at (s, m)
__device__ __forceinline__ void rephase(const InterfSrc &c, Lane &l)
{
    l.ph = c.ph0 + l.s * c.w + l.m * c.f0 + c.df * tri(l.m);
    l.step = c.f0 + l.m * c.df;
}

// (s, m, pp) := (s, m, pp) + (q sweeps and r samples, rp pulse positions), r < len, rp < period
__device__ __forceinline__ void advance(const InterfSrc &c, Lane &l, uint32_t q, uint32_t r, uint32_t rp)
{
    const uint64_t m = (uint64_t)l.m + r, pp = (uint64_t)l.pp + rp;  // (both terms may be close to 2^32)
    const bool over = m >= c.len;
    l.s += q + (uint32_t)over;
    l.m = (uint32_t)(over ? m - c.len : m);
    l.pp = (uint32_t)(pp >= c.period ? pp - c.period : pp);
    rephase(c, l);
}

// the lane's first sample lies `off` samples behind the call's first
__device__ __forceinline__ void seek(const InterfArgs &p, Lane (&L)[GAL_INTERF_MAX], uint32_t off)
{
#pragma unroll
    for (int k = 0; k < GAL_INTERF_MAX; ++k)
        if (k < p.n) {
            const InterfSrc &c = p.src[k];
            const uint32_t q = off / c.len;
            L[k].s = c.s0;
            L[k].m = c.m0;
            L[k].pp = c.p0;
            advance(c, L[k], q, off - q * c.len, off % c.period);
        }
}

__device__ __forceinline__ void jump(const InterfArgs &p, Lane (&L)[GAL_INTERF_MAX])
{
#pragma unroll
    for (int k = 0; k < GAL_INTERF_MAX; ++k)
        if (k < p.n) advance(p.src[k], L[k], p.src[k].jq, p.src[k].jr, p.src[k].jp);
}

// the lane that takes the samples behind the last whole trip starts from the tail's state
__device__ __forceinline__ void seek_tail(const InterfArgs &p, Lane (&L)[GAL_INTERF_MAX])
{
#pragma unroll
    for (int k = 0; k < GAL_INTERF_MAX; ++k)
        if (k < p.n) {
            L[k].s = p.src[k].ts;
            L[k].m = p.src[k].tm;
            L[k].pp = p.src[k].tp;
            rephase(p.src[k], L[k]);
        }
}

// the source terms of one complex sample added to (aI, aQ); every source steps to the next sample
__device__ __forceinline__ void sources(const InterfArgs &p, Lane (&L)[GAL_INTERF_MAX], const int16_t *ct, long long &aI, long long &aQ)
{
#pragma unroll
    for (int k = 0; k < GAL_INTERF_MAX; ++k)
        if (k < p.n) {
            const InterfSrc &c = p.src[k];
            Lane &l = L[k];
            const uint32_t i = l.ph >> 22;
            const int a = l.pp < c.on ? c.amp : 0;
            aI += (long long)a * ct[i];
            aQ += (long long)a * ct[(i - 256u) & 1023u];
            l.ph += l.step;
            const bool wrap = l.m + 1u == c.len;
            l.m = wrap ? 0u : l.m + 1u;
            l.step = wrap ? c.f0 : l.step + c.df;
            l.s += (uint32_t)wrap;
            l.pp = l.pp + 1u == c.period ? 0u : l.pp + 1u;
        }
}

// ---- the mix -------------------------------------------------------------------------------------------------------------------
// what every mix of one kernel instance needs; ip and L are empty without sources, gt / ct unset where the instance has no table
template <bool kSrc>
struct Mixer {
    const NoiseArgs &np;
    const std::conditional_t<kSrc, InterfArgs, NoSrcArgs> &ip;
    std::conditional_t<kSrc, Lane[GAL_INTERF_MAX], NoSrcArgs> L;
    const uint32_t *gt;
    const int16_t *ct;
};

// one complex sample (xI, xQ) with the Gaussian words (uI, uQ) -> (x G + z S + sources + 32768) >> 16 BEFORE the clamp to int16
// (|value| < 2^23: it fits an int); the plain instances pass x through
template <int kMode, bool kSrc>
__device__ __forceinline__ void mix(int xI, int xQ, uint32_t uI, uint32_t uQ, Mixer<kSrc> &m, int &vI, int &vQ)
{
    if constexpr (!kMode && !kSrc) {
        vI = xI;
        vQ = xQ;
    } else {
        long long aI = 32768, aQ = 32768;
        if constexpr (kSrc) sources(m.ip, m.L, m.ct, aI, aQ);
        aI += (long long)xI * m.np.g;
        aQ += (long long)xQ * m.np.g;
        if constexpr (kMode != 0) {
            aI += (long long)gauss_q12(uI, m.gt) * m.np.s;
            aQ += (long long)gauss_q12(uQ, m.gt) * m.np.s;
        }
        vI = (int)(aI >> 16);
        vQ = (int)(aQ >> 16);
    }
}

// the eight values of vector `a` (index i of the call: the complex samples 4 i .. 4 i + 3) mixed, not yet clamped
template <int kMode, bool kSrc>
__device__ __forceinline__ void mix8(v4i a, uint64_t i, Mixer<kSrc> &m, int (&v)[8])
{
    uint32_t u[8] = {};
    if constexpr (kMode != 0) {
        const uint64_t b = (m.np.j0 >> 2) + 2 * i;  // the block of the vector's first value (mode 2: from its word 2 on)
        uint32_t b0[4], b1[4];
        philox(b, m.np.k0, m.np.k1, m.np.stream, 0u, b0);
        philox(b + 1, m.np.k0, m.np.k1, m.np.stream, 0u, b1);
        if constexpr (kMode == 2) {
            uint32_t b2[4];
            philox(b + 2, m.np.k0, m.np.k1, m.np.stream, 0u, b2);
            u[0] = b0[2], u[1] = b0[3], u[2] = b1[0], u[3] = b1[1], u[4] = b1[2], u[5] = b1[3], u[6] = b2[0], u[7] = b2[1];
        } else {
            u[0] = b0[0], u[1] = b0[1], u[2] = b0[2], u[3] = b0[3], u[4] = b1[0], u[5] = b1[1], u[6] = b1[2], u[7] = b1[3];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) mix<kMode, kSrc>((a[k] << 16) >> 16, a[k] >> 16, u[2 * k], u[2 * k + 1], m, v[2 * k], v[2 * k + 1]);
}

// one complex sample of the tail: the values j, j + 1 of the call (j even: both lie in one Philox block)
template <int kMode, bool kSrc>
__device__ __forceinline__ void mix2(int xI, int xQ, uint64_t j, Mixer<kSrc> &m, int &vI, int &vQ)
{
    uint32_t o[4] = {};
    const uint64_t J = m.np.j0 + j;
    if constexpr (kMode != 0) philox(J >> 2, m.np.k0, m.np.k1, m.np.stream, 0u, o);
    const bool hi = (J & 2) != 0;
    mix<kMode, kSrc>(xI, xQ, hi ? o[2] : o[0], hi ? o[3] : o[1], m, vI, vQ);
}

// ---- formats -------------------------------------------------------------------------------------------------------------------
// f16 and f8 of a mixed value before the clamp to int16: iq_dev.h
__device__ __forceinline__ uint32_t f1(int v, uint32_t &sat)
{
    sat += (uint32_t)((v < -32768) | (v > 32767));
    return (uint32_t)(v > 0);
}

// A format: kVec 16-byte vectors (4 kVec complex samples) per lane and trip, run kUnrollMixed at a time in the mixed instances (the
// plain ones issue all loads of a trip at once); pack() turns the eight mixed values of vector k into kWords / kVec words of w[];
// join() makes the trip's one store of them; tail() stores one complex sample (j even; `acc` is the lane's own between calls).
struct FmtShort {  // in and out may be the same buffer: a lane reads its vector before it writes it, and no other lane touches it
    typedef const int16_t *in_t;
    typedef int16_t *out_t;
    typedef v4i store_t;
    static constexpr int kVec = 1, kWords = 4, kUnrollMixed = 1;
    static constexpr bool kPlainCounts = false;  // (no plain instance)
    static __device__ __forceinline__ void pack(const int (&v)[8], uint32_t *w, int, int, uint32_t &cnt)
    {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = f16(v[2 * k], cnt) | (f16(v[2 * k + 1], cnt) << 16);
    }
    static __device__ __forceinline__ store_t join(const uint32_t (&w)[kWords]) { return store_t{(int)w[0], (int)w[1], (int)w[2], (int)w[3]}; }
    static __device__ __forceinline__ void tail(out_t out, uint64_t j, uint64_t, int vI, int vQ, int, int, uint32_t &cnt, uint32_t &)
    {
        out[j] = (int16_t)f16(vI, cnt);
        out[j + 1] = (int16_t)f16(vQ, cnt);
    }
};

struct FmtByte {
    typedef const int16_t *__restrict__ in_t;
    typedef int8_t *__restrict__ out_t;
    typedef v4i store_t;
    static constexpr int kVec = 2, kWords = 4, kUnrollMixed = 2;
    static constexpr bool kPlainCounts = true;  // a plain value may leave +-127 after the shift
    static __device__ __forceinline__ void pack(const int (&v)[8], uint32_t *w, int s, int r, uint32_t &cnt)
    {
        w[0] = f8(v[0], s, r, cnt) | (f8(v[1], s, r, cnt) << 8) | (f8(v[2], s, r, cnt) << 16) | (f8(v[3], s, r, cnt) << 24);
        w[1] = f8(v[4], s, r, cnt) | (f8(v[5], s, r, cnt) << 8) | (f8(v[6], s, r, cnt) << 16) | (f8(v[7], s, r, cnt) << 24);
    }
    static __device__ __forceinline__ store_t join(const uint32_t (&w)[kWords]) { return store_t{(int)w[0], (int)w[1], (int)w[2], (int)w[3]}; }
    static __device__ __forceinline__ void tail(out_t out, uint64_t j, uint64_t, int vI, int vQ, int s, int r, uint32_t &cnt, uint32_t &)
    {
        out[j] = (int8_t)f8(vI, s, r, cnt);
        out[j + 1] = (int8_t)f8(vQ, s, r, cnt);
    }
};

struct FmtBit {
    typedef const int16_t *__restrict__ in_t;
    typedef uint8_t *__restrict__ out_t;
    typedef uint2 store_t;
    static constexpr int kVec = 8, kWords = 8, kUnrollMixed = 2;  // one byte of bits per vector
    static constexpr bool kPlainCounts = false;
    static __device__ __forceinline__ void pack(const int (&v)[8], uint32_t *w, int, int, uint32_t &cnt)
    {
        uint32_t b = 0;
#pragma unroll
        for (int m = 0; m < 8; ++m) b |= f1(v[m], cnt) << (7 - m);
        w[0] = b;
    }
    static __device__ __forceinline__ store_t join(const uint32_t (&w)[kWords])
    {
        return make_uint2(w[0] | (w[1] << 8) | (w[2] << 16) | (w[3] << 24), w[4] | (w[5] << 8) | (w[6] << 16) | (w[7] << 24));
    }
    // the tail starts at a byte: four complex samples to a byte, and the last byte is stored as far as it got
    static __device__ __forceinline__ void tail(out_t out, uint64_t j, uint64_t n_val, int vI, int vQ, int, int, uint32_t &cnt, uint32_t &acc)
    {
        const int k = (int)(j & 7);
        acc |= (f1(vI, cnt) << (7 - k)) | (f1(vQ, cnt) << (6 - k));
        if (k == 6 || j + 2 >= n_val) {
            out[j >> 3] = (uint8_t)acc;
            acc = 0;
        }
    }
};

// n_val (even) int16 values at `in` -> the same number of values in the format at `out`, both 16-byte aligned; s = the ibyte shift
template <class Fmt, int kMode, bool kSrc>
__global__ __launch_bounds__(kThreads) void k_iq_pass(typename Fmt::in_t in, typename Fmt::out_t out, uint64_t n_val, int s, NoiseArgs np,
                                                      std::conditional_t<kSrc, InterfArgs, NoSrcArgs> ip, unsigned long long *sat)
{
    constexpr bool kMixed = kMode != 0 || kSrc;
    constexpr int kUnroll = kMixed ? Fmt::kUnrollMixed : Fmt::kVec;
    constexpr int kRun = 4 * Fmt::kVec;  // complex samples per lane and trip
    Mixer<kSrc> m{np, ip, {}, nullptr, nullptr};
    if constexpr (kMode != 0) m.gt = load_gauss_table();
    if constexpr (kSrc) m.ct = load_cos_table();
    const int r = s ? 1 << (s - 1) : 0;
    const uint64_t n_trip = n_val / (2 * kRun);
    const v4i *vin = (const v4i *)in;
    typename Fmt::store_t *vout = (typename Fmt::store_t *)out;
    uint32_t cnt = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    const uint32_t lane = blockIdx.x * kThreads + threadIdx.x;
    if constexpr (kSrc)
        if (lane < n_trip) seek(ip, m.L, kRun * lane);
    for (uint64_t i = lane; i < n_trip; i += stride) {
        uint32_t w[Fmt::kWords];
#pragma unroll kUnroll
        for (int k = 0; k < Fmt::kVec; ++k) {
            int v[8];
            mix8<kMode, kSrc>(vin[Fmt::kVec * i + k], Fmt::kVec * i + k, m, v);
            Fmt::pack(v, &w[k * (Fmt::kWords / Fmt::kVec)], s, r, cnt);
        }
        vout[i] = Fmt::join(w);
        if constexpr (kSrc) jump(ip, m.L);
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0 && n_trip * (2 * kRun) < n_val) {  // tail: fewer than kRun complex samples
        if constexpr (kSrc) seek_tail(ip, m.L);
        uint32_t acc = 0;
        for (uint64_t j = n_trip * (2 * kRun); j < n_val; j += 2) {
            int vI, vQ;
            mix2<kMode, kSrc>(in[j], in[j + 1], j, m, vI, vQ);
            Fmt::tail(out, j, n_val, vI, vQ, s, r, cnt, acc);
        }
    }
    if constexpr (kMixed || Fmt::kPlainCounts) add_block_count<kThreads>(cnt, sat);
}

struct PassCall {
    const int16_t *in;
    void *out;
    uint64_t n_val;
    int shift;
    NoiseArgs np;
    InterfArgs ip;
    unsigned long long *sat;
    dim3 grid;
    hipStream_t st;
};

template <class Fmt, int kMode, bool kSrc>
void launch(const PassCall &c)
{
    std::conditional_t<kSrc, InterfArgs, NoSrcArgs> ip;
    if constexpr (kSrc) ip = c.ip;
    hipLaunchKernelGGL((k_iq_pass<Fmt, kMode, kSrc>), c.grid, dim3(kThreads), 0, c.st, (typename Fmt::in_t)c.in, (typename Fmt::out_t)c.out, c.n_val,
                       c.shift, c.np, ip, c.sat);
}

// [format][mode][sources]: the 17 instances (plain ishort is the caller's copy)
void (*const kLaunch[3][3][2])(const PassCall &) = {
    {{nullptr, launch<FmtShort, 0, true>}, {launch<FmtShort, 1, false>, launch<FmtShort, 1, true>}, {launch<FmtShort, 2, false>, launch<FmtShort, 2, true>}},
    {{launch<FmtByte, 0, false>, launch<FmtByte, 0, true>}, {launch<FmtByte, 1, false>, launch<FmtByte, 1, true>}, {launch<FmtByte, 2, false>, launch<FmtByte, 2, true>}},
    {{launch<FmtBit, 0, false>, launch<FmtBit, 0, true>}, {launch<FmtBit, 1, false>, launch<FmtBit, 1, true>}, {launch<FmtBit, 2, false>, launch<FmtBit, 2, true>}},
};

uint32_t tri_host(uint32_t m) { return (uint32_t)(((uint64_t)m * (uint64_t)(m ? m - 1 : 0)) >> 1); }

}  // namespace

extern "C" const int32_t *gal_tables_gauss(void) { return &kGaussT[0][0][0]; }
extern "C" const int16_t *gal_tables_cos1024(void) { return kInterfCos; }

// format 0 (ishort), 1 (ibyte) or 2 (ibit) of n_val int16 values with the noise floor (noise may be null: none) and n_src sources
// mixed in; with neither it is the plain conversion (not of format 0: that is a copy).  Arguments are checked by the caller
// (iq_api.cpp: iq_pass).
extern "C" hipError_t galk_launch_iq_pass(int format, const int16_t *in, uint64_t n_val, uint64_t first_sample, const gal_iq_noise_t *noise,
                                          const gal_iq_interf_t *src, int n_src, int shift, void *out, unsigned long long *sat, hipStream_t st)
{
    PassCall c;
    memset(&c, 0, sizeof(c));
    c.in = in;
    c.out = out;
    c.n_val = n_val;
    c.shift = shift;
    c.sat = sat;
    c.st = st;
    c.np.j0 = 2 * first_sample;
    c.np.g = 65536;
    if (noise) {
        c.np.k0 = (uint32_t)noise->seed;
        c.np.k1 = (uint32_t)(noise->seed >> 32);
        c.np.stream = noise->stream;
        c.np.g = (int)noise->gain_q16;
        c.np.s = (int)noise->sigma_q4;
    }
    const int run = format == 0 ? 4 : format == 1 ? 8 : 32;  // complex samples a lane handles per trip
    const uint64_t n_trip = n_val / (2 * (uint64_t)run), b = (n_trip + kThreads - 1) / kThreads;
    c.grid = dim3(b < 1 ? 1u : b > (uint64_t)kMaxBlocks ? (unsigned)kMaxBlocks : (unsigned)b);
    const uint64_t jump = (uint64_t)c.grid.x * kThreads * run - run;  // < 2^24
    const uint64_t tail = first_sample + n_trip * run;
    for (int k = 0; k < n_src; ++k) {
        if (src[k].amp_q4 == 0) continue;  // adds nothing
        InterfSrc &s = c.ip.src[c.ip.n++];
        s.amp = (int)src[k].amp_q4;
        s.ph0 = src[k].ph0;
        s.f0 = (uint32_t)src[k].f0;
        s.len = src[k].sweep_len ? src[k].sweep_len : 1u;  // CW: sweeps of one sample, W = f0
        s.df = src[k].sweep_len ? (uint32_t)src[k].df : 0u;
        s.w = s.len * s.f0 + s.df * tri_host(s.len);
        s.period = src[k].pulse_period ? src[k].pulse_period : 1u;
        s.on = src[k].pulse_period ? src[k].pulse_on : 1u;
        s.s0 = (uint32_t)(first_sample / s.len);
        s.m0 = (uint32_t)(first_sample % s.len);
        s.p0 = (uint32_t)(first_sample % s.period);
        s.ts = (uint32_t)(tail / s.len);
        s.tm = (uint32_t)(tail % s.len);
        s.tp = (uint32_t)(tail % s.period);
        s.jq = (uint32_t)(jump / s.len);
        s.jr = (uint32_t)(jump % s.len);
        s.jp = (uint32_t)(jump % s.period);
    }
    // without sources a given noise floor always runs (G applies even where S = 0); with them S = 0 needs no random work (z S = 0)
    const bool random = noise && (n_src == 0 || noise->sigma_q4 != 0);
    const int mode = !random ? 0 : (first_sample & 1) ? 2 : 1;
    kLaunch[format][mode][n_src > 0](c);
    return hipGetLastError();
}
