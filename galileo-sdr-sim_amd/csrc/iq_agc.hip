// iq_agc.hip -- the block AGC in front of the quantiser and the 2-bit format (include/galsynth.h: gal_synth_agc_set, gal_synth_iq_agc;
// DESIGN.md section 17).  y[n] = (I, Q)[n] the complex int16 samples of the WHOLE stream, block b = the samples [b B, (b + 1) B):
//
//   P[b]  = sum over the 2 B values of block b of y^2 (64-bit, exact);  P[b] = p_init for blocks in front of the stream
//   Q[b]  = P[b - W] + ... + P[b - 1]                         (the W blocks BEFORE b: every gain is known before its block begins)
//   g[b]  = clamp((target_q8 << 12) div max(isqrt((Q[b] << 16) div (2 B W)), 1), gain_min_q12, gain_max_q12)
//   z     = clamp16((int64(y) g[b] + 2048) >> 12)             (arithmetic shift), b the block of the value's sample
//   out   z in the format: ishort z; ibyte (z + r) >> s clamped to +-127 (iq_dev.h: f8); i2bit q = (z > thr) + (z > 0) + (z > -thr) - 2,
//         the code q & 3, four codes per byte with value 4k in bits 7..6, unused low bits of the last byte 0
//
// A value counts once as saturated if the int16 clamp or ibyte's +-127 clamp changed it.  Everything is integer arithmetic
// (tests/agc_model.py states it in numpy).
//
// A call takes the next n samples of the stream, local index i = 0 .. n - 1.  The device sees positions RELATIVE to the block that is
// open when the call begins: off0 = position mod B (the host keeps the position), block j of the call = block (position div B) + j.
// The call touches the blocks j = 0 .. nt - 1, nt = (off0 + n - 1) div B + 1, and completes the first nc = (off0 + n) div B of them.
// Three launches, no host synchronisation between them or between calls:
//
//   k_agc_power   sums[j] = the sum of squares of the call's samples in block j.  A workgroup owns a chunk of 16384 consecutive
//                 samples; a lane takes a run of 16 (four 16-byte loads), which crosses at most one block edge because B >= 16, and
//                 splits its sum there -- the edges fall anywhere relative to the 16-byte grid.  The lanes' sums meet in a segmented
//                 wave scan over the block index (shuffles), the last lane of each segment adds to the chunk's partials in LDS, and
//                 the chunk adds each of its blocks ONCE to sums[] (zeroed by the launcher).  Integer sums: any order is exact.
//   k_agc_gains   one lane per block touched: the window sum from the history and the call's complete blocks, isqrt (v_sqrt_f64 plus an
//                 integer fix-up), two 64-bit divisions; g to the call's gain table and, for the blocks that START in the call, to the
//                 caller's array.  The same launch rolls the state forward -- the powers of the last W complete blocks and the partial
//                 sum of the block left open -- from one of the handle's two state buffers into the other.
//   k_iq_agc<Fmt> apply and format, iq_pass.hip's shape: 16-byte loads, 64-bit indices, a grid-stride loop, one store per lane and
//                 trip, the samples behind the last whole trip in one lane.  A lane finds the block of its first run with one 32-bit
//                 division, steps the position sample by sample inside a run, and jumps to its next run with the host's (jump div B,
//                 jump mod B) and one conditional correction.  Saturated values: per lane, per wave, per block, one atomic per block.
#include "../../include/galsynth.h"
#include "iq_dev.h"

namespace {

// tests/agc_model.py repeats kThreads (iq_dev.h), kMaxBlocks, kPowChunk and the formats' runs (4 x kVec) as THREADS, MAX_BLOCKS, POWER_CHUNK and RUN:
// the GPU tests place their sizes at these edges.  Change them there too, or the edge sizes go stale without a failure.
constexpr int kMaxBlocks = 2048;  // 8 blocks of 4 waves per CU, the rest by the grid-stride loop
constexpr int kHistMax = GAL_AGC_MAX_WINDOW;  // a state buffer: [0 .. W-1] the powers of the last W complete blocks, oldest first; [kHistMax] the open block's partial sum

constexpr int kPowRun = 16;                                // samples per lane and trip of k_agc_power
constexpr int kPowTrips = 4;                               // trips per chunk
constexpr int kPowTrip = kThreads * kPowRun;               // 4096 samples
constexpr int kPowChunk = kPowTrip * kPowTrips;            // 16384 samples per workgroup
constexpr int kPowSlots = kPowChunk / GAL_AGC_MIN_BLOCK + 2;  // blocks a chunk can touch: (B - 1 + 16383) div B + 1 <= 1025 at B = 16
static_assert(kPowRun <= GAL_AGC_MIN_BLOCK, "a run of k_agc_power crosses at most one block edge");

// I^2 + Q^2 of one complex sample: at most 2^31, exact as an unsigned 32-bit number
__device__ __forceinline__ uint32_t power(uint32_t w)
{
    return (uint32_t)__builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, w), __builtin_bit_cast(v2s, w), 0, false);
}

// in: n >= 1 complex samples, 16-byte aligned; B the block length, off0 < B; (jq, jr) = (kPowTrip div B, kPowTrip mod B);
// sums: nt words, zeroed
__global__ __launch_bounds__(kThreads) void k_agc_power(const uint32_t *__restrict__ in, uint64_t n, uint32_t off0, uint32_t B, uint32_t jq, uint32_t jr,
                                                        unsigned long long *__restrict__ sums)
{
    __shared__ unsigned long long part[kPowSlots];
    const int t = threadIdx.x, wl = t & 63;
    const uint64_t c0 = (uint64_t)blockIdx.x * kPowChunk;  // the chunk's first sample
    const uint64_t base = (uint64_t)off0 + c0, kb = base / B;  // kb: the chunk's first block
    const uint32_t rb = (uint32_t)(base - kb * B);
    const uint64_t left = n - c0;
    const uint32_t len = left < (uint64_t)kPowChunk ? (uint32_t)left : (uint32_t)kPowChunk;  // samples of the chunk, >= 1
    const uint32_t nb = (rb + len - 1) / B + 1;  // blocks the chunk touches, <= kPowSlots - 1
    for (uint32_t k = t; k < nb; k += kThreads) part[k] = 0;
    __syncthreads();
    // the lane's run begins at block q of the chunk, `rem` samples into it
    uint32_t q = (rb + (uint32_t)t * kPowRun) / B, rem = rb + (uint32_t)t * kPowRun - q * B;
    for (int trip = 0; trip < kPowTrips; ++trip) {
        const uint32_t s = (uint32_t)trip * kPowTrip + (uint32_t)t * kPowRun;  // the run's first sample in the chunk
        if ((uint32_t)trip * kPowTrip >= len) break;  // (the same in every lane)
        unsigned long long a = 0, b = 0;  // the run's sums in block q and in block q + 1
        if (s < len) {
            const uint32_t *src = in + c0 + s;
            uint32_t w[kPowRun];
            if (s + kPowRun <= len) {
#pragma unroll
                for (int k = 0; k < kPowRun / 4; ++k) {
                    const v4i v = ((const v4i *)src)[k];
#pragma unroll
                    for (int m = 0; m < 4; ++m) w[4 * k + m] = (uint32_t)v[m];
                }
            } else {  // the call's last samples
#pragma unroll
                for (int m = 0; m < kPowRun; ++m) w[m] = s + m < len ? src[m] : 0u;
            }
            const uint32_t e = B - rem;  // the first e samples of the run lie in block q
#pragma unroll
            for (int m = 0; m < kPowRun; ++m) {
                const unsigned long long sq = power(w[m]);
                a += (uint32_t)m < e ? sq : 0ull;
                b += (uint32_t)m < e ? 0ull : sq;
            }
        }
        // segmented inclusive scan over the wave: q does not fall from lane to lane, so lanes with equal q are neighbours
        unsigned long long v = a;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long v2 = __shfl_up(v, o, 64);
            const uint32_t q2 = __shfl_up(q, o, 64);
            if (wl >= o && q2 == q) v += v2;
        }
        const uint32_t qn = __shfl_down(q, 1, 64);
        if ((wl == 63 || qn != q) && v) atomicAdd(&part[q], v);  // (v != 0: a sample of the call lies in block q, q < nb)
        if (b) atomicAdd(&part[q + 1], b);
        q += jq;
        rem += jr;
        if (rem >= B) {
            rem -= B;
            ++q;
        }
    }
    __syncthreads();
    for (uint32_t k = t; k < nb; k += kThreads) {
        const unsigned long long v = part[k];
        if (v) atomicAdd(&sums[kb + k], v);
    }
}

struct Shape {
    uint32_t B, W;
    unsigned long long den;     // 2 B W
    unsigned long long target;  // target_q8 << 12
    uint32_t gmin, gmax;
};

// floor(sqrt(v)), v <= 2^46 (exact as a double); the hardware's square root is not trusted: r^2 <= v < (r + 1)^2 by integer steps
__device__ __forceinline__ unsigned long long isqrt(unsigned long long v)
{
    unsigned long long r = (unsigned long long)__builtin_amdgcn_sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// sums: the call's nt block sums; nc: blocks the call completes; open: the call ends inside a block (then nc == nt - 1);
// st_in -> st_out: the handle's state; gains: nt + 1 words, the last one 0 (see step()); gains_out: null, or nt - (off0 != 0) words
__global__ __launch_bounds__(kThreads) void k_agc_gains(const unsigned long long *__restrict__ sums, uint64_t nt, uint64_t nc, uint32_t off0, int open,
                                                        Shape S, const unsigned long long *__restrict__ st_in, unsigned long long *__restrict__ st_out,
                                                        uint32_t *__restrict__ gains, uint32_t *__restrict__ gains_out)
{
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const int W = (int)S.W;
    // the power of block m of the call (m >= -W; m < 0: from the history; 0: the open block's partial sum goes in)
    auto P = [&](long long m) -> unsigned long long { return m < 0 ? st_in[W + m] : (m == 0 ? st_in[kHistMax] : 0ull) + sums[m]; };
    if (j < nt) {
        unsigned long long Q = 0;
        for (int i = 1; i <= W; ++i) Q += P((long long)j - i);
        const unsigned long long rms = isqrt((Q << 16) / S.den);
        unsigned long long g = S.target / (rms ? rms : 1ull);
        g = g < S.gmin ? S.gmin : g > S.gmax ? S.gmax : g;
        gains[j] = (uint32_t)g;
        if (gains_out && (j > 0 || off0 == 0)) gains_out[j - (off0 != 0)] = (uint32_t)g;
    }
    if (j < (uint64_t)W) st_out[j] = P((long long)nc - W + (long long)j);
    if (j == 0) {
        st_out[kHistMax] = open ? P((long long)nc) : 0ull;
        gains[nt] = 0;
    }
}

// ---- apply and format ----------------------------------------------------------------------------------------------------------
// (y g + 2048) >> 12 BEFORE the clamp to int16: |y g| <= 2^39, the result fits an int
__device__ __forceinline__ int scaled(int y, uint32_t g) { return (int)(((long long)y * (long long)(int)g + 2048) >> 12); }

// f16 and f8 of a scaled value before the clamp to int16: iq_dev.h
// the 2-bit code: the magnitude saturates by design and is not counted
__device__ __forceinline__ uint32_t f2(int v, int thr, uint32_t &sat)
{
    const int z = clamp16(v);
    sat += (uint32_t)(z != v);
    return (uint32_t)((int)(z > thr) + (int)(z > 0) + (int)(z > -thr) - 2) & 3u;
}

// A format (iq_pass.hip: FmtShort, FmtByte; the 2-bit one is new): kVec 16-byte vectors per lane and trip; pack() turns the eight
// scaled values of one vector into kWords / kVec words; join() makes the trip's one store; tail() stores complex sample s of the call.
// p = the ibyte shift or the i2bit threshold, r = the ibyte rounding term.
struct FmtShort {
    typedef int16_t *__restrict__ out_t;
    typedef v4i store_t;
    static constexpr int kVec = 1, kWords = 4;
    static __device__ __forceinline__ void pack(const int (&v)[8], uint32_t *w, int, int, uint32_t &cnt)
    {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = f16(v[2 * k], cnt) | (f16(v[2 * k + 1], cnt) << 16);
    }
    static __device__ __forceinline__ store_t join(const uint32_t (&w)[kWords]) { return store_t{(int)w[0], (int)w[1], (int)w[2], (int)w[3]}; }
    static __device__ __forceinline__ void tail(out_t out, uint64_t s, uint64_t, int vI, int vQ, int, int, uint32_t &cnt, uint32_t &)
    {
        out[2 * s] = (int16_t)f16(vI, cnt);
        out[2 * s + 1] = (int16_t)f16(vQ, cnt);
    }
};

struct FmtByte {
    typedef int8_t *__restrict__ out_t;
    typedef v4i store_t;
    static constexpr int kVec = 2, kWords = 4;
    static __device__ __forceinline__ void pack(const int (&v)[8], uint32_t *w, int s, int r, uint32_t &cnt)
    {
        w[0] = f8(v[0], s, r, cnt) | (f8(v[1], s, r, cnt) << 8) | (f8(v[2], s, r, cnt) << 16) | (f8(v[3], s, r, cnt) << 24);
        w[1] = f8(v[4], s, r, cnt) | (f8(v[5], s, r, cnt) << 8) | (f8(v[6], s, r, cnt) << 16) | (f8(v[7], s, r, cnt) << 24);
    }
    static __device__ __forceinline__ store_t join(const uint32_t (&w)[kWords]) { return store_t{(int)w[0], (int)w[1], (int)w[2], (int)w[3]}; }
    static __device__ __forceinline__ void tail(out_t out, uint64_t s, uint64_t, int vI, int vQ, int sh, int r, uint32_t &cnt, uint32_t &)
    {
        out[2 * s] = (int8_t)f8(vI, sh, r, cnt);
        out[2 * s + 1] = (int8_t)f8(vQ, sh, r, cnt);
    }
};

struct Fmt2Bit {
    typedef uint8_t *__restrict__ out_t;
    typedef uint2 store_t;
    static constexpr int kVec = 4, kWords = 4;  // two bytes of codes per vector
    static __device__ __forceinline__ void pack(const int (&v)[8], uint32_t *w, int thr, int, uint32_t &cnt)
    {
        const uint32_t b0 = (f2(v[0], thr, cnt) << 6) | (f2(v[1], thr, cnt) << 4) | (f2(v[2], thr, cnt) << 2) | f2(v[3], thr, cnt);
        const uint32_t b1 = (f2(v[4], thr, cnt) << 6) | (f2(v[5], thr, cnt) << 4) | (f2(v[6], thr, cnt) << 2) | f2(v[7], thr, cnt);
        w[0] = b0 | (b1 << 8);
    }
    static __device__ __forceinline__ store_t join(const uint32_t (&w)[kWords]) { return make_uint2(w[0] | (w[1] << 16), w[2] | (w[3] << 16)); }
    // the tail starts at a byte: two complex samples to a byte, and the last byte is stored as far as it got
    static __device__ __forceinline__ void tail(out_t out, uint64_t s, uint64_t n, int vI, int vQ, int thr, int, uint32_t &cnt, uint32_t &acc)
    {
        const int sh = (s & 1) ? 0 : 4;
        acc |= ((f2(vI, thr, cnt) << 2) | f2(vQ, thr, cnt)) << sh;
        if ((s & 1) || s + 1 >= n) {
            out[s >> 1] = (uint8_t)acc;
            acc = 0;
        }
    }
};

// where a lane stands in the stream: block q of the call, `rem` samples into it, g = gains[q]
struct Pos {
    uint64_t q;
    uint32_t rem, g;
};

// the next sample; a new block's gain is loaded as its first sample comes up (behind a call that ends on a block edge this reads
// gains[nt], which k_agc_gains sets to 0 and nobody uses)
__device__ __forceinline__ void step(Pos &p, uint32_t B, const uint32_t *__restrict__ gains)
{
    if (++p.rem == B) {
        p.rem = 0;
        p.g = gains[++p.q];
    }
}

// n complex samples at `in` -> the format at `out`, both 16-byte aligned; p = the ibyte shift / i2bit threshold; (jq, jr) = the
// samples from one run of a lane to its next, div and mod B; (tq, tr) = where the tail's first sample stands; gains: nt + 1 words
template <class Fmt>
__global__ __launch_bounds__(kThreads) void k_iq_agc(const int16_t *__restrict__ in, typename Fmt::out_t out, uint64_t n, int p, uint32_t B, uint32_t off0,
                                                     uint32_t jq, uint32_t jr, uint64_t tq, uint32_t tr, const uint32_t *__restrict__ gains,
                                                     unsigned long long *sat)
{
    constexpr int kRun = 4 * Fmt::kVec;  // complex samples per lane and trip
    const int r = p ? 1 << (p - 1) : 0;  // (ibyte only)
    const uint64_t n_trip = n / kRun;
    const v4i *vin = (const v4i *)in;
    typename Fmt::store_t *vout = (typename Fmt::store_t *)out;
    uint32_t cnt = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    const uint32_t lane = blockIdx.x * kThreads + threadIdx.x;
    // the lane's first run begins at sample kRun x lane: off0 + kRun x lane < 2^16 + 2^23
    uint64_t q0 = (off0 + (uint32_t)kRun * lane) / B;
    uint32_t rem0 = off0 + (uint32_t)kRun * lane - (uint32_t)q0 * B;
    for (uint64_t i = lane; i < n_trip; i += stride) {
        Pos ps{q0, rem0, gains[q0]};
        uint32_t w[Fmt::kWords];
#pragma unroll
        for (int k = 0; k < Fmt::kVec; ++k) {
            const v4i a = vin[Fmt::kVec * i + k];
            int v[8];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                v[2 * m] = scaled((a[m] << 16) >> 16, ps.g);
                v[2 * m + 1] = scaled(a[m] >> 16, ps.g);
                step(ps, B, gains);
            }
            Fmt::pack(v, &w[k * (Fmt::kWords / Fmt::kVec)], p, r, cnt);
        }
        vout[i] = Fmt::join(w);
        q0 += jq;
        rem0 += jr;
        if (rem0 >= B) {
            rem0 -= B;
            ++q0;
        }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0 && n_trip * kRun < n) {  // tail: fewer than kRun complex samples
        Pos ps{tq, tr, gains[tq]};
        uint32_t acc = 0;
        for (uint64_t s = n_trip * kRun; s < n; ++s) {
            const int vI = scaled(in[2 * s], ps.g), vQ = scaled(in[2 * s + 1], ps.g);
            Fmt::tail(out, s, n, vI, vQ, p, r, cnt, acc);
            step(ps, B, gains);
        }
    }
    add_block_count<kThreads>(cnt, sat);
}

template <class Fmt>
void launch(const int16_t *in, void *out, uint64_t n, int p, uint32_t B, uint32_t off0, const uint32_t *gains, unsigned long long *sat, hipStream_t st)
{
    constexpr uint64_t kRun = 4 * Fmt::kVec;
    const uint64_t n_trip = n / kRun, b = (n_trip + kThreads - 1) / kThreads;
    const unsigned grid = b < 1 ? 1u : b > (uint64_t)kMaxBlocks ? (unsigned)kMaxBlocks : (unsigned)b;
    const uint64_t jump = (uint64_t)grid * kThreads * kRun;  // <= 2^23
    const uint64_t tail = (uint64_t)off0 + n_trip * kRun;
    hipLaunchKernelGGL((k_iq_agc<Fmt>), dim3(grid), dim3(kThreads), 0, st, in, (typename Fmt::out_t)out, n, p, B, off0, (uint32_t)(jump / B),
                       (uint32_t)(jump % B), tail / B, (uint32_t)(tail % B), gains, sat);
}

}  // namespace

// The bytes of a call's scratch -- nt 64-bit block sums, then nt + 1 32-bit gains -- for a call of n >= 1 samples that begins off0
// samples into a block.  Host only.
extern "C" uint64_t galk_agc_scratch_bytes(uint64_t n, uint32_t off0, uint32_t block_len)
{
    const uint64_t nt = ((uint64_t)off0 + n - 1) / block_len + 1;
    return 8 * nt + 4 * (nt + 1);
}

// n >= 1 samples (< 2^41) that begin off0 < block_len samples into a block; format GAL_IQ_ISHORT, GAL_IQ_IBYTE or GAL_IQ_I2BIT; state_in /
// state_out: GAL_AGC_MAX_WINDOW + 1 words each; scratch: galk_agc_scratch_bytes, 8-byte aligned; gains_out may be null.  Arguments are
// checked by the caller (iq_api.cpp: gal_synth_iq_agc).
extern "C" hipError_t galk_launch_iq_agc(const int16_t *in, uint64_t n, uint32_t off0, int format, int param, const gal_iq_agc_t *p,
                                         const unsigned long long *state_in, unsigned long long *state_out, void *scratch, void *out,
                                         uint32_t *gains_out, unsigned long long *sat, hipStream_t st)
{
    const uint32_t B = p->block_len;
    const uint64_t end = (uint64_t)off0 + n, nt = (end - 1) / B + 1, nc = end / B;
    unsigned long long *sums = (unsigned long long *)scratch;
    uint32_t *gains = (uint32_t *)(sums + nt);
    hipError_t err = hipMemsetAsync(sums, 0, 8 * nt, st);
    if (err != hipSuccess) return err;
    const uint64_t chunks = (n + kPowChunk - 1) / kPowChunk;  // < 2^27
    hipLaunchKernelGGL(k_agc_power, dim3((unsigned)chunks), dim3(kThreads), 0, st, (const uint32_t *)in, n, off0, B, (uint32_t)kPowTrip / B,
                       (uint32_t)kPowTrip % B, sums);
    Shape S;
    S.B = B;
    S.W = p->window;
    S.den = 2ull * B * p->window;
    S.target = (unsigned long long)p->target_q8 << 12;
    S.gmin = p->gain_min_q12;
    S.gmax = p->gain_max_q12;
    hipLaunchKernelGGL(k_agc_gains, dim3((unsigned)((nt + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, sums, nt, nc, off0, (int)(end % B != 0), S,
                       state_in, state_out, gains, gains_out);
    if (format == GAL_IQ_ISHORT) launch<FmtShort>(in, out, n, param, B, off0, gains, sat, st);
    else if (format == GAL_IQ_IBYTE) launch<FmtByte>(in, out, n, param, B, off0, gains, sat, st);
    else launch<Fmt2Bit>(in, out, n, param, B, off0, gains, sat, st);
    return hipGetLastError();
}
