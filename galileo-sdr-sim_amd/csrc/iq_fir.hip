// iq_fir.hip -- the front-end (IF) FIR filter of the output stream (include/galsynth.h: gal_synth_fir_set, gal_synth_iq_fir; DESIGN.md
// section 15).  x[n] = (I, Q)[n] the complex int16 samples of the WHOLE stream, x[n] = 0 for n < 0; h[0 .. T-1] real int16 taps in Q14,
// 1 <= T <= 128.  Per rail, in integers:
//
//   a[n] = sum over k of h[k] x[n - k]
//   y[n] = clamp16((a[n] + 8192) >> 14)            (arithmetic shift: round to nearest, ties up)
//
// A value the clamp changes counts once as saturated.  The host admits only taps with sum |h[k]| <= 65535 (gal_synth_fir_check): then
// |a| + 8192 <= 65535 x 32768 + 8192 < 2^31 for ANY int16 input, and one int32 accumulator is exact (every partial sum is bounded the
// same way).  Integer arithmetic only: a fixed function of (taps, stream) on any machine and for any cut of the stream into calls
// (tests/fir_model.py states it in numpy).
//
// The stream across calls: the handle keeps the last kHist = 128 input samples of the stream (zeros in front of its start) in one of
// two small device buffers; a call reads the one the call before it wrote and writes the other, so no block of a launch reads what
// another block of the same launch writes, and launches of one handle are ordered by its stream.  The new history is the last 128
// samples of (old history, input): block 0 writes it, part old history and part input where the call is shorter than 128 samples.
//
// Shape.  One block filters a tile of kTile = 1024 consecutive output samples, 4 per lane.  It stages the tile and the Hs = T - 1
// rounded up to a multiple of 4 samples in front of it ONCE in LDS, with 16-byte loads (vectors that begin in front of the call come
// out of the history, which is laid out so that they are whole vectors too; a vector the end of the call cuts is read with 4-byte
// accesses, one sample at a time; what lies behind the call is 0 and multiplies nothing that reaches an output the call stores).
// I and Q are de-interleaved on the way: two int16 planes, so that a 32-bit LDS word holds two consecutive samples of ONE rail and
// v_dot2_i32_i16 covers two taps per instruction.
//
// With G[m], m = 0 .. Hs, the taps reversed and shifted to the staged window (G[m] = h[Hs - m], 0 beyond the taps) an output is
// a[n] = sum over m of G[m] s[n + m].  A lane owns the outputs n0 .. n0 + 3 (n0 = 4 lane) and walks the window in aligned words
// W[j] = (s[n0 + 2j], s[n0 + 2j + 1]):
//   a[n0]     = sum_j W[j]     . GE[j],   GE[j] = (G[2j],     G[2j + 1])
//   a[n0 + 1] = sum_j W[j]     . GO[j],   GO[j] = (G[2j - 1], G[2j])          (the same words against the taps moved by one)
//   a[n0 + 2] = sum_j W[j + 1] . GE[j]
//   a[n0 + 3] = sum_j W[j + 1] . GO[j]
// so no word is ever formed from two halves.  Words are read two at a time (8-byte LDS reads, consecutive lanes 8 bytes apart: no bank
// conflict); one trip of the loop takes one such read per rail and 16 dot products.  The tap pairs are the host's table
// (GE[2i], GO[2i], GE[2i + 1], GO[2i + 1]) per trip i, padded with zeros to whole trips, read through a uniform address: scalar
// loads, the taps sit in SGPRs.  64-bit sample indices throughout.  Saturated values are counted per lane, per wave, per block, one
// atomic per block that saw one (iq_dev.h: add_block_count).
#include "../../include/galsynth.h"
#include "iq_dev.h"

namespace {

constexpr int kTile = 4 * kThreads;  // complex samples per block
constexpr int kHist = 128;           // history the handle keeps: the last 128 input samples (>= GAL_FIR_MAX_TAPS - 1, whole vectors)
constexpr int kMaxTrips = 33;        // Hs / 2 + 1 <= 65 tap pairs, two per trip
// staged samples per rail: the halo, the tile, and what the padded last trip reads behind it (zero taps): the last lane reads the
// words up to 2 (kThreads - 1) + 2 kMaxTrips + 1
constexpr int kStage = 2 * (2 * (kThreads - 1) + 2 * kMaxTrips + 2);
static_assert(kStage >= kHist + kTile, "the stage holds the largest halo and the tile");
static_assert(GAL_FIR_MAX_TAPS - 1 <= kHist && kHist % 4 == 0, "the history holds the longest halo in whole vectors");

// in, out: n complex samples each, 16-byte aligned, not overlapping; taps: n_trips uint4 (see above); hs = the halo, a multiple of 4
// in 0 .. 128; hist_in / hist_out: kHist complex samples each, the handle's two history buffers
__global__ __launch_bounds__(kThreads) void k_iq_fir(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint64_t n,
                                                     const uint4 *__restrict__ taps, int n_trips, int hs,
                                                     const uint32_t *__restrict__ hist_in, uint32_t *__restrict__ hist_out,
                                                     unsigned long long *sat)
{
    __shared__ __attribute__((aligned(16))) uint32_t sI[kStage / 2], sQ[kStage / 2];  // two samples of one rail per word
    const int t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kTile;  // the tile's first sample, counted from the call's first

    // stage the samples [base - hs, base + kTile) of the call, four at a time
    const int nv = (hs + kTile) / 4;
    for (int v = t; v < nv; v += kThreads) {
        v4i a = {0, 0, 0, 0};
        if (4 * v < hs && base == 0) {  // in front of the call: the history ends where the call begins
            a = ((const v4i *)hist_in)[(kHist - hs) / 4 + v];
        } else {
            const uint64_t s = base + (uint64_t)(4 * v) - (uint64_t)hs;  // (not negative: base >= kTile > hs, or 4 v >= hs)
            if (s + 4 <= n) {
                a = ((const v4i *)in)[s >> 2];
            } else {
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    if (s + m < n) a[m] = (int)in[s + m];
            }
        }
        const uint32_t a0 = (uint32_t)a[0], a1 = (uint32_t)a[1], a2 = (uint32_t)a[2], a3 = (uint32_t)a[3];
        ((uint2 *)sI)[v] = make_uint2((a0 & 0xffffu) | (a1 << 16), (a2 & 0xffffu) | (a3 << 16));
        ((uint2 *)sQ)[v] = make_uint2((a0 >> 16) | (a1 & 0xffff0000u), (a2 >> 16) | (a3 & 0xffff0000u));
    }
    // the words behind the staged samples that the padded last trip reads: zeroed, so that nothing undefined enters the sums
    for (int w = nv * 2 + t; w < kStage / 2; w += kThreads) sI[w] = sQ[w] = 0;
    __syncthreads();

    // the next history: the last kHist samples of (history, input)
    if (blockIdx.x == 0 && t < kHist) {
        const uint64_t p = n + (uint64_t)t;  // sample p - kHist of the call
        hist_out[t] = p >= (uint64_t)kHist ? in[p - kHist] : hist_in[p];
    }

    uint32_t cnt = 0;
    if (base + 4 * (uint64_t)t < n) {
        int aI[4] = {8192, 8192, 8192, 8192}, aQ[4] = {8192, 8192, 8192, 8192};
        const uint2 *wI = (const uint2 *)sI + t, *wQ = (const uint2 *)sQ + t;  // the lane's words W[0], W[1]
        uint2 cI = wI[0], cQ = wQ[0];
        for (int i = 0; i < n_trips; ++i) {
            const uint4 g = taps[i];  // uniform: GE[2i], GO[2i], GE[2i + 1], GO[2i + 1]
            const uint2 nI = wI[i + 1], nQ = wQ[i + 1];
            aI[0] = dot2(cI.x, g.x, aI[0]);
            aI[1] = dot2(cI.x, g.y, aI[1]);
            aI[2] = dot2(cI.y, g.x, aI[2]);
            aI[3] = dot2(cI.y, g.y, aI[3]);
            aQ[0] = dot2(cQ.x, g.x, aQ[0]);
            aQ[1] = dot2(cQ.x, g.y, aQ[1]);
            aQ[2] = dot2(cQ.y, g.x, aQ[2]);
            aQ[3] = dot2(cQ.y, g.y, aQ[3]);
            aI[0] = dot2(cI.y, g.z, aI[0]);
            aI[1] = dot2(cI.y, g.w, aI[1]);
            aI[2] = dot2(nI.x, g.z, aI[2]);
            aI[3] = dot2(nI.x, g.w, aI[3]);
            aQ[0] = dot2(cQ.y, g.z, aQ[0]);
            aQ[1] = dot2(cQ.y, g.w, aQ[1]);
            aQ[2] = dot2(nQ.x, g.z, aQ[2]);
            aQ[3] = dot2(nQ.x, g.w, aQ[3]);
            cI = nI;
            cQ = nQ;
        }
        const uint64_t o = base + 4 * (uint64_t)t;
        if (o + 4 <= n) {
            v4i y;
#pragma unroll
            for (int m = 0; m < 4; ++m) y[m] = (int)(q14(aI[m], cnt) | (q14(aQ[m], cnt) << 16));
            ((v4i *)out)[o >> 2] = y;
        } else {  // the call's last samples, which do not fill a vector: 4-byte stores, and nothing behind them is stored or counted
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (o + m < n) out[o + m] = q14(aI[m], cnt) | (q14(aQ[m], cnt) << 16);
        }
    }
    add_block_count<kThreads>(cnt, sat);
}

}  // namespace

// The device table of n_taps (1 .. GAL_FIR_MAX_TAPS) taps for k_iq_fir: *n_trips uint4 of tap pairs, written to `table` (room for
// GAL_FIR_TABLE_WORDS = 4 x 33 words); *hs = the halo.  Host only.
extern "C" void galk_fir_table(const int16_t *h, int n_taps, uint32_t *table, int *n_trips, int *hs)
{
    const int Hs = (n_taps - 1 + 3) & ~3, trips = (Hs / 2 + 1 + 1) / 2;
    // G[m] = h[Hs - m] for 0 <= Hs - m < n_taps, else 0 (m may run past Hs and below 0 in the padded pairs)
    auto G = [&](int m) -> uint32_t {
        const int k = Hs - m;
        return (m >= 0 && k >= 0 && k < n_taps) ? (uint32_t)(uint16_t)h[k] : 0u;
    };
    for (int i = 0; i < trips; ++i)
        for (int q = 0; q < 2; ++q) {
            const int j = 2 * i + q;
            table[4 * i + 2 * q] = G(2 * j) | (G(2 * j + 1) << 16);      // GE[j]
            table[4 * i + 2 * q + 1] = G(2 * j - 1) | (G(2 * j) << 16);  // GO[j]
        }
    *n_trips = trips;
    *hs = Hs;
}

// n >= 1 complex samples; arguments are checked by the caller (iq_api.cpp: gal_synth_iq_fir), which also keeps n below 2^41
extern "C" hipError_t galk_launch_iq_fir(const int16_t *in, int16_t *out, uint64_t n, const uint32_t *table_dev, int n_trips, int hs,
                                         const uint32_t *hist_in, uint32_t *hist_out, unsigned long long *sat, hipStream_t st)
{
    const uint64_t blocks = (n + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_iq_fir, dim3((unsigned)blocks), dim3(kThreads), 0, st, (const uint32_t *)in, (uint32_t *)out, n, (const uint4 *)table_dev,
                       n_trips, hs, hist_in, hist_out, sat);
    return hipGetLastError();
}
