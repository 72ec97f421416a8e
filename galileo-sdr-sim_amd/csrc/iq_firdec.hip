// iq_firdec.hip -- the decimating front-end FIR filter (include/galsynth.h: gal_synth_firdec_set, gal_synth_iq_firdec; DESIGN.md section
// 16).  x[n] = (I, Q)[n] the complex int16 samples of the WHOLE high-rate stream, x[n] = 0 for n < 0; h[0 .. T-1] real int16 taps in
// Q14, 1 <= T <= 512; the decimation 2 <= M <= 16.  Per rail, in integers:
//
//   a[m] = sum over k of h[k] x[M m - k]
//   y[m] = clamp16((a[m] + 8192) >> 14)            (arithmetic shift: round to nearest, ties up)
//
// y[m] is sample M m of what iq_fir.hip defines for the same taps; only the kept outputs are computed, clamped and counted.  The host
// admits only taps with sum |h[k]| <= 65535 (gal_synth_firdec_check): one int32 accumulator is exact for any int16 input in any order
// of accumulation.  tests/firdec_model.py states the function in numpy.
//
// A call takes the next n input samples of the stream, local index i = 0 .. n - 1; i0 = the local index of the first sample whose global
// index is a multiple of M (the host keeps the stream's position modulo M).  Output j of the call sits at local index i0 + M j.
//
// Shape: polyphase planes.  With k = M u + r the sum is, per branch r = 0 .. min(M, T) - 1 (branches r >= T have no taps and are skipped),
//   a_j = sum_r sum_u h[M u + r] p_r[j + U - u],    p_r[e] = x[i0 - r + M (e - U)],    U = (T - 1) / M  (the halo in plane elements)
// a same-rate FIR of the taps h_r[u] = h[M u + r] over the plane p_r: consecutive outputs read consecutive elements of one plane.  One
// block filters a tile of OB = (4096 / M) & ~3 consecutive outputs -- M OB <= kTileIn = 4096 INPUT samples, so the staged window and
// the LDS are the same for every M.  It stages the M (OB + 4 trips) input samples from local index
//   lo = i0 + M OB block - M U - (M - 1)
// on ONCE, with 16-byte loads on the vector grid of the call (vectors in front of the call come whole out of the history, which ends
// where the call begins; a vector the end of the call cuts is read with 4-byte accesses; behind the call and more than 512 samples in
// front of it everything is 0).  The staged sample d = i - lo goes to element e = d / M of plane r = M - 1 - d % M, I and Q to int16
// planes of their own: every element of every plane is written exactly once, and a 32-bit LDS word holds two consecutive elements of
// ONE plane of ONE rail, so that v_dot2_i32_i16 covers two taps per instruction.
//
// Per branch the walk is iq_fir.hip's.  With G_r[m] = h_r[U - m] (0 outside the taps), a_j += sum_m G_r[m] p_r[j + m]; a lane owns the
// outputs j0 .. j0 + 3 (j0 = 4 x its group) and walks the plane in aligned words W[q] = (p_r[j0 + 2q], p_r[j0 + 2q + 1]):
//   a[j0]     += sum_q W[q]     . GE[q],   GE[q] = (G[2q],     G[2q + 1])
//   a[j0 + 1] += sum_q W[q]     . GO[q],   GO[q] = (G[2q - 1], G[2q])
//   a[j0 + 2] += sum_q W[q + 1] . GE[q]
//   a[j0 + 3] += sum_q W[q + 1] . GO[q]
// no word is ever formed from two halves.  8-byte LDS reads, consecutive lanes 8 bytes apart: no bank conflict at any M (the planes
// exist for this: over the two rail planes of iq_fir.hip the lanes would be 4 M samples apart, 2 M words -- an 8-way conflict at M = 4,
// 16-way at 8, 32-way at 16).  The tap pairs are the host's table (GE[2i], GO[2i], GE[2i + 1], GO[2i + 1]) per branch and trip i,
// every branch padded with zeros to the same number of trips, read through a uniform address: scalar loads, the taps sit in SGPRs.
// 64-bit sample indices throughout.  Saturated values are counted per lane, per wave, per block, one atomic per block that saw one.
//
// The stream across calls: the handle keeps the last kHist = 512 input samples (zeros in front of the stream's start) in one of two
// device buffers; a call reads the one the call before it wrote and block 0 writes the other.  A call that keeps no output still
// runs one block for this.
#include "../../include/galsynth.h"
#include "iq_dev.h"

namespace {

constexpr int kTileIn = 4096;  // input samples per block at most: a block filters (kTileIn / M) & ~3 outputs, M times that many inputs
constexpr int kHist = 512;     // history the handle keeps: the last 512 input samples (>= GAL_FIRDEC_MAX_TAPS - 1, whole vectors)
// staged elements per rail, all planes: M (OB + 4 trips) <= kTileIn + M (U + 5) <= kTileIn + 511 + 5 x 16 (galk_firdec_table checks it)
constexpr int kStage = kTileIn + 640;
static_assert(GAL_FIRDEC_MAX_TAPS - 1 <= kHist && kHist % 4 == 0, "the history holds the longest halo in whole vectors");
static_assert(kTileIn + (GAL_FIRDEC_MAX_TAPS - 1) + 5 * GAL_FIRDEC_MAX_DECIM <= kStage && kStage % 8 == 0, "the stage holds every shape");

struct Shape {
    int M;         // the decimation
    uint32_t inv;  // 2^32 / M + 1: d / M = umulhi(d, inv) for every staged d (< 2^16)
    int OB;        // outputs per block, a multiple of 4
    int PL;        // int16 elements per plane, OB + 4 trips
    int U;         // the halo in plane elements, (T - 1) / M
    int nb;        // branches with taps, min(M, T)
    int trips;     // trips of the loop per branch
};

// in: n input samples, 16-byte aligned; out: n_out outputs, 16-byte aligned, not overlapping; i0 = the local index of output 0,
// 0 .. M - 1; taps: nb x trips uint4 (see above); hist_in / hist_out: kHist complex samples each, the handle's two history buffers
__global__ __launch_bounds__(kThreads) void k_iq_firdec(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint64_t n,
                                                        uint64_t n_out, int i0, Shape S, const uint4 *__restrict__ taps,
                                                        const uint32_t *__restrict__ hist_in, uint32_t *__restrict__ hist_out,
                                                        unsigned long long *sat)
{
    __shared__ __attribute__((aligned(16))) uint16_t sI[kStage], sQ[kStage];  // plane r: elements [r PL, (r + 1) PL)
    const int t = threadIdx.x;
    const uint64_t obase = (uint64_t)blockIdx.x * (uint64_t)S.OB;  // the tile's first output, counted from the call's first

    // stage the local samples [lo, lo + M PL), four at a time on the call's vector grid
    const int64_t lo = (int64_t)i0 + (int64_t)(obase * (uint64_t)S.M) - (int64_t)(S.M * S.U + S.M - 1);
    const int64_t lo4 = lo & ~(int64_t)3;
    const int skip = (int)(lo - lo4), total = S.M * S.PL;
    const int nv = (total + skip + 3) / 4;
    for (int v = t; v < nv; v += kThreads) {
        const int64_t s = lo4 + 4 * (int64_t)v;  // a multiple of 4, of either sign
        v4i a = {0, 0, 0, 0};
        if (s < 0) {
            if (s >= -(int64_t)kHist) a = ((const v4i *)hist_in)[(s + kHist) >> 2];  // (further in front: no tap reaches it)
        } else if ((uint64_t)s + 4 <= n) {
            a = ((const v4i *)in)[s >> 2];
        } else {
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if ((uint64_t)s + m < n) a[m] = (int)in[s + m];
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int d = 4 * v + m - skip;
            if (d >= 0 && d < total) {
                const int e = (int)__umulhi((uint32_t)d, S.inv), r = S.M - 1 - (d - e * S.M);
                sI[r * S.PL + e] = (uint16_t)((uint32_t)a[m] & 0xffffu);
                sQ[r * S.PL + e] = (uint16_t)((uint32_t)a[m] >> 16);
            }
        }
    }
    __syncthreads();

    // the next history: the last kHist samples of (history, input)
    if (blockIdx.x == 0)
        for (int k = t; k < kHist; k += kThreads) {
            const uint64_t p = n + (uint64_t)k;  // sample p - kHist of the call
            hist_out[k] = p >= (uint64_t)kHist ? in[p - kHist] : hist_in[p];
        }

    uint32_t cnt = 0;
    for (int g0 = 0; 4 * g0 < S.OB; g0 += kThreads) {
        const int g = g0 + t;  // the lane's group: the outputs obase + 4 g .. + 3
        const uint64_t o = obase + 4 * (uint64_t)g;
        if (4 * g < S.OB && o < n_out) {
            int aI[4] = {8192, 8192, 8192, 8192}, aQ[4] = {8192, 8192, 8192, 8192};
            for (int r = 0; r < S.nb; ++r) {
                const uint2 *wI = (const uint2 *)(sI + r * S.PL) + g, *wQ = (const uint2 *)(sQ + r * S.PL) + g;  // the lane's words W[0], W[1]
                const uint4 *tp = taps + r * S.trips;
                uint2 cI = wI[0], cQ = wQ[0];
                for (int i = 0; i < S.trips; ++i) {
                    const uint4 q = tp[i];  // uniform: GE[2i], GO[2i], GE[2i + 1], GO[2i + 1]
                    const uint2 nI = wI[i + 1], nQ = wQ[i + 1];
                    aI[0] = dot2(cI.x, q.x, aI[0]);
                    aI[1] = dot2(cI.x, q.y, aI[1]);
                    aI[2] = dot2(cI.y, q.x, aI[2]);
                    aI[3] = dot2(cI.y, q.y, aI[3]);
                    aQ[0] = dot2(cQ.x, q.x, aQ[0]);
                    aQ[1] = dot2(cQ.x, q.y, aQ[1]);
                    aQ[2] = dot2(cQ.y, q.x, aQ[2]);
                    aQ[3] = dot2(cQ.y, q.y, aQ[3]);
                    aI[0] = dot2(cI.y, q.z, aI[0]);
                    aI[1] = dot2(cI.y, q.w, aI[1]);
                    aI[2] = dot2(nI.x, q.z, aI[2]);
                    aI[3] = dot2(nI.x, q.w, aI[3]);
                    aQ[0] = dot2(cQ.y, q.z, aQ[0]);
                    aQ[1] = dot2(cQ.y, q.w, aQ[1]);
                    aQ[2] = dot2(nQ.x, q.z, aQ[2]);
                    aQ[3] = dot2(nQ.x, q.w, aQ[3]);
                    cI = nI;
                    cQ = nQ;
                }
            }
            if (o + 4 <= n_out) {
                v4i y;
#pragma unroll
                for (int m = 0; m < 4; ++m) y[m] = (int)(q14(aI[m], cnt) | (q14(aQ[m], cnt) << 16));
                ((v4i *)out)[o >> 2] = y;
            } else {  // the call's last outputs, which do not fill a vector: 4-byte stores, and nothing behind them is stored or counted
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    if (o + m < n_out) out[o + m] = q14(aI[m], cnt) | (q14(aQ[m], cnt) << 16);
            }
        }
    }
    add_block_count<kThreads>(cnt, sat);
}

Shape shape_of(int n_taps, int decim)
{
    Shape S;
    S.M = decim;
    S.inv = (uint32_t)((1ull << 32) / (uint64_t)decim + 1);
    S.OB = (kTileIn / decim) & ~3;
    S.U = (n_taps - 1) / decim;
    S.nb = n_taps < decim ? n_taps : decim;
    const int pairs = (S.U + 1) / 2 + 1;  // GE[q], GO[q] for q = 0 .. ceil(U / 2)
    S.trips = (pairs + 1) / 2;
    S.PL = S.OB + 4 * S.trips;
    return S;
}

}  // namespace

// The device table of n_taps (1 .. GAL_FIRDEC_MAX_TAPS) taps at the decimation decim (2 .. GAL_FIRDEC_MAX_DECIM) for k_iq_firdec:
// min(decim, n_taps) branches x *trips uint4 of tap pairs, written to `table` (room for GAL_FIRDEC_TABLE_WORDS = 640 words; the return
// value = the words written, 0 if the shape did not fit, which no admitted shape does).  Host only.
extern "C" int galk_firdec_table(const int16_t *h, int n_taps, int decim, uint32_t *table, int *trips)
{
    const Shape S = shape_of(n_taps, decim);
    if (S.M * S.PL > kStage || 4 * S.nb * S.trips > 640) return 0;
    for (int r = 0; r < S.nb; ++r) {
        // G[m] = h[M (U - m) + r] for 0 <= m <= U and a tap there, else 0 (m may run past U and below 0 in the padded pairs)
        auto G = [&](int m) -> uint32_t {
            const int k = S.M * (S.U - m) + r;
            return (m >= 0 && m <= S.U && k < n_taps) ? (uint32_t)(uint16_t)h[k] : 0u;
        };
        uint32_t *row = table + 4 * r * S.trips;
        for (int i = 0; i < S.trips; ++i)
            for (int p = 0; p < 2; ++p) {
                const int q = 2 * i + p;
                row[4 * i + 2 * p] = G(2 * q) | (G(2 * q + 1) << 16);      // GE[q]
                row[4 * i + 2 * p + 1] = G(2 * q - 1) | (G(2 * q) << 16);  // GO[q]
            }
    }
    *trips = S.trips;
    return 4 * S.nb * S.trips;
}

// The input samples one block filters at this decimation: (4096 / decim) & ~3 outputs.  Host only.
extern "C" int galk_firdec_tile_inputs(int decim) { return ((kTileIn / decim) & ~3) * decim; }

// n >= 1 input samples, n_out outputs from local index i0 on; arguments are checked by the caller (iq_api.cpp: gal_synth_iq_firdec),
// which also keeps n below 2^41
extern "C" hipError_t galk_launch_iq_firdec(const int16_t *in, int16_t *out, uint64_t n, uint64_t n_out, int i0, int n_taps, int decim,
                                            const uint32_t *table_dev, const uint32_t *hist_in, uint32_t *hist_out,
                                            unsigned long long *sat, hipStream_t st)
{
    const Shape S = shape_of(n_taps, decim);
    uint64_t blocks = (n_out + (uint64_t)S.OB - 1) / (uint64_t)S.OB;
    if (blocks == 0) blocks = 1;  // no output: the history still moves on
    hipLaunchKernelGGL(k_iq_firdec, dim3((unsigned)blocks), dim3(kThreads), 0, st, (const uint32_t *)in, (uint32_t *)out, n, n_out, i0, S,
                       (const uint4 *)table_dev, hist_in, hist_out, sat);
    return hipGetLastError();
}
