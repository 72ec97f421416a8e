// iq_corr.hip -- the correlator bank of include/galsynth.h (gal_synth_correlate): despread a buffer of output IQ, in any of the three
// formats, with the replica of one satellite.  Per request, for every code period m < max_periods, Doppler bin d and delay k:
//
//   S_B(m, d, k) = sum over the samples n of period m of (I + iQ)(n) conj(w_d(n)) b[h_k(n)],   S_C with c[.]
//
// with P(n) = code_ph0 + n code_dph, m = (P >> 32) / 8184, h = (P >> 32) % 8184, h_k = (h - delay_k) mod 8184, w_d(n) = the 512-entry
// carrier table at (carr_ph0 + n (carr_dph + dopp0 + d dopp_step)) >> 23.  Integers only: the sums are a fixed function of the inputs
// (tests/corr_model.py states it in numpy).
//
// Shape: one launch per request, one block per (tile of kTile samples, Doppler bin).
//   1. The block wipes the carrier off its tile ONCE: per sample (Re, Im) of x conj(w) as two int32, the prompt half chip h and the
//      period m, 16 bytes in LDS.  |x conj(w)| <= 2 x 32768 x 250 per part.
//   2. The PRN's two replicas sit bit-packed in LDS (2 bits per half chip: b < 0, c < 0; 2 KB).
//   3. A lane takes one delay (256 delays per trip of the block).  It walks the tile: the sample is one broadcast 16-byte LDS read,
//      its own half chip is h - delay (one conditional add for the wrap), the two replica bits one LDS word; the four rails add or
//      subtract (x ^ s) - s.  Where a request has fewer than 129 delays the lanes split into 256 / KD segments of the tile per
//      delay (KD = the power of two >= n_delay) and the segments are summed through LDS behind the walk.
//   4. int32 accumulators hold at most kSub = 128 samples: 128 x 2 x 32768 x 250 = 2 097 152 000 < 2^31.  They are added into int64
//      registers, and those into `out` with 64-bit atomics (integer addition commutes: the result does not depend on the order).
//   5. code_dph <= 2^32 (one half chip per sample) keeps a tile of 2048 samples inside 2048 half chips < one period: a tile sees at
//      most ONE period boundary, at a block-uniform sample jb; every lane keeps two sets of sums, the period in front of jb and the
//      one behind it, and walks [.., jb) and [jb, ..) separately -- exact, with uniform control flow.
#include "iq_dev.h"

namespace {

constexpr int kTile = 2048;  // samples per block: 32 KB of LDS
constexpr int kSub = 128;    // samples per int32 accumulation (see 4. above)
constexpr int kHalfChips = 8184;

struct CorrArgs {
    uint64_t ph0, dph;    // code phase at sample 0 and per sample: half chips x 2^32
    uint64_t n_eff;       // samples to look at: min(n_samples, the first sample of period max_periods)
    uint32_t cph0;        // carrier phase at sample 0
    uint32_t cstep0;      // carr_dph + dopp0 (mod 2^32)
    uint32_t dopp_step;
    int delay0, delay_step, n_delay, n_dopp, max_periods;
    int kd;               // lanes per segment: min(256, power of two >= n_delay)
};

// the samples [s, e) of the tile against the replica delayed by dk (0 .. 8183), added into acc
__device__ __forceinline__ void walk(const int4 *tile, const uint32_t *code, int s, int e, int dk, long long (&acc)[4])
{
    for (int c0 = s; c0 < e; c0 += kSub) {
        const int c1 = min(c0 + kSub, e);
        int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        for (int j = c0; j < c1; ++j) {
            const int4 v = tile[j];
            int t = v.z - dk;
            t += t < 0 ? kHalfChips : 0;
            const uint32_t w = code[t >> 4] >> (2 * (t & 15));
            const int sb = -(int)(w & 1u), sc = -(int)((w >> 1) & 1u);
            a0 += (v.x ^ sb) - sb;
            a1 += (v.y ^ sb) - sb;
            a2 += (v.x ^ sc) - sc;
            a3 += (v.y ^ sc) - sc;
        }
        acc[0] += a0;
        acc[1] += a1;
        acc[2] += a2;
        acc[3] += a3;
    }
}

// lut: [512] cos | sin << 16; code: [512] words of the request's PRN, 2 bits per half chip (b < 0, c < 0)
template <int FMT>
__global__ __launch_bounds__(kThreads) void k_corr(const void *__restrict__ buf, const CorrArgs a, const uint32_t *__restrict__ lut,
                                                   const uint32_t *__restrict__ code_g, unsigned long long *__restrict__ out)
{
    __shared__ int4 tile[kTile];
    __shared__ uint32_t code[512];
    __shared__ uint32_t car[512];
    __shared__ int jb_s;

    const int tid = threadIdx.x, d = blockIdx.y;
    const uint64_t n0 = (uint64_t)blockIdx.x * kTile;
    if (n0 >= a.n_eff) return;
    const int cnt = (int)min((uint64_t)kTile, a.n_eff - n0);
    for (int k = tid; k < 512; k += kThreads) {
        code[k] = code_g[k];
        car[k] = lut[k];
    }
    if (tid == 0) jb_s = cnt;
    __syncthreads();

    // 1. carrier wipe-off, half chip and period of every sample of the tile
    const uint32_t cstep = a.cstep0 + (uint32_t)d * a.dopp_step;
    const uint32_t m_first = (uint32_t)((a.ph0 + n0 * a.dph) >> 32) / (uint32_t)kHalfChips;
    int jb = cnt;
    for (int j = tid; j < cnt; j += kThreads) {
        const uint64_t n = n0 + j;
        int I, Q;
        load_iq<FMT>(buf, n, I, Q);
        const uint32_t w = car[(a.cph0 + (uint32_t)n * cstep) >> 23];
        const int c = ((int)w << 16) >> 16, s = (int)w >> 16;
        const uint32_t hi = (uint32_t)((a.ph0 + n * a.dph) >> 32);
        const uint32_t m = hi / (uint32_t)kHalfChips;
        tile[j] = make_int4(I * c + Q * s, Q * c - I * s, (int)(hi - m * (uint32_t)kHalfChips), (int)m);
        if (m != m_first) jb = min(jb, j);
    }
    if (jb < cnt) atomicMin(&jb_s, jb);
    __syncthreads();
    jb = jb_s;  // the first sample of the tile's second period (cnt: there is none)
    if ((int)m_first >= a.max_periods) return;
    const int end = (int)m_first + 1 < a.max_periods ? cnt : jb;  // (n_eff already ends the last tile there)

    // 3. one delay per lane, KD delays x (256 / KD) segments of the tile per trip
    const int kd = a.kd, nseg = kThreads / kd, seg = tid / kd, seg_len = kTile / nseg;
    const int s0 = seg * seg_len, s1 = min(s0 + seg_len, end);
    const size_t row = (size_t)a.n_dopp * a.n_delay * 4;  // int64 per period
    for (int kbase = 0; kbase < a.n_delay; kbase += kd) {
        const int k = kbase + (tid & (kd - 1));
        long long accA[4] = {0, 0, 0, 0}, accB[4] = {0, 0, 0, 0};
        if (k < a.n_delay) {
            long long dl = ((long long)a.delay0 + (long long)k * a.delay_step) % kHalfChips;
            const int dk = (int)(dl < 0 ? dl + kHalfChips : dl);
            walk(tile, code, s0, min(s1, jb), dk, accA);
            walk(tile, code, max(s0, jb), s1, dk, accB);
        }
        if (nseg > 1) {  // (then n_delay <= kd: this is the only trip, and the tile is free)
            __syncthreads();
            long long *red = (long long *)tile;  // [256][8] = 16 KB
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                red[tid * 8 + r] = accA[r];
                red[tid * 8 + 4 + r] = accB[r];
            }
            __syncthreads();
            if (tid >= kd) continue;
            for (int g = 1; g < nseg; ++g) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    accA[r] += red[(g * kd + tid) * 8 + r];
                    accB[r] += red[(g * kd + tid) * 8 + 4 + r];
                }
            }
        }
        if (k < a.n_delay) {
            unsigned long long *o = out + (size_t)m_first * row + ((size_t)d * a.n_delay + k) * 4;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (accA[r]) atomicAdd(o + r, (unsigned long long)accA[r]);
            if (jb < end) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (accB[r]) atomicAdd(o + row + r, (unsigned long long)accB[r]);
            }
        }
    }
}

}  // namespace

// One request.  Arguments are checked by the caller (iq_api.cpp: gal_synth_correlate): code_dph <= 2^32, 1 <= n_delay <= 8184,
// 1 <= n_dopp <= 64, 1 <= max_periods <= 1024, `out` zeroed and large enough, n_eff <= n_samples of the buffer.
extern "C" hipError_t galk_launch_corr(int format, const void *buf, uint64_t n_eff, uint64_t code_ph0, uint64_t code_dph, uint32_t carr_ph0,
                                       uint32_t carr_step0, uint32_t dopp_step, int delay0, int delay_step, int n_delay, int n_dopp,
                                       int max_periods, const uint32_t *lut_dev, const uint32_t *code_dev, long long *out, hipStream_t st)
{
    if (n_eff == 0) return hipSuccess;
    CorrArgs a;
    a.ph0 = code_ph0;
    a.dph = code_dph;
    a.n_eff = n_eff;
    a.cph0 = carr_ph0;
    a.cstep0 = carr_step0;
    a.dopp_step = dopp_step;
    a.delay0 = delay0;
    a.delay_step = delay_step;
    a.n_delay = n_delay;
    a.n_dopp = n_dopp;
    a.max_periods = max_periods;
    int kd = 1;
    while (kd < n_delay && kd < kThreads) kd <<= 1;
    a.kd = kd;
    const dim3 grid((unsigned)((n_eff + kTile - 1) / kTile), (unsigned)n_dopp), blk(kThreads);
    unsigned long long *o = (unsigned long long *)out;
    if (format == 0) hipLaunchKernelGGL(k_corr<0>, grid, blk, 0, st, buf, a, lut_dev, code_dev, o);
    else if (format == 1) hipLaunchKernelGGL(k_corr<1>, grid, blk, 0, st, buf, a, lut_dev, code_dev, o);
    else hipLaunchKernelGGL(k_corr<2>, grid, blk, 0, st, buf, a, lut_dev, code_dev, o);
    return hipGetLastError();
}
