// iq_psd.hip -- the Welch power spectrum of include/galsynth.h (gal_synth_iq_psd): the sums over overlapping segments of |X[k]|^2,
// X the INTEGER radix-2 transform of the windowed segment, of a buffer of output IQ in any of the three formats.  Integers only: the
// sums are a fixed function of the inputs (tests/psd_model.py states it in numpy).
//
// Shape: one launch; a block of 256 lanes takes a run of slabs.  A slab is kSlabMin = 1024 points or one segment, whichever is more:
// G = max(1, 1024 / N) segments side by side, so that every lane has work at any N with ONE code path (a segment past the end of the
// block's run is loaded as zeros and adds nothing).
//   1. The block unfolds the N / 2 twiddles it needs, (C, S)[j 4096 / N], from the quarter wave into LDS, once.
//   2. Per slab: every point is read in its format, scaled to the int16 grid, windowed (the Hann window is the twiddle table's own
//      cosine) and stored at the bit-reversed place of its segment, as two int32.  Rows of 32 points are padded by one, so that the
//      stride-4 walks of the first stages spread over the banks.
//   3. The stages run two at a time: a lane takes the four points p, p + h, p + 2h, p + 3h, does the two butterflies of stage h and
//      the two of stage 2h in registers -- the same integers as two radix-2 stages, one LDS round trip.  An odd log2 N ends with one
//      radix-2 stage.  Products are int64 (v_mad_i64_i32), (x + 2^29) >> 30 is an arithmetic shift.
//   4. Every lane keeps the power sums of its points (point i of the slab is bin i mod N) in uint64 registers across the slabs and ends
//      with one 64-bit atomic add per point into `out`: integer addition commutes, the result does not depend on the order.
#define GAL_PSD_DEVICE_TABLE
#include "iq_dev.h"
#include "psd_table.inc"

namespace {

constexpr int kPsdMaxLog2 = 12, kPsdMaxN = 1 << kPsdMaxLog2;
constexpr int kSlabMin = 4 * kThreads;             // points of a slab at N <= 1024: four per lane
constexpr int kMaxPts = kPsdMaxN / kThreads;       // points per lane at N = 4096
constexpr int kMaxBlocks = 256;

struct PsdArgs {
    uint64_t n_seg;
    uint32_t hop;
    int log2_n, hann, gshift;
    uint32_t slabs, slabs_per_block;
};

__device__ __forceinline__ int pad(int i) { return i + (i >> 5); }

// C[j] of the whole 4096-entry table out of the quarter wave
__device__ __forceinline__ int cos4096(int j)
{
    j &= 4095;
    return j <= 1024 ? kPsdQuarterDev[j] : j <= 2048 ? -kPsdQuarterDev[2048 - j] : j <= 3072 ? -kPsdQuarterDev[j - 2048] : kPsdQuarterDev[4096 - j];
}

// (u, x) -> (u + t, u - t), t = x w rounded, w = (c, -s)
__device__ __forceinline__ void bfly(int2 &u, int2 &x, int2 cs)
{
    const long long wr = cs.x, wi = -(long long)cs.y;
    const int tr = (int)((x.x * wr - x.y * wi + (1ll << 29)) >> 30);
    const int ti = (int)((x.x * wi + x.y * wr + (1ll << 29)) >> 30);
    x = make_int2(u.x - tr, u.y - ti);
    u = make_int2(u.x + tr, u.y + ti);
}

template <int FMT>
__global__ __launch_bounds__(kThreads) void k_psd(const void *__restrict__ buf, const PsdArgs a, unsigned long long *__restrict__ out)
{
    __shared__ int2 x[kPsdMaxN + kPsdMaxN / 32];
    __shared__ int2 tw[kPsdMaxN / 2];

    const int tid = threadIdx.x, lg = a.log2_n, N = 1 << lg;
    const int M = max(N, kSlabMin), G = M >> lg;  // points and segments of a slab
    const int tstep = kPsdMaxN >> lg;             // table entries per twiddle of this size
    const int gs = 1 << a.gshift;

    for (int k = tid; k < N / 2; k += kThreads) tw[k] = make_int2(cos4096(k * tstep), cos4096(k * tstep - 1024));

    unsigned long long acc[kMaxPts];
#pragma unroll
    for (int r = 0; r < kMaxPts; ++r) acc[r] = 0;

    const uint32_t sl0 = blockIdx.x * a.slabs_per_block, sl1 = min(sl0 + a.slabs_per_block, a.slabs);
    for (uint32_t sl = sl0; sl < sl1; ++sl) {
        __syncthreads();  // the twiddles are there; the slab before this one has been read
        // 2. load, scale, window, bit-reverse
#pragma unroll
        for (int r = 0; r < kMaxPts; ++r) {
            const int i = tid + r * kThreads;
            if (i < M) {
                const int g = i >> lg, n = i & (N - 1);
                const uint64_t seg = (uint64_t)sl * G + g;
                int2 v = make_int2(0, 0);
                if (seg < a.n_seg) {
                    int I, Q;
                    load_iq<FMT>(buf, seg * a.hop + n, I, Q);
                    const int c = n < N / 2 ? tw[n].x : -tw[n - N / 2].x;
                    const int w = a.hann ? (int)(((1u << 30) - (unsigned)c) >> 16) : 32768;  // (2^31 at n = N / 2: unsigned)
                    v.x = (I * gs * w + (1 << 14)) >> 15;
                    v.y = (Q * gs * w + (1 << 14)) >> 15;
                }
                x[pad((g << lg) + (int)(__brev((unsigned)n) >> (32 - lg)))] = v;
            }
        }
        __syncthreads();
        // 3. two stages per round trip
        int lh = 0;
        for (; lh + 2 <= lg; lh += 2) {
            const int h = 1 << lh;
#pragma unroll
            for (int r = 0; r < kMaxPts / 4; ++r) {
                const int q = tid + r * kThreads;
                if (q < M / 4) {
                    const int m = q & (h - 1), p = ((q >> lh) << (lh + 2)) + m;
                    int2 &r0 = x[pad(p)], &r1 = x[pad(p + h)], &r2 = x[pad(p + 2 * h)], &r3 = x[pad(p + 3 * h)];
                    int2 y0 = r0, y1 = r1, y2 = r2, y3 = r3;
                    const int2 wa = tw[m << (lg - 1 - lh)];  // stage h: (p mod h) N / (2h)
                    bfly(y0, y1, wa);
                    bfly(y2, y3, wa);
                    bfly(y0, y2, tw[m << (lg - 2 - lh)]);        // stage 2h: (p mod 2h) N / (4h), p mod 2h = m
                    bfly(y1, y3, tw[(m + h) << (lg - 2 - lh)]);  //           ... and m + h for the pair that starts at p + h
                    r0 = y0, r1 = y1, r2 = y2, r3 = y3;
                }
            }
            __syncthreads();
        }
        if (lh < lg) {  // odd log2 N: the last stage on its own, h = N / 2
            const int h = 1 << lh;
#pragma unroll
            for (int r = 0; r < kMaxPts / 2; ++r) {
                const int q = tid + r * kThreads;
                if (q < M / 2) {
                    const int m = q & (h - 1), p = ((q >> lh) << (lh + 1)) + m;
                    int2 &r0 = x[pad(p)], &r1 = x[pad(p + h)];
                    int2 y0 = r0, y1 = r1;
                    bfly(y0, y1, tw[m]);
                    r0 = y0, r1 = y1;
                }
            }
            __syncthreads();
        }
        // 4. the power of this lane's points
#pragma unroll
        for (int r = 0; r < kMaxPts; ++r) {
            const int i = tid + r * kThreads;
            if (i < M) {
                const int2 v = x[pad(i)];
                acc[r] += (unsigned long long)((long long)v.x * v.x + (long long)v.y * v.y);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kMaxPts; ++r) {
        const int i = tid + r * kThreads;
        if (i < M && acc[r]) atomicAdd(out + (i & (N - 1)), acc[r]);
    }
}

}  // namespace

// The whole table on the host: [0, 4096) C, [4096, 8192) S (include/galsynth.h: gal_tables_psd)
extern "C" const int32_t *gal_tables_psd(void)
{
    static int32_t t[2 * 4096];
    static const bool once = [] {
        for (int k = 0; k < 4096; ++k)
            t[k] = k <= 1024 ? kPsdQuarter[k] : k <= 2048 ? -kPsdQuarter[2048 - k] : k <= 3072 ? -kPsdQuarter[k - 2048] : kPsdQuarter[4096 - k];
        for (int k = 0; k < 4096; ++k) t[4096 + k] = t[(k - 1024) & 4095];
        return true;
    }();
    (void)once;
    return t;
}

// Arguments are checked by the caller (iq_api.cpp: gal_synth_iq_psd): 3 <= log2_n <= 12, 1 <= hop <= N, n_seg >= 1 segments lie inside
// the buffer, n_seg N^2 <= 2^32, `out` = N zeroed uint64.
extern "C" hipError_t galk_launch_psd(int format, const void *buf, uint64_t n_seg, int log2_n, int hop, int window, unsigned long long *out,
                                      hipStream_t st)
{
    PsdArgs a;
    a.n_seg = n_seg;
    a.hop = (uint32_t)hop;
    a.log2_n = log2_n;
    a.hann = window;
    a.gshift = format == 0 ? 0 : format == 1 ? 8 : 14;
    const uint64_t per_slab = log2_n >= 10 ? 1 : (uint64_t)(kSlabMin >> log2_n);
    a.slabs = (uint32_t)((n_seg + per_slab - 1) / per_slab);
    a.slabs_per_block = (a.slabs + kMaxBlocks - 1) / kMaxBlocks;
    const dim3 grid((a.slabs + a.slabs_per_block - 1) / a.slabs_per_block), blk(kThreads);
    if (format == 0) hipLaunchKernelGGL(k_psd<0>, grid, blk, 0, st, buf, a, out);
    else if (format == 1) hipLaunchKernelGGL(k_psd<1>, grid, blk, 0, st, buf, a, out);
    else hipLaunchKernelGGL(k_psd<2>, grid, blk, 0, st, buf, a, out);
    return hipGetLastError();
}
