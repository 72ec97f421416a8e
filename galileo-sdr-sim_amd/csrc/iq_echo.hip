// iq_echo.hip -- per-satellite multipath (include/galsynth.h: gal_synth_iq_mpath, gal_synth_run_mpath): the weighted
// sum of iq_gain.hip plus n_echo delayed, phase-rotated copies of single parts.  With N = samples per epoch, n the complex sample,
// e = n div N, m = n mod N, g[e][k] the Q7 gain of part k and (A, D, ph0, dph) the row of echo r in epoch e, p = the echo's part:
//
//   u  = x_p[n - D]                                  (n - D < 0: the part's history line, the 1024 samples in front of the call)
//   i  = (ph0 + m dph mod 2^32) >> 22;  c = C[i], s = C[(i - 256) & 1023]          (C = gal_tables_cos1024(), Q12)
//   rI = (uI c - uQ s + 2048) >> 12;  rQ = (uI s + uQ c + 2048) >> 12              (arithmetic shifts)
//   w  = sum over k of g[e][k] x_k[n] + sum over r of A_r r_r                      (per rail)
//   y  = clamp16((w + 64) >> 7)
//
// A value the clamp changes counts once as saturated.  Integer arithmetic only (tests/mpath_model.py states it in numpy); n_echo = 0 is
// k_iq_wsum bit for bit.  |uI c - uQ s| <= 2 x 32768 x 4096 = 2^28, so |r| <= 65536 and the products before the shift fit an int32.
//
// k_iq_echo<kWide>: w in int32 (kWide false) where the host has checked sum_k g + 2 sum_r A <= 65535 in every epoch -- then
// |w| + 64 <= 65535 x 32768 + 64 < 2^31 for ANY int16 input --, else in int64.  The same bits either way.
//
// Shape: that of k_iq_wsum -- a two-dimensional grid, blockIdx.y strides over the epochs and blockIdx.x over the 16-byte vectors that
// lie wholly inside the epoch, so the gain row, the echo rows and the part pointers are uniform for the block (scalar loads); 16-byte
// loads and stores of the undelayed parts and the output; head and tail samples of unaligned epochs by the epoch's first block; the
// per-block saturation count.  The delayed samples n - D .. n - D + 3 of a lane's vector lie in the two ALIGNED vectors q and q + 1,
// q = floor((n - D) / 4): both are loaded with 16 bytes and the four wanted samples picked by D mod 4, which is uniform for the block
// (one load where D is a multiple of 4).  An aligned vector lies wholly in the call (q >= 0) or wholly in the history line (q < 0: the
// line is 256 vectors, the call begins on a vector), and q + 1 never lies behind the lane's own vector, so nothing is read that the
// undelayed load of some lane does not read too: the delayed reads hit lines that are in the cache already.  The cosine table (2 KB)
// is copied to LDS by every block.
#include <type_traits>

#include "../../include/galsynth.h"

#define GAL_INTERF_DEVICE_TABLE
#include "iq_dev.h"

namespace {

constexpr int kMaxBlocks = 2048;  // as k_iq_wsum: 8 blocks of 4 waves per CU, the rest by the grid-stride loops
constexpr int kHist = GAL_ECHO_MAX_DELAY;      // complex samples of one history line
constexpr int kHistVec = GAL_ECHO_MAX_DELAY / 4;

// one echo of one epoch as the kernel reads it (gal_iq_echo_t, 16 bytes: one scalar load)
struct EchoRow {
    uint32_t gain_delay;  // gain_q7 | delay << 16
    uint32_t ph0;
    int32_t dph;
    uint32_t reserved;
};
static_assert(sizeof(EchoRow) == sizeof(gal_iq_echo_t), "the kernel reads gal_iq_echo_t rows");

// the complex sample u (I in the low half) turned by the table phase `ph` and scaled by A, added to (wI, wQ)
template <class acc_t>
__device__ __forceinline__ void mac_echo(acc_t &wI, acc_t &wQ, int u, uint32_t ph, int A, const int16_t *cosl)
{
    mac_rot(wI, wQ, (int)(int16_t)u, u >> 16, ph, A, cosl);
}

// parts[k]: n_epochs * N complex samples, 16-byte aligned, none overlapping `out`; hist[k]: the kHist samples in front of part k (null
// for a part without a line: no echo reads it); gain[e * n_parts + k]: 0 .. 32767; rows[e * n_echo + r]; part_of[r]: 0 .. n_parts - 1
template <bool kWide>
__global__ __launch_bounds__(kThreads) void k_iq_echo(const int16_t *const *__restrict__ parts, const int16_t *const *__restrict__ hist,
                                                      const int *__restrict__ gain, const EchoRow *__restrict__ rows,
                                                      const int *__restrict__ part_of, int n_parts, int n_echo, int n_epochs, uint32_t N,
                                                      int16_t *__restrict__ out, unsigned long long *sat)
{
    typedef std::conditional_t<kWide, long long, int> acc_t;
    const int16_t *cosl = load_cos_table();
    uint32_t cnt = 0;
    for (int e = blockIdx.y; e < n_epochs; e += gridDim.y) {
        const int *__restrict__ g = gain + (size_t)e * n_parts;
        const EchoRow *__restrict__ row = rows + (size_t)e * n_echo;
        const uint64_t a = (uint64_t)e * N, b = a + N;    // the epoch's complex samples [a, b)
        const uint64_t v0 = (a + 3) >> 2, v1 = b >> 2;    // its whole vectors [v0, v1)
        const uint64_t stride = (uint64_t)gridDim.x * kThreads;
        for (uint64_t i = v0 + (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < v1; i += stride) {
            acc_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            int k = 0;
            for (; k + 4 <= n_parts; k += 4) {
                const v4i x0 = as_global<v4i>(parts[k])[i], x1 = as_global<v4i>(parts[k + 1])[i];
                const v4i x2 = as_global<v4i>(parts[k + 2])[i], x3 = as_global<v4i>(parts[k + 3])[i];
                mac8(w, x0, g[k]);
                mac8(w, x1, g[k + 1]);
                mac8(w, x2, g[k + 2]);
                mac8(w, x3, g[k + 3]);
            }
            for (; k < n_parts; ++k) mac8(w, as_global<v4i>(parts[k])[i], g[k]);
            const uint32_t m0 = (uint32_t)(4 * i - a);  // the vector's first sample inside the epoch
            for (int r = 0; r < n_echo; ++r) {
                const EchoRow er = row[r];
                const int A = (int)(er.gain_delay & 0xffffu);
                if (A == 0) continue;  // (uniform) nothing to add
                const uint32_t D = er.gain_delay >> 16;
                const int p = part_of[r];
                const int16_t *xp = parts[p], *hp = hist[p];
                // samples 4 i - D .. 4 i - D + 3 = elements sh .. sh + 3 of the aligned vectors q, q + 1
                const uint32_t sh = (0u - D) & 3u;
                const int64_t q = (int64_t)i - (int64_t)((D + 3) >> 2);
                const v4i lo = q >= 0 ? as_global<v4i>(xp)[q] : as_global<v4i>(hp)[q + kHistVec];
                v4i u = lo;
                if (sh) {  // (uniform; q + 1 <= i: never behind the lane's own vector)
                    const v4i hi = q + 1 >= 0 ? as_global<v4i>(xp)[q + 1] : as_global<v4i>(hp)[q + 1 + kHistVec];
                    if (sh == 1) {
                        u[0] = lo[1], u[1] = lo[2], u[2] = lo[3], u[3] = hi[0];
                    } else if (sh == 2) {
                        u[0] = lo[2], u[1] = lo[3], u[2] = hi[0], u[3] = hi[1];
                    } else {
                        u[0] = lo[3], u[1] = hi[0], u[2] = hi[1], u[3] = hi[2];
                    }
                }
                uint32_t ph = er.ph0 + m0 * (uint32_t)er.dph;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    mac_echo(w[2 * m], w[2 * m + 1], u[m], ph, A, cosl);
                    ph += (uint32_t)er.dph;
                }
            }
            v4i y;
#pragma unroll
            for (int m = 0; m < 4; ++m) y[m] = (int)(q7(w[2 * m], cnt) | (q7(w[2 * m + 1], cnt) << 16));
            ((v4i *)out)[i] = y;
        }
        if (blockIdx.x == 0) {  // head [a, he) and tail [ts, b): at most three complex samples each, one per lane
            const uint64_t he = 4 * v0 < b ? 4 * v0 : b, ts = 4 * v1 > he ? 4 * v1 : he;
            const uint32_t nh = (uint32_t)(he - a), nt = (uint32_t)(b - ts);
            if (threadIdx.x < nh + nt) {
                const uint64_t n = threadIdx.x < nh ? a + threadIdx.x : ts + (threadIdx.x - nh);
                acc_t wI = 0, wQ = 0;
                for (int k = 0; k < n_parts; ++k) {
                    const int x = as_global<int>(parts[k])[n];
                    wI += (acc_t)g[k] * (acc_t)(int16_t)x;
                    wQ += (acc_t)g[k] * (acc_t)(x >> 16);
                }
                for (int r = 0; r < n_echo; ++r) {
                    const EchoRow er = row[r];
                    const int A = (int)(er.gain_delay & 0xffffu);
                    if (A == 0) continue;
                    const int p = part_of[r];
                    const int64_t j = (int64_t)n - (int64_t)(er.gain_delay >> 16);
                    const int u = j >= 0 ? as_global<int>(parts[p])[j] : as_global<int>(hist[p])[j + kHist];
                    mac_echo(wI, wQ, u, er.ph0 + (uint32_t)(n - a) * (uint32_t)er.dph, A, cosl);
                }
                ((uint32_t *)out)[n] = q7(wI, cnt) | (q7(wQ, cnt) << 16);
            }
        }
    }
    add_block_count<kThreads>(cnt, sat);
}

// Block k: the new history line of part k = the last kHist samples of (old line, the call's n samples of the part).  hist_in[k] is
// read, hist_out[k] (another buffer) written; a part without a line (hist_out[k] null) is skipped.
__global__ __launch_bounds__(kThreads) void k_echo_hist(const int16_t *const *__restrict__ parts, const int16_t *const *__restrict__ hist_in,
                                                        int16_t *const *__restrict__ hist_out, uint64_t n)
{
    const int k = blockIdx.x;
    uint32_t *dst = (uint32_t *)hist_out[k];
    if (!dst) return;
    const int16_t *x = parts[k], *old = hist_in[k];
    for (int j = threadIdx.x; j < kHist; j += kThreads) {
        const int64_t s = (int64_t)n - kHist + j;  // index into the call; s < 0: element s + kHist = n + j of the old line
        dst[j] = (uint32_t)(s >= 0 ? as_global<int>(x)[s] : as_global<int>(old)[s + kHist]);
    }
}

}  // namespace

// the new history lines after a call of n complex samples (k_echo_hist): what galk_launch_iq_echo and galk_launch_iq_refl (iq_refl.hip) end with
extern "C" hipError_t galk_launch_echo_hist(const int16_t *const *parts_dev, const int16_t *const *hist_in_dev, int16_t *const *hist_out_dev,
                                            int n_parts, uint64_t n, hipStream_t st)
{
    hipLaunchKernelGGL(k_echo_hist, dim3((unsigned)n_parts), dim3(kThreads), 0, st, parts_dev, hist_in_dev, hist_out_dev, n);
    return hipGetLastError();
}

// tab_dev: the call's device table -- n_parts part pointers, hist_in and hist_out pointers at [GAL_ENGINE_MAX_CHAN] each (in that
// order), then the gains [n_epochs][n_parts] int32, the echo rows [n_epochs][n_echo] and part_of_echo [n_echo] at the given pointers.
// wide != 0: the int64 instance.  Arguments are checked by the caller (iq_api.cpp: gal_synth_iq_mpath).
extern "C" hipError_t galk_launch_iq_echo(const int16_t *const *parts_dev, const int16_t *const *hist_in_dev, int16_t *const *hist_out_dev,
                                          const int *gain_dev, const void *rows_dev, const int *part_of_dev, int n_parts, int n_echo,
                                          int n_epochs, int samples_per_epoch, int wide, int16_t *out, unsigned long long *sat, hipStream_t st)
{
    const unsigned by = (unsigned)(n_epochs < kMaxBlocks ? n_epochs : kMaxBlocks);
    const unsigned need = (unsigned)((samples_per_epoch / 4 + kThreads - 1) / kThreads), cap = (unsigned)kMaxBlocks / by;
    const unsigned bx = need < 1 ? 1u : need > cap ? (cap < 1 ? 1u : cap) : need;
    if (wide)
        hipLaunchKernelGGL(k_iq_echo<true>, dim3(bx, by), dim3(kThreads), 0, st, parts_dev, hist_in_dev, gain_dev, (const EchoRow *)rows_dev,
                           part_of_dev, n_parts, n_echo, n_epochs, (uint32_t)samples_per_epoch, out, sat);
    else
        hipLaunchKernelGGL(k_iq_echo<false>, dim3(bx, by), dim3(kThreads), 0, st, parts_dev, hist_in_dev, gain_dev, (const EchoRow *)rows_dev,
                           part_of_dev, n_parts, n_echo, n_epochs, (uint32_t)samples_per_epoch, out, sat);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    return galk_launch_echo_hist(parts_dev, hist_in_dev, hist_out_dev, n_parts, (uint64_t)n_epochs * (uint64_t)samples_per_epoch, st);
}
