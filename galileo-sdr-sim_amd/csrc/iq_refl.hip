// iq_refl.hip -- geometric reflectors (include/galsynth.h: gal_synth_iq_refl, gal_synth_run_refl): the echo pass of
// iq_echo.hip with a delay of D + F / 4096 samples.  With N = samples per epoch, n the complex sample, e = n div N, m = n mod N,
// g[e][k] the Q7 gain of part k and (A, D, ph0, dph, F) the row of echo r in epoch e, p = the echo's part:
//
//   a  = x_p[n - D],  b = x_p[n - D - 1]             (n - D < 0: the part's history line, the 1024 samples in front of the call)
//   u  = a + ((F (b - a) + 2048) >> 12)              (per rail, arithmetic shift; F = 0: u = a, and b is not read)
//   i  = (ph0 + m dph mod 2^32) >> 22;  c = C[i], s = C[(i - 256) & 1023]          (C = gal_tables_cos1024(), Q12)
//   rI = (uI c - uQ s + 2048) >> 12;  rQ = (uI s + uQ c + 2048) >> 12              (arithmetic shifts)
//   w  = sum over k of g[e][k] x_k[n] + sum over r of A_r r_r                      (per rail)
//   y  = clamp16((w + 64) >> 7)
//
// A value the clamp changes counts once as saturated.  Integer arithmetic only (tests/refl_model.py states it in numpy); F = 0 in every
// row is k_iq_echo bit for bit, n_echo = 0 k_iq_wsum.  |b - a| <= 65535 and F <= 4095, so |F (b - a)| < 2^28; u lies between a and b
// inclusive (the rounded term has the sign of b - a and at most its size), so |u| <= 32768 as for k_iq_echo and the bounds of mac_rot
// (iq_dev.h) and of the int32 accumulator (sum_k g + 2 sum_r A <= 65535: kWide false) carry over unchanged.
//
// Shape: that of k_iq_echo -- blockIdx.y strides over the epochs and blockIdx.x over the 16-byte vectors that lie wholly inside the
// epoch, so the gain row, the echo rows and the part pointers are uniform for the block (scalar loads); 16-byte loads and stores; head
// and tail samples of unaligned epochs by the epoch's first block; the cosine table (2 KB) in LDS.
//
// The delayed reads.  Let D' = D + (F > 0 ? 1 : 0), the oldest sample an output sample needs; the host has checked D' <= 1024.  A lane's
// vector i (samples 4 i .. 4 i + 3) needs the samples 4 i - D' .. 4 i - D + 3: four of them where F = 0, five where F > 0.  With
// q = i - ceil(D' / 4) and sh = (-D') mod 4 they are the elements sh .. sh + 3 (+ 1) of the eight samples of the ALIGNED vectors q and
// q + 1; sh + 4 <= 7, so two vectors always suffice, and q + 1 is needed unless F = 0 and sh = 0.  sh, F > 0 and hence the loads and the
// element picks are uniform for the block.  In the echo kernel's terms (its q is floor((4 i - D) / 4)) the window is its vectors q and
// q + 1, or q - 1 and q where D is a multiple of 4 and F > 0.  Since 1 <= ceil(D' / 4) <= 256 whenever q + 1 is read, q + 1 <= i: never
// behind the lane's own vector; and q >= i - 256 >= -256: an aligned vector lies wholly in the call (q >= 0, and then q <= i < the
// call's vectors) or wholly in the 256 vectors of the history line (the call begins on a vector).  So a delayed read touches only
// addresses that the undelayed read of the same part by some lane of the call, or the history line, touches too.  The head and tail
// lanes read the single samples n - D and n - D - 1 >= -1024 in the same way.
#include <type_traits>

#include "../../include/galsynth.h"

#define GAL_INTERF_DEVICE_TABLE
#include "iq_dev.h"

extern "C" hipError_t galk_launch_echo_hist(const int16_t *const *parts_dev, const int16_t *const *hist_in_dev, int16_t *const *hist_out_dev,
                                            int n_parts, uint64_t n, hipStream_t st);

namespace {

constexpr int kMaxBlocks = 2048;  // as k_iq_echo
constexpr int kHist = GAL_ECHO_MAX_DELAY;
constexpr int kHistVec = GAL_ECHO_MAX_DELAY / 4;

// one echo of one epoch as the kernel reads it (gal_iq_refl_t, 16 bytes: one scalar load)
struct ReflRow {
    uint32_t gain_delay;  // gain_q7 | delay << 16
    uint32_t ph0;
    int32_t dph;
    uint32_t frac;  // frac_q12 | reserved << 16; reserved = 0 (checked on the host)
};
static_assert(sizeof(ReflRow) == sizeof(gal_iq_refl_t), "the kernel reads gal_iq_refl_t rows");

// u = a + ((F (b - a) + 2048) >> 12) per rail of the complex samples a (at n - D) and b (one sample older), I in the low halves
__device__ __forceinline__ void lerp(int a, int b, int F, int &uI, int &uQ)
{
    const int aI = (int16_t)a, aQ = a >> 16, bI = (int16_t)b, bQ = b >> 16;
    uI = aI + ((F * (bI - aI) + 2048) >> 12);
    uQ = aQ + ((F * (bQ - aQ) + 2048) >> 12);
}

// the arguments are those of k_iq_echo (iq_echo.hip), the rows gal_iq_refl_t
template <bool kWide>
__global__ __launch_bounds__(kThreads) void k_iq_refl(const int16_t *const *__restrict__ parts, const int16_t *const *__restrict__ hist,
                                                      const int *__restrict__ gain, const ReflRow *__restrict__ rows,
                                                      const int *__restrict__ part_of, int n_parts, int n_echo, int n_epochs, uint32_t N,
                                                      int16_t *__restrict__ out, unsigned long long *sat)
{
    typedef std::conditional_t<kWide, long long, int> acc_t;
    const int16_t *cosl = load_cos_table();
    uint32_t cnt = 0;
    for (int e = blockIdx.y; e < n_epochs; e += gridDim.y) {
        const int *__restrict__ g = gain + (size_t)e * n_parts;
        const ReflRow *__restrict__ row = rows + (size_t)e * n_echo;
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
                const ReflRow er = row[r];
                const int A = (int)(er.gain_delay & 0xffffu);
                if (A == 0) continue;  // (uniform) nothing to add
                const int F = (int)(er.frac & 0xffffu);
                const uint32_t Dp = (er.gain_delay >> 16) + (F ? 1u : 0u);  // D' <= 1024
                const int16_t *xp = parts[part_of[r]], *hp = hist[part_of[r]];
                // samples 4 i - D' .. 4 i - D' + 4 = elements sh .. sh + 4 of the aligned vectors q, q + 1
                const uint32_t sh = (0u - Dp) & 3u;
                const int64_t q = (int64_t)i - (int64_t)((Dp + 3) >> 2);
                const v4i lo = q >= 0 ? as_global<v4i>(xp)[q] : as_global<v4i>(hp)[q + kHistVec];
                v4i hi = lo;
                if (sh | (uint32_t)F)  // (uniform; then D' >= 1 and q + 1 <= i: never behind the lane's own vector)
                    hi = q + 1 >= 0 ? as_global<v4i>(xp)[q + 1] : as_global<v4i>(hp)[q + 1 + kHistVec];
                int t[5];  // t[j] = sample 4 i - D' + j
                if (sh == 0) {
                    t[0] = lo[0], t[1] = lo[1], t[2] = lo[2], t[3] = lo[3], t[4] = hi[0];
                } else if (sh == 1) {
                    t[0] = lo[1], t[1] = lo[2], t[2] = lo[3], t[3] = hi[0], t[4] = hi[1];
                } else if (sh == 2) {
                    t[0] = lo[2], t[1] = lo[3], t[2] = hi[0], t[3] = hi[1], t[4] = hi[2];
                } else {
                    t[0] = lo[3], t[1] = hi[0], t[2] = hi[1], t[3] = hi[2], t[4] = hi[3];
                }
                uint32_t ph = er.ph0 + m0 * (uint32_t)er.dph;
                if (F) {  // (uniform) sample m of the vector: a = t[m + 1], b = t[m]
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        int uI, uQ;
                        lerp(t[m + 1], t[m], F, uI, uQ);
                        mac_rot(w[2 * m], w[2 * m + 1], uI, uQ, ph, A, cosl);
                        ph += (uint32_t)er.dph;
                    }
                } else {
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        mac_rot(w[2 * m], w[2 * m + 1], (int)(int16_t)t[m], t[m] >> 16, ph, A, cosl);
                        ph += (uint32_t)er.dph;
                    }
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
                    const ReflRow er = row[r];
                    const int A = (int)(er.gain_delay & 0xffffu);
                    if (A == 0) continue;
                    const int F = (int)(er.frac & 0xffffu);
                    const int16_t *xp = parts[part_of[r]], *hp = hist[part_of[r]];
                    const int64_t j = (int64_t)n - (int64_t)(er.gain_delay >> 16);
                    const int ua = j >= 0 ? as_global<int>(xp)[j] : as_global<int>(hp)[j + kHist];
                    int ub = ua;
                    if (F) ub = j >= 1 ? as_global<int>(xp)[j - 1] : as_global<int>(hp)[j - 1 + kHist];  // (j - 1 >= -D' >= -1024)
                    int uI, uQ;
                    lerp(ua, ub, F, uI, uQ);
                    mac_rot(wI, wQ, uI, uQ, er.ph0 + (uint32_t)(n - a) * (uint32_t)er.dph, A, cosl);
                }
                ((uint32_t *)out)[n] = q7(wI, cnt) | (q7(wQ, cnt) << 16);
            }
        }
    }
    add_block_count<kThreads>(cnt, sat);
}

}  // namespace

// The arguments are those of galk_launch_iq_echo (iq_echo.hip), rows_dev holding gal_iq_refl_t; the history lines are rolled by the
// same k_echo_hist.  Arguments are checked by the caller (iq_api.cpp: gal_synth_iq_refl).
extern "C" hipError_t galk_launch_iq_refl(const int16_t *const *parts_dev, const int16_t *const *hist_in_dev, int16_t *const *hist_out_dev,
                                          const int *gain_dev, const void *rows_dev, const int *part_of_dev, int n_parts, int n_echo,
                                          int n_epochs, int samples_per_epoch, int wide, int16_t *out, unsigned long long *sat, hipStream_t st)
{
    const unsigned by = (unsigned)(n_epochs < kMaxBlocks ? n_epochs : kMaxBlocks);
    const unsigned need = (unsigned)((samples_per_epoch / 4 + kThreads - 1) / kThreads), cap = (unsigned)kMaxBlocks / by;
    const unsigned bx = need < 1 ? 1u : need > cap ? (cap < 1 ? 1u : cap) : need;
    if (wide)
        hipLaunchKernelGGL(k_iq_refl<true>, dim3(bx, by), dim3(kThreads), 0, st, parts_dev, hist_in_dev, gain_dev, (const ReflRow *)rows_dev,
                           part_of_dev, n_parts, n_echo, n_epochs, (uint32_t)samples_per_epoch, out, sat);
    else
        hipLaunchKernelGGL(k_iq_refl<false>, dim3(bx, by), dim3(kThreads), 0, st, parts_dev, hist_in_dev, gain_dev, (const ReflRow *)rows_dev,
                           part_of_dev, n_parts, n_echo, n_epochs, (uint32_t)samples_per_epoch, out, sat);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    return galk_launch_echo_hist(parts_dev, hist_in_dev, hist_out_dev, n_parts, (uint64_t)n_epochs * (uint64_t)samples_per_epoch, st);
}
