// iq_gain.hip -- per-satellite signal power (include/galsynth.h: gal_synth_iq_wsum, gal_synth_run_gains): the
// weighted sum of n_parts interleaved int16 streams of equal length, each the engine's output for one group of channel slots.  With
// N = samples per epoch, e(j) = (j / 2) / N and g[e][k] the Q7 gain of part k in epoch e (128 = unity):
//
//   w[j] = sum over k of g[e(j)][k] x_k[j]
//   y[j] = clamp16((w[j] + 64) >> 7)              (arithmetic shift: round to nearest, ties up)
//
// A value the clamp changes counts once as saturated.  Integer arithmetic only: a fixed function of (gains, parts) on any machine
// (tests/gain_model.py states it in numpy).  All gains 128 and one part give y = x.
//
// k_iq_wsum<kWide>: w in int32 (kWide false) where the host has checked that no epoch's gains sum to more than 65535 -- then
// |w| + 64 <= 65535 x 32768 + 64 < 2^31 for ANY int16 input --, else in int64 (16 parts at gain 32767 on full-scale input: 2^34).
// The same bits either way; the engine's own streams (|x| <= 500 per slot) never need the wide one below a gain sum of 4.29 M.
//
// Shape: a memory-bound stream of (n_parts + 1) x 4 bytes per complex sample, nothing reused -- as k_iq_pass (iq_pass.hip): 16-byte
// loads and stores, 64-bit indices, plain loads (the parts have just been written by the synthesis: non-temporal loads lost there,
// DESIGN.md section 10), the per-lane / per-wave / per-block saturation count of iq_dev.h.  Nothing is divided per sample: the grid
// is two-dimensional, blockIdx.y strides over the epochs and blockIdx.x over the 16-byte vectors that lie wholly inside the epoch, so
// the epoch's gain row and the part pointers are uniform for the block (read through uniform addresses: scalar loads).  Four parts'
// loads are issued before the first is used.  An epoch boundary need not be 16-byte aligned (gal_synth_create accepts any
// samples_per_epoch >= 4): the up to three complex samples in front of an epoch's first whole vector and the up to three behind its
// last one are taken one per lane by the epoch's first block, with 4-byte accesses.
#include <type_traits>

#include "../../include/galsynth.h"
#include "iq_dev.h"

namespace {

constexpr int kMaxBlocks = 2048;  // 8 blocks of 4 waves per CU, the rest by the grid-stride loops

// parts[k]: n_epochs * N complex samples, 16-byte aligned, none overlapping `out`; gain[e * n_parts + k]: 0 .. 32767
template <bool kWide>
__global__ __launch_bounds__(kThreads) void k_iq_wsum(const int16_t *const *__restrict__ parts, const int *__restrict__ gain, int n_parts,
                                                      int n_epochs, uint32_t N, int16_t *__restrict__ out, unsigned long long *sat)
{
    typedef std::conditional_t<kWide, long long, int> acc_t;
    uint32_t cnt = 0;
    for (int e = blockIdx.y; e < n_epochs; e += gridDim.y) {
        const int *__restrict__ g = gain + (size_t)e * n_parts;
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
                ((uint32_t *)out)[n] = q7(wI, cnt) | (q7(wQ, cnt) << 16);
            }
        }
    }
    add_block_count<kThreads>(cnt, sat);
}

}  // namespace

// parts_dev: n_parts device pointers (a device table); gain_dev: [n_epochs][n_parts] int32 on the device; wide != 0: the int64 instance.
// Arguments are checked by the caller (iq_api.cpp: gal_synth_iq_wsum).
extern "C" hipError_t galk_launch_iq_wsum(const int16_t *const *parts_dev, const int *gain_dev, int n_parts, int n_epochs, int samples_per_epoch,
                                          int wide, int16_t *out, unsigned long long *sat, hipStream_t st)
{
    const unsigned by = (unsigned)(n_epochs < kMaxBlocks ? n_epochs : kMaxBlocks);
    const unsigned need = (unsigned)((samples_per_epoch / 4 + kThreads - 1) / kThreads), cap = (unsigned)kMaxBlocks / by;
    const unsigned bx = need < 1 ? 1u : need > cap ? (cap < 1 ? 1u : cap) : need;
    if (wide)
        hipLaunchKernelGGL(k_iq_wsum<true>, dim3(bx, by), dim3(kThreads), 0, st, parts_dev, gain_dev, n_parts, n_epochs, (uint32_t)samples_per_epoch,
                           out, sat);
    else
        hipLaunchKernelGGL(k_iq_wsum<false>, dim3(bx, by), dim3(kThreads), 0, st, parts_dev, gain_dev, n_parts, n_epochs,
                           (uint32_t)samples_per_epoch, out, sat);
    return hipGetLastError();
}
