// iq_array.hip -- the antenna array (include/galsynth.h: gal_synth_iq_array, gal_synth_run_array): K element streams
// out of P parts, each part turned and scaled by a complex Q12 weight per (epoch, element, part).  With N = samples per epoch, n the
// complex sample, e = n div N and (w_re, w_im) the weight of part k for element a in epoch e (4096 = the part at unity, unrotated):
//
//   AI = sum over k of (x_k.I w_re - x_k.Q w_im)        AQ = sum over k of (x_k.I w_im + x_k.Q w_re)
//   y_a.I = clamp16((AI + 2048) >> 12)                  y_a.Q = clamp16((AQ + 2048) >> 12)           (arithmetic shifts)
//
// A value the clamp changes counts once as saturated.  Integer arithmetic only (tests/array_model.py states it in numpy).  K = 1 and
// w = (32 g, 0) is k_iq_wsum bit for bit: floor((32 S + 2048) / 4096) = floor((S + 64) / 128).
//
// k_iq_array<K, kWide>: A in int32 (kWide false) where the host has checked sum_k (|w_re| + |w_im|) <= 65535 for every (epoch, element)
// -- then |A| + 2048 <= 32768 x 65535 + 2048 < 2^31 for ANY int16 input; the partial sums of v_dot2_i32_i16 (no clamp) are taken modulo
// 2^32 and the last one is the value --, else in int64.  The same bits either way.
//
// Shape: that of k_iq_wsum -- a two-dimensional grid, blockIdx.y strides over the epochs and blockIdx.x over the 16-byte vectors that
// lie wholly inside the epoch; head and tail samples of unaligned epochs by the epoch's first block; the per-block saturation count.
// Every part is read ONCE, with 16-byte loads, and feeds all K elements: K x 8 accumulators per lane live in registers (K is a
// template argument so that they are registers and not scratch: 64 VGPRs at K = 8, int32), K streams are written with 16-byte stores.
// The weights of an epoch are uniform for the block: the host packs them as two words per (epoch, part, element), (w_re, -w_im) and
// (w_im, w_re), the K elements of one part side by side, and the kernel reads them through uniform addresses (scalar loads, 8 K bytes per
// part) -- one v_dot2_i32_i16 per rail against the packed (I, Q) pair: 2 instructions per (element, part, sample).  No LDS but the
// count's.  Per complex sample 4 (P + K) bytes move, where K weighted sums move 4 K (P + 1).
#include <type_traits>

#include "../../include/galsynth.h"
#include "iq_dev.h"

namespace {

constexpr int kMaxBlocks = 2048;  // as k_iq_wsum: 8 blocks of 4 waves per CU, the rest by the grid-stride loops

// (A + 2048) >> 12 clamped to int16; `sat` counts the values the clamp changes
template <class acc_t>
__device__ __forceinline__ uint32_t q12(acc_t A, uint32_t &sat)
{
    const acc_t v = (A + 2048) >> 12;
    const acc_t y = v < -32768 ? (acc_t)-32768 : v > 32767 ? (acc_t)32767 : v;
    sat += (uint32_t)(y != v);
    return (uint32_t)y & 0xffffu;
}

// the complex sample x (I in the low half) times the weight (wa, wb) = ((w_re, -w_im), (w_im, w_re)), added to (AI, AQ)
__device__ __forceinline__ void mac_w(int &AI, int &AQ, uint32_t x, uint32_t wa, uint32_t wb)
{
    AI = dot2(x, wa, AI);
    AQ = dot2(x, wb, AQ);
}
__device__ __forceinline__ void mac_w(long long &AI, long long &AQ, uint32_t x, uint32_t wa, uint32_t wb)
{
    const long long xI = (int16_t)x, xQ = (int)x >> 16, re = (int)wb >> 16, im = (int16_t)wb;
    AI += xI * re - xQ * im;
    AQ += xI * im + xQ * re;
}

// parts[k]: n_epochs * N complex samples, 16-byte aligned; outs[a]: the same, none overlapping a part or another output;
// wts[((e * n_parts + k) * K + a) * 2]: the two packed words of the weight
template <int K, bool kWide>
__global__ __launch_bounds__(kThreads) void k_iq_array(const int16_t *const *__restrict__ parts, int16_t *const *__restrict__ outs,
                                                       const uint32_t *__restrict__ wts, int n_parts, int n_epochs, uint32_t N,
                                                       unsigned long long *sat)
{
    typedef std::conditional_t<kWide, long long, int> acc_t;
    uint32_t cnt = 0;
    for (int e = blockIdx.y; e < n_epochs; e += gridDim.y) {
        const uint32_t *__restrict__ w = wts + (size_t)e * n_parts * (2 * K);
        const uint64_t a = (uint64_t)e * N, b = a + N;    // the epoch's complex samples [a, b)
        const uint64_t v0 = (a + 3) >> 2, v1 = b >> 2;    // its whole vectors [v0, v1)
        const uint64_t stride = (uint64_t)gridDim.x * kThreads;
        for (uint64_t i = v0 + (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < v1; i += stride) {
            acc_t A[K][8];
#pragma unroll
            for (int el = 0; el < K; ++el)
#pragma unroll
                for (int m = 0; m < 8; ++m) A[el][m] = 0;
            int k = 0;
            for (; k + 2 <= n_parts; k += 2) {  // two parts' loads are issued before the first is used
                const v4i x0 = as_global<v4i>(parts[k])[i], x1 = as_global<v4i>(parts[k + 1])[i];
                const uint32_t *__restrict__ w0 = w + (size_t)k * (2 * K), *__restrict__ w1 = w0 + 2 * K;
#pragma unroll
                for (int el = 0; el < K; ++el)
#pragma unroll
                    for (int m = 0; m < 4; ++m) mac_w(A[el][2 * m], A[el][2 * m + 1], (uint32_t)x0[m], w0[2 * el], w0[2 * el + 1]);
#pragma unroll
                for (int el = 0; el < K; ++el)
#pragma unroll
                    for (int m = 0; m < 4; ++m) mac_w(A[el][2 * m], A[el][2 * m + 1], (uint32_t)x1[m], w1[2 * el], w1[2 * el + 1]);
            }
            if (k < n_parts) {
                const v4i x0 = as_global<v4i>(parts[k])[i];
                const uint32_t *__restrict__ w0 = w + (size_t)k * (2 * K);
#pragma unroll
                for (int el = 0; el < K; ++el)
#pragma unroll
                    for (int m = 0; m < 4; ++m) mac_w(A[el][2 * m], A[el][2 * m + 1], (uint32_t)x0[m], w0[2 * el], w0[2 * el + 1]);
            }
#pragma unroll
            for (int el = 0; el < K; ++el) {
                v4i y;
#pragma unroll
                for (int m = 0; m < 4; ++m) y[m] = (int)(q12(A[el][2 * m], cnt) | (q12(A[el][2 * m + 1], cnt) << 16));
                ((v4i *)outs[el])[i] = y;
            }
        }
        if (blockIdx.x == 0) {  // head [a, he) and tail [ts, b): at most three complex samples each, one per lane
            const uint64_t he = 4 * v0 < b ? 4 * v0 : b, ts = 4 * v1 > he ? 4 * v1 : he;
            const uint32_t nh = (uint32_t)(he - a), nt = (uint32_t)(b - ts);
            if (threadIdx.x < nh + nt) {
                const uint64_t n = threadIdx.x < nh ? a + threadIdx.x : ts + (threadIdx.x - nh);
                acc_t A[K][2];
#pragma unroll
                for (int el = 0; el < K; ++el) A[el][0] = A[el][1] = 0;
                for (int k = 0; k < n_parts; ++k) {
                    const uint32_t x = (uint32_t)as_global<int>(parts[k])[n];
                    const uint32_t *__restrict__ w0 = w + (size_t)k * (2 * K);
#pragma unroll
                    for (int el = 0; el < K; ++el) mac_w(A[el][0], A[el][1], x, w0[2 * el], w0[2 * el + 1]);
                }
#pragma unroll
                for (int el = 0; el < K; ++el) ((uint32_t *)outs[el])[n] = q12(A[el][0], cnt) | (q12(A[el][1], cnt) << 16);
            }
        }
    }
    add_block_count<kThreads>(cnt, sat);
}

template <int K>
void launch(dim3 grid, hipStream_t st, int wide, const int16_t *const *parts, int16_t *const *outs, const uint32_t *wts, int n_parts, int n_epochs,
            uint32_t N, unsigned long long *sat)
{
    if (wide)
        hipLaunchKernelGGL((k_iq_array<K, true>), grid, dim3(kThreads), 0, st, parts, outs, wts, n_parts, n_epochs, N, sat);
    else
        hipLaunchKernelGGL((k_iq_array<K, false>), grid, dim3(kThreads), 0, st, parts, outs, wts, n_parts, n_epochs, N, sat);
}

}  // namespace

// The two words the kernel reads for the weight (w_re, w_im), both in -32767 .. 32767: (w_re, -w_im) and (w_im, w_re), low half first.
extern "C" void galk_array_pack(int w_re, int w_im, uint32_t *two)
{
    two[0] = ((uint32_t)w_re & 0xffffu) | ((uint32_t)(-w_im) << 16);
    two[1] = ((uint32_t)w_im & 0xffffu) | ((uint32_t)w_re << 16);
}

// parts_dev: n_parts device pointers, outs_dev: n_elem (1 .. GAL_ARRAY_MAX_ELEM) device pointers (device tables); wts_dev:
// [n_epochs][n_parts][n_elem][2] words of galk_array_pack on the device; wide != 0: the int64 instance.  Arguments are checked by the
// caller (iq_api.cpp: gal_synth_iq_array).
extern "C" hipError_t galk_launch_iq_array(const int16_t *const *parts_dev, int16_t *const *outs_dev, const uint32_t *wts_dev, int n_parts,
                                           int n_elem, int n_epochs, int samples_per_epoch, int wide, unsigned long long *sat, hipStream_t st)
{
    const unsigned by = (unsigned)(n_epochs < kMaxBlocks ? n_epochs : kMaxBlocks);
    const unsigned need = (unsigned)((samples_per_epoch / 4 + kThreads - 1) / kThreads), cap = (unsigned)kMaxBlocks / by;
    const unsigned bx = need < 1 ? 1u : need > cap ? (cap < 1 ? 1u : cap) : need;
    const dim3 grid(bx, by);
    const uint32_t N = (uint32_t)samples_per_epoch;
    switch (n_elem) {
    case 1: launch<1>(grid, st, wide, parts_dev, outs_dev, wts_dev, n_parts, n_epochs, N, sat); break;
    case 2: launch<2>(grid, st, wide, parts_dev, outs_dev, wts_dev, n_parts, n_epochs, N, sat); break;
    case 3: launch<3>(grid, st, wide, parts_dev, outs_dev, wts_dev, n_parts, n_epochs, N, sat); break;
    case 4: launch<4>(grid, st, wide, parts_dev, outs_dev, wts_dev, n_parts, n_epochs, N, sat); break;
    case 5: launch<5>(grid, st, wide, parts_dev, outs_dev, wts_dev, n_parts, n_epochs, N, sat); break;
    case 6: launch<6>(grid, st, wide, parts_dev, outs_dev, wts_dev, n_parts, n_epochs, N, sat); break;
    case 7: launch<7>(grid, st, wide, parts_dev, outs_dev, wts_dev, n_parts, n_epochs, N, sat); break;
    case 8: launch<8>(grid, st, wide, parts_dev, outs_dev, wts_dev, n_parts, n_epochs, N, sat); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
