// iq_dev.h -- the device helpers the passes over the output stream share (iq_pass, iq_gain, iq_echo, iq_fir, iq_firdec, iq_agc, iq_osc,
// iq_corr, iq_psd .hip): ONE definition of each, force-inlined into the kernels of the file that includes it.  Everything is integer arithmetic.
//
// The two device tables reach only the files that ask for them: a file that needs the Gauss table defines GAL_GAUSS_DEVICE_TABLE before
// it includes this header, one that needs the cosine table GAL_INTERF_DEVICE_TABLE; only then are csrc/gauss_table.inc /
// csrc/interf_table.inc included and load_gauss_table() / load_cos_table() defined.  A file that defines neither carries no table.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#ifdef GAL_GAUSS_DEVICE_TABLE
#include "gauss_table.inc"
#endif
#ifdef GAL_INTERF_DEVICE_TABLE
#include "interf_table.inc"
#endif

namespace {

constexpr int kThreads = 256;  // lanes per block of every kernel of the passes (k_osc_scan alone has its own count)

typedef int v4i __attribute__((ext_vector_type(4)));
typedef short v2s __attribute__((ext_vector_type(2)));

// ---- the saturation count ------------------------------------------------------------------------------------------------------
// per-lane counts -> one ordinary global atomicAdd per block, and only where the block saw a saturated value: summed per wave by
// shuffles, per block through LDS.  Every lane of a block of kBlock lanes calls it, once, outside divergent control flow.
template <int kBlock>
__device__ __forceinline__ void add_block_count(uint32_t cnt, unsigned long long *sat)
{
    __shared__ unsigned long long part[kBlock / 64];
    unsigned long long c = cnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) s += part[w];
        if (s) atomicAdd(sat, s);
    }
}

// ---- noise ---------------------------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., Random123) of the counter (b lo, b hi, stream, c3) under the key (k0, k1).  c3 tells the users of one
// (seed, stream) apart: 0 the noise floor (iq_pass.hip), 1 the oscillator's phase noise (iq_osc.hip)
__device__ __forceinline__ void philox(uint64_t b, uint32_t k0, uint32_t k1, uint32_t stream, uint32_t c3, uint32_t (&o)[4])
{
    uint32_t c0 = (uint32_t)b, c1 = (uint32_t)(b >> 32), c2 = stream;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    o[0] = c0;
    o[1] = c1;
    o[2] = c2;
    o[3] = c3;
}

// uniform word -> z in Q12 (unit variance at 4096): the octave-segment inverse normal CDF of csrc/gauss_table.inc; tab = the packed
// table in LDS, one 32-bit word per cell, a | (a - b) << 16
__device__ __forceinline__ int gauss_q12(uint32_t u, const uint32_t *tab)
{
    const uint32_t w = u & 0x7fffffffu;
    const int o = w ? __builtin_clz(w) - 1 : 31;  // leading zeros of w as a 31-bit number
    const uint32_t wn = w << o;
    const uint32_t cell = tab[(o << 5) | ((wn >> 25) & 31u)];
    const int a = (int)(cell & 0xffffu), d = (int)(cell >> 16), f = (int)((wn >> 17) & 255u);
    const int mag = a - ((d * f + 128) >> 8);
    return (u >> 31) ? -mag : mag;
}

#ifdef GAL_GAUSS_DEVICE_TABLE
// the block's copy of the packed Gauss table (4 KB of LDS); every lane of a block of kThreads calls it
__device__ __forceinline__ const uint32_t *load_gauss_table()
{
    __shared__ uint32_t tab[1024];
    for (int k = threadIdx.x; k < 1024; k += kThreads) tab[k] = kGaussPacked[k];
    __syncthreads();
    return tab;
}
#endif

#ifdef GAL_INTERF_DEVICE_TABLE
// the block's copy of the 1024-entry Q12 cosine table (2 KB of LDS, filled by words of two entries); every lane of a block of
// kThreads calls it
__device__ __forceinline__ const int16_t *load_cos_table()
{
    __shared__ uint32_t cw[512];
    for (int k = threadIdx.x; k < 512; k += kThreads) cw[k] = kInterfCosPairs[k];
    __syncthreads();
    return (const int16_t *)cw;
}

// echoes (iq_echo.hip, iq_refl.hip): the complex value (uI, uQ), |u| <= 32768 per rail, turned by the table phase `ph` and scaled by A,
// added to (wI, wQ).  |uI c - uQ s| <= 2 x 32768 x 4096 = 2^28: the products before the shift fit an int32, |r| <= 65536
template <class acc_t>
__device__ __forceinline__ void mac_rot(acc_t &wI, acc_t &wQ, int uI, int uQ, uint32_t ph, int A, const int16_t *cosl)
{
    const uint32_t i = ph >> 22;
    const int c = cosl[i], s = cosl[(i - 256u) & 1023u];
    const int rI = (uI * c - uQ * s + 2048) >> 12, rQ = (uI * s + uQ * c + 2048) >> 12;
    wI += (acc_t)A * (acc_t)rI;
    wQ += (acc_t)A * (acc_t)rQ;
}
#endif

// ---- the formats' values -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int clamp16(int v) { return min(max(v, -32768), 32767); }

// v = a value before the clamp to int16; `sat` counts the values either clamp changes
__device__ __forceinline__ uint32_t f16(int v, uint32_t &sat)
{
    const int y = clamp16(v);
    sat += (uint32_t)(y != v);
    return (uint32_t)y & 0xffffu;
}

// ibyte: (y + r) >> s clamped to +-127, r = s ? 1 << (s - 1) : 0 (int32 arithmetic shift: round to nearest, ties up)
__device__ __forceinline__ uint32_t f8(int v, int s, int r, uint32_t &sat)
{
    const int y = clamp16(v), q = (y + r) >> s;
    sat += (uint32_t)((y != v) | (q < -127) | (q > 127));
    return (uint32_t)(min(max(q, -127), 127)) & 0xffu;
}

// the readers of a finished buffer (iq_corr.hip, iq_psd.hip): sample n of `buf` in format FMT (GAL_IQ_ISHORT, _IBYTE, _IBIT) as (I, Q)
template <int FMT>
__device__ __forceinline__ void load_iq(const void *buf, uint64_t n, int &I, int &Q)
{
    if (FMT == 0) {
        const int v = ((const int *)buf)[n];
        I = (v << 16) >> 16;
        Q = v >> 16;
    } else if (FMT == 1) {
        const int v = ((const unsigned short *)buf)[n];
        I = (v << 24) >> 24;
        Q = (v << 16) >> 24;
    } else {  // value 2n is bit 7 - (2n & 7) of byte n >> 2
        const int v = ((const unsigned char *)buf)[n >> 2];
        const int sh = 6 - 2 * (int)(n & 3);
        I = ((v >> (sh + 1)) & 1) * 2 - 1;
        Q = ((v >> sh) & 1) * 2 - 1;
    }
}

// ---- weighted sums of parts (iq_gain.hip, iq_echo.hip) ---------------------------------------------------------------------------
// a part's pointer comes out of a device table: say that it points to global memory (global_load instead of flat_load)
template <class T>
__device__ __forceinline__ const __attribute__((address_space(1))) T *as_global(const int16_t *p)
{
    return (const __attribute__((address_space(1))) T *)p;
}

// (w + 64) >> 7 clamped to int16; `sat` counts the values the clamp changes
template <class acc_t>
__device__ __forceinline__ uint32_t q7(acc_t w, uint32_t &sat)
{
    const acc_t v = (w + 64) >> 7;
    const acc_t y = v < -32768 ? (acc_t)-32768 : v > 32767 ? (acc_t)32767 : v;
    sat += (uint32_t)(y != v);
    return (uint32_t)y & 0xffffu;
}

// the four complex samples of vector `a` times g, added to w[0..7] (I0, Q0, I1, Q1, ...)
template <class acc_t>
__device__ __forceinline__ void mac8(acc_t (&w)[8], v4i a, int g)
{
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        w[2 * m] += (acc_t)g * (acc_t)(int16_t)a[m];
        w[2 * m + 1] += (acc_t)g * (acc_t)(a[m] >> 16);
    }
}

// ---- FIR walks (iq_fir.hip, iq_firdec.hip) -----------------------------------------------------------------------------------------
// acc + the two int16 of w times the two int16 of g (v_dot2_i32_i16)
__device__ __forceinline__ int dot2(uint32_t w, uint32_t g, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, w), __builtin_bit_cast(v2s, g), acc, false);
}

// (a + 8192) >> 14 is what `v` holds (the accumulators start at 8192); `sat` counts the values the clamp changes
__device__ __forceinline__ uint32_t q14(int v, uint32_t &sat)
{
    const int r = v >> 14, y = min(max(r, -32768), 32767);
    sat += (uint32_t)(y != r);
    return (uint32_t)y & 0xffffu;
}

}  // namespace
