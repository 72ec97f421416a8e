// iq_mix_dev.h -- device helpers shared by the passes over the final int16 stream (iq_noise.hip, iq_interf.hip): Philox4x32-10, the
// Gaussian word, the integer mix of include/galsynth.h, the three output formats with their saturation counts, the LDS copy of the
// Gauss table and the per-block count.  Everything is __forceinline__: each pass compiles its own copy.
#ifndef GAL_IQ_MIX_DEV_H_
#define GAL_IQ_MIX_DEV_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GAL_GAUSS_DEVICE_TABLE
#include "gauss_table.inc"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;  // 8 blocks of 4 waves per CU, the rest by the grid-stride loop

typedef int v4i __attribute__((ext_vector_type(4)));

struct NoiseArgs {
    uint64_t j0;      // 2 first_sample: the global index of the call's first value
    uint32_t k0, k1;  // seed, low and high word
    uint32_t stream;
    int g, s;         // gain_q16, sigma_q4 (both <= 2^20)
};

// Philox4x32-10 (Salmon et al., Random123) of the counter (b lo, b hi, stream, 0)
__device__ __forceinline__ void philox(uint64_t b, const NoiseArgs &p, uint32_t (&o)[4])
{
    uint32_t c0 = (uint32_t)b, c1 = (uint32_t)(b >> 32), c2 = p.stream, c3 = 0, k0 = p.k0, k1 = p.k1;
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

// uniform word -> z in Q12; tab = the packed table in LDS
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

// (x G + z S + 32768) >> 16 BEFORE the clamp to int16 (|value| < 2^21: it fits an int)
__device__ __forceinline__ int mix(int x, uint32_t u, const NoiseArgs &p, const uint32_t *tab)
{
    return (int)(((long long)x * p.g + (long long)gauss_q12(u, tab) * p.s + 32768) >> 16);
}

__device__ __forceinline__ int clamp16(int v) { return min(max(v, -32768), 32767); }

// the eight values of vector `a` (the vector with index i of the call: values 8 i .. 8 i + 7) mixed, not yet clamped
template <bool kOdd>
__device__ __forceinline__ void mix8(v4i a, uint64_t i, const NoiseArgs &p, const uint32_t *tab, int (&v)[8])
{
    const uint64_t b = (p.j0 >> 2) + 2 * i;  // the block of the vector's first value (kOdd: from its word 2 on)
    uint32_t u[8], b0[4], b1[4];
    philox(b, p, b0);
    philox(b + 1, p, b1);
    if (kOdd) {
        uint32_t b2[4];
        philox(b + 2, p, b2);
        u[0] = b0[2], u[1] = b0[3], u[2] = b1[0], u[3] = b1[1], u[4] = b1[2], u[5] = b1[3], u[6] = b2[0], u[7] = b2[1];
    } else {
        u[0] = b0[0], u[1] = b0[1], u[2] = b0[2], u[3] = b0[3], u[4] = b1[0], u[5] = b1[1], u[6] = b1[2], u[7] = b1[3];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[2 * k] = mix((a[k] << 16) >> 16, u[2 * k], p, tab);
        v[2 * k + 1] = mix(a[k] >> 16, u[2 * k + 1], p, tab);
    }
}

// one value of the tail: value j of the call
__device__ __forceinline__ int mix1(int x, uint64_t j, const NoiseArgs &p, const uint32_t *tab)
{
    const uint64_t J = p.j0 + j;
    uint32_t o[4];
    philox(J >> 2, p, o);
    const int k = (int)(J & 3);
    return mix(x, k == 0 ? o[0] : k == 1 ? o[1] : k == 2 ? o[2] : o[3], p, tab);
}

// formats: v = a mixed value before the clamp to int16; `sat` counts the values either clamp changes
__device__ __forceinline__ uint32_t f16(int v, uint32_t &sat)
{
    const int y = clamp16(v);
    sat += (uint32_t)(y != v);
    return (uint32_t)y & 0xffffu;
}

__device__ __forceinline__ uint32_t f8(int v, int s, int r, uint32_t &sat)
{
    const int y = clamp16(v), q = (y + r) >> s;
    sat += (uint32_t)((y != v) | (q < -127) | (q > 127));
    return (uint32_t)(min(max(q, -127), 127)) & 0xffu;
}

__device__ __forceinline__ uint32_t f1(int v, uint32_t &sat)
{
    sat += (uint32_t)((v < -32768) | (v > 32767));
    return (uint32_t)(v > 0);
}

__device__ __forceinline__ const uint32_t *load_table()
{
    __shared__ uint32_t tab[1024];
    for (int k = threadIdx.x; k < 1024; k += kThreads) tab[k] = kGaussPacked[k];
    __syncthreads();
    return tab;
}

// per-lane counts -> one atomicAdd per block (only where the block saw a saturated value)
__device__ __forceinline__ void add_block_count(uint32_t cnt, unsigned long long *sat)
{
    __shared__ unsigned long long part[kThreads / 64];
    unsigned long long c = cnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) s += part[w];
        if (s) atomicAdd(sat, s);
    }
}

inline unsigned blocks_for(uint64_t n_vec)
{
    const uint64_t b = (n_vec + kThreads - 1) / kThreads;
    return b < 1 ? 1u : b > (uint64_t)kMaxBlocks ? (unsigned)kMaxBlocks : (unsigned)b;
}

}  // namespace
#endif  // GAL_IQ_MIX_DEV_H_
