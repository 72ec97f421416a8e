// iq_noise.hip -- the seeded AWGN noise floor of include/galsynth.h (gal_synth_iq_convert_noise), fused with the output formats of
// iq_format.hip: one pass over the FINAL interleaved int16 stream x[j] = I0, Q0, I1, Q1, ... per format.  Per value, with
// J = 2 first_sample + j the index of the value in the whole output stream (64-bit):
//
//   u     word J & 3 of Philox4x32-10(counter = (B lo, B hi, stream, 0), key = (seed lo, seed hi)), B = J >> 2
//   z     the octave-segment inverse normal CDF of u in Q12 (table T of csrc/gauss_table.inc; unit variance at 4096)
//   y     clamp16((int64(x) G + int64(z) S + 32768) >> 16)
//   out   y in the format: ishort y; ibyte (y + r) >> s clamped to +-127; ibit y > 0, MSB first
//
// A value counts once as saturated if either clamp changed it.  Everything is integer arithmetic: the output is a fixed function of
// (seed, stream, J, x) on any machine (tests/noise_model.py states it in numpy).
//
// Shape: as iq_format.hip -- 16-byte loads, 64-bit indices, a grid-stride loop, the values behind the last whole vector in one lane,
// per-block saturation counts.  A 16-byte vector holds 8 values = two Philox blocks when first_sample is even; when it is odd the
// vector starts at word 2 of a block and takes three (kOdd: correct, a block per vector wasted; the CLI's batches are even).  The
// table sits in LDS as one 32-bit word per cell, a | (a - b) << 16, 4 KB: half of all look-ups fall into the 32 cells of octave 0,
// which lie in 32 different banks.  The pass is bound by the 40 32-bit multiplies of a Philox block, not by HBM.
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

// n_val int16 values at `in` -> n_val int16 values at `out`; out == in (exactly in place) is allowed: a lane reads its vector
// before it writes it, and no other lane touches it
template <bool kOdd>
__global__ __launch_bounds__(kThreads) void k_iqn_ishort(const int16_t *in, int16_t *out, uint64_t n_val, NoiseArgs p, unsigned long long *sat)
{
    const uint32_t *tab = load_table();
    const uint64_t n_vec = n_val >> 3;  // 8 values per lane and trip
    const v4i *vin = (const v4i *)in;
    v4i *vout = (v4i *)out;
    uint32_t cnt = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n_vec; i += stride) {
        int v[8];
        mix8<kOdd>(vin[i], i, p, tab, v);
        v4i o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (int)(f16(v[2 * k], cnt) | (f16(v[2 * k + 1], cnt) << 16));
        vout[i] = o;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)  // tail: fewer than 8 values
        for (uint64_t j = n_vec << 3; j < n_val; ++j) out[j] = (int16_t)f16(mix1(in[j], j, p, tab), cnt);
    add_block_count(cnt, sat);
}

// n_val int16 values at `in` -> n_val int8 codes at `out`
template <bool kOdd>
__global__ __launch_bounds__(kThreads) void k_iqn_ibyte(const int16_t *__restrict__ in, int8_t *__restrict__ out, uint64_t n_val, int s,
                                                        NoiseArgs p, unsigned long long *__restrict__ sat)
{
    const uint32_t *tab = load_table();
    const int r = s ? 1 << (s - 1) : 0;
    const uint64_t n_vec = n_val >> 4;  // 16 values per lane and trip
    const v4i *vin = (const v4i *)in;
    v4i *vout = (v4i *)out;
    uint32_t cnt = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n_vec; i += stride) {
        const v4i a = vin[2 * i], b = vin[2 * i + 1];
        int v[8];
        v4i o;
        mix8<kOdd>(a, 2 * i, p, tab, v);
        o[0] = (int)(f8(v[0], s, r, cnt) | (f8(v[1], s, r, cnt) << 8) | (f8(v[2], s, r, cnt) << 16) | (f8(v[3], s, r, cnt) << 24));
        o[1] = (int)(f8(v[4], s, r, cnt) | (f8(v[5], s, r, cnt) << 8) | (f8(v[6], s, r, cnt) << 16) | (f8(v[7], s, r, cnt) << 24));
        mix8<kOdd>(b, 2 * i + 1, p, tab, v);
        o[2] = (int)(f8(v[0], s, r, cnt) | (f8(v[1], s, r, cnt) << 8) | (f8(v[2], s, r, cnt) << 16) | (f8(v[3], s, r, cnt) << 24));
        o[3] = (int)(f8(v[4], s, r, cnt) | (f8(v[5], s, r, cnt) << 8) | (f8(v[6], s, r, cnt) << 16) | (f8(v[7], s, r, cnt) << 24));
        vout[i] = o;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)  // tail: fewer than 16 values
        for (uint64_t j = n_vec << 4; j < n_val; ++j) out[j] = (int8_t)f8(mix1(in[j], j, p, tab), s, r, cnt);
    add_block_count(cnt, sat);
}

// n_val int16 values at `in` -> ceil(n_val / 8) bytes of sign bits at `out`
template <bool kOdd>
__global__ __launch_bounds__(kThreads) void k_iqn_ibit(const int16_t *__restrict__ in, uint8_t *__restrict__ out, uint64_t n_val, NoiseArgs p,
                                                       unsigned long long *__restrict__ sat)
{
    const uint32_t *tab = load_table();
    const uint64_t n_vec = n_val >> 6;  // 64 values per lane and trip
    const v4i *vin = (const v4i *)in;
    uint2 *vout = (uint2 *)out;
    uint32_t cnt = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n_vec; i += stride) {
        uint32_t byte[8];
#pragma unroll 2
        for (int k = 0; k < 8; ++k) {
            int v[8];
            mix8<kOdd>(vin[8 * i + k], 8 * i + k, p, tab, v);
            uint32_t b = 0;
#pragma unroll
            for (int m = 0; m < 8; ++m) b |= f1(v[m], cnt) << (7 - m);
            byte[k] = b;
        }
        uint2 o;
        o.x = byte[0] | (byte[1] << 8) | (byte[2] << 16) | (byte[3] << 24);
        o.y = byte[4] | (byte[5] << 8) | (byte[6] << 16) | (byte[7] << 24);
        vout[i] = o;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {  // tail: fewer than 64 values, ceil(rest / 8) bytes
        for (uint64_t j0 = n_vec << 6; j0 < n_val; j0 += 8) {
            uint32_t b = 0;
            for (int k = 0; k < 8 && j0 + k < n_val; ++k) b |= f1(mix1(in[j0 + k], j0 + k, p, tab), cnt) << (7 - k);
            out[j0 >> 3] = (uint8_t)b;
        }
    }
    add_block_count(cnt, sat);
}

unsigned blocks_for(uint64_t n_vec)
{
    const uint64_t b = (n_vec + kThreads - 1) / kThreads;
    return b < 1 ? 1u : b > (uint64_t)kMaxBlocks ? (unsigned)kMaxBlocks : (unsigned)b;
}

}  // namespace

extern "C" const int32_t *gal_tables_gauss(void) { return &kGaussT[0][0][0]; }

// format 0 (ishort), 1 (ibyte) or 2 (ibit) of n_val int16 values with the noise floor mixed in.  Arguments are checked by the caller
// (synth_api.cpp: gal_synth_iq_convert_noise).
extern "C" hipError_t galk_launch_iq_noise(int format, const int16_t *in, uint64_t n_val, uint64_t first_sample, uint64_t seed,
                                           uint32_t stream, uint32_t gain_q16, uint32_t sigma_q4, int shift, void *out,
                                           unsigned long long *sat, hipStream_t st)
{
    NoiseArgs p;
    p.j0 = 2 * first_sample;
    p.k0 = (uint32_t)seed;
    p.k1 = (uint32_t)(seed >> 32);
    p.stream = stream;
    p.g = (int)gain_q16;
    p.s = (int)sigma_q4;
    const bool odd = first_sample & 1;
    const dim3 blk(kThreads);
    if (format == 0) {
        const dim3 grid(blocks_for(n_val >> 3));
        if (odd) hipLaunchKernelGGL(k_iqn_ishort<true>, grid, blk, 0, st, in, (int16_t *)out, n_val, p, sat);
        else hipLaunchKernelGGL(k_iqn_ishort<false>, grid, blk, 0, st, in, (int16_t *)out, n_val, p, sat);
    } else if (format == 1) {
        const dim3 grid(blocks_for(n_val >> 4));
        if (odd) hipLaunchKernelGGL(k_iqn_ibyte<true>, grid, blk, 0, st, in, (int8_t *)out, n_val, shift, p, sat);
        else hipLaunchKernelGGL(k_iqn_ibyte<false>, grid, blk, 0, st, in, (int8_t *)out, n_val, shift, p, sat);
    } else {
        const dim3 grid(blocks_for(n_val >> 6));
        if (odd) hipLaunchKernelGGL(k_iqn_ibit<true>, grid, blk, 0, st, in, (uint8_t *)out, n_val, p, sat);
        else hipLaunchKernelGGL(k_iqn_ibit<false>, grid, blk, 0, st, in, (uint8_t *)out, n_val, p, sat);
    }
    return hipGetLastError();
}
