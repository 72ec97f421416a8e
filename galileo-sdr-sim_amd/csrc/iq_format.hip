// iq_format.hip -- the 8-bit and 1-bit IQ output formats of include/galsynth.h (GAL_IQ_IBYTE, GAL_IQ_IBIT), converted on the
// device from the FINAL interleaved int16 stream x[j] = I0, Q0, I1, Q1, ... (src/galileo-sdr.cpp:536-537):
//
//   ibyte  out[j] = (int8) clamp((x[j] + r) >> s, -127, 127), r = s ? 1 << (s - 1) : 0 (int32 arithmetic shift: round to
//          nearest, ties up); a value whose shifted v lies outside [-127, 127] is SATURATED and counted
//   ibit   bit = x[j] > 0, byte k = x[8k] .. x[8k+7] with x[8k] in bit 7 (numpy.packbits(x > 0)); unused low bits of the
//          last byte are 0
//
// Both are memory-bound streams: every input byte is read once, nothing is reused.  One lane converts 16 int16 values
// (ibyte: two 16-byte loads, one 16-byte store) or 64 (ibit: eight 16-byte loads, one byte of bits per load, one 8-byte store)
// per trip of a grid-stride loop with 64-bit indices (a batch of the library may hold well over 2^31 bytes).  Input loads are
// plain: non-temporal ones (__builtin_nontemporal_load) were measured slower for ibit at every size (2.1x at 311.74 M samples) and
// for ibyte on the CLI's 128-epoch batch, which the synthesis has just written.  The values behind
// the last whole vector go through a short per-value path in one lane.  Saturated values are counted per lane in a register,
// summed per wave (shuffles) and per block (LDS), and one lane per block adds the block's sum to the handle's 64-bit counter
// with one ordinary global atomicAdd -- and only if it is not 0.
//
// This is a separate launch behind gal_synth_finish, never fused into the synthesis kernels: k_repair_g and the accumulating
// exact-replay launches rewrite int16 output after k_synth_g has run, and gal_synth_finish may synthesise the batch again.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kIqThreads = 256;
constexpr int kIqMaxBlocks = 2048;  // memory-bound: ~8 blocks per CU, the rest by the grid-stride loop

typedef int v4i __attribute__((ext_vector_type(4)));

// one int16 value -> int8 code; `sat` counts the values outside [-127, 127] after the shift
__device__ __forceinline__ uint32_t q8(int x, int s, int r, uint32_t &sat)
{
    const int v = (x + r) >> s;
    sat += (uint32_t)((v < -127) | (v > 127));
    return (uint32_t)(min(max(v, -127), 127)) & 0xffu;
}

// two int16 values (one little-endian word: low half first) -> two int8 codes in the low 16 bits
__device__ __forceinline__ uint32_t q8x2(int w, int s, int r, uint32_t &sat)
{
    return q8((w << 16) >> 16, s, r, sat) | (q8(w >> 16, s, r, sat) << 8);
}

// eight int16 values (one 16-byte vector) -> one byte of sign bits, the first value in bit 7
__device__ __forceinline__ uint32_t bits8(v4i a)
{
    uint32_t b = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int w = a[k];
        b |= (uint32_t)(((w << 16) >> 16) > 0) << (7 - 2 * k);
        b |= (uint32_t)((w >> 16) > 0) << (6 - 2 * k);
    }
    return b;
}

// per-lane counts -> one atomicAdd per block (only where the block saw a saturated value)
__device__ __forceinline__ void add_block_count(uint32_t cnt, unsigned long long *sat)
{
    __shared__ unsigned long long part[kIqThreads / 64];
    unsigned long long c = cnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < kIqThreads / 64; ++w) s += part[w];
        if (s) atomicAdd(sat, s);
    }
}

// n_val int16 values at `in` (16-byte aligned) -> n_val int8 codes at `out` (16-byte aligned)
__global__ __launch_bounds__(kIqThreads) void k_iq_ibyte(const int16_t *__restrict__ in, int8_t *__restrict__ out, uint64_t n_val,
                                                         int s, unsigned long long *__restrict__ sat)
{
    const int r = s ? 1 << (s - 1) : 0;
    const uint64_t n_vec = n_val >> 4;  // 16 values per lane and trip
    const v4i *vin = (const v4i *)in;
    v4i *vout = (v4i *)out;
    uint32_t cnt = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kIqThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kIqThreads + threadIdx.x; i < n_vec; i += stride) {
        const v4i a = vin[2 * i], b = vin[2 * i + 1];
        v4i o;
        o[0] = (int)(q8x2(a[0], s, r, cnt) | (q8x2(a[1], s, r, cnt) << 16));
        o[1] = (int)(q8x2(a[2], s, r, cnt) | (q8x2(a[3], s, r, cnt) << 16));
        o[2] = (int)(q8x2(b[0], s, r, cnt) | (q8x2(b[1], s, r, cnt) << 16));
        o[3] = (int)(q8x2(b[2], s, r, cnt) | (q8x2(b[3], s, r, cnt) << 16));
        vout[i] = o;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)  // tail: fewer than 16 values
        for (uint64_t j = n_vec << 4; j < n_val; ++j) out[j] = (int8_t)q8(in[j], s, r, cnt);
    add_block_count(cnt, sat);
}

// n_val int16 values at `in` (16-byte aligned) -> ceil(n_val / 8) bytes of sign bits at `out` (16-byte aligned)
__global__ __launch_bounds__(kIqThreads) void k_iq_ibit(const int16_t *__restrict__ in, uint8_t *__restrict__ out, uint64_t n_val)
{
    const uint64_t n_vec = n_val >> 6;  // 64 values per lane and trip
    const v4i *vin = (const v4i *)in;
    uint2 *vout = (uint2 *)out;
    const uint64_t stride = (uint64_t)gridDim.x * kIqThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kIqThreads + threadIdx.x; i < n_vec; i += stride) {
        v4i a[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = vin[8 * i + k];
        uint2 o;
        o.x = bits8(a[0]) | (bits8(a[1]) << 8) | (bits8(a[2]) << 16) | (bits8(a[3]) << 24);
        o.y = bits8(a[4]) | (bits8(a[5]) << 8) | (bits8(a[6]) << 16) | (bits8(a[7]) << 24);
        vout[i] = o;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {  // tail: fewer than 64 values, ceil(rest / 8) bytes
        for (uint64_t j0 = n_vec << 6; j0 < n_val; j0 += 8) {
            uint32_t b = 0;
            for (int k = 0; k < 8 && j0 + k < n_val; ++k) b |= (uint32_t)(in[j0 + k] > 0) << (7 - k);
            out[j0 >> 3] = (uint8_t)b;
        }
    }
}

unsigned blocks_for(uint64_t n_vec)
{
    const uint64_t b = (n_vec + kIqThreads - 1) / kIqThreads;
    return b < 1 ? 1u : b > (uint64_t)kIqMaxBlocks ? (unsigned)kIqMaxBlocks : (unsigned)b;
}

}  // namespace

// format 1 (ibyte) or 2 (ibit) of n_val int16 values.  Arguments are checked by the caller (synth_api.cpp: gal_synth_iq_convert).
extern "C" hipError_t galk_launch_iq(int format, const int16_t *in, uint64_t n_val, int shift, void *out, unsigned long long *sat,
                                     hipStream_t st)
{
    if (format == 1)
        hipLaunchKernelGGL(k_iq_ibyte, dim3(blocks_for(n_val >> 4)), dim3(kIqThreads), 0, st, in, (int8_t *)out, n_val, shift, sat);
    else
        hipLaunchKernelGGL(k_iq_ibit, dim3(blocks_for(n_val >> 6)), dim3(kIqThreads), 0, st, in, (uint8_t *)out, n_val);
    return hipGetLastError();
}
