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
#include "iq_mix_dev.h"

namespace {

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
