// iq_interf.hip -- the seeded interference sources of include/galsynth.h (gal_synth_iq_convert_interf): CW tones, linear chirps and
// pulsed sources, added in the same pass as the noise floor of iq_noise.hip, in front of the one clamp to int16 and the output format.
// Per complex sample N = first_sample + j / 2 (64-bit) and source:
//
//   (s, m)  = (N div sweep_len, N mod sweep_len)                     (a CW source is run as sweep_len 1, df 0: the same phase)
//   phi     = ph0 + s W + m f0 + df m (m - 1) / 2  (mod 2^32),  W = sweep_len f0 + df sweep_len (sweep_len - 1) / 2
//   i       = phi >> 22;  I takes A C[i], Q takes A C[(i - 256) & 1023] while (N mod pulse_period) < pulse_on
//   y       = clamp16((int64(x) G + int64(z) S + sum of the source terms + 32768) >> 16), then the format
//
// All of it is integer arithmetic: the output is a fixed function of (parameters, N, x) on any machine (tests/interf_model.py).
//
// Shape: as iq_noise.hip -- 16-byte loads, 64-bit indices, a grid-stride loop, a tail lane, per-block saturation counts, ishort
// exactly in place.  Nothing is divided per sample.  A lane handles a RUN of consecutive samples per trip (4 ishort, 8 ibyte, 32 ibit)
// and its next run lies a constant number of samples further on.  The host divides first_sample once per source; a lane finds its
// first (s, m) and pulse position with one 32-bit division per source, steps them sample by sample inside a run -- the phase by the
// recurrence phi += f0 + m df, which the closed form equals -- and takes the constant jump to its next run with the host's
// (jump div len, jump mod len) and one conditional correction, where the phase is formed anew from the closed form (four 32-bit
// multiplies).  The 2 KB cosine table sits in LDS beside the Gauss table; the source parameters arrive by value.
#include <string.h>

#include "../../include/galsynth.h"
#include "iq_mix_dev.h"

#define GAL_INTERF_DEVICE_TABLE
#include "interf_table.inc"

namespace {

struct InterfSrc {
    int amp;                  // A = amp_q4, 0 .. 2^20
    uint32_t ph0, f0, df, w;  // w = W, the phase advance of one whole sweep (mod 2^32)
    uint32_t len, period, on; // len >= 1 (CW: 1); period >= 1 (always on: 1 / 1)
    uint32_t s0, m0, p0;      // at the call's first sample: sweep number (low word), position in the sweep, position in the pulse period
    uint32_t ts, tm, tp;      // the same at the tail's first sample
    uint32_t jq, jr, jp;      // from the end of a run to the lane's next: jump div len, jump mod len, jump mod period
};

struct InterfArgs {
    int n;  // sources in use, 0 .. 4
    InterfSrc src[GAL_INTERF_MAX];
};

struct Lane {  // one source as one lane sees it, at the sample the lane handles next
    uint32_t s, m, pp, ph, step;
};

// m (m - 1) / 2 mod 2^32 (the product is even and below 2^64: halve the even factor first)
__device__ __forceinline__ uint32_t tri(uint32_t m) { return (m & 1u) ? m * ((m - 1u) >> 1) : (m >> 1) * (m - 1u); }

// phase and phase step of the closed form at (s, m)
__device__ __forceinline__ void rephase(const InterfSrc &c, Lane &l)
{
    l.ph = c.ph0 + l.s * c.w + l.m * c.f0 + c.df * tri(l.m);
    l.step = c.f0 + l.m * c.df;
}

// (s, m, pp) := (s, m, pp) + (q sweeps and r samples, rp pulse positions), r < len, rp < period
__device__ __forceinline__ void advance(const InterfSrc &c, Lane &l, uint32_t q, uint32_t r, uint32_t rp)
{
    const uint64_t m = (uint64_t)l.m + r, pp = (uint64_t)l.pp + rp;  // (both terms may be close to 2^32)
    const bool over = m >= c.len;
    l.s += q + (uint32_t)over;
    l.m = (uint32_t)(over ? m - c.len : m);
    l.pp = (uint32_t)(pp >= c.period ? pp - c.period : pp);
    rephase(c, l);
}

// the lane's first sample lies `off` samples behind the call's first
__device__ __forceinline__ void seek(const InterfArgs &p, Lane (&L)[GAL_INTERF_MAX], uint32_t off)
{
#pragma unroll
    for (int k = 0; k < GAL_INTERF_MAX; ++k)
        if (k < p.n) {
            const InterfSrc &c = p.src[k];
            const uint32_t q = off / c.len;
            L[k].s = c.s0;
            L[k].m = c.m0;
            L[k].pp = c.p0;
            advance(c, L[k], q, off - q * c.len, off % c.period);
        }
}

__device__ __forceinline__ void jump(const InterfArgs &p, Lane (&L)[GAL_INTERF_MAX])
{
#pragma unroll
    for (int k = 0; k < GAL_INTERF_MAX; ++k)
        if (k < p.n) advance(p.src[k], L[k], p.src[k].jq, p.src[k].jr, p.src[k].jp);
}

// the source terms of one complex sample added to (aI, aQ); every source steps to the next sample
__device__ __forceinline__ void sources(const InterfArgs &p, Lane (&L)[GAL_INTERF_MAX], const int16_t *ct, long long &aI, long long &aQ)
{
#pragma unroll
    for (int k = 0; k < GAL_INTERF_MAX; ++k)
        if (k < p.n) {
            const InterfSrc &c = p.src[k];
            Lane &l = L[k];
            const uint32_t i = l.ph >> 22;
            const int a = l.pp < c.on ? c.amp : 0;
            aI += (long long)a * ct[i];
            aQ += (long long)a * ct[(i - 256u) & 1023u];
            l.ph += l.step;
            const bool wrap = l.m + 1u == c.len;
            l.m = wrap ? 0u : l.m + 1u;
            l.step = wrap ? c.f0 : l.step + c.df;
            l.s += (uint32_t)wrap;
            l.pp = l.pp + 1u == c.period ? 0u : l.pp + 1u;
        }
}

// kMode 0: nothing random (S = 0: no Philox work); 1: noise, even first_sample; 2: noise, odd first_sample (iq_noise.hip: kOdd)
// the eight values of vector `a` (index i of the call: the complex samples 4 i .. 4 i + 3) mixed, not yet clamped
template <int kMode>
__device__ __forceinline__ void mix8i(v4i a, uint64_t i, const NoiseArgs &np, const InterfArgs &ip, Lane (&L)[GAL_INTERF_MAX],
                                      const uint32_t *gt, const int16_t *ct, int (&v)[8])
{
    uint32_t u[8];
    if (kMode) {
        const uint64_t b = (np.j0 >> 2) + 2 * i;
        uint32_t b0[4], b1[4];
        philox(b, np, b0);
        philox(b + 1, np, b1);
        if (kMode == 2) {
            uint32_t b2[4];
            philox(b + 2, np, b2);
            u[0] = b0[2], u[1] = b0[3], u[2] = b1[0], u[3] = b1[1], u[4] = b1[2], u[5] = b1[3], u[6] = b2[0], u[7] = b2[1];
        } else {
            u[0] = b0[0], u[1] = b0[1], u[2] = b0[2], u[3] = b0[3], u[4] = b1[0], u[5] = b1[1], u[6] = b1[2], u[7] = b1[3];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        long long aI = 32768, aQ = 32768;
        sources(ip, L, ct, aI, aQ);
        const int xI = (a[k] << 16) >> 16, xQ = a[k] >> 16;
        if (kMode) {
            aI += (long long)xI * np.g + (long long)gauss_q12(u[2 * k], gt) * np.s;
            aQ += (long long)xQ * np.g + (long long)gauss_q12(u[2 * k + 1], gt) * np.s;
        } else {
            aI += (long long)xI * np.g;
            aQ += (long long)xQ * np.g;
        }
        v[2 * k] = (int)(aI >> 16);  // |value| < 2^23: it fits an int
        v[2 * k + 1] = (int)(aQ >> 16);
    }
}

// one complex sample of the tail: the values j, j + 1 of the call (j even)
template <int kMode>
__device__ __forceinline__ void mix2i(int xI, int xQ, uint64_t j, const NoiseArgs &np, const InterfArgs &ip, Lane (&L)[GAL_INTERF_MAX],
                                      const uint32_t *gt, const int16_t *ct, int &vI, int &vQ)
{
    long long aI = 32768, aQ = 32768;
    sources(ip, L, ct, aI, aQ);
    if (kMode) {
        const uint64_t J = np.j0 + j;  // even: both values lie in one Philox block
        uint32_t o[4];
        philox(J >> 2, np, o);
        const bool hi = (J & 2) != 0;
        aI += (long long)xI * np.g + (long long)gauss_q12(hi ? o[2] : o[0], gt) * np.s;
        aQ += (long long)xQ * np.g + (long long)gauss_q12(hi ? o[3] : o[1], gt) * np.s;
    } else {
        aI += (long long)xI * np.g;
        aQ += (long long)xQ * np.g;
    }
    vI = (int)(aI >> 16);
    vQ = (int)(aQ >> 16);
}

__device__ __forceinline__ const int16_t *load_cos_table()
{
    __shared__ uint32_t cw[512];
    for (int k = threadIdx.x; k < 512; k += kThreads) cw[k] = kInterfCosPairs[k];
    __syncthreads();
    return (const int16_t *)cw;
}

// the lane that takes the values behind the last whole vector starts from the tail's state
__device__ __forceinline__ void seek_tail(const InterfArgs &p, Lane (&L)[GAL_INTERF_MAX])
{
#pragma unroll
    for (int k = 0; k < GAL_INTERF_MAX; ++k)
        if (k < p.n) {
            L[k].s = p.src[k].ts;
            L[k].m = p.src[k].tm;
            L[k].pp = p.src[k].tp;
            rephase(p.src[k], L[k]);
        }
}

// n_val int16 values at `in` -> n_val int16 values at `out`; out == in (exactly in place) is allowed: a lane reads its vector
// before it writes it, and no other lane touches it
template <int kMode>
__global__ __launch_bounds__(kThreads) void k_iqi_ishort(const int16_t *in, int16_t *out, uint64_t n_val, NoiseArgs np, InterfArgs ip,
                                                         unsigned long long *sat)
{
    const uint32_t *gt = load_table();
    const int16_t *ct = load_cos_table();
    const uint64_t n_vec = n_val >> 3;  // 8 values = 4 complex samples per lane and trip
    const v4i *vin = (const v4i *)in;
    v4i *vout = (v4i *)out;
    uint32_t cnt = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    const uint32_t lane = blockIdx.x * kThreads + threadIdx.x;
    Lane L[GAL_INTERF_MAX];
    if (lane < n_vec) seek(ip, L, 4 * lane);
    for (uint64_t i = lane; i < n_vec; i += stride) {
        int v[8];
        mix8i<kMode>(vin[i], i, np, ip, L, gt, ct, v);
        v4i o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (int)(f16(v[2 * k], cnt) | (f16(v[2 * k + 1], cnt) << 16));
        vout[i] = o;
        jump(ip, L);
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0 && (n_vec << 3) < n_val) {  // tail: fewer than 4 complex samples
        seek_tail(ip, L);
        for (uint64_t j = n_vec << 3; j < n_val; j += 2) {
            int vI, vQ;
            mix2i<kMode>(in[j], in[j + 1], j, np, ip, L, gt, ct, vI, vQ);
            out[j] = (int16_t)f16(vI, cnt);
            out[j + 1] = (int16_t)f16(vQ, cnt);
        }
    }
    add_block_count(cnt, sat);
}

// n_val int16 values at `in` -> n_val int8 codes at `out`
template <int kMode>
__global__ __launch_bounds__(kThreads) void k_iqi_ibyte(const int16_t *__restrict__ in, int8_t *__restrict__ out, uint64_t n_val, int s,
                                                        NoiseArgs np, InterfArgs ip, unsigned long long *__restrict__ sat)
{
    const uint32_t *gt = load_table();
    const int16_t *ct = load_cos_table();
    const int r = s ? 1 << (s - 1) : 0;
    const uint64_t n_vec = n_val >> 4;  // 16 values = 8 complex samples per lane and trip
    const v4i *vin = (const v4i *)in;
    v4i *vout = (v4i *)out;
    uint32_t cnt = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    const uint32_t lane = blockIdx.x * kThreads + threadIdx.x;
    Lane L[GAL_INTERF_MAX];
    if (lane < n_vec) seek(ip, L, 8 * lane);
    for (uint64_t i = lane; i < n_vec; i += stride) {
        const v4i a = vin[2 * i], b = vin[2 * i + 1];
        int v[8];
        v4i o;
        mix8i<kMode>(a, 2 * i, np, ip, L, gt, ct, v);
        o[0] = (int)(f8(v[0], s, r, cnt) | (f8(v[1], s, r, cnt) << 8) | (f8(v[2], s, r, cnt) << 16) | (f8(v[3], s, r, cnt) << 24));
        o[1] = (int)(f8(v[4], s, r, cnt) | (f8(v[5], s, r, cnt) << 8) | (f8(v[6], s, r, cnt) << 16) | (f8(v[7], s, r, cnt) << 24));
        mix8i<kMode>(b, 2 * i + 1, np, ip, L, gt, ct, v);
        o[2] = (int)(f8(v[0], s, r, cnt) | (f8(v[1], s, r, cnt) << 8) | (f8(v[2], s, r, cnt) << 16) | (f8(v[3], s, r, cnt) << 24));
        o[3] = (int)(f8(v[4], s, r, cnt) | (f8(v[5], s, r, cnt) << 8) | (f8(v[6], s, r, cnt) << 16) | (f8(v[7], s, r, cnt) << 24));
        vout[i] = o;
        jump(ip, L);
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0 && (n_vec << 4) < n_val) {  // tail: fewer than 8 complex samples
        seek_tail(ip, L);
        for (uint64_t j = n_vec << 4; j < n_val; j += 2) {
            int vI, vQ;
            mix2i<kMode>(in[j], in[j + 1], j, np, ip, L, gt, ct, vI, vQ);
            out[j] = (int8_t)f8(vI, s, r, cnt);
            out[j + 1] = (int8_t)f8(vQ, s, r, cnt);
        }
    }
    add_block_count(cnt, sat);
}

// n_val int16 values at `in` -> ceil(n_val / 8) bytes of sign bits at `out`
template <int kMode>
__global__ __launch_bounds__(kThreads) void k_iqi_ibit(const int16_t *__restrict__ in, uint8_t *__restrict__ out, uint64_t n_val, NoiseArgs np,
                                                       InterfArgs ip, unsigned long long *__restrict__ sat)
{
    const uint32_t *gt = load_table();
    const int16_t *ct = load_cos_table();
    const uint64_t n_vec = n_val >> 6;  // 64 values = 32 complex samples per lane and trip
    const v4i *vin = (const v4i *)in;
    uint2 *vout = (uint2 *)out;
    uint32_t cnt = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    const uint32_t lane = blockIdx.x * kThreads + threadIdx.x;
    Lane L[GAL_INTERF_MAX];
    if (lane < n_vec) seek(ip, L, 32 * lane);
    for (uint64_t i = lane; i < n_vec; i += stride) {
        uint32_t byte[8];
#pragma unroll 2
        for (int k = 0; k < 8; ++k) {
            int v[8];
            mix8i<kMode>(vin[8 * i + k], 8 * i + k, np, ip, L, gt, ct, v);
            uint32_t b = 0;
#pragma unroll
            for (int m = 0; m < 8; ++m) b |= f1(v[m], cnt) << (7 - m);
            byte[k] = b;
        }
        uint2 o;
        o.x = byte[0] | (byte[1] << 8) | (byte[2] << 16) | (byte[3] << 24);
        o.y = byte[4] | (byte[5] << 8) | (byte[6] << 16) | (byte[7] << 24);
        vout[i] = o;
        jump(ip, L);
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0 && (n_vec << 6) < n_val) {  // tail: fewer than 32 complex samples, ceil(rest / 8) bytes
        seek_tail(ip, L);
        for (uint64_t j0 = n_vec << 6; j0 < n_val; j0 += 8) {
            uint32_t b = 0;
            for (int k = 0; k < 8 && j0 + k < n_val; k += 2) {
                int vI, vQ;
                mix2i<kMode>(in[j0 + k], in[j0 + k + 1], j0 + k, np, ip, L, gt, ct, vI, vQ);
                b |= (f1(vI, cnt) << (7 - k)) | (f1(vQ, cnt) << (6 - k));
            }
            out[j0 >> 3] = (uint8_t)b;
        }
    }
    add_block_count(cnt, sat);
}

uint32_t tri_host(uint32_t m) { return (uint32_t)(((uint64_t)m * (uint64_t)(m ? m - 1 : 0)) >> 1); }

}  // namespace

extern "C" const int16_t *gal_tables_cos1024(void) { return kInterfCos; }

// format 0 (ishort), 1 (ibyte) or 2 (ibit) of n_val int16 values with the noise floor (noise may be null: none) and n_src sources
// mixed in.  Arguments are checked by the caller (synth_api.cpp: gal_synth_iq_convert_interf).
extern "C" hipError_t galk_launch_iq_interf(int format, const int16_t *in, uint64_t n_val, uint64_t first_sample, const gal_iq_noise_t *noise,
                                            const gal_iq_interf_t *src, int n_src, int shift, void *out, unsigned long long *sat,
                                            hipStream_t st)
{
    NoiseArgs np;
    memset(&np, 0, sizeof(np));
    np.j0 = 2 * first_sample;
    np.g = 65536;
    if (noise) {
        np.k0 = (uint32_t)noise->seed;
        np.k1 = (uint32_t)(noise->seed >> 32);
        np.stream = noise->stream;
        np.g = (int)noise->gain_q16;
        np.s = (int)noise->sigma_q4;
    }
    const int run = format == 0 ? 4 : format == 1 ? 8 : 32;  // complex samples a lane handles per trip
    const uint64_t n_vec = n_val / (2 * (uint64_t)run);
    const dim3 blk(kThreads), grid(blocks_for(n_vec));
    const uint64_t jump = (uint64_t)grid.x * kThreads * run - run;  // < 2^24
    const uint64_t tail = first_sample + n_vec * run;
    InterfArgs ip;
    memset(&ip, 0, sizeof(ip));
    for (int k = 0; k < n_src; ++k) {
        if (src[k].amp_q4 == 0) continue;  // adds nothing
        InterfSrc &c = ip.src[ip.n++];
        c.amp = (int)src[k].amp_q4;
        c.ph0 = src[k].ph0;
        c.f0 = (uint32_t)src[k].f0;
        c.len = src[k].sweep_len ? src[k].sweep_len : 1u;  // CW: sweeps of one sample, W = f0
        c.df = src[k].sweep_len ? (uint32_t)src[k].df : 0u;
        c.w = c.len * c.f0 + c.df * tri_host(c.len);
        c.period = src[k].pulse_period ? src[k].pulse_period : 1u;
        c.on = src[k].pulse_period ? src[k].pulse_on : 1u;
        c.s0 = (uint32_t)(first_sample / c.len);
        c.m0 = (uint32_t)(first_sample % c.len);
        c.p0 = (uint32_t)(first_sample % c.period);
        c.ts = (uint32_t)(tail / c.len);
        c.tm = (uint32_t)(tail % c.len);
        c.tp = (uint32_t)(tail % c.period);
        c.jq = (uint32_t)(jump / c.len);
        c.jr = (uint32_t)(jump % c.len);
        c.jp = (uint32_t)(jump % c.period);
    }
    const int mode = !noise || noise->sigma_q4 == 0 ? 0 : (first_sample & 1) ? 2 : 1;  // (z S = 0 whatever z)
    if (format == 0) {
        if (mode == 0) hipLaunchKernelGGL(k_iqi_ishort<0>, grid, blk, 0, st, in, (int16_t *)out, n_val, np, ip, sat);
        else if (mode == 1) hipLaunchKernelGGL(k_iqi_ishort<1>, grid, blk, 0, st, in, (int16_t *)out, n_val, np, ip, sat);
        else hipLaunchKernelGGL(k_iqi_ishort<2>, grid, blk, 0, st, in, (int16_t *)out, n_val, np, ip, sat);
    } else if (format == 1) {
        if (mode == 0) hipLaunchKernelGGL(k_iqi_ibyte<0>, grid, blk, 0, st, in, (int8_t *)out, n_val, shift, np, ip, sat);
        else if (mode == 1) hipLaunchKernelGGL(k_iqi_ibyte<1>, grid, blk, 0, st, in, (int8_t *)out, n_val, shift, np, ip, sat);
        else hipLaunchKernelGGL(k_iqi_ibyte<2>, grid, blk, 0, st, in, (int8_t *)out, n_val, shift, np, ip, sat);
    } else {
        if (mode == 0) hipLaunchKernelGGL(k_iqi_ibit<0>, grid, blk, 0, st, in, (uint8_t *)out, n_val, np, ip, sat);
        else if (mode == 1) hipLaunchKernelGGL(k_iqi_ibit<1>, grid, blk, 0, st, in, (uint8_t *)out, n_val, np, ip, sat);
        else hipLaunchKernelGGL(k_iqi_ibit<2>, grid, blk, 0, st, in, (uint8_t *)out, n_val, np, ip, sat);
    }
    return hipGetLastError();
}
