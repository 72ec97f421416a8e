// iq_osc.hip -- the receiver's local oscillator (include/galsynth.h: gal_synth_osc_set, gal_synth_iq_osc): a
// rotation common to everything in the stream, by a phase with an offset, a drift and white-FM phase noise.  x[n] = the complex int16
// sample with the global index N = first_sample + n; all phase arithmetic modulo 2^64, in units of 2^-64 cycles:
//
//   Phi(N) = P0 + N F + T(N) D + S Z(N),  T(N) = N (N - 1) / 2 (the even factor halved first),  Z(N) = sum of z(j) for N0 < j <= N
//   z(j)   = the Q12 Gaussian of iq_dev.h of word j & 3 of Philox4x32-10(counter = (B lo, B hi, stream, 1), key = seed), B = j >> 2
//   theta  = Phi >> 32;  t = theta + 2^21 (mod 2^32);  i = t >> 22;  e = ((t >> 10) & 4095) - 2048
//   c0 = C[i], s0 = C[(i - 256) & 1023];  c = c0 - ((s0 e 101 + 2^25) >> 26);  s = s0 + ((c0 e 101 + 2^25) >> 26)
//   yI = clamp16((xI c - xQ s + 2048) >> 12);  yQ = clamp16((xI s + xQ c + 2048) >> 12)
//
// A complex sample counts once as saturated if either clamp changed it.  Integer arithmetic only (tests/osc_model.py states it in
// numpy).  |s0 e 101| <= 4096 x 2048 x 101 < 2^30, |c|, |s| <= 4096 + 13, |xI c - xQ s| + 2048 <= 2 x 32768 x 4109 + 2048 < 2^29: int32.
//
// Z is a running sum over the whole stream, so a call is a scan in three launches, ordered by the stream alone -- no block waits for
// another.  A TILE is kTile = 1024 consecutive samples of the call (a block of 256 lanes, four consecutive samples per lane):
//
//   k_osc_tilesum  sums[t] = the sum of the z of tile t (int32: 1024 x 25960 < 2^25); a Philox block yields the four z of a lane
//   k_osc_scan     one block: pre[t] = R + sums[0] + ... + sums[t - 1] (int64), R = Z at the sample in front of the call, read from one
//                  of the handle's two state words; R + the sum of all tiles goes to the OTHER word, which the host then makes current
//   k_iq_osc       regenerates the z of the tile, scans them inside the tile (lane sums through the wave by shuffles, the four wave
//                  totals through LDS), forms Phi and rotates: 16-byte loads and stores, the cosine table (2 KB) in LDS
//
// Sums modulo 2^64 are associative: the bytes do not depend on the tile length or on how the stream is cut into calls.  With S = 0
// only k_iq_osc<false> runs, which has no Philox work, no Gauss table and no scan.  A call whose first sample is no multiple of four
// (mod 4 of the GLOBAL index) needs two Philox blocks per lane; the CLI's batches begin on a multiple.
//
// The deterministic part costs no 64 x 64 multiply per sample: per tile (uniform, scalar unit) A = P0 + Nt F + T(Nt) D and the step
// W = F + Nt D at the tile's first sample Nt; a lane at k = 4 lane starts from A + k W + T(k) D and steps Phi += w, w += D.
#include "../../include/galsynth.h"

#define GAL_GAUSS_DEVICE_TABLE
#define GAL_INTERF_DEVICE_TABLE
#include "iq_dev.h"

namespace {

// tests/osc_model.py repeats kTile (4 x iq_dev.h's kThreads) and kMaxBlocks as TILE and MAX_BLOCKS: the GPU tests place their lengths at these edges
constexpr int kTile = 4 * kThreads;
constexpr int kMaxBlocks = 2048;  // 8 blocks of 4 waves per CU, the rest by the grid-stride loop over the tiles
constexpr int kScanThreads = 1024;
static_assert((long long)kTile * 25960 * 7 < (1ll << 31), "a tile's sum of z stays far inside an int32");

struct OscArgs {
    uint64_t n1;  // the global index of the call's first sample
    uint64_t n0;  // N0: z(N0) is not part of Z
    uint64_t p0, f, d, s;
    uint32_t k0, k1, stream;
};

// the z of the samples 4 v .. 4 v + 3 of a call of n samples; 0 for a sample behind the call's end and for the sample N0
__device__ __forceinline__ void lane_z(const OscArgs &p, uint64_t v, uint64_t n, const uint32_t *gt, int (&z)[4])
{
    const uint64_t j0 = p.n1 + 4 * v;
    const uint32_t ph = (uint32_t)p.n1 & 3u;  // (uniform) where in its Philox block the lane's first sample lies
    uint32_t a[4], u[4];
    philox(j0 >> 2, p.k0, p.k1, p.stream, 1u, a);
    if (ph == 0) {
        u[0] = a[0], u[1] = a[1], u[2] = a[2], u[3] = a[3];
    } else {
        uint32_t b[4];
        philox((j0 >> 2) + 1, p.k0, p.k1, p.stream, 1u, b);
        if (ph == 1) {
            u[0] = a[1], u[1] = a[2], u[2] = a[3], u[3] = b[0];
        } else if (ph == 2) {
            u[0] = a[2], u[1] = a[3], u[2] = b[0], u[3] = b[1];
        } else {
            u[0] = a[3], u[1] = b[0], u[2] = b[1], u[3] = b[2];
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) z[m] = (4 * v + m < n && j0 + m != p.n0) ? gauss_q12(u[m], gt) : 0;
}

// sums: one word per tile of the call
__global__ __launch_bounds__(kThreads) void k_osc_tilesum(uint64_t n, OscArgs p, int *__restrict__ sums)
{
    __shared__ int part[2][kThreads / 64];
    const uint32_t *gt = load_gauss_table();
    const uint64_t nt = (n + kTile - 1) / kTile;
    int par = 0;
    for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x, par ^= 1) {
        int z[4];
        lane_z(p, t * kThreads + threadIdx.x, n, gt, z);
        int s = z[0] + z[1] + z[2] + z[3];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if ((threadIdx.x & 63) == 0) part[par][threadIdx.x >> 6] = s;
        __syncthreads();  // (part[] alternates: a lane still reading trip i's sums is at most one barrier behind)
        if (threadIdx.x == 0) sums[t] = part[par][0] + part[par][1] + part[par][2] + part[par][3];
    }
}

// one block: pre[t] = *st_in + sums[0] + ... + sums[t - 1]; *st_out = *st_in + the sum of all nt tiles
__global__ __launch_bounds__(kScanThreads) void k_osc_scan(const int *__restrict__ sums, uint64_t nt, const long long *__restrict__ st_in,
                                                           long long *__restrict__ st_out, long long *__restrict__ pre)
{
    __shared__ long long wtot[kScanThreads / 64];
    const uint64_t c = (nt + kScanThreads - 1) / kScanThreads;  // tiles per lane, consecutive
    const uint64_t a0 = (uint64_t)threadIdx.x * c, a = a0 < nt ? a0 : nt, b = a + c < nt ? a + c : nt;
    long long own = 0;
    for (uint64_t i = a; i < b; ++i) own += sums[i];
    long long incl = own;
    const int wl = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long up = __shfl_up(incl, o, 64);
        if (wl >= o) incl += up;
    }
    if (wl == 63) wtot[w] = incl;
    __syncthreads();
    long long run = *st_in + incl - own;
    for (int k = 0; k < w; ++k) run += wtot[k];
    for (uint64_t i = a; i < b; ++i) {
        pre[i] = run;
        run += sums[i];
    }
    if (threadIdx.x == kScanThreads - 1) *st_out = run;  // (the last lane's tiles end at nt, or it has none: everything in front of it)
}

// the complex sample x (I in the low half) turned by the phase Phi; `sat` counts the samples a clamp changes
__device__ __forceinline__ uint32_t rotate(int x, uint64_t Phi, const int16_t *cosl, uint32_t &sat)
{
    const uint32_t t = (uint32_t)(Phi >> 32) + (1u << 21);
    const uint32_t i = t >> 22;
    const int e = (int)((t >> 10) & 4095u) - 2048;
    const int c0 = cosl[i], s0 = cosl[(i - 256u) & 1023u];
    const int c = c0 - ((s0 * e * 101 + (1 << 25)) >> 26), s = s0 + ((c0 * e * 101 + (1 << 25)) >> 26);
    const int xI = (int16_t)x, xQ = x >> 16;
    const int vI = (xI * c - xQ * s + 2048) >> 12, vQ = (xI * s + xQ * c + 2048) >> 12;
    const int yI = clamp16(vI), yQ = clamp16(vQ);
    sat += (uint32_t)((yI != vI) | (yQ != vQ));
    return ((uint32_t)yI & 0xffffu) | ((uint32_t)yQ << 16);
}

// N (N - 1) / 2 mod 2^64
__device__ __forceinline__ uint64_t tri64(uint64_t N) { return (N & 1u) ? N * ((N - 1) >> 1) : (N >> 1) * (N - 1); }

// n >= 1 complex samples at `in` -> `out`, both 16-byte aligned, the same buffer or disjoint (a lane reads its vector before it writes
// it and no other lane touches it); pre: k_osc_scan's word per tile (kNoise only)
template <bool kNoise>
__global__ __launch_bounds__(kThreads) void k_iq_osc(const int16_t *in, int16_t *out, uint64_t n, OscArgs p, const long long *__restrict__ pre,
                                                     unsigned long long *sat)
{
    const int16_t *cosl = load_cos_table();
    __shared__ int wtot[2][kThreads / 64];
    const uint32_t *gt = nullptr;
    if constexpr (kNoise) gt = load_gauss_table();
    const uint64_t nt = (n + kTile - 1) / kTile, nfull = n >> 2;
    const int wl = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t k = 4u * threadIdx.x;  // the lane's first sample inside its tile
    uint32_t cnt = 0;
    int par = 0;
    for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x, par ^= 1) {
        const uint64_t v = t * kThreads + threadIdx.x;  // the lane's vector: the samples 4 v .. 4 v + 3 of the call
        const uint64_t Nt = p.n1 + t * kTile;           // (uniform) the global index of the tile's first sample
        const uint64_t A = p.p0 + Nt * p.f + tri64(Nt) * p.d, W = p.f + Nt * p.d;
        uint64_t phi = A + (uint64_t)k * W + (uint64_t)((k >> 1) * (k - 1u)) * p.d;  // (k is even: T(k) = (k / 2)(k - 1) < 2^19)
        uint64_t w = W + (uint64_t)k * p.d;
        int z[4] = {0, 0, 0, 0};
        long long zs = 0;  // Z at the sample in front of the lane's first
        if constexpr (kNoise) {
            lane_z(p, v, n, gt, z);
            const int own = z[0] + z[1] + z[2] + z[3];
            int incl = own;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(incl, o, 64);
                if (wl >= o) incl += up;
            }
            if (wl == 63) wtot[par][wv] = incl;
            __syncthreads();  // (wtot[] alternates: a lane still reading trip i's totals is at most one barrier behind)
            int ex = incl - own;
#pragma unroll
            for (int q = 0; q < kThreads / 64; ++q) ex += q < wv ? wtot[par][q] : 0;
            zs = pre[t] + ex;
        }
        if (4 * v < n) {
            const bool whole = v < nfull;
            v4i x = {0, 0, 0, 0};
            if (whole) {
                x = ((const v4i *)in)[v];
            } else {  // the call's last one to three samples
#pragma unroll
                for (int m = 0; m < 3; ++m)
                    if (4 * v + m < n) x[m] = ((const int *)in)[4 * v + m];
            }
            v4i y;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                uint64_t Phi = phi;
                if constexpr (kNoise) {
                    zs += z[m];
                    Phi += p.s * (uint64_t)zs;
                }
                y[m] = (int)rotate(x[m], Phi, cosl, cnt);  // (a sample behind the call's end is 0 and stays 0: it counts nothing)
                phi += w;
                w += p.d;
            }
            if (whole) {
                ((v4i *)out)[v] = y;
            } else {
#pragma unroll
                for (int m = 0; m < 3; ++m)
                    if (4 * v + m < n) ((int *)out)[4 * v + m] = y[m];
            }
        }
    }
    add_block_count<kThreads>(cnt, sat);
}

}  // namespace

// The bytes of a call's scratch -- one 64-bit word, then one 32-bit word per tile -- for a call of n >= 1 samples.  Host only.
extern "C" uint64_t galk_osc_scratch_bytes(uint64_t n)
{
    const uint64_t nt = (n + kTile - 1) / kTile;
    return 12 * nt;
}

// n >= 1 samples (< 2^41) whose first has the global index first_sample; n0 = N0 of the definition; state_in / state_out: one 64-bit
// word each, scratch: galk_osc_scratch_bytes, 8-byte aligned -- none of the three is touched where p->s == 0.  Arguments are checked
// by the caller (iq_api.cpp: gal_synth_iq_osc).
extern "C" hipError_t galk_launch_iq_osc(const int16_t *in, int16_t *out, uint64_t n, uint64_t first_sample, uint64_t n0, const gal_iq_osc_t *p,
                                         const long long *state_in, long long *state_out, void *scratch, unsigned long long *sat, hipStream_t st)
{
    OscArgs a;
    a.n1 = first_sample;
    a.n0 = n0;
    a.p0 = p->p0;
    a.f = (uint64_t)p->f;
    a.d = (uint64_t)p->d;
    a.s = p->s;
    a.k0 = (uint32_t)p->seed;
    a.k1 = (uint32_t)(p->seed >> 32);
    a.stream = p->stream;
    const uint64_t nt = (n + kTile - 1) / kTile;
    const unsigned grid = nt > (uint64_t)kMaxBlocks ? (unsigned)kMaxBlocks : (unsigned)nt;
    if (p->s == 0) {
        hipLaunchKernelGGL(k_iq_osc<false>, dim3(grid), dim3(kThreads), 0, st, in, out, n, a, (const long long *)nullptr, sat);
        return hipGetLastError();
    }
    long long *pre = (long long *)scratch;
    int *sums = (int *)(pre + nt);
    hipLaunchKernelGGL(k_osc_tilesum, dim3(grid), dim3(kThreads), 0, st, n, a, sums);
    hipLaunchKernelGGL(k_osc_scan, dim3(1), dim3(kScanThreads), 0, st, (const int *)sums, nt, state_in, state_out, pre);
    hipLaunchKernelGGL(k_iq_osc<true>, dim3(grid), dim3(kThreads), 0, st, in, out, n, a, (const long long *)pre, sat);
    return hipGetLastError();
}
