// iq_scint.hip -- per-satellite ionospheric scintillation (include/galsynth.h: gal_synth_iq_scint): ONE part of
// the sum times a slowly varying complex factor z.  x[n] = the complex int16 sample with the global index N = first_sample + n; z is a
// fixed integer function of (row, N): no state, any cut of the stream into calls gives the same bytes.
//
//   g(i)   = (gI, gQ) = the Q12 Gaussians of iq_dev.h of the words 0 and 1 of Philox4x32-10(counter = (i lo, i hi, stream, 2), key = seed)
//   node j:  S = sum_t h[t] g(j + t) (int64, t < 32, h = csrc/scint_table.inc);  X = (S + 2^14) >> 15
//            ZI[j] = clamp(A + ((B XI + 2048) >> 12), +-32767);  ZQ[j] = clamp((B XQ + 2048) >> 12, +-32767)
//   sample:  j = N div L, m = N mod L, fr = (m R) >> 20 with R = floor(2^32 / L)             (Q12, 0 .. 4095)
//            z = Z[j] + (((Z[j + 1] - Z[j]) fr + 2048) >> 12)                                (I and Q alike)
//            yI = clamp16((xI zI - xQ zQ + 2048) >> 12);  yQ = clamp16((xI zQ + xQ zI + 2048) >> 12)
//
// A complex sample counts once as saturated if either clamp changed it.  Integer arithmetic only (tests/scint_model.py states it in
// numpy).  |h g| <= 12211 x 25960 < 2^29 (an int32 product, summed in 64 bits); |X| < 2^17, B <= 4096: B X fits an int32; |Z| <= 32767 so
// |(Z[j + 1] - Z[j]) fr| < 2^28 and |xI zI - xQ zQ| + 2048 <= 2 x 32768 x 32767 + 2048 < 2^31.
//
// One launch for all jobs of a call: blockIdx.y = the job, blockIdx.x strides over the job's TILES of kTile = 1024 consecutive samples
// (a block of 256 lanes, four consecutive samples per lane, 16-byte loads and stores).  Nodes are computed once per tile, never per
// sample: a tile whose first sample lies m0 samples behind node j0 needs the nodes j0 .. j0 + (m0 + 1023) div L + 1 -- at most 18 with
// L >= 64 -- and those need at most 18 + 31 = 49 draws.  Lane d < 49 makes the draw j0 + d (one Philox block gives gI and gQ) into LDS;
// behind a barrier lane q < 36 sums the 32 taps of component q & 1 of node q >> 1; behind a second barrier every lane turns its four
// samples, stepping (j, m) from one 32-bit division per lane -- so a node boundary may fall anywhere inside a vector, and a
// first_sample that is no multiple of four costs nothing.  The only 64-bit division is that of a block's first tile; from tile to tile
// (j0, m0) advance by the constant (stride div L, stride mod L).  B = 0 (z = A, the identity at A = 4096) skips draws and sums.
#include "../../include/galsynth.h"

#define GAL_GAUSS_DEVICE_TABLE
#include "iq_dev.h"
#include "scint_table.inc"

namespace {

// tests/scint_model.py repeats kTile and kMaxBlocks as TILE and MAX_BLOCKS: the GPU tests place their lengths at these edges
constexpr int kTile = 4 * kThreads;
constexpr int kMaxBlocks = 2048;   // blocks of one call, all jobs together; the rest by the grid-stride loop over a job's tiles
constexpr int kMaxNodes = 18;      // (L - 1 + kTile - 1) div L + 2 at L = 64
constexpr int kMaxDraws = kMaxNodes + 31;
static_assert(kMaxDraws <= 64 && 2 * kMaxNodes <= 64, "draws and node sums are the work of the block's first wave");
static_assert((63 + kTile - 1) / 64 + 2 == kMaxNodes, "the node count of a tile at the smallest L");

// one job as the kernel reads it (iq_api.cpp fills the table; 64 bytes)
struct ScintJob {
    const int16_t *in;
    int16_t *out;
    uint64_t n;      // complex samples, >= 1
    uint64_t first;  // the global index of the job's first sample
    uint32_t k0, k1, stream;
    uint32_t L, R;   // node_len and floor(2^32 / L)
    int A, B;
    uint32_t pad;
};
static_assert(sizeof(ScintJob) == 64, "iq_api.cpp fills the same 64 bytes");

typedef const __attribute__((address_space(1))) v4i *gv4i_in;
typedef const __attribute__((address_space(1))) int *gint_in;
typedef __attribute__((address_space(1))) v4i *gv4i_out;
typedef __attribute__((address_space(1))) int *gint_out;

// the complex sample x (I in the low half) times (zI, zQ) in Q12; `sat` counts the samples a clamp changes
__device__ __forceinline__ uint32_t scale(int x, int zI, int zQ, uint32_t &sat)
{
    const int xI = (int16_t)x, xQ = x >> 16;
    const int vI = (xI * zI - xQ * zQ + 2048) >> 12, vQ = (xI * zQ + xQ * zI + 2048) >> 12;
    const int yI = clamp16(vI), yQ = clamp16(vQ);
    sat += (uint32_t)((yI != vI) | (yQ != vQ));
    return ((uint32_t)yI & 0xffffu) | ((uint32_t)yQ << 16);
}

// jobs[blockIdx.y]: in and out 16-byte aligned, the same buffer or disjoint (a lane reads its vector before it writes it and no other
// lane touches it); no job's output meets another job's buffers
__global__ __launch_bounds__(kThreads) void k_iq_scint(const ScintJob *__restrict__ jobs, unsigned long long *sat)
{
    __shared__ int g[2][kMaxDraws + 15];   // (the draws a tile needs; padded so that a clamped index stays inside)
    __shared__ int2 node[kMaxNodes + 2];   // (Z of the tile's nodes; a lane's last step may look one entry further than it uses)
    const uint32_t *gt = load_gauss_table();
    const ScintJob jb = jobs[blockIdx.y];
    const uint64_t n = jb.n, nt = (n + kTile - 1) / kTile, nfull = n >> 2;
    const uint32_t L = jb.L;
    const gv4i_in in4 = (gv4i_in)jb.in;
    const gint_in in1 = (gint_in)jb.in;
    const gv4i_out out4 = (gv4i_out)jb.out;
    const gint_out out1 = (gint_out)jb.out;
    // (uniform) the tile's first sample lies m0 samples behind node j0; from trip to trip both advance by the stride
    const uint64_t N0 = jb.first + (uint64_t)blockIdx.x * kTile;
    uint64_t j0 = N0 / L;
    uint32_t m0 = (uint32_t)(N0 - j0 * L);
    const uint32_t stride = gridDim.x * (uint32_t)kTile, sj = stride / L, sm = stride - sj * L;
    uint32_t cnt = 0;
    for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
        const uint32_t nn = (m0 + (uint32_t)kTile - 1) / L + 2;  // (uniform) nodes of this tile, <= kMaxNodes
        if (jb.B != 0) {
            if (threadIdx.x < nn + 31) {
                uint32_t w[4];
                philox(j0 + threadIdx.x, jb.k0, jb.k1, jb.stream, 2u, w);
                g[0][threadIdx.x] = gauss_q12(w[0], gt);
                g[1][threadIdx.x] = gauss_q12(w[1], gt);
            }
            __syncthreads();  // (the lanes that still read node[] of the trip before are in front of this barrier)
            if (threadIdx.x < 2 * nn) {
                const int c = threadIdx.x & 1, q = threadIdx.x >> 1;
                long long s = 0;
#pragma unroll
                for (int k = 0; k < 32; ++k) s += (long long)kScintH[k] * g[c][q + k];
                const int X = (int)((s + (1 << 14)) >> 15);
                const int Z = (c ? 0 : jb.A) + ((jb.B * X + 2048) >> 12);
                const int Zc = min(max(Z, -32767), 32767);
                if (c)
                    node[q].y = Zc;
                else
                    node[q].x = Zc;
            }
        } else {
            __syncthreads();
            if (threadIdx.x < nn) node[threadIdx.x] = make_int2(min(jb.A, 32767), 0);
        }
        __syncthreads();
        const uint64_t v = t * kThreads + threadIdx.x;  // the lane's vector: the samples 4 v .. 4 v + 3 of the job
        if (4 * v < n) {
            const bool whole = v < nfull;
            v4i x = {0, 0, 0, 0};
            if (whole) {
                x = in4[v];
            } else {  // the job's last one to three samples
#pragma unroll
                for (int m = 0; m < 3; ++m)
                    if (4 * v + m < n) x[m] = in1[4 * v + m];
            }
            const uint32_t mm = m0 + 4u * threadIdx.x;
            uint32_t dj = mm / L, r = mm - dj * L;
            int2 za = node[dj], zb = node[dj + 1];
            v4i y;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int fr = (int)((r * jb.R) >> 20);
                const int zI = za.x + (((zb.x - za.x) * fr + 2048) >> 12), zQ = za.y + (((zb.y - za.y) * fr + 2048) >> 12);
                y[m] = (int)scale(x[m], zI, zQ, cnt);  // (a sample behind the job's end is 0 and stays 0: it counts nothing)
                if (++r == L) {
                    r = 0;
                    ++dj;
                    za = zb;
                    zb = node[dj + 1];
                }
            }
            if (whole) {
                out4[v] = y;
            } else {
#pragma unroll
                for (int m = 0; m < 3; ++m)
                    if (4 * v + m < n) out1[4 * v + m] = y[m];
            }
        }
        j0 += sj;
        m0 += sm;
        if (m0 >= L) {
            m0 -= L;
            j0 += 1;
        }
    }
    add_block_count<kThreads>(cnt, sat);
}

}  // namespace

extern "C" const int32_t *gal_tables_scint(void) { return kScintH; }

// jobs_dev: n_jobs >= 1 jobs of 64 bytes each as struct ScintJob lays them out (iq_api.cpp: gal_synth_iq_scint checks the arguments and
// fills the table); max_n = the longest job's samples.
extern "C" hipError_t galk_launch_iq_scint(const void *jobs_dev, int n_jobs, uint64_t max_n, unsigned long long *sat, hipStream_t st)
{
    const uint64_t nt = (max_n + kTile - 1) / kTile;
    const uint64_t cap = (uint64_t)kMaxBlocks / (uint64_t)n_jobs;  // n_jobs <= 64: at least 32
    const unsigned bx = (unsigned)(nt < 1 ? 1 : nt > cap ? cap : nt);
    hipLaunchKernelGGL(k_iq_scint, dim3(bx, (unsigned)n_jobs), dim3(kThreads), 0, st, (const ScintJob *)jobs_dev, sat);
    return hipGetLastError();
}
