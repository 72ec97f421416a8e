/*
 * galsynth.h -- C ABI of the MI355X Galileo E1B/C baseband IQ synthesis engine.
 *
 * This is the drop-in boundary for the reference's per-sample hot loop.  The reference
 * (harshadms/galileo-sdr-sim) exposes no plugin/FFI interface for this path: the loop is inline in
 * galileo_task() at src/galileo-sdr.cpp:481-539.  The entry points below are what a maintainer
 * would call where that loop stands: everything the loop READS is carried by
 * gal_chan_epoch_t / gal_chan_state_t, everything it WRITES is the interleaved int16 IQ buffer
 * (src/galileo-sdr.cpp:536-537, the `ishort` wire format of gnss-sdr_Galileo_E1_ishort.conf:14-21)
 * plus the per-channel state that survives an epoch (carr_phase and page, §7.3-3 of SURVEY.md).
 *
 * Plain C, plain pointers and sizes; no torch / HIP types in the signatures (a hipStream_t is passed
 * as void*).  One handle per GPU/stream; a handle is thread-compatible, not thread-safe.
 * All functions return GAL_OK (0) or a negative gal_status_t; gal_synth_last_error() gives text.
 */
#ifndef GALSYNTH_H_
#define GALSYNTH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GAL_MAX_CHAN 16          /* reference MAX_CHAN, include/constants.h:10 (engine accepts up to 64) */
#define GAL_ENGINE_MAX_CHAN 64   /* packed I/Q accumulation stays inside int16 up to 65 channels       */
#define GAL_N_SYM_PAGE 500       /* symbols per page, include/constants.h:34                            */
#define GAL_PAGE_WORDS 16        /* 500 symbols, bit i of word i>>5 (LSB first) = symbol i              */
#define GAL_CODE_LEN 4092        /* CA_SEQ_LEN_E1, include/constants.h:124                              */
#define GAL_NUM_PRN 50

typedef enum gal_status {
    GAL_OK = 0,
    GAL_E_INVAL = -1,     /* bad argument                                                   */
    GAL_E_NOMEM = -2,     /* host or device allocation failed                               */
    GAL_E_DEVICE = -3,    /* HIP runtime error / no usable GPU (there is NO CPU fallback)   */
    GAL_E_STATE = -4,     /* call sequence error (execute before plan, ...)                 */
    GAL_E_CHAIN = -5,     /* NCO chain self-check failed (see gal_synth_stats_t)            */
    GAL_E_IO = -6,
    GAL_E_BUSY = -7,      /* a resource another instance holds (galscen: the UDP position port)   */
    GAL_E_EMPTY = -8      /* galscen: the duration holds no epoch, (int)(10 d + 0.5) < 2: nothing to generate (the reference
                             opens its sink and closes it again, src/galileo-sdr.cpp:438)        */
} gal_status_t;

/* gal_chan_epoch_t.flags */
#define GAL_CH_RESTART 1u /* channel (re)allocated before this epoch: carrier phase := carr_phase0, page := page_init
                             (src/channel.cpp:81-99) */

/*
 * What the hot loop reads for ONE channel slot in ONE 0.1 s epoch -- the values
 * computeCodePhase() (src/gal-sig.cpp:308-347) leaves in channel_t (include/structures.h:140-162)
 * right before `for (isamp...)` (src/galileo-sdr.cpp:481), plus the two pages the loop may use.
 */
typedef struct gal_chan_epoch {
    int32_t  prn;          /* 1..50; 0 = idle slot (chan[i].prn, src/galileo-sdr.cpp:489)                      */
    int32_t  ibit0;        /* chan.ibit at epoch start, 0..499 (src/gal-sig.cpp:334,338)                         */
    uint32_t flags;        /* GAL_CH_*                                                                           */
    uint32_t reserved;
    double   f_carr;       /* Hz, chan.f_carr (src/gal-sig.cpp:318); |f_carr| < sample_rate                     */
    double   f_code;       /* Hz, chan.f_code (src/gal-sig.cpp:320); 2^-20 <= f_code / sample_rate <= 0.5      */
    double   code_phase0;  /* chips, chan.code_phase at epoch start (src/gal-sig.cpp:336), in [0, 6138)         */
    double   carr_phase0;  /* cycles; used only with GAL_CH_RESTART (src/channel.cpp:98-99)                     */
    uint32_t page_next[GAL_PAGE_WORDS]; /* page generateINavMsg(grx_of_this_epoch) would produce: installed when
                                           ibit wraps 499->0 inside this epoch (src/galileo-sdr.cpp:497-506)    */
    uint32_t page_init[GAL_PAGE_WORDS]; /* page in force at epoch start; used only with GAL_CH_RESTART          */
} gal_chan_epoch_t;        /* 176 bytes */

/* State that survives an epoch (and a call): carr_phase and the current page, per slot. */
typedef struct gal_chan_state {
    double   carr_phase;               /* chan.carr_phase after the last sample (src/galileo-sdr.cpp:531-532) */
    uint32_t page[GAL_PAGE_WORDS];     /* chan.page                                                            */
    int32_t  prn;                      /* PRN the state belongs to (0 = none)                                   */
    int32_t  reserved;
} gal_chan_state_t;        /* 80 bytes */

typedef struct gal_synth_cfg {
    double  sample_rate;        /* Hz; reference: 2.6e6 (include/constants.h:96). delt = 1.0 / sample_rate     */
    int32_t samples_per_epoch;  /* reference: NUM_IQ_SAMPLES = 260000 (include/constants.h:82)                 */
    int32_t n_slots;            /* channel slots per epoch record row; reference MAX_CHAN = 16                 */
    int32_t device;             /* HIP device ordinal; -1 = current device                                     */
    int32_t chunk_samples;      /* 0 = auto (~1024); samples replayed by one lane (multiple of 4)              */
    int32_t max_walk_passes;    /* 0 = default (64 + carrier legs in the plan); cap on speculative carrier-walk
                                   passes before gal_synth_finish gives up with GAL_E_CHAIN                    */
    uint32_t flags;             /* GAL_CFG_*                                                                   */
    int32_t reserved[2];
} gal_synth_cfg_t;

/* gal_synth_cfg_t.flags */
#define GAL_CFG_CBOC 2u          /* opt-in: CBOC(6,1,1/11), the composite sub-carrier of the E1 OS ICD, instead of the
                                    BOC(1,1) the reference generates (src/gal-sig.cpp:198-233; the reference has no such
                                    mode).  Definition, per channel and sample, with x = code phase in chips,
                                    B = E1B chip x data symbol, C = E1C chip x secondary code (all +-1), sc_A = +1 if
                                    (int)(2 x) is odd else -1 (the reference's sboc convention), sc_B likewise from
                                    (int)(12 x), k = ((int)(511 carr_phase)) & 511:
                                        I += sc_A (B - C) TAcos[k] + sc_B (B + C) TBcos[k]      (Q with the sin tables)
                                    TA = lround(sqrt(10/11) x cosTable512 / sinTable512), TB = lround(sqrt(1/11) x ...);
                                    everything else (wrap, symbol, page, NCO updates, int16 store) as src/galileo-sdr.cpp:481-539 */
#define GAL_CFG_EXACT_REPLAY 4u  /* always synthesise with the exact-replay kernel (every lane steps the reference's two NCO
                                    recurrences sample by sample and checks its end state against the next checkpoint), also where
                                    the default kernel of the reference geometry -- 16-sample groups from closed-form start
                                    states, undecided groups replayed exactly -- could run.  Same bits either way; this one is
                                    slower and carries the replay self-check (gal_synth_stats_t.kernel_family says which ran) */
#define GAL_CFG_VERIFY_ALL 8u    /* accepted and ignored: what it asked for is the default since 0.4 (see GAL_CFG_VERIFY_SAMPLED)     */
#define GAL_CFG_VERIFY_SAMPLED 16u /* batches of the default kernel (kernel_family 1), which never forms an exact phase itself.  DEFAULT
                                    (flag clear): every carrier leg and every code leg of the executed epochs is walked once more from
                                    its own first checkpoint, genuinely, in every batch, and every checkpoint must come out bit for
                                    bit (k_verify) -- what the exact-replay kernel establishes on its way.
                                    Flag set (round 5's default; ~3-5 % less per step): an eighth of the leg positions of both
                                    chains per batch, rotating with the handle's batch count -- every (epoch, leg) position of a
                                    repeated plan is re-walked once per N = 8 batches --, plus every carrier leg whose translation
                                    used more than 1/256 of its margin, plus the chunks k_repair_g walks to their ends.  A wrong
                                    translation (a proof would have to be wrong) is then caught within 8 batches instead of in
                                    the batch it happens in                                                  */
#define GAL_CFG_SINGLE_STREAM 1u /* enqueue every kernel on the handle's stream (no internal high-priority walker
                                    streams): for callers that capture or serialise the stream themselves       */

typedef struct gal_synth_stats {
    int32_t walk_passes;        /* carrier-walker passes the last execute needed                               */
    int32_t chain_mismatch;     /* #chunk boundaries where the replay kernel disagreed with the walker (must be 0) */
    int32_t n_epochs;
    int32_t n_active_max;       /* max simultaneously active channels in the plan                              */
    int32_t chunk_samples;
    int32_t chunks_per_epoch;
    float   ms_walk;            /* device time of the walker kernels, last execute (0 if timing disabled)      */
    float   ms_synth;           /* device time of the synthesis kernel, last execute                           */
    int32_t window_mode;        /* fast body of the synthesis kernel: 1 / 2 / 3 / 4 resampled windows (one chip-pattern look-up
                                   per 16 samples; 1: 0.74 <= 2 f_code / fs < 1, as at the reference's 2.6 MS/s; 2: 2 f_code / fs
                                   <= 0.133, sample rates from 15.4 MS/s; 3: <= 0.266, from 7.7 MS/s; 4: what lies between,
                                   2.77 .. 7.7 MS/s (kernel_family 1 only); all need well separated pattern thresholds --
                                   a rate at which 2 f_code / fs is within 1e-3 of a fraction with a denominator up to 15,
                                   e.g. 4.092 MS/s, has none on the exact-replay kernel), 0 per-sample window index (any rate).
                                   + 16 (0.4, kernel_family 1): the thresholds crowd and a group's pattern was found by bisection
                                   over them instead of through the bin table.  Same bits either way.                       */
    int32_t synth_runs;         /* synthesis launches the last batch took: 1, or 2 when gal_synth_finish() had to repeat
                                   it (carrier chain not complete when the kernel was started, or the replay check failed) */
    int32_t kernel_family;      /* 0: exact replay, one chunk of ~1000 samples per lane (any rate, any signal); 1: one 16-sample
                                   group per lane, start states in closed form from the chunk's exact checkpoint, groups whose
                                   chip pattern or table index hangs on the rounding history replayed exactly afterwards -- the
                                   default wherever gal_synth_plan's gate admits the batch: automatic chunking, every code step
                                   in one form of the resampled windows (window_mode 1 ... 4: any rate from 2.05 MS/s up; pattern
                                   thresholds that crowd -- 4.092, 8.184 MS/s ... -- are searched by bisection since 0.4, BOC(1,1)
                                   only), every carrier step 0 or in [2^-40, 0.0147] cycles per sample;
                                   BOC(1,1) and the CBOC mode in all four forms                                              */
    int32_t repaired_groups;    /* family 1: 16-sample groups that were replayed exactly (about 1 in 10 000)                */
    float   ms_repair;          /* family 1: device time of that replay (k_repair_g, behind the synthesis kernel; not in ms_synth) */
    int32_t exact_records;      /* family 1: records (channel-epochs) of the batch that are not fit for the group kernel -- a carrier
                                   that stands still or is faster than 120 table entries per 16 samples, pattern thresholds that
                                   crowd, another window form than the batch's -- and took an accumulating exact-replay launch
                                   behind it (0 in every scenario of the reference's geometry seen so far)                      */
    float   ms_plan;            /* 0.4: host time of the gal_synth_plan[_async] call behind this batch (validation, lists, staging)    */
    float   ms_h2d;             /* 0.4: device time of its host->device copy (one copy of the SoA records out of pinned memory)        */
} gal_synth_stats_t;
/* The struct only ever GROWS AT ITS END (0.2: 40 bytes, walk_passes .. synth_runs; 0.3: 56; 0.4: 64).  gal_synth_finish and
 * gal_synth_run_host are function-like macros over the _n entry points below, which copy min(the caller's sizeof, the library's)
 * bytes: a caller compiled against an older header never gets more than its own struct holds.  The plain SYMBOLS of those two
 * names stay exported for binaries built against 0.2 and fill exactly those 40 bytes.  Caveat of the macros: the two names cannot
 * be used as function pointers -- take &gal_synth_finish_n / &gal_synth_run_host_n (or define GAL_SYNTH_NO_SIZED_MACROS before
 * including this header and get the 40-byte symbols).  gal_synth_stats_size() = the library's sizeof. */

typedef struct gal_synth gal_synth_t;

/* Library / build identification; never fails. */
const char *gal_synth_version(void);
/* Text of the last error on this thread. */
const char *gal_synth_last_error(void);
/* Number of usable gfx950 devices (0 if none). */
int gal_synth_device_count(void);

int gal_synth_create(const gal_synth_cfg_t *cfg, gal_synth_t **out);
int gal_synth_destroy(gal_synth_t *h);

/* Use `hip_stream` (a hipStream_t) for all work of this handle; NULL = the handle's own stream. */
int gal_synth_set_stream(gal_synth_t *h, void *hip_stream);

/*
 * Upload the per-epoch parameters of a batch: params[e * n_slots + s], e < n_epochs (host memory).
 * state_in (host, n_slots entries, may be NULL for a fresh run) gives carr_phase/page for channels
 * that continue from a previous batch (records without GAL_CH_RESTART in their first active epoch).
 * After this call the batch is resident in HBM.  GAL_E_STATE while a batch is in flight (gal_synth_plan_async may be called then).
 */
int gal_synth_plan(gal_synth_t *h, const gal_chan_epoch_t *params, int32_t n_epochs,
                   const gal_chan_state_t *state_in);

/*
 * The same without waiting: the host work of the plan -- validation, lists, the SoA split into the handle's pinned staging buffer --
 * is done when it returns (`params` and `state_in` may be reused).
 *   - Nothing in flight on the handle: the upload is ENQUEUED on the handle's stream; the walkers of the next
 *     gal_synth_execute[_range] wait for it on the device.
 *   - A batch IN FLIGHT (gal_synth_execute called, gal_synth_finish not yet): allowed -- this is plan(k+1) under execute(k).  The
 *     plan is staged on the host only (the arena still belongs to the batch in flight); the next gal_synth_execute[_range], which
 *     must come behind the gal_synth_finish of that batch, makes it the handle's plan, enqueues the upload and goes on.  Until then
 *     gal_synth_finish / gal_synth_walk_counts speak of the batch in flight; gal_synth_output_bytes of the staged plan.
 * This is how a caller with fresh parameters for every batch -- the reference computes them between epochs,
 * src/galileo-sdr.cpp:450-479 -- keeps two handles busy: finish(A); execute(A); plan_async(A, the scenario after next), the same
 * for B (bench.py: configs.fresh_plan).  One thread at a time per handle.  Errors of the upload itself surface in
 * gal_synth_execute / gal_synth_finish.
 */
int gal_synth_plan_async(gal_synth_t *h, const gal_chan_epoch_t *params, int32_t n_epochs,
                         const gal_chan_state_t *state_in);

/* Bytes of IQ the planned batch produces: n_epochs * samples_per_epoch * 4. */
size_t gal_synth_output_bytes(const gal_synth_t *h);

/*
 * Run the hot path for the planned batch: NCO walk + per-sample synthesis, writing
 * interleaved int16 I,Q (little endian) to iq_dev (DEVICE memory, 16-byte aligned).  Asynchronous: the
 * walker chain runs on the handle's own high-priority streams and starts at once (its inputs were uploaded by
 * gal_synth_plan, which is synchronous; it does not wait for other work on the handle's stream), the synthesis kernel
 * runs in order on the handle's stream; may be called repeatedly for the same plan.  Several
 * handles may be in flight on different streams: the latency-bound walk of one batch then runs beside the
 * synthesis kernel of another (bench.py --pipeline).
 */
int gal_synth_execute(gal_synth_t *h, int16_t *iq_dev);

/*
 * The same for the epochs [first_epoch, first_epoch + n_epochs) of the planned batch only: iq_dev receives
 * n_epochs * samples_per_epoch * 4 bytes.  This is how ONE scenario is cut into contiguous epoch ranges for several GPUs
 * without any exchange (bench.py --shard scenario): every rank plans the whole scenario and executes its own range.
 * The carrier chain never restarts, so the NCO walk covers the epochs [0, first_epoch + n_epochs): those in front of the
 * range silently (their states are needed, their checkpoints are not), those behind it not at all -- a rank's walker
 * work grows with the prefix it needs, not with the plan.  gal_synth_finish then returns the channel state at the END OF
 * THE EXECUTED RANGE (= the end of the plan for a range that reaches it, in particular for gal_synth_execute).
 */
int gal_synth_execute_range(gal_synth_t *h, int16_t *iq_dev, int32_t first_epoch, int32_t n_epochs);

/* Wait for the batch (its completion record -- counters, end state, a sequence number -- is written by the device into
 * pinned host memory behind the synthesis kernel and polled here; work the caller has enqueued on the stream BEHIND
 * gal_synth_execute is not waited for), check the chain self-check, return the end-of-batch channel state (host,
 * n_slots entries, may be NULL) and statistics (may be NULL).  The IQ in iq_dev is FINAL ONLY AFTER THIS CALL HAS
 * RETURNED GAL_OK: the carrier chain is evaluated speculatively, and if the speculation was not verified in time
 * (or the replay check disagreed) finish() repeats the synthesis into iq_dev.  Do not enqueue copies out of
 * iq_dev between execute() and finish(). */
int gal_synth_finish(gal_synth_t *h, gal_chan_state_t *state_out, gal_synth_stats_t *stats);
int gal_synth_finish_n(gal_synth_t *h, gal_chan_state_t *state_out, void *stats, size_t stats_bytes);
size_t gal_synth_stats_size(void);

/* Diagnostics of the last gal_synth_finish(): carrier-chain legs evaluated by walking, legs accepted by
 * translation (csrc/nco_walk.h: binade_margin), and how often (since create) the replay check forced the
 * all-walked fallback.  Any pointer may be NULL. */
int gal_synth_walk_counts(const gal_synth_t *h, int64_t *legs_walked, int64_t *legs_translated, int64_t *fallbacks);

/* Convenience: plan + execute into an internal device buffer + copy to host `iq_host` + finish. */
int gal_synth_run_host(gal_synth_t *h, const gal_chan_epoch_t *params, int32_t n_epochs,
                       const gal_chan_state_t *state_in, int16_t *iq_host,
                       gal_chan_state_t *state_out, gal_synth_stats_t *stats);
int gal_synth_run_host_n(gal_synth_t *h, const gal_chan_epoch_t *params, int32_t n_epochs,
                         const gal_chan_state_t *state_in, int16_t *iq_host,
                         gal_chan_state_t *state_out, void *stats, size_t stats_bytes);
#ifndef GAL_SYNTH_NO_SIZED_MACROS
#define gal_synth_finish(h, state_out, stats) gal_synth_finish_n((h), (state_out), (stats), sizeof(gal_synth_stats_t))
#define gal_synth_run_host(h, params, n_epochs, state_in, iq_host, state_out, stats) \
    gal_synth_run_host_n((h), (params), (n_epochs), (state_in), (iq_host), (state_out), (stats), sizeof(gal_synth_stats_t))
#endif

/*
 * Output formats.  x[j] = the interleaved int16 stream gal_synth_execute writes (I0, Q0, I1, Q1, ...):
 *   GAL_IQ_ISHORT  x itself, 4 bytes per complex sample (the reference's format)
 *   GAL_IQ_IBYTE   out[j] = (int8) clamp((x[j] + r) >> shift, -127, 127), r = shift ? 1 << (shift - 1) : 0 (int32 arithmetic shift:
 *                  round to nearest), 2 bytes per complex sample; a value whose shifted v lies outside [-127, 127] is SATURATED
 *   GAL_IQ_IBIT    bit = x[j] > 0, byte k holds x[8k] .. x[8k+7] with x[8k] in bit 7 (MSB first: numpy.packbits(x > 0)), the unused
 *                  low bits of the last byte 0; ceil(n / 4) bytes for n complex samples; nothing saturates
 */
#define GAL_IQ_ISHORT 0
#define GAL_IQ_IBYTE 1
#define GAL_IQ_IBIT 2
/* Bytes that n_samples complex samples take in `format`: 4 n, 2 n, ceil(n / 4); 0 for an unknown format.  Needs no GPU. */
size_t gal_synth_iq_bytes(int32_t format, size_t n_samples);
/* Enqueue on the handle's stream: convert n_samples interleaved int16 complex samples at iq_dev into `format` at out_dev (both DEVICE
 * memory, 16-byte aligned, not overlapping; out_dev holds gal_synth_iq_bytes(format, n_samples) bytes).  iq_dev must be FINAL
 * output: enqueue this behind gal_synth_finish of the batch that wrote it (GAL_E_STATE for a buffer of the batch in flight).
 * shift: 0..15 for GAL_IQ_IBYTE, 0 otherwise.  GAL_IQ_ISHORT is a device copy.  Saturated values add to the handle's counter.
 * GAL_E_INVAL for a null handle, an unknown format, a bad shift, a null or misaligned pointer, input and output that overlap. */
int gal_synth_iq_convert(gal_synth_t *h, const int16_t *iq_dev, size_t n_samples, int32_t format, int32_t shift, void *out_dev);
/* Wait for the conversions enqueued so far (whatever their format: this is their fence); *n_saturated = int16 values saturated since create (or since the last reset);
 * reset != 0 sets the counter back to 0. */
int gal_synth_iq_saturated(gal_synth_t *h, uint64_t *n_saturated, int32_t reset);

/*
 * Noise floor (not in the reference, which writes the bare sum of the satellite signals): seeded white Gaussian noise and a signal
 * gain, mixed into the final int16 stream in front of the format conversion, in one pass on the device.  It is a FIXED INTEGER
 * FUNCTION of (seed, stream, index of the value in the whole output stream, int16 input): the same bits on any machine, however the
 * stream is cut into batches and calls (tests/noise_model.py states it in numpy).
 *
 * x[j] = the interleaved int16 stream of one call (I0, Q0, I1, Q1, ...), first_sample = the index, counted from the start of the
 * whole output stream, of the call's first complex sample.
 *   J   = 2 (first_sample + j / 2) + (j & 1), 64-bit: the global value index
 *   u   = output word J & 3 of Philox4x32-10 (Salmon et al., Random123: multipliers 0xD2511F53, 0xCD9E8D57, key increments
 *         0x9E3779B9, 0xBB67AE85, ten rounds) with B = J >> 2, counter = (B & 0xffffffff, B >> 32, stream, 0),
 *         key = (seed & 0xffffffff, seed >> 32)
 *   z   = Gaussian in Q12 (unit variance at 4096; tails to 6.3 sigma), an inverse CDF over octave segments, integers only:
 *         neg = u >> 31; w = u & 0x7fffffff; o = leading zeros of w as a 31-bit number (0..30; 31 for w = 0);
 *         wn = w << o (0 for w = 0); s = (wn >> 25) & 31; f = (wn >> 17) & 255; (a, b) = T[o][s];
 *         mag = a - (((a - b) f + 128) >> 8); z = neg ? -mag : mag
 *         T = gal_tables_gauss(): with q(v) = -Phi^-1(v / 2^32), T[o][s] = (round(4096 q(2^(30-o) (1 + s/32))),
 *         round(4096 q(2^(30-o) (1 + (s+1)/32)))) for o <= 30 and T[31][.] = (t0, t0), t0 = round(4096 q(0.5)) = 25960
 *   y[j] = clamp((int64(x[j]) G + int64(z) S + 32768) >> 16, -32768, 32767)   (arithmetic shift), G = gain_q16, S = sigma_q4
 * y then takes the format definitions above unchanged (GAL_IQ_ISHORT: y; GAL_IQ_IBYTE: shift, round, clamp to +-127;
 * GAL_IQ_IBIT: y > 0).  A value counts ONCE as saturated if either clamp changed it.  G = 65536, S = 0 gives y = x exactly.
 */
typedef struct gal_iq_noise {
    uint64_t seed;      /* Philox key                                                                                    */
    uint32_t stream;    /* Philox counter word 2: independent noise for the same seed (the CLI: the site index of --sites) */
    uint32_t gain_q16;  /* G = round(signal gain x 2^16), 0 .. 2^20                                                        */
    uint32_t sigma_q4;  /* S = round(noise sigma in int16 LSB x 2^4), 0 .. 2^20                                            */
    uint32_t reserved;  /* 0                                                                                             */
} gal_iq_noise_t;
/* gal_synth_iq_convert with the noise floor in front of the format: the same rules (enqueued on the handle's stream, behind
 * gal_synth_finish of the batch that wrote iq_dev, 16-byte alignment, overlap refused, gal_synth_iq_saturated as fence and counter),
 * and: GAL_IQ_ISHORT may run exactly IN PLACE (out_dev == iq_dev; any other overlap is refused); noise == NULL behaves as
 * gal_synth_iq_convert (first_sample is then not looked at); GAL_E_INVAL also for gain_q16 or sigma_q4 above 2^20, reserved != 0,
 * first_sample >= 2^62.  Any first_sample gives the defined output; an even one (every batch of whole epochs) is the fast case. */
int gal_synth_iq_convert_noise(gal_synth_t *h, const int16_t *iq_dev, size_t n_samples, uint64_t first_sample,
                               const gal_iq_noise_t *noise, int32_t format, int32_t shift, void *out_dev);
/* Noise parameters for a carrier-to-noise-density ratio; needs no GPU.  gain_q16 = round(gain 65536),
 * sigma_q4 = round(16 x 250 gain sqrt(sample_rate / 10^(cn0_dbhz / 10))); seed, stream and reserved are set to 0.
 * 250 is the carrier-table amplitude of ONE E1 component (gal_tables_cos512()[0]); a satellite's E1B and E1C components are
 * orthogonal in I/Q, each of power 250^2 per rail, and the noise has sigma^2 per rail: cn0_dbhz is the C/N0 of the COMPOSITE
 * E1B + E1C signal of one satellite.  E1B alone (what a data-channel tracker sees) is 3 dB lower.
 * GAL_E_INVAL for a null `out`, a non-finite argument, sample_rate <= 0, gain outside [0, 16], or a sigma_q4 above 2^20. */
int gal_synth_noise_from_cn0(double cn0_dbhz, double sample_rate, double gain, gal_iq_noise_t *out);

/*
 * Interference (not in the reference): up to GAL_INTERF_MAX sources -- a CW tone, a linear chirp that restarts every sweep_len samples
 * (a sawtooth in frequency, phase-continuous), either of them pulsed -- added behind the signal gain and in front of the ONE clamp to
 * int16, in the same pass as the noise floor.  Like the noise it is a FIXED INTEGER FUNCTION of (parameters, index of the value in the
 * whole output stream, int16 input): the same bits on any machine and for any cut into batches and calls (tests/interf_model.py states
 * it in numpy).
 *
 * N = first_sample + j / 2, 64-bit: the global index of the complex sample that value j belongs to.  All phase arithmetic is modulo 2^32.
 *   (s, m) = (0, N) for sweep_len = 0, otherwise (N div sweep_len, N mod sweep_len)
 *   W      = sweep_len f0 + df sweep_len (sweep_len - 1) / 2, the phase advance of one whole sweep
 *   phi(N) = ph0 + s W + m f0 + df (m (m - 1) / 2)            (sweep_len = 0: ph0 + N f0)
 *            = the recurrence phi(0) = ph0, phi(N + 1) = phi(N) + f0 + (N mod sweep_len) df.  m (m - 1) is even and below 2^64, hence
 *            exact in uint64; of s only the low 32 bits matter
 *   i      = phi >> 22;  C = gal_tables_cos1024(): C[k] = round(4096 cos(2 pi k / 1024)), int16 in Q12
 *   gate   = 1 if pulse_period = 0 or (N mod pulse_period) < pulse_on, else 0
 *   t[j]   = gate A C[i] for the I value (j even), gate A C[(i - 256) & 1023] for the Q value (the sine: a positive f0 is a positive
 *            frequency offset), A = amp_q4
 *   y[j]   = clamp((int64(x[j]) G + int64(z) S + sum over the sources of t[j] + 32768) >> 16, -32768, 32767)
 * with x, G, S, z exactly as the noise floor defines them (no noise: G = 65536, S = 0).  y then takes the three formats unchanged.  A
 * value counts ONCE as saturated if either clamp changed it.  With no sources this is gal_synth_iq_convert_noise bit for bit.
 */
#define GAL_INTERF_MAX 4
typedef struct gal_iq_interf {
    uint32_t amp_q4;        /* A = amplitude in int16 LSB x 16, 0 .. 2^20                                                     */
    uint32_t ph0;           /* phase at sample 0 of the whole output stream, 2^-32 cycles                                     */
    int32_t  f0;            /* phase step per sample at the start of a sweep, 2^-32 cycles (signed: +- sample_rate / 2)        */
    int32_t  df;            /* increment of the step per sample inside a sweep; must be 0 when sweep_len = 0                   */
    uint32_t sweep_len;     /* samples per sweep; 0 = never restarts (CW)                                                     */
    uint32_t pulse_period;  /* samples; 0 = always on                                                                         */
    uint32_t pulse_on;      /* <= pulse_period: on while (N mod pulse_period) < pulse_on                                      */
    uint32_t reserved;      /* 0                                                                                              */
} gal_iq_interf_t;          /* 32 bytes */
/* gal_synth_iq_convert_noise with n_interf sources added: every rule of that call holds (enqueued on the handle's stream, 16-byte
 * alignment, GAL_IQ_ISHORT may run exactly in place and any other overlap is refused, GAL_E_STATE for the buffer of the batch in flight,
 * gal_synth_iq_saturated as fence and counter, first_sample < 2^62).  noise may be NULL: G = 65536, S = 0, nothing random.  n_interf = 0
 * IS gal_synth_iq_convert_noise.  `interf` is copied before the call returns.  GAL_E_INVAL also for n_interf outside
 * 0..GAL_INTERF_MAX, a null `interf` with n_interf > 0, amp_q4 above 2^20, df != 0 with sweep_len = 0, pulse_on > pulse_period,
 * reserved != 0. */
int gal_synth_iq_convert_interf(gal_synth_t *h, const int16_t *iq_dev, size_t n_samples, uint64_t first_sample,
                                const gal_iq_noise_t *noise, const gal_iq_interf_t *interf, int32_t n_interf, int32_t format,
                                int32_t shift, void *out_dev);
/* A source for a jammer-to-signal ratio; needs no GPU.  J/S is stated against the same C as gal_synth_noise_from_cn0: the composite
 * E1B + E1C signal of ONE satellite has the total (both rails) power C = 2 (250 gain)^2 and a tone A e^(j theta) the total power A^2,
 * so   amp_q4 = round(16 x 250 sqrt(2) gain 10^(js_db / 20)).
 * f0 = llround(f_lo_hz / sample_rate x 2^32).  sweep_s = 0: CW (f_hi_hz is not looked at, sweep_len = 0, df = 0); otherwise
 * sweep_len = llround(sweep_s sample_rate) >= 1 and df = llround((f_hi_hz - f_lo_hz) / sample_rate x 2^32 / sweep_len).
 * pulse_period, pulse_on = llround(seconds x sample_rate); ph0 and reserved are set to 0.
 * GAL_E_INVAL for a null `out`, a non-finite argument, sample_rate <= 0, a negative gain, time or duration, |f| >= sample_rate / 2,
 * an amplitude beyond the 2^20 of amp_q4, a sweep that rounds to 0 samples, lengths beyond 32 bits, pulse_on > pulse_period. */
int gal_synth_interf_make(double js_db, double gain, double sample_rate, double f_lo_hz, double f_hi_hz, double sweep_s,
                          double pulse_period_s, double pulse_on_s, gal_iq_interf_t *out);

/*
 * Per-satellite signal power (opt-in; the reference computes a gain per channel and epoch, src/galileo-sdr.cpp:469-477, and leaves it
 * commented out in its loop, :520-521: without these calls every satellite leaves the engine at the carrier-table amplitude of 250 and
 * every byte is the reference's).  Like the formats it is a FIXED INTEGER FUNCTION of its inputs (tests/gain_model.py states it in
 * numpy).
 *
 * x_s[j] = the interleaved int16 stream the engine writes for a batch when only the records of slot s are active (every other slot
 * with prn = 0; the carrier state of slot s as in the full run).  The engine's plain output is exactly sum_s x_s[j]: the accumulation
 * is in integers and stays inside int16.  g[e][s] = the gain of slot s in epoch e, Q7 in a uint16, 0 .. GAL_GAIN_MAX, GAL_GAIN_UNITY
 * = 128 = 1.0 (the reference's "scaled by 2^7"), constant within an epoch like everything else the loop reads.  With
 * e(j) = (j / 2) / samples_per_epoch:
 *   w[j] = sum_s int32(g[e(j)][s]) x_s[j]
 *   y[j] = clamp((w[j] + 64) >> 7, -32768, 32767)          (arithmetic shift: round to nearest, ties up)
 * A value the clamp changes counts once in the handle's saturation counter (gal_synth_iq_saturated).  All gains 128: y = x, the
 * reference's bytes.  y then takes noise, interference and the formats unchanged; gal_synth_noise_from_cn0 and gal_synth_interf_make
 * keep their meaning for a satellite at unity gain, and a satellite at gain g sits 20 log10(g / 128) dB from it.
 * w fits an int32: one slot contributes |x_s| <= 500 (BOC(1,1): v = E1B d - E1C s is 0 or +-2, times a table entry of at most 250;
 * CBOC: one of the two terms is 0 and the other +-2 x at most lround(sqrt(10/11) 250) = 238), so for GAL_ENGINE_MAX_CHAN = 64 slots at
 * GAL_GAIN_MAX |w| + 64 <= 64 x 32767 x 500 + 64 = 1 048 544 064 < 2^31.  (gal_synth_iq_wsum takes ANY int16 streams: where an
 * epoch's gains sum to more than 65535 it forms w in 64 bits, so the definition holds for them without a wrap.)
 */
#define GAL_GAIN_UNITY 128
#define GAL_GAIN_MAX 32767
#define GAL_GAIN_PATTERN_LEN 37 /* antenna pattern: one attenuation in dB per 5 degrees off boresight, 0 .. 180 */
/* Enqueue on the handle's stream: the weighted sum y of the n_parts (1 .. GAL_ENGINE_MAX_CHAN) streams parts_dev[k] -- DEVICE memory,
 * n_epochs x samples_per_epoch complex int16 samples each -- with the gains gain_q7[e * n_parts + k] (HOST memory, copied before the
 * call returns, as is the pointer array) into out_dev.  The rules of gal_synth_iq_convert: 16-byte alignment, an out_dev that overlaps
 * any part is refused (parts may overlap each other), GAL_E_STATE for a buffer of the batch in flight, gal_synth_iq_saturated is the
 * fence and the counter.  A handle holds one gain table: a call waits (on the host) for the kernel of the call before it.
 * GAL_E_INVAL for a null handle or pointer, a misaligned pointer, n_parts outside 1..GAL_ENGINE_MAX_CHAN, n_epochs < 1, a gain above
 * GAL_GAIN_MAX, an overlap; GAL_E_NOMEM if the table cannot be had. */
int gal_synth_iq_wsum(gal_synth_t *h, const int16_t *const *parts_dev, int32_t n_parts, const uint16_t *gain_q7, int32_t n_epochs,
                      int16_t *out_dev);
/* The batch of gal_synth_plan(params, n_epochs, state_in) with the gains gain_q7[e * n_slots + s] (HOST) into iq_dev (DEVICE, 16-byte
 * aligned, n_epochs x samples_per_epoch x 4 bytes).  Built from what exists: the slots are put into groups of equal gain (the same
 * gain in every epoch in which they are active); every group is run through gal_synth_plan / _execute / _finish with the other slots
 * idle, into scratch buffers the handle owns (they grow on demand and are freed by gal_synth_destroy), and gal_synth_iq_wsum is
 * enqueued behind the last one: the synthesis kernels see nothing of the gains, and the batch costs one synthesis run per distinct
 * gain column.  One group at unity -- all gains 128 -- is one run straight into iq_dev.  When the call returns the runs are finished
 * and the sum is ENQUEUED: gal_synth_iq_saturated, or any work on the handle's stream, orders behind it.
 * state_out (host, n_slots entries, may be NULL): for every slot the end state of its own run -- the state of the full run; a gain of
 * 0 still advances it.  state_in may be NULL as for gal_synth_plan.
 * GAL_E_STATE with a batch in flight, or with a plan of gal_synth_plan_async that still waits for its gal_synth_execute (gal_synth_plan
 * would replace such a plan; this call refuses it); GAL_E_INVAL for a null handle, params, gain_q7 or iq_dev, a misaligned iq_dev, a gain above
 * GAL_GAIN_MAX, n_epochs < 1 and whatever gal_synth_plan refuses; GAL_E_NOMEM, with the sizes in the text, if the scratch buffers
 * cannot be had. */
int gal_synth_run_gains(gal_synth_t *h, const gal_chan_epoch_t *params, int32_t n_epochs, const gal_chan_state_t *state_in,
                        const uint16_t *gain_q7, int16_t *iq_dev, gal_chan_state_t *state_out);
/* Synthesis runs (slot groups) the last gal_synth_run_gains of the handle took: 1 for the unity case or an empty sky, otherwise the
 * number of parts of its weighted sum; 0 before the first call.  GAL_E_INVAL for a null pointer. */
int gal_synth_gain_runs(const gal_synth_t *h, int32_t *n_runs);
/* The gain of one satellite in one epoch; host only, needs no GPU.  d_m = geometric distance in metres, elev_rad = elevation,
 * pattern_db = GAL_GAIN_PATTERN_LEN attenuations in dB, one per 5 degrees off boresight (boresight = the zenith), or NULL: isotropic.
 *   ibs  = (int)((90 - elev_rad x 57.2957795131) / 5) clamped to 0 .. 36
 *   *out = min(32767, (int)(128 x (23222000.0 / d_m) x 10^(-pattern_db[ibs] / 20) x 10^(offset_db / 20)))
 * evaluated in double from left to right; the truncation is the reference's (src/galileo-sdr.cpp:469-477).  The reference distance
 * is Galileo's nominal altitude, so a satellite at the zenith is about unity (the reference's 20 200 km is the GPS altitude).
 * GAL_E_INVAL for a null `out`, an argument or pattern value that is not finite, d_m <= 0. */
int gal_synth_gain_q7(double d_m, double elev_rad, const double *pattern_db, double offset_db, uint16_t *out);

/*
 * Front-end (IF) filter (not in the reference, whose files carry the unbounded spectrum of rectangular chips folded into the sample
 * rate): a real FIR filter over the complex int16 stream, between the noise / interference pass and the format conversion.  Like the
 * other passes it is a FIXED INTEGER FUNCTION of its inputs (tests/fir_model.py states it in numpy).
 *
 * x[n] = (I, Q)[n], the complex int16 samples of the WHOLE output stream, x[n] = 0 for n < 0; h[0 .. T-1] real int16 taps in Q14
 * (GAL_FIR_UNITY = 16384 = 1.0), 1 <= T <= GAL_FIR_MAX_TAPS.  Per rail, in integers:
 *   a[n] = sum over k of h[k] x[n - k]
 *   y[n] = clamp((a[n] + 8192) >> 14, -32768, 32767)          (arithmetic shift: round to nearest, ties up)
 * A value the clamp changes counts once in the handle's saturation counter (gal_synth_iq_saturated).  Taps are admitted only with
 * sum |h[k]| <= 65535: then |a| + 8192 <= 65535 x 32768 + 8192 < 2^31 for any int16 input, and a is exact in an int32.
 * h = {16384} gives y = x; h = 16384 at index D and 0 elsewhere gives y[n] = x[n - D], a pure delay.  A symmetric filter of T taps
 * delays the stream by (T - 1) / 2 samples.
 */
#define GAL_FIR_MAX_TAPS 128
#define GAL_FIR_UNITY 16384
/* GAL_OK if the taps are admitted, else GAL_E_INVAL: a null pointer, n_taps outside 1..GAL_FIR_MAX_TAPS, sum |h[k]| > 65535.  Host
 * only, needs no GPU. */
int gal_synth_fir_check(const int16_t *taps_q14, int32_t n_taps);
/* A low-pass: the Hamming-windowed sinc of n_taps taps (odd, 3 .. 127) with the cutoff (-6 dB) frequency cutoff_hz, 0 < cutoff_hz <
 * sample_rate / 2.  Host only, needs no GPU.  With M = n_taps - 1, fc = cutoff_hz / sample_rate, pi = 3.14159265358979323846, in
 * double, for k = 0 .. M:
 *   t    = k - M / 2                                   (an integer: M is even)
 *   s[k] = 2 fc                 for t = 0,    sin(2 pi fc t) / (pi t)  otherwise
 *   w[k] = 0.54 - 0.46 cos(2 pi k / M)
 *   S    = sum over k, in ascending order, of w[k] s[k]
 *   h[k] = llround(16384 x (w[k] s[k]) / S)            (16384 x (w[k] s[k]) first, then the division)
 * and then h[M / 2] += 16384 - sum of h, so that the DC gain is exactly 1.  The taps pass gal_synth_fir_check (GAL_E_INVAL if they
 * would not, or if a tap left the int16 range).  GAL_E_INVAL also for a null pointer, an even n_taps or one outside 3..127, arguments
 * that are not finite, sample_rate <= 0, a cutoff outside (0, sample_rate / 2). */
int gal_synth_fir_lowpass(double cutoff_hz, double sample_rate, int32_t n_taps, int16_t *taps_q14);
/* Give the handle a filter and START A STREAM: the taps (HOST memory, copied before the call returns) go to the device and the
 * handle's history -- the input samples in front of the next call -- is zeroed.  n_taps = 0 (taps_q14 is then not looked at) frees
 * the filter.  A handle holds one filter: the call waits (on the host) for a filter kernel of this handle that is still in flight.
 * GAL_E_INVAL for a null handle and whatever gal_synth_fir_check refuses -- the filter in force, and its history, then stay as they
 * are; GAL_E_NOMEM if the table cannot be had. */
int gal_synth_fir_set(gal_synth_t *h, const int16_t *taps_q14, int32_t n_taps);
/* Enqueue on the handle's stream: filter the NEXT n_samples complex samples of the stream, in_dev -> out_dev (both DEVICE memory,
 * n_samples x 4 bytes).  The handle keeps the last input samples on the device and the call continues from them: ANY CUT OF A
 * STREAM INTO CALLS GIVES THE SAME BYTES AS ONE CALL, calls shorter than the filter included.  n_samples may be any number, not only a
 * multiple of 4 (0: nothing happens).  The rules of gal_synth_iq_convert: 16-byte aligned pointers (of every call: a cut off the vector
 * grid needs a buffer of its own), GAL_E_STATE for a buffer of the batch in flight and with no filter set, gal_synth_iq_saturated is
 * the fence and the counter.  out_dev overlapping in_dev is refused, exactly in place included: neighbouring tiles read each other's
 * input.  GAL_E_INVAL for a null handle, a null or misaligned pointer, an overlap, n_samples >= 2^41.
 * Sharding: a caller that starts in the middle of a stream (gal_synth_execute_range on one of several GPUs) primes the history after
 * gal_synth_fir_set by filtering the T - 1 samples in front of its range (fewer at the start of the stream) and discarding that output. */
int gal_synth_iq_fir(gal_synth_t *h, const int16_t *in_dev, size_t n_samples, int16_t *out_dev);

/*
 * Decimating front-end filter: the stream is synthesised, weighted and given its noise and interference at M
 * times the output rate, and ONE pass filters it and keeps every M-th sample -- what a front-end does that filters wide and then
 * samples.  Only the kept outputs are computed.  A FIXED INTEGER FUNCTION of its inputs (tests/firdec_model.py states it in numpy).
 *
 * x[n] = (I, Q)[n], the complex int16 samples of the WHOLE INPUT (high-rate) stream, n the global index, x[n] = 0 for n < 0;
 * h[0 .. T-1] real int16 taps in Q14, 1 <= T <= GAL_FIRDEC_MAX_TAPS; the decimation 2 <= M <= GAL_FIRDEC_MAX_DECIM.  Per rail:
 *   a[m] = sum over k of h[k] x[M m - k]
 *   y[m] = clamp((a[m] + 8192) >> 14, -32768, 32767)          (arithmetic shift)
 * so y[m] is sample M m of what gal_synth_iq_fir defines for the same taps.  A value the clamp changes counts once in the handle's
 * saturation counter; only kept outputs count.  Taps are admitted only with sum |h[k]| <= 65535: a is exact in an int32 for any
 * int16 input, in any order of accumulation.  A symmetric filter of T taps with T - 1 a multiple of 2 M delays the OUTPUT stream by
 * (T - 1) / (2 M) samples.
 */
#define GAL_FIRDEC_MAX_TAPS 512
#define GAL_FIRDEC_MAX_DECIM 16
/* GAL_OK if taps and decimation are admitted, else GAL_E_INVAL: a null pointer, n_taps outside 1..GAL_FIRDEC_MAX_TAPS, decim outside
 * 2..GAL_FIRDEC_MAX_DECIM, sum |h[k]| > 65535.  Host only, needs no GPU. */
int gal_synth_firdec_check(const int16_t *taps_q14, int32_t n_taps, int32_t decim);
/* The low-pass of gal_synth_fir_lowpass, operation for operation as stated there, for the decimator: n_taps odd, 3 .. 511;
 * sample_rate_in is the rate of the INPUT stream.  The refusals are those of gal_synth_fir_lowpass.  Host only, needs no GPU. */
int gal_synth_firdec_lowpass(double cutoff_hz, double sample_rate_in, int32_t n_taps, int16_t *taps_q14);
/* The outputs a call of n_in input samples keeps when its first input sample has the global index first_sample: the number of m with
 * first_sample <= M m < first_sample + n_in = ceil((first_sample + n_in) / M) - ceil(first_sample / M).  0 for decim outside
 * 2..GAL_FIRDEC_MAX_DECIM or a sum beyond 2^64.  Host only, needs no GPU. */
uint64_t gal_synth_firdec_out_samples(uint64_t first_sample, uint64_t n_in, int32_t decim);
/* Give the handle a decimator and START A STREAM whose next input sample has the global index first_sample (only first_sample mod
 * decim matters): the taps (HOST memory, copied before the call returns) go to the device and the history -- the last 512 input
 * samples -- is zeroed.  n_taps = 0 (taps and decim are then not looked at) frees it.  The decimator has a slot, a tap table and a
 * history of its own: the filter of gal_synth_fir_set is independent of it and untouched.  The call waits (on the host) for a
 * decimator kernel of this handle that is still in flight.  GAL_E_INVAL for a null handle and whatever gal_synth_firdec_check refuses
 * -- the decimator in force, its history and its position then stay as they are; GAL_E_NOMEM if the table cannot be had. */
int gal_synth_firdec_set(gal_synth_t *h, const int16_t *taps_q14, int32_t n_taps, int32_t decim, uint64_t first_sample);
/* Enqueue on the handle's stream: consume the NEXT n_in input samples of the stream (in_dev, DEVICE memory, n_in x 4 bytes) and write
 * the outputs y[m] whose M m falls into them, contiguously from out_dev (DEVICE memory); *n_out = their number =
 * gal_synth_firdec_out_samples(position, n_in, M), known when the call returns (the handle advances its position on the host, at
 * enqueue time).  ANY CUT OF THE INPUT STREAM INTO CALLS GIVES THE BYTES OF ONE CALL: calls shorter than M, shorter than T - 1, not
 * multiples of M, and calls that keep no output (n_in = 0: nothing happens).  Nothing is written behind output *n_out - 1.  The rules
 * of gal_synth_iq_fir: 16-byte aligned pointers, GAL_E_STATE for a buffer of the batch in flight and with no decimator set,
 * gal_synth_iq_saturated is the fence and the counter.  Any overlap of [out_dev, + 4 *n_out) with [in_dev, + 4 n_in) is refused.
 * GAL_E_INVAL for a null handle, a null or misaligned pointer, a null n_out, an overlap, n_in >= 2^41.
 * Sharding: a caller that starts in the middle of a stream calls gal_synth_firdec_set with its own first_sample -- best the index of
 * the first of the T - 1 inputs in front of its range, with which it primes the history; what those produce it discards. */
int gal_synth_iq_firdec(gal_synth_t *h, const int16_t *in_dev, size_t n_in, int16_t *out_dev, size_t *n_out);

/*
 * Block AGC and 2-bit quantiser (not in the reference): what a front-end does between its filter and its ADC --
 * measure the power of the stream in blocks, set a gain from the last blocks, quantise.  The pass sits behind the gains, the noise,
 * the interference and the filter or decimator, in front of (and including) the format.  A FIXED INTEGER FUNCTION of its inputs: the
 * same bytes and gains on any machine, however the stream is cut into calls (tests/agc_model.py states it in numpy).
 *
 * y[n] = (I, Q)[n], the complex int16 samples of the WHOLE stream, n the global index; block b = the samples [b B, (b + 1) B).
 *   P[b] = sum over the 2 B values of block b of y^2, exact in 64 bits.  For a stream that gal_synth_agc_set starts at first_sample:
 *          P[b] = p_init for b < first_sample div B, and the samples in front of first_sample in its own block count as 0
 *   Q[b] = P[b - W] + ... + P[b - 1]: the W blocks BEFORE b.  Feed-forward with one block of delay: every block's gain is known
 *          before its first sample, which keeps the pass parallel and independent of how the stream is cut
 *   ms_q16 = (Q[b] << 16) div (2 B W);  rms_q8 = isqrt(ms_q16), the floor of the square root
 *   g[b] = clamp((target_q8 << 12) div max(rms_q8, 1), gain_min_q12, gain_max_q12)
 *   z    = clamp((int64(y) g[b] + 2048) >> 12, -32768, 32767)   (arithmetic shift), per value, b the block of the value's sample
 * z is then written in one of three formats:
 *   GAL_IQ_ISHORT  z itself
 *   GAL_IQ_IBYTE   the shift / round / +-127 rule of the format above applied to z
 *   GAL_IQ_I2BIT   q = (z > thr) + (z > 0) + (z > -thr) - 2, in {-2, -1, 0, 1}, standing for the value 2 q + 1 = -3, -1, +1, +3; the code is
 *                  q & 3, four codes per byte with value 4k in bits 7..6 (MSB first, as GAL_IQ_IBIT), the unused low bits of the last
 *                  byte 0; ceil(n / 2) bytes for n complex samples; thr = 1 .. 32767
 * Bounds: B W <= 65536, y^2 <= 2^30 and p_init <= 2^31 B give Q <= 2^47, so Q << 16 <= 2^63 fits an unsigned 64-bit word; ms_q16 <= 2^46
 * and rms_q8 <= 2^23; g <= 2^24 and |y g| <= 2^39.
 * A value counts once in the handle's saturation counter (gal_synth_iq_saturated) if the int16 clamp, or GAL_IQ_IBYTE's +-127 clamp,
 * changed it; the 2-bit magnitude saturates by design and does not count.
 * GAL_IQ_I2BIT is a format of gal_synth_iq_agc ONLY: gal_synth_iq_bytes(GAL_IQ_I2BIT, n) is 0 and the conversions and the correlator
 * refuse it.  GAL_IQ_IBIT is refused by gal_synth_iq_agc: a sign needs no gain control.
 */
#define GAL_IQ_I2BIT 3
#define GAL_AGC_MIN_BLOCK 16
#define GAL_AGC_MAX_BLOCK 65536
#define GAL_AGC_MAX_WINDOW 64
#define GAL_AGC_MAX_SPAN 65536   /* block_len x window at most */
#define GAL_AGC_GAIN_UNITY 4096
#define GAL_AGC_GAIN_MAX (1u << 24)
typedef struct gal_iq_agc {
    uint32_t block_len;     /* B: complex samples per block, 16 .. 65536, any integer                                          */
    uint32_t window;        /* W: blocks averaged, 1 .. 64, B W <= 65536                                                       */
    uint32_t target_q8;     /* wanted rms per rail in int16 LSB x 256, 1 .. 32767 x 256                                        */
    uint32_t gain_min_q12;  /* gain clamps, 4096 = 1.0: 1 <= gain_min_q12 <= gain_max_q12 <= 2^24                              */
    uint32_t gain_max_q12;
    uint32_t reserved;      /* 0                                                                                               */
    uint64_t p_init;        /* the power assumed for every block in front of the stream, <= 2^31 B                             */
} gal_iq_agc_t;             /* 32 bytes */
/* GAL_OK if the parameters are admitted, else GAL_E_INVAL: a null pointer, block_len outside 16..65536, window outside 1..64,
 * block_len x window > 65536, target_q8 outside 1..32767 x 256, gain_min_q12 < 1, gain_min_q12 > gain_max_q12, gain_max_q12 > 2^24,
 * p_init > 2^31 x block_len, reserved != 0.  Host only, needs no GPU. */
int gal_synth_agc_check(const gal_iq_agc_t *agc);
/* Bytes that n_samples complex samples take in an AGC output format: 4 n (GAL_IQ_ISHORT), 2 n (GAL_IQ_IBYTE), ceil(n / 2)
 * (GAL_IQ_I2BIT); 0 for any other format, GAL_IQ_IBIT included.  Needs no GPU. */
size_t gal_synth_agc_out_bytes(int32_t format, size_t n_samples);
/* The blocks whose FIRST sample lies in a call of n samples that begins at the global index first_sample: the number of b with
 * first_sample <= b B < first_sample + n = ceil((first_sample + n) / B) - ceil(first_sample / B).  0 for block_len outside 16..65536
 * or a sum beyond 2^64.  Host only, needs no GPU. */
uint64_t gal_synth_agc_blocks(uint64_t first_sample, uint64_t n_samples, int32_t block_len);
/* Parameters from rms values in int16 LSB per rail; host only, needs no GPU.  In double, operation for operation:
 *   target_q8 = llround(target_rms x 256.0)
 *   p_init    = 2 x block_len x llround(init_rms x init_rms)      (the product in double first, then llround, then integers)
 * gain_min_q12 = 1, gain_max_q12 = 2^24 (the clamps at their widest), reserved = 0.  GAL_E_INVAL for a null `out`, an argument that is
 * not finite, init_rms outside [0, 32768] and whatever gal_synth_agc_check refuses of the result (target_rms outside about
 * [0.002, 32767], the block and the window). */
int gal_synth_agc_from_rms(double target_rms, double init_rms, int32_t block_len, int32_t window, gal_iq_agc_t *out);
/* Give the handle an AGC and START A STREAM whose next sample has the global index first_sample (< 2^62).  The state lives on the
 * device: the power of the last W complete blocks (set to p_init) and the partial sum of the open block (0); the handle keeps the
 * position, and with it the sample count of the open block, on the host.  agc == NULL frees it.  The AGC has a slot of its own,
 * independent of the filters.  The call waits (on the host) for an AGC kernel of this handle that is still in flight.  GAL_E_INVAL for
 * a null handle, first_sample >= 2^62 and whatever gal_synth_agc_check refuses -- the AGC in force, its state and its position then
 * stay as they are; GAL_E_NOMEM if the state cannot be had. */
int gal_synth_agc_set(gal_synth_t *h, const gal_iq_agc_t *agc, uint64_t first_sample);
/* Enqueue on the handle's stream: consume the NEXT n_samples complex int16 samples of the stream (in_dev, DEVICE memory, n_samples x 4
 * bytes) and write them, gain-controlled, in `format` to out_dev (DEVICE memory, gal_synth_agc_out_bytes(format, n_samples) bytes).
 * param: the GAL_IQ_IBYTE shift 0..15, the GAL_IQ_I2BIT threshold 1..32767, 0 for GAL_IQ_ISHORT.  gains_dev may be NULL; otherwise
 * (DEVICE memory, 4-byte aligned) it receives uint32 g[b] for the blocks that START in the call, gal_synth_agc_blocks(position,
 * n_samples, B) of them.  n_gains may be NULL; otherwise *n_gains is that number, known when the call returns (the handle advances its
 * position on the host, at enqueue time).  ANY CUT OF THE STREAM INTO CALLS GIVES THE BYTES AND THE GAINS OF ONE CALL: calls shorter
 * than a block, calls that start or end inside one (n_samples = 0: nothing happens); for GAL_IQ_I2BIT where the cuts are at even sample
 * counts, so that every call begins at a byte.  Every call writes into a buffer of its own, as gal_synth_iq_convert does.  The rules of
 * gal_synth_iq_fir: 16-byte aligned in_dev and out_dev, GAL_E_STATE for a buffer of the batch in flight and with no AGC set,
 * gal_synth_iq_saturated is the fence and the counter.  Any overlap of the output or the gains with the input, or of one with the
 * other, is refused.  GAL_E_INVAL for a null handle, a null or misaligned pointer, GAL_IQ_IBIT or an unknown format, a param outside
 * its range, an overlap, n_samples >= 2^41; GAL_E_NOMEM if the call's scratch (12 bytes per block touched) cannot be had. */
int gal_synth_iq_agc(gal_synth_t *h, const int16_t *in_dev, size_t n_samples, int32_t format, int32_t param, void *out_dev,
                     uint32_t *gains_dev, size_t *n_gains);

/*
 * Correlator bank and C/N0 monitor (not in the reference): despread a device buffer of output IQ with the engine's own replica of one
 * satellite and get, per code period, delay and Doppler bin, the complex correlation sums of the E1B and the E1C component.  Read-only
 * on the buffer, in any of the three formats.  Like the formats and the noise floor it is a FIXED INTEGER FUNCTION of its inputs: the
 * same int64 sums on any machine (tests/corr_model.py states it in numpy).
 *
 * v[j] = the interleaved I/Q values of the buffer: GAL_IQ_ISHORT the int16, GAL_IQ_IBYTE the int8, GAL_IQ_IBIT +1 for a set bit and
 * -1 for a clear one (MSB first, as the format defines).  Sample n is (I, Q) = (v[2n], v[2n+1]).  With L = 8184 * 2^32:
 *   P(n)   = code_ph0 + n code_dph (64-bit, exact: the call refuses an n_samples for which it could overflow)
 *   m      = P(n) div L, the code period of sample n;  h(n) = (P(n) mod L) >> 32, the prompt half chip
 *   h_k(n) = (h(n) - (delay0 + k delay_step)) mod 8184 in [0, 8184) for delay index k (m is the prompt's, whatever k)
 *   b[h], c[h]  the E1B / E1C primary code chip of `prn` (gal_tables_e1b / gal_tables_e1c: bit (h >> 1) & 31 of word h >> 6; a set
 *          bit is -1, a clear one +1) times the BOC(1,1) sub-carrier in the sboc convention quoted at GAL_CFG_CBOC (+1 on an odd half
 *          chip, -1 on an even one); no data symbol, no secondary code, no minus sign on C
 *   phi_d(n) = (carr_ph0 + n (carr_dph + dopp0 + d dopp_step)) mod 2^32 for Doppler index d; i = phi_d(n) >> 23;
 *          w = gal_tables_cos512()[i] + i gal_tables_sin512()[i]
 *   S_B(m, d, k) = sum over the samples n of period m of (I + iQ)(n) conj(w) b[h_k(n)];  S_C the same with c
 * out[((m n_dopp + d) n_delay + k) 4 + (0, 1, 2, 3)] = Re S_B, Im S_B, Re S_C, Im S_C for m < max_periods; samples of later periods are
 * not looked at, periods the buffer does not reach stay 0.
 */
typedef struct gal_corr_req {
    int32_t  prn;         /* 1..50                                                                                            */
    int32_t  max_periods; /* 1..1024: code periods (4 ms at the nominal rate), counted from the one sample 0 lies in          */
    uint64_t code_ph0;    /* replica code phase at sample 0: half chips x 2^32, in [0, L)                                     */
    uint64_t code_dph;    /* half chips per sample x 2^32, <= 2^32 (one half chip per sample: the engine's f_code <= fs / 2)   */
    uint32_t carr_ph0;    /* carrier phase at sample 0, 2^-32 cycles                                                         */
    int32_t  carr_dph;    /* carrier phase step per sample, 2^-32 cycles (wraps modulo 2^32 with the Doppler grid added)      */
    int32_t  delay0;      /* first delay, half chips (may be negative); a positive delay = the replica LATER than planned      */
    int32_t  delay_step;  /* >= 1                                                                                             */
    int32_t  n_delay;     /* 1..8184                                                                                          */
    int32_t  dopp0;       /* first Doppler offset, units of carr_dph                                                          */
    int32_t  dopp_step;
    int32_t  n_dopp;      /* 1..64                                                                                            */
} gal_corr_req_t;         /* 56 bytes */
#define GAL_CORR_MAX_REQ 64
#define GAL_CORR_MAX_OUT_BYTES ((size_t)1 << 30) /* of one call, all requests together */
/* Bytes of `out` one request takes: max_periods n_dopp n_delay 4 int64; 0 for a null request or a grid outside the caps above.
 * Needs no GPU. */
size_t gal_synth_corr_out_bytes(const gal_corr_req_t *req);
/* Enqueue on the handle's stream: correlate the n_samples complex samples at buf_dev (DEVICE memory in `format`, 16-byte aligned,
 * gal_synth_iq_bytes(format, n_samples) bytes, only read) with every request; request r writes its sums at out_dev (DEVICE memory,
 * 16-byte aligned) + the sum of gal_synth_corr_out_bytes of the requests in front of it.  out_dev is zeroed by the call.  `reqs` is
 * copied before the call returns.  The rules of gal_synth_iq_convert hold: GAL_E_STATE for the int16 buffer of a batch in flight,
 * gal_synth_iq_saturated is the fence behind which out_dev may be copied.  GAL_E_INVAL for a null handle or pointer, a misaligned
 * pointer, an unknown format, n_req outside 1..GAL_CORR_MAX_REQ, a request outside the ranges stated at gal_corr_req_t, more than
 * GAL_CORR_MAX_OUT_BYTES of output, n_samples = 0 or so large that P(n) could pass 2^64, out_dev overlapping buf_dev. */
int gal_synth_correlate(gal_synth_t *h, const void *buf_dev, int32_t format, size_t n_samples, const gal_corr_req_t *reqs,
                        int32_t n_req, int64_t *out_dev);
/* The replica of a planned record, host only (no GPU): fills prn, code_ph0, code_dph, carr_ph0, carr_dph of *out and leaves the
 * grids and max_periods as they are.  sample_offset >= 0 = the position of the buffer's sample 0 inside the record's epoch.  All
 * rounding is to nearest (ties away from zero, llround):
 *   code_dph = llround(2 f_code / sample_rate x 2^32)
 *   code_ph0 = (llround(2 code_phase0 x 2^32) + sample_offset code_dph) mod L
 *   carr_dph = llround(f_carr / sample_rate x 2^32)   (GAL_E_INVAL where it does not fit an int32: |f_carr| >= sample_rate / 2)
 *   carr_ph0 = (llround(frac(carr_phase0) x 2^32) + sample_offset carr_dph) mod 2^32 with GAL_CH_RESTART, 0 otherwise (the phase a
 *              continuing channel carries is the engine's state, not the record's; |S| does not depend on it)
 * The engine advances its code phase by the double f_code / sample_rate per sample; the replica by code_dph 2^-32, which differs
 * from twice that by at most 2^-33 half chips: over the 260 000 samples of an epoch the replica drifts by at most 260 000 x 2^-33
 * = 3.1e-5 half chips (plus 2^-33 of code_ph0 and the rounding of the engine's own recurrence, ~1e-9 chips), i.e. the half chip
 * index differs on about 3e-5 of the samples at worst.  GAL_E_INVAL also for a null pointer, prn outside 1..50, a negative offset,
 * rates that are not finite or a code step above one half chip per sample. */
int gal_corr_from_epoch(const gal_chan_epoch_t *rec, double sample_rate, int64_t sample_offset, gal_corr_req_t *out);
/* C/N0 from the sums of ONE request copied to the host (`out_host`: gal_synth_corr_out_bytes(req) bytes), host only.  Over the WHOLE
 * periods m = 1 .. max_periods - 2 (m = 0 and the last one are cut by the buffer's ends; the caller keeps max_periods within what
 * the buffer holds; GAL_E_INVAL below 3 periods), at Doppler index d:
 *   Pp = mean of |S_B|^2 + |S_C|^2 at delay index k_prompt,  Pn = the same at k_noise (a delay far from the peak)
 *   T  = the mean period length in seconds = 8184 x 2^32 / (code_dph sample_rate)
 *   *cn0_dbhz = 10 log10((Pp - Pn) / (Pn T / 2)),  *peak_ratio = Pp / Pn
 * the C/N0 of the satellite's COMPOSITE E1B + E1C signal, the figure of gal_synth_noise_from_cn0.  Pp and Pn both sum TWO
 * components, each of which carries half of C against the whole of N0: (Pp - Pn) / Pn = (C / 2) T / N0, hence the factor 2
 * (DESIGN.md section 12 derives it from section 11's powers).  GAL_E_INVAL when Pp <= Pn, or for an index outside the request. */
int gal_corr_cn0(const int64_t *out_host, const gal_corr_req_t *req, int32_t k_prompt, int32_t k_noise, int32_t d, double sample_rate,
                 double *cn0_dbhz, double *peak_ratio);

/*
 * Welch power spectrum of the output stream (not in the reference): the power per frequency bin of a device buffer
 * of output IQ, summed over overlapping windowed segments.  Read-only on the buffer, in any of the three formats.  The transform is an
 * INTEGER one, so that the pass is, like every other, a FIXED INTEGER FUNCTION of its inputs: the same uint64 sums on any machine, in
 * whatever order the segments are added (tests/psd_model.py states it in numpy).  Every >> below is arithmetic (floor).
 *
 * v[j] = the interleaved values of the buffer as gal_synth_correlate defines them (GAL_IQ_ISHORT the int16, GAL_IQ_IBYTE the int8,
 * GAL_IQ_IBIT +-1, MSB first); sample n is (v[2n], v[2n+1]).  g = the format's scale: 0 for ishort, 8 for ibyte, 14 for ibit.
 * N = 2^log2_n.  Segment s covers the samples [s hop, s hop + N); n_seg = (n_samples - N) / hop + 1 for n_samples >= N; a tail shorter
 * than a segment is not looked at.  n_seg = 0 and n_seg N^2 > 2^32 are refused: |X|^2 <= N^2 2^31 per segment, so no sum passes 2^63.
 *   table   C[k] = llround(2^30 cos(2 pi k / 4096)), S[k] = llround(2^30 sin(2 pi k / 4096)), k < 4096 (gal_tables_psd()); size N uses
 *           every (4096 / N)-th entry
 *   window  rectangular: win[n] = 32768;  Hann (periodic): win[n] = (2^30 - C[n 4096 / N]) >> 16, 0 at n = 0 and 32768 at N / 2
 *           per rail xw = (v 2^g win + 2^14) >> 15
 *   transform  radix-2 decimation in time on int32 values with int64 products: bit-reverse the N windowed samples; for h = 1, 2, ..,
 *           N / 2 and every pair u (index p), x (index p + h) with p mod 2h < h:  j = (p mod h) (4096 / (2h)), w_r = C[j], w_i = -S[j],
 *             t_r = (x_r w_r - x_i w_i + 2^29) >> 30,  t_i = (x_r w_i + x_i w_r + 2^29) >> 30,  the pair becomes u + t and u - t
 *           No value leaves int32: the largest is N 32768 sqrt(2) = 2^27.5 at N = 4096.
 *   out[k] = sum over the segments of X_r[k]^2 + X_i[k]^2, uint64, k < N in natural order: bin k is the frequency k fs / N, the bins at
 *           and above N / 2 are the negative frequencies.
 * Against a float64 FFT of the same windowed integers |dX| stays below 0.7, 3.6, 35 and 140 at N = 8, 64, 1024 and 4096: about what
 * 1.4 LSB rms of noise on the input would add.
 */
typedef struct gal_iq_psd {
    int32_t log2_n;   /* 3..12: N = 8..4096 */
    int32_t hop;      /* 1..N samples between segment starts */
    int32_t window;   /* 0 rectangular, 1 Hann (periodic) */
    int32_t reserved; /* 0 */
} gal_iq_psd_t;       /* 16 bytes */
/* n_seg of a call with this configuration on n_samples samples; 0 where the call would be refused (a null cfg, a field out of range,
 * n_samples < N, n_seg N^2 > 2^32).  Host only, needs no GPU. */
int64_t gal_synth_psd_segments(const gal_iq_psd_t *cfg, size_t n_samples);
/* Enqueue on the handle's stream: the spectrum of the n_samples complex samples at buf_dev (DEVICE memory in `format`, 16-byte aligned,
 * gal_synth_iq_bytes(format, n_samples) bytes, only read) into out_dev (DEVICE memory, N uint64, 16-byte aligned; zeroed by the call).
 * *n_seg (host) = the segments summed.  The rules of gal_synth_correlate hold: GAL_E_STATE for the int16 buffer of a batch in flight,
 * gal_synth_iq_saturated is the fence behind which out_dev may be copied.  GAL_E_INVAL for a null handle, a null or misaligned pointer,
 * an unknown format or GAL_IQ_I2BIT, log2_n, hop, window or reserved out of range, n_seg = 0 or above the bound, out_dev overlapping the
 * buffer. */
int gal_synth_iq_psd(gal_synth_t *h, const void *buf_dev, int32_t format, size_t n_samples, const gal_iq_psd_t *cfg, uint64_t *out_dev,
                     int32_t *n_seg);

/*
 * Per-satellite multipath (not in the reference): a satellite's signal arrives a second time, later, weaker and
 * with another carrier phase.  An echo of part p is the part's own STREAM, delayed by a whole number of samples -- code, data symbols
 * and carrier together, as propagation delays them -- times a slowly rotating complex gain.  The pass takes the place of
 * gal_synth_iq_wsum; the synthesis sees nothing of it.  A FIXED INTEGER FUNCTION of its inputs (tests/mpath_model.py states it in numpy).
 *
 * x_k[n] = complex int16 sample n of part k, g[e][k] its Q7 gain in epoch e, as for gal_synth_iq_wsum; N = samples_per_epoch.  Echo r
 * (0 <= r < n_echo <= GAL_ECHO_MAX) has a constant part index p_r and, in every epoch e of the call, one row gal_iq_echo_t: gain A
 * (Q7, 0 .. GAL_GAIN_MAX), delay D (0 .. GAL_ECHO_MAX_DELAY samples), phase ph0 at the epoch's first sample and phase step dph per
 * sample (2^-32 cycles).  For the output sample n, e = n div N, m = n mod N, with the row of the OUTPUT sample's epoch:
 *   u     = x_p[n - D]                       (n - D < 0: the part's history, below; the delay may reach back over any number of epochs)
 *   i     = ((ph0 + m dph) mod 2^32) >> 22;  c = C[i], s = C[(i - 256) & 1023]            (C = gal_tables_cos1024(), Q12)
 *   rI    = (uI c - uQ s + 2048) >> 12;  rQ = (uI s + uQ c + 2048) >> 12                  (arithmetic shifts; |r| <= 65536)
 *   wI[n] = sum_k g[e][k] x_k.I[n] + sum_r A_r rI_r                                        (likewise Q)
 *   y     = clamp((w + 64) >> 7, -32768, 32767)
 * A value the clamp changes counts once in the handle's saturation counter.  n_echo = 0 is gal_synth_iq_wsum bit for bit.  w is formed
 * in an int32 where sum_k g + 2 sum_r A <= 65535 in every epoch (|w| + 64 <= 65535 x 32768 + 64 < 2^31 for any int16 input), in 64
 * bits otherwise: the same bits.
 *
 * History: the handle keeps GAL_ECHO_LINES = 64 lines of GAL_ECHO_MAX_DELAY complex samples.  hist_id[k] (NULL: k) names the line of
 * part k, 0 .. 63, or -1: none.  For a part with a line, the samples in front of the call (n - D < 0) are the last 1024 samples that
 * earlier calls gave under that id since the last gal_synth_mpath_reset (or the creation of the handle) -- zeros in front of those --,
 * and after the call the line holds the part's last 1024 samples (a call shorter than that rolls the line).  So ANY CUT OF A STREAM
 * INTO CALLS OF WHOLE EPOCHS GIVES THE SAME BYTES AS ONE CALL.  A line that no part of a call names stays as it is.
 */
#define GAL_ECHO_MAX 32
#define GAL_ECHO_MAX_DELAY 1024
#define GAL_ECHO_LINES 64
typedef struct gal_iq_echo {
    uint16_t gain_q7;   /* A: 0 .. GAL_GAIN_MAX, 128 = the part at unity                                                       */
    uint16_t delay;     /* D: 0 .. GAL_ECHO_MAX_DELAY samples                                                                  */
    uint32_t ph0;       /* phase at the epoch's first sample, 2^-32 cycles                                                     */
    int32_t  dph;       /* phase step per sample, 2^-32 cycles                                                                 */
    uint32_t reserved;  /* 0                                                                                                   */
} gal_iq_echo_t;        /* 16 bytes */
/* GAL_OK if the echo table is admitted, else GAL_E_INVAL: n_echo outside 0..GAL_ECHO_MAX, n_epochs < 1, n_parts outside
 * 1..GAL_ENGINE_MAX_CHAN, and with n_echo > 0 a null pointer, a part index outside 0..n_parts-1, a gain above GAL_GAIN_MAX, a delay
 * above GAL_ECHO_MAX_DELAY, reserved != 0.  echo_rows is [n_epochs][n_echo].  Host only, needs no GPU. */
int gal_synth_mpath_check(const gal_iq_echo_t *echo_rows, int32_t n_echo, int32_t n_epochs, const int32_t *part_of_echo, int32_t n_parts);
/* Zero every history line (enqueued on the handle's stream): the next call starts its streams.  GAL_E_INVAL for a null handle. */
int gal_synth_mpath_reset(gal_synth_t *h);
/* Enqueue on the handle's stream: y of the definition above into out_dev.  parts_dev, n_parts, gain_q7, n_epochs, out_dev and the
 * rules are those of gal_synth_iq_wsum: 16-byte alignment, an out_dev that overlaps a part is refused, GAL_E_STATE for a buffer of the
 * batch in flight, gal_synth_iq_saturated is the fence and the counter.  hist_id (HOST, n_parts entries, or NULL), part_of_echo (HOST,
 * n_echo entries) and echo_rows (HOST, [n_epochs][n_echo]) are copied before the call returns; with n_echo = 0 the last two are not
 * looked at.  A handle holds one table: a call waits (on the host) for the kernel of the call before it.  GAL_E_INVAL for what
 * gal_synth_iq_wsum and gal_synth_mpath_check refuse, a hist_id outside -1..63, one line named by two parts, an echo on a part whose
 * hist_id is -1; GAL_E_NOMEM if the table or the lines cannot be had. */
int gal_synth_iq_mpath(gal_synth_t *h, const int16_t *const *parts_dev, int32_t n_parts, const int32_t *hist_id, const uint16_t *gain_q7,
                       int32_t n_epochs, const int32_t *part_of_echo, const gal_iq_echo_t *echo_rows, int32_t n_echo, int16_t *out_dev);
/* gal_synth_run_gains with echoes: slot_of_echo[r] (0 .. n_slots-1, n_slots <= GAL_ECHO_LINES) is the channel slot echo r repeats.
 * Every slot that carries an echo is a group (a synthesis run) of its own, whatever its gains, also where it is idle in the whole
 * batch, and its history line is its SLOT INDEX: the history follows the slot from batch to batch.  An echo repeats the SLOT's stream and
 * a line is written only in calls in which its slot carries an echo: where another satellite takes over a slot, the first D delayed
 * samples are the earlier occupant's if both fall into one call, and the line as it was last written if a call boundary lies between
 * them, unless the caller calls gal_synth_mpath_reset.  gal_synth_iq_mpath takes the place of
 * the weighted sum.  n_echo = 0 is gal_synth_run_gains, the single-run unity case included; gal_synth_gain_runs counts the runs.
 * The refusals are those of gal_synth_run_gains, gal_synth_mpath_check (with the slots as parts) and gal_synth_iq_mpath. */
int gal_synth_run_mpath(gal_synth_t *h, const gal_chan_epoch_t *params, int32_t n_epochs, const gal_chan_state_t *state_in,
                        const uint16_t *gain_q7, const int32_t *slot_of_echo, const gal_iq_echo_t *echo_rows, int32_t n_echo,
                        int16_t *iq_dev, gal_chan_state_t *state_out);
/* One echo from physical figures; host only, needs no GPU.  In double, operation for operation:
 *   delay     = llround(delay_s x sample_rate)                           (samples, 0 .. GAL_ECHO_MAX_DELAY)
 *   alpha_q12 = llround(4096 x 10^(rel_db / 20))                         (amplitude relative to the direct signal, at most 8192 = +6.02 dB)
 *   ph0       = llround((phase_deg / 360 - floor(phase_deg / 360)) x 2^32) mod 2^32
 *   dph       = llround(fade_hz / sample_rate x 2^32)                    (must fit an int32: |fade_hz| < sample_rate / 2)
 * GAL_E_INVAL for a null `out`, an argument that is not finite, sample_rate <= 0, delay_s < 0 and a result outside the ranges above. */
typedef struct gal_mpath_echo {
    uint32_t delay;
    uint32_t alpha_q12;
    uint32_t ph0;
    int32_t  dph;
} gal_mpath_echo_t; /* 16 bytes */
int gal_synth_mpath_make(double delay_s, double rel_db, double phase_deg, double fade_hz, double sample_rate, gal_mpath_echo_t *out);
/* The row of `echo` in the epoch with the index `epoch` of the WHOLE stream, for a direct signal at the gain slot_gain_q7; host only:
 *   gain_q7 = min(GAL_GAIN_MAX, (slot_gain_q7 x alpha_q12 + 2048) >> 12)
 *   ph0     = (echo->ph0 + epoch x samples_per_epoch x dph) mod 2^32      (so that ph0[e + 1] = ph0[e] + N dph)
 * delay and dph as they are, reserved = 0.  GAL_E_INVAL for a null pointer, samples_per_epoch < 1, a slot gain above GAL_GAIN_MAX, an
 * echo outside the ranges of gal_synth_mpath_make. */
int gal_synth_mpath_row(const gal_mpath_echo_t *echo, uint16_t slot_gain_q7, uint64_t epoch, int32_t samples_per_epoch, gal_iq_echo_t *row);

/*
 * Geometric reflectors (not in the reference): the echo pass above with a delay of D + F / 4096 samples, and the
 * geometry that fills its rows from the satellite's azimuth and elevation -- a ground bounce, a wall --, so that an echo's delay, its
 * carrier phase and the rate at which that phase turns all follow from ONE excess path.  A FIXED INTEGER FUNCTION of its inputs
 * (tests/refl_model.py states it in numpy).
 *
 * Everything is as for gal_synth_iq_mpath but the row, gal_iq_refl_t, which carries F = frac_q12 (0 .. 4095) as well, and the delayed
 * value: for the output sample n, with the row of the OUTPUT sample's epoch,
 *   a = x_p[n - D],  b = x_p[n - D - 1]                    (history as for gal_synth_iq_mpath)
 *   u = a + ((F (b - a) + 2048) >> 12)                     (per rail, arithmetic shift; with F = 0, u = a and b is not read)
 * and u takes the place of x_p[n - D] in the rotation, the sum, the rounding, the clamp and the saturation count.  u lies between a
 * and b inclusive, so |u| <= 32768 and the int32 / int64 rule (sum_k g + 2 sum_r A <= 65535) is unchanged; |F (b - a)| < 2^28.
 * Range: D + (F > 0 ? 1 : 0) <= GAL_ECHO_MAX_DELAY -- D = 1024 only with F = 0.  With F = 0 in every row the output is
 * gal_synth_iq_mpath bit for bit (such a row IS a gal_iq_echo_t), with n_echo = 0 gal_synth_iq_wsum.  Linear interpolation because
 * the synthesised chips are rectangular and sample-held: the correlation of such a stream with the code is piecewise linear between
 * whole-sample lags, and a two-tap interpolation moves it by exactly the fraction.
 *
 * The pass shares the handle's GAL_ECHO_LINES history lines with gal_synth_iq_mpath: the same hist_id rules, the same "any cut into
 * calls of whole epochs gives the bytes of one call", also where calls of the two passes alternate on one handle;
 * gal_synth_mpath_reset zeroes the lines for both.
 */
typedef struct gal_iq_refl {
    uint16_t gain_q7;   /* A: 0 .. GAL_GAIN_MAX, 128 = the part at unity                                                       */
    uint16_t delay;     /* D: whole samples, 0 .. GAL_ECHO_MAX_DELAY (GAL_ECHO_MAX_DELAY - 1 where frac_q12 > 0)               */
    uint32_t ph0;       /* phase at the epoch's first sample, 2^-32 cycles                                                     */
    int32_t  dph;       /* phase step per sample, 2^-32 cycles                                                                 */
    uint16_t frac_q12;  /* F: the delay's fraction in 1/4096 sample, 0 .. 4095                                                 */
    uint16_t reserved;  /* 0                                                                                                   */
} gal_iq_refl_t;        /* 16 bytes */
/* gal_synth_mpath_check for rows of gal_iq_refl_t: it refuses what that refuses, frac_q12 > 4095 and a delay of GAL_ECHO_MAX_DELAY
 * with frac_q12 > 0.  Host only, needs no GPU. */
int gal_synth_refl_check(const gal_iq_refl_t *refl_rows, int32_t n_echo, int32_t n_epochs, const int32_t *part_of_echo, int32_t n_parts);
/* gal_synth_iq_mpath with rows of gal_iq_refl_t: the same arguments, rules, history lines and refusals (gal_synth_refl_check in the
 * place of gal_synth_mpath_check). */
int gal_synth_iq_refl(gal_synth_t *h, const int16_t *const *parts_dev, int32_t n_parts, const int32_t *hist_id, const uint16_t *gain_q7,
                      int32_t n_epochs, const int32_t *part_of_echo, const gal_iq_refl_t *refl_rows, int32_t n_echo, int16_t *out_dev);
/* gal_synth_run_mpath with rows of gal_iq_refl_t and gal_synth_iq_refl in the place of gal_synth_iq_mpath: every slot with an echo is
 * a group of its own, its history line is its slot index, n_echo = 0 is gal_synth_run_gains, gal_synth_gain_runs counts the runs. */
int gal_synth_run_refl(gal_synth_t *h, const gal_chan_epoch_t *params, int32_t n_epochs, const gal_chan_state_t *state_in,
                       const uint16_t *gain_q7, const int32_t *slot_of_echo, const gal_iq_refl_t *refl_rows, int32_t n_echo,
                       int16_t *iq_dev, gal_chan_state_t *state_out);
/* The excess path, in metres, of the reflection off one plane for a satellite at (az_rad from north over east, el_rad); host only,
 * needs no GPU.  In double, operation for operation:
 *   GAL_REFL_GROUND, p[0] = h, the antenna's height over a horizontal plane (>= 0):  excess = 2 h sin(el), an echo where el > 0
 *   GAL_REFL_WALL, p[0] = d (>= 0), p[1] = a_w: a vertical plane at the distance d in the direction of the azimuth a_w (rad):
 *                                                excess = -2 d cos(el) cos(az - a_w), an echo where excess > 0 (the satellite
 *                                                stands on the side away from the wall)
 * Where there is no echo, *excess_m = -1 and the return value is still GAL_OK: gal_synth_refl_row makes that a row of gain 0.
 * GAL_E_INVAL for a null pointer, another kind, an argument that is not finite, h < 0 or d < 0. */
#define GAL_REFL_GROUND 0
#define GAL_REFL_WALL 1
int gal_synth_refl_geom(int32_t kind, const double *p, double az_rad, double el_rad, double *excess_m);
/* The row of one epoch of N = samples_per_epoch samples from the excess path at the epoch's first sample (excess_now_m) and at the
 * next epoch's (excess_next_m), for a direct signal at the gain slot_gain_q7; host only.  In double, operation for operation, with
 * c = 299792458.0 and lambda = c / 1575420000.0 (that of gal_synth_array_phase):
 *   t       = excess_now_m / c x sample_rate;  D = floor(t);  F = llround((t - D) x 4096), and F = 4096 is D + 1, F = 0
 *   cyc(x)  = -x / lambda + refl_phase_deg / 360;  P(x) = llround((cyc - floor(cyc)) x 2^32) mod 2^32
 *   ph0     = P(excess_now_m)
 *   dph     = llround((double)(int32_t)(P(excess_next_m) - ph0) / N)      (the wrapped signed difference: ph0 + N dph meets the
 *                                                                          next epoch's ph0 to within N / 2 units of 2^-32 cycle)
 *   gain_q7 = min(GAL_GAIN_MAX, (slot_gain_q7 x llround(4096 x 10^(rel_db / 20)) + 2048) >> 12)    (as gal_synth_mpath_row)
 * excess_now_m < 0 (no echo in this epoch): the row is all zeros.  excess_next_m < 0 (none in the next): dph = 0.  GAL_E_INVAL for a
 * null row, an argument that is not finite, sample_rate <= 0, N < 1, a slot gain above GAL_GAIN_MAX, an amplitude above 2 (+6.02 dB)
 * and a delay outside the range of gal_iq_refl_t. */
int gal_synth_refl_row(double excess_now_m, double excess_next_m, double rel_db, double refl_phase_deg, double sample_rate,
                       int32_t samples_per_epoch, uint16_t slot_gain_q7, gal_iq_refl_t *row);

/*
 * Receiver oscillator (not in the reference, whose receiver has a perfect clock): a carrier offset, a linear
 * drift and white-FM phase noise of the local oscillator, i.e. ONE rotation common to everything that enters the mixer -- all
 * satellites, their echoes, the interference sources, the noise floor.  A FIXED INTEGER FUNCTION of (parameters, index of the sample
 * in the whole stream, int16 input): the same bytes on any machine and for any cut of the stream into calls (tests/osc_model.py states
 * it in numpy).
 *
 * x[n] = the complex int16 sample with the global index N = first_sample + n.  All phase arithmetic is modulo 2^64, in units of 2^-64
 * cycles (wrapping uint64 arithmetic is exact):
 *   Phi(N) = P0 + N F + T(N) D + S Z(N),   T(N) = N (N - 1) / 2  (halve the even factor first: exact mod 2^64)
 *   Z(N)   = sum of z(j) for N0 < j <= N,  N0 = the first_sample given to the set call below;  Z(N0) = 0
 *   z(j)   = the Q12 Gaussian of the noise floor above (same table T, same steps) of word j & 3 of Philox4x32-10 with the counter
 *            (B & 0xffffffff, B >> 32, stream, 1), B = j >> 2, key = (seed & 0xffffffff, seed >> 32).  Counter word 3 = 1 keeps it
 *            disjoint from the noise floor, which uses 0
 *   theta  = Phi >> 32  (uint32, 2^-32 cycles);  t = (theta + 2^21) mod 2^32
 *   i      = t >> 22  (0 .. 1023);  e = ((t >> 10) & 4095) - 2048  (the residual, 2^-22 cycles, -2048 .. 2047)
 *   c0 = C[i], s0 = C[(i - 256) & 1023]                                       (C = gal_tables_cos1024(), Q12)
 *   c  = c0 - ((s0 e 101 + 2^25) >> 26);  s = s0 + ((c0 e 101 + 2^25) >> 26)  (first-order correction; 101 = round(2 pi 2^4);
 *                                                                               arithmetic shifts)
 *   yI = clamp((xI c - xQ s + 2048) >> 12, -32768, 32767);  yQ = clamp((xI s + xQ c + 2048) >> 12, -32768, 32767)    (y = x e^{+j theta})
 * A complex sample counts ONCE as saturated if either clamp changed it.  |s0 e 101| <= 4096 x 2048 x 101 < 2^30, so |c|, |s| <= 4096
 * + 13 and every product and sum fits an int32 for any int16 input.  F = D = S = P0 = 0 gives c = 4096, s = 0 and y = x bit for bit.
 * The frequency resolution is sample_rate x 2^-64, the drift resolution sample_rate^2 x 2^-64 (4e-7 Hz/s at 2.6 MS/s); the 12-bit
 * residual keeps the table's 0.35 degree steps out of the result.  The sample clock stays ideal: the code rate is not scaled.
 */
typedef struct gal_iq_osc {
    uint64_t seed;      /* Philox key of the phase noise                                                                     */
    uint32_t stream;    /* Philox counter word 2 (the CLI: the site index of --sites)                                         */
    uint32_t reserved;  /* 0                                                                                                 */
    uint64_t p0;        /* P0: phase at N = 0, 2^-64 cycles                                                                   */
    int64_t  f;         /* F: phase step per sample, 2^-64 cycles (the carrier offset / sample_rate x 2^64)                   */
    int64_t  d;         /* D: change of the step per sample (the drift / sample_rate^2 x 2^64)                                */
    uint64_t s;         /* S <= 2^48: the phase-noise increment of a sample is S z 2^-64 cycles, sigma = S 2^-52 sqrt(var z) */
} gal_iq_osc_t;         /* 48 bytes */
/* GAL_OK if the parameters are admitted, else GAL_E_INVAL: a null pointer, reserved != 0, s > 2^48.  Host only, needs no GPU. */
int gal_synth_osc_check(const gal_iq_osc_t *osc);
/* Parameters from physical figures; host only, needs no GPU.  In double, operation for operation, rounding to nearest (llround):
 *   f = llround(f_hz / sample_rate x 2^64);   d = llround(drift_hz_s / sample_rate / sample_rate x 2^64)
 *   sigma_cycles = carrier_hz x sqrt(h0 / (2 sample_rate)): white-FM phase noise with the one-sided fractional-frequency PSD h0 (in
 *        seconds) gives the per-sample phase increment the variance (2 pi carrier_hz)^2 h0 / (2 sample_rate) rad^2
 *   s = llround(sigma_cycles / sqrt(v) x 2^52), v = the variance of z / 4096^2 taken from the table itself: v = M2 / 2^55 with the
 *        integer M2 = the sum of z(u)^2 over all 2^32 words u, halved (0.99999...: not assumed to be 1)
 * seed = 1, stream = 0, p0 = 0, reserved = 0.  GAL_E_INVAL for a null `out`, an argument that is not finite, sample_rate <= 0,
 * carrier_hz < 0, |f_hz| >= sample_rate / 2, a drift whose d does not fit an int64, h0 < 0, an s above 2^48. */
int gal_synth_osc_make(double f_hz, double drift_hz_s, double h0, double sample_rate, double carrier_hz, gal_iq_osc_t *out);
/* Give the handle the oscillator *osc (copied) and start a stream: N0 = first_sample (< 2^62) = the global index of the next sample,
 * and the running sum Z on the device is zeroed (enqueued on the handle's stream).  osc == NULL switches the oscillator off.
 * GAL_E_INVAL for a null handle, what the check refuses, first_sample >= 2^62; GAL_E_NOMEM if the state cannot be had. */
int gal_synth_osc_set(gal_synth_t *h, const gal_iq_osc_t *osc, uint64_t first_sample);
/* Enqueue on the handle's stream: the next n_samples complex int16 samples of the stream, in_dev -> out_dev (DEVICE memory, 16-byte
 * aligned, 4 n_samples bytes each).  It may run exactly IN PLACE (out_dev == in_dev); any other overlap is refused.  Calls continue
 * the stream where the last one ended: ANY CUT OF A STREAM INTO CALLS GIVES THE SAME BYTES AS ONE CALL.  With s > 0 a call is three
 * launches (tile sums, a scan of them, the rotation) ordered by the stream alone, and the handle keeps a scratch of 12 bytes per 1024
 * samples of its longest call.  gal_synth_iq_saturated is the fence and the counter.  GAL_E_INVAL for a null handle or pointer, a
 * misaligned pointer, n_samples >= 2^41, a partial overlap; GAL_E_STATE for a buffer of the batch in flight and where no oscillator is
 * set; GAL_E_NOMEM if the scratch cannot be had. */
int gal_synth_iq_osc(gal_synth_t *h, const int16_t *in_dev, size_t n_samples, int16_t *out_dev);
/* The deterministic step of the oscillator at sample N in the correlator's units, so that a replica can follow it: *carr_dph =
 * (int32)((F + N D) mod 2^64 >> 32) (2^-32 cycles per sample; add it to gal_corr_req_t.carr_dph).  Host only, needs no GPU.
 * GAL_E_INVAL for a null pointer. */
int gal_synth_osc_lo_step(const gal_iq_osc_t *osc, uint64_t N, int32_t *carr_dph);

/*
 * Ionospheric scintillation (not in the reference): ONE satellite's stream -- a "part" of gal_synth_run_gains /
 * gal_synth_run_mpath -- times a slowly varying complex factor z, a Rician field with a Gaussian spectrum: random, per-satellite
 * fading and phase wander.  z is a FIXED INTEGER FUNCTION of (row, index N of the sample in the whole stream); with the int16 input
 * that fixes every byte.  It keeps NO STATE: any cut of the stream into calls gives the same bytes as one call, without conditions
 * (tests/scint_model.py states it in numpy).
 *
 * Draw i (uint64): Philox4x32-10 as the noise floor uses it, key = (seed & 0xffffffff, seed >> 32), counter = (i & 0xffffffff,
 * i >> 32, stream, 2) -- counter word 3 is 0 for the noise floor and 1 for the oscillator, so the three are disjoint.  gI(i) = the Q12
 * Gaussian of output word 0, gQ(i) that of word 1 (the noise floor's table T and steps; |g| <= 25960).
 * h = gal_tables_scint(): h[t] = round(32768 c exp(-(t - 15.5)^2 / 32)), t < 32, c such that H2 = sum h^2 is as close to 2^30 as it
 * gets (sum h = 123382, H2 / 2^30 = 1.0000136; the committed table is the definition).
 * Node j (uint64):
 *   SI    = sum_t h[t] gI(j + t)  (int64);  XI = (SI + 2^14) >> 15                           (likewise SQ, XQ; |X| < 2^17)
 *   ZI[j] = clamp(A + ((B XI + 2048) >> 12), -32767, 32767);  ZQ[j] = clamp((B XQ + 2048) >> 12, -32767, 32767)
 * Sample N, with L = node_len:
 *   j  = N div L, m = N mod L;  R = floor(2^32 / L) (m R < 2^32);  fr = (m R) >> 20          (Q12, 0 .. 4095)
 *   zI = ZI[j] + (((ZI[j + 1] - ZI[j]) fr + 2048) >> 12)                                     (likewise zQ: linear between the nodes)
 *   yI = clamp((xI zI - xQ zQ + 2048) >> 12, -32768, 32767);  yQ = clamp((xI zQ + xQ zI + 2048) >> 12, -32768, 32767)
 * All shifts are arithmetic.  A complex sample counts ONCE in the handle's saturation counter if either clamp changed it.  The node
 * clamp keeps |z| <= 32767, so |xI zI - xQ zQ| + 2048 <= 2 x 32768 x 32767 + 2048 < 2^31: every product and sum fits an int32 for any
 * int16 input (B XI < 2^29 too).  A = 4096, B = 0 gives z = 4096 and y = x bit for bit.
 * The nodes are a unit-variance (at 4096) Gaussian sequence with the autocorrelation exp(-k^2 / 64): 1/e at a lag of 8 nodes, so
 * tau0 = 8 L / sample_rate is the 1/e decorrelation time of the scattered field.
 */
typedef struct gal_iq_scint {
    uint64_t seed;      /* Philox key                                                                                        */
    uint32_t stream;    /* Philox counter word 2 (the CLI: site index << 8 | PRN)                                            */
    uint32_t node_len;  /* L: samples between two nodes, 64 .. 2^24                                                          */
    uint16_t a_q12;     /* A <= 4096: the direct (specular) component of z                                                   */
    uint16_t b_q12;     /* B <= 4096: the scale of the scattered component                                                   */
    uint32_t reserved;  /* 0                                                                                                 */
} gal_iq_scint_t;       /* 24 bytes */
#define GAL_SCINT_MIN_NODE 64
#define GAL_SCINT_MAX_NODE (1u << 24)
#define GAL_SCINT_MAX_JOBS 64
/* GAL_OK if the row is admitted, else GAL_E_INVAL: a null pointer, node_len outside 64 .. 2^24, a_q12 or b_q12 above 4096,
 * reserved != 0.  Host only, needs no GPU. */
int gal_synth_scint_check(const gal_iq_scint_t *row);
/* A row from physical figures; host only, needs no GPU.  In double, operation for operation, rounding to nearest (llround):
 *   s4 in (0, 1):  m = 1 / s4^2 (the Nakagami m);  q = sqrt(m^2 - m);  K = q / (m - q) (the Rician K with that S4)
 *                  A = llround(4096 sqrt(K / (K + 1)));  B = llround(4096 sqrt(1 / (2 (K + 1) v)))
 *   v = the variance of XI / 4096 taken from the tables themselves: (H2 / 2^30) x (M2 / 2^55), M2 as for gal_synth_osc_make
 *   s4 = 0: A = 4096, B = 0 (the identity);  s4 = 1 (Rayleigh): A = 0, B = llround(4096 sqrt(1 / (2 v)))
 *   node_len = llround(tau0_s x sample_rate / 8)
 * seed = 1, stream = 0, reserved = 0.  The mean of |z|^2 is 4096^2.  GAL_E_INVAL for a null `out`, an argument that is not finite, s4
 * outside [0, 1], sample_rate <= 0, a node_len outside 64 .. 2^24. */
int gal_synth_scint_make(double s4, double tau0_s, double sample_rate, gal_iq_scint_t *out);
typedef struct gal_scint_job {
    const int16_t *in_dev;   /* DEVICE, 16-byte aligned, 4 n_samples bytes                                                   */
    int16_t       *out_dev;  /* DEVICE, 16-byte aligned: in_dev itself (in place) or a buffer that does not meet it          */
    uint64_t       n_samples;    /* complex samples, < 2^41 (0: the job does nothing)                                        */
    uint64_t       first_sample; /* N of the job's first sample, < 2^62                                                      */
    gal_iq_scint_t row;
} gal_scint_job_t;           /* 56 bytes */
/* Enqueue on the handle's stream: every job's y of the definition above, ALL JOBS IN ONE LAUNCH (1 <= n_jobs <= GAL_SCINT_MAX_JOBS).
 * `jobs` is HOST memory, copied before the call returns.  A job may run exactly IN PLACE; any other overlap of its two buffers is
 * refused, and so is a job's output that meets another job's input or output (two jobs may read one input).  A job with A = 4096,
 * B = 0 copies, or does nothing in place.  A handle holds one job table: a call waits (on the host) for the kernel of the call before
 * it.  gal_synth_iq_saturated is the fence and the counter.  GAL_E_INVAL for a null handle or pointer, n_jobs outside 1 .. 64, what
 * gal_synth_scint_check refuses, a misaligned pointer, first_sample >= 2^62, n_samples >= 2^41, an overlap; GAL_E_STATE for a buffer of
 * the batch in flight; GAL_E_NOMEM if the job table cannot be had. */
int gal_synth_iq_scint(gal_synth_t *h, const gal_scint_job_t *jobs, int32_t n_jobs);
/* gal_synth_run_mpath with scintillation: scint_rows is HOST [n_epochs][n_slots], the row of every slot in every epoch (a slot without
 * scintillation: A = 4096, B = 0, any admitted L; such a row is not looked at further), first_sample (< 2^62) the global index of the
 * batch's first sample.  Every slot that has a non-identity row in any epoch of the batch is a group (a synthesis run) of its own, as
 * a slot with an echo is; its part goes through gal_synth_iq_scint in place BEFORE gal_synth_iq_mpath (or the weighted sum), so its
 * echoes are echoes of the scintillated stream.  One job per slot and maximal run of epochs with an equal row, all jobs of the batch
 * in one call (in calls of 64 where there are more).  A row may change only at an epoch whose first sample is a multiple of four
 * samples into the batch (always, where samples_per_epoch is one).  scint_rows == NULL is gal_synth_run_mpath bit for bit;
 * gal_synth_gain_runs counts the runs.  The refusals are those of gal_synth_run_mpath, gal_synth_scint_check (every row) and
 * gal_synth_iq_scint. */
int gal_synth_run_scint(gal_synth_t *h, const gal_chan_epoch_t *params, int32_t n_epochs, const gal_chan_state_t *state_in,
                        const uint16_t *gain_q7, const int32_t *slot_of_echo, const gal_iq_echo_t *echo_rows, int32_t n_echo,
                        const gal_iq_scint_t *scint_rows, uint64_t first_sample, int16_t *iq_dev, gal_chan_state_t *state_out);

/*
 * Antenna array (not in the reference): K phase-coherent output streams, one per antenna element, out of the
 * P "parts" of gal_synth_run_gains -- in each of them every part carries the carrier phase its own direction of arrival gives it at
 * that element.  A FIXED INTEGER FUNCTION of its inputs (tests/array_model.py states it in numpy).
 *
 * x_k[n] = complex int16 sample n of part k, as for gal_synth_iq_wsum; N = samples_per_epoch, e = n div N.  (w_re, w_im) = the weight
 * row of (epoch e, element a, part k), Q12: 4096 = the part at unity, unrotated.  For element a:
 *   AI = sum_k (x_k.I w_re - x_k.Q w_im)        AQ = sum_k (x_k.I w_im + x_k.Q w_re)
 *   y_a.I = clamp((AI + 2048) >> 12, -32768, 32767)        likewise Q                    (arithmetic shift: round to nearest, ties up)
 * A value the clamp changes counts once in the handle's saturation counter.  A and its rounding term fit an int32 where
 * sum_k (|w_re| + |w_im|) <= 65535 for that (epoch, element): |A| + 2048 <= 32768 x 65535 + 2048 < 2^31 for ANY int16 input; otherwise
 * the sum is formed in 64 bits and gives the same bits.  With w = (32 g, 0) for a Q7 gain g <= 1023 the output is
 * clamp((sum_k g x_k + 64) >> 7), because floor((32 S + 2048) / 4096) = floor((S + 64) / 128): K = 1 with such weights is
 * gal_synth_iq_wsum bit for bit.
 */
#define GAL_ARRAY_MAX_ELEM 8
#define GAL_STEER_GAIN_MAX 1023 /* the largest Q7 gain gal_synth_steer_make turns into a weight: 32 x 1023 = 32736 */
typedef struct gal_iq_steer {
    int16_t w_re;  /* Q12, -32767 .. 32767 (-32768 is refused, so that a negated weight fits)                                    */
    int16_t w_im;  /* likewise                                                                                                */
} gal_iq_steer_t;  /* 4 bytes */
/* GAL_OK if the weight rows[(e * n_elem + a) * n_parts + k] are admitted, else GAL_E_INVAL: a null pointer, n_epochs < 1, n_elem
 * outside 1 .. GAL_ARRAY_MAX_ELEM, n_parts outside 1 .. GAL_ENGINE_MAX_CHAN, a component of -32768.  Host only, needs no GPU. */
int gal_synth_steer_check(const gal_iq_steer_t *rows, int32_t n_epochs, int32_t n_elem, int32_t n_parts);
/* The weight of a part at the Q7 gain g = gain_q7 turned by `phase` (2^-32 cycles, rounded -- not truncated -- to the 1024-entry
 * table); host only, needs no GPU.  Integers only, C = gal_tables_cos1024():
 *   i    = ((phase + 2^21) >> 22) & 1023
 *   w_re = (g C[i] + 64) >> 7;  w_im = (g C[(i - 256) & 1023] + 64) >> 7                 (g e^(+j 2 pi i / 1024), Q12)
 * g = 128, phase = 0 gives (4096, 0).  GAL_E_INVAL for a null `out` or g > 1023 (+18 dB over unity: the weight would leave int16). */
int gal_synth_steer_make(uint16_t gain_q7, uint32_t phase, gal_iq_steer_t *out);
/* The carrier phase, in 2^-32 cycles, that a plane wave from azimuth az_rad (from north over east, as the front-end's azel[0]) and
 * elevation el_rad has at an element displaced by enu_m = (east, north, up) metres from the array's reference point, relative to
 * that point; host only, needs no GPU.  In double, operation for operation:
 *   u = (sin az cos el, cos az cos el, sin el)            (the unit vector towards the source)
 *   cyc = (enu . u) / lambda, lambda = 299792458.0 / 1575420000.0;  *phase = llround((cyc - floor(cyc)) x 2^32) mod 2^32
 * An element displaced towards the source receives the wavefront earlier: its phase advances.  GAL_E_INVAL for a null pointer or a
 * value that is not finite. */
int gal_synth_array_phase(const double enu_m[3], double az_rad, double el_rad, uint32_t *phase);
/* Enqueue on the handle's stream: the n_elem (1 .. GAL_ARRAY_MAX_ELEM) element streams of the definition above, out of the n_parts
 * (1 .. GAL_ENGINE_MAX_CHAN) streams parts_dev[k] -- DEVICE memory, n_epochs x samples_per_epoch complex int16 samples each -- with
 * the weights rows[(e * n_elem + a) * n_parts + k] (HOST memory, copied before the call returns, as are both pointer arrays) into
 * out_dev[a] (DEVICE, the same size each).  Every part is read once, whatever n_elem is.  The rules of gal_synth_iq_wsum: 16-byte
 * alignment, GAL_E_STATE for a buffer of the batch in flight, gal_synth_iq_saturated is the fence and the counter; an output that
 * meets any part OR any other output is refused (parts may overlap each other).  A handle holds one weight table: a call waits (on
 * the host) for the kernel of the call before it.  GAL_E_INVAL for a null handle or pointer, a misaligned pointer, what
 * gal_synth_steer_check refuses, an overlap; GAL_E_NOMEM if the table cannot be had. */
int gal_synth_iq_array(gal_synth_t *h, const int16_t *const *parts_dev, int32_t n_parts, const gal_iq_steer_t *rows, int32_t n_epochs,
                       int32_t n_elem, int16_t *const *out_dev);
/* gal_synth_run_scint without echoes and with n_elem outputs: the batch of gal_synth_plan(params, n_epochs, state_in) as the n_elem
 * element streams out_dev[a] (HOST array of DEVICE pointers, 16-byte aligned, n_epochs x samples_per_epoch x 4 bytes each).  gain_q7 is
 * HOST [n_epochs][n_slots] as for gal_synth_run_gains, but at most 1023; phase is HOST [n_epochs][n_elem][n_slots], 2^-32 cycles
 * (gal_synth_array_phase).  EVERY slot that is active in any epoch of the batch is a group (a synthesis run) of its own, so that its
 * part is x_s itself; scintillation runs in place on the parts first if scint_rows is given (NULL: none); then gal_synth_iq_array is
 * enqueued with the weight gal_synth_steer_make(gain_q7[e][s], phase[e][a][s]) for slot s, element a in epoch e, and (0, 0) where the
 * slot is idle in e.  gal_synth_gain_runs counts the runs (an empty sky: one); state_out as for gal_synth_run_gains.  With n_elem = 1
 * and all phases 0 the output equals gal_synth_run_scint's bit for bit (it costs more runs).  The refusals are those of
 * gal_synth_run_scint and gal_synth_iq_array, and GAL_E_INVAL for a gain above 1023, with the slot and epoch in the text. */
int gal_synth_run_array(gal_synth_t *h, const gal_chan_epoch_t *params, int32_t n_epochs, const gal_chan_state_t *state_in,
                        const uint16_t *gain_q7, const uint32_t *phase, int32_t n_elem, const gal_iq_scint_t *scint_rows,
                        uint64_t first_sample, int16_t *const *out_dev, gal_chan_state_t *state_out);

/* Signal tables as the engine uses them (for tests and for the oracle to share DATA, not code). */
const uint32_t *gal_tables_e1b(void);   /* [50][128] */
const uint32_t *gal_tables_e1c(void);   /* [50][128] */
const int16_t  *gal_tables_cos512(void);/* [512]     */
const int16_t  *gal_tables_sin512(void);/* [512]     */
uint32_t        gal_tables_cs25(void);
const int32_t  *gal_tables_gauss(void); /* [32][32][2] = T of the noise floor (above); needs no GPU */
const int16_t  *gal_tables_cos1024(void);/* [1024] = C of the interference sources (above); needs no GPU */
const int32_t  *gal_tables_scint(void); /* [32] = h of the scintillation (above); needs no GPU */
const int32_t  *gal_tables_psd(void);   /* [2][4096] = C, then S, of the power spectrum (above); needs no GPU */

#ifdef __cplusplus
}
#endif
#endif /* GALSYNTH_H_ */
