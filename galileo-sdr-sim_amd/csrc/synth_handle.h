// synth_handle.h -- what the two host files of libgalsynth share: struct gal_synth (the handle of include/galsynth.h), the error
// return, HIP_TRY and the few questions both ask of a handle.  synth_api.cpp holds create / plan / execute / finish, iq_api.cpp the
// passes over the output stream (the output chain).  Internal: nothing here is part of the ABI, and nothing here depends on
// GAL_TEST_HOOKS -- iq_api.o is compiled once and linked into libgalsynth.so and libgalsynth_hooks.so alike.
#ifndef GAL_SYNTH_HANDLE_H_
#define GAL_SYNTH_HANDLE_H_

#include <cstddef>
#include <cstdint>
#include <vector>

#define GAL_SYNTH_NO_SIZED_MACROS 1
#include "synth_dev.h"

// Sets the calling thread's gal_synth_last_error text and returns `code` (synth_api.cpp).
__attribute__((visibility("hidden"))) int fail(int code, const char *fmt, ...);

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t err__ = (expr);                                                                 \
        if (err__ != hipSuccess)                                                                   \
            return fail(GAL_E_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(err__),   \
                        __FILE__, __LINE__);                                                       \
    } while (0)

constexpr int kDefaultPasses = 3;   // carrier passes enqueued up front for a NEW plan: walk + stitch (which translates on the spot), two spare --
                                    // no-op launches in front of k_synth when the chain is complete after one, as it is for four fresh
                                    // scenarios in five (tools/fresh_plan_probe.py, 32 seeds of M-SYN12: 26 x 1 pass, 4 x 2, 2 x 3; a batch that
                                    // needs more than were enqueued pays gal_synth_finish's iteration and a SECOND synthesis, 3.4 ms
                                    // instead of 1.9).  A plan that is executed again enqueues what its last execute needed (the chain
                                    // is deterministic); rounds 3-5 kept that count per HANDLE, right for a bench that re-executes one
                                    // resident plan and wrong for a caller with new parameters every batch

// What a plan produces on the host.  gal_synth_plan[_async] fills one of these (and the pinned staging buffer) WITHOUT touching what
// the batch in flight still needs; commit_staged() makes it the handle's plan and enqueues its upload -- at once if nothing is in
// flight, else at the next gal_synth_execute (behind the gal_synth_finish of the batch in flight): plan(k+1) under execute(k) on ONE
// handle (round 6).  Until the commit the device pointers of P are OFFSETS into the arena.
struct StagedPlan {
    DevPlan P{};
    int n_groups = 0, all_first = 0, all_count = 0, n_exact_records = 0, nact_max = 0;
    std::vector<int> group_nch, group_kind;
    std::vector<int64_t> act_prefix;
    size_t o_plan = 0, o_act = 0, o_nact = 0, up_bytes = 0, total = 0;
    size_t o_cpx = 0, o_ancw = 0, zero_end = 0, o_clmw = 0, clmw_bytes = 0, o_scanm = 0, scanm_clear = 0;
    int R = 0, nchunks = 0;
    float ms_plan = 0.0f;
};

// ---- the stages of the output chain (iq_api.cpp) -----------------------------------------------------------------------------------
// "The stage's last work on the device is done": an event, made at first need, and whether anybody has waited for it yet.  What a stage
// keeps on the device -- tables, histories, states, scratch -- belongs to its kernels (and uploads) in flight until wait() returns.
struct StageSync {
    hipEvent_t ev = nullptr;
    bool pending = false;
    hipError_t wait()
    {
        if (!pending) return hipSuccess;
        const hipError_t err = hipEventSynchronize(ev);
        if (err == hipSuccess) pending = false;
        return err;
    }
    hipError_t mark(hipStream_t st)
    {
        hipError_t err = ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (err == hipSuccess) err = hipEventRecord(ev, st);
        if (err == hipSuccess) pending = true;
        return err;
    }
    void destroy()
    {
        if (ev) hipEventDestroy(ev);
        ev = nullptr;
        pending = false;
    }
};

// A device buffer, with a pinned host twin of the same size where asked for, that grows when a call needs more than any call before it.
struct GrownBuf {
    char *dev = nullptr, *host = nullptr;
    size_t bytes = 0;
    // Room for `need` bytes.  Only where that takes a larger buffer: waits for `sync` (the kernels of the call before still use the old
    // one), frees, and allocates *cap = need + need / 4 + extra bytes.  GAL_OK; GAL_E_NOMEM with both pointers null, the HIP error
    // cleared and no message set (the caller words it, with *cap); GAL_E_DEVICE with its message where the wait failed.
    int reserve(uint64_t need, uint64_t extra, bool pinned, StageSync &sync, uint64_t *cap);
    void release()
    {
        if (dev) hipFree(dev);
        if (host) hipHostFree(host);
        dev = host = nullptr;
        bytes = 0;
    }
};

// gal_synth_fir_set / gal_synth_iq_fir (iq_fir.hip): d = the tap-pair table and the two history buffers of kFirHist complex samples, one
// device block; h_tab = the pinned copy of the table the upload reads
struct FirStage {
    uint32_t *d = nullptr, *h_tab = nullptr;
    int taps = 0, trips = 0, hs = 0;  // taps 0: no filter set
    int cur = 0;                      // the history buffer the next call reads (it writes the other)
    StageSync sync;
    void release()
    {
        if (d) hipFree(d);
        if (h_tab) hipHostFree(h_tab);
        d = h_tab = nullptr;
        taps = 0;
        sync.destroy();
    }
};

// gal_synth_firdec_set / gal_synth_iq_firdec (iq_firdec.hip): the same for the decimator; phase = the global index of the next input
// sample modulo decim
struct FirdecStage {
    uint32_t *d = nullptr, *h_tab = nullptr;
    int taps = 0, decim = 0, phase = 0;  // taps 0: no decimator set
    int cur = 0;
    StageSync sync;
    void release()
    {
        if (d) hipFree(d);
        if (h_tab) hipHostFree(h_tab);
        d = h_tab = nullptr;
        taps = 0;
        sync.destroy();
    }
};

// gal_synth_agc_set / gal_synth_iq_agc (iq_agc.hip): d = the two state buffers of kAgcState words (a call reads `cur` and writes the
// other); h_state = the pinned copy of the first state the upload reads; scratch = the block sums and gains of the last call; pos = the
// global index of the next sample
struct AgcStage {
    unsigned long long *d = nullptr, *h_state = nullptr;
    GrownBuf scratch;
    gal_iq_agc_t cfg = {};
    bool on = false;
    uint64_t pos = 0;
    int cur = 0;
    StageSync sync;
    void release()
    {
        if (d) hipFree(d);
        if (h_state) hipHostFree(h_state);
        d = h_state = nullptr;
        scratch.release();
        on = false;
        sync.destroy();
    }
};

// gal_synth_osc_set / gal_synth_iq_osc (iq_osc.hip): d = the two 64-bit words of the running sum Z (a call with s > 0 reads `cur` and
// writes the other); scratch = the tile sums and their scan of the last call; n0 = N0, pos = the global index of the next sample
struct OscStage {
    long long *d = nullptr;
    GrownBuf scratch;
    gal_iq_osc_t cfg = {};
    bool on = false;
    uint64_t n0 = 0, pos = 0;
    int cur = 0;
    StageSync sync;
    void release()
    {
        if (d) hipFree(d);
        d = nullptr;
        scratch.release();
        on = false;
        sync.destroy();
    }
};

// gal_synth_iq_wsum (iq_gain.hip): table = the part pointers ([GAL_ENGINE_MAX_CHAN]) and the gains ([n_epochs][n_parts] int32) of the
// last call, pinned on the host and on the device; sync = that call's kernel is done (both are free again)
struct GainStage {
    GrownBuf table;
    StageSync sync;
    void release()
    {
        table.release();
        sync.destroy();
    }
};

// gal_synth_iq_mpath (iq_echo.hip) and gal_synth_iq_refl (iq_refl.hip), which share all of it: d_hist = GAL_ECHO_LINES history lines
// x 2 buffers of GAL_ECHO_MAX_DELAY complex samples (a call reads buffer cur[id] of a line it names and writes the other); table = the table of the last call (part, history-in and history-out
// pointers, gains, echo rows, part indices), pinned on the host and on the device; sync = that call's kernels are done
struct MpathStage {
    uint32_t *d_hist = nullptr;
    uint8_t cur[GAL_ECHO_LINES] = {};
    GrownBuf table;
    StageSync sync;
    void release()
    {
        if (d_hist) hipFree(d_hist);
        d_hist = nullptr;
        table.release();
        sync.destroy();
    }
};

// gal_synth_iq_scint (iq_scint.hip): table = the job table of the last call (GAL_SCINT_MAX_JOBS jobs of 64 bytes as the kernel reads
// them), pinned on the host and on the device; sync = that call's kernel is done
struct ScintStage {
    GrownBuf table;
    StageSync sync;
    void release()
    {
        table.release();
        sync.destroy();
    }
};

// gal_synth_iq_array (iq_array.hip): table = the table of the last call (part pointers [GAL_ENGINE_MAX_CHAN], output pointers
// [GAL_ARRAY_MAX_ELEM], then the packed weights [n_epochs][n_parts][n_elem][2] words), pinned on the host and on the device; sync = that
// call's kernel is done
struct ArrayStage {
    GrownBuf table;
    StageSync sync;
    void release()
    {
        table.release();
        sync.destroy();
    }
};

struct gal_synth {
    StagedPlan staged;           // the plan made while a batch was in flight (or being committed)
    bool staged_pending = false;  // ... waits for its commit
    gal_synth_cfg_t cfg{};
    int device = 0;
    int n_cu = 256;  // compute units of the device (MI355X: 256)
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t aux_stream = nullptr;  // code-chain walk + page resolution run beside the carrier passes
    // the walker chain runs on the handle's own HIGH-PRIORITY stream: k_synth fills every SIMD's register file,
    // so walker workgroups of the next batch only get on when a synthesis wave retires -- with priority they
    // are first in line then, instead of queueing behind the pending synthesis workgroups of other handles
    hipStream_t walk_stream = nullptr;
    hipEvent_t ev_walk = nullptr;
    hipEvent_t ev_ver = nullptr;  // k_verify done (k_synth_g batches)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_prep = nullptr, ev_aux = nullptr;
    hipEvent_t ev_upd = nullptr;  // the plan's upload and memsets are complete (what the walkers of its first execute wait for)

    // tables in HBM
    int *d_lut = nullptr;
    uint32_t *d_str = nullptr;   // [50][512] half-chip streams (2 bits per BOC half chip)
    DevPlan *d_plan = nullptr;   // device copy of P, inside the arena (the hot kernel reads rarely used fields through it)
    char *h_up = nullptr;        // pinned staging buffer of plan(): the arena's upload region, byte for byte
    size_t h_up_bytes = 0;

    // arena for the planned batch
    void *arena = nullptr;
    size_t arena_bytes = 0;
    DevPlan P{};   // the planned batch
    DevPlan Pw{};  // what the walker kernels of the batch in flight see: P cut to the epochs [0, end of the executed range)
    bool planned = false;
    bool executed = false;
    bool in_flight = false;  // execute() enqueued, finish() not yet called
    int n_groups = 0;  // channel groups (each <= kKernelMaxChan) -> synth launches per execute
    std::vector<int> group_nch;
    std::vector<int> group_kind;     // 1: k_synth_g, 0: k_synth (k_synth_g batches: the records that are not fit for it, accumulating)
    int all_first = 0, all_count = 0;  // k_synth_g batches with records of kind 0: the groups that hold ALL records (list-overflow path)
    int n_exact_records = 0;         // records of the batch that take the exact-replay launch behind k_synth_g
    uint8_t *d_act = nullptr;  // [groups][E][kActRow]
    int *d_nact = nullptr;     // [groups][E]
    int nact_max = 0;
    uint32_t *last_iq = nullptr;
    int range_e0 = 0, range_ne = 0;  // epoch range of the last execute
    void *own_iq = nullptr;
    size_t own_iq_bytes = 0;
    void *own_pin = nullptr;  // gal_synth_run_host, small batches: pinned landing buffer of the device->host copy
    size_t own_pin_bytes = 0;
    int *h_ctr = nullptr;  // pinned: [CTR_COUNT] counters, [CTR_COUNT] spare, then the completion flag (k_publish)
    uint32_t *h_flag = nullptr;  // = (uint32_t *)(h_ctr + 2 * CTR_COUNT): sequence number of the last batch whose record is complete
    uint32_t seq = 0;            // sequence number of the batch in flight
    uint32_t scan_tag = 0;       // tag of the last stitch launched (k_scanm's look-back records carry it)
    size_t scanm_off = ~(size_t)0, scanm_clear = 0;  // where the stitch's records lie in the arena, as last cleared
    int64_t legs_walked = 0, legs_translated = 0, n_fallbacks = 0;  // last finish(): carrier legs walked / translated
    std::vector<int64_t> act_prefix;  // [E + 1] active records in the epochs before e (a first walker pass walks W legs of each)
    int64_t first_pass_legs = 0;      // legs walked by the first passes of the batch in flight (every active leg; not counted on the device)
    gal_chan_state_t *h_state = nullptr;  // pinned [S]
    bool state_fetched = false;           // h_state holds the state of the batch in flight
    gal_synth_stats_t stats{};
    int enq_passes = kDefaultPasses;  // carrier passes the next execute enqueues (see kDefaultPasses)
    int small_need = 2;               // ... what the handle's last plan of <= kSmallPlanEpochs epochs needed (its first: one spare)
    // k_synth's resampled-window body: per slot the last code step whose hold-pattern thresholds were examined and
    // their smallest distance (rw_threshold_gap) -- reused only for the identical step
    std::vector<double> rw_s0, rw_g0, rw_e0;
    // ... and, since round 6, for every step within rw_rad of it: the thresholds T_u = 1 - frac(u s) move by u |ds| <= 15 |ds| and no
    // u s crosses an integer while 15 |ds| stays below the distance of every T_u to 0 and 1 (rw_e0), so inside
    // |ds| < min((e0 - min) / 15, (g0 - min) / 14) both gates keep their verdict.  A Doppler moves the step of the reference geometry by
    // 2e-6 of itself, the radius is 6e-4: one evaluation per slot instead of one per record (14 388 x 0.3 us of a 1199-epoch plan)
    std::vector<double> rw_rad;
    bool host_only = false;       // GAL_TEST_HOOKS, gal_hooks_plan_host_ms: gal_synth_plan's host work without a device (timing on CPU)
    hipEvent_t ev_up0 = nullptr, ev_up1 = nullptr;  // around the upload of the last plan (timed: stats.ms_h2d)
    bool upload_pending = false;  // gal_synth_plan_async: the upload is enqueued, nobody has waited for it yet
    bool upload_timed = false;
    bool upload_unordered = false;  // ... and no execute has put its walkers behind it yet
    float ms_plan = 0.0f;         // host time of the last gal_synth_plan (validation, lists, staging; without the wait for the upload)
    double prev_wait_us = 0.0;  // how long the last gal_synth_finish waited for its batch (paces the next one's naps)
    int g_holdoff = 0;  // batches for which k_synth_g is not used although it could be: its last batch listed too many groups

    // the output chain (iq_api.cpp)
    unsigned long long *d_iq_sat = nullptr;  // the saturation counter of every pass (device; made at the first pass that may count)
    uint32_t *d_corr_tab = nullptr;  // gal_synth_correlate: [512] carrier table + [50][512] replica bits (device; made at the first call)
    void *own_parts = nullptr;  // gal_synth_run_gains / _run_mpath: the streams of the slot groups, one behind the other
    size_t own_parts_bytes = 0;
    int gain_runs = 0;          // ... synthesis runs the last call took (gal_synth_gain_runs)
    GainStage gain;
    MpathStage mp;
    FirStage fir;
    FirdecStage fd;
    AgcStage agc;
    OscStage osc;
    ScintStage scint;
    ArrayStage array;
};

// The stream the handle works on: the caller's (gal_synth_set_stream), or one of its own, made at first need.
static inline hipStream_t handle_stream(gal_synth *h)
{
    if (!h->stream) {
        if (!h->own_stream && hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) return nullptr;
        h->stream = h->own_stream;
    }
    return h->stream;
}

// [p, p + bytes) against the int16 output of the batch in flight (gal_synth_finish may still synthesise it again)
static inline bool hits_batch_in_flight(const gal_synth *h, const void *p, size_t bytes)
{
    if (!h->in_flight || !h->last_iq) return false;
    const char *x = (const char *)p, *y = x + bytes;
    const char *a = (const char *)h->last_iq, *b = a + (size_t)h->range_ne * (size_t)h->P.N * 4;
    return x < b && a < y;
}

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

#endif  // GAL_SYNTH_HANDLE_H_
