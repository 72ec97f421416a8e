// galileo-sdr-sim -- command-line front door with the reference's option surface and file format, so
// that reference command lines (README.md:63) run unchanged against the MI355X engine:
//
//   galileo-sdr-sim -e <rinex> [-l lat,lon,hgt | -u motion.csv] [-t YYYY/MM/DD,hh:mm:ss] [-d sec]
//                   [-o file|-] [-I x] [-U x] [-b x] [-v]
//
// Options follow src/main.cpp:216-326 (getopt string "e:n:o:u:g:l:T:t:d:G:a:p:iI:U:b:v"); USRP / bit
// streamer / UDP options are accepted and ignored (file sink only; -U/-b are therefore implied).  Output is
// the reference's `ishort` stream: headerless little-endian interleaved int16 I,Q at 2.6 MS/s, exactly
// ((int)(10 d + 0.5) - 1) * 260000 * 4 bytes (src/galileo-sdr.cpp:438,536-542); default name
// galileosim.ishort, "-" = stdout.  Errors print a message and exit(1); success exits 0.
// --iq-format ibyte|ibit (not in the reference; include/galsynth.h GAL_IQ_*): the same stream as 8-bit IQ (--iq-shift N, default 5)
// or 1-bit packed IQ, converted on the GPU behind each batch (gal_synth_iq_convert); half / a sixteenth of the bytes to move.
// --cn0 <dBHz> (not in the reference either): a seeded white Gaussian noise floor under the signals, in every format, mixed in on the
// GPU in the same pass (gal_synth_iq_convert_noise); the file is a fixed function of the command line, whatever the batch length.
// --jam js_db,f_hz[,f_hi_hz,sweep_us[,period_us,on_us]] (not in the reference), up to four times: CW, chirp or pulsed interference at
// a stated J/S, with or without --cn0, in that same pass (gal_synth_iq_convert_interf); again a fixed function of the command line.
//
// --power-model, --antenna <file>, --prn-power prn:dB[,...] (the reference computes such a gain per channel and epoch and leaves it
// commented out in its loop, src/galileo-sdr.cpp:469-477, 520-521): per-satellite signal power -- path loss, a receiver antenna pattern,
// per-PRN offsets -- as Q7 gains from the front-end (gal_scen_next_gains), applied by gal_synth_run_gains in front of noise,
// interference and the format.  Without the three options every byte is the reference's.
//
// --fir <file> | --fir-lowpass cutoff_hz[,n_taps] (not in the reference): a front-end (IF) FIR filter over the int16 stream, behind noise
// and interference and in front of the format (gal_synth_iq_fir); the file does not depend on -B.
//
// --oversample M (not in the reference): synthesis, gains, noise and interference at M x 2.6 MS/s, then ONE decimating FIR filter back to
// 2.6 MS/s (gal_synth_iq_firdec) in front of the format; --fir / --fir-lowpass then give the decimator's taps.
//
// --agc [target_rms], --iq-format i2bit (not in the reference): a block AGC in front of the quantiser, behind everything above, and the
// 2-bit format it makes possible (gal_synth_iq_agc); --agc-log <file> writes the gain of every block.
//
// --lo-offset hz[,drift_hz_per_s], --phase-noise h0 (not in the reference): the receiver's local oscillator -- a carrier offset, a drift and
// white-FM phase noise common to the whole stream, behind gains, --multipath, --cn0 and --jam and in front of --fir / the decimator, --agc
// and the format (gal_synth_iq_osc); the file does not depend on -B.
// --monitor <file> (not in the reference): the built-in receiver check -- every --monitor-every'th epoch (default 10) the first 25 code
// periods of every active channel are despread, in the buffer as it is written (behind noise and format), with the planned replica
// (gal_synth_correlate); one CSV line per (epoch, PRN) with the measured C/N0 and where the peak lies.  Read-only: the IQ is the same.
// --spectrum <file> (not in the reference): the other half of the self-check -- every --spectrum-every'th epoch (default 10) the Welch
// power spectrum of the epoch's 260 000 output samples, in the buffer as it is written (gal_synth_iq_psd: an exact integer transform;
// DESIGN.md section 24); one CSV line per reported epoch and the run's total.  Read-only: the IQ is the same.
//
// Pipeline: a producer thread runs the host front-end (libgalscen: orbits, ranges, I/NAV pages) up to two batches
// ahead -> the main thread plans and executes each batch on the GPU and, after gal_synth_finish(), enqueues the copy
// into one of two pinned buffers on two copy streams -> the sink moves full buffers into the output with sequential
// write()s.  (--writers n > 0: a regular file is sized up front and mapped instead, and n threads copy disjoint pieces of
// the pinned buffer into the mapping -- built to get past one core's copy speed, measured no faster once the unmap is
// counted: the kernel's page-cache insertion for ONE file does not scale with threads; kept as an option.)  In steady
// state the run time is that of the slowest stage: the device->host link for /dev/null, the page cache for a file.
//
// --sites <file>: BASELINE config 5 as a product entry point -- one line `lat,lon,hgt[,outfile]` per receiver site, one
// child process of this executable per site, spread over the GPUs of the node (GAL_DEVICE), every site's ishort file
// written on its own; the parent prints the aggregate.  This is the reference's way of doing it too: N independent
// usrp_galileo processes (src/main.cpp:168-408), nothing is exchanged between sites.
//
// Files: cli_options.h / .cpp -- the option table, argv -> Config with every refusal, the --sites parent; cli_sink.h -- the pinned
// slots and the output sink; this file -- the run: scenario, engine, buffers, the producer / main / writer pipeline, the report.
#include <hip/hip_runtime.h>
#include <signal.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>

#include "cli_options.h"
#include "cli_sink.h"

namespace {

using Clock = std::chrono::steady_clock;

// ---- --monitor ----------------------------------------------------------------------------------------------------
constexpr int kMonPeriods = 25;     // code periods looked at per monitored epoch (4 ms each: the epoch's first 0.1 s)
constexpr int kMonFarDelay = 2046;  // half chips: the noise tap, a quarter of a code period from the peak
constexpr double kMonBinHz = 250.0; // 1 / (4 ms)

struct MonEntry {  // one (epoch, channel): two requests -- delays -1, 0, +1 and the far delay, three Doppler bins each
    double t, f_carr;
    int prn;
    size_t off;  // of its sums in the batch's buffer, in int64
};
struct MonBatch {
    std::vector<MonEntry> entries;
    long long *dev = nullptr, *host = nullptr;  // sums: per entry [25][3][3][4] then [25][3][1][4]
    bool pending = false;
};
constexpr size_t kMonNear = (size_t)kMonPeriods * 3 * 3 * 4, kMonFar = (size_t)kMonPeriods * 3 * 1 * 4;  // int64 per request
struct MonSummary {
    int n = 0, off_peak = 0, no_peak = 0;
    double sum = 0.0, lo = 1e300, hi = -1e300;
};
struct MonRequests {  // of one batch's monitored epochs
    std::vector<gal_corr_req_t> reqs;
    std::vector<int> epoch;  // per pair of requests: the epoch's position in the batch
    std::vector<int> skip;   // ... and the samples skipped at its start (ibit: so that the address is 16-byte aligned)
};

// the lines of a batch whose sums have arrived (the stream has been waited for)
void monitor_flush(MonBatch &mb, FILE *fp, double sample_rate, const gal_corr_req_t &shape, MonSummary (&sum)[GAL_NUM_PRN + 1])
{
    for (const MonEntry &e : mb.entries) {
        // one [25][3][4][4] array: delays -1, 0, +1 and the far one
        std::vector<int64_t> all((size_t)kMonPeriods * 3 * 4 * 4);
        const long long *near = mb.host + e.off, *far = near + kMonNear;
        for (int m = 0; m < kMonPeriods; ++m)
            for (int d = 0; d < 3; ++d)
                for (int r = 0; r < 4; ++r) {
                    for (int k = 0; k < 3; ++k) all[(((size_t)m * 3 + d) * 4 + k) * 4 + r] = near[(((size_t)m * 3 + d) * 3 + k) * 4 + r];
                    all[(((size_t)m * 3 + d) * 4 + 3) * 4 + r] = far[((size_t)m * 3 + d) * 4 + r];
                }
        gal_corr_req_t q = shape;
        q.n_delay = 4;
        double cn0 = 0.0, ratio = 0.0, best = -1.0;
        const bool peak = gal_corr_cn0(all.data(), &q, 1, 3, 1, sample_rate, &cn0, &ratio) == GAL_OK;
        int bk = 0, bd = 0;
        for (int d = 0; d < 3; ++d)
            for (int k = 0; k < 3; ++k) {
                double p = 0.0;
                for (int m = 1; m < kMonPeriods - 1; ++m)
                    for (int r = 0; r < 4; ++r) {
                        const double v = (double)all[(((size_t)m * 3 + d) * 4 + k) * 4 + r];
                        p += v * v;
                    }
                if (p > best) best = p, bk = k - 1, bd = d - 1;
            }
        if (peak) fprintf(fp, "%.1f,%d,%.3f,%.2f,%.3f,%d,%d\n", e.t, e.prn, e.f_carr, cn0, ratio, bk, bd);
        else fprintf(fp, "%.1f,%d,%.3f,nan,%.3f,%d,%d\n", e.t, e.prn, e.f_carr, ratio, bk, bd);
        MonSummary &s = sum[e.prn];
        ++s.n;
        if (bk || bd) ++s.off_peak;
        if (!peak) ++s.no_peak;
        else {
            s.sum += cn0;
            s.lo = cn0 < s.lo ? cn0 : s.lo;
            s.hi = cn0 > s.hi ? cn0 : s.hi;
        }
    }
    mb.entries.clear();
    mb.pending = false;
}

// ---- --spectrum ---------------------------------------------------------------------------------------------------
struct SpecBatch {  // the reported epochs of one batch: per epoch N uint64 sums
    std::vector<int> epoch;  // index in the whole run
    std::vector<int32_t> n_seg;
    unsigned long long *dev = nullptr, *host = nullptr;
    void *d_line = nullptr;  // ibit: an epoch that begins 8 bytes off the 16-byte grid is copied here first
    bool pending = false;
};
typedef unsigned __int128 u128;
struct SpecTotal {
    std::vector<u128> p;  // natural bin order
    uint64_t n_seg = 0;
    int n_epochs = 0;
};

void print_u128(FILE *fp, u128 v)
{
    char buf[48];
    int i = sizeof(buf);
    buf[--i] = 0;
    do buf[--i] = (char)('0' + (int)(v % 10)), v /= 10;
    while (v);
    fputs(buf + i, fp);
}

// the lines of a batch whose sums have arrived (the stream has been waited for): frequency order, -fs / 2 first
void spectrum_flush(SpecBatch &sb, FILE *fp, int N, SpecTotal &tot)
{
    for (size_t i = 0; i < sb.epoch.size(); ++i) {
        const unsigned long long *p = sb.host + i * (size_t)N;
        fprintf(fp, "%.1f,%d", sb.epoch[i] * 0.1, sb.n_seg[i]);
        for (int k = 0; k < N; ++k) {
            const int b = (k + N / 2) & (N - 1);
            fprintf(fp, ",%llu", p[b]);
            tot.p[b] += p[b];
        }
        fputc('\n', fp);
        tot.n_seg += (uint64_t)sb.n_seg[i];
        ++tot.n_epochs;
    }
    sb.epoch.clear();
    sb.n_seg.clear();
    sb.pending = false;
}

// ---- what the three threads share -----------------------------------------------------------------------------------------------------
struct AgcLog {  // --agc-log: the gains of the blocks that start in a batch
    uint32_t *dev = nullptr, *host = nullptr;
    size_t n = 0;
    bool pending = false;
};

// One of the two batches in flight, with everything of it that lives on the device or in pinned memory.
// d_iq: the engine's int16 output; d_out: what the copies read -- d_iq itself for ishort (with --cn0: after the noise pass has run in
// place), d_fir behind a filter, a buffer of its own for every other format and behind the AGC (which does not run in place)
struct BatchSlot {
    int16_t *d_iq = nullptr, *d_fir = nullptr;
    void *d_out = nullptr;
    hipEvent_t converted = nullptr;  // the chain has run (Config::chain_on_engine_stream)
    Slot out;                        // pinned; `full` and `bytes` are the writer's hand-over, under SlotPair::mu
    MonBatch mon;                    // the main thread's alone, as are spec and agc_log
    SpecBatch spec;
    AgcLog agc_log;
};

// main thread -> writer thread: the main thread fills a slot that is not full and marks it full; the writer drains full slots in order
struct SlotPair {
    BatchSlot s[2];
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;                  // under mu: no batch follows
    std::atomic<bool> io_error{false};  // written by the writer, read by the main loop
};

// producer thread -> main thread: front-end rows, kBufs batches deep
struct RowRing {
    static constexpr int kBufs = 3;
    struct Buf {
        std::vector<gal_chan_epoch_t> rows;
        std::vector<uint16_t> gains;  // per-satellite signal power: [epochs][slots] Q7
        std::vector<double> azel;     // --array, --reflector: [epochs][slots][2] azimuth and elevation, radians
        bool ahead = false;           // --reflector: row n (one behind the batch) is the next batch's first epoch
        int n = 0;                    // epochs in it; < 0: front-end error, 0: end of the scenario
        bool ready = false;           // under mu: the producer's until ready, the main thread's until it clears it
    } buf[kBufs];
    std::mutex mu;
    std::condition_variable cv;
    bool consumer_gone = false;  // under mu
    std::string error;           // under mu, with n < 0
};

// --reflector: a batch with one epoch of look-ahead behind it, so that the last epoch's rows know the geometry of the epoch that
// follows (the phase runs from one epoch's start to the next; the file must not depend on -B).  The buffers hold batch_epochs + 1
// epochs; the look-ahead epoch is kept and opens the next batch.
struct LookAhead {
    std::vector<gal_chan_epoch_t> rows;
    std::vector<uint16_t> gains;
    std::vector<double> azel;
    bool have = false, ended = false;
    int next(gal_scen_t *scen, const Config &c, RowRing::Buf &b)
    {
        const size_t S = (size_t)c.sc.n_slots;
        b.ahead = false;
        if (ended) return 0;
        if (!have) {  // the scenario's first epoch
            const int n = gal_scen_next_azel(scen, 1, b.rows.data(), c.power_on ? b.gains.data() : nullptr, b.azel.data());
            if (n <= 0) return n;
        } else {
            std::copy(rows.begin(), rows.end(), b.rows.begin());
            std::copy(azel.begin(), azel.end(), b.azel.begin());
            if (c.power_on) std::copy(gains.begin(), gains.end(), b.gains.begin());
        }
        const int m = gal_scen_next_azel(scen, c.batch_epochs, b.rows.data() + S, c.power_on ? b.gains.data() + S : nullptr, b.azel.data() + 2 * S);
        if (m < 0) return m;
        if (m < c.batch_epochs) {  // the scenario ends inside this batch: 1 + m epochs, nothing behind them
            ended = true;
            return 1 + m;
        }
        rows.assign(b.rows.begin() + (size_t)m * S, b.rows.begin() + (size_t)(m + 1) * S);
        azel.assign(b.azel.begin() + 2 * (size_t)m * S, b.azel.begin() + 2 * (size_t)(m + 1) * S);
        if (c.power_on) gains.assign(b.gains.begin() + (size_t)m * S, b.gains.begin() + (size_t)(m + 1) * S);
        have = b.ahead = true;
        return m;
    }
};

void produce_rows(RowRing &ring, gal_scen_t *scen, const Config &c, Clock::time_point t_start)
{
    long produced_epochs = 0;
    LookAhead ahead;
    for (int w = 0;; w = (w + 1) % RowRing::kBufs) {
        RowRing::Buf &b = ring.buf[w];
        {
            std::unique_lock<std::mutex> lk(ring.mu);
            ring.cv.wait(lk, [&] { return !b.ready || ring.consumer_gone; });
            if (ring.consumer_gone) return;
        }
        // -r: FIFO-style pacing (the reference: src/fifo.cpp + src/galileo-sdr.cpp:570-595): epoch k is produced no earlier than
        // k * 0.1 s after the start, so that position updates are current
        if (c.realtime) std::this_thread::sleep_until(t_start + std::chrono::milliseconds(100) * produced_epochs);
        const int n = g_stop         ? 0
                      : c.refl_on()  ? ahead.next(scen, c, b)
                      : c.array_on() ? gal_scen_next_azel(scen, c.batch_epochs, b.rows.data(), c.power_on ? b.gains.data() : nullptr, b.azel.data())
                      : c.power_on   ? gal_scen_next_gains(scen, c.batch_epochs, b.rows.data(), b.gains.data())
                                   : gal_scen_next(scen, c.batch_epochs, b.rows.data());
        if (n > 0) produced_epochs += n;
        {
            std::lock_guard<std::mutex> lk(ring.mu);
            if (n < 0) ring.error = gal_scen_last_error();
            b.n = n;
            b.ready = true;
        }
        ring.cv.notify_all();
        if (n <= 0) return;
    }
}

// sinks: one per element (without --array: one)
void write_slots(SlotPair &sp, std::vector<Sink> &sinks)
{
    for (int next = 0;; next ^= 1) {
        Slot &s = sp.s[next].out;
        std::unique_lock<std::mutex> lk(sp.mu);
        sp.cv.wait(lk, [&] { return s.full || sp.done; });
        if (!s.full) return;
        lk.unlock();
        bool ok = hipEventSynchronize(s.copied[0]) == hipSuccess && hipEventSynchronize(s.copied[1]) == hipSuccess;
        for (int k = 0; k < s.n_elem && ok; ++k) ok = sinks[k].put((const char *)s.host + (size_t)k * s.stride, s.bytes);
        if (!ok) sp.io_error = true;
        lk.lock();
        s.full = false;
        lk.unlock();
        sp.cv.notify_all();
    }
}

// ---- the main thread's own -----------------------------------------------------------------------------------------------------------------
struct Run {
    const Config &c;
    gal_synth_t *eng = nullptr;
    gal_synth_cfg_t cfg;
    hipStream_t stream = nullptr, copy_stream[2] = {nullptr, nullptr};
    size_t epoch_bytes = 0, batch_bytes = 0;  // in the output format
    int K = 1;                                // --array: elements; their batches lie iq_stride (int16) / out_stride (format) bytes apart
    size_t iq_stride = 0, out_stride = 0;
    std::vector<uint16_t> ar_gains;           // --array: the batch's gains [epochs][slots] and phases [epochs][elements][slots]
    std::vector<uint32_t> ar_phase;
    int emitted = 0;                          // epochs handed to the writer
    std::vector<gal_chan_state_t> state;
    bool have_state = false;
    int prn_gain_lo[GAL_NUM_PRN + 1], prn_gain_hi[GAL_NUM_PRN + 1];  // per-satellite signal power: the gains each PRN was given
    std::vector<uint16_t> mp_gains;      // --multipath: the batch's gains [epochs][slots] ...
    std::vector<gal_iq_echo_t> mp_rows;  // ... its echo table [epochs][echoes in view] ...
    std::vector<int32_t> slot_of;        // ... and per echo in view its slot and its line of the file
    std::vector<const EchoSpec *> spec_of;
    std::vector<gal_iq_scint_t> sc_rows;  // --scint: the batch's rows [epochs][slots]
    std::vector<gal_iq_refl_t> rf_rows;   // --reflector: the rows [epochs][slots with echoes x reflectors] of one call
    gal_corr_req_t mon_shape;  // what every monitor request shares
    MonSummary mon_sum[GAL_NUM_PRN + 1];
    SpecTotal spec_total;
    uint64_t agc_logged = 0;  // blocks written to the log
    std::string err;          // why the loop was left; reported once, behind it

    explicit Run(const Config &cfg_) : c(cfg_) {}
    bool fail(const char *fmt, ...)
    {
        char buf[1024];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        err = buf;
        return false;
    }
    bool lib_fail() { return fail("%s", gal_synth_last_error()); }
    void note_gains(const gal_chan_epoch_t *rows, const uint16_t *g, size_t count)  // the summary's per-PRN range
    {
        for (size_t i = 0; i < count; ++i) {
            const int prn = rows[i].prn;
            if (prn < 1 || prn > GAL_NUM_PRN) continue;
            prn_gain_lo[prn] = g[i] < prn_gain_lo[prn] ? g[i] : prn_gain_lo[prn];
            prn_gain_hi[prn] = g[i] > prn_gain_hi[prn] ? g[i] : prn_gain_hi[prn];
        }
    }
    // the lines of a batch whose gains have arrived (the stream has been waited for)
    void agc_log_flush(AgcLog &l)
    {
        for (size_t k = 0; k < l.n; ++k, ++agc_logged)
            fprintf(c.agc_log_fp, "%.9f,%u,%.4f\n", (double)agc_logged * (double)c.agc_block / kOutRate, l.host[k], 20.0 * log10((double)l.host[k] / 4096.0));
        l.pending = false;
    }
};

// every device and pinned buffer of the two slots; false: an allocation failed
bool alloc_slots(const Run &r, SlotPair &sp)
{
    const Config &c = r.c;
    for (BatchSlot &b : sp.s) {
        if (hipMalloc((void **)&b.d_iq, r.iq_stride * r.K) != hipSuccess ||
            hipHostMalloc((void **)&b.out.host, r.out_stride * r.K, hipHostMallocDefault) != hipSuccess)
            return false;
        b.out.n_elem = r.K;
        b.out.stride = r.out_stride;
        b.d_out = b.d_iq;
        if (c.fir_on()) {  // the filtered int16 batch, which then is what the format conversion (ishort: the copies) reads
            if (hipMalloc((void **)&b.d_fir, (size_t)kOutSamplesPerEpoch * 4 * c.batch_epochs) != hipSuccess) return false;
            b.d_out = b.d_fir;
        }
        if ((c.iq_format != GAL_IQ_ISHORT || c.agc_on) && hipMalloc(&b.d_out, r.out_stride * r.K) != hipSuccess) return false;
        if (c.chain_on_engine_stream() && hipEventCreateWithFlags(&b.converted, hipEventDisableTiming) != hipSuccess) return false;
        hipEventCreate(&b.out.copied[0]);
        hipEventCreate(&b.out.copied[1]);
    }
    // --monitor: per batch slot the sums of its monitored epochs, on the device and pinned on the host
    const size_t mon_epochs_max = (size_t)(c.batch_epochs + c.monitor_every - 1) / c.monitor_every + 1;
    const size_t mon_bytes = mon_epochs_max * r.cfg.n_slots * (kMonNear + kMonFar) * sizeof(long long);
    if (c.monitor_fp)
        for (BatchSlot &b : sp.s)
            if (hipMalloc((void **)&b.mon.dev, mon_bytes) != hipSuccess || hipHostMalloc((void **)&b.mon.host, mon_bytes, hipHostMallocDefault) != hipSuccess)
                return false;
    // --spectrum: per batch slot the sums of its reported epochs, on the device and pinned on the host
    if (c.spectrum_fp) {
        const size_t spec_bytes = ((size_t)(c.batch_epochs + c.spectrum_every - 1) / c.spectrum_every + 1) * (sizeof(unsigned long long) << c.spectrum.log2_n);
        for (BatchSlot &b : sp.s)
            if (hipMalloc((void **)&b.spec.dev, spec_bytes) != hipSuccess || hipHostMalloc((void **)&b.spec.host, spec_bytes, hipHostMallocDefault) != hipSuccess ||
                (c.iq_format == GAL_IQ_IBIT && hipMalloc(&b.spec.d_line, r.epoch_bytes + 16) != hipSuccess))
                return false;
    }
    // --agc-log: per batch slot the gains of the blocks that start in it, on the device and pinned on the host
    const size_t g_bytes = ((size_t)c.batch_epochs * kOutSamplesPerEpoch / (size_t)c.agc_block + 2) * sizeof(uint32_t);
    if (c.agc_log_fp)
        for (BatchSlot &b : sp.s)
            if (hipMalloc((void **)&b.agc_log.dev, g_bytes) != hipSuccess || hipHostMalloc((void **)&b.agc_log.host, g_bytes, hipHostMallocDefault) != hipSuccess)
                return false;
    return true;
}

// --monitor: the requests of this batch's monitored epochs, made while the rows are still ours
MonRequests monitor_requests(const Run &r, const gal_chan_epoch_t *rows, int n, MonBatch &mb)
{
    const Config &c = r.c;
    MonRequests out;
    for (int e = 0; e < n; ++e) {
        if ((r.emitted + e) % c.monitor_every) continue;
        const size_t ob = c.out_bytes((size_t)e * kOutSamplesPerEpoch);
        int skip = c.iq_format == GAL_IQ_IBIT ? (int)((16 - ob % 16) % 16) * 4 : 0;
        if (c.fir_on() && skip < c.fir_delay) {  // the filtered stream lags by fir_delay: start there or later, on the same 16-byte grid
            const int g = c.iq_format == GAL_IQ_IBIT ? 64 : c.iq_format == GAL_IQ_IBYTE ? 8 : 4;  // samples per 16 bytes
            skip += (c.fir_delay - skip + g - 1) / g * g;
        }
        for (int s = 0; s < r.cfg.n_slots; ++s) {
            const gal_chan_epoch_t &rec = rows[(size_t)e * r.cfg.n_slots + s];
            if (rec.prn <= 0) continue;
            gal_corr_req_t q = r.mon_shape;
            if (gal_corr_from_epoch(&rec, kOutRate, skip - c.fir_delay, &q) != GAL_OK) continue;  // (a record the monitor cannot follow)
            if (c.osc_on) {
                // the replica follows the oscillator's offset and drift: its step at the window's first sample -- counted at the
                // rate the oscillator runs at, and where the filters' delay puts that sample -- times the M samples of that rate
                // in one of the output (the drift inside the window of 0.1 s is not followed: 0.2 Hz at 2 Hz/s)
                const int64_t off = ((int64_t)skip - c.fir_delay) * c.osr;
                const uint64_t n_lo = (uint64_t)(r.emitted + e) * (uint64_t)r.cfg.samples_per_epoch + (uint64_t)(off > 0 ? off : 0);
                int32_t lo_step = 0;
                gal_synth_osc_lo_step(&c.osc, n_lo, &lo_step);
                q.carr_dph = (int32_t)((uint32_t)q.carr_dph + (uint32_t)c.osr * (uint32_t)lo_step);
            }
            MonEntry me;
            me.t = (r.emitted + e) * 0.1;
            me.f_carr = rec.f_carr;
            me.prn = rec.prn;
            me.off = mb.entries.size() * (kMonNear + kMonFar);
            mb.entries.push_back(me);
            q.delay0 = -1;
            q.n_delay = 3;
            out.reqs.push_back(q);
            q.delay0 = kMonFarDelay;
            q.n_delay = 1;
            out.reqs.push_back(q);
            out.epoch.push_back(e);
            out.skip.push_back(skip);
        }
    }
    return out;
}

// behind the conversion, on the same stream, in the buffer the copies read: one call per monitored epoch
bool enqueue_monitor(Run &r, BatchSlot &b, const MonRequests &m)
{
    bool ok = true;
    for (size_t i = 0, j = 0; i < m.epoch.size() && ok; i = j) {
        while (j < m.epoch.size() && m.epoch[j] == m.epoch[i]) ++j;
        const size_t ob = r.c.out_bytes((size_t)m.epoch[i] * kOutSamplesPerEpoch) + r.c.out_bytes((size_t)m.skip[i]);
        ok = gal_synth_correlate(r.eng, (const char *)b.d_out + ob, r.c.iq_format, (size_t)kOutSamplesPerEpoch - m.skip[i], &m.reqs[2 * i],
                                 (int32_t)(2 * (j - i)), (int64_t *)(b.mon.dev + b.mon.entries[i].off)) == GAL_OK;
    }
    if (!ok || hipMemcpyAsync(b.mon.host, b.mon.dev, b.mon.entries.size() * (kMonNear + kMonFar) * sizeof(long long), hipMemcpyDeviceToHost,
                              r.stream) != hipSuccess)
        return r.fail("monitor: %s", ok ? "copy of the sums failed" : gal_synth_last_error());
    b.mon.pending = true;
    return true;
}

// --spectrum: behind the conversion, on the same stream, in the buffer the copies read: one call per reported epoch, always the whole
// epoch, so that the file does not depend on -B
bool enqueue_spectrum(Run &r, BatchSlot &b, int n)
{
    const Config &c = r.c;
    SpecBatch &sb = b.spec;
    const size_t N = (size_t)1 << c.spectrum.log2_n;
    for (int e = 0; e < n; ++e) {
        if ((r.emitted + e) % c.spectrum_every) continue;
        const void *src = (const char *)b.d_out + c.out_bytes((size_t)e * kOutSamplesPerEpoch);
        if ((uintptr_t)src & 15) {  // (ibit, an odd epoch of the batch: 65 000 bytes per epoch)
            if (hipMemcpyAsync(sb.d_line, src, r.epoch_bytes, hipMemcpyDeviceToDevice, r.stream) != hipSuccess) return r.fail("spectrum: copy of the epoch failed");
            src = sb.d_line;
        }
        int32_t n_seg = 0;
        if (gal_synth_iq_psd(r.eng, src, c.iq_format, (size_t)kOutSamplesPerEpoch, &c.spectrum, (uint64_t *)(sb.dev + sb.epoch.size() * N), &n_seg) != GAL_OK)
            return r.fail("spectrum: %s", gal_synth_last_error());
        sb.epoch.push_back(r.emitted + e);
        sb.n_seg.push_back(n_seg);
    }
    if (sb.epoch.empty()) return true;
    if (hipMemcpyAsync(sb.host, sb.dev, sb.epoch.size() * N * sizeof(unsigned long long), hipMemcpyDeviceToHost, r.stream) != hipSuccess)
        return r.fail("spectrum: copy of the sums failed");
    sb.pending = true;
    return true;
}

// ---- the three synthesis paths: a batch of rows into d_iq; the library's code ---------------------------------------------------------------
// plain: plan + execute; the IQ is final once the loop has called gal_synth_finish
int synth_plain(Run &r, const RowRing::Buf &rows, int n, int16_t *d_iq)
{
    const int rc = gal_synth_plan(r.eng, rows.rows.data(), n, r.have_state ? r.state.data() : nullptr);
    return rc != GAL_OK ? rc : gal_synth_execute(r.eng, d_iq);
}

// per-satellite signal power: one synthesis run per group of slots with equal gains, finished when the call returns, and the weighted
// sum enqueued on the engine's stream behind them (include/galsynth.h)
int synth_gains(Run &r, const RowRing::Buf &rows, int n, int16_t *d_iq)
{
    r.note_gains(rows.rows.data(), rows.gains.data(), (size_t)n * r.cfg.n_slots);
    return gal_synth_run_gains(r.eng, rows.rows.data(), n, r.have_state ? r.state.data() : nullptr, rows.gains.data(), d_iq, r.state.data());
}

// --multipath: the gains of --power-model and its kin, or unity; an echo goes to the slot that carries its PRN in this batch (a PRN that
// is not in view: no echo), with a row per epoch from the slot's gain and the epoch's index in the whole stream
int synth_mpath(Run &r, const RowRing::Buf &rows, int n, int16_t *d_iq)
{
    const int S = r.cfg.n_slots;
    const gal_chan_epoch_t *rec = rows.rows.data();
    if (r.c.power_on) {
        r.mp_gains.assign(rows.gains.begin(), rows.gains.begin() + (size_t)n * S);
        r.note_gains(rec, r.mp_gains.data(), (size_t)n * S);
    } else {
        r.mp_gains.assign((size_t)n * S, (uint16_t)GAL_GAIN_UNITY);
    }
    r.slot_of.clear();
    r.spec_of.clear();
    for (const EchoSpec &e : r.c.echoes) {
        int slot = -1;
        for (size_t i = 0; i < (size_t)n * S && slot < 0; ++i)
            if (rec[i].prn == e.prn) slot = (int)(i % S);
        if (slot < 0) continue;
        r.slot_of.push_back(slot);
        r.spec_of.push_back(&e);
    }
    const int n_echo = (int)r.slot_of.size();
    r.mp_rows.assign((size_t)n * (n_echo > 0 ? n_echo : 1), gal_iq_echo_t{});
    for (int e = 0; e < n; ++e)
        for (int k = 0; k < n_echo; ++k) {
            const size_t i = (size_t)e * S + r.slot_of[k];
            const bool here = rec[i].prn == r.spec_of[k]->prn;  // (the slot carries another satellite, or none, in this epoch: A = 0)
            const int rc = gal_synth_mpath_row(&r.spec_of[k]->echo, here ? r.mp_gains[i] : 0, (uint64_t)(r.emitted + e), r.cfg.samples_per_epoch,
                                               &r.mp_rows[(size_t)e * n_echo + k]);
            if (rc != GAL_OK) return rc;
        }
    // --scint: the row of the PRN a slot carries in the epoch; every other record the identity
    if (r.c.sc_on()) {
        gal_iq_scint_t ident;
        memset(&ident, 0, sizeof(ident));
        ident.seed = 1, ident.node_len = GAL_SCINT_MIN_NODE, ident.a_q12 = 4096;
        r.sc_rows.assign((size_t)n * S, ident);
        for (size_t i = 0; i < (size_t)n * S; ++i)
            for (const ScintSpec &s : r.c.scints)
                if (rec[i].prn == s.prn) r.sc_rows[i] = s.row;
    }
    return gal_synth_run_scint(r.eng, rec, n, r.have_state ? r.state.data() : nullptr, r.mp_gains.data(), r.slot_of.data(), r.mp_rows.data(), n_echo,
                               r.c.sc_on() ? r.sc_rows.data() : nullptr, (uint64_t)r.emitted * (uint64_t)r.cfg.samples_per_epoch, d_iq, r.state.data());
}

// --reflector: the gains of --power-model and its kin, or unity; every slot that carries an admitted satellite has one echo per
// reflector, with the rows of gal_synth_refl_geom / _row from the epoch's azimuth and elevation and the next epoch's (the batch's last
// epoch: the look-ahead row behind it).  The batch is cut into calls where the set of such slots changes, so that a call's table
// holds exactly reflectors x satellites columns: any cut into whole epochs gives the bytes of one call, and a slot's history line is
// written in every call in which it carries an echo
int synth_refl(Run &r, const RowRing::Buf &rows, int n, int16_t *d_iq)
{
    const Config &c = r.c;
    const int S = r.cfg.n_slots, R = (int)c.refls.size();
    const gal_chan_epoch_t *rec = rows.rows.data();
    if (c.power_on) {
        r.mp_gains.assign(rows.gains.begin(), rows.gains.begin() + (size_t)n * S);
        r.note_gains(rec, r.mp_gains.data(), (size_t)n * S);
    } else {
        r.mp_gains.assign((size_t)n * S, (uint16_t)GAL_GAIN_UNITY);
    }
    const auto echoes_in = [&](int e, int s) { const int prn = rec[(size_t)e * S + s].prn; return prn >= 1 && prn <= GAL_NUM_PRN && c.refl_prn[prn]; };
    const auto same_set = [&](int e0, int e1) {
        for (int s = 0; s < S; ++s)
            if (echoes_in(e0, s) != echoes_in(e1, s)) return false;
        return true;
    };
    for (int e0 = 0, e1; e0 < n; e0 = e1) {
        for (e1 = e0 + 1; e1 < n && same_set(e0, e1);) ++e1;
        r.slot_of.clear();
        for (int s = 0; s < S; ++s)
            for (int k = 0; k < R && echoes_in(e0, s); ++k) r.slot_of.push_back(s);
        const int n_echo = (int)r.slot_of.size();
        if (n_echo > GAL_ECHO_MAX) {
            r.fail("--reflector: %d reflectors x %d satellites = %d echoes in epoch %d (%.1f s), more than %d: use --reflector-prn", R, n_echo / R, n_echo,
                   r.emitted + e0, (r.emitted + e0) * 0.1, GAL_ECHO_MAX);
            return GAL_E_INVAL;
        }
        r.rf_rows.assign((size_t)(e1 - e0) * (n_echo > 0 ? n_echo : 1), gal_iq_refl_t{});
        for (int e = e0; e < e1; ++e)
            for (int j = 0; j < n_echo; ++j) {
                const int s = r.slot_of[j], k = j % R;
                const size_t i = (size_t)e * S + s, i1 = i + S;  // i1: the same slot one epoch on, inside the batch or the look-ahead row
                const ReflSpec &f = c.refls[k];
                double now = -1.0, next = -1.0;
                int rc = gal_synth_refl_geom(f.kind, f.p, rows.azel[2 * i], rows.azel[2 * i + 1], &now);
                if (rc == GAL_OK && (e + 1 < n || rows.ahead) && rec[i1].prn == rec[i].prn)
                    rc = gal_synth_refl_geom(f.kind, f.p, rows.azel[2 * i1], rows.azel[2 * i1 + 1], &next);
                gal_iq_refl_t &row = r.rf_rows[(size_t)(e - e0) * n_echo + j];
                if (rc == GAL_OK) rc = gal_synth_refl_row(now, next, f.rel_db, f.phase_deg, c.sample_rate(), r.cfg.samples_per_epoch, r.mp_gains[i], &row);
                if (rc != GAL_OK) return rc;
                if (c.refl_log_fp)
                    fprintf(c.refl_log_fp, "%.1f,%d,%d,%.9f,%u,%u,%u,%u,%d\n", (r.emitted + e) * 0.1, rec[i].prn, k, now, row.delay, row.frac_q12, row.ph0, row.gain_q7,
                            row.dph);
            }
        const int rc = gal_synth_run_refl(r.eng, rec + (size_t)e0 * S, e1 - e0, r.have_state || e0 > 0 ? r.state.data() : nullptr,
                                          r.mp_gains.data() + (size_t)e0 * S, r.slot_of.data(), r.rf_rows.data(), n_echo,
                                          d_iq + (size_t)e0 * r.cfg.samples_per_epoch * 2, r.state.data());
        if (rc != GAL_OK) return rc;
    }
    return GAL_OK;
}

// --array: every active satellite a run of its own, then the array pass into the K element batches that lie one behind the other in
// d_iq.  The gains are those of --power-model and its kin, or unity; the phases come from the front-end's azimuth and elevation
int synth_array(Run &r, const RowRing::Buf &rows, int n, int16_t *d_iq)
{
    const Config &c = r.c;
    const int S = r.cfg.n_slots, K = r.K;
    const gal_chan_epoch_t *rec = rows.rows.data();
    if (c.power_on) {
        r.ar_gains.assign(rows.gains.begin(), rows.gains.begin() + (size_t)n * S);
        r.note_gains(rec, r.ar_gains.data(), (size_t)n * S);
    } else {
        r.ar_gains.assign((size_t)n * S, (uint16_t)GAL_GAIN_UNITY);
    }
    r.ar_phase.assign((size_t)n * K * S, 0u);
    for (int e = 0; e < n; ++e)
        for (int s = 0; s < S; ++s) {
            const size_t i = (size_t)e * S + s;
            if (rec[i].prn <= 0) continue;
            const double az = rows.azel[2 * i], el = rows.azel[2 * i + 1];
            if (c.array_log_fp) fprintf(c.array_log_fp, "%.1f,%d,%.4f,%.4f", (r.emitted + e) * 0.1, rec[i].prn, az * 57.29577951308232, el * 57.29577951308232);
            for (int a = 0; a < K; ++a) {
                uint32_t ph = 0;
                const int rc = gal_synth_array_phase(c.array[a].enu, az, el, &ph);
                if (rc != GAL_OK) return rc;
                r.ar_phase[((size_t)e * K + a) * S + s] = ph;
                if (c.array_log_fp) fprintf(c.array_log_fp, ",%u", ((ph + (1u << 21)) >> 22) & 1023u);
            }
            if (c.array_log_fp) fputc('\n', c.array_log_fp);
        }
    if (c.sc_on()) {
        gal_iq_scint_t ident;
        memset(&ident, 0, sizeof(ident));
        ident.seed = 1, ident.node_len = GAL_SCINT_MIN_NODE, ident.a_q12 = 4096;
        r.sc_rows.assign((size_t)n * S, ident);
        for (size_t i = 0; i < (size_t)n * S; ++i)
            for (const ScintSpec &sp : c.scints)
                if (rec[i].prn == sp.prn) r.sc_rows[i] = sp.row;
    }
    int16_t *outs[GAL_ARRAY_MAX_ELEM];
    for (int a = 0; a < K; ++a) outs[a] = (int16_t *)((char *)d_iq + (size_t)a * r.iq_stride);
    return gal_synth_run_array(r.eng, rec, n, r.have_state ? r.state.data() : nullptr, r.ar_gains.data(), r.ar_phase.data(), K,
                               c.sc_on() ? r.sc_rows.data() : nullptr, (uint64_t)r.emitted * (uint64_t)r.cfg.samples_per_epoch, outs, r.state.data());
}

// ---- the output chain behind a batch, on the engine's stream ------------------------------------------------------------------------------------
//   1. noise and interference, in place        2. the oscillator, in place
//   3. --fir or the decimator into d_fir       4. the AGC or the format conversion into d_out
// Every stage's state (filter history, AGC window, oscillator phase) runs on from batch to batch inside the handle; first_sample is the
// running sample count, so the file does not depend on the batch length.
bool run_chain(Run &r, BatchSlot &b, int n)
{
    const Config &c = r.c;
    // --oversample: the batch is n x M x 260 000 samples up to the decimator, which keeps n x 260 000 of them
    const size_t n_samples = (size_t)n * r.cfg.samples_per_epoch, n_kept = (size_t)n * kOutSamplesPerEpoch;
    const uint64_t first_sample = (uint64_t)r.emitted * (uint64_t)r.cfg.samples_per_epoch;
    if (c.array_on()) {
        // every element on its own through the one fused pass: the SAME sigma and signal gain, a noise stream of its own
        // (8 x --noise-stream + k), and its copy of every --jam source at the phase its direction of arrival gives it at the element
        if (c.iq_format == GAL_IQ_ISHORT && !c.mix_on()) return true;
        for (int k = 0; k < r.K; ++k) {
            gal_iq_noise_t nz = c.noise;
            nz.stream = 8u * c.noise.stream + (uint32_t)k;
            gal_iq_interf_t src[GAL_INTERF_MAX];
            for (int j = 0; j < c.n_jam; ++j) {
                uint32_t ph = 0;
                if (gal_synth_array_phase(c.array[k].enu, c.jam_az[j], c.jam_el[j], &ph) != GAL_OK) return r.lib_fail();
                src[j] = c.interf[j];
                src[j].ph0 += ph;
            }
            if (gal_synth_iq_convert_interf(r.eng, (const int16_t *)((const char *)b.d_iq + (size_t)k * r.iq_stride), n_samples, first_sample,
                                            c.mix_on() ? &nz : NULL, src, c.n_jam, c.iq_format, c.iq_shift, (char *)b.d_out + (size_t)k * r.out_stride) != GAL_OK)
                return r.lib_fail();
        }
        return true;
    }
    if (!c.fir_on() && !c.agc_on && !c.osc_on) {
        // nothing needs the int16 stream between the noise and the format: ONE fused pass does both (ishort: in place in d_iq).
        // (without --cn0, `noise` still carries the signal gain of the --jam sources; with neither the library converts plainly)
        if (c.iq_format == GAL_IQ_ISHORT && !c.mix_on()) return true;  // the reference's stream as it is: the copies read d_iq
        return gal_synth_iq_convert_interf(r.eng, b.d_iq, n_samples, first_sample, c.mix_on() ? &c.noise : NULL, c.interf, c.n_jam, c.iq_format,
                                           c.iq_shift, b.d_out) == GAL_OK || r.lib_fail();
    }
    if (c.mix_on() && gal_synth_iq_convert_interf(r.eng, b.d_iq, n_samples, first_sample, &c.noise, c.interf, c.n_jam, GAL_IQ_ISHORT, 0, b.d_iq) != GAL_OK)
        return r.lib_fail();
    if (c.osc_on && gal_synth_iq_osc(r.eng, b.d_iq, n_samples, b.d_iq) != GAL_OK) return r.lib_fail();
    const int16_t *x = b.d_iq;  // the int16 stream the last stage reads, n_kept samples of it
    if (c.dec_on()) {
        size_t got = 0;
        if (gal_synth_iq_firdec(r.eng, b.d_iq, n_samples, b.d_fir, &got) != GAL_OK) return r.lib_fail();
        if (got != n_kept) return r.fail("the decimator kept %zu samples of the batch, not %zu", got, n_kept);
        x = b.d_fir;
    } else if (c.fir_on()) {
        if (gal_synth_iq_fir(r.eng, b.d_iq, n_samples, b.d_fir) != GAL_OK) return r.lib_fail();
        x = b.d_fir;
    }
    if (c.agc_on) {
        if (gal_synth_iq_agc(r.eng, x, n_kept, c.iq_format, c.agc_param(), b.d_out, b.agc_log.dev, &b.agc_log.n) != GAL_OK) return r.lib_fail();
    } else if (c.iq_format != GAL_IQ_ISHORT) {  // (ishort: the copies read x itself)
        if (gal_synth_iq_convert(r.eng, x, n_kept, c.iq_format, c.iq_shift, b.d_out) != GAL_OK) return r.lib_fail();
    }
    return true;
}

// device -> host in two halves on the two copy streams, split at an epoch boundary: epoch_bytes is whole bytes in every format
bool enqueue_copies(Run &r, BatchSlot &b, int n)
{
    if (r.K > 1 || r.c.array_on()) {  // --array: every element's batch, the elements alternating between the two copy streams
        hipError_t cerr = hipSuccess;
        for (int k = 0; k < r.K && cerr == hipSuccess; ++k)
            cerr = hipMemcpyAsync((char *)b.out.host + (size_t)k * r.out_stride, (const char *)b.d_out + (size_t)k * r.out_stride, b.out.bytes,
                                  hipMemcpyDeviceToHost, r.copy_stream[k & 1]);
        for (int k = 0; k < 2 && cerr == hipSuccess; ++k) cerr = hipEventRecord(b.out.copied[k], r.copy_stream[k]);
        return cerr == hipSuccess || r.fail("device -> host copy failed: %s", hipGetErrorString(cerr));
    }
    const size_t half = r.epoch_bytes * (size_t)((n + 1) / 2);
    const size_t part[2] = {half, b.out.bytes - half};
    size_t off = 0;
    hipError_t cerr = hipSuccess;
    for (int k = 0; k < 2; ++k) {
        if (part[k] && cerr == hipSuccess)
            cerr = hipMemcpyAsync((char *)b.out.host + off, (const char *)b.d_out + off, part[k], hipMemcpyDeviceToHost, r.copy_stream[k]);
        if (cerr == hipSuccess) cerr = hipEventRecord(b.out.copied[k], r.copy_stream[k]);
        off += part[k];
    }
    return cerr == hipSuccess || r.fail("device -> host copy failed: %s", hipGetErrorString(cerr));
}

// what follows a batch's synthesis: the chain, the side outputs, the copies
bool finish_batch(Run &r, BatchSlot &b, int n, const MonRequests &mon)
{
    const Config &c = r.c;
    b.out.bytes = r.epoch_bytes * n;
    if (!run_chain(r, b, n)) return false;
    if (c.agc_log_fp) {  // behind the AGC, on the same stream
        if (b.agc_log.n && hipMemcpyAsync(b.agc_log.host, b.agc_log.dev, b.agc_log.n * sizeof(uint32_t), hipMemcpyDeviceToHost, r.stream) != hipSuccess)
            return r.fail("AGC log: copy of the gains failed");
        b.agc_log.pending = true;
    }
    if (c.chain_on_engine_stream() &&  // what the copies read is enqueued on the engine's stream: they wait for it
        (hipEventRecord(b.converted, r.stream) != hipSuccess || hipStreamWaitEvent(r.copy_stream[0], b.converted, 0) != hipSuccess ||
         hipStreamWaitEvent(r.copy_stream[1], b.converted, 0) != hipSuccess))
        return r.fail("event after the IQ conversion failed");
    if (c.monitor_fp && !mon.reqs.empty() && !enqueue_monitor(r, b, mon)) return false;
    if (c.spectrum_fp && !enqueue_spectrum(r, b, n)) return false;
    return enqueue_copies(r, b, n);
}

// The main thread's loop: rows from the ring -> synthesis -> chain -> copies into a free slot -> the writer.  Leaves through one path;
// the reason, if there is one, is in r.err.  Returns the slot the next batch would have filled: the older of the two.  (SIGINT: the batch in flight is finished and written, batches queued behind it are dropped)
int run_loop(Run &r, RowRing &ring, SlotPair &sp, int total, Clock::time_point t_start)
{
    const Config &c = r.c;
    const bool batch_timing = getenv("GAL_CLI_TIMING") != nullptr;
    const auto ms_since = [](Clock::time_point a) { return std::chrono::duration<double, std::milli>(Clock::now() - a).count(); };
    const auto synth = c.array_on() ? synth_array : c.refl_on() ? synth_refl : c.parts_on() ? synth_mpath : c.power_on ? synth_gains : synth_plain;
    const bool finished_inside = c.array_on() || c.refl_on() || c.parts_on() || c.power_on;  // run_gains / run_mpath return with every group finished
    int cur = 0;
    for (int ri = 0; r.emitted < total && !sp.io_error && !g_stop; cur ^= 1, ri = (ri + 1) % RowRing::kBufs) {
        const auto tb0 = Clock::now();
        RowRing::Buf &rows = ring.buf[ri];
        BatchSlot &b = sp.s[cur];
        {
            std::unique_lock<std::mutex> lk(ring.mu);
            ring.cv.wait(lk, [&] { return rows.ready; });
        }
        const double tb_rows = ms_since(tb0);
        const int n = rows.n;
        if (n < 0) r.fail("%s", ring.error.c_str());
        if (n <= 0) break;
        {  // wait until the slot we are about to fill has been written out
            std::unique_lock<std::mutex> lk(sp.mu);
            sp.cv.wait(lk, [&] { return !b.out.full; });
        }
        const double tb_slot = ms_since(tb0);
        MonRequests mon;
        if (c.monitor_fp) {
            if (b.mon.pending) {  // (cannot happen: flushed behind the finish of the batch after it)
                r.fail("monitor buffer still in use");
                break;
            }
            mon = monitor_requests(r, rows.rows.data(), n, b.mon);
        }
        if (synth(r, rows, n, b.d_iq) != GAL_OK) {
            if (r.err.empty()) r.lib_fail();  // (synth_refl has said why itself where the reason is its own)
            break;
        }
        {  // plan() has uploaded the rows: the producer may refill this buffer
            std::lock_guard<std::mutex> lk(ring.mu);
            rows.ready = false;
        }
        ring.cv.notify_all();
        // The IQ in d_iq is final only once gal_synth_finish() has returned: finish() may find the speculative
        // carrier chain unverified (or the replay check unhappy) and synthesise the batch again.  The copies are
        // therefore enqueued after it; they still run beside the front-end and the synthesis of the next batch.
        if (!finished_inside && gal_synth_finish(r.eng, r.state.data(), nullptr) != GAL_OK) {
            r.lib_fail();
            break;
        }
        // (the stream has drained up to this batch's synthesis: the sums and gains of the batch before it are on the host)
        BatchSlot &prev = sp.s[cur ^ 1];
        if (c.monitor_fp && prev.mon.pending) monitor_flush(prev.mon, c.monitor_fp, kOutRate, r.mon_shape, r.mon_sum);
        if (c.agc_log_fp && prev.agc_log.pending) r.agc_log_flush(prev.agc_log);
        if (c.spectrum_fp && prev.spec.pending) spectrum_flush(prev.spec, c.spectrum_fp, 1 << c.spectrum.log2_n, r.spec_total);
        const double tb_synth = ms_since(tb0);
        if (batch_timing)
            fprintf(stderr, "[timing] batch at %7.2f ms: %3d epochs, waited %.2f ms for rows, %.2f for a free slot, %s %.2f\n",
                    std::chrono::duration<double, std::milli>(tb0 - t_start).count(), n, tb_rows, tb_slot - tb_rows,
                    c.array_on() ? "run_array (every satellite's plan + execute + finish, the array pass enqueued)"
                    : c.refl_on() ? "run_refl (every group's plan + execute + finish, the reflector pass enqueued)"
                    : c.parts_on() ? "run_scint (every group's plan + execute + finish, scintillation and the echo pass enqueued)"
                    : c.power_on ? "run_gains (every group's plan + execute + finish, the sum enqueued)"
                                 : "plan + execute + finish",
                    tb_synth - tb_slot);
        if (!finish_batch(r, b, n, mon)) break;
        r.have_state = true;
        {
            std::lock_guard<std::mutex> lk(sp.mu);
            b.out.full = true;
        }
        sp.cv.notify_all();
        r.emitted += n;
        if (c.verbose || isatty(fileno(stderr)))
            fprintf(stderr, "\rTime into run = %4.1f - %4.1f", r.emitted / 10.0, std::chrono::duration<double>(Clock::now() - t_start).count());
    }
    if (!r.err.empty()) fprintf(stderr, "\nERROR: %s\n", r.err.c_str());
    return cur;
}

// --spectrum: the last batches' lines, the total (sums in 128-bit integers, printed in decimal), the summary on stderr; false: the
// file is not whole
bool spectrum_report(Run &r, SlotPair &sp, int older)
{
    const Config &c = r.c;
    const int N = 1 << c.spectrum.log2_n;
    SpecTotal &t = r.spec_total;
    bool ok = hipStreamSynchronize(r.stream) == hipSuccess;
    for (int i = 0; i < 2 && ok; ++i)  // (the older batch first)
        if (sp.s[older ^ i].spec.pending) spectrum_flush(sp.s[older ^ i].spec, c.spectrum_fp, N, t);
    fprintf(c.spectrum_fp, "total,%llu", (unsigned long long)t.n_seg);
    for (int k = 0; k < N; ++k) {
        fputc(',', c.spectrum_fp);
        print_u128(c.spectrum_fp, t.p[(k + N / 2) & (N - 1)]);
    }
    fputc('\n', c.spectrum_fp);
    if (fclose(c.spectrum_fp) != 0) {
        fprintf(stderr, "ERROR: writing the spectrum file %s failed\n", c.spectrum_file);
        ok = false;
    }
    for (BatchSlot &b : sp.s) {
        hipFree(b.spec.dev);
        hipHostFree(b.spec.host);
        if (b.spec.d_line) hipFree(b.spec.d_line);
    }
    fprintf(stderr, "Spectrum (%s): %d epochs, %llu segments of %d, %s window\n", c.spectrum_file, t.n_epochs, (unsigned long long)t.n_seg, N,
            c.spectrum.window ? "Hann" : "rectangular");
    if (!t.n_seg) return ok;
    // in frequency order: the peak, the median, and the band that holds 99 % of the power (0.5 % cut off at either end)
    std::vector<long double> f((size_t)N);
    long double sum = 0.0L;
    int peak = 0;
    for (int k = 0; k < N; ++k) {
        f[k] = (long double)t.p[(k + N / 2) & (N - 1)];
        sum += f[k];
        if (f[k] > f[peak]) peak = k;
    }
    std::vector<long double> sorted(f);
    std::sort(sorted.begin(), sorted.end());
    const long double median = 0.5L * (sorted[N / 2 - 1] + sorted[N / 2]);
    int lo = 0, hi = N - 1;
    long double cut = 0.0L;
    while (lo < hi && cut + f[lo] <= 0.005L * sum) cut += f[lo++];
    cut = 0.0L;
    while (hi > lo && cut + f[hi] <= 0.005L * sum) cut += f[hi--];
    const double bin_hz = kOutRate / N;
    fprintf(stderr, "  peak at %+.1f Hz (bin %+d), %.2f dB over the median bin; 99 %% of the power within %.1f Hz (%+.1f .. %+.1f Hz)\n", (peak - N / 2) * bin_hz,
            peak - N / 2, median > 0.0L ? 10.0 * log10((double)(f[peak] / median)) : INFINITY, (hi - lo + 1) * bin_hz, (lo - N / 2 - 0.5) * bin_hz,
            (hi - N / 2 + 0.5) * bin_hz);
    return ok;
}

// behind "Done!": the side files' last lines and summaries, the notes, the saturation report.  Returns the exit code so far
int report(Run &r, SlotPair &sp, gal_scen_t *scen, int older)
{
    const Config &c = r.c;
    int rc = r.err.empty() ? 0 : 1;
    if (c.monitor_fp) {
        if (hipStreamSynchronize(r.stream) != hipSuccess) rc = 1;
        for (int i = 0; i < 2 && rc == 0; ++i)
            if (sp.s[i].mon.pending) monitor_flush(sp.s[i].mon, c.monitor_fp, kOutRate, r.mon_shape, r.mon_sum);
        if (fclose(c.monitor_fp) != 0) {
            fprintf(stderr, "ERROR: writing the monitor file %s failed\n", c.monitor_file);
            rc = 1;
        }
        fprintf(stderr, "Monitor (%s, every %d epochs, %d code periods each): C/N0 of the composite E1B + E1C signal\n", c.monitor_file, c.monitor_every,
                kMonPeriods);
        for (int prn = 1; prn <= GAL_NUM_PRN; ++prn) {
            const MonSummary &s = r.mon_sum[prn];
            if (!s.n) continue;
            if (s.n > s.no_peak)
                fprintf(stderr, "  PRN %2d: %4d epochs, C/N0 mean %.2f dB-Hz (min %.2f, max %.2f), peak off the plan in %d, no peak in %d\n", prn, s.n,
                        s.sum / (s.n - s.no_peak), s.lo, s.hi, s.off_peak, s.no_peak);
            else fprintf(stderr, "  PRN %2d: %4d epochs, no peak in any\n", prn, s.n);
        }
        for (BatchSlot &b : sp.s) {
            hipFree(b.mon.dev);
            hipHostFree(b.mon.host);
        }
    }
    if (c.agc_log_fp) {
        if (hipStreamSynchronize(r.stream) != hipSuccess) rc = 1;
        for (int i = 0; i < 2 && rc == 0; ++i)  // (the older batch first)
            if (sp.s[older ^ i].agc_log.pending) r.agc_log_flush(sp.s[older ^ i].agc_log);
        if (fclose(c.agc_log_fp) != 0) {
            fprintf(stderr, "ERROR: writing the AGC log %s failed\n", c.agc_log_file);
            rc = 1;
        }
        fprintf(stderr, "AGC log (%s): %llu blocks of %ld samples\n", c.agc_log_file, (unsigned long long)r.agc_logged, c.agc_block);
        for (BatchSlot &b : sp.s) {
            hipFree(b.agc_log.dev);
            hipHostFree(b.agc_log.host);
        }
    }
    if (c.spectrum_fp) rc = spectrum_report(r, sp, older) ? rc : 1;
    if (gal_scen_eph_gaps(scen) > 0)
        fprintf(stderr, "NOTE: %d (satellite, refresh) pairs ran on a stale ephemeris record (see the warning above)\n", gal_scen_eph_gaps(scen));
    if (c.power_on) {
        fprintf(stderr, "Signal power per PRN (Q7 gain, 128 = unity; dB against unity):\n");
        for (int prn = 1; prn <= GAL_NUM_PRN; ++prn)
            if (r.prn_gain_hi[prn] >= 0)
                fprintf(stderr, "  PRN %2d: gain %5d .. %5d  (%+.2f .. %+.2f dB)\n", prn, r.prn_gain_lo[prn], r.prn_gain_hi[prn],
                        r.prn_gain_lo[prn] > 0 ? 20.0 * log10(r.prn_gain_lo[prn] / 128.0) : -INFINITY,
                        r.prn_gain_hi[prn] > 0 ? 20.0 * log10(r.prn_gain_hi[prn] / 128.0) : -INFINITY);
    }
    if (c.reports_saturation()) {  // (stderr: with -o - the data go to stdout)
        uint64_t n_sat = 0;
        const double n_val = (double)r.emitted * r.cfg.samples_per_epoch * 2;
        if (gal_synth_iq_saturated(r.eng, &n_sat, 0) != GAL_OK) {
            fprintf(stderr, "ERROR: %s\n", gal_synth_last_error());
            rc = 1;
        } else if (n_sat > 0 && c.iq_format != GAL_IQ_IBYTE) {
            fprintf(stderr, "WARNING: %llu of %.0f IQ values (%.3g %%) saturated at int16; a smaller --signal-gain avoids the clipping\n",
                    (unsigned long long)n_sat, n_val, n_val > 0 ? 100.0 * (double)n_sat / n_val : 0.0);
        } else if (n_sat > 0) {
            fprintf(stderr, "WARNING: %llu of %.0f IQ values (%.3g %%) saturated at --iq-shift %d; a larger --iq-shift avoids the clipping\n",
                    (unsigned long long)n_sat, n_val, n_val > 0 ? 100.0 * (double)n_sat / n_val : 0.0, c.iq_shift);
        } else if (c.verbose && c.iq_format == GAL_IQ_IBYTE) {
            fprintf(stderr, "IQ values saturated at --iq-shift %d: 0 of %.0f\n", c.iq_shift, n_val);
        }
    }
    return rc;
}

// GAL_CLI_TIMING=1: where the start-up goes (stage times on stderr)
void stage(const char *what)
{
    static const bool on = getenv("GAL_CLI_TIMING") != nullptr;
    static auto t0 = Clock::now();
    static auto tl = t0;
    if (!on) return;
    const auto t = Clock::now();
    fprintf(stderr, "[timing] %-28s +%7.1f ms  (%7.1f ms since start)\n", what, std::chrono::duration<double, std::milli>(t - tl).count(),
            std::chrono::duration<double, std::milli>(t - t0).count());
    tl = t;
}

// the front-end; an empty scenario ends the command here as it ends the reference
gal_scen_t *open_scenario(Config &c)
{
    gal_scen_t *scen = nullptr;
    int orc = gal_scen_open(&c.sc, &scen);
    if (orc == GAL_E_BUSY && c.sc.udp_port > 0 && !c.udp_given) {
        // the default port is taken (another instance): the reference would exit; carry on without the listener
        fprintf(stderr, "WARNING: %s; continuing without run-time position updates\n", gal_scen_last_error());
        c.sc.udp_port = 0;
        orc = gal_scen_open(&c.sc, &scen);
    }
    if (orc != GAL_OK) {
        fprintf(stderr, "%s\n", gal_scen_last_error());
        if (orc == GAL_E_EMPTY && c.outfile != "-" && !c.array_on()) {
            // (int)(10 d + 0.5) < 2: the reference opens its sink, finds no epoch to generate and closes it (src/galileo-sdr.cpp:438)
            FILE *f = fopen(c.outfile.c_str(), "wb");
            if (f) fclose(f);
            exit(0);
        }
        exit(1);
    }
    if (c.power_on && (gal_scen_set_power(scen, c.have_antenna ? c.ant_db : nullptr, c.prn_db) != GAL_OK ||
                       gal_scen_set_path_loss(scen, c.power_model ? 1 : 0) != GAL_OK))
        die("ERROR: %s\n", gal_scen_last_error());
    return scen;
}

// the engine with the chain's stages set, its stream and the two copy streams
void open_engine(Run &r)
{
    const Config &c = r.c;
    // (Engine creation and buffer allocation one after the other: running them in two threads was measured -- 6 alternations
    // on one box, 157-318 ms against 250-328 ms for this stage, no difference beyond the run-to-run spread of the HIP
    // start-up itself; the runtime serialises code-object loading and page pinning.)
    if (gal_synth_create(&r.cfg, &r.eng) != GAL_OK) die("ERROR: %s\n", gal_synth_last_error());
    stage("gal_synth_create");
    if (c.fir_on() && (c.dec_on() ? gal_synth_firdec_set(r.eng, c.fir_taps, c.n_fir, c.osr, 0) : gal_synth_fir_set(r.eng, c.fir_taps, c.n_fir)) != GAL_OK)
        die("ERROR: %s\n", gal_synth_last_error());
    if (c.agc_on && gal_synth_agc_set(r.eng, &c.agc, 0) != GAL_OK) die("ERROR: %s\n", gal_synth_last_error());
    if (c.osc_on && gal_synth_osc_set(r.eng, &c.osc, 0) != GAL_OK) die("ERROR: %s\n", gal_synth_last_error());
}

// the streams, and the first use of the copy path
void open_streams(Run &r, SlotPair &sp)
{
    // (a stream for the engine, made here: left to the engine it would be made inside the first gal_synth_plan -- 7-17 ms
    // of the run instead of the start-up)
    hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking);
    gal_synth_set_stream(r.eng, r.stream);
    // device -> host on two streams of their own: two DMA engines share the link, and the copy of batch k runs
    // beside the front-end and the synthesis of batch k+1
    hipStreamCreateWithFlags(&r.copy_stream[0], hipStreamNonBlocking);
    hipStreamCreateWithFlags(&r.copy_stream[1], hipStreamNonBlocking);
    // First use of the copy path belongs to the start-up, not to the run: the first device -> host copy of a process
    // took 8 ms on its own (profiles/archive/r03p_cli_batches.log: batch 2 started 10.4 ms into a run whose batches take 2.35 ms)
    if (getenv("GAL_CLI_COLD_COPY")) return;
    for (BatchSlot &b : sp.s)
        for (int k = 0; k < 2; ++k) {
            const size_t off = k ? r.batch_bytes / 2 : 0, nb = r.batch_bytes / 2 < ((size_t)1 << 20) ? r.batch_bytes / 2 : ((size_t)1 << 20);
            if (nb) hipMemcpyAsync((char *)b.out.host + off, (const char *)b.d_out + off, nb, hipMemcpyDeviceToHost, r.copy_stream[k]);
        }
    hipStreamSynchronize(r.copy_stream[0]);
    hipStreamSynchronize(r.copy_stream[1]);
}

// the scenario through the engine into the sink; the exit code
int run(Config &c, gal_scen_t *scen)
{
    const int total = gal_scen_total_epochs(scen);
    int32_t wk;
    double ws;
    gal_scen_start_time(scen, &wk, &ws);
    fprintf(stderr, "\n%s\nStart = %d:%.0f  Duration = %.1f [sec]  (%d epochs of 0.1 s)\n",
            c.sc.motion_file ? "Using user motion file." : "Using static location mode.", wk, ws, (total + 1) / 10.0, total);
    Run r(c);
    memset(&r.cfg, 0, sizeof(r.cfg));
    r.cfg.sample_rate = c.sample_rate();
    r.cfg.samples_per_epoch = c.osr * kOutSamplesPerEpoch;
    r.cfg.n_slots = c.sc.n_slots;
    r.cfg.device = getenv("GAL_DEVICE") ? atoi(getenv("GAL_DEVICE")) : -1;
    if (c.cboc) r.cfg.flags |= GAL_CFG_CBOC;
    if (c.exact_replay) r.cfg.flags |= GAL_CFG_EXACT_REPLAY;
    // bytes per epoch in the output format: the per-batch split of the copies cuts at epoch boundaries, so every piece must be whole
    // bytes -- for ibit 260 000 % 4 == 0 (i2bit: 260 000 % 2 == 0)
    r.epoch_bytes = c.out_bytes((size_t)kOutSamplesPerEpoch);
    if (c.iq_format == GAL_IQ_IBIT && kOutSamplesPerEpoch % 4 != 0) die("ERROR: ibit needs a multiple of 4 samples per epoch.\n");
    // Default: the sequential sink.  Measured on the MI355X host (256 cores, tmpfs, 1.25 GB): write() stream 0.20 s;
    // mapped sink with 4 / 8 / 16 copy threads 0.24 / 0.22 / 0.24 s INCLUDING the unmap (0.10-0.21 s without it, which is
    // what round 3's first measurements showed): the kernel inserts pages into ONE file's page cache at ~6 GB/s whoever
    // asks -- write(), page faults of many threads, pwrite()s of many threads (inode lock) -- profiles/archive/r03a_sink_probe.log.
    if (c.n_writers < 0) c.n_writers = 0;
    r.K = c.n_elem();
    if (c.array_log_file && !(c.array_log_fp = fopen(c.array_log_file, "w"))) die("ERROR: --array-log %s cannot be written.\n", c.array_log_file);
    if (c.refl_log_file && !(c.refl_log_fp = fopen(c.refl_log_file, "w"))) die("ERROR: --reflector-log %s cannot be written.\n", c.refl_log_file);
    std::vector<Sink> sinks(r.K);
    for (int k = 0; k < r.K; ++k) {
        std::string path = c.outfile;
        if (c.array_on()) {  // NAME.EXT -> NAME.a<k>.EXT (no extension: NAME.a<k>), always with the suffix
            const size_t slash = path.find_last_of('/'), dot = path.find_last_of('.');
            const std::string tag = ".a" + std::to_string(k);
            if (dot == std::string::npos || (slash != std::string::npos && dot < slash) || dot == (slash == std::string::npos ? 0 : slash + 1)) path += tag;
            else path.insert(dot, tag);
            fprintf(stderr, "Element %d -> %s\n", k, path.c_str());
        }
        if (!sinks[k].open(path.c_str(), c.realtime ? 0 : (size_t)total * r.epoch_bytes, c.n_writers))  // (paced runs stream: they are slow by design)
            die("ERROR: Failed to open output file.\n");
    }
    stage("sink opened");
    open_engine(r);
    if (c.batch_epochs > total) c.batch_epochs = total > 0 ? total : 1;
    r.batch_bytes = r.epoch_bytes * c.batch_epochs;
    r.iq_stride = (size_t)r.cfg.samples_per_epoch * 4 * c.batch_epochs;  // (a multiple of 16: 260 000 samples of 4 bytes)
    r.out_stride = (r.batch_bytes + 15) / 16 * 16;                       // the library's buffers begin on 16 bytes
    memset(&r.mon_shape, 0, sizeof(r.mon_shape));
    r.mon_shape.max_periods = kMonPeriods;
    r.mon_shape.delay_step = 1;
    r.mon_shape.dopp_step = (int32_t)llround(kMonBinHz / kOutRate * 4294967296.0);
    r.mon_shape.dopp0 = -r.mon_shape.dopp_step;
    r.mon_shape.n_dopp = 3;
    // gal_corr_cn0 reads the period length off the shape: the nominal code step (a request's own differs by its code Doppler, a few
    // 1e-6: 1e-5 dB).  Left at 0 it made every C/N0 of the CSV "nan"
    r.mon_shape.code_dph = (uint64_t)llround(2.0 * 1.023e6 / kOutRate * 4294967296.0);
    if (c.spectrum_fp) r.spec_total.p.assign((size_t)1 << c.spectrum.log2_n, 0);
    SlotPair sp;
    if (!alloc_slots(r, sp)) die("ERROR: buffer allocation failed\n");
    stage("device + pinned buffers");
    open_streams(r, sp);
    stage("copy path warmed");

    std::thread writer(write_slots, std::ref(sp), std::ref(sinks));
    signal(SIGINT, on_sigint);
    const auto t_start = Clock::now();
    RowRing ring;
    for (auto &b : ring.buf) {
        const size_t epochs = (size_t)c.batch_epochs + (c.refl_on() ? 1 : 0);  // (--reflector: one epoch of look-ahead)
        b.rows.resize(epochs * c.sc.n_slots);
        if (c.power_on) b.gains.resize(epochs * c.sc.n_slots);
        if (c.azel_on()) b.azel.resize(epochs * c.sc.n_slots * 2);
    }
    std::thread producer(produce_rows, std::ref(ring), scen, std::cref(c), t_start);
    r.state.resize(c.sc.n_slots);
    memset(r.state.data(), 0, sizeof(gal_chan_state_t) * c.sc.n_slots);
    for (int i = 0; i <= GAL_NUM_PRN; ++i) r.prn_gain_lo[i] = GAL_GAIN_MAX + 1, r.prn_gain_hi[i] = -1;
    const int older = run_loop(r, ring, sp, total, t_start);
    // the way out, after the last batch or a failure alike: the producer is told to stop, the slots are drained, the writer is joined
    {
        std::lock_guard<std::mutex> lk(ring.mu);
        ring.consumer_gone = true;
    }
    ring.cv.notify_all();
    producer.join();
    {
        std::unique_lock<std::mutex> lk(sp.mu);
        sp.cv.wait(lk, [&] { return !sp.s[0].out.full && !sp.s[1].out.full; });
        sp.done = true;
    }
    sp.cv.notify_all();
    writer.join();
    // (the sink is closed inside the reported time: unmapping a 1.2 GB file mapping is not free, and the file is only
    // the caller's once it is closed)
    for (Sink &s : sinks)
        if (!s.finish()) sp.io_error = true;
    if (c.array_log_fp && fclose(c.array_log_fp) != 0) {
        fprintf(stderr, "ERROR: writing the array log %s failed\n", c.array_log_file);
        sp.io_error = true;
    }
    if (c.refl_log_fp && fclose(c.refl_log_fp) != 0) {
        fprintf(stderr, "ERROR: writing the reflector log %s failed\n", c.refl_log_file);
        sp.io_error = true;
    }
    stage("run (= Process time)");
    const double el = std::chrono::duration<double>(Clock::now() - t_start).count();
    fprintf(stderr, "\nDone!\nProcess time = %.2f [sec]  (%.1f Msamples/s, %.0fx real time)\n", el, r.emitted * 0.26 / el, r.emitted * 0.1 / el);
    int rc = report(r, sp, scen, older);
    gal_synth_destroy(r.eng);
    gal_scen_close(scen);
    stage("teardown");
    if (sp.io_error) {
        fprintf(stderr, "ERROR: short write on the output sink\n");
        rc = 1;
    }
    return rc;
}

}  // namespace

int main(int argc, char *argv[])
{
    stage("process start");
    if (argc < 3) {
        usage(argv[0]);
        exit(1);
    }
    Config c;
    parse_options(argc, argv, &c);
    if (!c.sitesfile.empty()) {
        char self[4096];
        const ssize_t n = readlink("/proc/self/exe", self, sizeof(self) - 1);
        if (n <= 0) snprintf(self, sizeof(self), "%s", argv[0]);
        else self[n] = 0;
        return run_sites(self, c);
    }
    if (c.outfile.empty()) {
        printf("[+] File sink not specified. Using galileosim.%s\n", kIqNames[c.iq_format]);
        c.outfile = std::string("galileosim.") + kIqNames[c.iq_format];
    }
    if (c.dec_on() && !c.have_batch) c.batch_epochs = 128 / c.osr > 8 ? 128 / c.osr : 8;  // the device buffers keep their size
    if (c.realtime && !c.have_batch) c.batch_epochs = 1;  // paced output: position updates take effect within 0.1 s
    if (c.batch_epochs < 1) c.batch_epochs = 1;
    c.sc.nav_file = c.navfile.c_str();
    c.sc.motion_file = c.umfile.empty() ? nullptr : c.umfile.c_str();
    c.sc.verbose = 1;
    gal_scen_t *scen = open_scenario(c);
    stage("scenario opened (RINEX)");
    return run(c, scen);
}
