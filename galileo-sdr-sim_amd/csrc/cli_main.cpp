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
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <getopt.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <cmath>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/galscen.h"
#include "../../include/galsynth.h"

namespace {

std::atomic<bool> g_stop{false};
void on_sigint(int) { g_stop = true; }

void usage(const char *prog)
{
    printf("Usage: %s [options]\n"
           "Options:\n"
           "  -e <Ephemeris>   RINEX navigation file for Galileo ephemerides (required)\n"
           "  -o <File sink>   File to store IQ samples (default galileosim.<format>, - = stdout)\n"
           "  -l <location>    Lat,Lon,Hgt (static mode) e.g. 35.274,137.014,100\n"
           "  -u <user_motion> ECEF user motion file t,x,y,z at 10 Hz (dynamic mode)\n"
           "  -t <date,time>   Scenario start time YYYY/MM/DD,hh:mm:ss\n"
           "  -d <duration>    Duration [sec]\n"
           "  -I <x>           Disable ionospheric delay\n"
           "  -T <date,time>   As the reference runs it: -t without its range check, UTC reference time overwritten (use `now` for\n"
           "                   the current time).  The same bytes as the reference program for the same command line: its loop that\n"
           "                   would shift TOC / TOE never runs, so a start outside the file's span gives an empty sky (warned about)\n"
           "  --shift-toe      with -T: what the option sets out to do -- TOC and TOE of every record shifted to the start time, the\n"
           "                   navigation file becomes valid at any start (include/galscen.h: time_overwrite 2; not the reference's bytes)\n"
           "  --ref-T          with -T: the explicit spelling of the default (kept for round 5's command lines)\n"
           "  -P <port>        UDP port for run-time position updates lat,lon,hgt as 3 doubles (0 = off; default: 7533 on\n"
           "                   the loopback interface; a port given here is bound on all interfaces, as the reference's)\n"
           "  -r               Pace the output to real time (one 0.1 s epoch per 0.1 s)\n"
           "  -C               CBOC(6,1,1/11) sub-carrier of the E1 OS ICD instead of the reference's BOC(1,1) (opt-in)\n"
           "  --exact-replay   Synthesise with the exact-replay kernel only (every sample of both NCO recurrences stepped; the same bytes, slower)\n"
           "  --strict         Stop with an error where a satellite in view runs out of ephemeris (default: its channel\n"
           "                   keeps the last valid record; the reference indexes out of bounds there)\n"
           "  --sites <file>   One line lat,lon,hgt[,outfile] per receiver site: one process per site over the GPUs of the\n"
           "                   node (--gpus N, default all; --per-gpu K processes per GPU, default 1); -o is the name stem;\n"
           "                   -P <port>: site k listens on port + k (default: no position listener)\n"
           "  --iq-format <f>  Output format: ishort (interleaved int16, the default), ibyte (interleaved int8: rounded\n"
           "                   x >> shift, clamped to +-127), ibit (1 bit per value, x > 0, packed MSB first)\n"
           "                   i2bit (2 bits per value: sign and magnitude against --i2bit-threshold, 4 values per byte, MSB first;\n"
           "                   implies --agc; default output name galileosim.i2bit)\n"
           "  --iq-shift <n>   ibyte only: right shift 0..15 before the clamp (default 5)\n"
           "  --agc [rms]      Block AGC in front of the quantiser, behind gains, noise, interference and --fir / the decimator: the power of\n"
           "                   the last --agc-window blocks sets the gain of the next block, so that the rms per rail becomes `rms` int16\n"
           "                   LSB (default: 32 x 2^shift for ibyte, 2048 for ishort, the threshold for i2bit); not with ibit.  With --agc the\n"
           "                   automatic --iq-shift of --cn0 / --jam leaves the --jam amplitudes out -- the AGC makes that room --: it is the\n"
           "                   smallest shift with 127 x 2^shift >= 4 sigma (--cn0), or >= the largest signal sum (--jam alone)\n"
           "  --agc-block <n>  with --agc: complex samples per block, 16..65536 (default 2600 = 1 ms)\n"
           "  --agc-window <n> with --agc: blocks averaged, 1..64, block x window <= 65536 (default 8)\n"
           "  --agc-init-rms <r> with --agc: the rms assumed in front of the stream (default: the noise sigma of --cn0, behind --fir or\n"
           "                   the decimator sigma x sqrt(sum h^2) / 16384; without --cn0 750)\n"
           "  --agc-log <file> with --agc: CSV, one line per block: time of its first sample, gain (4096 = 1.0), gain in dB\n"
           "  --i2bit-threshold <n> i2bit only: the magnitude threshold, 1..32767 (default 1024)\n"
           "  --cn0 <dBHz>     Add a white Gaussian noise floor: C/N0 of one satellite's composite E1B + E1C signal (E1B alone is\n"
           "                   3 dB lower); every format; the same bytes for the same options on any machine (default: no noise)\n"
           "  --noise-seed <n> with --cn0: seed of the noise, 0 .. 2^64 - 1 (default 1)\n"
           "  --noise-stream <n> with --cn0: independent noise under the same seed, 0 .. 2^32 - 1 (default 0; --sites: the site's index)\n"
           "  --signal-gain <g> with --cn0 or --jam: gain on the signals, 0 < g <= 16 (default: the largest power of two <= 1 that keeps\n"
           "                   5 sigma of noise + the largest signal sum + the --jam amplitudes inside int16)\n"
           "  --jam <spec>     Add an interference source, up to 4 times: js_db,f_hz[,f_hi_hz,sweep_us[,period_us,on_us]] -- J/S in dB against\n"
           "                   one satellite's composite signal, a CW tone at f_hz from the centre, or a chirp from f_hz to f_hi_hz that\n"
           "                   restarts every sweep_us microseconds, on for on_us of every period_us (f_hi_hz = sweep_us = 0: a pulsed\n"
           "                   CW tone); with or without --cn0\n"
           "  --power-model    Per-satellite signal power from the path loss: gain = 23 222 km / distance (a satellite at the zenith is\n"
           "                   about unity); --cn0 and --jam then hold for a satellite at unity gain\n"
           "  --antenna <file> Receiver antenna pattern: 37 attenuations in dB, one per 5 degrees off the zenith (default: isotropic)\n"
           "  --prn-power <l>  Per-PRN power offsets prn:dB[,prn:dB...], e.g. 5:-6,12:3 (PRN 1..50, -60..60 dB)\n"
           "  --fir <file>     Front-end FIR filter over the stream, behind noise / interference and in front of the format: integer\n"
           "                   taps in Q14 (16384 = 1.0), one per line, 1..128 of them, sum of |tap| <= 65535\n"
           "  --fir-lowpass <cutoff_hz>[,n_taps] the same with a Hamming-windowed sinc low-pass (n_taps odd, 3..127, default 63; the taps\n"
           "                   are printed on stderr); not together with --fir\n"
           "  --multipath <f>  Echoes of single satellites, one per line of the file: prn,delay_m,rel_db,phase_deg[,fade_hz] (# comments) --\n"
           "                   the satellite's own stream again, delay_m / c later (rounded to whole samples: 115 m at 2.6 MS/s, 7.7 m with\n"
           "                   --oversample 15; at most 1024 samples), rel_db against the direct signal (at most +6 dB), turned by phase_deg and\n"
           "                   rotating at fade_hz.  At most 32 lines, 4 per PRN; a PRN that is not in view has no effect.  Added on the GPU in\n"
           "                   front of noise, --jam, the filters and the AGC; --monitor then shows the multipath.\n"
           "  --oversample <M> Synthesise, weight, add noise and interference at M x 2.6 MS/s (M = 2..15) and bring the stream back to\n"
           "                   2.6 MS/s with one decimating FIR filter in front of the format: the file has the size and rate it has\n"
           "                   without the option.  --jam frequencies are then admitted up to +-M x 1.3 MHz.  --fir <file> then holds the\n"
           "                   decimator's taps at the high rate (1..512), --fir-lowpass designs them at the high rate (n_taps odd, 3..511);\n"
           "                   with neither: a low-pass at 1.17 MHz with 32 M + 1 taps (printed on stderr).  The automatic --iq-shift\n"
           "                   uses the sigma behind the filter, sigma x sqrt(sum h^2) / 16384.  --monitor needs taps whose\n"
           "                   (n_taps - 1) is a multiple of 2 M (a delay of whole output samples).  Default -B: max(8, 128 / M)\n"
           "  --lo-offset <hz>[,<drift_hz_per_s>] Receiver oscillator: rotate the whole stream -- satellites, echoes, --jam sources and noise --\n"
           "                   by a carrier offset and a linear drift, behind --cn0 / --jam and in front of --fir / the decimator, --agc and\n"
           "                   the format (with --oversample at the high rate).  --monitor follows the offset and the drift.  The sample\n"
           "                   clock stays ideal: the code rate is not scaled by the same ppm (a few 1e-6 of it at a TCXO's offset).\n"
           "  --phase-noise <h0> the same oscillator with white-FM phase noise of the one-sided fractional-frequency PSD h0 in seconds\n"
           "                   (1e-21: a good TCXO); the per-sample sigma, the rms phase over 1 and 4 ms and the linewidth are printed\n"
           "  --osc-seed <N>   with --phase-noise: the seed of the phase noise (unsigned 64-bit, default 1)\n"
           "  --osc-stream <N> with --phase-noise: its stream (unsigned 32-bit, default 0; --sites gives site i the stream i)\n"
           "  --monitor <file> Despread the output with the planned replicas and write one CSV line per monitored epoch and PRN:\n"
           "                   time, PRN, planned Doppler, measured C/N0 (composite E1B + E1C), peak ratio, strongest of the delays\n"
           "                   -1 / 0 / +1 half chip and of the Doppler offsets -1 / 0 / +1 bin of 250 Hz; a summary per PRN on stderr\n"
           "  --monitor-every <n> with --monitor: every n-th epoch of 0.1 s (default 10)\n"
           "  --writers <n>    Threads that move finished batches into a regular output file (default 0: sequential write(); > 0: mapped file, n copy threads)\n"
           "  -v               Verbose\n"
           "  -U/-b/-a/-G/-p/-n/-g/-i     accepted for compatibility (file sink only)\n",
           prog);
}

struct Slot {  // one pinned host buffer of the double-buffered sink
    int16_t *host = nullptr;
    size_t bytes = 0;
    hipEvent_t copied[2] = {nullptr, nullptr};  // the batch leaves the GPU in two halves on two copy streams
    bool full = false;
};

// ---- the output ------------------------------------------------------------------------------------------------
// Regular file: ftruncate to the final size + one shared mapping; put() has `n_workers` threads copy disjoint pieces.
// Anything else (stdout, pipe, device): sequential write().
class Sink {
public:
    ~Sink()
    {
        close_workers();
        if (prealloc_.joinable()) {
            stop_prealloc_ = true;
            prealloc_.join();
        }
    }

    bool open(const char *path, size_t total_bytes, int n_workers)
    {
        total_ = total_bytes;
        if (strcmp(path, "-") == 0) {
            fd_ = STDOUT_FILENO;
            own_fd_ = false;
        } else {
            fd_ = ::open(path, O_RDWR | O_CREAT | O_TRUNC, 0644);
            if (fd_ < 0) fd_ = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);  // write-only sinks (devices, FIFOs)
            if (fd_ < 0) return false;
            own_fd_ = true;
        }
        struct stat sb;
        const char *force = getenv("GAL_SINK");  // "stream": never map (A/B measurements)
        if (own_fd_ && fstat(fd_, &sb) == 0 && S_ISREG(sb.st_mode) && total_ > 0 && n_workers > 0 &&
            !(force && strcmp(force, "stream") == 0) && ftruncate(fd_, (off_t)total_) == 0) {
            void *m = mmap(nullptr, total_, PROT_READ | PROT_WRITE, MAP_SHARED, fd_, 0);
            if (m != MAP_FAILED) {
                map_ = (char *)m;
                for (int i = 0; i < n_workers; ++i) workers_.emplace_back([this, i] { worker(i); });
            } else if (ftruncate(fd_, 0) != 0) {
                return false;
            }
        }
        // Sequential sink into a regular file of known size: a helper thread allocates the file's pages ahead of the writes
        // (fallocate, size kept: the file grows as it is written), 64 MB at a time, WHILE the device starts up -- the run's
        // write()s then copy into pages that exist (tmpfs on the MI355X host: 1.19 GB allocate 70 ms, write() into allocated
        // pages 130 ms, write() that allocates as it goes 190 ms; profiles/archive/r03j_sink_probe.log).  Failure is not an error:
        // the writes allocate for themselves then.  GAL_SINK=noprealloc turns it off.
        if (!map_ && own_fd_ && fstat(fd_, &sb) == 0 && S_ISREG(sb.st_mode) && total_ > 0 &&
            !(force && (strcmp(force, "noprealloc") == 0))) {
            prealloc_ = std::thread([this] {
                const size_t step = (size_t)64 << 20;
                for (size_t o = 0; o < total_ && !stop_prealloc_.load(std::memory_order_relaxed); o += step) {
                    const size_t n = total_ - o < step ? total_ - o : step;
                    if (fallocate(fd_, FALLOC_FL_KEEP_SIZE, (off_t)o, (off_t)n) != 0) break;
                }
            });
        }
        return true;
    }
    bool mapped() const { return map_ != nullptr; }
    int workers() const { return (int)workers_.size(); }

    // appends `bytes` from `src`; returns false on an I/O error
    bool put(const char *src, size_t bytes)
    {
        if (map_) {
            if (pos_ + bytes > total_) return false;
            {
                std::lock_guard<std::mutex> lk(mu_);
                job_src_ = src;
                job_dst_ = map_ + pos_;
                job_bytes_ = bytes;
                job_next_ = 0;
                job_left_ = (int)workers_.size();
                ++job_id_;
            }
            cv_.notify_all();
            std::unique_lock<std::mutex> lk(mu_);
            done_cv_.wait(lk, [&] { return job_left_ == 0; });
            pos_ += bytes;
            return true;
        }
        while (bytes) {
            const ssize_t n = ::write(fd_, src, bytes < ((size_t)1 << 30) ? bytes : ((size_t)1 << 30));
            if (n < 0) {
                if (errno == EINTR) continue;
                return false;
            }
            src += n;
            bytes -= (size_t)n;
            pos_ += (size_t)n;
        }
        return true;
    }

    // all data are in the file (mapped sink: in its page cache); a run that stopped early is cut to what was written
    bool finish()
    {
        close_workers();
        bool ok = true;
        if (prealloc_.joinable()) {
            stop_prealloc_ = true;
            prealloc_.join();
            // a run that stopped early (SIGINT, error): give back the pages allocated beyond what was written
            if (pos_ < total_ && ftruncate(fd_, (off_t)pos_) != 0) ok = false;
        }
        if (map_) {
            munmap(map_, total_);
            map_ = nullptr;
            if (pos_ < total_ && ftruncate(fd_, (off_t)pos_) != 0) ok = false;
        }
        if (own_fd_ && fd_ >= 0 && ::close(fd_) != 0) ok = false;
        fd_ = -1;
        return ok;
    }

private:
    static constexpr size_t kPiece = (size_t)2 << 20;  // 2 MiB: whole huge pages where the file system has them

    void worker(int)
    {
        unsigned long seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return quit_ || job_id_ != seen; });
            if (quit_) return;
            seen = job_id_;
            for (;;) {
                const size_t o = job_next_;
                if (o >= job_bytes_) break;
                const size_t n = job_bytes_ - o < kPiece ? job_bytes_ - o : kPiece;
                job_next_ = o + n;
                lk.unlock();
                memcpy(job_dst_ + o, job_src_ + o, n);
                lk.lock();
            }
            if (--job_left_ == 0) done_cv_.notify_all();
        }
    }
    void close_workers()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            quit_ = true;
        }
        cv_.notify_all();
        for (auto &t : workers_) t.join();
        workers_.clear();
    }

    int fd_ = -1;
    bool own_fd_ = false;
    std::thread prealloc_;
    std::atomic<bool> stop_prealloc_{false};
    char *map_ = nullptr;
    size_t total_ = 0, pos_ = 0;
    std::vector<std::thread> workers_;
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    bool quit_ = false;
    unsigned long job_id_ = 0;
    const char *job_src_ = nullptr;
    char *job_dst_ = nullptr;
    size_t job_bytes_ = 0, job_next_ = 0;
    int job_left_ = 0;
};

// ---- --jam js_db,f_hz[,f_hi_hz,sweep_us[,period_us,on_us]] ---------------------------------------------------------------------
struct JamSpec {
    double js_db, f_lo, f_hi, sweep_s, period_s, on_s;
};

// two, four or six numbers with commas between them and nothing else
bool parse_jam(const char *arg, JamSpec *j)
{
    double v[6] = {0, 0, 0, 0, 0, 0};
    int n = 0;
    const char *p = arg;
    for (;;) {
        char *end = nullptr;
        if (n == 6 || !*p || *p == ',') return false;
        v[n++] = strtod(p, &end);
        if (end == p) return false;
        if (!*end) break;
        if (*end != ',') return false;
        p = end + 1;
    }
    if (n != 2 && n != 4 && n != 6) return false;
    if (n == 6 && v[2] == 0.0 && v[3] == 0.0) {
        // a pulsed CW tone: no chirp
    } else if (n >= 4 && !(v[3] > 0.0)) {
        return false;  // a chirp needs a sweep time
    }
    j->js_db = v[0];
    j->f_lo = v[1];
    j->f_hi = v[2];
    j->sweep_s = v[3] * 1e-6;
    j->period_s = v[4] * 1e-6;
    j->on_s = v[5] * 1e-6;
    return true;
}

// ---- --prn-power prn:dB[,prn:dB...] and --antenna <file> ----------------------------------------------------------------------------
constexpr double kPowerDbMax = 60.0;  // |offset| and |attenuation| accepted, dB

// a number that ends at `stop` (or at the end of the string), finite and within +-kPowerDbMax
bool parse_db(const char *p, char **end, double *v)
{
    if (!*p || *p == ' ' || *p == '\t' || *p == '\n') return false;
    *v = strtod(p, end);
    return *end != p && std::isfinite(*v) && fabs(*v) <= kPowerDbMax;
}

bool parse_prn_power(const char *arg, double (&off)[GAL_NUM_PRN])
{
    const char *p = arg;
    for (;;) {
        char *end = nullptr;
        if (*p < '0' || *p > '9') return false;
        const long prn = strtol(p, &end, 10);
        if (prn < 1 || prn > GAL_NUM_PRN || *end != ':') return false;
        double db;
        p = end + 1;
        if (!parse_db(p, &end, &db)) return false;
        off[prn - 1] = db;
        if (!*end) return true;
        if (*end != ',') return false;
        p = end + 1;
    }
}

// GAL_GAIN_PATTERN_LEN numbers separated by white space or commas, nothing else (# starts a comment that runs to the end of the line)
bool load_antenna(const char *path, double (&pat)[GAL_GAIN_PATTERN_LEN], std::string *why)
{
    FILE *fp = fopen(path, "r");
    if (!fp) {
        *why = "cannot read it";
        return false;
    }
    std::string text;
    char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), fp)) > 0 && text.size() < (1u << 20)) text.append(buf, n);
    fclose(fp);
    int count = 0;
    const char *p = text.c_str();
    for (;;) {
        while (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r' || *p == ',') ++p;
        if (*p == '#') {
            while (*p && *p != '\n') ++p;
            continue;
        }
        if (!*p) break;
        char *end = nullptr;
        double v;
        if (!parse_db(p, &end, &v)) {
            *why = "value " + std::to_string(count + 1) + " is not a number of dB within +-60";
            return false;
        }
        if (count < GAL_GAIN_PATTERN_LEN) pat[count] = v;
        ++count;
        p = end;
    }
    if (count != GAL_GAIN_PATTERN_LEN) {
        *why = "it holds " + std::to_string(count) + " values, not " + std::to_string(GAL_GAIN_PATTERN_LEN);
        return false;
    }
    return true;
}

// --multipath <file>: one echo per line, prn,delay_m,rel_db,phase_deg[,fade_hz]; lines that begin with # and blank lines are skipped
struct EchoSpec {
    int prn;
    double delay_m, rel_db, phase_deg, fade_hz;
    gal_mpath_echo_t echo;  // made once the sample rate is known
};
constexpr int kEchoPerPrn = 4;

bool load_multipath(const char *path, std::vector<EchoSpec> *out, std::string *why)
{
    FILE *fp = fopen(path, "r");
    if (!fp) {
        *why = "cannot read it";
        return false;
    }
    char line[1024];
    int lineno = 0, per_prn[GAL_NUM_PRN + 1] = {0};
    bool ok = true;
    while (ok && fgets(line, sizeof(line), fp)) {
        ++lineno;
        const char *p = line;
        while (*p == ' ' || *p == '\t') ++p;
        if (*p == '#' || *p == '\n' || *p == '\r' || !*p) continue;
        EchoSpec e;
        memset(&e, 0, sizeof(e));
        double v[5] = {0, 0, 0, 0, 0};
        int n = 0;
        for (; n < 5; ++n) {
            char *end = nullptr;
            v[n] = strtod(p, &end);
            if (end == p || !std::isfinite(v[n])) break;
            p = end;
            while (*p == ' ' || *p == '\t') ++p;
            if (*p != ',') {
                ++n;
                break;
            }
            ++p;
        }
        while (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r') ++p;
        const std::string at = "line " + std::to_string(lineno);
        if (n < 4 || *p) {
            *why = at + " is not prn,delay_m,rel_db,phase_deg[,fade_hz]";
            ok = false;
        } else if (v[0] != floor(v[0]) || v[0] < 1 || v[0] > GAL_NUM_PRN) {
            *why = at + ": PRN outside 1.." + std::to_string(GAL_NUM_PRN);
            ok = false;
        } else if ((int)out->size() >= GAL_ECHO_MAX) {
            *why = "more than " + std::to_string(GAL_ECHO_MAX) + " echoes";
            ok = false;
        } else if (++per_prn[(int)v[0]] > kEchoPerPrn) {
            *why = at + ": more than " + std::to_string(kEchoPerPrn) + " echoes of PRN " + std::to_string((int)v[0]);
            ok = false;
        } else {
            e.prn = (int)v[0];
            e.delay_m = v[1], e.rel_db = v[2], e.phase_deg = v[3], e.fade_hz = v[4];
            out->push_back(e);
        }
    }
    fclose(fp);
    if (ok && out->empty()) {
        *why = "it holds no echo";
        ok = false;
    }
    return ok;
}

// ---- --sites: one child process per receiver site ---------------------------------------------------------------
struct Site {
    std::string llh, out;
};

int run_sites(const char *self, const std::vector<std::string> &base_args, const char *sites_file, const char *out_stem,
              int n_gpus, int per_gpu, int udp_base, const char *fmt_name, double bytes_per_sample, bool noise_on, bool osc_on, const char *monitor_file)
{
    std::vector<Site> sites;
    FILE *fp = fopen(sites_file, "r");
    if (!fp) {
        fprintf(stderr, "ERROR: cannot read the site list %s\n", sites_file);
        return 1;
    }
    char line[4096];
    while (fgets(line, sizeof(line), fp)) {
        double a, b, c;
        int used = 0;
        if (line[0] == '#' || sscanf(line, " %lf , %lf , %lf%n", &a, &b, &c, &used) != 3) continue;
        Site s;
        char buf[128];
        snprintf(buf, sizeof(buf), "%.10g,%.10g,%.10g", a, b, c);
        s.llh = buf;
        const char *rest = line + used;
        while (*rest == ' ' || *rest == ',' || *rest == '\t') ++rest;
        std::string name(rest);
        while (!name.empty() && (name.back() == '\n' || name.back() == '\r' || name.back() == ' ')) name.pop_back();
        if (name.empty()) {
            const std::string ext = std::string(".") + fmt_name;
            snprintf(buf, sizeof(buf), ".site%zu%s", sites.size(), ext.c_str());
            std::string stem(out_stem[0] ? out_stem : "galileosim");
            if (stem.size() > ext.size() && stem.compare(stem.size() - ext.size(), ext.size(), ext) == 0)
                stem.resize(stem.size() - ext.size());
            name = stem + buf;
        }
        s.out = name;
        sites.push_back(s);
    }
    fclose(fp);
    if (sites.empty()) {
        fprintf(stderr, "ERROR: no site (lat,lon,hgt) in %s\n", sites_file);
        return 1;
    }
    if (udp_base > 0 && (size_t)udp_base + sites.size() - 1 > 65535) {  // site k listens on port + k
        fprintf(stderr, "ERROR: -P %d with %zu sites runs past port 65535\n", udp_base, sites.size());
        return 1;
    }
    if (n_gpus <= 0) n_gpus = gal_synth_device_count();
    if (n_gpus <= 0) {
        fprintf(stderr, "ERROR: no usable gfx950 device (there is no CPU fallback)\n");
        return 1;
    }
    if (per_gpu < 1) per_gpu = 1;
    const int lanes = n_gpus * per_gpu;
    fprintf(stderr, "%zu sites over %d GPU%s (%d process%s per GPU)\n", sites.size(), n_gpus, n_gpus > 1 ? "s" : "", per_gpu,
            per_gpu > 1 ? "es" : "");
    std::vector<pid_t> lane_pid(lanes, 0);
    std::vector<int> lane_site(lanes, -1);
    std::vector<std::chrono::steady_clock::time_point> lane_t0(lanes);
    const auto t0 = std::chrono::steady_clock::now();
    size_t next = 0, done = 0;
    int failed = 0;
    long long total_bytes = 0;
    signal(SIGINT, on_sigint);
    while (done < sites.size()) {
        for (int l = 0; l < lanes && next < sites.size() && !g_stop; ++l) {
            if (lane_pid[l] != 0) continue;
            const Site &s = sites[next];
            std::vector<std::string> args(base_args);
            args.push_back("-l");
            args.push_back(s.llh);
            args.push_back("-o");
            args.push_back(s.out);
            args.push_back("-P");
            args.push_back(std::to_string(udp_base > 0 ? udp_base + (int)next : 0));
            if (noise_on) {  // site i: noise stream i -- two sites never share their noise
                args.push_back("--noise-stream");
                args.push_back(std::to_string(next));
            }
            if (osc_on) {  // ... nor their oscillator's phase noise
                args.push_back("--osc-stream");
                args.push_back(std::to_string(next));
            }
            if (monitor_file) {  // site i: <file>.site<i>
                args.push_back("--monitor");
                args.push_back(std::string(monitor_file) + ".site" + std::to_string(next));
            }
            const pid_t pid = fork();
            if (pid < 0) {
                perror("fork");
                return 1;
            }
            if (pid == 0) {
                char dev[16];
                snprintf(dev, sizeof(dev), "%d", l % n_gpus);
                setenv("GAL_DEVICE", dev, 1);
                std::vector<char *> av;
                av.push_back(const_cast<char *>(self));
                for (auto &a : args) av.push_back(const_cast<char *>(a.c_str()));
                av.push_back(nullptr);
                execv(self, av.data());
                perror("execv");
                _exit(127);
            }
            lane_pid[l] = pid;
            lane_site[l] = (int)next;
            lane_t0[l] = std::chrono::steady_clock::now();
            ++next;
        }
        int status = 0;
        const pid_t pid = wait(&status);
        if (pid < 0) {
            if (errno == EINTR) continue;
            break;
        }
        for (int l = 0; l < lanes; ++l) {
            if (lane_pid[l] != pid) continue;
            const Site &s = sites[lane_site[l]];
            struct stat sb;
            const long long bytes = stat(s.out.c_str(), &sb) == 0 ? (long long)sb.st_size : 0;
            const bool ok = WIFEXITED(status) && WEXITSTATUS(status) == 0;
            const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - lane_t0[l]).count();
            // (the child's wall time: HIP start-up, front-end, synthesis, device->host copy, file -- the sink, not the engine, sets it)
            fprintf(stderr, "site %d (%s) on GPU %d -> %s: %s, %lld bytes in %.2f s = %.0f Msamples/s = %.2f GB/s into its file\n", lane_site[l],
                    s.llh.c_str(), l % n_gpus, s.out.c_str(), ok ? "ok" : "FAILED", bytes, dt, bytes / bytes_per_sample / dt / 1e6, bytes / dt / 1e9);
            if (!ok) ++failed;
            total_bytes += bytes;
            lane_pid[l] = 0;
            ++done;
        }
        if (g_stop && next < sites.size()) {  // interrupted: the sites not started yet are dropped
            done += sites.size() - next;
            next = sites.size();
        }
    }
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "\nDone!\nSites = %zu  failed = %d  Process time = %.2f [sec]  (%.1f Msamples/s aggregate over %d GPU%s, incl. process "
                    "start-up; per site the device->host link and the file system bound this figure, not the synthesis engine: see the "
                    "per-site lines)\n", sites.size(), failed, el, total_bytes / bytes_per_sample / el / 1e6, n_gpus, n_gpus > 1 ? "s" : "");
    return failed ? 1 : 0;
}

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

}  // namespace

// GAL_CLI_TIMING=1: where the start-up goes (stage times on stderr)
static void stage(const char *what)
{
    static const bool on = getenv("GAL_CLI_TIMING") != nullptr;
    static auto t0 = std::chrono::steady_clock::now();
    static auto tl = t0;
    if (!on) return;
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "[timing] %-28s +%7.1f ms  (%7.1f ms since start)\n", what, std::chrono::duration<double, std::milli>(t - tl).count(),
            std::chrono::duration<double, std::milli>(t - t0).count());
    tl = t;
}

int main(int argc, char *argv[])
{
    stage("process start");
    if (argc < 3) {
        usage(argv[0]);
        exit(1);
    }
    gal_scen_cfg_t sc;
    memset(&sc, 0, sizeof(sc));
    char navfile[4096] = "", outfile[4096] = "", umfile[4096] = "", sitesfile[4096] = "";
    sc.llh[0] = 42.3601;  // defaults of src/main.cpp:179-196
    sc.llh[1] = -71.0589;
    sc.llh[2] = 2;
    sc.duration_s = 300.0;
    sc.iono_enable = 1;
    sc.n_slots = GAL_MAX_CHAN;
    bool verbose = false, have_batch = false, udp_given = false, realtime = false, cboc = false, exact_replay = false, shift_toe = false, ref_T = false;
    int batch_epochs = 128, n_writers = -1, sites_gpus = 0, sites_per_gpu = 1;
    const char *iq_format_arg = "ishort", *iq_shift_arg = nullptr;
    const char *monitor_arg = nullptr, *monitor_every_arg = nullptr;
    const char *fir_arg = nullptr, *fir_lowpass_arg = nullptr, *oversample_arg = nullptr, *multipath_arg = nullptr;
    bool agc_given = false;
    const char *agc_arg = nullptr, *agc_block_arg = nullptr, *agc_window_arg = nullptr, *agc_init_arg = nullptr, *agc_log_arg = nullptr, *i2bit_thr_arg = nullptr;
    bool power_model = false;
    const char *antenna_arg = nullptr;
    std::vector<const char *> prn_power_args;
    const char *cn0_arg = nullptr, *noise_seed_arg = nullptr, *noise_stream_arg = nullptr, *signal_gain_arg = nullptr;
    std::vector<const char *> jam_args;
    const char *lo_offset_arg = nullptr, *phase_noise_arg = nullptr, *osc_seed_arg = nullptr, *osc_stream_arg = nullptr;
    sc.udp_port = GAL_SCEN_UDP_PORT;  // the reference always listens for position updates (src/galileo-sdr.cpp:185)
    sc.udp_loopback = 1;              // ... on every interface; the default listener here takes local datagrams only

    enum { OPT_STRICT = 1000, OPT_SITES, OPT_WRITERS, OPT_GPUS, OPT_PER_GPU, OPT_EXACT, OPT_SHIFT_TOE, OPT_REF_T, OPT_IQ_FORMAT, OPT_IQ_SHIFT, OPT_CN0, OPT_NOISE_SEED,
           OPT_NOISE_STREAM, OPT_SIGNAL_GAIN, OPT_MONITOR, OPT_MONITOR_EVERY, OPT_JAM, OPT_POWER_MODEL, OPT_ANTENNA, OPT_PRN_POWER, OPT_FIR, OPT_FIR_LOWPASS, OPT_OVERSAMPLE,
           OPT_AGC, OPT_AGC_BLOCK, OPT_AGC_WINDOW, OPT_AGC_INIT, OPT_AGC_LOG, OPT_I2BIT_THR, OPT_MULTIPATH, OPT_LO_OFFSET, OPT_PHASE_NOISE, OPT_OSC_SEED, OPT_OSC_STREAM };
    static const struct option long_opts[] = {{"strict", no_argument, nullptr, OPT_STRICT},
                                              {"exact-replay", no_argument, nullptr, OPT_EXACT},
                                              {"shift-toe", no_argument, nullptr, OPT_SHIFT_TOE},
                                             {"ref-T", no_argument, nullptr, OPT_REF_T},
                                              {"sites", required_argument, nullptr, OPT_SITES},
                                              {"writers", required_argument, nullptr, OPT_WRITERS},
                                              {"gpus", required_argument, nullptr, OPT_GPUS},
                                              {"per-gpu", required_argument, nullptr, OPT_PER_GPU},
                                              {"iq-format", required_argument, nullptr, OPT_IQ_FORMAT},
                                              {"iq-shift", required_argument, nullptr, OPT_IQ_SHIFT},
                                              {"cn0", required_argument, nullptr, OPT_CN0},
                                              {"noise-seed", required_argument, nullptr, OPT_NOISE_SEED},
                                              {"noise-stream", required_argument, nullptr, OPT_NOISE_STREAM},
                                              {"signal-gain", required_argument, nullptr, OPT_SIGNAL_GAIN},
                                              {"monitor", required_argument, nullptr, OPT_MONITOR},
                                              {"monitor-every", required_argument, nullptr, OPT_MONITOR_EVERY},
                                              {"jam", required_argument, nullptr, OPT_JAM},
                                              {"power-model", no_argument, nullptr, OPT_POWER_MODEL},
                                              {"antenna", required_argument, nullptr, OPT_ANTENNA},
                                              {"prn-power", required_argument, nullptr, OPT_PRN_POWER},
                                              {"fir", required_argument, nullptr, OPT_FIR},
                                              {"fir-lowpass", required_argument, nullptr, OPT_FIR_LOWPASS},
                                              {"oversample", required_argument, nullptr, OPT_OVERSAMPLE},
                                              {"agc", optional_argument, nullptr, OPT_AGC},
                                              {"agc-block", required_argument, nullptr, OPT_AGC_BLOCK},
                                              {"agc-window", required_argument, nullptr, OPT_AGC_WINDOW},
                                              {"agc-init-rms", required_argument, nullptr, OPT_AGC_INIT},
                                              {"agc-log", required_argument, nullptr, OPT_AGC_LOG},
                                              {"i2bit-threshold", required_argument, nullptr, OPT_I2BIT_THR},
                                              {"multipath", required_argument, nullptr, OPT_MULTIPATH},
                                              {"lo-offset", required_argument, nullptr, OPT_LO_OFFSET},
                                              {"phase-noise", required_argument, nullptr, OPT_PHASE_NOISE},
                                              {"osc-seed", required_argument, nullptr, OPT_OSC_SEED},
                                              {"osc-stream", required_argument, nullptr, OPT_OSC_STREAM},
                                              {nullptr, 0, nullptr, 0}};
    std::vector<std::string> child_args;  // --sites: everything but -l / -o / --sites / --gpus / --per-gpu / --noise-stream goes to the children
    int opt;
    while ((opt = getopt_long(argc, argv, "e:n:o:u:g:l:T:t:d:G:a:p:iI:U:b:vB:P:rC", long_opts, nullptr)) != -1) {
        // `--agc 4096`: getopt takes an optional argument only as --agc=4096; a following word that begins like a number is the target
        if (opt == OPT_AGC && !optarg && optind < argc && ((argv[optind][0] >= '0' && argv[optind][0] <= '9') || argv[optind][0] == '.'))
            optarg = argv[optind++];
        if (opt != 'l' && opt != 'o' && opt != 'P' && opt != OPT_SITES && opt != OPT_GPUS && opt != OPT_PER_GPU && opt != OPT_NOISE_STREAM && opt != OPT_OSC_STREAM && opt != OPT_MONITOR && opt != OPT_AGC_LOG && opt != '?' && opt != ':') {
            if (opt >= 1000) {
                child_args.push_back(opt == OPT_STRICT ? "--strict" : opt == OPT_EXACT ? "--exact-replay" : opt == OPT_SHIFT_TOE ? "--shift-toe" : opt == OPT_REF_T ? "--ref-T"
                                     : opt == OPT_IQ_FORMAT ? "--iq-format" : opt == OPT_IQ_SHIFT ? "--iq-shift" : opt == OPT_CN0 ? "--cn0"
                                     : opt == OPT_NOISE_SEED ? "--noise-seed" : opt == OPT_SIGNAL_GAIN ? "--signal-gain" : opt == OPT_MONITOR_EVERY ? "--monitor-every" : opt == OPT_JAM ? "--jam" : opt == OPT_POWER_MODEL ? "--power-model"
                                     : opt == OPT_ANTENNA ? "--antenna" : opt == OPT_PRN_POWER ? "--prn-power" : opt == OPT_FIR ? "--fir" : opt == OPT_FIR_LOWPASS ? "--fir-lowpass" : opt == OPT_OVERSAMPLE ? "--oversample"
                                     : opt == OPT_AGC ? "--agc" : opt == OPT_AGC_BLOCK ? "--agc-block" : opt == OPT_AGC_WINDOW ? "--agc-window" : opt == OPT_AGC_INIT ? "--agc-init-rms"
                                     : opt == OPT_I2BIT_THR ? "--i2bit-threshold" : opt == OPT_MULTIPATH ? "--multipath" : opt == OPT_LO_OFFSET ? "--lo-offset"
                                     : opt == OPT_PHASE_NOISE ? "--phase-noise" : opt == OPT_OSC_SEED ? "--osc-seed" : "--writers");
            } else {
                char name[3] = {'-', (char)opt, 0};
                child_args.push_back(name);
            }
            if (optarg) child_args.push_back(optarg);
        }
        switch (opt) {
        case 'e': snprintf(navfile, sizeof(navfile), "%s", optarg); break;
        case 'o': snprintf(outfile, sizeof(outfile), "%s", optarg); break;
        case 'u': snprintf(umfile, sizeof(umfile), "%s", optarg); break;
        case 'l': sscanf(optarg, "%lf,%lf,%lf", &sc.llh[0], &sc.llh[1], &sc.llh[2]); break;
        case 'T':  // -t without the range check, UTC reference time overwritten (src/main.cpp:237-257; galscen.h: time_overwrite)
            if (!sc.time_overwrite) sc.time_overwrite = 1;
            if (strncmp(optarg, "now", 3) == 0) {
                time_t timer;
                time(&timer);
                const struct tm *gmt = gmtime(&timer);
                sc.start[0] = gmt->tm_year + 1900; sc.start[1] = gmt->tm_mon + 1; sc.start[2] = gmt->tm_mday;
                sc.start[3] = gmt->tm_hour; sc.start[4] = gmt->tm_min;
                sc.start_sec = (double)gmt->tm_sec;
                sc.have_start = 1;
                break;
            }
            /* fall through */
        case 't':
            if (sscanf(optarg, "%d/%d/%d,%d:%d:%lf", &sc.start[0], &sc.start[1], &sc.start[2], &sc.start[3],
                       &sc.start[4], &sc.start_sec) != 6) {
                printf("ERROR: Invalid date and time.\n");
                exit(1);
            }
            sc.have_start = 1;
            break;
        case 'd': sc.duration_s = atof(optarg); break;
        case 'I': sc.iono_enable = 0; break;
        case 'v': verbose = true; break;
        case 'B': batch_epochs = atoi(optarg); have_batch = true; break;
        case 'P':
            sc.udp_port = atoi(optarg);
            sc.udp_loopback = 0;
            udp_given = true;
            break;
        case 'r': realtime = true; break;
        case 'C': cboc = true; break;
        case OPT_STRICT: sc.strict_eph = 1; break;
        case OPT_EXACT: exact_replay = true; break;
        case OPT_SHIFT_TOE: shift_toe = true; break;
        case OPT_REF_T: ref_T = true; break;
        case OPT_SITES: snprintf(sitesfile, sizeof(sitesfile), "%s", optarg); break;
        case OPT_WRITERS: n_writers = atoi(optarg); break;
        case OPT_GPUS: sites_gpus = atoi(optarg); break;
        case OPT_PER_GPU: sites_per_gpu = atoi(optarg); break;
        case OPT_IQ_FORMAT: iq_format_arg = optarg; break;
        case OPT_IQ_SHIFT: iq_shift_arg = optarg; break;
        case OPT_CN0: cn0_arg = optarg; break;
        case OPT_NOISE_SEED: noise_seed_arg = optarg; break;
        case OPT_NOISE_STREAM: noise_stream_arg = optarg; break;
        case OPT_LO_OFFSET: lo_offset_arg = optarg; break;
        case OPT_PHASE_NOISE: phase_noise_arg = optarg; break;
        case OPT_OSC_SEED: osc_seed_arg = optarg; break;
        case OPT_OSC_STREAM: osc_stream_arg = optarg; break;
        case OPT_SIGNAL_GAIN: signal_gain_arg = optarg; break;
        case OPT_MONITOR: monitor_arg = optarg; break;
        case OPT_MONITOR_EVERY: monitor_every_arg = optarg; break;
        case OPT_JAM: jam_args.push_back(optarg); break;
        case OPT_POWER_MODEL: power_model = true; break;
        case OPT_ANTENNA: antenna_arg = optarg; break;
        case OPT_PRN_POWER: prn_power_args.push_back(optarg); break;
        case OPT_FIR: fir_arg = optarg; break;
        case OPT_FIR_LOWPASS: fir_lowpass_arg = optarg; break;
        case OPT_OVERSAMPLE: oversample_arg = optarg; break;
        case OPT_MULTIPATH: multipath_arg = optarg; break;
        case OPT_AGC: agc_given = true; agc_arg = optarg; break;
        case OPT_AGC_BLOCK: agc_block_arg = optarg; break;
        case OPT_AGC_WINDOW: agc_window_arg = optarg; break;
        case OPT_AGC_INIT: agc_init_arg = optarg; break;
        case OPT_AGC_LOG: agc_log_arg = optarg; break;
        case OPT_I2BIT_THR: i2bit_thr_arg = optarg; break;
        case 'n': case 'g': case 'G': case 'a': case 'p': case 'i': case 'U': case 'b': break;
        case ':':
        case '?':
            usage(argv[0]);
            exit(1);
        default: break;
        }
    }
    if (navfile[0] == 0) {
        printf("ERROR: Galileo ephemeris/nav_msg file is not specified.\n");
        exit(1);
    }
    // plain -T is the reference as built (time_overwrite 1: the same command line gives the same bytes; ADVICE r5 -- round 5 had it
    // shift, and every replay of a reference command line had to add --ref-T); --shift-toe asks for the shift of TOC / TOE (2)
    if ((shift_toe || ref_T) && !sc.time_overwrite) {
        printf("ERROR: %s needs -T <date,time>.\n", ref_T ? "--ref-T" : "--shift-toe");
        exit(1);
    }
    if (shift_toe && ref_T) {
        printf("ERROR: --shift-toe and --ref-T exclude each other.\n");
        exit(1);
    }
    if (sc.time_overwrite) sc.time_overwrite = shift_toe ? 2 : 1;
    // output format: checked here, before any device work
    static const char *const kIqNames[] = {"ishort", "ibyte", "ibit", "i2bit"};  // GAL_IQ_ISHORT, GAL_IQ_IBYTE, GAL_IQ_IBIT, GAL_IQ_I2BIT
    int iq_format = -1, iq_shift = 0;
    for (int f = 0; f < 4; ++f)
        if (strcmp(iq_format_arg, kIqNames[f]) == 0) iq_format = f;
    if (iq_format < 0) {
        fprintf(stderr, "ERROR: unknown --iq-format '%s' (accepted: ishort, ibyte, ibit, i2bit).\n", iq_format_arg);
        exit(1);
    }
    // AGC: the strings are checked here, before any device work; the parameters are made below, once shift and sigma are known.
    // Without --agc and i2bit nothing below differs from a build without them.
    const bool agc_on = agc_given || iq_format == GAL_IQ_I2BIT;  // the 2-bit format implies the AGC
    if (!agc_on && (agc_block_arg || agc_window_arg || agc_init_arg || agc_log_arg)) {
        fprintf(stderr, "ERROR: --agc-block, --agc-window, --agc-init-rms and --agc-log need --agc.\n");
        exit(1);
    }
    if (agc_on && iq_format == GAL_IQ_IBIT) {
        fprintf(stderr, "ERROR: --agc does not go with --iq-format ibit: a sign needs no gain control.\n");
        exit(1);
    }
    if (monitor_arg && iq_format == GAL_IQ_I2BIT) {
        fprintf(stderr, "ERROR: --monitor does not read --iq-format i2bit (ishort and ibyte, with or without --agc, it does).\n");
        exit(1);
    }
    int i2bit_thr = 1024;
    if (i2bit_thr_arg) {
        char *end = nullptr;
        const long v = strtol(i2bit_thr_arg, &end, 10);
        if (iq_format != GAL_IQ_I2BIT) {
            fprintf(stderr, "ERROR: --i2bit-threshold applies to --iq-format i2bit only.\n");
            exit(1);
        }
        if (!*i2bit_thr_arg || *end || v < 1 || v > 32767) {
            fprintf(stderr, "ERROR: --i2bit-threshold '%s' out of range (1..32767).\n", i2bit_thr_arg);
            exit(1);
        }
        i2bit_thr = (int)v;
    }
    long agc_block = 2600, agc_window = 8;
    double agc_target = 0.0, agc_init = -1.0;  // (0 / < 0: the defaults, known further down)
    if (agc_on) {
        char *end = nullptr;
        if (agc_block_arg) {
            agc_block = strtol(agc_block_arg, &end, 10);
            if (!*agc_block_arg || *end || agc_block < GAL_AGC_MIN_BLOCK || agc_block > GAL_AGC_MAX_BLOCK) {
                fprintf(stderr, "ERROR: --agc-block '%s' out of range (%d..%d samples).\n", agc_block_arg, GAL_AGC_MIN_BLOCK, GAL_AGC_MAX_BLOCK);
                exit(1);
            }
        }
        if (agc_window_arg) {
            agc_window = strtol(agc_window_arg, &end, 10);
            if (!*agc_window_arg || *end || agc_window < 1 || agc_window > GAL_AGC_MAX_WINDOW) {
                fprintf(stderr, "ERROR: --agc-window '%s' out of range (1..%d blocks).\n", agc_window_arg, GAL_AGC_MAX_WINDOW);
                exit(1);
            }
        }
        if (agc_block * agc_window > GAL_AGC_MAX_SPAN) {
            fprintf(stderr, "ERROR: --agc-block %ld x --agc-window %ld = %ld samples, more than %d.\n", agc_block, agc_window, agc_block * agc_window,
                    GAL_AGC_MAX_SPAN);
            exit(1);
        }
        if (agc_arg) {
            agc_target = strtod(agc_arg, &end);
            if (!*agc_arg || *end || !(agc_target >= 1.0 / 256.0 && agc_target <= 32767.0)) {
                fprintf(stderr, "ERROR: --agc '%s' is not a target rms in int16 LSB (up to 32767).\n", agc_arg);
                exit(1);
            }
        }
        if (agc_init_arg) {
            agc_init = strtod(agc_init_arg, &end);
            if (!*agc_init_arg || *end || !(agc_init >= 0.0 && agc_init <= 32768.0)) {
                fprintf(stderr, "ERROR: --agc-init-rms '%s' out of range (0..32768 int16 LSB).\n", agc_init_arg);
                exit(1);
            }
        }
        if (agc_log_arg && (!*agc_log_arg || strcmp(agc_log_arg, "-") == 0)) {
            fprintf(stderr, "ERROR: --agc-log needs a file name.\n");
            exit(1);
        }
        if (agc_log_arg && sitesfile[0]) {
            fprintf(stderr, "ERROR: --agc-log writes one file; it does not go with --sites.\n");
            exit(1);
        }
    }
    if (iq_shift_arg) {
        char *end = nullptr;
        const long v = strtol(iq_shift_arg, &end, 10);
        if (iq_format != GAL_IQ_IBYTE) {
            fprintf(stderr, "ERROR: --iq-shift applies to --iq-format ibyte only.\n");
            exit(1);
        }
        if (!*iq_shift_arg || *end || v < 0 || v > 15) {
            fprintf(stderr, "ERROR: --iq-shift '%s' out of range (0..15).\n", iq_shift_arg);
            exit(1);
        }
        iq_shift = (int)v;
    } else if (iq_format == GAL_IQ_IBYTE) {
        iq_shift = 5;  // sigma of 9-12 channels ~ 750-870 LSB: 23-27 LSB after the shift, the clamp at ~5 sigma
    }
    // per-satellite signal power: checked here too.  Without the three options nothing below differs from a build without them.
    const bool power_on = power_model || antenna_arg || !prn_power_args.empty();
    double ant_db[GAL_GAIN_PATTERN_LEN], prn_db[GAL_NUM_PRN];
    memset(ant_db, 0, sizeof(ant_db));
    memset(prn_db, 0, sizeof(prn_db));
    for (const char *a : prn_power_args)
        if (!parse_prn_power(a, prn_db)) {
            fprintf(stderr, "ERROR: --prn-power '%s' is not prn:dB[,prn:dB...] (PRN 1..%d, -60..60 dB).\n", a, GAL_NUM_PRN);
            exit(1);
        }
    if (antenna_arg) {
        std::string why;
        if (!load_antenna(antenna_arg, ant_db, &why)) {
            fprintf(stderr, "ERROR: --antenna %s: %s.\n", antenna_arg, why.c_str());
            exit(1);
        }
    }
    // the largest gain the options can produce, as a factor: the path loss of a satellite at the zenith of a low orbit point (the
    // nominal altitude against 22 900 km: 1.4 %), the least attenuation of the pattern, the largest offset (PRNs without one: 0 dB).
    // It scales the 4100 LSB of the headroom rules below
    double power_peak = 1.0;
    if (power_on) {
        double att = ant_db[0], off = 0.0;
        for (double v : ant_db) att = v < att ? v : att;
        for (double v : prn_db) off = v > off ? v : off;
        power_peak = (power_model ? 23222000.0 / 22900000.0 : 1.0) * pow(10.0, -att / 20.0) * pow(10.0, off / 20.0);
        if (!sitesfile[0])
            fprintf(stderr, "Signal power: path loss %s, antenna %s, %zu PRN offset list%s; largest gain %.3f (%.2f dB)\n", power_model ? "on" : "off",
                    antenna_arg ? antenna_arg : "isotropic", prn_power_args.size(), prn_power_args.size() == 1 ? "" : "s", power_peak,
                    20.0 * log10(power_peak));
    }
    // --multipath: the file is read here, before any device work.  Without the option nothing below differs from a build without it.
    // A satellite with echoes can reach 1 + sum alpha times its own amplitude: the largest such sum scales the headroom's signal term
    std::vector<EchoSpec> echoes;
    double echo_peak = 1.0;
    if (multipath_arg) {
        std::string why;
        if (!load_multipath(multipath_arg, &echoes, &why)) {
            fprintf(stderr, "ERROR: --multipath %s: %s.\n", multipath_arg, why.c_str());
            exit(1);
        }
        double sum[GAL_NUM_PRN + 1] = {0};
        for (const EchoSpec &e : echoes) {
            sum[e.prn] += pow(10.0, e.rel_db / 20.0);
            echo_peak = 1.0 + sum[e.prn] > echo_peak ? 1.0 + sum[e.prn] : echo_peak;
        }
    }
    const bool mp_on = !echoes.empty();
    const double sig_peak = 4100.0 * power_peak * echo_peak;  // the largest |x| of the signal sum: 4100 in the reference's scenarios
    // noise floor: checked here too.  Without --cn0 nothing below differs from a build without it.
    // --oversample M: everything in front of the decimator runs at M x 2.6 MS/s (kSampleRate); the file and --monitor at kOutRate.
    // Without the option M = 1 and the two are the same number.
    int osr = 1;
    if (oversample_arg) {
        char *end = nullptr;
        const long v = strtol(oversample_arg, &end, 10);
        if (!*oversample_arg || *end || v < 2 || v > 15) {
            fprintf(stderr, "ERROR: --oversample '%s' out of range (2..15: the engine synthesises at up to 40 MS/s).\n", oversample_arg);
            exit(1);
        }
        osr = (int)v;
    }
    const bool dec_on = osr > 1;
    const double kOutRate = 2.6e6;
    const int kOutSamplesPerEpoch = 260000;
    const double kSampleRate = (double)osr * 2.6e6;
    const double kLight = 299792458.0;
    for (size_t k = 0; k < echoes.size(); ++k) {  // the delays in samples of the rate the pass runs at
        EchoSpec &e = echoes[k];
        if (gal_synth_mpath_make(e.delay_m / kLight, e.rel_db, e.phase_deg, e.fade_hz, kSampleRate, &e.echo) != GAL_OK) {
            fprintf(stderr, "ERROR: --multipath %s, echo %zu (PRN %d): %s\n", multipath_arg, k + 1, e.prn, gal_synth_last_error());
            exit(1);
        }
        if (!sitesfile[0])
            fprintf(stderr, "Multipath %zu: PRN %d, delay %u samples = %.2f m (asked %.2f m), amplitude %.4f (%.2f dB), phase %.2f deg, fading %.3f Hz\n",
                    k + 1, e.prn, e.echo.delay, e.echo.delay / kSampleRate * kLight, e.delay_m, e.echo.alpha_q12 / 4096.0, e.rel_db,
                    e.echo.ph0 / 4294967296.0 * 360.0, e.echo.dph / 4294967296.0 * kSampleRate);
    }
    if (mp_on && !sitesfile[0] && echo_peak > 1.0)
        fprintf(stderr, "Multipath: %zu echo%s; a satellite reaches up to %.3f times its own amplitude\n", echoes.size(), echoes.size() == 1 ? "" : "es", echo_peak);
    bool noise_on = false;
    gal_iq_noise_t noise;
    memset(&noise, 0, sizeof(noise));
    if (!cn0_arg && (noise_seed_arg || noise_stream_arg || (signal_gain_arg && jam_args.empty()))) {
        fprintf(stderr, "ERROR: --noise-seed, --noise-stream and --signal-gain need --cn0 <dBHz>.\n");
        exit(1);
    }
    // interference: the strings are checked here, the sources are made below, once the signal gain is known.  Without --jam nothing
    // below differs from a build without it.
    JamSpec jam[GAL_INTERF_MAX];
    const int n_jam = (int)jam_args.size();
    double jam_unit = 0.0;  // the sum of the amplitudes at signal gain 1, int16 LSB
    if (n_jam > GAL_INTERF_MAX) {
        fprintf(stderr, "ERROR: --jam may be given %d times at most.\n", GAL_INTERF_MAX);
        exit(1);
    }
    for (int k = 0; k < n_jam; ++k) {
        gal_iq_interf_t probe;
        if (!parse_jam(jam_args[k], &jam[k])) {
            fprintf(stderr, "ERROR: --jam '%s' is not js_db,f_hz[,f_hi_hz,sweep_us[,period_us,on_us]].\n", jam_args[k]);
            exit(1);
        }
        if (gal_synth_interf_make(jam[k].js_db, 0.0, kSampleRate, jam[k].f_lo, jam[k].f_hi, jam[k].sweep_s, jam[k].period_s, jam[k].on_s,
                                  &probe) != GAL_OK) {  // (gain 0: everything but the amplitude)
            fprintf(stderr, "ERROR: --jam %s: %s\n", jam_args[k], gal_synth_last_error());
            exit(1);
        }
        jam_unit += 250.0 * sqrt(2.0) * pow(10.0, jam[k].js_db / 20.0);
    }
    double gain = 1.0;
    const auto given_gain = [&]() {
        char *end = nullptr;
        gain = strtod(signal_gain_arg, &end);
        if (!*signal_gain_arg || *end || !(gain > 0.0 && gain <= 16.0)) {
            fprintf(stderr, "ERROR: --signal-gain '%s' out of range (0 < g <= 16).\n", signal_gain_arg);
            exit(1);
        }
    };
    if (cn0_arg) {
        char *end = nullptr;
        const double cn0 = strtod(cn0_arg, &end);
        if (!*cn0_arg || *end) {
            fprintf(stderr, "ERROR: --cn0 '%s' is not a number (dB-Hz).\n", cn0_arg);
            exit(1);
        }
        if (signal_gain_arg) {
            given_gain();
        } else {
            // the largest power of two <= 1 with 5 sigma + 4100 g + the --jam amplitudes <= 32767 (4100: the largest |x| of the
            // reference's scenarios); sigma and the amplitudes are proportional to g
            gal_iq_noise_t unit;
            if (gal_synth_noise_from_cn0(cn0, kSampleRate, 1.0, &unit) != GAL_OK) {
                fprintf(stderr, "ERROR: --cn0 %s: %s\n", cn0_arg, gal_synth_last_error());
                exit(1);
            }
            gain = 1.0;
            while (gain > 1.0 / 65536.0 && (5.0 * (unit.sigma_q4 / 16.0) + sig_peak + jam_unit) * gain > 32767.0) gain *= 0.5;
        }
        if (gal_synth_noise_from_cn0(cn0, kSampleRate, gain, &noise) != GAL_OK) {
            fprintf(stderr, "ERROR: --cn0 %s: %s\n", cn0_arg, gal_synth_last_error());
            exit(1);
        }
        noise.seed = 1;
        if (noise_seed_arg) {
            errno = 0;
            noise.seed = strtoull(noise_seed_arg, &end, 0);
            if (!*noise_seed_arg || *end || errno || noise_seed_arg[0] == '-') {
                fprintf(stderr, "ERROR: --noise-seed '%s' is not an unsigned 64-bit integer.\n", noise_seed_arg);
                exit(1);
            }
        }
        if (noise_stream_arg) {
            errno = 0;
            const unsigned long long v = strtoull(noise_stream_arg, &end, 0);
            if (!*noise_stream_arg || *end || errno || noise_stream_arg[0] == '-' || v > 0xffffffffull) {
                fprintf(stderr, "ERROR: --noise-stream '%s' is not an unsigned 32-bit integer.\n", noise_stream_arg);
                exit(1);
            }
            noise.stream = (uint32_t)v;
        }
        noise_on = true;
        const double sigma = noise.sigma_q4 / 16.0;
        if (iq_format == GAL_IQ_IBYTE && !iq_shift_arg && !dec_on) {  // the smallest shift with 127 x 2^s >= 4 sigma + the --jam amplitudes
            iq_shift = 0;
            while (iq_shift < 15 && 127.0 * (double)(1 << iq_shift) < 4.0 * sigma + (agc_on ? 0.0 : jam_unit * gain)) ++iq_shift;
        }
        if (!sitesfile[0]) {  // (--sites: every child prints its own)
            fprintf(stderr, "Noise floor: C/N0 %g dB-Hz -> sigma %.1f LSB, signal gain %g%s, seed %llu, stream %u", cn0, sigma, gain,
                    signal_gain_arg ? "" : " (chosen)", (unsigned long long)noise.seed, noise.stream);
            if (iq_format == GAL_IQ_IBYTE && (!dec_on || iq_shift_arg)) fprintf(stderr, ", --iq-shift %d%s", iq_shift, iq_shift_arg ? "" : " (chosen)");
            fprintf(stderr, "\n");
        }
    }
    gal_iq_interf_t interf[GAL_INTERF_MAX];
    memset(interf, 0, sizeof(interf));
    if (n_jam > 0) {
        if (!cn0_arg) {  // the sources alone on top of the scaled signals
            if (signal_gain_arg) given_gain();
            else
                while (gain > 1.0 / 65536.0 && (sig_peak + jam_unit) * gain > 32767.0) gain *= 0.5;
            noise.gain_q16 = (uint32_t)llround(gain * 65536.0);  // (sigma_q4 0: nothing random is computed)
            if (iq_format == GAL_IQ_IBYTE && !iq_shift_arg) {  // the smallest shift with 127 x 2^s >= 4100 g + the amplitudes
                iq_shift = 0;
                while (iq_shift < 15 && 127.0 * (double)(1 << iq_shift) < (sig_peak + (agc_on ? 0.0 : jam_unit)) * gain) ++iq_shift;
            }
        }
        for (int k = 0; k < n_jam; ++k)
            if (gal_synth_interf_make(jam[k].js_db, gain, kSampleRate, jam[k].f_lo, jam[k].f_hi, jam[k].sweep_s, jam[k].period_s, jam[k].on_s,
                                      &interf[k]) != GAL_OK) {
                fprintf(stderr, "ERROR: --jam %s: %s\n", jam_args[k], gal_synth_last_error());
                exit(1);
            }
        if (!sitesfile[0]) {  // (--sites: every child prints its own)
            if (!cn0_arg) {
                fprintf(stderr, "Interference without a noise floor: signal gain %g%s", gain, signal_gain_arg ? "" : " (chosen)");
                if (iq_format == GAL_IQ_IBYTE) fprintf(stderr, ", --iq-shift %d%s", iq_shift, iq_shift_arg ? "" : " (chosen)");
                fprintf(stderr, "\n");
            }
            for (int k = 0; k < n_jam; ++k) {
                const gal_iq_interf_t &c = interf[k];
                const double f_lo = c.f0 / 4294967296.0 * kSampleRate;
                fprintf(stderr, "Interference %d: J/S %g dB -> A %.1f LSB, %.1f Hz .. %.1f Hz, sweep %u samples, pulse %u of %u samples\n", k + 1,
                        jam[k].js_db, c.amp_q4 / 16.0, f_lo, f_lo + (double)c.df * c.sweep_len / 4294967296.0 * kSampleRate, c.sweep_len,
                        c.pulse_on, c.pulse_period);
            }
        }
    }
    const bool mix_on = noise_on || n_jam > 0;  // a pass over the final int16 batch in front of the format
    // monitor: checked here too, before any device work.  Without --monitor nothing below differs from a build without it.
    int monitor_every = 10;
    FILE *monitor_fp = nullptr;
    if (monitor_every_arg) {
        char *end = nullptr;
        const long v = strtol(monitor_every_arg, &end, 10);
        if (!monitor_arg) {
            fprintf(stderr, "ERROR: --monitor-every needs --monitor <file>.\n");
            exit(1);
        }
        if (!*monitor_every_arg || *end || v < 1 || v > 1000000) {
            fprintf(stderr, "ERROR: --monitor-every '%s' out of range (1..1000000 epochs).\n", monitor_every_arg);
            exit(1);
        }
        monitor_every = (int)v;
    }
    if (monitor_arg) {
        if (!*monitor_arg || strcmp(monitor_arg, "-") == 0) {
            fprintf(stderr, "ERROR: --monitor needs a file name.\n");
            exit(1);
        }
        if (cboc) {
            fprintf(stderr, "ERROR: --monitor despreads with the BOC(1,1) replica; it does not go with -C.\n");
            exit(1);
        }
        if (!sitesfile[0]) {  // (--sites: every child opens its own <file>.site<i>)
            monitor_fp = fopen(monitor_arg, "w");
            if (!monitor_fp) {
                fprintf(stderr, "ERROR: cannot write the monitor file %s.\n", monitor_arg);
                exit(1);
            }
            fprintf(monitor_fp, "time_s,prn,doppler_hz,cn0_dbhz,peak_ratio,best_delay_halfchips,best_doppler_bins\n");
        }
    }
    // front-end filter: checked here too, before any device work.  Without --fir / --fir-lowpass nothing below differs from a build
    // without them.
    int16_t fir_taps[GAL_FIRDEC_MAX_TAPS];
    int n_fir = 0;
    const int fir_max = dec_on ? GAL_FIRDEC_MAX_TAPS : GAL_FIR_MAX_TAPS;  // --oversample: the taps are the decimator's
    if (fir_arg && fir_lowpass_arg) {
        fprintf(stderr, "ERROR: --fir and --fir-lowpass exclude each other.\n");
        exit(1);
    }
    if (fir_arg) {
        FILE *fp = fopen(fir_arg, "r");
        if (!fp) {
            fprintf(stderr, "ERROR: cannot read the tap file %s.\n", fir_arg);
            exit(1);
        }
        char line[256];
        int lineno = 0;
        while (fgets(line, sizeof(line), fp)) {
            ++lineno;
            char *b = line, *end = nullptr;
            while (*b == ' ' || *b == '\t') ++b;
            if (*b == '\n' || *b == '\r' || *b == 0) continue;  // an empty line
            errno = 0;
            const long v = strtol(b, &end, 10);
            while (*end == ' ' || *end == '\t' || *end == '\r' || *end == '\n') ++end;
            if (end == b || *end || errno || v < -32768 || v > 32767) {
                fprintf(stderr, "ERROR: --fir %s, line %d: not an integer tap in -32768..32767 (Q14: 16384 = 1.0).\n", fir_arg, lineno);
                exit(1);
            }
            if (n_fir == fir_max) {
                fprintf(stderr, "ERROR: --fir %s holds more than %d taps.\n", fir_arg, fir_max);
                exit(1);
            }
            fir_taps[n_fir++] = (int16_t)v;
        }
        fclose(fp);
        if (n_fir == 0) {
            fprintf(stderr, "ERROR: --fir %s holds no tap.\n", fir_arg);
            exit(1);
        }
        if ((dec_on ? gal_synth_firdec_check(fir_taps, n_fir, osr) : gal_synth_fir_check(fir_taps, n_fir)) != GAL_OK) {
            fprintf(stderr, "ERROR: --fir %s: %s\n", fir_arg, gal_synth_last_error());
            exit(1);
        }
    }
    if (fir_lowpass_arg) {
        char *end = nullptr;
        const double fc = strtod(fir_lowpass_arg, &end);
        long nt = 63;
        bool ok = *fir_lowpass_arg && end != fir_lowpass_arg;
        if (ok && *end == ',') {
            const char *b = end + 1;
            nt = strtol(b, &end, 10);
            ok = *b && end != b && nt >= 0 && nt <= 1000;
        }
        if (!ok || *end) {
            fprintf(stderr, "ERROR: --fir-lowpass '%s' is not cutoff_hz[,n_taps].\n", fir_lowpass_arg);
            exit(1);
        }
        if ((dec_on ? gal_synth_firdec_lowpass(fc, kSampleRate, (int32_t)nt, fir_taps) : gal_synth_fir_lowpass(fc, kSampleRate, (int32_t)nt, fir_taps)) != GAL_OK) {
            fprintf(stderr, "ERROR: --fir-lowpass %s: %s\n", fir_lowpass_arg, gal_synth_last_error());
            exit(1);
        }
        n_fir = (int)nt;
        if (!sitesfile[0]) {
            fprintf(stderr, "Front-end filter: low-pass, cutoff %g Hz, %d taps (Q14):", fc, n_fir);
            for (int k = 0; k < n_fir; ++k) fprintf(stderr, " %d", fir_taps[k]);
            fprintf(stderr, "\n");
        }
    }
    if (dec_on && n_fir == 0) {  // the default decimator: 0.45 x the output rate, a delay of 16 output samples
        const double fc = 0.45 * kOutRate;
        n_fir = 32 * osr + 1;
        if (gal_synth_firdec_lowpass(fc, kSampleRate, n_fir, fir_taps) != GAL_OK) {
            fprintf(stderr, "ERROR: --oversample %d: %s\n", osr, gal_synth_last_error());
            exit(1);
        }
        if (!sitesfile[0]) {
            fprintf(stderr, "Front-end filter: low-pass, cutoff %g Hz, %d taps (Q14):", fc, n_fir);
            for (int k = 0; k < n_fir; ++k) fprintf(stderr, " %d", fir_taps[k]);
            fprintf(stderr, "\n");
        }
    }
    const bool fir_on = n_fir > 0;
    // the delay of a symmetric filter, in OUTPUT samples: what --monitor follows
    int fir_delay = fir_on ? (n_fir - 1) / 2 : 0;
    if (dec_on) {
        if (monitor_arg && (n_fir - 1) % (2 * osr) != 0) {
            fprintf(stderr, "ERROR: --monitor with --oversample %d needs taps whose (n_taps - 1) is a multiple of %d: %d taps delay the stream by %g output samples, "
                            "and the monitor follows whole samples only.\n", osr, 2 * osr, n_fir, (n_fir - 1) / (2.0 * osr));
            exit(1);
        }
        fir_delay = (n_fir - 1) / (2 * osr);
        if (iq_format == GAL_IQ_IBYTE && !iq_shift_arg && noise_on) {
            // the smallest shift with 127 x 2^s >= 4 sigma' + the --jam amplitudes, sigma' = sigma sqrt(sum h^2) / 16384 behind the filter
            double e2 = 0.0;
            for (int k = 0; k < n_fir; ++k) e2 += (double)fir_taps[k] * (double)fir_taps[k];
            const double sigma_out = noise.sigma_q4 / 16.0 * sqrt(e2) / 16384.0;
            iq_shift = 0;
            while (iq_shift < 15 && 127.0 * (double)(1 << iq_shift) < 4.0 * sigma_out + (agc_on ? 0.0 : jam_unit * gain)) ++iq_shift;
            if (!sitesfile[0]) fprintf(stderr, "Decimator: sigma %.1f LSB behind the filter, --iq-shift %d (chosen)\n", sigma_out, iq_shift);
        }
        if (!sitesfile[0])
            fprintf(stderr, "Oversampling: %d x 2.6 MS/s = %g MS/s in front of the decimator, %d taps, delay %g output samples\n", osr, kSampleRate / 1e6,
                    n_fir, (n_fir - 1) / (2.0 * osr));
    }
    // AGC: the parameters, now that shift and sigma are known
    gal_iq_agc_t agc;
    memset(&agc, 0, sizeof(agc));
    const int agc_param = iq_format == GAL_IQ_IBYTE ? iq_shift : iq_format == GAL_IQ_I2BIT ? i2bit_thr : 0;
    FILE *agc_log_fp = nullptr;
    if (agc_on) {
        if (agc_target == 0.0) agc_target = iq_format == GAL_IQ_IBYTE ? 32.0 * (double)(1 << iq_shift) : iq_format == GAL_IQ_I2BIT ? (double)i2bit_thr : 2048.0;
        if (agc_init < 0.0) {  // the noise sigma where the AGC sits: behind --fir or the decimator where there is one
            agc_init = 750.0;  // (the sigma of 9-12 channels)
            if (noise_on) {
                agc_init = noise.sigma_q4 / 16.0;
                if (fir_on) {
                    double e2 = 0.0;
                    for (int k = 0; k < n_fir; ++k) e2 += (double)fir_taps[k] * (double)fir_taps[k];
                    agc_init *= sqrt(e2) / 16384.0;
                }
            }
        }
        if (gal_synth_agc_from_rms(agc_target, agc_init, (int32_t)agc_block, (int32_t)agc_window, &agc) != GAL_OK) {
            fprintf(stderr, "ERROR: --agc: %s\n", gal_synth_last_error());
            exit(1);
        }
        if (!sitesfile[0]) {
            fprintf(stderr, "AGC: target rms %g LSB, blocks of %ld samples, window %ld blocks, initial rms %g LSB", agc_target, agc_block, agc_window, agc_init);
            if (iq_format == GAL_IQ_IBYTE) fprintf(stderr, ", --iq-shift %d%s", iq_shift, iq_shift_arg ? "" : " (chosen)");
            if (iq_format == GAL_IQ_I2BIT) fprintf(stderr, ", --i2bit-threshold %d", i2bit_thr);
            fprintf(stderr, "\n");
            if (agc_log_arg) {
                agc_log_fp = fopen(agc_log_arg, "w");
                if (!agc_log_fp) {
                    fprintf(stderr, "ERROR: cannot write the AGC log %s.\n", agc_log_arg);
                    exit(1);
                }
                fprintf(agc_log_fp, "time_s,gain_q12,gain_db\n");
            }
        }
    }
    // receiver oscillator: checked here too, before any device work.  Without --lo-offset / --phase-noise nothing below differs from a
    // build without them.
    gal_iq_osc_t osc;
    memset(&osc, 0, sizeof(osc));
    const bool osc_on = lo_offset_arg || phase_noise_arg;
    if (!osc_on && (osc_seed_arg || osc_stream_arg)) {
        fprintf(stderr, "ERROR: --osc-seed and --osc-stream need --lo-offset or --phase-noise.\n");
        exit(1);
    }
    if (osc_on) {
        double lo_hz = 0.0, lo_drift = 0.0, lo_h0 = 0.0;
        if (lo_offset_arg) {
            char *end = nullptr;
            lo_hz = strtod(lo_offset_arg, &end);
            bool ok = *lo_offset_arg && end != lo_offset_arg;
            if (ok && *end == ',') {
                const char *d = end + 1;
                lo_drift = strtod(d, &end);
                ok = *d && end != d;
            }
            if (!ok || *end) {
                fprintf(stderr, "ERROR: --lo-offset '%s' is not hz[,drift_hz_per_s].\n", lo_offset_arg);
                exit(1);
            }
        }
        if (phase_noise_arg) {
            char *end = nullptr;
            lo_h0 = strtod(phase_noise_arg, &end);
            if (!*phase_noise_arg || end == phase_noise_arg || *end) {
                fprintf(stderr, "ERROR: --phase-noise '%s' is not a number (h0 in seconds, e.g. 1e-21).\n", phase_noise_arg);
                exit(1);
            }
        }
        // the oscillator sits in front of the decimator: with --oversample M it runs at M x 2.6 MS/s
        if (gal_synth_osc_make(lo_hz, lo_drift, lo_h0, kSampleRate, 1575.42e6, &osc) != GAL_OK) {
            fprintf(stderr, "ERROR: --lo-offset / --phase-noise: %s\n", gal_synth_last_error());
            exit(1);
        }
        if (osc_seed_arg) {
            char *end = nullptr;
            errno = 0;
            osc.seed = strtoull(osc_seed_arg, &end, 0);
            if (!*osc_seed_arg || *end || errno || osc_seed_arg[0] == '-') {
                fprintf(stderr, "ERROR: --osc-seed '%s' is not an unsigned 64-bit integer.\n", osc_seed_arg);
                exit(1);
            }
        }
        if (osc_stream_arg) {
            char *end = nullptr;
            errno = 0;
            const unsigned long long v = strtoull(osc_stream_arg, &end, 0);
            if (!*osc_stream_arg || *end || errno || osc_stream_arg[0] == '-' || v > 0xffffffffull) {
                fprintf(stderr, "ERROR: --osc-stream '%s' is not an unsigned 32-bit integer.\n", osc_stream_arg);
                exit(1);
            }
            osc.stream = (uint32_t)v;
        }
        if (!sitesfile[0]) {
            const double two64 = 18446744073709551616.0, pi = 3.14159265358979323846;
            const double sig_cyc = 1575.42e6 * sqrt(lo_h0 / (2.0 * kSampleRate)), sig_rad = 2.0 * pi * sig_cyc;
            fprintf(stderr, "Oscillator: offset %.6f Hz, drift %.6g Hz/s (F = %lld, D = %lld at %g MS/s)", (double)osc.f / two64 * kSampleRate,
                    (double)osc.d / two64 * kSampleRate * kSampleRate, (long long)osc.f, (long long)osc.d, kSampleRate / 1e6);
            if (osc.s)
                fprintf(stderr, "; phase noise h0 %g s: sigma %.4g rad per sample (S = %llu), rms phase %.4g rad over 1 ms, %.4g rad over 4 ms, "
                                "Lorentzian linewidth %.4g Hz; seed %llu, stream %u",
                        lo_h0, sig_rad, (unsigned long long)osc.s, sig_rad * sqrt(kSampleRate * 1e-3), sig_rad * sqrt(kSampleRate * 4e-3),
                        sig_rad * sig_rad * kSampleRate / (2.0 * pi), (unsigned long long)osc.seed, osc.stream);
            fprintf(stderr, "\n");
        }
    }
    // bytes of n samples in the output format: the AGC has its own count (i2bit is a format of the AGC call only)
    const auto out_bytes = [&](size_t n) { return agc_on ? gal_synth_agc_out_bytes(iq_format, n) : gal_synth_iq_bytes(iq_format, n); };
    const double iq_bytes_per_sample = (double)out_bytes(4) / 4.0;
    if (sitesfile[0]) {
        // several listeners cannot share a port: the sites run without the position listener unless -P names a base port, in
        // which case site k (in file order) listens on port + k
        char self[4096];
        const ssize_t n = readlink("/proc/self/exe", self, sizeof(self) - 1);
        if (n <= 0) snprintf(self, sizeof(self), "%s", argv[0]);
        else self[n] = 0;
        return run_sites(self, child_args, sitesfile, outfile, sites_gpus, sites_per_gpu, udp_given ? sc.udp_port : 0,
                         kIqNames[iq_format], iq_bytes_per_sample, noise_on, osc_on, monitor_arg);
    }
    if (outfile[0] == 0) {
        printf("[+] File sink not specified. Using galileosim.%s\n", kIqNames[iq_format]);
        snprintf(outfile, sizeof(outfile), "galileosim.%s", kIqNames[iq_format]);
    }
    if (dec_on && !have_batch) batch_epochs = 128 / osr > 8 ? 128 / osr : 8;  // the device buffers keep their size
    if (realtime && !have_batch) batch_epochs = 1;  // paced output: position updates take effect within 0.1 s
    if (batch_epochs < 1) batch_epochs = 1;
    sc.nav_file = navfile;
    sc.motion_file = umfile[0] ? umfile : nullptr;
    sc.verbose = 1;

    gal_scen_t *scen = nullptr;
    int orc = gal_scen_open(&sc, &scen);
    if (orc == GAL_E_BUSY && sc.udp_port > 0 && !udp_given) {
        // the default port is taken (another instance): the reference would exit; carry on without the listener
        fprintf(stderr, "WARNING: %s; continuing without run-time position updates\n", gal_scen_last_error());
        sc.udp_port = 0;
        orc = gal_scen_open(&sc, &scen);
    }
    if (orc != GAL_OK) {
        fprintf(stderr, "%s\n", gal_scen_last_error());
        if (orc == GAL_E_EMPTY && strcmp(outfile, "-") != 0) {
            // (int)(10 d + 0.5) < 2: the reference opens its sink, finds no epoch to generate and closes it (src/galileo-sdr.cpp:438)
            FILE *f = fopen(outfile, "wb");
            if (f) fclose(f);
            exit(0);
        }
        exit(1);
    }
    if (power_on && (gal_scen_set_power(scen, antenna_arg ? ant_db : nullptr, prn_db) != GAL_OK ||
                     gal_scen_set_path_loss(scen, power_model ? 1 : 0) != GAL_OK)) {
        fprintf(stderr, "ERROR: %s\n", gal_scen_last_error());
        exit(1);
    }
    stage("scenario opened (RINEX)");
    const int total = gal_scen_total_epochs(scen);
    int32_t wk;
    double ws;
    gal_scen_start_time(scen, &wk, &ws);
    fprintf(stderr, "\n%s\nStart = %d:%.0f  Duration = %.1f [sec]  (%d epochs of 0.1 s)\n",
            sc.motion_file ? "Using user motion file." : "Using static location mode.", wk, ws, (total + 1) / 10.0, total);

    gal_synth_cfg_t cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.sample_rate = kSampleRate;
    cfg.samples_per_epoch = osr * kOutSamplesPerEpoch;
    cfg.n_slots = sc.n_slots;
    cfg.device = getenv("GAL_DEVICE") ? atoi(getenv("GAL_DEVICE")) : -1;
    if (cboc) cfg.flags |= GAL_CFG_CBOC;
    if (exact_replay) cfg.flags |= GAL_CFG_EXACT_REPLAY;
    // bytes per epoch in the output format: the per-batch split of the copies cuts at epoch boundaries, so every piece must be whole
    // bytes -- for ibit 260 000 % 4 == 0
    const size_t epoch_bytes = out_bytes((size_t)kOutSamplesPerEpoch);  // (i2bit: 260 000 % 2 == 0)
    if (iq_format == GAL_IQ_IBIT && kOutSamplesPerEpoch % 4 != 0) {
        fprintf(stderr, "ERROR: ibit needs a multiple of 4 samples per epoch.\n");
        exit(1);
    }

    if (n_writers < 0) {
        // Default: the sequential sink.  Measured on the MI355X host (256 cores, tmpfs, 1.25 GB): write() stream 0.20 s;
        // mapped sink with 4 / 8 / 16 copy threads 0.24 / 0.22 / 0.24 s INCLUDING the unmap (0.10-0.21 s without it, which is
        // what round 3's first measurements showed): the kernel inserts pages into ONE file's page cache at ~6 GB/s whoever
        // asks -- write(), page faults of many threads, pwrite()s of many threads (inode lock) -- profiles/archive/r03a_sink_probe.log.
        n_writers = 0;
    }
    Sink sink;
    if (!sink.open(outfile, realtime ? 0 : (size_t)total * epoch_bytes, n_writers)) {  // (paced runs stream: they are slow by design)
        fprintf(stderr, "ERROR: Failed to open output file.\n");
        exit(1);
    }

    stage("sink opened");
    // (Engine creation and buffer allocation one after the other: running them in two threads was measured -- 6 alternations
    // on one box, 157-318 ms against 250-328 ms for this stage, no difference beyond the run-to-run spread of the HIP
    // start-up itself; the runtime serialises code-object loading and page pinning.)
    gal_synth_t *eng = nullptr;
    if (gal_synth_create(&cfg, &eng) != GAL_OK) {
        fprintf(stderr, "ERROR: %s\n", gal_synth_last_error());
        exit(1);
    }
    stage("gal_synth_create");
    if (fir_on && (dec_on ? gal_synth_firdec_set(eng, fir_taps, n_fir, osr, 0) : gal_synth_fir_set(eng, fir_taps, n_fir)) != GAL_OK) {
        fprintf(stderr, "ERROR: %s\n", gal_synth_last_error());
        exit(1);
    }
    if (agc_on && gal_synth_agc_set(eng, &agc, 0) != GAL_OK) {
        fprintf(stderr, "ERROR: %s\n", gal_synth_last_error());
        exit(1);
    }
    if (osc_on && gal_synth_osc_set(eng, &osc, 0) != GAL_OK) {
        fprintf(stderr, "ERROR: %s\n", gal_synth_last_error());
        exit(1);
    }
    if (batch_epochs > total) batch_epochs = total > 0 ? total : 1;
    const size_t batch_bytes = epoch_bytes * batch_epochs;  // in the output format
    // d_iq: the engine's int16 output; d_out: what the copies read -- d_iq itself for ishort (with --cn0: after the noise pass has
    // run in place), the converted batch otherwise
    // --fir: d_fir holds the filtered int16 batch, which then is what the format conversion (ishort: the copies) reads
    // --agc: the AGC writes every format, ishort too, into d_out (it does not run in place)
    int16_t *d_iq[2] = {nullptr, nullptr};
    int16_t *d_fir[2] = {nullptr, nullptr};
    void *d_out[2] = {nullptr, nullptr};
    hipEvent_t converted[2] = {nullptr, nullptr};
    Slot slot[2];
    for (int i = 0; i < 2; ++i) {
        if (hipMalloc((void **)&d_iq[i], (size_t)cfg.samples_per_epoch * 4 * batch_epochs) != hipSuccess ||
            hipHostMalloc((void **)&slot[i].host, batch_bytes, hipHostMallocDefault) != hipSuccess) {
            fprintf(stderr, "ERROR: buffer allocation failed\n");
            exit(1);
        }
        d_out[i] = d_iq[i];
        if (fir_on) {
            if (hipMalloc((void **)&d_fir[i], (size_t)kOutSamplesPerEpoch * 4 * batch_epochs) != hipSuccess) {
                fprintf(stderr, "ERROR: buffer allocation failed\n");
                exit(1);
            }
            d_out[i] = d_fir[i];
        }
        if ((iq_format != GAL_IQ_ISHORT || agc_on) && hipMalloc(&d_out[i], batch_bytes) != hipSuccess) {
            fprintf(stderr, "ERROR: buffer allocation failed\n");
            exit(1);
        }
        if ((iq_format != GAL_IQ_ISHORT || mix_on || power_on || mp_on || fir_on || agc_on || osc_on) && hipEventCreateWithFlags(&converted[i], hipEventDisableTiming) != hipSuccess) {
            fprintf(stderr, "ERROR: buffer allocation failed\n");
            exit(1);
        }
        hipEventCreate(&slot[i].copied[0]);
        hipEventCreate(&slot[i].copied[1]);
    }
    // --monitor: per batch slot the sums of its monitored epochs, on the device and pinned on the host
    MonBatch mon[2];
    MonSummary mon_sum[GAL_NUM_PRN + 1];
    gal_corr_req_t mon_shape;  // what every monitor request shares
    memset(&mon_shape, 0, sizeof(mon_shape));
    mon_shape.max_periods = kMonPeriods;
    mon_shape.delay_step = 1;
    mon_shape.dopp_step = (int32_t)llround(kMonBinHz / kOutRate * 4294967296.0);
    mon_shape.dopp0 = -mon_shape.dopp_step;
    mon_shape.n_dopp = 3;
    // gal_corr_cn0 reads the period length off the shape: the nominal code step (a request's own differs by its code Doppler, a few
    // 1e-6: 1e-5 dB).  Left at 0 it made every C/N0 of the CSV "nan"
    mon_shape.code_dph = (uint64_t)llround(2.0 * 1.023e6 / kOutRate * 4294967296.0);
    const size_t mon_epochs_max = (size_t)(batch_epochs + monitor_every - 1) / monitor_every + 1;
    const size_t mon_bytes = mon_epochs_max * sc.n_slots * (kMonNear + kMonFar) * sizeof(long long);
    if (monitor_fp)
        for (int i = 0; i < 2; ++i)
            if (hipMalloc((void **)&mon[i].dev, mon_bytes) != hipSuccess ||
                hipHostMalloc((void **)&mon[i].host, mon_bytes, hipHostMallocDefault) != hipSuccess) {
                fprintf(stderr, "ERROR: buffer allocation failed\n");
                exit(1);
            }
    // --agc-log: per batch slot the gains of the blocks that start in it, on the device and pinned on the host
    struct AgcLog {
        uint32_t *dev = nullptr, *host = nullptr;
        size_t n = 0;
        bool pending = false;
    } agc_log[2];
    uint64_t agc_logged = 0;  // blocks written to the log
    if (agc_log_fp) {
        const size_t g_bytes = ((size_t)batch_epochs * kOutSamplesPerEpoch / (size_t)agc_block + 2) * sizeof(uint32_t);
        for (int i = 0; i < 2; ++i)
            if (hipMalloc((void **)&agc_log[i].dev, g_bytes) != hipSuccess || hipHostMalloc((void **)&agc_log[i].host, g_bytes, hipHostMallocDefault) != hipSuccess) {
                fprintf(stderr, "ERROR: buffer allocation failed\n");
                exit(1);
            }
    }
    // the lines of a batch whose gains have arrived (the stream has been waited for)
    const auto agc_log_flush = [&](AgcLog &l) {
        for (size_t k = 0; k < l.n; ++k, ++agc_logged)
            fprintf(agc_log_fp, "%.9f,%u,%.4f\n", (double)agc_logged * (double)agc_block / kOutRate, l.host[k], 20.0 * log10((double)l.host[k] / 4096.0));
        l.pending = false;
    };
    stage("device + pinned buffers");
    // (a stream for the engine, made here: left to the engine it would be made inside the first gal_synth_plan -- 7-17 ms
    // of the run instead of the start-up)
    hipStream_t stream;
    hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
    gal_synth_set_stream(eng, stream);
    // device -> host on two streams of their own: two DMA engines share the link, and the copy of batch k runs
    // beside the front-end and the synthesis of batch k+1
    hipStream_t copy_stream[2];
    hipStreamCreateWithFlags(&copy_stream[0], hipStreamNonBlocking);
    hipStreamCreateWithFlags(&copy_stream[1], hipStreamNonBlocking);
    // First use of the copy path belongs to the start-up, not to the run: the first device -> host copy of a process
    // took 8 ms on its own (profiles/archive/r03p_cli_batches.log: batch 2 started 10.4 ms into a run whose batches take 2.35 ms)
    if (!getenv("GAL_CLI_COLD_COPY")) {
        for (int i = 0; i < 2; ++i)
            for (int k = 0; k < 2; ++k) {
                const size_t off = k ? batch_bytes / 2 : 0, nb = batch_bytes / 2 < ((size_t)1 << 20) ? batch_bytes / 2 : ((size_t)1 << 20);
                if (nb) hipMemcpyAsync((char *)slot[i].host + off, (const char *)d_out[i] + off, nb, hipMemcpyDeviceToHost, copy_stream[k]);
            }
        hipStreamSynchronize(copy_stream[0]);
        hipStreamSynchronize(copy_stream[1]);
    }
    stage("copy path warmed");

    // writer thread: drains full slots in order
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    std::atomic<bool> io_error{false};  // written by the writer thread, read by the producer loop
    int next_write = 0;
    std::thread writer([&]() {
        for (;;) {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return slot[next_write].full || done; });
            if (!slot[next_write].full) return;
            Slot &s = slot[next_write];
            lk.unlock();
            if (hipEventSynchronize(s.copied[0]) != hipSuccess || hipEventSynchronize(s.copied[1]) != hipSuccess ||
                !sink.put((const char *)s.host, s.bytes))
                io_error = true;
            lk.lock();
            s.full = false;
            next_write ^= 1;
            lk.unlock();
            cv.notify_all();
        }
    });

    signal(SIGINT, on_sigint);
    const auto t_start = std::chrono::steady_clock::now();
    // producer: front-end rows, kRowBufs batches deep
    constexpr int kRowBufs = 3;
    struct RowBuf {
        std::vector<gal_chan_epoch_t> rows;
        std::vector<uint16_t> gains;  // per-satellite signal power: [epochs][slots] Q7
        int n = 0;  // epochs in it; < 0: front-end error, 0 with `last`: end of the scenario
        bool ready = false;
    };
    RowBuf rb[kRowBufs];
    for (auto &b : rb) {
        b.rows.resize((size_t)batch_epochs * sc.n_slots);
        if (power_on) b.gains.resize((size_t)batch_epochs * sc.n_slots);
    }
    std::mutex rmu;
    std::condition_variable rcv;
    bool consumer_gone = false;
    std::string scen_error;
    long produced_epochs = 0;
    std::thread producer([&]() {
        int w = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(rmu);
                rcv.wait(lk, [&] { return !rb[w].ready || consumer_gone; });
                if (consumer_gone) return;
            }
            if (realtime) {  // FIFO-style pacing (the reference: src/fifo.cpp + src/galileo-sdr.cpp:570-595): epoch k is
                             // produced no earlier than k * 0.1 s after the start, so that position updates are current
                std::this_thread::sleep_until(t_start + std::chrono::milliseconds(100) * produced_epochs);
            }
            const int n = g_stop      ? 0
                          : power_on ? gal_scen_next_gains(scen, batch_epochs, rb[w].rows.data(), rb[w].gains.data())
                                     : gal_scen_next(scen, batch_epochs, rb[w].rows.data());
            if (n > 0) produced_epochs += n;
            {
                std::lock_guard<std::mutex> lk(rmu);
                if (n < 0) scen_error = gal_scen_last_error();
                rb[w].n = n;
                rb[w].ready = true;
            }
            rcv.notify_all();
            if (n <= 0) return;
            w = (w + 1) % kRowBufs;
        }
    });
    std::vector<gal_chan_state_t> state(sc.n_slots);
    memset(state.data(), 0, sizeof(gal_chan_state_t) * sc.n_slots);
    bool have_state = false;
    int emitted = 0, cur = 0, rc = 0, r = 0;
    int prn_gain_lo[GAL_NUM_PRN + 1], prn_gain_hi[GAL_NUM_PRN + 1];  // per-satellite signal power: the gains each PRN was given
    std::vector<uint16_t> mp_gains;     // --multipath: the batch's gains [epochs][slots] ...
    std::vector<gal_iq_echo_t> mp_rows; // ... its echo table [epochs][echoes in view] ...
    std::vector<int32_t> slot_of;       // ... and per echo in view its slot and its line of the file
    std::vector<const EchoSpec *> spec_of;
    const auto note_gains = [&](const gal_chan_epoch_t *rows, const uint16_t *g, size_t count) {  // the summary's per-PRN range
        for (size_t i = 0; i < count; ++i) {
            const int prn = rows[i].prn;
            if (prn < 1 || prn > GAL_NUM_PRN) continue;
            prn_gain_lo[prn] = g[i] < prn_gain_lo[prn] ? g[i] : prn_gain_lo[prn];
            prn_gain_hi[prn] = g[i] > prn_gain_hi[prn] ? g[i] : prn_gain_hi[prn];
        }
    };
    for (int i = 0; i <= GAL_NUM_PRN; ++i) prn_gain_lo[i] = GAL_GAIN_MAX + 1, prn_gain_hi[i] = -1;
    // (SIGINT: the batch in flight is finished and written, batches the producer has queued behind it are dropped)
    const bool batch_timing = getenv("GAL_CLI_TIMING") != nullptr;
    auto ms_since = [&](std::chrono::steady_clock::time_point a) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
    };
    while (emitted < total && !io_error && !g_stop) {
        const auto tb0 = std::chrono::steady_clock::now();
        {
            std::unique_lock<std::mutex> lk(rmu);
            rcv.wait(lk, [&] { return rb[r].ready; });
        }
        const double tb_rows = ms_since(tb0);
        const int n = rb[r].n;
        const gal_chan_epoch_t *rows_ptr = rb[r].rows.data();
        if (n < 0) {
            fprintf(stderr, "\nERROR: %s\n", scen_error.c_str());
            rc = 1;
            break;
        }
        if (n == 0) break;
        {  // wait until the slot we are about to fill has been written out
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !slot[cur].full; });
        }
        const double tb_slot = ms_since(tb0);
        // --monitor: the requests of this batch's monitored epochs, made while the rows are still ours
        std::vector<gal_corr_req_t> mon_reqs;
        std::vector<int> mon_epoch;  // per pair of requests: the epoch's position in the batch
        std::vector<int> mon_skip;   // ... and the samples skipped at its start (ibit: so that the address is 16-byte aligned)
        if (monitor_fp) {
            if (mon[cur].pending) {  // (cannot happen: flushed behind the finish of the batch after it)
                fprintf(stderr, "\nERROR: monitor buffer still in use\n");
                rc = 1;
                break;
            }
            for (int e = 0; e < n; ++e) {
                if ((emitted + e) % monitor_every) continue;
                const size_t ob = out_bytes((size_t)e * kOutSamplesPerEpoch);
                int skip = iq_format == GAL_IQ_IBIT ? (int)((16 - ob % 16) % 16) * 4 : 0;
                if (fir_on && skip < fir_delay) {  // the filtered stream lags by fir_delay: start there or later, on the same 16-byte grid
                    const int g = iq_format == GAL_IQ_IBIT ? 64 : iq_format == GAL_IQ_IBYTE ? 8 : 4;  // samples per 16 bytes
                    skip += (fir_delay - skip + g - 1) / g * g;
                }
                for (int s = 0; s < sc.n_slots; ++s) {
                    const gal_chan_epoch_t &rec = rows_ptr[(size_t)e * sc.n_slots + s];
                    if (rec.prn <= 0) continue;
                    gal_corr_req_t q = mon_shape;
                    if (gal_corr_from_epoch(&rec, kOutRate, skip - fir_delay, &q) != GAL_OK) continue;  // (a record the monitor cannot follow)
                    if (osc_on) {
                        // the replica follows the oscillator's offset and drift: its step at the window's first sample -- counted at the
                        // rate the oscillator runs at, and where the filters' delay puts that sample -- times the M samples of that rate
                        // in one of the output (the drift inside the window of 0.1 s is not followed: 0.2 Hz at 2 Hz/s)
                        const int64_t off = ((int64_t)skip - fir_delay) * osr;
                        const uint64_t n_lo = (uint64_t)(emitted + e) * (uint64_t)cfg.samples_per_epoch + (uint64_t)(off > 0 ? off : 0);
                        int32_t lo_step = 0;
                        gal_synth_osc_lo_step(&osc, n_lo, &lo_step);
                        q.carr_dph = (int32_t)((uint32_t)q.carr_dph + (uint32_t)osr * (uint32_t)lo_step);
                    }
                    MonEntry me;
                    me.t = (emitted + e) * 0.1;
                    me.f_carr = rec.f_carr;
                    me.prn = rec.prn;
                    me.off = mon[cur].entries.size() * (kMonNear + kMonFar);
                    mon[cur].entries.push_back(me);
                    q.delay0 = -1;
                    q.n_delay = 3;
                    mon_reqs.push_back(q);
                    q.delay0 = kMonFarDelay;
                    q.n_delay = 1;
                    mon_reqs.push_back(q);
                    mon_epoch.push_back(e);
                    mon_skip.push_back(skip);
                }
            }
        }
        if (power_on && !mp_on) {
            // one synthesis run per group of slots with equal gains, finished when the call returns, and the weighted sum enqueued
            // on the engine's stream behind them (include/galsynth.h)
            const uint16_t *gp = rb[r].gains.data();
            note_gains(rows_ptr, gp, (size_t)n * sc.n_slots);
            if (gal_synth_run_gains(eng, rows_ptr, n, have_state ? state.data() : nullptr, gp, d_iq[cur], state.data()) != GAL_OK) {
                fprintf(stderr, "\nERROR: %s\n", gal_synth_last_error());
                rc = 1;
                break;
            }
        } else if (mp_on) {
            // the gains of --power-model and its kin, or unity; an echo goes to the slot that carries its PRN in this batch (a PRN that
            // is not in view: no echo), with a row per epoch from the slot's gain and the epoch's index in the whole stream
            const int S = sc.n_slots;
            if (power_on) {
                mp_gains.assign(rb[r].gains.begin(), rb[r].gains.begin() + (size_t)n * S);
                note_gains(rows_ptr, mp_gains.data(), (size_t)n * S);
            } else {
                mp_gains.assign((size_t)n * S, (uint16_t)GAL_GAIN_UNITY);
            }
            slot_of.clear();
            spec_of.clear();
            for (const EchoSpec &e : echoes) {
                int slot = -1;
                for (size_t i = 0; i < (size_t)n * S && slot < 0; ++i)
                    if (rows_ptr[i].prn == e.prn) slot = (int)(i % S);
                if (slot < 0) continue;
                slot_of.push_back(slot);
                spec_of.push_back(&e);
            }
            const int n_echo = (int)slot_of.size();
            mp_rows.assign((size_t)n * (n_echo > 0 ? n_echo : 1), gal_iq_echo_t{});
            bool ok = true;
            for (int e = 0; e < n && ok; ++e)
                for (int k = 0; k < n_echo && ok; ++k) {
                    const size_t i = (size_t)e * S + slot_of[k];
                    const bool here = rows_ptr[i].prn == spec_of[k]->prn;  // (the slot carries another satellite, or none, in this epoch: A = 0)
                    ok = gal_synth_mpath_row(&spec_of[k]->echo, here ? mp_gains[i] : 0, (uint64_t)(emitted + e), cfg.samples_per_epoch,
                                             &mp_rows[(size_t)e * n_echo + k]) == GAL_OK;
                }
            if (!ok || gal_synth_run_mpath(eng, rows_ptr, n, have_state ? state.data() : nullptr, mp_gains.data(), slot_of.data(), mp_rows.data(),
                                           n_echo, d_iq[cur], state.data()) != GAL_OK) {
                fprintf(stderr, "\nERROR: %s\n", gal_synth_last_error());
                rc = 1;
                break;
            }
        } else if (gal_synth_plan(eng, rows_ptr, n, have_state ? state.data() : nullptr) != GAL_OK ||
                   gal_synth_execute(eng, d_iq[cur]) != GAL_OK) {
            fprintf(stderr, "\nERROR: %s\n", gal_synth_last_error());
            rc = 1;
            break;
        }
        {  // plan() has uploaded the rows: the producer may refill this buffer
            std::lock_guard<std::mutex> lk(rmu);
            rb[r].ready = false;
        }
        rcv.notify_all();
        r = (r + 1) % kRowBufs;
        // The IQ in d_iq[cur] is final only once gal_synth_finish() has returned: finish() may find the speculative
        // carrier chain unverified (or the replay check unhappy) and synthesise the batch again.  The copies are
        // therefore enqueued after it; they still run beside the front-end and the synthesis of the next batch.
        if (!power_on && !mp_on && gal_synth_finish(eng, state.data(), nullptr) != GAL_OK) {
            fprintf(stderr, "\nERROR: %s\n", gal_synth_last_error());
            rc = 1;
            break;
        }
        // (the stream has drained up to this batch's synthesis: the sums of the batch before it are on the host)
        if (monitor_fp && mon[cur ^ 1].pending) monitor_flush(mon[cur ^ 1], monitor_fp, kOutRate, mon_shape, mon_sum);
        if (agc_log_fp && agc_log[cur ^ 1].pending) agc_log_flush(agc_log[cur ^ 1]);
        const double tb_synth = ms_since(tb0);
        if (batch_timing)
            fprintf(stderr, "[timing] batch at %7.2f ms: %3d epochs, waited %.2f ms for rows, %.2f for a free slot, %s %.2f\n",
                    std::chrono::duration<double, std::milli>(tb0 - t_start).count(), n, tb_rows, tb_slot - tb_rows,
                    mp_on      ? "run_mpath (every group's plan + execute + finish, the echo pass enqueued)"
                    : power_on ? "run_gains (every group's plan + execute + finish, the sum enqueued)"
                               : "plan + execute + finish",
                    tb_synth - tb_slot);
        slot[cur].bytes = epoch_bytes * n;
        if (fir_on) {
            // noise / interference into the int16 batch in place, the filter into d_fir[cur], the plain format conversion from there
            // (ishort: the copies read d_fir[cur] itself); the filter's history runs on from batch to batch inside the handle
            // --oversample: the batch is n x M x 260 000 samples up to the decimator, which keeps n x 260 000 of them
            const size_t n_samples = (size_t)n * cfg.samples_per_epoch, n_kept = (size_t)n * kOutSamplesPerEpoch;
            int crc = GAL_OK;
            if (mix_on)
                crc = gal_synth_iq_convert_interf(eng, d_iq[cur], n_samples, (uint64_t)emitted * (uint64_t)cfg.samples_per_epoch, &noise, interf, n_jam,
                                                  GAL_IQ_ISHORT, 0, d_iq[cur]);
            if (crc == GAL_OK && osc_on) crc = gal_synth_iq_osc(eng, d_iq[cur], n_samples, d_iq[cur]);  // the mixer: in front of the filter, in place
            if (crc == GAL_OK && dec_on) {
                size_t got = 0;
                crc = gal_synth_iq_firdec(eng, d_iq[cur], n_samples, d_fir[cur], &got);
                if (crc == GAL_OK && got != n_kept) {
                    fprintf(stderr, "\nERROR: the decimator kept %zu samples of the batch, not %zu\n", got, n_kept);
                    rc = 1;
                    break;
                }
            } else if (crc == GAL_OK) {
                crc = gal_synth_iq_fir(eng, d_iq[cur], n_samples, d_fir[cur]);
            }
            if (crc == GAL_OK && agc_on) crc = gal_synth_iq_agc(eng, d_fir[cur], n_kept, iq_format, agc_param, d_out[cur], agc_log[cur].dev, &agc_log[cur].n);
            else if (crc == GAL_OK && iq_format != GAL_IQ_ISHORT) crc = gal_synth_iq_convert(eng, d_fir[cur], n_kept, iq_format, iq_shift, d_out[cur]);
            if (crc != GAL_OK) {
                fprintf(stderr, "\nERROR: %s\n", gal_synth_last_error());
                rc = 1;
                break;
            }
        } else if (agc_on) {
            // noise / interference into the int16 batch in place, then the AGC and the format from there into d_out[cur]; the AGC's
            // state runs on from batch to batch inside the handle
            const size_t n_samples = (size_t)n * cfg.samples_per_epoch;
            int crc = GAL_OK;
            if (mix_on)
                crc = gal_synth_iq_convert_interf(eng, d_iq[cur], n_samples, (uint64_t)emitted * (uint64_t)cfg.samples_per_epoch, &noise, interf, n_jam,
                                                  GAL_IQ_ISHORT, 0, d_iq[cur]);
            if (crc == GAL_OK && osc_on) crc = gal_synth_iq_osc(eng, d_iq[cur], n_samples, d_iq[cur]);
            if (crc == GAL_OK) crc = gal_synth_iq_agc(eng, d_iq[cur], n_samples, iq_format, agc_param, d_out[cur], agc_log[cur].dev, &agc_log[cur].n);
            if (crc != GAL_OK) {
                fprintf(stderr, "\nERROR: %s\n", gal_synth_last_error());
                rc = 1;
                break;
            }
        } else if (osc_on) {
            // the oscillator needs the int16 stream between the noise pass and the format: noise / interference into the int16 batch in
            // place (as with --fir), the oscillator in place behind it, the plain format conversion from there (ishort: the copies read
            // d_iq[cur] itself); its phase runs on from batch to batch inside the handle
            const size_t n_samples = (size_t)n * cfg.samples_per_epoch;
            int crc = GAL_OK;
            if (mix_on)
                crc = gal_synth_iq_convert_interf(eng, d_iq[cur], n_samples, (uint64_t)emitted * (uint64_t)cfg.samples_per_epoch, &noise, interf, n_jam,
                                                  GAL_IQ_ISHORT, 0, d_iq[cur]);
            if (crc == GAL_OK) crc = gal_synth_iq_osc(eng, d_iq[cur], n_samples, d_iq[cur]);
            if (crc == GAL_OK && iq_format != GAL_IQ_ISHORT) crc = gal_synth_iq_convert(eng, d_iq[cur], n_samples, iq_format, iq_shift, d_out[cur]);
            if (crc != GAL_OK) {
                fprintf(stderr, "\nERROR: %s\n", gal_synth_last_error());
                rc = 1;
                break;
            }
        } else if (iq_format != GAL_IQ_ISHORT || mix_on) {
            // the conversion of the final int16 batch, on the engine's stream; both copy streams wait for it.  With --cn0 the noise
            // goes in in the same pass (ishort: in place in d_iq[cur]); first_sample is the running sample count, so the file does
            // not depend on the batch length
            const size_t n_samples = (size_t)n * cfg.samples_per_epoch;
            // (without --cn0, `noise` still carries the signal gain of the --jam sources; with neither the library converts plainly)
            const int crc = gal_synth_iq_convert_interf(eng, d_iq[cur], n_samples, (uint64_t)emitted * (uint64_t)cfg.samples_per_epoch,
                                                        mix_on ? &noise : NULL, interf, n_jam, iq_format, iq_shift, d_out[cur]);
            if (crc != GAL_OK) {
                fprintf(stderr, "\nERROR: %s\n", gal_synth_last_error());
                rc = 1;
                break;
            }
        }
        if (agc_log_fp) {  // behind the AGC, on the same stream
            if (agc_log[cur].n && hipMemcpyAsync(agc_log[cur].host, agc_log[cur].dev, agc_log[cur].n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream) != hipSuccess) {
                fprintf(stderr, "\nERROR: AGC log: copy of the gains failed\n");
                rc = 1;
                break;
            }
            agc_log[cur].pending = true;
        }
        if (iq_format != GAL_IQ_ISHORT || mix_on || power_on || mp_on || fir_on || agc_on || osc_on) {  // what the copies read is enqueued on the engine's stream: they wait for it
            if (hipEventRecord(converted[cur], stream) != hipSuccess || hipStreamWaitEvent(copy_stream[0], converted[cur], 0) != hipSuccess ||
                hipStreamWaitEvent(copy_stream[1], converted[cur], 0) != hipSuccess) {
                fprintf(stderr, "\nERROR: event after the IQ conversion failed\n");
                rc = 1;
                break;
            }
        }
        if (monitor_fp && !mon_reqs.empty()) {
            // behind the conversion, on the same stream, in the buffer the copies read: one call per monitored epoch
            bool mon_ok = true;
            size_t i = 0;
            while (i < mon_epoch.size() && mon_ok) {
                size_t j = i;
                while (j < mon_epoch.size() && mon_epoch[j] == mon_epoch[i]) ++j;
                const size_t ob = out_bytes((size_t)mon_epoch[i] * kOutSamplesPerEpoch) + out_bytes((size_t)mon_skip[i]);
                mon_ok = gal_synth_correlate(eng, (const char *)d_out[cur] + ob, iq_format, (size_t)kOutSamplesPerEpoch - mon_skip[i],
                                             &mon_reqs[2 * i], (int32_t)(2 * (j - i)), (int64_t *)(mon[cur].dev + mon[cur].entries[i].off)) == GAL_OK;
                i = j;
            }
            if (!mon_ok || hipMemcpyAsync(mon[cur].host, mon[cur].dev, mon[cur].entries.size() * (kMonNear + kMonFar) * sizeof(long long),
                                          hipMemcpyDeviceToHost, stream) != hipSuccess) {
                fprintf(stderr, "\nERROR: monitor: %s\n", mon_ok ? "copy of the sums failed" : gal_synth_last_error());
                rc = 1;
                break;
            }
            mon[cur].pending = true;
        }
        {
            // split at an epoch boundary: epoch_bytes is whole bytes in every format (see above)
            const size_t half = epoch_bytes * (size_t)((n + 1) / 2);
            const size_t part[2] = {half, slot[cur].bytes - half};
            size_t off = 0;
            hipError_t cerr = hipSuccess;
            for (int k = 0; k < 2; ++k) {
                if (part[k] && cerr == hipSuccess)
                    cerr = hipMemcpyAsync((char *)slot[cur].host + off, (const char *)d_out[cur] + off, part[k],
                                          hipMemcpyDeviceToHost, copy_stream[k]);
                if (cerr == hipSuccess) cerr = hipEventRecord(slot[cur].copied[k], copy_stream[k]);
                off += part[k];
            }
            if (cerr != hipSuccess) {
                fprintf(stderr, "\nERROR: device -> host copy failed: %s\n", hipGetErrorString(cerr));
                rc = 1;
                break;
            }
        }
        have_state = true;
        {
            std::lock_guard<std::mutex> lk(mu);
            slot[cur].full = true;
        }
        cv.notify_all();
        cur ^= 1;
        emitted += n;
        if (verbose || isatty(fileno(stderr))) {
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
            fprintf(stderr, "\rTime into run = %4.1f - %4.1f", emitted / 10.0, el);
        }
    }
    {
        std::lock_guard<std::mutex> lk(rmu);
        consumer_gone = true;
    }
    rcv.notify_all();
    producer.join();
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !slot[0].full && !slot[1].full; });
        done = true;
    }
    cv.notify_all();
    writer.join();
    // (the sink is closed inside the reported time: unmapping a 1.2 GB file mapping is not free, and the file is only
    // the caller's once it is closed)
    if (!sink.finish()) io_error = true;
    stage("run (= Process time)");
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    fprintf(stderr, "\nDone!\nProcess time = %.2f [sec]  (%.1f Msamples/s, %.0fx real time)\n", el,
            emitted * 0.26 / el, emitted * 0.1 / el);
    if (monitor_fp) {
        if (hipStreamSynchronize(stream) != hipSuccess) rc = 1;
        for (int i = 0; i < 2 && rc == 0; ++i)
            if (mon[i].pending) monitor_flush(mon[i], monitor_fp, kOutRate, mon_shape, mon_sum);
        if (fclose(monitor_fp) != 0) {
            fprintf(stderr, "ERROR: writing the monitor file %s failed\n", monitor_arg);
            rc = 1;
        }
        fprintf(stderr, "Monitor (%s, every %d epochs, %d code periods each): C/N0 of the composite E1B + E1C signal\n", monitor_arg, monitor_every,
                kMonPeriods);
        for (int prn = 1; prn <= GAL_NUM_PRN; ++prn) {
            const MonSummary &s = mon_sum[prn];
            if (!s.n) continue;
            if (s.n > s.no_peak)
                fprintf(stderr, "  PRN %2d: %4d epochs, C/N0 mean %.2f dB-Hz (min %.2f, max %.2f), peak off the plan in %d, no peak in %d\n", prn, s.n,
                        s.sum / (s.n - s.no_peak), s.lo, s.hi, s.off_peak, s.no_peak);
            else fprintf(stderr, "  PRN %2d: %4d epochs, no peak in any\n", prn, s.n);
        }
        for (int i = 0; i < 2; ++i) {
            hipFree(mon[i].dev);
            hipHostFree(mon[i].host);
        }
    }
    if (agc_log_fp) {
        if (hipStreamSynchronize(stream) != hipSuccess) rc = 1;
        for (int i = 0; i < 2 && rc == 0; ++i)  // (the older batch first)
            if (agc_log[cur ^ i].pending) agc_log_flush(agc_log[cur ^ i]);
        if (fclose(agc_log_fp) != 0) {
            fprintf(stderr, "ERROR: writing the AGC log %s failed\n", agc_log_arg);
            rc = 1;
        }
        fprintf(stderr, "AGC log (%s): %llu blocks of %ld samples\n", agc_log_arg, (unsigned long long)agc_logged, agc_block);
        for (int i = 0; i < 2; ++i) {
            hipFree(agc_log[i].dev);
            hipHostFree(agc_log[i].host);
        }
    }
    if (gal_scen_eph_gaps(scen) > 0)
        fprintf(stderr, "NOTE: %d (satellite, refresh) pairs ran on a stale ephemeris record (see the warning above)\n",
                gal_scen_eph_gaps(scen));
    if (power_on) {
        fprintf(stderr, "Signal power per PRN (Q7 gain, 128 = unity; dB against unity):\n");
        for (int prn = 1; prn <= GAL_NUM_PRN; ++prn)
            if (prn_gain_hi[prn] >= 0)
                fprintf(stderr, "  PRN %2d: gain %5d .. %5d  (%+.2f .. %+.2f dB)\n", prn, prn_gain_lo[prn], prn_gain_hi[prn],
                        prn_gain_lo[prn] > 0 ? 20.0 * log10(prn_gain_lo[prn] / 128.0) : -INFINITY, prn_gain_hi[prn] > 0 ? 20.0 * log10(prn_gain_hi[prn] / 128.0) : -INFINITY);
    }
    if (iq_format == GAL_IQ_IBYTE || mix_on || power_on || mp_on || fir_on || agc_on || osc_on) {
        // (stderr: with -o - the data go to stdout)
        uint64_t n_sat = 0;
        const double n_val = (double)emitted * cfg.samples_per_epoch * 2;
        if (gal_synth_iq_saturated(eng, &n_sat, 0) != GAL_OK) {
            fprintf(stderr, "ERROR: %s\n", gal_synth_last_error());
            rc = 1;
        } else if (n_sat > 0 && iq_format != GAL_IQ_IBYTE) {
            fprintf(stderr, "WARNING: %llu of %.0f IQ values (%.3g %%) saturated at int16; a smaller --signal-gain avoids the clipping\n",
                    (unsigned long long)n_sat, n_val, n_val > 0 ? 100.0 * (double)n_sat / n_val : 0.0);
        } else if (n_sat > 0) {
            fprintf(stderr, "WARNING: %llu of %.0f IQ values (%.3g %%) saturated at --iq-shift %d; a larger --iq-shift avoids the clipping\n",
                    (unsigned long long)n_sat, n_val, n_val > 0 ? 100.0 * (double)n_sat / n_val : 0.0, iq_shift);
        } else if (verbose && iq_format == GAL_IQ_IBYTE) {
            fprintf(stderr, "IQ values saturated at --iq-shift %d: 0 of %.0f\n", iq_shift, n_val);
        }
    }
    gal_synth_destroy(eng);
    gal_scen_close(scen);
    stage("teardown");
    if (io_error) {
        fprintf(stderr, "ERROR: short write on the output sink\n");
        rc = 1;
    }
    return rc;
}
