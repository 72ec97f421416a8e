// galileo-sdr-sim, the option stage: the option table, argv -> Config (csrc/cli_options.h) with every refusal and informational line,
// and the --sites parent.  No device is touched here; the option surface is documented at the top of cli_main.cpp.
#include <getopt.h>
#include <signal.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>

#include "cli_options.h"

std::atomic<bool> g_stop{false};
void on_sigint(int) { g_stop = true; }
const char *const kIqNames[4] = {"ishort", "ibyte", "ibit", "i2bit"};

void die(const char *fmt, ...)  // on stderr; exit(1)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    exit(1);
}

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

namespace {

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

constexpr int kEchoPerPrn = 4;  // --multipath: lines of the file per PRN (EchoSpec: csrc/cli_options.h)

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

bool load_scint(const char *path, std::vector<ScintSpec> *out, std::string *why)
{
    FILE *fp = fopen(path, "r");
    if (!fp) {
        *why = "cannot read it";
        return false;
    }
    char line[1024];
    int lineno = 0;
    bool seen[GAL_NUM_PRN + 1] = {false}, ok = true;
    while (ok && fgets(line, sizeof(line), fp)) {
        ++lineno;
        const char *p = line;
        while (*p == ' ' || *p == '\t') ++p;
        if (*p == '#' || *p == '\n' || *p == '\r' || !*p) continue;
        double v[3] = {0, 0, 0};
        int n = 0;
        for (; n < 3; ++n) {
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
        if (*p == '#') p = "";  // a comment behind the values
        const std::string at = "line " + std::to_string(lineno);
        if (n < 3 || *p) {
            *why = at + " is not prn,s4,tau0_s";
            ok = false;
        } else if (v[0] != floor(v[0]) || v[0] < 1 || v[0] > GAL_NUM_PRN) {
            *why = at + ": PRN outside 1.." + std::to_string(GAL_NUM_PRN);
            ok = false;
        } else if (seen[(int)v[0]]) {
            *why = at + ": a second line for PRN " + std::to_string((int)v[0]);
            ok = false;
        } else if (!(v[1] >= 0.0 && v[1] <= 1.0)) {
            *why = at + ": s4 outside 0..1";
            ok = false;
        } else {
            ScintSpec s;
            memset(&s, 0, sizeof(s));
            s.prn = (int)v[0];
            s.s4 = v[1], s.tau0_s = v[2];
            seen[s.prn] = true;
            out->push_back(s);
        }
    }
    fclose(fp);
    if (ok && out->empty()) {
        *why = "it holds no satellite";
        ok = false;
    }
    return ok;
}

// ---- refusing and parsing: the message stays at the call site ------------------------------------------------------------------------------
// the whole string is one number (no range: --cn0 leaves that to the library)
bool parse_double(const char *s, double *v)
{
    char *end = nullptr;
    *v = strtod(s, &end);
    return *s && !*end;
}
bool parse_double(const char *s, double lo, double hi, double *v) { return parse_double(s, v) && *v >= lo && *v <= hi; }
bool parse_long(const char *s, long lo, long hi, long *v)
{
    char *end = nullptr;
    *v = strtol(s, &end, 10);
    return *s && !*end && *v >= lo && *v <= hi;
}
bool parse_u64(const char *s, uint64_t *v)  // any base strtoull knows; a leading '-' is refused, not wrapped
{
    char *end = nullptr;
    errno = 0;
    *v = strtoull(s, &end, 0);
    return *s && !*end && !errno && s[0] != '-';
}
bool parse_u32(const char *s, uint32_t *v)
{
    uint64_t w = 0;
    if (!parse_u64(s, &w) || w > 0xffffffffull) return false;
    *v = (uint32_t)w;
    return true;
}

// ---- the derivation arithmetic ---------------------------------------------------------------------------------------------------------------
int shift_for(double peak)  // the smallest ibyte shift with 127 x 2^s >= peak
{
    int s = 0;
    while (s < 15 && 127.0 * (double)(1 << s) < peak) ++s;
    return s;
}
double gain_for(double peak_at_unity)  // the largest power of two <= 1 that keeps the peak inside int16
{
    double g = 1.0;
    while (g > 1.0 / 65536.0 && peak_at_unity * g > 32767.0) g *= 0.5;
    return g;
}
double tap_gain(const Config &c)  // what the filter does to a white sigma: sqrt(sum h^2) / 16384
{
    double e2 = 0.0;
    for (int k = 0; k < c.n_fir; ++k) e2 += (double)c.fir_taps[k] * (double)c.fir_taps[k];
    return sqrt(e2) / 16384.0;
}
void say(const Config &c, const char *fmt, ...)  // an informational line on stderr; silent under --sites
{
    if (!c.talk) return;
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
}
void say_taps(const Config &c, double fc)
{
    say(c, "Front-end filter: low-pass, cutoff %g Hz, %d taps (Q14):", fc, c.n_fir);
    for (int k = 0; k < c.n_fir; ++k) say(c, " %d", c.fir_taps[k]);
    say(c, "\n");
}

// ---- the option table: one row per option ------------------------------------------------------------------------------------------------
// What the command line said, as the strings it said it in, and what one feature's stage derives for a later one
struct Args {
    bool shift_toe = false, ref_T = false, agc_given = false, power_model = false;
    const char *iq_format = "ishort", *iq_shift = nullptr, *monitor = nullptr, *monitor_every = nullptr, *fir = nullptr, *fir_lowpass = nullptr,
               *oversample = nullptr, *multipath = nullptr, *agc = nullptr, *agc_block = nullptr, *agc_window = nullptr, *agc_init = nullptr,
               *agc_log = nullptr, *i2bit_thr = nullptr, *antenna = nullptr, *cn0 = nullptr, *noise_seed = nullptr, *noise_stream = nullptr,
               *signal_gain = nullptr, *lo_offset = nullptr, *phase_noise = nullptr, *osc_seed = nullptr, *osc_stream = nullptr,
               *scint = nullptr, *scint_seed = nullptr, *scint_site = nullptr, *array = nullptr, *array_log = nullptr, *reflector_prn = nullptr,
               *reflector_log = nullptr, *spectrum = nullptr, *spectrum_every = nullptr, *spectrum_size = nullptr, *spectrum_window = nullptr;
    std::vector<const char *> prn_power, jam, jam_dir, reflector;
    long agc_window_n = 8;
    double agc_target = 0.0, agc_init_rms = -1.0;  // (0 / < 0: the defaults, known once shift and sigma are)
    double sig_peak = 4100.0;                      // the largest |x| of the signal sum: 4100 in the reference's scenarios
    double jam_unit = 0.0, gain = 1.0;             // the sum of the --jam amplitudes at signal gain 1, int16 LSB; the signal gain
};

enum { OPT_STRICT = 1000, OPT_SITES, OPT_WRITERS, OPT_GPUS, OPT_PER_GPU, OPT_EXACT, OPT_SHIFT_TOE, OPT_REF_T, OPT_JAM, OPT_POWER_MODEL, OPT_PRN_POWER, OPT_AGC,
       OPT_JAM_DIR, OPT_REFLECTOR, OPT_STRING };  // OPT_STRING + k: the k-th row whose argument is only kept (Args::*dest)
constexpr int NO = no_argument, ARG = required_argument, MAYBE = optional_argument;
struct OptRow {
    const char *name;  // one letter: a short option (its id is the letter)
    int has_arg, id;
    bool to_children;  // --sites forwards it: not -l / -o / -P, which every site gets of its own, nor what is the parent's alone
    const char *Args::*dest;
};
const OptRow kOptions[] = {
    {"e", ARG, 'e', true, nullptr}, {"n", ARG, 'n', true, nullptr}, {"o", ARG, 'o', false, nullptr}, {"u", ARG, 'u', true, nullptr},
    {"g", ARG, 'g', true, nullptr}, {"l", ARG, 'l', false, nullptr}, {"T", ARG, 'T', true, nullptr}, {"t", ARG, 't', true, nullptr},
    {"d", ARG, 'd', true, nullptr}, {"G", ARG, 'G', true, nullptr}, {"a", ARG, 'a', true, nullptr}, {"p", ARG, 'p', true, nullptr},
    {"i", NO, 'i', true, nullptr}, {"I", ARG, 'I', true, nullptr}, {"U", ARG, 'U', true, nullptr}, {"b", ARG, 'b', true, nullptr},
    {"v", NO, 'v', true, nullptr}, {"B", ARG, 'B', true, nullptr}, {"P", ARG, 'P', false, nullptr}, {"r", NO, 'r', true, nullptr},
    {"C", NO, 'C', true, nullptr},
    {"strict", NO, OPT_STRICT, true, nullptr}, {"exact-replay", NO, OPT_EXACT, true, nullptr}, {"shift-toe", NO, OPT_SHIFT_TOE, true, nullptr},
    {"ref-T", NO, OPT_REF_T, true, nullptr}, {"sites", ARG, OPT_SITES, false, nullptr}, {"writers", ARG, OPT_WRITERS, true, nullptr},
    {"gpus", ARG, OPT_GPUS, false, nullptr}, {"per-gpu", ARG, OPT_PER_GPU, false, nullptr}, {"jam", ARG, OPT_JAM, true, nullptr},
    {"power-model", NO, OPT_POWER_MODEL, true, nullptr}, {"prn-power", ARG, OPT_PRN_POWER, true, nullptr}, {"agc", MAYBE, OPT_AGC, true, &Args::agc},
    {"iq-format", ARG, OPT_STRING + 0, true, &Args::iq_format}, {"iq-shift", ARG, OPT_STRING + 1, true, &Args::iq_shift},
    {"cn0", ARG, OPT_STRING + 2, true, &Args::cn0}, {"noise-seed", ARG, OPT_STRING + 3, true, &Args::noise_seed},
    {"noise-stream", ARG, OPT_STRING + 4, false, &Args::noise_stream}, {"signal-gain", ARG, OPT_STRING + 5, true, &Args::signal_gain},
    {"monitor", ARG, OPT_STRING + 6, false, &Args::monitor}, {"monitor-every", ARG, OPT_STRING + 7, true, &Args::monitor_every},
    {"antenna", ARG, OPT_STRING + 8, true, &Args::antenna}, {"fir", ARG, OPT_STRING + 9, true, &Args::fir},
    {"fir-lowpass", ARG, OPT_STRING + 10, true, &Args::fir_lowpass}, {"oversample", ARG, OPT_STRING + 11, true, &Args::oversample},
    {"agc-block", ARG, OPT_STRING + 12, true, &Args::agc_block}, {"agc-window", ARG, OPT_STRING + 13, true, &Args::agc_window},
    {"agc-init-rms", ARG, OPT_STRING + 14, true, &Args::agc_init}, {"agc-log", ARG, OPT_STRING + 15, false, &Args::agc_log},
    {"i2bit-threshold", ARG, OPT_STRING + 16, true, &Args::i2bit_thr}, {"multipath", ARG, OPT_STRING + 17, true, &Args::multipath},
    {"lo-offset", ARG, OPT_STRING + 18, true, &Args::lo_offset}, {"phase-noise", ARG, OPT_STRING + 19, true, &Args::phase_noise},
    {"osc-seed", ARG, OPT_STRING + 20, true, &Args::osc_seed}, {"osc-stream", ARG, OPT_STRING + 21, false, &Args::osc_stream},
    {"scint", ARG, OPT_STRING + 22, true, &Args::scint}, {"scint-seed", ARG, OPT_STRING + 23, true, &Args::scint_seed},
    {"scint-site", ARG, OPT_STRING + 24, false, &Args::scint_site}, {"array", ARG, OPT_STRING + 25, false, &Args::array},
    {"array-log", ARG, OPT_STRING + 26, false, &Args::array_log}, {"jam-dir", ARG, OPT_JAM_DIR, false, nullptr},
    {"reflector", ARG, OPT_REFLECTOR, true, nullptr}, {"reflector-prn", ARG, OPT_STRING + 27, true, &Args::reflector_prn},
    {"reflector-log", ARG, OPT_STRING + 28, false, &Args::reflector_log},
    {"spectrum", ARG, OPT_STRING + 29, false, &Args::spectrum}, {"spectrum-every", ARG, OPT_STRING + 30, false, &Args::spectrum_every},
    {"spectrum-size", ARG, OPT_STRING + 31, false, &Args::spectrum_size}, {"spectrum-window", ARG, OPT_STRING + 32, false, &Args::spectrum_window},
};

// the command line into Args and the Config's plain fields; every option with to_children also into c->child_args
void parse_args(int argc, char *argv[], Args *a, Config *c)
{
    std::string short_opts;
    std::vector<struct option> long_opts;
    for (const OptRow &r : kOptions) {
        if (!r.name[1]) short_opts += std::string(r.name) + (r.has_arg == ARG ? ":" : "");
        else long_opts.push_back({r.name, r.has_arg, nullptr, r.id});
    }
    long_opts.push_back({nullptr, 0, nullptr, 0});
    gal_scen_cfg_t &sc = c->sc;
    int opt;
    while ((opt = getopt_long(argc, argv, short_opts.c_str(), long_opts.data(), nullptr)) != -1) {
        // `--agc 4096`: getopt takes an optional argument only as --agc=4096; a following word that begins like a number is the target
        if (opt == OPT_AGC && !optarg && optind < argc && ((argv[optind][0] >= '0' && argv[optind][0] <= '9') || argv[optind][0] == '.'))
            optarg = argv[optind++];
        const OptRow *row = nullptr;
        for (const OptRow &r : kOptions)
            if (r.id == opt) row = &r;
        if (!row) {  // '?', ':'
            usage(argv[0]);
            exit(1);
        }
        if (row->to_children) {  // (--agc and its value: two words)
            c->child_args.push_back(std::string(row->name[1] ? "--" : "-") + row->name);
            if (optarg) c->child_args.push_back(optarg);
        }
        if (row->dest) a->*(row->dest) = optarg;
        switch (opt) {
        case 'e': c->navfile = optarg; break;
        case 'o': c->outfile = optarg; break;
        case 'u': c->umfile = optarg; break;
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
                printf("ERROR: Invalid date and time.\n");  // (the reference's wording, on stdout as the reference's)
                exit(1);
            }
            sc.have_start = 1;
            break;
        case 'd': sc.duration_s = atof(optarg); break;
        case 'I': sc.iono_enable = 0; break;
        case 'v': c->verbose = true; break;
        case 'B': c->batch_epochs = atoi(optarg); c->have_batch = true; break;
        case 'P':
            sc.udp_port = atoi(optarg);
            sc.udp_loopback = 0;
            c->udp_given = true;
            break;
        case 'r': c->realtime = true; break;
        case 'C': c->cboc = true; break;
        case OPT_STRICT: sc.strict_eph = 1; break;
        case OPT_EXACT: c->exact_replay = true; break;
        case OPT_SHIFT_TOE: a->shift_toe = true; break;
        case OPT_REF_T: a->ref_T = true; break;
        case OPT_SITES: c->sitesfile = optarg; break;
        case OPT_WRITERS: c->n_writers = atoi(optarg); break;
        case OPT_GPUS: c->sites_gpus = atoi(optarg); break;
        case OPT_PER_GPU: c->sites_per_gpu = atoi(optarg); break;
        case OPT_JAM: a->jam.push_back(optarg); break;
        case OPT_JAM_DIR: a->jam_dir.push_back(optarg); break;
        case OPT_REFLECTOR: a->reflector.push_back(optarg); break;
        case OPT_POWER_MODEL: a->power_model = true; break;
        case OPT_PRN_POWER: a->prn_power.push_back(optarg); break;
        case OPT_AGC: a->agc_given = true; break;
        default: break;  // a kept string, or -n -g -G -a -p -i -U -b: accepted for compatibility
        }
    }
}

// ---- one function per feature, in the order of the passes: messages and informational lines come out in this order ------------------
void cfg_time(const Args &a, Config &c)
{
    if (c.navfile.empty()) {
        printf("ERROR: Galileo ephemeris/nav_msg file is not specified.\n");
        exit(1);
    }
    // plain -T is the reference as built (time_overwrite 1: the same command line gives the same bytes; ADVICE r5 -- round 5 had it
    // shift, and every replay of a reference command line had to add --ref-T); --shift-toe asks for the shift of TOC / TOE (2)
    if ((a.shift_toe || a.ref_T) && !c.sc.time_overwrite) {
        printf("ERROR: %s needs -T <date,time>.\n", a.ref_T ? "--ref-T" : "--shift-toe");
        exit(1);
    }
    if (a.shift_toe && a.ref_T) {
        printf("ERROR: --shift-toe and --ref-T exclude each other.\n");
        exit(1);
    }
    if (c.sc.time_overwrite) c.sc.time_overwrite = a.shift_toe ? 2 : 1;
}

// the output format and the AGC's strings; the AGC's parameters are made in cfg_agc, once shift and sigma are known
void cfg_format(Args &a, Config &c)
{
    c.iq_format = -1;
    for (int f = 0; f < 4; ++f)
        if (strcmp(a.iq_format, kIqNames[f]) == 0) c.iq_format = f;
    if (c.iq_format < 0) die("ERROR: unknown --iq-format '%s' (accepted: ishort, ibyte, ibit, i2bit).\n", a.iq_format);
    c.agc_on = a.agc_given || c.iq_format == GAL_IQ_I2BIT;  // the 2-bit format implies the AGC
    if (!c.agc_on && (a.agc_block || a.agc_window || a.agc_init || a.agc_log))
        die("ERROR: --agc-block, --agc-window, --agc-init-rms and --agc-log need --agc.\n");
    if (c.agc_on && c.iq_format == GAL_IQ_IBIT) die("ERROR: --agc does not go with --iq-format ibit: a sign needs no gain control.\n");
    if (a.monitor && c.iq_format == GAL_IQ_I2BIT)
        die("ERROR: --monitor does not read --iq-format i2bit (ishort and ibyte, with or without --agc, it does).\n");
    long v = 0;
    if (a.i2bit_thr) {
        if (c.iq_format != GAL_IQ_I2BIT) die("ERROR: --i2bit-threshold applies to --iq-format i2bit only.\n");
        if (!parse_long(a.i2bit_thr, 1, 32767, &v)) die("ERROR: --i2bit-threshold '%s' out of range (1..32767).\n", a.i2bit_thr);
        c.i2bit_thr = (int)v;
    }
    if (c.agc_on) {
        if (a.agc_block && !parse_long(a.agc_block, GAL_AGC_MIN_BLOCK, GAL_AGC_MAX_BLOCK, &c.agc_block))
            die("ERROR: --agc-block '%s' out of range (%d..%d samples).\n", a.agc_block, GAL_AGC_MIN_BLOCK, GAL_AGC_MAX_BLOCK);
        if (a.agc_window && !parse_long(a.agc_window, 1, GAL_AGC_MAX_WINDOW, &a.agc_window_n))
            die("ERROR: --agc-window '%s' out of range (1..%d blocks).\n", a.agc_window, GAL_AGC_MAX_WINDOW);
        if (c.agc_block * a.agc_window_n > GAL_AGC_MAX_SPAN)
            die("ERROR: --agc-block %ld x --agc-window %ld = %ld samples, more than %d.\n", c.agc_block, a.agc_window_n, c.agc_block * a.agc_window_n,
                GAL_AGC_MAX_SPAN);
        if (a.agc && !parse_double(a.agc, 1.0 / 256.0, 32767.0, &a.agc_target))
            die("ERROR: --agc '%s' is not a target rms in int16 LSB (up to 32767).\n", a.agc);
        if (a.agc_init && !parse_double(a.agc_init, 0.0, 32768.0, &a.agc_init_rms))
            die("ERROR: --agc-init-rms '%s' out of range (0..32768 int16 LSB).\n", a.agc_init);
        if (a.agc_log && (!*a.agc_log || strcmp(a.agc_log, "-") == 0)) die("ERROR: --agc-log needs a file name.\n");
        if (a.agc_log && !c.talk) die("ERROR: --agc-log writes one file; it does not go with --sites.\n");
        c.agc_log_file = a.agc_log;
    }
    c.iq_shift_given = a.iq_shift != nullptr;
    if (a.iq_shift) {
        if (c.iq_format != GAL_IQ_IBYTE) die("ERROR: --iq-shift applies to --iq-format ibyte only.\n");
        if (!parse_long(a.iq_shift, 0, 15, &v)) die("ERROR: --iq-shift '%s' out of range (0..15).\n", a.iq_shift);
        c.iq_shift = (int)v;
    } else if (c.iq_format == GAL_IQ_IBYTE) {
        c.iq_shift = 5;  // sigma of 9-12 channels ~ 750-870 LSB: 23-27 LSB after the shift, the clamp at ~5 sigma
    }
}

// --array <file>: east_m,north_m,up_m per line; what follows a # is a comment
bool load_array(const char *path, std::vector<ArrayElem> *out, std::string *why)
{
    FILE *f = fopen(path, "r");
    if (!f) return *why = "cannot be opened", false;
    char line[512];
    for (int ln = 1; fgets(line, sizeof(line), f); ++ln) {
        if (char *h = strchr(line, '#')) *h = 0;
        const char *p = line;
        while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') ++p;
        if (!*p) continue;
        ArrayElem e;
        char tail = 0;
        if (sscanf(p, "%lf , %lf , %lf %c", &e.enu[0], &e.enu[1], &e.enu[2], &tail) != 3 || !std::isfinite(e.enu[0]) || !std::isfinite(e.enu[1]) ||
            !std::isfinite(e.enu[2])) {
            fclose(f);
            return *why = "line " + std::to_string(ln) + " is not east_m,north_m,up_m", false;
        }
        out->push_back(e);
    }
    fclose(f);
    if (out->empty() || out->size() > GAL_ARRAY_MAX_ELEM) return *why = "it must hold 1 to " + std::to_string(GAL_ARRAY_MAX_ELEM) + " elements", false;
    return true;
}

// --array, --array-log, --jam-dir: the elements, the directions of the --jam sources, and what does not go with an array.  Echo
// directions need a direction of arrival per echo, and the four stateful stages keep ONE state per handle where an array needs one per
// element
void cfg_array(const Args &a, Config &c)
{
    const double kD2R = 3.14159265358979323846 / 180.0;
    for (int k = 0; k < GAL_INTERF_MAX; ++k) c.jam_az[k] = 0.0, c.jam_el[k] = 90.0 * kD2R;
    if (!a.array) {
        if (a.array_log) die("ERROR: --array-log needs --array <file>.\n");
        if (!a.jam_dir.empty()) die("ERROR: --jam-dir needs --array <file>.\n");
        return;
    }
    if (a.multipath) die("ERROR: --array does not go with --multipath: an echo needs a direction of arrival of its own.\n");
    if (!a.reflector.empty()) die("ERROR: --reflector does not go with --array: an echo needs a direction of arrival of its own.\n");
    if (a.lo_offset || a.phase_noise) die("ERROR: --array does not go with --lo-offset / --phase-noise: the oscillator keeps one state per engine, an array needs one per element.\n");
    if (a.fir || a.fir_lowpass) die("ERROR: --array does not go with --fir / --fir-lowpass: the filter keeps one history per engine, an array needs one per element.\n");
    if (a.oversample) die("ERROR: --array does not go with --oversample: the decimator keeps one history per engine, an array needs one per element.\n");
    if (a.agc_given) die("ERROR: --array does not go with --agc: the AGC keeps one state per engine, an array needs one per element.\n");
    if (c.iq_format == GAL_IQ_I2BIT) die("ERROR: --array does not go with --iq-format i2bit: the 2-bit format is the AGC's.\n");
    if (a.monitor) die("ERROR: --array does not go with --monitor: the monitor follows one stream.\n");
    if (!c.sitesfile.empty()) die("ERROR: --array does not go with --sites.\n");
    if (c.outfile == "-") die("ERROR: --array writes one file per element; -o - is one stream.\n");
    if (a.jam_dir.size() > a.jam.size()) die("ERROR: --jam-dir may be given once per --jam (%zu --jam, %zu --jam-dir).\n", a.jam.size(), a.jam_dir.size());
    for (size_t k = 0; k < a.jam_dir.size(); ++k) {
        double az = 0.0, el = 0.0;
        char tail = 0;
        if (sscanf(a.jam_dir[k], "%lf , %lf %c", &az, &el, &tail) != 2 || !std::isfinite(az) || !std::isfinite(el) || el < -90.0 || el > 90.0)
            die("ERROR: --jam-dir '%s' is not az_deg,el_deg (elevation -90..90).\n", a.jam_dir[k]);
        c.jam_az[k] = az * kD2R;
        c.jam_el[k] = el * kD2R;
    }
    std::string why;
    if (!load_array(a.array, &c.array, &why)) die("ERROR: --array %s: %s.\n", a.array, why.c_str());
    if (a.array_log && (!*a.array_log || strcmp(a.array_log, "-") == 0)) die("ERROR: --array-log needs a file name.\n");
    c.array_log_file = a.array_log;
    say(c, "Antenna array: %zu element%s (east, north, up in metres from the reference point; the body does not rotate)\n", c.array.size(),
        c.array.size() == 1 ? "" : "s");
    for (size_t k = 0; k < c.array.size(); ++k)
        say(c, "  element %zu: %.4f, %.4f, %.4f%s\n", k, c.array[k].enu[0], c.array[k].enu[1], c.array[k].enu[2],
            a.cn0 ? (" (noise stream 8 x --noise-stream + " + std::to_string(k) + ")").c_str() : "");
    for (size_t k = 0; k < a.jam.size(); ++k)
        say(c, "  --jam %zu arrives from azimuth %.2f deg, elevation %.2f deg%s\n", k + 1, c.jam_az[k] / kD2R, c.jam_el[k] / kD2R,
            k < a.jam_dir.size() ? "" : " (no --jam-dir: the zenith)");
}

// --reflector, --reflector-prn, --reflector-log: the planes, the satellites that see them, and what does not go with them yet.  Returns
// the sum of the reflectors' amplitudes: a satellite can reach 1 + that sum times its own amplitude
double cfg_reflectors(const Args &a, Config &c)
{
    const double kD2R = 3.14159265358979323846 / 180.0;
    if (a.reflector.empty()) {
        if (a.reflector_prn || a.reflector_log) die("ERROR: --reflector-prn and --reflector-log need --reflector.\n");
        return 0.0;
    }
    if (a.multipath) die("ERROR: --reflector does not go with --multipath: both fill the one echo table of a batch.\n");
    if (a.scint) die("ERROR: --reflector does not go with --scint: the scintillated part is not handed to the reflector pass yet.\n");
    if (a.array) die("ERROR: --reflector does not go with --array: an echo needs a direction of arrival of its own.\n");
    if (a.reflector.size() > (size_t)kReflMax) die("ERROR: --reflector may be given %d times at most.\n", kReflMax);
    double sum = 0.0;
    for (const char *text : a.reflector) {
        ReflSpec r = {};
        double v[4] = {0, 0, 0, 0};
        char tail = 0;
        int got = 0;
        r.phase_deg = 180.0;
        if (strncmp(text, "ground,", 7) == 0) {
            r.kind = GAL_REFL_GROUND;
            got = sscanf(text + 7, "%lf , %lf , %lf %c", &v[0], &v[1], &v[2], &tail);
            if (got < 2 || got > 3) die("ERROR: --reflector '%s' is not ground,h_m,rel_db[,phase_deg].\n", text);
            r.p[0] = v[0], r.rel_db = v[1];
            if (got == 3) r.phase_deg = v[2];
        } else if (strncmp(text, "wall,", 5) == 0) {
            r.kind = GAL_REFL_WALL;
            got = sscanf(text + 5, "%lf , %lf , %lf , %lf %c", &v[0], &v[1], &v[2], &v[3], &tail);
            if (got < 3 || got > 4) die("ERROR: --reflector '%s' is not wall,dist_m,az_deg,rel_db[,phase_deg].\n", text);
            r.p[0] = v[0], r.p[1] = v[1] * kD2R, r.rel_db = v[2];
            if (got == 4) r.phase_deg = v[3];
        } else {
            die("ERROR: --reflector '%s' is neither ground,h_m,rel_db[,phase_deg] nor wall,dist_m,az_deg,rel_db[,phase_deg].\n", text);
        }
        // the library's own refusals, on a satellite at the zenith: a plane that is not finite or lies on the wrong side, an amplitude above 2
        double x = 0.0;
        gal_iq_refl_t row;
        if (!std::isfinite(r.phase_deg) || gal_synth_refl_geom(r.kind, r.p, 0.0, 90.0 * kD2R, &x) != GAL_OK ||
            gal_synth_refl_row(0.0, 0.0, r.rel_db, r.phase_deg, 2.6e6, 1, 0, &row) != GAL_OK)
            die("ERROR: --reflector %s: %s\n", text, std::isfinite(r.phase_deg) ? gal_synth_last_error() : "the phase is not finite");
        sum += pow(10.0, r.rel_db / 20.0);
        c.refls.push_back(r);
    }
    for (int p = 1; p <= GAL_NUM_PRN; ++p) c.refl_prn[p] = a.reflector_prn == nullptr;
    for (const char *s = a.reflector_prn; s && *s;) {
        char *end = nullptr;
        const long p = strtol(s, &end, 10);
        if (end == s || p < 1 || p > GAL_NUM_PRN || (*end && *end != ',')) die("ERROR: --reflector-prn '%s' is not prn[,prn...] (PRN 1..%d).\n", a.reflector_prn, GAL_NUM_PRN);
        c.refl_prn[p] = true;
        s = *end ? end + 1 : end;
    }
    if (a.reflector_prn && !*a.reflector_prn) die("ERROR: --reflector-prn '' is not prn[,prn...] (PRN 1..%d).\n", GAL_NUM_PRN);
    if (a.reflector_log && (!*a.reflector_log || strcmp(a.reflector_log, "-") == 0)) die("ERROR: --reflector-log needs a file name.\n");
    c.refl_log_file = a.reflector_log;
    for (size_t k = 0; k < c.refls.size(); ++k) {
        const ReflSpec &r = c.refls[k];
        if (r.kind == GAL_REFL_GROUND)
            say(c, "Reflector %zu: ground, antenna height %.3f m, amplitude %.4f (%.2f dB), reflection phase %.2f deg\n", k, r.p[0], pow(10.0, r.rel_db / 20.0), r.rel_db, r.phase_deg);
        else
            say(c, "Reflector %zu: wall at %.3f m towards azimuth %.2f deg, amplitude %.4f (%.2f dB), reflection phase %.2f deg\n", k, r.p[0], r.p[1] / kD2R,
                pow(10.0, r.rel_db / 20.0), r.rel_db, r.phase_deg);
    }
    say(c, "Reflectors: %zu; a satellite reaches up to %.3f times its own amplitude; at most %d echoes (reflectors x satellites) per epoch\n", c.refls.size(),
        1.0 + sum, GAL_ECHO_MAX);
    return sum;
}

// per-satellite signal power, --multipath and --oversample: what scales the headroom's signal term, and the rate the passes run at
void cfg_signals(Args &a, Config &c)
{
    c.power_model = a.power_model;
    c.have_antenna = a.antenna != nullptr;
    c.power_on = a.power_model || a.antenna || !a.prn_power.empty();
    for (const char *s : a.prn_power)
        if (!parse_prn_power(s, c.prn_db)) die("ERROR: --prn-power '%s' is not prn:dB[,prn:dB...] (PRN 1..%d, -60..60 dB).\n", s, GAL_NUM_PRN);
    std::string why;
    if (a.antenna && !load_antenna(a.antenna, c.ant_db, &why)) die("ERROR: --antenna %s: %s.\n", a.antenna, why.c_str());
    // the largest gain the options can produce, as a factor: the path loss of a satellite at the zenith of a low orbit point (the
    // nominal altitude against 22 900 km: 1.4 %), the least attenuation of the pattern, the largest offset (PRNs without one: 0 dB)
    double power_peak = 1.0;
    if (c.power_on) {
        double att = c.ant_db[0], off = 0.0;
        for (double v : c.ant_db) att = v < att ? v : att;
        for (double v : c.prn_db) off = v > off ? v : off;
        power_peak = (a.power_model ? 23222000.0 / 22900000.0 : 1.0) * pow(10.0, -att / 20.0) * pow(10.0, off / 20.0);
        say(c, "Signal power: path loss %s, antenna %s, %zu PRN offset list%s; largest gain %.3f (%.2f dB)\n", a.power_model ? "on" : "off",
            a.antenna ? a.antenna : "isotropic", a.prn_power.size(), a.prn_power.size() == 1 ? "" : "s", power_peak, 20.0 * log10(power_peak));
    }
    // a satellite with echoes can reach 1 + sum alpha times its own amplitude: the largest such sum
    double echo_peak = 1.0 + cfg_reflectors(a, c), echo_sum[GAL_NUM_PRN + 1] = {0};
    if (a.multipath) {
        if (!load_multipath(a.multipath, &c.echoes, &why)) die("ERROR: --multipath %s: %s.\n", a.multipath, why.c_str());
        for (const EchoSpec &e : c.echoes) {
            echo_sum[e.prn] += pow(10.0, e.rel_db / 20.0);
            echo_peak = 1.0 + echo_sum[e.prn] > echo_peak ? 1.0 + echo_sum[e.prn] : echo_peak;
        }
    }
    long v = 0;
    if (a.oversample && !parse_long(a.oversample, 2, 15, &v))
        die("ERROR: --oversample '%s' out of range (2..15: the engine synthesises at up to 40 MS/s).\n", a.oversample);
    if (a.oversample) c.osr = (int)v;
    const double kLight = 299792458.0, rate = c.sample_rate();
    for (size_t k = 0; k < c.echoes.size(); ++k) {  // the delays in samples of the rate the pass runs at
        EchoSpec &e = c.echoes[k];
        if (gal_synth_mpath_make(e.delay_m / kLight, e.rel_db, e.phase_deg, e.fade_hz, rate, &e.echo) != GAL_OK)
            die("ERROR: --multipath %s, echo %zu (PRN %d): %s\n", a.multipath, k + 1, e.prn, gal_synth_last_error());
        say(c, "Multipath %zu: PRN %d, delay %u samples = %.2f m (asked %.2f m), amplitude %.4f (%.2f dB), phase %.2f deg, fading %.3f Hz\n", k + 1,
            e.prn, e.echo.delay, e.echo.delay / rate * kLight, e.delay_m, e.echo.alpha_q12 / 4096.0, e.rel_db, e.echo.ph0 / 4294967296.0 * 360.0,
            e.echo.dph / 4294967296.0 * rate);
    }
    if (c.mp_on() && echo_peak > 1.0)
        say(c, "Multipath: %zu echo%s; a satellite reaches up to %.3f times its own amplitude\n", c.echoes.size(), c.echoes.size() == 1 ? "" : "es", echo_peak);
    // --scint: a scintillating satellite is taken at (A + 4 B) / 4096 times its own amplitude (the direct component plus four sigma of
    // a scattered one), its echoes with it: the largest of (A + 4 B) / 4096 x (1 + sum alpha) over the PRNs, and of echo_peak
    double sat_peak = echo_peak;
    if (!a.scint && (a.scint_seed || a.scint_site)) die("ERROR: --scint-seed and --scint-site need --scint <file>.\n");
    if (a.scint) {
        if (!load_scint(a.scint, &c.scints, &why)) die("ERROR: --scint %s: %s.\n", a.scint, why.c_str());
        uint64_t seed = 1;
        uint32_t site = 0;
        if (a.scint_seed && !parse_u64(a.scint_seed, &seed)) die("ERROR: --scint-seed '%s' is not an unsigned 64-bit integer.\n", a.scint_seed);
        if (a.scint_site && (!parse_u32(a.scint_site, &site) || site >> 24)) die("ERROR: --scint-site '%s' is not an integer in 0..2^24-1.\n", a.scint_site);
        for (ScintSpec &s : c.scints) {
            if (gal_synth_scint_make(s.s4, s.tau0_s, rate, &s.row) != GAL_OK) die("ERROR: --scint %s, PRN %d: %s\n", a.scint, s.prn, gal_synth_last_error());
            s.row.seed = seed;
            s.row.stream = (site << 8) | (uint32_t)s.prn;
            const double f = (s.row.a_q12 + 4.0 * s.row.b_q12) / 4096.0 * (1.0 + echo_sum[s.prn]);
            sat_peak = f > sat_peak ? f : sat_peak;
            say(c, "Scintillation: PRN %d, S4 %g, tau0 %g s -> A %u, B %u, L %u (tau0 %.6g s at %g MS/s), seed %llu, stream %u\n", s.prn, s.s4, s.tau0_s,
                s.row.a_q12, s.row.b_q12, s.row.node_len, 8.0 * s.row.node_len / rate, rate / 1e6, (unsigned long long)s.row.seed, s.row.stream);
        }
        if (sat_peak > 1.0) say(c, "Scintillation: a satellite is taken at up to %.3f times its own amplitude\n", sat_peak);
    }
    a.sig_peak = 4100.0 * power_peak * sat_peak;
    if (c.array_on()) {  // a rotation can move up to sqrt(2) of a part's amplitude onto one rail
        a.sig_peak *= sqrt(2.0);
        say(c, "Antenna array: the signal term of the automatic --signal-gain / --iq-shift is taken sqrt(2) larger, %.0f LSB (a rotated part)\n", a.sig_peak);
    }
}

void given_gain(Args &a)
{
    if (!parse_double(a.signal_gain, -HUGE_VAL, 16.0, &a.gain) || !(a.gain > 0.0)) die("ERROR: --signal-gain '%s' out of range (0 < g <= 16).\n", a.signal_gain);
}

// --cn0 and --jam: the noise floor, the signal gain, the automatic --iq-shift, the sources
void cfg_mix(Args &a, Config &c)
{
    const double rate = c.sample_rate();
    if (!a.cn0 && (a.noise_seed || a.noise_stream || (a.signal_gain && a.jam.empty())))
        die("ERROR: --noise-seed, --noise-stream and --signal-gain need --cn0 <dBHz>.\n");
    // interference: the strings are checked here, the sources are made below, once the signal gain is known
    JamSpec jam[GAL_INTERF_MAX];
    c.n_jam = (int)a.jam.size();
    if (c.n_jam > GAL_INTERF_MAX) die("ERROR: --jam may be given %d times at most.\n", GAL_INTERF_MAX);
    for (int k = 0; k < c.n_jam; ++k) {
        gal_iq_interf_t probe;
        if (!parse_jam(a.jam[k], &jam[k])) die("ERROR: --jam '%s' is not js_db,f_hz[,f_hi_hz,sweep_us[,period_us,on_us]].\n", a.jam[k]);
        if (gal_synth_interf_make(jam[k].js_db, 0.0, rate, jam[k].f_lo, jam[k].f_hi, jam[k].sweep_s, jam[k].period_s, jam[k].on_s, &probe) != GAL_OK)
            die("ERROR: --jam %s: %s\n", a.jam[k], gal_synth_last_error());  // (gain 0: everything but the amplitude)
        a.jam_unit += 250.0 * sqrt(2.0) * pow(10.0, jam[k].js_db / 20.0);
    }
    const bool auto_shift = c.iq_format == GAL_IQ_IBYTE && !c.iq_shift_given;
    const char *chosen = c.iq_shift_given ? "" : " (chosen)";
    if (a.cn0) {
        double cn0 = 0.0;
        if (!parse_double(a.cn0, &cn0)) die("ERROR: --cn0 '%s' is not a number (dB-Hz).\n", a.cn0);
        if (a.signal_gain) {
            given_gain(a);
        } else {
            // the largest power of two <= 1 with 5 sigma + 4100 g + the --jam amplitudes <= 32767; sigma and the amplitudes are proportional to g
            gal_iq_noise_t unit;
            if (gal_synth_noise_from_cn0(cn0, rate, 1.0, &unit) != GAL_OK) die("ERROR: --cn0 %s: %s\n", a.cn0, gal_synth_last_error());
            a.gain = gain_for(5.0 * (unit.sigma_q4 / 16.0) + a.sig_peak + a.jam_unit);
        }
        if (gal_synth_noise_from_cn0(cn0, rate, a.gain, &c.noise) != GAL_OK) die("ERROR: --cn0 %s: %s\n", a.cn0, gal_synth_last_error());
        c.noise.seed = 1;
        if (a.noise_seed && !parse_u64(a.noise_seed, &c.noise.seed)) die("ERROR: --noise-seed '%s' is not an unsigned 64-bit integer.\n", a.noise_seed);
        if (a.noise_stream && !parse_u32(a.noise_stream, &c.noise.stream))
            die("ERROR: --noise-stream '%s' is not an unsigned 32-bit integer.\n", a.noise_stream);
        c.noise_on = true;
        const double sigma = c.noise.sigma_q4 / 16.0;
        // the smallest shift with 127 x 2^s >= 4 sigma + the --jam amplitudes (--oversample: cfg_filter, with the sigma behind the decimator)
        if (auto_shift && !c.dec_on()) c.iq_shift = shift_for(4.0 * sigma + (c.agc_on ? 0.0 : a.jam_unit * a.gain));
        say(c, "Noise floor: C/N0 %g dB-Hz -> sigma %.1f LSB, signal gain %g%s, seed %llu, stream %u", cn0, sigma, a.gain, a.signal_gain ? "" : " (chosen)",
            (unsigned long long)c.noise.seed, c.noise.stream);
        if (c.iq_format == GAL_IQ_IBYTE && (!c.dec_on() || c.iq_shift_given)) say(c, ", --iq-shift %d%s", c.iq_shift, chosen);
        say(c, "\n");
    }
    if (c.n_jam == 0) return;
    if (!a.cn0) {  // the sources alone on top of the scaled signals
        if (a.signal_gain) given_gain(a);
        else a.gain = gain_for(a.sig_peak + a.jam_unit);
        c.noise.gain_q16 = (uint32_t)llround(a.gain * 65536.0);  // (sigma_q4 0: nothing random is computed)
        // the smallest shift with 127 x 2^s >= 4100 g + the amplitudes
        if (auto_shift) c.iq_shift = shift_for((a.sig_peak + (c.agc_on ? 0.0 : a.jam_unit)) * a.gain);
    }
    for (int k = 0; k < c.n_jam; ++k)
        if (gal_synth_interf_make(jam[k].js_db, a.gain, rate, jam[k].f_lo, jam[k].f_hi, jam[k].sweep_s, jam[k].period_s, jam[k].on_s, &c.interf[k]) != GAL_OK)
            die("ERROR: --jam %s: %s\n", a.jam[k], gal_synth_last_error());
    if (!a.cn0) {
        say(c, "Interference without a noise floor: signal gain %g%s", a.gain, a.signal_gain ? "" : " (chosen)");
        if (c.iq_format == GAL_IQ_IBYTE) say(c, ", --iq-shift %d%s", c.iq_shift, chosen);
        say(c, "\n");
    }
    for (int k = 0; k < c.n_jam; ++k) {
        const gal_iq_interf_t &s = c.interf[k];
        const double f_lo = s.f0 / 4294967296.0 * rate;
        say(c, "Interference %d: J/S %g dB -> A %.1f LSB, %.1f Hz .. %.1f Hz, sweep %u samples, pulse %u of %u samples\n", k + 1, jam[k].js_db,
            s.amp_q4 / 16.0, f_lo, f_lo + (double)s.df * s.sweep_len / 4294967296.0 * rate, s.sweep_len, s.pulse_on, s.pulse_period);
    }
}

// --spectrum: the sum of win^2, which turns the sums into a power density (header line of the CSV)
uint64_t spectrum_win2(const gal_iq_psd_t &p)
{
    const int32_t *C = gal_tables_psd();
    const int N = 1 << p.log2_n;
    uint64_t s = 0;
    for (int n = 0; n < N; ++n) {
        const uint64_t w = p.window ? (uint64_t)((((int64_t)1 << 30) - C[n * (4096 / N)]) >> 16) : 32768u;
        s += w * w;
    }
    return s;
}

// (usage() does not list the four --spectrum options: its text is recorded byte for byte by tests/golden/cli_transcript.json; README.md does)
void cfg_spectrum(const Args &a, Config &c)
{
    long v = 0;
    if (!a.spectrum) {
        if (a.spectrum_every || a.spectrum_size || a.spectrum_window) die("ERROR: --spectrum-every, --spectrum-size and --spectrum-window need --spectrum <file>.\n");
        return;
    }
    if (!*a.spectrum || strcmp(a.spectrum, "-") == 0) die("ERROR: --spectrum needs a file name.\n");
    if (c.iq_format == GAL_IQ_I2BIT) die("ERROR: --spectrum does not read --iq-format i2bit (ishort, ibyte and ibit it does).\n");
    if (c.array_on()) die("ERROR: --spectrum does not go with --array: the spectrum is of one stream.\n");
    if (!c.sitesfile.empty()) die("ERROR: --spectrum does not go with --sites: run the site on its own.\n");
    if (a.spectrum_every) {
        if (!parse_long(a.spectrum_every, 1, 1000000, &v)) die("ERROR: --spectrum-every '%s' out of range (1..1000000 epochs).\n", a.spectrum_every);
        c.spectrum_every = (int)v;
    }
    if (a.spectrum_size) {
        if (!parse_long(a.spectrum_size, 8, 4096, &v) || (v & (v - 1))) die("ERROR: --spectrum-size '%s' is not a power of two from 8 to 4096.\n", a.spectrum_size);
        c.spectrum.log2_n = 0;
        while ((1L << c.spectrum.log2_n) < v) ++c.spectrum.log2_n;
    }
    if (a.spectrum_window) {
        if (strcmp(a.spectrum_window, "hann") == 0) c.spectrum.window = 1;
        else if (strcmp(a.spectrum_window, "rect") == 0) c.spectrum.window = 0;
        else die("ERROR: --spectrum-window '%s' (accepted: hann, rect).\n", a.spectrum_window);
    }
    const int N = 1 << c.spectrum.log2_n;
    c.spectrum.hop = c.spectrum.window ? N / 2 : N;
    c.spectrum_file = a.spectrum;
    c.spectrum_fp = fopen(a.spectrum, "w");
    if (!c.spectrum_fp) die("ERROR: cannot write the spectrum file %s.\n", a.spectrum);
    fprintf(c.spectrum_fp, "# Welch power spectrum: N=%d hop=%d window=%s format=%s fs_hz=%.0f sum_win2=%llu; lines: time_s,n_seg,p[-N/2],...,p[N/2-1] "
                           "(frequency order, bin k at k fs / N); last line: total\n",
            N, c.spectrum.hop, c.spectrum.window ? "hann" : "rect", kIqNames[c.iq_format], kOutRate, (unsigned long long)spectrum_win2(c.spectrum));
    say(c, "Spectrum: every %d epochs, N = %d, hop %d, %s window -> %s\n", c.spectrum_every, N, c.spectrum.hop, c.spectrum.window ? "Hann" : "rectangular",
        a.spectrum);
}

void cfg_monitor(const Args &a, Config &c)
{
    long v = 0;
    if (a.monitor_every) {
        if (!a.monitor) die("ERROR: --monitor-every needs --monitor <file>.\n");
        if (!parse_long(a.monitor_every, 1, 1000000, &v)) die("ERROR: --monitor-every '%s' out of range (1..1000000 epochs).\n", a.monitor_every);
        c.monitor_every = (int)v;
    }
    c.monitor_file = a.monitor;
    if (!a.monitor) return;
    if (!*a.monitor || strcmp(a.monitor, "-") == 0) die("ERROR: --monitor needs a file name.\n");
    if (c.cboc) die("ERROR: --monitor despreads with the BOC(1,1) replica; it does not go with -C.\n");
    if (!c.talk) return;  // (--sites: every child opens its own <file>.site<i>)
    c.monitor_fp = fopen(a.monitor, "w");
    if (!c.monitor_fp) die("ERROR: cannot write the monitor file %s.\n", a.monitor);
    fprintf(c.monitor_fp, "time_s,prn,doppler_hz,cn0_dbhz,peak_ratio,best_delay_halfchips,best_doppler_bins\n");
}

// --fir <file>: integer taps in Q14, one per line
void load_taps(const char *path, Config &c, int fir_max)
{
    FILE *fp = fopen(path, "r");
    if (!fp) die("ERROR: cannot read the tap file %s.\n", path);
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
        if (end == b || *end || errno || v < -32768 || v > 32767)
            die("ERROR: --fir %s, line %d: not an integer tap in -32768..32767 (Q14: 16384 = 1.0).\n", path, lineno);
        if (c.n_fir == fir_max) die("ERROR: --fir %s holds more than %d taps.\n", path, fir_max);
        c.fir_taps[c.n_fir++] = (int16_t)v;
    }
    fclose(fp);
    if (c.n_fir == 0) die("ERROR: --fir %s holds no tap.\n", path);
}

// the front-end filter, or with --oversample the decimator (whose taps --fir / --fir-lowpass then give)
void cfg_filter(const Args &a, Config &c)
{
    const bool dec_on = c.dec_on();
    const double rate = c.sample_rate();
    if (a.fir && a.fir_lowpass) die("ERROR: --fir and --fir-lowpass exclude each other.\n");
    if (a.fir) {
        load_taps(a.fir, c, dec_on ? GAL_FIRDEC_MAX_TAPS : GAL_FIR_MAX_TAPS);
        if ((dec_on ? gal_synth_firdec_check(c.fir_taps, c.n_fir, c.osr) : gal_synth_fir_check(c.fir_taps, c.n_fir)) != GAL_OK)
            die("ERROR: --fir %s: %s\n", a.fir, gal_synth_last_error());
    }
    if (a.fir_lowpass) {
        char *end = nullptr;
        const double fc = strtod(a.fir_lowpass, &end);
        long nt = 63;
        bool ok = *a.fir_lowpass && end != a.fir_lowpass;
        if (ok && *end == ',') {
            const char *b = end + 1;
            nt = strtol(b, &end, 10);
            ok = *b && end != b && nt >= 0 && nt <= 1000;
        }
        if (!ok || *end) die("ERROR: --fir-lowpass '%s' is not cutoff_hz[,n_taps].\n", a.fir_lowpass);
        if ((dec_on ? gal_synth_firdec_lowpass(fc, rate, (int32_t)nt, c.fir_taps) : gal_synth_fir_lowpass(fc, rate, (int32_t)nt, c.fir_taps)) != GAL_OK)
            die("ERROR: --fir-lowpass %s: %s\n", a.fir_lowpass, gal_synth_last_error());
        c.n_fir = (int)nt;
        say_taps(c, fc);
    }
    if (dec_on && c.n_fir == 0) {  // the default decimator: 0.45 x the output rate, a delay of 16 output samples
        const double fc = 0.45 * kOutRate;
        c.n_fir = 32 * c.osr + 1;
        if (gal_synth_firdec_lowpass(fc, rate, c.n_fir, c.fir_taps) != GAL_OK) die("ERROR: --oversample %d: %s\n", c.osr, gal_synth_last_error());
        say_taps(c, fc);
    }
    c.fir_delay = c.fir_on() ? (c.n_fir - 1) / 2 : 0;
    if (!dec_on) return;
    if (a.monitor && (c.n_fir - 1) % (2 * c.osr) != 0)
        die("ERROR: --monitor with --oversample %d needs taps whose (n_taps - 1) is a multiple of %d: %d taps delay the stream by %g output samples, "
            "and the monitor follows whole samples only.\n", c.osr, 2 * c.osr, c.n_fir, (c.n_fir - 1) / (2.0 * c.osr));
    c.fir_delay = (c.n_fir - 1) / (2 * c.osr);
    if (c.iq_format == GAL_IQ_IBYTE && !c.iq_shift_given && c.noise_on) {
        // the smallest shift with 127 x 2^s >= 4 sigma' + the --jam amplitudes, sigma' = sigma sqrt(sum h^2) / 16384 behind the filter
        const double sigma_out = c.noise.sigma_q4 / 16.0 * tap_gain(c);
        c.iq_shift = shift_for(4.0 * sigma_out + (c.agc_on ? 0.0 : a.jam_unit * a.gain));
        say(c, "Decimator: sigma %.1f LSB behind the filter, --iq-shift %d (chosen)\n", sigma_out, c.iq_shift);
    }
    say(c, "Oversampling: %d x 2.6 MS/s = %g MS/s in front of the decimator, %d taps, delay %g output samples\n", c.osr, rate / 1e6, c.n_fir,
        (c.n_fir - 1) / (2.0 * c.osr));
}

// AGC: the parameters, now that shift and sigma are known
void cfg_agc(Args &a, Config &c)
{
    if (!c.agc_on) return;
    if (a.agc_target == 0.0)
        a.agc_target = c.iq_format == GAL_IQ_IBYTE ? 32.0 * (double)(1 << c.iq_shift) : c.iq_format == GAL_IQ_I2BIT ? (double)c.i2bit_thr : 2048.0;
    if (a.agc_init_rms < 0.0) {  // the noise sigma where the AGC sits: behind --fir or the decimator where there is one
        a.agc_init_rms = 750.0;  // (the sigma of 9-12 channels)
        if (c.noise_on) a.agc_init_rms = c.noise.sigma_q4 / 16.0;
        if (c.noise_on && c.fir_on()) a.agc_init_rms *= tap_gain(c);
    }
    if (gal_synth_agc_from_rms(a.agc_target, a.agc_init_rms, (int32_t)c.agc_block, (int32_t)a.agc_window_n, &c.agc) != GAL_OK)
        die("ERROR: --agc: %s\n", gal_synth_last_error());
    if (!c.talk) return;
    say(c, "AGC: target rms %g LSB, blocks of %ld samples, window %ld blocks, initial rms %g LSB", a.agc_target, c.agc_block, a.agc_window_n, a.agc_init_rms);
    if (c.iq_format == GAL_IQ_IBYTE) say(c, ", --iq-shift %d%s", c.iq_shift, c.iq_shift_given ? "" : " (chosen)");
    if (c.iq_format == GAL_IQ_I2BIT) say(c, ", --i2bit-threshold %d", c.i2bit_thr);
    say(c, "\n");
    if (!a.agc_log) return;
    c.agc_log_fp = fopen(a.agc_log, "w");
    if (!c.agc_log_fp) die("ERROR: cannot write the AGC log %s.\n", a.agc_log);
    fprintf(c.agc_log_fp, "time_s,gain_q12,gain_db\n");
}

// the receiver oscillator; it sits in front of the decimator: with --oversample M it runs at M x 2.6 MS/s
void cfg_osc(const Args &a, Config &c)
{
    c.osc_on = a.lo_offset || a.phase_noise;
    if (!c.osc_on && (a.osc_seed || a.osc_stream)) die("ERROR: --osc-seed and --osc-stream need --lo-offset or --phase-noise.\n");
    if (!c.osc_on) return;
    const double rate = c.sample_rate();
    double lo_hz = 0.0, lo_drift = 0.0, lo_h0 = 0.0;
    if (a.lo_offset) {
        char *end = nullptr;
        lo_hz = strtod(a.lo_offset, &end);
        bool ok = *a.lo_offset && end != a.lo_offset;
        if (ok && *end == ',') {
            const char *d = end + 1;
            lo_drift = strtod(d, &end);
            ok = *d && end != d;
        }
        if (!ok || *end) die("ERROR: --lo-offset '%s' is not hz[,drift_hz_per_s].\n", a.lo_offset);
    }
    if (a.phase_noise && !parse_double(a.phase_noise, &lo_h0)) die("ERROR: --phase-noise '%s' is not a number (h0 in seconds, e.g. 1e-21).\n", a.phase_noise);
    if (gal_synth_osc_make(lo_hz, lo_drift, lo_h0, rate, 1575.42e6, &c.osc) != GAL_OK) die("ERROR: --lo-offset / --phase-noise: %s\n", gal_synth_last_error());
    if (a.osc_seed && !parse_u64(a.osc_seed, &c.osc.seed)) die("ERROR: --osc-seed '%s' is not an unsigned 64-bit integer.\n", a.osc_seed);
    if (a.osc_stream && !parse_u32(a.osc_stream, &c.osc.stream)) die("ERROR: --osc-stream '%s' is not an unsigned 32-bit integer.\n", a.osc_stream);
    const double two64 = 18446744073709551616.0, pi = 3.14159265358979323846;
    const double sig_cyc = 1575.42e6 * sqrt(lo_h0 / (2.0 * rate)), sig_rad = 2.0 * pi * sig_cyc;
    say(c, "Oscillator: offset %.6f Hz, drift %.6g Hz/s (F = %lld, D = %lld at %g MS/s)", (double)c.osc.f / two64 * rate,
        (double)c.osc.d / two64 * rate * rate, (long long)c.osc.f, (long long)c.osc.d, rate / 1e6);
    if (c.osc.s)
        say(c, "; phase noise h0 %g s: sigma %.4g rad per sample (S = %llu), rms phase %.4g rad over 1 ms, %.4g rad over 4 ms, "
               "Lorentzian linewidth %.4g Hz; seed %llu, stream %u",
            lo_h0, sig_rad, (unsigned long long)c.osc.s, sig_rad * sqrt(rate * 1e-3), sig_rad * sqrt(rate * 4e-3), sig_rad * sig_rad * rate / (2.0 * pi),
            (unsigned long long)c.osc.seed, c.osc.stream);
    say(c, "\n");
}

// ---- --sites: one child process per receiver site ---------------------------------------------------------------
struct Site {
    std::string llh, out;
};

}  // namespace

int run_sites(const char *self, const Config &c)
{
    // several listeners cannot share a port: the sites run without the position listener unless -P names a base port, in
    // which case site k (in file order) listens on port + k
    const std::vector<std::string> &base_args = c.child_args;
    const char *sites_file = c.sitesfile.c_str(), *out_stem = c.outfile.c_str(), *fmt_name = kIqNames[c.iq_format], *monitor_file = c.monitor_file;
    int n_gpus = c.sites_gpus, per_gpu = c.sites_per_gpu;
    const int udp_base = c.udp_given ? c.sc.udp_port : 0;
    const double bytes_per_sample = (double)c.out_bytes(4) / 4.0;
    const bool noise_on = c.noise_on, osc_on = c.osc_on, sc_on = c.sc_on();
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
            if (sc_on) {  // ... nor their satellites' fading
                args.push_back("--scint-site");
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


void parse_options(int argc, char *argv[], Config *c)
{
    gal_scen_cfg_t &sc = c->sc;
    memset(&sc, 0, sizeof(sc));
    sc.llh[0] = 42.3601;  // defaults of src/main.cpp:179-196
    sc.llh[1] = -71.0589;
    sc.llh[2] = 2;
    sc.duration_s = 300.0;
    sc.iono_enable = 1;
    sc.n_slots = GAL_MAX_CHAN;
    sc.udp_port = GAL_SCEN_UDP_PORT;  // the reference always listens for position updates (src/galileo-sdr.cpp:185)
    sc.udp_loopback = 1;              // ... on every interface; the default listener here takes local datagrams only
    memset(c->ant_db, 0, sizeof(c->ant_db));
    memset(c->prn_db, 0, sizeof(c->prn_db));
    memset(&c->noise, 0, sizeof(c->noise));
    memset(c->interf, 0, sizeof(c->interf));
    memset(&c->agc, 0, sizeof(c->agc));
    memset(&c->osc, 0, sizeof(c->osc));
    Args a;
    parse_args(argc, argv, &a, c);
    c->talk = c->sitesfile.empty();
    cfg_time(a, *c);
    cfg_format(a, *c);
    cfg_array(a, *c);
    cfg_signals(a, *c);
    cfg_mix(a, *c);
    cfg_monitor(a, *c);
    cfg_spectrum(a, *c);
    cfg_filter(a, *c);
    cfg_agc(a, *c);
    cfg_osc(a, *c);
}
