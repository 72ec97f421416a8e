// galileo-sdr-sim: what the option stage decides (cli_options.cpp), as plain data, made before any device work.
#pragma once
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/galscen.h"
#include "../../include/galsynth.h"

extern std::atomic<bool> g_stop;  // SIGINT: set by on_sigint, read by the run loop, the producer and the --sites parent
void on_sigint(int);

constexpr double kOutRate = 2.6e6;  // the file's rate (and --monitor's); everything in front of the decimator runs at osr times it
constexpr int kOutSamplesPerEpoch = 260000;
extern const char *const kIqNames[4];  // GAL_IQ_ISHORT, GAL_IQ_IBYTE, GAL_IQ_IBIT, GAL_IQ_I2BIT

// --multipath <file>: one echo per line, prn,delay_m,rel_db,phase_deg[,fade_hz]; lines that begin with # and blank lines are skipped
struct EchoSpec {
    int prn;
    double delay_m, rel_db, phase_deg, fade_hz;
    gal_mpath_echo_t echo;  // made once the sample rate is known
};

// --scint <file>: one satellite per line, prn,s4,tau0_s; lines that begin with # and blank lines are skipped
struct ScintSpec {
    int prn;
    double s4, tau0_s;
    gal_iq_scint_t row;  // made once the sample rate is known; stream = site index << 8 | prn
};

// --array <file>: one antenna element per line, east_m,north_m,up_m from the array's reference point; # starts a comment
struct ArrayElem {
    double enu[3];
};

// --reflector ground,h_m,rel_db[,phase_deg] | wall,dist_m,az_deg,rel_db[,phase_deg]: a reflecting plane (gal_synth_refl_geom)
struct ReflSpec {
    int kind;     // GAL_REFL_GROUND, GAL_REFL_WALL
    double p[2];  // height | distance, azimuth of the wall in radians
    double rel_db, phase_deg;
};
constexpr int kReflMax = 4;  // --reflector may be given this often

struct Config {
    gal_scen_cfg_t sc;  // (nav_file / motion_file point into navfile / umfile: set by main, once the Config has its place)
    std::string navfile, outfile, umfile, sitesfile;
    bool verbose = false, have_batch = false, udp_given = false, realtime = false, cboc = false, exact_replay = false;
    int batch_epochs = 128, n_writers = -1, sites_gpus = 0, sites_per_gpu = 1;
    std::vector<std::string> child_args;  // --sites: the options every child gets
    bool talk = true;                     // informational lines are printed (not under --sites: every child prints its own)
    // the output format
    int iq_format = GAL_IQ_ISHORT, iq_shift = 0, i2bit_thr = 1024;
    bool iq_shift_given = false;
    int osr = 1;  // --oversample M; without it 1
    // the passes over the stream, in the order they run; without an option nothing differs from a build without it
    bool power_on = false, power_model = false, have_antenna = false;  // per-satellite signal power
    double ant_db[GAL_GAIN_PATTERN_LEN], prn_db[GAL_NUM_PRN];
    std::vector<EchoSpec> echoes;  // --multipath
    std::vector<ScintSpec> scints; // --scint
    std::vector<ArrayElem> array;  // --array: the batch goes through gal_synth_run_array, one output file per element
    double jam_az[GAL_INTERF_MAX], jam_el[GAL_INTERF_MAX];  // --jam-dir, radians; without one the zenith
    const char *array_log_file = nullptr;
    FILE *array_log_fp = nullptr;
    std::vector<ReflSpec> refls;          // --reflector: the batch goes through gal_synth_run_refl
    bool refl_prn[GAL_NUM_PRN + 1] = {};  // --reflector-prn: the satellites that have the echoes; without it all
    const char *refl_log_file = nullptr;
    FILE *refl_log_fp = nullptr;
    bool noise_on = false;         // --cn0
    gal_iq_noise_t noise;          // (without --cn0 it still carries the signal gain of the --jam sources)
    int n_jam = 0;
    gal_iq_interf_t interf[GAL_INTERF_MAX];
    bool osc_on = false;
    gal_iq_osc_t osc;
    int16_t fir_taps[GAL_FIRDEC_MAX_TAPS];  // --fir / --fir-lowpass; with --oversample the decimator's
    int n_fir = 0, fir_delay = 0;           // the delay of a symmetric filter, in OUTPUT samples: what --monitor follows
    bool agc_on = false;
    gal_iq_agc_t agc;
    long agc_block = 2600;
    const char *agc_log_file = nullptr;
    FILE *agc_log_fp = nullptr;
    const char *monitor_file = nullptr;
    int monitor_every = 10;
    FILE *monitor_fp = nullptr;
    const char *spectrum_file = nullptr;  // --spectrum: the Welch power spectrum of every spectrum_every'th epoch (gal_synth_iq_psd)
    int spectrum_every = 10;
    gal_iq_psd_t spectrum = {10, 512, 1, 0};  // --spectrum-size 1024, --spectrum-window hann: hop N / 2 (rect: N)
    FILE *spectrum_fp = nullptr;

    double sample_rate() const { return (double)osr * kOutRate; }
    bool dec_on() const { return osr > 1; }
    bool fir_on() const { return n_fir > 0; }
    bool mp_on() const { return !echoes.empty(); }
    bool sc_on() const { return !scints.empty(); }
    bool array_on() const { return !array.empty(); }
    bool refl_on() const { return !refls.empty(); }
    bool azel_on() const { return array_on() || refl_on(); }  // the front-end hands out azimuth and elevation
    int n_elem() const { return array_on() ? (int)array.size() : 1; }
    bool parts_on() const { return mp_on() || sc_on(); }  // the batch goes through gal_synth_run_scint (echoes, scintillation or both)
    bool mix_on() const { return noise_on || n_jam > 0; }  // a pass over the final int16 batch in front of the format
    int agc_param() const { return iq_format == GAL_IQ_IBYTE ? iq_shift : iq_format == GAL_IQ_I2BIT ? i2bit_thr : 0; }
    // bytes of n samples in the output format: the AGC has its own count (i2bit is a format of the AGC call only)
    size_t out_bytes(size_t n) const { return agc_on ? gal_synth_agc_out_bytes(iq_format, n) : gal_synth_iq_bytes(iq_format, n); }
    bool any_pass() const { return mix_on() || power_on || parts_on() || refl_on() || array_on() || fir_on() || agc_on || osc_on; }
    // what the copies read was enqueued on the engine's stream: they wait for an event behind it
    bool chain_on_engine_stream() const { return iq_format != GAL_IQ_ISHORT || any_pass(); }
    // the run ends with the saturation report.  Not the predicate above: ibit alone clamps nothing
    bool reports_saturation() const { return iq_format == GAL_IQ_IBYTE || any_pass(); }
};

void usage(const char *prog);
[[noreturn]] void die(const char *fmt, ...);  // the message on stderr, exit(1)
// argv -> Config: refuses (message, exit 1) and prints the informational lines in the order of the passes
void parse_options(int argc, char *argv[], Config *c);
// --sites <file>: one child process of `self` per receiver site; returns the exit code
int run_sites(const char *self, const Config &c);
