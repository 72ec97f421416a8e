// iq_api.cpp -- the output chain's half of the C ABI (include/galsynth.h): every pass over the finished int16 stream -- formats, noise
// floor, interference, per-satellite gains, multipath, scintillation, the antenna array, FIR, decimating FIR, AGC, oscillator -- the correlator bank and the power spectrum, over the kernels of
// csrc/iq_*.hip.  Host-side plumbing only: validation, the stages' device state, kernel sequencing.  The handle itself, plan, execute
// and finish are synth_api.cpp's; synth_handle.h is what the two share.  Nothing here depends on GAL_TEST_HOOKS: one object serves
// libgalsynth.so and libgalsynth_hooks.so.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "synth_handle.h"
#include "gain_q7.h"

extern "C" {
hipError_t galk_launch_iq_pass(int format, const int16_t *in, uint64_t n_val, uint64_t first_sample, const gal_iq_noise_t *noise,
                               const gal_iq_interf_t *src, int n_src, int shift, void *out, unsigned long long *sat, hipStream_t st);
hipError_t galk_launch_iq_fir(const int16_t *in, int16_t *out, uint64_t n, const uint32_t *table_dev, int n_trips, int hs, const uint32_t *hist_in,
                              uint32_t *hist_out, unsigned long long *sat, hipStream_t st);
void galk_fir_table(const int16_t *h, int n_taps, uint32_t *table, int *n_trips, int *hs);
hipError_t galk_launch_iq_firdec(const int16_t *in, int16_t *out, uint64_t n, uint64_t n_out, int i0, int n_taps, int decim,
                                 const uint32_t *table_dev, const uint32_t *hist_in, uint32_t *hist_out, unsigned long long *sat, hipStream_t st);
int galk_firdec_table(const int16_t *h, int n_taps, int decim, uint32_t *table, int *trips);
hipError_t galk_launch_iq_agc(const int16_t *in, uint64_t n, uint32_t off0, int format, int param, const gal_iq_agc_t *p,
                              const unsigned long long *state_in, unsigned long long *state_out, void *scratch, void *out, uint32_t *gains_out,
                              unsigned long long *sat, hipStream_t st);
uint64_t galk_agc_scratch_bytes(uint64_t n, uint32_t off0, uint32_t block_len);
hipError_t galk_launch_iq_osc(const int16_t *in, int16_t *out, uint64_t n, uint64_t first_sample, uint64_t n0, const gal_iq_osc_t *p,
                              const long long *state_in, long long *state_out, void *scratch, unsigned long long *sat, hipStream_t st);
uint64_t galk_osc_scratch_bytes(uint64_t n);
hipError_t galk_launch_iq_scint(const void *jobs_dev, int n_jobs, uint64_t max_n, unsigned long long *sat, hipStream_t st);
hipError_t galk_launch_iq_echo(const int16_t *const *parts_dev, const int16_t *const *hist_in_dev, int16_t *const *hist_out_dev, const int *gain_dev,
                               const void *rows_dev, const int *part_of_dev, int n_parts, int n_echo, int n_epochs, int samples_per_epoch, int wide,
                               int16_t *out, unsigned long long *sat, hipStream_t st);
hipError_t galk_launch_iq_refl(const int16_t *const *parts_dev, const int16_t *const *hist_in_dev, int16_t *const *hist_out_dev, const int *gain_dev,
                               const void *rows_dev, const int *part_of_dev, int n_parts, int n_echo, int n_epochs, int samples_per_epoch, int wide,
                               int16_t *out, unsigned long long *sat, hipStream_t st);
hipError_t galk_launch_iq_wsum(const int16_t *const *parts_dev, const int *gain_dev, int n_parts, int n_epochs, int samples_per_epoch, int wide,
                               int16_t *out, unsigned long long *sat, hipStream_t st);
hipError_t galk_launch_iq_array(const int16_t *const *parts_dev, int16_t *const *outs_dev, const uint32_t *wts_dev, int n_parts, int n_elem,
                                int n_epochs, int samples_per_epoch, int wide, unsigned long long *sat, hipStream_t st);
void galk_array_pack(int w_re, int w_im, uint32_t *two);
hipError_t galk_launch_corr(int format, const void *buf, uint64_t n_eff, uint64_t code_ph0, uint64_t code_dph, uint32_t carr_ph0,
                            uint32_t carr_step0, uint32_t dopp_step, int delay0, int delay_step, int n_delay, int n_dopp, int max_periods,
                            const uint32_t *lut_dev, const uint32_t *code_dev, long long *out, hipStream_t st);
hipError_t galk_launch_psd(int format, const void *buf, uint64_t n_seg, int log2_n, int hop, int window, unsigned long long *out, hipStream_t st);
}

// ---- what every stage's entry points repeat, once ----------------------------------------------------------------------------------
int GrownBuf::reserve(uint64_t need, uint64_t extra, bool pinned, StageSync &sync, uint64_t *cap)
{
    if (need <= bytes) return GAL_OK;
    HIP_TRY(sync.wait());
    release();
    *cap = need + need / 4 + extra;
    const bool fits = *cap == (uint64_t)(size_t)*cap;
    if (!fits || hipMalloc((void **)&dev, (size_t)*cap) != hipSuccess ||
        (pinned && hipHostMalloc((void **)&host, (size_t)*cap, hipHostMallocDefault) != hipSuccess)) {
        (void)hipGetLastError();
        release();
        return GAL_E_NOMEM;
    }
    bytes = (size_t)*cap;
    return GAL_OK;
}

// a stage's fixed device block with the pinned buffer its upload reads: both, or neither and the HIP error cleared
template <class T>
static bool alloc_pair(T **dev, size_t dev_bytes, T **pin, size_t pin_bytes)
{
    T *d = nullptr, *p = nullptr;
    if (hipMalloc((void **)&d, dev_bytes) != hipSuccess || hipHostMalloc((void **)&p, pin_bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        if (d) hipFree(d);
        return false;
    }
    *dev = d;
    *pin = p;
    return true;
}

// the handle's saturation counter, made (and zeroed on `st`) at the first pass that may count
static int ensure_sat_counter(gal_synth *h, hipStream_t st)
{
    if (h->d_iq_sat) return GAL_OK;
    unsigned long long *c = nullptr;
    HIP_TRY(hipMalloc((void **)&c, sizeof(unsigned long long)));
    const hipError_t err = hipMemsetAsync(c, 0, sizeof(unsigned long long), st);
    if (err != hipSuccess) {  // (never keep a counter that was not zeroed)
        hipFree(c);
        return fail(GAL_E_DEVICE, "hipMemsetAsync of the saturation counter failed: %s", hipGetErrorString(err));
    }
    h->d_iq_sat = c;
    return GAL_OK;
}

// The first device calls of an entry point, behind its validation: the handle's device and stream (*st), and, for a pass that counts,
// the saturation counter.
static int enter(gal_synth *h, hipStream_t *st, bool counts = true)
{
    HIP_TRY(hipSetDevice(h->device));
    *st = handle_stream(h);
    if (!*st) return fail(GAL_E_DEVICE, "hipStreamCreate failed");
    return counts ? ensure_sat_counter(h, *st) : GAL_OK;
}

// The three checks of a device buffer, `who` in the messages.
static int check_aligned(const char *who, const void *p, int part = -1)
{
    if (p && !((uintptr_t)p & 15)) return GAL_OK;
    if (part < 0) return fail(GAL_E_INVAL, "%s: device pointers must be non-null and 16-byte aligned", who);
    return fail(GAL_E_INVAL, "%s: device pointers must be non-null and 16-byte aligned (part %d)", who, part);
}

static bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    const char *x = (const char *)a, *o = (const char *)b;
    return x < o + b_bytes && o < x + a_bytes;
}

// in_place_ok: exactly in place (out == in) is no overlap; `why` ends the message
static int check_overlap(const char *who, const void *in, size_t in_bytes, const void *out, size_t out_bytes, bool in_place_ok, const char *why)
{
    if (in_place_ok && in == out) return GAL_OK;
    if (ranges_overlap(in, in_bytes, out, out_bytes)) return fail(GAL_E_INVAL, "%s: input and output overlap%s", who, why);
    return GAL_OK;
}

// what: "input of", "output of", ...
static int check_in_flight(const char *who, const gal_synth *h, const void *p, size_t bytes, const char *what)
{
    if (hits_batch_in_flight(h, p, bytes)) return fail(GAL_E_STATE, "%s: %s the batch in flight (call gal_synth_finish first)", who, what);
    return GAL_OK;
}

#define GAL_TRY(expr)                 \
    do {                              \
        const int rc__ = (expr);      \
        if (rc__) return rc__;        \
    } while (0)

extern "C" {

// ---- output formats, noise floor, interference sources (iq_pass.hip) ---------------------------------------------------------------
size_t gal_synth_iq_bytes(int32_t format, size_t n_samples)
{
    switch (format) {
    case GAL_IQ_ISHORT: return 4 * n_samples;
    case GAL_IQ_IBYTE: return 2 * n_samples;
    case GAL_IQ_IBIT: return (n_samples + 3) / 4;
    default: return 0;
    }
}

// The one check path of the three conversions below, `who` in the messages.  in_place: ishort may run with out_dev == iq_dev (every
// lane rewrites the vector it has read); otherwise any overlap would race (ibyte: lane i writes where lane i / 2 reads), and the
// kernels take both as __restrict__.
static int iq_pass(const char *who, bool in_place, gal_synth_t *h, const int16_t *iq_dev, size_t n_samples, uint64_t first_sample,
                   const gal_iq_noise_t *noise, const gal_iq_interf_t *interf, int32_t n_interf, int32_t format, int32_t shift, void *out_dev)
{
    if (!h) return fail(GAL_E_INVAL, "null handle");
    gal_iq_interf_t src[GAL_INTERF_MAX];  // the caller's array is not looked at again
    if (n_interf > 0) {
        if (!interf) return fail(GAL_E_INVAL, "%s: null interf with n_interf %d", who, n_interf);
        memcpy(src, interf, (size_t)n_interf * sizeof(gal_iq_interf_t));
    }
    for (int k = 0; k < n_interf; ++k) {
        const gal_iq_interf_t &c = src[k];
        if (c.amp_q4 > (1u << 20) || (c.sweep_len == 0 && c.df != 0) || c.pulse_on > c.pulse_period || c.reserved != 0)
            return fail(GAL_E_INVAL, "%s: source %d: amp_q4 %u (0..2^20), df %d with sweep_len %u (0 without a sweep), "
                        "pulse_on %u of pulse_period %u, reserved %u (0)", who, k, c.amp_q4, c.df, c.sweep_len, c.pulse_on, c.pulse_period, c.reserved);
    }
    if (format != GAL_IQ_ISHORT && format != GAL_IQ_IBYTE && format != GAL_IQ_IBIT)
        return fail(GAL_E_INVAL, "%s: unknown format %d (GAL_IQ_ISHORT 0, GAL_IQ_IBYTE 1, GAL_IQ_IBIT 2)", who, format);
    if (format == GAL_IQ_IBYTE ? (shift < 0 || shift > 15) : shift != 0)
        return fail(GAL_E_INVAL, "%s: shift %d (0..15 for GAL_IQ_IBYTE, 0 otherwise)", who, shift);
    if (noise && (noise->gain_q16 > (1u << 20) || noise->sigma_q4 > (1u << 20) || noise->reserved != 0))
        return fail(GAL_E_INVAL, "%s: gain_q16 %u, sigma_q4 %u (both 0..2^20), reserved %u (0)", who, noise->gain_q16, noise->sigma_q4,
                    noise->reserved);
    if (first_sample >> 62) return fail(GAL_E_INVAL, "%s: first_sample must be below 2^62", who);
    GAL_TRY(check_aligned(who, iq_dev));
    GAL_TRY(check_aligned(who, out_dev));
    if (n_samples == 0) return GAL_OK;
    GAL_TRY(check_overlap(who, iq_dev, 4 * n_samples, out_dev, gal_synth_iq_bytes(format, n_samples), in_place && format == GAL_IQ_ISHORT,
                          in_place ? " (only ishort exactly in place may)" : ""));
    GAL_TRY(check_in_flight(who, h, iq_dev, 4 * n_samples, "input of"));
    const bool copy = format == GAL_IQ_ISHORT && !noise && n_interf == 0;  // nothing to mix (and nothing to count)
    hipStream_t st;
    GAL_TRY(enter(h, &st, !copy));
    if (copy) {
        HIP_TRY(hipMemcpyAsync(out_dev, iq_dev, 4 * n_samples, hipMemcpyDeviceToDevice, st));
        return GAL_OK;
    }
    HIP_TRY(galk_launch_iq_pass(format, iq_dev, 2 * (uint64_t)n_samples, first_sample, noise, src, n_interf, shift, out_dev, h->d_iq_sat, st));
    return GAL_OK;
}

int gal_synth_iq_convert(gal_synth_t *h, const int16_t *iq_dev, size_t n_samples, int32_t format, int32_t shift, void *out_dev)
{
    return iq_pass("gal_synth_iq_convert", false, h, iq_dev, n_samples, 0, nullptr, nullptr, 0, format, shift, out_dev);
}

// ---- noise floor ---------------------------------------------------------------------------------------------------------------
int gal_synth_iq_convert_noise(gal_synth_t *h, const int16_t *iq_dev, size_t n_samples, uint64_t first_sample, const gal_iq_noise_t *noise,
                               int32_t format, int32_t shift, void *out_dev)
{
    if (!noise) return gal_synth_iq_convert(h, iq_dev, n_samples, format, shift, out_dev);
    return iq_pass("gal_synth_iq_convert_noise", true, h, iq_dev, n_samples, first_sample, noise, nullptr, 0, format, shift, out_dev);
}

int gal_synth_noise_from_cn0(double cn0_dbhz, double sample_rate, double gain, gal_iq_noise_t *out)
{
    if (!out) return fail(GAL_E_INVAL, "gal_synth_noise_from_cn0: null argument");
    if (!std::isfinite(cn0_dbhz) || !std::isfinite(sample_rate) || !std::isfinite(gain) || sample_rate <= 0.0 || gain < 0.0 || gain > 16.0)
        return fail(GAL_E_INVAL, "gal_synth_noise_from_cn0: C/N0 %g dB-Hz, sample rate %g Hz (> 0), gain %g (0..16)", cn0_dbhz, sample_rate, gain);
    // sigma of one rail in int16 LSB for a composite E1B + E1C signal of amplitude 250 per component (include/galsynth.h)
    const double sigma_q4 = 16.0 * 250.0 * gain * sqrt(sample_rate / pow(10.0, cn0_dbhz / 10.0));
    if (!(sigma_q4 <= 1048576.0))
        return fail(GAL_E_INVAL, "gal_synth_noise_from_cn0: sigma %g LSB at %g dB-Hz is beyond the 65536 LSB sigma_q4 holds", sigma_q4 / 16.0, cn0_dbhz);
    memset(out, 0, sizeof(*out));
    out->gain_q16 = (uint32_t)llround(gain * 65536.0);
    out->sigma_q4 = (uint32_t)llround(sigma_q4);
    return GAL_OK;
}

// ---- interference sources ------------------------------------------------------------------------------------------------------
int gal_synth_iq_convert_interf(gal_synth_t *h, const int16_t *iq_dev, size_t n_samples, uint64_t first_sample, const gal_iq_noise_t *noise,
                                const gal_iq_interf_t *interf, int32_t n_interf, int32_t format, int32_t shift, void *out_dev)
{
    if (n_interf < 0 || n_interf > GAL_INTERF_MAX)
        return fail(GAL_E_INVAL, "gal_synth_iq_convert_interf: n_interf %d (0..%d)", n_interf, GAL_INTERF_MAX);
    if (n_interf == 0) return gal_synth_iq_convert_noise(h, iq_dev, n_samples, first_sample, noise, format, shift, out_dev);
    return iq_pass("gal_synth_iq_convert_interf", true, h, iq_dev, n_samples, first_sample, noise, interf, n_interf, format, shift, out_dev);
}

int gal_synth_interf_make(double js_db, double gain, double sample_rate, double f_lo_hz, double f_hi_hz, double sweep_s, double pulse_period_s,
                          double pulse_on_s, gal_iq_interf_t *out)
{
    if (!out) return fail(GAL_E_INVAL, "gal_synth_interf_make: null argument");
    if (!std::isfinite(js_db) || !std::isfinite(gain) || !std::isfinite(sample_rate) || !std::isfinite(f_lo_hz) || !std::isfinite(sweep_s) ||
        !std::isfinite(pulse_period_s) || !std::isfinite(pulse_on_s) || (sweep_s != 0.0 && !std::isfinite(f_hi_hz)))
        return fail(GAL_E_INVAL, "gal_synth_interf_make: an argument is not finite");
    if (sample_rate <= 0.0 || gain < 0.0 || sweep_s < 0.0 || pulse_period_s < 0.0 || pulse_on_s < 0.0)
        return fail(GAL_E_INVAL, "gal_synth_interf_make: sample rate %g Hz (> 0), gain %g, sweep %g s, pulse %g of %g s (all >= 0)", sample_rate, gain,
                    sweep_s, pulse_on_s, pulse_period_s);
    // a tone A e^(j theta) has the power A^2, the composite signal of one satellite 2 (250 gain)^2 (include/galsynth.h)
    const double amp_q4 = 16.0 * 250.0 * sqrt(2.0) * gain * pow(10.0, js_db / 20.0);
    if (!(amp_q4 <= 1048576.0))
        return fail(GAL_E_INVAL, "gal_synth_interf_make: amplitude %g LSB at J/S %g dB is beyond the 65536 LSB amp_q4 holds", amp_q4 / 16.0, js_db);
    const double half = sample_rate / 2.0;
    if (!(fabs(f_lo_hz) < half) || (sweep_s != 0.0 && !(fabs(f_hi_hz) < half)))
        return fail(GAL_E_INVAL, "gal_synth_interf_make: frequencies %g, %g Hz must lie inside +-%g Hz", f_lo_hz, f_hi_hz, half);
    const double len = sweep_s * sample_rate, period = pulse_period_s * sample_rate, on = pulse_on_s * sample_rate;
    if (!(len < 4294967295.5) || !(period < 4294967295.5) || !(on < 4294967295.5))
        return fail(GAL_E_INVAL, "gal_synth_interf_make: sweep %g, pulse period %g, pulse on %g samples do not fit 32 bits", len, period, on);
    gal_iq_interf_t c;
    memset(&c, 0, sizeof(c));
    c.amp_q4 = (uint32_t)llround(amp_q4);
    const long long f0 = llround(f_lo_hz / sample_rate * 4294967296.0);
    long long df = 0;
    if (sweep_s != 0.0) {
        c.sweep_len = (uint32_t)llround(len);
        if (c.sweep_len < 1) return fail(GAL_E_INVAL, "gal_synth_interf_make: a sweep of %g s is less than one sample", sweep_s);
        df = llround((f_hi_hz - f_lo_hz) / sample_rate * 4294967296.0 / (double)c.sweep_len);
    }
    if (f0 < INT32_MIN || f0 > INT32_MAX || df < INT32_MIN || df > INT32_MAX)  // (a frequency that rounds to sample_rate / 2 itself)
        return fail(GAL_E_INVAL, "gal_synth_interf_make: phase step %lld, increment %lld per sample do not fit 32 bits", f0, df);
    c.f0 = (int32_t)f0;
    c.df = (int32_t)df;
    c.pulse_period = (uint32_t)llround(period);
    c.pulse_on = (uint32_t)llround(on);
    if (c.pulse_on > c.pulse_period)
        return fail(GAL_E_INVAL, "gal_synth_interf_make: pulse on %u of a period of %u samples", c.pulse_on, c.pulse_period);
    *out = c;
    return GAL_OK;
}

int gal_synth_iq_saturated(gal_synth_t *h, uint64_t *n_saturated, int32_t reset)
{
    if (!h || !n_saturated) return fail(GAL_E_INVAL, "gal_synth_iq_saturated: null argument");
    *n_saturated = 0;
    hipStream_t st;
    GAL_TRY(enter(h, &st, false));
    if (!h->d_iq_sat) {  // no ibyte conversion yet (the counter is made by the first): still the fence for ibit / ishort conversions
        HIP_TRY(hipStreamSynchronize(st));
        return GAL_OK;
    }
    unsigned long long v = 0;
    HIP_TRY(hipMemcpyAsync(&v, h->d_iq_sat, sizeof(v), hipMemcpyDeviceToHost, st));
    if (reset) HIP_TRY(hipMemsetAsync(h->d_iq_sat, 0, sizeof(v), st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_saturated = (uint64_t)v;
    return GAL_OK;
}


// ---- per-satellite signal power (iq_gain.hip) --------------------------------------------------------------------------------------
int gal_synth_gain_q7(double d_m, double elev_rad, const double *pattern_db, double offset_db, uint16_t *out)
{
    if (!out) return fail(GAL_E_INVAL, "gal_synth_gain_q7: null argument");
    bool ok = std::isfinite(d_m) && d_m > 0.0 && std::isfinite(elev_rad) && std::isfinite(offset_db);
    for (int i = 0; pattern_db && ok && i < GAL_GAIN_PATTERN_LEN; ++i) ok = std::isfinite(pattern_db[i]);
    if (!ok)
        return fail(GAL_E_INVAL, "gal_synth_gain_q7: distance %g m (> 0), elevation %g rad, offset %g dB and the pattern must be finite", d_m,
                    elev_rad, offset_db);
    *out = (uint16_t)gal_gain_q7_eval(d_m, elev_rad, pattern_db, offset_db);
    return GAL_OK;
}

// the parts of a weighted sum and its output, `bytes` each
static int check_parts(const char *who, const gal_synth *h, const int16_t *const *parts_dev, int n_parts, const int16_t *out_dev, size_t bytes)
{
    for (int k = 0; k < n_parts; ++k) {
        GAL_TRY(check_aligned(who, parts_dev[k], k));
        if (ranges_overlap(parts_dev[k], bytes, out_dev, bytes)) return fail(GAL_E_INVAL, "%s: part %d and the output overlap", who, k);
        GAL_TRY(check_in_flight(who, h, parts_dev[k], bytes, "input of"));
    }
    return check_in_flight(who, h, out_dev, bytes, "output of");
}

int gal_synth_iq_wsum(gal_synth_t *h, const int16_t *const *parts_dev, int32_t n_parts, const uint16_t *gain_q7, int32_t n_epochs,
                      int16_t *out_dev)
{
    const char *who = "gal_synth_iq_wsum";
    if (!h) return fail(GAL_E_INVAL, "null handle");
    if (!parts_dev || !gain_q7 || n_parts < 1 || n_parts > GAL_ENGINE_MAX_CHAN || n_epochs < 1)
        return fail(GAL_E_INVAL, "%s: null argument, n_parts %d (1..%d) or n_epochs %d (>= 1)", who, n_parts, GAL_ENGINE_MAX_CHAN, n_epochs);
    GAL_TRY(check_aligned(who, out_dev));
    const size_t bytes = (size_t)n_epochs * (size_t)h->cfg.samples_per_epoch * 4;
    GAL_TRY(check_parts(who, h, parts_dev, n_parts, out_dev, bytes));
    uint64_t row_max = 0;  // the largest sum of one epoch's gains: what w needs (iq_gain.hip)
    for (int e = 0; e < n_epochs; ++e) {
        uint64_t row = 0;
        for (int k = 0; k < n_parts; ++k) {
            const uint16_t g = gain_q7[(size_t)e * n_parts + k];
            if (g > GAL_GAIN_MAX) return fail(GAL_E_INVAL, "%s: gain %u of epoch %d, part %d (0..%d)", who, g, e, k, GAL_GAIN_MAX);
            row += g;
        }
        row_max = std::max(row_max, row);
    }
    hipStream_t st;
    GAL_TRY(enter(h, &st));
    // the table of this call: pointers, then gains.  One of each per handle: a call waits for the kernel of the call before it
    HIP_TRY(h->gain.sync.wait());
    const size_t o_gain = sizeof(void *) * GAL_ENGINE_MAX_CHAN, need = o_gain + (size_t)n_epochs * n_parts * sizeof(int);
    uint64_t cap = 0;
    const int rc = h->gain.table.reserve(need, 0, true, h->gain.sync, &cap);
    if (rc == GAL_E_NOMEM) return fail(GAL_E_NOMEM, "%s: the gain table of %zu bytes could not be allocated", who, (size_t)cap);
    if (rc) return rc;
    memset(h->gain.table.host, 0, o_gain);
    memcpy(h->gain.table.host, parts_dev, sizeof(void *) * (size_t)n_parts);
    int *const hg = (int *)(h->gain.table.host + o_gain);
    for (size_t i = 0; i < (size_t)n_epochs * n_parts; ++i) hg[i] = gain_q7[i];
    HIP_TRY(hipMemcpyAsync(h->gain.table.dev, h->gain.table.host, need, hipMemcpyHostToDevice, st));
    HIP_TRY(galk_launch_iq_wsum((const int16_t *const *)h->gain.table.dev, (const int *)(h->gain.table.dev + o_gain), n_parts, n_epochs, h->cfg.samples_per_epoch,
                                row_max > 65535 ? 1 : 0, out_dev, h->d_iq_sat, st));
    HIP_TRY(h->gain.sync.mark(st));
    return GAL_OK;
}

// ---- per-satellite multipath (iq_echo.hip) ----------------------------------------------------------------------------------------
int gal_synth_mpath_check(const gal_iq_echo_t *echo_rows, int32_t n_echo, int32_t n_epochs, const int32_t *part_of_echo, int32_t n_parts)
{
    const char *who = "gal_synth_mpath_check";
    if (n_echo < 0 || n_echo > GAL_ECHO_MAX) return fail(GAL_E_INVAL, "%s: %d echoes (0..%d)", who, n_echo, GAL_ECHO_MAX);
    if (n_epochs < 1 || n_parts < 1 || n_parts > GAL_ENGINE_MAX_CHAN)
        return fail(GAL_E_INVAL, "%s: n_epochs %d (>= 1) or n_parts %d (1..%d)", who, n_epochs, n_parts, GAL_ENGINE_MAX_CHAN);
    if (n_echo == 0) return GAL_OK;
    if (!echo_rows || !part_of_echo) return fail(GAL_E_INVAL, "%s: null argument", who);
    for (int r = 0; r < n_echo; ++r)
        if (part_of_echo[r] < 0 || part_of_echo[r] >= n_parts)
            return fail(GAL_E_INVAL, "%s: echo %d on part %d (0..%d)", who, r, part_of_echo[r], n_parts - 1);
    for (int e = 0; e < n_epochs; ++e)
        for (int r = 0; r < n_echo; ++r) {
            const gal_iq_echo_t &q = echo_rows[(size_t)e * n_echo + r];
            if (q.gain_q7 > GAL_GAIN_MAX) return fail(GAL_E_INVAL, "%s: gain %u of epoch %d, echo %d (0..%d)", who, q.gain_q7, e, r, GAL_GAIN_MAX);
            if (q.delay > GAL_ECHO_MAX_DELAY)
                return fail(GAL_E_INVAL, "%s: delay %u of epoch %d, echo %d (0..%d samples)", who, q.delay, e, r, GAL_ECHO_MAX_DELAY);
            if (q.reserved != 0) return fail(GAL_E_INVAL, "%s: reserved = %u in epoch %d, echo %d (must be 0)", who, q.reserved, e, r);
        }
    return GAL_OK;
}

static bool mpath_echo_ok(const gal_mpath_echo_t *q) { return q->delay <= GAL_ECHO_MAX_DELAY && q->alpha_q12 <= 8192; }

int gal_synth_mpath_make(double delay_s, double rel_db, double phase_deg, double fade_hz, double sample_rate, gal_mpath_echo_t *out)
{
    const char *who = "gal_synth_mpath_make";
    if (!out) return fail(GAL_E_INVAL, "%s: null argument", who);
    if (!std::isfinite(delay_s) || !std::isfinite(rel_db) || !std::isfinite(phase_deg) || !std::isfinite(fade_hz) || !std::isfinite(sample_rate) ||
        sample_rate <= 0.0 || delay_s < 0.0)
        return fail(GAL_E_INVAL, "%s: delay %g s (>= 0), %g dB, %g deg, %g Hz and the rate %g Hz (> 0) must be finite", who, delay_s, rel_db,
                    phase_deg, fade_hz, sample_rate);
    const double d = delay_s * sample_rate;
    if (d > GAL_ECHO_MAX_DELAY + 0.5) return fail(GAL_E_INVAL, "%s: a delay of %g samples, more than %d", who, d, GAL_ECHO_MAX_DELAY);
    const long long delay = llround(d);
    if (delay > GAL_ECHO_MAX_DELAY) return fail(GAL_E_INVAL, "%s: a delay of %lld samples, more than %d", who, delay, GAL_ECHO_MAX_DELAY);
    const double a = 4096.0 * pow(10.0, rel_db / 20.0);
    if (!(a <= 8192.0)) return fail(GAL_E_INVAL, "%s: %g dB is an amplitude of %g, more than 2 (+6.02 dB)", who, rel_db, a / 4096.0);
    const double turns = phase_deg / 360.0;
    const long long ph0 = llround((turns - floor(turns)) * 4294967296.0);
    const double step = fade_hz / sample_rate * 4294967296.0;
    if (!(fabs(step) < 2147483647.5)) return fail(GAL_E_INVAL, "%s: a fading rate of %g Hz must lie inside +-sample_rate / 2", who, fade_hz);
    const long long dph = llround(step);
    if (dph < INT32_MIN || dph > INT32_MAX) return fail(GAL_E_INVAL, "%s: a fading rate of %g Hz must lie inside +-sample_rate / 2", who, fade_hz);
    out->delay = (uint32_t)delay;
    out->alpha_q12 = (uint32_t)llround(a);
    out->ph0 = (uint32_t)(ph0 & 0xffffffffll);
    out->dph = (int32_t)dph;
    return GAL_OK;
}

int gal_synth_mpath_row(const gal_mpath_echo_t *echo, uint16_t slot_gain_q7, uint64_t epoch, int32_t samples_per_epoch, gal_iq_echo_t *row)
{
    const char *who = "gal_synth_mpath_row";
    if (!echo || !row) return fail(GAL_E_INVAL, "%s: null argument", who);
    if (samples_per_epoch < 1 || slot_gain_q7 > GAL_GAIN_MAX || !mpath_echo_ok(echo))
        return fail(GAL_E_INVAL, "%s: samples_per_epoch %d (>= 1), gain %u (0..%d), delay %u (0..%d) or alpha_q12 %u (0..8192)", who,
                    samples_per_epoch, slot_gain_q7, GAL_GAIN_MAX, echo->delay, GAL_ECHO_MAX_DELAY, echo->alpha_q12);
    const uint32_t A = ((uint32_t)slot_gain_q7 * echo->alpha_q12 + 2048u) >> 12;
    row->gain_q7 = (uint16_t)std::min<uint32_t>(A, GAL_GAIN_MAX);
    row->delay = (uint16_t)echo->delay;
    row->ph0 = echo->ph0 + (uint32_t)epoch * (uint32_t)samples_per_epoch * (uint32_t)echo->dph;  // (exact modulo 2^32)
    row->dph = echo->dph;
    row->reserved = 0;
    return GAL_OK;
}

static constexpr size_t kMpLineWords = GAL_ECHO_MAX_DELAY;                          // one history line: complex samples = uint32
static constexpr size_t kMpHistBytes = sizeof(uint32_t) * kMpLineWords * 2 * GAL_ECHO_LINES;  // two buffers per line

int gal_synth_mpath_reset(gal_synth_t *h)
{
    if (!h) return fail(GAL_E_INVAL, "null handle");
    if (!h->mp.d_hist) return GAL_OK;  // (the lines are made zeroed)
    hipStream_t st;
    GAL_TRY(enter(h, &st, false));
    HIP_TRY(h->mp.sync.wait());  // (whatever stream the last call ran on)
    HIP_TRY(hipMemsetAsync(h->mp.d_hist, 0, kMpHistBytes, st));
    return GAL_OK;
}

// gal_synth_iq_mpath (refl false: the rows are gal_iq_echo_t, which a gal_iq_refl_t with frac_q12 = 0 equals byte for byte; k_iq_echo)
// and gal_synth_iq_refl (refl true; k_iq_refl) over the one table and the one set of history lines of h->mp
static int echo_pass(const char *who, bool refl, gal_synth_t *h, const int16_t *const *parts_dev, int32_t n_parts, const int32_t *hist_id,
                     const uint16_t *gain_q7, int32_t n_epochs, const int32_t *part_of_echo, const gal_iq_refl_t *echo_rows, int32_t n_echo,
                     int16_t *out_dev)
{
    static_assert(sizeof(gal_iq_refl_t) == sizeof(gal_iq_echo_t) && offsetof(gal_iq_refl_t, frac_q12) == offsetof(gal_iq_echo_t, reserved),
                  "an echo row is a reflector row with frac_q12 = 0");
    if (!h) return fail(GAL_E_INVAL, "null handle");
    if (!parts_dev || !gain_q7 || n_parts < 1 || n_parts > GAL_ENGINE_MAX_CHAN || n_epochs < 1)
        return fail(GAL_E_INVAL, "%s: null argument, n_parts %d (1..%d) or n_epochs %d (>= 1)", who, n_parts, GAL_ENGINE_MAX_CHAN, n_epochs);
    GAL_TRY(check_aligned(who, out_dev));
    int rc = refl ? gal_synth_refl_check(echo_rows, n_echo, n_epochs, part_of_echo, n_parts)
                  : gal_synth_mpath_check((const gal_iq_echo_t *)echo_rows, n_echo, n_epochs, part_of_echo, n_parts);
    if (rc) return rc;
    const size_t bytes = (size_t)n_epochs * (size_t)h->cfg.samples_per_epoch * 4;
    GAL_TRY(check_parts(who, h, parts_dev, n_parts, out_dev, bytes));
    int id[GAL_ENGINE_MAX_CHAN];
    uint64_t named = 0;  // the lines this call names
    for (int k = 0; k < n_parts; ++k) {
        id[k] = hist_id ? hist_id[k] : k;
        if (id[k] < -1 || id[k] >= GAL_ECHO_LINES) return fail(GAL_E_INVAL, "%s: hist_id %d of part %d (-1..%d)", who, id[k], k, GAL_ECHO_LINES - 1);
        if (id[k] < 0) continue;
        if (named >> id[k] & 1) return fail(GAL_E_INVAL, "%s: history line %d is named by two parts", who, id[k]);
        named |= (uint64_t)1 << id[k];
    }
    for (int r = 0; r < n_echo; ++r)
        if (id[part_of_echo[r]] < 0) return fail(GAL_E_INVAL, "%s: echo %d repeats part %d, which has no history line (hist_id -1)", who, r, part_of_echo[r]);
    uint64_t row_max = 0;  // the largest of sum g + 2 sum A over the epochs: what w needs (iq_echo.hip)
    for (int e = 0; e < n_epochs; ++e) {
        uint64_t row = 0;
        for (int k = 0; k < n_parts; ++k) {
            const uint16_t g = gain_q7[(size_t)e * n_parts + k];
            if (g > GAL_GAIN_MAX) return fail(GAL_E_INVAL, "%s: gain %u of epoch %d, part %d (0..%d)", who, g, e, k, GAL_GAIN_MAX);
            row += g;
        }
        for (int r = 0; r < n_echo; ++r) row += 2 * (uint64_t)echo_rows[(size_t)e * n_echo + r].gain_q7;
        row_max = std::max(row_max, row);
    }
    hipStream_t st;
    GAL_TRY(enter(h, &st));
    HIP_TRY(h->mp.sync.wait());  // one table per handle: the call before has read it
    if (!h->mp.d_hist) {
        if (hipMalloc((void **)&h->mp.d_hist, kMpHistBytes) != hipSuccess) {
            (void)hipGetLastError();
            h->mp.d_hist = nullptr;
            return fail(GAL_E_NOMEM, "%s: the history lines of %zu bytes could not be allocated", who, kMpHistBytes);
        }
        HIP_TRY(hipMemsetAsync(h->mp.d_hist, 0, kMpHistBytes, st));
        memset(h->mp.cur, 0, sizeof(h->mp.cur));
    }
    // the table of this call: part pointers, history-in and history-out pointers, gains, echo rows, part indices
    const size_t o_hin = sizeof(void *) * GAL_ENGINE_MAX_CHAN, o_hout = 2 * o_hin, o_gain = 3 * o_hin;
    const size_t o_rows = align_up(o_gain + (size_t)n_epochs * n_parts * sizeof(int), 16);
    const size_t o_pof = o_rows + (size_t)n_epochs * n_echo * sizeof(gal_iq_echo_t), need = o_pof + sizeof(int) * GAL_ECHO_MAX;
    uint64_t cap = 0;
    rc = h->mp.table.reserve(need, 0, true, h->mp.sync, &cap);
    if (rc == GAL_E_NOMEM) return fail(GAL_E_NOMEM, "%s: the table of %zu bytes could not be allocated", who, (size_t)cap);
    if (rc) return rc;
    memset(h->mp.table.host, 0, o_gain);
    memcpy(h->mp.table.host, parts_dev, sizeof(void *) * (size_t)n_parts);
    uint32_t **const hin = (uint32_t **)(h->mp.table.host + o_hin), **const hout = (uint32_t **)(h->mp.table.host + o_hout);
    for (int k = 0; k < n_parts; ++k) {
        if (id[k] < 0) continue;
        uint32_t *const line = h->mp.d_hist + (size_t)id[k] * 2 * kMpLineWords;
        hin[k] = line + h->mp.cur[id[k]] * kMpLineWords;
        hout[k] = line + (h->mp.cur[id[k]] ^ 1) * kMpLineWords;
    }
    int *const hg = (int *)(h->mp.table.host + o_gain);
    for (size_t i = 0; i < (size_t)n_epochs * n_parts; ++i) hg[i] = gain_q7[i];
    if (n_echo > 0) {
        memcpy(h->mp.table.host + o_rows, echo_rows, (size_t)n_epochs * n_echo * sizeof(gal_iq_echo_t));
        memcpy(h->mp.table.host + o_pof, part_of_echo, sizeof(int) * (size_t)n_echo);
    }
    HIP_TRY(hipMemcpyAsync(h->mp.table.dev, h->mp.table.host, need, hipMemcpyHostToDevice, st));
    const auto launch = refl ? galk_launch_iq_refl : galk_launch_iq_echo;
    HIP_TRY(launch((const int16_t *const *)h->mp.table.dev, (const int16_t *const *)(h->mp.table.dev + o_hin), (int16_t *const *)(h->mp.table.dev + o_hout),
                   (const int *)(h->mp.table.dev + o_gain), h->mp.table.dev + o_rows, (const int *)(h->mp.table.dev + o_pof), n_parts, n_echo, n_epochs,
                   h->cfg.samples_per_epoch, row_max > 65535 ? 1 : 0, out_dev, h->d_iq_sat, st));
    for (int k = 0; k < n_parts; ++k)
        if (id[k] >= 0) h->mp.cur[id[k]] ^= 1;
    HIP_TRY(h->mp.sync.mark(st));
    return GAL_OK;
}

int gal_synth_iq_mpath(gal_synth_t *h, const int16_t *const *parts_dev, int32_t n_parts, const int32_t *hist_id, const uint16_t *gain_q7,
                       int32_t n_epochs, const int32_t *part_of_echo, const gal_iq_echo_t *echo_rows, int32_t n_echo, int16_t *out_dev)
{
    return echo_pass("gal_synth_iq_mpath", false, h, parts_dev, n_parts, hist_id, gain_q7, n_epochs, part_of_echo, (const gal_iq_refl_t *)echo_rows,
                     n_echo, out_dev);
}

// ---- geometric reflectors (iq_refl.hip) ---------------------------------------------------------------------------------------------
int gal_synth_refl_check(const gal_iq_refl_t *refl_rows, int32_t n_echo, int32_t n_epochs, const int32_t *part_of_echo, int32_t n_parts)
{
    const char *who = "gal_synth_refl_check";
    if (n_echo < 0 || n_echo > GAL_ECHO_MAX) return fail(GAL_E_INVAL, "%s: %d echoes (0..%d)", who, n_echo, GAL_ECHO_MAX);
    if (n_epochs < 1 || n_parts < 1 || n_parts > GAL_ENGINE_MAX_CHAN)
        return fail(GAL_E_INVAL, "%s: n_epochs %d (>= 1) or n_parts %d (1..%d)", who, n_epochs, n_parts, GAL_ENGINE_MAX_CHAN);
    if (n_echo == 0) return GAL_OK;
    if (!refl_rows || !part_of_echo) return fail(GAL_E_INVAL, "%s: null argument", who);
    for (int r = 0; r < n_echo; ++r)
        if (part_of_echo[r] < 0 || part_of_echo[r] >= n_parts)
            return fail(GAL_E_INVAL, "%s: echo %d on part %d (0..%d)", who, r, part_of_echo[r], n_parts - 1);
    for (int e = 0; e < n_epochs; ++e)
        for (int r = 0; r < n_echo; ++r) {
            const gal_iq_refl_t &q = refl_rows[(size_t)e * n_echo + r];
            if (q.gain_q7 > GAL_GAIN_MAX) return fail(GAL_E_INVAL, "%s: gain %u of epoch %d, echo %d (0..%d)", who, q.gain_q7, e, r, GAL_GAIN_MAX);
            if (q.frac_q12 > 4095) return fail(GAL_E_INVAL, "%s: frac_q12 %u of epoch %d, echo %d (0..4095)", who, q.frac_q12, e, r);
            if (q.delay + (q.frac_q12 > 0 ? 1 : 0) > GAL_ECHO_MAX_DELAY)
                return fail(GAL_E_INVAL, "%s: delay %u + %u/4096 of epoch %d, echo %d (the oldest sample read may lie %d samples back)", who, q.delay,
                            q.frac_q12, e, r, GAL_ECHO_MAX_DELAY);
            if (q.reserved != 0) return fail(GAL_E_INVAL, "%s: reserved = %u in epoch %d, echo %d (must be 0)", who, q.reserved, e, r);
        }
    return GAL_OK;
}

int gal_synth_iq_refl(gal_synth_t *h, const int16_t *const *parts_dev, int32_t n_parts, const int32_t *hist_id, const uint16_t *gain_q7,
                      int32_t n_epochs, const int32_t *part_of_echo, const gal_iq_refl_t *refl_rows, int32_t n_echo, int16_t *out_dev)
{
    return echo_pass("gal_synth_iq_refl", true, h, parts_dev, n_parts, hist_id, gain_q7, n_epochs, part_of_echo, refl_rows, n_echo, out_dev);
}

int gal_synth_refl_geom(int32_t kind, const double *p, double az_rad, double el_rad, double *excess_m)
{
    const char *who = "gal_synth_refl_geom";
    if (!p || !excess_m) return fail(GAL_E_INVAL, "%s: null argument", who);
    if (kind != GAL_REFL_GROUND && kind != GAL_REFL_WALL) return fail(GAL_E_INVAL, "%s: kind %d (GAL_REFL_GROUND, GAL_REFL_WALL)", who, kind);
    if (!std::isfinite(az_rad) || !std::isfinite(el_rad) || !std::isfinite(p[0]) || p[0] < 0.0 || (kind == GAL_REFL_WALL && !std::isfinite(p[1])))
        return fail(GAL_E_INVAL, "%s: the angles and the plane must be finite, its height or distance %g m >= 0", who, p[0]);
    if (kind == GAL_REFL_GROUND) {
        *excess_m = el_rad > 0.0 ? 2.0 * p[0] * sin(el_rad) : -1.0;
    } else {
        const double x = -2.0 * p[0] * cos(el_rad) * cos(az_rad - p[1]);
        *excess_m = x > 0.0 ? x : -1.0;
    }
    return GAL_OK;
}

// P(x) of include/galsynth.h: the carrier phase of an echo with the excess path x, in 2^-32 cycles
static uint32_t refl_phase(double excess_m, double refl_phase_deg)
{
    const double lambda = 299792458.0 / 1575420000.0;
    const double cyc = -excess_m / lambda + refl_phase_deg / 360.0;
    return (uint32_t)(llround((cyc - floor(cyc)) * 4294967296.0) & 0xffffffffll);
}

int gal_synth_refl_row(double excess_now_m, double excess_next_m, double rel_db, double refl_phase_deg, double sample_rate,
                       int32_t samples_per_epoch, uint16_t slot_gain_q7, gal_iq_refl_t *row)
{
    const char *who = "gal_synth_refl_row";
    if (!row) return fail(GAL_E_INVAL, "%s: null argument", who);
    if (!std::isfinite(excess_now_m) || !std::isfinite(excess_next_m) || !std::isfinite(rel_db) || !std::isfinite(refl_phase_deg) ||
        !std::isfinite(sample_rate) || sample_rate <= 0.0 || samples_per_epoch < 1 || slot_gain_q7 > GAL_GAIN_MAX)
        return fail(GAL_E_INVAL, "%s: the paths %g and %g m, %g dB, %g deg and the rate %g Hz (> 0) must be finite, samples_per_epoch %d >= 1, gain %u in 0..%d",
                    who, excess_now_m, excess_next_m, rel_db, refl_phase_deg, sample_rate, samples_per_epoch, slot_gain_q7, GAL_GAIN_MAX);
    const double alpha = 4096.0 * pow(10.0, rel_db / 20.0);
    if (!(alpha <= 8192.0)) return fail(GAL_E_INVAL, "%s: %g dB is an amplitude of %g, more than 2 (+6.02 dB)", who, rel_db, alpha / 4096.0);
    memset(row, 0, sizeof(*row));
    if (excess_now_m < 0.0) return GAL_OK;  // no echo in this epoch
    const double t = excess_now_m / 299792458.0 * sample_rate;
    if (!(t < GAL_ECHO_MAX_DELAY + 1.0)) return fail(GAL_E_INVAL, "%s: a delay of %g samples, more than %d", who, t, GAL_ECHO_MAX_DELAY);
    long long D = (long long)floor(t), F = llround((t - (double)D) * 4096.0);
    if (F == 4096) D += 1, F = 0;
    if (D + (F > 0 ? 1 : 0) > GAL_ECHO_MAX_DELAY) return fail(GAL_E_INVAL, "%s: a delay of %g samples, more than %d", who, t, GAL_ECHO_MAX_DELAY);
    const uint32_t A = ((uint32_t)slot_gain_q7 * (uint32_t)llround(alpha) + 2048u) >> 12;
    row->gain_q7 = (uint16_t)std::min<uint32_t>(A, GAL_GAIN_MAX);
    row->delay = (uint16_t)D;
    row->frac_q12 = (uint16_t)F;
    row->ph0 = refl_phase(excess_now_m, refl_phase_deg);
    if (excess_next_m >= 0.0)
        row->dph = (int32_t)llround((double)(int32_t)(refl_phase(excess_next_m, refl_phase_deg) - row->ph0) / (double)samples_per_epoch);
    return GAL_OK;
}

// ---- front-end FIR filter (iq_fir.hip) ---------------------------------------------------------------------------------------------
static constexpr int kFirTableWords = 4 * 33;  // (GE, GO) x 2 pairs per trip, (128 / 2 + 1 + 1) / 2 trips at most
static constexpr int kFirHist = 128;           // complex samples of history, as iq_fir.hip keeps them

int gal_synth_fir_check(const int16_t *taps_q14, int32_t n_taps)
{
    if (!taps_q14) return fail(GAL_E_INVAL, "gal_synth_fir_check: null taps");
    if (n_taps < 1 || n_taps > GAL_FIR_MAX_TAPS) return fail(GAL_E_INVAL, "gal_synth_fir_check: %d taps (1..%d)", n_taps, GAL_FIR_MAX_TAPS);
    long sum = 0;
    for (int k = 0; k < n_taps; ++k) sum += std::abs((long)taps_q14[k]);
    if (sum > 65535)
        return fail(GAL_E_INVAL, "gal_synth_fir_check: the taps' absolute values sum to %ld, more than 65535 (16384 = 1.0): the int32 accumulator could wrap", sum);
    return GAL_OK;
}

// the Hamming-windowed sinc of both low-pass designers, as include/galsynth.h states it; `check` = the admission of the caller's filter
static int lowpass_design(const char *who, double cutoff_hz, double sample_rate, int32_t n_taps, int max_odd, int16_t *taps_q14)
{
    if (!taps_q14) return fail(GAL_E_INVAL, "%s: null taps", who);
    if (n_taps < 3 || n_taps > max_odd || !(n_taps & 1)) return fail(GAL_E_INVAL, "%s: %d taps (odd, 3..%d)", who, n_taps, max_odd);
    if (!std::isfinite(cutoff_hz) || !std::isfinite(sample_rate) || sample_rate <= 0.0 || !(cutoff_hz > 0.0) || !(cutoff_hz < sample_rate / 2))
        return fail(GAL_E_INVAL, "%s: cutoff %g Hz must lie inside (0, sample_rate / 2 = %g Hz)", who, cutoff_hz, sample_rate / 2);
    const double pi = 3.14159265358979323846, fc = cutoff_hz / sample_rate;
    const int M = n_taps - 1;
    double ws[GAL_FIRDEC_MAX_TAPS], S = 0.0;
    for (int k = 0; k <= M; ++k) {
        const double t = (double)(k - M / 2);
        const double s = k == M / 2 ? 2.0 * fc : sin(2.0 * pi * fc * t) / (pi * t);
        const double w = 0.54 - 0.46 * cos(2.0 * pi * (double)k / (double)M);
        ws[k] = w * s;
        S += ws[k];
    }
    if (!std::isfinite(S) || S == 0.0) return fail(GAL_E_INVAL, "%s: the window's sum is %g", who, S);
    long long q[GAL_FIRDEC_MAX_TAPS], sum = 0;
    for (int k = 0; k <= M; ++k) {
        q[k] = llround(16384.0 * ws[k] / S);
        sum += q[k];
    }
    q[M / 2] += 16384 - sum;
    int16_t out[GAL_FIRDEC_MAX_TAPS];
    long asum = 0;
    for (int k = 0; k <= M; ++k) {
        if (q[k] < -32768 || q[k] > 32767) return fail(GAL_E_INVAL, "%s: tap %d = %lld does not fit an int16", who, k, q[k]);
        out[k] = (int16_t)q[k];
        asum += std::abs((long)out[k]);
    }
    if (asum > 65535)
        return fail(GAL_E_INVAL, "%s: the taps' absolute values sum to %ld, more than 65535 (16384 = 1.0): the int32 accumulator could wrap", who, asum);
    memcpy(taps_q14, out, sizeof(int16_t) * (size_t)n_taps);
    return GAL_OK;
}

int gal_synth_fir_lowpass(double cutoff_hz, double sample_rate, int32_t n_taps, int16_t *taps_q14)
{
    return lowpass_design("gal_synth_fir_lowpass", cutoff_hz, sample_rate, n_taps, GAL_FIR_MAX_TAPS - 1, taps_q14);
}

int gal_synth_fir_set(gal_synth_t *h, const int16_t *taps_q14, int32_t n_taps)
{
    const char *who = "gal_synth_fir_set";
    if (!h) return fail(GAL_E_INVAL, "null handle");
    if (n_taps != 0) {
        const int rc = gal_synth_fir_check(taps_q14, n_taps);
        if (rc) return rc;
    }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->fir.sync.wait());  // the table and the histories belong to the kernel in flight
    if (n_taps == 0) {
        h->fir.release();
        return GAL_OK;
    }
    hipStream_t st;
    GAL_TRY(enter(h, &st, false));
    const size_t table_bytes = sizeof(uint32_t) * kFirTableWords, bytes = table_bytes + 2 * sizeof(uint32_t) * kFirHist;
    if (!h->fir.d && !alloc_pair(&h->fir.d, bytes, &h->fir.h_tab, table_bytes))
        return fail(GAL_E_NOMEM, "%s: the filter table of %zu bytes could not be allocated", who, bytes);
    // from here on the filter in force is gone: a failure leaves the handle without one
    h->fir.taps = 0;
    memset(h->fir.h_tab, 0, table_bytes);
    int trips = 0, hs = 0;
    galk_fir_table(taps_q14, n_taps, h->fir.h_tab, &trips, &hs);
    HIP_TRY(hipMemcpyAsync(h->fir.d, h->fir.h_tab, table_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(h->fir.d + kFirTableWords, 0, 2 * sizeof(uint32_t) * kFirHist, st));
    HIP_TRY(h->fir.sync.mark(st));  // (the upload reads h_tab: the next call waits for it as for a kernel)
    h->fir.taps = n_taps;
    h->fir.trips = trips;
    h->fir.hs = hs;
    h->fir.cur = 0;
    return GAL_OK;
}

int gal_synth_iq_fir(gal_synth_t *h, const int16_t *in_dev, size_t n_samples, int16_t *out_dev)
{
    const char *who = "gal_synth_iq_fir";
    if (!h) return fail(GAL_E_INVAL, "null handle");
    GAL_TRY(check_aligned(who, in_dev));
    GAL_TRY(check_aligned(who, out_dev));
    if ((uint64_t)n_samples >> 41) return fail(GAL_E_INVAL, "%s: n_samples must be below 2^41", who);
    if (!h->fir.taps) return fail(GAL_E_STATE, "%s: no filter set (call gal_synth_fir_set first)", who);
    if (n_samples == 0) return GAL_OK;
    const size_t bytes = 4 * n_samples;
    GAL_TRY(check_overlap(who, in_dev, bytes, out_dev, bytes, false, " (in place is not possible: tiles read their neighbours' input)"));
    GAL_TRY(check_in_flight(who, h, in_dev, bytes, "input of"));
    GAL_TRY(check_in_flight(who, h, out_dev, bytes, "output of"));
    hipStream_t st;
    GAL_TRY(enter(h, &st));
    uint32_t *const hist = h->fir.d + kFirTableWords;
    HIP_TRY(galk_launch_iq_fir(in_dev, out_dev, (uint64_t)n_samples, h->fir.d, h->fir.trips, h->fir.hs, hist + h->fir.cur * kFirHist,
                               hist + (h->fir.cur ^ 1) * kFirHist, h->d_iq_sat, st));
    h->fir.cur ^= 1;
    HIP_TRY(h->fir.sync.mark(st));
    return GAL_OK;
}

// ---- decimating front-end filter (iq_firdec.hip) --------------------------------------------------------------------------------------
static constexpr int kFdTableWords = 640;  // min(M, T) branches x trips x 4 words <= T - 1 + 5 M (galk_firdec_table checks it)
static constexpr int kFdHist = 512;        // complex samples of history, as iq_firdec.hip keeps them

int gal_synth_firdec_check(const int16_t *taps_q14, int32_t n_taps, int32_t decim)
{
    const char *who = "gal_synth_firdec_check";
    if (!taps_q14) return fail(GAL_E_INVAL, "%s: null taps", who);
    if (n_taps < 1 || n_taps > GAL_FIRDEC_MAX_TAPS) return fail(GAL_E_INVAL, "%s: %d taps (1..%d)", who, n_taps, GAL_FIRDEC_MAX_TAPS);
    if (decim < 2 || decim > GAL_FIRDEC_MAX_DECIM) return fail(GAL_E_INVAL, "%s: decimation %d (2..%d)", who, decim, GAL_FIRDEC_MAX_DECIM);
    long sum = 0;
    for (int k = 0; k < n_taps; ++k) sum += std::abs((long)taps_q14[k]);
    if (sum > 65535)
        return fail(GAL_E_INVAL, "%s: the taps' absolute values sum to %ld, more than 65535 (16384 = 1.0): the int32 accumulator could wrap", who, sum);
    return GAL_OK;
}

int gal_synth_firdec_lowpass(double cutoff_hz, double sample_rate_in, int32_t n_taps, int16_t *taps_q14)
{
    return lowpass_design("gal_synth_firdec_lowpass", cutoff_hz, sample_rate_in, n_taps, GAL_FIRDEC_MAX_TAPS - 1, taps_q14);
}

uint64_t gal_synth_firdec_out_samples(uint64_t first_sample, uint64_t n_in, int32_t decim)
{
    if (decim < 2 || decim > GAL_FIRDEC_MAX_DECIM || first_sample + n_in < first_sample) return 0;
    const uint64_t M = (uint64_t)decim, end = first_sample + n_in;
    // ceil(a / M) = a / M + (a % M != 0), without a + M - 1 (which could wrap)
    return (end / M + (end % M != 0)) - (first_sample / M + (first_sample % M != 0));
}

int gal_synth_firdec_set(gal_synth_t *h, const int16_t *taps_q14, int32_t n_taps, int32_t decim, uint64_t first_sample)
{
    const char *who = "gal_synth_firdec_set";
    if (!h) return fail(GAL_E_INVAL, "null handle");
    if (n_taps != 0) {
        const int rc = gal_synth_firdec_check(taps_q14, n_taps, decim);
        if (rc) return rc;
    }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->fd.sync.wait());  // the table and the histories belong to the kernel in flight
    if (n_taps == 0) {
        h->fd.release();
        return GAL_OK;
    }
    hipStream_t st;
    GAL_TRY(enter(h, &st, false));
    const size_t table_bytes = sizeof(uint32_t) * kFdTableWords, bytes = table_bytes + 2 * sizeof(uint32_t) * kFdHist;
    if (!h->fd.d && !alloc_pair(&h->fd.d, bytes, &h->fd.h_tab, table_bytes))
        return fail(GAL_E_NOMEM, "%s: the filter table of %zu bytes could not be allocated", who, bytes);
    // from here on the decimator in force is gone: a failure leaves the handle without one
    h->fd.taps = 0;
    memset(h->fd.h_tab, 0, table_bytes);
    int trips = 0;
    const int words = galk_firdec_table(taps_q14, n_taps, decim, h->fd.h_tab, &trips);
    if (words <= 0 || words > kFdTableWords) return fail(GAL_E_INVAL, "%s: no kernel shape for %d taps at decimation %d", who, n_taps, decim);
    HIP_TRY(hipMemcpyAsync(h->fd.d, h->fd.h_tab, table_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(h->fd.d + kFdTableWords, 0, 2 * sizeof(uint32_t) * kFdHist, st));
    HIP_TRY(h->fd.sync.mark(st));  // (the upload reads h_tab: the next call waits for it as for a kernel)
    h->fd.taps = n_taps;
    h->fd.decim = decim;
    h->fd.phase = (int)(first_sample % (uint64_t)decim);
    h->fd.cur = 0;
    return GAL_OK;
}

int gal_synth_iq_firdec(gal_synth_t *h, const int16_t *in_dev, size_t n_in, int16_t *out_dev, size_t *n_out)
{
    const char *who = "gal_synth_iq_firdec";
    if (!h) return fail(GAL_E_INVAL, "null handle");
    if (!n_out) return fail(GAL_E_INVAL, "%s: null n_out", who);
    GAL_TRY(check_aligned(who, in_dev));
    GAL_TRY(check_aligned(who, out_dev));
    if ((uint64_t)n_in >> 41) return fail(GAL_E_INVAL, "%s: n_in must be below 2^41", who);
    if (!h->fd.taps) return fail(GAL_E_STATE, "%s: no decimator set (call gal_synth_firdec_set first)", who);
    if (n_in == 0) {
        *n_out = 0;
        return GAL_OK;
    }
    const uint64_t outs = gal_synth_firdec_out_samples((uint64_t)h->fd.phase, (uint64_t)n_in, h->fd.decim);
    const size_t in_bytes = 4 * n_in, out_bytes = 4 * (size_t)outs;
    GAL_TRY(check_overlap(who, in_dev, in_bytes, out_dev, out_bytes, false, " (tiles read their neighbours' input)"));
    GAL_TRY(check_in_flight(who, h, in_dev, in_bytes, "input of"));
    if (outs) GAL_TRY(check_in_flight(who, h, out_dev, out_bytes, "output of"));
    hipStream_t st;
    GAL_TRY(enter(h, &st));
    uint32_t *const hist = h->fd.d + kFdTableWords;
    const int i0 = (h->fd.decim - h->fd.phase) % h->fd.decim;  // the local index of the first input whose global index M divides
    HIP_TRY(galk_launch_iq_firdec(in_dev, out_dev, (uint64_t)n_in, outs, i0, h->fd.taps, h->fd.decim, h->fd.d, hist + h->fd.cur * kFdHist,
                                  hist + (h->fd.cur ^ 1) * kFdHist, h->d_iq_sat, st));
    h->fd.cur ^= 1;
    h->fd.phase = (int)(((uint64_t)h->fd.phase + (uint64_t)n_in) % (uint64_t)h->fd.decim);
    HIP_TRY(h->fd.sync.mark(st));
    *n_out = (size_t)outs;
    return GAL_OK;
}

// ---- block AGC and 2-bit quantiser (iq_agc.hip) ------------------------------------------------------------------------------------
static constexpr int kAgcState = GAL_AGC_MAX_WINDOW + 1;  // words of one state buffer, as iq_agc.hip keeps them

int gal_synth_agc_check(const gal_iq_agc_t *a)
{
    const char *who = "gal_synth_agc_check";
    if (!a) return fail(GAL_E_INVAL, "%s: null argument", who);
    if (a->block_len < GAL_AGC_MIN_BLOCK || a->block_len > GAL_AGC_MAX_BLOCK)
        return fail(GAL_E_INVAL, "%s: block_len %u (%d..%d)", who, a->block_len, GAL_AGC_MIN_BLOCK, GAL_AGC_MAX_BLOCK);
    if (a->window < 1 || a->window > GAL_AGC_MAX_WINDOW) return fail(GAL_E_INVAL, "%s: window %u (1..%d)", who, a->window, GAL_AGC_MAX_WINDOW);
    if ((uint64_t)a->block_len * a->window > GAL_AGC_MAX_SPAN)
        return fail(GAL_E_INVAL, "%s: block_len %u x window %u = %llu samples, more than %d: the window sum could pass 2^47", who, a->block_len,
                    a->window, (unsigned long long)a->block_len * a->window, GAL_AGC_MAX_SPAN);
    if (a->target_q8 < 1 || a->target_q8 > 32767u * 256u) return fail(GAL_E_INVAL, "%s: target_q8 %u (1..%u)", who, a->target_q8, 32767u * 256u);
    if (a->gain_min_q12 < 1 || a->gain_min_q12 > a->gain_max_q12 || a->gain_max_q12 > GAL_AGC_GAIN_MAX)
        return fail(GAL_E_INVAL, "%s: gain clamps %u .. %u (1 <= min <= max <= %u; 4096 = 1.0)", who, a->gain_min_q12, a->gain_max_q12, GAL_AGC_GAIN_MAX);
    if (a->p_init > ((uint64_t)a->block_len << 31))
        return fail(GAL_E_INVAL, "%s: p_init %llu is more than 2^31 x block_len = %llu", who, (unsigned long long)a->p_init,
                    (unsigned long long)a->block_len << 31);
    if (a->reserved != 0) return fail(GAL_E_INVAL, "%s: reserved %u (0)", who, a->reserved);
    return GAL_OK;
}

size_t gal_synth_agc_out_bytes(int32_t format, size_t n_samples)
{
    switch (format) {
    case GAL_IQ_ISHORT: return 4 * n_samples;
    case GAL_IQ_IBYTE: return 2 * n_samples;
    case GAL_IQ_I2BIT: return n_samples / 2 + (n_samples & 1);
    default: return 0;
    }
}

uint64_t gal_synth_agc_blocks(uint64_t first_sample, uint64_t n_samples, int32_t block_len)
{
    if (block_len < GAL_AGC_MIN_BLOCK || block_len > GAL_AGC_MAX_BLOCK || first_sample + n_samples < first_sample) return 0;
    const uint64_t B = (uint64_t)block_len, end = first_sample + n_samples;
    // ceil(a / B) = a / B + (a % B != 0), without a + B - 1 (which could wrap)
    return (end / B + (end % B != 0)) - (first_sample / B + (first_sample % B != 0));
}

int gal_synth_agc_from_rms(double target_rms, double init_rms, int32_t block_len, int32_t window, gal_iq_agc_t *out)
{
    const char *who = "gal_synth_agc_from_rms";
    if (!out) return fail(GAL_E_INVAL, "%s: null argument", who);
    if (!std::isfinite(target_rms) || !std::isfinite(init_rms) || !(init_rms >= 0.0) || !(init_rms <= 32768.0) || !(target_rms >= 0.0) ||
        !(target_rms <= 32768.0))
        return fail(GAL_E_INVAL, "%s: target rms %g, initial rms %g (finite, 0..32768 int16 LSB)", who, target_rms, init_rms);
    if (block_len < 0 || window < 0) return fail(GAL_E_INVAL, "%s: block_len %d, window %d", who, block_len, window);
    gal_iq_agc_t a;
    memset(&a, 0, sizeof(a));
    a.block_len = (uint32_t)block_len;
    a.window = (uint32_t)window;
    a.target_q8 = (uint32_t)llround(target_rms * 256.0);
    a.gain_min_q12 = 1;
    a.gain_max_q12 = GAL_AGC_GAIN_MAX;
    const double sq = init_rms * init_rms;
    a.p_init = 2ull * (uint64_t)block_len * (uint64_t)llround(sq);
    const int rc = gal_synth_agc_check(&a);
    if (rc) return rc;
    *out = a;
    return GAL_OK;
}

int gal_synth_agc_set(gal_synth_t *h, const gal_iq_agc_t *agc, uint64_t first_sample)
{
    const char *who = "gal_synth_agc_set";
    if (!h) return fail(GAL_E_INVAL, "null handle");
    gal_iq_agc_t a;
    if (agc) {
        a = *agc;  // the caller's struct is not looked at again
        const int rc = gal_synth_agc_check(&a);
        if (rc) return rc;
        if (first_sample >> 62) return fail(GAL_E_INVAL, "%s: first_sample must be below 2^62", who);
    }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->agc.sync.wait());  // the states and the scratch belong to the kernels in flight
    if (!agc) {
        h->agc.release();
        return GAL_OK;
    }
    hipStream_t st;
    GAL_TRY(enter(h, &st, false));
    const size_t state_bytes = sizeof(unsigned long long) * kAgcState;
    if (!h->agc.d && !alloc_pair(&h->agc.d, 2 * state_bytes, &h->agc.h_state, state_bytes))
        return fail(GAL_E_NOMEM, "%s: the state of %zu bytes could not be allocated", who, 2 * state_bytes);
    // from here on the AGC in force is gone: a failure leaves the handle without one
    h->agc.on = false;
    for (int k = 0; k < kAgcState; ++k) h->agc.h_state[k] = k < (int)a.window ? a.p_init : 0ull;
    HIP_TRY(hipMemcpyAsync(h->agc.d, h->agc.h_state, state_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(h->agc.sync.mark(st));  // (the upload reads h_state: the next call waits for it as for a kernel)
    h->agc.cfg = a;
    h->agc.pos = first_sample;
    h->agc.cur = 0;
    h->agc.on = true;
    return GAL_OK;
}

int gal_synth_iq_agc(gal_synth_t *h, const int16_t *in_dev, size_t n_samples, int32_t format, int32_t param, void *out_dev, uint32_t *gains_dev,
                     size_t *n_gains)
{
    const char *who = "gal_synth_iq_agc";
    if (!h) return fail(GAL_E_INVAL, "null handle");
    if (format != GAL_IQ_ISHORT && format != GAL_IQ_IBYTE && format != GAL_IQ_I2BIT)
        return fail(GAL_E_INVAL, "%s: format %d (GAL_IQ_ISHORT 0, GAL_IQ_IBYTE 1, GAL_IQ_I2BIT 3; a sign, GAL_IQ_IBIT, needs no gain control)", who, format);
    if (format == GAL_IQ_IBYTE ? (param < 0 || param > 15) : format == GAL_IQ_I2BIT ? (param < 1 || param > 32767) : param != 0)
        return fail(GAL_E_INVAL, "%s: param %d (the shift 0..15 for GAL_IQ_IBYTE, the threshold 1..32767 for GAL_IQ_I2BIT, 0 for GAL_IQ_ISHORT)", who, param);
    GAL_TRY(check_aligned(who, in_dev));
    GAL_TRY(check_aligned(who, out_dev));
    if ((uintptr_t)gains_dev & 3) return fail(GAL_E_INVAL, "%s: gains_dev must be 4-byte aligned", who);
    if ((uint64_t)n_samples >> 41) return fail(GAL_E_INVAL, "%s: n_samples must be below 2^41", who);
    if (!h->agc.on) return fail(GAL_E_STATE, "%s: no AGC set (call gal_synth_agc_set first)", who);
    if (n_samples == 0) {
        if (n_gains) *n_gains = 0;
        return GAL_OK;
    }
    const uint32_t B = h->agc.cfg.block_len, off0 = (uint32_t)(h->agc.pos % B);
    const uint64_t ng = gal_synth_agc_blocks(h->agc.pos, (uint64_t)n_samples, (int32_t)B);
    const size_t in_bytes = 4 * n_samples, out_bytes = gal_synth_agc_out_bytes(format, n_samples), g_bytes = gains_dev ? 4 * (size_t)ng : 0;
    GAL_TRY(check_overlap(who, in_dev, in_bytes, out_dev, out_bytes, false, ""));
    if (g_bytes && (ranges_overlap(in_dev, in_bytes, gains_dev, g_bytes) || ranges_overlap(out_dev, out_bytes, gains_dev, g_bytes)))
        return fail(GAL_E_INVAL, "%s: the gains overlap the input or the output", who);
    GAL_TRY(check_in_flight(who, h, in_dev, in_bytes, "input of"));
    GAL_TRY(check_in_flight(who, h, out_dev, out_bytes, "output of"));
    if (g_bytes) GAL_TRY(check_in_flight(who, h, gains_dev, g_bytes, "gains in"));
    hipStream_t st;
    GAL_TRY(enter(h, &st));
    // the scratch of this call: one per handle, grown when a call touches more blocks than any before it (only then the host waits
    // for the kernels of the call before)
    const uint64_t need = galk_agc_scratch_bytes((uint64_t)n_samples, off0, B);
    uint64_t cap = 0;
    const int rc = h->agc.scratch.reserve(need, 256, false, h->agc.sync, &cap);
    if (rc == GAL_E_NOMEM)
        return fail(GAL_E_NOMEM, "%s: the scratch of %llu bytes (12 per block touched) could not be allocated", who, (unsigned long long)cap);
    if (rc) return rc;
    HIP_TRY(galk_launch_iq_agc(in_dev, (uint64_t)n_samples, off0, format, param, &h->agc.cfg, h->agc.d + h->agc.cur * kAgcState,
                               h->agc.d + (h->agc.cur ^ 1) * kAgcState, h->agc.scratch.dev, out_dev, gains_dev, h->d_iq_sat, st));
    h->agc.cur ^= 1;
    h->agc.pos += (uint64_t)n_samples;
    HIP_TRY(h->agc.sync.mark(st));
    if (n_gains) *n_gains = (size_t)ng;
    return GAL_OK;
}

// ---- receiver oscillator (iq_osc.hip) ----------------------------------------------------------------------------------------------
static constexpr uint64_t kOscMaxS = 1ull << 48;

int gal_synth_osc_check(const gal_iq_osc_t *o)
{
    const char *who = "gal_synth_osc_check";
    if (!o) return fail(GAL_E_INVAL, "%s: null argument", who);
    if (o->reserved != 0) return fail(GAL_E_INVAL, "%s: reserved %u (0)", who, o->reserved);
    if (o->s > kOscMaxS) return fail(GAL_E_INVAL, "%s: s %llu is more than 2^48", who, (unsigned long long)o->s);
    return GAL_OK;
}

// M2 = the sum of mag(w)^2 over the 2^31 words w of the Gauss table's input (exact: below 2^31 x 2^30): per octave the 13 bits under
// the leading one choose the cell and the fraction, every (cell, fraction) 2^(low - 13) times where the octave has low >= 13 bits
// under its leading one, else only those whose missing low bits are 0, once
static uint64_t gauss_m2()
{
    const int32_t(*T)[32][2] = (const int32_t(*)[32][2])gal_tables_gauss();
    uint64_t m2 = 0;
    for (int o = 0; o < 31; ++o) {
        const int low = 30 - o, step = low >= 13 ? 1 : 1 << (13 - low);
        uint64_t acc = 0;
        for (int sf = 0; sf < 8192; sf += step) {
            const int64_t a = T[o][sf >> 8][0], b = T[o][sf >> 8][1], mag = a - (((a - b) * (sf & 255) + 128) >> 8);
            acc += (uint64_t)(mag * mag);
        }
        m2 += low >= 13 ? acc << (low - 13) : acc;
    }
    const int64_t m0 = T[31][0][0];  // w = 0
    return m2 + (uint64_t)(m0 * m0);
}

int gal_synth_osc_make(double f_hz, double drift_hz_s, double h0, double sample_rate, double carrier_hz, gal_iq_osc_t *out)
{
    const char *who = "gal_synth_osc_make";
    if (!out) return fail(GAL_E_INVAL, "%s: null argument", who);
    if (!std::isfinite(f_hz) || !std::isfinite(drift_hz_s) || !std::isfinite(h0) || !std::isfinite(sample_rate) || !std::isfinite(carrier_hz))
        return fail(GAL_E_INVAL, "%s: an argument is not finite", who);
    if (!(sample_rate > 0.0) || carrier_hz < 0.0 || h0 < 0.0)
        return fail(GAL_E_INVAL, "%s: sample rate %g (> 0), carrier %g Hz (>= 0), h0 %g s (>= 0)", who, sample_rate, carrier_hz, h0);
    if (!(fabs(f_hz) < sample_rate / 2)) return fail(GAL_E_INVAL, "%s: offset %g Hz must lie inside +-sample_rate / 2 = %g Hz", who, f_hz, sample_rate / 2);
    const double two64 = 18446744073709551616.0, two63 = 9223372036854775808.0;
    const double fv = f_hz / sample_rate * two64, dv = drift_hz_s / sample_rate / sample_rate * two64;
    if (!(fabs(fv) < two63)) return fail(GAL_E_INVAL, "%s: offset %g Hz must lie inside +-sample_rate / 2 = %g Hz", who, f_hz, sample_rate / 2);
    if (!(fabs(dv) < two63))
        return fail(GAL_E_INVAL, "%s: drift %g Hz/s does not fit (|drift| < sample_rate^2 / 2 = %g Hz/s)", who, drift_hz_s, sample_rate * sample_rate / 2);
    const double v = (double)gauss_m2() / 36028797018963968.0;  // 2^55 = 2^31 words x 4096^2
    const double sigma_cycles = carrier_hz * sqrt(h0 / (2.0 * sample_rate));
    const double sv = sigma_cycles / sqrt(v) * 4503599627370496.0;  // 2^52
    if (!(sv <= (double)kOscMaxS)) return fail(GAL_E_INVAL, "%s: the phase noise of h0 %g s needs s = %g, more than 2^48", who, h0, sv);
    gal_iq_osc_t o;
    memset(&o, 0, sizeof(o));
    o.seed = 1;
    o.f = (int64_t)llround(fv);
    o.d = (int64_t)llround(dv);
    o.s = (uint64_t)llround(sv);
    *out = o;
    return GAL_OK;
}

int gal_synth_osc_lo_step(const gal_iq_osc_t *osc, uint64_t N, int32_t *carr_dph)
{
    if (!osc || !carr_dph) return fail(GAL_E_INVAL, "gal_synth_osc_lo_step: null argument");
    *carr_dph = (int32_t)(uint32_t)(((uint64_t)osc->f + N * (uint64_t)osc->d) >> 32);
    return GAL_OK;
}

int gal_synth_osc_set(gal_synth_t *h, const gal_iq_osc_t *osc, uint64_t first_sample)
{
    const char *who = "gal_synth_osc_set";
    if (!h) return fail(GAL_E_INVAL, "null handle");
    gal_iq_osc_t o;
    if (osc) {
        o = *osc;  // the caller's struct is not looked at again
        const int rc = gal_synth_osc_check(&o);
        if (rc) return rc;
        if (first_sample >> 62) return fail(GAL_E_INVAL, "%s: first_sample must be below 2^62", who);
    }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->osc.sync.wait());  // the state and the scratch belong to the kernels in flight
    if (!osc) {
        h->osc.release();
        return GAL_OK;
    }
    hipStream_t st;
    GAL_TRY(enter(h, &st, false));
    if (!h->osc.d && hipMalloc((void **)&h->osc.d, 2 * sizeof(long long)) != hipSuccess) {
        h->osc.d = nullptr;
        (void)hipGetLastError();
        return fail(GAL_E_NOMEM, "%s: the state of 16 bytes could not be allocated", who);
    }
    // from here on the oscillator in force is gone: a failure leaves the handle without one
    h->osc.on = false;
    HIP_TRY(hipMemsetAsync(h->osc.d, 0, 2 * sizeof(long long), st));
    HIP_TRY(h->osc.sync.mark(st));
    h->osc.cfg = o;
    h->osc.n0 = h->osc.pos = first_sample;
    h->osc.cur = 0;
    h->osc.on = true;
    return GAL_OK;
}

int gal_synth_iq_osc(gal_synth_t *h, const int16_t *in_dev, size_t n_samples, int16_t *out_dev)
{
    const char *who = "gal_synth_iq_osc";
    if (!h) return fail(GAL_E_INVAL, "null handle");
    GAL_TRY(check_aligned(who, in_dev));
    GAL_TRY(check_aligned(who, out_dev));
    if ((uint64_t)n_samples >> 41) return fail(GAL_E_INVAL, "%s: n_samples must be below 2^41", who);
    if (!h->osc.on) return fail(GAL_E_STATE, "%s: no oscillator set (call gal_synth_osc_set first)", who);
    if (n_samples == 0) return GAL_OK;
    const size_t bytes = 4 * n_samples;
    GAL_TRY(check_overlap(who, in_dev, bytes, out_dev, bytes, true, " (only exactly in place may)"));
    GAL_TRY(check_in_flight(who, h, in_dev, bytes, "input of"));
    GAL_TRY(check_in_flight(who, h, out_dev, bytes, "output of"));
    hipStream_t st;
    GAL_TRY(enter(h, &st));
    const bool noise = h->osc.cfg.s != 0;
    // the scratch of this call: one per handle, grown when a call is longer than any before it (only then the host waits for the
    // kernels of the call before)
    const uint64_t need = noise ? galk_osc_scratch_bytes((uint64_t)n_samples) : 0;
    uint64_t cap = 0;
    const int rc = h->osc.scratch.reserve(need, 256, false, h->osc.sync, &cap);
    if (rc == GAL_E_NOMEM)
        return fail(GAL_E_NOMEM, "%s: the scratch of %llu bytes (12 per tile of 1024 samples) could not be allocated", who, (unsigned long long)cap);
    if (rc) return rc;
    HIP_TRY(galk_launch_iq_osc(in_dev, out_dev, (uint64_t)n_samples, h->osc.pos, h->osc.n0, &h->osc.cfg, h->osc.d + h->osc.cur, h->osc.d + (h->osc.cur ^ 1),
                               h->osc.scratch.dev, h->d_iq_sat, st));
    if (noise) h->osc.cur ^= 1;
    h->osc.pos += (uint64_t)n_samples;
    HIP_TRY(h->osc.sync.mark(st));
    return GAL_OK;
}

// ---- per-satellite ionospheric scintillation (iq_scint.hip) ------------------------------------------------------------------------
int gal_synth_scint_check(const gal_iq_scint_t *row)
{
    const char *who = "gal_synth_scint_check";
    if (!row) return fail(GAL_E_INVAL, "%s: null argument", who);
    if (row->reserved != 0) return fail(GAL_E_INVAL, "%s: reserved %u (0)", who, row->reserved);
    if (row->node_len < GAL_SCINT_MIN_NODE || row->node_len > GAL_SCINT_MAX_NODE)
        return fail(GAL_E_INVAL, "%s: node_len %u (%d..%u)", who, row->node_len, GAL_SCINT_MIN_NODE, GAL_SCINT_MAX_NODE);
    if (row->a_q12 > 4096 || row->b_q12 > 4096) return fail(GAL_E_INVAL, "%s: a_q12 %u, b_q12 %u (0..4096)", who, row->a_q12, row->b_q12);
    return GAL_OK;
}

static bool scint_identity(const gal_iq_scint_t &r) { return r.a_q12 == 4096 && r.b_q12 == 0; }

int gal_synth_scint_make(double s4, double tau0_s, double sample_rate, gal_iq_scint_t *out)
{
    const char *who = "gal_synth_scint_make";
    if (!out) return fail(GAL_E_INVAL, "%s: null argument", who);
    if (!std::isfinite(s4) || !std::isfinite(tau0_s) || !std::isfinite(sample_rate)) return fail(GAL_E_INVAL, "%s: an argument is not finite", who);
    if (!(s4 >= 0.0 && s4 <= 1.0) || !(sample_rate > 0.0)) return fail(GAL_E_INVAL, "%s: s4 %g (0..1), sample rate %g (> 0)", who, s4, sample_rate);
    const double lv = tau0_s * sample_rate / 8.0;
    if (!(lv >= 0.0 && lv < 4294967296.0)) return fail(GAL_E_INVAL, "%s: tau0 %g s gives no node_len in %d..%u", who, tau0_s, GAL_SCINT_MIN_NODE, GAL_SCINT_MAX_NODE);
    const long long L = llround(lv);
    if (L < GAL_SCINT_MIN_NODE || L > (long long)GAL_SCINT_MAX_NODE)
        return fail(GAL_E_INVAL, "%s: tau0 %g s at %g S/s gives node_len %lld (%d..%u)", who, tau0_s, sample_rate, L, GAL_SCINT_MIN_NODE, GAL_SCINT_MAX_NODE);
    const int32_t *ht = gal_tables_scint();
    int64_t h2 = 0;
    for (int t = 0; t < 32; ++t) h2 += (int64_t)ht[t] * ht[t];
    const double v = ((double)h2 / 1073741824.0) * ((double)gauss_m2() / 36028797018963968.0);  // (H2 / 2^30) x (M2 / 2^55)
    gal_iq_scint_t r;
    memset(&r, 0, sizeof(r));
    r.seed = 1;
    r.node_len = (uint32_t)L;
    if (s4 == 0.0) {
        r.a_q12 = 4096;
    } else if (s4 == 1.0) {
        r.b_q12 = (uint16_t)llround(4096.0 * sqrt(1.0 / (2.0 * v)));
    } else {
        const double m = 1.0 / (s4 * s4), q = sqrt(m * m - m), K = q / (m - q);
        r.a_q12 = (uint16_t)llround(4096.0 * sqrt(K / (K + 1.0)));
        r.b_q12 = (uint16_t)llround(4096.0 * sqrt(1.0 / (2.0 * (K + 1.0) * v)));
    }
    *out = r;
    return GAL_OK;
}

// one job as k_iq_scint reads it (iq_scint.hip: struct ScintJob)
struct ScintJobDev {
    const int16_t *in;
    int16_t *out;
    uint64_t n, first;
    uint32_t k0, k1, stream, L, R;
    int32_t A, B;
    uint32_t pad;
};
static_assert(sizeof(ScintJobDev) == 64, "iq_scint.hip reads 64 bytes per job");

int gal_synth_iq_scint(gal_synth_t *h, const gal_scint_job_t *jobs, int32_t n_jobs)
{
    const char *who = "gal_synth_iq_scint";
    if (!h) return fail(GAL_E_INVAL, "null handle");
    if (!jobs || n_jobs < 1 || n_jobs > GAL_SCINT_MAX_JOBS) return fail(GAL_E_INVAL, "%s: null argument or n_jobs %d (1..%d)", who, n_jobs, GAL_SCINT_MAX_JOBS);
    for (int k = 0; k < n_jobs; ++k) {
        const gal_scint_job_t &j = jobs[k];
        GAL_TRY(check_aligned(who, j.in_dev, k));
        GAL_TRY(check_aligned(who, j.out_dev, k));
        GAL_TRY(gal_synth_scint_check(&j.row));
        if (j.n_samples >> 41) return fail(GAL_E_INVAL, "%s: n_samples of job %d must be below 2^41", who, k);
        if (j.first_sample >> 62) return fail(GAL_E_INVAL, "%s: first_sample of job %d must be below 2^62", who, k);
    }
    for (int k = 0; k < n_jobs; ++k) {
        const gal_scint_job_t &j = jobs[k];
        const size_t bytes = 4 * (size_t)j.n_samples;
        if (bytes == 0) continue;
        if (j.in_dev != j.out_dev && ranges_overlap(j.in_dev, bytes, j.out_dev, bytes))
            return fail(GAL_E_INVAL, "%s: input and output of job %d overlap (only exactly in place may)", who, k);
        for (int i = 0; i < n_jobs; ++i) {  // the output of job k against the buffers of every other job
            const size_t other = 4 * (size_t)jobs[i].n_samples;
            if (i == k || other == 0) continue;
            if (ranges_overlap(j.out_dev, bytes, jobs[i].in_dev, other) || ranges_overlap(j.out_dev, bytes, jobs[i].out_dev, other))
                return fail(GAL_E_INVAL, "%s: the output of job %d meets a buffer of job %d", who, k, i);
        }
        GAL_TRY(check_in_flight(who, h, j.in_dev, bytes, "input of"));
        GAL_TRY(check_in_flight(who, h, j.out_dev, bytes, "output of"));
    }
    hipStream_t st;
    GAL_TRY(enter(h, &st));
    HIP_TRY(h->scint.sync.wait());  // one table per handle: the call before has read it
    uint64_t cap = 0;
    const int rc = h->scint.table.reserve(sizeof(ScintJobDev) * GAL_SCINT_MAX_JOBS, 0, true, h->scint.sync, &cap);
    if (rc == GAL_E_NOMEM) return fail(GAL_E_NOMEM, "%s: the job table of %zu bytes could not be allocated", who, (size_t)cap);
    if (rc) return rc;
    ScintJobDev *const tab = (ScintJobDev *)h->scint.table.host;
    int n = 0;
    uint64_t max_n = 0;
    for (int k = 0; k < n_jobs; ++k) {
        const gal_scint_job_t &j = jobs[k];
        if (j.n_samples == 0 || (scint_identity(j.row) && j.in_dev == j.out_dev)) continue;  // nothing to do
        ScintJobDev &d = tab[n++];
        d.in = j.in_dev;
        d.out = j.out_dev;
        d.n = j.n_samples;
        d.first = j.first_sample;
        d.k0 = (uint32_t)j.row.seed;
        d.k1 = (uint32_t)(j.row.seed >> 32);
        d.stream = j.row.stream;
        d.L = j.row.node_len;
        d.R = (uint32_t)(4294967296ull / j.row.node_len);
        d.A = j.row.a_q12;
        d.B = j.row.b_q12;
        d.pad = 0;
        max_n = std::max(max_n, d.n);
    }
    if (n == 0) return GAL_OK;
    HIP_TRY(hipMemcpyAsync(h->scint.table.dev, tab, sizeof(ScintJobDev) * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(galk_launch_iq_scint(h->scint.table.dev, n, max_n, h->d_iq_sat, st));
    HIP_TRY(h->scint.sync.mark(st));
    return GAL_OK;
}

// ---- antenna array (iq_array.hip) ---------------------------------------------------------------------------------------------------
int gal_synth_steer_check(const gal_iq_steer_t *rows, int32_t n_epochs, int32_t n_elem, int32_t n_parts)
{
    const char *who = "gal_synth_steer_check";
    if (!rows) return fail(GAL_E_INVAL, "%s: null rows", who);
    if (n_epochs < 1 || n_elem < 1 || n_elem > GAL_ARRAY_MAX_ELEM || n_parts < 1 || n_parts > GAL_ENGINE_MAX_CHAN)
        return fail(GAL_E_INVAL, "%s: n_epochs %d (>= 1), n_elem %d (1..%d) or n_parts %d (1..%d)", who, n_epochs, n_elem, GAL_ARRAY_MAX_ELEM, n_parts,
                    GAL_ENGINE_MAX_CHAN);
    const size_t per = (size_t)n_elem * n_parts;
    for (size_t i = 0; i < (size_t)n_epochs * per; ++i)
        if (rows[i].w_re == INT16_MIN || rows[i].w_im == INT16_MIN)
            return fail(GAL_E_INVAL, "%s: weight (%d, %d) of epoch %zu, element %zu, part %zu (-32767..32767)", who, rows[i].w_re, rows[i].w_im, i / per,
                        i % per / n_parts, i % n_parts);
    return GAL_OK;
}

int gal_synth_steer_make(uint16_t gain_q7, uint32_t phase, gal_iq_steer_t *out)
{
    if (!out) return fail(GAL_E_INVAL, "gal_synth_steer_make: null argument");
    if (gain_q7 > GAL_STEER_GAIN_MAX)
        return fail(GAL_E_INVAL, "gal_synth_steer_make: gain %u (0..%d: the weight would leave int16)", gain_q7, GAL_STEER_GAIN_MAX);
    const int16_t *C = gal_tables_cos1024();
    const uint32_t i = ((phase + (1u << 21)) >> 22) & 1023u;
    const int g = gain_q7;
    out->w_re = (int16_t)((g * C[i] + 64) >> 7);
    out->w_im = (int16_t)((g * C[(i - 256u) & 1023u] + 64) >> 7);
    return GAL_OK;
}

int gal_synth_array_phase(const double enu_m[3], double az_rad, double el_rad, uint32_t *phase)
{
    if (!enu_m || !phase) return fail(GAL_E_INVAL, "gal_synth_array_phase: null argument");
    if (!std::isfinite(enu_m[0]) || !std::isfinite(enu_m[1]) || !std::isfinite(enu_m[2]) || !std::isfinite(az_rad) || !std::isfinite(el_rad))
        return fail(GAL_E_INVAL, "gal_synth_array_phase: an argument is not finite");
    const double lambda = 299792458.0 / 1575420000.0;
    const double ce = cos(el_rad);
    const double u[3] = {sin(az_rad) * ce, cos(az_rad) * ce, sin(el_rad)};
    const double cyc = (enu_m[0] * u[0] + enu_m[1] * u[1] + enu_m[2] * u[2]) / lambda;
    *phase = (uint32_t)((uint64_t)llround((cyc - floor(cyc)) * 4294967296.0) & 0xffffffffull);
    return GAL_OK;
}

// the element outputs of an array call, `bytes` each: aligned, none meeting another
static int check_outputs(const char *who, int16_t *const *out_dev, int n_elem, size_t bytes)
{
    for (int a = 0; a < n_elem; ++a) {
        GAL_TRY(check_aligned(who, out_dev[a]));
        for (int b = 0; b < a; ++b)
            if (ranges_overlap(out_dev[a], bytes, out_dev[b], bytes)) return fail(GAL_E_INVAL, "%s: the outputs of elements %d and %d overlap", who, b, a);
    }
    return GAL_OK;
}

int gal_synth_iq_array(gal_synth_t *h, const int16_t *const *parts_dev, int32_t n_parts, const gal_iq_steer_t *rows, int32_t n_epochs,
                       int32_t n_elem, int16_t *const *out_dev)
{
    const char *who = "gal_synth_iq_array";
    if (!h) return fail(GAL_E_INVAL, "null handle");
    if (!parts_dev || !out_dev) return fail(GAL_E_INVAL, "%s: null argument", who);
    GAL_TRY(gal_synth_steer_check(rows, n_epochs, n_elem, n_parts));
    const size_t bytes = (size_t)n_epochs * (size_t)h->cfg.samples_per_epoch * 4;
    GAL_TRY(check_outputs(who, out_dev, n_elem, bytes));
    for (int a = 0; a < n_elem; ++a) GAL_TRY(check_parts(who, h, parts_dev, n_parts, out_dev[a], bytes));
    uint64_t row_max = 0;  // the largest sum of |w_re| + |w_im| over the parts of one (epoch, element): what A needs (iq_array.hip)
    for (size_t r = 0; r < (size_t)n_epochs * n_elem; ++r) {
        uint64_t row = 0;
        for (int k = 0; k < n_parts; ++k) row += (uint64_t)std::abs((int)rows[r * n_parts + k].w_re) + (uint64_t)std::abs((int)rows[r * n_parts + k].w_im);
        row_max = std::max(row_max, row);
    }
    hipStream_t st;
    GAL_TRY(enter(h, &st));
    // the table of this call: part pointers, output pointers, then the packed weights.  One per handle: a call waits for the kernel of
    // the call before it
    HIP_TRY(h->array.sync.wait());
    const size_t o_out = sizeof(void *) * GAL_ENGINE_MAX_CHAN, o_w = o_out + sizeof(void *) * GAL_ARRAY_MAX_ELEM;
    const size_t need = o_w + (size_t)n_epochs * n_parts * n_elem * 2 * sizeof(uint32_t);
    uint64_t cap = 0;
    const int rc = h->array.table.reserve(need, 0, true, h->array.sync, &cap);
    if (rc == GAL_E_NOMEM) return fail(GAL_E_NOMEM, "%s: the weight table of %zu bytes could not be allocated", who, (size_t)cap);
    if (rc) return rc;
    memset(h->array.table.host, 0, o_w);
    memcpy(h->array.table.host, parts_dev, sizeof(void *) * (size_t)n_parts);
    memcpy(h->array.table.host + o_out, out_dev, sizeof(void *) * (size_t)n_elem);
    uint32_t *const hw = (uint32_t *)(h->array.table.host + o_w);  // [e][k][a][2]: the elements of one part side by side
    for (int e = 0; e < n_epochs; ++e)
        for (int a = 0; a < n_elem; ++a)
            for (int k = 0; k < n_parts; ++k) {
                const gal_iq_steer_t &w = rows[((size_t)e * n_elem + a) * n_parts + k];
                galk_array_pack(w.w_re, w.w_im, hw + (((size_t)e * n_parts + k) * n_elem + a) * 2);
            }
    HIP_TRY(hipMemcpyAsync(h->array.table.dev, h->array.table.host, need, hipMemcpyHostToDevice, st));
    HIP_TRY(galk_launch_iq_array((const int16_t *const *)h->array.table.dev, (int16_t *const *)(h->array.table.dev + o_out),
                                 (const uint32_t *)(h->array.table.dev + o_w), n_parts, n_elem, n_epochs, h->cfg.samples_per_epoch, row_max > 65535 ? 1 : 0,
                                 h->d_iq_sat, st));
    HIP_TRY(h->array.sync.mark(st));
    return GAL_OK;
}

// what gal_synth_run_array adds to run_groups: every active slot a group of its own, and gal_synth_iq_array as the final stage
struct ArrayRun {
    const uint32_t *phase;  // [E][n_elem][S]
    int n_elem;
    int16_t *const *out_dev;
};

// gal_synth_run_gains (n_echo = 0), gal_synth_run_mpath, gal_synth_run_refl (refl_rows != null in the place of echo_rows),
// gal_synth_run_scint (scint_rows != null) and gal_synth_run_array (arr != null, iq_dev = its first output): the slot groups, one
// synthesis run per group, the scintillation of the parts that have one, then the weighted sum, the echo or reflector pass or the
// array pass
static int run_groups(const char *who, gal_synth_t *h, const gal_chan_epoch_t *params, int32_t n_epochs, const gal_chan_state_t *state_in,
                      const uint16_t *gain_q7, const int32_t *slot_of_echo, const gal_iq_echo_t *echo_rows, int32_t n_echo, int16_t *iq_dev,
                      gal_chan_state_t *state_out, const gal_iq_scint_t *scint_rows = nullptr, uint64_t first_sample = 0, const ArrayRun *arr = nullptr,
                      const gal_iq_refl_t *refl_rows = nullptr)
{
    if (!h || !params || !gain_q7 || !iq_dev || n_epochs < 1) return fail(GAL_E_INVAL, "%s: null argument or n_epochs %d (>= 1)", who, n_epochs);
    if ((uintptr_t)iq_dev & 15) return fail(GAL_E_INVAL, "%s: iq_dev must be 16-byte aligned", who);
    if (h->in_flight) return fail(GAL_E_STATE, "%s while a batch is in flight: call gal_synth_finish first", who);
    if (h->staged_pending)  // (gal_synth_plan would replace it silently: here the caller has not asked for a plan)
        return fail(GAL_E_STATE, "%s with a plan of gal_synth_plan_async waiting for its gal_synth_execute", who);
    const int E = n_epochs, S = h->cfg.n_slots;
    for (size_t i = 0; i < (size_t)E * S; ++i)
        if (gain_q7[i] > GAL_GAIN_MAX)
            return fail(GAL_E_INVAL, "%s: gain %u of epoch %zu, slot %zu (0..%d)", who, gain_q7[i], i / S, i % S, GAL_GAIN_MAX);
    // Slot groups: the slots of a group have the same gain in every epoch in which they are active, so one run of the existing path
    // with only those slots active is the part sum_s x_s of the group, and the group's gain of an epoch is that common value (first
    // fit; a slot that is never active joins no group).  All slots at one gain -- the unity case -- make one group
    struct Group {
        std::vector<int> slots;
        std::vector<int> g;  // [E]; -1: no slot of the group is active in that epoch
        bool solo = false;   // the one slot of the group carries an echo: no other slot joins it
    };
    std::vector<Group> groups;
    std::vector<int> group_of(S, -1);
    // a slot that carries an echo is a group of its own, idle or not: its part is what the echo delays, its line follows the slot
    std::vector<char> solo(S, 0);
    for (int r = 0; r < n_echo; ++r) solo[slot_of_echo[r]] = 1;
    const std::vector<char> has_echo = solo;
    // ... and so is a slot that scintillates in any epoch of the batch: its part is what gal_synth_iq_scint turns
    std::vector<char> fades(S, 0);
    bool any_fade = false;
    for (size_t i = 0; scint_rows && i < (size_t)E * S; ++i)
        if (!scint_identity(scint_rows[i])) fades[i % S] = solo[i % S] = 1, any_fade = true;
    // the end of the maximal run of epochs from e0 on in which slot s keeps one row: a job of gal_synth_iq_scint
    const auto row_run_end = [&](int s, int e0) {
        int e1 = e0 + 1;
        while (e1 < E && !memcmp(&scint_rows[(size_t)e1 * S + s], &scint_rows[(size_t)e0 * S + s], sizeof(gal_iq_scint_t))) ++e1;
        return e1;
    };
    // a job turns its part in place from the run's first sample on, and a pass starts on 16 bytes: refused here, before any run
    const uint64_t spe = (uint64_t)h->cfg.samples_per_epoch;
    for (int s = 0; s < S && any_fade; ++s)
        for (int e0 = 0; fades[s] && e0 < E; e0 = row_run_end(s, e0))
            if (!scint_identity(scint_rows[(size_t)e0 * S + s]) && ((e0 * spe) & 3))
                return fail(GAL_E_INVAL, "%s: the row of slot %d changes at epoch %d, %llu samples into the batch (a multiple of 4 only)", who, s, e0,
                            (unsigned long long)(e0 * spe));
    // ... and, for an array, every slot that is active in any epoch: its part is x_s itself, which the elements' weights turn
    for (size_t i = 0; arr && i < (size_t)E * S; ++i)
        if (params[i].prn > 0) solo[i % S] = 1;
    for (int s = 0; s < S; ++s) {
        bool active = solo[s];
        for (int e = 0; e < E && !active; ++e) active = params[(size_t)e * S + s].prn > 0;
        if (!active) continue;
        size_t k = solo[s] ? groups.size() : 0;
        for (; k < groups.size(); ++k) {
            bool fits = !groups[k].solo;
            for (int e = 0; e < E && fits; ++e)
                fits = params[(size_t)e * S + s].prn <= 0 || groups[k].g[e] < 0 || groups[k].g[e] == (int)gain_q7[(size_t)e * S + s];
            if (fits) break;
        }
        if (k == groups.size()) {
            groups.emplace_back();
            groups[k].g.assign(E, -1);
            groups[k].solo = solo[s];
        }
        groups[k].slots.push_back(s);
        group_of[s] = (int)k;
        for (int e = 0; e < E; ++e)
            if (params[(size_t)e * S + s].prn > 0) groups[k].g[e] = gain_q7[(size_t)e * S + s];
    }
    const int n_parts = groups.empty() ? 1 : (int)groups.size();  // (an empty sky: one run of nothing)
    bool unity = n_parts == 1 && n_echo == 0 && !any_fade && !arr;  // one part at gain 128 wherever it is not zero: y = x, the run goes straight into iq_dev
    if (!groups.empty())
        for (int e = 0; e < E && unity; ++e) unity = groups[0].g[e] < 0 || groups[0].g[e] == GAL_GAIN_UNITY;
    // a part's bytes, rounded up to the 16 that every pass asks of a buffer's start: the parts lie one behind the other in own_parts, and
    // a batch whose sample count is no multiple of 4 would put every second one on an address that gal_synth_execute refuses
    const size_t bytes = ((size_t)E * (size_t)h->cfg.samples_per_epoch * 4 + 15) & ~(size_t)15;
    // the weighted sum of the call before may still read the scratch buffers: wait for it here, whatever stream the handle is on now
    // (on one stream the runs below would order behind it by themselves)
    if (h->gain.sync.pending || h->mp.sync.pending || h->scint.sync.pending || h->array.sync.pending) {
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(h->gain.sync.wait());
        HIP_TRY(h->mp.sync.wait());
        HIP_TRY(h->scint.sync.wait());
        HIP_TRY(h->array.sync.wait());
    }
    h->gain_runs = 0;
    if (!unity && bytes * (size_t)n_parts > h->own_parts_bytes) {
        HIP_TRY(hipSetDevice(h->device));
        if (h->own_parts) hipFree(h->own_parts);
        h->own_parts = nullptr;
        h->own_parts_bytes = 0;
        if (hipMalloc(&h->own_parts, bytes * (size_t)n_parts) != hipSuccess) {
            (void)hipGetLastError();
            return fail(GAL_E_NOMEM, "%s: %d slot groups of %zu bytes each: hipMalloc of %zu bytes of scratch failed", who, n_parts, bytes,
                        bytes * (size_t)n_parts);
        }
        h->own_parts_bytes = bytes * (size_t)n_parts;
    }
    std::vector<gal_chan_epoch_t> one((size_t)E * S);
    std::vector<gal_chan_state_t> st_k(S), st_all(S);
    const int16_t *parts[GAL_ENGINE_MAX_CHAN];
    for (int k = 0; k < n_parts; ++k) {
        memcpy(one.data(), params, sizeof(gal_chan_epoch_t) * (size_t)E * S);
        for (int e = 0; e < E; ++e)
            for (int s = 0; s < S; ++s)
                if (group_of[s] != k) one[(size_t)e * S + s].prn = 0;
        int16_t *dst = unity ? iq_dev : (int16_t *)((char *)h->own_parts + bytes * (size_t)k);
        parts[k] = dst;
        int rc = gal_synth_plan(h, one.data(), E, state_in);
        if (rc == GAL_OK) rc = gal_synth_execute(h, dst);
        if (rc == GAL_OK) rc = gal_synth_finish_n(h, st_k.data(), nullptr, 0);
        if (rc != GAL_OK) return rc;
        h->gain_runs += 1;
        // the end state of a slot is that of its own run; a slot that is never active is idle in every run (the first one's record)
        for (int s = 0; s < S; ++s)
            if (group_of[s] == k || (k == 0 && group_of[s] < 0)) st_all[s] = st_k[s];
    }
    if (any_fade) {
        // one job per slot and maximal run of epochs with an equal row, in place on the slot's part; all jobs in one call (of 64)
        std::vector<gal_scint_job_t> jobs;
        for (int s = 0; s < S; ++s) {
            if (!fades[s]) continue;
            for (int e0 = 0, e1; e0 < E; e0 = e1) {
                const gal_iq_scint_t &row = scint_rows[(size_t)e0 * S + s];
                e1 = row_run_end(s, e0);
                if (scint_identity(row)) continue;
                gal_scint_job_t j;
                memset(&j, 0, sizeof(j));
                j.out_dev = (int16_t *)((char *)h->own_parts + bytes * (size_t)group_of[s]) + 2 * e0 * spe;
                j.in_dev = j.out_dev;
                j.n_samples = (uint64_t)(e1 - e0) * spe;
                j.first_sample = first_sample + e0 * spe;
                j.row = row;
                jobs.push_back(j);
            }
        }
        for (size_t at = 0; at < jobs.size(); at += GAL_SCINT_MAX_JOBS) {
            const int rc = gal_synth_iq_scint(h, jobs.data() + at, (int32_t)std::min<size_t>(GAL_SCINT_MAX_JOBS, jobs.size() - at));
            if (rc != GAL_OK) return rc;
        }
    }
    if (arr) {
        // the weight of (epoch, element, part): that of the part's one slot, (0, 0) where it is idle (and for the one part of an empty sky)
        const int K = arr->n_elem;
        std::vector<gal_iq_steer_t> w((size_t)E * K * n_parts);  // (value-initialised: zeros)
        for (int e = 0; e < E; ++e)
            for (int a = 0; a < K; ++a)
                for (size_t k = 0; k < groups.size(); ++k) {
                    const int s = groups[k].slots[0];
                    if (params[(size_t)e * S + s].prn <= 0) continue;
                    GAL_TRY(gal_synth_steer_make(gain_q7[(size_t)e * S + s], arr->phase[((size_t)e * K + a) * S + s], &w[((size_t)e * K + a) * n_parts + k]));
                }
        GAL_TRY(gal_synth_iq_array(h, parts, n_parts, w.data(), E, K, arr->out_dev));
    } else if (!unity) {
        std::vector<uint16_t> gp((size_t)E * n_parts);
        for (int e = 0; e < E; ++e)
            for (int k = 0; k < n_parts; ++k) gp[(size_t)e * n_parts + k] = (uint16_t)(groups[k].g[e] < 0 ? 0 : groups[k].g[e]);
        int rc;
        if (n_echo > 0) {
            std::vector<int32_t> hist_id(n_parts, -1), part_of(n_echo);
            for (int k = 0; k < n_parts; ++k)
                if (groups[k].solo && has_echo[groups[k].slots[0]]) hist_id[k] = groups[k].slots[0];
            for (int r = 0; r < n_echo; ++r) part_of[r] = group_of[slot_of_echo[r]];
            rc = refl_rows ? gal_synth_iq_refl(h, parts, n_parts, hist_id.data(), gp.data(), E, part_of.data(), refl_rows, n_echo, iq_dev)
                           : gal_synth_iq_mpath(h, parts, n_parts, hist_id.data(), gp.data(), E, part_of.data(), echo_rows, n_echo, iq_dev);
        } else {
            rc = gal_synth_iq_wsum(h, parts, n_parts, gp.data(), E, iq_dev);
        }
        if (rc != GAL_OK) return rc;
    }
    if (state_out) memcpy(state_out, st_all.data(), sizeof(gal_chan_state_t) * S);
    return GAL_OK;
}

int gal_synth_run_gains(gal_synth_t *h, const gal_chan_epoch_t *params, int32_t n_epochs, const gal_chan_state_t *state_in,
                        const uint16_t *gain_q7, int16_t *iq_dev, gal_chan_state_t *state_out)
{
    return run_groups("gal_synth_run_gains", h, params, n_epochs, state_in, gain_q7, nullptr, nullptr, 0, iq_dev, state_out);
}

int gal_synth_run_mpath(gal_synth_t *h, const gal_chan_epoch_t *params, int32_t n_epochs, const gal_chan_state_t *state_in,
                        const uint16_t *gain_q7, const int32_t *slot_of_echo, const gal_iq_echo_t *echo_rows, int32_t n_echo, int16_t *iq_dev,
                        gal_chan_state_t *state_out)
{
    const char *who = "gal_synth_run_mpath";
    if (n_echo == 0) return run_groups(who, h, params, n_epochs, state_in, gain_q7, nullptr, nullptr, 0, iq_dev, state_out);
    if (!h) return fail(GAL_E_INVAL, "%s: null handle", who);
    if (h->cfg.n_slots > GAL_ECHO_LINES) return fail(GAL_E_INVAL, "%s: %d slots, more than the %d history lines", who, h->cfg.n_slots, GAL_ECHO_LINES);
    const int rc = gal_synth_mpath_check(echo_rows, n_echo, n_epochs, slot_of_echo, h->cfg.n_slots);
    if (rc) return rc;
    return run_groups(who, h, params, n_epochs, state_in, gain_q7, slot_of_echo, echo_rows, n_echo, iq_dev, state_out);
}

int gal_synth_run_refl(gal_synth_t *h, const gal_chan_epoch_t *params, int32_t n_epochs, const gal_chan_state_t *state_in,
                       const uint16_t *gain_q7, const int32_t *slot_of_echo, const gal_iq_refl_t *refl_rows, int32_t n_echo, int16_t *iq_dev,
                       gal_chan_state_t *state_out)
{
    const char *who = "gal_synth_run_refl";
    if (n_echo == 0) return run_groups(who, h, params, n_epochs, state_in, gain_q7, nullptr, nullptr, 0, iq_dev, state_out);
    if (!h) return fail(GAL_E_INVAL, "%s: null handle", who);
    if (h->cfg.n_slots > GAL_ECHO_LINES) return fail(GAL_E_INVAL, "%s: %d slots, more than the %d history lines", who, h->cfg.n_slots, GAL_ECHO_LINES);
    GAL_TRY(gal_synth_refl_check(refl_rows, n_echo, n_epochs, slot_of_echo, h->cfg.n_slots));
    return run_groups(who, h, params, n_epochs, state_in, gain_q7, slot_of_echo, nullptr, n_echo, iq_dev, state_out, nullptr, 0, nullptr, refl_rows);
}

int gal_synth_run_scint(gal_synth_t *h, const gal_chan_epoch_t *params, int32_t n_epochs, const gal_chan_state_t *state_in,
                        const uint16_t *gain_q7, const int32_t *slot_of_echo, const gal_iq_echo_t *echo_rows, int32_t n_echo,
                        const gal_iq_scint_t *scint_rows, uint64_t first_sample, int16_t *iq_dev, gal_chan_state_t *state_out)
{
    const char *who = "gal_synth_run_scint";
    if (!scint_rows) return gal_synth_run_mpath(h, params, n_epochs, state_in, gain_q7, slot_of_echo, echo_rows, n_echo, iq_dev, state_out);
    if (!h) return fail(GAL_E_INVAL, "%s: null handle", who);
    if (n_epochs < 1) return fail(GAL_E_INVAL, "%s: n_epochs %d (>= 1)", who, n_epochs);
    const uint64_t total = (uint64_t)n_epochs * (uint64_t)h->cfg.samples_per_epoch;
    if (first_sample >> 62 || (first_sample + total) >> 62) return fail(GAL_E_INVAL, "%s: the batch must end below sample 2^62", who);
    for (size_t i = 0; i < (size_t)n_epochs * h->cfg.n_slots; ++i) GAL_TRY(gal_synth_scint_check(&scint_rows[i]));
    if (n_echo != 0) {
        if (h->cfg.n_slots > GAL_ECHO_LINES) return fail(GAL_E_INVAL, "%s: %d slots, more than the %d history lines", who, h->cfg.n_slots, GAL_ECHO_LINES);
        GAL_TRY(gal_synth_mpath_check(echo_rows, n_echo, n_epochs, slot_of_echo, h->cfg.n_slots));
    }
    return run_groups(who, h, params, n_epochs, state_in, gain_q7, n_echo ? slot_of_echo : nullptr, n_echo ? echo_rows : nullptr, n_echo, iq_dev, state_out,
                      scint_rows, first_sample);
}

int gal_synth_run_array(gal_synth_t *h, const gal_chan_epoch_t *params, int32_t n_epochs, const gal_chan_state_t *state_in,
                        const uint16_t *gain_q7, const uint32_t *phase, int32_t n_elem, const gal_iq_scint_t *scint_rows,
                        uint64_t first_sample, int16_t *const *out_dev, gal_chan_state_t *state_out)
{
    const char *who = "gal_synth_run_array";
    if (!h || !params || !gain_q7 || !phase || !out_dev || n_epochs < 1) return fail(GAL_E_INVAL, "%s: null argument or n_epochs %d (>= 1)", who, n_epochs);
    if (n_elem < 1 || n_elem > GAL_ARRAY_MAX_ELEM) return fail(GAL_E_INVAL, "%s: n_elem %d (1..%d)", who, n_elem, GAL_ARRAY_MAX_ELEM);
    const size_t S = (size_t)h->cfg.n_slots, bytes = (size_t)n_epochs * (size_t)h->cfg.samples_per_epoch * 4;
    for (size_t i = 0; i < (size_t)n_epochs * S; ++i)
        if (gain_q7[i] > GAL_STEER_GAIN_MAX)
            return fail(GAL_E_INVAL, "%s: gain %u of slot %zu in epoch %zu (0..%d: +18 dB over unity)", who, gain_q7[i], i % S, i / S, GAL_STEER_GAIN_MAX);
    GAL_TRY(check_outputs(who, out_dev, n_elem, bytes));  // before the synthesis runs: what gal_synth_iq_array would refuse behind them
    if (scint_rows) {
        const uint64_t total = (uint64_t)n_epochs * (uint64_t)h->cfg.samples_per_epoch;
        if (first_sample >> 62 || (first_sample + total) >> 62) return fail(GAL_E_INVAL, "%s: the batch must end below sample 2^62", who);
        for (size_t i = 0; i < (size_t)n_epochs * S; ++i) GAL_TRY(gal_synth_scint_check(&scint_rows[i]));
    }
    const ArrayRun arr = {phase, n_elem, out_dev};
    return run_groups(who, h, params, n_epochs, state_in, gain_q7, nullptr, nullptr, 0, out_dev[0], state_out, scint_rows, first_sample, &arr);
}

int gal_synth_gain_runs(const gal_synth_t *h, int32_t *n_runs)
{
    if (!h || !n_runs) return fail(GAL_E_INVAL, "gal_synth_gain_runs: null argument");
    *n_runs = h->gain_runs;
    return GAL_OK;
}

// ---- correlator bank and C/N0 monitor (iq_corr.hip) --------------------------------------------------------------------------
static constexpr uint64_t kCorrL = (uint64_t)(2 * GAL_CODE_LEN) << 32;  // one code period: 8184 half chips x 2^32

// nullptr: the request is fine; otherwise what is wrong with it
static const char *corr_req_fault(const gal_corr_req_t *q)
{
    if (q->prn < 1 || q->prn > GAL_NUM_PRN) return "prn outside 1..50";
    if (q->max_periods < 1 || q->max_periods > 1024) return "max_periods outside 1..1024";
    if (q->code_ph0 >= kCorrL) return "code_ph0 outside [0, 8184 x 2^32)";
    if (q->code_dph > ((uint64_t)1 << 32)) return "code_dph above 2^32 (one half chip per sample)";
    if (q->delay_step < 1) return "delay_step below 1";
    if (q->n_delay < 1 || q->n_delay > 2 * GAL_CODE_LEN) return "n_delay outside 1..8184";
    if (q->n_dopp < 1 || q->n_dopp > 64) return "n_dopp outside 1..64";
    return nullptr;
}

size_t gal_synth_corr_out_bytes(const gal_corr_req_t *req)
{
    if (!req || req->max_periods < 1 || req->max_periods > 1024 || req->n_delay < 1 || req->n_delay > 2 * GAL_CODE_LEN || req->n_dopp < 1 ||
        req->n_dopp > 64)
        return 0;
    return (size_t)req->max_periods * (size_t)req->n_dopp * (size_t)req->n_delay * 4 * sizeof(int64_t);
}

int gal_synth_correlate(gal_synth_t *h, const void *buf_dev, int32_t format, size_t n_samples, const gal_corr_req_t *reqs, int32_t n_req,
                        int64_t *out_dev)
{
    if (!h) return fail(GAL_E_INVAL, "null handle");
    if (format != GAL_IQ_ISHORT && format != GAL_IQ_IBYTE && format != GAL_IQ_IBIT)
        return fail(GAL_E_INVAL, "gal_synth_correlate: unknown format %d (GAL_IQ_ISHORT 0, GAL_IQ_IBYTE 1, GAL_IQ_IBIT 2)", format);
    if (!buf_dev || !out_dev || !reqs || ((uintptr_t)buf_dev & 15) || ((uintptr_t)out_dev & 15))
        return fail(GAL_E_INVAL, "gal_synth_correlate: pointers must be non-null, the device pointers 16-byte aligned");
    if (n_req < 1 || n_req > GAL_CORR_MAX_REQ) return fail(GAL_E_INVAL, "gal_synth_correlate: %d requests (1..%d)", n_req, GAL_CORR_MAX_REQ);
    if (n_samples == 0 || n_samples > ((size_t)1 << 32)) return fail(GAL_E_INVAL, "gal_synth_correlate: n_samples %zu (1..2^32)", n_samples);
    size_t total = 0;
    for (int r = 0; r < n_req; ++r) {
        const char *what = corr_req_fault(&reqs[r]);
        if (what) return fail(GAL_E_INVAL, "gal_synth_correlate: request %d: %s", r, what);
        // P(n) = code_ph0 + n code_dph must stay below 2^64 for every n < n_samples
        if (reqs[r].code_dph && (uint64_t)(n_samples - 1) > (UINT64_MAX - reqs[r].code_ph0) / reqs[r].code_dph)
            return fail(GAL_E_INVAL, "gal_synth_correlate: request %d: the code phase overflows 64 bits within %zu samples", r, n_samples);
        total += gal_synth_corr_out_bytes(&reqs[r]);
        if (total > GAL_CORR_MAX_OUT_BYTES)
            return fail(GAL_E_INVAL, "gal_synth_correlate: the requests take more than %zu bytes of output", (size_t)GAL_CORR_MAX_OUT_BYTES);
    }
    const size_t buf_bytes = gal_synth_iq_bytes(format, n_samples);
    if (ranges_overlap(buf_dev, buf_bytes, out_dev, total)) return fail(GAL_E_INVAL, "gal_synth_correlate: buffer and output overlap");
    GAL_TRY(check_in_flight("gal_synth_correlate", h, buf_dev, buf_bytes, "buffer of"));
    GAL_TRY(check_in_flight("gal_synth_correlate", h, out_dev, total, "buffer of"));
    hipStream_t st;
    GAL_TRY(enter(h, &st, false));
    if (!h->d_corr_tab) {
        // [512] cos | sin << 16, then per PRN 8184 half chips x 2 bits: bit 2 (h & 15) of word h >> 4 = (b[h] < 0), the next one (c[h] < 0);
        // b[h] = (E1B chip: set bit -1) x (sboc: even half chip -1), as the synthesis kernels take them out of the same tables
        const int16_t *const g_cos = gal_tables_cos512(), *const g_sin = gal_tables_sin512();
        const uint32_t(*const kE1B)[128] = (const uint32_t(*)[128])gal_tables_e1b();
        const uint32_t(*const kE1C)[128] = (const uint32_t(*)[128])gal_tables_e1c();
        std::vector<uint32_t> tab(512 + 50 * 512, 0u);
        for (int k = 0; k < 512; ++k) tab[k] = (uint32_t)(uint16_t)g_cos[k] | ((uint32_t)(uint16_t)g_sin[k] << 16);
        for (int prn = 0; prn < 50; ++prn)
            for (int hc = 0; hc < 2 * GAL_CODE_LEN; ++hc) {
                const int chip = hc >> 1;
                const uint32_t b = (kE1B[prn][chip >> 5] >> (chip & 31)) & 1u, c = (kE1C[prn][chip >> 5] >> (chip & 31)) & 1u;
                const uint32_t even = (uint32_t)(~hc & 1);
                tab[512 + prn * 512 + (hc >> 4)] |= ((b ^ even) | ((c ^ even) << 1)) << (2 * (hc & 15));
            }
        uint32_t *d = nullptr;
        HIP_TRY(hipMalloc((void **)&d, tab.size() * sizeof(uint32_t)));
        const hipError_t err = hipMemcpy(d, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (err != hipSuccess) {
            hipFree(d);
            return fail(GAL_E_DEVICE, "gal_synth_correlate: table upload failed: %s", hipGetErrorString(err));
        }
        h->d_corr_tab = d;
    }
    HIP_TRY(hipMemsetAsync(out_dev, 0, total, st));
    size_t off = 0;
    for (int r = 0; r < n_req; ++r) {  // the request travels as kernel arguments: copied when this returns
        const gal_corr_req_t &q = reqs[r];
        // the first sample of period max_periods: nothing from there on is wanted
        uint64_t n_eff = n_samples;
        if (q.code_dph) {
            const uint64_t span = (uint64_t)q.max_periods * kCorrL - q.code_ph0;  // > 0
            const uint64_t first = (span + q.code_dph - 1) / q.code_dph;
            if (first < n_eff) n_eff = first;
        }
        HIP_TRY(galk_launch_corr(format, buf_dev, n_eff, q.code_ph0, q.code_dph, q.carr_ph0, (uint32_t)q.carr_dph + (uint32_t)q.dopp0,
                                 (uint32_t)q.dopp_step, q.delay0, q.delay_step, q.n_delay, q.n_dopp, q.max_periods, h->d_corr_tab,
                                 h->d_corr_tab + 512 + (size_t)(q.prn - 1) * 512, (long long *)((char *)out_dev + off), st));
        off += gal_synth_corr_out_bytes(&q);
    }
    return GAL_OK;
}

int gal_corr_from_epoch(const gal_chan_epoch_t *rec, double sample_rate, int64_t sample_offset, gal_corr_req_t *out)
{
    if (!rec || !out) return fail(GAL_E_INVAL, "gal_corr_from_epoch: null argument");
    if (rec->prn < 1 || rec->prn > GAL_NUM_PRN) return fail(GAL_E_INVAL, "gal_corr_from_epoch: prn %d (1..50)", rec->prn);
    if (sample_offset < 0 || sample_offset > ((int64_t)1 << 32)) return fail(GAL_E_INVAL, "gal_corr_from_epoch: sample_offset outside 0..2^32");
    if (!std::isfinite(sample_rate) || sample_rate <= 0.0 || !std::isfinite(rec->f_code) || !std::isfinite(rec->f_carr) ||
        !std::isfinite(rec->code_phase0) || !std::isfinite(rec->carr_phase0))
        return fail(GAL_E_INVAL, "gal_corr_from_epoch: a rate or phase is not finite, or sample_rate <= 0");
    const double two32 = 4294967296.0;
    const double dph = 2.0 * rec->f_code / sample_rate * two32, cdph = rec->f_carr / sample_rate * two32;
    if (!(dph >= 0.0 && dph <= two32)) return fail(GAL_E_INVAL, "gal_corr_from_epoch: f_code %g outside [0, sample_rate / 2]", rec->f_code);
    if (!(std::fabs(cdph) < 2147483647.5)) return fail(GAL_E_INVAL, "gal_corr_from_epoch: |f_carr| %g is not below sample_rate / 2", rec->f_carr);
    if (!(rec->code_phase0 >= 0.0 && rec->code_phase0 < 3.0 * GAL_CODE_LEN))
        return fail(GAL_E_INVAL, "gal_corr_from_epoch: code_phase0 %g outside [0, 3 x 4092)", rec->code_phase0);
    out->prn = rec->prn;
    out->code_dph = (uint64_t)llround(dph);
    const unsigned __int128 p = (unsigned __int128)(uint64_t)llround(2.0 * rec->code_phase0 * two32) +
                                (unsigned __int128)(uint64_t)sample_offset * out->code_dph;
    out->code_ph0 = (uint64_t)(p % kCorrL);
    out->carr_dph = (int32_t)llround(cdph);
    out->carr_ph0 = 0;
    if (rec->flags & GAL_CH_RESTART) {
        const double fr = rec->carr_phase0 - std::floor(rec->carr_phase0);
        out->carr_ph0 = (uint32_t)((uint64_t)llround(fr * two32) + (uint64_t)sample_offset * (uint64_t)(int64_t)out->carr_dph);
    }
    return GAL_OK;
}

int gal_corr_cn0(const int64_t *out_host, const gal_corr_req_t *req, int32_t k_prompt, int32_t k_noise, int32_t d, double sample_rate,
                 double *cn0_dbhz, double *peak_ratio)
{
    if (!out_host || !req || !cn0_dbhz || !peak_ratio) return fail(GAL_E_INVAL, "gal_corr_cn0: null argument");
    if (gal_synth_corr_out_bytes(req) == 0 || req->max_periods < 3 || req->code_dph == 0 || k_prompt < 0 || k_prompt >= req->n_delay ||
        k_noise < 0 || k_noise >= req->n_delay || d < 0 || d >= req->n_dopp || !std::isfinite(sample_rate) || sample_rate <= 0.0)
        return fail(GAL_E_INVAL, "gal_corr_cn0: a grid outside the caps, fewer than 3 periods, code_dph 0, an index outside the grid or a bad sample rate");
    double pp = 0.0, pn = 0.0;
    for (int m = 1; m < req->max_periods - 1; ++m) {
        const int64_t *a = out_host + (((size_t)m * req->n_dopp + d) * req->n_delay + k_prompt) * 4;
        const int64_t *b = out_host + (((size_t)m * req->n_dopp + d) * req->n_delay + k_noise) * 4;
        for (int r = 0; r < 4; ++r) {
            pp += (double)a[r] * (double)a[r];
            pn += (double)b[r] * (double)b[r];
        }
    }
    const int M = req->max_periods - 2;
    pp /= M;
    pn /= M;
    *cn0_dbhz = 0.0;
    *peak_ratio = pn > 0.0 ? pp / pn : 0.0;
    if (!(pp > pn) || !(pn > 0.0)) return fail(GAL_E_INVAL, "gal_corr_cn0: no peak (Pp %g <= Pn %g)", pp, pn);
    const double T = (double)kCorrL / (double)req->code_dph / sample_rate;
    *cn0_dbhz = 10.0 * log10((pp - pn) / (pn * T / 2.0));
    return GAL_OK;
}

// ---- Welch power spectrum (iq_psd.hip) -----------------------------------------------------------------------------------------
// nullptr: the configuration is fine; otherwise what is wrong with it
static const char *psd_cfg_fault(const gal_iq_psd_t *c)
{
    if (c->log2_n < 3 || c->log2_n > 12) return "log2_n outside 3..12";
    if (c->hop < 1 || c->hop > (1 << c->log2_n)) return "hop outside 1..N";
    if (c->window != 0 && c->window != 1) return "window is neither 0 (rectangular) nor 1 (Hann)";
    if (c->reserved != 0) return "reserved is not 0";
    return nullptr;
}

int64_t gal_synth_psd_segments(const gal_iq_psd_t *cfg, size_t n_samples)
{
    if (!cfg || psd_cfg_fault(cfg)) return 0;
    const uint64_t N = (uint64_t)1 << cfg->log2_n;
    if (n_samples < N) return 0;
    const uint64_t n_seg = ((uint64_t)n_samples - N) / (uint64_t)cfg->hop + 1;
    if (n_seg > (((uint64_t)1 << 32) >> (2 * cfg->log2_n))) return 0;  // n_seg N^2 <= 2^32: no bin's sum passes 2^63
    return (int64_t)n_seg;
}

int gal_synth_iq_psd(gal_synth_t *h, const void *buf_dev, int32_t format, size_t n_samples, const gal_iq_psd_t *cfg, uint64_t *out_dev,
                     int32_t *n_seg)
{
    static const char *const who = "gal_synth_iq_psd";
    if (!h) return fail(GAL_E_INVAL, "null handle");
    if (format != GAL_IQ_ISHORT && format != GAL_IQ_IBYTE && format != GAL_IQ_IBIT)
        return fail(GAL_E_INVAL, "%s: format %d (GAL_IQ_ISHORT 0, GAL_IQ_IBYTE 1, GAL_IQ_IBIT 2; GAL_IQ_I2BIT is the AGC's alone)", who, format);
    if (!cfg || !n_seg) return fail(GAL_E_INVAL, "%s: null cfg or n_seg", who);
    GAL_TRY(check_aligned(who, buf_dev));
    GAL_TRY(check_aligned(who, out_dev));
    const char *what = psd_cfg_fault(cfg);
    if (what) return fail(GAL_E_INVAL, "%s: %s", who, what);
    const int64_t segs = gal_synth_psd_segments(cfg, n_samples);
    if (segs <= 0)
        return fail(GAL_E_INVAL, "%s: %zu samples hold no segment of %d, or more than 2^32 / N^2 = %llu of them", who, n_samples, 1 << cfg->log2_n,
                    (unsigned long long)(((uint64_t)1 << 32) >> (2 * cfg->log2_n)));
    const size_t buf_bytes = gal_synth_iq_bytes(format, n_samples), out_bytes = sizeof(uint64_t) << cfg->log2_n;
    GAL_TRY(check_overlap(who, buf_dev, buf_bytes, out_dev, out_bytes, false, ""));
    GAL_TRY(check_in_flight(who, h, buf_dev, buf_bytes, "buffer of"));
    GAL_TRY(check_in_flight(who, h, out_dev, out_bytes, "buffer of"));
    hipStream_t st;
    GAL_TRY(enter(h, &st, false));
    HIP_TRY(hipMemsetAsync(out_dev, 0, out_bytes, st));
    HIP_TRY(galk_launch_psd(format, buf_dev, (uint64_t)segs, cfg->log2_n, cfg->hop, cfg->window, (unsigned long long *)out_dev, st));
    *n_seg = (int32_t)segs;
    return GAL_OK;
}

}  // extern "C"
