// gain_q7.h -- the per-satellite gain of include/galsynth.h (gal_synth_gain_q7) as ONE inline function, compiled into libgalsynth.so
// (the entry point itself) and into libgalscen.so (gal_scen_next_gains): the two libraries do not link each other, and the value must
// be the same double arithmetic in both.  Host only.
//
// The reference computes it once per channel and epoch, src/galileo-sdr.cpp:469-477 (and never applies it, :520-521):
//     path_loss = 20200000.0 / rho.d;  ibs = (int)((90.0 - rho.azel[1] * R2D) / 5.0);  gain = (int)(path_loss * ant_pat[ibs] * 128.0)
// Here the reference distance is Galileo's nominal altitude (the reference's 20 200 km is the GPS altitude of gps-sdr-sim: every
// Galileo satellite would sit 1.2 dB or more under unity), the pattern is given in dB of attenuation as the reference's table is
// before its conversion (src/galileo-sdr.cpp:365), and a per-PRN offset in dB is added.  The truncation is the reference's.
#ifndef GAL_GAIN_Q7_H_
#define GAL_GAIN_Q7_H_

#include <math.h>

#define GAL_GAIN_REF_DISTANCE_M 23222000.0
#define GAL_GAIN_R2D 57.2957795131 /* the reference's R2D, include/constants.h:178 */

// d_m > 0 and every argument finite (the callers check); pattern_db: 37 values or null (isotropic)
static inline int gal_gain_q7_eval(double d_m, double elev_rad, const double *pattern_db, double offset_db)
{
    const double off = (90.0 - elev_rad * GAL_GAIN_R2D) / 5.0;
    const int ibs = off <= 0.0 ? 0 : off >= 36.0 ? 36 : (int)off;
    const double ant = pattern_db ? pow(10.0, -pattern_db[ibs] / 20.0) : 1.0;
    const double v = 128.0 * (GAL_GAIN_REF_DISTANCE_M / d_m) * ant * pow(10.0, offset_db / 20.0);
    return v >= 32767.0 ? 32767 : (int)v;
}

#endif
