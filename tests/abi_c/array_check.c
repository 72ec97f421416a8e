/* The antenna array's part of the two headers as plain C99: layouts by _Static_assert, and the entry points that need no GPU, linked
 * against both libraries (tests/test_iq_array_cpu.py compiles and runs this as tests/test_abi.py does abi_check.c). */
#include <stddef.h>
#include <stdio.h>

#include "galscen.h"
#include "galsynth.h"

_Static_assert(sizeof(gal_iq_steer_t) == 4, "gal_iq_steer_t is 4 bytes");
_Static_assert(offsetof(gal_iq_steer_t, w_re) == 0 && offsetof(gal_iq_steer_t, w_im) == 2, "gal_iq_steer_t: w_re, w_im");
_Static_assert(GAL_ARRAY_MAX_ELEM == 8 && GAL_STEER_GAIN_MAX == 1023, "the array's limits");

int main(void)
{
    gal_iq_steer_t w = {1, 1}, rows[2] = {{4096, 0}, {0, -32767}};
    const double origin[3] = {0.0, 0.0, 0.0};
    uint32_t phase = 1;
    int32_t (*next_azel)(gal_scen_t *, int32_t, gal_chan_epoch_t *, uint16_t *, double *) = gal_scen_next_azel;
    if (gal_synth_steer_make(GAL_GAIN_UNITY, 0, &w) != GAL_OK || w.w_re != 4096 || w.w_im != 0) return 1;
    if (gal_synth_steer_make(GAL_STEER_GAIN_MAX + 1, 0, &w) != GAL_E_INVAL) return 2;
    if (gal_synth_steer_check(rows, 1, 1, 2) != GAL_OK || gal_synth_steer_check(rows, 1, 2, 1) != GAL_OK) return 3;
    rows[1].w_re = -32767 - 1;
    if (gal_synth_steer_check(rows, 1, 1, 2) != GAL_E_INVAL) return 4;
    if (gal_synth_array_phase(origin, 1.0, 0.5, &phase) != GAL_OK || phase != 0) return 5;
    if (gal_synth_iq_array(NULL, NULL, 1, rows, 1, 1, NULL) != GAL_E_INVAL) return 6;
    if (gal_synth_run_array(NULL, NULL, 1, NULL, NULL, NULL, 1, NULL, 0, NULL, NULL) != GAL_E_INVAL) return 7;
    if (next_azel(NULL, 1, NULL, NULL, NULL) != GAL_E_INVAL) return 8;
    printf("array ok\n");
    return 0;
}
