"""ctypes mirror of include/galsynth.h -- the drop-in boundary of the reference's per-sample loop
(reference src/galileo-sdr.cpp:481-539).  Same names, same argument meaning, same error behaviour as
the C-ABI; records travel as numpy structured arrays whose layout IS the C struct layout.

There is no CPU implementation behind this module: if libgalsynth.so is missing, or no gfx950 device is
usable, every entry point raises.
"""
import ctypes
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libgalsynth.so")
# the same sources built with -DGAL_TEST_HOOKS (fault injection for the repair-path tests; tests only)
HOOKS_LIB_PATH = os.path.join(PKG_DIR, "libgalsynth_hooks.so")
GAL_CFG_SINGLE_STREAM = 1
GAL_CFG_EXACT_REPLAY = 4  # always the exact-replay kernel (k_synth), also where k_synth_g could run
GAL_CFG_VERIFY_ALL = 8  # accepted and ignored since 0.4: full verification is the default
GAL_CFG_VERIFY_SAMPLED = 16  # k_synth_g batches: re-walk a rotating eighth of the leg positions of both chains per batch (default: every leg)
GAL_CFG_CBOC = 2  # opt-in CBOC(6,1,1/11) sub-carrier (not in the reference; defined by the oracle's CBOC mode)

GAL_CH_RESTART = 1
# output formats (gal_synth_iq_convert): interleaved int16, int8 (rounded shift, symmetric clamp), 1 bit (MSB first)
GAL_IQ_ISHORT = 0
GAL_IQ_IBYTE = 1
GAL_IQ_IBIT = 2
IQ_FORMATS = {"ishort": GAL_IQ_ISHORT, "ibyte": GAL_IQ_IBYTE, "ibit": GAL_IQ_IBIT}
IQ_SHIFT_DEFAULT = 5  # ibyte: the CLI's default --iq-shift
GAL_PAGE_WORDS = 16
GAL_N_SYM_PAGE = 500
# per-satellite signal power (gal_synth_run_gains): Q7 gains in a uint16, 128 = unity
GAL_GAIN_UNITY = 128
GAL_GAIN_MAX = 32767
GAL_GAIN_PATTERN_LEN = 37
GAL_FIR_MAX_TAPS = 128  # front-end filter (gal_synth_fir_set): taps in Q14
GAL_FIR_UNITY = 16384
GAL_FIRDEC_MAX_TAPS = 512  # decimating front-end filter (gal_synth_firdec_set)
GAL_FIRDEC_MAX_DECIM = 16
GAL_ENGINE_MAX_CHAN = 64
# block AGC and 2-bit quantiser (gal_synth_agc_set, gal_synth_iq_agc): the 2-bit format is a format of the AGC call only
GAL_IQ_I2BIT = 3
AGC_FORMATS = {"ishort": GAL_IQ_ISHORT, "ibyte": GAL_IQ_IBYTE, "i2bit": GAL_IQ_I2BIT}
GAL_AGC_MIN_BLOCK = 16
GAL_AGC_MAX_BLOCK = 65536
GAL_AGC_MAX_WINDOW = 64
GAL_AGC_MAX_SPAN = 65536
GAL_AGC_GAIN_UNITY = 4096
GAL_AGC_GAIN_MAX = 1 << 24
I2BIT_THRESHOLD_DEFAULT = 1024  # the CLI's default --i2bit-threshold

# gal_chan_epoch_t (176 bytes)
CHAN_EPOCH_DTYPE = np.dtype(
    [
        ("prn", "<i4"),
        ("ibit0", "<i4"),
        ("flags", "<u4"),
        ("reserved", "<u4"),
        ("f_carr", "<f8"),
        ("f_code", "<f8"),
        ("code_phase0", "<f8"),
        ("carr_phase0", "<f8"),
        ("page_next", "<u4", (GAL_PAGE_WORDS,)),
        ("page_init", "<u4", (GAL_PAGE_WORDS,)),
    ],
    align=True,
)
assert CHAN_EPOCH_DTYPE.itemsize == 176

# gal_chan_state_t (80 bytes)
CHAN_STATE_DTYPE = np.dtype(
    [("carr_phase", "<f8"), ("page", "<u4", (GAL_PAGE_WORDS,)), ("prn", "<i4"), ("reserved", "<i4")], align=True
)
assert CHAN_STATE_DTYPE.itemsize == 80


class _Cfg(ctypes.Structure):
    _fields_ = [
        ("sample_rate", ctypes.c_double),
        ("samples_per_epoch", ctypes.c_int32),
        ("n_slots", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("chunk_samples", ctypes.c_int32),
        ("max_walk_passes", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("reserved", ctypes.c_int32 * 2),
    ]


class _Stats(ctypes.Structure):
    _fields_ = [
        ("walk_passes", ctypes.c_int32),
        ("chain_mismatch", ctypes.c_int32),
        ("n_epochs", ctypes.c_int32),
        ("n_active_max", ctypes.c_int32),
        ("chunk_samples", ctypes.c_int32),
        ("chunks_per_epoch", ctypes.c_int32),
        ("ms_walk", ctypes.c_float),
        ("ms_synth", ctypes.c_float),
        ("window_mode", ctypes.c_int32),
        ("synth_runs", ctypes.c_int32),
        ("kernel_family", ctypes.c_int32),
        ("repaired_groups", ctypes.c_int32),
        ("ms_repair", ctypes.c_float),
        ("exact_records", ctypes.c_int32),
        ("ms_plan", ctypes.c_float),
        ("ms_h2d", ctypes.c_float),
    ]


class _Noise(ctypes.Structure):  # gal_iq_noise_t
    _fields_ = [
        ("seed", ctypes.c_uint64),
        ("stream", ctypes.c_uint32),
        ("gain_q16", ctypes.c_uint32),
        ("sigma_q4", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class _Interf(ctypes.Structure):  # gal_iq_interf_t (32 bytes)
    _fields_ = [
        ("amp_q4", ctypes.c_uint32),
        ("ph0", ctypes.c_uint32),
        ("f0", ctypes.c_int32),
        ("df", ctypes.c_int32),
        ("sweep_len", ctypes.c_uint32),
        ("pulse_period", ctypes.c_uint32),
        ("pulse_on", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


assert ctypes.sizeof(_Interf) == 32
INTERF_FIELDS = tuple(name for name, _ in _Interf._fields_ if name != "reserved")
GAL_INTERF_MAX = 4


class _Agc(ctypes.Structure):  # gal_iq_agc_t (32 bytes)
    _fields_ = [
        ("block_len", ctypes.c_uint32),
        ("window", ctypes.c_uint32),
        ("target_q8", ctypes.c_uint32),
        ("gain_min_q12", ctypes.c_uint32),
        ("gain_max_q12", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("p_init", ctypes.c_uint64),
    ]


AGC_FIELDS = ("block_len", "window", "target_q8", "gain_min_q12", "gain_max_q12", "p_init")
assert ctypes.sizeof(_Agc) == 32


class _Osc(ctypes.Structure):  # gal_iq_osc_t (48 bytes)
    _fields_ = [
        ("seed", ctypes.c_uint64),
        ("stream", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("p0", ctypes.c_uint64),
        ("f", ctypes.c_int64),
        ("d", ctypes.c_int64),
        ("s", ctypes.c_uint64),
    ]


OSC_FIELDS = ("seed", "stream", "p0", "f", "d", "s")
assert ctypes.sizeof(_Osc) == 48
GAL_OSC_MAX_S = 1 << 48


class _Scint(ctypes.Structure):  # gal_iq_scint_t (24 bytes)
    _fields_ = [
        ("seed", ctypes.c_uint64),
        ("stream", ctypes.c_uint32),
        ("node_len", ctypes.c_uint32),
        ("a_q12", ctypes.c_uint16),
        ("b_q12", ctypes.c_uint16),
        ("reserved", ctypes.c_uint32),
    ]


class _ScintJob(ctypes.Structure):  # gal_scint_job_t (56 bytes)
    _fields_ = [("in_dev", ctypes.c_void_p), ("out_dev", ctypes.c_void_p), ("n_samples", ctypes.c_uint64), ("first_sample", ctypes.c_uint64),
                ("row", _Scint)]


SCINT_FIELDS = ("seed", "stream", "node_len", "a_q12", "b_q12")
assert ctypes.sizeof(_Scint) == 24 and ctypes.sizeof(_ScintJob) == 56
# one row of a scintillation table as numpy sees it: scint_rows are arrays of this type, [n_epochs, n_slots]
SCINT_DTYPE = np.dtype([("seed", "<u8"), ("stream", "<u4"), ("node_len", "<u4"), ("a_q12", "<u2"), ("b_q12", "<u2"), ("reserved", "<u4")])
assert SCINT_DTYPE.itemsize == 24
GAL_SCINT_MIN_NODE = 64
GAL_SCINT_MAX_NODE = 1 << 24
GAL_SCINT_MAX_JOBS = 64


class _Steer(ctypes.Structure):  # gal_iq_steer_t (4 bytes)
    _fields_ = [("w_re", ctypes.c_int16), ("w_im", ctypes.c_int16)]


assert ctypes.sizeof(_Steer) == 4
# one weight of an array as numpy sees it: steer rows are arrays of this type, [n_epochs, n_elem, n_parts]
STEER_DTYPE = np.dtype([("w_re", "<i2"), ("w_im", "<i2")])
assert STEER_DTYPE.itemsize == 4
GAL_ARRAY_MAX_ELEM = 8
GAL_STEER_GAIN_MAX = 1023


class _Echo(ctypes.Structure):  # gal_iq_echo_t (16 bytes)
    _fields_ = [
        ("gain_q7", ctypes.c_uint16),
        ("delay", ctypes.c_uint16),
        ("ph0", ctypes.c_uint32),
        ("dph", ctypes.c_int32),
        ("reserved", ctypes.c_uint32),
    ]


assert ctypes.sizeof(_Echo) == 16
# one row of an echo table as numpy sees it: echo_rows are arrays of this type, [n_epochs, n_echo]
ECHO_DTYPE = np.dtype([("gain_q7", "<u2"), ("delay", "<u2"), ("ph0", "<u4"), ("dph", "<i4"), ("reserved", "<u4")])
assert ECHO_DTYPE.itemsize == 16
GAL_ECHO_MAX = 32
GAL_ECHO_MAX_DELAY = 1024
GAL_ECHO_LINES = 64


class _Refl(ctypes.Structure):  # gal_iq_refl_t (16 bytes)
    _fields_ = [
        ("gain_q7", ctypes.c_uint16),
        ("delay", ctypes.c_uint16),
        ("ph0", ctypes.c_uint32),
        ("dph", ctypes.c_int32),
        ("frac_q12", ctypes.c_uint16),
        ("reserved", ctypes.c_uint16),
    ]


assert ctypes.sizeof(_Refl) == 16
# one row of a reflector table: refl_rows are arrays of this type, [n_epochs, n_echo]; with frac_q12 = 0 its bytes are an ECHO_DTYPE row
REFL_DTYPE = np.dtype([("gain_q7", "<u2"), ("delay", "<u2"), ("ph0", "<u4"), ("dph", "<i4"), ("frac_q12", "<u2"), ("reserved", "<u2")])
assert REFL_DTYPE.itemsize == 16
GAL_REFL_GROUND = 0
GAL_REFL_WALL = 1


class _MpathEcho(ctypes.Structure):  # gal_mpath_echo_t (16 bytes)
    _fields_ = [("delay", ctypes.c_uint32), ("alpha_q12", ctypes.c_uint32), ("ph0", ctypes.c_uint32), ("dph", ctypes.c_int32)]


assert ctypes.sizeof(_MpathEcho) == 16
MPATH_ECHO_FIELDS = tuple(name for name, _ in _MpathEcho._fields_)


class _CorrReq(ctypes.Structure):  # gal_corr_req_t (56 bytes)
    _fields_ = [
        ("prn", ctypes.c_int32),
        ("max_periods", ctypes.c_int32),
        ("code_ph0", ctypes.c_uint64),
        ("code_dph", ctypes.c_uint64),
        ("carr_ph0", ctypes.c_uint32),
        ("carr_dph", ctypes.c_int32),
        ("delay0", ctypes.c_int32),
        ("delay_step", ctypes.c_int32),
        ("n_delay", ctypes.c_int32),
        ("dopp0", ctypes.c_int32),
        ("dopp_step", ctypes.c_int32),
        ("n_dopp", ctypes.c_int32),
    ]


assert ctypes.sizeof(_CorrReq) == 56
CORR_REQ_FIELDS = tuple(name for name, _ in _CorrReq._fields_)
GAL_CORR_MAX_REQ = 64


class _Psd(ctypes.Structure):  # gal_iq_psd_t (16 bytes)
    _fields_ = [
        ("log2_n", ctypes.c_int32),
        ("hop", ctypes.c_int32),
        ("window", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


assert ctypes.sizeof(_Psd) == 16
PSD_WINDOWS = {"rect": 0, "hann": 1}


class GalSynthError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("galsynth error %d: %s" % (code, msg))
        self.code = code


# every symbol include/galsynth.h declares (tests check the library exports all of them)
EXPORTED_SYMBOLS = (
    "gal_synth_version",
    "gal_synth_last_error",
    "gal_synth_device_count",
    "gal_synth_create",
    "gal_synth_destroy",
    "gal_synth_set_stream",
    "gal_synth_plan",
    "gal_synth_plan_async",
    "gal_synth_output_bytes",
    "gal_synth_walk_counts",
    "gal_synth_execute",
    "gal_synth_execute_range",
    "gal_synth_finish",
    "gal_synth_finish_n",
    "gal_synth_stats_size",
    "gal_synth_run_host",
    "gal_synth_run_host_n",
    "gal_synth_iq_bytes",
    "gal_synth_iq_convert",
    "gal_synth_iq_saturated",
    "gal_synth_iq_convert_noise",
    "gal_synth_noise_from_cn0",
    "gal_synth_iq_convert_interf",
    "gal_synth_interf_make",
    "gal_synth_iq_wsum",
    "gal_synth_run_gains",
    "gal_synth_gain_runs",
    "gal_synth_gain_q7",
    "gal_synth_mpath_check",
    "gal_synth_mpath_reset",
    "gal_synth_iq_mpath",
    "gal_synth_run_mpath",
    "gal_synth_mpath_make",
    "gal_synth_mpath_row",
    "gal_synth_refl_check",
    "gal_synth_iq_refl",
    "gal_synth_run_refl",
    "gal_synth_refl_geom",
    "gal_synth_refl_row",
    "gal_synth_fir_check",
    "gal_synth_fir_lowpass",
    "gal_synth_fir_set",
    "gal_synth_iq_fir",
    "gal_synth_firdec_check",
    "gal_synth_firdec_lowpass",
    "gal_synth_firdec_out_samples",
    "gal_synth_firdec_set",
    "gal_synth_iq_firdec",
    "gal_synth_agc_check",
    "gal_synth_agc_out_bytes",
    "gal_synth_agc_blocks",
    "gal_synth_agc_from_rms",
    "gal_synth_agc_set",
    "gal_synth_iq_agc",
    "gal_synth_osc_check",
    "gal_synth_osc_make",
    "gal_synth_osc_set",
    "gal_synth_iq_osc",
    "gal_synth_osc_lo_step",
    "gal_synth_scint_check",
    "gal_synth_scint_make",
    "gal_synth_iq_scint",
    "gal_synth_run_scint",
    "gal_synth_steer_check",
    "gal_synth_steer_make",
    "gal_synth_array_phase",
    "gal_synth_iq_array",
    "gal_synth_run_array",
    "gal_synth_corr_out_bytes",
    "gal_synth_correlate",
    "gal_synth_psd_segments",
    "gal_synth_iq_psd",
    "gal_tables_e1b",
    "gal_tables_e1c",
    "gal_tables_cos512",
    "gal_tables_sin512",
    "gal_tables_cs25",
    "gal_tables_gauss",
    "gal_tables_cos1024",
    "gal_tables_scint",
    "gal_tables_psd",
)

_libs = {}


def load_library(hooks=False):
    """dlopen libgalsynth.so (built in-tree by build.py).  Raises if it is not there: no fallback.
    hooks=True loads the GAL_TEST_HOOKS build instead (tests of the repair paths only)."""
    if hooks in _libs:
        return _libs[hooks]
    path = HOOKS_LIB_PATH if hooks else LIB_PATH
    if not hooks and os.environ.get("GAL_SYNTH_LIB"):
        # A/B experiments only (build_variant.sh (a tool of rounds 3-5: git history)): another build of the same sources, e.g. other register targets;
        # bench.py marks such a line "variant_lib" -- never a result
        path = os.path.abspath(os.environ["GAL_SYNTH_LIB"])
    if not os.path.exists(path):
        raise RuntimeError(
            "%s not found: build it first (python -c 'import __graft_entry__ as g; g.build()'). "
            "The synthesis engine has no CPU fallback." % path
        )
    lib = ctypes.CDLL(path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.gal_synth_version.restype = ctypes.c_char_p
    lib.gal_synth_last_error.restype = ctypes.c_char_p
    lib.gal_synth_device_count.restype = ctypes.c_int
    lib.gal_synth_create.argtypes = [ctypes.POINTER(_Cfg), ctypes.POINTER(vp)]
    lib.gal_synth_destroy.argtypes = [vp]
    lib.gal_synth_set_stream.argtypes = [vp, vp]
    lib.gal_synth_plan.argtypes = [vp, vp, i32, vp]
    lib.gal_synth_plan_async.argtypes = [vp, vp, i32, vp]
    lib.gal_synth_walk_counts.argtypes = [vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                          ctypes.POINTER(ctypes.c_int64)]
    lib.gal_synth_walk_counts.restype = ctypes.c_int
    lib.gal_synth_output_bytes.argtypes = [vp]
    lib.gal_synth_output_bytes.restype = ctypes.c_size_t
    lib.gal_synth_execute.argtypes = [vp, vp]
    lib.gal_synth_execute_range.argtypes = [vp, vp, ctypes.c_int32, ctypes.c_int32]
    lib.gal_synth_execute_range.restype = ctypes.c_int
    lib.gal_synth_finish.argtypes = [vp, vp, ctypes.POINTER(_Stats)]
    lib.gal_synth_run_host.argtypes = [vp, vp, i32, vp, vp, vp, ctypes.POINTER(_Stats)]
    # the sized entry points (what the header's macros call): the library copies min(our sizeof, its own) bytes of statistics
    lib.gal_synth_finish_n.argtypes = [vp, vp, ctypes.POINTER(_Stats), ctypes.c_size_t]
    lib.gal_synth_run_host_n.argtypes = [vp, vp, i32, vp, vp, vp, ctypes.POINTER(_Stats), ctypes.c_size_t]
    lib.gal_synth_stats_size.restype = ctypes.c_size_t
    lib.gal_synth_iq_bytes.argtypes = [i32, ctypes.c_size_t]
    lib.gal_synth_iq_bytes.restype = ctypes.c_size_t
    lib.gal_synth_iq_convert.argtypes = [vp, vp, ctypes.c_size_t, i32, i32, vp]
    lib.gal_synth_iq_convert.restype = ctypes.c_int
    lib.gal_synth_iq_saturated.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), i32]
    lib.gal_synth_iq_saturated.restype = ctypes.c_int
    lib.gal_synth_iq_convert_noise.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_uint64, ctypes.POINTER(_Noise), i32, i32, vp]
    lib.gal_synth_iq_convert_noise.restype = ctypes.c_int
    lib.gal_synth_noise_from_cn0.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.POINTER(_Noise)]
    lib.gal_synth_noise_from_cn0.restype = ctypes.c_int
    lib.gal_synth_iq_convert_interf.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_uint64, ctypes.POINTER(_Noise), ctypes.POINTER(_Interf), i32,
                                                i32, i32, vp]
    lib.gal_synth_iq_convert_interf.restype = ctypes.c_int
    lib.gal_synth_interf_make.argtypes = [ctypes.c_double] * 8 + [ctypes.POINTER(_Interf)]
    lib.gal_synth_interf_make.restype = ctypes.c_int
    lib.gal_synth_iq_wsum.argtypes = [vp, ctypes.POINTER(vp), i32, vp, i32, vp]
    lib.gal_synth_iq_wsum.restype = ctypes.c_int
    lib.gal_synth_run_gains.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    lib.gal_synth_run_gains.restype = ctypes.c_int
    lib.gal_synth_gain_runs.argtypes = [vp, ctypes.POINTER(i32)]
    lib.gal_synth_gain_runs.restype = ctypes.c_int
    lib.gal_synth_gain_q7.argtypes = [ctypes.c_double, ctypes.c_double, vp, ctypes.c_double, ctypes.POINTER(ctypes.c_uint16)]
    lib.gal_synth_gain_q7.restype = ctypes.c_int
    lib.gal_synth_mpath_check.argtypes = [vp, i32, i32, vp, i32]
    lib.gal_synth_mpath_check.restype = ctypes.c_int
    lib.gal_synth_mpath_reset.argtypes = [vp]
    lib.gal_synth_mpath_reset.restype = ctypes.c_int
    lib.gal_synth_iq_mpath.argtypes = [vp, ctypes.POINTER(vp), i32, vp, vp, i32, vp, vp, i32, vp]
    lib.gal_synth_iq_mpath.restype = ctypes.c_int
    lib.gal_synth_run_mpath.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp, vp]
    lib.gal_synth_run_mpath.restype = ctypes.c_int
    lib.gal_synth_mpath_make.argtypes = [ctypes.c_double] * 5 + [ctypes.POINTER(_MpathEcho)]
    lib.gal_synth_mpath_make.restype = ctypes.c_int
    lib.gal_synth_mpath_row.argtypes = [ctypes.POINTER(_MpathEcho), ctypes.c_uint16, ctypes.c_uint64, i32, ctypes.POINTER(_Echo)]
    lib.gal_synth_mpath_row.restype = ctypes.c_int
    lib.gal_synth_refl_check.argtypes = [vp, i32, i32, vp, i32]
    lib.gal_synth_refl_check.restype = ctypes.c_int
    lib.gal_synth_iq_refl.argtypes = [vp, ctypes.POINTER(vp), i32, vp, vp, i32, vp, vp, i32, vp]
    lib.gal_synth_iq_refl.restype = ctypes.c_int
    lib.gal_synth_run_refl.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp, vp]
    lib.gal_synth_run_refl.restype = ctypes.c_int
    lib.gal_synth_refl_geom.argtypes = [i32, ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_double)]
    lib.gal_synth_refl_geom.restype = ctypes.c_int
    lib.gal_synth_refl_row.argtypes = [ctypes.c_double] * 5 + [i32, ctypes.c_uint16, ctypes.POINTER(_Refl)]
    lib.gal_synth_refl_row.restype = ctypes.c_int
    lib.gal_synth_fir_check.argtypes = [vp, i32]
    lib.gal_synth_fir_check.restype = ctypes.c_int
    lib.gal_synth_fir_lowpass.argtypes = [ctypes.c_double, ctypes.c_double, i32, vp]
    lib.gal_synth_fir_lowpass.restype = ctypes.c_int
    lib.gal_synth_fir_set.argtypes = [vp, vp, i32]
    lib.gal_synth_fir_set.restype = ctypes.c_int
    lib.gal_synth_iq_fir.argtypes = [vp, vp, ctypes.c_size_t, vp]
    lib.gal_synth_iq_fir.restype = ctypes.c_int
    lib.gal_synth_firdec_check.argtypes = [vp, i32, i32]
    lib.gal_synth_firdec_check.restype = ctypes.c_int
    lib.gal_synth_firdec_lowpass.argtypes = [ctypes.c_double, ctypes.c_double, i32, vp]
    lib.gal_synth_firdec_lowpass.restype = ctypes.c_int
    lib.gal_synth_firdec_out_samples.argtypes = [ctypes.c_uint64, ctypes.c_uint64, i32]
    lib.gal_synth_firdec_out_samples.restype = ctypes.c_uint64
    lib.gal_synth_firdec_set.argtypes = [vp, vp, i32, i32, ctypes.c_uint64]
    lib.gal_synth_firdec_set.restype = ctypes.c_int
    lib.gal_synth_iq_firdec.argtypes = [vp, vp, ctypes.c_size_t, vp, ctypes.POINTER(ctypes.c_size_t)]
    lib.gal_synth_iq_firdec.restype = ctypes.c_int
    lib.gal_synth_agc_check.argtypes = [ctypes.POINTER(_Agc)]
    lib.gal_synth_agc_check.restype = ctypes.c_int
    lib.gal_synth_agc_out_bytes.argtypes = [i32, ctypes.c_size_t]
    lib.gal_synth_agc_out_bytes.restype = ctypes.c_size_t
    lib.gal_synth_agc_blocks.argtypes = [ctypes.c_uint64, ctypes.c_uint64, i32]
    lib.gal_synth_agc_blocks.restype = ctypes.c_uint64
    lib.gal_synth_agc_from_rms.argtypes = [ctypes.c_double, ctypes.c_double, i32, i32, ctypes.POINTER(_Agc)]
    lib.gal_synth_agc_from_rms.restype = ctypes.c_int
    lib.gal_synth_agc_set.argtypes = [vp, ctypes.POINTER(_Agc), ctypes.c_uint64]
    lib.gal_synth_agc_set.restype = ctypes.c_int
    lib.gal_synth_iq_agc.argtypes = [vp, vp, ctypes.c_size_t, i32, i32, vp, vp, ctypes.POINTER(ctypes.c_size_t)]
    lib.gal_synth_iq_agc.restype = ctypes.c_int
    lib.gal_synth_osc_check.argtypes = [ctypes.POINTER(_Osc)]
    lib.gal_synth_osc_check.restype = ctypes.c_int
    lib.gal_synth_osc_make.argtypes = [ctypes.c_double] * 5 + [ctypes.POINTER(_Osc)]
    lib.gal_synth_osc_make.restype = ctypes.c_int
    lib.gal_synth_osc_set.argtypes = [vp, ctypes.POINTER(_Osc), ctypes.c_uint64]
    lib.gal_synth_osc_set.restype = ctypes.c_int
    lib.gal_synth_iq_osc.argtypes = [vp, vp, ctypes.c_size_t, vp]
    lib.gal_synth_iq_osc.restype = ctypes.c_int
    lib.gal_synth_osc_lo_step.argtypes = [ctypes.POINTER(_Osc), ctypes.c_uint64, ctypes.POINTER(i32)]
    lib.gal_synth_osc_lo_step.restype = ctypes.c_int
    lib.gal_synth_scint_check.argtypes = [ctypes.POINTER(_Scint)]
    lib.gal_synth_scint_check.restype = ctypes.c_int
    lib.gal_synth_scint_make.argtypes = [ctypes.c_double] * 3 + [ctypes.POINTER(_Scint)]
    lib.gal_synth_scint_make.restype = ctypes.c_int
    lib.gal_synth_iq_scint.argtypes = [vp, ctypes.POINTER(_ScintJob), i32]
    lib.gal_synth_iq_scint.restype = ctypes.c_int
    lib.gal_synth_run_scint.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp, ctypes.c_uint64, vp, vp]
    lib.gal_synth_run_scint.restype = ctypes.c_int
    lib.gal_synth_steer_check.argtypes = [vp, i32, i32, i32]
    lib.gal_synth_steer_check.restype = ctypes.c_int
    lib.gal_synth_steer_make.argtypes = [ctypes.c_uint16, ctypes.c_uint32, ctypes.POINTER(_Steer)]
    lib.gal_synth_steer_make.restype = ctypes.c_int
    lib.gal_synth_array_phase.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_uint32)]
    lib.gal_synth_array_phase.restype = ctypes.c_int
    lib.gal_synth_iq_array.argtypes = [vp, vp, i32, vp, i32, i32, vp]
    lib.gal_synth_iq_array.restype = ctypes.c_int
    lib.gal_synth_run_array.argtypes = [vp, vp, i32, vp, vp, vp, i32, vp, ctypes.c_uint64, vp, vp]
    lib.gal_synth_run_array.restype = ctypes.c_int
    lib.gal_synth_corr_out_bytes.argtypes = [ctypes.POINTER(_CorrReq)]
    lib.gal_synth_corr_out_bytes.restype = ctypes.c_size_t
    lib.gal_synth_correlate.argtypes = [vp, vp, i32, ctypes.c_size_t, ctypes.POINTER(_CorrReq), i32, vp]
    lib.gal_synth_correlate.restype = ctypes.c_int
    lib.gal_corr_from_epoch.argtypes = [vp, ctypes.c_double, ctypes.c_int64, ctypes.POINTER(_CorrReq)]
    lib.gal_corr_from_epoch.restype = ctypes.c_int
    lib.gal_corr_cn0.argtypes = [vp, ctypes.POINTER(_CorrReq), i32, i32, i32, ctypes.c_double, ctypes.POINTER(ctypes.c_double),
                                 ctypes.POINTER(ctypes.c_double)]
    lib.gal_corr_cn0.restype = ctypes.c_int
    lib.gal_synth_psd_segments.argtypes = [ctypes.POINTER(_Psd), ctypes.c_size_t]
    lib.gal_synth_psd_segments.restype = ctypes.c_int64
    lib.gal_synth_iq_psd.argtypes = [vp, vp, i32, ctypes.c_size_t, ctypes.POINTER(_Psd), vp, ctypes.POINTER(i32)]
    lib.gal_synth_iq_psd.restype = ctypes.c_int
    for name in ("gal_tables_e1b", "gal_tables_e1c", "gal_tables_cos512", "gal_tables_sin512", "gal_tables_gauss", "gal_tables_cos1024",
                 "gal_tables_scint", "gal_tables_psd"):
        getattr(lib, name).restype = vp
    lib.gal_tables_cs25.restype = ctypes.c_uint32
    _libs[hooks] = lib
    return lib


def device_count():
    return int(load_library().gal_synth_device_count())


def iq_format_code(fmt):
    """"ishort" | "ibyte" | "ibit" (or the GAL_IQ_* integer) -> the GAL_IQ_* integer."""
    if isinstance(fmt, str):
        if fmt not in IQ_FORMATS:
            raise ValueError("unknown IQ format %r (accepted: %s)" % (fmt, ", ".join(IQ_FORMATS)))
        return IQ_FORMATS[fmt]
    return int(fmt)


def iq_bytes(fmt, n_samples):
    """Bytes that n_samples complex samples take in `fmt`: 4 n, 2 n, ceil(n / 4); 0 for an unknown integer format (no GPU needed)."""
    return int(load_library().gal_synth_iq_bytes(iq_format_code(fmt), int(n_samples)))


def noise_from_cn0(cn0_dbhz, sample_rate, gain=1.0):
    """gal_synth_noise_from_cn0 (no GPU needed): the `noise` dict of SynthEngine.iq_convert for a C/N0 in dB-Hz of one satellite's
    composite E1B + E1C signal -- seed 0, stream 0, gain_q16 = round(gain 65536), sigma_q4 = round(16 x 250 gain sqrt(rate / cn0))."""
    lib = load_library()
    n = _Noise()
    rc = lib.gal_synth_noise_from_cn0(float(cn0_dbhz), float(sample_rate), float(gain), ctypes.byref(n))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())
    return {"seed": int(n.seed), "stream": int(n.stream), "gain_q16": int(n.gain_q16), "sigma_q4": int(n.sigma_q4)}


def _noise_struct(noise):
    """dict with the keys seed, stream, gain_q16, sigma_q4 (seed and stream default to 0), or a tuple in that order."""
    if isinstance(noise, dict):
        unknown = set(noise) - {"seed", "stream", "gain_q16", "sigma_q4"}
        if unknown:
            raise ValueError("noise: unknown keys %s" % sorted(unknown))
        noise = (noise.get("seed", 0), noise.get("stream", 0), noise["gain_q16"], noise["sigma_q4"])
    seed, stream, gain_q16, sigma_q4 = (int(v) for v in noise)
    return _Noise(seed, stream, gain_q16, sigma_q4, 0)


def interf_make(js_db, gain, sample_rate, f_lo_hz, f_hi_hz=0.0, sweep_s=0.0, pulse_period_s=0.0, pulse_on_s=0.0):
    """gal_synth_interf_make (no GPU needed): one source of the `interf` list of SynthEngine.iq_convert for a jammer-to-signal ratio
    in dB against one satellite's composite E1B + E1C signal at `gain` -- a CW tone at f_lo_hz (sweep_s = 0) or a chirp from f_lo_hz
    to f_hi_hz that restarts every sweep_s seconds, on for pulse_on_s of every pulse_period_s seconds (0: always)."""
    lib = load_library()
    c = _Interf()
    rc = lib.gal_synth_interf_make(float(js_db), float(gain), float(sample_rate), float(f_lo_hz), float(f_hi_hz), float(sweep_s),
                                   float(pulse_period_s), float(pulse_on_s), ctypes.byref(c))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())
    return {k: int(getattr(c, k)) for k in INTERF_FIELDS}


def _interf_struct(src):
    """dict with the fields of gal_iq_interf_t but `reserved` (amp_q4 is required, the others default to 0), or an _Interf."""
    if isinstance(src, _Interf):
        return src
    unknown = set(src) - set(INTERF_FIELDS)
    if unknown:
        raise ValueError("interference source: unknown keys %s" % sorted(unknown))
    d = dict.fromkeys(INTERF_FIELDS, 0)
    d.update(src)
    if "amp_q4" not in src:
        raise ValueError("interference source: amp_q4 is required")
    return _Interf(**{k: int(d[k]) for k in INTERF_FIELDS})


def gain_q7(d_m, elev_rad, pattern_db=None, offset_db=0.0):
    """gal_synth_gain_q7 (no GPU needed): the Q7 gain (128 = unity) of a satellite at the geometric distance d_m [m] and the elevation
    elev_rad -- path loss against Galileo's nominal altitude, the attenuation pattern_db[(int)((90 - elev) / 5)] (37 values in dB, one
    per 5 degrees off the zenith; None: isotropic) and an offset in dB; truncated, at most 32767."""
    lib = load_library()
    pat = None
    if pattern_db is not None:
        pat = np.ascontiguousarray(pattern_db, dtype=np.float64)
        if pat.shape != (GAL_GAIN_PATTERN_LEN,):
            raise ValueError("gain_q7: pattern_db must hold %d values" % GAL_GAIN_PATTERN_LEN)
    g = ctypes.c_uint16(0)
    rc = lib.gal_synth_gain_q7(float(d_m), float(elev_rad), pat.ctypes.data if pat is not None else None, float(offset_db), ctypes.byref(g))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())
    return int(g.value)


def _fir_taps(taps, who):
    t = np.asarray(taps)
    if t.ndim != 1 or (t.size and (not np.issubdtype(t.dtype, np.integer) or t.min() < -32768 or t.max() > 32767)):
        raise ValueError("%s: taps must be a one-dimensional sequence of integers that fit an int16 (Q14: 16384 = 1.0)" % who)
    return np.ascontiguousarray(t, dtype=np.int16)


def fir_check(taps):
    """gal_synth_fir_check (no GPU needed): raises GalSynthError unless the Q14 taps are admitted -- 1 .. GAL_FIR_MAX_TAPS of them
    with sum |h| <= 65535."""
    lib = load_library()
    t = _fir_taps(taps, "fir_check")
    rc = lib.gal_synth_fir_check(t.ctypes.data if t.size else None, int(t.size))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())


def fir_lowpass(cutoff_hz, sample_rate, n_taps=63):
    """gal_synth_fir_lowpass (no GPU needed): the int16 Q14 taps of a Hamming-windowed sinc low-pass of n_taps (odd, 3 .. 127) taps
    with DC gain exactly 1 (the taps sum to 16384)."""
    lib = load_library()
    t = np.zeros(GAL_FIR_MAX_TAPS, dtype=np.int16)
    rc = lib.gal_synth_fir_lowpass(float(cutoff_hz), float(sample_rate), int(n_taps), t.ctypes.data)
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())
    return t[: int(n_taps)].copy()


def firdec_check(taps, decim):
    """gal_synth_firdec_check (no GPU needed): raises GalSynthError unless the Q14 taps and the decimation are admitted -- 1 ..
    GAL_FIRDEC_MAX_TAPS taps with sum |h| <= 65535, decim 2 .. GAL_FIRDEC_MAX_DECIM."""
    lib = load_library()
    t = _fir_taps(taps, "firdec_check")
    rc = lib.gal_synth_firdec_check(t.ctypes.data if t.size else None, int(t.size), int(decim))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())


def firdec_lowpass(cutoff_hz, sample_rate_in, n_taps):
    """gal_synth_firdec_lowpass (no GPU needed): the low-pass of fir_lowpass for the decimator, n_taps odd, 3 .. 511, designed at the
    rate of the decimator's INPUT stream."""
    lib = load_library()
    t = np.zeros(GAL_FIRDEC_MAX_TAPS, dtype=np.int16)
    rc = lib.gal_synth_firdec_lowpass(float(cutoff_hz), float(sample_rate_in), int(n_taps), t.ctypes.data)
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())
    return t[: int(n_taps)].copy()


def firdec_out_samples(first_sample, n_in, decim):
    """gal_synth_firdec_out_samples (no GPU needed): the outputs a call of n_in inputs keeps when its first input has the global index
    first_sample -- the number of m with first_sample <= decim * m < first_sample + n_in."""
    return int(load_library().gal_synth_firdec_out_samples(int(first_sample), int(n_in), int(decim)))


def agc_format_code(fmt):
    """"ishort" | "ibyte" | "i2bit" (or the GAL_IQ_* integer) -> the GAL_IQ_* integer of an AGC output format."""
    if isinstance(fmt, str):
        if fmt not in AGC_FORMATS:
            raise ValueError("unknown AGC output format %r (accepted: %s)" % (fmt, ", ".join(AGC_FORMATS)))
        return AGC_FORMATS[fmt]
    return int(fmt)


def _agc_struct(agc):
    """dict with the fields of gal_iq_agc_t but `reserved` (block_len, window and target_q8 are required; the gain clamps default to
    their widest, p_init to 0), or an _Agc."""
    if isinstance(agc, _Agc):
        return agc
    unknown = set(agc) - set(AGC_FIELDS)
    if unknown:
        raise ValueError("agc: unknown keys %s" % sorted(unknown))
    d = {"gain_min_q12": 1, "gain_max_q12": GAL_AGC_GAIN_MAX, "p_init": 0}
    d.update(agc)
    for k in ("block_len", "window", "target_q8"):
        if k not in d:
            raise ValueError("agc: %s is required" % k)
    for k in AGC_FIELDS:
        if not 0 <= int(d[k]) < (1 << 64 if k == "p_init" else 1 << 32):
            raise ValueError("agc: %s = %r does not fit its field" % (k, d[k]))
    return _Agc(int(d["block_len"]), int(d["window"]), int(d["target_q8"]), int(d["gain_min_q12"]), int(d["gain_max_q12"]), 0, int(d["p_init"]))


def agc_check(agc):
    """gal_synth_agc_check (no GPU needed): raises GalSynthError unless the AGC parameters are admitted -- block_len 16 .. 65536, window
    1 .. 64, block_len x window <= 65536, target_q8 1 .. 32767 x 256, 1 <= gain_min_q12 <= gain_max_q12 <= 2^24, p_init <= 2^31 block_len."""
    lib = load_library()
    a = _agc_struct(agc)
    rc = lib.gal_synth_agc_check(ctypes.byref(a))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())


def agc_from_rms(target_rms, init_rms, block_len=2600, window=8):
    """gal_synth_agc_from_rms (no GPU needed): the `agc` dict of SynthEngine.agc_set for a wanted rms per rail and the rms assumed in
    front of the stream, both in int16 LSB -- target_q8 = llround(256 target_rms), p_init = 2 block_len llround(init_rms^2), the gain
    clamps at their widest."""
    lib = load_library()
    a = _Agc()
    rc = lib.gal_synth_agc_from_rms(float(target_rms), float(init_rms), int(block_len), int(window), ctypes.byref(a))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())
    return {k: int(getattr(a, k)) for k in AGC_FIELDS}


def agc_out_bytes(fmt, n_samples):
    """gal_synth_agc_out_bytes (no GPU needed): 4 n ("ishort"), 2 n ("ibyte"), ceil(n / 2) ("i2bit"); 0 for any other integer format."""
    return int(load_library().gal_synth_agc_out_bytes(agc_format_code(fmt), int(n_samples)))


def agc_blocks(first_sample, n_samples, block_len):
    """gal_synth_agc_blocks (no GPU needed): the blocks whose first sample lies in a call of n_samples that begins at the global index
    first_sample -- the number of b with first_sample <= b block_len < first_sample + n_samples."""
    return int(load_library().gal_synth_agc_blocks(int(first_sample), int(n_samples), int(block_len)))


def _osc_struct(osc):
    """dict with the fields of gal_iq_osc_t but `reserved` (all optional: seed defaults to 1, the others to 0), or an _Osc."""
    if isinstance(osc, _Osc):
        return osc
    unknown = set(osc) - set(OSC_FIELDS)
    if unknown:
        raise ValueError("osc: unknown keys %s" % sorted(unknown))
    d = {"seed": 1, "stream": 0, "p0": 0, "f": 0, "d": 0, "s": 0}
    d.update(osc)
    for k in OSC_FIELDS:
        lo, hi = (-(1 << 63), 1 << 63) if k in ("f", "d") else (0, 1 << 32) if k == "stream" else (0, 1 << 64)
        if not lo <= int(d[k]) < hi:
            raise ValueError("osc: %s = %r does not fit its field" % (k, d[k]))
    return _Osc(int(d["seed"]), int(d["stream"]), 0, int(d["p0"]), int(d["f"]), int(d["d"]), int(d["s"]))


def osc_check(osc):
    """gal_synth_osc_check (no GPU needed): raises GalSynthError unless the oscillator parameters are admitted (s <= 2^48)."""
    lib = load_library()
    o = _osc_struct(osc)
    rc = lib.gal_synth_osc_check(ctypes.byref(o))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())


def osc_make(f_hz=0.0, drift_hz_s=0.0, h0=0.0, sample_rate=2.6e6, carrier_hz=1575.42e6):
    """gal_synth_osc_make (no GPU needed): the `osc` dict of SynthEngine.osc_set for a carrier offset f_hz, a drift in Hz/s and white-FM
    phase noise of the one-sided fractional-frequency PSD h0 (s) at carrier_hz -- f = llround(f_hz / fs 2^64), d = llround(drift / fs^2
    2^64), s = llround(carrier_hz sqrt(h0 / (2 fs)) / sqrt(var z) 2^52); seed 1, stream 0, p0 0."""
    lib = load_library()
    o = _Osc()
    rc = lib.gal_synth_osc_make(float(f_hz), float(drift_hz_s), float(h0), float(sample_rate), float(carrier_hz), ctypes.byref(o))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())
    return {k: int(getattr(o, k)) for k in OSC_FIELDS}


def osc_lo_step(osc, n):
    """gal_synth_osc_lo_step (no GPU needed): the oscillator's deterministic phase step at the global sample n in the correlator's
    units, (F + n D) mod 2^64 >> 32 as an int32 -- add it to a request's carr_dph."""
    lib = load_library()
    o = _osc_struct(osc)
    out = ctypes.c_int32(0)
    rc = lib.gal_synth_osc_lo_step(ctypes.byref(o), int(n), ctypes.byref(out))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())
    return int(out.value)


def _scint_struct(row):
    """dict with the fields of gal_iq_scint_t but `reserved` (seed defaults to 1, stream to 0, node_len to 64, a_q12 to 4096, b_q12 to 0:
    the identity), or a _Scint."""
    if isinstance(row, _Scint):
        return row
    unknown = set(row) - set(SCINT_FIELDS)
    if unknown:
        raise ValueError("scint: unknown keys %s" % sorted(unknown))
    d = {"seed": 1, "stream": 0, "node_len": GAL_SCINT_MIN_NODE, "a_q12": 4096, "b_q12": 0}
    d.update(row)
    for k, bits in (("seed", 64), ("stream", 32), ("node_len", 32), ("a_q12", 16), ("b_q12", 16)):
        if not 0 <= int(d[k]) < 1 << bits:
            raise ValueError("scint: %s = %r does not fit its field" % (k, d[k]))
    return _Scint(int(d["seed"]), int(d["stream"]), int(d["node_len"]), int(d["a_q12"]), int(d["b_q12"]), 0)


def scint_check(row):
    """gal_synth_scint_check (no GPU needed): raises GalSynthError unless the scintillation row is admitted (64 <= node_len <= 2^24,
    a_q12 and b_q12 <= 4096)."""
    lib = load_library()
    r = _scint_struct(row)
    rc = lib.gal_synth_scint_check(ctypes.byref(r))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())


def scint_make(s4, tau0_s, sample_rate=2.6e6):
    """gal_synth_scint_make (no GPU needed): the scintillation row, as a dict, of the index s4 (0 .. 1) and the 1/e decorrelation time
    tau0_s of the scattered field at sample_rate: a_q12, b_q12 from the Rician K with that S4, node_len = llround(tau0_s sample_rate /
    8); seed 1, stream 0."""
    lib = load_library()
    r = _Scint()
    rc = lib.gal_synth_scint_make(float(s4), float(tau0_s), float(sample_rate), ctypes.byref(r))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())
    return {k: int(getattr(r, k)) for k in SCINT_FIELDS}


def scint_rows(rows, n_epochs, n_slots):
    """A scintillation table [n_epochs, n_slots] (SCINT_DTYPE): rows = {slot: row dict}, every other slot the identity."""
    out = np.zeros((int(n_epochs), int(n_slots)), dtype=SCINT_DTYPE)
    out["seed"], out["node_len"], out["a_q12"] = 1, GAL_SCINT_MIN_NODE, 4096
    for slot, row in rows.items():
        r = _scint_struct(row)
        out[:, int(slot)] = (r.seed, r.stream, r.node_len, r.a_q12, r.b_q12, 0)
    return out


def _steer_table(rows, who):
    """The weights [n_epochs, n_elem, n_parts] as a contiguous STEER_DTYPE array; an integer array [..., 2] of (w_re, w_im) is packed."""
    a = np.asarray(rows)
    if a.dtype != STEER_DTYPE:
        if a.ndim != 4 or a.shape[3] != 2:
            raise ValueError("%s: rows must be STEER_DTYPE [n_epochs, n_elem, n_parts] or integers [n_epochs, n_elem, n_parts, 2]" % who)
        if a.size and (a.min() < -32768 or a.max() > 32767):
            raise ValueError("%s: a weight does not fit an int16" % who)
        t = np.zeros(a.shape[:3], dtype=STEER_DTYPE)
        t["w_re"], t["w_im"] = a[..., 0], a[..., 1]
        a = t
    if a.ndim != 3:
        raise ValueError("%s: rows must have shape [n_epochs, n_elem, n_parts]" % who)
    return np.ascontiguousarray(a)


def steer_check(rows, n_epochs=None, n_elem=None, n_parts=None):
    """gal_synth_steer_check (no GPU needed): raises GalSynthError unless the weights rows [n_epochs, n_elem, n_parts] are admitted
    (1 .. 8 elements, 1 .. 64 parts, no component of -32768).  rows None passes a null pointer with the three counts given."""
    lib = load_library()
    if rows is None:
        rc = lib.gal_synth_steer_check(None, int(n_epochs), int(n_elem), int(n_parts))
    else:
        t = _steer_table(rows, "steer_check")
        rc = lib.gal_synth_steer_check(t.ctypes.data if t.size else None, t.shape[0], t.shape[1], t.shape[2])
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())


def steer_make(gain_q7, phase):
    """gal_synth_steer_make (no GPU needed): the Q12 weight (w_re, w_im) of a part at the Q7 gain gain_q7 (0 .. 1023) turned by `phase`
    (2^-32 cycles, rounded to the 1024-entry cosine table)."""
    if not 0 <= int(gain_q7) <= 65535:
        raise ValueError("steer_make: gain_q7 = %r does not fit a uint16" % (gain_q7,))
    lib = load_library()
    w = _Steer()
    rc = lib.gal_synth_steer_make(int(gain_q7), int(phase) & 0xffffffff, ctypes.byref(w))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())
    return int(w.w_re), int(w.w_im)


def array_phase(enu_m, az_rad, el_rad):
    """gal_synth_array_phase (no GPU needed): the carrier phase, in 2^-32 cycles, of a plane wave from (az_rad from north over east,
    el_rad) at an element enu_m = (east, north, up) metres from the array's reference point.  enu_m None passes a null pointer."""
    lib = load_library()
    v = None if enu_m is None else (ctypes.c_double * 3)(*[float(x) for x in enu_m])
    ph = ctypes.c_uint32(0)
    rc = lib.gal_synth_array_phase(v, float(az_rad), float(el_rad), ctypes.byref(ph))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())
    return int(ph.value)


def _echo_table(echo_rows, n_epochs, who, dtype=ECHO_DTYPE):
    """echo_rows -> a contiguous ECHO_DTYPE (REFL_DTYPE) array [n_epochs, n_echo] (None or an empty one: no echoes)."""
    if echo_rows is None:
        return np.zeros((n_epochs, 0), dtype=dtype)
    r = np.ascontiguousarray(echo_rows, dtype=dtype)
    if r.ndim != 2 or r.shape[0] != n_epochs:
        raise ValueError("%s: echo_rows must have shape [n_epochs=%d, n_echo]" % (who, n_epochs))
    return r


def mpath_check(echo_rows, part_of_echo, n_parts):
    """gal_synth_mpath_check (no GPU needed): raises GalSynthError(GAL_E_INVAL) for an echo table [n_epochs, n_echo] (ECHO_DTYPE) or
    part indices that the echo pass would refuse."""
    lib = load_library()
    r = np.ascontiguousarray(echo_rows, dtype=ECHO_DTYPE)
    if r.ndim != 2:
        raise ValueError("mpath_check: echo_rows must have shape [n_epochs, n_echo]")
    pof = np.ascontiguousarray(part_of_echo, dtype=np.int32)
    if pof.shape != (r.shape[1],):
        raise ValueError("mpath_check: part_of_echo must have n_echo = %d entries" % r.shape[1])
    rc = lib.gal_synth_mpath_check(r.ctypes.data, r.shape[1], r.shape[0], pof.ctypes.data, int(n_parts))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())


def mpath_make(delay_s, rel_db, phase_deg=0.0, fade_hz=0.0, sample_rate=2.6e6):
    """gal_synth_mpath_make (no GPU needed): one echo from physical figures as a dict -- delay (samples), alpha_q12 (amplitude relative
    to the direct signal, 4096 = equal), ph0 and dph (2^-32 cycles, per sample)."""
    lib = load_library()
    q = _MpathEcho()
    rc = lib.gal_synth_mpath_make(float(delay_s), float(rel_db), float(phase_deg), float(fade_hz), float(sample_rate), ctypes.byref(q))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())
    return {k: int(getattr(q, k)) for k in MPATH_ECHO_FIELDS}


def mpath_rows(echo, slot_gain_q7, first_epoch, samples_per_epoch):
    """gal_synth_mpath_row (no GPU needed) for the epochs first_epoch, first_epoch + 1, ... of the whole stream: the column of an echo
    table (ECHO_DTYPE, one row per entry of slot_gain_q7, the Q7 gains of the direct signal) for the dict `echo` of mpath_make."""
    lib = load_library()
    q = _MpathEcho(**{k: int(echo[k]) for k in MPATH_ECHO_FIELDS})
    gains = np.asarray(slot_gain_q7).ravel()
    out = np.zeros(gains.size, dtype=ECHO_DTYPE)
    row = _Echo()
    for e, g in enumerate(gains):
        if not 0 <= int(g) <= 65535:
            raise ValueError("mpath_rows: a gain does not fit a uint16")
        rc = lib.gal_synth_mpath_row(ctypes.byref(q), int(g), int(first_epoch) + e, int(samples_per_epoch), ctypes.byref(row))
        if rc != 0:
            raise GalSynthError(rc, lib.gal_synth_last_error().decode())
        out[e] = (row.gain_q7, row.delay, row.ph0, row.dph, row.reserved)
    return out


def refl_check(refl_rows, part_of_echo, n_parts):
    """gal_synth_refl_check (no GPU needed): raises GalSynthError(GAL_E_INVAL) for a reflector table [n_epochs, n_echo] (REFL_DTYPE) or
    part indices that the reflector pass would refuse."""
    lib = load_library()
    r = np.ascontiguousarray(refl_rows, dtype=REFL_DTYPE)
    if r.ndim != 2:
        raise ValueError("refl_check: refl_rows must have shape [n_epochs, n_echo]")
    pof = np.ascontiguousarray(part_of_echo, dtype=np.int32)
    if pof.shape != (r.shape[1],):
        raise ValueError("refl_check: part_of_echo must have n_echo = %d entries" % r.shape[1])
    rc = lib.gal_synth_refl_check(r.ctypes.data, r.shape[1], r.shape[0], pof.ctypes.data, int(n_parts))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())


def refl_geom(kind, p, az_rad, el_rad):
    """gal_synth_refl_geom (no GPU needed): the excess path in metres of the reflection off a plane -- kind GAL_REFL_GROUND with
    p = (height,), GAL_REFL_WALL with p = (distance, azimuth of the wall in rad) -- for a satellite at (az_rad, el_rad); -1.0 where the
    geometry gives no echo."""
    lib = load_library()
    v = (ctypes.c_double * 2)(*([float(x) for x in p] + [0.0, 0.0])[:2])
    x = ctypes.c_double()
    rc = lib.gal_synth_refl_geom(int(kind), v, float(az_rad), float(el_rad), ctypes.byref(x))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())
    return float(x.value)


def refl_row(excess_now_m, excess_next_m, rel_db, refl_phase_deg=180.0, sample_rate=2.6e6, samples_per_epoch=260000, slot_gain_q7=128):
    """gal_synth_refl_row (no GPU needed): the row (a REFL_DTYPE scalar) of one epoch from the excess path at its start and at the next
    epoch's; a negative excess_now_m (no echo) gives the zero row."""
    lib = load_library()
    if not 0 <= int(slot_gain_q7) <= 65535:
        raise ValueError("refl_row: the gain does not fit a uint16")
    row = _Refl()
    rc = lib.gal_synth_refl_row(float(excess_now_m), float(excess_next_m), float(rel_db), float(refl_phase_deg), float(sample_rate),
                                int(samples_per_epoch), int(slot_gain_q7), ctypes.byref(row))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())
    return np.array((row.gain_q7, row.delay, row.ph0, row.dph, row.frac_q12, row.reserved), dtype=REFL_DTYPE)


def _corr_struct(req):
    """dict with the fields of gal_corr_req_t (grids default to one prompt cell, max_periods to 1), or a _CorrReq."""
    if isinstance(req, _CorrReq):
        return req
    unknown = set(req) - set(CORR_REQ_FIELDS)
    if unknown:
        raise ValueError("correlator request: unknown keys %s" % sorted(unknown))
    d = {"max_periods": 1, "carr_ph0": 0, "carr_dph": 0, "delay0": 0, "delay_step": 1, "n_delay": 1, "dopp0": 0, "dopp_step": 0, "n_dopp": 1}
    d.update(req)
    return _CorrReq(**{k: int(d[k]) for k in CORR_REQ_FIELDS})


def corr_out_bytes(req):
    """gal_synth_corr_out_bytes (no GPU needed): bytes of sums one request takes, 0 for a grid outside the caps."""
    return int(load_library().gal_synth_corr_out_bytes(ctypes.byref(_corr_struct(req))))


def _psd_struct(log2_n, hop, window, reserved=0):
    w = PSD_WINDOWS[window] if isinstance(window, str) else int(window)
    return _Psd(int(log2_n), int(hop), w, int(reserved))


def psd_segments(log2_n, hop, window, n_samples, reserved=0):
    """gal_synth_psd_segments (no GPU needed): the segments SynthEngine.iq_psd would sum over n_samples samples; 0 where it would refuse
    (a field out of range, fewer than N = 2^log2_n samples, n_seg N^2 > 2^32).  window: "rect" | "hann" or 0 | 1."""
    return int(load_library().gal_synth_psd_segments(ctypes.byref(_psd_struct(log2_n, hop, window, reserved)), int(n_samples)))


def corr_from_epoch(rec, sample_rate, sample_offset=0, **grid):
    """gal_corr_from_epoch (no GPU needed): the replica of one planned record (a CHAN_EPOCH_DTYPE element) as a request dict --
    prn, code_ph0, code_dph, carr_ph0, carr_dph -- with `grid` (delay0, n_delay, dopp_step, max_periods, ...) merged in."""
    lib = load_library()
    r = np.ascontiguousarray(rec, dtype=CHAN_EPOCH_DTYPE).reshape(1)
    q = _CorrReq()
    rc = lib.gal_corr_from_epoch(r.ctypes.data, float(sample_rate), int(sample_offset), ctypes.byref(q))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())
    out = {k: int(getattr(q, k)) for k in ("prn", "code_ph0", "code_dph", "carr_ph0", "carr_dph")}
    out.update({k: int(v) for k, v in grid.items()})
    return out


def corr_cn0(sums, req, k_prompt, k_noise, d, sample_rate):
    """gal_corr_cn0 (no GPU needed): (C/N0 in dB-Hz of the composite E1B + E1C signal, Pp / Pn) from the [m, d, k, 4] sums of one
    request, over the whole periods m = 1 .. max_periods - 2.  Raises GalSynthError(GAL_E_INVAL) where there is no peak."""
    lib = load_library()
    q = _corr_struct(req)
    a = np.ascontiguousarray(sums, dtype=np.int64)
    if a.size * 8 != int(lib.gal_synth_corr_out_bytes(ctypes.byref(q))):
        raise ValueError("corr_cn0: sums of %d values do not belong to this request" % a.size)
    cn0, ratio = ctypes.c_double(0.0), ctypes.c_double(0.0)
    rc = lib.gal_corr_cn0(a.ctypes.data, ctypes.byref(q), int(k_prompt), int(k_noise), int(d), float(sample_rate), ctypes.byref(cn0),
                          ctypes.byref(ratio))
    if rc != 0:
        raise GalSynthError(rc, lib.gal_synth_last_error().decode())
    return float(cn0.value), float(ratio.value)


def tables():
    """The signal tables exactly as the engine uses them (numpy copies)."""
    lib = load_library()

    def arr(ptr, ctype, n, shape):
        buf = (ctype * n).from_address(ptr)
        return np.frombuffer(buf, dtype=np.dtype(ctype)).reshape(shape).copy()

    return {
        "e1b": arr(lib.gal_tables_e1b(), ctypes.c_uint32, 50 * 128, (50, 128)),
        "e1c": arr(lib.gal_tables_e1c(), ctypes.c_uint32, 50 * 128, (50, 128)),
        "cos512": arr(lib.gal_tables_cos512(), ctypes.c_int16, 512, (512,)),
        "sin512": arr(lib.gal_tables_sin512(), ctypes.c_int16, 512, (512,)),
        "cs25": int(lib.gal_tables_cs25()),
        "gauss": arr(lib.gal_tables_gauss(), ctypes.c_int32, 32 * 32 * 2, (32, 32, 2)),
        "cos1024": arr(lib.gal_tables_cos1024(), ctypes.c_int16, 1024, (1024,)),
        "scint": arr(lib.gal_tables_scint(), ctypes.c_int32, 32, (32,)),
        "psd": arr(lib.gal_tables_psd(), ctypes.c_int32, 2 * 4096, (2, 4096)),
    }


def pack_page(symbols):
    """500 symbols {0,1} -> 16 little-endian words, bit i of word i>>5 = symbol i."""
    sym = np.asarray(symbols).astype(np.uint8).ravel()
    assert sym.size == GAL_N_SYM_PAGE
    bits = np.zeros(GAL_PAGE_WORDS * 32, dtype=np.uint8)
    bits[:GAL_N_SYM_PAGE] = sym > 0
    return np.packbits(bits, bitorder="little").view("<u4").copy()


def unpack_page(words):
    w = np.ascontiguousarray(np.asarray(words, dtype="<u4"))
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:GAL_N_SYM_PAGE].copy()


class SynthEngine:
    """One handle per GPU / stream (gal_synth_t).  Thread-compatible, not thread-safe."""

    def __init__(self, sample_rate=2.6e6, samples_per_epoch=260000, n_slots=16, device=-1, chunk_samples=0,
                 max_walk_passes=0, flags=0, test_hooks=False):
        self._lib = load_library(hooks=test_hooks)
        self._h = ctypes.c_void_p()
        cfg = _Cfg(float(sample_rate), int(samples_per_epoch), int(n_slots), int(device), int(chunk_samples),
                   int(max_walk_passes), int(flags))
        self._check(self._lib.gal_synth_create(ctypes.byref(cfg), ctypes.byref(self._h)))
        self.sample_rate = float(sample_rate)
        self.samples_per_epoch = int(samples_per_epoch)
        self.n_slots = int(n_slots)
        self.n_epochs = 0
        self._keep = None

    def _check(self, rc):
        if rc != 0:
            raise GalSynthError(rc, self._lib.gal_synth_last_error().decode())

    def close(self):
        if self._h:
            self._lib.gal_synth_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- boundary calls ------------------------------------------------------------------------
    def _params(self, params):
        p = np.ascontiguousarray(params, dtype=CHAN_EPOCH_DTYPE)
        if p.ndim != 2 or p.shape[1] != self.n_slots:
            raise ValueError("params must have shape [n_epochs, n_slots=%d]" % self.n_slots)
        return p

    def _state(self, state_in):
        if state_in is None:
            return None
        s = np.ascontiguousarray(state_in, dtype=CHAN_STATE_DTYPE)
        if s.shape != (self.n_slots,):
            raise ValueError("state_in must have shape [n_slots]")
        return s

    def set_stream(self, hip_stream):
        """hip_stream: integer hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) or None."""
        self._check(self._lib.gal_synth_set_stream(self._h, ctypes.c_void_p(hip_stream or 0)))

    def plan(self, params, state_in=None, wait=True):
        """wait=False: gal_synth_plan_async -- returns once the upload is enqueued; the next execute's walkers wait for it."""
        p = self._params(params)
        s = self._state(state_in)
        fn = self._lib.gal_synth_plan if wait else self._lib.gal_synth_plan_async
        self._check(fn(self._h, p.ctypes.data, p.shape[0], s.ctypes.data if s is not None else None))
        self.n_epochs = p.shape[0]

    def output_bytes(self):
        return int(self._lib.gal_synth_output_bytes(self._h))

    def walk_counts(self):
        """(legs walked, legs translated, fallbacks since create) of the last finish()."""
        a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.gal_synth_walk_counts(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def execute(self, iq_dev_ptr, first_epoch=0, n_epochs=None):
        """iq_dev_ptr: integer device address (e.g. torch tensor .data_ptr()), 16-byte aligned.  With
        first_epoch / n_epochs only that epoch range of the plan is synthesised (into a buffer of that size)."""
        if first_epoch == 0 and n_epochs is None:
            self._check(self._lib.gal_synth_execute(self._h, ctypes.c_void_p(int(iq_dev_ptr))))
        else:
            n = self.n_epochs - first_epoch if n_epochs is None else n_epochs
            self._check(self._lib.gal_synth_execute_range(self._h, ctypes.c_void_p(int(iq_dev_ptr)), int(first_epoch), int(n)))

    def finish(self):
        st = np.zeros(self.n_slots, dtype=CHAN_STATE_DTYPE)
        stats = _Stats()
        self._check(self._lib.gal_synth_finish_n(self._h, st.ctypes.data, ctypes.byref(stats), ctypes.sizeof(_Stats)))
        return st, {k: getattr(stats, k) for k, _ in _Stats._fields_}

    def run_host(self, params, state_in=None):
        """plan + execute + copy to host.  Returns (iq int16 [n_epochs*N*2], state_out, stats)."""
        p = self._params(params)
        s = self._state(state_in)
        iq = np.empty(p.shape[0] * self.samples_per_epoch * 2, dtype=np.int16)
        st = np.zeros(self.n_slots, dtype=CHAN_STATE_DTYPE)
        stats = _Stats()
        self._check(
            self._lib.gal_synth_run_host_n(
                self._h, p.ctypes.data, p.shape[0], s.ctypes.data if s is not None else None, iq.ctypes.data,
                st.ctypes.data, ctypes.byref(stats), ctypes.sizeof(_Stats)
            )
        )
        self.n_epochs = p.shape[0]
        return iq, st, {k: getattr(stats, k) for k, _ in _Stats._fields_}

    def iq_convert(self, iq_ptr, n_samples, fmt, shift=None, out_ptr=None, noise=None, first_sample=0, interf=None):
        """Enqueue on the handle's stream: n_samples complex int16 samples at device address iq_ptr (final output: behind finish())
        -> `fmt` ("ishort" | "ibyte" | "ibit") at device address out_ptr (iq_bytes(fmt, n_samples) bytes, not overlapping the input).
        Both 16-byte aligned; shift 0..15 for "ibyte" (None: IQ_SHIFT_DEFAULT), 0 (or None) otherwise.  iq_saturated() is the fence.
        noise: a dict (seed, stream, gain_q16, sigma_q4; noise_from_cn0 makes one) or a tuple in that order -- the seeded noise floor
        of gal_synth_iq_convert_noise in front of the format; first_sample is then the index of the call's first complex sample in
        the whole output stream, and "ishort" may run in place (out_ptr == iq_ptr).
        interf: a list of up to GAL_INTERF_MAX sources (dicts with the fields of gal_iq_interf_t; interf_make makes one) -- CW, chirp
        and pulsed interference of gal_synth_iq_convert_interf, added in the same pass, with or without `noise`."""
        if out_ptr is None:
            raise ValueError("iq_convert: out_ptr is required")
        if shift is None:
            shift = IQ_SHIFT_DEFAULT if iq_format_code(fmt) == GAL_IQ_IBYTE else 0
        src = [_interf_struct(c) for c in interf or ()]  # (the library itself goes on to the noise / plain call where one is absent)
        nz = _noise_struct(noise) if noise is not None else None
        self._check(self._lib.gal_synth_iq_convert_interf(self._h, ctypes.c_void_p(int(iq_ptr)), int(n_samples), int(first_sample),
                                                          ctypes.byref(nz) if nz is not None else None, (_Interf * max(1, len(src)))(*src),
                                                          len(src), iq_format_code(fmt), int(shift), ctypes.c_void_p(int(out_ptr))))

    def iq_saturated(self, reset=False):
        """Waits for the conversions enqueued so far; int16 values saturated by "ibyte" conversions since create (or the last reset)."""
        n = ctypes.c_uint64(0)
        self._check(self._lib.gal_synth_iq_saturated(self._h, ctypes.byref(n), 1 if reset else 0))
        return int(n.value)

    def iq_wsum(self, part_ptrs, gain_q7, out_ptr):
        """gal_synth_iq_wsum, enqueued on the handle's stream: out = clamp((sum_k gain_q7[e, k] x part k + 64) >> 7) per epoch e, for the
        device addresses part_ptrs (n_epochs x samples_per_epoch complex int16 samples each, 16-byte aligned, none overlapping out_ptr)
        and gain_q7 of shape [n_epochs, n_parts] (0 .. GAL_GAIN_MAX).  iq_saturated() is the fence and counts the clamped values."""
        g = np.asarray(gain_q7)
        if g.ndim != 2 or g.shape[1] != len(part_ptrs):
            raise ValueError("iq_wsum: gain_q7 must have shape [n_epochs, n_parts=%d]" % len(part_ptrs))
        if g.size and (g.min() < 0 or g.max() > 65535):
            raise ValueError("iq_wsum: a gain does not fit a uint16")
        g = np.ascontiguousarray(g, dtype=np.uint16)
        ptrs = (ctypes.c_void_p * max(1, len(part_ptrs)))(*[int(p) for p in part_ptrs])
        self._check(self._lib.gal_synth_iq_wsum(self._h, ptrs, len(part_ptrs), g.ctypes.data, g.shape[0], ctypes.c_void_p(int(out_ptr))))

    def iq_mpath(self, part_ptrs, gain_q7, out_ptr, part_of_echo=(), echo_rows=None, hist_id=None):
        """gal_synth_iq_mpath, enqueued on the handle's stream: iq_wsum plus the echoes echo_rows [n_epochs, n_echo] (ECHO_DTYPE) of the
        parts part_of_echo [n_echo].  hist_id: per part the history line (0 .. 63) that carries its last 1024 samples from call to call,
        -1 for none; None names line k for part k.  Any cut of a stream into calls of whole epochs gives the same bytes.
        iq_saturated() is the fence and counts the clamped values."""
        self._echo_pass("iq_mpath", self._lib.gal_synth_iq_mpath, ECHO_DTYPE, part_ptrs, gain_q7, out_ptr, part_of_echo, echo_rows, hist_id)

    def iq_refl(self, part_ptrs, gain_q7, out_ptr, part_of_echo=(), refl_rows=None, hist_id=None):
        """gal_synth_iq_refl, enqueued on the handle's stream: iq_mpath with rows of REFL_DTYPE, whose frac_q12 adds a fraction of a
        sample to the delay (linear interpolation between two samples).  The history lines are iq_mpath's."""
        self._echo_pass("iq_refl", self._lib.gal_synth_iq_refl, REFL_DTYPE, part_ptrs, gain_q7, out_ptr, part_of_echo, refl_rows, hist_id)

    def _echo_pass(self, who, fn, dtype, part_ptrs, gain_q7, out_ptr, part_of_echo, echo_rows, hist_id):
        """iq_mpath and iq_refl: `fn` over rows of `dtype`."""
        g = np.asarray(gain_q7)
        if g.ndim != 2 or g.shape[1] != len(part_ptrs):
            raise ValueError("%s: gain_q7 must have shape [n_epochs, n_parts=%d]" % (who, len(part_ptrs)))
        if g.size and (g.min() < 0 or g.max() > 65535):
            raise ValueError("%s: a gain does not fit a uint16" % who)
        g = np.ascontiguousarray(g, dtype=np.uint16)
        rows = _echo_table(echo_rows, g.shape[0], who, dtype)
        pof = np.ascontiguousarray(part_of_echo, dtype=np.int32).ravel()
        if pof.size != rows.shape[1]:
            raise ValueError("%s: part_of_echo must have n_echo = %d entries" % (who, rows.shape[1]))
        hid = None if hist_id is None else np.ascontiguousarray(hist_id, dtype=np.int32).ravel()
        if hid is not None and hid.size != len(part_ptrs):
            raise ValueError("%s: hist_id must have n_parts = %d entries" % (who, len(part_ptrs)))
        ptrs = (ctypes.c_void_p * max(1, len(part_ptrs)))(*[int(p) for p in part_ptrs])
        self._check(fn(self._h, ptrs, len(part_ptrs), hid.ctypes.data if hid is not None else None, g.ctypes.data, g.shape[0],
                       pof.ctypes.data if pof.size else None, rows.ctypes.data if rows.size else None, rows.shape[1],
                       ctypes.c_void_p(int(out_ptr))))

    def mpath_reset(self):
        """gal_synth_mpath_reset: zero every history line of iq_mpath / run_mpath (enqueued): the next call starts its streams."""
        self._check(self._lib.gal_synth_mpath_reset(self._h))

    def run_mpath(self, params, gain_q7, iq_dev_ptr, slot_of_echo=(), echo_rows=None, state_in=None):
        """gal_synth_run_mpath: run_gains with the echoes echo_rows [n_epochs, n_echo] (ECHO_DTYPE) of the channel slots slot_of_echo
        [n_echo] -- every such slot is a synthesis run of its own, and its history follows the slot from batch to batch.  No echoes:
        run_gains.  The echo pass is ENQUEUED when this returns (iq_saturated() is the fence).  Returns state_out."""
        return self._run_echo("run_mpath", self._lib.gal_synth_run_mpath, ECHO_DTYPE, params, gain_q7, iq_dev_ptr, slot_of_echo, echo_rows, state_in)

    def run_refl(self, params, gain_q7, iq_dev_ptr, slot_of_echo=(), refl_rows=None, state_in=None):
        """gal_synth_run_refl: run_mpath with rows of REFL_DTYPE and the reflector pass in the place of the echo pass.  Returns state_out."""
        return self._run_echo("run_refl", self._lib.gal_synth_run_refl, REFL_DTYPE, params, gain_q7, iq_dev_ptr, slot_of_echo, refl_rows, state_in)

    def _run_echo(self, who, fn, dtype, params, gain_q7, iq_dev_ptr, slot_of_echo, echo_rows, state_in):
        """run_mpath and run_refl: `fn` over rows of `dtype`."""
        p = self._params(params)
        s = self._state(state_in)
        g = np.asarray(gain_q7)
        if g.shape != p.shape:
            raise ValueError("%s: gain_q7 must have shape [n_epochs, n_slots=%d]" % (who, self.n_slots))
        if g.size and (g.min() < 0 or g.max() > 65535):
            raise ValueError("%s: a gain does not fit a uint16" % who)
        g = np.ascontiguousarray(g, dtype=np.uint16)
        rows = _echo_table(echo_rows, p.shape[0], who, dtype)
        sof = np.ascontiguousarray(slot_of_echo, dtype=np.int32).ravel()
        if sof.size != rows.shape[1]:
            raise ValueError("%s: slot_of_echo must have n_echo = %d entries" % (who, rows.shape[1]))
        st = np.zeros(self.n_slots, dtype=CHAN_STATE_DTYPE)
        self._check(fn(self._h, p.ctypes.data, p.shape[0], s.ctypes.data if s is not None else None, g.ctypes.data,
                       sof.ctypes.data if sof.size else None, rows.ctypes.data if rows.size else None, rows.shape[1],
                       ctypes.c_void_p(int(iq_dev_ptr)), st.ctypes.data))
        self.n_epochs = p.shape[0]
        return st

    def iq_scint(self, jobs):
        """gal_synth_iq_scint, enqueued on the handle's stream, ALL JOBS IN ONE LAUNCH: jobs = a sequence of (in_ptr, out_ptr, n_samples,
        first_sample, row) -- device addresses (16-byte aligned; the same address or disjoint), the global index of the job's first
        sample and a row dict (scint_make makes one).  z is a function of (row, global index) alone: any cut of a stream into calls
        gives the same bytes.  iq_saturated() is the fence and counts the clamped samples."""
        arr = (_ScintJob * max(1, len(jobs)))()
        for k, (src, dst, n, first, row) in enumerate(jobs):
            arr[k] = _ScintJob(int(src) or None, int(dst) or None, int(n), int(first), _scint_struct(row))
        self._check(self._lib.gal_synth_iq_scint(self._h, arr, len(jobs)))

    def run_scint(self, params, gain_q7, iq_dev_ptr, scint_rows=None, first_sample=0, slot_of_echo=(), echo_rows=None, state_in=None):
        """gal_synth_run_scint: run_mpath with the scintillation table scint_rows [n_epochs, n_slots] (SCINT_DTYPE; the module's
        scint_rows makes one) -- every slot with a non-identity row is a synthesis run of its own and its part goes through iq_scint in
        place before the echo pass (or the weighted sum); first_sample = the global index of the batch's first sample.  None:
        run_mpath.  Returns state_out."""
        p = self._params(params)
        s = self._state(state_in)
        g = np.asarray(gain_q7)
        if g.shape != p.shape:
            raise ValueError("run_scint: gain_q7 must have shape [n_epochs, n_slots=%d]" % self.n_slots)
        if g.size and (g.min() < 0 or g.max() > 65535):
            raise ValueError("run_scint: a gain does not fit a uint16")
        g = np.ascontiguousarray(g, dtype=np.uint16)
        rows = _echo_table(echo_rows, p.shape[0], "run_scint")
        sof = np.ascontiguousarray(slot_of_echo, dtype=np.int32).ravel()
        if sof.size != rows.shape[1]:
            raise ValueError("run_scint: slot_of_echo must have n_echo = %d entries" % rows.shape[1])
        sc = None
        if scint_rows is not None:
            sc = np.ascontiguousarray(scint_rows, dtype=SCINT_DTYPE)
            if sc.shape != p.shape:
                raise ValueError("run_scint: scint_rows must have shape [n_epochs, n_slots=%d]" % self.n_slots)
        st = np.zeros(self.n_slots, dtype=CHAN_STATE_DTYPE)
        self._check(self._lib.gal_synth_run_scint(self._h, p.ctypes.data, p.shape[0], s.ctypes.data if s is not None else None, g.ctypes.data,
                                                  sof.ctypes.data if sof.size else None, rows.ctypes.data if rows.size else None, rows.shape[1],
                                                  sc.ctypes.data if sc is not None else None, int(first_sample),
                                                  ctypes.c_void_p(int(iq_dev_ptr)), st.ctypes.data))
        self.n_epochs = p.shape[0]
        return st

    def iq_array(self, part_ptrs, rows, out_ptrs):
        """gal_synth_iq_array, enqueued on the handle's stream: the len(out_ptrs) (1 .. 8) element streams out of the parts at the device
        addresses part_ptrs, each part read once, with the Q12 weights rows [n_epochs, n_elem, n_parts] (STEER_DTYPE, or integers
        [..., 2]): out a = clamp((sum_k part k x rows[e, a, k] + 2048) >> 12), a complex product.  An output may meet neither a part nor
        another output.  iq_saturated() is the fence and counts the clamped values."""
        t = _steer_table(rows, "iq_array")
        if t.shape[1] != len(out_ptrs) or t.shape[2] != len(part_ptrs):
            raise ValueError("iq_array: rows must have shape [n_epochs, n_elem=%d, n_parts=%d]" % (len(out_ptrs), len(part_ptrs)))
        ptrs = (ctypes.c_void_p * max(1, len(part_ptrs)))(*[int(p) for p in part_ptrs])
        outs = (ctypes.c_void_p * max(1, len(out_ptrs)))(*[int(p) for p in out_ptrs])
        self._check(self._lib.gal_synth_iq_array(self._h, ptrs, len(part_ptrs), t.ctypes.data if t.size else None, t.shape[0], len(out_ptrs), outs))

    def run_array(self, params, gain_q7, phase, out_ptrs, scint_rows=None, first_sample=0, state_in=None):
        """gal_synth_run_array: the batch as len(out_ptrs) (1 .. 8) element streams.  gain_q7 [n_epochs, n_slots] (0 .. 1023), phase
        [n_epochs, n_elem, n_slots] in 2^-32 cycles (array_phase makes one).  Every active slot is a synthesis run of its own
        (gain_runs() counts them); scint_rows as for run_scint.  The array pass is ENQUEUED when this returns (iq_saturated() is the
        fence).  Returns state_out."""
        p = self._params(params)
        s = self._state(state_in)
        g = np.asarray(gain_q7)
        if g.shape != p.shape:
            raise ValueError("run_array: gain_q7 must have shape [n_epochs, n_slots=%d]" % self.n_slots)
        if g.size and (g.min() < 0 or g.max() > 65535):
            raise ValueError("run_array: a gain does not fit a uint16")
        g = np.ascontiguousarray(g, dtype=np.uint16)
        ph = np.asarray(phase)
        if ph.shape != (p.shape[0], len(out_ptrs), self.n_slots):
            raise ValueError("run_array: phase must have shape [n_epochs, n_elem=%d, n_slots=%d]" % (len(out_ptrs), self.n_slots))
        ph = np.ascontiguousarray(ph.astype(np.int64) & 0xffffffff, dtype=np.uint32)
        sc = None
        if scint_rows is not None:
            sc = np.ascontiguousarray(scint_rows, dtype=SCINT_DTYPE)
            if sc.shape != p.shape:
                raise ValueError("run_array: scint_rows must have shape [n_epochs, n_slots=%d]" % self.n_slots)
        outs = (ctypes.c_void_p * max(1, len(out_ptrs)))(*[int(q) for q in out_ptrs])
        st = np.zeros(self.n_slots, dtype=CHAN_STATE_DTYPE)
        self._check(self._lib.gal_synth_run_array(self._h, p.ctypes.data, p.shape[0], s.ctypes.data if s is not None else None, g.ctypes.data,
                                                  ph.ctypes.data if ph.size else None, len(out_ptrs), sc.ctypes.data if sc is not None else None,
                                                  int(first_sample), outs, st.ctypes.data))
        self.n_epochs = p.shape[0]
        return st

    def fir_set(self, taps):
        """gal_synth_fir_set: give the handle the front-end filter `taps` (int16 Q14, 1 .. GAL_FIR_MAX_TAPS, sum |h| <= 65535) and start
        a stream (the history is zeroed); None or an empty sequence frees the filter."""
        t = _fir_taps(taps if taps is not None else [], "fir_set")
        self._check(self._lib.gal_synth_fir_set(self._h, t.ctypes.data if t.size else None, int(t.size)))

    def iq_fir(self, in_ptr, n_samples, out_ptr):
        """gal_synth_iq_fir, enqueued on the handle's stream: filter the next n_samples complex int16 samples of the stream, device
        address in_ptr -> out_ptr (both 16-byte aligned, not overlapping).  The handle carries the filter's history from call to call:
        any cut of a stream into calls gives the same bytes.  iq_saturated() is the fence and counts the clamped values."""
        self._check(self._lib.gal_synth_iq_fir(self._h, ctypes.c_void_p(int(in_ptr)), int(n_samples), ctypes.c_void_p(int(out_ptr))))

    def firdec_set(self, taps, decim=2, first_sample=0):
        """gal_synth_firdec_set: give the handle the decimating front-end filter `taps` (int16 Q14, 1 .. GAL_FIRDEC_MAX_TAPS, sum |h|
        <= 65535) at the decimation decim (2 .. GAL_FIRDEC_MAX_DECIM) and start a stream whose next input sample has the global index
        first_sample (the history is zeroed); None or an empty sequence frees it.  Independent of fir_set."""
        t = _fir_taps(taps if taps is not None else [], "firdec_set")
        self._check(self._lib.gal_synth_firdec_set(self._h, t.ctypes.data if t.size else None, int(t.size), int(decim), int(first_sample)))

    def iq_firdec(self, in_ptr, n_in, out_ptr):
        """gal_synth_iq_firdec, enqueued on the handle's stream: consume the next n_in complex int16 input samples at device address
        in_ptr and write the outputs whose decim * m falls into them from device address out_ptr on (both 16-byte aligned, not
        overlapping); returns their number.  Any cut of the input stream into calls gives the same bytes.  iq_saturated() is the fence
        and counts the clamped values."""
        n_out = ctypes.c_size_t(0)
        self._check(self._lib.gal_synth_iq_firdec(self._h, ctypes.c_void_p(int(in_ptr)), int(n_in), ctypes.c_void_p(int(out_ptr)),
                                                  ctypes.byref(n_out)))
        return int(n_out.value)

    def agc_set(self, agc, first_sample=0):
        """gal_synth_agc_set: give the handle the block AGC `agc` (a dict with the fields of gal_iq_agc_t; agc_from_rms makes one) and
        start a stream whose next sample has the global index first_sample (every block in front of it has the power p_init); None
        frees it.  Independent of fir_set and firdec_set."""
        if agc is None:
            self._check(self._lib.gal_synth_agc_set(self._h, None, 0))
            return
        a = _agc_struct(agc)
        self._check(self._lib.gal_synth_agc_set(self._h, ctypes.byref(a), int(first_sample)))

    def iq_agc(self, in_ptr, n_samples, fmt, param, out_ptr, gains_ptr=None):
        """gal_synth_iq_agc, enqueued on the handle's stream: consume the next n_samples complex int16 samples at device address in_ptr
        and write them, gain-controlled, as `fmt` ("ishort" | "ibyte" | "i2bit") to device address out_ptr (agc_out_bytes(fmt,
        n_samples) bytes; both 16-byte aligned, not overlapping).  param: the "ibyte" shift, the "i2bit" threshold, 0 for "ishort".
        gains_ptr: None, or a device address that receives the uint32 Q12 gains of the blocks that start in the call.  Returns their
        number.  Any cut of the stream into calls gives the same bytes and gains.  iq_saturated() is the fence and the counter."""
        n_gains = ctypes.c_size_t(0)
        self._check(self._lib.gal_synth_iq_agc(self._h, ctypes.c_void_p(int(in_ptr)), int(n_samples), agc_format_code(fmt), int(param),
                                               ctypes.c_void_p(int(out_ptr)), ctypes.c_void_p(int(gains_ptr)) if gains_ptr else None,
                                               ctypes.byref(n_gains)))
        return int(n_gains.value)

    def osc_set(self, osc, first_sample=0):
        """gal_synth_osc_set: give the handle the receiver oscillator `osc` (a dict with the fields of gal_iq_osc_t; osc_make makes one)
        and start a stream whose next sample has the global index first_sample (the phase-noise sum Z is 0 there); None switches it
        off.  Independent of fir_set, firdec_set and agc_set."""
        if osc is None:
            self._check(self._lib.gal_synth_osc_set(self._h, None, 0))
            return
        o = _osc_struct(osc)
        self._check(self._lib.gal_synth_osc_set(self._h, ctypes.byref(o), int(first_sample)))

    def iq_osc(self, in_ptr, n_samples, out_ptr):
        """gal_synth_iq_osc, enqueued on the handle's stream: rotate the next n_samples complex int16 samples of the stream by the
        oscillator's phase, device address in_ptr -> out_ptr (both 16-byte aligned; the same address or disjoint).  Any cut of a stream
        into calls gives the same bytes.  iq_saturated() is the fence and counts the clamped samples."""
        self._check(self._lib.gal_synth_iq_osc(self._h, ctypes.c_void_p(int(in_ptr)), int(n_samples), ctypes.c_void_p(int(out_ptr))))

    def run_gains(self, params, gain_q7, iq_dev_ptr, state_in=None):
        """gal_synth_run_gains: the batch with per-slot, per-epoch Q7 gains gain_q7 [n_epochs, n_slots] (128 = unity) into the device
        address iq_dev_ptr (16-byte aligned) -- one synthesis run per group of slots with equal gains, then the weighted sum, which is
        ENQUEUED when this returns (iq_saturated() is the fence).  Returns state_out: per slot the end state of the full run."""
        p = self._params(params)
        s = self._state(state_in)
        g = np.asarray(gain_q7)
        if g.shape != p.shape:
            raise ValueError("run_gains: gain_q7 must have shape [n_epochs, n_slots=%d]" % self.n_slots)
        if g.size and (g.min() < 0 or g.max() > 65535):
            raise ValueError("run_gains: a gain does not fit a uint16")
        g = np.ascontiguousarray(g, dtype=np.uint16)
        st = np.zeros(self.n_slots, dtype=CHAN_STATE_DTYPE)
        self._check(self._lib.gal_synth_run_gains(self._h, p.ctypes.data, p.shape[0], s.ctypes.data if s is not None else None, g.ctypes.data,
                                                  ctypes.c_void_p(int(iq_dev_ptr)), st.ctypes.data))
        self.n_epochs = p.shape[0]
        return st

    def gain_runs(self):
        """gal_synth_gain_runs: synthesis runs (slot groups) the last run_gains took; 1 for the unity case."""
        n = ctypes.c_int32(0)
        self._check(self._lib.gal_synth_gain_runs(self._h, ctypes.byref(n)))
        return int(n.value)

    def correlate(self, buf_ptr, fmt, n_samples, reqs, out_ptr=None):
        """gal_synth_correlate: despread the n_samples complex samples in format `fmt` at device address buf_ptr (16-byte aligned, final
        output) with each request (dicts as corr_from_epoch makes them, or one dict).  Returns the sums as int64 numpy arrays of shape
        [max_periods, n_dopp, n_delay, 4] (Re S_B, Im S_B, Re S_C, Im S_C), one per request (a single array for a single dict); waits
        for them.  out_ptr: a device address for the sums (16-byte aligned, the sum of corr_out_bytes) -- then nothing is copied or
        waited for and None is returned; iq_saturated() is the fence."""
        single = isinstance(reqs, (dict, _CorrReq))
        qs = [_corr_struct(r) for r in ([reqs] if single else reqs)]
        arr = (_CorrReq * max(1, len(qs)))(*qs)
        sizes = [int(self._lib.gal_synth_corr_out_bytes(ctypes.byref(q))) for q in qs]
        if out_ptr is not None:
            self._check(self._lib.gal_synth_correlate(self._h, ctypes.c_void_p(int(buf_ptr)), iq_format_code(fmt), int(n_samples), arr,
                                                      len(qs), ctypes.c_void_p(int(out_ptr))))
            return None
        import torch

        out = torch.empty(max(2, sum(sizes) // 8), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()  # (the block may come from torch's cache with work of torch's stream still behind it)
        self._check(self._lib.gal_synth_correlate(self._h, ctypes.c_void_p(int(buf_ptr)), iq_format_code(fmt), int(n_samples), arr, len(qs),
                                                  ctypes.c_void_p(out.data_ptr())))
        self.iq_saturated()
        host = out.cpu().numpy()
        res, off = [], 0
        for q, nb in zip(qs, sizes):
            res.append(host[off:off + nb // 8].reshape(q.max_periods, q.n_dopp, q.n_delay, 4).copy())
            off += nb // 8
        return res[0] if single else res

    def iq_psd(self, buf_ptr, fmt, n_samples, log2_n, hop, window, out_ptr=None, reserved=0):
        """gal_synth_iq_psd: the Welch power spectrum of the n_samples complex samples in format `fmt` at device address buf_ptr (16-byte
        aligned, final output): N = 2^log2_n, segments `hop` samples apart, window "rect" | "hann" (0 | 1).  Returns (the uint64 sums
        of |X[k]|^2 over the segments, k < N in natural order, n_seg); waits for them.  out_ptr: a device address for the sums (16-byte
        aligned, N uint64) -- then nothing is copied or waited for and (None, n_seg) is returned; iq_saturated() is the fence."""
        cfg = _psd_struct(log2_n, hop, window, reserved)
        n_seg = ctypes.c_int32(0)
        if out_ptr is not None:
            self._check(self._lib.gal_synth_iq_psd(self._h, ctypes.c_void_p(int(buf_ptr)), iq_format_code(fmt), int(n_samples), ctypes.byref(cfg),
                                                   ctypes.c_void_p(int(out_ptr)), ctypes.byref(n_seg)))
            return None, int(n_seg.value)
        import torch

        out = torch.empty(max(2, 1 << max(0, min(int(log2_n), 12))), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()  # (the block may come from torch's cache with work of torch's stream still behind it)
        self._check(self._lib.gal_synth_iq_psd(self._h, ctypes.c_void_p(int(buf_ptr)), iq_format_code(fmt), int(n_samples), ctypes.byref(cfg),
                                               ctypes.c_void_p(out.data_ptr()), ctypes.byref(n_seg)))
        self.iq_saturated()
        return out.cpu().numpy().view(np.uint64)[:1 << int(log2_n)].copy(), int(n_seg.value)
