#!/usr/bin/env python3
"""Records what the galileo-sdr-sim executable does, so that a change to the command's own code can be held against it:

  tools/cli_golden.py transcript   the option stage -> tests/golden/cli_transcript.json (any machine: no device is touched)
  tools/cli_golden.py chain        the run loop     -> tests/golden/cli_chain_md5.json  (needs the MI355X)

Both are run at the commit whose behaviour is to be kept; tests/test_cli_transcript.py and tests/test_cli_chain_gpu.py only read the
two files and compare for equality.  The case lists live here, and the fixtures carry them along (argument vectors, input files).
tests/test_cli_chain_model_gpu.py takes the chain's scenario, cases and runner (run_chain_files) from here and computes the bytes."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE_WORD = "galileo-sdr-sim"  # what the executable's own path is replaced with (usage text, getopt's complaints)

# ---- the option stage ------------------------------------------------------------------------------------------------------------------
# -e names a navigation file that does not exist: every case ends in front of gal_scen_open or at it.  File names are relative to the
# case's working directory, which holds FILES.
FILES = {
    "taps.txt": "1000\n14384\n1000\n",
    "taps_text.txt": "1000\nabc\n",
    "taps_range.txt": "40000\n",
    "taps_many.txt": "1\n" * 129,
    "taps_many_dec.txt": "1\n" * 513,
    "taps_none.txt": "\n  \n",
    "taps_sum.txt": "16384\n" * 5,
    "taps4.txt": "4096\n4096\n4096\n4096\n",
    "ant.txt": "# dB per 5 degrees off the zenith\n" + " ".join("%.1f" % (0.25 * k) for k in range(37)) + "\n",
    "ant_short.txt": "0 1 2\n",
    "ant_text.txt": "0 1 x\n",
    "mp.txt": "# prn,delay_m,rel_db,phase_deg[,fade_hz]\n5,300,-6,90\n5,650,-10,0,0.5\n",
    "mp_line.txt": "5,300,-6\n",
    "mp_prn.txt": "51,300,-6,90\n",
    "mp_many.txt": "".join("%d,300,-6,90\n" % (k + 1) for k in range(33)),
    "mp_per_prn.txt": "7,300,-6,90\n" * 5,
    "mp_none.txt": "# nothing\n\n",
    "mp_far.txt": "5,400000,-6,90\n",
    "mp_loud.txt": "5,300,7,90\n",
    "sites_bad.txt": "# lat,lon,hgt\nnot a site\n1,2\n",
    "sites.txt": "10,20,30\n11,21,31,second.ishort\n",
}
E = ["-e", "absent.rnx"]


def _c(name, *args):
    return {"name": name, "argv": list(args)}


TRANSCRIPT_CASES = [
    # usage and the reference's own wording on stdout
    _c("no_args"), _c("one_arg", "-v"), _c("unknown_option", "-e", "absent.rnx", "--no-such-option"), _c("missing_argument", "-v", "-e"),
    _c("no_nav", "-v", "-v"), _c("bad_date", *E, "-t", "2022-02-20"), _c("bad_date_T", *E, "-T", "yesterday"),
    _c("shift_toe_without_T", *E, "--shift-toe"), _c("ref_T_without_T", *E, "--ref-T"),
    _c("shift_toe_and_ref_T", *E, "-T", "2022/02/20,12:00:00", "--shift-toe", "--ref-T"),
    _c("plain", *E), _c("plain_T", *E, "-T", "2022/02/20,12:00:00", "--shift-toe", "-o", "x.ishort"),
    # format, shift, threshold
    _c("format_unknown", *E, "--iq-format", "ifloat"), _c("format_ibyte", *E, "--iq-format", "ibyte"), _c("format_ibit", *E, "--iq-format", "ibit"),
    _c("shift_not_ibyte", *E, "--iq-shift", "3"), _c("shift_range", *E, "--iq-format", "ibyte", "--iq-shift", "16"),
    _c("shift_text", *E, "--iq-format", "ibyte", "--iq-shift", "3x"), _c("shift_empty", *E, "--iq-format", "ibyte", "--iq-shift", ""),
    _c("thr_not_i2bit", *E, "--i2bit-threshold", "100"), _c("thr_range", *E, "--iq-format", "i2bit", "--i2bit-threshold", "0"),
    _c("thr_range_hi", *E, "--iq-format", "i2bit", "--i2bit-threshold", "32768"),
    # AGC
    _c("agc_block_without_agc", *E, "--agc-block", "100"), _c("agc_log_without_agc", *E, "--agc-log", "g.csv"),
    _c("agc_ibit", *E, "--agc", "--iq-format", "ibit"), _c("monitor_i2bit", *E, "--iq-format", "i2bit", "--monitor", "m.csv"),
    _c("agc_block_range", *E, "--agc", "--agc-block", "15"), _c("agc_block_text", *E, "--agc", "--agc-block", "x"),
    _c("agc_window_range", *E, "--agc", "--agc-window", "65"), _c("agc_span", *E, "--agc", "--agc-block", "65536", "--agc-window", "2"),
    _c("agc_target_range", *E, "--agc=0.001"), _c("agc_target_text", *E, "--agc=12x"), _c("agc_target_hi", *E, "--agc", "40000"),
    _c("agc_init_range", *E, "--agc", "--agc-init-rms", "-1"), _c("agc_init_hi", *E, "--agc", "--agc-init-rms", "32769"),
    _c("agc_log_name", *E, "--agc", "--agc-log", "-"), _c("agc_log_sites", *E, "--agc", "--agc-log", "g.csv", "--sites", "sites.txt", "--gpus", "1"),
    _c("agc_log_unwritable", *E, "--agc", "--agc-log", "no_such_dir/g.csv"),
    _c("agc_from_rms", *E, "--agc", "--iq-format", "ibyte", "--iq-shift", "15"),
    _c("agc_ishort", *E, "--agc"), _c("agc_ishort_target_next_word", *E, "--agc", "4096", "-v"), _c("agc_ishort_target_point", *E, "--agc", ".5"),
    _c("agc_not_a_target", *E, "--agc", "-v"),
    _c("agc_ibyte", *E, "--agc", "--iq-format", "ibyte", "--agc-block", "1300", "--agc-window", "4", "--agc-log", "g.csv"),
    _c("agc_i2bit", *E, "--iq-format", "i2bit", "--i2bit-threshold", "900", "--agc-init-rms", "500"),
    _c("agc_init_behind_filter", *E, "--agc", "--cn0", "45", "--fir-lowpass", "1e6,25"),
    _c("agc_init_behind_decimator", *E, "--agc", "--cn0", "45", "--oversample", "2", "--iq-format", "ibyte"),
    # signal power
    _c("prn_power_text", *E, "--prn-power", "5:-6,x"), _c("prn_power_prn", *E, "--prn-power", "51:3"), _c("prn_power_db", *E, "--prn-power", "5:61"),
    _c("antenna_absent", *E, "--antenna", "absent.txt"), _c("antenna_short", *E, "--antenna", "ant_short.txt"),
    _c("antenna_text", *E, "--antenna", "ant_text.txt"),
    _c("power_all", *E, "--power-model", "--antenna", "ant.txt", "--prn-power", "5:-6,12:3", "--prn-power", "7:1.5"),
    _c("power_model_alone", *E, "--power-model"), _c("power_cn0", *E, "--power-model", "--prn-power", "3:6", "--cn0", "40"),
    # multipath
    _c("mp_absent", *E, "--multipath", "absent.txt"), _c("mp_line", *E, "--multipath", "mp_line.txt"), _c("mp_prn", *E, "--multipath", "mp_prn.txt"),
    _c("mp_many", *E, "--multipath", "mp_many.txt"), _c("mp_per_prn", *E, "--multipath", "mp_per_prn.txt"), _c("mp_none", *E, "--multipath", "mp_none.txt"),
    _c("mp_far", *E, "--multipath", "mp_far.txt"), _c("mp_loud", *E, "--multipath", "mp_loud.txt"),
    _c("mp_two_echoes", *E, "--multipath", "mp.txt"), _c("mp_oversampled", *E, "--multipath", "mp.txt", "--oversample", "15", "--cn0", "45"),
    # oversampling and the filters
    _c("osr_range", *E, "--oversample", "1"), _c("osr_range_hi", *E, "--oversample", "16"), _c("osr_text", *E, "--oversample", "2.5"),
    _c("osr_default_taps", *E, "--oversample", "2"), _c("osr_lowpass", *E, "--oversample", "3", "--fir-lowpass", "1.1e6,49"),
    _c("osr_cn0_ibyte", *E, "--oversample", "2", "--cn0", "45", "--iq-format", "ibyte"),
    _c("osr_cn0_ibyte_jam_agc", *E, "--oversample", "2", "--cn0", "45", "--iq-format", "ibyte", "--jam", "30,2e6", "--agc"),
    _c("osr_cn0_ibyte_shift", *E, "--oversample", "2", "--cn0", "45", "--iq-format", "ibyte", "--iq-shift", "6"),
    _c("osr_fir_file", *E, "--oversample", "2", "--fir", "taps4.txt"), _c("osr_fir_many", *E, "--oversample", "2", "--fir", "taps_many_dec.txt"),
    _c("osr_monitor_taps", *E, "--oversample", "2", "--fir-lowpass", "1e6,63", "--monitor", "m.csv"),
    _c("osr_monitor", *E, "--oversample", "2", "--monitor", "m.csv", "-B", "4"),
    _c("fir_both", *E, "--fir", "taps.txt", "--fir-lowpass", "1e6"), _c("fir_absent", *E, "--fir", "absent.txt"), _c("fir_text", *E, "--fir", "taps_text.txt"),
    _c("fir_range", *E, "--fir", "taps_range.txt"), _c("fir_many", *E, "--fir", "taps_many.txt"), _c("fir_none", *E, "--fir", "taps_none.txt"),
    _c("fir_sum", *E, "--fir", "taps_sum.txt"), _c("fir_file", *E, "--fir", "taps.txt", "--cn0", "45", "--iq-format", "ibyte"),
    _c("lowpass_text", *E, "--fir-lowpass", "abc"), _c("lowpass_comma", *E, "--fir-lowpass", "1e6,"), _c("lowpass_tail", *E, "--fir-lowpass", "1e6,25x"),
    _c("lowpass_cutoff", *E, "--fir-lowpass", "2e6"), _c("lowpass_even", *E, "--fir-lowpass", "1e6,24"), _c("lowpass_default", *E, "--fir-lowpass", "1e6"),
    _c("lowpass_25", *E, "--fir-lowpass", "1e6,25"),
    # noise floor
    _c("seed_without_cn0", *E, "--noise-seed", "3"), _c("stream_without_cn0", *E, "--noise-stream", "3"), _c("gain_without_cn0", *E, "--signal-gain", "0.5"),
    _c("cn0_text", *E, "--cn0", "45dB"), _c("cn0_empty", *E, "--cn0", ""), _c("cn0_low", *E, "--cn0", "-40"), _c("cn0_low_given_gain", *E, "--cn0", "0", "--signal-gain", "1"),
    _c("gain_range", *E, "--cn0", "45", "--signal-gain", "17"), _c("gain_text", *E, "--cn0", "45", "--signal-gain", "x"),
    _c("seed_text", *E, "--cn0", "45", "--noise-seed", "12x"), _c("seed_negative", *E, "--cn0", "45", "--noise-seed", "-1"),
    _c("seed_overflow", *E, "--cn0", "45", "--noise-seed", "18446744073709551616"),
    _c("stream_range", *E, "--cn0", "45", "--noise-stream", "4294967296"), _c("stream_negative", *E, "--cn0", "45", "--noise-stream", "-1"),
    _c("cn0_gain_1", *E, "--cn0", "45"), _c("cn0_gain_below_1", *E, "--cn0", "25"), _c("cn0_given_gain", *E, "--cn0", "45", "--signal-gain", "0.75"),
    _c("cn0_seed_stream", *E, "--cn0", "45", "--noise-seed", "0x10", "--noise-stream", "7", "--iq-format", "ibit"),
    _c("cn0_ibyte", *E, "--cn0", "45", "--iq-format", "ibyte"), _c("cn0_ibyte_shift", *E, "--cn0", "45", "--iq-format", "ibyte", "--iq-shift", "4"),
    _c("cn0_ibyte_low", *E, "--cn0", "30", "--iq-format", "ibyte"),
    # interference
    _c("jam_five", *E, *(["--jam", "10,1000"] * 5)), _c("jam_text", *E, "--jam", "10"), _c("jam_three", *E, "--jam", "10,1000,2000"),
    _c("jam_no_sweep", *E, "--jam", "10,1000,2000,0"), _c("jam_tail", *E, "--jam", "10,1000,"), _c("jam_frequency", *E, "--jam", "10,2e6"),
    _c("jam_pulse", *E, "--jam", "10,1000,0,0,100,200"), _c("jam_amplitude", *E, "--jam", "60,1000", "--signal-gain", "16"),
    _c("jam_gain_range", *E, "--jam", "10,1000", "--signal-gain", "0"),
    _c("jam_alone", *E, "--jam", "20,1000"), _c("jam_alone_ibyte", *E, "--jam", "30,-5e5,5e5,100", "--iq-format", "ibyte"),
    _c("jam_alone_ibyte_agc", *E, "--jam", "30,1000", "--iq-format", "ibyte", "--agc"), _c("jam_alone_given_gain", *E, "--jam", "20,1000", "--signal-gain", "0.5", "--iq-format", "ibyte", "--iq-shift", "7"),
    _c("jam_loud", *E, "--jam", "45,1000", "--jam", "40,0,0,0,1000,100"),
    _c("jam_cn0", *E, "--jam", "30,1000,3e5,50", "--cn0", "45", "--iq-format", "ibyte"),
    _c("jam_cn0_agc", *E, "--jam", "30,1000", "--cn0", "45", "--agc", "--iq-format", "ibyte"),
    _c("jam_cn0_agc_ishort", *E, "--jam", "40,1000", "--jam", "35,2000,0,0,500,100", "--cn0", "42", "--agc", "1500"),
    _c("jam_oversampled", *E, "--jam", "10,2e6", "--oversample", "2"),
    # monitor
    _c("every_without_monitor", *E, "--monitor-every", "5"), _c("every_range", *E, "--monitor", "m.csv", "--monitor-every", "0"),
    _c("every_text", *E, "--monitor", "m.csv", "--monitor-every", "x"), _c("monitor_name", *E, "--monitor", "-"), _c("monitor_empty", *E, "--monitor", ""),
    _c("monitor_cboc", *E, "--monitor", "m.csv", "-C"), _c("monitor_unwritable", *E, "--monitor", "no_such_dir/m.csv"),
    _c("monitor", *E, "--monitor", "m.csv", "--monitor-every", "3"),
    # oscillator
    _c("osc_seed_alone", *E, "--osc-seed", "5"), _c("osc_stream_alone", *E, "--osc-stream", "5"), _c("lo_text", *E, "--lo-offset", "abc"),
    _c("lo_comma", *E, "--lo-offset", "1500,"), _c("lo_tail", *E, "--lo-offset", "1500,2,3"), _c("lo_range", *E, "--lo-offset", "1.3e6"),
    _c("pn_text", *E, "--phase-noise", "x"), _c("pn_tail", *E, "--phase-noise", "1e-21s"), _c("pn_negative", *E, "--phase-noise", "-1e-21"),
    _c("pn_range", *E, "--phase-noise", "1e-9"), _c("osc_seed_negative", *E, "--lo-offset", "10", "--osc-seed", "-3"),
    _c("osc_seed_text", *E, "--lo-offset", "10", "--osc-seed", "3x"), _c("osc_stream_range", *E, "--lo-offset", "10", "--osc-stream", "4294967296"),
    _c("osc_stream_text", *E, "--lo-offset", "10", "--osc-stream", ""),
    _c("lo_drift", *E, "--lo-offset", "1500,2"), _c("lo_alone", *E, "--lo-offset", "-250.5"),
    _c("pn_seed_stream", *E, "--phase-noise", "1e-21", "--osc-seed", "99", "--osc-stream", "3"),
    _c("osc_oversampled", *E, "--lo-offset", "1500,2", "--phase-noise", "1e-21", "--oversample", "2"),
    # everything at once: the order of the informational lines
    _c("all", *E, "--power-model", "--antenna", "ant.txt", "--prn-power", "5:-6", "--multipath", "mp.txt", "--oversample", "2", "--cn0", "45",
       "--jam", "30,1000", "--fir-lowpass", "1.1e6,33", "--agc", "--agc-log", "g.csv", "--iq-format", "ibyte", "--lo-offset", "1500,2", "--phase-noise", "1e-21",
       "--monitor", "m.csv", "-o", "all.ibyte"),
    _c("first_refusal_wins", *E, "--iq-shift", "99", "--cn0", "x", "--jam", "1", "--lo-offset", "x"),
    # --sites: the option stage runs (silently), then the site list is read
    _c("sites_absent", *E, "--sites", "absent.txt", "--gpus", "1"), _c("sites_malformed", *E, "--sites", "sites_bad.txt", "--gpus", "1", "--cn0", "45"),
    _c("sites_ports", *E, "--sites", "sites.txt", "--gpus", "1", "-P", "65535"), _c("sites_refusal", *E, "--sites", "sites.txt", "--gpus", "1", "--cn0", "x"),
]


def run_transcript_case(exe, case, files):
    """One case in a fresh directory that holds `files`; the executable's own path does not appear in what is returned."""
    with tempfile.TemporaryDirectory() as d:
        for name, text in files.items():
            with open(os.path.join(d, name), "w") as fh:
                fh.write(text)
        r = subprocess.run([exe] + case["argv"], cwd=d, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    return {"exit": r.returncode, "stdout": r.stdout.replace(exe, EXE_WORD), "stderr": r.stderr.replace(exe, EXE_WORD)}


def record_transcript():
    names = [c["name"] for c in TRANSCRIPT_CASES]
    assert len(set(names)) == len(names)
    cases = [dict(c, **run_transcript_case(CLI, c, FILES)) for c in TRANSCRIPT_CASES]
    with open(os.path.join(GOLDEN, "cli_transcript.json"), "w") as fh:
        json.dump({"files": FILES, "cases": cases}, fh, indent=1)
        fh.write("\n")
    print("%d cases, exit codes %s" % (len(cases), sorted(set(c["exit"] for c in cases))))


# ---- the run loop ------------------------------------------------------------------------------------------------------------------------
# G1's sky, four epochs: -B 1 wraps the two output slots and the three row buffers, -B 3 ends on a short batch
NAV = os.path.join(GOLDEN, "20feb2022.rnx")
CHAIN_SCEN = ["-l", "-6,51,100", "-t", "2022/02/20,12:00:00", "-d", "0.5", "-U", "1", "-b", "1", "-I", "1", "-P", "0"]
CHAIN_BATCHES = (1, 3)
OSC = ["--lo-offset", "1500,2", "--phase-noise", "1e-21"]
CHAIN_FILES = {"mp.txt": "# PRNs 5 and 9 are in view, 17 is not\n5,300,-6,90\n5,650,-10,0,0.5\n9,200,-3,45\n17,300,-6,0\n",
               "sc.txt": "# prn,s4,tau0_s: 5 has echoes in mp.txt\n5,0.8,0.02\n9,0.5,0.05\n17,0.9,0.02\n",
               "arr.txt": "0,0,0\n0.095,0,0\n0,0.12,0.05\n"}
# name, format, options; "monitor" / "agc_log" ask for the side files; "elements": --array's files out.a<k>.<fmt>, hashed one behind the other
CHAIN_CASES = [
    {"name": "plain_ishort", "fmt": "ishort", "argv": []},
    {"name": "ibit_alone", "fmt": "ibit", "argv": []},
    {"name": "cn0_ibyte_fused", "fmt": "ibyte", "argv": ["--cn0", "45"]},
    {"name": "osc_ishort", "fmt": "ishort", "argv": OSC},
    {"name": "cn0_jam_osc_ibyte", "fmt": "ibyte", "argv": ["--cn0", "45", "--jam", "30,1000,3e5,50"] + OSC},
    {"name": "cn0_agc_log_ishort", "fmt": "ishort", "argv": ["--cn0", "45", "--agc"], "agc_log": True},
    {"name": "jam_osc_i2bit", "fmt": "i2bit", "argv": ["--jam", "25,1000"] + OSC},
    {"name": "cn0_osc_fir_agc_monitor_ibyte", "fmt": "ibyte", "argv": ["--cn0", "45", "--fir-lowpass", "1e6,25", "--agc", "--monitor-every", "1"] + OSC, "monitor": True},
    {"name": "osr_cn0_osc_mpath_power_ibyte", "fmt": "ibyte", "argv": ["--oversample", "2", "--cn0", "45", "--multipath", "mp.txt", "--power-model"] + OSC},
    {"name": "power_prn_ishort", "fmt": "ishort", "argv": ["--power-model", "--prn-power", "5:-6,9:3"]},
    {"name": "mpath_alone_monitor_ishort", "fmt": "ishort", "argv": ["--multipath", "mp.txt", "--monitor-every", "2"], "monitor": True},
    {"name": "scint_mpath_power_ishort", "fmt": "ishort", "argv": ["--scint", "sc.txt", "--multipath", "mp.txt", "--power-model"]},
    {"name": "array_scint_cn0_ibyte", "fmt": "ibyte", "argv": ["--array", "arr.txt", "--scint", "sc.txt", "--cn0", "45"], "elements": 3},
    {"name": "refl_cn0_osc_ibyte", "fmt": "ibyte", "argv": ["--reflector", "ground,2,-6", "--reflector", "wall,100,90,-3", "--cn0", "45"] + OSC},
]


def _md5(*blobs):
    h = hashlib.md5()
    for blob in blobs:
        h.update(blob)
    return h.hexdigest()


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def run_chain_files(exe, case, batch, files):
    """One run; returns what it wrote: "iq" (the bytes of the IQ file, or of every element's), the side files asked for, "stderr"."""
    with tempfile.TemporaryDirectory() as d:
        for name, text in files.items():
            with open(os.path.join(d, name), "w") as fh:
                fh.write(text)
        out = "out." + case["fmt"]
        argv = ["-e", NAV] + CHAIN_SCEN + ["--iq-format", case["fmt"], "-B", str(batch), "-o", out] + case["argv"]
        if case.get("monitor"):
            argv += ["--monitor", "mon.csv"]
        if case.get("agc_log"):
            argv += ["--agc-log", "agc.csv"]
        r = subprocess.run([exe] + argv, cwd=d, capture_output=True, text=True, timeout=120, stdin=subprocess.DEVNULL)
        if r.returncode != 0:
            raise RuntimeError("%s -B %d: exit %d\n%s" % (case["name"], batch, r.returncode, r.stderr[-2000:]))
        outs = [os.path.join(d, "out.a%d.%s" % (k, case["fmt"])) for k in range(case["elements"])] if case.get("elements") else [os.path.join(d, out)]
        wrote = {"iq": [_read(o) for o in outs], "stderr": r.stderr}
        if case.get("monitor"):
            wrote["monitor"] = _read(os.path.join(d, "mon.csv"))
        if case.get("agc_log"):
            wrote["agc_log"] = _read(os.path.join(d, "agc.csv"))
    return wrote


def run_chain_case(exe, case, batch, files):
    """One run; returns the md5 of the IQ file and of the side files asked for."""
    wrote = run_chain_files(exe, case, batch, files)
    got = {"iq": _md5(*wrote["iq"]), "iq_bytes": sum(len(b) for b in wrote["iq"])}
    if case.get("monitor"):
        got["monitor"] = _md5(wrote["monitor"])
        got["monitor_lines"] = len(wrote["monitor"].decode().splitlines())
    if case.get("agc_log"):
        got["agc_log"] = _md5(wrote["agc_log"])
    return got


def record_chain():
    cases = []
    for c in CHAIN_CASES:
        got = {str(b): run_chain_case(CLI, c, b, CHAIN_FILES) for b in CHAIN_BATCHES}
        print(c["name"], got, flush=True)
        cases.append(dict(c, expected=got))
    with open(os.path.join(GOLDEN, "cli_chain_md5.json"), "w") as fh:
        json.dump({"scenario": CHAIN_SCEN, "files": CHAIN_FILES, "cases": cases}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "transcript":
        record_transcript()
    elif len(sys.argv) == 2 and sys.argv[1] == "chain":
        record_chain()
    else:
        sys.exit(__doc__)
