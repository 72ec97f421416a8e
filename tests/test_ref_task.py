"""THE REFERENCE PROGRAM ITSELF as the judge of the whole path: oracle/_ref/ref_task is the reference's file-sink program compiled
from the reference's own text with its own flags -- no stand-in header or library (oracle/ref_task_harness.cpp, oracle/Makefile) --
so the md5 of what it writes is the reference's answer, produced here.  CPU tests: the recorded golden md5s are reproduced by it,
and the repository's front-end -> oracle chain equals it on scenarios that no recorded md5 covers.  GPU test: the product CLI's
file equals the reference program's file byte for byte, both run on the same command line (the binary travels to the GPU box with
oracle/_ref/; /root/reference is not needed at run time).  tools/ref_task_goldens.py (all nine goldens, profiles/archive/r04_ref_task_md5.log)
and tools/ref_task_fuzz.py (random scenarios, profiles/archive/r04_ref_task_fuzz.log) are the long forms."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_binding import oracle_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ref_task_goldens import ARGS, run_ref_task  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
NAV = os.path.join(G, "20feb2022.rnx")
REF = json.load(open(os.path.join(G, "reference_md5.json")))
BIN = os.path.join(ROOT, "oracle", "_ref", "ref_task")
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
BIN_HIP = os.path.join(ROOT, "oracle", "_ref", "ref_task_hip")

needs_ref_task = pytest.mark.skipif(not os.path.exists(BIN), reason="oracle/_ref/ref_task not built (needs /root/reference at build time)")


@needs_ref_task
@pytest.mark.parametrize("name", ["G1", "G2", "G9"])
def test_reference_program_reproduces_the_recorded_md5(name, tmp_path):
    """The recorded md5s (stand-in-header builds by the survey and the judges) against the reference compiled here without stand-ins."""
    md5, n, _, _ = run_ref_task(BIN, ARGS[name], str(tmp_path / "r.bin"))
    assert (md5, n) == (REF[name]["md5"], REF[name]["bytes"])


# scenarios no recorded md5 covers: another hemisphere and hour each, iono on and off, -T inside the file's span
UNSEEN = [
    dict(llh="-41.3673238,136.919575,2039.16324", t="2022/02/20,16:38:02", d=3, iono=True, T=False),
    dict(llh="71.2,-156.8,10", t="2022/02/20,03:07:41", d=4, iono=False, T=False),
    dict(llh="1.38345806,133.682176,1445.05624", t="2022/02/20,02:03:39", d=3, iono=False, T=True),
    dict(llh="52.8783583,-11.543417,1212.12971", t="2022/02/20,21:44:28", d=32, iono=True, T=False),  # crosses the 30 s re-allocation
]


def _args(k):
    return "-l %s -%s %s -d %g%s" % (k["llh"], "T" if k["T"] else "t", k["t"], k["d"], "" if k["iono"] else " -I 1")


# the reference program's answers on UNSEEN, recorded by oracle/_ref/ref_task: where the binary is not built they stand in for it,
# where it is, the tests below hold the record to it
UNSEEN_REF = json.load(open(os.path.join(G, "ref_task_unseen.json")))["cases"]


def _reference_answer(k, path):
    """(md5, bytes) of the reference program's file for scenario k: run live when oracle/_ref/ref_task is built, recorded otherwise."""
    rec = UNSEEN_REF[_args(k)]
    if not os.path.exists(BIN):
        return rec["md5"], rec["bytes"]
    md5, n, _, _ = run_ref_task(BIN, _args(k), path)
    assert {"md5": md5, "bytes": n} == rec, "tests/golden/ref_task_unseen.json differs from the reference program"
    return md5, n


@pytest.mark.parametrize("k", UNSEEN, ids=[k["t"][-8:] for k in UNSEEN])
def test_front_end_and_oracle_equal_the_reference_program(pkg, k, tmp_path):
    ref_md5, ref_n = _reference_answer(k, str(tmp_path / "r.bin"))
    rows = pkg.Scenario(NAV, llh=tuple(float(v) for v in k["llh"].split(",")), start=k["t"], duration_s=k["d"], iono_enable=k["iono"],
                        time_overwrite="ref" if k["T"] else False).all()
    assert (rows["prn"] > 0).any()
    iq, _ = oracle_run(rows, 260000, 2.6e6)
    assert (hashlib.md5(iq.tobytes()).hexdigest(), iq.nbytes) == (ref_md5, ref_n)


@pytest.mark.gpu
@pytest.mark.parametrize("k", UNSEEN, ids=[k["t"][-8:] for k in UNSEEN])
def test_cli_file_equals_the_reference_programs_file(k, tmp_path):
    """Same command line into the reference program and into the product CLI (front-end -> HIP -> file): the same bytes (where the
    reference program is not built, the md5 and size of its file, recorded in tests/golden/ref_task_unseen.json)."""
    ref_path, out = str(tmp_path / "r.bin"), str(tmp_path / "o.bin")
    ref_md5, ref_n = _reference_answer(k, ref_path)
    # (the very same arguments, -T included: plain -T is the reference as built)
    r = subprocess.run([CLI, "-e", NAV] + _args(k).split() + ["-P", "0", "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    b = np.fromfile(out, dtype=np.int16)
    assert b.size * 2 == ref_n and b.any()
    if os.path.exists(ref_path):
        assert np.array_equal(np.fromfile(ref_path, dtype=np.int16), b)
    assert hashlib.md5(b.tobytes()).hexdigest() == ref_md5


@pytest.mark.skipif(not (os.path.exists(BIN) and os.path.exists(BIN_HIP)), reason="oracle/_ref/ref_task{,_hip} not built")
@pytest.mark.gpu
@pytest.mark.parametrize("k", [UNSEEN[0], UNSEEN[3]], ids=["3s", "32s_across_a_refresh"])
def test_reference_with_the_loop_patch_writes_the_reference_file(k, tmp_path):
    """THE DROP-IN ON THE REFERENCE ITSELF.  oracle/_ref/ref_task_hip is the reference's file-sink program with its per-sample loop
    (src/galileo-sdr.cpp:481-539) replaced by galileo-sdr-sim_amd/integration/galileo_sdr_loop_patch.inc -- INTEGRATION.md section B,
    the text a maintainer would add: channel records out of chan[], one gal_synth_run_host() per epoch into iq_buff, carrier phase
    and page back into chan[] -- and linked against libgalsynth.so; everything else (RINEX, orbits, channel allocation, page
    generation, fwrite) is the reference's own code.  Its file must be the unpatched reference program's, byte for byte."""
    ref_path, out = str(tmp_path / "r.bin"), str(tmp_path / "h.bin")
    _, ref_n, _, _ = run_ref_task(BIN, _args(k), ref_path)
    md5, n, _, _ = run_ref_task(BIN_HIP, _args(k), out)
    assert n == ref_n and n > 0
    a, b = np.fromfile(ref_path, dtype=np.int16), np.fromfile(out, dtype=np.int16)
    assert a.any() and np.array_equal(a, b)


# ---- answers the reference program gave HERE, kept as a fixture: tests/golden/ref_task_recorded.json (tools/ref_task_fuzz.py --record:
# every random case with the md5 and the byte count of the reference's file).  Needs neither /root/reference nor the binary at test time.
RECORDED = os.path.join(G, "ref_task_recorded.json")


def _recorded(max_dur, count):
    if not os.path.exists(RECORDED):
        return []
    cases = [k for k in json.load(open(RECORDED)) if k["recorded"][0] not in (None, "timeout") and k["dur"] <= max_dur]
    step = max(1, len(cases) // count)
    return cases[::step][:count]


def _case_args(k):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from ref_task_fuzz import case_args
    return case_args(dict(k, llh=tuple(k["llh"])))


@pytest.mark.parametrize("k", _recorded(3.0, 8), ids=lambda k: "case%d" % k["c"])
def test_front_end_and_oracle_reproduce_recorded_reference_answers(pkg, k):
    args = _case_args(k)
    llh = (42.3601, -71.0589, 2.0) if k["no_l"] else tuple(float(v) for v in args.split()[1].split(","))
    sc = pkg.Scenario(NAV, llh=llh, start=None if k["no_t"] else k["start"], duration_s=k["dur"], iono_enable=k["iono"], time_overwrite="ref" if k["tovr"] else False)
    rows = sc.all()
    if sc.eph_gaps:
        pytest.skip("ephemeris gap: the reference's behaviour is undefined there")
    iq, _ = oracle_run(rows, 260000, 2.6e6)
    assert [hashlib.md5(iq.tobytes()).hexdigest(), iq.nbytes] == k["recorded"][:2], args


@pytest.mark.gpu
@pytest.mark.parametrize("k", _recorded(5.0, 32), ids=lambda k: "case%d" % k["c"])
def test_cli_reproduces_recorded_reference_answers(k, tmp_path):
    args = _case_args(k)
    out = str(tmp_path / "o.bin")
    r = subprocess.run([CLI, "-e", NAV] + args.split() + ["-P", "0", "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if "no ephemeris within an hour" in r.stderr:
        pytest.skip("ephemeris gap: the reference's behaviour is undefined there")
    data = open(out, "rb").read()
    assert [hashlib.md5(data).hexdigest(), len(data)] == k["recorded"][:2], args


RECORDED_300S = os.path.join(G, "ref_task_recorded_300s.json")


def _recorded_300s():
    if not os.path.exists(RECORDED_300S):
        return []
    return [k for k in json.load(open(RECORDED_300S)) if k["recorded"][0] not in (None, "timeout")]


@pytest.mark.gpu
def test_cli_reproduces_recorded_reference_answers_of_300s_runs():
    """30 random scenarios of 200-300 s -- up to the reference's cap of 3000 epochs (USER_MOTION_SIZE,
    include/constants.h:14), six to ten 30 s re-allocations and several TOC marks per run -- whose answers the reference program gave
    where it can be built (tools/ref_task_fuzz.py 30 606 6 --long300 --record ...): the product CLI on the same command line must
    write the same bytes (md5 and count; 2-3 GB per case, into /dev/shm, four cases at a time: the runs are bound by the host's md5)."""
    from concurrent.futures import ThreadPoolExecutor

    cases = _recorded_300s()
    assert len(cases) >= 29
    shm = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else "/tmp"

    def run(k):
        args = _case_args(k)
        out = os.path.join(shm, "galtest_%d_300s_%d.ishort" % (os.getpid(), k["c"]))
        try:
            r = subprocess.run([CLI, "-e", NAV] + args.split() + ["-P", "0", "-o", out], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                return k["c"], args, "exit %d: %s" % (r.returncode, r.stderr[-300:])
            if "no ephemeris within an hour" in r.stderr:
                return k["c"], args, None  # ephemeris gap: the reference's behaviour is undefined there
            h, n = hashlib.md5(), 0
            with open(out, "rb") as fh:
                for blk in iter(lambda: fh.read(1 << 24), b""):
                    h.update(blk)
                    n += len(blk)
        finally:
            if os.path.exists(out):
                os.remove(out)
        return k["c"], args, None if [h.hexdigest(), n] == k["recorded"][:2] else "md5 %s, %d bytes; the reference: %s" % (h.hexdigest(), n, k["recorded"][:2])

    with ThreadPoolExecutor(4) as ex:
        res = list(ex.map(run, cases))
    bad = [r for r in res if r[2] is not None]
    assert not bad, bad


def test_front_end_and_oracle_reproduce_a_config5_unit_of_the_reference_program(pkg):
    """BASELINE config 5's per-rank unit, 300 s at one of its eight sites (tests/golden/ref_task_config5.json: the reference program's
    md5 and byte count for every site, recorded by tools/ref_task_config5.py): front-end -> oracle on the CPU gives the reference's
    file for the site with the fewest satellites (5 SVs, 35 s of CPU); all eight go through the product on the GPU box
    (tests/test_cli.py::test_cli_config5_all_eight_sites)."""
    rec = json.load(open(os.path.join(G, "ref_task_config5.json")))
    k = 4
    assert tuple(rec["sites"][k]["llh"]) == tuple(pkg.shard.LOCATIONS[k])
    rows = pkg.Scenario(NAV, llh=pkg.shard.LOCATIONS[k], start=rec["start"], duration_s=rec["duration_s"], iono_enable=True).all()
    h, st, n = hashlib.md5(), None, 0
    for a in range(0, rows.shape[0], 200):
        iq, st = oracle_run(rows[a:a + 200], 260000, 2.6e6, state_in=st)
        h.update(iq.tobytes())
        n += iq.nbytes
    assert (h.hexdigest(), n) == (rec["sites"][k]["md5"], rec["sites"][k]["bytes"])
