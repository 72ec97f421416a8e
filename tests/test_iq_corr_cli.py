"""galileo-sdr-sim --monitor: the argument checks (no GPU: they fail before any device work) and, on the MI355X, a 20 s run under
a 45 dB-Hz noise floor -- every line names the planned delay and Doppler as the strongest, every PRN of the plan appears, and the IQ
file is the one the same command writes without --monitor."""
import hashlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
G1 = ["-l", "-6,51,100", "-t", "2022/02/20,12:00:00", "-U", "1", "-b", "1", "-I", "1", "-P", "0"]  # the golden scenario G1's sky


def _run(args, **kw):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=600, **kw)


def test_monitor_argument_checks(pkg, tmp_path):
    """Each of these ends with exit code 1 and its own message before the scenario is opened or a device is touched (the navigation
    file named does not even exist)."""
    nav = str(tmp_path / "does_not_exist.rnx")
    mon = str(tmp_path / "m.csv")
    r = _run(["-e", nav, "--monitor-every", "5"])
    assert r.returncode == 1 and "--monitor-every needs --monitor" in r.stderr
    for bad in ("0", "-3", "ten", "2000000", ""):
        r = _run(["-e", nav, "--monitor", mon, "--monitor-every", bad])
        assert r.returncode == 1 and "--monitor-every" in r.stderr and "out of range" in r.stderr, bad
    r = _run(["-e", nav, "--monitor", str(tmp_path / "no_such_dir" / "m.csv")])
    assert r.returncode == 1 and "cannot write the monitor file" in r.stderr
    r = _run(["-e", nav, "--monitor", "-"])
    assert r.returncode == 1 and "--monitor needs a file name" in r.stderr
    r = _run(["-e", nav, "--monitor", mon, "-C"])
    assert r.returncode == 1 and "does not go with -C" in r.stderr
    r = _run(["-e", nav, "--monitor"])
    assert r.returncode == 1
    # accepted: the run then fails at the navigation file, not at the option
    r = _run(["-e", nav, "--monitor", mon, "--monitor-every", "7"])
    assert r.returncode == 1 and "--monitor" not in r.stderr and "monitor file" not in r.stderr
    h = _run(["-e"])
    assert "--monitor <file>" in h.stdout and "--monitor-every" in h.stdout


@pytest.mark.gpu
def test_monitor_run_names_the_plan_and_leaves_the_iq_alone(pkg, tmp_path):
    """20 s at --cn0 45.  All satellites share one power, so every estimate sits below 45 dB-Hz by the multiple-access floor of the
    others: not bounded here, written to monitor_cn0.txt in the test's directory (DESIGN.md section 12 quotes a run)."""
    common = ["-e", NAV] + G1 + ["-d", "20", "--cn0", "45"]
    with_mon, without = str(tmp_path / "a.ishort"), str(tmp_path / "b.ishort")
    mon = str(tmp_path / "monitor.csv")
    r = _run(common + ["-o", with_mon, "--monitor", mon])
    assert r.returncode == 0, r.stderr[-2000:]
    r0 = _run(common + ["-o", without])
    assert r0.returncode == 0, r0.stderr[-2000:]

    def md5(path):
        h = hashlib.md5()
        with open(path, "rb") as f:
            for piece in iter(lambda: f.read(1 << 24), b""):
                h.update(piece)
        return h.hexdigest()

    assert os.path.getsize(with_mon) == 199 * 260000 * 4
    assert md5(with_mon) == md5(without)
    lines = open(mon).read().strip().split("\n")
    assert lines[0] == "time_s,prn,doppler_hz,cn0_dbhz,peak_ratio,best_delay_halfchips,best_doppler_bins"
    rows = [ln.split(",") for ln in lines[1:]]
    assert rows and all(len(x) == 7 for x in rows)
    times = sorted({float(x[0]) for x in rows})
    assert times == [float(t) for t in range(0, 20)]  # every 10th epoch of 199
    per_prn = {}
    for x in rows:
        assert (x[5], x[6]) == ("0", "0"), x  # the planned delay and Doppler bin are the strongest
        per_prn.setdefault(int(x[1]), []).append(float(x[3]))
    summary = [ln for ln in r.stderr.split("\n") if ln.strip().startswith("PRN")]
    assert sorted(per_prn) == sorted(int(ln.split()[1].rstrip(":")) for ln in summary)
    # every PRN of the plan: the front-end's own rows of the monitored epochs
    sc = pkg.Scenario(NAV, llh=(-6.0, 51.0, 100.0), start="2022/02/20,12:00:00", duration_s=20.0, iono_enable=False)
    plan = sc.all()
    sc.close()
    assert plan.shape[0] == 199
    planned = {}
    for e in range(0, 199, 10):
        for prn in plan["prn"][e][plan["prn"][e] > 0]:
            planned[int(prn)] = planned.get(int(prn), 0) + 1
    assert len(planned) >= 4 and {k: len(v) for k, v in per_prn.items()} == planned
    with open(str(tmp_path / "monitor_cn0.txt"), "w") as f:
        for prn in sorted(per_prn):
            v = per_prn[prn]
            f.write("PRN %2d: %d epochs, C/N0 mean %.2f min %.2f max %.2f dB-Hz\n" % (prn, len(v), sum(v) / len(v), min(v), max(v)))
    print(open(str(tmp_path / "monitor_cn0.txt")).read())
    print("\n".join(summary))
