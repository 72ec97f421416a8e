"""galileo-sdr-sim --spectrum on the MI355X: every line of the CSV, the total included, is the numpy model (tests/psd_model.py) run
on the IQ file the same command wrote; the IQ file does not change and the CSV does not depend on -B; a --jam tone lands in the bin
it was put in; a --fir-lowpass removes what its taps say; the refusals."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import psd_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
G1 = ["-l", "-6,51,100", "-t", "2022/02/20,12:00:00", "-U", "1", "-b", "1", "-I", "1", "-P", "0"]  # the golden scenario G1's sky
N_EPOCH = 260000
# -d 1.1: the command writes (int)(10 d + 0.5) - 1 epochs, so 1.1 s are the TEN epochs 0 .. 9 of which every third is 0, 3, 6, 9
TEN = ["-d", "1.1"]


def _run(args, **kw):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=600, **kw)


def _ok(args):
    r = _run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _md5(path):
    with open(path, "rb") as f:
        return hashlib.md5(f.read()).hexdigest()


def _csv(path):
    """(header, [(time, n_seg, [python ints in frequency order])], (segments, [totals]))"""
    lines = open(path).read().strip().split("\n")
    assert lines[0].startswith("#")
    rows = []
    for ln in lines[1:-1]:
        x = ln.split(",")
        rows.append((float(x[0]), int(x[1]), [int(v) for v in x[2:]]))
    t = lines[-1].split(",")
    assert t[0] == "total"
    return lines[0], rows, (int(t[1]), [int(v) for v in t[2:]])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ("ishort", "ibyte"))
def test_csv_is_the_model_on_the_file(pkg, tmp_path, fmt):
    common = ["-e", NAV] + G1 + TEN + ["--cn0", "45", "--iq-format", fmt]
    iq, plain, csv, csv3 = (str(tmp_path / n) for n in ("a.iq", "b.iq", "s.csv", "s3.csv"))
    r = _ok(common + ["-o", iq, "-B", "1", "--spectrum", csv, "--spectrum-every", "3"])
    _ok(common + ["-o", plain, "-B", "1"])
    _ok(common + ["-o", str(tmp_path / "c.iq"), "-B", "3", "--spectrum", csv3, "--spectrum-every", "3"])
    assert _md5(iq) == _md5(plain) == _md5(str(tmp_path / "c.iq"))
    assert open(csv).read() == open(csv3).read()
    code = {"ishort": 0, "ibyte": 1}[fmt]
    per = N_EPOCH * (4 if fmt == "ishort" else 2)
    raw = np.fromfile(iq, dtype=np.uint8)
    assert raw.size == 10 * per
    head, rows, (tot_seg, tot) = _csv(csv)
    for word in ("N=1024", "hop=512", "window=hann", "format=" + fmt, "fs_hz=2600000", "sum_win2=%d" % int((psd_model.window(10, 1) ** 2).sum()),
                 "frequency order"):
        assert word in head, word
    assert [t for t, _, _ in rows] == [0.0, 0.3, 0.6, 0.9]
    want_tot = [0] * 1024
    for (t, n_seg, p), e in zip(rows, (0, 3, 6, 9)):
        v = psd_model.values(raw[e * per:(e + 1) * per], code)
        want, want_seg = psd_model.psd(v, code, 10, 512, 1)
        assert n_seg == want_seg == 506
        ordered = [int(x) for x in np.roll(want, 512)]  # frequency order: bin -N / 2 first
        assert p == ordered, (fmt, e)
        want_tot = [a + b for a, b in zip(want_tot, ordered)]
    assert tot_seg == 4 * 506 and tot == want_tot
    assert "Spectrum (" in r.stderr and "peak at" in r.stderr and "99 % of the power within" in r.stderr


@pytest.mark.gpu
def test_ibit_epochs_off_the_16_byte_grid(pkg, tmp_path):
    """ibit: 65 000 bytes per epoch, so every odd epoch of a batch begins 8 bytes off the 16-byte grid the library asks for and is
    copied to an aligned line first: at -B 3 with every epoch reported, the lines are still the model's on the file's epochs, and the
    file at -B 1"""
    common = ["-e", NAV] + G1 + ["-d", "0.7", "--cn0", "45", "--iq-format", "ibit", "--spectrum-every", "1", "--spectrum-size", "64"]
    iq, csv, csv1 = (str(tmp_path / n) for n in ("a.ibit", "s.csv", "s1.csv"))
    _ok(common + ["-o", iq, "-B", "3", "--spectrum", csv])
    _ok(common + ["-o", str(tmp_path / "b.ibit"), "-B", "1", "--spectrum", csv1])
    assert open(csv).read() == open(csv1).read()
    raw = np.fromfile(iq, dtype=np.uint8)
    assert raw.size == 6 * 65000
    _, rows, (tot_seg, _) = _csv(csv)
    assert len(rows) == 6
    for e, (t, n_seg, p) in enumerate(rows):
        want, want_seg = psd_model.psd(psd_model.values(raw[e * 65000:(e + 1) * 65000], 2), 2, 6, 32, 1)
        assert n_seg == want_seg and p == [int(x) for x in np.roll(want, 32)], e
    assert tot_seg == sum(r[1] for r in rows)


@pytest.mark.gpu
def test_a_tone_lands_where_it_was_put(pkg, tmp_path):
    """406 250 Hz = 160 x 2.6 MHz / 1024: bin +160 exactly"""
    csv = str(tmp_path / "s.csv")
    r = _ok(["-e", NAV] + G1 + TEN + ["--cn0", "45", "--jam", "30,406250", "--spectrum-size", "1024", "--spectrum", csv, "-o", str(tmp_path / "a.iq")])
    _, rows, (_, tot) = _csv(csv)
    assert len(tot) == 1024 and int(np.argmax(np.array(tot, dtype=np.float64))) - 512 == 160
    assert "peak at +406250.0 Hz (bin +160)" in r.stderr


@pytest.mark.gpu
def test_a_filter_removes_what_it_says(pkg, tmp_path):
    """The per-bin ratio of the totals with and without --fir-lowpass 500000 against |H(f)|^2 of the taps the command prints, over
    groups of 16 bins, where |H|^2 >= -40 dB: within 1 dB.  29 epochs x 506 segments = 14 674 half-overlapping Hann segments (the
    equivalent of 0.52 x 14 674 independent ones; Welch 1967) x 16 bins: a standard deviation of 10 / ln 10 / sqrt(0.52 x 14 674 x 16) =
    0.012 dB per total, 0.018 dB for the ratio.  The Hann window smears each bin over +-2 bins (main lobe 4 bins = 10 kHz wide): a
    group's mean ratio follows the mean of |H|^2 over the group only where |H|^2 is smooth over that width, so the comparison is
    restricted, as the issue allows, to groups across which |H|^2 changes by less than 3 dB; the margin stays 1 dB."""
    common = ["-e", NAV] + G1 + ["-d", "3", "--cn0", "45", "--spectrum-every", "1", "-o", "/dev/null"]
    a, b = str(tmp_path / "fir.csv"), str(tmp_path / "plain.csv")
    r = _ok(common + ["--fir-lowpass", "500000", "--spectrum", a])
    _ok(common + ["--spectrum", b])
    m = re.search(r"Front-end filter: low-pass, cutoff \S+ Hz, (\d+) taps \(Q14\):((?: -?\d+)+)", r.stderr)
    assert m, r.stderr[-2000:]
    taps = np.array([int(x) for x in m.group(2).split()], dtype=np.float64) / 16384.0
    assert taps.size == int(m.group(1))
    _, _, (seg_a, ta) = _csv(a)
    _, _, (seg_b, tb) = _csv(b)
    assert seg_a == seg_b == 29 * 506 >= 7000
    f = (np.arange(1024) - 512) / 1024.0  # cycles per sample, frequency order
    H2 = np.abs(np.exp(-2j * np.pi * np.outer(f, np.arange(taps.size))) @ taps) ** 2
    ratio = (np.array(ta, dtype=np.float64).reshape(64, 16).sum(axis=1)) / (np.array(tb, dtype=np.float64).reshape(64, 16).sum(axis=1))
    h2g = H2.reshape(64, 16)
    used, worst = 0, 0.0
    for g in range(64):
        lo, hi = h2g[g].min(), h2g[g].max()
        if lo < 1e-4 or 10 * np.log10(hi / lo) >= 3.0:
            continue
        d = abs(10 * np.log10(ratio[g]) - 10 * np.log10(h2g[g].mean()))
        print("group %2d: |H|^2 %.3f dB, measured %.3f dB" % (g, 10 * np.log10(h2g[g].mean()), 10 * np.log10(ratio[g])))
        used += 1
        worst = max(worst, d)
    assert used >= 20, used  # the pass band (1 MHz of 2.6: 25 groups) at the least
    assert worst <= 1.0, worst


def test_refusals(pkg, tmp_path):
    """before the scenario is opened or a device is touched (the navigation file named does not even exist)"""
    nav = str(tmp_path / "does_not_exist.rnx")
    csv = str(tmp_path / "s.csv")
    arr = tmp_path / "array.txt"
    arr.write_text("0,0,0\n0.1,0,0\n")
    sites = tmp_path / "sites.txt"
    sites.write_text("-6,51,100\n")
    for extra in (["--iq-format", "i2bit"], ["--array", str(arr)], ["--sites", str(sites)]):
        r = _run(["-e", nav, "--spectrum", csv] + extra)
        assert r.returncode != 0 and "--spectrum" in r.stderr, (extra, r.stderr[-500:])
    r = _run(["-e", nav, "--spectrum-every", "5"])
    assert r.returncode == 1 and "need --spectrum" in r.stderr
    for bad in ("7", "1000", "4", "8192", "x"):
        r = _run(["-e", nav, "--spectrum", csv, "--spectrum-size", bad])
        assert r.returncode == 1 and "--spectrum-size" in r.stderr, bad
    r = _run(["-e", nav, "--spectrum", csv, "--spectrum-window", "hamming"])
    assert r.returncode == 1 and "--spectrum-window" in r.stderr
    r = _run(["-e", nav, "--spectrum", csv, "--spectrum-every", "0"])
    assert r.returncode == 1 and "--spectrum-every" in r.stderr
    r = _run(["-e", nav, "--spectrum", str(tmp_path / "no_such_dir" / "s.csv")])
    assert r.returncode == 1 and "cannot write the spectrum file" in r.stderr
    # accepted: the run then fails at the navigation file, not at the option
    r = _run(["-e", nav, "--spectrum", csv, "--spectrum-size", "4096", "--spectrum-window", "rect", "--spectrum-every", "2"])
    assert r.returncode == 1 and "ERROR: --spectrum" not in r.stderr
