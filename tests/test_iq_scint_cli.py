"""galileo-sdr-sim --scint: the refused files and options with their messages and the printed rows (before any device work) and, on the
MI355X, the file -- the same bytes for two batch lengths, the plain run's file at s4 = 0 and for a PRN that is not in view, another
file for another --scint-seed."""
import hashlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "galileo-sdr-sim_amd", "galileo-sdr-sim")
NAV = os.path.join(ROOT, "tests", "golden", "20feb2022.rnx")
START = "2022/02/20,12:00:00"
G1 = ["-l", "-6,51,100", "-t", START, "-d", "2", "-U", "1", "-b", "1", "-I", "1", "-P", "0"]  # the golden scenario G1's sky, 19 epochs
EPOCHS = 19
FS = 2.6e6
LINE = re.compile(r"Scintillation: PRN (\d+), S4 (\S+), tau0 (\S+) s -> A (\d+), B (\d+), L (\d+) \(tau0 (\S+) s at (\S+) MS/s\), seed (\d+), stream (\d+)")


def _run(args, **kw):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=600, **kw)


def _ok(args):
    r = _run(["-e", NAV] + G1 + args)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _md5(path):
    return hashlib.md5(open(str(path), "rb").read()).hexdigest()


@pytest.fixture(scope="module")
def sky(pkg):
    rows = pkg.Scenario(NAV, llh=(-6, 51, 100), start=START, duration_s=2, iono_enable=False).all()
    assert rows.shape[0] == EPOCHS
    rows.setflags(write=False)
    return rows


def _in_view(sky):
    return [int(p) for p in sky["prn"][0] if p > 0], next(p for p in range(1, 51) if not (sky["prn"] == p).any())


def test_refused_files_and_options_before_any_device_work(tmp_path):
    f = tmp_path / "s.txt"
    cases = [("5,0.8\n", "line 1 is not prn,s4,tau0_s"), ("5,0.8,0.5,1\n", "line 1 is not prn,s4,tau0_s"), ("5,abc,0.5\n", "line 1 is not"),
             ("# only a comment\n\n", "it holds no satellite"), ("0,0.5,0.5\n", "PRN outside 1..50"), ("51,0.5,0.5\n", "PRN outside 1..50"),
             ("5.5,0.5,0.5\n", "PRN outside 1..50"), ("5,0.5,0.5\n# again\n5,0.2,0.5\n", "line 3: a second line for PRN 5"),
             ("5,1.5,0.5\n", "line 1: s4 outside 0..1"), ("5,-0.1,0.5\n", "line 1: s4 outside 0..1"),
             ("5,0.5,0.0001\n", "node_len"), ("5,0.5,100\n", "node_len"), ("5,0.5,-1\n", "node_len")]
    for text, want in cases:
        f.write_text(text)
        r = _run(["-e", NAV] + G1 + ["-o", str(tmp_path / "x.ishort"), "--scint", str(f)])
        assert r.returncode == 1 and "ERROR: --scint" in r.stderr and want in r.stderr, (text, r.stderr[-500:])
    r = _run(["-e", NAV] + G1 + ["-o", str(tmp_path / "x.ishort"), "--scint", str(tmp_path / "missing.txt")])
    assert r.returncode == 1 and "cannot read it" in r.stderr
    f.write_text("5,0.5,0.5\n")
    for extra, want in ((["--scint-seed", "-1"], "--scint-seed '-1' is not an unsigned 64-bit integer"),
                        (["--scint-seed", "x"], "--scint-seed 'x'"), (["--scint-site", str(1 << 24)], "--scint-site")):
        r = _run(["-e", NAV] + G1 + ["-o", str(tmp_path / "x.ishort"), "--scint", str(f)] + extra)
        assert r.returncode == 1 and want in r.stderr, r.stderr[-500:]
    for extra in (["--scint-seed", "3"], ["--scint-site", "3"]):
        r = _run(["-e", NAV] + G1 + ["-o", str(tmp_path / "x.ishort")] + extra)
        assert r.returncode == 1 and "need --scint <file>" in r.stderr
    assert not (tmp_path / "x.ishort").exists()


@pytest.mark.parametrize("osr", [1, 3])
def test_the_printed_rows_are_those_of_scint_make(pkg, tmp_path, osr):
    """The lines come out of the option stage, in front of any device work: they are there with or without a GPU.  A comment behind
    the values, blanks around them; the rate is the one the synthesis runs at; stream = site << 8 | prn."""
    f = tmp_path / "s.txt"
    spec = [(5, 0.8, 0.5), (12, 0.3, 1.0), (31, 1.0, 0.02), (7, 0.0, 2.0)]
    f.write_text("# prn,s4,tau0_s\n\n5,0.8,0.5\n 12 , 0.3 , 1.0   # mild\n31,1,0.02\n7,0,2\n")
    args = ["--scint", str(f), "--scint-seed", "77", "--scint-site", "3"] + (["--oversample", str(osr)] if osr > 1 else [])
    r = _run(["-e", NAV] + G1 + ["-o", str(tmp_path / "x.ishort")] + args)
    got = {int(m.group(1)): m for m in LINE.finditer(r.stdout + r.stderr)}
    assert sorted(got) == [5, 7, 12, 31], (r.stdout + r.stderr)[-2000:]
    for prn, s4, tau0 in spec:
        want = pkg.scint_make(s4, tau0, osr * FS)
        m = got[prn]
        assert (int(m.group(4)), int(m.group(5)), int(m.group(6))) == (want["a_q12"], want["b_q12"], want["node_len"]), prn
        assert abs(float(m.group(7)) - 8.0 * want["node_len"] / (osr * FS)) < 1e-6 * tau0 + 1e-9
        assert abs(float(m.group(8)) - osr * 2.6) < 1e-9 and int(m.group(9)) == 77 and int(m.group(10)) == (3 << 8) | prn
    # the headroom: the largest (A + 4 B) / 4096, here the Rayleigh row's
    ray = pkg.scint_make(1.0, 0.02, osr * FS)
    m = re.search(r"a satellite is taken at up to (\S+) times its own amplitude", r.stdout + r.stderr)
    assert m and abs(float(m.group(1)) - 4.0 * ray["b_q12"] / 4096.0) < 1e-3


@pytest.mark.gpu
def test_the_file_for_two_batch_lengths_seeds_and_the_identity(pkg, sky, tmp_path):
    in_view, absent = _in_view(sky)
    f = tmp_path / "s.txt"
    f.write_text("%d,0.8,0.02\n%d,0.4,0.05\n%d,0.9,0.02\n" % (in_view[0], in_view[2], absent))
    plain = tmp_path / "plain.ishort"
    _ok(["-o", str(plain)])
    assert os.path.getsize(str(plain)) == 4 * EPOCHS * 260000
    a, b, c = tmp_path / "a.ishort", tmp_path / "b.ishort", tmp_path / "c.ishort"
    _ok(["-o", str(a), "--scint", str(f), "-B", "4"])
    _ok(["-o", str(b), "--scint", str(f), "-B", "7"])
    assert os.path.getsize(str(a)) == os.path.getsize(str(plain))
    assert _md5(a) == _md5(b) != _md5(plain)
    _ok(["-o", str(c), "--scint", str(f), "-B", "7", "--scint-seed", "2"])
    assert _md5(c) not in (_md5(a), _md5(plain))
    _ok(["-o", str(c), "--scint", str(f), "-B", "7", "--scint-seed", "1", "--scint-site", "0"])  # the defaults, spelled out
    assert _md5(c) == _md5(a)
    _ok(["-o", str(c), "--scint", str(f), "-B", "7", "--scint-site", "1"])
    assert _md5(c) not in (_md5(a), _md5(plain))
    # s4 = 0 for every PRN, and a PRN that is not in view: the file of the run without the option
    f.write_text("".join("%d,0,0.5\n" % p for p in range(1, 51)))
    _ok(["-o", str(c), "--scint", str(f)])
    assert _md5(c) == _md5(plain)
    f.write_text("%d,0.9,0.02\n" % absent)
    _ok(["-o", str(c), "--scint", str(f), "-B", "5"])
    assert _md5(c) == _md5(plain)
