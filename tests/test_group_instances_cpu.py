"""The census behind tests/test_group_instances_gpu.py, without a GPU: the dispatch model (tests/group_instance_model.py) against the
host-only plan of the hooks build for every batch of the matrix, the union of the matrix's instances against the model's reachable
set, the model's channel counts and forms against the launchers' switch statements in synth_group.hip, and what the sweep shows about
the accumulating instances below six positions: none of them can be launched."""
import os
import re

import pytest

import group_instance_model as gim
import test_group_instances_gpu as matrix

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "galileo-sdr-sim_amd", "csrc")


@pytest.fixture(scope="module")
def matrix_instances(pkg):
    """{(family, form, n_chan): the instances the model names} for every batch, each checked against the plan on the way."""
    saved = {k: os.environ.pop(k, None) for k in ("GAL_G_WIDE", "GAL_G_NARROW", "GAL_G_LINEAR", "GAL_G_SEARCH")}
    out = {}
    try:
        for family, form in matrix.CASES:
            if family == "wide":
                os.environ["GAL_G_WIDE"] = "1"
            for n_chan in matrix.channels_of(family):
                p, rate, flags = matrix.build_batch(pkg, family, form, n_chan)
                out[family, form, n_chan] = matrix.check_plan(pkg, family, form, p, rate, flags)
            os.environ.pop("GAL_G_WIDE", None)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return out


def test_model_against_the_plan(pkg, matrix_instances):
    """check_plan has compared family, form, launches per execute and every launch's size with the plan; here: the batches are what
    the matrix is said to be -- 2 k channels launch <k, false> and <k, true>, an idle slot leaves the sizes alone."""
    assert len(matrix_instances) == 16 * len(matrix.NARROW_CHANNELS) + 4 * len(matrix.WIDE_CHANNELS)
    for (family, form, n_chan), inst in matrix_instances.items():
        p, rate, _ = matrix.build_batch(pkg, family, form, n_chan)
        assert matrix.active_counts(p) == [n_chan, n_chan - (1 if n_chan >= 3 else 0), n_chan]
        limit = gim.WIDE_MAX if family == "wide" else gim.NARROW_MAX
        if n_chan <= limit:
            assert inst == [(family, n_chan, False, form)]
        elif n_chan % 2 == 0:
            assert inst == [(family, n_chan // 2, False, form), (family, n_chan // 2, True, form)]
        else:
            assert inst == [(family, 7, False, form), (family, 6, True, form)] and n_chan == 13
        # every Doppler but the legacy family's one record is inside the linear gate, signs alternate, no two are equal
        f = p["f_carr"][0, :n_chan]
        f_in = matrix.f_carr_at_limit(rate)
        assert (abs(f[1:]) <= f_in).all() and (abs(f[0]) <= f_in) == (family != "legacy")
        assert len(set(abs(f))) == n_chan and ((f[1::2] < 0).all() and (f[2::2] > 0).all())


def test_census(matrix_instances):
    covered = set()
    for inst in matrix_instances.values():
        covered.update(inst)
    reachable = gim.reachable_set()
    print("reachable instances: %d of %d compiled, per family %s" % (len(reachable), len(gim.compiled_set()), gim.per_family(reachable)))
    assert reachable <= gim.compiled_set()
    assert sorted(reachable - covered) == [], "reachable and not in the matrix"
    assert sorted(covered - reachable) == []
    assert len(reachable) == 400 and gim.per_family(reachable) == {"linear": 76, "legacy": 76, "search": 76, "cboc": 76, "wide": 96}


def test_source_against_model():
    """The channel counts the launchers' switch statements name, and their forms: a change there must be followed in the model."""
    with open(os.path.join(CSRC, "synth_group.hip")) as f:
        src = f.read()

    def counts(macro):
        return tuple(int(n) for n in re.findall(r"\b%s\((\d+)\)" % macro, src))

    assert counts("GAL_CASE") == counts("GAL_LCASE") == counts("GAL_SCASE") == gim.NARROW_COUNTS == tuple(range(1, 13))
    assert counts("GAL_WCASE") == gim.WIDE_COUNTS == tuple(range(13, 25))
    mode_lists = re.findall(r"switch \((?:mode|P->rw)\) \{\s*((?:(?:GAL_MCASE|SG_MODE_CASE)\(\d\)\s*)+)default:", src)
    assert len(mode_lists) == 5                   # wide, bisection, linear start; the CBOC and the BOC(1,1) switch of galk_launch_synth_g
    for m in mode_lists:
        assert tuple(int(d) for d in re.findall(r"\((\d)\)", m)) == gim.MODES == (1, 2, 3, 4)
    assert int(re.search(r"#define SG_MAXCH (\d+)", src).group(1)) == gim.NARROW_MAX
    with open(os.path.join(CSRC, "synth_api.cpp")) as f:
        api = f.read()
    assert int(re.search(r"constexpr int kKernelMaxChan = (\d+);", api).group(1)) == gim.NARROW_MAX
    assert int(re.search(r"constexpr int kGroupMaxChan = (\d+);", api).group(1)) == gim.WIDE_MAX
    assert int(re.search(r"constexpr int kGroupChunk = (\d+);", api).group(1)) == gim.GROUP_CHUNK
    assert len(gim.compiled_set()) == 480


def test_accumulating_instances_below_six_positions_are_never_launched():
    """A later launch exists only for more than 12 positions (24 with the wide instances), and its share of the largest epoch is at
    least 6 (13 = 7 + 6, 61 = 5 x 11 + 6); with three to five launches at least 7.  So k_synth_g<1..5, true, ...> of the four narrow
    families -- 5 counts x 4 forms x 4 families = 80 instances -- are compiled and never launched; every wide instance is reachable."""
    unreachable = gim.unreachable_set()
    assert unreachable == {(fam, nch, True, mode) for fam in gim.FAMILIES[:4] for nch in range(1, 6) for mode in gim.MODES}
    assert len(unreachable) == 80
    least = {}
    for most in range(1, gim.MAX_CHAN + 1):
        sizes = gim.launch_sizes([most], gim.NARROW_MAX)
        assert sum(sizes) == most and max(sizes) <= gim.NARROW_MAX and sizes[0] == max(sizes)
        if len(sizes) > 1:
            least[len(sizes)] = min(least.get(len(sizes), 99), min(sizes[1:]))
    assert least == {2: 6, 3: 7, 4: 7, 5: 7, 6: 6}
    # epochs of different sizes: a launch's size is the maximum over the epochs, never below its share of the largest epoch
    for a in range(0, gim.MAX_CHAN + 1):
        for b in range(max(a, 1), gim.MAX_CHAN + 1):
            for max_ch in (gim.NARROW_MAX, gim.WIDE_MAX):
                alone, both = gim.launch_sizes([b], max_ch), gim.launch_sizes([a, b], max_ch)
                assert len(both) == len(alone) and both[0] == alone[0]
                assert all(x <= y <= max_ch for x, y in zip(alone, both)), (a, b, alone, both)
