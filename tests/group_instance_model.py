"""Which k_synth_g<NCH, ACC, MODE, ...> instances one execute launches, restated from the host code in plain Python -- the dispatch only,
none of the kernel's arithmetic (synth_api.cpp: the plan's add_groups and narrow_g, enqueue_synth's `accumulate = k > 0`; synth_group.hip:
galk_launch_synth_g / launch_synth_g_t).  A batch is what the dispatch sees of it: the number of records fit for the kernel in every
epoch, its window form, the verdicts of the plan's gates (bisection instances, linear carrier start), the CBOC flag and the hooks.

The kernel is compiled for 12 channel counts x ACC x 4 forms in five families (compiled_set): 480 instances.  reachable_set sweeps the
largest epoch of a batch over 1 .. GAL_ENGINE_MAX_CHAN and says which of them a plan can launch at all: 400.  What is left out are the
accumulating instances below 6 positions of the four narrow families (unreachable_set: 5 x 4 x 4 = 80): a later launch exists only
for more than 12 positions, and the even split of 13 is 7 + 6.

Epochs of different sizes add nothing to that set.  The number of launches comes from the largest epoch; a launch's size is the
maximum over the epochs; the first launch's is the largest epoch's own share, and a later launch's is at least its share of the largest
epoch and at most the launch limit -- values the sweep has already (test_group_instances_cpu.py tries every pair of epoch sizes)."""

MAX_CHAN = 64                 # GAL_ENGINE_MAX_CHAN
NARROW_MAX = 12               # kKernelMaxChan, SG_MAXCH: GAL_CASE / GAL_LCASE / GAL_SCASE name 1 .. 12
WIDE_MAX = 24                 # kGroupMaxChan: GAL_WCASE names 13 .. 24
MODES = (1, 2, 3, 4)          # SG_MODE_CASE / GAL_MCASE
FAMILIES = ("linear", "legacy", "search", "cboc", "wide")
NARROW_COUNTS = tuple(range(1, NARROW_MAX + 1))
WIDE_COUNTS = tuple(range(NARROW_MAX + 1, WIDE_MAX + 1))
GROUP_CHUNK = 1024            # kGroupChunk


def narrow_g(n_epochs, n_samp, search=False, hooks=()):
    """The plan's narrow_g: the wide instances only where a block is a whole long epoch and the launch has many rounds of them, never
    for a batch on the bisection instances; GAL_G_NARROW / GAL_G_WIDE of the hooks build override the sizes."""
    narrow = not (n_epochs >= 2048 and (n_samp + GROUP_CHUNK - 1) // GROUP_CHUNK >= 1024) or search
    if "GAL_G_NARROW" in hooks:
        narrow = True
    if "GAL_G_WIDE" in hooks and not search:
        narrow = False
    return narrow


def launch_sizes(counts, max_ch):
    """add_groups for the records the kernel takes: counts[e] positions in epoch e, split evenly over ceil(most / max_ch) launches;
    a launch is as large as its largest epoch.  A batch without any such record still has one (empty) launch."""
    most = max(counts)
    ng = 1 if most == 0 else (most + max_ch - 1) // max_ch
    sizes = [0] * ng
    for n in counts:
        per = (n + ng - 1) // ng
        k = 0
        for g in range(ng):
            m = max(0, min(n - k, per))
            sizes[g] = max(sizes[g], m)
            k += m
    return sizes


def family_of(nch, cboc=False, search=False, linear=True):
    """launch_synth_g_t's order: the CBOC instances by the flag; then the bisection ones, the wide ones for more than 12 positions,
    the linear carrier start where the plan's gate allows it, else the legacy start."""
    if cboc:
        return "cboc"
    if search:
        return "search"
    if nch > NARROW_MAX:
        return "wide"
    return "linear" if linear else "legacy"


def launches(counts, form, n_samp, cboc=False, search=False, linear=True, hooks=()):
    """[(family, NCH, ACC, MODE)] of one execute of a batch whose records are all fit for the kernel.  search, linear: what the plan's
    gates say (P.rw_search; g_lin, which GAL_G_LINEAR=0 of the hooks build turns off); the CBOC mode has neither."""
    assert form in MODES
    search = search and not cboc
    if "GAL_G_LINEAR=0" in hooks:
        linear = False
    linear = linear and not search and not cboc
    wide_ok = not cboc and not narrow_g(len(counts), n_samp, search, hooks)
    sizes = launch_sizes(counts, WIDE_MAX if wide_ok else NARROW_MAX)
    return [(family_of(nch, cboc, search, linear), nch, k > 0, form) for k, nch in enumerate(sizes)]


def compiled_set():
    """Every instance synth_group.hip instantiates: its launchers' switch statements over the channel count, ACC and the form."""
    out = set()
    for fam in FAMILIES:
        for nch in (WIDE_COUNTS if fam == "wide" else NARROW_COUNTS):
            for acc in (False, True):
                for mode in MODES:
                    out.add((fam, nch, acc, mode))
    return out


def reachable_set():
    """What a plan can launch: every family's settings with 1 .. MAX_CHAN positions in the largest epoch, every form."""
    settings = {"linear": {}, "legacy": {"linear": False}, "search": {"search": True}, "cboc": {"cboc": True},
                "wide": {"hooks": ("GAL_G_WIDE",)}, "wide_legacy": {"linear": False, "hooks": ("GAL_G_WIDE",)}}
    out = set()
    for kw in settings.values():
        for most in range(1, MAX_CHAN + 1):
            for mode in MODES:
                out.update(launches([most], mode, 2148, **kw))
    return out


def unreachable_set():
    return compiled_set() - reachable_set()


def per_family(instances):
    return {fam: sum(1 for i in instances if i[0] == fam) for fam in FAMILIES}
