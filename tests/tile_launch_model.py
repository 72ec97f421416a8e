"""The launches of the two passes that walk TILES of 1024 consecutive samples with a grid-stride loop and carry something from one trip of
that loop to the next (csrc/iq_osc.hip: galk_launch_iq_osc, k_osc_tilesum, k_osc_scan, k_iq_osc; csrc/iq_scint.hip:
galk_launch_iq_scint, k_iq_scint), restated -- TEST INFRASTRUCTURE: the product never imports this.

  oscillator     nt = ceil(n / 1024) tiles, grid = min(nt, 2048) blocks; block x takes the tiles x, x + grid, ... and alternates
                 between two LDS sets from trip to trip, so trip i + 2 writes the set that trip i read: a THIRD trip is the first that
                 reuses a set.  k_osc_scan is one block of 1024 lanes with c = ceil(nt / 1024) consecutive tiles per lane; its last
                 lane writes the state word of the call behind, from its own tiles where it has any.
  scintillation  blockIdx.y = the job; bx = min(nt of the longest job, 2048 / n_jobs) blocks walk a job's tiles.  Block x begins with
                 one 64-bit division, (j0, m0) = divmod(first + 1024 x, L), and steps from trip to trip by (sj, sm) = divmod(1024 bx, L)
                 with ONE conditional correction (m0 >= L: m0 -= L, j0 += 1); a tile needs nn = (m0 + 1023) div L + 2 nodes.

tests/test_iq_launch_geometry_cpu.py asserts what each named geometry below is for; tests/test_iq_osc_gpu.py and
tests/test_iq_scint_gpu.py run the kernels at them."""
import numpy as np

TILE, MAX_BLOCKS, SCAN_LANES = 1024, 2048, 1024  # kTile, kMaxBlocks of both .hip files; kScanThreads of iq_osc.hip
MAX_NODES = 18                                   # kMaxNodes of iq_scint.hip
MAX_JOBS = 64                                    # GAL_SCINT_MAX_JOBS


def osc_launch(n):
    """What a call of n >= 1 samples launches.  trips: of block 0 (the most); blocks_at_trips: how many blocks take that many;
    scan_lanes: the scan's lanes that hold a tile; last_lane_tiles: how many tiles the scan's lane 1023 holds (c: it is full)."""
    nt = -(-n // TILE)
    grid = min(nt, MAX_BLOCKS)
    trips = -(-nt // grid)
    c = -(-nt // SCAN_LANES)
    last = max(0, nt - (SCAN_LANES - 1) * c)
    return {"nt": nt, "grid": grid, "trips": trips, "min_trips": nt // grid, "blocks_at_trips": nt - (trips - 1) * grid, "c": c,
            "scan_lanes": -(-nt // c), "last_lane_tiles": last, "last_lane_full": last == c}


def scint_launch(max_n, n_jobs):
    """The grid of a call of n_jobs jobs whose longest has max_n samples: bx blocks per job."""
    assert 1 <= n_jobs <= MAX_JOBS
    nt = -(-max_n // TILE)
    return {"nt": nt, "bx": max(1, min(nt, MAX_BLOCKS // n_jobs)), "by": n_jobs}


def scint_trips(n, first, L, bx):
    """One job (n, first, L) on bx blocks: arrays [trip, block] of the kernel's (j0, m0, nn) as its recurrence produces them, of
    `fired` (the correction was taken on the step INTO that trip), of `live` (the block has a tile on that trip: everything else is
    meaningless where it is False) and of the direct values (dj, dm) = divmod(first + 1024 t, L) of the tile t = block + trip bx.
    The kernel holds m0, sm and the stride in 32 bits: that they fit is asserted here."""
    n, first, L, bx = int(n), int(first), int(L), int(bx)
    nt = -(-n // TILE)
    stride = bx * TILE
    sj, sm = divmod(stride, L)
    assert stride < 1 << 32 and L < 1 << 32
    trips = -(-nt // bx)
    x = np.arange(bx, dtype=np.int64)
    j0 = (first + x * TILE) // L
    m0 = first + x * TILE - j0 * L
    out = {k: np.zeros((trips, bx), dtype=np.int64) for k in ("j0", "m0", "nn", "dj", "dm")}
    out.update({k: np.zeros((trips, bx), dtype=bool) for k in ("fired", "live")})
    for i in range(trips):
        t = x + i * bx
        out["live"][i] = t < nt
        out["j0"][i], out["m0"][i], out["nn"][i] = j0, m0, (m0 + TILE - 1) // L + 2
        out["dj"][i], out["dm"][i] = (first + t * TILE) // L, (first + t * TILE) % L
        j0, m0 = j0 + sj, m0 + sm
        assert int(m0.max()) < 1 << 32
        fix = m0 >= L
        j0, m0 = j0 + fix, m0 - fix * L
        if i + 1 < trips:
            out["fired"][i + 1] = fix
    out.update(nt=nt, bx=bx, trips=trips, sj=sj, sm=sm)
    return out


T, B = TILE, MAX_BLOCKS

# name: (n, first_sample) of ONE gal_synth_iq_osc call
OSC_GEOMETRIES = {
    # 2 x 2048 + 4 tiles, the last of two samples: blocks 0 .. 3 take a third trip and reuse their first LDS set; a first sample that
    # is 1 mod 4 (two Philox blocks per lane) and beyond 2^33; the scan's lanes hold c = 5 tiles and the last 204 hold none
    "third_trip": ((2 * B + 3) * T + 2, 2 ** 40 + 1),
    # every block takes exactly three trips and every tile is whole; all 1024 lanes of the scan hold c = 6 tiles, so the state word
    # comes out of the last lane's own tiles; a first sample that is a multiple of four, as the CLI's batches are
    "full_scan": (3 * B * T, 2 ** 34 + 8),
}

_FILL = [(4, k, 64) for k in range(MAX_JOBS)]  # jobs of one vector: they only take their share of the grid
_LONG = 97 * T                                 # 3 x 32 + 1 tiles; the ragged ends below make it 98 tiles: blocks 0 and 1 take four trips


def _in_front_of_a_node(L, at_least, ahead):
    """The smallest first sample >= at_least that lies `ahead` samples in front of a node."""
    return -(-(at_least + ahead) // L) * L - ahead


# name: (n_jobs, [(n, first_sample, L)]): the jobs of ONE gal_synth_iq_scint call, the long ones last
SCINT_GEOMETRIES = {
    # 64 jobs -> 32 blocks each, a stride of 32768 samples; five long jobs of 98 tiles, three or four trips per block:
    #   L = 1025     just above a tile: tiles 49 and 50 lie between two nodes (nn = 2), every other has one inside (nn = 3);
    #                (sj, sm) = (31, 993), the correction fires on most steps and not on all
    #   L = 40000    above the stride: sj = 0; nodes at the job's samples 1001, 41001, 81001, each the second sample of a vector
    #   L = 162500   --scint at tau0 = 0.5 s: sj = 0; blocks 0 .. 16 add 32768 to m0 twice before the correction fires, the others fire
    #                at once and then not again; a first sample that is 3 mod 4; one node, at the job's sample 50001
    #   L = 2^24     the largest: r R comes to 2^32 - 256; first = k 2^24 - 5 beyond 2^40: block 0 alone has the job's one node, in its
    #                second vector, and its first step is the only one that fires
    #   L = 67       the case the suite had at two trips, now at four: nn = 17 or 18
    "node_lens_at_four_trips": (64, _FILL[:59] + [
        (_LONG + 1, _in_front_of_a_node(1025, 2 ** 33, 975), 1025),
        (_LONG + 2, _in_front_of_a_node(40000, 2 ** 36, 1001), 40000),
        (_LONG + 3, _in_front_of_a_node(162500, 2 ** 35, 50001), 162500),
        (_LONG + 5, (2 ** 16 + 3) * 2 ** 24 - 5, 2 ** 24),
        (_LONG + 1023, 2 ** 40 + 1, 67)]),
    # the default batch's split: 12 scintillating satellites -> 170 blocks each, a stride of 174080 samples against L = 162500:
    # (sj, sm) = (1, 11580); 2 x 170 + 5 tiles and three samples: blocks 0 .. 5 take a third trip, the last of them a partial tile;
    # every job at a first sample of its own, all four residues mod 4; job 0 lies so that the step INTO its third trips fires
    "cli_split": (12, [((2 * 170 + 5) * T + 3, 2 ** 33 + k * 2080000 + k if k else _in_front_of_a_node(162500, 2 ** 33, 21128), 162500)
                       for k in range(12)]),
    # B = 0 (one barrier fewer, no draws) at four trips beside 63 jobs that draw
    "b0_at_four_trips": (64, _FILL[:63] + [(_LONG + 2, 2 ** 40 + 3, 67)]),
}


def scint_geometry(name):
    """(launch, [scint_trips of every job]) of a named geometry."""
    n_jobs, jobs = SCINT_GEOMETRIES[name]
    assert len(jobs) == n_jobs
    la = scint_launch(max(n for n, _, _ in jobs), n_jobs)
    return la, [scint_trips(n, first, L, la["bx"]) for n, first, L in jobs]
