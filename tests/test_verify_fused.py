"""k_verify: ONE verification launch for both chains (synth_kernels.hip).  The grid's index arithmetic on the CPU (the library's own,
galk_verify_position = the function the kernel calls), clean runs, the execution modes and perturbed checkpoints on the GPU.
(The walk's body is unchanged, so its own tests stand: checkpoints and end states bitwise against brute-force stepping in
tests/test_walker_cpu.py; the stitch's look-back over 1 .. many blocks, GAL_SCAN_BLOCK_LEGS, in the GAL_SCAN_BLOCK_LEGS cases of tests/test_parity_gpu.py.)"""
import ctypes

import numpy as np
import pytest

N, RATE = 260000, 2.6e6
E, S, NCH = 5, 16, 12
GATE_LO = 2.0 ** -40            # k_synth_g's gate on the carrier step, cycles per sample (synth_api.cpp)
GATE_HI = 120.0 / (16.0 * 511.0)


def _position(lib, t, e, s, w, wc, mod, rem):
    out = [ctypes.c_int(-1) for _ in range(4)]
    rc = lib.galk_verify_position(t, e, s, w, wc, mod, rem, *[ctypes.byref(o) for o in out])
    return rc, tuple(o.value for o in out)


@pytest.mark.parametrize("w,wc", [(8, 4), (32, 16)])
def test_rotation_visits_every_position_exactly_once(pkg, w, wc):
    """Sampled mode: over 8 consecutive batches (ver_rem = 0 .. 7) every (slot, epoch, leg) of both chains is re-walked exactly once;
    default mode (ver_mod = 1): every one in every batch.  The carrier threads come first, in whole waves: no wave holds both bodies."""
    lib = pkg.synth.load_library()
    lib.galk_verify_position.argtypes = [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_int)] * 4
    want = {(0, s, e, k) for s in range(S) for e in range(E) for k in range(w)} | {(1, s, e, k) for s in range(S) for e in range(E) for k in range(wc)}
    for mod, rems in ((8, range(8)), (1, (0,))):
        seen = {}
        for rem in rems:
            t, chains = 0, []
            while True:
                rc, pos = _position(lib, t, E, S, w, wc, mod, rem)
                if rc < 0:
                    break
                chains.append(pos[0] if rc == 0 else None)
                if rc == 0:
                    seen[pos] = seen.get(pos, 0) + 1
                t += 1
            assert t >= E * S * wc and t < 2 * (E * S * (w + wc)) + 512
            # the code part is the last E * S * wc threads of the grid; the carrier part in front of it is whole blocks
            nc = t - E * S * wc
            assert nc > 0 and nc % 256 == 0
            assert all(c != 1 for c in chains[:nc]) and all(c != 0 for c in chains[nc:])
            for g in range(0, t, 64):
                assert len({c for c in chains[g:g + 64] if c is not None}) <= 1
        assert set(seen) == want and set(seen.values()) == {1}, mod


@pytest.fixture(scope="module")
def batch(pkg):
    """5 epochs x 16 slots, 12 active; carrier steps: 0, +-2^-40 (the gate's edge), a sign change between consecutive epochs, the gate's
    maximum 120 / (16 x 511); the other channels as the synthetic workload draws them.  The oracle's samples, computed once."""
    from oracle_binding import oracle_run

    p = pkg.workloads.make_synthetic(n_epochs=E, n_chan=NCH, n_slots=S, samples_per_epoch=N, seed=4711)
    fc = p["f_carr"]
    fc[:, 0] = 0.0
    fc[:, 1] = GATE_LO * RATE * (1 + 1e-12)
    fc[:, 2] = -GATE_LO * RATE * (1 + 1e-12)
    fc[:, 3] = np.array([420.0, -420.0, 419.5, -0.25, 0.25])
    fc[:, 4] = GATE_HI * RATE * (1 - 1e-12)
    fc[:, 5] = -GATE_HI * RATE * (1 - 1e-12)
    ref_iq, ref_st = oracle_run(p, N, RATE)
    ref_iq.setflags(write=False)
    return p, ref_iq, ref_st


def _engine(pkg, flags):
    return pkg.SynthEngine(samples_per_epoch=N, n_slots=S, device=0, test_hooks=True, flags=flags)


@pytest.mark.gpu
@pytest.mark.parametrize("legs", ["8", "32"])
@pytest.mark.parametrize("sampled", [False, True])
def test_clean_run_counts_no_mismatch(pkg, batch, monkeypatch, legs, sampled):
    """A clean batch: 0 mismatches, no fallback, oracle-equal samples -- every leg of both chains (default) and the sampled rotation."""
    p, ref_iq, ref_st = batch
    monkeypatch.setenv("GAL_WALK_LEGS", legs)  # (GAL_TEST_HOOKS build)
    with _engine(pkg, pkg.synth.GAL_CFG_VERIFY_SAMPLED if sampled else 0) as eng:
        for _ in range(2 if sampled else 1):
            iq, st, stats = eng.run_host(p)
            assert stats["chain_mismatch"] == 0 and eng.walk_counts()[2] == 0
            assert stats["kernel_family"] == 1  # the batch runs k_synth_g, the family k_verify belongs to
            assert np.array_equal(iq, ref_iq)
    act = ref_st["prn"] > 0
    assert np.array_equal(st["carr_phase"][act].view(np.uint64), ref_st["carr_phase"][act].view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("first,count", [(2, 3), (4, 1)])
def test_executed_range_skips_the_prefix(pkg, batch, first, count):
    """gal_synth_execute_range with e_first > 0: the epochs in front carry no checkpoints (cp_e0 > 0) and both parts of k_verify skip
    their legs; the range comes out oracle-equal with 0 mismatches."""
    import torch

    p, ref_iq, _ = batch
    out = torch.empty(count * N * 2, dtype=torch.int16, device="cuda")
    with _engine(pkg, 0) as eng:
        eng.plan(p)
        eng.execute(out.data_ptr(), first, count)
        _, stats = eng.finish()
        assert stats["chain_mismatch"] == 0 and eng.walk_counts()[2] == 0
    assert np.array_equal(out.cpu().numpy(), ref_iq[first * N * 2:(first + count) * N * 2])


@pytest.mark.gpu
def test_single_epoch_call(pkg, batch):
    """One epoch per call (INTEGRATION.md option B), the state carried from call to call: k_verify on the smallest grid."""
    p, ref_iq, _ = batch
    state = None
    with _engine(pkg, 0) as eng:
        for e in range(3):
            iq, state, stats = eng.run_host(p[e:e + 1], state_in=state)
            assert stats["chain_mismatch"] == 0 and eng.walk_counts()[2] == 0
            assert np.array_equal(iq, ref_iq[e * N * 2:(e + 1) * N * 2]), e


# ---- perturbed checkpoints.  The batch above at its plan's geometry: 1024-sample chunks, 254 per epoch + the end state (CP1 = 255), 32
# carrier legs of 8 chunks, 16 code legs of 16 chunks; the word perturbed belongs to (slot 7, epoch 2), an ordinary channel.
CP1, LC, LKC, NCHUNKS = 255, 8, 16, 254
PS, PE = 7, 2
BASE = (PE * S + PS) * CP1
# what (0 cp_p one ulp, 1 cp_x one ulp, 2 cp_ib ^= bits, 3 flip_in ^= 1), index, bits, mismatches.  The counts are what the PARENT's two
# kernels (k_verify_carr + k_verify_code, over every leg) count for the same perturbation of the same batch, recorded from a run of the
# parent commit with the same hook; where a single comparison is hit, reasoning gives the same 1: a leg is re-walked from its own FIRST
# checkpoint, so a word inside a leg fails its own comparison and nothing else; a leg's first word fails the hand-over of the leg in
# front and then every comparison of its own leg that the moved start reaches -- all 16 of a code leg whose symbol counter is off by one
# (17; leg 0 has the host-given start in the hand-over's place: 17 again), none of a carrier leg moved by one ulp of a low binade, which
# the first rounded add into the next binade absorbs (1).
PERTURBATIONS = {
    "carr_mid": (0, BASE + 3 * LC + 3, 0, 1),
    "carr_leg_first": (0, BASE + 3 * LC, 0, 1),
    "code_x_mid": (1, BASE + 2 * LKC + 5, 0, 1),
    "code_ib_mid": (2, BASE + 2 * LKC + 5, 1, 1),
    "code_ib_leg_first": (2, BASE + 2 * LKC, 1, 17),
    "code_ib_epoch_start": (2, BASE, 1, 17),       # leg 0: the host-given x0 / ib0 as well
    "code_flag_epoch_end": (2, BASE + NCHUNKS, 0x10000, 1),  # the end-of-epoch state's flip flag
    "flip_in": (3, PE * S + PS, 0, 1),                            # what k_pages reads
}


@pytest.mark.gpu
def test_perturbed_checkpoint_is_counted_like_the_two_kernels_did(pkg, batch):
    """One word of a finished batch's checkpoint arrays perturbed, the verifier launched on the batch's own plan (hooks build:
    gal_synth_test_verify_count), the word put back: exactly the parent's counts, a count and never a fault; the handle is intact after."""
    p, ref_iq, _ = batch
    with _engine(pkg, 0) as eng:
        iq, _, stats = eng.run_host(p)
        assert stats["chain_mismatch"] == 0 and stats["chunk_samples"] == 1024 and stats["chunks_per_epoch"] == NCHUNKS
        fn = eng._lib.gal_synth_test_verify_count
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_uint, ctypes.POINTER(ctypes.c_int)]
        got = {}
        for name, (what, idx, bits, _) in PERTURBATIONS.items():
            c = ctypes.c_int(-1)
            assert fn(eng._h, what, idx, bits, ctypes.byref(c)) == 0, name
            got[name] = c.value
        print("mismatches counted:", got)
        assert got == {k: v[3] for k, v in PERTURBATIONS.items()}
        c = ctypes.c_int(-1)
        assert fn(eng._h, 0, E * S * CP1, 0, ctypes.byref(c)) != 0  # an index outside the arrays is refused, nothing is launched
        iq2, _, stats2 = eng.run_host(p)
        assert stats2["chain_mismatch"] == 0 and eng.walk_counts()[2] == 0 and np.array_equal(iq2, ref_iq)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["carr_mid", "code_ib_mid"])
def test_perturbation_in_a_live_batch_ends_in_the_all_walked_fallback(pkg, batch, monkeypatch, name):
    """The same perturbation written between the stitch and the verifier of a batch in flight (GAL_VERIFY_POKE, hooks build): the
    mismatch sends gal_synth_finish into the all-walked fallback, which delivers oracle-equal samples and an exact end state."""
    p, ref_iq, ref_st = batch
    what, idx, bits, _ = PERTURBATIONS[name]
    monkeypatch.setenv("GAL_VERIFY_POKE", "%d,%d,%d" % (what, idx, bits))
    with _engine(pkg, 0) as eng:
        iq, st, stats = eng.run_host(p)
        assert eng.walk_counts()[2] == 1 and stats["chain_mismatch"] == 0 and stats["synth_runs"] == 2
    assert np.array_equal(iq, ref_iq)
    act = ref_st["prn"] > 0
    assert np.array_equal(st["carr_phase"][act].view(np.uint64), ref_st["carr_phase"][act].view(np.uint64))
