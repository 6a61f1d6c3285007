"""k_sorted_point_setup: what k_nn_search_sorted needs to know about a point (co_find, the centred coordinates, the seed and its
distance, the thresholds, the slot a lane takes as its point r) is worked out once per search and read back by every (split,
block) item as a record.  That may only change the SPEED: every answer must stay the oracle's brute force, bit for bit -- for
poses where both matrices matter, a target centred far from the origin, seeds that are rejected, missing (NaN, overflow) or left
behind by a large step, padding slots, every points-per-thread / tile size / queue / level-0v / order / first-search variant,
and the tile order an item derives from its block's home tile (splits of several tiles, homes inside and outside the split)."""
import numpy as np
import pytest

N_SRC = 6000                                             # not a multiple of 1024: padding slots, several source blocks
I_NAN, I_HUGE = 1234, 4321                               # the two points without a usable distance


def _rigid(rotvec, t):
    from object_alignment_amd import synth
    return synth.rigid4(synth.rotation_from_rotvec(rotvec), t)


_SCENES = {}


def _scene(orc, tail):
    """target (24 blocks of 256 along u around x = 1000, + 77 vertices when tail), source, the two poses of the align object,
    the base object's matrix, the make_pairs threshold and the oracle's answers at both poses -- computed once per variant"""
    if tail in _SCENES:
        return _SCENES[tail]
    rng = np.random.default_rng(1000 + int(tail))
    nt = 256 * 24 + (77 if tail else 0)
    i = np.arange(nt)
    u = 1000.0 + (i // 256) * 1.0 + (i % 256) * (0.5 / 256)      # slabs of 0.5 in u, 0.5 apart
    tgt = np.stack([u, rng.uniform(0, 8, size=nt), rng.normal(0, 0.05, size=nt)], axis=1).astype(np.float32)
    mxb = _rigid([0.2, -0.1, 0.3], [3.0, -2.0, 1.5])            # mx2: the base object, rotated and moved
    mxa = _rigid([-0.5, 0.8, 0.1], [-40.0, 25.0, 7.0])          # mx1: the align object
    # points next to target vertices in base-local space, carried to align-local space (float64, rounded once)
    q = tgt[rng.integers(0, nt, size=N_SRC)].astype(np.float64) + rng.normal(0, 0.02, size=(N_SRC, 3))
    to_align = np.linalg.inv(mxa.astype(np.float64)) @ mxb.astype(np.float64)
    src = (q @ to_align[:3, :3].T + to_align[:3, 3]).astype(np.float32)
    src[I_NAN, 1] = np.float32(np.nan)
    src[I_HUGE, 0] = np.float32(1e30)
    # the seeded search's pose: 0.8 along the base object's u -- most points end up nearer to the next slab than to their seed's
    step = mxb.astype(np.float64) @ _rigid([0.0, 0.0, 1e-5], [0.8, 0.03, 0.0]).astype(np.float64) @ np.linalg.inv(mxb.astype(np.float64))
    mxa2 = (step @ mxa.astype(np.float64)).astype(np.float32)
    imxb = orc.mat4_inverted(mxb)
    ref = []
    with np.errstate(all="ignore"):
        for m in (mxa, mxa2):
            w = np.array([orc.mat4_mul_vec3(imxb, orc.mat4_mul_vec3(m, p)) for p in src], np.float32)   # co_find
            ref.append(orc.nn_brute(w, tgt))
    d = np.sqrt(ref[0][1][np.isfinite(ref[0][1])].astype(np.float64))
    thresh = float(np.median(d))                                # about half of the slots keep no seed
    assert 0.3 < np.mean(ref[0][0] // 256 != ref[1][0] // 256)   # the step takes points out of their seed's slab
    _SCENES[tail] = (tgt, src, mxa, mxa2, mxb, thresh, ref)
    return _SCENES[tail]


# every value of every knob, not their product:  R, OA_NN_BIGTILE, OA_NN_PERSIST, OA_NN_VCHUNK, OA_NN_WAVE_ORDER, OA_NN_HOME_PASS,
# OA_NN_SPLITS (0: the library's own; 3: splits of several tiles, so that the visiting order has something to order), tail
VARIANTS = [
    (1, "0", "4", "1", "1", "1", 0, False),
    (2, "1", "0", "0", "0", "0", 0, True),
    (4, "0", "4", "1", "0", "0", 3, False),
    (4, "1", "4", "1", "1", "1", 0, True),
    (4, "1", "0", "0", "1", "1", 3, False),
    (4, "0", "0", "1", "1", "0", 0, True),
    (2, "0", "4", "0", "1", "1", 3, False),
    (1, "1", "0", "1", "0", "1", 2, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("R,bigtile,persist,vchunk,wave_order,home,splits,tail", VARIANTS)
def test_setup_records_give_the_oracles_answers(orc, R, bigtile, persist, vchunk, wave_order, home, splits, tail, monkeypatch):
    from object_alignment_amd.engine import IcpEngine
    monkeypatch.setenv("OA_NN_R", str(R))
    monkeypatch.setenv("OA_NN_BIGTILE", bigtile)
    monkeypatch.setenv("OA_NN_PERSIST", persist)
    monkeypatch.setenv("OA_NN_QUEUE_MIN_ITEMS", "0")
    monkeypatch.setenv("OA_NN_VCHUNK", vchunk)
    monkeypatch.setenv("OA_NN_WAVE_ORDER", wave_order)
    monkeypatch.setenv("OA_NN_HOME_PASS", home)
    if splits:
        monkeypatch.setenv("OA_NN_SPLITS", str(splits))
    tgt, src, mxa, mxa2, mxb, thresh, ref = _scene(orc, tail)
    with IcpEngine(0) as e:
        e.set_search_mode("brute")
        e.set_target(tgt)
        e.set_source(src)
        e.set_matrices(mxa, mxb)
        idx, d2, _ = e.nn_search()                      # unseeded
        assert e.stat("brute_kernel") == 3.0
        A, _, _ = e.make_pairs(thresh)                  # winner records = seeds, for the slots that pass
        e.set_matrices(mxa2, mxb)
        idx2, d22, _ = e.nn_search()                    # seeded, after a large step
    assert 0.25 * N_SRC < A.shape[1] < 0.75 * N_SRC     # some slots have a seed, some were rejected
    (r1, rd1), (r2, rd2) = ref
    assert np.array_equal(idx, r1) and np.array_equal(d2, rd1, equal_nan=True)
    assert np.array_equal(idx2, r2) and np.array_equal(d22, rd2, equal_nan=True)


@pytest.mark.gpu
def test_short_loop_is_the_oracles_and_the_same_without_the_queue(orc, monkeypatch):
    """6 iterations of 20k <-> 20k brute force: pairs per iteration exact, every step's matrix within 1e-9 of the oracle's loop,
    and the final matrix bitwise the same with one workgroup per item (OA_NN_PERSIST=0)."""
    from object_alignment_amd import synth
    from object_alignment_amd.engine import IcpEngine
    src, tgt, mxa, mxb = synth.c3_random_pair(20000)[:4]
    ref = orc.icp_run(src, tgt, mxa, mxb, iters=6, sample=1, thresh=0.5, target_d=1e-300, use_target=True, kd=orc.KDTree(tgt))
    out = {}
    for persist in ("4", "0"):
        monkeypatch.setenv("OA_NN_PERSIST", persist)
        monkeypatch.setenv("OA_NN_QUEUE_MIN_ITEMS", "0")
        with IcpEngine(0) as e:
            e.set_search_mode("brute")
            e.set_target(tgt)
            e.set_source(src, stride=1)
            e.set_matrices(mxa, mxb)
            out[persist] = e.run(iters=6, thresh=0.5, target_d=0.01, use_target=True, early_exit=False)
            assert e.stat("brute_kernel") == 3.0
    res = out["4"]
    assert res.iters_done == 6 == ref["iters_done"]
    assert np.array_equal(res.step_K, ref["step_K"])
    assert np.abs(res.step_M - ref["step_M"]).max() < 1e-9
    assert np.array_equal(res.matrix_world, out["0"].matrix_world)
