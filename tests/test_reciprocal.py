"""Reciprocal correspondences (oa_set_reciprocal, IcpSettings.reciprocal): keep a pair only if it is mutual.

The rule (include/oa_icp.h): with b the float32 point make_pairs emits in B and p_k the selected source points, the pair of slot i
is kept iff d2(b, p_i) <= r2 * min_k d2(b, p_k), d2 = the project's fp32 metric, r2 = float32(ratio^2), one fp32 multiply.

The numpy reference lives here, on top of what is already there: test_plane_metric.ref_pairs gives the pairs and B;
orc.nn_brute(B32, src_sel) gives m -- the oracle's metric, which the engine's searches match bit for bit --;
orc.nn_brute(B32[k:k+1], p_i) gives d2(b, p_i); the fp32 comparison of the definition closes it.  The steps' solves are
test_robust_weights.ref_step's (weighted Kabsch / weighted plane solve with loss "none" = every weight one).
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from object_alignment_amd import synth
from test_plane_metric import TOL, ref_pairs, scaled_base, selection
from test_robust_weights import ref_step as solve_step, world_scale

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROTVEC, SHIFT = (0.10, -0.07, 0.12), (0.05, -0.03, 0.02)      # the usual test pose
THRESH = 0.5


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build_hip()
    return g


# ------------------------------------------------------------------------------------------------ the cases
def usual_pose():
    P = synth.rigid4(synth.rotation_from_rotvec(list(ROTVEC)), list(SHIFT), dtype=np.float64)
    return np.linalg.inv(P).astype(np.float32), np.eye(4, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def upper_half():
    """bunny_surface(4000, 0.0)[z > 0]: the partial scan (2000 points)"""
    t = np.asarray(synth.bunny_surface(4000, 0.0), np.float32)
    return np.ascontiguousarray(t[t[:, 2] > 0])


def whole(n=3000):
    return np.asarray(synth.bunny_surface(n, 0.5), np.float32)


# ------------------------------------------------------------------------------------------------ the reference
def recip_keep(orc, A, B, src_sel, ratio=1.0):
    """The definition over the pairs ref_pairs returned (A: their source points, B: their b, both float32 values in fp64) against
    the selection src_sel: the mask of the pairs that stay."""
    if len(A) == 0:
        return np.zeros(0, bool)
    A32, B32, sel32 = np.asarray(A, np.float32), np.asarray(B, np.float32), np.asarray(src_sel, np.float32)
    _, m = orc.nn_brute(B32, sel32)
    own = np.array([orc.nn_brute(B32[k:k + 1], A32[k:k + 1])[1][0] for k in range(len(A32))], np.float32)
    assert np.all(m <= own)                                    # p_i is one of the candidates
    r2 = np.float32(ratio * ratio)
    return own <= r2 * m                                       # one fp32 multiply, fp32 comparison


def recip_pairs(orc, src_sel, mx1, mx2, tgt, ratio=1.0, counts=None, **kw):
    """ref_pairs, then the reciprocal rule.  counts (a list): gets (plain K, kept K)."""
    if kw.get("tris") is None and kw.get("tgt_normals") is None:
        kw["tgt_normals"] = np.ones((len(tgt), 3), np.float32)          # (only the plane metric reads them)
    A, B, N, D = ref_pairs(orc, src_sel, mx1, mx2, tgt, **kw)
    keep = recip_keep(orc, A, B, src_sel, ratio)
    if counts is not None:
        counts.append((len(A), int(keep.sum())))
    return A[keep], B[keep], N[keep], D[keep]


def _kabsch(a, b):
    ca, cb = a.mean(0), b.mean(0)
    u, _, vh = np.linalg.svd((b - cb).T @ (a - ca))
    R = u @ vh
    if np.linalg.det(R) < 0.0:
        R = R - np.outer(u[:, 2], vh[2] * 2.0)
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = cb - R @ ca
    return M


@functools.lru_cache(maxsize=None)
def numpy_loop(reciprocal, iters=60):
    """The issue's measurement: plain numpy, fp64, a KD-tree, `iters` point-metric steps of the whole source onto the upper half
    from the test pose, mx_base = I.  Returns (pairs in the first step, translation error, rotation error in degrees): the true
    pose brings matrix_world to the identity, so what is left of it is the error."""
    from oracle import oracle as orc
    orc.build()
    src, tgt = whole().astype(np.float64), upper_half().astype(np.float64)
    kt, ks = orc.KDTree(tgt), orc.KDTree(src)
    M = usual_pose()[0].astype(np.float64)
    first = None
    for _ in range(iters):
        w = src @ M[:3, :3].T + M[:3, 3]
        q = tgt[kt.query(w)[0]]
        keep = np.linalg.norm(w - q, axis=1) < THRESH
        Mi = np.linalg.inv(M)
        b = q @ Mi[:3, :3].T + Mi[:3, 3]
        if reciprocal:
            j = ks.query(b)[0]
            keep &= ((b - src) ** 2).sum(1) <= ((b - src[j]) ** 2).sum(1) * (1.0 + 1e-9)
        if first is None:
            first = int(keep.sum())
        M = M @ _kabsch(src[keep], b[keep])
    ang = np.degrees(np.arccos(np.clip((np.trace(M[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))
    return first, float(np.linalg.norm(M[:3, 3])), float(ang)


def translation_error(matrix_world):
    return float(np.linalg.norm(np.asarray(matrix_world, np.float64)[:3, 3]))


# ------------------------------------------------------------------------------------------------ CPU
def test_reciprocal_abi_and_bindings(built):
    """Fails without the feature: the header, the library, the bindings, the settings and the add-on all name the check."""
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators import icp_align
    from object_alignment_amd.operators.icp_align import IcpSettings, reciprocal_of
    hdr = open(os.path.join(ROOT, "include", "oa_icp.h")).read()
    assert re.search(r"\bint\s+oa_set_reciprocal\s*\(\s*oa_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*,\s*double\s+\w+\s*\)", hdr)
    assert "oa_set_reciprocal" in _capi.SYMBOLS
    for name, val in (("OA_STAT_RECIPROCAL", 37), ("OA_STAT_RECIPROCAL_RATIO", 38), ("OA_STAT_RECIP_REJECTED", 39)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name
        assert getattr(_capi, name) == val
    for lib in ("liboa_icp.so", "liboa_icp_exp.so"):
        assert hasattr(C.CDLL(os.path.join(ROOT, "object_alignment_amd", lib)), "oa_set_reciprocal"), lib
    assert _capi.load().oa_set_reciprocal.argtypes == [C.c_void_p, C.c_int, C.c_double]
    assert callable(IcpEngine.set_reciprocal)
    assert (IcpEngine.STATS["reciprocal"], IcpEngine.STATS["reciprocal_ratio"], IcpEngine.STATS["recip_rejected"]) == (37, 38, 39)
    s = IcpSettings()
    assert s.reciprocal is False and s.reciprocal_ratio == 1.0
    assert reciprocal_of(s) == (False, 1.0)
    assert reciprocal_of(IcpSettings(reciprocal=True, reciprocal_ratio=1.5)) == (True, 1.5)

    class Prefs:                                                  # the registered add-on preferences' names
        icp_reciprocal, icp_reciprocal_ratio = True, 2.0
    assert reciprocal_of(Prefs()) == (True, 2.0)
    assert reciprocal_of(object()) == (False, 1.0)
    addon = open(os.path.join(ROOT, "object_alignment_amd", "blender_addon.py")).read()
    assert re.search(r"icp_reciprocal\s*:\s*BoolProperty", addon) and re.search(r"icp_reciprocal_ratio\s*:\s*FloatProperty", addon)
    assert callable(icp_align.apply_reciprocal)


def test_apply_reciprocal_hands_the_setting_over_every_time():
    from object_alignment_amd.operators.icp_align import IcpSettings, apply_reciprocal

    class E:
        def __init__(self):
            self.calls = []

        def set_reciprocal(self, on, ratio):
            self.calls.append((on, ratio))
    e = E()
    apply_reciprocal(e, IcpSettings(reciprocal=True, reciprocal_ratio=1.25))
    apply_reciprocal(e, IcpSettings())
    assert e.calls == [(True, 1.25), (False, 1.0)]                # off is handed over too: the engine is shared
    apply_reciprocal(object(), IcpSettings())                     # an engine without the setter counts as check-off
    with pytest.raises(RuntimeError):
        apply_reciprocal(object(), IcpSettings(reciprocal=True))


def test_reference_shows_the_effect():
    """The yardstick itself (passes without the feature): on the whole source against the upper half the numpy loop with the
    check ends with a translation error at most a quarter of the plain loop's (observed 0.0052 against 0.182), and its first
    step keeps between 20 % and 80 % of the plain pairs (observed 1264 of 2153) -- or the case does not count."""
    k0, te0, ang0 = numpy_loop(False)
    k1, te1, ang1 = numpy_loop(True)
    print("plain: %d pairs, ends at %.3g deg, translation error %.4g; reciprocal: %d pairs, %.3g deg, %.4g" % (k0, ang0, te0, k1, ang1, te1))
    assert te1 <= 0.25 * te0
    assert 0.2 * k0 <= k1 <= 0.8 * k0


def test_reference_rule_on_a_handful_of_points(orc):
    """recip_keep on a case small enough to see: two source points, three correspondences."""
    sel = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    A = sel[[0, 0, 1]].astype(np.float64)
    B = np.array([[0.4, 0, 0], [0.5, 0, 0], [0.75, 0, 0]], np.float64)   # nearer to its own point; a tie; nearer to its own point
    assert recip_keep(orc, A, B, sel).tolist() == [True, True, True]
    A = sel[[0, 1]].astype(np.float64)
    B = np.array([[0.75, 0, 0], [0.25, 0, 0]], np.float64)               # each nearer to the OTHER point: 0.5625 against 0.0625
    assert recip_keep(orc, A, B, sel).tolist() == [False, False]
    assert recip_keep(orc, A, B, sel, ratio=2.9).tolist() == [False, False]     # 8.41 x 0.0625 < 0.5625
    assert recip_keep(orc, A, B, sel, ratio=3.0).tolist() == [True, True]       # 9 x 0.0625 = 0.5625: a tie is kept


# ------------------------------------------------------------------------------------------------ GPU
def pairs_case(name):
    """(src, vlist, stride, target, tris, mx_align, mx_base, ratio) of a make_pairs case"""
    mxa, mxb = usual_pose()
    src, vlist, stride, tgt, tris, ratio = None, None, 1, upper_half(), None, 1.0
    if name.startswith("n"):
        src = whole(int(name[1:]))
    elif name == "vlist_stride2":
        src = whole(4097)
        vlist, stride = np.arange(len(src) - 1, -1, -1, dtype=np.int64)[:3000], 2
    elif name == "scaled_base":
        src = whole(1000)
        B = scaled_base()
        mxa, mxb = (B @ mxa.astype(np.float64)).astype(np.float32), B.astype(np.float32)
    elif name == "ratio_1_5":
        src, ratio = whole(1000), 1.5
    elif name == "source_is_target":
        src = tgt = np.asarray(synth.bunny_surface(1000, 0.0), np.float32)
        mxa = np.eye(4, dtype=np.float32)
    elif name == "duplicated":
        s = whole(1000)
        src = np.ascontiguousarray(np.concatenate([s, s]))
    elif name == "mesh":
        src = whole(1000)
        tgt, tris = synth.cubed_surface_mesh(40)
    else:
        raise ValueError(name)
    return src, vlist, stride, np.asarray(tgt, np.float32), tris, mxa, mxb, ratio


PAIRS_CASES = ["n1", "n63", "n64", "n65", "n4097", "vlist_stride2", "scaled_base", "ratio_1_5", "source_is_target", "duplicated", "mesh"]
# (kept, plain) of the five sizes, as counted in numpy when the check was specified
SIZE_COUNTS = {"n1": (1, 1), "n63": (38, 45), "n64": (39, 46), "n65": (39, 48), "n4097": (1501, 2939)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", PAIRS_CASES)
def test_gpu_make_pairs_bit_for_bit(orc, name):
    """With the check on, make_pairs returns exactly the reference's A and B -- same K, same order, same bits -- and
    OA_STAT_RECIP_REJECTED the reference's count.  Sizes 1, 63, 64, 65, 4097: one leaf, the leaf boundary, three tree levels."""
    from object_alignment_amd.engine import IcpEngine
    src, vlist, stride, tgt, tris, mxa, mxb, ratio = pairs_case(name)
    sel = np.asarray(src, np.float32)[selection(len(src), vlist, stride)]
    counts = []
    A, B, _, _ = recip_pairs(orc, sel, mxa, mxb, tgt, ratio=ratio, counts=counts, tris=tris, thresh=THRESH)
    plain, kept = counts[0]
    print("%s: kept %d of %d pairs (%d selected points)" % (name, kept, plain, len(sel)))
    if name in SIZE_COUNTS:
        assert (kept, plain) == SIZE_COUNTS[name]
    if name != "n1" and name != "source_is_target":
        assert 0 < kept < plain                                    # both verdicts
    if name == "source_is_target":
        assert kept == plain == len(sel)                           # d2 = 0 everywhere: ties, all kept
    if name == "duplicated":
        assert kept % 2 == 0 and np.array_equal(A[:kept // 2], A[kept // 2:])   # equal points tie: both copies stay, or neither
    with IcpEngine(0) as e:
        if tris is not None:
            e.set_target_mesh(tgt, tris)
        else:
            e.set_target(tgt)
        e.set_source(src, vlist=vlist, stride=stride)
        e.set_matrices(mxa, mxb)
        A0, _, _ = e.make_pairs(THRESH)
        assert e.stat("recip_rejected") == 0.0 and e.stat("reciprocal") == 0.0
        e.set_reciprocal(True, ratio)
        assert e.stat("reciprocal") == 1.0 and e.stat("reciprocal_ratio") == ratio
        for _ in range(2):                                         # (the second call finds the tree built)
            Ae, Be, _ = e.make_pairs(THRESH)
            assert Ae.shape == (3, kept) and A0.shape == (3, plain)
            assert np.array_equal(Ae.T, A) and np.array_equal(Be.T, B)
            assert e.stat("recip_rejected") == float(plain - kept)
        _, _, ds = e.make_pairs(THRESH, calc_stats=True)            # (two passes: the check runs in both)
        assert e.stat("recip_rejected") == float(plain - kept)
        e.set_reciprocal(False)
        A1, _, _ = e.make_pairs(THRESH)
        assert np.array_equal(A1, A0) and e.stat("recip_rejected") == 0.0


def step_parity(orc, eng, metric, loss, c, src_sel, mxa, mxb, tgt, steps, **kw):
    """test_plane_metric.step_parity's discipline with the reciprocal pairs: before every step the engine's matrix_world goes to
    the reference; K exact, M within TOL -- where the reference's forward and reversed pair order agree to that tolerance."""
    s_world = world_scale(mxa)
    rejected = 0
    for it in range(steps):
        mw = eng.matrix_world()
        counts = []
        ref = solve_step(orc, metric, loss, c, src_sel, None, mw, mxb, tgt, s_world=s_world,
                         pairs=functools.partial(recip_pairs, counts=counts), **kw)
        assert np.max(np.abs(ref["M"] - ref["M_rev"])) < TOL, "the case is ill-conditioned for the reference itself"
        M, st = eng.iterate(thresh=kw.get("thresh", THRESH), target_d=1e-4)
        dM = float(np.max(np.abs(M - ref["M"])))
        print("step %d: K %d / %d (of %d plain), |dM| %.3g, d mean %.3g" % (it, st["K"], ref["K"], counts[0][0], dM, abs(st["mean_dist"] - ref["mean"])))
        assert st["K"] == ref["K"]
        assert dM <= TOL
        assert abs(st["mean_dist"] - ref["mean"]) <= TOL and abs(st["std_dist"] - ref["std"]) <= TOL
        rejected += counts[0][0] - counts[0][1]
    assert rejected > 0                                            # the check had something to say


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["point", "plane_mesh", "tukey"])
def test_gpu_step_parity(orc, case):
    from object_alignment_amd.engine import IcpEngine
    mxa, mxb = usual_pose()
    src = whole(3000)
    with IcpEngine(0) as e:
        e.set_reciprocal(True)
        kw = dict(thresh=THRESH)
        metric, loss, c = "point", "none", 0.0
        if case == "plane_mesh":
            tgt, tris = synth.cubed_surface_mesh(40)
            e.set_target_mesh(tgt, tris)
            e.set_metric("plane")
            kw.update(tris=tris)
            metric = "plane"
        else:
            tgt = upper_half()
            e.set_target(tgt)
        if case == "tukey":
            loss, c = "tukey", 0.05
            e.set_robust(loss, c)
        e.set_source(src, stride=1)
        e.set_matrices(mxa, mxb)
        assert e.stat("reciprocal") == 1.0                          # survives the uploads and set_matrices
        step_parity(orc, e, metric, loss, c, src, mxa, mxb, np.asarray(tgt, np.float32), 6, **kw)


@pytest.mark.gpu
def test_gpu_search_modes_agree_bitwise():
    from object_alignment_amd.engine import IcpEngine
    mxa, mxb = usual_pose()
    src, tgt = whole(3000), upper_half()
    hist = {}
    for mode in ("brute", "grid", "bvh", "auto", "auto"):
        with IcpEngine(0) as e:
            e.set_reciprocal(True)
            e.set_search_mode(mode)
            e.set_target(tgt)
            e.set_source(src, stride=1)
            e.set_matrices(mxa, mxb)
            r = e.run(iters=10, thresh=THRESH, target_d=1e-4, early_exit=False)
            assert e.stat("recip_rejected") > 0.0
        assert r.iters_done == 10
        hist.setdefault(mode, []).append((r.step_M.copy(), r.step_new.copy(), r.step_K.copy(), r.step_stats.copy(), r.matrix_world.copy()))
    first = hist["brute"][0]
    for mode, runs in hist.items():
        for run in runs:
            for x, y in zip(first, run):
                assert np.array_equal(x, y), mode


@pytest.mark.gpu
def test_gpu_behaviour_whole_model_onto_half_scan():
    """IcpAlign.run, 60 iterations: with reciprocal=True the loop ends within 1.5 x the numpy reference loop's translation error
    (+ 1e-4: near-tie flips between the fp64 KD-tree loop and the float32 engine move the end point slightly), and at most a
    quarter of the engine's own plain loop's."""
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings
    mxa, mxb = usual_pose()
    src, tgt = whole(3000), upper_half()
    _, te_ref, _ = numpy_loop(True)
    te = {}
    with IcpEngine(0) as e:
        for on in (True, False):
            st = IcpSettings(icp_iterations=60, sample_fraction=1, min_start=THRESH, reciprocal=on)
            r = IcpAlign(st, engine=e).run(src, tgt, mxa, mxb, early_exit=False)
            assert r.iters_done == 60 and e.stat("reciprocal") == (1.0 if on else 0.0)
            te[on] = translation_error(r.matrix_world)
    print("translation error: engine reciprocal %.4g (numpy %.4g), engine plain %.4g" % (te[True], te_ref, te[False]))
    assert te[True] <= 1.5 * te_ref + 1e-4
    assert te[True] <= 0.25 * te[False]


def _history(e, src, tgt, mxa, mxb, iters=15):
    e.set_search_mode("grid")
    e.set_target(tgt)
    e.set_source(src, stride=1)
    e.set_matrices(mxa, mxb)
    r = e.run(iters=iters, thresh=THRESH, target_d=0.01, early_exit=False)
    return r, e.stat("fast_iterations")


@pytest.mark.gpu
def test_gpu_off_means_off():
    """A context that ran with the check and then switches it off produces, over 15 iterations, bitwise the history of a fresh
    context (the fused path in both); nn_search, deviation and coarse_align do not look at the setting at all."""
    from object_alignment_amd.engine import IcpEngine
    src, tgt, mxa, mxb = synth.c2_bunny_pair(100000)
    with IcpEngine(0) as e:
        plain, fast0 = _history(e, src, tgt, mxa, mxb)
    with IcpEngine(0) as e:
        e.set_reciprocal(True)
        visited, fast_on = _history(e, src, tgt, mxa, mxb, iters=3)
        assert fast_on == 0 and e.stat("recip_rejected") > 0.0       # search -> check -> accumulate: never the fused path
        e.set_reciprocal(False)
        back, fast1 = _history(e, src, tgt, mxa, mxb)
    assert fast0 > 0 and fast1 > 0
    for name in ("step_M", "step_new", "step_K", "step_stats", "step_trans", "matrix_world"):
        assert np.array_equal(getattr(plain, name), getattr(back, name)), name

    mxa, mxb = usual_pose()
    src, tgt = whole(3000), upper_half()
    out = {}
    with IcpEngine(0) as e:
        e.set_target(tgt)
        e.set_target_normals(np.asarray(tgt, np.float32) / np.linalg.norm(tgt, axis=1, keepdims=True).astype(np.float32))
        e.set_source(src, stride=1)
        for on in (False, True):
            e.set_reciprocal(on)
            e.set_matrices(mxa, mxb)
            idx, d2, _ = e.nn_search()
            dev = e.deviation(thresh=THRESH, outputs=("signed_d", "dist", "closest", "idx", "feature"))
            e.set_matrices(mxa, mxb)
            scores = e.score_poses(np.stack([mxa, np.eye(4, dtype=np.float32)]), THRESH)
            co = e.coarse_align(THRESH, n_rot=32, n_refine=4, refine_iters=5, stride=2)
            out[on] = (idx, d2, dev, scores, co)
    a, b = out[False], out[True]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    for k in ("signed_d", "dist", "closest", "idx", "feature"):
        assert np.array_equal(a[2][k], b[2][k], equal_nan=True), k
    for k, v in a[2]["report"].items():
        if not k.endswith("_ms"):
            assert v == b[2]["report"][k] or (v != v and b[2]["report"][k] != b[2]["report"][k]), k
    for k, v in a[4].items():
        if not k.endswith("_ms"):
            assert np.array_equal(np.asarray(v), np.asarray(b[4][k])), k


@pytest.mark.gpu
def test_gpu_empty_selection_and_stale_count():
    """With the check on an empty selection launches no check: the loop ends as it does with the check off (fewer than 3 pairs,
    the reference's ValueError), and the context stays usable.  OA_STAT_RECIP_REJECTED never speaks of an older source or
    setting: 0 after set_source and after set_reciprocal until a step has run."""
    from object_alignment_amd.engine import IcpEngine, REF_VALUEERROR
    mxa, mxb = usual_pose()
    src, tgt = whole(3000), upper_half()
    with IcpEngine(0) as e:
        e.set_target(tgt)
        e.set_reciprocal(True)
        e.set_source(src, vlist=np.zeros(0, np.int64))
        assert e.n_selected == 0
        e.set_matrices(mxa, mxb)
        with pytest.raises(ValueError, match=REF_VALUEERROR):
            e.run(iters=3, thresh=THRESH)
        with pytest.raises(ValueError, match=REF_VALUEERROR):
            e.iterate(thresh=THRESH)
        A, _, _ = e.make_pairs(THRESH)
        assert A.shape == (3, 0) and e.stat("recip_rejected") == 0.0
        e.set_source(src, stride=1)
        e.set_matrices(mxa, mxb)
        A, _, _ = e.make_pairs(THRESH)
        assert A.shape == (3, 1264) and e.stat("recip_rejected") == float(2153 - 1264)     # (the first step of the table's case)
        e.set_reciprocal(True, 2.0)
        assert e.stat("recip_rejected") == 0.0                      # a changed setting: no step of it has run
        e.make_pairs(THRESH)
        assert e.stat("recip_rejected") == float(2153 - 1583)          # (ratio 2 keeps 1583 of them, counted in numpy)
        e.set_source(src, stride=2)
        assert e.stat("recip_rejected") == 0.0                      # a new source
        e.set_reciprocal(False)
        e.set_reciprocal(True)
        assert e.stat("recip_rejected") == 0.0
        r = e.run(iters=5, thresh=THRESH, target_d=0.01, early_exit=False)
        assert r.iters_done == 5 and e.stat("recip_rejected") > 0.0


@pytest.mark.gpu
def test_gpu_refusals_leave_the_context_usable():
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    mxa, mxb = usual_pose()
    src, tgt = whole(3000), upper_half()

    def plain_loop_ok(e, shards=False):
        e.set_reciprocal(False)
        if shards:
            e.set_source(src, stride=1)
        e.set_matrices(mxa, mxb)
        r = e.run(iters=5, thresh=THRESH, target_d=0.01, early_exit=False)
        assert r.iters_done == 5 and np.array_equal(r.step_K, want.step_K)
        assert np.max(np.abs(r.matrix_world.astype(np.float64) - want.matrix_world.astype(np.float64))) <= 1e-5

    with IcpEngine(0) as e:
        e.set_target(tgt)
        e.set_source(src, stride=1)
        e.set_matrices(mxa, mxb)
        want = e.run(iters=5, thresh=THRESH, target_d=0.01, early_exit=False)
        for ratio in (0.5, 0.0, 16.5, float("nan"), float("inf")):
            with pytest.raises(_capi.OaError, match=r"\[1, 16\]") as ei:
                e.set_reciprocal(True, ratio)
            assert ei.value.code == _capi.OA_E_BAD_ARG
        assert e.stat("reciprocal") == 0.0 and e.stat("reciprocal_ratio") == 1.0
        e.set_reciprocal(True, 16.0)
        e.set_reciprocal(True)
        e.set_matrices(mxa, mxb)
        with pytest.raises(_capi.OaError, match="oa_set_reciprocal") as ei:
            e.run_begin(iters=5)
        assert ei.value.code == _capi.OA_E_STATE
        plain_loop_ok(e)
        e.set_reciprocal(True)
        e.set_source(src, stride=1, shard_index=0, shard_count=2)
        e.set_matrices(mxa, mxb)
        with pytest.raises(_capi.OaError, match="shard") as ei:
            e.run(iters=5)
        assert ei.value.code == _capi.OA_E_STATE
        with pytest.raises(_capi.OaError, match="shard"):
            e.iterate()
        with pytest.raises(_capi.OaError, match="shard"):
            e.make_pairs(THRESH)
        plain_loop_ok(e, shards=True)
    with IcpEngine(devices=[0, 0]) as m:
        m.set_target(tgt)
        m.set_source(src, stride=1)
        m.set_matrices(mxa, mxb)
        m.set_reciprocal(True)
        assert m.stat("reciprocal") == 1.0
        with pytest.raises(_capi.OaError, match="single-device") as ei:
            m.run(iters=5)
        assert ei.value.code == _capi.OA_E_STATE
        with pytest.raises(_capi.OaError, match="single-device"):
            m.iterate()
        with pytest.raises(_capi.OaError, match="single-device") as ei:
            m.make_pairs(THRESH)
        assert ei.value.code == _capi.OA_E_STATE
        plain_loop_ok(m)
