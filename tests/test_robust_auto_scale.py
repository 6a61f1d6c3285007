"""The robust loss's scale from each step's own residuals (oa_set_robust_auto): c_i = max(m q_i, c_min), q_i the
ceil(p K_q)-th smallest float32 residual of step i's pairs.

The reference is the one of tests/test_robust_weights.py -- numpy, fp64, on the oracle's pairs -- with the scale formed here
from the same pairs: np.sort of the float32-rounded residuals (pairs of vertex weight 0 left out), the order statistic
k = ceil(float64(p) * float64(K_q)), c = max(m * float64(q), floor).  For the point metric the pair distances are the engine's
bit for bit, so the scale is held to `==`; for the plane metric the fp64 residuals differ in their last bits and the key is
their float32 rounding: 1 float32 ulp.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from object_alignment_amd import synth
from test_plane_metric import TOL, ref_pairs, scaled_base, selection, table_case, ulp_diff32
from test_robust_weights import (LOSSES, OUT_TARGET_D, _mul_v3, fast_pairs, kept_index, outlier_case, pose_error, psi,
                                 recorded_outlier_reference, vertex_weights, weighted_kabsch, weighted_plane_solve, world_scale)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 1e-4
GOLDEN = os.path.join(ROOT, "tests", "golden", "robust_auto_reference.npz")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build_hip()
    return g


def mad_tuning():
    from object_alignment_amd.operators.icp_align import MAD_TUNING
    return MAD_TUNING


# ------------------------------------------------------------------------------------------------ the reference
def order_statistic(res, wv, p):
    """(q, K_q): the ceil(p K_q)-th smallest (1-based) of the float32-rounded residuals whose vertex weight is > 0; (None, 0)
    when none takes part."""
    rho = np.asarray(res, np.float64).astype(np.float32)
    if wv is not None:
        rho = rho[np.asarray(wv) > 0]
    kq = len(rho)
    if kq == 0:
        return None, 0
    k = int(np.ceil(np.float64(p) * np.float64(kq)))
    return np.sort(rho)[k - 1], kq


def auto_c(res, wv, m, p, floor):
    q, _ = order_statistic(res, wv, p)
    return float(floor) if q is None else max(float(m) * float(np.float64(q)), float(floor))


def ref_step_auto(orc, metric, loss, m, p, floor, src_sel, wv_sel, mx1, mx2, tgt, s_world=1.0, c_given=None, **kw):
    """ref_step of test_robust_weights with the scale taken from the step's own pairs (c_given: use this scale instead, the
    plane test's second half).  dict(M, M_rev, new_mat, mw, K, W, mean, std, rank, c, Kq)."""
    if kw.get("tris") is None and kw.get("tgt_normals") is None:
        kw["tgt_normals"] = np.ones((len(tgt), 3), np.float32)
    pairs = kw.pop("pairs", ref_pairs)
    A, B, N, D = pairs(orc, src_sel, mx1, mx2, tgt, **kw)
    wv = None if wv_sel is None else np.asarray(wv_sel, np.float32).astype(np.float64)[kept_index(src_sel, A)]
    res = s_world * np.abs(np.einsum("ij,ij->i", N, A - B)) if metric == "plane" else D
    c = auto_c(res, wv, m, p, floor)
    w = (np.ones(len(A)) if wv is None else wv) * psi(loss, res, c if c_given is None else c_given)
    piv = src_sel[0].astype(np.float64)
    if metric == "plane":
        M, rank = weighted_plane_solve(A, B, N, w, piv)
        M_rev, _ = weighted_plane_solve(A, B, N, w, piv, reverse=True)
    else:
        M, rank = weighted_kabsch(A, B, w, piv), 0
        M_rev = weighted_kabsch(A, B, w, piv, reverse=True)
    new_mat = M.astype(np.float32)
    return dict(M=M, M_rev=M_rev, new_mat=new_mat, mw=orc.mat4_mul(np.asarray(mx1, np.float32), new_mat), K=len(A), W=float(w.sum()),
                mean=float(np.mean(D)), std=float(np.std(D)), rank=rank, c=c, Kq=order_statistic(res, wv, p)[1])


def ref_loop_auto(orc, loss, m, p, floor, src_sel, mx1, mx2, tgt, iters=50, target_d=1e-4, **kw):
    """ref_loop of test_robust_weights (point metric) around ref_step_auto; also the scales it went through."""
    mx1 = np.asarray(mx1, np.float32).copy()
    ring = [2.0 * target_d] * 5
    out = dict(iters_done=0, converged=False, scales=[], K=[])
    for n in range(iters):
        s = ref_step_auto(orc, "point", loss, m, p, floor, src_sel, None, mx1, mx2, tgt, **kw)
        mx1 = s["mw"]
        ring[n % 5] = orc.vec3_length(s["new_mat"][:3, 3])
        out["scales"].append(s["c"])
        out["K"].append(s["K"])
        out.update(iters_done=n + 1, matrix_world=mx1)
        if all(t < target_d for t in ring):
            out["converged"] = True
            break
    return out


@functools.lru_cache(maxsize=None)
def outlier_auto_reference():
    from oracle import oracle as orc
    orc.build()
    src, verts, tris, mxa, mxb = outlier_case()
    return ref_loop_auto(orc, "tukey", mad_tuning()["tukey"], 0.5, FLOOR, src, mxa, mxb, verts, iters=50, target_d=OUT_TARGET_D,
                         tris=tris, thresh=0.5, pairs=fast_pairs)


def vertex_pairs(orc, src_sel, mx1, mx2, tgt, thresh=0.5, **_):
    """ref_pairs for a vertex target without normals, over arrays (262 145 points in a second); (A, B, N = 0, D).
    test_reference_vertex_pairs holds it to ref_pairs."""
    mx1, mx2 = np.asarray(mx1, np.float32), np.asarray(mx2, np.float32)
    imx1, imx2 = orc.mat4_inverted(mx1), orc.mat4_inverted(mx2)
    src_sel, tgt = np.asarray(src_sel, np.float32), np.asarray(tgt, np.float32)
    w = _mul_v3(imx2, _mul_v3(mx1, src_sel))
    idx, _ = orc.nn_brute(w, tgt)
    wb = _mul_v3(mx2, tgt[idx])
    d = _mul_v3(mx2, w) - wb
    dist = np.sqrt(((d[:, 2] * d[:, 2]).astype(np.float64) + (d[:, 1] * d[:, 1]).astype(np.float64)) + (d[:, 0] * d[:, 0]).astype(np.float64))
    keep = dist < thresh
    return src_sel[keep].astype(np.float64), _mul_v3(imx1, wb)[keep].astype(np.float64), np.zeros((int(keep.sum()), 3)), dist[keep]


# ------------------------------------------------------------------------------------------------ CPU
def test_robust_auto_abi_and_bindings(built):
    """Fails without the feature: the header, the library, the bindings and the settings all name the estimated scale."""
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators import icp_align
    from object_alignment_amd.operators.icp_align import IcpSettings
    hdr = open(os.path.join(ROOT, "include", "oa_icp.h")).read()
    assert re.search(r"\bint\s+oa_set_robust_auto\s*\(\s*oa_ctx\s*\*\s*\w+\s*,\s*double\s+\w+\s*,\s*double\s+\w+\s*\)", hdr)
    for name, val in (("OA_STAT_ROBUST_SCALE", 32), ("OA_STAT_ROBUST_QUANTILE", 33)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name
    L = C.CDLL(os.path.join(ROOT, "object_alignment_amd", "liboa_icp.so"))
    assert hasattr(L, "oa_set_robust_auto")
    assert "oa_set_robust_auto" in _capi.SYMBOLS
    LL = _capi.load()
    assert LL.oa_set_robust_auto.argtypes is not None and len(LL.oa_set_robust_auto.argtypes) == 3
    assert IcpEngine.STATS["robust_scale"] == 32 and IcpEngine.STATS["robust_quantile"] == 33
    assert hasattr(IcpEngine, "set_robust_auto")
    st = IcpSettings()
    assert st.robust_quantile == 0.0 and st.robust_scale_min is None
    assert set(icp_align.MAD_TUNING) == {"huber", "tukey", "cauchy"}
    assert icp_align.MAD_TUNING["tukey"] == 4.685 * 1.4826 and icp_align.MAD_TUNING["huber"] == 1.345 * 1.4826
    assert icp_align.MAD_TUNING["cauchy"] == 2.385 * 1.4826
    assert C.sizeof(_capi.Settings) == 32 and C.sizeof(_capi.Report) == 72
    assert "OA_NSUMS 24" in hdr


def test_apply_robust_hands_the_auto_setting_over_every_time():
    from object_alignment_amd.operators.icp_align import IcpSettings, MAD_TUNING, apply_robust

    class Eng:
        def __init__(self):
            self.calls = []

        def set_robust(self, loss, scale):
            self.calls.append(("robust", loss, scale))

        def set_robust_auto(self, quantile, scale_min):
            self.calls.append(("auto", quantile, scale_min))

    e = Eng()
    apply_robust(e, IcpSettings(robust_loss="tukey", robust_scale=MAD_TUNING["tukey"], robust_quantile=0.5, target_d=2e-3))
    apply_robust(e, IcpSettings(robust_loss="tukey", robust_scale=0.15))
    apply_robust(e, IcpSettings(robust_loss="huber", robust_scale=2.0, robust_quantile=0.25, robust_scale_min=0.05))
    apply_robust(e, IcpSettings())
    assert e.calls == [("robust", "tukey", MAD_TUNING["tukey"]), ("auto", 0.5, 2e-3),      # floor None: the settings' target_d
                       ("robust", "tukey", 0.15), ("auto", 0.0, 0.0),                       # off is handed over too
                       ("robust", "huber", 2.0), ("auto", 0.25, 0.05),
                       ("robust", "none", 0.0), ("auto", 0.0, 0.0)]

    class Old:                                                      # an engine without set_robust_auto counts as off
        def set_robust(self, loss, scale):
            pass

    apply_robust(Old(), IcpSettings(robust_loss="tukey", robust_scale=0.15))
    with pytest.raises(RuntimeError):
        apply_robust(Old(), IcpSettings(robust_loss="tukey", robust_scale=1.0, robust_quantile=0.5))

    class Prefs:                                                    # the add-on's preference names
        icp_robust_loss, icp_robust_scale, icp_robust_quantile, icp_robust_scale_min, target_d = "cauchy", 3.5, 0.5, 0.0, 0.01

    apply_robust(e, Prefs())
    assert e.calls[-2:] == [("robust", "cauchy", 3.5), ("auto", 0.5, 0.01)]


def test_reference_vertex_pairs(orc):
    """vertex_pairs (the array form the large shards of the GPU tests use) is ref_pairs: A, B and the distances bit for bit."""
    src = synth.bunny_surface(300, 0.5)
    tgt = synth.bunny_surface(2000)
    _, _, _, mxa, mxb = table_case()
    for mx1, mx2 in ((mxa, mxb), ((scaled_base() @ mxa.astype(np.float64)).astype(np.float32), scaled_base().astype(np.float32))):
        x = vertex_pairs(orc, src, mx1, mx2, tgt)
        y = ref_pairs(orc, src, mx1, mx2, tgt, tgt_normals=np.ones((len(tgt), 3), np.float32))
        assert len(x[3]) > 100
        for k in (0, 1, 3):
            assert np.array_equal(x[k], y[k])
    assert order_statistic([3.0, 1.0, 2.0, 4.0], None, 0.5)[0] == 2.0 and order_statistic([3.0, 1.0, 2.0, 4.0], None, 0.51)[0] == 3.0
    assert order_statistic([3.0, 1.0, 2.0, 4.0], [1, 0, 1, 1], 1.0 / 3.0) == (2.0, 3)
    assert order_statistic([], None, 0.5) == (None, 0) and auto_c([], None, 2.0, 0.5, 0.25) == 0.25


def test_reference_auto_tukey_ends_closer_than_the_fixed_scale(orc):
    """The yardstick of the GPU outlier test: on outlier_case() the Tukey loop with the median-based scale
    (m = MAD_TUNING["tukey"], p = 0.5, floor 1e-4) converges and ends closer to the true pose than both recorded loops of
    robust_outlier_reference.npz, the unweighted one and the hand-picked fixed c = 0.15.  tests/golden/robust_auto_reference.npz
    holds its iteration count, convergence and final matrix_world (written once by this reference; recomputed here and held to
    the file).  Here: 27 iterations, pose error 7.04e-3 (unweighted 3.70e-2, fixed Tukey 9.71e-3); K = 5000 throughout, c from
    0.372 down to 0.0140."""
    ref = outlier_auto_reference()
    if not os.path.exists(GOLDEN):                                  # (first run in a fresh tree: the reference records itself)
        np.savez(GOLDEN, iters=np.int64(ref["iters_done"]), converged=np.bool_(ref["converged"]),
                 matrix_world=np.asarray(ref["matrix_world"], np.float32), scales=np.asarray(ref["scales"], np.float64))
    rec, old = np.load(GOLDEN), recorded_outlier_reference()
    print("auto tukey: %d iterations, pose error %.4g (unweighted %.4g, fixed tukey %.4g); K %d .. %d, c %.4g .. %.4g"
          % (ref["iters_done"], pose_error(ref["matrix_world"]), pose_error(old["none_matrix_world"]), pose_error(old["tukey_matrix_world"]),
             min(ref["K"]), max(ref["K"]), ref["scales"][0], ref["scales"][-1]))
    assert int(rec["iters"]) == ref["iters_done"] and bool(rec["converged"]) == ref["converged"]
    assert np.max(np.abs(rec["matrix_world"].astype(np.float64) - ref["matrix_world"].astype(np.float64))) < 1e-6
    assert np.max(np.abs(rec["scales"] - np.asarray(ref["scales"]))) < 1e-6
    assert ref["converged"]
    assert pose_error(ref["matrix_world"]) < pose_error(old["tukey_matrix_world"]) < pose_error(old["none_matrix_world"])


# ------------------------------------------------------------------------------------------------ GPU
def step_parity_auto(orc, eng, metric, loss, m, p, floor, src_sel, wv_sel, mxa, mxb, tgt, steps, **kw):
    s_world = world_scale(mxa)
    for it in range(steps):
        mw = eng.matrix_world()
        ref = ref_step_auto(orc, metric, loss, m, p, floor, src_sel, wv_sel, mw, mxb, tgt, s_world=s_world, **kw)
        M, st = eng.iterate(thresh=kw.get("thresh", 0.5), target_d=1e-4)
        c_dev = eng.stat("robust_scale")
        print("step %d: scale %.17g / %.17g, K_q %d" % (it, c_dev, ref["c"], ref["Kq"]))
        if metric == "plane":
            # the fp64 residuals differ in their last bits from numpy's and the key is their float32 rounding: 1 float32 ulp of
            # q, i.e. of c / m -- then the step itself with the device's scale in the reference
            assert ref["c"] > floor and ulp_diff32(np.float32(c_dev / m), np.float32(ref["c"] / m)) <= 1.0
            ref = ref_step_auto(orc, metric, loss, m, p, floor, src_sel, wv_sel, mw, mxb, tgt, s_world=s_world, c_given=c_dev, **kw)
        else:
            assert c_dev == ref["c"]
        assert np.max(np.abs(ref["M"] - ref["M_rev"])) < TOL, "the case is ill-conditioned for the reference itself"
        _, sN, _, _, _ = eng._history(1)
        dM, W = float(np.max(np.abs(M - ref["M"]))), eng.stat("weight_sum")
        print("        K %d / %d, |dM| %.3g, d mean %.3g, d std %.3g, new_mat ulps %.3g, sum w %.17g / %.17g"
              % (st["K"], ref["K"], dM, abs(st["mean_dist"] - ref["mean"]), abs(st["std_dist"] - ref["std"]),
                 ulp_diff32(sN[-1], ref["new_mat"]), W, ref["W"]))
        assert st["K"] == ref["K"]
        assert dM <= TOL
        assert abs(st["mean_dist"] - ref["mean"]) <= TOL and abs(st["std_dist"] - ref["std"]) <= TOL
        assert ulp_diff32(sN[-1], ref["new_mat"]) <= 1.0
        assert abs(W - ref["W"]) <= 1e-9 * ref["W"]
        if metric == "plane":
            assert int(eng.stat("plane_rank")) == ref["rank"]


@pytest.mark.gpu
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("case", ["surface", "vertex", "scaled_base", "vlist_stride2", "mode_brute", "mode_grid", "mode_bvh",
                                  "vertex_weights"])
def test_gpu_auto_point_step_parity(orc, case, loss):
    from object_alignment_amd.engine import IcpEngine
    src, verts, tris, mxa, mxb = table_case()
    m, p = mad_tuning()[loss], 0.5
    vlist, stride, wv, kw = None, 1, None, dict(thresh=0.5)
    with IcpEngine(0) as e:
        e.set_robust(loss, m)
        e.set_robust_auto(p, FLOOR)
        if case.startswith("mode_"):
            e.set_search_mode(case[5:])
        if case == "scaled_base":
            B = scaled_base()
            mxa = (B @ mxa.astype(np.float64)).astype(np.float32)
            mxb = B.astype(np.float32)
        if case == "vertex":
            tgt = synth.bunny_surface(20000)
            e.set_target(tgt)
        else:
            tgt = verts
            e.set_target_mesh(verts, tris)
            kw.update(tris=tris)
        if case == "vlist_stride2":
            vlist, stride = np.arange(len(src) - 1, -1, -1, dtype=np.int64)[: 4000], 2
        e.set_source(src, vlist=vlist, stride=stride)
        sel = selection(len(src), vlist, stride)
        if case == "vertex_weights":
            wv = vertex_weights(len(src))
            e.set_source_weights(wv)
        e.set_matrices(mxa, mxb)
        assert e.stat("robust_quantile") == p                       # survives the uploads and set_matrices
        step_parity_auto(orc, e, "point", loss, m, p, FLOOR, np.asarray(src, np.float32)[sel], None if wv is None else wv[sel],
                         mxa, mxb, tgt, 3, **kw)


@pytest.mark.gpu
def test_gpu_auto_quantile_edges(orc):
    """p = 1: the largest residual; p = 1 / K_q: the smallest; 0.25 and 0.9: their order statistics; a floor above m q: the
    floor.  One step each from the same pose, against np.sort of the oracle's distances.  The floor of the first four is far
    below every m q of this case (the smallest distance is 8e-6), so that the order statistic itself shows."""
    from object_alignment_amd.engine import IcpEngine
    src, verts, tris, mxa, mxb = table_case()
    A, _, _, D = fast_pairs(orc, np.asarray(src, np.float32), mxa, mxb, verts, tris)
    kq, m = len(D), 2.5
    rho = np.sort(D.astype(np.float32))
    with IcpEngine(0) as e:
        e.set_target_mesh(verts, tris)
        e.set_source(src, stride=1)
        e.set_robust("huber", m)
        tiny = 1e-12
        assert 0.0 < tiny < m * float(rho[0])
        for p, floor in ((1.0, tiny), (1.0 / kq, tiny), (0.25, tiny), (0.9, tiny), (0.5, 10.0), (1.0 / kq, FLOOR)):
            e.set_robust_auto(p, floor)
            e.set_matrices(mxa, mxb)
            _, st = e.iterate(thresh=0.5, target_d=1e-4)
            k = int(np.ceil(np.float64(p) * np.float64(kq)))
            c, want = e.stat("robust_scale"), max(m * float(np.float64(rho[k - 1])), floor)
            print("p %.6g: k %d of %d, scale %.17g / %.17g" % (p, k, kq, c, want))
            assert st["K"] == kq and c == want
            assert c == auto_c(D, None, m, p, floor)
            if p == 1.0:
                assert c == m * float(np.float64(rho[-1]))
            if p == 1.0 / kq and floor == tiny:
                assert k == 1 and c == m * float(np.float64(rho[0]))
            if floor != tiny:                                       # 10 > m q(0.5); 1e-4 > m x the smallest distance
                assert c == floor


@pytest.mark.gpu
@pytest.mark.parametrize("n_src", [65, 513, 262145])
def test_gpu_auto_selection_sizes(orc, n_src):
    """One wave plus one, one workgroup plus one, one more than the switch to 512-thread workgroups: the order statistic of a
    whole shard against np.sort (vertex target, 2 000 points)."""
    from object_alignment_amd.engine import IcpEngine
    _, _, _, mxa, mxb = table_case()
    src, tgt = synth.bunny_surface(n_src, 0.5), synth.bunny_surface(2000)
    _, _, _, D = vertex_pairs(orc, src, mxa, mxb, tgt)
    with IcpEngine(0) as e:
        e.set_target(tgt)
        e.set_source(src, stride=1)
        e.set_robust("tukey", 3.0)
        for p in (0.5, 1.0, 1.0 / len(D)):
            e.set_robust_auto(p, FLOOR)
            e.set_matrices(mxa, mxb)
            _, st = e.iterate(thresh=0.5, target_d=1e-4)
            c = e.stat("robust_scale")
            print("n %d, p %.6g: K %d / %d, scale %.17g / %.17g" % (n_src, p, st["K"], len(D), c, auto_c(D, None, 3.0, p, FLOOR)))
            assert st["K"] == len(D) and len(D) > n_src // 2
            assert c == auto_c(D, None, 3.0, p, FLOOR)


def _lattice(n=9, h=0.25):
    g = np.arange(n, dtype=np.float32) * np.float32(h)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


@pytest.mark.gpu
def test_gpu_auto_selection_degenerate_keys(orc):
    """A shard of one point (K < 3 fails as ever; the context stays usable); all residuals identical (a copy of the target's
    vertices under an exact translation along x: every key in one bin at every level); exact zeros in the lower half (q = 0:
    the floor decides)."""
    from object_alignment_amd.engine import IcpEngine
    eye = np.eye(4, dtype=np.float32)
    tgt = _lattice()
    shift = np.float32(0.0625)
    with IcpEngine(0) as e:
        e.set_target(tgt)
        e.set_robust("tukey", 3.0)
        e.set_robust_auto(0.5, FLOOR)
        e.set_source(tgt[:1] + np.array([shift, 0, 0], np.float32), stride=1)
        e.set_matrices(eye, eye)
        with pytest.raises(ValueError, match="input arrays are of wrong shape or type"):
            e.iterate(thresh=0.5, target_d=1e-4)
        # identical residuals
        src = tgt.copy()
        src[:, 0] += shift
        e.set_source(src, stride=1)
        e.set_matrices(eye, eye)
        D = vertex_pairs(orc, src, eye, eye, tgt)[3]
        assert len(D) == len(tgt) and np.all(D == 0.0625)
        for p in (0.5, 1.0, 1.0 / len(D)):
            e.set_robust_auto(p, FLOOR)
            e.set_matrices(eye, eye)
            _, st = e.iterate(thresh=0.5, target_d=1e-4)
            assert st["K"] == len(D) and e.stat("robust_scale") == 3.0 * 0.0625 == auto_c(D, None, 3.0, p, FLOOR)
        # zeros in the lower half
        src = tgt.copy()
        src[len(tgt) * 6 // 10:, 0] += shift
        e.set_source(src, stride=1)
        D = vertex_pairs(orc, src, eye, eye, tgt)[3]
        assert len(D) == len(tgt) and np.count_nonzero(D == 0.0) == len(tgt) * 6 // 10
        for p, want in ((0.5, FLOOR), (0.59, FLOOR), (0.61, 3.0 * 0.0625)):     # k = 365, 431 <= 437 zeros < 445
            e.set_robust_auto(p, FLOOR)
            e.set_matrices(eye, eye)
            _, st = e.iterate(thresh=0.5, target_d=1e-4)
            assert st["K"] == len(D) and e.stat("robust_scale") == want == auto_c(D, None, 3.0, p, FLOOR)
            if want == FLOOR:                                       # Tukey at c = floor: exactly the pairs at distance 0 weigh (1)
                assert e.stat("weight_sum") == float(np.count_nonzero(D == 0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["surface", "vertex_normals"])
def test_gpu_auto_plane_step_parity(orc, case):
    from object_alignment_amd.engine import IcpEngine
    src, verts, tris, mxa, mxb = table_case()
    m, kw = mad_tuning()["tukey"], dict(thresh=0.5)
    with IcpEngine(0) as e:
        e.set_metric("plane")
        e.set_robust("tukey", m)
        e.set_robust_auto(0.5, FLOOR)
        if case == "vertex_normals":
            tgt, tn = synth.bunny_surface_with_normals(20000)
            e.set_target(tgt)
            e.set_target_normals(tn)
            kw.update(tgt_normals=tn)
        else:
            tgt = verts
            e.set_target_mesh(verts, tris)
            kw.update(tris=tris)
        e.set_source(src, stride=1)
        e.set_matrices(mxa, mxb)
        step_parity_auto(orc, e, "plane", "tukey", m, 0.5, FLOOR, np.asarray(src, np.float32), None, mxa, mxb, tgt, 3, **kw)


def _auto_loop(e, src, verts, tris, mxa, mxb, iters=8):
    e.set_target_mesh(verts, tris)
    e.set_source(src, stride=1)
    e.set_matrices(mxa, mxb)
    return e.run(iters=iters, thresh=0.5, target_d=1e-4, early_exit=False)


RUN_FIELDS = ("step_M", "step_new", "step_K", "step_stats", "step_trans", "matrix_world")


@pytest.mark.gpu
def test_gpu_auto_bitwise_stability():
    from object_alignment_amd.engine import IcpEngine
    src, verts, tris, mxa, mxb = table_case()
    m = mad_tuning()["tukey"]
    runs = []
    for mode in (None, None, "brute", "grid", "bvh"):
        with IcpEngine(0) as e:
            if mode:
                e.set_search_mode(mode)
            e.set_robust("tukey", m)
            e.set_robust_auto(0.5, FLOOR)
            runs.append((_auto_loop(e, src, verts, tris, mxa, mxb), e.stat("robust_scale"), e.stat("weight_sum")))
            assert runs[-1][0].iters_done == 8 and FLOOR < runs[-1][1] < 0.5 and 0.0 < runs[-1][2] < float(runs[-1][0].last_K)
    for r, c, W in runs[1:]:
        for name in RUN_FIELDS:
            assert np.array_equal(getattr(r, name), getattr(runs[0][0], name)), name
        assert c == runs[0][1] and W == runs[0][2]
    # on, then off: the fixed-scale loop of a fresh engine, bit for bit
    with IcpEngine(0) as e:
        e.set_robust("tukey", 0.15)
        fixed = _auto_loop(e, src, verts, tris, mxa, mxb)
        assert e.stat("robust_scale") == 0.15 and e.stat("robust_quantile") == 0.0
    with IcpEngine(0) as e:
        e.set_robust("tukey", m)
        e.set_robust_auto(0.5, FLOOR)
        visit = _auto_loop(e, src, verts, tris, mxa, mxb, iters=3)
        e.set_robust_auto(0)
        e.set_robust("tukey", 0.15)
        back = _auto_loop(e, src, verts, tris, mxa, mxb)
        assert e.stat("robust_scale") == 0.15
    assert not np.array_equal(visit.step_M[0], fixed.step_M[0])
    # loss none with the setting on: inert, the unweighted loop
    with IcpEngine(0) as e:
        plain = _auto_loop(e, src, verts, tris, mxa, mxb)
    with IcpEngine(0) as e:
        e.set_robust_auto(0.5, FLOOR)
        inert = _auto_loop(e, src, verts, tris, mxa, mxb)
        assert e.stat("robust_scale") == 0.0 and e.stat("robust_quantile") == 0.5
    for name in RUN_FIELDS:
        assert np.array_equal(getattr(fixed, name), getattr(back, name)), name
        assert np.array_equal(getattr(plain, name), getattr(inert, name)), name


@pytest.mark.gpu
def test_gpu_auto_zero_one_weights_are_a_vlist():
    from object_alignment_amd.engine import IcpEngine
    src, verts, tris, mxa, mxb = table_case()
    rng = np.random.default_rng(9)
    w = np.ones(len(src), np.float32)
    zeros = 1 + rng.permutation(len(src) - 1)[:700]
    w[zeros] = 0.0
    keep = np.flatnonzero(w > 0).astype(np.int64)
    runs = {}
    for how in ("weights", "vlist"):
        with IcpEngine(0) as e:
            e.set_robust("tukey", mad_tuning()["tukey"])
            e.set_robust_auto(0.5, FLOOR)
            e.set_target_mesh(verts, tris)
            e.set_source(src, vlist=keep if how == "vlist" else None, stride=1)
            if how == "weights":
                e.set_source_weights(w)
            e.set_matrices(mxa, mxb)
            runs[how] = [e.iterate(thresh=0.5, target_d=1e-4) + (e.stat("robust_scale"),) for _ in range(3)]
    for (M0, s0, c0), (M1, s1, c1) in zip(runs["weights"], runs["vlist"]):
        print("|dM| %.3g, K %d / %d, scale %.17g / %.17g" % (np.max(np.abs(M0 - M1)), s0["K"], s1["K"], c0, c1))
        assert c0 == c1 and c0 > FLOOR
        assert np.max(np.abs(M0 - M1)) <= TOL
        assert s0["K"] - s1["K"] == len(zeros)


@pytest.mark.gpu
def test_gpu_auto_outlier_case_ends_closer():
    """The parameter-free setting through IcpAlign on outlier_case(): the iteration count and convergence of the recorded
    reference loop, its final matrix_world, and a pose closer than the unweighted loop's.  The final-pose bound: every step's M
    is the reference's to 1e-9 (the step-parity tests) and each of the recorded loop's iterations rounds matrix_world to
    float32 once, entries of magnitude <= 1: at most iterations x 2^-23."""
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings
    src, verts, tris, mxa, mxb = outlier_case()
    rec, old = np.load(GOLDEN), recorded_outlier_reference()
    with IcpEngine(0) as e:
        st = IcpSettings(sample_fraction=1, target_d=OUT_TARGET_D, robust_loss="tukey", robust_scale=mad_tuning()["tukey"],
                         robust_quantile=0.5)
        res = IcpAlign(st, engine=e).run(src, verts, mxa, mxb, target_tris=tris)
        assert e.stat("robust_quantile") == 0.5 and e.stat("robust_loss") == 2.0
        c_last = e.stat("robust_scale")
        plain = IcpAlign(IcpSettings(sample_fraction=1, target_d=OUT_TARGET_D), engine=e).run(src, verts, mxa, mxb, target_tris=tris)
        assert e.stat("robust_quantile") == 0.0
    d = float(np.max(np.abs(res.matrix_world.astype(np.float64) - rec["matrix_world"].astype(np.float64))))
    print("auto tukey: %d iterations (reference %d), pose error %.4g (reference %.4g, unweighted %.4g), |d matrix_world| %.3g, last scale %.6g / %.6g"
          % (res.iters_done, int(rec["iters"]), pose_error(res.matrix_world), pose_error(rec["matrix_world"]), pose_error(plain.matrix_world),
             d, c_last, float(rec["scales"][-1])))
    assert res.iters_done == int(rec["iters"]) and bool(res.converged) == bool(rec["converged"])
    assert d <= int(rec["iters"]) * 2.0 ** -23
    assert pose_error(res.matrix_world) < pose_error(plain.matrix_world)
    assert plain.iters_done == int(old["none_iters"])


@pytest.mark.gpu
def test_gpu_auto_refusals_leave_the_context_usable():
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    src, verts, tris, mxa, mxb = table_case()

    def refused(call, code=_capi.OA_E_BAD_ARG):
        with pytest.raises(_capi.OaError) as ei:
            call()
        assert ei.value.code == code
        return ei.value

    with IcpEngine(0) as e:
        e.set_robust("tukey", 0.15)
        e.set_target_mesh(verts, tris)
        e.set_source(src, stride=1)
        e.set_matrices(mxa, mxb)
        good = e.run(iters=5, thresh=0.5, target_d=1e-4, early_exit=False)

        def fixed_loop_ok(x):
            x.set_matrices(mxa, mxb)
            r = x.run(iters=5, thresh=0.5, target_d=1e-4, early_exit=False)
            assert r.iters_done == 5 and x.stat("robust_scale") == 0.15 and x.stat("robust_quantile") == 0.0
            for it in range(5):
                assert np.max(np.abs(r.step_M[it] - good.step_M[it])) <= TOL
            return r

        for bad in (-0.1, 1.5, float("nan")):
            refused(lambda: e.set_robust_auto(bad, FLOOR))
            assert np.array_equal(fixed_loop_ok(e).matrix_world, good.matrix_world)
        for bad in (0.0, -1e-3, float("inf"), float("nan")):
            refused(lambda: e.set_robust_auto(0.5, bad))
            assert np.array_equal(fixed_loop_ok(e).matrix_world, good.matrix_world)
        e.set_robust_auto(0.0, float("nan"))                        # (off: the floor is not looked at)
        e.set_robust_auto(0.5, FLOOR)
        e.set_matrices(mxa, mxb)
        err = refused(lambda: e.run_begin(iters=5, thresh=0.5, target_d=1e-4, early_exit=False), _capi.OA_E_STATE)
        assert "single-device" in str(err)
        e.set_robust_auto(0)
        assert np.array_equal(fixed_loop_ok(e).matrix_world, good.matrix_world)
    with IcpEngine(devices=[0, 0]) as mdev:
        mdev.set_target_mesh(verts, tris)
        mdev.set_source(src, stride=1)
        mdev.set_matrices(mxa, mxb)
        mdev.set_robust("tukey", 0.15)
        mdev.set_robust_auto(0.5, FLOOR)
        assert mdev.stat("robust_quantile") == 0.5
        with pytest.raises(_capi.OaError, match="single-device") as ei:
            mdev.run(iters=5)
        assert ei.value.code == _capi.OA_E_STATE
        with pytest.raises(_capi.OaError, match="single-device"):
            mdev.iterate()
        mdev.set_robust_auto(0)
        fixed_loop_ok(mdev)
