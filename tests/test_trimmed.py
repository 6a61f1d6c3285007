"""Trimmed ICP (oa_set_trim, IcpSettings.trim): every step keeps only its best pairs, the share fixed or estimated.

The rule (include/oa_icp.h).  The candidates of a step are the K_q pairs counted in K with a vertex weight > 0 (after the reciprocal
check, when that is on); each has the float32-rounded residual r the losses use.  Fixed share f: k = clamp(ceil(f K_q), min(3,
K_q), K_q), the cut q = the k-th smallest r.  Estimated share: S_j = sum_{i <= j} r_(i)^2 in fp64 over the sorted residuals, J(j) =
S_j j^-(1 + 2 lambda), k = the smallest j in [k_min, K_q] that minimises J, q = r_(k).  A candidate stays iff r <= q in float32.

The numpy reference lives here, on top of what is already there: test_plane_metric.ref_pairs / test_gicp_metric.ref_pairs (its
array form, with both normals; held to the former below) give the pairs, test_robust_weights' weighted solves, world_scale and psi
and test_gicp_metric.gicp_step the steps, test_robust_auto_scale.order_statistic the fixed cut, np.sort and a sequential
np.cumsum in fp64 the estimated one.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from object_alignment_amd import synth
import test_gicp_metric as G
from test_plane_metric import TOL, ref_pairs, selection, ulp_diff32
from test_reciprocal import THRESH, _kabsch, recip_keep, translation_error, upper_half, usual_pose, whole
from test_robust_auto_scale import FLOOR, _lattice, auto_c, mad_tuning, order_statistic, vertex_pairs
from test_robust_weights import psi, weighted_kabsch, weighted_plane_solve, world_scale

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO = "auto"
FMIN, LAM = 0.3, 2.0                 # the Python layer's defaults
J_MARGIN = 1e-9                      # n eps for n <= 8 388 608 fp64 additions: what a different summation order may move J by


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build_hip()
    return g


# ------------------------------------------------------------------------------------------------ the reference
def rank_floor(kq):
    return min(3, kq)


def fixed_rank(f, kq):
    """k = clamp(ceil(f K_q), min(3, K_q), K_q), fp64, 1-based"""
    return int(min(max(np.ceil(np.float64(f) * np.float64(kq)), rank_floor(kq)), kq))


def fixed_cut(res, f):
    """(q float32, k, K_q) of the candidates' residuals; (float32(0), 0, 0) without candidates.  The order statistic is
    test_robust_auto_scale's wherever the floor of three does not bind."""
    rho = np.asarray(res, np.float64).astype(np.float32)
    kq = len(rho)
    if kq == 0:
        return np.float32(0.0), 0, 0
    k = fixed_rank(f, kq)
    q = np.sort(rho)[k - 1]
    if k == int(np.ceil(np.float64(f) * np.float64(kq))):
        assert q == order_statistic(res, None, f)[0]
    return q, k, kq


def J_curve(res, lam=LAM):
    """(sorted float32 residuals, J(1 .. K_q)): S_j a sequential fp64 running sum of the exact squares"""
    rho = np.sort(np.asarray(res, np.float64).astype(np.float32))
    S = np.cumsum(rho.astype(np.float64) ** 2)
    j = np.arange(1, len(rho) + 1, dtype=np.float64)
    return rho, S * j ** -(1.0 + 2.0 * lam)


def estimated_cut(res, fmin=FMIN, lam=LAM):
    """(q float32, k, K_q): the smallest j in [k_min, K_q] that minimises J"""
    rho, J = J_curve(res, lam)
    kq = len(rho)
    if kq == 0:
        return np.float32(0.0), 0, 0
    k_min = fixed_rank(fmin, kq)
    k = k_min + int(np.argmin(J[k_min - 1:]))                      # (argmin: the first of equal minima)
    return rho[k - 1], k, kq


def cut_of(res, fraction, fmin=FMIN, lam=LAM):
    return estimated_cut(res, fmin, lam) if fraction == AUTO else fixed_cut(res, fraction)


def trim_keep(res, cand, q):
    """the mask of the pairs that stay: a candidate iff its float32 residual is <= q, anything else as it was"""
    rho = np.asarray(res, np.float64).astype(np.float32)
    return ~np.asarray(cand, bool) | (rho <= np.float32(q))


def check_estimate(res, q_engine, fmin=FMIN, lam=LAM):
    """The engine's k may differ from numpy's only at a near-tie: J_ref(k_engine) <= J_ref(k_ref) (1 + 1e-9), and k_engine ==
    k_ref whenever every other rank's J is more than 1e-9 above the minimum.  Returns the reference's (q, k, K_q)."""
    rho, J = J_curve(res, lam)
    q_ref, k_ref, kq = estimated_cut(res, fmin, lam)
    if kq == 0:
        assert q_engine == 0.0
        return q_ref, k_ref, kq
    k_min = fixed_rank(fmin, kq)
    ranks = np.flatnonzero(rho == np.float32(q_engine)) + 1        # the ranks that carry the engine's cut
    ranks = ranks[ranks >= k_min]
    assert len(ranks) > 0, "the engine's cut %r is no residual of a competing rank" % (q_engine,)
    J_engine = float(np.min(J[ranks - 1]))
    assert J_engine <= float(J[k_ref - 1]) * (1.0 + J_MARGIN)
    others = np.delete(J[k_min - 1:], k_ref - k_min)
    if len(others) == 0 or float(np.min(others)) > float(J[k_ref - 1]) * (1.0 + J_MARGIN):
        assert np.float32(q_engine) == q_ref
    return q_ref, k_ref, kq


def residuals(metric, P, piv, s_world, eps=G.EPS):
    """the residual the losses use, fp64 (its float32 rounding is the key): point: the world-space pair distance; plane:
    s |n . (a - b)|; GICP: s sqrt(e^T W e) -- a, b about the pivot, summed left to right as the kernels do"""
    if metric == "point":
        return P["dist"]
    e = (P["a"] - piv) - (P["b"] - piv)
    if metric == "plane":
        n = P["n_b"]
        return s_world * np.abs((n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2])
    W = G.gicp_weights(P["n_a"], P["n_b"], eps)
    rr = np.einsum("ki,ki->k", e, np.einsum("kij,kj->ki", W, e))
    return s_world * np.sqrt(np.maximum(rr, 0.0))


def solve(metric, P, keep, piv, w=None, eps=G.EPS):
    """(M, M_rev, rank) of the kept pairs; w: one weight per kept pair (None: every pair weighs one)"""
    a, b, na, nb = P["a"][keep], P["b"][keep], P["n_a"][keep], P["n_b"][keep]
    ones = np.ones(len(a)) if w is None else w
    if metric == "point":
        return weighted_kabsch(a, b, ones, piv), weighted_kabsch(a, b, ones, piv, reverse=True), 0
    if metric == "plane":
        M, rank = weighted_plane_solve(a, b, nb, ones, piv)
        return M, weighted_plane_solve(a, b, nb, ones, piv, reverse=True)[0], rank
    M, rank, _, _ = G.gicp_step(a, b, na, nb, piv, eps, w_vertex=w)
    return M, G.gicp_step(a, b, na, nb, piv, eps, reverse=True, w_vertex=w)[0], rank


# ---- the partial-overlap case of the issue's table: the whole source onto the upper half, 60 point-metric steps in fp64
@functools.lru_cache(maxsize=None)
def numpy_loop(trim, lam=LAM, fmin=FMIN, iters=60):
    """Written like test_reciprocal.numpy_loop.  trim: 0.0 (plain), a share, or "auto".  Returns (translation error, rotation
    error in degrees, K_q of the last step, pairs kept in the last step)."""
    from oracle import oracle as orc
    orc.build()
    src, tgt = whole().astype(np.float64), upper_half().astype(np.float64)
    kt = orc.KDTree(tgt)
    M = usual_pose()[0].astype(np.float64)
    kq = kept = 0
    for _ in range(iters):
        w = src @ M[:3, :3].T + M[:3, 3]
        q = tgt[kt.query(w)[0]]
        d = np.linalg.norm(w - q, axis=1)
        keep = d < THRESH
        Mi = np.linalg.inv(M)
        b = q @ Mi[:3, :3].T + Mi[:3, 3]
        kq = int(keep.sum())
        if trim != 0.0:
            cut, _, _ = cut_of(d[keep], trim, fmin, lam)
            keep &= d.astype(np.float32) <= cut
        kept = int(keep.sum())
        M = M @ _kabsch(src[keep], b[keep])
    ang = np.degrees(np.arccos(np.clip((np.trace(M[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))
    return float(np.linalg.norm(M[:3, 3])), float(ang), kq, kept


# ------------------------------------------------------------------------------------------------ CPU
def test_trim_abi_and_bindings(built):
    """Fails without the feature: the header, both libraries, the bindings, the settings and the add-on all name the trim."""
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators import icp_align
    from object_alignment_amd.operators.icp_align import IcpSettings
    hdr = open(os.path.join(ROOT, "include", "oa_icp.h")).read()
    assert re.search(r"\bint\s+oa_set_trim\s*\(\s*oa_ctx\s*\*\s*\w*\s*,\s*double\s+\w+\s*,\s*double\s+\w+\s*,\s*double\s+\w+\s*\)", hdr)
    assert re.search(r"#define\s+OA_TRIM_AUTO\s+\(-1\.0\)", hdr) and _capi.OA_TRIM_AUTO == -1.0
    for name, val in (("OA_STAT_TRIM", 40), ("OA_STAT_TRIM_CANDIDATES", 41), ("OA_STAT_TRIM_KEPT", 42), ("OA_STAT_TRIM_CUT", 43)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name
        assert getattr(_capi, name) == val
    assert "oa_set_trim" in _capi.SYMBOLS
    for lib in ("liboa_icp.so", "liboa_icp_exp.so"):
        assert hasattr(C.CDLL(os.path.join(ROOT, "object_alignment_amd", lib)), "oa_set_trim"), lib
    assert _capi.load().oa_set_trim.argtypes == [C.c_void_p, C.c_double, C.c_double, C.c_double]
    assert callable(IcpEngine.set_trim)
    assert [IcpEngine.STATS[k] for k in ("trim", "trim_candidates", "trim_kept", "trim_cut")] == [40, 41, 42, 43]
    s = IcpSettings()
    assert s.trim == 0.0 and s.trim_min == 0.3 and s.trim_lambda == 2.0
    assert icp_align.trim_of(s) == (0.0, 0.3, 2.0)
    assert icp_align.trim_of(IcpSettings(trim=0.6)) == (0.6, 0.3, 2.0)
    assert icp_align.trim_of(IcpSettings(trim="auto", trim_min=0.4, trim_lambda=3.0)) == ("auto", 0.4, 3.0)
    with pytest.raises(ValueError):
        icp_align.trim_of(IcpSettings(trim="most"))

    class Prefs:                                                  # the registered add-on preferences' names
        icp_trim, icp_trim_auto, icp_trim_min = 0.7, False, 0.25
    assert icp_align.trim_of(Prefs()) == (0.7, 0.25, 2.0)
    Prefs.icp_trim_auto = True
    assert icp_align.trim_of(Prefs()) == ("auto", 0.25, 2.0)
    assert icp_align.trim_of(object()) == (0.0, 0.3, 2.0)
    addon = open(os.path.join(ROOT, "object_alignment_amd", "blender_addon.py")).read()
    assert re.search(r"icp_trim\s*:\s*FloatProperty", addon) and re.search(r"icp_trim_auto\s*:\s*BoolProperty", addon)
    assert re.search(r"icp_trim_min\s*:\s*FloatProperty", addon)
    assert C.sizeof(_capi.Settings) == 32 and C.sizeof(_capi.Report) == 72       # oa_settings / oa_report do not change

    class E:
        def __init__(self):
            self.calls = []

        def set_trim(self, fraction, fraction_min, lam):
            self.calls.append((fraction, fraction_min, lam))
    e = E()
    icp_align.apply_trim(e, IcpSettings(trim=0.5))
    icp_align.apply_trim(e, IcpSettings(trim="auto", trim_min=0.2))
    icp_align.apply_trim(e, IcpSettings())
    assert e.calls == [(0.5, 0.3, 2.0), ("auto", 0.2, 2.0), (0.0, 0.3, 2.0)]     # off is handed over too: the engine is shared
    icp_align.apply_trim(object(), IcpSettings())                 # an engine without the setter counts as trim-off
    with pytest.raises(RuntimeError):
        icp_align.apply_trim(object(), IcpSettings(trim=0.5))


def test_reference_rule_on_a_handful_of_residuals():
    r = [0.5, 0.1, 0.4, 0.2, 0.3, 0.6, 0.7, 0.8]
    assert fixed_cut(r, 0.5) == (np.float32(0.4), 4, 8) and fixed_cut(r, 0.51)[1] == 5 and fixed_cut(r, 1.0)[0] == np.float32(0.8)
    assert fixed_cut(r, 0.01)[1] == 3 and fixed_cut(r[:2], 0.01)[1] == 2 and fixed_cut([], 0.5) == (np.float32(0.0), 0, 0)
    assert trim_keep(r, np.ones(8, bool), np.float32(0.4)).tolist() == [False, True, True, True, True, False, False, False]
    assert trim_keep(r, [False] + [True] * 7, np.float32(0.4))[0]                # not a candidate: the verdict it had
    # J: four small residuals, then a jump -- the jump does not pay at lambda = 2, whatever the floor below it
    rr = [0.010, 0.011, 0.012, 0.013, 0.5, 0.6]
    assert estimated_cut(rr, 0.3, 2.0)[1] == 4 and estimated_cut(rr, 1.0, 2.0)[1] == 6
    assert estimated_cut([0.0, 0.0, 0.0, 0.0, 0.2, 0.3], 0.5, 2.0)[1] == 3       # S_j = 0: every J ties at 0, k_min wins
    assert estimated_cut([0.25] * 6, 0.3, 2.0)[:2] == (np.float32(0.25), 6)       # equal residuals: J falls with j


def test_reference_pairs_agree(orc):
    """test_gicp_metric.ref_pairs (arrays; what the step tests use for all three metrics) is test_plane_metric.ref_pairs: a, b, the
    target's unit normal and the distances, bit for bit."""
    src, sn, verts, tris, mxa, mxb = G.table_case()
    tgt, tn = synth.bunny_surface_with_normals(2000)
    for kw in (dict(tris=tris), dict(tgt_normals=tn)):
        t = verts if "tris" in kw else tgt
        A, B, N, D = ref_pairs(orc, src[:200], mxa, mxb, t, thresh=THRESH, **kw)
        P = G.ref_pairs(orc, src[:200], sn[:200], mxa, mxb, t, thresh=THRESH, **kw)
        assert len(D) > 100
        assert np.array_equal(A, P["a"]) and np.array_equal(B, P["b"]) and np.array_equal(D, P["dist"])
        assert np.max(np.abs(N - P["n_b"])) <= 1e-15


def test_reference_discriminates():
    """The issue's table, recomputed: on the whole source against the upper half (true overlap 0.50) trim 0.5 and the estimated
    share each end at a translation error below a quarter of the plain loop's (measured 1.8e-1 against 3.4e-3 and 7.8e-3), and
    the estimated loop's last kept share, times K_q / N, lies within 0.1 of the overlap (measured 0.52)."""
    te0, ang0, kq0, _ = numpy_loop(0.0)
    te5, ang5, _, _ = numpy_loop(0.5)
    tea, anga, kqa, kepta = numpy_loop(AUTO)
    n = len(whole())
    print("plain %.3g / %.3g deg (K_q %d); trim 0.5 %.3g / %.3g deg; estimated %.3g / %.3g deg, kept %d of %d candidates of %d points"
          % (te0, ang0, kq0, te5, ang5, tea, anga, kepta, kqa, n))
    assert te5 < 0.25 * te0 and tea < 0.25 * te0
    assert abs(kepta / n - 0.5) <= 0.1


# ------------------------------------------------------------------------------------------------ GPU: step parity
CASES = ["surface", "vertex", "scaled_base", "vlist_stride2"]
MODES = ["brute", "grid", "bvh"]
METRICS = ["point", "plane", "gicp"]


@functools.lru_cache(maxsize=None)
def parity_case(case):
    """dict(src, sn, sel, vlist, stride, tgt, tris, tn, mxa, mxb): the shapes of the sibling files' step-parity cases"""
    src, sn, verts, tris, mxa, mxb = G.table_case()
    d = dict(src=src, sn=sn, vlist=None, stride=1, tgt=verts, tris=tris, tn=None, mxa=mxa, mxb=mxb)
    if case == "vertex":
        tgt, tn = synth.bunny_surface_with_normals(20000)
        d.update(tgt=np.asarray(tgt, np.float32), tn=np.asarray(tn, np.float32), tris=None)
    elif case == "scaled_base":
        B = G.scaled_base()
        d.update(mxa=(B @ mxa.astype(np.float64)).astype(np.float32), mxb=B.astype(np.float32))
    elif case == "vlist_stride2":
        d.update(vlist=np.arange(len(src) - 1, -1, -1, dtype=np.int64)[:4000], stride=2)
    elif case != "surface":
        raise ValueError(case)
    d["sel"] = selection(len(src), d["vlist"], d["stride"])
    return d


_PAIRS = {}


def case_pairs(orc, case, mw):
    """the pairs of `case` at matrix_world mw, computed once: the search modes (and the first step of every metric and fraction)
    meet the same poses bit for bit"""
    key = (case, np.asarray(mw, np.float32).tobytes())
    if key not in _PAIRS:
        d = parity_case(case)
        _PAIRS[key] = G.ref_pairs(orc, d["src"][d["sel"]], d["sn"][d["sel"]], mw, d["mxb"], d["tgt"], tris=d["tris"], tgt_normals=d["tn"],
                                  thresh=THRESH)
    return _PAIRS[key]


def open_case(e, case, mode, metric):
    d = parity_case(case)
    e.set_search_mode(mode)
    e.set_metric(metric)
    if d["tris"] is None:
        e.set_target(d["tgt"])
        e.set_target_normals(d["tn"])
    else:
        e.set_target_mesh(d["tgt"], d["tris"])
    e.set_source(d["src"], vlist=d["vlist"], stride=d["stride"])
    e.set_source_normals(d["sn"])
    e.set_matrices(d["mxa"], d["mxb"])
    return d


def trimmed_step_parity(orc, e, case, metric, fraction, steps=3):
    """step_parity_auto's discipline: before every step the engine's matrix_world goes to the reference.  K, the candidates, the
    survivors and the bits of the cut exact (estimated share: the cut under check_estimate's rule, then the reference step from
    the engine's cut); M within the sibling files' TOL."""
    d = parity_case(case)
    piv = d["src"][d["sel"]][0].astype(np.float64)
    s_world = world_scale(e.matrix_world())                        # (the sequence of iterate() calls starts here)
    for it in range(steps):
        mw = e.matrix_world()
        P = case_pairs(orc, case, mw)
        res = residuals(metric, P, piv, s_world)
        M_dev, st = e.iterate(thresh=THRESH, target_d=1e-4)
        cand, kept, cut = int(e.stat("trim_candidates")), int(e.stat("trim_kept")), e.stat("trim_cut")
        if fraction == AUTO:
            q_ref, k_ref, kq = check_estimate(res, cut)
            q = np.float32(cut)
        else:
            q, k_ref, kq = fixed_cut(res, fraction)
            assert np.float32(cut) == q and float(np.float32(cut)) == cut, "the cut's bits"
        keep = trim_keep(res, np.ones(len(res), bool), q)
        M, M_rev, rank = solve(metric, P, keep, piv)
        spread = float(np.max(np.abs(M - M_rev)))
        tol = TOL if (metric != "gicp" or spread <= TOL / 10) else 100.0 * spread      # (test_gicp_metric.step_parity's bound)
        assert spread < TOL or metric == "gicp", "the case is ill-conditioned for the reference itself"
        D = P["dist"][keep]
        dM = float(np.max(np.abs(M_dev - M)))
        print("step %d: K %d / %d, candidates %d / %d, kept %d / %d (rank %d), cut %.9g / %.9g, |dM| %.3g, d mean %.3g"
              % (it, st["K"], int(keep.sum()), cand, kq, kept, int(keep.sum()), k_ref, cut, float(q), dM, abs(st["mean_dist"] - D.mean())))
        assert cand == kq == len(res) and kept == int(keep.sum()) and st["K"] == kept
        assert kept >= k_ref or fraction == AUTO
        if fraction == 1.0:
            assert kept == kq and cut == float(np.max(res.astype(np.float32)))       # nothing trimmed: the plain step's sums
        elif fraction != AUTO:
            assert kept < kq                                        # the trim had something to say
        assert dM <= tol
        assert abs(st["mean_dist"] - float(np.mean(D))) <= TOL and abs(st["std_dist"] - float(np.std(D))) <= TOL
        _, sN, _, _, _ = e._history(1)
        assert ulp_diff32(sN[-1], M.astype(np.float32)) <= 1.0
        if metric != "point":
            assert int(e.stat("plane_rank")) == rank


@pytest.mark.gpu
@pytest.mark.parametrize("fraction", [0.5, 1.0])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_gpu_fixed_share_step_parity(orc, case, mode, metric, fraction):
    from object_alignment_amd.engine import IcpEngine
    with IcpEngine(0) as e:
        e.set_trim(fraction)
        open_case(e, case, mode, metric)
        assert e.stat("trim") == fraction                           # survives the uploads and set_matrices
        assert e.stat("trim_candidates") == 0.0 and e.stat("trim_cut") == 0.0      # no step has run
        trimmed_step_parity(orc, e, case, metric, fraction)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_gpu_estimated_share_step_parity(orc, case, mode, metric):
    from object_alignment_amd.engine import IcpEngine
    with IcpEngine(0) as e:
        e.set_trim(AUTO)
        open_case(e, case, mode, metric)
        assert e.stat("trim") == -1.0
        trimmed_step_parity(orc, e, case, metric, AUTO)


# ------------------------------------------------------------------------------------------------ GPU: sizes, degenerate keys
@functools.lru_cache(maxsize=None)
def size_case(n_src):
    from oracle import oracle as orc
    orc.build()
    _, _, _, _, mxa, mxb = G.table_case()
    src, tgt = synth.bunny_surface(n_src, 0.5), synth.bunny_surface(2000)
    return src, tgt, mxa, mxb, vertex_pairs(orc, src, mxa, mxb, tgt)[3]


@pytest.mark.gpu
@pytest.mark.parametrize("fraction", [0.5, AUTO])
@pytest.mark.parametrize("n_src", [65, 513, 8193, 20481])
def test_gpu_selection_sizes(n_src, fraction):
    """One wave plus one, one workgroup plus one, one past SORT_SMALL_MAX (the first LSD sort), ten scan tiles plus one element:
    cut, kept count and K of a whole shard against np.sort (vertex target, 2 000 points)."""
    from object_alignment_amd.engine import IcpEngine
    src, tgt, mxa, mxb, D = size_case(n_src)
    with IcpEngine(0) as e:
        e.set_target(tgt)
        e.set_source(src, stride=1)
        e.set_trim(fraction)
        e.set_matrices(mxa, mxb)
        _, st = e.iterate(thresh=THRESH, target_d=1e-4)
        cut = e.stat("trim_cut")
        q, k, kq = check_estimate(D, cut) if fraction == AUTO else fixed_cut(D, fraction)
        if fraction == AUTO:
            q = np.float32(cut)
        kept = int(np.count_nonzero(D.astype(np.float32) <= q))
        print("n %d, %s: candidates %d / %d, rank %d, cut %.9g / %.9g, kept %d / %d" % (n_src, fraction, e.stat("trim_candidates"), kq, k, cut, float(q),
                                                                                       e.stat("trim_kept"), kept))
        assert n_src // 2 < kq == len(D) == e.stat("trim_candidates")
        assert np.float32(cut) == q and float(np.float32(cut)) == cut
        assert e.stat("trim_kept") == kept == st["K"] and k <= kept <= kq
        assert kept < kq or fraction == AUTO                        # (the estimate may keep every pair of a full overlap)


def _one_step(e, fraction, eye):
    e.set_trim(fraction)
    e.set_matrices(eye, eye)
    _, st = e.iterate(thresh=THRESH, target_d=1e-4)
    return st["K"], int(e.stat("trim_candidates")), int(e.stat("trim_kept")), e.stat("trim_cut")


@pytest.mark.gpu
def test_gpu_degenerate_keys(orc):
    """On the 729-point lattice, the source its copy under exact shifts along x: all residuals equal (ties keep everything); two
    values with the k-th on the boundary; a run of exact zeros at the front (S_j = 0: the estimate lands on k_min); K_q = 3;
    K_q = 0 (every weight zero: nothing trimmed)."""
    from object_alignment_amd.engine import IcpEngine, REF_VALUEERROR
    eye = np.eye(4, dtype=np.float32)
    tgt = _lattice()
    n = len(tgt)
    big, small = np.float32(0.0625), np.float32(0.03125)
    with IcpEngine(0) as e:
        e.set_target(tgt)
        src = tgt.copy()
        src[:, 0] += big
        e.set_source(src, stride=1)
        for fraction in (0.5, 1.0 / n, 1.0, AUTO):
            assert _one_step(e, fraction, eye) == (n, n, n, 0.0625)
        # two values: n_small of the smaller one
        n_small = 291
        src = tgt.copy()
        src[:n_small, 0] += small
        src[n_small:, 0] += big
        e.set_source(src, stride=1)
        D = vertex_pairs(orc, src, eye, eye, tgt)[3]
        assert len(D) == n and np.count_nonzero(D == 0.03125) == n_small and np.count_nonzero(D == 0.0625) == n - n_small
        for k in (n_small - 1, n_small, n_small + 1):
            f = (k - 0.5) / n                                       # ceil(f n) = k
            assert fixed_rank(f, n) == k
            want = (n_small, 0.03125) if k <= n_small else (n, 0.0625)
            assert _one_step(e, f, eye) == (want[0], n, want[0], want[1])
            assert fixed_cut(D, f)[0] == np.float32(want[1])
        # zeros at the front: 437 of them, k_min = ceil(0.3 x 729) = 219 <= 437
        n_zero = n * 6 // 10
        src = tgt.copy()
        src[n_zero:, 0] += big
        e.set_source(src, stride=1)
        D = vertex_pairs(orc, src, eye, eye, tgt)[3]
        assert np.count_nonzero(D == 0.0) == n_zero and estimated_cut(D)[:2] == (np.float32(0.0), 219)
        assert _one_step(e, AUTO, eye) == (n_zero, n, n_zero, 0.0)
        assert _one_step(e, 0.5, eye) == (n_zero, n, n_zero, 0.0)   # k = 365 <= 437: the cut is 0 here too, the zeros tie
        assert _one_step(e, 0.61, eye) == (n, n, n, 0.0625)         # k = 445 > 437
        # K_q = 3: the floor of three keeps all of them, whatever the share
        three = tgt[[0, 1, 9]].copy()
        three[:, 0] += np.array([small, big, big + small], np.float32)
        e.set_source(three, stride=1)
        for fraction in (0.01, 0.5, AUTO):
            assert _one_step(e, fraction, eye) == (3, 3, 3, float(big + small))
        # K_q = 0: every vertex weight zero -- no candidate, nothing trimmed, the cut 0
        src = tgt.copy()
        src[:, 0] += big
        e.set_source(src, stride=1)
        e.set_source_weights(np.zeros(n, np.float32))
        for fraction in (0.5, AUTO):
            e.set_trim(fraction)
            e.set_matrices(eye, eye)
            A, _, _ = e.make_pairs(THRESH)
            assert A.shape == (3, n) and (e.stat("trim_candidates"), e.stat("trim_kept"), e.stat("trim_cut")) == (0.0, 0.0, 0.0)
            with pytest.raises(ValueError, match=REF_VALUEERROR):   # (sum w = 0: the weighted step has nothing to solve, as ever)
                e.iterate(thresh=THRESH, target_d=1e-4)
        e.set_source_weights(None)
        assert _one_step(e, 0.5, eye) == (n, n, n, 0.0625)          # the context stays usable


# ------------------------------------------------------------------------------------------------ GPU: composition
@pytest.mark.gpu
@pytest.mark.parametrize("fraction", [0.5, AUTO])
def test_gpu_composes_with_the_reciprocal_check(orc, fraction):
    """With oa_set_reciprocal on the candidates are the mutual pairs: TRIM_CANDIDATES == K_plain - recip_rejected, and make_pairs
    returns the reference's mutual pairs under the cut of their own distances."""
    from object_alignment_amd.engine import IcpEngine
    mxa, mxb = usual_pose()
    src, tgt = whole(1000), upper_half()
    A, B, _, D = ref_pairs(orc, src, mxa, mxb, tgt, tgt_normals=np.ones((len(tgt), 3), np.float32), thresh=THRESH)
    mutual = recip_keep(orc, A, B, src)
    q, k, kq = cut_of(D[mutual], fraction)
    keep = mutual & (D.astype(np.float32) <= q)
    with IcpEngine(0) as e:
        e.set_target(tgt)
        e.set_source(src, stride=1)
        e.set_matrices(mxa, mxb)
        e.set_reciprocal(True)
        e.set_trim(fraction)
        Ae, Be, _ = e.make_pairs(THRESH)
        rejected = e.stat("recip_rejected")
        print("%s: %d plain, %d mutual, %d kept (rank %d), cut %.9g / %.9g" % (fraction, len(D), kq, int(keep.sum()), k, e.stat("trim_cut"), float(q)))
        assert 0 < rejected == len(D) - kq and e.stat("trim_candidates") == len(D) - rejected
        if fraction == AUTO:
            check_estimate(D[mutual], e.stat("trim_cut"))
        assert np.float32(e.stat("trim_cut")) == q and e.stat("trim_kept") == keep.sum() and 3 <= keep.sum() < kq
        assert np.array_equal(Ae.T, A[keep]) and np.array_equal(Be.T, B[keep])


@pytest.mark.gpu
def test_gpu_composes_with_the_estimated_robust_scale(orc):
    """Tukey with oa_set_robust_auto on top of the trim: robust_scale is the quantile of the SURVIVORS' residuals, three steps."""
    from object_alignment_amd.engine import IcpEngine
    m, p = mad_tuning()["tukey"], 0.5
    with IcpEngine(0) as e:
        e.set_trim(0.5)
        e.set_robust("tukey", m)
        e.set_robust_auto(p, FLOOR)
        d = open_case(e, "surface", "auto", "point")
        piv = d["src"][0].astype(np.float64)
        for it in range(3):
            P = case_pairs(orc, "surface", e.matrix_world())
            q, _, kq = fixed_cut(P["dist"], 0.5)
            keep = trim_keep(P["dist"], np.ones(kq, bool), q)
            c = auto_c(P["dist"][keep], None, m, p, FLOOR)
            c_all = auto_c(P["dist"], None, m, p, FLOOR)
            w = psi("tukey", P["dist"][keep], c)
            M, _, _ = solve("point", P, keep, piv, w)
            M_dev, st = e.iterate(thresh=THRESH, target_d=1e-4)
            print("step %d: scale %.17g / %.17g (over all candidates it would be %.17g), K %d / %d, |dM| %.3g"
                  % (it, e.stat("robust_scale"), c, c_all, st["K"], int(keep.sum()), np.max(np.abs(M_dev - M))))
            assert e.stat("robust_scale") == c != c_all
            assert st["K"] == keep.sum() and e.stat("trim_kept") == keep.sum() and np.float32(e.stat("trim_cut")) == q
            assert np.max(np.abs(M_dev - M)) <= TOL
            assert abs(e.stat("weight_sum") - w.sum()) <= 1e-9 * w.sum()


@pytest.mark.gpu
@pytest.mark.parametrize("fraction", [0.5, AUTO])
def test_gpu_zero_one_weights_are_a_vlist(fraction):
    """Zero / one vertex weights against the vlist of the ones: the same candidates, cuts, survivors and float32 poses bit for
    bit, step after step; K differs by the zero-weight pairs (no candidates: they keep their verdict), and the fp64 M agrees to
    TOL (the two selections' partial sums are grouped differently)."""
    from object_alignment_amd.engine import IcpEngine
    src, verts, tris, mxa, mxb = G.table_case()[0], *G.table_case()[2:]
    rng = np.random.default_rng(9)
    w = np.ones(len(src), np.float32)
    zeros = 1 + rng.permutation(len(src) - 1)[:700]
    w[zeros] = 0.0
    keep = np.flatnonzero(w > 0).astype(np.int64)
    runs = {}
    for how in ("weights", "vlist"):
        with IcpEngine(0) as e:
            e.set_trim(fraction)
            e.set_target_mesh(verts, tris)
            e.set_source(src, vlist=keep if how == "vlist" else None, stride=1)
            if how == "weights":
                e.set_source_weights(w)
            e.set_matrices(mxa, mxb)
            runs[how] = []
            for _ in range(4):
                M, st = e.iterate(thresh=THRESH, target_d=1e-4)
                runs[how].append((M, st["K"], e.stat("trim_candidates"), e.stat("trim_kept"), e.stat("trim_cut"), e._history(1)[1][-1].copy(),
                                  e.matrix_world().copy()))
    for a, b in zip(runs["weights"], runs["vlist"]):
        print("|dM| %.3g, K %d / %d, candidates %d, kept %d, cut %.9g" % (np.max(np.abs(a[0] - b[0])), a[1], b[1], a[2], a[3], a[4]))
        assert a[2:5] == b[2:5] and 0 < a[3] < a[2]
        assert a[1] - b[1] == len(zeros) and b[1] == b[3]
        assert np.max(np.abs(a[0] - b[0])) <= TOL
        assert np.array_equal(a[5], b[5]) and np.array_equal(a[6], b[6])


@pytest.mark.gpu
@pytest.mark.parametrize("fraction", [0.5, AUTO])
@pytest.mark.parametrize("name", ["whole", "vlist_stride2"])
def test_gpu_make_pairs(orc, name, fraction):
    """A and B are exactly the reference's kept pairs in vlist order, K and dstats over them (the point residual)."""
    from object_alignment_amd.engine import IcpEngine
    mxa, mxb = usual_pose()
    tgt = upper_half()
    src, vlist, stride = whole(1000), None, 1
    if name == "vlist_stride2":
        src, vlist, stride = whole(2049), np.arange(2048, -1, -1, dtype=np.int64)[:1800], 2
    sel = src[selection(len(src), vlist, stride)]
    A, B, _, D = ref_pairs(orc, sel, mxa, mxb, tgt, tgt_normals=np.ones((len(tgt), 3), np.float32), thresh=THRESH)
    q, k, kq = cut_of(D, fraction)
    keep = D.astype(np.float32) <= q
    with IcpEngine(0) as e:
        e.set_metric("plane")                                       # (oa_make_pairs does not look at the metric)
        e.set_target(tgt)
        e.set_source(src, vlist=vlist, stride=stride)
        e.set_matrices(mxa, mxb)
        e.set_trim(fraction)
        for stats in (False, True):
            Ae, Be, ds = e.make_pairs(THRESH, calc_stats=stats)
            if fraction == AUTO:
                check_estimate(D, e.stat("trim_cut"))
            assert e.stat("trim_candidates") == kq == len(D) and np.float32(e.stat("trim_cut")) == q
            assert e.stat("trim_kept") == keep.sum() and k <= keep.sum() < kq
            assert Ae.shape == (3, int(keep.sum()))
            assert np.array_equal(Ae.T, A[keep]) and np.array_equal(Be.T, B[keep])
        assert abs(ds[0] - float(np.mean(D[keep]))) <= 1e-12 and abs(ds[1] - float(np.std(D[keep]))) <= 1e-12
        e.set_trim(0.0)
        A0, _, _ = e.make_pairs(THRESH)
        assert np.array_equal(A0.T, A) and e.stat("trim_candidates") == 0.0


# ------------------------------------------------------------------------------------------------ GPU: off, stability, end to end
RUN_FIELDS = ("step_M", "step_new", "step_K", "step_stats", "step_trans", "matrix_world")


def _loop(e, metric, n_src, iters=8):
    src, sn, verts, tris, mxa, mxb = G.table_case()
    e.set_metric(metric)
    e.set_target_mesh(verts, tris)
    e.set_source(src[:n_src], stride=1)
    e.set_source_normals(sn[:n_src])
    e.set_matrices(mxa, mxb)
    return e.run(iters=iters, thresh=THRESH, target_d=1e-4, early_exit=False)


@pytest.mark.gpu
@pytest.mark.parametrize("n_src", [513, 5000])
@pytest.mark.parametrize("metric", METRICS)
def test_gpu_off_means_off(metric, n_src):
    """set_trim(0.5), a loop, set_trim(0): the next 8-iteration loop returns the bits of a context that never heard of it."""
    from object_alignment_amd.engine import IcpEngine
    with IcpEngine(0) as e:
        plain = _loop(e, metric, n_src)
        assert e.stat("trim") == 0.0 and e.stat("trim_candidates") == 0.0
    with IcpEngine(0) as e:
        e.set_trim(0.5)
        visit = _loop(e, metric, n_src, iters=3)
        assert 0 < e.stat("trim_kept") < e.stat("trim_candidates")
        e.set_trim(0)
        assert e.stat("trim_candidates") == 0.0
        back = _loop(e, metric, n_src)
    assert not np.array_equal(visit.step_M[0], plain.step_M[0])
    for name in RUN_FIELDS:
        assert np.array_equal(getattr(plain, name), getattr(back, name)), name


@pytest.mark.gpu
def test_gpu_estimated_share_bitwise_stability():
    """The estimated mode's 8-iteration loop, twice on one context and once on a fresh one: identical history bits."""
    from object_alignment_amd.engine import IcpEngine
    runs = []
    with IcpEngine(0) as e:
        e.set_trim(AUTO)
        for _ in range(2):
            runs.append((_loop(e, "point", 5000), e.stat("trim_candidates"), e.stat("trim_kept"), e.stat("trim_cut")))
    with IcpEngine(0) as e:
        e.set_trim(AUTO)
        runs.append((_loop(e, "point", 5000), e.stat("trim_candidates"), e.stat("trim_kept"), e.stat("trim_cut")))
    assert runs[0][0].iters_done == 8 and 0 < runs[0][2] < runs[0][1]
    for r in runs[1:]:
        assert r[1:] == runs[0][1:]
        for name in RUN_FIELDS:
            assert np.array_equal(getattr(r[0], name), getattr(runs[0][0], name)), name


@pytest.mark.gpu
def test_gpu_end_to_end_whole_model_onto_half_scan():
    """The table's case through IcpAlign, 60 iterations: trim="auto" and trim=0.5 each end at a translation error <= 2 x the numpy
    loop's own figure + 1e-6, and below a quarter of the plain engine loop's."""
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings
    mxa, mxb = usual_pose()
    src, tgt = whole(3000), upper_half()
    te = {}
    with IcpEngine(0) as e:
        for trim in (AUTO, 0.5, 0.0):
            st = IcpSettings(icp_iterations=60, sample_fraction=1, min_start=THRESH, trim=trim)
            r = IcpAlign(st, engine=e).run(src, tgt, mxa, mxb, early_exit=False)
            assert r.iters_done == 60 and e.stat("trim") == (-1.0 if trim == AUTO else trim)
            te[trim] = translation_error(r.matrix_world)
    ref = {trim: numpy_loop(trim)[0] for trim in (AUTO, 0.5)}
    print("translation error: estimated %.4g (numpy %.4g), trim 0.5 %.4g (numpy %.4g), plain %.4g" % (te[AUTO], ref[AUTO], te[0.5], ref[0.5], te[0.0]))
    for trim in (AUTO, 0.5):
        assert te[trim] <= 2.0 * ref[trim] + 1e-6
        assert te[trim] < 0.25 * te[0.0]


# ------------------------------------------------------------------------------------------------ GPU: refusals
@pytest.mark.gpu
def test_gpu_refusals_leave_the_context_usable():
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    mxa, mxb = usual_pose()
    src, tgt = whole(3000), upper_half()

    def plain_loop_ok(e, shards=False):
        e.set_trim(0)
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
        e.set_trim(0.75, 0.3, 3.0)
        for args in ((-0.5,), (1.5,), (float("nan"),), (float("inf"),), (-2.0,), (AUTO, 0.0), (AUTO, 1.5), (AUTO, float("nan")),
                     (0.5, 0.3, 0.25), (0.5, 0.3, 8.5), (AUTO, 0.3, float("nan")), (AUTO, 0.3, float("inf"))):
            with pytest.raises(_capi.OaError, match="oa_set_trim") as ei:
                e.set_trim(*args)
            assert ei.value.code == _capi.OA_E_BAD_ARG
            assert e.stat("trim") == 0.75                           # the setting in force stays
        e.set_trim(0.5, float("nan"))                               # (a fixed share: fraction_min is not looked at)
        e.set_trim(AUTO, 1.0, 0.5)
        e.set_trim(AUTO, 0.3, 8.0)
        for fraction in (0.5, AUTO):
            e.set_trim(fraction)
            e.set_matrices(mxa, mxb)
            with pytest.raises(_capi.OaError, match="oa_set_trim") as ei:
                e.run_begin(iters=5)
            assert ei.value.code == _capi.OA_E_STATE
            plain_loop_ok(e)
            e.run_begin(iters=5)                                    # the same call, after set_trim(0)
            e.set_trim(fraction)
            e.set_source(src, stride=1, shard_index=0, shard_count=2)
            e.set_matrices(mxa, mxb)
            for call in (lambda: e.run(iters=5), lambda: e.iterate(), lambda: e.make_pairs(THRESH)):
                with pytest.raises(_capi.OaError, match="oa_set_trim") as ei:
                    call()
                assert ei.value.code == _capi.OA_E_STATE and "shard" in str(ei.value)
            e.set_trim(0)
            e.set_matrices(mxa, mxb)
            assert e.run(iters=5, thresh=THRESH, target_d=0.01, early_exit=False).iters_done == 5      # the shard's own loop
            plain_loop_ok(e, shards=True)
    with IcpEngine(devices=[0, 0]) as m:
        m.set_target(tgt)
        m.set_source(src, stride=1)
        m.set_matrices(mxa, mxb)
        m.set_trim(0.5)
        assert m.stat("trim") == 0.5
        for call in (lambda: m.run(iters=5), lambda: m.iterate(), lambda: m.make_pairs(THRESH)):
            with pytest.raises(_capi.OaError, match="oa_set_trim") as ei:
                call()
            assert ei.value.code == _capi.OA_E_STATE and "single-device" in str(ei.value)
        plain_loop_ok(m)
        m.make_pairs(THRESH)
