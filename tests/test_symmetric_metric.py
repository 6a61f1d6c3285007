"""Symmetric ICP (Rusinkiewicz, "A Symmetric Objective Function for ICP", SIGGRAPH 2019): oa_set_metric(OA_METRIC_SYMMETRIC),
oa_symmetric_step, IcpEngine.set_metric("symmetric") / symmetric_step, IcpSettings(metric="symmetric"),
IcpAlign.run(..., source_normals=array | "estimate").

The CPU reference of the step lives here (symm_step): numpy, fp64 -- every pair its own n = (n_b + s n_a) / 2, r and row J in the
contract's operation order, the pairs' J J^T and J r added one after the other in pair order (numpy.cumsum), or in the reverse
order --, numpy.linalg.eigh with the 1e-10 x lambda_max cut, and the step composed from 4 x 4 matrix products,
M = T(c) R T(t) R T(-c).  Pairs, loop, cases and bounds are tests/test_gicp_metric.py's: the engine is held to the reference one
step at a time, each from the device's own matrix_world.

PYTHONPATH=. python tests/test_symmetric_metric.py rewrites tests/golden/symm_table_case.json from this file's reference loop.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from object_alignment_amd import synth
import test_gicp_metric as G
from test_gicp_metric import (TOL, POSE, psi, ref_loop, ref_pairs, res_scale_of, scaled_base, selection, shape_case, table_case,
                              ulp_diff32, unit_rows, pose_error, random_pairs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "symm_table_case.json")
SYMMETRIC = 3
THRESH = 0.5


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build_hip()
    return g


# ------------------------------------------------------------------------------------------------ the reference
def symm_terms(a, b, n_a, n_b, c):
    """(n, r, J) of the pairs (a, b) with unit normals (n_a, n_b) about the pivot c, in the contract's order: s from the
    left-to-right sum n_a . n_b (an exact 0 counts as +1), n = (n_b + s n_a) / 2, r = n . (a' - b') left to right,
    J = [(a' + b') x n, n]."""
    a, b, n_a, n_b = (np.asarray(x, np.float64) for x in (a, b, n_a, n_b))
    ap, bp = a - c, b - c
    dot = (n_a[:, 0] * n_b[:, 0] + n_a[:, 1] * n_b[:, 1]) + n_a[:, 2] * n_b[:, 2]
    s = np.where(dot < 0.0, -1.0, 1.0)[:, None]
    n = 0.5 * (n_b + s * n_a)
    e, m = ap - bp, ap + bp
    r = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
    J = np.concatenate([np.stack([m[:, 1] * n[:, 2] - m[:, 2] * n[:, 1], m[:, 2] * n[:, 0] - m[:, 0] * n[:, 2],
                                  m[:, 0] * n[:, 1] - m[:, 1] * n[:, 0]], axis=1), n], axis=1)
    return n, r, J


def trans4(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def symm_compose(x, c):
    """M = T(c) R T(t) R T(-c): theta = atan(|a~|), R = exp(theta [a~ / |a~|]x), t = t~ cos(theta); |a~| = 0: R = I, t = t~."""
    at, tt = np.asarray(x[:3], np.float64), np.asarray(x[3:], np.float64)
    u = float(np.linalg.norm(at))
    R4 = np.eye(4)
    theta = 0.0
    if u > 0.0:
        theta = float(np.arctan(u))
        R4[:3, :3] = G.rodrigues(at * (theta / u))
    return trans4(c) @ R4 @ trans4(tt * np.cos(theta)) @ R4 @ trans4(-np.asarray(c, np.float64))


def solve6_symm(H, g, c):
    """test_gicp_metric.solve6 with the symmetric composition: the minimum-norm x of H x = -g -> (M, rank)."""
    lam, V = np.linalg.eigh(H)
    keep = lam > G.EIG_CUT * lam.max()
    x = -(V[:, keep] @ ((V[:, keep].T @ g) / lam[keep]))
    return symm_compose(x, np.asarray(c, np.float64)), int(keep.sum())


def symm_step(a, b, n_a, n_b, pivot, reverse=False, loss=None, scale=1.0, res_scale=1.0, w_vertex=None):
    """The step of the pairs -> (M 4x4, rank, r per pair, sum w).  w = w_vertex psi(res_scale |r|), else 1."""
    if len(a) < 3:
        raise ValueError("input arrays are of wrong shape or type")
    c = np.asarray(pivot, np.float64)
    _, r, J = symm_terms(a, b, n_a, n_b, c)
    w = np.ones(len(r))
    if loss is not None:
        w = psi(loss, res_scale * np.abs(r), scale)
    if w_vertex is not None:
        w = w * np.asarray(w_vertex, np.float64)
    Hk = w[:, None, None] * (J[:, :, None] * J[:, None, :])
    gk = w[:, None] * (J * r[:, None])
    if reverse:
        Hk, gk = Hk[::-1], gk[::-1]
    H, g = np.cumsum(Hk, axis=0)[-1], np.cumsum(gk, axis=0)[-1]
    if not w.sum() > 0.0:
        raise ValueError("input arrays are of wrong shape or type")
    M, rank = solve6_symm(H, g, c)
    return M, rank, r, float(w.sum())


def ref_step(orc, src_sel, sn_sel, mx1, mx2, tgt, loss=None, scale=1.0, w_sel=None, res_scale=None, keep=None, **kw):
    """test_gicp_metric.ref_step with symm_step in gicp_step's place.  keep(P, r_world) -> mask: a selection among the step's
    pairs (the trim's), applied before the step."""
    P = ref_pairs(orc, src_sel, sn_sel, mx1, mx2, tgt, **kw)
    c = np.asarray(src_sel, np.float32)[0].astype(np.float64)
    rs = res_scale_of(mx1) if res_scale is None else res_scale
    if keep is not None:
        k = keep(P, rs * np.abs(symm_terms(P["a"], P["b"], P["n_a"], P["n_b"], c)[1]))
        P = {name: v[k] for name, v in P.items()}
    wkw = dict(loss=loss, scale=scale, res_scale=rs, w_vertex=None if w_sel is None else np.asarray(w_sel, np.float32)[P["slot"]])
    M, rank, r, wsum = symm_step(P["a"], P["b"], P["n_a"], P["n_b"], c, **wkw)
    M_rev = symm_step(P["a"], P["b"], P["n_a"], P["n_b"], c, reverse=True, **wkw)[0]
    new_mat = M.astype(np.float32)
    return dict(M=M, M_rev=M_rev, new_mat=new_mat, mw=orc.mat4_mul(np.asarray(mx1, np.float32), new_mat), K=len(P["a"]),
                mean=float(np.mean(P["dist"])), std=float(np.std(P["dist"])), rank=rank, wsum=wsum, pairs=P, r=r)


def scaled_pose_case(factor):
    """table_case with its pose's rotation vector and translation multiplied by `factor`"""
    src, sn, verts, tris, _, mxb = table_case()
    P = synth.rigid4(synth.rotation_from_rotvec([factor * v for v in POSE["rotvec"]]), [factor * v for v in POSE["t"]], dtype=np.float64)
    return src, sn, verts, tris, np.linalg.inv(P).astype(np.float32), mxb


def metric_loops(orc, case, metrics=("symmetric", "plane", "gicp")):
    """the reference loop (thresh 0.5, target_d 1e-4) of each metric on `case` -> {metric: ref_loop's dict}"""
    src, sn, verts, tris, mxa, mxb = case
    piv = src[0].astype(np.float64)

    def plane_step(m):
        P = ref_pairs(orc, src, sn, m, mxb, verts, tris=tris, thresh=THRESH)
        new_mat = G.plane_solve(P["a"], P["b"], P["n_b"], piv)[0].astype(np.float32)
        return dict(new_mat=new_mat, mw=orc.mat4_mul(np.asarray(m, np.float32), new_mat), mean=float(np.mean(P["dist"])))

    steps = dict(symmetric=lambda m: ref_step(orc, src, sn, m, mxb, verts, tris=tris, thresh=THRESH),
                 gicp=lambda m: G.ref_step(orc, src, sn, m, mxb, verts, tris=tris, thresh=THRESH), plane=plane_step)
    return {name: ref_loop(orc, steps[name], mxa) for name in metrics}


def ellipsoid_pairs(K=2000, angle=0.5, seed=7):
    """Exact pairs on an ellipsoid (semi-axes 1 / 0.7 / 0.5): b and its normals on the surface, a = the same points and normals
    shifted and turned back by `angle` rad about a fixed axis -> (a, b, n_a, n_b, R) with b = R a + t."""
    rng = np.random.default_rng(seed)
    ax = np.array([1.0, 0.7, 0.5])
    u = unit_rows(rng.normal(size=(K, 3)))[0]
    b = u * ax
    n_b = unit_rows(b / (ax * ax))[0]
    R = synth.rotation_from_rotvec(list(angle * np.array([2.0, -1.0, 2.0]) / 3.0)).astype(np.float64)
    return (b - np.array(POSE["t"])) @ R, b, n_b @ R, n_b, R        # (rows: a_i = R^T (b_i - t), t the table case's shift)


# ------------------------------------------------------------------------------------------------ CPU
def test_symmetric_abi_and_bindings(built):
    """Fails without the feature: the header, the library, the bindings and the settings all name the symmetric metric."""
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings
    hdr = open(os.path.join(ROOT, "include", "oa_icp.h")).read()
    L = C.CDLL(os.path.join(ROOT, "object_alignment_amd", "liboa_icp.so"))
    LL = _capi.load()
    assert re.search(r"#define\s+OA_METRIC_SYMMETRIC\s+3\b", hdr)
    assert re.search(r"\bint\s+oa_symmetric_step\s*\(", hdr)
    assert "oa_symmetric_step" in _capi.SYMBOLS and hasattr(L, "oa_symmetric_step")
    assert len(LL.oa_symmetric_step.argtypes) == 8
    assert _capi.OA_METRIC_SYMMETRIC == SYMMETRIC and IcpEngine.METRICS["symmetric"] == SYMMETRIC
    assert callable(IcpEngine.symmetric_step)
    st = IcpSettings(metric="symmetric")
    assert st.metric == "symmetric" and IcpSettings().metric == "point"
    assert C.sizeof(_capi.Settings) == 32 and C.sizeof(_capi.Report) == 72
    # the bad string is refused before an engine is opened (there is no GPU here to open one on)
    z = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="source_normals"):
        IcpAlign(st).run(z, z, np.eye(4), np.eye(4), source_normals="bogus")
    # the add-on's enum got no item (DESIGN 3.13's reason: the operators do not read the align object's normals)
    addon = open(os.path.join(ROOT, "object_alignment_amd", "blender_addon.py")).read()
    assert '"symmetric"' not in addon


def test_reference_restatement():
    rng = np.random.default_rng(17)
    # r = 0 for arbitrary pairs of points on a unit sphere with their own normals, up to a quarter turn apart.  (Beyond it
    # n_a . n_b < 0 and the contract's s reads the pair as normals of opposite sign -- the price of the sign invariance below:
    # n = (q - p) / 2 and r = -|p - q|^2 / 2.  A pair of a converging loop is nowhere near a quarter turn.)
    p, q = unit_rows(rng.normal(size=(500, 3)))[0], unit_rows(rng.normal(size=(500, 3)))[0]
    far = np.einsum("ij,ij->i", p, q) < 0.0
    assert 100 < far.sum() < 400
    r_far = symm_terms(p[far], q[far], p[far], q[far], np.zeros(3))[1]
    assert np.allclose(r_far, -0.5 * np.einsum("ij,ij->i", p[far] - q[far], p[far] - q[far]), rtol=0, atol=1e-15)
    q[far] = -q[far]
    _, r, _ = symm_terms(p, q, p, q, np.zeros(3))
    print("sphere: max |r| %.3g over angles up to %.3g rad" % (np.max(np.abs(r)), np.max(np.arccos(np.einsum("ij,ij->i", p, q)))))
    assert np.max(np.abs(r)) <= 1e-15
    # n_a = n_b: |n| = 1 and r is the plane metric's
    a, b, n_a, n_b = random_pairs(400)
    c = a[0].copy()
    n, r, _ = symm_terms(a, b, n_b, n_b, c)
    e = (a - c) - (b - c)
    assert np.array_equal(n, n_b) and np.array_equal(r, (n_b[:, 0] * e[:, 0] + n_b[:, 1] * e[:, 1]) + n_b[:, 2] * e[:, 2])
    assert np.allclose(r, np.einsum("ij,ij->i", n_b, a - b), rtol=0, atol=1e-15)
    # |n|^2 = (1 + |cos|) / 2
    n = symm_terms(a, b, n_a, n_b, c)[0]
    assert np.allclose(np.einsum("ij,ij->i", n, n), 0.5 * (1.0 + np.abs(np.einsum("ij,ij->i", n_a, n_b))), rtol=0, atol=1e-15)
    # sign flips of arbitrary normals on either side: M bit for bit
    M = symm_step(a, b, n_a, n_b, c)[0]
    sa = np.where(rng.random(len(a)) < 0.5, -1.0, 1.0)[:, None]
    sb = np.where(rng.random(len(a)) < 0.5, -1.0, 1.0)[:, None]
    assert np.array_equal(symm_terms(a, b, n_a * sa, n_b, c)[0], symm_terms(a, b, n_a, n_b, c)[0])
    assert np.array_equal(symm_step(a, b, n_a * sa, n_b * sb, c)[0], M)
    # the order of the pairs
    M_rev = symm_step(a, b, n_a, n_b, c, reverse=True)[0]
    print("forward / reverse spread %.3g" % np.max(np.abs(M - M_rev)))
    assert np.max(np.abs(M - M_rev)) < TOL / 10
    # the composition: a pure translation, and the rotation split in two halves about the pivot
    assert np.allclose(symm_compose(np.array([0, 0, 0, 0.1, 0.2, 0.3]), c), trans4([0.1, 0.2, 0.3]), rtol=0, atol=1e-15)
    w = np.array([0.3, -0.2, 0.1])
    th = np.arctan(np.linalg.norm(w))
    Mc = symm_compose(np.concatenate([w, np.zeros(3)]), c)
    assert np.allclose(Mc[:3, :3], G.rodrigues(w / np.linalg.norm(w) * 2.0 * th), rtol=0, atol=1e-15)
    assert np.allclose(Mc[:3, :3] @ c + Mc[:3, 3], c, rtol=0, atol=1e-15)


def test_reference_ellipsoid_exact_pairs():
    """Exact pairs 0.5 rad apart: one symmetric step leaves less than a tenth of the plane step's error, two leave none."""
    a, b, n_a, n_b, _ = ellipsoid_pairs()
    err = {}
    for name in ("symmetric", "plane"):
        x, nx, errs = a.copy(), n_a.copy(), []
        for _ in range(2):
            c = x[0].copy()
            M = symm_step(x, b, nx, n_b, c)[0] if name == "symmetric" else G.plane_solve(x, b, n_b, c)[0]
            x, nx = x @ M[:3, :3].T + M[:3, 3], nx @ M[:3, :3].T
            errs.append(float(np.max(np.linalg.norm(x - b, axis=1))))
        err[name] = errs
    print("largest point error after one / two steps: symmetric %.3g / %.3g, plane %.3g / %.3g"
          % (err["symmetric"][0], err["symmetric"][1], err["plane"][0], err["plane"][1]))
    assert err["symmetric"][0] < 0.1 * err["plane"][0]
    assert err["symmetric"][1] < 1e-12


def reference_table_loop(orc):
    loops = metric_loops(orc, table_case())
    s = loops["symmetric"]
    return loops, dict(iters_done=int(s["iters_done"]), pose_error=pose_error(s["matrix_world"]), mean_dist=float(s["mean"]))


def test_reference_symmetric_loop_on_the_table_case(orc):
    """The yardstick itself: the reference's symmetric loop converges on DESIGN 3.9's case; its count, final pose error and mean
    distance are the fixture the GPU loop is held to.  The plane and GICP loops are printed beside it; no order is asserted."""
    src, sn, verts, tris, mxa, mxb = table_case()
    first = ref_step(orc, src, sn, mxa, mxb, verts, tris=tris, thresh=THRESH)
    print("first step: forward / reverse spread %.3g, rank %d" % (np.max(np.abs(first["M"] - first["M_rev"])), first["rank"]))
    assert np.max(np.abs(first["M"] - first["M_rev"])) < TOL / 10 and first["rank"] == 6
    loops, mine = reference_table_loop(orc)
    for name, o in loops.items():
        print("%s: %d iterations, pose error %.3g, mean distance %.3g" % (name, o["iters_done"], pose_error(o["matrix_world"]), o["mean"]))
    assert all(o["converged"] for o in loops.values())
    fx = json.load(open(FIXTURE))
    assert abs(mine["iters_done"] - fx["iters_done"]) <= 1
    assert mine["pose_error"] <= 2.0 * fx["pose_error"] + 1e-6 and fx["pose_error"] <= 2.0 * mine["pose_error"] + 1e-6


# ------------------------------------------------------------------------------------------------ GPU
def step_parity(orc, eng, src_sel, sn_sel, mxb, tgt, steps, thresh=THRESH, **kw):
    """test_gicp_metric.step_parity with this file's ref_step: `steps` steps of the engine against the reference, each from the
    device's own matrix_world.  The bound on |dM| is TOL, or -- where the reference's own forward / reverse spread exceeds
    TOL / 10 -- 100 x that spread (measured on the reference alone)."""
    res_scale = res_scale_of(eng.matrix_world())                   # the sequence of iterate() calls starts here
    for it in range(steps):
        mw = eng.matrix_world()
        ref = ref_step(orc, src_sel, sn_sel, mw, mxb, tgt, thresh=thresh, res_scale=res_scale, **kw)
        spread = float(np.max(np.abs(ref["M"] - ref["M_rev"])))
        tol = TOL if spread <= TOL / 10 else 100.0 * spread
        M, st = eng.iterate(thresh=thresh, target_d=1e-4)
        _, sN, _, _, _ = eng._history(1)
        dM = float(np.max(np.abs(M - ref["M"])))
        print("step %d: K %d / %d, |dM| %.3g (reference spread %.3g, bound %.3g), d mean %.3g, d std %.3g, new_mat ulps %.3g, rank %d / %d"
              % (it, st["K"], ref["K"], dM, spread, tol, abs(st["mean_dist"] - ref["mean"]), abs(st["std_dist"] - ref["std"]),
                 ulp_diff32(sN[-1], ref["new_mat"]), int(eng.stat("plane_rank")), ref["rank"]))
        assert st["K"] == ref["K"]
        assert dM <= tol
        assert abs(st["mean_dist"] - ref["mean"]) <= TOL and abs(st["std_dist"] - ref["std"]) <= TOL
        assert ulp_diff32(sN[-1], ref["new_mat"]) <= 1.0
        assert int(eng.stat("plane_rank")) == ref["rank"]
        if kw.get("loss") is not None or kw.get("w_sel") is not None:
            assert abs(eng.stat("weight_sum") - ref["wsum"]) <= 1e-9 * max(1.0, ref["wsum"])
    return ref


def open_table(e, mode=None):
    src, sn, verts, tris, mxa, mxb = table_case()
    e.set_metric("symmetric")
    if mode is not None:
        e.set_search_mode(mode)
    e.set_target_mesh(verts, tris)
    e.set_source(src, stride=1)
    e.set_source_normals(sn)
    e.set_matrices(mxa, mxb)
    return src, sn, verts, tris, mxa, mxb


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["surface", "vertex_normals", "scaled_base", "vlist_stride2", "normal_test", "mode_brute", "mode_grid",
                                  "mode_bvh"])
def test_gpu_symmetric_step_parity(orc, case):
    """Measured on an MI355X: every case holds all bounds over its 4 steps with new_mat equal bit for bit (this file's largest
    |dM|: 2.3e-15, at 262 145 points); no case's reference spread exceeded TOL / 10, so none took the widened bound."""
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    src, sn, verts, tris, mxa, mxb = table_case()
    vlist, stride, kw = None, 1, {}
    with IcpEngine(0) as e:
        e.set_metric("symmetric")
        assert e.stat("metric") == float(SYMMETRIC)
        if case.startswith("mode_"):
            e.set_search_mode(case[5:])
        if case == "scaled_base":
            B = scaled_base()
            mxa = (B @ mxa.astype(np.float64)).astype(np.float32)
            mxb = B.astype(np.float32)
        if case == "vertex_normals":
            tgt, tn = synth.bunny_surface_with_normals(20000)
            e.set_target(tgt)
            e.set_target_normals(tn)
            kw.update(tgt_normals=tn)
        else:
            tgt = verts
            e.set_target_mesh(verts, tris)
            kw.update(tris=tris)
        if case == "vlist_stride2":
            vlist, stride = np.arange(len(src) - 1, -1, -1, dtype=np.int64)[: 4000], 2
        e.set_source(src, vlist=vlist, stride=stride)
        sel = selection(len(src), vlist, stride)
        if case == "normal_test":
            e.set_normals(sn, None, max_angle_deg=60.0)                 # the test's array is the metric's
            kw.update(max_angle_deg=60.0)
        else:
            e.set_source_normals(sn)
        e.set_matrices(mxa, mxb)
        assert e.stat("metric") == float(SYMMETRIC)                 # survives the uploads and set_matrices
        step_parity(orc, e, src[sel], sn[sel], mxb, tgt, 4, **kw)
        assert e.stat("acc_path") == float(_capi.OA_ACC_PLANE)      # the plane kernel's row and epilogue


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 63, 64, 65, 511, 512, 513, 262145])
def test_gpu_symmetric_launch_shapes(orc, n):
    """K's minimum, the wave's and the workgroup's edges, and the first size past the 256 -> 512-thread switch."""
    from object_alignment_amd.engine import IcpEngine
    src, sn, tgt, tn, mxa, mxb = shape_case(n)
    with IcpEngine(0) as e:
        e.set_metric("symmetric")
        e.set_target(tgt)
        e.set_target_normals(tn)
        e.set_source(src, stride=1)
        e.set_source_normals(sn)
        e.set_matrices(mxa, mxb)
        ref = step_parity(orc, e, src, sn, mxb, tgt, 1, tgt_normals=tn)
        assert ref["K"] == n                                        # every slot of the launch carries a pair


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 65, 513])
def test_gpu_symmetric_step_from_pairs(K):
    """oa_symmetric_step against the numpy step: normals of any length and sign, some zero normals on each side."""
    from object_alignment_amd.engine import IcpEngine
    a, b, n_a, n_b = random_pairs(K + 4)
    rng = np.random.default_rng(K)
    la, lb = rng.uniform(0.2, 5.0, K + 4)[:, None], rng.uniform(0.2, 5.0, K + 4)[:, None]
    la[1::3] *= -1.0
    NA, NB = n_a * la, n_b * lb
    NA[[1, K + 2]] = 0.0                                            # (pair 0 stays: its point is the pivot either way)
    NB[[2, K + 3]] = 0.0
    ua, oka = unit_rows(NA)
    ub, okb = unit_rows(NB)
    ok = oka & okb
    assert int(ok.sum()) == K
    M_ref, rank, _, _ = symm_step(a[ok], b[ok], ua[ok], ub[ok], a[0])
    M_rev = symm_step(a[ok], b[ok], ua[ok], ub[ok], a[0], reverse=True)[0]
    spread = float(np.max(np.abs(M_ref - M_rev)))
    tol = TOL if spread <= TOL / 10 else 100.0 * spread
    with IcpEngine(0) as e:
        M = e.symmetric_step(a.T, b.T, NA.T, NB.T)
        print("K %d: |dM| %.3g (reference spread %.3g, bound %.3g), rank %d / %d" % (K, np.max(np.abs(M - M_ref)), spread, tol, int(e.stat("plane_rank")), rank))
        assert np.max(np.abs(M - M_ref)) <= tol
        assert int(e.stat("plane_rank")) == rank
        assert e.stat("metric") == 0.0                              # it does not look at the context's metric, nor set it
        with pytest.raises(ValueError, match="input arrays are of wrong shape or type"):
            e.symmetric_step(a[:2].T, b[:2].T, n_a[:2].T, n_b[:2].T)            # K = 2: OA_E_TOO_FEW_PAIRS
        with pytest.raises(ValueError, match="input arrays are of wrong shape or type"):
            e.symmetric_step(a[:4].T, b[:4].T, np.zeros((3, 4)), n_b[:4].T)     # no usable pair
        M2 = e.symmetric_step(a.T, b.T, NA.T, NB.T)
        assert np.array_equal(M, M2)


@pytest.mark.gpu
def test_gpu_symmetric_normal_signs_drop_out():
    from object_alignment_amd.engine import IcpEngine
    src, sn, _, _, mxa, mxb = table_case()
    tgt, tn = synth.bunny_surface_with_normals(20000)
    rng = np.random.default_rng(11)
    sg_s = np.where(rng.random(len(sn)) < 0.5, -1.0, 1.0).astype(np.float32)[:, None]
    sg_t = np.where(rng.random(len(tn)) < 0.5, -1.0, 1.0).astype(np.float32)[:, None]
    out = []
    for s_n, t_n in ((sn, np.asarray(tn, np.float32)), (sn * sg_s, np.asarray(tn, np.float32) * sg_t)):
        with IcpEngine(0) as e:
            e.set_metric("symmetric")
            e.set_target(tgt)
            e.set_target_normals(t_n)
            e.set_source(src, stride=1)
            e.set_source_normals(s_n)
            e.set_matrices(mxa, mxb)
            r = e.run(iters=3, thresh=THRESH, target_d=1e-4, early_exit=False)
            assert r.iters_done == 3
            out.append((r.step_M.copy(), r.matrix_world.copy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.gpu
def test_gpu_symmetric_dropped_pairs(orc):
    from object_alignment_amd.engine import IcpEngine
    src, sn, verts, tris, mxa, mxb = table_case()
    bad = sn.copy()
    bad[[0, 63, 64, 1000]] = 0.0
    bad[[5, 511]] = np.nan
    bad[700, 1] = np.nan
    bad[[6, 512]] = np.inf
    bad[4999, 2] = -np.inf
    bad_slots = [0, 63, 64, 1000, 5, 511, 700, 6, 512, 4999]
    with IcpEngine(0) as e:
        open_table(e)
        e.set_source_normals(bad)
        e.set_matrices(mxa, mxb)
        full = ref_pairs(orc, src, sn, mxa, mxb, verts, tris=tris, thresh=THRESH)["slot"]
        left = ref_pairs(orc, src, bad, mxa, mxb, verts, tris=tris, thresh=THRESH)["slot"]
        gone = sorted(set(full) - set(left))
        assert gone == sorted(set(bad_slots) & set(full)) and len(gone) >= 5      # the reference drops exactly the marked slots
        step_parity(orc, e, src, bad, mxb, verts, 2, tris=tris)
        # nothing but zero normals: no pair is left
        e.set_source_normals(np.zeros_like(sn))
        e.set_matrices(mxa, mxb)
        with pytest.raises(ValueError, match="input arrays are of wrong shape or type"):
            e.iterate(thresh=THRESH, target_d=1e-4)
        e.set_source_normals(sn)
        e.set_matrices(mxa, mxb)
        step_parity(orc, e, src, sn, mxb, verts, 1, tris=tris)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["huber", "tukey", "cauchy", "vertex_weights"])
def test_gpu_symmetric_weighted_step_parity(orc, case):
    from object_alignment_amd.engine import IcpEngine
    kw = {}
    with IcpEngine(0) as e:
        src, sn, verts, tris, mxa, mxb = open_table(e)
        kw.update(tris=tris)
        if case == "vertex_weights":
            wv = np.random.default_rng(2).uniform(0.0, 2.0, len(src)).astype(np.float32)
            wv[::7] = 0.0
            e.set_source_weights(wv)
            kw.update(w_sel=wv)
        else:
            scale = {"huber": 0.01, "tukey": 0.05, "cauchy": 0.01}[case]       # inside the residuals of the first steps
            e.set_robust(case, scale)
            kw.update(loss=case, scale=scale)
        e.set_matrices(mxa, mxb)
        ref = step_parity(orc, e, src, sn, mxb, verts, 2, **kw)
        if case != "vertex_weights":
            assert ref["wsum"] < 0.98 * ref["K"]                    # the loss bites at this scale


@pytest.mark.gpu
@pytest.mark.parametrize("fraction", [0.6, "auto"])
def test_gpu_symmetric_trimmed_step(orc, fraction):
    """One trimmed step: the candidates, the survivors and the cut are test_trimmed's rule on the symmetric residual (fixed share:
    the cut's bits; estimated share: check_estimate's near-tie rule, then the reference from the engine's cut)."""
    import test_trimmed as T
    from object_alignment_amd.engine import IcpEngine
    with IcpEngine(0) as e:
        e.set_trim(fraction)
        src, sn, verts, tris, mxa, mxb = open_table(e)
        seen = {}

        def keep(P, res):
            seen.update(res=res)
            if fraction == "auto":
                return np.ones(len(res), bool)                      # (the cut comes from the engine below)
            q, k, kq = T.fixed_cut(res, fraction)
            rho = np.sort(res.astype(np.float32))
            assert k == kq or rho[k] > q, "the reference's cut is tied: choose another case"
            seen.update(q=q, kq=kq)
            return T.trim_keep(res, np.ones(len(res), bool), q)

        ref = ref_step(orc, src, sn, mxa, mxb, verts, tris=tris, thresh=THRESH, keep=keep)
        M, st = e.iterate(thresh=THRESH, target_d=1e-4)
        cand, kept, cut = int(e.stat("trim_candidates")), int(e.stat("trim_kept")), e.stat("trim_cut")
        if fraction == "auto":
            q_ref, k_ref, kq = T.check_estimate(seen["res"], cut)
            ref = ref_step(orc, src, sn, mxa, mxb, verts, tris=tris, thresh=THRESH,
                           keep=lambda P, res: T.trim_keep(res, np.ones(len(res), bool), np.float32(cut)))
            assert kq == len(seen["res"])
        else:
            assert np.float32(cut) == seen["q"] and float(np.float32(cut)) == cut, "the cut's bits"
            assert seen["kq"] == len(seen["res"]) and ref["K"] < seen["kq"]           # the trim had something to say
        dM = float(np.max(np.abs(M - ref["M"])))
        print("trim %r: candidates %d / %d, kept %d / %d, cut %.9g, |dM| %.3g" % (fraction, cand, len(seen["res"]), kept, ref["K"], cut, dM))
        assert np.max(np.abs(ref["M"] - ref["M_rev"])) <= TOL / 10
        assert cand == len(seen["res"]) and kept == ref["K"] == st["K"]
        assert dM <= TOL
        assert abs(st["mean_dist"] - ref["mean"]) <= TOL and abs(st["std_dist"] - ref["std"]) <= TOL
        assert ulp_diff32(e._history(1)[1][-1], ref["new_mat"]) <= 1.0
        assert int(e.stat("plane_rank")) == ref["rank"]


@pytest.mark.gpu
def test_gpu_symmetric_estimated_robust_scale(orc):
    """One step with the loss's scale from the step's own residuals (GICP refuses this; this metric does not): the scale is
    test_robust_auto_scale's order statistic of the symmetric residual -- within 1 float32 ulp of q, that file's rule for a
    residual formed in fp64 -- then the step with the device's scale in the reference."""
    import test_robust_auto_scale as A
    from object_alignment_amd.engine import IcpEngine
    m, p = A.mad_tuning()["tukey"], 0.5
    with IcpEngine(0) as e:
        e.set_robust("tukey", m)
        e.set_robust_auto(p, A.FLOOR)
        src, sn, verts, tris, mxa, mxb = open_table(e)
        plain = ref_step(orc, src, sn, mxa, mxb, verts, tris=tris, thresh=THRESH)
        res = res_scale_of(mxa) * np.abs(plain["r"])
        c_ref = A.auto_c(res, None, m, p, A.FLOOR)
        M, st = e.iterate(thresh=THRESH, target_d=1e-4)
        c_dev = e.stat("robust_scale")
        print("scale %.17g / %.17g" % (c_dev, c_ref))
        assert c_ref > A.FLOOR and ulp_diff32(np.float32(c_dev / m), np.float32(c_ref / m)) <= 1.0
        ref = ref_step(orc, src, sn, mxa, mxb, verts, tris=tris, thresh=THRESH, loss="tukey", scale=c_dev)
        dM = float(np.max(np.abs(M - ref["M"])))
        print("K %d / %d, |dM| %.3g, sum w %.17g / %.17g" % (st["K"], ref["K"], dM, e.stat("weight_sum"), ref["wsum"]))
        assert np.max(np.abs(ref["M"] - ref["M_rev"])) <= TOL / 10
        assert st["K"] == ref["K"] and dM <= TOL
        assert ulp_diff32(e._history(1)[1][-1], ref["new_mat"]) <= 1.0
        assert abs(e.stat("weight_sum") - ref["wsum"]) <= 1e-9 * ref["wsum"] and ref["wsum"] < 0.98 * ref["K"]


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["reciprocal", "boundary"])
def test_gpu_symmetric_with_reciprocal_and_boundary(orc, what, tmp_path):
    """One step with the verdict bytes written by the reciprocal check / the boundary rejection, on test_boundary's cloud case (the
    whole model onto the half scan): the reference step over the pairs test_reciprocal's / test_boundary's rule leaves."""
    import test_boundary as B
    from object_alignment_amd.engine import IcpEngine
    d = dict(B.step_case("gicp_cloud"), metric="symmetric")
    src, sn, tgt, tn, mxa, mxb = d["src"], d["sn"], d["tgt"], d["tn"], d["mxa"], d["mxb"]
    if what == "reciprocal":
        select = lambda P, res: B.recip_keep(orc, P["a"], P["b"], src)
    else:
        vmask, emask = B.masks_of(d)
        select = lambda P, res: ~B.rim_slots(orc, src, mxa, mxb, tgt, None, vmask, emask, tmp_path)[P["slot"]]
    ref = ref_step(orc, src, sn, mxa, mxb, tgt, tgt_normals=tn, thresh=B.THRESH, keep=select)
    plain = ref_step(orc, src, sn, mxa, mxb, tgt, tgt_normals=tn, thresh=B.THRESH)
    with IcpEngine(0) as e:
        if what == "reciprocal":
            e.set_reciprocal(True)
        else:
            e.set_reject_boundary(True)
        B.open_step_case(e, d)
        M, st = e.iterate(thresh=B.THRESH, target_d=1e-4)
        rejected = int(e.stat("recip_rejected" if what == "reciprocal" else "boundary_rejected"))
        dM = float(np.max(np.abs(M - ref["M"])))
        print("%s: K %d / %d of %d, rejected %d, |dM| %.3g" % (what, st["K"], ref["K"], plain["K"], rejected, dM))
        assert np.max(np.abs(ref["M"] - ref["M_rev"])) <= TOL / 10
        assert st["K"] == ref["K"] and 0 < rejected == plain["K"] - ref["K"]
        assert dM <= TOL
        assert abs(st["mean_dist"] - ref["mean"]) <= TOL and abs(st["std_dist"] - ref["std"]) <= TOL
        assert ulp_diff32(e._history(1)[1][-1], ref["new_mat"]) <= 1.0
        assert int(e.stat("plane_rank")) == ref["rank"]


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["point", "plane"])
def test_gpu_other_metrics_unmoved_by_a_visit_to_symmetric(metric):
    from object_alignment_amd.engine import IcpEngine
    src, sn, verts, tris, mxa, mxb = table_case()

    def history(e):
        e.set_matrices(mxa, mxb)
        return e.run(iters=10, thresh=THRESH, target_d=0.01, early_exit=False)

    runs = []
    for visit in ("never", "metric_only", "with_normals"):
        with IcpEngine(0) as e:
            if visit != "never":
                e.set_metric("symmetric")
            e.set_target_mesh(verts, tris)
            e.set_source(src, stride=1)
            if visit == "with_normals":
                e.set_source_normals(sn)
                e.set_matrices(mxa, mxb)
                assert e.run(iters=2, thresh=THRESH, target_d=0.01, early_exit=False).iters_done == 2      # a symmetric loop in between
            e.set_metric(metric)
            runs.append(history(e))
    for other in runs[1:]:
        for name in ("step_M", "step_new", "step_K", "step_stats", "step_trans", "matrix_world"):
            assert np.array_equal(getattr(runs[0], name), getattr(other, name)), name


@pytest.mark.gpu
def test_gpu_symmetric_loop_on_the_table_case():
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings
    src, sn, verts, tris, mxa, mxb = table_case()
    fx = json.load(open(FIXTURE))
    with IcpEngine(0) as e:
        res = IcpAlign(IcpSettings(metric="symmetric", sample_fraction=1, target_d=1e-4), engine=e).run(
            src, verts, mxa, mxb, source_normals=sn, target_tris=tris)
        assert e.stat("metric") == float(SYMMETRIC) and e.stat("acc_path") == float(_capi.OA_ACC_PLANE)
        again = IcpAlign(IcpSettings(metric="symmetric", sample_fraction=1, target_d=1e-4), engine=e).run(
            src, verts, mxa, mxb, source_normals=sn, target_tris=tris)
        # the pose x 4 (0.68 rad): printed for DESIGN 3.20, not asserted
        _, _, _, _, mxa4, _ = scaled_pose_case(4.0)
        counts = {}
        for metric in ("symmetric", "plane"):
            r4 = IcpAlign(IcpSettings(metric=metric, sample_fraction=1, target_d=1e-4), engine=e).run(
                src, verts, mxa4, mxb, source_normals=sn, target_tris=tris)
            counts[metric] = (r4.iters_done, pose_error(r4.matrix_world), bool(r4.converged))
    err = pose_error(res.matrix_world)
    print("symmetric loop: %d iterations (fixture %d), pose error %.3g (fixture %.3g), mean distance %.3g (fixture %.3g)"
          % (res.iters_done, fx["iters_done"], err, fx["pose_error"], res.mean_dist, fx["mean_dist"]))
    print("pose x 4: symmetric %d iterations (pose error %.3g, converged %s), plane %d iterations (pose error %.3g, converged %s)"
          % (counts["symmetric"] + counts["plane"]))
    assert res.converged
    assert abs(res.iters_done - fx["iters_done"]) <= 1
    assert err <= 2.0 * fx["pose_error"] + 1e-6
    assert np.array_equal(res.matrix_world, again.matrix_world) and res.iters_done == again.iters_done      # two runs, the same bits


@pytest.mark.gpu
def test_gpu_symmetric_loop_with_estimated_normals():
    """IcpAlign.run(source_normals="estimate") serves this metric as it serves "gicp": both sides' normals estimated, unoriented."""
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings
    src = synth.bunny_surface(2000, 0.5)
    tgt = synth.bunny_surface(8000)
    P = synth.rigid4(synth.rotation_from_rotvec(list(POSE["rotvec"])), list(POSE["t"]), dtype=np.float64)
    mxa, mxb = np.linalg.inv(P).astype(np.float32), np.eye(4, dtype=np.float32)
    with IcpEngine(0) as e:
        r = IcpAlign(IcpSettings(metric="symmetric", sample_fraction=1, target_d=1e-4), engine=e).run(
            src, tgt, mxa, mxb, source_normals="estimate", target_normals="estimate")
    print("estimated normals: %d iterations, mean_dist %.4g" % (r.iters_done, r.mean_dist))
    assert r.converged


@pytest.mark.gpu
def test_gpu_symmetric_refusals_leave_the_context_usable():
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    src, sn, verts, tris, mxa, mxb = table_case()

    def loop_ok(e):
        e.set_matrices(mxa, mxb)
        r = e.run(iters=3, thresh=THRESH, target_d=0.01)
        assert r.iters_done >= 1 and np.all(np.isfinite(r.matrix_world))

    def refused(e, code, match, call=None):
        with pytest.raises(_capi.OaError, match=match) as ei:
            (call or (lambda: e.run(iters=3, thresh=THRESH, target_d=0.01)))()
        assert ei.value.code == code

    with IcpEngine(0) as e:
        e.set_metric("symmetric")
        e.set_target_mesh(verts, tris)
        e.set_source(src, stride=1)
        e.set_matrices(mxa, mxb)
        refused(e, _capi.OA_E_STATE, "symmetric metric needs source normals")
        refused(e, _capi.OA_E_STATE, "symmetric metric needs source normals", lambda: e.iterate())
        e.set_source_normals(sn)
        loop_ok(e)
        refused(e, _capi.OA_E_BAD_ARG, "symmetric metric solves for a rigid step", lambda: e.run(iters=3, with_scale=True))
        refused(e, _capi.OA_E_BAD_ARG, "symmetric metric solves for a rigid step", lambda: e.iterate(with_scale=True))
        refused(e, _capi.OA_E_STATE, "symmetric metric runs on a single-device", lambda: e.run_begin(iters=3))
        loop_ok(e)
        # a vertex-mode target without normals
        e.set_target(verts)
        e.set_matrices(mxa, mxb)
        refused(e, _capi.OA_E_STATE, "symmetric metric needs target normals")
        e.set_target_mesh(verts, tris)
        loop_ok(e)
        with pytest.raises(_capi.OaError) as ei:
            e.set_metric(4)
        assert ei.value.code == _capi.OA_E_BAD_ARG
        assert e.stat("metric") == float(SYMMETRIC)
    with IcpEngine(devices=[0, 0]) as m:
        m.set_target_mesh(verts, tris)
        m.set_source(src, stride=1)
        m.set_source_normals(sn)
        m.set_matrices(mxa, mxb)
        m.set_metric("symmetric")
        refused(m, _capi.OA_E_STATE, "single-device")
        refused(m, _capi.OA_E_STATE, "single-device", lambda: m.iterate())
        m.set_metric("point")
        m.set_matrices(mxa, mxb)
        r = m.run(iters=3, thresh=THRESH, target_d=0.01)
        assert r.iters_done >= 1 and np.all(np.isfinite(r.matrix_world))


if __name__ == "__main__":
    from oracle import oracle
    oracle.build()
    _, fixture = reference_table_loop(oracle)
    with open(FIXTURE, "w") as f:
        json.dump(fixture, f)
    print(fixture)
