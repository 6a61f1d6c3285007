"""Robust pair weights (oa_set_robust: Huber / Tukey / Cauchy at a fixed scale) and per-vertex weights (oa_set_source_weights).

The CPU reference lives here: numpy, fp64 -- a weighted Kabsch step (weighted centroids, H = sum w b a^T - W cb ca^T, SVD with
the reflection fix) and the plane solve of tests/test_plane_metric.py with every pair's J J^T and J r multiplied by w -- on top
of the pairs that module's ref_pairs forms (the oracle's correspondences and float32 helpers: the engine's pairs bit for bit).
The pair weight is w = w_vertex * psi(r): r the float32-derived pair distance (point metric) or s |n . (a - b)| with
s = cbrt(|det mx_align[:3,:3]|) taken ONCE from the matrix the loop starts from (plane metric).  As in the plane tests the
engine is held to the reference one step at a time -- before every step its matrix_world goes to the reference -- the
reference is run over the pairs in forward and in reversed order, and a case only counts if those two agree to the tolerance.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from object_alignment_amd import synth
from test_plane_metric import (EIG_CUT, TOL, ref_pairs, rodrigues, scaled_base, selection, table_case, ulp_diff32)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSSES = ("huber", "tukey", "cauchy")
SCALE = 0.05                # the issue's c for the parity cases


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build_hip()
    return g


# ------------------------------------------------------------------------------------------------ the reference
def psi(loss, r, c):
    r = np.asarray(r, np.float64)
    if loss == "none":
        return np.ones_like(r)
    if loss == "huber":
        return np.where(r <= c, 1.0, c / np.maximum(r, 1e-300))
    if loss == "tukey":
        return np.where(r < c, (1.0 - (r / c) ** 2) ** 2, 0.0)
    if loss == "cauchy":
        return 1.0 / (1.0 + (r / c) ** 2)
    raise ValueError(loss)


def weighted_kabsch(a, b, w, c, reverse=False, scale=False):
    """a, b: K x 3, w: K, pivot c.  M (4 x 4, fp64) of the weighted least-squares rigid (or similarity) step a -> b."""
    a, b, w = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(w, np.float64)
    if len(a) < 3 or not w.sum() > 0.0:
        raise ValueError("input arrays are of wrong shape or type")
    if reverse:
        a, b, w = a[::-1], b[::-1], w[::-1]
    a, b = a - c, b - c
    W = w.sum()
    ca, cb = (w[:, None] * a).sum(0) / W, (w[:, None] * b).sum(0) / W
    a0, b0 = a - ca, b - cb
    H = b0.T @ (w[:, None] * a0)
    u, _, vh = np.linalg.svd(H)
    R = u @ vh
    if np.linalg.det(R) < 0.0:
        R = R - np.outer(u[:, 2], vh[2, :] * 2.0)
    if scale:
        R = R * np.sqrt((w * (b0 * b0).sum(1)).sum() / (w * (a0 * a0).sum(1)).sum())
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = (cb + c) - R @ (ca + c)
    return M


def weighted_plane_solve(a, b, n, w, c, reverse=False):
    """plane_solve of test_plane_metric with every pair's row and residual weighted: H = sum w J J^T, g = sum w J r.
    a, b, n as ref_pairs returns them (n unit)."""
    a, b, n, w = (np.asarray(x, np.float64) for x in (a, b, n, w))
    if len(a) < 3 or not w.sum() > 0.0:
        raise ValueError("input arrays are of wrong shape or type")
    if reverse:
        a, b, n, w = a[::-1], b[::-1], n[::-1], w[::-1]
    a, b = a - c, b - c
    r = np.einsum("ij,ij->i", n, a - b)
    J = np.concatenate([np.cross(a, n), n], axis=1)
    H, g = J.T @ (w[:, None] * J), J.T @ (w * r)
    lam, V = np.linalg.eigh(H)
    keep = lam > EIG_CUT * lam.max()
    x = -(V[:, keep] @ ((V[:, keep].T @ g) / lam[keep]))
    R = rodrigues(x[:3])
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = c + x[3:] - R @ c
    return M, int(keep.sum())


def kept_index(src_sel, A):
    """ref_pairs drops pairs without saying which: A's rows are rows of src_sel, in order -- walk both."""
    src64 = np.asarray(src_sel, np.float64)
    out, k = np.empty(len(A), np.int64), 0
    for i in range(len(A)):
        while not np.array_equal(src64[k], A[i]):
            k += 1
        out[i] = k
        k += 1
    return out


def world_scale(mx_align):
    """s of the plane residual: cbrt(|det|) of the float32 matrix the loop starts from, in fp64."""
    return float(np.cbrt(abs(np.linalg.det(np.asarray(mx_align, np.float32)[:3, :3].astype(np.float64)))))


def ref_step(orc, metric, loss, c, src_sel, wv_sel, mx1, mx2, tgt, s_world=1.0, **kw):
    """One weighted step from matrix_world mx1: dict(M, M_rev, new_mat, mw, K, W, mean, std, rank)."""
    if kw.get("tris") is None and kw.get("tgt_normals") is None:
        kw["tgt_normals"] = np.ones((len(tgt), 3), np.float32)          # (the point metric does not read them)
    pairs = kw.pop("pairs", ref_pairs)
    A, B, N, D = pairs(orc, src_sel, mx1, mx2, tgt, **kw)
    wv = np.ones(len(A)) if wv_sel is None else np.asarray(wv_sel, np.float32).astype(np.float64)[kept_index(src_sel, A)]
    piv = src_sel[0].astype(np.float64)
    if metric == "plane":
        w = wv * psi(loss, s_world * np.abs(np.einsum("ij,ij->i", N, A - B)), c)
        M, rank = weighted_plane_solve(A, B, N, w, piv)
        M_rev, _ = weighted_plane_solve(A, B, N, w, piv, reverse=True)
    else:
        w = wv * psi(loss, D, c)
        M, rank = weighted_kabsch(A, B, w, piv), 0
        M_rev = weighted_kabsch(A, B, w, piv, reverse=True)
    new_mat = M.astype(np.float32)
    return dict(M=M, M_rev=M_rev, new_mat=new_mat, mw=orc.mat4_mul(np.asarray(mx1, np.float32), new_mat), K=len(A),
                W=float(w.sum()), mean=float(np.mean(D)), std=float(np.std(D)), rank=rank)


def _mul_v3(M, P):
    """mat4_mul_vec3 of the oracle over an array: float32 products, accumulated in double in order, w = 1, rounded to float32."""
    M, P = np.asarray(M, np.float32), np.asarray(P, np.float32)
    out = np.empty_like(P)
    for r in range(3):
        acc = (M[r, 0] * P[:, 0]).astype(np.float64)
        acc = acc + (M[r, 1] * P[:, 1]).astype(np.float64)
        acc = acc + (M[r, 2] * P[:, 2]).astype(np.float64)
        acc = acc + np.float64(M[r, 3] * np.float32(1.0))
        out[:, r] = acc.astype(np.float32)
    return out


def fast_pairs(orc, src_sel, mx1, mx2, tgt, tris, thresh=0.5):
    """ref_pairs for a surface target without the normal-angle test, over arrays instead of point by point (a whole loop of the
    outlier case in seconds, not a minute).  test_reference_tukey_ends_closer_on_the_outlier_case holds it to ref_pairs."""
    mx1, mx2 = np.asarray(mx1, np.float32), np.asarray(mx2, np.float32)
    imx1, imx2 = orc.mat4_inverted(mx1), orc.mat4_inverted(mx2)
    src_sel, tgt = np.asarray(src_sel, np.float32), np.asarray(tgt, np.float32)
    w = _mul_v3(imx2, _mul_v3(mx1, src_sel))
    face, co1, _ = orc.nn_tri_brute(w, tgt, tris)
    ta, tb, tc = (tgt[np.asarray(tris)[face, k]] for k in range(3))
    e1, e2 = ta - tb, tb - tc
    tn = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                   e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1).astype(np.float32)
    wb = _mul_v3(mx2, co1)
    d = _mul_v3(mx2, w) - wb
    dist = np.sqrt(((d[:, 2] * d[:, 2]).astype(np.float64) + (d[:, 1] * d[:, 1]).astype(np.float64)) + (d[:, 0] * d[:, 0]).astype(np.float64))
    nl = (tn.astype(np.float64) @ imx2[:3, :3].astype(np.float64)) @ mx1[:3, :3].astype(np.float64)   # mx1^T (imx2^T tn)
    n2 = np.einsum("ij,ij->i", nl, nl)
    keep = (dist < thresh) & np.isfinite(n2) & (n2 > 0.0)
    return (src_sel[keep].astype(np.float64), _mul_v3(imx1, wb)[keep].astype(np.float64), nl[keep] / np.sqrt(n2[keep])[:, None],
            dist[keep])


def ref_loop(orc, metric, loss, c, src_sel, wv_sel, mx1, mx2, tgt, iters=50, target_d=1e-4, **kw):
    """The reference's loop (5-slot ring of step lengths against target_d) around the weighted step."""
    mx1 = np.asarray(mx1, np.float32).copy()
    s_world = world_scale(mx1)
    ring = [2.0 * target_d] * 5
    out = dict(iters_done=0, converged=False)
    for n in range(iters):
        s = ref_step(orc, metric, loss, c, src_sel, wv_sel, mx1, mx2, tgt, s_world=s_world, **kw)
        mx1 = s["mw"]
        ring[n % 5] = orc.vec3_length(s["new_mat"][:3, 3])
        out.update(iters_done=n + 1, matrix_world=mx1, mean=s["mean"])
        if all(t < target_d for t in ring):
            out["converged"] = True
            break
    return out


# ---- the outlier case (GPU test 10; CPU test 3 fixes its numbers) ----
OUT_SHIFT, OUT_C, OUT_TARGET_D = 0.2, 0.15, 1e-4


def outlier_case():
    """table_case with every tenth source point moved OUT_SHIFT along +x in align-local space: inside thresh = 0.5, so the
    unweighted loop takes the moved points for good ones.  The true pose of the others is matrix_world = identity."""
    src, verts, tris, mxa, mxb = table_case()
    src = np.array(src, np.float32)
    src[::10, 0] += np.float32(OUT_SHIFT)
    return src, verts, tris, mxa, mxb


def pose_error(matrix_world):
    """The loop's estimate of the pose P (mx_align = P^-1) is matrix_world @ P; its error against the known P is the motion
    (matrix_world @ P) @ P^-1 = matrix_world that is left over: rotation angle + length of the translation."""
    E = np.asarray(matrix_world, np.float64)
    ang = np.arccos(np.clip((np.trace(E[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))
    return float(ang + np.linalg.norm(E[:3, 3]))


@functools.lru_cache(maxsize=None)
def outlier_reference(loss):
    from oracle import oracle as orc
    orc.build()
    src, verts, tris, mxa, mxb = outlier_case()
    return ref_loop(orc, "point", loss, OUT_C, src, None, mxa, mxb, verts, iters=50, target_d=OUT_TARGET_D, tris=tris, thresh=0.5,
                    pairs=fast_pairs)


def recorded_outlier_reference():
    """tests/golden/robust_outlier_reference.npz: iterations, convergence and final matrix_world of outlier_reference("none") and
    ("tukey"), recorded once (two loops of 17 + 27 exhaustive searches take 20 s on the CPU);
    test_reference_tukey_ends_closer_on_the_outlier_case recomputes them and holds the file to the result."""
    return np.load(os.path.join(ROOT, "tests", "golden", "robust_outlier_reference.npz"))


# ------------------------------------------------------------------------------------------------ CPU
def test_robust_abi_and_bindings(built):
    """Fails without the feature: the header, the library, the bindings and the settings all name the loss and the weights."""
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators import icp_align
    from object_alignment_amd.operators.icp_align import IcpSettings
    hdr = open(os.path.join(ROOT, "include", "oa_icp.h")).read()
    assert re.search(r"\bint\s+oa_set_robust\s*\(\s*oa_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*double\s+\w+\s*\)", hdr)
    assert re.search(r"\bint\s+oa_set_source_weights\s*\(\s*oa_ctx\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*\)", hdr)
    for name, val in (("OA_LOSS_NONE", 0), ("OA_LOSS_HUBER", 1), ("OA_LOSS_TUKEY", 2), ("OA_LOSS_CAUCHY", 3),
                      ("OA_STAT_ROBUST_LOSS", 30), ("OA_STAT_WEIGHT_SUM", 31)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name
    L = C.CDLL(os.path.join(ROOT, "object_alignment_amd", "liboa_icp.so"))
    for fn in ("oa_set_robust", "oa_set_source_weights"):
        assert hasattr(L, fn), fn
        assert fn in _capi.SYMBOLS
    LL = _capi.load()
    assert LL.oa_set_robust.argtypes is not None and len(LL.oa_set_robust.argtypes) == 3
    assert LL.oa_set_source_weights.argtypes is not None and len(LL.oa_set_source_weights.argtypes) == 3
    assert (_capi.OA_LOSS_NONE, _capi.OA_LOSS_HUBER, _capi.OA_LOSS_TUKEY, _capi.OA_LOSS_CAUCHY) == (0, 1, 2, 3)
    assert IcpEngine.STATS["robust_loss"] == 30 and IcpEngine.STATS["weight_sum"] == 31
    assert hasattr(IcpEngine, "set_robust") and hasattr(IcpEngine, "set_source_weights")
    st = IcpSettings()
    assert st.robust_loss == "none" and st.robust_scale == 0.0
    assert callable(icp_align.apply_robust)
    assert C.sizeof(_capi.Settings) == 32 and C.sizeof(_capi.Report) == 72
    assert "OA_NSUMS 24" in hdr                                    # the multi-GPU exchange keeps its width


def test_apply_robust_hands_the_loss_over_every_time():
    from object_alignment_amd.operators.icp_align import IcpSettings, apply_robust

    class Eng:
        def __init__(self):
            self.calls = []

        def set_robust(self, loss, scale):
            self.calls.append((loss, scale))

    e = Eng()
    apply_robust(e, IcpSettings(robust_loss="tukey", robust_scale=0.15))
    apply_robust(e, IcpSettings())
    assert e.calls == [("tukey", 0.15), ("none", 0.0)]
    apply_robust(object(), IcpSettings())                            # an engine without set_robust counts as loss-none
    with pytest.raises(RuntimeError):
        apply_robust(object(), IcpSettings(robust_loss="huber", robust_scale=0.1))

    class Prefs:                                                    # the add-on's preference names
        icp_robust_loss, icp_robust_scale = "cauchy", 0.25

    apply_robust(e, Prefs())
    assert e.calls[-1] == ("cauchy", 0.25)


def test_reference_sanity(orc):
    """Passes without the feature: with all w = 1 the weighted Kabsch reference is the oracle's unweighted solve, the weighted
    plane solve is the plane tests' plane_solve, and the three psi are continuous at r = c."""
    from test_plane_metric import plane_solve
    rng = np.random.default_rng(11)
    a = rng.normal(size=(500, 3))
    R = synth.rotation_from_rotvec([0.2, -0.1, 0.15]).astype(np.float64)
    b = a @ R.T + np.array([0.1, -0.2, 0.05]) + 0.01 * rng.normal(size=a.shape)
    for scale in (False, True):
        M = weighted_kabsch(a, b * (1.3 if scale else 1.0), np.ones(len(a)), a[0], scale=scale)
        ref = orc.affine_matrix_from_points(a.T, (b * (1.3 if scale else 1.0)).T, shear=False, scale=scale, usesvd=True)
        assert np.max(np.abs(M - ref)) < 1e-12
    assert np.max(np.abs(weighted_kabsch(a, b, np.ones(len(a)), a[0]) - weighted_kabsch(a, b, np.ones(len(a)), a[0], reverse=True))) < 1e-12
    # doubling every weight changes nothing; a zero weight is the pair left out
    w = rng.uniform(0.0, 2.0, len(a))
    w[::7] = 0.0
    assert np.max(np.abs(weighted_kabsch(a, b, w, a[0]) - weighted_kabsch(a, b, 2.0 * w, a[0]))) < 1e-12
    assert np.max(np.abs(weighted_kabsch(a, b, w, a[0]) - weighted_kabsch(a[w > 0], b[w > 0], w[w > 0], a[0]))) < 1e-12
    n = rng.normal(size=a.shape)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    Mp, rank = weighted_plane_solve(a, b, n, np.ones(len(a)), a[0])
    Mr, rrank = plane_solve(a, b, n, a[0])
    assert np.max(np.abs(Mp - Mr)) < 1e-12 and rank == rrank == 6
    c = 0.05
    for loss in LOSSES:
        lo, at, hi = (float(psi(loss, r, c)) for r in (c * (1.0 - 1e-12), c, c * (1.0 + 1e-12)))
        assert abs(lo - at) < 1e-10 and abs(hi - at) < 1e-10, loss
        assert float(psi(loss, 0.0, c)) == 1.0
        assert float(psi(loss, 1e30, 1e30)) == (0.0 if loss == "tukey" else (0.5 if loss == "cauchy" else 1.0))
    assert float(psi("huber", 0.49, 1e30)) == 1.0                   # GPU test 7a: every w is exactly 1


def test_reference_tukey_ends_closer_on_the_outlier_case(orc):
    """The yardstick of the GPU outlier test, on the CPU reference loop alone: with every tenth point moved 0.2 along +x the
    Tukey loop (c = 0.15) ends closer to the true pose than the unweighted loop; both converge."""
    src, verts, tris, mxa, mxb = outlier_case()
    for x, y in zip(fast_pairs(orc, src, mxa, mxb, verts, tris), ref_pairs(orc, src, mxa, mxb, verts, tris=tris)):
        assert x.shape == y.shape and np.max(np.abs(x - y)) < 1e-15     # (A, B and the distances bit for bit; the normals to rounding)
    for k in (0, 1, 3):
        assert np.array_equal(fast_pairs(orc, src, mxa, mxb, verts, tris)[k], ref_pairs(orc, src, mxa, mxb, verts, tris=tris)[k])
    plain, tukey = outlier_reference("none"), outlier_reference("tukey")
    rec = recorded_outlier_reference()                              # what the GPU test reads instead of running these loops again
    for loss, ref in (("none", plain), ("tukey", tukey)):
        assert int(rec[loss + "_iters"]) == ref["iters_done"] and bool(rec[loss + "_converged"]) == ref["converged"]
        assert np.max(np.abs(rec[loss + "_matrix_world"].astype(np.float64) - ref["matrix_world"].astype(np.float64))) < 1e-6
    print("unweighted: %d iterations, pose error %.4g; tukey: %d iterations, pose error %.4g"
          % (plain["iters_done"], pose_error(plain["matrix_world"]), tukey["iters_done"], pose_error(tukey["matrix_world"])))
    assert plain["converged"] and tukey["converged"]
    assert pose_error(tukey["matrix_world"]) < pose_error(plain["matrix_world"])


# ------------------------------------------------------------------------------------------------ GPU
def step_parity(orc, eng, metric, loss, c, src_sel, wv_sel, mxa, mxb, tgt, steps, **kw):
    s_world = world_scale(mxa)
    for it in range(steps):
        mw = eng.matrix_world()
        ref = ref_step(orc, metric, loss, c, src_sel, wv_sel, mw, mxb, tgt, s_world=s_world, **kw)
        assert np.max(np.abs(ref["M"] - ref["M_rev"])) < TOL, "the case is ill-conditioned for the reference itself"
        M, st = eng.iterate(thresh=kw.get("thresh", 0.5), target_d=1e-4)
        _, sN, _, _, _ = eng._history(1)
        dM, W = float(np.max(np.abs(M - ref["M"]))), eng.stat("weight_sum")
        print("step %d: K %d / %d, |dM| %.3g, d mean %.3g, d std %.3g, new_mat ulps %.3g, sum w %.17g / %.17g"
              % (it, st["K"], ref["K"], dM, abs(st["mean_dist"] - ref["mean"]), abs(st["std_dist"] - ref["std"]),
                 ulp_diff32(sN[-1], ref["new_mat"]), W, ref["W"]))
        assert st["K"] == ref["K"]
        assert dM <= TOL
        assert abs(st["mean_dist"] - ref["mean"]) <= TOL and abs(st["std_dist"] - ref["std"]) <= TOL
        assert ulp_diff32(sN[-1], ref["new_mat"]) <= 1.0
        assert abs(W - ref["W"]) <= 1e-9 * ref["W"]
        if metric == "plane":
            assert int(eng.stat("plane_rank")) == ref["rank"]


def vertex_weights(n, seed=5):
    """random weights in [0, 2], a tenth of them exactly 0"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.0, 2.0, n).astype(np.float32)
    w[rng.permutation(n)[: n // 10]] = 0.0
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("case", ["surface", "vertex", "scaled_base", "vlist_stride2", "mode_brute", "mode_grid", "mode_bvh",
                                  "vertex_weights"])
def test_gpu_point_step_parity(orc, case, loss):
    from object_alignment_amd.engine import IcpEngine
    src, verts, tris, mxa, mxb = table_case()
    steps, vlist, stride, wv, kw = 4, None, 1, None, dict(thresh=0.5)
    with IcpEngine(0) as e:
        e.set_robust(loss, SCALE)
        assert e.stat("robust_loss") == float(IcpEngine.LOSSES[loss])
        if case.startswith("mode_"):
            e.set_search_mode(case[5:])
            steps = 3
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
        assert e.stat("robust_loss") == float(IcpEngine.LOSSES[loss])          # survives the uploads and set_matrices
        step_parity(orc, e, "point", loss, SCALE, np.asarray(src, np.float32)[sel], None if wv is None else wv[sel], mxa, mxb, tgt,
                    steps, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("case", ["surface", "scaled_base", "vertex_normals"])
def test_gpu_plane_step_parity_weighted(orc, case, loss):
    from object_alignment_amd.engine import IcpEngine
    src, verts, tris, mxa, mxb = table_case()
    kw = dict(thresh=0.5)
    with IcpEngine(0) as e:
        e.set_metric("plane")
        e.set_robust(loss, SCALE)
        if case == "scaled_base":                                   # |det mx_align| = 1.1: the factor s
            B = scaled_base()
            mxa = (B @ mxa.astype(np.float64)).astype(np.float32)
            mxb = B.astype(np.float32)
            assert abs(world_scale(mxa) - 1.0) > 0.01
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
        step_parity(orc, e, "plane", loss, SCALE, np.asarray(src, np.float32), None, mxa, mxb, tgt, 4, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["point", "plane"])
def test_gpu_tiny_shard(orc, metric):
    """67 selected points: one partial workgroup, more than one wave."""
    from object_alignment_amd.engine import IcpEngine
    src, verts, tris, mxa, mxb = table_case()
    vlist = np.arange(0, 67 * 70, 70, dtype=np.int64)
    assert len(vlist) == 67
    wv = vertex_weights(len(src), seed=6)
    with IcpEngine(0) as e:
        e.set_metric(metric)
        e.set_robust("tukey", SCALE * 4)
        e.set_target_mesh(verts, tris)
        e.set_source(src, vlist=vlist, stride=1)
        e.set_source_weights(wv)
        e.set_matrices(mxa, mxb)
        assert e.n_selected == 67
        step_parity(orc, e, metric, "tukey", SCALE * 4, np.asarray(src, np.float32)[vlist], wv[vlist], mxa, mxb, verts, 1, tris=tris,
                    thresh=0.5)


def _steps(e, n, **kw):
    out = []
    for _ in range(n):
        M, st = e.iterate(thresh=0.5, target_d=1e-4, **kw)
        out.append((M, st))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("metric,n_src", [("point", 5000), ("plane", 5000), ("plane", 262145)])
def test_gpu_huber_at_1e30_is_the_unweighted_step(metric, n_src):
    """Every w is exactly 1 (r <= c): the weighted kernels and the solve's mass from sum w give the loss-none step to 1e-9,
    the same K and the same statistics.  262 145 points: the first size on 512-thread workgroups.

    "The same statistics": the two paths add the same K doubles (d - d_pivot), each below thresh, but in different workgroups
    (the unweighted loop accumulates in its search's epilogue, the weighted one in k_pair_accumulate_weighted), i.e. in a different
    order.  Any order of a sum of K doubles is within (K - 1) u sum|x| of the exact sum (u = 2^-53), so two orders differ by at
    most K eps thresh / K = eps K thresh in the mean (eps = 2^-52) -- 5.6e-13 at 5 000 points -- and by at most
    2 K eps thresh^2 / std in the standard deviation (var = S_DD / K - mean^2, d std = d var / (2 std)); neither bound is ever
    wider than the 1e-9 DESIGN 5.2 holds the statistics to.  (A first version asked for bit equality, which different summation
    orders do not give: 0.054657054740403735 against 0.05465705474040375 on an MI355X, one unit in the last place.)"""
    eps, thresh = 2.0 ** -52, 0.5
    from object_alignment_amd.engine import IcpEngine
    _, verts, tris, mxa, mxb = table_case()
    src = synth.bunny_surface(n_src, 0.5)
    runs = {}
    for loss in ("none", "huber"):
        with IcpEngine(0) as e:
            e.set_metric(metric)
            e.set_robust(loss, 1e30 if loss == "huber" else 0.0)
            e.set_target_mesh(verts, tris)
            e.set_source(src, stride=1)
            e.set_matrices(mxa, mxb)
            runs[loss] = _steps(e, 4)
            W = e.stat("weight_sum")
            assert W == float(runs[loss][-1][1]["K"])                # all w = 1: sum w = K; off: K by definition
    for (M0, s0), (M1, s1) in zip(runs["none"], runs["huber"]):
        print("|dM| %.3g, K %d / %d" % (np.max(np.abs(M0 - M1)), s0["K"], s1["K"]))
        assert np.max(np.abs(M0 - M1)) <= TOL
        assert s0["K"] == s1["K"] and s0["K"] > n_src // 2
        K = s0["K"]
        d_mean, d_std = abs(s0["mean_dist"] - s1["mean_dist"]), abs(s0["std_dist"] - s1["std_dist"])
        print("d mean %.3g (bound %.3g), d std %.3g (bound %.3g)"
              % (d_mean, min(TOL, eps * K * thresh), d_std, min(TOL, 2.0 * K * eps * thresh ** 2 / s0["std_dist"])))
        assert d_mean <= min(TOL, eps * K * thresh)
        assert d_std <= min(TOL, 2.0 * K * eps * thresh ** 2 / s0["std_dist"])


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["point", "plane"])
def test_gpu_zero_one_weights_are_a_vlist(metric):
    """Vertex weights in {0, 1} against a vlist that omits the zero-weight vertices: the same step; K differs by the zeros.
    (The pivot is the first selected vertex: vertex 0 keeps weight 1 so that both selections start with it.)"""
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
            e.set_metric(metric)
            e.set_target_mesh(verts, tris)
            e.set_source(src, vlist=keep if how == "vlist" else None, stride=1)
            if how == "weights":
                e.set_source_weights(w)
            e.set_matrices(mxa, mxb)
            runs[how] = [e.iterate(thresh=0.5, target_d=1e-4) + (e.stat("weight_sum"),) for _ in range(3)]
    for (M0, s0, W0), (M1, s1, W1) in zip(runs["weights"], runs["vlist"]):
        print("|dM| %.3g, K %d / %d, sum w %.17g / %.17g" % (np.max(np.abs(M0 - M1)), s0["K"], s1["K"], W0, W1))
        assert np.max(np.abs(M0 - M1)) <= TOL
        assert s0["K"] - s1["K"] == len(zeros)                      # every point of this case pairs inside thresh
        assert W0 == float(s1["K"]) and W1 == float(s1["K"])


def _loop(e, src, verts, tris, mxa, mxb, iters=8):
    e.set_target_mesh(verts, tris)
    e.set_source(src, stride=1)
    e.set_matrices(mxa, mxb)
    return e.run(iters=iters, thresh=0.5, target_d=1e-4, early_exit=False)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["point", "plane"])
def test_gpu_off_means_off(metric):
    """A loss-none loop after a visit to Tukey + vertex weights (a weighted loop ran; then both cleared) is the fresh
    engine's loop bit for bit."""
    from object_alignment_amd.engine import IcpEngine
    src, verts, tris, mxa, mxb = table_case()
    with IcpEngine(0) as e:
        e.set_metric(metric)
        plain = _loop(e, src, verts, tris, mxa, mxb)
        assert e.stat("weight_sum") == float(plain.last_K)
    with IcpEngine(0) as e:
        e.set_metric(metric)
        e.set_robust("tukey", 0.15)
        e.set_target_mesh(verts, tris)
        e.set_source(src, stride=1)
        e.set_source_weights(vertex_weights(len(src)))
        e.set_matrices(mxa, mxb)
        visit = e.run(iters=3, thresh=0.5, target_d=1e-4, early_exit=False)
        assert visit.iters_done == 3 and e.stat("weight_sum") < float(visit.last_K)
        e.set_robust("none")
        e.set_source_weights(None)
        assert e.stat("robust_loss") == 0.0
        back = _loop(e, src, verts, tris, mxa, mxb)
    assert not np.array_equal(visit.step_M[0], plain.step_M[0])     # (the visit was a different loop)
    for name in ("step_M", "step_new", "step_K", "step_stats", "step_trans", "matrix_world"):
        assert np.array_equal(getattr(plain, name), getattr(back, name)), name


@pytest.mark.gpu
def test_gpu_weighted_point_loop_across_shards():
    """Point metric, Tukey, vertex weights: a three-child multi-device context and the split-phase loop (one context, reducing
    with itself) against the single-device loop over 5 iterations; slot 20 of the exchanged row is sum w (0 when off)."""
    import torch
    from object_alignment_amd import _capi
    from object_alignment_amd.distributed import EngineShard, new_sums_tensor
    from object_alignment_amd.engine import IcpEngine
    src, verts, tris, mxa, mxb = table_case()
    wv = vertex_weights(len(src))

    def setup(e, weighted=True):
        e.set_robust("tukey" if weighted else "none", 0.15 if weighted else 0.0)
        e.set_target_mesh(verts, tris)
        e.set_source(src, stride=1)
        e.set_source_weights(wv if weighted else None)
        e.set_matrices(mxa, mxb)

    kw = dict(iters=5, thresh=0.5, target_d=1e-4, early_exit=False)
    with IcpEngine(0) as e:
        setup(e)
        one = e.run(**kw)
        W_one = e.stat("weight_sum")
    assert one.iters_done == 5
    with IcpEngine(devices=[0, 0, 0]) as m:
        setup(m)
        multi = m.run(**kw)
        W_multi = m.stat("weight_sum")
        # the children end bitwise equal to each other: every child searches its own shard from its own matrix_world, and the
        # answers are those of one context at the first child's matrix_world -- squared float32 distances included
        idx_m, d2_m, _ = m.nn_search()
    with IcpEngine(0) as e:
        setup(e)
        e.set_matrices(multi.matrix_world, mxb)
        idx_1, d2_1, _ = e.nn_search()
    assert np.array_equal(idx_m, idx_1) and np.array_equal(d2_m, d2_1)
    split_sums = {}
    for weighted in (True, False):
        with IcpEngine(0) as e:
            setup(e, weighted)
            sums = new_sums_tensor(torch.device("cuda:0"))
            shard = EngineShard(e, **kw)
            shard.begin()
            for _ in range(5):
                shard.partial(sums)
                torch.cuda.synchronize()
                split_sums.setdefault(weighted, []).append(sums.cpu().numpy().copy())
                shard.finish(sums)
            res = shard.end()
            e.set_stream(None)
            if weighted:
                split, W_split = res, e.stat("weight_sum")
    for name, other in (("multi", multi), ("split", split)):
        assert other.iters_done == 5
        for it in range(5):
            d = float(np.max(np.abs(other.step_M[it] - one.step_M[it])))
            print("%s iteration %d: |dM| %.3g, K %d / %d" % (name, it, d, other.step_K[it], one.step_K[it]))
            assert d <= TOL
        assert np.array_equal(other.step_K, one.step_K)
    assert abs(W_multi - W_one) <= 1e-9 * W_one and abs(W_split - W_one) <= 1e-9 * W_one
    for row in split_sums[True]:
        assert 0.0 < row[20] < row[17] and np.all(row[21:] == 0.0)
    assert abs(split_sums[True][-1][20] - W_one) <= 1e-9 * W_one
    for row in split_sums[False]:
        assert row[17] > 0.0 and np.all(row[20:] == 0.0)             # off: slot 20 stays 0


@pytest.mark.gpu
def test_gpu_outlier_case_tukey_ends_closer(orc):
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings
    src, verts, tris, mxa, mxb = outlier_case()
    res = {}
    with IcpEngine(0) as e:
        for loss in ("none", "tukey"):
            st = IcpSettings(sample_fraction=1, target_d=OUT_TARGET_D, robust_loss=loss, robust_scale=OUT_C if loss != "none" else 0.0)
            res[loss] = IcpAlign(st, engine=e).run(src, verts, mxa, mxb, target_tris=tris)
            assert e.stat("robust_loss") == (2.0 if loss == "tukey" else 0.0)
    rec = recorded_outlier_reference()
    for loss in res:
        print("%s: %d iterations (reference %d), pose error %.4g (reference %.4g)"
              % (loss, res[loss].iters_done, int(rec[loss + "_iters"]), pose_error(res[loss].matrix_world), pose_error(rec[loss + "_matrix_world"])))
    assert res["none"].converged and res["tukey"].converged
    assert pose_error(res["tukey"].matrix_world) < pose_error(res["none"].matrix_world)
    for loss in res:
        assert res[loss].iters_done == int(rec[loss + "_iters"])


@pytest.mark.gpu
def test_gpu_robust_refusals_leave_the_context_usable():
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    src, verts, tris, mxa, mxb = table_case()

    def point_loop_ok(e):
        e.set_metric("point")
        e.set_matrices(mxa, mxb)
        r = e.run(iters=5, thresh=0.5, target_d=0.01)
        assert r.iters_done >= 1 and np.all(np.isfinite(r.matrix_world))

    def refused(call, code=_capi.OA_E_BAD_ARG):
        with pytest.raises(_capi.OaError) as ei:
            call()
        assert ei.value.code == code

    with IcpEngine(0) as e:
        refused(lambda: e.set_source_weights(np.ones(len(src), np.float32)), _capi.OA_E_STATE)      # weights before a source
        e.set_target_mesh(verts, tris)
        e.set_source(src, stride=1)
        e.set_matrices(mxa, mxb)
        refused(lambda: e.set_robust(4, 0.1))
        refused(lambda: e.set_robust(-1, 0.1))
        with pytest.raises(ValueError):
            e.set_robust("welsch", 0.1)
        point_loop_ok(e)
        for bad in (0.0, -0.1, float("nan"), float("inf")):
            for loss in LOSSES:
                refused(lambda: e.set_robust(loss, bad))
        assert e.stat("robust_loss") == 0.0
        e.set_robust("none", float("nan"))                          # (the scale of loss none is not looked at)
        point_loop_ok(e)
        w = np.ones(len(src), np.float32)
        for bad in (-1e-3, float("nan"), float("inf")):
            wb = w.copy()
            wb[1234] = bad
            refused(lambda: e.set_source_weights(wb))
        refused(lambda: e.set_source_weights(w[:-1]))
        refused(lambda: e.set_source_weights(np.ones(len(src) + 1, np.float32)))
        point_loop_ok(e)
        last_K = e.run(iters=1, thresh=0.5).last_K
        assert e.stat("weight_sum") == float(last_K)                # none of them took hold
        e.set_source_weights(np.zeros(len(src), np.float32))        # all weights zero: K pairs, no mass
        e.set_matrices(mxa, mxb)
        with pytest.raises(ValueError, match="input arrays are of wrong shape or type"):
            e.run(iters=5, thresh=0.5)
        with pytest.raises(ValueError, match="input arrays are of wrong shape or type"):
            e.iterate(thresh=0.5)
        e.set_metric("plane")
        e.set_matrices(mxa, mxb)
        with pytest.raises(ValueError, match="input arrays are of wrong shape or type"):
            e.run(iters=5, thresh=0.5)
        e.set_source_weights(None)
        point_loop_ok(e)
    with IcpEngine(devices=[0, 0]) as m:
        m.set_target_mesh(verts, tris)
        m.set_source(src, stride=1)
        m.set_matrices(mxa, mxb)
        m.set_metric("plane")
        m.set_robust("tukey", 0.15)
        with pytest.raises(_capi.OaError, match="single-device") as ei:
            m.run(iters=5)
        assert ei.value.code == _capi.OA_E_STATE
        with pytest.raises(_capi.OaError, match="single-device"):
            m.iterate()
        point_loop_ok(m)                                            # (the weighted point loop of a multi-device context)
        assert m.stat("robust_loss") == 2.0 and m.stat("weight_sum") > 0.0
