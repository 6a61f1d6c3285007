"""Plane-to-plane ICP (Generalized-ICP: Segal, Haehnel, Thrun 2009): oa_set_metric(OA_METRIC_GICP) / oa_set_gicp /
oa_set_source_normals, IcpEngine.set_gicp / set_source_normals, IcpSettings(metric="gicp", gicp_epsilon=...),
IcpAlign.run(..., source_normals=array | "estimate").

The CPU reference of the step lives here (gicp_step): numpy, fp64, dense -- every pair its own 3 x 3 M inverted by
numpy.linalg.inv, its own 3 x 6 J and 6 x 6 J^T W J, the pairs added one after the other in pair order --, numpy.linalg.eigh
with the 1e-10 x lambda_max cut and Rodrigues for the solve, as tests/test_plane_metric.py's plane_solve.  The pairs come from
the oracle's searches (nn_tri_brute / nn_brute) and a numpy restatement of its float32 helpers that is checked against them
bit for bit.  The engine is held to the reference one step at a time: before every step the device's matrix_world goes to the
reference, so a last-bit difference in one step cannot move a correspondence in the next.
"""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

from object_alignment_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gicp_table_case.json")
EIG_CUT = 1e-10
TOL = 1e-9          # tests/test_plane_metric.py's bound for the plane step, copied
EPS = 1e-3          # the default gicp_epsilon
POSE = dict(rotvec=(0.10, -0.07, 0.12), t=(0.05, -0.03, 0.02))     # the pose of DESIGN 3.9's case


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build_hip()
    return g


# ------------------------------------------------------------------------------------------------ the reference
def rodrigues(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-4:
        a, b = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
    else:
        a, b = np.sin(th) / th, 2.0 * np.sin(0.5 * th) ** 2 / (th * th)
    return np.eye(3) + a * K + b * (K @ K)


def solve6(H, g, c):
    """The minimum-norm step of H x = -g about the pivot c -> (M 4x4, rank): plane_solve's second half."""
    lam, V = np.linalg.eigh(H)
    keep = lam > EIG_CUT * lam.max()
    x = -(V[:, keep] @ ((V[:, keep].T @ g) / lam[keep]))
    R = rodrigues(x[:3])
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = c + x[3:] - R @ c
    return M, int(keep.sum())


def plane_solve(a, b, n, c):
    """tests/test_plane_metric.py's plane_solve, restated (unit n, every pair valid)."""
    a, b, n = (np.asarray(x, np.float64) for x in (a, b, n))
    a = a - c
    b = b - c
    r = np.einsum("ij,ij->i", n, a - b)
    J = np.concatenate([np.cross(a, n), n], axis=1)
    return solve6(J.T @ J, J.T @ r, c)


def point_gn_solve(a, b, c):
    """The Gauss-Newton point-to-point step: minimise sum |e + J x|^2, J = [-[a']x, I]."""
    a, b = np.asarray(a, np.float64) - c, np.asarray(b, np.float64) - c
    H, g = np.zeros((6, 6)), np.zeros(6)
    for k in range(len(a)):
        J = np.concatenate([-skew(a[k]), np.eye(3)], axis=1)
        H += J.T @ J
        g += J.T @ (a[k] - b[k])
    return solve6(H, g, c)


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def unit_rows(n):
    """(unit rows fp64, ok) in the operation order the contract gives both normals (plane_normal's): n2 = (x x + y y) + z z,
    n * (1 / sqrt(n2)).  A row of zero or non-finite length is not ok (and comes back as zeros).  The order matters: at
    eps = 1e-6 a last-bit difference in the normals moves M by 3e-15 .. 7e-15 (measured on the CPU), more than everything else."""
    n = np.asarray(n, np.float64)
    with np.errstate(all="ignore"):
        n2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        ok = (n2 > 0.0) & (n2 < np.inf)
        u = np.where(ok[:, None], n * (1.0 / np.sqrt(np.where(ok, n2, 1.0)))[:, None], 0.0)
    return u, ok


def transposed_apply(M, v):
    """M[:3, :3]^T v per row of v, in fp64 from the float32 matrix, summed left to right (plane_normal's and the normal-angle
    test's order; numpy's matmul leaves the order to the BLAS): out[:, k] = (M[0, k] v0 + M[1, k] v1) + M[2, k] v2."""
    M, v = np.asarray(M, np.float32).astype(np.float64), np.asarray(v, np.float64)
    return np.stack([(M[0, k] * v[:, 0] + M[1, k] * v[:, 1]) + M[2, k] * v[:, 2] for k in range(3)], axis=1)


def gicp_weights(n_a, n_b, eps):
    """W = 2 eps M^-1 per pair (K x 3 x 3), M = 2 I - (1 - eps)(n_a n_a^T + n_b n_b^T), numpy.linalg.inv one matrix at a time."""
    M = 2.0 * np.eye(3)[None] - (1.0 - eps) * (n_a[:, :, None] * n_a[:, None, :] + n_b[:, :, None] * n_b[:, None, :])
    return 2.0 * eps * np.linalg.inv(M)


def psi(loss, r, c):
    if loss == "huber":
        return np.where(r <= c, 1.0, c / np.maximum(r, 1e-300))
    q2 = (r / c) ** 2
    if loss == "tukey":
        return np.where(r < c, (1.0 - q2) ** 2, 0.0)
    if loss == "cauchy":
        return 1.0 / (1.0 + q2)
    return np.ones_like(r)


def gicp_step(a, b, n_a, n_b, pivot, eps, W=None, reverse=False, loss=None, scale=1.0, res_scale=1.0, w_vertex=None):
    """The step of the pairs (a, b) with unit normals (n_a, n_b), all K x 3 fp64, about `pivot` -> (M 4x4, rank, e^T W e per pair,
    sum w).  Dense: per pair W (numpy.linalg.inv of its M, or the W given), J = [-[a']x, I3], J^T W J (6 x 6), J^T W e; the
    pairs' terms are added one after the other in pair order (numpy.cumsum along the pair axis is that running sum), or in the
    reverse order.  loss / scale / res_scale / w_vertex: w = w_vertex psi(res_scale sqrt(e^T W e)), else 1."""
    a, b, n_a, n_b = (np.asarray(x, np.float64) for x in (a, b, n_a, n_b))
    if len(a) < 3:
        raise ValueError("input arrays are of wrong shape or type")
    c = np.asarray(pivot, np.float64)
    ap, e = a - c, (a - c) - (b - c)
    if W is None:
        W = gicp_weights(n_a, n_b, eps)
    J = np.zeros((len(a), 3, 6))
    J[:, 0, 1], J[:, 0, 2], J[:, 1, 0], J[:, 1, 2], J[:, 2, 0], J[:, 2, 1] = ap[:, 2], -ap[:, 1], -ap[:, 2], ap[:, 0], ap[:, 1], -ap[:, 0]
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0                       # J = [-[a']x, I3]
    u = np.einsum("kij,kj->ki", W, e)
    rr = np.einsum("ki,ki->k", e, u)
    w = np.ones(len(a))
    if loss is not None:
        w = psi(loss, res_scale * np.sqrt(np.maximum(rr, 0.0)), scale)
    if w_vertex is not None:
        w = w * np.asarray(w_vertex, np.float64)
    Hk = w[:, None, None] * (np.transpose(J, (0, 2, 1)) @ W @ J)
    gk = w[:, None] * np.einsum("kji,kj->ki", J, u)
    if reverse:
        Hk, gk = Hk[::-1], gk[::-1]
    H, g = np.cumsum(Hk, axis=0)[-1], np.cumsum(gk, axis=0)[-1]
    if not w.sum() > 0.0:
        raise ValueError("input arrays are of wrong shape or type")
    M, rank = solve6(H, g, c)
    return M, rank, rr, float(w.sum())


# ---- the oracle's float32 helpers over arrays (checked against the oracle's own in test_reference_restatement)
def m4v3(M, v):
    """mat4_mul_vec3 row by row: float32 products, summed in fp64 in order (w = 1), rounded once."""
    M, v = np.asarray(M, np.float32), np.asarray(v, np.float32).reshape(-1, 3)
    out = np.empty_like(v)
    for r in range(3):
        acc = (M[r, 0] * v[:, 0]).astype(np.float64)
        acc = acc + (M[r, 1] * v[:, 1]).astype(np.float64)
        acc = acc + (M[r, 2] * v[:, 2]).astype(np.float64)
        acc = acc + np.float64(M[r, 3] * np.float32(1.0))
        out[:, r] = acc.astype(np.float32)
    return out


def v3len(d):
    """vec3_length: float32 squares, summed in fp64 last component first."""
    d = np.asarray(d, np.float32)
    acc = (d[:, 2] * d[:, 2]).astype(np.float64)
    acc = acc + (d[:, 1] * d[:, 1]).astype(np.float64)
    acc = acc + (d[:, 0] * d[:, 0]).astype(np.float64)
    return np.sqrt(acc)


def selection(n_verts, vlist, stride):
    sel = np.arange(n_verts) if vlist is None else np.asarray(vlist, np.int64)
    return sel[::stride] if stride > 1 else sel


def ref_pairs(orc, src_sel, sn_sel, mx1, mx2, tgt, tris=None, tgt_normals=None, thresh=0.5, max_angle_deg=None):
    """The pairs of one step as the engine forms them, fp64 from the float32 values: dict(a, b, n_a, n_b, dist, slot).  A pair
    with a normal of zero or non-finite length on either side is dropped (slot: which slots are left)."""
    mx1, mx2 = np.asarray(mx1, np.float32), np.asarray(mx2, np.float32)
    imx1, imx2 = orc.mat4_inverted(mx1), orc.mat4_inverted(mx2)
    tgt = np.asarray(tgt, np.float32)
    src_sel, sn_sel = np.asarray(src_sel, np.float32), np.asarray(sn_sel, np.float32)
    w = m4v3(imx2, m4v3(mx1, src_sel))                                                                   # co_find
    if tris is not None:
        face, co1, _ = orc.nn_tri_brute(w, tgt, tris)
        ta, tb, tc = (tgt[np.asarray(tris)[face, k]] for k in range(3))
        e1, e2 = ta - tb, tb - tc                                                                        # float32, no fma
        tn = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1).astype(np.float32)
    else:
        idx, _ = orc.nn_brute(w, tgt)
        co1 = tgt[idx]
        tn = np.asarray(tgt_normals, np.float32)[idx]
    wa, wb = m4v3(mx2, w), m4v3(mx2, co1)
    dist = v3len(wa - wb)
    keep = dist < thresh
    nw = transposed_apply(imx2, tn.astype(np.float64))               # base-local -> world: inverse transpose of mx2
    if max_angle_deg is not None:
        cos_min = np.cos(max_angle_deg * 3.14159265358979323846 / 180.0)
        sw = transposed_apply(imx1, sn_sel.astype(np.float64))
        with np.errstate(all="ignore"):
            cc = np.einsum("ij,ij->i", sw, nw) / np.sqrt(np.einsum("ij,ij->i", sw, sw) * np.einsum("ij,ij->i", nw, nw))
        keep &= cc >= cos_min
    n_b, ok_b = unit_rows(transposed_apply(mx1, nw))                 # world -> align-local: mx1^T
    n_a, ok_a = unit_rows(sn_sel)
    keep &= ok_b & ok_a
    return dict(a=src_sel[keep].astype(np.float64), b=m4v3(imx1, wb)[keep].astype(np.float64), n_a=n_a[keep], n_b=n_b[keep],
                dist=dist[keep], slot=np.nonzero(keep)[0])


def res_scale_of(mx1):
    """align-local residual -> world units: cbrt(|det|) of the float32 matrix_world a loop STARTS from, in fp64 (the step is rigid)"""
    return float(np.cbrt(abs(np.linalg.det(np.asarray(mx1, np.float32)[:3, :3].astype(np.float64)))))


def ref_step(orc, src_sel, sn_sel, mx1, mx2, tgt, eps=EPS, loss=None, scale=1.0, w_sel=None, res_scale=None, **kw):
    """One GICP step from matrix_world mx1: dict(M, M_rev, new_mat, mw, K, mean, std, rank, wsum).  res_scale: the loop's (taken
    from the matrix_world its first step started from); None: this step is the first."""
    P = ref_pairs(orc, src_sel, sn_sel, mx1, mx2, tgt, **kw)
    c = np.asarray(src_sel, np.float32)[0].astype(np.float64)
    wkw = dict(loss=loss, scale=scale, res_scale=res_scale_of(mx1) if res_scale is None else res_scale,
               w_vertex=None if w_sel is None else np.asarray(w_sel, np.float32)[P["slot"]])
    M, rank, _, wsum = gicp_step(P["a"], P["b"], P["n_a"], P["n_b"], c, eps, **wkw)
    M_rev = gicp_step(P["a"], P["b"], P["n_a"], P["n_b"], c, eps, reverse=True, **wkw)[0]
    new_mat = M.astype(np.float32)
    return dict(M=M, M_rev=M_rev, new_mat=new_mat, mw=orc.mat4_mul(np.asarray(mx1, np.float32), new_mat), K=len(P["a"]),
                mean=float(np.mean(P["dist"])), std=float(np.std(P["dist"])), rank=rank, wsum=wsum, pairs=P)


def ref_loop(orc, step, mx1, iters=50, target_d=1e-4):
    """The reference's loop (5-slot ring of step lengths against target_d) around step(mx1) -> dict(mw, new_mat, mean)."""
    mx1 = np.asarray(mx1, np.float32).copy()
    ring = [2.0 * target_d] * 5
    out = dict(iters_done=0, converged=False, mean=None, matrix_world=mx1)
    for n in range(iters):
        s = step(mx1)
        mx1 = s["mw"]
        ring[n % 5] = orc.vec3_length(s["new_mat"][:3, 3])
        out.update(iters_done=n + 1, mean=s["mean"], matrix_world=mx1)
        if all(t < target_d for t in ring):
            out["converged"] = True
            break
    return out


def pose_error(mw):
    """table_case starts from the inverse of the pose with the points on the surface: the aligned matrix_world is the identity."""
    return float(np.max(np.abs(np.asarray(mw, np.float64) - np.eye(4))))


@functools.lru_cache(maxsize=None)
def table_case():
    """DESIGN 3.9's case with the source's analytic normals: 5 000 bunny points on the 19 200-triangle cubed sphere."""
    src, sn = synth.bunny_surface_with_normals(5000, 0.5)
    verts, tris = synth.cubed_surface_mesh(40)
    P = synth.rigid4(synth.rotation_from_rotvec(list(POSE["rotvec"])), list(POSE["t"]), dtype=np.float64)
    return np.asarray(src, np.float32), np.asarray(sn, np.float32), verts, tris, np.linalg.inv(P).astype(np.float32), np.eye(4, dtype=np.float32)


def scaled_base():
    R = synth.rotation_from_rotvec([0.3, -0.2, 0.25]).astype(np.float64)
    B = np.eye(4)
    B[:3, :3] = R @ np.diag([1.25, 0.8, 1.1])
    B[:3, 3] = [0.4, -0.3, 0.2]
    return B


def random_pairs(K, seed=5, noise=0.02):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(K, 3))
    n_b = unit_rows(rng.normal(size=(K, 3)))[0]
    n_a = unit_rows(n_b + 0.3 * rng.normal(size=(K, 3)))[0]
    b = a + noise * rng.normal(size=(K, 3)) + np.array([0.01, -0.02, 0.015])
    return a, b, n_a, n_b


# ------------------------------------------------------------------------------------------------ CPU
def test_gicp_abi_and_bindings(built):
    """Fails without the feature: the header, the library, the bindings and the settings all name the GICP metric."""
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings
    hdr = open(os.path.join(ROOT, "include", "oa_icp.h")).read()
    L = C.CDLL(os.path.join(ROOT, "object_alignment_amd", "liboa_icp.so"))
    LL = _capi.load()
    for fn in ("oa_set_gicp", "oa_set_source_normals"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, hdr), fn
        assert fn in _capi.SYMBOLS
        assert hasattr(L, fn), fn
        assert getattr(LL, fn).argtypes is not None
    assert re.search(r"#define\s+OA_METRIC_GICP\s+2\b", hdr)
    assert _capi.OA_METRIC_GICP == 2 and IcpEngine.METRICS["gicp"] == 2
    assert callable(IcpEngine.set_gicp) and callable(IcpEngine.set_source_normals)
    st = IcpSettings(metric="gicp", gicp_epsilon=1e-2)
    assert st.metric == "gicp" and st.gicp_epsilon == 1e-2 and IcpSettings().gicp_epsilon == 1e-3 and IcpSettings().metric == "point"
    assert C.sizeof(_capi.Settings) == 32 and C.sizeof(_capi.Report) == 72
    # the bad string is refused before an engine is opened (there is no GPU here to open one on)
    z = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="source_normals"):
        IcpAlign(st).run(z, z, np.eye(4), np.eye(4), source_normals="bogus")


def test_reference_restatement(orc):
    """gicp_step against what it must reduce to, and the float32 helpers against the oracle's, bit for bit."""
    a, b, n_a, n_b = random_pairs(400)
    c = a[0].copy()
    # W = n n^T: the plane metric's step
    M, rank, rr, _ = gicp_step(a, b, n_a, n_b, c, EPS, W=n_b[:, :, None] * n_b[:, None, :])
    Mp, rank_p = plane_solve(a, b, n_b, c)
    assert np.max(np.abs(M - Mp)) < 1e-12 and rank == rank_p == 6
    assert np.allclose(rr, np.einsum("ij,ij->i", n_b, a - b) ** 2, rtol=0, atol=1e-15)
    # eps = 1: W = I, the Gauss-Newton point step
    M1, rank1, rr1, _ = gicp_step(a, b, n_a, n_b, c, 1.0)
    Mg, rank_g = point_gn_solve(a, b, c)
    assert np.max(np.abs(M1 - Mg)) < 1e-12 and rank1 == rank_g == 6
    assert np.allclose(rr1, np.einsum("ij,ij->i", a - b, a - b), rtol=1e-13, atol=0)
    # agreeing normals, eps -> 0: e^T W e -> (n . e)^2
    rr0 = gicp_step(a, b, n_b, n_b, c, 1e-6)[2]
    assert np.allclose(rr0, np.einsum("ij,ij->i", n_b, a - b) ** 2, rtol=0, atol=1e-5 * np.max(np.einsum("ij,ij->i", a - b, a - b)))
    # the order of the pairs
    for eps in (1.0, EPS, 1e-6):
        f, r = gicp_step(a, b, n_a, n_b, c, eps)[0], gicp_step(a, b, n_a, n_b, c, eps, reverse=True)[0]
        assert np.max(np.abs(f - r)) < TOL / 10
    # the signs of the normals drop out of the reference exactly
    sg = np.where(np.arange(len(a)) % 2 == 0, -1.0, 1.0)[:, None]
    assert np.array_equal(gicp_step(a, b, n_a * sg, n_b * -sg, c, EPS)[0], gicp_step(a, b, n_a, n_b, c, EPS)[0])
    # the float32 helpers
    rng = np.random.default_rng(3)
    Mx = (scaled_base() @ synth.rigid4(synth.rotation_from_rotvec([0.2, 0.1, -0.3]), [0.3, 0.2, -0.1], dtype=np.float64)).astype(np.float32)
    v = rng.normal(size=(300, 3)).astype(np.float32)
    assert np.array_equal(m4v3(Mx, v), np.array([orc.mat4_mul_vec3(Mx, p) for p in v]))
    assert np.array_equal(v3len(v), np.array([orc.vec3_length(p) for p in v]))


def test_reference_gicp_loop_on_the_table_case(orc):
    """The yardstick itself: the reference's GICP loop converges on DESIGN 3.9's case; its count and final pose error are the
    fixture the GPU loop is held to.  The point and plane loops are printed beside it; no order between them is asserted."""
    src, sn, verts, tris, mxa, mxb = table_case()
    first = ref_step(orc, src, sn, mxa, mxb, verts, tris=tris, thresh=0.5)
    assert np.max(np.abs(first["M"] - first["M_rev"])) < TOL / 10 and first["rank"] == 6
    gicp = ref_loop(orc, lambda m: ref_step(orc, src, sn, m, mxb, verts, tris=tris, thresh=0.5), mxa)

    def plane_step(m):
        P = ref_pairs(orc, src, sn, m, mxb, verts, tris=tris, thresh=0.5)
        new_mat = plane_solve(P["a"], P["b"], P["n_b"], src[0].astype(np.float64))[0].astype(np.float32)
        return dict(new_mat=new_mat, mw=orc.mat4_mul(np.asarray(m, np.float32), new_mat), mean=float(np.mean(P["dist"])))

    plane = ref_loop(orc, plane_step, mxa)
    point = orc.icp_run(src, verts, mxa, mxb, iters=50, sample=1, thresh=0.5, target_d=1e-4, use_target=True, tris=tris)
    print("iterations / pose error: gicp %d / %.3g, plane %d / %.3g, point %d / %.3g"
          % (gicp["iters_done"], pose_error(gicp["matrix_world"]), plane["iters_done"], pose_error(plane["matrix_world"]),
             point["iters_done"], pose_error(point["matrix_world"])))
    assert gicp["converged"] and plane["converged"] and point["converged"]
    fx = json.load(open(FIXTURE))
    assert fx["gicp_epsilon"] == EPS
    assert abs(gicp["iters_done"] - fx["iters_done"]) <= 1
    assert pose_error(gicp["matrix_world"]) <= 2.0 * fx["pose_error"] + 1e-6 and fx["pose_error"] <= 2.0 * pose_error(gicp["matrix_world"]) + 1e-6


# ------------------------------------------------------------------------------------------------ GPU
def ulp_diff32(a, b):
    a, b = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    return np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64))


def step_parity(orc, eng, src_sel, sn_sel, mxb, tgt, steps, thresh=0.5, **kw):
    """`steps` steps of the engine against ref_step, each from the device's own matrix_world.  The bound on |dM| is TOL, or --
    where the reference's own forward / reverse spread exceeds TOL / 10 -- 100 x that spread (measured on the reference alone)."""
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


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["surface", "vertex_normals", "scaled_base", "vlist_stride2", "normal_test", "eps_1", "eps_1e-6",
                                  "mode_brute", "mode_grid", "mode_bvh"])
def test_gpu_gicp_step_parity(orc, case):
    """Measured on an MI355X: every case holds all bounds with |dM| <= 2e-15 and new_mat equal bit for bit over its 4 steps.
    eps_1e-6 is the sensitive one (cond(M) = 1e6): while the reference formed its normals through numpy's matmul and n / |n|, a
    last-bit difference from the contract's n * (1 / sqrt(n2)) moved M by up to 5.5e-15 and new_mat by 2 ulps in the fourth step
    (whose entries are near 1e-8); the adjugate against numpy.linalg.inv moves it by 1e-15 only."""
    from object_alignment_amd.engine import IcpEngine
    src, sn, verts, tris, mxa, mxb = table_case()
    vlist, stride, kw = None, 1, {}
    with IcpEngine(0) as e:
        e.set_metric("gicp")
        assert e.stat("metric") == 2.0
        if case.startswith("mode_"):
            e.set_search_mode(case[5:])
        if case.startswith("eps_"):
            kw.update(eps=float(case[4:]))
            e.set_gicp(kw["eps"])
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
        assert e.stat("metric") == 2.0                              # survives the uploads and set_matrices
        step_parity(orc, e, src[sel], sn[sel], mxb, tgt, 4, **kw)


@functools.lru_cache(maxsize=None)
def shape_case(n):
    tgt, tn = synth.bunny_surface_with_normals(500)
    src, sn = synth.bunny_surface_with_normals(n, 0.5)
    P = synth.rigid4(synth.rotation_from_rotvec([0.03, -0.02, 0.04]), [0.02, -0.01, 0.01], dtype=np.float64)
    return (np.asarray(src, np.float32), np.asarray(sn, np.float32), np.asarray(tgt, np.float32), np.asarray(tn, np.float32),
            np.linalg.inv(P).astype(np.float32), np.eye(4, dtype=np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 63, 64, 65, 511, 512, 513, 262145])
def test_gpu_gicp_launch_shapes(orc, n):
    """One wave and less, the wave's and the workgroup's edges, and the first size past the 256 -> 512-thread switch."""
    from object_alignment_amd.engine import IcpEngine
    src, sn, tgt, tn, mxa, mxb = shape_case(n)
    with IcpEngine(0) as e:
        e.set_metric("gicp")
        e.set_target(tgt)
        e.set_target_normals(tn)
        e.set_source(src, stride=1)
        e.set_source_normals(sn)
        e.set_matrices(mxa, mxb)
        ref = step_parity(orc, e, src, sn, mxb, tgt, 1, tgt_normals=tn)
        assert ref["K"] == n                                        # every slot of the launch carries a pair


@pytest.mark.gpu
def test_gpu_gicp_dropped_pairs(orc):
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
        e.set_metric("gicp")
        e.set_target_mesh(verts, tris)
        e.set_source(src, stride=1)
        e.set_source_normals(bad)
        e.set_matrices(mxa, mxb)
        full = ref_pairs(orc, src, sn, mxa, mxb, verts, tris=tris, thresh=0.5)["slot"]
        left = ref_pairs(orc, src, bad, mxa, mxb, verts, tris=tris, thresh=0.5)["slot"]
        gone = sorted(set(full) - set(left))
        assert gone == sorted(set(bad_slots) & set(full)) and len(gone) >= 5      # the reference drops exactly the marked slots
        step_parity(orc, e, src, bad, mxb, verts, 2, tris=tris)
        # nothing but zero normals: no pair is left
        e.set_source_normals(np.zeros_like(sn))
        e.set_matrices(mxa, mxb)
        with pytest.raises(ValueError, match="input arrays are of wrong shape or type"):
            e.iterate(thresh=0.5, target_d=1e-4)
        e.set_source_normals(sn)
        e.set_matrices(mxa, mxb)
        step_parity(orc, e, src, sn, mxb, verts, 1, tris=tris)


@pytest.mark.gpu
def test_gpu_gicp_normal_signs_drop_out():
    from object_alignment_amd.engine import IcpEngine
    src, sn, _, _, mxa, mxb = table_case()
    tgt, tn = synth.bunny_surface_with_normals(20000)
    rng = np.random.default_rng(11)
    sg_s = np.where(rng.random(len(sn)) < 0.5, -1.0, 1.0).astype(np.float32)[:, None]
    sg_t = np.where(rng.random(len(tn)) < 0.5, -1.0, 1.0).astype(np.float32)[:, None]
    out = []
    for s_n, t_n in ((sn, np.asarray(tn, np.float32)), (sn * sg_s, np.asarray(tn, np.float32) * sg_t)):
        with IcpEngine(0) as e:
            e.set_metric("gicp")
            e.set_target(tgt)
            e.set_target_normals(t_n)
            e.set_source(src, stride=1)
            e.set_source_normals(s_n)
            e.set_matrices(mxa, mxb)
            r = e.run(iters=3, thresh=0.5, target_d=1e-4, early_exit=False)
            assert r.iters_done == 3
            out.append((r.step_M.copy(), r.matrix_world.copy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["huber", "tukey", "cauchy", "vertex_weights", "huber_1e30"])
def test_gpu_gicp_weighted_step_parity(orc, case):
    from object_alignment_amd.engine import IcpEngine
    src, sn, verts, tris, mxa, mxb = table_case()
    kw = dict(tris=tris)
    with IcpEngine(0) as e:
        e.set_metric("gicp")
        e.set_target_mesh(verts, tris)
        e.set_source(src, stride=1)
        e.set_source_normals(sn)
        if case == "vertex_weights":
            wv = np.random.default_rng(2).uniform(0.0, 2.0, len(src)).astype(np.float32)
            wv[::7] = 0.0
            e.set_source_weights(wv)
            kw.update(w_sel=wv)
        elif case == "huber_1e30":
            e.set_robust("huber", 1e30)
            kw.update(loss="huber", scale=1e30)
        else:
            scale = {"huber": 0.01, "tukey": 0.05, "cauchy": 0.01}[case]       # inside the residuals of the first steps
            e.set_robust(case, scale)
            kw.update(loss=case, scale=scale)
        e.set_matrices(mxa, mxb)
        ref = step_parity(orc, e, src, sn, mxb, verts, 2, **kw)
        if case == "huber_1e30":                                    # every weight is one: the unweighted step
            plain = gicp_step(ref["pairs"]["a"], ref["pairs"]["b"], ref["pairs"]["n_a"], ref["pairs"]["n_b"], src[0].astype(np.float64), EPS)[0]
            assert np.max(np.abs(e._history(1)[0][-1] - plain)) <= TOL and ref["wsum"] == ref["K"]
        elif case != "vertex_weights":
            assert ref["wsum"] < 0.98 * ref["K"]                    # the loss bites at this scale


@pytest.mark.gpu
def test_gpu_gicp_search_modes_agree_bitwise():
    from object_alignment_amd.engine import IcpEngine
    src, sn, verts, tris, mxa, mxb = table_case()
    hist = {}
    for mode in ("brute", "grid", "bvh", "auto", "auto"):
        with IcpEngine(0) as e:
            e.set_metric("gicp")
            e.set_search_mode(mode)
            e.set_target_mesh(verts, tris)
            e.set_source(src, stride=1)
            e.set_source_normals(sn)
            e.set_matrices(mxa, mxb)
            r = e.run(iters=8, thresh=0.5, target_d=1e-4, early_exit=False)
        assert r.iters_done == 8
        hist.setdefault(mode, []).append((r.step_M.copy(), r.step_new.copy(), r.step_K.copy(), r.matrix_world.copy()))
    first = hist["brute"][0]
    for mode, runs in hist.items():
        for run in runs:
            for x, y in zip(first, run):
                assert np.array_equal(x, y), mode


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["point", "plane"])
def test_gpu_other_metrics_unmoved_by_a_visit_to_gicp(metric):
    from object_alignment_amd.engine import IcpEngine
    src, sn, verts, tris, mxa, mxb = table_case()

    def history(e):
        e.set_matrices(mxa, mxb)
        return e.run(iters=10, thresh=0.5, target_d=0.01, early_exit=False)

    runs = []
    for visit in ("never", "metric_only", "with_normals"):
        with IcpEngine(0) as e:
            if visit != "never":
                e.set_metric("gicp")
                e.set_gicp(1e-2)
            e.set_target_mesh(verts, tris)
            e.set_source(src, stride=1)
            if visit == "with_normals":
                e.set_source_normals(sn)
                e.set_matrices(mxa, mxb)
                assert e.run(iters=2, thresh=0.5, target_d=0.01, early_exit=False).iters_done == 2      # a GICP loop in between
            e.set_metric(metric)
            runs.append(history(e))
            if visit == "never":
                runs.append(history(e))                             # the same loop twice, before any visit
    for other in runs[1:]:
        for name in ("step_M", "step_new", "step_K", "step_stats", "step_trans", "matrix_world"):
            assert np.array_equal(getattr(runs[0], name), getattr(other, name)), name


@pytest.mark.gpu
def test_gpu_gicp_loop_on_the_table_case():
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings
    src, sn, verts, tris, mxa, mxb = table_case()
    fx = json.load(open(FIXTURE))
    with IcpEngine(0) as e:
        res = IcpAlign(IcpSettings(metric="gicp", sample_fraction=1, target_d=1e-4), engine=e).run(
            src, verts, mxa, mxb, source_normals=sn, target_tris=tris)
        assert e.stat("metric") == 2.0
        again = IcpAlign(IcpSettings(metric="gicp", sample_fraction=1, target_d=1e-4), engine=e).run(
            src, verts, mxa, mxb, source_normals=sn, target_tris=tris)
    err = pose_error(res.matrix_world)
    print("gicp loop: %d iterations (fixture %d), pose error %.3g (fixture %.3g)" % (res.iters_done, fx["iters_done"], err, fx["pose_error"]))
    assert res.converged
    assert abs(res.iters_done - fx["iters_done"]) <= 2
    assert err <= 2.0 * fx["pose_error"] + 1e-6
    assert np.array_equal(res.matrix_world, again.matrix_world) and res.iters_done == again.iters_done      # two runs, the same bits


@pytest.mark.gpu
def test_gpu_gicp_loop_with_estimated_normals():
    """A 2 000-point source against DESIGN 3.12's 8 000-point cloud, the normals of both estimated on the device."""
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings
    src = synth.bunny_surface(2000, 0.5)
    tgt = synth.bunny_surface(8000)
    P = synth.rigid4(synth.rotation_from_rotvec(list(POSE["rotvec"])), list(POSE["t"]), dtype=np.float64)
    mxa, mxb = np.linalg.inv(P).astype(np.float32), np.eye(4, dtype=np.float32)
    with IcpEngine(0) as e:
        gicp = IcpAlign(IcpSettings(metric="gicp", sample_fraction=1, target_d=1e-4), engine=e).run(
            src, tgt, mxa, mxb, source_normals="estimate", target_normals="estimate")
        plane = IcpAlign(IcpSettings(metric="plane", sample_fraction=1, target_d=1e-4), engine=e).run(
            src, tgt, mxa, mxb, target_normals="estimate")
    print("estimated normals: gicp %d iterations (mean_dist %.4g), plane %d iterations (mean_dist %.4g)"
          % (gicp.iters_done, gicp.mean_dist, plane.iters_done, plane.mean_dist))
    assert gicp.converged


@pytest.mark.gpu
def test_gpu_gicp_refusals_leave_the_context_usable():
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    src, sn, verts, tris, mxa, mxb = table_case()

    def gicp_loop_ok(e):
        e.set_matrices(mxa, mxb)
        r = e.run(iters=3, thresh=0.5, target_d=0.01)
        assert r.iters_done >= 1 and np.all(np.isfinite(r.matrix_world))

    def refused(e, code, match, call=None):
        with pytest.raises(_capi.OaError, match=match) as ei:
            (call or (lambda: e.run(iters=3, thresh=0.5, target_d=0.01)))()
        assert ei.value.code == code

    with IcpEngine(0) as e:
        e.set_metric("gicp")
        e.set_target_mesh(verts, tris)
        e.set_source(src, stride=1)
        e.set_matrices(mxa, mxb)
        refused(e, _capi.OA_E_STATE, "oa_set_source_normals")       # no source normals
        refused(e, _capi.OA_E_STATE, "oa_set_source_normals", lambda: e.iterate())
        refused(e, _capi.OA_E_BAD_ARG, "source normals for", lambda: e.set_source_normals(sn[:-1]))     # wrong n_verts
        e.set_source_normals(sn)
        gicp_loop_ok(e)
        refused(e, _capi.OA_E_BAD_ARG, "with_scale", lambda: e.run(iters=3, with_scale=True))
        refused(e, _capi.OA_E_BAD_ARG, "with_scale", lambda: e.iterate(with_scale=True))
        refused(e, _capi.OA_E_STATE, "oa_set_metric", lambda: e.run_begin(iters=3))
        gicp_loop_ok(e)
        # the estimated robust scale: refused together with a loss, inert without one
        e.set_robust_auto(0.5, 1e-4)
        gicp_loop_ok(e)
        e.set_robust("huber", 1.5)
        refused(e, _capi.OA_E_STATE, "oa_set_robust_auto")
        e.set_robust_auto(0.0, 0.0)
        gicp_loop_ok(e)
        e.set_robust("none")
        # epsilon
        for bad in (0.0, 9e-7, 1.0000001, -1e-3, float("nan"), float("inf")):
            refused(e, _capi.OA_E_BAD_ARG, "epsilon", lambda: e.set_gicp(bad))
        e.set_gicp(1e-6)
        e.set_gicp(1.0)
        e.set_gicp(1e-3)
        gicp_loop_ok(e)
        # a new source upload forgets the normals; switching the normal-angle test off keeps them
        e.set_source(src, stride=1)
        e.set_matrices(mxa, mxb)
        refused(e, _capi.OA_E_STATE, "oa_set_source_normals")
        e.set_normals(sn, None, max_angle_deg=60.0)
        e.set_normals(None)
        gicp_loop_ok(e)
        # a vertex-mode target without normals
        e.set_target(verts)
        e.set_matrices(mxa, mxb)
        refused(e, _capi.OA_E_STATE, "oa_set_target_normals")
        e.set_target_mesh(verts, tris)
        gicp_loop_ok(e)
    with IcpEngine(0) as fresh:
        refused(fresh, _capi.OA_E_STATE, "oa_set_source first", lambda: fresh.set_source_normals(sn))
    with IcpEngine(devices=[0, 0]) as m:
        m.set_target_mesh(verts, tris)
        m.set_source(src, stride=1)
        m.set_source_normals(sn)                                    # routed to every child
        m.set_matrices(mxa, mxb)
        m.set_metric("gicp")
        refused(m, _capi.OA_E_STATE, "single-device")
        refused(m, _capi.OA_E_STATE, "single-device", lambda: m.iterate())
        m.set_metric("point")
        m.set_matrices(mxa, mxb)
        r = m.run(iters=3, thresh=0.5, target_d=0.01)
        assert r.iters_done >= 1 and np.all(np.isfinite(r.matrix_world))
