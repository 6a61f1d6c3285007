"""Point-to-plane ICP (Chen & Medioni): oa_set_metric / oa_set_target_normals / oa_point_to_plane, IcpSettings.metric.

The CPU reference of the plane step lives here: numpy, fp64, numpy.linalg.eigh, the 1e-10 x lambda_max cut, Rodrigues --
on top of the oracle's correspondences (nn_tri_brute / nn_brute) and its float32 helpers, which give the engine's pairs
bit for bit.  The engine is held to it one step at a time: before every step the device's matrix_world goes to the
reference, so a last-bit difference in one step cannot move a correspondence in the next.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from object_alignment_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIG_CUT = 1e-10
TOL = 1e-9          # the bound DESIGN 5.2 holds every per-iteration M to


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


def plane_solve(a, b, n, c, reverse=False):
    """a, b, n: K x 3 (n need not be unit); pivot c.  Returns (M 4x4, rank).  K < 3: the reference's ValueError."""
    a, b, n = (np.asarray(x, np.float64) for x in (a, b, n))
    n2 = np.einsum("ij,ij->i", n, n)
    ok = np.isfinite(n2) & (n2 > 0.0)
    a, b, n = a[ok], b[ok], n[ok] / np.sqrt(n2[ok])[:, None]
    if len(a) < 3:
        raise ValueError("input arrays are of wrong shape or type")
    if reverse:
        a, b, n = a[::-1], b[::-1], n[::-1]
    a = a - c
    b = b - c
    r = np.einsum("ij,ij->i", n, a - b)
    J = np.concatenate([np.cross(a, n), n], axis=1)
    H, g = J.T @ J, J.T @ r
    lam, V = np.linalg.eigh(H)
    keep = lam > EIG_CUT * lam.max()
    x = -(V[:, keep] @ ((V[:, keep].T @ g) / lam[keep]))
    R = rodrigues(x[:3])
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = c + x[3:] - R @ c
    return M, int(keep.sum())


def selection(n_verts, vlist, stride):
    sel = np.arange(n_verts) if vlist is None else np.asarray(vlist, np.int64)
    return sel[::stride] if stride > 1 else sel


def ref_pairs(orc, src_sel, mx1, mx2, tgt, tris=None, tgt_normals=None, thresh=0.5, src_normals_sel=None, max_angle_deg=None):
    """The pairs of one step as the engine forms them: (a, b, n_align_local, dist), fp64 from the float32 values."""
    mx1, mx2 = np.asarray(mx1, np.float32), np.asarray(mx2, np.float32)
    imx1, imx2 = orc.mat4_inverted(mx1), orc.mat4_inverted(mx2)
    tgt = np.asarray(tgt, np.float32)
    w = np.array([orc.mat4_mul_vec3(imx2, orc.mat4_mul_vec3(mx1, p)) for p in src_sel], np.float32)      # co_find
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
    A, B, N, D = [], [], [], []
    i1t, i2t, m1t = imx1[:3, :3].astype(np.float64).T, imx2[:3, :3].astype(np.float64).T, mx1[:3, :3].astype(np.float64).T
    cos_min = None if max_angle_deg is None else np.cos(max_angle_deg * 3.14159265358979323846 / 180.0)
    for k in range(len(src_sel)):
        wa, wb = orc.mat4_mul_vec3(mx2, w[k]), orc.mat4_mul_vec3(mx2, co1[k])
        dist = orc.vec3_length(wa - wb)
        if not dist < thresh:
            continue
        nw = i2t @ tn[k].astype(np.float64)                      # base-local -> world: inverse transpose of mx2
        if cos_min is not None:
            sw = i1t @ src_normals_sel[k].astype(np.float64)
            cc = (sw @ nw) / np.sqrt((sw @ sw) * (nw @ nw))
            if not cc >= cos_min:
                continue
        nl = m1t @ nw                                            # world -> align-local: mx1^T
        n2 = nl @ nl
        if not (np.isfinite(n2) and n2 > 0.0):
            continue
        A.append(src_sel[k].astype(np.float64))
        B.append(orc.mat4_mul_vec3(imx1, wb).astype(np.float64))
        N.append(nl / np.sqrt(n2))
        D.append(dist)
    return np.array(A).reshape(-1, 3), np.array(B).reshape(-1, 3), np.array(N).reshape(-1, 3), np.array(D)


def ref_step(orc, src_sel, mx1, mx2, tgt, **kw):
    """One plane step from matrix_world mx1: dict(M, new_mat, mw, K, mean, std, rank, M_rev)."""
    A, B, N, D = ref_pairs(orc, src_sel, mx1, mx2, tgt, **kw)
    c = src_sel[0].astype(np.float64)
    M, rank = plane_solve(A, B, N, c)
    M_rev, _ = plane_solve(A, B, N, c, reverse=True)
    new_mat = M.astype(np.float32)
    return dict(M=M, M_rev=M_rev, new_mat=new_mat, mw=orc.mat4_mul(np.asarray(mx1, np.float32), new_mat), K=len(A),
                mean=float(np.mean(D)), std=float(np.std(D)), rank=rank)


def ref_loop(orc, src_sel, mx1, mx2, tgt, iters=50, target_d=1e-4, **kw):
    """The reference's loop (5-slot ring of step lengths against target_d) around the plane step."""
    mx1 = np.asarray(mx1, np.float32).copy()
    ring = [2.0 * target_d] * 5
    out = dict(iters_done=0, converged=False, mean=None)
    for n in range(iters):
        s = ref_step(orc, src_sel, mx1, mx2, tgt, **kw)
        mx1 = s["mw"]
        ring[n % 5] = orc.vec3_length(s["new_mat"][:3, 3])
        out.update(iters_done=n + 1, mean=s["mean"], matrix_world=mx1)
        if all(t < target_d for t in ring):
            out["converged"] = True
            break
    return out


def table_case(rotvec=(0.10, -0.07, 0.12), t=(0.05, -0.03, 0.02)):
    """The issue's case: 5 000 bunny points on the 19 200-triangle cubed sphere, mx_base = I, mx_align = the inverse pose."""
    src = synth.bunny_surface(5000, 0.5)
    verts, tris = synth.cubed_surface_mesh(40)
    P = synth.rigid4(synth.rotation_from_rotvec(list(rotvec)), list(t), dtype=np.float64)
    mxa = np.linalg.inv(P).astype(np.float32)
    return src, verts, tris, mxa, np.eye(4, dtype=np.float32)


def scaled_base():
    R = synth.rotation_from_rotvec([0.3, -0.2, 0.25]).astype(np.float64)
    B = np.eye(4)
    B[:3, :3] = R @ np.diag([1.25, 0.8, 1.1])
    B[:3, 3] = [0.4, -0.3, 0.2]
    return B


# ------------------------------------------------------------------------------------------------ CPU
def test_plane_abi_and_bindings(built):
    """Fails without the feature: the header, the library, the bindings and the settings all name the plane metric."""
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators.icp_align import IcpSettings
    hdr = open(os.path.join(ROOT, "include", "oa_icp.h")).read()
    for fn in ("oa_set_metric", "oa_set_target_normals", "oa_point_to_plane"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, hdr), fn
        assert fn in _capi.SYMBOLS
    for name, val in (("OA_METRIC_POINT", 0), ("OA_METRIC_PLANE", 1), ("OA_STAT_METRIC", 28), ("OA_STAT_PLANE_RANK", 29)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name
    L = C.CDLL(os.path.join(ROOT, "object_alignment_amd", "liboa_icp.so"))
    for fn in ("oa_set_metric", "oa_set_target_normals", "oa_point_to_plane"):
        assert hasattr(L, fn), fn
    LL = _capi.load()
    assert LL.oa_point_to_plane.argtypes is not None and LL.oa_set_metric.argtypes is not None and LL.oa_set_target_normals.argtypes is not None
    assert (_capi.OA_METRIC_POINT, _capi.OA_METRIC_PLANE) == (0, 1)
    assert IcpEngine.STATS["metric"] == 28 and IcpEngine.STATS["plane_rank"] == 29
    assert IcpSettings().metric == "point"
    assert C.sizeof(_capi.Settings) == 32 and C.sizeof(_capi.Report) == 72
    assert "OA_NSUMS 24" in hdr                                    # the multi-GPU exchange keeps its width


def test_reference_plane_loop_beats_point_loop(orc):
    """The yardstick itself (passes without the feature): on the issue's case the reference's plane loop converges in fewer
    iterations than the oracle's point loop and ends closer; and its step does not depend on the order the pairs are summed in."""
    src, verts, tris, mxa, mxb = table_case()
    point = orc.icp_run(src, verts, mxa, mxb, iters=50, sample=1, thresh=0.5, target_d=1e-4, use_target=True, tris=tris)
    first = ref_step(orc, src, mxa, mxb, verts, tris=tris, thresh=0.5)
    assert np.max(np.abs(first["M"] - first["M_rev"])) < TOL
    assert first["rank"] == 6
    plane = ref_loop(orc, src, mxa, mxb, verts, iters=50, target_d=1e-4, tris=tris, thresh=0.5)
    print("point-to-point: %d iterations, mean %.3g; point-to-plane: %d iterations, mean %.3g"
          % (point["iters_done"], point["mean_dist"], plane["iters_done"], plane["mean"]))
    assert point["converged"] and plane["converged"]
    assert plane["iters_done"] < point["iters_done"]
    assert plane["mean"] < point["mean_dist"]


def test_rodrigues_is_a_rotation():
    for w in ([0.0, 0.0, 0.0], [1e-9, -2e-9, 1e-9], [3e-5, 1e-5, -2e-5], [0.3, -0.2, 0.1], [2.0, 1.0, -2.5]):
        R = rodrigues(np.array(w))
        assert np.max(np.abs(R @ R.T - np.eye(3))) < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14


# ------------------------------------------------------------------------------------------------ GPU
def ulp_diff32(a, b):
    a, b = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    return np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64))


def step_parity(orc, eng, src_sel, mxb, tgt, steps, **kw):
    for it in range(steps):
        mw = eng.matrix_world()
        ref = ref_step(orc, src_sel, mw, mxb, tgt, **kw)
        assert np.max(np.abs(ref["M"] - ref["M_rev"])) < TOL, "the case is ill-conditioned for the reference itself"
        M, st = eng.iterate(thresh=kw.get("thresh", 0.5), target_d=1e-4)
        _, sN, _, _, _ = eng._history(1)
        dM = float(np.max(np.abs(M - ref["M"])))
        print("step %d: K %d / %d, |dM| %.3g, d mean %.3g, d std %.3g, new_mat ulps %.3g, rank %d / %d"
              % (it, st["K"], ref["K"], dM, abs(st["mean_dist"] - ref["mean"]), abs(st["std_dist"] - ref["std"]),
                 ulp_diff32(sN[-1], ref["new_mat"]), int(eng.stat("plane_rank")), ref["rank"]))
        assert st["K"] == ref["K"]
        assert dM <= TOL
        assert abs(st["mean_dist"] - ref["mean"]) <= TOL and abs(st["std_dist"] - ref["std"]) <= TOL
        assert ulp_diff32(sN[-1], ref["new_mat"]) <= 1.0
        assert int(eng.stat("plane_rank")) == ref["rank"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["surface", "scaled_base", "vertex_normals", "normal_test", "vlist_stride2",
                                  "mode_brute", "mode_grid", "mode_bvh"])
def test_gpu_plane_step_parity(orc, case):
    from object_alignment_amd.engine import IcpEngine
    src, verts, tris, mxa, mxb = table_case()
    steps, vlist, stride, kw = 4, None, 1, dict(thresh=0.5)
    with IcpEngine(0) as e:
        e.set_metric("plane")
        assert e.stat("metric") == 1.0
        if case == "surface":
            steps = 10
        if case.startswith("mode_"):
            e.set_search_mode(case[5:])
            steps = 3
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
            pts, sn = synth.bunny_surface_with_normals(5000, 0.5)
            assert np.array_equal(np.asarray(pts, np.float32), np.asarray(src, np.float32))
            e.set_normals(sn, None, max_angle_deg=60.0)
            kw.update(src_normals_sel=np.asarray(sn, np.float32)[sel], max_angle_deg=60.0)
        e.set_matrices(mxa, mxb)
        assert e.stat("metric") == 1.0                              # survives the uploads and set_matrices
        step_parity(orc, e, np.asarray(src, np.float32)[sel], mxb, tgt, steps, **kw)


@pytest.mark.gpu
def test_gpu_plane_loop_converges_sooner_than_point():
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings
    src, verts, tris, mxa, mxb = table_case()
    res = {}
    with IcpEngine(0) as e:
        for metric in ("point", "plane"):
            st = IcpSettings(metric=metric, sample_fraction=1, target_d=1e-4)
            res[metric] = IcpAlign(st, engine=e).run(src, verts, mxa, mxb, target_tris=tris)
            assert e.stat("metric") == (1.0 if metric == "plane" else 0.0)
    print("iterations point %d, plane %d; mean_dist point %.3g, plane %.3g"
          % (res["point"].iters_done, res["plane"].iters_done, res["point"].mean_dist, res["plane"].mean_dist))
    assert res["plane"].converged and res["point"].converged
    assert res["plane"].iters_done < res["point"].iters_done
    assert res["plane"].mean_dist <= res["point"].mean_dist


def _p2p_check(e, a, b, n, rank=None):
    M = e.point_to_plane(a.T, b.T, n.T)
    ref, rrank = plane_solve(a, b, n, a[0].astype(np.float64))
    assert np.max(np.abs(M - ref)) <= TOL, np.max(np.abs(M - ref))
    assert int(e.stat("plane_rank")) == rrank
    if rank is not None:
        assert rrank == rank
    return M


@pytest.mark.gpu
def test_gpu_point_to_plane_alone():
    from object_alignment_amd.engine import IcpEngine
    rng = np.random.default_rng(7)
    with IcpEngine(0) as e:
        for K in (6, 64, 100000):
            a = rng.normal(size=(K, 3))
            n = rng.normal(size=(K, 3))
            b = a + 0.05 * rng.normal(size=(K, 3))
            _p2p_check(e, a, b, n, rank=6)
        K = 2000
        # a plane with one normal: rank 3 -- no in-plane translation, no rotation about the normal
        a = np.c_[rng.normal(size=(K, 2)), np.zeros(K)]
        n = np.tile([0.0, 0.0, 1.0], (K, 1))
        tilt = synth.rotation_from_rotvec([0.02, -0.03, 0.0]).astype(np.float64)
        b = a @ tilt.T + np.array([0.1, 0.2, 0.05])
        M = _p2p_check(e, a, b, n, rank=3)
        c = a[0]
        step_t = M[:3, :3] @ c + M[:3, 3] - c                      # t of (omega, t) about the pivot
        w = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) * 0.5
        size = np.linalg.norm(step_t) + np.linalg.norm(w)
        assert size > 1e-3
        assert abs(step_t[0]) <= 1e-9 * size and abs(step_t[1]) <= 1e-9 * size and abs(w[2]) <= 1e-9 * size
        # non-unit normals: the result of the normalised ones
        M2 = e.point_to_plane(a.T, b.T, (n * rng.uniform(0.1, 10.0, size=(K, 1))).T)
        assert np.max(np.abs(M2 - M)) <= TOL
        # a sphere with radial normals: rank 3 (rotations about the centre are invisible)
        a = rng.normal(size=(K, 3))
        a /= np.linalg.norm(a, axis=1, keepdims=True)
        _p2p_check(e, a, a + np.array([0.02, -0.01, 0.03]), a.copy(), rank=3)
        # a cylinder: rank 4
        t = rng.uniform(0, 2 * np.pi, K)
        a = np.c_[np.cos(t), np.sin(t), rng.normal(size=K)]
        n = np.c_[np.cos(t), np.sin(t), np.zeros(K)]
        _p2p_check(e, a, a + np.array([0.02, -0.01, 0.5]), n, rank=4)
        with pytest.raises(ValueError, match="input arrays are of wrong shape or type"):
            e.point_to_plane(np.zeros((3, 2)), np.zeros((3, 2)), np.ones((3, 2)))
        assert e.stat("metric") == 0.0                              # the call does not look at the metric, nor set it


@pytest.mark.gpu
def test_gpu_plane_search_modes_agree_bitwise():
    from object_alignment_amd.engine import IcpEngine
    src, verts, tris, mxa, mxb = table_case()
    hist = {}
    for mode in ("brute", "grid", "bvh", "auto", "auto"):
        with IcpEngine(0) as e:
            e.set_metric("plane")
            e.set_search_mode(mode)
            e.set_target_mesh(verts, tris)
            e.set_source(src, stride=1)
            e.set_matrices(mxa, mxb)
            r = e.run(iters=8, thresh=0.5, target_d=1e-4, early_exit=False)
        assert r.iters_done == 8
        hist.setdefault(mode, []).append((r.step_M.copy(), r.step_new.copy(), r.step_K.copy(), r.matrix_world.copy()))
    first = hist["brute"][0]
    for mode, runs in hist.items():
        for run in runs:
            for x, y in zip(first, run):
                assert np.array_equal(x, y), mode


def _point_history(e, src, tgt, mxa, mxb, tris=None, mode=None, iters=15):
    if mode:
        e.set_search_mode(mode)
    if tris is not None:
        e.set_target_mesh(tgt, tris)
    else:
        e.set_target(tgt)
    e.set_source(src, stride=1)
    e.set_matrices(mxa, mxb)
    r = e.run(iters=iters, thresh=0.5, target_d=0.01, early_exit=False)
    return r, e.stat("fast_iterations")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cloud", "surface"])
def test_gpu_point_metric_unmoved_by_a_visit_to_plane(kind):
    from object_alignment_amd.engine import IcpEngine
    if kind == "cloud":
        src, tgt, mxa, mxb = synth.c2_bunny_pair(100000)
        tris, mode = None, "grid"
    else:
        src, tgt, tris, mxa, mxb = table_case()
        mode = None
    with IcpEngine(0) as e:
        plain, fast0 = _point_history(e, src, tgt, mxa, mxb, tris, mode)
    with IcpEngine(0) as e:
        e.set_metric("plane")
        e.set_metric("point")
        back, fast1 = _point_history(e, src, tgt, mxa, mxb, tris, mode)
    if kind == "cloud":
        assert fast0 > 0 and fast1 > 0                              # the fused path ran in both
    for name in ("step_M", "step_new", "step_K", "step_stats", "step_trans", "matrix_world"):
        assert np.array_equal(getattr(plain, name), getattr(back, name)), name


@pytest.mark.gpu
def test_gpu_plane_refusals_leave_the_context_usable():
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    src, verts, tris, mxa, mxb = table_case()

    def point_loop_ok(e):
        e.set_metric("point")
        e.set_matrices(mxa, mxb)
        r = e.run(iters=5, thresh=0.5, target_d=0.01)
        assert r.iters_done >= 1 and np.all(np.isfinite(r.matrix_world))

    with IcpEngine(0) as e:
        e.set_target_mesh(verts, tris)
        e.set_source(src, stride=1)
        e.set_matrices(mxa, mxb)
        e.set_metric("plane")
        with pytest.raises(_capi.OaError, match="with_scale") as ei:
            e.run(iters=5, with_scale=True)
        assert ei.value.code == _capi.OA_E_BAD_ARG
        with pytest.raises(_capi.OaError, match="with_scale"):
            e.iterate(with_scale=True)
        with pytest.raises(_capi.OaError, match="oa_set_metric") as ei:
            e.run_begin(iters=5)
        assert ei.value.code == _capi.OA_E_STATE
        point_loop_ok(e)
        # a vertex-mode target without normals
        e.set_target(verts)
        e.set_matrices(mxa, mxb)
        e.set_metric("plane")
        with pytest.raises(_capi.OaError, match="oa_set_target_normals") as ei:
            e.run(iters=5)
        assert ei.value.code == _capi.OA_E_STATE
        point_loop_ok(e)
        with pytest.raises(ValueError):
            e.set_metric("planar")
    with IcpEngine(devices=[0, 0]) as m:
        m.set_target_mesh(verts, tris)
        m.set_source(src, stride=1)
        m.set_matrices(mxa, mxb)
        m.set_metric("plane")
        with pytest.raises(_capi.OaError, match="single-device") as ei:
            m.run(iters=5)
        assert ei.value.code == _capi.OA_E_STATE
        with pytest.raises(_capi.OaError, match="single-device"):
            m.iterate()
        point_loop_ok(m)
