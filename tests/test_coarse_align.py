"""Coarse global alignment: batched pose scoring (oa_score_poses), the rotation candidates (oa_coarse_candidates) and the
multi-start recipe (oa_coarse_align, IcpAlign.run(coarse=...)).

The reference for a score is the pinned CPU restatement oracle.make_pairs(..., sample=stride, calc_stats=True) per pose: K from
its pair count, mean / std from its d_stats, cost = (K mean + (S - K) thresh) / S.  K is exact; mean, std and cost agree to 1e-9
relative, the bound of every d_stats comparison in this suite.  The recipe itself is restated here in numpy (nearest vertex,
Kabsch) -- that restatement guards the fixture of the capability test on the CPU.
"""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

from object_alignment_amd import _hostmath, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-9
PSI = 1.533751168755204288118041


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build_hip()
    return g


# ------------------------------------------------------------------------------------------------ numpy restatements
def super_fibonacci(n):
    """(n, 4) unit quaternions (x, y, z, w) of the n-point super-Fibonacci set on SO(3) (Alexa 2022)."""
    s = np.arange(n, dtype=np.float64) + 0.5
    r, R = np.sqrt(s / n), np.sqrt(1.0 - s / n)
    a, b = 2.0 * np.pi * s / np.sqrt(2.0), 2.0 * np.pi * s / PSI
    return np.stack([r * np.sin(a), r * np.cos(a), R * np.sin(b), R * np.cos(b)], axis=1)


def quat_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)


def trans4(t):
    m = np.identity(4)
    m[:3, 3] = t
    return m


def candidates_numpy(src_sel, tgt, mx_align, mx_base, n):
    """float32(T(c_t) R_k T(-c_s) mx_align): fp64 centroids of the float32 matrix @ vertex images, the closed form above."""
    cs = np.mean([_hostmath.mat4_mul_vec3(mx_align, v).astype(np.float64) for v in src_sel], axis=0)
    ct = np.mean([_hostmath.mat4_mul_vec3(mx_base, v).astype(np.float64) for v in tgt], axis=0)
    right = trans4(-cs) @ np.asarray(mx_align, np.float64)
    out = np.empty((n, 4, 4), np.float32)
    for k, q in enumerate(super_fibonacci(n)):
        R = np.identity(4)
        R[:3, :3] = quat_matrix(q)
        out[k] = (trans4(ct) @ (R @ right)).astype(np.float32)
    return out


def asym_shape(n, off=0.0):
    """bunny_surface made clearly asymmetric: one radial bump and an anisotropic scale (the plain surface is nearly symmetric
    under a half turn and scores the flipped pose within 3 % of the true one)."""
    p = synth.bunny_surface(n, off).astype(np.float64)
    u = p / np.linalg.norm(p, axis=1, keepdims=True)
    p = p + 0.9 * np.exp(-np.sum((u - np.array([0.6, 0.64, 0.48])) ** 2, axis=1) / 0.15)[:, None] * u
    return (p * np.array([1.0, 0.75, 0.55])).astype(np.float32)


STARTS = [(2.4, 0.3, -0.5), (0.2, -2.9, 0.4), (-1.9, 1.5, 1.1)]
START_T = (0.4, -0.3, 0.25)


@functools.lru_cache(maxsize=None)
def capability_case():
    return asym_shape(3000), asym_shape(1500, 0.37)


def start_pose(rv):
    return synth.rigid4(synth.rotation_from_rotvec(rv), START_T)


def pose_error(M):
    """(rotation angle in degrees, |translation|) of a 4x4 against the identity."""
    M = np.asarray(M, np.float64)
    c = (np.trace(M[:3, :3]) - 1.0) / 2.0
    return math.degrees(math.acos(max(-1.0, min(1.0, c)))), float(np.linalg.norm(M[:3, 3]))


def kabsch_numpy(a, b):
    """The rigid 4x4 that carries the rows of a onto those of b (least squares)."""
    ca, cb = a.mean(axis=0), b.mean(axis=0)
    U, _, Vt = np.linalg.svd((b - cb).T @ (a - ca))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    M = np.identity(4)
    M[:3, :3] = U @ D @ Vt
    M[:3, 3] = cb - M[:3, :3] @ ca
    return M


class NumpyRecipe:
    """The recipe of oa_coarse_align and the loop behind it in plain numpy: base = identity, nearest target vertex."""

    def __init__(self, orc, src_sel, tgt):
        self.kd = orc.KDTree(tgt)
        self.tgt = np.asarray(tgt, np.float64)
        self.sel = np.asarray(src_sel, np.float64)

    def nearest(self, w):
        idx, _ = self.kd.query(w.astype(np.float32))
        q = self.tgt[np.asarray(idx)]
        return q, np.linalg.norm(w - q, axis=1)

    def cost(self, M, pts, thresh):
        _, d = self.nearest(pts @ M[:3, :3].T + M[:3, 3])
        return float(np.mean(np.minimum(d, thresh)))

    def icp(self, M, pts, thresh, iters):
        M = np.array(M, np.float64)
        for _ in range(iters):
            w = pts @ M[:3, :3].T + M[:3, 3]
            q, d = self.nearest(w)
            keep = d < thresh
            if keep.sum() < 3:
                break
            M = kabsch_numpy(w[keep], q[keep]) @ M
        return M

    def coarse(self, M0, n_rot=256, n_refine=8, refine_iters=10, stride=4, thresh=None):
        M0 = np.asarray(M0, np.float64)
        sample = self.sel[::stride]
        if thresh is None:
            thresh = 0.1 * float(np.linalg.norm(self.tgt.max(axis=0) - self.tgt.min(axis=0)))
        cs = (self.sel @ M0[:3, :3].T + M0[:3, 3]).mean(axis=0)
        ct = self.tgt.mean(axis=0)
        right = trans4(-cs) @ M0
        cand = []
        for q in super_fibonacci(n_rot):
            R = np.identity(4)
            R[:3, :3] = quat_matrix(q)
            cand.append(trans4(ct) @ R @ right)
        cand.append(M0)
        costs = np.array([self.cost(M, sample, thresh) for M in cand])
        pick = list(np.argsort(costs, kind="stable")[:n_refine])
        if n_rot not in pick:
            pick[-1] = n_rot
        refined = [self.icp(cand[k], sample, thresh, refine_iters) for k in pick]
        rc = np.array([self.cost(M, sample, thresh) for M in refined])
        win = int(np.argmin(rc))
        return refined[win] if rc[win] < costs[n_rot] else M0


def score_reference(orc, src, tgt, poses, mx_base, thresh, stride=1, vlist=None, tris=None):
    """(P, 4) [K, mean, std, cost] from oracle.make_pairs, and S."""
    n_all = len(vlist) if vlist is not None else len(src)
    step = stride if stride > 1 else 1
    S = (n_all + step - 1) // step
    kd = orc.KDTree(tgt) if tris is None else None
    out = np.empty((len(poses), 4), np.float64)
    for p, M in enumerate(poses):
        A, _, ds = orc.make_pairs(src, tgt, M, mx_base, thresh, vlist=vlist, sample=stride, calc_stats=True, kd=kd, tris=tris)
        K = A.shape[1]
        mean, std = (ds[0], ds[1]) if K > 0 else (np.nan, np.nan)
        out[p] = [K, mean, std, ((K * mean if K > 0 else 0.0) + (S - K) * thresh) / S]
    return out, S


def assert_scores(got, ref, what=""):
    assert got.shape == ref.shape, what
    assert np.array_equal(got[:, 0], ref[:, 0]), "%s K: %s vs %s" % (what, got[:, 0], ref[:, 0])
    for col, name in ((1, "mean"), (2, "std"), (3, "cost")):
        g, r = got[:, col], ref[:, col]
        assert np.array_equal(np.isnan(g), np.isnan(r)), "%s %s NaN pattern" % (what, name)
        ok = ~np.isnan(r)
        print(what, name, "max rel err", float(np.max(np.abs(g[ok] - r[ok]) / np.maximum(np.abs(r[ok]), 1e-300))) if ok.any() else 0.0)
        assert np.allclose(g[ok], r[ok], rtol=RTOL, atol=0.0), "%s %s: %s vs %s" % (what, name, g, r)


def base_scaled():
    """A base matrix with a rotation, a non-uniform scale and a translation."""
    M = np.identity(4)
    M[:3, :3] = synth.rotation_from_rotvec([0.3, -0.2, 0.5]) @ np.diag([1.2, 0.9, 1.1])
    M[:3, 3] = [0.3, -0.1, 0.2]
    return M.astype(np.float32)


def five_poses(mx_base):
    """identity, a 170 degree turn, far away (K = 0), about half of the points inside thresh, a scale of 1.5 -- all relative to
    the base matrix, so that the identity lays the source over the target."""
    B = np.asarray(mx_base, np.float64)
    far = trans4([100.0, 0.0, 0.0])
    half = trans4([0.33, 0.0, 0.0])
    big = np.diag([1.5, 1.5, 1.5, 1.0])
    turn = synth.rigid4(synth.rotation_from_rotvec([0.0, 0.0, math.radians(170.0)]), None, dtype=np.float64)
    return np.stack([(B @ D).astype(np.float32) for D in (np.identity(4), turn, far, half, big)])


THRESH = 0.25


# ------------------------------------------------------------------------------------------------ CPU tests
def test_struct_layouts_and_symbols(built):
    from object_alignment_amd import _capi
    assert C.sizeof(_capi.CoarseSettings) == 24
    assert C.sizeof(_capi.CoarseReport) == 64
    assert _capi.CoarseReport.K_refined.offset == 40 and _capi.CoarseSettings.thresh.offset == 16
    assert _capi.OA_POSE_NSCORE == 4
    header = open(os.path.join(ROOT, "include", "oa_icp.h")).read()
    assert re.search(r"#define\s+OA_POSE_NSCORE\s+4\b", header)
    L = _capi.load()
    for name in ("oa_score_poses", "oa_coarse_candidates", "oa_coarse_align"):
        assert name in _capi.SYMBOLS and hasattr(L, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    for field, _ in _capi.CoarseSettings._fields_ + _capi.CoarseReport._fields_:
        assert re.search(r"\b%s\b" % field, header), field


def test_super_fibonacci_units_and_covering():
    q = super_fibonacci(256)
    assert np.allclose(np.linalg.norm(q, axis=1), 1.0, rtol=0, atol=1e-15)
    for k in (0, 17, 255):
        R = quat_matrix(q[k])
        assert np.allclose(R @ R.T, np.identity(3), atol=1e-14) and abs(np.linalg.det(R) - 1.0) < 1e-14
    rng = np.random.default_rng(7)
    dense = rng.standard_normal((20000, 4))
    dense /= np.linalg.norm(dense, axis=1, keepdims=True)            # uniform on SO(3)
    angle = lambda probes: np.degrees(2.0 * np.arccos(np.minimum(1.0, np.max(np.abs(probes @ q.T), axis=1))))
    covering = float(np.max(angle(dense)))                          # the set's covering angle, measured on 20 000 rotations
    probe = float(np.max(angle(dense[:1000])))                      # the fixed probe set: the first 1 000 of them
    # n balls of angle t cover SO(3) only if n (t - sin t) / pi >= 1 (the Haar measure of a ball): the bound below which no
    # set of 256 rotations can get.  A cubic lattice covers 1.4 x as far as that bound, a random set several times as far
    lo, hi = 0.0, math.pi
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if 256 * (mid - math.sin(mid)) / math.pi < 1.0 else (lo, mid)
    bound = math.degrees(hi)
    print("super-Fibonacci n = 256: covering angle %.2f deg (1 000 probes: %.2f deg), volume bound %.2f deg" % (covering, probe, bound))
    assert probe <= covering
    assert bound <= covering <= 2.0 * bound


def test_coarse_settings_defaults_and_checks():
    from object_alignment_amd.operators import CoarseAlign, CoarseSettings     # noqa: F401  (both exported)
    s = CoarseSettings()
    assert (s.n_rot, s.n_refine, s.refine_iters, s.stride, s.thresh) == (256, 8, 10, 4, None)
    for bad in (dict(n_rot=0), dict(n_rot=65537), dict(n_refine=0), dict(refine_iters=-1), dict(stride=0), dict(thresh=0.0),
                dict(thresh=float("nan")), dict(n_rot=2.5)):
        with pytest.raises(ValueError):
            CoarseSettings(**bad)
    from object_alignment_amd.operators.coarse_align import default_thresh
    cube = np.array([[0, 0, 0], [1, 2, 2]], np.float32)
    assert default_thresh(cube, np.identity(4)) == pytest.approx(0.3)
    assert default_thresh(cube, np.diag([2.0, 2.0, 2.0, 1.0])) == pytest.approx(0.6)


def test_numpy_recipe_recovers_the_three_starts(orc):
    """Guards the fixture of the capability test: the restated recipe alone recovers every start, the plain loop none."""
    tgt, src = capability_case()
    sel = src[::2]                                                   # IcpSettings.sample_fraction = 0.5
    rec = NumpyRecipe(orc, sel, tgt)
    for rv in STARTS:
        M0 = start_pose(rv).astype(np.float64)
        plain = pose_error(rec.icp(M0, rec.sel, 0.5, 50))
        multi = pose_error(rec.icp(rec.coarse(M0), rec.sel, 0.5, 50))
        print("start %s: plain loop ends %.2f deg / %.4f away, multi-start %.3f deg / %.4f" % (rv, plain[0], plain[1], multi[0], multi[1]))
        assert plain[0] > 45.0
        assert multi[0] < 0.5 and multi[1] < 0.02


# ------------------------------------------------------------------------------------------------ GPU tests
@functools.lru_cache(maxsize=None)
def vertex_case():
    return synth.bunny_surface(300), synth.bunny_surface(257, 0.37)


def engine_for(tgt, src, mx_base, vlist=None, tris=None):
    from object_alignment_amd.engine import IcpEngine
    eng = IcpEngine(0)
    if tris is not None:
        eng.set_target_mesh(tgt, tris)
    else:
        eng.set_target(tgt)
    eng.set_source(src, vlist=vlist, stride=1)
    eng.set_matrices(np.identity(4, dtype=np.float32), mx_base)
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("base", ["scaled", "identity"])
def test_score_parity_vertex_mode(built, orc, base):
    tgt, src = vertex_case()
    mx_base = base_scaled() if base == "scaled" else np.identity(4, dtype=np.float32)
    poses = five_poses(mx_base)
    every_third_out = [i for i in range(len(src)) if i % 3 != 2]
    for stride, vlist in ((1, None), (4, None), (1, every_third_out), (4, every_third_out)):
        ref, S = score_reference(orc, src, tgt, poses, mx_base, THRESH, stride, vlist)
        assert ref[2, 0] == 0 and ref[2, 3] == THRESH                # far away: K = 0, cost = thresh
        assert 0.25 * S < ref[3, 0] < 0.75 * S, ref[3, 0]            # about half of the points pass
        with engine_for(tgt, src, mx_base, vlist) as eng:
            got = eng.score_poses(poses, THRESH, stride)
            again = eng.score_poses(poses, THRESH, stride)
        assert_scores(got, ref, "%s stride %d vlist %s" % (base, stride, vlist is not None))
        assert got.tobytes() == again.tobytes()
        assert np.isnan(got[2, 1]) and np.isnan(got[2, 2]) and got[2, 3] == THRESH


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 255, 256, 257])
def test_sample_counts_around_wave_and_workgroup_edges(built, orc, S):
    tgt, src = vertex_case()
    mx_base = base_scaled()
    poses = five_poses(mx_base)[[0, 3, 1]]
    vlist = list(range(S))
    ref, s_ref = score_reference(orc, src, tgt, poses, mx_base, THRESH, 1, vlist)
    assert s_ref == S
    with engine_for(tgt, src, mx_base, vlist) as eng:
        got = eng.score_poses(poses, THRESH, 1)
    assert_scores(got, ref, "S = %d" % S)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 2, 64, 65])
def test_pose_counts_and_no_leak_between_poses(built, orc, P):
    tgt, src = vertex_case()
    mx_base = base_scaled()
    B = mx_base.astype(np.float64)
    rng = np.random.default_rng(11)
    same = (B @ trans4([0.05, -0.02, 0.03])).astype(np.float32)
    poses = np.stack([same if p % 7 == 0 else
                      (B @ synth.rigid4(synth.rotation_from_rotvec(rng.uniform(-0.6, 0.6, 3)), rng.uniform(-0.2, 0.2, 3), dtype=np.float64)).astype(np.float32)
                      for p in range(P)])
    vlist = list(range(65))
    ref, _ = score_reference(orc, src, tgt, poses, mx_base, THRESH, 1, vlist)
    with engine_for(tgt, src, mx_base, vlist) as eng:
        got = eng.score_poses(poses, THRESH, 1)
    assert_scores(got, ref, "P = %d" % P)
    for p in range(0, P, 7):
        assert got[p].tobytes() == got[0].tobytes(), p


@pytest.mark.gpu
def test_score_parity_surface_mode(built, orc):
    verts, tris = synth.icosphere_mesh(2)
    verts = (verts.astype(np.float64) * np.array([1.0, 0.75, 0.55])).astype(np.float32)
    src = synth.bunny_surface(130)
    mx_base = base_scaled()
    poses = five_poses(mx_base)
    for stride in (1, 4):
        ref, S = score_reference(orc, src, verts, poses, mx_base, THRESH, stride, None, tris=tris)
        assert ref[2, 0] == 0 and 0 < ref[3, 0] < S
        with engine_for(verts, src, mx_base, tris=tris) as eng:
            assert eng.stat("surface") == 1.0
            got = eng.score_poses(poses, THRESH, stride)
            again = eng.score_poses(poses, THRESH, stride)
        assert_scores(got, ref, "surface stride %d" % stride)
        assert got.tobytes() == again.tobytes()


@pytest.mark.gpu
def test_no_side_effects(built):
    tgt, src = vertex_case()
    mx_base = base_scaled()
    mx_align = (mx_base.astype(np.float64) @ synth.rigid4(synth.rotation_from_rotvec([0.05, -0.04, 0.06]), [0.02, 0.01, -0.02], dtype=np.float64)).astype(np.float32)
    poses = five_poses(mx_base)

    def sequence(eng, disturb):
        eng.set_matrices(mx_align, mx_base)
        out = []
        if disturb:
            eng.score_poses(poses, THRESH, 2)
            eng.coarse_candidates(7)
        for k in range(5):
            if disturb and k in (2, 4):
                eng.score_poses(poses, THRESH, 1)
                eng.coarse_candidates(3)
            M, st = eng.iterate(thresh=0.5)
            out.append(M.tobytes())
            out.append(np.array([st["K"], st["mean_dist"], st["std_dist"], st["translation"], st["rot_angle"]]).tobytes())
            out.append(eng.matrix_world().tobytes())
        eng.set_matrices(mx_align, mx_base)
        if disturb:
            eng.score_poses(poses, THRESH, 1)
        res = eng.run(iters=5, thresh=0.5, early_exit=False)
        out += [res.matrix_world.tobytes(), res.step_M.tobytes(), res.step_K.tobytes(), res.step_stats.tobytes()]
        return out

    with engine_for(tgt, src, mx_base) as a, engine_for(tgt, src, mx_base) as b:
        assert sequence(a, False) == sequence(b, True)
        b.set_metric("plane")
        b.set_robust("huber", 0.1)
        before = (b.stat("metric"), b.stat("robust_loss"), b.stat("robust_scale"))
        rep = b.coarse_align(THRESH, n_rot=16, n_refine=3, refine_iters=2, stride=2)
        assert (b.stat("metric"), b.stat("robust_loss"), b.stat("robust_scale")) == before
        assert rep["cost_refined"] <= rep["cost_start"]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7, 256])
def test_candidates(built, n):
    tgt, src = vertex_case()
    mx_base = base_scaled()
    mx_align = (mx_base.astype(np.float64) @ synth.rigid4(synth.rotation_from_rotvec([0.4, 0.1, -0.3]), [0.2, 0.1, -0.1], dtype=np.float64)).astype(np.float32)
    vlist = [i for i in range(len(src)) if i % 3 != 2]
    with engine_for(tgt, src, mx_base, vlist) as eng:
        eng.set_matrices(mx_align, mx_base)
        got = eng.coarse_candidates(n)
        assert got.tobytes() == eng.coarse_candidates(n).tobytes()
    ref = candidates_numpy(src[vlist], tgt, mx_align, mx_base, n)
    assert got.shape == ref.shape == (n, 4, 4)
    ulp = np.spacing(np.max(np.abs(ref), axis=2, keepdims=True).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / ulp
    print("n = %d: largest difference %.2f ulp of the row's largest entry" % (n, float(err.max())))
    assert float(err.max()) <= 2.0


@pytest.mark.gpu
@pytest.mark.parametrize("rv", STARTS)
def test_capability_multi_start_recovers_what_the_loop_cannot(built, rv):
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators import CoarseSettings, IcpAlign, IcpSettings
    tgt, src = capability_case()
    eye = np.identity(4, dtype=np.float32)
    with IcpEngine(0) as eng:
        op = IcpAlign(IcpSettings(icp_iterations=50), engine=eng)
        # all 50 iterations, as in the numpy restatement: the reference's convergence test looks at the steps' translations
        # alone, and a loop that turns about the centroid passes it after five iterations, degrees away from where it would end
        plain = op.run(src, tgt, start_pose(rv), eye, early_exit=False, coarse=None)
        assert op.last_coarse is None
        res = op.run(src, tgt, start_pose(rv), eye, early_exit=False, coarse=CoarseSettings(n_rot=256))
        rep = op.last_coarse
        ang0, _ = pose_error(plain.matrix_world)
        ang, tr = pose_error(res.matrix_world)
        print("start %s: plain loop %.2f deg away; multi-start %.4f deg, %.5f; report %s" % (rv, ang0, ang, tr, {k: v for k, v in rep.items() if k != "matrix_world"}))
        assert ang0 > 45.0
        assert ang < 0.5 and tr < 0.02
        assert rep["cost_refined"] <= rep["cost_start"]
        assert rep["n_candidates"] == 256 and rep["status"] == 0
        # the reported winner's cost is the score of the matrix the stage left in force
        from object_alignment_amd.operators.coarse_align import default_thresh
        thresh = default_thresh(tgt, eye)
        eng.set_matrices(start_pose(rv), eye)
        rep2 = eng.coarse_align(thresh, n_rot=256)
        sc = eng.score_poses(rep2["matrix_world"], thresh, 4)
        assert sc[0, 3] == pytest.approx(rep2["cost_refined"], rel=RTOL, abs=0.0)
        assert sc[0, 0] == rep2["K_refined"]
        assert rep2["cost_refined"] == rep["cost_refined"]


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(built):
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    tgt, src = vertex_case()
    eye = np.identity(4, dtype=np.float32)
    poses = five_poses(eye)

    def refused(code, call, text=None):
        with pytest.raises(_capi.OaError) as ei:
            call()
        assert ei.value.code == code, ei.value
        if text:
            assert text in ei.value.msg

    with IcpEngine(0) as eng:
        eng.set_target(tgt)
        refused(_capi.OA_E_STATE, lambda: eng.score_poses(poses, THRESH))           # no source
        refused(_capi.OA_E_STATE, lambda: eng.coarse_candidates(4))
        eng.set_source(src, stride=1)
        refused(_capi.OA_E_STATE, lambda: eng.score_poses(poses, THRESH))           # no matrices
        refused(_capi.OA_E_STATE, lambda: eng.coarse_align(THRESH))
        eng.set_matrices(eye, eye)
        good = eng.score_poses(poses, THRESH)
        for thresh in (0.0, -1.0):
            refused(_capi.OA_E_BAD_THRESH, lambda: eng.score_poses(poses, thresh))
            refused(_capi.OA_E_BAD_THRESH, lambda: eng.coarse_align(thresh))
            assert eng.score_poses(poses, THRESH).tobytes() == good.tobytes()
        refused(_capi.OA_E_BAD_ARG, lambda: eng.score_poses(np.zeros((0, 4, 4), np.float32), THRESH))
        assert eng.score_poses(poses, THRESH).tobytes() == good.tobytes()
        bad = poses.copy()
        bad[1, 2, 3] = np.nan
        refused(_capi.OA_E_BAD_ARG, lambda: eng.score_poses(bad, THRESH))
        assert eng.score_poses(poses, THRESH).tobytes() == good.tobytes()
        refused(_capi.OA_E_BAD_ARG, lambda: eng.coarse_candidates(0))
        refused(_capi.OA_E_BAD_ARG, lambda: eng.coarse_align(THRESH, n_rot=0))
        assert eng.coarse_candidates(4).shape == (4, 4, 4)
        assert eng.coarse_align(THRESH, n_rot=8, n_refine=2, refine_iters=1)["status"] == 0
    with IcpEngine(devices=[0, 0]) as meng:
        meng.set_target(tgt)
        meng.set_source(src, stride=1)
        meng.set_matrices(eye, eye)
        refused(_capi.OA_E_STATE, lambda: meng.score_poses(poses, THRESH), "single-device")
        refused(_capi.OA_E_STATE, lambda: meng.coarse_candidates(4), "single-device")
        refused(_capi.OA_E_STATE, lambda: meng.coarse_align(THRESH), "single-device")
        assert meng.run(iters=2, thresh=0.5, early_exit=False).iters_done == 2
