"""The target's boundary (oa_target_boundary) and the rejection of pairs on it (oa_set_reject_boundary, IcpSettings.reject_boundary).

The contract (include/oa_icp.h).  Mesh: an undirected edge {u, v}, u != v, is a boundary edge iff exactly one triangle
lists both ends; a boundary vertex ends one; edge_mask[t] bit j = local edge j (ab, bc, ca), vertex_mask 0 / 1.  Cloud: for vertex
i with normal n, the first k entries of its k-nearest row of k + 1 that are not i, projected on the tangent basis u = normalise(n x e),
v = n^ x u (e: the axis of n's smallest component); flagged iff the largest gap between the sorted angles, the wrap-around included,
exceeds angle_deg pi / 180 -- or the normal is unusable, or fewer than 3 neighbours project.  A pair lies on the boundary iff its
closest point lies on a flagged edge or vertex of the winning triangle (closest_on_tri_region), or its winning vertex is flagged.

The numpy reference of both masks lives here (mesh_boundary_ref, cloud_boundary_ref).  The pairs are test_gicp_metric.ref_pairs'
(arrays; bit for bit test_plane_metric.ref_pairs', tests/test_trimmed.py), the regions tools/region_check.exe's: the library's own
float32 function compiled for the host.  The steps' solves are test_trimmed.solve's.
"""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_gicp_metric as G
from object_alignment_amd import synth
from test_deviation import closest_with_regions, host_regions
from test_plane_metric import TOL, scaled_base, selection
from test_reciprocal import THRESH, _kabsch, recip_keep, translation_error, upper_half, usual_pose, whole
from test_robust_weights import psi, world_scale
from test_trimmed import fixed_cut, residuals, solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_DEF, ANGLE_DEF = 16, 90.0


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build_hip()
    return g


# ------------------------------------------------------------------------------------------------ the reference: masks
def mesh_boundary_ref(n_verts, tris):
    """(vertex_mask uint8 (n_verts,), edge_mask uint8 (n_tris,)): integers only"""
    T = np.asarray(tris, np.int64).reshape(-1, 3)
    e0, e1 = T, np.roll(T, -1, axis=1)                              # local edges ab, bc, ca
    lo, hi = np.minimum(e0, e1), np.maximum(e0, e1)
    key = lo * int(n_verts) + hi
    proper = lo != hi
    # every undirected edge a triangle lists, once per triangle
    tk = np.stack([np.repeat(np.arange(len(T)), 3), key.ravel()], axis=1)[proper.ravel()]
    tk = np.unique(tk, axis=0)
    uniq, cnt = np.unique(tk[:, 1], return_counts=True)
    boundary = proper & np.isin(key, uniq[cnt == 1])
    edge_mask = (boundary * np.array([1, 2, 4])).sum(axis=1).astype(np.uint8)
    vertex_mask = np.zeros(n_verts, np.uint8)
    vertex_mask[e0[boundary]] = 1
    vertex_mask[e1[boundary]] = 1
    return vertex_mask, edge_mask


def knn_rows_ref(xyz, k1):
    """rows of k1 nearest indices (the vertex itself included), ascending (d2, index); fp64 on the float32 values; a non-finite
    distance never enters (-1 fills the row)"""
    X = np.asarray(xyz, np.float32).astype(np.float64)
    rows = np.full((len(X), k1), -1, np.int64)
    for i in range(len(X)):
        with np.errstate(all="ignore"):
            d = X - X[i]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        ok = np.flatnonzero(np.isfinite(d2))
        order = ok[np.lexsort((ok, d2[ok]))][:k1]
        rows[i, :len(order)] = order
    return rows


def cloud_boundary_ref(xyz, normals, rows, k=K_DEF, angle_deg=ANGLE_DEF):
    """(vertex_mask uint8, largest gap per vertex -- nan where the vertex is flagged for its normal or its neighbour count).
    rows: (n, k + 1) k-nearest rows (knn_rows_ref, or IcpEngine.target_knn(k + 1)[0])."""
    X = np.asarray(xyz, np.float32).astype(np.float64)
    Nn = np.asarray(normals, np.float32).astype(np.float64)
    thr = angle_deg * np.pi / 180.0
    mask = np.zeros(len(X), np.uint8)
    gaps = np.full(len(X), np.nan)
    for i in range(len(X)):
        n = Nn[i]
        l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        if not (l2 > 0.0 and np.isfinite(l2)):
            mask[i] = 1
            continue
        e = np.zeros(3)
        e[int(np.argmin(np.abs(n)))] = 1.0                          # (argmin: the lowest axis on ties)
        u = np.cross(n, e)
        u = u / np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
        v = np.cross(n / np.sqrt(l2), u)
        nb = [int(j) for j in rows[i] if j != i][:k]
        th = []
        for j in nb:
            if j < 0:
                continue
            with np.errstate(all="ignore"):
                d = X[j] - X[i]
                a, b = (d[0] * u[0] + d[1] * u[1]) + d[2] * u[2], (d[0] * v[0] + d[1] * v[1]) + d[2] * v[2]
            if not (np.isfinite(a) and np.isfinite(b)) or (a == 0.0 and b == 0.0):
                continue
            th.append(np.arctan2(b, a))
        if len(th) < 3:
            mask[i] = 1
            continue
        th = np.sort(np.array(th))
        gaps[i] = max(float(np.max(np.diff(th))), float(th[0] + 2.0 * np.pi - th[-1]))
        mask[i] = 1 if gaps[i] > thr else 0
    return mask, gaps


def near_threshold(gaps, angle_deg, band):
    return np.flatnonzero(np.abs(gaps - angle_deg * np.pi / 180.0) <= band)     # (nan compares false)


# ------------------------------------------------------------------------------------------------ the cases
def half_mesh(level=3):
    """the triangles of bumpy_icosphere_mesh(level) whose three vertices have z > 0 (all vertices stay)"""
    V, T = synth.bumpy_icosphere_mesh(level)
    V, T = np.asarray(V, np.float32), np.asarray(T, np.int32)
    return V, np.ascontiguousarray(T[np.all(V[T][:, :, 2] > 0, axis=1)])


@functools.lru_cache(maxsize=None)
def half_cloud():
    """bunny_surface_with_normals(4000, 0.0)[z > 0]: test_reciprocal.upper_half() with its analytic normals"""
    t, n = synth.bunny_surface_with_normals(4000, 0.0)
    t, n = np.asarray(t, np.float32), np.asarray(n, np.float32)
    keep = t[:, 2] > 0
    return np.ascontiguousarray(t[keep]), np.ascontiguousarray(n[keep])


def grid_cloud(n=9):
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), axis=-1).reshape(-1, 2)
    xyz = np.concatenate([g, np.zeros((len(g), 1))], axis=1).astype(np.float32)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (len(g), 1))
    ring = ((g == 0) | (g == n - 1)).any(axis=1)
    return xyz, nrm, ring


def mesh_cases():
    ico_v, ico_t = synth.icosphere_mesh(2)
    ico_v, ico_t = np.asarray(ico_v, np.float32), np.asarray(ico_t, np.int32)
    b2_v, b2_t = synth.bumpy_icosphere_mesh(2)
    b2_v, b2_t = np.asarray(b2_v, np.float32), np.asarray(b2_t, np.int32)
    quad = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1]], np.float32)
    cases = {
        "closed": (ico_v, ico_t),
        "one_triangle": (quad[:3], np.array([[0, 1, 2]], np.int32)),
        "two_triangles": (quad[:4], np.array([[0, 1, 2], [0, 2, 3]], np.int32)),
        "three_on_one_edge": (quad, np.array([[0, 2, 1], [0, 2, 3], [0, 2, 4]], np.int32)),
        "one_removed": (ico_v, ico_t[1:]),
        "half_bumpy3": half_mesh(3),
        # a triangle that lists a vertex twice: its proper edge counts, its u == u edge never does
        "vertex_twice": (quad, np.array([[0, 1, 2], [0, 2, 2], [2, 3, 3], [0, 2, 3], [4, 4, 4]], np.int32)),
        "lattice": tuple(np.asarray(a) for a in synth.lattice_surface_mesh(12, 16)),
    }
    for n in (1, 63, 64, 65, 257):
        cases["first_%d" % n] = (b2_v, np.ascontiguousarray(b2_t[:n]))
    return cases


MESH_CASES = ["closed", "one_triangle", "two_triangles", "three_on_one_edge", "one_removed", "half_bumpy3", "vertex_twice", "lattice",
              "first_1", "first_63", "first_64", "first_65", "first_257"]


# ------------------------------------------------------------------------------------------------ the reference: pairs
def rim_slots(orc, src_sel, mx1, mx2, tgt, tris, vmask, emask, tmp_path):
    """per selected source point: does its correspondence lie on the target's boundary.  Surface mode: triangle from
    orc.nn_tri_brute, region from closest_on_tri_region compiled for the host (test_deviation.host_regions)"""
    mx1, mx2 = np.asarray(mx1, np.float32), np.asarray(mx2, np.float32)
    tgt, src_sel = np.asarray(tgt, np.float32), np.asarray(src_sel, np.float32)
    w = G.m4v3(orc.mat4_inverted(mx2), G.m4v3(mx1, src_sel))       # co_find, as G.ref_pairs forms it
    if tris is None:
        idx, _ = orc.nn_brute(w, tgt)
        return vmask[idx] != 0
    face, _, _ = orc.nn_tri_brute(w, tgt, tris)
    T = np.asarray(tris, np.int64)[face]
    feat = host_regions(w, tgt[T[:, 0]], tgt[T[:, 1]], tgt[T[:, 2]], tmp_path)
    rim = np.zeros(len(w), bool)
    e = (feat >= 1) & (feat <= 3)
    rim[e] = ((emask[face[e]] >> (feat[e] - 1)) & 1) != 0
    v = feat >= 4
    rim[v] = vmask[T[v, feat[v] - 4]] != 0
    return rim


def bnd_pairs(orc, src_sel, sn_sel, mx1, mx2, tgt, tris, tn, vmask, emask, tmp_path, thresh=THRESH):
    """(P, rim): G.ref_pairs' pairs and, per pair, whether it lies on the boundary"""
    P = G.ref_pairs(orc, src_sel, sn_sel, mx1, mx2, tgt, tris=tris, tgt_normals=tn, thresh=thresh)
    rim = rim_slots(orc, src_sel, mx1, mx2, tgt, tris, vmask, emask, tmp_path)
    return P, rim[P["slot"]]


# ------------------------------------------------------------------------------------------------ the issue's table in numpy
def _end_error(M):
    ang = np.degrees(np.arccos(np.clip((np.trace(M[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))
    return float(np.linalg.norm(M[:3, 3])), float(ang)


@functools.lru_cache(maxsize=None)
def numpy_loop_cloud(reject, iters=60):
    """test_reciprocal.numpy_loop with the boundary rule: (translation error, rotation error, pairs in step 1, of them on the rim)"""
    from oracle import oracle as orc
    orc.build()
    src = whole().astype(np.float64)
    t32, n32 = half_cloud()
    tgt = t32.astype(np.float64)
    mask, _ = cloud_boundary_ref(t32, n32, knn_rows_ref(t32, K_DEF + 1))
    kt = orc.KDTree(tgt)
    M = usual_pose()[0].astype(np.float64)
    first = None
    for _ in range(iters):
        w = src @ M[:3, :3].T + M[:3, 3]
        j = kt.query(w)[0]
        q = tgt[j]
        keep = np.linalg.norm(w - q, axis=1) < THRESH
        if first is None:
            first = (int(keep.sum()), int((keep & (mask[j] != 0)).sum()))
        if reject:
            keep &= mask[j] == 0
        Mi = np.linalg.inv(M)
        b = q @ Mi[:3, :3].T + Mi[:3, 3]
        M = M @ _kabsch(src[keep], b[keep])
    return _end_error(M) + first


@functools.lru_cache(maxsize=None)
def numpy_loop_mesh(reject, iters=40):
    """the same on bunny_surface(2000, 0.5) against the z > 0 half of bumpy_icosphere_mesh(3): closest points, regions, fp64"""
    src = np.asarray(synth.bunny_surface(2000, 0.5), np.float32).astype(np.float64)
    V, T = half_mesh(3)
    vmask, emask = mesh_boundary_ref(len(V), T)
    M = usual_pose()[0].astype(np.float64)
    first = None
    for _ in range(iters):
        w = src @ M[:3, :3].T + M[:3, 3]
        face, q, feat, d2 = closest_with_regions(w, V, T)
        keep = np.sqrt(d2) < THRESH
        rim = np.zeros(len(w), bool)
        e = (feat >= 1) & (feat <= 3)
        rim[e] = ((emask[face[e]] >> (feat[e] - 1)) & 1) != 0
        v = feat >= 4
        rim[v] = vmask[T[face[v], feat[v] - 4]] != 0
        if first is None:
            first = (int(keep.sum()), int((keep & rim).sum()))
        if reject:
            keep &= ~rim
        Mi = np.linalg.inv(M)
        b = q @ Mi[:3, :3].T + Mi[:3, 3]
        M = M @ _kabsch(src[keep], b[keep])
    return _end_error(M) + first


# ------------------------------------------------------------------------------------------------ CPU
def test_boundary_abi_and_bindings(built):
    from object_alignment_amd import _capi, blender_addon
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators import icp_align
    from object_alignment_amd.operators.icp_align import IcpSettings, boundary_of
    import object_alignment_amd
    hdr = open(os.path.join(ROOT, "include", "oa_icp.h")).read()
    assert re.search(r"\bint\s+oa_target_boundary\s*\(\s*oa_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*,\s*double\s+\w+\s*,\s*uint8_t\s*\*\s*\w+\s*,\s*uint8_t\s*\*\s*\w+\s*\)", hdr)
    assert re.search(r"\bint\s+oa_set_reject_boundary\s*\(\s*oa_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*double\s+\w+\s*\)", hdr)
    stats = {"OA_STAT_REJECT_BOUNDARY": 44, "OA_STAT_BOUNDARY_REJECTED": 45, "OA_STAT_TARGET_BOUNDARY": 46,
             "OA_STAT_BOUNDARY_VERTICES": 47, "OA_STAT_BOUNDARY_EDGES": 48}
    for name, number in stats.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, number), hdr), name
        assert getattr(_capi, name) == number
    u8 = C.POINTER(C.c_uint8)
    L = _capi.load()
    for sym in ("oa_target_boundary", "oa_set_reject_boundary"):
        assert sym in _capi.SYMBOLS and hasattr(L, sym), sym
        # (the experiments' flavour is looked at in a child: this file runs first, and a second copy of the library's device code in
        #  the suite's own process is not this test's to load)
        lib = os.path.join(ROOT, "object_alignment_amd", "liboa_icp_exp.so")
        code = "import ctypes, sys; sys.exit(0 if hasattr(ctypes.CDLL(sys.argv[1]), sys.argv[2]) else 1)"
        assert subprocess.run([sys.executable, "-c", code, lib, sym], timeout=120).returncode == 0, (lib, sym)
    assert L.oa_target_boundary.argtypes == [C.c_void_p, C.c_int, C.c_double, u8, u8]
    assert L.oa_set_reject_boundary.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_double]
    assert C.sizeof(_capi.Settings) == 32 and C.sizeof(_capi.Report) == 72
    assert callable(IcpEngine.set_reject_boundary) and callable(IcpEngine.target_boundary)
    assert [IcpEngine.STATS[n] for n in ("reject_boundary", "boundary_rejected", "target_boundary", "boundary_vertices", "boundary_edges")] == \
        [44, 45, 46, 47, 48]
    s = IcpSettings()
    assert s.reject_boundary is False and s.boundary_k == 16 and s.boundary_angle == 90.0
    assert boundary_of(s) == (False, 16, 90.0)
    assert boundary_of(IcpSettings(reject_boundary=True, boundary_k=8, boundary_angle=120.0)) == (True, 8, 120.0)

    class Prefs:
        icp_reject_boundary = True
    assert boundary_of(Prefs()) == (True, 16, 90.0)
    assert boundary_of(object()) == (False, 16, 90.0)
    assert boundary_of(IcpSettings(reject_boundary=True, boundary_k=0, boundary_angle=0.0)) == (True, 0, 0.0)     # (the library's to refuse)
    addon = open(blender_addon.__file__).read()
    assert re.search(r"icp_reject_boundary\s*:\s*BoolProperty", addon)
    assert len(re.findall(r'"icp_reject_boundary"', addon)) == 2   # the preferences' and the panel's draw
    assert callable(icp_align.apply_boundary)
    assert callable(object_alignment_amd.mesh_boundary) and callable(object_alignment_amd.cloud_boundary)


def test_apply_boundary_hands_the_setting_over_every_time():
    from object_alignment_amd.operators.icp_align import IcpSettings, apply_boundary

    class Eng:
        def __init__(self):
            self.calls = []

        def set_reject_boundary(self, on, k, angle_deg):
            self.calls.append((on, k, angle_deg))
    e = Eng()
    apply_boundary(e, IcpSettings(reject_boundary=True, boundary_k=12, boundary_angle=100.0))
    apply_boundary(e, IcpSettings())
    assert e.calls == [(True, 12, 100.0), (False, 16, 90.0)]
    apply_boundary(object(), IcpSettings())                        # an engine without the setter counts as off
    with pytest.raises(RuntimeError):
        apply_boundary(object(), IcpSettings(reject_boundary=True))


def test_reference_masks_on_known_answers():
    cases = mesh_cases()
    n_edges = lambda em: int(sum(bin(int(b)).count("1") for b in em))   # noqa: E731
    V, T = cases["closed"]
    vm, em = mesh_boundary_ref(len(V), T)
    assert not vm.any() and not em.any()
    vm, em = mesh_boundary_ref(3, cases["one_triangle"][1])
    assert em.tolist() == [7] and vm.tolist() == [1, 1, 1]
    vm, em = mesh_boundary_ref(4, cases["two_triangles"][1])
    assert n_edges(em) == 4 and em.tolist() == [3, 6] and vm.tolist() == [1, 1, 1, 1]        # (0-2 is ca of the first, ab of the second)
    vm, em = mesh_boundary_ref(5, cases["three_on_one_edge"][1])
    assert em.tolist() == [6, 6, 6] and n_edges(em) == 6                                     # ab = 0-2 clear in all three
    V, T = cases["one_removed"]
    vm, em = mesh_boundary_ref(len(V), T)
    assert n_edges(em) == 3 and int(vm.sum()) == 3
    V, T = cases["half_bumpy3"]
    vm, em = mesh_boundary_ref(len(V), T)
    assert len(T) == 562 and n_edges(em) == 46 and int(vm.sum()) == 46
    vm, em = mesh_boundary_ref(5, cases["vertex_twice"][1])
    # [0,1,2]: ab, bc boundary, ca = 0-2 held by three triangles.  [0,2,2]: nothing.  [2,3,3]: 2-3 is also [0,2,3]'s bc.  [0,2,3]: ca = 3-0
    assert em.tolist() == [3, 0, 0, 4, 0] and vm.tolist() == [1, 1, 1, 1, 0]
    xyz, nrm, ring = grid_cloud(9)
    mask, gaps = cloud_boundary_ref(xyz, nrm, knn_rows_ref(xyz, 9), k=8, angle_deg=90.0)
    assert np.array_equal(mask != 0, ring)
    assert np.all(np.isfinite(gaps)) and float(np.min(np.abs(gaps - np.pi / 2))) >= 0.785
    t32, n32 = half_cloud()
    mask, gaps = cloud_boundary_ref(t32, n32, knn_rows_ref(t32, K_DEF + 1))
    assert len(t32) == 2000 and int(mask.sum()) == 148
    assert len(near_threshold(gaps, ANGLE_DEF, 1e-3)) == 0


def test_reference_loops_reproduce_the_table():
    """plain numpy, fp64, the usual pose, thresh 0.5, point metric.  Measured when this test was written: mesh target, 40 steps,
    translation error 0.1912 plain and 0.00596 with the boundary pairs dropped (1372 pairs in step 1, 504 of them on the rim);
    cloud target, 60 steps, 0.1819 plain and 0.00062 with them dropped (2153 pairs, 773 on the rim)."""
    m0, m1, c0, c1 = numpy_loop_mesh(False), numpy_loop_mesh(True), numpy_loop_cloud(False), numpy_loop_cloud(True)
    print("mesh : plain %.4g / %.3g deg, boundary %.4g / %.3g deg, step 1: %d pairs, %d on the rim" % (m0[0], m0[1], m1[0], m1[1], m0[2], m0[3]))
    print("cloud: plain %.4g / %.3g deg, boundary %.4g / %.3g deg, step 1: %d pairs, %d on the rim" % (c0[0], c0[1], c1[0], c1[1], c0[2], c0[3]))
    assert (m0[2], m0[3]) == (1372, 504) and (c0[2], c0[3]) == (2153, 773)
    assert m1[0] * 10.0 < m0[0] and c1[0] * 10.0 < c0[0]
    assert abs(m0[0] - 0.1912) < 2e-3 and abs(m1[0] - 0.00596) < 3e-4
    assert abs(c0[0] - 0.1819) < 2e-3 and abs(c1[0] - 0.00062) < 1e-4


# ------------------------------------------------------------------------------------------------ GPU: the masks
@pytest.mark.gpu
@pytest.mark.parametrize("name", MESH_CASES)
def test_gpu_mesh_masks_bit_for_bit(name):
    import object_alignment_amd
    from object_alignment_amd.engine import IcpEngine
    V, T = mesh_cases()[name]
    vm, em = mesh_boundary_ref(len(V), T)
    with IcpEngine(0) as e:
        e.set_target_mesh(V, T)
        assert e.stat("target_boundary") == 0.0 and e.stat("boundary_vertices") == 0.0 and e.stat("boundary_edges") == 0.0
        for _ in range(2):                                         # (the second call finds them built)
            v, ed = e.target_boundary()
            assert v.dtype == np.uint8 and ed.dtype == np.uint8
            assert np.array_equal(v, vm) and np.array_equal(ed, em)
            assert e.stat("target_boundary") == 1.0
            assert e.stat("boundary_vertices") == float(vm.sum())
            assert e.stat("boundary_edges") == float(sum(bin(int(b)).count("1") for b in em))
        e.mesh_pseudonormals()                                     # (the corner rows are shared with the pseudo-normals)
        v, ed = e.target_boundary()
        assert np.array_equal(v, vm) and np.array_equal(ed, em)
        e.set_target_mesh(V, T)
        assert e.stat("target_boundary") == 0.0                    # a new upload forgets them
    if name == "half_bumpy3":
        v, ed = object_alignment_amd.mesh_boundary(V, T)
        assert np.array_equal(v, vm) and np.array_equal(ed, em)


def cloud_case(name):
    """(xyz, normals or "estimate", k, angle_deg)"""
    if name == "grid":
        xyz, nrm, _ = grid_cloud(9)
        return xyz, nrm, 8, 90.0
    if name == "four_points":
        return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.3, 0.3, 0]], np.float32), np.tile(np.array([[0, 0, 1]], np.float32), (4, 1)), 3, 90.0
    t32, n32 = half_cloud()
    if name == "every_point_twice":
        return np.concatenate([t32[:300], t32[:300]]), np.concatenate([n32[:300], n32[:300]]), K_DEF, ANGLE_DEF
    if name == "non_finite_vertex":
        x = t32[:500].copy()
        x[17, 1] = np.nan
        return x, n32[:500], K_DEF, ANGLE_DEF
    if name == "zero_normal":
        n = n32[:500].copy()
        n[23] = 0.0
        n[24, 0] = np.inf
        return t32[:500], n, K_DEF, ANGLE_DEF
    if name == "half_cloud":
        return t32, n32, K_DEF, ANGLE_DEF
    if name == "half_cloud_estimated":
        return t32, "estimate", K_DEF, ANGLE_DEF
    if name == "half_cloud_k63":
        return t32, n32, 63, 120.0
    raise ValueError(name)


CLOUD_CASES = ["grid", "four_points", "every_point_twice", "non_finite_vertex", "zero_normal", "half_cloud", "half_cloud_estimated",
               "half_cloud_k63"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLOUD_CASES)
def test_gpu_cloud_masks(name):
    """The engine's mask against numpy's over the engine's own k-nearest rows (the contract's neighbours), leaving out vertices
    whose largest gap is within 1e-9 rad of the threshold -- there are none in these inputs, asserted on the reference side."""
    import object_alignment_amd
    from object_alignment_amd.engine import IcpEngine
    xyz, nrm, k, angle = cloud_case(name)
    with IcpEngine(0) as e:
        e.set_target(xyz)
        if isinstance(nrm, str):
            nrm, _ = e.estimate_target_normals(k=k, orient="none", install=True)
        else:
            e.set_target_normals(nrm)
        rows, _ = e.target_knn(k + 1)
        want, gaps = cloud_boundary_ref(xyz, nrm, rows, k, angle)
        assert len(near_threshold(gaps, angle, 1e-9)) == 0
        print("%s: %d of %d flagged, %d within 1e-3 rad of the threshold" % (name, int(want.sum()), len(xyz), len(near_threshold(gaps, angle, 1e-3))))
        for _ in range(2):
            got, edges = e.target_boundary(k, angle)
            assert edges is None and got.dtype == np.uint8
            assert np.array_equal(got, want)
            assert e.stat("target_boundary") == 1.0 and e.stat("boundary_vertices") == float(want.sum()) and e.stat("boundary_edges") == 0.0
        if name == "grid":
            assert np.array_equal(got != 0, grid_cloud(9)[2])
        if name == "non_finite_vertex":
            assert got[17] == 1
        if name == "zero_normal":
            assert got[23] == 1 and got[24] == 1
        if name == "half_cloud":
            assert int(want.sum()) == 148 and len(near_threshold(gaps, angle, 1e-3)) == 0
            assert np.array_equal(object_alignment_amd.cloud_boundary(xyz, nrm, k, angle), want)
            other, _ = cloud_boundary_ref(xyz, nrm, e.target_knn(9)[0], 8, 60.0)
            assert np.array_equal(e.target_boundary(8, 60.0)[0], other) and not np.array_equal(other, want)     # changed (k, angle) rebuild
        if name == "half_cloud_estimated":
            assert np.array_equal(object_alignment_amd.cloud_boundary(xyz, "estimate", k, angle), want)
        # new normals rebuild the mask: with every normal zero, every vertex is flagged
        e.set_target_normals(np.zeros_like(np.asarray(nrm, np.float32)))
        assert e.stat("target_boundary") == 0.0
        assert e.target_boundary(k, angle)[0].all()


# ------------------------------------------------------------------------------------------------ GPU: the pairs
def pairs_case(name):
    """dict(src, sn, vlist, stride, tgt, tris, tn, mxa, mxb, thresh)"""
    mxa, mxb = usual_pose()
    d = dict(vlist=None, stride=1, tris=None, mxa=mxa, mxb=mxb, thresh=THRESH)
    d["tgt"], d["tn"] = half_cloud()
    if name.startswith("cloud_n"):
        d["src"] = whole(int(name[7:]))
    elif name.startswith("mesh_n"):
        d["src"] = whole(int(name[6:]))
        d["tgt"], d["tris"] = half_mesh(3)
        d["tn"] = None
    elif name in ("vlist_stride2", "mesh_vlist_stride2"):
        d["src"] = whole(4097)
        d.update(vlist=np.arange(4096, -1, -1, dtype=np.int64)[:3000], stride=2)
    elif name in ("scaled_base", "mesh_scaled_base"):
        d["src"] = whole(1000)
        B = scaled_base()
        d.update(mxa=(B @ mxa.astype(np.float64)).astype(np.float32), mxb=B.astype(np.float32))
    elif name == "closed_mesh":
        d["src"] = whole(1000)
        d["tgt"], d["tris"] = (np.asarray(a) for a in synth.bumpy_icosphere_mesh(3))
        d["tn"] = None
    else:
        raise ValueError(name)
    if name.startswith("mesh_") and d["tris"] is None:
        d["tgt"], d["tris"] = half_mesh(3)
        d["tn"] = None
    d["src"] = np.asarray(d["src"], np.float32)
    d["sn"] = np.ones_like(d["src"])
    d["sel"] = selection(len(d["src"]), d["vlist"], d["stride"])
    return d


def open_pairs_case(e, d):
    if d["tris"] is None:
        e.set_target(d["tgt"])
        e.set_target_normals(d["tn"])
    else:
        e.set_target_mesh(d["tgt"], d["tris"])
    e.set_source(d["src"], vlist=d["vlist"], stride=d["stride"])
    e.set_matrices(d["mxa"], d["mxb"])


def masks_of(d):
    if d["tris"] is None:
        return cloud_boundary_ref(d["tgt"], d["tn"], knn_rows_ref(d["tgt"], K_DEF + 1))[0], None
    return mesh_boundary_ref(len(d["tgt"]), d["tris"])


PAIRS_CASES = ["cloud_n1", "cloud_n63", "cloud_n64", "cloud_n65", "cloud_n257", "cloud_n4097", "mesh_n1", "mesh_n63", "mesh_n64", "mesh_n65", "mesh_n257", "mesh_n4097",
               "vlist_stride2", "mesh_vlist_stride2", "scaled_base", "mesh_scaled_base", "closed_mesh"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", PAIRS_CASES)
def test_gpu_make_pairs_bit_for_bit(orc, name, tmp_path):
    """With the setting on, make_pairs returns exactly the reference's A and B -- same K, same order, same bits -- and
    OA_STAT_BOUNDARY_REJECTED the reference's count."""
    from object_alignment_amd.engine import IcpEngine
    d = pairs_case(name)
    vmask, emask = masks_of(d)
    src_sel = d["src"][d["sel"]]
    P, rim = bnd_pairs(orc, src_sel, d["sn"][d["sel"]], d["mxa"], d["mxb"], d["tgt"], d["tris"], d["tn"], vmask, emask, tmp_path)
    plain, kept = len(rim), int((~rim).sum())
    print("%s: kept %d of %d pairs (%d selected points)" % (name, kept, plain, len(src_sel)))
    if name == "closed_mesh":
        assert kept == plain > 0
    elif not name.endswith("_n1"):
        assert 0 < kept < plain                                    # both verdicts
    with IcpEngine(0) as e:
        open_pairs_case(e, d)
        A0, B0, _ = e.make_pairs(THRESH)
        assert A0.shape == (3, plain) and e.stat("boundary_rejected") == 0.0 and e.stat("reject_boundary") == 0.0
        assert np.array_equal(A0.T, P["a"]) and np.array_equal(B0.T, P["b"])
        e.set_reject_boundary(True)
        assert e.stat("reject_boundary") == 1.0
        for _ in range(2):                                         # (the second call finds the masks built)
            A, B, _ = e.make_pairs(THRESH)
            assert A.shape == (3, kept)
            assert np.array_equal(A.T, P["a"][~rim]) and np.array_equal(B.T, P["b"][~rim])
            assert e.stat("boundary_rejected") == float(plain - kept) and e.stat("target_boundary") == 1.0
        _, _, ds = e.make_pairs(THRESH, calc_stats=True)            # (two passes: the verdict runs in both)
        assert e.stat("boundary_rejected") == float(plain - kept)
        if kept > 0:
            D = P["dist"][~rim]
            assert abs(ds[0] - D.mean()) <= TOL and abs(ds[1] - D.std()) <= TOL
        e.set_reject_boundary(False)
        A1, B1, _ = e.make_pairs(THRESH)
        assert np.array_equal(A1, A0) and np.array_equal(B1, B0) and e.stat("boundary_rejected") == 0.0


@pytest.mark.gpu
def test_gpu_source_beyond_the_rim(orc, tmp_path):
    """A source entirely beyond the rim: every pair is rejected, a step has fewer than 3 pairs (the reference's ValueError), and the
    context stays usable."""
    from object_alignment_amd.engine import IcpEngine, REF_VALUEERROR
    V, T = half_mesh(3)
    full_v, _ = synth.bumpy_icosphere_mesh(3)
    full_v = np.asarray(full_v, np.float32)
    src = np.ascontiguousarray(full_v[full_v[:, 2] < -0.3])
    eye = np.eye(4, dtype=np.float32)
    vmask, emask = mesh_boundary_ref(len(V), T)
    P, rim = bnd_pairs(orc, src, np.ones_like(src), eye, eye, V, T, None, vmask, emask, tmp_path, thresh=3.0)
    assert len(rim) == len(src) > 100 and rim.all()
    with IcpEngine(0) as e:
        e.set_target_mesh(V, T)
        e.set_source(src)
        e.set_matrices(eye, eye)
        e.set_reject_boundary(True)
        A, _, _ = e.make_pairs(3.0)
        assert A.shape == (3, 0) and e.stat("boundary_rejected") == float(len(src))
        with pytest.raises(ValueError, match=REF_VALUEERROR):
            e.iterate(thresh=3.0)
        with pytest.raises(ValueError, match=REF_VALUEERROR):
            e.run(iters=3, thresh=3.0)
        e.set_reject_boundary(False)
        e.set_matrices(eye, eye)
        r = e.run(iters=3, thresh=3.0, early_exit=False)
        assert r.iters_done == 3 and r.last_K == len(src)


# ------------------------------------------------------------------------------------------------ GPU: the steps
def step_case(case):
    mxa, mxb = usual_pose()
    src, sn = synth.bunny_surface_with_normals(3000, 0.5)
    d = dict(src=np.asarray(src, np.float32), sn=np.asarray(sn, np.float32), tris=None, mxa=mxa, mxb=mxb, metric="point", loss="none", c=0.0)
    d["tgt"], d["tn"] = half_cloud()
    if case == "plane_mesh":
        d["tgt"], d["tris"] = half_mesh(3)
        d.update(tn=None, metric="plane")
    elif case == "gicp_cloud":
        d["metric"] = "gicp"
    elif case == "tukey":
        d.update(loss="tukey", c=0.05)
    elif case != "point":
        raise ValueError(case)
    return d


def open_step_case(e, d):
    e.set_metric(d["metric"])
    e.set_robust(d["loss"], d["c"])
    if d["tris"] is None:
        e.set_target(d["tgt"])
        e.set_target_normals(d["tn"])
    else:
        e.set_target_mesh(d["tgt"], d["tris"])
    e.set_source(d["src"], stride=1)
    e.set_source_normals(d["sn"])
    e.set_matrices(d["mxa"], d["mxb"])


def ref_step_of(orc, d, mw, vmask, emask, tmp_path, piv, s_world, recip=False, trim=0.0):
    """dict(M, spread, K, rejected, mean, std, candidates): the reference step at matrix_world mw"""
    P, rim = bnd_pairs(orc, d["src"], d["sn"], mw, d["mxb"], d["tgt"], d["tris"], d["tn"], vmask, emask, tmp_path)
    keep = np.ones(len(rim), bool)
    if recip:
        keep &= recip_keep(orc, P["a"], P["b"], d["src"])
    rejected = int((keep & rim).sum())
    keep &= ~rim
    res = residuals(d["metric"], P, piv, s_world)
    candidates = int(keep.sum())
    if trim:
        q, _, _ = fixed_cut(res[keep], trim)
        keep &= res.astype(np.float32) <= np.float32(q)
    w = None
    if d["loss"] != "none":
        w = psi(d["loss"], res[keep], d["c"])
    M, M_rev, _ = solve(d["metric"], P, keep, piv, w=w)
    D = P["dist"][keep]
    return dict(M=M, spread=float(np.max(np.abs(M - M_rev))), K=int(keep.sum()), rejected=rejected, mean=float(D.mean()), std=float(D.std()),
                candidates=candidates)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["point", "plane_mesh", "gicp_cloud", "tukey"])
def test_gpu_step_parity(orc, case, tmp_path):
    """Six steps; before every step the engine's matrix_world goes to the reference.  K and the rejected count exact, M within TOL,
    all four cases; the reference's own two summation orders agree to TOL too."""
    from object_alignment_amd.engine import IcpEngine
    d = step_case(case)
    vmask, emask = masks_of(d)
    piv = d["src"][0].astype(np.float64)
    total = 0
    with IcpEngine(0) as e:
        e.set_reject_boundary(True)
        open_step_case(e, d)
        assert e.stat("reject_boundary") == 1.0                     # survives the uploads and set_matrices
        s_world = world_scale(e.matrix_world())
        for it in range(6):
            ref = ref_step_of(orc, d, e.matrix_world(), vmask, emask, tmp_path, piv, s_world)
            M, st = e.iterate(thresh=THRESH, target_d=1e-4)
            dM = float(np.max(np.abs(M - ref["M"])))
            rejected = int(e.stat("boundary_rejected"))
            print("step %d: K %d / %d, rejected %d / %d, |dM| %.3g (reference spread %.3g)" % (it, st["K"], ref["K"], rejected, ref["rejected"], dM, ref["spread"]))
            assert ref["spread"] < TOL, "the case is ill-conditioned for the reference itself"
            assert st["K"] == ref["K"] and rejected == ref["rejected"]
            assert dM <= TOL
            assert abs(st["mean_dist"] - ref["mean"]) <= TOL and abs(st["std_dist"] - ref["std"]) <= TOL
            total += rejected
    assert total > 0                                               # the rule had something to say


@pytest.mark.gpu
@pytest.mark.parametrize("with_", ["reciprocal", "trim", "reciprocal+trim"])
def test_gpu_composition(orc, with_, tmp_path):
    """With the reciprocal check on the rejected count is over the mutual pairs; with trim = 0.5 the candidates exclude the boundary
    pairs.  Three steps against the reference.  reciprocal+trim: all three filters in one step -- the one combination in which
    every stage finds the verdict bytes written by the stage before it."""
    from object_alignment_amd.engine import IcpEngine
    d = step_case("point")
    vmask, emask = masks_of(d)
    piv = d["src"][0].astype(np.float64)
    recip, trim = "reciprocal" in with_, "trim" in with_
    with IcpEngine(0) as e:
        e.set_reject_boundary(True)
        if recip:
            e.set_reciprocal(True)
        if trim:
            e.set_trim(0.5)
        open_step_case(e, d)
        s_world = world_scale(e.matrix_world())
        for it in range(3):
            ref = ref_step_of(orc, d, e.matrix_world(), vmask, emask, tmp_path, piv, s_world, recip=recip, trim=0.5 if trim else 0.0)
            M, st = e.iterate(thresh=THRESH, target_d=1e-4)
            dM = float(np.max(np.abs(M - ref["M"])))
            print("step %d: K %d / %d, rejected %d / %d, |dM| %.3g" % (it, st["K"], ref["K"], int(e.stat("boundary_rejected")), ref["rejected"], dM))
            assert st["K"] == ref["K"] and e.stat("boundary_rejected") == float(ref["rejected"]) and ref["rejected"] > 0
            if trim:
                assert e.stat("trim_candidates") == float(ref["candidates"]) and e.stat("trim_kept") == float(ref["K"])
            if recip:
                assert e.stat("recip_rejected") > 0.0
            assert ref["spread"] < TOL and dM <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("target", ["cloud", "mesh"])
def test_gpu_search_modes_agree_bitwise(target):
    from object_alignment_amd.engine import IcpEngine
    d = pairs_case("cloud_n3000" if target == "cloud" else "mesh_n3000")
    hist = {}
    for mode in ("brute", "grid", "bvh", "auto"):
        with IcpEngine(0) as e:
            e.set_reject_boundary(True)
            e.set_search_mode(mode)
            open_pairs_case(e, d)
            r = e.run(iters=10, thresh=THRESH, target_d=1e-4, early_exit=False)
            assert r.iters_done == 10 and e.stat("boundary_rejected") > 0.0
        hist[mode] = (r.step_M.copy(), r.step_new.copy(), r.step_K.copy(), r.step_stats.copy(), r.matrix_world.copy())
    for mode, run in hist.items():
        for x, y in zip(hist["brute"], run):
            assert np.array_equal(x, y), mode


@pytest.mark.gpu
@pytest.mark.parametrize("target", ["cloud", "mesh"])
def test_gpu_off_means_off(target):
    """A context that ran with the setting and then switches it off repeats a fresh context's 15-iteration history bit for bit;
    nn_search and deviation do not look at the setting."""
    from object_alignment_amd.engine import IcpEngine
    d = pairs_case("cloud_n3000" if target == "cloud" else "mesh_n3000")

    def history(e, iters=15):
        e.set_search_mode("grid")
        open_pairs_case(e, d)
        return e.run(iters=iters, thresh=THRESH, target_d=0.01, early_exit=False), e.stat("fast_iterations")
    with IcpEngine(0) as e:
        plain, fast0 = history(e)
    with IcpEngine(0) as e:
        e.set_reject_boundary(True)
        _, fast_on = history(e, iters=3)
        assert fast_on == 0 and e.stat("boundary_rejected") > 0.0   # search -> verdict -> accumulate: never the fused path
        e.set_matrices(d["mxa"], d["mxb"])
        idx_on, d2_on, _ = e.nn_search()
        dev_on = e.deviation(thresh=THRESH, outputs=("dist", "idx"))
        e.set_reject_boundary(False)
        e.set_matrices(d["mxa"], d["mxb"])
        idx_off, d2_off, _ = e.nn_search()
        dev_off = e.deviation(thresh=THRESH, outputs=("dist", "idx"))
        back, fast1 = history(e)
    assert fast1 == fast0
    for name in ("step_M", "step_new", "step_K", "step_stats", "step_trans", "matrix_world"):
        assert np.array_equal(getattr(plain, name), getattr(back, name)), name
    assert np.array_equal(idx_on, idx_off) and np.array_equal(d2_on, d2_off)
    assert np.array_equal(dev_on["dist"], dev_off["dist"], equal_nan=True) and np.array_equal(dev_on["idx"], dev_off["idx"])


@pytest.mark.gpu
@pytest.mark.parametrize("target", ["mesh", "cloud"])
def test_gpu_behaviour_on_the_table_cases(target):
    """IcpAlign.run with IcpSettings(reject_boundary=True) on both cases of the table: the loop ends within 1.5 x the numpy loop's
    translation error + 1e-4 (test_reciprocal.py's margin for its own engine-against-numpy comparison) and at least 10 x closer
    than the engine's own plain loop (the numpy loops' ratios: 32 x and 290 x)."""
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings
    mxa, mxb = usual_pose()
    if target == "mesh":
        src, iters, te_ref = np.asarray(synth.bunny_surface(2000, 0.5), np.float32), 40, numpy_loop_mesh(True)[0]
        tgt, tris = half_mesh(3)
        kw = dict(target_tris=tris)
    else:
        src, iters, te_ref = whole(3000), 60, numpy_loop_cloud(True)[0]
        tgt, tn = half_cloud()
        kw = dict(target_normals=tn)
    te = {}
    with IcpEngine(0) as e:
        for on in (True, False):
            st = IcpSettings(icp_iterations=iters, sample_fraction=1, min_start=THRESH, reject_boundary=on)
            r = IcpAlign(st, engine=e).run(src, tgt, mxa, mxb, early_exit=False, **kw)
            assert r.iters_done == iters and e.stat("reject_boundary") == (1.0 if on else 0.0)
            assert (e.stat("boundary_rejected") > 0.0) == on
            te[on] = translation_error(r.matrix_world)
            if on:                                                 # RunResult of a run with the setting on
                assert r.last_K == int(r.step_K[-1]) and r.step_M.shape == (iters, 4, 4) and np.isfinite(r.mean_dist)
    print("%s: translation error: engine boundary %.4g (numpy %.4g), engine plain %.4g" % (target, te[True], te_ref, te[False]))
    assert te[True] <= 1.5 * te_ref + 1e-4
    assert te[True] * 10.0 <= te[False]


@pytest.mark.gpu
def test_gpu_off_works_on_a_cloud_smaller_than_k():
    """The setting is handed over on every run, off included: a cloud target of at most 16 points (fewer than the default k + 1)
    takes set_reject_boundary(False) and IcpAlign.run with default settings; switched on, the loop names k and the context
    stays usable."""
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings
    mxa, mxb = usual_pose()
    tgt = np.asarray(synth.icosphere(0), np.float32)
    assert len(tgt) == 12
    src = (tgt.astype(np.float64) * 1.01).astype(np.float32)
    nrm = tgt / np.linalg.norm(tgt, axis=1, keepdims=True).astype(np.float32)
    with IcpEngine(0) as e:
        e.set_target(tgt)
        e.set_reject_boundary(False)
        e.set_reject_boundary(False, 16, 90.0)
        r = IcpAlign(IcpSettings(icp_iterations=5, sample_fraction=1, min_start=2.0), engine=e).run(src, tgt, mxa, mxb, early_exit=False)
        assert r.iters_done == 5 and r.last_K == 12 and e.stat("reject_boundary") == 0.0
        e.set_target_normals(nrm)
        e.set_reject_boundary(True)                                # k = 16 > nt - 1: taken here, refused where the masks are built
        e.set_matrices(mxa, mxb)
        with pytest.raises(_capi.OaError, match="k = 16") as ei:
            e.run(iters=5, thresh=2.0)
        assert ei.value.code == _capi.OA_E_BAD_ARG
        e.set_reject_boundary(True, 8, 90.0)
        e.set_matrices(mxa, mxb)
        r8 = e.run(iters=5, thresh=2.0, early_exit=False)
        assert r8.iters_done == 5 and r8.last_K == 12 and e.stat("boundary_vertices") == 0.0    # a closed shell: nothing on a rim
        e.set_reject_boundary(False, 16, 90.0)
        e.set_matrices(mxa, mxb)
        r0 = e.run(iters=5, thresh=2.0, early_exit=False)
        assert np.array_equal(r0.step_K, r.step_K)


@pytest.mark.gpu
def test_gpu_refusals_leave_the_context_usable():
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    mxa, mxb = usual_pose()
    src = whole(3000)
    tgt, tn = half_cloud()

    def plain_loop_ok(e, reload=False):
        e.set_reject_boundary(False)
        if reload:
            e.set_source(src, stride=1)
        e.set_matrices(mxa, mxb)
        r = e.run(iters=5, thresh=THRESH, target_d=0.01, early_exit=False)
        assert r.iters_done == 5 and np.array_equal(r.step_K, want.step_K)

    with IcpEngine(0) as e:
        with pytest.raises(_capi.OaError) as ei:                   # no target
            e.target_boundary()
        assert ei.value.code == _capi.OA_E_STATE
        e.set_target(tgt)
        e.set_source(src, stride=1)
        e.set_matrices(mxa, mxb)
        want = e.run(iters=5, thresh=THRESH, target_d=0.01, early_exit=False)
        for k, angle in ((2, 90.0), (64, 90.0), (0, 90.0), (16, 0.0), (16, 360.0), (16, float("nan")), (16, -5.0)):
            with pytest.raises(_capi.OaError) as ei:
                e.set_reject_boundary(True, k, angle)
            assert ei.value.code == _capi.OA_E_BAD_ARG
        assert e.stat("reject_boundary") == 0.0
        # a cloud without normals: the setter takes it, the loop and the masks name what is missing
        e.set_reject_boundary(True)
        e.set_matrices(mxa, mxb)
        for call in (lambda: e.run(iters=5, thresh=THRESH), lambda: e.make_pairs(THRESH), lambda: e.target_boundary()):
            with pytest.raises(_capi.OaError, match="oa_set_target_normals") as ei:
                call()
            assert ei.value.code == _capi.OA_E_STATE
        plain_loop_ok(e)
        e.set_target_normals(tn)
        for k, angle in ((2, 90.0), (64, 90.0), (16, 360.0)):
            with pytest.raises(_capi.OaError) as ei:
                e.target_boundary(k, angle)
            assert ei.value.code == _capi.OA_E_BAD_ARG
        edges = np.zeros(len(tgt), np.uint8)
        u8 = C.POINTER(C.c_uint8)
        assert e._L.oa_target_boundary(e._h, 16, 90.0, None, edges.ctypes.data_as(u8)) == _capi.OA_E_BAD_ARG      # edge_mask for a cloud
        assert e._L.oa_target_boundary(e._h, 16, 90.0, None, None) == 0 and e.stat("target_boundary") == 1.0       # both pointers may be NULL
        e.set_reject_boundary(True)
        e.set_matrices(mxa, mxb)
        with pytest.raises(_capi.OaError, match="oa_set_reject_boundary") as ei:
            e.run_begin(iters=5)
        assert ei.value.code == _capi.OA_E_STATE
        plain_loop_ok(e)
        e.set_reject_boundary(True)
        e.set_source(src, stride=1, shard_index=0, shard_count=2)
        e.set_matrices(mxa, mxb)
        for call in (lambda: e.run(iters=5), lambda: e.iterate(), lambda: e.make_pairs(THRESH)):
            with pytest.raises(_capi.OaError, match="oa_set_reject_boundary") as ei:
                call()
            assert ei.value.code == _capi.OA_E_STATE
        plain_loop_ok(e, reload=True)
    with IcpEngine(devices=[0, 0]) as m:
        m.set_target(tgt)
        m.set_target_normals(tn)
        m.set_source(src, stride=1)
        m.set_matrices(mxa, mxb)
        m.set_reject_boundary(True)
        assert m.stat("reject_boundary") == 1.0
        for call in (lambda: m.run(iters=5), lambda: m.iterate(), lambda: m.make_pairs(THRESH)):
            with pytest.raises(_capi.OaError, match="oa_set_reject_boundary") as ei:
                call()
            assert ei.value.code == _capi.OA_E_STATE
        with pytest.raises(_capi.OaError, match="single-device") as ei:
            m._chk(m._L.oa_target_boundary(m._h, 16, 90.0, None, None))
        assert ei.value.code == _capi.OA_E_STATE
        m.set_reject_boundary(False)
        r = m.run(iters=5, thresh=THRESH, target_d=0.01, early_exit=False)
        assert r.iters_done == 5
