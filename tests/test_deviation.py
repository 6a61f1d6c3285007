"""The deviation report (oa_deviation): signed per-point distances and fit statistics.

CPU: symbols and struct layout, argument checks, the fixture guard (the numpy restatement of the sign rule against the generalized
winding number), closest_on_tri_region against closest_on_tri on the host.  GPU: the pseudo-normals, the per-slot outputs, the
sign, search-mode independence, the statistics, the edge cases and the public surface."""
import ctypes as C
import dataclasses
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from object_alignment_amd import _capi, synth                                    # noqa: E402
from object_alignment_amd.operators.icp_align import DeviationSettings, IcpAlign, IcpSettings   # noqa: E402

gpu = pytest.mark.gpu
EYE = np.eye(4, dtype=np.float32)
SIZES = (1, 63, 64, 65, 257)                  # + the whole query set (~900): partial wave, one wave, more than one workgroup


# ------------------------------------------------------------------------------------------------------------------------
# meshes: closed, consistently wound (counter-clockwise seen from outside), welded
# ------------------------------------------------------------------------------------------------------------------------
def needle_mesh():
    """A tetrahedron with a base about 0.2 wide and the apex 2.0 away."""
    v = np.array([[0.1, 0.0, 0.0], [-0.05, 0.0866, 0.0], [-0.05, -0.0866, 0.0], [0.0, 0.0, 2.0]], np.float32)
    t = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    return v, t


def l_prism_mesh():
    """An L-shaped prism: 12 vertices, 20 triangles, one concave edge."""
    poly = np.array([[0, 0], [2, 0], [2, 1], [1, 1], [1, 2], [0, 2]], np.float64)
    h = 0.7
    v = np.concatenate([np.c_[poly, np.zeros(6)], np.c_[poly, np.full(6, h)]]).astype(np.float32)
    fan = [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5)]
    t = [(a, c, b) for a, b, c in fan] + [(a + 6, b + 6, c + 6) for a, b, c in fan]
    for i in range(6):
        j = (i + 1) % 6
        t += [(i, j, j + 6), (i, j + 6, i + 6)]
    return v, np.array(t, np.int32)


def bipyramid_mesh(n=600):
    """Two apexes of valence n over a ring of n vertices.  The apex comes first in every triangle."""
    ph = 2.0 * math.pi * np.arange(n) / n
    v = np.concatenate([np.c_[np.cos(ph), np.sin(ph), np.zeros(n)], [[0, 0, 0.8], [0, 0, -0.8]]]).astype(np.float32)
    i = np.arange(n)
    j = (i + 1) % n
    top = np.stack([np.full(n, n), i, j], 1)
    bottom = np.stack([np.full(n, n + 1), j, i], 1)
    return v, np.concatenate([top, bottom]).astype(np.int32)


MESHES = {
    "bumpy1": lambda: synth.bumpy_icosphere_mesh(1),
    "bumpy2": lambda: synth.bumpy_icosphere_mesh(2),
    "needle": needle_mesh,
    "lprism": l_prism_mesh,
    "bipyramid": bipyramid_mesh,
}
CLOSED = tuple(MESHES)


# ------------------------------------------------------------------------------------------------------------------------
# the numpy restatement (fp64): closest point with regions, pseudo-normals, the sign rule; the winding number
# ------------------------------------------------------------------------------------------------------------------------
def closest_with_regions(P, V, T, chunk=128):
    """Brute force in fp64: (idx, r, feature, d2) per query; closest_on_tri's tests in its order, lowest index on ties."""
    V = np.asarray(V, np.float64)
    A, B, Cc = V[T[:, 0]][None], V[T[:, 1]][None], V[T[:, 2]][None]
    ab, ac, cb = B - A, Cc - A, Cc - B
    out_i, out_r, out_f, out_d = [], [], [], []
    dot = lambda x, y: np.sum(x * y, axis=2)   # noqa: E731
    for s in range(0, len(P), chunk):
        p = np.asarray(P[s:s + chunk], np.float64)[:, None, :]
        ap, bp, cp = p - A, p - B, p - Cc
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
        codes = [4, 5, 1, 6, 3, 2]
        feat = np.select(conds, codes, default=0)
        with np.errstate(all="ignore"):
            den = (va + vb) + vc
            pts = [A + 0 * p, B + 0 * p, A + (d1 / (d1 - d3))[..., None] * ab, Cc + 0 * p, A + (d2 / (d2 - d6))[..., None] * ac,
                   B + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None] * cb]
            inside = A + (vb / den)[..., None] * ab + (vc / den)[..., None] * ac
            r = np.select([c[..., None] for c in conds], pts, default=inside)
            dd = np.sum((r - p) ** 2, axis=2)
        dd = np.where(np.isnan(dd), np.inf, dd)
        i = np.argmin(dd, axis=1)
        q = np.arange(len(i))
        out_i.append(i); out_r.append(r[q, i]); out_f.append(feat[q, i]); out_d.append(dd[q, i])
    return np.concatenate(out_i), np.concatenate(out_r), np.concatenate(out_f), np.concatenate(out_d)


def pseudonormals(V, T):
    """(face_n (nt, 3), vertex_n (nv, 3), edge_n (nt, 3, 3)) as DESIGN.md 3.16 defines them, fp64 on the float32 vertices."""
    V = np.asarray(V, np.float32).astype(np.float64)
    T = np.asarray(T, np.int64)
    a, b, c = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]
    n = np.cross(b - a, c - a)
    with np.errstate(all="ignore"):
        l2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        ok = (l2 > 0) & np.isfinite(l2)
        fn = np.where(ok[:, None], n * (1.0 / np.sqrt(np.where(ok, l2, 1.0)))[:, None], 0.0)
        ang = np.zeros((len(T), 3))
        for k in range(3):
            u, v = V[T[:, (k + 1) % 3]] - V[T[:, k]], V[T[:, (k + 2) % 3]] - V[T[:, k]]
            ang[:, k] = np.where(ok, np.arctan2(np.linalg.norm(np.cross(u, v), axis=1), np.sum(u * v, axis=1)), 0.0)
    vn = np.zeros((len(V), 3))
    np.add.at(vn, T.ravel(), (ang[:, :, None] * fn[:, None, :]).reshape(-1, 3))        # ascending (triangle, corner)
    e0, e1 = T, np.roll(T, -1, axis=1)                                                  # edges ab, bc, ca
    key = (np.minimum(e0, e1) * len(V) + np.maximum(e0, e1)).ravel()
    uniq, inv = np.unique(key, return_inverse=True)
    es = np.zeros((len(uniq), 3))
    np.add.at(es, inv, np.repeat(fn, 3, axis=0))                                        # ascending triangle
    return fn, vn, es[inv].reshape(len(T), 3, 3)


def feature_normal(idx, feat, T, fn, vn, en):
    N = fn[idx].copy()
    e = (feat >= 1) & (feat <= 3)
    N[e] = en[idx[e], feat[e] - 1]
    v = feat >= 4
    N[v] = vn[T[idx[v], feat[v] - 4]]
    return N


def winding_number(P, V, T, chunk=128):
    """The generalized winding number (van Oosterom & Strackee's solid angles / 4 pi)."""
    V = np.asarray(V, np.float64)
    A, B, Cc = V[T[:, 0]][None], V[T[:, 1]][None], V[T[:, 2]][None]
    out = []
    for s in range(0, len(P), chunk):
        p = np.asarray(P[s:s + chunk], np.float64)[:, None, :]
        a, b, c = A - p, B - p, Cc - p
        la, lb, lc = np.linalg.norm(a, axis=2), np.linalg.norm(b, axis=2), np.linalg.norm(c, axis=2)
        num = np.sum(a * np.cross(b, c), axis=2)
        den = la * lb * lc + np.sum(a * b, axis=2) * lc + np.sum(b * c, axis=2) * la + np.sum(c * a, axis=2) * lb
        out.append(np.sum(2.0 * np.arctan2(num, den), axis=1) / (4.0 * math.pi))
    return np.concatenate(out)


def queries_for(name, V, T, per_group=300):
    rng = np.random.default_rng(sum(map(ord, name)) + 20261019)
    V64 = V.astype(np.float64)
    lo, hi = V64.min(0) - 0.3, V64.max(0) + 0.3
    box = rng.uniform(lo, hi, size=(per_group, 3))
    vi = rng.integers(0, len(V), per_group)
    if name == "bipyramid":
        vi[: per_group // 2] = len(V) - 2                                # half of the near-vertex group sits at the (top) apex
    near_v = V64[vi] + rng.normal(0.0, 0.05, (per_group, 3))
    ti, ek = rng.integers(0, len(T), per_group), rng.integers(0, 3, per_group)
    near_e = 0.5 * (V64[T[ti, ek]] + V64[T[ti, (ek + 1) % 3]]) + rng.normal(0.0, 0.05, (per_group, 3))
    return np.concatenate([box, near_v, near_e]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """Everything the tests need of one mesh, computed once: queries, the restatement's answers, the ground truth."""
    V, T = MESHES[name]()
    Q = queries_for(name, V, T)
    idx, r, feat, d2 = closest_with_regions(Q, V, T)
    fn, vn, en = pseudonormals(V, T)
    # what the library stores: vertex and edge normals as float32
    N = feature_normal(idx, feat, T, fn, vn.astype(np.float32).astype(np.float64), en.astype(np.float32).astype(np.float64))
    d = Q.astype(np.float64) - r
    with np.errstate(all="ignore"):
        s = (d[:, 0] * N[:, 0] + d[:, 1] * N[:, 1]) + d[:, 2] * N[:, 2]
        cos = s / (np.linalg.norm(d, axis=1) * np.linalg.norm(N, axis=1))
        s_face = np.sum(d * fn[idx], axis=1)
    keep = np.isfinite(cos) & (np.abs(cos) >= 1e-3)
    w = winding_number(Q, V, T)
    for a in (V, T, Q):
        a.setflags(write=False)
    return dict(V=V, T=T, Q=Q, idx=idx, r=r, feat=feat, fn=fn, vn=vn, en=en, keep=keep, w=w, inside=np.abs(w) > 0.5,
                neg=s < 0, neg_face=s_face < 0)


def region_exe():
    import __graft_entry__ as entry
    exe = [e for e in entry.build_tools() if e.endswith("region_check.exe")]
    assert exe, "tools/region_check.hip did not build"
    return exe[0]


def host_regions(P, A, B, Cc, tmp_path):
    """closest_on_tri_region on the host (tools/region_check.exe --pairs) for rows of float32 (p, a, b, c)."""
    rows = np.ascontiguousarray(np.concatenate([P, A, B, Cc], axis=1), dtype=np.float32)
    path = os.path.join(str(tmp_path), "pairs.bin")
    rows.tofile(path)
    out = subprocess.run([region_exe(), "--pairs", path], stdout=subprocess.PIPE, text=True, check=True, timeout=120).stdout
    return np.array(out.split(), dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_layout():
    header = open(os.path.join(ROOT, "include", "oa_icp.h")).read()
    L = C.CDLL(os.path.join(ROOT, "object_alignment_amd", "liboa_icp.so"))
    for name in ("oa_deviation", "oa_get_mesh_pseudonormals"):
        assert "int %s(" % name in header and name in _capi.SYMBOLS and hasattr(L, name), name
    assert "#define OA_STAT_MESH_PSEUDONORMALS 36" in header and _capi.OA_STAT_MESH_PSEUDONORMALS == 36
    S, R = _capi.DeviationSettings, _capi.DeviationReport
    assert C.sizeof(S) == 104
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 8, 12, 16, 80, 84, 88, 96]
    assert C.sizeof(R) == 200
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 160, 164, 168, 172, 176, 184, 192]
    for f in ("thresh", "signed_mode", "n_quantiles", "quantiles[8]", "n_bins", "hist_lo, hist_hi", "n_valid", "n_inlier", "n_inside", "n_unsigned",
              "max_index", "fitness", "mean_signed", "max_dist", "quantile_values[8]", "signed_used", "search_ms, total_ms"):
        assert f in header, f


def test_settings_defaults_unchanged():
    from object_alignment_amd.engine import RunResult
    s = IcpSettings()
    assert (s.icp_iterations, s.min_start, s.target_d, s.use_target, s.align_meth, s.metric, s.robust_loss, s.sample_voxel) == \
        (50, 0.5, 0.01, True, "0", "point", "none", 0.0)
    fields = {f.name: f for f in dataclasses.fields(RunResult)}
    assert fields["deviation"].default is None
    assert [n for n, f in fields.items() if f.default is dataclasses.MISSING and f.default_factory is dataclasses.MISSING] == \
        ["iters_done", "converged", "matrix_world", "last_K", "last_translation", "mean_dist", "std_dist", "mean_rot_angle", "nn_ms_total",
         "loop_ms", "step_M", "step_new", "step_K", "step_stats", "step_trans"]
    d = DeviationSettings()
    assert (d.thresh, d.signed, d.quantiles, d.bins, d.hist_range, d.outputs) == \
        (None, "auto", (0.5, 0.9, 0.95, 0.99), 0, None, ("signed_d", "closest", "idx", "feature"))
    import inspect
    assert inspect.signature(IcpAlign.run).parameters["deviation"].default is None


@pytest.mark.parametrize("kw", [
    dict(thresh=0.0), dict(thresh=-1.0), dict(thresh=float("nan")), dict(thresh=-float("inf")),
    dict(quantiles=(0.0,)), dict(quantiles=(1.5,)), dict(quantiles=(float("nan"),)), dict(quantiles=tuple([0.5] * 9)),
    dict(bins=-1), dict(bins=1025), dict(bins=2.5, hist_range=(0.0, 1.0)),
    dict(bins=4, hist_range=(1.0, 1.0)), dict(bins=4, hist_range=(2.0, 1.0)), dict(bins=4, hist_range=(0.0, float("inf"))),
    dict(bins=4, hist_range=(float("nan"), 1.0)),
    dict(signed="maybe"), dict(signed=2), dict(outputs=("signed_d", "colour")),
])
def test_deviation_settings_reject(kw, monkeypatch):
    import object_alignment_amd
    from object_alignment_amd import engine

    def no_engine(*a, **k):
        raise AssertionError("an engine was opened before the arguments were checked")
    monkeypatch.setattr(engine.IcpEngine, "__init__", no_engine)
    with pytest.raises(ValueError):
        DeviationSettings(**kw)
    with pytest.raises(ValueError):
        object_alignment_amd.deviation(np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), **kw)


def test_deviation_settings_accept():
    DeviationSettings(thresh=float("inf"), quantiles=(1.0,), bins=1024, hist_range=(-1.0, 1.0), signed=True, outputs=())
    DeviationSettings(thresh=0.25, quantiles=(), bins=0, signed=False, outputs=("dist",))


@pytest.mark.parametrize("name", CLOSED)
def test_fixture_guard(name):
    """The numpy restatement alone: its sign is the winding number's on every query it keeps; the fixtures hit every feature and
    can tell the pseudo-normal rule from the face-normal one."""
    f = fixture(name)
    n, keep = len(f["Q"]), f["keep"]
    margin = float(np.min(np.abs(np.abs(f["w"]) - 0.5)))
    print("%s: %d queries, %d left out, smallest | |w| - 0.5 | = %.11f, face-normal rule wrong on %d" %
          (name, n, int(np.sum(~keep)), margin, int(np.sum(f["neg_face"][keep] != f["inside"][keep]))))
    assert np.all(np.isclose(f["w"], np.round(f["w"]), atol=1e-6)), "the mesh is not closed and consistently wound"
    assert np.sum(~keep) <= 0.01 * n
    assert np.array_equal(f["neg"][keep], f["inside"][keep])
    assert np.any(f["inside"]) and np.any(~f["inside"])
    want = {0, 1, 2, 3, 4, 6} if name == "bipyramid" else set(range(7))
    assert want <= set(np.unique(f["feat"]).tolist())
    if name in ("needle", "bipyramid"):
        assert np.any(f["neg_face"][keep] != f["inside"][keep])


def test_closed_meshes_wind_outward():
    """Positive winding number inside: the convention the sign rule states (counter-clockwise seen from outside)."""
    inner = {"bumpy1": [0, 0, 0], "bumpy2": [0, 0, 0], "needle": [0, 0, 0.3], "lprism": [0.5, 0.5, 0.3], "bipyramid": [0, 0, 0.1]}
    for name in CLOSED:
        V, T = MESHES[name]()
        assert abs(winding_number(np.array([inner[name]], np.float64), V, T)[0] - 1.0) < 1e-9, name
    assert len(l_prism_mesh()[1]) == 20 and len(bipyramid_mesh()[1]) == 1200


def test_region_variant_on_host():
    """closest_on_tri_region returns closest_on_tri's bits, on ~1e6 random pairs and the constructed ones; every region occurs."""
    out = subprocess.run([region_exe(), "1000000", "20261019"], stdout=subprocess.PIPE, text=True, timeout=300)
    print(out.stdout)
    words = out.stdout.split()
    assert out.returncode == 0 and words[0] == "pairs" and words[2] == "mismatches" and words[4] == "regions"
    assert int(words[1]) >= 5000000 and int(words[3]) == 0
    assert len(words[5:]) == 7 and all(int(w) > 0 for w in words[5:])


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
MX_ALIGN = synth.rigid4(synth.rotation_from_rotvec([0.3, -0.2, 0.5]), [0.4, -0.1, 0.25])
MX_BASE = synth.rigid4(1.7 * synth.rotation_from_rotvec([-0.4, 0.1, 0.2]), [-0.3, 0.2, 0.6])
MX_BASE_MIRROR = (MX_BASE.astype(np.float64) @ np.diag([-1.0, 1.0, 1.0, 1.0])).astype(np.float32)


def source_for(Q, mx_align, mx_base):
    """Source points whose co_find = inv(mx_base) @ mx_align @ p lands on Q (up to float32 rounding)."""
    M = np.linalg.inv(mx_align.astype(np.float64)) @ mx_base.astype(np.float64)
    return (Q.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)


def co_find_of(src, mx_align, mx_base, orc):
    """The library's co_find, bit for bit (the oracle's float32 matrix arithmetic)."""
    if np.array_equal(mx_base, EYE) and np.array_equal(mx_align, EYE):
        return src.copy()
    inv = orc.mat4_inverted(mx_base)
    return np.array([orc.mat4_mul_vec3(inv, orc.mat4_mul_vec3(mx_align, p)) for p in src], np.float32)


def engine():
    from object_alignment_amd.engine import IcpEngine
    return IcpEngine(0)


ALL_OUT = ("signed_d", "dist", "closest", "idx", "feature")
POSES = (("identity", EYE, EYE), ("moved", MX_ALIGN, MX_BASE))


@gpu
def test_pseudonormals_match_restatement():
    meshes = {name: MESHES[name]() for name in CLOSED}
    meshes["lattice"] = synth.lattice_surface_mesh(12, 700)           # open, polar fans of 700
    for name, (V, T) in meshes.items():
        fn, vn, en = pseudonormals(V, T)
        got = []
        for _ in range(2):                                            # two builds on fresh contexts
            with engine() as eng:
                eng.set_target_mesh(V, T)
                assert eng.stat("mesh_pseudonormals") == 0.0
                got.append(eng.mesh_pseudonormals())
                assert eng.stat("mesh_pseudonormals") == 1.0
        (gv, ge), (gv2, ge2) = got
        assert gv.tobytes() == gv2.tobytes() and ge.tobytes() == ge2.tobytes(), name
        ev = np.linalg.norm(gv.astype(np.float64) - vn, axis=1) / np.linalg.norm(vn, axis=1)
        ee = np.linalg.norm(ge.astype(np.float64) - en, axis=2) / np.linalg.norm(en, axis=2)
        print("%s: vertex normals off by %.3g, edge normals by %.3g (relative)" % (name, ev.max(), ee.max()))
        assert ev.max() <= 1e-6 and ee.max() <= 1e-6, name
        # both triangles of every shared edge hold the same bits
        e0, e1 = T.astype(np.int64), np.roll(T, -1, axis=1).astype(np.int64)
        key = (np.minimum(e0, e1) * len(V) + np.maximum(e0, e1)).ravel()
        order = np.argsort(key, kind="stable")
        flat = ge.reshape(-1, 3).view(np.uint32)[order]
        same = key[order][1:] == key[order][:-1]
        assert np.sum(same) >= len(T) and np.array_equal(flat[1:][same], flat[:-1][same]), name


@gpu
@pytest.mark.parametrize("name", CLOSED)
def test_per_slot_outputs_exact(name, orc, tmp_path):
    f = fixture(name)
    V, T, Q = f["V"], f["T"], f["Q"]
    with engine() as eng:
        eng.set_target_mesh(V, T)
        for pose, mxa, mxb in POSES:
            src_all = source_for(Q, mxa, mxb) if pose == "moved" else Q
            for n in SIZES + (len(Q),):
                src = src_all[:n]
                eng.set_source(src)
                eng.set_matrices(mxa, mxb)
                idx, _, _ = eng.nn_search()
                dev = eng.deviation(outputs=ALL_OUT)
                assert np.array_equal(dev["idx"], idx) and np.all(idx >= 0)
                assert np.array_equal(np.abs(dev["signed_d"]).view(np.uint64), dev["dist"].view(np.uint64))
                assert dev["report"]["n"] == n == dev["report"]["n_valid"] and dev["report"]["surface"] == 1
                cf = co_find_of(src, mxa, mxb, orc)
                reg = host_regions(cf, V[T[idx, 0]], V[T[idx, 1]], V[T[idx, 2]], tmp_path)
                assert np.array_equal(dev["feature"], reg)
                if pose == "identity":
                    _, Bp, _ = eng.make_pairs(float("inf"))
                    assert Bp.shape[1] == n and np.array_equal(dev["closest"].astype(np.float64), Bp.T)
                    zero = np.float32(0.0)                            # (x + 0 carries a negative zero, which no product with the identity keeps, to +0)
                    assert np.array_equal((dev["closest"] + zero).view(np.uint32), (Bp.T.astype(np.float32) + zero).view(np.uint32))
                B64 = mxb.astype(np.float64)
                wa = cf.astype(np.float64) @ B64[:3, :3].T + B64[:3, 3]
                wb = dev["closest"].astype(np.float64) @ B64[:3, :3].T + B64[:3, 3]
                ref = np.linalg.norm(wa - wb, axis=1)
                ulp = np.spacing(np.maximum(np.abs(wa).max(axis=1), np.abs(wb).max(axis=1)).astype(np.float32)).astype(np.float64)
                assert np.all(np.abs(dev["dist"] - ref) <= 4.0 * ulp), float(np.max(np.abs(dev["dist"] - ref) / ulp))


@gpu
@pytest.mark.parametrize("name", CLOSED)
def test_sign_is_the_winding_numbers(name):
    f = fixture(name)
    V, T, Q, keep, inside = f["V"], f["T"], f["Q"], f["keep"], f["inside"]
    with engine() as eng:
        eng.set_target_mesh(V, T)
        signs = {}
        for pose, mxa, mxb in POSES + (("mirrored", MX_ALIGN, MX_BASE_MIRROR),):
            eng.set_source(source_for(Q, mxa, mxb) if pose != "identity" else Q)
            eng.set_matrices(mxa, mxb)
            dev = eng.deviation(signed=True, outputs=("signed_d",))
            neg = dev["signed_d"] < 0
            signs[pose] = neg
            wrong = np.flatnonzero(neg[keep] != inside[keep])
            assert len(wrong) == 0, (pose, wrong[:10])
            rep = dev["report"]
            assert rep["signed_used"] == 1 and rep["n_unsigned"] == 0 and rep["n_inside"] == int(np.sum(neg))
            if np.all(keep):
                assert rep["n_inside"] == int(np.sum(inside))
        assert np.array_equal(signs["moved"][keep], signs["mirrored"][keep])


def _doubles_bits(rep):
    skip = ("search_ms", "total_ms", "pseudonormal_ms", "quantiles")
    vals = [v for k, v in sorted(rep.items()) if k not in skip] + [v for _, v in sorted(rep["quantiles"].items())]
    return np.array(vals, np.float64).view(np.uint64).tolist()


@gpu
def test_search_mode_independence():
    f = fixture("bumpy2")
    src = source_for(f["Q"], MX_ALIGN, MX_BASE)
    kw = dict(thresh=0.2, outputs=ALL_OUT, bins=16, hist_range=(-0.1, 0.25))
    runs = []
    for mode in ("brute", "grid", "bvh", "bvh"):
        with engine() as eng:
            eng.set_search_mode(mode)
            eng.set_target_mesh(f["V"], f["T"])
            eng.set_source(src)
            eng.set_matrices(MX_ALIGN, MX_BASE)
            runs.append(eng.deviation(**kw))
            runs.append(eng.deviation(**kw))                          # seeded this time
    for r in runs[1:]:
        for k in ALL_OUT:
            assert r[k].tobytes() == runs[0][k].tobytes(), k
        assert np.array_equal(r["hist"], runs[0]["hist"])
        assert _doubles_bits(r["report"]) == _doubles_bits(runs[0]["report"])


def _hist_ref(d, lo, hi, n_bins):
    d = d[np.isfinite(d)]
    b = np.floor((d - lo) * (n_bins / (hi - lo)))
    mid = (d >= lo) & (d < hi)
    h = np.zeros(n_bins + 2, np.int64)
    h[0], h[-1] = np.sum(d < lo), np.sum(d >= hi)
    np.add.at(h, 1 + np.minimum(b[mid], n_bins - 1).astype(np.int64), 1)
    return h


def _check_stats(dev, thresh, quantiles):
    rep, dist, sd = dev["report"], dev["dist"], dev["signed_d"]
    valid = ~np.isnan(dist)
    n, dv = len(dist), dist[valid]
    inl = valid & (dist < thresh)
    assert (rep["n"], rep["n_valid"], rep["n_inlier"], rep["n_inside"]) == (n, int(valid.sum()), int(inl.sum()), int(np.sum(sd < 0)))
    assert rep["fitness"] == inl.sum() / n
    assert rep["max_dist"] == dv.max() and rep["max_index"] == int(np.flatnonzero(dist == dv.max())[0])
    k = np.sort(dv.astype(np.float32))
    for q in quantiles:
        assert rep["quantiles"][q] == float(k[int(math.ceil(q * len(k))) - 1]), q
    tol = n * 2.0 ** -50 * dv.max()
    assert abs(rep["mean"] - np.mean(dist[inl])) <= tol
    assert abs(rep["mean_signed"] - np.mean(sd[inl])) <= tol
    assert abs(rep["rms"] - math.sqrt(np.mean(dist[inl] ** 2))) <= tol
    assert abs(rep["rms"] ** 2 - np.mean(dist[inl] ** 2)) <= tol * dv.max()
    assert rep["std"] == math.sqrt(max(rep["rms"] * rep["rms"] - rep["mean"] * rep["mean"], 0.0))


@gpu
def test_statistics():
    f = fixture("bumpy2")
    quantiles = (0.5, 0.9, 0.95, 0.99, 1.0, 0.001, 0.25, 0.75)
    with engine() as eng:
        eng.set_target_mesh(f["V"], f["T"])
        for pose, mxa, mxb in POSES:
            src_all = source_for(f["Q"], mxa, mxb) if pose == "moved" else f["Q"]
            for n in SIZES + (len(src_all),):
                eng.set_source(src_all[:n])
                eng.set_matrices(mxa, mxb)
                dev = eng.deviation(quantiles=quantiles, outputs=ALL_OUT)
                _check_stats(dev, float("inf"), quantiles)
                assert dev["report"]["fitness"] == 1.0 and dev["hist"] is None
                again = eng.deviation(quantiles=quantiles, outputs=ALL_OUT)
                assert _doubles_bits(again["report"]) == _doubles_bits(dev["report"])
            # a threshold at the median: half of the points are inliers, and the statistics are theirs
            med = float(np.median(dev["dist"]))
            half = eng.deviation(thresh=med, quantiles=quantiles, outputs=ALL_OUT)
            _check_stats(half, med, quantiles)
            assert abs(half["report"]["fitness"] - 0.5) <= 1.0 / len(src_all)
            # histograms: points in both overflow bins, one value exactly on lo and one exactly on hi
            s = np.sort(dev["signed_d"])
            lo, hi = float(s[len(s) // 5]), float(s[(4 * len(s)) // 5])
            for n_bins in (1, 7, 256, 1024):
                h = eng.deviation(bins=n_bins, hist_range=(lo, hi), outputs=("signed_d",))
                ref = _hist_ref(h["signed_d"], lo, hi, n_bins)
                assert h["hist"].dtype == np.int64 and np.array_equal(h["hist"], ref), n_bins
                assert ref[0] > 0 and ref[-1] > 0 and ref[1] >= 1 and int(h["hist"].sum()) == len(s)


@gpu
def test_non_finite_sources():
    f = fixture("bumpy1")
    src = f["Q"][:300].copy()
    bad = np.array([0, 17, 63, 64, 130, 299])
    src[bad[:2]] = np.nan
    src[bad[2:4], 1] = np.inf
    src[bad[4:], 2] = -np.inf
    with engine() as eng:
        eng.set_target_mesh(f["V"], f["T"])
        eng.set_source(src)
        eng.set_matrices(EYE, EYE)
        dev = eng.deviation(outputs=ALL_OUT, bins=8, hist_range=(-0.2, 0.2))
    good = np.setdiff1d(np.arange(len(src)), bad)
    assert np.all(dev["idx"][bad] == -1) and np.all(dev["feature"][bad] == -1)
    assert np.all(np.isnan(dev["dist"][bad])) and np.all(np.isnan(dev["signed_d"][bad]))
    assert np.all(dev["idx"][good] >= 0) and np.all(np.isfinite(dev["dist"][good]))
    assert dev["report"]["n"] - dev["report"]["n_valid"] == len(bad)
    assert int(dev["hist"].sum()) == len(good)
    _check_stats(dev, float("inf"), (0.5, 0.9, 0.95, 0.99))


@gpu
def test_zero_area_triangles():
    V = np.array([[0.125, 0.0, 0.0], [-0.0625, 0.125, 0.0], [-0.0625, -0.125, 0.0], [0.0, 0.0, 2.0],
                  [0.03125, 0.0625, 0.0],                                   # exactly half way between vertices 0 and 1
                  [5.0, 0.0, 0.0], [6.0, 0.0, 0.0], [7.0, 0.0, 0.0]], np.float32)
    T_clean = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    T = np.concatenate([T_clean, [[0, 1, 4], [5, 6, 7]]]).astype(np.int32)
    with engine() as eng:
        eng.set_target_mesh(V[:4], T_clean)
        cv, ce = eng.mesh_pseudonormals()
        eng.set_target_mesh(V, T)
        assert eng.stat("mesh_pseudonormals") == 0.0                   # a new mesh forgets them
        gv, ge = eng.mesh_pseudonormals()
        assert np.array_equal(gv[:4], cv) and np.array_equal(ge[:4], ce)       # the flat triangle adds nothing to its neighbours
        # ... and takes none for itself, except on the edge it shares: that edge's sum, the same bits as in its neighbours
        assert not np.any(gv[4:]) and not np.any(ge[4, 1:]) and not np.any(ge[5]) and np.array_equal(ge[4, 0], ge[1, 0])
        fn, vn, en = pseudonormals(V, T)
        assert np.allclose(gv, vn, rtol=1e-6, atol=0) and np.allclose(ge, en, rtol=1e-6, atol=0)
        src = np.array([[6.0, 0.1, 0.0], [0.0, 0.0, 2.5], [0.0, 0.0, 0.5]], np.float32)
        eng.set_source(src)
        eng.set_matrices(EYE, EYE)
        dev = eng.deviation(outputs=ALL_OUT)
    assert dev["idx"][0] == 5 and dev["report"]["n_unsigned"] == 1 and dev["signed_d"][0] == dev["dist"][0] > 0
    assert dev["signed_d"][1] > 0 and dev["signed_d"][2] < 0 and dev["report"]["n_inside"] == 1


@gpu
def test_vertex_mode_targets():
    from object_alignment_amd.engine import IcpEngine                 # noqa: F401
    tgt, nrm = synth.bunny_surface_with_normals(2000)
    rng = np.random.default_rng(5)
    src = (tgt[rng.integers(0, len(tgt), 257)].astype(np.float64) * rng.uniform(0.9, 1.1, (257, 1))).astype(np.float32)
    with engine() as eng:
        eng.set_target(tgt)
        eng.set_source(src)
        eng.set_matrices(EYE, EYE)
        dev = eng.deviation(outputs=ALL_OUT)
        assert dev["report"]["signed_used"] == 0 and dev["report"]["surface"] == 0 and dev["report"]["n_inside"] == 0
        assert np.array_equal(dev["signed_d"], dev["dist"]) and np.all(dev["feature"] == -1)
        assert np.array_equal(dev["closest"], tgt[dev["idx"]])
        with pytest.raises(_capi.OaError) as exc:
            eng.deviation(signed=True)
        assert exc.value.code == _capi.OA_E_STATE
        assert eng.deviation(signed=False)["report"]["signed_used"] == 0
        eng.set_target_normals(nrm)
        sig = eng.deviation(signed=True, outputs=ALL_OUT)
        assert sig["report"]["signed_used"] == 2 and np.array_equal(sig["dist"], dev["dist"]) and np.array_equal(sig["idx"], dev["idx"])
        d = src.astype(np.float64) - tgt[sig["idx"]].astype(np.float64)
        s = np.sum(d * nrm[sig["idx"]].astype(np.float64), axis=1)
        sure = np.abs(s) > 1e-9
        assert np.array_equal((sig["signed_d"] < 0)[sure], (s < 0)[sure]) and 0 < sig["report"]["n_inside"] < len(src)
        _check_stats(sig, float("inf"), (0.5, 0.9, 0.95, 0.99))


@gpu
def test_multi_device_refused_and_usable():
    from object_alignment_amd.engine import IcpEngine
    f = fixture("bumpy1")
    with IcpEngine(devices=[0, 0]) as eng:
        eng.set_target_mesh(f["V"], f["T"])
        eng.set_source(f["Q"][:257])
        eng.set_matrices(EYE, EYE)
        with pytest.raises(_capi.OaError) as exc:
            eng.deviation()
        assert exc.value.code == _capi.OA_E_STATE
        idx, _, _ = eng.nn_search()
    with engine() as one:
        one.set_target_mesh(f["V"], f["T"])
        one.set_source(f["Q"][:257])
        one.set_matrices(EYE, EYE)
        assert np.array_equal(one.deviation(outputs=("idx",))["idx"], idx)


@gpu
def test_report_alone_and_rebuild():
    f, g = fixture("bumpy1"), fixture("needle")
    with engine() as eng:
        eng.set_target_mesh(f["V"], f["T"])
        eng.set_source(f["Q"])
        eng.set_matrices(EYE, EYE)
        full = eng.deviation(outputs=ALL_OUT)
        bare = eng.deviation(outputs=())                               # every output pointer NULL
        assert set(bare) == {"report", "hist"} and _doubles_bits(bare["report"]) == _doubles_bits(full["report"])
        assert eng.stat("mesh_pseudonormals") == 1.0
        eng.set_target_mesh(g["V"], g["T"])
        assert eng.stat("mesh_pseudonormals") == 0.0
        eng.set_source(g["Q"])
        eng.set_matrices(EYE, EYE)
        dev = eng.deviation(outputs=("signed_d",))
        assert eng.stat("mesh_pseudonormals") == 1.0 and dev["report"]["pseudonormal_ms"] > 0.0
        assert np.array_equal((dev["signed_d"] < 0)[g["keep"]], g["inside"][g["keep"]])
        unsigned = eng.deviation(signed=False, outputs=("signed_d", "dist"))
        assert unsigned["report"]["signed_used"] == 0 and np.array_equal(unsigned["signed_d"], unsigned["dist"])


@gpu
def test_through_the_public_surface():
    import object_alignment_amd
    V, T = synth.bumpy_icosphere_mesh(3)
    src = synth.bumpy_icosphere(3)
    start = synth.rigid4(synth.rotation_from_rotvec([0.05, -0.04, 0.06]), [0.03, -0.02, 0.025])
    with engine() as eng:
        plain = IcpAlign(IcpSettings(), engine=eng).run(src, V, start, EYE, target_tris=T)
        assert plain.deviation is None
        eng.set_matrices(start, EYE)
        before = eng.deviation(thresh=0.5)["report"]
        res = IcpAlign(IcpSettings(), engine=eng).run(src, V, start, EYE, target_tris=T, deviation=DeviationSettings())
    assert res.iters_done == plain.iters_done and res.matrix_world.tobytes() == plain.matrix_world.tobytes()
    rep = res.deviation["report"]
    assert rep["thresh"] == 0.5 and rep["n"] == len(src) // 2 and rep["signed_used"] == 1
    assert rep["rms"] < before["rms"] and rep["fitness"] == 1.0
    one = object_alignment_amd.deviation(src[::2], V, T, mx_align=res.matrix_world, mx_base=EYE, thresh=0.5)
    for k in ("signed_d", "closest", "idx", "feature"):
        assert one[k].tobytes() == res.deviation[k].tobytes(), k
    assert _doubles_bits(one["report"]) == _doubles_bits(rep)
