"""Radius-limited neighbourhoods and the cloud's own point spacing: oa_set_neighbor_radius / oa_get_neighbor_radius /
oa_target_spacing, IcpEngine.set_neighbor_radius / neighbor_radius / target_spacing, the radius= keyword of target_knn,
estimate_target_normals, target_fpfh and target_boundary, object_alignment_amd.cloud_spacing and the radius= of estimate_normals /
fpfh / cloud_boundary, IcpSettings.normal_radius / boundary_radius and CoarseSettings.feature_radius.

The contract is restated in numpy below (knn_radius_ref): fp64 squared distances, rows ascending by (d2, index), entries beyond
r2 = (float32 radius)^2 dropped, rows padded with -1 / +inf.  PCA, FPFH and the boundary criterion of such rows are the
restatements of tests/test_target_normals.py, tests/test_feature_align.py and tests/test_boundary.py."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from object_alignment_amd import synth
from test_boundary import cloud_boundary_ref, near_threshold
from test_clustering import lattice_case, r2_of
from test_feature_align import fpfh_numpy
from test_target_normals import EIG_GAP, angle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24
NEAR_R2 = 1e-6        # relative distance of an fp64 squared distance from r2 below which the float32 metric may decide the other way
TIE = 1e-5            # relative gap of two fp64 squared distances below which the float32 metric may order them the other way
K = 16
SHEET_RADII = (0.035, 0.04, 0.045)
MULTIPLES = (2, 4, 8)
BAD_RADII = (-1.0, float("inf"), float("nan"), 1.9e19, "0.1", True)       # (and 0 where a value is required)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build_hip()
    return g


# ------------------------------------------------------------------------------------------------ the clouds
@functools.lru_cache(maxsize=None)
def two_sheets():
    """two parallel sheets 0.05 apart, 2 000 uniform points each on the unit square"""
    rng = np.random.default_rng(5)
    a, b = rng.uniform(0, 1, (2000, 2)), rng.uniform(0, 1, (2000, 2))
    return np.concatenate([np.c_[a, np.zeros(2000)], np.c_[b, np.full(2000, 0.05)]]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cloud(name):
    if name == "bunny":
        return synth.bunny_surface(700, 0.21)
    if name == "sheets":
        return two_sheets()
    if name == "holes":                                             # the 65-point lattice case: two non-finite vertices, one point three times
        x = lattice_case(65).copy()
        x[7, 1] = np.nan
        x[20, 2] = np.inf
        x[30] = x[12]
        x[31] = x[12]
        return x
    return lattice_case(int(name))


# ------------------------------------------------------------------------------------------------ the numpy restatement
def knn_radius_ref(xyz, k, r=None):
    """(idx int32 (n, k), d2 fp64 (n, k), raw fp64 (n, min(k + 1, n)): the nearest squared distances before the cut).  fp64 squared
    distances of the float32 coordinates, rows ascending by (d2, index), self included; entries with d2 > r2_of(r) dropped (r None:
    none), rows padded with -1 / +inf; a non-finite vertex has an empty row and is in nobody's row."""
    x = np.asarray(xyz, np.float32).astype(np.float64)
    n, kk = len(x), min(k + 1, len(x))
    finite = np.isfinite(x).all(axis=1)
    idx, raw = np.empty((n, kk), np.int64), np.empty((n, kk), np.float64)
    for b in range(0, n, 512):
        with np.errstate(all="ignore"):
            d = ((x[b:b + 512, None, :] - x[None, :, :]) ** 2).sum(axis=2)
        d[~finite[b:b + 512], :] = np.inf
        d[:, ~finite] = np.inf
        o = np.argsort(d, axis=1, kind="stable")[:, :kk]            # stable: lowest index first on ties
        idx[b:b + 512] = o
        raw[b:b + 512] = np.take_along_axis(d, o, axis=1)
    keep = np.isfinite(raw[:, :k])
    if r is not None:
        keep &= raw[:, :k] <= r2_of(r)
    pad = np.zeros((n, k - min(k, kk)), bool)
    keep = np.concatenate([keep, pad], axis=1)
    full_i = np.concatenate([idx[:, :k], np.zeros((n, k - min(k, kk)), np.int64)], axis=1)
    full_d = np.concatenate([raw[:, :k], np.zeros((n, k - min(k, kk)))], axis=1)
    return np.where(keep, full_i, -1).astype(np.int32), np.where(keep, full_d, np.inf), raw


def guarded_rows(raw, r=None):
    """rows in which some fp64 d2 lies within NEAR_R2 relative of r2, or in which two successive d2 that matter (the smaller one
    inside the radius) lie within TIE relative of each other: there the float32 metric may give another row than fp64"""
    with np.errstate(invalid="ignore"):
        a, b = raw[:, :-1], raw[:, 1:]
        tie = np.isfinite(b) & ((b - a) <= TIE * b)
        if r is None:
            return tie.any(axis=1)
        r2 = r2_of(r)
        near = np.isfinite(raw) & (np.abs(raw - r2) <= NEAR_R2 * r2)
        return near.any(axis=1) | (tie & (a <= r2 * (1.0 + NEAR_R2))).any(axis=1)


def spacing_ref(xyz):
    """fp64 mean distance to the nearest other point"""
    raw = knn_radius_ref(xyz, 2)[2]
    s = np.sqrt(raw[:, 1])
    return float(s[np.isfinite(s)].mean())


def round3(v):
    return float("%.3g" % v)


@functools.lru_cache(maxsize=None)
def general_radii(name):
    """2, 4 and 8 x the cloud's spacing, the spacing rounded to three digits so that the restated and the measured one agree"""
    s = round3(spacing_ref(cloud(name)))
    return tuple(m * s for m in MULTIPLES)


def pairs_used():
    """every (cloud, radius) the GPU tests use on general clouds: the rows at the spacing's multiples, the capability's radii"""
    out = [(name, r) for name in ("bunny", "sheets") for r in general_radii(name)]
    return out + [("sheets", r) for r in SHEET_RADII]


@functools.lru_cache(maxsize=None)
def general_ref(name, r):
    idx, d2, raw = knn_radius_ref(cloud(name), K, r)
    return idx, d2, guarded_rows(raw, r)


def pca_rows_ref(xyz, idx):
    """(normal fp64 (n, 3) of arbitrary sign -- zero for rows of fewer than 3 neighbours --, curvature, eigenvalues ascending
    (n, 3), m (n,)) from rows padded with -1: the mean of the m filled entries, then centred products, both summed in list order;
    numpy.linalg.eigh (test_target_normals.pca_ref for rows of any length)."""
    x = np.asarray(xyz, np.float32).astype(np.float64)
    idx = np.asarray(idx, np.int64)
    valid = idx >= 0
    m = valid.sum(axis=1)
    nb = x[np.where(valid, idx, 0)]
    s = np.zeros((len(idx), 3))
    for j in range(idx.shape[1]):
        s += np.where(valid[:, j, None], nb[:, j], 0.0)
    d = nb - (s / np.maximum(m, 1)[:, None])[:, None, :]
    cov = np.zeros((len(idx), 3, 3))
    for j in range(idx.shape[1]):
        cov += np.where(valid[:, j, None, None], d[:, j, :, None] * d[:, j, None, :], 0.0)
    lam, vec = np.linalg.eigh(cov)
    few = m < 3
    tot = lam.sum(axis=1)
    curv = np.where(few | (tot <= 0.0), 0.0, lam[:, 0] / np.where(tot > 0.0, tot, 1.0))
    return np.where(few[:, None], 0.0, vec[:, :, 0]), curv, lam, m


def within_10_degrees_of_z(n):
    n = np.asarray(n, np.float64)
    length = np.linalg.norm(n, axis=1)
    return (length > 0) & (np.abs(n[:, 2]) >= np.cos(np.radians(10.0)) * np.where(length > 0, length, 1.0))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _engine(xyz, **kw):
    from object_alignment_amd.engine import IcpEngine
    e = IcpEngine(0, **kw)
    e.set_target(xyz)
    return e


# ------------------------------------------------------------------------------------------------ CPU
def test_radius_abi_and_bindings(built):
    """The header, both library flavours and the bindings name the three calls; the report has the header's fields and size."""
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    hdr = open(os.path.join(ROOT, "include", "oa_icp.h")).read()
    assert re.search(r"\bint\s+oa_set_neighbor_radius\s*\(oa_ctx \*ctx, float radius\);", hdr)
    assert re.search(r"\bint\s+oa_get_neighbor_radius\s*\(oa_ctx \*ctx, float \*radius\);", hdr)
    assert re.search(r"\bint\s+oa_target_spacing\s*\(oa_ctx \*ctx, oa_spacing_report \*rep\);", hdr)
    for name in ("oa_set_neighbor_radius", "oa_get_neighbor_radius", "oa_target_spacing"):
        assert name in _capi.SYMBOLS
        for lib in ("liboa_icp.so", "liboa_icp_exp.so"):
            assert hasattr(C.CDLL(os.path.join(ROOT, "object_alignment_amd", lib)), name), (lib, name)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    body = re.search(r"typedef struct oa_spacing_report \{(.*?)\} oa_spacing_report;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(n.strip(), ctype[t]) for t, names in re.findall(r"(int32_t|int64_t|double)\s+([^;]+);", body) for n in names.split(",")]
    assert fields == list(_capi.SpacingReport._fields_) and C.sizeof(_capi.SpacingReport) == 32
    assert tuple(n for n, _ in fields) == ("mean", "std", "n_finite", "n_nonfinite")
    for name in ("set_neighbor_radius", "target_spacing"):
        assert callable(getattr(IcpEngine, name))
    assert isinstance(IcpEngine.neighbor_radius, property)


def test_radius_argument_errors_touch_no_device():
    """Every bad radius is refused in Python: by the engine's methods before the library is called, by the module-level functions
    before a context opens, by the settings when they are made and again by IcpAlign.run before an engine is touched."""
    import object_alignment_amd as oa
    from object_alignment_amd.engine import IcpEngine, _radius_arg
    from object_alignment_amd.operators.coarse_align import CoarseSettings
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("touched (%s)" % name)

    eng = object.__new__(IcpEngine)
    eng._L, eng._h, eng.n_target = Untouchable(), None, 40
    pts = np.zeros((40, 3), np.float32)
    eye = np.eye(4, dtype=np.float32)
    for bad in BAD_RADII:
        with pytest.raises(ValueError):
            eng.set_neighbor_radius(bad)
    for bad in (0, 0.0) + BAD_RADII:
        for call in (lambda: eng.target_knn(4, radius=bad), lambda: eng.estimate_target_normals(k=8, radius=bad),
                     lambda: eng.target_fpfh(k=8, radius=bad), lambda: eng.target_boundary(radius=bad),
                     lambda: oa.estimate_normals(pts, radius=bad), lambda: oa.fpfh(pts, radius=bad),
                     lambda: oa.cloud_boundary(pts, "estimate", radius=bad), lambda: oa.cloud_boundary(pts, pts, radius=bad),
                     lambda: IcpSettings(normal_radius=bad), lambda: IcpSettings(boundary_radius=bad),
                     lambda: CoarseSettings(feature_radius=bad), lambda: _radius_arg(bad)):
            with pytest.raises(ValueError):
                call()
        for field in ("normal_radius", "boundary_radius"):          # a setting changed after it was made
            for engine in (Untouchable(), None):
                s = IcpSettings()
                setattr(s, field, bad)
                op = IcpAlign(s, engine=engine)
                with pytest.raises(ValueError):
                    op.run(pts, pts, eye, eye, target_normals="estimate")
                assert op._engine is engine
    assert _radius_arg(0, off_ok=True) == 0.0 and _radius_arg(0.045) == float(np.float32(0.045)) and _radius_arg(np.float32(2)) == 2.0
    assert _radius_arg(1.8e19) == float(np.float32(1.8e19)) and _radius_arg(1) == 1.0
    with pytest.raises(ValueError):
        _radius_arg(1e-60)                                          # (0 as a float32: it would read as "no limit")
    s = IcpSettings()
    assert s.normal_radius is None and s.boundary_radius is None and CoarseSettings().feature_radius is None


def test_fixture_guard():
    """For every (cloud, radius) the GPU tests compare rows at: the rows in which the float32 metric may decide another way than
    fp64 -- a d2 within 1e-6 relative of r2, or two successive d2 within 1e-5 of each other -- are at most 1 % of the cloud; on the
    two-sheet cloud no d2 among a vertex's 16 nearest lies within 1e-6 of r2 at 0.035, 0.04 and 0.045."""
    for name, r in pairs_used():
        raw = knn_radius_ref(cloud(name), K, r)[2]
        g = general_ref(name, r)[2]
        r2 = r2_of(r)
        near = int((np.abs(raw - r2) <= NEAR_R2 * r2).any(axis=1).sum())
        print("guard: %s at radius %.6g: %d of %d rows left out (%d for a d2 next to r2)" % (name, r, int(g.sum()), len(g), near))
        assert g.mean() <= 0.01, (name, r)
        if name == "sheets" and r in SHEET_RADII:
            assert near == 0
    for name in ("bunny", "sheets"):
        g = guarded_rows(knn_radius_ref(cloud(name), K)[2])
        print("guard: %s without a radius: %d of %d rows left out" % (name, int(g.sum()), len(g)))
        assert g.mean() <= 0.01
    assert abs(spacing_ref(two_sheets()) - 0.01125) < 5e-6


def test_capability_guard():
    """The restatement alone, two sheets 0.05 apart at k = 16: without a radius the neighbours reach the other sheet and fewer than
    80 % of the PCA normals are within 10 degrees of +-z; within 0.045 at least 99 % are, and at most 5 vertices have fewer than
    three neighbours."""
    xyz = two_sheets()
    free = pca_rows_ref(xyz, knn_radius_ref(xyz, K)[0])[0]
    n, _, _, m = pca_rows_ref(xyz, knn_radius_ref(xyz, K, 0.045)[0])
    share_free, share = float(within_10_degrees_of_z(free).mean()), float(within_10_degrees_of_z(n).mean())
    few = [int(((knn_radius_ref(xyz, K, r)[0] >= 0).sum(axis=1) < 3).sum()) for r in (0.045, 0.04, 0.035)]
    print("capability: %.2f %% without a radius, %.2f %% within 0.045; fewer than 3 neighbours at 0.045 / 0.04 / 0.035: %s"
          % (100 * share_free, 100 * share, few))
    assert share_free < 0.80 and share >= 0.99 and int((m < 3).sum()) <= 5
    assert few == [1, 4, 33]


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 64, 65, 4097])
def test_gpu_rows_on_lattices_under_ties(built, n):
    """Integer lattices with one far point (a partial leaf, then one, two and three box levels): the float32 metric is exact and
    d2 == r2 occurs everywhere -- indices equal, d2 bit for bit, rows of the query alone and the far point's included."""
    pts = cloud(str(n))
    with _engine(pts) as e:
        for r in (1.0, 1.5, 2.0):
            ridx, rd2, _ = knn_radius_ref(pts, min(64, n), r)
            if n == 4097:                                            # (1.5: 2.25 is no sum of three squares)
                assert (rd2 == r2_of(r)).any() == (r != 1.5)
            assert ridx[n - 1, 0] == n - 1 and (ridx[n - 1, 1:] == -1).all()
            for k in sorted({min(k, n) for k in (1, 4, 16, 64)}):
                idx, d2 = e.target_knn(k, radius=r)
                assert idx.dtype == np.int32 and d2.dtype == np.float32 and idx.shape == (n, k)
                assert np.array_equal(idx, ridx[:, :k]), (n, r, k)
                assert np.array_equal(bits(d2), bits(rd2[:, :k].astype(np.float32))), (n, r, k)
        assert e.neighbor_radius == 0.0


@pytest.mark.gpu
def test_gpu_rows_with_non_finite_vertices_and_duplicates(built):
    pts = cloud("holes")
    with _engine(pts) as e:
        for r in (None, 1.0, 1.5, 2.0):
            ridx, rd2, _ = knn_radius_ref(pts, K, r)
            idx, d2 = e.target_knn(K) if r is None else e.target_knn(K, radius=r)
            assert np.array_equal(idx, ridx) and np.array_equal(bits(d2), bits(rd2.astype(np.float32))), r
            for bad in (7, 20):                                     # empty rows, and in nobody's row
                assert (idx[bad] == -1).all() and np.isinf(d2[bad]).all() and not (idx == bad).any()
            for a in (12, 30, 31):                                  # every copy is in the rows of the others, at distance 0
                assert set(idx[a, :3].tolist()) == {12, 30, 31} and (d2[a, :3] == 0).all()
            n, curv = e.estimate_target_normals(k=K, install=False) if r is None else e.estimate_target_normals(k=K, install=False, radius=r)
            few = (idx >= 0).sum(axis=1) < 3
            assert not n[few].any() and not curv[few].any() and few[7] and few[20]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bunny", "sheets"])
def test_gpu_general_clouds(built, name):
    """Rows, normals, descriptors and the boundary mask at 2, 4 and 8 x the cloud's spacing."""
    import object_alignment_amd as oa
    pts = cloud(name)
    x = pts.astype(np.float64)
    assert round3(oa.cloud_spacing(pts)["mean"]) == round3(spacing_ref(pts))   # (the radii below are multiples of this figure)
    with _engine(pts) as e:
        for r in general_radii(name):
            ridx, rd2, guarded = general_ref(name, r)
            idx, d2 = e.target_knn(K, radius=r)
            ok = ~guarded
            assert np.array_equal(idx[ok], ridx[ok]), (name, r)
            filled = idx >= 0
            exact = ((x[:, None, :] - x[np.where(filled, idx, 0)]) ** 2).sum(axis=2)
            rel = np.abs(d2.astype(np.float64) - exact)[filled] / np.where(exact[filled] > 0.0, exact[filled], 1.0)
            assert np.all(rel <= 6.0 * U32) and np.all(d2[filled] <= np.float32(r2_of(r))) and np.isinf(d2[~filled]).all()
            # normals: the restated PCA over the device's own rows, to test_target_normals' tolerance
            rn, rcurv, lam, m = pca_rows_ref(pts, idx)
            n, curv = e.estimate_target_normals(k=K, orient="none", install=True, radius=r)
            few = m < 3
            assert not n[few].any() and not curv[few].any()
            held = ~few & ((lam[:, 1] - lam[:, 0]) >= EIG_GAP * lam[:, 2])
            ang = angle(n[held], rn[held])
            length = np.linalg.norm(n[~few].astype(np.float64), axis=1)
            cerr = np.abs(curv.astype(np.float64) - rcurv)
            print("%s r=%.4g: %d short rows, %d with fewer than 3, %d held; largest angle %.3g rad, curvature error %.3g"
                  % (name, r, int((m < K).sum()), int(few.sum()), int(held.sum()), ang.max(), cerr.max()))
            assert held.any() and np.all(ang <= 1e-6)
            assert np.all((np.abs(length - 1.0) <= 2.0 ** -22) | (length == 0.0))
            assert np.all(cerr <= 1e-7 + 1e-6 * np.abs(rcurv))
            # descriptors and the boundary mask: their restatements over the device's own rows and normals
            ref, left_out = fpfh_numpy(pts, n, idx)
            got = e.target_fpfh(k=K, keep=False, radius=r)
            assert np.abs(got.astype(np.float64) - ref)[~left_out].max() <= 1e-4
            rows17, _ = e.target_knn(K + 1, radius=r)
            want, gaps = cloud_boundary_ref(pts, n, rows17, K, 90.0)
            close = near_threshold(gaps, 90.0, 1e-9)
            mask, edges = e.target_boundary(K, 90.0, radius=r)
            keep = np.ones(len(pts), bool)
            keep[close] = False
            assert edges is None and np.array_equal(mask[keep], want[keep]) and len(close) <= 0.01 * len(pts)
            assert e.neighbor_radius == 0.0


@pytest.mark.gpu
def test_gpu_capability_on_the_device(built):
    xyz = two_sheets()
    with _engine(xyz) as e:
        free, _ = e.estimate_target_normals(k=K, install=False)
        n, _ = e.estimate_target_normals(k=K, install=False, radius=0.045)
    share_free, share = float(within_10_degrees_of_z(free).mean()), float(within_10_degrees_of_z(n).mean())
    zero = int((~n.any(axis=1)).sum())
    print("device: %.2f %% without a radius, %.2f %% within 0.045, %d zero normals" % (100 * share_free, 100 * share, zero))
    assert share_free < 0.80 and share >= 0.99 and zero <= 5


def _everything(e, radius=None):
    kw = {} if radius is None else {"radius": radius}
    idx, d2 = e.target_knn(K, **kw)
    n, curv = e.estimate_target_normals(k=K, orient="none", install=True, **kw)
    return [idx.tobytes(), d2.tobytes(), n.tobytes(), curv.tobytes(), e.target_fpfh(k=K, keep=False, **kw).tobytes(),
            e.target_boundary(K, 90.0, **kw)[0].tobytes()]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bunny", "holes"])
def test_gpu_unlimited_is_unchanged(built, name):
    """radius=None, set_neighbor_radius(0) and a radius of twice the cloud's diagonal: the same bytes everywhere."""
    pts = cloud(name)
    fin = pts[np.isfinite(pts).all(axis=1)].astype(np.float64)
    diag = float(np.linalg.norm(fin.max(axis=0) - fin.min(axis=0)))
    with _engine(pts) as e:
        plain = _everything(e)
        e.set_neighbor_radius(0.37)
        e.set_neighbor_radius(0)
        assert _everything(e) == plain
        assert _everything(e, radius=2.0 * diag) == plain
        e.set_neighbor_radius(2.0 * diag)
        assert _everything(e) == plain
        e.set_neighbor_radius(None)
        assert e.neighbor_radius == 0.0 and _everything(e) == plain


@pytest.mark.gpu
def test_gpu_the_setting_stays_where_it_belongs(built):
    from object_alignment_amd import _capi
    pts = cloud("bunny")
    s = round3(spacing_ref(pts))

    def others(e):
        out = e.target_outliers("statistical", k=8)
        cl = e.target_clusters(3 * s, min_points=4)
        on, fl, comp, rep = e.orient_target_normals(k=8, install=False)
        return [out["keep"].tobytes(), out["score"].tobytes(), repr(sorted(out["report"].items())), e.target_radius_count(3 * s).tobytes(),
                cl["label"].tobytes(), cl["sizes"].tobytes(), repr(sorted(cl["report"].items())), on.tobytes(), fl.tobytes(), comp.tobytes(),
                repr(sorted(rep.items())), repr(sorted(e.target_spacing().items()))]

    with _engine(pts) as e:
        e.estimate_target_normals(k=K, orient="away", install=True)
        plain = others(e)
        e.set_neighbor_radius(1.5 * s)
        assert e.neighbor_radius == float(np.float32(1.5 * s))      # the float32 that was set
        assert (e.target_knn(K)[0] == -1).any()                      # (it is small enough to cut rows)
        assert others(e) == plain
        # the keyword restores the previous value, after a refused call too
        before = e.target_knn(K)[0]
        wide = e.target_knn(K, radius=6 * s)[0]
        assert e.neighbor_radius == float(np.float32(1.5 * s)) and not np.array_equal(before, wide)
        with pytest.raises(_capi.OaError):
            e.target_knn(len(pts) + 1, radius=6 * s)
        with pytest.raises(_capi.OaError):
            e.estimate_target_normals(k=2, radius=6 * s)
        assert e.neighbor_radius == float(np.float32(1.5 * s)) and np.array_equal(e.target_knn(K)[0], before)
        e.set_target(pts)                                            # the setting survives an upload
        assert e.neighbor_radius == float(np.float32(1.5 * s)) and np.array_equal(e.target_knn(K)[0], before)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["65", "4097", "holes", "bunny", "sheets"])
def test_gpu_spacing(built, name):
    """mean and std against fp64 numpy over sqrt((double)d2) of the device's own target_knn(2) rows; the counts exact."""
    import object_alignment_amd as oa
    pts = cloud(name)
    with _engine(pts) as e:
        e.set_neighbor_radius(1e-3)                                  # (it does not apply: target_knn below runs without it)
        rep = e.target_spacing()
        again = e.target_spacing()
        e.set_neighbor_radius(0)
        _, d2 = e.target_knn(2)
    s = np.sqrt(d2[:, 1].astype(np.float64))
    s = s[np.isfinite(s)]
    mean = float(s.sum() / len(s))
    std = float(np.sqrt(((s - mean) ** 2).sum() / (len(s) - 1)))
    print("%s: spacing %.9g +- %.9g over %d of %d vertices" % (name, rep["mean"], rep["std"], rep["n_finite"], len(pts)))
    assert abs(rep["mean"] - mean) <= 1e-12 * mean and abs(rep["std"] - std) <= 1e-12 * std
    assert rep["n_finite"] == len(s) and rep["n_nonfinite"] == len(pts) - len(s)
    assert rep["n_nonfinite"] == int((~np.isfinite(pts).all(axis=1)).sum()) == (2 if name == "holes" else 0)
    assert again == rep and np.float64(again["mean"]).tobytes() == np.float64(rep["mean"]).tobytes()
    assert oa.cloud_spacing(pts) == rep
    if name == "holes":
        assert s.min() == 0.0                                        # a duplicate gives 0


def _recording_engine():
    from object_alignment_amd.engine import IcpEngine

    class Recording(IcpEngine):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.seen = []

        def estimate_target_normals(self, *a, **kw):
            out = super().estimate_target_normals(*a, **kw)
            self.seen.append(("normals", kw.get("radius"), out[0].copy()))
            return out

        def target_fpfh(self, *a, **kw):
            out = super().target_fpfh(*a, **kw)
            self.seen.append(("fpfh", kw.get("radius"), out.copy()))
            return out

    return Recording(0)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_gpu_through_the_operator(built, scale):
    """IcpSettings.normal_radius / boundary_radius and CoarseSettings.feature_radius are world lengths: each reaches its call
    divided by the target's world scale, and what the engine then holds is what the direct call with that radius gives."""
    from object_alignment_amd.operators.coarse_align import CoarseSettings
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings
    tgt = two_sheets()
    mxb = np.diag([scale, scale, scale, 1.0]).astype(np.float32)
    P = synth.rigid4(synth.rotation_from_rotvec([0.01, -0.008, 0.012]), [0.004, -0.003, 0.002], dtype=np.float64)
    src = tgt[::3].copy()
    mxa = (P @ mxb.astype(np.float64)).astype(np.float32)
    # world lengths: 0.045, 0.03 and 0.035 of the target's own unit.  The 16 nearest of this cloud lie within about 0.05, so
    # the last two must stay below that to cut rows at all (the restatement: 0.03 changes 2 633 mask bytes, 0.035 changes 3 423
    # descriptor rows; at 0.06 the mask and at 0.09 both are what they are without a radius)
    nr, br, fr = 0.045 * scale, 0.03 * scale, 0.035 * scale
    # what the library receives: the float32 of the world length over the world scale (the scale itself is a cube root in
    # fp64, so the quotient is compared after the rounding to float32 that the engine applies)
    local = lambda r: float(np.float32(float(np.float32(r)) / scale))    # noqa: E731
    with _engine(tgt) as f:
        want_n, _ = f.estimate_target_normals(k=K, orient="away", install=True, radius=local(nr))
        free_n, _ = f.estimate_target_normals(k=K, orient="away", install=False)
        want_f = f.target_fpfh(k=K, keep=False, radius=local(fr))
        free_f = f.target_fpfh(k=K, keep=False)
        want_b = f.target_boundary(K, 90.0, radius=local(br))[0].copy()
        free_b = f.target_boundary(K, 90.0)[0].copy()
    assert not np.array_equal(want_n, free_n) and not np.array_equal(want_f, free_f) and not np.array_equal(want_b, free_b)
    with _recording_engine() as e:
        op = IcpAlign(IcpSettings(metric="plane", normal_radius=nr, icp_iterations=3, min_start=0.2 * scale), engine=e)
        res = op.run(src, tgt, mxa, mxb, target_normals="estimate")
        assert res.iters_done >= 1 and [c[0] for c in e.seen] == ["normals"]
        assert np.float32(e.seen[0][1]) == np.float32(local(nr)) and np.array_equal(bits(e.seen[0][2]), bits(want_n))
        assert e.neighbor_radius == 0.0
        # the coarse stage's descriptors and the loop's boundary mask
        e.seen.clear()
        coarse = CoarseSettings(method="features", feature_radius=fr, n_hyp=64, n_refine=1, refine_iters=1, thresh=0.2 * scale)
        op = IcpAlign(IcpSettings(metric="plane", normal_radius=nr, reject_boundary=True, boundary_radius=br, icp_iterations=3,
                                  min_start=0.2 * scale), engine=e)
        op.run(src, tgt, mxa, mxb, target_normals="estimate", coarse=coarse)
        assert [c[0] for c in e.seen] == ["normals", "fpfh"]
        assert np.float32(e.seen[1][1]) == np.float32(local(fr)) and np.array_equal(bits(e.seen[1][2]), bits(want_f))
        assert e.neighbor_radius == 0.0
        assert e.stat("target_boundary") == 1.0 and e.stat("boundary_vertices") == float(want_b.sum())
        e.set_neighbor_radius(local(br))                             # the mask the loop built is keyed by its radius: no rebuild changes it
        assert np.array_equal(e.target_boundary(K, 90.0)[0], want_b)
        e.set_neighbor_radius(0)
        assert np.array_equal(e.target_boundary(K, 90.0)[0], free_b)


@pytest.mark.gpu
def test_gpu_refusals_leave_the_context_usable(built):
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    pts = cloud("bunny")
    s = round3(spacing_ref(pts))
    verts, tris = synth.icosphere_mesh(2)
    with _engine(pts) as f:
        want = f.target_knn(K, radius=3 * s)
        want_sp = f.target_spacing()
    with IcpEngine(0) as e:
        L, h = e._L, e._h
        rep = _capi.SpacingReport()
        assert L.oa_target_spacing(h, C.byref(rep)) == _capi.OA_E_STATE          # no target
        assert L.oa_target_spacing(h, None) == _capi.OA_E_BAD_ARG
        e.set_target_mesh(verts, tris)
        assert L.oa_target_spacing(h, C.byref(rep)) == _capi.OA_E_STATE          # a surface target
        e.set_target(pts)
        e.set_neighbor_radius(3 * s)
        for bad in (-1.0, float("nan"), float("inf"), 1e30):
            assert L.oa_set_neighbor_radius(h, C.c_float(bad)) == _capi.OA_E_BAD_ARG, bad
            assert e.neighbor_radius == float(np.float32(3 * s))
        assert L.oa_get_neighbor_radius(h, None) == _capi.OA_E_BAD_ARG
        got = e.target_knn(K)
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
        assert e.target_spacing() == want_sp
    # a multi-device context on one physical device hands the setting to its children
    with _engine(pts) as f:
        want_n = f.estimate_target_normals(k=K, install=False, radius=3 * s)
    with _engine(pts, devices=[0, 0]) as m:
        m.set_neighbor_radius(3 * s)
        assert m.neighbor_radius == float(np.float32(3 * s))
        got = m.target_knn(K)
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
        n, curv = m.estimate_target_normals(k=K, install=False)
        assert np.array_equal(bits(n), bits(want_n[0])) and np.array_equal(bits(curv), bits(want_n[1]))
        with pytest.raises(_capi.OaError) as err:
            m.target_spacing()
        assert err.value.code == _capi.OA_E_STATE
        m.set_neighbor_radius(0)
        assert (m.target_knn(K)[0] >= 0).all()
