"""Outlier removal for raw clouds: oa_target_radius_count, oa_target_outliers, IcpEngine.target_outliers /
target_radius_count, object_alignment_amd.remove_outliers and IcpSettings.clean_target / clean_source.

The numpy restatement lives here: fixed-radius counts by fp64 brute force against the float32 square of the float32 radius, the
statistical score from rows of k + 1 squared distances (a loop over the entries in list order, np.sqrt on float64, one division),
two-pass mean and standard deviation.  Every test fails on a tree without the feature: the symbols and methods are not there.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 1e-6            # relative distance of an fp64 squared distance from r^2 below which float32 may decide the other way


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build_hip()
    return g


# ------------------------------------------------------------------------------------------------ the clouds
def torus(n, R=1.0, r=0.35, seed=1):
    """(points float32, analytic outward normals fp64): n random points of a torus"""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    x = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], 1)
    return x.astype(np.float32), np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)


def strays(m):
    return np.random.default_rng(7).uniform([-2, -2, -0.6], [2, 2, 0.6], (m, 3)).astype(np.float32)


def torus_distance(x, R=1.0, r=0.35):
    x = np.asarray(x, np.float64)
    return np.abs(np.sqrt((np.sqrt(x[:, 0] ** 2 + x[:, 1] ** 2) - R) ** 2 + x[:, 2] ** 2) - r)


@functools.lru_cache(maxsize=None)
def fixture():
    """(xyz, is_surface, is_far_stray): torus(6000, seed=1) + strays(300), shuffled"""
    pts = np.concatenate([torus(6000, seed=1)[0], strays(300)])
    perm = np.random.default_rng(0).permutation(len(pts))
    xyz = np.ascontiguousarray(pts[perm])
    surface = perm < 6000
    return xyz, surface, ~surface & (torus_distance(xyz) > 0.1)


def lattice(nx, ny, nz, seed=3):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).reshape(-1, 3)
    return g[np.random.default_rng(seed).permutation(len(g))].astype(np.float32)


@functools.lru_cache(maxsize=None)
def lattice_case(name):
    if name == "210":
        return lattice(7, 6, 5)
    if name == "5":
        return lattice(7, 6, 5)[:5].copy()
    n = int(name)                                                  # 64, 65, 4097: one, two and three box levels
    pts = lattice(8, 8, 64)
    return np.concatenate([pts[: n - 1], np.array([[1000.0, -500.0, 250.0]], np.float32)]) if n != 64 else pts[:64].copy()


# ------------------------------------------------------------------------------------------------ numpy restatements
def r2_of(radius):
    """(float)radius * (float)radius, float32 with one rounding, as a float64"""
    rf = np.float32(radius)
    return float(np.float32(rf * rf))


def pair_d2(xyz):
    """blocks of the fp64 squared distance matrix: (first row, block); a non-finite coordinate makes its row and column NaN / inf"""
    x = np.asarray(xyz, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(0, len(x), 512):
            yield b, ((x[b:b + 512, None, :] - x[None, :, :]) ** 2).sum(axis=2)


def radius_count_ref(xyz, radius, cap=0):
    """(count int32, near: some squared distance lies within GAP relative of r^2)"""
    r2 = r2_of(radius)
    count, near = np.empty(len(xyz), np.int64), np.empty(len(xyz), bool)
    for b, d in pair_d2(xyz):
        with np.errstate(invalid="ignore"):
            count[b:b + len(d)] = (d <= r2).sum(axis=1)
            near[b:b + len(d)] = (np.abs(d - r2) <= GAP * r2).any(axis=1)
    if cap > 0:
        count = np.minimum(count, cap)
    return count.astype(np.int32), near


@functools.lru_cache(maxsize=None)
def fixture_counts(radius):
    return radius_count_ref(fixture()[0], radius)


def knn_d2_exact(xyz, k):
    """the k + 1 smallest fp64 squared distances of every vertex (itself included), ascending"""
    out = np.empty((len(xyz), k + 1), np.float64)
    for b, d in pair_d2(xyz):
        out[b:b + len(d)] = np.sort(d, axis=1)[:, : k + 1]
    return out


def score_ref(d2_rows):
    """The statistical score from rows of k + 1 squared distances (unfilled entries +inf): S summed in list order over the m filled
    entries, np.sqrt on float64, one division by m - 1; +inf for m < 2."""
    d2 = np.asarray(d2_rows)
    S, m = np.zeros(len(d2), np.float64), np.zeros(len(d2), np.int64)
    for j in range(d2.shape[1]):
        filled = np.isfinite(d2[:, j])
        S = np.where(filled, S + np.sqrt(np.where(filled, d2[:, j], 0).astype(np.float64)), S)
        m += filled
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(m >= 2, S / np.maximum(m - 1, 1).astype(np.float64), np.inf)


def stats_ref(score, std_ratio):
    """(mean, std, threshold) of the finite scores, two passes"""
    s = score[np.isfinite(score)]
    n = len(s)
    mean = float(s.sum() / n) if n else 0.0
    std = float(np.sqrt(((s - mean) ** 2).sum() / (n - 1))) if n >= 2 else 0.0
    return mean, std, mean + std_ratio * std


@functools.lru_cache(maxsize=None)
def fixture_statistical(k, std_ratio):
    score = score_ref(knn_d2_exact(fixture()[0], k))
    return score, score <= stats_ref(score, std_ratio)[2]


def _engine(xyz, **kw):
    from object_alignment_amd.engine import IcpEngine
    e = IcpEngine(0, **kw)
    e.set_target(xyz)
    return e


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


# ------------------------------------------------------------------------------------------------ CPU
def test_outlier_abi_and_bindings(built):
    """The header, both library flavours and the bindings name the two calls; the structs have the header's fields and sizes."""
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    hdr = open(os.path.join(ROOT, "include", "oa_icp.h")).read()
    for fn in ("oa_target_outliers", "oa_target_radius_count"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, hdr), fn
        assert fn in _capi.SYMBOLS
        for lib in ("liboa_icp.so", "liboa_icp_exp.so"):
            assert hasattr(C.CDLL(os.path.join(ROOT, "object_alignment_amd", lib)), fn), (lib, fn)
    for name, val in (("OA_OUTLIER_STATISTICAL", 0), ("OA_OUTLIER_RADIUS", 1), ("OA_STAT_TARGET_CLEANED", 51)):
        m = re.search(r"#define\s+%s\s+(\d+)\b" % name, hdr)
        assert m and int(m.group(1)) == val == getattr(_capi, name), name
    assert IcpEngine.STATS["target_cleaned"] == 51
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    for struct, cls, size in (("oa_outlier_settings", _capi.OutlierSettings, 32), ("oa_outlier_report", _capi.OutlierReport, 48)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [(n.strip(), ctype[t]) for t, names in re.findall(r"(int32_t|int64_t|double)\s+([^;]+);", body) for n in names.split(",")]
        assert fields == list(cls._fields_), struct
        assert C.sizeof(cls) == size, struct


def test_outlier_argument_errors_touch_no_device():
    """Every range of the settings is refused in Python: by the engine's methods before the library is called, by remove_outliers
    before a context opens, by OutlierSettings when it is made, and by IcpAlign.run(clean_target, target_tris) before an engine
    is touched."""
    import object_alignment_amd as oa
    from object_alignment_amd.engine import IcpEngine, _outlier_args
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings, OutlierSettings

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("touched (%s)" % name)

    eng = object.__new__(IcpEngine)
    eng._L, eng._h, eng.n_target = Untouchable(), None, 40
    bad = [dict(method="bogus"), dict(method=2), dict(method=True), dict(k=0), dict(k=64), dict(k=40), dict(k=2.5), dict(k=True),
           dict(std_ratio=-0.1), dict(std_ratio=float("inf")), dict(std_ratio=float("nan")), dict(std_ratio="2"),
           dict(method="radius"), dict(method="radius", radius=-1.0), dict(method="radius", radius=float("inf")),
           dict(method="radius", radius=float("nan")), dict(method="radius", radius="1"), dict(method="radius", radius=0.1, min_neighbors=0),
           dict(method="radius", radius=0.1, min_neighbors=1.5), dict(method="radius", radius=0.1, min_neighbors=8, count_cap=8),
           dict(method="radius", radius=0.1, min_neighbors=8, count_cap=-1)]
    pts = np.zeros((40, 3), np.float32)
    for kw in bad:
        with pytest.raises(ValueError):
            eng.target_outliers(**kw)
        with pytest.raises(ValueError):
            oa.remove_outliers(pts, **kw)
        if kw != dict(k=40):                                       # (k against the cloud's size is known at the call only)
            with pytest.raises(ValueError):
                OutlierSettings(**kw)
    assert OutlierSettings(k=40).k == 40
    for kw in (dict(radius=0.0), dict(radius=float("inf")), dict(radius="1"), dict(radius=0.1, cap=-1), dict(radius=0.1, cap=1.5)):
        with pytest.raises(ValueError):
            eng.target_radius_count(**kw)
    with pytest.raises(ValueError):
        oa.remove_outliers(np.zeros((5, 2), np.float32))
    assert _outlier_args("radius", radius=0.5, min_neighbors=8, count_cap=9) == (1, 1, 0.0, 0.5, 8, 9)
    assert _outlier_args("statistical", k=63, std_ratio=0, n=64) == (0, 63, 0.0, 0.0, 1, 0)
    eye = np.eye(4, dtype=np.float32)
    for engine in (Untouchable(), None):                           # None: no engine may be created either
        op = IcpAlign(IcpSettings(clean_target=OutlierSettings()), engine=engine)
        with pytest.raises(ValueError):
            op.run(pts, pts, eye, eye, target_tris=np.array([[0, 1, 2]], np.int32))
        assert op._engine is engine
        with pytest.raises(TypeError):
            IcpAlign(IcpSettings(clean_source="statistical"), engine=engine).run(pts, pts, eye, eye)
    assert IcpSettings().clean_target is None and IcpSettings().clean_source is None


def test_fixture_guard_statistical():
    """The restatement on brute-force rows: k = 16, ratio 1.0 keeps the surface and removes the far strays."""
    _, surface, far = fixture()
    _, keep = fixture_statistical(16, 1.0)
    kept, removed = float(keep[surface].mean()), float((~keep[far]).mean())
    print("statistical k=16 ratio 1.0: surface kept %.4f, far strays removed %.4f (%d far of 300)" % (kept, removed, far.sum()))
    assert kept >= 0.995 and removed >= 0.90


def test_fixture_guard_radius():
    """Radius 0.12 / 8 neighbours on the restatement, and the gap condition the GPU comparison relies on: the share of vertices
    with an fp64 squared distance within a relative 1e-6 of r^2 is at most 0.1 % at every radius the GPU tests use."""
    _, surface, far = fixture()
    count, _ = fixture_counts(0.12)
    keep = count - 1 >= 8
    kept, removed = float(keep[surface].mean()), float((~keep[far]).mean())
    print("radius 0.12 / 8: surface kept %.4f, far strays removed %.4f" % (kept, removed))
    assert kept >= 0.99 and removed >= 0.99
    for radius in (0.08, 0.1, 0.12):
        share = float(fixture_counts(radius)[1].mean())
        print("radius %.2f: share of vertices with a pair within 1e-6 of r^2: %.5f" % (radius, share))
        assert share <= 0.001


# ------------------------------------------------------------------------------------------------ GPU
LATTICE_RADII = (1.0, float(np.float32(np.sqrt(2.0))), 2.0, 3.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["210", "5", "64", "65", "4097"])
def test_gpu_radius_count_under_ties(built, name):
    """Integer lattices: every float32 operation of the metric is exact and d2 = r^2 is everywhere (sqrt(2) as a float32 squares to
    just above 2) -- the counts are numpy's, uncapped and capped at 1, 7 and 64."""
    pts = lattice_case(name)
    with _engine(pts) as e:
        for radius in LATTICE_RADII:
            ref, _ = radius_count_ref(pts, radius)
            assert ref.min() >= 1
            for cap in (0, 1, 7, 64):
                got = e.target_radius_count(radius, cap)
                assert got.dtype == np.int32 and got.shape == (len(pts),)
                assert np.array_equal(got, np.minimum(ref, cap) if cap else ref), (name, radius, cap)


@pytest.mark.gpu
def test_gpu_radius_count_of_duplicates(built):
    pts = np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (200, 1))
    with _engine(pts) as e:
        assert np.array_equal(e.target_radius_count(0.5), np.full(200, 200, np.int32))
        assert np.array_equal(e.target_radius_count(1e-30), np.full(200, 200, np.int32))


@pytest.mark.gpu
def test_gpu_radius_count_on_the_fixture(built):
    """Exact against fp64 brute force on every vertex the gap condition admits; at most 0.1 % are left out (the CPU guard: none)."""
    xyz = fixture()[0]
    with _engine(xyz) as e:
        for radius in (0.08, 0.12):
            ref, near = fixture_counts(radius)
            assert float(near.mean()) <= 0.001
            for cap in (0, 9):
                got = e.target_radius_count(radius, cap)
                want = np.minimum(ref, cap) if cap else ref
                assert np.array_equal(got[~near], want[~near]), (radius, cap)
                again = e.target_radius_count(radius, cap)
                assert np.array_equal(got, again)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["fixture", "4097"])
def test_gpu_scores_are_the_restatement_bit_for_bit(built, which):
    """From the library's own target_knn(k + 1) rows: score bitwise, mean / std / threshold to 1e-12 relative, and keep, index and
    the report's counts exactly what they say."""
    xyz = fixture()[0] if which == "fixture" else lattice_case("4097")
    with _engine(xyz) as e:
        for k in (1, 16, 63):
            _, d2 = e.target_knn(k + 1)
            ref = score_ref(d2)
            out = e.target_outliers(method="statistical", k=k, std_ratio=1.0)
            rep = out["report"]
            assert out["score"].dtype == np.float64 and np.array_equal(bits(out["score"]), bits(ref)), (which, k)
            mean, std, thr = stats_ref(ref, 1.0)
            print("%s k=%d: mean %.17g (numpy %.17g), std %.17g (%.17g), threshold %.17g (%.17g)"
                  % (which, k, rep["mean"], mean, rep["std"], std, rep["threshold"], thr))
            assert abs(rep["mean"] - mean) <= 1e-12 * abs(mean)
            assert abs(rep["std"] - std) <= 1e-12 * abs(std)
            assert abs(rep["threshold"] - thr) <= 1e-12 * abs(thr)
            assert np.array_equal(out["keep"], (out["score"] <= rep["threshold"]).astype(np.uint8))
            assert out["index"].dtype == np.int32 and np.array_equal(out["index"], np.flatnonzero(out["keep"]))
            assert rep["n_kept"] == len(out["index"]) and rep["n_kept"] + rep["n_removed"] == len(xyz) and rep["n_nonfinite"] == 0


@pytest.mark.gpu
def test_gpu_outliers_with_non_finite_vertices(built):
    """Three NaN / inf vertices among 500: count 0, score +inf, not kept, reported, and in nobody's count."""
    xyz = torus(500, seed=3)[0].copy()
    bad = [7, 250, 499]
    xyz[7, 0], xyz[250, 1], xyz[499] = np.nan, np.inf, (-np.inf, np.nan, 1.0)
    good = np.setdiff1d(np.arange(500), bad)
    with _engine(xyz) as e:
        count = e.target_radius_count(0.3)
        ref, near = radius_count_ref(xyz[good], 0.3)
        assert not near.any()
        assert np.array_equal(count[bad], [0, 0, 0]) and np.array_equal(count[good], ref)
        rad = e.target_outliers(method="radius", radius=0.3, min_neighbors=1)
        assert np.array_equal(rad["count"], count) and not rad["keep"][bad].any() and rad["report"]["n_nonfinite"] == 3
        out = e.target_outliers(method="statistical", k=8, std_ratio=3.0)
        assert np.all(np.isposinf(out["score"][bad])) and np.isfinite(out["score"][good]).all()
        assert not out["keep"][bad].any() and out["report"]["n_nonfinite"] == 3
        _, d2 = e.target_knn(9)
        assert np.array_equal(bits(out["score"]), bits(score_ref(d2)))
        mean, std, _ = stats_ref(out["score"], 3.0)
        assert abs(out["report"]["mean"] - mean) <= 1e-12 * mean and abs(out["report"]["std"] - std) <= 1e-12 * std


@pytest.mark.gpu
def test_gpu_outliers_on_two_points_and_on_identical_points(built):
    two = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]], np.float32)
    with _engine(two) as e:
        out = e.target_outliers(method="statistical", k=1, std_ratio=0.0)
        assert np.array_equal(out["score"], [5.0, 5.0]) and out["report"]["std"] == 0.0 and out["report"]["threshold"] == 5.0
        assert np.array_equal(out["keep"], [1, 1]) and np.array_equal(e.target_radius_count(5.0), [2, 2])
        assert np.array_equal(e.target_radius_count(4.999), [1, 1])
    same = np.tile(np.array([[1.0, 2.0, 3.0]], np.float32), (300, 1))
    with _engine(same) as e:
        out = e.target_outliers(method="statistical", k=16, std_ratio=0.0)
        assert not out["score"].any() and out["report"]["std"] == 0.0 and out["keep"].all() and out["report"]["n_kept"] == 300


@pytest.mark.gpu
def test_gpu_outliers_without_a_resident_tree(built):
    """OA_SEARCH_BRUTE skips the tree with the upload: the calls build one of their own and return the same bits."""
    from object_alignment_amd.engine import IcpEngine
    xyz = fixture()[0]
    with _engine(xyz) as e:
        count, out = e.target_radius_count(0.12), e.target_outliers(method="statistical", k=16, std_ratio=1.0)
    with IcpEngine(0) as b:
        b.set_search_mode("brute")
        b.set_target(xyz)
        assert np.array_equal(b.target_radius_count(0.12), count)
        bout = b.target_outliers(method="statistical", k=16, std_ratio=1.0)
    assert np.array_equal(bits(bout["score"]), bits(out["score"])) and np.array_equal(bout["keep"], out["keep"])
    assert bout["report"] == out["report"]


@pytest.mark.gpu
def test_gpu_outlier_refusals_leave_the_context_usable(built):
    """OA_E_STATE without a target, on a surface target and on a multi-device context; OA_E_BAD_ARG for every range, through the
    error text channel; the context runs a loop afterwards."""
    from object_alignment_amd import _capi, synth
    from object_alignment_amd.engine import IcpEngine
    L = _capi.load()
    x = torus(300, seed=4)[0]
    eye = np.identity(4, dtype=np.float32)

    def outliers(e, **kw):
        st = _capi.OutlierSettings(kw.get("method", 0), kw.get("k", 8), kw.get("std_ratio", 2.0), kw.get("radius", 0.1),
                                   kw.get("min_neighbors", 4), kw.get("count_cap", 0))
        rc = L.oa_target_outliers(e._h, C.byref(st), kw.get("apply", 0), None, None, None, None, None)
        return rc, L.oa_last_error().decode()

    def count(e, radius=0.1, cap=0):
        rc = L.oa_target_radius_count(e._h, radius, cap, None)
        return rc, L.oa_last_error().decode()

    with IcpEngine(0) as e:
        for rc, msg in (outliers(e), count(e)):
            assert rc == _capi.OA_E_STATE and "oa_set_target" in msg            # no target
        e.set_target(x)
        for kw in (dict(method=2), dict(method=-1), dict(k=0), dict(k=64), dict(k=300), dict(std_ratio=-1.0), dict(std_ratio=float("nan")),
                   dict(std_ratio=float("inf")), dict(method=1, radius=0.0), dict(method=1, radius=float("inf")),
                   dict(method=1, radius=float("nan")), dict(method=1, min_neighbors=0), dict(method=1, min_neighbors=4, count_cap=4),
                   dict(method=1, count_cap=-1)):
            rc, msg = outliers(e, **kw)
            assert rc == _capi.OA_E_BAD_ARG and "oa_target_outliers" in msg, (kw, rc, msg)
        for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(cap=-1)):
            rc, msg = count(e, **kw)
            assert rc == _capi.OA_E_BAD_ARG and "oa_target_radius_count" in msg, (kw, rc, msg)
        assert L.oa_target_outliers(e._h, None, 0, None, None, None, None, None) == _capi.OA_E_BAD_ARG
        assert outliers(e, k=63)[0] == _capi.OA_OK and outliers(e, method=1, count_cap=5)[0] == _capi.OA_OK and count(e)[0] == _capi.OA_OK
        verts, tris = synth.icosphere_mesh(1)
        e.set_target_mesh(verts, tris)
        for rc, msg in (outliers(e), count(e)):
            assert rc == _capi.OA_E_STATE and "surface" in msg
        e.set_target(x)
        e.set_source(x, stride=1)
        e.set_matrices(eye, eye)
        assert e.run(iters=3).iters_done >= 1
    with IcpEngine(devices=[0, 0]) as m:
        m.set_target(x)
        for rc, msg in (outliers(m), count(m)):
            assert rc == _capi.OA_E_STATE and "multi-device" in msg
        m.set_source(x, stride=1)                                                # ... and it goes on working
        m.set_matrices(eye, eye)
        assert m.nn_search()[0].shape == (300,) and m.run(iters=3).iters_done >= 1


def _pose():
    from object_alignment_amd import synth
    P = synth.rigid4(synth.rotation_from_rotvec([0.05, -0.04, 0.06]), [0.03, -0.02, 0.01], dtype=np.float64)
    return np.linalg.inv(P).astype(np.float32), np.eye(4, dtype=np.float32)


@pytest.mark.gpu
def test_gpu_apply_is_a_plain_upload_of_the_kept_points(built):
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    xyz = fixture()[0]
    src = torus(1500, seed=5)[0]
    mxa, mxb = _pose()
    with _engine(xyz) as e, IcpEngine(0) as f:
        e.estimate_target_normals(k=8, install=True)                # (what an apply has to forget)
        out = e.target_outliers(method="statistical", k=16, std_ratio=1.0, apply=True)
        keep = out["keep"].astype(bool)
        assert 0 < out["report"]["n_removed"] < len(xyz) and e.n_target == out["report"]["n_kept"] == int(keep.sum())
        assert e.stat("target_cleaned") == out["report"]["n_removed"] and e.stat("target_normals") == 0
        f.set_target(xyz[keep])
        assert f.stat("target_cleaned") == 0
        results = []
        for g in (e, f):
            g.set_source(src, stride=1)
            g.set_matrices(mxa, mxb)
            idx, d2, _ = g.nn_search()
            kidx, kd2 = g.target_knn(8)
            res = g.run(iters=10, thresh=0.5, target_d=1e-9)
            results.append((idx, bits(d2), kidx, bits(kd2), bits(res.matrix_world), bits(res.step_new), res.iters_done))
        for a, b in zip(*results):
            assert np.array_equal(a, b)
        assert results[0][-1] >= 2
        # nothing kept: refused, nothing applied, the old target still answers
        with pytest.raises(_capi.OaError) as err:
            e.target_outliers(method="radius", radius=0.05, min_neighbors=100000, apply=True)
        assert err.value.code == _capi.OA_E_TOO_FEW_PAIRS and "oa_target_outliers" in str(err.value)
        assert e.n_target == int(keep.sum()) and e.stat("target_cleaned") == out["report"]["n_removed"]
        assert np.array_equal(e.nn_search()[0], f.nn_search()[0])          # (both stand at the pose their loops ended on)
        e.set_target(xyz)
        assert e.stat("target_cleaned") == 0 and e.n_target == len(xyz)


RADIUS_CLEAN = dict(method="radius", radius=0.12, min_neighbors=8)


def _recording_engine():
    from object_alignment_amd.engine import IcpEngine

    class Recording(IcpEngine):
        def estimate_target_normals(self, *a, **kw):
            self.estimated = super().estimate_target_normals(*a, **kw)
            return self.estimated

        def set_source(self, xyz, vlist=None, **kw):
            self.vlist_seen = None if vlist is None else np.array(vlist)
            return super().set_source(xyz, vlist=vlist, **kw)

    return Recording(0)


@pytest.mark.gpu
def test_gpu_clean_target_through_the_operator(built):
    """IcpAlign.run with clean_target is a run on the pre-cleaned cloud, bit for bit; the index map is the restatement's; an
    estimate sees the cleaned cloud; a deviation report speaks of the caller's vertices."""
    import object_alignment_amd as oa
    from object_alignment_amd.operators.icp_align import DeviationSettings, IcpAlign, IcpSettings, OutlierSettings
    xyz = fixture()[0]
    src = torus(1500, seed=5)[0]
    mxa, mxb = _pose()
    count, near = fixture_counts(0.12)
    assert not near.any()
    index = np.flatnonzero(count - 1 >= 8)
    common = dict(icp_iterations=10, target_d=1e-9)
    with _recording_engine() as e:
        op = IcpAlign(IcpSettings(clean_target=OutlierSettings(**RADIUS_CLEAN), **common), engine=e)
        res = op.run(src, xyz, mxa, mxb, deviation=DeviationSettings())
        assert np.array_equal(op.last_cleaning["target"]["index"], index) and op.last_cleaning["source"] is None
        assert op.last_cleaning["target"]["report"]["n_removed"] == len(xyz) - len(index)
        plain = IcpAlign(IcpSettings(**common), engine=e)
        ref = plain.run(src, xyz[index], mxa, mxb, deviation=DeviationSettings())
        assert plain.last_cleaning is None
        assert np.array_equal(bits(res.matrix_world), bits(ref.matrix_world)) and np.array_equal(bits(res.step_new), bits(ref.step_new))
        assert np.array_equal(res.deviation["idx"], np.where(ref.deviation["idx"] >= 0, index[np.maximum(ref.deviation["idx"], 0)], -1))
        # a world twice as large: the radius is a world length, the cloud's own unit is half of one
        shrink = np.diag([0.5, 0.5, 0.5, 1.0]).astype(np.float32)
        op.run(src, xyz, shrink @ mxa, shrink @ mxb)
        half, near = radius_count_ref(xyz, 0.24)
        assert float(near.mean()) <= 0.001
        assert np.array_equal(op.last_cleaning["target"]["keep"][~near], (half - 1 >= 8)[~near].astype(np.uint8))
        # the estimate sees the cleaned cloud, the plane metric runs on it
        op = IcpAlign(IcpSettings(clean_target=OutlierSettings(**RADIUS_CLEAN), metric="plane", **common), engine=e)
        got = op.run(src, xyz, mxa, mxb, target_normals="estimate")
        want_n, want_c = oa.estimate_normals(xyz[index], k=16, orient="away")
        assert np.array_equal(bits(e.estimated[0]), bits(want_n)) and np.array_equal(bits(e.estimated[1]), bits(want_c))
        # given normals are gathered through the index map
        full_n = np.zeros((len(xyz), 3), np.float32)
        full_n[index] = want_n
        given = op.run(src, xyz, mxa, mxb, target_normals=full_n)
        assert np.array_equal(bits(given.matrix_world), bits(got.matrix_world))


@pytest.mark.gpu
def test_gpu_clean_source_through_the_operator(built):
    """The selection loses its stray points first: set_source sees vlist[keep of the selected]; with both settings off nothing is
    recorded and two runs give the same pose."""
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings, OutlierSettings
    xyz = fixture()[0]
    tgt = torus(4000, seed=9)[0]
    mxa, mxb = _pose()
    vlist = np.arange(0, len(xyz), 2, dtype=np.int64)[::-1].copy()          # (not ascending: the order is the caller's)
    count, near = radius_count_ref(xyz[vlist], 0.15)
    assert not near.any()
    keep = count - 1 >= 6
    with _recording_engine() as e:
        op = IcpAlign(IcpSettings(clean_source=OutlierSettings(method="radius", radius=0.15, min_neighbors=6), sample_fraction=1.0,
                                  icp_iterations=5), engine=e)
        op.run(xyz, tgt, mxa, mxb, vlist=vlist)
        assert np.array_equal(e.vlist_seen, vlist[keep]) and op.last_cleaning["target"] is None
        assert np.array_equal(op.last_cleaning["source"]["keep"], keep.astype(np.uint8))
        op.run(xyz, tgt, mxa, mxb)                                           # no vlist: the whole cloud is the selection
        whole, _ = radius_count_ref(xyz, 0.15)
        assert np.array_equal(e.vlist_seen, np.flatnonzero(whole - 1 >= 6))
        # both settings off: the run of tests/test_target_normals.py's capability test, twice
        from test_target_normals import capability_case
        s, t, a, b = capability_case()
        off = IcpAlign(IcpSettings(icp_iterations=50, target_d=1e-4, sample_fraction=1.0), engine=e)
        first = off.run(s, t, a, b)
        assert off.last_cleaning is None and e.vlist_seen is None
        second = off.run(s, t, a, b)
        assert np.array_equal(bits(first.matrix_world), bits(second.matrix_world)) and first.iters_done == second.iters_done


@pytest.mark.gpu
def test_gpu_remove_outliers_module_level(built):
    import object_alignment_amd as oa
    xyz = fixture()[0]
    _, ref_keep = fixture_statistical(16, 1.0)
    out = oa.remove_outliers(xyz, method="statistical", k=16, std_ratio=1.0)
    assert np.array_equal(out["xyz"], xyz[out["index"]]) and out["xyz"].dtype == np.float32
    assert np.array_equal(out["index"], np.flatnonzero(out["keep"]))
    again = oa.remove_outliers(xyz, method="statistical", k=16, std_ratio=1.0)
    assert np.array_equal(bits(out["score"]), bits(again["score"])) and np.array_equal(out["index"], again["index"])
    assert out["report"] == again["report"]
    # float32 rows against the fp64 restatement: the capability, not the bits
    _, surface, far = fixture()
    keep = out["keep"].astype(bool)
    assert float(np.mean(keep == ref_keep)) >= 0.999
    assert float(keep[surface].mean()) >= 0.995 and float((~keep[far]).mean()) >= 0.90
    rad = oa.remove_outliers(xyz, **RADIUS_CLEAN)
    assert np.array_equal(rad["index"], np.flatnonzero(fixture_counts(0.12)[0] - 1 >= 8)) and "count" in rad and "score" not in rad
