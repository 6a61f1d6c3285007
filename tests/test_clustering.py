"""Clustering of raw clouds: oa_target_clusters, IcpEngine.target_clusters, object_alignment_amd.cluster_dbscan and
IcpSettings.segment_target / segment_source.

The numpy restatement lives here: fp64 squared distances against the float32 square of the float32 eps, core vertices by count,
scipy's connected_components on the core graph, clusters numbered by their lowest core index, a border vertex to the lowest label
among its core neighbours.  It is itself checked against scikit-learn's brute-force DBSCAN, on the CPU.  The GPU results are
integers and are compared for equality.  Every test fails on a tree without the feature: the symbols and methods are not there.
"""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 1e-6            # relative distance of an fp64 squared distance from r^2 below which float32 may decide the other way
KEEP_MODES = ("clustered", "largest", "min_size")
REPORT_FIELDS = ("n_clusters", "n_core", "n_border", "n_noise", "n_nonfinite", "largest_label", "largest_size", "n_kept", "n_removed")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build_hip()
    return g


# ------------------------------------------------------------------------------------------------ the clouds
def torus(n, R=1.0, r=0.35, seed=1):
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    return np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], 1).astype(np.float32)


def strays(m):
    return np.random.default_rng(7).uniform([-2, -2, -0.6], [2, 2, 0.6], (m, 3)).astype(np.float32)


def table(m=600):
    """a flat patch 0.8 x 0.8 at z = -0.9"""
    xy = np.random.default_rng(11).uniform(-0.4, 0.4, (m, 2))
    return np.concatenate([xy, np.full((m, 1), -0.9)], 1).astype(np.float32)


def clamp(m=250):
    """a ball of radius 0.08 at (1.9, 0, 0.5)"""
    rng = np.random.default_rng(13)
    d = rng.normal(size=(m, 3))
    d *= (0.08 * rng.uniform(0, 1, m) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
    return (d + [1.9, 0.0, 0.5]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fixture():
    """(xyz, part): torus(6000, seed=1) + strays(300) + table(600) + clamp(250), shuffled; part 0 torus, 1 stray, 2 table, 3 clamp"""
    pts = np.concatenate([torus(6000, seed=1), strays(300), table(), clamp()])
    part = np.repeat(np.arange(4), [6000, 300, 600, 250])
    perm = np.random.default_rng(0).permutation(len(pts))
    return np.ascontiguousarray(pts[perm]), part[perm]


@functools.lru_cache(maxsize=None)
def lattice_case(n):
    """n - 1 random points of the 8 x 8 x 64 integer lattice and one point far away"""
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(64), indexing="ij"), axis=-1).reshape(-1, 3)
    g = g[np.random.default_rng(3).permutation(len(g))].astype(np.float32)
    return np.concatenate([g[: n - 1], np.array([[1000.0, -500.0, 250.0]], np.float32)])


def blocks_cloud(second_first):
    """Two 5 x 5 x 5 blocks two units apart with one point midway, and two more with a line of five points between them.  Returns
    (points, names): names[i] says what vertex i is.  second_first: the block at x = 6 .. 10 holds the lowest indices."""
    def block(x0):
        return np.stack(np.meshgrid(np.arange(x0, x0 + 5), np.arange(5), np.arange(5), indexing="ij"), axis=-1).reshape(-1, 3)
    a, b, c, d = block(0), block(6), block(20), block(30)
    mid = np.array([[5, 2, 2]])
    line = np.array([[x, 2, 2] for x in range(25, 30)])
    parts = [("b", b), ("a", a)] if second_first else [("a", a), ("b", b)]
    parts += [("mid", mid), ("c", c), ("line", line), ("d", d)]
    pts = np.concatenate([p for _, p in parts]).astype(np.float32)
    names = np.concatenate([[name] * len(p) for name, p in parts])
    return pts, names


# ------------------------------------------------------------------------------------------------ the numpy restatement
def r2_of(eps):
    """(float)eps * (float)eps, float32 with one rounding, as a float64"""
    ef = np.float32(eps)
    return float(np.float32(ef * ef))


def neighbours(xyz, eps):
    """(A bool n x n: fp64 d2 <= r2, rows and columns of non-finite vertices empty; near: the number of pairs within GAP of r2)"""
    x = np.asarray(xyz, np.float64)
    r2 = r2_of(eps)
    A = np.zeros((len(x), len(x)), bool)
    near = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(0, len(x), 512):
            d = ((x[b:b + 512, None, :] - x[None, :, :]) ** 2).sum(axis=2)
            A[b:b + 512] = d <= r2
            near += int((np.abs(d - r2) <= GAP * r2).sum())
    return A, near


def dbscan_ref(xyz, eps, min_points, A=None):
    """label int32 (n,), sizes int32 (n_clusters,), core bool (n,) by the contract of oa_target_clusters"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    if A is None:
        A = neighbours(xyz, eps)[0]
    n = len(A)
    core = A.sum(axis=1) >= min_points
    label = np.full(n, -1, np.int64)
    ci = np.flatnonzero(core)
    if len(ci):
        _, comp = connected_components(csr_matrix(A[np.ix_(ci, ci)]), directed=False)
        _, first = np.unique(comp, return_index=True)               # each component's lowest core index (ci ascends)
        dense = np.empty(len(first), np.int64)
        dense[np.argsort(first)] = np.arange(len(first))             # numbered in ascending order of it
        label[ci] = dense[comp]
        for i in np.flatnonzero(~core):
            nb = A[i] & core
            if nb.any():
                label[i] = label[nb].min()
    n_clusters = int(label.max()) + 1 if len(ci) else 0
    sizes = np.bincount(label[label >= 0], minlength=n_clusters).astype(np.int32)
    return label.astype(np.int32), sizes, core


def keep_ref(label, sizes, keep, min_size=0):
    if keep == "clustered":
        return label >= 0
    if keep == "largest":
        return (label == int(np.argmax(sizes))) if len(sizes) else np.zeros(len(label), bool)      # (argmax: the first of equals)
    return (label >= 0) & (sizes[np.maximum(label, 0)] >= min_size) if len(sizes) else np.zeros(len(label), bool)


def report_ref(xyz, label, sizes, core, keep):
    n = len(label)
    return {"n_clusters": len(sizes), "n_core": int(core.sum()), "n_border": int(((label >= 0) & ~core).sum()), "n_noise": int((label < 0).sum()),
            "n_nonfinite": int((~np.isfinite(np.asarray(xyz, np.float64)).all(axis=1)).sum()),
            "largest_label": int(np.argmax(sizes)) if len(sizes) else -1, "largest_size": int(sizes.max()) if len(sizes) else 0,
            "n_kept": int(keep.sum()), "n_removed": n - int(keep.sum())}


def check(out, xyz, ref, keep, min_size=0):
    """every output of one call against the restatement: integers, no tolerance"""
    label, sizes, core = ref
    want = keep_ref(label, sizes, keep, min_size)
    assert out["label"].dtype == np.int32 and out["label"].shape == (len(xyz),) and np.array_equal(out["label"], label)
    assert out["sizes"].dtype == np.int32 and np.array_equal(out["sizes"], sizes)
    assert out["keep"].dtype == np.uint8 and np.array_equal(out["keep"], want.astype(np.uint8))
    assert out["index"].dtype == np.int32 and np.array_equal(out["index"], np.flatnonzero(want))
    assert out["report"] == report_ref(xyz, label, sizes, core, want) and tuple(out["report"]) == REPORT_FIELDS


@functools.lru_cache(maxsize=None)
def fixture_neighbours(eps):
    return neighbours(fixture()[0], eps)


@functools.lru_cache(maxsize=None)
def fixture_ref(eps=0.12, min_points=8):
    return dbscan_ref(None, eps, min_points, A=fixture_neighbours(eps)[0])


def _engine(xyz, **kw):
    from object_alignment_amd.engine import IcpEngine
    e = IcpEngine(0, **kw)
    e.set_target(xyz)
    return e


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


# ------------------------------------------------------------------------------------------------ CPU
def test_cluster_abi_and_bindings(built):
    """The header, both library flavours and the bindings name the call; the structs have the header's fields and sizes."""
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import CLUSTER_KEEP, IcpEngine
    hdr = open(os.path.join(ROOT, "include", "oa_icp.h")).read()
    assert re.search(r"\bint\s+oa_target_clusters\s*\(oa_ctx \*ctx, const oa_cluster_settings \*s, int apply,\s*int32_t \*label[^,]*,\s*int32_t \*sizes"
                     r"[^,]*,[^,]*,\s*uint8_t \*keep[^,]*,\s*int32_t \*kept_index[^,]*,[^,]*,\s*oa_cluster_report \*rep\);", hdr)
    assert "oa_target_clusters" in _capi.SYMBOLS
    for lib in ("liboa_icp.so", "liboa_icp_exp.so"):
        assert hasattr(C.CDLL(os.path.join(ROOT, "object_alignment_amd", lib)), "oa_target_clusters"), lib
    for name, val in (("OA_CLUSTER_KEEP_CLUSTERED", 0), ("OA_CLUSTER_KEEP_LARGEST", 1), ("OA_CLUSTER_KEEP_MIN_SIZE", 2)):
        m = re.search(r"#define\s+%s\s+(\d+)\b" % name, hdr)
        assert m and int(m.group(1)) == val == getattr(_capi, name), name
    assert CLUSTER_KEEP == {"clustered": 0, "largest": 1, "min_size": 2}
    assert re.search(r"#define OA_STAT_TARGET_CLEANED\s+51\s*/\*[^*]*oa_target_outliers\(apply\)[^*]*oa_target_clusters\(apply\)", hdr)
    assert callable(IcpEngine.target_clusters)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    for struct, cls, size in (("oa_cluster_settings", _capi.ClusterSettings, 24), ("oa_cluster_report", _capi.ClusterReport, 72)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [(n.strip(), ctype[t]) for t, names in re.findall(r"(int32_t|int64_t|double)\s+([^;]+);", body) for n in names.split(",")]
        assert fields == list(cls._fields_), struct
        assert C.sizeof(cls) == size, struct
    assert tuple(n for n, _ in _capi.ClusterReport._fields_) == REPORT_FIELDS


def test_cluster_argument_errors_touch_no_device():
    """Every range of the settings is refused in Python: by the engine's method before the library is called, by cluster_dbscan
    before a context opens, by ClusterSettings when it is made, and by IcpAlign.run(segment_target, target_tris) before an engine is
    touched."""
    import object_alignment_amd as oa
    from object_alignment_amd.engine import IcpEngine, _cluster_args
    from object_alignment_amd.operators.icp_align import ClusterSettings, IcpAlign, IcpSettings

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("touched (%s)" % name)

    eng = object.__new__(IcpEngine)
    eng._L, eng._h, eng.n_target = Untouchable(), None, 40
    bad = [dict(eps=0.0), dict(eps=-1.0), dict(eps=float("inf")), dict(eps=float("nan")), dict(eps="1"), dict(eps=True),
           dict(eps=0.1, min_points=0), dict(eps=0.1, min_points=1.5), dict(eps=0.1, min_points=True), dict(eps=0.1, keep="bogus"),
           dict(eps=0.1, keep=3), dict(eps=0.1, keep=True), dict(eps=0.1, keep=None), dict(eps=0.1, min_size=-1), dict(eps=0.1, min_size=2.5)]
    pts = np.zeros((40, 3), np.float32)
    for kw in bad:
        with pytest.raises(ValueError):
            eng.target_clusters(**kw)
        with pytest.raises(ValueError):
            oa.cluster_dbscan(pts, **kw)
        with pytest.raises(ValueError):
            ClusterSettings(**kw)
    with pytest.raises(TypeError):
        ClusterSettings()                                          # (eps has no default)
    with pytest.raises(ValueError):
        oa.cluster_dbscan(np.zeros((5, 2), np.float32), 0.1)
    assert _cluster_args(0.5) == (0.5, 8, 1, 0) and _cluster_args(2, 1, "min_size", 10) == (2.0, 1, 2, 10)
    assert _cluster_args(0.5, keep="clustered")[2] == 0 and _cluster_args(0.5, keep=np.int32(2))[2] == 2
    assert ClusterSettings(eps=0.5).kwargs(2.0) == dict(eps=0.25, min_points=8, keep="largest", min_size=0)
    eye = np.eye(4, dtype=np.float32)
    for engine in (Untouchable(), None):                           # None: no engine may be created either
        op = IcpAlign(IcpSettings(segment_target=ClusterSettings(eps=0.1)), engine=engine)
        with pytest.raises(ValueError):
            op.run(pts, pts, eye, eye, target_tris=np.array([[0, 1, 2]], np.int32))
        assert op._engine is engine
        with pytest.raises(TypeError):
            IcpAlign(IcpSettings(segment_source="largest"), engine=engine).run(pts, pts, eye, eye)
    assert IcpSettings().segment_target is None and IcpSettings().segment_source is None


def _sklearn_labels(xyz, eps, min_points):
    from sklearn.cluster import DBSCAN
    x = np.asarray(xyz, np.float64)
    # scikit-learn compares distances, not squares: hand it the squares as a precomputed "distance" and r2 as eps
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
    return DBSCAN(eps=r2_of(eps), min_samples=min_points, metric="precomputed", algorithm="brute").fit(d2).labels_


def test_restatement_is_scikit_learns_dbscan():
    """300 random integer-lattice clouds (n 5 .. 400, eps in {1, 1.5, 2, 2.25}, min_points 1 .. 8) and the fixture: the restatement's
    labels are scikit-learn's, numbering and border assignment included."""
    pytest.importorskip("sklearn")
    rng = np.random.default_rng(2024)
    for trial in range(300):
        n = int(rng.integers(5, 401))
        side = int(rng.integers(3, 12))
        pts = rng.integers(0, side, (n, 3)).astype(np.float32)      # (duplicates happen: they count)
        eps = float(rng.choice([1.0, 1.5, 2.0, 2.25]))
        mp = int(rng.integers(1, 9))
        label, sizes, core = dbscan_ref(pts, eps, mp)
        want = _sklearn_labels(pts, eps, mp)
        assert np.array_equal(label, want), (trial, n, side, eps, mp)
        assert np.array_equal(sizes, np.bincount(want[want >= 0], minlength=len(sizes)))
    from sklearn.cluster import DBSCAN
    xyz = fixture()[0]
    want = DBSCAN(eps=float(np.sqrt(r2_of(0.12))), min_samples=8, algorithm="brute").fit(xyz.astype(np.float64)).labels_
    assert fixture_neighbours(0.12)[1] == 0                         # (so a distance against sqrt(r2) decides as a square against r2)
    assert np.array_equal(fixture_ref()[0], want)


def test_fixture_guard():
    """The cloud of the issue: at eps 0.12 (and 0.11, 0.125) no fp64 squared distance lies within 1e-6 relative of r2; 0.12 / 8
    gives the torus with its 48 nearby strays, the table and the clamp, and 252 noise points; the largest cluster holds every
    torus point and no table or clamp point."""
    _, part = fixture()
    for eps in (0.11, 0.12, 0.125):
        assert fixture_neighbours(eps)[1] == 0, eps
    label, sizes, core = fixture_ref()
    print("sizes", sizes.tolist(), "noise", int((label < 0).sum()))
    assert sorted(sizes.tolist(), reverse=True) == [6048, 600, 250] and int((label < 0).sum()) == 252
    big = label == int(np.argmax(sizes))
    assert big[part == 0].all() and not big[part == 2].any() and not big[part == 3].any()
    for eps, torus_size in ((0.11, 6044), (0.125, 6050)):
        s = dbscan_ref(None, eps, 8, A=fixture_neighbours(eps)[0])[1]
        assert sorted(s.tolist(), reverse=True) == [torus_size, 600, 250], (eps, s.tolist())


def test_union_find_under_threads(tmp_path):
    """csrc/oa_unionfind.hpp on the host: tests/host/unionfind_check.cpp links random edge lists from 16 threads and compares roots
    and partition with a sequential union-find, built with -fsanitize=thread where the toolchain has that runtime (else plain).
    A stand-alone program: nothing is preloaded and nothing is loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    src = os.path.join(ROOT, "tests", "host", "unionfind_check.cpp")
    exe = str(tmp_path / "unionfind_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-pthread", "-I", os.path.join(ROOT, "object_alignment_amd", "csrc"), src, "-o", exe]
    tsan = subprocess.run(base + ["-fsanitize=thread"], capture_output=True, text=True)
    if tsan.returncode != 0:
        print("no -fsanitize=thread here (%s): built plain" % tsan.stderr.strip().splitlines()[-1:])
        subprocess.run(base, check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if run.returncode != 0 and "unexpected memory mapping" in run.stderr:
        # the sanitizer's runtime cannot lay out its shadow memory under this kernel's address randomisation: once more without
        # the randomisation, and if that is not to be had, the plain build
        print("ThreadSanitizer could not start (%s)" % run.stderr.strip().splitlines()[-1:])
        setarch = shutil.which("setarch")
        if setarch:
            run = subprocess.run([setarch, os.uname().machine, "-R", exe], capture_output=True, text=True, timeout=300)
        if run.returncode != 0 and ("unexpected memory mapping" in run.stderr or "setarch" in run.stderr):
            print("built plain")
            subprocess.run(base, check=True)
            run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0 and "ThreadSanitizer" not in run.stderr and "OK" in run.stdout


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 64, 65, 4097])
def test_gpu_clusters_on_lattices_under_ties(built, n):
    """Integer lattices: every float32 operation of the metric is exact and d2 = r2 is everywhere.  A partial leaf, then one, two
    and three box levels; min_points 1 is plain Euclidean clustering."""
    pts = lattice_case(n)
    with _engine(pts) as e:
        for eps in (1.0, 1.5):
            A = neighbours(pts, eps)[0]
            for mp in (1, 2, 4, 7):
                ref = dbscan_ref(pts, eps, mp, A=A)
                for keep in KEEP_MODES:
                    check(e.target_clusters(eps, min_points=mp, keep=keep, min_size=3), pts, ref, keep, 3)


@pytest.mark.gpu
def test_gpu_clusters_on_a_chain(built):
    """3 000 points in a row, eps = the spacing: deep parent chains and failed compare-and-swaps.  One cluster in every index order;
    with every 500th point gone six, the same six sets in every order."""
    full = np.zeros((3000, 3), np.float32)
    full[:, 0] = np.arange(3000)
    cut = full[(np.arange(3000) + 1) % 500 != 0]
    for pts, n_clusters in ((full, 1), (cut, 6)):
        n = len(pts)
        orders = [np.arange(n), np.arange(n)[::-1].copy(), np.random.default_rng(5).permutation(n)]
        by_position = []
        for order in orders:
            p = np.ascontiguousarray(pts[order])
            ref = dbscan_ref(p, 1.0, 2)
            assert len(ref[1]) == n_clusters
            with _engine(p) as e:
                out = e.target_clusters(1.0, min_points=2, keep="largest")
                check(out, p, ref, "largest")
                again = e.target_clusters(1.0, min_points=2, keep="largest")
            assert np.array_equal(out["label"], again["label"]) and np.array_equal(out["sizes"], again["sizes"])
            back = np.empty(n, np.int32)
            back[order] = out["label"]                               # the labels by position along the row
            by_position.append(back)
        for other in by_position[1:]:
            pairs = np.unique(np.stack([by_position[0], other], 1), axis=0)
            assert len(pairs) == n_clusters                          # a bijection between the labels: the same sets


@pytest.mark.gpu
@pytest.mark.parametrize("second_first", [False, True])
def test_gpu_bridge_and_border(built, second_first):
    """A point midway between two blocks counts 3 < min_points 4: it is a border vertex of both and takes the LOWER label, which is
    the second block's when that block holds the lower indices.  A line of such points between two other blocks does not merge
    them: its ends are border, its middle is noise."""
    pts, names = blocks_cloud(second_first)
    ref = dbscan_ref(pts, 1.0, 4)
    label, sizes, core = ref
    assert len(sizes) == 4 and not core[names == "mid"].any() and not core[names == "line"].any()
    first_block = "b" if second_first else "a"
    assert label[names == "mid"][0] == label[names == first_block][0] == 0
    assert label[names == "line"].tolist() == [label[names == "c"][0], -1, -1, -1, label[names == "d"][0]]
    assert label[names == "c"][0] != label[names == "d"][0]
    with _engine(pts) as e:
        for keep in KEEP_MODES:
            check(e.target_clusters(1.0, min_points=4, keep=keep, min_size=126), pts, ref, keep, 126)


@pytest.mark.gpu
def test_gpu_clusters_with_non_finite_vertices_and_duplicates(built):
    xyz = np.concatenate([torus(500, seed=3), torus(500, seed=3)[:40]])            # forty duplicates
    bad = [7, 250, 499]
    xyz[7, 0], xyz[250, 1], xyz[499] = np.nan, np.inf, (-np.inf, np.nan, 1.0)
    A, near = neighbours(xyz, 0.3)
    assert near == 0
    with _engine(xyz) as e:
        for mp in (1, 6):
            ref = dbscan_ref(xyz, 0.3, mp, A=A)
            out = e.target_clusters(0.3, min_points=mp, keep="clustered")
            check(out, xyz, ref, "clustered")
            assert np.array_equal(out["label"][bad], [-1, -1, -1]) and out["report"]["n_nonfinite"] == 3


@pytest.mark.gpu
def test_gpu_clusters_on_degenerate_clouds(built):
    from object_alignment_amd import _capi
    two = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]], np.float32)
    with _engine(two) as e:
        for eps, mp in ((5.0, 2), (4.999, 2), (4.999, 1), (5.0, 3)):
            check(e.target_clusters(eps, min_points=mp, keep="largest"), two, dbscan_ref(two, eps, mp), "largest")
    same = np.tile(np.array([[1.0, 2.0, 3.0]], np.float32), (300, 1))
    with _engine(same) as e:
        out = e.target_clusters(1e-30, min_points=300, keep="largest")
        check(out, same, dbscan_ref(same, 1e-30, 300), "largest")
        assert out["sizes"].tolist() == [300] and out["report"]["n_core"] == 300
        # a min_points nobody reaches: no cluster, nothing to keep -- refused with apply, and the context goes on
        none = e.target_clusters(1.0, min_points=301, keep="clustered")
        check(none, same, dbscan_ref(same, 1.0, 301), "clustered")
        assert none["report"]["n_clusters"] == 0 and none["report"]["largest_label"] == -1 and len(none["index"]) == 0
        with pytest.raises(_capi.OaError) as err:
            e.target_clusters(1.0, min_points=301, keep="clustered", apply=True)
        assert err.value.code == _capi.OA_E_TOO_FEW_PAIRS and "oa_target_clusters" in str(err.value)
        assert e.n_target == 300 and e.stat("target_cleaned") == 0
        assert e.target_clusters(1.0, min_points=300)["report"]["n_kept"] == 300


@pytest.mark.gpu
def test_gpu_clusters_on_the_fixture(built):
    """eps 0.12 / 8: all three keep modes, two calls give identical bytes, and a context without a resident tree the same."""
    from object_alignment_amd.engine import IcpEngine
    xyz, part = fixture()
    assert fixture_neighbours(0.12)[1] == 0
    ref = fixture_ref()
    outs = {}
    with _engine(xyz) as e:
        for keep in KEEP_MODES:
            outs[keep] = e.target_clusters(0.12, min_points=8, keep=keep, min_size=300)
            check(outs[keep], xyz, ref, keep, 300)
            again = e.target_clusters(0.12, min_points=8, keep=keep, min_size=300)
            for name in ("label", "sizes", "keep", "index"):
                assert outs[keep][name].tobytes() == again[name].tobytes(), (keep, name)
            assert outs[keep]["report"] == again["report"]
    big = outs["largest"]["keep"].astype(bool)
    assert big[part == 0].all() and not big[part >= 2].any() and outs["largest"]["report"]["largest_size"] == 6048
    assert outs["min_size"]["report"]["n_kept"] == 6648 and outs["clustered"]["report"]["n_noise"] == 252
    with IcpEngine(0) as b:
        b.set_search_mode("brute")                                   # (skips the tree with the upload: the call builds its own)
        b.set_target(xyz)
        bout = b.target_clusters(0.12, min_points=8, keep="largest")
    assert all(bout[name].tobytes() == outs["largest"][name].tobytes() for name in ("label", "sizes", "keep", "index"))
    assert bout["report"] == outs["largest"]["report"]


def _pose():
    from object_alignment_amd import synth
    P = synth.rigid4(synth.rotation_from_rotvec([0.05, -0.04, 0.06]), [0.03, -0.02, 0.01], dtype=np.float64)
    return np.linalg.inv(P).astype(np.float32), np.eye(4, dtype=np.float32)


@pytest.mark.gpu
def test_gpu_cluster_apply_is_a_plain_upload_of_the_kept_points(built):
    from object_alignment_amd.engine import IcpEngine
    xyz = fixture()[0]
    src = torus(1500, seed=5)
    mxa, mxb = _pose()
    with _engine(xyz) as e, IcpEngine(0) as f:
        e.estimate_target_normals(k=8, install=True)                # (what an apply has to forget)
        out = e.target_clusters(0.12, min_points=8, keep="largest", apply=True)
        check(out, xyz, fixture_ref(), "largest")
        keep = out["keep"].astype(bool)
        assert out["report"]["n_removed"] == 1102 and e.n_target == out["report"]["n_kept"] == 6048
        assert e.stat("target_cleaned") == 1102 and e.stat("target_normals") == 0
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
        e.set_target(xyz)
        assert e.stat("target_cleaned") == 0 and e.n_target == len(xyz)


def _recording_engine():
    from object_alignment_amd.engine import IcpEngine

    class Recording(IcpEngine):
        calls = ()

        def target_clusters(self, *a, **kw):
            self.calls = self.calls + ("target_clusters",)
            return super().target_clusters(*a, **kw)

        def target_outliers(self, *a, **kw):
            self.calls = self.calls + ("target_outliers",)
            return super().target_outliers(*a, **kw)

        def set_source(self, xyz, vlist=None, **kw):
            self.vlist_seen = None if vlist is None else np.array(vlist)
            return super().set_source(xyz, vlist=vlist, **kw)

    return Recording(0)


RADIUS_CLEAN = dict(method="radius", radius=0.12, min_neighbors=8)


@pytest.mark.gpu
def test_gpu_segment_target_through_the_operator(built):
    """IcpAlign.run with segment_target is a run on the largest cluster, bit for bit; after clean_target the kept indices are
    composed into the caller's numbering; eps is a world length; with both settings None nothing of this is called."""
    from object_alignment_amd.operators.icp_align import ClusterSettings, DeviationSettings, IcpAlign, IcpSettings, OutlierSettings
    xyz = fixture()[0]
    src = torus(1500, seed=5)
    mxa, mxb = _pose()
    label, sizes, _ = fixture_ref()
    index = np.flatnonzero(keep_ref(label, sizes, "largest"))
    common = dict(icp_iterations=10, target_d=1e-9)
    seg = ClusterSettings(eps=0.12, min_points=8)
    with _recording_engine() as e:
        plain = IcpAlign(IcpSettings(**common), engine=e)
        ref = plain.run(src, xyz[index], mxa, mxb, deviation=DeviationSettings())
        assert plain.last_segmentation is None and e.calls == ()    # None: nothing extra is launched
        op = IcpAlign(IcpSettings(segment_target=seg, **common), engine=e)
        res = op.run(src, xyz, mxa, mxb, deviation=DeviationSettings())
        got = op.last_segmentation
        assert e.calls == ("target_clusters",) and got["source"] is None and op.last_cleaning is None
        assert np.array_equal(got["target"]["index"], index) and np.array_equal(got["target"]["label"], label)
        assert got["target"]["report"]["n_kept"] == len(index) == 6048
        assert np.array_equal(bits(res.matrix_world), bits(ref.matrix_world)) and np.array_equal(bits(res.step_new), bits(ref.step_new))
        assert np.array_equal(res.deviation["idx"], np.where(ref.deviation["idx"] >= 0, index[np.maximum(ref.deviation["idx"], 0)], -1))
        # a world half as large: eps is a world length, 0.06 of it are 0.12 of the cloud's own unit (no squared distance lies
        # within 1e-6 of that r2 -- the guard above --, so the last bit of the scale does not matter)
        shrink = np.diag([0.5, 0.5, 0.5, 1.0]).astype(np.float32)
        half = IcpAlign(IcpSettings(segment_target=ClusterSettings(eps=0.06, min_points=8), **common), engine=e)
        half.run(src, xyz, shrink @ mxa, shrink @ mxb)
        assert np.array_equal(half.last_segmentation["target"]["label"], label)
        assert np.array_equal(half.last_segmentation["target"]["index"], index)
        e.calls = ()
        # after clean_target: the clustering sees the cleaned cloud, the indices speak of the caller's
        cleaned = np.flatnonzero(fixture_neighbours(0.12)[0].sum(axis=1) - 1 >= 8)
        sub = dbscan_ref(xyz[cleaned], 0.12, 8)
        composed = cleaned[keep_ref(sub[0], sub[1], "largest")]
        e.calls = ()
        both = IcpAlign(IcpSettings(clean_target=OutlierSettings(**RADIUS_CLEAN), segment_target=seg, **common), engine=e)
        res2 = both.run(src, xyz, mxa, mxb)
        assert e.calls == ("target_outliers", "target_clusters")
        assert np.array_equal(both.last_cleaning["target"]["index"], cleaned)
        assert np.array_equal(both.last_segmentation["target"]["index"], composed)
        assert np.array_equal(both.last_segmentation["target"]["label"], sub[0])
        ref2 = plain.run(src, xyz[composed], mxa, mxb)
        assert np.array_equal(bits(res2.matrix_world), bits(ref2.matrix_world))
        # given normals are gathered through the composed map
        full_n = np.zeros((len(xyz), 3), np.float32)
        full_n[composed] = xyz[composed] / np.linalg.norm(xyz[composed], axis=1, keepdims=True)
        planes = IcpAlign(IcpSettings(clean_target=OutlierSettings(**RADIUS_CLEAN), segment_target=seg, metric="plane", **common), engine=e)
        given = planes.run(src, xyz, mxa, mxb, target_normals=full_n)
        want = IcpAlign(IcpSettings(metric="plane", **common), engine=e).run(src, xyz[composed], mxa, mxb, target_normals=full_n[composed])
        assert np.array_equal(bits(given.matrix_world), bits(want.matrix_world))


@pytest.mark.gpu
def test_gpu_segment_source_through_the_operator(built):
    """The selection keeps its largest cluster: set_source sees vlist[kept]; after clean_source the kept positions are composed."""
    from object_alignment_amd.operators.icp_align import ClusterSettings, IcpAlign, IcpSettings, OutlierSettings
    xyz = fixture()[0]
    tgt = torus(4000, seed=9)
    mxa, mxb = _pose()
    vlist = np.arange(0, len(xyz), 2, dtype=np.int64)[::-1].copy()          # (not ascending: the order is the caller's)
    sel = xyz[vlist]
    A, near = neighbours(sel, 0.15)
    assert near == 0
    label, sizes, _ = dbscan_ref(sel, 0.15, 6, A=A)
    kept = np.flatnonzero(keep_ref(label, sizes, "largest"))
    assert 2500 < len(kept) < len(sel)
    seg = ClusterSettings(eps=0.15, min_points=6)
    with _recording_engine() as e:
        op = IcpAlign(IcpSettings(segment_source=seg, sample_fraction=1.0, icp_iterations=5), engine=e)
        op.run(xyz, tgt, mxa, mxb, vlist=vlist)
        got = op.last_segmentation
        assert np.array_equal(e.vlist_seen, vlist[kept]) and got["target"] is None and e.calls == ()     # (a context of its own)
        assert np.array_equal(got["source"]["index"], kept) and np.array_equal(got["source"]["label"], label)
        assert np.array_equal(got["source"]["vlist"], vlist[kept])
        # after clean_source
        cleaned = np.flatnonzero(A.sum(axis=1) - 1 >= 6)
        sub = dbscan_ref(sel[cleaned], 0.15, 6)
        composed = cleaned[keep_ref(sub[0], sub[1], "largest")]
        both = IcpAlign(IcpSettings(clean_source=OutlierSettings(method="radius", radius=0.15, min_neighbors=6), segment_source=seg,
                                    sample_fraction=1.0, icp_iterations=5), engine=e)
        both.run(xyz, tgt, mxa, mxb, vlist=vlist)
        assert np.array_equal(both.last_cleaning["source"]["index"], cleaned)
        assert np.array_equal(both.last_segmentation["source"]["index"], composed)
        assert np.array_equal(e.vlist_seen, vlist[composed])
        # no vlist: the whole cloud is the selection
        whole = IcpAlign(IcpSettings(segment_source=ClusterSettings(eps=0.12, min_points=8), sample_fraction=1.0, icp_iterations=5), engine=e)
        whole.run(xyz, tgt, mxa, mxb)
        assert np.array_equal(e.vlist_seen, np.flatnonzero(keep_ref(fixture_ref()[0], fixture_ref()[1], "largest")))
        # both settings off: nothing recorded, the selection untouched
        off = IcpAlign(IcpSettings(sample_fraction=1.0, icp_iterations=5), engine=e)
        off.run(xyz, tgt, mxa, mxb)
        assert off.last_segmentation is None and e.vlist_seen is None and e.calls == ()


@pytest.mark.gpu
def test_gpu_cluster_dbscan_module_level(built):
    import object_alignment_amd as oa
    xyz = fixture()[0]
    out = oa.cluster_dbscan(xyz, 0.12)
    check({k: v for k, v in out.items() if k != "xyz"}, xyz, fixture_ref(), "clustered")
    assert out["xyz"].dtype == np.float32 and np.array_equal(out["xyz"], xyz[out["index"]])
    big = oa.cluster_dbscan(xyz.astype(np.float64).tolist(), 0.12, min_points=8, keep="min_size", min_size=601)
    check({k: v for k, v in big.items() if k != "xyz"}, xyz, fixture_ref(), "min_size", 601)
    assert len(big["xyz"]) == 6048


@pytest.mark.gpu
def test_gpu_cluster_refusals_leave_the_context_usable(built):
    """OA_E_STATE without a target, on a surface target and on a multi-device context; OA_E_BAD_ARG for every range, through the
    error text channel; the context runs a loop afterwards."""
    from object_alignment_amd import _capi, synth
    from object_alignment_amd.engine import IcpEngine
    L = _capi.load()
    x = torus(300, seed=4)
    eye = np.identity(4, dtype=np.float32)

    def clusters(e, **kw):
        st = _capi.ClusterSettings(kw.get("eps", 0.2), kw.get("min_points", 4), kw.get("keep", 1), kw.get("min_size", 0))
        rc = L.oa_target_clusters(e._h, C.byref(st), kw.get("apply", 0), None, None, None, None, None)
        return rc, L.oa_last_error().decode()

    with IcpEngine(0) as e:
        rc, msg = clusters(e)
        assert rc == _capi.OA_E_STATE and "oa_set_target" in msg                # no target
        e.set_target(x)
        for kw in (dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(min_points=0), dict(min_points=-3),
                   dict(keep=3), dict(keep=-1), dict(min_size=-1)):
            rc, msg = clusters(e, **kw)
            assert rc == _capi.OA_E_BAD_ARG and "oa_target_clusters" in msg, (kw, rc, msg)
        assert L.oa_target_clusters(e._h, None, 0, None, None, None, None, None) == _capi.OA_E_BAD_ARG
        assert clusters(e)[0] == _capi.OA_OK and clusters(e, keep=2, min_size=10**12)[0] == _capi.OA_OK      # every output NULL
        verts, tris = synth.icosphere_mesh(1)
        e.set_target_mesh(verts, tris)
        rc, msg = clusters(e)
        assert rc == _capi.OA_E_STATE and "surface" in msg
        e.set_target(x)
        e.set_source(x, stride=1)
        e.set_matrices(eye, eye)
        assert e.run(iters=3).iters_done >= 1
    with IcpEngine(devices=[0, 0]) as m:
        m.set_target(x)
        rc, msg = clusters(m)
        assert rc == _capi.OA_E_STATE and "multi-device" in msg
        m.set_source(x, stride=1)                                                # ... and it goes on working
        m.set_matrices(eye, eye)
        assert m.nn_search()[0].shape == (300,) and m.run(iters=3).iters_done >= 1
