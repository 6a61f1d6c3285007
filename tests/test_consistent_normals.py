"""One consistent sign for a cloud's normals (oa_orient_target_normals): the contract restated in numpy -- Kruskal
with union-find over the edges of the LIBRARY's own k-nearest rows (so that ties between neighbours cannot matter), the same float32
weight expression, the order (w, lo, hi), signs by a walk over the tree, the seed rule in fp64 -- and the library against it,
EXACTLY: flipped, component, the normals' bits and the report.  What the call is for: on a torus the sign of a point-cloud
target's deviation is right everywhere with it and on fewer than 70 % of the points with normals turned away from the centroid.

CPU: -m "not gpu" (ABI, argument errors, the fixture guards on the restatement with brute-force neighbours); GPU: -m gpu.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build_hip()
    return g


@pytest.fixture(scope="module")
def eng(built):
    from object_alignment_amd.engine import IcpEngine
    with IcpEngine(0) as e:
        yield e


# ------------------------------------------------------------------------------------------------ the clouds
def torus(n, R=1.0, r=0.35, seed=1):
    """(points float32, analytic outward normals fp64): n random points of a torus"""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    x = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], 1)
    return x.astype(np.float32), np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)


def bent_tube(n, R=1.0, r=0.25, seed=2):
    """a tube bent over 300 degrees, open ends: an arch"""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, np.pi * 5 / 3, n), rng.uniform(0, 2 * np.pi, n)
    x = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], 1)
    return x.astype(np.float32), np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)


def two_tori_and_island():
    """tori of 3 000 and 1 500 points and an island of 40 points 8 units away, shuffled; (points, analytic normals, on a torus)"""
    x1, n1 = torus(3000, seed=3)
    x2, n2 = torus(1500, R=0.6, r=0.2, seed=4)
    x2 = x2 + np.float32([3.0, 0.5, 0.2])
    rng = np.random.default_rng(6)
    isl = np.concatenate([rng.uniform(-0.15, 0.15, (40, 2)), rng.uniform(-0.002, 0.002, (40, 1))], 1) + np.array([0.0, 8.0, 0.0])
    x = np.concatenate([x1, x2, isl.astype(np.float32)])
    ana = np.concatenate([n1, n2, np.tile([0.0, 0.0, 1.0], (40, 1))])
    perm = np.random.default_rng(0).permutation(len(x))
    return x[perm], ana[perm], (np.arange(len(x)) < 4500)[perm]


def flat_lattice():
    """a flat 40 x 30 lattice, shuffled, with normals (0, 0, +-1) of random sign: every weight is 0, the indices decide everything"""
    g = np.stack(np.meshgrid(np.arange(40), np.arange(30), indexing="ij"), -1).reshape(-1, 2)
    x = np.concatenate([g, np.zeros((len(g), 1))], 1).astype(np.float32)
    x = x[np.random.default_rng(1).permutation(len(x))]
    sign = np.random.default_rng(2).choice([-1.0, 1.0], len(x)).astype(np.float32)
    return x, np.tile(np.float32([0, 0, 1]), (len(x), 1)) * sign[:, None]


def ribbon():
    """3 x 3 000 points on a helical strip: long chains of hooks in a round, deep pointer jumping; (points, radial normals)"""
    t, s = np.repeat(np.arange(3000), 3) * 0.01, np.tile(np.arange(3), 3000) * 0.01
    x = np.stack([np.cos(t), np.sin(t), 0.05 * t + s], 1).astype(np.float32)
    return x, np.stack([np.cos(t), np.sin(t), 0 * t], 1)


def lattice(nx, ny, nz, seed=3):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).reshape(-1, 3)
    return g[np.random.default_rng(seed).permutation(len(g))].astype(np.float32)


def boundary_cloud(n):
    """2, 5, 64, 65 and 4 097 vertices (one, two and three box levels, as tests/test_target_normals.py's lattice cases) with random
    unit normals of random sign"""
    pts = lattice(8, 8, 64)
    x = pts[:n].copy() if n <= 64 else np.concatenate([pts[: n - 1], np.array([[1000.0, -500.0, 250.0]], np.float32)])
    nrm = np.random.default_rng(100 + n).normal(size=(n, 3))
    return x, (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the restatement
def knn_brute(xyz, k):
    """(idx int32 (n, k), d2 float32 (n, k)) by brute force in fp64, sorted by (d2, index), self included: the CPU guards' rows"""
    x = np.asarray(xyz, np.float64)
    idx, d2 = np.empty((len(x), k), np.int32), np.empty((len(x), k), np.float32)
    for b in range(0, len(x), 512):
        d = ((x[b:b + 512, None, :] - x[None, :, :]) ** 2).sum(axis=2)
        o = np.argsort(d, axis=1, kind="stable")[:, :k]
        idx[b:b + 512], d2[b:b + 512] = o, np.take_along_axis(d, o, axis=1)
    return idx, d2


def pca_normals(xyz, idx):
    """PCA normals (float32, canonical sign) from neighbour lists: the CPU guards' normals"""
    x = np.asarray(xyz, np.float64)
    nb = x[np.asarray(idx, np.int64)]
    c = nb - nb.mean(axis=1, keepdims=True)
    _, vec = np.linalg.eigh(np.einsum("nki,nkj->nij", c, c))
    n = vec[:, :, 0]
    m = np.argmax(np.abs(n), axis=1)
    return (n * np.where(n[np.arange(len(n)), m] < 0, -1.0, 1.0)[:, None]).astype(np.float32)


def away_from_centroid(xyz, n32):
    x = np.asarray(xyz, np.float64)
    dot = np.einsum("ij,ij->i", n32.astype(np.float64), x - x.mean(axis=0))
    return n32 * np.where(dot < 0, -1.0, 1.0).astype(np.float32)[:, None]


def eligible_of(xyz, n32):
    return np.isfinite(n32).all(axis=1) & (n32 != 0).any(axis=1) & np.isfinite(xyz).all(axis=1)


def graph_edges(xyz, n32, idx, d2, max_dist):
    """the undirected edges (lo, hi), their float32 weights and flips, from k-nearest rows: include/oa_icp.h's rule"""
    N, k = idx.shape
    ok = eligible_of(xyz, n32)
    i, j = np.repeat(np.arange(N), k), idx.reshape(-1).astype(np.int64)
    m = (j >= 0) & (j < N) & (j != i)
    m[m] &= ok[i[m]] & ok[j[m]]
    if max_dist > 0:
        m &= d2.reshape(-1) <= np.float32(max_dist) * np.float32(max_dist)
    i, j = i[m], j[m]
    e = np.unique(np.stack([np.minimum(i, j), np.maximum(i, j)], 1), axis=0).reshape(-1, 2)
    lo, hi = e[:, 0], e[:, 1]
    a, b = n32[lo], n32[hi]
    with np.errstate(all="ignore"):
        d = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]      # float32 arrays: one rounding per operation
        t = np.float32(1) - np.abs(d)
    assert d.dtype == np.float32 and t.dtype == np.float32
    return lo, hi, np.where(t > 0, t, np.float32(0)), d < 0, ok


def kruskal(N, lo, hi, w):
    """the edges of the minimum spanning forest under (w, lo, hi), by union-find"""
    par = np.arange(N)

    def find(a):
        while par[a] != a:
            par[a] = par[par[a]]
            a = par[a]
        return a

    tree = []
    for e in np.lexsort((hi, lo, w)):
        a, b = find(lo[e]), find(hi[e])
        if a != b:
            par[a] = b
            tree.append(e)
    return np.array(tree, np.int64)


def boruvka_rounds(N, lo, hi, w):
    """rounds in which components merge when every component takes its least edge (w, lo, hi) out, all at once"""
    pos = np.empty(len(lo), np.int64)
    pos[np.lexsort((hi, lo, w))] = np.arange(len(lo))
    by_pos = np.argsort(pos)
    comp, rounds = np.arange(N), 0
    while True:
        out = comp[lo] != comp[hi]
        if not out.any():
            return rounds
        rounds += 1
        best = np.full(N, len(lo), np.int64)
        np.minimum.at(best, comp[lo[out]], pos[out])
        np.minimum.at(best, comp[hi[out]], pos[out])
        par = np.arange(N)

        def find(a):
            while par[a] != a:
                par[a] = par[par[a]]
                a = par[a]
            return a

        for e in by_pos[np.unique(best[best < len(lo)])]:
            a, b = find(comp[lo[e]]), find(comp[hi[e]])
            if a != b:
                par[max(a, b)] = min(a, b)
        comp = np.array([find(c) for c in comp])


def orient_numpy(xyz, normals, idx, d2, seed="away", point=None, max_dist=0.0):
    """(normals, flipped uint8, component int32, report) as include/oa_icp.h states them, from the rows (idx, d2)"""
    xyz, n32 = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(normals, np.float32)
    N = len(xyz)
    lo, hi, w, flip, ok = graph_edges(xyz, n32, np.asarray(idx), np.asarray(d2), max_dist)
    tree = kruskal(N, lo, hi, w)
    nbr = [[] for _ in range(N)]
    for e in tree:
        nbr[lo[e]].append((hi[e], bool(flip[e])))
        nbr[hi[e]].append((lo[e], bool(flip[e])))
    comp, par = np.full(N, -1, np.int64), np.zeros(N, bool)         # par: the sign relative to the component's lowest index
    for s in range(N):
        if not ok[s] or comp[s] >= 0:
            continue
        comp[s] = s
        stack = [s]
        while stack:
            a = stack.pop()
            for b, f in nbr[a]:
                if comp[b] < 0:
                    comp[b], par[b] = s, par[a] ^ f
                    stack.append(b)
    x64, n64 = xyz.astype(np.float64), n32.astype(np.float64)
    if seed != "keep":
        p = x64[np.isfinite(xyz).all(axis=1)].mean(axis=0) if point is None else np.asarray(point, np.float32).astype(np.float64)
    flipped = np.zeros(N, bool)
    labels = np.unique(comp[comp >= 0])
    for s in labels:
        m = np.where(comp == s)[0]
        want = False
        if seed == "keep":
            sd = s
        else:
            d = x64[m] - p
            dist = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            sd = m[np.argmin(dist) if seed == "toward" else np.argmax(dist)]       # (the first of equal ones: the lowest index)
            v = (p - x64[sd]) if seed == "toward" else (x64[sd] - p)
            want = bool((n64[sd, 0] * v[0] + n64[sd, 1] * v[1]) + n64[sd, 2] * v[2] < 0.0)
        flipped[m] = par[m] ^ par[sd] ^ want
    out = n32.copy().view(np.uint32)
    out[flipped] ^= np.uint32(0x80000000)
    report = {"n_components": len(labels), "n_left_out": int((~ok).sum()), "n_flipped": int(flipped.sum()),
              "rounds": boruvka_rounds(N, lo, hi, w)}
    return out.view(np.float32), flipped.astype(np.uint8), comp.astype(np.int32), report


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def agreement(n32, analytic):
    return float(np.mean(np.einsum("ij,ij->i", np.asarray(n32, np.float64), analytic) > 0))


def deviation_case():
    """the torus' points pushed +-0.05 off the surface along the analytic normal: (queries float32, the side of each)"""
    x, ana = torus(4000)
    side = np.random.default_rng(5).choice([-1.0, 1.0], len(x))
    return (x + (0.05 * side)[:, None] * ana).astype(np.float32), side


def nearest_sign(xyz, n32, q):
    """the sign of (q - v) . n_v at q's nearest vertex v (brute force, fp64)"""
    x, qq = np.asarray(xyz, np.float64), np.asarray(q, np.float64)
    near = np.concatenate([np.argmin(((qq[b:b + 512, None, :] - x[None, :, :]) ** 2).sum(axis=2), axis=1) for b in range(0, len(qq), 512)])
    return np.sign(np.einsum("ij,ij->i", n32[near].astype(np.float64), qq - x[near]))


# ------------------------------------------------------------------------------------------------ CPU
def test_orient_abi_and_bindings(built):
    from object_alignment_amd import _capi
    from object_alignment_amd.operators import IcpSettings
    header = open(os.path.join(ROOT, "include", "oa_icp.h")).read()
    L = _capi.load()
    assert "oa_orient_target_normals" in _capi.SYMBOLS and hasattr(L, "oa_orient_target_normals")
    assert re.search(r"\bint\s+oa_orient_target_normals\s*\(", header)
    R = _capi.OrientReport
    assert C.sizeof(R) == 32
    assert (R.n_components.offset, R.n_left_out.offset, R.n_flipped.offset, R.rounds.offset, R.reserved.offset) == (0, 8, 16, 24, 28)
    body = re.search(r"typedef struct oa_orient_report \{(.*?)\} oa_orient_report;", header, re.S).group(1)
    declared = re.findall(r"\b([A-Za-z_]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert declared == [f for f, _ in R._fields_], declared
    for name, value in (("OA_SEED_KEEP", 0), ("OA_SEED_TOWARD", 1), ("OA_SEED_AWAY", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header) and getattr(_capi, name) == value
    assert os.path.exists(os.path.join(ROOT, "object_alignment_amd", "csrc", "oa_orient.hpp"))
    assert IcpSettings().normal_orient == "away"


def test_orient_argument_errors_before_any_engine_opens(monkeypatch):
    import object_alignment_amd as oa
    from object_alignment_amd import engine as eng_mod
    from object_alignment_amd.operators import IcpAlign, IcpSettings

    def no_engine(*a, **k):
        raise AssertionError("an engine was opened")

    monkeypatch.setattr(eng_mod.IcpEngine, "__init__", no_engine)
    xyz, nrm = boundary_cloud(64)
    for bad in (dict(k=1), dict(k=65), dict(k=8.0), dict(k=True), dict(k=None), dict(max_dist=-1.0), dict(max_dist=float("inf")),
                dict(max_dist=float("nan")), dict(max_dist="1"), dict(seed="outward"), dict(seed=3), dict(seed=None), dict(seed="toward"),
                dict(seed="toward", point=None), dict(point=[0.0, 1.0]), dict(point=[0.0, float("nan"), 0.0]),
                dict(point=[0.0, float("inf"), 0.0])):
        with pytest.raises(ValueError):
            oa.orient_normals(xyz, nrm, **bad)
    for bad_rows in (nrm[:, :2], nrm.reshape(-1), nrm[:10], np.array([["a", "b", "c"]] * 64), None):
        with pytest.raises(ValueError):
            oa.orient_normals(xyz, bad_rows)
    with pytest.raises(ValueError):
        oa.orient_normals(xyz[:1], nrm[:1])
    with pytest.raises(ValueError):
        oa.orient_normals(xyz[:5], nrm[:5], k=6)                       # k > n
    e = object.__new__(eng_mod.IcpEngine)                             # the argument checks need no context
    e._h, e.n_target = None, 64
    for bad in (dict(k=1), dict(k=65), dict(seed="up"), dict(seed="toward"), dict(max_dist=-0.5), dict(normals=nrm[:5]), dict(point=[1.0])):
        with pytest.raises(ValueError):
            e.orient_target_normals(**bad)
    eye = np.identity(4, dtype=np.float32)
    for bad in ("toward", "Consistent", "", None, 1):
        with pytest.raises(ValueError):
            IcpAlign(IcpSettings(normal_orient=bad)).run(xyz, xyz, eye, eye, target_normals="estimate")


GUARD = {"torus": torus, "tube": bent_tube}


@functools.lru_cache(maxsize=None)
def guard_case(name):
    """with brute-force neighbours and numpy PCA normals (k = 16): the share of vertices on which normals turned away from the
    centroid agree with the analytic ones, the share for the restated consistent orientation (graph k = 8), and those normals"""
    x, ana = GUARD[name](4000)
    idx, d2 = knn_brute(x, 16)
    n32 = pca_normals(x, idx)
    away = away_from_centroid(x, n32)
    out, _, comp, rep = orient_numpy(x, n32, idx[:, :8], d2[:, :8], seed="away")
    return x, ana, away, out, comp, rep


@pytest.mark.parametrize("name", ["torus", "tube"])
def test_fixture_guard_away_is_wrong_and_the_restatement_is_right(name):
    x, ana, away, out, comp, rep = guard_case(name)
    assert agreement(away, ana) < 0.70, agreement(away, ana)         # (62.6 % on the torus, 58.3 % on the tube)
    assert agreement(out, ana) == 1.0, agreement(out, ana)
    assert rep["n_components"] == 1 and rep["n_left_out"] == 0 and (comp == 0).all()


def test_fixture_guard_deviation_sign():
    x, ana, away, out, _, _ = guard_case("torus")
    q, side = deviation_case()
    assert float(np.mean(nearest_sign(x, out, q) == side)) == 1.0
    assert float(np.mean(nearest_sign(x, away, q) == side)) < 0.70


def test_fixture_guard_flat_lattice_and_ribbon():
    x, nrm = flat_lattice()
    idx, d2 = knn_brute(x, 9)
    lo, hi, w, _, _ = graph_edges(x, nrm, idx, d2, 0.0)
    assert (w == 0).all() and len(lo) > len(x)                       # every weight ties: the indices decide
    below = np.float32([20.0, 15.0, -100.0])
    out, _, comp, rep = orient_numpy(x, nrm, idx, d2, seed="toward", point=below)
    assert (out[:, 2] < 0).all() and rep["n_components"] == 1        # toward a point below the plane
    out, flipped, _, _ = orient_numpy(x, nrm, idx, d2, seed="keep")
    assert (out[:, 2] == nrm[0, 2]).all() and not flipped[0]
    xr, radial = ribbon()
    idx, d2 = knn_brute(xr, 12)
    out, _, _, rep = orient_numpy(xr, pca_normals(xr, idx), idx[:, :8], d2[:, :8], seed="away", point=[0.0, 0.0, 0.75])
    assert rep["n_components"] == 1 and agreement(out, radial) in (0.0, 1.0)


# ------------------------------------------------------------------------------------------------ GPU
def upload(eng, xyz, normals=None, pca_k=16):
    """the cloud as the engine's target; its normals installed: the given ones, or the library's own PCA estimate of canonical sign.
    Returns them."""
    eng.set_target(xyz)
    if normals is None:
        return eng.estimate_target_normals(k=pca_k, orient="none", install=True)[0]
    eng.set_target_normals(normals)
    return np.ascontiguousarray(normals, np.float32)


def check_exact(eng, xyz, n32, k, seed="away", point=None, max_dist=0.0, given=False):
    """one library call against the restatement over the library's own rows; returns what the library gave"""
    idx, d2 = eng.target_knn(k)
    got = eng.orient_target_normals(k=k, max_dist=max_dist, seed=seed, point=point, normals=n32 if given else None, install=False)
    want = orient_numpy(xyz, n32, idx, d2, seed=seed, point=point, max_dist=max_dist)
    assert got[3] == want[3], (got[3], want[3])
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[1], want[1]), int((got[1] != want[1]).sum())
    assert same_bits(got[0], want[0])
    assert got[0].dtype == np.float32 and got[1].dtype == np.uint8 and got[2].dtype == np.int32
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("k", [8, 16])
def test_gpu_torus_matches_the_restatement(eng, k):
    x, ana = torus(4000)
    n32 = upload(eng, x)
    out, flipped, comp, rep = check_exact(eng, x, n32, k)
    assert rep["n_components"] == 1 and rep["n_left_out"] == 0 and rep["rounds"] >= 2
    if k == 8:                                                       # two calls give the same bytes
        again = eng.orient_target_normals(k=k, install=False)
        assert same_bits(again[0], out) and np.array_equal(again[1], flipped) and np.array_equal(again[2], comp) and again[3] == rep


@pytest.mark.gpu
def test_gpu_bent_tube_matches_the_restatement(eng):
    x, ana = bent_tube(4000)
    n32 = upload(eng, x)
    check_exact(eng, x, n32, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("max_dist", [0.5, 0.0])
def test_gpu_two_tori_and_an_island(eng, max_dist):
    x, ana, on_torus = two_tori_and_island()
    n32 = upload(eng, x)
    out, flipped, comp, rep = check_exact(eng, x, n32, 8, max_dist=max_dist)
    assert rep["n_components"] == 3 and len(np.unique(comp)) == 3    # each seeded on its own
    assert agreement(out[on_torus], ana[on_torus]) == 1.0


@pytest.mark.gpu
def test_gpu_flat_lattice_every_weight_ties(eng):
    x, nrm = flat_lattice()
    upload(eng, x, nrm)
    below = [20.0, 15.0, -100.0]
    out, _, comp, rep = check_exact(eng, x, nrm, 9, seed="toward", point=below)
    assert (out[:, 2] < 0).all() and rep["n_components"] == 1 and (comp == 0).all()
    out, flipped, _, _ = check_exact(eng, x, nrm, 9, seed="keep")
    assert (out[:, 2] == nrm[0, 2]).all() and flipped[0] == 0
    check_exact(eng, x, nrm, 9, seed="away", point=below, given=True)


@pytest.mark.gpu
def test_gpu_helical_ribbon_long_chains(eng):
    x, radial = ribbon()
    n32 = upload(eng, x, pca_k=12)
    out, _, _, rep = check_exact(eng, x, n32, 8, seed="away", point=[0.0, 0.0, 0.75])
    assert rep["n_components"] == 1 and agreement(out, radial) in (0.0, 1.0)       # one sign throughout


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 5, 64, 65, 4097])
def test_gpu_tiny_and_boundary_sizes(eng, n):
    x, nrm = boundary_cloud(n)
    upload(eng, x, nrm)
    k = min(n, 8)
    for seed, point in (("keep", None), ("away", None), ("toward", [3.5, 3.5, -40.0])):
        check_exact(eng, x, nrm, k, seed=seed, point=point)
    if n == 2:
        out, flipped, comp, rep = eng.orient_target_normals(k=2, seed="keep", install=False)
        assert rep["n_components"] == 1 and rep["rounds"] == 1 and list(comp) == [0, 0] and flipped[0] == 0
    if n == 5:                                                       # the cap cuts the graph: without it one component
        assert check_exact(eng, x, nrm, 5, seed="keep")[3]["n_components"] == 1
        d2 = eng.target_knn(5)[1]
        cut = float(np.sqrt(np.sort(np.unique(d2[d2 > 0]))[0])) * 1.0001
        assert check_exact(eng, x, nrm, 5, seed="keep", max_dist=cut)[3]["n_components"] > 1


@pytest.mark.gpu
def test_gpu_vertices_left_out(eng):
    x, _ = torus(700, seed=9)
    x = x.copy()
    nrm = pca_normals(x, knn_brute(x, 12)[0])
    nrm[[3, 90, 91, 400]] = 0.0
    nrm[17, 1] = np.nan
    nrm[250, 0] = np.inf
    x[333, 2] = np.inf
    out_of = np.array([3, 17, 90, 91, 250, 333, 400])
    eng.set_target(x)
    for seed, point in (("keep", None), ("toward", [0.0, 0.0, 5.0])):
        out, flipped, comp, rep = check_exact(eng, x, nrm, 8, seed=seed, point=point, given=True)
        assert rep["n_left_out"] == len(out_of) and (comp[out_of] == -1).all() and (flipped[out_of] == 0).all()
        assert same_bits(out[out_of], nrm[out_of]) and (np.delete(comp, out_of) >= 0).all()


@pytest.mark.gpu
def test_gpu_installed_orientation_signs_the_deviation(eng):
    """The capability: on the torus the sign of the deviation of points pushed +-0.05 off the surface."""
    x, ana = torus(4000)
    q, side = deviation_case()
    eye = np.identity(4, dtype=np.float32)
    right = {}
    for how in ("away", "consistent"):
        eng.set_target(x)
        eng.estimate_target_normals(k=16, orient="away", install=True)
        if how == "consistent":
            out = eng.orient_target_normals(k=8, install=True)[0]
            assert agreement(out, ana) == 1.0
        eng.set_source(q, stride=1)
        eng.set_matrices(eye, eye)
        dev = eng.deviation(signed=True, outputs=("signed_d",))
        right[how] = float(np.mean(np.sign(dev["signed_d"]) == side))
    print("deviation sign right: %r" % (right,))
    assert right["consistent"] == 1.0
    assert right["away"] < 0.70


def installed_normals(eng, k=8):
    """the target's installed normals, read through a call that does not install: out = installed with the flipped ones toggled"""
    out, flipped, _, _ = eng.orient_target_normals(k=k, seed="keep", install=False)
    bits = out.copy().view(np.uint32)
    bits[flipped.astype(bool)] ^= np.uint32(0x80000000)
    return bits.view(np.float32)


@pytest.mark.gpu
def test_gpu_run_with_normal_orient(eng):
    from object_alignment_amd.operators.icp_align import IcpAlign, IcpSettings
    from object_alignment_amd import synth
    x, _ = torus(4000)
    src = x[::4].copy()
    mxa = synth.rigid4(synth.rotation_from_rotvec([0.02, -0.01, 0.015]), [0.01, -0.005, 0.008])
    eye = np.identity(4, dtype=np.float32)
    eng.set_target(x)
    away = eng.estimate_target_normals(k=16, orient="away", install=True)[0]
    consistent = eng.orient_target_normals(k=16, seed="away", install=True)[0]
    assert not same_bits(away, consistent)
    IcpAlign(IcpSettings(normal_k=16, normal_orient="consistent"), engine=eng).run(src, x, mxa, eye, target_normals="estimate")
    assert same_bits(installed_normals(eng), consistent)
    IcpAlign(IcpSettings(normal_k=16), engine=eng).run(src, x, mxa, eye, target_normals="estimate")
    assert same_bits(installed_normals(eng), away)                  # the default: today's normals, bit for bit


@pytest.mark.gpu
def test_gpu_orient_normals_of_any_cloud(eng):
    import object_alignment_amd as oa
    x, ana = bent_tube(4000)
    n32 = upload(eng, x)
    want = eng.orient_target_normals(k=8, install=False)
    got = oa.orient_normals(x, n32, k=8)
    assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[3] == want[3]
    assert agreement(got[0], ana) == 1.0


@pytest.mark.gpu
def test_gpu_refusals_leave_the_context_usable(built):
    from object_alignment_amd import _capi, synth
    from object_alignment_amd.engine import IcpEngine
    L = _capi.load()
    x, nrm = boundary_cloud(64)
    rep = _capi.OrientReport()
    point = _capi.as_f32([0.0, 0.0, 1.0])

    def call(e, k=8, max_dist=0.0, seed=0, pt=None, normals=nrm):
        rc = L.oa_orient_target_normals(e._h, k, max_dist, seed, _capi.fptr(pt) if pt is not None else None,
                                        _capi.fptr(normals) if normals is not None else None, 0, None, None, None, C.byref(rep))
        return rc, L.oa_last_error().decode()

    with IcpEngine(0) as e:
        rc, msg = call(e)
        assert rc == _capi.OA_E_STATE and "oa_set_target" in msg                # no target
        e.set_target(x)
        for kw in (dict(k=1), dict(k=65), dict(seed=-1), dict(seed=3), dict(seed=1), dict(pt=_capi.as_f32([0.0, np.nan, 0.0])),
                   dict(pt=_capi.as_f32([np.inf, 0.0, 0.0]), seed=2), dict(max_dist=-1.0), dict(max_dist=float("inf")), dict(max_dist=float("nan"))):
            rc, msg = call(e, **kw)
            assert rc == _capi.OA_E_BAD_ARG and "oa_orient_target_normals" in msg, (kw, rc, msg)
        rc, msg = call(e, normals=None)
        assert rc == _capi.OA_E_STATE and "normals" in msg                      # NULL normals and none installed
        assert call(e, seed=1, pt=point)[0] == _capi.OA_OK and rep.n_components >= 1
        e.set_target(x[:5])
        assert call(e, k=6, normals=nrm[:5])[0] == _capi.OA_E_BAD_ARG           # k > nt
        assert call(e, k=5, normals=nrm[:5])[0] == _capi.OA_OK
        verts, tris = synth.icosphere_mesh(1)
        e.set_target_mesh(verts, tris)
        rc, msg = call(e, normals=np.zeros((len(verts), 3), np.float32))
        assert rc == _capi.OA_E_STATE and "surface" in msg
        e.set_target(x)
        assert call(e)[0] == _capi.OA_OK
    with IcpEngine(devices=[0, 0]) as m:
        m.set_target(x)
        rc, msg = call(m)
        assert rc == _capi.OA_E_STATE and "multi-device" in msg
        m.set_source(x, stride=1)                                                # ... and it goes on working
        m.set_matrices(np.identity(4, dtype=np.float32), np.identity(4, dtype=np.float32))
        assert m.nn_search()[0].shape == (64,)


@pytest.mark.gpu
def test_gpu_refusal_capacity(built):
    """nt k beyond what one int32 entry index reaches: refused before anything is allocated, and the context goes on working"""
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    L = _capi.load()
    n = (2 ** 31 - 2 ** 20) // 64 + 1                               # with k = 64 the first size past the limit
    i = np.arange(n, dtype=np.int64)
    x = np.stack([i % 512, (i // 512) % 512, i // (512 * 512)], 1).astype(np.float32)
    rep = _capi.OrientReport()
    with IcpEngine(0) as e:
        e.set_search_mode("brute")                                   # (no index is built with the upload)
        e.set_target(x)
        rc = L.oa_orient_target_normals(e._h, 64, 0.0, 0, None, _capi.fptr(x), 0, None, None, None, C.byref(rep))
        assert rc == _capi.OA_E_CAPACITY and "entries" in L.oa_last_error().decode()
        small, nrm = boundary_cloud(64)
        e.set_target(small)
        assert e.orient_target_normals(k=8, seed="keep", normals=nrm, install=False)[3]["n_components"] == 1
