"""Normal-space sampling and the stability report (oa_normal_space_sample, oa_stability): both contracts restated
in numpy, the library against the restatement -- the sample bit for bit, the 6 x 6 matrix within a rounding bound derived from
the number of terms and their magnitudes --, and what the sample is for: on a grooved plane it conditions the loop's 6 x 6
system at least twice as well as an every-k-th sample.

CPU: -m "not gpu" (ABI, argument errors, the fixture guards on the restatement alone); GPU: -m gpu.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53                  # the unit roundoff of fp64
EIG_CUT = 1e-10                 # PLANE_EIG_CUT of csrc/oa_kernels.hpp
SORT_SMALL_MAX = 8192           # csrc/oa_sort.hpp: above this the three-pass sort takes over from the one-workgroup sort


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


# ------------------------------------------------------------------------------------------------ the restatements
def eligible_normals(normals):
    n32 = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    d = n32.astype(np.float64)
    with np.errstate(all="ignore"):
        l2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        ok = np.all(np.isfinite(n32), axis=1) & np.isfinite(l2) & (l2 > 0.0)
    return d, l2, ok


def bins_numpy(normals, G=8, unoriented=False):
    """The bin of every normal (-1: not eligible), include/oa_icp.h's rule in fp64."""
    d, _, ok = eligible_normals(normals)
    n = len(d)
    d = np.where(ok[:, None], d, 1.0)                               # (the others' arithmetic is dropped)
    ad = np.abs(d)
    a = np.zeros(n, np.int64)
    big = ad[:, 0].copy()
    m1 = ad[:, 1] > big
    a[m1] = 1
    big[m1] = ad[m1, 1]
    a[ad[:, 2] > big] = 2
    rows = np.arange(n)
    na, nb, nc = d[rows, a], d[rows, (a + 1) % 3], d[rows, (a + 2) % 3]
    den = na if unoriented else np.abs(na)
    half = 0.5 * float(G)
    iu = np.minimum(G - 1, np.floor((nb / den + 1.0) * half).astype(np.int64))
    iv = np.minimum(G - 1, np.floor((nc / den + 1.0) * half).astype(np.int64))
    f = a if unoriented else 2 * a + (na < 0.0)
    return np.where(ok, (f * G + iv) * G + iu, -1).astype(np.int32)


def nss_numpy(normals, m, G=8, unoriented=False, seed=0):
    """The contract of oa_normal_space_sample: {"idx", "bin", "report", "remainder"}."""
    bins = bins_numpy(normals, G, unoriented)
    n = len(bins)
    h = (np.arange(n, dtype=np.uint32) ^ np.uint32(seed)) * np.uint32(0x9E3779B1)
    elig = np.flatnonzero(bins >= 0)
    if len(elig) == 0:
        raise ValueError("no eligible point")
    order = elig[np.lexsort((h[elig], bins[elig]))]                 # by bin, then by hash
    c = np.bincount(bins[elig], minlength=(3 if unoriented else 6) * G * G).astype(np.int64)
    given = lambda t: int(np.minimum(c, t).sum())
    if m >= len(elig):
        t, r = int(c.max()), 0
    else:
        lo, hi = 0, int(c.max())                                    # given(lo) <= m < given(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if given(mid) <= m else (lo, mid)
        t, r = lo, m - given(lo)
        assert given(t) <= m < given(t + 1)
    take = np.minimum(c, t)
    take[np.flatnonzero(c > t)[:r]] += 1
    start = np.concatenate([[0], np.cumsum(c)[:-1]])
    idx = np.sort(np.concatenate([order[start[b]: start[b] + take[b]] for b in np.flatnonzero(take)])).astype(np.int64)
    report = {"n_in": n, "n_eligible": len(elig), "bins_occupied": int((c > 0).sum()), "level": t, "max_bin_count": int(c.max())}
    return {"idx": idx, "bin": bins, "report": report, "remainder": r}


def used_rows(xyz, normals, idx):
    """(p, n, l2) of the eligible points among those idx lists (None: all), in fp64."""
    p32 = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    use = np.arange(len(p32)) if idx is None else np.asarray(idx, np.int64)
    d, l2, ok = eligible_normals(np.ascontiguousarray(normals, np.float32).reshape(-1, 3)[use])
    p = p32[use]
    ok &= np.all(np.isfinite(p), axis=1)
    return p[ok].astype(np.float64), d[ok], l2[ok]


def stability_rows(xyz, normals, idx, c, s):
    """v = [q x nh ; nh] of the eligible used points, one row each, in fp64 with the contract's grouping."""
    p, d, l2 = used_rows(xyz, normals, idx)
    nh = d * (1.0 / np.sqrt(l2))[:, None]
    q = (p - c) * s
    cross = np.stack([q[:, 1] * nh[:, 2] - q[:, 2] * nh[:, 1], q[:, 2] * nh[:, 0] - q[:, 0] * nh[:, 2], q[:, 0] * nh[:, 1] - q[:, 1] * nh[:, 0]], axis=1)
    return np.concatenate([cross, nh], axis=1)


def mean_distance(p, c):
    dx, dy, dz = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def stability_numpy(xyz, normals, idx=None):
    """The contract of oa_stability with exactly rounded sums (math.fsum) and numpy's eigenvalues: what the GPU result is near."""
    p = used_rows(xyz, normals, idx)[0]
    k = len(p)
    c = np.array([math.fsum(p[:, a]) / k for a in range(3)])
    mean = math.fsum(mean_distance(p, c)) / k
    s = 1.0 / mean if (mean > 0.0 and np.isfinite(mean)) else 0.0
    v = stability_rows(xyz, normals, idx, c, s)
    Cm = np.array([[math.fsum(v[:, i] * v[:, j]) for j in range(6)] for i in range(6)])
    lam = np.linalg.eigvalsh(Cm)[::-1]
    rank = int((lam > EIG_CUT * lam[0]).sum()) if s > 0.0 else 0
    cond = float("inf") if (s == 0.0 or not lam[5] > 0.0) else lam[0] / lam[5]
    return {"n_used": k, "centroid": c, "scale": s, "C": Cm, "eigenvalues": lam, "rank": rank, "cond": cond}


# ------------------------------------------------------------------------------------------------ fixtures
def grooved_plane(ns):
    """x, y on linspace(-1, 1, ns)^2; two V-grooves at x = 0.3 and y = -0.2, half-width 0.1, depth 0.05."""
    x, y = np.meshgrid(np.linspace(-1.0, 1.0, ns), np.linspace(-1.0, 1.0, ns), indexing="ij")
    x, y = x.reshape(-1), y.reshape(-1)

    def g(u):
        return np.where(np.abs(u) < 0.1, -0.05 * (1.0 - np.abs(u) / 0.1), 0.0)

    def dg(u):
        return np.where(np.abs(u) < 0.1, 0.5 * np.sign(u), 0.0)

    z = g(x - 0.3) + g(y + 0.2)
    nrm = np.stack([-dg(x - 0.3), -dg(y + 0.2), np.ones_like(x)], axis=1)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return np.stack([x, y, z], axis=1).astype(np.float32), nrm.astype(np.float32)


def shape(name):
    """(xyz, normals, expected rank)"""
    rng = np.random.default_rng(11)
    if name == "plane":
        u, v = np.meshgrid(np.linspace(-1, 1, 8), np.linspace(-1, 1, 8), indexing="ij")
        p = np.stack([u.reshape(-1), v.reshape(-1), np.zeros(64)], axis=1)
        return p.astype(np.float32), np.tile(np.float32([0, 0, 1]), (64, 1)), 3
    if name == "sphere":
        d = rng.normal(size=(2000, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        return (np.array([0.3, -0.2, 0.5]) + 1.5 * d).astype(np.float32), d.astype(np.float32), 3
    if name == "cylinder":
        th, z = rng.uniform(0, 2 * np.pi, 2000), rng.uniform(-1, 1, 2000)
        d = np.stack([np.cos(th), np.sin(th), np.zeros(2000)], axis=1)
        return (d + np.stack([np.zeros(2000), np.zeros(2000), z], axis=1)).astype(np.float32), d.astype(np.float32), 4
    if name == "patches":
        u, v = np.meshgrid(np.linspace(0.2, 1.0, 20), np.linspace(0.2, 1.0, 20), indexing="ij")
        u, v, o = u.reshape(-1), v.reshape(-1), np.zeros(400)
        p = np.concatenate([np.stack([u, v, o], 1), np.stack([o, u, v], 1), np.stack([u, o, v], 1)])
        nrm = np.concatenate([np.tile([0.0, 0, 1], (400, 1)), np.tile([1.0, 0, 0], (400, 1)), np.tile([0.0, 1, 0], (400, 1))])
        return p.astype(np.float32), nrm.astype(np.float32), 6
    raise KeyError(name)


SHAPES = ["plane", "sphere", "cylinder", "patches"]


def odd_rows():
    """Normals that take no part, or whose bin hangs on a detail: -0.0, denormal, NaN, inf, zero, huge."""
    tiny = np.float32(1e-40)
    return np.array([[np.nan, 0, 1], [0, np.inf, 0], [-np.inf, 1, 1], [0, 0, 0], [0, -0.0, 0], [-0.0, 1, 0], [1, -0.0, -0.0],
                     [tiny, 0, 0], [tiny, -tiny, tiny], [0, 0, -tiny], [3e38, 1, 1], [-3e38, 3e38, 3e38], [1, np.nan, np.nan]], np.float32)


def random_normals(n, seed=0, odd=True):
    rng = np.random.default_rng(1000 + n + seed)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    nrm[: n // 3] *= np.float32([0.2, 0.2, 1.0])                    # a crowded pole: bins far above the level beside nearly empty ones
    if odd and n >= 63:
        rows = odd_rows()
        nrm[rng.choice(n, len(rows), replace=False)] = rows
    return nrm


def border_normals():
    """Axis ties and cell borders: (1, 1, 0), (1, 1, 1), (-1, 1, 1) in every order and sign; components like (4, 1, -2), whose
    (u + 1) * 4 is a whole number."""
    rows = []
    for base in ([1, 1, 0], [1, 1, 1], [-1, 1, 1], [4, 1, -2], [4, 3, 0], [8, -5, 7], [4, -4, 2], [2, 1, 1], [4, -1, -3]):
        for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)):
            for sx in (1, -1):
                for sy in (1, -1):
                    for sz in (1, -1):
                        rows.append([base[perm[0]] * sx, base[perm[1]] * sy, base[perm[2]] * sz])
    return np.array(rows, np.float32)


def same_sample(got, ref):
    assert np.array_equal(got["idx"], ref["idx"]), (got["idx"][:8], ref["idx"][:8])
    assert got["idx"].dtype == np.int64 and got["bin"].dtype == np.int32
    assert np.array_equal(got["bin"], ref["bin"]), np.flatnonzero(got["bin"] != ref["bin"])[:8]
    for k, v in ref["report"].items():
        assert got["report"][k] == v, (k, got["report"][k], v)


def cond_of(xyz, normals, idx):
    return stability_numpy(xyz, normals, idx)["cond"]


# ------------------------------------------------------------------------------------------------ CPU tests
def test_symbols_structs_and_settings(built):
    from object_alignment_amd import _capi
    from object_alignment_amd.operators import IcpSettings
    header = open(os.path.join(ROOT, "include", "oa_icp.h")).read()
    L = _capi.load()
    for name in ("oa_normal_space_sample", "oa_stability"):
        assert name in _capi.SYMBOLS and hasattr(L, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
    assert C.sizeof(_capi.SampleReport) == 48 and _capi.SampleReport.total_ms.offset == 40
    S = _capi.StabilityReport
    assert C.sizeof(S) == 8 + 24 + 8 + 288 + 48 + 288 + 8 + 8 + 8
    assert (S.centroid.offset, S.scale.offset, S.C.offset, S.eigenvalues.offset, S.eigenvectors.offset) == (8, 32, 40, 328, 376)
    assert (S.rank.offset, S.cond.offset, S.total_ms.offset) == (664, 672, 680)
    for struct, cname in ((_capi.SampleReport, "oa_sample_report"), (S, "oa_stability_report")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
        declared = re.findall(r"\b([A-Za-z_]+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert declared == [f for f, _ in struct._fields_], declared
    assert C.sizeof(_capi.Settings) == 32 and C.sizeof(_capi.Report) == 72
    assert os.path.exists(os.path.join(ROOT, "object_alignment_amd", "csrc", "oa_sample.hpp"))
    s = IcpSettings()
    assert s.sample_normal_space == 0 and s.sample_normal_grid == 8


def test_argument_errors_before_any_engine_opens(monkeypatch):
    import object_alignment_amd as oa
    from object_alignment_amd import engine as eng_mod
    from object_alignment_amd.operators import IcpAlign, IcpSettings

    def no_engine(*a, **k):
        raise AssertionError("an engine was opened")

    monkeypatch.setattr(eng_mod.IcpEngine, "__init__", no_engine)
    xyz, nrm = grooved_plane(8)
    for bad_m in (0, -3, 1.5, None, True, "4"):
        with pytest.raises(ValueError):
            oa.normal_space_sample(nrm, bad_m)
    for bad_grid in (0, 33, -1, 8.0, None, True):
        with pytest.raises(ValueError):
            oa.normal_space_sample(nrm, 4, grid=bad_grid)
    for bad_seed in (-1, 2 ** 32, 0.5):
        with pytest.raises(ValueError):
            oa.normal_space_sample(nrm, 4, seed=bad_seed)
    for bad_rows in (nrm[:, :2], nrm.reshape(-1), nrm[:0], np.array([["a", "b", "c"]])):
        with pytest.raises(ValueError):
            oa.normal_space_sample(bad_rows, 4)
        with pytest.raises(ValueError):
            oa.stability(xyz, bad_rows)
        with pytest.raises(ValueError):
            oa.stability(bad_rows, nrm)
    for bad_idx in ([], [-1], [len(xyz)], [0.5], [[0, 1]]):
        with pytest.raises(ValueError):
            oa.stability(xyz, nrm, idx=bad_idx)
    e = object.__new__(eng_mod.IcpEngine)                             # the argument checks need no context
    e._h = None
    with pytest.raises(ValueError):
        e.normal_space_sample(nrm, 0)
    with pytest.raises(ValueError):
        e.stability(xyz, nrm[:5])
    eye = np.identity(4, dtype=np.float32)
    for field, bad in (("sample_normal_space", -1), ("sample_normal_space", 2.5), ("sample_normal_space", True), ("sample_normal_grid", 0),
                       ("sample_normal_grid", 33), ("sample_normal_grid", 4.0)):
        with pytest.raises(ValueError):
            IcpAlign(IcpSettings(**{"sample_normal_space": 10, field: bad}), engine=e).run(xyz, xyz, eye, eye, source_normals=nrm)
    # the setting on and no normals to sample
    with pytest.raises(ValueError, match="source_normals"):
        IcpAlign(IcpSettings(sample_normal_space=10), engine=e).run(xyz, xyz, eye, eye)


@pytest.mark.parametrize("ns", [72, 120])
def test_fixture_guard_grooved_plane(ns):
    """The restatement alone: 300 distinct indices, and the sample's 6 x 6 system is conditioned at least twice as well as that of
    an every-k-th sample of the same size (measured: 9.1 against 52.4 at 72 x 72, 6.9 against 49.1 at 120 x 120)."""
    xyz, nrm = grooved_plane(ns)
    N, m = len(xyz), 300
    pick = nss_numpy(nrm, m, G=8, unoriented=False, seed=0)["idx"]
    assert len(pick) == m == len(np.unique(pick))
    uniform = np.arange(0, N, N // m)[:m]
    c_nss, c_uni = cond_of(xyz, nrm, pick), cond_of(xyz, nrm, uniform)
    print("grooved plane %d x %d: cond %.1f (normal space) against %.1f (every k-th)" % (ns, ns, c_nss, c_uni))
    assert c_nss <= 0.5 * c_uni, (c_nss, c_uni)


@pytest.mark.parametrize("name", SHAPES)
def test_fixture_guard_ranks(name):
    xyz, nrm, rank = shape(name)
    assert stability_numpy(xyz, nrm)["rank"] == rank


def test_restatement_shares():
    """The share rule on counts small enough to do by hand: c = (5, 1, 3), m = 6 -> level 2 gives 2 + 1 + 2 = 5, the remainder 1
    goes to the first bin above the level."""
    nrm = np.float32([[1, 0, 0]] * 5 + [[-1, 0, 0]] + [[0, 1, 0]] * 3)
    ref = nss_numpy(nrm, 6, G=1)
    assert ref["report"]["level"] == 2 and ref["remainder"] == 1 and ref["report"]["bins_occupied"] == 3
    assert np.bincount(ref["bin"][ref["idx"]], minlength=3).tolist() == [3, 1, 2]
    assert nss_numpy(nrm, 100, G=1)["report"]["level"] == 5 and len(nss_numpy(nrm, 100, G=1)["idx"]) == 9


# ------------------------------------------------------------------------------------------------ GPU: the sample
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, SORT_SMALL_MAX, SORT_SMALL_MAX + 1, 20000])
def test_sample_equals_the_restatement(eng, n):
    nrm = random_normals(n)
    n_el = int((bins_numpy(nrm) >= 0).sum())
    ms = {1, max(1, n - 1), n, n + 5, max(1, n_el - 1), n_el}
    with_remainder = [m for m in range(max(1, n // 3), max(1, n // 3) + 64) if m < n_el and nss_numpy(nrm, m)["remainder"] > 0][:1]
    assert with_remainder or n < 63
    for m in sorted(ms | set(with_remainder)):
        ref = nss_numpy(nrm, m)
        got = eng.normal_space_sample(nrm, m)
        same_sample(got, ref)
        assert len(got["idx"]) == min(m, n_el)


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 8, 32])
@pytest.mark.parametrize("unoriented", [False, True])
def test_sample_grids_borders_and_signs(eng, G, unoriented):
    rows = border_normals()
    nrm = np.concatenate([rows, random_normals(700, seed=G), -rows, odd_rows()])
    for m, seed in ((1, 0), (len(nrm) // 4, 0), (len(nrm) // 4 + 7, 0xDEADBEEF), (len(nrm), 5)):
        same_sample(eng.normal_space_sample(nrm, m, grid=G, unoriented=unoriented, seed=seed), nss_numpy(nrm, m, G, unoriented, seed))
    if unoriented:
        b = eng.normal_space_sample(nrm, 1, grid=G, unoriented=True)["bin"]
        assert np.array_equal(b[: len(rows)], b[len(rows) + 700: 2 * len(rows) + 700])     # n and -n share a bin
        assert b.max() < 3 * G * G


@pytest.mark.gpu
def test_sample_one_bin_repeats_and_device_input(eng):
    import torch
    same = np.tile(np.float32([0.1, -0.7, 0.3]), (9000, 1))
    for m in (1, 17, 8999, 9000, 9005):
        same_sample(eng.normal_space_sample(same, m, seed=3), nss_numpy(same, m, seed=3))
    nrm = random_normals(20000, seed=1)
    a = eng.normal_space_sample(nrm, 5000, seed=9)
    b = eng.normal_space_sample(nrm, 5000, seed=9)
    d = eng.normal_space_sample(torch.from_numpy(nrm).cuda(), 5000, seed=9)
    for other in (b, d):
        assert np.array_equal(a["idx"], other["idx"]) and np.array_equal(a["bin"], other["bin"])
        assert {k: v for k, v in a["report"].items() if k != "total_ms"} == {k: v for k, v in other["report"].items() if k != "total_ms"}
    assert not np.array_equal(a["idx"], eng.normal_space_sample(nrm, 5000, seed=10)["idx"])


@pytest.mark.gpu
def test_sample_refusals(eng, built):
    from object_alignment_amd import _capi
    L = _capi.load()
    nrm = random_normals(100)
    ip = _capi.iptr
    out, got, rep = np.zeros(100, np.int64), C.c_int64(0), _capi.SampleReport()

    def call(n=100, m=10, grid=8, cap=100, rows=nrm):
        return L.oa_normal_space_sample(eng._h, C.c_void_p(rows.ctypes.data), n, 0, m, grid, 0, 0, cap, ip(out), None, C.byref(got), C.byref(rep))

    assert call() == _capi.OA_OK and got.value == 10
    for kw in (dict(m=0), dict(m=-1), dict(grid=0), dict(grid=33), dict(n=0), dict(n=2 ** 31 - 2 ** 20 + 1)):
        assert call(**kw) == _capi.OA_E_BAD_ARG, kw
    dead = np.zeros((100, 3), np.float32)
    dead[::2] = np.nan
    assert call(rows=dead) == _capi.OA_E_BAD_ARG and rep.n_eligible == 0 and rep.n_in == 100
    before = out.copy()
    assert call(m=50, cap=49) == _capi.OA_E_CAPACITY
    assert got.value == 50 and rep.n_eligible == nss_numpy(nrm, 50)["report"]["n_eligible"] and np.array_equal(out, before)
    from object_alignment_amd.engine import IcpEngine
    with IcpEngine(devices=[0, 0]) as multi:
        with pytest.raises(_capi.OaError) as ei:
            multi.normal_space_sample(nrm, 10)
        assert ei.value.code == _capi.OA_E_STATE
        with pytest.raises(_capi.OaError) as ei:
            multi.stability(nrm, nrm)
        assert ei.value.code == _capi.OA_E_STATE


# ------------------------------------------------------------------------------------------------ GPU: the stability report
def check_stability(got, xyz, nrm, idx=None):
    """C, centroid and scale against exactly rounded sums.  A sum of k fp64 terms, added in ANY order, is off by at most
    gamma_k sum |term| with gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability, 4.2); the terms themselves are restated
    bit for bit (IEEE products, differences, one division and one square root each), from the centroid and scale the library
    reports.  One more rounding (u times the result) where a division follows the sum."""
    p = used_rows(xyz, nrm, idx)[0]
    k = len(p)
    gamma = k * U / (1.0 - k * U)
    assert got["n_used"] == k
    for a in range(3):
        exact = math.fsum(p[:, a]) / k
        assert abs(got["centroid"][a] - exact) <= gamma * np.abs(p[:, a]).sum() / k + 2 * U * abs(exact), (a, got["centroid"][a], exact)
    c = got["centroid"]
    dist = mean_distance(p, c)
    mean = math.fsum(dist) / k
    if mean > 0.0:
        assert abs(1.0 / got["scale"] - mean) <= (gamma + 4 * U) * mean, (got["scale"], 1.0 / mean)
    else:
        assert got["scale"] == 0.0
    v = stability_rows(xyz, nrm, idx, c, got["scale"])
    for i in range(6):
        for j in range(6):
            t = v[:, i] * v[:, j]
            assert abs(got["C"][i, j] - math.fsum(t)) <= gamma * np.abs(t).sum(), (i, j, got["C"][i, j], math.fsum(t))
    assert np.array_equal(got["C"], got["C"].T)
    # The eigen-decomposition: at most 32 sweeps of 15 Jacobi rotations; one rotation replaces two rows and two columns by
    # c a -+ s b with c, s each a few roundings off an exact rotation -- a relative perturbation of at most 8 u of the matrix and
    # of the accumulated vectors per rotation, 32 * 15 * 8 u = 3840 u in all (first order); what the sweeps leave off the diagonal
    # is below 1e-18 of it; the check's own products add 6 u per entry.  4000 u covers the three.
    tol = 4000 * U
    Cm, X, lam = got["C"], got["eigenvectors"], got["eigenvalues"]
    norm = np.linalg.norm(Cm)
    assert np.linalg.norm(Cm @ X - X * lam[None, :]) <= tol * norm
    assert np.linalg.norm(X.T @ X - np.identity(6)) <= tol
    assert np.all(np.diff(lam) <= 0.0)
    assert np.abs(lam - np.linalg.eigvalsh(Cm)[::-1]).max() <= tol * norm        # (Weyl: a residual bounds the eigenvalues' distance)
    for kcol in range(6):
        col = X[:, kcol]
        assert col[int(np.argmax(np.abs(col)))] > 0.0                # (argmax: the lowest index on ties)
    if got["scale"] > 0.0:
        assert got["rank"] == int((lam > EIG_CUT * lam[0]).sum())
        assert got["cond"] == (lam[0] / lam[5] if lam[5] > 0.0 else float("inf"))
    else:
        assert got["rank"] == 0 and got["cond"] == float("inf")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHAPES)
def test_stability_on_shapes(eng, name):
    xyz, nrm, rank = shape(name)
    got = eng.stability(xyz, nrm)
    check_stability(got, xyz, nrm)
    assert got["rank"] == rank == stability_numpy(xyz, nrm)["rank"]
    again = eng.stability(xyz, nrm)
    for key in ("C", "eigenvalues", "eigenvectors", "centroid"):
        assert np.array_equal(got[key], again[key]), key
    assert (got["scale"], got["rank"], got["cond"], got["n_used"]) == (again["scale"], again["rank"], again["cond"], again["n_used"])


@pytest.mark.gpu
def test_stability_selections_sizes_and_device_input(eng):
    import torch
    xyz, nrm = grooved_plane(72)
    ref = nss_numpy(nrm, 300)
    pick = ref["idx"]
    by_idx = eng.stability(xyz, nrm, idx=pick)
    direct = eng.stability(xyz[pick], nrm[pick])
    on_dev = eng.stability(torch.from_numpy(xyz).cuda(), torch.from_numpy(nrm).cuda(), idx=pick)
    for other in (direct, on_dev):
        for key in ("C", "eigenvalues", "eigenvectors", "centroid"):
            assert np.array_equal(by_idx[key], other[key]), key
        assert (by_idx["scale"], by_idx["rank"], by_idx["cond"]) == (other["scale"], other["rank"], other["cond"])
    check_stability(by_idx, xyz, nrm, pick)
    assert by_idx["rank"] == 6 and by_idx["cond"] <= 0.5 * eng.stability(xyz, nrm, idx=np.arange(0, len(xyz), len(xyz) // 300)[:300])["cond"]
    # more than one workgroup, more partials than one wave's lanes, rows that take no part, a point listed twice
    rng = np.random.default_rng(5)
    n = 256 * 70 + 3
    big_xyz = rng.normal(size=(n, 3)).astype(np.float32) * np.float32([3.0, 1.0, 0.2]) + np.float32([10.0, -4.0, 0.5])
    big_nrm = random_normals(n, seed=2)
    big_xyz[7] = np.nan
    big_xyz[300, 1] = np.inf
    check_stability(eng.stability(big_xyz, big_nrm), big_xyz, big_nrm)
    twice = np.concatenate([np.arange(0, n, 3), [9, 9, 12]])
    check_stability(eng.stability(big_xyz, big_nrm, idx=twice), big_xyz, big_nrm, twice)


@pytest.mark.gpu
def test_stability_degenerate_inputs(eng):
    from object_alignment_amd import _capi
    one = eng.stability(np.float32([[1, 2, 3]]), np.float32([[0, 0, 2]]))
    assert one["n_used"] == 1 and one["rank"] == 0 and one["scale"] == 0.0 and one["cond"] == float("inf")
    assert np.array_equal(one["centroid"], [1.0, 2.0, 3.0])
    check_stability(one, np.float32([[1, 2, 3]]), np.float32([[0, 0, 2]]))
    same = np.tile(np.float32([0.5, -1.25, 2.0]), (500, 1))
    nrm = random_normals(500, odd=False)
    got = eng.stability(same, nrm)
    assert got["rank"] == 0 and got["scale"] == 0.0 and got["n_used"] == 500 and np.array_equal(got["centroid"], [0.5, -1.25, 2.0])
    check_stability(got, same, nrm)
    with pytest.raises(_capi.OaError) as ei:
        eng.stability(same, np.zeros_like(same))
    assert ei.value.code == _capi.OA_E_BAD_ARG


# ------------------------------------------------------------------------------------------------ GPU: through the operator
@pytest.mark.gpu
def test_sample_normal_space_through_the_operator(eng):
    from object_alignment_amd import synth
    from object_alignment_amd.operators import IcpAlign, IcpSettings
    xyz, nrm = grooved_plane(72)
    mxa = synth.rigid4(synth.rotation_from_rotvec([0.0, 0.0, np.radians(1.0)]), [0.02, 0.02, 0.0])
    eye = np.identity(4, dtype=np.float32)
    kw = dict(target_normals=nrm, source_normals=nrm)
    base = dict(metric="plane", icp_iterations=15, min_start=0.5)
    on = IcpAlign(IcpSettings(sample_normal_space=300, **base), engine=eng)
    res = on.run(xyz, xyz, mxa, eye, **kw)
    cand = np.arange(0, len(xyz), round(1 / IcpSettings().sample_fraction))      # what the loop would have used
    pick = cand[nss_numpy(nrm[cand], 300)["idx"]]
    assert np.array_equal(on.last_sampling["idx"], pick) and len(pick) == 300
    assert on.last_sampling["report"]["n_eligible"] == len(cand)
    assert on.last_sampling["stability"]["rank"] == 6 and on.last_sampling["stability"]["n_used"] == 300
    by_hand = IcpAlign(IcpSettings(sample_fraction=1.0, **base), engine=eng)
    ref = by_hand.run(xyz, xyz, mxa, eye, vlist=pick, **kw)
    assert by_hand.last_sampling is None
    assert np.array_equal(res.matrix_world, ref.matrix_world) and res.iters_done == ref.iters_done and res.last_K == ref.last_K
    # a vlist, a voxel grid and sample_fraction in front of it: still the candidates the loop would have used
    from object_alignment_amd.operators.icp_align import voxel_vlist
    vl = np.arange(100, len(xyz) - 100)
    on2 = IcpAlign(IcpSettings(sample_normal_space=200, sample_normal_grid=4, sample_voxel=0.06, sample_fraction=0.34, **base), engine=eng)
    on2.run(xyz, xyz, mxa, eye, vlist=vl, **kw)
    thinned = voxel_vlist(eng, xyz, vl, mxa, 0.06)
    cand2 = thinned[::3]
    assert 200 < len(cand2) and len(thinned) < len(vl) // 2 and on2.last_sampling["report"]["n_in"] == len(cand2)
    assert np.array_equal(on2.last_sampling["idx"], cand2[nss_numpy(nrm[cand2], 200, G=4)["idx"]])
    # the setting off: the same result as ever, twice
    off1 = IcpAlign(IcpSettings(**base), engine=eng)
    off2 = IcpAlign(IcpSettings(**base), engine=eng)
    r1, r2 = off1.run(xyz, xyz, mxa, eye, **kw), off2.run(xyz, xyz, mxa, eye, **kw)
    assert off1.last_sampling is None and off2.last_sampling is None
    assert np.array_equal(r1.matrix_world, r2.matrix_world) and r1.last_K == r2.last_K
