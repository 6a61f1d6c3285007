"""k_nn_search_sorted's level 0 on PAIRS of vertices (round 11, csrc/oa_pairgap.hpp): positions (4g, 4g+1) and (4g+2, 4g+3) of the
sorted order are tested through their midpoint and half-width, | |m - hu| - w | = the smaller of the two gaps.  That may only
change the SPEED: an unseeded and then a seeded search must give the oracle's brute force bit for bit (index and d^2), and what
OA_NN_VCHUNK=0 (the single gaps of before) gives.  The shapes are the smallest that can break it: odd vertex counts (a vertex paired
with padding), the block (256) and tile (1024) boundaries, pairs of width zero, a point on a vertex / on its pair's midpoint /
between two mirror-symmetric vertices (lowest original index wins), offsets and scales that stress the midpoint's rounding, a seed
that already is the answer (the threshold at its tightest).  Every problem and its oracle answers are built once and shared by all
configurations."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 5, 7, 9, 255, 256, 257, 1023, 1025]
N_SOURCE = [300, 1500]
# (OA_NN_BIGTILE, OA_NN_R, OA_NN_SPLITS or 0)
CONFIGS = [(b, r, 0) for b in ("0", "1") for r in (1, 2, 4)] + [("0", 4, 7)]
EYE = np.identity(4, dtype=np.float32)


def _pose(scale):
    m = EYE.copy()
    m[:3, 3] = np.float32(0.01 * scale)
    return m


def _ordered_target(nt):
    """vertex i: u = i / 64 (dyadic: midpoints are exact), the two vertices of a pair share v = (i // 2) / 1024 and d = 0, so the sorted order is
    the index order (u rises; within a block v rises with it) and the pairs are (2k, 2k + 1)"""
    i = np.arange(nt)
    return np.stack([i / 64.0, (i // 2) / 1024.0, np.zeros(nt)], axis=1)


def _special(case, rng):
    """(target, source, pose of the seeded search) in float64; the caller rounds to float32 and shuffles the target's rows"""
    nt = 2048 + 5                                                   # 9 tiles of 256 vertices: OA_NN_SPLITS=7 is really 7 splits
    if case == "blocks_of_one_u":                                   # every block on one u: every pair has w = 0
        tgt = rng.uniform(-0.4, 0.4, size=(nt, 3))
        tgt[:, 0] = (np.arange(nt) // 256) * 1.0
        src = rng.uniform(-0.5, 0.5, size=(1500, 3))
        src[:, 0] = rng.uniform(-1.0, 9.0, size=1500)
        return tgt, src, _pose(1.0)
    if case == "one_point":                                         # all vertices the same point: no extent at all
        tgt = np.tile([[0.25, -0.5, 0.125]], (41, 1))
        return tgt, rng.uniform(-1, 1, size=(300, 3)), _pose(1.0)
    if case == "point_on_vertex":
        tgt = rng.uniform(-1, 1, size=(nt, 3))
        return tgt, tgt[rng.permutation(nt)[:1500]].copy(), _pose(1.0)
    if case == "point_on_midpoint":                                 # |m - hu| = 0: a = w exactly, the real gap
        tgt = _ordered_target(nt)
        k = rng.integers(0, nt // 2, size=1500)
        src = np.stack([(2 * k + 0.5) / 64.0, k / 1024.0 + rng.integers(-2, 3, size=1500) / 4096.0, rng.integers(-2, 3, size=1500) / 4096.0], axis=1)
        src[::3, 0] = (2 * k[::3] + 1.5) / 64.0                     # ... and midway between two pairs
        return tgt, src, _pose(1.0)
    if case == "mirror_vertices":                                   # equal distances to both vertices of a pair: the lowest ORIGINAL index
        tgt = _ordered_target(nt)
        k = rng.integers(0, nt // 2, size=1500)
        src = np.stack([(2 * k + 0.5) / 64.0, k / 1024.0, rng.integers(-3, 4, size=1500) / 2048.0], axis=1)
        return tgt, src, EYE.copy()
    if case == "offset_1e4":                                        # spacing 1e-3 at 1e4: an ulp of float32 there is 9.8e-4
        g = np.stack(np.meshgrid(np.arange(13), np.arange(13), np.arange(13), indexing="ij"), axis=-1).reshape(-1, 3)
        tgt = 1.0e4 + 1.0e-3 * g * [3.0, 1.0, 1.0]
        src = 1.0e4 + 1.0e-3 * rng.uniform(-1, 14, size=(1500, 3)) * [3.0, 1.0, 1.0]
        return tgt, src, _pose(1.0e-2)
    if case in ("scale_1e-18", "scale_1e15"):
        s = float(case[6:])
        tgt = rng.uniform(-1, 1, size=(nt, 3)) * s
        src = (tgt[rng.permutation(nt)[:1500]] + rng.normal(0, 0.01 * s, size=(1500, 3)))
        return tgt, src, _pose(s)
    if case == "seed_is_the_answer":                                # nothing moves between the two searches
        tgt = rng.uniform(-1, 1, size=(nt, 3))
        src = tgt[rng.permutation(nt)[:1500]] + rng.normal(0, 4e-3, size=(1500, 3))
        src[::4] = tgt[rng.permutation(nt)[:len(src[::4])]]        # ... and best = 0
        return tgt, src, EYE.copy()
    raise KeyError(case)


SPECIAL = ["blocks_of_one_u", "one_point", "point_on_vertex", "point_on_midpoint", "mirror_vertices", "offset_1e4", "scale_1e-18",
           "scale_1e15", "seed_is_the_answer"]


def _moved(orc, m, src):
    return np.array([orc.mat4_mul_vec3(m, p) for p in src], np.float32)


def _with_answers(orc, name, tgt, src, m):
    tgt, src = np.ascontiguousarray(tgt, np.float32), np.ascontiguousarray(src, np.float32)
    first = orc.nn_brute(src, tgt)
    second = first if np.array_equal(m, EYE) else orc.nn_brute(_moved(orc, m, src), tgt)
    return name, tgt, src, m, first, second


@functools.lru_cache(maxsize=None)
def _problems(orc):
    """every problem with the oracle's answers, once for all configurations: (name, target, source, pose, (idx, d2), (idx, d2))"""
    out = []
    for nt in SIZES:
        for ns in N_SOURCE:
            rng = np.random.default_rng(1000 * nt + ns)
            tgt = rng.uniform(-1, 1, size=(nt, 3)) * [2.0, 1.0, 0.5]
            src = rng.uniform(-1, 1, size=(ns, 3)) * [2.2, 1.0, 0.5]
            src[: ns // 3] = tgt[rng.integers(0, nt, size=ns // 3)] + rng.normal(0, 2e-3, size=(ns // 3, 3))
            out.append(_with_answers(orc, "nt_%d_ns_%d" % (nt, ns), tgt, src, _pose(1.0)))
    for i, case in enumerate(SPECIAL):
        rng = np.random.default_rng(77 + i)
        tgt, src, m = _special(case, rng)
        tgt = tgt[rng.permutation(len(tgt))]                        # original indices are not the sorted positions
        out.append(_with_answers(orc, case, tgt, src, m))
    return out


def _search_twice(e, tgt, src, m):
    """an unseeded search at the identity, then one seeded from its pairs at pose m"""
    e.set_target(tgt)
    e.set_source(src)
    e.set_matrices(EYE, EYE)
    first = e.nn_search()[:2]
    if len(tgt) >= 2:
        assert e.stat("brute_kernel") == 3.0
    e.make_pairs(1e30)                                               # winner records = seeds
    e.set_matrices(m, EYE)
    second = e.nn_search()[:2]
    return first, second


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _engines(monkeypatch):
    """the pair kernel (OA_NN_VCHUNK=1) and the single gaps it replaced (0), under whatever else the environment says"""
    from object_alignment_amd.engine import IcpEngine
    out = []
    for vchunk in ("1", "0"):
        monkeypatch.setenv("OA_NN_VCHUNK", vchunk)
        e = IcpEngine(0)
        e.set_search_mode("brute")
        out.append(e)
    return out


@pytest.mark.parametrize("bigtile,R,splits", CONFIGS)
def test_pair_level0_answers_are_the_oracles(orc, bigtile, R, splits, monkeypatch):
    monkeypatch.setenv("OA_NN_BIGTILE", bigtile)
    monkeypatch.setenv("OA_NN_R", str(R))
    if splits:
        monkeypatch.setenv("OA_NN_SPLITS", str(splits))
    pairs, plain = _engines(monkeypatch)
    with pairs, plain:
        for name, tgt, src, m, ref1, ref2 in _problems(orc):
            got1, got2 = _search_twice(pairs, tgt, src, m)
            assert _same(got1, ref1), (name, "unseeded")
            assert _same(got2, ref2), (name, "seeded")
            old1, old2 = _search_twice(plain, tgt, src, m)
            assert _same(got1, old1) and _same(got2, old2), (name, "OA_NN_VCHUNK=0")


def test_pair_level0_fuzz(orc, monkeypatch):
    """a few hundred random small problems: sizes, extents, offsets, duplicated vertices and poses at random"""
    rng = np.random.default_rng(20261019)
    pairs, plain = _engines(monkeypatch)
    with pairs, plain:
        for trial in range(300):
            nt, ns = int(rng.integers(2, 700)), int(rng.integers(1, 400))
            scale = 10.0 ** rng.uniform(-6, 6)
            tgt = rng.uniform(-1, 1, size=(nt, 3)) * 10.0 ** rng.uniform(-3, 0, size=3)
            if trial % 3 == 0:
                tgt = tgt[rng.integers(0, nt, size=nt)]                # duplicates: pairs of width zero, ties on the distance
            if trial % 5 == 0:
                tgt[:, int(rng.integers(0, 3))] = np.round(tgt[:, int(rng.integers(0, 3))] * 8) / 8   # a quantised axis
            src = tgt[rng.integers(0, nt, size=ns)] + rng.normal(0, 10.0 ** rng.uniform(-6, -1), size=(ns, 3))
            off = rng.uniform(-1, 1, size=3) * (10.0 ** rng.uniform(-2, 3) if trial % 2 else 0.0)
            tgt, src = ((tgt + off) * scale).astype(np.float32), ((src + off) * scale).astype(np.float32)
            m = _pose(scale * 10.0 ** rng.uniform(-3, 0)) if trial % 4 else EYE.copy()
            got1, got2 = _search_twice(pairs, tgt, src, m)
            ref1 = orc.nn_brute(src, tgt)
            ref2 = ref1 if np.array_equal(m, EYE) else orc.nn_brute(_moved(orc, m, src), tgt)
            assert _same(got1, ref1), (trial, "unseeded")
            assert _same(got2, ref2), (trial, "seeded")
            old1, old2 = _search_twice(plain, tgt, src, m)
            assert _same(got1, old1) and _same(got2, old2), (trial, "OA_NN_VCHUNK=0")
