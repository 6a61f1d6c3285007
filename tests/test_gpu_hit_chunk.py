"""k_nn_search_sorted's hit path (round 17): a chunk of 16 vertices that level 0v lets through is scored at level 1 in ONE pass -- its
12 tile reads together, the four groups' minima kept, one test and one branch per chunk -- and a lane enters levels 2-3 for a group
whose stored minimum is not above its thr2 as it stands then.  That may only change the SPEED: an unseeded and then a seeded search
(a second search after a small pose change) must give the oracle's brute force bit for bit (index and d^2), and what the
OA_NN_VCHUNK=0 instances (no chunks at all: every group of a hit block on its own) give.  OA_NN_R=4 throughout -- sources this small
would otherwise run one point per lane --, both tile sizes.  The shapes are the smallest that can break it: vertex counts around
the block (256) and tile (1024) boundaries and more than one tile (the padded last block, a block's position 0, a one-block target),
source sizes that leave lanes, waves and point pairs partly empty, a target on one v (every chunk passes level 0v: level 1 decides
everything), duplicated vertices (ties on the distance: the lowest ORIGINAL index wins, whatever group it sits in), points exactly on
vertices (best = 0, the thresholds at their floor) and non-finite points (NaN passes every filter and wins nothing).
Every problem and its oracle answers are built once and shared by all configurations."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_TARGET = [255, 256, 257, 1023, 1025, 4100]
N_SOURCE = [1, 128, 129, 300]
EYE = np.identity(4, dtype=np.float32)


def _pose(scale):
    m = EYE.copy()
    m[:3, 3] = np.float32(0.01 * scale)
    return m


def _special(case, rng):
    """(target, source, pose of the seeded search) in float64; the caller rounds to float32"""
    if case in ("one_v", "one_v_nearly"):
        # u = x; y is the same for every vertex and z the same (one_v) or within 1e-6 of it (one_v_nearly: z is then v): no chunk's
        # ends can rule a nearby point out
        nt = 1025
        tgt = np.stack([rng.uniform(-2, 2, size=nt), np.full(nt, 0.25), np.full(nt, -0.5)], axis=1)
        if case == "one_v_nearly":
            tgt[:, 2] += rng.uniform(-1e-6, 1e-6, size=nt)
        src = tgt[rng.integers(0, nt, size=300)] + rng.normal(0, 2e-2, size=(300, 3))
        return tgt, src, _pose(1.0)
    if case == "duplicate_vertices":
        # every vertex four times, far apart in the original order; points on the mirror plane of two distinct vertices as well
        base = rng.uniform(-1, 1, size=(300, 3)) * [2.0, 1.0, 0.5]
        tgt = np.tile(base, (4, 1))[rng.permutation(1200)]
        src = base[rng.integers(0, 300, size=300)] + rng.normal(0, 3e-3, size=(300, 3))
        src[::5] = base[rng.integers(0, 300, size=60)]
        return tgt, src, _pose(0.5)
    if case == "duplicates_in_one_chunk":
        # blocks of ONE u and chunks of ONE v: 16 copies of a vertex fill a chunk, the copies' original indices in a random order
        # over its four groups -- the group order decides the tie
        base = np.stack([np.repeat(np.arange(5), 16) * 1.0, np.tile(np.arange(16), 5) / 16.0, np.zeros(80)], axis=1)
        tgt = np.repeat(base, 16, axis=0)[rng.permutation(1280)]
        src = base[rng.integers(0, 80, size=300)] + rng.normal(0, 1e-2, size=(300, 3))
        return tgt, src, _pose(0.3)
    if case == "on_a_vertex":                                       # best = 0 from the first hit on; nothing moves between the searches
        tgt = rng.uniform(-1, 1, size=(1025, 3)) * [2.0, 1.0, 0.5]
        return tgt, tgt[rng.permutation(1025)[:300]].copy(), EYE.copy()
    if case == "on_a_vertex_then_moved":
        tgt = rng.uniform(-1, 1, size=(4100, 3)) * [2.0, 1.0, 0.5]
        return tgt, tgt[rng.permutation(4100)[:129]].copy(), _pose(1.0)
    if case == "non_finite_points":
        tgt = rng.uniform(-1, 1, size=(1025, 3)) * [2.0, 1.0, 0.5]
        src = tgt[rng.integers(0, 1025, size=300)] + rng.normal(0, 5e-3, size=(300, 3))
        src[0::7] = np.nan
        src[1::7, 1] = np.nan                                       # (v alone)
        src[2::7, 0] = 1e30                                         # (finite, its square is not)
        src[3::7, 2] = np.inf
        return tgt, src, _pose(1.0)
    raise KeyError(case)


SPECIAL = ["one_v", "one_v_nearly", "duplicate_vertices", "duplicates_in_one_chunk", "on_a_vertex", "on_a_vertex_then_moved",
           "non_finite_points"]


def _moved(orc, m, src):
    return np.array([orc.mat4_mul_vec3(m, p) for p in src], np.float32)


def _with_answers(orc, name, tgt, src, m, thresh=1e30):
    tgt, src = np.ascontiguousarray(tgt, np.float32), np.ascontiguousarray(src, np.float32)
    with np.errstate(all="ignore"):
        first = orc.nn_brute(src, tgt)
        second = first if np.array_equal(m, EYE) else orc.nn_brute(_moved(orc, m, src), tgt)
    return name, tgt, src, m, thresh, first, second


@functools.lru_cache(maxsize=None)
def _problems(orc):
    """every fixed problem with the oracle's answers, once for both tile sizes: (name, target, source, pose, threshold, (idx, d2), (idx, d2))"""
    out = []
    for nt in N_TARGET:
        for ns in N_SOURCE:
            rng = np.random.default_rng(1700 * nt + ns)
            tgt = rng.uniform(-1, 1, size=(nt, 3)) * [2.0, 1.0, 0.5]
            src = rng.uniform(-1, 1, size=(ns, 3)) * [2.2, 1.0, 0.5]
            near = (ns + 1) // 2                                    # half the points beside a vertex: short reaches, few chunks each
            src[:near] = tgt[rng.integers(0, nt, size=near)] + rng.normal(0, 2e-3, size=(near, 3))
            out.append(_with_answers(orc, "nt_%d_ns_%d" % (nt, ns), tgt, src, _pose(1.0)))
    for i, case in enumerate(SPECIAL):
        tgt, src, m = _special(case, np.random.default_rng(1717 + i))
        out.append(_with_answers(orc, case, tgt, src, m))
    return out


@functools.lru_cache(maxsize=None)
def _fuzz_problems(orc):
    """200 random small seeded problems: sizes, extents, offsets, flat and duplicated targets, poses and which seeds survive at random"""
    rng = np.random.default_rng(20261020)
    out = []
    for trial in range(200):
        nt, ns = int(rng.integers(2, 2001)), int(rng.integers(1, 601))
        scale = 10.0 ** rng.uniform(-4, 4)
        tgt = rng.uniform(-1, 1, size=(nt, 3)) * 10.0 ** rng.uniform(-3, 0, size=3)
        if trial % 3 == 0:
            tgt = tgt[rng.integers(0, nt, size=nt)]                 # duplicates: ties on the distance
        if trial % 5 == 0:
            tgt[:, int(rng.integers(0, 3))] = np.round(tgt[:, int(rng.integers(0, 3))] * 8) / 8   # a quantised axis: chunks of one v
        src = tgt[rng.integers(0, nt, size=ns)] + rng.normal(0, 10.0 ** rng.uniform(-6, -1), size=(ns, 3))
        if trial % 7 == 0:
            src[:: 3] = tgt[rng.integers(0, nt, size=len(src[::3]))]   # on a vertex
        off = rng.uniform(-1, 1, size=3) * (10.0 ** rng.uniform(-2, 2) if trial % 2 else 0.0)
        m = _pose(scale * 10.0 ** rng.uniform(-3, 0)) if trial % 4 else EYE.copy()
        thresh = 1e30 if trial % 3 else scale * 10.0 ** rng.uniform(-5, -1)   # some seeds rejected: an unseeded point beside seeded ones
        out.append(_with_answers(orc, "trial_%d" % trial, (tgt + off) * scale, (src + off) * scale, m, thresh))
    return out


def _search_twice(e, tgt, src, m, thresh=1e30):
    """an unseeded search at the identity, then one seeded from its pairs (those within thresh) at pose m"""
    e.set_target(tgt)
    e.set_source(src)
    e.set_matrices(EYE, EYE)
    first = e.nn_search()[:2]
    assert e.stat("brute_kernel") == 3.0
    e.make_pairs(thresh)                                             # winner records = seeds
    e.set_matrices(m, EYE)
    second = e.nn_search()[:2]
    return first, second


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


def _engines(monkeypatch, bigtile):
    """the chunked hit path (OA_NN_VCHUNK=1) and the instances without chunks (0), four points per lane, one tile size"""
    from object_alignment_amd.engine import IcpEngine
    monkeypatch.setenv("OA_NN_R", "4")
    monkeypatch.setenv("OA_NN_BIGTILE", bigtile)
    out = []
    for vchunk in ("1", "0"):
        monkeypatch.setenv("OA_NN_VCHUNK", vchunk)
        e = IcpEngine(0)
        e.set_search_mode("brute")
        out.append(e)
    return out


def _check(problems, chunked, plain):
    for name, tgt, src, m, thresh, ref1, ref2 in problems:
        got1, got2 = _search_twice(chunked, tgt, src, m, thresh)
        assert _same(got1, ref1), (name, "unseeded")
        assert _same(got2, ref2), (name, "seeded")
        old1, old2 = _search_twice(plain, tgt, src, m, thresh)
        assert _same(got1, old1) and _same(got2, old2), (name, "OA_NN_VCHUNK=0")


@pytest.mark.parametrize("bigtile", ["0", "1"])
def test_hit_chunk_answers_are_the_oracles(orc, bigtile, monkeypatch):
    chunked, plain = _engines(monkeypatch, bigtile)
    with chunked, plain:
        _check(_problems(orc), chunked, plain)


@pytest.mark.parametrize("bigtile", ["0", "1"])
def test_hit_chunk_fuzz(orc, bigtile, monkeypatch):
    chunked, plain = _engines(monkeypatch, bigtile)
    with chunked, plain:
        _check(_fuzz_problems(orc), chunked, plain)
