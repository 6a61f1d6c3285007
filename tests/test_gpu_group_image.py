"""k_nn_search_sorted's level 0 on images of V = 16 (or 8, at build time) sorted positions (round 19, group_image in csrc/oa_octgap.hpp): V
consecutive positions of the final order are tested through one {mm, ww, ws} -- every one of them within ws of mm + ww or mm - ww
-- under the target's cap c, a lane's points (2p, 2p + 1) through {hm, hw' = max(hw, c)}, with the chain and the threshold of round
18.  That may only change the SPEED: an unseeded and then a seeded search must give the oracle's brute force bit for bit (index and
d^2), and what OA_NN_VCHUNK=0 (single gaps per point and vertex) gives.  Unseeded and seeded, OA_NN_R=4 and 2, both tile sizes, both
slot orders (with OA_SORT_SOURCE=0 and OA_NN_WAVE_ORDER=0 slot i pairs with slot i ^ 64).

The shapes are the smallest at which an image, a chunk of 16 or a block of 256 can go wrong: every vertex count 1 .. 17 and those
around 32, 64, 256, 256 + 8, 256 + 16 and 1024; source sizes around a wave, a workgroup and a block of slots.  Level 0's hit is
decided per block of 256 positions, and a seed's own image keeps its block, so random problems alone rarely depend on one image:
the directed cases do.
  outlier_last_image_*   every chunk of 16 positions is fifteen vertices at u = k and one at k + 0.6, the last position of the chunk
                         (v grows with the position, so the block's order by v keeps it there).  A lane's point starts at 15.85
                         (nearest: u = 16, in block 1, at 0.15) and moves to 15.70: the seed is 0.3 away, the answer is the vertex
                         at 15.6 -- the last position of block 0, 0.6 beyond the rest of its image -- at 0.1.  Its image stands on
                         {15, 15.3} and reaches it only through ws = 0.3: with ws taken from the image's first half, t = 0.4 > thr1
                         and block 0 is pruned.  _wide: the lane's other point is 17 chunks away (hw = 8.5 > c = 7.9, e = 0);
                         _coincident: it is 1e-4 away (hw' = c, e = c - hw in the threshold).
  lattice_points_share_u u on levels 1.0 apart, a block per level (ww = ws = 0 everywhere), both points of a lane on vertices of one
                         level and then moved by 0.03 along every axis: t = |0.03 - c| = 0.44 > thr1 on the own level's images, only
                         e in the threshold keeps the block that holds the answer.
  last_block_lone_vertex 257, 265 and 273 vertices: the last block's last image is one vertex + padding, and points sit beside the
                         vertices of that block.
  tiny_target_*          3 and 5 vertices (the cap is 43 and 26 extents: every lane is on hw' = c) and 256 (c is half the extent),
                         points from two extents below the cloud to two above.
Every problem and its oracle answers are built once and shared by all configurations.  Then ~300 small seeded random problems at
R = 4, and the call order that builds the images inside an open sequence of iterations, once behind another target's smaller cap.
profiles/r19a_vertex_octets.txt says which of these caught which of two deliberately wrong builds."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = list(range(1, 18)) + [31, 32, 33, 63, 64, 65, 255, 256, 257, 263, 264, 265, 271, 272, 273, 1023, 1024, 1025]
N_SOURCE = [1, 63, 64, 65, 128, 255, 256, 257, 1024, 1025]
# (OA_NN_BIGTILE, OA_NN_R)
CONFIGS = [(b, r) for b in ("0", "1") for r in (4, 2)]
EYE = np.identity(4, dtype=np.float32)
NS = 256                                                            # a wave of four points per lane, two waves of two: whole pairs


def _pose(shift):
    m = EYE.copy()
    m[:3, 3] = np.float32(shift)
    return m


def _paired(a, b):
    """the source whose slot order pairs a[k] with b[k] (runs of 64 of a and of b alternate: slot i pairs with slot i ^ 64)"""
    n = len(a)
    assert n == len(b) and n % 64 == 0
    return np.stack([a.reshape(n // 64, 64, 3), b.reshape(n // 64, 64, 3)], axis=1).reshape(2 * n, 3)


def _special(case, rng):
    """(target, source, pose of the seeded search) in float64; the caller rounds to float32 and shuffles the target's rows"""
    h = NS // 2
    if case.startswith("outlier_last_image"):
        nt = 640                                                    # 40 chunks, two and a half blocks; c = 39.6 * 128 / 640 = 7.92
        i = np.arange(nt)
        tgt = np.stack([i // 16 + 0.6 * (i % 16 == 15), i / 10000.0, np.zeros(nt)], axis=1)
        jit = rng.uniform(0, 1e-5, size=h)
        du = rng.uniform(-0.02, 0.02, size=h)                       # (0.08 .. 0.12 from the answer, 0.28 .. 0.32 from the seed)
        a = np.stack([15.85 + du, 0.0255 + jit, np.zeros(h)], axis=1)
        if case.endswith("wide"):
            b = np.stack([32.85 + du, 0.0527 + jit, np.zeros(h)], axis=1)
        else:
            b = a + [1e-4, 0.0, 0.0]
        m = EYE.copy()
        m[0, 3] = np.float32(-0.15)
        return tgt, _paired(a, b), m
    if case == "lattice_points_share_u":
        nt = 1540                                                   # six levels and four vertices of a seventh; c = 0.5
        i = np.arange(nt)
        tgt = np.stack([(i // 256) * 1.0, ((i % 256) // 16) * 0.02, (i % 16) * 0.02], axis=1)
        k = rng.integers(0, nt // 256, size=h)
        pick = lambda: np.stack([k * 1.0, rng.integers(0, 15, size=h) * 0.02, rng.integers(0, 15, size=h) * 0.02], axis=1)
        return tgt, _paired(pick(), pick()), _pose(0.03)
    if case.startswith("last_block_lone_vertex"):
        nt = int(case.rsplit("_", 1)[1])
        tgt = rng.uniform(0, 1, size=(nt, 3)) * [4.0, 1.0, 0.1]
        top = np.argsort(tgt[:, 0])[-24:]                           # the last block's vertices and their neighbours in u
        src = tgt[top[rng.integers(0, 24, size=NS)]] + rng.normal(0, 2e-3, size=(NS, 3))
        return tgt, src, _pose(0.004)
    if case.startswith("tiny_target"):
        nt = int(case.rsplit("_", 1)[1])
        tgt = rng.uniform(0, 1, size=(nt, 3)) * [2.0, 1.0, 0.1]
        src = rng.uniform(-2, 3, size=(NS, 3)) * [2.0, 1.0, 0.1]
        src[::2] = tgt[rng.integers(0, nt, size=NS // 2)] + rng.normal(0, 1e-3, size=(NS // 2, 3))
        return tgt, src, _pose(0.02)
    raise KeyError(case)


SPECIAL = ["outlier_last_image_wide", "outlier_last_image_coincident", "lattice_points_share_u", "last_block_lone_vertex_257",
           "last_block_lone_vertex_265", "last_block_lone_vertex_273", "tiny_target_3", "tiny_target_5", "tiny_target_256"]


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
            tgt = rng.uniform(-1, 1, size=(nt, 3)) * [2.0, 1.0, 0.05]
            src = rng.uniform(-1, 1, size=(ns, 3)) * [2.2, 1.0, 0.05]
            src[: ns // 2] = tgt[rng.integers(0, nt, size=ns // 2)] + rng.normal(0, 2e-3, size=(ns // 2, 3))
            out.append(_with_answers(orc, "nt_%d_ns_%d" % (nt, ns), tgt, src, _pose(0.01)))
    for i, case in enumerate(SPECIAL):
        rng = np.random.default_rng(1919 + i)
        tgt, src, m = _special(case, rng)
        tgt = tgt[rng.permutation(len(tgt))]                        # original indices are not the sorted positions
        out.append(_with_answers(orc, case, tgt, src, m))
    return out


def _search_twice(e, tgt, src, m, thresh=1e30):
    """an unseeded search at the identity, then one seeded from its pairs (those within thresh) at pose m"""
    e.set_target(tgt)
    e.set_source(src)
    e.set_matrices(EYE, EYE)
    first = e.nn_search()[:2]
    if len(tgt) >= 2:
        assert e.stat("brute_kernel") == 3.0
    e.make_pairs(thresh)                                             # winner records = seeds
    e.set_matrices(m, EYE)
    second = e.nn_search()[:2]
    return first, second


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


def _engines(monkeypatch):
    """the kernel that folds the images (OA_NN_VCHUNK=1) and the single gaps (0), under whatever else the environment says"""
    from object_alignment_amd.engine import IcpEngine
    out = []
    for vchunk in ("1", "0"):
        monkeypatch.setenv("OA_NN_VCHUNK", vchunk)
        e = IcpEngine(0)
        e.set_search_mode("brute")
        out.append(e)
    return out


@pytest.mark.parametrize("own_order", [False, True])
@pytest.mark.parametrize("bigtile,R", CONFIGS)
def test_group_image_level0_answers_are_the_oracles(orc, bigtile, R, own_order, monkeypatch):
    monkeypatch.setenv("OA_NN_BIGTILE", bigtile)
    monkeypatch.setenv("OA_NN_R", str(R))
    if own_order:                                                    # the test's order of points is the lanes': slot i pairs with i ^ 64
        monkeypatch.setenv("OA_SORT_SOURCE", "0")
        monkeypatch.setenv("OA_NN_WAVE_ORDER", "0")
    images, plain = _engines(monkeypatch)
    with images, plain:
        for name, tgt, src, m, ref1, ref2 in _problems(orc):
            got1, got2 = _search_twice(images, tgt, src, m)
            assert _same(got1, ref1), (name, "unseeded")
            assert _same(got2, ref2), (name, "seeded")
            old1, old2 = _search_twice(plain, tgt, src, m)
            assert _same(got1, old1) and _same(got2, old2), (name, "OA_NN_VCHUNK=0")


def test_group_image_level0_fuzz(orc, monkeypatch):
    """~300 random small seeded problems at four points per lane: sizes, extents, offsets, duplicated vertices and points, runs of
    vertices that share their u but for one (an outlier inside an image), poses and which seeds survive at random"""
    monkeypatch.setenv("OA_NN_R", "4")
    rng = np.random.default_rng(20261019)
    images, plain = _engines(monkeypatch)
    with images, plain:
        for trial in range(300):
            nt, ns = int(rng.integers(2, 1300)), int(rng.integers(1, 400))
            scale = 10.0 ** rng.uniform(-6, 6)
            tgt = rng.uniform(-1, 1, size=(nt, 3)) * 10.0 ** rng.uniform(-3, 0, size=3)
            if trial % 3 == 0:
                tgt = tgt[rng.integers(0, nt, size=nt)]                # duplicates: images of width zero, ties on the distance
            if trial % 5 == 0:
                ax = int(rng.integers(0, 3))
                tgt[:, ax] = np.round(tgt[:, ax] * 8) / 8               # a quantised axis: whole images on one level ...
                out = rng.integers(0, nt, size=1 + nt // 16)
                tgt[out, ax] += rng.uniform(0, 0.1, size=len(out))      # ... but for an outlier here and there
            if trial % 11 == 0:
                tgt[rng.integers(0, nt, size=1 + nt // 50)] += rng.uniform(-1, 1, size=3) * 30.0      # an outlier cluster: capped images
            src = tgt[rng.integers(0, nt, size=ns)] + rng.normal(0, 10.0 ** rng.uniform(-6, -1), size=(ns, 3))
            if trial % 7 == 0:
                src = src[rng.integers(0, ns, size=ns)]                # duplicated points: Hw = 0
            off = rng.uniform(-1, 1, size=3) * (10.0 ** rng.uniform(-2, 3) if trial % 2 else 0.0)
            tgt, src = ((tgt + off) * scale).astype(np.float32), ((src + off) * scale).astype(np.float32)
            m = _pose(0.01 * scale * 10.0 ** rng.uniform(-3, 0)) if trial % 4 else EYE.copy()
            thresh = 1e30 if trial % 3 else scale * 10.0 ** rng.uniform(-5, -1)   # some seeds rejected: thr1 = +inf beside a seeded partner
            got1, got2 = _search_twice(images, tgt, src, m, thresh)
            ref1 = orc.nn_brute(src, tgt)
            ref2 = ref1 if np.array_equal(m, EYE) else orc.nn_brute(_moved(orc, m, src), tgt)
            assert _same(got1, ref1), (trial, "unseeded")
            assert _same(got2, ref2), (trial, "seeded")
            old1, old2 = _search_twice(plain, tgt, src, m, thresh)
            assert _same(got1, old1) and _same(got2, old2), (trial, "OA_NN_VCHUNK=0")


@pytest.mark.parametrize("R", [4, 2])
@pytest.mark.parametrize("earlier_target", [False, True])
def test_group_images_built_inside_an_open_sequence(orc, R, earlier_target, monkeypatch):
    """The sorted images may be built while a sequence of iterations is open: a target uploaded for the automatic search, one
    iteration, oa_set_search_mode(brute) -- which builds the images and their cap there and then --, the next iteration through
    k_nn_search_sorted.  The set-up must take the cap those images were built with, not one staged before they existed (0 on a fresh
    context; with earlier_target, what a brute-force search on the same cloud at a sixteenth of the size left behind: a smaller
    cap).  The second iteration's pair count and distance statistics are the oracle's at the pose the first one reached (sums of <=
    256 doubles: 1e-8 relative, the tolerance the loop's statistics are held to elsewhere; one wrong neighbour moves the mean by 1e-6
    or more)."""
    from object_alignment_amd.engine import IcpEngine
    monkeypatch.setenv("OA_NN_R", str(R))
    monkeypatch.setenv("OA_SORT_SOURCE", "0")
    monkeypatch.setenv("OA_NN_WAVE_ORDER", "0")
    problems = {p[0]: p for p in _problems(orc)}
    with IcpEngine(0) as e:
        for name in ("outlier_last_image_wide", "outlier_last_image_coincident", "lattice_points_share_u", "last_block_lone_vertex_265"):
            _, tgt, src, m, _, _ = problems[name]
            if earlier_target:
                e.set_search_mode("brute")
                e.set_target(np.ascontiguousarray(tgt * np.float32(0.0625)))   # the same cloud at a sixteenth of the size: a sixteenth of the cap
                e.set_source(src)
                e.set_matrices(EYE, EYE)
                e.nn_search()
            e.set_search_mode("auto")
            e.set_target(tgt)
            e.set_source(src)
            e.set_matrices(m, EYE)
            e.iterate(thresh=10.0, target_d=1e-9)
            m1 = e.matrix_world()
            e.set_search_mode("brute")                               # builds the images; the sequence stays open
            _, st = e.iterate(thresh=10.0, target_d=1e-9)
            assert e.stat("brute_kernel") == 3.0, name
            A, _, ds = orc.make_pairs(src, tgt, m1, EYE, 10.0, calc_stats=True)
            assert st["K"] == A.shape[1], name
            assert np.isclose(st["mean_dist"], ds[0], rtol=1e-8, atol=0.0) and np.isclose(st["std_dist"], ds[1], rtol=1e-8, atol=1e-12), (name, st, ds)
