"""k_nn_search_sorted's level 0 on QUADS of vertices and pairs of a lane's points (round 18, csrc/oa_octgap.hpp): a group of four
sorted positions is tested through {mm, ww, ws} under the target's cap c, a lane's points (2p, 2p + 1) through {hm, hw' = max(hw, c)},
t = |||mm - hm| - hw'| - ww| - ws <= the smallest of the eight gaps + e, against one threshold that holds e.  That may only change
the SPEED: an unseeded and then a seeded search must give the oracle's brute force bit for bit (index and d^2), and what
OA_NN_VCHUNK=0 (single gaps per point and vertex) gives.  Unseeded and seeded, OA_NN_R=4 and 2, both tile sizes, both slot orders
(with OA_SORT_SOURCE=0 and OA_NN_WAVE_ORDER=0 slot i pairs with slot i ^ 64).  The shapes: vertex counts around the quad, block (256)
and tile (1024) boundaries and 4100 (17 blocks: the cap is then a thirty-second of the extent and level 0 really prunes); source
sizes that pair real slots with padding.  The special inputs are the ones the cap's two sides and the wider-pair rule decide: a
lattice target (WW = w = 0) under points that share their u (every lane on hw' = c: leaving e out of the threshold prunes the
block that holds the answer), groups of a pair of width zero and a wide one under points that move onto the wide pair's far end
(ws = min(wa, wb) prunes the group that holds the answer), flat random targets under tight seeds, an outlier cluster inside the last
block (quads capped, WW > c), a non-finite point, an offset of 1000 extents.  Every problem and its oracle answers are built once and
shared by all configurations.  Last, the call order that builds the images inside an open sequence of iterations."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 5, 255, 256, 257, 1023, 1025, 4100]
N_SOURCE = [1, 2, 63, 128, 129, 300]
# (OA_NN_BIGTILE, OA_NN_R)
CONFIGS = [(b, r) for b in ("0", "1") for r in (4, 2)]
EYE = np.identity(4, dtype=np.float32)
NT = 4100                                                           # 17 blocks of 256 (the last one 4 vertices + padding)
NS = 1024                                                           # four runs of 256 slots: every lane of them holds two whole pairs


def _pose(shift):
    m = EYE.copy()
    m[:3, 3] = np.float32(shift)
    return m


def _paired(a, b):
    """the source whose slot order pairs a[k] with b[k] (runs of 64 of a and of b alternate: slot i pairs with slot i ^ 64)"""
    n = len(a)
    assert n == len(b) and n % 64 == 0
    return np.stack([a.reshape(n // 64, 64, 3), b.reshape(n // 64, 64, 3)], axis=1).reshape(2 * n, 3)


def _lattice(nt):
    """u on levels 1.0 apart, 256 vertices per level on a 16 x 16 grid of spacing 0.02 in (v, d): every block of the sorted order is
    one level -- every pair and every quad has width zero, and the cap is about 0.47 of a level"""
    i = np.arange(nt)
    return np.stack([(i // 256) * 1.0, ((i % 256) // 16) * 0.02, (i % 16) * 0.02], axis=1)


def _special(case, rng):
    """(target, source, pose of the seeded search, make_pairs threshold) in float64; the caller rounds to float32 and shuffles the
    target's rows"""
    h = NS // 2
    if case == "lattice_points_share_u":
        # both points of a lane ON vertices of one level, then moved by 0.03 along every axis: the nearest vertex is the diagonal
        # neighbour, the seed (distance 0.052) is stale, the own level's quads give t = |0.03 - c| = 0.44 > thr1: only e keeps the block
        tgt = _lattice(NT)
        k = rng.integers(0, NT // 256, size=h)
        pick = lambda: np.stack([k * 1.0, rng.integers(0, 15, size=h) * 0.02, rng.integers(0, 15, size=h) * 0.02], axis=1)
        return tgt, _paired(pick(), pick()), _pose(0.03), 1e30
    if case == "lattice_random_points":
        tgt = _lattice(NT)
        src = rng.uniform(-0.5, 16.5, size=(NS, 3)) * [1.0, 0.02, 0.02]
        return tgt, src, _pose(0.013), 1e30
    if case == "flat_target_tight_seeds":
        # nearest-neighbour distances (0.02) far below the quads' widths (up to the cap, 0.125): which vertex of a quad is the
        # nearest, the wider pair's far end included, decides
        tgt = rng.uniform(0, 1, size=(NT, 3)) * [4.0, 1.0, 0.0]
        src = tgt[rng.permutation(NT)[:NS]] + rng.normal(0, 2e-3, size=(NS, 3)) * [1.0, 1.0, 0.0]
        return tgt, src, _pose(0.011), 1e30
    if case == "flat_target_wide_point_pairs":
        # ... with every lane's two points at least a cap apart along u (hw' = hw, e = 0: nothing but ws stands for the widths)
        tgt = rng.uniform(0, 1, size=(NT, 3)) * [4.0, 1.0, 0.0]
        p = rng.permutation(NT)
        a = tgt[p[:h]] + rng.normal(0, 2e-3, size=(h, 3)) * [1.0, 1.0, 0.0]
        b = tgt[p[h:2 * h]] + rng.normal(0, 2e-3, size=(h, 3)) * [1.0, 1.0, 0.0]
        return tgt, _paired(a, b), _pose(0.011), 1e30
    if case == "far_end_of_the_wider_pair":
        # group k of the order is u = k, k, k, k + 0.6 (v = k / 1000 keeps it together): a pair of width zero and one of half-width
        # 0.3, the quad's image stands on {k, k + 0.3}.  A lane's points start at k + 0.85 and k + 65.85 (hw = 32.5 > c = 31.9: e = 0;
        # nearest: k + 1 at 0.15) and then move -0.15 along u: the seed is 0.3 away, the nearest vertex is k + 0.6 at 0.1, BEYOND the
        # image, and its group's t is 0.1 only with ws = 0.3 -- 0.4 > thr1 with ws = 0.  k = 63 is the LAST group of a block of 256
        # vertices: the seed's group, which no bound can rule out, is in the next block and does not carry this one to level 0v.
        # 130 groups only: thr1 also carries 2^-20 of the cloud's squared extent, 0.33 here
        nt, ka = 520, np.full(h, 63)
        k = np.arange(nt) // 4
        tgt = np.stack([k + 0.6 * (np.arange(nt) % 4 == 3), k / 1000.0, np.zeros(nt)], axis=1)
        a = np.stack([ka + 0.85, ka / 1000.0, np.zeros(h)], axis=1)
        b = np.stack([ka + 65.85, (ka + 65) / 1000.0, np.zeros(h)], axis=1)
        m = EYE.copy()
        m[0, 3] = np.float32(-0.15)
        return tgt, _paired(a, b), m, 1e30
    if case == "outlier_cluster_in_the_last_block":
        # 40 vertices ten extents away share the last whole block with 216 of the cloud's: its quads' pairs lie 18 apart, WW > c
        tgt = rng.uniform(0, 1, size=(NT, 3)) * [4.0, 1.0, 0.2]
        far = rng.permutation(NT)[:40]
        tgt[far] = rng.uniform(0, 1, size=(40, 3)) * [1.0, 1.0, 0.2] + [40.0, 0.0, 0.0]
        src = tgt[rng.permutation(NT)[:NS]] + rng.normal(0, 5e-3, size=(NS, 3))
        src[:128] = rng.uniform(0, 1, size=(128, 3)) * [50.0, 1.0, 0.2]            # ... and points in the gap and beyond
        return tgt, src, _pose(0.02), 1e30
    if case == "non_finite_points":
        tgt = rng.uniform(0, 1, size=(NT, 3)) * [4.0, 1.0, 0.2]
        a = tgt[rng.permutation(NT)[:h]] + rng.normal(0, 5e-3, size=(h, 3))
        b = a[rng.permutation(h)].copy()
        b[0::3] = np.nan
        b[1::3, 0] = 1e30                                           # (finite, its square is not)
        b[2::96, 0] = np.inf
        return tgt, _paired(a, b), _pose(0.01), 1e30
    if case == "offset_1000_extents":
        tgt = rng.uniform(0, 1, size=(NT, 3)) * [4.0, 1.0, 0.2] + 4000.0
        src = tgt[rng.permutation(NT)[:NS]] + rng.normal(0, 5e-3, size=(NS, 3))
        return tgt, src, _pose(0.01), 1e30
    if case == "seeded_partner_unseeded":                           # make_pairs rejects b's pairs: thr1 = +inf beside a tight one
        tgt = rng.uniform(0, 1, size=(NT, 3)) * [4.0, 1.0, 0.0]
        a = tgt[rng.permutation(NT)[:h]] + rng.normal(0, 2e-3, size=(h, 3))
        b = rng.uniform(0, 1, size=(h, 3)) * [4.0, 1.0, 0.0] + [0.0, 0.0, 0.8]
        return tgt, _paired(a, b), _pose(0.004), 0.1
    raise KeyError(case)


SPECIAL = ["lattice_points_share_u", "lattice_random_points", "flat_target_tight_seeds", "flat_target_wide_point_pairs",
           "far_end_of_the_wider_pair", "outlier_cluster_in_the_last_block", "non_finite_points", "offset_1000_extents", "seeded_partner_unseeded"]


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
    """every problem with the oracle's answers, once for all configurations: (name, target, source, pose, threshold, (idx, d2), (idx, d2))"""
    out = []
    for nt in SIZES:
        for ns in N_SOURCE:
            rng = np.random.default_rng(1000 * nt + ns)
            tgt = rng.uniform(-1, 1, size=(nt, 3)) * [2.0, 1.0, 0.05]
            src = rng.uniform(-1, 1, size=(ns, 3)) * [2.2, 1.0, 0.05]
            src[: ns // 2] = tgt[rng.integers(0, nt, size=ns // 2)] + rng.normal(0, 2e-3, size=(ns // 2, 3))
            out.append(_with_answers(orc, "nt_%d_ns_%d" % (nt, ns), tgt, src, _pose(0.01)))
    for i, case in enumerate(SPECIAL):
        rng = np.random.default_rng(1877 + i)
        tgt, src, m, thresh = _special(case, rng)
        tgt = tgt[rng.permutation(len(tgt))]                        # original indices are not the sorted positions
        out.append(_with_answers(orc, case, tgt, src, m, thresh))
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
    """the quad kernel (OA_NN_VCHUNK=1) and the single gaps (0), under whatever else the environment says"""
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
def test_vertex_quad_level0_answers_are_the_oracles(orc, bigtile, R, own_order, monkeypatch):
    monkeypatch.setenv("OA_NN_BIGTILE", bigtile)
    monkeypatch.setenv("OA_NN_R", str(R))
    if own_order:                                                    # the test's order of points is the lanes': slot i pairs with i ^ 64
        monkeypatch.setenv("OA_SORT_SOURCE", "0")
        monkeypatch.setenv("OA_NN_WAVE_ORDER", "0")
    quads, plain = _engines(monkeypatch)
    with quads, plain:
        for name, tgt, src, m, thresh, ref1, ref2 in _problems(orc):
            got1, got2 = _search_twice(quads, tgt, src, m, thresh)
            assert _same(got1, ref1), (name, "unseeded")
            assert _same(got2, ref2), (name, "seeded")
            old1, old2 = _search_twice(plain, tgt, src, m, thresh)
            assert _same(got1, old1) and _same(got2, old2), (name, "OA_NN_VCHUNK=0")


def test_vertex_quad_level0_fuzz(orc, monkeypatch):
    """a few hundred random small seeded problems: sizes, extents, offsets, duplicated vertices and points, poses and which seeds
    survive at random; four points per lane (two pairs), which sources this small would not get by themselves"""
    monkeypatch.setenv("OA_NN_R", "4")
    rng = np.random.default_rng(20261020)
    quads, plain = _engines(monkeypatch)
    with quads, plain:
        for trial in range(300):
            nt, ns = int(rng.integers(2, 2600)), int(rng.integers(1, 600))
            scale = 10.0 ** rng.uniform(-6, 6)
            tgt = rng.uniform(-1, 1, size=(nt, 3)) * 10.0 ** rng.uniform(-3, 0, size=3)
            if trial % 3 == 0:
                tgt = tgt[rng.integers(0, nt, size=nt)]                # duplicates: quads of width zero, ties on the distance
            if trial % 5 == 0:
                tgt[:, int(rng.integers(0, 3))] = np.round(tgt[:, int(rng.integers(0, 3))] * 8) / 8   # a quantised axis
            if trial % 11 == 0:
                tgt[rng.integers(0, nt, size=1 + nt // 50)] += rng.uniform(-1, 1, size=3) * 30.0      # an outlier cluster: capped quads
            src = tgt[rng.integers(0, nt, size=ns)] + rng.normal(0, 10.0 ** rng.uniform(-6, -1), size=(ns, 3))
            if trial % 7 == 0:
                src = src[rng.integers(0, ns, size=ns)]                # duplicated points: Hw = 0
            off = rng.uniform(-1, 1, size=3) * (10.0 ** rng.uniform(-2, 3) if trial % 2 else 0.0)
            tgt, src = ((tgt + off) * scale).astype(np.float32), ((src + off) * scale).astype(np.float32)
            m = _pose(0.01 * scale * 10.0 ** rng.uniform(-3, 0)) if trial % 4 else EYE.copy()
            thresh = 1e30 if trial % 3 else scale * 10.0 ** rng.uniform(-5, -1)   # some seeds rejected: thr1 = +inf beside a seeded partner
            got1, got2 = _search_twice(quads, tgt, src, m, thresh)
            ref1 = orc.nn_brute(src, tgt)
            ref2 = ref1 if np.array_equal(m, EYE) else orc.nn_brute(_moved(orc, m, src), tgt)
            assert _same(got1, ref1), (trial, "unseeded")
            assert _same(got2, ref2), (trial, "seeded")
            old1, old2 = _search_twice(plain, tgt, src, m, thresh)
            assert _same(got1, old1) and _same(got2, old2), (trial, "OA_NN_VCHUNK=0")


@pytest.mark.parametrize("R", [4, 2])
@pytest.mark.parametrize("earlier_target", [False, True])
def test_images_built_inside_an_open_sequence(orc, R, earlier_target, monkeypatch):
    """The sorted images may be built while a sequence of iterations is open: a target uploaded for the automatic search, one
    iteration, oa_set_search_mode(brute) -- which builds the quad images and their cap there and then --, the next iteration through
    k_nn_search_sorted.  The set-up must take the cap those images were built with, not one staged before they existed (0 on a fresh
    context; with earlier_target, what a brute-force search on the same cloud at a sixteenth of the size left behind).  The second iteration's
    pair count and distance statistics are the oracle's at the pose the first one reached (sums of <= 1024 doubles: 1e-8 relative,
    the tolerance the loop's statistics are held to elsewhere; one wrong neighbour moves the mean by 1e-6 or more)."""
    from object_alignment_amd.engine import IcpEngine
    monkeypatch.setenv("OA_NN_R", str(R))
    monkeypatch.setenv("OA_SORT_SOURCE", "0")
    monkeypatch.setenv("OA_NN_WAVE_ORDER", "0")
    problems = {p[0]: p for p in _problems(orc)}
    with IcpEngine(0) as e:
        for name in ("lattice_points_share_u", "flat_target_tight_seeds", "far_end_of_the_wider_pair", "outlier_cluster_in_the_last_block"):
            _, tgt, src, m, _, _, _ = problems[name]
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
            with np.errstate(all="ignore"):
                A, _, ds = orc.make_pairs(src, tgt, m1, EYE, 10.0, calc_stats=True)
            assert st["K"] == A.shape[1], name
            assert np.isclose(st["mean_dist"], ds[0], rtol=1e-8, atol=0.0) and np.isclose(st["std_dist"], ds[1], rtol=1e-8, atol=1e-12), (name, st, ds)
