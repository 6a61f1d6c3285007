"""k_nn_search_sorted's level 0v from the ends of each chunk (OA_NN_VCHUNK=1): positions 1 .. 255 of a block of sorted vertices
are in the order of v, so a chunk whose two ends are both farther than thr1 along v on the same side of the point is ruled out.
That may only change the SPEED: every answer must stay the oracle's brute force, bit for bit.  The targets are built so that
the sorted order is known: vertex i has u = i / 256 + small, so block b holds vertices 256 b .. 256 b + 255 and vertex 256 b is
its position 0 (kept in place, out of v order).  The cases: many equal v values, a position 0 far from its block's v range,
the padded last block, points whose v falls exactly on a chunk's end or between two chunks -- each unseeded and seeded, at
1 / 2 / 4 points per thread, in both tile sizes, with the work queue and without.  A CPU check pins the bound itself."""
import zlib

import numpy as np
import pytest

CASES = ["equal_v", "far_position0", "padded_tail", "chunk_ends", "between_chunks"]


def _slabs(case, rng):
    """(target, source) float32: blocks of 256 along u, v values laid out per chunk of 16 sorted positions"""
    nb = 24
    nt = 256 * nb + (77 if case == "padded_tail" else 0)
    i = np.arange(nt)
    u = (i // 256) * 1.0 + (i % 256) * (0.5 / 256)                # strictly rising: the sorted order is the index order
    if case == "equal_v":
        v = rng.integers(0, 3, size=nt) * 0.5                      # three values of v shared by every block
    else:
        # sorted position j of a block: v = chunk + 0.01 (j mod 16), gaps of 0.85 between chunks; shuffled per block so that
        # the sort by v has work to do
        j = np.arange(256)
        vs = (j // 16) * 1.0 + (j % 16) * 0.01
        v = np.concatenate([rng.permutation(vs) for _ in range((nt + 255) // 256)])[:nt]
    d = rng.normal(0, 0.02, size=nt)
    if case == "far_position0":
        v[::256] = 40.0 + rng.uniform(0, 1, size=len(v[::256]))   # each block's position 0 far above the rest of its block
    tgt = np.stack([u, v, d * 0.1], axis=1)
    tgt[:, 1] *= 0.5                                                # extents: u the longest axis, then v, then d
    b = rng.integers(0, (nt + 255) // 256, size=6000)
    su = b * 1.0 + rng.uniform(0, 0.5, size=len(b))
    if case == "far_position0":
        k = rng.integers(0, 2, size=len(b))                        # half the points next to a block's position 0
        sv = np.where(k == 1, v[np.minimum(256 * b, nt - 1)], rng.uniform(0, 16, size=len(b)))
        su = np.where(k == 1, u[np.minimum(256 * b, nt - 1)] + rng.normal(0, 1e-3, size=len(b)), su)
    elif case == "padded_tail":
        b[: len(b) // 2] = nb                                      # half the points in the last, partial block
        su = b * 1.0 + rng.uniform(0, 0.5 * 77 / 256, size=len(b))
        sv = rng.uniform(0, 16, size=len(b))
    elif case == "chunk_ends":
        c = rng.integers(0, 16, size=len(b))
        sv = c * 1.0 + rng.integers(0, 2, size=len(b)) * 0.15     # exactly a chunk's first or last v
    elif case == "between_chunks":
        c = rng.integers(0, 15, size=len(b))
        sv = c * 1.0 + 0.15 + rng.uniform(0.0, 0.85, size=len(b))  # in the gap between two chunks
        sv[::3] = c[::3] * 1.0 + 0.575                              # and exactly midway
    else:
        sv = rng.integers(0, 3, size=len(b)) * 0.5 + rng.normal(0, 0.01, size=len(b))
    src = np.stack([su, sv * 0.5, rng.normal(0, 0.002, size=len(b))], axis=1)
    return tgt.astype(np.float32), src.astype(np.float32)


def _search_twice(tgt, src, m):
    """an unseeded search at the identity, then one seeded from its pairs at pose m"""
    from object_alignment_amd.engine import IcpEngine
    eye = np.identity(4, dtype=np.float32)
    with IcpEngine(0) as e:
        e.set_search_mode("brute")
        e.set_target(tgt)
        e.set_source(src)
        e.set_matrices(eye, eye)
        idx, d2, _ = e.nn_search()
        assert e.stat("brute_kernel") == 3.0
        e.make_pairs(1e30)                               # winner records = seeds
        e.set_matrices(m, eye)
        idx2, d22, _ = e.nn_search()
    return idx, d2, idx2, d22


@pytest.mark.gpu
@pytest.mark.parametrize("R,bigtile,persist", [(1, "0", "4"), (2, "1", "0"), (4, "0", "4"), (4, "1", "4"), (4, "0", "0"),
                                               (4, "1", "0")])
@pytest.mark.parametrize("case", CASES)
def test_vends_answers_are_the_oracles(orc, case, R, bigtile, persist, monkeypatch):
    monkeypatch.setenv("OA_NN_VCHUNK", "1")
    monkeypatch.setenv("OA_NN_R", str(R))
    monkeypatch.setenv("OA_NN_BIGTILE", bigtile)
    monkeypatch.setenv("OA_NN_PERSIST", persist)
    monkeypatch.setenv("OA_NN_QUEUE_MIN_ITEMS", "0")
    tgt, src = _slabs(case, np.random.default_rng(zlib.crc32(case.encode()) + R))
    m = np.identity(4, dtype=np.float32)
    m[1, 3] = np.float32(0.004)                          # a small step along v for the seeded search
    idx, d2, idx2, d22 = _search_twice(tgt, src, m)
    ridx, rd2 = orc.nn_brute(src, tgt)
    assert np.array_equal(idx, ridx) and np.array_equal(d2, rd2, equal_nan=True)
    moved = np.array([orc.mat4_mul_vec3(m, p) for p in src], np.float32)
    r2, rd22 = orc.nn_brute(moved, tgt)
    assert np.array_equal(idx2, r2) and np.array_equal(d22, rd22, equal_nan=True)


def _chunks(rng, n, kind):
    """n chunks of 16 float32 v values in ascending order"""
    if kind == "uniform":
        q = rng.uniform(-1, 1, size=(n, 16))
    elif kind == "ties":
        q = rng.integers(-2, 3, size=(n, 16)) * 0.25
    elif kind == "tiny":
        q = rng.uniform(-1, 1, size=(n, 16)) * 1e-38            # around the denormal range
    elif kind == "wide":
        q = rng.uniform(-1, 1, size=(n, 16)) * 10.0 ** rng.integers(-30, 30, size=(n, 16))
    else:                                                         # zeros of both signs and values next to them
        q = rng.choice(np.array([-0.0, 0.0, 1e-45, -1e-45, 1.0, -1.0], np.float32), size=(n, 16))
    return np.sort(q.astype(np.float32), axis=1, kind="stable")


@pytest.mark.parametrize("kind", ["uniform", "ties", "tiny", "wide", "signed_zeros"])
def test_endpoint_mask_is_a_superset_of_the_fold(kind):
    """What the ends rule out, the fold over every vertex of the chunk (the round-7 test) rules out too: max(L, -F) > thr
    implies min |fl32(hv - qv_j)| > thr, for points on, between and away from the chunk's values and thresholds from 0 up."""
    rng = np.random.default_rng(zlib.crc32(kind.encode()))
    q = _chunks(rng, 4000, kind)
    with np.errstate(over="ignore", invalid="ignore"):
        pick = q[np.arange(len(q)), rng.integers(0, 16, size=len(q))]
        hv = np.where(rng.uniform(size=len(q)) < 0.5, pick, pick + (rng.normal(size=len(q)) * np.abs(pick)).astype(np.float32))
        hv = hv.astype(np.float32)
        for thr in (np.float32(0.0), np.float32(1e-40), np.float32(1e-3), np.float32(0.3), np.float32(np.inf)):
            a = (hv[:, None] - q).astype(np.float32)           # fl32(hv - qv_j), decreasing along the chunk
            fold_out = np.abs(a).min(axis=1) > thr
            end_out = np.maximum(a[:, -1], -a[:, 0]) > thr
            assert not np.any(end_out & ~fold_out)
            assert not np.any(end_out) or thr < np.inf
