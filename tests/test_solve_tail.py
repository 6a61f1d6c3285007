"""The loop's solve and its tail on injected sums, and the row-count edges of the fixed-order reduction.

Every point-metric iteration ends in solve_update_block (csrc/oa_kernels.hpp): the row reduction, a one-sided Jacobi SVD that is
warm-started from the last iteration's V, then matrix_world @ new_mat, the inverse, the convergence ring, halt and the step
record.  On the device the Jacobi angles come from reciprocal / reciprocal-square-root seeds plus Newton steps, with an IEEE
branch for magnitudes outside 1e-280 < h2 < 1e280; the host build of the header only has the IEEE branch, so only a GPU test
sees the code the GPU runs.  Two seams make that code a pure function of its inputs:

  * oa_iter_finish(ctx, d_sums) launches k_solve_update on whatever 24 doubles it is handed, the loop state (warm V, ring,
    d_pivot, matrix_world) carried on the device from call to call;
  * oa_kabsch_from_sums is its cold one-shot twin, and oa_kabsch reduces exactly min(4096, ceil(K / 256)) rows.

The reference (ref_solve) is the same operation in mpmath at 60 digits.  Tolerance, from the issue: the rotation block within
1e-12 * max(1, 1e-3 * sigma1 / gap) of the reference (1e-12 is what test_kabsch_properties asks of R; gap = sigma2 +
sign(det H) sigma3 is what the corrected rotation's conditioning depends on), the translation within that times
max(1, |c_a + pivot|, |c_b + pivot|).  The CPU guard holds the oracle's own host Jacobi to the same bound on every pair case, so
the reference and the cases are checked before any GPU run.

CPU: -m "not gpu" (layout, guard); GPU: -m gpu.
"""
import functools
import os
import re
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "object_alignment_amd", "csrc", "oa_kernels.hpp")

# layout of the 24 sums, restated from csrc/oa_kernels.hpp:33 ("constexpr int S_A = 0, S_B = 3, S_H = 6, ..."; the comment
# above it, :28-32, says what each slot holds: H[3 i + j] = sum b'_i a'_j, everything relative to the pivot)
NSUMS = 24
S_A, S_B, S_H, S_AA, S_BB, S_K, S_D, S_DD, S_W = 0, 3, 6, 15, 16, 17, 18, 19, 20
# oa_kabsch's launch shape: k_accumulate_pairs runs min(ACC_MAX_BLOCKS, ceil(K / ACC_THREADS)) workgroups (csrc/oa_icp.hip,
# oa_kabsch), one row of partials each; ACC_THREADS = 256 and ACC_MAX_BLOCKS = 4096 are csrc/oa_kernels.hpp:62-63.
# reduce_rows_block (same header) gives a row of NSUMS doubles to NSUMS / 2 = 12 threads, so its RED_THREADS = 1024 threads
# form RED_SLICES = 1024 // 12 = 85 slices.  test_layout_restated reads all of them back from the header.
ACC_THREADS, ACC_MAX_BLOCKS, RED_THREADS, RED_SLICES = 256, 4096, 1024, 85

TOL_R = 1e-12
P0 = np.array([0.5, -0.25, 0.125])                  # a float32-exact pivot for the loops whose case does not bring its own
REF_MSG = "input arrays are of wrong shape or type"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build_hip()
    return g


@pytest.fixture(scope="module")
def eng():
    from object_alignment_amd.engine import IcpEngine
    e = IcpEngine(0)
    e.set_search_mode("brute")
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------ the reference
class Ref:
    pass


def ref_solve(sums, pivot=None, with_scale=False, weighted=False):
    """The step from 24 sums in mpmath at 60 digits: mass, centroids, H = S_H - mass c_b c_a^T, SVD, R = U diag(1, 1,
    det(U V^T)) V^T, the scale from S_AA, S_BB when asked, M = T(c_b + pivot) sR T(-(c_a + pivot)).  Returns M, R (float64),
    the scale, sigma1..3, gap = sigma2 + sign(det H) sigma3 and the un-pivoted centroids."""
    import mpmath as mp
    with mp.workdps(60):
        s = [mp.mpf(float(x)) for x in np.asarray(sums, np.float64).reshape(NSUMS)]
        pv = [mp.mpf(float(x)) for x in (np.zeros(3) if pivot is None else np.asarray(pivot, np.float64))]
        mass = s[S_W] if weighted else s[S_K]
        ca = [s[S_A + i] / mass for i in range(3)]
        cb = [s[S_B + i] / mass for i in range(3)]
        H = mp.matrix(3, 3)
        for i in range(3):
            for j in range(3):
                H[i, j] = s[S_H + 3 * i + j] - mass * cb[i] * ca[j]
        U, S, V = mp.svd_r(H)                                   # H = U diag(S) V, S descending
        d = mp.mpf(1) if mp.det(U * V) > 0 else mp.mpf(-1)
        R = U * mp.diag([1, 1, d]) * V
        sc = mp.mpf(1)
        if with_scale:
            n0 = s[S_AA] - mass * sum(x * x for x in ca)
            n1 = s[S_BB] - mass * sum(x * x for x in cb)
            sc = mp.sqrt(n1 / n0)
        c0 = [ca[i] + pv[i] for i in range(3)]
        c1 = [cb[i] + pv[i] for i in range(3)]
        r = Ref()
        r.M = np.identity(4)
        for i in range(3):
            t = c1[i]
            for j in range(3):
                r.M[i, j] = float(sc * R[i, j])
                t -= sc * R[i, j] * c0[j]
            r.M[i, 3] = float(t)
        r.R = np.array([[float(R[i, j]) for j in range(3)] for i in range(3)])
        r.scale = float(sc)
        sig = sorted((S[k] for k in range(3)), reverse=True)
        r.sigma = [float(x) for x in sig]
        r.gap_over_s1 = float((sig[1] + d * sig[2]) / sig[0])
        r.c0 = np.array([float(x) for x in c0])
        r.c1 = np.array([float(x) for x in c1])
    return r


def centroids(sums, pivot, weighted=False):
    s = np.asarray(sums, np.float64)
    mass = s[S_W] if weighted else s[S_K]
    pv = np.zeros(3) if pivot is None else np.asarray(pivot, np.float64)
    return s[S_A:S_A + 3] / mass + pv, s[S_B:S_B + 3] / mass + pv


def tolerances(ref):
    """(rotation block, translation) bounds of the issue for one reference step; a similarity step's block s R and its
    translation carry the factor max(1, s)."""
    assert ref.gap_over_s1 > 0.0, "a case with a unique rotation has a positive gap"
    tol_r = TOL_R * max(1.0, 1e-3 / ref.gap_over_s1) * max(1.0, ref.scale)
    return tol_r, tol_r * max(1.0, float(np.linalg.norm(ref.c0)), float(np.linalg.norm(ref.c1)))


def check_step(M, ref, what):
    M = np.asarray(M, np.float64).reshape(4, 4)
    tol_r, tol_t = tolerances(ref)
    err_r = float(np.abs(M[:3, :3] - ref.M[:3, :3]).max())
    err_t = float(np.abs(M[:3, 3] - ref.M[:3, 3]).max())
    print("%-40s |dR| %.3g (tol %.3g)  |dt| %.3g (tol %.3g)  gap/s1 %.3g" % (what, err_r, tol_r, err_t, tol_t, ref.gap_over_s1))
    assert np.isfinite(M).all(), (what, M)
    assert err_r <= tol_r, (what, "rotation block", err_r, tol_r)
    assert err_t <= tol_t, (what, "translation", err_t, tol_t)
    assert np.array_equal(M[3], [0.0, 0.0, 0.0, 1.0]), (what, M[3])


def check_properties(M, sums, pivot, what, weighted=False):
    """What holds where the rotation is not unique: M finite, R^T R = I to 1e-12, det R = +1, centroid to centroid."""
    M = np.asarray(M, np.float64).reshape(4, 4)
    assert np.isfinite(M).all(), (what, M)
    R = M[:3, :3]
    orth = float(np.abs(R.T @ R - np.identity(3)).max())
    det = float(np.linalg.det(R))
    c0, c1 = centroids(sums, pivot, weighted)
    moved = float(np.abs(R @ c0 + M[:3, 3] - c1).max())
    print("%-40s |R^T R - I| %.3g  det %.17g  |M c_a - c_b| %.3g" % (what, orth, det, moved))
    assert orth <= 1e-12, (what, orth)
    assert abs(det - 1.0) <= 1e-11, (what, det)
    assert moved <= 1e-12 * max(1.0, float(np.linalg.norm(c0)), float(np.linalg.norm(c1))), (what, moved)
    assert np.array_equal(M[3], [0.0, 0.0, 0.0, 1.0]), (what, M[3])


# ------------------------------------------------------------------------------------------------ the cases
def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    t = np.deg2rad(deg)
    return np.identity(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def exact_sums(A, B, pivot, w=None):
    """The 24 sums of the pairs (A, B) (3 x K, float64) about `pivot`, exact (rationals) and rounded once; w: a weight per pair
    (sums 0..16 carry it, S_W is its mass, S_K the count -- the weighted layout of oa_kernels.hpp:31-32)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    K = A.shape[1]
    p = [Fraction(float(x)) for x in pivot]
    ws = [Fraction(1)] * K if w is None else [Fraction(float(x)) for x in w]
    a = [[Fraction(float(A[i, k])) - p[i] for k in range(K)] for i in range(3)]
    b = [[Fraction(float(B[i, k])) - p[i] for k in range(K)] for i in range(3)]
    s = [Fraction(0)] * NSUMS
    for i in range(3):
        s[S_A + i] = sum(ws[k] * a[i][k] for k in range(K))
        s[S_B + i] = sum(ws[k] * b[i][k] for k in range(K))
        for j in range(3):
            s[S_H + 3 * i + j] = sum(ws[k] * b[i][k] * a[j][k] for k in range(K))
    s[S_AA] = sum(ws[k] * (a[0][k] ** 2 + a[1][k] ** 2 + a[2][k] ** 2) for k in range(K))
    s[S_BB] = sum(ws[k] * (b[0][k] ** 2 + b[1][k] ** 2 + b[2][k] ** 2) for k in range(K))
    s[S_K] = Fraction(K)
    if w is not None:
        s[S_W] = sum(ws)
    return np.array([float(x) for x in s], np.float64)


R0 = rot([0.3, -0.5, 0.8], 37.0)
T0 = np.array([0.4, -0.2, 0.3])
# full-rank covariances for the sums-only cases and the loops' unrelated steps: U diag(3, 2, 1) V^T, gap / sigma1 = 1
H0 = rot([1.0, 2.0, -1.5], 63.0) @ np.diag([3.0, 2.0, 1.0]) @ rot([-0.4, 0.1, 0.9], -48.0)
H1 = rot([0.2, -1.0, 0.3], 121.0) @ np.diag([3.0, 2.0, 1.0]) @ rot([0.7, 0.7, -0.2], 15.0)
H2 = rot([-1.0, 0.1, 0.4], -77.0) @ np.diag([3.0, 2.0, 1.0]) @ rot([0.1, 0.5, 1.0], 99.0)


def sums_from_H(H, cb=(0.3, -0.2, 0.1), K=8.0, w=0.0):
    """Sums no cloud has to produce: S_A = 0, so H = S_H exactly and c_b = `cb`; S_AA, S_BB give the scale sqrt(3 / 2).
    w: S_W (then the mass of a weighted step; S_B follows it)."""
    s = np.zeros(NSUMS)
    mass = w if w else K
    cb = np.asarray(cb, np.float64)
    s[S_H:S_H + 9] = np.asarray(H, np.float64).reshape(9)
    s[S_B:S_B + 3] = mass * cb
    s[S_AA] = 2.0 * mass
    s[S_BB] = mass * float(cb @ cb) + 3.0 * mass
    s[S_K] = K
    s[S_W] = w
    return s


@functools.lru_cache(maxsize=None)
def pair_cases():
    """name -> (A, B, pivot): the 0-cases with a unique rotation that are clouds.  The pivot is the first column unless said."""
    rng = np.random.default_rng(20240611)
    c = {}

    def put(name, A, B, pivot=None):
        c[name] = (A, B, A[:, 0].copy() if pivot is None else np.asarray(pivot, np.float64))

    A = rng.normal(size=(3, 40))
    put("generic", A, R0 @ A + T0[:, None] + 1e-3 * rng.normal(size=A.shape))
    A = rng.normal(size=(3, 33))
    A[2] = 0.0                                                        # a'_z = 0 exactly: the third column of H is exactly 0
    put("planar", A, R0 @ A + T0[:, None])
    A = rng.normal(size=(3, 37))
    A[2] *= 1e-7                                                      # sigma3 / sigma1 ~ 1e-14
    put("slab", A, R0 @ A + T0[:, None] + 1e-9 * rng.normal(size=A.shape))
    A = rng.normal(size=(3, 3))
    put("K3", A, R0 @ A + T0[:, None] + 1e-3 * rng.normal(size=A.shape))
    A = np.array([[1.0, -1, 0, 0, 0, 0], [0, 0, 1.0, -1, 0, 0], [0, 0, 0, 0, 1.0, -1]])
    put("octahedron", A, R0 @ A + T0[:, None])                      # H = 2 R0: sigma1 = sigma2 = sigma3
    A = np.diag([3.0, 2.0, 1.0]) @ rng.normal(size=(3, 40))
    put("mirror_noisy", A, R0 @ np.diag([1.0, 1.0, -1.0]) @ A + T0[:, None] + 1e-3 * rng.normal(size=A.shape))   # det H < 0
    A = np.diag([3.0, 1.0, 0.0]) @ rng.normal(size=(3, 35))
    put("mirror_planar", A, R0 @ np.diag([1.0, -1.0, 1.0]) @ A + T0[:, None])
    # 3e4 from the origin, on a grid of 1 / 64 (float32-exact): every sum below is exact in float64 about either pivot, so the
    # reference sees the cloud itself and not a rounding of its second moments
    ctr = np.array([30000.0, 29000.0, 31000.0])
    A = np.round((ctr[:, None] + rng.normal(size=(3, 40))) * 64.0) / 64.0
    B = np.round((R0 @ (A - ctr[:, None]) + ctr[:, None] + T0[:, None]) * 64.0) / 64.0
    put("far_pivot_first", A, B)
    put("far_pivot_zero", A, B, np.zeros(3))
    A = rng.normal(size=(3, 40))
    put("rot179", A, rot([0.6, 0.1, -0.7], 179.99) @ A + T0[:, None] + 1e-3 * rng.normal(size=A.shape))
    A, B, _ = c["generic"]
    put("tiny", A * 1e-18, B * 1e-18)
    put("huge", A * 1e18, B * 1e18)
    return c


PAIR_NAMES = ("generic", "planar", "slab", "K3", "octahedron", "mirror_noisy", "mirror_planar", "far_pivot_first",
              "far_pivot_zero", "rot179", "tiny", "huge")
# H scaled so that jacobi_rotate's h2 = w^2 + 4 dpq^2 (fourth powers of H) leaves (1e-280, 1e280) -- the device's IEEE branch --
# or stays just inside it
SUMS_ONLY = {"H_1e72": 1e72, "H_1e-72": 1e-72, "H_1e60": 1e60, "H_1e-60": 1e-60}
UNIQUE_NAMES = PAIR_NAMES + tuple(SUMS_ONLY)
WELL_CONDITIONED = ("generic", "octahedron", "mirror_noisy", "far_pivot_first", "rot179", "tiny", "huge")
NON_UNIQUE = ("collinear", "all_equal", "s2_eq_s3_neg")


@functools.lru_cache(maxsize=None)
def case_sums(name, loop=False):
    """(sums, pivot) of a named case.  loop: about the pivot a loop's context can have -- a float32 point (the first source
    vertex); the cloud beyond float32 geometry's comfort (huge) and the sums-only cases take P0."""
    if name in SUMS_ONLY:
        return sums_from_H(H0 * SUMS_ONLY[name]), P0.copy()
    if name == "s2_eq_s3_neg":
        U, V = rot([1.0, 2.0, -1.5], 63.0), rot([-0.4, 0.1, 0.9], -48.0)
        return sums_from_H(U @ np.diag([3.0, 1.0, -1.0]) @ V), P0.copy()
    if name == "collinear":
        rng = np.random.default_rng(5)
        A = np.outer([0.6, -0.3, 0.74], rng.normal(size=20))
        A, B, pivot = A, R0 @ A + T0[:, None], A[:, 0].copy()
    elif name == "all_equal":
        A = np.repeat(np.array([[0.25], [0.5], [-0.75]]), 9, axis=1)
        A, B, pivot = A, A + T0[:, None], A[:, 0].copy()
    else:
        A, B, pivot = pair_cases()[name]
    if loop:
        pivot = P0.copy() if name == "huge" else pivot.astype(np.float32).astype(np.float64)
    return exact_sums(A, B, pivot), pivot


@functools.lru_cache(maxsize=None)
def case_ref(name, with_scale=False, loop=False):
    s, pv = case_sums(name, loop)
    return ref_solve(s, pv, with_scale)


# ------------------------------------------------------------------------------------------------ 0. layout and guard (CPU)
def test_layout_restated(built):
    """The constants restated above are the header's, and the library is built with them."""
    from object_alignment_amd import _capi
    text = open(HEADER).read()
    m = re.search(r"constexpr int (S_A = [^;]*);", text)
    got = {k.strip(): int(v) for k, v in (kv.split("=") for kv in m.group(1).split(","))}
    assert got == dict(S_A=S_A, S_B=S_B, S_H=S_H, S_AA=S_AA, S_BB=S_BB, S_K=S_K, S_D=S_D, S_DD=S_DD, S_W=S_W)
    for name, val in (("NSUMS", NSUMS), ("ACC_THREADS", ACC_THREADS), ("ACC_MAX_BLOCKS", ACC_MAX_BLOCKS), ("RED_THREADS", RED_THREADS)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)) == val, name
    assert RED_SLICES == RED_THREADS // (NSUMS // 2) and _capi.OA_NSUMS == NSUMS
    assert hasattr(_capi.load(), "oa_kabsch_from_sums") and hasattr(_capi.load(), "oa_iter_finish")


@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("name", PAIR_NAMES)
def test_guard_host_jacobi_inside_tolerance(orc, name, with_scale):
    """The reference and the cases, before any GPU run: the oracle's own host Jacobi (IEEE, from the points) is inside the
    tolerance on every pair case; the cases are what their names say."""
    A, B, pivot = pair_cases()[name]
    ref = case_ref(name, with_scale)
    check_step(orc.kabsch_c(A, B, scale=with_scale), ref, "guard %s scale=%d" % (name, with_scale))
    s1, s2, s3 = ref.sigma
    if name in ("planar", "mirror_planar"):
        assert s3 == 0.0 or s3 <= 1e-30 * s1
    if name == "slab":
        assert 1e-16 < s3 / s1 < 1e-12
    if name == "octahedron":
        assert (s1 - s3) <= 1e-12 * s1
    if name == "mirror_noisy":
        assert s3 > 0.1 * s1 and ref.gap_over_s1 < s2 / s1           # det H < 0: the gap is sigma2 - sigma3
    if name.startswith("far"):
        assert np.array_equal(A.astype(np.float32).astype(np.float64), A) and np.linalg.norm(ref.c0) > 3e4


def test_guard_sums_only_cases():
    """The sums-only cases are what they claim: H0 scaled, its fourth power outside / inside (1e-280, 1e280); the non-unique
    ones have the degeneracy named."""
    for name, f in SUMS_ONLY.items():
        ref = case_ref(name)
        assert abs(ref.gap_over_s1 - 1.0) < 1e-12 and abs(ref.sigma[0] / f - 3.0) < 1e-12
        h2 = (ref.sigma[0] ** 2 - ref.sigma[2] ** 2) ** 2
        assert (1e-280 < h2 < 1e280) == (name in ("H_1e60", "H_1e-60")), (name, h2)
    s, pv = case_sums("s2_eq_s3_neg")
    sv = np.linalg.svd(s[S_H:S_H + 9].reshape(3, 3), compute_uv=False)
    assert abs(sv[1] - sv[2]) < 1e-14 and np.linalg.det(s[S_H:S_H + 9].reshape(3, 3)) < 0
    for name, rank in (("collinear", 1), ("all_equal", 0)):
        s, pv = case_sums(name)
        ca, cb = s[S_A:S_A + 3] / s[S_K], s[S_B:S_B + 3] / s[S_K]
        sv = np.linalg.svd(s[S_H:S_H + 9].reshape(3, 3) - s[S_K] * np.outer(cb, ca), compute_uv=False)
        assert int((sv > 1e-12 * max(sv[0], 1e-300)).sum()) == rank, (name, sv)


# ------------------------------------------------------------------------------------------------ 1. cold solve from sums
@pytest.mark.gpu
@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("name", UNIQUE_NAMES)
def test_cold_from_sums(eng, name, with_scale):
    """Every 0-case through the cold solve.  far_pivot_zero is the case that found something: before solve_from_sums redid
    heavily cancelling differences in two doubles (CANCEL_GATE) it gave |dR| 9.2e-8 and |dt| 5.8e-3 here, 2.2e-16 and 1.5e-11
    since."""
    s, pv = case_sums(name)
    check_step(eng.kabsch_from_sums(s, pv, scale=with_scale), case_ref(name, with_scale), "cold %s scale=%d" % (name, with_scale))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NON_UNIQUE)
def test_cold_from_sums_non_unique(eng, name):
    s, pv = case_sums(name)
    check_properties(eng.kabsch_from_sums(s, pv), s, pv, "cold " + name)


@pytest.mark.gpu
def test_cold_pivot_none(eng):
    A, B, _ = pair_cases()["generic"]
    s = exact_sums(A, B, np.zeros(3))
    check_step(eng.kabsch_from_sums(s, None), ref_solve(s, None), "cold generic, sums about the origin, pivot=None")
    assert np.array_equal(eng.kabsch_from_sums(s, None), eng.kabsch_from_sums(s, np.zeros(3)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", WELL_CONDITIONED)
def test_from_sums_equals_kabsch(eng, name):
    """Exact sums into the solve against the device's own accumulation of the same pairs: 1e-12 relative."""
    A, B, pivot = pair_cases()[name]
    for sc in (False, True):
        M1, M2 = eng.kabsch_from_sums(exact_sums(A, B, pivot), pivot, scale=sc), eng.kabsch(A, B, scale=sc)
        err = float(np.abs(M1 - M2).max())
        print("from_sums vs kabsch %-16s scale=%d: %.3g" % (name, sc, err))
        assert err <= 1e-12 * max(1.0, float(np.abs(M2).max())), (name, sc, err)


@pytest.mark.gpu
def test_from_sums_too_few_pairs_and_slot_20(eng):
    A, B, pivot = pair_cases()["generic"]
    s = exact_sums(A, B, pivot)
    with pytest.raises(ValueError, match=REF_MSG):
        eng.kabsch(A[:, :2], B[:, :2])
    for k in (2.0, 2.999, float("nan")):
        bad = s.copy()
        bad[S_K] = k
        with pytest.raises(ValueError, match=REF_MSG):
            eng.kabsch_from_sums(bad, pivot)
    M = eng.kabsch_from_sums(s, pivot)
    for w in (0.125, -3.0, 1e300, float("nan")):                  # slot 20 is the mass of WEIGHTED steps only: ignored here
        other = s.copy()
        other[S_W] = w
        assert np.array_equal(eng.kabsch_from_sums(other, pivot), M), w


# ------------------------------------------------------------------------------------------------ 2. iter_finish: the harness
def with_stats(rows, seed=1):
    """Copies of the rows with crafted distance sums.  The device sums distances relative to the previous step's mean, so
    S_D = K (mean_i - mean_{i-1}) and S_DD = K (that difference squared + variance); every third row's variance comes out
    negative (S_DD a little short), which the tail clamps to 0."""
    rng = np.random.default_rng(seed)
    out = []
    for i, row in enumerate(rows):
        r = np.array(row, np.float64)
        if r[S_K] >= 3.0:
            delta = float(rng.normal()) * 0.05
            r[S_D] = r[S_K] * delta
            r[S_DD] = r[S_K] * (delta * delta + float(rng.uniform(0.0, 0.01))) if i % 3 != 2 else r[S_K] * delta * delta * 0.999
        out.append(r)
    return out


def loop_geometry(pivot):
    """Any 8-point source whose first vertex is the pivot, and a target next to it."""
    corners = np.array([[i & 1, (i >> 1) & 1, (i >> 2) & 1] for i in range(8)], np.float64)
    src = (np.asarray(pivot, np.float64)[None, :] + 0.25 * corners).astype(np.float32)
    src[0] = np.asarray(pivot, np.float32)
    return src, (src.astype(np.float64) + 0.01).astype(np.float32)


class LoopOut:
    pass


def run_sums(e, pivot, rows, iters=None, weights=None, start=None, **kw):
    """A loop whose steps are iter_finish on crafted sums: upload any geometry with `pivot` as first source vertex, run_begin,
    one iter_finish per row, run_end.  iter_partial is never called.  Returns the RunResult's fields, or on an error status
    what the history and the context hold, with the exception in .error."""
    import torch
    from object_alignment_amd._capi import OaError
    src, tgt = loop_geometry(pivot)
    eye = np.identity(4, dtype=np.float32)
    e.set_search_mode("brute")
    e.set_target(tgt)
    e.set_source(src, stride=1)
    if weights is not None:
        e.set_source_weights(weights)
    e.set_matrices(eye if start is None else start, eye)
    assert np.array_equal(e.pivot(), np.asarray(pivot, np.float64)), (e.pivot(), pivot)
    t = torch.tensor(np.asarray(rows, np.float64).reshape(-1, NSUMS), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()                                        # the context reads the rows on its own stream
    e.run_begin(iters=len(rows) if iters is None else iters, thresh=0.5, **kw)
    for i in range(len(rows)):
        e.iter_finish(t[i].data_ptr())
    out = LoopOut()
    out.error = None
    try:
        res = e.run_end()
        out.iters_done, out.converged, out.matrix_world = res.iters_done, res.converged, res.matrix_world
        out.step_M, out.step_new, out.step_K, out.step_stats, out.step_trans = res.step_M, res.step_new, res.step_K, res.step_stats, res.step_trans
    except (ValueError, OaError) as ex:
        out.error = ex
        out.step_M, out.step_new, out.step_K, out.step_stats, out.step_trans = e._history(len(rows))
        out.iters_done, out.converged, out.matrix_world = len(out.step_M), None, e.matrix_world()
    del t
    return out


def ulps(a, b):
    return abs(a - b) / np.spacing(abs(b)) if b != 0.0 else (0.0 if a == 0.0 else np.inf)


def check_tail(orc, out, rows, start=None):
    """What follows M in every step, from the device's own step_new: new_mat = float32(M), matrix_world the left fold of
    mat4_mul, |translation|, K, the running mean and the clamped one-pass deviation."""
    n = out.iters_done
    assert len(out.step_M) == n and n <= len(rows)
    assert np.array_equal(out.step_new.view(np.uint32), out.step_M.astype(np.float32).view(np.uint32))
    mw = np.identity(4, dtype=np.float32) if start is None else np.asarray(start, np.float32)
    mean = 0.0
    with np.errstate(all="ignore"):
        for i in range(n):
            mw = orc.mat4_mul(mw, out.step_new[i])
            assert out.step_trans[i] == orc.vec3_length(out.step_new[i][:3, 3]), i
            K = rows[i][S_K]
            assert out.step_K[i] == int(K), i
            md = rows[i][S_D] / K
            mean = md + mean
            std = np.sqrt(max(0.0, rows[i][S_DD] / K - md * md))
            assert ulps(out.step_stats[i][0], mean) <= 2 and ulps(out.step_stats[i][1], std) <= 2, (i, out.step_stats[i], mean, std)
    assert np.array_equal(mw.view(np.uint32), out.matrix_world.view(np.uint32)), (mw, out.matrix_world)


def check_sequence(orc, out, rows, pivot, unique, what, weighted=False, with_scale=False):
    """unique[i]: step i has one answer (reference + tolerance) or not (properties)."""
    assert out.error is None, out.error
    assert out.iters_done == len(rows)
    for i, row in enumerate(rows):
        if unique[i]:
            check_step(out.step_M[i], ref_solve(row, pivot, with_scale, weighted), "%s step %d" % (what, i))
        else:
            check_properties(out.step_M[i], row, pivot, "%s step %d" % (what, i), weighted)
    check_tail(orc, out, rows)


@pytest.mark.gpu
def test_seam_replays_a_real_loop(golden_dir):
    """The seam is what it seems: a real split-phase loop (iter_partial, iter_finish on its own sums), then the same loop with
    every step's sums taken to the host, uploaded into a fresh tensor and handed to iter_finish alone -- bitwise the same."""
    import torch
    from object_alignment_amd.engine import IcpEngine
    g = np.load(os.path.join(golden_dir, "icp_loop_bumpy_converge.npz"), allow_pickle=False)
    dev = torch.device("cuda:0")
    kw = dict(iters=6, thresh=0.5, target_d=0.01, use_target=True, early_exit=False)
    with IcpEngine(0) as e:
        e.set_stream(torch.cuda.current_stream().cuda_stream)
        e.set_target(g["tgt"])
        e.set_source(g["src"], stride=1)
        e.set_matrices(g["mx_align"], g["mx_base"])
        sums = torch.zeros(NSUMS, dtype=torch.float64, device=dev)
        e.run_begin(**kw)
        host = []
        for _ in range(6):
            e.iter_partial(sums.data_ptr())
            host.append(sums.cpu().numpy().copy())
            e.iter_finish(sums.data_ptr())
        real = e.run_end()
        e.set_matrices(g["mx_align"], g["mx_base"])
        e.run_begin(**kw)
        keep = []
        for i in range(6):
            keep.append(torch.tensor(host[i], dtype=torch.float64, device=dev))
            e.iter_finish(keep[-1].data_ptr())
        replay = e.run_end()
    assert real.iters_done == replay.iters_done == 6
    assert np.array_equal(real.step_K, [int(h[S_K]) for h in host])
    for name in ("step_M", "step_new", "matrix_world", "step_stats", "step_trans", "step_K"):
        a, b = getattr(real, name), getattr(replay, name)
        assert a.tobytes() == b.tobytes(), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", UNIQUE_NAMES)
def test_warm_after_unrelated_step(eng, orc, name):
    """a. every unique case behind one step on another covariance: the warm V is valid but has nothing to do with H."""
    s, pv = case_sums(name, loop=True)
    rows = with_stats([sums_from_H(H1), s])
    check_sequence(orc, run_sums(eng, pv, rows), rows, pv, [True, True], "warm " + name)


@pytest.mark.gpu
def test_warm_repeat_then_large_step(eng, orc):
    """b. the same covariance 12 times (the warm V diagonalises it: no rotation at all), its rotation by 170 degrees about a
    skew axis, and back: a V left stale by a large step."""
    far = sums_from_H(rot([0.5, -0.8, 0.33], 170.0) @ H0)
    rows = with_stats([sums_from_H(H0)] * 12 + [far, sums_from_H(H0), far, far, sums_from_H(H0)])
    check_sequence(orc, run_sums(eng, P0, rows), rows, P0, [True] * len(rows), "repeat/170")


@pytest.mark.gpu
def test_warm_rank_and_reflection_alternate(eng, orc):
    """c, d. full rank / exactly planar / full rank / planar about another normal; det H > 0 against det H < 0."""
    planar_z, planar_x = H0 @ np.diag([1.0, 1.0, 0.0]), H1 @ np.diag([0.0, 1.0, 1.0])
    neg0, neg1 = H0 @ np.diag([1.0, 1.0, -1.0]), np.diag([-1.0, 1.0, 1.0]) @ H1
    for what, hs in (("rank 3/2", [H0, planar_z, H1, planar_x, H0, planar_x, planar_z, H2]),
                     ("det +/-", [H0, neg0, H0, neg1, H1, neg1, neg0, H2, neg0])):
        rows = with_stats([sums_from_H(h) for h in hs])
        check_sequence(orc, run_sums(eng, P0, rows), rows, P0, [True] * len(rows), what)


@pytest.mark.gpu
def test_warm_both_branches_of_jacobi_rotate(eng, orc):
    """e. H at 1e+-72 (IEEE branch) and 1e+-60 (seeds + Newton, near the range's ends) between steps at scale 1."""
    hs = [H0, H1 * 1e72, H2, H0 * 1e-72, H1, H2 * 1e60, H0 * 1e-60, H1 * 1e-72, H2 * 1e72, H0]
    rows = with_stats([sums_from_H(h) for h in hs])
    check_sequence(orc, run_sums(eng, P0, rows), rows, P0, [True] * len(rows), "1e+-72")


@pytest.mark.gpu
def test_warm_non_unique_does_not_poison(eng, orc):
    """f. collinear, H = 0 and sigma2 = sigma3 with det H < 0 in the middle of a loop: properties only there, and the next
    unique step is back inside the tolerance."""
    pv = case_sums("collinear", loop=True)[1]
    rows, unique = [], []
    for h, name in ((H0, "collinear"), (H1, "s2_eq_s3_neg"), (H2, "collinear"), (H0, "s2_eq_s3_neg")):
        rows += [sums_from_H(h), case_sums(name, loop=True)[0] if name == "collinear" else case_sums(name)[0]]
        unique += [True, False]
    rows, unique = with_stats(rows + [sums_from_H(H1)]), unique + [True]
    check_sequence(orc, run_sums(eng, pv, rows), rows, pv, unique, "non-unique")
    pv = case_sums("all_equal", loop=True)[1]
    zero = case_sums("all_equal", loop=True)[0]
    rows = with_stats([sums_from_H(H0), zero, sums_from_H(H1), zero, zero, sums_from_H(H2)])
    check_sequence(orc, run_sums(eng, pv, rows), rows, pv, [True, False, True, False, False, True], "H = 0")


@pytest.mark.gpu
def test_weighted_loop_takes_its_mass_from_s_w(eng, orc):
    """g. DevState::weighted = 1 (vertex weights set): the mass is S_W, the pair count stays S_K; a mass of 0 ends the loop
    like K < 3."""
    A, B, _ = pair_cases()["generic"]
    w = np.random.default_rng(3).uniform(0.25, 2.0, size=A.shape[1])
    rows = with_stats([sums_from_H(H0, K=8.0, w=5.5), exact_sums(A, B, P0, w), sums_from_H(H1, K=40.0, w=0.375),
                       sums_from_H(np.diag([1.0, 1.0, -1.0]) @ H2, K=3.0, w=17.25)])
    assert all(r[S_W] != r[S_K] for r in rows)
    vw = np.linspace(0.5, 1.5, 8).astype(np.float32)
    check_sequence(orc, run_sums(eng, P0, rows, weights=vw), rows, P0, [True] * 4, "weighted", weighted=True)
    rows = with_stats([sums_from_H(H0, K=8.0, w=5.5), sums_from_H(H1, K=5.0, w=0.0), sums_from_H(H2, K=8.0, w=2.0)])
    out = run_sums(eng, P0, rows, weights=vw)
    assert isinstance(out.error, ValueError) and REF_MSG in str(out.error) and out.iters_done == 1
    check_step(out.step_M[0], ref_solve(rows[0], P0, weighted=True), "weighted step before the empty mass")


@pytest.mark.gpu
def test_drift_2000_steps(eng, orc):
    """h. 2000 steps on H = R_i diag(3, 2, 1) Q_i, both rotations moving 5 degrees a step: the V that open loops carry without
    ever re-orthogonalising.  numpy's SVD is the reference (gap / sigma1 = 1: fp64 is enough)."""
    rng = np.random.default_rng(77)
    Ri, Qi = rot([1.0, 0.2, -0.3], 20.0), rot([0.1, -1.0, 0.5], -35.0)
    rows, want = [], []
    for _ in range(2000):
        Ri = Ri @ rot(rng.normal(size=3), 5.0)
        Qi = rot(rng.normal(size=3), 5.0) @ Qi
        u, _, vt = np.linalg.svd(Ri)
        Ri = u @ vt                                                   # (the test's own rotations stay orthogonal)
        u, _, vt = np.linalg.svd(Qi)
        Qi = u @ vt
        H = Ri @ np.diag([3.0, 2.0, 1.0]) @ Qi
        cb = 1e-3 * rng.normal(size=3)
        rows.append(sums_from_H(H, cb=cb))
        u, _, vt = np.linalg.svd(H)
        R = u @ np.diag([1.0, 1.0, np.sign(np.linalg.det(u @ vt))]) @ vt
        M = np.identity(4)
        M[:3, :3] = R
        M[:3, 3] = (cb + P0) - R @ P0
        want.append(M)
    rows = with_stats(rows)
    out = run_sums(eng, P0, rows)
    assert out.error is None and out.iters_done == 2000
    R = out.step_M[:, :3, :3]
    orth = np.abs(np.einsum("nki,nkj->nij", R, R) - np.identity(3)).max(axis=(1, 2))
    err_r = np.abs(R - np.array(want)[:, :3, :3]).max(axis=(1, 2))
    err_t = np.abs(out.step_M[:, :3, 3] - np.array(want)[:, :3, 3]).max(axis=1)
    print("drift: max |R^T R - I| %.3g (step %d), max |dR| %.3g (step %d), max |dt| %.3g" % (orth.max(), orth.argmax(), err_r.max(), err_r.argmax(), err_t.max()))
    assert np.isfinite(out.step_M).all() and np.isfinite(out.matrix_world).all()
    assert orth.max() <= 1e-12 and err_r.max() <= TOL_R and err_t.max() <= TOL_R * max(1.0, float(np.linalg.norm(P0 + 4e-3)))
    check_tail(orc, out, rows)


# ------------------------------------------------------------------------------------------------ 2. the convergence ring
def ring_rows(sizes):
    """Steps whose rotation is the identity and whose translation is (size, 0, 0): S_A = 0 and H diagonal, so M = T(c_b)."""
    return with_stats([sums_from_H(np.diag([3.0, 2.0, 1.0]), cb=(t, 0.0, 0.0)) for t in sizes])


TARGET_D = 0.01
UNDER, OVER = 0.001, 0.1
RING = [UNDER] * 4 + [OVER] + [UNDER] * 5            # four under target_d, one over, five under: converged at the tenth


@pytest.mark.gpu
def test_ring_converges_exactly_at_the_tenth(eng, orc):
    for n in (9, 10):
        rows = ring_rows(RING[:n])
        out = run_sums(eng, P0, rows, iters=50, target_d=TARGET_D, use_target=True, early_exit=True)
        assert out.error is None and out.iters_done == n and out.converged == (n == 10), (n, out.iters_done, out.converged)
        check_tail(orc, out, rows)
    # early exit: the calls after the tenth change nothing
    rows = ring_rows(RING + [OVER, UNDER, OVER, UNDER, UNDER])
    frozen = run_sums(eng, P0, rows, iters=50, target_d=TARGET_D, use_target=True, early_exit=True)
    assert frozen.error is None and frozen.iters_done == 10 and frozen.converged
    assert np.array_equal(frozen.matrix_world, out.matrix_world) and np.array_equal(frozen.step_M, out.step_M)
    check_tail(orc, frozen, rows)
    # without it the loop runs on, converged all the same; here to exactly `iters`, whatever is enqueued after
    on = run_sums(eng, P0, rows, iters=13, target_d=TARGET_D, use_target=True, early_exit=False)
    assert on.error is None and on.iters_done == 13 and on.converged
    check_tail(orc, on, rows)
    assert np.array_equal(on.step_M[:10], out.step_M)
    # no target: never converged
    never = run_sums(eng, P0, rows, iters=50, target_d=TARGET_D, use_target=False, early_exit=True)
    assert never.error is None and never.iters_done == len(rows) and not never.converged
    check_tail(orc, never, rows)
    # the ring is five long: an over-target step every fifth keeps it open
    rows = ring_rows(([UNDER] * 4 + [OVER]) * 3)
    open_ = run_sums(eng, P0, rows, iters=50, target_d=TARGET_D, use_target=True, early_exit=True)
    assert open_.error is None and open_.iters_done == 15 and not open_.converged


@pytest.mark.gpu
def test_too_few_pairs_mid_loop_leaves_the_context_usable(eng, orc):
    from object_alignment_amd import synth
    from object_alignment_amd.engine import IcpEngine
    bad = sums_from_H(H1)
    bad[S_K] = 2.0
    rows = with_stats([sums_from_H(H0), sums_from_H(H2), bad, sums_from_H(H0)])
    out = run_sums(eng, P0, rows)
    assert isinstance(out.error, ValueError) and REF_MSG in str(out.error)
    assert out.iters_done == 2
    check_tail(orc, out, rows)                                        # the two steps before it were applied, nothing after
    cloud = synth.bumpy_icosphere(2)
    mxa = synth.rigid4(synth.rotation_from_rotvec([0.03, -0.02, 0.04]), [0.02, -0.01, 0.015])
    eye = np.identity(4, dtype=np.float32)
    res = []
    with IcpEngine(0) as fresh:
        for e in (eng, fresh):
            e.set_search_mode("brute")
            e.set_target(cloud)
            e.set_source(cloud, stride=1)
            e.set_matrices(mxa, eye)
            res.append(e.run(iters=8, thresh=0.5, target_d=1e-9, use_target=True, early_exit=True))
    assert res[0].iters_done == res[1].iters_done == 8
    for name in ("step_M", "step_new", "matrix_world", "step_stats", "step_trans", "step_K"):
        assert getattr(res[0], name).tobytes() == getattr(res[1], name).tobytes(), name


@pytest.mark.gpu
def test_with_scale_degenerate_ends(eng, orc):
    """with_scale at n1 = 0 (every b equal: the zero block, a singular matrix_world, status -4) and at n0 = 0 (every a equal:
    the reference divides by zero)."""
    from object_alignment_amd import _capi
    rng = np.random.default_rng(9)
    A = rng.normal(size=(3, 16))                                     # (16 pairs: c_b and K |c_b|^2 are exact, n1 is exactly 0)
    B = np.repeat(np.array([[0.5], [0.25], [-1.0]]), 16, axis=1)
    rows = with_stats([sums_from_H(H0), exact_sums(A, B, P0), sums_from_H(H1)])
    out = run_sums(eng, P0, rows, with_scale=True)
    assert isinstance(out.error, _capi.OaError) and out.error.code == _capi.OA_E_SINGULAR, out.error
    assert out.iters_done == 2 and np.array_equal(out.step_M[1][:3, :3], np.zeros((3, 3)))
    assert np.array_equal(out.matrix_world[:3, :3], np.zeros((3, 3), np.float32))
    check_tail(orc, out, rows)
    # n0 = 0
    B = rng.normal(size=(3, 12))
    A = np.repeat(P0[:, None], 12, axis=1)
    with np.errstate(all="ignore"):
        want = orc.affine_matrix_from_points(A, B, shear=False, scale=True)
    rows = with_stats([sums_from_H(H0), exact_sums(A, B, P0)])
    out = run_sums(eng, P0, rows, with_scale=True)
    if np.isfinite(want).all():
        assert out.error is None and np.abs(out.step_M[1] - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
    else:
        assert out.error is not None or not np.isfinite(out.step_M[1]).all(), out.step_M[1]
    with np.errstate(all="ignore"):
        if np.isfinite(want).all():
            assert np.abs(eng.kabsch_from_sums(exact_sums(A, B, P0), P0, scale=True) - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
        else:
            assert not np.isfinite(eng.kabsch_from_sums(exact_sums(A, B, P0), P0, scale=True)).all()


# ------------------------------------------------------------------------------------------------ 3. row-count edges
# rows of partials oa_kabsch reduces: 85 = RED_SLICES; 4 * 85 = 340 is where reduce_rows_block's last batch switches from four
# wide to sixteen wide; 15 * 85 = 1275 is the main loop's entry and 16 * 85 = 1360 its step; 4096 = ACC_MAX_BLOCKS
ROW_COUNTS = (1, 2, 84, 85, 86, 340, 341, 342, 425, 426, 1275, 1276, 1277, 1360, 1361, 1445, 1446, 4095, 4096)
K_GRID_STRIDE = ACC_THREADS * ACC_MAX_BLOCKS + 12345               # more pairs than threads: k_accumulate_pairs' grid-stride loop
PERM = np.array([[0, 0, -1], [1, 0, 0], [0, -1, 0]], np.int64)      # a signed permutation (det +1)
SHIFT = np.array([3, -5, 2], np.int64)


@functools.lru_cache(maxsize=None)
def integer_cloud():
    return np.random.default_rng(4242).integers(-8, 9, size=(3, K_GRID_STRIDE)).astype(np.int64)


def integer_pairs_and_sums(K):
    """Integers in [-8, 8] and B = P A + t: every product and every sum is a small integer, exact in float64 in any order."""
    A = np.ascontiguousarray(integer_cloud()[:, :K])
    B = PERM @ A + SHIFT[:, None]
    p = A[:, :1]
    a, b = A - p, B - p
    s = np.zeros(NSUMS, np.int64)
    s[S_A:S_A + 3], s[S_B:S_B + 3] = a.sum(axis=1), b.sum(axis=1)
    s[S_H:S_H + 9] = (b @ a.T).reshape(9)
    s[S_AA], s[S_BB], s[S_K] = (a * a).sum(), (b * b).sum(), K
    assert np.abs(s).max() < 2 ** 52
    return A.astype(np.float64), B.astype(np.float64), s.astype(np.float64)


def check_rows_bitwise(e, K, rows):
    assert min(ACC_MAX_BLOCKS, -(-K // ACC_THREADS)) == rows
    A, B, s = integer_pairs_and_sums(K)
    got, want = e.kabsch(A, B), e.kabsch_from_sums(s, A[:, 0])
    assert got.tobytes() == want.tobytes(), (K, rows, np.abs(got - want).max())
    if K >= ACC_THREADS:
        assert np.abs(want[:3, :3] - PERM).max() <= 1e-12              # (and it is the motion that made B)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_reduction_row_count_edges(eng, rows):
    """The same solve kernel on equal sums gives equal bits, so any difference between oa_kabsch (accumulate, reduce `rows`
    rows, solve) and oa_kabsch_from_sums (exact sums, solve) is a row counted wrongly.  K = 256 rows fills the last
    workgroup, K = 256 rows - 255 leaves it one thread of work."""
    check_rows_bitwise(eng, ACC_THREADS * rows, rows)
    check_rows_bitwise(eng, max(3, ACC_THREADS * rows - (ACC_THREADS - 1)), rows)     # (one row: the fewest pairs a solve takes)


@pytest.mark.gpu
def test_reduction_grid_stride(eng):
    check_rows_bitwise(eng, K_GRID_STRIDE, ACC_MAX_BLOCKS)
