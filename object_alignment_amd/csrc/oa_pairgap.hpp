// oa_pairgap.hpp -- level 0 of k_nn_search_sorted on PAIRS of vertices (round 11): the three functions the upload, the kernel and
// the thresholds share.  Compiles for the device and, without a GPU, for the host (tests/test_pair_gap_bound.py runs this very
// code against long double).
//
// Two vertices q1, q2 along u and a point h:  with M = (q1 + q2) / 2 and W = |q2 - q1| / 2,
//     min(|q1 - h|, |q2 - h|) = | |M - h| - W |            (x = h - M: the gaps are |x + W|, |x - W|; for W >= 0 their minimum is ||x| - W|)
// so the smaller of a pair's two gaps costs two subtractions -- as the two gaps did -- and NO comparison.
// In float32, with m = fl(M), w = fl(W), s = fl(m - h), a = fl(|s| - w) and u = 2^-24:
//     |s| - w  =  |M - h| - W + d,   |d| <= |m - M| + u |m - h| + |w - W| <= u (|M| + |m - h| + W)
//     |a| <= (g + u (|M| + |m - h| + W)) (1 + u),        g = ||M - h| - W| the real smaller gap
// and with |M| <= qmax, W <= qmax, |m - h| <= qmax + |h| (qmax: the largest |q| of the target, which bounds every |qu|; rounding
// is monotone, so |m| <= qmax too):
//     |a| <= (g + pair_allowance(qmax, h)) (1 + u),      pair_allowance = u (3 qmax + |h|).
// (m and w are rounded from double sums that are themselves rounded when the two exponents lie more than 29 apart: u (1 + 2^-29)
// instead of u, inside the 2^-22 the threshold adds -- sorted_thresholds, oa_kernels.hpp.  A denormal s or w flushed to zero moves
// |a| by at most 2^-126 each: the threshold is never below sqrt(FILTER_ABS) = 1e-15, whose 2^-22 is 2e-22.)
#pragma once

#if defined(__HIPCC__)
#define OA_PAIRGAP_FN __host__ __device__ __forceinline__
#else
#define OA_PAIRGAP_FN inline
#endif

namespace oa {

constexpr float PAIR_PAD_U = 1.0e18f;       // k_pack_sorted's u of a padding position (beyond every vertex, -2 u finite)

// The image {m, w} of the pair of sorted positions that hold q1 and q2 (the centred float32 u of tfs).  real1 / real2: the
// position holds a vertex (padding only ever follows the vertices).  Padding never reaches the cancellation |1e18 - h| - 5e17:
// a (vertex, padding) pair is the vertex alone, a (padding, padding) pair is padding alone -- both with w = 0, where a = |m - h|
// is the gap level 0 computed until round 10.  (The images are only built for a finite target: build_filter, oa_icp.hip.)
OA_PAIRGAP_FN void pair_image(float q1, bool real1, float q2, bool real2, float &m, float &w)
{
    w = 0.0f;
    if (real1 && real2) {
        m = (float)(((double)q1 + (double)q2) / 2.0);
        w = (float)(__builtin_fabs((double)q2 - (double)q1) / 2.0);
    } else
        m = real1 ? q1 : (real2 ? q2 : PAIR_PAD_U);
}

// |a|, a = fl(|fl(m - h)| - w): two subtractions, the inner |.| a source modifier of the second, the outer one of the min tree's
// v_min3_f32 (as the single gap's was).
OA_PAIRGAP_FN float pair_gap(float m, float w, float h)
{
    const float s = m - h;
    return __builtin_fabsf(__builtin_fabsf(s) - w);
}

// what rounding can add to |a| over the real gap (header): 2^-24 (3 qmax + |h|)
OA_PAIRGAP_FN double pair_allowance(double qmax, float h)
{
    return 0x1p-24 * (3.0 * qmax + __builtin_fabs((double)h));
}

}  // namespace oa
