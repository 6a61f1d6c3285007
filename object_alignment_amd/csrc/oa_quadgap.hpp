// oa_quadgap.hpp -- level 0 of k_nn_search_sorted on pairs of vertices AND pairs of points (round 13): the functions the point
// set-up, the kernel and its threshold share.  Compiles for the device and, without a GPU, for the host
// (tests/test_quad_gap_bound.py runs this very code against long double).
//
// A lane's points r = 2p, 2p + 1 have the u-coordinates h1, h2:  Hm = (h1 + h2) / 2, Hw = |h2 - h1| / 2.  A pair of vertices has
// M = (q1 + q2) / 2, W = |q2 - q1| / 2 (oa_pairgap.hpp).  The four gaps |q - h| are |x + s W + s' Hw|, x = M - Hm, s, s' = +-1;
// let T be the smallest of them.  The kernel computes the SIGNED value
//     t = | |x| - Hw | - W                                                          (three subtractions for four (vertex, point) pairs)
// and t > Thr proves T > Thr: all four pairs are losers.  The min tree takes t as it is, without |.|.
//
// (1) Real numbers: t <= T for every Hw, W >= 0, in either order.  With p = |x| the four gaps are, by the symmetry x -> -x,
//     |p - Hw - W|, |p - Hw + W|, |p + Hw - W|, |p + Hw + W|.  The first two are >= |p - Hw| - W (reverse triangle inequality);
//     the last two are >= |p + Hw| - W >= |p - Hw| - W because p, Hw >= 0.  For Hw >= W and t >= 0, t IS T (the zeros of T are the
//     symmetric set {+-Hw +- W} and t is the distance to it); for Hw < W, or t < 0 (a vertex pair within W of a point: a hit
//     anyway), t only understates.  Nothing depends on which of Hw, W is larger, nor on how the slots were paired.
// (2) float32, u = 2^-24: m = fl(M), w = fl(W), hm = fl(Hm), hw = fl(Hw), x = fl(m - hm), y = fl(|x| - hw), t = fl(|y| - w).
//     Against the real chain X = M - Hm, Y = |X| - Hw, t* = |Y| - W:
//         |x - X| <= |m - M| + |hm - Hm| + u |m - hm|                  <= u (|M| + |Hm| + |m - hm|)
//         |y - Y| <= |x - X| + |hw - Hw| + u ||x| - hw|                (||a| - |b|| <= |a - b|)
//         z = |y| - w <= t* + d,   d = u (|M| + |Hm| + |m - hm| + Hw + ||x| - hw| + W)
//     and t = fl(z) <= z (1 + u) when z >= 0, t <= 0 otherwise.  With qmax the largest |q| of the target, hmax = max(|h1|, |h2|):
//     |M|, W, |m| <= qmax;  |Hm|, Hw, |hm|, hw <= hmax (rounding is monotone);  |m - hm| <= qmax + hmax;
//     ||x| - hw| <= max(|x|, hw) <= (qmax + hmax)(1 + u).  So
//         d <= u (4 qmax + 4 hmax) + u^2 (qmax + hmax) <= A + u^2 qmax,       A = quad_allowance = u (4 qmax + 5 hmax),
//         t <= (T + A + u^2 qmax)(1 + u) <= (T + A)(1 + u) + u (T + A) = (T + A)(1 + 2^-23)         (u^2 qmax (1 + u) <= u A).
//     (m, w, hm, hw are rounded from double sums that are themselves rounded when the exponents lie far apart: u (1 + 2^-29) in
//     place of u, inside the step from 2^-23 to the 2^-22 of the threshold.)
// (3) The threshold.  thr1 of point r (sorted_thresholds) is >= (sqrt(base_r) + pair_allowance)(1 + 2^-22) > sqrt(base_r), and a
//     vertex whose real gap along u exceeds sqrt(base_r) is a proven loser for point r.  With
//         Thr = quad_threshold(thr1_a, thr1_b, A) >= (max(sqrt(base_a), sqrt(base_b)) + A)(1 + 2^-22),
//     t > Thr  =>  (T + A)(1 + 2^-23) > (max(..) + A)(1 + 2^-22)  =>  T > sqrt(base) of BOTH points: the max rule -- the pair is
//     skipped only when the point with the larger reach could skip it.  quad_threshold in float32: s = fl(max(thr1) + A) >=
//     (max(thr1) + A)(1 - u), Thr = fl(s + 2^-21 s) >= s (1 + 2^-21)(1 - u) >= (max(thr1) + A)(1 + 2^-22).  +inf in gives +inf out.
// (4) Flushed denormals: each of m, w, hm, hw, x, y, t moves by less than 2^-126 when flushed, A by as much: 2^-123 in all, against
//     thr1 >= sqrt(FILTER_ABS) = 1e-15 whose 2^-23 of slack is 1e-22.
// (5) Padding positions of the target: the image {1e18, 0} of (padding, padding) gives t = ||1e18 - hm| - hw|, some value or other
//     for vertices that can never win -- a hit it causes is wasted work, a skip is right.  (vertex, padding) is {q1, 0}: the
//     quadruple q1, q1, h1, h2 with W = 0, covered by (1) and (2).
// (6) A threshold that is too high only prunes less: a hit marks the block for both points of the pair, and level 0v and levels
//     1-3 decide per point as they always did.  So where the bound is not claimed the set-up stores A = +inf (Thr = +inf, t > Thr never true, NaN
//     included): a point whose hu is not finite, and a pair of one real slot with one padding slot of the source.  An unseeded
//     point has thr1 = +inf and the max rule does the same.
#pragma once

#include "oa_pairgap.hpp"

namespace oa {

// The image {hm, hw} of the lane's two points, formed in double and rounded once, as pair_image.
OA_PAIRGAP_FN void point_pair_image(float h1, float h2, float &hm, float &hw)
{
    hm = (float)(((double)h1 + (double)h2) / 2.0);
    hw = (float)(__builtin_fabs((double)h2 - (double)h1) / 2.0);
}

// t = fl(|fl(|fl(m - hm)| - hw)| - w), SIGNED: three subtractions, both |.| source modifiers of the subtraction that follows.
OA_PAIRGAP_FN float quad_gap(float m, float w, float hm, float hw)
{
    const float x = m - hm;
    const float y = __builtin_fabsf(x) - hw;
    return __builtin_fabsf(y) - w;
}

// what rounding can add to t over the real smallest gap (header, (2)): 2^-24 (4 qmax + 5 max(|h1|, |h2|))
OA_PAIRGAP_FN double quad_allowance(double qmax, float h1, float h2)
{
    const double a1 = __builtin_fabs((double)h1), a2 = __builtin_fabs((double)h2);
    return 0x1p-24 * (4.0 * qmax + 5.0 * (a1 > a2 ? a1 : a2));
}

// the pair's threshold from its points' thr1 and its allowance (rounded UP to float32 by the set-up): header, (3)
OA_PAIRGAP_FN float quad_threshold(float thr1_a, float thr1_b, float allowance)
{
    const float s = (thr1_a > thr1_b ? thr1_a : thr1_b) + allowance;
    return __builtin_fmaf(s, 0x1p-21f, s);
}

}  // namespace oa
