// oa_octgap.hpp -- level 0 of k_nn_search_sorted on QUADS of vertices and pairs of points (round 18): the functions the upload, the
// point set-up, the kernel and its threshold share.  Compiles for the device and, without a GPU, for the host
// (tests/test_oct_gap_bound.py runs this very code against long double).
//
// A group of 4 sorted positions holds two vertex pairs with the images {Ma, Wa}, {Mb, Wb} along u (pair_image, oa_pairgap.hpp); a
// lane's points 2p, 2p + 1 have {Hm, Hw} (oa_quadgap.hpp).  With a cap c >= 0, one number per target:
//     MM = (Ma + Mb) / 2,   WW = |Mb - Ma| / 2,   B = min(WW, c),   S = max(Wa, Wb) + (WW - B)            (the quad's image {MM, B, S})
//     A = max(Hw, c),       e = |A - Hw|                                                                  (the point pair's {Hm, A})
// The eight gaps |q - h| are |X - o|, X = MM - Hm, o = s3 Hw - s1 WW - s2 W(s1), s1, s2, s3 = +-1; let T be the smallest of them.
// The kernel computes the SIGNED value
//     t = | | |X| - A | - B | - S                                                   (four subtractions for eight (vertex, point) pairs)
// and t > Thr + e proves T > Thr: all eight pairs are losers.  The min tree takes t as it is, without |.|.
//
// (1) Real numbers, A >= B >= 0:  D = ||X| - A| - B| is the distance from X to the set {+-A +- B} -- with p = |X|, D = |p - A - B| for
//     p >= A, D = |A - B - p| for p <= A (A - p >= 0 is compared with B), and these are the distances to A + B and A - B, the two
//     nearest members for p >= 0.  (In the other order D overstates: X = 0.25, A = 0.5, B = 1 gives 0.75 against the true 0.25.
//     Hence the cap: B <= c <= A by construction, whatever the widths.)  Every offset o lies within S + e of the member
//     s3 A - s1 B:  |o - (s3 A - s1 B)| <= |Hw - A| + |WW - B| + W(s1) <= e + (WW - B) + max(Wa, Wb).  So for the o of the smallest gap
//         D <= |X - (s3 A - s1 B)| <= T + S + e,        t = D - S <= T + e.
//     Any c >= 0 is valid; c only tunes what the bound loses: the narrower pair counts as wide as the wider, a quad whose pairs lie
//     further apart than 2 c degrades towards an interval, a lane whose two points nearly share their u pays e <= c of reach.
// (2) float32, u = 2^-24.  The point pair's hw' = fl(max(Hw, c)) is taken AS the real A of (1) -- e is formed in double from the
//     float that is stored, so A carries no rounding -- and ww = fl(B) <= c <= hw' because rounding is monotone and c is a float:
//     the order of (1) holds for the numbers the instructions see.  mm = fl(MM), ws = fl(S), hm = fl(Hm),
//         x = fl(mm - hm),  y = fl(|x| - hw'),  z = fl(|y| - ww),  t = fl(|z| - ws).
//     Against the real chain X, Y = |X| - A, Z = |Y| - B, t* = |Z| - S:
//         |x - X| <= |mm - MM| + |hm - Hm| + u |mm - hm|               <= u (qmax + hmax + (qmax + hmax))
//         |y - Y| <= |x - X| + u ||x| - hw'|                           ||x| - hw'| <= max(|x|, hw') <= (qmax + hmax + c)(1 + u)
//         |z - Z| <= |y - Y| + |ww - B| + u ||y| - ww|                 |ww - B| <= u qmax,  ||y| - ww| <= (qmax + hmax + c)(1 + u)^2
//         |z| - ws <= t* + |z - Z| + |ws - S|                          |ws - S| <= u S <= 2 u qmax       (Wa, Wb, WW <= qmax)
//     with qmax the largest |q| of the target and hmax = max(|h1|, |h2|).  The sum is u (7 qmax + 4 hmax + 2 c) and terms of u^2
//     times at most three times as much; the images are rounded from double sums that are themselves rounded (2^-53 relative per
//     operation, at most 2^-50 qmax in S), and e from a double Hw (2^-53 hmax).  All of it is inside
//         Aq = oct_allowance = u (8 qmax + 5 hmax + 3 c):        |z| - ws <= t* + Aq - u (qmax + hmax + c) / 2,
//     and t = fl(|z| - ws) <= (|z| - ws)(1 + u) when that is >= 0, t <= 0 otherwise.  So, as oa_quadgap.hpp (2),
//         t <= (T + e + Aq)(1 + 2^-23).
// (3) The threshold.  The set-up stores Q = round_up(Aq + e) and the kernel forms Thr = quad_threshold(thr1_a, thr1_b, Q)
//     >= (max(sqrt(base_a), sqrt(base_b)) + Aq + e)(1 + 2^-22) (oa_quadgap.hpp (3), unchanged).  t > Thr  =>  (T + e + Aq)(1 + 2^-23)
//     > (max(..) + Aq + e)(1 + 2^-22)  =>  T > sqrt(base) of BOTH points.
// (4) Flushed denormals: each of mm, ww, ws, hm, hw', x, y, z, t moves by less than 2^-126 when flushed, monotonely (ww <= hw'
//     stays true): 2^-122 in all, against thr1 >= sqrt(FILTER_ABS) = 1e-15 whose 2^-23 of slack is 1e-22.
// (5) Padding positions of the target (pair_image's rules first: (vertex, padding) is {q, 0}, (padding, padding) {1e18, 0}).  A
//     quad of a pair that holds a vertex and a pair of padding alone is the first pair as it is: {Ma, 0, Wa} -- the octuple
//     q1, q2, q1, q2 with WW = 0, covered by (1) and (2), never the cancellation |1e18 - h| - 5e17.  A quad of padding alone is
//     {1e18, 0, 0}: t = ||1e18 - hm| - hw'|, some value or other for vertices that can never win -- a hit it causes is wasted work,
//     a skip is right.  A quad whose second pair is (vertex, padding) is an ordinary quad with Wb = 0.
// (6) Where the bound is not claimed the set-up stores Q = +inf as before (oa_quadgap.hpp (6)): a point whose hu is not finite, a
//     real slot of the source paired with a padding slot.  c = +inf (or a Hw that overflows) gives e = +inf and the same.
#pragma once

#include "oa_quadgap.hpp"

namespace oa {

// The image {mm, ww, ws} of a group's two vertex pairs {ma, wa}, {mb, wb} (pair_image's floats) under the cap c, formed in double
// and rounded once.  real_a / real_b: the pair holds at least one vertex (padding only ever follows the vertices).
OA_PAIRGAP_FN void quad_image(float ma, float wa, bool real_a, float mb, float wb, bool real_b, float c, float &mm, float &ww, float &ws)
{
    if (real_a && real_b) {
        const double MM = ((double)ma + (double)mb) / 2.0;
        const double WW = __builtin_fabs((double)mb - (double)ma) / 2.0;
        const double B = WW < (double)c ? WW : (double)c;
        const double W = (double)(wa > wb ? wa : wb);
        mm = (float)MM; ww = (float)B; ws = (float)(W + (WW - B));
    } else if (real_a) {
        mm = ma; ww = 0.0f; ws = wa;
    } else {
        mm = PAIR_PAD_U; ww = 0.0f; ws = 0.0f;
    }
}

// The image {hm, hw'} of the lane's two points under the cap c, and e = |hw' - Hw| in double from the float hw' that is stored.
OA_PAIRGAP_FN void point_pair_image_capped(float h1, float h2, float c, float &hm, float &hwc, double &e)
{
    const double Hw = __builtin_fabs((double)h2 - (double)h1) / 2.0;
    hm = (float)(((double)h1 + (double)h2) / 2.0);
    hwc = (float)(Hw > (double)c ? Hw : (double)c);
    e = __builtin_fabs((double)hwc - Hw);
}

// t = fl(|fl(|fl(|fl(mm - hm)| - hw')| - ww)| - ws), SIGNED: four subtractions, each |.| a source modifier of the next one.
OA_PAIRGAP_FN float oct_gap(float mm, float ww, float ws, float hm, float hwc)
{
    const float x = mm - hm;
    const float y = __builtin_fabsf(x) - hwc;
    const float z = __builtin_fabsf(y) - ww;
    return __builtin_fabsf(z) - ws;
}

// what rounding can add to t over T + e (header, (2)): 2^-24 (8 qmax + 5 max(|h1|, |h2|) + 3 c)
OA_PAIRGAP_FN double oct_allowance(double qmax, float h1, float h2, float c)
{
    const double a1 = __builtin_fabs((double)h1), a2 = __builtin_fabs((double)h2);
    return 0x1p-24 * (8.0 * qmax + 5.0 * (a1 > a2 ? a1 : a2) + 3.0 * (double)c);
}

}  // namespace oa
