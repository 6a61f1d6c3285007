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
//
// Round 19: level 0 on GROUPS of V = 8 or 16 sorted positions (group_image<V> below; V = 4 is quad_image above, untouched).  The chain
// of four subtractions, the point pair's {hm, hw' = max(Hw, c)}, e and the threshold are the same; only the image changes, and it is
// defined by a property of the floats that are stored rather than by a formula:
//     (P)  0 <= ww <= c,  ws >= 0,  and every real q_j of the group lies within ws of mm + ww or of mm - ww     (as real numbers,
//          for the float32 mm, ww, ws as stored).
// (1') Real numbers, A = hw' >= c >= ww = B.  Let q*, h be the vertex and the point of the smallest of the 2V gaps, T = |q* - h|.
//     By (P) q* = mm + s1 ww + d with |d| <= ws, and h = Hm + s3 Hw.  With X = mm - Hm:  X - (s3 A - s1 B) = (q* - h) - d - s3 (A - Hw),
//     so |X - (s3 A - s1 B)| <= T + ws + e, and D = |||X| - A| - B| is the distance from X to the nearest of {+-A +- B} ((1), which
//     needs only A >= B >= 0):  D <= T + ws + e,  t = D - ws <= T + e.  ws stands where (1) has W(s1) + (WW - B).
// (2') float32.  mm, ww, ws ARE the reals of (1'): (P) is a statement about the stored floats, so the terms |mm - MM|, |ww - B|,
//     |ws - S| of (2) vanish.  What is left is |hm - Hm| and the four subtractions' own roundings, u (3 qmax + 4 hmax + 2 c) by (2)'s
//     lines with |mm|, ww <= qmax (mm lies between the group's smallest and largest q, rounding being monotone; ww is half a
//     distance of two such centres) -- inside oct_allowance = u (8 qmax + 5 hmax + 3 c) as it stands:
//     k_sorted_point_setup and quad_threshold are unchanged, and (3) holds word for word.
//     How group_image makes (P) true: mm and ww are rounded from double (any rounding is allowed: (P) is evaluated afterwards; ww <=
//     c because rounding is monotone and c is a float), then for every real q_j the two distances |q_j - (mm -+ ww)| are evaluated
//     in double FROM THE FLOATS mm, ww and bounded from above: s = fl64(mm + ww) is off by at most 2^-53 (|mm| + ww) (exact when ww =
//     0), fl64(q_j - s) by 2^-53 relative, so  |q_j - (mm + ww)| <= fl64|q_j - s| (1 + 2^-51) + 2^-52 (|mm| + ww) [ww > 0]  with room
//     for the roundings of that expression itself.  ws is the largest over j of the smaller of the two, rounded UP to float32.  A
//     group of duplicates has mm = q, ww = 0 and every distance exactly 0: ws = 0.
// (4') Flushed denormals: as (4); a flushed ws or ww moves t by less than 2^-126.
// (5') Padding (only ever after the vertices).  Only real positions enter the centres and ws.  A group whose second half is all
//     padding is the group of its first half, group_image<V / 2> (down to one vertex: {q, 0, 0}); a group of padding alone is
//     {1e18, 0, 0} as (5).  1e18 never meets a vertex in one expression.
// (6') Non-finite hu, a real slot beside a padding slot, c = +inf: Q = +inf from the set-up, as (6).  The target's q are finite
//     (the images are only built for a finite target); a NaN q_j would drop out of every comparison here and can never win.
#pragma once

#include "oa_quadgap.hpp"

namespace oa {

// the smallest float32 >= v, for v >= 0 (or v = +inf)
OA_PAIRGAP_FN float octgap_round_up(double v)
{
    float f = (float)v;
    if ((double)f < v) {
        unsigned b;
        __builtin_memcpy(&b, &f, 4);
        ++b;
        __builtin_memcpy(&f, &b, 4);
    }
    return f;
}

// The image {mm, ww, ws} of V consecutive sorted positions with the centred float32 u q[0 .. V), the first n_real of them vertices,
// under the cap c: property (P) of the header, (2').  mm and ww from the centres of the two halves (a half's centre: the midpoint
// of its smallest and largest real q), ws from the stored mm and ww.
template <int V>
OA_PAIRGAP_FN void group_image(const float *q, int n_real, float c, float &mm, float &ww, float &ws)
{
    static_assert(V == 1 || V == 2 || V == 4 || V == 8 || V == 16, "group_image: halves of halves");
    if (n_real <= 0) { mm = PAIR_PAD_U; ww = 0.0f; ws = 0.0f; return; }
    if constexpr (V == 1) { mm = q[0]; ww = 0.0f; ws = 0.0f; return; }
    else {
        if (n_real <= V / 2) { group_image<V / 2>(q, n_real, c, mm, ww, ws); return; }
        const int n = n_real < V ? n_real : V;
        double lo_a = (double)q[0], hi_a = lo_a, lo_b = (double)q[V / 2], hi_b = lo_b;
        for (int k = 1; k < V / 2; ++k) { const double v = (double)q[k]; lo_a = v < lo_a ? v : lo_a; hi_a = v > hi_a ? v : hi_a; }
        for (int k = V / 2 + 1; k < n; ++k) { const double v = (double)q[k]; lo_b = v < lo_b ? v : lo_b; hi_b = v > hi_b ? v : hi_b; }
        const double Ca = (lo_a + hi_a) / 2.0, Cb = (lo_b + hi_b) / 2.0;
        const double WW = __builtin_fabs(Cb - Ca) / 2.0;
        mm = (float)((Ca + Cb) / 2.0);
        ww = (float)(WW < (double)c ? WW : (double)c);
        const double sp = (double)mm + (double)ww, sm = (double)mm - (double)ww;
        const double slack = ww > 0.0f ? 0x1p-52 * (__builtin_fabs((double)mm) + (double)ww) : 0.0;
        double S = 0.0;
        for (int k = 0; k < n; ++k) {
            const double dp = __builtin_fabs((double)q[k] - sp), dm = __builtin_fabs((double)q[k] - sm);
            const double d = (dp < dm ? dp : dm) * (1.0 + 0x1p-51) + slack;
            S = d > S ? d : S;
        }
        ws = octgap_round_up(S);
    }
}

// The image {mm, ww, ws} of a group's two vertex pairs {ma, wa}, {mb, wb} (pair_image's floats) under the cap c, formed in double
// and rounded once.  real_a / real_b: the pair holds at least one vertex (padding only ever follows the vertices).
// (No device caller: kept because tests/c/oct_gap_bound.cpp checks (1)-(6) through it, and (1')-(6') build on them.)
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
