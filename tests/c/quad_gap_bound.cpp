// The rounding bound of level 0's quad gap (object_alignment_amd/csrc/oa_quadgap.hpp), checked on the host against long double:
//     quad_gap(m, w, hm, hw) <= (T + quad_allowance(qmax, h1, h2)) (1 + 2^-23),   T = min over q in {q1, q2}, h in {h1, h2} of |q - h|,
// {m, w} = pair_image(q1, q2), {hm, hw} = point_pair_image(h1, h2), qmax = max(|q1|, |q2|) -- the smallest qmax a target that holds
// the pair can have; and
//     quad_threshold(thr1_a, thr1_b, A) >= (max(sqrt(base_a), sqrt(base_b)) + A)(1 + 2^-22)
// for thr1 as sorted_thresholds forms it, thr1 = round_up((sqrt(base) + pair_allowance)(1 + 2^-22)), and A rounded up to float32 as
// the set-up stores it.  Built with -ffp-contract=off: the three subtractions round separately, as the kernel's do.
// usage: quad_gap_bound [random quadruples]     exit status 1 on the first violation
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "oa_quadgap.hpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    uint64_t x = rng_state;
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    return rng_state = x;
}
static double uni() { return (double)(rnd() >> 11) * 0x1p-53; }               // [0, 1)
static double sgn() { return (rnd() & 1) ? 1.0 : -1.0; }

static long long checked = 0, thresholds = 0;

static float round_up_to_float(double v)
{
    float f = (float)v;
    if ((double)f < v) f = nextafterf(f, INFINITY);
    return f;
}

// one pair of positions (real1 / real2: a vertex, else padding) and one pair of points
static void check(float q1, bool real1, float q2, bool real2, float h1, float h2, const char *what)
{
    float m, w, hm, hw;
    oa::pair_image(q1, real1, q2, real2, m, w);
    oa::point_pair_image(h1, h2, hm, hw);
    const float t = oa::quad_gap(m, w, hm, hw);
    // what level 0 must not overstate: the smallest real gap of the positions the image stands for to either point
    const float p1 = real1 ? q1 : (real2 ? q2 : oa::PAIR_PAD_U), p2 = real2 ? q2 : p1;
    const float qs[2] = { p1, p2 }, hs[2] = { h1, h2 };
    long double T = INFINITY;
    for (float q : qs)
        for (float h : hs) {
            const long double g = fabsl((long double)q - (long double)h);
            if (g < T) T = g;
        }
    const double qmax = fmax(fabs((double)p1), fabs((double)p2));
    const long double bound = (T + (long double)oa::quad_allowance(qmax, h1, h2)) * (1.0L + 0x1p-23L);
    ++checked;
    if (!((long double)t <= bound)) {
        printf("VIOLATION (%s): q1 %.9g%s q2 %.9g%s h1 %.9g h2 %.9g -> m %.9g w %.9g hm %.9g hw %.9g t %.9g > bound %.12Lg (T %.12Lg)\n", what,
               (double)q1, real1 ? "" : " (pad)", (double)q2, real2 ? "" : " (pad)", (double)h1, (double)h2, (double)m, (double)w, (double)hm,
               (double)hw, (double)t, bound, T);
        exit(1);
    }
}

// the threshold of a pair whose points have the right-hand sides base_a, base_b (sorted_thresholds) against its specification
static void check_threshold(double base_a, double base_b, double qmax, float h1, float h2)
{
    const float thr_a = round_up_to_float((sqrt(base_a) + oa::pair_allowance(qmax, h1)) * (1.0 + 0x1p-22));
    const float thr_b = round_up_to_float((sqrt(base_b) + oa::pair_allowance(qmax, h2)) * (1.0 + 0x1p-22));
    const double A = oa::quad_allowance(qmax, h1, h2);
    const float thr = oa::quad_threshold(thr_a, thr_b, round_up_to_float(A));
    const long double sa = sqrtl((long double)base_a), sb = sqrtl((long double)base_b);
    const long double spec = ((sa > sb ? sa : sb) + (long double)A) * (1.0L + 0x1p-22L);
    ++thresholds;
    if (!((long double)thr >= spec)) {
        printf("VIOLATION (threshold): base %.17g %.17g qmax %.9g h %.9g %.9g -> thr1 %.9g %.9g thr %.9g < %.12Lg\n", base_a, base_b, qmax,
               (double)h1, (double)h2, (double)thr_a, (double)thr_b, (double)thr, spec);
        exit(1);
    }
    // an unseeded point (thr1 = +inf) and an allowance of +inf (the set-up's "no claim") must give +inf
    if (!(oa::quad_threshold(INFINITY, thr_b, (float)A) == INFINITY) || !(oa::quad_threshold(thr_a, INFINITY, (float)A) == INFINITY) ||
        !(oa::quad_threshold(thr_a, thr_b, INFINITY) == INFINITY)) {
        printf("VIOLATION (threshold): +inf in does not give +inf out\n");
        exit(1);
    }
}

// every pair of points worth trying against one pair of vertices
static void points(float q1, float q2, double scale, const char *what)
{
    float m, w;
    oa::pair_image(q1, true, q2, true, m, w);
    const float far = (float)(q1 + 1e3 * scale);
    // (h1, h2): Hw = 0, Hw = W, Hw < W, Hw > W, x = 0, |x| = Hw and an ulp to either side, a point on a vertex with its partner far away
    const float hs[][2] = {
        { q1, q1 }, { m, m }, { 0.0f, 0.0f },                                                   // Hw = 0 (h1 = h2)
        { q1, q2 }, { q2, q1 },                                                                  // the points on the vertices: Hw = W, x = 0
        { (float)(q1 + scale), (float)(q2 + scale) }, { (float)(q1 - 3.0 * scale), (float)(q2 - 3.0 * scale) },   // Hw = W, shifted
        { m, (float)(m + 0.25 * ((double)q2 - (double)q1)) },                                    // Hw < W
        { (float)(m - 0.125 * ((double)q2 - (double)q1)), (float)(m + 0.125 * ((double)q2 - (double)q1)) },   // Hw < W, x = 0
        { (float)(m - scale), (float)(m + scale) },                                              // x = 0, Hw > W mostly
        { m, (float)(m + 2.0 * scale) }, { (float)(m - 2.0 * scale), m },                        // |x| = Hw: a point on the midpoint
        { nextafterf(m, INFINITY), (float)(m + 2.0 * scale) }, { nextafterf(m, -INFINITY), (float)(m + 2.0 * scale) },
        { q1, far }, { far, q2 }, { q2, -far },                                                  // best = 0 for one, the partner far away
        { (float)(q1 + w), (float)(q1 + w + 7.0 * scale) },                                      // a vertex pair centred on ... (t = -W)
        { m, (float)(m + 1e4 * scale) }, { (float)(-1e-4 * scale), (float)(1e4 * scale) },
        { nextafterf(q1, -INFINITY), nextafterf(q2, INFINITY) }, { -q1, q2 },
    };
    for (const auto &h : hs) {
        check(q1, true, q2, true, h[0], h[1], what);
        check(q2, true, q1, true, h[1], h[0], what);
        check(q1, true, oa::PAIR_PAD_U, false, h[0], h[1], "vertex + padding");
        check(oa::PAIR_PAD_U, false, oa::PAIR_PAD_U, false, h[0], h[1], "padding + padding");
    }
}

int main(int argc, char **argv)
{
    const long long n_random = argc > 1 ? atoll(argv[1]) : 10000000;
    // adversarial: scales 1e-30 .. 1e18, vertex spreads from the whole scale down to one ulp and to zero (W = 0)
    for (int e = -30; e <= 18; ++e) {
        const double scale = pow(10.0, e);
        for (int k = 0; k < 100; ++k) {
            const float q1 = (float)(sgn() * scale * (0.1 + 0.9 * uni()));
            points(q1, q1, scale, "q1 == q2");
            points(q1, nextafterf(q1, INFINITY), scale, "one ulp apart");
            points(q1, -q1, scale, "mirror images about 0");
            for (int s = 0; s >= -8; --s) points(q1, (float)(q1 + sgn() * scale * pow(10.0, s) * uni()), scale, "spread");
        }
    }
    // offsets of 1e4 with a spacing of 1e-3 (an ulp of float32 there is 9.8e-4)
    for (int k = 0; k < 20000; ++k) {
        const float q1 = (float)(1.0e4 + 1.0e-3 * (double)(rnd() % 40)), q2 = (float)(1.0e4 + 1.0e-3 * (double)(rnd() % 40));
        const float h1 = (float)(1.0e4 + 1.0e-3 * 40.0 * uni()), h2 = (float)(1.0e4 + 1.0e-3 * 40.0 * uni());
        check(q1, true, q2, true, h1, h2, "offset 1e4");
        check(q1, true, q2, true, h1, h1, "offset 1e4");
    }
    const long long n_adversarial = checked;
    // random quadruples: a pair of vertices at a random scale and spread, a pair of points narrower or wider than it, near or far
    for (long long i = 0; i < n_random; ++i) {
        const double scale = pow(10.0, -30.0 + 48.0 * uni());
        const float q1 = (float)(sgn() * scale * uni());
        const double dq = scale * pow(10.0, -8.0 * uni()) * uni();
        const float q2 = (float)(q1 + sgn() * dq);
        const unsigned pick = (unsigned)(rnd() & 7);
        float h1, h2;
        if (pick == 0) h1 = q1;
        else if (pick == 1) { float m, w; oa::pair_image(q1, true, q2, true, m, w); h1 = m; }
        else if (pick == 2) h1 = (float)(sgn() * scale * 10.0 * uni());
        else h1 = (float)(q1 + sgn() * dq * 4.0 * uni());             // within a few spreads of the pair
        const unsigned pick2 = (unsigned)(rnd() & 3);
        if (pick2 == 0) h2 = (float)(h1 + sgn() * dq * pow(10.0, 2.0 - 4.0 * uni()));      // Hw around W, either side of it
        else if (pick2 == 1) h2 = (float)(h1 + sgn() * scale * pow(10.0, -8.0 * uni()) * uni());
        else if (pick2 == 2) h2 = (float)(sgn() * scale * 10.0 * uni());
        else h2 = (float)((double)q1 + (double)q2 - (double)h1);       // mirror image about the vertices' midpoint: x = 0
        check(q1, true, q2, true, h1, h2, "random");
        if ((i & 7) == 0) {
            // thresholds: base = FILTER_ABS (1e-30) at the least, up to the square of a few scales
            const double qmax = fmax(fabs((double)q1), fabs((double)q2)) * (1.0 + 3.0 * uni());
            const double ba = 1e-30 + pow(scale * pow(10.0, 1.0 - 9.0 * uni()), 2.0), bb = (rnd() & 1) ? ba : 1e-30 + pow(scale * pow(10.0, 1.0 - 9.0 * uni()), 2.0);
            check_threshold(ba, bb, qmax, h1, h2);
        }
    }
    printf("quad_gap_bound: %lld adversarial + %lld random quadruples, %lld thresholds, 0 violations\n", n_adversarial, checked - n_adversarial,
           thresholds);
    return 0;
}
