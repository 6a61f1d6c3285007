// The rounding bound of level 0's oct gap (object_alignment_amd/csrc/oa_octgap.hpp), checked on the host against long double:
//     oct_gap(mm, ww, ws, hm, hw') <= (T + oct_allowance(qmax, h1, h2, c) + e) (1 + 2^-23),
// T = min over the positions q the quad's image stands for and h in {h1, h2} of |q - h|, {mm, ww, ws} = quad_image of the two
// pair_images under the cap c, {hm, hw', e} = point_pair_image_capped(h1, h2, c), qmax = the largest |q| of those positions -- the
// smallest qmax a target that holds the quad can have; and
//     quad_threshold(thr1_a, thr1_b, Q) >= (max(sqrt(base_a), sqrt(base_b)) + A + e)(1 + 2^-22),    Q = round_up(A + e)
// for thr1 as sorted_thresholds forms it and Q as the set-up stores it.  Built with -ffp-contract=off: the four subtractions round
// separately, as the kernel's do.
// usage: oct_gap_bound [random octuples]     exit status 1 on the first violation
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "oa_octgap.hpp"

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

// one group of four positions, the first n_real of them vertices (padding only ever follows the vertices), one pair of points, a cap
static void check(const float q[4], int n_real, float h1, float h2, float c, const char *what)
{
    float ma, wa, mb, wb, mm, ww, ws, hm, hwc;
    double e;
    oa::pair_image(q[0], n_real > 0, q[1], n_real > 1, ma, wa);
    oa::pair_image(q[2], n_real > 2, q[3], n_real > 3, mb, wb);
    oa::quad_image(ma, wa, n_real > 0, mb, wb, n_real > 2, c, mm, ww, ws);
    oa::point_pair_image_capped(h1, h2, c, hm, hwc, e);
    const float t = oa::oct_gap(mm, ww, ws, hm, hwc);
    // what level 0 must not overstate: the smallest real gap of the positions the image stands for to either point
    const float pad = oa::PAIR_PAD_U;
    const float hs[2] = { h1, h2 };
    long double T = INFINITY;
    double qmax = 0.0;
    for (int k = 0; k < (n_real > 0 ? n_real : 1); ++k) {
        const float p = n_real > 0 ? q[k] : pad;
        qmax = fmax(qmax, fabs((double)p));
        for (float h : hs) {
            const long double g = fabsl((long double)p - (long double)h);
            if (g < T) T = g;
        }
    }
    const long double bound = (T + (long double)oa::oct_allowance(qmax, h1, h2, c) + (long double)e) * (1.0L + 0x1p-23L);
    ++checked;
    // the order the proof rests on, for the floats the instructions see
    if (!((long double)t <= bound) || !(ww <= hwc) || !(ww >= 0.0f) || !(ws >= 0.0f) || !(e >= 0.0)) {
        printf("VIOLATION (%s): q %.9g %.9g %.9g %.9g (%d real) h1 %.9g h2 %.9g c %.9g -> mm %.9g ww %.9g ws %.9g hm %.9g hw' %.9g e %.9g t %.9g > "
               "bound %.12Lg (T %.12Lg)\n", what, (double)q[0], (double)q[1], (double)q[2], (double)q[3], n_real, (double)h1, (double)h2, (double)c,
               (double)mm, (double)ww, (double)ws, (double)hm, (double)hwc, e, (double)t, bound, T);
        exit(1);
    }
}

// the padding rules' images, said once more: what the kernel reads must be exactly this
static void check_padding_images(float q1, float q2, float q3, float c)
{
    float ma, wa, mb, wb, mm, ww, ws;
    bool ok = true;
    oa::pair_image(q1, true, q2, true, ma, wa); oa::pair_image(0.f, false, 0.f, false, mb, wb);
    oa::quad_image(ma, wa, true, mb, wb, false, c, mm, ww, ws);
    ok = ok && mm == ma && ww == 0.0f && ws == wa;                              // (real, padding): the real pair with ww = 0
    oa::pair_image(q1, true, 0.f, false, ma, wa);
    oa::quad_image(ma, wa, true, mb, wb, false, c, mm, ww, ws);
    ok = ok && mm == q1 && ww == 0.0f && ws == 0.0f;                            // one vertex: itself
    oa::pair_image(0.f, false, 0.f, false, ma, wa);
    oa::quad_image(ma, wa, false, mb, wb, false, c, mm, ww, ws);
    ok = ok && mm == oa::PAIR_PAD_U && ww == 0.0f && ws == 0.0f;                // all padding
    oa::pair_image(q3, true, 0.f, false, mb, wb);
    ok = ok && mb == q3 && wb == 0.0f;                                          // (vertex, padding) keeps w = 0
    if (!ok) { printf("VIOLATION (padding images): q %.9g %.9g %.9g c %.9g\n", (double)q1, (double)q2, (double)q3, (double)c); exit(1); }
}

// the threshold of a pair whose points have the right-hand sides base_a, base_b (sorted_thresholds) against its specification
static void check_threshold(double base_a, double base_b, double qmax, float h1, float h2, float c)
{
    const float thr_a = round_up_to_float((sqrt(base_a) + oa::pair_allowance(qmax, h1)) * (1.0 + 0x1p-22));
    const float thr_b = round_up_to_float((sqrt(base_b) + oa::pair_allowance(qmax, h2)) * (1.0 + 0x1p-22));
    float hm, hwc;
    double e;
    oa::point_pair_image_capped(h1, h2, c, hm, hwc, e);
    const double A = oa::oct_allowance(qmax, h1, h2, c);
    const float thr = oa::quad_threshold(thr_a, thr_b, round_up_to_float(A + e));
    const long double sa = sqrtl((long double)base_a), sb = sqrtl((long double)base_b);
    const long double spec = ((sa > sb ? sa : sb) + (long double)A + (long double)e) * (1.0L + 0x1p-22L);
    ++thresholds;
    if (!((long double)thr >= spec)) {
        printf("VIOLATION (threshold): base %.17g %.17g qmax %.9g h %.9g %.9g c %.9g -> thr1 %.9g %.9g thr %.9g < %.12Lg\n", base_a, base_b, qmax,
               (double)h1, (double)h2, (double)c, (double)thr_a, (double)thr_b, (double)thr, spec);
        exit(1);
    }
    if (!(oa::quad_threshold(INFINITY, thr_b, (float)A) == INFINITY) || !(oa::quad_threshold(thr_a, thr_b, INFINITY) == INFINITY)) {
        printf("VIOLATION (threshold): +inf in does not give +inf out\n");
        exit(1);
    }
}

// every pair of points and every cap worth trying against one group of four vertices
static void points(const float q[4], double scale, const char *what)
{
    float ma, wa, mb, wb;
    oa::pair_image(q[0], true, q[1], true, ma, wa);
    oa::pair_image(q[2], true, q[3], true, mb, wb);
    const double MM = ((double)ma + (double)mb) / 2.0, WW = fabs((double)mb - (double)ma) / 2.0;
    const float far = (float)(q[0] + 1e3 * scale);
    // the caps: 0, tiny, WW itself and an ulp to either side (WW = c), half and twice it (WW > c, WW < c), the wider w, the scale, huge
    const float caps[] = { 0.0f, (float)(1e-6 * scale), (float)WW, nextafterf((float)WW, INFINITY), nextafterf((float)WW, -INFINITY) < 0.f ? 0.f : nextafterf((float)WW, -INFINITY),
                           (float)(0.5 * WW), (float)(2.0 * WW), wa > wb ? wa : wb, (float)scale, (float)(1e6 * scale), 1.0e30f };
    for (const float c : caps) {
        float m4, w4, s4;
        oa::quad_image(ma, wa, true, mb, wb, true, c, m4, w4, s4);
        const double A = (double)c;                                             // hw' of the lanes with Hw <= c
        // (h1, h2): Hw = 0, Hw = c, Hw < c, Hw > c; X = 0; |X| = hw' and ||X| - hw'| = WW' and an ulp to either side of each; a point on a
        // vertex with everything else far away
        const float hs[][2] = {
            { q[0], q[0] }, { q[3], q[3] }, { (float)MM, (float)MM }, { 0.0f, 0.0f },                     // Hw = 0
            { (float)(MM - A), (float)(MM + A) }, { (float)(q[0] - A), (float)(q[0] + A) },                  // Hw = c
            { (float)(MM - 0.5 * A), (float)(MM + 0.5 * A) }, { q[1], (float)(q[1] + 0.25 * A) },            // Hw < c
            { (float)(MM - 3.0 * A - scale), (float)(MM + 3.0 * A + scale) }, { q[0], q[3] }, { q[1], q[2] }, { q[3], q[0] },   // Hw > c mostly
            { (float)(MM + A), (float)(MM + A) }, { nextafterf((float)(MM + A), INFINITY), (float)(MM + A) },   // |X| = hw' (Hw = 0)
            { nextafterf((float)(MM + A), -INFINITY), nextafterf((float)(MM + A), -INFINITY) },
            { (float)(MM - A), (float)(MM - A) }, { (float)(MM + 2.0 * A), (float)MM }, { (float)(MM - 2.0 * A), (float)MM },
            { (float)(MM + A + w4), (float)(MM + A + w4) }, { (float)(MM + A - w4), (float)(MM + A - w4) },   // ||X| - hw'| = WW'
            { nextafterf((float)(MM + A + w4), INFINITY), (float)(MM + A + w4) }, { nextafterf((float)(MM + A - w4), -INFINITY), (float)(MM + A - w4) },
            { (float)(MM - A - w4), (float)(MM - A - w4) }, { (float)(MM - A + w4), nextafterf((float)(MM - A + w4), INFINITY) },
            { q[0], far }, { far, q[1] }, { q[2], -far }, { q[3], far }, { -far, q[3] },                    // best = 0 for one, the partner far away
            { (float)(MM + 1e4 * scale), (float)MM }, { (float)(-1e-4 * scale), (float)(1e4 * scale) },
            { nextafterf(q[0], -INFINITY), nextafterf(q[3], INFINITY) }, { -q[0], q[3] },
        };
        for (const auto &h : hs) {
            check(q, 4, h[0], h[1], c, what);
            const float r[4] = { q[3], q[2], q[1], q[0] }, s[4] = { q[0], q[2], q[1], q[3] };
            check(r, 4, h[1], h[0], c, what);
            check(s, 4, h[0], h[1], c, what);                                   // (any pairing of the four)
            check(q, 3, h[0], h[1], c, "three vertices + padding");
            check(q, 2, h[0], h[1], c, "a pair + a pair of padding");
            check(q, 1, h[0], h[1], c, "one vertex + padding");
            check(q, 0, h[0], h[1], c, "padding alone");
        }
        check_padding_images(q[0], q[1], q[2], c);
    }
}

int main(int argc, char **argv)
{
    const long long n_random = argc > 1 ? atoll(argv[1]) : 10000000;
    // adversarial: scales 1e-30 .. 1e18; the pairs' widths equal, orders of magnitude apart, zero; the pairs on top of each other
    // (WW = 0), an ulp apart, far apart (WW > c for the small caps)
    for (int e = -30; e <= 18; ++e) {
        const double scale = pow(10.0, e);
        for (int k = 0; k < 6; ++k) {
            const float q1 = (float)(sgn() * scale * (0.1 + 0.9 * uni()));
            { const float q[4] = { q1, q1, q1, q1 }; points(q, scale, "a lattice: WW = w = 0"); }
            { const float q[4] = { q1, nextafterf(q1, INFINITY), q1, nextafterf(q1, INFINITY) }; points(q, scale, "WW = 0, one ulp wide"); }
            { const float q[4] = { q1, q1, -q1, -q1 }; points(q, scale, "w = 0, mirror images about 0"); }
            { const float q[4] = { q1, (float)(q1 + 1e-6 * scale), (float)(q1 + 0.3 * scale), (float)(q1 + 0.9 * scale) }; points(q, scale, "wa << wb"); }
            { const float q[4] = { q1, (float)(q1 - 0.7 * scale), (float)(q1 + 2e-7 * scale), (float)(q1 + 3e-7 * scale) }; points(q, scale, "wa >> wb"); }
            for (int s = 0; s >= -8; s -= 2) {
                const double d = scale * pow(10.0, s);
                const float q[4] = { q1, (float)(q1 + sgn() * d * uni()), (float)(q1 + sgn() * d * uni()), (float)(q1 + sgn() * d * uni()) };
                points(q, scale, "spread");
            }
        }
    }
    // offsets of 1e4 with a spacing of 1e-3 (an ulp of float32 there is 9.8e-4)
    for (int k = 0; k < 20000; ++k) {
        float q[4];
        for (float &v : q) v = (float)(1.0e4 + 1.0e-3 * (double)(rnd() % 40));
        const float h1 = (float)(1.0e4 + 1.0e-3 * 40.0 * uni()), h2 = (float)(1.0e4 + 1.0e-3 * 40.0 * uni());
        const float c = (float)(1.0e-3 * (double)(rnd() % 8));
        check(q, 4, h1, h2, c, "offset 1e4");
        check(q, 4, h1, h1, c, "offset 1e4");
        check(q, 3, h1, h2, c, "offset 1e4");
    }
    const long long n_adversarial = checked;
    // random octuples: four vertices at a random scale and spread, a cap around the pairs' distance or far from it, a pair of points
    // narrower or wider than the cap, near or far
    for (long long i = 0; i < n_random; ++i) {
        const double scale = pow(10.0, -30.0 + 48.0 * uni());
        const double dq = scale * pow(10.0, -8.0 * uni()) * uni();
        float q[4];
        q[0] = (float)(sgn() * scale * uni());
        for (int k = 1; k < 4; ++k) q[k] = (rnd() & 7) == 0 ? q[k - 1] : (float)(q[0] + sgn() * dq * ((rnd() & 3) == 0 ? pow(10.0, -6.0 * uni()) : 1.0) * uni());
        const unsigned pc = (unsigned)(rnd() & 7);
        const float c = pc == 0 ? 0.0f : (pc == 1 ? (float)(scale * 10.0 * uni()) : (float)(dq * pow(10.0, 1.0 - 3.0 * uni())));
        const unsigned pick = (unsigned)(rnd() & 7);
        float h1, h2;
        if (pick < 4) h1 = q[pick];
        else if (pick == 4) h1 = (float)(sgn() * scale * 10.0 * uni());
        else h1 = (float)(q[0] + sgn() * (dq + c) * 4.0 * uni());        // within a few spreads of the quad
        const unsigned pick2 = (unsigned)(rnd() & 3);
        if (pick2 == 0) h2 = (float)(h1 + sgn() * (double)c * pow(10.0, 1.0 - 3.0 * uni()));          // Hw around c, either side of it
        else if (pick2 == 1) h2 = (float)(h1 + sgn() * scale * pow(10.0, -8.0 * uni()) * uni());
        else if (pick2 == 2) h2 = (rnd() & 1) ? h1 : (float)(sgn() * scale * 10.0 * uni());
        else h2 = (float)(0.5 * ((double)q[0] + (double)q[1] + (double)q[2] + (double)q[3]) - (double)h1);   // mirror image about MM: X = 0
        const unsigned nr = (unsigned)(rnd() & 15);
        check(q, nr < 4 ? (int)nr : 4, h1, h2, c, "random");
        if ((i & 7) == 0) {
            // thresholds: base = FILTER_ABS (1e-30) at the least, up to the square of a few scales
            double qmax = 0.0;
            for (float v : q) qmax = fmax(qmax, fabs((double)v));
            qmax *= 1.0 + 3.0 * uni();
            const double ba = 1e-30 + pow(scale * pow(10.0, 1.0 - 9.0 * uni()), 2.0), bb = (rnd() & 1) ? ba : 1e-30 + pow(scale * pow(10.0, 1.0 - 9.0 * uni()), 2.0);
            check_threshold(ba, bb, qmax, h1, h2, c);
        }
    }
    printf("oct_gap_bound: %lld adversarial + %lld random octuples, %lld thresholds, 0 violations\n", n_adversarial, checked - n_adversarial,
           thresholds);
    return 0;
}
