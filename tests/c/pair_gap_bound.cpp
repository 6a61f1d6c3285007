// The rounding bound of level 0's pair gap (object_alignment_amd/csrc/oa_pairgap.hpp), checked on the host against long double:
//     pair_gap(m, w, h) <= (g + pair_allowance(qmax, h)) (1 + 2^-23),      g = min(|q1 - h|, |q2 - h|),
// {m, w} = pair_image(q1, q2), qmax = max(|q1|, |q2|) -- the smallest qmax a target that holds the pair can have.  The kernel's
// threshold relies on it with 2^-24 in place of 2^-23 and then adds 2^-22 of its own (sorted_thresholds), so 2^-23 here still
// proves it.  Built with -ffp-contract=off: the two subtractions round separately, as the kernel's do.
// usage: pair_gap_bound [random triples]     exit status 1 on the first violation
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "oa_pairgap.hpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    uint64_t x = rng_state;
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    return rng_state = x;
}
static double uni() { return (double)(rnd() >> 11) * 0x1p-53; }               // [0, 1)
static double sgn() { return (rnd() & 1) ? 1.0 : -1.0; }

static long long checked = 0;

// one pair of positions (real1 / real2: a vertex, else padding) and one point
static void check(float q1, bool real1, float q2, bool real2, float h, const char *what)
{
    float m, w;
    oa::pair_image(q1, real1, q2, real2, m, w);
    const float a = oa::pair_gap(m, w, h);
    // what level 0 must not overstate: the smaller real gap of the positions the image stands for
    const float p1 = real1 ? q1 : (real2 ? q2 : oa::PAIR_PAD_U), p2 = real2 ? q2 : p1;
    const long double g1 = fabsl((long double)p1 - (long double)h), g2 = fabsl((long double)p2 - (long double)h);
    const long double g = g1 < g2 ? g1 : g2;
    const double qmax = fmax(fabs((double)p1), fabs((double)p2));
    const long double bound = (g + (long double)oa::pair_allowance(qmax, h)) * (1.0L + 0x1p-23L);
    ++checked;
    if (!((long double)a <= bound)) {
        printf("VIOLATION (%s): q1 %.9g%s q2 %.9g%s h %.9g -> m %.9g w %.9g a %.9g > bound %.12Lg (g %.12Lg)\n", what, (double)q1,
               real1 ? "" : " (pad)", (double)q2, real2 ? "" : " (pad)", (double)h, (double)m, (double)w, (double)a, bound, g);
        exit(1);
    }
}

// every point worth trying against one pair
static void points(float q1, float q2, double scale, const char *what)
{
    float m, w;
    oa::pair_image(q1, true, q2, true, m, w);
    const float hs[] = { q1, q2, m, nextafterf(m, INFINITY), nextafterf(m, -INFINITY), nextafterf(q1, -INFINITY), nextafterf(q2, INFINITY),
                         0.0f, -q1, (float)(q1 + scale), (float)(q1 - 3.0 * scale), (float)(1e4 * scale), (float)(-1e-4 * scale) };
    for (float h : hs) {
        check(q1, true, q2, true, h, what);
        check(q2, true, q1, true, h, what);
        check(q1, true, oa::PAIR_PAD_U, false, h, "vertex + padding");
        check(oa::PAIR_PAD_U, false, oa::PAIR_PAD_U, false, h, "padding + padding");
    }
}

int main(int argc, char **argv)
{
    const long long n_random = argc > 1 ? atoll(argv[1]) : 10000000;
    // adversarial: scales 1e-30 .. 1e18, spreads from the whole scale down to one ulp and to zero
    for (int e = -30; e <= 18; ++e) {
        const double scale = pow(10.0, e);
        for (int k = 0; k < 200; ++k) {
            const float q1 = (float)(sgn() * scale * (0.1 + 0.9 * uni()));
            points(q1, q1, scale, "q1 == q2");
            points(q1, nextafterf(q1, INFINITY), scale, "one ulp apart");
            points(q1, nextafterf(nextafterf(q1, INFINITY), INFINITY), scale, "two ulps apart");
            points(q1, -q1, scale, "mirror images about 0");
            for (int s = 0; s >= -8; --s) points(q1, (float)(q1 + sgn() * scale * pow(10.0, s) * uni()), scale, "spread");
        }
    }
    const long long n_adversarial = checked;
    // random triples: a pair at a random scale and spread, a point near it, on it or far from it
    for (long long i = 0; i < n_random; ++i) {
        const double scale = pow(10.0, -30.0 + 48.0 * uni());
        const float q1 = (float)(sgn() * scale * uni());
        const float q2 = (float)(q1 + sgn() * scale * pow(10.0, -8.0 * uni()) * uni());
        const unsigned pick = (unsigned)(rnd() & 7);
        float h;
        if (pick == 0) h = q1;
        else if (pick == 1) { float m, w; oa::pair_image(q1, true, q2, true, m, w); h = m; }
        else if (pick == 2) h = (float)(sgn() * scale * 10.0 * uni());
        else h = (float)(q1 + sgn() * fabs((double)q2 - (double)q1) * 4.0 * uni());   // within a few spreads of the pair
        check(q1, true, q2, true, h, "random");
    }
    printf("pair_gap_bound: %lld adversarial + %lld random triples, 0 violations\n", n_adversarial, checked - n_adversarial);
    return 0;
}
