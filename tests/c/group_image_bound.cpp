// Level 0's images of V = 8 and V = 16 sorted positions (group_image<V>, object_alignment_amd/csrc/oa_octgap.hpp), checked on the host
// against long double:
//   (P)  0 <= ww <= c, ws >= 0, and every real q_j of the group lies within ws of mm + ww or of mm - ww -- for the float32 mm, ww, ws
//        as stored, the distances in long double (exact for floats within 2^40 of each other; beyond that an ulp of long double is
//        far below an ulp of what group_image adds to ws);
//   (B)  oct_gap(group_image, point_pair_image_capped) <= (T + oct_allowance(qmax, h1, h2, c) + e)(1 + 2^-23), T the smallest of the 2V
//        real gaps |q_j - h|, qmax the largest |q| of the group -- the smallest qmax a target that holds the group can have;
//   and the padding rules: a group whose second half is padding has the image of its first half, padding alone is {1e18, 0, 0}.
// Built with -ffp-contract=off: the four subtractions round separately, as the kernel's do.
// usage: group_image_bound [random groups per V]     exit status 1 on the first violation
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
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

static long long checked = 0;

template <int V> static void fail(const char *what, const char *which, const float *q, int n_real, float h1, float h2, float c, float mm, float ww, float ws)
{
    printf("VIOLATION V=%d (%s; %s): %d real, h1 %.9g h2 %.9g c %.9g -> mm %.9g ww %.9g ws %.9g; q", V, what, which, n_real, (double)h1, (double)h2,
           (double)c, (double)mm, (double)ww, (double)ws);
    for (int k = 0; k < V; ++k) printf(" %.9g", (double)q[k]);
    printf("\n");
    exit(1);
}

// one group of V positions, the first n_real of them vertices (padding only ever follows the vertices), one pair of points, a cap
template <int V> static void check(const float *q, int n_real, float h1, float h2, float c, const char *what)
{
    float mm, ww, ws, hm, hwc;
    double e;
    oa::group_image<V>(q, n_real, c, mm, ww, ws);
    ++checked;
    if (n_real == 0) {
        if (!(mm == oa::PAIR_PAD_U && ww == 0.0f && ws == 0.0f)) fail<V>(what, "padding alone is {1e18, 0, 0}", q, n_real, h1, h2, c, mm, ww, ws);
        return;
    }
    // (P) on the stored floats
    if (!(ww >= 0.0f) || !(ww <= c) || !(ws >= 0.0f)) fail<V>(what, "0 <= ww <= c, ws >= 0", q, n_real, h1, h2, c, mm, ww, ws);
    const long double sp = (long double)mm + (long double)ww, sm = (long double)mm - (long double)ww;
    double qmax = 0.0;
    for (int k = 0; k < n_real; ++k) {
        const long double dp = fabsl((long double)q[k] - sp), dm = fabsl((long double)q[k] - sm);
        if (!((dp < dm ? dp : dm) <= (long double)ws)) fail<V>(what, "(P): a vertex further than ws from mm +- ww", q, n_real, h1, h2, c, mm, ww, ws);
        qmax = fmax(qmax, fabs((double)q[k]));
    }
    // (B) the kernel's chain against the smallest real gap
    oa::point_pair_image_capped(h1, h2, c, hm, hwc, e);
    const float t = oa::oct_gap(mm, ww, ws, hm, hwc);
    const float hs[2] = { h1, h2 };
    long double T = INFINITY;
    for (int k = 0; k < n_real; ++k)
        for (float h : hs) {
            const long double g = fabsl((long double)q[k] - (long double)h);
            if (g < T) T = g;
        }
    const long double bound = (T + (long double)oa::oct_allowance(qmax, h1, h2, c) + (long double)e) * (1.0L + 0x1p-23L);
    if (!((long double)t <= bound) || !(ww <= hwc) || !(e >= 0.0)) {
        printf("t %.9g > bound %.12Lg (T %.12Lg, e %.9g, hm %.9g hw' %.9g)\n", (double)t, bound, T, e, (double)hm, (double)hwc);
        fail<V>(what, "(B): oct_gap overstates the smallest gap", q, n_real, h1, h2, c, mm, ww, ws);
    }
    // the padding rules: a second half of padding alone leaves the first half's image; one vertex is itself; duplicates are a point
    if (n_real <= V / 2) {
        float m2, w2, s2;
        oa::group_image<V / 2>(q, n_real, c, m2, w2, s2);
        if (!(m2 == mm && w2 == ww && s2 == ws)) fail<V>(what, "second half padding: the first half's image", q, n_real, h1, h2, c, mm, ww, ws);
    }
    if (n_real == 1 && !(mm == q[0] && ww == 0.0f && ws == 0.0f)) fail<V>(what, "one vertex is itself", q, n_real, h1, h2, c, mm, ww, ws);
    bool same = true;
    for (int k = 1; k < n_real; ++k) same = same && q[k] == q[0];
    if (same && !(mm == q[0] && ww == 0.0f && ws == 0.0f)) fail<V>(what, "duplicates: ww = ws = 0", q, n_real, h1, h2, c, mm, ww, ws);
}

// every pair of points, every cap and every padding count worth trying against one group of V vertices
template <int V> static void points(const float *q, double scale, const char *what)
{
    double lo_a = q[0], hi_a = q[0], lo_b = q[V / 2], hi_b = q[V / 2];
    for (int k = 0; k < V / 2; ++k) { lo_a = fmin(lo_a, q[k]); hi_a = fmax(hi_a, q[k]); lo_b = fmin(lo_b, q[V / 2 + k]); hi_b = fmax(hi_b, q[V / 2 + k]); }
    const double Ca = (lo_a + hi_a) / 2.0, Cb = (lo_b + hi_b) / 2.0, MM = (Ca + Cb) / 2.0, WW = fabs(Cb - Ca) / 2.0;
    const float far = (float)(q[0] + 1e3 * scale);
    const float wwf = (float)WW, below = nextafterf(wwf, -INFINITY) < 0.f ? 0.f : nextafterf(wwf, -INFINITY);
    // the caps: 0, tiny, WW itself (halves exactly 2 c apart) and an ulp to either side, half and twice it (halves further apart than 2 c,
    // nearer), a half's own width, the scale, huge
    const float caps[] = { 0.0f, (float)(1e-6 * scale), wwf, nextafterf(wwf, INFINITY), below, (float)(0.5 * WW), (float)(2.0 * WW), (float)((hi_a - lo_a) / 2.0),
                           (float)scale, (float)(1e6 * scale), 1.0e30f };
    for (const float c : caps) {
        float m4, w4, s4;
        oa::group_image<V>(q, V, c, m4, w4, s4);
        const double A = (double)c;                                             // hw' of the lanes with Hw <= c
        // (h1, h2): Hw = 0, Hw = c, Hw < c, Hw > c; X = 0; |X| = hw' and ||X| - hw'| = ww and an ulp to either side of each; a point on a vertex
        // with everything else far away
        const float hs[][2] = {
            { q[0], q[0] }, { q[V - 1], q[V - 1] }, { (float)MM, (float)MM }, { 0.0f, 0.0f },                                       // Hw = 0
            { (float)(MM - A), (float)(MM + A) }, { (float)(q[0] - A), (float)(q[0] + A) },                                         // Hw = c
            { (float)(MM - 0.5 * A), (float)(MM + 0.5 * A) }, { q[1], (float)(q[1] + 0.25 * A) },                                   // Hw < c
            { (float)(MM - 3.0 * A - scale), (float)(MM + 3.0 * A + scale) }, { q[0], q[V - 1] }, { q[1], q[V / 2] }, { q[V - 1], q[0] },   // Hw > c mostly
            { (float)(MM + A), (float)(MM + A) }, { nextafterf((float)(MM + A), INFINITY), (float)(MM + A) },                         // |X| = hw' (Hw = 0)
            { nextafterf((float)(MM + A), -INFINITY), nextafterf((float)(MM + A), -INFINITY) },
            { (float)(MM - A), (float)(MM - A) }, { (float)(MM + 2.0 * A), (float)MM }, { (float)(MM - 2.0 * A), (float)MM },
            { (float)(MM + A + w4), (float)(MM + A + w4) }, { (float)(MM + A - w4), (float)(MM + A - w4) },                           // ||X| - hw'| = ww
            { nextafterf((float)(MM + A + w4), INFINITY), (float)(MM + A + w4) }, { nextafterf((float)(MM + A - w4), -INFINITY), (float)(MM + A - w4) },
            { (float)(MM - A - w4), (float)(MM - A - w4) }, { (float)(MM - A + w4), nextafterf((float)(MM - A + w4), INFINITY) },
            { q[0], far }, { far, q[1] }, { q[V / 2], -far }, { q[V - 1], far }, { -far, q[V - 1] },                                // best = 0 for one, the partner far
            { (float)(MM + 1e4 * scale), (float)MM }, { (float)(-1e-4 * scale), (float)(1e4 * scale) },
            { nextafterf(q[0], -INFINITY), nextafterf(q[V - 1], INFINITY) }, { -q[0], q[V - 1] },
        };
        for (const auto &h : hs) {
            check<V>(q, V, h[0], h[1], c, what);
            float r[V], s[V];
            for (int k = 0; k < V; ++k) { r[k] = q[V - 1 - k]; s[k] = q[(k * 5 + 3) % V]; }       // (any order of the V: 5 is coprime to 8 and 16)
            check<V>(r, V, h[1], h[0], c, what);
            check<V>(s, V, h[0], h[1], c, what);
            for (int n = 0; n < V; ++n) check<V>(q, n, h[0], h[1], c, n == 1 ? "1 vertex + V - 1 padding" : (n == V / 2 ? "V / 2 + V / 2 padding" : "padding"));
            // every vertex of the group as a point of its own, on it and an ulp beside it
            for (int k = 0; k < V; ++k) { check<V>(q, V, q[k], h[1], c, what); check<V>(q, V, h[0], nextafterf(q[k], INFINITY), c, what); }
        }
    }
}

template <int V> static void run(long long n_random)
{
    const long long before = checked;
    // adversarial: scales 1e-30 .. 1e18
    for (int e = -30; e <= 18; ++e) {
        const double scale = pow(10.0, e);
        for (int rep = 0; rep < 1; ++rep) {
            const float q1 = (float)(sgn() * scale * (0.1 + 0.9 * uni()));
            float q[V];
            for (int k = 0; k < V; ++k) q[k] = q1;
            points<V>(q, scale, "duplicates: ww = ws = 0");
            for (int k = 0; k < V; ++k) q[k] = (k & 1) ? nextafterf(q1, INFINITY) : q1;
            points<V>(q, scale, "halves on top of each other (0 apart), one ulp wide");
            for (int k = 0; k < V; ++k) q[k] = k < V / 2 ? q1 : -q1;
            points<V>(q, scale, "two lattices, mirror images about 0");
            for (int s = 0; s >= -8; s -= 4) {
                const double d = scale * pow(10.0, s);
                for (const int out : { 0, V / 2 - 1, V / 2, V - 1 }) {      // the outlier first, at either side of the middle, last
                    for (int k = 0; k < V; ++k) q[k] = (float)(q1 + 1e-6 * d * uni());
                    q[out] = (float)(q1 + sgn() * d);
                    points<V>(q, scale, "one outlier in a tight group");
                }
                for (int k = 0; k < V; ++k) q[k] = (float)(q1 + (k < V / 2 ? 0.0 : d) + 1e-3 * d * uni());
                points<V>(q, scale, "two tight halves far apart");
                for (int k = 0; k < V; ++k) q[k] = (float)(q1 + (k < V / 2 ? 1e-6 : 1.0) * d * uni());
                points<V>(q, scale, "a narrow half and a wide one");
                for (int k = 0; k < V; ++k) q[k] = (float)(q1 + sgn() * d * uni());
                points<V>(q, scale, "spread");
            }
        }
    }
    // offsets of 1e4 with a spacing of 1e-3 (an ulp of float32 there is 9.8e-4)
    for (int k = 0; k < 20000; ++k) {
        float q[V];
        for (float &v : q) v = (float)(1.0e4 + 1.0e-3 * (double)(rnd() % 40));
        const float h1 = (float)(1.0e4 + 1.0e-3 * 40.0 * uni()), h2 = (float)(1.0e4 + 1.0e-3 * 40.0 * uni());
        const float c = (float)(1.0e-3 * (double)(rnd() % 8));
        check<V>(q, V, h1, h2, c, "offset 1e4");
        check<V>(q, V, h1, h1, c, "offset 1e4");
        check<V>(q, (int)(rnd() % (V + 1)), h1, h2, c, "offset 1e4 + padding");
    }
    const long long n_adversarial = checked - before;
    // random groups: V vertices at a random scale and spread (sorted like the upload's, or not: the u order is quantised and a block
    // is in the order of v), a cap around the spread or far from it, a pair of points narrower or wider than the cap, near or far
    for (long long i = 0; i < n_random; ++i) {
        const double scale = pow(10.0, -30.0 + 48.0 * uni());
        const double dq = scale * pow(10.0, -8.0 * uni()) * uni();
        float q[V];
        q[0] = (float)(sgn() * scale * uni());
        const bool walk = rnd() & 1;
        for (int k = 1; k < V; ++k) {
            const double step = dq * ((rnd() & 3) == 0 ? pow(10.0, -6.0 * uni()) : 1.0) * uni();
            q[k] = (rnd() & 7) == 0 ? q[k - 1] : (walk ? (float)(q[k - 1] + step / V) : (float)(q[0] + sgn() * step));
        }
        const unsigned pc = (unsigned)(rnd() & 7);
        const float c = pc == 0 ? 0.0f : (pc == 1 ? (float)(scale * 10.0 * uni()) : (float)(dq * pow(10.0, 1.0 - 3.0 * uni())));
        const unsigned pick = (unsigned)(rnd() & 7);
        float h1, h2;
        if (pick < 4) h1 = q[rnd() % V];
        else if (pick == 4) h1 = (float)(sgn() * scale * 10.0 * uni());
        else h1 = (float)(q[0] + sgn() * (dq + c) * 4.0 * uni());        // within a few spreads of the group
        const unsigned pick2 = (unsigned)(rnd() & 3);
        if (pick2 == 0) h2 = (float)(h1 + sgn() * (double)c * pow(10.0, 1.0 - 3.0 * uni()));          // Hw around c, either side of it
        else if (pick2 == 1) h2 = (float)(h1 + sgn() * scale * pow(10.0, -8.0 * uni()) * uni());
        else if (pick2 == 2) h2 = (rnd() & 1) ? h1 : (float)(sgn() * scale * 10.0 * uni());
        else h2 = (float)((double)q[0] + (double)q[V - 1] - (double)h1);                              // mirror image about the group: X near 0
        const unsigned nr = (unsigned)(rnd() % (4 * V));
        check<V>(q, nr <= (unsigned)V ? (int)nr : V, h1, h2, c, "random");
    }
    printf("group_image_bound V=%d: %lld adversarial + %lld random groups, 0 violations\n", V, n_adversarial, checked - before - n_adversarial);
}

int main(int argc, char **argv)
{
    const long long n_random = argc > 1 ? atoll(argv[1]) : 10000000;
    run<8>(n_random);
    run<16>(n_random);
    return 0;
}
