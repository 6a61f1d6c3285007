// region_check.hip -- closest_on_tri_region (oa_deviation.hpp) against closest_on_tri (oa_kernels.hpp) on the HOST: the same r,
// bit for bit, on random triangle/point pairs and on constructed ones (the point at a vertex, on an edge, in the plane;
// degenerate triangles).  Prints the mismatches and how often every region occurred.
// build: __graft_entry__.build_tools()     run: tools/region_check.exe [pairs] [seed]
// With `--pairs FILE`: reads float32 rows of 12 (p, a, b, c) from FILE and prints one region code per row (the tests' reference
// for the device's `feature` output).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <random>
#include <vector>
#include "oa_kernels.hpp"
#include "oa_deviation.hpp"

static long long g_mismatch = 0, g_count[7] = { 0, 0, 0, 0, 0, 0, 0 }, g_total = 0;

static void check(const float *p, const float *a, const float *b, const float *c)
{
    float r0[3], r1[3];
    oa::closest_on_tri(p, a, b, c, r0);
    const int region = oa::closest_on_tri_region(p, a, b, c, r1);
    ++g_total;
    if (region < 0 || region > 6) { ++g_mismatch; return; }
    ++g_count[region];
    if (memcmp(r0, r1, sizeof r0) != 0) {
        if (g_mismatch < 10)
            fprintf(stderr, "mismatch: region %d  r = %a %a %a  vs  %a %a %a\n", region, r0[0], r0[1], r0[2], r1[0], r1[1], r1[2]);
        ++g_mismatch;
    }
}

int main(int argc, char **argv)
{
    if (argc >= 3 && strcmp(argv[1], "--pairs") == 0) {
        FILE *f = fopen(argv[2], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
        float row[12], r[3];
        while (fread(row, sizeof(float), 12, f) == 12) printf("%d\n", oa::closest_on_tri_region(row, row + 3, row + 6, row + 9, r));
        fclose(f);
        return 0;
    }
    const long long n = argc > 1 ? atoll(argv[1]) : 1000000;
    std::mt19937_64 rng(argc > 2 ? (uint64_t)atoll(argv[2]) : 20260929ull);
    std::uniform_real_distribution<float> uni(-1.f, 1.f);
    std::normal_distribution<float> nrm(0.f, 1.f);
    auto rnd3 = [&](float *v, float s) { for (int k = 0; k < 3; ++k) v[k] = s * uni(rng); };
    for (long long i = 0; i < n; ++i) {
        float a[3], b[3], c[3], p[3];
        const float ts = (i & 3) == 0 ? 0.05f : 1.f, ps = (i & 4) ? 3.f : 1.f;      // small triangles far away; points well outside
        rnd3(a, 1.f);
        rnd3(b, ts); rnd3(c, ts);
        for (int k = 0; k < 3; ++k) { b[k] += a[k]; c[k] += a[k]; }
        rnd3(p, ps);
        check(p, a, b, c);
        // the constructed ones, from the same triangle
        const float *v[3] = { a, b, c };
        const int k0 = (int)(i % 3), k1 = (k0 + 1) % 3;
        float q[3];
        check(v[k0], a, b, c);                                                       // the point AT a vertex
        const float t = 0.5f * (uni(rng) + 1.f);
        for (int k = 0; k < 3; ++k) q[k] = v[k0][k] + t * (v[k1][k] - v[k0][k]);     // ON an edge (up to rounding)
        check(q, a, b, c);
        const float u = 0.5f * (uni(rng) + 1.f), w = (1.f - u) * 0.5f * (uni(rng) + 1.f);
        for (int k = 0; k < 3; ++k) q[k] = a[k] + u * (b[k] - a[k]) + w * (c[k] - a[k]);   // IN the plane, inside
        check(q, a, b, c);
        for (int k = 0; k < 3; ++k) q[k] = a[k] + 2.f * uni(rng) * (b[k] - a[k]) + 2.f * uni(rng) * (c[k] - a[k]);   // in the plane, anywhere
        check(q, a, b, c);
        if ((i & 15) == 0) {                                                         // degenerate triangles
            check(p, a, a, a);                                                       // a point
            check(p, a, b, b);                                                       // a segment, twice a corner
            check(p, a, a, c);
            for (int k = 0; k < 3; ++k) q[k] = a[k] + 0.5f * (b[k] - a[k]);
            check(p, a, b, q);                                                       // collinear corners
            check(p, a, q, b);
        }
    }
    printf("pairs %lld mismatches %lld regions", g_total, g_mismatch);
    for (int k = 0; k < 7; ++k) printf(" %lld", g_count[k]);
    printf("\n");
    return g_mismatch ? 1 : 0;
}
