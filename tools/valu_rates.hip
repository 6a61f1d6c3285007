// Issue rates of the vector-ALU instructions the search kernels choose between, measured on the GPU box (not part of the library).
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Wno-unused-value -I object_alignment_amd/csrc -o tools/_exp/valu_rates tools/valu_rates.hip
//   gpurun -- 'tools/_exp/valu_rates'                                                                   (results: profiles/r05q_valu_rates.txt)
// Each kernel runs 16 independent dependency chains of ONE instruction per lane, 8 waves per SIMD on every SIMD; the figure is
// nanoseconds per wave-instruction per SIMD (1.0 ns ~ one instruction every two cycles at ~2 GHz = the full rate).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include "oa_level0.hpp"
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
template <int OP> __global__ __launch_bounds__(256) void burn(float *out, int trips, float seed)
{
    float a[16]; h2 p[16];
    for (int k = 0; k < 16; ++k) { a[k] = seed + k + threadIdx.x; p[k] = h2{(_Float16)(seed + k), (_Float16)(seed - k)}; }
    float b = seed * 0.5f, c = seed * 0.25f; h2 pb = h2{(_Float16)b, (_Float16)c}, pc = h2{(_Float16)c, (_Float16)b};
    for (int t = 0; t < trips; ++t) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (OP == 0) asm volatile("v_add_f32 %0, %0, %1" : "+v"(a[k]) : "v"(b));
                if (OP == 1) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[k]) : "v"(b), "v"(c));
                if (OP == 2) asm volatile("v_pk_fma_f16 %0, %0, %1, %2" : "+v"(p[k]) : "v"(pb), "v"(pc));
                if (OP == 3) asm volatile("v_pk_min_f16 %0, %0, %1" : "+v"(p[k]) : "v"(pb));
                if (OP == 4) asm volatile("v_pk_add_f16 %0, %0, %1" : "+v"(p[k]) : "v"(pb));
                if (OP == 5) asm volatile("v_min3_f32 %0, %0, %1, %2" : "+v"(a[k]) : "v"(b), "v"(c));
                if (OP == 6) asm volatile("v_min_f32 %0, %0, %1" : "+v"(a[k]) : "v"(b));
                if (OP == 7) asm volatile("v_pk_fma_f16 %0, %1, %2, %0" : "+v"(p[k]) : "v"(pb), "v"(pc));
                if (OP == 8) asm volatile("v_pk_fma_f16 %0, %0, %1, %2 op_sel_hi:[1,0,1]" : "+v"(p[k]) : "v"(pb), "v"(pc));
                if (OP == 9) asm volatile("v_pk_min_i16 %0, %0, %1" : "+v"(p[k]) : "v"(pb));
                if (OP == 10) asm volatile("v_pk_max_f16 %0, %0, %0 neg_lo:[0,1] neg_hi:[0,1]" : "+v"(p[k]));
                if (OP == 11) asm volatile("v_and_b32 %0, %0, %1" : "+v"(a[k]) : "v"(b));
                if (OP == 12) asm volatile("v_pk_mul_f16 %0, %0, %1" : "+v"(p[k]) : "v"(pb));
                if (OP == 13) asm volatile("v_cmp_gt_f32 vcc, %0, %1" :: "v"(a[k]), "v"(b) : "vcc");
                if (OP == 14) asm volatile("v_pk_min_u16 %0, %0, %1" : "+v"(p[k]) : "v"(pb));
                if (OP == 15) asm volatile("v_min_u32 %0, %0, %1" : "+v"(a[k]) : "v"(b));
                if (OP == 16) asm volatile("v_min_f16 %0, %0, %1" : "+v"(a[k]) : "v"(b));
                if (OP == 17) asm volatile("v_sub_f32 %0, %1, %0" : "+v"(a[k]) : "v"(b));
                if (OP == 18) asm volatile("v_dot2_f32_f16 %0, %1, %2, %0" : "+v"(a[k]) : "v"(pb), "v"(pc));
                if (OP == 20) asm volatile("v_min3_f16 %0, %0, %1, %2" : "+v"(a[k]) : "v"(b), "v"(c));
                if (OP == 21) asm volatile("v_sub_f16 %0, %1, %0" : "+v"(a[k]) : "v"(b));
                if (OP == 22) asm volatile("v_pk_minimum3_f16 %0, %0, %1, %2" : "+v"(p[k]) : "v"(pb), "v"(pc));
                if (OP == 23) asm volatile("v_minimum3_f32 %0, %0, %1, %2" : "+v"(a[k]) : "v"(b), "v"(c));
                if (OP == 24) asm volatile("v_min3_u16 %0, %0, %1, %2" : "+v"(a[k]) : "v"(b), "v"(c));
                if (OP == 25) asm volatile("v_min3_u32 %0, %0, %1, %2" : "+v"(a[k]) : "v"(b), "v"(c));
                if (OP == 26) asm volatile("v_or3_b32 %0, %0, %1, %2" : "+v"(a[k]) : "v"(b), "v"(c));
                if (OP == 27) asm volatile("v_sad_u16 %0, %1, %2, %0" : "+v"(a[k]) : "v"(b), "v"(c));
                if (OP == 28) asm volatile("v_cvt_pkrtz_f16_f32 %0, %0, %1" : "+v"(a[k]) : "v"(b));
                if (OP == 29) asm volatile("v_min3_f16 %0, |%0|, |%1|, |%2| op_sel:[1,1,0,0]" : "+v"(a[k]) : "v"(b), "v"(c));
                if (OP == 30) asm volatile("v_med3_f32 %0, %0, %1, %2" : "+v"(a[k]) : "v"(b), "v"(c));
                if (OP == 31) asm volatile("v_sub_u16 %0, %1, %0" : "+v"(a[k]) : "v"(b));
                if (OP == 32) asm volatile("v_sub_u32 %0, %1, %0" : "+v"(a[k]) : "v"(b));
                if (OP == 33) asm volatile("v_pk_sub_u16 %0, %1, %0" : "+v"(a[k]) : "v"(b));
                if (OP == 34) asm volatile("v_min_u16 %0, %1, %0" : "+v"(a[k]) : "v"(b));
                if (OP == 35) asm volatile("v_max_f16 %0, %1, %0" : "+v"(a[k]) : "v"(b));
                if (OP == 40) asm volatile("v_sub_f32_e64 %0, |%0|, %1" : "+v"(a[k]) : "v"(b));          // round 11: the pair gap's second subtract
                if (OP == 41) asm volatile("v_sub_f32 %0, %0, %1\n\tv_sub_f32_e64 %0, |%0|, %2" : "+v"(a[k]) : "v"(b), "v"(c));   // (two instructions)
                if (OP == 42) asm volatile("v_fma_f32 %0, |%0|, 1.0, -%1" : "+v"(a[k]) : "v"(b));         // the same value through the fma pipe
                if (OP == 43) asm volatile("v_sub_f32 %0, %0, %1\n\tv_sub_f32_e64 %0, |%0|, %2\n\tv_sub_f32_e64 %0, |%0|, %1"    // round 13: the quad gap's chain
                                           : "+v"(a[k]) : "v"(b), "v"(c));                                   // (three instructions)
                if (OP == 44) asm volatile("v_sub_f32 %0, %0, %1\n\tv_sub_f32_e64 %0, |%0|, %2\n\tv_sub_f32_e64 %0, |%0|, %1\n\tv_sub_f32_e64 %0, |%0|, %2"
                                           : "+v"(a[k]) : "v"(b), "v"(c));                                   // round 18: the oct gap's chain (four)
                if (OP == 19) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(*(double*)&a[k & ~1]) : "v"(*(double*)&b));
            }
    }
    float s = 0; for (int k = 0; k < 16; ++k) s += a[k] + (float)p[k].x + (float)p[k].y;
    if (s == 12345.678f) out[0] = s;
}
// Level 0 of k_nn_search_sorted as an instruction MIX, 16 independent min chains per lane over 32 "tile" registers:
//   MIX 0 (until round 10)  per 2 vertices  sub, sub, min3(acc, |t0|, |t1|)                          2 full-rate : 1 half-rate
//   MIX 1 (round 11)        per 4 vertices  sub, sub |.|, sub, sub |.|, min3(acc, |t0|, |t1|)        4 : 1
//   MIX 2                   MIX 1 with v_fma_f32 d, |a|, 1.0, -w for the second subtract
//   MIX 3 (round 13)        per 8 (vertex, point) pairs: two chains sub, sub |.|, sub |.| and min3(acc, t0, t1), no modifier
//                           on the min's sources (oa_quadgap.hpp)                                      6 : 1
template <int MIX> __global__ __launch_bounds__(256) void mix(float *out, int trips, float seed)
{
    float a[16], q[32];
    for (int k = 0; k < 16; ++k) a[k] = seed + k + threadIdx.x;
    for (int k = 0; k < 32; ++k) q[k] = seed * 0.5f + k;
    const float h = seed * 0.25f, hw = seed * 0.125f;
    for (int t = 0; t < trips; ++t) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                float t0, t1;
                if (MIX == 0)
                    asm volatile("v_sub_f32 %1, %3, %5\n\tv_sub_f32 %2, %4, %5\n\tv_min3_f32 %0, %0, |%1|, |%2|"
                                 : "+v"(a[k]), "=&v"(t0), "=&v"(t1) : "v"(q[2 * k]), "v"(q[2 * k + 1]), "v"(h));
                if (MIX == 1)
                    asm volatile("v_sub_f32 %1, %3, %5\n\tv_sub_f32 %2, %4, %5\n\tv_sub_f32_e64 %1, |%1|, %4\n\tv_sub_f32_e64 %2, |%2|, %3\n\t"
                                 "v_min3_f32 %0, %0, |%1|, |%2|"
                                 : "+v"(a[k]), "=&v"(t0), "=&v"(t1) : "v"(q[2 * k]), "v"(q[2 * k + 1]), "v"(h));
                if (MIX == 2)
                    asm volatile("v_sub_f32 %1, %3, %5\n\tv_sub_f32 %2, %4, %5\n\tv_fma_f32 %1, |%1|, 1.0, -%4\n\tv_fma_f32 %2, |%2|, 1.0, -%3\n\t"
                                 "v_min3_f32 %0, %0, |%1|, |%2|"
                                 : "+v"(a[k]), "=&v"(t0), "=&v"(t1) : "v"(q[2 * k]), "v"(q[2 * k + 1]), "v"(h));
                if (MIX == 3)
                    asm volatile("v_sub_f32 %1, %3, %5\n\tv_sub_f32 %2, %4, %5\n\tv_sub_f32_e64 %1, |%1|, %6\n\tv_sub_f32_e64 %2, |%2|, %6\n\t"
                                 "v_sub_f32_e64 %1, |%1|, %4\n\tv_sub_f32_e64 %2, |%2|, %3\n\tv_min3_f32 %0, %0, %1, %2"
                                 : "+v"(a[k]), "=&v"(t0), "=&v"(t1) : "v"(q[2 * k]), "v"(q[2 * k + 1]), "v"(h), "v"(hw));
            }
    }
    float s = 0; for (int k = 0; k < 16; ++k) s += a[k];
    if (s == 12345.678f) out[0] = s;
}
// Round 18: level 0's fold of a block of 256 vertices for a lane of 4 points (two point pairs) as k_nn_search_sorted writes it, the
// tile registers fed by broadcast ds_read_b128 from LDS -- the compiler's own schedule of the library's own functions:
//   OCT 0 (round 13)  per 16 vertices 4 float4 of pair images, 2 x 24 subtracts + 2 x 4 min3 (oa_quadgap.hpp)       6 : 1, 16 tile registers
//   OCT 1 (round 18)  per 16 vertices 3 float4 of quad images, 2 x 16 subtracts + 2 x 2 min3 (oa_octgap.hpp)        8 : 1, 12 tile registers
//   OCT 2 (round 19)  V = 8: the same body per 32 vertices, 8 trips of the chunk loop per block                      16 : 1
//   OCT 4 (round 19)  V = 16: the same body per 64 vertices, 4 trips                                                32 : 1
// A trip is one block: 256 vertices x 4 points = 1024 (vertex, point) pairs per lane.
template <int OCT> __global__ __launch_bounds__(256, 2) void fold(float *out, int trips, float seed)
{
    __shared__ float4 tl[2][64];
    if (threadIdx.x < 128) tl[threadIdx.x >> 6][threadIdx.x & 63] = make_float4(seed * 0.5f + threadIdx.x, seed, seed * 3.0f - threadIdx.x, seed * 0.125f);
    __syncthreads();
    float qhm[2] = {seed + threadIdx.x, seed * 2.0f - threadIdx.x}, qhw[2] = {seed * 0.25f, seed * 0.375f}, qthr[2] = {seed * 1e9f, seed * 2e9f};
    int hits = 0;
    for (int t = 0; t < trips; ++t) {
        int cur = t & 1;
        asm volatile("" : "+s"(cur));                          // (the tile anew every trip, as the kernel's)
        float qm[2], qodd[2];                                  // (the library's folds, oa_level0.hpp, as the kernel calls them)
#pragma unroll
        for (int c = 0; c < (OCT >= 2 ? 16 / OCT : 16); ++c) {
            if (OCT) oa::level0_images<4>(&tl[cur][3 * c], c == 0, qhm, qhw, qm, qodd);
            else oa::level0_point_pairs<4>(&tl[cur][4 * c], c == 0, qhm, qhw, qm, qodd);
        }
        bool hit[4];                                           // (a hit marks both points of a pair)
        oa::level0_pair_hits<4>(qm, qodd, qthr, hit);
        hits += (hit[0] ? 1 : 0) + (hit[2] ? 1 : 0);
    }
    if (hits == 12345) out[0] = (float)hits;
}
template <int OCT> void run_fold(const char *name, int wps)
{
    float *d; (void)hipMalloc(&d, 4);
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    const int trips = 100000, blocks = 256 * wps;
    fold<OCT><<<blocks, 256>>>(d, 100, 1.0f);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0); fold<OCT><<<blocks, 256>>>(d, trips, 1.0f); (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
    float ms; (void)hipEventElapsedTime(&ms, e0, e1);
    const double pairs = (double)wps * trips * 1024.0;        // (vertex, point) pairs per lane, per SIMD
    printf("%-34s %8.3f ms  %d waves/SIMD  %.4f ns per (vertex, point) pair per SIMD\n", name, ms, wps, ms * 1e6 / pairs);
    (void)hipFree(d);
}
// wps waves per SIMD (the search kernel runs at 4); per_step instructions and vertices per inner step
template <int MIX> void run_mix(const char *name, int wps, int per_step, int vertices)
{
    float *d; (void)hipMalloc(&d, 4);
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    const int trips = 10000, blocks = 256 * wps;
    mix<MIX><<<blocks, 256>>>(d, 100, 1.0f);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0); mix<MIX><<<blocks, 256>>>(d, trips, 1.0f); (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
    float ms; (void)hipEventElapsedTime(&ms, e0, e1);
    const double steps = (double)blocks * 4 * trips * 64 / 1024.0;    // inner steps per SIMD
    printf("%-34s %8.3f ms  %d waves/SIMD  %.3f ns per instr per SIMD  %.3f ns per vertex per SIMD\n", name, ms, wps,
           ms * 1e6 / (steps * per_step), ms * 1e6 / (steps * vertices));
    (void)hipFree(d);
}
template <int OP> void run(const char *name, int per_step = 1)
{
    float *d; (void)hipMalloc(&d, 4);
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    const int trips = 20000, blocks = 256 * 8;     // 8 waves / SIMD
    burn<OP><<<blocks, 256>>>(d, 100, 1.0f);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0); burn<OP><<<blocks, 256>>>(d, trips, 1.0f); (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
    float ms; (void)hipEventElapsedTime(&ms, e0, e1);
    const double winst = (double)blocks * 4 * trips * 64 * per_step;            // wave-instructions
    const double per_simd = winst / 1024.0;
    printf("%-34s %8.3f ms  %7.2f G wave-instr/s/SIMD  (%.3f ns per instr per SIMD)\n", name, ms, per_simd / ms / 1e6, ms * 1e6 / per_simd);
    (void)hipFree(d);
}
static void fold_gate()
{
    // round 19 (profiles/r19a_vertex_octets.txt): the fold on images of 8 and 16 positions beside rounds 13 and 18, in one run
    for (int rep = 0; rep < 2; ++rep)
        for (int wps = 4; wps <= 8; wps += 4) {
            run_fold<0>("fold, point pairs (6:1, LDS)", wps); run_fold<1>("fold, vertex quads V=4 (8:1, LDS)", wps);
            run_fold<2>("fold, vertex octets V=8 (LDS)", wps); run_fold<4>("fold, groups of 16 V=16 (LDS)", wps);
        }
}
int main(int argc, char **argv)
{
    if (argc > 1 && argv[1][0] == 'f') { fold_gate(); return 0; }      // "fold": the round-19 gate alone
    run<0>("v_add_f32 2src"); run<1>("v_fma_f32 3src"); run<17>("v_sub_f32"); run<6>("v_min_f32"); run<5>("v_min3_f32");
    run<2>("v_pk_fma_f16 3src"); run<7>("v_pk_fma_f16 (acc in src2)"); run<8>("v_pk_fma_f16 op_sel splat"); run<3>("v_pk_min_f16"); run<4>("v_pk_add_f16");
    run<12>("v_pk_mul_f16"); run<10>("v_pk_max_f16 neg (abs)"); run<9>("v_pk_min_i16"); run<14>("v_pk_min_u16"); run<11>("v_and_b32"); run<15>("v_min_u32"); run<16>("v_min_f16");
    run<13>("v_cmp_gt_f32"); run<18>("v_dot2_f32_f16");
    run<20>("v_min3_f16"); run<29>("v_min3_f16 abs op_sel"); run<21>("v_sub_f16"); run<22>("v_pk_minimum3_f16"); run<23>("v_minimum3_f32"); run<24>("v_min3_u16"); run<25>("v_min3_u32");
    run<26>("v_or3_b32"); run<27>("v_sad_u16"); run<28>("v_cvt_pkrtz_f16_f32"); run<30>("v_med3_f32"); run<31>("v_sub_u16"); run<32>("v_sub_u32"); run<33>("v_pk_sub_u16"); run<34>("v_min_u16"); run<35>("v_max_f16");
    run<0>("v_add_f32 2src (again)");
    // round 11 (profiles/r11a_pair_gap.txt): the pair gap | |m - h| - w |
    run<17>("v_sub_f32 (again)"); run<40>("v_sub_f32_e64 |a|, b"); run<41>("v_sub_f32 -> v_sub_f32_e64 |.|", 2); run<42>("v_fma_f32 |a|, 1.0, -b");
    run_mix<0>("level 0 until round 10 (2:1)", 4, 3, 2); run_mix<1>("level 0 on pairs, sub (4:1)", 4, 5, 4); run_mix<2>("level 0 on pairs, fma (4:1)", 4, 5, 4);
    run_mix<0>("level 0 until round 10 (2:1)", 8, 3, 2); run_mix<1>("level 0 on pairs, sub (4:1)", 8, 5, 4);
    // round 13 (profiles/r13a_point_pairs.txt): the quad gap | |m - hm| - hw | - w, three dependent subtracts, two with |.| on a source
    run<17>("v_sub_f32 (again)"); run<43>("v_sub -> v_sub_e64 |.| -> v_sub_e64 |.|", 3);
    run_mix<1>("level 0 on pairs, sub (4:1)", 4, 5, 4); run_mix<3>("level 0 on point pairs (6:1)", 4, 7, 8);
    run_mix<1>("level 0 on pairs, sub (4:1)", 8, 5, 4); run_mix<3>("level 0 on point pairs (6:1)", 8, 7, 8);
    // round 18 (profiles/r18a_vertex_quads.txt): the oct gap | | |mm - hm| - hw'| - ww | - ws, four dependent subtracts, and the
    // block's fold from LDS tiles beside round 13's in the same run
    run<17>("v_sub_f32 (again)"); run<43>("v_sub -> 2 x v_sub_e64 |.|", 3); run<44>("v_sub -> 3 x v_sub_e64 |.|", 4);
    for (int rep = 0; rep < 2; ++rep) {
        run_fold<0>("fold, point pairs (6:1, LDS)", 4); run_fold<1>("fold, vertex quads (8:1, LDS)", 4);
        run_fold<0>("fold, point pairs (6:1, LDS)", 8); run_fold<1>("fold, vertex quads (8:1, LDS)", 8);
    }
    fold_gate();
    return 0;
}
